/*
 * rdsp_engine_tone.h -- what the tone-squelch kernel (rdsp_engine_tone.hip) and its owner on the host (EngTone,
 * rdsp_engine_tone_host.hip) share: the kernel's arguments and its launch.  The arithmetic is rdsp_tone.h's, include/rdsp.h has
 * the definition.
 */
#ifndef RDSP_ENGINE_TONE_H
#define RDSP_ENGINE_TONE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rdsp_tone.h"

namespace rdsp_eng {

/* one NFM group's channel range in a call: the kernel stands behind the group's meter kernel (behind its tail kernel without a meter) */
struct ToneParams {
  const float *audio; size_t audio_stride; /* [ch][t]: the demodulated rows the group's FM kernel wrote (16-byte aligned rows) */
  int32_t *out; size_t out_stride;         /* [ch][t] words: the audio behind the group's tail kernel and meter */
  int out_vec;                             /* the rows of out are 16-byte aligned */
  int n_channels, n_blocks;
  int reset;                               /* the group's pending RESET_FM: the words are read as zeros */
  rdsp_tone::ToneLaw law;                  /* of the group's settings */
  const uint32_t *dphi;                    /* [ch]: the channel's step, 0: no tone */
  const float4 *tab;                       /* [TUNE_N], rdsp_tune.h's table */
  uint32_t *state;                         /* [ch][TONE_WORDS] */
  float *a2; uint8_t *tone; size_t rec_stride; /* the call's records, [ch][max_blocks] */
  /* the meter's, null without one (then nothing is gated): its open records of the call [ch][open_stride] and its words, of
   * which MT_ANY is rewritten */
  uint8_t *open; size_t open_stride;
  float *meter_words;
};

}  // namespace rdsp_eng

/* stream-ordered */
hipError_t rdsp_engine_tone_launch(const rdsp_eng::ToneParams &p, hipStream_t s);

#endif
