/*
 * rdsp_engine_dcs.h -- what the code-squelch kernel (rdsp_engine_dcs.hip) and its owner on the host (EngDcs,
 * rdsp_engine_dcs_host.hip) share: the kernel's arguments and its launch.  The arithmetic is rdsp_dcs.h's, include/rdsp.h has
 * the definition.
 */
#ifndef RDSP_ENGINE_DCS_H
#define RDSP_ENGINE_DCS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rdsp_dcs.h"

namespace rdsp_eng {

/* one NFM group's channel range in a call: the kernel stands behind the group's tone-squelch kernel (behind its meter kernel
 * without one, behind its tail kernel without either) */
struct DcsParams {
  const float *audio; size_t audio_stride; /* [ch][t]: the demodulated rows the group's FM kernel wrote (16-byte aligned rows) */
  int32_t *out; size_t out_stride;         /* [ch][t] words: the audio behind the group's tail kernel, meter and tone squelch */
  int out_vec;                             /* the rows of out are 16-byte aligned */
  int n_channels, n_blocks;
  int reset;                               /* the group's pending RESET_FM: the words are read as zeros */
  rdsp_dcs::DcsLaw law;                    /* of the group's settings */
  const uint32_t *sel;                     /* [ch]: dcs_sel of the channel's code, 0: none */
  uint32_t *state;                         /* [ch][DCS_WORDS] */
  uint8_t *dcs, *hits; uint32_t *word; size_t rec_stride; /* the call's records, [ch][max_blocks] */
  /* the meter's, null without one (then nothing is gated): its open records of the call [ch][open_stride] and its words, of
   * which MT_ANY is rewritten */
  uint8_t *open; size_t open_stride;
  float *meter_words;
};

}  // namespace rdsp_eng

/* stream-ordered */
hipError_t rdsp_engine_dcs_launch(const rdsp_eng::DcsParams &p, hipStream_t s);

#endif
