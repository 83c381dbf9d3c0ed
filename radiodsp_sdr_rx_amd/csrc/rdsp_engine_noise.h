/*
 * rdsp_engine_noise.h -- what the noise-squelch kernel (rdsp_engine_noise.hip) and its owner on the host (EngNoise,
 * rdsp_engine_noise_host.hip) share: the kernel's arguments and its launch.  The arithmetic is rdsp_noise.h's, include/rdsp.h has
 * the definition.
 */
#ifndef RDSP_ENGINE_NOISE_H
#define RDSP_ENGINE_NOISE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rdsp_noise.h"

namespace rdsp_eng {

/* one NFM group's channel range in a call: the kernel stands behind the group's meter kernel (behind its tail kernel without a
 * meter), in front of its tone kernel.  The group's mode is 1 or 2 */
struct NoiseParams {
  const float *audio; size_t audio_stride; /* [ch][t]: the demodulated rows the group's FM kernel wrote (16-byte aligned rows) */
  int32_t *out; size_t out_stride;         /* [ch][t] words: the audio behind the group's tail kernel and meter */
  int out_vec;                             /* the rows of out are 16-byte aligned */
  int n_channels, n_blocks;
  int reset;                               /* the group's pending RESET_FM: the words are read as those of another key */
  uint32_t key;                            /* noise_key of the group's mode, W and tau_us */
  rdsp_noise::NoiseSet set;                /* the group's settings */
  uint32_t *state;                         /* [ch][NOISE_WORDS] */
  float *noise; uint8_t *nopen; size_t rec_stride; /* the call's records, [ch][max_blocks] */
  /* the meter's, null without one or at mode 1 (then nothing is gated): its open records of the call [ch][open_stride] and its
   * words, of which MT_ANY is rewritten */
  uint8_t *open; size_t open_stride;
  float *meter_words;
  float taps[rdsp_noise::NOISE_TAPS + 3];  /* noise_taps of the group's tau_us, by value: kernel arguments are read with scalar loads */
};

}  // namespace rdsp_eng

/* stream-ordered */
hipError_t rdsp_engine_noise_launch(const rdsp_eng::NoiseParams &p, hipStream_t s);

#endif
