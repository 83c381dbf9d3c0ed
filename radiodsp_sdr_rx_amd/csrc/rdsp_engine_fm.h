/*
 * rdsp_engine_fm.h -- what the narrow-band FM kernel (rdsp_engine_fm.hip) and its owner on the host (EngFm,
 * rdsp_engine_fm_host.hip) share: the kernel's arguments and its launch.  The arithmetic is rdsp_fm.h's, include/rdsp.h has the
 * definition.
 */
#ifndef RDSP_ENGINE_FM_H
#define RDSP_ENGINE_FM_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rdsp_fm.h"

namespace rdsp_eng {

/* one NFM group's channel range in a call: the kernel stands where the front and Hilbert kernels stand for the other modes */
struct FmParams {
  const int32_t *iq; size_t in_stride;  /* [ch][t] words: I | Q << 16, the rows rdsp_engine_update was handed */
  int in_vec;                           /* the rows of iq are 16-byte aligned */
  int n_channels, n_blocks;
  int W, deemph, reset;                 /* reset: the group's pending RESET_FM -- the state is read as zeros */
  float k, a;                           /* rdsp_fm.h's fm_scale and fm_deemph_a of the group's settings */
  const float *taps;                    /* [16 W] of the group's W, read-only for the launch */
  uint32_t *state;                      /* [ch][FM_STATE_WORDS] */
  float *audio; size_t audio_stride;    /* [ch][t]: y, the engine's demodulated rows (16-byte aligned rows) */
  float *level; size_t level_stride;    /* [ch][t]: lvl, what an NFM group's meter measures (16-byte aligned rows) */
};

}  // namespace rdsp_eng

/* stream-ordered */
hipError_t rdsp_engine_fm_launch(const rdsp_eng::FmParams &p, hipStream_t s);

#endif
