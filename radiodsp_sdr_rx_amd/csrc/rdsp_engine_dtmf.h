/*
 * rdsp_engine_dtmf.h -- what the DTMF kernel (rdsp_engine_dtmf.hip) and its owner on the host (EngDtmf,
 * rdsp_engine_dtmf_host.hip) share: the kernel's arguments and its launch.  The arithmetic is rdsp_dtmf.h's, include/rdsp.h has
 * the definition.
 */
#ifndef RDSP_ENGINE_DTMF_H
#define RDSP_ENGINE_DTMF_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rdsp_dtmf.h"

namespace rdsp_eng {

/* one NFM group's channel range in a call: the kernel stands behind the group's other detector kernels and only reads the audio */
struct DtmfParams {
  const float *audio; size_t audio_stride; /* [ch][t]: the demodulated rows the group's FM kernel wrote (16-byte aligned rows) */
  int n_channels, n_blocks;
  int reset;                               /* the group's pending RESET_FM: the words are read as zeros */
  rdsp_dtmf::DtmfLaw law;                  /* of the group's settings, K > 0 */
  const float4 *tab;                       /* [TUNE_N], rdsp_tune.h's table */
  uint32_t *state;                         /* [ch][DTMF_WORDS] */
  uint8_t *key, *fresh; float *lo, *hi; size_t rec_stride; /* the call's records, [ch][max_blocks]: key_rec, new_rec, lo_rec, hi_rec */
};

}  // namespace rdsp_eng

/* stream-ordered */
hipError_t rdsp_engine_dtmf_launch(const rdsp_eng::DtmfParams &p, hipStream_t s);

#endif
