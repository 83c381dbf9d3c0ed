/*
 * rdsp_engine_afsk.h -- what the AFSK 1200 kernel (rdsp_engine_afsk.hip) and its owner on the host (EngAfsk,
 * rdsp_engine_afsk_host.hip) share: the kernel's arguments and its launch.  The arithmetic is rdsp_afsk.h's, include/rdsp.h has
 * the definition.
 */
#ifndef RDSP_ENGINE_AFSK_H
#define RDSP_ENGINE_AFSK_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rdsp_afsk.h"

namespace rdsp_eng {

/* one NFM group's channel range in a call: the kernel stands behind the group's other detector kernels and only reads the audio */
struct AfskParams {
  const float *audio; size_t audio_stride; /* [ch][t]: the demodulated rows the group's FM kernel wrote (16-byte aligned rows) */
  int n_channels, n_blocks;
  int reset;                               /* the group's pending RESET_FM: the words are read as zeros */
  rdsp_afsk::AfskLaw law;                  /* of the group's settings, on == 1 */
  const float4 *tab;                       /* [TUNE_N], rdsp_tune.h's table */
  uint32_t *state;                         /* [ch][AFSK_WORDS] */
  uint8_t *sync, *fresh, *bad; float *lvl; size_t rec_stride; /* the call's records, [ch][max_blocks]: sync_rec, new_rec, bad_rec, lvl_rec */
};

}  // namespace rdsp_eng

/* stream-ordered */
hipError_t rdsp_engine_afsk_launch(const rdsp_eng::AfskParams &p, hipStream_t s);

#endif
