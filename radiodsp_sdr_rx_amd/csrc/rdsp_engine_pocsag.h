/*
 * rdsp_engine_pocsag.h -- what the POCSAG kernel (rdsp_engine_pocsag.hip) and its owner on the host (EngPocsag,
 * rdsp_engine_pocsag_host.hip) share: the kernel's arguments and its launch.  The arithmetic is rdsp_pocsag.h's, include/rdsp.h
 * has the definition.
 */
#ifndef RDSP_ENGINE_POCSAG_H
#define RDSP_ENGINE_POCSAG_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rdsp_pocsag.h"

namespace rdsp_eng {

/* one NFM group's channel range in a call: the kernel stands behind the group's other detector kernels and only reads the audio */
struct PocsagParams {
  const float *audio; size_t audio_stride; /* [ch][t]: the demodulated rows the group's FM kernel wrote (16-byte aligned rows) */
  int n_channels, n_blocks;
  int reset;                               /* the group's pending RESET_FM: the words are read as zeros */
  rdsp_pocsag::PocsagLaw law;              /* of the group's settings, baud != 0 */
  uint32_t *state;                         /* [ch][POCSAG_WORDS] */
  uint8_t *sync, *fresh, *bad; float *lvl, *dc; size_t rec_stride; /* the call's records, [ch][max_blocks] */
};

}  // namespace rdsp_eng

/* stream-ordered */
hipError_t rdsp_engine_pocsag_launch(const rdsp_eng::PocsagParams &p, hipStream_t s);

#endif
