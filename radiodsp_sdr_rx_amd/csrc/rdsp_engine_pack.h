/*
 * rdsp_engine_pack.h -- what the pack kernels (rdsp_engine_pack.hip) and their owner on the host (EngMeter,
 * rdsp_engine_meter_host.hip) share: the kernels' arguments and the one launch.  include/rdsp.h has the definition.
 */
#ifndef RDSP_ENGINE_PACK_H
#define RDSP_ENGINE_PACK_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rdsp_eng {

/* one rdsp_engine_pack_active call, every channel of the object */
struct PackParams {
  const int32_t *lr; size_t lr_stride; /* [ch][t] words {L, R}: the caller's rows, as the last update wrote them */
  int lr_vec;                          /* the rows of lr are 16-byte aligned */
  int n_channels, n_blocks;
  const uint8_t *open; size_t rec_stride; /* the last call's gate records, [ch][max_blocks] */
  int32_t *offset;                     /* [ch] scratch: a channel's count of open blocks, then the index of its first packed block */
  int16_t *audio;                      /* [capacity][128], 16-byte aligned */
  int2 *records;                       /* [capacity] {channel, block} */
  int capacity;                        /* 0: counts only */
  int32_t *counts;                     /* [2]: needed, written */
};

}  // namespace rdsp_eng

/* stream-ordered: count, scan and -- with a capacity -- gather */
hipError_t rdsp_engine_pack_launch(const rdsp_eng::PackParams &p, hipStream_t s);

#endif
