/*
 * rdsp_engine_meter.h -- what the meter's kernels (rdsp_engine_meter.hip) and their owner on the host (EngMeter,
 * rdsp_engine_meter_host.hip) share: the kernels' arguments, a channel's meter words, the two launches.  The arithmetic is rdsp_meter.h's.
 */
#ifndef RDSP_ENGINE_METER_H
#define RDSP_ENGINE_METER_H

#include <hip/hip_runtime.h>

#include "rdsp_meter.h"

namespace rdsp_eng {

/* per-channel meter words, floats (ints bit-cast): [channel][MT_WORDS].  The first three are signal state (a state blob
 * carries them); the others belong to the last call: the last block's mean square and peak, and whether the gate was open
 * in any of its blocks (what the active list is made of) */
enum { MT_LEVEL = 0, MT_OPEN, MT_HANG, MT_LAST_MS, MT_LAST_PK, MT_ANY, MT_WORDS = 8 };
constexpr int MT_STATE_WORDS = 3;

/* one group's channel range in a call */
struct MeterParams {
  const float *audio; size_t audio_stride; /* [ch][t]: the demodulated rows the group's front / Hilbert kernel wrote */
  int32_t *out; size_t out_stride;         /* [ch][t] words: the audio the group's tail kernel wrote */
  int out_vec;                             /* the rows of out are 16-byte aligned */
  int n_channels, n_blocks;
  float *words;                            /* [ch][MT_WORDS] */
  float *level, *peak; uint8_t *open; size_t rec_stride; /* the call's records, [ch][max_blocks] */
  rdsp_meter::MeterSet set;
};
/* the active list of a call, every channel of the object */
struct ActiveParams {
  const float *words;
  int n_channels;
  int32_t *list, *count;
};

}  // namespace rdsp_eng

/* stream-ordered; the meter behind the group's tail kernel, the list once behind every group's meter */
hipError_t rdsp_engine_meter_launch(const rdsp_eng::MeterParams &p, hipStream_t s);
hipError_t rdsp_engine_active_launch(const rdsp_eng::ActiveParams &p, hipStream_t s);

#endif
