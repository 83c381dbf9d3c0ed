/*
 * rdsp_engine_voice.h -- what the voice-rate kernels (rdsp_engine_voice.hip) and their owner on the host (EngVoice,
 * rdsp_engine_voice_host.hip) share: the kernels' arguments and the two launches.  The arithmetic is rdsp_voice.h's,
 * include/rdsp.h has the definition.
 */
#ifndef RDSP_ENGINE_VOICE_H
#define RDSP_ENGINE_VOICE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rdsp_voice.h"

namespace rdsp_eng {

/* the stage of one call, every channel of the object */
struct VoiceParams {
  const int32_t *lr; size_t lr_stride; /* [ch][t] words {L, R}: the caller's rows as the call leaves them (behind the gate) */
  int lr_vec;                          /* the rows of lr are 16-byte aligned */
  int n_channels, n_blocks, R;
  const int32_t *tap_pairs;            /* [16][R / 2][2] words of rdsp_voice.h's voice_tap_pairs, read-only for the launch */
  int32_t *hist;                       /* [ch][VOICE_HIST] left words, oldest first */
  int16_t *rows; size_t row_stride;    /* [ch][max_blocks 128 / R]: the engine's voice rows */
};
/* the gather of one rdsp_engine_pack_voice call, behind the pack's count and scan (rdsp_engine_pack.h) */
struct VoicePackParams {
  const int16_t *rows; size_t row_stride;
  int n_channels, n_blocks, R;
  const uint8_t *open; size_t rec_stride; /* the last call's gate records, [ch][max_blocks] */
  const int32_t *offset;                  /* [ch]: the index of the channel's first packed block (the scan's) */
  int16_t *audio;                         /* [capacity][128 / R], 16-byte aligned */
  int2 *records;                          /* [capacity] {channel, block} */
  int capacity;                           /* above 0 */
  int32_t *counts;                        /* [2]: needed (the scan's), written (set here) */
};

}  // namespace rdsp_eng

/* stream-ordered */
hipError_t rdsp_engine_voice_launch(const rdsp_eng::VoiceParams &p, hipStream_t s);
hipError_t rdsp_engine_voice_gather_launch(const rdsp_eng::VoicePackParams &p, hipStream_t s);

#endif
