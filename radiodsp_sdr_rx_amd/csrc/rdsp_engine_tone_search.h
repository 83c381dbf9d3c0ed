/*
 * rdsp_engine_tone_search.h -- what the tone-search kernel (rdsp_engine_tone_search.hip) and its owner on the host
 * (EngToneSearch, rdsp_engine_tone_search_host.hip) share: the kernel's arguments and its launch.  The arithmetic is
 * rdsp_tone_search.h's, include/rdsp.h has the definition.
 */
#ifndef RDSP_ENGINE_TONE_SEARCH_H
#define RDSP_ENGINE_TONE_SEARCH_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rdsp_tone_search.h"

namespace rdsp_eng {

/* one NFM group's channel range in a call: the kernel stands behind the group's tone-squelch kernel and only reads the audio */
struct ToneSearchParams {
  const float *audio; size_t audio_stride; /* [ch][t]: the demodulated rows the group's FM kernel wrote (16-byte aligned rows) */
  int n_channels, n_blocks;
  int reset;                               /* the group's pending RESET_FM: the words are read as zeros */
  rdsp_tone_search::SearchLaw law;         /* of the group's settings, K > 0 */
  uint32_t n_tones, bank_key;              /* of the engine's bank */
  const uint32_t *dphi;                    /* [MAX_TONES]: the bank's steps, zeros from n_tones on */
  const float4 *tab;                       /* [TUNE_N], rdsp_tune.h's table */
  uint32_t *state;                         /* [ch][SEARCH_WORDS] */
  uint8_t *best; float *a2, *next; size_t rec_stride; /* the call's records, [ch][max_blocks] */
};

}  // namespace rdsp_eng

/* stream-ordered */
hipError_t rdsp_engine_tone_search_launch(const rdsp_eng::ToneSearchParams &p, hipStream_t s);

#endif
