/*
 * rdsp_engine_events.h -- what the event kernels (rdsp_engine_events.hip) and their owner on the host (EngEvents,
 * rdsp_engine_events_host.hip) share: the kernels' arguments and the one launch.  include/rdsp.h has the definition,
 * rdsp_events.h its plain loop.
 */
#ifndef RDSP_ENGINE_EVENTS_H
#define RDSP_ENGINE_EVENTS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rdsp_events.h"

namespace rdsp_eng {

/* one rdsp_engine_gather_events call, every channel of the object */
struct EventsParams {
  const uint32_t *state[rdsp_events::KINDS]; /* [ch][the kind's words]; NULL: the decoder is off */
  const uint8_t *fresh[rdsp_events::KINDS];  /* the last call's `new` records, [ch][rec_stride] */
  const uint8_t *ran;                        /* [kind][ch] scratch: 1 where the kind's decoder ran on the channel in the last call */
  size_t rec_stride;
  int n_channels, n_blocks;
  int4 *chan;                                /* [ch] scratch: {events, words, lost, takes}, then {first event, first word, lost, takes} */
  int4 *records;                             /* [capacity_events], 16-byte aligned */
  uint32_t *words;                           /* [capacity_words], 16-byte aligned */
  int capacity_events, capacity_words;       /* capacity_events 0: counts only */
  int32_t *counts;                           /* [5]: needed_events, written_events, needed_words, written_words, lost */
};

}  // namespace rdsp_eng

/* stream-ordered: count, scan and -- with a capacity -- gather */
hipError_t rdsp_engine_events_launch(const rdsp_eng::EventsParams &p, hipStream_t s);

#endif
