/*
 * rdsp_events.h -- the definition of rdsp_engine_gather_events (include/rdsp.h, "decoder events"), shared by the kernels
 * (rdsp_engine_events.hip), the host entry points (rdsp_engine_events_host.hip) and the host program of the tests
 * (tests/host/host_events_check.cpp).  Integers only.  It needs nothing but the C library: the places of the count words and the
 * rings are restated here, and rdsp_engine_events_host.hip holds them to rdsp_dtmf.h, rdsp_afsk.h and rdsp_pocsag.h.
 *
 * Per channel and kind (DTMF 0, AFSK 1, POCSAG 2), `new` the kind's record of the last call as its read call returns it:
 *   c = the blocks with new != 255 (DTMF), the sum of new (AFSK, POCSAG); n = the detector's count word; R = 16, 4, 4
 *   take = min(c, R), lost = c - take; the items are seq = n - take ... n - 1, oldest first, item seq in ring slot seq mod R
 *   an item's payload is the used part of its slot: 1 word (DTMF), 2 + ceil(len / 4) words (AFSK), 4 + n_cw words (POCSAG)
 * The events run by channel, then kind, then seq; an event's offset is the sum of the n_words of all before it.  c <= n holds
 * behind every update; where it does not, take is n (the items the ring can have) and the pair is counted as a violation.
 */
#ifndef RDSP_EVENTS_H
#define RDSP_EVENTS_H

#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RDSP_EV_HD __host__ __device__ inline
#else
#define RDSP_EV_HD inline
#endif

namespace rdsp_events {

constexpr int KINDS = 3;
enum { EV_DTMF = 0, EV_AFSK = 1, EV_POCSAG = 2 };
constexpr int SLOT_MAX = 84;               /* the words of an AFSK or POCSAG ring slot */
constexpr int AFSK_MAX_LEN = 328, POCSAG_MAX_CW = 80;
constexpr int CHANNEL_MAX_WORDS = 16 + 4 * SLOT_MAX + 4 * SLOT_MAX; /* 688: what one channel can contribute */

/* a kind's detector words: how many a channel has, where the count word and the ring are, the ring's slots and a slot's words */
struct Layout {
  int words, count, ring, slots, slot_words;
};
RDSP_EV_HD constexpr Layout layout(int kind) {
  return kind == EV_DTMF ? Layout{168, 6, 16, 16, 1} : kind == EV_AFSK ? Layout{448, 10, 112, 4, SLOT_MAX} : Layout{456, 13, 120, 4, SLOT_MAX};
}
/* the payload's words of the item in `slot` (its header word is slot[0]): never more than the slot has */
RDSP_EV_HD uint32_t payload_words(int kind, uint32_t head) {
  if (kind == EV_DTMF) return 1u;
  if (kind == EV_AFSK) return 2u + ((head < (uint32_t)AFSK_MAX_LEN ? head : (uint32_t)AFSK_MAX_LEN) + 3u) / 4u;
  const uint32_t n_cw = head & 0xFFu;
  return 4u + (n_cw < (uint32_t)POCSAG_MAX_CW ? n_cw : (uint32_t)POCSAG_MAX_CW);
}
/* what a block's record counts */
RDSP_EV_HD uint32_t record_count(int kind, uint8_t rec) { return kind == EV_DTMF ? (rec != 255u ? 1u : 0u) : (uint32_t)rec; }
/* c and n -> take (clamped to n: never an item the ring cannot have) and lost */
RDSP_EV_HD void take_of(uint32_t c, uint32_t n, uint32_t R, uint32_t &take, uint32_t &lost) {
  take = c < R ? c : R;
  lost = c - take;
  if (take > n) take = n;
}
/* does event k, n_words long at `offset`, lie inside the capacities */
RDSP_EV_HD bool fits(uint32_t k, uint32_t offset, uint32_t n_words, uint32_t capacity_events, uint32_t capacity_words) {
  return k < capacity_events && offset <= capacity_words && n_words <= capacity_words - offset;
}

struct Record {
  int32_t channel;
  uint32_t kind_words, seq, offset; /* kind | n_words << 8 */
};
static_assert(sizeof(Record) == 16, "rdsp_event_record_t");

/* the plain loop, which is the definition.  fresh[k]: kind k's record [n_channels][stride], state[k]: its detector words
 * [n_channels][layout(k).words]; either NULL: the kind is off.  counts[5] = needed_events, written_events, needed_words,
 * written_words, lost.  Returns the number of (channel, kind) pairs with c > n (0 behind every update). */
inline int events_reference(const uint8_t *const fresh[KINDS], size_t stride, const uint32_t *const state[KINDS], int n_channels, int n_blocks,
                            Record *records, size_t capacity_events, uint32_t *words, size_t capacity_words, int32_t counts[5]) {
  uint32_t k = 0, offset = 0, lost_sum = 0, written_events = 0, written_words = 0;
  bool open = true; /* every event so far was written */
  int violations = 0;
  for (int ch = 0; ch < n_channels; ch++) {
    for (int kind = 0; kind < KINDS; kind++) {
      if (!fresh[kind] || !state[kind]) continue;
      const Layout l = layout(kind);
      const uint8_t *rec = fresh[kind] + (size_t)ch * stride;
      const uint32_t *w = state[kind] + (size_t)ch * (size_t)l.words;
      uint32_t c = 0;
      for (int b = 0; b < n_blocks; b++) c += record_count(kind, rec[b]);
      const uint32_t n = w[l.count];
      uint32_t take, lost;
      take_of(c, n, (uint32_t)l.slots, take, lost);
      if (c > n) violations++;
      lost_sum += lost;
      for (uint32_t seq = n - take; seq != n; seq++) {
        const uint32_t *slot = w + l.ring + (size_t)(seq % (uint32_t)l.slots) * (size_t)l.slot_words;
        const uint32_t n_words = payload_words(kind, slot[0]);
        if (open && fits(k, offset, n_words, (uint32_t)capacity_events, (uint32_t)capacity_words)) {
          records[k] = Record{ch, (uint32_t)kind | n_words << 8, seq, offset};
          memcpy(words + offset, slot, (size_t)n_words * 4);
          written_events = k + 1u;
          written_words = offset + n_words;
        } else {
          open = false;
        }
        k++;
        offset += n_words;
      }
    }
  }
  counts[0] = (int32_t)k; counts[1] = (int32_t)written_events; counts[2] = (int32_t)offset; counts[3] = (int32_t)written_words; counts[4] = (int32_t)lost_sum;
  return violations;
}
}  // namespace rdsp_events

#endif
