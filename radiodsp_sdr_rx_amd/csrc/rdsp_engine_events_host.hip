/* rdsp_engine_events_host.hip -- rdsp_engine_gather_events on the host: EngEvents (rdsp_engine_host.h) owns the call's scratch
 * and makes the launch; the entry points check their arguments.  include/rdsp.h has the definition, rdsp_events.h its plain loop
 * (exported as rdsp_events_reference); the kernels are rdsp_engine_events.hip's.  It reads the decoders' words, records and rows
 * (EngDtmf, EngAfsk, EngPocsag) and writes nothing of the engine but the scratch. */
#include "rdsp_engine_host.h"

using namespace rdsp_events;

/* rdsp_events.h restates the places it reads: they are the decoders' */
static_assert(layout(EV_DTMF).words == rdsp_dtmf::DTMF_WORDS && layout(EV_DTMF).count == rdsp_dtmf::DT_NDIGITS && layout(EV_DTMF).ring == rdsp_dtmf::DT_RING &&
              layout(EV_DTMF).slots == rdsp_dtmf::RING, "rdsp_dtmf.h");
static_assert(layout(EV_AFSK).words == rdsp_afsk::AFSK_WORDS && layout(EV_AFSK).count == rdsp_afsk::AF_NFRAMES && layout(EV_AFSK).ring == rdsp_afsk::AF_RING &&
              layout(EV_AFSK).slots == rdsp_afsk::RING && layout(EV_AFSK).slot_words == rdsp_afsk::SLOT_WORDS && AFSK_MAX_LEN == 4 * rdsp_afsk::SLOT_DATA,
              "rdsp_afsk.h");
static_assert(layout(EV_POCSAG).words == rdsp_pocsag::POCSAG_WORDS && layout(EV_POCSAG).count == rdsp_pocsag::PG_NMSGS &&
              layout(EV_POCSAG).ring == rdsp_pocsag::PG_RING && layout(EV_POCSAG).slots == rdsp_pocsag::RING &&
              layout(EV_POCSAG).slot_words == rdsp_pocsag::SLOT_WORDS && POCSAG_MAX_CW == rdsp_pocsag::MSG_MAX, "rdsp_pocsag.h");
/* the gather's 16-byte loads: a ring slot of 84 words starts on a 16-byte boundary */
static_assert(layout(EV_AFSK).words % 4 == 0 && layout(EV_AFSK).ring % 4 == 0 && layout(EV_POCSAG).words % 4 == 0 && layout(EV_POCSAG).ring % 4 == 0 &&
              SLOT_MAX % 4 == 0, "16-byte slots");
static_assert(sizeof(rdsp_event_record_t) == sizeof(Record) && RDSP_EVENT_DTMF == EV_DTMF && RDSP_EVENT_AFSK == EV_AFSK && RDSP_EVENT_POCSAG == EV_POCSAG,
              "include/rdsp.h");

hipError_t EngEvents::init(size_t n) {
  n_channels = n;
  hipError_t err = chan.alloc(n);
  if (err == hipSuccess) err = ran.alloc((size_t)KINDS * n);
  return err;
}
hipError_t EngEvents::launch(const rdsp_engine *e, EventsParams p, hipStream_t s) {
  using Rows = std::vector<std::pair<size_t, size_t>>;
  const Rows *rows[KINDS] = {nullptr, nullptr, nullptr};
  if (e->dtmf) { p.state[EV_DTMF] = e->dtmf->state; p.fresh[EV_DTMF] = e->dtmf->fresh; rows[EV_DTMF] = &e->dtmf->rows; }
  if (e->afsk) { p.state[EV_AFSK] = e->afsk->state; p.fresh[EV_AFSK] = e->afsk->fresh; rows[EV_AFSK] = &e->afsk->rows; }
  if (e->pocsag) { p.state[EV_POCSAG] = e->pocsag->state; p.fresh[EV_POCSAG] = e->pocsag->fresh; rows[EV_POCSAG] = &e->pocsag->rows; }
  /* the record buffers keep an earlier call's values for receivers a decoder did not run on: only its rows count, as in its
   * read call */
  hipError_t err = hipMemsetAsync(ran, 0, (size_t)KINDS * n_channels, s);
  for (int k = 0; k < KINDS && err == hipSuccess; k++)
    for (size_t r = 0; rows[k] && r < rows[k]->size() && err == hipSuccess; r++)
      err = hipMemsetAsync(ran + (size_t)k * n_channels + (*rows[k])[r].first, 1, (*rows[k])[r].second, s);
  if (err != hipSuccess) return err;
  p.ran = ran; p.chan = chan; p.rec_stride = (size_t)e->max_blocks; p.n_channels = e->n_channels;
  return rdsp_engine_events_launch(p, s);
}

/* what both entry points refuse, but for the alignment of device buffers */
static bool events_args_bad(int n_channels, const void *records, size_t capacity_events, const void *words, size_t capacity_words, const int32_t *counts) {
  return !counts || (capacity_events > 0 && !records) || (capacity_words > 0 && !words) || capacity_events > (size_t)INT32_MAX ||
         capacity_words > (size_t)INT32_MAX || n_channels < 0 || (size_t)n_channels * (size_t)CHANNEL_MAX_WORDS > (size_t)INT32_MAX;
}

extern "C" {

int rdsp_engine_gather_events(rdsp_engine_t *e, rdsp_event_record_t *d_records, size_t capacity_events, uint32_t *d_words, size_t capacity_words,
                              int32_t *d_counts, void *stream) {
  if (!e) return RDSP_ERR_INVALID;
  if (!e->dtmf && !e->afsk && !e->pocsag) {
    rdsp_set_error("rdsp_engine_gather_events: no decoder is on; call rdsp_engine_enable_dtmf, rdsp_engine_enable_afsk or rdsp_engine_enable_pocsag first");
    return RDSP_ERR_NOT_READY;
  }
  if (events_args_bad(e->n_channels, d_records, capacity_events, d_words, capacity_words, d_counts) || ((uintptr_t)d_records & 15) != 0 ||
      ((uintptr_t)d_words & 15) != 0) {
    rdsp_set_error("rdsp_engine_gather_events: bad argument (d_counts not NULL; d_records and d_words 16-byte aligned, and not NULL with a capacity; "
                   "capacity_events %zu and capacity_words %zu at most INT32_MAX; %d channels of at most %d)", capacity_events, capacity_words,
                   e->n_channels, INT32_MAX / CHANNEL_MAX_WORDS);
    return RDSP_ERR_INVALID;
  }
  hipStream_t s = (hipStream_t)stream;
  hipError_t err = hipSetDevice(e->device);
  if (err != hipSuccess) return engine_fail("rdsp_engine_gather_events", err);
  if (e->event_blocks == 0) { /* no call yet, a call of no blocks, or the words are no longer the last call's */
    err = hipMemsetAsync(d_counts, 0, 5 * sizeof(int32_t), s);
    return err == hipSuccess ? RDSP_OK : engine_fail("rdsp_engine_gather_events", err);
  }
  if (!e->events) { /* the first gather: an engine that decodes and never gathers allocates nothing for it */
    auto t = std::make_unique<EngEvents>();
    if ((err = t->init((size_t)e->n_channels)) != hipSuccess) {
      rdsp_set_error("rdsp_engine_gather_events: %s", hipGetErrorString(err));
      return RDSP_ERR_NOMEM;
    }
    e->events = std::move(t);
  }
  EventsParams p{};
  p.n_blocks = e->event_blocks; p.records = (int4 *)d_records; p.words = d_words; p.capacity_events = (int)capacity_events;
  p.capacity_words = (int)capacity_words; p.counts = d_counts;
  err = e->events->launch(e, p, s);
  return err == hipSuccess ? RDSP_OK : engine_fail("rdsp_engine_gather_events", err);
}

int rdsp_events_reference(const uint8_t *new_dtmf, const uint8_t *new_afsk, const uint8_t *new_pocsag, size_t new_stride, const uint32_t *dtmf_words,
                          const uint32_t *afsk_words, const uint32_t *pocsag_words, int n_channels, int n_blocks, rdsp_event_record_t *records,
                          size_t capacity_events, uint32_t *words, size_t capacity_words, int32_t *counts) {
  if (events_args_bad(n_channels, records, capacity_events, words, capacity_words, counts) || n_blocks < 0 || new_stride < (size_t)std::max(n_blocks, 0)) {
    rdsp_set_error("rdsp_events_reference: bad argument (counts not NULL; records and words not NULL with a capacity; capacities at most INT32_MAX; "
                   "%d channels of at most %d; new_stride at least n_blocks %d)", n_channels, INT32_MAX / CHANNEL_MAX_WORDS, n_blocks);
    return RDSP_ERR_INVALID;
  }
  const uint8_t *const fresh[KINDS] = {new_dtmf, new_afsk, new_pocsag};
  const uint32_t *const state[KINDS] = {dtmf_words, afsk_words, pocsag_words};
  return events_reference(fresh, new_stride, state, n_channels, n_blocks, (Record *)records, capacity_events, words, capacity_words, counts);
}

}  // extern "C"
