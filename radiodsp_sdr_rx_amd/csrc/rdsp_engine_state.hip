/*
 * rdsp_engine_state.hip -- the signal state of a channel range of rdsp_engine_t as data: resume, or move receivers between
 * objects / GPUs.  Blob = header {magic, version, n_channels, flags} + per channel: the 96 state words, the last 512 samples
 * of both lines of the side-band network in time order (whatever the ring's size and position here or there), the blanker's
 * lines, the ALS filter's line and taps; then one array per optional part of the engine, in flag order: each channel's tuning
 * phase accumulator of an engine with sources (rdsp_engine_set_sources), {level, open, hang} per channel of one with the
 * meter, the last 60 left words per channel of one with the voice-rate audio, the 50 detector words per channel of one with
 * narrow-band FM (rdsp_engine_enable_fm), the 8 tone-detector words per channel of one with the tone squelch
 * (rdsp_engine_enable_tone), the 200 tone-search words per channel of one with the tone search (rdsp_engine_enable_tone_search),
 * the 232 code-squelch words per channel of one with the code squelch (rdsp_engine_enable_dcs),
 * the 68 noise-squelch words per channel of one with the noise squelch (rdsp_engine_enable_noise),
 * the 168 DTMF words per channel of one with the DTMF decoder (rdsp_engine_enable_dtmf),
 * the 448 AFSK words per channel of one with the AFSK 1200 decoder (rdsp_engine_enable_afsk),
 * the 456 POCSAG words per channel of one with the POCSAG decoder (rdsp_engine_enable_pocsag).  Settings are not part of it (they belong to the group the channels land in).  The blob of an engine without a part
 * is as it was before the part existed (no flag, nothing appended).
 */
#include <array>

#include "rdsp_engine_host.h"

namespace {
constexpr uint32_t STATE_MAGIC = 0x45534452u; /* "RDSE" */
constexpr uint32_t STATE_PHASES = 1u, STATE_METER = 2u, STATE_VOICE = 4u, STATE_FM = 8u, STATE_TONE = 16u, STATE_SEARCH = 32u, STATE_DCS = 64u, STATE_NOISE = 128u, STATE_DTMF = 256u, STATE_AFSK = 512u, STATE_POCSAG = 1024u;
/* where a channel's planes lie in its blob words: whole, but of a ring its last RING_KEPT samples in time order */
constexpr size_t RING_KEPT = 512;
constexpr size_t BLOB_OFF[N_PLANES] = {0, NF, NF + RING_KEPT, NF + 2 * RING_KEPT, NF + 2 * RING_KEPT + NB_WORDS};
constexpr size_t STATE_CH_WORDS = BLOB_OFF[PL_ALS] + ALS_WORDS;
/* an optional part: the first blob_words of every channel's dev_words on the device (dev: the owner's words; null: the engine
 * has no such part), in the blob under a header flag; needs: what load_state asks for when only the blob has the part */
struct StatePart { uint32_t flag; size_t dev_words, blob_words; float *dev; const char *needs; };
constexpr int N_PARTS = 11; /* in flag order, which is their order in the blob */
using StateParts = std::array<StatePart, N_PARTS>;
StateParts state_parts(const rdsp_engine_t *e) {
  return {{{STATE_PHASES, 1, 1, e && e->src ? (float *)e->src->phase.p : nullptr, "tuning phases; call rdsp_engine_set_sources"},
           {STATE_METER, MT_WORDS, MT_STATE_WORDS, e && e->meter ? e->meter->words.p : nullptr, "meter state; call rdsp_engine_enable_meter"},
           {STATE_VOICE, rdsp_voice::VOICE_HIST, rdsp_voice::VOICE_HIST, e && e->voice ? (float *)e->voice->hist.p : nullptr,
            "voice history; call rdsp_engine_enable_voice"},
           {STATE_FM, rdsp_fm::FM_STATE_WORDS, rdsp_fm::FM_STATE_WORDS, e && e->fm ? (float *)e->fm->state.p : nullptr,
            "FM detector state; call rdsp_engine_enable_fm"},
           {STATE_TONE, rdsp_tone::TONE_WORDS, rdsp_tone::TONE_WORDS, e && e->tone ? (float *)e->tone->state.p : nullptr,
            "tone detector state; call rdsp_engine_enable_tone"},
           {STATE_SEARCH, rdsp_tone_search::SEARCH_WORDS, rdsp_tone_search::SEARCH_WORDS, e && e->search ? (float *)e->search->state.p : nullptr,
            "tone search state; call rdsp_engine_enable_tone_search"},
           {STATE_DCS, rdsp_dcs::DCS_WORDS, rdsp_dcs::DCS_WORDS, e && e->dcs ? (float *)e->dcs->state.p : nullptr,
            "code squelch state; call rdsp_engine_enable_dcs"},
           {STATE_NOISE, rdsp_noise::NOISE_WORDS, rdsp_noise::NOISE_WORDS, e && e->noise ? (float *)e->noise->state.p : nullptr,
            "noise squelch state; call rdsp_engine_enable_noise"},
           {STATE_DTMF, rdsp_dtmf::DTMF_WORDS, rdsp_dtmf::DTMF_WORDS, e && e->dtmf ? (float *)e->dtmf->state.p : nullptr,
            "DTMF decoder state; call rdsp_engine_enable_dtmf"},
           {STATE_AFSK, rdsp_afsk::AFSK_WORDS, rdsp_afsk::AFSK_WORDS, e && e->afsk ? (float *)e->afsk->state.p : nullptr,
            "AFSK decoder state; call rdsp_engine_enable_afsk"},
           {STATE_POCSAG, rdsp_pocsag::POCSAG_WORDS, rdsp_pocsag::POCSAG_WORDS, e && e->pocsag ? (float *)e->pocsag->state.p : nullptr,
            "POCSAG decoder state; call rdsp_engine_enable_pocsag"}}};
}
/* the flags of a blob the engine writes (its own parts), or with all = true every flag a blob may carry */
uint32_t state_flags(const StateParts &parts, bool all = false) {
  uint32_t f = 0;
  for (const StatePart &p : parts) f |= all || p.dev ? p.flag : 0;
  return f;
}
/* the one size formula: a blob of n channels whose header carries `flags` */
size_t blob_bytes(const StateParts &parts, uint32_t flags, size_t n) {
  size_t words = STATE_CH_WORDS;
  for (const StatePart &p : parts) words += flags & p.flag ? p.blob_words : 0;
  return 16 + n * words * 4;
}
struct StateImage { /* host images of n channels: the planes, and the parts the engine has */
  std::vector<float> plane[N_PLANES], part[N_PARTS];
  StateImage(const rdsp_engine_t *e, const StateParts &parts, size_t n) {
    for (int k = 0; k < N_PLANES; k++) plane[k].assign(n * e->plane_words[k], 0.0f);
    for (int k = 0; k < N_PARTS; k++) part[k].assign(parts[k].dev ? n * parts[k].dev_words : 0, 0.0f);
  }
};
/* channels c0 .. c0 + n - 1 between the device and the image, then the stream drained */
hipError_t image_copy(rdsp_engine_t *e, const StateParts &parts, StateImage &im, bool save, size_t c0, size_t n, hipStream_t s) {
  const hipMemcpyKind kind = save ? hipMemcpyDeviceToHost : hipMemcpyHostToDevice;
  auto copy = [&](void *dev, void *host, size_t bytes) { return hipMemcpyAsync(save ? host : dev, save ? dev : host, bytes, kind, s); };
  hipError_t err = hipSetDevice(e->device);
  for (int k = 0; k < N_PARTS && err == hipSuccess; k++)
    if (const StatePart &p = parts[k]; p.dev) err = copy(p.dev + c0 * p.dev_words, im.part[k].data(), n * p.dev_words * 4);
  for (int k = 0; k < N_PLANES && err == hipSuccess; k++) err = copy(e->plane[k] + c0 * e->plane_words[k], im.plane[k].data(), im.plane[k].size() * 4);
  if (err == hipSuccess) err = hipStreamSynchronize(s);
  return err;
}
/* the words w of a blob with `flags` (n channels from first_channel on) from the image, or the image from them */
void blob_move(const rdsp_engine_t *e, const StateParts &parts, StateImage &im, bool save, uint32_t flags, int first_channel, size_t n, float *w) {
  for (size_t c = 0; c < n; c++, w += STATE_CH_WORDS) {
    const uint32_t pos = e->grp[(size_t)group_of(e->first, first_channel + (int)c)].pos;
    for (int k = 0; k < N_PLANES; k++) {
      float *b = w + BLOB_OFF[k], *h = &im.plane[k][c * e->plane_words[k]];
      if (k != PL_RING_I && k != PL_RING_Q) { memcpy(save ? b : h, save ? h : b, e->plane_words[k] * 4); continue; }
      for (uint32_t i = 0; i < RING_KEPT; i++) { /* sample pos - 512 + i */
        float &x = h[(pos - (uint32_t)RING_KEPT + i) & (e->ring_size - 1)];
        if (save) b[i] = x;
        else x = b[i];
      }
    }
  }
  for (int k = 0; k < N_PARTS; k++) { /* after the last channel's words: the array of every part the blob has */
    const StatePart &p = parts[k];
    for (size_t c = 0; (flags & p.flag) && c < n; c++, w += p.blob_words) {
      float *h = &im.part[k][c * p.dev_words];
      memcpy(save ? w : h, save ? h : w, p.blob_words * 4);
    }
  }
}
}  // namespace

extern "C" {

size_t rdsp_engine_state_bytes(const rdsp_engine_t *e, int n_channels) {
  const StateParts parts = state_parts(e);
  return (e && n_channels > 0) ? blob_bytes(parts, state_flags(parts), (size_t)n_channels) : 0;
}
int rdsp_engine_save_state(rdsp_engine_t *e, int first_channel, int n_channels, void *host_buf, size_t bytes, void *stream) {
  if (!e || !host_buf || first_channel < 0 || n_channels < 1 || first_channel + n_channels > e->n_channels ||
      bytes < rdsp_engine_state_bytes(e, n_channels)) {
    rdsp_set_error("rdsp_engine_save_state: bad argument");
    return RDSP_ERR_INVALID;
  }
  const size_t n = (size_t)n_channels;
  const StateParts parts = state_parts(e);
  StateImage im(e, parts, n);
  const hipError_t err = image_copy(e, parts, im, true, (size_t)first_channel, n, (hipStream_t)stream);
  if (err != hipSuccess) return engine_fail("rdsp_engine_save_state", err);
  uint32_t *hdr = (uint32_t *)host_buf;
  hdr[0] = STATE_MAGIC; hdr[1] = 1; hdr[2] = (uint32_t)n_channels; hdr[3] = state_flags(parts);
  blob_move(e, parts, im, true, hdr[3], first_channel, n, (float *)(hdr + 4));
  return RDSP_OK;
}
int rdsp_engine_load_state(rdsp_engine_t *e, int first_channel, const void *host_buf, size_t bytes, void *stream) {
  const uint32_t *hdr = (const uint32_t *)host_buf;
  const StateParts parts = state_parts(e);
  if (!e || !host_buf || bytes < 16 || hdr[0] != STATE_MAGIC || hdr[1] != 1 || (hdr[3] & ~state_flags(parts, true)) != 0) {
    rdsp_set_error("rdsp_engine_load_state: not an engine state blob of this version");
    return RDSP_ERR_INVALID;
  }
  const size_t n = hdr[2], c0 = (size_t)first_channel;
  if (first_channel < 0 || n < 1 || c0 + n > (size_t)e->n_channels || bytes < blob_bytes(parts, hdr[3], n)) {
    rdsp_set_error("rdsp_engine_load_state: %zu channels at %d do not fit", n, first_channel);
    return RDSP_ERR_INVALID;
  }
  for (const StatePart &p : parts)
    if ((hdr[3] & p.flag) && !p.dev) {
      rdsp_set_error("rdsp_engine_load_state: the blob carries %s first", p.needs);
      return RDSP_ERR_NOT_READY;
    }
  /* zeros: the rings outside the kept samples, the phases of a blob from an engine that never tuned, the meter words of one
   * that never metered (and always those of the last call: they are no state), the voice history of one without the stage, the
   * detector words of one without FM, the tone words of one without the tone squelch, the search words of one without the
   * tone search, the code-squelch words of one without the code squelch, the noise-squelch words of one without the noise squelch (which
   * restarts the detector closed: a zero key is no key), the DTMF words of one without the DTMF decoder, the AFSK words of one without the AFSK decoder, the POCSAG words of one without the POCSAG decoder */
  e->event_blocks = 0; /* the decoders' words are no longer what the last call's records tell of */
  StateImage im(e, parts, n);
  blob_move(e, parts, im, false, hdr[3], first_channel, n, (float *)(hdr + 4)); /* read only: save is false */
  const hipError_t err = image_copy(e, parts, im, false, c0, n, (hipStream_t)stream);
  return err == hipSuccess ? RDSP_OK : engine_fail("rdsp_engine_load_state", err);
}

}  // extern "C"
