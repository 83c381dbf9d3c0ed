/* rdsp_engine_voice_host.hip -- the voice-rate audio of rdsp_engine_t on the host: EngVoice (rdsp_engine_host.h) owns the
 * history, the taps and the decimated rows and makes the launch; the entry points check their arguments.  include/rdsp.h has
 * the definition; the kernels are rdsp_engine_voice.hip's, the arithmetic rdsp_voice.h's.  rdsp_engine_pack_voice runs the
 * pack's own count and scan (EngMeter::launch_pack without a capacity), then the gather over the voice rows. */
#include "rdsp_engine_host.h"

using rdsp_voice::VOICE_HIST;

hipError_t EngVoice::init(size_t n, size_t max_blocks, int rate) {
  n_channels = n; R = rate; row_words = max_blocks * BS / (size_t)R;
  int32_t q[rdsp_voice::TAPS_PER_PHASE * rdsp_voice::MAX_R];
  uint32_t pairs[rdsp_voice::TAPS_PER_PHASE * rdsp_voice::MAX_R];
  rdsp_voice::voice_taps(R, q);
  rdsp_voice::voice_tap_pairs(R, q, pairs);
  hipError_t err = alloc_zero(hist, n * VOICE_HIST);
  if (err == hipSuccess) err = alloc_zero(rows, n * row_words);
  if (err == hipSuccess) err = taps.alloc((size_t)rdsp_voice::TAPS_PER_PHASE * R);
  if (err == hipSuccess) err = hipMemcpy(taps, pairs, (size_t)rdsp_voice::TAPS_PER_PHASE * R * 4, hipMemcpyHostToDevice);
  return err;
}
hipError_t EngVoice::reset(hipStream_t s) { return hipMemsetAsync(hist, 0, n_channels * VOICE_HIST * 4, s); }
hipError_t EngVoice::launch(const int16_t *d_lr, size_t out_stride, int n_blocks, hipStream_t s) {
  VoiceParams p{};
  p.lr = (const int32_t *)d_lr; p.lr_stride = out_stride; p.lr_vec = ((uintptr_t)d_lr & 15) == 0 && out_stride % 4 == 0;
  p.n_channels = (int)n_channels; p.n_blocks = n_blocks; p.R = R; p.tap_pairs = taps; p.hist = hist; p.rows = rows; p.row_stride = row_words;
  blocks = n_blocks;
  return rdsp_engine_voice_launch(p, s);
}

namespace {
bool no_voice(const rdsp_engine_t *e, const char *who) {
  if (!e->voice) rdsp_set_error("%s: the voice-rate audio is off; call rdsp_engine_enable_voice first", who);
  return !e->voice;
}
}  // namespace

extern "C" {

int rdsp_engine_voice_taps(int R, int32_t *out) {
  if (!rdsp_voice::rate_ok(R) || !out) {
    rdsp_set_error("rdsp_engine_voice_taps: bad argument (R %d of 2 or 4, out not NULL)", R);
    return RDSP_ERR_INVALID;
  }
  rdsp_voice::voice_taps(R, out);
  return RDSP_OK;
}

int rdsp_engine_enable_voice(rdsp_engine_t *e, int R) {
  if (!e || !rdsp_voice::rate_ok(R) || (e->voice && e->voice->R != R)) {
    rdsp_set_error("rdsp_engine_enable_voice: bad argument (R %d of 2 or 4; one R per engine, here %d)", R, e && e->voice ? e->voice->R : 0);
    return RDSP_ERR_INVALID;
  }
  if (e->voice) return RDSP_OK;
  auto v = std::make_unique<EngVoice>(); /* the object stays without the stage unless all of it exists */
  hipError_t err = hipSetDevice(e->device);
  if (err == hipSuccess) err = hipDeviceSynchronize(); /* the next call of every stream runs with the stage */
  if (err == hipSuccess) err = v->init((size_t)e->n_channels, (size_t)e->max_blocks, R);
  if (err == hipSuccess) err = hipDeviceSynchronize();
  if (err != hipSuccess) {
    rdsp_set_error("rdsp_engine_enable_voice: %s", hipGetErrorString(err));
    return RDSP_ERR_NOMEM;
  }
  e->voice = std::move(v);
  return RDSP_OK;
}
int rdsp_engine_voice_rate(const rdsp_engine_t *e) { return e && e->voice ? e->voice->R : 0; }

int rdsp_engine_read_voice(rdsp_engine_t *e, int n_blocks, int16_t *d_out, size_t out_stride, void *stream) {
  if (!e) return RDSP_ERR_INVALID;
  if (no_voice(e, "rdsp_engine_read_voice")) return RDSP_ERR_NOT_READY;
  const EngVoice &v = *e->voice;
  const size_t width = (size_t)std::max(n_blocks, 0) * BS / (size_t)v.R;
  if (!d_out || n_blocks < 0 || n_blocks > v.blocks || out_stride < width) {
    rdsp_set_error("rdsp_engine_read_voice: bad argument (d_out not NULL; n_blocks %d of the last call's %d; out_stride at least n_blocks * 128 / %d)",
                   n_blocks, v.blocks, v.R);
    return RDSP_ERR_INVALID;
  }
  if (width == 0) return RDSP_OK;
  hipError_t err = hipSetDevice(e->device);
  if (err == hipSuccess)
    err = hipMemcpy2DAsync(d_out, out_stride * 2, v.rows, v.row_words * 2, width * 2, (size_t)e->n_channels, hipMemcpyDeviceToDevice, (hipStream_t)stream);
  return err == hipSuccess ? RDSP_OK : engine_fail("rdsp_engine_read_voice", err);
}

int rdsp_engine_pack_voice(rdsp_engine_t *e, int n_blocks, int16_t *d_audio, rdsp_pack_record_t *d_records, size_t capacity_blocks,
                           int32_t *d_counts, void *stream) {
  if (!e) return RDSP_ERR_INVALID;
  if (no_meter(e, "rdsp_engine_pack_voice") || no_voice(e, "rdsp_engine_pack_voice")) return RDSP_ERR_NOT_READY;
  EngMeter &m = *e->meter;
  const EngVoice &v = *e->voice;
  if (!d_counts || n_blocks < 0 || n_blocks > m.blocks || n_blocks > v.blocks || (capacity_blocks > 0 && (!d_audio || !d_records)) ||
      ((uintptr_t)d_audio & 15) != 0 || capacity_blocks > (size_t)INT32_MAX || (size_t)e->n_channels * (size_t)std::max(n_blocks, 0) > (size_t)INT32_MAX) {
    rdsp_set_error("rdsp_engine_pack_voice: bad argument (d_counts not NULL; n_blocks %d of the last call's %d; d_audio 16-byte aligned, and "
                   "d_records, not NULL with a capacity; capacity_blocks %zu at most INT32_MAX)", n_blocks, std::min(m.blocks, v.blocks), capacity_blocks);
    return RDSP_ERR_INVALID;
  }
  hipStream_t s = (hipStream_t)stream;
  hipError_t err = hipSetDevice(e->device);
  if (err != hipSuccess) return engine_fail("rdsp_engine_pack_voice", err);
  if (n_blocks == 0) { /* also: no call yet */
    err = hipMemsetAsync(d_counts, 0, 2 * sizeof(int32_t), s);
    return err == hipSuccess ? RDSP_OK : engine_fail("rdsp_engine_pack_voice", err);
  }
  if (!m.pack_offset) { /* the pack's scratch, as rdsp_engine_pack_active's first call allocates it */
    DevBuf<int32_t> b;
    if ((err = b.alloc((size_t)e->n_channels)) != hipSuccess) {
      b.p = nullptr;
      rdsp_set_error("rdsp_engine_pack_voice: %s", hipGetErrorString(err));
      return RDSP_ERR_NOMEM;
    }
    std::swap(m.pack_offset.p, b.p);
  }
  PackParams c{}; /* count and scan: counts = {needed, 0}, offset[ch] = the channel's first packed block */
  c.n_blocks = n_blocks; c.counts = d_counts;
  err = m.launch_pack(c, s);
  if (err == hipSuccess && capacity_blocks > 0) {
    VoicePackParams p{};
    p.rows = v.rows; p.row_stride = v.row_words; p.n_channels = e->n_channels; p.n_blocks = n_blocks; p.R = v.R;
    p.open = m.open; p.rec_stride = m.max_blocks; p.offset = m.pack_offset;
    p.audio = d_audio; p.records = (int2 *)d_records; p.capacity = (int)capacity_blocks; p.counts = d_counts;
    err = rdsp_engine_voice_gather_launch(p, s);
  }
  return err == hipSuccess ? RDSP_OK : engine_fail("rdsp_engine_pack_voice", err);
}

}  // extern "C"
