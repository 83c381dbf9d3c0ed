/* rdsp_engine_meter_host.hip -- the signal meter, the squelch, the active-receiver list and the packed audio of the open
 * receivers of rdsp_engine_t on the host: EngMeter (rdsp_engine_host.h) owns the buffers and makes the launches; the entry
 * points check their arguments.  include/rdsp.h has the definition; the kernels are rdsp_engine_meter.hip's and
 * rdsp_engine_pack.hip's, the arithmetic rdsp_meter.h's. */
#include "rdsp_engine_host.h"

hipError_t EngMeter::init(size_t n, size_t blocks_per_call) {
  n_channels = n; max_blocks = blocks_per_call;
  const size_t rec = n * max_blocks;
  hipError_t err = alloc_zero(words, n * MT_WORDS);
  if (err == hipSuccess) err = alloc_zero(level, rec);
  if (err == hipSuccess) err = alloc_zero(peak, rec);
  if (err == hipSuccess) err = alloc_zero(open, rec);
  if (err == hipSuccess) err = alloc_zero(list, n);
  if (err == hipSuccess) err = alloc_zero(count, 1);
  return err;
}
hipError_t EngMeter::reset(hipStream_t s) { return hipMemsetAsync(words, 0, n_channels * MT_WORDS * 4, s); }
hipError_t EngMeter::launch_group(const EngParams &p, size_t c0, const rdsp_meter::MeterSet &set, const int16_t *d_lr, hipStream_t s) const {
  MeterParams mp;
  mp.audio = p.audio; mp.audio_stride = p.audio_stride; mp.out = p.out; mp.out_stride = p.out_stride;
  mp.out_vec = ((uintptr_t)d_lr & 15) == 0 && p.out_stride % 4 == 0;
  mp.n_channels = p.n_channels; mp.n_blocks = p.n_blocks; mp.words = words + c0 * MT_WORDS;
  mp.rec_stride = max_blocks;
  mp.level = level + c0 * mp.rec_stride; mp.peak = peak + c0 * mp.rec_stride; mp.open = open + c0 * mp.rec_stride;
  mp.set = set;
  return rdsp_engine_meter_launch(mp, s);
}
hipError_t EngMeter::launch_list(int n_blocks, hipStream_t s) {
  blocks = n_blocks;
  return rdsp_engine_active_launch(ActiveParams{words, (int)n_channels, list, count}, s);
}
hipError_t EngMeter::launch_pack(PackParams p, hipStream_t s) const {
  p.n_channels = (int)n_channels; p.open = open; p.rec_stride = max_blocks; p.offset = pack_offset;
  return rdsp_engine_pack_launch(p, s);
}

namespace {
/* n_blocks of the last call's max_blocks-wide rows into the caller's rows, stream-ordered; a NULL destination is skipped */
hipError_t copy_rows(void *dst, size_t dst_stride, const void *src, size_t src_stride, size_t width, size_t rows, size_t size, hipStream_t s) {
  if (!dst || width == 0) return hipSuccess;
  return hipMemcpy2DAsync(dst, dst_stride * size, src, src_stride * size, width * size, rows, hipMemcpyDeviceToDevice, s);
}
}  // namespace

extern "C" {

int rdsp_engine_enable_meter(rdsp_engine_t *e) {
  if (!e) return RDSP_ERR_INVALID;
  if (e->meter) return RDSP_OK;
  auto m = std::make_unique<EngMeter>(); /* the object stays without a meter unless all of it exists */
  hipError_t err = hipSetDevice(e->device);
  if (err == hipSuccess) err = hipDeviceSynchronize(); /* the next call of every stream runs with the meter */
  if (err == hipSuccess) err = m->init((size_t)e->n_channels, (size_t)e->max_blocks);
  if (err == hipSuccess) err = hipDeviceSynchronize();
  if (err != hipSuccess) {
    rdsp_set_error("rdsp_engine_enable_meter: %s", hipGetErrorString(err));
    return RDSP_ERR_NOMEM;
  }
  e->meter = std::move(m);
  return RDSP_OK;
}
int rdsp_engine_meter_enabled(const rdsp_engine_t *e) { return e && e->meter ? 1 : 0; }

int rdsp_engine_set_meter(rdsp_engine_t *e, float attack, float decay) {
  if (!e || !rdsp_meter::coefficients_ok(attack, decay)) {
    rdsp_set_error("rdsp_engine_set_meter: bad argument (attack %g and decay %g must lie in (0, 1])", (double)attack, (double)decay);
    return RDSP_ERR_INVALID;
  }
  return for_selected(e, [&](EngSettings &s) { s.meter.attack = attack; s.meter.decay = decay; });
}
int rdsp_engine_set_squelch(rdsp_engine_t *e, float open_ms, float close_ms, int hang_blocks) {
  if (!e || !rdsp_meter::squelch_ok(open_ms, close_ms, hang_blocks)) {
    rdsp_set_error("rdsp_engine_set_squelch: bad argument (0 <= close_ms %g <= open_ms %g, both finite; hang_blocks %d of 0 .. %d)",
                   (double)close_ms, (double)open_ms, hang_blocks, rdsp_meter::HANG_MAX);
    return RDSP_ERR_INVALID;
  }
  return for_selected(e, [&](EngSettings &s) {
    s.meter.squelch = 1; s.meter.open_ms = open_ms; s.meter.close_ms = close_ms; s.meter.hang_blocks = hang_blocks;
  });
}
int rdsp_engine_disable_squelch(rdsp_engine_t *e) { return for_selected(e, [](EngSettings &s) { s.meter.squelch = 0; }); }

int rdsp_engine_read_meter(rdsp_engine_t *e, int n_blocks, float *d_level, size_t level_stride, float *d_peak, size_t peak_stride,
                           uint8_t *d_open, size_t open_stride, void *stream) {
  if (!e) return RDSP_ERR_INVALID;
  if (no_meter(e, "rdsp_engine_read_meter")) return RDSP_ERR_NOT_READY;
  const size_t w = (size_t)std::max(n_blocks, 0);
  if (n_blocks < 0 || n_blocks > e->meter->blocks || (d_level && level_stride < w) || (d_peak && peak_stride < w) || (d_open && open_stride < w)) {
    rdsp_set_error("rdsp_engine_read_meter: bad argument (n_blocks %d of the last call's %d; strides at least n_blocks)", n_blocks, e->meter->blocks);
    return RDSP_ERR_INVALID;
  }
  const EngMeter &m = *e->meter;
  const size_t n = (size_t)e->n_channels, rs = (size_t)e->max_blocks;
  hipStream_t s = (hipStream_t)stream;
  hipError_t err = hipSetDevice(e->device);
  if (err == hipSuccess) err = copy_rows(d_level, level_stride, m.level, rs, w, n, 4, s);
  if (err == hipSuccess) err = copy_rows(d_peak, peak_stride, m.peak, rs, w, n, 4, s);
  if (err == hipSuccess) err = copy_rows(d_open, open_stride, m.open, rs, w, n, 1, s);
  return err == hipSuccess ? RDSP_OK : engine_fail("rdsp_engine_read_meter", err);
}

int rdsp_engine_active(rdsp_engine_t *e, int32_t *d_list, int32_t *d_count, void *stream) {
  if (!e) return RDSP_ERR_INVALID;
  if (no_meter(e, "rdsp_engine_active")) return RDSP_ERR_NOT_READY;
  hipStream_t s = (hipStream_t)stream;
  hipError_t err = hipSetDevice(e->device);
  if (err == hipSuccess && d_list) err = hipMemcpyAsync(d_list, e->meter->list, (size_t)e->n_channels * 4, hipMemcpyDeviceToDevice, s);
  if (err == hipSuccess && d_count) err = hipMemcpyAsync(d_count, e->meter->count, 4, hipMemcpyDeviceToDevice, s);
  return err == hipSuccess ? RDSP_OK : engine_fail("rdsp_engine_active", err);
}

int rdsp_engine_pack_active(rdsp_engine_t *e, const int16_t *d_lr, size_t out_stride, int n_blocks, int16_t *d_audio,
                            rdsp_pack_record_t *d_records, size_t capacity_blocks, int32_t *d_counts, void *stream) {
  if (!e) return RDSP_ERR_INVALID;
  if (no_meter(e, "rdsp_engine_pack_active")) return RDSP_ERR_NOT_READY;
  EngMeter &m = *e->meter;
  if (!d_lr || !d_counts || n_blocks < 0 || n_blocks > m.blocks || out_stride < (size_t)std::max(n_blocks, 0) * BS ||
      (capacity_blocks > 0 && (!d_audio || !d_records)) || ((uintptr_t)d_audio & 15) != 0 || capacity_blocks > (size_t)INT32_MAX ||
      (size_t)e->n_channels * (size_t)std::max(n_blocks, 0) > (size_t)INT32_MAX) {
    rdsp_set_error("rdsp_engine_pack_active: bad argument (d_lr and d_counts not NULL; n_blocks %d of the last call's %d; out_stride at least "
                   "n_blocks * 128; d_audio 16-byte aligned, and d_records, not NULL with a capacity; capacity_blocks %zu at most INT32_MAX)",
                   n_blocks, m.blocks, capacity_blocks);
    return RDSP_ERR_INVALID;
  }
  hipStream_t s = (hipStream_t)stream;
  hipError_t err = hipSetDevice(e->device);
  if (err != hipSuccess) return engine_fail("rdsp_engine_pack_active", err);
  if (n_blocks == 0) { /* also: no call yet */
    err = hipMemsetAsync(d_counts, 0, 2 * sizeof(int32_t), s);
    return err == hipSuccess ? RDSP_OK : engine_fail("rdsp_engine_pack_active", err);
  }
  if (!m.pack_offset) { /* the first pack call: an engine that meters and never packs allocates nothing for it */
    DevBuf<int32_t> b;
    if ((err = b.alloc((size_t)e->n_channels)) != hipSuccess) {
      b.p = nullptr;
      rdsp_set_error("rdsp_engine_pack_active: %s", hipGetErrorString(err));
      return RDSP_ERR_NOMEM;
    }
    std::swap(m.pack_offset.p, b.p);
  }
  PackParams p{};
  p.lr = (const int32_t *)d_lr; p.lr_stride = out_stride; p.lr_vec = ((uintptr_t)d_lr & 15) == 0 && out_stride % 4 == 0;
  p.n_blocks = n_blocks; p.audio = d_audio; p.records = (int2 *)d_records; p.capacity = (int)capacity_blocks; p.counts = d_counts;
  err = m.launch_pack(p, s);
  return err == hipSuccess ? RDSP_OK : engine_fail("rdsp_engine_pack_active", err);
}

int rdsp_engine_get_meter(rdsp_engine_t *e, float *host_out, void *stream) {
  if (!e || !host_out) return RDSP_ERR_INVALID;
  if (no_meter(e, "rdsp_engine_get_meter")) return RDSP_ERR_NOT_READY;
  std::vector<float> w((size_t)e->n_channels * MT_WORDS);
  hipError_t err = hipSetDevice(e->device);
  if (err == hipSuccess) err = hipMemcpyAsync(w.data(), e->meter->words, w.size() * 4, hipMemcpyDeviceToHost, (hipStream_t)stream);
  if (err == hipSuccess) err = hipStreamSynchronize((hipStream_t)stream);
  if (err != hipSuccess) return engine_fail("rdsp_engine_get_meter", err);
  for (int c = 0; c < e->n_channels; c++) {
    const float *m = &w[(size_t)c * MT_WORDS];
    float *o = host_out + (size_t)c * 4;
    o[0] = m[MT_LEVEL]; o[1] = m[MT_LAST_MS]; o[2] = m[MT_LAST_PK]; o[3] = (float)f_bits(m[MT_OPEN]);
  }
  return RDSP_OK;
}

int rdsp_engine_read_demod(rdsp_engine_t *e, int n_blocks, float *d_out, size_t out_stride, void *stream) {
  if (!e || !d_out || n_blocks < 0 || n_blocks > e->last_blocks || out_stride < (size_t)n_blocks * BS) {
    rdsp_set_error("rdsp_engine_read_demod: bad argument (n_blocks %d of the last call's %d; out_stride at least n_blocks * 128)",
                   n_blocks, e ? e->last_blocks : 0);
    return RDSP_ERR_INVALID;
  }
  hipError_t err = hipSetDevice(e->device);
  if (err == hipSuccess)
    err = copy_rows(d_out, out_stride, e->d_audio, (size_t)e->max_blocks * BS, (size_t)n_blocks * BS, (size_t)e->n_channels, 4, (hipStream_t)stream);
  return err == hipSuccess ? RDSP_OK : engine_fail("rdsp_engine_read_demod", err);
}

}  // extern "C"
