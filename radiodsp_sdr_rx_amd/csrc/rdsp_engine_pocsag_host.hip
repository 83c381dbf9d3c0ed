/* rdsp_engine_pocsag_host.hip -- the POCSAG pager decoder of rdsp_engine_t on the host: EngPocsag (rdsp_engine_host.h) owns the
 * detector words and the records and makes the launch; the entry points check their arguments.  include/rdsp.h has the
 * definition; the kernel is rdsp_engine_pocsag.hip's, the arithmetic rdsp_pocsag.h's.  rdsp_engine_update launches it per NFM
 * group with a paging baud rate behind the group's other detectors. */
#include "rdsp_engine_host.h"

using namespace rdsp_pocsag;

hipError_t EngPocsag::init(size_t n, size_t blocks_per_call) {
  n_channels = n; max_blocks = blocks_per_call;
  hipError_t err = alloc_zero(state, n * POCSAG_WORDS);
  if (err == hipSuccess) err = alloc_zero(sync, n * max_blocks);
  if (err == hipSuccess) err = alloc_zero(fresh, n * max_blocks);
  if (err == hipSuccess) err = alloc_zero(bad, n * max_blocks);
  if (err == hipSuccess) err = alloc_zero(lvl, n * max_blocks);
  if (err == hipSuccess) err = alloc_zero(dc, n * max_blocks);
  return err;
}
hipError_t EngPocsag::reset(hipStream_t s) { return hipMemsetAsync(state, 0, n_channels * POCSAG_WORDS * 4, s); }
hipError_t EngPocsag::launch_group(const EngParams &p, size_t c0, const PocsagSet &set, hipStream_t s) {
  PocsagParams t{};
  t.audio = p.audio; t.audio_stride = p.audio_stride;
  t.n_channels = p.n_channels; t.n_blocks = p.n_blocks; t.reset = (p.resets & RESET_FM) != 0;
  t.law = pocsag_law(set);
  t.state = state + c0 * POCSAG_WORDS;
  t.rec_stride = max_blocks; t.sync = sync + c0 * max_blocks; t.fresh = fresh + c0 * max_blocks; t.bad = bad + c0 * max_blocks;
  t.lvl = lvl + c0 * max_blocks; t.dc = dc + c0 * max_blocks;
  const hipError_t err = rdsp_engine_pocsag_launch(t, s);
  if (err == hipSuccess) rows.emplace_back(c0, (size_t)p.n_channels); /* only rows a launch wrote are read_pocsag's */
  return err;
}
hipError_t EngPocsag::clear_group(size_t c0, size_t count, hipStream_t s) {
  return hipMemsetAsync(state + c0 * POCSAG_WORDS, 0, count * POCSAG_WORDS * 4, s);
}

extern "C" {

const uint16_t *rdsp_engine_pocsag_bch_table(void) { return pocsag_table().e; }

uint32_t rdsp_engine_pocsag_codeword(uint32_t data21) { return pocsag_codeword(data21); }

int rdsp_engine_enable_pocsag(rdsp_engine_t *e) {
  if (!e) return RDSP_ERR_INVALID;
  if (e->pocsag) return RDSP_OK;
  if (!e->fm) {
    rdsp_set_error("rdsp_engine_enable_pocsag: the POCSAG decoder runs on narrow-band FM receivers; call rdsp_engine_enable_fm first");
    return RDSP_ERR_NOT_READY;
  }
  auto t = std::make_unique<EngPocsag>(); /* the object stays without the decoder unless all of it exists */
  hipError_t err = hipSetDevice(e->device);
  if (err == hipSuccess) err = hipDeviceSynchronize(); /* the next call of every stream may run it */
  if (err == hipSuccess) err = t->init((size_t)e->n_channels, (size_t)e->max_blocks);
  if (err == hipSuccess) err = hipDeviceSynchronize();
  if (err != hipSuccess) {
    rdsp_set_error("rdsp_engine_enable_pocsag: %s", hipGetErrorString(err));
    return RDSP_ERR_NOMEM;
  }
  e->pocsag = std::move(t);
  return RDSP_OK;
}
int rdsp_engine_pocsag_enabled(const rdsp_engine_t *e) { return e && e->pocsag ? 1 : 0; }

int rdsp_engine_set_pocsag(rdsp_engine_t *e, int baud, int invert, int pull, int sync_errs, int fix_addr, int fix_data) {
  if (!e || !pocsag_ok(baud, invert, pull, sync_errs, fix_addr, fix_data)) {
    rdsp_set_error("rdsp_engine_set_pocsag: bad argument (baud %d of 0, 512, 1200, 2400; invert %d of 0 .. 2; pull %d of 1 .. 4; sync_errs %d of 0 .. 3; "
                   "fix_addr %d, fix_data %d of 0 .. 2)", baud, invert, pull, sync_errs, fix_addr, fix_data);
    return RDSP_ERR_INVALID;
  }
  return for_selected(e, [&](EngSettings &s) { s.pocsag = {baud, invert, pull, sync_errs, fix_addr, fix_data}; });
}

int rdsp_engine_read_pocsag(rdsp_engine_t *e, int n_blocks, uint8_t *d_sync, size_t sync_stride, uint8_t *d_new, size_t new_stride, uint8_t *d_bad,
                            size_t bad_stride, float *d_lvl, size_t lvl_stride, float *d_dc, size_t dc_stride, void *stream) {
  if (!e) return RDSP_ERR_INVALID;
  if (!e->pocsag) {
    rdsp_set_error("rdsp_engine_read_pocsag: the POCSAG decoder is off; call rdsp_engine_enable_pocsag first");
    return RDSP_ERR_NOT_READY;
  }
  const size_t w = (size_t)std::max(n_blocks, 0);
  if (n_blocks < 0 || n_blocks > e->last_blocks || (d_sync && sync_stride < w) || (d_new && new_stride < w) || (d_bad && bad_stride < w) ||
      (d_lvl && lvl_stride < w) || (d_dc && dc_stride < w)) {
    rdsp_set_error("rdsp_engine_read_pocsag: bad argument (n_blocks %d of the last call's %d; strides at least n_blocks)", n_blocks, e->last_blocks);
    return RDSP_ERR_INVALID;
  }
  if (w == 0) return RDSP_OK;
  const EngPocsag &t = *e->pocsag;
  hipStream_t s = (hipStream_t)stream;
  const size_t n = (size_t)e->n_channels;
  hipError_t err = hipSetDevice(e->device);
  /* receivers the decoder did not run on: zeros */
  if (err == hipSuccess && d_sync) err = hipMemset2DAsync(d_sync, sync_stride, 0, w, n, s);
  if (err == hipSuccess && d_new) err = hipMemset2DAsync(d_new, new_stride, 0, w, n, s);
  if (err == hipSuccess && d_bad) err = hipMemset2DAsync(d_bad, bad_stride, 0, w, n, s);
  if (err == hipSuccess && d_lvl) err = hipMemset2DAsync(d_lvl, lvl_stride * 4, 0, w * 4, n, s);
  if (err == hipSuccess && d_dc) err = hipMemset2DAsync(d_dc, dc_stride * 4, 0, w * 4, n, s);
  for (size_t k = 0; k < t.rows.size() && err == hipSuccess; k++) {
    const size_t c0 = t.rows[k].first, count = t.rows[k].second, mb = t.max_blocks;
    if (d_sync) err = hipMemcpy2DAsync(d_sync + c0 * sync_stride, sync_stride, t.sync + c0 * mb, mb, w, count, hipMemcpyDeviceToDevice, s);
    if (err == hipSuccess && d_new) err = hipMemcpy2DAsync(d_new + c0 * new_stride, new_stride, t.fresh + c0 * mb, mb, w, count, hipMemcpyDeviceToDevice, s);
    if (err == hipSuccess && d_bad) err = hipMemcpy2DAsync(d_bad + c0 * bad_stride, bad_stride, t.bad + c0 * mb, mb, w, count, hipMemcpyDeviceToDevice, s);
    if (err == hipSuccess && d_lvl) err = hipMemcpy2DAsync(d_lvl + c0 * lvl_stride, lvl_stride * 4, t.lvl + c0 * mb, mb * 4, w * 4, count, hipMemcpyDeviceToDevice, s);
    if (err == hipSuccess && d_dc) err = hipMemcpy2DAsync(d_dc + c0 * dc_stride, dc_stride * 4, t.dc + c0 * mb, mb * 4, w * 4, count, hipMemcpyDeviceToDevice, s);
  }
  return err == hipSuccess ? RDSP_OK : engine_fail("rdsp_engine_read_pocsag", err);
}

int rdsp_engine_read_pocsag_messages(rdsp_engine_t *e, int first_channel, int n_channels, uint32_t *d_count, uint32_t *d_ring, void *stream) {
  if (!e) return RDSP_ERR_INVALID;
  if (!e->pocsag) {
    rdsp_set_error("rdsp_engine_read_pocsag_messages: the POCSAG decoder is off; call rdsp_engine_enable_pocsag first");
    return RDSP_ERR_NOT_READY;
  }
  if (first_channel < 0 || n_channels < 1 || n_channels > e->n_channels - first_channel) {
    rdsp_set_error("rdsp_engine_read_pocsag_messages: bad argument (channels %d .. of %d)", first_channel, e->n_channels);
    return RDSP_ERR_INVALID;
  }
  const uint32_t *w = e->pocsag->state + (size_t)first_channel * POCSAG_WORDS;
  hipStream_t s = (hipStream_t)stream;
  constexpr size_t ring_bytes = (size_t)RING * SLOT_WORDS * 4;
  hipError_t err = hipSetDevice(e->device);
  if (err == hipSuccess && d_count) err = hipMemcpy2DAsync(d_count, 4, w + PG_NMSGS, POCSAG_WORDS * 4, 4, (size_t)n_channels, hipMemcpyDeviceToDevice, s);
  if (err == hipSuccess && d_ring) err = hipMemcpy2DAsync(d_ring, ring_bytes, w + PG_RING, POCSAG_WORDS * 4, ring_bytes, (size_t)n_channels, hipMemcpyDeviceToDevice, s);
  return err == hipSuccess ? RDSP_OK : engine_fail("rdsp_engine_read_pocsag_messages", err);
}

}  // extern "C"
