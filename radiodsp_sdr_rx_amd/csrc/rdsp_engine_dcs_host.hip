/* rdsp_engine_dcs_host.hip -- the DCS code squelch of rdsp_engine_t on the host: EngDcs (rdsp_engine_host.h) owns the detector
 * words, the channels' settings as the kernel reads them and the records and makes the launch; the entry points check their
 * arguments.  include/rdsp.h has the definition; the kernel is rdsp_engine_dcs.hip's, the arithmetic rdsp_dcs.h's.
 * rdsp_engine_update launches it per NFM group behind the group's tone squelch. */
#include "rdsp_engine_host.h"

using namespace rdsp_dcs;

hipError_t EngDcs::init(size_t n, size_t blocks_per_call) {
  n_channels = n; max_blocks = blocks_per_call;
  hipError_t err = alloc_zero(state, n * DCS_WORDS);
  if (err == hipSuccess) err = alloc_zero(sel, n);
  if (err == hipSuccess) err = alloc_zero(dcs, n * max_blocks);
  if (err == hipSuccess) err = alloc_zero(hits, n * max_blocks);
  if (err == hipSuccess) err = alloc_zero(word, n * max_blocks);
  if (err == hipSuccess) err = sel_ev.create(hipEventDisableTiming);
  if (err == hipSuccess) err = hipEventRecord(sel_ev, nullptr);
  sel_stage.assign(n, 0u);
  return err;
}
hipError_t EngDcs::reset(hipStream_t s) { return hipMemsetAsync(state, 0, n_channels * DCS_WORDS * 4, s); }
hipError_t EngDcs::upload(const std::vector<uint16_t> &codes, hipStream_t s) {
  if (!stale) return hipSuccess;
  hipError_t err = hipEventSynchronize(sel_ev); /* the last upload has left sel_stage */
  for (size_t c = 0; c < n_channels; c++) sel_stage[c] = c < codes.size() ? dcs_sel(codes[c]) : 0u;
  if (err == hipSuccess) err = hipMemcpyAsync(sel, sel_stage.data(), n_channels * 4, hipMemcpyHostToDevice, s);
  if (err == hipSuccess) err = hipEventRecord(sel_ev, s);
  if (err == hipSuccess) stale = false;
  return err;
}
hipError_t EngDcs::launch_group(const EngParams &p, size_t c0, const DcsSet &set, const EngMeter *meter, const int16_t *d_lr, hipStream_t s) {
  DcsParams t{};
  t.audio = p.audio; t.audio_stride = p.audio_stride; t.out = p.out; t.out_stride = p.out_stride;
  t.out_vec = ((uintptr_t)d_lr & 15) == 0 && p.out_stride % 4 == 0;
  t.n_channels = p.n_channels; t.n_blocks = p.n_blocks; t.reset = (p.resets & RESET_FM) != 0;
  t.law = dcs_law(set);
  t.sel = sel + c0; t.state = state + c0 * DCS_WORDS;
  t.rec_stride = max_blocks; t.dcs = dcs + c0 * max_blocks; t.hits = hits + c0 * max_blocks; t.word = word + c0 * max_blocks;
  if (meter) { t.open = meter->open + c0 * meter->max_blocks; t.open_stride = meter->max_blocks; t.meter_words = meter->words + c0 * MT_WORDS; }
  const hipError_t err = rdsp_engine_dcs_launch(t, s);
  if (err == hipSuccess) rows.emplace_back(c0, (size_t)p.n_channels); /* only rows a launch wrote are read_dcs's */
  return err;
}

extern "C" {

uint32_t rdsp_dcs_codeword(int code) {
  if (code < 0 || code > DCS_MAX_CODE) {
    rdsp_set_error("rdsp_dcs_codeword: code %d of 0 .. %d", code, DCS_MAX_CODE);
    return 0u;
  }
  return dcs_codeword(code);
}

int rdsp_dcs_standard(uint16_t *out104) {
  if (!out104) return RDSP_ERR_INVALID;
  std::copy(STANDARD, STANDARD + STANDARD_CODES, out104);
  return STANDARD_CODES;
}

int rdsp_dcs_code_of_word(uint32_t word, int *code, int *inverted) {
  if (!code || !inverted || word == 0u || word > WORD_MASK) {
    rdsp_set_error("rdsp_dcs_code_of_word: bad argument (code and inverted not NULL; word 0x%x of 1 .. 0x7FFFFF)", word);
    return RDSP_ERR_INVALID;
  }
  const uint32_t c = dcs_canon(word);
  for (int inv = 0; inv < 2; inv++)
    for (int k = 0; k < STANDARD_CODES; k++)
      if (dcs_canon(dcs_codeword(STANDARD[k]) ^ (inv ? WORD_MASK : 0u)) == c) {
        *code = STANDARD[k]; *inverted = inv;
        return RDSP_OK;
      }
  rdsp_set_error("rdsp_dcs_code_of_word: 0x%06x is no rotation of a standard code's word", word);
  return RDSP_ERR_INVALID;
}

int rdsp_engine_enable_dcs(rdsp_engine_t *e) {
  if (!e) return RDSP_ERR_INVALID;
  if (e->dcs) return RDSP_OK;
  if (!e->fm) {
    rdsp_set_error("rdsp_engine_enable_dcs: the code squelch runs on narrow-band FM receivers; call rdsp_engine_enable_fm first");
    return RDSP_ERR_NOT_READY;
  }
  auto t = std::make_unique<EngDcs>(); /* the object stays without the detector unless all of it exists */
  hipError_t err = hipSetDevice(e->device);
  if (err == hipSuccess) err = hipDeviceSynchronize(); /* the next call of every stream may run it */
  if (err == hipSuccess) err = t->init((size_t)e->n_channels, (size_t)e->max_blocks);
  if (err == hipSuccess) err = hipDeviceSynchronize();
  if (err != hipSuccess) {
    rdsp_set_error("rdsp_engine_enable_dcs: %s", hipGetErrorString(err));
    return RDSP_ERR_NOMEM;
  }
  e->dcs = std::move(t);
  return RDSP_OK;
}
int rdsp_engine_dcs_enabled(const rdsp_engine_t *e) { return e && e->dcs ? 1 : 0; }

int rdsp_engine_set_dcs_codes(rdsp_engine_t *e, int first_channel, int n_channels, const uint16_t *codes) {
  if (!e || !codes || first_channel < 0 || n_channels < 1 || n_channels > e->n_channels - first_channel) {
    rdsp_set_error("rdsp_engine_set_dcs_codes: bad argument (codes not NULL; channels %d .. of %d)", first_channel, e ? e->n_channels : 0);
    return RDSP_ERR_INVALID;
  }
  for (int k = 0; k < n_channels; k++)
    if (!code_ok(codes[k])) {
      rdsp_set_error("rdsp_engine_set_dcs_codes: channel %d: code 0x%04x; 0 (none), 1 .. %d, the same + 0x8000 (inverted) or 0xFFFF (any)",
                     first_channel + k, (unsigned)codes[k], DCS_MAX_CODE);
      return RDSP_ERR_INVALID;
    }
  if (e->dcs_codes.empty()) e->dcs_codes.assign((size_t)e->n_channels, (uint16_t)0);
  std::copy(codes, codes + n_channels, e->dcs_codes.begin() + first_channel);
  if (e->dcs) e->dcs->stale = true;
  return RDSP_OK;
}

int rdsp_engine_set_dcs_squelch(rdsp_engine_t *e, int K, int max_err, int on_hits, int off_hits) {
  if (!e || !squelch_ok(K, max_err, on_hits, off_hits)) {
    rdsp_set_error("rdsp_engine_set_dcs_squelch: bad argument (K %d of %d .. %d; max_err %d of 0 .. %d; 1 <= off_hits %d <= on_hits %d <= K 1024 / 2625)", K,
                   DCS_MIN_K, DCS_MAX_K, max_err, DCS_MAX_ERR, off_hits, on_hits);
    return RDSP_ERR_INVALID;
  }
  return for_selected(e, [&](EngSettings &s) { s.dcs = {K, max_err, on_hits, off_hits}; });
}

int rdsp_engine_read_dcs(rdsp_engine_t *e, int n_blocks, uint8_t *d_dcs, size_t dcs_stride, uint8_t *d_hits, size_t hits_stride, uint32_t *d_word,
                         size_t word_stride, void *stream) {
  if (!e) return RDSP_ERR_INVALID;
  if (!e->dcs) {
    rdsp_set_error("rdsp_engine_read_dcs: the code squelch is off; call rdsp_engine_enable_dcs first");
    return RDSP_ERR_NOT_READY;
  }
  const size_t w = (size_t)std::max(n_blocks, 0);
  if (n_blocks < 0 || n_blocks > e->last_blocks || (d_dcs && dcs_stride < w) || (d_hits && hits_stride < w) || (d_word && word_stride < w)) {
    rdsp_set_error("rdsp_engine_read_dcs: bad argument (n_blocks %d of the last call's %d; strides at least n_blocks)", n_blocks, e->last_blocks);
    return RDSP_ERR_INVALID;
  }
  if (w == 0) return RDSP_OK;
  const EngDcs &t = *e->dcs;
  hipStream_t s = (hipStream_t)stream;
  const size_t n = (size_t)e->n_channels;
  hipError_t err = hipSetDevice(e->device);
  /* receivers the detector did not run on: zeros */
  if (err == hipSuccess && d_dcs) err = hipMemset2DAsync(d_dcs, dcs_stride, 0, w, n, s);
  if (err == hipSuccess && d_hits) err = hipMemset2DAsync(d_hits, hits_stride, 0, w, n, s);
  if (err == hipSuccess && d_word) err = hipMemset2DAsync(d_word, word_stride * 4, 0, w * 4, n, s);
  for (size_t k = 0; k < t.rows.size() && err == hipSuccess; k++) {
    const size_t c0 = t.rows[k].first, count = t.rows[k].second, mb = t.max_blocks;
    if (d_dcs) err = hipMemcpy2DAsync(d_dcs + c0 * dcs_stride, dcs_stride, t.dcs + c0 * mb, mb, w, count, hipMemcpyDeviceToDevice, s);
    if (err == hipSuccess && d_hits) err = hipMemcpy2DAsync(d_hits + c0 * hits_stride, hits_stride, t.hits + c0 * mb, mb, w, count, hipMemcpyDeviceToDevice, s);
    if (err == hipSuccess && d_word)
      err = hipMemcpy2DAsync(d_word + c0 * word_stride, word_stride * 4, t.word + c0 * mb, mb * 4, w * 4, count, hipMemcpyDeviceToDevice, s);
  }
  return err == hipSuccess ? RDSP_OK : engine_fail("rdsp_engine_read_dcs", err);
}

}  // extern "C"
