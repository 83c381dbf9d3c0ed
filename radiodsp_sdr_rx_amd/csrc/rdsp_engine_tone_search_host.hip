/* rdsp_engine_tone_search_host.hip -- the CTCSS tone search of rdsp_engine_t on the host: EngToneSearch (rdsp_engine_host.h) owns
 * the detector words, the bank's steps, the records and its copy of the phasor table and makes the launch; the entry points
 * check their arguments.  include/rdsp.h has the definition; the kernel is rdsp_engine_tone_search.hip's, the arithmetic
 * rdsp_tone_search.h's.  rdsp_engine_update launches it per NFM group with a window behind the group's tone squelch. */
#include "rdsp_engine_host.h"

using namespace rdsp_tone_search;

SearchBank rdsp_engine_search_bank(const rdsp_engine_t *e) {
  return e->bank_hz.empty() ? search_bank(STANDARD_HZ, STANDARD_TONES) : search_bank(e->bank_hz.data(), (int)e->bank_hz.size());
}

hipError_t EngToneSearch::init(size_t n, size_t blocks_per_call) {
  n_channels = n; max_blocks = blocks_per_call;
  hipError_t err = alloc_zero(state, n * SEARCH_WORDS);
  if (err == hipSuccess) err = alloc_zero(dphi, (size_t)MAX_TONES);
  if (err == hipSuccess) err = alloc_zero(best, n * max_blocks);
  if (err == hipSuccess) err = alloc_zero(a2, n * max_blocks);
  if (err == hipSuccess) err = alloc_zero(next, n * max_blocks);
  if (err == hipSuccess) err = tab.alloc(rdsp_tune::TUNE_N);
  if (err == hipSuccess) err = hipMemcpy(tab, rdsp_engine_tune_table(), rdsp_tune::TUNE_N * sizeof(float4), hipMemcpyHostToDevice);
  if (err == hipSuccess) err = bank_ev.create(hipEventDisableTiming);
  if (err == hipSuccess) err = hipEventRecord(bank_ev, nullptr);
  memset(&bank, 0, sizeof bank);
  return err;
}
hipError_t EngToneSearch::reset(hipStream_t s) { return hipMemsetAsync(state, 0, n_channels * SEARCH_WORDS * 4, s); }
hipError_t EngToneSearch::upload(const SearchBank &b, hipStream_t s) {
  if (!stale) return hipSuccess;
  hipError_t err = hipEventSynchronize(bank_ev); /* the last upload has left `bank` */
  bank = b;
  if (err == hipSuccess) err = hipMemcpyAsync(dphi, bank.dphi, sizeof bank.dphi, hipMemcpyHostToDevice, s);
  if (err == hipSuccess) err = hipEventRecord(bank_ev, s);
  if (err == hipSuccess) stale = false;
  return err;
}
hipError_t EngToneSearch::launch_group(const EngParams &p, size_t c0, const SearchSet &set, hipStream_t s) {
  ToneSearchParams t{};
  t.audio = p.audio; t.audio_stride = p.audio_stride;
  t.n_channels = p.n_channels; t.n_blocks = p.n_blocks; t.reset = (p.resets & RESET_FM) != 0;
  t.law = search_law(set);
  t.n_tones = bank.n_tones; t.bank_key = bank.key; t.dphi = dphi; t.tab = tab; t.state = state + c0 * SEARCH_WORDS;
  t.rec_stride = max_blocks; t.best = best + c0 * max_blocks; t.a2 = a2 + c0 * max_blocks; t.next = next + c0 * max_blocks;
  const hipError_t err = rdsp_engine_tone_search_launch(t, s);
  if (err == hipSuccess) rows.emplace_back(c0, (size_t)p.n_channels); /* only rows a launch wrote are read_tone_search's */
  return err;
}
hipError_t EngToneSearch::clear_group(size_t c0, size_t count, hipStream_t s) {
  return hipMemsetAsync(state + c0 * SEARCH_WORDS, 0, count * SEARCH_WORDS * 4, s);
}

extern "C" {

int rdsp_engine_tone_standard(float *out50) {
  if (!out50) return RDSP_ERR_INVALID;
  std::copy(STANDARD_HZ, STANDARD_HZ + STANDARD_TONES, out50);
  return STANDARD_TONES;
}

double rdsp_engine_tone_search_gain(float tone_hz, float tau_us) {
  if (!(tone_hz > 0.0f && tone_hz < (float)rdsp_tune::TUNE_MAX_HZ) || !rdsp_fm::tau_ok(tau_us)) {
    rdsp_set_error("rdsp_engine_tone_search_gain: bad argument (tone_hz %g of (0, 22050); tau_us %g of 0 or 25 .. 1000)", (double)tone_hz, (double)tau_us);
    return 0.0;
  }
  return search_boxcar_gain(tone_hz) * rdsp_engine_tone_gain(tone_hz, tau_us);
}

int rdsp_engine_enable_tone_search(rdsp_engine_t *e) {
  if (!e) return RDSP_ERR_INVALID;
  if (e->search) return RDSP_OK;
  if (!e->fm) {
    rdsp_set_error("rdsp_engine_enable_tone_search: the tone search runs on narrow-band FM receivers; call rdsp_engine_enable_fm first");
    return RDSP_ERR_NOT_READY;
  }
  auto t = std::make_unique<EngToneSearch>(); /* the object stays without the detector unless all of it exists */
  hipError_t err = hipSetDevice(e->device);
  if (err == hipSuccess) err = hipDeviceSynchronize(); /* the next call of every stream may run it */
  if (err == hipSuccess) err = t->init((size_t)e->n_channels, (size_t)e->max_blocks);
  if (err == hipSuccess) err = hipDeviceSynchronize();
  if (err != hipSuccess) {
    rdsp_set_error("rdsp_engine_enable_tone_search: %s", hipGetErrorString(err));
    return RDSP_ERR_NOMEM;
  }
  e->search = std::move(t);
  return RDSP_OK;
}
int rdsp_engine_tone_search_enabled(const rdsp_engine_t *e) { return e && e->search ? 1 : 0; }

int rdsp_engine_set_tone_bank(rdsp_engine_t *e, const float *tone_hz, int n_tones) {
  if (!e || !bank_ok(tone_hz, n_tones)) {
    rdsp_set_error("rdsp_engine_set_tone_bank: bad argument (1 .. %d tones of %g .. %g Hz, strictly ascending; %d given)", MAX_TONES,
                   (double)rdsp_tone::TONE_MIN_HZ, (double)rdsp_tone::TONE_MAX_HZ, n_tones);
    return RDSP_ERR_INVALID;
  }
  e->bank_hz.assign(tone_hz, tone_hz + n_tones);
  if (e->search) e->search->stale = true;
  return RDSP_OK;
}
int rdsp_engine_tone_bank(const rdsp_engine_t *e, float *out64) {
  if (!e || !out64) return RDSP_ERR_INVALID;
  if (e->bank_hz.empty()) return rdsp_engine_tone_standard(out64);
  std::copy(e->bank_hz.begin(), e->bank_hz.end(), out64);
  return (int)e->bank_hz.size();
}

int rdsp_engine_set_tone_search(rdsp_engine_t *e, int K, float min_amp, float ratio) {
  if (!e || !search_ok(K, min_amp, ratio)) {
    rdsp_set_error("rdsp_engine_set_tone_search: bad argument (K %d of 0 or %d .. %d; 0 < min_amp %g <= 1; 1 <= ratio %g <= 1e6)", K,
                   rdsp_tone::TONE_MIN_K, rdsp_tone::TONE_MAX_K, (double)min_amp, (double)ratio);
    return RDSP_ERR_INVALID;
  }
  return for_selected(e, [&](EngSettings &s) { s.search = {K, min_amp, ratio}; });
}

int rdsp_engine_read_tone_search(rdsp_engine_t *e, int n_blocks, uint8_t *d_best, size_t best_stride, float *d_a2, size_t a2_stride, float *d_next,
                                 size_t next_stride, void *stream) {
  if (!e) return RDSP_ERR_INVALID;
  if (!e->search) {
    rdsp_set_error("rdsp_engine_read_tone_search: the tone search is off; call rdsp_engine_enable_tone_search first");
    return RDSP_ERR_NOT_READY;
  }
  const size_t w = (size_t)std::max(n_blocks, 0);
  if (n_blocks < 0 || n_blocks > e->last_blocks || (d_best && best_stride < w) || (d_a2 && a2_stride < w) || (d_next && next_stride < w)) {
    rdsp_set_error("rdsp_engine_read_tone_search: bad argument (n_blocks %d of the last call's %d; strides at least n_blocks)", n_blocks, e->last_blocks);
    return RDSP_ERR_INVALID;
  }
  if (w == 0) return RDSP_OK;
  const EngToneSearch &t = *e->search;
  hipStream_t s = (hipStream_t)stream;
  const size_t n = (size_t)e->n_channels;
  hipError_t err = hipSetDevice(e->device);
  /* receivers the detector did not run on: none, 0, 0 */
  if (err == hipSuccess && d_best) err = hipMemset2DAsync(d_best, best_stride, SEARCH_NONE, w, n, s);
  if (err == hipSuccess && d_a2) err = hipMemset2DAsync(d_a2, a2_stride * 4, 0, w * 4, n, s);
  if (err == hipSuccess && d_next) err = hipMemset2DAsync(d_next, next_stride * 4, 0, w * 4, n, s);
  for (size_t k = 0; k < t.rows.size() && err == hipSuccess; k++) {
    const size_t c0 = t.rows[k].first, count = t.rows[k].second, mb = t.max_blocks;
    if (d_best) err = hipMemcpy2DAsync(d_best + c0 * best_stride, best_stride, t.best + c0 * mb, mb, w, count, hipMemcpyDeviceToDevice, s);
    if (err == hipSuccess && d_a2) err = hipMemcpy2DAsync(d_a2 + c0 * a2_stride, a2_stride * 4, t.a2 + c0 * mb, mb * 4, w * 4, count, hipMemcpyDeviceToDevice, s);
    if (err == hipSuccess && d_next)
      err = hipMemcpy2DAsync(d_next + c0 * next_stride, next_stride * 4, t.next + c0 * mb, mb * 4, w * 4, count, hipMemcpyDeviceToDevice, s);
  }
  return err == hipSuccess ? RDSP_OK : engine_fail("rdsp_engine_read_tone_search", err);
}

int rdsp_engine_read_tone_spectrum(rdsp_engine_t *e, int first_channel, int n_channels, float *d_power, size_t stride, void *stream) {
  if (!e) return RDSP_ERR_INVALID;
  if (!e->search) {
    rdsp_set_error("rdsp_engine_read_tone_spectrum: the tone search is off; call rdsp_engine_enable_tone_search first");
    return RDSP_ERR_NOT_READY;
  }
  const size_t n_tones = e->bank_hz.empty() ? (size_t)STANDARD_TONES : e->bank_hz.size();
  if (!d_power || first_channel < 0 || n_channels < 1 || n_channels > e->n_channels - first_channel || stride < n_tones) {
    rdsp_set_error("rdsp_engine_read_tone_spectrum: bad argument (d_power not NULL; channels %d .. of %d; stride at least the bank's %zu tones)",
                   first_channel, e->n_channels, n_tones);
    return RDSP_ERR_INVALID;
  }
  hipError_t err = hipSetDevice(e->device);
  if (err == hipSuccess)
    err = hipMemcpy2DAsync(d_power, stride * 4, e->search->state + (size_t)first_channel * SEARCH_WORDS + TS_P, SEARCH_WORDS * 4, n_tones * 4,
                           (size_t)n_channels, hipMemcpyDeviceToDevice, (hipStream_t)stream);
  return err == hipSuccess ? RDSP_OK : engine_fail("rdsp_engine_read_tone_spectrum", err);
}

}  // extern "C"
