/* rdsp_engine_tone_host.hip -- the CTCSS tone squelch of rdsp_engine_t on the host: EngTone (rdsp_engine_host.h) owns the
 * detector words, the steps, the records and its copy of the phasor table and makes the launch; the entry points check their
 * arguments.  include/rdsp.h has the definition; the kernel is rdsp_engine_tone.hip's, the arithmetic rdsp_tone.h's.
 * rdsp_engine_update launches it per NFM group behind the group's meter. */
#include "rdsp_engine_host.h"

using namespace rdsp_tone;

hipError_t EngTone::init(size_t n, size_t blocks_per_call) {
  n_channels = n; max_blocks = blocks_per_call;
  hipError_t err = alloc_zero(state, n * TONE_WORDS);
  if (err == hipSuccess) err = alloc_zero(dphi, n);
  if (err == hipSuccess) err = alloc_zero(a2, n * max_blocks);
  if (err == hipSuccess) err = alloc_zero(tone, n * max_blocks);
  if (err == hipSuccess) err = tab.alloc(rdsp_tune::TUNE_N);
  if (err == hipSuccess) err = hipMemcpy(tab, rdsp_engine_tune_table(), rdsp_tune::TUNE_N * sizeof(float4), hipMemcpyHostToDevice);
  if (err == hipSuccess) err = dphi_ev.create(hipEventDisableTiming);
  if (err == hipSuccess) err = hipEventRecord(dphi_ev, nullptr);
  dphi_stage.assign(n, 0u);
  return err;
}
hipError_t EngTone::reset(hipStream_t s) { return hipMemsetAsync(state, 0, n_channels * TONE_WORDS * 4, s); }
hipError_t EngTone::upload(const std::vector<float> &tone_hz, hipStream_t s) {
  if (!stale) return hipSuccess;
  hipError_t err = hipEventSynchronize(dphi_ev); /* the last upload has left dphi_stage */
  for (size_t c = 0; c < n_channels; c++) dphi_stage[c] = c < tone_hz.size() ? tone_dphi(tone_hz[c]) : 0u;
  if (err == hipSuccess) err = hipMemcpyAsync(dphi, dphi_stage.data(), n_channels * 4, hipMemcpyHostToDevice, s);
  if (err == hipSuccess) err = hipEventRecord(dphi_ev, s);
  if (err == hipSuccess) stale = false;
  return err;
}
hipError_t EngTone::launch_group(const EngParams &p, size_t c0, const ToneSet &set, const EngMeter *meter, const int16_t *d_lr, hipStream_t s) {
  ToneParams t{};
  t.audio = p.audio; t.audio_stride = p.audio_stride; t.out = p.out; t.out_stride = p.out_stride;
  t.out_vec = ((uintptr_t)d_lr & 15) == 0 && p.out_stride % 4 == 0;
  t.n_channels = p.n_channels; t.n_blocks = p.n_blocks; t.reset = (p.resets & RESET_FM) != 0;
  t.law = tone_law(set);
  t.dphi = dphi + c0; t.tab = tab; t.state = state + c0 * TONE_WORDS;
  t.rec_stride = max_blocks; t.a2 = a2 + c0 * max_blocks; t.tone = tone + c0 * max_blocks;
  if (meter) { t.open = meter->open + c0 * meter->max_blocks; t.open_stride = meter->max_blocks; t.meter_words = meter->words + c0 * MT_WORDS; }
  const hipError_t err = rdsp_engine_tone_launch(t, s);
  if (err == hipSuccess) rows.emplace_back(c0, (size_t)p.n_channels); /* only rows a launch wrote are read_tone's */
  return err;
}

extern "C" {

double rdsp_engine_tone_gain(float tone_hz, float tau_us) {
  if (!(tone_hz > 0.0f && tone_hz < (float)rdsp_tune::TUNE_MAX_HZ) || !rdsp_fm::tau_ok(tau_us)) {
    rdsp_set_error("rdsp_engine_tone_gain: bad argument (tone_hz %g of (0, 22050); tau_us %g of 0 or 25 .. 1000)", (double)tone_hz, (double)tau_us);
    return 0.0;
  }
  return tau_us == 0.0f ? 1.0 : tone_gain(tone_hz, rdsp_fm::fm_deemph_a(tau_us));
}

int rdsp_engine_enable_tone(rdsp_engine_t *e) {
  if (!e) return RDSP_ERR_INVALID;
  if (e->tone) return RDSP_OK;
  if (!e->fm) {
    rdsp_set_error("rdsp_engine_enable_tone: the tone squelch runs on narrow-band FM receivers; call rdsp_engine_enable_fm first");
    return RDSP_ERR_NOT_READY;
  }
  auto t = std::make_unique<EngTone>(); /* the object stays without the detector unless all of it exists */
  hipError_t err = hipSetDevice(e->device);
  if (err == hipSuccess) err = hipDeviceSynchronize(); /* the next call of every stream may run it */
  if (err == hipSuccess) err = t->init((size_t)e->n_channels, (size_t)e->max_blocks);
  if (err == hipSuccess) err = hipDeviceSynchronize();
  if (err != hipSuccess) {
    rdsp_set_error("rdsp_engine_enable_tone: %s", hipGetErrorString(err));
    return RDSP_ERR_NOMEM;
  }
  e->tone = std::move(t);
  return RDSP_OK;
}
int rdsp_engine_tone_enabled(const rdsp_engine_t *e) { return e && e->tone ? 1 : 0; }

int rdsp_engine_set_tones(rdsp_engine_t *e, int first_channel, int n_channels, const float *tone_hz) {
  if (!e || !tone_hz || first_channel < 0 || n_channels < 1 || n_channels > e->n_channels - first_channel) {
    rdsp_set_error("rdsp_engine_set_tones: bad argument (tone_hz not NULL; channels %d .. of %d)", first_channel, e ? e->n_channels : 0);
    return RDSP_ERR_INVALID;
  }
  for (int k = 0; k < n_channels; k++)
    if (!tone_ok(tone_hz[k])) {
      rdsp_set_error("rdsp_engine_set_tones: channel %d: tone %g Hz; 0 (none) or %g .. %g Hz", first_channel + k, (double)tone_hz[k],
                     (double)TONE_MIN_HZ, (double)TONE_MAX_HZ);
      return RDSP_ERR_INVALID;
    }
  if (e->tone_hz.empty()) e->tone_hz.assign((size_t)e->n_channels, 0.0f);
  std::copy(tone_hz, tone_hz + n_channels, e->tone_hz.begin() + first_channel);
  if (e->tone) e->tone->stale = true;
  return RDSP_OK;
}

int rdsp_engine_set_tone_squelch(rdsp_engine_t *e, int K, float on_amp, float off_amp) {
  if (!e || !squelch_ok(K, on_amp, off_amp)) {
    rdsp_set_error("rdsp_engine_set_tone_squelch: bad argument (K %d of %d .. %d; 0 < off_amp %g <= on_amp %g <= 1)", K, TONE_MIN_K, TONE_MAX_K,
                   (double)off_amp, (double)on_amp);
    return RDSP_ERR_INVALID;
  }
  return for_selected(e, [&](EngSettings &s) { s.tone = {K, on_amp, off_amp}; });
}

int rdsp_engine_read_tone(rdsp_engine_t *e, int n_blocks, float *d_a2, size_t a2_stride, uint8_t *d_tone, size_t tone_stride, void *stream) {
  if (!e) return RDSP_ERR_INVALID;
  if (!e->tone) {
    rdsp_set_error("rdsp_engine_read_tone: the tone squelch is off; call rdsp_engine_enable_tone first");
    return RDSP_ERR_NOT_READY;
  }
  const size_t w = (size_t)std::max(n_blocks, 0);
  if (n_blocks < 0 || n_blocks > e->last_blocks || (d_a2 && a2_stride < w) || (d_tone && tone_stride < w)) {
    rdsp_set_error("rdsp_engine_read_tone: bad argument (n_blocks %d of the last call's %d; strides at least n_blocks)", n_blocks, e->last_blocks);
    return RDSP_ERR_INVALID;
  }
  if (w == 0) return RDSP_OK;
  const EngTone &t = *e->tone;
  hipStream_t s = (hipStream_t)stream;
  const size_t n = (size_t)e->n_channels;
  hipError_t err = hipSetDevice(e->device);
  /* receivers the detector did not run on: zeros */
  if (err == hipSuccess && d_a2) err = hipMemset2DAsync(d_a2, a2_stride * 4, 0, w * 4, n, s);
  if (err == hipSuccess && d_tone) err = hipMemset2DAsync(d_tone, tone_stride, 0, w, n, s);
  for (size_t k = 0; k < t.rows.size() && err == hipSuccess; k++) {
    const size_t c0 = t.rows[k].first, count = t.rows[k].second;
    if (d_a2) err = hipMemcpy2DAsync(d_a2 + c0 * a2_stride, a2_stride * 4, t.a2 + c0 * t.max_blocks, t.max_blocks * 4, w * 4, count, hipMemcpyDeviceToDevice, s);
    if (err == hipSuccess && d_tone)
      err = hipMemcpy2DAsync(d_tone + c0 * tone_stride, tone_stride, t.tone + c0 * t.max_blocks, t.max_blocks, w, count, hipMemcpyDeviceToDevice, s);
  }
  return err == hipSuccess ? RDSP_OK : engine_fail("rdsp_engine_read_tone", err);
}

}  // extern "C"
