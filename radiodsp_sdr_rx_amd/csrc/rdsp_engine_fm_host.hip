/* rdsp_engine_fm_host.hip -- the narrow-band FM detector of rdsp_engine_t on the host: EngFm (rdsp_engine_host.h) owns the
 * state words, the level rows and the taps and makes the launch; the entry points check their arguments.  include/rdsp.h has
 * the definition; the kernel is rdsp_engine_fm.hip's, the arithmetic rdsp_fm.h's.  rdsp_engine_setDemodMode
 * (rdsp_engine_host.hip) puts a group into the mode, rdsp_engine_update launches it. */
#include "rdsp_engine_host.h"

using namespace rdsp_fm;

hipError_t EngFm::init(size_t n, size_t max_blocks) {
  n_channels = n; row_words = max_blocks * BS;
  float h[TAPS_PER_W * 2 + MAX_T];
  fm_taps(2, h);
  fm_taps(3, h + TAPS_PER_W * 2);
  hipError_t err = alloc_zero(state, n * FM_STATE_WORDS);
  if (err == hipSuccess) err = alloc_zero(level, n * row_words);
  if (err == hipSuccess) err = taps.alloc(sizeof h / sizeof h[0]);
  if (err == hipSuccess) err = hipMemcpy(taps, h, sizeof h, hipMemcpyHostToDevice);
  return err;
}
hipError_t EngFm::reset(hipStream_t s) { return hipMemsetAsync(state, 0, n_channels * FM_STATE_WORDS * 4, s); }
hipError_t EngFm::launch_group(const EngParams &p, size_t c0, const FmSet &set, const int16_t *d_iq, hipStream_t s) {
  FmParams f{};
  f.iq = p.iq; f.in_stride = p.in_stride; f.in_vec = ((uintptr_t)d_iq & 15) == 0 && p.in_stride % 4 == 0;
  f.n_channels = p.n_channels; f.n_blocks = p.n_blocks;
  f.W = set.W; f.deemph = set.tau_us != 0.0f; f.reset = (p.resets & RESET_FM) != 0;
  f.k = fm_scale(set.deviation_hz); f.a = fm_deemph_a(set.tau_us);
  f.taps = taps + (set.W == 3 ? TAPS_PER_W * 2 : 0);
  f.state = state + c0 * FM_STATE_WORDS;
  f.audio = p.audio; f.audio_stride = p.audio_stride;
  f.level = level + c0 * row_words; f.level_stride = row_words;
  const hipError_t err = rdsp_engine_fm_launch(f, s);
  if (err == hipSuccess) nfm_rows.emplace_back(c0, (size_t)p.n_channels); /* only rows a launch wrote are read_fm_level's */
  return err;
}

extern "C" {

float rdsp_engine_fm_atan2(float y, float x) { return fm_atan2(y, x); }

int rdsp_engine_fm_constants(float deviation_hz, float tau_us, float *out) {
  if (!out || !deviation_ok(deviation_hz) || !tau_ok(tau_us)) {
    rdsp_set_error("rdsp_engine_fm_constants: bad argument (deviation_hz %g of 1000 .. 7500; tau_us %g of 0 or 25 .. 1000; out not NULL)",
                   (double)deviation_hz, (double)tau_us);
    return RDSP_ERR_INVALID;
  }
  out[0] = fm_scale(deviation_hz);
  out[1] = fm_deemph_a(tau_us);
  return RDSP_OK;
}

int rdsp_engine_enable_fm(rdsp_engine_t *e) {
  if (!e) return RDSP_ERR_INVALID;
  if (e->fm) return RDSP_OK;
  auto f = std::make_unique<EngFm>(); /* the object stays without the detector unless all of it exists */
  hipError_t err = hipSetDevice(e->device);
  if (err == hipSuccess) err = hipDeviceSynchronize(); /* the next call of every stream may run it */
  if (err == hipSuccess) err = f->init((size_t)e->n_channels, (size_t)e->max_blocks);
  if (err == hipSuccess) err = hipDeviceSynchronize();
  if (err != hipSuccess) {
    rdsp_set_error("rdsp_engine_enable_fm: %s", hipGetErrorString(err));
    return RDSP_ERR_NOMEM;
  }
  e->fm = std::move(f);
  return RDSP_OK;
}
int rdsp_engine_fm_enabled(const rdsp_engine_t *e) { return e && e->fm ? 1 : 0; }

int rdsp_engine_set_fm(rdsp_engine_t *e, int W, float deviation_hz, float tau_us) {
  if (!e || !width_ok(W) || !deviation_ok(deviation_hz) || !tau_ok(tau_us)) {
    rdsp_set_error("rdsp_engine_set_fm: bad argument (W %d of 2 or 3; deviation_hz %g of 1000 .. 7500; tau_us %g of 0 or 25 .. 1000)", W,
                   (double)deviation_hz, (double)tau_us);
    return RDSP_ERR_INVALID;
  }
  return for_selected(e, [&](EngSettings &s) { s.fm = {W, deviation_hz, tau_us}; });
}

int rdsp_engine_read_fm_level(rdsp_engine_t *e, int n_blocks, float *d_out, size_t stride, void *stream) {
  if (!e) return RDSP_ERR_INVALID;
  if (!e->fm) {
    rdsp_set_error("rdsp_engine_read_fm_level: the FM detector is off; call rdsp_engine_enable_fm first");
    return RDSP_ERR_NOT_READY;
  }
  if (!d_out || n_blocks < 0 || n_blocks > e->last_blocks || stride < (size_t)n_blocks * BS) {
    rdsp_set_error("rdsp_engine_read_fm_level: bad argument (d_out not NULL; n_blocks %d of the last call's %d; stride at least n_blocks * 128)",
                   n_blocks, e->last_blocks);
    return RDSP_ERR_INVALID;
  }
  const size_t width = (size_t)n_blocks * BS * 4;
  if (width == 0) return RDSP_OK;
  const EngFm &f = *e->fm;
  hipStream_t s = (hipStream_t)stream;
  hipError_t err = hipSetDevice(e->device);
  if (err == hipSuccess) err = hipMemset2DAsync(d_out, stride * 4, 0, width, (size_t)e->n_channels, s); /* receivers not in NFM: zeros */
  for (size_t k = 0; k < f.nfm_rows.size() && err == hipSuccess; k++)
    err = hipMemcpy2DAsync(d_out + f.nfm_rows[k].first * stride, stride * 4, f.level + f.nfm_rows[k].first * f.row_words, f.row_words * 4, width,
                           f.nfm_rows[k].second, hipMemcpyDeviceToDevice, s);
  return err == hipSuccess ? RDSP_OK : engine_fail("rdsp_engine_read_fm_level", err);
}

}  // extern "C"
