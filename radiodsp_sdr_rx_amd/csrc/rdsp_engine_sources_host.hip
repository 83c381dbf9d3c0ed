/* rdsp_engine_sources_host.hip -- the entry points of rdsp_engine_t's shared IQ streams: receivers tuned to stations inside
 * source rows.  They check their arguments and make one call into the front end (rdsp_engine_sources.h), which the object
 * holds from the first rdsp_engine_set_sources on; and the host-only tap and rate helpers. */
#include "rdsp_engine_host.h"

namespace {
/* the stream of source rows; an engine without sources answers as one at 44 100 Hz on int16 rows */
SourceStream source_stream(const rdsp_engine_t *e) { return e && e->src ? e->src->st : SourceStream(); }
bool gain_ok(float gain) { return gain > 0.0f && std::isfinite(gain); }
/* the first channel whose station lies outside +-band, or -1 */
int station_outside(const rdsp_engine_t *e, double band) {
  for (size_t c = 0; c < e->station.size(); c++)
    if (!(fabs(e->station[c]) < band)) return (int)c;
  return -1;
}
/* the end of every setter that may begin another stream */
int configure_sources(rdsp_engine_t *e, const char *who, int P, int Q, float gain, int format) {
  hipError_t err = hipSetDevice(e->device);
  if (err == hipSuccess) err = e->src->configure(P, Q, gain, e->src->st.n_sources, format);
  return err == hipSuccess ? RDSP_OK : engine_fail(who, err);
}
}  // namespace

extern "C" {

const float *rdsp_engine_tune_table(void) {
  static const std::vector<float4> tab = [] {
    std::vector<float4> t(rdsp_tune::TUNE_N);
    rdsp_tune::tune_table(t.data());
    return t;
  }();
  return (const float *)tab.data();
}

int rdsp_engine_set_sources(rdsp_engine_t *e, int n_sources, const int *source_of_channel) {
  if (!e || n_sources < 1 || !source_of_channel) {
    rdsp_set_error("rdsp_engine_set_sources: bad argument (n_sources %d)", n_sources);
    return RDSP_ERR_INVALID;
  }
  for (int c = 0; c < e->n_channels; c++)
    if (source_of_channel[c] < 0 || source_of_channel[c] >= n_sources) {
      rdsp_set_error("rdsp_engine_set_sources: channel %d listens to source %d of %d", c, source_of_channel[c], n_sources);
      return RDSP_ERR_INVALID;
    }
  hipError_t err = hipSetDevice(e->device);
  if (err == hipSuccess && !e->src) {
    auto q = std::make_unique<EngFrontEnd>(e->n_channels, e->max_blocks); /* the object stays without sources unless all of it exists */
    err = q->init();
    if (err != hipSuccess) {
      rdsp_set_error("rdsp_engine_set_sources: %s", hipGetErrorString(err));
      return RDSP_ERR_NOMEM;
    }
    e->src = std::move(q);
    if (e->station.empty()) e->station.assign((size_t)e->n_channels, 0.0);
  }
  if (err == hipSuccess) err = e->src->set_map(n_sources, source_of_channel);
  return err == hipSuccess ? RDSP_OK : engine_fail("rdsp_engine_set_sources", err);
}

int rdsp_engine_set_source_decimation(rdsp_engine_t *e, int D, float gain) {
  if (!e || D < 1 || D > rdsp_tune::DDC_MAX_D || !gain_ok(gain)) {
    rdsp_set_error("rdsp_engine_set_source_decimation: bad argument (D %d of 1 .. %d, gain %g must be finite and above 0)", D, rdsp_tune::DDC_MAX_D, (double)gain);
    return RDSP_ERR_INVALID;
  }
  if (no_sources(e, "rdsp_engine_set_source_decimation")) return RDSP_ERR_NOT_READY;
  SourceStream to;
  to.P = D;
  if (const int c = station_outside(e, to.band_hz()); c >= 0) {
    rdsp_set_error("rdsp_engine_set_source_decimation: channel %d is tuned to %g Hz, outside a source at %d x 44100 Hz", c, e->station[(size_t)c], D);
    return RDSP_ERR_INVALID;
  }
  if ((uint64_t)e->n_channels * (uint64_t)(rdsp_tune::DDC_TAPS_PER_PHASE * D) > 0xffffffffull) {
    rdsp_set_error("rdsp_engine_set_source_decimation: %d channels x %d taps do not fit the pass's tap table", e->n_channels, rdsp_tune::DDC_TAPS_PER_PHASE * D);
    return RDSP_ERR_UNSUPPORTED;
  }
  return configure_sources(e, "rdsp_engine_set_source_decimation", D, 1, gain, e->src->st.format);
}
int rdsp_engine_source_decimation(const rdsp_engine_t *e) { return e && source_stream(e).Q == 1 ? source_stream(e).P : 0; }

int rdsp_engine_set_source_rate(rdsp_engine_t *e, int P, int Q, float gain) {
  if (!e || !rdsp_tune::rate_reduce(P, Q) || !gain_ok(gain)) {
    rdsp_set_error("rdsp_engine_set_source_rate: bad argument (in lowest terms 1 <= Q <= %d and Q <= P <= %d Q: P %d, Q %d; gain %g must be "
                   "finite and above 0)", rdsp_tune::RATE_MAX_Q, rdsp_tune::RATE_MAX_RATIO, P, Q, (double)gain);
    return RDSP_ERR_INVALID;
  }
  if (no_sources(e, "rdsp_engine_set_source_rate")) return RDSP_ERR_NOT_READY;
  if (Q == 1) return rdsp_engine_set_source_decimation(e, P, gain); /* an integer multiple: its checks and its texts */
  SourceStream to;
  to.P = P; to.Q = Q;
  if (const int c = station_outside(e, to.band_hz()); c >= 0) {
    rdsp_set_error("rdsp_engine_set_source_rate: channel %d is tuned to %g Hz, outside a source at 44100 x %d / %d Hz", c, e->station[(size_t)c], P, Q);
    return RDSP_ERR_INVALID;
  }
  return configure_sources(e, "rdsp_engine_set_source_rate", P, Q, gain, e->src->st.format);
}
int rdsp_engine_source_rate(const rdsp_engine_t *e, int *P, int *Q) {
  if (!e || !P || !Q) return RDSP_ERR_INVALID;
  *P = source_stream(e).P;
  *Q = source_stream(e).Q;
  return RDSP_OK;
}
size_t rdsp_engine_source_pairs(const rdsp_engine_t *e, int n_blocks) {
  return e && n_blocks >= 0 ? source_stream(e).pairs((uint32_t)n_blocks * BS) : 0;
}
int rdsp_engine_rate_of_hz(double fs_hz, int *P, int *Q) {
  const double top = (double)rdsp_tune::RATE_MAX_RATIO * rdsp_tune::TUNE_FS;
  if (!P || !Q || !(fs_hz >= rdsp_tune::TUNE_FS) || !(fs_hz <= top) || fs_hz != floor(fs_hz)) {
    rdsp_set_error("rdsp_engine_rate_of_hz: %g Hz is not an integer rate in 44100 ... %g Hz", fs_hz, top);
    return RDSP_ERR_INVALID;
  }
  int p = (int)fs_hz, q = 44100;
  if (!rdsp_tune::rate_reduce(p, q)) {
    rdsp_set_error("rdsp_engine_rate_of_hz: %g Hz is 44100 x %d / %d, outside Q <= %d", fs_hz, p, q, rdsp_tune::RATE_MAX_Q);
    return RDSP_ERR_INVALID;
  }
  *P = p; *Q = q;
  return RDSP_OK;
}
int rdsp_engine_rate_taps(int P, int Q, float gain, float *out) {
  if (!rdsp_tune::rate_reduce(P, Q) || !gain_ok(gain) || !out) {
    rdsp_set_error("rdsp_engine_rate_taps: bad argument (in lowest terms 1 <= Q <= %d and Q <= P <= %d Q: P %d, Q %d; gain %g)",
                   rdsp_tune::RATE_MAX_Q, rdsp_tune::RATE_MAX_RATIO, P, Q, (double)gain);
    return RDSP_ERR_INVALID;
  }
  rdsp_tune::rate_taps(P, Q, (double)gain, out);
  return RDSP_OK;
}
int rdsp_engine_ddc_taps(int D, float gain, float *out) {
  if (D < 1 || D > rdsp_tune::DDC_MAX_D || !gain_ok(gain) || !out) {
    rdsp_set_error("rdsp_engine_ddc_taps: bad argument (D %d of 1 .. %d, gain %g)", D, rdsp_tune::DDC_MAX_D, (double)gain);
    return RDSP_ERR_INVALID;
  }
  rdsp_tune::ddc_taps(D, (double)gain, out);
  return RDSP_OK;
}

int rdsp_engine_tune(rdsp_engine_t *e, int first_channel, int n_channels, const double *station_hz) {
  if (!e || !station_hz || first_channel < 0 || n_channels < 1 || n_channels > e->n_channels - first_channel) {
    rdsp_set_error("rdsp_engine_tune: bad argument (channels %d .. %d of %d)", first_channel, first_channel + n_channels - 1, e ? e->n_channels : 0);
    return RDSP_ERR_INVALID;
  }
  const double band = source_stream(e).band_hz();
  for (int k = 0; k < n_channels; k++)
    if (!(fabs(station_hz[k]) < band)) {
      rdsp_set_error("rdsp_engine_tune: channel %d: station %g Hz; |f| must be below %g Hz", first_channel + k, station_hz[k], band);
      return RDSP_ERR_INVALID;
    }
  if (e->station.empty()) e->station.assign((size_t)e->n_channels, 0.0);
  std::copy(station_hz, station_hz + n_channels, e->station.begin() + first_channel);
  if (e->src) e->src->steps_changed();
  return RDSP_OK;
}

/* The format of the source rows.  A setting: kept by reset, set_sources and the rate setters, in no blob.  Another format
 * begins another stream: the source histories (reallocated: words for S16, float2 values otherwise) and frac go to zero as
 * with a change of rate; the phases stay with their channels. */
int rdsp_engine_set_source_format(rdsp_engine_t *e, int format) {
  if (!e || format < 0 || format >= rdsp_tune::SRC_FORMATS) {
    rdsp_set_error("rdsp_engine_set_source_format: bad argument (format %d of RDSP_SRC_S16 = 0, U8 = 1, S8 = 2, F32 = 3)", format);
    return RDSP_ERR_INVALID;
  }
  if (no_sources(e, "rdsp_engine_set_source_format")) return RDSP_ERR_NOT_READY;
  const EngFrontEnd &f = *e->src;
  return format == f.st.format ? RDSP_OK : configure_sources(e, "rdsp_engine_set_source_format", f.st.P, f.st.Q, f.gain, format);
}
int rdsp_engine_source_format(const rdsp_engine_t *e) { return e ? source_stream(e).format : RDSP_ERR_INVALID; }

namespace {
/* both entry points; who: the one that was called, for the error text */
int update_source_rows(const char *who, rdsp_engine_t *e, const void *d_src, size_t src_stride, int n_blocks, int16_t *d_lr, size_t out_stride, void *stream) {
  const SourceStream st = source_stream(e);
  const size_t pair = (size_t)rdsp_tune::src_pair_bytes(st.format), need = st.pairs((uint32_t)std::max(n_blocks, 0) * BS);
  const bool bad = !e || !d_src || !d_lr || n_blocks < 0 || n_blocks > e->max_blocks || src_stride < need || out_stride < (size_t)n_blocks * BS;
  if (st.Q > 1) { /* a rational rate: rows of rdsp_engine_source_pairs pairs, aligned to a pair */
    if (bad || (uintptr_t)d_src % pair != 0) {
      rdsp_set_error("%s: bad argument (n_blocks %d of at most %d; source rows %zu-byte aligned and at least "
                     "rdsp_engine_source_pairs = %zu pairs long at 44100 x %d / %d Hz)", who, n_blocks, e->max_blocks, pair, need, st.P, st.Q);
      return RDSP_ERR_INVALID;
    }
  } else if (bad || (src_stride * pair) % 16 != 0 || ((uintptr_t)d_src & 15) != 0) {
    rdsp_set_error("%s: bad argument (n_blocks %d of at most %d; source rows 16-byte aligned, a multiple of 16 "
                   "bytes apart and at least n_blocks * 128 * D pairs long, D = %d)", who, n_blocks, e ? e->max_blocks : 0, e ? st.P : 0);
    return RDSP_ERR_INVALID;
  }
  if (no_sources(e, who)) return RDSP_ERR_NOT_READY;
  if (!e->tables) {
    rdsp_set_error("%s: the engine's coefficient tables are not loaded (rdsp_engine_load_tables)", who);
    return RDSP_ERR_NOT_READY;
  }
  if (n_blocks == 0) { e->event_blocks = 0; return RDSP_OK; } /* as rdsp_engine_update's call of no blocks */
  hipError_t err = hipSetDevice(e->device);
  const SourceTuning tuning{e->first, [e](size_t g) { return e->grp[g].tuning_offset; }, e->station};
  if (err == hipSuccess) err = e->src->run(d_src, src_stride, n_blocks, tuning, (hipStream_t)stream);
  if (err != hipSuccess) return engine_fail(who, err);
  return rdsp_engine_update(e, (const int16_t *)e->src->tuned.p, (size_t)e->max_blocks * BS, n_blocks, d_lr, out_stride, stream);
}

}  // namespace

int rdsp_engine_update_source_samples(rdsp_engine_t *e, const void *d_src, size_t src_stride, int n_blocks, int16_t *d_lr, size_t out_stride, void *stream) {
  return update_source_rows("rdsp_engine_update_source_samples", e, d_src, src_stride, n_blocks, d_lr, out_stride, stream);
}

int rdsp_engine_update_sources(rdsp_engine_t *e, const int16_t *d_src, size_t src_stride, int n_blocks, int16_t *d_lr, size_t out_stride, void *stream) {
  if (source_stream(e).format != rdsp_tune::SRC_S16) {
    rdsp_set_error("rdsp_engine_update_sources: the engine's source format is %d, not int16; call rdsp_engine_update_source_samples", source_stream(e).format);
    return RDSP_ERR_INVALID;
  }
  return update_source_rows("rdsp_engine_update_sources", e, d_src, src_stride, n_blocks, d_lr, out_stride, stream);
}

}  // extern "C"
