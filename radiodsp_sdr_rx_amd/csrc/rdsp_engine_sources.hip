/*
 * rdsp_engine_sources.hip -- the source front end of rdsp_engine_t (rdsp_engine_sources.h): the map from receivers to shared
 * IQ rows, the rows' rate P / Q and format, each receiver's phase and step, the prototype's taps and ONE history per source.
 * rdsp_engine_update_sources runs a pass that writes each receiver's row -- its source row shifted to the engine's IF, and at
 * a rate above 44 100 Hz low-passed and resampled -- into `tuned`, then the engine's own launches of rdsp_engine_update on
 * those rows.  The pass follows from the rate: Q > 1 the polyphase pass (rdsp_engine_rate.hip), else P > 1 the decimating pass
 * (rdsp_engine_ddc.hip), else the tuning pass (rdsp_engine_tune.hip); after a filter bank the one finish kernel.  Host code
 * only.  Compiled with the kernels' flags (-ffp-contract=off): the steps and the taps computed here are held bit for bit.
 */
#include "rdsp_engine_sources.h"

#include <algorithm>

using namespace rdsp_eng;
using namespace rdsp_tune;

hipError_t EngFrontEnd::init() {
  const size_t n = (size_t)n_channels;
  hipError_t err = phase.alloc(n);
  if (err == hipSuccess) err = dphi.alloc(n);
  if (err == hipSuccess) err = source_of.alloc(n);
  if (err == hipSuccess) err = order.alloc(n);
  for (int k = 0; k < 2 && err == hipSuccess; k++) {
    err = run_first[k].alloc(n);
    if (err == hipSuccess) err = run_count[k].alloc(n);
  }
  if (err == hipSuccess) err = tab.alloc(TUNE_N);
  if (err == hipSuccess) err = tuned.alloc(n * (size_t)max_blocks * BS);
  if (err == hipSuccess) err = dphi_ev.create(hipEventDisableTiming);
  if (err == hipSuccess) err = hipEventRecord(dphi_ev, nullptr);
  if (err == hipSuccess) err = hipMemset(phase, 0, n * 4);
  if (err == hipSuccess) err = hipMemcpy(tab, rdsp_engine_tune_table(), TUNE_N * sizeof(float4), hipMemcpyHostToDevice);
  dphi_stage.assign(n, 0u);
  return err;
}

hipError_t EngFrontEnd::configure(int P, int Q, float new_gain, int n_sources, int format) {
  SourceStream to = st;
  to.P = P; to.Q = Q; to.n_sources = n_sources; to.format = format;
  const bool restart = !buf || !to.same(st);
  if (restart) to.frac = 0;
  /* the prototype by branches, hb[r][j] = h[j Q + r] (Q = 1: h itself); the tuning pass has none */
  const size_t Tb = (size_t)rate_tb(P, Q), n_taps = to.keep() ? Tb * (size_t)Q : 0, words = to.hist_words();
  std::vector<float> h(n_taps), hb(n_taps);
  if (n_taps) rate_taps(P, Q, (double)new_gain, h.data());
  for (size_t r = 0; r < (size_t)Q && n_taps; r++)
    for (size_t j = 0; j < Tb; j++) hb[r * Tb + j] = h[j * (size_t)Q + r];
  hipError_t err = hipDeviceSynchronize(); /* queued passes read the taps and the histories */
  std::unique_ptr<Bufs> fresh;
  if (err == hipSuccess && restart) {
    fresh = std::make_unique<Bufs>();
    if (n_taps) err = fresh->h.alloc(n_taps);
    if (err == hipSuccess && n_taps && Q == 1) err = fresh->g.alloc((size_t)n_channels * n_taps);
    if (err == hipSuccess && Q > 1) err = fresh->sched.alloc((size_t)max_blocks * BS);
    if (err == hipSuccess && words) err = fresh->hist.alloc(words);
    if (err == hipSuccess && words) err = hipMemset(fresh->hist, 0, words * 4);
  }
  if (err == hipSuccess && n_taps) err = hipMemcpy((restart ? fresh : buf)->h, hb.data(), n_taps * 4, hipMemcpyHostToDevice);
  if (err != hipSuccess) return err;
  if (restart) buf = std::move(fresh);
  st = to;
  gain = new_gain;
  dphi_stale = true; /* the step is per source sample */
  return hipSuccess;
}

hipError_t EngFrontEnd::set_map(int n_sources, const int *source_of_channel) {
  std::vector<int> ord((size_t)n_channels), first((size_t)n_channels), count((size_t)n_channels);
  for (int c = 0; c < n_channels; c++) ord[(size_t)c] = c;
  std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return source_of_channel[a] < source_of_channel[b]; });
  hipError_t err = hipDeviceSynchronize(); /* queued passes may still read the old map */
  if (err == hipSuccess) err = hipMemcpy(source_of, source_of_channel, (size_t)n_channels * sizeof(int), hipMemcpyHostToDevice);
  if (err == hipSuccess) err = hipMemcpy(order, ord.data(), (size_t)n_channels * sizeof(int), hipMemcpyHostToDevice);
  for (int k = 0; k < 2 && err == hipSuccess; k++) {
    const int runs = source_runs(ord.data(), source_of_channel, n_channels, k ? RATE_RPW : DDC_RPW, first.data(), count.data());
    err = hipMemcpy(run_first[k], first.data(), (size_t)runs * sizeof(int), hipMemcpyHostToDevice);
    if (err == hipSuccess) err = hipMemcpy(run_count[k], count.data(), (size_t)runs * sizeof(int), hipMemcpyHostToDevice);
    if (err == hipSuccess) n_runs[k] = runs;
  }
  /* another number of rows: their histories start at zero */
  return err == hipSuccess ? configure(st.P, st.Q, gain, n_sources, st.format) : err;
}

hipError_t EngFrontEnd::reset(hipStream_t s) {
  hipError_t err = hipMemsetAsync(phase, 0, (size_t)n_channels * 4, s); /* the stations are settings: kept */
  if (err == hipSuccess && st.hist_words()) err = hipMemsetAsync(buf->hist, 0, st.hist_words() * 4, s);
  st.frac = 0;
  return err;
}

/* The steps are computed from each channel's station and its group's current mode: round((TuningOffset - station) 2^32 /
 * (44100 P / Q)) per source sample.  They are uploaded only when one of them changed. */
hipError_t EngFrontEnd::upload_dphi(const SourceTuning &t, hipStream_t s) {
  const size_t n_groups = t.first.size();
  bool changed = dphi_stale || tune_to.size() != n_groups;
  for (size_t g = 0; !changed && g < n_groups; g++) changed = tune_to[g] != t.offset(g);
  if (!changed) return hipSuccess;
  hipError_t err = hipEventSynchronize(dphi_ev); /* the last upload has left dphi_stage */
  tune_to.resize(n_groups);
  for (size_t g = 0; g < n_groups; g++) {
    const int c1 = g + 1 < n_groups ? t.first[g + 1] : n_channels;
    tune_to[g] = t.offset(g);
    for (int c = t.first[g]; c < c1; c++) dphi_stage[(size_t)c] = rate_dphi(tune_to[g], t.station[(size_t)c], st.P, st.Q);
  }
  if (err == hipSuccess) err = hipMemcpyAsync(dphi, dphi_stage.data(), dphi_stage.size() * 4, hipMemcpyHostToDevice, s);
  if (err == hipSuccess) err = hipEventRecord(dphi_ev, s);
  if (err == hipSuccess) dphi_stale = false;
  return err;
}

hipError_t EngFrontEnd::run(const void *d_src, size_t src_stride, int n_blocks, const SourceTuning &t, hipStream_t s) {
  hipError_t err = upload_dphi(t, s);
  if (err != hipSuccess) return err;
  const uint32_t n_out = (uint32_t)n_blocks * BS, pairs = (uint32_t)st.pairs(n_out);
  SourceParams b;
  b.src = d_src; b.src_stride = src_stride; b.format = st.format;
  b.dst = tuned; b.dst_stride = (size_t)max_blocks * BS;
  b.order = order; b.source_of = source_of;
  b.phase = phase; b.dphi = dphi; b.tab = tab; b.n_channels = n_channels;
  if (st.Q > 1) { /* tune, low-pass and resample by Q / P */
    RateParams q{b};
    q.hist = buf->hist; q.hb = buf->h; q.sched = buf->sched; q.wg_first = run_first[1]; q.wg_count = run_count[1]; q.n_wg = n_runs[1];
    q.P = st.P; q.Q = st.Q; q.frac = st.frac; q.n_out = n_out; q.pairs = pairs;
    err = rdsp_engine_rate_launch(q, s);
  } else if (st.P > 1) { /* tune, low-pass and decimate */
    DdcParams q{b};
    q.hist = buf->hist; q.h = buf->h; q.g = buf->g; q.wg_first = run_first[0]; q.wg_count = run_count[0]; q.n_wg = n_runs[0];
    q.D = st.P; q.n_out = n_out;
    err = rdsp_engine_ddc_launch(q, s);
  } else { /* tune: the kernel advances the phases itself, and nothing is kept */
    TuneParams p{b};
    p.cpw = std::min(TUNE_MAX_CPW, std::max(1, n_channels / 1024)); /* about a thousand workgroups or more */
    p.n_samples = n_out;
    return rdsp_engine_tune_launch(p, s);
  }
  if (err == hipSuccess) err = rdsp_engine_source_finish_launch(b, buf->hist, (uint32_t)st.keep(), pairs, st.n_sources, s);
  if (err == hipSuccess) st.frac = rate_frac_after(st.frac, st.P, st.Q, n_out);
  return err;
}
