/*
 * rdsp_engine_sources.h -- the source front end of rdsp_engine_t (rdsp_engine_sources.hip): receivers tuned to stations inside
 * shared IQ rows.  The engine's host object (rdsp_engine_host.h) holds one, from the first rdsp_engine_set_sources on; the entry
 * points (rdsp_engine_sources_host.hip) validate their arguments and hand them over; the arithmetic is rdsp_tune.h's.
 */
#ifndef RDSP_ENGINE_SOURCES_H
#define RDSP_ENGINE_SOURCES_H

#include <functional>
#include <memory>
#include <vector>

#include "rdsp_engine_int.h"
#include "rdsp_tune.h"

namespace rdsp_eng {

/* what a stream of source rows is: rows at 44 100 P / Q Hz (lowest terms; an integer multiple D is P = D, Q = 1) in `format`,
 * and where the stream stands.  An engine without sources answers as the default: 44 100 Hz, int16. */
struct SourceStream {
  int P = 1, Q = 1, n_sources = 0, format = rdsp_tune::SRC_S16;
  uint32_t frac = 0; /* (outputs since the last restart x P) mod Q; stays 0 while Q = 1 */
  bool same(const SourceStream &o) const { return P == o.P && Q == o.Q && n_sources == o.n_sources && format == o.format; }
  int keep() const { return rdsp_tune::rate_keep(P, Q); } /* pairs of history per source */
  size_t hist_words() const { return (size_t)n_sources * (size_t)keep() * (size_t)rdsp_tune::src_hist_words(format); }
  size_t pairs(uint32_t n_out) const { return (size_t)rdsp_tune::rate_pairs(frac, P, Q, n_out); } /* of the next call */
  double band_hz() const { return (rdsp_tune::TUNE_MAX_HZ * (double)P) / (double)Q; } /* |station| must stay below it */
};

/* what the steps are computed from, handed in by the engine with every call: the first channel of each of its groups, the
 * group's tuning offset, every channel's station */
struct SourceTuning {
  const std::vector<int> &first;
  std::function<float(size_t)> offset;
  const std::vector<double> &station;
};

struct EngFrontEnd {
  const int n_channels, max_blocks;
  SourceStream st;
  float gain = 1.0f;
  /* the map: receivers in `order` (sorted by source), and both filter banks' workgroups: runs of one source's receivers */
  DevBuf<int> source_of, order, run_first[2], run_count[2];
  int n_runs[2] = {0, 0}; /* [0] of at most DDC_RPW receivers, [1] of at most RATE_RPW */
  /* per channel: phase accumulators, steps (with the host side of their last upload), the tuned rows; the phasor table */
  DevBuf<uint32_t> phase, dphi, tuned;
  DevBuf<float4> tab;
  std::vector<uint32_t> dphi_stage;
  rdsp_dev::Event dphi_ev;    /* the last upload of dphi has left dphi_stage */
  std::vector<float> tune_to; /* per group: the tuning offset the steps were computed with */
  bool dphi_stale = true;
  /* what a stream needs beyond the map: the prototype's taps by branch ([Q][Tb]; Q = 1: the 16 D taps), every receiver's
   * translated taps (Q = 1), the call's schedule (Q > 1), and per SOURCE the last keep() pairs */
  struct Bufs { DevBuf<float> h; DevBuf<float2> g; DevBuf<rdsp_tune::RateStep> sched; DevBuf<uint32_t> hist; };
  std::unique_ptr<Bufs> buf;

  EngFrontEnd(int n_channels, int max_blocks) : n_channels(n_channels), max_blocks(max_blocks) {}
  hipError_t init(); /* the per-channel buffers, the table; phases 0 */
  /* The ONE place where a stream restarts.  When the rate, the number of rows or the format changes, the histories are new
   * (zero) and frac = 0; the taps are always recomputed, the steps always marked stale, the phases never touched.  Everything
   * new exists before anything is replaced: a failure leaves the object as it was.  Waits for queued work first. */
  hipError_t configure(int P, int Q, float gain, int n_sources, int format);
  hipError_t set_map(int n_sources, const int *source_of_channel); /* the map, then configure with the new number of rows */
  hipError_t reset(hipStream_t s);                                 /* phases, histories, frac: zero */
  void steps_changed() { dphi_stale = true; }
  /* the pass the rate asks for on n_blocks blocks of rows the caller has checked, into `tuned`; then the histories and frac */
  hipError_t run(const void *d_src, size_t src_stride, int n_blocks, const SourceTuning &t, hipStream_t s);

 private:
  hipError_t upload_dphi(const SourceTuning &t, hipStream_t s);
};

}  // namespace rdsp_eng

#endif
