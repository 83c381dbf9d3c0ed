/*
 * rdsp_channelizer.h -- what the two halves of rdsp_channelizer_t (include/rdsp.h) share: the object and its kernel
 * (rdsp_channelizer.hip) and the host-only half (rdsp_channelizer_host.cpp, which a stand-alone program links alone).  The
 * schedule, the prototype and the sample formats are rdsp_tune.h's; nothing of them is restated here.
 */
#ifndef RDSP_CHANNELIZER_H
#define RDSP_CHANNELIZER_H

#include "rdsp_tune.h"

namespace rdsp_chan {

constexpr int MIN_D2 = 2, MAX_D2 = rdsp_tune::DDC_MAX_D;
constexpr long long FLAT_HZ = 12000; /* the prototype's flat band is |f| <= FLAT_HZ D2, a receiver needs +-FLAT_HZ around its station */

inline bool m_ok(int M) { return M == 8 || M == 16 || M == 32 || M == 64; }

/* host only: P / (Q D2) in lowest terms, P / Q reduced by the engine's rule first; false when a limit is passed */
inline bool rate(int P, int Q, int D2, int &P1, int &Q1) {
  if (D2 < MIN_D2 || D2 > MAX_D2 || !rdsp_tune::rate_reduce(P, Q)) return false;
  long long a = P, b = (long long)Q * D2;
  while (b) { const long long t = a % b; a = b; b = t; }
  const long long p1 = P / a, q1 = ((long long)Q * D2) / a;
  if (p1 < q1 || q1 > rdsp_tune::RATE_MAX_Q) return false;
  P1 = (int)p1; Q1 = (int)q1;
  return true;
}
/* host only: fs / (2 M) + 12000 <= 12000 D2 with fs = 44100 P / Q, in integers: a station anywhere in the band lies within half
 * a spacing of a sub-band centre, and the +-12 kHz around it inside the prototype's flat band */
inline bool band_ok(int P, int Q, int M, int D2) {
  return 44100ll * P <= 2ll * M * Q * FLAT_HZ * (D2 - 1);
}

/* the kernel's arguments */
struct Params {
  const void *src; size_t src_stride;   /* [source][pairs] in the object's format, the stride in pairs */
  float2 *hist;                         /* [source][Tb]: the pairs before the call, as values */
  const float *hb;                      /* [Q1][Tb]: branch-major taps */
  const float2 *tw;                     /* [M][M]: row k holds twiddles[(k q) mod M], q = 0 ... M - 1 */
  float2 *sub; size_t sub_stride;       /* [source M + k][i] */
  int P1, Q1, Tb, xs_cap;               /* xs_cap: pairs of the source tile in LDS */
  uint32_t frac, tmod, n_out, pairs;    /* tmod = T mod M; n_out a multiple of 128 */
};

constexpr int THREADS = 256; /* four waves share a tile of TILE output instants */
constexpr int TILE = 64;
/* pairs a tile reads: n(i0 + 63) - n(i0) <= 63 Dc1, and Tb - 1 = 16 Dc1 - 1 pairs before n(i0) */
inline int tile_pairs(int Dc1) { return (TILE - 1) * Dc1 + rdsp_tune::DDC_TAPS_PER_PHASE * Dc1; }

}  // namespace rdsp_chan

hipError_t rdsp_channelizer_launch(int M, int format, const rdsp_chan::Params &p, int n_sources, hipStream_t s);

#endif
