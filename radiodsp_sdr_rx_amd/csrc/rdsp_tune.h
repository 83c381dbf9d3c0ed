/*
 * rdsp_tune.h -- the arithmetic of rdsp_engine_t's tuning pass (rdsp_engine_update_sources, include/rdsp.h): receiver
 * ch's row is its source row times e^{+j phi[n]}, phi a uint32 phase accumulator, requantized to int16.  Shared by the
 * kernel (rdsp_engine_tune.hip) and the host restatement of the tests (tests/host/host_source_pass_check.cpp), so both evaluate
 * the same operations in the same order; both are compiled with -ffp-contract=off, and every fused operation is an fmaf.
 *
 * The phasor: a table of TUNE_N entries {cos, sin of 2 pi k / TUNE_N, and the steps to entry k + 1}, generated on the host
 * (libm in double, rounded to float), and linear interpolation by the low TUNE_FRAC_BITS of the phase.  The chord's error is
 * at most (2 pi / TUNE_N)^2 / 8 = 4.7e-6 at TUNE_N = 1024, below 2^-17 with the rounding of the table and of the fmaf
 * (tests/test_engine_tuning.py sweeps it).  Phase 0 is entry 0 with a zero fraction: exactly (1, 0), so a receiver whose
 * shift is 0 gets its source's pairs unchanged, -32768 included.
 *
 * The source rows may hold int16, uint8, int8 or float32 pairs (rdsp_engine_set_source_format): src_value below is the one
 * place where an element becomes the float that enters the arithmetic, for all three passes and for the host restatements.
 */
#ifndef RDSP_TUNE_H
#define RDSP_TUNE_H

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <type_traits>

#ifndef RDSP_HD
#define RDSP_HD __host__ __device__ __forceinline__
#endif

namespace rdsp_tune {

constexpr int TUNE_BITS = 10;
constexpr int TUNE_N = 1 << TUNE_BITS;
constexpr int TUNE_FRAC_BITS = 32 - TUNE_BITS;
constexpr double TUNE_FS = 44100.0; /* the engine's only rate */
constexpr double TUNE_MAX_HZ = 22050.0; /* |station| must stay below it */

/* host only: the table, float4 {cos, sin, cos[k + 1] - cos[k], sin[k + 1] - sin[k]} (entry TUNE_N is entry 0) */
inline void tune_table(float4 *tab) {
  float c[TUNE_N + 1], s[TUNE_N + 1];
  for (int k = 0; k < TUNE_N; k++) {
    const double a = 2.0 * 3.14159265358979323846 * (double)k / (double)TUNE_N;
    c[k] = (float)cos(a);
    s[k] = (float)sin(a);
  }
  c[0] = 1.0f; s[0] = 0.0f;
  c[TUNE_N] = c[0]; s[TUNE_N] = s[0];
  for (int k = 0; k < TUNE_N; k++) tab[k] = make_float4(c[k], s[k], c[k + 1] - c[k], s[k + 1] - s[k]);
}

/* e^{+j 2 pi ph / 2^32} as (cos, sin) */
RDSP_HD float2 tune_phasor(const float4 *tab, uint32_t ph) {
  const float4 t = tab[ph >> TUNE_FRAC_BITS];
  const float f = (float)(ph & ((1u << TUNE_FRAC_BITS) - 1u)) * 0x1p-22f; /* exact: 22 bits */
  return make_float2(fmaf(f, t.z, t.x), fmaf(f, t.w, t.y));
}

/* round half to even, then saturate */
RDSP_HD uint32_t tune_q16(float v) {
  v = fminf(fmaxf(rintf(v), -32768.0f), 32767.0f);
  return (uint32_t)(uint16_t)(int16_t)(int)v;
}

/* ---- the value of a source sample (rdsp_engine_set_source_format): the float, in counts on the int16 scale, that enters the
 * arithmetic of all three passes.  `bits` is the element zero-extended (a float's bit pattern).  ONE function for the kernels
 * and the host restatements; everything after it is the same arithmetic in every format.
 *   S16  (float)x
 *   U8   offset binary: (float)(2 u - 255) x 128, exact, +-32 640, symmetric about 127.5 where a dongle's zero sits
 *   S8   (float)s x 256, exact
 *   F32  full scale +-1.0: NaN -> 0; otherwise clamp(x, -256, 256) x 32768 (the scale is exact; +-inf and wild values stay
 *        finite at +-2^23 counts, and the output saturates as always)
 * Every 8-bit value is an exact int16, and a float k / 32768 is the int16 k: those rows give the bits of the int16 pass. */
constexpr int SRC_S16 = 0, SRC_U8 = 1, SRC_S8 = 2, SRC_F32 = 3, SRC_FORMATS = 4;
RDSP_HD float src_value(int fmt, uint32_t bits) {
  switch (fmt) {
    case SRC_U8: return (float)(2 * (int)(bits & 0xffu) - 255) * 128.0f;
    case SRC_S8: return (float)(int8_t)(uint8_t)(bits & 0xffu) * 256.0f;
    case SRC_F32: {
      const float x = __builtin_bit_cast(float, bits);
      if (x != x) return 0.0f;
      return fminf(fmaxf(x, -256.0f), 256.0f) * 32768.0f;
    }
    default: return (float)(int16_t)(uint16_t)(bits & 0xffffu);
  }
}
/* bytes of a pair I, Q (interleaved in every format); words of a pair in the engine's history: S16 keeps the packed word, the
 * other formats keep float2 VALUES, so that a fresh history is exactly 0 in every format (no uint8 byte has the value 0) */
RDSP_HD int src_pair_bytes(int fmt) { return fmt == SRC_F32 ? 8 : fmt == SRC_S16 ? 4 : 2; }
RDSP_HD int src_hist_words(int fmt) { return fmt == SRC_S16 ? 1 : 2; }
/* where pair i of a row in format F lies */
template <int F>
RDSP_HD const void *src_at(const void *row, size_t i) {
  if constexpr (F == SRC_F32) return (const uint2 *)row + i;
  else if constexpr (F == SRC_S16) return (const uint32_t *)row + i;
  else return (const uint16_t *)row + i;
}
/* pair i of a row in format F; the row is aligned to a pair */
template <int F>
RDSP_HD float2 src_pair(const void *row, long long i) {
  if constexpr (F == SRC_F32) {
    const uint2 w = ((const uint2 *)row)[i];
    return make_float2(src_value(F, w.x), src_value(F, w.y));
  } else if constexpr (F == SRC_S16) {
    const uint32_t w = ((const uint32_t *)row)[i];
    return make_float2(src_value(F, w & 0xffffu), src_value(F, w >> 16));
  } else {
    const uint32_t w = ((const uint16_t *)row)[i];
    return make_float2(src_value(F, w & 0xffu), src_value(F, w >> 8));
  }
}
/* pair i of the call's row, or for i < 0 of the `keep` pairs the engine kept from the calls before */
template <int F, typename I>
RDSP_HD float2 src_or_hist(const void *row, const void *hist, I i, int keep) {
  if constexpr (F == SRC_S16) {
    const uint32_t w = i >= 0 ? ((const uint32_t *)row)[i] : ((const uint32_t *)hist)[i + keep];
    return make_float2(src_value(F, w & 0xffffu), src_value(F, w >> 16));
  } else {
    return i >= 0 ? src_pair<F>(row, i) : ((const float2 *)hist)[i + keep];
  }
}

/* fmt in f's argument as a compile-time constant (an std::integral_constant): the one switch of the launchers */
template <typename Fn>
inline hipError_t dispatch_format(int fmt, Fn f) {
  switch (fmt) {
    case SRC_S16: f(std::integral_constant<int, SRC_S16>()); break;
    case SRC_U8: f(std::integral_constant<int, SRC_U8>()); break;
    case SRC_S8: f(std::integral_constant<int, SRC_S8>()); break;
    case SRC_F32: f(std::integral_constant<int, SRC_F32>()); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

/* a pair as values: of an int16 word I | Q << 16, or the values themselves.  What follows takes either through it. */
RDSP_HD float2 pair_value(uint32_t w) { return make_float2(src_value(SRC_S16, w & 0xffffu), src_value(SRC_S16, w >> 16)); }
RDSP_HD float2 pair_value(float2 x) { return x; }

/* one pair (a word or values) times (c + j s), rotated as the engine's shifter rotates */
template <typename X>
RDSP_HD uint32_t tune_pair(X pair, float2 cs) {
  const float2 x = pair_value(pair);
  const float ir = fmaf(x.x, cs.x, -(x.y * cs.y));
  const float qr = fmaf(x.y, cs.x, x.x * cs.y);
  return tune_q16(ir) | tune_q16(qr) << 16;
}

/* phase of sample t of a call that starts at phase ph0; the accumulator after a call of n samples is tune_phase(ph0, dphi, n) */
RDSP_HD uint32_t tune_phase(uint32_t ph0, uint32_t dphi, uint32_t t) { return ph0 + t * dphi; }

/* host only: the step per source sample that moves a station at station_hz (from the stream's centre) to the engine's IF, the
 * source at 44 100 P / Q Hz (Q = 1: P x 44 100 Hz, the division by 1.0 exact; P = Q = 1 divides by TUNE_FS itself) */
inline uint32_t rate_dphi(float tuning_offset, double station_hz, int P, int Q) {
  return (uint32_t)(unsigned long long)llround(((double)tuning_offset - station_hz) * 4294967296.0 / (((double)P * TUNE_FS) / (double)Q));
}
inline uint32_t ddc_dphi(float tuning_offset, double station_hz, int D) { return rate_dphi(tuning_offset, station_hz, D, 1); }
inline uint32_t tune_dphi(float tuning_offset, double station_hz) { return rate_dphi(tuning_offset, station_hz, 1, 1); }

/* what the arguments of all three passes share.  Receivers are visited in `order` (grouped by source).  The order of the
 * fields here and in the three structs that extend it decides how the compiler groups the kernels' scalar argument loads: with
 * this one the tuning, the decimating and the int16 polyphase kernel keep the registers and instruction counts they had with a
 * struct each (docs/engine.md). */
struct SourceParams {
  int n_channels;
  int format;                               /* SRC_* */
  const void *src; size_t src_stride;       /* [source][t] pairs in `format`, the stride in pairs; rows pair-aligned */
  uint32_t *dst; size_t dst_stride;         /* [ch][t] */
  const int *order, *source_of;             /* [n_channels] */
  uint32_t *phase; const uint32_t *dphi;    /* [n_channels] */
  const float4 *tab;                        /* [TUNE_N] */
};
/* host only: the workgroups of a filter-bank pass: runs of at most `max` receivers of ONE source that are neighbours in `order`
 * (n receivers).  first[w], count[w] (room for n each) describe run w; returns how many there are. */
inline int source_runs(const int *order, const int *source_of, int n, int max, int *first, int *count) {
  int runs = 0;
  for (int i = 0; i < n;) {
    int j = i + 1;
    while (j < n && j - i < max && source_of[order[j]] == source_of[order[i]]) j++;
    first[runs] = i;
    count[runs++] = j - i;
    i = j;
  }
  return runs;
}

/* the tuning pass's arguments: cpw receivers per workgroup */
struct TuneParams : SourceParams {
  int cpw;
  uint32_t n_samples;                       /* a multiple of 8 */
};
constexpr int TUNE_THREADS = 256;
constexpr int TUNE_MAX_CPW = 8;

/* ---- sources at D x 44 100 Hz: tune, low-pass and decimate by D (rdsp_engine_set_source_decimation) ---------------------------
 * Output m of a receiver whose source row is x (pairs before the call included):
 *   y[m] = sat16(rne(e^{+j phi_m} * sum_{k < T} g_k x[(m + 1) D - 1 - k])),  g_k = h_k e^{-j 2 pi k dphi / 2^32},  T = 16 D,
 *   phi_{m + 1} = phi_m + D dphi,  dphi = round((TuningOffset - station) 2^32 / (D 44100)).
 * h is the prototype low-pass below (a design of this build).  The order of the operations, fixed here for the kernel
 * (rdsp_engine_ddc.hip) and for the host restatement (tests/host/host_source_pass_check.cpp): g_k = (h_k c, h_k s), (c, s) =
 * tune_phasor(-k dphi); ONE serial chain over k = 0 ... T - 1 per component, four fmaf a tap (ddc_mac); the rotation,
 * rounding and saturation of tune_pair (ddc_rot).  The chain has no tile, register block or call size in it, so neither
 * has the result. */
constexpr int DDC_MAX_D = 64;
constexpr int DDC_TAPS_PER_PHASE = 16;          /* T = 16 D */
constexpr int DDC_HIST_PER_PHASE = DDC_TAPS_PER_PHASE - 1; /* a source keeps its last 15 D pairs between calls */

/* host only, libm-free (+ - * / sqrt in double, so any host evaluates the same bits): sin(pi r / (2 D)) for 0 <= r <= D */
inline double ddc_sin_quarter(int r, int D) {
  const double a = (3.141592653589793 * (double)r) / (2.0 * (double)D), a2 = a * a;
  double term = a, sum = a;
  for (int n = 1; n <= 14; n++) {
    term = -(term * a2) / (double)((2 * n) * (2 * n + 1));
    sum += term;
  }
  return sum;
}
/* sin(pi q / (2 D)), q >= 0: the argument is reduced in integers */
inline double ddc_sin_halfpi(int q, int D) {
  int r = q % (4 * D);
  double sign = 1.0;
  if (r >= 2 * D) { sign = -1.0; r -= 2 * D; }
  if (r > D) r = 2 * D - r;
  return sign * ddc_sin_quarter(r, D);
}
/* the modified Bessel function I0 by its power series, 40 terms (x <= 9: the 40th is below 1e-40 of the sum) */
inline double ddc_i0(double x) {
  const double y = x / 2.0;
  double term = 1.0, sum = 1.0;
  for (int n = 1; n <= 40; n++) {
    const double t = y / (double)n;
    term = term * (t * t);
    sum += term;
  }
  return sum;
}
constexpr double DDC_KAISER_BETA = 9.0;
RDSP_HD int rate_dc(int P, int Q) { return (P + Q - 1) / Q; }
RDSP_HD int rate_tb(int P, int Q) { return DDC_TAPS_PER_PHASE * rate_dc(P, Q); }
/* host only, libm-free: the prototype of a source at 44 100 P / Q Hz (the polyphase pass below; Q = 1: this pass, P = D), Tp = Tb Q
 * taps at the rate 44 100 P: a sinc with its cutoff at the output's Nyquist frequency (22 050 Hz) under a Kaiser window of
 * beta = 9, normalised to sum 1 (summed in tap order), times Q gain (every branch then sums to about gain), rounded to float.
 * Symmetric: every term is a function of |2 i - (Tp - 1)|.  Up to 451 584 taps: the doubles are taken from the heap. */
inline void rate_taps(int P, int Q, double gain, float *out) {
  const int Tp = rate_tb(P, Q) * Q;
  double *h = new double[(size_t)Tp], sum = 0.0;
  const double i0b = ddc_i0(DDC_KAISER_BETA);
  for (int i = 0; i < Tp; i++) {
    const int q = 2 * i - (Tp - 1) < 0 ? (Tp - 1) - 2 * i : 2 * i - (Tp - 1); /* odd: the sinc's argument is q / (2 P), never 0 */
    const double u = (3.141592653589793 * (double)q) / (2.0 * (double)P);
    const double rho = (double)q / (double)(Tp - 1);
    h[i] = (ddc_sin_halfpi(q, P) / u) * (ddc_i0(DDC_KAISER_BETA * sqrt(1.0 - rho * rho)) / i0b);
  }
  for (int i = 0; i < Tp; i++) sum += h[i];
  const double scale = (double)Q * gain;
  for (int i = 0; i < Tp; i++) out[i] = (float)((h[i] / sum) * scale);
  delete[] h;
}
inline void ddc_taps(int D, double gain, float *out) { rate_taps(D, 1, gain, out); }

/* tap k of a receiver: the prototype's tap translated onto the station */
RDSP_HD float2 ddc_tap(const float4 *tab, float h, uint32_t dphi, uint32_t k) {
  const float2 cs = tune_phasor(tab, 0u - k * dphi);
  return make_float2(h * cs.x, h * cs.y);
}
/* acc += g x, one tap of the chain */
RDSP_HD void ddc_mac(float &re, float &im, float2 g, float xi, float xq) {
  re = fmaf(g.x, xi, re);
  re = fmaf(-g.y, xq, re);
  im = fmaf(g.x, xq, im);
  im = fmaf(g.y, xi, im);
}
/* the filtered sample times (c + j s), as tune_pair rotates, rounds and saturates */
RDSP_HD uint32_t ddc_rot(float re, float im, float2 cs) {
  const float ir = fmaf(re, cs.x, -(im * cs.y));
  const float qr = fmaf(im, cs.x, re * cs.y);
  return tune_q16(ir) | tune_q16(qr) << 16;
}
/* one output: newest points at x[(m + 1) D - 1] (the T - 1 pairs before it are read; words, or the values of src_pair of any
 * format and of the history), g at the receiver's T taps */
template <typename X>
RDSP_HD uint32_t ddc_output(const float2 *g, int T, const X *newest, float2 cs) {
  float re = 0.0f, im = 0.0f;
  for (int k = 0; k < T; k++) {
    const float2 x = pair_value(newest[-k]);
    ddc_mac(re, im, g[k], x.x, x.y);
  }
  return ddc_rot(re, im, cs);
}

/* the decimating pass's arguments.  Receivers are visited in `order` (grouped by source); workgroup w of a tile takes the
 * DDC_RPW-or-fewer receivers order[wg_first[w]] ... of ONE source. */
constexpr int DDC_THREADS = 256;
constexpr int DDC_C = 4;                          /* receivers per wave, a register block */
constexpr int DDC_RPW = DDC_C * (DDC_THREADS / 64); /* receivers per workgroup */
struct DdcParams : SourceParams {           /* n_out * D pairs per source row */
  const void *hist;                         /* [source][15 D]: the pairs before the call (S16: words; otherwise float2 values) */
  const int *wg_first, *wg_count;           /* [n_wg] */
  const float *h;                           /* [16 D] */
  float2 *g;                                /* [n_channels][16 D], written by the pass's first kernel */
  int n_wg, D;
  uint32_t n_out;                           /* a multiple of 128 */
};

/* ---- sources at 44 100 P / Q Hz: tune, low-pass and change the rate by Q / P in one polyphase pass (rdsp_engine_set_source_rate) --
 * P / Q in lowest terms, 1 <= Q <= 441, Q <= P <= 64 Q; Q = 1 IS the decimating pass above (the engine routes it there).
 * Dc = ceil(P / Q); a branch has Tb = 16 Dc taps; the prototype has Tp = Tb Q taps at the rate 44 100 P.
 * Schedule: with M outputs since the last reset, frac = (M P) mod Q.  Output i of a call has its newest source pair at
 * local index n(i) = (frac + (i + 1) P) div Q - 1 (>= 0, as P >= Q) and uses branch r(i) = (frac + (i + 1) P) mod Q; a call
 * of n_out outputs consumes (frac + n_out P) div Q pairs and leaves frac = (frac + n_out P) mod Q.  The products are taken
 * in 64 bits (n_out P reaches 1.9e9).
 * Arithmetic of output i, x the row with the pairs of earlier calls before it, hb[r][j] = h[j Q + r]:
 *   e_j = tune_phasor(0 - j dphi);  u_j = (hb[r][j] xI[n - j], hb[r][j] xQ[n - j]), two rounded products (rate_u);
 *   ONE chain over j = 0 ... Tb - 1 per component from 0: ddc_mac(re, im, e_j, u_j.x, u_j.y);
 *   y[i] = ddc_rot(re, im, tune_phasor(ph0 + (n + 1 - Dc) dphi));  the phase after the call is ph0 + pairs dphi.
 * The tap multiplies the SAMPLE, not the phasor: u_j does not depend on the receiver, so a workgroup computes it once for
 * all its receivers (rdsp_engine_rate.hip).  For Q = 1 the window and the phases are the decimating pass's. */
constexpr int RATE_MAX_Q = 441;
constexpr int RATE_MAX_RATIO = DDC_MAX_D; /* P <= 64 Q */

struct RateStep { int n, r; }; /* newest pair's local index, branch */
RDSP_HD RateStep rate_step(uint32_t frac, int P, int Q, uint32_t i) {
  const uint64_t t = (uint64_t)frac + ((uint64_t)i + 1u) * (uint64_t)P;
  RateStep s;
  s.n = (int)(t / (uint64_t)Q) - 1;
  s.r = (int)(t % (uint64_t)Q);
  return s;
}
/* pairs a call of n_out outputs consumes, and frac after it */
RDSP_HD uint64_t rate_pairs(uint32_t frac, int P, int Q, uint32_t n_out) { return ((uint64_t)frac + (uint64_t)n_out * (uint64_t)P) / (uint64_t)Q; }
RDSP_HD uint32_t rate_frac_after(uint32_t frac, int P, int Q, uint32_t n_out) { return (uint32_t)(((uint64_t)frac + (uint64_t)n_out * (uint64_t)P) % (uint64_t)Q); }

/* host only: P / Q in lowest terms and inside the limits? (reduces in place) */
inline bool rate_reduce(int &P, int &Q) {
  if (P < 1 || Q < 1) return false;
  int a = P, b = Q;
  while (b) { const int t = a % b; a = b; b = t; }
  P /= a; Q /= a;
  return Q <= RATE_MAX_Q && P >= Q && (long long)P <= (long long)RATE_MAX_RATIO * Q;
}
/* the tap on the sample: two rounded products */
template <typename X>
RDSP_HD float2 rate_u(float h, X pair) {
  const float2 x = pair_value(pair);
  return make_float2(h * x.x, h * x.y);
}
/* one output: hb points at its branch's Tb taps, newest at x[n(i)] (the Tb - 1 pairs before it are read; words or values) */
template <typename X>
RDSP_HD uint32_t rate_output(const float4 *tab, const float *hb, int Tb, uint32_t dphi, const X *newest, float2 cs) {
  float re = 0.0f, im = 0.0f;
  uint32_t ph = 0u;
  for (int j = 0; j < Tb; j++, ph -= dphi) { /* ph = 0 - j dphi */
    const float2 u = rate_u(hb[j], newest[-j]);
    ddc_mac(re, im, tune_phasor(tab, ph), u.x, u.y);
  }
  return ddc_rot(re, im, cs);
}
/* the phase of output i's rotation */
RDSP_HD uint32_t rate_phase(uint32_t ph0, uint32_t dphi, int n, int Dc) { return ph0 + (uint32_t)(n + 1 - Dc) * dphi; }

/* the polyphase pass's arguments.  Workgroup w takes the RATE_RPW-or-fewer receivers order[wg_first[w]] ... of ONE source. */
constexpr int RATE_THREADS = 256;
constexpr int RATE_C = 2;                 /* receivers per lane */
constexpr int RATE_O = 16;                /* outputs per wave; two waves of a workgroup split a tile of 32 */
constexpr int RATE_TILE = 2 * RATE_O;
constexpr int RATE_RPW = 64 * RATE_C * 2; /* receivers per workgroup: two waves split them */
constexpr int RATE_CHUNK = 128;           /* taps staged in LDS at a time */
struct RateParams : SourceParams {          /* `pairs` pairs per source row */
  const float *hb;                          /* [Q][Tb] */
  RateStep *sched;                          /* [n_out], written by the pass's first kernel */
  const void *hist;                         /* [source][Tb]: the pairs before the call (S16: words; otherwise float2 values) */
  const int *wg_first, *wg_count;           /* [n_wg] */
  int n_wg, P, Q;
  uint32_t frac, n_out, pairs;              /* n_out a multiple of 128 */
};

/* ---- what a source keeps between calls: its last rate_keep(P, Q) pairs, src_hist_words(format) words each.  Nothing else
 * computes a history's size.  The pass follows from the rate: Q > 1 the polyphase pass, else P > 1 the decimating pass, else
 * the tuning pass, which keeps nothing. */
RDSP_HD int rate_keep(int P, int Q) { return Q > 1 ? rate_tb(P, Q) : P > 1 ? DDC_HIST_PER_PHASE * P : 0; }

}  // namespace rdsp_tune

hipError_t rdsp_engine_tune_launch(const rdsp_tune::TuneParams &p, hipStream_t s);
hipError_t rdsp_engine_ddc_launch(const rdsp_tune::DdcParams &p, hipStream_t s);
hipError_t rdsp_engine_rate_launch(const rdsp_tune::RateParams &p, hipStream_t s);
/* after a filter bank, in its stream: the last `keep` of the call's `pairs` pairs of every source row -> hist (words for S16,
 * float2 values otherwise), and every receiver's phase += pairs dphi */
hipError_t rdsp_engine_source_finish_launch(const rdsp_tune::SourceParams &p, void *hist, uint32_t keep, uint32_t pairs, int n_sources, hipStream_t s);

#endif
