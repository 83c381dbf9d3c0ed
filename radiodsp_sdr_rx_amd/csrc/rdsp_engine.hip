/*
 * rdsp_engine.hip -- `AudioSDR SDR;` (RadioDSP_SDR_RX.ino:54; wired :81-86, configured :117-139, driven from
 * RDSP_controls.h:149-423) for n_channels receivers on one GPU, computing what the reference's engine computes.
 *
 * The engine is Derek Rowell's AudioSDR library, which is not in the reference tree; what the reference holds of it is
 * its compiled code in pre_compiled/RadioDSP_SDR_RX.ino.hex (AudioSDR::update at ITCM 0xe730).  The arithmetic below
 * follows that code stage by stage -- which products are rounded before they are added, which are fused, where it widens
 * to double, its truncating conversions -- so that, on the same int16 IQ, this object returns the int16 audio the
 * image's update() returns (tests/test_engine_kat.py: the known answers are the image's own, recorded under the
 * interpreter of tests/golden/).  It is a low-IF receiver: IQ / 32767 x gains -> [impulse blanker] -> IF band-pass
 * (4 biquad sections per rail) -> table oscillator shifts the carrier to 0 Hz -> I delayed 128 samples, Q through a
 * 257-tap Hilbert transformer, sum or difference picks the side band  (AM: second IF pass, shift by the IF, low-pass,
 * envelope; SAM: a PLL on the IF signal with the envelope detector as its out-of-lock fallback) -> audio band-pass
 * -> hang AGC (peak envelope, gain by a curve) -> ALS line enhancer (delayed-input LMS) -> x output gain x 32767.
 *
 * Mapping to the machine.  Every stage but the Hilbert transformer is a recursion in time that has to be evaluated in the
 * image's order, so the parallel axes are channels, rails and -- for the transformer -- samples; and a lone wave issues an
 * instruction every five cycles or so whatever it depends on, so a launch lasts as long as ONE workgroup's chain of
 * instructions per block, times the blocks.  Hence: few channels per workgroup (8), the sections of a cascade on the four
 * lanes of a quad (sample n enters section s at step n + s), everything that is a pure function of a recursion's state
 * (table look-ups, gain curve, conversions, pack) spread over all lanes behind a recursion reduced to its few dependent
 * operations, and the passes of a block on different waves, each a block behind the previous one's:
 *   rdsp_engine_front_pipe_kernel  SSB / CW, no blanker: waves 2 + 3 convert block s and rotate / store block s - 2, wave 0
 *                              runs the IF cascades of block s - 1 (16 rows x 4 sections), wave 1 the oscillator's phase
 *   rdsp_engine_front_kernel   blanker, AM, SAM: the same passes one after the other (the PLL and the blanker's running
 *                              average are long recursions of their own)
 *   rdsp_engine_hilbert_kernel eight outputs of one parity per lane, sliding windows in registers, LDS split by parity
 *   rdsp_engine_tail_pipe_kernel   waves 2 + 3 load block s and finish block s - 3 (gain by the curve, clamp, pack), wave 0
 *                              the audio cascade of block s - 1, wave 1 the AGC envelope of block s - 2
 *   rdsp_engine_tail_kernel    with the ALS filter: its 55-tap chain on the lanes of a quad (the four samples between two
 *                              tap moves), taps in registers
 * int16 rows enter and leave in coalesced 256-byte segments through LDS tiles at a 129-word pitch.  The three launches of a
 * call are stream-ordered; a call takes any number of 128-sample blocks up to the engine's max_blocks_per_call.  HBM
 * traffic is 8 B per sample of algorithm (int16 IQ in, int16 L = R out) plus 28 B of float intermediates (the ring and the
 * audio row): the path is bound by the latency of its recursions, not by bandwidth.
 *
 * Three of the engine's tables have no closed form (fifteen sets of four biquad sections, 64 Hilbert taps): the host
 * loads them (rdsp_engine_load_tables; tests take them from tests/golden/firmware_tables.npz); update() refuses to run
 * without them.  The sine table and the AGC's gain curve are generated here the way the library generates them.
 *
 * The hang AGC, the ALS filter and the output word are the pieces of rdsp_engine_laws.h, which the chain's engine-law
 * tail stage (rdsp_tail_engine.hip) calls too; the two tail kernels here keep their lanes, tiles and HBM layouts.
 *
 * The host object (settings, receiver groups, shared sources, state blobs, the C-ABI) is rdsp_engine_host.hip; it hands
 * rdsp_engine_launch, at the end of this file, one group's arguments (rdsp_engine_int.h).  Compiled with -ffp-contract=off: every fused operation below is written as one (fmaf / fma).
 */
#include <hip/hip_runtime.h>
#include <math.h>

#include "rdsp_engine_int.h"
#include "rdsp_engine_laws.h"
#include "rdsp_sync.h"

using namespace rdsp_eng;

namespace {

static_assert(BS == RDSP_BLOCK, "the tail kernels hand rdsp_engine_laws.h rows of BS samples");
constexpr int PITCH = BS + 1;
constexpr float TWO_PI_F = 6.2831854820251465f;   /* the float the image holds for 2 pi */
constexpr float RAD_PER_HZ = 0.00014247586659621447f; /* 2 pi / 44100, its float */

/* the oscillator: sin of a phase in [0, 2 pi) by linear interpolation in the 256-step table, through double as the image does */
/* trunc(RN(a / d)) for a >= 0 and d = the double of the image's 2 pi, without the division: k d is exact for k < 2^16 (a
 * 24-bit d), so floor(a / d) follows from two exact comparisons around the estimate a (1 / d); and the correctly rounded
 * quotient cannot lie across an integer from the true one, because a is either exactly k d or at least an ulp of a away
 * from it, which is more than half an ulp of the quotient (tests/test_host_logic.py walks every k and its neighbours) */
__device__ __forceinline__ int index_of_phase(double a) {
  const double d = (double)TWO_PI_F;
  int k = (int)(a * (1.0 / d));
  if ((double)k * d > a) k--;
  else if ((double)(k + 1) * d <= a) k++;
  return k;
}
__device__ __forceinline__ float table_sin(const float *sine, float ph) {
  const int idx = index_of_phase((double)ph * 65535.0);
  const int hi = (idx >> 8) & 0xff;
  const float lo = (float)(unsigned)(idx & 0xff);
  const float t0 = sine[hi], t1 = sine[hi + 1];
  return (float)fma((double)((t1 - t0) * lo), 0.00390625, (double)t0);
}
__device__ __forceinline__ float dpp_up1(float v) { /* lane s of a quad takes lane s - 1's value: quad_perm [0,0,1,2] */
  const int w = __builtin_bit_cast(int, v);
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(w, w, 0x90, 0xF, 0xF, false)); /* every lane has a source: `old` is never kept */
}
__device__ __forceinline__ float quick_root_guess(float p) { return __uint_as_float((__float_as_uint(p) >> 1) + 0x1fa00000u + 0x1b4000u + 3886u); }
__device__ __forceinline__ float quick_sqrt1(float p) { const float g = quick_root_guess(p); return (p / g + g) * 0.5f; }
__device__ __forceinline__ float quick_sqrt2(float p) { const float y = quick_sqrt1(p); return (p / y + y) * 0.5f; }

/* ---- stages of a cascade on neighbouring lanes --------------------------------------------------------------------
 * arm_biquad_cascade_df1_f32 runs section after section over the block; the result is the same when sample n enters
 * section s at step n + s.  Lane s of a quad holds section s of one row of the tile (its five coefficients and four
 * state words) and at step i works on sample i - s, taking its input from lane s - 1's previous output (one DPP move):
 * a block costs 131 steps of ONE section instead of 128 of four, and a row occupies four lanes. */
struct Section {
  float b0, b1, b2, a1, a2, x1, x2, y1, y2;
  __device__ __forceinline__ void load(const float *coef5, const float *state4, bool clear) {
    b0 = coef5[0]; b1 = coef5[1]; b2 = coef5[2]; a1 = coef5[3]; a2 = coef5[4];
    x1 = clear ? 0.0f : state4[0]; x2 = clear ? 0.0f : state4[1]; y1 = clear ? 0.0f : state4[2]; y2 = clear ? 0.0f : state4[3];
  }
  __device__ __forceinline__ void store(float *state4) const { state4[0] = x1; state4[1] = x2; state4[2] = y1; state4[3] = y2; }
  __device__ __forceinline__ float eval(float x) const { /* products rounded, summed left to right */
    float y = b0 * x;
    y = y + b1 * x1;
    y = y + b2 * x2;
    y = y + a1 * y1;
    y = y + a2 * y2;
    return y;
  }
  __device__ __forceinline__ void commit(float x, float y) { x2 = x1; x1 = x; y2 = y1; y1 = y; }
};
/* one block of one tile row through the cascade, in place; called by all four lanes of the row's quad */
/* LEAN: the form for the kernels that carry blanker / detector code beside it (fewer registers: two workgroups per CU) */
template <bool LEAN = false>
__device__ __forceinline__ void cascade_row(Section &sec, float *row, int s) {
  float yprev = 0.0f, xnext = row[0];
#pragma unroll 4
  for (int i = 0; i < BS + 3; i++) {
    const int n = i - s;
    const float up = dpp_up1(yprev);
    const float xin = xnext;
    xnext = row[i + 1 < BS ? i + 1 : BS - 1]; /* asked for a step ahead: the read's latency passes behind this step's arithmetic
                                               * (the row is also written below, so the compiler will not move the read itself) */
    const float x = s == 0 ? xin : up;
    const float y = sec.eval(x);
    const bool live = n >= 0 && n < BS;
    if (live) {
      sec.commit(x, y);
      yprev = y;
    }
    if constexpr (LEAN) {
      if (live && s == 3) row[n] = y;
    } else {
      row[(live && s == 3) ? n : BS] = y; /* the last section's lane writes the sample; every other lane the row's spare word */
    }
  }
}
/* the oscillator in two passes: the phase recursion alone (one lane per channel: a float add and the wrap), then cosine,
 * sine and the complex product for every sample of the tile in parallel -- they are pure functions of the phase */
__device__ __forceinline__ void phase_row(float &ph, float inc, float *out) {
  for (int t = 0; t < BS; t++) { /* both wrapped candidates are formed and one value selected: as branches the three cases cost
                                  * the lone wave more instructions (exec-mask bookkeeping) than the arithmetic */
    out[t] = ph;
    ph = ph + inc;
    const float down = ph - TWO_PI_F, up = ph + TWO_PI_F;
    ph = ph > TWO_PI_F ? down : (ph < 0.0f ? up : ph);
  }
}
__device__ __forceinline__ void rotate_sample(const float *sine, float ph, float &x, float &y) {
  float pc = (float)((double)ph + 1.5707963267948966);
  if (pc >= TWO_PI_F) pc -= TWO_PI_F;
  if (pc < 0.0f) pc += TWO_PI_F;
  const float c = table_sin(sine, pc);
  float ps = ph >= TWO_PI_F ? ph - TWO_PI_F : ph;
  if (ps < 0.0f) ps += TWO_PI_F;
  const float s = table_sin(sine, ps);
  const float xi = x, yq = y;
  x = fmaf(xi, c, -(s * yq));
  y = fmaf(yq, c, xi * s);
}

/* v / 32767.0 correctly rounded without the division: q0 = v y, r = v - 32767 q0 (exact, fused), q = q0 + r y with
 * y = RN(1 / 32767) -- equal to the IEEE quotient for every int16 v (tests/test_host_logic.py tries all 65 536) */
__device__ __forceinline__ double over_32767(int v) {
  const double y = 1.0 / 32767.0, x = (double)v;
  const double q0 = x * y;
  return fma(fma(-q0, 32767.0, x), y, q0);
}

/* ---- front: conversion, blanker, IF filter, frequency shift (SSB / CW) or the AM / SAM detectors ----------------------
 * 8 channels = 16 tile rows (channel, rail) per workgroup of four waves -- a launch's duration is one workgroup's chain
 * of blocks whatever the grid, so the fewer channels a workgroup carries the shorter it is, down to what the recursions
 * need.  Per block: conversion and the mixer's table work spread over all 256 lanes (element e = lane + 256 j: consecutive
 * lanes on consecutive samples of a row); the cascades with a quad per row on waves 0 and 1 while wave 2 runs the
 * oscillator's phase, one lane per channel; the PLL and the blanker -- true recursions -- on one lane per channel or row. */
constexpr int FW = 256, FCH = 8, PW = 256; /* threads, channels per workgroup; PW: threads of the pipelined kernels (four waves, as FW) */
template <bool NB>
__global__ __launch_bounds__(FW, 2) void rdsp_engine_front_kernel(const EngParams p) {
  __shared__ float tf[2 * FCH][PITCH];
  __shared__ float phs[FCH][PITCH];
  __shared__ int locked_of[FCH];
  __shared__ float sine[257];                                     /* the oscillator's table: the PLL reads it twice per sample of a dependent chain */
  const int tid = threadIdx.x, c0 = blockIdx.x * FCH;
  for (int i = tid; i < 257; i += FW) sine[i] = p.sine[i];
  const bool casc = tid < 8 * FCH;                              /* cascade role: section sct of tile row `row` */
  const int row = (tid >> 2) & (2 * FCH - 1), sct = tid & 3;
  const int rch = min(c0 + (row >> 1), p.n_channels - 1);
  const bool row_valid = casc && c0 + (row >> 1) < p.n_channels;
  const bool ssb = p.mode <= 3 || p.mode == 6, am = p.mode == 4 || p.mode == 5;
  Section pre, amf;
  pre.load(p.sets + 20 * p.pre_set + 5 * sct, p.st + (size_t)rch * NF + ST_PRE + 16 * (row & 1) + 4 * sct, (p.resets & RESET_PRE) != 0);
  amf.load(p.sets + 20 * 13 + 5 * sct, p.st + (size_t)rch * NF + ST_AM + 16 * (row & 1) + 4 * sct, false);
  /* serial role: lane 128 + c owns channel c0 + c's scalars (wave 2, beside the cascades' waves 0 and 1) */
  const bool ser = tid >= 128 && tid < 128 + FCH;
  const int sc = (tid - 128) & (FCH - 1);
  const int sch = min(c0 + sc, p.n_channels - 1);
  const bool ser_valid = ser && c0 + sc < p.n_channels;
  float *sst = p.st + (size_t)sch * NF;
  float nco = sst[ST_NCO], amph = sst[ST_AMPH];
  float sam_c = sst[ST_SAM_COS], sam_s = sst[ST_SAM_SIN], sam_u = sst[ST_SAM_U], sam_err = sst[ST_SAM_ERR], sam_hz = sst[ST_SAM_HZ],
        sam_ph = sst[ST_SAM_PH];
  int sam_locked = __float_as_int(sst[ST_SAM_LOCK]);
  /* the blanker's lines: three blocks of I, Q and mask per channel in LDS, slot (n / 128 + nb_base) % 3 holding samples
   * n .. n + 127 of the 384-sample line, so that a block boundary moves a base instead of 768 words */
  constexpr int NBP = NB ? 388 : 1;
  __shared__ float nbl[NB ? 3 : 1][NB ? FCH : 1][NBP];
  __shared__ float nbmag[NB ? FCH : 1][NB ? 180 : 1];
  int nb_base = 0;
  auto nbx = [&](int n) { int sl = (n >> 7) + nb_base; sl = sl >= 3 ? sl - 3 : sl; return sl * 128 + (n & 127); };
  float nb_avg = sst[ST_NB_AVG], nb_last = sst[ST_NB_LAST];
  int nb_hit = __float_as_int(sst[ST_NB_HIT]);
  if constexpr (NB) {
    for (int e = tid; e < 3 * FCH * 384; e += FW) { /* HBM keeps them in line order: I, Q, mask */
      const int k = e / (FCH * 384), r = e - k * (FCH * 384), cl = r / 384, i = r - cl * 384;
      nbl[k][cl][i] = c0 + cl < p.n_channels ? p.nb[(size_t)(c0 + cl) * NB_WORDS + 384 * k + i] : (k == 2 ? 1.0f : 0.0f);
    }
    __syncthreads();
  }
  const float nco_inc = -(p.tuning_offset * RAD_PER_HZ), am_inc = -p.if_centre * RAD_PER_HZ;
  constexpr int EP = FCH * BS / FW; /* elements (int16 pairs, complex samples) per lane and pass */

  for (int b = 0; b < p.n_blocks; b++) {
    for (int j = 0; j < EP; j++) { /* 0xe7b4: / 32767 and the rail's gain, in double; one int16 pair per element */
      const int e = tid + FW * j, cl = e >> 7, t = e & 127;
      const int w = c0 + cl < p.n_channels ? p.iq[(size_t)(c0 + cl) * p.in_stride + (size_t)b * BS + t] : 0;
      tf[2 * cl][t] = (float)(over_32767((int)(int16_t)(w & 0xffff)) * (double)p.gain_i);
      tf[2 * cl + 1][t] = (float)(over_32767(w >> 16) * (double)p.gain_q);
    }
    __syncthreads();
    if constexpr (NB) { /* 0xe14c: two blocks of delay; |I + jQ| against its running average; blanking mask with a taper */
      nb_base = nb_base == 2 ? 0 : nb_base + 1;                    /* the oldest block's slot takes the new one */
      for (int j = 0; j < EP; j++) {
        const int e = tid + FW * j, cl = e >> 7, t = e & 127, at = nbx(256 + t);
        nbl[0][cl][at] = tf[2 * cl][t]; nbl[1][cl][at] = tf[2 * cl + 1][t]; nbl[2][cl][at] = 1.0f;
      }
      __syncthreads();
      for (int e = tid; e < FCH * 178; e += FW) {                  /* the magnitudes are pure functions of the samples */
        const int cl = e / 178, n = 78 + e - cl * 178, at = nbx(n);
        const float vi = nbl[0][cl][at], vq = nbl[1][cl][at];
        nbmag[cl][n - 78] = quick_sqrt1(fmaf(vi, vi, vq * vq));
      }
      __syncthreads();
      if (ser) { /* what is a recursion: the running average and what it decides, then the taper in front of every 0 -> 1 step */
        float *mask = nbl[2][sc];
        nb_hit = 0;
        int zeroed_to = 67;                      /* hits come in rising order: what an earlier one of this pass zeroed stays zero */
        for (int n = 78; n < 256; n++) {
          const float limit = nb_avg * p.nb_ratio;
          nb_last = nbmag[sc][n - 78];
          if (limit < nb_last) {
            if (-p.nb_before <= p.nb_after) {
              const int lo = max(n - p.nb_before, zeroed_to + 1), hi = n + p.nb_after;
              for (int j = lo; j <= hi; j++) mask[nbx(j)] = 0.0f;
              zeroed_to = max(zeroed_to, hi);
            }
            nb_hit = 1;
          }
          nb_avg = fmaf(nb_avg, p.nb_keep, nb_last * p.nb_new);
        }
        const float taper[7] = {0.933f, 0.75f, 0.5f, 0.25f, 0.067f, 0.0f, 0.0f};
        for (int i = 128; i < 256; i++)
          if (mask[nbx(i)] == 1.0f && mask[nbx(i - 1)] == 0.0f)
            for (int j = 0; j < 7; j++) mask[nbx(i - 7 + j)] = taper[j];
      }
      __syncthreads();
      for (int j = 0; j < EP; j++) {
        const int e = tid + FW * j, cl = e >> 7, t = e & 127, at = nbx(t);
        const float mk = nbl[2][cl][at];
        tf[2 * cl][t] = mk * nbl[0][cl][at]; tf[2 * cl + 1][t] = mk * nbl[1][cl][at];
      }
      __syncthreads();
    }
    if (casc) cascade_row<true>(pre, tf[row], sct);
    else if (ser && ssb) phase_row(nco, nco_inc, phs[sc]);       /* 0xe94e: the phase falls by the tuning offset */
    __syncthreads();
    if (ssb) {
      for (int j = 0; j < EP; j++) {
        const int e = tid + FW * j, cl = e >> 7, t = e & 127;
        float x = tf[2 * cl][t], y = tf[2 * cl + 1][t];
        rotate_sample(sine, phs[cl][t], x, y);
        tf[2 * cl][t] = x; tf[2 * cl + 1][t] = y;
      }
      __syncthreads();
      const uint32_t at = p.pos + (uint32_t)b * BS, m = p.ring_size - 1;
      for (int j = 0; j < 2 * EP; j++) { /* into the rings: tile row r is (channel c0 + r / 2, rail r & 1) */
        const int e = tid + FW * j, r = e >> 7, t = e & 127;
        if (c0 + (r >> 1) < p.n_channels)
          ((r & 1) ? p.ring_q : p.ring_i)[(size_t)(c0 + (r >> 1)) * p.ring_size + ((at + (uint32_t)t) & m)] = tf[r][t];
      }
    } else if (am) {
      if (casc) cascade_row<true>(pre, tf[row], sct);                  /* 0xec1c: the IF filter a second time */
      __syncthreads();
      if (p.mode == 5) { /* 0xe390: PLL on the IF signal, one lane per channel */
        if (ser) {
          const float HALF_PI = 1.5707963705062866f, A1 = 0.97239410877227783f, A3 = -0.19194795191287994f;
          float *ri = tf[2 * sc], *rq = tf[2 * sc + 1];
          for (int t = 0; t < BS; t++) {
            const float x = ri[t], q = rq[t];
            const float re = fmaf(x, sam_c, q * sam_s), im = fmaf(q, sam_c, -(sam_s * x));
            float err;
            if (re == 0.0f) err = im > 0.0f ? HALF_PI : (im < 0.0f ? -HALF_PI : 0.0f);
            else if (fabsf(re) > fabsf(im)) {
              const float z = im / re;
              err = fmaf(z, z * A3, A1) * z;
              if (!(re > 0.0f)) err = (float)(im >= 0.0f ? (double)err + 3.1415926535897931 : (double)err - 3.1415926535897931);
            } else {
              const float z = re / im;
              err = fmaf(-z, fmaf(z, z * A3, A1), im > 0.0f ? HALF_PI : -HALF_PI);
            }
            const float u = fmaf(err, p.sam_ga, p.sam_gb * sam_err);
            const double phd = fma((double)(u + sam_u), 0.5, (double)sam_ph);
            sam_hz = fmaf(p.sam_keep, sam_hz, (u * p.sam_hz_per_rad) * p.sam_new);
            sam_ph = (float)phd;
            if ((double)sam_ph >= 3.1415926535897931) sam_ph -= TWO_PI_F;
            if ((double)sam_ph < -3.1415926535897931) sam_ph += TWO_PI_F;
            sam_locked = sam_hz > p.sam_lock_lo ? (sam_hz < p.sam_lock_hi) : 0;
            float pc = (float)((double)sam_ph + 1.5707963267948966);
            if (pc >= TWO_PI_F) pc -= TWO_PI_F;
            if (pc < 0.0f) pc += TWO_PI_F;
            sam_c = table_sin(sine, pc);
            float ps = sam_ph >= TWO_PI_F ? sam_ph - TWO_PI_F : sam_ph;
            if (ps < 0.0f) ps += TWO_PI_F;
            sam_s = table_sin(sine, ps);
            if (sam_locked) {
              ri[t] = fmaf(x, sam_c, q * sam_s);
              rq[t] = fmaf(-x, sam_s, q * sam_c);
            }
            sam_u = u; sam_err = err;
          }
          locked_of[sc] = sam_locked;
        }
      } else if (ser) locked_of[sc] = 0;
      __syncthreads();
      /* AM, and SAM out of lock (0xed02): shift by the IF centre, low-pass, envelope.  A channel in lock keeps the rotated
       * I rail as its audio and none of the detector's state moves */
      if (ser && !locked_of[sc]) phase_row(amph, am_inc, phs[sc]);
      __syncthreads();
      for (int j = 0; j < EP; j++) {
        const int e = tid + FW * j, cl = e >> 7, t = e & 127;
        if (locked_of[cl]) continue;
        float x = tf[2 * cl][t], y = tf[2 * cl + 1][t];
        rotate_sample(sine, phs[cl][t], x, y);
        tf[2 * cl][t] = x; tf[2 * cl + 1][t] = y;
      }
      __syncthreads();
      if (casc) {
        const bool detect = !locked_of[row >> 1];
        const Section keep = amf;
        cascade_row<true>(amf, detect ? tf[row] : phs[row >> 1], sct);   /* the quads of a locked channel run on a row nobody reads ... */
        if (!detect) amf = keep;                                 /* ... and keep their state */
      }
      __syncthreads();
      for (int j = 0; j < EP; j++) {
        const int e = tid + FW * j, cl = e >> 7, t = e & 127;
        if (locked_of[cl]) continue;
        const float x = tf[2 * cl][t], y = tf[2 * cl + 1][t];
        tf[2 * cl][t] = quick_sqrt2(fmaf(x, x, y * y));
      }
      __syncthreads();
      for (int j = 0; j < EP; j++) { /* the demodulated audio is in the I rows */
        const int e = tid + FW * j, cl = e >> 7, t = e & 127;
        if (c0 + cl < p.n_channels) p.audio[(size_t)(c0 + cl) * p.audio_stride + (size_t)b * BS + t] = tf[2 * cl][t];
      }
    }
    __syncthreads();
  }
  if (row_valid) {
    pre.store(p.st + (size_t)rch * NF + ST_PRE + 16 * (row & 1) + 4 * sct);
    if (am) amf.store(p.st + (size_t)rch * NF + ST_AM + 16 * (row & 1) + 4 * sct);
  }
  if (ser_valid) {
    sst[ST_NCO] = nco; sst[ST_AMPH] = amph;
    sst[ST_SAM_COS] = sam_c; sst[ST_SAM_SIN] = sam_s; sst[ST_SAM_U] = sam_u; sst[ST_SAM_ERR] = sam_err; sst[ST_SAM_HZ] = sam_hz;
    sst[ST_SAM_PH] = sam_ph; sst[ST_SAM_LOCK] = __int_as_float(sam_locked);
  }
  if constexpr (NB) {
    if (ser_valid) { sst[ST_NB_AVG] = nb_avg; sst[ST_NB_LAST] = nb_last; sst[ST_NB_HIT] = __int_as_float(nb_hit); }
    __syncthreads();
    for (int e = tid; e < 3 * FCH * 384; e += FW) {
      const int k = e / (FCH * 384), r = e - k * (FCH * 384), cl = r / 384, i = r - cl * 384;
      if (c0 + cl < p.n_channels) p.nb[(size_t)(c0 + cl) * NB_WORDS + 384 * k + i] = nbl[k][cl][nbx(i)];
    }
  }
}

/* ---- the same front stage for the SSB / CW modes without the blanker, as a pipeline of waves ------------------------
 * A lone wave issues an instruction every five cycles or so whatever it depends on, so a block costs its workgroup the SUM
 * of its passes' instruction counts -- unless the passes run on different waves at the same time.  Here they do, each on
 * the block behind the previous one's: waves 2 and 3 convert block s into tile slot s & 3 and rotate / store block s - 2
 * out of slot (s - 2) & 3 (the longest pass of the step: knocking the rotation out cuts 2.2 us of 8.4 per block, knocking
 * the cascade out nothing; six waves per workgroup instead of four ran 1.5 x slower), wave 0 runs the cascades of block s - 1, wave 1 the oscillator's phase of block s - 1; one
 * barrier per step.  A step then lasts as long as its longest pass (the cascade: 131 dependent steps), and the arithmetic
 * of every sample is what it was. */
__global__ __launch_bounds__(PW, 2) void rdsp_engine_front_pipe_kernel(const EngParams p) {
  __shared__ float tf[4][2 * FCH][PITCH];
  __shared__ float phs[4][FCH][PITCH];
  __shared__ float sine[257];                                     /* the oscillator's table beside the data it turns */
  const int tid = threadIdx.x, wave = tid >> 6, c0 = blockIdx.x * FCH;
  for (int i = tid; i < 257; i += PW) sine[i] = p.sine[i];
  __syncthreads();
  const int row = (tid >> 2) & (2 * FCH - 1), sct = tid & 3;      /* wave 0: section sct of tile row `row` */
  const int rch = min(c0 + (row >> 1), p.n_channels - 1);
  Section pre;
  pre.load(p.sets + 20 * p.pre_set + 5 * sct, p.st + (size_t)rch * NF + ST_PRE + 16 * (row & 1) + 4 * sct, (p.resets & RESET_PRE) != 0);
  const int sc = tid & (FCH - 1);                                 /* wave 1, lanes 64 ... 64 + FCH - 1: channel sc's oscillator */
  const bool ser = wave == 1 && (tid & 63) < FCH;
  const int sch = min(c0 + sc, p.n_channels - 1);
  float nco = p.st[(size_t)sch * NF + ST_NCO];
  const float nco_inc = -(p.tuning_offset * RAD_PER_HZ);
  const int wl = tid - 128;                                       /* waves 2 and 3: 128 lanes for the element passes */
  constexpr int EP = FCH * BS / (PW - 128);
  const uint32_t m = p.ring_size - 1;
  for (int step = 0; step < p.n_blocks + 2; step++) {
    if (wave >= 2) {
      if (step < p.n_blocks) { /* 0xe7b4: block `step` comes in */
        float (*t0)[PITCH] = tf[step & 3];
        for (int j = 0; j < EP; j++) {
          const int e = wl + (PW - 128) * j, cl = e >> 7, t = e & 127;
          const int w = c0 + cl < p.n_channels ? p.iq[(size_t)(c0 + cl) * p.in_stride + (size_t)step * BS + t] : 0;
          t0[2 * cl][t] = (float)(over_32767((int)(int16_t)(w & 0xffff)) * (double)p.gain_i);
          t0[2 * cl + 1][t] = (float)(over_32767(w >> 16) * (double)p.gain_q);
        }
      }
      const int b = step - 2;
      if (b >= 0) { /* 0xe94e: block step - 2, filtered and with its phases known, is rotated and leaves for the rings */
        float (*t2)[PITCH] = tf[b & 3];
        const float (*ph)[PITCH] = phs[b & 3];
        const uint32_t at = p.pos + (uint32_t)b * BS;
        for (int j = 0; j < EP; j++) {
          const int e = wl + (PW - 128) * j, cl = e >> 7, t = e & 127;
          float x = t2[2 * cl][t], y = t2[2 * cl + 1][t];
          rotate_sample(sine, ph[cl][t], x, y);
          if (c0 + cl < p.n_channels) {
            const size_t o = (size_t)(c0 + cl) * p.ring_size + ((at + (uint32_t)t) & m);
            p.ring_i[o] = x; p.ring_q[o] = y;
          }
        }
      }
    } else {
      const int b = step - 1;
      if (b >= 0 && b < p.n_blocks) {
        if (wave == 0) cascade_row(pre, tf[b & 3][row], sct);
        else if (ser) phase_row(nco, nco_inc, phs[b & 3][sc]);
      }
    }
    __syncthreads();
  }
  if (wave == 0 && c0 + (row >> 1) < p.n_channels) pre.store(p.st + (size_t)rch * NF + ST_PRE + 16 * (row & 1) + 4 * sct);
  if (ser && c0 + sc < p.n_channels) p.st[(size_t)sch * NF + ST_NCO] = nco;
}

/* ---- 0xea7e: I delayed by 128, Q through the 257-tap Hilbert transformer (odd taps, antisymmetric), side band by sign ---
 * out[t] = sum_k h[k] (q[t - 1 - 2k] - q[t - 255 + 2k]), k = 0 .. 63 in this order, one fused multiply-add each.  An output
 * only meets samples of the other parity, and the outputs t, t + 2, ... meet the same ones shifted by a tap: a lane takes
 * EIGHT outputs of one parity (t = 2 (8 l + j) + p), keeps the two sliding windows in registers, and reads 142 words of
 * LDS for them instead of 1024.  The window of the ring sits in LDS split by parity, index m at m + m / 8: lanes are 8
 * indices apart, so their reads fall 9 words apart (no bank conflicts) and every offset is an immediate.  The delayed I
 * samples come in, and the audio leaves, through a row at pitch 17 for 16 (coalesced 256-byte segments in HBM). */
constexpr int HB_OUT = 2048;                      /* outputs per workgroup */
constexpr int HB_M = (HB_OUT + 256) / 2;          /* samples per parity in the window */
template <int P>
__device__ __forceinline__ void hilbert_eight(const float *par, const float *h, float (&acc)[8]) {
  /* par: the parity array this lane's outputs read (the other parity), already offset by 9 l; P: the outputs' parity */
  float U[8], L[8];
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const int ru = j + 127 + P, rl = j + P;
    U[j] = par[ru + (ru >> 3)];
    L[j] = par[rl + (rl >> 3)];
    acc[j] = 0.0f;
  }
#pragma unroll
  for (int k = 0; k < 64; k++) {
    const float hk = h[k];
#pragma unroll
    for (int j = 0; j < 8; j++) acc[j] = fmaf(hk, U[j] - L[j], acc[j]);
    if (k < 63) { /* tap k + 1: the upper window moves one index down, the lower one up */
#pragma unroll
      for (int j = 7; j > 0; j--) U[j] = U[j - 1];
#pragma unroll
      for (int j = 0; j < 7; j++) L[j] = L[j + 1];
      const int ru = 127 + P - (k + 1), rl = 7 + P + (k + 1);
      U[0] = par[ru + (ru >> 3)];
      L[7] = par[rl + (rl >> 3)];
    }
  }
}
__global__ __launch_bounds__(256) void rdsp_engine_hilbert_kernel(const EngParams p) {
  __shared__ float par[2][HB_M + HB_M / 8];
  __shared__ float row[HB_OUT + HB_OUT / 16];
  __shared__ float h[64];
  const int tid = threadIdx.x, ch = blockIdx.y;
  const uint32_t t0 = blockIdx.x * (uint32_t)HB_OUT, m = p.ring_size - 1, n = (uint32_t)p.n_blocks * BS;
  const float *rq = p.ring_q + (size_t)ch * p.ring_size, *ri = p.ring_i + (size_t)ch * p.ring_size;
  for (int i = tid; i < HB_OUT + 256; i += 256) { /* window sample i = t0 - 256 + i, by parity */
    const int mm = i >> 1;
    par[i & 1][mm + (mm >> 3)] = rq[(p.pos + t0 - 256u + (uint32_t)i) & m];
  }
  for (int i = tid; i < HB_OUT; i += 256) row[i + (i >> 4)] = ri[(p.pos + t0 + (uint32_t)i - 128u) & m];
  if (tid < 64) h[tid] = p.hilbert[tid];
  __syncthreads();
  const int P = tid >> 7, lp = tid & 127;             /* waves 0, 1: the even outputs; waves 2, 3: the odd ones */
  float acc[8];
  /* output o = 2 (8 lp + j) + P reads the window at i = o + 255 - 2k and o + 1 + 2k: parity 1 - P, indices
   * 8 lp + j + 127 + P - k and 8 lp + j + P + k */
  if (P == 0) hilbert_eight<0>(par[1] + 9 * lp, h, acc);
  else hilbert_eight<1>(par[0] + 9 * lp, h, acc);
  const bool minus = p.mode == 6 || (p.mode & ~2) == 1;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    float *slot = &row[17 * lp + 2 * j + P];          /* o + o / 16 with o = 16 lp + 2 j + P */
    *slot = minus ? *slot - acc[j] : *slot + acc[j];
  }
  __syncthreads();
  for (int i = tid; i < HB_OUT; i += 256)
    if (t0 + (uint32_t)i < n) p.audio[(size_t)ch * p.audio_stride + t0 + (uint32_t)i] = row[i + (i >> 4)];
}

/* ---- tail: audio band-pass (0xd944), AGC (0xdb58), ALS (0xda24), output (0xebfa) ------------------------------------- */

/* 8 channels (16 with the ALS filter) per workgroup of four waves.  Per block: the audio cascade with a quad per channel (wave 0); the AGC's
 * envelope -- the only true recursion in it -- on one lane per channel (wave 1), which leaves for every sample the
 * envelope value its gain is looked up from (or "none yet": the gain carried in); gain, clamp and pack are then pure
 * functions and run on all lanes. */
template <bool ALS>
__global__ __launch_bounds__(FW, 2) void rdsp_engine_tail_kernel(const EngParams p) {
  constexpr int TCH = ALS ? 16 : 8; /* channels per workgroup (measured: 8 is 12 % faster than 16 without the ALS filter, half as fast with it) */
  __shared__ float ta[TCH][PITCH];
  __shared__ float ge[TCH][PITCH];
  __shared__ float curve[130];
  __shared__ float g_in[TCH];
  constexpr int LP = 260;                 /* pitch of a channel's 256-sample ALS line */
  __shared__ float line[ALS ? TCH : 1][ALS ? LP : 1];
  const int tid = threadIdx.x, c0 = blockIdx.x * TCH;
  /* ALS role: wave 1 as 16 quads, quad ac on channel c0 + ac; its lane aq works on every fourth sample */
  const bool als_lane = ALS && (tid >> 6) == 1;
  const int ac = (tid >> 2) & (TCH - 1), aq = tid & 3;
  const int ach = min(c0 + ac, p.n_channels - 1);
  float w[ALS ? RDSP_ENG_ALS_TAPS : 1];
  const bool casc = tid < 4 * TCH;
  const int row = (tid >> 2) & (TCH - 1), sct = tid & 3;
  const int rch = min(c0 + row, p.n_channels - 1);
  Section aud;
  aud.load(p.sets + 20 * p.audio_set + 5 * sct, p.st + (size_t)rch * NF + ST_AUDIO + 4 * sct, (p.resets & RESET_AUDIO) != 0);
  const bool ser = tid >= 64 && tid < 64 + TCH;
  const int sc = (tid - 64) & (TCH - 1);
  const bool ser_valid = ser && c0 + sc < p.n_channels;
  const int sch = min(c0 + sc, p.n_channels - 1);
  float *sst = p.st + (size_t)sch * NF + ST_AGC_ENV;
  EngineAgcState agc;
  agc.load(sst);
  for (int i = tid; i < 130; i += FW) curve[i] = p.curve[i];
  if constexpr (ALS) {
    if (als_lane) {
      const float *a = p.als + (size_t)ach * ALS_WORDS;
      const bool clear = (p.resets & RESET_ALS) != 0;
      for (int i = aq; i < 256; i += 4) line[ac][i] = clear ? 0.0f : a[i];
#pragma unroll
      for (int k = 0; k < RDSP_ENG_ALS_TAPS; k++) w[k] = clear ? 0.0f : a[256 + k];
    }
  }
  constexpr int EP = TCH * BS / FW;
  for (int b = 0; b < p.n_blocks; b++) {
    __syncthreads();
    for (int j = 0; j < EP; j++) {
      const int e = tid + FW * j, r = e >> 7, t = e & 127;
      ta[r][t] = c0 + r < p.n_channels ? p.audio[(size_t)(c0 + r) * p.audio_stride + (size_t)b * BS + t] : 0.0f;
    }
    __syncthreads();
    if (p.audio_on) {
      if (casc) cascade_row<true>(aud, ta[row], sct);
      __syncthreads();
    }
    if (p.agc_on) {
      if (ser) {
        g_in[sc] = agc.g;
        agc_envelope(agc, p.agc, curve, ta[sc], ge[sc]);
      }
      __syncthreads();
      for (int j = 0; j < EP; j++) {
        const int e = tid + FW * j, r = e >> 7, t = e & 127;
        ta[r][t] = agc_gain_clamp(p.agc, curve, ge[r][t], g_in[r], ta[r][t]);
      }
      __syncthreads();
    }
    if constexpr (ALS) {
      /* the line: the previous block, then this one (samples 128 .. 255) */
      if (als_lane) {
        float *x = line[ac], *rowp = ta[ac];
        for (int i = aq; i < 128; i += 4) { x[i] = x[i + 128]; x[i + 128] = rowp[i]; }
        wg_sync<1>();
        als_block<128>(w, x, rowp, aq, p.als_notch, p.als_adaptive);
      }
      __syncthreads();
    }
    for (int j = 0; j < EP; j++) {
      const int e = tid + FW * j, r = e >> 7, t = e & 127;
      if (c0 + r < p.n_channels) p.out[(size_t)(c0 + r) * p.out_stride + (size_t)b * BS + t] = engine_out_word(ta[r][t], p.output_gain, p.mute);
    }
  }
  if (casc && c0 + row < p.n_channels) aud.store(p.st + (size_t)rch * NF + ST_AUDIO + 4 * sct);
  if (ser_valid) agc.store(sst);
  if constexpr (ALS) {
    if (als_lane && c0 + ac < p.n_channels) {
      float *a = p.als + (size_t)ach * ALS_WORDS;
      for (int i = aq; i < 256; i += 4) a[i] = line[ac][i];
      if (aq == 0) {
#pragma unroll
        for (int k = 0; k < RDSP_ENG_ALS_TAPS; k++) a[256 + k] = w[k];
      }
    }
  }
}

/* The tail stage without the ALS filter as a pipeline of waves (see rdsp_engine_front_pipe_kernel): waves 2 and 3 bring
 * block s in and send block s - 3 out (gain by the curve, clamp, pack), wave 0 runs the audio cascade of block s - 1,
 * wave 1 the AGC's envelope of block s - 2. */
__global__ __launch_bounds__(PW, 2) void rdsp_engine_tail_pipe_kernel(const EngParams p) {
  constexpr int TCH = 8;
  __shared__ float ta[4][TCH][PITCH];
  __shared__ float ge[4][TCH][PITCH];
  __shared__ float g_in[4][TCH];
  __shared__ float curve[130];
  const int tid = threadIdx.x, wave = tid >> 6, c0 = blockIdx.x * TCH;
  const int row = (tid >> 2) & (TCH - 1), sct = tid & 3;
  const bool casc = wave == 0 && tid < 4 * TCH;
  const int rch = min(c0 + row, p.n_channels - 1);
  Section aud;
  aud.load(p.sets + 20 * p.audio_set + 5 * sct, p.st + (size_t)rch * NF + ST_AUDIO + 4 * sct, (p.resets & RESET_AUDIO) != 0);
  const int sc = tid & (TCH - 1);
  const bool ser = wave == 1 && (tid & 63) < TCH;
  const int sch = min(c0 + sc, p.n_channels - 1);
  float *sst = p.st + (size_t)sch * NF + ST_AGC_ENV;
  EngineAgcState agc;
  agc.load(sst);
  for (int i = tid; i < 130; i += PW) curve[i] = p.curve[i];
  const int wl = tid - 128;
  constexpr int EP = TCH * BS / (PW - 128);
  __syncthreads();
  for (int step = 0; step < p.n_blocks + 3; step++) {
    if (wave >= 2) {
      if (step < p.n_blocks) {
        float (*t0)[PITCH] = ta[step & 3];
        for (int j = 0; j < EP; j++) {
          const int e = wl + (PW - 128) * j, r = e >> 7, t = e & 127;
          t0[r][t] = c0 + r < p.n_channels ? p.audio[(size_t)(c0 + r) * p.audio_stride + (size_t)step * BS + t] : 0.0f;
        }
      }
      const int b = step - 3;
      if (b >= 0) { /* gain, clamp (0xdc10), then 0xebfa: x output gain x 32767 toward zero, the low half-word, on both outputs */
        const float (*t3)[PITCH] = ta[b & 3];
        const float (*e3)[PITCH] = ge[b & 3];
        for (int j = 0; j < EP; j++) {
          const int e = wl + (PW - 128) * j, r = e >> 7, t = e & 127;
          float y = t3[r][t];
          if (p.agc_on) y = agc_gain_clamp(p.agc, curve, e3[r][t], g_in[b & 3][r], y);
          if (c0 + r < p.n_channels) p.out[(size_t)(c0 + r) * p.out_stride + (size_t)b * BS + t] = engine_out_word(y, p.output_gain, p.mute);
        }
      }
    } else if (wave == 0) {
      const int b = step - 1;
      if (casc && p.audio_on && b >= 0 && b < p.n_blocks) cascade_row(aud, ta[b & 3][row], sct);
    } else {
      const int b = step - 2;
      if (ser && p.agc_on && b >= 0 && b < p.n_blocks) {
        g_in[b & 3][sc] = agc.g;
        agc_envelope(agc, p.agc, curve, ta[b & 3][sc], ge[b & 3][sc]);
      }
    }
    __syncthreads();
  }
  if (casc && c0 + row < p.n_channels) aud.store(p.st + (size_t)rch * NF + ST_AUDIO + 4 * sct);
  if (ser && c0 + sc < p.n_channels) agc.store(sst);
}

}  // namespace

hipError_t rdsp_engine_launch(const EngParams &p, bool blanker, bool als, hipStream_t s) {
  const int n = p.n_channels, tch = als ? 16 : 8;
  const bool ssb = p.mode <= 3 || p.mode == 6;
  const dim3 gf((unsigned)((n + FCH - 1) / FCH)), gt((unsigned)((n + tch - 1) / tch));
  if (blanker) hipLaunchKernelGGL(rdsp_engine_front_kernel<true>, gf, dim3(FW), 0, s, p);
  else if (ssb) hipLaunchKernelGGL(rdsp_engine_front_pipe_kernel, gf, dim3(PW), 0, s, p);
  else hipLaunchKernelGGL(rdsp_engine_front_kernel<false>, gf, dim3(FW), 0, s, p);
  const dim3 gh((unsigned)((p.n_blocks * BS + HB_OUT - 1) / HB_OUT), (unsigned)n);
  if (ssb) hipLaunchKernelGGL(rdsp_engine_hilbert_kernel, gh, dim3(256), 0, s, p); /* (an unknown mode number leaves the audio buffer as the last call did) */
  if (als) hipLaunchKernelGGL(rdsp_engine_tail_kernel<true>, gt, dim3(FW), 0, s, p);
  else hipLaunchKernelGGL(rdsp_engine_tail_pipe_kernel, gt, dim3(PW), 0, s, p);
  return hipGetLastError();
}
