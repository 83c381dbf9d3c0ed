/*
 * rdsp_engine_front.hip -- the front stage of rdsp_engine_t (rdsp_engine.hip has the engine's narrative and the map of the
 * image's addresses): conversion (0xe7b4), impulse blanker (0xe14c), IF filter, then the frequency shift into the rings
 * (SSB / CW, 0xe94e) or the AM / SAM detectors (0xec1c, 0xe390, 0xed02) into the audio rows.  Two kernels: the passes of a
 * block one after the other (blanker, AM, SAM), or on different waves a block apart (SSB / CW without the blanker).
 * Compiled with -ffp-contract=off: every fused operation below is written as one (fmaf / fma).
 */
#include <hip/hip_runtime.h>
#include <math.h>

#include "rdsp_engine_dev.h"

namespace {

/* ---- front: conversion, blanker, IF filter, frequency shift (SSB / CW) or the AM / SAM detectors ----------------------
 * 8 channels = 16 tile rows (channel, rail) per workgroup of four waves -- a launch's duration is one workgroup's chain
 * of blocks whatever the grid, so the fewer channels a workgroup carries the shorter it is, down to what the recursions
 * need.  Per block: conversion and the mixer's table work spread over all 256 lanes (element e = lane + 256 j: consecutive
 * lanes on consecutive samples of a row); the cascades with a quad per row on waves 0 and 1 while wave 2 runs the
 * oscillator's phase, one lane per channel; the PLL and the blanker -- true recursions -- on one lane per channel or row. */

/* 0xe7b4: / 32767 and the rail's gain, in double; one int16 pair per element.  Block b of the workgroup's channels into the
 * tile (rows 2 cl and 2 cl + 1: channel c0 + cl's rails), on LANES lanes */
template <int LANES>
__device__ __forceinline__ void convert_block(const EngParams &p, int c0, int lane, int b, float (*tf)[PITCH]) {
  for (int j = 0; j < TILE_STEPS<LANES, FCH>; j++) {
    const auto [cl, t] = tile_at<LANES>(lane, j);
    const int w = c0 + cl < p.n_channels ? p.iq[(size_t)(c0 + cl) * p.in_stride + (size_t)b * BS + t] : 0;
    tf[2 * cl][t] = (float)(over_32767((int)(int16_t)(w & 0xffff)) * (double)p.gain_i);
    tf[2 * cl + 1][t] = (float)(over_32767(w >> 16) * (double)p.gain_q);
  }
}

/* 0xe94e / 0xed02: every sample of the tile turned by its phase, on all FW lanes; SOME: the channels whose flag in `skip` is
 * set stay as they are */
template <bool SOME>
__device__ __forceinline__ void rotate_tile(int tid, const float *sine, float (*tf)[PITCH], const float (*phs)[PITCH], const int *skip) {
  for (int j = 0; j < TILE_STEPS<FW, FCH>; j++) {
    const auto [cl, t] = tile_at<FW>(tid, j);
    if (SOME && skip[cl]) continue;
    float x = tf[2 * cl][t], y = tf[2 * cl + 1][t];
    rotate_sample(sine, phs[cl][t], x, y);
    tf[2 * cl][t] = x; tf[2 * cl + 1][t] = y;
  }
}

/* ---- 0xe14c: the impulse blanker.  Two blocks of delay; |I + jQ| against its running average; blanking mask with a taper.
 * The lines: three blocks of I, Q and mask per channel in LDS, slot (n / 128 + base) % 3 holding samples n .. n + 127 of
 * the 384-sample line, so that a block boundary moves a base instead of 768 words.  One per workgroup: every lane holds
 * the base, the serial lanes their channel's three state words. */
template <bool NB>
struct Blanker {
  struct Lines {                                                  /* the workgroup's LDS (nothing to speak of without the blanker) */
    float l[NB ? 3 : 1][NB ? FCH : 1][NB ? 388 : 1];              /* I, Q, mask */
    float mag[NB ? FCH : 1][NB ? 180 : 1];
  };
  Lines &s;
  int base;
  float avg, last;
  int hit;
  __device__ __forceinline__ int at(int n) const { int sl = (n >> 7) + base; sl = sl >= 3 ? sl - 3 : sl; return sl * 128 + (n & 127); }
  __device__ __forceinline__ void load_state(const float *sst) { avg = sst[ST_NB_AVG]; last = sst[ST_NB_LAST]; hit = __float_as_int(sst[ST_NB_HIT]); }
  __device__ __forceinline__ void store_state(float *sst) const { sst[ST_NB_AVG] = avg; sst[ST_NB_LAST] = last; sst[ST_NB_HIT] = __int_as_float(hit); }
  /* the lines come from (IN) or go to HBM, which keeps them in line order: I, Q, mask; a channel beyond the engine's has
   * zero lines under a mask of ones */
  template <bool IN>
  __device__ __forceinline__ void lines(const EngParams &p, int c0, int tid) {
    for (int e = tid; e < 3 * FCH * 384; e += FW) {
      const int k = e / (FCH * 384), r = e - k * (FCH * 384), cl = r / 384, i = r - cl * 384;
      const bool there = c0 + cl < p.n_channels;
      float *hbm = p.nb + (size_t)(c0 + cl) * NB_WORDS + 384 * k + i, &lds = s.l[k][cl][at(i)];
      if constexpr (IN) lds = there ? *hbm : (k == 2 ? 1.0f : 0.0f);
      else if (there) *hbm = lds;
    }
  }
  __device__ __forceinline__ void load(const EngParams &p, int c0, int tid) {
    base = 0;
    lines<true>(p, c0, tid);
    __syncthreads();
  }
  __device__ __forceinline__ void store(const EngParams &p, int c0, int tid) {
    __syncthreads();
    lines<false>(p, c0, tid);
  }
  /* one block: the tile's rows go in, the rows of two blocks ago come out under their mask */
  __device__ __forceinline__ void block(const EngParams &p, float (*tf)[PITCH], int tid, const SerialRole &ser) {
    base = base == 2 ? 0 : base + 1;                              /* the oldest block's slot takes the new one */
    for (int j = 0; j < TILE_STEPS<FW, FCH>; j++) {
      const auto [cl, t] = tile_at<FW>(tid, j);
      const int a = at(256 + t);
      s.l[0][cl][a] = tf[2 * cl][t]; s.l[1][cl][a] = tf[2 * cl + 1][t]; s.l[2][cl][a] = 1.0f;
    }
    __syncthreads();
    for (int e = tid; e < FCH * 178; e += FW) {                   /* the magnitudes are pure functions of the samples */
      const int cl = e / 178, n = 78 + e - cl * 178, a = at(n);
      const float vi = s.l[0][cl][a], vq = s.l[1][cl][a];
      s.mag[cl][n - 78] = quick_sqrt1(fmaf(vi, vi, vq * vq));
    }
    __syncthreads();
    if (ser.on) { /* what is a recursion: the running average and what it decides, then the taper in front of every 0 -> 1 step */
      float *mask = s.l[2][ser.sc];
      hit = 0;
      int zeroed_to = 67;                      /* hits come in rising order: what an earlier one of this pass zeroed stays zero */
      for (int n = 78; n < 256; n++) {
        const float limit = avg * p.nb_ratio;
        last = s.mag[ser.sc][n - 78];
        if (limit < last) {
          if (-p.nb_before <= p.nb_after) {
            const int lo = max(n - p.nb_before, zeroed_to + 1), hi = n + p.nb_after;
            for (int j = lo; j <= hi; j++) mask[at(j)] = 0.0f;
            zeroed_to = max(zeroed_to, hi);
          }
          hit = 1;
        }
        avg = fmaf(avg, p.nb_keep, last * p.nb_new);
      }
      const float taper[7] = {0.933f, 0.75f, 0.5f, 0.25f, 0.067f, 0.0f, 0.0f};
      for (int i = 128; i < 256; i++)
        if (mask[at(i)] == 1.0f && mask[at(i - 1)] == 0.0f)
          for (int j = 0; j < 7; j++) mask[at(i - 7 + j)] = taper[j];
    }
    __syncthreads();
    for (int j = 0; j < TILE_STEPS<FW, FCH>; j++) {
      const auto [cl, t] = tile_at<FW>(tid, j);
      const int a = at(t);
      const float mk = s.l[2][cl][a];
      tf[2 * cl][t] = mk * s.l[0][cl][a]; tf[2 * cl + 1][t] = mk * s.l[1][cl][a];
    }
    __syncthreads();
  }
};

/* ---- 0xe390: the SAM detector's PLL on the IF signal, one lane per channel: its seven state words, and a block's recursion */
struct SamPll {
  float c, s, u, err, hz, ph;
  int locked;
  __device__ __forceinline__ void load(const float *sst) {
    c = sst[ST_SAM_COS]; s = sst[ST_SAM_SIN]; u = sst[ST_SAM_U]; err = sst[ST_SAM_ERR]; hz = sst[ST_SAM_HZ];
    ph = sst[ST_SAM_PH];
    locked = __float_as_int(sst[ST_SAM_LOCK]);
  }
  __device__ __forceinline__ void store(float *sst) const {
    sst[ST_SAM_COS] = c; sst[ST_SAM_SIN] = s; sst[ST_SAM_U] = u; sst[ST_SAM_ERR] = err; sst[ST_SAM_HZ] = hz;
    sst[ST_SAM_PH] = ph; sst[ST_SAM_LOCK] = __int_as_float(locked);
  }
  /* the arctangent of the phase detector: a cubic in the smaller ratio, by octant */
  static __device__ __forceinline__ float phase_error(float re, float im) {
    const float HALF_PI = 1.5707963705062866f, A1 = 0.97239410877227783f, A3 = -0.19194795191287994f;
    float e;
    if (re == 0.0f) e = im > 0.0f ? HALF_PI : (im < 0.0f ? -HALF_PI : 0.0f);
    else if (fabsf(re) > fabsf(im)) {
      const float z = im / re;
      e = fmaf(z, z * A3, A1) * z;
      if (!(re > 0.0f)) e = (float)(im >= 0.0f ? (double)e + 3.1415926535897931 : (double)e - 3.1415926535897931);
    } else {
      const float z = re / im;
      e = fmaf(-z, fmaf(z, z * A3, A1), im > 0.0f ? HALF_PI : -HALF_PI);
    }
    return e;
  }
  /* one block of a channel's rails ri, rq: the loop, and in lock the rails turned by its oscillator */
  __device__ __forceinline__ void block(const EngParams &p, const float *sine, float *ri, float *rq) {
    for (int t = 0; t < BS; t++) {
      const float x = ri[t], q = rq[t];
      const float re = fmaf(x, c, q * s), im = fmaf(q, c, -(s * x));
      const float e = phase_error(re, im);
      const float un = fmaf(e, p.sam_ga, p.sam_gb * err);
      const double phd = fma((double)(un + u), 0.5, (double)ph);
      hz = fmaf(p.sam_keep, hz, (un * p.sam_hz_per_rad) * p.sam_new);
      ph = (float)phd;
      if ((double)ph >= 3.1415926535897931) ph -= TWO_PI_F;
      if ((double)ph < -3.1415926535897931) ph += TWO_PI_F;
      locked = hz > p.sam_lock_lo ? (hz < p.sam_lock_hi) : 0;
      table_cos_sin(sine, ph, c, s);
      if (locked) {
        ri[t] = fmaf(x, c, q * s);
        rq[t] = fmaf(-x, s, q * c);
      }
      u = un; err = e;
    }
  }
};

/* ---- 0xed02: AM, and SAM out of lock: shift by the IF centre, low-pass, envelope.  A channel in lock (locked_of) keeps the
 * rotated I rail as its audio and none of the detector's state moves.  Called by the whole workgroup; leaves the
 * demodulated audio in the I rows */
__device__ __forceinline__ void am_detector(int tid, const QuadRole q, bool casc, const SerialRole ser, const float *sine, const int *locked_of,
                                            float &amph, float am_inc, Section &amf, float (*tf)[PITCH], float (*phs)[PITCH]) {
  if (ser.on && !locked_of[ser.sc]) phase_row(amph, am_inc, phs[ser.sc]);
  __syncthreads();
  rotate_tile<true>(tid, sine, tf, phs, locked_of);
  __syncthreads();
  if (casc) {
    const bool detect = !locked_of[q.row >> 1];
    const Section keep = amf;
    cascade_row<true>(amf, detect ? tf[q.row] : phs[q.row >> 1], q.sct);   /* the quads of a locked channel run on a row nobody reads ... */
    if (!detect) amf = keep;                                     /* ... and keep their state */
  }
  __syncthreads();
  for (int j = 0; j < TILE_STEPS<FW, FCH>; j++) {
    const auto [cl, t] = tile_at<FW>(tid, j);
    if (locked_of[cl]) continue;
    const float x = tf[2 * cl][t], y = tf[2 * cl + 1][t];
    tf[2 * cl][t] = quick_sqrt2(fmaf(x, x, y * y));
  }
  __syncthreads();
}

template <bool NB>
__global__ __launch_bounds__(FW, 2) void rdsp_engine_front_kernel(const EngParams p) {
  __shared__ float tf[2 * FCH][PITCH];
  __shared__ float phs[FCH][PITCH];
  __shared__ int locked_of[FCH];
  __shared__ float sine[257];                                     /* the oscillator's table: the PLL reads it twice per sample of a dependent chain */
  __shared__ typename Blanker<NB>::Lines nb_lines;
  const int tid = threadIdx.x, c0 = blockIdx.x * FCH;
  for (int i = tid; i < 257; i += FW) sine[i] = p.sine[i];
  const bool casc = tid < 8 * FCH;                                /* cascade role: waves 0 and 1 */
  const QuadRole q = quad_role<2 * FCH, 2>(tid, c0, p.n_channels);
  const bool ssb = p.mode <= 3 || p.mode == 6, am = p.mode == 4 || p.mode == 5;
  float *qst = p.st + (size_t)q.ch * NF + 16 * (q.row & 1) + 4 * q.sct;
  Section pre, amf;
  pre.load(p.sets + 20 * p.pre_set + 5 * q.sct, qst + ST_PRE, (p.resets & RESET_PRE) != 0);
  amf.load(p.sets + 20 * 13 + 5 * q.sct, qst + ST_AM, false);
  const SerialRole ser = serial_role<FCH>(tid, 128, c0, p.n_channels); /* wave 2, beside the cascades' waves 0 and 1 */
  float *sst = p.st + (size_t)ser.ch * NF;
  float nco = sst[ST_NCO], amph = sst[ST_AMPH];
  SamPll pll;
  pll.load(sst);
  Blanker<NB> nb{nb_lines};
  nb.load_state(sst);
  if constexpr (NB) nb.load(p, c0, tid);
  const float nco_inc = -(p.tuning_offset * RAD_PER_HZ), am_inc = -p.if_centre * RAD_PER_HZ;

  for (int b = 0; b < p.n_blocks; b++) {
    convert_block<FW>(p, c0, tid, b, tf);                          /* 0xe7b4 */
    __syncthreads();
    if constexpr (NB) nb.block(p, tf, tid, ser);                   /* 0xe14c */
    if (casc) cascade_row<true>(pre, tf[q.row], q.sct);
    else if (ser.on && ssb) phase_row(nco, nco_inc, phs[ser.sc]);  /* 0xe94e: the phase falls by the tuning offset */
    __syncthreads();
    if (ssb) {
      rotate_tile<false>(tid, sine, tf, phs, nullptr);
      __syncthreads();
      const uint32_t at = p.pos + (uint32_t)b * BS, m = p.ring_size - 1;
      for (int j = 0; j < TILE_STEPS<FW, 2 * FCH>; j++) {
        const auto [r, t] = tile_at<FW>(tid, j); /* into the rings: tile row r is (channel c0 + r / 2, rail r & 1) */
        if (c0 + (r >> 1) < p.n_channels)
          ((r & 1) ? p.ring_q : p.ring_i)[(size_t)(c0 + (r >> 1)) * p.ring_size + ((at + (uint32_t)t) & m)] = tf[r][t];
      }
    } else if (am) {
      if (casc) cascade_row<true>(pre, tf[q.row], q.sct);          /* 0xec1c: the IF filter a second time */
      __syncthreads();
      if (p.mode == 5) {
        if (ser.on) {
          pll.block(p, sine, tf[2 * ser.sc], tf[2 * ser.sc + 1]);  /* 0xe390 */
          locked_of[ser.sc] = pll.locked;
        }
      } else if (ser.on) locked_of[ser.sc] = 0;
      __syncthreads();
      am_detector(tid, q, casc, ser, sine, locked_of, amph, am_inc, amf, tf, phs); /* 0xed02 */
      for (int j = 0; j < TILE_STEPS<FW, FCH>; j++) {
        const auto [cl, t] = tile_at<FW>(tid, j); /* the demodulated audio is in the I rows */
        if (c0 + cl < p.n_channels) p.audio[(size_t)(c0 + cl) * p.audio_stride + (size_t)b * BS + t] = tf[2 * cl][t];
      }
    }
    __syncthreads();
  }
  if (casc && q.valid) {
    pre.store(qst + ST_PRE);
    if (am) amf.store(qst + ST_AM);
  }
  if (ser.valid) {
    sst[ST_NCO] = nco; sst[ST_AMPH] = amph;
    pll.store(sst);
  }
  if constexpr (NB) {
    if (ser.valid) nb.store_state(sst);
    nb.store(p, c0, tid);
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
  const QuadRole q = quad_role<2 * FCH, 2>(tid, c0, p.n_channels); /* wave 0: section sct of tile row `row` */
  float *qst = p.st + (size_t)q.ch * NF + ST_PRE + 16 * (q.row & 1) + 4 * q.sct;
  Section pre;
  pre.load(p.sets + 20 * p.pre_set + 5 * q.sct, qst, (p.resets & RESET_PRE) != 0);
  const SerialRole ser = serial_role<FCH>(tid, 64, c0, p.n_channels); /* wave 1, lanes 64 ... 64 + FCH - 1: channel sc's oscillator */
  float nco = p.st[(size_t)ser.ch * NF + ST_NCO];
  const float nco_inc = -(p.tuning_offset * RAD_PER_HZ);
  const int wl = tid - 128;                                       /* waves 2 and 3: 128 lanes for the element passes */
  const uint32_t m = p.ring_size - 1;
  for (int step = 0; step < p.n_blocks + 2; step++) {
    if (wave >= 2) {
      if (step < p.n_blocks) convert_block<PW - 128>(p, c0, wl, step, tf[step & 3]); /* block `step` comes in */
      const int b = step - 2;
      if (b >= 0) { /* 0xe94e: block step - 2, filtered and with its phases known, is rotated and leaves for the rings */
        float (*t2)[PITCH] = tf[b & 3];
        const float (*ph)[PITCH] = phs[b & 3];
        const uint32_t at = p.pos + (uint32_t)b * BS;
        for (int j = 0; j < TILE_STEPS<PW - 128, FCH>; j++) {
          const auto [cl, t] = tile_at<PW - 128>(wl, j);
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
        if (wave == 0) cascade_row(pre, tf[b & 3][q.row], q.sct);
        else if (ser.on) phase_row(nco, nco_inc, phs[b & 3][ser.sc]);
      }
    }
    __syncthreads();
  }
  if (wave == 0 && q.valid) pre.store(qst);
  if (ser.valid) p.st[(size_t)ser.ch * NF + ST_NCO] = nco;
}

}  // namespace

namespace rdsp_eng {
/* which kernel: the pipeline of waves has no place for the blanker's, the PLL's and the detector's passes */
void engine_launch_front(const EngParams &p, bool blanker, hipStream_t s) {
  const bool ssb = p.mode <= 3 || p.mode == 6;
  const dim3 g((unsigned)((p.n_channels + FCH - 1) / FCH));
  if (blanker) hipLaunchKernelGGL(rdsp_engine_front_kernel<true>, g, dim3(FW), 0, s, p);
  else if (ssb) hipLaunchKernelGGL(rdsp_engine_front_pipe_kernel, g, dim3(PW), 0, s, p);
  else hipLaunchKernelGGL(rdsp_engine_front_kernel<false>, g, dim3(FW), 0, s, p);
}
}  // namespace rdsp_eng
