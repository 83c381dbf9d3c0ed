/*
 * rdsp_front_frame.h -- device code shared by the three front-kernel families (rdsp_front_direct.hip,
 * rdsp_front_fd.hip, rdsp_front_rd.hip): the stages behind the decimator.
 *
 *   arm_fast_sin_turns, spec_resynthesize_literal, spec_table_factor
 *                       A6 re-synthesis as the reference writes it (rdsp_set_spectral_resynthesis)
 *   kernarg_late, RDSP_LATE, RDSP_GROUP_LATE_*
 *                       kernel parameters and group-record fields read where they are used
 *   front_frame         A5 overlap-save filter, A6 spectral NR, demod select, A9 AGC, gain, A10 pack: one frame
 *                       of N/2 new samples over a workgroup
 *   QUAD_*, quad_chain, front_frame_quad
 *                       the same for FFT_L 256 on 16-lane rows, four frames per pass
 *
 * Every function is inlined into the kernel that calls it; the kernels sit at their register limits, so a passage
 * that exists twice here (front_frame / front_frame_quad) names its twin instead of sharing a helper with it.
 */
#ifndef RDSP_FRONT_FRAME_H
#define RDSP_FRONT_FRAME_H

#include "rdsp_front.h"
#include "rdsp_wave.h"

namespace rdsp {

/* arm_sin_f32 / arm_cos_f32 of CMSIS-DSP as published (FastMathFunctions): the angle in turns, its fractional
 * part times 512 as a table index, linear interpolation between neighbouring entries of the 513-entry table.
 * `in` = x * 0.159154943092f for the sine, + 0.25f for the cosine. */
__device__ __forceinline__ float arm_fast_sin_turns(float in, const float *tab) {
  int n = (int)in;
  if (in < 0.0f) n--;
  in = in - (float)n;
  float findex = 512.0f * in;
  int index = (int)findex;
  if (index >= 512) { index = 0; findex -= 512.0f; }
  const float fract = findex - (float)index;
  const auto gt = (const __attribute__((address_space(1))) float *)tab; /* a global load, not a FLAT one */
  const float a = gt[index], b = gt[index + 1];
  return (1.0f - fract) * a + fract * b;
}
/* SPEC:213-217 and 226-235 as written, for the P bins of a thread: the new magnitude (0.2 mag at or under the
 * floor, mag - floor above it) and the bin rebuilt from it and the original phase,
 *   phi = atan2(im, re);  re' = mag' arm_cos_f32(phi);  im' = mag' arm_sin_f32(phi).
 * An opt-in mode (rdsp_set_spectral_resynthesis) inside kernels whose register budget decides their occupancy: the
 * bins go through the transform's work buffer in LDS -- `slot(e)`: the thread's own entries of the last forward /
 * first inverse pass -- and ONE rolled loop does the work, so the mode costs the default path
 * no registers (unrolled in place, sixteen atan2 chains took the 512-point kernel from 176 to 253 VGPRs). */
template <int P, typename SLOT>
__device__ __forceinline__ void spec_resynthesize_literal(float2 (&v)[P], float floor_, const float *tab, float2 *wb, SLOT slot) {
#pragma unroll
  for (int e = 0; e < P; e++) wb[slot(e)] = v[e];
#pragma unroll 1
  for (int e = 0; e < P; e++) {
    const float2 x = lds_ld(&wb[slot(e)]);
    const float pw = fmaf(x.y, x.y, fmaf(x.x, x.x, 1e-30f)); /* the same |X| as the caller's (SPEC:182) */
    const float m0 = pw * __builtin_amdgcn_rsqf(pw);
    const float m1 = (m0 <= floor_) ? 0.2f * m0 : m0 - floor_;                     /* SPEC:213-217 */
    const float turns = atan2f(x.y, x.x) * 0.159154943092f;                        /* SPEC:229 */
    wb[slot(e)] = make_float2(m1 * arm_fast_sin_turns(turns + 0.25f, tab),         /* SPEC:231 */
                              m1 * arm_fast_sin_turns(turns, tab));                /* SPEC:232 */
  }
#pragma unroll
  for (int e = 0; e < P; e++) v[e] = lds_ld(&wb[slot(e)]); /* single ds_read_b64, like the transform's passes */
}

/* SPEC:229-232 as written -- re' = mag' arm_cos_f32(phi), im' = mag' arm_sin_f32(phi), phi = atan2(im, re) -- evaluated
 * in closed form.  arm_sin_f32 interpolates linearly in a 512-step table: between the nodes phi0 and phi0 + h
 * (h = 2 pi / 512) at the fraction f it returns (1 - f) sin(phi0) + f sin(phi0 + h) = A(f) sin(phi) + B(f) cos(phi) with
 * A = (1 - f) cos(f h) + f cos((1 - f) h) = 1 - (h^2 / 2) f (1 - f) + O(h^4) and |B| < 3e-8; the cosine (phi + a quarter
 * turn = 128 table steps exactly) meets the same f.  So the as-written bin is the exact one, X mag'/mag, times A(f): what
 * the table's interpolation costs, 1.9e-5 of the bin at most -- and this expression is within 5e-8 of the table's own
 * arithmetic (tests/test_host_logic.py evaluates both over the circle).  f (1 - f) is the same in every octant, so
 * f comes from atan(min / max) alone: a degree-11 odd polynomial in table steps (error 1.4e-4 of a step, 1e-8 of the
 * result), no branches, no table, 14 operations a bin where atan2f and two interpolated look-ups took 95. */
__device__ __forceinline__ float spec_table_factor(float2 x) {
  const float ax = fabsf(x.x), ay = fabsf(x.y);
  const float mx = fmaxf(fmaxf(ax, ay), 1e-30f), mn = fminf(ax, ay);
  const float z = mn * __builtin_amdgcn_rcpf(mx), s = z * z;
  const float u = fmaf(s, fmaf(s, fmaf(s, fmaf(s, fmaf(s, -0.954960883f, 4.29009151f), -9.48728275f), 15.7710886f), -27.1045456f), 81.4854736f) * z;
  const float f = __builtin_amdgcn_fractf(u);
  return fmaf(fmaf(-f, f, f), -7.52982e-05f, 1.0f); /* (2 pi / 512)^2 / 2 */
}

/* A field of the kernel's parameter block (or of the channel's group record) read where it is used, not at kernel
 * entry.  The compiler loads every kernarg it will ever need in the prologue, and with more than a hundred scalar values
 * live across the frame loop it spills them to VGPR lanes: 79 spilled SGPRs and ~95 v_readlane reloads per decimator
 * frame in the K2 instance of rdsp_front_fd_kernel, every one an issue slot of the vector unit.  What only the call's
 * first frame, an option's own branch or the state write-back at the end needs comes through here instead: a scalar load
 * from the kernarg segment through a pointer the optimizer cannot identify with the one it loaded from at entry (the
 * parameter block is the kernels' only argument: offset 0 of the segment). */
template <typename T>
__device__ __forceinline__ T kernarg_late(unsigned off) {
  auto kp = (const __attribute__((address_space(4))) unsigned char *)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(kp));
  return *reinterpret_cast<const __attribute__((address_space(4))) T *>(kp + off);
}
#define RDSP_LATE(field) kernarg_late<decltype(RdspFrontParams::field)>((unsigned)offsetof(RdspFrontParams, field))
/* the group record's cold fields (what the 256 history samples were mixed with): read like the record at kernel entry,
 * vector loads of a wave-uniform address, made scalar by v_readfirstlane */
__device__ __forceinline__ uint32_t group_late_word(uint32_t gi, unsigned off) {
  const uint32_t *gw = reinterpret_cast<const uint32_t *>(RDSP_LATE(groups) + gi) + off / 4;
  asm volatile("" : "+s"(gw));
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)*(const __attribute__((address_space(1))) uint32_t *)gw);
}
__device__ __forceinline__ float2 group_late_f2(uint32_t gi, unsigned off) {
  return make_float2(__builtin_bit_cast(float, group_late_word(gi, off)), __builtin_bit_cast(float, group_late_word(gi, off + 4)));
}
#define RDSP_GROUP_LATE_F2(gi, field) group_late_f2(gi, (unsigned)offsetof(RdspGroup, field))
#define RDSP_GROUP_LATE_U32(gi, field) group_late_word(gi, (unsigned)offsetof(RdspGroup, field))

/* ---- A5/A6 + epilogue: one overlap-save frame of H = N/2 new samples ------------------
 * Shared by the front kernels (direct-form and FFT-domain decimator).  fetch(i) returns new
 * sample i of the hop from wherever the producer left it in LDS. */
template <int N, int P, bool WALIAS, typename TW, typename FETCH>
__device__ __forceinline__ void front_frame(const RdspFrontParams &p, const RdspGroup &G, const TW &tw,
                                            const LdsBases<N, P, WALIAS> &lb, float2 *wb, float *red,
                                            const float2 (&mreg)[P], uint32_t vadbits, float vad_inv,
                                            float2 (&vprev)[P / 2], float &nfloor, float &agc_g, float &am_dc,
                                            int &frame_idx, size_t ch, int tid, FETCH fetch) {
  using PL = FftPlan<N, P>;
  constexpr int NT = PL::NT;
  constexpr int NW = NT / 64;
  constexpr int H = N / 2;
  constexpr int PH = P / 2;
  constexpr int NB = H / RDSP_BLOCK; /* 128-blocks per hop */
  const int lane = tid & 63;
  const int wave = tid >> 6;
  {
  float2 v[P];
  /* CONV:267-285: [previous hop | current hop]; CONV:274-278: the current hop is
   * the next frame's previous hop (this thread's elements stay in its registers) */
#pragma unroll
  for (int j = 0; j < PH; j++) {
    v[j] = vprev[j];
    v[j + PH] = fetch(tid + j * NT);
    vprev[j] = v[j + PH];
  }
  auto sync = []() { wg_sync<NW>(); };
  {
    float2 twp[P - 1];
    tw.template get<0>(twp);
    fwd_pass0_store<N, P>(lb, v, wb, twp); /* CONV:291 */
  }
  wg_sync<NW>();
  fwd_mid_all<N, P, 1, PL::NP - 1, WALIAS>(lb, wb, tw, sync);
  fwd_pass_last<N, P>(lb, v, wb);

  if (p.spectral_on) { /* SPEC:182-235 on the un-masked spectrum (twin: the spectral stage of front_frame_quad) */
    float mag[P], rmag[P];
    float part = 0.f;
#pragma unroll
    for (int e = 0; e < P; e++) {
      /* |X| and 1/|X| from one v_rsq_f32 (1 ulp) instead of a correctly rounded sqrt and a
       * division per bin; the floor keeps rsq finite on empty bins (|X| = 1e-15 there; it is
       * absorbed by any power above 1e-22) */
      const float pw = fmaf(v[e].y, v[e].y, fmaf(v[e].x, v[e].x, 1e-30f)); /* the floor rides in the sum */
      rmag[e] = __builtin_amdgcn_rsqf(pw);
      mag[e] = pw * rmag[e];                              /* SPEC:182 */
      part += ((vadbits >> e) & 1u) ? mag[e] : 0.f;       /* SPEC:194-197 */
    }
    float tot = wave_sum(part);
    if constexpr (NW > 1) {
      if (lane == 0) red[wave] = tot;
      wg_sync<NW>();
      tot = (red[0] + red[1]) + (red[2] + red[3]);
      wg_sync<NW>();
    }
    float th = tot * vad_inv;                      /* SPEC:200 */
    th = th * p.spectral_k;                        /* SPEC:202 */
    if (p.spectral_on == 2) {
      nfloor = th;                                 /* BK_INO:1595-1596: no smoothing */
    } else {
      nfloor += (th - nfloor) * 0.65f;             /* SPEC:205 */
      nfloor = nfloor > 0.f ? nfloor : 0.f;        /* SPEC:206 */
    }
    if (p.spectral_literal == 1) { /* rdsp_set_spectral_resynthesis(c, 1): SPEC:213-217, 226-235 as written, the table's interpolation in closed form */
#pragma unroll
      for (int e = 0; e < P; e++) {
        const float sc = ((mag[e] <= nfloor) ? 0.2f : fmaf(-nfloor, rmag[e], 1.f)) * spec_table_factor(v[e]);
        v[e].x *= sc;
        v[e].y *= sc;
      }
    } else if (p.spectral_literal) { /* (c, 2): the same with atan2f and the table looked up */
      /* the thread's own P entries of the work buffer: what it read in the last forward pass and writes in the
       * first inverse pass, so no other lane ever touches them in between (and they are inside the buffer under
       * either map, also where it is cut into the FIR planes behind their history) */
      const int own = lb.bi[PL::NP - 1];
      spec_resynthesize_literal<P>(v, nfloor, RDSP_LATE(sin_table), wb, [&](int e) { return own + e; });
    } else {
#pragma unroll
      for (int e = 0; e < P; e++) {
        /* SPEC:213-217, 226-235: X * mag'/mag with mag' = 0.2 mag at or under the floor and
         * mag - floor above it, i.e. a gain of 0.2 or 1 - floor/mag (an empty bin stays 0) */
        const float sc = (mag[e] <= nfloor) ? 0.2f : fmaf(-nfloor, rmag[e], 1.f);
        v[e].x *= sc;
        v[e].y *= sc;
      }
    }
  }
  /* CONV:301: spectrum x mask */
#pragma unroll
  for (int e = 0; e < P; e++) v[e] = cmul(v[e], mreg[e]);

  inv_pass_last<N, P>(lb, v, wb); /* CONV:309 */
  wg_sync<NW>();
  inv_mid_all<N, P, PL::NP - 2, WALIAS>(lb, wb, tw, sync);
  {
    float2 twp[P - 1];
    tw.template get<0>(twp);
    inv_pass0_load<N, P>(lb, v, wb, twp);
  }
  wg_sync<NW>(); /* wb is free again (next frame / taps / FIR partials) */

  /* CONV:314-318: keep the second half.  v[PH + jj] = y[N/2 + tid + jj*NT] */
  float L[PH], R[PH];
#pragma unroll
  for (int jj = 0; jj < PH; jj++) {
    L[jj] = v[PH + jj].x;
    R[jj] = v[PH + jj].y;
  }

  /* helper: per-128-block sums of a per-thread value over the workgroup */
  float bs[NB];
  auto block_sums = [&](const float(&pv)[PH]) {
#pragma unroll
    for (int jj = 0; jj < PH; jj++) {
      float s = wave_sum(pv[jj]);
      if (lane == 0) red[wave * PH + jj] = s;
    }
    wg_sync<NW>();
#pragma unroll
    for (int b = 0; b < NB; b++) {
      float s = 0.f;
#pragma unroll
      for (int w = 0; w < NW; w++)
#pragma unroll
        for (int jj = 0; jj < PH; jj++)
          if (((jj * NT + w * 64) >> 7) == b) s += red[w * PH + jj];
      bs[b] = s;
    }
    wg_sync<NW>();
  };

  if (G.demod == RDSP_K_DEMOD_REAL) {
#pragma unroll
    for (int jj = 0; jj < PH; jj++) R[jj] = L[jj];
  } else if (G.demod == RDSP_K_DEMOD_AM) {
    float a[PH];
#pragma unroll
    for (int jj = 0; jj < PH; jj++) a[jj] = __builtin_amdgcn_sqrtf(L[jj] * L[jj] + R[jj] * R[jj]);
    block_sums(a);
    float d0[NB], d1[NB];
#pragma unroll
    for (int b = 0; b < NB; b++) {
      float m = bs[b] / (float)RDSP_BLOCK;
      float dn = am_dc + 0.25f * (m - am_dc);
      d0[b] = am_dc;
      d1[b] = dn;
      am_dc = dn;
    }
#pragma unroll
    for (int jj = 0; jj < PH; jj++) {
      const int b0 = (jj * NT) >> 7;
      float s0 = d0[b0], s1 = d1[b0];
      if constexpr (NT == 256) {
        if (tid >= 128) { s0 = d0[b0 + 1]; s1 = d1[b0 + 1]; }
      }
      int i = (tid + jj * NT) & 127;
      float dc = s0 + (s1 - s0) * ((float)(i + 1) / (float)RDSP_BLOCK);
      L[jj] = a[jj] - dc;
      R[jj] = L[jj];
    }
  }

  const size_t tout = (size_t)frame_idx * H;
  if (p.to_mid) {
#pragma unroll
    for (int jj = 0; jj < PH; jj++) p.mid[ch * p.mid_stride + tout + tid + jj * NT] = L[jj];
    if (G.demod == RDSP_K_DEMOD_SAM) { /* the PLL stage needs the quadrature part too */
#pragma unroll
      for (int jj = 0; jj < PH; jj++) p.mid_q[ch * p.mid_stride + tout + tid + jj * NT] = R[jj];
    }
  } else {
    if (p.agc_on) {
      float pw[PH];
#pragma unroll
      for (int jj = 0; jj < PH; jj++) pw[jj] = L[jj] * L[jj] + R[jj] * R[jj];
      block_sums(pw);
      float g0[NB], g1[NB];
#pragma unroll
      for (int b = 0; b < NB; b++) {
        float pp = bs[b] / (float)(2 * RDSP_BLOCK);
        float rms = __builtin_amdgcn_sqrtf(pp); /* 1 ulp; the loop gain is a contraction */
        float gt = 0.25f * __builtin_amdgcn_rcpf(rms + 1e-6f);
        gt = fminf(gt, 100.0f);
        float coef = (gt < agc_g) ? p.agc_attack : p.agc_decay;
        float gn = agc_g + coef * (gt - agc_g);
        g0[b] = agc_g;
        g1[b] = gn;
        agc_g = gn;
      }
#pragma unroll
      for (int jj = 0; jj < PH; jj++) {
        const int b0 = (jj * NT) >> 7;
        float s0 = g0[b0], s1 = g1[b0];
        if constexpr (NT == 256) {
          if (tid >= 128) { s0 = g0[b0 + 1]; s1 = g1[b0 + 1]; }
        }
        int i = (tid + jj * NT) & 127;
        float g = s0 + (s1 - s0) * ((float)(i + 1) / (float)RDSP_BLOCK);
        L[jj] *= g;
        R[jj] *= g;
      }
    }
#pragma unroll
    for (int jj = 0; jj < PH; jj++) {
      float l = L[jj] * p.out_gain, r = R[jj] * p.out_gain;
      size_t o = ch * p.out_stride + tout + tid + jj * NT;
      __builtin_nontemporal_store(pack_lr(l, r), p.out_i16 + o); /* CONV:346-347; written once, read by nobody here */
      if (p.out_f32) p.out_f32[o] = make_float2(l, r);
    }
  }
  frame_idx++;
  }
}

/* ---- FFT_L = 256 behind the frequency-domain decimator: FOUR overlap-save frames per pass ----------
 * 256 points over a whole wave are 4 points per lane: four radix-4 passes, three LDS exchanges each way,
 * every pass a quarter-filled instruction stream -- the filter stage of K1 / K2 (the reference's own
 * FFT_L, CONV:36) cost as many VALU instructions and more LDS cycles than the 256-tap decimator in front
 * of it.  Overlap-save frames do not depend on each other (each is two consecutive hops of the decimated
 * stream, which sits in the ring), so here a 16-lane DPP row takes one frame -- 16 points per lane, two
 * radix-16 passes, ONE exchange each way -- and the wave takes four consecutive frames at once: a third
 * of the LDS operations per frame and about half the instructions.  What IS sequential across frames
 * (NFloor SPEC:205, the AGC gain, the AM detector's DC) depends on one number per frame: the four row
 * sums are read out with v_readlane and the four steps of the recursion run on wave-uniform values.
 * The mask is read from the same device image as the radix-4 plan's (digit-reversed for FftPlan<256, 4>):
 * bin k = i + 16 e of lane i sits at 64 e1 + e0 + 16 i0 + 4 i1 (i = i0 + 4 i1, e = e0 + 4 e1).
 * Ring: eight hops of 128, each padded by 16 float2 so that the two rows of a 32-lane group read disjoint
 * halves of the 64 banks.  The hop in front of the oldest unconsumed one is never overwritten (it is the
 * first frame's overlap, CONV:267-271: no previous-hop register file as in front_frame): a decimator frame adds
 * 448 samples when at most 448 are unconsumed (a quad goes as soon as 512 are there, and the counts are
 * multiples of 64), 128 + 448 + 448 = the ring.
 * Cost of the shape: 226 VGPRs and 18 KiB of LDS per channel (the four rows' exchange buffers), where the
 * one-frame form takes 187 and 12.9.  Alone that is still two waves per SIMD and eight channels per CU, and
 * K2 runs 0.6775 -> 0.6115 ms per step (same-box A/B); beside a tail kernel (124 VGPRs, 12.5 KiB per four
 * channels) it would be one wave per SIMD, so chains that hand their audio to the tail kernel keep the
 * one-frame form (template Q4, chosen by the launch code).  Moving mask and twiddles to LDS instead
 * (171 VGPRs, 22-23 KiB: seven or six channels per CU) measured 0.710 / 0.744 ms: occupancy is worth more. */
constexpr int QUAD_HOPS = 8, QUAD_PITCH = 128 + 16, QUAD_RING = QUAD_HOPS * QUAD_PITCH;
constexpr int QUAD_WB = 4 * FftPlan<256, 16>::WB;

template <typename F>
__device__ __forceinline__ void quad_chain(float x, int g, int nf, float &state, float &before, float &after, F step) {
  const float x0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), 0));
  const float x1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), 16));
  const float x2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), 32));
  const float x3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), 48));
  const float s0 = state, s1 = step(s0, x0), s2 = step(s1, x1), s3 = step(s2, x2), s4 = step(s3, x3);
  before = g == 0 ? s0 : (g == 1 ? s1 : (g == 2 ? s2 : s3));
  after = g == 0 ? s1 : (g == 1 ? s2 : (g == 2 ? s3 : s4));
  state = nf == 1 ? s1 : (nf == 2 ? s2 : (nf == 3 ? s3 : s4)); /* frames g >= nf are not there: their sums are never used */
}

template <int HOPS = QUAD_HOPS, typename TW>
__device__ __forceinline__ void front_frame_quad(const RdspFrontParams &p, const RdspGroup &G, const TW &tw,
                                                 const LdsBases<256, 16, false> &lb, float2 *wbg, const float2 *ring,
                                                 int rhop, int nf, int mbase, uint32_t vadbits, float vad_inv, float &nfloor,
                                                 float &agc_g, float &am_dc, int frame_idx, size_t ch, int lane) {
  constexpr int N = 256, P = 16;
  const int g = lane >> 4, i = lane & 15;
  int hc = rhop + g;
  hc = hc >= HOPS ? hc - HOPS : hc;
  const int hp = hc == 0 ? HOPS - 1 : hc - 1;
  const float2 *cur = ring + hc * QUAD_PITCH + i, *prv = ring + hp * QUAD_PITCH + i;
  /* this lane's sixteen bins of the group's mask: L2-resident, land behind the forward transform */
  float2 mreg[P];
  {
    const float2 *mp = p.mask_pool + G.mask_off;
    asm volatile("" : "+s"(mp));
    const auto gp = as_global(mp);
#pragma unroll
    for (int e = 0; e < P; e++) mreg[e] = gp[mbase + 64 * (e >> 2) + (e & 3)];
  }
  float2 v[P];
#pragma unroll
  for (int j = 0; j < P / 2; j++) { /* CONV:267-285: [previous hop | current hop], v[j] = x[i + 16 j] */
    v[j] = lds_ld(prv + 16 * j);
    v[j + P / 2] = lds_ld(cur + 16 * j);
  }
  {
    float2 twp[P - 1];
    tw.template get<0>(twp);
    fwd_pass0_store<N, P>(lb, v, wbg, twp); /* CONV:291 */
  }
  wg_sync<1>();
  fwd_pass_last<N, P>(lb, v, wbg);

  if (p.spectral_on) { /* SPEC:182-235 on the un-masked spectrum (twin: the spectral stage of front_frame) */
    float mag[P], rmag[P];
    float part = 0.f;
#pragma unroll
    for (int e = 0; e < P; e++) {
      const float pw = fmaf(v[e].y, v[e].y, fmaf(v[e].x, v[e].x, 1e-30f));
      rmag[e] = __builtin_amdgcn_rsqf(pw);
      mag[e] = pw * rmag[e];                              /* SPEC:182 */
      part += ((vadbits >> e) & 1u) ? mag[e] : 0.f;       /* SPEC:194-197 */
    }
    float th = row_allsum(part) * vad_inv;                /* SPEC:200 */
    th = th * p.spectral_k;                               /* SPEC:202 */
    float nf0, mine;
    const int old_variant = p.spectral_on == 2;
    quad_chain(th, g, nf, nfloor, nf0, mine, [&](float s, float t) {
      float n = s + (t - s) * 0.65f;                      /* SPEC:205 */
      n = n > 0.f ? n : 0.f;                              /* SPEC:206 */
      return old_variant ? t : n;                         /* BK_INO:1595-1596: no smoothing */
    });
    if (p.spectral_literal == 1) { /* SPEC:226-235 as written, as in front_frame */
#pragma unroll
      for (int e = 0; e < P; e++) {
        const float sc = ((mag[e] <= mine) ? 0.2f : fmaf(-mine, rmag[e], 1.f)) * spec_table_factor(v[e]);
        v[e].x *= sc;
        v[e].y *= sc;
      }
    } else if (p.spectral_literal) { /* the same with atan2f and the table looked up */
      const int own = lb.bi[FftPlan<256, 16>::NP - 1];
      spec_resynthesize_literal<P>(v, mine, RDSP_LATE(sin_table), wbg, [&](int e) { return own + e; });
    } else {
#pragma unroll
      for (int e = 0; e < P; e++) {
        const float sc = (mag[e] <= mine) ? 0.2f : fmaf(-mine, rmag[e], 1.f); /* SPEC:213-217, 226-235 */
        v[e].x *= sc;
        v[e].y *= sc;
      }
    }
  }
#pragma unroll
  for (int e = 0; e < P; e++) v[e] = cmul(v[e], mreg[e]); /* CONV:301 */

  inv_pass_last<N, P>(lb, v, wbg); /* CONV:309 */
  wg_sync<1>();
  {
    float2 twp[P - 1];
    tw.template get<0>(twp);
    inv_pass0_load<N, P>(lb, v, wbg, twp);
  }
  wg_sync<1>();

  /* CONV:314-318: keep the second half.  v[8 + j] = y[128 + i + 16 j]; sample o = i + 16 j of the hop */
  constexpr int Q = P / 2;
  float L[Q], R[Q], ramp[Q];
#pragma unroll
  for (int j = 0; j < Q; j++) {
    L[j] = v[Q + j].x;
    R[j] = v[Q + j].y;
    ramp[j] = (float)(i + 16 * j + 1) / (float)RDSP_BLOCK;
  }
  if (G.demod == RDSP_K_DEMOD_REAL) {
#pragma unroll
    for (int j = 0; j < Q; j++) R[j] = L[j];
  } else if (G.demod == RDSP_K_DEMOD_AM) {
    float a[Q], s = 0.f;
#pragma unroll
    for (int j = 0; j < Q; j++) {
      a[j] = __builtin_amdgcn_sqrtf(L[j] * L[j] + R[j] * R[j]);
      s += a[j];
    }
    float d0, d1;
    quad_chain(row_allsum(s), g, nf, am_dc, d0, d1, [&](float dc, float sum) {
      const float m = sum / (float)RDSP_BLOCK;
      return dc + 0.25f * (m - dc);
    });
#pragma unroll
    for (int j = 0; j < Q; j++) {
      L[j] = a[j] - (d0 + (d1 - d0) * ramp[j]);
      R[j] = L[j];
    }
  }
  const bool valid = g < nf;
  const size_t tout = (size_t)(frame_idx + g) * RDSP_BLOCK + (size_t)i;
  { /* the launch code takes this form only for chains whose audio ends here (no intermediate for a tail stage) */
    if (p.agc_on) {
      float pw = 0.f;
#pragma unroll
      for (int j = 0; j < Q; j++) pw += L[j] * L[j] + R[j] * R[j];
      float g0, g1;
      quad_chain(row_allsum(pw), g, nf, agc_g, g0, g1, [&](float gain, float sum) {
        const float pp = sum / (float)(2 * RDSP_BLOCK);
        const float rms = __builtin_amdgcn_sqrtf(pp);
        float gt = 0.25f * __builtin_amdgcn_rcpf(rms + 1e-6f);
        gt = fminf(gt, 100.0f);
        const float coef = (gt < gain) ? p.agc_attack : p.agc_decay;
        return gain + coef * (gt - gain);
      });
#pragma unroll
      for (int j = 0; j < Q; j++) {
        const float gg = g0 + (g1 - g0) * ramp[j];
        L[j] *= gg;
        R[j] *= gg;
      }
    }
    if (valid) {
#pragma unroll
      for (int j = 0; j < Q; j++) {
        const float l = L[j] * p.out_gain, r = R[j] * p.out_gain;
        const size_t o = ch * p.out_stride + tout + 16 * j;
        __builtin_nontemporal_store(pack_lr(l, r), p.out_i16 + o); /* CONV:346-347 */
        if (p.out_f32) p.out_f32[o] = make_float2(l, r);
      }
    }
  }
}

}  // namespace rdsp

#endif
