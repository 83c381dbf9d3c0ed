/*
 * rdsp_front_fd.hip -- the front kernel with the decimator in the frequency domain on wave-wide frames
 * (rdsp_front_fd_kernel), its LDS plan and its launch code.  The stages behind the decimator are front_frame /
 * front_frame_quad (rdsp_front_frame.h).  Which instance a call runs is rdsp_front_pick's decision
 * (rdsp_kernels.hip); front_fd_launch at the end of this file maps its record to the template arguments.
 */
#include <stdlib.h>

#include "rdsp_front_frame.h"
#include "rdsp_front_launch.h"

using namespace rdsp;

namespace {

/* LDS plan of rdsp_front_fd_kernel, shared with the launch code: sizes in elements, offsets in bytes */
template <int N, int P, bool Q4>
struct FrontFdLds {
  static constexpr int NW = N / P / 64;
  static constexpr int RING_N = Q4 ? QUAD_RING : (NW == 1 ? 1024 : 4096); /* float2: decimated samples */
  /* float2: the filter's work buffer, every wave's decimator work buffer, front_frame_quad's four */
  static constexpr int WB_N0 = FftPlan<N, P>::WB > NW * FftPlan<RDSP_FD_N, RDSP_FD_P>::WB ? FftPlan<N, P>::WB : NW * FftPlan<RDSP_FD_N, RDSP_FD_P>::WB;
  static constexpr int WB_N = (Q4 && QUAD_WB > WB_N0) ? QUAD_WB : WB_N0;
  static constexpr int RED_N = 64; /* float: reduction scratch */
  /* the blanker's hand-over area of the four-wave kernels: every wave's last column as blanked, the per-lane sums of
   * the open window, the level (16 bytes for it) */
  static constexpr int NBCOL_N = NW > 1 ? NW * 64 : 0; /* uint4 */
  static constexpr int NBACC_N = NW > 1 ? 64 : 0;      /* float */
  static constexpr int NBS_BYTES = NW > 1 ? 16 : 0;
  static constexpr size_t RING = 0;
  static constexpr size_t WB = RING + RING_N * sizeof(float2);
  static constexpr size_t RED = WB + WB_N * sizeof(float2);
  static constexpr size_t NBCOL = RED + RED_N * sizeof(float);
  static constexpr size_t NBACC = NBCOL + NBCOL_N * sizeof(uint4);
  static constexpr size_t NBS = NBACC + NBACC_N * sizeof(float);
  static constexpr size_t BYTES = NBS + NBS_BYTES;
};

/* ---- front kernel with the decimator in the frequency domain -----------------------------
 * Same chain as rdsp_front_kernel<N, P, 4, ...>; stage A3 (y[m] = sum_{k<256} h[k] x[4m - k]) is
 * evaluated as a polyphase overlap-save convolution instead of 1024 packed FMAs per chunk and lane:
 *     x[4q + r] = X_r[q]  (r = 0..3: the four int16 pairs of one aligned 16-byte load),
 *     y[m] = sum_r sum_{k<=64} g_r[k] X_r[m - k],   g_r[k] = h[4k - r]  (zero outside 0..255),
 * i.e. four 512-point forward transforms of the mixed input at the LOW rate (512 whatever FFT_L is:
 * 448 of 512 outputs are valid, and the radix-8 passes are the cheapest per point), a
 * multiply-accumulate with the branch spectra G_r (host-computed, /512, digit-reversed like the
 * filter mask) and ONE inverse transform: 448 valid outputs per frame.  That is the 4N-point overlap-save decimator
 * with its first two radix-2 levels folded into the masks (only N of the 4N bins survive the
 * fold by 4).  Per frame and lane at N = 512: 4 x 183 + 64 + 183 = 980 VALU instructions for
 * 1792 input samples, against 1792 packed FMAs in the direct form.
 *
 * Layout: one wave per channel; lane t owns window quads t + 64 j (j < P), exactly the
 * x[t + j NT] the first FFT pass wants, so the input goes from the 16-byte global loads straight
 * into the transform's registers -- no polyphase planes in LDS.  Consecutive windows overlap by 64
 * quads (the 256 raw samples of the FIR history): the j = P-1 quads of one frame are the j = 0
 * quads of the next and stay in registers; HBM is still read exactly once.  Decimated samples go
 * into a ring in LDS from which the overlap-save frames (front_frame) take N/2 at a time.
 *
 * Two frame lengths (template VC, new quad columns per frame; state is the same 256 raw samples as the
 * direct form in both):
 *   VC = 7 (fir_variant 2, bench.py): 448 outputs per 512-point window.  Frames are anchored at the call's first
 *     sample and the last one of a call is partial (inputs past the end of the call are zeros; every output depends
 *     on inputs at or before its own time only, so the valid ones are exact).  A stream cut into calls differently
 *     rounds differently (the frame grid moves).
 *   VC = 4 (the library's default): ONE GRANULE per frame -- 256 outputs, the window's last three columns zeros.
 *     Every call boundary is a frame boundary and a frame's input is a function of the absolute sample position:
 *     the same bits for any call split, at 5 transforms per 256 outputs instead of per 448.
 * Pipelining, sub-batches and the channel partition never change a bit in either.  The pre-processor's IQ swap and
 * the noise blanker are compiled in with PRE.
 *
 * ROTG (chains of at most RDSP_FD_ROT_GROUPS groups, rdsp_front_pick_rotg): sample 4 q + r of a quad follows sample 4 q by
 * the rotation rot_r, one constant per branch and group, and a constant factor on a transform's whole input commutes with
 * the transform:  sum_r G_r . FFT(x_r P rot_r) = sum_r (rot_r G_r) . FFT(x_r P).  The group's own rot_r G_r come from its
 * slot of p.rot_pool (filled on the host at every retune, the layout of fd_mask) and every branch is mixed with the column
 * phasors pj[j] alone: 24 complex products per frame and lane less, and rot1..3 out of the scalar registers.  Only column 0
 * of the first frame behind a retune was mixed with other rotations (roth_r): its phasor takes roth_r conj(rot_r) there.
 * The two forms round differently (1e-7); which one a chain runs depends on its number of groups alone (include/rdsp.h).
 *
 * SHF (with ROTG, the one-wave plans: rdsp_front_pick_shift): the NCO runs behind the decimator.  For a constant increment
 *     sum_k h[k] x[4m - k] exp(-j theta (4m - k)) = exp(-j theta 4m) sum_k (h[k] exp(+j theta k)) x[4m - k]:
 * the branch transforms take the converted raw samples, the group's slot of p.rot_pool holds the spectra of the shifted
 * taps (rdsp_fd_shift_image) and the frame's 64 VC outputs are multiplied by gain x exp(-j phi) at their absolute input
 * index before they go into the ring: VC complex products per frame and lane in place of 4 (VC + 1), the column phasors
 * (one nco_phasor_alu from the absolute position, then rotq1..3) on the output side, and no phasor live across the
 * transforms.  Column 0 of the first frame behind a retune came in under dphi_hist: there only, its raw samples take the
 * per-sample phasor of the increment difference, so that the window is consistent with the new theta.
 * Gains: one common gain in the frame's window (every column's I and Q gain, the history's included) rides on the output
 * phasor; anything else is scaled per sample, every column with its own two gains, and the phasor carries none.  The rule
 * looks at the frame's own columns only and is the same with and without PRE (without PRE the launch code guarantees one
 * gain), so a sample rounds the same whichever of the two kernels runs its frame. */
template <int N, int P, bool LEAN, bool PRE, bool Q4 = false, int VC = RDSP_FD_P - 1, bool ROTG = false, bool SHF = false>
__global__ void __launch_bounds__(N / P, 2) rdsp_front_fd_kernel(RdspFrontParams p) {
  static_assert(!SHF || (ROTG && N / P == 64), "the shifted spectra come from the pool; one-wave plans");
  using PL = FftPlan<N, P>;              /* the overlap-save filter's transform (FFT_L)     */
  constexpr int ND = RDSP_FD_N, PD = RDSP_FD_P; /* the decimator's: 512 points whatever FFT_L is  */
  using PLD = FftPlan<ND, PD>;
  constexpr int NT = PL::NT;
  constexpr int H = N / 2;
  constexpr int PH = P / 2;
  /* VC: quad columns of new input per decimator frame.  7 (448 outputs of the 512-point window: the throughput
   * form, fir_variant 2) or 4: frames of ONE GRANULE -- 256 outputs, the window's last three columns zeros --
   * so that every call boundary is a frame boundary and every frame's input is a function of the absolute
   * sample position: the same bits for any call split (fir_variant 4, the library's default), at 5 transforms
   * per 256 outputs instead of per 448 */
  constexpr int VAL = 64 * VC; /* valid outputs per decimator frame */
  constexpr int NC = VC + 1;   /* data columns of a frame's window: the shared / history column and VC new ones */
  static_assert(VC == PD - 1 || VC == 4, "448-sample frames or one granule per frame");
  /* FFT_L >= 2048 runs four waves per channel: every wave takes its own decimator frame (four
   * frames per round, no sums across waves), then all of them share the overlap-save frames */
  constexpr int NW = NT / 64;
  /* FFT_L 256: four overlap-save frames per pass, a 16-lane row each (front_frame_quad) */
  constexpr bool QUAD = Q4;
  static_assert(!Q4 || N == 256, "the four-frame form exists for FFT_L 256");
  using LY = FrontFdLds<N, P, Q4>;
  constexpr int RING = LY::RING_N; /* >= (H - 1) + NW * VAL, power of two (QUAD: eight padded hops) */
  constexpr bool SAME = (N == ND && P == PD);   /* one plan: twiddles and LDS bases are shared */
  static_assert((NT == 64 || NT == 256) && PLD::NT == 64, "one or four waves per channel, one per decimator frame");
  static_assert(QUAD || H - 1 + NW * VAL <= RING, "ring holds a round's outputs behind an unfinished hop");
  static_assert(!QUAD || H + (4 * H - 64) + VAL <= QUAD_HOPS * H, "the overlap hop and what is unconsumed (< 4 hops, in steps of 64) survive a frame's seven columns");

  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  float2 *ring = reinterpret_cast<float2 *>(smem_raw + LY::RING);
  float2 *wb = reinterpret_cast<float2 *>(smem_raw + LY::WB);
  float *red = reinterpret_cast<float *>(smem_raw + LY::RED);

  const bool SWAP_IQ = PRE && p.swap_iq != 0;
  /* the noise blanker takes the quad columns in stream order.  With four waves per channel the
   * frames of a round run side by side, so the blanker's pre-pass goes round the waves in frame
   * order before the transforms start: its state (level, per-lane window sums) and every frame's
   * last column as blanked (the next frame's column 0) are handed on through LDS */
  const bool NB_ON = PRE && p.nb_on != 0;
  uint4 *nbcol = reinterpret_cast<uint4 *>(smem_raw + LY::NBCOL); /* [NW][64] (four-wave kernels only) */
  float *nbacc = reinterpret_cast<float *>(smem_raw + LY::NBACC); /* [64] per-lane sums of the open window */
  float *nbs = reinterpret_cast<float *>(smem_raw + LY::NBS);     /* [0]: level */
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  float2 *wbd = wb + wave * PLD::WB; /* this wave's decimator work buffer (inside the filter's) */
  const size_t ch = (size_t)p.ch_base + blockIdx.x;
  const uint32_t *iq = p.iq + ch * p.in_stride;
  /* (twin: the group-record load of rdsp_front_rd_kernel, rdsp_front_rd.hip) */
  RdspGroup G; /* its hot fields; what only the call's first frame needs is read there (RDSP_GROUP_LATE_*) */
  const uint32_t gi = p.group_of ? (uint32_t)__builtin_amdgcn_readfirstlane((int)p.group_of[ch]) : 0u;
  {
    const uint32_t *gw = reinterpret_cast<const uint32_t *>(p.groups + gi);
    uint32_t r[32];
#pragma unroll
    for (int i = 0; i < 32; i++) r[i] = (i < 31) ? (uint32_t)__builtin_amdgcn_readfirstlane((int)gw[i]) : 0u;
    G = __builtin_bit_cast(RdspGroup, r);
  }
  const int total = p.n_chunks * 256; /* outputs = input quads of this call */

  /* raw quads of this wave's first frame (frame `wave`): column j holds quads
   * fr*VAL - 64 + lane + 64 j; for frame 0 column 0 is the FIR history (the 64 quads before the call) */
  /* The call's input of this channel as a raw buffer: a quad past the end of the call reads as zeros by the
   * buffer's range check -- no compare, no exec-mask branch and no zeroed registers per load, and the
   * loads are unconditional, so the waits for the table loads issued before them are counted exactly
   * (behind a conditional load the compiler has to assume it was not issued, and every wait for an
   * older load became a wait for the whole prefetch: an HBM round trip inside the frame) */
  const __amdgpu_buffer_rsrc_t iq_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t *>(iq), 0, 16 * total, 0x00020000);
  auto ld_quad = [&](int q) { /* (twin: ld_quad of rdsp_front_rd_kernel, rdsp_front_rd.hip) */
    typedef int v4i __attribute__((ext_vector_type(4)));
    /* aux 2 = nt: the stream passes once (one wave per channel).  Four waves per channel re-read each other's
     * frame overlap, which they should find in L2: default policy there */
    const v4i v = __builtin_amdgcn_raw_buffer_load_b128(iq_rsrc, 16 * q, 0, NW == 1 ? 2 : 0);
    return make_uint4((uint32_t)v.x, (uint32_t)v.y, (uint32_t)v.z, (uint32_t)v.w);
  };
  uint4 rq[NC];
#pragma unroll
  for (int j = 0; j < NC; j++) {
    const int q = wave * VAL - 64 + lane + 64 * j;
    if (q < 0) rq[j] = *reinterpret_cast<const uint4 *>(p.st_hist + ch * 256 + 4 * lane);
    else rq[j] = ld_quad(q);
  }

  Twiddles<N, P, LEAN> tw;
  LdsBases<N, P, false> lb;
  if constexpr (!QUAD) {
    tw.init(tid);
    make_lds_bases<N, P, false>(tid, lb);
  }
  /* FFT_L 256: the 16-point-per-lane plan of front_frame_quad, a lane's place in its row */
  Twiddles<256, 16, LEAN> tw16;
  LdsBases<256, 16, false> lb16;
  if constexpr (QUAD) {
    tw16.init(lane & 15);
    make_lds_bases<256, 16, false>(lane & 15, lb16);
  }
  const int mbase = 16 * (lane & 3) + 4 * ((lane >> 2) & 3); /* this lane's bins in the radix-4 plan's mask image */
  /* the decimator's plan: its own twiddles and LDS bases unless it is the filter's plan */
  Twiddles<ND, PD, false> twd_own;
  LdsBases<ND, PD, false> lbd_own;
  if constexpr (!SAME) {
    twd_own.init(lane);
    make_lds_bases<ND, PD, false>(lane, lbd_own);
  }
  const auto &twd = [&]() -> const auto & { if constexpr (SAME) return tw; else return twd_own; }();
  const auto &lbd = [&]() -> const auto & { if constexpr (SAME) return lb; else return lbd_own; }();
  uint32_t vadbits = 0; /* (twins: the VAD bits of rdsp_front_rd_kernel, rdsp_front_rd.hip, and of rdsp_front_kernel, rdsp_front_direct.hip) */
  if constexpr (QUAD) {
#pragma unroll
    for (int e = 0; e < 16; e++) {
      const int k = (lane & 15) + 16 * e; /* bin_of_pos<256, 16>(16 i + e) */
      if (k >= p.vad_lo && k <= p.vad_hi) vadbits |= 1u << e;
    }
  } else {
#pragma unroll
    for (int e = 0; e < P; e++) {
      int k = bin_of_pos<N, P>(tid * P + e);
      if (k >= p.vad_lo && k <= p.vad_hi) vadbits |= 1u << e;
    }
  }
  /* state in (twin: rdsp_front_rd_kernel, rdsp_front_rd.hip) */
  float nfloor = p.st_scal[ch * 4 + 0];
  const float vad_inv = 1.0f / (float)(p.vad_hi - p.vad_lo);
  float agc_g = p.st_scal[ch * 4 + 1];
  float am_dc = p.st_scal[ch * 4 + 2];
  float nb_level = p.st_scal[ch * 4 + 3], nb_acc = 0.f;
  uint4 hist_save = make_uint4(0u, 0u, 0u, 0u); /* the call's last 64 quads as they entered the decimator */
  float2 vprev[PH];
  if constexpr (QUAD) { /* the previous hop goes in front of the ring's first one (the last of the ring) */
#pragma unroll
    for (int j = 0; j < PH; j++) ring[(QUAD_HOPS - 1) * QUAD_PITCH + tid + j * NT] = p.st_prev[ch * H + tid + j * NT];
  } else {
#pragma unroll
    for (int j = 0; j < PH; j++) vprev[j] = p.st_prev[ch * H + tid + j * NT];
  }
  int frame_idx = 0;
  int produced = 0, consumed = 0;
  int rhop = 0; /* QUAD: ring hop of the oldest unconsumed sample */
  auto wsync = []() { wg_sync<1>(); };
  if constexpr (NW > 1) {
    if (NB_ON) {
      if (tid < 64) nbacc[tid] = 0.f;
      if (tid == 0) nbs[0] = nb_level;
      wg_sync<NW>();
    }
  }

#pragma unroll 1
  for (int round = 0; produced < total; round++) {
    const int fr = round * NW + wave; /* this wave's frame; past the end of the call it works on zeros */
    if (NB_ON) {
      /* noise blanker (engine feature, build-defined): decision windows of 1024 input samples =
       * four quad columns; a frame brings seven new columns (j = 1..7), taken in stream order.  A
       * sample whose power exceeds the reference level x threshold is zeroed in the raw word, so it
       * stays blanked in the next frame's column 0 and in the FIR history; the level moves at the
       * end of every window from the mean post-blanking power (one wave reduction) */
      auto blank_frame = [&]() {
#pragma unroll
        for (int j = 1; j < NC; j++) {
          const int c = VC * fr + (j - 1); /* column of the call */
          if (64 * c < total) {
            const float thr = nb_level * p.nb_thr;
            uint32_t w[4] = {rq[j].x, rq[j].y, rq[j].z, rq[j].w};
#pragma unroll
            for (int r = 0; r < 4; r++) {
              const uint32_t ww = SWAP_IQ ? __builtin_amdgcn_alignbit(w[r], w[r], 16) : w[r];
              const float2 x = unpack_iq(ww, p.scale_i, p.scale_q);
              const float pw = x.x * x.x + x.y * x.y;
              const bool blanked = nb_level > 0.f && pw > thr;
              w[r] = blanked ? 0u : w[r];
              nb_acc += blanked ? 0.f : pw;
            }
            rq[j] = make_uint4(w[0], w[1], w[2], w[3]);
            if ((c & 3) == 3) {
              const float mean = wave_sum(nb_acc) / 1024.0f;
              nb_level = (nb_level > 0.f) ? nb_level + 0.2f * (mean - nb_level) : mean;
              nb_acc = 0.f;
            }
            if (64 * (c + 1) == total) {
              if constexpr (NW == 1) hist_save = rq[j];
              else *reinterpret_cast<uint4 *>(RDSP_LATE(st_hist) + ch * 256 + 4 * lane) = rq[j]; /* the call's last 64 quads */
            }
          }
        }
      };
      if constexpr (NW == 1) {
        blank_frame();
      } else {
#pragma unroll 1
        for (int w = 0; w < NW; w++) {
          if (wave == w) {
            nb_level = nbs[0];
            nb_acc = nbacc[lane];
            if (fr > 0) rq[0] = nbcol[(w + NW - 1) % NW * 64 + lane]; /* the frame before, as blanked */
            blank_frame();
            nbcol[w * 64 + lane] = rq[VC];
            nbacc[lane] = nb_acc;
            if (lane == 0) nbs[0] = nb_level;
          }
          wg_sync<NW>();
        }
      }
    }
    /* ---- A2: phasors of this lane's P quad columns (sample 4 q + r of a quad follows by rot_r) */
    const uint32_t nq = p.n0 + 4u * (uint32_t)(fr * VAL - 64 + lane); /* absolute index of column 0 */
    const bool hist = (fr == 0);
    /* column 0 of the call's first frame is the previous call's samples: they keep the swap flag and
     * the gains they came in with (uniform values, chosen once per frame).  Only the PRE kernels carry
     * this: the launch code picks them for the one call after such a setting changed */
    float si0 = p.scale_i, sq0 = p.scale_q;
    bool swap0 = PRE && p.swap_iq != 0;
    uint32_t dphi_hist = G.dphi;
    if (hist) { /* round 0 only: read here, not held in scalar registers for the whole launch */
      if constexpr (PRE) {
        si0 = RDSP_LATE(scale_i_hist);
        sq0 = RDSP_LATE(scale_q_hist);
        swap0 = RDSP_LATE(swap_hist) != 0;
      }
      dphi_hist = RDSP_GROUP_LATE_U32(gi, dphi_hist);
    }
    /* Gains.  A column whose I and Q gains are equal carries its gain on the phasor (two packed multiplies per
     * frame instead of 32 on the samples; x (g ph) = (x g) ph to the bit when g is a power of two -- unit input
     * gain -- and to an ulp otherwise); a column with two gains (IQ balance) is scaled per sample.  The rule
     * looks at the column's own gains only, in the kernels with and without PRE alike (without PRE the launch
     * code guarantees one gain, history included), so how a sample rounds does not depend on which of the two
     * kernels a call split happens to run it through */
    /* SHF: the phasor is on the output side, behind the sum over the window's columns: it can carry one gain only, the
     * one every column of this frame has (the kernel's comment) */
    const bool one = p.scale_i == p.scale_q && si0 == p.scale_i && sq0 == p.scale_q;
    const bool fold = !PRE || (SHF ? one : p.scale_i == p.scale_q), fold0 = !PRE || (SHF ? one : si0 == sq0);
    const float gph = fold ? p.scale_i : 1.0f, gph0 = fold0 ? si0 : 1.0f;      /* on the phasor ...           */
    const float sxi = fold ? 1.0f : p.scale_i, sxq = fold ? 1.0f : p.scale_q;  /* ... or on the samples (x 1.0 is exact) */
    const float sxi0 = fold0 ? 1.0f : si0, sxq0 = fold0 ? 1.0f : sq0;
    const bool retuned = hist && dphi_hist != G.dphi; /* column 0 came in under another increment */
    float2 pj[NC];
    if constexpr (!SHF) {
      float2 b1u = make_float2(1.f, 0.f);
      if (G.dphi != 0u) b1u = nco_phasor_alu((nq + 256u) * G.dphi);
      const float2 b1 = make_float2(b1u.x * gph, b1u.y * gph); /* the gain first, the rotations after it */
      /* column 0: one column before b1, evaluated the same way in every frame -- a frame's phasors are a
       * function of its absolute position (and the column's own gain), not of where the call began.  Only
       * behind a retune (the previous call's samples were mixed with another increment) it is evaluated
       * directly with that increment */
      if (hist && dphi_hist != G.dphi) {
        const float2 d = (dphi_hist != 0u) ? nco_phasor_alu(nq * dphi_hist) : make_float2(1.f, 0.f);
        pj[0] = make_float2(d.x * gph0, d.y * gph0);
      } else if (PRE && gph0 != gph) {
        pj[0] = cmulc_uniform(make_float2(b1u.x * gph0, b1u.y * gph0), G.rotq1);
      } else {
        pj[0] = cmulc_uniform(b1, G.rotq1);
      }
      pj[1] = b1;
      if constexpr (PD > 2) pj[2] = cmul_pinned_u(b1, G.rotq1);
      if constexpr (PD > 3) pj[3] = cmul_pinned_u(b1, G.rotq2);
#pragma unroll
      for (int j = 4; j < NC; j++) pj[j] = cmul_pinned_u(pj[j - 3], G.rotq3);
    }

    /* ---- A1 + A3: four branch transforms, multiply-accumulate with the branch spectra ------- */
    float2 acc[PD];
#pragma unroll
    for (int r = 0; r < 4; r++) {
      float2 gm[PD]; /* G_r slice of this lane: L2-resident, lands behind the transform */
      {
        const float2 *mp = ROTG ? p.rot_pool + G.rot_off + (size_t)r * ND : p.fd_mask + (size_t)r * ND;
        asm volatile("" : "+s"(mp));
        const auto gp = as_global(mp);
#pragma unroll
        for (int e = 0; e < PD; e++) gm[e] = gp[e * 64 + lane];
      }
      float2 v[PD];
#pragma unroll
      for (int j = NC; j < PD; j++) v[j] = make_float2(0.f, 0.f); /* granule frames: the rest of the window is zeros */
#pragma unroll
      for (int j = 0; j < NC; j++) {
        uint32_t w = (r == 0) ? rq[j].x : (r == 1) ? rq[j].y : (r == 2) ? rq[j].z : rq[j].w;
        if (j == 0 ? swap0 : SWAP_IQ) w = __builtin_amdgcn_alignbit(w, w, 16);
        float2 x = make_float2((float)(int16_t)(w & 0xFFFFu), (float)(int16_t)(w >> 16));
        if constexpr (PRE) x = make_float2(x.x * (j == 0 ? sxi0 : sxi), x.y * (j == 0 ? sxq0 : sxq));
        if constexpr (SHF) {
          /* raw samples; behind a retune the history column turns by the difference of the two increments, per sample */
          if (j == 0 && retuned) x = cmul_pinned(x, nco_phasor_alu((nq + (uint32_t)r) * (dphi_hist - G.dphi)));
          v[j] = x;
          continue;
        }
        float2 ph = pj[j];
        if constexpr (ROTG) {
          /* rot_r rides on the branch's spectrum; the history column behind a retune came in under roth_r */
          if (r > 0 && j == 0 && hist && dphi_hist != G.dphi) {
            ph = cmul_pinned_u(ph, (r == 1) ? RDSP_GROUP_LATE_F2(gi, roth1) : (r == 2) ? RDSP_GROUP_LATE_F2(gi, roth2) : RDSP_GROUP_LATE_F2(gi, roth3));
            ph = cmulc_uniform(ph, (r == 1) ? RDSP_GROUP_LATE_F2(gi, rot1) : (r == 2) ? RDSP_GROUP_LATE_F2(gi, rot2) : RDSP_GROUP_LATE_F2(gi, rot3));
          }
        } else if (r > 0) {
          const float2 rr = (r == 1) ? G.rot1 : (r == 2) ? G.rot2 : G.rot3;
          if (j == 0) { /* the history column of the call's first frame: the rotation it was mixed with */
            float2 r0 = rr;
            if (hist) r0 = (r == 1) ? RDSP_GROUP_LATE_F2(gi, roth1) : (r == 2) ? RDSP_GROUP_LATE_F2(gi, roth2) : RDSP_GROUP_LATE_F2(gi, roth3);
            ph = cmul_pinned_u(ph, r0);
          } else {
            ph = cmul_pinned_u(ph, rr);
          }
        }
        v[j] = cmul_pinned(x, ph);
      }
      if (r == 3) { /* the raw registers are free: the next frame's loads land behind the transforms */
        if constexpr (NW == 1) rq[0] = rq[VC]; /* consecutive frames share a column */
#pragma unroll
        for (int j = (NW == 1 ? 1 : 0); j < NC; j++) {
          const int q = (fr + NW) * VAL - 64 + lane + 64 * j; /* >= 0: this is frame 1 or later */
          rq[j] = ld_quad(q);
        }
      }
      {
        float2 twp[PD - 1];
        twd.template get<0>(twp);
        fwd_pass0_store<ND, PD>(lbd, v, wbd, twp);
      }
      /* the decimator's transforms run in a work buffer of the wave's own (wbd), also with four waves per
       * channel: the lanes of ONE wave are all that has to be ordered here.  Between waves the barriers are the
       * one behind the ring writes below and the one that ends every overlap-save frame ("wb is free again") */
      wg_sync<1>();
      fwd_mid_all<ND, PD, 1, PLD::NP - 1, false>(lbd, wbd, twd, wsync);
      fwd_pass_last<ND, PD>(lbd, v, wbd);
      wg_sync<1>(); /* wbd is rewritten by the next branch */
#pragma unroll
      for (int e = 0; e < PD; e++) acc[e] = (r == 0) ? cmul(v[e], gm[e]) : cmac(acc[e], v[e], gm[e]);
    }
    inv_pass_last<ND, PD>(lbd, acc, wbd);
    wg_sync<1>();
    inv_mid_all<ND, PD, PLD::NP - 2, false>(lbd, wbd, twd, wsync);
    {
      float2 twp[PD - 1];
      twd.template get<0>(twp);
      inv_pass0_load<ND, PD>(lbd, acc, wbd, twp);
    }
    /* acc[j] = y at window index lane + 64 j; index 64 (j = 1) is output fr*VAL of the call */
    if constexpr (SHF) {
      /* the NCO, on the decimated samples: output j stands at input column j of the window (nq + 256 j), its phasor a
       * function of that absolute position -- and of the window's common gain, if it has one */
      float2 b1u = make_float2(1.f, 0.f);
      if (G.dphi != 0u) b1u = nco_phasor_alu((nq + 256u) * G.dphi);
      float2 po[NC];
      po[1] = make_float2(b1u.x * gph, b1u.y * gph); /* the gain first, the rotations after it */
      if constexpr (NC > 2) po[2] = cmul_pinned_u(po[1], G.rotq1);
      if constexpr (NC > 3) po[3] = cmul_pinned_u(po[1], G.rotq2);
#pragma unroll
      for (int j = 4; j < NC; j++) po[j] = cmul_pinned_u(po[j - 3], G.rotq3);
#pragma unroll
      for (int j = 1; j < NC; j++) acc[j] = cmul_pinned(acc[j], po[j]);
    }
    {
      /* a frame's outputs start at a multiple of 64 in the ring, so a column of 64 never wraps: the wrap is
       * scalar arithmetic per column, one vector add per store (past the end of the call: slots nobody
       * consumes, `produced` stops at total) */
      if constexpr (QUAD) { /* columns of 64 in padded hops */
        const int w0 = __builtin_amdgcn_readfirstlane((fr * VC) % (2 * QUAD_HOPS));
#pragma unroll
        for (int j = 1; j < NC; j++) {
          int cw = w0 + (j - 1);
          cw = cw >= 2 * QUAD_HOPS ? cw - 2 * QUAD_HOPS : cw;
          ring[cw * 64 + (cw >> 1) * (QUAD_PITCH - 128) + lane] = acc[j];
        }
      } else {
        const int m0 = __builtin_amdgcn_readfirstlane(fr * VAL);
        static_assert(VAL % 64 == 0 && (QUAD || RING % 64 == 0), "ring columns");
#pragma unroll
        for (int j = 1; j < NC; j++) ring[((m0 + 64 * (j - 1)) & (RING - 1)) + lane] = acc[j];
      }
    }
    produced = (round + 1) * NW * VAL < total ? (round + 1) * NW * VAL : total;
    wg_sync<NW>();

    /* ---- A5/A6: overlap-save frames over what the ring holds ------------------------------
     * (twin: the hop-consumer loops and their mask slice in rdsp_front_rd_kernel, rdsp_front_rd.hip) */
    if constexpr (QUAD) {
      /* four at a time; at the end of the call whatever is left (frames are complete hops: the call is whole granules) */
#pragma unroll 1
      while (produced - consumed >= 4 * H || (produced == total && produced - consumed >= H)) {
        int nf = (produced - consumed) / H;
        nf = nf > 4 ? 4 : nf;
        front_frame_quad(p, G, tw16, lb16, wb + (lane >> 4) * FftPlan<256, 16>::WB, ring, rhop, nf, mbase, vadbits, vad_inv,
                         nfloor, agc_g, am_dc, frame_idx, ch, lane);
        frame_idx += nf;
        consumed += nf * H;
        rhop += nf;
        rhop = rhop >= QUAD_HOPS ? rhop - QUAD_HOPS : rhop;
      }
      continue;
    }
#pragma unroll 1
    while (produced - consumed >= H) {
      float2 mreg[P];
      {
        const float2 *mp = p.mask_pool + G.mask_off;
        asm volatile("" : "+s"(mp));
        const auto gp = as_global(mp);
#pragma unroll
        for (int e = 0; e < P; e++) mreg[e] = gp[e * NT + tid];
      }
      /* hops start at multiples of H in a ring of a multiple of H: the hop is contiguous */
      static_assert(QUAD || RING % H == 0, "a hop never wraps");
      const float2 *hop = ring + (consumed & (RING - 1));
      front_frame<N, P, false>(p, G, tw, lb, wb, red, mreg, vadbits, vad_inv, vprev, nfloor, agc_g, am_dc, frame_idx, ch,
                               tid, [&](int i) { return hop[i]; });
      consumed += H;
    }
  }

  /* ---- state out: previous hop, the last 256 raw samples (an L2 re-read), scalars ---------
   * (twin: rdsp_front_rd_kernel, rdsp_front_rd.hip) */
  float2 *const st_prev = RDSP_LATE(st_prev); /* the state pointers again: not kept across the frame loop */
  uint32_t *const st_hist = RDSP_LATE(st_hist);
  float *const st_scal = RDSP_LATE(st_scal);
  if constexpr (QUAD) {
    const int hp = rhop == 0 ? QUAD_HOPS - 1 : rhop - 1; /* the last hop consumed */
#pragma unroll
    for (int j = 0; j < PH; j++) st_prev[ch * H + tid + j * NT] = ring[hp * QUAD_PITCH + tid + j * NT];
  } else {
#pragma unroll
    for (int j = 0; j < PH; j++) st_prev[ch * H + tid + j * NT] = vprev[j];
  }
  if (tid < 64 && !(NB_ON && NW > 1)) /* four waves with the blanker: stored by the wave that blanked them */
    *reinterpret_cast<uint4 *>(st_hist + ch * 256 + 4 * tid) =
        NB_ON ? hist_save : *reinterpret_cast<const uint4 *>(iq + 4 * (total - 64 + tid));
  if (tid == 0) {
    st_scal[ch * 4 + 0] = nfloor;
    if (!p.to_mid) st_scal[ch * 4 + 1] = agc_g;
    st_scal[ch * 4 + 2] = am_dc;
    if (NB_ON) st_scal[ch * 4 + 3] = (NW > 1) ? nbs[0] : nb_level;
  }
}

/* Measurement switch RDSP_FD_LDS_PAD (bytes): unused LDS asked for on top of the one-wave frequency-domain kernels' own,
 * so that fewer of their workgroups fit on a compute unit beside the tail kernel (pipelined mode).  Both forms lose by
 * it (tests/micro/fd_lds_pad_sweep.sh, fd_lds_pad_sweep7.sh): the library never pads. */
inline size_t granule_form_lds_pad(int to_mid) {
  static const long env = getenv("RDSP_FD_LDS_PAD") ? atol(getenv("RDSP_FD_LDS_PAD")) : -1;
  if (env >= 0) return (size_t)env;
  (void)to_mid;
  return 0;
}

template <int N, int P, bool LEAN, bool PRE, bool Q4, int VC, bool ROTG, bool SHF>
int launch_fd(const RdspFrontParams *p, int n_channels, hipStream_t stream) {
  constexpr size_t lds = FrontFdLds<N, P, Q4>::BYTES;
  static_assert(!Q4 || lds <= 48 * 1024, "no raised dynamic-LDS limit needed");
  if constexpr (lds > 48 * 1024) {
    int e = ensure_lds_limit<&rdsp_front_fd_kernel<N, P, LEAN, PRE, Q4, VC, ROTG, SHF>>(lds);
    if (e != 0) return e;
  }
  size_t ask = lds;
  if constexpr (!Q4 && lds <= 16 * 1024) ask = lds + granule_form_lds_pad(p->to_mid);
  hipLaunchKernelGGL((rdsp_front_fd_kernel<N, P, LEAN, PRE, Q4, VC, ROTG, SHF>), dim3(n_channels), dim3(N / P), ask, stream, *p);
  return (int)hipGetLastError();
}

/* the instances that exist: no full-register one at radix 16, four frames per pass at FFT_L 256 only */
template <int N, int P, bool LEAN, bool Q4>
constexpr bool fd_instance = (LEAN || P != 16) && (!Q4 || N == 256);

}  // namespace

int rdsp::front_fd_launch(int fft_l, const RdspFrontPick &k, const RdspFrontParams *p, int n_channels, hipStream_t stream) {
  if (k.frame != 4 && k.frame != RDSP_FD_P - 1) return (int)hipErrorInvalidValue;
  return with_front_plan(fft_l, (int)hipErrorInvalidValue, [&](auto plan) {
    return with_flag(k.lean, [&](auto lean) {
      return with_flag(k.pre, [&](auto pre) {
        return with_flag(k.q4, [&](auto q4) {
          constexpr int N = decltype(plan)::N, P = decltype(plan)::P;
          constexpr bool LEAN = decltype(lean)::value, PRE = decltype(pre)::value, Q4 = decltype(q4)::value;
          if constexpr (fd_instance<N, P, LEAN, Q4>)
            return with_flag(rdsp_front_pick_rotg(p) != 0, [&](auto rotg) {
              return with_flag(rdsp_front_pick_shift(fft_l, p) != 0, [&](auto shf) {
                constexpr bool ROTG = decltype(rotg)::value, SHF = decltype(shf)::value;
                if constexpr (SHF && !(ROTG && N / P == 64)) return (int)hipErrorInvalidValue; /* no such instance */
                else
                  return k.frame == 4 ? launch_fd<N, P, LEAN, PRE, Q4, 4, ROTG, SHF>(p, n_channels, stream)
                                      : launch_fd<N, P, LEAN, PRE, Q4, RDSP_FD_P - 1, ROTG, SHF>(p, n_channels, stream);
              });
            });
          else return (int)hipErrorInvalidValue;
        });
      });
    });
  });
}
