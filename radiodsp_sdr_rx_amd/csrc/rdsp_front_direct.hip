/*
 * rdsp_front_direct.hip -- the front kernel with the decimator in direct form (or none), hand-written for CDNA4
 * (gfx950).  No MFMA: the path is streaming FIR/FFT work in fp32.
 *
 *   rdsp_front_kernel<N,P,DECIM>  one channel per workgroup of NT = N/P threads
 *       A1  int16 IQ unpack           RDSP_convolutional.h:241-242
 *       A2  NCO mixer                 (AudioSDR, build-defined)
 *       A3  256-tap polyphase /4 FIR  (build-defined)
 *       A5  overlap-save filter       RDSP_convolutional.h:256-318
 *       A6  spectral subtraction NR   backup/RDSP_convolutional_spec.h:182-238
 *       demod select, and when no NLMS stage is active: A9 AGC, output gain,
 *       A10 pack                      RDSP_convolutional.h:342-350
 *   (A5 onwards: front_frame, rdsp_front_frame.h)
 *
 * Data movement: int16 IQ is read once with 16-byte coalesced loads (prefetched
 * one chunk ahead), everything between stays in LDS/registers, and audio is
 * written once.  Per-channel state (FIR history, overlap block, NFloor, AGC
 * gain) is read at launch start and written back at the end, so
 * its traffic is amortised over the time batch.
 *
 * Which instance a call runs is rdsp_front_pick's decision (rdsp_kernels.hip); front_direct_launch at the end of
 * this file maps its record to the template arguments.
 */
#include "rdsp_front_frame.h"
#include "rdsp_front_launch.h"

using namespace rdsp;

namespace {

/* ---- front kernel -------------------------------------------------------- */
/* LDS plan of the front kernel (float2 units), shared with the launch code */
template <int N, int P, int DECIM>
struct FrontLds {
  static constexpr int NT = N / P;
  static constexpr int H = N / 2;
  static constexpr int XS_N = (DECIM == 4) ? 16 * RDSP_XP : 0;
  static constexpr int HB_N = (H > 256) ? H : 256; /* new samples of one chunk / one hop */
  /* one-wave kernels with a work buffer that fits behind the FIR history reuse the planes */
  static constexpr bool ALIAS = (DECIM == 4) && (NT == 64) && (N <= 512);
  static constexpr int WB_N = ALIAS ? 0 : FftPlan<N, P>::WB;
  static constexpr int TAPS_N = (DECIM == 4) ? 128 : 0;
  static constexpr size_t BYTES = (size_t)(XS_N + HB_N + WB_N + TAPS_N) * sizeof(float2) + 64 * sizeof(float);
};

/* LEAN = true trades registers for a little recomputation (twiddle powers per pass,
 * mask slice re-read per chunk).  It pays at radix 16, where it buys the second wave per
 * SIMD.  At radix 8 it was what let two front waves and a tail wave share the 512-register
 * file of a SIMD in pipelined mode; since the butterflies and the FIR were written out by
 * hand the full-register kernel needs 185 VGPRs, fits as well (2 x 192 + 112) and is the
 * default in both modes (the lean one stays selectable, rdsp_chain_set_front_variant).
 * The decimating FIR as v_mfma_f32_16x16x4_f32 GEMM slices was built and measured (docs/history.md, DESIGN.md
 * section 4.1c): fp32 MFMA and fp32 VALU work do not overlap on a gfx950 SIMD (tests/micro/mfma_valu_overlap.hip:
 * one wave of each takes the sum of both times), so it is not a second pipe; it won 10 % at K2, 6 % on the K3
 * front kernel and 2 % at K4 through fewer LDS reads and instructions and 40-60 fewer VGPRs -- and its 32-cycle
 * instructions starved a co-resident tail wave (pipelined K3: 2.21 -> 2.58 ms).  Not adopted. */
template <int N, int P, int DECIM, bool LEAN, bool PRE>
__global__ void __launch_bounds__(N / P, 2) rdsp_front_kernel(RdspFrontParams p) {
  using PL = FftPlan<N, P>;
  constexpr int NT = PL::NT;
  constexpr int NW = NT / 64;
  constexpr int H = N / 2;
  constexpr int PH = P / 2;
  constexpr int CH_OUT = 256;
  constexpr int CH_IN = CH_OUT * DECIM;
  constexpr int FPC = (H >= CH_OUT) ? 1 : CH_OUT / H; /* frames per chunk */
  constexpr int CPF = (H >= CH_OUT) ? H / CH_OUT : 1; /* chunks per frame */
  using LY = FrontLds<N, P, DECIM>;
  constexpr bool ALIAS = LY::ALIAS;
  constexpr int LP = (CH_IN / 4 + NT - 1) / NT; /* uint4 loads per thread per chunk */
  static_assert(DECIM == 1 || DECIM == 4, "decimation 1 or 4");
  static_assert(NT == 64 || NT == 256, "one or four waves per channel");
  static_assert(NW == 1 || PL::WB >= 4 * CH_OUT, "work buffer holds the FIR partial sums");
  static_assert(LP == 4 || LP == 1, "the history phasor below follows the scatter loop's passes");

  /* LDS: [polyphase planes | new hop(s) | work buffer (unless aliased into the
   * planes) | decimator taps | reduction scratch].  The previous hop is not in
   * LDS: every thread keeps its own P/2 elements of it in registers (vprev). */
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  float2 *xs = reinterpret_cast<float2 *>(smem_raw);
  float2 *hb = xs + LY::XS_N;
  float2 *wb = ALIAS ? xs : hb + LY::HB_N;
  float4 *taps_lds = reinterpret_cast<float4 *>(hb + LY::HB_N + (ALIAS ? 0 : PL::WB));
  float *red = reinterpret_cast<float *>(reinterpret_cast<float2 *>(taps_lds) + LY::TAPS_N);

  /* PRE: the pre-processor's IQ swap and the noise blanker are compiled in (their
   * run-time tests inside the unpack loop cost ~2 % when both are off, measured) */
  const bool NB_ON = PRE && p.nb_on != 0, SWAP_IQ = PRE && p.swap_iq != 0;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const size_t ch = (size_t)p.ch_base + blockIdx.x;
  const uint32_t *iq = p.iq + ch * p.in_stride;
  /* this channel's group record into scalar registers */
  RdspGroup G;
  {
    const uint32_t gi = p.group_of ? (uint32_t)p.group_of[ch] : 0u;
    const uint32_t *gw = reinterpret_cast<const uint32_t *>(p.groups + gi);
    uint32_t r[32];
#pragma unroll
    for (int i = 0; i < 32; i++) r[i] = (i < 24) ? (uint32_t)__builtin_amdgcn_readfirstlane((int)gw[i]) : 0u;
    G = __builtin_bit_cast(RdspGroup, r);
  }

  /* first uint4 loads of chunk 0 go out before anything else */
  uint4 raw[LP];
#pragma unroll
  for (int k = 0; k < LP; k++) {
    int idx = tid + NT * k;
    if (idx < CH_IN / 4) raw[k] = *reinterpret_cast<const uint4 *>(iq + 4 * idx);
  }

  /* per-thread constants that stay in registers for the whole launch: FFT
   * twiddles, LDS bases of every pass, this thread's slice of the filter mask
   * (digit-reversed, /N), its VAD-bin membership bits and its four taps */
  Twiddles<N, P, LEAN> tw;
  tw.init(tid);
  LdsBases<N, P, ALIAS> lb;
  make_lds_bases<N, P, ALIAS>(tid, lb);
  uint32_t vadbits = 0; /* (twins: the VAD bits of rdsp_front_fd_kernel, rdsp_front_fd.hip, and rdsp_front_rd_kernel, rdsp_front_rd.hip) */
#pragma unroll
  for (int e = 0; e < P; e++) {
    int k = bin_of_pos<N, P>(tid * P + e);
    if (k >= p.vad_lo && k <= p.vad_hi) vadbits |= 1u << e;
  }
  if constexpr (DECIM == 4) {
    if (tid < 64) taps_lds[tid] = reinterpret_cast<const float4 *>(p.fir_hc)[tid];
  }

  float nfloor = p.st_scal[ch * 4 + 0];
  const float vad_inv = 1.0f / (float)(p.vad_hi - p.vad_lo); /* SPEC:200, once per launch */
  float agc_g = p.st_scal[ch * 4 + 1];
  float am_dc = p.st_scal[ch * 4 + 2];
  float nb_level = p.st_scal[ch * 4 + 3];

  /* state in: previous hop -> registers, FIR history -> polyphase planes */
  float2 vprev[PH];
#pragma unroll
  for (int j = 0; j < PH; j++) vprev[j] = p.st_prev[ch * H + tid + j * NT];
  if constexpr (DECIM == 4) {
    for (int i = tid; i < 64; i += NT) {
      uint4 w4 = *reinterpret_cast<const uint4 *>(p.st_hist + ch * 256 + 4 * i);
      uint32_t w[4] = {w4.x, w4.y, w4.z, w4.w};
      if (PRE && p.swap_hist != 0) { /* the stored history is the raw stream: swapped as the call it came in with swapped */
#pragma unroll
        for (int k = 0; k < 4; k++) w[k] = __builtin_amdgcn_alignbit(w[k], w[k], 16);
      }
      /* the same phasor arithmetic these samples went through as the last 256 of the
       * previous chunk (pass LP-1 of the scatter loop below), so that a stream gives
       * the same bits however it is cut into calls */
      float2 ph0 = make_float2(1.f, 0.f);
      if (G.dphi_hist != 0u) {
        if constexpr (LP == 4) {
          ph0 = nco_phasor_alu((p.n0 - (uint32_t)CH_IN + 4u * (uint32_t)i) * G.dphi_hist);
          ph0 = cmul_pinned_u(ph0, G.rothp3);
        } else {
          ph0 = nco_phasor_alu((p.n0 - 256u + 4u * (uint32_t)i) * G.dphi_hist);
        }
      }
#pragma unroll
      for (int k = 0; k < 4; k++) {
        float2 x = unpack_iq(w[k], PRE ? p.scale_i_hist : p.scale_i, PRE ? p.scale_q_hist : p.scale_q); /* ... and the gains of that call */
        { /* the history keeps the mixing it went through when it was new (identity phasors when
           * the NCO was off: roth* are (1, -0) then and the products are exact) */
          float2 ph = (k == 0) ? ph0 : cmul_pinned_u(ph0, k == 1 ? G.roth1 : (k == 2 ? G.roth2 : G.roth3));
          x = cmul_pinned(x, ph);
        }
        xs[xs_pos(-256 + 4 * i + k)] = x;
      }
    }
  }
  int frame_idx = 0;
  wg_sync<NW>();

  for (int chunk = 0; chunk < p.n_chunks; chunk++) {
    /* ---- A1 + A2: unpack, gains, mix; scatter into the polyphase planes ----
     * One accurate phasor per thread per chunk (ALU only: no memory traffic in
     * the loop besides the IQ stream); the other samples of the thread follow
     * by constant rotations (k*4*NT samples between passes, 1..3 inside one). */
    /* (twins: the mask slice in the hop-consumer loops of rdsp_front_fd_kernel and rdsp_front_rd_kernel)
     * this thread's slice of the mask (digit-reversed, /N, thread-major): L2-resident,
     * requested at the top of the chunk and consumed after the forward transform, so
     * its latency hides behind the FIR.  The pointer is made opaque so the loads are
     * not hoisted out of the chunk loop into 2P persistent registers. */
    float2 mreg[P];
    {
      const float2 *mp = p.mask_pool + G.mask_off;
      if constexpr (LEAN) asm volatile("" : "+s"(mp));
      const auto gp = as_global(mp);
#pragma unroll
      for (int e = 0; e < P; e++) mreg[e] = gp[e * NT + tid];
    }
    float2 ph_base = make_float2(1.f, 0.f);
    if (G.dphi != 0u)
      ph_base = nco_phasor_alu((p.n0 + (uint32_t)chunk * CH_IN + 4u * (uint32_t)tid) * G.dphi);
    /* noise blanker (engine feature, build-defined): one decision window per chunk; the
     * threshold comes from the windows before this one, so the chunk stays parallel */
    const float nb_t = nb_level * p.nb_thr;
    float nb_acc = 0.f;
#pragma unroll
    for (int k = 0; k < LP; k++) {
      int idx = tid + NT * k;
      if (idx < CH_IN / 4) {
        uint32_t w[4] = {raw[k].x, raw[k].y, raw[k].z, raw[k].w};
        if (SWAP_IQ) { /* preProcessor.swapIQ(true), INO:118 */
#pragma unroll
          for (int j = 0; j < 4; j++) w[j] = __builtin_amdgcn_alignbit(w[j], w[j], 16);
        }
        float2 ph0 = ph_base;
        if (k > 0) ph0 = cmul_pinned_u(ph_base, k == 1 ? G.rotp1 : (k == 2 ? G.rotp2 : G.rotp3));
        bool blanked[4] = {false, false, false, false};
        /* the four phasors first, then the four products: independent chains the scheduler can
         * interleave (each complex product is a dependent pair of packed instructions).
         * NCO off: the record's rotations are (1, -0) and every product is exact, so the
         * multiplies stay unconditional (a select per sample cost more than they do). */
        float2 ph[4], x[4];
        ph[0] = ph0;
        ph[1] = cmul_pinned_u(ph0, G.rot1);
        ph[2] = cmul_pinned_u(ph0, G.rot2);
        ph[3] = cmul_pinned_u(ph0, G.rot3);
#pragma unroll
        for (int j = 0; j < 4; j++) {
          x[j] = unpack_iq(w[j], p.scale_i, p.scale_q);
          if (NB_ON) {
            const float pw = x[j].x * x[j].x + x[j].y * x[j].y;
            blanked[j] = nb_level > 0.f && pw > nb_t;
            x[j] = blanked[j] ? make_float2(0.f, 0.f) : x[j];
            nb_acc += blanked[j] ? 0.f : pw;
          }
        }
#pragma unroll
        for (int j = 0; j < 4; j++) x[j] = cmul_pinned(x[j], ph[j]);
#pragma unroll
        for (int j = 0; j < 4; j++) {
          if constexpr (DECIM == 4) {
            xs[xs_pos(4 * idx + j)] = x[j];
          } else {
            int m = 4 * idx + j; /* no decimator: the sample is the "output" */
            hb[(chunk % CPF) * CH_OUT + m] = x[j];
          }
        }
        if (NB_ON) { /* a blanked sample stays blanked when it becomes FIR history */
          raw[k].x = blanked[0] ? 0u : raw[k].x;
          raw[k].y = blanked[1] ? 0u : raw[k].y;
          raw[k].z = blanked[2] ? 0u : raw[k].z;
          raw[k].w = blanked[3] ? 0u : raw[k].w;
        }
      }
    }
    if (NB_ON) {
      float tot = wave_sum(nb_acc);
      if constexpr (NW > 1) {
        if (lane == 0) red[wave] = tot;
        wg_sync<NW>();
        tot = (red[0] + red[1]) + (red[2] + red[3]);
        wg_sync<NW>();
      }
      const float mean = tot / (float)CH_IN;
      nb_level = (nb_level > 0.f) ? nb_level + 0.2f * (mean - nb_level) : mean;
    }
    /* prefetch the next chunk's raw samples; they land during FIR + FFT */
    if (chunk + 1 < p.n_chunks) {
#pragma unroll
      for (int k = 0; k < LP; k++) {
        int idx = tid + NT * k;
        if (idx < CH_IN / 4)
          raw[k] = *reinterpret_cast<const uint4 *>(iq + (size_t)(chunk + 1) * CH_IN + 4 * idx);
      }
    }
    wg_sync<NW>();

    /* ---- A3: polyphase decimating FIR ------------------------------------ */
    if constexpr (DECIM == 4) {
      float2 acc[4];
#pragma unroll
      for (int r = 0; r < 4; r++) acc[r] = make_float2(0.f, 0.f);
      if constexpr (NW == 1) {
        /* when a tail-kernel wave shares the SIMD (pipelined mode), the FIR -- the
         * throughput-bound part -- takes issue priority; the rest of the chunk runs at
         * normal priority so the latency-bound tail keeps pace (measured balance) */
        if (p.front_prio == 1) __builtin_amdgcn_s_setprio(1);
        else if (p.front_prio == 2) __builtin_amdgcn_s_setprio(2);
        else if (p.front_prio == 3) __builtin_amdgcn_s_setprio(3);
        fir_lane<(P >= 8)>(lane, 0, 4, xs, taps_lds, acc);
        if (p.front_prio > 0) __builtin_amdgcn_s_setprio(0);
#pragma unroll
        for (int r = 0; r < 4; r++) hb[(chunk % CPF) * CH_OUT + 4 * lane + r] = acc[r];
        wg_sync<NW>();
      } else {
        /* four waves: wave w takes polyphase branch w; partials summed via LDS */
        fir_lane<(P >= 8)>(lane, wave, wave + 1, xs, taps_lds, acc);
#pragma unroll
        for (int r = 0; r < 4; r++) wb[wave * CH_OUT + 4 * lane + r] = acc[r];
        wg_sync<NW>();
        {
          float2 s0 = wb[tid], s1 = wb[CH_OUT + tid], s2 = wb[2 * CH_OUT + tid], s3 = wb[3 * CH_OUT + tid];
          float2 s = cadd(cadd(s0, s1), cadd(s2, s3));
          hb[(chunk % CPF) * CH_OUT + tid] = s;
        }
      }
      /* slide the FIR history: entries 64..80 of every plane -> 0..16 */
      {
        float4 *xs4 = reinterpret_cast<float4 *>(xs);
        for (int i = tid; i < 8 * 17; i += NT) {
          int sp = i / 17, e = i % 17;
          xs4[sp * RDSP_XP + e] = xs4[sp * RDSP_XP + 64 + e];
        }
      }
      wg_sync<NW>();
    }

    if ((chunk + 1) % CPF != 0) continue;

    /* ---- A5/A6: overlap-save frames ---------------------------------------- */
#pragma unroll 1
    for (int f = 0; f < FPC; f++) {
      const float2 *hnew = hb + f * H;
      front_frame<N, P, ALIAS>(p, G, tw, lb, wb, red, mreg, vadbits, vad_inv, vprev, nfloor, agc_g, am_dc, frame_idx,
                                ch, tid, [&](int i) { return hnew[i]; }); /* advances frame_idx */
    }
  }

  /* ---- state out --------------------------------------------------------- */
#pragma unroll
  for (int j = 0; j < PH; j++) p.st_prev[ch * H + tid + j * NT] = vprev[j];
  if constexpr (DECIM == 4) {
    /* the last 256 input samples as they entered the FIR (blanked ones as zero): the
     * registers of the last load pass still hold them, no prefetch followed */
    if constexpr (LP == 4) {
      *reinterpret_cast<uint4 *>(p.st_hist + ch * 256 + 4 * tid) = raw[LP - 1];
    } else {
      if (tid >= NT - 64) *reinterpret_cast<uint4 *>(p.st_hist + ch * 256 + 4 * (tid - (NT - 64))) = raw[0];
    }
  } else {
    /* no FIR history at decim 1, but the call's last raw word still has a reader: the I2S slip correction,
     * switched on between two calls, pairs the next call's first sample with it (rdsp_chain_process) */
    if (tid == 0) p.st_hist[ch * 256 + 255] = iq[(size_t)p.n_chunks * CH_IN - 1];
  }
  if (tid == 0) {
    p.st_scal[ch * 4 + 0] = nfloor;
    if (!p.to_mid) p.st_scal[ch * 4 + 1] = agc_g;
    p.st_scal[ch * 4 + 2] = am_dc;
    p.st_scal[ch * 4 + 3] = nb_level;
  }
}

template <int N, int P, int DECIM, bool LEAN, bool PRE>
int launch_direct(const RdspFrontParams *p, int n_channels, hipStream_t stream) {
  constexpr size_t lds = FrontLds<N, P, DECIM>::BYTES;
  int e = ensure_lds_limit<&rdsp_front_kernel<N, P, DECIM, LEAN, PRE>>(lds);
  if (e != 0) return e;
  hipLaunchKernelGGL((rdsp_front_kernel<N, P, DECIM, LEAN, PRE>), dim3(n_channels), dim3(N / P), lds, stream, *p);
  return (int)hipGetLastError();
}

/* the instances that exist: no full-register one at radix 16 */
template <int P, bool LEAN>
constexpr bool direct_instance = LEAN || P != 16;

template <int N, int P, int DECIM>
int launch_direct_flags(const RdspFrontPick &k, const RdspFrontParams *p, int n_channels, hipStream_t stream) {
  return with_flag(k.lean, [&](auto lean) {
    return with_flag(k.pre, [&](auto pre) {
      constexpr bool LEAN = decltype(lean)::value, PRE = decltype(pre)::value;
      if constexpr (direct_instance<P, LEAN>) return launch_direct<N, P, DECIM, LEAN, PRE>(p, n_channels, stream);
      else return (int)hipErrorInvalidValue;
    });
  });
}

}  // namespace

int rdsp::front_direct_launch(int fft_l, int decim, const RdspFrontPick &k, const RdspFrontParams *p, int n_channels,
                              hipStream_t stream) {
  return with_front_plan(fft_l, (int)hipErrorInvalidValue, [&](auto plan) {
    constexpr int N = decltype(plan)::N, P = decltype(plan)::P;
    return decim == 4 ? launch_direct_flags<N, P, 4>(k, p, n_channels, stream)
                      : launch_direct_flags<N, P, 1>(k, p, n_channels, stream);
  });
}

extern "C" size_t rdsp_front_lds_bytes(int fft_l, int decim) {
  return with_front_plan(fft_l, (size_t)0, [&](auto plan) {
    constexpr int N = decltype(plan)::N, P = decltype(plan)::P;
    return decim == 4 ? FrontLds<N, P, 4>::BYTES : FrontLds<N, P, 1>::BYTES;
  });
}
