/*
 * rdsp_engine_afsk.hip -- rdsp_engine_t's AFSK 1200 packet decoder (include/rdsp.h has the definition, rdsp_afsk.h the
 * arithmetic): the kernel an NFM group with the decoder on launches behind its other detector kernels.  It reads the group's
 * demodulated rows once and writes four records a block and its own state words; the audio, the meter's records, the gates and
 * the active list are not touched.  Compiled with the engine's flags (-ffp-contract=off).
 *
 * rdsp_engine_afsk_kernel has the DTMF kernel's shape: one wave per channel, four channels a workgroup, the phasor table a
 * 16 KiB LDS copy behind the only barrier; a wave past the last channel leaves behind it.  Eight blocks, 256 decimated samples,
 * a trip: in pass k = 0 ... 3 lane l loads samples 4 l ... 4 l + 3 of block 2 k + (l >> 5) and adds them as dtmf_quad, so it
 * holds decimated sample 64 k + l of the trip.  It writes that sample's four products (mark and space, cos and sin) as one
 * float4 into the wave's LDS row behind the products of the 11 samples carried from the trip (or the call) before, and reads its
 * window of 12 back: stages 1 and 2 are parallel over the samples.  A pass's 64 decisions raw[m] are one ballot, a wave-uniform
 * 64-bit mask, and stages 3 to 5 run on the masks in scalar registers, per RUN, not per sample: a run ends at a transition or
 * at a block's end; between the two the clock is linear, so the bits sampled in a run of n samples are a 64-bit quotient
 * (afsk_clock), the first of them is the NRZI bit raw == prev_sampled and the others are ones.  Each sampled bit goes through
 * afsk_hdlc, the same function the plain loop calls; a run of ones that has saturated `ones` is cut short, since the machine
 * does not move any more.  The frame's bytes live in LDS during a call; a frame whose FCS holds leaves for its ring slot as
 * vector stores by the whole wave.
 */
#include <hip/hip_runtime.h>

#include "rdsp_engine_afsk.h"
#include "rdsp_wave.h"

using namespace rdsp_eng;
using namespace rdsp_afsk;

namespace {
constexpr int AW = 256, ACH = AW / 64; /* four waves, four channels */
constexpr int ASTEP = 8;               /* blocks in flight per wave */
constexpr int TRIP = ASTEP * PER_BLOCK, PASSES = TRIP / 64;
constexpr int FIRST = WINDOW;          /* the trip's sample j lies at row[FIRST + j], the carried 11 at row[1 ... 11] */
constexpr int ROW = FIRST + TRIP;

__device__ __forceinline__ uint32_t uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
}  // namespace

__global__ __launch_bounds__(AW) void rdsp_engine_afsk_kernel(const AfskParams p) {
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6, half = lane >> 5, l32 = lane & 31;
  const int ch = (int)blockIdx.x * ACH + wave;
  __shared__ float4 tab[rdsp_tune::TUNE_N];
  __shared__ float4 rows[ACH][ROW];
  __shared__ uint32_t bufs[ACH][BUF_WORDS];
  for (int i = (int)threadIdx.x; i < rdsp_tune::TUNE_N; i += AW) tab[i] = p.tab[i];
  __syncthreads(); /* the only barrier: every wave of the workgroup filled its quarter */
  if (ch >= p.n_channels) return;
  float4 *row = rows[wave];
  uint32_t *bufw = bufs[wave];
  uint8_t *buf = (uint8_t *)bufw;
  uint32_t *w = p.state + (size_t)ch * AFSK_WORDS;
  const AfskLaw law = p.law;
  /* the detector the call begins with (afsk_start) */
  const bool fresh = p.reset != 0 || uniform(w[AF_ON]) != 1u;
  AfskBits s;
  s.pll = fresh ? 0u : uniform(w[AF_PLL]);
  s.prev_raw = fresh ? 0u : uniform(w[AF_PREV_RAW]);
  s.prev_sampled = fresh ? 0u : uniform(w[AF_PREV_SAMPLED]);
  s.ones = fresh ? 0u : uniform(w[AF_ONES]);
  s.inframe = fresh ? 0u : uniform(w[AF_INFRAME]);
  s.byte = fresh ? 0u : uniform(w[AF_BYTE]);
  s.nb = fresh ? 0u : uniform(w[AF_NB]);
  s.nbytes = fresh ? 0u : uniform(w[AF_NBYTES]);
  s.crc = fresh ? 0u : uniform(w[AF_CRC]);
  s.n_frames = fresh ? 0u : uniform(w[AF_NFRAMES]);
  s.n_bad = fresh ? 0u : uniform(w[AF_NBAD]);
  s.t_blocks = fresh ? 0u : uniform(w[AF_TBLOCKS]);
  for (int k = lane; k < BUF_WORDS; k += 64) bufw[k] = fresh ? 0u : w[AF_BUF + k];
  if (fresh) { /* wave-uniform: the ring is zeros before this call's frames land in it */
    for (int k = lane; k < RING * SLOT_WORDS; k += 64) w[AF_RING + k] = 0u;
    __threadfence();
  }
  uint32_t m0 = (uint32_t)PER_BLOCK * s.t_blocks;
  if (lane < HIST) row[1 + lane] = afsk_products(tab, law, m0 - (uint32_t)(HIST - lane), fresh ? 0.0f : __uint_as_float(w[AF_HIST + lane]));
  const float4 *audio = (const float4 *)(p.audio + (size_t)ch * p.audio_stride);
  uint8_t *sync_rec = p.sync + (size_t)ch * p.rec_stride, *new_rec = p.fresh + (size_t)ch * p.rec_stride, *bad_rec = p.bad + (size_t)ch * p.rec_stride;
  float *lvl_rec = p.lvl + (size_t)ch * p.rec_stride;
  float d[PASSES];
  int cnt = 0;
  for (int b0 = 0; b0 < p.n_blocks; b0 += ASTEP) {
    cnt = PER_BLOCK * min(ASTEP, p.n_blocks - b0); /* the trip's samples */
#pragma unroll
    for (int k = 0; k < PASSES; k++) {
      const int b = b0 + 2 * k + half;
      const float4 v = b < p.n_blocks ? audio[(size_t)b * (BLOCK / 4) + l32] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      d[k] = dtmf_quad(v.x, v.y, v.z, v.w);
      row[FIRST + 64 * k + lane] = afsk_products(tab, law, m0 + (uint32_t)(64 * k + lane), d[k]);
    }
    wg_sync<1>(); /* the wave's own row: its LDS operations execute in order */
    uint64_t mask[PASSES];
#pragma unroll
    for (int k = 0; k < PASSES; k++) {
      const float2 P = afsk_powers(row + (FIRST - HIST + 64 * k + lane), law.g);
      mask[k] = __ballot(afsk_raw(P));
      float t = row_allsum(afsk_level(P)); /* afsk_tree32: float addition commutes */
      t += __shfl_xor(t, 16);
      const int b = b0 + 2 * k + half;
      if (l32 == 0 && b < p.n_blocks) lvl_rec[b] = t * law.lscale;
    }
    /* stages 3 to 5, wave-uniform */
    uint32_t rec_sync = 0u, rec_new = 0u, rec_bad = 0u, n_new = 0u, n_bad = 0u;
    for (int k = 0; k < PASSES; k++) {
      const int valid = min(64, cnt - 64 * k);
      if (valid <= 0) break;
      const uint64_t M = mask[k];
      const uint64_t T = M ^ (M << 1 | (uint64_t)s.prev_raw);     /* sample pos differs from the one before it */
      const uint64_t starts = T | 1ull | 1ull << PER_BLOCK;       /* a run starts at a transition and at a block's first sample */
      int pos = 0;
      while (pos < valid) {
        const uint32_t raw = (uint32_t)(M >> pos) & 1u;
        if ((T >> pos) & 1ull) s.pll = afsk_pulled(s.pll, law.pull);
        const uint64_t above = pos < 63 ? (starts >> (pos + 1)) << (pos + 1) : 0ull;
        const int next = min(above ? (int)__builtin_ctzll(above) : 64, valid);
        const uint32_t c = afsk_clock(s.pll, law.step, (uint32_t)(next - pos));
        for (uint32_t i = 0; i < c; i++) {
          const uint32_t bit = raw == s.prev_sampled ? 1u : 0u;
          s.prev_sampled = raw;
          if (bit && s.ones >= 7u && !s.inframe) break; /* the run's other bits are ones too: the machine stays where it is */
          /* wave-uniform: every lane holds the same s, so the byte afsk_hdlc stores is the same value to the same LDS address
           * from all 64 lanes (no race), and the CRC's eight steps are scalar work */
          const uint32_t ev = afsk_hdlc(s, buf, bit, law.min_bytes);
          if ((ev & 3u) == AFSK_EV_FRAME) {
            const uint32_t len = (ev >> 2) - 2u;
            uint32_t *slot = w + AF_RING + (s.n_frames % RING) * SLOT_WORDS;
            wg_sync<1>(); /* the bytes are in LDS */
            for (int q = lane; q < SLOT_WORDS; q += 64) slot[q] = afsk_ring_word(q, len, s.t_blocks + 1u, q >= 2 ? bufw[q - 2] : 0u);
            wg_sync<1>();
            s.n_frames += 1u;
            n_new += 1u;
          } else if ((ev & 3u) == AFSK_EV_BAD) {
            n_bad += 1u;
          }
        }
        pos = next;
        if ((pos & (PER_BLOCK - 1)) == 0) { /* a block's end */
          s.t_blocks += 1u;
          if (lane == 2 * k + (pos >> 5) - 1) { rec_sync = s.inframe; rec_new = n_new; rec_bad = n_bad; }
          n_new = 0u; n_bad = 0u;
        }
      }
      s.prev_raw = (uint32_t)(M >> (valid - 1)) & 1u;
    }
    if (lane < ASTEP && b0 + lane < p.n_blocks) {
      sync_rec[b0 + lane] = (uint8_t)rec_sync;
      new_rec[b0 + lane] = (uint8_t)rec_new;
      bad_rec[b0 + lane] = (uint8_t)rec_bad;
    }
    if (b0 + ASTEP < p.n_blocks) { /* the next trip's carried products: this one was whole */
      wg_sync<1>();
      const float4 t = row[FIRST + TRIP - HIST + (lane < HIST ? lane : 0)];
      wg_sync<1>();
      if (lane < HIST) row[1 + lane] = t;
      m0 += (uint32_t)TRIP;
    }
  }
  /* the words; the ring's are in place */
  const int j = cnt - HIST + (lane < HIST ? lane : 0); /* cnt >= 32 */
  float h = 0.0f;
#pragma unroll
  for (int k = 0; k < PASSES; k++) {
    const float t = __shfl(d[k], j & 63);
    h = (j >> 6) == k ? t : h;
  }
  if (lane < WINDOW) w[AF_HIST + lane] = lane < HIST ? __float_as_uint(h) : 0u;
  wg_sync<1>();
  for (int k = lane; k < BUF_WORDS; k += 64) w[AF_BUF + k] = bufw[k];
  if (lane == 0) {
    w[AF_ON] = 1u; w[AF_PLL] = s.pll; w[AF_PREV_RAW] = s.prev_raw; w[AF_PREV_SAMPLED] = s.prev_sampled; w[AF_ONES] = s.ones; w[AF_INFRAME] = s.inframe;
    w[AF_BYTE] = s.byte; w[AF_NB] = s.nb; w[AF_NBYTES] = s.nbytes; w[AF_CRC] = s.crc; w[AF_NFRAMES] = s.n_frames; w[AF_NBAD] = s.n_bad;
    w[AF_TBLOCKS] = s.t_blocks;
#pragma unroll
    for (int k = AF_TBLOCKS + 1; k < AF_HIST; k++) w[k] = 0u;
  }
}

hipError_t rdsp_engine_afsk_launch(const AfskParams &p, hipStream_t s) {
  if (p.n_channels < 1 || p.n_blocks < 1) return hipSuccess;
  hipLaunchKernelGGL(rdsp_engine_afsk_kernel, dim3((unsigned)((p.n_channels + ACH - 1) / ACH)), dim3(AW), 0, s, p);
  return hipGetLastError();
}
