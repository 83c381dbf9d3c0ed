/*
 * rdsp_engine_pocsag.hip -- rdsp_engine_t's POCSAG pager decoder (include/rdsp.h has the definition, rdsp_pocsag.h the
 * arithmetic): the kernel an NFM group with a paging baud rate launches behind its other detector kernels.  It reads the group's
 * demodulated rows once and writes five records a block and its own state words; the audio, the meter's records, the gates and
 * the active list are not touched.  Compiled with the engine's flags (-ffp-contract=off).
 *
 * rdsp_engine_pocsag_kernel has the AFSK kernel's shape without its table and its barrier: one wave per channel, four channels
 * a workgroup; a wave past the last channel leaves at once.  Eight blocks, 256 decimated samples, a trip: in pass k = 0 ... 3
 * lane l loads samples 4 l ... 4 l + 3 of block 2 k + (l >> 5) and adds them as dtmf_quad, so it holds decimated sample
 * 64 k + l of the trip.  It writes the sample into the wave's LDS row behind the 19 samples carried from the trip (or the call)
 * before, and reads its window of W = 20, 8 or 4 back (W is the launch's, one group's): the matched filter is parallel over
 * the samples and recomputed for every one of them.  A pass's 64 decisions raw[m] = S[m] < 0 are one ballot, a wave-uniform
 * 64-bit mask, and framing, correction and messages run on the masks in scalar registers, per RUN, not per sample: a run ends
 * at a transition or at a block's end; between the two the clock is linear, so the bits sampled in a run of n samples are a
 * 64-bit quotient (afsk_clock) and all have the run's value.  Each sampled bit goes through pocsag_bit, the same function the
 * plain loop calls.  The syndrome is integer division in scalar registers, the error pattern one look-up in a 1024-entry uint16
 * table in constant memory.  The open message's words live in LDS during a call; a closed message leaves for its ring slot as
 * vector stores by the whole wave.
 */
#include <hip/hip_runtime.h>

#include "rdsp_engine_pocsag.h"
#include "rdsp_wave.h"

using namespace rdsp_eng;
using namespace rdsp_pocsag;

namespace {
constexpr int PW = 256, PCH = PW / 64; /* four waves, four channels */
constexpr int PSTEP = 8;               /* blocks in flight per wave */
constexpr int TRIP = PSTEP * PER_BLOCK, PASSES = TRIP / 64;
constexpr int FIRST = MAX_WINDOW;      /* the trip's sample j lies at row[FIRST + j], the carried 19 at row[1 ... 19] */
constexpr int ROW = FIRST + TRIP;

__constant__ PocsagTable bch_table = pocsag_make_table();

__device__ __forceinline__ uint32_t uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
}  // namespace

__global__ __launch_bounds__(PW) void rdsp_engine_pocsag_kernel(const PocsagParams p) {
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6, half = lane >> 5, l32 = lane & 31;
  const int ch = (int)blockIdx.x * PCH + wave;
  __shared__ float rows[PCH][ROW];
  __shared__ uint32_t msgs[PCH][MSG_MAX];
  if (ch >= p.n_channels) return; /* no barrier in this kernel */
  float *row = rows[wave];
  uint32_t *msgw = msgs[wave];
  uint32_t *w = p.state + (size_t)ch * POCSAG_WORDS;
  const PocsagLaw law = p.law;
  /* the detector the call begins with (pocsag_start) */
  const bool fresh = p.reset != 0 || uniform(w[PG_BAUD]) != law.baud;
  PocsagBits s;
  s.pll = fresh ? 0u : uniform(w[PG_PLL]);
  s.prev_raw = fresh ? 0u : uniform(w[PG_PREV_RAW]);
  s.sr = fresh ? 0u : uniform(w[PG_SR]);
  s.insync = fresh ? 0u : uniform(w[PG_INSYNC]);
  s.pol = fresh ? 0u : uniform(w[PG_POL]);
  s.nbits = fresh ? 0u : uniform(w[PG_NBITS]);
  s.ncw = fresh ? 0u : uniform(w[PG_NCW]);
  s.open = fresh ? 0u : uniform(w[PG_OPEN]);
  s.m_ncw = fresh ? 0u : uniform(w[PG_M_NCW]);
  s.m_flags = fresh ? 0u : uniform(w[PG_M_FLAGS]);
  s.m_addr = fresh ? 0u : uniform(w[PG_M_ADDR]);
  s.m_counts = fresh ? 0u : uniform(w[PG_M_COUNTS]);
  s.n_msgs = fresh ? 0u : uniform(w[PG_NMSGS]);
  s.n_bad = fresh ? 0u : uniform(w[PG_NBAD]);
  s.t_blocks = fresh ? 0u : uniform(w[PG_TBLOCKS]);
  for (int k = lane; k < MSG_MAX; k += 64) msgw[k] = fresh ? 0u : w[PG_MSG + MSG_HEAD + k];
  if (fresh) { /* wave-uniform: the ring is zeros before this call's messages land in it */
    for (int k = lane; k < RING * SLOT_WORDS; k += 64) w[PG_RING + k] = 0u;
    __threadfence();
  }
  if (lane < HIST) row[1 + lane] = fresh ? 0.0f : __uint_as_float(w[PG_HIST + lane]);
  const float4 *audio = (const float4 *)(p.audio + (size_t)ch * p.audio_stride);
  uint8_t *sync_rec = p.sync + (size_t)ch * p.rec_stride, *new_rec = p.fresh + (size_t)ch * p.rec_stride, *bad_rec = p.bad + (size_t)ch * p.rec_stride;
  float *lvl_rec = p.lvl + (size_t)ch * p.rec_stride, *dc_rec = p.dc + (size_t)ch * p.rec_stride;
  float d[PASSES];
  int cnt = 0;
  for (int b0 = 0; b0 < p.n_blocks; b0 += PSTEP) {
    cnt = PER_BLOCK * min(PSTEP, p.n_blocks - b0); /* the trip's samples */
#pragma unroll
    for (int k = 0; k < PASSES; k++) {
      const int b = b0 + 2 * k + half;
      const float4 v = b < p.n_blocks ? audio[(size_t)b * (BLOCK / 4) + l32] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      d[k] = dtmf_quad(v.x, v.y, v.z, v.w);
      row[FIRST + 64 * k + lane] = d[k];
    }
    wg_sync<1>(); /* the wave's own row: its LDS operations execute in order */
    uint64_t mask[PASSES];
#pragma unroll
    for (int k = 0; k < PASSES; k++) {
      const float S = pocsag_window_sum(row + (FIRST + 64 * k + lane), law.window);
      mask[k] = __ballot(pocsag_raw(S));
      float t = row_allsum(fabsf(S)), u = row_allsum(d[k]); /* pocsag_tree32: float addition commutes */
      t += __shfl_xor(t, 16);
      u += __shfl_xor(u, 16);
      const int b = b0 + 2 * k + half;
      if (l32 == 0 && b < p.n_blocks) { lvl_rec[b] = t * law.lscale; dc_rec[b] = u * law.dscale; }
    }
    /* framing, correction and messages, wave-uniform */
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
          /* wave-uniform: every lane holds the same s, so the word pocsag_bit stores is the same value to the same LDS address
           * from all 64 lanes (no race) */
          const PocsagEvent ev = pocsag_bit(s, msgw, bch_table.e, raw, law);
          if (ev.closed) {
            uint32_t *slot = w + PG_RING + (s.n_msgs % RING) * SLOT_WORDS;
            wg_sync<1>(); /* the words are in LDS */
            for (int q = lane; q < SLOT_WORDS; q += 64) slot[q] = pocsag_ring_word(q, ev, s.t_blocks + 1u, q >= MSG_HEAD ? msgw[q - MSG_HEAD] : 0u);
            wg_sync<1>();
            s.n_msgs += 1u;
            n_new += 1u;
          }
          n_bad += ev.bad;
        }
        pos = next;
        if ((pos & (PER_BLOCK - 1)) == 0) { /* a block's end */
          s.t_blocks += 1u;
          if (lane == 2 * k + (pos >> 5) - 1) { rec_sync = s.insync; rec_new = n_new; rec_bad = min(n_bad, 255u); }
          n_new = 0u; n_bad = 0u;
        }
      }
      s.prev_raw = (uint32_t)(M >> (valid - 1)) & 1u;
    }
    if (lane < PSTEP && b0 + lane < p.n_blocks) {
      sync_rec[b0 + lane] = (uint8_t)rec_sync;
      new_rec[b0 + lane] = (uint8_t)rec_new;
      bad_rec[b0 + lane] = (uint8_t)rec_bad;
    }
    if (b0 + PSTEP < p.n_blocks) { /* the next trip's carried samples: this one was whole */
      wg_sync<1>();
      const float t = row[FIRST + TRIP - HIST + (lane < HIST ? lane : 0)];
      wg_sync<1>();
      if (lane < HIST) row[1 + lane] = t;
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
  if (lane < MAX_WINDOW) w[PG_HIST + lane] = lane < HIST ? __float_as_uint(h) : 0u;
  wg_sync<1>();
  if (lane < MSG_HEAD) w[PG_MSG + lane] = 0u;
  for (int k = lane; k < MSG_MAX; k += 64) w[PG_MSG + MSG_HEAD + k] = msgw[k];
  if (lane == 0) {
    w[PG_BAUD] = law.baud; w[PG_PLL] = s.pll; w[PG_PREV_RAW] = s.prev_raw; w[PG_SR] = s.sr; w[PG_INSYNC] = s.insync; w[PG_POL] = s.pol;
    w[PG_NBITS] = s.nbits; w[PG_NCW] = s.ncw; w[PG_OPEN] = s.open; w[PG_M_NCW] = s.m_ncw; w[PG_M_FLAGS] = s.m_flags; w[PG_M_ADDR] = s.m_addr;
    w[PG_M_COUNTS] = s.m_counts; w[PG_NMSGS] = s.n_msgs; w[PG_NBAD] = s.n_bad; w[PG_TBLOCKS] = s.t_blocks;
  }
}

hipError_t rdsp_engine_pocsag_launch(const PocsagParams &p, hipStream_t s) {
  if (p.n_channels < 1 || p.n_blocks < 1) return hipSuccess;
  hipLaunchKernelGGL(rdsp_engine_pocsag_kernel, dim3((unsigned)((p.n_channels + PCH - 1) / PCH)), dim3(PW), 0, s, p);
  return hipGetLastError();
}
