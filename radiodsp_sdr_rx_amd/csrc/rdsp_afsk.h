/*
 * rdsp_afsk.h -- the arithmetic of rdsp_engine_t's AFSK 1200 (Bell 202, AX.25) packet decoder (include/rdsp.h has the
 * definition), shared by the kernel (rdsp_engine_afsk.hip), the host entry points (rdsp_engine_afsk_host.hip) and the host
 * program of the tests (tests/host/host_afsk_check.cpp).  Compile with -ffp-contract=off: every product and sum below is rounded
 * on its own, the fused operations are written as fmaf.
 *
 * Per channel, a[n] the receiver's "demod" tap (rdsp_fm.h's y[n]), blocks of 128 samples counted from the detector's start:
 *   d[m] = dtmf_quad(a[4 m ... 4 m + 3]), m = 32 t_blocks + r (uint32), 11 025 Hz, 9.1875 samples a bit; 0 before the start
 *   p_f[m] = (d c, d s), (c, s) = tune_phasor(tab, m dphi_f), f = 1200 (mark), 2200 (space)
 *   S_f[m] = the sum of p_f[m - 11 ... m] per component as (q0 + q1) + q2, q_i = dtmf_quad of terms 4 i ... 4 i + 3
 *   P_f = fmaf(S.x, S.x, S.y S.y); gp = g P_space; raw[m] = P_mark - gp > 0; lvl = tree32(P_mark + gp) lscale a block
 *   the bit clock (afsk_clock), the HDLC machine (afsk_hdlc) and the frame ring (afsk_ring_word) are integers only.
 * A channel's state is AFSK_WORDS = 448 words: on, pll, prev_raw, prev_sampled, ones, inframe, byte, nb, nbytes, crc, n_frames,
 * n_bad, t_blocks, three zeros; hist[11] (d[m - 11 ... m - 1] of the next m) and a zero; buf (330 bytes and the byte behind them,
 * padded to 84 words); ring[4][84] (len, t_blocks, 82 words of bytes).  A detector whose stored `on` is not the one it is run
 * with starts from zeros (afsk_start).
 */
#ifndef RDSP_AFSK_H
#define RDSP_AFSK_H

#include <math.h>
#include <stdint.h>
#include <string.h>

#include "rdsp_dtmf.h"
#include "rdsp_tune.h"

namespace rdsp_afsk {

using rdsp_dtmf::dtmf_quad;

constexpr int BLOCK = 128, DEC = 4, PER_BLOCK = BLOCK / DEC; /* 32 decimated samples a block */
constexpr int WINDOW = 12, HIST = WINDOW - 1;
constexpr int AFSK_MAX_BYTES = 330, AFSK_MIN_BYTES = 9, BUF_WORDS = 84, RING = 4, SLOT_WORDS = 84, SLOT_DATA = 82;
enum { AF_ON = 0, AF_PLL, AF_PREV_RAW, AF_PREV_SAMPLED, AF_ONES, AF_INFRAME, AF_BYTE, AF_NB, AF_NBYTES, AF_CRC, AF_NFRAMES, AF_NBAD, AF_TBLOCKS,
       AF_HIST = 16, AF_BUF = AF_HIST + WINDOW, AF_RING = AF_BUF + BUF_WORDS, AFSK_WORDS = AF_RING + RING * SLOT_WORDS };
static_assert(AFSK_WORDS == 448, "the state layout of include/rdsp.h");
constexpr float AFSK_MARK_HZ = 1200.0f, AFSK_SPACE_HZ = 2200.0f, AFSK_BAUD = 1200.0f;
constexpr float AFSK_DEFAULT_GAIN = 1.0f, AFSK_MIN_GAIN = 0.0625f, AFSK_MAX_GAIN = 16.0f;
constexpr int AFSK_DEFAULT_PULL = 2, AFSK_DEFAULT_MIN_BYTES = 17;
constexpr uint32_t AFSK_CRC_INIT = 0xFFFFu, AFSK_CRC_POLY = 0x8408u, AFSK_CRC_RESIDUE = 0xF0B8u;
enum { AFSK_EV_NONE = 0, AFSK_EV_FRAME = 1, AFSK_EV_BAD = 2 };

/* a group's settings (rdsp_engine_set_afsk) */
struct AfskSet {
  int on;
  float space_gain;
  int pull, min_bytes;
};
/* what the kernel is handed of them */
struct AfskLaw {
  uint32_t pull, min_bytes, step, dphi_mark, dphi_space;
  float g, lscale;
};

/* the setter's limits (a NaN fails every comparison) */
inline bool afsk_ok(int on, float space_gain, int pull, int min_bytes) {
  return (on == 0 || on == 1) && space_gain >= AFSK_MIN_GAIN && space_gain <= AFSK_MAX_GAIN && pull >= 1 && pull <= 4 && min_bytes >= AFSK_MIN_BYTES &&
         min_bytes <= AFSK_MAX_BYTES;
}
/* host only, libm-free but for the rounding: the step per DECIMATED sample */
inline uint32_t afsk_dphi(float hz) { return (uint32_t)(unsigned long long)llround((double)hz * 4294967296.0 * (double)DEC / rdsp_tune::TUNE_FS); }
inline float afsk_lscale() { return (float)(1.0 / (32.0 * 24.0 * 24.0)); }
inline AfskLaw afsk_law(const AfskSet &s) {
  AfskLaw l;
  l.pull = (uint32_t)s.pull; l.min_bytes = (uint32_t)s.min_bytes;
  l.step = afsk_dphi(AFSK_BAUD); l.dphi_mark = afsk_dphi(AFSK_MARK_HZ); l.dphi_space = afsk_dphi(AFSK_SPACE_HZ);
  l.g = s.space_gain; l.lscale = afsk_lscale();
  return l;
}

/* ---- the frame check sequence: CRC-16/X-25, reflected ---- */
RDSP_HD uint32_t afsk_crc_byte(uint32_t crc, uint32_t byte) {
  crc ^= byte & 0xFFu;
  for (int k = 0; k < 8; k++) crc = (crc >> 1) ^ ((crc & 1u) ? AFSK_CRC_POLY : 0u);
  return crc;
}
inline uint32_t afsk_fcs(const uint8_t *bytes, size_t n) {
  uint32_t crc = AFSK_CRC_INIT;
  for (size_t k = 0; k < n; k++) crc = afsk_crc_byte(crc, bytes[k]);
  return crc ^ 0xFFFFu;
}

/* ---- stage 2: one decimated sample's two products and one window ---- */
RDSP_HD float4 afsk_products(const float4 *tab, const AfskLaw &law, uint32_t m, float d) {
  const float2 a = rdsp_tune::tune_phasor(tab, m * law.dphi_mark), b = rdsp_tune::tune_phasor(tab, m * law.dphi_space);
  return make_float4(d * a.x, d * a.y, d * b.x, d * b.y);
}
RDSP_HD float afsk_sum12(float t0, float t1, float t2, float t3, float t4, float t5, float t6, float t7, float t8, float t9, float t10, float t11) {
  return (dtmf_quad(t0, t1, t2, t3) + dtmf_quad(t4, t5, t6, t7)) + dtmf_quad(t8, t9, t10, t11);
}
/* p: the window's products, oldest first, WINDOW of them `stride` apart -> P_mark, g P_space */
template <typename P>
RDSP_HD float2 afsk_powers(P p, float g) {
  const float mx = afsk_sum12(p[0].x, p[1].x, p[2].x, p[3].x, p[4].x, p[5].x, p[6].x, p[7].x, p[8].x, p[9].x, p[10].x, p[11].x);
  const float my = afsk_sum12(p[0].y, p[1].y, p[2].y, p[3].y, p[4].y, p[5].y, p[6].y, p[7].y, p[8].y, p[9].y, p[10].y, p[11].y);
  const float sx = afsk_sum12(p[0].z, p[1].z, p[2].z, p[3].z, p[4].z, p[5].z, p[6].z, p[7].z, p[8].z, p[9].z, p[10].z, p[11].z);
  const float sy = afsk_sum12(p[0].w, p[1].w, p[2].w, p[3].w, p[4].w, p[5].w, p[6].w, p[7].w, p[8].w, p[9].w, p[10].w, p[11].w);
  return make_float2(fmaf(mx, mx, my * my), g * fmaf(sx, sx, sy * sy));
}
RDSP_HD bool afsk_raw(float2 P) { return P.x - P.y > 0.0f; }
RDSP_HD float afsk_level(float2 P) { return P.x + P.y; }

/* ---- stages 3 and 4: the integers ---- */
struct AfskBits {
  uint32_t pll, prev_raw, prev_sampled, ones, inframe, byte, nb, nbytes, crc, n_frames, n_bad, t_blocks;
};
/* (a) of the bit clock: a transition pulls the clock towards 0 */
RDSP_HD uint32_t afsk_pulled(uint32_t pll, uint32_t pull) { return (uint32_t)((int32_t)pll - ((int32_t)pll >> pull)); }
/* (b) over a run of n >= 0 samples without a transition: the bits sampled in it.  A bit is sampled when the clock goes from
 * [0, 2^31) to [2^31, 2^32), which is a carry out of the clock with its top bit flipped (step < 2^31), so n steps carry
 * (u + n step) >> 32 times */
RDSP_HD uint32_t afsk_clock(uint32_t &pll, uint32_t step, uint32_t n) {
  const uint64_t t = (uint64_t)(pll ^ 0x80000000u) + (uint64_t)n * (uint64_t)step;
  pll = (uint32_t)t ^ 0x80000000u;
  return (uint32_t)(t >> 32);
}
/* one sampled bit into the HDLC machine; buf: the frame's bytes (AFSK_MAX_BYTES + 1 of them).  Returns ev | nbytes << 2 of a
 * frame a flag closed (AFSK_EV_FRAME: the FCS holds, the caller puts buf[0 ... nbytes - 3] into the ring; AFSK_EV_BAD: it does
 * not, n_bad is counted here), else 0 */
template <typename B>
RDSP_HD uint32_t afsk_hdlc(AfskBits &s, B buf, uint32_t bit, uint32_t min_bytes) {
  uint32_t ev = AFSK_EV_NONE;
  if (bit) {
    s.ones = s.ones < 7u ? s.ones + 1u : 7u;
    if (s.ones >= 7u) s.inframe = 0u;
    else if (s.inframe) { s.byte |= 1u << s.nb; s.nb += 1u; }
  } else {
    if (s.ones == 6u) {
      if (s.inframe && s.nb == 7u && s.nbytes >= min_bytes) {
        ev = (s.crc == AFSK_CRC_RESIDUE ? (uint32_t)AFSK_EV_FRAME : (uint32_t)AFSK_EV_BAD) | s.nbytes << 2;
        if (s.crc != AFSK_CRC_RESIDUE) s.n_bad += 1u;
      }
      s.inframe = 1u; s.nbytes = 0u; s.byte = 0u; s.nb = 0u; s.crc = AFSK_CRC_INIT;
    } else if (s.ones != 5u && s.inframe) {
      s.nb += 1u;
    }
    s.ones = 0u;
  }
  if (s.inframe && s.nb == 8u) {
    buf[s.nbytes] = (uint8_t)s.byte;
    s.nbytes += 1u;
    s.crc = afsk_crc_byte(s.crc, s.byte);
    s.byte = 0u; s.nb = 0u;
    if (s.nbytes > (uint32_t)AFSK_MAX_BYTES) s.inframe = 0u;
  }
  return ev;
}
/* word k = 0 ... 83 of a ring slot: len, t_blocks, the len bytes (bufw: buf as little-endian words), zeros */
RDSP_HD uint32_t afsk_ring_word(int k, uint32_t len, uint32_t t_blocks, uint32_t bufw) {
  if (k == 0) return len;
  if (k == 1) return t_blocks;
  const uint32_t at = 4u * (uint32_t)(k - 2);
  if (at >= len) return 0u;
  return len - at >= 4u ? bufw : bufw & ((1u << (8u * (len - at))) - 1u);
}
/* the pairwise tree over a block's 32 values */
inline float afsk_tree32(const float *v) {
  float t[PER_BLOCK];
  memcpy(t, v, sizeof t);
  for (int n = PER_BLOCK; n > 1; n /= 2)
    for (int k = 0; k < n / 2; k++) t[k] = t[2 * k] + t[2 * k + 1];
  return t[0];
}

/* a channel's detector on the host: its 448 words */
struct AfskState {
  uint32_t on;
  AfskBits s;
  float hist[WINDOW]; /* hist[11] stays 0 */
  uint8_t buf[BUF_WORDS * 4];
  uint32_t ring[RING][SLOT_WORDS];
};
inline void afsk_load(AfskState &q, const uint32_t *w) {
  q.on = w[AF_ON];
  q.s = {w[AF_PLL], w[AF_PREV_RAW], w[AF_PREV_SAMPLED], w[AF_ONES], w[AF_INFRAME], w[AF_BYTE], w[AF_NB], w[AF_NBYTES], w[AF_CRC], w[AF_NFRAMES], w[AF_NBAD],
         w[AF_TBLOCKS]};
  memcpy(q.hist, &w[AF_HIST], sizeof q.hist);
  for (int k = 0; k < BUF_WORDS * 4; k++) q.buf[k] = (uint8_t)(w[AF_BUF + k / 4] >> (8 * (k % 4)));
  memcpy(q.ring, &w[AF_RING], sizeof q.ring);
}
inline void afsk_store(const AfskState &q, uint32_t *w) {
  memset(w, 0, AFSK_WORDS * 4);
  w[AF_ON] = q.on; w[AF_PLL] = q.s.pll; w[AF_PREV_RAW] = q.s.prev_raw; w[AF_PREV_SAMPLED] = q.s.prev_sampled; w[AF_ONES] = q.s.ones;
  w[AF_INFRAME] = q.s.inframe; w[AF_BYTE] = q.s.byte; w[AF_NB] = q.s.nb; w[AF_NBYTES] = q.s.nbytes; w[AF_CRC] = q.s.crc; w[AF_NFRAMES] = q.s.n_frames;
  w[AF_NBAD] = q.s.n_bad; w[AF_TBLOCKS] = q.s.t_blocks;
  memcpy(&w[AF_HIST], q.hist, sizeof q.hist);
  for (int k = 0; k < BUF_WORDS * 4; k++) w[AF_BUF + k / 4] |= (uint32_t)q.buf[k] << (8 * (k % 4));
  memcpy(&w[AF_RING], q.ring, sizeof q.ring);
}
/* the detector a call begins with: zeros behind a reset or another `on` */
inline void afsk_start(AfskState &q, uint32_t on, bool reset) {
  if (reset || q.on != on) memset(&q, 0, sizeof q);
  q.on = on;
}
/* the plain loop, which is the definition: n_blocks blocks of a behind the channel's words -> the records of the call, the
 * words renewed */
inline void afsk_reference(const float4 *tab, const AfskLaw &law, bool reset, uint32_t *words /* [AFSK_WORDS] */, const float *a, int n_blocks,
                           uint8_t *sync_rec, uint8_t *new_rec, uint8_t *bad_rec, float *lvl_rec) {
  AfskState q;
  afsk_load(q, words);
  afsk_start(q, 1u, reset);
  AfskBits &s = q.s;
  for (int b = 0; b < n_blocks; b++) {
    const float *x = a + (size_t)b * BLOCK;
    float lvl[PER_BLOCK];
    uint32_t fresh = 0u, bad = 0u;
    for (int r = 0; r < PER_BLOCK; r++) {
      const uint32_t m = (uint32_t)PER_BLOCK * s.t_blocks + (uint32_t)r;
      float4 p[WINDOW];
      for (int k = 0; k < HIST; k++) p[k] = afsk_products(tab, law, m - (uint32_t)(HIST - k), q.hist[k]);
      const float d = dtmf_quad(x[4 * r], x[4 * r + 1], x[4 * r + 2], x[4 * r + 3]);
      p[HIST] = afsk_products(tab, law, m, d);
      memmove(q.hist, q.hist + 1, (HIST - 1) * sizeof(float));
      q.hist[HIST - 1] = d;
      const float2 P = afsk_powers(p, law.g);
      lvl[r] = afsk_level(P);
      const uint32_t raw = afsk_raw(P) ? 1u : 0u;
      if (raw != s.prev_raw) { s.pll = afsk_pulled(s.pll, law.pull); s.prev_raw = raw; }
      const uint32_t old = s.pll;
      s.pll += law.step;
      if ((int32_t)old >= 0 && (int32_t)s.pll < 0) {
        const uint32_t bit = raw == s.prev_sampled ? 1u : 0u;
        s.prev_sampled = raw;
        const uint32_t ev = afsk_hdlc(s, q.buf, bit, law.min_bytes);
        if ((ev & 3u) == AFSK_EV_FRAME) {
          const uint32_t len = (ev >> 2) - 2u;
          uint32_t *slot = q.ring[s.n_frames % RING];
          for (int k = 0; k < SLOT_WORDS; k++) {
            uint32_t bw = 0u;
            if (k >= 2) memcpy(&bw, q.buf + 4 * (k - 2), 4); /* little-endian hosts, as the device */
            slot[k] = afsk_ring_word(k, len, s.t_blocks + 1u, bw);
          }
          s.n_frames += 1u;
          fresh += 1u;
        } else if ((ev & 3u) == AFSK_EV_BAD) {
          bad += 1u;
        }
      }
    }
    s.t_blocks += 1u;
    sync_rec[b] = (uint8_t)s.inframe;
    new_rec[b] = (uint8_t)fresh;
    bad_rec[b] = (uint8_t)bad;
    lvl_rec[b] = afsk_tree32(lvl) * law.lscale;
  }
  afsk_store(q, words);
}

}  // namespace rdsp_afsk

#endif
