/*
 * rdsp_chain_state.hip -- rdsp_chain_t's per-channel state as data: the table of state planes (rdsp_chain_int.h) with what
 * allocates and boots them, the state blob (save, load, bytes), and the read-backs.
 */
#include "rdsp_chain_int.h"

/* ---- the state planes ------------------------------------------------------------------------------------------------ */
template <typename T>
static void **slot_of(DevBuf<T> &b) { return (void **)&b.p; }

std::array<StatePlane, 16> chain_planes(rdsp_chain_t *c) {
  const size_t slip_row = (size_t)c->slip_phase; /* the carry the next call reads */
  return {{
      {slot_of(c->d_hist), 0, 1, sizeof(uint32_t) * 256, BOOT_ZERO, INST_NONE, OPT_NONE},
      {slot_of(c->d_prev), 0, 1, sizeof(float2) * (size_t)(c->N / 2), BOOT_ZERO, INST_NONE, OPT_NONE},
      {slot_of(c->d_scal), 0, 1, sizeof(float) * 4, BOOT_GAIN_ONE, INST_NONE, OPT_NONE},
      {slot_of(c->d_nr_w), 0, 1, sizeof(float) * RDSP_LMS_TAPS, BOOT_ZERO, INST_NR, OPT_NONE},
      {slot_of(c->d_nr_prev), 0, 1, sizeof(float) * RDSP_BLOCK, BOOT_ZERO, INST_NR, OPT_NONE},
      {slot_of(c->d_nr_energy), 0, 1, sizeof(float), BOOT_ZERO, INST_NR, OPT_NONE},
      {slot_of(c->d_als_w), 0, 1, sizeof(float) * RDSP_LMS_TAPS, BOOT_ZERO, INST_ALS, OPT_NONE},
      {slot_of(c->d_als_prev), 0, 1, sizeof(float) * RDSP_BLOCK, BOOT_ZERO, INST_ALS, OPT_NONE},
      {slot_of(c->d_als_energy), 0, 1, sizeof(float), BOOT_ZERO, INST_ALS, OPT_NONE},
      {slot_of(c->d_status), 0, 2, sizeof(uint32_t), BOOT_ZERO, INST_NR, OPT_NONE}, /* health words: DSP-NR, ALS */
      {slot_of(c->d_status), 1, 0, sizeof(uint32_t), BOOT_ZERO, INST_ALS, OPT_NONE},
      {slot_of(c->d_sam), 0, 1, sizeof(float) * 4, BOOT_ZERO, INST_NONE, OPT_SAM},
      {slot_of(c->d_iir_state), 0, 1, sizeof(float) * 16, BOOT_ZERO, INST_NONE, OPT_IIR},
      {slot_of(c->d_slip_carry), slip_row, 2, sizeof(uint32_t), BOOT_ZERO, INST_NONE, OPT_SLIP},
      {slot_of(c->d_eng_st), 0, 1, sizeof(float) * RDSP_ENG_ST_WORDS, BOOT_ENGINE_AGC, INST_NONE, OPT_ENG_TAIL},
      {slot_of(c->d_eng_als), 0, 1, sizeof(float) * RDSP_ENG_ALS_WORDS, BOOT_ZERO, INST_NONE, OPT_ENG_TAIL},
  }};
}

int chain_gain_one(rdsp_chain_t *c, int first, int n, bool keep_rest) {
  std::vector<float> sc(4 * (size_t)n, 0.0f);
  float *dev = c->d_scal + 4 * (size_t)first;
  if (keep_rest) HIP_TRY(hipMemcpy(sc.data(), dev, sc.size() * sizeof(float), hipMemcpyDeviceToHost));
  for (int i = 0; i < n; i++) sc[4 * (size_t)i + 1] = 1.0f; /* AGC gain starts at 1 */
  HIP_TRY(hipMemcpy(dev, sc.data(), sc.size() * sizeof(float), hipMemcpyHostToDevice));
  return RDSP_OK;
}

int chain_plane_boot(rdsp_chain_t *c, const StatePlane &pl, int first, int n) {
  if (pl.boot == BOOT_GAIN_ONE) return chain_gain_one(c, first, n, false);
  if (pl.boot == BOOT_ENGINE_AGC) {
    /* envelope, gain and hang counter 0, the active flag 1 (the constructor's values, until the AGC first runs).
     * Behind everything queued on any stream. */
    HIP_TRY(hipDeviceSynchronize());
    std::vector<float> st((size_t)RDSP_ENG_ST_WORDS * (size_t)n, 0.0f);
    for (int i = 0; i < n; i++) {
      const int one = 1;
      memcpy(&st[(size_t)RDSP_ENG_ST_WORDS * i + 3], &one, 4);
    }
    HIP_TRY(hipMemcpy(pl.at(c, (size_t)first), st.data(), st.size() * sizeof(float), hipMemcpyHostToDevice));
    return RDSP_OK;
  }
  HIP_TRY(hipMemset(pl.at(c, (size_t)first), 0, pl.per_channel * (size_t)n));
  return RDSP_OK;
}

int chain_planes_create(rdsp_chain_t *c, int opt) {
  const size_t nch = (size_t)c->n_channels;
  for (const auto &pl : chain_planes(c)) {
    if (pl.opt != opt || pl.rows == 0 || pl.present()) continue;
    HIP_TRY(hipMalloc(pl.slot, pl.rows * nch * pl.per_channel)); /* into its DevBuf */
    StatePlane all = pl;                                          /* every row of the allocation */
    all.row = 0;
    all.per_channel = pl.rows * pl.per_channel;
    RC_TRY(chain_plane_boot(c, all, 0, c->n_channels));
  }
  return RDSP_OK;
}

/* ---- per-channel state as data: checkpoint / resume, channels moved between chains or GPUs ------
 * The reference keeps its DSP state in globals (CONV:50-57,77-80; NR:26-32; SPEC:109) and has no
 * persistence; here the state is an explicit per-channel record, so a range of
 * channels can be written out and read back into the same range of another chain -- same FFT_L and
 * decimation, same settings (modes, filters and gains are configuration: the caller re-applies them).
 * Blob: header, then the arrays of DESIGN.md 3 for the n channels, each [n][...]. */
namespace {
struct StateHeader {
  uint32_t magic, version; /* "RDSP", 4 */
  int32_t n_channels, fft_l, decim;
  int32_t has_sam, has_iir;
  int32_t old_nr_level;
  uint64_t n_in;
  int64_t nr_calls, als_calls;
  float nr_mu, als_mu;
  int32_t hist_valid, hist_swap;
  float hist_scale_i, hist_scale_q;
  int32_t n_groups;      /* followed by n_groups x {has_dev_dphi, dev_dphi}: the NCO increment each group's FIR
                            history was mixed with (a tuning change right before the checkpoint) */
  int32_t has_slip;      /* the last call ran with the I2S slip correction: its carry word travels too */
  int32_t fir_fd;        /* stage A3 of the saving chain: 0 direct, 1 frequency domain with 448-sample frames, 2 with
                            granule frames (informative: all keep the same 256 raw samples, so a stream may be
                            continued in any of them) */
  int32_t has_eng_tail;  /* the engine-law tail state travels (allocated by a switch to RDSP_TAIL_ENGINE); this word
                            sits in what was the header's tail padding, zero in every blob of a chain without it */
};
static_assert(sizeof(StateHeader) == 96, "the blob header of chains without the engine-law state keeps its size");
constexpr uint32_t kStateVersion = 4;
constexpr uint32_t kStateMagic = 0x50534452u; /* 'R' 'D' 'S' 'P' */
/* the optional stages whose planes a blob carries / a chain has, as bits 1 << OPT_* */
unsigned opts_of(const StateHeader &h) {
  return (h.has_sam ? 1u << OPT_SAM : 0u) | (h.has_iir ? 1u << OPT_IIR : 0u) | (h.has_slip ? 1u << OPT_SLIP : 0u) |
         (h.has_eng_tail ? 1u << OPT_ENG_TAIL : 0u);
}
bool carried(const StatePlane &pl, unsigned opts) { return pl.opt == OPT_NONE || (opts >> pl.opt & 1u); }
size_t state_bytes(rdsp_chain_t *c, int n, unsigned opts, size_t n_groups) {
  size_t b = sizeof(StateHeader) + 2 * sizeof(uint32_t) * n_groups;
  for (const auto &pl : chain_planes(c))
    if (carried(pl, opts)) b += pl.per_channel * (size_t)n;
  return b;
}
}  // namespace

extern "C" size_t rdsp_chain_state_bytes(const rdsp_chain_t *c_, int n_channels) {
  rdsp_chain_t *c = const_cast<rdsp_chain_t *>(c_); /* the table holds the owners' slots; nothing is written */
  if (!c || n_channels <= 0 || n_channels > c->n_channels) return 0;
  /* an upper bound that only set-up calls change: optional parts count once their buffers exist (the slip
   * carry travels only when the last call ran corrected, but its place is reserved as soon as
   * rdsp_pre_setIQslip has allocated it), so a buffer sized after set-up fits every later save */
  unsigned opts = 0;
  for (const auto &pl : chain_planes(c))
    if (pl.present()) opts |= 1u << pl.opt;
  return state_bytes(c, n_channels, opts, c->groups.size());
}

/* everything queued so far has finished when the copy is taken (a control-path call) */
extern "C" int rdsp_chain_save_state(rdsp_chain_t *c, int first_channel, int n_channels, void *host_buf, size_t bytes,
                                     void *stream) {
  NEED(c);
  if (!host_buf || first_channel < 0 || n_channels <= 0 || first_channel + n_channels > c->n_channels ||
      bytes < rdsp_chain_state_bytes(c, n_channels))
    return chain_fail(RDSP_ERR_INVALID, "rdsp_chain_save_state: bad argument (channels %d..%d of %d, %zu bytes, %zu needed)", first_channel,
                                        first_channel + n_channels, c->n_channels, bytes, rdsp_chain_state_bytes(c, n_channels));
  if (c->engine)
    return chain_fail(RDSP_ERR_UNSUPPORTED, "rdsp_chain_save_state: the chain is engine-literal and the blob does not carry the pre-processor's and "
                                            "the engine's state; save those with rdsp_engine_save_state on rdsp_chain_engine(chain)");
  RC_TRY(chain_check_device(c));
  RC_TRY(chain_drain_all(c, stream));
  StateHeader h;
  memset(&h, 0, sizeof(h));
  h.magic = kStateMagic; h.version = kStateVersion;
  h.has_slip = c->slip_prev_on ? 1 : 0;
  h.fir_fd = chain_fir_fd(c); /* decim 1: no decimator */
  h.n_channels = n_channels; h.fft_l = c->N; h.decim = c->decim;
  h.has_sam = c->d_sam != nullptr; h.has_iir = c->d_iir_state != nullptr;
  h.has_eng_tail = c->d_eng_st != nullptr;
  h.old_nr_level = c->old_nr_level; h.n_in = c->n_in;
  h.nr_calls = c->nr_calls; h.als_calls = c->als_calls;
  h.nr_mu = c->nr_mu; h.als_mu = c->als_mu;
  h.hist_valid = c->hist_valid; h.hist_swap = c->hist_swap;
  h.hist_scale_i = c->hist_scale_i; h.hist_scale_q = c->hist_scale_q;
  h.n_groups = (int32_t)c->groups.size();
  unsigned char *dst = (unsigned char *)host_buf;
  memcpy(dst, &h, sizeof(h));
  dst += sizeof(h);
  for (const auto &g : c->groups) {
    const uint32_t w[2] = {g.has_dev_dphi ? 1u : 0u, g.dev_dphi};
    memcpy(dst, w, sizeof(w));
    dst += sizeof(w);
  }
  for (const auto &pl : chain_planes(c)) {
    if (!carried(pl, opts_of(h))) continue;
    const size_t n = pl.per_channel * (size_t)n_channels;
    HIP_TRY(hipMemcpy(dst, pl.at(c, (size_t)first_channel), n, hipMemcpyDeviceToHost));
    dst += n;
  }
  return RDSP_OK;
}

/* the blob's channels become channels first_channel .. of this chain.  A chain that has not processed
 * anything yet also takes the stream position and the call history (resume); one that has must be at
 * the same stream position (channels moved between shards of one stream). */
extern "C" int rdsp_chain_load_state(rdsp_chain_t *c, int first_channel, const void *host_buf, size_t bytes, void *stream) {
  NEED(c);
  StateHeader h;
  if (!host_buf || bytes < sizeof(h)) return chain_fail(RDSP_ERR_INVALID, "rdsp_chain_load_state: bad argument");
  memcpy(&h, host_buf, sizeof(h));
  if (c->engine)
    return chain_fail(RDSP_ERR_UNSUPPORTED, "rdsp_chain_load_state: the chain is engine-literal and a chain blob does not carry the pre-processor's "
                                            "and the engine's state; move those with rdsp_engine_save_state / load_state on rdsp_chain_engine(chain)");
  if (h.magic != kStateMagic || h.version != kStateVersion || h.fft_l != c->N || h.decim != c->decim || h.n_channels <= 0 ||
      h.n_groups < 1 || first_channel < 0 || first_channel + h.n_channels > c->n_channels)
    return chain_fail(RDSP_ERR_INVALID, "rdsp_chain_load_state: blob (version %u) of %d channels, FFT_L %d, decimation %d does not fit channels %d.. "
                                        "of a chain of %d channels, FFT_L %d, decimation %d (blob version %u)", h.version, h.n_channels, h.fft_l,
                                        h.decim, first_channel, c->n_channels, c->N, c->decim, kStateVersion);
  RC_TRY(chain_check_device(c));
  /* A stream continued from a blob is the uninterrupted stream bit for bit, or the call fails: nothing
   * is restored in part.  Optional state the blob carries must have a place in this chain. */
  if (h.has_iir && !c->d_iir_state)
    return chain_fail(RDSP_ERR_INVALID, "rdsp_chain_load_state: the blob carries the IIR audio filter's state; select it first "
                                        "(rdsp_sdr_setAudioFilterKind(chain, RDSP_AUDIO_KIND_IIR))");
  if (h.has_slip && !c->d_slip_carry)
    return chain_fail(RDSP_ERR_INVALID, "rdsp_chain_load_state: the blob was taken with the I2S slip correction on; call rdsp_pre_setIQslip first");
  if (h.has_eng_tail && !c->d_eng_st)
    return chain_fail(RDSP_ERR_INVALID, "rdsp_chain_load_state: the blob carries the engine-law tail state; select the law first "
                                        "(rdsp_chain_set_tail_law(chain, RDSP_TAIL_ENGINE))");
  if (h.has_sam && chain_ensure_sam(c) != RDSP_OK) return RDSP_ERR_HIP;
  if (bytes < state_bytes(c, h.n_channels, opts_of(h), (size_t)h.n_groups))
    return chain_fail(RDSP_ERR_INVALID, "rdsp_chain_load_state: blob truncated");
  const unsigned char *gsrc = (const unsigned char *)host_buf + sizeof(h);
  const bool fresh = c->n_in == 0 && c->call_idx == 0;
  if ((size_t)h.n_groups != c->groups.size()) { /* another partition: fine unless a history increment would be lost */
    for (int g = 0; g < h.n_groups; g++) {
      uint32_t w[2];
      memcpy(w, gsrc + 2 * sizeof(uint32_t) * (size_t)g, sizeof(w));
      if (w[0])
        return chain_fail(RDSP_ERR_INVALID, "rdsp_chain_load_state: the blob has %d receiver groups with a tuning change pending in a FIR history, "
                                            "the chain %zu groups: set the same groups first", h.n_groups, c->groups.size());
    }
  }
  if (!fresh) { /* channels moved between shards of one stream: both sides must be at the same point of it */
    const bool same = c->n_in == h.n_in && (c->nr_calls == 0) == (h.nr_calls == 0) && (c->als_calls == 0) == (h.als_calls == 0) &&
                      c->hist_valid == (h.hist_valid != 0) && c->hist_swap == h.hist_swap && c->hist_scale_i == h.hist_scale_i &&
                      c->hist_scale_q == h.hist_scale_q && c->old_nr_level == h.old_nr_level && c->slip_prev_on == (h.has_slip != 0);
    if (!same)
      return chain_fail(RDSP_ERR_INVALID, "rdsp_chain_load_state: the chain (input sample %llu) and the blob (input sample %llu) are not at the same "
                                          "point of the stream / call history", (unsigned long long)c->n_in, (unsigned long long)h.n_in);
  }
  RC_TRY(chain_drain_all(c, stream));
  const unsigned char *src = gsrc + 2 * sizeof(uint32_t) * (size_t)h.n_groups;
  for (const auto &pl : chain_planes(c)) {
    if (carried(pl, opts_of(h))) {
      const size_t n = pl.per_channel * (size_t)h.n_channels;
      HIP_TRY(hipMemcpy(pl.at(c, (size_t)first_channel), src, n, hipMemcpyHostToDevice));
      src += n;
    } else if (pl.present() && pl.opt != OPT_SLIP) {
      /* optional state the chain has and the blob does not starts as a fresh chain's for these channels */
      RC_TRY(chain_plane_boot(c, pl, first_channel, h.n_channels));
    }
  }
  if (fresh) {
    c->n_in = h.n_in;
    c->old_nr_level = h.old_nr_level;
    c->nr_calls = (long)h.nr_calls; c->als_calls = (long)h.als_calls;
    c->nr_mu = h.nr_mu; c->als_mu = h.als_mu;
    c->hist_valid = h.hist_valid != 0; c->hist_swap = h.hist_swap;
    c->hist_scale_i = h.hist_scale_i; c->hist_scale_q = h.hist_scale_q;
    c->slip_prev_on = h.has_slip != 0;
    if ((size_t)h.n_groups == c->groups.size()) /* same partition: the increments the histories came in with */
      for (auto &g : c->groups) {
        uint32_t w[2];
        memcpy(w, gsrc, sizeof(w));
        gsrc += sizeof(w);
        g.has_dev_dphi = w[0] != 0;
        g.dev_dphi = w[1];
        g.dirty = true;
      }
  }
  return RDSP_OK;
}

/* ---- state read-back ------------------------------------------------------- */
extern "C" int rdsp_chain_get_scalars(rdsp_chain_t *c, float *host_out, void *stream) {
  NEED(c);
  RC_TRY(chain_check_device(c));
  RC_TRY(chain_drain_all(c, stream));
  HIP_TRY(hipMemcpy(host_out, c->d_scal, sizeof(float) * 4 * (size_t)c->n_channels, hipMemcpyDeviceToHost));
  if (c->tail_law == RDSP_TAIL_ENGINE) { /* slot 1: the engine AGC's gain */
    std::vector<float> st((size_t)RDSP_ENG_ST_WORDS * (size_t)c->n_channels);
    HIP_TRY(hipMemcpy(st.data(), c->d_eng_st, st.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (int i = 0; i < c->n_channels; i++) host_out[4 * (size_t)i + 1] = st[(size_t)RDSP_ENG_ST_WORDS * i + 1];
  }
  return RDSP_OK;
}
/* A channel whose NLMS instance has run away (rdsp_chain_get_status) stays dead: arm_lms_norm_init_f32
 * leaves the coefficients (NR:62), so Init_LMS_NR does not clear infinite weights, and the sketch's only
 * cure is a power cycle.  With thousands of receivers the host clears just the ones that need it: the
 * instance's weights, delay block, energy and health word of channels [first, first + count) go back to
 * their boot values, in stream order behind everything queued so far; no other channel is touched. */
extern "C" int rdsp_chain_reset_nlms_channels(rdsp_chain_t *c, int which, int first_channel, int n_channels, void *stream_) {
  NEED(c);
  if ((which != 0 && which != 1) || first_channel < 0 || n_channels <= 0 || first_channel + n_channels > c->n_channels)
    return chain_fail(RDSP_ERR_INVALID, "rdsp_chain_reset_nlms_channels: bad argument");
  RC_TRY(chain_check_device(c));
  hipStream_t stream = (hipStream_t)stream_;
  RC_TRY(chain_drain_tail(c)); /* the tail stage owns these arrays */
  for (const auto &pl : chain_planes(c)) /* the planes of an NLMS instance boot to zero */
    if (pl.inst == which)
      HIP_TRY(hipMemsetAsync(pl.at(c, (size_t)first_channel), 0, pl.per_channel * (size_t)n_channels, stream));
  if (c->s_tail) {
    HIP_TRY(hipEventRecord(c->ev_misc, stream));
    HIP_TRY(hipStreamWaitEvent(c->s_tail, c->ev_misc, 0));
  }
  return RDSP_OK;
}
/* per-channel health word: RDSP_STATUS_* bits, sticky until rdsp_Init_LMS_NR (DSP-NR bits) / rdsp_chain_reset */
extern "C" int rdsp_chain_get_status(rdsp_chain_t *c, uint32_t *host_out, void *stream) {
  NEED(c);
  if (!host_out) return RDSP_ERR_INVALID;
  RC_TRY(chain_check_device(c));
  RC_TRY(chain_drain_all(c, stream));
  const size_t nch = (size_t)c->n_channels;
  std::vector<uint32_t> w(2 * nch);
  HIP_TRY(hipMemcpy(w.data(), c->d_status, sizeof(uint32_t) * 2 * nch, hipMemcpyDeviceToHost));
  const uint32_t als_bits = c->tail_law == RDSP_TAIL_ENGINE ? 0u : 3u; /* the engine's ALS filter has no health words */
  for (size_t i = 0; i < nch; i++) host_out[i] = (w[i] & 3u) | ((w[nch + i] & als_bits) << 4);
  return RDSP_OK;
}
extern "C" int rdsp_chain_get_lms_coeffs(rdsp_chain_t *c, int which, float *host_out, void *stream) {
  NEED(c);
  RC_TRY(chain_check_device(c));
  RC_TRY(chain_drain_all(c, stream));
  HIP_TRY(hipMemcpy(host_out, which ? c->d_als_w : c->d_nr_w,
                    sizeof(float) * RDSP_LMS_TAPS * (size_t)c->n_channels, hipMemcpyDeviceToHost));
  return RDSP_OK;
}
extern "C" int rdsp_chain_get_mask(rdsp_chain_t *c, float *host_out) {
  NEED(c);
  memcpy(host_out, c->groups[0].mask_nat.data(), sizeof(float) * 2 * (size_t)c->N);
  return RDSP_OK;
}
extern "C" int rdsp_chain_get_fir_taps(rdsp_chain_t *c, float *host_out) {
  NEED(c);
  memcpy(host_out, c->fir_nat.data(), sizeof(float) * 256);
  return RDSP_OK;
}
