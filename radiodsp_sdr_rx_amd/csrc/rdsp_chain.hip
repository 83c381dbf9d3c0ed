/*
 * rdsp_chain.hip -- C-ABI launch layer: the chain object (per-channel state in
 * HBM, shared tables) and the calls declared in include/rdsp.h that create, destroy,
 * reset and run it.  Its groups, their selection logic, setters and state live in rdsp_chain_groups.hip,
 * rdsp_chain_select.hip, rdsp_chain_ctl.hip and rdsp_chain_state.hip (rdsp_chain_int.h).  Host logic
 * only; the arithmetic lives in the kernel files (rdsp_front_*.hip, rdsp_tail*.hip, ...).  No CPU fallback exists: if
 * HIP reports no device every compute entry point returns RDSP_ERR_NO_DEVICE.
 */
#include <stdarg.h>
#include <stdio.h>

#include "rdsp_chain_int.h"

static thread_local char g_err[512] = "";

extern "C" void rdsp_set_error(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
int chain_fail(int code, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}
extern "C" const char *rdsp_last_error(void) { return g_err; }
extern "C" const char *rdsp_version(void) { return "rdsp-amd 0.2 (gfx950)"; }
extern "C" int rdsp_experimental_build(void) { return 0; } /* there is one build (include/rdsp.h) */

extern "C" int rdsp_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int chain_check_device(rdsp_chain_t *c) {
  if (hipSetDevice(c->device) != hipSuccess) return chain_fail(RDSP_ERR_HIP, "hipSetDevice(%d) failed", c->device);
  return RDSP_OK;
}

static void agc_params(int mode, float *attack, float *decay) {
  *attack = 0.6f;
  switch (mode) {
    case RDSP_AGC_FAST: *decay = 0.10f; break;
    case RDSP_AGC_MEDIUM: *decay = 0.03f; break;
    case RDSP_AGC_SLOW: *decay = 0.008f; break;
    default: *decay = 0.0f; break;
  }
}

static int chain_build(rdsp_chain_t *c, const rdsp_chain_config_t *cfg, int n_channels, int device,
                       int max_blocks_per_call, int decim) {
  c->cfg = *cfg;
  c->cfg.decim = decim;
  c->n_channels = n_channels;
  c->device = device;
  c->max_blocks = max_blocks_per_call;
  c->N = cfg->fft_l;
  c->decim = decim;
  c->hop = c->N / 2;
  c->n_in = 0;
  c->old_nr_level = 15;            /* CONV:80 */
  c->nr_mu = rdsp_lms_mu(15);      /* Init_LMS_NR(15), INO:172 */
  c->als_mu = rdsp_lms_mu(cfg->als_strength > 0 ? cfg->als_strength : 15);
  c->nr_calls = c->als_calls = 0;
  c->eng_agc_set = (cfg->agc_mode >= RDSP_AGC_FAST && cfg->agc_mode <= RDSP_AGC_SLOW) ? cfg->agc_mode : 0;
  c->fir_nat.assign(256, 0.0f);
  RC_TRY(chain_check_device(c));
  RC_TRY(chain_groups_resize(c, 1));
  GroupState &g0 = c->groups[0];
  g0.lo = cfg->flo_hz; g0.hi = cfg->fhi_hz; g0.nco_hz = cfg->nco_hz; g0.demod = cfg->demod;

  const size_t nch = (size_t)n_channels;
  HIP_TRY(alloc_zero(c->d_fir_hc, 256));
  RC_TRY(chain_planes_create(c, OPT_NONE));
  c->mid_stride = (size_t)max_blocks_per_call * RDSP_BLOCK / decim;
  HIP_TRY(alloc_zero(c->d_mid, c->mid_stride * nch));
  if (decim == 4) {
    std::vector<float> hc(256);
    if (rdsp_design_decimator(256, cfg->fir_cut_hz, cfg->fs_in, cfg->window, c->fir_nat.data(), hc.data()) != 0)
      return chain_fail(RDSP_ERR_INVALID, "decimator design failed");
    HIP_TRY(hipMemcpy(c->d_fir_hc, hc.data(), sizeof(float) * 256, hipMemcpyHostToDevice));
    std::vector<float> img(2 * 4 * (size_t)RDSP_FD_N);
    if (rdsp_fd_decimator_image(c->fir_nat.data(), RDSP_FD_N, img.data()) != 0)
      return chain_fail(RDSP_ERR_INVALID, "decimator spectra failed");
    HIP_TRY(c->d_fd_mask.alloc(img.size() / 2));
    HIP_TRY(hipMemcpy(c->d_fd_mask, img.data(), img.size() * sizeof(float), hipMemcpyHostToDevice));
    c->fd_img = std::move(img); /* the groups' rotated spectra are made from it (chain_groups_commit) */
    std::vector<float> rimg(2 * 4 * 256);
    rdsp_rd_decimator_image(c->fir_nat.data(), rimg.data());
    HIP_TRY(c->d_rd_mask.alloc(rimg.size() / 2));
    HIP_TRY(hipMemcpy(c->d_rd_mask, rimg.data(), rimg.size() * sizeof(float), hipMemcpyHostToDevice));
  }
  /* boot order of the sketch: doConvolutionalInitialize (INO:180, mask from the
   * still-zero taps) then reInitializeFilter (INO:183) */
  int rc = rdsp_doConvolutionalInitialize(c, nullptr);
  if (rc == RDSP_OK) rc = rdsp_reInitializeFilter(c, cfg->flo_hz, cfg->fhi_hz, nullptr);
  if (rc == RDSP_OK && cfg->demod == RDSP_DEMOD_SAM) rc = chain_ensure_sam(c);
  return rc;
}

extern "C" int rdsp_chain_create(const rdsp_chain_config_t *cfg, int n_channels, int device,
                                 int max_blocks_per_call, rdsp_chain_t **out) {
  if (!cfg || !out || n_channels <= 0 || max_blocks_per_call <= 0)
    return chain_fail(RDSP_ERR_INVALID, "rdsp_chain_create: bad argument");
  if (rdsp_plan_radix(cfg->fft_l) == 0)
    return chain_fail(RDSP_ERR_INVALID, "fft_l %d not in {256,512,1024,2048,4096}", cfg->fft_l);
  const int decim = cfg->decim <= 1 ? 1 : cfg->decim;
  if (decim != 1 && decim != 4) return chain_fail(RDSP_ERR_INVALID, "decim %d not supported (1 or 4)", cfg->decim);
  if (decim == 4 && cfg->fir_taps != 256)
    return chain_fail(RDSP_ERR_INVALID, "decimator needs 256 taps (got %d)", cfg->fir_taps);
  if (rdsp_device_count() <= 0)
    return chain_fail(RDSP_ERR_NO_DEVICE, "no HIP device: the rdsp product path has no CPU fallback");
  rdsp_chain_t *c = new rdsp_chain();
  const int rc_build = chain_build(c, cfg, n_channels, device, max_blocks_per_call, decim);
  if (rc_build != RDSP_OK) {
    rdsp_chain_destroy(c); /* frees whatever was allocated before the failure */
    return rc_build;
  }
  *out = c;
  return RDSP_OK;
}

/* The owners in the object release everything (rdsp_chain_int.h); what is queued on the internal streams is waited for
 * here, before any of it goes. */
extern "C" void rdsp_chain_destroy(rdsp_chain_t *c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  for (hipStream_t s : {c->s_copy.s, c->s_mid.s, c->s_tail.s})
    if (s) (void)hipStreamSynchronize(s);
  if (c->engine) rdsp_engine_destroy(c->engine);
  if (c->pre) rdsp_preproc_destroy(c->pre);
  delete c;
}

extern "C" int rdsp_chain_channels(const rdsp_chain_t *c) { return c ? c->n_channels : 0; }
extern "C" int rdsp_chain_decim(const rdsp_chain_t *c) { return c ? c->decim : 0; }
extern "C" int rdsp_chain_device(const rdsp_chain_t *c) { return c ? c->device : -1; }

/* RdspFrontParams::fir_fd of a chain: 0 direct form (and every decim-1 chain), 1 / 2 the wave-wide frequency-domain
 * forms (448-sample frames / one granule per frame), 3 the row form (128 outputs per window) */
int chain_fir_fd(const rdsp_chain_t *c) {
  if (!c->d_fd_mask) return 0;
  switch (c->fir_mode) {
    case 2: return 1;
    case -1: case 4: return 2;
    case 5: return 3;
    default: return 0;
  }
}
/* the smallest call: one kernel chunk = 256 output samples; an overlap-save frame needs fft_l/2 of them */
extern "C" int rdsp_chain_call_unit_blocks(const rdsp_chain_t *c) {
  if (!c) return 0;
  const int out_samples = c->hop > 256 ? c->hop : 256;
  return out_samples * c->decim / RDSP_BLOCK;
}
/* the unit a stream is cut in for bits that do not depend on the cut.  Default decimator, direct form, decim 1:
 * the call unit.  448-sample decimator frames (fir_variant 2; 14 input blocks each): the least common multiple of
 * a frame and the call unit -- calls of whole granules are whole frames, so the frame grid sits at absolute stream
 * positions whatever the split (the reference restricts its call boundaries the same way: `available() >
 * N_BLOCKS`, CONV:231) */
extern "C" int rdsp_chain_granule_blocks(const rdsp_chain_t *c) {
  if (!c) return 0;
  const int unit = rdsp_chain_call_unit_blocks(c);
  if (c->fir_mode != 2 || !c->d_fd_mask) return unit;
  const int frame = 14; /* 448 outputs x 4 / 128 */
  int a = unit, b = frame;
  while (b) { const int t = a % b; a = b; b = t; }
  return unit / a * frame;
}

extern "C" int rdsp_chain_reset(rdsp_chain_t *c, void *stream_) {
  if (!c) return RDSP_ERR_INVALID;
  hipStream_t stream = (hipStream_t)stream_;
  RC_TRY(chain_check_device(c));
  RC_TRY(chain_drain_all(c, stream_));
  c->call_idx = 0;
  c->tail_slot = -1;
  for (const auto &pl : chain_planes(c)) /* the slip carry is not read after a reset (slip_prev_on) */
    if (pl.present() && pl.opt != OPT_SLIP) RC_TRY(chain_plane_boot(c, pl, 0, c->n_channels));
  c->slip_prev_on = false;
  c->n_in = 0;
  c->hist_valid = false;
  c->nr_calls = c->als_calls = 0;
  c->old_nr_level = 15;
  c->nr_mu = rdsp_lms_mu(15);
  for (auto &g : c->groups) { g.has_dev_dphi = false; g.dirty = true; }
  if (c->engine) { /* engine-literal: the pre-processor and the engine in front are part of the chain's signal state */
    RC_TRY(rdsp_preproc_reset(c->pre, stream));
    RC_TRY(rdsp_engine_reset(c->engine, stream));
  }
  return RDSP_OK;
}

/* NR:35-64: new mu; delay line and filter state cleared, energy = 0; the
 * coefficients are NOT cleared (arm_lms_norm_init_f32 leaves them) */
extern "C" int rdsp_Init_LMS_NR(rdsp_chain_t *c, int strength, void *stream_) {
  if (!c) return RDSP_ERR_INVALID;
  RC_TRY(chain_check_device(c));
  hipStream_t stream = (hipStream_t)stream_;
  c->nr_mu = rdsp_lms_mu(strength);
  const size_t nch = (size_t)c->n_channels;
  RC_TRY(chain_drain_tail(c)); /* the tail stage owns these arrays */
  for (const auto &pl : chain_planes(c)) /* the instance's delay block, energy and health words; not its coefficients */
    if (pl.inst == INST_NR && *pl.slot != (void *)c->d_nr_w.p)
      HIP_TRY(hipMemsetAsync(pl.at(c, 0), 0, pl.per_channel * nch, stream));
  if (c->s_tail) {
    HIP_TRY(hipEventRecord(c->ev_misc, stream));
    HIP_TRY(hipStreamWaitEvent(c->s_tail, c->ev_misc, 0));
  }
  return RDSP_OK;
}

/* what a launch of the engine-law stage takes from the chain's settings */
static void eng_tail_params(const rdsp_chain_t *c, RdspTailEngineParams *ep, float *rows, size_t stride, int n_blocks) {
  memset(ep, 0, sizeof(*ep));
  rdsp_tail_engine_constants(ep, c->eng_agc_set);
  ep->in = rows;
  ep->in_stride = stride;
  ep->n_channels = c->n_channels;
  ep->n_blocks = n_blocks;
  ep->st = c->d_eng_st;
  ep->als = c->d_eng_als;
  ep->agc_on = c->cfg.agc_mode != RDSP_AGC_OFF;
  ep->als_on = c->cfg.als_mode != RDSP_ALS_OFF;
  ep->als_notch = c->cfg.als_mode == RDSP_ALS_NOTCH;
  ep->als_clear = c->eng_als_clear ? 1 : 0;
}

/* ---- rdsp_chain_process: one call, in the steps rdsp_chain_process lists ---------------------------------------------- */
struct Call { /* what the steps of one call share */
  const int16_t *d_iq; /* the front kernel's input: the caller's, the engine-literal front's, or the slip pass's */
  size_t in_stride;
  int n_blocks;
  int16_t *d_out; size_t out_stride; float *d_out_f32;
  size_t n_in, n_out;                   /* samples per channel */
  hipStream_t stream, tstream, mstream; /* the caller's; the tail stage's; the SAM PLL's and the IIR cascade's */
  bool sam, iir, eng, tail;             /* stages of this call (eng: the tail runs the engine's laws) */
  bool piped, mid_stage, timed;
  float attack, decay, og;
  int slot, nsb, sbn;                   /* intermediate buffer; channel sub-batches and their size */
  hipEvent_t ev[4];                     /* timed: front begin / end, tail begin / end */
  RdspFrontParams fp;
};

static int check_call(const rdsp_chain_t *c, const int16_t *d_iq, size_t in_stride, int n_blocks, int16_t *d_out,
                      size_t out_stride) {
  if (!c || !d_iq || !d_out || n_blocks <= 0) return chain_fail(RDSP_ERR_INVALID, "rdsp_chain_process: bad argument");
  const int gran = rdsp_chain_call_unit_blocks(c);
  if (n_blocks % gran != 0)
    return chain_fail(RDSP_ERR_NOT_READY, "n_blocks %d is not a multiple of the call unit %d", n_blocks, gran);
  if (n_blocks > c->max_blocks)
    return chain_fail(RDSP_ERR_INVALID, "n_blocks %d exceeds max_blocks_per_call %d", n_blocks, c->max_blocks);
  const size_t n_in = (size_t)n_blocks * RDSP_BLOCK;
  const size_t n_out = n_in / c->decim;
  if (in_stride < n_in || out_stride < n_out || (in_stride & 3) != 0 ||
      ((uintptr_t)d_iq & 15) != 0 || ((uintptr_t)d_out & 15) != 0 || (out_stride & 3) != 0)
    return chain_fail(RDSP_ERR_INVALID, "strides/alignment: in_stride %zu (>= %zu, %%4), out_stride %zu (>= %zu, %%4), 16-byte aligned bases",
                                        in_stride, n_in, out_stride, n_out);
  return RDSP_OK;
}

/* INO:71-72,81-86: IQ -> preProcessor -> SDR -> the record queues; this chain is the CONV stage behind them */
static int engine_front(rdsp_chain_t *c, Call &k) {
  const size_t st = (size_t)c->max_blocks * RDSP_BLOCK;
  RC_TRY(rdsp_preproc_update(c->pre, k.d_iq, k.in_stride, k.n_blocks, c->d_engine_io, st, k.stream));
  RC_TRY(rdsp_engine_update(c->engine, c->d_engine_io, st, k.n_blocks, c->d_engine_io, st, k.stream));
  k.d_iq = c->d_engine_io;
  k.in_stride = st;
  return RDSP_OK;
}

/* which stages the call runs and on which streams; changes nothing */
static int call_stages(const rdsp_chain_t *c, Call &k) {
  const rdsp_chain_config_t &cf = c->cfg;
  k.sam = false; /* any group on the PLL demodulator: its serial stage runs before the tail */
  for (const auto &g : c->groups) k.sam = k.sam || (g.demod == RDSP_DEMOD_SAM);
  if (k.sam && !c->d_sam) /* rdsp_*_setDemodMode(SAM) allocates them; nothing is allocated here */
    return chain_fail(RDSP_ERR_INVALID, "SAM group without PLL buffers (internal)");
  k.iir = c->audio_kind == RDSP_AUDIO_KIND_IIR && cf.filter_on;
  if (k.iir && (!c->d_iir_coef || c->iir_sets < (int)c->groups.size()))
    return chain_fail(RDSP_ERR_INVALID, "IIR audio filter without its buffers (internal)");
  /* RDSP_TAIL_ENGINE: the engine's AGC and ALS filter run in a tail stage whenever either is on; the front kernel's own
   * AGC stays off */
  k.eng = c->tail_law == RDSP_TAIL_ENGINE;
  const bool eng_stage = k.eng && (cf.agc_mode != RDSP_AGC_OFF || cf.als_mode != RDSP_ALS_OFF);
  k.tail = k.sam || k.iir || (cf.lms_nr > 0) || (!k.eng && cf.als_mode != RDSP_ALS_OFF) || eng_stage;
  agc_params(cf.agc_mode, &k.attack, &k.decay);
  k.og = cf.mute ? 0.0f : cf.output_gain;
  k.timed = c->timing_on && 4 * (c->ev_used + 1) <= c->ev.size();
  k.piped = k.tail && c->pipe_on;
  k.slot = (int)(c->call_idx % 3);
  k.tstream = k.piped ? c->s_tail.s : k.stream;
  k.mid_stage = k.sam || k.iir;
  k.mstream = (k.piped && k.mid_stage) ? c->s_mid.s : k.tstream; /* SAM PLL / IIR cascade */
  /* channel sub-batches (see sub_batch): only where the tail runs on its own stream */
  k.nsb = (k.piped && !k.sam) ? chain_sub_batches(c) : 1;
  k.sbn = k.nsb > 1 ? c->sub_batch : c->n_channels;
  return RDSP_OK;
}

/* rdsp_pre_setIQslip: the corrected words of this call go to d_slip_buf, which the front kernel then reads */
static int slip_pass(rdsp_chain_t *c, Call &k) {
  if (c->iq_slip != 0) {
    /* the word in front of this call's first sample: the previous pass's carry, or -- when the previous
     * call ran without the correction -- the last word of the FIR history, which is raw then */
    const size_t sstride = (size_t)c->max_blocks * RDSP_BLOCK;
    const uint32_t *cin = c->slip_prev_on ? c->slip_carry(c->slip_phase) : c->d_hist + 255;
    int e = rdsp_launch_iq_slip(reinterpret_cast<const uint32_t *>(k.d_iq), k.in_stride, c->d_slip_buf, sstride, cin,
                                c->slip_prev_on ? 1 : 256, c->slip_carry(c->slip_phase ^ 1), (int)k.n_in, c->iq_slip,
                                c->n_channels, k.stream);
    if (e != 0) return launch_failed("slip kernel launch failed", e);
    k.d_iq = reinterpret_cast<const int16_t *>(c->d_slip_buf.p);
    k.in_stride = sstride;
    c->slip_phase ^= 1;
  }
  c->slip_prev_on = c->iq_slip != 0;
  return RDSP_OK;
}

/* the front kernel's arguments (and front_name) from the chain's settings and the call's stages */
static void front_params(rdsp_chain_t *c, Call &k) {
  const rdsp_chain_config_t &cf = c->cfg;
  RdspFrontParams &fp = k.fp;
  memset(&fp, 0, sizeof(fp));
  fp.iq = reinterpret_cast<const uint32_t *>(k.d_iq);
  fp.in_stride = k.in_stride;
  fp.n_chunks = (int)(k.n_in / (size_t)(256 * c->decim));
  fp.n0 = (uint32_t)c->n_in;
  fp.scale_i = cf.iq_balance * cf.input_gain * (1.0f / 32768.0f);
  fp.scale_q = cf.input_gain * (1.0f / 32768.0f);
  fp.swap_iq = c->swap_iq;
  fp.swap_hist = c->hist_valid ? c->hist_swap : fp.swap_iq;
  fp.scale_i_hist = c->hist_valid ? c->hist_scale_i : fp.scale_i;
  fp.scale_q_hist = c->hist_valid ? c->hist_scale_q : fp.scale_q;
  fp.nb_on = c->nb_on;
  fp.nb_thr = (float)pow(10.0, (double)c->nb_threshold_db / 10.0);
  fp.fir_hc = c->d_fir_hc;
  fp.groups = c->d_groups;
  fp.group_of = c->d_group_of;
  fp.mask_pool = c->d_mask_pool;
  fp.spectral_on = cf.spectral_nr == 2 ? 2 : (cf.spectral_nr ? 1 : 0);
  if (cf.spectral_nr == 2) { /* older variant, backup/RadioDSP_SDR_RX_Conv.ino:1594-1596: bins 60..120, x3 */
    fp.spectral_k = 3.0f;
    fp.vad_lo = 60 * c->N / 256;
    fp.vad_hi = 120 * c->N / 256;
  } else {
    fp.spectral_k = (float)((double)cf.spectral_level * 1.5);
    fp.vad_lo = 30 * c->N / 256; /* STATING_BIN_VAD_ANALISYS, SPEC:34, scaled with FFT_L */
    fp.vad_hi = 180 * c->N / 256;
  }
  /* SPEC only: the older variant scales the bin (BK_INO:1614-1628) */
  fp.spectral_literal = (c->spectral_literal && cf.spectral_nr == 1) ? c->spectral_literal : 0;
  fp.sin_table = c->d_sin_table;
  fp.to_mid = k.tail ? 1 : 0;
  fp.agc_on = !k.eng && cf.agc_mode != RDSP_AGC_OFF;
  fp.agc_attack = k.attack;
  fp.agc_decay = k.decay;
  fp.out_gain = k.og;
  fp.st_hist = c->d_hist;
  fp.st_prev = c->d_prev;
  fp.st_scal = c->d_scal;
  fp.out_i16 = reinterpret_cast<uint32_t *>(k.d_out);
  fp.out_stride = k.out_stride;
  fp.out_f32 = reinterpret_cast<float2 *>(k.d_out_f32);
  fp.mid_stride = c->mid_stride;
  /* full-register front kernel in both modes: since its butterflies shrank to 199 VGPRs two of
   * its waves and a tail wave fit one SIMD, and the lean variant's twiddle chains only cost */
  fp.lean = (c->lean_mode < 0) ? 0 : c->lean_mode;
  fp.front_prio = k.piped ? c->front_fir_prio : 0;
  fp.fir_matrix = 0;
  /* stage A3 (rdsp_chain_set_fir_variant).  Default (-1) and 4: in the frequency domain with frames of one granule
   * (256 outputs per 512-point window): every frame's input is a function of the absolute sample position, so the
   * bits do not depend on how the stream is cut into calls -- like the direct form (0), at about two thirds of
   * its cost.  2: 448-sample frames anchored at the call's first sample: the throughput form bench.py selects. */
  fp.fir_fd = chain_fir_fd(c);
  /* the default (-1) picks between the two split-invariant frequency-domain forms: on 16-lane rows where no tail kernel
   * will share the SIMDs with this call's front kernel (4-10 % faster there), wave-wide frames of one granule beside
   * it (the rows' 233-256 registers would leave one front wave per SIMD).  A function of the chain's settings at this
   * call, not of how the stream is cut: both give the same bits for any split. */
  if (c->fir_mode == -1 && fp.fir_fd == 2 && !fp.to_mid) fp.fir_fd = 3;
  fp.fd_mask = c->d_fd_mask;
  fp.rot_pool = c->d_rot_pool; /* null above RDSP_FD_ROT_GROUPS groups: the instance that rotates per frame (rdsp_front_pick_rotg) */
  fp.fd_shift = c->d_rot_pool && rdsp_fd_shift_plan(c->N); /* what group_stage_rot fills the pool with */
  fp.rd_mask = c->d_rd_mask;
  RdspFrontPick pick; /* the kernel this call runs, for the timing records (a refusal leaves the name: the launch reports it) */
  if (rdsp_front_pick(c->N, c->decim, &fp, &pick) == 0) c->front_name = rdsp_front_kernel_name(pick.family);
  /* the intermediate buffers of this call: slot 0 is d_mid */
  fp.mid = (k.piped && k.slot) ? c->d_midx[k.slot - 1].p : c->d_mid.p;
  fp.mid_q = c->d_mid_q[k.piped ? k.slot : 0];
}

/* what the caller's stream waits for before the front kernels, the first timing event, the group records */
static int front_waits(rdsp_chain_t *c, Call &k) {
  hipStream_t stream = k.stream;
  /* the tail of call k-2 read this intermediate buffer: wait for it */
  if (k.piped && c->call_idx >= 3) HIP_TRY(hipStreamWaitEvent(stream, c->ev_tail[k.slot], 0));
  if (!k.piped && c->tail_slot >= 0) {
    /* the previous call's tail stage may still be running on s_tail: it owns that call's d_out and
     * updates the AGC gain (st_scal) this call's front kernel reads and writes when it packs itself
     * (tail stage switched off between two calls), and the NLMS state an in-stream tail uses */
    HIP_TRY(hipStreamWaitEvent(stream, c->ev_tail[c->tail_slot], 0));
    c->tail_slot = -1;
  }
  if (k.timed) { /* events come from a pool created in rdsp_chain_set_timing */
    for (int i = 0; i < 4; i++) k.ev[i] = c->ev[4 * c->ev_used + i];
    HIP_TRY(hipEventRecord(k.ev[0], stream));
  }
  /* the PLL kernel of the previous call (on s_tail) reads the group records: a record is only
   * rewritten after it has finished */
  bool any_dirty = false;
  for (const auto &g : c->groups) any_dirty = any_dirty || g.dirty;
  if (any_dirty && c->d_sam && c->tail_slot >= 0) HIP_TRY(hipStreamWaitEvent(stream, c->ev_tail[c->tail_slot], 0));
  return chain_groups_commit(c, stream);
}

/* the front kernels, one per channel sub-batch, and what marks them done */
static int launch_fronts(rdsp_chain_t *c, Call &k) {
  hipStream_t stream = k.stream;
  if (k.nsb > 1 && c->ev_front_sb[k.slot].size() < (size_t)k.nsb) /* made by set_pipelined / set_sub_batch */
    return chain_fail(RDSP_ERR_INVALID, "sub-batch events missing (internal)");
  int e = 0;
  for (int b = 0; b < k.nsb && e == 0; b++) {
    k.fp.ch_base = b * k.sbn;
    const int count = (c->n_channels - k.fp.ch_base < k.sbn) ? c->n_channels - k.fp.ch_base : k.sbn;
    e = rdsp_launch_front(c->N, c->decim, &k.fp, count, stream);
    if (k.nsb > 1 && e == 0) HIP_TRY(hipEventRecord(c->ev_front_sb[k.slot][b], stream));
  }
  if (k.timed) HIP_TRY(hipEventRecord(k.ev[1], stream));
  HIP_TRY(hipEventRecord(c->ev_fence, stream));
  c->fence_valid = true;
  if (e != 0) return launch_failed("front kernel launch failed", e);
  if (k.piped && k.nsb == 1) {
    HIP_TRY(hipEventRecord(c->ev_front[k.slot], stream));
    HIP_TRY(hipStreamWaitEvent(k.mid_stage ? c->s_mid : c->s_tail, c->ev_front[k.slot], 0));
  }
  return RDSP_OK;
}

static int sam_stage(rdsp_chain_t *c, Call &k) {
  RdspSamParams sp = {};
  sp.mid = k.fp.mid;
  sp.mid_q = k.fp.mid_q;
  sp.mid_stride = c->mid_stride;
  sp.n_channels = c->n_channels;
  sp.n_samples = (int)k.n_out;
  sp.groups = c->d_groups;
  sp.group_of = c->d_group_of;
  rdsp_sam_constants(c->cfg.fs_in / (double)c->decim, &sp.g1, &sp.g2, &sp.wmin, &sp.wmax);
  sp.st_sam = c->d_sam;
  int es = rdsp_launch_sam(&sp, k.mstream);
  return es != 0 ? launch_failed("SAM kernel launch failed", es) : RDSP_OK;
}

/* SDR.setAudioFilter as a biquad cascade on the demodulated audio, before NR / notch / AGC */
static int iir_stage(rdsp_chain_t *c, Call &k) {
  for (size_t gi = 0; gi < c->groups.size(); gi++) {
    GroupState &g = c->groups[gi];
    if (!g.iir_dirty) continue;
    int eb = rdsp_launch_biquad_coef_store(c->d_iir_coef + 20 * gi, g.iir, k.mstream);
    if (eb != 0) return launch_failed("IIR coefficient store failed", eb);
    g.iir_dirty = false;
  }
  RdspBiquadParams bp = {};
  bp.buf = k.fp.mid;
  bp.stride = c->mid_stride;
  bp.n_channels = c->n_channels;
  bp.n_samples = (int)k.n_out;
  bp.coef = c->d_iir_coef;
  bp.set_of = c->d_group_of;
  bp.state = c->d_iir_state;
  if (k.nsb > 1) /* sub-batched fronts: the cascade covers all channels, after the last of them */
    for (int b = 0; b < k.nsb; b++) HIP_TRY(hipStreamWaitEvent(k.mstream, c->ev_front_sb[k.slot][b], 0));
  int eb = rdsp_launch_biquad(&bp, k.mstream);
  return eb != 0 ? launch_failed("biquad kernel launch failed", eb) : RDSP_OK;
}

/* NLMS noise reduction, notch / peak filter, AGC, pack -- under the build's law or the engine's */
static int tail_stage(rdsp_chain_t *c, Call &k) {
  const rdsp_chain_config_t &cf = c->cfg;
  if (k.piped && k.mid_stage) { /* the tail stage of this call follows its PLL / cascade */
    HIP_TRY(hipEventRecord(c->ev_mid[k.slot], c->s_mid));
    HIP_TRY(hipStreamWaitEvent(c->s_tail, c->ev_mid[k.slot], 0));
  }
  RdspTailParams tp = {};
  tp.mid = k.fp.mid;
  tp.mid_stride = c->mid_stride;
  tp.n_channels = c->n_channels;
  tp.n_blocks = (int)(k.n_out / RDSP_BLOCK);
  tp.nr_on = cf.lms_nr > 0;
  tp.als_mode = k.eng ? RDSP_ALS_OFF : cf.als_mode;
  tp.nr_mu = c->nr_mu;
  tp.als_mu = c->als_mu;
  tp.nr_first = (c->nr_calls == 0);
  tp.als_first = (c->als_calls == 0);
  tp.nr_w = c->d_nr_w; tp.nr_prev = c->d_nr_prev; tp.nr_energy = c->d_nr_energy;
  tp.als_w = c->d_als_w; tp.als_prev = c->d_als_prev; tp.als_energy = c->d_als_energy;
  tp.agc_on = k.fp.agc_on;
  tp.agc_attack = k.attack;
  tp.agc_decay = k.decay;
  tp.out_gain = k.og;
  tp.st_scal = c->d_scal;
  tp.st_status = c->d_status;
  tp.st_status_stride = (size_t)c->n_channels;
  tp.prio = k.piped ? c->tail_prio : 0;
  tp.energy_running = c->nlms_energy_running;
  tp.out_i16 = reinterpret_cast<uint32_t *>(k.d_out);
  tp.out_stride = k.out_stride;
  tp.out_f32 = reinterpret_cast<float2 *>(k.d_out_f32);
  RdspTailEngineParams ep;
  if (k.eng) {
    /* [A7 DSP-NR as rdsp_LMS_NoiseReduction runs it, x 1.1 (CONV:334), floats in place] -> engine AGC -> engine ALS
     * -> output gain -> pack */
    eng_tail_params(c, &ep, k.fp.mid, c->mid_stride, (int)(k.n_out / RDSP_BLOCK));
    ep.out_i16 = tp.out_i16; ep.out_f32 = tp.out_f32; ep.out_stride = k.out_stride; ep.out_gain = k.og;
    ep.prio = tp.prio;
    tp.raw_out = k.fp.mid;
    tp.nr_mode = 0;
  }
  if (k.timed) HIP_TRY(hipEventRecord(k.ev[2], k.tstream));
  int e = 0;
  for (int b = 0; b < k.nsb && e == 0; b++) {
    tp.ch_base = b * k.sbn;
    tp.n_channels = (c->n_channels - tp.ch_base < k.sbn) ? c->n_channels : tp.ch_base + k.sbn;
    if (k.nsb > 1) HIP_TRY(hipStreamWaitEvent(c->s_tail, c->ev_front_sb[k.slot][b], 0));
    if (!k.eng || tp.nr_on) e = rdsp_launch_tail(&tp, c->tail_lpc, k.tstream);
    if (k.eng && e == 0) {
      ep.ch_base = tp.ch_base;
      ep.n_channels = tp.n_channels;
      e = rdsp_launch_tail_engine(&ep, k.tstream);
    }
  }
  if (k.eng && ep.als_on) c->eng_als_clear = false;
  if (e != 0) return launch_failed("tail kernel launch failed", e);
  if (k.timed) HIP_TRY(hipEventRecord(k.ev[3], k.tstream));
  if (k.piped) {
    HIP_TRY(hipEventRecord(c->ev_tail[k.slot], c->s_tail));
    c->tail_slot = k.slot;
  }
  if (tp.nr_on) c->nr_calls += tp.n_blocks;
  if (tp.als_mode) c->als_calls += tp.n_blocks;
  return RDSP_OK;
}

/* the call is queued: it becomes the history of the next one */
static void finish_call(rdsp_chain_t *c, const Call &k) {
  if (k.timed) {
    c->ev_has_tail[c->ev_used] = k.tail ? 1 : 0;
    c->ev_used++;
  }
  c->call_idx++;
  c->n_in += k.n_in;
  c->hist_valid = true;
  c->hist_swap = k.fp.swap_iq;
  c->hist_scale_i = k.fp.scale_i;
  c->hist_scale_q = k.fp.scale_q;
}

extern "C" int rdsp_chain_process(rdsp_chain_t *c, const int16_t *d_iq, size_t in_stride,
                                  int n_blocks, int16_t *d_out, size_t out_stride,
                                  float *d_out_f32, void *stream_) {
  RC_TRY(check_call(c, d_iq, in_stride, n_blocks, d_out, out_stride));
  RC_TRY(chain_check_device(c));
  Call k = {d_iq, in_stride, n_blocks, d_out, out_stride, d_out_f32}; /* the rest zero */
  k.n_in = (size_t)n_blocks * RDSP_BLOCK;
  k.n_out = k.n_in / c->decim;
  k.stream = (hipStream_t)stream_;
  if (c->engine) RC_TRY(engine_front(c, k));
  if (c->cfg.lms_nr > 0 && c->cfg.lms_nr != c->old_nr_level) { /* CONV:326-330: nr level change re-initialises the NLMS instance */
    RC_TRY(rdsp_Init_LMS_NR(c, c->cfg.lms_nr, k.stream));
    c->old_nr_level = c->cfg.lms_nr;
  }
  RC_TRY(call_stages(c, k));
  RC_TRY(slip_pass(c, k));
  front_params(c, k);
  RC_TRY(front_waits(c, k));
  RC_TRY(launch_fronts(c, k));
  if (k.sam) RC_TRY(sam_stage(c, k));
  if (k.iir) RC_TRY(iir_stage(c, k));
  if (k.tail) RC_TRY(tail_stage(c, k));
  finish_call(c, k);
  return RDSP_OK;
}

/* LMS_NoiseReduction(blockSize, nrbuffer), NR:66-80: the DSP-NR instance alone, in
 * place on float buffers [n_channels][stride], n_samples a multiple of 128 */
extern "C" int rdsp_LMS_NoiseReduction(rdsp_chain_t *c, int n_samples, float *d_nrbuffer,
                                       size_t stride, void *stream_) {
  if (!c || !d_nrbuffer || n_samples <= 0 || n_samples % RDSP_BLOCK != 0 || stride < (size_t)n_samples ||
      (stride & 3) != 0 || ((uintptr_t)d_nrbuffer & 15) != 0)
    return chain_fail(RDSP_ERR_INVALID, "rdsp_LMS_NoiseReduction: bad argument");
  RC_TRY(chain_check_device(c));
  RC_TRY(chain_drain_tail(c));
  RdspTailParams tp = {};
  tp.mid = d_nrbuffer;
  tp.mid_stride = stride;
  tp.raw_out = d_nrbuffer;
  tp.n_channels = c->n_channels;
  tp.n_blocks = n_samples / RDSP_BLOCK;
  tp.nr_on = 1;
  tp.nr_mode = 2;
  tp.nr_mu = c->nr_mu;
  tp.nr_first = (c->nr_calls == 0);
  tp.energy_running = c->nlms_energy_running;
  tp.nr_w = c->d_nr_w; tp.nr_prev = c->d_nr_prev; tp.nr_energy = c->d_nr_energy;
  tp.st_scal = c->d_scal;
  tp.st_status = c->d_status;
  tp.st_status_stride = (size_t)c->n_channels;
  int e = rdsp_launch_tail(&tp, c->tail_lpc, (hipStream_t)stream_);
  if (e != 0) return launch_failed("tail kernel launch failed", e);
  c->nr_calls += tp.n_blocks;
  return RDSP_OK;
}

/* ---- the engine law of the chain's tail (RDSP_TAIL_ENGINE) --------------------------------------------------- */
extern "C" int rdsp_chain_set_tail_law(rdsp_chain_t *c, int law) {
  if (!c) return RDSP_ERR_INVALID;
  if (law != RDSP_TAIL_BUILD && law != RDSP_TAIL_ENGINE)
    return chain_fail(RDSP_ERR_INVALID, "rdsp_chain_set_tail_law: law %d is not RDSP_TAIL_BUILD (0) or RDSP_TAIL_ENGINE (1)", law);
  if (law == RDSP_TAIL_ENGINE && c->engine)
    return chain_fail(RDSP_ERR_UNSUPPORTED, "rdsp_chain_set_tail_law: the engine-literal chain runs the reference's engine itself; "
                                            "its setters reach that object");
  if (law == c->tail_law) return RDSP_OK;
  RC_TRY(chain_check_device(c));
  RC_TRY(chain_drain_tail(c));
  HIP_TRY(hipDeviceSynchronize());
  if (law == RDSP_TAIL_ENGINE) {
    if (!c->d_eng_st || !c->d_eng_als) RC_TRY(chain_planes_create(c, OPT_ENG_TAIL)); /* the first switch allocates them, booted */
    else
      for (const auto &pl : chain_planes(c))
        if (pl.opt == OPT_ENG_TAIL) RC_TRY(chain_plane_boot(c, pl, 0, c->n_channels));
    c->eng_als_clear = false;
  } else { /* the build law's tail state as a fresh chain has it: ALS instance cleared, AGC gain 1 */
    for (const auto &pl : chain_planes(c))
      if (pl.inst == INST_ALS) RC_TRY(chain_plane_boot(c, pl, 0, c->n_channels));
    RC_TRY(chain_gain_one(c, 0, c->n_channels, true));
    c->als_calls = 0;
  }
  c->tail_law = law;
  return RDSP_OK;
}
extern "C" int rdsp_chain_get_tail_law(const rdsp_chain_t *c) { return c ? c->tail_law : RDSP_ERR_INVALID; }

/* the engine-law AGC then ALS filter alone, in place on float audio [n_channels][stride] (what rdsp_LMS_NoiseReduction
 * is to the DSP-NR instance) */
extern "C" int rdsp_chain_run_tail_f32(rdsp_chain_t *c, float *d_audio, size_t stride, int n_samples, void *stream) {
  if (!c) return RDSP_ERR_INVALID;
  if (c->tail_law != RDSP_TAIL_ENGINE)
    return chain_fail(RDSP_ERR_UNSUPPORTED, "rdsp_chain_run_tail_f32: the chain's tail law is not RDSP_TAIL_ENGINE");
  if (!d_audio || n_samples <= 0 || n_samples % RDSP_BLOCK != 0 || stride < (size_t)n_samples)
    return chain_fail(RDSP_ERR_INVALID, "rdsp_chain_run_tail_f32: bad argument (n_samples %d: a positive multiple of %d, stride %zu)", n_samples,
                                        RDSP_BLOCK, stride);
  RC_TRY(chain_check_device(c));
  RC_TRY(chain_drain_tail(c));
  RdspTailEngineParams ep;
  eng_tail_params(c, &ep, d_audio, stride, n_samples / RDSP_BLOCK);
  ep.raw_out = d_audio;
  int e = rdsp_launch_tail_engine(&ep, (hipStream_t)stream);
  if (e != 0) return launch_failed("engine-law tail kernel launch failed", e);
  if (ep.als_on) c->eng_als_clear = false;
  return RDSP_OK;
}

extern "C" int rdsp_doConvolutionalProcessing(rdsp_chain_t *c, float iNRLevel, int bFilterEnabled,
                                              double dFLoCut, double dFHiCut, const int16_t *d_iq,
                                              size_t in_stride, int n_blocks, int16_t *d_out,
                                              size_t out_stride, void *stream) {
  (void)dFLoCut; /* ignored by the reference too: only bFilterEnabled is read, CONV:300 */
  (void)dFHiCut;
  if (!c) return RDSP_ERR_INVALID;
  c->cfg.lms_nr = (int)iNRLevel;
  const int f = bFilterEnabled ? 1 : 0;
  if (f != c->cfg.filter_on) {
    c->cfg.filter_on = f;
    for (size_t i = 0; i < c->groups.size(); i++) RC_TRY(chain_group_stage(c, (int)i));
  }
  return rdsp_chain_process(c, d_iq, in_stride, n_blocks, d_out, out_stride, nullptr, stream);
}

extern "C" int rdsp_q15_to_float(const int16_t *d_src, float *d_dst, size_t n, void *stream) {
  if (rdsp_device_count() <= 0) return chain_fail(RDSP_ERR_NO_DEVICE, "no HIP device");
  int e = rdsp_launch_q15_to_float(d_src, d_dst, n, (hipStream_t)stream);
  return e ? launch_failed("q15_to_float launch", e) : RDSP_OK;
}
extern "C" int rdsp_float_to_q15(const float *d_src, int16_t *d_dst, size_t n, void *stream) {
  if (rdsp_device_count() <= 0) return chain_fail(RDSP_ERR_NO_DEVICE, "no HIP device");
  int e = rdsp_launch_float_to_q15(d_src, d_dst, n, (hipStream_t)stream);
  return e ? launch_failed("float_to_q15 launch", e) : RDSP_OK;
}
