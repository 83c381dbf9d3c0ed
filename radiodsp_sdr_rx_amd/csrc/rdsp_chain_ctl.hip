/*
 * rdsp_chain_ctl.hip -- rdsp_chain_t's control path: the rdsp_sdr_* / rdsp_pre_* / rdsp_set_* setters, pipelined mode,
 * sub-batches, priorities, kernel variants, flush, timing, and the engine-literal switch.
 */
#include "rdsp_chain_int.h"

/* ---- engine setters ------------------------------------------------------- */
extern "C" int rdsp_sdr_enableAGC(rdsp_chain_t *c) {
  TO_ENGINE(c, rdsp_engine_enableAGC(c->engine));
  if (c->cfg.agc_mode == RDSP_AGC_OFF) c->cfg.agc_mode = c->saved_agc_mode;
  return RDSP_OK;
}
extern "C" int rdsp_sdr_disableAGC(rdsp_chain_t *c) {
  TO_ENGINE(c, rdsp_engine_setAGCmode(c->engine, 0));
  if (c->cfg.agc_mode != RDSP_AGC_OFF) c->saved_agc_mode = c->cfg.agc_mode;
  c->cfg.agc_mode = RDSP_AGC_OFF;
  return RDSP_OK;
}
extern "C" int rdsp_sdr_setAGCmode(rdsp_chain_t *c, int mode) {
  TO_ENGINE(c, rdsp_engine_setAGCmode(c->engine, mode));
  if (mode < RDSP_AGC_OFF || mode > RDSP_AGC_SLOW) return RDSP_ERR_INVALID;
  c->cfg.agc_mode = mode;
  if (mode != RDSP_AGC_OFF) c->eng_agc_set = mode; /* 0xdfe0: mode 0 only switches the engine AGC off */
  return RDSP_OK;
}
extern "C" int rdsp_sdr_enableALSfilter(rdsp_chain_t *c) {
  TO_ENGINE(c, rdsp_engine_enableALSfilter(c->engine));
  if (c->cfg.als_mode == RDSP_ALS_OFF) c->cfg.als_mode = c->saved_als_mode;
  c->eng_als_clear = true;
  return RDSP_OK;
}
extern "C" int rdsp_sdr_disableALSfilter(rdsp_chain_t *c) {
  TO_ENGINE(c, rdsp_engine_disableALSfilter(c->engine));
  if (c->cfg.als_mode != RDSP_ALS_OFF) c->saved_als_mode = c->cfg.als_mode;
  c->cfg.als_mode = RDSP_ALS_OFF;
  return RDSP_OK;
}
static int set_als_shape(rdsp_chain_t *c, int mode) { /* the shape is kept while the filter is off */
  c->saved_als_mode = mode;
  if (c->cfg.als_mode != RDSP_ALS_OFF) c->cfg.als_mode = mode;
  return RDSP_OK;
}
extern "C" int rdsp_sdr_setALSfilterNotch(rdsp_chain_t *c) {
  TO_ENGINE(c, rdsp_engine_setALSfilterNotch(c->engine));
  return set_als_shape(c, RDSP_ALS_NOTCH);
}
extern "C" int rdsp_sdr_setALSfilterPeak(rdsp_chain_t *c) {
  TO_ENGINE(c, rdsp_engine_setALSfilterPeak(c->engine));
  return set_als_shape(c, RDSP_ALS_PEAK);
}
extern "C" int rdsp_sdr_setALSfilterAdaptive(rdsp_chain_t *c) {
  TO_ENGINE(c, rdsp_engine_setALSfilterAdaptive(c->engine));
  return RDSP_OK; /* the NLMS always adapts */
}
/* noise blanker (AudioSDR feature; arithmetic build-defined): wide-band,
 * before the mixer; windows of 256*decim input samples */
extern "C" int rdsp_sdr_enableNoiseBlanker(rdsp_chain_t *c) { NEED(c); TO_ENGINE(c, rdsp_engine_enableNoiseBlanker(c->engine)); c->nb_on = 1; return RDSP_OK; }
extern "C" int rdsp_sdr_disableNoiseBlanker(rdsp_chain_t *c) {
  TO_ENGINE(c, rdsp_engine_disableNoiseBlanker(c->engine));
  c->nb_on = 0;
  return RDSP_OK;
}
extern "C" int rdsp_sdr_setNoiseBlankerThresholdDb(rdsp_chain_t *c, float db) {
  NEED(c);
  if (!(db >= 0.0f && db <= 60.0f)) return chain_fail(RDSP_ERR_INVALID, "noise blanker threshold %g dB outside 0..60", (double)db);
  c->nb_threshold_db = db;
  return RDSP_OK;
}
/* AudioSDRpreProcessor (INO:117-118) */
extern "C" int rdsp_pre_swapIQ(rdsp_chain_t *c, int swap) {
  TO_ENGINE(c, rdsp_preproc_swapIQ(c->pre, swap));
  c->swap_iq = swap ? 1 : 0;
  return RDSP_OK;
}
/* INO:117 guards against a Teensy I2S bus fault that leaves one rail of the codec stream a sample
 * behind the other.  There is no bus here, so there is nothing to watch at run time; a RECORDING made
 * through such a front end carries the fault: rdsp_estimate_iq_slip finds it, rdsp_pre_setIQslip
 * corrects it. */
extern "C" int rdsp_pre_startAutoI2SerrorDetection(rdsp_chain_t *c) {
  TO_ENGINE(c, rdsp_preproc_startAutoI2SerrorDetection(c->pre));
  return RDSP_OK;
}
/* slip +1: pair I[n-1] with Q[n] (delay the I rail by one sample); -1: pair I[n] with Q[n-1]; 0: off.
 * Applies to samples as they arrive, from the next call on (what is already in the FIR history keeps
 * the pairing it came in with).  A set-up call: the first non-zero value allocates the corrected-input
 * buffer ([n_channels][max_blocks_per_call * 128] words). */
extern "C" int rdsp_pre_setIQslip(rdsp_chain_t *c, int slip) {
  NEED(c);
  if (slip < -1 || slip > 1) return RDSP_ERR_INVALID;
  if (slip != 0 && c->engine)
    return chain_fail(RDSP_ERR_UNSUPPORTED, "rdsp_pre_setIQslip: the chain is engine-literal; its pre-processor finds and repairs the slip itself "
                                            "(rdsp_pre_startAutoI2SerrorDetection)");
  if (slip != 0 && (!c->d_slip_buf || !c->d_slip_carry)) {
    RC_TRY(chain_check_device(c));
    if (!c->d_slip_buf) HIP_TRY(c->d_slip_buf.alloc((size_t)c->n_channels * (size_t)c->max_blocks * RDSP_BLOCK));
    RC_TRY(chain_planes_create(c, OPT_SLIP));
  }
  c->iq_slip = slip;
  return RDSP_OK;
}
extern "C" int rdsp_sdr_setInputGain(rdsp_chain_t *c, float g) {
  TO_ENGINE(c, rdsp_engine_setInputGain(c->engine, g));
  c->cfg.input_gain = g;
  return RDSP_OK;
}
extern "C" int rdsp_sdr_setOutputGain(rdsp_chain_t *c, float g) {
  TO_ENGINE(c, rdsp_engine_setOutputGain(c->engine, g));
  c->cfg.output_gain = g;
  return RDSP_OK;
}
extern "C" int rdsp_sdr_setIQgainBalance(rdsp_chain_t *c, float g) {
  TO_ENGINE(c, rdsp_engine_setIQgainBalance(c->engine, g));
  c->cfg.iq_balance = g;
  return RDSP_OK;
}
extern "C" int rdsp_sdr_enableAudioFilter(rdsp_chain_t *c) {
  TO_ENGINE(c, rdsp_engine_enableAudioFilter(c->engine)); /* the engine's audio filter, not the CONV stage's bFilterEnabled */
  c->cfg.filter_on = 1;
  for (size_t i = 0; i < c->groups.size(); i++) RC_TRY(chain_group_stage(c, (int)i));
  return RDSP_OK;
}
extern "C" int rdsp_sdr_setMute(rdsp_chain_t *c, int mute) {
  TO_ENGINE(c, rdsp_engine_setMute(c->engine, mute));
  c->cfg.mute = mute ? 1 : 0;
  return RDSP_OK;
}
extern "C" int rdsp_group_setTuningOffsetHz(rdsp_chain_t *c, int group, double hz) {
  if (chain_check_group(c, group) != RDSP_OK) return RDSP_ERR_INVALID;
  c->groups[(size_t)group].nco_hz = hz;
  c->groups[(size_t)group].dirty = true;
  if (group == 0) c->cfg.nco_hz = hz;
  return RDSP_OK;
}
extern "C" int rdsp_sdr_setTuningOffsetHz(rdsp_chain_t *c, double hz) {
  NEED(c);
  if (c->engine) return RDSP_OK; /* the engine moves the carrier from its own offset to 0 Hz itself (INO:139, CTL:447) */
  for (size_t i = 0; i < c->groups.size(); i++) (void)rdsp_group_setTuningOffsetHz(c, (int)i, hz);
  return RDSP_OK;
}
extern "C" int rdsp_set_nr_level(rdsp_chain_t *c, int lvl) { NEED(c); c->cfg.lms_nr = lvl; return RDSP_OK; }
extern "C" int rdsp_set_spectral_nr(rdsp_chain_t *c, int on, float level) {
  NEED(c);
  if (on < 0 || on > 2) return RDSP_ERR_INVALID;
  c->cfg.spectral_nr = on;
  c->cfg.spectral_level = level;
  return RDSP_OK;
}

/* How both NLMS instances keep arm_lms_norm_f32's window energy.  0 (default): the reference's running difference
 * (`energy -= x0 * x0; energy += in * in`, NR:73) re-started from the exact 96-sample window sum at every 128-sample
 * block -- a deliberate deviation: after a loud-to-quiet transition the reference's own recursion can leave energy +
 * 1.19e-7 <= 0 and lose the channel.  1: the reference's arithmetic, one running difference for the whole stream,
 * for hosts that want NR:73 as it is, residue and all. */
extern "C" int rdsp_set_nlms_energy_mode(rdsp_chain_t *c, int running) {
  NEED(c);
  c->nlms_energy_running = running ? 1 : 0;
  return RDSP_OK;
}
/* SPEC:226-235 writes the re-synthesis as mag' (arm_cos_f32(phi) + j arm_sin_f32(phi)), phi = atan2(im, re).  0
 * (default): the exact-arithmetic equivalent X mag'/mag; 1: as written, with CMSIS' table-interpolated sine and
 * cosine as published (the two are 1.7e-5 - 1.9e-5 of the peak apart: the table's own interpolation error) */
extern "C" int rdsp_set_spectral_resynthesis(rdsp_chain_t *c, int literal) {
  NEED(c);
  if (literal && !c->d_sin_table) {
    RC_TRY(chain_check_device(c));
    float tab[513];
    rdsp_arm_sin_table(tab);
    HIP_TRY(c->d_sin_table.alloc(513));
    HIP_TRY(hipMemcpy(c->d_sin_table, tab, sizeof(tab), hipMemcpyHostToDevice));
  }
  c->spectral_literal = literal == 2 ? 2 : (literal ? 1 : 0);
  return RDSP_OK;
}

/* ---- pipelined mode ---------------------------------------------------------------- */
int chain_drain_tail(rdsp_chain_t *c) {
  if (c->s_tail) HIP_TRY(hipStreamSynchronize(c->s_tail));
  return RDSP_OK;
}
int chain_drain_all(rdsp_chain_t *c, void *stream) {
  RC_TRY(chain_drain_tail(c));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  return RDSP_OK;
}
extern "C" int rdsp_chain_set_pipelined(rdsp_chain_t *c, int on) {
  NEED(c);
  RC_TRY(chain_check_device(c));
  RC_TRY(chain_drain_tail(c));
  if (on) { /* whatever an earlier call that failed half-way left out is made now */
    /* (a queue priority on this stream, hipStreamCreateWithPriority high or low, changes nothing: K3 1.168-1.192 /
     * 1.165-1.178 against 1.163-1.190 ms, K5 2.305-2.316 / 2.323-2.415 against 2.293-2.335; round 5, same box) */
    if (!c->ev_misc) HIP_TRY(c->ev_misc.create(hipEventDisableTiming)); /* first: where s_tail exists, ev_misc does */
    if (!c->s_tail) HIP_TRY(c->s_tail.create(hipStreamNonBlocking));
    if (!c->s_mid) HIP_TRY(c->s_mid.create(hipStreamNonBlocking));
    for (int i = 0; i < 3; i++) {
      if (!c->ev_mid[i]) HIP_TRY(c->ev_mid[i].create(hipEventDisableTiming));
      if (!c->ev_front[i]) HIP_TRY(c->ev_front[i].create(hipEventDisableTiming));
      if (!c->ev_tail[i]) HIP_TRY(c->ev_tail[i].create(hipEventDisableTiming));
    }
    for (auto &m : c->d_midx)
      if (!m) HIP_TRY(m.alloc(c->mid_stride * (size_t)c->n_channels));
  }
  c->pipe_on = on ? 1 : 0;
  c->call_idx = 0;
  c->tail_slot = -1; /* drained above */
  return on ? chain_ensure_sub_batch_events(c) : RDSP_OK;
}
int chain_sub_batches(const rdsp_chain_t *c) {
  if (c->sub_batch <= 0 || c->n_channels < c->sub_batch + c->sub_batch / 2) return 1;
  return (c->n_channels + c->sub_batch - 1) / c->sub_batch;
}
/* one event per channel sub-batch and intermediate buffer; made here and in
 * rdsp_chain_set_sub_batch, never on the streaming path */
int chain_ensure_sub_batch_events(rdsp_chain_t *c) {
  if (!c->s_tail) return RDSP_OK;
  const int nsb = chain_sub_batches(c);
  for (auto &evs : c->ev_front_sb)
    while (nsb > 1 && evs.size() < (size_t)nsb) HIP_TRY(push_event(evs, hipEventDisableTiming));
  return RDSP_OK;
}
/* front-kernel variant: -1 = auto (full-register; measured faster with and without the
 * concurrent tail stage), 0 = full-register, 1 = lean (FFT twiddles rebuilt per pass).  Both compute the same chain; they differ in the
 * rounding of the FFT twiddles (power chain vs direct), ~3e-7. */
extern "C" int rdsp_chain_set_front_variant(rdsp_chain_t *c, int lean) {
  NEED(c);
  if (lean < -1 || lean > 1) return RDSP_ERR_INVALID;
  c->lean_mode = lean;
  return RDSP_OK;
}
/* pipelined calls are launched in channel sub-batches of this size (a multiple of 64; 0 = one
 * launch per stage whatever the channel count).  Results do not depend on it. */
extern "C" int rdsp_chain_set_sub_batch(rdsp_chain_t *c, int channels) {
  NEED(c);
  if (channels < 0 || channels % 64 != 0) return RDSP_ERR_INVALID;
  RC_TRY(chain_check_device(c));
  c->sub_batch = channels;
  return chain_ensure_sub_batch_events(c);
}
/* wave priorities (s_setprio 0..3) used while the tail stage shares the SIMDs with the front
 * stage of the next call: the front kernel's during its FIR, the tail kernel's throughout */
extern "C" int rdsp_chain_set_priorities(rdsp_chain_t *c, int front_fir_prio, int tail_prio) {
  NEED(c);
  if (front_fir_prio < 0 || front_fir_prio > 3 || tail_prio < 0 || tail_prio > 3) return RDSP_ERR_INVALID;
  c->front_fir_prio = front_fir_prio;
  c->tail_prio = tail_prio;
  return RDSP_OK;
}
/* stage A3 of the front kernel (decim 4; decim-1 chains have no decimator and always run rdsp_front_kernel).
 * -1 (default): 4, or 5 for calls that no tail / SAM / IIR stage follows and that run without the blanker (rdsp_chain_process).
 * 4: in the frequency domain -- polyphase overlap-save: four low-rate transforms, branch
 * spectra, one inverse -- with frames of one granule (256 outputs; the rest of the 512-point window zeros): every
 * call boundary is a frame boundary and every frame's input is a function of the absolute sample position, so a
 * stream gives the same bits however it is cut into calls, like the reference's fixed 128-sample blocks
 * (CONV:231-245).  0: the direct form (packed FMAs), split-invariant too, ~1.3x slower.  2: the frequency domain
 * with 448-sample frames anchored at each call's first sample: 5 transforms per 448 outputs instead of per 256,
 * but a different call split frames and rounds differently (~3e-7): the throughput form, what bench.py selects.
 * 5: the frequency domain on 16-lane rows -- 256-point windows, four per wave, 128 outputs each (two frames per
 * granule): split-invariant like the default, ~10 % faster than it for chains without a tail stage (K2 0.727 against
 * 0.808 ms), no gain beside a tail kernel (250 registers); with the noise blanker on it runs the default form.
 * Same taps and the same exact linear convolution in all of them; the sums associate differently (~2e-7).
 * 1 and 3 (v_mfma GEMM slices; 3 unless the tail stage runs concurrently) and 6 (the row form with 192 outputs per
 * window, frames anchored at the call's first sample) were measured and not adopted (docs/history.md): unsupported. */
extern "C" int rdsp_chain_set_fir_variant(rdsp_chain_t *c, int variant) {
  NEED(c);
  if (variant < -1 || variant > 6) return RDSP_ERR_INVALID;
  if ((variant == 2 || variant >= 4) && !c->d_fd_mask)
    return chain_fail(RDSP_ERR_UNSUPPORTED, "the frequency-domain decimator needs decim = 4");
  if (variant == 1 || variant == 3)
    return chain_fail(RDSP_ERR_UNSUPPORTED, "the matrix-core FIR was measured and not adopted (docs/history.md)");
  if (variant == 6)
    return chain_fail(RDSP_ERR_UNSUPPORTED, "the row form with 192 outputs per window was measured and not adopted (docs/history.md)");
  c->fir_mode = variant;
  return RDSP_OK;
}
/* tail-kernel variant.  (16, 2) is the kernel there is (rdsp_tail.hip: a channel per 16-lane DPP row, two
 * steps per reduction).  Measured and not adopted (docs/history.md), unsupported: (16, 4) weights one block stale
 * with a hand-interleaved issue order, (16, 5) four steps per reduction (both round 3), (16, 3) one reduction per
 * step (round 1), (8, 2) half a row per channel, (16 | 8, 1) the reduction on the matrix pipe, (16, 0) the delay
 * line shifted by DPP. */
extern "C" int rdsp_chain_set_tail_variant(rdsp_chain_t *c, int lanes_per_channel, int matrix_reduce) {
  NEED(c);
  if ((lanes_per_channel != 8 && lanes_per_channel != 16) || (lanes_per_channel == 8 && !matrix_reduce) ||
      matrix_reduce < 0 || matrix_reduce > 5 || (lanes_per_channel == 8 && matrix_reduce > 2))
    return RDSP_ERR_INVALID;
  if (lanes_per_channel != 16 || matrix_reduce != 2) {
    rdsp_set_error("tail-kernel variants other than (16, 2) were measured and not adopted (docs/history.md)");
    return RDSP_ERR_UNSUPPORTED;
  }
  RC_TRY(chain_drain_tail(c));
  c->tail_lpc = 100;
  return RDSP_OK;
}
/* `stream` waits for every call issued so far (outputs complete after it) */
extern "C" int rdsp_chain_flush(rdsp_chain_t *c, void *stream) {
  NEED(c);
  RC_TRY(chain_check_device(c));
  if (c->tail_slot >= 0) HIP_TRY(hipStreamWaitEvent((hipStream_t)stream, c->ev_tail[c->tail_slot], 0));
  return RDSP_OK;
}

/* name of the front kernel the most recent rdsp_chain_process launched (as the profiler shows it,
 * without template arguments): rdsp_front_fd_kernel or rdsp_front_kernel */
extern "C" const char *rdsp_chain_front_kernel_name(const rdsp_chain_t *c) { return c ? c->front_name : ""; }

/* ---- per-kernel timing with HIP events on the launch stream -------------------- */
extern "C" int rdsp_chain_set_timing(rdsp_chain_t *c, int on) {
  NEED(c);
  RC_TRY(chain_check_device(c));
  const size_t kMaxCalls = 1024; /* calls beyond the pool are simply not timed */
  if (on && c->ev.size() < 4 * kMaxCalls) {
    while (c->ev.size() < 4 * kMaxCalls) HIP_TRY(push_event(c->ev, hipEventDefault));
    c->ev_has_tail.assign(kMaxCalls, 0);
  }
  c->ev_used = 0;
  c->timing_on = on ? 1 : 0;
  return RDSP_OK;
}
/* sums over the calls recorded since rdsp_chain_set_timing(c, 1) */
extern "C" int rdsp_chain_get_timing(rdsp_chain_t *c, double *front_ms, double *tail_ms, int *calls) {
  NEED(c);
  RC_TRY(chain_check_device(c));
  double f = 0.0, t = 0.0;
  const size_t n = c->ev_used;
  for (size_t i = 0; i < n; i++) {
    float a = 0.f, b = 0.f;
    HIP_TRY(hipEventSynchronize(c->ev[4 * i + 1]));
    HIP_TRY(hipEventElapsedTime(&a, c->ev[4 * i], c->ev[4 * i + 1]));
    f += a;
    if (c->ev_has_tail[i]) {
      HIP_TRY(hipEventSynchronize(c->ev[4 * i + 3]));
      HIP_TRY(hipEventElapsedTime(&b, c->ev[4 * i + 2], c->ev[4 * i + 3]));
      t += b;
    }
  }
  if (front_ms) *front_ms = f;
  if (tail_ms) *tail_ms = t;
  if (calls) *calls = (int)n;
  return RDSP_OK;
}

/* milliseconds from the end of the first recorded call's last kernel to the end of the last recorded call's:
 * (calls - 1) steady-state periods of a pipelined sequence, without the pipeline's fill (the first call's
 * front kernel has no tail kernel to overlap with) */
extern "C" int rdsp_chain_get_timing_span(rdsp_chain_t *c, double *span_ms, int *calls) {
  NEED(c);
  RC_TRY(chain_check_device(c));
  const size_t n = c->ev_used;
  float ms = 0.f;
  if (n >= 2) {
    hipEvent_t a = c->ev[4 * 0 + (c->ev_has_tail[0] ? 3 : 1)];
    hipEvent_t b = c->ev[4 * (n - 1) + (c->ev_has_tail[n - 1] ? 3 : 1)];
    HIP_TRY(hipEventSynchronize(b));
    HIP_TRY(hipEventElapsedTime(&ms, a, b));
  }
  if (span_ms) *span_ms = ms;
  if (calls) *calls = (int)n;
  return RDSP_OK;
}

/* ---- the sketch as shipped inside one chain (round 6) -----------------------------------------------------------------
 * A chain created as the bare CONV stage (decim 1, 44.1 kHz, RDSP_DEMOD_IQ, no mixer offset, unit gains, AGC / ALS /
 * spectral stage off: what loop() runs, INO:198) can take the reference's own pre-processor and engine in front of it:
 * rdsp_chain_process then is IQ -> AudioSDRpreProcessor::update -> AudioSDR::update -> doConvolutionalProcessing, and the
 * rdsp_sdr_* / rdsp_pre_* setters reach those objects (rdsp_engine_t, rdsp_preproc_t: the image's arithmetic, bit for bit)
 * instead of this build's stand-ins.  The engine's coefficient tables come from the host (rdsp_sdr_load_engine_tables). */
extern "C" int rdsp_sdr_set_engine_literal(rdsp_chain_t *c, int on) {
  NEED(c);
  if (!on) {
    if (c->engine) rdsp_engine_destroy(c->engine);
    if (c->pre) rdsp_preproc_destroy(c->pre);
    c->engine = nullptr;
    c->pre = nullptr;
    return RDSP_OK;
  }
  if (c->engine) return RDSP_OK;
  if (c->nb_on || c->swap_iq || c->iq_slip) /* after the switch these setters reach the engine's objects: nothing could turn the stand-ins off */
    return chain_fail(RDSP_ERR_UNSUPPORTED, "rdsp_sdr_set_engine_literal: the chain's own noise blanker (%d), swapIQ (%d) or I2S slip correction (%d) is "
                                            "on; turn it off first (rdsp_sdr_disableNoiseBlanker, rdsp_pre_swapIQ(0), rdsp_pre_setIQslip(0)) and make "
                                            "those calls again after the switch", c->nb_on, c->swap_iq, c->iq_slip);
  if (c->tail_law == RDSP_TAIL_ENGINE)
    return chain_fail(RDSP_ERR_UNSUPPORTED, "rdsp_sdr_set_engine_literal: the chain runs the engine-law tail (rdsp_chain_set_tail_law); switch it back first");
  const rdsp_chain_config_t &cf = c->cfg;
  if (c->decim != 1 || cf.fs_in != 44100.0 || cf.demod != RDSP_DEMOD_IQ || cf.nco_hz != 0.0 || cf.agc_mode != RDSP_AGC_OFF ||
      cf.als_mode != RDSP_ALS_OFF || cf.spectral_nr != 0 || cf.input_gain != 1.0f || cf.output_gain != 1.0f || cf.iq_balance != 1.0f ||
      c->groups.size() != 1)
    return chain_fail(RDSP_ERR_INVALID, "rdsp_sdr_set_engine_literal: the chain must be the bare CONV stage (decim 1, 44.1 kHz, RDSP_DEMOD_IQ, nco 0, "
                                        "AGC / ALS / spectral stage off, unit gains, one group)");
  RC_TRY(chain_check_device(c));
  int rc = rdsp_preproc_create(c->n_channels, c->device, &c->pre);
  if (rc == RDSP_OK) rc = rdsp_engine_create(c->n_channels, c->device, c->max_blocks, &c->engine);
  if (rc == RDSP_OK && !c->d_engine_io &&
      c->d_engine_io.alloc((size_t)c->n_channels * (size_t)c->max_blocks * RDSP_BLOCK * 2) != hipSuccess)
    rc = RDSP_ERR_NOMEM;
  if (rc != RDSP_OK) (void)rdsp_sdr_set_engine_literal(c, 0);
  return rc;
}
extern "C" int rdsp_sdr_load_engine_tables(rdsp_chain_t *c, const float *biquad_sets15x20, const float *hilbert64) {
  NEED(c);
  if (!c->engine)
    return chain_fail(RDSP_ERR_INVALID, "rdsp_sdr_load_engine_tables: rdsp_sdr_set_engine_literal(chain, 1) first");
  return rdsp_engine_load_tables(c->engine, biquad_sets15x20, hilbert64);
}
extern "C" rdsp_engine_t *rdsp_chain_engine(rdsp_chain_t *c) { return c ? c->engine : nullptr; }
extern "C" rdsp_preproc_t *rdsp_chain_preproc(rdsp_chain_t *c) { return c ? c->pre : nullptr; }
