/*
 * rdsp_chain_select.hip -- what selects a receiver group's filter and demodulator, as the sketch does it: the
 * filter design entry points, pass bands, the audio-filter kind and its IIR coefficients, demodulator modes, PBT,
 * tuningMode.  Host settings: a group's new mask reaches the device through chain_group_stage (rdsp_chain_groups.hip)
 * alone, and nothing else here does but the IIR bank's first allocation.
 */
#include "rdsp_chain_int.h"

static uint32_t demod_tuning_offset(int demod) {
  /* `TuningOffset = SDR.setDemodMode(mode)` (INO:139, CTL:337-407): where the engine wants the carrier in the IQ stream.
   * AudioSDR is not in the tree, but it is in the reference's firmware image, and asked there (its constructor and
   * setDemodMode run under tests/golden/thumb_emu.py; tests/golden/firmware_kat.npz `engine_tuning_offset`) it answers
   * as a low-IF receiver: IF centre 6890 Hz, SSB band 3000 Hz, CW band 1000 Hz, the carrier at the centre plus (lower
   * side band) or minus (upper side band) half the band; AM / SAM at the centre.  (Until round 5: 700 Hz for the CW
   * modes and 0 otherwise, build-defined.)  The engine also oscillates at this frequency itself; here the mixer is a
   * setting of its own (rdsp_*_setTuningOffsetHz), so a host that mirrors the sketch hands the value on. */
  switch (demod) {
    case RDSP_DEMOD_LSB: return 8390u;
    case RDSP_DEMOD_USB: return 5390u;
    case RDSP_DEMOD_CW_LSB: return 7390u;
    case RDSP_DEMOD_CW_USB: return 6390u;
    case RDSP_DEMOD_AM:
    case RDSP_DEMOD_SAM: return 6890u;
    default: return 0u; /* RDSP_DEMOD_IQ: the literal CONV stage, no engine in front */
  }
}

static void group_design(rdsp_chain_t *c, GroupState &g) { /* CONV:209-224 without the upload */
  const double fs_out = c->cfg.fs_in / (double)c->decim;
  rdsp_calc_cplx_FIR_coeffs(g.coef_I.data(), g.coef_Q.data(), c->hop + 1, g.lo, g.hi, fs_out, c->cfg.window);
}

/* CONV:187-207 for one group: build the mask from whatever the tap arrays hold */
static int group_initialize(rdsp_chain_t *c, int gi) {
  GroupState &g = c->groups[(size_t)gi];
  if (rdsp_init_filter_mask(g.mask_nat.data(), g.coef_I.data(), g.coef_Q.data(), c->N) != 0)
    return chain_fail(RDSP_ERR_INVALID, "init_filter_mask failed");
  return chain_group_stage(c, gi);
}

extern "C" int rdsp_doConvolutionalInitialize(rdsp_chain_t *c, void *stream) {
  (void)stream; /* the new mask is switched in by the next processing call, in its stream's order */
  if (!c) return RDSP_ERR_INVALID;
  RC_TRY(chain_check_device(c));
  for (size_t i = 0; i < c->groups.size(); i++) RC_TRY(group_initialize(c, (int)i));
  return RDSP_OK;
}

/* CONV:209-224 for one group.  Host-side design, asynchronous upload into
 * the group's idle mask buffer; processing never waits on the host. */
extern "C" int rdsp_group_reInitializeFilter(rdsp_chain_t *c, int group, double lo, double hi, void *stream) {
  (void)stream;
  if (chain_check_group(c, group) != RDSP_OK) return RDSP_ERR_INVALID;
  RC_TRY(chain_check_device(c));
  GroupState &g = c->groups[(size_t)group];
  g.lo = lo;
  g.hi = hi;
  group_design(c, g);
  if (group == 0) { c->cfg.flo_hz = lo; c->cfg.fhi_hz = hi; }
  return group_initialize(c, group);
}

/* CONV:209-224: every group gets the same band */
extern "C" int rdsp_reInitializeFilter(rdsp_chain_t *c, double lo, double hi, void *stream) {
  if (!c) return RDSP_ERR_INVALID;
  for (size_t i = 0; i < c->groups.size(); i++) RC_TRY(rdsp_group_reInitializeFilter(c, (int)i, lo, hi, stream));
  return RDSP_OK;
}

static int engine_mode_of(int demod) { /* rdsp_demod_t -> the engine's numbering (as the compiled tuningMode() passes it) */
  switch (demod) {
    case RDSP_DEMOD_LSB: return 0; case RDSP_DEMOD_USB: return 1; case RDSP_DEMOD_CW_LSB: return 2; case RDSP_DEMOD_CW_USB: return 3;
    case RDSP_DEMOD_AM: return 4; case RDSP_DEMOD_SAM: return 5; default: return -1;
  }
}
static int engine_filter_of(int filter) { /* rdsp_audio_filter_t -> the engine's id (as the compiled filterMode() passes it) */
  switch (filter) {
    case RDSP_AUDIO_AM: return 0; case RDSP_AUDIO_CW: return 1; case RDSP_AUDIO_2100: return 3; case RDSP_AUDIO_2700: return 6;
    case RDSP_AUDIO_3100: return 8; default: return -1;
  }
}
/* pass bands per audio filter and mode (CTL:149-191 names; Appendix C of the
 * survey: 150 Hz .. 2.1/2.7/3.1/3.9 kHz; CW 500 Hz wide around the 700 Hz pitch) */
static void passband(int filter, int demod, double *lo, double *hi) {
  double a = 150.0, b = 2700.0;
  switch (filter) {
    case RDSP_AUDIO_CW: a = 450.0; b = 950.0; break;
    case RDSP_AUDIO_2100: b = 2100.0; break;
    case RDSP_AUDIO_2700: b = 2700.0; break;
    case RDSP_AUDIO_3100: b = 3100.0; break;
    case RDSP_AUDIO_AM: b = 3900.0; break;
    case RDSP_AUDIO_WSPR: a = 1400.0; b = 1600.0; break;
    default: break;
  }
  if (demod == RDSP_DEMOD_LSB || demod == RDSP_DEMOD_CW_LSB) { *lo = -b; *hi = -a; }
  else if (demod == RDSP_DEMOD_AM || demod == RDSP_DEMOD_SAM) { *lo = -b; *hi = b; }
  else { *lo = a; *hi = b; }
}
/* the group's pass band under the current implementation of the audio filter: the mask carries
 * it (MASK), or the mask only selects the side band (50 Hz ... 4 kHz on the demodulator's side;
 * both sides for AM / SAM) and the band-pass is the group's biquad cascade (IIR) */
static int group_apply_audio_filter(rdsp_chain_t *c, int group, void *stream) {
  GroupState &g = c->groups[(size_t)group];
  double lo, hi;
  passband(g.audio_filter, g.demod, &lo, &hi);
  if (c->audio_kind == RDSP_AUDIO_KIND_IIR) {
    const double a = fabs(lo) < fabs(hi) ? fabs(lo) : fabs(hi), b = fabs(lo) < fabs(hi) ? fabs(hi) : fabs(lo);
    const double f1 = (g.demod == RDSP_DEMOD_AM || g.demod == RDSP_DEMOD_SAM) ? 150.0 : a;
    rdsp_design_audio_iir(f1, b, c->cfg.fs_in / (double)c->decim, g.iir);
    g.iir_dirty = true;
    if (g.demod == RDSP_DEMOD_LSB || g.demod == RDSP_DEMOD_CW_LSB) { lo = -4000.0; hi = -50.0; }
    else if (g.demod == RDSP_DEMOD_AM || g.demod == RDSP_DEMOD_SAM) { lo = -4000.0; hi = 4000.0; }
    else { lo = 50.0; hi = 4000.0; }
  }
  return rdsp_group_reInitializeFilter(c, group, lo, hi, stream);
}
extern "C" int rdsp_group_setAudioFilter(rdsp_chain_t *c, int group, int filter, void *stream) {
  if (chain_check_group(c, group) != RDSP_OK) return RDSP_ERR_INVALID;
  if (filter < RDSP_AUDIO_CW || filter > RDSP_AUDIO_WSPR) return RDSP_ERR_INVALID;
  c->groups[(size_t)group].audio_filter = filter;
  return group_apply_audio_filter(c, group, stream);
}
/* which implementation SDR.setAudioFilter() selects filters of; re-applies every group's
 * current audio filter.  A control-path call: allocates the cascade's buffers on first use and
 * drains the tail stream (the cascade's state belongs to it). */
extern "C" int rdsp_sdr_setAudioFilterKind(rdsp_chain_t *c, int kind, void *stream) {
  NEED(c);
  if (kind != RDSP_AUDIO_KIND_MASK && kind != RDSP_AUDIO_KIND_IIR) return RDSP_ERR_INVALID;
  RC_TRY(chain_check_device(c));
  RC_TRY(chain_drain_tail(c));
  if (kind == RDSP_AUDIO_KIND_IIR) {
    const size_t ng = c->groups.size();
    RC_TRY(chain_planes_create(c, OPT_IIR));
    if (c->iir_sets < (int)ng) {
      HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
      c->iir_sets = 0;
      HIP_TRY(c->d_iir_coef.alloc(20 * ng));
      c->iir_sets = (int)ng;
      for (auto &g : c->groups) g.iir_dirty = true;
    }
  }
  c->audio_kind = kind;
  for (size_t i = 0; i < c->groups.size(); i++) RC_TRY(group_apply_audio_filter(c, (int)i, stream));
  return RDSP_OK;
}
/* An explicit cascade for the group's audio filter instead of the designed one -- e.g. one of the engine's own
 * coefficient sets (the reference's firmware image holds fifteen of them): coef20 = four sections
 * {b0, b1, b2, a1, a2} in arm_biquad_cascade_df1_f32 order (feedback terms added).  Needs RDSP_AUDIO_KIND_IIR; the
 * mask keeps the side-band selection it has; the next setAudioFilter / setDemodMode designs a cascade again.
 * The sections' state is kept (a coefficient change mid-stream, like the sketch's filter menu). */
extern "C" int rdsp_group_setAudioIIRCoefficients(rdsp_chain_t *c, int group, const float *coef20) {
  if (chain_check_group(c, group) != RDSP_OK || !coef20) return RDSP_ERR_INVALID;
  if (c->audio_kind != RDSP_AUDIO_KIND_IIR)
    return chain_fail(RDSP_ERR_UNSUPPORTED, "rdsp_group_setAudioIIRCoefficients: select RDSP_AUDIO_KIND_IIR first (rdsp_sdr_setAudioFilterKind)");
  for (int i = 0; i < 20; i++)
    if (!(coef20[i] == coef20[i]) || fabsf(coef20[i]) > 1e6f)
      return chain_fail(RDSP_ERR_INVALID, "rdsp_group_setAudioIIRCoefficients: coefficient %d is not a finite filter coefficient", i);
  GroupState &g = c->groups[(size_t)group];
  memcpy(g.iir, coef20, sizeof(g.iir));
  g.iir_dirty = true;
  return RDSP_OK;
}
extern "C" int rdsp_sdr_setAudioIIRCoefficients(rdsp_chain_t *c, const float *coef20) {
  NEED(c);
  for (size_t i = 0; i < c->groups.size(); i++) RC_TRY(rdsp_group_setAudioIIRCoefficients(c, (int)i, coef20));
  return RDSP_OK;
}
extern "C" int rdsp_chain_get_iir_coeffs(rdsp_chain_t *c, int group, float *out20) {
  if (chain_check_group(c, group) != RDSP_OK || !out20) return RDSP_ERR_INVALID;
  memcpy(out20, c->groups[(size_t)group].iir, sizeof(float) * 20);
  return RDSP_OK;
}
extern "C" int rdsp_sdr_setAudioFilter(rdsp_chain_t *c, int filter, void *stream) {
  NEED(c);
  if (c->engine) {
    const int id = engine_filter_of(filter);
    if (id < 0) return chain_fail(RDSP_ERR_INVALID, "rdsp_sdr_setAudioFilter: no engine filter id known for %d", filter);
    return rdsp_engine_setAudioFilter(c->engine, id);
  }
  for (size_t i = 0; i < c->groups.size(); i++) RC_TRY(rdsp_group_setAudioFilter(c, (int)i, filter, stream));
  return RDSP_OK;
}
extern "C" uint32_t rdsp_group_setDemodMode(rdsp_chain_t *c, int group, int mode, void *stream) {
  if (chain_check_group(c, group) != RDSP_OK || mode < RDSP_DEMOD_IQ || mode > RDSP_DEMOD_SAM) return 0;
  GroupState &g = c->groups[(size_t)group];
  if (mode == RDSP_DEMOD_SAM && chain_ensure_sam(c) != RDSP_OK) return 0;
  g.demod = mode;
  if (group == 0) c->cfg.demod = mode;
  (void)group_apply_audio_filter(c, group, stream);
  return demod_tuning_offset(mode);
}
extern "C" uint32_t rdsp_sdr_setDemodMode(rdsp_chain_t *c, int mode, void *stream) {
  if (!c || mode < RDSP_DEMOD_IQ || mode > RDSP_DEMOD_SAM) return 0;
  if (c->engine) return engine_mode_of(mode) < 0 ? 0u : (uint32_t)rdsp_engine_setDemodMode(c->engine, engine_mode_of(mode));
  for (size_t i = 0; i < c->groups.size(); i++) (void)rdsp_group_setDemodMode(c, (int)i, mode, stream);
  return demod_tuning_offset(mode);
}

/* checkPBT_Increase / checkPBT_Decrease (CTL:569-612) on a pair of cut-offs:
 * edge 0 = LOCUT (button D3), 1 = HICUT (D6); dir +1 / -1; 50 Hz steps inside
 * [MIN_LOW, MAX_LOW] and [MIN_HI, MAX_HI] (RDSP_general_includes.h:79-82), with the
 * reference's comparisons (<= when increasing, > when decreasing). */
extern "C" int rdsp_pbt_step(double *lo, double *hi, int edge, int dir) {
  if (!lo || !hi || (edge != 0 && edge != 1) || (dir != 1 && dir != -1)) return RDSP_ERR_INVALID;
  const double MIN_LOW = 0.0, MAX_LOW = 700.0, MIN_HI = 800.0, MAX_HI = 4000.0;
  if (dir > 0) {
    if (edge == 0) *lo = (*lo + 50) <= MAX_LOW ? (*lo + 50) : *lo; /* CTL:574 */
    else *hi = (*hi + 50) <= MAX_HI ? (*hi + 50) : *hi;            /* CTL:581 */
  } else {
    if (edge == 0) {
      *lo = (*lo - 50) > MIN_LOW ? (*lo - 50) : *lo; /* CTL:595 */
      if (*lo < 0.0) *lo = 0.0;                      /* CTL:596 */
    } else {
      *hi = (*hi - 50) > MIN_HI ? (*hi - 50) : *hi;  /* CTL:604 */
    }
  }
  return RDSP_OK;
}
extern "C" int rdsp_group_pbt(rdsp_chain_t *c, int group, int edge, int dir, void *stream) {
  if (chain_check_group(c, group) != RDSP_OK) return RDSP_ERR_INVALID;
  GroupState &g = c->groups[(size_t)group];
  double lo = g.lo, hi = g.hi;
  RC_TRY(rdsp_pbt_step(&lo, &hi, edge, dir));
  return rdsp_group_reInitializeFilter(c, group, lo, hi, stream); /* CTL:575,582,597,605 */
}

/* tuningMode() (CTL:330-423): the mode table of the sketch.  mndx 0 "CW N" (500 Hz),
 * 1 "CW" (2.1 kHz), 2 "USB", 3 "LSB", 4 "AM", 5 "SAM", 6 "RTTY"; CW side chosen by
 * vfoFreq > 10 MHz (CTL:337,349).  Returns TuningOffset. */
extern "C" uint32_t rdsp_group_tuningMode(rdsp_chain_t *c, int group, int mndx, double vfo_hz, void *stream) {
  if (chain_check_group(c, group) != RDSP_OK) return 0;
  int filter, mode;
  switch (mndx) {
    case 0: filter = RDSP_AUDIO_CW; mode = vfo_hz > 10000000.0 ? RDSP_DEMOD_CW_USB : RDSP_DEMOD_CW_LSB; break;
    case 1: filter = RDSP_AUDIO_2100; mode = vfo_hz > 10000000.0 ? RDSP_DEMOD_CW_USB : RDSP_DEMOD_CW_LSB; break;
    case 2: filter = RDSP_AUDIO_2700; mode = RDSP_DEMOD_USB; break;
    case 3: filter = RDSP_AUDIO_2700; mode = RDSP_DEMOD_LSB; break;
    case 4: filter = RDSP_AUDIO_AM; mode = RDSP_DEMOD_AM; break;
    case 5: filter = RDSP_AUDIO_AM; mode = RDSP_DEMOD_SAM; break;
    case 6: filter = RDSP_AUDIO_2100; mode = RDSP_DEMOD_USB; break;
    default: rdsp_set_error("tuningMode: no menu entry %d (CTL:330-423 has 0..6)", mndx); return 0;
  }
  c->groups[(size_t)group].audio_filter = filter;      /* SDR.setAudioFilter(...) */
  return rdsp_group_setDemodMode(c, group, mode, stream); /* TuningOffset = SDR.setDemodMode(...) */
}
