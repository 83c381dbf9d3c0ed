/*
 * rdsp_engine_host.hip -- the host object behind rdsp_engine_t (include/rdsp.h): the sketch's settings and setters, and what
 * creates, destroys, resets and runs the object (rdsp_engine_host.h has the object and names the other host files).  The
 * signal path is rdsp_engine.hip's, the kernels are its stage files' (rdsp_engine_front / _hilbert / _tail.hip); a call hands rdsp_engine_launch (rdsp_engine_int.h) one group's
 * arguments.  Every device buffer has one owner (DevBuf): deleting the object frees them.
 * Compiled with the kernels' flags (-ffp-contract=off): the constants and tables computed here are held bit for bit. */
#include "rdsp_engine_host.h"

namespace {
constexpr size_t TAB_SETS = 0, TAB_HILBERT = 300, TAB_SINE = 364, TAB_CURVE = 621, TAB_WORDS = 751;

void engine_sam_constants(rdsp_engine_t *e) { /* 0xed34 with the constructor's loop parameters */
  const float wn = bits_f(0x3e50fac7), zeta = 2.0f, kd = 1.0f, ko = 1.0f;
  const double k4 = (double)(1.0f / (kd * ko)) * 4.0, den = 1.0 / ((double)zeta * 4.0) + (double)zeta;
  const float g1 = (float)((k4 * (double)zeta * (double)wn) / den), g2 = (float)((k4 * (double)wn * (double)wn) / (den * den));
  e->sam_ga = g1 + g2;
  e->sam_gb = g2;
}
void settings_agc_mode(EngSettings &s, int mode) { /* 0xdfe0 */
  if (mode == 0) { s.agc_on = 0; return; }
  if (mode < 0 || mode > 3) return; /* the engine ignores other values */
  s.agc = engine_agc_set(mode);
  s.agc_on = 1;
}
void settings_demod(const rdsp_engine_t *e, EngSettings &s, int mode) { /* 0xd798 */
  s.mode = mode & 0xffff;
  s.nfm = 0;
  switch (s.mode) {
    case RDSP_ENGINE_MODE_NFM: /* this build's own; without rdsp_engine_enable_fm a value the engine does not know */
      if (!e->fm) return;
      s.nfm = 1; s.tuning_offset = 0.0f; /* the station sits at DC */
      s.resets |= RESET_FM;
      return;
    case 0: s.tuning_offset = (float)((double)e->if_centre + (double)e->ssb_band * 0.5); s.pre_set = 12; break;
    case 1: s.tuning_offset = (float)((double)e->if_centre - (double)e->ssb_band * 0.5); s.pre_set = 12; break;
    case 6: s.tuning_offset = (float)((double)e->if_centre - (double)e->ssb_band * 0.5); s.pre_set = 11; break;
    case 2: s.tuning_offset = (float)((double)e->if_centre + (double)e->cw_band * 0.5); s.pre_set = 10; break;
    case 3: s.tuning_offset = (float)((double)e->if_centre - (double)e->cw_band * 0.5); s.pre_set = 10; break;
    case 4: case 5: s.tuning_offset = e->if_centre; s.pre_set = 14; break;
    default: return;
  }
  s.resets |= RESET_PRE; /* arm_biquad_cascade_df1_init_f32 clears the state */
}
EngSettings settings_as_constructed(const rdsp_engine_t *e) { /* AudioSDR::AudioSDR (0x6744) and its init (0xede4) */
  EngSettings s;
  memset(&s, 0, sizeof s);
  s.input_gain = s.gain_i = s.gain_q = s.iq_balance = s.output_gain = 1.0f;
  s.audio_set = 3; s.nb_on = 1; s.als_notch = 1; s.als_adaptive = 1;
  s.agc = engine_agc_set(0); /* 0xdf14: the medium attack with the slow decay and the fast hang time */
  s.agc_on = 1;
  s.meter.attack = rdsp_meter::ATTACK_DEFAULT; s.meter.decay = rdsp_meter::DECAY_DEFAULT; /* squelch off, thresholds and hang 0 */
  s.fm = {rdsp_fm::FM_DEFAULT_W, rdsp_fm::FM_DEFAULT_DEVIATION, rdsp_fm::FM_DEFAULT_TAU};
  s.tone = {rdsp_tone::TONE_DEFAULT_K, rdsp_tone::TONE_DEFAULT_ON, rdsp_tone::TONE_DEFAULT_OFF};
  s.search = {0, rdsp_tone_search::SEARCH_DEFAULT_MIN, rdsp_tone_search::SEARCH_DEFAULT_RATIO}; /* off */
  s.dcs = {rdsp_dcs::DCS_DEFAULT_K, rdsp_dcs::DCS_DEFAULT_ERR, rdsp_dcs::DCS_DEFAULT_ON, rdsp_dcs::DCS_DEFAULT_OFF};
  s.noise = {rdsp_noise::NOISE_OFF, rdsp_noise::NOISE_DEFAULT_OPEN, rdsp_noise::NOISE_DEFAULT_CLOSE, rdsp_noise::NOISE_DEFAULT_HANG,
             rdsp_noise::NOISE_DEFAULT_FALL, rdsp_noise::NOISE_DEFAULT_RISE}; /* off */
  s.dtmf = {0, rdsp_dtmf::DTMF_DEFAULT_MIN, rdsp_dtmf::DTMF_DEFAULT_RATIO, rdsp_dtmf::DTMF_DEFAULT_TWIST, rdsp_dtmf::DTMF_DEFAULT_SHARE,
            rdsp_dtmf::DTMF_DEFAULT_ON, rdsp_dtmf::DTMF_DEFAULT_OFF}; /* off */
  s.afsk = {0, rdsp_afsk::AFSK_DEFAULT_GAIN, rdsp_afsk::AFSK_DEFAULT_PULL, rdsp_afsk::AFSK_DEFAULT_MIN_BYTES}; /* off */
  s.pocsag = {0, rdsp_pocsag::POCSAG_DEFAULT_INVERT, rdsp_pocsag::POCSAG_DEFAULT_PULL, rdsp_pocsag::POCSAG_DEFAULT_SYNC_ERRS,
               rdsp_pocsag::POCSAG_DEFAULT_FIX_ADDR, rdsp_pocsag::POCSAG_DEFAULT_FIX_DATA}; /* off */
  settings_demod(e, s, 0);
  s.resets = 0;
  return s;
}
/* a call's arguments (the object's, the caller's rows and strides, n_blocks) for group g: its channel range and settings */
EngParams group_params(const rdsp_engine_t *e, size_t g, const EngParams &call) {
  const EngSettings &q = e->grp[g];
  const size_t c0 = (size_t)e->first[g];
  EngParams p = call;
  p.n_channels = range_end(e->first, g, e->n_channels) - e->first[g]; p.audio = e->d_audio + c0 * p.audio_stride;
  p.iq = call.iq + c0 * p.in_stride; p.out = call.out + c0 * p.out_stride;
  p.st = e->plane[PL_ST] + c0 * NF; p.nb = e->plane[PL_NB] + c0 * NB_WORDS; p.als = e->plane[PL_ALS] + c0 * ALS_WORDS;
  p.ring_i = e->plane[PL_RING_I] + c0 * e->ring_size; p.ring_q = e->plane[PL_RING_Q] + c0 * e->ring_size; p.pos = q.pos;
  p.mode = q.mode; p.mute = q.mute; p.audio_on = q.audio_on; p.agc_on = q.agc_on; p.als_notch = q.als_notch;
  p.als_adaptive = q.als_adaptive; p.resets = q.resets; p.pre_set = q.pre_set; p.audio_set = q.audio_set;
  p.gain_i = q.gain_i; p.gain_q = q.gain_q; p.output_gain = q.output_gain; p.tuning_offset = q.tuning_offset;
  p.agc = q.agc;
  return p;
}
}  // namespace

extern "C" {

int rdsp_engine_setAGCmode(rdsp_engine_t *e, int mode) { return for_selected(e, [&](EngSettings &s) { settings_agc_mode(s, mode); }); }
int rdsp_engine_enableAGC(rdsp_engine_t *e) { return for_selected(e, [](EngSettings &s) { s.agc_on = 1; }); } /* 0xdfd4 */
float rdsp_engine_setDemodMode(rdsp_engine_t *e, int mode) {
  if (!e) return 0.0f;
  (void)for_selected(e, [&](EngSettings &s) { settings_demod(e, s, mode); });
  return e->grp[e->sel < 0 ? 0 : (size_t)e->sel].tuning_offset;
}
int rdsp_engine_setAudioFilter(rdsp_engine_t *e, int id) { /* 0xd97c */
  static const int set_of_id[10] = {7, 8, 9, 0, 1, 2, 3, 4, 5, 6};
  return for_selected(e, [&](EngSettings &s) {
    if (id == 10) s.audio_on = 0;
    else if (id >= 0 && id < 10) { s.audio_set = set_of_id[id]; s.resets |= RESET_AUDIO; }
    s.audio_id = id;
  });
}
int rdsp_engine_enableAudioFilter(rdsp_engine_t *e) { return for_selected(e, [](EngSettings &s) { s.audio_on = 1; }); }
int rdsp_engine_setInputGain(rdsp_engine_t *e, float g) { /* 0xd8a0 */
  if (g > 10.0f) g = 10.0f;
  else if (g < 0.0f) g = 0.0f;
  return for_selected(e, [&](EngSettings &s) { s.input_gain = g; s.gain_i = s.iq_balance * g; s.gain_q = g; });
}
int rdsp_engine_setIQgainBalance(rdsp_engine_t *e, float b) { /* 0xd8f0 */
  return for_selected(e, [&](EngSettings &s) { s.iq_balance = b; s.gain_i = b * s.input_gain; s.gain_q = s.input_gain; });
}
int rdsp_engine_setOutputGain(rdsp_engine_t *e, float g) { return for_selected(e, [&](EngSettings &s) { s.output_gain = g; }); }
int rdsp_engine_setMute(rdsp_engine_t *e, int on) { return for_selected(e, [&](EngSettings &s) { s.mute = on ? 1 : 0; }); }
int rdsp_engine_enableALSfilter(rdsp_engine_t *e) { return for_selected(e, [](EngSettings &s) { s.als_on = 1; s.resets |= RESET_ALS; }); }
int rdsp_engine_disableALSfilter(rdsp_engine_t *e) { return for_selected(e, [](EngSettings &s) { s.als_on = 0; }); }
int rdsp_engine_setALSfilterNotch(rdsp_engine_t *e) { return for_selected(e, [](EngSettings &s) { s.als_notch = 1; }); }
int rdsp_engine_setALSfilterPeak(rdsp_engine_t *e) { return for_selected(e, [](EngSettings &s) { s.als_notch = 0; }); }
int rdsp_engine_setALSfilterAdaptive(rdsp_engine_t *e) { return for_selected(e, [](EngSettings &s) { s.als_adaptive = 1; }); }
int rdsp_engine_enableNoiseBlanker(rdsp_engine_t *e) { return for_selected(e, [](EngSettings &s) { s.nb_on = 1; }); }
int rdsp_engine_disableNoiseBlanker(rdsp_engine_t *e) { return for_selected(e, [](EngSettings &s) { s.nb_on = 0; }); }
int rdsp_engine_channels(const rdsp_engine_t *e) { return e ? e->n_channels : 0; }
int rdsp_engine_device(const rdsp_engine_t *e) { return e ? e->device : -1; }
int rdsp_engine_max_blocks(const rdsp_engine_t *e) { return e ? e->max_blocks : 0; }
const float *rdsp_engine_agc_curve(const rdsp_engine_t *e) { return e ? e->curve : nullptr; }
const float *rdsp_engine_sine_table(const rdsp_engine_t *e) { return e ? e->sine : nullptr; }

void rdsp_engine_destroy(rdsp_engine_t *e) {
  if (!e) return;
  (void)hipSetDevice(e->device);
  delete e;
}

/* device state as AudioSDR::AudioSDR (0x6744) + its init (0xede4) leave it: lines and filter states zero, the blanker's
 * mask lines 1.0, its running average 10.0, the PLL's frequency estimate 1890 Hz */
int rdsp_engine_reset(rdsp_engine_t *e, void *stream) {
  if (!e) return RDSP_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  hipError_t err = hipSetDevice(e->device);
  const size_t n = (size_t)e->n_channels;
  std::vector<float> fill[N_PLANES]; /* what a plane starts from; an empty one: zeros */
  fill[PL_ST].assign(n * NF, 0.0f); fill[PL_NB].assign(n * NB_WORDS, 0.0f);
  float *st = fill[PL_ST].data(), *nb = fill[PL_NB].data();
  for (size_t c = 0; c < n; c++) {
    st[c * NF + ST_SAM_HZ] = 1890.0f;
    st[c * NF + ST_NB_AVG] = 10.0f;
    st[c * NF + ST_AGC_ACTIVE] = bits_f(1u); /* the flag's value until the AGC first runs */
    for (int i = 0; i < 384; i++) nb[c * NB_WORDS + 768 + i] = 1.0f;
  }
  for (int k = 0; k < N_PLANES && err == hipSuccess; k++)
    err = fill[k].empty() ? hipMemsetAsync(e->plane[k], 0, n * e->plane_words[k] * 4, s)
                          : hipMemcpyAsync(e->plane[k], fill[k].data(), fill[k].size() * 4, hipMemcpyHostToDevice, s);
  if (err == hipSuccess && e->src) err = e->src->reset(s);
  if (err == hipSuccess && e->meter) err = e->meter->reset(s);
  if (err == hipSuccess && e->voice) err = e->voice->reset(s);
  if (err == hipSuccess && e->fm) err = e->fm->reset(s);
  if (err == hipSuccess && e->tone) err = e->tone->reset(s);
  if (err == hipSuccess && e->search) err = e->search->reset(s);
  if (err == hipSuccess && e->dcs) err = e->dcs->reset(s);
  if (err == hipSuccess && e->noise) err = e->noise->reset(s);
  if (err == hipSuccess && e->dtmf) err = e->dtmf->reset(s);
  if (err == hipSuccess && e->afsk) err = e->afsk->reset(s);
  if (err == hipSuccess && e->pocsag) err = e->pocsag->reset(s);
  if (err == hipSuccess) err = hipStreamSynchronize(s); /* the host vectors go away */
  for (auto &g : e->grp) { g.pos = 0; g.resets = 0; }
  e->event_blocks = 0; /* the decoders' words are zeros: the last call's records tell of nothing in them */
  return err == hipSuccess ? RDSP_OK : engine_fail("rdsp_engine_reset", err);
}

int rdsp_engine_create(int n_channels, int device, int max_blocks_per_call, rdsp_engine_t **out) {
  if (!out || n_channels < 1 || max_blocks_per_call < 1 || max_blocks_per_call > 4096) {
    rdsp_set_error("rdsp_engine_create: bad argument");
    return RDSP_ERR_INVALID;
  }
  *out = nullptr;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count < 1) {
    rdsp_set_error("rdsp_engine_create: no HIP device (this library has no CPU path)");
    return RDSP_ERR_NO_DEVICE;
  }
  if (device < 0 || device >= count || hipSetDevice(device) != hipSuccess) {
    rdsp_set_error("rdsp_engine_create: device %d of %d", device, count);
    return RDSP_ERR_INVALID;
  }
  rdsp_engine_t *e = new rdsp_engine();
  e->n_channels = n_channels; e->device = device; e->max_blocks = max_blocks_per_call;
  e->ring_size = 512;
  while (e->ring_size < (uint32_t)max_blocks_per_call * BS + 256u) e->ring_size <<= 1;
  e->tables = false;
  /* the constructor's values */
  e->if_centre = 6890.0f; e->ssb_band = 3000.0f; e->cw_band = 1000.0f;
  e->agc_threshold_db = ENGINE_AGC_THRESHOLD_DB; e->agc_slope = bits_f(ENGINE_AGC_SLOPE_BITS); e->agc_knee_db = ENGINE_AGC_KNEE_DB;
  engine_agc_curve(e->agc_threshold_db, e->agc_knee_db, e->agc_slope, e->curve);
  engine_sam_constants(e);
  for (int k = 0; k < 257; k++) e->sine[k] = (float)(round(sin(2.0 * 3.14159265358979323846 * k / 256.0) * 1e8) / 1e8);
  e->grp.assign(1, settings_as_constructed(e));
  e->first.assign(1, 0);
  const size_t n = (size_t)n_channels, words[N_PLANES] = {NF, e->ring_size, e->ring_size, NB_WORDS, ALS_WORDS};
  hipError_t err = hipSuccess;
  for (int k = 0; k < N_PLANES && err == hipSuccess; k++) err = e->plane[k].alloc(n * (e->plane_words[k] = words[k]));
  if (err == hipSuccess) err = e->d_audio.alloc(n * (size_t)max_blocks_per_call * BS);
  if (err == hipSuccess) err = e->d_tab.alloc(TAB_WORDS);
  if (err != hipSuccess) {
    rdsp_engine_destroy(e);
    rdsp_set_error("rdsp_engine_create: %s", hipGetErrorString(err));
    return RDSP_ERR_NOMEM;
  }
  const int rc = rdsp_engine_reset(e, nullptr);
  if (rc != RDSP_OK) { rdsp_engine_destroy(e); return rc; }
  *out = e;
  return RDSP_OK;
}

/* the engine's coefficient tables: fifteen sets of four {b0, b1, b2, a1, a2} sections in the image's order (ten audio
 * band-passes, then the IF filters: CW, mode 6, SSB, the AM detector's low-pass, AM) and the 64 taps of one side of the
 * Hilbert transformer, outermost first */
int rdsp_engine_load_tables(rdsp_engine_t *e, const float *biquad_sets15x20, const float *hilbert64) {
  if (!e || !biquad_sets15x20 || !hilbert64) return RDSP_ERR_INVALID;
  std::vector<float> t(TAB_WORDS);
  memcpy(&t[TAB_SETS], biquad_sets15x20, 300 * 4);
  memcpy(&t[TAB_HILBERT], hilbert64, 64 * 4);
  memcpy(&t[TAB_SINE], e->sine, 257 * 4);
  memcpy(&t[TAB_CURVE], e->curve, 130 * 4);
  hipError_t err = hipSetDevice(e->device);
  if (err == hipSuccess) err = hipMemcpy(e->d_tab, t.data(), TAB_WORDS * 4, hipMemcpyHostToDevice);
  if (err != hipSuccess) return engine_fail("rdsp_engine_load_tables", err);
  EngParams &p = e->base; /* rdsp_engine_update writes every other field */
  p.ring_size = e->ring_size; p.audio_stride = (size_t)e->max_blocks * BS; p.if_centre = e->if_centre;
  p.sets = e->d_tab + TAB_SETS; p.hilbert = e->d_tab + TAB_HILBERT; p.sine = e->d_tab + TAB_SINE; p.curve = e->d_tab + TAB_CURVE;
  p.nb_keep = 0.995f; p.nb_new = bits_f(0x3ba3d700); p.nb_ratio = 1.2f; p.nb_before = 10; p.nb_after = 10;
  p.sam_keep = 0.995f; p.sam_new = bits_f(0x3ba3d700); p.sam_hz_per_rad = bits_f(0x45db55dd); p.sam_lock_lo = 3890.0f; p.sam_lock_hi = 9890.0f;
  p.sam_ga = e->sam_ga; p.sam_gb = e->sam_gb;
  e->tables = true;
  return RDSP_OK;
}

/* AudioSDR::update (0xe730) for n_blocks consecutive 128-sample blocks of every channel.  d_iq: [ch][t] int16 pairs
 * (I, Q), in_stride pairs from one channel's row to the next; d_lr: [ch][t] int16 pairs, the engine's two outputs
 * (it transmits the same block on both, INO:81-86) */
int rdsp_engine_update(rdsp_engine_t *e, const int16_t *d_iq, size_t in_stride, int n_blocks, int16_t *d_lr, size_t out_stride, void *stream) {
  if (!e || !d_iq || !d_lr || n_blocks < 0 || n_blocks > e->max_blocks || in_stride < (size_t)n_blocks * BS || out_stride < (size_t)n_blocks * BS) {
    rdsp_set_error("rdsp_engine_update: bad argument (n_blocks %d of at most %d)", n_blocks, e ? e->max_blocks : 0);
    return RDSP_ERR_INVALID;
  }
  if (!e->tables) {
    rdsp_set_error("rdsp_engine_update: the engine's coefficient tables are not loaded (rdsp_engine_load_tables)");
    return RDSP_ERR_NOT_READY;
  }
  e->event_blocks = 0; /* until this call has run: rdsp_engine_gather_events counts nothing behind a call of no blocks or a failed one */
  if (n_blocks == 0) return RDSP_OK;
  hipStream_t s = (hipStream_t)stream;
  hipError_t err = hipSetDevice(e->device);
  if (err != hipSuccess) return engine_fail("rdsp_engine_update", err);
  EngParams call = e->base;
  call.iq = (const int32_t *)d_iq; call.in_stride = in_stride; call.out = (int32_t *)d_lr; call.out_stride = out_stride; call.n_blocks = n_blocks;
  if (e->fm) e->fm->nfm_rows.clear();
  if (e->tone) {
    e->tone->rows.clear();
    if ((err = e->tone->upload(e->tone_hz, s)) != hipSuccess) return engine_fail("rdsp_engine_update", err);
  }
  if (e->search) {
    e->search->rows.clear();
    if (e->search->stale && (err = e->search->upload(rdsp_engine_search_bank(e), s)) != hipSuccess) return engine_fail("rdsp_engine_update", err);
  }
  if (e->dcs) {
    e->dcs->rows.clear();
    if ((err = e->dcs->upload(e->dcs_codes, s)) != hipSuccess) return engine_fail("rdsp_engine_update", err);
  }
  if (e->noise) e->noise->rows.clear();
  if (e->dtmf) e->dtmf->rows.clear();
  if (e->afsk) e->afsk->rows.clear();
  if (e->pocsag) e->pocsag->rows.clear();
  for (size_t g = 0; g < e->grp.size(); g++) {
    EngSettings &q = e->grp[g];
    const EngParams p = group_params(e, g, call);
    const size_t c0 = (size_t)e->first[g];
    const bool nfm = e->fm && q.nfm; /* the detector in place of the front and Hilbert kernels, the tail on what it wrote */
    if (nfm) {
      err = e->fm->launch_group(p, c0, q.fm, d_iq, s);
      if (err == hipSuccess) { engine_launch_tail(p, q.als_on != 0, s); err = hipGetLastError(); }
    } else {
      err = rdsp_engine_launch(p, q.nb_on != 0, q.als_on != 0, s);
    }
    if (err == hipSuccess && e->meter) err = e->meter->launch_group(nfm ? e->fm->metered(p, c0) : p, c0, q.meter, d_lr, s); /* NFM: a carrier squelch */
    if (err == hipSuccess && e->noise && nfm) err = e->noise->launch_group(p, c0, q.noise, q.fm, e->meter.get(), d_lr, s); /* a noise squelch behind it */
    if (err == hipSuccess && e->tone && nfm) err = e->tone->launch_group(p, c0, q.tone, e->meter.get(), d_lr, s); /* and a tone squelch behind it */
    if (err == hipSuccess && e->search) /* the tone search reads the same rows; a group without a window keeps zero words */
      err = q.search.K == 0 ? e->search->clear_group(c0, (size_t)p.n_channels, s) : nfm ? e->search->launch_group(p, c0, q.search, s) : hipSuccess;
    if (err == hipSuccess && e->dcs && nfm) err = e->dcs->launch_group(p, c0, q.dcs, e->meter.get(), d_lr, s); /* and a code squelch behind both */
    if (err == hipSuccess && e->dtmf) /* the DTMF decoder reads the same rows; a group without a frame length keeps zero words */
      err = q.dtmf.K == 0 ? e->dtmf->clear_group(c0, (size_t)p.n_channels, s) : nfm ? e->dtmf->launch_group(p, c0, q.dtmf, s) : hipSuccess;
    if (err == hipSuccess && e->afsk && nfm) /* and the AFSK decoder behind it; an NFM group with it off keeps zero words */
      err = q.afsk.on == 0 ? e->afsk->clear_group(c0, (size_t)p.n_channels, s) : e->afsk->launch_group(p, c0, q.afsk, s);
    if (err == hipSuccess && e->pocsag && nfm) /* and the POCSAG decoder; an NFM group with baud 0 keeps zero words */
      err = q.pocsag.baud == 0 ? e->pocsag->clear_group(c0, (size_t)p.n_channels, s) : e->pocsag->launch_group(p, c0, q.pocsag, s);
    if (err != hipSuccess) return engine_fail("rdsp_engine_update launch", err);
    if (!nfm && (q.mode <= 3 || q.mode == 6)) q.pos = (q.pos + (uint32_t)n_blocks * BS) & (e->ring_size - 1); /* the lines only move when the SSB / CW path runs */
    q.resets = 0;
  }
  e->last_blocks = n_blocks;
  e->event_blocks = n_blocks;
  if (e->meter && (err = e->meter->launch_list(n_blocks, s)) != hipSuccess) return engine_fail("rdsp_engine_update launch", err);
  if (e->voice && (err = e->voice->launch(d_lr, out_stride, n_blocks, s)) != hipSuccess) return engine_fail("rdsp_engine_update launch", err);
  return RDSP_OK;
}

/* per-channel scalars for tests and monitoring: [n_channels][8] = oscillator phase, AGC gain, AGC envelope, hang counter,
 * AGC-active flag, PLL frequency estimate (Hz), PLL lock flag, blanker-hit flag */
int rdsp_engine_get_scalars(rdsp_engine_t *e, float *host_out, void *stream) {
  if (!e || !host_out) return RDSP_ERR_INVALID;
  std::vector<float> st((size_t)e->n_channels * NF);
  hipError_t err = hipSetDevice(e->device);
  if (err == hipSuccess) err = hipMemcpyAsync(st.data(), e->plane[PL_ST], st.size() * 4, hipMemcpyDeviceToHost, (hipStream_t)stream);
  if (err == hipSuccess) err = hipStreamSynchronize((hipStream_t)stream);
  if (err != hipSuccess) return engine_fail("rdsp_engine_get_scalars", err);
  for (int c = 0; c < e->n_channels; c++) {
    const float *s = &st[(size_t)c * NF];
    float *o = host_out + (size_t)c * 8;
    int hang, active, lock, hit;
    memcpy(&hang, &s[ST_AGC_HANG], 4); memcpy(&active, &s[ST_AGC_ACTIVE], 4); memcpy(&lock, &s[ST_SAM_LOCK], 4); memcpy(&hit, &s[ST_NB_HIT], 4);
    o[0] = s[ST_NCO]; o[1] = s[ST_AGC_GAIN]; o[2] = s[ST_AGC_ENV]; o[3] = (float)hang; o[4] = (float)active; o[5] = s[ST_SAM_HZ];
    o[6] = (float)lock; o[7] = (float)hit;
  }
  return RDSP_OK;
}

}  // extern "C"
