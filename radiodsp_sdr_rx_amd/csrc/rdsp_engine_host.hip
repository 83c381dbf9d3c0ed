/*
 * rdsp_engine_host.hip -- the host object behind rdsp_engine_t (include/rdsp.h): the sketch's settings, receiver groups, the
 * signal state as a blob, and every rdsp_engine_* entry point.  The kernels and the signal path are rdsp_engine.hip's; a call
 * hands rdsp_engine_launch (rdsp_engine_int.h) one group's arguments.  Receivers on shared IQ sources are the front end's
 * (rdsp_engine_sources.h): the entry points here check their arguments and make one call into it.  Every device buffer has
 * one owner (DevBuf): deleting the object frees them.
 * Compiled with the kernels' flags (-ffp-contract=off): the constants and tables computed here are held bit for bit. */
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <memory>
#include <vector>

#include "rdsp_engine_int.h"
#include "rdsp_engine_laws.h"
#include "rdsp_engine_meter.h"
#include "rdsp_engine_sources.h"

using namespace rdsp_eng;

/* what the sketch's calls set: one set per receiver group (one group = the whole object unless rdsp_engine_set_groups cut it) */
struct EngSettings {
  float input_gain, gain_i, gain_q, iq_balance, output_gain, tuning_offset;
  int mode, mute, audio_on, audio_id, audio_set, pre_set, agc_on, als_on, als_notch, als_adaptive, nb_on, resets;
  EngineAgcSet agc;
  rdsp_meter::MeterSet meter; /* rdsp_engine_set_meter / set_squelch: in force once rdsp_engine_enable_meter was called */
  uint32_t pos; /* where the group's next sample goes in its channels' rings (they only move in the SSB / CW modes) */
};
/* the planes of a channel's signal state: create allocates them, reset fills them, save_state / load_state move them */
enum { PL_ST, PL_RING_I, PL_RING_Q, PL_NB, PL_ALS, N_PLANES };
/* what rdsp_engine_enable_meter allocates: every channel's meter words, the last call's records [ch][max_blocks], its list */
struct EngMeter {
  DevBuf<float> words, level, peak;
  DevBuf<uint8_t> open;
  DevBuf<int32_t> list, count;
  int blocks = 0; /* of the last call that left records */
};
struct rdsp_engine {
  int n_channels, device, max_blocks;
  uint32_t ring_size;
  bool tables;
  DevBuf<float> plane[N_PLANES], d_audio, d_tab;
  size_t plane_words[N_PLANES]; /* per channel */
  EngParams base;               /* the kernels' arguments that belong to the object (rdsp_engine_load_tables) */
  float curve[130], sine[257];
  /* constants of the object (docs/engine.md has their places in the image's AudioSDR) */
  float if_centre, ssb_band, cw_band, agc_knee_db, agc_slope, agc_threshold_db, sam_ga, sam_gb;
  std::vector<EngSettings> grp; /* at least one */
  std::vector<int> first;       /* first channel of each group, ascending; first[0] = 0 */
  int sel = -1;                 /* the group the setters address; -1: all of them */
  /* shared IQ streams (rdsp_engine_set_sources / tune / update_sources): the front end, from the first set_sources on */
  std::unique_ptr<EngFrontEnd> src;
  std::unique_ptr<EngMeter> meter; /* the signal meter, from rdsp_engine_enable_meter on */
  int last_blocks = 0;             /* of the last call that ran: what rdsp_engine_read_demod may ask for */
  std::vector<double> station; /* per channel, Hz from its stream's centre (0 until tuned): a setting that may precede the sources */
};

namespace {
constexpr size_t TAB_SETS = 0, TAB_HILBERT = 300, TAB_SINE = 364, TAB_CURVE = 621, TAB_WORDS = 751;

void engine_sam_constants(rdsp_engine_t *e) { /* 0xed34 with the constructor's loop parameters */
  const float wn = bits_f(0x3e50fac7), zeta = 2.0f, kd = 1.0f, ko = 1.0f;
  const double k4 = (double)(1.0f / (kd * ko)) * 4.0, den = 1.0 / ((double)zeta * 4.0) + (double)zeta;
  const float g1 = (float)((k4 * (double)zeta * (double)wn) / den), g2 = (float)((k4 * (double)wn * (double)wn) / (den * den));
  e->sam_ga = g1 + g2;
  e->sam_gb = g2;
}
/* the stream of source rows; an engine without sources answers as one at 44 100 Hz on int16 rows */
SourceStream source_stream(const rdsp_engine_t *e) { return e && e->src ? e->src->st : SourceStream(); }
/* the setters address the selected group, or all of them */
template <typename F>
int for_selected(rdsp_engine_t *e, F f) {
  if (!e) return RDSP_ERR_INVALID;
  for (size_t g = 0; g < e->grp.size(); g++)
    if (e->sel < 0 || (size_t)e->sel == g) f(e->grp[g]);
  return RDSP_OK;
}
void settings_agc_mode(EngSettings &s, int mode) { /* 0xdfe0 */
  if (mode == 0) { s.agc_on = 0; return; }
  if (mode < 0 || mode > 3) return; /* the engine ignores other values */
  s.agc = engine_agc_set(mode);
  s.agc_on = 1;
}
void settings_demod(const rdsp_engine_t *e, EngSettings &s, int mode) { /* 0xd798 */
  s.mode = mode & 0xffff;
  switch (s.mode) {
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
  settings_demod(e, s, 0);
  s.resets = 0;
  return s;
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

/* Receiver groups: the sketch has ONE receiver, so one mode, one audio filter, one AGC setting; an object of many channels
 * can be cut into groups of consecutive channels that each carry their own.  first_channel[g] is group g's first channel
 * (ascending, first_channel[0] = 0); new groups start as copies of the group their first channel was in.  The setters
 * address the group chosen with rdsp_engine_select_group (-1, the default: every group).  A call of rdsp_engine_update
 * launches each group's kernels on its channel range; the signal state of a channel does not care which group it is in.
 * The side-band lines are rings written at the group's position `pos`, which only moves while the group runs SSB / CW, so
 * two groups' positions differ once one of them spent blocks in AM / SAM: a channel whose group's position changes has its
 * rings rotated by the difference (one strided copy per run of channels that share old and new group, through a scratch
 * buffer), after everything queued on the device has finished.  Pending resets (a setDemodMode / setAudioFilter /
 * enableALSfilter not yet followed by an update) are settings of the group too: a new group whose channels come from
 * old groups with different ones is refused, since only one of them could be kept. */
namespace {
int group_of(const std::vector<int> &first, int ch) {
  size_t g = 0;
  while (g + 1 < first.size() && first[g + 1] <= ch) g++;
  return (int)g;
}
/* where range g of `first` ends: the channels of group g are first[g] .. range_end(first, g, n_channels) - 1 */
int range_end(const std::vector<int> &first, size_t g, int n_channels) { return g + 1 < first.size() ? first[g + 1] : n_channels; }
/* new[(i + d) & (R - 1)] = old[i] for channels c0 .. c0 + n - 1 of one ring */
hipError_t rotate_rings(float *ring, float *scratch, size_t R, size_t c0, size_t n, uint32_t d) {
  float *base = ring + c0 * R;
  hipError_t err = hipMemcpyAsync(scratch, base, n * R * 4, hipMemcpyDeviceToDevice, nullptr);
  if (err == hipSuccess) err = hipMemcpy2DAsync(base + d, R * 4, scratch, R * 4, (R - d) * 4, n, hipMemcpyDeviceToDevice, nullptr);
  if (err == hipSuccess) err = hipMemcpy2DAsync(base, R * 4, scratch + (R - d), R * 4, (size_t)d * 4, n, hipMemcpyDeviceToDevice, nullptr);
  if (err == hipSuccess) err = hipStreamSynchronize(nullptr); /* the scratch buffer is reused by the next run */
  return err;
}
}  // namespace
int rdsp_engine_set_groups(rdsp_engine_t *e, int n_groups, const int *first_channel) {
  if (!e || n_groups < 1 || !first_channel || first_channel[0] != 0) return RDSP_ERR_INVALID;
  for (int g = 1; g < n_groups; g++)
    if (first_channel[g] <= first_channel[g - 1] || first_channel[g] >= e->n_channels) return RDSP_ERR_INVALID;
  std::vector<EngSettings> grp((size_t)n_groups);
  for (int g = 0; g < n_groups; g++) grp[(size_t)g] = e->grp[(size_t)group_of(e->first, first_channel[g])];
  /* runs of channels with the same old and new group: ranges of run_first */
  const std::vector<int> nf(first_channel, first_channel + n_groups);
  std::vector<int> run_first(e->first);
  run_first.insert(run_first.end(), nf.begin(), nf.end());
  std::sort(run_first.begin(), run_first.end());
  run_first.erase(std::unique(run_first.begin(), run_first.end()), run_first.end());
  size_t widest = 0;
  for (size_t k = 0; k < run_first.size(); k++) {
    const int r1 = range_end(run_first, k, e->n_channels);
    const EngSettings &was = e->grp[(size_t)group_of(e->first, run_first[k])], &now = grp[(size_t)group_of(nf, run_first[k])];
    if (was.resets != now.resets) {
      rdsp_set_error("rdsp_engine_set_groups: channels %d..%d have other resets pending (setDemodMode / setAudioFilter / "
                     "enableALSfilter since the last update) than the group they would join; call rdsp_engine_update first",
                     run_first[k], r1 - 1);
      return RDSP_ERR_UNSUPPORTED;
    }
    if (was.pos != now.pos) widest = std::max(widest, (size_t)(r1 - run_first[k]));
  }
  if (widest > 0) {
    const size_t R = e->ring_size, chunk = std::min(widest, std::max((size_t)1, ((size_t)64 << 20) / (R * 4)));
    DevBuf<float> scratch;
    hipError_t err = hipSetDevice(e->device);
    if (err == hipSuccess) err = hipDeviceSynchronize(); /* every stream's queued updates have written the rings */
    if (err == hipSuccess) err = scratch.alloc(chunk * R);
    for (size_t k = 0; err == hipSuccess && k < run_first.size(); k++) {
      const size_t r1 = (size_t)range_end(run_first, k, e->n_channels);
      const uint32_t d = (grp[(size_t)group_of(nf, run_first[k])].pos - e->grp[(size_t)group_of(e->first, run_first[k])].pos) & (uint32_t)(R - 1);
      for (size_t c = (size_t)run_first[k]; d != 0 && err == hipSuccess && c < r1; c += chunk) {
        const size_t n = std::min(chunk, r1 - c);
        err = rotate_rings(e->plane[PL_RING_I], scratch, R, c, n, d);
        if (err == hipSuccess) err = rotate_rings(e->plane[PL_RING_Q], scratch, R, c, n, d);
      }
    }
    if (err != hipSuccess) return engine_fail("rdsp_engine_set_groups", err);
  }
  e->grp.swap(grp);
  e->first.assign(first_channel, first_channel + n_groups);
  e->sel = -1;
  if (e->src) e->src->steps_changed(); /* a channel's step follows its new group's mode */
  return RDSP_OK;
}
int rdsp_engine_groups(const rdsp_engine_t *e) { return e ? (int)e->grp.size() : 0; }
int rdsp_engine_select_group(rdsp_engine_t *e, int group) {
  if (!e || group < -1 || group >= (int)e->grp.size()) return RDSP_ERR_INVALID;
  e->sel = group;
  return RDSP_OK;
}

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
  if (err == hipSuccess && e->meter) err = hipMemsetAsync(e->meter->words, 0, n * MT_WORDS * 4, s); /* level 0, gate closed, hang 0 */
  if (err == hipSuccess) err = hipStreamSynchronize(s); /* the host vectors go away */
  for (auto &g : e->grp) { g.pos = 0; g.resets = 0; }
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
  if (n_blocks == 0) return RDSP_OK;
  hipStream_t s = (hipStream_t)stream;
  hipError_t err = hipSetDevice(e->device);
  if (err != hipSuccess) return engine_fail("rdsp_engine_update", err);
  EngParams p = e->base;
  p.in_stride = in_stride; p.out_stride = out_stride; p.n_blocks = n_blocks;
  for (size_t g = 0; g < e->grp.size(); g++) {
    EngSettings &q = e->grp[g];
    const size_t c0 = (size_t)e->first[g];
    p.n_channels = range_end(e->first, g, e->n_channels) - e->first[g]; p.audio = e->d_audio + c0 * p.audio_stride;
    p.iq = (const int32_t *)d_iq + c0 * in_stride; p.out = (int32_t *)d_lr + c0 * out_stride;
    p.st = e->plane[PL_ST] + c0 * NF; p.nb = e->plane[PL_NB] + c0 * NB_WORDS; p.als = e->plane[PL_ALS] + c0 * ALS_WORDS;
    p.ring_i = e->plane[PL_RING_I] + c0 * e->ring_size; p.ring_q = e->plane[PL_RING_Q] + c0 * e->ring_size; p.pos = q.pos;
    p.mode = q.mode; p.mute = q.mute; p.audio_on = q.audio_on; p.agc_on = q.agc_on; p.als_notch = q.als_notch;
    p.als_adaptive = q.als_adaptive; p.resets = q.resets; p.pre_set = q.pre_set; p.audio_set = q.audio_set;
    p.gain_i = q.gain_i; p.gain_q = q.gain_q; p.output_gain = q.output_gain; p.tuning_offset = q.tuning_offset;
    p.agc = q.agc;
    err = rdsp_engine_launch(p, q.nb_on != 0, q.als_on != 0, s);
    if (err == hipSuccess && e->meter) { /* behind the group's tail kernel: it measures p.audio and gates p.out */
      const EngMeter &m = *e->meter;
      MeterParams mp;
      mp.audio = p.audio; mp.audio_stride = p.audio_stride; mp.out = p.out; mp.out_stride = out_stride;
      mp.out_vec = ((uintptr_t)d_lr & 15) == 0 && out_stride % 4 == 0;
      mp.n_channels = p.n_channels; mp.n_blocks = n_blocks; mp.words = m.words + c0 * MT_WORDS;
      mp.rec_stride = (size_t)e->max_blocks;
      mp.level = m.level + c0 * mp.rec_stride; mp.peak = m.peak + c0 * mp.rec_stride; mp.open = m.open + c0 * mp.rec_stride;
      mp.set = q.meter;
      err = rdsp_engine_meter_launch(mp, s);
    }
    if (err != hipSuccess) return engine_fail("rdsp_engine_update launch", err);
    if (q.mode <= 3 || q.mode == 6) q.pos = (q.pos + (uint32_t)n_blocks * BS) & (e->ring_size - 1); /* the lines only move when the SSB / CW path runs */
    q.resets = 0;
  }
  e->last_blocks = n_blocks;
  if (e->meter) {
    e->meter->blocks = n_blocks;
    err = rdsp_engine_active_launch(ActiveParams{e->meter->words, e->n_channels, e->meter->list, e->meter->count}, s);
    if (err != hipSuccess) return engine_fail("rdsp_engine_update launch", err);
  }
  return RDSP_OK;
}

/* ---- the signal meter, the squelch and the active-receiver list (include/rdsp.h has the definition; the kernels are
 * rdsp_engine_meter.hip's, the arithmetic rdsp_meter.h's) ----------------------------------------------------------------- */
namespace {
bool no_meter(const rdsp_engine_t *e, const char *who) {
  if (!e->meter) rdsp_set_error("%s: the meter is off; call rdsp_engine_enable_meter first", who);
  return !e->meter;
}
/* n_blocks of the last call's max_blocks-wide rows into the caller's rows, stream-ordered; a NULL destination is skipped */
hipError_t copy_rows(void *dst, size_t dst_stride, const void *src, size_t src_stride, size_t width, size_t rows, size_t size, hipStream_t s) {
  if (!dst || width == 0) return hipSuccess;
  return hipMemcpy2DAsync(dst, dst_stride * size, src, src_stride * size, width * size, rows, hipMemcpyDeviceToDevice, s);
}
}  // namespace

int rdsp_engine_enable_meter(rdsp_engine_t *e) {
  if (!e) return RDSP_ERR_INVALID;
  if (e->meter) return RDSP_OK;
  const size_t n = (size_t)e->n_channels, rec = n * (size_t)e->max_blocks;
  auto m = std::make_unique<EngMeter>(); /* the object stays without a meter unless all of it exists */
  hipError_t err = hipSetDevice(e->device);
  if (err == hipSuccess) err = hipDeviceSynchronize(); /* the next call of every stream runs with the meter */
  if (err == hipSuccess) err = m->words.alloc(n * MT_WORDS);
  if (err == hipSuccess) err = m->level.alloc(rec);
  if (err == hipSuccess) err = m->peak.alloc(rec);
  if (err == hipSuccess) err = m->open.alloc(rec);
  if (err == hipSuccess) err = m->list.alloc(n);
  if (err == hipSuccess) err = m->count.alloc(1);
  if (err == hipSuccess) err = hipMemset(m->words, 0, n * MT_WORDS * 4);
  if (err == hipSuccess) err = hipMemset(m->level, 0, rec * 4);
  if (err == hipSuccess) err = hipMemset(m->peak, 0, rec * 4);
  if (err == hipSuccess) err = hipMemset(m->open, 0, rec);
  if (err == hipSuccess) err = hipMemset(m->list, 0, n * 4);
  if (err == hipSuccess) err = hipMemset(m->count, 0, 4);
  if (err == hipSuccess) err = hipDeviceSynchronize();
  if (err != hipSuccess) {
    rdsp_set_error("rdsp_engine_enable_meter: %s", hipGetErrorString(err));
    return RDSP_ERR_NOMEM;
  }
  e->meter = std::move(m);
  return RDSP_OK;
}
int rdsp_engine_meter_enabled(const rdsp_engine_t *e) { return e && e->meter ? 1 : 0; }

int rdsp_engine_set_meter(rdsp_engine_t *e, float attack, float decay) {
  if (!e || !rdsp_meter::coefficients_ok(attack, decay)) {
    rdsp_set_error("rdsp_engine_set_meter: bad argument (attack %g and decay %g must lie in (0, 1])", (double)attack, (double)decay);
    return RDSP_ERR_INVALID;
  }
  return for_selected(e, [&](EngSettings &s) { s.meter.attack = attack; s.meter.decay = decay; });
}
int rdsp_engine_set_squelch(rdsp_engine_t *e, float open_ms, float close_ms, int hang_blocks) {
  if (!e || !rdsp_meter::squelch_ok(open_ms, close_ms, hang_blocks)) {
    rdsp_set_error("rdsp_engine_set_squelch: bad argument (0 <= close_ms %g <= open_ms %g, both finite; hang_blocks %d of 0 .. %d)",
                   (double)close_ms, (double)open_ms, hang_blocks, rdsp_meter::HANG_MAX);
    return RDSP_ERR_INVALID;
  }
  return for_selected(e, [&](EngSettings &s) {
    s.meter.squelch = 1; s.meter.open_ms = open_ms; s.meter.close_ms = close_ms; s.meter.hang_blocks = hang_blocks;
  });
}
int rdsp_engine_disable_squelch(rdsp_engine_t *e) { return for_selected(e, [](EngSettings &s) { s.meter.squelch = 0; }); }

int rdsp_engine_read_meter(rdsp_engine_t *e, int n_blocks, float *d_level, size_t level_stride, float *d_peak, size_t peak_stride,
                           uint8_t *d_open, size_t open_stride, void *stream) {
  if (!e) return RDSP_ERR_INVALID;
  if (no_meter(e, "rdsp_engine_read_meter")) return RDSP_ERR_NOT_READY;
  const size_t w = (size_t)std::max(n_blocks, 0);
  if (n_blocks < 0 || n_blocks > e->meter->blocks || (d_level && level_stride < w) || (d_peak && peak_stride < w) || (d_open && open_stride < w)) {
    rdsp_set_error("rdsp_engine_read_meter: bad argument (n_blocks %d of the last call's %d; strides at least n_blocks)", n_blocks, e->meter->blocks);
    return RDSP_ERR_INVALID;
  }
  const EngMeter &m = *e->meter;
  const size_t n = (size_t)e->n_channels, rs = (size_t)e->max_blocks;
  hipStream_t s = (hipStream_t)stream;
  hipError_t err = hipSetDevice(e->device);
  if (err == hipSuccess) err = copy_rows(d_level, level_stride, m.level, rs, w, n, 4, s);
  if (err == hipSuccess) err = copy_rows(d_peak, peak_stride, m.peak, rs, w, n, 4, s);
  if (err == hipSuccess) err = copy_rows(d_open, open_stride, m.open, rs, w, n, 1, s);
  return err == hipSuccess ? RDSP_OK : engine_fail("rdsp_engine_read_meter", err);
}

int rdsp_engine_active(rdsp_engine_t *e, int32_t *d_list, int32_t *d_count, void *stream) {
  if (!e) return RDSP_ERR_INVALID;
  if (no_meter(e, "rdsp_engine_active")) return RDSP_ERR_NOT_READY;
  hipStream_t s = (hipStream_t)stream;
  hipError_t err = hipSetDevice(e->device);
  if (err == hipSuccess && d_list) err = hipMemcpyAsync(d_list, e->meter->list, (size_t)e->n_channels * 4, hipMemcpyDeviceToDevice, s);
  if (err == hipSuccess && d_count) err = hipMemcpyAsync(d_count, e->meter->count, 4, hipMemcpyDeviceToDevice, s);
  return err == hipSuccess ? RDSP_OK : engine_fail("rdsp_engine_active", err);
}

int rdsp_engine_get_meter(rdsp_engine_t *e, float *host_out, void *stream) {
  if (!e || !host_out) return RDSP_ERR_INVALID;
  if (no_meter(e, "rdsp_engine_get_meter")) return RDSP_ERR_NOT_READY;
  std::vector<float> w((size_t)e->n_channels * MT_WORDS);
  hipError_t err = hipSetDevice(e->device);
  if (err == hipSuccess) err = hipMemcpyAsync(w.data(), e->meter->words, w.size() * 4, hipMemcpyDeviceToHost, (hipStream_t)stream);
  if (err == hipSuccess) err = hipStreamSynchronize((hipStream_t)stream);
  if (err != hipSuccess) return engine_fail("rdsp_engine_get_meter", err);
  for (int c = 0; c < e->n_channels; c++) {
    const float *m = &w[(size_t)c * MT_WORDS];
    float *o = host_out + (size_t)c * 4;
    o[0] = m[MT_LEVEL]; o[1] = m[MT_LAST_MS]; o[2] = m[MT_LAST_PK]; o[3] = (float)f_bits(m[MT_OPEN]);
  }
  return RDSP_OK;
}

int rdsp_engine_read_demod(rdsp_engine_t *e, int n_blocks, float *d_out, size_t out_stride, void *stream) {
  if (!e || !d_out || n_blocks < 0 || n_blocks > e->last_blocks || out_stride < (size_t)n_blocks * BS) {
    rdsp_set_error("rdsp_engine_read_demod: bad argument (n_blocks %d of the last call's %d; out_stride at least n_blocks * 128)",
                   n_blocks, e ? e->last_blocks : 0);
    return RDSP_ERR_INVALID;
  }
  hipError_t err = hipSetDevice(e->device);
  if (err == hipSuccess)
    err = copy_rows(d_out, out_stride, e->d_audio, (size_t)e->max_blocks * BS, (size_t)n_blocks * BS, (size_t)e->n_channels, 4, (hipStream_t)stream);
  return err == hipSuccess ? RDSP_OK : engine_fail("rdsp_engine_read_demod", err);
}

/* ---- shared IQ streams: receivers tuned to stations inside source rows (the front end, rdsp_engine_sources.hip) ---------- */
namespace {
bool gain_ok(float gain) { return gain > 0.0f && std::isfinite(gain); }
/* the refusal of everything that needs rdsp_engine_set_sources first */
bool no_sources(const rdsp_engine_t *e, const char *who) {
  if (!e->src) rdsp_set_error("%s: no sources; call rdsp_engine_set_sources first", who);
  return !e->src;
}
/* the first channel whose station lies outside +-band, or -1 */
int station_outside(const rdsp_engine_t *e, double band) {
  for (size_t c = 0; c < e->station.size(); c++)
    if (!(fabs(e->station[c]) < band)) return (int)c;
  return -1;
}
/* the end of every setter that may begin another stream */
int configure_sources(rdsp_engine_t *e, const char *who, int P, int Q, float gain, int format) {
  hipError_t err = hipSetDevice(e->device);
  if (err == hipSuccess) err = e->src->configure(P, Q, gain, e->src->st.n_sources, format);
  return err == hipSuccess ? RDSP_OK : engine_fail(who, err);
}
}  // namespace

const float *rdsp_engine_tune_table(void) {
  static const std::vector<float4> tab = [] {
    std::vector<float4> t(rdsp_tune::TUNE_N);
    rdsp_tune::tune_table(t.data());
    return t;
  }();
  return (const float *)tab.data();
}

int rdsp_engine_set_sources(rdsp_engine_t *e, int n_sources, const int *source_of_channel) {
  if (!e || n_sources < 1 || !source_of_channel) {
    rdsp_set_error("rdsp_engine_set_sources: bad argument (n_sources %d)", n_sources);
    return RDSP_ERR_INVALID;
  }
  for (int c = 0; c < e->n_channels; c++)
    if (source_of_channel[c] < 0 || source_of_channel[c] >= n_sources) {
      rdsp_set_error("rdsp_engine_set_sources: channel %d listens to source %d of %d", c, source_of_channel[c], n_sources);
      return RDSP_ERR_INVALID;
    }
  hipError_t err = hipSetDevice(e->device);
  if (err == hipSuccess && !e->src) {
    auto q = std::make_unique<EngFrontEnd>(e->n_channels, e->max_blocks); /* the object stays without sources unless all of it exists */
    err = q->init();
    if (err != hipSuccess) {
      rdsp_set_error("rdsp_engine_set_sources: %s", hipGetErrorString(err));
      return RDSP_ERR_NOMEM;
    }
    e->src = std::move(q);
    if (e->station.empty()) e->station.assign((size_t)e->n_channels, 0.0);
  }
  if (err == hipSuccess) err = e->src->set_map(n_sources, source_of_channel);
  return err == hipSuccess ? RDSP_OK : engine_fail("rdsp_engine_set_sources", err);
}

int rdsp_engine_set_source_decimation(rdsp_engine_t *e, int D, float gain) {
  if (!e || D < 1 || D > rdsp_tune::DDC_MAX_D || !gain_ok(gain)) {
    rdsp_set_error("rdsp_engine_set_source_decimation: bad argument (D %d of 1 .. %d, gain %g must be finite and above 0)", D, rdsp_tune::DDC_MAX_D, (double)gain);
    return RDSP_ERR_INVALID;
  }
  if (no_sources(e, "rdsp_engine_set_source_decimation")) return RDSP_ERR_NOT_READY;
  SourceStream to;
  to.P = D;
  if (const int c = station_outside(e, to.band_hz()); c >= 0) {
    rdsp_set_error("rdsp_engine_set_source_decimation: channel %d is tuned to %g Hz, outside a source at %d x 44100 Hz", c, e->station[(size_t)c], D);
    return RDSP_ERR_INVALID;
  }
  if ((uint64_t)e->n_channels * (uint64_t)(rdsp_tune::DDC_TAPS_PER_PHASE * D) > 0xffffffffull) {
    rdsp_set_error("rdsp_engine_set_source_decimation: %d channels x %d taps do not fit the pass's tap table", e->n_channels, rdsp_tune::DDC_TAPS_PER_PHASE * D);
    return RDSP_ERR_UNSUPPORTED;
  }
  return configure_sources(e, "rdsp_engine_set_source_decimation", D, 1, gain, e->src->st.format);
}
int rdsp_engine_source_decimation(const rdsp_engine_t *e) { return e && source_stream(e).Q == 1 ? source_stream(e).P : 0; }

int rdsp_engine_set_source_rate(rdsp_engine_t *e, int P, int Q, float gain) {
  if (!e || !rdsp_tune::rate_reduce(P, Q) || !gain_ok(gain)) {
    rdsp_set_error("rdsp_engine_set_source_rate: bad argument (in lowest terms 1 <= Q <= %d and Q <= P <= %d Q: P %d, Q %d; gain %g must be "
                   "finite and above 0)", rdsp_tune::RATE_MAX_Q, rdsp_tune::RATE_MAX_RATIO, P, Q, (double)gain);
    return RDSP_ERR_INVALID;
  }
  if (no_sources(e, "rdsp_engine_set_source_rate")) return RDSP_ERR_NOT_READY;
  if (Q == 1) return rdsp_engine_set_source_decimation(e, P, gain); /* an integer multiple: its checks and its texts */
  SourceStream to;
  to.P = P; to.Q = Q;
  if (const int c = station_outside(e, to.band_hz()); c >= 0) {
    rdsp_set_error("rdsp_engine_set_source_rate: channel %d is tuned to %g Hz, outside a source at 44100 x %d / %d Hz", c, e->station[(size_t)c], P, Q);
    return RDSP_ERR_INVALID;
  }
  return configure_sources(e, "rdsp_engine_set_source_rate", P, Q, gain, e->src->st.format);
}
int rdsp_engine_source_rate(const rdsp_engine_t *e, int *P, int *Q) {
  if (!e || !P || !Q) return RDSP_ERR_INVALID;
  *P = source_stream(e).P;
  *Q = source_stream(e).Q;
  return RDSP_OK;
}
size_t rdsp_engine_source_pairs(const rdsp_engine_t *e, int n_blocks) {
  return e && n_blocks >= 0 ? source_stream(e).pairs((uint32_t)n_blocks * BS) : 0;
}
int rdsp_engine_rate_of_hz(double fs_hz, int *P, int *Q) {
  const double top = (double)rdsp_tune::RATE_MAX_RATIO * rdsp_tune::TUNE_FS;
  if (!P || !Q || !(fs_hz >= rdsp_tune::TUNE_FS) || !(fs_hz <= top) || fs_hz != floor(fs_hz)) {
    rdsp_set_error("rdsp_engine_rate_of_hz: %g Hz is not an integer rate in 44100 ... %g Hz", fs_hz, top);
    return RDSP_ERR_INVALID;
  }
  int p = (int)fs_hz, q = 44100;
  if (!rdsp_tune::rate_reduce(p, q)) {
    rdsp_set_error("rdsp_engine_rate_of_hz: %g Hz is 44100 x %d / %d, outside Q <= %d", fs_hz, p, q, rdsp_tune::RATE_MAX_Q);
    return RDSP_ERR_INVALID;
  }
  *P = p; *Q = q;
  return RDSP_OK;
}
int rdsp_engine_rate_taps(int P, int Q, float gain, float *out) {
  if (!rdsp_tune::rate_reduce(P, Q) || !gain_ok(gain) || !out) {
    rdsp_set_error("rdsp_engine_rate_taps: bad argument (in lowest terms 1 <= Q <= %d and Q <= P <= %d Q: P %d, Q %d; gain %g)",
                   rdsp_tune::RATE_MAX_Q, rdsp_tune::RATE_MAX_RATIO, P, Q, (double)gain);
    return RDSP_ERR_INVALID;
  }
  rdsp_tune::rate_taps(P, Q, (double)gain, out);
  return RDSP_OK;
}
int rdsp_engine_ddc_taps(int D, float gain, float *out) {
  if (D < 1 || D > rdsp_tune::DDC_MAX_D || !gain_ok(gain) || !out) {
    rdsp_set_error("rdsp_engine_ddc_taps: bad argument (D %d of 1 .. %d, gain %g)", D, rdsp_tune::DDC_MAX_D, (double)gain);
    return RDSP_ERR_INVALID;
  }
  rdsp_tune::ddc_taps(D, (double)gain, out);
  return RDSP_OK;
}

int rdsp_engine_tune(rdsp_engine_t *e, int first_channel, int n_channels, const double *station_hz) {
  if (!e || !station_hz || first_channel < 0 || n_channels < 1 || n_channels > e->n_channels - first_channel) {
    rdsp_set_error("rdsp_engine_tune: bad argument (channels %d .. %d of %d)", first_channel, first_channel + n_channels - 1, e ? e->n_channels : 0);
    return RDSP_ERR_INVALID;
  }
  const double band = source_stream(e).band_hz();
  for (int k = 0; k < n_channels; k++)
    if (!(fabs(station_hz[k]) < band)) {
      rdsp_set_error("rdsp_engine_tune: channel %d: station %g Hz; |f| must be below %g Hz", first_channel + k, station_hz[k], band);
      return RDSP_ERR_INVALID;
    }
  if (e->station.empty()) e->station.assign((size_t)e->n_channels, 0.0);
  std::copy(station_hz, station_hz + n_channels, e->station.begin() + first_channel);
  if (e->src) e->src->steps_changed();
  return RDSP_OK;
}

/* The format of the source rows.  A setting: kept by reset, set_sources and the rate setters, in no blob.  Another format
 * begins another stream: the source histories (reallocated: words for S16, float2 values otherwise) and frac go to zero as
 * with a change of rate; the phases stay with their channels. */
int rdsp_engine_set_source_format(rdsp_engine_t *e, int format) {
  if (!e || format < 0 || format >= rdsp_tune::SRC_FORMATS) {
    rdsp_set_error("rdsp_engine_set_source_format: bad argument (format %d of RDSP_SRC_S16 = 0, U8 = 1, S8 = 2, F32 = 3)", format);
    return RDSP_ERR_INVALID;
  }
  if (no_sources(e, "rdsp_engine_set_source_format")) return RDSP_ERR_NOT_READY;
  const EngFrontEnd &f = *e->src;
  return format == f.st.format ? RDSP_OK : configure_sources(e, "rdsp_engine_set_source_format", f.st.P, f.st.Q, f.gain, format);
}
int rdsp_engine_source_format(const rdsp_engine_t *e) { return e ? source_stream(e).format : RDSP_ERR_INVALID; }

namespace {
/* both entry points; who: the one that was called, for the error text */
int update_source_rows(const char *who, rdsp_engine_t *e, const void *d_src, size_t src_stride, int n_blocks, int16_t *d_lr, size_t out_stride, void *stream) {
  const SourceStream st = source_stream(e);
  const size_t pair = (size_t)rdsp_tune::src_pair_bytes(st.format), need = st.pairs((uint32_t)std::max(n_blocks, 0) * BS);
  const bool bad = !e || !d_src || !d_lr || n_blocks < 0 || n_blocks > e->max_blocks || src_stride < need || out_stride < (size_t)n_blocks * BS;
  if (st.Q > 1) { /* a rational rate: rows of rdsp_engine_source_pairs pairs, aligned to a pair */
    if (bad || (uintptr_t)d_src % pair != 0) {
      rdsp_set_error("%s: bad argument (n_blocks %d of at most %d; source rows %zu-byte aligned and at least "
                     "rdsp_engine_source_pairs = %zu pairs long at 44100 x %d / %d Hz)", who, n_blocks, e->max_blocks, pair, need, st.P, st.Q);
      return RDSP_ERR_INVALID;
    }
  } else if (bad || (src_stride * pair) % 16 != 0 || ((uintptr_t)d_src & 15) != 0) {
    rdsp_set_error("%s: bad argument (n_blocks %d of at most %d; source rows 16-byte aligned, a multiple of 16 "
                   "bytes apart and at least n_blocks * 128 * D pairs long, D = %d)", who, n_blocks, e ? e->max_blocks : 0, e ? st.P : 0);
    return RDSP_ERR_INVALID;
  }
  if (no_sources(e, who)) return RDSP_ERR_NOT_READY;
  if (!e->tables) {
    rdsp_set_error("%s: the engine's coefficient tables are not loaded (rdsp_engine_load_tables)", who);
    return RDSP_ERR_NOT_READY;
  }
  if (n_blocks == 0) return RDSP_OK;
  hipError_t err = hipSetDevice(e->device);
  const SourceTuning tuning{e->first, [e](size_t g) { return e->grp[g].tuning_offset; }, e->station};
  if (err == hipSuccess) err = e->src->run(d_src, src_stride, n_blocks, tuning, (hipStream_t)stream);
  if (err != hipSuccess) return engine_fail(who, err);
  return rdsp_engine_update(e, (const int16_t *)e->src->tuned.p, (size_t)e->max_blocks * BS, n_blocks, d_lr, out_stride, stream);
}

}  // namespace

int rdsp_engine_update_source_samples(rdsp_engine_t *e, const void *d_src, size_t src_stride, int n_blocks, int16_t *d_lr, size_t out_stride, void *stream) {
  return update_source_rows("rdsp_engine_update_source_samples", e, d_src, src_stride, n_blocks, d_lr, out_stride, stream);
}

int rdsp_engine_update_sources(rdsp_engine_t *e, const int16_t *d_src, size_t src_stride, int n_blocks, int16_t *d_lr, size_t out_stride, void *stream) {
  if (source_stream(e).format != rdsp_tune::SRC_S16) {
    rdsp_set_error("rdsp_engine_update_sources: the engine's source format is %d, not int16; call rdsp_engine_update_source_samples", source_stream(e).format);
    return RDSP_ERR_INVALID;
  }
  return update_source_rows("rdsp_engine_update_sources", e, d_src, src_stride, n_blocks, d_lr, out_stride, stream);
}

/* ---- the signal state of a channel range as data: resume, or move receivers between objects / GPUs ---------------------
 * Blob = header {magic, version, n_channels, flags} + per channel: the 96 state words, the last 512 samples of both lines
 * of the side-band network in time order (whatever the ring's size and position here or there), the blanker's lines, the
 * ALS filter's line and taps.  Settings are not part of it (they belong to the group the channels land in).  An engine with
 * sources (rdsp_engine_set_sources) sets flag STATE_PHASES and appends each channel's tuning phase accumulator; the blob
 * of any other engine is as it was before sources existed (flags 0, nothing appended). */
namespace {
constexpr uint32_t STATE_MAGIC = 0x45534452u; /* "RDSE" */
constexpr uint32_t STATE_PHASES = 1u;
constexpr uint32_t STATE_METER = 2u; /* an engine with the meter appends {level, open, hang} per channel, behind the phases */
/* where a channel's planes lie in its blob words: whole, but of a ring its last RING_KEPT samples in time order */
constexpr size_t RING_KEPT = 512;
constexpr size_t BLOB_OFF[N_PLANES] = {0, NF, NF + RING_KEPT, NF + 2 * RING_KEPT, NF + 2 * RING_KEPT + NB_WORDS};
constexpr size_t STATE_CH_WORDS = BLOB_OFF[PL_ALS] + ALS_WORDS;
struct StateImage { /* host images of the planes of n channels */
  std::vector<float> plane[N_PLANES];
  std::vector<uint32_t> ph; /* tuning phases, of an engine with sources */
  std::vector<float> mt;    /* meter words, of an engine with the meter */
  StateImage(const rdsp_engine_t *e, size_t n) : ph(e->src ? n : 0, 0u), mt(e->meter ? n * MT_WORDS : 0, 0.0f) {
    for (int k = 0; k < N_PLANES; k++) plane[k].assign(n * e->plane_words[k], 0.0f);
  }
};
/* channels c0 .. c0 + n - 1 between the device and the image, then the stream drained */
hipError_t image_copy(rdsp_engine_t *e, StateImage &im, bool save, size_t c0, size_t n, hipStream_t s) {
  const hipMemcpyKind kind = save ? hipMemcpyDeviceToHost : hipMemcpyHostToDevice;
  auto copy = [&](void *dev, void *host, size_t bytes) { return hipMemcpyAsync(save ? host : dev, save ? dev : host, bytes, kind, s); };
  hipError_t err = hipSetDevice(e->device);
  if (err == hipSuccess && e->src) err = copy(e->src->phase + c0, im.ph.data(), n * 4);
  if (err == hipSuccess && e->meter) err = copy(e->meter->words + c0 * MT_WORDS, im.mt.data(), n * MT_WORDS * 4);
  for (int k = 0; k < N_PLANES && err == hipSuccess; k++) err = copy(e->plane[k] + c0 * e->plane_words[k], im.plane[k].data(), im.plane[k].size() * 4);
  if (err == hipSuccess) err = hipStreamSynchronize(s);
  return err;
}
/* the blob's channel words w (n channels from first_channel on) from the image, or the image from them; returns their end */
float *blob_move(const rdsp_engine_t *e, StateImage &im, bool save, int first_channel, size_t n, float *w) {
  for (size_t c = 0; c < n; c++, w += STATE_CH_WORDS) {
    const uint32_t pos = e->grp[(size_t)group_of(e->first, first_channel + (int)c)].pos;
    for (int k = 0; k < N_PLANES; k++) {
      float *b = w + BLOB_OFF[k], *h = &im.plane[k][c * e->plane_words[k]];
      if (k != PL_RING_I && k != PL_RING_Q) { memcpy(save ? b : h, save ? h : b, e->plane_words[k] * 4); continue; }
      for (uint32_t i = 0; i < RING_KEPT; i++) { /* sample pos - 512 + i */
        float &x = h[(pos - (uint32_t)RING_KEPT + i) & (e->ring_size - 1)];
        if (save) b[i] = x;
        else x = b[i];
      }
    }
  }
  return w;
}
}  // namespace
size_t rdsp_engine_state_bytes(const rdsp_engine_t *e, int n_channels) {
  return (e && n_channels > 0) ? 16 + (size_t)n_channels * (STATE_CH_WORDS + (e->src ? 1 : 0) + (e->meter ? MT_STATE_WORDS : 0)) * 4 : 0;
}
int rdsp_engine_save_state(rdsp_engine_t *e, int first_channel, int n_channels, void *host_buf, size_t bytes, void *stream) {
  if (!e || !host_buf || first_channel < 0 || n_channels < 1 || first_channel + n_channels > e->n_channels ||
      bytes < rdsp_engine_state_bytes(e, n_channels)) {
    rdsp_set_error("rdsp_engine_save_state: bad argument");
    return RDSP_ERR_INVALID;
  }
  const size_t n = (size_t)n_channels;
  StateImage im(e, n);
  const hipError_t err = image_copy(e, im, true, (size_t)first_channel, n, (hipStream_t)stream);
  if (err != hipSuccess) return engine_fail("rdsp_engine_save_state", err);
  uint32_t *hdr = (uint32_t *)host_buf;
  hdr[0] = STATE_MAGIC; hdr[1] = 1; hdr[2] = (uint32_t)n_channels; hdr[3] = (e->src ? STATE_PHASES : 0) | (e->meter ? STATE_METER : 0);
  float *end = blob_move(e, im, true, first_channel, n, (float *)(hdr + 4));
  if (e->src) { memcpy(end, im.ph.data(), n * 4); end += n; } /* after the last channel's words */
  for (size_t c = 0; e->meter && c < n; c++) memcpy(end + c * MT_STATE_WORDS, &im.mt[c * MT_WORDS], MT_STATE_WORDS * 4);
  return RDSP_OK;
}
int rdsp_engine_load_state(rdsp_engine_t *e, int first_channel, const void *host_buf, size_t bytes, void *stream) {
  const uint32_t *hdr = (const uint32_t *)host_buf;
  if (!e || !host_buf || bytes < 16 || hdr[0] != STATE_MAGIC || hdr[1] != 1 || (hdr[3] & ~(STATE_PHASES | STATE_METER)) != 0) {
    rdsp_set_error("rdsp_engine_load_state: not an engine state blob of this version");
    return RDSP_ERR_INVALID;
  }
  const bool phases = (hdr[3] & STATE_PHASES) != 0, meter = (hdr[3] & STATE_METER) != 0;
  const size_t n = hdr[2], c0 = (size_t)first_channel;
  if (first_channel < 0 || n < 1 || c0 + n > (size_t)e->n_channels || bytes < 16 + n * (STATE_CH_WORDS + (phases ? 1 : 0) + (meter ? MT_STATE_WORDS : 0)) * 4) {
    rdsp_set_error("rdsp_engine_load_state: %zu channels at %d do not fit", n, first_channel);
    return RDSP_ERR_INVALID;
  }
  if (phases && !e->src) {
    rdsp_set_error("rdsp_engine_load_state: the blob carries tuning phases; call rdsp_engine_set_sources first");
    return RDSP_ERR_NOT_READY;
  }
  if (meter && !e->meter) {
    rdsp_set_error("rdsp_engine_load_state: the blob carries meter state; call rdsp_engine_enable_meter first");
    return RDSP_ERR_NOT_READY;
  }
  /* zeros: the rings outside the kept samples, the phases of a blob from an engine that never tuned, the meter words of one
   * that never metered (and always those of the last call: they are no state) */
  StateImage im(e, n);
  const float *end = blob_move(e, im, false, first_channel, n, (float *)(hdr + 4)); /* read only: save is false */
  if (phases) { memcpy(im.ph.data(), end, n * 4); end += n; }
  for (size_t c = 0; meter && c < n; c++) memcpy(&im.mt[c * MT_WORDS], end + c * MT_STATE_WORDS, MT_STATE_WORDS * 4);
  const hipError_t err = image_copy(e, im, false, c0, n, (hipStream_t)stream);
  return err == hipSuccess ? RDSP_OK : engine_fail("rdsp_engine_load_state", err);
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
