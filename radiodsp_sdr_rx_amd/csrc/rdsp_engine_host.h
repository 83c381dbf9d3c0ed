/*
 * rdsp_engine_host.h -- what the host files of rdsp_engine_t (include/rdsp.h) share: the object, a group's settings, the
 * meter as an owner, the walk over groups.  rdsp_engine_host.hip holds the sketch's settings and setters and creates, resets
 * and runs the object; rdsp_engine_groups.hip the receiver groups; rdsp_engine_meter_host.hip the signal meter's owner and
 * entry points, rdsp_engine_pack_active among them; rdsp_engine_sources_host.hip the entry points of the shared IQ sources;
 * rdsp_engine_voice_host.hip the voice-rate audio's owner and entry points; rdsp_engine_fm_host.hip the narrow-band FM
 * detector's; rdsp_engine_tone_host.hip the tone squelch's; rdsp_engine_tone_search_host.hip the tone search's;
 * rdsp_engine_dcs_host.hip the code squelch's; rdsp_engine_noise_host.hip the noise squelch's; rdsp_engine_dtmf_host.hip the DTMF decoder's; rdsp_engine_afsk_host.hip the AFSK 1200 decoder's; rdsp_engine_pocsag_host.hip the POCSAG decoder's; rdsp_engine_events_host.hip the owner and entry points of rdsp_engine_gather_events; rdsp_engine_state.hip the state blob.  Host logic only: the kernels
 * are rdsp_engine.hip's stage files' (rdsp_engine_front / _hilbert / _tail.hip), rdsp_engine_meter.hip's, rdsp_engine_pack.hip's,
 * rdsp_engine_voice.hip's, rdsp_engine_fm.hip's, rdsp_engine_tone.hip's, rdsp_engine_tone_search.hip's, rdsp_engine_dcs.hip's, rdsp_engine_noise.hip's, rdsp_engine_dtmf.hip's, rdsp_engine_afsk.hip's, rdsp_engine_pocsag.hip's and rdsp_engine_events.hip's, the front end is
 * rdsp_engine_sources.h's.  All fifteen are compiled with the kernels' flags (-ffp-contract=off).
 */
#ifndef RDSP_ENGINE_HOST_H
#define RDSP_ENGINE_HOST_H

#include <string.h>

#include <algorithm>
#include <cmath>
#include <memory>
#include <vector>

#include "rdsp_engine_afsk.h"
#include "rdsp_engine_dcs.h"
#include "rdsp_engine_dtmf.h"
#include "rdsp_engine_events.h"
#include "rdsp_engine_fm.h"
#include "rdsp_engine_int.h"
#include "rdsp_engine_laws.h"
#include "rdsp_engine_meter.h"
#include "rdsp_engine_noise.h"
#include "rdsp_engine_pocsag.h"
#include "rdsp_engine_pack.h"
#include "rdsp_engine_sources.h"
#include "rdsp_engine_tone.h"
#include "rdsp_engine_tone_search.h"
#include "rdsp_engine_voice.h"

using namespace rdsp_eng;

/* what the sketch's calls set: one set per receiver group (one group = the whole object unless rdsp_engine_set_groups cut it) */
struct EngSettings {
  float input_gain, gain_i, gain_q, iq_balance, output_gain, tuning_offset;
  int mode, mute, audio_on, audio_id, audio_set, pre_set, agc_on, als_on, als_notch, als_adaptive, nb_on, resets;
  int nfm; /* the group demodulates narrow-band FM: setDemodMode(RDSP_ENGINE_MODE_NFM) behind rdsp_engine_enable_fm */
  rdsp_fm::FmSet fm; /* rdsp_engine_set_fm: in force while the group is in NFM */
  rdsp_tone::ToneSet tone; /* rdsp_engine_set_tone_squelch: in force while the group is in NFM behind rdsp_engine_enable_tone */
  rdsp_tone_search::SearchSet search; /* rdsp_engine_set_tone_search: in force while the group is in NFM behind rdsp_engine_enable_tone_search */
  rdsp_dcs::DcsSet dcs; /* rdsp_engine_set_dcs_squelch: in force while the group is in NFM behind rdsp_engine_enable_dcs */
  rdsp_noise::NoiseSet noise; /* rdsp_engine_set_noise_squelch: in force while the group is in NFM behind rdsp_engine_enable_noise */
  rdsp_dtmf::DtmfSet dtmf; /* rdsp_engine_set_dtmf: in force while the group is in NFM behind rdsp_engine_enable_dtmf */
  rdsp_afsk::AfskSet afsk; /* rdsp_engine_set_afsk: in force while the group is in NFM behind rdsp_engine_enable_afsk */
  rdsp_pocsag::PocsagSet pocsag; /* rdsp_engine_set_pocsag: in force while the group is in NFM behind rdsp_engine_enable_pocsag */
  EngineAgcSet agc;
  rdsp_meter::MeterSet meter; /* rdsp_engine_set_meter / set_squelch: in force once rdsp_engine_enable_meter was called */
  uint32_t pos; /* where the group's next sample goes in its channels' rings (they only move in the SSB / CW modes) */
};
/* the planes of a channel's signal state: create allocates them, reset fills them, save_state / load_state move them */
enum { PL_ST, PL_RING_I, PL_RING_Q, PL_NB, PL_ALS, N_PLANES };
/* the signal meter (rdsp_engine_meter_host.hip): every channel's meter words, the last call's records [ch][max_blocks], its list */
struct EngMeter {
  DevBuf<float> words, level, peak;
  DevBuf<uint8_t> open;
  DevBuf<int32_t> list, count;
  DevBuf<int32_t> pack_offset; /* [ch], rdsp_engine_pack_active's scratch: allocated by its first call, not by init */
  size_t n_channels = 0, max_blocks = 0;
  int blocks = 0; /* of the last call that left records */
  hipError_t init(size_t n_channels, size_t max_blocks); /* every buffer, zeroed */
  hipError_t reset(hipStream_t s);                       /* level 0, gate closed, hang 0 */
  /* behind the tail kernel of the group p launched (channels c0 on): it measures p.audio and gates p.out, rows of the caller's d_lr */
  hipError_t launch_group(const EngParams &p, size_t c0, const rdsp_meter::MeterSet &set, const int16_t *d_lr, hipStream_t s) const;
  hipError_t launch_list(int n_blocks, hipStream_t s); /* once behind every group's meter: the list of a call of n_blocks */
  /* the open blocks of the last call's first n_blocks, out of the caller's rows: p carries the caller's arguments, the rest is filled in here */
  hipError_t launch_pack(PackParams p, hipStream_t s) const;
};
/* the voice-rate audio (rdsp_engine_voice_host.hip): every channel's history of left words, the last call's decimated rows */
struct EngVoice {
  int R = 0;
  DevBuf<int32_t> hist, taps; /* [ch][VOICE_HIST]; the 16 R tap words of voice_tap_pairs */
  DevBuf<int16_t> rows;       /* [ch][row_words], row_words = max_blocks 128 / R */
  size_t n_channels = 0, row_words = 0;
  int blocks = 0; /* of the last call */
  hipError_t init(size_t n_channels, size_t max_blocks, int R); /* every buffer; history and rows zeroed */
  hipError_t reset(hipStream_t s);                              /* the history zero */
  hipError_t launch(const int16_t *d_lr, size_t out_stride, int n_blocks, hipStream_t s); /* once per call, behind the last group's meter */
};
/* the narrow-band FM detector (rdsp_engine_fm_host.hip): every channel's state words, the last call's level rows, the taps */
struct EngFm {
  DevBuf<uint32_t> state; /* [ch][FM_STATE_WORDS] */
  DevBuf<float> level;    /* [ch][row_words], row_words = max_blocks 128: what an NFM group's meter measures */
  DevBuf<float> taps;     /* the 32 taps of W = 2, then the 48 of W = 3 */
  size_t n_channels = 0, row_words = 0;
  std::vector<std::pair<size_t, size_t>> nfm_rows; /* of the last call: first channel and count of every group that ran the detector */
  hipError_t init(size_t n_channels, size_t max_blocks); /* every buffer; state and rows zeroed */
  hipError_t reset(hipStream_t s);                       /* the state zero */
  /* in place of the front and Hilbert kernels of the group p describes (channels c0 on): y into p.audio, the level rows beside it */
  hipError_t launch_group(const EngParams &p, size_t c0, const rdsp_fm::FmSet &set, const int16_t *d_iq, hipStream_t s);
  /* p with the group's level rows where its demodulated rows were: what the meter of an NFM group is handed */
  EngParams metered(EngParams p, size_t c0) const { p.audio = level + c0 * row_words; p.audio_stride = row_words; return p; }
};
/* the tone squelch (rdsp_engine_tone_host.hip): every channel's detector words and step, the last call's records, the table */
struct EngTone {
  DevBuf<uint32_t> state, dphi; /* [ch][TONE_WORDS]; [ch] */
  DevBuf<float> a2;             /* [ch][max_blocks] */
  DevBuf<uint8_t> tone;         /* [ch][max_blocks] */
  DevBuf<float4> tab;           /* rdsp_tune.h's table, the detector's own copy: the engine may have no sources */
  rdsp_dev::Event dphi_ev;      /* the last upload has left dphi_stage */
  std::vector<uint32_t> dphi_stage;
  bool stale = true;            /* rdsp_engine_set_tones since the last upload */
  size_t n_channels = 0, max_blocks = 0;
  std::vector<std::pair<size_t, size_t>> rows; /* of the last call: first channel and count of every group that ran the detector */
  hipError_t init(size_t n_channels, size_t max_blocks); /* every buffer; state, steps and records zeroed */
  hipError_t reset(hipStream_t s);                       /* the state zero */
  hipError_t upload(const std::vector<float> &tone_hz, hipStream_t s); /* the steps of the channels' tones, when they changed */
  /* behind the meter kernel of the NFM group p describes (channels c0 on), behind its tail kernel without a meter */
  hipError_t launch_group(const EngParams &p, size_t c0, const rdsp_tone::ToneSet &set, const EngMeter *meter, const int16_t *d_lr, hipStream_t s);
};
/* the tone search (rdsp_engine_tone_search_host.hip): every channel's detector words, the bank's steps, the last call's records,
 * the table */
struct EngToneSearch {
  DevBuf<uint32_t> state, dphi; /* [ch][SEARCH_WORDS]; [MAX_TONES] */
  DevBuf<uint8_t> best;         /* [ch][max_blocks] */
  DevBuf<float> a2, next;       /* [ch][max_blocks] */
  DevBuf<float4> tab;           /* rdsp_tune.h's table, the detector's own copy: the engine may have no sources */
  rdsp_dev::Event bank_ev;      /* the last upload has left `bank` */
  rdsp_tone_search::SearchBank bank; /* as uploaded last: what the kernel runs with */
  bool stale = true;            /* rdsp_engine_set_tone_bank since the last upload (or none yet) */
  size_t n_channels = 0, max_blocks = 0;
  std::vector<std::pair<size_t, size_t>> rows; /* of the last call: first channel and count of every group that ran the detector */
  hipError_t init(size_t n_channels, size_t max_blocks); /* every buffer; state, steps and records zeroed */
  hipError_t reset(hipStream_t s);                       /* the state zero */
  hipError_t upload(const rdsp_tone_search::SearchBank &b, hipStream_t s); /* the bank's steps, when it changed */
  /* behind the tone-squelch kernel of the NFM group p describes (channels c0 on); set.K > 0 */
  hipError_t launch_group(const EngParams &p, size_t c0, const rdsp_tone_search::SearchSet &set, hipStream_t s);
  hipError_t clear_group(size_t c0, size_t count, hipStream_t s); /* a group with K == 0: its channels' words are zeros */
};
/* the code squelch (rdsp_engine_dcs_host.hip): every channel's detector words and setting, the last call's records */
struct EngDcs {
  DevBuf<uint32_t> state, sel;  /* [ch][DCS_WORDS]; [ch]: dcs_sel of the channel's code */
  DevBuf<uint8_t> dcs, hits;    /* [ch][max_blocks] */
  DevBuf<uint32_t> word;        /* [ch][max_blocks] */
  rdsp_dev::Event sel_ev;       /* the last upload has left sel_stage */
  std::vector<uint32_t> sel_stage;
  bool stale = true;            /* rdsp_engine_set_dcs_codes since the last upload */
  size_t n_channels = 0, max_blocks = 0;
  std::vector<std::pair<size_t, size_t>> rows; /* of the last call: first channel and count of every group that ran the detector */
  hipError_t init(size_t n_channels, size_t max_blocks); /* every buffer; state, settings and records zeroed */
  hipError_t reset(hipStream_t s);                       /* the state zero */
  hipError_t upload(const std::vector<uint16_t> &codes, hipStream_t s); /* the channels' settings, when they changed */
  /* behind the tone-squelch kernel of the NFM group p describes (channels c0 on), behind its meter or tail kernel without one */
  hipError_t launch_group(const EngParams &p, size_t c0, const rdsp_dcs::DcsSet &set, const EngMeter *meter, const int16_t *d_lr, hipStream_t s);
};
/* the noise squelch (rdsp_engine_noise_host.hip): every channel's detector words, the last call's records, the taps by time constant */
struct EngNoise {
  DevBuf<uint32_t> state; /* [ch][NOISE_WORDS] */
  DevBuf<float> noise;    /* [ch][max_blocks] */
  DevBuf<uint8_t> nopen;  /* [ch][max_blocks] */
  struct Taps { float tau_us; float g[rdsp_noise::NOISE_TAPS]; };
  std::vector<Taps> taps; /* noise_taps of every tau_us a group was run with: computed when a group's set_fm brings a new one */
  size_t n_channels = 0, max_blocks = 0;
  std::vector<std::pair<size_t, size_t>> rows; /* of the last call: first channel and count of every group that ran the detector */
  hipError_t init(size_t n_channels, size_t max_blocks); /* every buffer; state and records zeroed */
  hipError_t reset(hipStream_t s);                       /* the state zero */
  const float *taps_of(float tau_us);
  /* behind the meter kernel of the NFM group p describes (channels c0 on), behind its tail kernel without a meter; set.mode == 0:
   * the group's words are zeroed instead */
  hipError_t launch_group(const EngParams &p, size_t c0, const rdsp_noise::NoiseSet &set, const rdsp_fm::FmSet &fm, const EngMeter *meter,
                          const int16_t *d_lr, hipStream_t s);
};
/* the DTMF decoder (rdsp_engine_dtmf_host.hip): every channel's detector words, the last call's records, the table */
struct EngDtmf {
  DevBuf<uint32_t> state;   /* [ch][DTMF_WORDS] */
  DevBuf<uint8_t> key, fresh; /* [ch][max_blocks]: key_rec, new_rec */
  DevBuf<float> lo, hi;     /* [ch][max_blocks] */
  DevBuf<float4> tab;       /* rdsp_tune.h's table, the detector's own copy: the engine may have no sources */
  size_t n_channels = 0, max_blocks = 0;
  std::vector<std::pair<size_t, size_t>> rows; /* of the last call: first channel and count of every group that ran the detector */
  hipError_t init(size_t n_channels, size_t max_blocks); /* every buffer; state and records zeroed */
  hipError_t reset(hipStream_t s);                       /* the state zero */
  /* behind the other detector kernels of the NFM group p describes (channels c0 on); set.K > 0 */
  hipError_t launch_group(const EngParams &p, size_t c0, const rdsp_dtmf::DtmfSet &set, hipStream_t s);
  hipError_t clear_group(size_t c0, size_t count, hipStream_t s); /* a group with K == 0: its channels' words are zeros */
};
/* the AFSK 1200 packet decoder (rdsp_engine_afsk_host.hip): every channel's detector words, the last call's records, the table */
struct EngAfsk {
  DevBuf<uint32_t> state;          /* [ch][AFSK_WORDS] */
  DevBuf<uint8_t> sync, fresh, bad; /* [ch][max_blocks]: sync_rec, new_rec, bad_rec */
  DevBuf<float> lvl;               /* [ch][max_blocks] */
  DevBuf<float4> tab;              /* rdsp_tune.h's table, the detector's own copy: the engine may have no sources */
  size_t n_channels = 0, max_blocks = 0;
  std::vector<std::pair<size_t, size_t>> rows; /* of the last call: first channel and count of every group that ran the detector */
  hipError_t init(size_t n_channels, size_t max_blocks); /* every buffer; state and records zeroed */
  hipError_t reset(hipStream_t s);                       /* the state zero */
  /* behind the other detector kernels of the NFM group p describes (channels c0 on); set.on == 1 */
  hipError_t launch_group(const EngParams &p, size_t c0, const rdsp_afsk::AfskSet &set, hipStream_t s);
  hipError_t clear_group(size_t c0, size_t count, hipStream_t s); /* a group with the decoder off: its channels' words are zeros */
};
/* the POCSAG pager decoder (rdsp_engine_pocsag_host.hip): every channel's detector words and the last call's records */
struct EngPocsag {
  DevBuf<uint32_t> state;          /* [ch][POCSAG_WORDS] */
  DevBuf<uint8_t> sync, fresh, bad; /* [ch][max_blocks]: sync_rec, new_rec, bad_rec */
  DevBuf<float> lvl, dc;           /* [ch][max_blocks] */
  size_t n_channels = 0, max_blocks = 0;
  std::vector<std::pair<size_t, size_t>> rows; /* of the last call: first channel and count of every group that ran the detector */
  hipError_t init(size_t n_channels, size_t max_blocks); /* every buffer; state and records zeroed */
  hipError_t reset(hipStream_t s);                       /* the state zero */
  /* behind the other detector kernels of the NFM group p describes (channels c0 on); set.baud != 0 */
  hipError_t launch_group(const EngParams &p, size_t c0, const rdsp_pocsag::PocsagSet &set, hipStream_t s);
  hipError_t clear_group(size_t c0, size_t count, hipStream_t s); /* a group with baud 0: its channels' words are zeros */
};
/* the decoders' events (rdsp_engine_events_host.hip): rdsp_engine_gather_events' scratch, allocated by its first call; it owns no
 * state and reads the decoders' */
struct EngEvents {
  DevBuf<int4> chan;   /* [ch]: a channel's counts, then where its first event and word go */
  DevBuf<uint8_t> ran; /* [kind][ch]: 1 where the kind's decoder ran on the channel in the last call (its owner's `rows`) */
  size_t n_channels = 0;
  hipError_t init(size_t n_channels); /* both buffers */
  /* p carries the caller's arguments; the decoders' words, records and rows are filled in here */
  hipError_t launch(const rdsp_engine *e, rdsp_eng::EventsParams p, hipStream_t s);
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
  std::unique_ptr<EngVoice> voice; /* the voice-rate audio, from rdsp_engine_enable_voice on */
  std::unique_ptr<EngFm> fm;       /* the narrow-band FM detector, from rdsp_engine_enable_fm on */
  std::unique_ptr<EngTone> tone;   /* the tone squelch, from rdsp_engine_enable_tone on */
  std::unique_ptr<EngToneSearch> search; /* the tone search, from rdsp_engine_enable_tone_search on */
  std::unique_ptr<EngDcs> dcs;     /* the code squelch, from rdsp_engine_enable_dcs on */
  std::unique_ptr<EngNoise> noise; /* the noise squelch, from rdsp_engine_enable_noise on */
  std::unique_ptr<EngDtmf> dtmf;   /* the DTMF decoder, from rdsp_engine_enable_dtmf on */
  std::unique_ptr<EngAfsk> afsk;   /* the AFSK 1200 decoder, from rdsp_engine_enable_afsk on */
  std::unique_ptr<EngPocsag> pocsag; /* the POCSAG decoder, from rdsp_engine_enable_pocsag on */
  std::unique_ptr<EngEvents> events; /* rdsp_engine_gather_events' scratch, from its first call on */
  int last_blocks = 0;             /* of the last call that ran: what rdsp_engine_read_demod may ask for */
  int event_blocks = 0;            /* the blocks of the last update while the decoders' words are still as it left them: 0 behind an update
                                      of no blocks, rdsp_engine_reset and rdsp_engine_load_state (rdsp_engine_gather_events then counts nothing) */
  std::vector<float> tone_hz;      /* per channel (empty: all 0), rdsp_engine_set_tones: a setting that may precede the detector */
  std::vector<uint16_t> dcs_codes; /* per channel (empty: all 0), rdsp_engine_set_dcs_codes: a setting that may precede the detector */
  std::vector<float> bank_hz;      /* rdsp_engine_set_tone_bank (empty: the 50 standard tones): a setting that may precede the search */
  std::vector<double> station; /* per channel, Hz from its stream's centre (0 until tuned): a setting that may precede the sources */
};

/* the engine's bank as the tone search runs it: the caller's (rdsp_engine_set_tone_bank), or the standard tones */
rdsp_tone_search::SearchBank rdsp_engine_search_bank(const rdsp_engine_t *e);

/* the setters address the selected group, or all of them */
template <typename F>
static inline int for_selected(rdsp_engine_t *e, F f) {
  if (!e) return RDSP_ERR_INVALID;
  for (size_t g = 0; g < e->grp.size(); g++)
    if (e->sel < 0 || (size_t)e->sel == g) f(e->grp[g]);
  return RDSP_OK;
}
static inline int group_of(const std::vector<int> &first, int ch) {
  size_t g = 0;
  while (g + 1 < first.size() && first[g + 1] <= ch) g++;
  return (int)g;
}
/* where range g of `first` ends: the channels of group g are first[g] .. range_end(first, g, n_channels) - 1 */
static inline int range_end(const std::vector<int> &first, size_t g, int n_channels) { return g + 1 < first.size() ? first[g + 1] : n_channels; }
/* the refusals of everything that needs rdsp_engine_enable_meter / rdsp_engine_set_sources first */
static inline bool no_meter(const rdsp_engine_t *e, const char *who) {
  if (!e->meter) rdsp_set_error("%s: the meter is off; call rdsp_engine_enable_meter first", who);
  return !e->meter;
}
static inline bool no_sources(const rdsp_engine_t *e, const char *who) {
  if (!e->src) rdsp_set_error("%s: no sources; call rdsp_engine_set_sources first", who);
  return !e->src;
}

#endif
