/*
 * rdsp_engine_int.h -- what rdsp_engine_t's kernels (rdsp_engine.hip and the stage files it names) and its host object (rdsp_engine_host.h) share: the
 * kernels' arguments, a channel's state words, the launch of one group's kernels; and what the engine's and the
 * pre-processor's (rdsp_preproc.hip) host sides share: the owner of a device allocation (rdsp_dev.h), the HIP error return. */
#ifndef RDSP_ENGINE_INT_H
#define RDSP_ENGINE_INT_H

#include <hip/hip_runtime.h>

#include "rdsp_dev.h"
#include "rdsp_host.h"
#include "rdsp_kernels.h"

namespace rdsp_eng {

constexpr int BS = RDSP_BLOCK_SAMPLES;
/* per-channel state, floats (ints bit-cast): [channel][NF] */
enum { ST_PRE = 0, ST_AM = 32, ST_AUDIO = 64, ST_NCO = 80, ST_AMPH, ST_SAM_COS, ST_SAM_SIN, ST_SAM_U, ST_SAM_ERR, ST_SAM_HZ,
       ST_SAM_PH, ST_SAM_LOCK, ST_AGC_ENV, ST_AGC_GAIN, ST_AGC_HANG, ST_AGC_ACTIVE, ST_NB_AVG, ST_NB_HIT, ST_NB_LAST, NF = 96 };
enum { RESET_PRE = 1, RESET_AUDIO = 2, RESET_ALS = 4, RESET_FM = 8 }; /* RESET_FM: the host's and the FM kernel's (rdsp_engine_fm.h) */
constexpr int ALS_WORDS = 256 + 64;                       /* per channel in HBM: the 256-sample line, then the taps (64 words) */
constexpr int NB_WORDS = 3 * 384;                          /* per channel: I line, Q line, mask */

struct EngParams {
  const int32_t *iq; size_t in_stride;   /* [ch][t] words: I | Q << 16 */
  int32_t *out; size_t out_stride;       /* [ch][t] words: L | R << 16 */
  int n_channels, n_blocks;
  float *st;
  float *ring_i, *ring_q; uint32_t ring_size, pos; /* [ch][ring_size], power of two; pos = where this call's first sample goes */
  float *audio; size_t audio_stride;     /* [ch][max samples per call] */
  float *nb, *als;
  const float *sets, *hilbert, *sine, *curve;
  int mode, mute, audio_on, agc_on, als_notch, als_adaptive, resets;
  int pre_set, audio_set;
  float gain_i, gain_q, output_gain, tuning_offset, if_centre;
  EngineAgcSet agc;
  float nb_keep, nb_new, nb_ratio; int nb_before, nb_after;
  float sam_keep, sam_new, sam_hz_per_rad, sam_lock_lo, sam_lock_hi, sam_ga, sam_gb;
};

using rdsp_dev::DevBuf; /* the one owner of a device allocation: freed with its owner (whose destroy makes the device current first) */
static inline int engine_fail(const char *what, hipError_t err) {
  rdsp_set_error("%s: %s", what, hipGetErrorString(err));
  return RDSP_ERR_HIP;
}

/* the stages' launch entries, each beside its kernels: rdsp_engine_front.hip (the kernel by blanker and mode),
 * rdsp_engine_hilbert.hip (SSB / CW only), rdsp_engine_tail.hip (the kernel by ALS) */
void engine_launch_front(const EngParams &p, bool blanker, hipStream_t s);
void engine_launch_hilbert(const EngParams &p, hipStream_t s);
void engine_launch_tail(const EngParams &p, bool als, hipStream_t s);
}  // namespace rdsp_eng

/* one group's launches of a call, stream-ordered: the three stages above (rdsp_engine.hip); p holds the group's channel
 * range and settings */
hipError_t rdsp_engine_launch(const rdsp_eng::EngParams &p, bool blanker, bool als, hipStream_t s);

#endif
