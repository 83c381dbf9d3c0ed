/*
 * rdsp_chain_int.h -- what the host files of rdsp_chain_t share: the object, the error returns, the table of per-channel
 * state planes.  rdsp_chain.hip creates, destroys, resets and runs it; rdsp_chain_groups.hip holds the receiver groups'
 * device side (their double-buffered slots, GroupSlot below, and their records); rdsp_chain_select.hip what selects a
 * group's filter and demodulator; rdsp_chain_ctl.hip the setters; rdsp_chain_state.hip the state planes, the blob and the
 * read-backs.  Host logic only; the arithmetic lives in the kernel files (rdsp_front_*.hip, rdsp_tail*.hip, ...).
 */
#ifndef RDSP_CHAIN_INT_H
#define RDSP_CHAIN_INT_H

#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <array>
#include <deque>
#include <vector>

#include "rdsp_dev.h"
#include "rdsp_host.h"
#include "rdsp_kernels.h"
#include "rdsp_slot.h"

using namespace rdsp_dev; /* DevBuf, PinnedBuf, Stream, Event */

/* the error text and the code to return with it (rdsp_chain.hip) */
int chain_fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
#define NEED(c) do { if (!(c)) return RDSP_ERR_INVALID; } while (0)
/* a setter's first line: with rdsp_sdr_set_engine_literal(chain, 1) the `SDR.` / `preProcessor.` calls reach the reference's own objects */
#define TO_ENGINE(c, call) do { NEED(c); if ((c)->engine) return (call); } while (0)

/* a launch returned e != 0 */
static inline int launch_failed(const char *what, int e) {
  return chain_fail(RDSP_ERR_HIP, "%s: %s", what, hipGetErrorString((hipError_t)e));
}
/* one more created event at the back of a pool; a failure leaves the pool as it was */
static inline hipError_t push_event(std::deque<Event> &pool, unsigned flags) {
  pool.emplace_back();
  const hipError_t e = pool.back().create(flags);
  if (e != hipSuccess) pool.pop_back();
  return e;
}

/* One double-buffered per-group table that the front kernels read while the host replaces it (rdsp_slot.h has the protocol):
 * group g's two halves are pool[(g * 2 + half) * words ...], and there are two pinned images with the event of the upload
 * that last read each.  A fill writes the image whose upload is two fills old, so the host never overwrites an image that an
 * earlier, still queued upload has yet to read (streams only wait for uploads on the device; the host does not know when
 * one has run).  Used by rdsp_chain_groups.hip alone. */
struct GroupSlot {
  rdsp_slot::Slot plan;
  size_t words = 0; /* float2 per half and per image */
  PinnedBuf<float> image[2];
  Event ev[2];
  bool issued[2] = {false, false};
  int create(size_t n_words) { /* idempotent */
    words = n_words;
    for (int k = 0; k < 2; k++) {
      if (!ev[k]) HIP_TRY(ev[k].create(hipEventDisableTiming));
      if (!image[k]) HIP_TRY(image[k].alloc(2 * words));
    }
    return RDSP_OK;
  }
  /* the image to write.  The upload that last read it is two fills old: almost always long done; if not (a burst of
   * retunes of one group while the device is calls behind) the host waits for it */
  int begin_fill(float **img) {
    const int si = plan.next_image;
    if (issued[si]) HIP_TRY(hipEventSynchronize(ev[si]));
    *img = image[si];
    return RDSP_OK;
  }
  /* queue that image's upload on `stream`, behind `fence` if there is one: kernels launched so far may still read the
   * target half (it was live before the last switch) */
  int upload(float2 *pool, int group, hipEvent_t fence, hipStream_t stream) {
    const rdsp_slot::Fill f = plan.fill();
    if (fence) HIP_TRY(hipStreamWaitEvent(stream, fence, 0));
    float2 *dst = pool + ((size_t)group * 2 + (size_t)f.target) * words;
    HIP_TRY(hipMemcpyAsync(dst, image[f.image], sizeof(float2) * words, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipEventRecord(ev[f.image], stream));
    issued[f.image] = true;
    return RDSP_OK;
  }
  hipEvent_t last_upload() const { return ev[plan.last_image]; }
  uint32_t live_off(int group) const { return (uint32_t)(((size_t)group * 2 + (size_t)plan.live) * words); }
};

/* host side of one receiver group: filter, tuning offset, demodulator.  The device sees it as one RdspGroup
 * record plus its slots of the mask pool and of the rotated pool; a retune fills the half the record does not point to and
 * the record is rewritten in stream order at the next processing call. */
struct GroupState {
  double lo = 0.0, hi = 0.0, nco_hz = 0.0;
  int demod = RDSP_DEMOD_USB, audio_filter = RDSP_AUDIO_2700;
  std::vector<double> coef_I, coef_Q; /* FIR_Coef_I/Q, CONV:69-70 */
  std::vector<float> mask_nat;        /* FIR_filter_mask, CONV:77 */
  bool dirty = true; /* the device record must be rewritten before the next launch */
  bool has_dev_dphi = false; /* dev_dphi: increment the last launch mixed with */
  uint32_t dev_dphi = 0;
  GroupSlot mask; /* d_mask_pool: N float2, uploaded on the copy stream by a filter change */
  /* d_rot_pool: 4 x RDSP_FD_N float2, valid for the increment rot_dphi.  Derived data: made from the decimator's spectra
   * and the tuning offset on the processing stream, at the commit that follows a retune, a regrouping or a loaded state,
   * never part of the state blob */
  GroupSlot rot;
  bool rot_valid = false;
  uint32_t rot_dphi = 0;
  float iir[20];           /* the group's audio band-pass as four biquads (RDSP_AUDIO_KIND_IIR) */
  bool iir_dirty = true;
};
/* Every device buffer, stream and event below has one owner (rdsp_dev.h), so `delete` releases the object once, whatever
 * set-up call failed half-way.  Nothing may still be queued on an internal stream at that point: rdsp_chain_destroy
 * synchronises s_copy, s_mid and s_tail first.  Those explicit synchronisations are the guarantee, not the order in which
 * the members below are destroyed. */
struct rdsp_chain {
  rdsp_chain_config_t cfg;
  int n_channels, device, max_blocks;
  int N, decim, hop;
  uint64_t n_in;       /* absolute input sample counter */
  int old_nr_level;    /* oldNRLevel, CONV:80 */
  float nr_mu, als_mu;
  long nr_calls, als_calls; /* NR:69 ring statics: only "first call" matters */
  std::vector<float> fir_nat;
  std::deque<GroupState> groups;      /* at least one; a deque: growing it relocates no owner */
  std::vector<uint16_t> group_of;     /* empty: every channel in group 0 */
  /* device */
  DevBuf<RdspGroup> d_groups;
  DevBuf<uint16_t> d_group_of;
  DevBuf<float2> d_mask_pool;         /* [n_groups][2][N] */
  Stream s_copy;                      /* mask uploads, concurrent with processing */
  Event ev_fence;                     /* after the most recent front launch */
  bool fence_valid = false;
  DevBuf<float> d_fir_hc;
  DevBuf<float2> d_fd_mask; /* [4][512] branch spectra of the frequency-domain decimator (decim 4 only) */
  DevBuf<float2> d_rd_mask; /* [4][256] the same for the 256-point windows of the row forms */
  std::vector<float> fd_img;     /* d_fd_mask's contents on the host: what the groups' rotated spectra are made from */
  DevBuf<float2> d_rot_pool;     /* [n_groups][2][4][512] rot_r x d_fd_mask per group (RdspFrontParams::rot_pool); chains of
                                    at most RDSP_FD_ROT_GROUPS groups with decimation 4, else none.  On the one-wave plans
                                    (rdsp_fd_shift_plan) the spectra of fir_nat shifted by the group's increment instead */
  DevBuf<float> d_sin_table; /* [513] sinTable_f32 (spectral stage as written, rdsp_set_spectral_resynthesis); made on first use */
  int spectral_literal = 0;
  /* rdsp_sdr_set_engine_literal: the reference's own pre-processor and engine in front of the CONV stage (INO:53-54,71-86) */
  rdsp_engine_t *engine = nullptr;
  rdsp_preproc_t *pre = nullptr;
  DevBuf<int16_t> d_engine_io; /* [n_channels][max_blocks * 128][2]: what the record queues would hold */
  int nlms_energy_running = 0; /* rdsp_set_nlms_energy_mode */
  DevBuf<uint32_t> d_hist;
  DevBuf<float2> d_prev;
  DevBuf<float> d_scal;
  DevBuf<float> d_nr_w, d_nr_prev, d_nr_energy;
  DevBuf<float> d_als_w, d_als_prev, d_als_energy;
  DevBuf<uint32_t> d_status; /* [2][n_channels] sticky NLMS health words: DSP-NR instance, ALS instance */
  DevBuf<float> d_mid;
  size_t mid_stride = 0;
  /* SAM groups: quadrature part of the base band (three buffers, like d_mid), PLL state */
  DevBuf<float> d_mid_q[3], d_sam;
  /* pipelined mode: the serial tail stage of call k runs on an internal stream,
   * concurrently with the front stage of call k+1 (three intermediate buffers: the front
   * stage of call k+1 never waits for the tail stage of call k-1) */
  int pipe_on = 0;
  Stream s_tail;
  /* the serial per-channel stages between front and tail stage (SAM PLL, IIR cascade) run on a stream
   * of their own when pipelined: three stages in flight, the tail stage waits for ev_mid */
  Stream s_mid;
  Event ev_mid[3];
  /* three intermediate buffers: the front stage may run two calls ahead of the tail stage, so
   * neither stream waits on the other in steady state (with two, every call paid two
   * cross-stream event waits, ~0.1 ms of a 2 ms step) */
  Event ev_front[3], ev_tail[3], ev_misc;
  /* pipelined calls over many channels go out as channel sub-batches: front(A), front(B), ... on the
   * caller's stream, tail(A), tail(B), ... on the tail stream, tail(A) waiting for front(A) only.
   * Every launch then has the shape the kernels' co-residency was balanced for (one tail wave and
   * two front waves per SIMD at 4096 channels), and the halves of one call overlap each other. */
  int sub_batch = 4096;
  std::deque<Event> ev_front_sb[3]; /* [slot][sub-batch], created on first use */
  DevBuf<float> d_midx[2]; /* slots 1 and 2 (slot 0 is d_mid) */
  long call_idx = 0;
  int tail_slot = -1; /* slot of the last call whose tail stage went to s_tail (its ev_tail marks
                         when d_out, the AGC gain and the NLMS state of that call are final); -1: none */
  /* optional per-kernel HIP-event timing (bench.py roofline leg) */
  int timing_on = 0;
  std::deque<Event> ev; /* pool, groups of 4: front begin/end, tail begin/end */
  std::vector<int> ev_has_tail;
  size_t ev_used = 0; /* calls recorded so far */
  int lean_mode = -1; /* -1 auto (= full), 0 full-register front kernel, 1 lean */
  int fir_mode = -1;  /* stage A3 (rdsp_chain_set_fir_variant): 4 frequency domain, one granule per frame (split-
                         invariant bits); -1 (default) that or 5, by what follows the front kernel; 0 direct form; 2
                         frequency domain, 448-sample frames;
                         5 frequency domain on 16-lane rows, 128 outputs per 256-point window (split-invariant);
                         1, 3 and 6 (measured and not adopted, docs/history.md) are never stored */
  /* wave priorities while both kernels share the SIMDs: the direct-form front kernel raises its
   * own to front_fir_prio during the FIR, the frequency-domain one never does; the tail kernel runs
   * at tail_prio throughout.  Round 2, frequency-domain front kernel, tail priority 0 / 1 / 2 / 3:
   * K3 1.191 / - / 1.188 / - ms, K5 2.72 / 2.36 / 2.34 / 2.36 ms per step (at equal priority the tail
   * kernels of two sub-batches are starved by the front waves).  Round 5 looked at the library's default decimator
   * (one granule per frame: half as much front-kernel work again per step), where the tail kernel is the starved one
   * (1.4 - 2.0 ms per launch against 1.06 alone): tail priority 0 instead of 2 measured 1.335-1.513 against 1.423-1.689
   * ms per K3 step in one interleaved A/B, 1.387-1.472 against 1.465-1.543 in a second, and 1.95 against 1.63 under
   * the profiler and 1.83 against 1.50 as a leg of the default bench run -- no consistent gain, so the priority stays 2
   * in every form (tests/micro/prio_default.sh, default_form_trace.sh) */
  int front_fir_prio = 2, tail_prio = 2;
  /* tail kernel (rdsp_launch_tail): 100, rdsp_tail.hip's -- a channel per 16-lane DPP row, two steps per reduction */
  int tail_lpc = 100;
  int saved_agc_mode = RDSP_AGC_MEDIUM, saved_als_mode = RDSP_ALS_NOTCH;
  /* the engine's IIR audio filter bank (RDSP_AUDIO_KIND_IIR): coefficient sets per group, DF1
   * state per channel; allocated by rdsp_sdr_setAudioFilterKind */
  const char *front_name = "rdsp_front_kernel"; /* front kernel of the most recent call (measurement reports) */
  int audio_kind = RDSP_AUDIO_KIND_MASK;
  DevBuf<float> d_iir_coef, d_iir_state;
  int iir_sets = 0;
  int swap_iq = 0;            /* preProcessor.swapIQ, INO:118 */
  int iq_slip = 0;            /* rdsp_pre_setIQslip: +1 delays the I rail by one sample, -1 the Q rail */
  DevBuf<uint32_t> d_slip_buf;         /* [n_channels][max_blocks * 128] corrected words of a call */
  DevBuf<uint32_t> d_slip_carry;       /* [2][n_channels] last raw word of the previous / this call (slip_carry()) */
  int slip_phase = 0;
  uint32_t *slip_carry(int phase) const { return d_slip_carry + (size_t)n_channels * (size_t)phase; }
  bool slip_prev_on = false;  /* the previous call ran with the correction (its history words are corrected ones) */
  /* swap flag and input scales of the previous call (its samples are this call's FIR history) */
  bool hist_valid = false;
  int hist_swap = 0;
  float hist_scale_i = 0.f, hist_scale_q = 0.f;
  int nb_on = 0;              /* SDR.enableNoiseBlanker, BK_INO:1259 */
  float nb_threshold_db = 10.0f;
  /* rdsp_chain_set_tail_law: A8 / A9 as this build's stand-ins (RDSP_TAIL_BUILD) or as the engine's own laws
   * (RDSP_TAIL_ENGINE: rdsp_tail_engine.hip).  The engine law's state ([ch][4] AGC words, [ch][128] ALS line and
   * taps) is allocated by the first switch to it */
  int tail_law = RDSP_TAIL_BUILD;
  int eng_agc_set = 0;        /* the engine AGC's constants: 0 the constructor's (0xdf14), 1 .. 3 setAGCmode's */
  bool eng_als_clear = false; /* enableALSfilter clears the engine ALS line and taps at the next launch (0xdb2c) */
  DevBuf<float> d_eng_st, d_eng_als;
};
int chain_check_device(rdsp_chain_t *c);
/* everything queued on the internal tail stream has finished when this returns */
int chain_drain_tail(rdsp_chain_t *c);
/* the same, then everything queued on the caller's stream: what a read-back or a blocking reset starts with */
int chain_drain_all(rdsp_chain_t *c, void *stream);
/* RdspFrontParams::fir_fd of a chain */
int chain_fir_fd(const rdsp_chain_t *c);
/* in how many channel sub-batches a pipelined call without a SAM group goes out (1: whole) */
int chain_sub_batches(const rdsp_chain_t *c);
int chain_ensure_sub_batch_events(rdsp_chain_t *c);

/* receiver groups (rdsp_chain_groups.hip) */
int chain_check_group(const rdsp_chain_t *c, int group);
int chain_groups_resize(rdsp_chain_t *c, int n);
int chain_group_stage(rdsp_chain_t *c, int gi);
int chain_groups_commit(rdsp_chain_t *c, hipStream_t stream);
int chain_ensure_sam(rdsp_chain_t *c);

/* ---- the per-channel state planes (rdsp_chain_state.hip) --------------------------------------------------------------
 * One description per plane, in blob order.  chain_build allocates the planes every chain has, the set-up call of an
 * optional stage allocates that stage's; rdsp_chain_reset, the build-law branch of rdsp_chain_set_tail_law,
 * rdsp_chain_reset_nlms_channels, save_state and load_state walk the same table.  It is built on control-path calls only
 * and holds no heap memory (rdsp_chain_process does not allocate). */
enum { BOOT_ZERO, BOOT_GAIN_ONE /* d_scal: word 1, the AGC gain, is 1.0f */, BOOT_ENGINE_AGC /* d_eng_st: the active flag is 1 */ };
enum { INST_NONE = -1, INST_NR = 0, INST_ALS = 1 }; /* the NLMS instance a plane belongs to (rdsp_chain_reset_nlms_channels) */
enum { OPT_NONE = 0, OPT_SAM, OPT_IIR, OPT_SLIP, OPT_ENG_TAIL }; /* the optional stage a plane belongs to; OPT_NONE: every chain has it */
struct StatePlane {
  void **slot;        /* the owner's pointer; null while an optional plane is not allocated */
  size_t row, rows;   /* the allocation is [rows][n_channels] planes and this is plane `row` of it (rows 0: not the allocating entry) */
  size_t per_channel; /* bytes */
  int boot, inst, opt;
  bool present() const { return *slot != nullptr; }
  unsigned char *at(const rdsp_chain_t *c, size_t ch) const { return (unsigned char *)*slot + (row * (size_t)c->n_channels + ch) * per_channel; }
};
std::array<StatePlane, 16> chain_planes(rdsp_chain_t *c);
/* allocate and boot the planes of one optional stage (OPT_NONE: of every chain) that are not there yet */
int chain_planes_create(rdsp_chain_t *c, int opt);
/* channels [first, first + n) of a plane as a fresh chain has them; blocking */
int chain_plane_boot(rdsp_chain_t *c, const StatePlane &pl, int first, int n);
/* the AGC gain (d_scal word 1) of channels [first, first + n) back to 1, the plane's other words kept or zeroed */
int chain_gain_one(rdsp_chain_t *c, int first, int n, bool keep_rest);

#endif
