/*
 * rdsp_chain_groups.hip -- the device side of rdsp_chain_t's receiver groups: resize, the staging of a group's
 * mask and of its rotated branch spectra into their double-buffered slots (GroupSlot, rdsp_chain_int.h), the device records
 * and their commit in stream order; the regrouping entry points.  What selects a group's filter and demodulator is
 * rdsp_chain_select.hip.
 */
#include "rdsp_chain_int.h"

/* ---- receiver groups: double-buffered slots, records rewritten in stream order ---- */
static const size_t kRotImg = 4 * (size_t)RDSP_FD_N; /* float2 of one group's rotated branch spectra (one half) */
/* the fence behind the front kernels launched so far, if any was */
static hipEvent_t group_fence(const rdsp_chain_t *c) { return c->fence_valid ? (hipEvent_t)c->ev_fence : nullptr; }
/* (re)allocate the device side for n groups; existing groups keep their settings,
 * new ones copy group 0.  Synchronous: called at create time and from
 * rdsp_chain_set_groups, never on the streaming path. */
int chain_groups_resize(rdsp_chain_t *c, int n) {
  HIP_TRY(hipDeviceSynchronize());
  if (!c->s_copy) HIP_TRY(c->s_copy.create(hipStreamNonBlocking));
  if (!c->ev_fence) HIP_TRY(c->ev_fence.create(hipEventDisableTiming));
  const size_t old = c->groups.size();
  while (c->groups.size() > (size_t)n) c->groups.pop_back();
  while (c->groups.size() < (size_t)n) c->groups.emplace_back();
  for (size_t i = 0; i < (size_t)n; i++) {
    GroupState &g = c->groups[i];
    if (i >= old) {
      if (i > 0) {
        const GroupState &g0 = c->groups[0];
        g.lo = g0.lo; g.hi = g0.hi; g.nco_hz = g0.nco_hz; g.demod = g0.demod; g.audio_filter = g0.audio_filter;
        g.coef_I = g0.coef_I; g.coef_Q = g0.coef_Q; g.mask_nat = g0.mask_nat;
        memcpy(g.iir, g0.iir, sizeof(g.iir));
      } else {
        for (int st = 0; st < 4; st++) {
          g.iir[5 * st] = 1.0f;
          g.iir[5 * st + 1] = g.iir[5 * st + 2] = g.iir[5 * st + 3] = g.iir[5 * st + 4] = 0.0f;
        }
        g.coef_I.assign(c->hop + 1, 0.0);
        g.coef_Q.assign(c->hop + 1, 0.0);
        g.mask_nat.assign(2 * (size_t)c->N, 0.0f);
      }
    }
    RC_TRY(g.mask.create((size_t)c->N));
  }
  c->d_groups.release();
  c->d_mask_pool.release();
  c->d_rot_pool.release();
  HIP_TRY(alloc_zero(c->d_groups, (size_t)n));
  HIP_TRY(alloc_zero(c->d_mask_pool, 2 * (size_t)c->N * (size_t)n));
  /* the rotated branch spectra of the frequency-domain decimator, per group while the groups are few (rdsp_kernels.h) */
  const bool rot = c->decim == 4 && n <= RDSP_FD_ROT_GROUPS;
  if (rot) HIP_TRY(alloc_zero(c->d_rot_pool, 2 * kRotImg * (size_t)n));
  for (auto &g : c->groups) { /* pool contents are gone: every group restages */
    g.mask.plan.reset();
    g.rot.plan.reset();
    g.dirty = true;
    g.rot_valid = false;
    if (rot) RC_TRY(g.rot.create(kRotImg));
  }
  c->fence_valid = false;
  return RDSP_OK;
}

/* queue the upload of group gi's current mask (all-pass when the filter is off)
 * into the half of its slot that its device record does not point to; never blocks the
 * processing stream (the reference does this under AudioNoInterrupts, CONV:211-222) */
int chain_group_stage(rdsp_chain_t *c, int gi) {
  GroupState &g = c->groups[(size_t)gi];
  float *img;
  RC_TRY(g.mask.begin_fill(&img));
  rdsp_mask_device_image(c->cfg.filter_on ? g.mask_nat.data() : nullptr, c->N, img);
  RC_TRY(g.mask.upload(c->d_mask_pool, gi, group_fence(c), c->s_copy));
  g.dirty = true;
  return RDSP_OK;
}

static float2 nco_rot(uint32_t dphi, int k) {
  float t[2];
  rdsp_nco_rot(dphi, k, t);
  return make_float2(t[0], t[1]);
}
static void group_record(const rdsp_chain_t *c, const GroupState &g, int gi, RdspGroup *r) {
  memset(r, 0, sizeof(*r));
  r->dphi = rdsp_nco_dphi(g.nco_hz, c->cfg.fs_in);
  r->demod = (g.demod == RDSP_DEMOD_IQ) ? RDSP_K_DEMOD_IQ
             : (g.demod == RDSP_DEMOD_AM ? RDSP_K_DEMOD_AM
                : (g.demod == RDSP_DEMOD_SAM ? RDSP_K_DEMOD_SAM : RDSP_K_DEMOD_REAL));
  r->rot1 = nco_rot(r->dphi, 1);
  r->rot2 = nco_rot(r->dphi, 2);
  r->rot3 = nco_rot(r->dphi, 3);
  const int nt = c->N / rdsp_plan_radix(c->N); /* threads per channel */
  r->rotp1 = nco_rot(r->dphi, 4 * nt);
  r->rotp2 = nco_rot(r->dphi, 8 * nt);
  r->rotp3 = nco_rot(r->dphi, 12 * nt);
  r->rotq1 = nco_rot(r->dphi, 256);
  r->rotq2 = nco_rot(r->dphi, 512);
  r->rotq3 = nco_rot(r->dphi, 768);
  r->mask_off = g.mask.live_off(gi);
  r->rot_off = c->d_rot_pool ? g.rot.live_off(gi) : 0u;
  /* the FIR history was mixed with the increment of the launch that brought it in */
  r->dphi_hist = g.has_dev_dphi ? g.dev_dphi : r->dphi;
  r->roth1 = nco_rot(r->dphi_hist, 1);
  r->roth2 = nco_rot(r->dphi_hist, 2);
  r->roth3 = nco_rot(r->dphi_hist, 3);
  r->rothp3 = nco_rot(r->dphi_hist, 12 * nt);
}

/* Group gi's rotated branch spectra for its current tuning offset -- where the NCO runs behind the decimator, the spectra of
 * the shifted taps (rdsp_fd_shift_plan) -- into the half of its slot that the device record does not point to; the record written right behind it (chain_groups_commit) switches over.  The copy is queued on the
 * processing stream itself, behind every front kernel launched so far (the fence covers launches on another stream), so
 * nothing that still reads that half -- it was live two retunes ago -- runs beside it. */
static int group_stage_rot(rdsp_chain_t *c, int gi, uint32_t dphi, hipStream_t stream) {
  GroupState &g = c->groups[(size_t)gi];
  float *img;
  RC_TRY(g.rot.begin_fill(&img));
  if (rdsp_fd_shift_plan(c->N)) { /* the NCO behind the decimator: the spectra of the shifted taps */
    if (rdsp_fd_shift_image(c->fir_nat.data(), RDSP_FD_N, dphi, img) != 0) return chain_fail(RDSP_ERR_NOMEM, "shifted branch spectra");
  } else {
    rdsp_fd_rot_image(c->fd_img.data(), RDSP_FD_N, dphi, img);
  }
  RC_TRY(g.rot.upload(c->d_rot_pool, gi, group_fence(c), stream));
  g.rot_dphi = dphi;
  g.rot_valid = true;
  return RDSP_OK;
}

/* before a launch on `stream`: switch every changed group over, in stream order */
int chain_groups_commit(rdsp_chain_t *c, hipStream_t stream) {
  for (size_t i = 0; i < c->groups.size(); i++) {
    GroupState &g = c->groups[i];
    if (!g.dirty) continue;
    /* the mask went up on the copy stream; the rotated spectra go up on `stream` itself */
    if (g.mask.plan.pending >= 0) HIP_TRY(hipStreamWaitEvent(stream, g.mask.last_upload(), 0));
    if (c->d_rot_pool) { /* a retune, a regrouping, the chain's first call: the slot follows the tuning offset */
      const uint32_t dphi = rdsp_nco_dphi(g.nco_hz, c->cfg.fs_in);
      if (!g.rot_valid || g.rot_dphi != dphi) RC_TRY(group_stage_rot(c, (int)i, dphi, stream));
    }
    g.mask.plan.switch_over();
    g.rot.plan.switch_over();
    RdspGroup r;
    group_record(c, g, (int)i, &r);
    int e = rdsp_launch_group_store(c->d_groups + i, &r, stream);
    if (e != 0) return launch_failed("group record update failed", e);
    /* after a tuning change the record is written once more, for the launch after this one */
    g.dirty = (r.dphi_hist != r.dphi);
    g.has_dev_dphi = true;
    g.dev_dphi = r.dphi;
  }
  return RDSP_OK;
}

int chain_check_group(const rdsp_chain_t *c, int group) {
  if (!c || group < 0 || (size_t)group >= c->groups.size())
    return chain_fail(RDSP_ERR_INVALID, "group %d out of range", group);
  return RDSP_OK;
}

/* ---- receiver groups ---------------------------------------------------- */
extern "C" int rdsp_chain_groups(const rdsp_chain_t *c) { return c ? (int)c->groups.size() : 0; }

/* partition the channels into n_groups receiver groups; group_of_channel[ch] < n_groups
 * (NULL with n_groups == 1 restores the single shared group).  Synchronises the
 * device: a set-up call, not a streaming one.  New groups start as copies of group 0. */
extern "C" int rdsp_chain_set_groups(rdsp_chain_t *c, int n_groups, const uint16_t *group_of_channel) {
  NEED(c);
  if (n_groups < 1 || n_groups > 65535 || (n_groups > 1 && !group_of_channel))
    return chain_fail(RDSP_ERR_INVALID, "rdsp_chain_set_groups: bad argument");
  RC_TRY(chain_check_device(c));
  if (group_of_channel)
    for (int i = 0; i < c->n_channels; i++)
      if (group_of_channel[i] >= n_groups)
        return chain_fail(RDSP_ERR_INVALID, "channel %d: group %d >= n_groups %d", i, (int)group_of_channel[i], n_groups);
  RC_TRY(chain_drain_tail(c));
  /* documented as synchronising: the caller's processing stream is not known here and may be a
   * non-blocking one (no null-stream sync covers it), and the group tables below are freed and
   * reallocated -- every kernel that may still read them has finished after this */
  HIP_TRY(hipDeviceSynchronize());
  RC_TRY(chain_groups_resize(c, n_groups));
  c->d_group_of.release();
  c->group_of.clear();
  if (group_of_channel && n_groups > 1) {
    c->group_of.assign(group_of_channel, group_of_channel + c->n_channels);
    HIP_TRY(c->d_group_of.alloc((size_t)c->n_channels));
    HIP_TRY(hipMemcpy(c->d_group_of, c->group_of.data(), sizeof(uint16_t) * (size_t)c->n_channels, hipMemcpyHostToDevice));
  }
  /* with the IIR bank selected, re-selecting it stages every group's mask (side-band selector) and
   * coefficient set; otherwise the masks alone */
  if (c->audio_kind == RDSP_AUDIO_KIND_IIR) return rdsp_sdr_setAudioFilterKind(c, RDSP_AUDIO_KIND_IIR, nullptr);
  for (int g = 0; g < n_groups; g++) RC_TRY(chain_group_stage(c, g));
  return RDSP_OK;
}

extern "C" int rdsp_group_get_mask(rdsp_chain_t *c, int group, float *host_out) {
  if (chain_check_group(c, group) != RDSP_OK || !host_out) return RDSP_ERR_INVALID;
  memcpy(host_out, c->groups[(size_t)group].mask_nat.data(), sizeof(float) * 2 * (size_t)c->N);
  return RDSP_OK;
}

/* PLL state and the quadrature intermediates of the SAM demodulator: allocated when a group is
 * first switched to SAMmode (a control-path call), not by the processing call */
int chain_ensure_sam(rdsp_chain_t *c) {
  if (c->d_sam) return RDSP_OK;
  RC_TRY(chain_check_device(c));
  for (auto &q : c->d_mid_q)
    if (!q) HIP_TRY(q.alloc(c->mid_stride * (size_t)c->n_channels));
  return chain_planes_create(c, OPT_SAM); /* last: d_sam says that all of it is there */
}
