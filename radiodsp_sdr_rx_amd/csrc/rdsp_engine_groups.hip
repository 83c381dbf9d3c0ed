/*
 * rdsp_engine_groups.hip -- the receiver groups of rdsp_engine_t (rdsp_engine_host.h has the object).
 * The sketch has ONE receiver, so one mode, one audio filter, one AGC setting; an object of many channels
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
#include "rdsp_engine_host.h"

extern "C" {

namespace {
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

}  // extern "C"
