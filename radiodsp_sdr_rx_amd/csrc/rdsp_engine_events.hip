/*
 * rdsp_engine_events.hip -- rdsp_engine_gather_events' kernels: the digits, frames and messages the decoders emitted in the last
 * call, gathered into dense payload words with a {channel, kind | n_words << 8, seq, offset} record each, channel ascending, then
 * kind, then seq (include/rdsp.h has the definition, rdsp_events.h its plain loop and every rule used here).  Integers only;
 * compiled with the engine's flags like the rest of the engine.  Three launches a call, no atomics, nothing that waits on another
 * workgroup, after the model of rdsp_engine_pack.hip:
 *
 * rdsp_engine_events_count_kernel: one wave per channel, four channels a workgroup, no LDS, no barrier (a wave past the last
 * channel leaves at once).  Per kind the wave reads the channel's `new` records 64 blocks a trip -- a ballot's population count
 * for DTMF, a wave sum for the other two -- and the count word; a kind that is off, or whose decoder did not run on the channel
 * in the last call (p.ran), counts nothing.  A channel has at most 16 + 4 + 4 items: lane l holds DTMF item l (l < 16), AFSK item
 * l - 16 (l < 20) or POCSAG item l - 20 (l < 24), oldest first, so the lanes' order is the sequence's.  A lane below its kind's
 * take reads its slot's header word and derives n_words; lane 0 writes {events, words, lost, the three takes} into chan[ch].
 * rdsp_engine_events_scan_kernel: one workgroup walks the channels in ascending chunks of 1024, as rdsp_engine_pack_scan_kernel
 * does: a wave scan inside a wave, the waves' totals added in wave order through LDS, the chunks in chunk order, for the three
 * sums at once.  chan[ch] becomes {first event, first word, ...}; the totals are needed_events, needed_words and lost; the
 * written counts are the needed ones when everything fits and 0 without a capacity for events.
 * rdsp_engine_events_gather_kernel: the count kernel's shape, launched only with a capacity for events.  The wave walks its
 * channel's items in lane order, everything about an item wave-uniform: lanes 0 ... 20 load the slot 16 bytes each and store 16
 * bytes where the item's offset is a multiple of four words and the four words are the payload's, else word by word; lane 0
 * writes the record with one 16-byte store.  An item that does not fit ends the wave's walk; it is the sequence's first such
 * item exactly when the event before it fits, which its own index and offset tell, and then lane 0 writes written_events and
 * written_words: one wave at most does.  Nothing at or behind `written` is written, and no slot is read past its 84 words.
 */
#include <hip/hip_runtime.h>

#include "rdsp_engine_events.h"

using namespace rdsp_eng;
using namespace rdsp_events;

namespace {
constexpr int EW = 256, ECH = EW / 64; /* the count's and the gather's workgroup: four waves, four channels */
constexpr int SW = 1024;               /* the scan's workgroup */
constexpr int L_AFSK = 16, L_POCSAG = 20, L_END = 24; /* the lanes of a channel's items */

/* the sum of v over the wave, in every lane */
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d);
  return v;
}
/* a kind's c of channel ch: the same value in every lane */
__device__ __forceinline__ uint32_t count_new(const EventsParams &p, int kind, int ch, int lane) {
  const uint8_t *rec = p.fresh[kind] + (size_t)ch * p.rec_stride;
  uint32_t c = 0;
  for (int b0 = 0; b0 < p.n_blocks; b0 += 64) {
    const int b = b0 + lane;
    const uint32_t v = b < p.n_blocks ? (uint32_t)rec[b] : (kind == EV_DTMF ? 255u : 0u);
    if (kind == EV_DTMF) c += (uint32_t)__popcll(__ballot(v != 255u));
    else c += v;
  }
  return kind == EV_DTMF ? c : wave_sum(c);
}
/* the three takes in one word, eight bits each */
__device__ __forceinline__ int take_at(int takes, int kind) { return (takes >> (8 * kind)) & 0xFF; }

/* the item a lane holds */
struct Item {
  int kind, slot;     /* slot: the ring slot's index */
  uint32_t seq, n_words; /* n_words 0: the lane holds none */
  int rank;           /* the item's place among the channel's */
};
__device__ __forceinline__ const uint32_t *slot_of(const EventsParams &p, int ch, int kind, int slot) {
  const Layout l = layout(kind);
  return p.state[kind] + (size_t)ch * (size_t)l.words + l.ring + (size_t)slot * (size_t)l.slot_words;
}
__device__ __forceinline__ Item item_of(const EventsParams &p, int ch, int lane, int takes) {
  Item it;
  it.kind = lane < L_AFSK ? EV_DTMF : lane < L_POCSAG ? EV_AFSK : EV_POCSAG;
  const int i = lane - (lane < L_AFSK ? 0 : lane < L_POCSAG ? L_AFSK : L_POCSAG);
  const int take = take_at(takes, it.kind);
  it.rank = i + (it.kind > EV_DTMF ? take_at(takes, EV_DTMF) : 0) + (it.kind > EV_AFSK ? take_at(takes, EV_AFSK) : 0);
  it.seq = 0u; it.slot = 0; it.n_words = 0u;
  if (lane < L_END && i < take) { /* take > 0: the kind is on and p.state[kind] is there */
    const Layout l = layout(it.kind);
    const uint32_t n = p.state[it.kind][(size_t)ch * (size_t)l.words + l.count];
    it.seq = n - (uint32_t)take + (uint32_t)i;
    it.slot = (int)(it.seq % (uint32_t)l.slots);
    it.n_words = payload_words(it.kind, slot_of(p, ch, it.kind, it.slot)[0]);
  }
  return it;
}
}  // namespace

__global__ __launch_bounds__(EW) void rdsp_engine_events_count_kernel(const EventsParams p) {
  const int lane = (int)threadIdx.x & 63;
  const int ch = (int)blockIdx.x * ECH + ((int)threadIdx.x >> 6);
  if (ch >= p.n_channels) return;
  int takes = 0, events = 0;
  uint32_t lost_sum = 0;
#pragma unroll
  for (int kind = 0; kind < KINDS; kind++) {
    if (!p.state[kind] || !p.ran[(size_t)kind * (size_t)p.n_channels + ch]) continue; /* wave-uniform */
    const Layout l = layout(kind);
    const uint32_t c = count_new(p, kind, ch, lane);
    const uint32_t n = p.state[kind][(size_t)ch * (size_t)l.words + l.count];
    uint32_t take, lost;
    take_of(c, n, (uint32_t)l.slots, take, lost);
    takes |= (int)take << (8 * kind);
    events += (int)take;
    lost_sum += lost;
  }
  const uint32_t words = wave_sum(item_of(p, ch, lane, takes).n_words);
  if (lane == 0) p.chan[ch] = make_int4(events, (int)words, (int)lost_sum, takes);
}

__global__ __launch_bounds__(SW) void rdsp_engine_events_scan_kernel(const EventsParams p) {
  __shared__ int wave_count[3][SW / 64];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int base[3] = {0, 0, 0};
  for (int c0 = 0; c0 < p.n_channels; c0 += SW) { /* the same trips for every thread */
    const int c = c0 + tid;
    const int4 v = c < p.n_channels ? p.chan[c] : make_int4(0, 0, 0, 0);
    const int n[3] = {v.x, v.y, v.z};
    int upto[3] = {v.x, v.y, v.z}; /* the counts of the wave's lanes 0 ... lane */
    for (int d = 1; d < 64; d <<= 1) {
#pragma unroll
      for (int q = 0; q < 3; q++) {
        const int t = __shfl_up(upto[q], d);
        if (lane >= d) upto[q] += t;
      }
    }
    if (lane == 63) { wave_count[0][wave] = upto[0]; wave_count[1][wave] = upto[1]; wave_count[2][wave] = upto[2]; }
    __syncthreads();
    int before[3] = {base[0], base[1], base[2]}, total[3] = {0, 0, 0};
    for (int k = 0; k < SW / 64; k++) {
#pragma unroll
      for (int q = 0; q < 3; q++) {
        if (k < wave) before[q] += wave_count[q][k];
        total[q] += wave_count[q][k];
      }
    }
    if (c < p.n_channels) p.chan[c] = make_int4(before[0] + upto[0] - n[0], before[1] + upto[1] - n[1], v.z, v.w);
#pragma unroll
    for (int q = 0; q < 3; q++) base[q] += total[q];
    __syncthreads(); /* wave_count is written again */
  }
  if (tid == 0) {
    p.counts[0] = base[0]; p.counts[2] = base[1]; p.counts[4] = base[2];
    const bool all = base[0] <= p.capacity_events && base[1] <= p.capacity_words;
    if (all || p.capacity_events == 0) { /* otherwise the gather's wave that meets the first event outside writes them */
      p.counts[1] = all ? base[0] : 0;
      p.counts[3] = all ? base[1] : 0;
    }
  }
}

__global__ __launch_bounds__(EW) void rdsp_engine_events_gather_kernel(const EventsParams p) {
  const int lane = (int)threadIdx.x & 63;
  const int ch = (int)blockIdx.x * ECH + ((int)threadIdx.x >> 6);
  if (ch >= p.n_channels) return;
  const int4 c = p.chan[ch];
  if ((c.w & 0xFFFFFF) == 0) return; /* no items */
  const Item it = item_of(p, ch, lane, c.w);
  int upto = (int)it.n_words; /* the words of lanes 0 ... lane */
  for (int d = 1; d < 64; d <<= 1) {
    const int t = __shfl_up(upto, d);
    if (lane >= d) upto += t;
  }
  const uint32_t my_offset = (uint32_t)c.y + (uint32_t)upto - it.n_words;
  unsigned long long m = __ballot(it.n_words != 0u);
  while (m) { /* wave-uniform: the items in lane order */
    const int src = __ffsll(m) - 1;
    m &= m - 1ull;
    const int kind = __shfl(it.kind, src), slot = __shfl(it.slot, src);
    const uint32_t seq = (uint32_t)__shfl((int)it.seq, src), n_words = (uint32_t)__shfl((int)it.n_words, src);
    const uint32_t k = (uint32_t)(c.x + __shfl(it.rank, src)), offset = (uint32_t)__shfl((int)my_offset, src);
    if (!fits(k, offset, n_words, (uint32_t)p.capacity_events, (uint32_t)p.capacity_words)) {
      /* the sequence's first event outside: none before it, or the one before it fits (it ends where this one begins) */
      if (lane == 0 && (k == 0u || (k - 1u < (uint32_t)p.capacity_events && offset <= (uint32_t)p.capacity_words))) {
        p.counts[1] = (int)k;
        p.counts[3] = (int)offset;
      }
      return;
    }
    const uint32_t *from = slot_of(p, ch, kind, slot);
    uint32_t *to = p.words + offset;
    if (kind == EV_DTMF) {
      if (lane == 0) to[0] = from[0];
    } else if (4u * (uint32_t)lane < n_words) { /* n_words <= 84: lanes 0 ... 20, inside the slot's 21 x 16 bytes */
      const uint4 v = ((const uint4 *)from)[lane];
      const uint32_t w0 = 4u * (uint32_t)lane;
      if ((offset & 3u) == 0u && w0 + 4u <= n_words) {
        ((uint4 *)to)[lane] = v;
      } else {
        to[w0] = v.x;
        if (w0 + 1u < n_words) to[w0 + 1u] = v.y;
        if (w0 + 2u < n_words) to[w0 + 2u] = v.z;
        if (w0 + 3u < n_words) to[w0 + 3u] = v.w;
      }
    }
    if (lane == 0) p.records[k] = make_int4(ch, (int)((uint32_t)kind | n_words << 8), (int)seq, (int)offset);
  }
}

hipError_t rdsp_engine_events_launch(const EventsParams &p, hipStream_t s) {
  const dim3 per_channel((unsigned)((p.n_channels + ECH - 1) / ECH));
  hipLaunchKernelGGL(rdsp_engine_events_count_kernel, per_channel, dim3(EW), 0, s, p);
  hipLaunchKernelGGL(rdsp_engine_events_scan_kernel, dim3(1), dim3(SW), 0, s, p);
  if (p.capacity_events > 0) hipLaunchKernelGGL(rdsp_engine_events_gather_kernel, per_channel, dim3(EW), 0, s, p);
  return hipGetLastError();
}
