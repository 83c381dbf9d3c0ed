/*
 * rdsp_stream.hip -- streaming runner: host source -> HBM ->
 * receive chain -> HBM -> host sink, what loop() + the I2S DMA do in the sketch
 * (RadioDSP_SDR_RX.ino:195-198; queues RDSP_convolutional.h:231-244,344-349),
 * for recorded IQ.  Three HIP streams (upload, compute, download) over two
 * slots of pinned host memory, so that reading the next batch, the PCIe copies
 * and the kernels of consecutive batches overlap; the host only ever waits for
 * the download of the batch before the one it just queued.
 */
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>

#include "rdsp_dev.h"
#include "rdsp_host.h"

namespace {
using namespace rdsp_dev;

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

/* what a run has done so far */
struct Progress {
  int64_t blocks = 0;
  double t_read = 0.0, t_write = 0.0; /* inside the source and the sink */
  const double t_begin = now_s();
};
void fill_stats(rdsp_stream_stats_t *stats, const Progress &r, int decim) {
  if (!stats) return;
  stats->blocks = r.blocks;
  stats->samples_in = r.blocks * RDSP_BLOCK_SAMPLES;
  stats->samples_out = r.blocks * RDSP_BLOCK_SAMPLES / decim;
  stats->seconds = now_s() - r.t_begin;
  stats->read_seconds = r.t_read;
  stats->write_seconds = r.t_write;
}

int check_call_unit(rdsp_chain_t *c, int blocks_per_call) {
  const int gran = rdsp_chain_call_unit_blocks(c);
  if (blocks_per_call <= 0 || blocks_per_call % gran != 0) {
    rdsp_set_error("blocks_per_call %d is not a multiple of the call unit %d", blocks_per_call, gran);
    return RDSP_ERR_NOT_READY;
  }
  return RDSP_OK;
}
/* a run's buffers, streams and events live on the chain's device, whatever the calling thread had selected (a host that
 * drives several GPUs from one process) */
int use_chain_device(rdsp_chain_t *c) {
  if (hipSetDevice(rdsp_chain_device(c)) != hipSuccess) {
    rdsp_set_error("hipSetDevice(%d) failed", rdsp_chain_device(c));
    return RDSP_ERR_HIP;
  }
  return RDSP_OK;
}

/* The three streams and two device slots both runners drive: batch `it` goes through slot it & 1, uploaded on s_up, computed
 * on s_comp, downloaded on s_down; the events order a slot's three steps and keep batch it + 2 off a slot still in use.
 * Rows are IQ pairs per channel; `contiguous` is a whole slot in one copy (host rows at the slot's pitch, all of them full). */
struct Pipeline {
  rdsp_chain_t *c = nullptr;
  size_t nch = 0, in_row = 0, out_row = 0; /* a slot: [nch][in_row][2] in, [nch][out_row][2] out */
  DevBuf<int16_t> din[2], dout[2];
  Stream s_up, s_comp, s_down;
  Event ev_up[2], ev_comp[2], ev_down[2];

  int create(rdsp_chain_t *chain, int blocks_per_call) {
    c = chain;
    nch = (size_t)rdsp_chain_channels(c);
    in_row = (size_t)blocks_per_call * RDSP_BLOCK_SAMPLES;
    out_row = in_row / (size_t)rdsp_chain_decim(c);
    for (int i = 0; i < 2; i++) {
      HIP_TRY(din[i].alloc(in_row * 2 * nch));
      HIP_TRY(dout[i].alloc(out_row * 2 * nch));
      HIP_TRY(ev_up[i].create(hipEventDisableTiming));
      HIP_TRY(ev_comp[i].create(hipEventDisableTiming));
      HIP_TRY(ev_down[i].create(hipEventDisableTiming));
    }
    HIP_TRY(s_up.create(hipStreamNonBlocking));
    HIP_TRY(s_comp.create(hipStreamNonBlocking));
    HIP_TRY(s_down.create(hipStreamNonBlocking));
    return RDSP_OK;
  }
  /* after the compute of two batches ago has finished reading din[slot] */
  int upload(int slot, int64_t it, const int16_t *src, size_t src_pitch, size_t pairs, bool contiguous) {
    if (it >= 2) HIP_TRY(hipStreamWaitEvent(s_up, ev_comp[slot], 0));
    if (contiguous) HIP_TRY(hipMemcpyAsync(din[slot], src, in_row * 4 * nch, hipMemcpyHostToDevice, s_up));
    else HIP_TRY(hipMemcpy2DAsync(din[slot], in_row * 4, src, src_pitch * 4, pairs * 4, nch, hipMemcpyHostToDevice, s_up));
    HIP_TRY(hipEventRecord(ev_up[slot], s_up));
    return RDSP_OK;
  }
  /* needs the upload, and dout[slot] drained by the download of two batches ago; s_down then waits for the whole chain of
   * this batch (pipelined mode: its tail stage) */
  int compute(int slot, int64_t it, int blocks) {
    HIP_TRY(hipStreamWaitEvent(s_comp, ev_up[slot], 0));
    if (it >= 2) HIP_TRY(hipStreamWaitEvent(s_comp, ev_down[slot], 0));
    RC_TRY(rdsp_chain_process(c, din[slot], in_row, blocks, dout[slot], out_row, nullptr, s_comp));
    HIP_TRY(hipEventRecord(ev_comp[slot], s_comp));
    HIP_TRY(hipStreamWaitEvent(s_down, ev_comp[slot], 0));
    return rdsp_chain_flush(c, s_down);
  }
  int download(int slot, int16_t *dst, size_t dst_pitch, size_t pairs, bool contiguous) {
    if (contiguous) HIP_TRY(hipMemcpyAsync(dst, dout[slot], out_row * 4 * nch, hipMemcpyDeviceToHost, s_down));
    else HIP_TRY(hipMemcpy2DAsync(dst, dst_pitch * 4, dout[slot], out_row * 4, pairs * 4, nch, hipMemcpyDeviceToHost, s_down));
    HIP_TRY(hipEventRecord(ev_down[slot], s_down));
    return RDSP_OK;
  }
  int wait_up(int slot) { HIP_TRY(hipEventSynchronize(ev_up[slot])); return RDSP_OK; }
  int wait_down(int slot) { HIP_TRY(hipEventSynchronize(ev_down[slot])); return RDSP_OK; }
  void drain() { /* before a run returns, failed or not: nothing of it is in flight when its buffers go */
    for (hipStream_t s : {s_up.s, s_comp.s, s_down.s})
      if (s) (void)hipStreamSynchronize(s);
  }
};

/* the staged runner: the callbacks fill and empty two slots of pinned host memory, so that reading the next batch, the copies
 * and the kernels of consecutive batches overlap; the host only ever waits for the download of the batch before the one it
 * just queued */
struct Staged {
  Pipeline p;
  PinnedBuf<int16_t> hin[2], hout[2];
  int out_pairs[2] = {0, 0}; /* what hout[slot] holds for the sink */
  rdsp_sink_fn sink;
  void *sink_user;

  int hand_over(int slot, Progress &r) {
    if (out_pairs[slot] <= 0) return RDSP_OK;
    RC_TRY(p.wait_down(slot));
    const double t0 = now_s();
    const int w = sink(sink_user, hout[slot], p.out_row, out_pairs[slot]); /* Q_out_L/R.playBuffer(), CONV:344-349 */
    r.t_write += now_s() - t0;
    out_pairs[slot] = 0;
    if (w < 0) {
      rdsp_set_error("stream sink failed (%d)", w);
      return RDSP_ERR_INVALID;
    }
    return RDSP_OK;
  }
  int run(rdsp_chain_t *c, rdsp_source_fn source, void *source_user, int blocks_per_call, int64_t max_blocks, Progress &r) {
    const int gran = rdsp_chain_call_unit_blocks(c), decim = rdsp_chain_decim(c);
    RC_TRY(p.create(c, blocks_per_call));
    for (int i = 0; i < 2; i++) {
      HIP_TRY(hin[i].alloc(p.in_row * 2 * p.nch));
      HIP_TRY(hout[i].alloc(p.out_row * 2 * p.nch));
    }
    int64_t it = 0;
    for (bool ended = false; !ended; it++) {
      const int slot = (int)(it & 1);
      int want = blocks_per_call;
      if (max_blocks > 0 && max_blocks - r.blocks < (int64_t)want) want = (int)(max_blocks - r.blocks);
      want -= want % gran;
      if (want <= 0) break;
      if (it >= 2) RC_TRY(p.wait_up(slot)); /* the pinned input slot is free again */
      const double t0 = now_s();
      int got = source(source_user, hin[slot], p.in_row, want); /* Q_in_L/R.readBuffer(), CONV:236-244 */
      r.t_read += now_s() - t0;
      if (got < 0) {
        rdsp_set_error("stream source failed (%d)", got);
        return RDSP_ERR_INVALID;
      }
      if (got < want) ended = true; /* the sketch would keep waiting for a full granule (CONV:231): stop */
      got -= got % gran;
      if (got > 0) {
        const bool full = got == blocks_per_call;
        RC_TRY(p.upload(slot, it, hin[slot], p.in_row, (size_t)got * RDSP_BLOCK_SAMPLES, full));
        RC_TRY(p.compute(slot, it, got));
        out_pairs[slot] = got * RDSP_BLOCK_SAMPLES / decim;
        RC_TRY(p.download(slot, hout[slot], p.out_row, (size_t)out_pairs[slot], full));
        r.blocks += got;
      }
      RC_TRY(hand_over(slot ^ 1, r)); /* the previous batch goes to the sink while this one is in flight */
    }
    return hand_over((int)((it - 1) & 1), r); /* the last batch */
  }
};
}  // namespace

extern "C" int rdsp_stream_run(rdsp_chain_t *c, rdsp_source_fn source, void *source_user, rdsp_sink_fn sink,
                               void *sink_user, int blocks_per_call, int64_t max_blocks,
                               rdsp_stream_stats_t *stats) {
  if (!c || !source || !sink || blocks_per_call <= 0) {
    rdsp_set_error("rdsp_stream_run: bad argument");
    return RDSP_ERR_INVALID;
  }
  RC_TRY(check_call_unit(c, blocks_per_call));
  RC_TRY(use_chain_device(c));
  Staged st;
  st.sink = sink;
  st.sink_user = sink_user;
  Progress r;
  const int rc = st.run(c, source, source_user, blocks_per_call, max_blocks, r);
  st.p.drain();
  fill_stats(stats, r, rdsp_chain_decim(c));
  return rc;
}

/* ---- files: one reader and one writer per channel ------------------------------------ */
struct FileEnds {
  rdsp_iq_reader_t *const *readers;
  rdsp_audio_writer_t *const *writers;
  int nch;
};

static int file_source(void *user, int16_t *dst, size_t stride_pairs, int n_blocks) {
  FileEnds *fe = (FileEnds *)user;
  const size_t want = (size_t)n_blocks * RDSP_BLOCK_SAMPLES;
  size_t least = want;
#pragma omp parallel for schedule(dynamic, 1) reduction(min : least)
  for (int ch = 0; ch < fe->nch; ch++) {
    const size_t got = rdsp_iq_reader_read(fe->readers[ch], dst + (size_t)ch * stride_pairs * 2, want);
    if (got < least) least = got;
  }
  return (int)(least / RDSP_BLOCK_SAMPLES); /* the shortest recording ends the run */
}

static int file_sink(void *user, const int16_t *src, size_t stride_pairs, int n_pairs) {
  FileEnds *fe = (FileEnds *)user;
  int bad = 0;
#pragma omp parallel for schedule(dynamic, 1) reduction(+ : bad)
  for (int ch = 0; ch < fe->nch; ch++)
    if (rdsp_audio_writer_write(fe->writers[ch], src + (size_t)ch * stride_pairs * 2, (size_t)n_pairs) != (size_t)n_pairs) bad++;
  return bad ? -1 : n_pairs;
}

extern "C" int rdsp_stream_run_files(rdsp_chain_t *c, rdsp_iq_reader_t *const *readers,
                                     rdsp_audio_writer_t *const *writers, int blocks_per_call,
                                     int64_t max_blocks, rdsp_stream_stats_t *stats) {
  if (!c || !readers || !writers) return RDSP_ERR_INVALID;
  FileEnds fe = {readers, writers, rdsp_chain_channels(c)};
  for (int i = 0; i < fe.nch; i++)
    if (!readers[i] || !writers[i]) {
      rdsp_set_error("channel %d has no reader/writer", i);
      return RDSP_ERR_INVALID;
    }
  return rdsp_stream_run(c, file_source, &fe, file_sink, &fe, blocks_per_call, max_blocks, stats);
}

/* ---- memory: host arrays [n_channels][stride] at both ends ------------------------------ */
struct MemEnds {
  const int16_t *in;
  size_t in_stride;
  int64_t blocks_left, in_pos;
  int16_t *out;
  size_t out_stride;
  int64_t out_pos;
  int nch;
};

static int mem_source(void *user, int16_t *dst, size_t stride_pairs, int n_blocks) {
  MemEnds *m = (MemEnds *)user;
  const int take = (int)((int64_t)n_blocks < m->blocks_left ? (int64_t)n_blocks : m->blocks_left);
  const size_t pairs = (size_t)take * RDSP_BLOCK_SAMPLES;
#pragma omp parallel for schedule(static)
  for (int ch = 0; ch < m->nch; ch++)
    memcpy(dst + (size_t)ch * stride_pairs * 2, m->in + ((size_t)ch * m->in_stride + (size_t)m->in_pos) * 2, pairs * 4);
  m->in_pos += (int64_t)pairs;
  m->blocks_left -= take;
  return take;
}

static int mem_sink(void *user, const int16_t *src, size_t stride_pairs, int n_pairs) {
  MemEnds *m = (MemEnds *)user;
#pragma omp parallel for schedule(static)
  for (int ch = 0; ch < m->nch; ch++)
    memcpy(m->out + ((size_t)ch * m->out_stride + (size_t)m->out_pos) * 2, src + (size_t)ch * stride_pairs * 2, (size_t)n_pairs * 4);
  m->out_pos += n_pairs;
  return n_pairs;
}

/* both arrays page-locked (hipHostMalloc / hipHostRegister / torch pin_memory): the DMA engines
 * read and write them directly, no staging slots and no host copies */
static bool is_pinned_host(const void *p) {
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return a.type == hipMemoryTypeHost;
}

static int pinned_batches(Pipeline &p, rdsp_chain_t *c, const int16_t *host_iq, size_t in_stride, int64_t n_blocks, int16_t *host_out,
                          size_t out_stride, int blocks_per_call, Progress &r) {
  const int gran = rdsp_chain_call_unit_blocks(c);
  const size_t decim = (size_t)rdsp_chain_decim(c);
  RC_TRY(p.create(c, blocks_per_call));
  for (int64_t it = 0; r.blocks < n_blocks; it++) {
    const int slot = (int)(it & 1);
    int take = (int)((n_blocks - r.blocks) < (int64_t)blocks_per_call ? (n_blocks - r.blocks) : (int64_t)blocks_per_call);
    take -= take % gran;
    if (take <= 0) break;
    const size_t at = (size_t)r.blocks * RDSP_BLOCK_SAMPLES, pairs = (size_t)take * RDSP_BLOCK_SAMPLES;
    RC_TRY(p.upload(slot, it, host_iq + at * 2, in_stride, pairs, false));
    RC_TRY(p.compute(slot, it, take));
    RC_TRY(p.download(slot, host_out + at / decim * 2, out_stride, pairs / decim, false));
    r.blocks += take;
  }
  return RDSP_OK;
}
static int stream_pinned(rdsp_chain_t *c, const int16_t *host_iq, size_t in_stride, int64_t n_blocks, int16_t *host_out,
                         size_t out_stride, int blocks_per_call, rdsp_stream_stats_t *stats) {
  RC_TRY(check_call_unit(c, blocks_per_call));
  RC_TRY(use_chain_device(c));
  Pipeline p;
  Progress r;
  const int rc = pinned_batches(p, c, host_iq, in_stride, n_blocks, host_out, out_stride, blocks_per_call, r);
  p.drain();
  fill_stats(stats, r, rdsp_chain_decim(c));
  return rc;
}

extern "C" int rdsp_stream_run_memory(rdsp_chain_t *c, const int16_t *host_iq, size_t in_stride_pairs,
                                      int64_t n_blocks, int16_t *host_out, size_t out_stride_pairs,
                                      int blocks_per_call, rdsp_stream_stats_t *stats) {
  if (!c || !host_iq || !host_out || n_blocks <= 0) return RDSP_ERR_INVALID;
  const int decim = rdsp_chain_decim(c);
  if (in_stride_pairs < (size_t)n_blocks * RDSP_BLOCK_SAMPLES ||
      out_stride_pairs < (size_t)n_blocks * RDSP_BLOCK_SAMPLES / (size_t)decim) {
    rdsp_set_error("rdsp_stream_run_memory: strides too small");
    return RDSP_ERR_INVALID;
  }
  if (is_pinned_host(host_iq) && is_pinned_host(host_out))
    return stream_pinned(c, host_iq, in_stride_pairs, n_blocks, host_out, out_stride_pairs, blocks_per_call, stats);
  MemEnds m = {host_iq, in_stride_pairs, n_blocks, 0, host_out, out_stride_pairs, 0, rdsp_chain_channels(c)};
  return rdsp_stream_run(c, mem_source, &m, mem_sink, &m, blocks_per_call, n_blocks, stats);
}
