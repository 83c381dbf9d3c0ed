/*
 * rdsp_graph_sdr.hip -- the device nodes of the block graph but the biquad's: the chain (below), the two integer analysers
 * (one node struct) and the reference's own engine and pre-processor.  The SDR engine node first: the role of
 * `AudioSDR SDR;` (+ the convolutional stage that loop() runs between the record
 * and play queues) in RadioDSP_SDR_RX.ino:53-54,81-89.  Two inputs (I, Q tiles),
 * two outputs (L, R tiles).  update() gathers input tiles until the chain's
 * granule is available (the `available() > N_BLOCKS` gate of
 * RDSP_convolutional.h:231), runs the GPU chain on them and hands the audio out
 * one 128-sample tile pair per tick.  Every compute step is rdsp_chain_process;
 * there is no host DSP here.
 */
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include <deque>
#include <vector>

#include "rdsp_host.h"
#include "rdsp_node_dev.h"
#include "rdsp_q15_host.h"

using namespace rdsp_node_dev;

namespace {
struct SdrNode : NodeDev<> {
  rdsp_chain_t *chain;
  int n_channels, gran, decim;
  int have; /* input blocks staged */
  std::vector<int16_t> h_iq;  /* [ch][gran*128][2] */
  std::vector<int16_t> h_out; /* [ch][gran*128/decim][2] */
  std::deque<std::vector<int16_t>> out_l, out_r; /* audio tiles waiting for a tick */
};

void sdr_update(rdsp_node_t *n, void *u) {
  SdrNode *s = node_of<SdrNode>(u);
  rdsp_block_t *bi = rdsp_receive_readonly(n, 0);
  rdsp_block_t *bq = rdsp_receive_readonly(n, 1);
  if (bi && bq) {
    tiles_to_pairs(rdsp_block_data(bi), rdsp_block_data(bq), s->n_channels, s->h_iq.data(), (size_t)s->gran * RDSP_BLOCK_SAMPLES,
                   (size_t)s->have * RDSP_BLOCK_SAMPLES);
    s->have++;
  }
  rdsp_release(bi); /* a lone I or Q block is dropped, like a node returning early */
  rdsp_release(bq);

  if (s->have == s->gran) {
    const size_t in_row = (size_t)s->gran * RDSP_BLOCK_SAMPLES;
    const size_t out_row = in_row / (size_t)s->decim;
    /* a chain in pipelined mode finishes d_out on its internal tail stream: the flush makes the copy back wait for it */
    const bool ok = s->run("sdr node", s->h_iq.data(), s->h_iq.size(), [&](int16_t *d_iq, int16_t *d_out, hipStream_t st) {
      const int rc = rdsp_chain_process(s->chain, d_iq, in_row, s->gran, d_out, out_row, nullptr, st);
      return rc != RDSP_OK ? rc : rdsp_chain_flush(s->chain, st);
    }, s->h_out.data(), s->h_out.size());
    for (size_t t = 0; ok && t < out_row / RDSP_BLOCK_SAMPLES; t++) {
      std::vector<int16_t> L((size_t)s->n_channels * RDSP_BLOCK_SAMPLES), R(L.size());
      pairs_to_tiles(s->h_out.data(), out_row, t * RDSP_BLOCK_SAMPLES, s->n_channels, L.data(), R.data());
      s->out_l.push_back(std::move(L));
      s->out_r.push_back(std::move(R));
    }
    s->have = 0;
  }

  if (!s->out_l.empty()) {
    rdsp_block_t *bl = rdsp_allocate(n), *br = rdsp_allocate(n);
    if (bl && br) {
      memcpy(rdsp_block_data(bl), s->out_l.front().data(), s->out_l.front().size() * sizeof(int16_t));
      memcpy(rdsp_block_data(br), s->out_r.front().data(), s->out_r.front().size() * sizeof(int16_t));
      s->out_l.pop_front();
      s->out_r.pop_front();
      rdsp_transmit(n, bl, 0);
      rdsp_transmit(n, br, 1);
    }
    rdsp_release(bl);
    rdsp_release(br);
  }
}
}  // namespace

extern "C" rdsp_node_t *rdsp_sdr_node_create(rdsp_graph_t *g, rdsp_chain_t *chain) {
  if (!g || !chain || rdsp_graph_channels(g) != rdsp_chain_channels(chain)) {
    rdsp_set_error("rdsp_sdr_node_create: graph and chain must have the same channel count");
    return nullptr;
  }
  SdrNode *s = new SdrNode();
  s->chain = chain;
  s->n_channels = rdsp_chain_channels(chain);
  s->gran = rdsp_chain_call_unit_blocks(chain); /* one call per call unit: a fixed split, the same grid on every run */
  s->decim = rdsp_chain_decim(chain);
  s->have = 0;
  const size_t in_n = (size_t)s->n_channels * s->gran * RDSP_BLOCK_SAMPLES * 2;
  s->h_iq.assign(in_n, 0);
  s->h_out.assign(in_n / s->decim, 0);
  return make_node(g, 2, sdr_update, s, "rdsp_sdr_node_create", rdsp_chain_device(chain), in_n, in_n / s->decim);
}

extern "C" int rdsp_sdr_node_status(rdsp_node_t *n) { return node_status(n); }

/* ---- the two integer analysers as graph nodes ------------------------------------------
 * `AudioAnalyzeFFT256IQ FFT;` with `AudioConnection(preProcessor, 0, FFT, 0)` and (.., 1, FFT, 1) in the sketch
 * (RadioDSP_SDR_RX.ino:57,73-74; analyze_fft256iq.h:52-110): two inputs (I, Q tiles), 256 bins, update() is
 * FFTIQ.cpp:65-118 for every channel of the tile -- the tick's blocks are interleaved, uploaded and handed to
 * rdsp_spectrum_update (which keeps the previous block on the device).  `AudioAnalyzeFFT1024 AudioFFT;` fed from Q_out_L
 * (INO:57,87): one input, uploaded from its block, 512 bins.  Neither has outputs; available() / output[] / read() follow
 * FFTIQ.h:62-86,99, the range form of read() by each class's own rule (rdsp_q15_tables.c). */
namespace {
struct AnalyserNode : NodeDev<uint16_t> {
  typedef int (*Call)(void *obj, int16_t *d_in, uint16_t *d_out, int *n_out, hipStream_t st);
  void *obj = nullptr; /* the analyser, and one block of every channel through its update */
  Call call = nullptr;
  const char *name = "";
  int n_channels = 0, inputs = 0, inclusive = 0;
  unsigned bins = 0;
  std::vector<int16_t> h_in;   /* two inputs: [ch][128][2] */
  std::vector<uint16_t> h_out; /* [ch][bins] */
  int outputflag = 0;          /* FFTIQ.h:63 */
};

void analyser_update(rdsp_node_t *n, void *u) {
  AnalyserNode *s = node_of<AnalyserNode>(u);
  rdsp_block_t *b0 = rdsp_receive_readonly(n, 0); /* FFTIQ.cpp:70-71 */
  rdsp_block_t *b1 = s->inputs == 2 ? rdsp_receive_readonly(n, 1) : nullptr;
  if (!b0 || (s->inputs == 2 && !b1)) { /* FFTIQ.cpp:72: return when a block is missing */
    rdsp_release(b0);
    rdsp_release(b1);
    return;
  }
  const int16_t *h_in = rdsp_block_data(b0);
  if (s->inputs == 2) {
    tiles_to_pairs(rdsp_block_data(b0), rdsp_block_data(b1), s->n_channels, s->h_in.data(), RDSP_BLOCK_SAMPLES, 0);
    h_in = s->h_in.data();
    rdsp_release(b0); /* FFTIQ.cpp:114-115 (the previous block lives on the device) */
    rdsp_release(b1);
    b0 = nullptr;
  }
  int n_out = 0;
  const bool ok = s->run(s->name, h_in, (size_t)s->n_channels * RDSP_BLOCK_SAMPLES * s->inputs,
                         [&](int16_t *d_in, uint16_t *d_out, hipStream_t st) { return s->call(s->obj, d_in, d_out, &n_out, st); },
                         s->h_out.data(), s->h_out.size(), &n_out);
  rdsp_release(b0); /* a lone input: after the synchronize, the upload read it */
  if (ok && n_out > 0) s->outputflag = 1; /* FFTIQ.cpp:112 */
}
rdsp_node_t *analyser_create(rdsp_graph_t *g, const char *who, const char *name, void *obj, AnalyserNode::Call call, int device,
                             int inputs, unsigned bins, int inclusive) {
  AnalyserNode *s = new AnalyserNode();
  s->obj = obj; s->call = call; s->name = name;
  s->n_channels = rdsp_graph_channels(g);
  s->inputs = inputs; s->bins = bins; s->inclusive = inclusive;
  const size_t n_in = (size_t)s->n_channels * RDSP_BLOCK_SAMPLES * inputs;
  if (inputs == 2) s->h_in.assign(n_in, 0);
  s->h_out.assign((size_t)s->n_channels * bins, 0);
  return make_node(g, inputs, analyser_update, s, who, device, n_in, s->h_out.size());
}
/* FFTIQ.h:62-68: true once per finished average, cleared by the call */
int analyser_available(rdsp_node_t *n) {
  AnalyserNode *s = node_of<AnalyserNode>(rdsp_node_user(n));
  if (!s) return 0;
  const int f = s->outputflag;
  s->outputflag = 0;
  return f;
}
/* FFTIQ.h:99 `uint16_t output[256]` of every channel: [n_channels][bins], valid until the next update */
const uint16_t *analyser_output(rdsp_node_t *n) {
  AnalyserNode *s = node_of<AnalyserNode>(rdsp_node_user(n));
  return s ? s->h_out.data() : nullptr;
}
/* read(bin) / read(binFirst, binLast) of channel `ch` (FFTIQ.h:70-86) */
const uint16_t *analyser_row(rdsp_node_t *n, int ch, AnalyserNode **s) {
  *s = node_of<AnalyserNode>(rdsp_node_user(n));
  return (!*s || ch < 0 || ch >= (*s)->n_channels) ? nullptr : (*s)->h_out.data() + (size_t)ch * (*s)->bins;
}
float analyser_read(rdsp_node_t *n, int ch, unsigned int binNumber) {
  AnalyserNode *s;
  const uint16_t *row = analyser_row(n, ch, &s);
  return row ? rdsp_q15_read(row, s->bins, binNumber) : 0.0f;
}
float analyser_read_range(rdsp_node_t *n, int ch, unsigned int binFirst, unsigned int binLast) {
  AnalyserNode *s;
  const uint16_t *row = analyser_row(n, ch, &s);
  return row ? rdsp_q15_read_range(row, s->bins, binFirst, binLast, s->inclusive) : 0.0f;
}
int spectrum_call(void *o, int16_t *d_iq, uint16_t *d_out, int *n_out, hipStream_t st) {
  return rdsp_spectrum_update(static_cast<rdsp_spectrum_t *>(o), d_iq, RDSP_BLOCK_SAMPLES, 1, d_out, 1, n_out, st);
}
int fft1024_call(void *o, int16_t *d_in, uint16_t *d_out, int *n_out, hipStream_t st) {
  return rdsp_fft1024_update(static_cast<rdsp_fft1024_t *>(o), d_in, RDSP_BLOCK_SAMPLES, 1, 1, d_out, 1, n_out, st);
}
}  // namespace

extern "C" rdsp_node_t *rdsp_spectrum_node_create(rdsp_graph_t *g, rdsp_spectrum_t *spec) {
  if (!g || !spec) {
    rdsp_set_error("rdsp_spectrum_node_create: bad argument");
    return nullptr;
  }
  return analyser_create(g, "rdsp_spectrum_node_create", "spectrum node", spec, spectrum_call, spec->device, 2, 256, 0);
}
extern "C" rdsp_node_t *rdsp_fft1024_node_create(rdsp_graph_t *g, rdsp_fft1024_t *an) {
  if (!g || !an || an->n_channels != rdsp_graph_channels(g)) {
    rdsp_set_error("rdsp_fft1024_node_create: bad argument (the analyser needs the graph's channel count)");
    return nullptr;
  }
  return analyser_create(g, "rdsp_fft1024_node_create", "fft1024 node", an, fft1024_call, an->device, 1, 512, 1);
}
extern "C" int rdsp_spectrum_node_available(rdsp_node_t *n) { return analyser_available(n); }
extern "C" const uint16_t *rdsp_spectrum_node_output(rdsp_node_t *n) { return analyser_output(n); }
extern "C" float rdsp_spectrum_node_read(rdsp_node_t *n, int ch, unsigned int bin) { return analyser_read(n, ch, bin); }
extern "C" float rdsp_spectrum_node_read_range(rdsp_node_t *n, int ch, unsigned int first, unsigned int last) { return analyser_read_range(n, ch, first, last); }
extern "C" int rdsp_spectrum_node_status(rdsp_node_t *n) { return node_status(n); }
extern "C" int rdsp_fft1024_node_available(rdsp_node_t *n) { return analyser_available(n); }
extern "C" const uint16_t *rdsp_fft1024_node_output(rdsp_node_t *n) { return analyser_output(n); }
extern "C" float rdsp_fft1024_node_read(rdsp_node_t *n, int ch, unsigned int bin) { return analyser_read(n, ch, bin); }
extern "C" float rdsp_fft1024_node_read_range(rdsp_node_t *n, int ch, unsigned int first, unsigned int last) { return analyser_read_range(n, ch, first, last); }
extern "C" int rdsp_fft1024_node_status(rdsp_node_t *n) { return node_status(n); }

/* ---- the reference's own engine objects as graph nodes -------------------------------------------------------------------
 * `AudioSDRpreProcessor preProcessor;` and `AudioSDR SDR;` (RadioDSP_SDR_RX.ino:53-54) wired as INO:71-72,81-86: two inputs
 * (I, Q tiles), two outputs, one block per tick like the library's update().  The arithmetic is rdsp_preproc_update /
 * rdsp_engine_update (csrc/rdsp_preproc.hip, csrc/rdsp_engine.hip and its stage files); the node only carries tiles to the device and back. */
namespace {
struct PairNode : NodeDev<> {
  rdsp_engine_t *engine = nullptr;
  rdsp_preproc_t *pre = nullptr;
  int n_channels = 0;
  std::vector<int16_t> h_in, h_out; /* [ch][128][2] */
};
void pair_update(rdsp_node_t *n, void *u) {
  PairNode *s = node_of<PairNode>(u);
  rdsp_block_t *bi = rdsp_receive_readonly(n, 0), *bq = rdsp_receive_readonly(n, 1);
  if (!bi || !bq) { /* the library's update() returns when a block is missing (image 0xe756 ... 0xe77a, 0xeea4 ... 0xeebc) */
    rdsp_release(bi);
    rdsp_release(bq);
    return;
  }
  tiles_to_pairs(rdsp_block_data(bi), rdsp_block_data(bq), s->n_channels, s->h_in.data(), RDSP_BLOCK_SAMPLES, 0);
  rdsp_release(bi);
  rdsp_release(bq);
  const bool ok = s->run("engine node", s->h_in.data(), s->h_in.size(), [&](int16_t *d_in, int16_t *d_out, hipStream_t st) {
    return s->engine ? rdsp_engine_update(s->engine, d_in, RDSP_BLOCK_SAMPLES, 1, d_out, RDSP_BLOCK_SAMPLES, st)
                     : rdsp_preproc_update(s->pre, d_in, RDSP_BLOCK_SAMPLES, 1, d_out, RDSP_BLOCK_SAMPLES, st);
  }, s->h_out.data(), s->h_out.size());
  if (!ok) return;
  rdsp_block_t *b0 = rdsp_allocate(n), *b1 = rdsp_allocate(n);
  if (b0 && b1) {
    pairs_to_tiles(s->h_out.data(), RDSP_BLOCK_SAMPLES, 0, s->n_channels, rdsp_block_data(b0), rdsp_block_data(b1));
    rdsp_transmit(n, b0, 0);
    rdsp_transmit(n, b1, 1);
  }
  rdsp_release(b0);
  rdsp_release(b1);
}
rdsp_node_t *pair_create(rdsp_graph_t *g, rdsp_engine_t *engine, rdsp_preproc_t *pre) {
  const int nch = engine ? rdsp_engine_channels(engine) : rdsp_preproc_channels(pre);
  if (!g || rdsp_graph_channels(g) != nch) {
    rdsp_set_error("engine / pre-processor node: graph and object must have the same channel count");
    return nullptr;
  }
  PairNode *s = new PairNode();
  s->engine = engine; s->pre = pre; s->n_channels = nch;
  s->h_in.assign((size_t)nch * RDSP_BLOCK_SAMPLES * 2, 0);
  s->h_out.assign(s->h_in.size(), 0);
  return make_node(g, 2, pair_update, s, "engine / pre-processor node", engine ? rdsp_engine_device(engine) : rdsp_preproc_device(pre),
                   s->h_in.size(), s->h_in.size());
}
}  // namespace

extern "C" rdsp_node_t *rdsp_engine_node_create(rdsp_graph_t *g, rdsp_engine_t *e) { return e ? pair_create(g, e, nullptr) : nullptr; }
extern "C" rdsp_node_t *rdsp_preproc_node_create(rdsp_graph_t *g, rdsp_preproc_t *p) { return p ? pair_create(g, nullptr, p) : nullptr; }
extern "C" int rdsp_engine_node_status(rdsp_node_t *n) { return node_status(n); }
