/*
 * rdsp_node_dev.h -- what the graph nodes that run a device object have in common: the device and the status word
 * (NodeBase: the node's user pointer points at it, whatever the kind of node, so that destroy_node and every *_node_status
 * read it without knowing the kind), an input and an output buffer and a stream on the object's device (NodeDev), one
 * tile's round trip through them (NodeDev::run), the node made of a user struct derived from a NodeDev (make_node), and the
 * planar tiles <-> interleaved pairs copies.
 */
#ifndef RDSP_NODE_DEV_H
#define RDSP_NODE_DEV_H

#include "rdsp_dev.h"

namespace rdsp_node_dev {

struct NodeBase {
  int device = 0, status = RDSP_OK;
};
/* the user struct of kind T behind a node's user pointer; the status of any device node */
template <typename T> T *node_of(void *u) { return static_cast<T *>(static_cast<NodeBase *>(u)); }
static inline int node_status(rdsp_node_t *n) {
  const NodeBase *b = static_cast<NodeBase *>(rdsp_node_user(n));
  return b ? b->status : RDSP_ERR_INVALID;
}

template <typename Out = int16_t>
struct NodeDev : NodeBase {
  rdsp_dev::Stream stream;
  rdsp_dev::DevBuf<int16_t> d_in;
  rdsp_dev::DevBuf<Out> d_out;

  bool create(int dev, size_t n_in, size_t n_out) { /* the buffers and the stream live where the object does */
    device = dev;
    return hipSetDevice(dev) == hipSuccess && d_in.alloc(n_in) == hipSuccess && d_out.alloc(n_out) == hipSuccess &&
           stream.create(hipStreamDefault) == hipSuccess;
  }
  /* upload h_in[n_in], rc = call(d_in, d_out, stream), download h_out[n_out] (only while *gate > 0 where a gate is given:
   * the call sets it), synchronize.  false: `status` holds the object's refusal, or RDSP_ERR_HIP and the error text
   * "<name>: ..." */
  template <typename Call>
  bool run(const char *name, const int16_t *h_in, size_t n_in, Call call, Out *h_out, size_t n_out, const int *gate = nullptr) {
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipMemcpyAsync(d_in, h_in, n_in * sizeof(int16_t), hipMemcpyHostToDevice, stream);
    int rc = RDSP_OK;
    if (e == hipSuccess) rc = call(d_in.p, d_out.p, stream.s);
    if (e == hipSuccess && rc == RDSP_OK && n_out > 0 && (!gate || *gate > 0))
      e = hipMemcpyAsync(h_out, d_out, n_out * sizeof(Out), hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess && rc == RDSP_OK) e = hipStreamSynchronize(stream);
    if (e == hipSuccess && rc == RDSP_OK) return true;
    status = (rc != RDSP_OK) ? rc : RDSP_ERR_HIP;
    if (e != hipSuccess) rdsp_set_error("%s: %s", name, hipGetErrorString(e));
    return false;
  }
};

template <typename T>
void destroy_node(void *u) {
  T *s = node_of<T>(u);
  (void)hipSetDevice(s->device);
  delete s;
}
/* the node of the freshly made *s, which it owns from here on: nullptr (and *s deleted) when the device or the graph refuses */
template <typename T>
rdsp_node_t *make_node(rdsp_graph_t *g, int ninputs, rdsp_update_fn update, T *s, const char *who, int device, size_t n_in,
                       size_t n_out) {
  rdsp_node_t *n = nullptr;
  NodeBase *u = s;
  if (!s->create(device, n_in, n_out)) rdsp_set_error("%s: device allocation failed", who);
  else n = rdsp_node_create(g, ninputs, update, u);
  if (n) rdsp_node_set_destructor(n, destroy_node<T>);
  else destroy_node<T>(u);
  return n;
}

/* planar tiles I, Q [ch][128] -> pairs [ch][row][2], at sample `at` of every row; and back */
static inline void tiles_to_pairs(const int16_t *pi, const int16_t *pq, int nch, int16_t *pairs, size_t row, size_t at) {
  for (int c = 0; c < nch; c++) {
    int16_t *dst = pairs + ((size_t)c * row + at) * 2;
    const int16_t *si = pi + (size_t)c * RDSP_BLOCK_SAMPLES, *sq = pq + (size_t)c * RDSP_BLOCK_SAMPLES;
    for (int i = 0; i < RDSP_BLOCK_SAMPLES; i++) {
      dst[2 * i] = si[i];
      dst[2 * i + 1] = sq[i];
    }
  }
}
static inline void pairs_to_tiles(const int16_t *pairs, size_t row, size_t at, int nch, int16_t *o0, int16_t *o1) {
  for (int c = 0; c < nch; c++) {
    const int16_t *src = pairs + ((size_t)c * row + at) * 2;
    for (int i = 0; i < RDSP_BLOCK_SAMPLES; i++) {
      o0[(size_t)c * RDSP_BLOCK_SAMPLES + i] = src[2 * i];
      o1[(size_t)c * RDSP_BLOCK_SAMPLES + i] = src[2 * i + 1];
    }
  }
}

}  // namespace rdsp_node_dev
#endif
