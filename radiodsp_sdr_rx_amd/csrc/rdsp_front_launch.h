/*
 * rdsp_front_launch.h -- host side of the front kernels, between rdsp_launch_front (rdsp_kernels.hip) and the three
 * files that hold the kernel families.  rdsp_front_pick decides the instance; each family file exposes one entry that
 * turns the record into its template arguments and launches.  The entries decide nothing: a record that names an
 * instance the build does not carry is hipErrorInvalidValue.
 */
#ifndef RDSP_FRONT_LAUNCH_H
#define RDSP_FRONT_LAUNCH_H

#include <mutex>
#include <type_traits>

#include "rdsp_kernels.h"

namespace rdsp {

int front_direct_launch(int fft_l, int decim, const RdspFrontPick &k, const RdspFrontParams *p, int n_channels, hipStream_t stream);
int front_fd_launch(int fft_l, const RdspFrontPick &k, const RdspFrontParams *p, int n_channels, hipStream_t stream);
int front_rd_launch(int fft_l, const RdspFrontPick &k, const RdspFrontParams *p, int n_channels, hipStream_t stream);

/* FFT_L and the radix the kernels run it with, as template arguments: f(FrontPlan<N, P>{}); `other` for any other FFT_L */
template <int N_, int P_>
struct FrontPlan {
  static constexpr int N = N_, P = P_;
};
template <typename R, typename F>
R with_front_plan(int fft_l, R other, F f) {
  switch (fft_l) {
    case 256: return f(FrontPlan<256, 4>{});
    case 512: return f(FrontPlan<512, 8>{});
    case 1024: return f(FrontPlan<1024, 16>{});
    case 2048: return f(FrontPlan<2048, 8>{});
    case 4096: return f(FrontPlan<4096, 16>{});
    default: return other;
  }
}
/* a flag of the record as a template argument: f(std::true_type{}) or f(std::false_type{}) */
template <typename F>
int with_flag(int flag, F f) {
  return flag ? f(std::true_type{}) : f(std::false_type{});
}

/* the raised dynamic-LDS limit is a per-device property of a kernel function: one bit per device,
 * set under a lock (chains on several devices may launch from several host threads) */
template <auto Kernel> /* one flag set per kernel instance */
int ensure_lds_limit(size_t lds) {
  static std::mutex mu;
  static uint64_t done = 0;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev > 63) return (int)hipErrorInvalidDevice;
  std::lock_guard<std::mutex> lk(mu);
  if (!((done >> dev) & 1u)) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
    done |= (uint64_t)1 << dev;
  }
  return 0;
}

}  // namespace rdsp

#endif
