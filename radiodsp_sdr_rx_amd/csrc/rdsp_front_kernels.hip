/*
 * rdsp_front_kernels.hip -- the three front-kernel families, compiled as ONE translation unit.
 *
 * Each of the three files stands on its own (its kernel, its LDS plan, its launch entry; it compiles alone), but the
 * library builds them together, because the compiler's view of the whole unit reaches into the kernels: the
 * transform helpers of the 512-point radix-8 plan (rdsp_fft.h) are shared by every rdsp_front_fd_kernel (its
 * decimator), by rdsp_front_kernel<512, 8, ...> and by rdsp_front_rd_kernel<512, 8, ...>.  Device functions are
 * internal to a unit, so what the optimizer infers about such a helper comes from all of its callers in the unit.
 * Compiled apart, six instances of rdsp_front_kernel<512, 8> and two of rdsp_front_rd_kernel<512, 8> come out with
 * other instruction streams (a few instructions shorter or longer, other register allocation); the other 80 kernels
 * are the same either way.  These kernels sit at their register limits and their speed is measured, not assumed:
 * until the other code has been measured on the GPU, the unit stays whole.
 */
#include "rdsp_front_direct.hip"
#include "rdsp_front_fd.hip"
#include "rdsp_front_rd.hip"
