// conv_common.h -- what the convolution kernels (conv_*_impl.h) share: vector types, the raw buffer resource, the dynamic-LDS attribute
// and the launch tail on the host side; the workgroup remap, leaky_relu, compile-time loops and reciprocal division on the device side.
#pragma once
#include <atomic>
#include <type_traits>
#include <utility>

#include "film_kernels.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float bf4 __attribute__((ext_vector_type(4)));
typedef int bi4 __attribute__((ext_vector_type(4)));

enum : int {
  CONV_B_XCD_M = 4,  // XCD-contiguous block mapping (each XCD walks a contiguous range of M tiles)
};

// raw buffer resource over [p, p + 4 GiB): stride 0, num_records = 0xFFFFFFFF bytes, gfx9 dword3 for raw
// 32-bit access.  A lane whose offset is 0xFFFFFFFF fails the bounds check and loads zeros.
typedef __amdgpu_buffer_rsrc_t conv_rsrc_t;
__device__ __forceinline__ conv_rsrc_t conv_make_rsrc(const void* p) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, -1, 0x00020000);
}

__device__ __forceinline__ bf4 conv_buf_load(conv_rsrc_t rsrc, unsigned voff, unsigned soff) {
  return __builtin_bit_cast(bf4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)voff, (int)soff, 0));
}

// ---- host: the dynamic-LDS attribute, the launch tail, the reciprocals -------------------------------------------------------------

// hipFuncAttributeMaxDynamicSharedMemorySize belongs to the function ON the current device and is idempotent: set on the first launch
// per (kernel instantiation, device).  The "already set" flags are atomics (relaxed is enough: a second thread that misses the flag
// only repeats the call) - several handles on several host threads may launch the same instantiation (include/film_hip.h).
struct ConvLdsAttrFlags { std::atomic<bool> set[64]; };
inline hipError_t conv_allow_dynamic_lds(const void* kern, ConvLdsAttrFlags& flags, int bytes) {
  int dev = 0;
  (void)hipGetDevice(&dev);
  const bool tracked = dev >= 0 && dev < 64;
  if (tracked && flags.set[dev].load(std::memory_order_relaxed)) return hipSuccess;
  const hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e == hipSuccess && tracked) flags.set[dev].store(true, std::memory_order_relaxed);
  return e;
}

// The tail of a launcher.  KERN is the kernel instantiation itself, so every instantiation has its own flags.  lds_allow = the dynamic LDS
// the instantiation may ask for over all its launches (the attribute is set once): above 64 KB it needs the attribute.
template <auto KERN>
hipError_t conv_launch(dim3 grid, dim3 block, size_t lds, hipStream_t s, const ConvParams& p, size_t lds_allow) {
  if (lds_allow > 64 * 1024) {
    static ConvLdsAttrFlags attr_flags;
    if (const hipError_t e = conv_allow_dynamic_lds(reinterpret_cast<const void*>(KERN), attr_flags, (int)lds_allow); e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(KERN, grid, block, lds, s, p);
  return hipGetLastError();
}
template <auto KERN>
hipError_t conv_launch(dim3 grid, dim3 block, size_t lds, hipStream_t s, const ConvParams& p) { return conv_launch<KERN>(grid, block, lds, s, p, lds); }

// ceil(2^32 / d) for conv_udiv: exact for x < xmax when xmax d < 2^32 (else `exact` turns false); 0 says the divisor is 1
inline unsigned conv_magic(unsigned long long d, unsigned long long xmax, bool& exact) {
  if (d <= 1) return 0u;
  if (xmax * d >= (1ull << 32)) { exact = false; return 0u; }
  return (unsigned)(((1ull << 32) + d - 1) / d);
}

// ---- device ----------------------------------------------------------------------------------------------------------------------

// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>): every index a compile-time constant
template <class F, int... G>
__device__ __forceinline__ void conv_for_each(F&& f, std::integer_sequence<int, G...>) { (f(std::integral_constant<int, G>{}), ...); }

// x / d by conv_magic's reciprocal, x and magic uniform; magic = 0 says d = 1 (a scalar select spelled out: hipcc made a branch around
// the s_mul_hi_u32)
__device__ __forceinline__ unsigned conv_udiv(unsigned x, unsigned magic) {
  unsigned q;
  const unsigned h = __umulhi(x, magic);
  asm("s_cmp_eq_u32 %2, 0\n\ts_cselect_b32 %0, %1, %3" : "=s"(q) : "s"(x), "s"(magic), "s"(h) : "scc");
  return q;
}

// CONV_B_XCD_M: workgroups are dealt to the 8 XCDs round robin; linear workgroup -> the block it would be if each XCD walked a contiguous
// range of the launch (neighbouring M tiles share halo rows and weights in one XCD's L2)
// (bx, by) = blockIdx.x, blockIdx.y on entry.  conv_wino2d / conv_fold4 spell the same remap out with the grid from their argument batch and
// the quotient by conv_udiv; conv_wino43 deals block pairs.
__device__ __forceinline__ void conv_xcd_remap(int& bx, int& by) {
  const int nbx = gridDim.x, nby = gridDim.y;
  const int nwg = nbx * nby;
  const int lin = by * nbx + bx;
  const int xcd = lin & 7, idx = lin >> 3;
  const int q = nwg >> 3, r = nwg & 7;
  const int base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  const int nl = base + idx;
  bx = nl / nby;
  by = nl - bx * nby;
}
__device__ __forceinline__ float leaky02(float v) { return v > 0.f ? v : 0.2f * v; }

// a pointer the compiler may hold in vector registers -> scalar registers (a buffer resource must be uniform)
__device__ __forceinline__ const float* conv_uniform_ptr(const float* q) {
  const unsigned long long v = (unsigned long long)(uintptr_t)q;
  return reinterpret_cast<const float*>((uintptr_t)(((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32) |
                                                      (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v)));
}
