// conv_args.h -- what the forward / dgrad implicit-GEMM conv kernels of every family share: THE prefix of their argument blocks (ConvCore),
// the row-of-four load / store of the accumulator-layout epilogues (Out4) and the tail of their launchers (conv_launch, pair_grid).
// The host side that fills a ConvCore from a layer's geometry is conv_fwd_host.h.
#pragma once
#include <stddef.h>
#include "common.h"
#include "conv_epilogue.h"

// ConvArgs (conv_igemm.hip), ConvDmaArgs (conv_igemm128.h) and Conv256Args (conv_igemm256.h) derive from this and add their own tail: the kernels
// read p.x, p.M, ... of any of them, pair_swap_common / epi_flags (conv_epilogue.h) are templates on the block's type.
struct ConvCore {
  const void* x; const void* w; void* y;
  const float* bias; const void* residual; const void* mask_ref;
  int N, H, W, C;
  int K, R, S, stride, pad;
  int OH, OW;
  int ldy, oy_mul, OHf, OWf;
  int relu;
  int Kgemm;   // R*S*C
  int M;       // N*OH*OW
  int tiles_m, tiles_n;
  unsigned x_bytes, w_bytes;
};
// the kernarg layout: 136 bytes without tail padding, so that a derived block's first own member starts right behind them
static_assert(sizeof(ConvCore) == 136 && alignof(ConvCore) == 8, "ConvCore: the 28 shared fields, 136 bytes");
// (offsetof into a derived class: conditionally supported, exact on this compiler)
#define CONV_ARGS_TAIL_AT_136(T, member)                                                                    \
  _Pragma("clang diagnostic push") _Pragma("clang diagnostic ignored \"-Winvalid-offsetof\"")               \
  static_assert(__builtin_offsetof(T, member) == sizeof(ConvCore), #T ": " #member " follows the shared prefix") \
  _Pragma("clang diagnostic pop")

// four consecutive output channels of one pixel as floats, loaded / stored as 16 B (fp32) or 8 B (bf16)
template <typename TO> struct Out4;
template <> struct Out4<float> {
  static __device__ __forceinline__ void load(const float* p, float (&v)[4]) { f32x4 a = *reinterpret_cast<const f32x4*>(p); v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3]; }
  static __device__ __forceinline__ void store(float* p, const float (&v)[4]) { f32x4 a = {v[0], v[1], v[2], v[3]}; *reinterpret_cast<f32x4*>(p) = a; }
};
template <> struct Out4<bf16_t> {
  static __device__ __forceinline__ void load(const bf16_t* p, float (&v)[4]) {
    bf16x4 a = *reinterpret_cast<const bf16x4*>(p);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = (float)a[i];
  }
  static __device__ __forceinline__ void store(bf16_t* p, const float (&v)[4]) {
    bf16x4 a;
#pragma unroll
    for (int i = 0; i < 4; ++i) a[i] = (bf16_t)v[i];
    *reinterpret_cast<bf16x4*>(p) = a;
  }
};

// The tail of every launcher: raise the kernel's dynamic-LDS limit once (the static belongs to this instantiation, i.e. to Kern; `lds` is a
// constant of the kernel), launch, check. Twin: the PAIR / non-PAIR sibling whose limit is raised at the same first launch.
template <auto Kern, auto Twin = Kern, typename Args>
static int conv_launch(int grid, int block, size_t lds, const Args& a, hipStream_t st) {
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute((const void*)Kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if ((const void*)Twin != (const void*)Kern) (void)hipFuncSetAttribute((const void*)Twin, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    attr_set = true;
  }
  Kern<<<grid, block, lds, st>>>(a);
  UNIT_LAUNCH_CHECK();
  return UNIT_OK;
}

// Non-persistent pair launch (conv_epilogue.h ConvSecond): the second problem's tiles of BM rows follow the first's; returns the grid of both
template <typename Args>
static inline int pair_grid(Args& a, int BM) {
  a.second.tiles_m = cdiv(a.second.M, BM);
  a.second.tiles0 = a.tiles_m * a.tiles_n;
  return (a.tiles_m + a.second.tiles_m) * a.tiles_n;
}
