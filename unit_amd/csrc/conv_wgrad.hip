// conv_wgrad.hip -- weight gradient of the NHWC implicit-GEMM convolution on CDNA4 MFMA (gfx950).
//
//   dW[n][k] = sum_m dy[m][n] * im2col(x)[m][k]        n = out channel, k = (r,s,c), m = output pixel
// Both operands are contraction(m)-major in memory, so the MFMA fragments (8 consecutive m per lane) are produced by
// the CDNA4 transposing LDS read ds_read_b64_tr_b16 from row-major [m][k] / [m][n] LDS tiles (bf16); the fp32 parity
// path uses v_mfma_f32_16x16x4_f32 whose one-float-per-lane operands are plain ds_read_b32.
//   MFMA A (rows) = im2col(x)^T [k][m],  MFMA B (cols) = dy [m][n]  -> lane holds 4 consecutive k of one n: 16-B stores
// The m-range is split across workgroups (split-M); partial fp32 slabs go to the workspace and unit_wgrad_reduce sums
// them in a fixed order (bit-reproducible), applies the FrozenBN scale[n] fold and writes / accumulates dW [K][R][S][C].
#include "common.h"
#include "conv_wgrad_host.h"

template <typename TI> struct WgCfg;
template <> struct WgCfg<bf16_t> { static constexpr int ROWB = 288, MS = 64, EPC = 8; };   // 128 elems * 2 B + 32 pad
template <> struct WgCfg<float>  { static constexpr int ROWB = 576, MS = 32, EPC = 4; };   // 128 elems * 4 B + 64 pad

// fragment fetch: returns the per-lane operand for k-substep `sub` (bf16: 32 m-rows; fp32: 16 m-rows = 4 MFMAs)
template <typename TI> struct WgFrag;
template <> struct WgFrag<bf16_t> {
  typedef bf16x8 frag_t;
  // lane l: g = l>>4, i = l&15 = 4q+p ; reads rows (32*sub + 16h + 4g + q), cols col0 + 4p..4p+3 ; element j=4h+q' of
  // lane i <-> m-row 32*sub + 16h + 4g + q', column col0 + i.  (same m permutation for both operands)
  static __device__ __forceinline__ frag_t load(const char* tile, int sub, int col0, int lane) {
    int g = lane >> 4, i = lane & 15, q = i >> 2, pq = i & 3;
    const char* a0 = tile + (32 * sub + 4 * g + q) * 288 + (col0 + 4 * pq) * 2;
    s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(a0));
    s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(a0 + 16 * 288));
    typedef __attribute__((ext_vector_type(8))) short s16x8;
    s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8, v);
  }
  static __device__ __forceinline__ void mma(const frag_t& a, const frag_t& b, f32x4& acc) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
  }
};
template <> struct WgFrag<float> {
  typedef f32x4 frag_t;   // 4 consecutive MFMA k-steps: element e <-> m-row 16*sub + 4e + (l>>4)
  static __device__ __forceinline__ frag_t load(const char* tile, int sub, int col0, int lane) {
    int g = lane >> 4, i = lane & 15;
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = *reinterpret_cast<const float*>(tile + (16 * sub + 4 * e + g) * 576 + (col0 + i) * 4);
    return v;
  }
  static __device__ __forceinline__ void mma(const frag_t& a, const frag_t& b, f32x4& acc) {
#pragma unroll
    for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], b[e], acc, 0, 0, 0);
  }
};

template <typename TI>
__global__ void __launch_bounds__(256, 2) conv_wgrad_kernel(Wgrad256Args p) {
  typedef WgCfg<TI> Cfg;
  constexpr int ROWB = Cfg::ROWB, MS = Cfg::MS, EPC = Cfg::EPC;
  constexpr int BK = 128, BN = 128;
  constexpr int CPR = 128 / EPC;                // 16-B chunks per tile row (16 bf16 / 32 fp32)
  constexpr int NL = MS * CPR / 256;            // chunks per thread per operand per step (4)
  constexpr int TILE_BYTES = MS * ROWB;
  constexpr int SUBS = 2;                       // MFMA sub-steps per staged tile (bf16: 2x32 rows, fp32: 2x16 rows)
  extern __shared__ __attribute__((aligned(16))) char smem[];

  int bid = blockIdx.x;
  int tile_k = bid % p.tiles_k; int t = bid / p.tiles_k;
  int tile_n = t % p.tiles_n; int split = t / p.tiles_n;
  int k0 = tile_k * BK, n0 = tile_n * BN;
  int m_begin = split * p.m_per_split, m_end = min(p.M, m_begin + p.m_per_split);

  const TI* __restrict__ X = (const TI*)p.x;
  const TI* __restrict__ DY = (const TI*)p.dy;
  __amdgpu_buffer_rsrc_t rsX = __builtin_amdgcn_make_buffer_rsrc(const_cast<TI*>(X), 0, (int)p.x_bytes, 0x00020000);
  __amdgpu_buffer_rsrc_t rsD = __builtin_amdgcn_make_buffer_rsrc(const_cast<TI*>(DY), 0, (int)p.dy_bytes, 0x00020000);
  constexpr unsigned OOB = 0xFFFFFFF0u;

  int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  int wk = wid >> 1, wn = wid & 1;
  int lc = tid % CPR, lr = tid / CPR;           // chunk column and first row of this thread
  constexpr int RSTEP = 256 / CPR;              // row step between this thread's chunks (16 bf16 / 8 fp32)
  // this thread's k-chunk is fixed for the whole kernel: decompose once
  int kk = k0 + lc * EPC;
  bool k_ok = kk < p.Kgemm;
  int rs = kk / p.C, ch = kk - rs * p.C, kr = rs / p.S, ksx = rs - kr * p.S;
  int nn = n0 + lc * EPC;
  bool n_ok = nn < p.K;   // K multiple of EPC assumed for full chunks; partial chunk columns are masked in the epilogue
  bool pointwise = (p.R == 1 && p.S == 1 && p.stride == 1 && p.pad == 0);

  i32x4 rx[NL], rd[NL];
  auto gload = [&](int mstep) {
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      int m = mstep + lr + RSTEP * i;
      bool mok = m < m_end;
      unsigned xoff;
      bool ok = mok && k_ok;
      if (pointwise) xoff = ((unsigned)m * (unsigned)p.x_pitch + (unsigned)ch) * (unsigned)sizeof(TI);
      else {
        // m -> (n, oh, ow) with multiply-high "magic" division (the rows change every step here, unlike the forward
        // kernel): q = umulhi(m, ceil(2^32/d)) is exact while m*d < 2^32 (checked on the host), else one correction
        unsigned um = (unsigned)m, n, oh, ow;
        if (p.use_magic) {
          n = __umulhi(um, p.magic_ohw); unsigned rem = um - n * (unsigned)p.OHW;
          if (rem >= (unsigned)p.OHW) { rem -= p.OHW; ++n; }
          oh = __umulhi(rem, p.magic_ow); ow = rem - oh * (unsigned)p.OW;
          if (ow >= (unsigned)p.OW) { ow -= p.OW; ++oh; }
        } else {
          ow = um % (unsigned)p.OW; unsigned tt = um / (unsigned)p.OW; oh = tt % (unsigned)p.OH; n = tt / (unsigned)p.OH;
        }
        int ih = (int)oh * p.stride - p.pad + kr, iw = (int)ow * p.stride - p.pad + ksx;
        ok = ok && (unsigned)ih < (unsigned)p.H && (unsigned)iw < (unsigned)p.W;
        xoff = ((unsigned)n * (unsigned)(p.H * p.W * p.x_pitch) + (unsigned)((ih * p.W + iw) * p.x_pitch + ch)) * (unsigned)sizeof(TI);
      }
      rx[i] = __builtin_amdgcn_raw_buffer_load_b128(rsX, ok ? xoff : OOB, 0, 0);
      unsigned doff = ((unsigned)m * (unsigned)p.ldy + (unsigned)nn) * (unsigned)sizeof(TI);
      rd[i] = __builtin_amdgcn_raw_buffer_load_b128(rsD, (mok && n_ok) ? doff : OOB, 0, 0);
    }
  };
  auto lstore = [&](int buf) {
    char* bx = smem + buf * 2 * TILE_BYTES;
    char* bd = bx + TILE_BYTES;
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      int row = lr + RSTEP * i;
      *reinterpret_cast<i32x4*>(bx + row * ROWB + lc * 16) = rx[i];
      *reinterpret_cast<i32x4*>(bd + row * ROWB + lc * 16) = rd[i];
    }
  };

  f32x4 acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

  int nsteps = (m_end - m_begin + MS - 1) / MS;
  if (nsteps > 0) {
    gload(m_begin);
    lstore(0);
  }
  __syncthreads();
  for (int st = 0; st < nsteps; ++st) {
    int buf = st & 1;
    if (st + 1 < nsteps) gload(m_begin + (st + 1) * MS);
    const char* bx = smem + buf * 2 * TILE_BYTES;
    const char* bd = bx + TILE_BYTES;
#pragma unroll
    for (int sub = 0; sub < SUBS; ++sub) {
      typename WgFrag<TI>::frag_t fa[4], fb[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) fa[a] = WgFrag<TI>::load(bx, sub, wk * 64 + a * 16, lane);
#pragma unroll
      for (int b = 0; b < 4; ++b) fb[b] = WgFrag<TI>::load(bd, sub, wn * 64 + b * 16, lane);
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) WgFrag<TI>::mma(fa[a], fb[b], acc[a][b]);
    }
    if (st + 1 < nsteps) lstore(buf ^ 1);
    __syncthreads();
  }

  // epilogue: D[row = k][col = n] -> partial[split][n][k..k+3]
  float* out = p.partial + (size_t)split * p.K * p.Kgemm;
  int fq = lane >> 4, fr = lane & 15;
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    int n = n0 + wn * 64 + b * 16 + fr;
    if (n >= p.K) continue;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      int k = k0 + wk * 64 + a * 16 + fq * 4;
      if (k >= p.Kgemm) continue;
      *reinterpret_cast<f32x4*>(out + (size_t)n * p.Kgemm + k) = acc[a][b];
    }
  }
}

// dW[n][k] = (accumulate ? dW : 0) + scale[n] * sum_s partial[s][n][k]     (fixed summation order)
__global__ void wgrad_reduce_kernel(const float* __restrict__ partial, int splits, long KK, int Kgemm, const float* __restrict__ scale,
                                    float* __restrict__ dw, int accumulate) {
  long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i >= KK) return;
  f32x4 s = *reinterpret_cast<const f32x4*>(partial + i);
  for (int sp = 1; sp < splits; ++sp) {
    f32x4 v = *reinterpret_cast<const f32x4*>(partial + (size_t)sp * KK + i);
    s += v;
  }
  if (scale) { float sc = scale[i / Kgemm]; s *= sc; }
  if (accumulate) s += *reinterpret_cast<const f32x4*>(dw + i);
  *reinterpret_cast<f32x4*>(dw + i) = s;
}

// conv_wgrad256.hip: the 256x256 tile's kernels for the big-M bf16 layers (same slab layout) on a filled argument block
int unit_wgrad_big_launch_args(Wgrad256Args& a, int variant, size_t workspace_bytes, hipStream_t st);

extern "C" size_t unit_conv2d_wgrad_workspace_bytes(int in_dtype, int N, int OH, int OW, int K, int R, int S, int C) {
  return (size_t)wgrad_select(in_dtype, N, OH, OW, K, R, S, C).splits * K * R * S * C * sizeof(float);
}

// one pass of split-M slabs into `workspace` (no reduction); returns the number of slabs written or a negative status.
// x_pitch: elements per pixel row of x; x_span / dy_span: bytes from x / dy to the end of their tensors (the buffer range of the loads).
static int wgrad_pass(const void* x, const void* dy, int in_dtype, int N, int H, int W, int C, int K, int R, int S, int stride, int pad, int OH,
                      int OW, int ldy, int variant, void* workspace, size_t workspace_bytes, int x_pitch, size_t x_span, size_t dy_span,
                      void* stream) {
  UNIT_CHECK_ARG(variant >= 0 && variant <= 4, "wgrad: variant 0..4");
  int epc = in_dtype == UNIT_BF16 ? 8 : 4;
  UNIT_CHECK_ARG(C % epc == 0 && K % epc == 0 && ldy % epc == 0, "wgrad: C, K, ldy must be multiples of 8 (bf16) / 4 (fp32)");
  UNIT_CHECK_ARG(((uintptr_t)x % 16 == 0) && ((uintptr_t)dy % 16 == 0), "wgrad: 16B alignment");
  UNIT_CHECK_ARG(R * S * C % 4 == 0, "wgrad: R*S*C % 4 != 0");
  const WgradChoice ch = wgrad_select(in_dtype, N, OH, OW, K, R, S, C);
  Wgrad256Args a;
  int rc = wgrad_fill(a, "wgrad: operand larger than 4 GiB", x, dy, (float*)workspace, N, H, W, C, K, R, S, stride, pad, OH, OW, ldy, x_pitch,
                      x_span, dy_span, ch.tile, ch.ms, ch.splits);
  if (rc != UNIT_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (ch.family == WGRAD_BIG) return unit_wgrad_big_launch_args(a, variant <= 3 ? variant : 0, workspace_bytes, st);
  size_t need = (size_t)a.splits * K * a.Kgemm * sizeof(float);
  if (workspace_bytes < need) { unit_set_error("wgrad: workspace too small"); return UNIT_ERR_WORKSPACE; }
  int grid = a.tiles_k * a.tiles_n * a.splits;
  // bf16 layers whose tiles are full (every trainable backbone / RPN conv): LDS-DMA ring kernel (conv_wgrad128r.hip), same slabs
  if (ch.family == WGRAD_RING128 && variant != 4) {
    rc = unit_wgrad128_ring_launch(a, st);
    if (rc != UNIT_OK) return rc;
  } else if (in_dtype == UNIT_BF16) {
    size_t lds = (size_t)2 * 2 * WgCfg<bf16_t>::MS * WgCfg<bf16_t>::ROWB;
    static bool set1 = false;
    if (!set1) { (void)hipFuncSetAttribute((const void*)conv_wgrad_kernel<bf16_t>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); set1 = true; }
    conv_wgrad_kernel<bf16_t><<<grid, 256, lds, st>>>(a);
  } else {
    size_t lds = (size_t)2 * 2 * WgCfg<float>::MS * WgCfg<float>::ROWB;
    static bool set2 = false;
    if (!set2) { (void)hipFuncSetAttribute((const void*)conv_wgrad_kernel<float>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); set2 = true; }
    conv_wgrad_kernel<float><<<grid, 256, lds, st>>>(a);
  }
  UNIT_LAUNCH_CHECK();
  return a.splits;
}

// x [N,H,W,C], dy [M][ldy] (pixels of the conv's OUTPUT grid, row-major), dw fp32 [K][R][S][C].
extern "C" int unit_conv2d_wgrad(const void* x, const void* dy, float* dw, const float* scale_k, int in_dtype, int N,
                                 int H, int W, int C, int K, int R, int S, int stride, int pad, int OH, int OW, int ldy,
                                 int accumulate, int variant, void* workspace, size_t workspace_bytes, void* stream) {
  UNIT_CHECK_ARG((uintptr_t)dw % 16 == 0, "wgrad: 16B alignment");
  size_t esz = in_dtype == UNIT_BF16 ? 2 : 4;
  int sp = wgrad_pass(x, dy, in_dtype, N, H, W, C, K, R, S, stride, pad, OH, OW, ldy, variant, workspace, workspace_bytes, C,
                      (size_t)N * H * W * C * esz, (size_t)N * OH * OW * ldy * esz, stream);
  if (sp < 0) return sp;
  if (dw == nullptr) return UNIT_OK;   // partial slabs only: the caller reduces later (unit_multi_wgrad_reduce)
  long KK = (long)K * R * S * C;
  wgrad_reduce_kernel<<<cdiv(KK / 4, 256), 256, 0, (hipStream_t)stream>>>((const float*)workspace, sp, KK, R * S * C, scale_k, dw, accumulate);
  UNIT_LAUNCH_CHECK();
  return UNIT_OK;
}

// bf16x3 weight gradient (csrc/split.hip): x split [N,H,W][2][C], dy split [M][2][ldy] -> dW ~ hi^T.hi + hi^T.lo + lo^T.hi as THREE passes of
// the bf16 kernels above over the planes, each pass with its own split-M slabs (3 * unit_conv2d_wgrad_splits(UNIT_BF16, ...) in all, at
// workspace + s*K*R*S*C floats like unit_conv2d_wgrad's); dw != NULL: reduced here, else the caller folds them (unit_multi_wgrad_reduce).
extern "C" int unit_conv2d_wgrad_x3(const void* x, const void* dy, float* dw, const float* scale_k, int N, int H, int W, int C, int K, int R,
                                    int S, int stride, int pad, int OH, int OW, int ldy, int accumulate, int variant, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  UNIT_CHECK_ARG((uintptr_t)dw % 16 == 0, "wgrad_x3: 16B alignment");
  UNIT_CHECK_ARG(C % 8 == 0 && ldy % 8 == 0, "wgrad_x3: C, ldy must be multiples of 8");
  const size_t xt = (size_t)N * H * W * C * 4, dt = (size_t)N * OH * OW * ldy * 4;      // bytes of the split tensors
  const size_t slab = (size_t)K * R * S * C * sizeof(float);
  const int xpl[3] = {0, 0, 1}, dpl[3] = {0, 1, 0};                                    // plane of x / dy per pass: (hi, hi), (hi, lo), (lo, hi)
  // variant bits 8-9: how many of the three passes run (0 = all; 1 = hi^T.hi only: bf16-grade products of the rounded operands, fp32 sums)
  const int npass = ((variant >> 8) & 3) ? ((variant >> 8) & 3) : 3;
  variant &= 0xff;
  int total = 0;
  for (int ps = 0; ps < npass; ++ps) {
    size_t used = (size_t)total * slab;
    if (workspace_bytes < used) { unit_set_error("wgrad_x3: workspace too small"); return UNIT_ERR_WORKSPACE; }
    const char* xp = (const char*)x + (size_t)xpl[ps] * C * 2;
    const char* dp = (const char*)dy + (size_t)dpl[ps] * ldy * 2;
    int sp = wgrad_pass(xp, dp, UNIT_BF16, N, H, W, C, K, R, S, stride, pad, OH, OW, 2 * ldy, variant, (char*)workspace + used,
                        workspace_bytes - used, 2 * C, xt - (size_t)xpl[ps] * C * 2, dt - (size_t)dpl[ps] * ldy * 2, stream);
    if (sp < 0) return sp;
    total += sp;
  }
  if (dw == nullptr) return UNIT_OK;
  long KK = (long)K * R * S * C;
  wgrad_reduce_kernel<<<cdiv(KK / 4, 256), 256, 0, (hipStream_t)stream>>>((const float*)workspace, total, KK, R * S * C, scale_k, dw, accumulate);
  UNIT_LAUNCH_CHECK();
  return UNIT_OK;
}

// number of split-M slabs unit_conv2d_wgrad writes for this shape (slab s at workspace + s*K*R*S*C floats)
extern "C" int unit_conv2d_wgrad_splits(int in_dtype, int N, int OH, int OW, int K, int R, int S, int C) {
  return wgrad_select(in_dtype, N, OH, OW, K, R, S, C).splits;
}


// ---- grouped launches (conv_wgrad128r.hip: conv_wgrad128_group_kernel; conv_wgrad256p8.hip: conv_wgrad256_group_kernel) -------------
// x / dy / partial as unit_conv2d_wgrad(dw = NULL) takes them, for n layers at once; pr[i].splits / kind from unit_conv2d_wgrad_group_plan.
// Slab s of layer i at partial + s*K*R*S*C floats, same layout as unit_conv2d_wgrad's (unit_multi_wgrad_reduce folds them).
// Which layers share a grid and where their units run is the planner's business (conv_wgrad_plan.hip); this is the piece that launches.
static int wgrad_group_launch(void* stream, const WgradGroupArgs& g, int kind, int slots_per_xcd, const int*) {
  return kind == 2 ? unit_wgrad256_group_launch(g, slots_per_xcd, (hipStream_t)stream) : unit_wgrad128_group_launch(g, slots_per_xcd, (hipStream_t)stream);
}

extern "C" int unit_conv2d_wgrad_group(const UnitWgradProblem* pr, int n, int in_dtype, void* stream) {
  UNIT_CHECK_ARG(in_dtype == UNIT_BF16, "wgrad_group: bf16 only");
  UNIT_CHECK_ARG(pr != nullptr && n >= 0, "wgrad_group: no problems");
  return wgrad_group_each_launch(pr, n, wgrad_group_launch, stream);
}
