// roi_pool.hip -- RoIPool (max over integer feature-grid windows) forward / deterministic gather backward, NHWC.
// Reference: Detectron2 v0.3 modeling/poolers.py ROIPooler -> torchvision.ops.RoIPool, reached from
// the reference's modeling/roi_heads/roi_heads.py:499,511 under MODEL.ROI_BOX_HEAD.POOLER_TYPE: "ROIPool"
// (configs/COCO/COCO-VGG-CNN-F-split1-dock.yaml).
//
// The operator, in integer arithmetic on the feature grid (torchvision roi_pool_kernel.cu):
//   x1 = roundf(roi[1] * scale) ... y2 = roundf(roi[4] * scale)      (halves away from zero)
//   roi_w = max(x2 - x1 + 1, 1), bin_w = (float)roi_w / pooled       (likewise h)
//   bin (ph, pw): rows [floorf(ph * bin_h), ceilf((ph + 1) * bin_h)) + y1 clamped to [0, H], columns likewise; empty if hend <= hstart
//   || wend <= wstart. The window is scanned row-major with a strict `>` from -FLT_MAX: the first maximum wins, a NaN is never selected.
//   The output is the selected element's bits; an empty bin gives +0, a window without a selectable element (-FLT_MAX as T); argmax -1 for both.
// Lanes own 8 consecutive channels (16 B bf16 / 32 B fp32) as in roi_align.hip, and `bin_step` / `out_size` mean what they mean there:
// bins (oph * bin_step, opw * bin_step) of the full `pooled_size` grid are produced, their windows are those of the full grid.
// argmax element: int32 y * W + x inside the RoI's image (what torchvision stores), -1 for none.
#include "common.h"
#include <float.h>

// roi_align.hip: a contiguous run of work items per XCD keeps a RoI's bins (forward) / a band of image rows (backward) behind ONE L2
__device__ __forceinline__ long xcd_contiguous(long bid, long n) {
  long q = n / 8, r = n % 8, xcd = bid % 8, loc = bid / 8;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
}

struct PoolWin { float bw, bh; int b, x1, y1; };

// scaled corner -> grid index; kept inside +-2^24 so that no sum of two of them (or with a bin offset) leaves int range
__device__ __forceinline__ int pool_corner(float v) {
  return (int)fminf(fmaxf(roundf(v), -16777216.0f), 16777216.0f);
}

__device__ __forceinline__ PoolWin pool_win(const float* __restrict__ roi, float scale, int pooled) {
  PoolWin g;
  g.b = (int)roi[0];
  g.x1 = pool_corner(roi[1] * scale); g.y1 = pool_corner(roi[2] * scale);
  int x2 = pool_corner(roi[3] * scale), y2 = pool_corner(roi[4] * scale);
  int rw = max(x2 - g.x1 + 1, 1), rh = max(y2 - g.y1 + 1, 1);
  g.bw = (float)rw / (float)pooled; g.bh = (float)rh / (float)pooled;
  return g;
}

// rows (columns) [lo, hi) of bin p of the full grid, clamped to the map
__device__ __forceinline__ void pool_bin_range(int p, float bsz, int start, int L, int& lo, int& hi) {
  float fl = fminf(floorf((float)p * bsz), 33554432.0f), fh = fminf(ceilf((float)(p + 1) * bsz), 33554432.0f);
  lo = min(max((int)fl + start, 0), L);
  hi = min(max((int)fh + start, 0), L);
}

// the 8 channels of a lane as stored (no conversion on the way through: the output is the selected element bit for bit)
template <typename T> struct Raw8;
template <> struct Raw8<float> {
  static __device__ __forceinline__ void load(const float* p, float (&v)[8]) { Vec8<float>::load(p, v); }
  static __device__ __forceinline__ void store(float* p, const float (&v)[8]) { Vec8<float>::store(p, v); }
};
template <> struct Raw8<bf16_t> {
  static __device__ __forceinline__ void load(const bf16_t* p, bf16_t (&v)[8]) {
    bf16x8 a = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = a[i];
  }
  static __device__ __forceinline__ void store(bf16_t* p, const bf16_t (&v)[8]) {
    bf16x8 a;
#pragma unroll
    for (int i = 0; i < 8; ++i) a[i] = v[i];
    *reinterpret_cast<bf16x8*>(p) = a;
  }
};

__device__ __forceinline__ void store_idx8(int* p, const int (&v)[8]) {
  i32x4 a = {v[0], v[1], v[2], v[3]}, b = {v[4], v[5], v[6], v[7]};
  *reinterpret_cast<i32x4*>(p) = a; *reinterpret_cast<i32x4*>(p + 4) = b;
}
__device__ __forceinline__ void load_idx8(const int* p, int (&v)[8]) {
  i32x4 a = *reinterpret_cast<const i32x4*>(p), b = *reinterpret_cast<const i32x4*>(p + 4);
  v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3]; v[4] = b[0]; v[5] = b[1]; v[6] = b[2]; v[7] = b[3];
}

// grid: R * out_size workgroups, one per (RoI, row of output bins) as roi_align_fwd_row_kernel ; block: C/8 lanes (rounded up to 64)
template <typename T>
__global__ void roi_pool_fwd_kernel(const T* __restrict__ feat, int N, int H, int W, int C, const float* __restrict__ rois,
                                    const int* __restrict__ roi_count, int pooled, int out_size, int bin_step, float scale,
                                    T* __restrict__ out, int* __restrict__ argmax) {
  int row = (int)xcd_contiguous(blockIdx.x, gridDim.x);
  int r = row / out_size, oph = row - r * out_size;
  int c0 = threadIdx.x * 8;
  if (c0 >= C) return;
  size_t obase = ((size_t)row * out_size) * C + c0;
  bool live = !(roi_count && r >= *roi_count);
  PoolWin g;
  if (live) { g = pool_win(rois + 5 * (size_t)r, scale, pooled); live = g.b >= 0 && g.b < N; }
  if (!live) {          // an unused slot (or a RoI naming no image of the batch): zeros, no argmax
    T z[8]; int none[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) { z[i] = (T)0.0f; none[i] = -1; }
    for (int opw = 0; opw < out_size; ++opw) {
      Raw8<T>::store(out + obase + (size_t)opw * C, z);
      if (argmax) store_idx8(argmax + obase + (size_t)opw * C, none);
    }
    return;
  }
  int hs, he;
  pool_bin_range(oph * bin_step, g.bh, g.y1, H, hs, he);
  const T* f = feat + (size_t)g.b * H * W * C + c0;
  for (int opw = 0; opw < out_size; ++opw) {
    int ws, we;
    pool_bin_range(opw * bin_step, g.bw, g.x1, W, ws, we);
    bool empty = he <= hs || we <= ws;
    float bestf[8]; T best[8]; int idx[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) { bestf[i] = empty ? 0.0f : -FLT_MAX; best[i] = (T)bestf[i]; idx[i] = -1; }
    if (!empty) {
      for (int y = hs; y < he; ++y) {
        for (int x = ws; x < we; ++x) {
          T v[8];
          Raw8<T>::load(f + ((size_t)y * W + x) * C, v);
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            float vf = (float)v[i];
            if (vf > bestf[i]) { bestf[i] = vf; best[i] = v[i]; idx[i] = y * W + x; }
          }
        }
      }
    }
    Raw8<T>::store(out + obase + (size_t)opw * C, best);
    if (argmax) store_idx8(argmax + obase + (size_t)opw * C, idx);
  }
}

extern "C" size_t unit_roi_pool_argmax_bytes(int R, int out_size, int C) {
  return sizeof(int) * (size_t)(R > 0 ? R : 0) * (size_t)out_size * (size_t)out_size * (size_t)C;
}

extern "C" int unit_roi_pool_fwd(const void* feat_nhwc, int dtype, int N, int H, int W, int C, const float* rois, const int* roi_count_dev,
                                 int R, int pooled_size, int out_size, int bin_step, float spatial_scale, void* out, void* argmax,
                                 void* stream) {
  UNIT_CHECK_ARG(C > 0 && C % 8 == 0 && C / 8 <= 1024, "roi_pool: C % 8 != 0 or C > 8192");
  UNIT_CHECK_ARG(pooled_size > 0 && out_size > 0 && bin_step > 0 && (out_size - 1) * bin_step < pooled_size,
                 "roi_pool: out_size/bin_step exceed pooled_size");
  UNIT_CHECK_ARG(dtype == UNIT_F32 || dtype == UNIT_BF16, "roi_pool: dtype must be fp32 or bf16");
  UNIT_CHECK_ARG(N >= 0 && H > 0 && W > 0 && (long)H * W < (1L << 31), "roi_pool: H * W must fit the int32 argmax");
  if (R <= 0) return UNIT_OK;
  int threads = ((C / 8 + 63) / 64) * 64;
  long blocks = (long)R * out_size;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == UNIT_BF16)
    roi_pool_fwd_kernel<bf16_t><<<blocks, threads, 0, st>>>((const bf16_t*)feat_nhwc, N, H, W, C, rois, roi_count_dev, pooled_size, out_size,
                                                          bin_step, spatial_scale, (bf16_t*)out, (int*)argmax);
  else
    roi_pool_fwd_kernel<float><<<blocks, threads, 0, st>>>((const float*)feat_nhwc, N, H, W, C, rois, roi_count_dev, pooled_size, out_size,
                                                         bin_step, spatial_scale, (float*)out, (int*)argmax);
  UNIT_LAUNCH_CHECK();
  return UNIT_OK;
}

// =====================================================================================================================
// Deterministic RoIPool backward in GATHER form (no atomics): one workgroup per feature-map pixel, lanes over channels.
//   dfeat[n,y,x,c] = sum over the RoIs r of image n (ascending slot), over the produced bins (oph, opw) of r whose window holds (y, x)
//                    (row-major), of  g[r,oph,opw,c]  where argmax[r,oph,opw,c] == y * W + x
// Additions only, in that fixed order, into an fp32 accumulator that starts at +0 -> bit-reproducible, and bit-comparable with a host
// restatement that adds in the same order. Then the RoIAlign gather's epilogue: out = cast((acc [+ addend]) [* (mask_ref > 0)]).
// A RoI smaller than the grid (bin_h < 1) puts one pixel into up to `pooled` windows per axis: every produced bin is tested, none assumed.
// =====================================================================================================================
struct PoolG { float bw, bh; int b, x1, y1, y0, yend, x0, xend; };          // [y0, yend) x [x0, xend): hull of the produced bins' windows

__global__ void roi_pool_geom_kernel(const float* __restrict__ rois, const int* __restrict__ roi_count, int R, int N, int H, int W,
                                     int pooled, int out_size, int bin_step, float scale, PoolG* __restrict__ tab) {
  int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  PoolG t;
  t.bw = t.bh = 0.f; t.b = -1; t.x1 = t.y1 = 0; t.y0 = t.yend = t.x0 = t.xend = 0;
  if (!(roi_count && r >= *roi_count)) {
    PoolWin g = pool_win(rois + 5 * (size_t)r, scale, pooled);
    if (g.b >= 0 && g.b < N) {
      int plast = (out_size - 1) * bin_step, lo, hi;
      t.bw = g.bw; t.bh = g.bh; t.b = g.b; t.x1 = g.x1; t.y1 = g.y1;
      pool_bin_range(0, g.bh, g.y1, H, t.y0, hi); pool_bin_range(plast, g.bh, g.y1, H, lo, t.yend);
      pool_bin_range(0, g.bw, g.x1, W, t.x0, hi); pool_bin_range(plast, g.bw, g.x1, W, lo, t.xend);
    }
  }
  tab[r] = t;
}

template <typename T, typename TOUT>
__global__ void roi_pool_bwd_gather_kernel(const T* __restrict__ gout, const int* __restrict__ argmax, int H, int W, int C,
                                           const PoolG* __restrict__ tab, int R, int rois_per_image, int image_offset, int out_size,
                                           int bin_step, const T* __restrict__ addend, int addend_images, const T* __restrict__ mask_ref,
                                           TOUT* __restrict__ dfeat) {
  int pix = (int)xcd_contiguous(blockIdx.x, gridDim.x);
  int n = pix / (H * W); int rem = pix - n * H * W; int py = rem / W, px = rem - py * W;
  int lane = threadIdx.x & 63;
  int c0 = threadIdx.x * 8;
  bool cvalid = c0 < C;
  float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  int r_begin = 0, r_end = R;
  if (rois_per_image > 0) { r_begin = n * rois_per_image; r_end = min(R, r_begin + rois_per_image); }
  // 64 RoIs are tested per iteration (one per lane, hull of their produced windows); only the hits are visited, in ascending slot order
  for (int rb = r_begin; rb < r_end; rb += 64) {
    bool hit = false;
    if (rb + lane < r_end) {
      const PoolG& q = tab[rb + lane];
      hit = q.b == n + image_offset && py >= q.y0 && py < q.yend && px >= q.x0 && px < q.xend;
    }
    for (unsigned long long hm = __ballot(hit); hm; hm &= hm - 1) {
      int r = rb + __ffsll((long long)hm) - 1;
      PoolG t = tab[r];                                   // wave-uniform
      // lanes 0..out-1: does the row window of bin (lane*step) hold py; lanes 32..32+out-1: the column window and px
      bool in = false;
      int o = lane & 31;
      if (o < out_size) {
        bool isx = lane >= 32;
        int lo, hi;
        pool_bin_range(o * bin_step, isx ? t.bw : t.bh, isx ? t.x1 : t.y1, isx ? W : H, lo, hi);
        int pp = isx ? px : py;
        in = pp >= lo && pp < hi;
      }
      unsigned long long nz = __ballot(in);
      unsigned ymask = (unsigned)(nz & 0xFFFFFFFFull), xmask = (unsigned)(nz >> 32);
      if (ymask == 0u || xmask == 0u || !cvalid) continue;
      size_t rbase = (size_t)r * out_size * out_size * C + c0;
      int want = py * W + px;
      for (unsigned ym = ymask; ym; ym &= ym - 1) {
        int oy = __ffs(ym) - 1;
        for (unsigned xm = xmask; xm; xm &= xm - 1) {
          int ox = __ffs(xm) - 1;
          size_t off = rbase + ((size_t)oy * out_size + ox) * C;
          int am[8];
          load_idx8(argmax + off, am);
          bool any = false;
#pragma unroll
          for (int j = 0; j < 8; ++j) any = any || am[j] == want;
          if (!any) continue;
          float v[8];
          Vec8<T>::load(gout + off, v);
#pragma unroll
          for (int j = 0; j < 8; ++j) if (am[j] == want) acc[j] += v[j];
        }
      }
    }
  }
  if (!cvalid) return;
  size_t o = (size_t)pix * C + c0;
  if (addend && n < addend_images) {
    float a[8]; Vec8<T>::load(addend + o, a);
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] += a[j];
  }
  if (mask_ref) {
    float m[8]; Vec8<T>::load(mask_ref + o, m);
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = m[j] > 0.f ? acc[j] : 0.f;
  }
  Vec8<TOUT>::store(dfeat + o, acc);
}

extern "C" size_t unit_roi_pool_bwd_gather_workspace_bytes(int R) { return sizeof(PoolG) * (size_t)(R > 0 ? R : 1); }

// dfeat (out_dtype: 0 fp32 / 1 bf16) [N,H,W,C] is fully written (no pre-zeroing needed). `argmax` is what unit_roi_pool_fwd stored for
// the same rois / pooled_size / out_size / bin_step. rois_per_image, image_offset, addend, mask_ref: as unit_roi_align_bwd_gather.
extern "C" int unit_roi_pool_bwd_gather(const void* gout, const void* argmax, int dtype, int N, int H, int W, int C, const float* rois,
                                        const int* roi_count_dev, int R, int rois_per_image, int image_offset, int pooled_size, int out_size,
                                        int bin_step, float spatial_scale, const void* addend, int addend_images, const void* mask_ref,
                                        void* dfeat, int out_dtype, void* workspace, size_t workspace_bytes, void* stream) {
  UNIT_CHECK_ARG(C > 0 && C % 8 == 0 && C / 8 <= 1024 && out_size > 0 && out_size <= 16, "roi_pool_bwd_gather: C % 8, C <= 8192, out_size <= 16");
  UNIT_CHECK_ARG(pooled_size > 0 && bin_step > 0 && (out_size - 1) * bin_step < pooled_size, "roi_pool_bwd_gather: out_size/bin_step exceed pooled_size");
  UNIT_CHECK_ARG(dtype == UNIT_F32 || dtype == UNIT_BF16, "roi_pool_bwd_gather: dtype must be fp32 or bf16");
  UNIT_CHECK_ARG(out_dtype == UNIT_F32 || out_dtype == dtype, "roi_pool_bwd_gather: out dtype must be fp32 or the input dtype");
  UNIT_CHECK_ARG(N >= 0 && H > 0 && W > 0 && (long)N * H * W < (1L << 31) && image_offset >= 0, "roi_pool_bwd_gather: N * H * W must fit int32");
  UNIT_CHECK_ARG(argmax != nullptr || R <= 0, "roi_pool_bwd_gather: the forward's argmax is required");
  if (workspace_bytes < unit_roi_pool_bwd_gather_workspace_bytes(R)) { unit_set_error("roi_pool_bwd_gather: workspace too small"); return UNIT_ERR_WORKSPACE; }
  hipStream_t st = (hipStream_t)stream;
  PoolG* tab = (PoolG*)workspace;
  if (R < 0) R = 0;
  if (R > 0) {
    roi_pool_geom_kernel<<<cdiv(R, 256), 256, 0, st>>>(rois, roi_count_dev, R, N + image_offset, H, W, pooled_size, out_size, bin_step,
                                                     spatial_scale, tab);
    UNIT_LAUNCH_CHECK();
  }
  int threads = ((C / 8 + 63) / 64) * 64;
  long blocks = (long)N * H * W;
  if (blocks == 0) return UNIT_OK;
#define LAUNCH_G(T, TOUT) roi_pool_bwd_gather_kernel<T, TOUT><<<blocks, threads, 0, st>>>((const T*)gout, (const int*)argmax, H, W, C, tab, R, \
    rois_per_image, image_offset, out_size, bin_step, (const T*)addend, addend_images, (const T*)mask_ref, (TOUT*)dfeat)
  if (dtype == UNIT_BF16 && out_dtype == UNIT_BF16) LAUNCH_G(bf16_t, bf16_t);
  else if (dtype == UNIT_BF16) LAUNCH_G(bf16_t, float);
  else LAUNCH_G(float, float);
#undef LAUNCH_G
  UNIT_LAUNCH_CHECK();
  return UNIT_OK;
}
