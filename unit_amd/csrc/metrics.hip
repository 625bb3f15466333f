// metrics.hip -- the step scalars Detectron2 logs beside the losses, counted on the device (no host sync, replay-safe arguments):
//   unit_metrics_rpn       rpn/num_pos_anchors, rpn/num_neg_anchors          modeling/proposal_generator/rpn.py:61-66 of the reference
//   unit_metrics_fastrcnn  fast_rcnn/cls_accuracy, fg_cls_accuracy, false_negative (Detectron2 v0.3 FastRCNNOutputs._log_accuracy behind
//                          modeling/roi_heads/fast_rcnn.py:438-445) and roi_head/num_fg_samples, num_bg_samples (ROIHeads.label_and_sample_proposals
//                          behind modeling/roi_heads/roi_heads.py:563)
//   unit_metrics_mask      mask_rcnn/accuracy, false_positive, false_negative (Detectron2 v0.3 mask_rcnn_loss behind modeling/roi_heads/mask_head.py:34)
// Every scalar is a ratio of integer counts; the kernels ADD the counts into an int32 vector the caller zeroed (unit_fill_zero) and the
// host divides when somebody asks (unit_amd/metrics.py). Per workgroup: per-lane counts -> wave sum by __shfl_xor -> LDS -> ONE atomicAdd
// per non-zero counter. Integer addition is associative and commutative, so the totals do not depend on the order in which the workgroups
// (or the three kernels, which run on different streams into different slots of one vector) arrive: bit-reproducible, unlike a float atomic.
#include "common.h"

#define METRICS_THREADS 256

__device__ __forceinline__ int wave_reduce_sum_int(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// per-thread counts -> m[0..NC): every thread of the (<= 256-thread) workgroup calls this exactly once
template <int NC>
__device__ __forceinline__ void block_add_counters(int (&v)[NC], int* __restrict__ m) {
  __shared__ int lds[NC][METRICS_THREADS / 64];
  const int wave = threadIdx.x >> 6, nwaves = (blockDim.x + 63) >> 6;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    int t = wave_reduce_sum_int(v[c]);
    if ((threadIdx.x & 63) == 0) lds[c][wave] = t;
  }
  __syncthreads();
  if (threadIdx.x < NC) {
    int t = 0;
    for (int w = 0; w < nwaves; ++w) t += lds[threadIdx.x][w];
    if (t != 0) atomicAdd(m + threadIdx.x, t);
  }
}

// ---------------------------------------------------------------------------------------------------
// sampled anchor labels [n] int8 (1 positive, 0 negative, -1 ignored): four labels per lane and load (one 32-bit word where the
// pointer allows it), consecutive lanes on consecutive words
// ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(METRICS_THREADS) metrics_rpn_kernel(const int8_t* __restrict__ labels, int n, int* __restrict__ m) {
  int v[2] = {0, 0};
  const bool word_ok = (reinterpret_cast<uintptr_t>(labels) & 3) == 0;
  const int groups = (n + 3) >> 2;
  for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += gridDim.x * blockDim.x) {
    const int i0 = g << 2;
    if (word_ok && i0 + 4 <= n) {
      unsigned w = *reinterpret_cast<const unsigned*>(labels + i0);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        unsigned b = (w >> (8 * j)) & 0xffu;
        v[0] += b == 1u;
        v[1] += b == 0u;
      }
    } else {
      for (int i = i0; i < n && i < i0 + 4; ++i) {
        int b = labels[i];
        v[0] += b == 1;
        v[1] += b == 0;
      }
    }
  }
  block_add_counters<2>(v, m);
}

extern "C" int unit_metrics_rpn(const int8_t* labels, int n, int* m, void* stream) {
  UNIT_CHECK_ARG(n >= 0, "metrics_rpn: negative size");
  UNIT_CHECK_ARG(m != nullptr, "metrics_rpn: null counters");
  if (n == 0) return UNIT_OK;
  UNIT_CHECK_ARG(labels != nullptr, "metrics_rpn: null labels");
  int blocks = min(1024, cdiv(cdiv(n, 4), METRICS_THREADS));
  metrics_rpn_kernel<<<blocks, METRICS_THREADS, 0, (hipStream_t)stream>>>(labels, n, m);
  UNIT_LAUNCH_CHECK();
  return UNIT_OK;
}

// ---------------------------------------------------------------------------------------------------
// classifier rows: G = 8 / 16 / 32 / 64 lanes per row (the smallest that is >= ncls, 64 for 65..96 columns: two per lane), 64 / G rows
// per wave, the lanes of a group on consecutive columns -- a wave reads 64 consecutive floats of the score matrix when ld == ncls.
// argmax by torch.argmax's CPU rule: the lowest index among equal maxima, a NaN larger than anything, the first NaN wins.
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool argmax_takes(float v, int i, float bv, int bi) {
  const bool vn = v != v, bn = bv != bv;
  if (vn != bn) return vn;                     // exactly one NaN: it wins
  if (!vn && v != bv) return v > bv;           // two numbers that differ
  return i < bi;                               // equal (or both NaN): the lower index
}

__global__ void __launch_bounds__(METRICS_THREADS) metrics_fastrcnn_kernel(const float* __restrict__ scores, int ld, int col0, int ncls,
                                                                            const int* __restrict__ roi_cls, int R, int lg,
                                                                            int* __restrict__ m) {
  const int G = 1 << lg;
  const int sub = threadIdx.x & (G - 1);
  const int rows_per_block = blockDim.x >> lg;
  const int K = ncls - 1;
  int v[5] = {0, 0, 0, 0, 0};
  // (uniform trip count per workgroup: every lane reaches the shuffles)
  for (int r0 = blockIdx.x * rows_per_block; r0 < R; r0 += gridDim.x * rows_per_block) {
    const int r = r0 + (threadIdx.x >> lg);
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    if (r < R) {
      const float* x = scores + (size_t)r * ld + col0;
      for (int c = sub; c < ncls; c += G) {          // ascending columns: a strict "takes" keeps the first of equals
        float xv = x[c];
        if (argmax_takes(xv, c, bv, bi)) { bv = xv; bi = c; }
      }
    }
    for (int o = G >> 1; o > 0; o >>= 1) {
      float ov = __shfl_xor(bv, o, 64);
      int oi = __shfl_xor(bi, o, 64);
      if (argmax_takes(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    if (sub == 0 && r < R) {
      const int gt = roi_cls[r];
      if (gt >= 0 && gt <= K) {                      // anything else is an empty slot (unit_gather_rois writes -1), no instance
        const bool fg = gt < K, hit = bi == gt;
        v[0] += 1;
        v[1] += hit;
        v[2] += fg;
        v[3] += fg && hit;
        v[4] += fg && bi == K;
      }
    }
  }
  block_add_counters<5>(v, m);
}

extern "C" int unit_metrics_fastrcnn(const float* scores, int ld, int col0, int ncls, const int* roi_cls, int R, int* m, void* stream) {
  UNIT_CHECK_ARG(R >= 0 && ld >= 0 && col0 >= 0 && ncls >= 1, "metrics_fastrcnn: negative size");
  if (ncls > 96) { unit_set_error("metrics_fastrcnn: at most 96 columns (the bound of the loss kernels)"); return UNIT_ERR_UNSUPPORTED; }
  UNIT_CHECK_ARG((long)col0 + ncls <= ld, "metrics_fastrcnn: col0 + ncls exceeds the row stride");
  UNIT_CHECK_ARG(m != nullptr, "metrics_fastrcnn: null counters");
  if (R == 0) return UNIT_OK;
  UNIT_CHECK_ARG(scores != nullptr && roi_cls != nullptr, "metrics_fastrcnn: null input");
  int lg = 3;
  while ((1 << lg) < ncls && lg < 6) ++lg;
  int rows_per_block = METRICS_THREADS >> lg;
  int blocks = min(1024, cdiv(R, rows_per_block));
  metrics_fastrcnn_kernel<<<blocks, METRICS_THREADS, 0, (hipStream_t)stream>>>(scores, ld, col0, ncls, roi_cls, R, lg, m);
  UNIT_LAUNCH_CHECK();
  return UNIT_OK;
}

// ---------------------------------------------------------------------------------------------------
// mask logits in unit_mask_bce_loss's layout, [S][P][P][4][ldk] fp32 (P = M / 2; pixel (Y, X) -> [Y/2][X/2][(Y&1)*2 + (X&1)]), targets
// [S][M][M] uint8 (0 / 1, unit_mask_targets). Only the gt-class column of every ldk-float pixel row is read, so no lane order makes the
// logit reads contiguous: the lanes walk the pixel rows in MEMORY order (one constant stride between lanes); the four target bytes of a
// 2x2 cell come from two 28-byte image rows that stay in cache.
// ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(METRICS_THREADS) metrics_mask_kernel(const float* __restrict__ logits, int K, int ldk,
                                                                        const int* __restrict__ cls, const unsigned char* __restrict__ tgt,
                                                                        int S, int M, int* __restrict__ m) {
  const int P = M >> 1, MM = M * M;
  const long total = (long)S * MM;
  int v[5] = {0, 0, 0, 0, 0};
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int s = (int)(i / MM);
    const int j = (int)(i - (long)s * MM);          // pixel row of the slot in memory order: ((Y/2) * P + X/2) * 4 + (Y&1)*2 + (X&1)
    const int c = cls[s];
    if (c < 0 || c >= K) continue;
    const int q = j & 3, cell = j >> 2;
    const int Y = (cell / P) * 2 + (q >> 1), X = (cell % P) * 2 + (q & 1);
    const bool pred = logits[(size_t)i * ldk + c] > 0.0f;
    const bool t = tgt[(size_t)s * MM + Y * M + X] != 0;
    v[0] += 1;
    v[1] += pred != t;
    v[2] += t;
    v[3] += pred && !t;
    v[4] += !pred && t;
  }
  block_add_counters<5>(v, m);
}

extern "C" int unit_metrics_mask(const float* logits, int K, int ldk, const int* cls, const unsigned char* targets, int S, int M, int* m,
                                 void* stream) {
  UNIT_CHECK_ARG(S >= 0 && M >= 0 && K >= 0 && ldk >= 0, "metrics_mask: negative size");
  UNIT_CHECK_ARG((M & 1) == 0, "metrics_mask: M must be even (2x2 deconvolution cells)");
  UNIT_CHECK_ARG(K <= ldk, "metrics_mask: K exceeds the pixel row stride");
  UNIT_CHECK_ARG(m != nullptr, "metrics_mask: null counters");
  if (S == 0 || M == 0 || K == 0) return UNIT_OK;
  UNIT_CHECK_ARG(logits != nullptr && cls != nullptr && targets != nullptr, "metrics_mask: null input");
  int blocks = min(1024, cdiv((long)S * M * M, METRICS_THREADS));
  metrics_mask_kernel<<<blocks, METRICS_THREADS, 0, (hipStream_t)stream>>>(logits, K, ldk, cls, targets, S, M, m);
  UNIT_LAUNCH_CHECK();
  return UNIT_OK;
}
