// similarity.hip -- the similarity terms of WSROIHead.get_similarity_matrices beyond 'lingual' + 'visual' under "Sum"
// (modeling/roi_heads/roi_heads.py:245-336): TopK-k, WTopK-k, LSDA-k (:273-305, from the refinement predictors' weights), VisualK-k
// (:306-315, per RoI), Average (:318-320), None (:321-324) and the "Product" combination (:325-332). detect.hip keeps the two-term
// kernels; modeling/similarity_terms.py decides per head which of the two a term list takes.
//   unit_similarity_static   A[n][b] = w (softmax(lingual) + TopK + WTopK + LSDA)      one workgroup per novel class
//   unit_similarity_ex       sim[R][n][b] = normalise(A + w (VisualK | visual)) | 1/b | 0   one wavefront per RoI
//   unit_similarity_bwd_ex   dsim -> d(refinement logits) through the per-RoI term          one wavefront per RoI
#include "common.h"

#define SIM_MAXB 96           // base classes: DET_MAXC of detect.hip
#define SIM_MAXC 128          // logit columns of one refinement stream: two per lane

// wave arg-max of (v, i): the larger v, on equal v the smaller i; i < 0 = no candidate
__device__ __forceinline__ void wave_argmax(float& v, int& i) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    float ov = __shfl_xor(v, o, 64);
    int oi = __shfl_xor(i, o, 64);
    if (oi >= 0 && (i < 0 || ov > v || (ov == v && oi < i))) { v = ov; i = oi; }
  }
}

// torch.topk(k) of a row of n <= 128 values held two per lane (columns lane and lane + 64): k rounds of a wave arg-max
// (largest = false: arg-min), first index on ties -> s0 / s1: is this lane's column selected
__device__ __forceinline__ void wave_topk(float v0, float v1, int n, int k, bool largest, bool& s0, bool& s1) {
  int lane = threadIdx.x & 63;
  float a0 = largest ? v0 : -v0, a1 = largest ? v1 : -v1;
  s0 = s1 = false;
  for (int t = 0; t < k; ++t) {
    float bv = 0.f;
    int bi = -1;
    if (lane < n && !s0) { bv = a0; bi = lane; }
    if (lane + 64 < n && !s1 && (bi < 0 || a1 > bv)) { bv = a1; bi = lane + 64; }
    wave_argmax(bv, bi);
    if (bi == lane) s0 = true;
    if (bi == lane + 64) s1 = true;
  }
}

// every lane: s[0] + s[1] + ... in index order -- the order of detect.hip's one-thread-per-RoI kernel, so that a plan of 'lingual' /
// 'visual' alone gives the same bits on both paths
__device__ __forceinline__ float seq_sum(const float* s, int n) {
  float t = 0.f;
  for (int i = 0; i < n; ++i) t += s[i];
  return t;
}

// ---------------------------------------------------------------------------------------------------
// The per-model part (roi_heads.py:270-305). W = mean over the refinement predictors of `weight` (rows row0 + k * ncls + c of the
// fused fp32 master matrix, D columns), S = W[novel] W[base]^T, dist = |W[novel_j] - W[base_b]|_2:
//   A[j][b] = 0 + w softmax(lingual[j])[b] + w TopK + w WTopK + w LSDA           (in the reference's order; a k of 0 = term absent)
//   TopK:  1/k on the k largest S[j][:]      WTopK: S[j][b] / (sum of the k largest) on them (no clamp)      LSDA: 1/k on the k smallest dist
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void similarity_static_kernel(const float* __restrict__ w, int ld, int row0, int n_oicr, int ncls, int D,
                                                                const int* __restrict__ base, int n_base, const int* __restrict__ novel,
                                                                const float* __restrict__ lingual, float wgt, int use_lingual, int k_topk,
                                                                int k_wtopk, int k_lsda, float* __restrict__ A) {
  extern __shared__ float smem[];          // nv[D] | dotv[SIM_MAXB] | dist[SIM_MAXB]
  float* nv = smem;
  float* dotv = smem + D;
  float* dist = dotv + SIM_MAXB;
  int j = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (k_topk | k_wtopk | k_lsda) {
    const float* wn = w + (size_t)(row0 + novel[j]) * ld;
    for (int d = tid; d < D; d += 256) {
      float s = 0.f;
      for (int k = 0; k < n_oicr; ++k) s += wn[(size_t)k * ncls * ld + d];
      nv[d] = s / (float)n_oicr;
    }
    __syncthreads();
    for (int b = wv; b < n_base; b += 4) {
      const float* wb = w + (size_t)(row0 + base[b]) * ld;
      float dp = 0.f, ds = 0.f;
      for (int d = lane; d < D; d += 64) {
        float s = 0.f;
        for (int k = 0; k < n_oicr; ++k) s += wb[(size_t)k * ncls * ld + d];
        s = s / (float)n_oicr;
        float df = nv[d] - s;
        dp += nv[d] * s;
        ds += df * df;
      }
      dp = wave_reduce_sum(dp);
      ds = wave_reduce_sum(ds);
      if (lane == 0) { dotv[b] = dp; dist[b] = sqrtf(ds); }
    }
    __syncthreads();
  }
  if (wv != 0) return;
  int b0 = lane, b1 = lane + 64;
  bool in0 = b0 < n_base, in1 = b1 < n_base;
  float acc0 = 0.f, acc1 = 0.f;
  if (use_lingual) {
    const float* L = lingual + (size_t)j * n_base;
    float lmx = -INFINITY, lse = 0.f;
    for (int b = 0; b < n_base; ++b) lmx = fmaxf(lmx, L[b]);
    for (int b = 0; b < n_base; ++b) lse += expf(L[b] - lmx);
    if (in0) acc0 = acc0 + wgt * (expf(L[b0] - lmx) / lse);
    if (in1) acc1 = acc1 + wgt * (expf(L[b1] - lmx) / lse);
  }
  float s0v = in0 ? dotv[b0] : 0.f, s1v = in1 ? dotv[b1] : 0.f;
  bool s0, s1;
  if (k_topk) {
    wave_topk(s0v, s1v, n_base, k_topk, true, s0, s1);
    float t = 1.0f / (float)k_topk;
    if (s0) acc0 = acc0 + wgt * t;
    if (s1) acc1 = acc1 + wgt * t;
  }
  if (k_wtopk) {
    wave_topk(s0v, s1v, n_base, k_wtopk, true, s0, s1);
    float tsum = wave_reduce_sum((s0 ? s0v : 0.f) + (s1 ? s1v : 0.f));
    if (s0) acc0 = acc0 + wgt * (s0v / tsum);
    if (s1) acc1 = acc1 + wgt * (s1v / tsum);
  }
  if (k_lsda) {
    wave_topk(in0 ? dist[b0] : 0.f, in1 ? dist[b1] : 0.f, n_base, k_lsda, false, s0, s1);
    float t = 1.0f / (float)k_lsda;
    if (s0) acc0 = acc0 + wgt * t;
    if (s1) acc1 = acc1 + wgt * t;
  }
  if (in0) A[(size_t)j * n_base + b0] = acc0;
  if (in1) A[(size_t)j * n_base + b1] = acc1;
}

extern "C" int unit_similarity_static(const float* w_master, int ld, int row0, int n_oicr, int ncls, int D, const int* base_dev, int n_base,
                                      const int* novel_dev, int n_novel, const float* lingual, float weight, int use_lingual, int k_topk,
                                      int k_wtopk, int k_lsda, float* A, void* stream) {
  UNIT_CHECK_ARG(n_base >= 1 && n_base <= SIM_MAXB, "similarity_static: 1 .. 96 base classes");
  UNIT_CHECK_ARG(n_oicr >= 1 && D >= 1 && D <= 8192 && ld >= D, "similarity_static: n_oicr >= 1, 1 <= D <= 8192, ld >= D");
  UNIT_CHECK_ARG(row0 >= 0 && ncls >= 1 && n_novel >= 0, "similarity_static: row0 >= 0, ncls >= 1, n_novel >= 0");
  UNIT_CHECK_ARG(k_topk >= 0 && k_topk <= n_base && k_wtopk >= 0 && k_wtopk <= n_base && k_lsda >= 0 && k_lsda <= n_base,
                 "similarity_static: every k in [0, n_base]");
  if (n_novel == 0) return UNIT_OK;
  size_t lds = (size_t)(D + 2 * SIM_MAXB) * sizeof(float);
  similarity_static_kernel<<<n_novel, 256, lds, (hipStream_t)stream>>>(w_master, ld, row0, n_oicr, ncls, D, base_dev, n_base, novel_dev, lingual,
                                                                     weight, use_lingual, k_topk, k_wtopk, k_lsda, A);
  UNIT_LAUNCH_CHECK();
  return UNIT_OK;
}

// ---------------------------------------------------------------------------------------------------
// The per-RoI term of one row, base columns lane and lane + 64 (roi_heads.py:250-257 'visual', :306-314 'VisualK'):
//   p = mean_k oicr_k(x)      visual:  q = softmax(p[0 .. K])      VisualK: q = softmax(p[0 .. K - 1])   (no background column)
//   m = q[base] / max(sum q[base], 1e-9)
//   visual:  v = m, zero below the threshold          VisualK: v = m / (sum of the k largest m) on them, zero elsewhere
// 'visual' keeps similarity_kernel's operations and their order (detect.hip). Leaves exp(p - max) of the softmax columns in `ebuf`.
// ---------------------------------------------------------------------------------------------------
struct RowTerm {
  float v0, v1, m0, m1, q0, q1;
  float se, tot, tsum;
  bool s0, s1;          // kept (visual) / selected (VisualK)
};

__device__ __forceinline__ RowTerm row_term(const float* __restrict__ x, int n_oicr, int ncls, const int* __restrict__ base, int n_base, float thr,
                                            int use_visual, int k_visual, float* ebuf, float* sbuf) {
  int lane = threadIdx.x & 63;
  int nc = use_visual ? ncls : ncls - 1;
  RowTerm t;
  float p0 = -INFINITY, p1 = -INFINITY;
  if (lane < nc) {
    float s = 0.f;
    for (int k = 0; k < n_oicr; ++k) s += x[k * ncls + lane];
    p0 = s / (float)n_oicr;
  }
  if (lane + 64 < nc) {
    float s = 0.f;
    for (int k = 0; k < n_oicr; ++k) s += x[k * ncls + lane + 64];
    p1 = s / (float)n_oicr;
  }
  float mx = wave_reduce_max(fmaxf(p0, p1));
  if (lane < nc) ebuf[lane] = expf(p0 - mx);
  if (lane + 64 < nc) ebuf[lane + 64] = expf(p1 - mx);
  __syncthreads();
  t.se = seq_sum(ebuf, nc);
  bool in0 = lane < n_base, in1 = lane + 64 < n_base;
  t.q0 = in0 ? ebuf[base[lane]] / t.se : 0.f;
  t.q1 = in1 ? ebuf[base[lane + 64]] / t.se : 0.f;
  if (in0) sbuf[lane] = t.q0;
  if (in1) sbuf[lane + 64] = t.q1;
  __syncthreads();
  t.tot = seq_sum(sbuf, n_base);
  float totc = fmaxf(t.tot, 1e-9f);
  t.m0 = t.q0 / totc;
  t.m1 = t.q1 / totc;
  t.tsum = 1.f;
  if (use_visual) {
    t.s0 = in0 && !(t.m0 < thr);
    t.s1 = in1 && !(t.m1 < thr);
    t.v0 = t.s0 ? t.m0 : 0.f;
    t.v1 = t.s1 ? t.m1 : 0.f;
  } else {
    wave_topk(t.m0, t.m1, n_base, k_visual, true, t.s0, t.s1);
    t.tsum = wave_reduce_sum((t.s0 ? t.m0 : 0.f) + (t.s1 ? t.m1 : 0.f));
    t.v0 = t.s0 ? t.m0 / t.tsum : 0.f;
    t.v1 = t.s1 ? t.m1 / t.tsum : 0.f;
  }
  __syncthreads();          // sbuf is the caller's from here
  return t;
}

// sim[r][j][b] (roi_heads.py:315-324 "Sum", :325-332 "Product"):
//   u = A[j][b] + w v[r][b]  ;  Average: u = 1/b  ;  sim = u / max(sum_b u, 1e-9)        none: 0        product: softmax(0) = 1/b
__global__ __launch_bounds__(64) void similarity_ex_kernel(const float* __restrict__ lin, int ld, int col0, int n_oicr, int ncls,
                                                           const int* __restrict__ base, int n_base, const float* __restrict__ A, int n_novel,
                                                           float thr, float wgt, int use_visual, int k_visual, int average, int none, int product,
                                                           float* __restrict__ sim) {
  __shared__ float ebuf[SIM_MAXC];
  __shared__ float sbuf[SIM_MAXB];
  int r = blockIdx.x, lane = threadIdx.x;
  bool in0 = lane < n_base, in1 = lane + 64 < n_base;
  float* o = sim + (size_t)r * n_novel * n_base;
  if (none || product) {
    float c = none ? 0.f : 1.0f / (float)n_base;          // (an empty list is zero under either combination)
    for (int j = 0; j < n_novel; ++j) {
      if (in0) o[(size_t)j * n_base + lane] = c;
      if (in1) o[(size_t)j * n_base + lane + 64] = c;
    }
    return;
  }
  bool per_row = (use_visual || k_visual) && !average;
  RowTerm t;
  t.v0 = t.v1 = 0.f;
  if (per_row) t = row_term(lin + (size_t)r * ld + col0, n_oicr, ncls, base, n_base, thr, use_visual, k_visual, ebuf, sbuf);
  for (int j = 0; j < n_novel; ++j) {
    float u0 = 0.f, u1 = 0.f;
    if (average) {
      u0 = u1 = 1.0f / (float)n_base;
    } else {
      if (in0) u0 = A[(size_t)j * n_base + lane];
      if (in1) u1 = A[(size_t)j * n_base + lane + 64];
      if (per_row) { u0 = u0 + wgt * t.v0; u1 = u1 + wgt * t.v1; }
    }
    if (in0) sbuf[lane] = u0;
    if (in1) sbuf[lane + 64] = u1;
    __syncthreads();
    float T = fmaxf(seq_sum(sbuf, n_base), 1e-9f);
    __syncthreads();
    if (in0) o[(size_t)j * n_base + lane] = u0 / T;
    if (in1) o[(size_t)j * n_base + lane + 64] = u1 / T;
  }
}

#define SIM_EX_CHECKS(what)                                                                                                        \
  UNIT_CHECK_ARG(n_base >= 1 && n_base <= SIM_MAXB, what ": 1 .. 96 base classes");                                                \
  UNIT_CHECK_ARG(ncls >= 2 && ncls <= SIM_MAXC && n_oicr >= 1, what ": 2 .. 128 logit columns per stream, n_oicr >= 1");           \
  UNIT_CHECK_ARG(!(use_visual && k_visual), what ": 'visual' and 'VisualK' exclude each other");                                   \
  UNIT_CHECK_ARG(k_visual >= 0 && k_visual <= n_base, what ": VisualK's k in [0, n_base] (0: no VisualK term)")

extern "C" int unit_similarity_ex(const float* lin_weak, int ld, int col0, int n_oicr, int ncls, const int* base_dev, int n_base, const float* A,
                                  int n_novel, float visual_threshold, float weight, int use_visual, int k_visual, int average, int none,
                                  int product, float* sim, int R, void* stream) {
  SIM_EX_CHECKS("similarity_ex");
  UNIT_CHECK_ARG(col0 >= 0 && col0 + n_oicr * ncls <= ld, "similarity_ex: the logit columns leave the row");
  if (R == 0 || n_novel == 0) return UNIT_OK;
  similarity_ex_kernel<<<R, 64, 0, (hipStream_t)stream>>>(lin_weak, ld, col0, n_oicr, ncls, base_dev, n_base, A, n_novel, visual_threshold, weight,
                                                        use_visual, k_visual, average, none, product, sim);
  UNIT_LAUNCH_CHECK();
  return UNIT_OK;
}

// ---------------------------------------------------------------------------------------------------
// Backward of similarity_ex_kernel for the per-RoI term (the reference computes it with grad in the fine-tune heads' training forward,
// roi_heads.py:852): dsim [R][n][b] -> the n_oicr logit groups of dlin, 1 / n_oicr each (cf. similarity_bwd_kernel, detect.hip).
//   S = u / Tc, u[j][b] = A[j][b] + w v[b], Tc = max(T, 1e-9):      dv[b] = sum_j w (G[j][b] - [T >= 1e-9] sum_b G S) / Tc
//   visual:   dm = dv on the kept entries (the in-place zeroing passes nothing to the others)
//   VisualK:  v = m / ts on the selected entries, ts = their sum (no clamp):      dm = (dv - sum_sel dv v) / ts on them, 0 elsewhere
//   m = q[base] / max(tot, 1e-9):      dq[base] = (dm - [tot >= 1e-9] sum dm m) / max(tot, 1e-9)
//   q = softmax(p) over the term's columns:      dp = q (dq - sum q dq)           (VisualK: the background column gets 0)
// ---------------------------------------------------------------------------------------------------
template <typename TD>
__global__ __launch_bounds__(64) void similarity_bwd_ex_kernel(const float* __restrict__ lin, int ld, int col0, int n_oicr, int ncls,
                                                               const int* __restrict__ base, int n_base, const float* __restrict__ A, int n_novel,
                                                               float thr, float wgt, int use_visual, int k_visual,
                                                               const float* __restrict__ dsim, TD* __restrict__ dlin, int ldl, int dcol0) {
  __shared__ float ebuf[SIM_MAXC];
  __shared__ float sbuf[SIM_MAXB];
  __shared__ float dqc[SIM_MAXC];
  int r = blockIdx.x, lane = threadIdx.x;
  bool in0 = lane < n_base, in1 = lane + 64 < n_base;
  RowTerm t = row_term(lin + (size_t)r * ld + col0, n_oicr, ncls, base, n_base, thr, use_visual, k_visual, ebuf, sbuf);
  const float* g = dsim + (size_t)r * n_novel * n_base;
  float dv0 = 0.f, dv1 = 0.f;
  for (int j = 0; j < n_novel; ++j) {
    float u0 = 0.f, u1 = 0.f, g0 = 0.f, g1 = 0.f;
    if (in0) { u0 = A[(size_t)j * n_base + lane] + wgt * t.v0; g0 = g[(size_t)j * n_base + lane]; }
    if (in1) { u1 = A[(size_t)j * n_base + lane + 64] + wgt * t.v1; g1 = g[(size_t)j * n_base + lane + 64]; }
    float T = wave_reduce_sum(u0 + u1);
    float Tc = fmaxf(T, 1e-9f);
    float dot = T >= 1e-9f ? wave_reduce_sum(g0 * (u0 / Tc) + g1 * (u1 / Tc)) : 0.f;
    dv0 += wgt * (g0 - dot) / Tc;
    dv1 += wgt * (g1 - dot) / Tc;
  }
  if (!t.s0) dv0 = 0.f;
  if (!t.s1) dv1 = 0.f;
  if (!use_visual) {
    float dk = wave_reduce_sum(dv0 * t.v0 + dv1 * t.v1);
    dv0 = t.s0 ? (dv0 - dk) / t.tsum : 0.f;
    dv1 = t.s1 ? (dv1 - dk) / t.tsum : 0.f;
  }
  float totc = fmaxf(t.tot, 1e-9f);
  float dot2 = t.tot >= 1e-9f ? wave_reduce_sum(dv0 * t.m0 + dv1 * t.m1) : 0.f;
  float dq0 = in0 ? (dv0 - dot2) / totc : 0.f, dq1 = in1 ? (dv1 - dot2) / totc : 0.f;
  float sq = wave_reduce_sum(t.q0 * dq0 + t.q1 * dq1);
  dqc[lane] = 0.f;
  dqc[lane + 64] = 0.f;
  __syncthreads();
  if (in0) dqc[base[lane]] = dq0;
  if (in1) dqc[base[lane + 64]] = dq1;
  __syncthreads();
  int nc = use_visual ? ncls : ncls - 1;
  TD* o = dlin + (size_t)r * ldl + dcol0;
  for (int c = lane; c < ncls; c += 64) {
    float q = c < nc ? ebuf[c] / t.se : 0.f;
    float dp = q * (dqc[c] - sq) / (float)n_oicr;
    for (int k = 0; k < n_oicr; ++k) o[k * ncls + c] = (TD)dp;
  }
}

extern "C" int unit_similarity_bwd_ex(const float* lin_weak, int ld, int col0, int n_oicr, int ncls, const int* base_dev, int n_base, const float* A,
                                      int n_novel, float visual_threshold, float weight, int use_visual, int k_visual, int average, int none,
                                      int product, const float* dsim, void* dlin, int dlin_dtype, int ldl, int dcol0, int R, void* stream) {
  SIM_EX_CHECKS("similarity_bwd_ex");
  UNIT_CHECK_ARG(dcol0 >= 0 && dcol0 + n_oicr * ncls <= ldl && col0 >= 0 && col0 + n_oicr * ncls <= ld, "similarity_bwd_ex: the logit columns leave the row");
  if (R == 0) return UNIT_OK;
  hipStream_t st = (hipStream_t)stream;
  (void)hipMemsetAsync(dlin, 0, (size_t)R * ldl * (dlin_dtype == UNIT_BF16 ? 2 : 4), st);
  if (average || none || product || !(use_visual || k_visual) || n_novel == 0) return UNIT_OK;          // no per-RoI term: the matrix does not depend on the logits
  if (dlin_dtype == UNIT_BF16)
    similarity_bwd_ex_kernel<bf16_t><<<R, 64, 0, st>>>(lin_weak, ld, col0, n_oicr, ncls, base_dev, n_base, A, n_novel, visual_threshold, weight,
                                                     use_visual, k_visual, dsim, (bf16_t*)dlin, ldl, dcol0);
  else
    similarity_bwd_ex_kernel<float><<<R, 64, 0, st>>>(lin_weak, ld, col0, n_oicr, ncls, base_dev, n_base, A, n_novel, visual_threshold, weight,
                                                    use_visual, k_visual, dsim, (float*)dlin, ldl, dcol0);
  UNIT_LAUNCH_CHECK();
  return UNIT_OK;
}
