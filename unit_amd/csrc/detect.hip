// detect.hip -- base->novel similarity transfer (fine-tune / eval predictor) and the detection post-processing.
//   a14  WSROIHead.get_similarity_matrices  modeling/roi_heads/roi_heads.py:245-336  ('lingual' + 'visual', "Sum"; every other term and
//        "Product": similarity.hip)
//        SupervisedDetectorOutputs*.forward transfer   modeling/roi_heads/fast_rcnn.py:401-423, 504-523
//   a15  SupervisedDetectorOutputsBase.inference -> detectron2 fast_rcnn_inference (fast_rcnn.py:455-468)
#include "common.h"

#define DET_MAXC 96

// out[i][j] = sum_k a[i][k] * b[j][k]   (tiny: label-embedding similarity 5x300 . 15x300^T, fast_rcnn.py:376-382)
__global__ void small_matmul_nt_kernel(const float* __restrict__ a, const int* __restrict__ arow, int M, const float* __restrict__ b,
                                       const int* __restrict__ brow, int N, int Kd, int lda, float* __restrict__ out) {
  int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= M * N) return;
  int i = idx / N, j = idx - i * N;
  const float* pa = a + (size_t)(arow ? arow[i] : i) * lda;
  const float* pb = b + (size_t)(brow ? brow[j] : j) * lda;
  float s = 0.f;
  for (int k = 0; k < Kd; ++k) s += pa[k] * pb[k];
  out[idx] = s;
}
extern "C" int unit_embedding_similarity(const float* emb, int ld, int dim, const int* novel_rows, int n_novel, const int* base_rows,
                                         int n_base, float* out, void* stream) {
  if (n_novel * n_base == 0) return UNIT_OK;
  small_matmul_nt_kernel<<<cdiv(n_novel * n_base, 128), 128, 0, (hipStream_t)stream>>>(emb, novel_rows, n_novel, emb, base_rows, n_base, dim, ld, out);
  UNIT_LAUNCH_CHECK();
  return UNIT_OK;
}

// sim[r][j][b] for j in novel, b in base (roi_heads.py:250-257, 269-272, 316-322):
//   probs = mean_k oicr_k(x)           (K+1 logits)           vis = softmax(probs)[base] ; vis /= max(sum, 1e-9) ; vis[vis < thr] = 0
//   s = 0.5 * softmax(lingual[j,:]) + 0.5 * vis              s /= max(sum_b s, 1e-9)
__global__ void similarity_kernel(const float* __restrict__ lin, int ld, int col0, int n_oicr, int ncls, const int* __restrict__ base,
                                  int n_base, const float* __restrict__ lingual, int n_novel, float thr, int use_lingual,
                                  int use_visual, float* __restrict__ sim, int R) {
  int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  float vis[DET_MAXC];
  if (use_visual) {
    const float* x = lin + (size_t)r * ld + col0;
    float mx = -INFINITY;
    for (int c = 0; c < ncls; ++c) {
      float s = 0.f;
      for (int k = 0; k < n_oicr; ++k) s += x[k * ncls + c];
      mx = fmaxf(mx, s / (float)n_oicr);
    }
    float se = 0.f;
    for (int c = 0; c < ncls; ++c) {
      float s = 0.f;
      for (int k = 0; k < n_oicr; ++k) s += x[k * ncls + c];
      se += expf(s / (float)n_oicr - mx);
    }
    float tot = 0.f;
    for (int b = 0; b < n_base; ++b) {
      int c = base[b];
      float s = 0.f;
      for (int k = 0; k < n_oicr; ++k) s += x[k * ncls + c];
      vis[b] = expf(s / (float)n_oicr - mx) / se;
      tot += vis[b];
    }
    tot = fmaxf(tot, 1e-9f);
    for (int b = 0; b < n_base; ++b) { float v = vis[b] / tot; vis[b] = v < thr ? 0.f : v; }
  }
  float nterms = (float)(use_lingual + use_visual);
  float wgt = nterms > 0.f ? 1.0f / nterms : 0.f;
  for (int j = 0; j < n_novel; ++j) {
    float lmx = -INFINITY, lse = 0.f;
    if (use_lingual) {
      for (int b = 0; b < n_base; ++b) lmx = fmaxf(lmx, lingual[j * n_base + b]);
      for (int b = 0; b < n_base; ++b) lse += expf(lingual[j * n_base + b] - lmx);
    }
    float tot = 0.f;
    float* o = sim + ((size_t)r * n_novel + j) * n_base;
    for (int b = 0; b < n_base; ++b) {
      float s = 0.f;
      if (use_lingual) s = s + wgt * (expf(lingual[j * n_base + b] - lmx) / lse);
      if (use_visual) s = s + wgt * vis[b];
      o[b] = s; tot += s;
    }
    tot = fmaxf(tot, 1e-9f);
    for (int b = 0; b < n_base; ++b) o[b] = nterms > 0.f ? o[b] / tot : 0.f;
  }
}
extern "C" int unit_similarity(const float* lin_weak, int ld, int col0, int n_oicr, int ncls, const int* base_dev, int n_base,
                               const float* lingual, int n_novel, float visual_threshold, int use_lingual, int use_visual,
                               float* sim, int R, void* stream) {
  UNIT_CHECK_ARG(n_base <= DET_MAXC, "similarity: more than 96 base classes");
  if (R == 0) return UNIT_OK;
  similarity_kernel<<<cdiv(R, 64), 64, 0, (hipStream_t)stream>>>(lin_weak, ld, col0, n_oicr, ncls, base_dev, n_base, lingual, n_novel,
                                                                visual_threshold, use_lingual, use_visual, sim, R);
  UNIT_LAUNCH_CHECK();
  return UNIT_OK;
}

// fast_rcnn.py:401-423 / 504-523 + :425-426 (+ :525-528 fine-tune heads):
//   scores[r,c] = delta[r,c] + [c novel] sum_b sim_cls[r,j,b] * delta[r,base_b]  + mean_k oicr_k  (+ ft)
//   bbox[r,c,:] = (c base) delta ; (c novel) sum_b sim_bbox[r,j,b] * delta[r,base_b,:] ; (else) 0   (+ 0 weak) (+ ft)
// WB (unit_transfer_predictions_ex, REGRESSION_BRANCH under the fine-tune predictor): the [R, 4K] block of weak box deltas at column wbcol0 of
// `weak` is added BEFORE the ft term, (o + weak) + ft -- get_cls_bbox (fast_rcnn.py:370-374, :526) runs before `bbox + proposal_ft` (:528).
// Latency-sized (R * (K + 1) threads, a few hundred rows): the base-class loop reads its row of `lin` through L1 / L2 as before; staging the
// row in LDS would add a barrier to a launch whose time is the launch.
template <bool WB>
__global__ void transfer_kernel(const float* __restrict__ lin, int ld, int ccol0, int bcol0, int K, const float* __restrict__ weak, int ldw,
                                int wcol0, int n_oicr, int wbcol0, const float* __restrict__ ft, int ldf, int fccol0, int fbcol0,
                                const float* __restrict__ sim_cls, const float* __restrict__ sim_bbox, const int* __restrict__ base, int n_base,
                                const int* __restrict__ novel, int n_novel, const int8_t* __restrict__ role /* K: 0 none,1 base,2 novel */,
                                const int* __restrict__ slot /* K: index into base/novel list */, float* __restrict__ scores, int lds_,
                                float* __restrict__ bbox, int ldb, int R) {
  int idx = blockIdx.x * blockDim.x + threadIdx.x;
  int ncls = K + 1;
  if (idx >= R * ncls) return;
  int r = idx / ncls, c = idx - r * ncls;
  const float* x = lin + (size_t)r * ld;
  float s = x[ccol0 + c];
  if (c < K && sim_cls && role[c] == 2) {
    const float* sm = sim_cls + ((size_t)r * n_novel + slot[c]) * n_base;
    float t = 0.f;
    for (int b = 0; b < n_base; ++b) t += sm[b] * x[ccol0 + base[b]];
    s = s + t;
  }
  if (weak) {
    float w = 0.f;
    for (int k = 0; k < n_oicr; ++k) w += weak[(size_t)r * ldw + wcol0 + k * ncls + c];
    s = s + w / (float)n_oicr;
  }
  if (ft) s = s + ft[(size_t)r * ldf + fccol0 + c];
  scores[(size_t)r * lds_ + c] = s;
  if (c >= K) return;
  float o[4] = {0.f, 0.f, 0.f, 0.f};
  if (!sim_bbox || role[c] == 1) {
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = x[bcol0 + 4 * c + j];
  } else if (role[c] == 2) {
    const float* sm = sim_bbox + ((size_t)r * n_novel + slot[c]) * n_base;
    for (int b = 0; b < n_base; ++b) {
      float w = sm[b];
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] += w * x[bcol0 + 4 * base[b] + j];
    }
  }
  if (WB) {
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = o[j] + weak[(size_t)r * ldw + wbcol0 + 4 * c + j];
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) bbox[(size_t)r * ldb + 4 * c + j] = o[j] + (ft ? ft[(size_t)r * ldf + fbcol0 + 4 * c + j] : 0.f);
}
extern "C" int unit_transfer_predictions(const float* lin, int ld, int ccol0, int bcol0, int K, const float* weak, int ldw, int wcol0,
                                         int n_oicr, const float* ft, int ldf, int fccol0, int fbcol0, const float* sim_cls,
                                         const float* sim_bbox, const int* base_dev, int n_base, const int* novel_dev, int n_novel,
                                         const int8_t* role_dev, const int* slot_dev, float* scores, int lds, float* bbox, int ldb,
                                         int R, void* stream) {
  if (R == 0) return UNIT_OK;
  transfer_kernel<false><<<cdiv(R * (K + 1), 256), 256, 0, (hipStream_t)stream>>>(lin, ld, ccol0, bcol0, K, weak, ldw, wcol0, n_oicr, -1, ft, ldf,
                                                                              fccol0, fbcol0, sim_cls, sim_bbox, base_dev, n_base, novel_dev,
                                                                              n_novel, role_dev, slot_dev, scores, lds, bbox, ldb, R);
  UNIT_LAUNCH_CHECK();
  return UNIT_OK;
}
// unit_transfer_predictions plus the weak head's box deltas: wbcol0 >= 0 is the first of 4K columns of `weak` added to the transferred deltas
// before the ft term; wbcol0 < 0 is the entry above, bit for bit (the same instantiation).
extern "C" int unit_transfer_predictions_ex(const float* lin, int ld, int ccol0, int bcol0, int K, const float* weak, int ldw, int wcol0,
                                            int n_oicr, int wbcol0, const float* ft, int ldf, int fccol0, int fbcol0, const float* sim_cls,
                                            const float* sim_bbox, const int* base_dev, int n_base, const int* novel_dev, int n_novel,
                                            const int8_t* role_dev, const int* slot_dev, float* scores, int lds, float* bbox, int ldb,
                                            int R, void* stream) {
  if (R == 0) return UNIT_OK;          // (an empty matrix has no address: nothing to check, nothing to launch)
  UNIT_CHECK_ARG(wbcol0 < 0 || weak != nullptr, "transfer_predictions_ex: wbcol0 names columns of `weak`, which is NULL");
  UNIT_CHECK_ARG(wbcol0 < 0 || (long)wbcol0 + 4L * K <= (long)ldw, "transfer_predictions_ex: wbcol0 + 4K columns pass the row stride of `weak`");
  UNIT_CHECK_ARG(n_base <= DET_MAXC, "transfer_predictions_ex: more than 96 base classes");
  dim3 grid(cdiv(R * (K + 1), 256));
  hipStream_t st = (hipStream_t)stream;
  if (wbcol0 >= 0)
    transfer_kernel<true><<<grid, 256, 0, st>>>(lin, ld, ccol0, bcol0, K, weak, ldw, wcol0, n_oicr, wbcol0, ft, ldf, fccol0, fbcol0, sim_cls, sim_bbox,
                                                base_dev, n_base, novel_dev, n_novel, role_dev, slot_dev, scores, lds, bbox, ldb, R);
  else
    transfer_kernel<false><<<grid, 256, 0, st>>>(lin, ld, ccol0, bcol0, K, weak, ldw, wcol0, n_oicr, -1, ft, ldf, fccol0, fbcol0, sim_cls, sim_bbox,
                                                 base_dev, n_base, novel_dev, n_novel, role_dev, slot_dev, scores, lds, bbox, ldb, R);
  UNIT_LAUNCH_CHECK();
  return UNIT_OK;
}

// ---------------------------------------------------------------------------------------------------
// Backward of the transfer (fine-tune configurations whose box head trains: COCO-RCNN-50-C4-split1-segm-ft.yaml). The reference
// computes the similarity WITHOUT no_grad in training (roi_heads.py:852 -> :245-336), so d(loss) flows
//   scores / bbox -> [delta heads' outputs (frozen weights, but their input is the trainable box head's feature), similarity]
//   dlin_cls[r,c]    = dsc[r,c] + [c base] sum_j sim_cls[r,j,slot c] dsc[r,novel_j]
//   dlin_bbox[r,c,:] = [c base] (dbb[r,c,:] + sum_j sim_bbox[r,j,slot c] dbb[r,novel_j,:])       (novel / other rows of the delta
//                      head are overwritten by the transfer: no gradient)
//   dsim[r,j,b]      = dsc[r,novel_j] lin_cls[r,base_b] + sum_k dbb[r,novel_j,k] lin_bbox[r,base_b,k]   (cls and bbox use the
//                      same matrix when their term lists are equal; `dsim` is WRITTEN here, the mask head adds to it afterwards)
// dy = d(loss)/d[scores | bbox] in the ft heads' column layout (dccol0 / dbcol0); dlin has the delta heads' layout.
// ---------------------------------------------------------------------------------------------------
template <typename TD>
__global__ void transfer_bwd_kernel(const TD* __restrict__ dy, int ldd, int dccol0, int dbcol0, const float* __restrict__ lin, int ld,
                                    int ccol0, int bcol0, int K, const float* __restrict__ sim_cls, const float* __restrict__ sim_bbox,
                                    const int* __restrict__ base, int n_base, const int* __restrict__ novel, int n_novel,
                                    const int8_t* __restrict__ role, const int* __restrict__ slot, TD* __restrict__ dlin, int ldl,
                                    float* __restrict__ dsim, int R) {
  int idx = blockIdx.x * blockDim.x + threadIdx.x;
  int ncls = K + 1;
  int n1 = R * ncls, n2 = R * n_novel * n_base;
  if (idx < n1) {
    int r = idx / ncls, c = idx - r * ncls;
    const TD* d = dy + (size_t)r * ldd;
    float g = (float)d[dccol0 + c];
    float gb[4] = {0.f, 0.f, 0.f, 0.f};
    if (c < K && role[c] == 1) {
      int sb = slot[c];
#pragma unroll
      for (int k = 0; k < 4; ++k) gb[k] = (float)d[dbcol0 + 4 * c + k];
      for (int j = 0; j < n_novel; ++j) {
        int cn = novel[j];
        size_t so = ((size_t)r * n_novel + j) * n_base + sb;
        g += sim_cls[so] * (float)d[dccol0 + cn];
        float wb = sim_bbox[so];
#pragma unroll
        for (int k = 0; k < 4; ++k) gb[k] += wb * (float)d[dbcol0 + 4 * cn + k];
      }
    }
    TD* o = dlin + (size_t)r * ldl;
    o[ccol0 + c] = (TD)g;
    if (c < K) {
#pragma unroll
      for (int k = 0; k < 4; ++k) o[bcol0 + 4 * c + k] = (TD)gb[k];
    }
  } else if (idx < n1 + n2) {
    int t = idx - n1;
    int r = t / (n_novel * n_base); int rem = t - r * n_novel * n_base; int j = rem / n_base, b = rem - j * n_base;
    const TD* d = dy + (size_t)r * ldd;
    const float* x = lin + (size_t)r * ld;
    int cn = novel[j], cb = base[b];
    float v = (float)d[dccol0 + cn] * x[ccol0 + cb];
#pragma unroll
    for (int k = 0; k < 4; ++k) v += (float)d[dbcol0 + 4 * cn + k] * x[bcol0 + 4 * cb + k];
    dsim[t] = v;
  }
}
extern "C" int unit_transfer_predictions_bwd(const void* dy, int dy_dtype, int ldd, int dccol0, int dbcol0, const float* lin, int ld,
                                             int ccol0, int bcol0, int K, const float* sim_cls, const float* sim_bbox, const int* base_dev,
                                             int n_base, const int* novel_dev, int n_novel, const int8_t* role_dev, const int* slot_dev,
                                             void* dlin, int ldl, float* dsim, int R, void* stream) {
  if (R == 0) return UNIT_OK;
  long n = (long)R * (K + 1) + (long)R * n_novel * n_base;
  hipStream_t st = (hipStream_t)stream;
  (void)hipMemsetAsync(dlin, 0, (size_t)R * ldl * (dy_dtype == UNIT_BF16 ? 2 : 4), st);
  if (dy_dtype == UNIT_BF16)
    transfer_bwd_kernel<bf16_t><<<cdiv(n, 256), 256, 0, st>>>((const bf16_t*)dy, ldd, dccol0, dbcol0, lin, ld, ccol0, bcol0, K, sim_cls, sim_bbox,
                                                            base_dev, n_base, novel_dev, n_novel, role_dev, slot_dev, (bf16_t*)dlin, ldl, dsim, R);
  else
    transfer_bwd_kernel<float><<<cdiv(n, 256), 256, 0, st>>>((const float*)dy, ldd, dccol0, dbcol0, lin, ld, ccol0, bcol0, K, sim_cls, sim_bbox,
                                                          base_dev, n_base, novel_dev, n_novel, role_dev, slot_dev, (float*)dlin, ldl, dsim, R);
  UNIT_LAUNCH_CHECK();
  return UNIT_OK;
}

// Backward of similarity_kernel: dsim [R][n_novel][n_base] -> d(mean OICR logits) -> the n_oicr logit groups of `dlin` (each gets
// 1 / n_oicr of it; the predictors' weights are frozen in every fine-tune yaml, the gradient continues into their input).
//   S = u / T, u[j,b] = w L[j,b] + w v_b, T_j = max(sum_b u, 1e-9);  v_b = v'_b (>= thr) | 0,  v' = q[base] / max(sum q[base], 1e-9),
//   q = softmax(p).   (the in-place zeroing of roi_heads.py:257 passes no gradient to the zeroed entries)
template <typename TD>
__global__ void similarity_bwd_kernel(const float* __restrict__ lin, int ld, int col0, int n_oicr, int ncls, const int* __restrict__ base,
                                      int n_base, const float* __restrict__ lingual, int n_novel, float thr, int use_lingual,
                                      int use_visual, const float* __restrict__ dsim, TD* __restrict__ dlin, int ldl, int dcol0, int R) {
  int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R || !use_visual) return;
  float vis[DET_MAXC], vraw[DET_MAXC], dv[DET_MAXC];
  const float* x = lin + (size_t)r * ld + col0;
  float mx = -INFINITY;
  for (int c = 0; c < ncls; ++c) {
    float s = 0.f;
    for (int k = 0; k < n_oicr; ++k) s += x[k * ncls + c];
    mx = fmaxf(mx, s / (float)n_oicr);
  }
  float se = 0.f;
  for (int c = 0; c < ncls; ++c) {
    float s = 0.f;
    for (int k = 0; k < n_oicr; ++k) s += x[k * ncls + c];
    se += expf(s / (float)n_oicr - mx);
  }
  float tot = 0.f;
  for (int b = 0; b < n_base; ++b) {
    int c = base[b];
    float s = 0.f;
    for (int k = 0; k < n_oicr; ++k) s += x[k * ncls + c];
    vraw[b] = expf(s / (float)n_oicr - mx) / se;          // q[base_b]
    tot += vraw[b];
  }
  float totc = fmaxf(tot, 1e-9f);
  for (int b = 0; b < n_base; ++b) { float v = vraw[b] / totc; vis[b] = v < thr ? 0.f : v; dv[b] = 0.f; }
  float nterms = (float)(use_lingual + use_visual);
  float wgt = 1.0f / nterms;
  for (int j = 0; j < n_novel; ++j) {
    float lmx = -INFINITY, lse = 0.f;
    if (use_lingual) {
      for (int b = 0; b < n_base; ++b) lmx = fmaxf(lmx, lingual[j * n_base + b]);
      for (int b = 0; b < n_base; ++b) lse += expf(lingual[j * n_base + b] - lmx);
    }
    float T = 0.f;
    for (int b = 0; b < n_base; ++b) {
      float u = use_lingual ? wgt * (expf(lingual[j * n_base + b] - lmx) / lse) : 0.f;
      T += u + wgt * vis[b];
    }
    float Tc = fmaxf(T, 1e-9f);
    const float* g = dsim + ((size_t)r * n_novel + j) * n_base;
    float dot = 0.f;                                      // sum_b G[j,b] S[j,b]
    if (T >= 1e-9f) {
      for (int b = 0; b < n_base; ++b) {
        float u = (use_lingual ? wgt * (expf(lingual[j * n_base + b] - lmx) / lse) : 0.f) + wgt * vis[b];
        dot += g[b] * (u / Tc);
      }
    }
    for (int b = 0; b < n_base; ++b) dv[b] += wgt * (g[b] - dot) / Tc;       // d u[j,b] = (G - sum G S) / T  (T clamped: dot = 0)
  }
  // v_b = v'_b (kept) -> v'_b = w_b / tot
  float dot2 = 0.f;
  for (int b = 0; b < n_base; ++b) { if (vis[b] == 0.f) dv[b] = 0.f; }
  if (tot >= 1e-9f) for (int b = 0; b < n_base; ++b) dot2 += dv[b] * (vraw[b] / totc);
  // dq[c] for base columns, then dp = q (dq - sum q dq)
  float sq = 0.f;
  for (int b = 0; b < n_base; ++b) { dv[b] = (dv[b] - dot2) / totc; sq += vraw[b] * dv[b]; }     // dv now = dq[base_b]; sq = sum_c q_c dq_c
  TD* o = dlin + (size_t)r * ldl + dcol0;
  for (int c = 0; c < ncls; ++c) {
    float s = 0.f;
    for (int k = 0; k < n_oicr; ++k) s += x[k * ncls + c];
    float q = expf(s / (float)n_oicr - mx) / se;
    float dq = 0.f;
    for (int b = 0; b < n_base; ++b) if (base[b] == c) dq = dv[b];
    float dp = q * (dq - sq) / (float)n_oicr;
    for (int k = 0; k < n_oicr; ++k) o[k * ncls + c] = (TD)dp;
  }
}
extern "C" int unit_similarity_bwd(const float* lin_weak, int ld, int col0, int n_oicr, int ncls, const int* base_dev, int n_base,
                                   const float* lingual, int n_novel, float visual_threshold, int use_lingual, int use_visual,
                                   const float* dsim, void* dlin, int dlin_dtype, int ldl, int dcol0, int R, void* stream) {
  UNIT_CHECK_ARG(n_base <= DET_MAXC, "similarity_bwd: more than 96 base classes");
  if (R == 0) return UNIT_OK;
  hipStream_t st = (hipStream_t)stream;
  (void)hipMemsetAsync(dlin, 0, (size_t)R * ldl * (dlin_dtype == UNIT_BF16 ? 2 : 4), st);
  if (dlin_dtype == UNIT_BF16)
    similarity_bwd_kernel<bf16_t><<<cdiv(R, 64), 64, 0, st>>>(lin_weak, ld, col0, n_oicr, ncls, base_dev, n_base, lingual, n_novel, visual_threshold,
                                                            use_lingual, use_visual, dsim, (bf16_t*)dlin, ldl, dcol0, R);
  else
    similarity_bwd_kernel<float><<<cdiv(R, 64), 64, 0, st>>>(lin_weak, ld, col0, n_oicr, ncls, base_dev, n_base, lingual, n_novel, visual_threshold,
                                                           use_lingual, use_visual, dsim, (float*)dlin, ldl, dcol0, R);
  UNIT_LAUNCH_CHECK();
  return UNIT_OK;
}

// row softmax (predict_probs: F.softmax(scores, dim=-1)): the row's maximum and sum of exponentials, then one probability per column.
// unit_softmax_rows and unit_tta_accumulate share these two functions: the same operations in the same order, the same bits.
__device__ __forceinline__ void softmax_row_stats(const float* __restrict__ p, int ncls, float* mx_out, float* se_out) {
  float mx = -INFINITY;
  for (int c = 0; c < ncls; ++c) mx = fmaxf(mx, p[c]);
  float se = 0.f;
  for (int c = 0; c < ncls; ++c) se += expf(p[c] - mx);
  *mx_out = mx; *se_out = se;
}
__device__ __forceinline__ float softmax_row_prob(float x, float mx, float se) { return expf(x - mx) / se; }

__global__ void softmax_rows_kernel(const float* __restrict__ x, int ld, int ncls, float* __restrict__ y, int ldy, int R) {
  int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  const float* p = x + (size_t)r * ld;
  float mx, se;
  softmax_row_stats(p, ncls, &mx, &se);
  for (int c = 0; c < ncls; ++c) y[(size_t)r * ldy + c] = softmax_row_prob(p[c], mx, se);
}
extern "C" int unit_softmax_rows(const float* x, int ld, int ncls, float* y, int ldy, int R, void* stream) {
  if (R == 0) return UNIT_OK;
  softmax_rows_kernel<<<cdiv(R, 128), 128, 0, (hipStream_t)stream>>>(x, ld, ncls, y, ldy, R);
  UNIT_LAUNCH_CHECK();
  return UNIT_OK;
}

// ---- test-time augmentation, combining the views: WeaklySupervisedRCNNNoMeta.inference, meta_arch/rcnn.py:511-524 -------------------
//   cls_pred_scores = torch.stack(cls_pred_scores).sum(0)   (:516; each entry softmax(scores) of one view, fast_rcnn.py:456-458; NOT renormalised)
//   cls_pred_boxes  = torch.stack(cls_pred_boxes).mean(0)    (:524; the flipped views' dx are averaged as they are)
// One launch takes the predictions of n_in (1 or 2) consecutive views, v and v + 1, and adds them in view order: "=" for view 0, "+=" after it.
// With the last view delta_sum / n is written as delta_mean -- a division, as torch's mean is sum / n. The first R threads own one row of
// probs_sum each (the softmax is serial over the K + 1 columns, as in softmax_rows_kernel), the R * K after them one f32x4 of deltas each.
// Rows >= *count: zeros are written with view 0 (and to delta_mean with the last view), nothing is read. Latency-sized: a few hundred KB.
__global__ void __launch_bounds__(256) tta_accumulate_kernel(const float* __restrict__ scores, int lds_, int scol0, const float* __restrict__ deltas,
                                                             int ldd, long view_rows, int n_in, int K, int R, const int* __restrict__ count, int v,
                                                             int n, float* __restrict__ probs_sum, float* __restrict__ delta_sum,
                                                             float* __restrict__ delta_mean) {
  long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int ncls = K + 1;
  const int live = count ? min(max(*count, 0), R) : R;
  const bool last = v + n_in == n;
  if (idx < R) {
    const int r = (int)idx;
    float* o = probs_sum + (size_t)r * ncls;
    if (r >= live) {
      if (v == 0) for (int c = 0; c < ncls; ++c) o[c] = 0.f;
      return;
    }
    for (int j = 0; j < n_in; ++j) {
      const float* p = scores + ((size_t)j * view_rows + r) * lds_ + scol0;
      float mx, se;
      softmax_row_stats(p, ncls, &mx, &se);
      if (v + j == 0) for (int c = 0; c < ncls; ++c) o[c] = softmax_row_prob(p[c], mx, se);
      else for (int c = 0; c < ncls; ++c) o[c] = o[c] + softmax_row_prob(p[c], mx, se);
    }
    return;
  }
  idx -= R;
  if (idx >= (long)R * K) return;
  const int r = (int)(idx / K), k = (int)(idx - (long)r * K);
  f32x4* s = reinterpret_cast<f32x4*>(delta_sum + (size_t)r * 4 * K + 4 * k);
  f32x4* m = reinterpret_cast<f32x4*>(delta_mean + (size_t)r * 4 * K + 4 * k);
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  if (r >= live) {
    if (v == 0) *s = zero;
    if (last) *m = zero;
    return;
  }
  f32x4 acc = *reinterpret_cast<const f32x4*>(deltas + (size_t)r * ldd + 4 * k);
  if (v != 0) acc = *s + acc;
  if (n_in == 2) acc = acc + *reinterpret_cast<const f32x4*>(deltas + ((size_t)view_rows + r) * ldd + 4 * k);
  *s = acc;
  if (last) { const float d = (float)n; *m = f32x4{acc[0] / d, acc[1] / d, acc[2] / d, acc[3] / d}; }
}
extern "C" int unit_tta_accumulate(const float* scores, int lds, int scol0, const float* deltas, int ldd, long view_rows, int n_in, int K, int R,
                                   const int* count, int v, int n, float* probs_sum, float* delta_sum, float* delta_mean, void* stream) {
  UNIT_CHECK_ARG(K >= 1 && R >= 0 && (n_in == 1 || n_in == 2), "tta_accumulate: K >= 1, one or two views per launch");
  UNIT_CHECK_ARG(n >= 1 && v >= 0 && v + n_in <= n, "tta_accumulate: views v .. v + n_in - 1 of n");
  UNIT_CHECK_ARG(scol0 >= 0 && lds >= scol0 + K + 1 && ldd >= 4 * K && ldd % 4 == 0, "tta_accumulate: row strides (deltas: a multiple of 4 floats)");
  UNIT_CHECK_ARG(n_in == 1 || view_rows >= R, "tta_accumulate: the second view starts view_rows >= R rows behind the first");
  UNIT_CHECK_ARG(((uintptr_t)deltas | (uintptr_t)delta_sum | (uintptr_t)delta_mean) % 16 == 0, "tta_accumulate: 16-byte aligned delta buffers");
  UNIT_CHECK_ARG(delta_mean != delta_sum, "tta_accumulate: delta_mean needs a buffer of its own");
  if (R == 0) return UNIT_OK;
  long threads = (long)R + (long)R * K;
  tta_accumulate_kernel<<<cdiv(threads, 256L), 256, 0, (hipStream_t)stream>>>(scores, lds, scol0, deltas, ldd, view_rows, n_in, K, R, count, v, n,
                                                                            probs_sum, delta_sum, delta_mean);
  UNIT_LAUNCH_CHECK();
  return UNIT_OK;
}

// fast_rcnn_inference_single_image, first half: decode (weights w), drop non-finite RoIs, clip, score > thresh -> candidates in
// (roi, class) row-major order, compacted. One workgroup per image. Also returns max coordinate over the candidates (batched_nms offset).
// A RoI is dropped WHOLE when any of its K decoded boxes (before clipping) or any of its K+1 scores is non-finite (detectron2
// fast_rcnn_inference_single_image: `valid_mask = isfinite(boxes).all(1) & isfinite(scores).all(1)`). More than `cap`
// candidates: the first `cap` in (roi, class) order are kept.
__device__ __forceinline__ int2 det_scan2(int2 v, int2* total, int2* lds) {
  int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
  int2 inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    int ax = __shfl_up(inc.x, o, 64), ay = __shfl_up(inc.y, o, 64);
    if (lane >= o) { inc.x += ax; inc.y += ay; }
  }
  if (lane == 63) lds[wid] = inc;
  __syncthreads();
  if (threadIdx.x == 0) { int2 run = {0, 0}; for (int w = 0; w < nw; ++w) { int2 t = lds[w]; lds[w] = run; run.x += t.x; run.y += t.y; } lds[16] = run; }
  __syncthreads();
  int2 base = lds[wid];
  *total = lds[16];
  int2 ex = {base.x + inc.x - v.x, base.y + inc.y - v.y};
  __syncthreads();
  return ex;
}

// Box2BoxTransform.apply_deltas for one (RoI, class); torch.clamp(max=) keeps a NaN dw / dh, so must the comparison here (fminf would not)
__device__ __forceinline__ f32x4 det_decode(const float* __restrict__ dp, const float* __restrict__ pb, f32x4 w, float clampv) {
  float bw = pb[2] - pb[0], bh = pb[3] - pb[1];
  float cx = pb[0] + 0.5f * bw, cy = pb[1] + 0.5f * bh;
  float dx = dp[0] / w[0], dy = dp[1] / w[1];
  float dw = dp[2] / w[2], dh = dp[3] / w[3];
  dw = dw > clampv ? clampv : dw; dh = dh > clampv ? clampv : dh;
  float pcx = dx * bw + cx, pcy = dy * bh + cy;
  float pw = expf(dw) * bw, ph = expf(dh) * bh;
  return f32x4{pcx - 0.5f * pw, pcy - 0.5f * ph, pcx + 0.5f * pw, pcy + 0.5f * ph};
}

#define DET_MAX_RCAP (1 << 18)          // one validity bit per RoI in LDS: 32 KB

__global__ void det_select_kernel(const float* __restrict__ probs, int ldp, const float* __restrict__ deltas, int ldd,
                                  const float* __restrict__ props, const int* __restrict__ pcount, int Rcap, int K, f32x4 w,
                                  float clampv, const float* __restrict__ image_hw, float thresh, int cap, float* __restrict__ cboxes,
                                  float* __restrict__ cscores, int* __restrict__ cclass, int* __restrict__ croi, int* __restrict__ ccount,
                                  float* __restrict__ cmax) {
  extern __shared__ unsigned dropped[];          // [cdiv(Rcap, 32)] bit r: RoI r has a non-finite box or score
  __shared__ int2 lds[17];
  __shared__ float smax[16];
  int b = blockIdx.x;
  int R = min(pcount ? pcount[b] : Rcap, Rcap);
  float imh = image_hw[2 * b], imw = image_hw[2 * b + 1];
  int total = R * K;
  for (int i = threadIdx.x; i < (R + 31) / 32; i += blockDim.x) dropped[i] = 0u;
  __syncthreads();
  // validity of every RoI: all K boxes before clipping, all K+1 scores (the thread of class 0 also looks at the background score)
  for (int i = threadIdx.x; i < total; i += blockDim.x) {
    int r = i / K, k = i - r * K;
    size_t row = (size_t)b * Rcap + r;
    float sc = probs[row * ldp + k];
    f32x4 bx = det_decode(deltas + row * ldd + 4 * k, props + row * 4, w, clampv);
    bool fin = isfinite(bx[0]) && isfinite(bx[1]) && isfinite(bx[2]) && isfinite(bx[3]) && isfinite(sc);
    if (k == 0) fin = fin && isfinite(probs[row * ldp + K]);
    if (!fin) atomicOr(&dropped[r >> 5], 1u << (r & 31));
  }
  __syncthreads();
  int chunk = (total + blockDim.x - 1) / blockDim.x;
  int i0 = threadIdx.x * chunk, i1 = min(total, i0 + chunk);
  int2 c = {0, 0};
  float mx = -INFINITY;
  for (int pass = 0; pass < 2; ++pass) {
    int2 ex = {0, 0}, tot = {0, 0};
    if (pass == 1) ex = det_scan2(c, &tot, lds);
    for (int i = i0; i < i1; ++i) {
      int r = i / K, k = i - r * K;
      size_t row = (size_t)b * Rcap + r;
      float sc = probs[row * ldp + k];
      bool keep = !((dropped[r >> 5] >> (r & 31)) & 1u) && sc > thresh;
      if (pass == 0) { c.x += keep ? 1 : 0; }
      else if (keep) {
        if (ex.x < cap) {
          f32x4 bx = det_decode(deltas + row * ldd + 4 * k, props + row * 4, w, clampv);
          bx[0] = fminf(fmaxf(bx[0], 0.f), imw); bx[1] = fminf(fmaxf(bx[1], 0.f), imh);
          bx[2] = fminf(fmaxf(bx[2], 0.f), imw); bx[3] = fminf(fmaxf(bx[3], 0.f), imh);
          size_t o = (size_t)b * cap + ex.x;
          *reinterpret_cast<f32x4*>(cboxes + 4 * o) = bx;
          cscores[o] = sc; cclass[o] = k; croi[o] = r;
          mx = fmaxf(mx, fmaxf(fmaxf(bx[0], bx[1]), fmaxf(bx[2], bx[3])));
        }
        ex.x++;
      }
    }
    if (pass == 1 && threadIdx.x == 0) ccount[b] = min(tot.x, cap);
  }
  mx = wave_reduce_max(mx);
  if ((threadIdx.x & 63) == 0) smax[threadIdx.x >> 6] = mx;
  __syncthreads();
  if (threadIdx.x == 0) { float m = -INFINITY; for (int w2 = 0; w2 < (int)(blockDim.x >> 6); ++w2) m = fmaxf(m, smax[w2]); cmax[b] = m; }
}
extern "C" int unit_detection_candidates(const float* probs, int ldp, const float* deltas, int ldd, const float* props, const int* pcount,
                                         int B, int Rcap, int K, const float* weights4, float scale_clamp, const float* image_hw_dev,
                                         float score_thresh, int cap, float* cand_boxes, float* cand_scores, int* cand_class, int* cand_roi,
                                         int* cand_count, float* cand_max, void* stream) {
  UNIT_CHECK_ARG(Rcap >= 0 && Rcap <= DET_MAX_RCAP, "detection_candidates: at most 262144 RoIs per image");
  if (B == 0) return UNIT_OK;
  f32x4 w = {weights4[0], weights4[1], weights4[2], weights4[3]};
  size_t lds_bytes = (size_t)cdiv(Rcap, 32) * sizeof(unsigned);
  det_select_kernel<<<B, 1024, lds_bytes, (hipStream_t)stream>>>(probs, ldp, deltas, ldd, props, pcount, Rcap, K, w, scale_clamp, image_hw_dev,
                                                                score_thresh, cap, cand_boxes, cand_scores, cand_class, cand_roi, cand_count, cand_max);
  UNIT_LAUNCH_CHECK();
  return UNIT_OK;
}

// batched_nms helper: gather candidates into score order and add class * (max_coordinate + 1) to all four coordinates
__global__ void det_offset_gather_kernel(const float* __restrict__ cboxes, const int* __restrict__ cclass, const int* __restrict__ order,
                                         const int* __restrict__ ccount, const float* __restrict__ cmax, int cap, float* __restrict__ out) {
  int b = blockIdx.y;
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= cap) return;
  f32x4 v = {0, 0, 0, 0};
  if (i < ccount[b]) {
    int src = order[(size_t)b * cap + i];
    v = *reinterpret_cast<const f32x4*>(cboxes + ((size_t)b * cap + src) * 4);
    float off = (float)cclass[(size_t)b * cap + src] * (cmax[b] + 1.0f);
    v[0] += off; v[1] += off; v[2] += off; v[3] += off;
  }
  *reinterpret_cast<f32x4*>(out + ((size_t)b * cap + i) * 4) = v;
}
extern "C" int unit_detection_offset_gather(const float* cand_boxes, const int* cand_class, const int* order, const int* cand_count,
                                            const float* cand_max, int B, int cap, float* out, void* stream) {
  if (B == 0 || cap == 0) return UNIT_OK;
  det_offset_gather_kernel<<<dim3(cdiv(cap, 256), B), 256, 0, (hipStream_t)stream>>>(cand_boxes, cand_class, order, cand_count, cand_max, cap, out);
  UNIT_LAUNCH_CHECK();
  return UNIT_OK;
}

// final gather: keep[j] indexes the score-sorted list; emit boxes (un-offset), scores, classes, roi indices
__global__ void det_final_kernel(const float* __restrict__ cboxes, const float* __restrict__ cscores, const int* __restrict__ cclass,
                                 const int* __restrict__ croi, const int* __restrict__ order, const int* __restrict__ keep,
                                 const int* __restrict__ keep_count, int cap, int topk, float* __restrict__ oboxes, float* __restrict__ oscores,
                                 int* __restrict__ oclass, int* __restrict__ oroi, int* __restrict__ ocount) {
  int b = blockIdx.x;
  int n = min(keep_count[b], topk);
  for (int j = threadIdx.x; j < topk; j += blockDim.x) {
    size_t o = (size_t)b * topk + j;
    if (j < n) {
      int src = order[(size_t)b * cap + keep[(size_t)b * topk + j]];
      size_t s = (size_t)b * cap + src;
      *reinterpret_cast<f32x4*>(oboxes + 4 * o) = *reinterpret_cast<const f32x4*>(cboxes + 4 * s);
      oscores[o] = cscores[s]; oclass[o] = cclass[s]; oroi[o] = croi[s];
    } else {
      *reinterpret_cast<f32x4*>(oboxes + 4 * o) = f32x4{0, 0, 0, 0};
      oscores[o] = 0.f; oclass[o] = -1; oroi[o] = -1;
    }
  }
  if (threadIdx.x == 0) ocount[b] = n;
}
extern "C" int unit_detection_finalize(const float* cand_boxes, const float* cand_scores, const int* cand_class, const int* cand_roi,
                                       const int* order, const int* keep, const int* keep_count, int B, int cap, int topk,
                                       float* out_boxes, float* out_scores, int* out_class, int* out_roi, int* out_count, void* stream) {
  if (B == 0) return UNIT_OK;
  det_final_kernel<<<B, 128, 0, (hipStream_t)stream>>>(cand_boxes, cand_scores, cand_class, cand_roi, order, keep, keep_count, cap, topk,
                                                      out_boxes, out_scores, out_class, out_roi, out_count);
  UNIT_LAUNCH_CHECK();
  return UNIT_OK;
}

// ---- class-segmented NMS stage: the K independent per-class problems instead of one all-pairs problem over the shifted list ----------
// Boxes of different classes never overlap after the batched_nms shift and a class holds at most one candidate per RoI, so the score-sorted
// list is regrouped by class (a stable counting sort on the class id, chip-wide: 256 sorted positions per workgroup), unit_nms runs on the
// B * K segments of capacity Rseg, and the K keep lists of an image are merged back by global position.
//  (1) det_seg_hist_kernel: class histogram of every 256-position tile -> hist [B][nblk][K]
//  (2) det_seg_scan_kernel: per (image, class) the exclusive prefix over the tiles (in place) and the segment counts
//  (3) det_seg_scatter_kernel: slot = tile base + the number of earlier positions of the tile with the same class (stable), writes the
//      shifted box, the score and the global position
#define DET_SEG_TILE 256
#define DET_SORT_MAX_KEYS (1 << 20)          // unit_sort_desc_stable refuses more keys (1024 * SORT_THREADS, sort_nms.hip)
extern "C" int unit_nms_max_candidates(void);          // sort_nms.hip: the capacity of one unit_nms problem, here of one class

__device__ __forceinline__ int det_seg_class(const int* __restrict__ cclass, const int* __restrict__ order, int b, int i, int n, int cap, int K,
                                             int* src_out) {
  if (i >= n) return -1;
  int src = order[(size_t)b * cap + i];
  if ((unsigned)src >= (unsigned)cap) return -1;
  int c = cclass[(size_t)b * cap + src];
  *src_out = src;
  return (unsigned)c < (unsigned)K ? c : -1;
}

__global__ void __launch_bounds__(DET_SEG_TILE) det_seg_hist_kernel(const int* __restrict__ cclass, const int* __restrict__ order,
                                                                    const int* __restrict__ ccount, int cap, int K, int nblk,
                                                                    int* __restrict__ hist) {
  __shared__ int h[DET_MAXC];
  int b = blockIdx.y, blk = blockIdx.x, tid = threadIdx.x;
  if (tid < K) h[tid] = 0;
  __syncthreads();
  int n = min(ccount[b], cap), src;
  int c = det_seg_class(cclass, order, b, blk * DET_SEG_TILE + tid, n, cap, K, &src);
  if (c >= 0) atomicAdd(&h[c], 1);
  __syncthreads();
  if (tid < K) hist[((size_t)b * nblk + blk) * K + tid] = h[tid];
}

__global__ void __launch_bounds__(128) det_seg_scan_kernel(int* __restrict__ hist, int K, int nblk, int Rseg, int* __restrict__ seg_count) {
  int b = blockIdx.x, k = threadIdx.x;
  if (k >= K) return;
  int* hb = hist + (size_t)b * nblk * K + k;
  int run = 0;
#pragma unroll 8
  for (int blk = 0; blk < nblk; ++blk) { int t = hb[(size_t)blk * K]; hb[(size_t)blk * K] = run; run += t; }
  seg_count[b * K + k] = min(run, Rseg);
}

__global__ void __launch_bounds__(DET_SEG_TILE) det_seg_scatter_kernel(const float* __restrict__ cboxes, const float* __restrict__ cscores,
                                                                       const int* __restrict__ cclass, const int* __restrict__ order,
                                                                       const int* __restrict__ ccount, const float* __restrict__ cmax, int cap,
                                                                       int K, int nblk, int Rseg, const int* __restrict__ hist,
                                                                       float* __restrict__ seg_boxes, float* __restrict__ seg_scores,
                                                                       int* __restrict__ seg_pos) {
  __shared__ int cls[DET_SEG_TILE];
  int b = blockIdx.y, blk = blockIdx.x, tid = threadIdx.x;
  int n = min(ccount[b], cap), src = 0;
  int i = blk * DET_SEG_TILE + tid;
  int c = det_seg_class(cclass, order, b, i, n, cap, K, &src);
  cls[tid] = c;
  __syncthreads();
  if (c < 0) return;
  int rank = 0;
  for (int j = 0; j < tid; ++j) rank += cls[j] == c ? 1 : 0;
  int slot = hist[((size_t)b * nblk + blk) * K + c] + rank;
  if (slot >= Rseg) return;          // (a class with more than Rseg candidates: more than one per RoI, not produced by unit_detection_candidates)
  f32x4 v = *reinterpret_cast<const f32x4*>(cboxes + ((size_t)b * cap + src) * 4);
  float off = (float)c * (cmax[b] + 1.0f);          // det_offset_gather_kernel's shift, the same float operations
  v[0] += off; v[1] += off; v[2] += off; v[3] += off;
  size_t o = ((size_t)b * K + c) * Rseg + slot;
  *reinterpret_cast<f32x4*>(seg_boxes + 4 * o) = v;
  seg_scores[o] = cscores[(size_t)b * cap + src];
  seg_pos[o] = i;
}

extern "C" int unit_detection_max_candidates(void) {
  long lim = (long)DET_MAX_RCAP * DET_MAXC;          // the candidate kernel: DET_MAX_RCAP RoIs of at most DET_MAXC classes
  if (lim > DET_SORT_MAX_KEYS) lim = DET_SORT_MAX_KEYS;          // the sorter
  if (lim > 0x7fffffffL / 4) lim = 0x7fffffffL / 4;          // int positions, 4 coordinates per candidate (the per-image offsets are size_t)
  return (int)lim;
}
// every bound of the segmented form, without a launch (ops.detections asks before it starts the chain)
extern "C" int unit_detection_segments_check(int B, int cap, int K, int Rseg) {
  UNIT_CHECK_ARG(B >= 0 && K >= 1 && K <= DET_MAXC, "detection_class_segments: 1 to 96 classes");
  UNIT_CHECK_ARG(cap >= 1 && cap <= unit_detection_max_candidates(), "detection_class_segments: more than 1048576 candidates per image");
  UNIT_CHECK_ARG(Rseg >= 1 && Rseg <= cap, "detection_class_segments: the segment capacity must lie in 1 .. cap");
  UNIT_CHECK_ARG(Rseg <= unit_nms_max_candidates(), "detection_class_segments: more than 65536 candidates per class (unit_nms)");
  UNIT_CHECK_ARG((long)B * K <= 65535, "detection_class_segments: more than 65535 (image, class) segments");
  return UNIT_OK;
}
extern "C" size_t unit_detection_segments_workspace_bytes(int B, int cap, int K) {
  return (size_t)B * cdiv(cap > 0 ? cap : 1, DET_SEG_TILE) * K * sizeof(int);
}
extern "C" int unit_detection_class_segments(const float* cand_boxes, const float* cand_scores, const int* cand_class, const int* order,
                                             const int* cand_count, const float* cand_max, int B, int cap, int K, int Rseg, float* seg_boxes,
                                             float* seg_scores, int* seg_count, int* seg_pos, void* workspace, size_t workspace_bytes,
                                             void* stream) {
  int rc = unit_detection_segments_check(B, cap, K, Rseg);
  if (rc != UNIT_OK) return rc;
  if (workspace_bytes < unit_detection_segments_workspace_bytes(B, cap, K)) { unit_set_error("detection_class_segments: workspace too small"); return UNIT_ERR_WORKSPACE; }
  if (B == 0) return UNIT_OK;
  hipStream_t st = (hipStream_t)stream;
  int nblk = cdiv(cap, DET_SEG_TILE);
  int* hist = (int*)workspace;
  det_seg_hist_kernel<<<dim3(nblk, B), DET_SEG_TILE, 0, st>>>(cand_class, order, cand_count, cap, K, nblk, hist);
  UNIT_LAUNCH_CHECK();
  det_seg_scan_kernel<<<B, 128, 0, st>>>(hist, K, nblk, Rseg, seg_count);
  UNIT_LAUNCH_CHECK();
  det_seg_scatter_kernel<<<dim3(nblk, B), DET_SEG_TILE, 0, st>>>(cand_boxes, cand_scores, cand_class, order, cand_count, cand_max, cap, K, nblk,
                                                                Rseg, hist, seg_boxes, seg_scores, seg_pos);
  UNIT_LAUNCH_CHECK();
  return UNIT_OK;
}

// merge of the K per-class keep lists of an image (each ascending in global position) into the first topk of their union, ascending: an
// element's output rank is the number of kept positions below it over all K lists (positions are unique), found by binary search -- no LDS,
// no atomics. det_keep_pos_kernel first turns the in-segment keep indices into global positions (INT_MAX behind a list's count).
__global__ void __launch_bounds__(256) det_keep_pos_kernel(const int* __restrict__ seg_keep, const int* __restrict__ seg_keep_count,
                                                           const int* __restrict__ seg_pos, int K, int Rseg, int topk, int* __restrict__ keep_pos,
                                                           int* __restrict__ keep_count) {
  int b = blockIdx.z, k = blockIdx.y, j = blockIdx.x * blockDim.x + threadIdx.x;
  size_t s = (size_t)b * K + k;
  if (j < topk) {
    int idx = j < min(seg_keep_count[s], topk) ? seg_keep[s * topk + j] : -1;
    keep_pos[s * topk + j] = (unsigned)idx < (unsigned)Rseg ? seg_pos[s * Rseg + idx] : 0x7fffffff;
  }
  if (k == 0 && j == 0) {
    long total = 0;
    for (int q = 0; q < K; ++q) total += min(seg_keep_count[(size_t)b * K + q], topk);
    keep_count[b] = (int)(total < topk ? total : topk);
  }
}

__global__ void __launch_bounds__(256) det_merge_keep_kernel(const int* __restrict__ keep_pos, const int* __restrict__ keep_count, int K, int topk,
                                                             int cap, int* __restrict__ keep) {
  int b = blockIdx.z, k = blockIdx.y, j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= topk) return;
  if (k == 0 && j >= keep_count[b]) keep[(size_t)b * topk + j] = -1;          // the tail behind the kept prefix
  const int* kp = keep_pos + (size_t)b * K * topk;
  int p = kp[(size_t)k * topk + j];
  if ((unsigned)p >= (unsigned)cap) return;          // behind this list's count
  int rank = j;                                      // its own list
  for (int q = 0; q < K && rank < topk; ++q) {
    if (q == k) continue;
    const int* lq = kp + (size_t)q * topk;
    int lo = 0, hi = topk;                           // first entry >= p (INT_MAX pads the list)
    while (lo < hi) { int mid = (lo + hi) >> 1; if (lq[mid] < p) lo = mid + 1; else hi = mid; }
    rank += lo;
  }
  if (rank < topk) keep[(size_t)b * topk + rank] = p;
}

extern "C" int unit_detection_merge_keep(const int* seg_keep, const int* seg_keep_count, const int* seg_pos, int B, int K, int Rseg, int cap,
                                         int topk, int* keep_pos, int* keep, int* keep_count, void* stream) {
  UNIT_CHECK_ARG(B >= 0 && K >= 1 && K <= DET_MAXC, "detection_merge_keep: 1 to 96 classes");
  UNIT_CHECK_ARG(topk >= 1 && Rseg >= 1 && cap >= Rseg, "detection_merge_keep: topk and the segment capacity must be positive, cap >= Rseg");
  UNIT_CHECK_ARG(B <= 65535, "detection_merge_keep: more than 65535 images");
  if (B == 0) return UNIT_OK;
  hipStream_t st = (hipStream_t)stream;
  dim3 grid(cdiv(topk, 256), K, B);
  det_keep_pos_kernel<<<grid, 256, 0, st>>>(seg_keep, seg_keep_count, seg_pos, K, Rseg, topk, keep_pos, keep_count);
  UNIT_LAUNCH_CHECK();
  det_merge_keep_kernel<<<grid, 256, 0, st>>>(keep_pos, keep_count, K, topk, cap, keep);
  UNIT_LAUNCH_CHECK();
  return UNIT_OK;
}

// detector_postprocess (rcnn.py:411-429 -> detectron2): scale to the output resolution, clip, flag non-empty
__global__ void postprocess_kernel(float* __restrict__ boxes, const int* __restrict__ count, int topk, const float* __restrict__ scale_xy,
                                   const float* __restrict__ out_hw, unsigned char* __restrict__ nonempty) {
  int b = blockIdx.x;
  for (int j = threadIdx.x; j < topk; j += blockDim.x) {
    size_t o = (size_t)b * topk + j;
    f32x4 v = *reinterpret_cast<f32x4*>(boxes + 4 * o);
    float sx = scale_xy[2 * b], sy = scale_xy[2 * b + 1], oh = out_hw[2 * b], ow = out_hw[2 * b + 1];
    v[0] = fminf(fmaxf(v[0] * sx, 0.f), ow); v[2] = fminf(fmaxf(v[2] * sx, 0.f), ow);
    v[1] = fminf(fmaxf(v[1] * sy, 0.f), oh); v[3] = fminf(fmaxf(v[3] * sy, 0.f), oh);
    *reinterpret_cast<f32x4*>(boxes + 4 * o) = v;
    nonempty[o] = (j < count[b] && (v[2] - v[0]) > 0.f && (v[3] - v[1]) > 0.f) ? 1 : 0;
  }
}
extern "C" int unit_detector_postprocess(float* boxes, const int* count, int B, int topk, const float* scale_xy_dev, const float* out_hw_dev,
                                         unsigned char* nonempty, void* stream) {
  if (B == 0) return UNIT_OK;
  postprocess_kernel<<<B, 128, 0, (hipStream_t)stream>>>(boxes, count, topk, scale_xy_dev, out_hw_dev, nonempty);
  UNIT_LAUNCH_CHECK();
  return UNIT_OK;
}

// ---- output assembly without stock operators (modeling/inference.py) ---------------------------------------------------------------
// Stable compaction of the kept detections of every image (keep = j < count[b] [&& nonempty[b][j]]): rows of boxes / scores / classes
// (as int64, the reference's pred_classes dtype) / RoI indices / mask probabilities move to the front of their image's block, out_count[b]
// = rows kept. One workgroup per image; topk <= 1024. The reference does this with boolean-mask indexing per image and field
// (detectron2 detector_postprocess via meta_arch/rcnn.py:411-429): ~6 launches and a host sync per image.
__global__ void __launch_bounds__(256) compact_detections_kernel(const float* __restrict__ boxes, const float* __restrict__ scores, const int* __restrict__ cls,
                                                                 const int* __restrict__ roi, const float* __restrict__ masks, int mask_elems,
                                                                 const int* __restrict__ count, const unsigned char* __restrict__ nonempty, int topk,
                                                                 float* __restrict__ oboxes, float* __restrict__ oscores, long* __restrict__ ocls,
                                                                 int* __restrict__ oroi, float* __restrict__ omasks, int* __restrict__ out_count) {
  __shared__ int pos[1024];
  __shared__ int total;
  const int b = blockIdx.x, c = min(count[b], topk);
  if (threadIdx.x == 0) {          // serial prefix over <= 1024 flags: a few hundred cycles, once per image
    int n = 0;
    for (int j = 0; j < topk; ++j) {
      bool keep = j < c && (nonempty == nullptr || nonempty[(size_t)b * topk + j]);
      pos[j] = keep ? n++ : -1;
    }
    total = n;
    out_count[b] = n;
  }
  __syncthreads();
  for (int j = threadIdx.x; j < topk; j += blockDim.x) {
    int d = pos[j];
    if (d < 0) continue;
    size_t s = (size_t)b * topk + j, o = (size_t)b * topk + d;
    *reinterpret_cast<f32x4*>(oboxes + 4 * o) = *reinterpret_cast<const f32x4*>(boxes + 4 * s);
    oscores[o] = scores[s]; ocls[o] = (long)cls[s]; oroi[o] = roi[s];
  }
  if (masks != nullptr) {
    for (int j = 0; j < topk; ++j) {
      int d = pos[j];
      if (d < 0) continue;
      const float* src = masks + ((size_t)b * topk + j) * mask_elems;
      float* dst = omasks + ((size_t)b * topk + d) * mask_elems;
      for (int e = threadIdx.x; e < mask_elems; e += blockDim.x) dst[e] = src[e];
    }
  }
}
extern "C" int unit_compact_detections(const float* boxes, const float* scores, const int* cls, const int* roi, const float* masks, int mask_elems,
                                       const int* count, const unsigned char* nonempty, int B, int topk, float* oboxes, float* oscores,
                                       long* ocls, int* oroi, float* omasks, int* out_count, void* stream) {
  UNIT_CHECK_ARG(topk >= 0 && topk <= 1024, "compact_detections: topk <= 1024");
  UNIT_CHECK_ARG(masks == nullptr || (omasks != nullptr && omasks != masks), "compact_detections: masks need a separate output");
  if (B == 0) return UNIT_OK;
  compact_detections_kernel<<<B, 256, 0, (hipStream_t)stream>>>(boxes, scores, cls, roi, masks, mask_elems, count, nonempty, topk, oboxes, oscores, ocls,
                                                                oroi, omasks, out_count);
  UNIT_LAUNCH_CHECK();
  return UNIT_OK;
}

// ---- pseudo ground truth of the weak images: WeaklySupervisedRCNNRPN.forward, meta_arch/rcnn.py:594-599 ---------------------------
// The eval-mode detections of a weak image whose class is one of the image's labels (`labels_mask`, :594-595) and whose score is
// strictly above WEAK_RPN_SCORE_TRESHOLD (`score_mask`, :596-597; a NaN score compares false and drops the row) become the image's
// ground-truth boxes (:598), in detection order: the matcher's ties go to the first box. One workgroup per image, the kept rows of each
// 256-row chunk ranked by ballot + popcount within a wave and a four-entry prefix over the waves: no atomics, the order is the input's.
// Rows past gt_count[b] are zero boxes / index -1. T <= 1024; gt_boxes must not alias boxes.
__global__ void __launch_bounds__(256) pseudo_gt_kernel(const float* __restrict__ boxes, const float* __restrict__ scores, const int* __restrict__ cls,
                                                        const int* __restrict__ count, const unsigned char* __restrict__ multihot, int K,
                                                        float threshold, int T, float* __restrict__ gt_boxes, int* __restrict__ gt_count,
                                                        int* __restrict__ kept_idx) {
  __shared__ int wcnt[4];
  const int b = blockIdx.x, lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int c = min(max(count[b], 0), T);
  int base = 0;
  for (int j0 = 0; j0 < c; j0 += 256) {          // (c is the same for the whole workgroup: every thread reaches both barriers)
    const int j = j0 + threadIdx.x;
    const size_t s = (size_t)b * T + j;
    bool keep = false;
    if (j < c) {
      int k = cls[s];
      keep = k >= 0 && k < K && multihot[(size_t)b * K + k] != 0 && scores[s] > threshold;
    }
    const unsigned long long bal = __ballot(keep);
    if (lane == 0) wcnt[wid] = __popcll(bal);
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) { int n = wcnt[w]; before += w < wid ? n : 0; all += n; }
    if (keep) {
      const size_t o = (size_t)b * T + base + before + __popcll(bal & ((1ull << lane) - 1ull));
      *reinterpret_cast<f32x4*>(gt_boxes + 4 * o) = *reinterpret_cast<const f32x4*>(boxes + 4 * s);
      kept_idx[o] = j;
    }
    base += all;
    __syncthreads();          // wcnt is rewritten by the next chunk
  }
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  for (int j = base + threadIdx.x; j < T; j += blockDim.x) {
    const size_t o = (size_t)b * T + j;
    *reinterpret_cast<f32x4*>(gt_boxes + 4 * o) = zero;
    kept_idx[o] = -1;
  }
  if (threadIdx.x == 0) gt_count[b] = base;
}
extern "C" int unit_pseudo_gt(const float* boxes, const float* scores, const int* cls, const int* count, const unsigned char* multihot,
                              int B, int T, int K, float threshold, float* gt_boxes, int* gt_count, int* kept_idx, void* stream) {
  UNIT_CHECK_ARG(T >= 0 && T <= 1024, "pseudo_gt: T <= 1024");
  UNIT_CHECK_ARG(K >= 1, "pseudo_gt: K >= 1");
  UNIT_CHECK_ARG(gt_boxes != boxes, "pseudo_gt: gt_boxes needs a buffer of its own");
  if (B == 0) return UNIT_OK;
  pseudo_gt_kernel<<<B, 256, 0, (hipStream_t)stream>>>(boxes, scores, cls, count, multihot, K, threshold, T, gt_boxes, gt_count, kept_idx);
  UNIT_LAUNCH_CHECK();
  return UNIT_OK;
}

// A weak image without pseudo ground truth contributes 0 to the weak RPN losses (rcnn.py:607-609: the proposal generator is not called for
// it): its sampled anchor labels -- all background, the matcher's answer to zero boxes -- become -1 (ignored) before the batched loss launch.
__global__ void gate_anchor_labels_kernel(signed char* __restrict__ labels, const int* __restrict__ gt_count, int Ncap) {
  const int b = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < Ncap && gt_count[b] <= 0) labels[(size_t)b * Ncap + i] = -1;
}
extern "C" int unit_gate_anchor_labels(signed char* labels, const int* gt_count, int B, int Ncap, void* stream) {
  if (B == 0 || Ncap == 0) return UNIT_OK;
  gate_anchor_labels_kernel<<<dim3(cdiv(Ncap, 256), B), 256, 0, (hipStream_t)stream>>>(labels, gt_count, Ncap);
  UNIT_LAUNCH_CHECK();
  return UNIT_OK;
}

// boxes [B][T][4] -> RoIAlign rows [B*T][5] = (image index, x0, y0, x1, y1)
__global__ void boxes_to_rois5_kernel(const float* __restrict__ boxes, int T, long n, float* __restrict__ rois5) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  f32x4 v = *reinterpret_cast<const f32x4*>(boxes + 4 * i);
  float* o = rois5 + 5 * i;
  o[0] = (float)(i / T); o[1] = v[0]; o[2] = v[1]; o[3] = v[2]; o[4] = v[3];
}
extern "C" int unit_boxes_to_rois5(const float* boxes, int B, int T, float* rois5, void* stream) {
  long n = (long)B * T;
  if (n == 0) return UNIT_OK;
  boxes_to_rois5_kernel<<<(unsigned)cdiv(n, 256L), 256, 0, (hipStream_t)stream>>>(boxes, T, n, rois5);
  UNIT_LAUNCH_CHECK();
  return UNIT_OK;
}

// out[b * T + j][:] = src[b * rcap + max(idx[b][j], 0)][:]   (rows of `row_bytes` bytes, a multiple of 4): similarity['seg'][filter_inds]
// of roi_heads.py:768-771, and any other per-image row gather
__global__ void gather_rows_kernel(const unsigned* __restrict__ src, const int* __restrict__ idx, int T, int rcap, int row_words, long n_rows,
                                   unsigned* __restrict__ out) {
  long r = blockIdx.x;
  if (r >= n_rows) return;
  long b = r / T;
  int k = idx[r];
  const unsigned* s = src + ((size_t)b * rcap + (k > 0 ? k : 0)) * row_words;
  unsigned* d = out + (size_t)r * row_words;
  for (int e = threadIdx.x; e < row_words; e += blockDim.x) d[e] = s[e];
}
extern "C" int unit_gather_rows(const void* src, const int* idx, int B, int T, int rcap, int row_bytes, void* out, void* stream) {
  UNIT_CHECK_ARG(row_bytes % 4 == 0, "gather_rows: rows of whole 32-bit words");
  long n = (long)B * T;
  if (n == 0 || row_bytes == 0) return UNIT_OK;
  UNIT_CHECK_ARG(n < 0x7FFFFFFFl, "gather_rows: too many rows");
  gather_rows_kernel<<<(unsigned)n, 128, 0, (hipStream_t)stream>>>((const unsigned*)src, idx, T, rcap, row_bytes / 4, n, (unsigned*)out);
  UNIT_LAUNCH_CHECK();
  return UNIT_OK;
}

// the first `take` rows of each of `nb` blocks of `block_rows` rows -> one dense [nb * take][row] tensor (rows of `row_bytes` bytes, a multiple
// of 4): the foreground RoI slots of every image for the mask head (roi_heads.py:691-710 select_foreground_proposals; the sampler emits
// [fg..., bg...] per image). Replaces one torch.cat of per-image slices per field.
__global__ void gather_blocks_kernel(const unsigned* __restrict__ src, int block_rows, int take, int row_words, unsigned* __restrict__ out) {
  long r = blockIdx.x;                      // output row
  long b = r / take, j = r - b * take;
  const unsigned* s = src + ((size_t)b * block_rows + j) * row_words;
  unsigned* d = out + (size_t)r * row_words;
  if ((row_words & 3) == 0) {
    for (int e = threadIdx.x; e < row_words / 4; e += blockDim.x) reinterpret_cast<u32x4*>(d)[e] = reinterpret_cast<const u32x4*>(s)[e];
  } else {
    for (int e = threadIdx.x; e < row_words; e += blockDim.x) d[e] = s[e];
  }
}
extern "C" int unit_gather_blocks(const void* src, int nb, int block_rows, int take, int row_bytes, void* out, void* stream) {
  UNIT_CHECK_ARG(row_bytes % 4 == 0 && take <= block_rows, "gather_blocks: rows of whole 32-bit words, take <= block_rows");
  UNIT_CHECK_ARG((row_bytes % 16 != 0) || (((uintptr_t)src % 16 == 0) && ((uintptr_t)out % 16 == 0)), "gather_blocks: 16B alignment");
  long n = (long)nb * take;
  if (n == 0 || row_bytes == 0) return UNIT_OK;
  gather_blocks_kernel<<<(unsigned)n, row_bytes >= 4096 ? 256 : 64, 0, (hipStream_t)stream>>>((const unsigned*)src, block_rows, take, row_bytes / 4, (unsigned*)out);
  UNIT_LAUNCH_CHECK();
  return UNIT_OK;
}
