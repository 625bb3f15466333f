// pcl.hip -- Proposal Cluster Learning (Tang et al., TPAMI 2018), the weak detector's TYPE "PCL" loss:
//   PCLFunction  modeling/roi_heads/pcl_loss.py:6-61, applied per image at weak_detector_fast_rcnn.py:233-238.
// Loss value and d(loss)/d(logits) of one OICR refinement stream in one launch, the fused-loss convention of losses.hip.
#include "common.h"

template <typename T> __device__ __forceinline__ void pcl_st(T* p, float v) { *p = (T)v; }

// fixed-order sum over the 256 threads of a workgroup
__device__ __forceinline__ float pcl_block_sum(float v, float* lds /* >= 5 */) {
  v = wave_reduce_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) lds[4] = (lds[0] + lds[1]) + (lds[2] + lds[3]);
  __syncthreads();
  return lds[4];
}

// ---------------------------------------------------------------------------------------------------
// PCL loss + logits gradient. Images in fixed slots of S rows (row b*S + i, valid[row] >= 0), clusters in slots of ldc
// (b*ldc + j, j < n_pc[b]). Per image, with p = softmax(logits[row, col0 : col0+K+1]) (unclamped) and N_b valid rows:
//   loss_b = -( sum_{rows, label == K} w_r log p_rK + sum_{j} icw_j log pc_probs_j ) / N_b
//   g[r, K]     = -w_r / p_rK / N_b                                           (label == K)
//   g[r, label] = -icw_j / (pc_count_j * pc_probs_j) / N_b,  j = gt_assign[r]  (label < K)
//   dy[r, :]    = gscale * p_r * (g_r - <g_r, p_r>)                            (softmax Jacobian)
//   *loss       = sum_b loss_b / B
// PCLFunction.backward never reads grad_output, so the reference's gradient is NOT divided by B (nor scaled by any loss weight):
// gscale = 1 reproduces it. A label < K row whose gt_assign is outside [0, n_pc) gets no gradient (the reference would index
// cluster -1; the Matcher's 0.5 equals FG_THRESHOLD in every shipped config, so it does not arise). Invalid rows get dy = 0.
// Layout: one wave per row (lane c and c + 64 hold columns c, c + 64 of the K+1 <= 96: coalesced, one expf per element); grid
// (blocks per image, images), 4 waves per workgroup striding over the image's rows. Every workgroup's partial
// -(its rows' terms [+ the cluster terms in the image's first workgroup]) / N_b is non-negative and enters the loss through the
// fixed-point accumulator of common.h (packed_sum_finish), so the loss is the same bit for bit whatever the arrival order; with
// acc == NULL one workgroup walks everything.
// ---------------------------------------------------------------------------------------------------
template <typename TD>
__global__ __launch_bounds__(256) void pcl_loss_kernel(const float* __restrict__ logits, int ld, int col0, int K,
                                                       const int* __restrict__ valid, int S, int B, const int* __restrict__ labels,
                                                       const float* __restrict__ cls_w, const int* __restrict__ gt_assign,
                                                       const int* __restrict__ pc_count, const float* __restrict__ pc_icw,
                                                       const float* __restrict__ pc_probs, const int* __restrict__ n_pc, int ldc,
                                                       float gscale, float* __restrict__ loss, TD* __restrict__ dy, int ldd, int dcol0,
                                                       unsigned long long* __restrict__ acc) {
  __shared__ float lds[5];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, ncol = K + 1;
  const int c0 = lane, c1 = lane + 64;
  float partial = 0.f;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    int nv = 0;
    for (int i = tid; i < S; i += blockDim.x) nv += valid[(size_t)b * S + i] >= 0 ? 1 : 0;
    const float nb = pcl_block_sum((float)nv, lds);
    const int npc = min(n_pc[b], ldc);
    float part = 0.f;                                  // lane 0 of every wave carries its rows' terms
    if (blockIdx.x == 0)
      for (int j = tid; j < npc; j += blockDim.x) {
        size_t q = (size_t)b * ldc + j;
        part += pc_icw[q] * logf(pc_probs[q]);
      }
    for (int i = blockIdx.x * 4 + wave; i < S; i += gridDim.x * 4) {
      size_t row = (size_t)b * S + i;
      TD* d = dy ? dy + row * ldd + dcol0 : nullptr;
      int lab = valid[row] >= 0 ? labels[row] : -1;   // wave-uniform from here on
      if (lab < 0 || lab > K) {
        if (d) { if (c0 < ncol) pcl_st(d + c0, 0.f); if (c1 < ncol) pcl_st(d + c1, 0.f); }
        continue;
      }
      const float* x = logits + row * ld + col0;
      float x0 = c0 < ncol ? x[c0] : -INFINITY, x1 = c1 < ncol ? x[c1] : -INFINITY;
      float mx = wave_reduce_max(fmaxf(x0, x1));
      float e0 = c0 < ncol ? expf(x0 - mx) : 0.f, e1 = c1 < ncol ? expf(x1 - mx) : 0.f;
      float se = wave_reduce_sum(e0 + e1);
      float p0 = e0 / se, p1 = e1 / se;
      float pt = __shfl(lab < 64 ? p0 : p1, lab & 63, 64);
      float g = 0.f;
      if (lab == K) {
        float w = cls_w[row];
        if (lane == 0) part += w * logf(pt);
        g = -w / pt;
      } else {
        int j = gt_assign[row];
        if (j >= 0 && j < npc) {
          size_t q = (size_t)b * ldc + j;
          g = -pc_icw[q] / ((float)pc_count[q] * pc_probs[q]);
        }
      }
      g = g / nb;
      if (d) {
        float gp = g * pt;                             // <g, p>: g has one non-zero entry
        if (c0 < ncol) pcl_st(d + c0, gscale * ((c0 == lab ? gp : 0.f) - p0 * gp));
        if (c1 < ncol) pcl_st(d + c1, gscale * ((c1 == lab ? gp : 0.f) - p1 * gp));
      }
    }
    float lb = pcl_block_sum(part, lds);
    if (nb > 0.f) partial += -lb / nb;                 // block-uniform: lb and nb come from LDS
  }
  if (tid != 0) return;
  if (acc == nullptr) { *loss = partial / (float)B; return; }
  float t;
  if (packed_sum_finish(acc, partial < 0.f ? 0.f : partial, gridDim.x * gridDim.y, &t)) *loss = t / (float)B;   // (-0 / rounding)
}

extern "C" int unit_pcl_loss(const float* logits, int ld, int col0, int K, const int* valid, int S, int B, const int* labels,
                             const float* cls_weights, const int* gt_assign, const int* pc_count, const float* pc_img_cls_weights,
                             const float* pc_probs, const int* n_pc, int ldc, float gscale, float* loss, void* dy, int dy_dtype,
                             int ldd, int dcol0, unsigned long long* acc, void* stream) {
  UNIT_CHECK_ARG(K > 0 && K < 96 && S >= 0 && B >= 0 && ldc >= 0, "pcl_loss: bad shape (K >= 96?)");
  UNIT_CHECK_ARG(col0 >= 0 && ld >= col0 + K + 1, "pcl_loss: logits columns [col0, col0+K+1) outside the row stride ld");
  UNIT_CHECK_ARG(dy == nullptr || (dcol0 >= 0 && ldd >= dcol0 + K + 1), "pcl_loss: dy columns [dcol0, dcol0+K+1) outside the row stride ldd");
  UNIT_CHECK_ARG(dy == nullptr || dy_dtype == UNIT_F32 || dy_dtype == UNIT_BF16, "pcl_loss: dy dtype");
  UNIT_CHECK_ARG((long)B * S < (1l << 31), "pcl_loss: B * S rows");
  hipStream_t s = (hipStream_t)stream;
  if (B == 0) return hipMemsetAsync(loss, 0, sizeof(float), s) == hipSuccess ? UNIT_OK : UNIT_ERR_LAUNCH;
  // <= 240 workgroups (packed_sum_finish counts arrivals in 8 bits), >= 16 rows per workgroup
  int gx = 1, gy = 1;
  if (acc != nullptr) {
    gy = B < 240 ? B : 240;
    gx = cdiv(S, 16);
    int cap = 240 / gy;
    gx = gx < 1 ? 1 : (gx > cap ? cap : gx);
  }
  dim3 grid(gx, gy);
  if (dy_dtype == UNIT_BF16 && dy != nullptr)
    pcl_loss_kernel<bf16_t><<<grid, 256, 0, s>>>(logits, ld, col0, K, valid, S, B, labels, cls_weights, gt_assign, pc_count,
                                                 pc_img_cls_weights, pc_probs, n_pc, ldc, gscale, loss, (bf16_t*)dy, ldd, dcol0, acc);
  else
    pcl_loss_kernel<float><<<grid, 256, 0, s>>>(logits, ld, col0, K, valid, S, B, labels, cls_weights, gt_assign, pc_count,
                                                pc_img_cls_weights, pc_probs, n_pc, ldc, gscale, loss, (float*)dy, ldd, dcol0, acc);
  UNIT_LAUNCH_CHECK();
  return UNIT_OK;
}
