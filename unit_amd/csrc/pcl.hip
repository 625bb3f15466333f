// pcl.hip -- Proposal Cluster Learning (Tang et al., TPAMI 2018), the weak detector's TYPE "PCL" loss:
//   PCLFunction  modeling/roi_heads/pcl_loss.py:6-61, applied per image at weak_detector_fast_rcnn.py:233-238.
// Loss value and d(loss)/d(logits) of one OICR refinement stream in one launch, the fused-loss convention of losses.hip.
//   compute_pcl_loss_inputs  weak_detector_fast_rcnn.py:476-507 (get_graph_centers :415-463): the loss's inputs, unit_pcl_targets below.
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

// ---------------------------------------------------------------------------------------------------
// PCL targets: compute_pcl_loss_inputs (weak_detector_fast_rcnn.py:476-507) with get_graph_centers (:415-463) and
// get_top_ranking_proposals (:465-474), for every image of the weak batch and a list of refinement streams in one launch: everything
// unit_pcl_loss consumes, in its fixed-slot layout. One workgroup per (image, stream); the classes of an image are sequential (the
// centres a class selects leave the rows before the next class is fitted).
//
// The k-means is tests/golden/pcl_kmeans.py step for step (that file's docstring is the specification: which sums are float32 and pairwise,
// which are float64 and sequential, the 256-row chunks of the Lloyd sums, relocation, both stopping rules). The seven doubles a fit draws
// from RandomState(3) do not depend on the data and the reference never passes another seed: they are constants here
// (unit_kmeans_draws exports them; tests/test_pcl_targets_cpu.py ties them to pcl_kmeans.draws()).
//
// The greedy loop follows the canonical rule of DESIGN.md section 8, the reference under a stable argsort: the FIRST node of maximum
// degree; the kept centres in descending score, the LATER cluster first among equal scores. The IoU graph is never stored: degrees are
// counted once (m^2 IoUs) and lowered by the edges to the rows each round removes (m^2 IoUs in total again), with the IoU arithmetic of
// unit_iou_match. Every loop is counted: Lloyd <= 300 rounds, greedy <= m rounds (a round removes at least one row, or finds no edge
// left and ends). The latter is the zero-area-box case, where the reference raises (torch.max of an empty tensor): the image is
// poisoned instead -- every cls_weight and pc_img_cls_weight of it is NaN, so unit_pcl_loss gives NaN and loss_dict() raises.
// ---------------------------------------------------------------------------------------------------
#define PT_SMAX 2048
#define PT_NT 256
#define PT_LLOYD_MAX 300

__device__ const double PT_DRAWS[7] = {0x1.1a022ec486c1ap-1, 0x1.6a9259f5c1b9ap-1, 0x1.29e2ee8f87b1ep-2, 0x1.058b32246f98cp-1,
                                       0x1.c93057dbf8d2ap-1, 0x1.cae6ed81332adp-1, 0x1.0132df0a66c68p-3};
static const double PT_DRAWS_HOST[7] = {0x1.1a022ec486c1ap-1, 0x1.6a9259f5c1b9ap-1, 0x1.29e2ee8f87b1ep-2, 0x1.058b32246f98cp-1,
                                        0x1.c93057dbf8d2ap-1, 0x1.cae6ed81332adp-1, 0x1.0132df0a66c68p-3};

struct PtShared {
  unsigned short row[PT_SMAX];   // the image's remaining rows (slot indices), ascending
  float p[PT_SMAX];              // clamped score of the current class per remaining row
  float x[PT_SMAX];              // k-means: centred scores; greedy loop: score of every kept centre
  float cl[PT_SMAX];             // k-means++: squared distance to the closest centre; greedy loop: node of every kept centre (as int)
  unsigned char lab[PT_SMAX];    // Lloyd labels
  unsigned char old[PT_SMAX];    // Lloyd labels of the round before; removal flags afterwards
  unsigned short top[PT_SMAX];   // top-ranking rows: positions into row[]
  short deg[PT_SMAX];
  unsigned char alive[PT_SMAX];
  unsigned short rem[PT_SMAX];   // the rows one greedy round removes
  double node[3][64];            // pairwise sums: 1-based heap of partial sums
  float cs[8][3], cw[8][3];      // Lloyd: per-chunk cluster sums and counts
  float rv[4]; int ri[4];        // reductions
  float bv; int bi;
  int scan[4];
  int cand[3];
  int nrem, npc, poison;
};

__device__ __forceinline__ float pt_iou(const f32x4 a, const f32x4 b) {      // == iou1 of boxes.hip
  float area1 = (a[2] - a[0]) * (a[3] - a[1]);
  float area2 = (b[2] - b[0]) * (b[3] - b[1]);
  float w = fminf(a[2], b[2]) - fmaxf(a[0], b[0]);
  float h = fminf(a[3], b[3]) - fmaxf(a[1], b[1]);
  w = w < 0.f ? 0.f : w;
  h = h < 0.f ? 0.f : h;
  float inter = w * h;
  return inter > 0.f ? inter / (area1 + area2 - inter) : 0.0f;
}

// block arg-max of (v, idx): the largest v, among equal v the smallest idx (later == false) or the largest (later == true). Threads
// without a candidate pass v = -INFINITY, idx = -1. Result in s.bv / s.bi (bi == -1: no candidate), valid after the call for all threads.
__device__ __forceinline__ void pt_argmax(PtShared& s, float v, int idx, bool later) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    float ov = __shfl_xor(v, o, 64);
    int oi = __shfl_xor(idx, o, 64);
    bool take = oi >= 0 && (idx < 0 || ov > v || (ov == v && (later ? oi > idx : oi < idx)));
    if (take) { v = ov; idx = oi; }
  }
  __syncthreads();
  if ((tid & 63) == 0) { s.rv[tid >> 6] = v; s.ri[tid >> 6] = idx; }
  __syncthreads();
  if (tid == 0) {
    float bv = s.rv[0]; int bi = s.ri[0];
    for (int w = 1; w < PT_NT / 64; ++w) {
      float ov = s.rv[w]; int oi = s.ri[w];
      if (oi >= 0 && (bi < 0 || ov > bv || (ov == bv && (later ? oi > bi : oi < bi)))) { bv = ov; bi = oi; }
    }
    s.bv = bv; s.bi = bi;
  }
  __syncthreads();
}

// exclusive scan of one int per thread in thread order; *total = the sum
__device__ __forceinline__ int pt_scan(PtShared& s, int v, int* total) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    int t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  __syncthreads();
  if (lane == 63) s.scan[w] = inc;
  __syncthreads();
  int base = 0, tot = 0;
  for (int i = 0; i < PT_NT / 64; ++i) { int t = s.scan[i]; tot += t; if (i < w) base += t; }
  *total = tot;
  return base + inc - v;
}

// numpy's add.reduce of n contiguous elements f(which, i) of type T (pairwise: halves rounded down to a multiple of 8 until a run has
// at most 128 elements, 8 running sums inside a run), NS <= 3 independent sums at once: wave `which` owns sum `which`, lane h the node
// h of a 1-based heap over the recursion (depth <= 5 for n <= 2048). Result: s.node[which][1].
template <typename T, int NS, typename F>
__device__ __forceinline__ void pt_pairwise(PtShared& s, int n, F f) {
  const int tid = threadIdx.x, which = tid >> 6, h = tid & 63;
  bool exists = h >= 1 && which < NS;
  int start = 0, len = n, depth = exists ? 31 - __clz(h) : 0;
  if (exists)
    for (int bit = depth - 1; bit >= 0; --bit) {
      if (len <= 128) { exists = false; break; }
      int n2 = len / 2;
      n2 -= n2 % 8;
      if ((h >> bit) & 1) { start += n2; len -= n2; } else len = n2;
    }
  const bool leaf = exists && (len <= 128 || depth == 5);
  __syncthreads();
  if (leaf) {
    T r;
    if (len < 8) {
      r = (T)0;
      for (int i = 0; i < len; ++i) r = r + f(which, start + i);
    } else {
      T a[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) a[j] = f(which, start + j);
      int i = 8;
      for (; i < len - (len % 8); i += 8) {
#pragma unroll
        for (int j = 0; j < 8; ++j) a[j] = a[j] + f(which, start + i + j);
      }
      r = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
      for (; i < len; ++i) r = r + f(which, start + i);
    }
    s.node[which][h] = (double)r;
  }
  __syncthreads();
  for (int d = 4; d >= 0; --d) {
    if (exists && !leaf && depth == d) s.node[which][h] = (double)((T)s.node[which][2 * h] + (T)s.node[which][2 * h + 1]);
    __syncthreads();
  }
}

// _euclidean_distances_upcast of one centre against one point (float64 inside, rounded to float32, clamped at 0)
__device__ __forceinline__ float pt_sqdist(float c, float x) {
  double c64 = (double)c, x64 = (double)x;
  double d = ((-2.0 * (c64 * x64)) + c64 * c64) + x64 * x64;
  return fmaxf((float)d, 0.f);
}

__device__ __forceinline__ int pt_assign(float x, const float (&cen)[3]) {
  float best = cen[0] * cen[0] + (-2.0f) * (x * cen[0]);
  int lab = 0;
#pragma unroll
  for (int j = 1; j < 3; ++j) {
    float d = cen[j] * cen[j] + (-2.0f) * (x * cen[j]);
    if (d < best) { best = d; lab = j; }
  }
  return lab;
}

// get_top_ranking_proposals on s.p[0, n): s.top[0, m) = ascending positions of the top-ranking rows; returns m >= 1 (n >= 1)
__device__ int pt_top_ranking(PtShared& s, int n) {
  const int tid = threadIdx.x;
  if (n < 3) {                                           // torch.argmax: the first maximum
    pt_argmax(s, tid < n ? s.p[tid] : -INFINITY, tid < n ? tid : -1, false);
    if (tid == 0) s.top[0] = (unsigned short)max(s.bi, 0);
    __syncthreads();
    return 1;
  }
  // ---- fit(): X -= X.mean(), tol = mean(var(X)) * 1e-4, float32 pairwise sums
  pt_pairwise<float, 1>(s, n, [&](int, int i) { return s.p[i]; });
  const float mean = (float)s.node[0][1] / (float)n;
  for (int i = tid; i < n; i += PT_NT) s.x[i] = s.p[i] - mean;
  pt_pairwise<float, 1>(s, n, [&](int, int i) { float d = s.x[i]; return d * d; });
  const float tol = ((float)s.node[0][1] / (float)n) * 1e-4f;
  // ---- k-means++, n_local_trials = 3
  if (tid == 0) {                                        // RandomState.choice(n, p = 1/n): float64 cdf, normalised, searched side='right'
    const double w = (double)(1.0f / (float)n), u0 = PT_DRAWS[0];
    double last = 0.0;
    for (int i = 0; i < n; ++i) last += w;
    double c = 0.0;
    int c0 = n - 1;
    for (int i = 0; i < n; ++i) {
      c += w;
      if (c / last > u0) { c0 = i; break; }
    }
    s.cand[0] = c0;
  }
  __syncthreads();
  float cen[3];
  cen[0] = s.x[s.cand[0]];
  for (int i = tid; i < n; i += PT_NT) s.cl[i] = pt_sqdist(cen[0], s.x[i]);
  pt_pairwise<double, 1>(s, n, [&](int, int i) { return (double)s.cl[i]; });
  float pot = (float)s.node[0][1];
  for (int c = 1; c < 3; ++c) {
    if (tid == 0) {                                      // searchsorted (side='left') in the sequential float64 cumulative sum
      const double r0 = PT_DRAWS[1 + 3 * (c - 1)] * (double)pot, r1 = PT_DRAWS[2 + 3 * (c - 1)] * (double)pot,
                   r2 = PT_DRAWS[3 + 3 * (c - 1)] * (double)pot;
      int c0 = -1, c1 = -1, c2 = -1;
      double cum = 0.0;
      for (int i = 0; i < n; ++i) {
        cum += (double)s.cl[i];
        if (c0 < 0 && cum >= r0) c0 = i;
        if (c1 < 0 && cum >= r1) c1 = i;
        if (c2 < 0 && cum >= r2) c2 = i;
        if (c0 >= 0 && c1 >= 0 && c2 >= 0) break;
      }
      s.cand[0] = c0 < 0 ? n - 1 : c0; s.cand[1] = c1 < 0 ? n - 1 : c1; s.cand[2] = c2 < 0 ? n - 1 : c2;
    }
    __syncthreads();
    pt_pairwise<double, 3>(s, n, [&](int t, int i) { return (double)fminf(s.cl[i], pt_sqdist(s.x[s.cand[t]], s.x[i])); });
    int best = 0;
    float bp = (float)s.node[0][1];
    for (int t = 1; t < 3; ++t) { float pt = (float)s.node[t][1]; if (pt < bp) { bp = pt; best = t; } }
    cen[c] = s.x[s.cand[best]];
    pot = bp;
    __syncthreads();                                     // cand / node are rewritten below
    for (int i = tid; i < n; i += PT_NT) s.cl[i] = fminf(s.cl[i], pt_sqdist(cen[c], s.x[i]));
    __syncthreads();
  }
  // ---- Lloyd
  for (int i = tid; i < n; i += PT_NT) s.old[i] = 255;
  const int nchunk = (n + 255) >> 8;
  bool strict = false;
  for (int it = 0; it < PT_LLOYD_MAX; ++it) {
    for (int i = tid; i < n; i += PT_NT) s.lab[i] = (unsigned char)pt_assign(s.x[i], cen);
    __syncthreads();
    {                                                    // sequential float32 sums inside 256-row chunks: chunk c on wave c & 3, lane c >> 2
      const int c = ((tid & 63) << 2) | (tid >> 6);
      if ((tid & 63) < 2 && c < nchunk) {
        float a0 = 0.f, a1 = 0.f, a2 = 0.f;
        int k0 = 0, k1 = 0, k2 = 0;
        const int e = min(n, (c + 1) << 8);
        for (int i = c << 8; i < e; ++i) {
          const int l = s.lab[i];
          const float v = s.x[i];
          if (l == 0) { a0 += v; ++k0; } else if (l == 1) { a1 += v; ++k1; } else { a2 += v; ++k2; }
        }
        s.cs[c][0] = a0; s.cs[c][1] = a1; s.cs[c][2] = a2;
        s.cw[c][0] = (float)k0; s.cw[c][1] = (float)k1; s.cw[c][2] = (float)k2;
      }
    }
    __syncthreads();
    float csum[3] = {0.f, 0.f, 0.f}, wsum[3] = {0.f, 0.f, 0.f};
    for (int c = 0; c < nchunk; ++c)
#pragma unroll
      for (int j = 0; j < 3; ++j)
        if (s.cw[c][j] > 0.f) { csum[j] += s.cs[c][j]; wsum[j] += s.cw[c][j]; }
    const bool e0 = wsum[0] == 0.f, e1 = wsum[1] == 0.f, e2 = wsum[2] == 0.f;
    if (e0 || e1 || e2) {                                // _relocate_empty_clusters: the farthest points, the last index among equals
      int taken0 = -1, taken1 = -1;
      bool go = true;
      for (int e = 0; e < 3 && go; ++e) {
        if (!(e == 0 ? e0 : (e == 1 ? e1 : e2))) continue;
        float bv = -INFINITY;
        int bi = -1;
        for (int i = tid; i < n; i += PT_NT) {
          if (i == taken0 || i == taken1) continue;
          const int l = s.lab[i];
          const float d0 = s.x[i] - (l == 0 ? cen[0] : (l == 1 ? cen[1] : cen[2]));
          const float d = d0 * d0;
          if (bi < 0 || d > bv || (d == bv && i > bi)) { bv = d; bi = i; }
        }
        pt_argmax(s, bv, bi, true);
        const int far = s.bi;
        if (far < 0 || (taken0 < 0 && s.bv == 0.f)) { go = false; break; }      // dist.max() == 0: nothing is relocated
        const int oldl = s.lab[far];
        const float xf = s.x[far];
        __syncthreads();
        if (tid == 0) s.lab[far] = (unsigned char)e;
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          if (j == oldl) { csum[j] = csum[j] - xf; wsum[j] = wsum[j] - 1.0f; }
        }
#pragma unroll
        for (int j = 0; j < 3; ++j)
          if (j == e) { csum[j] = xf; wsum[j] = 1.0f; }
        if (taken0 < 0) taken0 = far; else taken1 = far;
      }
    }
    float nw[3], tot = 0.f, sh[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      nw[j] = wsum[j] > 0.f ? csum[j] * (float)(1.0 / (double)wsum[j]) : csum[j];
      const float d = nw[j] - cen[j];
      sh[j] = sqrtf(d * d);
      cen[j] = nw[j];
    }
    tot = (sh[0] * sh[0] + sh[1] * sh[1]) + sh[2] * sh[2];
    int diff = 0;
    for (int i = tid; i < n; i += PT_NT) diff |= s.lab[i] != s.old[i];
    if (!__syncthreads_or(diff)) { strict = true; break; }
    if (tot <= tol) break;
    for (int i = tid; i < n; i += PT_NT) s.old[i] = s.lab[i];
    __syncthreads();
  }
  if (!strict) {
    __syncthreads();
    for (int i = tid; i < n; i += PT_NT) s.lab[i] = (unsigned char)pt_assign(s.x[i], cen);
  }
  __syncthreads();
  // ---- the members of the cluster whose centre (+ mean, float32) is the largest, the first among equals
  int hi = 0;
  float hv = cen[0] + mean;
  for (int j = 1; j < 3; ++j) { float v = cen[j] + mean; if (v > hv) { hv = v; hi = j; } }
  const int per = (n + PT_NT - 1) / PT_NT, lo = min(n, tid * per), up = min(n, lo + per);
  int cnt = 0;
  for (int i = lo; i < up; ++i) cnt += s.lab[i] == hi;
  int m, o = pt_scan(s, cnt, &m);
  for (int i = lo; i < up; ++i) if (s.lab[i] == hi) s.top[o++] = (unsigned short)i;
  __syncthreads();
  if (m == 0) {
    float bv = -INFINITY;
    int bi = -1;
    for (int i = tid; i < n; i += PT_NT) if (bi < 0 || s.p[i] > bv) { bv = s.p[i]; bi = i; }
    pt_argmax(s, bv, bi, false);
    if (tid == 0) s.top[0] = (unsigned short)max(s.bi, 0);
    __syncthreads();
    m = 1;
  }
  return m;
}

struct PtSrc { const float* m; int ld, col0, mode; const float* mx; const float* se; };
// clamp(p, 1e-9, 1 - 1e-9) as torch clamps a float32 tensor: the upper bound rounds to 1
__device__ __forceinline__ float pt_prob(const PtSrc& q, size_t row, int i, int c) {
  float v = q.m[row * q.ld + q.col0 + c];
  if (q.mode == 1) v = expf(v - q.mx[i]) / q.se[i];       // == unit_softmax_rows
  return fminf(fmaxf(v, 1e-9f), 1.0f);
}

__global__ __launch_bounds__(PT_NT) void pcl_targets_kernel(const float* __restrict__ src, int ld, int col0, int mode, int step,
                                                           const float* __restrict__ nxt, int ldn, int ncol0, int nmode, int nstep, int K,
                                                           const float* __restrict__ rois5, const int* __restrict__ valid, int S, int B,
                                                           const unsigned char* __restrict__ multihot, float fg_thresh, float bg_thresh,
                                                           float graph_thresh, int max_pc, int* __restrict__ labels,
                                                           float* __restrict__ cls_w, int* __restrict__ gt_assign, int* __restrict__ n_pc,
                                                           int* __restrict__ pc_labels, int* __restrict__ pc_count,
                                                           float* __restrict__ pc_icw, float* __restrict__ pc_probs, int ldc,
                                                           float* __restrict__ gt_boxes /* [n_streams][B*S][4] or null */,
                                                           float* __restrict__ ws, int S4) {
  __shared__ PtShared s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x, t = blockIdx.y;
  const size_t unit = (size_t)t * B + b, row0 = (size_t)b * S;
  float* w0 = ws + unit * 13 * (size_t)S4;
  f32x4* cbox = reinterpret_cast<f32x4*>(w0);
  f32x4* gbox = reinterpret_cast<f32x4*>(w0 + 4 * (size_t)S4);
  float* gscore = w0 + 8 * (size_t)S4;
  float* mx0 = gscore + S4; float* se0 = mx0 + S4; float* mx1 = se0 + S4; float* se1 = mx1 + S4;
  const PtSrc q0 = {src, ld, col0 + t * step, mode, mx0, se0}, q1 = {nxt, ldn, ncol0 + t * nstep, nmode, mx1, se1};
  labels += unit * S; cls_w += unit * S; gt_assign += unit * S;
  // the row's matched centre box (label_and_sample_proposals :337-346), written by the thread that owns the row
  f32x4* gout = gt_boxes ? reinterpret_cast<f32x4*>(gt_boxes) + unit * S : nullptr;
  pc_labels += unit * ldc; pc_count += unit * ldc; pc_icw += unit * ldc; pc_probs += unit * ldc;

  // ---- the image's rows; softmax statistics of the logits inputs
  int n = 0;
  {
    const int per = (S + PT_NT - 1) / PT_NT, lo = min(S, tid * per), up = min(S, lo + per);
    int cnt = 0;
    for (int i = lo; i < up; ++i) cnt += valid[row0 + i] >= 0;
    int o = pt_scan(s, cnt, &n);
    for (int i = lo; i < up; ++i) if (valid[row0 + i] >= 0) s.row[o++] = (unsigned short)i;
    if (tid == 0) { s.npc = 0; s.poison = 0; }
  }
  for (int i = tid; i < S; i += PT_NT) {
    if (valid[row0 + i] < 0) continue;
    for (int w = 0; w < 2; ++w) {
      const PtSrc& q = w ? q1 : q0;
      if (q.mode != 1) continue;
      const float* x = q.m + (row0 + i) * q.ld + q.col0;
      float mx = -INFINITY, se = 0.f;
      for (int c = 0; c <= K; ++c) mx = fmaxf(mx, x[c]);
      for (int c = 0; c <= K; ++c) se += expf(x[c] - mx);
      (w ? mx1 : mx0)[i] = mx; (w ? se1 : se0)[i] = se;
    }
  }
  __syncthreads();

  // ---- get_graph_centers: the classes in ascending order over the rows still present
  for (int c = 0; c < K; ++c) {
    if (!multihot[(size_t)b * K + c] || n == 0) continue;            // block-uniform
    for (int i = tid; i < n; i += PT_NT) s.p[i] = pt_prob(q0, row0 + s.row[i], s.row[i], c);
    __syncthreads();
    const int m = pt_top_ranking(s, n);
    for (int i = tid; i < m; i += PT_NT) {
      const float* r = rois5 + (row0 + s.row[s.top[i]]) * 5;
      cbox[i] = f32x4{r[1], r[2], r[3], r[4]};
      s.alive[i] = 1;
    }
    for (int i = tid; i < n; i += PT_NT) s.old[i] = 0;               // removal flags
    __syncthreads();
    for (int i = tid; i < m; i += PT_NT) {
      const f32x4 bi = cbox[i];
      int d = 0;
      for (int j = 0; j < m; ++j) d += pt_iou(bi, cbox[j]) > graph_thresh;
      s.deg[i] = (short)d;
    }
    __syncthreads();
    float* kscore = s.x;
    int* knode = reinterpret_cast<int*>(s.cl);
    int count = m, nk = 0;
    for (int round = 0; round < m; ++round) {
      float bv = -INFINITY;
      int bi = -1;
      for (int i = tid; i < m; i += PT_NT) { float d = (float)s.deg[i]; if (bi < 0 || d > bv) { bv = d; bi = i; } }
      pt_argmax(s, bv, bi, false);
      const int v = s.bi;
      if (v < 0 || s.bv <= 0.f) {                                    // no edge left: the reference raises here
        if (tid == 0) s.poison = 1;
        break;
      }
      if (tid == 0) s.nrem = 0;
      __syncthreads();
      const f32x4 bxv = cbox[v];
      float sc = -INFINITY;
      for (int j = tid; j < m; j += PT_NT)
        if (s.alive[j] && pt_iou(bxv, cbox[j]) > graph_thresh) {
          s.rem[atomicAdd(&s.nrem, 1)] = (unsigned short)j;
          sc = fmaxf(sc, s.p[s.top[j]]);
          s.alive[j] = 0;
          s.deg[j] = 0;
        }
      pt_argmax(s, sc, sc > -INFINITY ? tid : -1, false);
      if (tid == 0) { kscore[nk] = s.bv; knode[nk] = v; }
      ++nk;
      const int nr = s.nrem;
      count -= nr;
      if (count <= 5) break;
      for (int i = tid; i < m; i += PT_NT) {
        if (!s.alive[i]) continue;
        const f32x4 bi2 = cbox[i];
        int d = 0;
        for (int k = 0; k < nr; ++k) d += pt_iou(bi2, cbox[s.rem[k]]) > graph_thresh;
        s.deg[i] = (short)(s.deg[i] - d);
      }
      __syncthreads();
    }
    __syncthreads();
    // ---- at most max_pc centres: descending score, the later cluster first among equal scores
    const int nsel = min(nk, max_pc);
    for (int qi = 0; qi < nsel; ++qi) {
      float bv = -INFINITY;
      int bi = -1;
      for (int k = tid; k < nk; k += PT_NT) { float v = kscore[k]; if (v > -INFINITY && (bi < 0 || v >= bv)) { bv = v; bi = k; } }
      pt_argmax(s, bv, bi, true);
      if (s.bi < 0) break;                                           // (scores are >= 1e-9: only NaN inputs get here)
      if (tid == 0) {
        const int k = s.bi, v = knode[k], g = s.npc;
        if (g < ldc && g < S) {
          gbox[g] = cbox[v]; gscore[g] = kscore[k]; pc_labels[g] = c;
          s.npc = g + 1;
        } else {
          s.poison = 1;                                              // ldc too small for this image: never silently dropped
        }
        s.old[s.top[v]] = 1;
        kscore[k] = -INFINITY;
      }
      __syncthreads();
    }
    __syncthreads();
    // ---- the selected rows leave before the next class
    {
      const int per = (n + PT_NT - 1) / PT_NT, lo = min(n, tid * per), up = min(n, lo + per);
      unsigned short keep[PT_SMAX / PT_NT];
      int cnt = 0;
#pragma unroll
      for (int k = 0; k < PT_SMAX / PT_NT; ++k) {
        const int i = lo + k;
        if (i < up && !s.old[i]) keep[cnt++] = s.row[i];
      }
      int tot, o = pt_scan(s, cnt, &tot);
      __syncthreads();
      for (int k = 0; k < cnt; ++k) s.row[o + k] = keep[k];
      n = tot;
      __syncthreads();
    }
  }
  __syncthreads();

  // ---- label_and_sample_proposals with Matcher([0.5], [0, 1]) over the cluster boxes (first maximum IoU), then :490-499
  const int M = s.npc, poison = s.poison;
  for (int i = tid; i < S; i += PT_NT) {
    const size_t row = row0 + i;
    if (valid[row] < 0 || M == 0) {
      if (gout) gout[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (valid[row] < 0) { labels[i] = -1; cls_w[i] = 0.f; gt_assign[i] = -1; continue; }
      labels[i] = K; cls_w[i] = poison ? NAN : 0.f; gt_assign[i] = -1; continue;
    }
    const float* r = rois5 + row * 5;
    const f32x4 me = {r[1], r[2], r[3], r[4]};
    float best = -1.f;
    int bi = 0;
    for (int g = 0; g < M; ++g) { float v = pt_iou(gbox[g], me); if (v > best) { best = v; bi = g; } }
    labels[i] = best >= 0.5f ? pc_labels[bi] : K;
    float w = gscore[bi];
    if (best < bg_thresh) w = 0.f;
    cls_w[i] = poison ? NAN : w;
    gt_assign[i] = best < fg_thresh ? -1 : bi;
    if (gout) gout[i] = gbox[bi];
  }
  __threadfence_block();
  __syncthreads();
  // ---- per cluster: pc_count, sum of cls_weights, mean next-iteration score (:501-507). One wave per cluster, rows in lane order.
  for (int g = wave; g < ldc; g += PT_NT / 64) {
    if (g >= M) {
      if (lane == 0) { pc_labels[g] = -1; pc_count[g] = 0; pc_icw[g] = 0.f; pc_probs[g] = 0.f; }
      continue;
    }
    const int cls = pc_labels[g];
    float cnt = 0.f, sw = 0.f, sp = 0.f;
    for (int i = lane; i < S; i += 64) {
      if (valid[row0 + i] < 0 || gt_assign[i] != g) continue;
      cnt += 1.f;
      sw += cls_w[i];
      sp += pt_prob(q1, row0 + i, i, cls);
    }
    cnt = wave_reduce_sum(cnt); sw = wave_reduce_sum(sw); sp = wave_reduce_sum(sp);
    if (lane == 0) { pc_count[g] = (int)cnt; pc_icw[g] = sw; pc_probs[g] = sp / cnt; }
  }
  if (tid == 0) n_pc[unit] = M;
}

extern "C" int unit_kmeans_draws(unsigned long long* bits7) {
  memcpy(bits7, PT_DRAWS_HOST, sizeof(PT_DRAWS_HOST));
  return UNIT_OK;
}

extern "C" size_t unit_workspace_bytes_pcl_targets(int B, int S, int n_streams) {
  if (B < 0 || S < 0 || n_streams < 0) return 0;
  size_t s4 = ((size_t)S + 3) & ~(size_t)3;
  return sizeof(float) * 13 * s4 * (size_t)B * (size_t)n_streams + 16;
}

extern "C" int unit_pcl_targets_ex(const float* src, int ld, int col0, int mode, int step, const float* nxt, int ldn, int ncol0, int nmode,
                                   int nstep, int K, const float* rois5, const int* valid, int S, int B, int n_streams,
                                   const unsigned char* multihot, float fg_thresh, float bg_thresh, float graph_iou_thresh, int max_pc_num,
                                   int* labels, float* cls_weights, int* gt_assign, int* n_pc, int* pc_labels, int* pc_count,
                                   float* pc_img_cls_weights, float* pc_probs, int ldc, float* gt_boxes, void* workspace,
                                   size_t workspace_bytes, void* stream) {
  UNIT_CHECK_ARG(((uintptr_t)gt_boxes & 15) == 0, "pcl_targets: gt_boxes must be 16-byte aligned");
  UNIT_CHECK_ARG(K > 0 && K < 96 && S >= 0 && B >= 0 && n_streams >= 0, "pcl_targets: bad shape (K >= 96?)");
  UNIT_CHECK_ARG(S <= PT_SMAX, "pcl_targets: S > 2048 rows per image");
  UNIT_CHECK_ARG((mode == 0 || mode == 1) && (nmode == 0 || nmode == 1), "pcl_targets: mode is 0 (probabilities) or 1 (logits)");
  UNIT_CHECK_ARG(max_pc_num >= 1 && ldc >= max_pc_num, "pcl_targets: ldc smaller than max_pc_num");
  UNIT_CHECK_ARG(n_streams <= 65535 && step >= 0 && nstep >= 0, "pcl_targets: stream list");
  const int last = n_streams > 0 ? n_streams - 1 : 0;
  UNIT_CHECK_ARG(col0 >= 0 && ld >= col0 + last * step + K + mode, "pcl_targets: source columns outside the row stride ld");
  UNIT_CHECK_ARG(ncol0 >= 0 && ldn >= ncol0 + last * nstep + K + 1, "pcl_targets: next-iteration columns outside the row stride ldn");
  UNIT_CHECK_ARG((long)B * S < (1l << 31) && (long)B * S * (n_streams > 0 ? n_streams : 1) < (1l << 31), "pcl_targets: B * S rows");
  if (workspace_bytes < unit_workspace_bytes_pcl_targets(B, S, n_streams)) { unit_set_error("pcl_targets: workspace too small"); return UNIT_ERR_WORKSPACE; }
  if (B == 0 || n_streams == 0) return UNIT_OK;
  float* ws = reinterpret_cast<float*>(((uintptr_t)workspace + 15) & ~(uintptr_t)15);
  pcl_targets_kernel<<<dim3(B, n_streams), PT_NT, 0, (hipStream_t)stream>>>(
      src, ld, col0, mode, step, nxt, ldn, ncol0, nmode, nstep, K, rois5, valid, S, B, multihot, fg_thresh, bg_thresh, graph_iou_thresh,
      max_pc_num, labels, cls_weights, gt_assign, n_pc, pc_labels, pc_count, pc_img_cls_weights, pc_probs, ldc, gt_boxes, ws, (S + 3) & ~3);
  UNIT_LAUNCH_CHECK();
  return UNIT_OK;
}
extern "C" int unit_pcl_targets(const float* src, int ld, int col0, int mode, int step, const float* nxt, int ldn, int ncol0, int nmode,
                                int nstep, int K, const float* rois5, const int* valid, int S, int B, int n_streams,
                                const unsigned char* multihot, float fg_thresh, float bg_thresh, float graph_iou_thresh, int max_pc_num,
                                int* labels, float* cls_weights, int* gt_assign, int* n_pc, int* pc_labels, int* pc_count,
                                float* pc_img_cls_weights, float* pc_probs, int ldc, void* workspace, size_t workspace_bytes,
                                void* stream) {
  return unit_pcl_targets_ex(src, ld, col0, mode, step, nxt, ldn, ncol0, nmode, nstep, K, rois5, valid, S, B, n_streams, multihot, fg_thresh,
                             bg_thresh, graph_iou_thresh, max_pc_num, labels, cls_weights, gt_assign, n_pc, pc_labels, pc_count,
                             pc_img_cls_weights, pc_probs, ldc, nullptr, workspace, workspace_bytes, stream);
}
