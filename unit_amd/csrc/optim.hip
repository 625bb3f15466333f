// optim.hip -- Detectron2's gradient clipping (solver/build.py maybe_add_gradient_clipping: torch clip_grad_value_ / clip_grad_norm_ per
// parameter, "full_model" = one coefficient for all) and torch.optim.SGD's Nesterov form on the flat parameter store, sync-free:
//   unit_grad_clip_coefs  per-tensor p-norms (p = 1, 2, inf) of g * grad_scale and the coefficients min(1, clip / (norm + 1e-6)) for the
//                         rows [seg_lo, seg_hi) of a device table of (offset, numel): TWO launches for any number of tensors.
//   unit_sgd_step         unit_sgd_momentum's update on a flat range with the clip applied on the fly (the gradient buffer is only read)
//                         and the optional Nesterov look-ahead.
//   unit_sgd_step_masked  unit_sgd_step that leaves the tensors of dead table rows (live[r] == 0) untouched: what torch.optim.SGD does with a
//                         parameter whose .grad is None (no weight decay, no momentum) -- the weak-only training mode.
//
// Norm layout. A tensor is cut into chunks of CLIP_CHUNK elements counted from ITS OWN first element (the last one short): a chunk never
// spans two tensors and the partition depends on the table alone. Launch 1: one 256-lane workgroup per chunk; every lane adds its
// elements in a fixed order into an fp64 accumulator (fp64 FMA rate is far above what one read of the gradients needs), lanes combine by
// a shuffle tree, the four waves through LDS in wave order -> one fp64 partial per chunk in the caller's workspace. Launch 2: ONE
// workgroup; a wave per tensor adds the tensor's partials (lane-strided, shuffle tree), takes the root, writes norm and coefficient;
// under the full-model flag wave 0 then folds the per-tensor values into one coefficient. No atomics, no arrival order anywhere: the
// result is the same bit for bit on every run. fp64 accumulation leaves one fp32 rounding in the norm (2^-24 relative).
// Which chunk a workgroup owns: the exclusive prefix of the rows' chunk counts, rebuilt by every workgroup in LDS from the table (a few
// hundred rows, L2-resident: loads + one wave scan) -- no state beside the table, so a fresh workspace can never send a kernel astray.
// The host states the chunk count of the range (it sizes the grid); the combine kernel checks it against the table and answers NaN
// for the whole range if they differ, as it does for a row that does not lie inside the gradient buffer (such a row is never read).
// Offsets may be any element (packed fused heads): per chunk a scalar head up to the first 16-byte boundary, 16-byte loads, scalar tail.
// The max-norm propagates NaN like torch.linalg.vector_norm(inf) (fmax would drop it).
#include "common.h"

#define CLIP_CHUNK 16384
#define CLIP_THREADS 256
#define CLIP_MAX_ROWS 4096          // rows per call: the prefix lives in LDS
#define CLIP_FIN_THREADS 1024

#define NORM_INF 0
#define NORM_L1 1
#define NORM_L2 2

__device__ __forceinline__ bool clip_row_ok(long off, long n, long g_numel) { return off >= 0 && n >= 0 && off <= g_numel && n <= g_numel - off; }

template <int KIND> __device__ __forceinline__ double clip_comb(double a, double b) {
  if (KIND == NORM_INF) return (b > a || b != b) ? b : a;          // NaN on either side stays
  return a + b;
}
template <int KIND> __device__ __forceinline__ void clip_acc(double& a, float g, float scale) {
  float x = g * scale;          // the value the update uses
  if (KIND == NORM_L2) a += (double)x * (double)x;
  else a = clip_comb<KIND>(a, fabs((double)x));
}
template <int KIND> __device__ __forceinline__ double clip_wave_reduce(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = clip_comb<KIND>(v, __shfl_xor(v, o, 64));
  return v;
}

// pre[0 .. n] = exclusive prefix of the chunk counts of rows seg_lo .. seg_lo + n (a row outside the buffer counts 0); every thread of the
// workgroup calls it, n <= CLIP_MAX_ROWS; ends with a barrier
__device__ __forceinline__ void clip_chunk_prefix(const long* __restrict__ table, int seg_lo, int n, long g_numel, int* pre) {
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    long off = table[2 * (long)(seg_lo + i)], m = table[2 * (long)(seg_lo + i) + 1];
    pre[i] = clip_row_ok(off, m, g_numel) ? (int)((m + CLIP_CHUNK - 1) / CLIP_CHUNK) : 0;
  }
  __syncthreads();
  if (threadIdx.x < 64) {          // wave 0: a contiguous run of rows per lane, then a scan of the 64 run totals
    const int lane = threadIdx.x, per = (n + 63) / 64, a = lane * per;
    int s = 0;
    for (int k = 0; k < per; ++k) if (a + k < n) s += pre[a + k];
    int incl = s;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { int t = __shfl_up(incl, o, 64); if (lane >= o) incl += t; }
    int run = incl - s;
    for (int k = 0; k < per; ++k) if (a + k < n) { int c = pre[a + k]; pre[a + k] = run; run += c; }
    if (lane == 63) pre[n] = incl;
  }
  __syncthreads();
}

template <int KIND>
__global__ void __launch_bounds__(CLIP_THREADS) clip_partial_kernel(const float* __restrict__ g, long g_numel, const long* __restrict__ table,
                                                                    int seg_lo, int n, float scale, double* __restrict__ part) {
  __shared__ int pre[CLIP_MAX_ROWS + 1];
  __shared__ int sh_row;
  __shared__ double sh_w[CLIP_THREADS / 64];
  const int tid = threadIdx.x, b = blockIdx.x;
  if (tid == 0) sh_row = -1;
  clip_chunk_prefix(table, seg_lo, n, g_numel, pre);
  for (int i = tid; i < n; i += CLIP_THREADS) if (pre[i] <= b && b < pre[i + 1]) sh_row = i;          // exactly one row owns chunk b
  __syncthreads();
  const int row = sh_row;
  if (row < 0) return;          // the host asked for more chunks than the table has: the combine kernel reports it
  const long off = table[2 * (long)(seg_lo + row)], numel = table[2 * (long)(seg_lo + row) + 1];
  const long c0 = (long)(b - pre[row]) * CLIP_CHUNK;
  const int len = (int)(numel - c0 < CLIP_CHUNK ? numel - c0 : CLIP_CHUNK);
  const float* gp = g + off + c0;
  int head = (int)((4 - (((uintptr_t)gp >> 2) & 3)) & 3);
  if (head > len) head = len;
  const int nvec = (len - head) >> 2, tail = len - head - 4 * nvec;
  double a = 0.0;
  if (tid < head) clip_acc<KIND>(a, gp[tid], scale);
  const f32x4* vp = reinterpret_cast<const f32x4*>(gp + head);
  int v = tid;
  for (; v + 3 * CLIP_THREADS < nvec; v += 4 * CLIP_THREADS) {          // four 16-byte loads in flight per lane
    f32x4 x0 = vp[v], x1 = vp[v + CLIP_THREADS], x2 = vp[v + 2 * CLIP_THREADS], x3 = vp[v + 3 * CLIP_THREADS];
#pragma unroll
    for (int j = 0; j < 4; ++j) clip_acc<KIND>(a, x0[j], scale);
#pragma unroll
    for (int j = 0; j < 4; ++j) clip_acc<KIND>(a, x1[j], scale);
#pragma unroll
    for (int j = 0; j < 4; ++j) clip_acc<KIND>(a, x2[j], scale);
#pragma unroll
    for (int j = 0; j < 4; ++j) clip_acc<KIND>(a, x3[j], scale);
  }
  for (; v < nvec; v += CLIP_THREADS) {
    f32x4 x0 = vp[v];
#pragma unroll
    for (int j = 0; j < 4; ++j) clip_acc<KIND>(a, x0[j], scale);
  }
  if (tid < tail) clip_acc<KIND>(a, gp[head + 4 * nvec + tid], scale);
  a = clip_wave_reduce<KIND>(a);
  if ((tid & 63) == 0) sh_w[tid >> 6] = a;
  __syncthreads();
  if (tid == 0) {
    double t = sh_w[0];
    for (int w = 1; w < CLIP_THREADS / 64; ++w) t = clip_comb<KIND>(t, sh_w[w]);
    part[b] = t;
  }
}

__device__ __forceinline__ float clip_coef_of(double norm, float clip_value) {
  float nf = (float)norm;
  if (!(nf - nf == 0.f)) return __builtin_nanf("");          // NaN or infinite norm (torch: error_if_nonfinite=False, this tensor only)
  return (float)fmin(1.0, (double)clip_value / (norm + 1e-6));
}

template <int KIND>
__global__ void __launch_bounds__(CLIP_FIN_THREADS) clip_finish_kernel(const long* __restrict__ table, long g_numel, int seg_lo, int n, int n_chunks,
                                                                       float clip_value, int full_model, const double* __restrict__ part,
                                                                       float* __restrict__ norms, float* __restrict__ coefs) {
  __shared__ int pre[CLIP_MAX_ROWS + 1];
  __shared__ double rowv[CLIP_MAX_ROWS];          // per row: sum of squares / sum / max, before the root
  __shared__ double sh_total;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  clip_chunk_prefix(table, seg_lo, n, g_numel, pre);
  const bool ok = pre[n] == n_chunks;
  for (int i = wave; i < n; i += CLIP_FIN_THREADS / 64) {
    const long off = table[2 * (long)(seg_lo + i)], numel = table[2 * (long)(seg_lo + i) + 1];
    double a = 0.0;
    if (ok) for (int k = pre[i] + lane; k < pre[i + 1]; k += 64) a = clip_comb<KIND>(a, part[k]);
    a = clip_wave_reduce<KIND>(a);
    if (!ok || !clip_row_ok(off, numel, g_numel)) a = __builtin_nan("");
    if (lane == 0) {
      rowv[i] = a;
      double nrm = KIND == NORM_L2 ? sqrt(a) : a;
      norms[seg_lo + i] = (float)nrm;
      if (!full_model) coefs[seg_lo + i] = clip_coef_of(nrm, clip_value);
    }
  }
  if (!full_model) return;
  __syncthreads();
  if (wave == 0) {          // the p-norm of the per-tensor norms = the p-norm of everything
    double a = 0.0;
    for (int i = lane; i < n; i += 64) a = clip_comb<KIND>(a, rowv[i]);
    a = clip_wave_reduce<KIND>(a);
    if (lane == 0) sh_total = KIND == NORM_L2 ? sqrt(a) : a;
  }
  __syncthreads();
  const float c = clip_coef_of(sh_total, clip_value);
  for (int i = tid; i < n; i += CLIP_FIN_THREADS) coefs[seg_lo + i] = c;
}

extern "C" int unit_grad_clip_chunk(void) { return CLIP_CHUNK; }
extern "C" size_t unit_grad_clip_workspace_bytes(long g_numel, int n_seg) {
  return (size_t)(g_numel / CLIP_CHUNK + n_seg + 1) * sizeof(double);          // a tensor adds at most one short chunk
}

template <int KIND>
static int clip_launch(const float* g, long g_numel, const long* table, int seg_lo, int n, int n_chunks, float clip_value, float grad_scale,
                       int full_model, float* norms, float* coefs, double* part, hipStream_t st) {
  if (n_chunks > 0) {
    clip_partial_kernel<KIND><<<n_chunks, CLIP_THREADS, 0, st>>>(g, g_numel, table, seg_lo, n, grad_scale, part);
    UNIT_LAUNCH_CHECK();
  }
  clip_finish_kernel<KIND><<<1, CLIP_FIN_THREADS, 0, st>>>(table, g_numel, seg_lo, n, n_chunks, clip_value, full_model, part, norms, coefs);
  UNIT_LAUNCH_CHECK();
  return UNIT_OK;
}

extern "C" int unit_grad_clip_coefs(const float* g, long g_numel, const long* table, int n_seg, int seg_lo, int seg_hi, int n_chunks,
                                    int norm_kind, float clip_value, float grad_scale, int full_model, float* norms, float* coefs,
                                    void* workspace, size_t workspace_bytes, void* stream) {
  UNIT_CHECK_ARG(g && table && norms && coefs, "grad_clip_coefs: null pointer");
  UNIT_CHECK_ARG((uintptr_t)g % 4 == 0 && (uintptr_t)table % 8 == 0, "grad_clip_coefs: alignment");
  UNIT_CHECK_ARG(0 <= seg_lo && seg_lo <= seg_hi && seg_hi <= n_seg, "grad_clip_coefs: row range outside the table");
  UNIT_CHECK_ARG(norm_kind == NORM_INF || norm_kind == NORM_L1 || norm_kind == NORM_L2, "grad_clip_coefs: norm_kind must be 0 (inf), 1 or 2");
  UNIT_CHECK_ARG(g_numel >= 0 && n_chunks >= 0, "grad_clip_coefs: negative size");
  const int n = seg_hi - seg_lo;
  if (n == 0) return UNIT_OK;
  if (n > CLIP_MAX_ROWS) { unit_set_error("grad_clip_coefs: more than 4096 rows in one call"); return UNIT_ERR_UNSUPPORTED; }
  if (!workspace || (uintptr_t)workspace % 8 || workspace_bytes < (size_t)n_chunks * sizeof(double)) {
    unit_set_error("grad_clip_coefs: workspace missing, misaligned or smaller than one double per chunk");
    return UNIT_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  double* part = (double*)workspace;
  if (norm_kind == NORM_L2) return clip_launch<NORM_L2>(g, g_numel, table, seg_lo, n, n_chunks, clip_value, grad_scale, full_model, norms, coefs, part, st);
  if (norm_kind == NORM_L1) return clip_launch<NORM_L1>(g, g_numel, table, seg_lo, n, n_chunks, clip_value, grad_scale, full_model, norms, coefs, part, st);
  return clip_launch<NORM_INF>(g, g_numel, table, seg_lo, n, n_chunks, clip_value, grad_scale, full_model, norms, coefs, part, st);
}

// ---------------------------------------------------------------------------------------------------
// unit_sgd_step: gs = g * grad_scale ; gc = clip(gs) ; d = gc + wd * p ; b = momentum * b + d (first step: b = d) ;
//                p -= lr * (nesterov ? d + momentum * b : b)          -- unit_sgd_momentum's arithmetic when nothing is switched on
// ---------------------------------------------------------------------------------------------------
#define CLIP_NONE 0
#define CLIP_VALUE 1
#define CLIP_COEF 2

// last row whose offset is <= idx, -1 if none (the offsets ascend)
__device__ __forceinline__ int clip_find_row(const long* __restrict__ table, int n_seg, long idx) {
  int l = 0, h = n_seg;
  while (l < h) {
    int m = (l + h) >> 1;
    if (table[2 * (long)m] <= idx) l = m + 1; else h = m;
  }
  return l - 1;
}
// the coefficient of flat element idx: its tensor's, 1 for padding
__device__ __forceinline__ float clip_coef_at(const long* __restrict__ table, int n_seg, const float* __restrict__ coefs, long idx) {
  int r = clip_find_row(table, n_seg, idx);
  return (r >= 0 && idx < table[2 * (long)r] + table[2 * (long)r + 1]) ? coefs[r] : 1.f;
}

template <int MODE>
__device__ __forceinline__ void sgd_step_elem(float& p, float g, float& b, float coef, float lr, float momentum, float wd, float grad_scale,
                                              float clip_value, int first, int nesterov) {
  float x = g * grad_scale;
  if (MODE == CLIP_VALUE) x = x > clip_value ? clip_value : (x < -clip_value ? -clip_value : x);          // (NaN stays NaN)
  if (MODE == CLIP_COEF) x = x * coef;
  float d = x + wd * p;
  float nb = first ? d : momentum * b + d;
  b = nb;
  p = p - lr * (nesterov ? d + momentum * nb : nb);
}

// p, g, buf point at flat element `lo`; 16-byte aligned. One 4-element vector per lane, 1024 elements per workgroup. Coefficient mode: the
// workgroup's first element is looked up with wave-uniform loads; a workgroup that lies inside one tensor (nearly all of them: the large
// tensors hold nearly all elements) is done with that, the others search per vector, and per element where a vector crosses a border.
template <int MODE>
__global__ void __launch_bounds__(256) sgd_step_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf, long lo, long n,
                                                       float lr, float momentum, float wd, float grad_scale, float clip_value, int first,
                                                       int nesterov, const long* __restrict__ table, int n_seg,
                                                       const float* __restrict__ coefs, const float* __restrict__ lr_dev) {
  const long e0 = (long)blockIdx.x * 1024;
  const long i = e0 + (long)threadIdx.x * 4;
  float cu = 1.f;
  bool uniform = MODE != CLIP_COEF;
  if (MODE == CLIP_COEF) {
    const long b1 = lo + (e0 + 1024 < n ? e0 + 1024 : n);
    const int r = clip_find_row(table, n_seg, lo + e0);
    if (r >= 0 && b1 <= table[2 * (long)r] + table[2 * (long)r + 1]) { uniform = true; cu = coefs[r]; }
  }
  if (i >= n) return;
  if (lr_dev) lr = lr * *lr_dev;
  if (i + 4 <= n) {
    float c[4] = {cu, cu, cu, cu};
    if (!uniform) {
      const int r = clip_find_row(table, n_seg, lo + i);
      if (r >= 0 && lo + i + 4 <= table[2 * (long)r] + table[2 * (long)r + 1]) c[0] = c[1] = c[2] = c[3] = coefs[r];
      else for (int j = 0; j < 4; ++j) c[j] = clip_coef_at(table, n_seg, coefs, lo + i + j);
    }
    f32x4 pv = *reinterpret_cast<f32x4*>(p + i), gv = *reinterpret_cast<const f32x4*>(g + i);
    f32x4 bv = *reinterpret_cast<f32x4*>(buf + i);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float pj = pv[j], bj = bv[j];
      sgd_step_elem<MODE>(pj, gv[j], bj, c[j], lr, momentum, wd, grad_scale, clip_value, first, nesterov);
      pv[j] = pj; bv[j] = bj;
    }
    *reinterpret_cast<f32x4*>(p + i) = pv; *reinterpret_cast<f32x4*>(buf + i) = bv;
  } else {
    for (long j = i; j < n; ++j) {
      float c = uniform ? cu : clip_coef_at(table, n_seg, coefs, lo + j);
      sgd_step_elem<MODE>(p[j], g[j], buf[j], c, lr, momentum, wd, grad_scale, clip_value, first, nesterov);
    }
  }
}
// a range that starts inside a packed fused head (flat.py segments()): small, one element per lane
template <int MODE>
__global__ void __launch_bounds__(256) sgd_step_scalar_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf, long lo, long n,
                                                              float lr, float momentum, float wd, float grad_scale, float clip_value, int first,
                                                              int nesterov, const long* __restrict__ table, int n_seg,
                                                              const float* __restrict__ coefs, const float* __restrict__ lr_dev) {
  const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  if (lr_dev) lr = lr * *lr_dev;
  float c = MODE == CLIP_COEF ? clip_coef_at(table, n_seg, coefs, lo + j) : 1.f;
  sgd_step_elem<MODE>(p[j], g[j], buf[j], c, lr, momentum, wd, grad_scale, clip_value, first, nesterov);
}

template <int MODE>
static int sgd_step_launch(float* p, const float* g, float* buf, long lo, long n, float lr, float momentum, float wd, float grad_scale,
                           float clip_value, int first, int nesterov, const long* table, int n_seg, const float* coefs, const float* lr_dev,
                           hipStream_t st) {
  if (((uintptr_t)p % 16) || ((uintptr_t)g % 16) || ((uintptr_t)buf % 16))
    sgd_step_scalar_kernel<MODE><<<cdiv(n, 256), 256, 0, st>>>(p, g, buf, lo, n, lr, momentum, wd, grad_scale, clip_value, first, nesterov, table,
                                                                n_seg, coefs, lr_dev);
  else
    sgd_step_kernel<MODE><<<cdiv(n, 1024), 256, 0, st>>>(p, g, buf, lo, n, lr, momentum, wd, grad_scale, clip_value, first, nesterov, table, n_seg,
                                                         coefs, lr_dev);
  UNIT_LAUNCH_CHECK();
  return UNIT_OK;
}

extern "C" int unit_sgd_step(float* p, const float* g, float* buf, long lo, long n, float lr, float momentum, float wd, float grad_scale,
                             float clip_value, int first_step, int nesterov, int clip_mode, const long* table, int n_seg, const float* coefs,
                             const float* lr_dev, void* stream) {
  if (n == 0) return UNIT_OK;
  UNIT_CHECK_ARG(p && g && buf && lo >= 0 && n > 0, "sgd_step: null pointer or negative range");
  UNIT_CHECK_ARG(((uintptr_t)p % 4 == 0) && ((uintptr_t)g % 4 == 0) && ((uintptr_t)buf % 4 == 0), "sgd_step: 4B alignment");
  UNIT_CHECK_ARG(clip_mode == CLIP_NONE || clip_mode == CLIP_VALUE || clip_mode == CLIP_COEF, "sgd_step: clip_mode must be 0, 1 or 2");
  UNIT_CHECK_ARG(clip_mode != CLIP_COEF || (table && coefs && n_seg >= 0 && (uintptr_t)table % 8 == 0), "sgd_step: coefficient mode needs the table and coefs");
  hipStream_t st = (hipStream_t)stream;
  p += lo; g += lo; buf += lo;
  if (clip_mode == CLIP_COEF)
    return sgd_step_launch<CLIP_COEF>(p, g, buf, lo, n, lr, momentum, wd, grad_scale, clip_value, first_step, nesterov, table, n_seg, coefs, lr_dev, st);
  if (clip_mode == CLIP_VALUE)
    return sgd_step_launch<CLIP_VALUE>(p, g, buf, lo, n, lr, momentum, wd, grad_scale, clip_value, first_step, nesterov, table, n_seg, coefs, lr_dev, st);
  return sgd_step_launch<CLIP_NONE>(p, g, buf, lo, n, lr, momentum, wd, grad_scale, clip_value, first_step, nesterov, table, n_seg, coefs, lr_dev, st);
}

// ---------------------------------------------------------------------------------------------------
// unit_sgd_step_masked: unit_sgd_step, but an element whose table row r has live[r] == 0 is neither read-modify-written nor stored: p and
// buf keep their bits whatever g holds. Elements of live rows and padding elements (no row) get unit_sgd_step's result bit for bit
// (the same sgd_step_elem). A dead tensor needs no first-step flag of its own: the momentum buffer starts at zero, and
// momentum * 0 + d == d is `first ? d : ...` on whichever step the tensor first becomes live.
// ---------------------------------------------------------------------------------------------------
// the table row that holds flat element idx, -1 for a padding element
__device__ __forceinline__ int clip_row_at(const long* __restrict__ table, int n_seg, long idx) {
  int r = clip_find_row(table, n_seg, idx);
  return (r >= 0 && idx < table[2 * (long)r] + table[2 * (long)r + 1]) ? r : -1;
}

// same geometry as sgd_step_kernel. A workgroup inside one dead tensor returns after two wave-uniform loads (its bytes are never moved);
// a vector inside one tensor takes that tensor's flag and coefficient; a vector that crosses a border is looked up per element, and
// stored as a vector only when all four elements are updated -- otherwise element by element, the dead ones skipped.
template <int MODE>
__global__ void __launch_bounds__(256) sgd_step_masked_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf, long lo,
                                                              long n, float lr, float momentum, float wd, float grad_scale, float clip_value,
                                                              int first, int nesterov, const long* __restrict__ table, int n_seg,
                                                              const float* __restrict__ coefs, const unsigned char* __restrict__ live,
                                                              const float* __restrict__ lr_dev) {
  const long e0 = (long)blockIdx.x * 1024;
  const long i = e0 + (long)threadIdx.x * 4;
  float cu = 1.f;
  bool uniform = false;
  {
    const long b1 = lo + (e0 + 1024 < n ? e0 + 1024 : n);
    const int r = clip_find_row(table, n_seg, lo + e0);
    if (r >= 0 && b1 <= table[2 * (long)r] + table[2 * (long)r + 1]) {
      if (!live[r]) return;
      uniform = true;
      if (MODE == CLIP_COEF) cu = coefs[r];
    }
  }
  if (i >= n) return;
  if (lr_dev) lr = lr * *lr_dev;
  float c[4] = {cu, cu, cu, cu};
  bool on[4] = {true, true, true, true};
  const int cnt = i + 4 <= n ? 4 : (int)(n - i);
  if (!uniform) {
    const int r = clip_find_row(table, n_seg, lo + i);
    if (r >= 0 && lo + i + cnt <= table[2 * (long)r] + table[2 * (long)r + 1]) {
      if (!live[r]) return;
      if (MODE == CLIP_COEF) c[0] = c[1] = c[2] = c[3] = coefs[r];
    } else {
      for (int j = 0; j < cnt; ++j) {
        const int rj = clip_row_at(table, n_seg, lo + i + j);
        on[j] = rj < 0 || live[rj] != 0;
        if (MODE == CLIP_COEF) c[j] = rj >= 0 ? coefs[rj] : 1.f;
      }
    }
  }
  if (cnt == 4 && on[0] && on[1] && on[2] && on[3]) {
    f32x4 pv = *reinterpret_cast<f32x4*>(p + i), gv = *reinterpret_cast<const f32x4*>(g + i);
    f32x4 bv = *reinterpret_cast<f32x4*>(buf + i);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float pj = pv[j], bj = bv[j];
      sgd_step_elem<MODE>(pj, gv[j], bj, c[j], lr, momentum, wd, grad_scale, clip_value, first, nesterov);
      pv[j] = pj; bv[j] = bj;
    }
    *reinterpret_cast<f32x4*>(p + i) = pv; *reinterpret_cast<f32x4*>(buf + i) = bv;
  } else {
    for (int j = 0; j < cnt; ++j)
      if (on[j]) sgd_step_elem<MODE>(p[i + j], g[i + j], buf[i + j], c[j], lr, momentum, wd, grad_scale, clip_value, first, nesterov);
  }
}
// unaligned base pointers: one element per lane
template <int MODE>
__global__ void __launch_bounds__(256) sgd_step_masked_scalar_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf,
                                                                     long lo, long n, float lr, float momentum, float wd, float grad_scale,
                                                                     float clip_value, int first, int nesterov, const long* __restrict__ table,
                                                                     int n_seg, const float* __restrict__ coefs,
                                                                     const unsigned char* __restrict__ live, const float* __restrict__ lr_dev) {
  const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const int r = clip_row_at(table, n_seg, lo + j);
  if (r >= 0 && !live[r]) return;
  if (lr_dev) lr = lr * *lr_dev;
  float c = (MODE == CLIP_COEF && r >= 0) ? coefs[r] : 1.f;
  sgd_step_elem<MODE>(p[j], g[j], buf[j], c, lr, momentum, wd, grad_scale, clip_value, first, nesterov);
}

template <int MODE>
static int sgd_step_masked_launch(float* p, const float* g, float* buf, long lo, long n, float lr, float momentum, float wd, float grad_scale,
                                  float clip_value, int first, int nesterov, const long* table, int n_seg, const float* coefs,
                                  const unsigned char* live, const float* lr_dev, hipStream_t st) {
  if (((uintptr_t)p % 16) || ((uintptr_t)g % 16) || ((uintptr_t)buf % 16))
    sgd_step_masked_scalar_kernel<MODE><<<cdiv(n, 256), 256, 0, st>>>(p, g, buf, lo, n, lr, momentum, wd, grad_scale, clip_value, first, nesterov,
                                                                       table, n_seg, coefs, live, lr_dev);
  else
    sgd_step_masked_kernel<MODE><<<cdiv(n, 1024), 256, 0, st>>>(p, g, buf, lo, n, lr, momentum, wd, grad_scale, clip_value, first, nesterov, table,
                                                                n_seg, coefs, live, lr_dev);
  UNIT_LAUNCH_CHECK();
  return UNIT_OK;
}

extern "C" int unit_sgd_step_masked(float* p, const float* g, float* buf, long lo, long n, float lr, float momentum, float wd, float grad_scale,
                                    float clip_value, int first_step, int nesterov, int clip_mode, const long* table, int n_seg,
                                    const float* coefs, const unsigned char* live, const float* lr_dev, void* stream) {
  UNIT_CHECK_ARG(live && table && (uintptr_t)table % 8 == 0, "sgd_step_masked: needs the table and one live byte per row of it");
  UNIT_CHECK_ARG(n_seg > 0, "sgd_step_masked: n_seg must be the table's (and the mask's) row count, > 0");
  if (n == 0) return UNIT_OK;
  UNIT_CHECK_ARG(p && g && buf && lo >= 0 && n > 0, "sgd_step_masked: null pointer or negative range");
  UNIT_CHECK_ARG(((uintptr_t)p % 4 == 0) && ((uintptr_t)g % 4 == 0) && ((uintptr_t)buf % 4 == 0), "sgd_step_masked: 4B alignment");
  UNIT_CHECK_ARG(clip_mode == CLIP_NONE || clip_mode == CLIP_VALUE || clip_mode == CLIP_COEF, "sgd_step_masked: clip_mode must be 0, 1 or 2");
  UNIT_CHECK_ARG(clip_mode != CLIP_COEF || coefs, "sgd_step_masked: coefficient mode needs coefs");
  hipStream_t st = (hipStream_t)stream;
  p += lo; g += lo; buf += lo;
  if (clip_mode == CLIP_COEF)
    return sgd_step_masked_launch<CLIP_COEF>(p, g, buf, lo, n, lr, momentum, wd, grad_scale, clip_value, first_step, nesterov, table, n_seg, coefs, live, lr_dev, st);
  if (clip_mode == CLIP_VALUE)
    return sgd_step_masked_launch<CLIP_VALUE>(p, g, buf, lo, n, lr, momentum, wd, grad_scale, clip_value, first_step, nesterov, table, n_seg, coefs, live, lr_dev, st);
  return sgd_step_masked_launch<CLIP_NONE>(p, g, buf, lo, n, lr, momentum, wd, grad_scale, clip_value, first_step, nesterov, table, n_seg, coefs, live, lr_dev, st);
}
