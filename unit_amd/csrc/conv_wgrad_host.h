// conv_wgrad_host.h -- host side of every weight-gradient launch: THE per-layer decision (kernel family, staging step, split-M slabs:
// wgrad_select), THE fill of the kernels' argument block (wgrad_fill) and what the planner of the grouped launches (conv_wgrad_plan.hip)
// exposes to the file that launches them (conv_wgrad.hip). Nothing in here launches and every extern below is defined in
// conv_wgrad_plan.hip, which holds no kernel: a host-only program links against that one file (tools/wgrad_plan_check.hip does, under
// sanitizers). A new field of Wgrad256Args is derived in wgrad_fill and nowhere else; a new rule of the decision goes into wgrad_select,
// which is what the workspace / split queries and the launches all ask.
#pragma once
#include "conv_wgrad256.h"

// does the 256x256 tile handle a shape, and with how many split-M slabs
extern "C" int unit_wgrad_use_big(int in_dtype, long M, int K, int C, int RS);
extern "C" int unit_wgrad_big_splits(long M, int tiles, int R, int S, int OHW);

// 128x128 tile: the LDS-DMA ring kernel (conv_wgrad128r.hip) where it applies (bf16, C % 128 == 0, K % 128 == 0), variant 4 = the
// register-staged kernel (conv_wgrad.hip) everywhere. Isolated the two are equal on the backbone shapes (tools/wgrad128_bench.py: 18.2 vs 18.5 us,
// 31.9 vs 30.4 us; RPN 3x3 306 vs 284 us -- at M = 9 576 these launches are bound by their fp32 slab store and input streaming, not by
// the loop's load latency); inside the step the ring form is 0.05-0.1 ms ahead on the same box (18.36 vs 18.44-18.48 ms).
inline int choose_splits(int M, int tiles, int ms) {
  // 2 workgroups of this kernel are co-resident per CU (72 KB LDS each): 512 slots per "round" on 256 CUs. Pick the
  // split count whose grid fills whole rounds best (tile quantisation), preferring fewer splits (less slab traffic).
  // Cost model (us), fitted to tools/microbench.py on the res3/res4/RPN shapes: a workgroup needs ~4 us of fixed time
  // (launch ramp, first loads, slab store) plus ~1.0 us per staged 64-row step (operand-feed bound at this tile); the
  // grid runs in rounds of 512 workgroups; every split writes one fp32 slab of the whole dW (64 KB per tile) that the
  // reduction reads back: ~2 x 64 KB per tile and split at ~4 TB/s.
  int maxs = (M + 4 * ms - 1) / (4 * ms);   // at least 4 staged steps per split
  if (maxs < 1) maxs = 1;
  if (maxs > 64) maxs = 64;
  int best = 1; double best_cost = 1e30;
  double steps_total = (double)((M + ms - 1) / ms);
  for (int s = 1; s <= maxs; ++s) {
    long blocks = (long)tiles * s;
    long rounds = (blocks + 511) / 512;
    double per_block = 4.0 + 1.0 * (steps_total / s) * (ms / 64.0);
    double slab = (double)blocks * 2.0 * 65536.0 / 4.0e6;      // bytes / (4 TB/s) in us
    double cost = rounds * per_block + slab;
    if (cost < best_cost) { best_cost = cost; best = s; }
  }
  return best;
}

enum WgradFamily { WGRAD_REG = 0, WGRAD_RING128 = 1, WGRAD_BIG = 2 };   // register-staged 128 tile / LDS-DMA ring 128 tile / the 256 tile's kernels
struct WgradChoice {
  int family;
  int tile;      // edge of a workgroup's k x n tile: 128 / 256
  int ms;        // pixels per staged step: 64 (bf16) / 32 (fp32)
  int splits;    // split-M slabs the launch writes = K*R*S*C floats each in the workspace
};

// what unit_conv2d_wgrad's policy runs for a layer. force_big: the 256 tile whatever the policy says (unit_conv2d_wgrad_big_launch).
inline WgradChoice wgrad_select(int in_dtype, int N, int OH, int OW, int K, int R, int S, int C, bool force_big = false) {
  long M = (long)N * OH * OW;
  int Kgemm = R * S * C;
  if (force_big || unit_wgrad_use_big(in_dtype, M, K, C, R * S))
    return WgradChoice{WGRAD_BIG, 256, 64, unit_wgrad_big_splits(M, (Kgemm / 256) * (K / 256), R, S, OH * OW)};
  int ms = in_dtype == UNIT_BF16 ? 64 : 32;
  bool ring = in_dtype == UNIT_BF16 && C % 128 == 0 && K % 128 == 0;
  return WgradChoice{ring ? WGRAD_RING128 : WGRAD_REG, 128, ms, choose_splits((int)M, cdiv(Kgemm, 128) * cdiv(K, 128), ms)};
}

// Every field of the argument block from the layer's geometry. x_pitch: elements per pixel row of x; x_span / dy_span: bytes from x / dy
// to the end of their tensors (the buffer range of the loads; `too_large` = the caller's error string past 4 GiB); tile / ms / splits as
// in WgradChoice. valid_only = 0: the callers that may contract over in-map pixels only set it by their own rule.
inline int wgrad_fill(Wgrad256Args& a, const char* too_large, const void* x, const void* dy, float* partial, int N, int H, int W, int C, int K,
                      int R, int S, int stride, int pad, int OH, int OW, int ldy, int x_pitch, size_t x_span, size_t dy_span, int tile, int ms,
                      int splits) {
  a.x = x; a.dy = dy; a.partial = partial; a.x_pitch = x_pitch;
  a.N = N; a.H = H; a.W = W; a.C = C; a.K = K; a.R = R; a.S = S; a.stride = stride; a.pad = pad; a.OH = OH; a.OW = OW;
  a.ldy = ldy; a.Kgemm = R * S * C; a.M = N * OH * OW;
  UNIT_CHECK_ARG(x_span < 0xFFFFFFF0ull && dy_span < 0xFFFFFFF0ull, too_large);
  a.x_bytes = (unsigned)x_span; a.dy_bytes = (unsigned)dy_span;
  // m -> (n, oh, ow) by multiply-high: q = umulhi(m, ceil(2^32 / d)) is exact while m * d < 2^32 (else the kernels divide), one correction;
  // for d == 1 the quotient is m itself: magic 0xFFFFFFFF gives m - 1 for m > 0 and the correction fixes it
  a.OHW = OH * OW;
  a.use_magic = ((unsigned long long)(a.M + 64) * (unsigned long long)a.OHW < 0xFFFFFFFFull) ? 1 : 0;
  a.magic_ohw = a.OHW > 1 ? (unsigned)((0x100000000ull + a.OHW - 1) / (unsigned long long)a.OHW) : 0xFFFFFFFFu;
  a.magic_ow = OW > 1 ? (unsigned)((0x100000000ull + OW - 1) / (unsigned long long)OW) : 0xFFFFFFFFu;
  a.tiles_k = cdiv(a.Kgemm, tile); a.tiles_n = cdiv(K, tile);
  a.splits = splits;
  a.m_per_split = cdiv(cdiv(a.M > 0 ? a.M : 1, splits), ms) * ms;
  a.valid_only = 0;
  return UNIT_OK;
}

// THE rule for "contract over in-map pixels only" (Wgrad256Args::valid_only): a 3x3 s1 p1 "same" conv on a small map. Asked by the 256
// tile's policy (conv_wgrad256.hip) and by the grouped launches' fill; the grouped launches' units follow the flag.
inline bool wgrad_valid_only(const Wgrad256Args& a) {
  return a.R == 3 && a.S == 3 && a.stride == 1 && a.pad == 1 && a.OH == a.H && a.OW == a.W && a.OHW <= 512;
}

// ---- grouped launches: the planner (conv_wgrad_plan.hip) ------------------------------------------------------------------------------
// mirrors include/unit_hip.h
struct UnitWgradProblem {
  const void* x; const void* dy; void* partial;
  int N, H, W, C, K, R, S, stride, pad, OH, OW, ldy;
  int splits, kind;
  int x_pitch;            // 0 = C; one pass of a bf16x3 weight gradient: 2 * C (x, dy point at the pass's planes, ldy = 2 * K), x_back / dy_back =
  int x_back, dy_back;    // elements between the tensor's start and the x / dy pointer (0 or one plane: keeps the loads' buffer range exact)
};

// every launch of the problems' grids in order -- the 256-tile kind first, per kind as many launches as WG_GROUP_MAX_PROBLEMS and the unit
// table need: `each` gets the filled kernel argument (layer blocks + unit table), the tile kind, the workgroup slots of the fullest XCD
// (grid = 8 x that) and, per layer block, its index into pr. Stops at the first status != UNIT_OK and returns it. Reads the dealing
// switches (UNIT_WGRAD_GANG / UNIT_WGRAD_DEAL) once per call.
typedef int (*WgradLaunchFn)(void* ctx, const WgradGroupArgs& g, int kind, int slots_per_xcd, const int* pidx);
int wgrad_group_each_launch(const UnitWgradProblem* pr, int n, WgradLaunchFn each, void* ctx);
