// conv_wgrad_plan.hip -- the weight gradients' host-only decisions: which tile and how many split-M slabs a layer gets, and the planner of
// the grouped launches (include/unit_hip.h: unit_conv2d_wgrad_group): split counts per layer, problems packed into launches, their units
// enumerated, formed into gangs and dealt to the 8 XCDs. No kernel and no launch in this file: everything runs without a GPU
// (unit_conv2d_wgrad_group_layout; tools/wgrad_plan_check.hip links this file alone and runs it under sanitizers).
// Below wgrad_deal_options() every function depends on its arguments only (and on the table cache, which holds shapes -> tables).
#include <math.h>
#include <stdlib.h>
#include <algorithm>
#include "conv_wgrad_host.h"

// ---- the 256x256 tile: which shapes, how many slabs -----------------------------------------------------------------------------------
extern "C" int unit_wgrad_use_big(int in_dtype, long M, int K, int C, int RS) {
  if (in_dtype != UNIT_BF16 || (C % 256) != 0 || (K % 256) != 0) return 0;
  // few pixels need many tiles: with >= 96 tiles (RPN 3x3 1024->1024 on 4 images: 144) two or three split-M slabs fill the chip
  // and each workgroup still runs >= 50 steps; the backbone layers (4-16 tiles) would need ~64 slabs of 2-3 steps each
  long tiles = (long)(RS * C / 256) * (K / 256);
  return M >= 16384 || (M >= 8192 && tiles >= 96);
}

// 3x3 convs on small maps get one spare slab: the valid-only contraction of conv_wgrad256p8.hip deals its workgroups to the filter
// taps unevenly (Wgrad256Args::valid_only); where that path does not apply the spare is simply one more split.
// Weaker than wgrad_valid_only ON PURPOSE: no stride, pad or same-size condition -- a split count is wanted before the launch knows
// them, and tests/golden/wgrad_select_golden.json pins the counts this rule gives.
extern "C" int unit_wgrad_big_splits_base(long M, int tiles);
extern "C" int unit_wgrad_big_splits(long M, int tiles, int R, int S, int OHW) {
  int s = unit_wgrad_big_splits_base(M, tiles);
  return (R == 3 && S == 3 && OHW <= 512) ? s + 1 : s;
}

extern "C" int unit_wgrad_big_splits_base(long M, int tiles) {
  // one workgroup per CU (128 KB of LDS): 256 slots per round; >= 8 staged steps per split. Cost model (us): a workgroup
  // needs ~6 us of fixed time plus ~1.3 us per 64-pixel step; the grid runs in rounds of 256 workgroups; every workgroup
  // writes a 256 KB fp32 slab that the reduction reads back (~2 x 256 KB at ~4 TB/s).
  int maxs = (int)((M + 8 * 64 - 1) / (8 * 64));
  if (maxs < 1) maxs = 1;
  if (maxs > 64) maxs = 64;
  int best = 1; double best_cost = 1e30;
  double steps_total = (double)((M + 63) / 64);
  for (int s = 1; s <= maxs; ++s) {
    long blocks = (long)tiles * s;
    long rounds = (blocks + 255) / 256;
    double cost = rounds * (6.0 + 1.3 * steps_total / s) + (double)blocks * 2.0 * 262144.0 / 4.0e6;
    if (cost < best_cost) { best_cost = cost; best = s; }
  }
  return best;
}

// ---- grouped launches (conv_wgrad128r.hip: conv_wgrad128_group_kernel; conv_wgrad256p8.hip: conv_wgrad256_group_kernel) -------------
extern "C" size_t unit_wgrad_problem_bytes(void) { return sizeof(UnitWgradProblem); }

// 0 = not eligible; 1 = 128x128 ring tiles; 2 = 256x256 phase-interleaved tiles (half the operand bytes per flop; needs enough pixels
// for a few 64-pixel steps per split)
extern "C" int unit_conv2d_wgrad_group_supported(int in_dtype, int N, int OH, int OW, int K, int R, int S, int C) {
  if (in_dtype != UNIT_BF16 || (C % 128) != 0 || (K % 128) != 0) return 0;
  long M = (long)N * OH * OW;
  if (M <= 0 || M > 0x7FFFFFFFl) return 0;
  if ((C % 256) == 0 && (K % 256) == 0 && M >= 2048 && (R * S * C / 256) * (K / 256) <= 4096) return 2;
  if ((R * S * C / 128) * (K / 128) > 4096) return 0;
  return 1;
}

// split counts of the layers of a grouped launch, per tile kind. All workgroups of a grid should run about the same number of pixels, so
// layer p gets s_p ~ s_ref * M_p / M_max slabs;
//  kind 1 (two workgroups per CU): s_ref from choose_splits()'s cost model over the whole grid: rounds of 512 slots, ~4 us fixed + ~1 us
//  per 64 pixels per workgroup, two transfers of every workgroup's 64 KB slab tile at ~4 TB/s;
//  kind 2 (one per CU): rounds of 256 slots with the constants measured below.
extern "C" int unit_conv2d_wgrad_group_plan(UnitWgradProblem* pr, int n, int splits_hint) {
  UNIT_CHECK_ARG(pr != nullptr && n > 0, "wgrad_group_plan: no problems");
  for (int i = 0; i < n; ++i) {
    pr[i].kind = unit_conv2d_wgrad_group_supported(UNIT_BF16, pr[i].N, pr[i].OH, pr[i].OW, pr[i].K, pr[i].R, pr[i].S, pr[i].C);
    UNIT_CHECK_ARG(pr[i].kind != 0, "wgrad_group_plan: layer not eligible (unit_conv2d_wgrad_group_supported)");
  }
  // a few 256x256 tiles alone cannot fill 256 CUs with long loops (res3's one 256 -> 512 shortcut: 2 tiles): they join the 128x128 grid
  long tiles2 = 0;
  for (int i = 0; i < n; ++i)
    if (pr[i].kind == 2) tiles2 += (long)(pr[i].R * pr[i].S * pr[i].C / 256) * (pr[i].K / 256);
  if (tiles2 < 16)
    for (int i = 0; i < n; ++i)
      if (pr[i].kind == 2) pr[i].kind = 1;
  for (int kind = 1; kind <= 2; ++kind) {
    long mmax = 0;
    for (int i = 0; i < n; ++i)
      if (pr[i].kind == kind) { long M = (long)pr[i].N * pr[i].OH * pr[i].OW; if (M > mmax) mmax = M; }
    if (mmax == 0) continue;
    const int T = kind == 2 ? 256 : 128;
    auto splits_of = [&](int i, int sref) {
      long M = (long)pr[i].N * pr[i].OH * pr[i].OW;
      long s = (M * sref + mmax / 2) / mmax;
      long maxs = (M + 255) / 256;              // >= 4 staged 64-pixel steps per split
      if (s > maxs) s = maxs;
      if (s < 1) s = 1;
      if (s > 64) s = 64;
      return (int)s;
    };
    int best = 1;
    if (splits_hint > 0) best = splits_hint;
    else if (kind == 1) {
      double best_cost = 1e30;
      for (int sref = 1; sref <= 32; ++sref) {
        long wgs = 0;
        for (int i = 0; i < n; ++i)
          if (pr[i].kind == kind) wgs += (long)(pr[i].R * pr[i].S * pr[i].C / T) * (pr[i].K / T) * splits_of(i, sref);
        long rounds = (wgs + 511) / 512;
        double cost = rounds * (4.0 + 1.0 * ((double)mmax / sref) / 64.0) + (double)wgs * 2.0 * 65536.0 / 4.0e6;
        if (cost < best_cost) { best_cost = cost; best = sref; }
      }
    } else {
      // rounds of 256 workgroups (one per CU), each ~12 us of fixed time (launch ramp, first loads, 256 KB slab store) + ~2.2 us per
      // 64-pixel step when every CU streams. Fits tools/wgrad_group_bench.py within a few percent where the loops are short -- a res4
      // bucket (102 tiles, 150 steps): 315 / 177 / 219 / 176 / 191 / 209 us measured with 1 / 2 / 3 / 4 / 6 / 8 slabs per layer, model 342 /
      // 177 / 244 / 188 / 201 / 212; the RPN's 3x3 (144 tiles, 75 steps): 180 / 188 / 134 measured with 1 / 2 / 3, model 177 / 188 / 134.
      // For the long loops of a Res5 head (236 tiles, 784 steps) the model is flat (1.74-1.82 ms) while 3-8 slabs measured 5-8 % faster
      // than 1-2 (1.49-1.55 against 1.62 ms: units of 16-36 tiles quantise on an XCD's 32 CUs until there are several rounds of them).
      // At least 24 steps per workgroup.
      long tiles = 0;
      for (int i = 0; i < n; ++i)
        if (pr[i].kind == kind) tiles += (long)(pr[i].R * pr[i].S * pr[i].C / T) * (pr[i].K / T);
      double steps = (double)((mmax + 63) / 64), tmin = 1e30;
      int smax = (int)(steps / 24.0);
      if (smax < 1) smax = 1;
      if (smax > 64) smax = 64;
      // (a round counts as full at 90 % of its slots: the units are dealt to the XCDs by weight, not evenly by workgroup count)
      auto model = [&](int sref) { return ceil((double)(tiles * sref) / (0.9 * 256.0)) * (12.0 + 2.2 * steps / sref); };
      int argmin = 1;
      for (int sref = 1; sref <= smax; ++sref)
        if (model(sref) < tmin) { tmin = model(sref); argmin = sref; }
      // every slab is read back by the reduction (a Res5 head: 60 MB each): of the split counts within 3 % of the best, the SMALLEST that
      // still gives 2.5 rounds of workgroups (3 slabs per layer for a Res5 head: 1 522 us against 1 541 with 5); none such: the model's best
      best = argmin;
      for (int sref = smax; sref >= 1; --sref)
        if (model(sref) <= 1.03 * tmin && tiles * sref >= 640) best = sref;
    }
    for (int i = 0; i < n; ++i)
      if (pr[i].kind == kind) pr[i].splits = splits_of(i, best);
  }
  return UNIT_OK;
}

static int wgrad_group_fill(const UnitWgradProblem& q, Wgrad256Args& b) {
  const int T = q.kind == 2 ? 256 : 128;
  UNIT_CHECK_ARG(q.kind == 1 || q.kind == 2, "wgrad_group: kind 1 / 2 (unit_conv2d_wgrad_group_plan)");
  UNIT_CHECK_ARG(q.C % T == 0 && q.K % T == 0 && q.ldy % 8 == 0, "wgrad_group: C, K must be multiples of the tile, ldy of 8");
  UNIT_CHECK_ARG(((uintptr_t)q.x % 16 == 0) && ((uintptr_t)q.dy % 16 == 0) && ((uintptr_t)q.partial % 16 == 0) && q.partial != nullptr,
                 "wgrad_group: 16B alignment");
  UNIT_CHECK_ARG(q.splits >= 1 && q.splits <= WG_GROUP_MAX_SPLITS, "wgrad_group: splits 1..127 (unit_conv2d_wgrad_group_plan)");
  UNIT_CHECK_ARG(q.N * q.OH * q.OW > 0, "wgrad_group: empty problem");
  const int x_pitch = q.x_pitch > 0 ? q.x_pitch : q.C;
  UNIT_CHECK_ARG(x_pitch >= q.C && x_pitch % 8 == 0 && q.x_back >= 0 && q.dy_back >= 0, "wgrad_group: x_pitch / x_back / dy_back");
  int rc = wgrad_fill(b, "wgrad_group: operand larger than 4 GiB", q.x, q.dy, (float*)q.partial, q.N, q.H, q.W, q.C, q.K, q.R, q.S, q.stride, q.pad,
                      q.OH, q.OW, q.ldy, x_pitch, ((size_t)q.N * q.H * q.W * x_pitch - q.x_back) * 2,
                      ((size_t)q.N * q.OH * q.OW * q.ldy - q.dy_back) * 2, T, 64, q.splits);
  if (rc != UNIT_OK) return rc;
  b.valid_only = (q.kind == 2 && wgrad_valid_only(b)) ? 1 : 0;
  UNIT_CHECK_ARG(b.tiles_k * b.tiles_n <= 4096, "wgrad_group: more than 4096 tiles in one layer");
  return UNIT_OK;
}

// ---- the dealing switches -------------------------------------------------------------------------------------------------------------
// gangs (UNIT_WGRAD_GANG, profiles/r06_exp_wgrad_gangs.txt): the nine filter-tap units of one split of a valid_only 3x3 layer contract over the
// SAME x / dy rows; dealt one by one (0) they land on up to eight XCDs and every one of those L2s fetches the rows for itself.
// 1: all nine on one XCD (36 tiles on 32 CUs, and the taps drift apart: 36 / 42 / 49 valid positions per 7x7 image);
// 2 (default): the taps that walk at the same pace -- 4 corner, 4 edge, the centre tap -- form a gang: a Res5 head's grid 4.00 -> 2.67 GB past L2
// UNIT_WGRAD_DEAL: 0 = by summed weight alone (round 5), 1 = by makespan. Default: makespan for gangs, weight for single units (measured,
// isolated Res5-head grid: gangs 1 599 / 1 625 -> 1 564 / 1 588 us; single units 1 534 / 1 495 -> 1 643 / 1 611: the model's equal step time
// per tile is only roughly true)
struct WgradDealOptions { int gangs; bool by_makespan; };
static WgradDealOptions wgrad_deal_options() {          // read per call (a handful per step): the tests switch them in-process
  const char* gang_env = getenv("UNIT_WGRAD_GANG");
  const char* deal_env = getenv("UNIT_WGRAD_DEAL");
  const int gangs = gang_env ? atoi(gang_env) : 2;
  return WgradDealOptions{gangs, deal_env ? deal_env[0] != '0' : gangs != 0};
}

// ---- units ----------------------------------------------------------------------------------------------------------------------------
constexpr int WG_FIXED_STEPS = 6;          // a tile's fixed time in 64-pixel steps (~12 us against ~2.2 us per step, unit_conv2d_wgrad_group_plan)
constexpr int WG_LAUNCH_MAX_UNITS = 8 * WG_GROUP_MAX_UNITS;
struct WgradUnit {
  long w;                       // weight: tiles x pixels
  int p, tap, s, tiles, tile0;  // layer block of the launch, filter tap, split, tile count and first tile
  int gang; long gw;            // units that share an XCD where one has room, and their summed weight
  int d;                        // a tile's duration in 64-pixel steps
};

// units of a layer: one per split (x 9 filter taps for valid_only layers), each cut into chunks of at most one XCD's workgroup slots
// (32 CUs: one 256x256 workgroup or two 128x128 ones per CU) -- whole rows of k tiles (they share the dy columns) where a row fits
static int unit_chunk(int tiles_k, int tiles, int kind) {
  const int L = kind == 2 ? 32 : 64;
  if (tiles <= L + L / 4) return tiles;
  return tiles_k <= L ? tiles_k * (L / tiles_k) : L;
}

// THE enumeration of a filled layer block's units (p = its index in the launch), in the order (filter tap,) split, chunk: appended to
// us[*nu ...] with weight, duration and gang id (gangs / *ngang: wgrad_deal_options, the launch's running gang count; a lone unit gets
// -1); us == nullptr: counted only.
static int wgrad_units(const Wgrad256Args& a, int kind, int p, int gangs, int* ngang, WgradUnit* us, int* nu) {
  const int taps = a.valid_only ? 9 : 1, tiles_k = a.tiles_k / taps, per = tiles_k * a.tiles_n, ch = unit_chunk(tiles_k, per, kind);
  for (int tap = 0; tap < taps; ++tap) {
    const int kr = tap / 3, ks = tap % 3, cls = (kr != 1) + (ks != 1);            // pace class: 0 centre, 1 edge, 2 corner
    const long meff = (long)a.N * std::max(a.OH - (kr != 1), 0) * std::max(a.OW - (ks != 1), 0);      // 3x3 s1 p1 "same": the border taps lose a row / column
    for (int sp = 0; sp < a.splits; ++sp) {
      const int mb = sp * a.m_per_split, m = std::max(std::min(a.M, mb + a.m_per_split) - mb, 0);      // the split's pixels of a full contraction
      const long per_tile = a.valid_only ? meff / a.splits + 1 : m, rows = a.valid_only ? (meff + a.splits - 1) / a.splits : m;
      const int gang = !a.valid_only ? -1 : gangs == 1 ? *ngang + sp : gangs == 2 ? *ngang + sp * 3 + cls : -1;
      for (int t0 = 0; t0 < per; t0 += ch, ++*nu) {
        if (us == nullptr) continue;
        UNIT_CHECK_ARG(*nu < WG_LAUNCH_MAX_UNITS, "wgrad_group: more units than one grid holds");
        const int nt = std::min(per - t0, ch);
        us[*nu] = WgradUnit{nt * per_tile, p, tap, sp, nt, t0, gang, 0, (int)((rows + 63) / 64) + WG_FIXED_STEPS};
      }
    }
  }
  if (a.valid_only) *ngang += a.splits * 3;
  return UNIT_OK;
}
static int units_of(const Wgrad256Args& a, int kind) {
  int nu = 0, ngang = 0;
  (void)wgrad_units(a, kind, 0, 0, &ngang, nullptr, &nu);
  return nu;
}

// one launch: the next problems of this kind from *cursor on that fit WG_GROUP_MAX_PROBLEMS and the unit table, filled into g.p, their
// indices into pidx. Returns how many (0: none left) or a negative status.
static int next_launch(const UnitWgradProblem* pr, int n, int kind, int* cursor, WgradGroupArgs& g, int* pidx) {
  int cnt = 0, units = 0, i = *cursor;
  for (; i < n; ++i) {
    if (pr[i].kind != kind) continue;
    if (cnt == WG_GROUP_MAX_PROBLEMS) break;
    int rc = wgrad_group_fill(pr[i], g.p[cnt]);
    if (rc != UNIT_OK) return rc;
    int u = units_of(g.p[cnt], kind);
    if (units + u > WG_LAUNCH_MAX_UNITS) break;
    units += u;
    pidx[cnt++] = i;
  }
  UNIT_CHECK_ARG(cnt > 0 || i >= n, "wgrad_group: a layer with more units than one grid holds");
  *cursor = i;
  return cnt;
}

// the launch's units in dealing order: a gang is dealt as one item of its units' total weight, a lone unit is its own gang; gangs by
// descending weight, inside a gang the heaviest unit first (the centre tap: the units past an XCD's 32 workgroup slots start late, they
// should be the short ones). Insertion sort, stable (<= 192 entries).
static int wgrad_launch_units(const WgradGroupArgs& g, int cnt, int kind, int gangs, WgradUnit* us, int* nu) {
  int ngang = 0;
  *nu = 0;
  for (int p = 0; p < cnt; ++p) {
    int rc = wgrad_units(g.p[p], kind, p, gangs, &ngang, us, nu);
    if (rc != UNIT_OK) return rc;
  }
  for (int a = 0; a < *nu; ++a) {
    if (us[a].gang < 0) { us[a].gang = ngang++; us[a].gw = us[a].w; continue; }
    long t = 0;
    for (int b = 0; b < *nu; ++b) if (us[b].gang == us[a].gang) t += us[b].w;
    us[a].gw = t;
  }
  auto before = [](const WgradUnit& p, const WgradUnit& q) { return p.gw != q.gw ? p.gw > q.gw : p.gang != q.gang ? p.gang < q.gang : p.w > q.w; };
  for (int a = 1; a < *nu; ++a) {
    WgradUnit v = us[a]; int b = a - 1;
    while (b >= 0 && before(v, us[b])) { us[b + 1] = us[b]; --b; }
    us[b + 1] = v;
  }
  return UNIT_OK;
}

// ---- dealing: units (gangs of units), heaviest first, to XCDs that still have free unit entries ------------------------------------------
// unit u becomes the next entry of XCD x (unit_start[x][n_units[x]] is the XCD's running slot total; the table starts zeroed)
static int place(WgradUnitTable& t, int x, const WgradUnit& u) {
  UNIT_CHECK_ARG(x >= 0 && t.n_units[x] < WG_GROUP_MAX_UNITS, "wgrad_group: unit table full");
  int k = t.n_units[x]++, end = t.unit_start[x][k] + u.tiles;
  UNIT_CHECK_ARG(end < 65536, "wgrad_group: more than 65535 workgroups on one XCD");
  t.unit_code[x][k] = pack_unit_code(u.p, u.tap, u.s);
  t.unit_tile0[x][k] = (unsigned short)u.tile0;
  t.unit_start[x][k + 1] = (unsigned short)end;
  return UNIT_OK;
}

// every gang to the XCD with the least summed weight that has entries for all of it; none has: unit by unit
static int deal_by_weight(const WgradUnit* us, int nu, WgradUnitTable& t) {
  long load[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  int bx = -1;
  for (int a = 0; a < nu; ++a) {
    if (a == 0 || us[a].gang != us[a - 1].gang) {
      int need = 1;
      while (a + need < nu && us[a + need].gang == us[a].gang) ++need;
      bx = -1;
      for (int x = 0; x < 8; ++x)
        if (t.n_units[x] + need <= WG_GROUP_MAX_UNITS && (bx < 0 || load[x] < load[bx])) bx = x;
    }
    if (bx < 0 || t.n_units[bx] >= WG_GROUP_MAX_UNITS) {          // no XCD has room for the whole gang: unit by unit
      bx = -1;
      for (int x = 0; x < 8; ++x)
        if (t.n_units[x] < WG_GROUP_MAX_UNITS && (bx < 0 || load[x] < load[bx])) bx = x;
    }
    int rc = place(t, bx, us[a]);
    if (rc != UNIT_OK) return rc;
    load[bx] += us[a].w;
  }
  return UNIT_OK;
}

// list-scheduling makespan on an XCD's 32 CUs of its nx units list[] plus us[a0 .. a0 + na), both longest tiles first
static int xcd_makespan(const WgradUnit* us, const int* list, int nx, int a0, int na) {
  int cu[32] = {0};
  int ia = 0, ib = 0, worst = 0;
  while (ia < nx || ib < na) {
    const WgradUnit& v = (ib >= na || (ia < nx && us[list[ia]].d >= us[a0 + ib].d)) ? us[list[ia++]] : us[a0 + ib++];
    for (int t = 0; t < v.tiles; ++t) {
      int m = 0;
      for (int c = 1; c < 32; ++c) if (cu[c] < cu[m]) m = c;
      cu[m] += v.d;
      if (cu[m] > worst) worst = cu[m];
    }
  }
  return worst;
}

// 256-tiles, one workgroup per CU: an XCD's 32 CUs take its slots in order, so what ends the grid is the XCD's list-scheduling makespan,
// not its summed weight (a Res5 head: 2.7 rounds of tiles that last 265 / 228 / 196 steps -- dealt by weight alone the 16-tile gangs cost
// 798 steps on the slowest XCD against 728, profiles/r06_exp_wgrad_gangs.txt). Every gang goes to the XCD whose makespan with it is the
// shortest (then the lighter one), an XCD's units run longest-first. Costs ~4 ms for a Res5 head's 100 units: the tables are cached.
static int deal_by_makespan(WgradUnit* us, int nu, WgradUnitTable& t) {
  static thread_local int xl[8][WG_GROUP_MAX_UNITS];          // per XCD: its units (indices into us), longest first
  int nx[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  long load[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int a = 0; a < nu;) {
    int need = 1;
    while (a + need < nu && us[a + need].gang == us[a].gang) ++need;
    for (int b = a + 1; b < a + need; ++b) {             // the gang's units longest first (they are merged into sorted lists)
      WgradUnit v = us[b]; int c = b - 1;
      while (c >= a && us[c].d < v.d) { us[c + 1] = us[c]; --c; }
      us[c + 1] = v;
    }
    int bx = -1, bm = 0, take = need;
    for (;;) {
      for (int x = 0; x < 8; ++x) {
        if (nx[x] + take > WG_GROUP_MAX_UNITS) continue;
        int m = xcd_makespan(us, xl[x], nx[x], a, take);
        if (bx < 0 || m < bm || (m == bm && load[x] < load[bx])) { bx = x; bm = m; }
      }
      if (bx >= 0 || take == 1) break;
      take = 1;                                          // no XCD has entries for the whole gang: unit by unit
    }
    UNIT_CHECK_ARG(bx >= 0, "wgrad_group: unit table full");
    for (int b = a; b < a + take; ++b) {                 // merge into the XCD's list, longest first, a gang's units adjacent
      int k = nx[bx]++;
      while (k > 0 && us[xl[bx][k - 1]].d < us[b].d) { xl[bx][k] = xl[bx][k - 1]; --k; }
      xl[bx][k] = b;
      load[bx] += us[b].w;
    }
    a += take;
  }
  for (int x = 0; x < 8; ++x)
    for (int k = 0; k < nx[x]; ++k) {
      int rc = place(t, x, us[xl[x][k]]);
      if (rc != UNIT_OK) return rc;
    }
  return UNIT_OK;
}

// ---- the last few launches' tables: the makespan rule depends on shapes only ------------------------------------------------------------
struct WgradTableKey { int v[3 + 12 * WG_GROUP_MAX_PROBLEMS]; };          // zero-padded; all zero = an empty entry (no launch has kind 0)
struct WgradCachedTable { WgradTableKey key; WgradUnitTable t; };
static thread_local WgradCachedTable wgrad_cache[8];
static thread_local int wgrad_cache_next = 0;

static WgradTableKey table_key(const WgradGroupArgs& g, int cnt, int kind, int gangs) {
  WgradTableKey key = {{kind, cnt, gangs}};
  int n = 3;
  for (int p = 0; p < cnt; ++p) {
    const Wgrad256Args& a = g.p[p];
    for (int v : {a.N, a.H, a.W, a.C, a.K, a.R, a.S, a.stride, a.pad, a.OH, a.OW, a.splits}) key.v[n++] = v;
  }
  return key;
}
static const WgradUnitTable* cached_table(const WgradTableKey& key) {
  for (const WgradCachedTable& e : wgrad_cache)
    if (memcmp(&e.key, &key, sizeof(key)) == 0) return &e.t;
  return nullptr;
}

// the unit table of the launch whose cnt layer blocks are in g.p
static int wgrad_deal(WgradGroupArgs& g, int cnt, int kind, const WgradDealOptions& opt) {
  static thread_local WgradUnit us[WG_LAUNCH_MAX_UNITS];
  const bool by_makespan = kind == 2 && opt.by_makespan;          // which launches pay for the makespan rule -- and are therefore cached
  const WgradTableKey key = by_makespan ? table_key(g, cnt, kind, opt.gangs) : WgradTableKey{};
  if (const WgradUnitTable* hit = by_makespan ? cached_table(key) : nullptr) { g.t = *hit; return UNIT_OK; }
  int nu = 0;
  int rc = wgrad_launch_units(g, cnt, kind, opt.gangs, us, &nu);
  if (rc != UNIT_OK) return rc;
  g.t = WgradUnitTable{};
  rc = by_makespan ? deal_by_makespan(us, nu, g.t) : deal_by_weight(us, nu, g.t);
  if (rc != UNIT_OK) return rc;
  if (by_makespan) wgrad_cache[wgrad_cache_next++ & 7] = WgradCachedTable{key, g.t};
  return UNIT_OK;
}

int wgrad_group_each_launch(const UnitWgradProblem* pr, int n, WgradLaunchFn each, void* ctx) {
  static thread_local WgradGroupArgs g;         // 3.8 KB; filled here, passed to the kernels by value
  const WgradDealOptions opt = wgrad_deal_options();
  int pidx[WG_GROUP_MAX_PROBLEMS];
  for (int kind = 2; kind >= 1; --kind)           // the long 256-tile grid first
    for (int cursor = 0;;) {
      int cnt = next_launch(pr, n, kind, &cursor, g, pidx);
      if (cnt < 0) return cnt;
      if (cnt == 0) break;
      int rc = wgrad_deal(g, cnt, kind, opt);
      if (rc != UNIT_OK) return rc;
      int most = 0;
      for (int x = 0; x < 8; ++x)
        if (g.t.unit_start[x][g.t.n_units[x]] > most) most = g.t.unit_start[x][g.t.n_units[x]];
      rc = each(ctx, g, kind, most, pidx);
      if (rc != UNIT_OK) return rc;
    }
  return UNIT_OK;
}

// layout rows instead of launches: one row of 9 ints per unit -- {launch, tile kind, XCD, first workgroup slot on that XCD, tiles, index into
// pr, filter tap, split, first tile} (what the CPU tests check the dealing on)
struct WgradLayoutSink { int* rows; int cap, n, launch_no; };
static int wgrad_layout_launch(void* ctx, const WgradGroupArgs& g, int kind, int, const int* pidx) {
  WgradLayoutSink& o = *(WgradLayoutSink*)ctx;
  for (int x = 0; x < 8; ++x)
    for (int k = 0; k < g.t.n_units[x]; ++k) {
      UNIT_CHECK_ARG(o.n < o.cap, "wgrad_group_layout: more units than rows");
      const WgradUnitCode c = unpack_unit_code(g.t.unit_code[x][k]);
      int* r = o.rows + 9 * o.n++;
      r[0] = o.launch_no; r[1] = kind; r[2] = x; r[3] = g.t.unit_start[x][k]; r[4] = g.t.unit_start[x][k + 1] - g.t.unit_start[x][k];
      r[5] = pidx[c.problem]; r[6] = c.tap; r[7] = c.split; r[8] = g.t.unit_tile0[x][k];
    }
  ++o.launch_no;
  return UNIT_OK;
}

extern "C" int unit_conv2d_wgrad_group_layout(const UnitWgradProblem* pr, int n, int* layout, int layout_rows, int* rows) {
  UNIT_CHECK_ARG(pr != nullptr && n >= 0 && layout != nullptr && rows != nullptr, "wgrad_group_layout: null argument");
  WgradLayoutSink o{layout, layout_rows, 0, 0};
  int rc = wgrad_group_each_launch(pr, n, wgrad_layout_launch, &o);
  if (rc != UNIT_OK) return rc;
  *rows = o.n;
  return UNIT_OK;
}
