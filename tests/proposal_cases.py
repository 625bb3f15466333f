"""Seeded inputs and the per-image CPU reference for the proposal / sampling tests (test_proposal_ops_cpu.py / _gpu.py).

Every output of these kernels is an index decision or a box, so the inputs are built to make each comparison bit for bit:
  matcher    integer-corner boxes: IoUs are ratios of small integers and land exactly on float32(0.3), 0.5 and float32(0.7) -- and, for
             three boxes found by search, on the float just below each; regions far apart keep the planted situations from touching
  sampler    labels and permutations only
  codec      the "exact" recipe: anchors with integer corners and even sizes, dw = dh = 0 (exp(0) = 1 exactly), dx / dy from
             {0, +-0.125, +-0.25} (times the weights): every decoded coordinate is a multiple of 1/8, exact in fp32 and in fp64
  rpn        the exact recipe in the RPN head's layout, with planted rows the reference drops (NaN delta, overflowing dx, +-inf logit,
             dw = -inf) or keeps (dw = +inf: clamped, then clipped to the whole image)
The reference helpers loop over images and call the oracle (Matcher, pairwise_iou, subsample_labels, get_deltas, apply_deltas,
find_top_rpn_proposals, label_and_sample_proposals, grid_anchors); they have no arithmetic of their own.
"""
import functools

import torch

import unit_oracle as orc

NAN, INF = float("nan"), float("inf")
ALL = 1 << 30          # "no limit"
CONFIGS = {"rpn": ([0.3, 0.7], [0, -1, 1], True), "roi": ([0.5], [0, 1], False)}          # (thresholds, labels, allow_low_quality)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _ri(gen, lo, hi, n):
    return torch.randint(lo, hi + 1, (n,), generator=gen)


def ref_match(q, cfg):
    th, lb, lq = CONFIGS[cfg]
    return orc.Matcher(th, lb, lq)(q)


# ------------------------------------------------------------------------------------------------ 1. matcher on a matrix
# the values a planted matrix draws from: each cut point, the float below it, and a few others -- so that columns tie between GTs (the first
# GT wins), row maxima are shared by many columns (all of them become 1 under allow_low_quality) and values sit on the cut points
def _below(x):
    t = torch.tensor(x, dtype=torch.float32)
    return float(torch.nextafter(t, torch.tensor(0.0)))


MATRIX_VALUES = [0.0, 0.125, _below(0.3), 0.3, _below(0.5), 0.5, _below(0.7), 0.7, 0.875]
TIES_ROW_VALUES = (6, 4, 9, 7)
MATRIX_CASES = {"n1": (3, 1), "n255": (5, 255), "n256": (5, 256), "n257": (5, 257), "m1": (1, 70), "m300": (300, 130), "ties": (4, 70)}


@functools.lru_cache(maxsize=None)
def matrix_case(name):
    """-> q [M,N] fp32. "ties" draws from MATRIX_VALUES only; the others are uniform with a sprinkling of those values"""
    m, n = MATRIX_CASES[name]
    gen = _gen(11 + sorted(MATRIX_CASES).index(name))
    vals = torch.tensor(MATRIX_VALUES, dtype=torch.float32)
    planted = vals[torch.randint(0, len(vals), (m, n), generator=gen)]
    if name == "ties":          # row r draws from the first TIES_ROW_VALUES[r] values: row maxima of 0.5, 0.3, 0.875 and just below 0.7
        return torch.stack([vals[torch.randint(0, k, (n,), generator=gen)] for k in TIES_ROW_VALUES])
    q = torch.where(torch.rand(m, n, generator=gen) < 0.25, planted, torch.rand(m, n, generator=gen))
    if m > 100:          # like a real IoU matrix: mostly zeros
        q = torch.where(torch.rand(m, n, generator=gen) < 0.01, q, torch.zeros(()))
    return q


# ------------------------------------------------------------------------------------------------ 2. fused matcher
MATCH_MCAP = 8
# boxes inside a GT [0,0,a,b] whose IoU (= c*d / (a*b)) is the float32 just below 0.3 / 0.5 / 0.7: (a, b, c, d), found by search and asserted
# by test_proposal_ops_cpu.py
BELOW = {0.3: (2486, 2489, 1373, 1352), 0.5: (3339, 3350, 2385, 2345), 0.7: (1527, 1538, 1511, 1088)}
BELOW_ORIGIN = {0.3: (0, 20000), 0.5: (0, 30000), 0.7: (0, 40000)}
G0 = [0, 0, 10, 10]
TIE_GT = [10020, 20, 10040, 40]
TIE_BOXES = [[10020, 20, 10040, 30], [10020, 30, 10040, 40], [10020, 20, 10030, 40]]          # IoU 0.5 each: tied for TIE_GT's maximum
ORPHAN_GT = [50000, 50000, 50010, 50010]          # overlaps no box
FILL_GTS = [[20030, 30, 20090, 80], [20100, 100, 20170, 180], [20010, 90, 20070, 150], [20090, 10, 20150, 70]]
MATCH_IMAGES = ("thresholds", "duplicates", "rowties", "orphan", "nogt", "short")
SHORT_BY = 40          # the "short" image's box_count is Ncap - SHORT_BY


def _shift(box, origin):
    return [box[0] + origin[0], box[1] + origin[1], box[2] + origin[0], box[3] + origin[1]]


def _below_gt(t):
    a, b, _, _ = BELOW[t]
    return _shift([0, 0, a, b], BELOW_ORIGIN[t])


def _below_box(t):
    _, _, c, d = BELOW[t]
    return _shift([0, 0, c, d], BELOW_ORIGIN[t])


# index of each planted box in the list: the four around G0 first, the rest at the very end (the last one alone in a block at Ncap = 257)
HEAD_BOXES = {"at0.3": [0, 0, 10, 3], "at0.5": [0, 0, 10, 5], "at0.7": [0, 0, 10, 7], "g0": G0}
TAIL_BOXES = {"tie0": TIE_BOXES[0], "tie1": TIE_BOXES[1], "tie2": TIE_BOXES[2],
              "gt0.3": _below_gt(0.3), "gt0.5": _below_gt(0.5), "gt0.7": _below_gt(0.7),
              "below0.3": _below_box(0.3), "below0.5": _below_box(0.5), "below0.7": _below_box(0.7)}


def planted_index(name, ncap):
    if name in HEAD_BOXES:
        return list(HEAD_BOXES).index(name)
    return ncap - len(TAIL_BOXES) + list(TAIL_BOXES).index(name)


@functools.lru_cache(maxsize=None)
def match_boxes(ncap):
    """the one box list [Ncap,4] every image of the matcher batch sees: planted boxes at both ends, seeded integer boxes in the fill region
    (around FILL_GTS) between them"""
    gen = _gen(100 + ncap)
    n = ncap - len(HEAD_BOXES) - len(TAIL_BOXES)
    x0, y0 = _ri(gen, 20000, 20160, n), _ri(gen, 0, 160, n)
    fill = torch.stack([x0, y0, x0 + _ri(gen, 10, 80, n), y0 + _ri(gen, 10, 80, n)], 1)
    return torch.cat([torch.tensor(list(HEAD_BOXES.values())), fill, torch.tensor(list(TAIL_BOXES.values()))]).float()


def match_gts():
    """-> (gt [B,Mcap,4] with NaN past each count, gt_count int32 [B]), one row per MATCH_IMAGES entry"""
    f = FILL_GTS
    per_image = {
        "thresholds": [G0, _below_gt(0.3), _below_gt(0.5), _below_gt(0.7), f[0], f[1]],
        "duplicates": [f[0], f[0], f[1], f[0]],          # the lower index wins
        "rowties": [TIE_GT, f[2]],
        "orphan": [f[0], ORPHAN_GT, f[3]],          # a row maximum of 0: every box has IoU 0 with ORPHAN_GT
        "nogt": [],
        "short": [G0, f[1], f[2], f[3], f[0], f[0], f[2], TIE_GT],          # Mcap GTs
    }
    gt = torch.full((len(MATCH_IMAGES), MATCH_MCAP, 4), NAN)
    for i, name in enumerate(MATCH_IMAGES):
        if per_image[name]:
            gt[i, : len(per_image[name])] = torch.tensor(per_image[name]).float()
    return gt, torch.tensor([len(per_image[n]) for n in MATCH_IMAGES], dtype=torch.int32)


def match_batch(ncap, form, junk=NAN):
    """-> (gt, gt_count, boxes, box_count). form "shared": boxes [Ncap,4], box_count None. form "per_image": boxes [B,Ncap,4], box_count
    int32 [B] = Ncap except for the "short" image, whose slots past its count hold `junk`"""
    gt, gt_count = match_gts()
    boxes = match_boxes(ncap)
    if form == "shared":
        return gt, gt_count, boxes, None
    b = len(MATCH_IMAGES)
    boxes = boxes[None].repeat(b, 1, 1)
    count = torch.full((b,), ncap, dtype=torch.int32)
    s = MATCH_IMAGES.index("short")
    count[s] = ncap - SHORT_BY
    boxes[s, ncap - SHORT_BY:] = junk
    return gt, gt_count, boxes, count


def ref_match_batch(gt, gt_count, boxes, box_count, cfg):
    """per image orc.Matcher(orc.pairwise_iou(gt, boxes)) -> (idx int64, label int8, val fp32), each [B,Ncap]; slots past an image's
    box_count: 0 / -1 / 0 (unit_iou_match's contract)"""
    b, ncap = gt.shape[0], boxes.shape[-2]
    idx, lab, val = torch.zeros(b, ncap, dtype=torch.int64), torch.full((b, ncap), -1, dtype=torch.int8), torch.zeros(b, ncap)
    for i in range(b):
        n = ncap if box_count is None else int(box_count[i])
        bx = boxes if boxes.dim() == 2 else boxes[i]
        idx[i, :n], lab[i, :n], val[i, :n] = ref_match(orc.pairwise_iou(gt[i, : int(gt_count[i])], bx[:n]), cfg)
    return idx, lab, val


def match_batch_mcap256(ncap=300):
    """Mcap = 256: one image with 256 GTs in the fill region, one with 3 -> (gt, gt_count, boxes [Ncap,4])"""
    gen = _gen(7)
    x0, y0 = _ri(gen, 20000, 20160, 256), _ri(gen, 0, 160, 256)
    gt = torch.full((2, 256, 4), NAN)
    gt[0] = torch.stack([x0, y0, x0 + _ri(gen, 10, 80, 256), y0 + _ri(gen, 10, 80, 256)], 1).float()
    gt[1, :3] = torch.tensor(FILL_GTS[:3]).float()
    return gt, torch.tensor([256, 3], dtype=torch.int32), match_boxes(ncap)


# ------------------------------------------------------------------------------------------------ 3. sampler
SAMPLER_SIZES = (1, 5, 1023, 1024, 1025, 2049)
SAMPLER_IMAGES = ("mixed", "no_pos", "no_neg", "all_ignored", "few_pos", "few_candidates", "short_count")
SAMPLER_K = 20


def sampler_params(n, kind):
    """-> (num_samples, positive_fraction, bg_label): the RPN's and the RoI heads' at full size, 4 samples for the tiny sizes"""
    if kind == "int8":
        return (256 if n > 5 else 4), 0.5, 0
    return (512 if n > 5 else 4), 0.25, SAMPLER_K


@functools.lru_cache(maxsize=None)
def sampler_batch(n, kind):
    """Ncap = Pcap = n, one image per SAMPLER_IMAGES entry -> (labels [B,n] int8 | int64, count int32 [B], perm int32 [B,n]). Positives are
    1 (int8) or classes 0..K-1 (int64, class 0 included); every permutation entry lies in [0, n)"""
    gen = _gen(1000 + n + (0 if kind == "int8" else 1))
    _, _, bg = sampler_params(n, kind)
    b = len(SAMPLER_IMAGES)

    def pos(m):
        return torch.ones(m, dtype=torch.int64) if kind == "int8" else torch.randint(0, SAMPLER_K, (m,), generator=gen)

    def scatter(n_pos, n_neg):
        """n_pos positives and n_neg negatives at random places, -1 elsewhere"""
        lab = torch.full((n,), -1, dtype=torch.int64)
        where = torch.randperm(n, generator=gen)
        lab[where[:n_pos]] = pos(n_pos)
        lab[where[n_pos: n_pos + n_neg]] = bg
        return lab

    labels = torch.empty(b, n, dtype=torch.int64)
    labels[0] = scatter(2 * n // 5, 2 * n // 5)
    labels[1] = scatter(0, n - n // 5)
    labels[2] = scatter((n + 1) // 2, 0)
    labels[3] = -1
    labels[4] = scatter(min(10, n // 3), n - min(10, n // 3))
    labels[5] = scatter(min(7, n // 3), min(20, n // 3))
    labels[6] = scatter(2 * n // 5, 2 * n // 5)
    count = torch.full((b,), n, dtype=torch.int32)
    count[6] = 2 * n // 3
    labels[6, int(count[6]):] = pos(n - int(count[6]))          # junk past the count that would be sampled if it were read
    perm = torch.stack([torch.randperm(n, generator=gen) for _ in range(b)]).int()
    return labels.to(torch.int8 if kind == "int8" else torch.int64), count, perm


def ref_sampler(labels, count, perm, num_samples, frac, bg):
    """per image orc.subsample_labels -> (out_labels int8 [B,n], sampled_idx int32 [B,S] with a -1 tail, counts int32 [B,2])"""
    b, n = labels.shape
    out, sidx = torch.full((b, n), -1, dtype=torch.int8), torch.full((b, num_samples), -1, dtype=torch.int32)
    counts = torch.zeros(b, 2, dtype=torch.int32)
    for i in range(b):
        pos, neg = orc.subsample_labels(labels[i, : int(count[i])], num_samples, frac, bg, perm[i].long())
        out[i, pos], out[i, neg] = 1, 0
        sidx[i, : len(pos) + len(neg)] = torch.cat([pos, neg]).int()
        counts[i, 0], counts[i, 1] = len(pos), len(neg)
    return out, sidx, counts


# ------------------------------------------------------------------------------------------------ 4. codec
UNIT_WEIGHTS = (1.0, 1.0, 1.0, 1.0)
HEAD_WEIGHTS = (10.0, 10.0, 5.0, 5.0)
HEAD_LD, HEAD_COL0, HEAD_K = 104, 21, 20          # the box head's row: 21 class scores, 80 deltas, 3 columns of padding
SHIFTS = (-0.25, -0.125, 0.0, 0.125, 0.25)


def exact_anchors(n, seed, x=(44, 200), y=(-20, 130)):
    """integer corners, even widths / heights in 4..46 px"""
    gen = _gen(seed)
    x0, y0 = _ri(gen, x[0], x[1], n), _ri(gen, y[0], y[1], n)
    return torch.stack([x0, y0, x0 + 2 * _ri(gen, 2, 23, n), y0 + 2 * _ri(gen, 2, 23, n)], 1).float()


def exact_deltas(n, k, seed, weights=UNIT_WEIGHTS):
    """[n, 4k]: dw = dh = 0; dx, dy = SHIFTS times the weight (-2.5 .. 2.5 for a weight of 10: IEEE division gives the shift back exactly)"""
    gen = _gen(seed)
    vals = torch.tensor(SHIFTS)
    d = torch.zeros(n, k, 4)
    d[..., 0] = vals[torch.randint(0, 5, (n, k), generator=gen)] * weights[0]
    d[..., 1] = vals[torch.randint(0, 5, (n, k), generator=gen)] * weights[1]
    return d.reshape(n, 4 * k)


def head_layout_case(n=300, seed=41):
    """the box head's layout: deltas of HEAD_K classes at column HEAD_COL0 of a HEAD_LD-wide row, NaN in every other column
    -> (rows [n,104], boxes [n,4])"""
    rows = torch.full((n, HEAD_LD), NAN)
    rows[:, HEAD_COL0: HEAD_COL0 + 4 * HEAD_K] = exact_deltas(n, HEAD_K, seed, HEAD_WEIGHTS)
    return rows, exact_anchors(n, seed + 1)


def general_boxes(n, seed, w=1000.0, h=600.0):
    gen = _gen(seed)
    x0, y0 = torch.rand(n, generator=gen) * (w - 200.0), torch.rand(n, generator=gen) * (h - 200.0)
    return torch.stack([x0, y0, x0 + 2.0 + torch.rand(n, generator=gen) * 190.0, y0 + 2.0 + torch.rand(n, generator=gen) * 190.0], 1)


# ------------------------------------------------------------------------------------------------ 4. rpn decode / select
RPN_A, RPN_LD, RPN_COL0 = 3, 16, 3          # per pixel: 3 logits, 12 deltas, one column of padding (NaN)
RPN_SIZES = [(96, 160), (80, 120), (24, 24)]          # every anchor starts at x >= 44: all of them clip to zero width in the last image
RPN_EMPTY_IMAGE = 2
RPN_CASES = [(3, 3), (1026, 1023), (1026, 1024), (1026, 1025), (16386, 16384), (16386, 16385), (16386, 16386)]          # (Ncap, topk)
RPN_LARGE = (1026, 16386)
RPN_MIN_SIZES = (0.0, 4.0)
SAFE_ANCHOR = [60, 20, 100, 60]          # 40 px wide, well inside the first two images: dropped only for what is planted in its row
EDGE_ANCHOR = [156, 30, 166, 50]         # clips to a width of exactly 4 in the 160 px image
NARROW_ANCHOR = [70, 30, 74, 50]         # 4 px wide
DROP_KINDS = ("dx_nan", "dw_nan", "dx_overflow", "pos_inf_logit", "neg_inf_logit", "dw_neg_inf")
KEEP_KINDS = ("dw_pos_inf",)
RPN_KINDS = DROP_KINDS + KEEP_KINDS
_PLANT_ORDER = ("dx_nan", "dw_nan", "dx_overflow", "pos_inf_logit", "neg_inf_logit", "dw_pos_inf", "dw_neg_inf")
RPN_LOWEST = 6          # so many unplanted SAFE_ANCHOR rows get the lowest finite logits: survivors on both sides of the last 1024 boundary
_TINY_PLAN = [(0, 2, "neg_inf_logit"), (1, 0, "dw_pos_inf"), (1, 1, "dw_nan")]


def _safe_rows(ncap):
    return [a for a in range(ncap) if a % 50 == 7]


def rpn_plan(ncap):
    """-> [(image, anchor id, kind)]: what is planted where. Only SAFE_ANCHOR rows (anchor id % 50 == 7) carry a defect; the second image's
    sit at other rows than the first's"""
    if ncap == 3:
        return list(_TINY_PLAN)
    safe = _safe_rows(ncap)
    assert len(safe) >= 2 * len(_PLANT_ORDER) + RPN_LOWEST
    return [(0, a, k) for a, k in zip(safe, _PLANT_ORDER)] + [(1, a, k) for a, k in zip(reversed(safe), _PLANT_ORDER)]


@functools.lru_cache(maxsize=None)
def rpn_case(ncap, kinds=RPN_KINDS):
    """-> dict(anchors [Ncap,4], logits [B,Ncap], deltas [B,Ncap,4], head [B,Ncap/A,ld], sorted_logit [B,Ncap], sorted_idx int32 [B,Ncap],
    image_hw [B,2]). A kind left out of `kinds` is not planted; its +-inf logit becomes +-1e30, so the sorted order is the same in every
    variant"""
    b = len(RPN_SIZES)
    gen = _gen(500 + ncap)
    anchors = exact_anchors(ncap, 600 + ncap)
    logits = torch.stack([(torch.randperm(ncap, generator=gen).float() - ncap // 2) / 256.0 for _ in range(b)])          # all distinct
    deltas = torch.stack([exact_deltas(ncap, 1, 700 + ncap + i) for i in range(b)])
    aid = torch.arange(ncap)
    if ncap == 3:
        anchors = torch.tensor([SAFE_ANCHOR, NARROW_ANCHOR, SAFE_ANCHOR]).float()
        deltas[:, :, :2] = 0
    else:
        for rem, box in ((7, SAFE_ANCHOR), (11, EDGE_ANCHOR), (13, NARROW_ANCHOR)):
            anchors[aid % 50 == rem] = torch.tensor(box).float()
            deltas[:, aid % 50 == rem] = 0
        free = _safe_rows(ncap)[len(_PLANT_ORDER): len(_PLANT_ORDER) + RPN_LOWEST]
        for i in range(b):          # hand the lowest logits to unplanted SAFE_ANCHOR rows (a swap: the values stay a permutation)
            for a, low in zip(free, torch.argsort(logits[i])[:RPN_LOWEST].tolist()):
                logits[i, [a, low]] = logits[i, [low, a]]
    for img, a, kind in rpn_plan(ncap):
        on = kind in kinds
        if kind == "dx_nan" and on:
            deltas[img, a, 0] = NAN
        elif kind == "dw_nan" and on:
            deltas[img, a, 2] = NAN
        elif kind == "dx_overflow" and on:
            deltas[img, a, 0] = 3.0e38          # times 40 px overflows fp32
        elif kind == "pos_inf_logit":
            logits[img, a] = INF if on else 1.0e30
        elif kind == "neg_inf_logit":
            logits[img, a] = -INF if on else -1.0e30
        elif kind == "dw_pos_inf" and on:
            deltas[img, a, 2] = INF           # clamped to SCALE_CLAMP: 62.5 * 40 px, clips to the whole image width
        elif kind == "dw_neg_inf" and on:
            deltas[img, a, 2] = -INF          # exp(-inf) = 0: zero width
    head = torch.full((b, ncap // RPN_A, RPN_LD), NAN)
    head[:, :, :RPN_A] = logits.view(b, -1, RPN_A)
    head[:, :, RPN_COL0: RPN_COL0 + 4 * RPN_A] = deltas.view(b, -1, 4 * RPN_A)
    sl, si = torch.sort(logits, dim=1, descending=True, stable=True)
    return dict(anchors=anchors, logits=logits, deltas=deltas, head=head, sorted_logit=sl, sorted_idx=si.int(),
                image_hw=torch.tensor(RPN_SIZES, dtype=torch.float32))


@functools.lru_cache(maxsize=None)
def rpn_candidates(ncap, topk, min_size, kinds=RPN_KINDS):
    """the reference's pre-NMS candidate list per image, [(boxes [n,4], logits [n])]: find_top_rpn_proposals read back through an NMS that
    suppresses nothing (threshold 2.0) and no post-NMS limit"""
    c = rpn_case(ncap, kinds)
    return orc.find_top_rpn_proposals(c["anchors"], c["logits"], c["deltas"], RPN_SIZES, nms_thresh=2.0, pre_nms_topk=topk,
                                      post_nms_topk=ALL, min_box_size=min_size)


# ------------------------------------------------------------------------------------------------ 5. RoI plumbing
ROI_K, ROI_PCAP, ROI_MCAP = 20, 700, 8
ROI_IMAGES = ("ordinary", "no_gt", "no_proposals", "few_candidates")
ROI_PCOUNT, ROI_GCOUNT = (650, 200, 0, 30), (5, 0, 3, 2)
ROI_SAMPLES = ((128, 0.25), (512, 0.25))


def _int_boxes(gen, n, lo=10, hi=120, w=400, h=300):
    x0, y0 = _ri(gen, 0, w, n), _ri(gen, 0, h, n)
    return torch.stack([x0, y0, x0 + _ri(gen, lo, hi, n), y0 + _ri(gen, lo, hi, n)], 1).float()


@functools.lru_cache(maxsize=None)
def roi_batch():
    """-> dict(props [B,Pcap,4], pcount, gt [B,Mcap,4], gcount, gt_classes int64 [B,Mcap], perm int32 [B,Pcap+Mcap]); NaN (classes: 99) in
    every slot past a count. A third of each image's proposals are its GTs jittered by up to 8 px"""
    gen = _gen(77)
    b = len(ROI_IMAGES)
    props, gt = torch.full((b, ROI_PCAP, 4), NAN), torch.full((b, ROI_MCAP, 4), NAN)
    gcls = torch.full((b, ROI_MCAP), 99, dtype=torch.int64)
    for i, (pc, gc) in enumerate(zip(ROI_PCOUNT, ROI_GCOUNT)):
        g = _int_boxes(gen, gc, 40, 160)
        p = _int_boxes(gen, pc)
        if gc and pc:
            near = pc // 3
            p[:near] = g[torch.randint(0, gc, (near,), generator=gen)] + torch.randint(-8, 9, (near, 4), generator=gen).float()
        props[i, :pc], gt[i, :gc], gcls[i, :gc] = p, g, torch.randint(0, ROI_K, (gc,), generator=gen)
    perm = torch.stack([torch.randperm(ROI_PCAP + ROI_MCAP, generator=gen) for _ in range(b)]).int()
    return dict(props=props, pcount=torch.tensor(ROI_PCOUNT, dtype=torch.int32), gt=gt, gcount=torch.tensor(ROI_GCOUNT, dtype=torch.int32),
                gt_classes=gcls, perm=perm)


@functools.lru_cache(maxsize=None)
def ref_roi_batch(num_samples, frac):
    """orc.label_and_sample_proposals on the batch's valid rows -> its list of dicts"""
    c = roi_batch()
    n = len(ROI_IMAGES)
    props = [(c["props"][i, : ROI_PCOUNT[i]], torch.zeros(ROI_PCOUNT[i])) for i in range(n)]
    gts = [c["gt"][i, : ROI_GCOUNT[i]] for i in range(n)]
    gcls = [c["gt_classes"][i, : ROI_GCOUNT[i]] for i in range(n)]
    return orc.label_and_sample_proposals(props, gts, gcls, [c["perm"][i].long() for i in range(n)], ROI_K, num_samples, frac)


# ------------------------------------------------------------------------------------------------ 6. anchor grid
GRID_SHAPES = ((1, 1), (1, 7), (5, 1))
GRID_OFFSETS = (0.0, 0.5)
