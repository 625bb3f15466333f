"""Seeded inputs and the batched CPU reference for the detection post-processing tests (test_detect_ops_cpu.py / _gpu.py).

The "exact" recipe makes the fp32 box decode bit-exact on both sides, so every decision (class, RoI index, count, order) and every
coordinate can be compared with torch.equal:
  proposals  integer corners, even widths / heights in 4..46 px, ~9 "objects" with +-6 px jitter (heavy suppression); every 17th
             proposal lies wholly right of the image and clips to zero width
  deltas     dw = dh = 0 (exp(0) = 1 exactly); dx, dy from {-2.5, -1.25, 0, 1.25, 2.5} with weights (10, 10, 5, 5): IEEE division
             gives +-0.25 / +-0.125 / 0, so every decoded coordinate is a multiple of 1/8 and so is the batched_nms class offset
  scores     integers 0..16 per entry, normalised per row, rounded to multiples of 1/64: hundreds of exact ties, which the reference
             orders by (RoI, class) through a stable sort
`ref_detections` loops over the images and calls the oracle (apply_deltas, fast_rcnn_inference_single, detector_postprocess); it has no
arithmetic of its own.
"""
import functools

import torch

import unit_oracle as orc

WEIGHTS = (10.0, 10.0, 5.0, 5.0)
IMAGE_HW = (96, 160)
OUT_HW = (192, 480)
NMS_THRESH = 0.5
ALL = 1 << 30          # "no topk"

# (name, R, K, topk, score threshold): one image each. The shapes are the smallest at which det_select_kernel's paths differ: fewer
# candidates than a wave; R*K = the block size and one more; K = 1; a chunk of 20 with threads straddling RoIs; several threads per RoI
# with the largest class offsets (K = 80: the 0.05 threshold admits nothing under this recipe, hence 0.01)
SINGLE_CASES = [
    ("r5_k3", 5, 3, 50, 0.05),
    ("r128_k8", 128, 8, 50, 0.05),
    ("r205_k5", 205, 5, 50, 0.05),
    ("r137_k7", 137, 7, 50, 0.05),
    ("r53_k1", 53, 1, 100, 0.05),
    ("r1000_k20", 1000, 20, 100, 0.05),
    ("r300_k80", 300, 80, 100, 0.01),
]
LARGE_CASES = ("r1000_k20", "r300_k80")
BATCH_RCAP, BATCH_K, BATCH_TOPK = 137, 7, 50
BATCH_HW = [(96, 160), (64, 64), (96, 160), (80, 120)]
BATCH_EMPTY_IMAGE = 2          # its class scores all equal 3/64: below 0.05, AT the threshold 3/64


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _ri(gen, lo, hi, n):
    return torch.randint(lo, hi + 1, (n,), generator=gen)


def exact_proposals(r, seed, hw=IMAGE_HW):
    gen = _gen(seed)
    h, w = hw
    n_obj = min(9, max(1, r // 3))          # ~9 objects; fewer for a handful of RoIs, so that they still overlap
    ow, oh = 2 * _ri(gen, 2, 23, n_obj), 2 * _ri(gen, 2, 23, n_obj)
    ox, oy = _ri(gen, 0, w - 46, n_obj), _ri(gen, 0, h - 46, n_obj)
    obj = _ri(gen, 0, n_obj - 1, r)
    bw = (ow[obj] + 2 * _ri(gen, -3, 3, r)).clamp(4, 46)
    bh = (oh[obj] + 2 * _ri(gen, -3, 3, r)).clamp(4, 46)
    x0, y0 = ox[obj] + _ri(gen, -6, 6, r), oy[obj] + _ri(gen, -6, 6, r)
    x0 = torch.where(torch.arange(r) % 17 == 3, w + 2 + _ri(gen, 0, 6, r), x0)          # wholly right of the image
    return torch.stack([x0, y0, x0 + bw, y0 + bh], 1).float()


def exact_deltas(r, k, seed):
    gen = _gen(seed)
    vals = torch.tensor([-2.5, -1.25, 0.0, 1.25, 2.5])
    d = torch.zeros(r, k, 4)
    d[..., 0] = vals[torch.randint(0, 5, (r, k), generator=gen)]
    d[..., 1] = vals[torch.randint(0, 5, (r, k), generator=gen)]
    return d.reshape(r, 4 * k)


def exact_scores(r, k, seed):
    gen = _gen(seed)
    v = torch.randint(0, 17, (r, k + 1), generator=gen).float()
    return torch.round(v / v.sum(1, keepdim=True).clamp(min=1.0) * 64.0) / 64.0


def exact_single(r, k, seed=0):
    """one image: (probs [R,K+1], deltas [R,4K], props [1,R,4], pcount [1] int32, image_hw [1,2])"""
    return (exact_scores(r, k, 100 + seed), exact_deltas(r, k, 200 + seed), exact_proposals(r, 300 + seed)[None],
            torch.tensor([r], dtype=torch.int32), torch.tensor([IMAGE_HW], dtype=torch.float32))


def exact_batch(empty_image=BATCH_EMPTY_IMAGE, seed=7):
    """B = 4 ragged images, pcount = [Rcap, 0, 1, Rcap - 3], per-image sizes; every row past pcount is NaN in probs, deltas and props"""
    rcap, k = BATCH_RCAP, BATCH_K
    pcount = [rcap, 0, 1, rcap - 3]
    b = len(pcount)
    probs = torch.full((b * rcap, k + 1), float("nan"))
    deltas = torch.full((b * rcap, 4 * k), float("nan"))
    props = torch.full((b, rcap, 4), float("nan"))
    for i, n in enumerate(pcount):
        rows = slice(i * rcap, i * rcap + n)
        probs[rows] = exact_scores(n, k, seed + 10 * i)
        deltas[rows] = exact_deltas(n, k, seed + 10 * i + 1)
        props[i, :n] = exact_proposals(n, seed + 10 * i + 2)
        if i == empty_image:
            probs[rows] = 3.0 / 64.0
    return probs, deltas, props, torch.tensor(pcount, dtype=torch.int32), torch.tensor(BATCH_HW, dtype=torch.float32)


# RoI rows of image 0 / 1 of `nonfinite_batch` and what is wrong with them. The first six make the reference drop the RoI whole; the
# last two are finite in the reference (clamped / zero width) and stay.
NONFINITE_DROPPED = {"dx_nan": 3, "dw_nan": 7, "dx_overflow": 12, "bg_prob_nan": 18, "cls_prob_nan": 23, "prop_inf": 31}
NONFINITE_KEPT = {"dw_pos_inf": 9, "dw_neg_inf": 27}
NONFINITE_R, NONFINITE_K, NONFINITE_CLASS = 40, 5, 2


def nonfinite_batch(seed=21):
    """B = 2 images of 40 RoIs x 5 classes from the exact recipe; image 0 carries all eight defects, image 1 only two of them (at other
    rows), so a per-image mix-up shows. Every defective RoI scores above the threshold in every class: dropping only the defective
    (RoI, class) pair is visible."""
    r, k, c = NONFINITE_R, NONFINITE_K, NONFINITE_CLASS
    probs = torch.cat([exact_scores(r, k, seed), exact_scores(r, k, seed + 1)])
    deltas = torch.cat([exact_deltas(r, k, seed + 2), exact_deltas(r, k, seed + 3)])
    props = torch.stack([exact_proposals(r, seed + 4), exact_proposals(r, seed + 5)])
    nan, inf = float("nan"), float("inf")
    loud = (4.0 + (torch.arange(k + 1) % 5).float()) / 64.0

    def put(img, row, kind):
        g = img * r + row
        probs[g] = loud
        props[img, row] = torch.tensor([60.0, 30.0, 100.0, 70.0])
        if kind == "dx_nan":
            deltas[g, 4 * c + 0] = nan
        elif kind == "dw_nan":
            deltas[g, 4 * c + 2] = nan
        elif kind == "dx_overflow":
            deltas[g, 4 * c + 0] = 3.0e38          # / 10 * 40 px overflows fp32
        elif kind == "bg_prob_nan":
            probs[g, k] = nan
        elif kind == "cls_prob_nan":
            probs[g, c] = nan
        elif kind == "prop_inf":
            props[img, row, 2] = inf
        elif kind == "dw_pos_inf":
            deltas[g, 4 * c + 2] = inf           # clamped to SCALE_CLAMP: 62.5 * 40 px, clips to the whole image width
        elif kind == "dw_neg_inf":
            deltas[g, 4 * c + 2] = -inf          # exp(-inf) = 0: a zero-width box
    for kind, row in {**NONFINITE_DROPPED, **NONFINITE_KEPT}.items():
        put(0, row, kind)
    put(1, 5, "bg_prob_nan")
    put(1, 14, "dw_nan")
    pcount = torch.tensor([r, r], dtype=torch.int32)
    return probs, deltas, props, pcount, torch.tensor([IMAGE_HW, IMAGE_HW], dtype=torch.float32)


def general_batch(seed=33, b=2, r=150, k=6, hw=(1200.0, 2000.0)):
    """fractional proposals and random deltas, dw / dh (after the weights) in [-3, 6] so that some exceed SCALE_CLAMP = 4.135"""
    gen = _gen(seed)
    n = b * r
    x0 = torch.rand(n, generator=gen) * (hw[1] - 200.0)
    y0 = torch.rand(n, generator=gen) * (hw[0] - 200.0)
    bw = 4.0 + torch.rand(n, generator=gen) * 180.0
    bh = 4.0 + torch.rand(n, generator=gen) * 180.0
    props = torch.stack([x0, y0, x0 + bw, y0 + bh], 1).reshape(b, r, 4)
    d = torch.empty(n, k, 4)
    d[..., :2] = (torch.rand(n, k, 2, generator=gen) - 0.5) * 2.0 * torch.tensor(WEIGHTS[:2])
    d[..., 2:] = (torch.rand(n, k, 2, generator=gen) * 9.0 - 3.0) * torch.tensor(WEIGHTS[2:])
    probs = torch.cat([exact_scores(r, k, seed + 1 + i) for i in range(b)])
    pcount = torch.tensor([r, r - 11][:b], dtype=torch.int32)
    return probs, d.reshape(n, 4 * k), props, pcount, torch.tensor([hw] * b, dtype=torch.float32)


def ref_detections(probs, deltas, props, pcount, image_hw, score_thresh, nms_thresh, topk, weights=WEIGHTS, out_hw=None):
    """the reference chain per image -> list of dicts: boxes [n,4], scores [n], classes [n] int64, roi [n] int64 (ORIGINAL rows of the
    image: the reference's own indices count its filtered rows, mapped back through valid.nonzero()), valid [R] bool; with out_hw (one
    (h, w) or a list of them) also pp_boxes [n,4] and nonempty [n] bool from detector_postprocess"""
    b, rcap = props.shape[0], props.shape[1]
    out = []
    for i in range(b):
        n = min(int(pcount[i]), rcap)
        rows = slice(i * rcap, i * rcap + n)
        hw = (float(image_hw[i][0]), float(image_hw[i][1]))
        boxes = orc.apply_deltas(deltas[rows], props[i, :n], weights)
        sc = probs[rows]
        bx, ss, cls, roi = orc.fast_rcnn_inference_single(boxes, sc, hw, score_thresh, nms_thresh, topk)
        valid = torch.isfinite(boxes).all(dim=1) & torch.isfinite(sc).all(dim=1)          # the reference's own row filter
        d = dict(boxes=bx, scores=ss, classes=cls, roi=valid.nonzero()[:, 0][roi], valid=valid)
        if out_hw is not None:
            ohw = out_hw[i] if isinstance(out_hw[0], (tuple, list)) else out_hw
            d["pp_boxes"], d["nonempty"] = orc.detector_postprocess(bx, hw, ohw)
        out.append(d)
    return out


def padded(ref, topk):
    """the per-image reference as ops.detections lays it out: ([B,topk,4], [B,topk], int32 [B,topk] x 2, int32 [B]), tails 0 / -1"""
    b = len(ref)
    boxes, scores = torch.zeros(b, topk, 4), torch.zeros(b, topk)
    cls, roi = torch.full((b, topk), -1, dtype=torch.int32), torch.full((b, topk), -1, dtype=torch.int32)
    cnt = torch.zeros(b, dtype=torch.int32)
    for i, d in enumerate(ref):
        n = d["scores"].numel()
        boxes[i, :n], scores[i, :n], cls[i, :n], roi[i, :n], cnt[i] = d["boxes"], d["scores"], d["classes"].int(), d["roi"].int(), n
    return boxes, scores, cls, roi, cnt


def candidates(probs, deltas, props, pcount, image_hw, score_thresh, weights=WEIGHTS):
    """the reference's candidate list per image in (RoI, class) order: (boxes [n,4] clipped, scores [n], classes [n], roi [n]) -- what
    fast_rcnn_inference_single hands to batched_nms, read back through an NMS that suppresses nothing and no topk"""
    out = []
    for d in ref_detections(probs, deltas, props, pcount, image_hw, score_thresh, 2.0, ALL, weights):
        key = d["roi"] * (probs.shape[1] - 1) + d["classes"]
        o = torch.argsort(key)
        out.append((d["boxes"][o], d["scores"][o], d["classes"][o], d["roi"][o]))
    return out


@functools.lru_cache(maxsize=None)
def single_case(name):
    """inputs and reference (with detector_postprocess to OUT_HW) of one SINGLE_CASES entry, computed once per session"""
    _, r, k, topk, thr = next(c for c in SINGLE_CASES if c[0] == name)
    inp = exact_single(r, k, seed=[c[0] for c in SINGLE_CASES].index(name))
    return dict(inputs=inp, k=k, topk=topk, thresh=thr, ref=ref_detections(*inp, thr, NMS_THRESH, topk, out_hw=OUT_HW))


@functools.lru_cache(maxsize=None)
def batch_case(empty_image=BATCH_EMPTY_IMAGE, thresh=0.05, topk=BATCH_TOPK):
    inp = exact_batch(empty_image)
    return dict(inputs=inp, k=BATCH_K, topk=topk, thresh=thresh, ref=ref_detections(*inp, thresh, NMS_THRESH, topk, out_hw=OUT_HW))
