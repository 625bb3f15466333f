"""Named, seeded cases for the class-segmented NMS stage (test_detect_seg_cpu.py / test_detect_seg_ops_gpu.py), built from the exact
recipe of tests/detect_cases.py: integer proposals, dw = dh = 0, deltas that decode to multiples of 1/8, scores that are multiples of
1/64 (1/1024 in the "all passing" cases). The fp32 decode is exact on both sides, so every comparison is torch.equal.

A case: dict(inputs=(probs, deltas, props, pcount, image_hw), k, thresh, topk, cand_cap (None: the default), and what it promises:
pops (per image the class populations) / n_cand / tie facts), see `case(name)`.
"""
import functools

import torch

import detect_cases as dc
import detect_seg_ref as sr

NMS_THRESH = dc.NMS_THRESH
OLD_LIMIT = 65536
POPS = (63, 64, 0, 65, 128, 129, 1)          # class populations of "pops": both sides of one and two 64-candidate words
OVER = {"over_k80": (900, 80), "over_k20": (3300, 20), "long_segment": (16500, 4)}          # R, K: all R * K candidates pass


def _single(r, k, seed):
    return dc.exact_scores(r, k, 100 + seed), dc.exact_deltas(r, k, 200 + seed), dc.exact_proposals(r, 300 + seed)


def _pack(probs, deltas, props):
    r = props.shape[0]
    return (probs, deltas, props[None], torch.tensor([r], dtype=torch.int32), torch.tensor([dc.IMAGE_HW], dtype=torch.float32))


def _populate(probs, pops, thresh):
    """class c keeps its first pops[c] passing scores (in RoI order), the others become 0"""
    probs = probs.clone()
    for c, want in enumerate(pops):
        passing = (probs[:, c] > thresh).nonzero()[:, 0]
        assert passing.numel() >= want, (c, passing.numel(), want)
        probs[passing[want:], c] = 0.0
    return probs


def _all_passing(r, k, seed):
    """exact scores plus a (RoI, class) pattern of 1..16 / 1024: every score > 0, still exact, ties across classes and RoIs everywhere"""
    probs, deltas, props = _single(r, k, seed)
    bump = (1 + (torch.arange(r)[:, None] * 7 + torch.arange(k + 1)[None] * 3) % 16).float() / 1024.0
    return probs + bump, deltas, props


def _build(name):
    thresh, topk, cap, extra = 0.05, 100, None, {}
    if name == "pops":
        probs, deltas, props = _single(220, len(POPS), 41)
        inputs = _pack(_populate(probs, POPS, thresh), deltas, props)
        extra = dict(pops=[list(POPS)])
    elif name == "empty_class_between":
        probs, deltas, props = _single(64, 3, 42)
        inputs = _pack(_populate(probs, (40, 0, 40), thresh), deltas, props)
        extra = dict(pops=[[40, 0, 40]])
    elif name == "one_class_all_rois":
        r, k = 150, 6
        probs, deltas, props = _single(r, k, 43)
        probs[:, 2] = torch.maximum(probs[:, 2], torch.tensor(4.0 / 64.0))          # class 2: every score at or below the threshold lifted over it
        probs = _populate(probs, (1, 1, r, 1, 1, 1), thresh)
        inputs = _pack(probs, deltas, props)
        extra = dict(pops=[[1, 1, r, 1, 1, 1]])
    elif name == "batch_empty_image":
        inputs = dc.exact_batch(dc.BATCH_EMPTY_IMAGE)          # pcount [137, 0, 1, 134]; image 2 scores 3/64 everywhere: below the threshold
        topk = dc.BATCH_TOPK
    elif name in ("ties_at_cut", "topk_1", "topk_above_union", "topk_5000"):
        inputs = _pack(*_single(300, 8, 44))
        if name == "topk_1":
            topk = 1
        elif name == "topk_5000":
            topk = 5000          # above NMS_DQ_MAXKEEP = 4096: unit_nms takes the plain scan for every segment
        else:
            bx, sc, cls, roi = sr.host_candidates(*inputs, thresh, dc.WEIGHTS)[0]
            keep = sr.full_keep(bx, sc, cls, NMS_THRESH, dc.ALL)
            if name == "topk_above_union":
                topk = keep.numel() + 9
                extra = dict(survivors=keep.numel())
            else:
                # the first cut that falls inside a run of equal scores holding several classes and several RoIs on both sides
                ks, kc, kr = sc[keep], cls[keep], roi[keep]
                topk = next(t for t in range(8, keep.numel() - 8)
                            if ks[t - 2] == ks[t + 1] and kc[t - 1] != kc[t] and kr[t - 1] != kr[t] and len(set(kr[t - 2:t + 2].tolist())) >= 3)
    elif name in ("count_equals_cap", "count_cap_minus_1"):
        inputs = _pack(*_single(137, 7, 45))
        n = sr.host_candidates(*inputs, thresh, dc.WEIGHTS)[0][1].numel()
        cap = n if name == "count_equals_cap" else n + 1
        extra = dict(n_cand=n)
    elif name in OVER:
        r, k = OVER[name]
        inputs = _pack(*_all_passing(r, k, 46 + list(OVER).index(name)))
        thresh, cap = 0.0, r * k
        extra = dict(n_cand=r * k)
    else:
        raise KeyError(name)
    k = inputs[1].shape[1] // 4
    return dict(name=name, inputs=inputs, k=k, thresh=thresh, topk=topk, cand_cap=cap, **extra)


SMALL = ("pops", "empty_class_between", "one_class_all_rois", "batch_empty_image", "ties_at_cut", "topk_1", "topk_above_union", "topk_5000",
         "count_equals_cap", "count_cap_minus_1")
LARGE = tuple(OVER)


@functools.lru_cache(maxsize=None)
def case(name):
    return _build(name)


@functools.lru_cache(maxsize=None)
def case_candidates(name):
    """the case's candidate lists per image (host_candidates), computed once"""
    c = case(name)
    return sr.host_candidates(*c["inputs"], c["thresh"], dc.WEIGHTS)


@functools.lru_cache(maxsize=None)
def case_ref(name):
    """the segmented rule's detections per image, computed once and shared"""
    c = case(name)
    return sr.segmented_detections(case_candidates(name), c["k"], NMS_THRESH, c["topk"])
