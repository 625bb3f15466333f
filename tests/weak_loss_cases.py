"""Named, seeded inputs of the weak-loss kernel tests (test_weak_loss_ops_cpu.py / test_weak_loss_ops_gpu.py; references: weak_loss_ref.py).

Small on purpose: each case sits on one rule of a kernel (its docstring in the tables below says which). Every input carries junk columns in
front of and behind the live ones and a row stride that is not the live width; the rows of empty slots hold NaN (MIL, mode 1) or a value
larger than every live one (mode 0): a kernel that reads outside its contract shows. `dy` buffers are made by the GPU test, filled with SENTINEL.

Boxes of every OICR case have small integer coordinates: areas, intersections and unions are exact in fp32 however the compiler contracts
them, an IoU is one correctly rounded division and has the same bits on the device, in torch fp32 and as the rounded float64 value.

Conditions on the inputs, asserted HERE when a case is built (never filtered at test time; a case that fails is given another seed):
  * mode 1, and MIL's x_r feeding mode 0: every chosen maximum leads its runner-up by a relative gap >= GAP in the float64 reference
  * every IoU that decides a row and was not placed on a threshold by hand lies >= GAP from both thresholds
"""
import functools

import numpy as np
import torch

import weak_loss_ref as ref

SENTINEL = 9.0          # bf16-representable
GAP = 1e-4
NAN = float("nan")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def valid_pattern(pattern, S, B):
    """-> int32 [B * S], 0 live / -1 empty.
    all: every slot live | ragged: image b keeps its first S - b * max(1, S // 5) slots (image 0 all of them) | third: rows 0, 3, 6, .. empty
    (image 1: rows 1, 4, ..) | wave: rows 64 .. 127 empty | mixed: image 0 loses its last S // 5 slots, image 1 is wholly empty, image 2 `third`"""
    v = torch.zeros(B, S, dtype=torch.int32)
    for b in range(B):
        kind = pattern if pattern != "mixed" else ("ragged", "empty", "third")[b % 3]
        if kind == "ragged" and S > 1:
            drop = (b if pattern == "ragged" else 1) * max(1, S // 5)
            if drop:
                v[b, S - drop:] = -1
        elif kind == "third":
            v[b, (b % 3)::3] = -1
        elif kind == "wave":
            v[b, 64:128] = -1
        elif kind == "empty":
            v[b] = -1
    return v.reshape(-1)


# ==================================================================================================== MIL
# name -> (B, S, K, valid pattern, (tc, td, mult, gscale), special, seed)
T0 = (1.0, 2.0, 1.0, 1.0)
T1 = (0.5, 3.0, 0.25, 0.125)
MIL = {
    # one row: the det softmax is 1 and p = softmax(cls); a cls logit at +100 puts p = 1.0 there and < 1e-6 elsewhere: both clamps, gradient 0
    "s1_k20_hi": (1, 1, 20, "all", T0, "hi", 11),
    "s63_k20_all": (2, 63, 20, "all", T0, None, 12),          # one wave, its last lane idle
    "s65_k20_ragged": (2, 65, 20, "ragged", T0, None, 13),          # image 0: the second wave holds one row; image 1 ends inside wave 0
    "s130_k32_third": (2, 130, 32, "third", T0, None, 14),          # register kernel's last K; empty slots inside every wave
    "s130_k32_wave": (2, 130, 32, "wave", T0, None, 15),          # register kernel: wave 1 wholly empty between two live ones
    "s130_k32_lo": (2, 130, 32, "all", T0, "lo", 16),          # register kernel: class 5 at cls -60 in every row, p < 1e-6 for y = 1 and y = 0
    "s130_k33_third": (2, 130, 33, "third", T0, None, 17),          # generic kernel's first K; valid < 0 in the middle of its waves
    "s130_k33_wave": (2, 130, 33, "wave", T0, None, 18),          # generic kernel: an empty wave
    "s130_k33_lo": (2, 130, 33, "all", T0, "lo", 19),          # generic kernel, lower clamp
    "s130_k33_temps": (2, 130, 33, "ragged", T1, None, 20),          # generic kernel, other temperatures / multiplier / gscale
    "s512_k20_all": (3, 512, 20, "all", T0, None, 21),          # the training shape: eight full waves, three images on the loss atomic
    "s512_k20_mixed": (3, 512, 20, "mixed", T0, None, 22),          # ragged, wholly empty and every-third images side by side
    "s512_k20_temps": (3, 512, 20, "ragged", T1, None, 23),
    "s513_k20_all": (2, 513, 20, "all", T0, None, 24),          # generic kernel because S > 512: thread 0 owns rows 0 and 512
    "s513_k20_hi1": (1, 513, 20, "hi1", T0, "hi", 25),          # generic kernel, upper clamp: one live row (512, thread 0's second) among empty ones
    "s1000_k80_third": (2, 1000, 80, "third", T0, None, 26),          # two rows per thread for most threads, K = 80
    "s70_k96_all": (1, 70, 96, "all", T0, None, 27),          # MIL_MAXK
}


@functools.lru_cache(maxsize=None)
def mil_case(name):
    """-> dict: streams [B*S, ld] fp32 (cls at ccol0, det at dcol0, junk elsewhere, NaN rows in empty slots), valid, multihot uint8 [B, K],
    B, S, K, tc, td, mult, gscale, ldd / dyc0 / dyd0 (the dy layout the GPU test uses)"""
    B, S, K, pattern, (tc, td, mult, gscale), special, seed = MIL[name]
    g = _gen(seed)
    ccol0, dcol0 = 3, 3 + K + 2
    ld = dcol0 + K + 4
    if pattern == "hi1":
        valid = torch.full((B * S,), -1, dtype=torch.int32)
        valid[S - 1] = 0
    else:
        valid = valid_pattern(pattern, S, B)
    streams = torch.full((B * S, ld), 7777.0)
    streams[:, ccol0:ccol0 + K] = torch.randn(B * S, K, generator=g) * 2.0
    streams[:, dcol0:dcol0 + K] = torch.randn(B * S, K, generator=g) * 3.0
    multihot = (torch.rand(B, K, generator=g) < 0.2).to(torch.uint8)
    multihot[:, 1] = 1          # every image has a label
    if special == "hi":
        streams[:, ccol0 + 2] = 100.0
    if special == "lo":
        streams[:, ccol0 + 5] = -60.0
        multihot[0, 5], multihot[1, 5] = 1, 0
    streams[valid < 0] = NAN
    return dict(name=name, streams=streams, ccol0=ccol0, dcol0=dcol0, K=K, valid=valid, S=S, B=B, multihot=multihot, tc=tc, td=td, mult=mult,
                gscale=gscale, special=special, ldd=2 * K + 11, dyc0=4, dyd0=4 + K + 3)


@functools.lru_cache(maxsize=None)
def mil_ref(name, dtype=torch.float64):
    c = mil_case(name)
    return ref.mil(c["streams"], c["ccol0"], c["dcol0"], c["K"], c["valid"], c["S"], c["B"], c["multihot"], c["tc"], c["td"], c["mult"],
                   c["gscale"], dtype=dtype)


# ==================================================================================================== OICR targets
def _int_boxes(g, n, lo=0, span=60, size=(4, 40)):
    x1 = torch.randint(lo, lo + span, (n,), generator=g)
    y1 = torch.randint(lo, lo + span, (n,), generator=g)
    w = torch.randint(size[0], size[1] + 1, (n,), generator=g)
    h = torch.randint(size[0], size[1] + 1, (n,), generator=g)
    return torch.stack([x1, y1, x1 + w, y1 + h], 1).float()


# the hand-placed rows of a mode 0 case (image 0), boxes against pseudo-GT A = (10, 10, 30, 30), area 400, and B = (40, 10, 60, 30)
GT_A, GT_B, GT_C, GT_D = (10, 10, 30, 30), (40, 10, 60, 30), (300, 300, 320, 320), (500, 500, 510, 510)
THRESHOLD_ROWS = {          # row -> (box, exact IoU with A as a fraction)
    41: ((10, 10, 20, 30), (200, 400)),          # 0.5
    42: ((10, 10, 20, 29), (190, 400)),          # one step under
    43: ((10, 10, 21, 29), (209, 400)),          # one step over
    44: ((10, 10, 12, 30), (40, 400)),          # float32(0.1)
    45: ((10, 10, 12, 29), (38, 400)),
    46: ((10, 10, 13, 24), (42, 400)),
    47: ((10, 10, 22, 30), (240, 400)),          # float32(0.6)
    48: ((10, 10, 16, 30), (120, 400)),          # float32(0.3)
    50: ((10, 10, 22, 29), (228, 400)),
    51: ((10, 10, 23, 29), (247, 400)),
    52: ((10, 10, 16, 29), (114, 400)),
    53: ((10, 10, 17, 28), (126, 400)),
}
EQUAL_IOU_ROW = 49          # (20, 10, 50, 30): 200 / 800 with A and with B -> the first (A) is matched
HAND_LABELS = lambda K: [1, 4, 7, 11, K - 1]

# name -> (mode, S, K, (fg, bg), seed)
OICR = {
    # mode 0, hand-placed (see _oicr_hand): the S names how many waves the block argmax combines
    "m0_s1_k20": (0, 1, 20, (0.5, 0.1), 31),          # one row, two labels: both pseudo-GT are that row (the second found among zeros)
    "m0_s64_k20": (0, 64, 20, (0.5, 0.1), 32),          # one wave: every tie is between lanes
    "m0_s65_k80": (0, 65, 80, (0.5, 0.1), 33),          # the tie partner is the only live row of wave 1
    "m0_s200_k95": (0, 200, 95, (0.6, 0.3), 34),          # K = 95, the largest; the other thresholds
    "m0_s512_k20": (0, 512, 20, (0.5, 0.1), 35),
    "m0_s512_k20_t": (0, 512, 20, (0.6, 0.3), 36),
    "m0_s1000_k80": (0, 1000, 80, (0.5, 0.1), 37),          # 16 waves, the last one ragged
    "m0_s1024_k95": (0, 1024, 95, (0.6, 0.3), 38),          # the largest block
    # mode 1, random logits (softmax in the kernel), images `third` and `ragged`
    "m1_s1_k20": (1, 1, 20, (0.5, 0.1), 41),
    "m1_s64_k80": (1, 64, 80, (0.6, 0.3), 42),
    "m1_s65_k95": (1, 65, 95, (0.5, 0.1), 43),
    "m1_s200_k20": (1, 200, 20, (0.5, 0.1), 44),
    "m1_s512_k20": (1, 512, 20, (0.6, 0.3), 45),
    "m1_s1000_k95": (1, 1000, 95, (0.5, 0.1), 46),
    "m1_s1024_k80": (1, 1024, 80, (0.5, 0.1), 47),
}


def _near_thresholds(info, valid, S, fg, bg, constructed):
    """-> the rows (into [B * S]) whose deciding IoU lies within GAP of a threshold and was not put there by hand (constructed: row numbers)"""
    out = []
    for b, best in enumerate(info["iou"]):
        if best is None:
            continue
        d = np.minimum(np.abs(best.astype(np.float64) - fg), np.abs(best.astype(np.float64) - bg))
        rows = ref.live_rows(valid, S, b)[torch.from_numpy(np.nonzero(d < GAP)[0])].tolist()
        out += [r for r in rows if r not in constructed]
    return out


def _settle(g, src, mode, K, rois5, valid, S, B, multihot, thr, col0, constructed):
    """draw the boxes of the rows of _near_thresholds again until there are none. Which rows become pseudo-GT depends on the scores alone, and
    a pseudo-GT's own deciding IoU is 1: the redraw never moves a pseudo-GT. -> (reference outputs, info)"""
    for _ in range(50):
        info = {}
        out = ref.oicr_targets(src, mode, K, rois5, valid, S, B, multihot, thr[0], thr[1], col0=col0, info=info)
        near = _near_thresholds(info, valid, S, thr[0], thr[1], constructed)
        if not near:
            return out, info
        rois5[near, 1:] = _int_boxes(g, len(near))
    raise AssertionError(("IoU within GAP of a threshold in rows", near))


def _oicr_hand(S, K, thr, seed):
    """Three images. Image 0 (labels 1, 4, 7, 11, K - 1; slots 60, 61, 62 empty) carries, in order of the classes:
      class 1: 0.75 in row 5 (box A) and in row t1 of the LAST wave (S >= 65; row 58 at S = 64), a far box: row 5 must win, across waves
      class 4: 0.5 in rows 20 (box B) and 33 (far box), two lanes of wave 0: row 20 must win
      class 7: 0.875 in the last live row S - 1 (box C); the empty slots hold 9.0 in every column, which must be ignored
      class 11: its column is zero in every live row -> the lowest row, row 0 (box D), score 0
      class K-1: zero again -> row 0 again although it has been zeroed: a second pseudo-GT with the same box; row 0 itself then has IoU 1 with
                 both and takes the first (class 11)
      so five labels meet three non-zero rows. Rows 41 .. 53 sit on and beside the thresholds against A (THRESHOLD_ROWS), row 49 has the same
      IoU to A and to B. At S = 65 the tie partner t1 IS the last row, 64, the only row of wave 1. Image 1 has no label, image 2 only empty
      slots (and labels). S = 1: image 0 is one row with two labels."""
    g = _gen(seed)
    B, col0, ld = 3, 2, K + 5
    src = torch.full((B * S, ld), SENTINEL)
    rois5 = torch.zeros(B * S, 5)
    valid = torch.zeros(B * S, dtype=torch.int32)
    multihot = torch.zeros(B, K, dtype=torch.uint8)
    rois5[:, 0] = torch.arange(B).repeat_interleave(S).float()
    rois5[:, 1:] = _int_boxes(g, B * S)
    src[:, col0:col0 + K] = torch.randint(0, 64, (B * S, K), generator=g).float() / 256.0          # < 0.25, exact
    valid[2 * S:] = -1
    constructed = set()
    if S == 1:
        multihot[0, [2, 5]] = 1
        multihot[2, 3] = 1
    else:
        multihot[0, HAND_LABELS(K)] = 1
        multihot[2, [0, 3]] = 1
        valid[60:63] = -1
        last = S - 1
        t1 = 58 if S == 64 else (64 if S == 65 else S - 5)
        assert t1 // 64 == last // 64 and (t1 >= 64 or S == 64)
        p = src[:S, col0:col0 + K]
        p[:, 11], p[:, K - 1] = 0.0, 0.0
        p[5, 1], p[t1, 1] = 0.75, 0.75
        p[20, 4], p[33, 4] = 0.5, 0.5
        p[last, 7] = 0.875
        b = rois5[:S, 1:]
        box = lambda t: torch.tensor(t).float()
        b[t1], b[33] = box((100, 100, 130, 130)), box((200, 200, 210, 210))
        b[5], b[20], b[last], b[0] = box(GT_A), box(GT_B), box(GT_C), box(GT_D)
        for r, (bx, _) in THRESHOLD_ROWS.items():
            b[r] = box(bx)
        b[EQUAL_IOU_ROW] = box((20, 10, 50, 30))
        constructed = set(THRESHOLD_ROWS) | {EQUAL_IOU_ROW}
    src[valid < 0] = SENTINEL
    out, info = _settle(g, src, 0, K, rois5, valid, S, B, multihot, thr, col0, constructed)
    return dict(src=src, col0=col0, rois5=rois5, valid=valid, multihot=multihot, B=B, constructed=constructed, ref=out, info=info)


def _oicr_random(S, K, thr, seed):
    g = _gen(seed)
    B, col0, ld = 2, 3, K + 1 + 7
    src = torch.full((B * S, ld), 50.0)          # a junk logit of 50 would own the softmax
    src[:, col0:col0 + K + 1] = torch.randn(B * S, K + 1, generator=g) * 2.0
    valid = torch.cat([valid_pattern("third", S, 1), valid_pattern("ragged", S, 2)[S:]]) if S > 1 else torch.zeros(B, dtype=torch.int32)
    src[valid < 0] = NAN
    rois5 = torch.zeros(B * S, 5)
    rois5[:, 0] = torch.arange(B).repeat_interleave(S).float()
    rois5[:, 1:] = _int_boxes(g, B * S)
    multihot = torch.zeros(B, K, dtype=torch.uint8)
    for b in range(B):
        multihot[b, torch.randperm(K, generator=g)[:2 + 2 * b]] = 1
    out, info = _settle(g, src, 1, K, rois5, valid, S, B, multihot, thr, col0, set())
    return dict(src=src, col0=col0, rois5=rois5, valid=valid, multihot=multihot, B=B, constructed=set(), ref=out, info=info)


@functools.lru_cache(maxsize=None)
def oicr_case(name):
    """-> dict: src [B*S, ld] (live columns at col0), rois5, valid, multihot, B, S, K, mode, fg, bg, ref = (labels, weights, boxes) of the float64
    reference, info (weak_loss_ref.oicr_targets), constructed (image 0's hand-placed threshold rows)"""
    mode, S, K, thr, seed = OICR[name]
    c = (_oicr_hand if mode == 0 else _oicr_random)(S, K, thr, seed)
    c.update(name=name, mode=mode, S=S, K=K, fg=thr[0], bg=thr[1])
    assert not _near_thresholds(c["info"], c["valid"], S, thr[0], thr[1], c["constructed"]), name
    if mode == 1 and S > 1:
        assert c["info"]["gap"] >= GAP, (name, "argmax lead", c["info"]["gap"])
    return c


CHAIN = "s512_k20_all"          # the MIL case whose x_r feeds mode 0


@functools.lru_cache(maxsize=None)
def chain_case():
    """MIL -> OICR mode 0 on the training shape: the float64 x_r of mil_case(CHAIN) as probabilities, integer boxes. The device feeds its own
    fp32 x_r; the lead of every chosen maximum (>= GAP, asserted) is far above x_r's error, so the decisions are the same"""
    m = mil_case(CHAIN)
    B, S, K = m["B"], m["S"], m["K"]
    g = _gen(51)
    rois5 = torch.zeros(B * S, 5)
    rois5[:, 0] = torch.arange(B).repeat_interleave(S).float()
    rois5[:, 1:] = _int_boxes(g, B * S)
    xr = mil_ref(CHAIN)[1]
    out, info = _settle(g, xr, 0, K, rois5, m["valid"], S, B, m["multihot"], (0.5, 0.1), 0, set())
    assert info["gap"] >= GAP, info["gap"]
    return dict(rois5=rois5, ref=out, info=info)


# ==================================================================================================== softmax cross-entropy
CE_NCLS = [2, 21, 32, 33, 81]
CE_ROWS = [1, 256, 257, 1000, 15425]          # 15425 = 240 * 64 + 65: the multi-workgroup grid stride wraps
CE_VARIANTS = [          # (weights, -inf columns, gscale), dealt round-robin over ncls x R
    ("none", False, 1.0), ("some", True, 0.25), ("zeros", False, 3.0), ("some", False, 1.0), ("none", True, 3.0), ("zeros", True, 0.25),
]
CE = {}
for _i, _n in enumerate(CE_NCLS):
    for _j, _r in enumerate(CE_ROWS):
        _w, _inf, _gs = CE_VARIANTS[(_i * len(CE_ROWS) + _j) % len(CE_VARIANTS)]
        _inf = _inf and _n > 2          # two classes leave no column to mask
        CE[f"c{_n}_r{_r}_w{_w}{'_inf' if _inf else ''}_g{_gs:g}"] = (_n, _r, _w, _inf, _gs, False)
CE["c21_r257_all_ignored"] = (21, 257, "some", False, 1.0, True)
CE["c81_r1000_all_ignored"] = (81, 1000, "none", True, 1.0, True)


@functools.lru_cache(maxsize=None)
def ce_case(name):
    """-> dict: logits [R, ld] fp32 (live at col0), labels int32 [R] (about one in eight -1 when R > 1), weights fp32 [R] or None
    (non-negative; `zeros`: a third of them 0, never row 0's), gscale, ldd / dcol0 for dy"""
    ncls, R, wkind, inf, gscale, ignored = CE[name]
    g = _gen(1000 * ncls + R)
    col0, ld = 5, ncls + 9
    logits = torch.full((R, ld), 7777.0)
    logits[:, col0:col0 + ncls] = torch.randn(R, ncls, generator=g) * 3.0
    labels = torch.randint(0, ncls, (R,), generator=g).int()
    if inf and ncls > 2:          # the novel mask: the same columns in every row, never the last column, never a label
        cols = torch.arange(1, ncls - 1, 4)
        logits[:, col0 + cols] = float("-inf")
        clash = torch.isin(labels, cols.int())
        labels[clash] = ncls - 1
    if R > 1:
        labels[torch.rand(R, generator=g) < 0.125] = -1
    if ignored:
        labels[:] = -1
    weights = None
    if wkind != "none":
        weights = torch.rand(R, generator=g) + 0.01
        if wkind == "zeros":
            weights[1:][torch.rand(R - 1, generator=g) < 0.33] = 0.0          # (row 0 keeps its weight: R = 1 is not a batch of weight 0)
    return dict(name=name, logits=logits, col0=col0, ncls=ncls, labels=labels, weights=weights, gscale=gscale, R=R, ldd=ncls + 6, dcol0=4,
                ignored=ignored)


@functools.lru_cache(maxsize=None)
def ce_ref(name, dtype=torch.float64):
    c = ce_case(name)
    return ref.softmax_ce(c["logits"], c["col0"], c["ncls"], c["labels"], c["weights"], c["gscale"], dtype=dtype)


# ==================================================================================================== score assembly, loss sum
SUP = {}
for _r, _n, _k in [(1, 21, 3), (300, 21, 3), (70, 81, 3), (70, 80, 1)]:          # (70, 80, n_oicr 1): the regression-branch call, never masked
    for _weak in (True, False):
        for _extra in (True, False):
            for _mask in ((True, False) if _n != 80 else (False,)):
                SUP[f"r{_r}_c{_n}{'_weak' if _weak else ''}{'_extra' if _extra else ''}{'_mask' if _mask else ''}"] = (_r, _n, _k, _weak, _extra, _mask)


@functools.lru_cache(maxsize=None)
def sup_case(name):
    R, ncls, n_oicr, has_weak, has_extra, has_mask = SUP[name]
    g = _gen(7 * R + ncls + 2 * has_weak + has_extra)
    dcol0, wcol0, ecol0 = 2, 3, 1

    def wide(cols, c0):
        t = torch.full((R, c0 + cols + 5), 7777.0)
        t[:, c0:c0 + cols] = torch.randn(R, cols, generator=g)
        return t
    mask = None
    if has_mask:
        mask = torch.zeros(ncls - 1, dtype=torch.uint8)
        mask[1::3] = 1
        mask[ncls - 2] = 1          # the last maskable column
    return dict(name=name, R=R, ncls=ncls, n_oicr=n_oicr, delta=wide(ncls, dcol0), dcol0=dcol0, weak=wide(n_oicr * ncls, wcol0) if has_weak else None,
                wcol0=wcol0, extra=wide(ncls, ecol0) if has_extra else None, ecol0=ecol0, mask=mask)


def sum_case(n):
    return torch.randn(9, generator=_gen(60 + n))[:n].contiguous() * 3.0
