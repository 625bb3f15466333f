"""The cases of weak_wide_cases.py, anchored on the CPU before the GPU test (test_weak_wide_ops_gpu.py) compares unit_oicr_targets_wide with
them: the float64 reference (weak_loss_ref.py) and oracle/unit_oracle.py agree on every case; every decision of a mode 1 case has a margin far
above fp32 rounding (so no comparison is excluded anywhere: the excluded share is 0); and the cases hold what their names and docstrings say."""
import numpy as np
import pytest
import torch

import unit_oracle as orc
import weak_loss_cases as C
import weak_loss_ref as ref
import weak_wide_cases as W

U = 2.0 ** -24


def _packed(c, b):
    return ref.live_rows(c["valid"], c["S"], b)


def _oracle_targets(c, probs32):
    """oracle.oicr_targets on the packed rows of the images that have any -> (rows, labels, weights)"""
    K, B = c["K"], c["B"]
    rows = [_packed(c, b) for b in range(B)]
    keep = [b for b in range(B) if len(rows[b])]
    boxes = [c["rois5"][rows[b], 1:] for b in keep]
    gtc = [torch.nonzero(c["multihot"][b])[:, 0] for b in keep]
    idx = np.insert(np.cumsum([len(rows[b]) for b in keep]), 0, 0).tolist()
    allrows = torch.cat([rows[b] for b in keep])
    lab, w = orc.oicr_targets(boxes, probs32[allrows], gtc, idx, c["fg"], c["bg"], num_classes=K)
    return allrows, lab, w


@pytest.mark.parametrize("name", list(W.CASES))
def test_reference_vs_oracle(name):
    """labels exactly; weights bit for bit in mode 0 (copies) and within fp32 rounding in mode 1; empty slots (-1, 0, zeros); an image without a
    label (K, 0, zeros); a matched box is a box of a row of the same image"""
    c = W.case(name)
    K, B = c["K"], c["B"]
    lab, w, gb = c["ref"]
    x = c["src"][:, c["col0"]:c["col0"] + (K if c["mode"] == 0 else K + 1)]
    probs32 = x if c["mode"] == 0 else torch.softmax(x, -1)
    allrows, olab, ow = _oracle_targets(c, probs32)
    assert torch.equal(lab[allrows], olab)
    if c["mode"] == 0:
        assert torch.equal(w[allrows].float(), ow)
    else:
        assert torch.allclose(w[allrows], ow.double(), rtol=1e-5, atol=2e-6 * float(ow.abs().max()))
    empty = c["valid"] < 0
    assert bool(empty.any()) and bool((lab[empty] == -1).all()) and float(w[empty].abs().max()) == 0 and float(gb[empty].abs().max()) == 0
    for b in range(B):
        rows = _packed(c, b)
        if not len(rows):
            continue
        if not c["multihot"][b].any():
            assert bool((lab[rows] == K).all()) and float(w[rows].abs().max()) == 0 and float(gb[rows].abs().max()) == 0
            continue
        own = c["rois5"][rows, 1:].double()
        picked = own[torch.as_tensor(c["info"]["picks"][b])]
        assert bool((gb[rows][:, None, :] == picked[None]).all(-1).any(1).all())


@pytest.mark.parametrize("name", [n for n, v in W.CASES.items() if v[0] == 1])
def test_mode1_margins(name):
    """every decision of a mode 1 case: each chosen maximum leads its runner-up by a relative >= GAP = 1e-4 in float64, while an fp32 softmax
    value is off by a relative (K + 5 + 2 A) u ~ 1e-5 at the very worst (test_weak_loss_ops_gpu.py: _floor_oicr_weight; A the spread of a row's
    logits; measured errors are ~1e-7) -- asserted below, and the fp32 evaluation decides the same, checked; every deciding IoU is one correctly rounded division of exact integers (the same bits
    everywhere) and, where it meets a threshold, >= GAP away from it. Nothing is excluded from any comparison."""
    c = W.case(name)
    K, S, B = c["K"], c["S"], c["B"]
    assert c["info"]["gap"] >= W.GAP
    x = c["src"][c["valid"] >= 0, c["col0"]:c["col0"] + K + 1].double()
    spread = float((x.max(1).values - x.min(1).values).max())
    assert 2 * (2 * (K + 5 + 2 * spread) * U) < W.GAP          # both values off by the worst case, against each other: still under half the lead
    assert not C._near_thresholds(c["info"], c["valid"], S, c["fg"], c["bg"], set())
    boxes = c["rois5"][:, 1:]
    assert bool((boxes == boxes.round()).all()) and float(boxes.max()) < 2048          # areas and intersections < 2^24: exact in fp32
    probs32 = torch.softmax(torch.nan_to_num(c["src"][:, c["col0"]:c["col0"] + K + 1]), -1)
    info32 = {}
    lab32, _, gb32 = ref.oicr_targets(probs32, 0, K, c["rois5"], c["valid"], S, B, c["multihot"], c["fg"], c["bg"], info=info32)
    assert info32["picks"] == c["info"]["picks"] and torch.equal(lab32, c["ref"][0]) and torch.equal(gb32, c["ref"][2])


def test_cases_cover_the_shapes():
    v = list(W.CASES.values())
    assert {x[1] for x in v} == set(W.SIZES) == {1000, 1024, 1025, 2047, 2048, 2049, 5000, 8192}
    for mode in (0, 1):
        assert {x[1] for x in v if x[0] == mode} == set(W.SIZES)
        assert {x[2] for x in v if x[0] == mode} == {20, 80, 95} and {x[3] for x in v if x[0] == mode} == {1, 3}
        assert {x[4] for x in v if x[0] == mode} == {(0.5, 0.1), (0.6, 0.3)}
    assert len({x[5] for x in v}) == len(v)


@pytest.mark.parametrize("name", W.HAND)
def test_hand_placed_rows(name):
    """the decisions the rows were placed for, spelled out on the reference's outputs"""
    c = W.case(name)
    K, S, fg, bg = c["K"], c["S"], c["fg"], c["bg"]
    lab, w, gb = c["ref"]
    pl = c["places"]
    T, wave = W.THREADS, lambda r: (r % W.THREADS) // 64
    live = _packed(c, 0).tolist()
    picks = [live[j] for j in c["info"]["picks"][0]]
    assert picks == [pl["same"][0], pl["threads"][0], pl["runner"], pl["waves"][0], pl["cross"][0], pl["shared"][0], pl["shared"][1], 0]
    p = c["src"][:S, c["col0"]:c["col0"] + K]
    tie = lambda rows, cls: float(p[rows[0], cls]) == float(p[rows[1], cls]) == float(p[[r for r in live], cls].max()) and rows[0] < rows[1]
    assert tie(pl["same"], W.CLS_SAME_THREAD) and tie(pl["threads"], W.CLS_TWO_THREADS) and tie(pl["waves"], W.CLS_TWO_WAVES)
    assert tie(pl["cross"], W.CLS_LOW_ROW_HIGH_THREAD)
    # where the tied rows sit
    a, a2 = pl["same"]
    if S > T:
        assert a2 == a + T and a % T == a2 % T                                  # two rows of one thread
        lo, hi = pl["cross"]
        assert lo // T == 0 and hi // T == 1 and wave(lo) == 15 and wave(hi) == 0          # the lower ROW belongs to the higher thread and wave
    t0, t1 = pl["threads"]
    assert t0 // T == t1 // T and wave(t0) == wave(t1) and t0 % T != t1 % T          # two threads of one wave
    w0, w1 = pl["waves"]
    assert w0 // T == w1 // T == max(0, (S - 324) // T) and wave(w0) != wave(w1)          # two waves, the highest slot that holds both
    if S >= 1100:
        assert t0 // T == 1 and w0 // T >= 1          # the winners sit in a second or later slot of their threads ...
    # ... and the zeroing is seen by the next class: its own largest entry is in the zeroed row
    assert float(p[t0, W.CLS_AFTER_ZEROING]) == 0.9375 > float(p[pl["runner"], W.CLS_AFTER_ZEROING]) == 0.625
    assert float(p[live, W.CLS_AFTER_ZEROING].max()) == 0.9375
    # two labelled classes whose maxima sit in the same row
    s0, s1 = pl["shared"]
    assert int(p[:, W.CLS_SHARED_A][live].argmax()) == live.index(s0) and int(p[:, W.CLS_SHARED_B][live].argmax()) == live.index(s0)
    assert float(w[s1]) == 0.4375 and int(lab[s1]) == W.CLS_SHARED_B and int(lab[s0]) == W.CLS_SHARED_A
    # the all-zero class: the lowest row, score 0; its row keeps the label of the first pseudo-GT with its box
    assert float(p[live, K - 1].abs().max()) == 0
    assert int(lab[0]) == (W.CLS_SAME_THREAD if a == 0 else K - 1) and float(w[0]) == (0.75 if a == 0 else 0.0)
    # empty slots inside a wave, a whole wave, a range across waves in the second slot; they hold the sentinel, larger than every live value
    for lo, hi in pl["empty"]:
        assert bool((c["valid"][lo:hi] < 0).all()) and float(c["src"][lo:hi].min()) == W.SENTINEL and bool((lab[lo:hi] == -1).all())
    assert (60, 63) in pl["empty"] and (64, 128) in pl["empty"] and (S <= 1470 or any(lo // 64 != (hi - 1) // 64 and lo >= T for lo, hi in pl["empty"]))
    assert float(p[live].max()) < W.SENTINEL
    # the threshold rows, exactly on and beside fg / bg against GT_A
    tb = pl["tb"]
    A = torch.tensor(C.GT_A).double()
    f32 = np.float32
    assert tb == (T if S >= 1100 else 0)
    for r, (box, (num, den)) in C.THRESHOLD_ROWS.items():
        iou32 = f32(ref.pairwise_iou(A[None].numpy(), torch.tensor(box).double()[None].numpy())[0, 0])
        assert iou32 == f32(num) / f32(den)
        assert torch.equal(gb[r + tb], A), r
        assert int(lab[r + tb]) == (W.CLS_SAME_THREAD if iou32 >= f32(fg) else K), r
        assert float(w[r + tb]) == (0.75 if iou32 >= f32(bg) else 0.0), r
    on = {0.5: 41, 0.1: 44, 0.6: 47, 0.3: 48}
    assert int(lab[on[fg] + tb]) == W.CLS_SAME_THREAD and float(w[on[bg] + tb]) == 0.75          # exactly fg is foreground, exactly bg keeps its weight
    e = C.EQUAL_IOU_ROW + tb
    assert torch.equal(gb[e], A) and int(lab[e]) == K and float(w[e]) == (0.75 if bg <= 0.25 else 0.0)
    # image 1: no label; image 2: wholly empty (with labels)
    assert not c["multihot"][1].any() and bool((c["valid"][S:2 * S] >= 0).all()) and bool((lab[S:2 * S] == K).all())
    assert bool(c["multihot"][2].any()) and bool((c["valid"][2 * S:] < 0).all()) and bool((lab[2 * S:] == -1).all())


def test_more_labels_than_live_rows():
    c = W.case(W.FEW)
    lab, w, gb = c["ref"]
    live = _packed(c, 0).tolist()
    assert live == list(W.FEW_ROWS) and int(c["multihot"].sum()) == 4 > len(live)
    assert live[0] // W.THREADS != live[1] // W.THREADS and live[0] % W.THREADS != live[1] % W.THREADS
    assert [live[j] for j in c["info"]["picks"][0]] == [W.FEW_ROWS[1], W.FEW_ROWS[0], W.FEW_ROWS[0], W.FEW_ROWS[0]]
    # each live row is its own first pseudo-GT (IoU 1): the higher row carries class 2 at 0.5, the lower class 6
    assert int(lab[W.FEW_ROWS[1]]) == W.FEW_LABELS[0] and float(w[W.FEW_ROWS[1]]) == 0.5 and int(lab[W.FEW_ROWS[0]]) == W.FEW_LABELS[1]


def test_mode1_cases_have_empty_slots_inside_and_between_waves():
    for name, v in W.CASES.items():
        if v[0] != 1:
            continue
        c = W.case(name)
        S, val = c["S"], c["valid"]
        assert bool((val[:S][0::3] < 0).all()) and bool((val[:S][1::3] >= 0).all())          # inside every wave
        if v[3] == 3:
            assert bool((val[2 * S - S // 5:2 * S] < 0).all()) and bool((val[2 * S + 64:2 * S + 128] < 0).all())          # a tail, a whole wave
            assert S <= 1300 or bool((val[2 * S + 1100:2 * S + 1300] < 0).all())
