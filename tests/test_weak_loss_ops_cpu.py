"""The float64 references of weak_loss_ref.py, anchored: the GPU tests (test_weak_loss_ops_gpu.py) compare the kernels with them, so they are
first compared with the reference project's own recorded results (tests/golden/unit_golden.npz: W20, W20b, W80) and, on every named case of
weak_loss_cases.py, with oracle/unit_oracle.py run in fp32 on the packed rows. The conditions the cases promise (stable argmaxes, IoUs off the
thresholds unless placed there, clamps really reached, threshold rows really on their thresholds) are asserted here too."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import unit_oracle as orc
import weak_loss_cases as C
import weak_loss_ref as ref

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "unit_golden.npz"))


def T(k):
    return torch.from_numpy(GOLD[k])


def close(a, b, rtol=1e-5, atol=1e-6):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    assert a.shape == b.shape, (a.shape, b.shape)
    assert torch.allclose(a, b, rtol=rtol, atol=atol), (a - b).abs().max()


def fp32_close(got64, want32):
    """within the fp32 oracle's rounding: a few ulp of the value, plus a few ulp of the largest value for what is a sum of many terms"""
    want = torch.as_tensor(want32).double()
    big = float(want.abs().max()) if want.numel() else 0.0
    close(got64, want, rtol=1e-5, atol=2e-6 * big + 1e-30)


# ---------------------------------------------------------------------------------------------------- the reference project's recorded results
def _slots(tag, K):
    """the fixture in the kernels' layout, as test_unit_golden_gpu.py packs it: ragged images in slots of S = max(sizes) rows"""
    sizes = GOLD[f"{tag}/sizes"].tolist()
    B, S = len(sizes), max(sizes)
    rows = torch.cat([torch.arange(i * S, i * S + n) for i, n in enumerate(sizes)])
    lin = torch.full((B * S, 2 * K + 3 * (K + 1) + 4), float("nan"))
    lin[rows, :K] = T(f"{tag}/cls_stream")
    lin[rows, K:2 * K] = T(f"{tag}/det_stream") * 2.0          # the raw Linear output; DETECTOR_TEMP 2
    for k in range(3):
        lin[rows, 2 * K + k * (K + 1): 2 * K + (k + 1) * (K + 1)] = T(f"{tag}/oicr{k}")
    rois5 = torch.zeros(B * S, 5)
    valid = torch.full((B * S,), -1, dtype=torch.int32)
    valid[rows] = 0
    multihot = torch.zeros(B, K, dtype=torch.uint8)
    for i, n in enumerate(sizes):
        rois5[i * S:i * S + n, 1:] = T(f"{tag}/boxes{i}")
        multihot[i, T(f"{tag}/targets{i}").long()] = 1
    return B, S, rows, lin, rois5, valid, multihot


@pytest.mark.parametrize("tag,K", [("W20", 20), ("W20b", 20), ("W80", 80)])
def test_reference_reproduces_the_recorded_weak_losses(tag, K):
    """labels exactly; weights and losses at the tolerances test_unit_golden_cpu.py holds the oracle to"""
    B, S, rows, lin, rois5, valid, multihot = _slots(tag, K)
    loss, xr, _, _ = ref.mil(lin, 0, K, K, valid, S, B, multihot, 1.0, 2.0, 1.0, 1.0)
    close(loss, T(f"{tag}/loss_im_cls"), rtol=1e-5, atol=1e-6)
    for it in range(3):
        if it == 0:
            lab, w, _ = ref.oicr_targets(xr, 0, K, rois5, valid, S, B, multihot)
        else:
            lab, w, _ = ref.oicr_targets(lin, 1, K, rois5, valid, S, B, multihot, col0=2 * K + (it - 1) * (K + 1))
        assert torch.equal(lab[rows], T(f"{tag}/oicr_labels{it}")), it
        close(w[rows], T(f"{tag}/oicr_weights{it}"), rtol=1e-6, atol=1e-7)
        assert bool((lab[valid < 0] == -1).all()) and float(w[valid < 0].abs().max() if (valid < 0).any() else 0) == 0
        l, _ = ref.softmax_ce(lin, 2 * K + it * (K + 1), K + 1, lab, w)
        close(l, T(f"{tag}/loss_oicr_{it + 1}"), rtol=1e-5, atol=1e-6)


# ---------------------------------------------------------------------------------------------------- MIL cases against the oracle
def _packed(c, b):
    return ref.live_rows(c["valid"], c["S"], b)


@pytest.mark.parametrize("name", list(C.MIL))
def test_mil_reference_vs_oracle(name):
    """oracle.weak_losses (fp32, packed rows, autograd) gives the same loss and gradients; x_r is the product of the two softmaxes in fp32"""
    c = C.mil_case(name)
    K, S, B = c["K"], c["S"], c["B"]
    loss, xr, dcls, ddet = C.mil_ref(name)
    rows = [_packed(c, b) for b in range(B)]
    allrows = torch.cat(rows)
    cls = c["streams"][allrows, c["ccol0"]:c["ccol0"] + K].clone().requires_grad_(True)
    det = c["streams"][allrows, c["dcol0"]:c["dcol0"] + K].clone().requires_grad_(True)
    boxes = [torch.zeros(len(r), 4) for r in rows]
    targets = [torch.nonzero(c["multihot"][b])[:, 0] for b in range(B)]
    lo = orc.weak_losses(cls / c["tc"], det / c["td"], [], boxes, targets, mil_multiplier=c["mult"], num_classes=K)["loss_im_cls"]
    (lo * c["gscale"]).backward()
    fp32_close(loss, lo.detach())
    fp32_close(dcls[allrows], cls.grad)
    fp32_close(ddet[allrows], det.grad)
    off = 0
    for r in rows:
        a, d = cls.detach()[off:off + len(r)] / c["tc"], det.detach()[off:off + len(r)] / c["td"]
        fp32_close(xr[r], torch.softmax(a, -1) * torch.softmax(d, 0))
        off += len(r)
    empty = c["valid"] < 0
    if empty.any():
        assert float(xr[empty].abs().max()) == 0 and float(dcls[empty].abs().max()) == 0 and float(ddet[empty].abs().max()) == 0
    assert torch.isfinite(xr).all() and torch.isfinite(dcls).all() and torch.isfinite(ddet).all()


def test_mil_clamp_cases_are_clamped():
    """the class vector of the clamp cases lies outside [1e-6, 1 - 1e-6] by a factor >= 10 (or is exactly 1) where the case says so, and the
    reference's gradient through those classes is zero; every other case stays inside"""
    for name in C.MIL:
        c = C.mil_case(name)
        p = ref.mil_class_vector(c["streams"], c["ccol0"], c["dcol0"], c["K"], c["valid"], c["S"], c["B"], c["tc"], c["td"])
        has_rows = torch.tensor([len(_packed(c, b)) > 0 for b in range(c["B"])])
        if c["special"] == "hi":
            assert float(p[0, 2]) == 1.0 and float(p[0].float()[2]) == 1.0
            rest = torch.cat([p[0, :2], p[0, 3:]])
            assert float(rest.max()) <= 1e-7
            assert float(C.mil_ref(name)[2].abs().max()) == 0 and float(C.mil_ref(name)[3].abs().max()) == 0
        elif c["special"] == "lo":
            assert float(p[:, 5].max()) <= 1e-7
            assert c["multihot"][0, 5] == 1 and c["multihot"][1, 5] == 0
            dcls = C.mil_ref(name)[2]
            assert float(dcls.abs().max()) > 0          # the other classes still train
            inside = torch.ones(c["K"], dtype=torch.bool)
            inside[5] = False
            assert bool(((p[:, inside] > 1e-5) & (p[:, inside] < 1 - 1e-5)).all())
        else:
            q = p[has_rows]
            assert bool(((q > 1e-5) & (q < 1 - 1e-5)).all()), name
            assert float(p[~has_rows].abs().max() if (~has_rows).any() else 0) == 0          # an image without rows: p = 0, clamped to 1e-6


def test_mil_cases_reach_every_path():
    """which kernel a case runs (K <= 32 and S <= 512: the register kernel), and that each kernel has its multi-wave, empty-wave, clamped cases"""
    reg = {n for n, v in C.MIL.items() if v[2] <= 32 and v[1] <= 512}
    gen = set(C.MIL) - reg
    for group in (reg, gen):
        assert any(C.MIL[n][1] > 64 for n in group)
        assert any(C.MIL[n][3] == "wave" for n in group)
        assert any(C.MIL[n][5] == "lo" for n in group) and any(C.MIL[n][5] == "hi" for n in group)
        assert any(C.MIL[n][4] != C.T0 for n in group)
    assert any(C.MIL[n][2] > 32 for n in gen) and any(C.MIL[n][1] > 512 and C.MIL[n][2] <= 32 for n in gen)
    assert {(v[0], v[1], v[2]) for v in C.MIL.values()} >= {(1, 1, 20), (2, 63, 20), (2, 65, 20), (2, 130, 32), (2, 130, 33), (3, 512, 20),
                                                             (2, 513, 20), (2, 1000, 80), (1, 70, 96)}


# ---------------------------------------------------------------------------------------------------- OICR cases against the oracle
def _oracle_targets(c, probs32):
    """oracle.oicr_targets on the packed rows of the images that have any (it cannot take an image without rows) -> (rows, labels, weights)"""
    K, S, B = c["K"], c["S"], c["B"]
    rows = [_packed(c, b) for b in range(B)]
    keep = [b for b in range(B) if len(rows[b])]
    boxes = [c["rois5"][rows[b], 1:] for b in keep]
    gtc = [torch.nonzero(c["multihot"][b])[:, 0] for b in keep]
    idx = np.insert(np.cumsum([len(rows[b]) for b in keep]), 0, 0).tolist()
    allrows = torch.cat([rows[b] for b in keep])
    lab, w = orc.oicr_targets(boxes, probs32[allrows], gtc, idx, c["fg"], c["bg"], num_classes=K)
    return allrows, lab, w


@pytest.mark.parametrize("name", list(C.OICR))
def test_oicr_reference_vs_oracle(name):
    """labels exactly, weights within fp32 rounding (mode 0: they are copies, bit for bit); empty slots (-1, 0, zeros); an image without a label
    (K, 0, zeros); a matched box is the box of a row of the same image and, for a foreground row, overlaps it by >= fg"""
    c = C.oicr_case(name)
    K, S, B = c["K"], c["S"], c["B"]
    lab, w, gb = c["ref"]
    x = c["src"][:, c["col0"]:c["col0"] + (K if c["mode"] == 0 else K + 1)]
    probs32 = x if c["mode"] == 0 else torch.softmax(x, -1)
    allrows, olab, ow = _oracle_targets(c, probs32)
    assert torch.equal(lab[allrows], olab)
    if c["mode"] == 0:
        assert torch.equal(w[allrows].float(), ow)
    else:
        fp32_close(w[allrows], ow)
    empty = c["valid"] < 0
    assert bool((lab[empty] == -1).all()) and float(w[empty].abs().max() if empty.any() else 0) == 0
    assert float(gb[empty].abs().max() if empty.any() else 0) == 0
    for b in range(B):
        rows = _packed(c, b)
        if not len(rows):
            continue
        if not c["multihot"][b].any():
            assert bool((lab[rows] == K).all()) and float(w[rows].abs().max()) == 0 and float(gb[rows].abs().max()) == 0
            continue
        own = c["rois5"][rows, 1:].double()
        assert bool((gb[rows][:, None, :] == own[None]).all(-1).any(1).all())
        iou = np.diagonal(ref.pairwise_iou(gb[rows].numpy(), own.numpy()))
        fgrows = (lab[rows] < K).numpy()
        assert (iou[fgrows] >= c["fg"] - 1e-7).all() and (iou[~fgrows] < c["fg"] + 1e-7).all()


@pytest.mark.parametrize("name", [n for n, v in C.OICR.items() if v[0] == 0 and v[1] > 1])
def test_oicr_hand_placed_rows(name):
    """the decisions the hand-placed rows were placed for, spelled out; the threshold rows sit on their thresholds bit for bit"""
    c = C.oicr_case(name)
    K, S, fg, bg = c["K"], c["S"], c["fg"], c["bg"]
    lab, w, gb = c["ref"]
    last = S - 1
    live = _packed(c, 0).tolist()
    assert [live[j] for j in c["info"]["picks"][0]] == [5, 20, last, 0, 0]          # cross-wave tie, lane tie, last row (not the junk slots), zeros
    t1 = 58 if S == 64 else (64 if S == 65 else S - 5)
    p = c["src"][:S, c["col0"]:c["col0"] + K]
    assert p[5, 1] == p[t1, 1] == 0.75 and (t1 // 64 > 0 or S == 64) and p[20, 4] == p[33, 4] == 0.5
    assert float(p[60:63].min()) == C.SENTINEL and bool((c["valid"][60:63] < 0).all()) and bool((lab[60:63] == -1).all())
    A = torch.tensor(C.GT_A).double()
    f32 = np.float32
    for r, (box, (num, den)) in C.THRESHOLD_ROWS.items():
        iou32 = f32(ref.pairwise_iou(A[None].numpy(), torch.tensor(box).double()[None].numpy())[0, 0])
        assert iou32 == f32(num) / f32(den) == f32(num / den)          # one correctly rounded division, in fp32 and as the rounded float64
        assert torch.equal(gb[r], A), r
        assert int(lab[r]) == (1 if iou32 >= f32(fg) else K), r
        assert float(w[r]) == (0.75 if iou32 >= f32(bg) else 0.0), r
    assert f32(200) / f32(400) == f32(0.5) and f32(40) / f32(400) == f32(0.1) and f32(240) / f32(400) == f32(0.6) and f32(120) / f32(400) == f32(0.3)
    on = {0.5: 41, 0.1: 44, 0.6: 47, 0.3: 48}
    assert int(lab[on[fg]]) == 1 and float(w[on[bg]]) == 0.75          # exactly fg is foreground, exactly bg keeps its weight
    assert int(lab[42]) == K and int(lab[43]) == (1 if fg == 0.5 else K) and float(w[45]) == 0.0
    # the same IoU (0.25) to A and B: the first; the same box twice (row 0): the first, class 11, score 0
    assert torch.equal(gb[C.EQUAL_IOU_ROW], A) and float(w[C.EQUAL_IOU_ROW]) == (0.75 if bg <= 0.25 else 0.0) and int(lab[C.EQUAL_IOU_ROW]) == K
    assert int(lab[0]) == 11 and float(w[0]) == 0.0 and torch.equal(gb[0], torch.tensor(C.GT_D).double())
    assert int(lab[5]) == 1 and int(lab[20]) == 4 and int(lab[last]) == 7 and float(w[last]) == 0.875 and float(w[20]) == 0.5
    # image 1: no label; image 2: nothing but empty slots
    assert bool((lab[S:2 * S] == K).all()) and bool((lab[2 * S:] == -1).all())


def test_oicr_cases_cover_the_shapes():
    assert {v[1] for v in C.OICR.values()} == {1, 64, 65, 200, 512, 1000, 1024} and {v[2] for v in C.OICR.values()} == {20, 80, 95}
    for mode in (0, 1):
        assert {v[1] for v in C.OICR.values() if v[0] == mode} == {1, 64, 65, 200, 512, 1000, 1024}
        assert {v[3] for v in C.OICR.values() if v[0] == mode} == {(0.5, 0.1), (0.6, 0.3)}


def test_stability_conditions():
    """the promises of weak_loss_cases.py's docstring, on every case (building a case asserts them; here none is left unbuilt)"""
    for name, v in C.OICR.items():
        c = C.oicr_case(name)
        assert not C._near_thresholds(c["info"], c["valid"], c["S"], c["fg"], c["bg"], c["constructed"]), name
        if v[0] == 1 and v[1] > 1:
            assert c["info"]["gap"] >= C.GAP, name
    ch = C.chain_case()
    m = C.mil_case(C.CHAIN)
    assert ch["info"]["gap"] >= C.GAP
    assert not C._near_thresholds(ch["info"], m["valid"], m["S"], 0.5, 0.1, set())
    # the chain's decisions are those of the fp32 x_r too
    lab32 = ref.oicr_targets(C.mil_ref(C.CHAIN, torch.float32)[1], 0, m["K"], ch["rois5"], m["valid"], m["S"], m["B"], m["multihot"])[0]
    assert torch.equal(lab32, ch["ref"][0])


# ---------------------------------------------------------------------------------------------------- cross-entropy, score assembly, loss sum
@pytest.mark.parametrize("name", list(C.CE))
def test_ce_reference_vs_torch(name):
    """F.cross_entropy (fp32, autograd) over the live rows gives the same loss and gradient; ignored rows are zero; all ignored: loss 0"""
    c = C.ce_case(name)
    loss, dy = C.ce_ref(name)
    live = c["labels"] >= 0
    assert float(dy[~live].abs().max() if (~live).any() else 0) == 0 and torch.isfinite(dy).all()
    if c["ignored"]:
        assert float(loss) == 0 and float(dy.abs().max()) == 0
        return
    x = c["logits"][live, c["col0"]:c["col0"] + c["ncls"]].clone().requires_grad_(True)
    w = c["weights"][live] if c["weights"] is not None else torch.ones(int(live.sum()))
    l = (F.cross_entropy(x, c["labels"][live].long(), reduction="none") * w).mean()
    (l * c["gscale"]).backward()
    fp32_close(loss, l.detach())
    assert torch.isfinite(x.grad).all()
    fp32_close(dy[live], x.grad)
    if "_inf" in name:
        assert bool(torch.isinf(x.detach()).any()) and float(dy[:, torch.isinf(x.detach()[0])].abs().max()) == 0


def test_ce_cases_cover_the_shapes():
    assert {(v[0], v[1]) for v in C.CE.values()} == {(n, r) for n in C.CE_NCLS for r in C.CE_ROWS}
    assert sum(v[5] for v in C.CE.values()) == 2
    for path in (lambda n: n <= 32, lambda n: n > 32):          # both row paths: beyond one grid sweep, with -inf, with zero weights, ignored
        vs = [v for v in C.CE.values() if path(v[0])]
        assert any(v[1] > 240 * 64 for v in vs) and any(v[3] for v in vs) and any(v[2] == "zeros" for v in vs) and any(v[5] for v in vs)
        assert any(v[2] == "none" for v in vs) and any(v[4] != 1.0 for v in vs)


@pytest.mark.parametrize("name", list(C.SUP))
def test_sup_scores_reference_vs_oracle_formula(name):
    """fast_rcnn.py:425-428: delta + mean of the stacked weak streams (+ extra), novel columns -inf -- torch's own mean agrees to fp32 rounding,
    and the mask is exact"""
    c = C.sup_case(name)
    n, k = c["ncls"], c["n_oicr"]
    got = ref.sup_scores(c["delta"], c["dcol0"], c["weak"], c["wcol0"], k, n, c["mask"], c["extra"], c["ecol0"])
    want = c["delta"][:, c["dcol0"]:c["dcol0"] + n].clone()
    if c["weak"] is not None:
        want = want + torch.stack([c["weak"][:, c["wcol0"] + t * n: c["wcol0"] + (t + 1) * n] for t in range(k)], 0).mean(0)
    if c["extra"] is not None:
        want = want + c["extra"][:, c["ecol0"]:c["ecol0"] + n]
    masked = torch.zeros(n, dtype=torch.bool)
    if c["mask"] is not None:
        masked[:n - 1] = c["mask"].bool()
        assert bool(masked.any()) and not bool(masked[n - 1])
    assert bool(torch.isneginf(got[:, masked]).all()) and torch.isfinite(got[:, ~masked]).all()
    close(got[:, ~masked], want[:, ~masked], rtol=1e-5, atol=1e-6)


def test_sum_losses_reference():
    for n in range(1, 10):
        v = C.sum_case(n)
        assert v.numel() == n and abs(float(ref.sum_losses(v.numpy())) - float(v.double().sum())) <= 1e-5
