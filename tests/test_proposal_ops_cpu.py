"""Preconditions of the proposal / sampling cases (tests/proposal_cases.py), asserted on the CPU reference alone: the GPU parity tests of
test_proposal_ops_gpu.py compare decisions bit for bit, and they mean something only if the cases really contain IoUs on the cut points,
ties, a GT without overlap, every sampler regime, an exact decode, and candidates that are dropped for each reason."""
import os

import numpy as np
import pytest
import torch

import proposal_cases as pc
import unit_oracle as orc

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "matcher_golden.npz")


# ------------------------------------------------------------------------------------------------ 1. matcher on a matrix
def test_golden_matrices_are_the_ten_recorded_cases():
    gold = np.load(GOLDEN)
    names = sorted({k.split("/")[0] for k in gold.files})
    assert len(names) == 10 and {"ties", "allbelow", "zeros", "emptyM", "single"} <= set(names)
    for name in names:
        q = torch.from_numpy(gold[f"{name}/q"])
        for cfg in pc.CONFIGS:          # the oracle's Matcher reproduces the recorded answers: one reference, two sources
            idx, lab, val = pc.ref_match(q, cfg)
            assert np.array_equal(idx.numpy(), gold[f"{name}/{cfg}/idx"]) and np.array_equal(lab.numpy(), gold[f"{name}/{cfg}/label"])
            assert np.array_equal(val.numpy(), gold[f"{name}/{cfg}/val"])


def test_planted_matrix_has_column_ties_row_ties_and_cut_points():
    q = pc.matrix_case("ties")
    best = q.max(dim=0).values
    tied_cols = (q == best[None]).sum(0) > 1
    assert int(tied_cols.sum()) >= 10          # several GTs share a column's maximum: the first one wins
    idx, lab, val = pc.ref_match(q, "rpn")
    first = torch.stack([(q[:, n] == best[n]).nonzero()[0, 0] for n in range(q.shape[1])])
    assert torch.equal(idx, first)
    rowmax = q.max(dim=1).values
    assert bool(((q == rowmax[:, None]).sum(1) > 1).all())          # every row maximum is shared ...
    shared = (q == rowmax[:, None]).any(0)
    assert bool((lab[shared] == 1).all()) and int((shared & (val < 0.7)).sum()) > 0          # ... and lifts columns that the thresholds would not
    th = torch.tensor([0.3, 0.5, 0.7], dtype=torch.float32)
    for t in th:
        assert bool((val == t).any()) and bool((val == torch.nextafter(t, torch.tensor(0.0))).any())
    assert int((pc.ref_match(q, "roi")[1] == 0).sum()) > 0 and int((pc.ref_match(q, "roi")[1] == 1).sum()) > 0


def test_matrix_case_shapes():
    assert {pc.MATRIX_CASES[k][1] for k in ("n1", "n255", "n256", "n257")} == {1, 255, 256, 257}
    assert pc.MATRIX_CASES["m1"][0] == 1 and pc.MATRIX_CASES["m300"][0] == 300
    for name in pc.MATRIX_CASES:
        assert pc.matrix_case(name).shape == pc.MATRIX_CASES[name]
        if pc.MATRIX_CASES[name][1] > 1:
            assert len(set(pc.ref_match(pc.matrix_case(name), "roi")[1].tolist())) == 2, name
            if pc.MATRIX_CASES[name][0] <= 5:          # (300 row maxima lift every one of the 130 columns)
                assert len(set(pc.ref_match(pc.matrix_case(name), "rpn")[1].tolist())) >= 2, name


# ------------------------------------------------------------------------------------------------ 2. fused matcher
def _f32(x):
    return torch.tensor(x, dtype=torch.float32)


def test_integer_boxes_hit_the_cut_points_and_the_float_below():
    g0 = _f32([pc.G0])
    for t, name in ((0.3, "at0.3"), (0.5, "at0.5"), (0.7, "at0.7")):
        assert orc.pairwise_iou(g0, _f32([pc.HEAD_BOXES[name]]))[0, 0] == _f32(t)
        below = orc.pairwise_iou(_f32([pc.TAIL_BOXES[f"gt{t}"]]), _f32([pc.TAIL_BOXES[f"below{t}"]]))[0, 0]
        assert below == torch.nextafter(_f32(t), _f32(0.0)), (t, float(below))


@pytest.mark.parametrize("ncap", [255, 256, 257])
def test_match_batch_contains_what_it_claims(ncap):
    gt, gt_count, boxes, _ = pc.match_batch(ncap, "shared")
    assert boxes.shape == (ncap, 4) and torch.equal(boxes, boxes.round())
    assert int(gt_count.max()) == pc.MATCH_MCAP == gt.shape[1]
    at = lambda name: pc.planted_index(name, ncap)
    assert at("below0.7") == ncap - 1
    rpn, roi = pc.ref_match_batch(gt, gt_count, boxes, None, "rpn"), pc.ref_match_batch(gt, gt_count, boxes, None, "roi")
    img = pc.MATCH_IMAGES.index
    # thresholds: a value ON a cut point belongs to the interval above it, the float below to the one beneath
    i = img("thresholds")
    assert [float(rpn[2][i, at(n)]) for n in ("at0.3", "at0.5", "at0.7")] == [float(_f32(0.3)), 0.5, float(_f32(0.7))]
    assert [int(rpn[1][i, at(n)]) for n in ("at0.3", "below0.3", "at0.7", "below0.7")] == [-1, 0, 1, -1]
    assert [int(roi[1][i, at(n)]) for n in ("at0.5", "below0.5")] == [1, 0]
    assert [int(rpn[0][i, at(n)]) for n in ("below0.3", "below0.5", "below0.7")] == [1, 2, 3]
    # duplicates: GTs 0, 1 and 3 are one box; nothing is ever matched to 1 or 3
    i = img("duplicates")
    assert int((rpn[2][i] > 0).sum()) > 20 and set(rpn[0][i].tolist()) == {0, 2}
    # rowties: three boxes at IoU 0.5 share TIE_GT's maximum: all three are 1 with low-quality matches, and only then
    i = img("rowties")
    ties = [at("tie0"), at("tie1"), at("tie2")]
    assert rpn[2][i, ties].tolist() == [0.5] * 3 and rpn[1][i, ties].tolist() == [1] * 3
    assert float(orc.pairwise_iou(_f32([pc.TIE_GT]), boxes).max()) == 0.5
    # orphan: a GT with a row maximum of 0 makes every box of the image positive under allow_low_quality, and changes nothing without
    i = img("orphan")
    assert float(orc.pairwise_iou(_f32([pc.ORPHAN_GT]), boxes).max()) == 0.0
    assert bool((rpn[1][i] == 1).all()) and int((rpn[2][i] == 0).sum()) > 10
    assert int((roi[1][i] == 0).sum()) > 10 and int((roi[1][i] == 1).sum()) > 0
    others = [j for j in range(len(pc.MATCH_IMAGES)) if j != i]
    assert all(int((rpn[1][j] != 1).sum()) > 10 for j in others)
    # nogt: everything is labels[0]
    i = img("nogt")
    assert int(gt_count[i]) == 0 and bool((rpn[1][i] == 0).all()) and bool((rpn[0][i] == 0).all()) and bool((rpn[2][i] == 0).all())


def test_short_image_junk_is_nan_and_its_reference_ignores_it():
    ncap = 257
    gt, gt_count, boxes, count = pc.match_batch(ncap, "per_image")
    s = pc.MATCH_IMAGES.index("short")
    n = int(count[s])
    assert n == ncap - pc.SHORT_BY and torch.isnan(boxes[s, n:]).all() and torch.isfinite(boxes[s, :n]).all()
    assert count.tolist() == [ncap] * s + [n]
    assert torch.isnan(gt[0, int(gt_count[0]):]).all()          # GT slots past the count are junk too
    idx, lab, val = pc.ref_match_batch(gt, gt_count, boxes, count, "rpn")
    assert bool((idx[s, n:] == 0).all()) and bool((lab[s, n:] == -1).all()) and bool((val[s, n:] == 0).all())
    clean = pc.ref_match_batch(*pc.match_batch(ncap, "per_image", junk=0.0), "rpn")
    assert all(torch.equal(a, b) for a, b in zip((idx, lab, val), clean))


# ------------------------------------------------------------------------------------------------ 3. sampler
@pytest.mark.parametrize("kind", ["int8", "int64"])
@pytest.mark.parametrize("n", pc.SAMPLER_SIZES)
def test_sampler_batch_contains_every_regime(n, kind):
    labels, count, perm = pc.sampler_batch(n, kind)
    s, frac, bg = pc.sampler_params(n, kind)
    max_pos = int(s * frac)
    assert labels.shape == perm.shape == (len(pc.SAMPLER_IMAGES), n)
    assert int(perm.min()) >= 0 and int(perm.max()) < n
    assert all(sorted(p.tolist()) == list(range(n)) for p in perm)
    out, sidx, counts = pc.ref_sampler(labels, count, perm, s, frac, bg)
    img = pc.SAMPLER_IMAGES.index
    assert counts[img("no_pos")][0] == 0 and counts[img("no_neg")][1] == 0 and counts[img("all_ignored")].tolist() == [0, 0]
    assert bool((out[img("all_ignored")] == -1).all()) and bool((sidx[img("all_ignored")] == -1).all())
    short = img("short_count")
    assert int(count[short]) < n or n == 1
    assert bool((out[short, int(count[short]):] == -1).all())
    assert int((sidx[short] >= int(count[short])).sum()) == 0
    if n > 5:
        assert counts[img("mixed")].tolist() == [max_pos, s - max_pos]                      # both classes cut off
        assert counts[img("no_pos")].tolist() == [0, s] and counts[img("no_neg")].tolist() == [max_pos, 0]
        few = counts[img("few_pos")].tolist()
        assert 0 < few[0] < max_pos and sum(few) == s                                        # negatives fill up
        cand = counts[img("few_candidates")].tolist()
        assert cand[0] > 0 and cand[1] > 0 and sum(cand) < s and int((sidx[img("few_candidates")] == -1).sum()) == s - sum(cand)
        assert int((perm[short] >= int(count[short])).sum()) > 100                            # entries the kernel has to skip
        assert int(counts[short][0]) == max_pos and int(counts[short][1]) > 0
        if kind == "int64":
            assert int((labels[img("mixed")] == 0).sum()) > 0                                # class 0 is a positive


# ------------------------------------------------------------------------------------------------ 4. codec
def _decodes_exactly(deltas, boxes, weights):
    d32 = orc.apply_deltas(deltas, boxes, weights)
    d64 = orc.apply_deltas(deltas.double(), boxes.double(), weights)
    assert d32.dtype == torch.float32 and d64.dtype == torch.float64
    assert torch.equal(d32.double(), d64)                  # fp32 and fp64 agree bit for bit ...
    assert torch.equal(d64 * 8.0, (d64 * 8.0).round())     # ... on multiples of 1/8
    return d32


def test_exact_recipe_decodes_to_the_same_bits_in_fp32_and_fp64():
    moved = 0
    for k, w, seed in ((1, pc.UNIT_WEIGHTS, 1), (3, pc.UNIT_WEIGHTS, 2), (pc.HEAD_K, pc.HEAD_WEIGHTS, 3)):
        boxes = pc.exact_anchors(300, 30 + seed)
        dec = _decodes_exactly(pc.exact_deltas(300, k, 40 + seed, w), boxes, w)
        moved += int((dec.reshape(300, k, 4) != boxes[:, None]).any(-1).sum())
    assert moved > 300
    rows, boxes = pc.head_layout_case()
    assert rows.shape[1] == pc.HEAD_LD == pc.HEAD_COL0 + 4 * pc.HEAD_K + 3
    inner = rows[:, pc.HEAD_COL0: pc.HEAD_COL0 + 4 * pc.HEAD_K]
    assert torch.isfinite(inner).all() and torch.isnan(rows[:, : pc.HEAD_COL0]).all() and torch.isnan(rows[:, pc.HEAD_COL0 + 4 * pc.HEAD_K:]).all()
    _decodes_exactly(inner, boxes, pc.HEAD_WEIGHTS)


def test_exact_recipe_encodes_back_exactly():
    """get_deltas of (anchor, decoded box) returns the planted deltas: the log columns are log(1) = 0"""
    for w, seed in ((pc.UNIT_WEIGHTS, 1), (pc.HEAD_WEIGHTS, 2)):
        boxes, deltas = pc.exact_anchors(300, 50 + seed), pc.exact_deltas(300, 1, 60 + seed, w)
        back = orc.get_deltas(boxes, orc.apply_deltas(deltas, boxes, w), w)
        assert torch.equal(back, deltas)
        assert torch.equal(back.double(), orc.get_deltas(boxes.double(), orc.apply_deltas(deltas.double(), boxes.double(), w), w))


# ------------------------------------------------------------------------------------------------ 4. rpn decode / select
def _clean_deltas(case):
    d = case["deltas"].clone()
    d[~torch.isfinite(d) | (d.abs() > 1.0)] = 0.0          # (the planted rows: not part of the exact recipe)
    return d


@pytest.mark.parametrize("ncap", [c for c in pc.RPN_LARGE] + [3])
def test_rpn_case_layout_and_exact_decode(ncap):
    c = pc.rpn_case(ncap)
    b = len(pc.RPN_SIZES)
    assert ncap % pc.RPN_A == 0 and c["head"].shape == (b, ncap // pc.RPN_A, pc.RPN_LD)
    assert len({hw for hw in pc.RPN_SIZES}) == 3
    assert torch.isnan(c["head"][:, :, pc.RPN_LD - 1]).all()          # the padding column is junk
    assert torch.equal(c["anchors"], c["anchors"].round()) and bool(((c["anchors"][:, 2:] - c["anchors"][:, :2]) % 2 == 0).all())
    for i in range(b):
        assert sorted(c["sorted_idx"][i].tolist()) == list(range(ncap))          # always valid indices
        assert torch.equal(c["sorted_logit"][i], c["logits"][i][c["sorted_idx"][i].long()])
        _decodes_exactly(_clean_deltas(c)[i], c["anchors"], pc.UNIT_WEIGHTS)
    if ncap > 3:
        for row in c["logits"]:
            assert row.unique().numel() == row.numel()          # survivors can be told apart by their logit


@pytest.mark.parametrize("ncap,topk", pc.RPN_CASES)
def test_rpn_cases_contain_what_they_claim(ncap, topk):
    c = pc.rpn_case(ncap)
    for min_size in pc.RPN_MIN_SIZES:
        cands = pc.rpn_candidates(ncap, topk, min_size)
        assert cands[pc.RPN_EMPTY_IMAGE][1].numel() == 0          # every anchor lies right of the 24 px image
        for i in (0, 1):
            boxes, logit = cands[i]
            h, w = pc.RPN_SIZES[i]
            assert torch.isfinite(boxes).all() and torch.isfinite(logit).all()
            wd, ht = boxes[:, 2] - boxes[:, 0], boxes[:, 3] - boxes[:, 1]
            assert bool((wd > min_size).all()) and bool((ht > min_size).all())
            if ncap == 3:
                continue
            assert 0.2 * topk <= logit.numel() <= 0.8 * topk, (i, logit.numel())
            assert bool((boxes[:, 0] == 0).any() or (boxes[:, 1] == 0).any()) and bool((boxes[:, 2] == w).any()) and bool((boxes[:, 3] == h).any())
            # dw = +inf is kept: clamped, it spans the whole image width; nothing else does
            assert int(((boxes[:, 0] == 0) & (boxes[:, 2] == w)).sum()) == len(pc.KEEP_KINDS)
            # survivors on both sides of every 1024 boundary, within one wave of it
            alive = torch.isin(c["sorted_logit"][i, :topk], logit)
            assert int(alive.sum()) == logit.numel()
            for edge in range(1024, topk, 1024):
                assert bool(alive[edge - 64: edge].any()) and bool(alive[edge: min(edge + 64, topk)].any()), (i, edge)
            assert bool(alive[topk - 1 if topk < ncap else topk - 2])          # the last entry survives (the last but one where the -inf logit is in), ...
            if topk % 1024 in (1, 2):          # ... and so do both neighbours of the 1024 boundary just before it
                edge = topk - topk % 1024
                assert bool(alive[edge - 1]) and bool(alive[edge]), (i, edge)
    if ncap == 3:
        assert [pc.rpn_candidates(3, 3, 0.0)[i][1].numel() for i in range(3)] == [2, 2, 0] and topk == ncap
        assert [pc.rpn_candidates(3, 3, 4.0)[i][1].numel() for i in range(3)] == [1, 2, 0]
        return
    # a box whose clipped width equals min_size exactly is dropped: present at min_size 0, gone at 4
    lo, hi = pc.rpn_candidates(ncap, topk, 0.0), pc.rpn_candidates(ncap, topk, 4.0)
    for i in (0, 1):
        w0 = lo[i][0][:, 2] - lo[i][0][:, 0]
        assert int((w0 == 4.0).sum()) >= 3 and lo[i][1].numel() > hi[i][1].numel()
    clipped_to_4 = (lo[0][0][:, 2] == pc.RPN_SIZES[0][1]) & (lo[0][0][:, 0] == pc.RPN_SIZES[0][1] - 4)
    assert int(clipped_to_4.sum()) >= 1
    # the -inf logit sorts last: one of the first topk entries only where topk = Ncap
    for i in (0, 1):
        assert c["sorted_logit"][i, ncap - 1] == -pc.INF and c["sorted_logit"][i, 0] == pc.INF


@pytest.mark.parametrize("ncap,topk", [(1026, 1023), (16386, 16386)])
@pytest.mark.parametrize("kind", pc.RPN_KINDS)
def test_each_planted_kind_drops_or_keeps_its_rows(ncap, topk, kind):
    """against the same case without that one kind: every drop reason removes at least one candidate per image, dw = +inf removes none"""
    without = tuple(k for k in pc.RPN_KINDS if k != kind)
    n_rows = sum(1 for (img, _, k) in pc.rpn_plan(ncap) if k == kind and img == 0)
    for i in (0, 1):
        full, less = pc.rpn_candidates(ncap, topk, 0.0)[i][1].numel(), pc.rpn_candidates(ncap, topk, 0.0, without)[i][1].numel()
        if kind == "neg_inf_logit" and topk < ncap:          # (the last entry of the order is not one of the first topk)
            assert less == full
        elif kind in pc.DROP_KINDS:
            assert less - full == n_rows >= 1, (kind, i, less, full)
        else:
            assert less == full


# ------------------------------------------------------------------------------------------------ 5. RoI plumbing
@pytest.mark.parametrize("num_samples,frac", pc.ROI_SAMPLES)
def test_roi_batch_contains_what_it_claims(num_samples, frac):
    c = pc.roi_batch()
    ref = pc.ref_roi_batch(num_samples, frac)
    img = pc.ROI_IMAGES.index
    k, max_pos = pc.ROI_K, int(num_samples * frac)
    assert c["pcount"].tolist() == list(pc.ROI_PCOUNT) and c["gcount"].tolist() == list(pc.ROI_GCOUNT)
    for i in range(len(pc.ROI_IMAGES)):
        assert torch.isnan(c["props"][i, pc.ROI_PCOUNT[i]:]).all() and torch.isnan(c["gt"][i, pc.ROI_GCOUNT[i]:]).all()
    assert int(c["perm"].min()) >= 0 and int(c["perm"].max()) < pc.ROI_PCAP + pc.ROI_MCAP
    ordinary = ref[img("ordinary")]
    assert len(ordinary["sampled_idx"]) == num_samples and int((ordinary["gt_classes"] != k).sum()) == max_pos          # both classes cut off
    assert int((ordinary["sampled_idx"] >= pc.ROI_PCOUNT[0]).sum()) > 0                                                # an appended GT is sampled
    no_gt = ref[img("no_gt")]
    assert bool((no_gt["gt_classes"] == k).all()) and bool((no_gt["gt_boxes"] == 0).all())
    assert len(no_gt["sampled_idx"]) == min(num_samples, pc.ROI_PCOUNT[1])
    no_props = ref[img("no_proposals")]
    assert len(no_props["sampled_idx"]) == pc.ROI_GCOUNT[2] and bool((no_props["gt_classes"] != k).all())
    few = ref[img("few_candidates")]
    assert len(few["sampled_idx"]) == pc.ROI_PCOUNT[3] + pc.ROI_GCOUNT[3] < num_samples
    assert 0 < int((few["gt_classes"] != k).sum()) < len(few["sampled_idx"])
