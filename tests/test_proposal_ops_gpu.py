"""Direct parity tests of the training-time proposal path against the CPU oracle: csrc/boxes.hip (matrix_rowmax / matrix_match, iou_match /
low_quality, subsample, box_encode / box_decode, rpn_decode_select and its rows form, anchor_grid) and the RoI plumbing of csrc/losses.hip
(append_gt, roi_classes, gather_rois). The inputs (tests/proposal_cases.py) make every decision and every coordinate reproducible bit for
bit, so every comparison is torch.equal / np.array_equal; the one toleranced check (the logarithm columns of box_encode on general boxes)
keeps test_box_codec's tolerance. test_proposal_ops_cpu.py asserts that the cases contain what the tests below rely on."""
import os

import numpy as np
import pytest
import torch

import proposal_cases as pc
import unit_oracle as orc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "matcher_golden.npz")


def ops():
    from unit_amd import ops as o
    return o


def _d(t, dev):
    return None if t is None else t.to(dev)


# ------------------------------------------------------------------------------------------------ 1. matcher on a matrix
def _match_both_ways(dev, q, cfg):
    """-> [(idx, label, val)] on the CPU: through ops.match_matrix and through the plugin surface's Matcher class"""
    from unit_amd.modeling import Matcher
    th, lb, lq = pc.CONFIGS[cfg]
    outs = [ops().match_matrix(q.to(dev), th, lb, lq), Matcher(th, lb, allow_low_quality_matches=lq)(q.to(dev))]
    return [tuple(t.cpu() for t in out) for out in outs]


@pytest.mark.parametrize("cfg", list(pc.CONFIGS))
def test_match_matrix_recorded_cases(dev, cfg):
    """all ten recorded cases of the reference matcher, the adversarial matrices (ties, allbelow, zeros, emptyM, single) included"""
    gold = np.load(GOLDEN)
    names = sorted({k.split("/")[0] for k in gold.files})
    assert len(names) == 10
    for name in names:
        q = torch.from_numpy(gold[f"{name}/q"])
        for idx, lab, val in _match_both_ways(dev, q, cfg):
            assert idx.dtype == torch.int64 and lab.dtype == torch.int8 and val.dtype == torch.float32
            assert np.array_equal(idx.numpy(), gold[f"{name}/{cfg}/idx"]), name
            assert np.array_equal(lab.numpy(), gold[f"{name}/{cfg}/label"]), name
            assert np.array_equal(val.numpy(), gold[f"{name}/{cfg}/val"]), name


@pytest.mark.parametrize("cfg", list(pc.CONFIGS))
@pytest.mark.parametrize("name", list(pc.MATRIX_CASES))
def test_match_matrix_edges(dev, name, cfg):
    """N = 1 and around the block size, M = 1, M = 300 (no GT limit here), planted column ties and row-maximum ties"""
    q = pc.matrix_case(name)
    ridx, rlab, rval = pc.ref_match(q, cfg)
    for idx, lab, val in _match_both_ways(dev, q, cfg):
        assert torch.equal(idx, ridx) and torch.equal(lab, rlab) and torch.equal(val, rval)


# ------------------------------------------------------------------------------------------------ 2. fused matcher
def _iou_match(dev, gt, gt_count, boxes, box_count, cfg):
    th, lb, lq = pc.CONFIGS[cfg]
    return tuple(t.cpu() for t in ops().iou_match(_d(gt, dev), _d(gt_count, dev), _d(boxes, dev), _d(box_count, dev), th, lb, lq))


@pytest.mark.parametrize("cfg", list(pc.CONFIGS))
@pytest.mark.parametrize("form", ["shared", "per_image"])
@pytest.mark.parametrize("ncap", [255, 256, 257])
def test_iou_match_planted_batch(dev, ncap, form, cfg):
    """one launch over the six images of proposal_cases.MATCH_IMAGES: IoUs on the cut points and one float below, duplicate GTs, boxes
    tied for a GT's maximum, a GT that overlaps nothing, no GT, and (per-image form) a box_count below Ncap with NaN past it"""
    batch = pc.match_batch(ncap, form)
    ref = pc.ref_match_batch(*batch, cfg)
    got = _iou_match(dev, *batch, cfg)
    for name, g, r in zip(("idx", "label", "val"), got, ref):
        assert g.dtype == r.dtype and torch.equal(g, r), name
    if form == "per_image":
        s, n = pc.MATCH_IMAGES.index("short"), ncap - pc.SHORT_BY
        assert bool((got[0][s, n:] == 0).all()) and bool((got[1][s, n:] == -1).all()) and bool((got[2][s, n:] == 0).all())
        clean = _iou_match(dev, *pc.match_batch(ncap, form, junk=0.0), cfg)          # the same batch without the junk
        assert all(torch.equal(a, b) for a, b in zip(got, clean))
    orphan = pc.MATCH_IMAGES.index("orphan")
    assert bool((got[1][orphan] == 1).all()) == pc.CONFIGS[cfg][2]          # every box positive, under allow_low_quality only


def test_iou_match_gt_capacity(dev):
    """Mcap = 256 works (one image with 256 GTs, one with 3); Mcap = 257 is refused by the argument check before anything is launched"""
    from unit_amd._lib import UnitLibError
    gt, gt_count, boxes = pc.match_batch_mcap256()
    for cfg in pc.CONFIGS:
        ref = pc.ref_match_batch(gt, gt_count, boxes, None, cfg)
        got = _iou_match(dev, gt, gt_count, boxes, None, cfg)
        assert all(torch.equal(g, r) for g, r in zip(got, ref)), cfg
        assert int(got[0][0].max()) > 200
    wide = torch.zeros(2, 257, 4)
    with pytest.raises(UnitLibError, match="iou_match: Mcap > 256"):
        _iou_match(dev, wide, gt_count, boxes, None, "rpn")


# ------------------------------------------------------------------------------------------------ 3. sampler
@pytest.mark.parametrize("kind", ["int8", "int64"])
@pytest.mark.parametrize("n", pc.SAMPLER_SIZES)
def test_subsample_labels_regimes(dev, n, kind):
    """Ncap = Pcap below, at and above the block size (a chunk of 1 with idle threads, chunks straddling 1024); no positives, no negatives,
    nothing but -1, too few positives, too few candidates, and a count below Ncap whose permutation entries >= count are skipped"""
    labels, count, perm = pc.sampler_batch(n, kind)
    s, frac, bg = pc.sampler_params(n, kind)
    ref = pc.ref_sampler(labels, count, perm, s, frac, bg)
    got = ops().subsample_labels(labels.to(dev), count.to(dev), perm.to(dev), s, frac, bg)
    for name, g, r in zip(("labels", "sampled_idx", "counts"), got, ref):
        assert g.dtype == r.dtype and torch.equal(g.cpu(), r), name
    _, sidx, counts = ops().subsample_labels(labels.to(dev), count.to(dev), perm.to(dev), s, frac, bg, want_labels=False)
    assert torch.equal(sidx.cpu(), ref[1]) and torch.equal(counts.cpu(), ref[2])


# ------------------------------------------------------------------------------------------------ 4. codec
@pytest.mark.parametrize("n,k,weights", [(1, 1, pc.UNIT_WEIGHTS), (300, 1, pc.UNIT_WEIGHTS), (257, 3, pc.UNIT_WEIGHTS), (300, 20, pc.HEAD_WEIGHTS)])
def test_box_decode_exact(dev, n, k, weights):
    boxes, deltas = pc.exact_anchors(n, 80 + k), pc.exact_deltas(n, k, 90 + k, weights)
    got = ops().box_decode(deltas.to(dev), boxes.to(dev), weights).cpu()
    assert torch.equal(got, orc.apply_deltas(deltas, boxes, weights))


def test_box_decode_box_head_layout(dev):
    """deltas of 20 classes at column 21 of a 104-wide row (NaN everywhere else), weights (10, 10, 5, 5)"""
    rows, boxes = pc.head_layout_case()
    got = ops().box_decode(rows.to(dev), boxes.to(dev), pc.HEAD_WEIGHTS, k=pc.HEAD_K, col0=pc.HEAD_COL0).cpu()
    ref = orc.apply_deltas(rows[:, pc.HEAD_COL0: pc.HEAD_COL0 + 4 * pc.HEAD_K].contiguous(), boxes, pc.HEAD_WEIGHTS)
    assert got.shape == (rows.shape[0], 4 * pc.HEAD_K) and torch.equal(got, ref)


@pytest.mark.parametrize("weights", [pc.UNIT_WEIGHTS, pc.HEAD_WEIGHTS])
def test_box_encode_exact(dev, weights):
    """on the exact recipe (target = the decoded anchor) every column is reproducible: log(1) = 0"""
    for n in (1, 300):
        boxes, deltas = pc.exact_anchors(n, 50 + n), pc.exact_deltas(n, 1, 60 + n, weights)
        tgt = orc.apply_deltas(deltas, boxes, weights)
        got = ops().box_encode(boxes.to(dev), tgt.to(dev), weights).cpu()
        assert torch.equal(got, orc.get_deltas(boxes, tgt, weights)) and torch.equal(got, deltas)


@pytest.mark.parametrize("weights", [pc.UNIT_WEIGHTS, pc.HEAD_WEIGHTS])
def test_box_encode_general(dev, weights):
    """fractional boxes: the dx / dy columns are IEEE multiply, subtract and divide -- exact; the logarithm columns keep test_box_codec's
    tolerance"""
    src, tgt = pc.general_boxes(500, 1), pc.general_boxes(500, 2)
    ref = orc.get_deltas(src, tgt, weights)
    got = ops().box_encode(src.to(dev), tgt.to(dev), weights).cpu()
    assert torch.equal(got[:, :2], ref[:, :2])
    assert torch.allclose(got[:, 2:], ref[:, 2:], rtol=1e-5, atol=1e-5)


# ------------------------------------------------------------------------------------------------ 4. rpn decode / select
def _rpn_select(dev, ncap, topk, min_size):
    c = pc.rpn_case(ncap)
    out = ops().rpn_decode_select(c["head"].to(dev), pc.RPN_A, pc.RPN_COL0, c["anchors"].to(dev), c["sorted_idx"].to(dev),
                                  c["sorted_logit"].to(dev), topk, c["image_hw"].to(dev), min_size=min_size)
    return tuple(t.cpu() for t in out)


@pytest.mark.parametrize("min_size", pc.RPN_MIN_SIZES)
@pytest.mark.parametrize("ncap,topk", pc.RPN_CASES)
def test_rpn_decode_select_exact(dev, ncap, topk, min_size):
    """A = 3, ld = 16, three image sizes; topk up to 16384 runs rpn_decode_select_rows_kernel, above it rpn_decode_select_kernel. The count and
    the first `count` boxes and scores equal the reference's pre-NMS candidate list: non-finite rows dropped, strict > min_size, clipping per
    image, order kept across rows and waves"""
    cb, cs, cc = _rpn_select(dev, ncap, topk, min_size)
    ref = pc.rpn_candidates(ncap, topk, min_size)
    assert cc.dtype == torch.int32 and cc.tolist() == [r[1].numel() for r in ref]
    assert int(cc[pc.RPN_EMPTY_IMAGE]) == 0
    for i, (rb, rs) in enumerate(ref):
        n = rs.numel()
        assert torch.equal(cs[i, :n], rs), i
        assert torch.equal(cb[i, :n], rb), i


@pytest.mark.parametrize("min_size", pc.RPN_MIN_SIZES)
def test_rpn_decode_select_two_kernels_agree(dev, min_size):
    """the list at topk = 16384 (rows kernel) is a prefix of the list at 16385 (fallback kernel), which has one candidate more"""
    cb0, cs0, cc0 = _rpn_select(dev, 16386, 16384, min_size)
    cb1, cs1, cc1 = _rpn_select(dev, 16386, 16385, min_size)
    assert (cc1 - cc0).tolist() == [1, 1, 0]
    for i in range(len(pc.RPN_SIZES)):
        n = int(cc0[i])
        assert torch.equal(cb0[i, :n], cb1[i, :n]) and torch.equal(cs0[i, :n], cs1[i, :n])


def test_rpn_decode_select_refuses_topk_above_ncap(dev):
    from unit_amd._lib import UnitLibError
    with pytest.raises(UnitLibError, match="topk > Ncap"):
        _rpn_select(dev, 3, 4, 0.0)


# ------------------------------------------------------------------------------------------------ 5. RoI plumbing
@pytest.mark.parametrize("num_samples,frac", pc.ROI_SAMPLES)
def test_roi_plumbing_end_to_end(dev, num_samples, frac):
    """append_gt -> iou_match -> roi_classes -> subsample_labels -> gather_rois against label_and_sample_proposals, on one batch of an
    ordinary image, one without GT, one without proposals and one with fewer candidates than samples"""
    o = ops()
    c = {k: v.to(dev) for k, v in pc.roi_batch().items()}
    ref = pc.ref_roi_batch(num_samples, frac)
    s, k = num_samples, pc.ROI_K
    th, lb, lq = pc.CONFIGS["roi"]
    cat, cc = o.append_gt(c["props"], c["pcount"], c["gt"], c["gcount"])
    assert cc.tolist() == [p + g for p, g in zip(pc.ROI_PCOUNT, pc.ROI_GCOUNT)]
    idx, lab, _ = o.iou_match(c["gt"], c["gcount"], cat, cc, th, lb, lq)
    cls = o.roi_classes(idx, lab, cc, c["gt_classes"], c["gcount"], k)
    _, sidx, counts = o.subsample_labels(cls, cc, c["perm"], s, frac, k, want_labels=False)
    rois, rcls, rgt = o.gather_rois(cat, sidx, cls, idx, c["gt"], c["gcount"])
    cls, sidx, counts = cls.cpu(), sidx.cpu(), counts.cpu()
    rois, rcls, rgt = rois.cpu().view(-1, s, 5), rcls.cpu().view(-1, s), rgt.cpu().view(-1, s, 4)
    assert rcls.dtype == torch.int32
    for i, r in enumerate(ref):
        m = len(r["sampled_idx"])
        n = pc.ROI_PCOUNT[i] + pc.ROI_GCOUNT[i]
        assert int(counts[i].sum()) == m <= s and counts[i, 0] == int((r["gt_classes"] != k).sum())
        assert torch.equal(sidx[i, :m].long(), r["sampled_idx"]) and bool((sidx[i, m:] == -1).all())
        assert bool((rois[i, :, 0] == i).all())
        assert torch.equal(rois[i, :m, 1:], r["boxes"]) and bool((rois[i, m:, 1:] == 0).all())
        assert torch.equal(rcls[i, :m].long(), r["gt_classes"]) and bool((rcls[i, m:] == -1).all())
        assert torch.equal(rgt[i, :m], r["gt_boxes"]) and bool((rgt[i, m:] == 0).all())
        assert bool((cls[i, n:] == -1).all())
    img = pc.ROI_IMAGES.index
    n = pc.ROI_PCOUNT[img("no_gt")]
    assert bool((cls[img("no_gt"), :n] == k).all()) and bool((rgt[img("no_gt")] == 0).all()) and int(counts[img("no_gt"), 0]) == 0
    g = pc.ROI_GCOUNT[img("no_proposals")]
    assert counts[img("no_proposals")].tolist() == [min(g, int(s * frac)), 0]          # only the appended GT, each matched to itself
    assert torch.equal(rois[img("no_proposals"), : int(counts[img("no_proposals"), 0]), 1:], rgt[img("no_proposals"), : int(counts[img("no_proposals"), 0])])
    assert int(counts[img("few_candidates")].sum()) == pc.ROI_PCOUNT[3] + pc.ROI_GCOUNT[3] < s


def test_append_gt_clamps_pcount_and_zeroes_the_tail(dev):
    """pcount above Pcap counts as Pcap; the slots past pc + gc are zero; NaN past the counts is never copied"""
    gen = torch.Generator().manual_seed(3)
    pcap, mcap = 300, 8
    pcount, gcount = [pcap + 5, 3, 0, pcap], [2, mcap, 0, mcap]
    props, gt = torch.rand(4, pcap, 4, generator=gen) * 100, torch.rand(4, mcap, 4, generator=gen) * 100
    for i, (p, g) in enumerate(zip(pcount, gcount)):
        props[i, p:], gt[i, g:] = pc.NAN, pc.NAN
    cat, cc = ops().append_gt(props.to(dev), torch.tensor(pcount, dtype=torch.int32, device=dev), gt.to(dev),
                              torch.tensor(gcount, dtype=torch.int32, device=dev))
    assert cat.shape == (4, pcap + mcap, 4) and cc.dtype == torch.int32
    assert cc.tolist() == [pcap + 2, 3 + mcap, 0, pcap + mcap]
    for i, (p, g) in enumerate(zip(pcount, gcount)):
        p = min(p, pcap)
        want = torch.cat([props[i, :p], gt[i, :g], torch.zeros(pcap + mcap - p - g, 4)])
        assert torch.equal(cat[i].cpu(), want), i


# ------------------------------------------------------------------------------------------------ 6. anchor grid
@pytest.mark.parametrize("offset", pc.GRID_OFFSETS)
@pytest.mark.parametrize("h,w", pc.GRID_SHAPES)
def test_anchor_grid_edges(dev, h, w, offset):
    o = ops()
    got = o.anchor_grid(h, w, o.cell_anchors().to(dev), offset=offset).cpu()
    ref = orc.grid_anchors(h, w, offset=offset)
    assert got.shape == ref.shape == (h * w * 15, 4) and torch.equal(got, ref)
