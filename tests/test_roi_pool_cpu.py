"""RoIPool without a GPU: the host reference (roi_pool_ref.py) against a second source and against its own brute-force restatement, the
preconditions test_roi_pool_ops_gpu.py / test_pooler_types_gpu.py rely on (roi_pool_cases.py), the pooler-type switch and the C ABI."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import roi_pool_cases as pc
import roi_pool_ref as ref

C_LOOP = 3          # channels the element-by-element restatements walk


# ---------------------------------------------------------------------------------------------------- second source: max_pool2d
@pytest.mark.parametrize("P,k", [(7, 2), (6, 2), (14, 1), (7, 1), (3, 4)])
def test_exact_tiling_rois_equal_max_pool2d(P, k):
    """x1 = 16 a, x2 = 16 (a + P k) - 16 (likewise y): the window is P k pixels a side and every bin exactly k x k, so the forward is
    max_pool2d(crop, k) and, on a tie-free map, the backward is autograd through it"""
    H, W, C = 16, 18, 5
    g = torch.Generator().manual_seed(7 + P + k)
    n = 2 * H * W
    f = (torch.argsort(torch.rand(n, C, generator=g), dim=0).float() - n // 2).reshape(2, H, W, C)          # tie-free
    corners = [(0, 0, 0), (1, 2, 1), (0, W - P * k, H - P * k)]          # (image, a_x, a_y)
    rois = np.array([[b, 16.0 * ax, 16.0 * ay, 16.0 * (ax + P * k) - 16, 16.0 * (ay + P * k) - 16] for b, ax, ay in corners], np.float32)
    out, arg = ref.forward(f.numpy(), rois, P)
    assert not ref.empty_bins(rois, (H, W), P).any()
    gout = torch.randn(len(rois), P, P, C, generator=g)
    got_d = ref.backward_acc(gout.numpy(), arg, (2, H, W), rois)
    want_d = torch.zeros(2, C, H, W)
    for r, (b, ax, ay) in enumerate(corners):
        x = f.permute(0, 3, 1, 2)[b:b + 1].clone().requires_grad_(True)
        y = F.max_pool2d(x[:, :, ay:ay + P * k, ax:ax + P * k], k)
        assert torch.equal(y[0].permute(1, 2, 0), torch.from_numpy(out[r])), r
        y.backward(gout[r].permute(2, 0, 1)[None])
        want_d[b] += x.grad[0]          # (the three windows of this test overlap in at most one image each: image 0 holds two)
    # image 0 receives two RoIs: both sides add them in RoI order, one fp32 addition per pixel
    assert torch.equal(torch.from_numpy(got_d), want_d.permute(0, 2, 3, 1))


def test_round_half_away_is_not_round_half_even():
    assert [ref.round_half_away(v) for v in (-0.5, 0.5, 1.5, 2.5, 3.5, -1.5, -2.5, 2.25, 2.75, -0.25, 0.0)] == [-1, 1, 2, 3, 4, -2, -3, 2, 3, 0, 0]
    b, x1, y1, bw, bh = ref.window(pc.named_rois(pc.MAPS[0])["halves"], 14)
    assert (b, x1, y1) == (1, -1, 2) and bw == np.float32(6) / np.float32(14) and bh == np.float32(2) / np.float32(14)
    assert np.rint(np.float32(2.5)) == 2          # what the reference must NOT use


# ---------------------------------------------------------------------------------------------------- brute force == vectorised
@pytest.mark.parametrize("mode", pc.MODES)
@pytest.mark.parametrize("hw", pc.MAPS)
@pytest.mark.parametrize("kind", pc.KINDS)
def test_loops_equal_the_vectorised_form(kind, hw, mode):
    pooled, out, step = mode
    f = pc.feat(kind, hw, C_LOOP).numpy()
    rois = pc.np_rois(pc.rois(hw))
    b = pc.bins(pooled, out, step)
    o1, a1 = ref.forward(f, rois, pooled, bins=b)
    o2, a2 = ref.forward_loops(f, rois, pooled, bins=b)
    assert np.array_equal(o1.view(np.int32), o2.view(np.int32)) and np.array_equal(a1, a2)          # bits: -0 is not +0 here
    g = pc.gout(len(rois), out)[..., :C_LOOP].numpy()
    d1 = ref.backward_acc(g, a1, (pc.N_IMAGES,) + hw, rois)
    d2 = ref.backward_loops(g, a1, (pc.N_IMAGES,) + hw, rois)
    assert np.array_equal(d1.view(np.int32), d2.view(np.int32))
    # the sum of a pixel's gradient over everything equals the sum of gout over the bins that selected something
    assert np.isclose(d1.astype(np.float64).sum(), g.astype(np.float64)[a1 >= 0].sum(), rtol=1e-5, atol=1e-3)


def test_roi_count_and_image_offset_in_the_reference():
    hw = pc.MAPS[0]
    f = pc.feat("random", hw, C_LOOP).numpy()
    rois = pc.np_rois(pc.rois(hw))
    o, a = ref.forward(f, rois, 7)
    oc, ac = ref.forward(f, rois, 7, roi_count=5)
    assert np.array_equal(oc[:5], o[:5]) and not oc[5:].any() and (ac[5:] == -1).all()
    r1 = pc.np_rois(pc.rois_one_image(hw, 1))
    o1, a1 = ref.forward(f, r1, 7)
    o2, a2 = ref.forward(f[1:], r1, 7, image_offset=1)
    assert np.array_equal(o1, o2) and np.array_equal(a1, a2)          # the argmax stays local to the image
    g = pc.gout(len(rois), 7)[..., :C_LOOP].numpy()
    assert np.array_equal(ref.backward_acc(g, a1, (2,) + hw, r1)[1:], ref.backward_acc(g, a2, (1,) + hw, r1, image_offset=1))


# ---------------------------------------------------------------------------------------------------- preconditions of the GPU files
@pytest.mark.parametrize("mode", pc.MODES)
@pytest.mark.parametrize("hw", pc.MAPS)
def test_case_preconditions(hw, mode):
    pooled, out, step = mode
    b = pc.bins(pooled, out, step)
    rois = pc.np_rois(pc.rois(hw))
    empty = ref.empty_bins(rois, hw, pooled, bins=b)
    live = ~empty
    tied = ref.tied_bins(pc.feat("ties", hw, 64).numpy(), rois, pooled, bins=b)
    assert tied.sum() >= live.sum() / 4, (tied.sum(), live.sum())          # a quarter of the bins that have a window at all
    for kind in ("random", "nan"):
        f = np.nan_to_num(pc.feat(kind, hw, 64).numpy(), nan=-1e30)          # (a NaN is never a maximum: below everything for this count)
        assert not ref.tied_bins(f, rois, pooled, bins=b).any(), kind
    zeros = pc.feat("zeros", hw, 8).numpy()          # every window of two or more pixels is a tie; both signs occur among the elements taken
    assert ref.tied_bins(zeros, rois, pooled, bins=b).any()
    oz = ref.forward(zeros, rois, pooled, bins=b)[0][live]
    assert not oz.any() and np.signbit(oz).any() and not np.signbit(oz).all()
    # every case lists its empty bins: the argmax is -1 there and only there on the tie-free map
    _, arg = ref.forward(pc.feat("random", hw, 8).numpy(), rois, pooled, bins=b)
    assert np.array_equal((arg == -1).all(-1), empty) and np.array_equal((arg == -1).any(-1), empty)
    assert empty[pc.index("outside")].all() and not empty[pc.index("whole")].any()
    assert empty[pc.index("partly")].any() and not empty[pc.index("partly")].all()
    if hw == pc.MAPS[0]:
        assert not empty[pc.index("one_pixel")].any() and not empty[pc.index("reversed")].any()
        assert empty[pc.index("halves")][:, 0].all() and not empty[pc.index("halves")][:, -1].any()          # x1 = -1: its first column is off the map
        y, x = pc.pixel(hw)
        assert (arg[pc.index("one_pixel")] == y * hw[1] + x).all()
        # narrow_x: narrower than the grid in x (one pixel in several bins of a row), not in y at the 6 and 7 grids
        _, x1, y1, bw, bh = ref.window(rois[pc.index("narrow_x")], pooled)
        assert bw < 1 and (bh >= 1) == (pooled <= 7)
    # the NaN map: one_pixel's windows hold nothing else
    o, a = ref.forward(pc.feat("nan", hw, 8).numpy(), rois, pooled, bins=b)
    op = o[pc.index("one_pixel")]
    assert (a[pc.index("one_pixel")] == -1).all() and ((op == -ref.FLT_MAX) | empty[pc.index("one_pixel")][..., None]).all()
    assert not np.isnan(o).any()
    assert torch.isinf(ref.to_dtype(np.float32([-ref.FLT_MAX]), torch.bfloat16)).all()


def test_slot_rois_follow_the_fixed_slot_rule():
    for hw in pc.MAPS:
        r = pc.slot_rois(hw)
        assert r.shape == (pc.N_IMAGES * pc.SLOTS, 5)
        assert torch.equal(r[:, 0], torch.arange(pc.N_IMAGES).repeat_interleave(pc.SLOTS).float())
        assert not r[pc.SLOTS - pc.SLOTS_EMPTY: pc.SLOTS, 1:].any()


def test_step_proposals_sit_on_the_lattice():
    for boxes, logits in pc.lattice_proposals(4, 100, (128, 192), 11):
        assert boxes.shape == (100, 4) and torch.equal(boxes, (boxes / pc.LATTICE).round() * pc.LATTICE)
        assert (boxes[:, 2] > boxes[:, 0]).all() and (boxes[:, 3] > boxes[:, 1]).all() and boxes.min() >= 0
        assert boxes[:, 2].max() <= 192 and boxes[:, 3].max() <= 128
        frac = (boxes / 16) % 1
        assert set(frac.unique().tolist()) <= {0.0, 0.25, 0.5, 0.75}
        assert (frac == 0.5).any()          # halves do occur: the rounding rule matters in the step tests
        assert (logits[:-1] >= logits[1:]).all()


def test_autograd_function_has_the_oracles_signature():
    import inspect

    import unit_oracle as orc
    assert str(inspect.signature(ref.roi_pool)) == str(inspect.signature(orc.roi_align))
    hw = pc.MAPS[0]
    f = pc.feat("random", hw, 8).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    rois = pc.rois(hw)
    y = ref.roi_pool(f, rois, 7)
    assert y.shape == (len(rois), 8, 7, 7)
    o, a = ref.forward(pc.feat("random", hw, 8).numpy(), pc.np_rois(rois), 7)
    assert torch.equal(y.detach().permute(0, 2, 3, 1), torch.from_numpy(o))
    g = pc.gout(len(rois), 7)[..., :8]
    y.backward(g.permute(0, 3, 1, 2))
    assert torch.equal(f.grad.permute(0, 2, 3, 1), torch.from_numpy(ref.backward_acc(g.numpy(), a, (2,) + hw, pc.np_rois(rois))))


# ---------------------------------------------------------------------------------------------------- config and C ABI
def _cfg(pooler):
    from unit_amd import config
    c = config.voc_rcnn_c4_split1(50)
    c.MODEL.DEVICE = "cpu"
    c.MODEL.ROI_BOX_HEAD.POOLER_TYPE = pooler
    return c


@pytest.mark.parametrize("pooler", ["ROIAlignV2", "ROIAlign", "ROIPool"])
def test_accepted_pooler_types_construct(pooler):
    from unit_amd.modeling import build_model
    rh = build_model(_cfg(pooler)).roi_heads
    assert rh.pooler_type == pooler and rh.max_pool == (pooler == "ROIPool")
    for mode, want in (("strided", (7, 2)), ("full", (14, 1))):
        rh.pool_mode = mode
        assert rh.pool_out == want


@pytest.mark.parametrize("pooler", ["ROIAlignRotated", "roipool", ""])
def test_other_pooler_types_are_refused_by_name(pooler):
    from unit_amd.modeling import build_model
    from unit_amd.modeling.inference import UnsupportedConfig
    with pytest.raises(UnsupportedConfig, match="MODEL.ROI_BOX_HEAD.POOLER_TYPE"):
        build_model(_cfg(pooler))


def test_header_declares_the_roi_pool_entries():
    from unit_amd import _lib
    protos, names = _lib.parse_header(), _lib.parse_header_names()
    assert names["unit_roi_pool_fwd"] == ["feat_nhwc", "dtype", "N", "H", "W", "C", "rois", "roi_count_dev", "R", "pooled_size", "out_size", "bin_step",
                                          "spatial_scale", "out", "argmax", "stream"]
    align = [a for a in names["unit_roi_align_bwd_gather"] if a not in ("sampling_ratio", "aligned")]
    assert names["unit_roi_pool_bwd_gather"] == align[:1] + ["argmax"] + align[1:]
    assert names["unit_roi_pool_argmax_bytes"] == ["R", "out_size", "C"] and names["unit_roi_pool_bwd_gather_workspace_bytes"] == ["R"]
    for n in ("unit_roi_pool_fwd", "unit_roi_pool_bwd_gather"):
        assert _lib.enqueues(n) and len(protos[n][1]) <= _lib.UnitCall.INTS          # a replayed step can carry them
    assert not _lib.enqueues("unit_roi_pool_argmax_bytes") and not _lib.enqueues("unit_roi_pool_bwd_gather_workspace_bytes")
    hdr = open(_lib.HEADER).read()
    assert "torchvision.ops.RoIPool" in hdr[hdr.index("unit_roi_pool_argmax_bytes") - 900: hdr.index("unit_roi_pool_argmax_bytes")]
    import os
    from unit_amd import build
    assert "roi_pool.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "roi_pool.hip"))
