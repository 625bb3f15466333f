"""Direct parity tests of csrc/roi_pool.hip against the host reference (roi_pool_ref.py) on the cases of roi_pool_cases.py
(test_roi_pool_cpu.py checks the reference against a second source and the cases against what is assumed of them here).

Everything is compared BIT FOR BIT: the forward copies an element and stores an index, the backward holds fp32 additions only, in the order
the reference adds in, and the epilogue is one addition, one select and one conversion (round to nearest even on both sides)."""
import functools

import numpy as np
import pytest
import torch

import roi_pool_cases as pc
import roi_pool_ref as ref

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]


def ops():
    from unit_amd import ops as o
    return o


def _count(k, dev):
    return torch.tensor([k], dtype=torch.int32, device=dev)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert torch.equal(_bits(got), _bits(want)), (what, int((_bits(got) != _bits(want)).sum()))


@functools.lru_cache(maxsize=None)
def _ref_fwd(kind, hw, mode, which="all", roi_count=None, image_offset=0):
    """-> (out float32, argmax int32) numpy [R, out, out, C_MAX]: computed once per case, sliced per channel count, never written"""
    pooled, out, step = mode
    rois = {"all": pc.rois(hw), "image1": pc.rois_one_image(hw, 1), "slots": pc.slot_rois(hw)}[which]
    f = pc.feat(kind, hw).numpy()[image_offset:]
    return ref.forward(f, pc.np_rois(rois), pooled, bins=pc.bins(pooled, out, step), roi_count=roi_count, image_offset=image_offset)


def _fwd(dev, f, rois, mode, want_argmax=True, **kw):
    pooled, out, step = mode
    am = torch.full((rois.shape[0], out, out, f.shape[3]), -7, dtype=torch.int32, device=dev) if want_argmax else None
    y = ops().roi_pool(f.to(dev), rois.to(dev), pooled, out, step, 1 / 16, argmax=am, **kw)
    return y.cpu(), (am.cpu() if want_argmax else None)


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("mode", pc.MODES)
@pytest.mark.parametrize("hw", pc.MAPS)
@pytest.mark.parametrize("kind", pc.KINDS)
def test_forward_value_and_argmax(dev, kind, hw, mode):
    """every map kind (tie-free, integer ties, the -0 / +0 tie, the all-NaN window), both maps, the four grids, fp32 and bf16, 1 / 8 / 9 / 128
    lanes: value and argmax equal the reference's bits; argmax = NULL gives the same values"""
    o_ref, a_ref = _ref_fwd(kind, hw, mode)
    for dtype in DTYPES:
        for c in pc.CHANNELS:
            f = pc.feat(kind, hw, c).to(dtype)
            got, am = _fwd(dev, f, pc.rois(hw), mode)
            _same(got, ref.to_dtype(o_ref[..., :c], dtype), (kind, hw, mode, dtype, c))
            assert torch.equal(am, torch.from_numpy(np.ascontiguousarray(a_ref[..., :c]))), (kind, hw, mode, dtype, c)
            if c in (8, 72):
                _same(_fwd(dev, f, pc.rois(hw), mode, want_argmax=False)[0], got, "argmax = NULL")
    if kind == "nan":          # -FLT_MAX in the output type where the window held nothing but NaN
        r = pc.index("one_pixel")
        live = ~ref.empty_bins(pc.np_rois(pc.rois(hw)), hw, mode[0], bins=pc.bins(*mode))[r]
        assert live.any() and (got[r][torch.from_numpy(live)] == float("-inf")).all() and (am[r] == -1).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hw", pc.MAPS)
def test_forward_roi_count_image_offset_and_unnamed_image(dev, hw, dtype):
    mode, c = (14, 7, 2), 72
    rois = pc.rois(hw)
    # slots at or past *roi_count_dev: zeros and argmax -1
    k = len(rois) - 5
    o_ref, a_ref = _ref_fwd("random", hw, mode, roi_count=k)
    got, am = _fwd(dev, pc.feat("random", hw, c).to(dtype), rois, mode, roi_count=_count(k, dev))
    _same(got, ref.to_dtype(o_ref[..., :c], dtype), "roi_count")
    assert torch.equal(am, torch.from_numpy(np.ascontiguousarray(a_ref[..., :c]))) and not got[k:].any() and (am[k:] == -1).all()
    # image_offset = 1: the map handed over starts at image 1, the RoIs' indices still count from image 0, the argmax stays image-local
    r1 = pc.rois_one_image(hw, 1)
    o_ref, a_ref = _ref_fwd("ties", hw, mode, which="image1", image_offset=1)
    o_all, a_all = _ref_fwd("ties", hw, mode, which="image1")
    assert np.array_equal(o_ref, o_all) and np.array_equal(a_ref, a_all)
    f = pc.feat("ties", hw, c).to(dtype)
    got, am = _fwd(dev, f[1:].contiguous(), r1, mode, image_offset=1)
    _same(got, ref.to_dtype(o_ref[..., :c], dtype), "image_offset")
    assert torch.equal(am, torch.from_numpy(np.ascontiguousarray(a_ref[..., :c])))
    got2, am2 = _fwd(dev, f, r1, mode)          # the same RoIs on the whole batch: image 0 is named by none of them
    _same(got2, got, "whole batch")
    assert torch.equal(am2, am)


# ------------------------------------------------------------------------------------------------ backward
def _bwd(dev, g, am, n_images, hw, rois, mode, out_dtype, **kw):
    pooled, out, step = mode
    res = torch.full((n_images, hw[0], hw[1], g.shape[3]), float("nan"), dtype=out_dtype, device=dev)          # fully written: no NaN survives
    kw = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in kw.items()}
    ops().roi_pool_bwd_gather(g.to(dev), am.to(dev), n_images, hw[0], hw[1], rois.to(dev), res, pooled, step, 1 / 16, **kw)
    return res.cpu()


@pytest.mark.parametrize("mode", pc.MODES)
@pytest.mark.parametrize("hw", pc.MAPS)
@pytest.mark.parametrize("kind", ["random", "ties"])
def test_backward_four_forms(dev, kind, hw, mode):
    """fp32 out plain / bf16 out / + addend / * (mask_ref > 0), and all of them together, at 1, 9 and 128 lanes. On the `ties` map many bins
    of a RoI name the same pixel (one_pixel: all of them), so the order of the additions shows in the bits."""
    rois = pc.rois(hw)
    _, a_ref = _ref_fwd(kind, hw, mode)
    g_all = pc.gout(len(rois), mode[1])
    acc = ref.backward_acc(g_all.numpy(), a_ref, (pc.N_IMAGES,) + hw, pc.np_rois(rois))
    add, msk = pc.addend(hw), pc.mask_ref(hw)
    for c in (8, 72, 1024):
        g, am = g_all[..., :c].contiguous(), torch.from_numpy(np.ascontiguousarray(a_ref[..., :c]))
        a_c, add_c, msk_c = acc[..., :c], add[..., :c].contiguous(), msk[..., :c].contiguous()
        _same(_bwd(dev, g, am, 2, hw, rois, mode, torch.float32), ref.to_dtype(a_c, torch.float32), ("plain", c))
        _same(_bwd(dev, g.bfloat16(), am, 2, hw, rois, mode, torch.bfloat16), ref.to_dtype(a_c, torch.bfloat16), ("bf16 out", c))
        _same(_bwd(dev, g.bfloat16(), am, 2, hw, rois, mode, torch.float32), ref.to_dtype(a_c, torch.float32), ("bf16 in, fp32 out", c))
        _same(_bwd(dev, g, am, 2, hw, rois, mode, torch.float32, addend=add_c, addend_images=2),
              ref.to_dtype(ref.epilogue(a_c, addend=add_c.numpy()), torch.float32), ("addend", c))
        _same(_bwd(dev, g, am, 2, hw, rois, mode, torch.float32, mask_ref=msk_c),
              ref.to_dtype(ref.epilogue(a_c, mask_ref=msk_c.numpy()), torch.float32), ("mask_ref", c))
        _same(_bwd(dev, g.bfloat16(), am, 2, hw, rois, mode, torch.bfloat16, addend=add_c.bfloat16(), addend_images=2, mask_ref=msk_c.bfloat16()),
              ref.to_dtype(ref.epilogue(a_c, addend=add_c.numpy(), mask_ref=msk_c.numpy()), torch.bfloat16), ("all, bf16", c))
    if hw == pc.MAPS[0]:          # one_pixel: its pixel holds the ordered sum of all of its gout (plus whatever other RoIs add there)
        y, x = pc.pixel(hw)
        assert (a_ref[pc.index("one_pixel")] == y * hw[1] + x).all()


@pytest.mark.parametrize("mode", [(14, 7, 2), (6, 6, 1)])
@pytest.mark.parametrize("hw", pc.MAPS)
def test_backward_fixed_slots_equal_the_table_walk(dev, hw, mode):
    """rois_per_image set (image i owns slots [i S, (i + 1) S), the last ones unused) against the walk over all R rows, and both against the
    reference; roi_count below R; image_offset = 1 on the second image's slots alone"""
    c, s = 72, pc.SLOTS
    rois = pc.slot_rois(hw)
    _, a_ref = _ref_fwd("ties", hw, mode, which="slots")
    am = torch.from_numpy(np.ascontiguousarray(a_ref[..., :c]))
    g = pc.gout(len(rois), mode[1])[..., :c].contiguous()
    want = ref.to_dtype(ref.backward_acc(g.numpy(), a_ref[..., :c], (2,) + hw, pc.np_rois(rois)), torch.float32)
    walk = _bwd(dev, g, am, 2, hw, rois, mode, torch.float32)
    slots = _bwd(dev, g, am, 2, hw, rois, mode, torch.float32, rois_per_image=s)
    _same(walk, want, "table walk")
    _same(slots, want, "fixed slots")
    k = s + 3          # image 1 keeps its first three RoIs
    wantk = ref.to_dtype(ref.backward_acc(g.numpy(), a_ref[..., :c], (2,) + hw, pc.np_rois(rois), roi_count=k), torch.float32)
    _same(_bwd(dev, g, am, 2, hw, rois, mode, torch.float32, roi_count=_count(k, dev)), wantk, "roi_count, walk")
    _same(_bwd(dev, g, am, 2, hw, rois, mode, torch.float32, roi_count=_count(k, dev), rois_per_image=s), wantk, "roi_count, slots")
    add = pc.addend(hw)[1:, ..., :c].contiguous()
    want1 = ref.to_dtype(ref.epilogue(ref.backward_acc(g[s:].numpy(), a_ref[s:, ..., :c], (1,) + hw, pc.np_rois(rois[s:]), image_offset=1),
                                      addend=add.numpy()), torch.float32)
    _same(want1, ref.to_dtype(ref.epilogue(want.numpy()[1:], addend=add.numpy()), torch.float32), "the reference's own slices agree")
    got1 = _bwd(dev, g[s:].contiguous(), am[s:].contiguous(), 1, hw, rois[s:].contiguous(), mode, torch.float32, rois_per_image=s, image_offset=1,
                addend=add, addend_images=1)
    _same(got1, want1, "image_offset")


def test_backward_image_no_roi_names_is_written_zero(dev):
    hw, mode, c = pc.MAPS[0], (7, 7, 1), 64
    r0 = pc.rois_one_image(hw, 0)
    f = pc.feat("random", hw, c)
    o_ref, a_ref = ref.forward(f.numpy(), pc.np_rois(r0), 7)
    got, am = _fwd(dev, f, r0, mode)
    _same(got, ref.to_dtype(o_ref, torch.float32), "forward")
    assert torch.equal(am, torch.from_numpy(a_ref))
    g = pc.gout(len(r0), 7)[..., :c].contiguous()
    d = _bwd(dev, g, am, 2, hw, r0, mode, torch.float32)
    _same(d, ref.to_dtype(ref.backward_acc(g.numpy(), a_ref, (2,) + hw, pc.np_rois(r0)), torch.float32), "backward")
    assert not d[1].any() and not torch.signbit(d[1]).any() and d[0].any()


# ------------------------------------------------------------------------------------------------ the model's three methods
def test_pool_bwd_accumulates_through_the_gather(dev):
    """WSROIHeadNoMeta.pool / pool_bwd under ROIPool: pool_bwd (the accumulate-into-dfeat32 form) is the gather with addend = dfeat32"""
    from unit_amd import config
    from unit_amd.modeling.roi_heads import WSROIHeadNoMeta
    hw, c = pc.MAPS[0], 1024
    cfg = config.voc_rcnn_c4_split1(50)
    cfg.MODEL.ROI_BOX_HEAD.POOLER_TYPE = "ROIPool"
    rh = WSROIHeadNoMeta(cfg)
    rois, f = pc.rois(hw), pc.feat("ties", hw, c)
    for pool_mode, mode in (("strided", (14, 7, 2)), ("full", (14, 14, 1))):
        rh.pool_mode = pool_mode
        o_ref, a_ref = _ref_fwd("ties", hw, mode)
        pooled, am = rh.pool_train(f.to(dev), rois.to(dev))
        _same(pooled.cpu(), ref.to_dtype(o_ref, torch.float32), pool_mode)
        assert torch.equal(am.cpu(), torch.from_numpy(a_ref))
        _same(rh.pool(f.to(dev), rois.to(dev)).cpu(), pooled.cpu(), "inference form")
        g = pc.gout(len(rois), mode[1])
        start = pc.addend(hw).to(dev)
        d = rh.pool_bwd(g.to(dev), (2,) + hw + (c,), rois.to(dev), start.clone(), argmax=am)
        acc = ref.backward_acc(g.numpy(), a_ref, (2,) + hw, pc.np_rois(rois))
        _same(d.cpu(), ref.to_dtype(ref.epilogue(acc, addend=start.cpu().numpy()), torch.float32), "pool_bwd")


# ------------------------------------------------------------------------------------------------ refused arguments
def test_unsupported_arguments_are_refused(dev):
    from unit_amd._lib import UnitLibError
    o = ops()

    def z(*shape, dt=torch.float32):
        return torch.zeros(shape, dtype=dt, device=dev)

    rois = pc.rois(pc.MAPS[0]).to(dev)[:4].contiguous()
    with pytest.raises(UnitLibError, match="C % 8"):
        o.roi_pool(z(2, 5, 7, 12), rois, 14, 7, 2)
    with pytest.raises(UnitLibError, match="exceed pooled_size"):
        o.roi_pool(z(2, 5, 7, 8), rois, 14, 8, 2)          # bins 0, 2, .., 14: the last is not one of the 14 x 14 grid
    with pytest.raises(UnitLibError, match="exceed pooled_size"):
        o.roi_pool_bwd_gather(z(4, 8, 8, 8), z(4, 8, 8, 8, dt=torch.int32), 2, 5, 7, rois, z(2, 5, 7, 8), 14, 2)
    with pytest.raises(UnitLibError, match="C % 8"):
        o.roi_pool_bwd_gather(z(4, 7, 7, 12), z(4, 7, 7, 12, dt=torch.int32), 2, 5, 7, rois, z(2, 5, 7, 12), 14, 2)
    with pytest.raises(UnitLibError, match="out dtype"):
        o.roi_pool_bwd_gather(z(4, 7, 7, 8), z(4, 7, 7, 8, dt=torch.int32), 2, 5, 7, rois, z(2, 5, 7, 8, dt=torch.bfloat16), 14, 2)
    from unit_amd._lib import lib
    assert lib().unit_roi_pool_argmax_bytes(2048, 7, 1024) == 2048 * 49 * 1024 * 4
    assert lib().unit_roi_pool_bwd_gather_workspace_bytes(0) > 0
