"""Direct parity tests of csrc/roi_align.hip at the edges of the sampling rule, every kernel variant and every argument reached:
roi_align_fwd_kernel<float, 0> / <bf16, 2> / <bf16, 0>, roi_align_fwd_row_kernel (merged taps and its per-sample loop), the atomic
backward, roi_geom_kernel + the gather backward with its fused epilogue (and unit_add_cast, which the epilogue replaces).

Two references (tests/test_roi_align_ops_cpu.py checks one against the other and the cases they run on, roi_align_cases.py):
  the oracle's float32 loop   the fp32 forward and every bf16 variant that keeps the reference's order are compared bit for bit
  the fp64 matrix form        roi_align_ref.py, with derived bounds; A = forward_abs, B = backward_abs, n = terms_per_pixel:
      bf16 merged taps   |got - ref| <= 2^-8 |ref| + 2^-18 A            bf16's half ulp + the float32 roundings of the other association
      backward, fp32     |got - ref| <= (16 + n) 2^-24 B                 each term a few roundings, n float32 accumulations
      backward, bf16 out |got - ref| <= 2^-8 |ref| + (16 + n) 2^-24 B
All inputs are finite and every batch index is in range."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import roi_align_cases as rc
import roi_align_ref as ref
import unit_oracle as orc

pytestmark = pytest.mark.gpu

HW = rc.MAPS[0]
SRS = [0, 1, 2, 3]
NAN = float("nan")


def ops():
    from unit_amd import ops as o
    return o


def _count(k, dev):
    return torch.tensor([k], dtype=torch.int32, device=dev)


def _oracle_fwd(hw, c, P, sr, aligned, rois=None):
    """-> [R, P, P, c] fp32 (torch): the oracle's float32 loop on the map of the cases"""
    rois = rc.np_rois() if rois is None else rois
    return rc.nhwc(torch.from_numpy(orc.roi_align_forward(rc.nchw(rc.feat(hw, c)).numpy(), rois, P, 1 / 16, sr, aligned)))


@functools.lru_cache(maxsize=None)
def _oracle_fwd_small(hw, P, sr, aligned):
    return _oracle_fwd(hw, 72, P, sr, aligned)


def _strided(full, out, step):
    return full[:, ::step, ::step][:, :out, :out].contiguous()


def _check_merged(got, f, rois, P, sr, aligned, bins, what):
    """the merged-tap bound |got - ref64| <= 2^-8 |ref64| + 2^-18 A on the bf16 result `got` of the RoIs `rois` (numpy)"""
    r64, a = ref.forward(f.numpy(), rois, P, sr, aligned, bins=bins), ref.forward_abs(f.numpy(), rois, P, sr, aligned, bins=bins)
    err, bound = np.abs(got.float().numpy().astype(np.float64) - r64), 2.0 ** -8 * np.abs(r64) + 2.0 ** -18 * a
    m = bound > 0
    print(f"merged {what}: {float((err[m] / bound[m]).max()) if m.any() else 0.0:.3f} of the bound")
    assert (err <= bound).all(), what


def _fwd(dev, f, rois, mode, sr, aligned=True, **kw):
    pooled, out, step = mode
    return ops().roi_align(f.to(dev), rois.to(dev), pooled, out, step, 1 / 16, sr, aligned, **kw).cpu()


# ------------------------------------------------------------------------------------------------ forward, fp32
@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("hw", rc.MAPS)
def test_forward_fp32_bit_equal_to_the_oracle(dev, hw, aligned):
    """roi_align_fwd_kernel<float, 0>: same operations in the same order, no contraction -> the oracle's bits, for every sampling ratio,
    full and strided grids of 14 and 7, maps with H = 1 and / or W = 1"""
    f, rois = rc.feat(hw, 72), rc.rois()
    for sr in SRS:
        for mode in rc.MODES:
            pooled, out, step = mode
            want = _strided(_oracle_fwd_small(hw, pooled, sr, aligned), out, step)
            got = _fwd(dev, f, rois, mode, sr, aligned)
            assert got.shape == want.shape and np.array_equal(got.numpy(), want.numpy()), (sr, mode)


@pytest.mark.parametrize("c", rc.CHANNELS)
def test_forward_fp32_widths_count_and_image_offset(dev, c):
    """1, 9, 65 and 128 lanes; roi_count below R (the slots past it exactly 0, the others unchanged); image_offset = 1 on feat[1:] with
    the batch indices left as they are"""
    f, rois, r = rc.feat(HW, c), rc.rois(), len(rc.rois())
    for sr in (0, 2):
        for mode in ((14, 14, 1), (14, 7, 2)):
            want = _strided(_oracle_fwd(HW, c, 14, sr, True), mode[1], mode[2])
            got = _fwd(dev, f, rois, mode, sr)
            assert np.array_equal(got.numpy(), want.numpy()), (sr, mode)
            k = r - 7
            out = torch.full(want.shape, NAN, device=dev)
            got_c = _fwd(dev, f, rois, mode, sr, roi_count=_count(k, dev), out=out)
            assert torch.equal(got_c[:k], got[:k]) and bool((got_c[k:] == 0).all())
            one = rois[:, 0] == 1
            fd = f.to(dev)
            got_o = ops().roi_align(fd[1:], rois[one].to(dev), mode[0], mode[1], mode[2], 1 / 16, sr, True, image_offset=1).cpu()
            assert int(one.sum()) > 10 and torch.equal(got_o, got[one])


def test_forward_small_launches(dev):
    """R = 0 returns an empty tensor (no launch); R = 1 with out = 7 is 49 bins; grids of fewer workgroups than the 8 XCDs the work is dealt
    over (1, 2, 4 and 7 of them), fp32 (one workgroup a bin) and bf16 (one a row of bins)"""
    f = rc.feat(HW, 72)
    for dtype in (torch.float32, torch.bfloat16):
        empty = ops().roi_align(f.to(dev).to(dtype), torch.zeros(0, 5, device=dev), 14, 7, 2, 1 / 16, 2, True)
        assert empty.shape == (0, 7, 7, 72)
    torch.cuda.synchronize()
    for name in ("whole", "top_left", "grid_3x1"):
        one = rc.rois()[rc.index(name)][None]
        for sr in (0, 2):
            for mode in ((14, 7, 2), (14, 1, 1), (14, 2, 1), (7, 4, 2)):
                pooled, out, step = mode
                want = _strided(_oracle_fwd_small(HW, pooled, sr, True)[rc.index(name)][None], out, step)
                assert np.array_equal(_fwd(dev, f, one, mode, sr).numpy(), want.numpy()), (name, sr, mode)
                got_b = _fwd(dev, f.bfloat16(), one, mode, sr)          # grid <= 2 x 2: merged taps, else the reference's order
                if max(ref.grid(one[0].numpy(), pooled, sr)) > 2:
                    assert torch.equal(got_b, want.bfloat16()), (name, sr, mode)
                else:
                    _check_merged(got_b, f, one.numpy(), pooled, sr, True, rc.bins(*mode), (name, sr, mode))


# ------------------------------------------------------------------------------------------------ forward, bf16, reference order
@pytest.mark.parametrize("sr", SRS)
def test_forward_bf16_per_bin_kernels_bit_equal(dev, sr):
    """C = 2112 (264 lanes: more than the row kernel takes) runs roi_align_fwd_kernel<bf16, 2> for sampling_ratio 2 and <bf16, 0> otherwise.
    Both keep the reference's order in float32 and round once: the oracle's float32 result, rounded to bf16 by torch, bit for bit."""
    c, rois = rc.C_MAX, rc.rois()
    f = rc.feat(HW, c)
    full = _oracle_fwd(HW, c, 14, sr, True)
    for mode in ((14, 14, 1), (14, 7, 2)):
        got = _fwd(dev, f.bfloat16(), rois, mode, sr)
        assert got.dtype == torch.bfloat16 and torch.equal(got, _strided(full, mode[1], mode[2]).bfloat16()), mode
    k = len(rois) - 7
    got_c = _fwd(dev, f.bfloat16(), rois, (14, 7, 2), sr, roi_count=_count(k, dev), out=torch.full((len(rois), 7, 7, c), NAN, device=dev, dtype=torch.bfloat16))
    assert torch.equal(got_c[:k], got[:k]) and bool((got_c[k:] == 0).all())
    for hw, aligned, mode in (((1, 13), True, (7, 7, 1)), ((9, 1), False, (7, 4, 2)), ((1, 1), True, (14, 14, 1))):
        want = _strided(_oracle_fwd(hw, c, mode[0], sr, aligned), mode[1], mode[2]).bfloat16()
        assert torch.equal(_fwd(dev, rc.feat(hw, c).bfloat16(), rois, mode, sr, aligned), want), (hw, aligned, mode)


@pytest.mark.parametrize("c", [72, 520, 1024])
def test_forward_bf16_row_kernel_loop_branch_bit_equal(dev, c):
    """C <= 2048: roi_align_fwd_row_kernel. A RoI whose grid exceeds 2 in either axis (grid_1x4 and grid_3x1 in one axis only, every RoI
    under sampling_ratio 3) takes its per-sample loop, the reference's order: bit-equal to the oracle rounded to bf16"""
    rois = rc.rois()
    for hw, aligned in ((HW, True), (HW, False), ((1, 13), True), ((9, 1), True)):
        f = rc.feat(hw, c)
        for sr in (0, 3):
            for mode in rc.MODES if c == 72 else rc.MODES[:2]:
                pooled, out, step = mode
                loop = torch.tensor([max(ref.grid(q, pooled, sr, aligned)) > 2 for q in rois.numpy()])
                assert int(loop.sum()) >= 2 and (sr == 0 or bool(loop.all()))
                want = _strided(_oracle_fwd(hw, c, pooled, sr, aligned, rois[loop].numpy()), out, step).bfloat16()
                got = _fwd(dev, f.bfloat16(), rois, mode, sr, aligned)
                assert torch.equal(got[loop], want), (hw, aligned, sr, mode)


# ------------------------------------------------------------------------------------------------ forward, bf16, merged taps
@pytest.mark.parametrize("sr", [0, 1, 2])
@pytest.mark.parametrize("c", rc.CHANNELS)
def test_forward_bf16_merged_taps(dev, c, sr):
    """grids <= 2 x 2 at C <= 2048: the separable, merged form -- the reference's sum in another association, so bounded, not bit-equal:
    |got - ref64| <= 2^-8 |ref64| + 2^-18 A. The strided output is every other bin of the full one bit for bit; slots past roi_count are 0."""
    rois = rc.rois()
    cases = ([(hw, True) for hw in rc.MAPS] + [(HW, False)]) if c == 72 else [(HW, True)]
    for hw, aligned in cases:
        f = rc.feat(hw, c)
        for P in (14, 7):
            full_mode, strided_mode = [m for m in rc.MODES if m[0] == P]
            got = _fwd(dev, f.bfloat16(), rois, full_mode, sr, aligned)
            merged = np.array([max(ref.grid(q, P, sr, aligned)) <= 2 for q in rois.numpy()])
            assert merged.sum() >= 40
            _check_merged(got[torch.from_numpy(merged)], f, rois.numpy()[merged], P, sr, aligned, None, (c, sr, hw, aligned, P))
            got_s = _fwd(dev, f.bfloat16(), rois, strided_mode, sr, aligned)
            assert torch.equal(got_s, _strided(got, strided_mode[1], strided_mode[2])), (hw, aligned, P)
            k = len(rois) - 7
            out = torch.full(got_s.shape, NAN, device=dev, dtype=torch.bfloat16)
            got_c = _fwd(dev, f.bfloat16(), rois, strided_mode, sr, aligned, roi_count=_count(k, dev), out=out)
            assert torch.equal(got_c[:k], got_s[:k]) and bool((got_c[k:] == 0).all())


# ------------------------------------------------------------------------------------------------ backward
def _bwd_ref(hw, g, rois, mode, sr, aligned, n_images=rc.N_IMAGES):
    """-> (ref64, B, n[..., None]) for the gradient g [R, out, out, C] of the bins of `mode`"""
    pooled, out, step = mode
    shape, b = (n_images,) + tuple(hw), rc.bins(*mode)
    rois = rois.numpy() if torch.is_tensor(rois) else rois
    return (ref.backward(g.numpy(), shape, rois, pooled, sr, aligned, bins=b), ref.backward_abs(g.numpy(), shape, rois, pooled, sr, aligned, bins=b),
            ref.terms_per_pixel(shape, rois, pooled, sr, aligned, bins=b)[..., None])


def _check_bwd(got, r64, bb, n, what, half_ulp=0.0, base=None):
    """|got - ref| <= half_ulp |ref| + (16 + n) 2^-24 B; where n = 0 the result is `base` (0 if None) exactly"""
    got = got.float().cpu().numpy().astype(np.float64)
    err, bound = np.abs(got - r64), half_ulp * np.abs(r64) + (16 + n) * 2.0 ** -24 * bb
    m = bound > 0
    print(f"{what}: {float((err[m] / bound[m]).max()) if m.any() else 0.0:.3f} of the bound")
    assert (err <= bound).all(), what
    none = np.broadcast_to(n == 0, got.shape)
    assert none.any() and np.array_equal(got[none], (np.zeros_like(got) if base is None else base)[none]), what


def _sweep(c):
    """(sampling_ratio, aligned, mode): everything at C = 72, the model's two ratios and modes at the other widths"""
    if c == 72:
        return [(sr, al, m) for sr in SRS for al in (True, False) for m in rc.MODES]
    return [(sr, True, m) for sr in (0, 2) for m in rc.MODES[:2]]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("c", rc.CHANNELS)
def test_backward_atomic(dev, c, dtype):
    """roi_align_bwd_kernel against the transpose of the matrix form; image 2 (n = 0) stays exactly as it was"""
    o, rois = ops(), rc.rois()
    for sr, aligned, mode in _sweep(c):
        pooled, out, step = mode
        g = rc.gout(len(rois), out, c)          # bf16-representable: one reference for both gradient types
        r64, bb, n = _bwd_ref(HW, g, rois, mode, sr, aligned)
        got = o.roi_align_bwd(g.to(dev).to(dtype), (3,) + HW + (c,), rois.to(dev), None, pooled, step, 1 / 16, sr, aligned)
        assert got.dtype == torch.float32
        _check_bwd(got, r64, bb, n, f"atomic c {c} sr {sr} aligned {aligned} {mode}")


@pytest.mark.parametrize("hw", rc.MAPS[1:])
def test_backward_atomic_thin_maps(dev, hw):
    o, rois, c = ops(), rc.rois(), 72
    for sr in SRS:
        for mode in rc.MODES[:2]:
            g = rc.gout(len(rois), mode[1], c)
            r64, bb, n = _bwd_ref(hw, g, rois, mode, sr, True)
            got = o.roi_align_bwd(g.to(dev), (3,) + hw + (c,), rois.to(dev), None, mode[0], mode[2], 1 / 16, sr, True)
            _check_bwd(got, r64, bb, n, f"atomic {hw} sr {sr} {mode}")


@pytest.mark.parametrize("c", [72, 520])
def test_backward_atomic_count_and_accumulation(dev, c):
    """roi_count below R: the RoIs past it add nothing. A caller-supplied non-zero dfeat32 is accumulated into: it counts as one more term
    of every pixel's sum (n + 1 terms of total magnitude B + |dfeat32|), and stays bit for bit where no RoI reaches."""
    o, rois = ops(), rc.rois()
    k = len(rois) - 7
    init = torch.randn(3, HW[0], HW[1], c, generator=torch.Generator().manual_seed(5))
    for sr in (0, 2, 3):
        for mode in rc.MODES[:2]:
            pooled, out, step = mode
            g = rc.gout(len(rois), out, c)
            r64, bb, n = _bwd_ref(HW, g, rois[:k], mode, sr, True)
            got = o.roi_align_bwd(g.to(dev), (3,) + HW + (c,), rois.to(dev), None, pooled, step, 1 / 16, sr, True, roi_count=_count(k, dev))
            _check_bwd(got, r64, bb, n, f"atomic roi_count sr {sr} {mode}")
            r64, bb, n = _bwd_ref(HW, g, rois, mode, sr, True)
            base = init.numpy().astype(np.float64)
            acc = o.roi_align_bwd(g.to(dev), (3,) + HW + (c,), rois.to(dev), init.clone().to(dev), pooled, step, 1 / 16, sr, True)
            _check_bwd(acc, r64 + base, bb + np.abs(base), np.where(n > 0, n + 1, 0), f"atomic accumulate sr {sr} {mode}", base=base)


def _gather(dev, g, n_images, hw, rois, mode, sr, aligned=True, out_dtype=torch.float32, **kw):
    pooled, out, step = mode
    c = g.shape[3]
    res = torch.full((n_images, hw[0], hw[1], c), NAN, device=dev, dtype=out_dtype)          # the kernel promises to write every pixel
    kw = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in kw.items()}
    ops().roi_align_bwd_gather(g.to(dev), n_images, hw[0], hw[1], rois.to(dev), res, pooled, step, 1 / 16, sr, aligned, **kw)
    return res.cpu()


@pytest.mark.parametrize("c", rc.CHANNELS)
def test_backward_gather(dev, c):
    """roi_geom_kernel + roi_align_bwd_gather_kernel, fp32 out into a NaN-filled tensor: the bound, and exact zeros where no RoI reaches
    (all of image 2). C = 520 and 1024 run two waves, each with its own LDS slice."""
    rois = rc.rois()
    for sr, aligned, mode in _sweep(c):
        g = rc.gout(len(rois), mode[1], c)
        r64, bb, n = _bwd_ref(HW, g, rois, mode, sr, aligned)
        got = _gather(dev, g, 3, HW, rois, mode, sr, aligned)
        _check_bwd(got, r64, bb, n, f"gather c {c} sr {sr} aligned {aligned} {mode}")
        if aligned and mode[2] == 2:
            got_b = _gather(dev, g.bfloat16(), 3, HW, rois, mode, sr, aligned, out_dtype=torch.bfloat16)
            assert got_b.dtype == torch.bfloat16
            _check_bwd(got_b, r64, bb, n, f"gather bf16 c {c} sr {sr} {mode}", half_ulp=2.0 ** -8)
            assert torch.equal(_gather(dev, g.bfloat16(), 3, HW, rois, mode, sr, aligned), got)          # bf16 in, fp32 out: the same sums


@pytest.mark.parametrize("hw", rc.MAPS[1:])
def test_backward_gather_thin_maps(dev, hw):
    """H = 1 and / or W = 1; the (1, 1) map is a grid of 3 workgroups for 8 XCDs"""
    rois, c = rc.rois(), 72
    for sr in SRS:
        for mode in rc.MODES[:2]:
            g = rc.gout(len(rois), mode[1], c)
            r64, bb, n = _bwd_ref(hw, g, rois, mode, sr, True)
            _check_bwd(_gather(dev, g, 3, hw, rois, mode, sr), r64, bb, n, f"gather {hw} sr {sr} {mode}")


@pytest.mark.parametrize("c", [72, 520])
def test_backward_gather_count_and_image_offset(dev, c):
    """roi_count (the rows past it are marked b = -1 by roi_geom_kernel); roi_count = 0 with the epilogue leaves addend * (mask > 0);
    image_offset = 1: the output is images 1 and 2 of the batch, image 2 written as zeros"""
    rois = rc.rois()
    k = len(rois) - 7
    gen = torch.Generator().manual_seed(9)
    add, msk = torch.randn(2, HW[0], HW[1], c, generator=gen), torch.randn(3, HW[0], HW[1], c, generator=gen)
    for sr in (0, 2, 3):
        for mode in rc.MODES[:2]:
            g = rc.gout(len(rois), mode[1], c)
            r64, bb, n = _bwd_ref(HW, g, rois[:k], mode, sr, True)
            _check_bwd(_gather(dev, g, 3, HW, rois, mode, sr, roi_count=_count(k, dev)), r64, bb, n, f"gather roi_count sr {sr} {mode}")
            none = _gather(dev, g, 3, HW, rois, mode, sr, roi_count=_count(0, dev), addend=add, addend_images=2, mask_ref=msk)
            want = torch.cat([add, torch.zeros(1, HW[0], HW[1], c)]) * (msk > 0)
            assert torch.equal(none, want)
            r64, bb, n = _bwd_ref(HW, g, rois, mode, sr, True)
            got = _gather(dev, g, 2, HW, rois, mode, sr, image_offset=1)
            _check_bwd(got, r64[1:], bb[1:], n[1:], f"gather image_offset sr {sr} {mode}")
            assert bool((got[1] == 0).all()) and torch.equal(got, _gather(dev, g, 3, HW, rois, mode, sr)[1:])


@pytest.mark.parametrize("empty", [rc.SLOTS_EMPTY, 0])
@pytest.mark.parametrize("c", [72, 520])
def test_backward_gather_fixed_slots(dev, c, empty):
    """3 images x 70 slots: under the rois_per_image hint every pixel walks two 64-RoI chunks of its own image's slots (the second one holds
    only gather_rois' empty rows, or -- empty = 0 -- live RoIs). Hinted and generic calls and two launches agree bit for bit."""
    rois = rc.slot_rois(empty)
    for sr in (0, 2):
        for mode in rc.MODES[:2] if c == 72 else rc.MODES[1:2]:
            g = rc.gout(len(rois), mode[1], c)
            r64, bb, n = _bwd_ref(HW, g, rois, mode, sr, True)
            hinted = _gather(dev, g, 3, HW, rois, mode, sr, rois_per_image=rc.SLOTS)
            got = hinted.numpy().astype(np.float64)
            assert (np.abs(got - r64) <= (16 + n) * 2.0 ** -24 * bb).all(), (sr, mode)
            assert torch.equal(hinted, _gather(dev, g, 3, HW, rois, mode, sr))
            assert torch.equal(hinted, _gather(dev, g, 3, HW, rois, mode, sr, rois_per_image=rc.SLOTS))
            tail = _gather(dev, g[rc.SLOTS:], 2, HW, rois[rc.SLOTS:], mode, sr, rois_per_image=rc.SLOTS, image_offset=1)
            assert torch.equal(tail, hinted[1:])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("c", [72, 520])
def test_backward_gather_fused_epilogue_equals_add_cast(dev, c, dtype):
    """out = cast((sum + addend) * (mask_ref > 0)) in one launch == ops.add_cast on the unfused fp32 sum, bit for bit; the images past
    addend_images get no addend. unit_add_cast itself is checked against torch first."""
    o, rois = ops(), rc.rois()
    gen = torch.Generator().manual_seed(13)
    shape = (3, HW[0], HW[1], c)
    add, msk, a32 = (torch.randn(shape, generator=gen).to(dtype) for _ in range(3))
    msk[0, 0, 0, :4] = 0.0          # a mask value of exactly 0 is not > 0
    a32 = a32.float() * 3
    for b, m in ((add, msk), (None, msk), (add, None), (None, None)):
        y = o.add_cast(a32.to(dev), None if b is None else b.to(dev), dtype, mask_ref=None if m is None else m.to(dev)).cpu()
        want = a32 + (0 if b is None else b.float())
        want = want if m is None else torch.where(m.float() > 0, want, torch.zeros(()))
        assert y.dtype == dtype and torch.equal(y, want.to(dtype))
    for sr in (0, 2):
        for mode in rc.MODES[:2]:
            g = rc.gout(len(rois), mode[1], c).to(dtype)
            plain = _gather(dev, g, 3, HW, rois, mode, sr).to(dev)          # fp32 out, no epilogue
            for images in (1, 2):
                fused = _gather(dev, g, 3, HW, rois, mode, sr, out_dtype=dtype, addend=add[:images], addend_images=images, mask_ref=msk)
                want = torch.cat([o.add_cast(plain[:images].contiguous(), add[:images].to(dev), dtype, mask_ref=msk[:images].to(dev)),
                                  o.add_cast(plain[images:].contiguous(), None, dtype, mask_ref=msk[images:].to(dev))]).cpu()
                assert fused.dtype == dtype and torch.equal(fused, want), (sr, mode, images)
            only_add = _gather(dev, g, 3, HW, rois, mode, sr, out_dtype=dtype, addend=add, addend_images=3)
            assert torch.equal(only_add, o.add_cast(plain, add.to(dev), dtype).cpu())


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_by_error_code(dev):
    """argument errors are returned before anything is launched: status -1 (argument), -3 (workspace)"""
    from unit_amd._lib import UnitLibError, check, lib
    o = ops()
    rois = rc.rois()[:4].to(dev)
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)
    with pytest.raises(UnitLibError, match="status -1"):
        o.roi_align(z(3, 9, 13, 12), rois)          # C % 8 != 0
    with pytest.raises(UnitLibError, match="status -1"):
        o.roi_align_bwd_gather(z(4, 7, 7, 12), 3, 9, 13, rois, z(3, 9, 13, 12), 14, 2)
    with pytest.raises(UnitLibError, match="status -1"):
        o.roi_align(z(3, 9, 13, 8), rois, 14, 8, 2)          # (out - 1) * step = 14 >= pooled
    with pytest.raises(UnitLibError, match="status -1"):
        o.roi_align(z(3, 9, 13, 8), rois, 7, 8, 1)
    with pytest.raises(UnitLibError, match="status -1"):
        o.roi_align_bwd_gather(z(4, 17, 17, 8), 3, 9, 13, rois, z(3, 9, 13, 8), 17, 1)          # out_size > 16
    with pytest.raises(UnitLibError, match="status -1"):
        o.roi_align_bwd_gather(z(4, 7, 7, 8), 3, 9, 13, rois, z(3, 9, 13, 8, dt=torch.bfloat16), 14, 2)          # fp32 in, bf16 out
    g, out = z(4, 7, 7, 8), torch.full((3, 9, 13, 8), 7.0, device=dev)
    need = lib().unit_roi_align_bwd_gather_workspace_bytes(4)
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)

    def call(nbytes):
        return lib().unit_roi_align_bwd_gather(o._p(g), 0, 3, 9, 13, 8, o._p(rois), None, 4, 0, 0, 14, 7, 2, ctypes.c_float(1 / 16), 0, 1, None, 0, None,
                                               o._p(out), 0, o._p(ws), nbytes, o._s())
    with pytest.raises(UnitLibError, match="status -3"):
        check(call(need - 1), "roi_align_bwd_gather")
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())          # nothing ran
    check(call(need), "roi_align_bwd_gather")          # the exact size is enough
    torch.cuda.synchronize()
    assert bool((out == 0.0).all())
