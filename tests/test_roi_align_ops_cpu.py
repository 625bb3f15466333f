"""Preconditions of test_roi_align_ops_gpu.py, checked without a GPU: the cases of roi_align_cases.py contain what the GPU tests rely on,
and the two references agree -- the oracle's per-sample loop (oracle_c.c, float32) against the fp64 matrix form of roi_align_ref.py --
within the bounds the GPU tests then apply to the kernels:
    forward    |oracle - ref| <= 2^-20 * A                 A = forward_abs: the operator on |F| (a sum of <= 4 * grid products of float32
                                                            weights, each weight two roundings from exact, rounded as it accumulates)
    backward   |oracle - ref| <= (8 + n) * 2^-24 * B       B = backward_abs, n = terms_per_pixel: each term g * w / count is rounded to
                                                            float32 before it is accumulated (in fp64 by the oracle); 0 exactly where n = 0
"""
import numpy as np
import pytest
import torch

import roi_align_cases as rc
import roi_align_ref as ref
import unit_oracle as orc

HW = rc.MAPS[0]
SRS = [0, 1, 2, 3]


def _grid(name, P=14, sr=0, aligned=True):
    return ref.grid(rc.NAMED[name], P, sr, aligned)


# ------------------------------------------------------------------------------------------------ the cases
def test_named_rois_are_what_their_names_say():
    h, w = HW
    assert _grid("zero_area") == (0, 0) and _grid("zero_area", sr=2) == (2, 2)
    gh, gw = _grid("reversed")
    assert gh <= 0 and gw <= 0 and _grid("reversed", sr=3) == (3, 3)
    ys, xs = ref.roi_samples(rc.NAMED["reversed"], 14, 2)
    assert ys[0, 0] > ys[13, 1] and xs[0, 0] > xs[13, 1]          # negative bin size: the samples run backwards
    ys, xs = ref.roi_samples(rc.NAMED["zero_area"], 14, 2)
    assert np.ptp(ys) == 0 and np.ptp(xs) == 0 and 0 < ys[0, 0] < h - 1 and 0 < xs[0, 0] < w - 1          # one point, inside the map
    for sr in (0, 2):
        ys, xs = ref.roi_samples(rc.NAMED["top_left"], 14, sr)
        for s in (ys, xs):
            assert (s < -1).any() and ((s > -1) & (s < 0)).any() and (s > 0).any()
        ys, xs = ref.roi_samples(rc.NAMED["bottom_right"], 14, sr)
        for s, L in ((ys, h), (xs, w)):
            assert (s > L).any() and ((s > L - 1) & (s < L)).any() and (s < L - 1).any()
        ys, xs = ref.roi_samples(rc.NAMED["outside"], 14, sr)
        assert ys.size and xs.size and (ys < -1).all() and (xs < -1).all()
    ys, xs = ref.roi_samples(rc.NAMED["tenth"], 14, 0)
    assert _grid("tenth") == (1, 1) and np.ptp(ys) < 0.11 and np.ptp(xs) < 0.11 and len(np.unique(ys.astype(int))) == 1
    assert _grid("whole") == (1, 1)
    ys, xs = ref.roi_samples(rc.NAMED["whole"], 14, 0)
    assert ys.min() > -0.5 and ys.max() < h - 0.5 and xs.min() > -0.5 and xs.max() < w - 0.5
    assert _grid("grid_1x4") == (1, 4) and _grid("grid_3x1") == (3, 1) and _grid("grid_2x2") == (2, 2)


def test_integer_sample_rois_land_on_the_edges_of_the_validity_rule():
    """recomputed in float32: at P = 14, sampling_ratio = 2 the samples of int_y / int_x are k + p + 0.5 and k + p + 1.0 exactly, and the
    integer ones reach -1, 0, L-1 and L (== is valid: -1 clamps to 0, L puts its weight on L-1)"""
    for name, (ky, kx) in rc.INT_K.items():
        ys, xs = ref.roi_samples(rc.NAMED[name], rc.INT_P, rc.INT_SR)
        assert ys.dtype == np.float32 and xs.dtype == np.float32
        p = np.arange(14, dtype=np.float64)[:, None]
        assert np.array_equal(ys.astype(np.float64), ky + p + np.array([0.5, 1.0])[None, :])
        assert np.array_equal(xs.astype(np.float64), kx + p + np.array([0.5, 1.0])[None, :])
    yy, yx = ref.roi_samples(rc.NAMED["int_y"], rc.INT_P, rc.INT_SR)
    xy, xx = ref.roi_samples(rc.NAMED["int_x"], rc.INT_P, rc.INT_SR)
    for h, w in rc.MAPS:
        assert {-1.0, 0.0, h - 1.0, float(h)} <= set(yy.ravel().tolist())          # all four on one RoI
        assert {-1.0, 0.0, w - 1.0} <= set(xx.ravel().tolist())
        assert {0.0, w - 1.0, float(w)} <= set(yx.ravel().tolist()) or w == 1
        assert {-1.0, 0.0, w - 1.0, float(w)} <= set(xx.ravel().tolist()) | set(yx.ravel().tolist())
        if w == 1:
            assert {-1.0, 0.0, 1.0} <= set(xx.ravel().tolist())
    # the rule at those points, through the reference: -1 and L are valid (weight 1 on pixel 0 / L-1), the next float32 outside is not
    for L in (1, 9, 13):
        s = np.array([[-1.0, np.nextafter(np.float32(-1), np.float32(-2)), L, np.nextafter(np.float32(L), np.float32(L + 1))]], np.float32)
        for j, (pix, wt) in enumerate([(0, 1.0), (0, 0.0), (L - 1, 1.0), (L - 1, 0.0)]):
            assert ref.weights_1d(s[:, j:j + 1], L)[0, pix] == wt and ref.weights_1d(s[:, j:j + 1], L).sum() == wt


def test_random_rois_and_slot_set():
    r = rc.rois()
    assert r.shape == (len(rc.NAMED) + rc.RANDOM, 5) and bool(torch.isfinite(r).all())
    assert set(r[:, 0].tolist()) == {0.0, 1.0}          # image 2 is named by no RoI
    rnd = r[len(rc.NAMED):]
    side = torch.cat([rnd[:, 3] - rnd[:, 1], rnd[:, 4] - rnd[:, 2]])
    assert float(side.min()) >= 1 and float(side.max()) <= 150
    off = (rnd[:, 1] < 0) | (rnd[:, 2] < 0) | (rnd[:, 3] > 208) | (rnd[:, 4] > 144)
    assert 5 <= int(off.sum()) <= rc.RANDOM - 5          # partly off the map, partly inside
    for empty in (rc.SLOTS_EMPTY, 0):
        s = rc.slot_rois(empty)
        assert s.shape == (3 * rc.SLOTS, 5) and rc.SLOTS > 64          # a second 64-RoI chunk per image
        assert torch.equal(s[:, 0], torch.arange(3).repeat_interleave(rc.SLOTS).float())
        tail = s.view(3, rc.SLOTS, 5)[:, rc.SLOTS - empty:, 1:]
        assert float(tail.abs().sum()) == 0.0
        live = s.view(3, rc.SLOTS, 5)[:, : rc.SLOTS - empty]
        assert bool(((live[..., 3] > live[..., 1]) | (live[..., 0] < 2)).all())
    assert all(ref.grid(q, 14, 0)[0] > 0 for q in rc.slot_rois(0).numpy()[64:70])          # live RoIs in the second chunk of image 0


@pytest.mark.parametrize("mode", rc.MODES)
@pytest.mark.parametrize("sr", SRS)
def test_untouched_pixels_and_non_empty_share(sr, mode):
    """pixels with terms_per_pixel == 0 exist (all of image 2; the RoIs cover images 0 and 1), so the 'exactly untouched' / 'written as
    zero' checks look at something; at least 90 % of the RoIs have a non-empty grid, so no test is vacuous"""
    pooled, out, step = mode
    rois = rc.np_rois()
    nonempty = [min(ref.grid(q, pooled, sr)) > 0 for q in rois]
    assert np.mean(nonempty) >= 0.9
    n = ref.terms_per_pixel((3,) + HW, rois, pooled, sr, bins=rc.bins(*mode))
    assert (n[2] == 0).all() and (n[:2] > 0).any()
    # the slot set names every image
    ns = ref.terms_per_pixel((3,) + HW, rc.np_rois(rc.slot_rois()), pooled, sr, bins=rc.bins(*mode))
    assert all((ns[i] > 0).any() for i in range(3))


def test_merged_and_loop_branches_are_both_populated():
    """the bf16 row kernel merges taps for grids <= 2 x 2 and loops otherwise: under the adaptive ratio both sets are non-empty at either P"""
    for P in (14, 7):
        g = [ref.grid(q, P, 0) for q in rc.np_rois()]
        loop = [max(a, b) > 2 for a, b in g]
        assert sum(loop) >= 2 and sum(not x for x in loop) >= 40


# ------------------------------------------------------------------------------------------------ oracle == matrix form
def _oracle_fwd(f, rois, P, sr, aligned):
    return rc.nhwc(torch.from_numpy(orc.roi_align_forward(rc.nchw(f).numpy(), rois, P, 1 / 16, sr, aligned))).numpy().astype(np.float64)


def _oracle_bwd(g, shape, rois, P, sr, aligned):
    n, h, w = shape
    d = orc.roi_align_backward(rc.nchw(g).numpy(), (n, g.shape[3], h, w), rois, P, 1 / 16, sr, aligned)
    return np.ascontiguousarray(d.transpose(0, 2, 3, 1))


@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("P", [14, 7])
@pytest.mark.parametrize("sr", SRS)
def test_oracle_against_the_matrix_form(sr, P, aligned):
    rois, c = rc.np_rois(), 8
    worst_f = worst_b = 0.0
    for hw in rc.MAPS:
        f = rc.feat(hw, c)
        r64 = ref.forward(f.numpy(), rois, P, sr, aligned)
        a = ref.forward_abs(f.numpy(), rois, P, sr, aligned)
        err = np.abs(_oracle_fwd(f, rois, P, sr, aligned) - r64)
        assert (err <= 2.0 ** -20 * a).all(), (hw, float((err / np.maximum(a, 1e-300)).max()))
        worst_f = max(worst_f, float((err[a > 0] / (2.0 ** -20 * a[a > 0])).max()))
        g = rc.gout(len(rois), P, c)
        shape = (3,) + hw
        b64 = ref.backward(g.numpy(), shape, rois, P, sr, aligned)
        bb = ref.backward_abs(g.numpy(), shape, rois, P, sr, aligned)
        n = ref.terms_per_pixel(shape, rois, P, sr, aligned)[..., None]
        got = _oracle_bwd(g, shape, rois, P, sr, aligned)
        err = np.abs(got - b64)
        bound = (8 + n) * 2.0 ** -24 * bb
        assert (err <= bound).all()
        assert (got[np.broadcast_to(n == 0, got.shape)] == 0).all() and (bb[np.broadcast_to(n == 0, bb.shape)] == 0).all()
        m = bound > 0
        worst_b = max(worst_b, float((err[m] / bound[m]).max()))
    print(f"sr {sr} P {P} aligned {aligned}: forward {worst_f:.3f} of 2^-20 A, backward {worst_b:.3f} of (8 + n) 2^-24 B")
    assert worst_f <= 0.5 and worst_b <= 0.5          # the margin the GPU bounds rest on: the oracle uses at most half of either


@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("mode", rc.MODES)
def test_adjoint_identity(mode, aligned):
    """<forward(F), g> == <F, backward(g)> in fp64: the backward of the reference is the transpose of its forward, strided modes included"""
    pooled, out, step = mode
    rois, c = rc.np_rois(), 8
    for hw in rc.MAPS:
        for sr in SRS:
            f, g = rc.feat(hw, c).numpy().astype(np.float64), rc.gout(len(rois), out, c).numpy().astype(np.float64)
            lhs = float((ref.forward(f, rois, pooled, sr, aligned, bins=rc.bins(*mode)) * g).sum())
            rhs = float((f * ref.backward(g, (3,) + hw, rois, pooled, sr, aligned, bins=rc.bins(*mode))).sum())
            scale = float((ref.forward_abs(f, rois, pooled, sr, aligned, bins=rc.bins(*mode)) * np.abs(g)).sum())
            assert abs(lhs - rhs) <= 1e-12 * scale and scale > 0


# ------------------------------------------------------------------------------------------------ the merged-tap arithmetic, emulated
def _taps_f32(v, n):
    ok = not (v < -1.0 or v > n)
    v = np.float32(0) if v <= 0 else v
    lo = int(v)
    if lo >= n - 1:
        lo = hi = n - 1
        v = np.float32(lo)
    else:
        hi = lo + 1
    whi = np.float32(v - np.float32(lo))
    return ok, lo, hi, np.float32(np.float32(1) - whi), whi


def _merge(idx, wts):
    for k in range(1, 4):
        for j in range(k):
            if wts[k] != 0 and idx[k] == idx[j]:
                wts[j] = np.float32(wts[j] + wts[k])
                wts[k] = np.float32(0)


def _axis(smp, g, L):
    """the row kernel's four (pixel, weight) pairs of one bin and axis: two samples, each two taps, equal pixels merged"""
    idx, wts = [0] * 4, [np.float32(0)] * 4
    for i in range(2):
        ok, lo, hi, wl, wh = (False, 0, 0, 0, 0) if i >= g else _taps_f32(smp[i], L)
        idx[2 * i], idx[2 * i + 1] = lo, hi
        wts[2 * i], wts[2 * i + 1] = (wl, wh) if ok else (np.float32(0), np.float32(0))
    _merge(idx, wts)
    return idx, wts


def _merged_forward_f32(f, rois, P, sr):
    """float32 emulation of roi_align_fwd_row_kernel's merged-tap branch (grids <= 2 x 2), the final bf16 rounding included"""
    _, H, W, C = f.shape
    out = np.zeros((len(rois), P, P, C), np.float32)
    f = f.astype(np.float32)
    for r, roi in enumerate(rois):
        gh, gw = ref.grid(roi, P, sr)
        if max(gh, gw) > 2:
            continue
        ys, xs = ref.roi_samples(roi, P, sr)
        count = np.float32(max(gh * gw, 1))
        b = int(roi[0])
        for ph in range(P):
            rr, wr = _axis(ys[ph], gh, H)
            for pw in range(P):
                cc, wc = _axis(xs[pw], gw, W)
                acc = np.zeros(C, np.float32)
                for k in range(4):
                    if wr[k] == 0:
                        continue
                    ra = np.zeros(C, np.float32)
                    for m in range(4):
                        if wc[m] != 0:
                            ra = ra + wc[m] * f[b, rr[k], cc[m]]
                    acc = acc + wr[k] * ra
                out[r, ph, pw] = acc / count
    return torch.from_numpy(out).bfloat16().float().numpy()


@pytest.mark.parametrize("sr", [0, 1, 2])
def test_merged_tap_arithmetic_meets_the_bf16_forward_bound(sr):
    """the bound test_roi_align_ops_gpu.py puts on the merged-tap kernel, 2^-8 |ref| + 2^-18 A, holds for a float32 emulation of that
    arithmetic: the first term is bf16's half ulp, the second the float32 roundings of the other association"""
    rois, c, hw = rc.np_rois(), 8, HW
    f = rc.feat(hw, c).numpy()
    got = _merged_forward_f32(f, rois, 14, sr).astype(np.float64)
    r64, a = ref.forward(f, rois, 14, sr), ref.forward_abs(f, rois, 14, sr)
    sel = [max(ref.grid(q, 14, sr)) <= 2 for q in rois]
    assert sum(sel) >= 40
    err, bound = np.abs(got - r64)[sel], (2.0 ** -8 * np.abs(r64) + 2.0 ** -18 * a)[sel]
    assert (err <= bound).all()
    print(f"sr {sr}: merged-tap emulation uses {float((err[bound > 0] / bound[bound > 0]).max()):.3f} of the bound")
