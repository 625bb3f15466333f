"""The weak-loss kernels of csrc/losses.hip (unit_wsddn_mil -- both of its kernels --, unit_oicr_targets / _ex, unit_softmax_ce in both
workgroup forms, unit_sup_scores, unit_sum_losses) called directly, against the float64 references of weak_loss_ref.py on the named cases of
weak_loss_cases.py (anchored on the CPU by test_weak_loss_ops_cpu.py). One test id per named case; no case and no row is left out.

Decisions (labels, matched boxes, -inf columns) and copies (mode 0 weights, the score assembly, the loss sum) are compared bit for bit.
Values are held to this project's standing rule (test_box_loss_gpu.py), nothing fitted to the kernels: a device value may deviate from the
float64 reference by 4 x what the torch-fp32 evaluation of the same case deviates from it (the 4 covers an expf / division that rounds the other
way), or by one fp32 ulp of the largest value compared where the fp32 evaluation happens to be closer than that.

The MIL loss is added across images with a float atomic: with three images the order of the additions is not fixed, so its BITS are compared
(run to run, fp32 / bf16 / no dy) only for B <= 2, where a + b = b + a; x_r and dy are bit-identical whatever B.

MEASURED (MI355X), worst error / bar over the cases of each kernel (every test prints its own figures before it asserts):
  MIL   x_r 0.45 (s65_k20_ragged: 2.1e-8 / 4.6e-8), dy cls 0.46, dy det 0.41 (s130_k33_third: 9.7e-10 / 2.1e-9, 8.7e-10 / 2.1e-9);
        loss 0.14 (s513_k20_hi1: 2.1e-7 / 1.5e-6, the bar being the derived floor; largest error in ulp of the loss: 2.3, s512_k20_all)
  OICR  mode 1 weights 0.04 (m1_s1024_k80: 2.0e-7 / 5.7e-6, derived floor; 2 ulp of the weight at m1_s1000_k95); everything else bit-equal
  CE    dy 0.40 in both forms (c81_r257_wnone_inf_g3: 1.0e-8 / 2.5e-8); loss 0.03 in both forms (c81_r15425_wnone_g1: 8.9e-7 / 3.1e-5, derived
        floor; largest error in ulp of the loss: 1.1, c32_r15425_wzeros_g3)
Under the rule alone (a floor of one ulp) three scalars miss: see the note above the _floor functions."""
import numpy as np
import pytest
import torch

import weak_loss_cases as C
import weak_loss_ref as ref

pytestmark = pytest.mark.gpu

S9 = C.SENTINEL
WORST = {}


def _ops():
    from unit_amd import ops
    return ops


def _ulp32(x):
    return float(np.spacing(np.float32(abs(float(x)))))


def _bar(dev, largest):
    return max(4.0 * float(dev), _ulp32(largest))


def _within(kernel, what, name, got, want64, fp32, floor=0.0):
    """got (device, fp32) against want64 under the module's rule, the bar taken from fp32 (the torch-fp32 evaluation); prints the figures first.
    floor: a derived worst-case rounding bound (the _floor functions below) that stands in for the rule's single ulp where it is larger"""
    got, want64, fp32 = (torch.as_tensor(t).double().reshape(-1) for t in (got, want64, fp32))
    assert torch.isfinite(got).all(), (name, what)
    err = float((got - want64).abs().max())
    bar = max(_bar((fp32 - want64).abs().max(), want64.abs().max()), float(floor))
    ratio = err / bar
    key = f"{kernel} {what}"
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    print(f"{kernel} {name} {what}: err {err:.3g} bar {bar:.3g} ratio {ratio:.2f} (worst so far {WORST[key]:.2f})")
    return err <= bar, (name, what, err, bar)


# ---- The three quantities that are ONE number (a loss) or a handful (the mode 1 weights: one per pseudo-GT). There the fp32 yardstick is a single
# draw: where torch's fp32 result happens to land within a fraction of an ulp, the rule leaves one ulp, and a correct fp32 kernel that sums in
# another order misses it (first run on the MI355X: MIL loss of s512_k20_all 2.3 ulp off at a yardstick of 0.3 ulp, CE loss of c32_r15425 1.1 ulp,
# a weight of m1_s1000_k95 2 ulp -- while every vector quantity, x_r and the gradients, stays below half its bar). For these three the single ulp
# is replaced by the worst-case rounding bound of the arithmetic the kernel is documented to do, derived here from the formats alone; u = 2^-24.
#   (S) a sum of non-negative fp32 addends through a reduction of depth D (every addend passes through <= D additions) is off by <= D u total:
#       the partial sums of one level add up to the total, each is rounded by <= u times itself.
#   (E) expf / logf are 1 ulp = 2 u functions; the argument x - max of an expf is itself rounded: a relative u |x - max| in the result.
U = 2.0 ** -24


def _spread(x):
    """max over rows of (row max - row min over the finite entries): bounds every |x - max| of (E); an expf(-inf) is an exact 0"""
    fin = torch.isfinite(x)
    hi = torch.where(fin, x, torch.full_like(x, float("-inf"))).amax(1)
    lo = torch.where(fin, x, torch.full_like(x, float("inf"))).amin(1)
    return float((hi - lo).max())


def _floor_mil_loss(c, l64):
    """loss = mult / (B K) sum_{b,c} t_bc, t = -log p or -log(1 - p). The sum: ceil(log2 K) butterfly levels that meet two non-zero partials,
    B - 1 atomics, the product with mult and the division: (S) gives (ceil(log2 K) + B + 1) u loss; logf adds 2 u loss (E).
    p = sum_r x_r over <= 2 rows per thread, 6 butterfly levels, 8 waves: 16 u (S); x_r = s1 s2: two expf (2 u + spread u each), their two
    denominators (K - 1 serial additions of terms that carry (E); 16 levels over the rows), two divisions and the product:
    delta p / p <= (K + 44 + 2 (A_cls + A_det)) u. It moves t by |dt/dp| delta p = (delta p / p) x (1 for y = 1, p / (1 - p) for y = 0), nothing
    through a clamped class."""
    K, B = c["K"], c["B"]
    p = ref.mil_class_vector(c["streams"], c["ccol0"], c["dcol0"], K, c["valid"], c["S"], B, c["tc"], c["td"])
    inside = (p > ref.P_LO) & (p < ref.P_HI)
    sens = float(torch.where(c["multihot"].bool(), torch.ones_like(p), p / (1 - p))[inside].sum()) / (B * K)
    live = c["valid"] >= 0
    a_cls = _spread(c["streams"][live, c["ccol0"]:c["ccol0"] + K].double() / c["tc"])
    det = c["streams"][live, c["dcol0"]:c["dcol0"] + K].double() / c["td"]
    a_det = float(det.max() - det.min())          # over all rows: no smaller than any column's spread within an image
    return ((int(np.ceil(np.log2(K))) + B + 3) * abs(float(l64)) + (K + 44 + 2 * (a_cls + a_det)) * sens * c["mult"]) * U


def _floor_oicr_weight(c):
    """w = expf(x - max) / se, se the serial sum of K + 1 expf: K u (S, depth K) + (2 + A) u for its addends (E); the numerator (2 + A) u;
    the division u: relative (K + 5 + 2 A) u, A the largest spread of a live row"""
    K = c["K"]
    x = c["src"][c["valid"] >= 0, c["col0"]:c["col0"] + K + 1].double()
    return (K + 5 + 2 * _spread(x)) * U * float(c["ref"][1].abs().max())


def _floor_ce_loss(c, l64):
    """loss = (1 / n) sum_r w_r t_r, t = lse - x_label >= 0, w >= 0. The sum over rows: <= ceil(R / 1024) serial additions a thread, 6 butterfly
    levels, <= 16 waves, the product with 1 / n, which is itself rounded: D = ceil(R / 1024) + 24 (the multi-workgroup form is shallower: its
    fixed point truncates each of <= 240 partials by < 2^-24 absolute). (S): D u loss.
    An addend: se is a serial sum of ncls expf: (ncls - 1 + 2 + A) u relative (S, E) = absolute in log se; logf 2 u |log se|; + max: u |lse|;
    - x_label and x w: 2 u t. Their mean weighs at most w_max of that."""
    n, R = c["ncls"], c["R"]
    live = c["labels"] >= 0
    if not live.any():
        return 0.0
    x = c["logits"][live, c["col0"]:c["col0"] + n].double()
    lse = torch.logsumexp(x, -1)
    t = lse - x.gather(1, c["labels"][live].long()[:, None])[:, 0]
    wmax = float(c["weights"].max()) if c["weights"] is not None else 1.0
    per = (n + 1 + _spread(x)) + 3 * float(lse.abs().max()) + 2 * float(t.abs().max())
    return ((int(np.ceil(R / 1024)) + 24) * abs(float(l64)) + wmax * per + 240.0 / int(live.sum())) * U


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


# ---------------------------------------------------------------------------------------------------- MIL
def _mil_run(c, dev, dy_dtype=torch.float32, want_dy=True, gscale=None):
    """-> (loss [3] with the value in the middle, x_r, dy or None), on the CPU"""
    o = _ops()
    n = c["B"] * c["S"]
    dy = torch.full((n, c["ldd"]), S9, dtype=dy_dtype, device=dev) if want_dy else None
    out = torch.full((3,), S9, device=dev)
    _, xr = o.wsddn_mil(c["streams"].to(dev), c["ccol0"], c["dcol0"], c["K"], c["valid"].to(dev), c["S"], c["B"], c["multihot"].to(dev), c["tc"],
                        c["td"], c["mult"], dy=dy, dyc0=c["dyc0"], dyd0=c["dyd0"], gscale=c["gscale"] if gscale is None else gscale,
                        loss_out=out[1:2])
    torch.cuda.synchronize()
    return out.cpu(), xr.cpu(), (dy.cpu() if want_dy else None)


def _dy_blocks(c, dy):
    K = c["K"]
    return dy[:, c["dyc0"]:c["dyc0"] + K], dy[:, c["dyd0"]:c["dyd0"] + K]


def _dy_rest_untouched(c, dy):
    rest = torch.ones(dy.shape[1], dtype=torch.bool)
    rest[c["dyc0"]:c["dyc0"] + c["K"]] = False
    rest[c["dyd0"]:c["dyd0"] + c["K"]] = False
    return bool(rest.any()) and bool((dy[:, rest].float() == S9).all())


@pytest.mark.parametrize("name", list(C.MIL))
def test_mil(dev, name):
    """unit_wsddn_mil: loss, x_r, dy (cls and det blocks) against float64 under the module's rule; the rows of empty slots exactly 0 in x_r and
    in both dy blocks; the columns of dy beside the blocks and the neighbours of the loss untouched; bf16 dy = the fp32 dy rounded to bf16, bit
    for bit; dy = None and bf16 give the same x_r bits (and loss bits, B <= 2: the loss is a float atomic over images); gscale scales dy (a power
    of two: exactly) and not the loss; a second run is bit-identical in x_r and dy.
    MEASURED (MI355X) worst error / bar over the cases: x_r 0.45, dy cls 0.46, dy det 0.41, loss 0.14 (against its derived floor)."""
    c = C.mil_case(name)
    K, B = c["K"], c["B"]
    l64, xr64, dc64, dd64 = C.mil_ref(name)
    l32, xr32, dc32, dd32 = C.mil_ref(name, torch.float32)
    out, xr, dy = _mil_run(c, dev)
    dcls, ddet = _dy_blocks(c, dy)
    floor = _floor_mil_loss(c, l64)
    checks = [_within("mil", "loss", name, out[1], l64, l32, floor), _within("mil", "x_r", name, xr, xr64, xr32),
              _within("mil", "dy_cls", name, dcls, dc64, dc32), _within("mil", "dy_det", name, ddet, dd64, dd32)]
    for ok, why in checks:
        assert ok, why
    empty = c["valid"] < 0
    if empty.any():
        assert float(xr[empty].abs().max()) == 0 and float(dcls[empty].abs().max()) == 0 and float(ddet[empty].abs().max()) == 0
    assert _dy_rest_untouched(c, dy) and float(out[0]) == S9 and float(out[2]) == S9
    if c["special"] != "hi":
        assert float(dcls.abs().max()) > 0 and float(ddet.abs().max()) > 0
    fixed_loss = B <= 2
    # bf16
    out16, xr16, dy16 = _mil_run(c, dev, dy_dtype=torch.bfloat16)
    for blk16, blk32 in zip(_dy_blocks(c, dy16), (dcls, ddet)):
        assert _same_bits(blk16, blk32.to(torch.bfloat16))
    assert _dy_rest_untouched(c, dy16) and _same_bits(xr16, xr) and (not fixed_loss or _same_bits(out16, out))
    # no dy
    out0, xr0, _ = _mil_run(c, dev, want_dy=False)
    assert _same_bits(xr0, xr) and (not fixed_loss or _same_bits(out0, out))
    # gscale
    outh, xrh, dyh = _mil_run(c, dev, gscale=c["gscale"] * 0.5)
    assert _same_bits(xrh, xr) and (not fixed_loss or _same_bits(outh, out))
    assert _same_bits(_dy_blocks(c, dyh)[0], dcls * 0.5) and _same_bits(_dy_blocks(c, dyh)[1], ddet * 0.5)
    ok, why = _within("mil", "loss", name + "/gscale", outh[1], l64, l32, floor)
    assert ok, why
    # again
    out2, xr2, dy2 = _mil_run(c, dev)
    assert _same_bits(xr2, xr) and _same_bits(dy2, dy) and (not fixed_loss or _same_bits(out2, out))


# ---------------------------------------------------------------------------------------------------- OICR targets
def _oicr_run(c, dev, src=None, rois5=None, col0=None, mode=None, fg=None, bg=None):
    o = _ops()
    src = (c["src"] if src is None else src).to(dev)
    args = (src, c["col0"] if col0 is None else col0, c["mode"] if mode is None else mode, c["K"], (c["rois5"] if rois5 is None else rois5).to(dev),
            c["valid"].to(dev), c["S"], c["B"], c["multihot"].to(dev))
    kw = dict(fg_thresh=c.get("fg", 0.5) if fg is None else fg, bg_thresh=c.get("bg", 0.1) if bg is None else bg)
    lab, w = o.oicr_targets(*args, **kw)
    lab_x, w_x, gb = o.oicr_targets(*args, want_boxes=True, **kw)
    torch.cuda.synchronize()
    assert torch.equal(lab, lab_x) and _same_bits(w, w_x)          # the plain and the _ex export
    return lab.cpu(), w.cpu(), gb.cpu()


@pytest.mark.parametrize("name", list(C.OICR))
def test_oicr(dev, name):
    """unit_oicr_targets / unit_oicr_targets_ex. Mode 0 (hand-placed probabilities, exact in fp32): labels, weights and matched boxes bit-equal to
    the reference -- they are decisions and copies of inputs; this holds the cross-wave and in-wave ties, the last live row, the ignored junk
    slots, the choice among zeros, the rows exactly on fg / bg and the equal IoUs of test_weak_loss_ops_cpu.py::test_oicr_hand_placed_rows.
    Mode 1 (softmax in the kernel; argmax leads >= 1e-4 by construction): labels and boxes exact, weights under the module's rule.
    The plain and the _ex export agree bit for bit.
    MEASURED (MI355X): mode 0 bit-equal in all eight cases; mode 1 weights worst error / bar 0.04 (against the derived floor)."""
    c = C.oicr_case(name)
    lab64, w64, gb64 = c["ref"]
    lab, w, gb = _oicr_run(c, dev)
    assert torch.equal(lab.long(), lab64), (lab.long() != lab64).nonzero()[:8, 0].tolist()
    assert _same_bits(gb, gb64.float())
    if c["mode"] == 0:
        assert _same_bits(w, w64.float())
    else:
        K = c["K"]
        probs32 = torch.softmax(torch.nan_to_num(c["src"][:, c["col0"]:c["col0"] + K + 1]), -1)          # (empty slots hold NaN; they are not read)
        lab32, w32, _ = ref.oicr_targets(probs32, 0, K, c["rois5"], c["valid"], c["S"], c["B"], c["multihot"], c["fg"], c["bg"])
        assert torch.equal(lab32, lab64)
        ok, why = _within("oicr", "weights", name, w, w64, w32, _floor_oicr_weight(c))
        assert ok, why
        assert bool(((w == 0) == (w64 == 0)).all())


def test_oicr_after_mil(dev):
    """MIL -> mode 0 on the training shape (3 x 512 x 20): the device's own x_r as probabilities. The labels and boxes are those of the float64
    chain (every argmax leads by >= 1e-4, x_r is right to ~1e-7); and, bit for bit, what the reference decides on the device's x_r."""
    m, ch = C.mil_case(C.CHAIN), C.chain_case()
    _, xr, _ = _mil_run(m, dev, want_dy=False)
    lab, w, gb = _oicr_run(m, dev, src=xr, rois5=ch["rois5"], col0=0, mode=0)
    lab64, w64, gb64 = ch["ref"]
    assert torch.equal(lab.long(), lab64) and _same_bits(gb, gb64.float())
    labx, wx, gbx = ref.oicr_targets(xr, 0, m["K"], ch["rois5"], m["valid"], m["S"], m["B"], m["multihot"])
    assert torch.equal(lab.long(), labx) and _same_bits(w, wx.float()) and _same_bits(gb, gbx.float())
    xr64, xr32 = C.mil_ref(C.CHAIN)[1], C.mil_ref(C.CHAIN, torch.float32)[1]
    assert float((w.double() - w64).abs().max()) <= _bar((xr32 - xr64).abs().max(), xr64.abs().max())


# ---------------------------------------------------------------------------------------------------- softmax cross-entropy
def _ce_run(c, dev, dy_dtype=torch.float32, want_dy=True):
    o = _ops()
    dy = torch.full((c["R"], c["ldd"]), S9, dtype=dy_dtype, device=dev) if want_dy else None
    out = torch.full((3,), S9, device=dev)
    o.softmax_ce(c["logits"].to(dev), c["col0"], c["ncls"], c["labels"].to(dev), weights=c["weights"].to(dev) if c["weights"] is not None else None,
                 dy=dy, dcol0=c["dcol0"], gscale=c["gscale"], loss_out=out[1:2])
    acc = o._loss_acc(dev)
    torch.cuda.synchronize()
    return out.cpu(), (dy.cpu() if want_dy else None), (acc.cpu() if acc is not None else None)


@pytest.mark.parametrize("name", list(C.CE))
def test_ce(dev, name):
    """unit_softmax_ce in its single- and its multi-workgroup form (ops._MULTI_WG_LOSSES both ways; more than 256 rows make the difference): loss
    and dy against float64 under the module's rule; dy of ignored rows exactly 0, of -inf columns exactly 0; all rows ignored: loss 0, dy 0; the
    columns of dy beside the block and the neighbours of loss_out untouched; dy bit-identical between the two forms; the accumulator handed
    back zero; dy = None gives the same loss bits; bf16 dy = the fp32 dy rounded, bit for bit.
    MEASURED (MI355X) worst error / bar: dy 0.40 and loss 0.03 (against its derived floor), the same in both forms."""
    o = _ops()
    c = C.ce_case(name)
    n, d0 = c["ncls"], c["dcol0"]
    l64, dy64 = C.ce_ref(name)
    l32, dy32 = C.ce_ref(name, torch.float32)
    saved = o._MULTI_WG_LOSSES
    seen = {}
    try:
        for multi in (True, False):
            o._MULTI_WG_LOSSES = multi
            out, dy, acc = _ce_run(c, dev)
            form = "multi" if multi else "single"
            assert (acc is not None) == multi and (acc is None or int(acc.abs().max()) == 0)
            block = dy[:, d0:d0 + n]
            ok1, why1 = _within("ce", f"loss {form}", name, out[1], l64, l32, _floor_ce_loss(c, l64))
            ok2, why2 = _within("ce", f"dy {form}", name, block, dy64, dy32)
            assert ok1, why1
            assert ok2, why2
            ignored = c["labels"] < 0
            if ignored.any():
                assert float(block[ignored].abs().max()) == 0
            if c["ignored"]:
                assert float(out[1]) == 0 and float(block.abs().max()) == 0
            else:
                assert float(block.abs().max()) > 0 and float(out[1]) > 0
            inf_cols = torch.isinf(c["logits"][0, c["col0"]:c["col0"] + n])
            assert "_inf" not in name or (bool(inf_cols.any()) and float(block[:, inf_cols].abs().max()) == 0)
            assert bool((dy[:, :d0] == S9).all()) and bool((dy[:, d0 + n:] == S9).all()) and float(out[0]) == S9 and float(out[2]) == S9
            out0, _, acc0 = _ce_run(c, dev, want_dy=False)
            assert _same_bits(out0, out) and (acc0 is None or int(acc0.abs().max()) == 0)
            _, dy16, _ = _ce_run(c, dev, dy_dtype=torch.bfloat16)
            assert _same_bits(dy16[:, d0:d0 + n], block.to(torch.bfloat16)) and bool((dy16[:, :d0].float() == S9).all())
            seen[multi] = (out, dy)
    finally:
        o._MULTI_WG_LOSSES = saved
    assert _same_bits(seen[True][1], seen[False][1])


# ---------------------------------------------------------------------------------------------------- score assembly, loss sum
@pytest.mark.parametrize("name", list(C.SUP))
def test_sup_scores(dev, name):
    """unit_sup_scores, bit for bit: delta + (weak streams added in order) / n + extra, in fp32; -inf exactly at the masked columns; the mask
    buffer has a set entry behind its ncls - 1 live ones, which the last column must not take"""
    o = _ops()
    c = C.sup_case(name)
    d = lambda t: t.to(dev) if t is not None else None
    mask = None if c["mask"] is None else torch.cat([c["mask"], torch.ones(3, dtype=torch.uint8)])
    got = o.sup_scores(d(c["delta"]), c["dcol0"], d(c["weak"]), c["wcol0"], c["n_oicr"], c["ncls"], novel_mask=d(mask), extra=d(c["extra"]),
                       ecol0=c["ecol0"]).cpu()
    want = ref.sup_scores(c["delta"], c["dcol0"], c["weak"], c["wcol0"], c["n_oicr"], c["ncls"], mask, c["extra"], c["ecol0"])
    assert _same_bits(got, want)
    neg = torch.isneginf(got)
    if mask is None:
        assert not bool(neg.any())
    else:
        cols = torch.zeros(c["ncls"], dtype=torch.bool)
        cols[:c["ncls"] - 1] = c["mask"].bool()
        assert bool((neg == cols[None]).all()) and bool(torch.isfinite(got[:, -1]).all())


@pytest.mark.parametrize("n", range(1, 10))
def test_sum_losses(dev, n):
    """unit_sum_losses = the sequential fp32 sum, bit for bit; the neighbours of `out` stay"""
    o = _ops()
    v = C.sum_case(n)
    out = torch.full((3,), S9, device=dev)
    o.sum_losses(v.to(dev), out=out[1:2])
    out = out.cpu()
    assert np.float32(out[1].item()).tobytes() == np.float32(ref.sum_losses(v.numpy())).tobytes() and float(out[0]) == S9 and float(out[2]) == S9


# ---------------------------------------------------------------------------------------------------- argument checks
def test_argument_checks(dev):
    """K = 97 (MIL), K = 96 or S = 1025 (OICR) and want_boxes with a row count that is not B * S raise, and nothing is launched: the loss (not even
    zeroed) and dy keep their sentinels. MIL takes K = 96 (MIL_MAXK, case s70_k96_all) while the targets kernel stops at 95 (its per-class arrays
    hold MIL_MAXK entries and the mode 1 row has K + 1 columns): pinned as it is, noted in include/unit_hip.h."""
    o = _ops()
    from unit_amd._lib import UnitLibError
    S, B = 8, 1
    valid = torch.zeros(B * S, dtype=torch.int32, device=dev)

    def mil(K):
        out = torch.full((3,), S9, device=dev)
        dy = torch.full((B * S, 2 * K), S9, device=dev)
        call = lambda: o.wsddn_mil(torch.zeros(B * S, 2 * K, device=dev), 0, K, K, valid, S, B, torch.ones(B, K, dtype=torch.uint8, device=dev), 1.0, 2.0,
                                   1.0, dy=dy, dyc0=0, dyd0=K, loss_out=out[1:2])
        return call, out, dy

    call, out, dy = mil(97)
    with pytest.raises(UnitLibError):
        call()
    torch.cuda.synchronize()
    assert bool((out.cpu() == S9).all()) and bool((dy.cpu() == S9).all())
    call, out, dy = mil(96)
    call()
    torch.cuda.synchronize()
    out, dy = out.cpu(), dy.cpu()
    assert float(out[0]) == S9 and float(out[2]) == S9 and np.isfinite(float(out[1])) and float(out[1]) != S9 and bool((dy != S9).all())

    def targets(K, S, rows=None, want_boxes=False, B=1):
        rows = B * S if rows is None else rows
        return o.oicr_targets(torch.zeros(rows, K, device=dev), 0, 0, K, torch.zeros(rows, 5, device=dev),
                              torch.zeros(rows, dtype=torch.int32, device=dev), S, B, torch.ones(B, K, dtype=torch.uint8, device=dev), want_boxes=want_boxes)

    for want_boxes in (False, True):
        with pytest.raises(UnitLibError):
            targets(96, 8, want_boxes=want_boxes)
        with pytest.raises(UnitLibError):
            targets(20, 1025, want_boxes=want_boxes)
    with pytest.raises(ValueError):
        targets(20, 8, rows=9, want_boxes=True)
    lab, w, gb = targets(95, 8, want_boxes=True)
    torch.cuda.synchronize()
    # K = 95 is taken: all-zero probabilities and empty boxes -> every pseudo-GT is row 0, every IoU 0: background, weight 0
    assert bool((lab.cpu() == 95).all()) and float(w.abs().max()) == 0 and float(gb.abs().max()) == 0
