"""unit_oicr_targets_wide (csrc/losses.hip; ops.oicr_targets(..., wide=True)) called directly on the named cases of weak_wide_cases.py, which
test_weak_wide_cpu.py anchors on the CPU. One test id per case, no case and no row left out.

Up to 1024 rows per image both kernels run: there the wide form equals the narrow one bit for bit in labels, weights and matched boxes.
Above, the narrow one refuses (pinned here and in test_weak_loss_ops_gpu.py) and the wide one is compared with the float64 reference under the
rules of test_weak_loss_ops_gpu.py, whose helpers are used as they are: decisions and copies (labels, matched boxes, mode 0 weights) bit for
bit; mode 1 weights within 4 x the error of the torch-fp32 evaluation of the same case (or the derived rounding floor of w = expf / se)."""
import pytest
import torch

import weak_loss_ref as ref
import weak_wide_cases as W
from test_weak_loss_ops_gpu import _floor_oicr_weight, _same_bits, _within

pytestmark = pytest.mark.gpu

S9 = W.SENTINEL


def _ops():
    from unit_amd import ops
    return ops


def _run(c, dev, wide):
    """-> (labels, weights, boxes) on the CPU; the form without boxes is run too and must give the same labels and weights"""
    o = _ops()
    args = (c["src"].to(dev), c["col0"], c["mode"], c["K"], c["rois5"].to(dev), c["valid"].to(dev), c["S"], c["B"], c["multihot"].to(dev))
    kw = dict(fg_thresh=c["fg"], bg_thresh=c["bg"], wide=wide)
    lab, w = o.oicr_targets(*args, **kw)
    lab_x, w_x, gb = o.oicr_targets(*args, want_boxes=True, **kw)
    torch.cuda.synchronize()
    assert torch.equal(lab, lab_x) and _same_bits(w, w_x)
    return lab.cpu(), w.cpu(), gb.cpu()


def test_max_weak_rows():
    assert _ops().max_weak_rows() == W.THREADS * W.SLOTS == 8192


@pytest.mark.parametrize("name", list(W.CASES))
def test_wide(dev, name):
    """every case against the float64 reference; at S <= 1024 against the narrow kernel, bit for bit; a second run gives the same bits"""
    c = W.case(name)
    K, S = c["K"], c["S"]
    lab64, w64, gb64 = c["ref"]
    lab, w, gb = _run(c, dev, True)
    if S <= W.THREADS:
        nlab, nw, ngb = _run(c, dev, False)
        assert torch.equal(lab, nlab) and _same_bits(w, nw) and _same_bits(gb, ngb)
    assert torch.equal(lab.long(), lab64), (lab.long() != lab64).nonzero()[:8, 0].tolist()
    assert _same_bits(gb, gb64.float())
    if c["mode"] == 0:
        assert _same_bits(w, w64.float())
    else:
        probs32 = torch.softmax(torch.nan_to_num(c["src"][:, c["col0"]:c["col0"] + K + 1]), -1)          # (empty slots hold NaN; they are not read)
        lab32, w32, _ = ref.oicr_targets(probs32, 0, K, c["rois5"], c["valid"], S, c["B"], c["multihot"], c["fg"], c["bg"])
        assert torch.equal(lab32, lab64)
        ok, why = _within("oicr_wide", "weights", name, w, w64, w32, _floor_oicr_weight(c))
        assert ok, why
        assert bool(((w == 0) == (w64 == 0)).all())
    lab2, w2, gb2 = _run(c, dev, True)
    assert torch.equal(lab2, lab) and _same_bits(w2, w) and _same_bits(gb2, gb)


def test_refusals_leave_the_outputs_alone(dev):
    """S = 8193 and K = 96 raise UnitLibError from the wide export and nothing is launched: labels, weights and boxes keep their sentinels (the
    export is called on buffers of this test's own); S = 8192 with K = 95 is taken; the default ops.oicr_targets still refuses S = 1025"""
    o = _ops()
    from unit_amd._lib import UnitLibError, lib

    def call(K, S, B=1):
        rows = B * S
        src = torch.zeros(rows, K, device=dev)
        rois5 = torch.zeros(rows, 5, device=dev)
        valid = torch.zeros(rows, dtype=torch.int32, device=dev)
        mh = torch.ones(B, K, dtype=torch.uint8, device=dev)
        lab = torch.full((rows,), 77, dtype=torch.int32, device=dev)
        w = torch.full((rows,), S9, device=dev)
        gb = torch.full((rows, 4), S9, device=dev)
        run = lambda: o.check(lib().unit_oicr_targets_wide(o._p(src), K, 0, 0, K, o._p(rois5), o._p(valid), S, B, o._p(mh), 0.5, 0.1, o._p(lab), o._p(w),
                                                           o._p(gb), o._s()), "oicr_targets_wide")
        return run, lab, w, gb

    for K, S in ((20, 8193), (96, 8), (96, 8192)):
        run, lab, w, gb = call(K, S)
        with pytest.raises(UnitLibError):
            run()
        torch.cuda.synchronize()
        assert bool((lab.cpu() == 77).all()) and bool((w.cpu() == S9).all()) and bool((gb.cpu() == S9).all())
        for want_boxes in (False, True):
            with pytest.raises(UnitLibError):
                o.oicr_targets(torch.zeros(S, K, device=dev), 0, 0, K, torch.zeros(S, 5, device=dev), torch.zeros(S, dtype=torch.int32, device=dev), S, 1,
                               torch.ones(1, K, dtype=torch.uint8, device=dev), want_boxes=want_boxes, wide=True)
    run, lab, w, gb = call(95, 8192)
    run()
    torch.cuda.synchronize()
    # all-zero probabilities and empty boxes: every pseudo-GT is row 0, every IoU 0 -> background, weight 0, the (zero) box of row 0
    assert bool((lab.cpu() == 95).all()) and float(w.abs().max()) == 0 and float(gb.abs().max()) == 0
    for want_boxes in (False, True):
        with pytest.raises(UnitLibError):
            o.oicr_targets(torch.zeros(1025, 20, device=dev), 0, 0, 20, torch.zeros(1025, 5, device=dev), torch.zeros(1025, dtype=torch.int32, device=dev),
                           1025, 1, torch.ones(1, 20, dtype=torch.uint8, device=dev), want_boxes=want_boxes)
    with pytest.raises(ValueError):
        o.oicr_targets(torch.zeros(9, 20, device=dev), 0, 0, 20, torch.zeros(9, 5, device=dev), torch.zeros(9, dtype=torch.int32, device=dev), 8, 1,
                       torch.ones(1, 20, dtype=torch.uint8, device=dev), wide=True)
