"""tests/mask_ref.py -- the fp64 reference tests/test_mask_head_gpu.py holds csrc/mask.hip against -- pinned to the CPU oracle:
the loss and its gradients to orc.mask_head_logits + orc.mask_rcnn_loss on the reference's own M20 tensors (unit_golden.npz), the
logit layout to a spelled-out index loop, the pre-threshold crop averages to the oracle's RoIAlign; and the property of the bitmask
fixture that makes bit-exact agreement a fair demand of unit_mask_targets."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mask_ref as R
import unit_oracle as orc

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "unit_golden.npz"))


def T(k):
    return torch.from_numpy(GOLD[k])


def close(a, b, rtol=1e-5, atol=1e-6):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    assert a.shape == b.shape, (a.shape, b.shape)
    assert torch.allclose(a, b, rtol=rtol, atol=atol), (a - b).abs().max()


@pytest.mark.parametrize("kind", ["sim", "ft"])
def test_mask_loss_ref_vs_oracle(kind):
    """loss, d/dsim directly; d/dlg and d/ddelta through the gradients they induce on the head's parameters and input (the oracle
    exposes no logit leaf: the reference gradient is pushed through the same fp32 convs and must arrive where autograd's does)."""
    K, gscale = 20, 0.37
    pre = f"M20/{kind}/param/"
    names = [k[len(pre):] for k in GOLD.files if k.startswith(pre)]
    x = T("M20/x")
    s = x.shape[0]
    g = torch.Generator().manual_seed(11)
    cls = torch.tensor([2, 0, K, 13, 19, -1, 5, 7, 17])          # novel, base, background (both spellings), base, novel ...
    tgt = (torch.rand(s, 14, 14, generator=g) < 0.4).to(torch.uint8)
    rows = torch.randperm(s, generator=g)
    sim = T("M20/sim_seg")
    fg = ((cls >= 0) & (cls < K)).nonzero().flatten()

    # the oracle, fp32 autograd
    po = {"m." + n: T(pre + n).clone().requires_grad_(True) for n in names}
    xo, simo = x.clone().requires_grad_(True), sim.clone().requires_grad_(True)
    lg_o = orc.mask_head_logits(xo, po, "m", similarity=simo[rows], base_classes=orc.VOC_BASE_SPLIT1, novel_classes=orc.VOC_NOVEL_SPLIT1,
                                finetune=(kind == "ft"))
    loss_o = orc.mask_rcnn_loss(lg_o[fg], cls[fg], tgt[fg])
    (gscale * loss_o).backward()

    # the reference, on the same head's raw column groups
    pr = {n: T(pre + n).clone().requires_grad_(True) for n in names}
    xr = x.clone().requires_grad_(True)
    y = F.relu(F.conv_transpose2d(xr, pr["deconv.weight"], pr["deconv.bias"], stride=2))
    lg = F.conv2d(y, pr["predictor.weight"], pr["predictor.bias"])
    delta = F.conv2d(y, pr["predictor_delta.weight"], pr["predictor_delta.bias"]) if kind == "ft" else None
    loss, dlg, ddelta, dsim = R.mask_loss_ref(lg, delta, cls, tgt, sim, rows, orc.VOC_BASE_SPLIT1, orc.VOC_NOVEL_SPLIT1, gscale)
    close(loss, loss_o.detach())
    close(dsim, simo.grad)
    assert dsim.abs().max() > 1e-4 and dlg.abs().max() > 1e-5
    heads, grads = [lg], [dlg.float()]
    if kind == "ft":
        heads.append(delta)
        grads.append(ddelta.float())
    torch.autograd.backward(heads, grads)
    close(xr.grad, xo.grad)
    for n in names:
        close(pr[n].grad, po["m." + n].grad)
    # no sim, no delta: the plain head
    loss2, dlg2, dd2, ds2 = R.mask_loss_ref(lg, None, cls, tgt, None, None, None, None, 1.0)
    lgl = lg.detach().clone().requires_grad_(True)
    l2 = orc.mask_rcnn_loss(lgl[fg], cls[fg], tgt[fg])
    l2.backward()
    close(loss2, l2.detach())
    close(dlg2, lgl.grad, rtol=1e-5, atol=1e-8)
    assert dd2 is None and ds2 is None
    # no foreground slot: 0 and zero gradients
    loss3, dlg3, _, ds3 = R.mask_loss_ref(lg, None, torch.full((s,), K), tgt, sim, rows, orc.VOC_BASE_SPLIT1, orc.VOC_NOVEL_SPLIT1, 1.0)
    assert loss3.item() == 0.0 and not dlg3.any() and not ds3.any()


@pytest.mark.parametrize("m", [2, 14, 16])
def test_pack_logits_layout_and_round_trip(m):
    s, widths, kp = 3, (5, 4), 16
    g = torch.Generator().manual_seed(m)
    cols = [torch.randn(s, c, m, m, generator=g, dtype=torch.float64) for c in widths]
    packed = R.pack_logits(cols, kp)
    assert packed.shape == (s * m * m, kp)
    p = m // 2
    for si in range(s):
        for yy in range(m):
            for xx in range(m):
                row = ((si * p + yy // 2) * p + xx // 2) * 4 + (yy % 2) * 2 + xx % 2
                assert torch.equal(packed[row, :5], cols[0][si, :, yy, xx]) and torch.equal(packed[row, 5:9], cols[1][si, :, yy, xx])
    assert not packed[:, 9:].any()
    back = R.unpack_logits(packed, widths, m)
    assert all(torch.equal(a, b) for a, b in zip(back, cols))
    assert torch.equal(R.pack_logits(cols[0], 8)[:, :5], packed[:, :5])


# What the bitmask fixture must be for `unit_mask_targets == oracle, bit for bit` to be a fair demand: the device and the oracle both
# evaluate the averages in fp32 (same expression order, no contraction), and a decision can only depend on that arithmetic where the
# true average is close to 0.5. The fp64 averages of the fixture (seed BITMASK_SEED) hold
#     M = 14: 26 values == 0.5 exactly, 0 with 0 < |v - 0.5| < 1e-6, 13.0 % foreground
#     M = 28: 28 values == 0.5 exactly, 0 with 0 < |v - 0.5| < 1e-6, 13.0 % foreground
# 14 (M = 14) and 28 (M = 28) of the exact ties are by design: the half-pixel samples of FIXED_BOXES[0] resp. FIXED_BOXES[1] across the
# straight edge of the sixth mask. Every operand there is a dyadic rational, so fp32 reproduces 0.5 exactly and `>= 0.5` must say 1.
# (The other 12 at M = 14 fall in two random boxes, slots 30 and 34.)
@pytest.mark.parametrize("m", [14, 28])
def test_bitmask_fixture_ties_and_oracle(m):
    masks, rois5, gt_index, cls = R.bitmask_fixture()
    b, mcap, h, w = masks.shape
    assert len({bytes(x.numpy().tobytes()) for x in masks.view(-1, h, w)}) == b * mcap          # six distinct masks
    fg = ((cls >= 0) & (cls < R.BITMASK_K)).nonzero().flatten()
    assert fg.numel() == 69
    sel = masks.view(-1, h, w)[(rois5[fg, 0].long() * mcap + gt_index[fg].long())]
    boxes = rois5[fg, 1:]
    assert ((boxes[:, 0] < 0) | (boxes[:, 1] < 0) | (boxes[:, 2] > w) | (boxes[:, 3] > h)).sum() >= 10          # boxes across the border
    avg = R.crop_and_resize_ref64(sel, boxes, m)
    d = (avg - 0.5).abs()
    exact, near = int((d == 0).sum()), int(((d > 0) & (d < 1e-6)).sum())
    print(f"M={m}: exact ties {exact}, near ties {near}, foreground {(avg >= 0.5).double().mean().item():.3f}")
    assert near == 0 and exact >= 10
    # the straight-edge column: FIXED_BOXES[0] at M = 14, FIXED_BOXES[1] at M = 28
    assert bool((avg[64 + (m == 28), :, 6] == 0.5).all())
    # the fp64 helper is the oracle's sampling: same averages up to fp32 rounding of coordinates < 64 (ulp 2^-18 ~ 4e-6, a few per
    # sample), the same decisions everywhere
    ora = orc.roi_align_forward(sel[:, None].float().numpy(), torch.cat([torch.arange(len(fg))[:, None].float(), boxes], 1).numpy(), m, 1.0, 0, True)
    assert np.abs(ora[:, 0] - avg.numpy()).max() <= 4e-5
    got = orc.crop_and_resize_bitmasks(sel, boxes, m)
    assert torch.equal(got, avg >= 0.5)
    assert not got[66:69].any()          # zero-area, outside, inverted
    assert 0.05 < got.float().mean().item() < 0.5
