"""unit_pcl_loss (csrc/pcl.hip) against the reference's own TYPE "PCL" weak detector (tests/golden/pcl_golden.npz, generator
tests/golden/gen_pcl_golden.py: the reference's compute_pcl_loss_inputs decisions per refinement iteration, its PCLFunction losses and their
gradients): loss within rtol 1e-5 (NaN where the reference's is), logits gradient within rtol 2e-4 / atol 2e-6 (the bars of the OICR
fixtures), ragged images in fixed slots, bit-identical run to run, bad shapes and strides refused with an error status."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "pcl_golden.npz"))
CASES = [(t, k, it) for t, k in (("P20", 20), ("P20n", 20), ("P80", 80), ("P20r", 20)) for it in range(3)]


def slots(tag, K, it, dev, pad=3):
    """the fixture in the fixed-slot layout of the fused step: S = max rows + pad, clusters in [b, ldc] tables, logits at column 5"""
    sizes = GOLD[f"{tag}/sizes"].tolist()
    b, s = len(sizes), max(sizes) + pad
    G = lambda k: GOLD[f"{tag}/it{it}/{k}"]
    ldc = max(len(G(f"pc_count{i}")) for i in range(b)) + 2
    col0, ld = 5, 5 + K + 1 + 3
    lg = G("logits")
    logits = torch.full((b * s, ld), 7.0)
    valid = torch.full((b * s,), -1, dtype=torch.int32)
    labels = torch.full((b * s,), -1, dtype=torch.int32)
    cls_w = torch.zeros(b * s)
    ga = torch.full((b * s,), -1, dtype=torch.int32)
    cnt, icw, pcp = torch.zeros(b, ldc, dtype=torch.int32), torch.zeros(b, ldc), torch.zeros(b, ldc)
    npc = torch.zeros(b, dtype=torch.int32)
    rows, o = [], 0
    for i, n in enumerate(sizes):
        r = slice(i * s, i * s + n)
        rows.append(torch.arange(i * s, i * s + n))
        logits[r, col0:col0 + K + 1] = torch.from_numpy(lg[o:o + n])
        valid[r] = 0
        labels[r] = torch.from_numpy(G(f"labels{i}")).int()
        cls_w[r] = torch.from_numpy(G(f"cls_weights{i}"))
        ga[r] = torch.from_numpy(G(f"gt_assignment{i}")).int()
        m = len(G(f"pc_count{i}"))
        npc[i] = m
        cnt[i, :m] = torch.from_numpy(G(f"pc_count{i}")).int()
        icw[i, :m] = torch.from_numpy(G(f"img_cls_weights{i}"))
        pcp[i, :m] = torch.from_numpy(G(f"pc_probs{i}"))
        o += n
    d = lambda t: t.to(dev).contiguous()
    args = dict(logits=d(logits), col0=col0, k=K, valid=d(valid), s=s, b=b, labels=d(labels), cls_weights=d(cls_w), gt_assign=d(ga),
                pc_count=d(cnt), pc_img_cls_weights=d(icw), pc_probs=d(pcp), n_pc=d(npc))
    return args, torch.cat(rows), ld


@pytest.mark.parametrize("tag,K,it", CASES)
def test_pcl_loss_vs_reference(dev, tag, K, it):
    from unit_amd import ops
    a, rows, ld = slots(tag, K, it, dev)
    dy = torch.full((a["b"] * a["s"], ld), 3.0, device=dev)
    loss = ops.pcl_loss(**a, dy=dy, dcol0=a["col0"])
    torch.testing.assert_close(loss.cpu()[0], torch.from_numpy(GOLD[f"{tag}/it{it}/loss"]), rtol=1e-5, atol=1e-6, equal_nan=True)
    g = dy.cpu()
    torch.testing.assert_close(g[rows, a["col0"]:a["col0"] + K + 1], torch.from_numpy(GOLD[f"{tag}/it{it}/grad_logits"]), rtol=2e-4,
                               atol=2e-6)
    pad = torch.ones(g.shape[0], dtype=torch.bool)
    pad[rows] = False
    assert float(g[pad, a["col0"]:a["col0"] + K + 1].abs().max()) == 0.0          # padding rows: zero gradient
    assert float((g[:, :a["col0"]] - 3.0).abs().max()) == 0.0                      # other columns untouched
    assert float((g[:, a["col0"] + K + 1:] - 3.0).abs().max()) == 0.0


@pytest.mark.parametrize("tag,K,it", [CASES[1], CASES[7]])
def test_pcl_loss_bf16_dy_and_reproducible(dev, tag, K, it):
    from unit_amd import ops
    a, rows, ld = slots(tag, K, it, dev)
    outs = []
    for _ in range(3):
        dy = torch.zeros((a["b"] * a["s"], ld), dtype=torch.bfloat16, device=dev)
        loss = ops.pcl_loss(**a, dy=dy, dcol0=a["col0"])
        outs.append((loss.cpu().clone(), dy.cpu().clone()))
    for o in outs[1:]:
        assert torch.equal(outs[0][0], o[0]) and torch.equal(outs[0][1], o[1])
    ref = torch.from_numpy(GOLD[f"{tag}/it{it}/grad_logits"])
    torch.testing.assert_close(outs[0][1][rows, a["col0"]:a["col0"] + K + 1].float(), ref.to(torch.bfloat16).float(), rtol=1e-2, atol=1e-5)
    no_dy = ops.pcl_loss(**a)
    assert torch.equal(no_dy.cpu(), outs[0][0])


def test_pcl_loss_refuses_bad_shapes(dev):
    from unit_amd import ops
    from unit_amd._lib import UnitLibError, check, lib
    from unit_amd.ops import _p, _s
    a, _, ld = slots("P80", 80, 0, dev)
    with pytest.raises(UnitLibError):                                  # K >= 96
        ops.pcl_loss(**dict(a, logits=torch.zeros((a["b"] * a["s"], 100), device=dev), k=96))
    with pytest.raises(UnitLibError):                                  # columns [col0, col0+K+1) beyond the row
        ops.pcl_loss(**dict(a, col0=ld - a["k"]))
    with pytest.raises(UnitLibError):                                  # dy too narrow for [dcol0, dcol0+K+1)
        ops.pcl_loss(**a, dy=torch.zeros((a["b"] * a["s"], a["k"]), device=dev), dcol0=0)
    with pytest.raises(ValueError):                                    # row counts that are not b * s
        ops.pcl_loss(**dict(a, s=a["s"] + 1))
    loss = torch.empty(1, device=dev)
    with pytest.raises(UnitLibError):                                  # the C ABI itself: negative col0
        check(lib().unit_pcl_loss(_p(a["logits"]), ld, -1, 80, _p(a["valid"]), a["s"], a["b"], _p(a["labels"]), _p(a["cls_weights"]),
                                  _p(a["gt_assign"]), _p(a["pc_count"]), _p(a["pc_img_cls_weights"]), _p(a["pc_probs"]), _p(a["n_pc"]),
                                  a["pc_count"].shape[1], 1.0, _p(loss), None, 0, 0, 0, None, _s()), "pcl_loss")
