"""unit_pcl_targets (csrc/pcl.hip) against the reference's own TYPE "PCL" weak detector under the canonical tie rule
(tests/golden/pcl_targets_golden.npz, `stable/...`; on tie-free units that is the unmodified reference) and, where no recording exists,
against the numpy restatement tests/golden/pcl_targets.py: integer decisions and cls_weights exact, the summed floats within rtol 1e-5;
then unit_pcl_targets -> unit_pcl_loss against the recorded losses and logits gradients (the bars of tests/test_pcl_gpu.py)."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GDIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GDIR)
import pcl_targets as pt  # noqa: E402

G = np.load(os.path.join(GDIR, "pcl_targets_golden.npz"))
OLD = np.load(os.path.join(GDIR, "pcl_golden.npz"))
TAGS = pt.tags(G)
DENSE = [t for t in TAGS if not int(G[f"{t}/sparse"])]
OUT_KEYS = ("labels", "cls_weights", "gt_assign", "n_pc", "pc_labels", "pc_count", "pc_img_cls_weights", "pc_probs")


def slots(dev, K, boxes, mats, classes, pad=3, col0=(2, 1), tail=2):
    """images of different sizes in fixed slots of S = max rows + pad; mats = (src, nxt) row-concatenated matrices, each embedded at its
    column offset in a wider matrix filled with 7 (so a wrong column or row shows)"""
    sizes = [len(b) for b in boxes]
    b, s = len(sizes), max(sizes) + pad
    rois5 = torch.zeros(b * s, 5)
    valid = torch.full((b * s,), -1, dtype=torch.int32)
    multihot = torch.zeros(b, K, dtype=torch.uint8)
    wide = [torch.full((b * s, c0 + m.shape[1] + tail), 7.0) for m, c0 in zip(mats, col0)]
    o = 0
    for i, n in enumerate(sizes):
        r = slice(i * s, i * s + n)
        rois5[r, 0] = i
        rois5[r, 1:] = torch.from_numpy(np.asarray(boxes[i], np.float32))
        valid[r] = 0
        multihot[i, torch.tensor(list(classes[i]), dtype=torch.long)] = 1
        for w, m, c0 in zip(wide, mats, col0):
            w[r, c0:c0 + m.shape[1]] = torch.from_numpy(np.asarray(m[o:o + n], np.float32))
        o += n
    d = lambda t: t.to(dev).contiguous()
    return dict(src=d(wide[0]), col0=col0[0], nxt=d(wide[1]), ncol0=col0[1], k=K, rois5=d(rois5), valid=d(valid), s=s, b=b,
                multihot=d(multihot)), sizes


def per_image(out, sizes, s, t=0):
    """the launch's fixed-slot outputs of stream t -> per image dicts with the reference's names; checks the padding rows and slots"""
    o = {k: v[t].cpu().numpy() for k, v in out.items()}
    res = []
    for i, n in enumerate(sizes):
        m = int(o["n_pc"][i])
        r = slice(i * s, i * s + n)
        pad = slice(i * s + n, (i + 1) * s)
        assert (o["labels"][pad] == -1).all() and (o["gt_assign"][pad] == -1).all() and (o["cls_weights"][pad] == 0).all()
        assert (o["pc_count"][i, m:] == 0).all() and (o["pc_labels"][i, m:] == -1).all()
        res.append(dict(labels=o["labels"][r], cls_weights=o["cls_weights"][r], gt_assignment=o["gt_assign"][r], pc_labels=o["pc_labels"][i, :m],
                        pc_count=o["pc_count"][i, :m], img_cls_weights=o["pc_img_cls_weights"][i, :m], pc_probs=o["pc_probs"][i, :m]))
    return res


def case_inputs(tag):
    sizes, K = G[f"{tag}/sizes"].tolist(), int(G[f"{tag}/K"])
    boxes = [G[f"{tag}/boxes{i}"] for i in range(len(sizes))]
    classes = [G[f"{tag}/targets{i}"].tolist() for i in range(len(sizes))]
    return sizes, K, boxes, classes


@pytest.mark.parametrize("tag", TAGS)
def test_pcl_targets_mode0_vs_reference(dev, tag):
    from unit_amd import ops
    sizes, K, boxes, classes = case_inputs(tag)
    for it in range(3):
        p0, p1 = pt.case_probs(G, tag, it)
        a, _ = slots(dev, K, boxes, (p0, p1), classes)
        got = per_image(ops.pcl_targets(**a, mode=0, nmode=0, ldc=5 * max(len(c) for c in classes) + 1), sizes, a["s"])
        for i in range(len(sizes)):
            pt.check_unit(got[i], pt.expected(G, tag, it, i, "stable"), f"{tag} it{it} image {i} (stable)")
            if int(G[f"{tag}/it{it}/tie_free{i}"]):
                pt.check_unit(got[i], pt.expected(G, tag, it, i, "ref"), f"{tag} it{it} image {i} (ref)")


@pytest.mark.parametrize("tag", DENSE)
def test_pcl_targets_mode1_on_logits(dev, tag):
    """logits in, softmax in the kernel: bit-equal to mode 0 fed with ops.softmax_rows of the same logits, integers equal to the recording"""
    from unit_amd import ops
    sizes, K, boxes, classes = case_inputs(tag)
    ldc = 5 * max(len(c) for c in classes)
    for it in range(3):
        lg1 = pt.recorded(G, OLD, tag, it, "logits")
        if it == 0:
            src, mode = G[f"{tag}/it0/probs"], 0
        else:
            src, mode = pt.recorded(G, OLD, tag, it - 1, "logits"), 1
        a, _ = slots(dev, K, boxes, (src, lg1), classes)
        out1 = ops.pcl_targets(**a, mode=mode, nmode=1, ldc=ldc)
        sm = lambda m: ops.softmax_rows(torch.from_numpy(np.ascontiguousarray(m)).to(dev), K + 1).cpu().numpy()
        a0, _ = slots(dev, K, boxes, (sm(src) if mode else src, sm(lg1)), classes)
        out0 = ops.pcl_targets(**a0, mode=0, nmode=0, ldc=ldc)
        for k in OUT_KEYS:
            assert np.array_equal(out1[k].cpu().numpy(), out0[k].cpu().numpy(), equal_nan=True), f"{tag} it{it} {k}"
        got = per_image(out1, sizes, a["s"])
        for i in range(len(sizes)):
            exp = pt.expected(G, tag, it, i, "stable")
            for key in pt.INT_KEYS:
                assert np.array_equal(got[i][key].astype(np.int64), exp[key].astype(np.int64)), f"{tag} it{it} image {i} {key}"


def _random_case(seed, K, sizes, classes, scale, w=400.0, h=300.0):
    g = np.random.default_rng(seed)
    boxes, p0, p1 = [], [], []
    for n in sizes:
        c = g.integers(0, 3, n)
        ctr = np.array([[100, 90, 120, 100], [280, 180, 150, 140], [200, 120, 60, 200]], np.float32)[c]
        jit = (g.random((n, 4)).astype(np.float32) - 0.5) * np.array([30, 30, 60, 60], np.float32)
        cx, cy, bw, bh = ctr[:, 0] + jit[:, 0], ctr[:, 1] + jit[:, 1], np.maximum(ctr[:, 2] + jit[:, 2], 8), np.maximum(ctr[:, 3] + jit[:, 3], 8)
        b = np.stack([np.clip(cx - bw / 2, 0, w), np.clip(cy - bh / 2, 0, h), np.clip(cx + bw / 2, 0, w), np.clip(cy + bh / 2, 0, h)], 1)
        boxes.append(b.astype(np.float32))
        mil = pt.softmax(g.normal(size=(n, K)) * scale * 6) * pt.softmax((g.normal(size=(n, K)) * scale * 6).T).T
        p0.append(mil.astype(np.float32))
        p1.append(pt.softmax(g.normal(size=(n, K + 1)) * scale * 6))
    return boxes, np.concatenate(p0), np.concatenate(p1)


def _vs_restatement(dev, K, sizes, classes, seed, scale, boxes_edit=None):
    from unit_amd import ops
    boxes, p0, p1 = _random_case(seed, K, sizes, classes, scale)
    if boxes_edit is not None:
        boxes_edit(boxes)
    a, _ = slots(dev, K, boxes, (p0, p1), classes, pad=0)
    out = ops.pcl_targets(**a, mode=0, nmode=0, ldc=5 * max(1, max(len(c) for c in classes)))
    got = per_image(out, sizes, a["s"])
    o, exps = 0, []
    for i, n in enumerate(sizes):
        exp = pt.image_targets(boxes[i], p0[o:o + n], p1[o:o + n], sorted(classes[i]), K)
        pt.check_unit(got[i], exp, f"image {i}")
        exps.append(exp)
        o += n
    return a, out, exps


def test_pcl_targets_2048_rows_near_uniform_and_tiny_images(dev):
    """S = 2048 with near-uniform scores (large top-ranking sets, equal degrees everywhere), images with 1 and 2 rows, an image without a class"""
    _vs_restatement(dev, 20, [2048, 1, 2, 300], [[3, 7, 12], [5], [0, 19], []], 31, 0.02)


def test_pcl_targets_k80_eight_classes(dev):
    _vs_restatement(dev, 80, [600, 512], [[0, 9, 17, 30, 41, 55, 68, 79], [5, 6]], 32, 0.3)


def test_pcl_targets_peaked_512(dev):
    _vs_restatement(dev, 20, [512, 512], [[1, 4], [0, 8, 15]], 33, 0.5)


def test_pcl_targets_zero_area_boxes_poison_the_image(dev):
    """no self-edge on a zero-area box: the reference raises (torch.max of an empty tensor); here the launch finishes (every loop is counted),
    the image's weights are NaN and so is the loss; the other image of the launch is untouched"""
    from unit_amd import ops

    def flat(boxes):
        boxes[0][:, 2] = boxes[0][:, 0]
    a, out, exps = _vs_restatement(dev, 20, [40, 30], [[2, 6], [9]], 34, 0.05, boxes_edit=flat)
    assert exps[0]["poisoned"] and not exps[1]["poisoned"]
    assert torch.isnan(out["cls_weights"][0, :40]).all() and torch.isfinite(out["cls_weights"][0, a["s"]:]).all()
    g = torch.Generator().manual_seed(1)
    logits = torch.randn(a["b"] * a["s"], 21, generator=g).to(dev)
    loss = ops.pcl_loss(logits, 0, 20, a["valid"], a["s"], a["b"], out["labels"][0], out["cls_weights"][0], out["gt_assign"][0], out["pc_count"][0],
                        out["pc_img_cls_weights"][0], out["pc_probs"][0], out["n_pc"][0])
    assert torch.isnan(loss).all()


def test_pcl_targets_stream_list_and_reproducible(dev):
    """two streams in one launch (column steps) equal two single launches; three launches bit-identical"""
    from unit_amd import ops
    tag = "S40"
    sizes, K, boxes, classes = case_inputs(tag)
    lg = [pt.recorded(G, OLD, tag, it, "logits") for it in range(3)]
    a, _ = slots(dev, K, boxes, (np.concatenate(lg, 1), np.concatenate(lg, 1)), classes, col0=(3, 3))
    kw = dict(a, mode=1, nmode=1, ldc=16)
    del kw["ncol0"], kw["col0"]
    both = [ops.pcl_targets(**kw, n_streams=2, step=K + 1, nstep=K + 1, col0=3, ncol0=3 + K + 1) for _ in range(3)]
    for t in range(2):
        one = ops.pcl_targets(**kw, col0=3 + t * (K + 1), ncol0=3 + (t + 1) * (K + 1))
        for k in OUT_KEYS:
            assert np.array_equal(both[0][k][t].cpu().numpy(), one[k][0].cpu().numpy(), equal_nan=True), (t, k)
        got = per_image(both[0], sizes, a["s"], t)
        for i in range(len(sizes)):
            exp = pt.expected(G, tag, t + 1, i, "stable")
            for key in pt.INT_KEYS:
                assert np.array_equal(got[i][key].astype(np.int64), exp[key].astype(np.int64)), (t, i, key)
    for r in both[1:]:
        for k in OUT_KEYS:
            assert np.array_equal(both[0][k].cpu().numpy(), r[k].cpu().numpy(), equal_nan=True), k


def test_pcl_targets_refuses_bad_shapes(dev):
    from unit_amd import ops
    from unit_amd._lib import UnitLibError, lib
    sizes, K, boxes, classes = case_inputs("S16")
    p0, p1 = pt.case_probs(G, "S16", 0)
    a, _ = slots(dev, K, boxes, (p0, p1), classes)
    ok = dict(a, mode=0, nmode=0, ldc=10)
    ops.pcl_targets(**ok)
    with pytest.raises(UnitLibError):
        ops.pcl_targets(**dict(ok, k=96, multihot=torch.zeros(a["b"], 96, dtype=torch.uint8, device=dev)))
    with pytest.raises(UnitLibError):
        ops.pcl_targets(**dict(ok, ldc=4))                                   # smaller than max_pc_num
    with pytest.raises(UnitLibError):
        ops.pcl_targets(**dict(ok, col0=a["src"].shape[1] - K + 1))         # source columns beyond the row
    with pytest.raises(UnitLibError):
        ops.pcl_targets(**dict(ok, ncol0=a["nxt"].shape[1] - K))            # next-iteration columns beyond the row
    with pytest.raises(UnitLibError):
        ops.pcl_targets(**dict(ok, n_streams=2, step=K))                     # the second stream's columns beyond the row
    with pytest.raises(UnitLibError):
        ops.pcl_targets(**dict(ok, mode=2))
    big = 2049
    with pytest.raises(UnitLibError):                                        # S above the supported maximum
        ops.pcl_targets(torch.zeros(big, K, device=dev), 0, 0, torch.zeros(big, K + 1, device=dev), 0, 0, K, torch.zeros(big, 5, device=dev),
                        torch.zeros(big, dtype=torch.int32, device=dev), big, 1, torch.zeros(1, K, dtype=torch.uint8, device=dev), 10)
    p = lambda t: t.data_ptr()
    o = ops.pcl_targets(**ok)
    need = lib().unit_workspace_bytes_pcl_targets(a["b"], a["s"], 1)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    st = lib().unit_pcl_targets(p(a["src"]), a["src"].shape[1], a["col0"], 0, 0, p(a["nxt"]), a["nxt"].shape[1], a["ncol0"], 0, 0, K, p(a["rois5"]),
                                p(a["valid"]), a["s"], a["b"], 1, p(a["multihot"]), 0.5, 0.1, 0.4, 5, p(o["labels"]), p(o["cls_weights"]),
                                p(o["gt_assign"]), p(o["n_pc"]), p(o["pc_labels"]), p(o["pc_count"]), p(o["pc_img_cls_weights"]),
                                p(o["pc_probs"]), 10, p(ws), need - 17, torch.cuda.current_stream().cuda_stream)
    assert st < 0 and b"workspace" in lib().unit_last_error()


@pytest.mark.parametrize("tag", DENSE)
def test_pcl_targets_then_loss_vs_reference(dev, tag):
    """the composition the model runs: loss within rtol 1e-5 (NaN where the reference's is), logits gradient rtol 2e-4 / atol 2e-6"""
    from unit_amd import ops
    sizes, K, boxes, classes = case_inputs(tag)
    for it in range(3):
        lg1 = pt.recorded(G, OLD, tag, it, "logits")
        src, mode = (G[f"{tag}/it0/probs"], 0) if it == 0 else (pt.recorded(G, OLD, tag, it - 1, "logits"), 1)
        a, _ = slots(dev, K, boxes, (src, lg1), classes)
        t = ops.pcl_targets(**a, mode=mode, nmode=1, ldc=5 * max(len(c) for c in classes))
        dy = torch.full((a["b"] * a["s"], a["nxt"].shape[1]), 3.0, device=dev)
        loss = ops.pcl_loss(a["nxt"], a["ncol0"], K, a["valid"], a["s"], a["b"], t["labels"][0], t["cls_weights"][0], t["gt_assign"][0],
                            t["pc_count"][0], t["pc_img_cls_weights"][0], t["pc_probs"][0], t["n_pc"][0], dy=dy, dcol0=a["ncol0"])
        torch.testing.assert_close(loss.cpu()[0], torch.from_numpy(pt.recorded(G, OLD, tag, it, "loss")), rtol=1e-5, atol=1e-6, equal_nan=True)
        rows = torch.cat([torch.arange(i * a["s"], i * a["s"] + n) for i, n in enumerate(sizes)])
        torch.testing.assert_close(dy.cpu()[rows, a["ncol0"]:a["ncol0"] + K + 1], torch.from_numpy(pt.recorded(G, OLD, tag, it, "grad_logits")),
                                   rtol=2e-4, atol=2e-6)
