"""WeaklySupervisedRCNNRPN on the device: unit_pseudo_gt bit for bit against the numpy restatement of meta_arch/rcnn.py:594-599, the fp32
step against the reference's own forward (tests/golden/rpn_pseudo_golden.npz, generator tests/golden/gen_rpn_pseudo_golden.py) at the
tolerances of tests/test_unit_golden_gpu.py::test_hip_step_vs_reference_orchestration, and the behaviour of the weak keys."""
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GDIR = os.path.join(os.path.dirname(__file__), "golden")
sys.path.insert(0, GDIR)
import gen_rpn_pseudo_golden as P  # noqa: E402

FX = np.load(os.path.join(GDIR, "rpn_pseudo_golden.npz"))
K = 20


# ---------------------------------------------------------------------------------------------------- the kernel
def restate(boxes, scores, classes, count, multihot, thr):
    """rcnn.py:594-599 per image, in numpy: (gt_boxes, gt_count, kept_idx) as unit_pseudo_gt lays them out"""
    n, t = scores.shape
    gt, cnt, kept = np.zeros((n, t, 4), np.float32), np.zeros(n, np.int32), np.full((n, t), -1, np.int32)
    for b in range(n):
        rows = [j for j in range(min(max(int(count[b]), 0), t))
                if 0 <= classes[b, j] < multihot.shape[1] and multihot[b, classes[b, j]] and scores[b, j] > np.float32(thr)]
        cnt[b] = len(rows)
        gt[b, :len(rows)] = boxes[b, rows]
        kept[b, :len(rows)] = rows
    return gt, cnt, kept


def _case(n, t, seed, mode):
    g = np.random.default_rng(seed)
    thr = np.float32(0.5)
    boxes = g.random((n, t, 4), dtype=np.float32) * 100
    scores = g.random((n, t), dtype=np.float32)
    classes = g.integers(-1, K + 2, size=(n, t)).astype(np.int32)          # -1 (the fill of unused rows) and K, K + 1: outside the labels
    count = g.integers(0, t + 1, size=n).astype(np.int32)
    multihot = np.zeros((n, K), np.uint8)
    for b in range(n):
        labels = g.integers(0, K, size=3)
        labels[2] = labels[1]          # duplicate labels: the multi-hot row holds a class once
        multihot[b, labels] = 1
    scores[:, ::5] = thr                                                   # equal to the threshold: dropped (strict comparison)
    scores[:, 3::7] = np.nan                                               # NaN: dropped
    scores[:, 4::11] = np.inf
    if mode == "mixed" and t >= 63:          # at least one kept row per image whatever the draw: a labelled class, above the threshold, inside count
        count = g.integers(t // 2 + 1, t + 1, size=n).astype(np.int32)
        for b in range(n):
            classes[b, t // 2], scores[b, t // 2] = int(np.nonzero(multihot[b])[0][0]), np.float32(0.9)
    if mode == "count_zero":
        count[:] = 0
    elif mode == "count_full":
        count[:] = t
    elif mode == "none":
        multihot[:] = 0
        count[:] = t
    elif mode == "all":
        multihot[:] = 1
        classes = g.integers(0, K, size=(n, t)).astype(np.int32)
        scores = thr + np.float32(0.01) + g.random((n, t), dtype=np.float32)
        count[:] = t
    return boxes, scores, classes, count, multihot, thr


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("t", [1, 63, 64, 65, 100, 256, 257, 600])          # wave and chunk boundaries (64 lanes, 256 rows per chunk)
def test_pseudo_gt_kernel_bit_for_bit(dev, n, t):
    from unit_amd import ops
    for mode in ("mixed", "count_zero", "count_full", "none", "all"):
        boxes, scores, classes, count, multihot, thr = _case(n, t, 1000 * n + t, mode)
        d = lambda a: torch.from_numpy(a).to(dev)
        gt, cnt, kept = ops.pseudo_gt(d(boxes), d(scores), d(classes), d(count), d(multihot), float(thr))
        rgt, rcnt, rkept = restate(boxes, scores, classes, count, multihot, thr)
        assert np.array_equal(cnt.cpu().numpy(), rcnt), (mode, cnt.tolist(), rcnt.tolist())
        assert np.array_equal(kept.cpu().numpy(), rkept), mode
        assert np.array_equal(gt.cpu().numpy().view(np.uint32), rgt.view(np.uint32)), mode
        if mode == "none" or mode == "count_zero":
            assert int(cnt.sum()) == 0
        if mode == "all":
            assert cnt.tolist() == [t] * n
        if mode == "mixed" and t >= 63:
            assert (rcnt >= 1).all() and (rcnt < count).all()


def test_pseudo_gt_argument_checks(dev):
    from unit_amd import ops
    from unit_amd._lib import UnitLibError
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)
    with pytest.raises(UnitLibError, match="T <= 1024"):
        ops.pseudo_gt(z(1, 1025, 4), z(1, 1025), z(1, 1025, dt=torch.int32), z(1, dt=torch.int32), z(1, K, dt=torch.uint8), 0.5)


def test_gate_anchor_labels(dev):
    from unit_amd import ops
    lab = torch.randint(-1, 2, (3, 777), dtype=torch.int8, device=dev)
    cnt = torch.tensor([2, 0, 1], dtype=torch.int32, device=dev)
    want = lab.clone()
    want[1] = -1
    assert torch.equal(ops.gate_anchor_labels(lab, cnt), want)


# ---------------------------------------------------------------------------------------------------- the step
def _dperms(cfg, batch, perms, dev):
    cap = cfg.MODEL.RPN.POST_NMS_TOPK_TRAIN + batch.gt_boxes.shape[1]
    roi = torch.stack([torch.cat([p, torch.arange(len(p), cap)]) for p in perms["roi"]])      # capacity-sized permutation
    return {"rpn": torch.stack(perms["rpn"]).int().to(dev), "roi": roi.int().to(dev), "weak_rpn": torch.stack(perms["weak_rpn"]).int().to(dev)}


@functools.lru_cache(maxsize=None)
def _step(regressor=True, dtype="fp32", with_weak=True, flip_empty=False, plugin=False):
    """one training step of the fixture's model -> dict of host copies (computed once per form, shared by the tests below)"""
    dev = torch.device("cuda:0")
    cfg, model, sup, weak, perms = P.pseudo_inputs(device="cuda", regressor=regressor)
    model.train()
    model.compute_mode = dtype
    if flip_empty:
        i = min(range(2), key=lambda j: len(FX[f"on/weak/kept{j}"]))          # the weak image without pseudo ground truth: other pixels
        weak[i]["image"] = weak[i]["image"].flip(-1).contiguous()
    batch = model.pack_batch(sup, weak if with_weak else None)
    model._ensure_ready()
    dperms = _dperms(cfg, batch, perms, dev)
    out = {}
    if plugin:
        model.next_perms = dperms
        loss_dict = model(sup, weak if with_weak else None)
        sum(loss_dict.values()).backward()
        out["loss_dict"] = {k: float(v.detach()) for k, v in loss_dict.items()}
    else:
        step = model.forward_train(batch, dperms, early_backward=True)
        model.backward_train(step)
        out["losses"] = dict(zip(model.loss_names, step.losses.cpu().tolist()))
        out["anchor_labels"] = step.anchor_labels.cpu().numpy()
        if step.weak is not None:
            out["weak"] = {k: v.cpu().numpy() for k, v in step.weak.items()}
    torch.cuda.synchronize()
    assert model.proposal_generator.rpn_head.second_group is None          # consumed by the step's one RPN-head backward
    out["grads"] = {n: q.grad.detach().cpu().clone() for n, q in model.named_parameters() if q.requires_grad and q.grad is not None}
    return out


@pytest.mark.parametrize("tag", P.CASES)
def test_fp32_step_vs_the_reference_forward(dev, tag):
    """losses 1e-4, pseudo-GT rows and weak anchor labels exact, gradient norms and heads 2e-3 of the norm: the bars of
    test_unit_golden_gpu.py::test_hip_step_vs_reference_orchestration on the same quantities"""
    r = _step(regressor=(tag == "on"))
    names = [str(k) for k in FX[f"{tag}/loss_names"]]
    for k, v in zip(names, FX[f"{tag}/losses"]):
        print(tag, k, r["losses"][k], v)
        assert abs(r["losses"][k] - v) <= 1e-4 * max(1.0, abs(v)), (tag, k, r["losses"][k], v)
    for k in set(r["losses"]) - set(names):          # slots the reference's dictionary does not have: never written
        assert r["losses"][k] == 0.0, k
    assert np.array_equal(r["anchor_labels"], FX[f"{tag}/anchor_labels"])
    w = r["weak"]
    for i in range(2):
        kept = FX[f"{tag}/weak/kept{i}"]
        assert int(w["gt_count"][i]) == len(kept) and np.array_equal(w["kept"][i, :len(kept)], kept) and (w["kept"][i, len(kept):] == -1).all()
        assert np.abs(w["gt_boxes"][i, :len(kept)] - FX[f"{tag}/weak/pseudo_boxes{i}"]).max(initial=0.0) <= 1e-4 * 128
        assert (w["gt_boxes"][i, len(kept):] == 0).all()
        key = f"{tag}/weak/anchor_labels{i}"
        if key in FX.files:
            assert np.array_equal(w["anchor_labels"][i], FX[key])
        else:
            assert (w["anchor_labels"][i] == -1).all()          # gated: no background anchor of this image is sampled into the loss
    pre = f"{tag}/gradnorm/"
    keys = [k[len(pre):] for k in FX.files if k.startswith(pre)]
    assert sum(k.startswith("proposal_generator.rpn_head.") for k in keys) == 6 and any(k.startswith("backbone.") for k in keys)
    for k in keys:
        g = r["grads"][k]
        n = float(FX[pre + k])
        print(tag, k, abs(g.double().norm().item() - n) / n)
        assert abs(g.double().norm().item() - n) <= 2e-3 * n + 1e-8, (tag, k, g.double().norm().item(), n)
        ref = torch.from_numpy(FX[f"{tag}/gradhead/{k}"])
        if g.dim() == 4:
            g = g.contiguous()
        assert (g.reshape(-1)[: ref.numel()] - ref).abs().max() <= 2e-3 * n + 1e-8, (tag, k)


def test_the_weak_half_adds_nothing_below_the_rpn_head(dev):
    """backbone and ROI-head gradients equal the supervised-only step's bit for bit; the RPN head's three convolutions do not"""
    a, b = _step()["grads"], _step(with_weak=False)["grads"]
    assert set(a) == set(b)
    moved = [n for n in a if not torch.equal(a[n], b[n])]
    assert sorted(moved) == sorted(n for n in a if n.startswith("proposal_generator.rpn_head.")) and len(moved) == 6, moved
    assert any(n.startswith("backbone.") for n in a) and any(n.startswith("roi_heads.box_head.") for n in a)


def test_weak_keys_edge_behaviour(dev):
    on, off, sup_only = _step(), _step(regressor=False), _step(with_weak=False)
    # weak_batched_inputs=None: the two slots stay zero and the dictionary has no weak keys (below); the other losses are the same
    assert sup_only["losses"]["weak_loss_rpn_cls"] == 0.0 and sup_only["losses"]["weak_loss_rpn_loc"] == 0.0 and "weak" not in sup_only
    for k in ("loss_cls", "loss_box_reg", "loss_rpn_cls", "loss_rpn_loc"):
        assert sup_only["losses"][k] == on["losses"][k], k
    for k in ("loss_im_cls", "loss_oicr_1", "loss_oicr_2", "loss_oicr_3"):          # rcnn.py:644: the ROI heads never see the weak batch
        assert on["losses"][k] == 0.0
    # TRAIN_PROPOSAL_REGRESSOR off: the loc term is exactly 0, the cls term unchanged
    assert off["losses"]["weak_loss_rpn_loc"] == 0.0 and on["losses"]["weak_loss_rpn_loc"] > 0.0
    assert off["losses"]["weak_loss_rpn_cls"] == on["losses"]["weak_loss_rpn_cls"]
    assert torch.equal(off["grads"]["proposal_generator.rpn_head.objectness_logits.weight"], on["grads"]["proposal_generator.rpn_head.objectness_logits.weight"])
    assert not torch.equal(off["grads"]["proposal_generator.rpn_head.anchor_deltas.weight"], on["grads"]["proposal_generator.rpn_head.anchor_deltas.weight"])


def test_weak_image_without_pseudo_gt_changes_nothing(dev):
    """other pixels in the weak image that keeps no detection (it still keeps none): every loss and every gradient bit for bit the same"""
    a, b = _step(), _step(flip_empty=True)
    i = min(range(2), key=lambda j: len(FX[f"on/weak/kept{j}"]))
    assert int(b["weak"]["gt_count"][i]) == 0 and int(b["weak"]["gt_count"][1 - i]) == int(a["weak"]["gt_count"][1 - i]) >= 2
    assert not np.array_equal(a["weak"]["det_scores"][i], b["weak"]["det_scores"][i])          # its detections did change
    assert a["losses"] == b["losses"]
    for n in a["grads"]:
        assert torch.equal(a["grads"][n], b["grads"][n]), n


def test_plugin_forward_and_autograd_equal_train_step(dev):
    a, p = _step(), _step(plugin=True)
    assert set(p["loss_dict"]) == {"loss_cls", "loss_box_reg", "loss_rpn_cls", "loss_rpn_loc", "weak_loss_rpn_cls", "weak_loss_rpn_loc"}
    for k, v in p["loss_dict"].items():
        assert abs(v - a["losses"][k]) <= 1e-6 * max(1.0, abs(a["losses"][k])), (k, v, a["losses"][k])
    for n, g in a["grads"].items():
        assert (p["grads"][n] - g).abs().max().item() <= 1e-5 * g.abs().max().item() + 1e-8, n
    q = _step(with_weak=False, plugin=True)
    assert set(q["loss_dict"]) == {"loss_cls", "loss_box_reg", "loss_rpn_cls", "loss_rpn_loc"}          # rcnn.py:630-632


def test_bf16_step_keeps_the_same_detections(dev):
    r, f = _step(dtype="bf16"), _step()
    vals = [r["losses"][k] for k in ("loss_cls", "loss_box_reg", "loss_rpn_cls", "loss_rpn_loc", "weak_loss_rpn_cls", "weak_loss_rpn_loc")]
    assert np.isfinite(vals).all() and min(vals) > 0, vals
    assert np.array_equal(r["weak"]["gt_count"], f["weak"]["gt_count"]) and np.array_equal(r["weak"]["kept"], f["weak"]["kept"])


def test_trainer_runs_the_class_eagerly_and_refuses_graph_and_replay(dev):
    from unit_amd import engine
    cfg, model, sup, weak, perms = P.pseudo_inputs(device="cuda")
    model.train()
    model.compute_mode = "bf16"
    for kw in (dict(use_graph=True), dict(use_replay=True)):
        with pytest.raises(NotImplementedError, match="runs eagerly only"):
            engine.TrainerNoMeta(cfg, model, **kw)
    fired = []
    tr = engine.TrainerNoMeta(cfg, model, metrics=True)
    model.on_grad_ready = fired.append
    for _ in range(2):
        tr.run_step(sup, weak)
    d = tr.loss_dict()
    assert list(d)[-2:] == ["weak_loss_rpn_cls", "weak_loss_rpn_loc"] and all(np.isfinite(v) for v in d.values())
    assert fired.count("rpn") == 2          # the bucket's hook fires once per step: after the sum of both row groups
    assert model.last_metrics_images == len(sup)          # the step scalars keep counting over the supervised images only
    m = tr.metrics_dict()
    sup_labels = FX["on/anchor_labels"]          # (how many anchors a sampler takes does not depend on its permutation)
    assert m["rpn/num_pos_anchors"] == (sup_labels == 1).sum() / len(sup) and m["rpn/num_neg_anchors"] == (sup_labels == 0).sum() / len(sup)


def test_nometa_step_records_the_parent_commits_call_list(dev):
    """a WeaklySupervisedRCNNNoMeta step is untouched by the new class: the calls it records are, name for name and in order, the ones the
    commit before recorded for the same setup (tests/golden/rpn_pseudo_parent_plan.json, written there by gen_rpn_pseudo_parent_plan.py),
    and its four loss vectors are that commit's bit for bit"""
    import gen_rpn_pseudo_parent_plan as Q
    with open(os.path.join(GDIR, "rpn_pseudo_parent_plan.json")) as f:
        parent = json.load(f)
    got = Q.run()
    assert got["stats"] == parent["stats"] == {"eager": 2, "captured": 1, "replayed": 1}
    assert len(got["names"]) == len(parent["names"]) and got["names"] == parent["names"]
    assert "unit_pseudo_gt" not in got["names"] and "unit_gate_anchor_labels" not in got["names"]
    assert got["losses"] == parent["losses"]


def test_weak_batch_of_another_size_rpn_gradient_vs_autograd(dev):
    """the usual case in training: the weak batch pads to another size than the supervised one (here 112 x 160 from a 112 x 144 and an 80 x 160
    image, against 96 x 128), so the RPN conv's weight gradient takes two parts of different geometry. What the weak half adds to the six
    RPN-head gradients (step with weak images minus supervised-only step, fp32) against torch autograd on the CPU through the same head and
    the oracle's RPN loss, combined as rcnn.py:601-609, :622-624; the two weak losses to 1e-4, the gradients to 2e-3 of their norm"""
    import torch.nn.functional as F
    import unit_oracle as orc
    from unit_amd import ops
    thr, sizes = 0.3, [(112, 144), (80, 160)]
    g = torch.Generator().manual_seed(5)
    wperm = torch.stack([torch.randperm(7 * 10 * 15, generator=g) for _ in sizes]).int().to(dev)
    imgs = [torch.rand(3, h, w, generator=g) * 255.0 for h, w in sizes]

    def run(with_weak):
        cfg, model, sup, weak, perms = P.pseudo_inputs(device="cuda", threshold=thr)
        model.train()
        model.compute_mode = "fp32"
        for x, im in zip(weak, imgs):
            x["image"], x["height"], x["width"] = im, im.shape[1], im.shape[2]
            x["instances"] = type(x["instances"])(tuple(im.shape[1:]), gt_classes=torch.arange(K))          # every class a label
        batch = model.pack_batch(sup, weak if with_weak else None)
        model._ensure_ready()
        dperms = _dperms(cfg, batch, perms, dev)
        dperms["weak_rpn"] = wperm
        step = model.forward_train(batch, dperms, early_backward=True)
        model.backward_train(step)
        torch.cuda.synchronize()
        grads = {n: q.grad.detach().cpu().clone() for n, q in model.named_parameters() if n.startswith("proposal_generator.rpn_head.")}
        return model, batch, step, grads

    model, batch, step, ga = run(True)
    _, _, _, gb = run(False)
    w = {k: v.cpu().numpy() for k, v in step.weak.items()}
    assert w["gt_count"].min() >= 1, w["gt_count"]          # both images have pseudo ground truth at this threshold
    # the reference arithmetic on the CPU, from the weak feature map the device's backbone gives
    with torch.no_grad():
        x, _ = ops.preprocess_images(batch.images[batch.n_sup:], model._pixel_mean, model._pixel_std, torch.float32, 8, model.normalize_images)
        feat = model.backbone.fwd(x)[0].permute(0, 3, 1, 2).contiguous().cpu()
    assert tuple(feat.shape[-2:]) == (7, 10)
    pre = "proposal_generator.rpn_head."
    p = {n: q.detach().cpu().clone().contiguous().requires_grad_(True) for n, q in model.named_parameters() if n.startswith(pre)}
    t = F.relu(F.conv2d(feat, p[pre + "conv.weight"], p[pre + "conv.bias"], padding=1))
    lg = F.conv2d(t, p[pre + "objectness_logits.weight"], p[pre + "objectness_logits.bias"]).permute(0, 2, 3, 1).flatten(1)
    dl = F.conv2d(t, p[pre + "anchor_deltas.weight"], p[pre + "anchor_deltas.bias"])
    dl = dl.view(dl.shape[0], -1, 4, 7, 10).permute(0, 3, 4, 1, 2).flatten(1, -2)
    anchors = orc.grid_anchors(7, 10)
    cls, loc = [], []
    for i in range(2):
        gt = torch.from_numpy(w["gt_boxes"][i, : w["gt_count"][i]])
        lab, matched = orc.label_and_sample_anchors(anchors, [gt], [wperm[i].long().cpu()])
        assert np.array_equal(lab[0].numpy(), w["anchor_labels"][i]), i
        li = orc.rpn_losses(anchors, lg[i:i + 1], lab, dl[i:i + 1], matched, batch_size_per_image=256)
        cls.append(li["loss_rpn_cls"] * thr * P.DIVISOR)
        loc.append(li["loss_rpn_loc"] * thr * P.DIVISOR)
    cls, loc = torch.stack(cls).mean(), torch.stack(loc).mean()
    (cls + loc).backward()
    got = dict(zip(model.loss_names, step.losses.cpu().tolist()))
    for k, v in (("weak_loss_rpn_cls", cls.item()), ("weak_loss_rpn_loc", loc.item())):
        print(k, got[k], v)
        assert v > 0 and abs(got[k] - v) <= 1e-4 * max(1.0, abs(v)), (k, got[k], v)
    for n, q in p.items():
        d, n_ref = ga[n] - gb[n], q.grad.double().norm().item()
        print(n, "weak share of the gradient", n_ref / gb[n].double().norm().item(), "error / norm", (d - q.grad).double().norm().item() / n_ref)
        assert n_ref > 0 and abs(d.double().norm().item() - n_ref) <= 2e-3 * n_ref + 1e-8, (n, d.double().norm().item(), n_ref)
        assert (d - q.grad).abs().max().item() <= 2e-3 * n_ref + 1e-8, n
