"""Test-time augmentation (TEST.AUG) on the device: the three kernels against numpy restatements, bit for bit; the resized views against
Pillow's (stored in the fixture); the model-level result against the fixture recorded from the reference's own `inference`
(tests/golden/gen_tta_golden.py -> tests/golden/tta_golden.npz). fp32 compute mode unless stated."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GDIR = os.path.join(HERE, "golden")
for p_ in (HERE, GDIR):
    if p_ not in sys.path:
        sys.path.insert(0, p_)
import tta_ref  # noqa: E402

GOLD = np.load(os.path.join(GDIR, "tta_golden.npz"))
H, W = 96, 128
RECORDED = ("tta", "tta_ft", "tta_noflip")
_MODELS = {}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def model_of(name):
    """the fixture case's model (shared between the tests of one model), its TEST.AUG set to the case's"""
    import gen_ref_step as S
    from unit_amd.config import CN
    case = tta_ref.CASE_MODEL[name]
    if case not in _MODELS:
        cfg, model, sup, _, _, _ = S.step_inputs(case, device="cuda")
        model.eval()
        _MODELS[case] = (model, sup[0]["image"])
    model, image = _MODELS[case]
    sizes, max_size, flip = tta_ref.CASE_AUG[name]
    model.cfg.TEST.AUG = CN(ENABLED=True, MIN_SIZES=sizes, MAX_SIZE=max_size, FLIP=flip)
    model.compute_dtype = torch.float32
    return model, image


def inputs_of(name, image, device=None):
    from unit_amd.structures import Boxes, Instances
    boxes = torch.from_numpy(GOLD[f"{name}/proposals"])
    if device is not None:
        boxes, image = boxes.to(device), image.to(device)
    return {"image": image, "height": 2 * H, "width": 2 * W, "proposals": Instances((H, W), proposal_boxes=Boxes(boxes))}


# ---------------------------------------------------------------------------------------------------------------- unit_tta_boxes
@pytest.mark.parametrize("p", [0, 1, 63, 64, 65, 257])
def test_tta_boxes_bit_for_bit(dev, p):
    from unit_amd import ops
    g = np.random.RandomState(100 + p)
    h, w = 97, 131
    b = np.stack([g.uniform(-5, w, p), g.uniform(-5, h, p), g.uniform(0, w + 5, p), g.uniform(0, h + 5, p)], 1).astype(np.float32)
    b[:, 2:] = np.maximum(b[:, 2:], b[:, :2])
    if p >= 3:
        b[0, 0], b[1, 2], b[2] = 0.0, float(w), (10.0, 3.0, 10.0, 40.0)          # flips onto exactly W / exactly 0; zero width
    views10 = [(h, w, False), (h, w, True), (64, 86, False), (64, 86, True), (200, 270, True), (33, 45, False), (97, 262, True), (194, 131, False),
               (120, 160, True), (1200, 1621, True)]          # a scale of exactly 1, non-integer scales, an integer scale
    props = torch.from_numpy(b).to(dev)
    pcap = p + 7
    count = torch.tensor([p], dtype=torch.int32, device=dev)
    for views in (views10[:1], views10[:2], views10):
        table = ops.tta_view_table(h, w, views).to(dev)
        out = ops.tta_boxes(props, count, table, pcap).cpu().numpy()
        assert out.shape == (len(views), pcap, 4)
        for i, (nh, nw, fl) in enumerate(views):
            want = tta_ref.view_boxes(b, h, w, nh, nw, fl)
            assert np.array_equal(bits(out[i, :p]), bits(want)), (p, i)
            assert (out[i, p:] == 0).all()
            if fl and p >= 3:          # x0 = 0 flips onto W; x1 = w flips onto exactly 0 where w * sx is exact (scale 1 and 2)
                assert out[i, 0, 2] == np.float32(nw) and (nw % w != 0 or out[i, 1, 0] == 0.0)
    # a count below P: the rows behind it are zeros as well
    if p >= 2:
        short = torch.tensor([p - 1], dtype=torch.int32, device=dev)
        out = ops.tta_boxes(props, short, ops.tta_view_table(h, w, views10[:2]).to(dev), pcap).cpu().numpy()
        assert (out[:, p - 1:] == 0).all() and np.array_equal(bits(out[1, :p - 1]), bits(tta_ref.view_boxes(b[:p - 1], h, w, h, w, True)))


# ---------------------------------------------------------------------------------------------------------------- unit_image_chw_to_u8
@pytest.mark.parametrize("hw", [(5, 7), (33, 65)])
def test_image_chw_to_u8(dev, hw):
    from unit_amd import ops
    g = np.random.RandomState(7)
    img = g.uniform(0, 255.999, (3,) + hw).astype(np.float32)
    img.reshape(-1)[:4] = (0.0, 0.5, 254.999, 255.0)
    got = ops.image_chw_to_u8(torch.from_numpy(img).to(dev)).cpu().numpy()
    want = img.transpose(1, 2, 0).astype(np.uint8)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    assert got.reshape(-1, 3)[:4, 0].tolist() == [0, 0, 254, 255]
    u8 = g.randint(0, 256, (3,) + hw).astype(np.uint8)
    assert np.array_equal(ops.image_chw_to_u8(torch.from_numpy(u8).to(dev)).cpu().numpy(), u8.transpose(1, 2, 0))


# ---------------------------------------------------------------------------------------------------------------- unit_tta_accumulate
@pytest.mark.parametrize("k", [20, 80])
@pytest.mark.parametrize("r", [1, 65, 300])
def test_tta_accumulate_bit_for_bit(dev, k, r):
    """probs_sum = the fp32 sum, in view order, of ops.softmax_rows outputs; delta_mean = the sequential fp32 sum divided by n (numpy on the
    host: a true division). Layouts: the dense [R, K+1] / [R, 4K] tensors the predictor's transfer returns, and one fused buffer with the deltas
    in columns 0..4K and the scores behind them (row stride and column offset). The two-views-per-launch form against the one-view form."""
    from unit_amd import ops
    g = torch.Generator().manual_seed(1000 + k + r)
    ld = ((5 * k + 1 + 7) // 8) * 8
    rcap = r + 3
    count = torch.tensor([r], dtype=torch.int32, device=dev)
    for n in (1, 2, 10):
        fused = [(torch.randn(rcap, ld, generator=g) * 3).to(dev) for _ in range(n)]
        probs = [ops.softmax_rows(f[:, 4 * k:4 * k + k + 1].contiguous(), k + 1).cpu().numpy() for f in fused]
        deltas = [f[:, :4 * k].cpu().numpy() for f in fused]
        ps, dsum = probs[0].copy(), deltas[0].copy()
        for v in range(1, n):
            ps, dsum = ps + probs[v], dsum + deltas[v]
        dmean = dsum / np.float32(n)
        assert ps.dtype == np.float32 and dmean.dtype == np.float32
        ps[r:], dmean[r:] = 0, 0
        results = []
        for layout in ("fused", "dense"):
            for pair in ((False, True) if n >= 2 else (False,)):
                out = [torch.full((rcap, c), float("nan"), device=dev) for c in (k + 1, 4 * k, 4 * k)]
                step = 2 if pair else 1
                for v in range(0, n, step):
                    if pair:          # two views in one buffer, the second `rcap` rows behind the first, as a twin batch's predictions lie
                        src = torch.cat([fused[v], fused[v + 1]], 0)
                    else:
                        src = fused[v]
                    if layout == "fused":
                        ops.tta_accumulate(src, src, k, rcap, v, n, *out, count=count, n_in=step, view_rows=rcap, scol0=4 * k)
                    else:
                        sc, de = src[:, 4 * k:4 * k + k + 1].contiguous(), src[:, :4 * k].contiguous()
                        ops.tta_accumulate(sc, de, k, rcap, v, n, *out, count=count, n_in=step, view_rows=rcap)
                got_ps, got_dm = out[0].cpu().numpy(), out[2].cpu().numpy()
                assert np.array_equal(bits(got_ps), bits(ps)), (k, r, n, layout, pair, np.abs(got_ps - ps).max())
                assert np.array_equal(bits(got_dm), bits(dmean)), (k, r, n, layout, pair, np.abs(got_dm - dmean).max())
                results.append((got_ps, got_dm))
        assert all(np.array_equal(bits(a), bits(results[0][0])) and np.array_equal(bits(b), bits(results[0][1])) for a, b in results)


def test_tta_accumulate_refuses_short_delta_rows(dev):
    from unit_amd import ops
    from unit_amd._lib import UnitLibError
    x = torch.zeros(4, 101 + 3, device=dev)
    out = [torch.zeros(4, c, device=dev) for c in (21, 80, 80)]
    with pytest.raises(UnitLibError, match="row strides"):          # 21 columns of deltas where 4K = 80 are read
        ops.tta_accumulate(x, x[:, :21].contiguous(), 20, 4, 0, 1, *out)


# ---------------------------------------------------------------------------------------------------------------- the views
def test_views_equal_pillow_and_the_reference_boxes(dev):
    """the resized uint8 views against Pillow's (stored: Pillow is an authoring-side tool), the unchanged size without a resampling pass,
    every view's boxes against the reference's bit for bit"""
    from unit_amd.modeling.inference import tta_predict
    model, image = model_of("tta")
    model._ensure_ready()
    with torch.no_grad():
        *_, views, plan = tta_predict(model, inputs_of("tta", image), want_views=True)
    assert [list(map(int, v)) for v in plan] == GOLD["tta/views"].tolist()
    u8 = image.permute(1, 2, 0).numpy().astype(np.uint8)
    for i, (r8, vb) in enumerate(views):
        want = GOLD[f"tta/view_image{2 * i}"]
        assert np.array_equal(r8.cpu().numpy(), want), i
        if want.shape[:2] == (H, W):
            assert np.array_equal(want, u8)
        for j in range(2):
            assert np.array_equal(bits(vb[j].cpu().numpy()), bits(GOLD[f"tta/view_boxes{2 * i + j}"])), (i, j)


# ---------------------------------------------------------------------------------------------------------------- model level
@pytest.mark.parametrize("name", RECORDED)
def test_tta_inference_vs_reference(dev, name):
    """classes exact, boxes at the eval bar (rtol 1e-4, atol 2e-2), scores rtol 1e-4 / atol n_views x 1e-5 (1e-5 per softmax, n_views terms);
    probs_sum at the same bar, delta_mean rtol 1e-4 / atol 1e-5. The worst errors are printed before the assertions (DESIGN.md quotes them)."""
    from unit_amd.modeling.inference import tta_predict
    model, image = model_of(name)
    n_views = len(GOLD[f"{name}/views"])
    inp = inputs_of(name, image)
    out = model.inference([inp])[0]["instances"]
    with torch.no_grad():
        probs_sum, delta_mean, *_ = tta_predict(model, inp)
    ps, dm = probs_sum.cpu().numpy(), delta_mean.cpu().numpy()
    e = dict(probs_sum=np.abs(ps - GOLD[f"{name}/probs_sum"]).max(), delta_mean=np.abs(dm - GOLD[f"{name}/delta_mean"]).max())
    got_c, got_s, got_b = out.pred_classes.cpu().numpy(), out.scores.cpu().numpy(), out.pred_boxes.tensor.cpu().numpy()
    if got_s.shape == GOLD[f"{name}/scores"].shape:
        e.update(scores=np.abs(got_s - GOLD[f"{name}/scores"]).max(), boxes=np.abs(got_b - GOLD[f"{name}/boxes"]).max())
    print(f"{name}: {len(got_s)} detections ({len(GOLD[f'{name}/scores'])} recorded), worst absolute errors", {k: float(v) for k, v in e.items()})
    assert np.allclose(ps, GOLD[f"{name}/probs_sum"], rtol=1e-4, atol=1e-5 * n_views)
    assert np.allclose(dm, GOLD[f"{name}/delta_mean"], rtol=1e-4, atol=1e-5)
    assert np.array_equal(got_c, GOLD[f"{name}/classes"])
    assert np.allclose(got_b, GOLD[f"{name}/boxes"], rtol=1e-4, atol=2e-2)
    assert np.allclose(got_s, GOLD[f"{name}/scores"], rtol=1e-4, atol=1e-5 * n_views)
    assert out.image_size == (2 * H, 2 * W) and not out.has("pred_masks")
    assert got_s.max() > 1.0 or n_views < 3          # (the sum is not renormalised)
    # do_postprocess=False: the instances before _postprocess, in the coordinates of the original proposals' image
    raw = model.inference([inp], do_postprocess=False)[0]
    assert raw.image_size == (H, W) and len(raw) >= len(out)
    # the twin batch against one pass per view: the same decisions
    from unit_amd.modeling.inference import inference_tta
    with torch.no_grad():
        single = inference_tta(model, [inp], twin_batch=False)[0]["instances"]
    assert np.array_equal(single.pred_classes.cpu().numpy(), got_c)
    assert np.allclose(single.scores.cpu().numpy(), got_s, rtol=1e-4, atol=1e-5 * n_views)


def test_tta_refused_on_mask_heads_as_the_reference_fails_there(dev):
    """the reference's own TTA stops at roi_heads.py:770 on its mask ROI heads (recorded in the fixture): refused here, before anything runs"""
    from unit_amd.modeling.inference import TTA_MASK_HEADS, UnsupportedConfig
    assert int(GOLD["tta_mask/reference_raises_at"]) == 770
    model, image = model_of("tta_mask")
    with pytest.raises(UnsupportedConfig) as e:
        model.inference([inputs_of("tta_mask", image)])
    assert str(e.value) == TTA_MASK_HEADS
    model.cfg.TEST.AUG.ENABLED = False          # the single-scale path of the same model is untouched: masks as ever
    out = model.inference([inputs_of("tta_mask", image)])[0]["instances"]
    assert out.has("pred_masks")


def test_refusals_at_the_call(dev):
    from unit_amd.modeling.inference import UnsupportedConfig
    model, image = model_of("tta")
    with pytest.raises(UnsupportedConfig, match="needs precomputed proposals"):
        model.inference([{"image": image, "height": H, "width": W}])
    with pytest.raises(NotImplementedError, match="detected_instances"):
        model.inference([inputs_of("tta", image)], detected_instances=[None])
    model.cfg.TEST.AUG.MIN_SIZES = ()
    with pytest.raises(UnsupportedConfig, match="empty TEST.AUG.MIN_SIZES"):
        model.inference([inputs_of("tta", image)])


def test_disabled_is_the_single_scale_path_bit_for_bit(dev):
    """ENABLED=False: `inference` gives what the eval branch gave before it was split into a predict and a detect half -- restated here
    launch for launch from the ops"""
    from unit_amd import ops
    from unit_amd.modeling import inference as I
    model, image = model_of("tta")
    model.cfg.TEST.AUG.ENABLED = False
    inp = inputs_of("tta", image)
    out = model.inference([inp], do_postprocess=False)[0]
    with torch.no_grad():
        rh, bp = model.roi_heads, model.roi_heads.box_predictor
        wh = bp.weak_detector_head
        x, sizes = ops.preprocess_images([image.to(dev).float()], model._pixel_mean, model._pixel_std, torch.float32, 8, model.normalize_images)
        feat, _ = model.backbone.fwd(x)
        props, pcount = I.pack_proposal_instances([inp["proposals"]], dev)
        hw = model._sizes_on_device(sizes)
        rois5, _ = ops.first_k_rois(props, pcount, props.shape[1], 0)
        pooled = rh.pool(feat, rois5)
        box_feat, _ = rh.box_head.fwd(pooled)
        sup_weak = rh.weak_box_head.fwd(pooled)[0]
        lin_sup, lin_w_box, lin_w_sup = bp.group.fwd(box_feat), wh.group.fwd(box_feat), wh.group.fwd(sup_weak)
        sims = I.similarity_dict(rh, lin_w_box)
        scores, bbox = bp.transfer(lin_sup, lin_w_sup, sims["cls"], sims["bbox"], I.class_roles(rh), ft=None)
        probs = ops.softmax_rows(scores, rh.num_classes + 1)
        boxes, sc, cls, roi, cnt = ops.detections(probs, bbox, props, pcount, hw, bp.bbox_reg_weights, bp.test_score_thresh, bp.test_nms_thresh,
                                                  bp.test_topk_per_image)
        same = I.roi_heads_inference(rh, feat, props, pcount, hw, torch.float32)
    n = int(cnt[0])
    assert n == len(out) and n > 3
    assert torch.equal(out.pred_boxes.tensor, boxes[0, :n]) and torch.equal(out.scores, sc[0, :n]) and torch.equal(out.pred_classes, cls[0, :n].long())
    for a, b in zip(same[:5], (boxes, sc, cls, roi, cnt)):
        assert torch.equal(a, b)


def test_tta_call_launches_no_aten_kernel(dev):
    """the check of tools/stock_ops.py on a steady-state TTA call with device-resident inputs: every ATen operator dispatched is a view or an
    allocation, but for the one read of the kept counts at the API boundary"""
    from torch.utils._python_dispatch import TorchDispatchMode
    # pure metadata / allocation, no kernel behind them: the list of tools/stock_ops.py
    meta = {"empty", "empty_like", "empty_strided", "new_empty", "new_empty_strided", "view", "slice", "select", "as_strided", "reshape", "detach",
            "alias", "transpose", "permute", "unsqueeze", "squeeze", "expand", "record_stream", "_unsafe_view", "t", "unbind", "split",
            "split_with_sizes", "narrow", "_local_scalar_dense", "is_pinned", "unfold", "lift_fresh", "_reshape_alias", "resize_", "set_",
            "stride", "size", "sym_size", "numel", "is_same_size", "view_as", "chunk", "diagonal"}
    model, image = model_of("tta")
    inp = inputs_of("tta", image, device=dev)
    model.inference([inp])
    calls, host_reads = [], []

    class Log(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            res = func(*args, **(kwargs or {}))
            parts = str(func).split(".")
            if (parts[1] if len(parts) >= 2 else parts[0]) not in meta:
                if str(func) == "aten._to_copy.default" and res.device.type == "cpu":
                    host_reads.append(args[0].numel())          # a device-to-host read, no kernel: build_instances' kept counts
                else:
                    calls.append(str(func))
            return res
    with Log():
        out = model.inference([inp])
    assert len(out[0]["instances"]) > 3
    assert calls == [], calls
    assert host_reads == [1], host_reads          # the call's one sync: one int per image, read once


def test_tta_bf16_runs(dev):
    """bf16 compute mode: asserted only that it runs and returns finite scores; the agreement with the fp32 fixture is reported"""
    model, image = model_of("tta")
    model.compute_dtype = torch.bfloat16
    try:
        out = model.inference([inputs_of("tta", image)])[0]["instances"]
    finally:
        model.compute_dtype = torch.float32
    assert len(out) > 0 and bool(torch.isfinite(out.scores).all()) and bool(torch.isfinite(out.pred_boxes.tensor).all())
    want = GOLD["tta/classes"]
    got = out.pred_classes.cpu().numpy()
    n = min(len(want), len(got))
    print(f"bf16: {len(got)} detections ({len(want)} in the fp32 fixture); the same class at {int((got[:n] == want[:n]).sum())} of the first {n} ranks; "
          f"class histogram distance {int(np.abs(np.bincount(got, minlength=20) - np.bincount(want, minlength=20)).sum())}")
