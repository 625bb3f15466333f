"""Test-time augmentation: what does one TTA `inference` call cost, and against what?      python tools/tta_time.py [--reps N] [--out FILE]
R101, K = 20, bf16, one 600 x 1000 image with 1000 seeded proposals, the reference's TEST.AUG (MIN_SIZES 480..1200, MAX_SIZE 2000, FLIP).
Every view shape is warmed first; then, ALTERNATING in the same run:
  (a)  one TTA `inference` call (the twin batch: one backbone + ROI-heads pass of N = 2 per size)
  (a1) the same with one pass of N = 1 per view
  (b)  what a user did before: ten single-scale forward passes on host-prepared views, as `inference` ran them (upload, preprocess, backbone,
       the RPN head whose output is thrown away, ROI heads, softmax, a sync per call) plus the combination with torch operators and one
       detection pass. The host resize itself is NOT in the timed region (it is done once, before; Pillow where importable, else torch's
       bilinear -- the pixels differ, the shapes and the work do not), which flatters (b).
Host clock around each call; every call ends in a sync (build_instances reads the kept counts).
  python tools/tta_time.py --trace-summary <kernel_trace.csv>    sums a `rocprofv3 --kernel-trace` CSV of `--reps 1 --only a` per size."""
import argparse
import csv
import json
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")


def trace_summary(path):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    starts = [i for i, r in enumerate(rows) if "image_chw_to_u8_kernel" in r["Kernel_Name"]]
    call = rows[starts[-1]:]          # the last TTA call
    marks = [i for i, r in enumerate(call) if "preprocess_u8_kernel" in r["Kernel_Name"]]
    groups = [marks[i] for i in range(len(marks)) if i == 0 or marks[i] != marks[i - 1] + 1]          # (two launches per size under FLIP)
    bounds = groups + [next(i for i, r in enumerate(call) if "det_select_kernel" in r["Kernel_Name"])]
    dur = lambda rs: sum(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rs) / 1e6
    print(f"last TTA call: {len(call)} kernels, busy {dur(call):.3f} ms")
    for g, (a, b) in enumerate(zip(bounds[:-1], bounds[1:])):
        grid = next(r for r in call[a:b] if "preprocess_u8_kernel" in r["Kernel_Name"])
        print(f"  size {g}: {b - a:4d} kernels, busy {dur(call[a:b]):8.3f} ms (both views of the size; preprocess grid {grid['Grid_Size_X']})")
    print(f"  combine + detect + output: {len(call) - bounds[-1]} kernels, busy {dur(call[bounds[-1]:]):.3f} ms")
    for name in ("tta_boxes_kernel", "tta_accumulate_kernel", "image_chw_to_u8_kernel"):
        rs = [r for r in call if name in r["Kernel_Name"]]
        print(f"  {name}: x{len(rs)}, {dur(rs) * 1e3:.1f} us in all")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("--trace-summary", default="")
    a = ap.parse_args()
    if a.trace_summary:
        return trace_summary(a.trace_summary)
    from unit_amd import config, ops
    from unit_amd.modeling import build_model
    from unit_amd.modeling import inference as I
    from unit_amd.structures import Boxes, Instances
    from unit_amd.synthetic import init_synthetic_weights, synthetic_batch
    cfg = config.voc_rcnn_c4_split1(101)
    cfg.MODEL.DEVICE = "cuda:0"
    cfg.TEST.AUG.ENABLED = True
    model = build_model(cfg)
    init_synthetic_weights(model, seed=1)
    with torch.no_grad():
        w = model.roi_heads.box_predictor.cls_score_delta.weight
        w.copy_(torch.randn(w.shape, generator=torch.Generator().manual_seed(40)) * 0.02)
    model.eval()
    model.compute_mode = "bf16"
    dev = model.device
    H, W, P, K = 600, 1000, 1000, 20
    sup, _ = synthetic_batch(1, 0, hw=(H, W), seed=7)
    image = sup[0]["image"]
    g = np.random.RandomState(3)
    cx, cy, bw, bh = g.uniform(0, W, P), g.uniform(0, H, P), g.uniform(16, 500, P), g.uniform(16, 400, P)
    boxes = np.stack([(cx - bw / 2).clip(0, W), (cy - bh / 2).clip(0, H), (cx + bw / 2).clip(0, W), (cy + bh / 2).clip(0, H)], 1).astype(np.float32)
    inp = {"image": image.to(dev), "height": H, "width": W, "proposals": Instances((H, W), proposal_boxes=Boxes(torch.from_numpy(boxes).to(dev)))}
    plan = I.tta_view_plan(H, W, cfg.TEST.AUG)
    lines = [f"tta_time: R101 K={K} bf16, image {H}x{W}, {P} proposals, views {[(h, w, int(f)) for h, w, f in plan]}"]

    # ---- (b): host-prepared views (outside the timed region)
    u8 = image.permute(1, 2, 0).numpy().astype(np.uint8)
    try:
        from PIL import Image
        resize = lambda nh, nw: np.asarray(Image.fromarray(u8).resize((nw, nh), Image.BILINEAR)) if (nh, nw) != (H, W) else u8
        lines.append("host views: Pillow")
    except ImportError:
        f32 = torch.from_numpy(u8).permute(2, 0, 1)[None].float()
        resize = lambda nh, nw: torch.nn.functional.interpolate(f32, size=(nh, nw), mode="bilinear", align_corners=False)[0].permute(1, 2, 0).byte().numpy()
        lines.append("host views: torch bilinear (Pillow not importable here; pixels differ, shapes and work do not)")
    host_views = []
    for nh, nw, fl in plan:
        v = resize(nh, nw)
        v = np.flip(v, axis=1) if fl else v
        b = boxes.copy()
        b[:, 0::2] *= np.float32(nw * 1.0 / W)
        b[:, 1::2] *= np.float32(nh * 1.0 / H)
        b = b.clip(min=0)
        if fl:
            b[:, 0], b[:, 2] = (np.float32(nw) - b[:, 2]).clip(min=0), (np.float32(nw) - b[:, 0]).clip(min=0)
        host_views.append((torch.from_numpy(np.ascontiguousarray(v)).permute(2, 0, 1).float().contiguous(),
                           Instances((nh, nw), proposal_boxes=Boxes(torch.from_numpy(b)))))
    rh, rpn, dt = model.roi_heads, model.proposal_generator, model.compute_dtype
    props0, pcount0 = I.pack_proposal_instances([inp["proposals"]], dev)
    hw0 = model._sizes_on_device([(H, W)])

    @torch.no_grad()
    def run_b():
        probs, deltas = [], []
        for img, pr in host_views:          # one single-scale call per view, as modeling/inference.py ran it, up to the class probabilities
            x, sizes = ops.preprocess_images([img.to(dev)], model._pixel_mean, model._pixel_std, dt, 8, model.normalize_images)
            feat, _ = model.backbone.fwd(x)
            rpn.rpn_head.fwd(feat)          # (executed in every call although its output is thrown away)
            props, pcount = I.pack_proposal_instances([pr], dev)
            scores, bbox, _ = I.roi_heads_predict(rh, feat, props, pcount)
            probs.append(ops.softmax_rows(scores, K + 1))
            deltas.append(bbox)
            torch.cuda.synchronize()          # the API boundary of each call
        ps, dm = torch.stack(probs).sum(0), torch.stack(deltas).mean(0)
        out = I.roi_heads_detect(rh, None, ps, dm, props0, pcount0, hw0, None, with_mask=False, cand_cap=P * K)
        return I.build_instances(*out[:5], None, [(H, W)], [(H, W)], consts=model._const_on_device)

    run_a = lambda: I.inference_tta(model, [inp], twin_batch=True)
    run_a1 = lambda: I.inference_tta(model, [inp], twin_batch=False)
    runs = {"a": run_a, "a1": run_a1, "b": run_b}
    if a.only:
        runs = {k: v for k, v in runs.items() if k in a.only.split(",")}
    model._ensure_ready()
    with torch.no_grad():
        res = {}
        for k, fn in runs.items():          # warm every view shape, in every form
            for _ in range(2):
                res[k] = fn()
        torch.cuda.synchronize()
        t = {k: [] for k in runs}
        for _ in range(a.reps):
            for k, fn in runs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                t[k].append((time.perf_counter() - t0) * 1e3)
    n = {k: len(v[0]["instances"]) for k, v in res.items()}
    lines.append(f"detections per form: {n}")
    if "a" in res and "b" in res:
        sa, sb = res["a"][0]["instances"].scores.cpu(), res["b"][0]["instances"].scores.cpu()
        m = min(len(sa), len(sb))
        lines.append(f"(a) vs (b) top scores (different resize on this host unless Pillow): max |diff| over the first {m} = {float((sa[:m] - sb[:m]).abs().max()):.4f}")
    for k, v in t.items():
        lines.append(f"({k}) ms per call, {a.reps} alternating repeats: median {statistics.median(v):9.2f}  min {min(v):9.2f}  max {max(v):9.2f}   all {[round(x, 2) for x in v]}")
    lines.append(json.dumps({"tta_time": {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in t.items()},
                             "reps": a.reps, "views": len(plan), "proposals": P}))
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
