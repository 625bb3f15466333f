"""What the similarity terms beyond 'lingual' + 'visual' cost in the eval path: inference.roi_heads_inference (RoIAlign, Res5 head, predictors,
similarity matrices, base -> novel transfer, detections) on the 1000 proposals of one 600 x 1000 image (R101, bf16), with the default terms
(['lingual', 'visual'] on every head: unit_similarity), with ['lingual', 'VisualK-5'] and with ['WTopK-5'] (unit_similarity_static +
unit_similarity_ex), same model, same process, in the order A B A C A. HIP events around every call, median of 20 after 5 warm-ups; one JSON
line per configuration.
  python tools/similarity_terms_time.py"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def median_ms(fn, n=20, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        ts.append(t0.elapsed_time(t1))
    return round(statistics.median(ts), 3), round(min(ts), 3)


def main():
    from unit_amd import config, ops
    from unit_amd.modeling import build_model
    from unit_amd.modeling.inference import roi_heads_inference
    from unit_amd.synthetic import init_synthetic_weights, synthetic_batch
    cfg = config.voc_rcnn_c4_split1(101)
    cfg.MODEL.DEVICE = "cuda:0"
    model = build_model(cfg)
    init_synthetic_weights(model, seed=1)
    model.eval()
    model.compute_mode = "bf16"
    model._ensure_ready()
    rh, dt = model.roi_heads, model.compute_dtype
    default = {h: list(t) for h, t in rh.terms.items()}
    sup, _ = synthetic_batch(1, 0, seed=100)
    with torch.no_grad():
        x, sizes = ops.preprocess_images([sup[0]["image"].to(model.device).float()], model._pixel_mean, model._pixel_std, dt, 8, model.normalize_images)
        feat, _ = model.backbone.fwd(x)
        hw = model._sizes_on_device(sizes)
        # 1000 proposals, as a trained RPN hands over (POST_NMS_TOPK_TEST; with synthetic weights NMS leaves fewer): random boxes in the image
        n_props = 1000
        g = torch.Generator().manual_seed(0)
        h, w = sizes[0]
        x0, y0 = torch.rand(n_props, generator=g) * (w - 64), torch.rand(n_props, generator=g) * (h - 64)
        bw, bh = 16 + torch.rand(n_props, generator=g) * 300, 16 + torch.rand(n_props, generator=g) * 300
        boxes = torch.stack([x0, y0, (x0 + bw).clamp(max=w), (y0 + bh).clamp(max=h)], 1)
        props = boxes[None].contiguous().to(model.device)
        pcount = torch.tensor([n_props], dtype=torch.int32).to(model.device)
        for name, terms in (("default", None), ("lingual+VisualK-5", ["lingual", "VisualK-5"]), ("default", None), ("WTopK-5", ["WTopK-5"]),
                            ("default", None)):
            rh.terms = default if terms is None else {h: list(terms) for h in default}
            med, lo = median_ms(lambda: roi_heads_inference(rh, feat, props, pcount, hw, dt))
            print(json.dumps({"what": "roi_heads_inference", "image": list(sizes[0]), "proposals": n_props, "terms": rh.terms["cls"], "name": name,
                              "median_ms": med, "min_ms": lo}), flush=True)


if __name__ == "__main__":
    main()
