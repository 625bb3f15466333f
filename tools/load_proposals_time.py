"""What MODEL.LOAD_PROPOSALS costs (profiles/r16_load_proposals.txt holds a run):
  kernels (default): unit_oicr_targets_wide at 2 images x 2000 rows (Detectron2's POST_NMS_TOPK_TRAIN / PRECOMPUTED_PROPOSAL_TOPK_TRAIN default)
    for K = 20 with 3 labels an image and K = 80 with 8, logits in (mode 1, the softmax in the kernel) and probabilities in (mode 0), with and
    without the matched boxes; beside it, for scale, the narrow unit_oicr_targets at its largest shape, 2 x 1024 rows, on the same kind of
    input, and the wide kernel on that shape too. HIP events around every launch, median of 50 after warm-up; one JSON line per measurement.
  `step`: the eager S1 training step at the benchmark's shapes (R101, 600 x 1000, 2 + 2 images, bf16) with the switch off and on -- on: every
    one of the RPN's 2000 proposal slots of a weak image is a weak RoI instead of the first 512 -- median of 20 steps.
The default benchmark line itself is `python bench.py --gpus 1 --steps K --warmup W` of this commit beside the parent's."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from unit_amd import ops  # noqa: E402


def inputs(b, s, k, labels, dev, seed=0, d=32):
    """random logits of a random linear head on random features ([b * s, k + 1] at a row stride that is a multiple of 8), boxes scattered
    around three centres, `labels` classes per image"""
    g = torch.Generator().manual_seed(seed)
    n = b * s
    ld = (k + 1 + 7) // 8 * 8
    lin = torch.zeros(n, ld)
    lin[:, :k + 1] = torch.randn(n, d, generator=g) @ (torch.randn(d, k + 1, generator=g) * 0.5)
    centers = torch.tensor([[100.0, 90.0, 120.0, 100.0], [280.0, 180.0, 150.0, 140.0], [200.0, 120.0, 60.0, 200.0]])
    c = centers[torch.randint(0, 3, (n,), generator=g)]
    jit = (torch.rand(n, 4, generator=g) - 0.5) * torch.tensor([30.0, 30.0, 60.0, 60.0])
    cx, cy, bw, bh = c[:, 0] + jit[:, 0], c[:, 1] + jit[:, 1], (c[:, 2] + jit[:, 2]).clamp(min=8), (c[:, 3] + jit[:, 3]).clamp(min=8)
    rois5 = torch.stack([torch.arange(n) // s, (cx - bw / 2).clamp(0, 400), (cy - bh / 2).clamp(0, 300), (cx + bw / 2).clamp(0, 400),
                         (cy + bh / 2).clamp(0, 300)], 1).float()
    multihot = torch.zeros(b, k, dtype=torch.uint8)
    for i in range(b):
        multihot[i, torch.randperm(k, generator=g)[:labels]] = 1
    probs = torch.softmax(lin[:, :k + 1], -1)[:, :k].contiguous()
    return dict(lin=lin.to(dev), probs=probs.to(dev), rois5=rois5.to(dev), valid=torch.zeros(n, dtype=torch.int32, device=dev),
                multihot=multihot.to(dev))


def median_us(fn, n=50, warm=10):
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
        ts.append(t0.elapsed_time(t1) * 1000)
    return round(statistics.median(ts), 1), round(min(ts), 1)


def kernels():
    dev = torch.device("cuda:0")
    b = 2
    for k, labels in ((20, 3), (80, 8)):
        for s, forms in ((2000, (True,)), (1024, (False, True))):
            a = inputs(b, s, k, labels, dev)
            for wide in forms:
                for mode, src in ((1, a["lin"]), (0, a["probs"])):
                    for boxes in (False, True):
                        fn = lambda: ops.oicr_targets(src, 0, mode, k, a["rois5"], a["valid"], s, b, a["multihot"], want_boxes=boxes, wide=wide)
                        med, lo = median_us(fn)
                        print(json.dumps({"what": "unit_oicr_targets_wide" if wide else ("unit_oicr_targets_ex" if boxes else "unit_oicr_targets"),
                                          "K": k, "labels_per_image": labels, "images": b, "rows_per_image": s, "mode": mode, "boxes": boxes,
                                          "median_us": med, "min_us": lo}), flush=True)


def steps():
    from unit_amd import config
    from unit_amd.modeling import build_model
    from unit_amd.solver import FlatSGD
    from unit_amd.synthetic import init_synthetic_weights, synthetic_batch
    for load in (False, True):
        cfg = config.voc_rcnn_c4_split1(101)
        cfg.MODEL.DEVICE = "cuda:0"
        cfg.MODEL.LOAD_PROPOSALS = load
        cfg.SEED = 0
        model = build_model(cfg)
        init_synthetic_weights(model, seed=1)
        model.train()
        model.compute_mode = "bf16"
        batch = model.pack_batch(*synthetic_batch(2, 2, seed=100))
        opt = FlatSGD(model, cfg)
        rows = []

        def step():
            st = model.forward_train(batch, early_backward=True)
            model.backward_train(st)
            opt.step()
            rows[:] = [st.sw, st.rw]
        med, lo = median_us(step, n=20, warm=5)
        print(json.dumps({"what": "training_step", "LOAD_PROPOSALS": load, "weak_rows_per_image": rows[0], "weak_rois": rows[1],
                          "median_ms": round(med / 1000, 3), "min_ms": round(lo / 1000, 3)}), flush=True)
        del model, opt, batch
        torch.cuda.empty_cache()


if __name__ == "__main__":
    steps() if "step" in sys.argv[1:] else kernels()
