"""Device time of unit_pcl_targets (csrc/pcl.hip) at the step's weak-loss shape: 2 weak images x 512 RoIs, K = 20, three refinement streams
(logits in, one launch), for peaked (head weights x 0.5) and near-uniform (x 0.05, as early in training) scores; beside it the OICR window
it replaces (3 x unit_oicr_targets + 3 x unit_softmax_ce) and unit_pcl_loss, measured in the same run. HIP events around every launch,
median of 50 after warm-up; one JSON line per measurement. With `step` as argument: the whole training step (R101, 600 x 1000, 2 + 2
images, bf16) with TYPE "OICR" and TYPE "PCL" of the same build, median of 20 steps.
For kernel-only times run it under `rocprofv3 --kernel-trace --stats -- python tools/pcl_targets_time.py`."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from unit_amd import ops  # noqa: E402

CENTERS = torch.tensor([[100.0, 90.0, 120.0, 100.0], [280.0, 180.0, 150.0, 140.0], [200.0, 120.0, 60.0, 200.0]])


def inputs(b, s, k, scale, classes, dev, seed=0, d=32):
    """a random weak head (weights x scale) on random features, boxes scattered around three centres (every IoU band occurs)"""
    g = torch.Generator().manual_seed(seed)
    n = b * s
    ld = (2 * k + 3 * (k + 1) + 7) // 8 * 8
    lin = torch.zeros(n, ld)
    lin[:, :2 * k + 3 * (k + 1)] = torch.randn(n, d, generator=g) @ (torch.randn(d, 2 * k + 3 * (k + 1), generator=g) * scale)
    c = CENTERS[torch.randint(0, 3, (n,), generator=g)]
    jit = (torch.rand(n, 4, generator=g) - 0.5) * torch.tensor([30.0, 30.0, 60.0, 60.0])
    cx, cy, bw, bh = c[:, 0] + jit[:, 0], c[:, 1] + jit[:, 1], (c[:, 2] + jit[:, 2]).clamp(min=8), (c[:, 3] + jit[:, 3]).clamp(min=8)
    rois5 = torch.stack([torch.arange(n) // s, (cx - bw / 2).clamp(0, 400), (cy - bh / 2).clamp(0, 300), (cx + bw / 2).clamp(0, 400),
                         (cy + bh / 2).clamp(0, 300)], 1).float()
    multihot = torch.zeros(b, k, dtype=torch.uint8)
    for i, cl in enumerate(classes):
        multihot[i, cl] = 1
    return dict(lin=lin.to(dev), rois5=rois5.to(dev), valid=torch.zeros(n, dtype=torch.int32, device=dev), multihot=multihot.to(dev)), ld


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
    b, s, k = 2, 512, 20
    for name, scale in (("peaked", 0.5), ("near_uniform", 0.05)):
        a, ld = inputs(b, s, k, scale, [[3, 7, 12], [0, 15]], dev)
        lin, c0 = a["lin"], 2 * k
        dy = torch.zeros((b * s, ld), dtype=torch.bfloat16, device=dev)
        _, xr = ops.wsddn_mil(lin, 0, k, k, a["valid"], s, b, a["multihot"], 1.0, 2.0, 4.0)
        kw = dict(k=k, rois5=a["rois5"], valid=a["valid"], s=s, b=b, multihot=a["multihot"], ldc=5 * k)
        step = k + 1
        three = lambda: ops.pcl_targets(lin, c0, 1, lin, c0, 1, n_streams=3, step=step, nstep=step, **kw)          # three logits streams: the step's shape of work
        first = lambda: ops.pcl_targets(xr, 0, 0, lin, c0, 1, **kw)
        later = lambda: ops.pcl_targets(lin, c0, 1, lin, c0 + step, 1, n_streams=2, step=step, nstep=step, **kw)
        t = ops.pcl_targets(lin, c0, 1, lin, c0, 1, **kw)

        def loss():
            ops.pcl_loss(lin, c0, k, a["valid"], s, b, t["labels"][0], t["cls_weights"][0], t["gt_assign"][0], t["pc_count"][0],
                         t["pc_img_cls_weights"][0], t["pc_probs"][0], t["n_pc"][0], dy=dy, dcol0=c0)

        def oicr_window():
            for it in range(3):
                if it == 0:
                    lab, w = ops.oicr_targets(xr, 0, 0, k, a["rois5"], a["valid"], s, b, a["multihot"])
                else:
                    lab, w = ops.oicr_targets(lin, c0 + (it - 1) * step, 1, k, a["rois5"], a["valid"], s, b, a["multihot"])
                ops.softmax_ce(lin, c0 + it * step, k + 1, lab, weights=w, dy=dy, dcol0=c0 + it * step)
        for what, fn in (("pcl_targets_3_streams", three), ("pcl_targets_iteration_0", first), ("pcl_targets_iterations_1_2", later),
                         ("pcl_loss", loss), ("oicr_window_3x_targets_3x_softmax_ce", oicr_window)):
            med, lo = median_us(fn)
            print(json.dumps({"scores": name, "what": what, "K": k, "images": b, "rows_per_image": s, "median_us": med, "min_us": lo,
                              "clusters": t["n_pc"][0].tolist()}), flush=True)


def steps():
    from unit_amd import config
    from unit_amd.modeling import build_model
    from unit_amd.solver import FlatSGD
    from unit_amd.synthetic import init_synthetic_weights, synthetic_batch
    for typ in ("OICR", "PCL"):
        cfg = config.voc_rcnn_c4_split1(101)
        cfg.MODEL.DEVICE = "cuda:0"
        cfg.MODEL.ROI_HEADS.FAST_RCNN.WEAK_DETECTOR.TYPE = typ
        cfg.SEED = 0
        model = build_model(cfg)
        init_synthetic_weights(model, seed=1)
        model.train()
        model.compute_mode = "bf16"
        batch = model.pack_batch(*synthetic_batch(2, 2, seed=100))
        opt = FlatSGD(model, cfg)

        def step():
            st = model.forward_train(batch, early_backward=True)
            model.backward_train(st)
            opt.step()
        med, lo = median_us(step, n=20, warm=5)
        print(json.dumps({"what": "training_step", "TYPE": typ, "median_ms": round(med / 1000, 3), "min_ms": round(lo / 1000, 3)}), flush=True)
        del model, opt, batch
        torch.cuda.empty_cache()


if __name__ == "__main__":
    steps() if "step" in sys.argv[1:] else kernels()
