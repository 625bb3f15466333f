"""Cost of the training-metrics kernels (csrc/metrics.hip; DESIGN.md section 8 "Training metrics on the device").

  python tools/metrics_time.py kernels
      the three kernels and their neighbours in the step on the same inputs, at the BASELINE shapes -- VOC S1: 1024 RoIs x 21 classes, the
      sampled anchor labels of two 600x1000 images; COCO + mask head: 1024 RoIs x 81 classes, 256 foreground slots x 14x14 x 80 classes.
      Prints HIP-event means per launch; for kernel-only durations run it under
      `rocprofv3 --kernel-trace --stats -d <dir> -o metrics --output-format csv -- python tools/metrics_time.py kernels` and read
      <dir>/metrics_kernel_stats.csv (metrics_*_kernel against softmax_ce_kernel / mask_loss_kernel).
  python tools/metrics_time.py step [pairs] [steps]
      the bench workload's step (R101 S1, 2 + 2 images of 600x1000, bf16, call-list replay) with the switch off and on, alternated in one
      process after warm-up: one JSON line with every block's ms per step, both medians and the spread of the off blocks.
"""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from unit_amd import ops  # noqa: E402


def _timed(fn, n=200, warm=20):
    for _ in range(warm):
        fn()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(n):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return round(t0.elapsed_time(t1) * 1000 / n, 2)


def kernels():
    from unit_amd._lib import check, lib
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    m = torch.zeros(16, dtype=torch.int32, device=dev)
    out = {}
    for k in (20, 80):
        r, ncls = 1024, k + 1
        scores = (torch.randn(r, ncls, generator=g) * 2).to(dev)
        cls = torch.where(torch.rand(r, generator=g) < 0.75, torch.full((r,), k), torch.randint(0, k, (r,), generator=g)).int().to(dev)
        dy = torch.zeros((r, 128), dtype=torch.bfloat16, device=dev)
        out[f"softmax_ce K={k} us"] = _timed(lambda: ops.softmax_ce(scores, 0, ncls, cls, dy=dy, dcol0=0))
        out[f"metrics_fastrcnn K={k} us"] = _timed(lambda: ops.metrics_fastrcnn(scores, 0, ncls, cls, m[5:10]))
    labels = torch.full((2, 38 * 63 * 15), -1, dtype=torch.int8)          # after sampling: 256 labelled anchors per image, the rest ignored
    for i in range(2):
        idx = torch.randperm(labels.shape[1], generator=g)[:256]
        labels[i, idx[:24]], labels[i, idx[24:]] = 1, 0
    labels = labels.to(dev)
    out["metrics_rpn 2 x 35910 anchors us"] = _timed(lambda: ops.metrics_rpn(labels, m[0:5]))
    s, msz, k, ldk = 256, 14, 80, 80          # 2 images x 128 foreground slots, 14 x 14 mask logits
    lg = torch.randn(s * msz * msz, ldk, generator=g).to(dev)
    tg = (torch.rand(s, msz, msz, generator=g) < 0.4).to(torch.uint8).to(dev)
    mc = torch.randint(0, k, (s,), generator=g).int().to(dev)
    loss = torch.zeros(1, device=dev)
    dlg = torch.empty((s * msz * msz, ldk), dtype=torch.bfloat16, device=dev)
    out[f"mask_bce_loss {s} slots {msz}x{msz} K={k} us"] = _timed(lambda: check(lib().unit_mask_bce_loss(
        ops._p(lg), k, ldk, ops._p(mc), ops._p(tg), s, msz, 1.0, ops._p(loss), ops._p(dlg), ops.dt(torch.bfloat16), ops._s()), "mask_bce_loss"), n=100)
    out[f"metrics_mask {s} slots {msz}x{msz} K={k} us"] = _timed(lambda: ops.metrics_mask(lg, k, ldk, mc, tg, m[10:15]), n=100)
    print(json.dumps(out))


def step(pairs=4, steps=30):
    from unit_amd import config
    from unit_amd.engine import ReplayedStep
    from unit_amd.modeling import build_model
    from unit_amd.solver import FlatSGD
    from unit_amd.synthetic import init_synthetic_weights, synthetic_batch
    cfg = config.voc_rcnn_c4_split1(101)
    cfg.MODEL.DEVICE = "cuda:0"
    cfg.SEED = 0
    model = build_model(cfg)
    init_synthetic_weights(model, seed=1)
    model.train()
    model.compute_mode = "bf16"
    sup, weak = synthetic_batch(2, 2, seed=100)
    batch = model.pack_batch(sup, weak)
    opt = FlatSGD(model, cfg)
    runs = {}
    for on in (False, True):          # one recorded call list per setting (the switch is read while the step is recorded), one model
        model.collect_metrics = on
        rs = ReplayedStep(model, opt, warmup_steps=2)
        for _ in range(6):
            rs.run(packed=batch)
        assert rs.stats["replayed"] >= 3
        runs[on] = rs
    torch.cuda.synchronize()
    blocks = {False: [], True: []}
    for _ in range(pairs):
        for on in (False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                runs[on].run(packed=batch)
            torch.cuda.synchronize()
            blocks[on].append(round((time.perf_counter() - t0) / steps * 1e3, 4))
    off, on = blocks[False], blocks[True]
    calls = {str(k): next(iter(v.plans.values()))[0].n_calls for k, v in runs.items()}
    print(json.dumps({"ms_per_step_off": off, "ms_per_step_on": on, "median_off": statistics.median(off), "median_on": statistics.median(on),
                      "spread_off": round(max(off) - min(off), 4), "on_minus_off": round(statistics.median(on) - statistics.median(off), 4),
                      "steps_per_block": steps, "recorded_calls": calls, "last_metrics": model.last_metrics.cpu().tolist()}))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "step":
        step(*[int(a) for a in sys.argv[2:4]])
    else:
        kernels()
