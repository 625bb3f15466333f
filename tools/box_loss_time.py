"""Per-launch time of the two box-regression loss kernels under each loss type, in the bench step (R101 S1, 2 + 2 images of 600 x 1000, bf16).

    python tools/box_loss_time.py [steps=10]

For each of (smooth_l1, beta 0) -- the plain exports --, (smooth_l1, beta 1/9) and (giou, 0) on both heads: one model, a warm-up step, then
`steps` eager single-stream steps under ops.PROFILER, whose `_timed("rpn_loss")` / `_timed("box_reg_loss")` brackets put a HIP-event pair
around each launch (the pair includes the kernel's memsets and the ~5 us a launch costs on an empty stream). Prints the median and the
min - max per launch in microseconds. No bar: a measurement for DESIGN.md section 8."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from unit_amd import config, ops  # noqa: E402
from unit_amd.modeling import build_model  # noqa: E402
from unit_amd.synthetic import init_synthetic_weights, synthetic_batch  # noqa: E402


def measure(loss_type, beta, steps):
    cfg = config.voc_rcnn_c4_split1(101)
    cfg.MODEL.DEVICE = "cuda:0"
    for node in (cfg.MODEL.RPN, cfg.MODEL.ROI_BOX_HEAD):
        node.BBOX_REG_LOSS_TYPE, node.SMOOTH_L1_BETA = loss_type, beta
    cfg.SEED = 0
    model = build_model(cfg)
    init_synthetic_weights(model, seed=1)
    model.train()
    model.compute_mode = "bf16"
    model.overlap_streams = False
    batch = model.pack_batch(*synthetic_batch(2, 2, seed=100))

    def step():
        model.backward_train(model.forward_train(batch, early_backward=True))
    step()
    torch.cuda.synchronize()
    prof = ops.PROFILER = {}
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    ops.PROFILER = None
    out = {}
    for name in ("rpn_loss", "box_reg_loss"):
        us = [e[0].elapsed_time(e[1]) * 1e3 for e in prof[name]]
        out[name] = (statistics.median(us), min(us), max(us), len(us))
    return out


if __name__ == "__main__":
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    for loss_type, beta in (("smooth_l1", 0.0), ("smooth_l1", 1.0 / 9), ("giou", 0.0)):
        for name, (med, lo, hi, n) in measure(loss_type, beta, steps).items():
            print(f"{loss_type:9s} beta {beta:.3f}  {name:12s} median {med:7.2f} us  [{lo:.2f} - {hi:.2f}]  {n} launches")
