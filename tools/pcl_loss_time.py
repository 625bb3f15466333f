"""Device time of unit_pcl_loss (csrc/pcl.hip) at the step's weak-loss shape: B weak images x S RoIs, K classes, up to 5 clusters per
gt class, fp32 logits in the fused Linear layout, bf16 dy. Prints one JSON line per (K, S) with the mean time per launch from HIP events.
For kernel-only times run it under `rocprofv3 --kernel-trace --stats -- python tools/pcl_loss_time.py`."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from unit_amd import ops  # noqa: E402


def inputs(b, s, k, ncls, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    ldc = 5 * ncls
    ld = (2 * k + 3 * (k + 1) + 7) // 8 * 8
    logits = torch.randn(b * s, ld, generator=g) * 2
    labels = torch.where(torch.rand(b * s, generator=g) < 0.7, torch.full((b * s,), k), torch.randint(0, k, (b * s,), generator=g))
    ga = torch.where(labels < k, torch.randint(0, ldc, (b * s,), generator=g), torch.full((b * s,), -1))
    d = lambda t, dt=torch.float32: t.to(dt).to(dev).contiguous()
    return dict(logits=d(logits), col0=2 * k, k=k, valid=d(torch.zeros(b * s), torch.int32), s=s, b=b, labels=d(labels, torch.int32),
                cls_weights=d(torch.rand(b * s, generator=g)), gt_assign=d(ga, torch.int32),
                pc_count=d(torch.randint(1, 40, (b, ldc), generator=g), torch.int32), pc_img_cls_weights=d(torch.rand(b, ldc, generator=g) * 5),
                pc_probs=d(torch.rand(b, ldc, generator=g) * 0.5 + 0.1), n_pc=d(torch.full((b,), ldc), torch.int32)), ld


def main():
    dev = torch.device("cuda:0")
    for k, s, ncls in ((20, 512, 2), (80, 512, 3), (20, 64, 2), (80, 128, 3)):
        a, ld = inputs(2, s, k, ncls, dev)
        dy = torch.zeros((2 * s, ld), dtype=torch.bfloat16, device=dev)
        for _ in range(20):
            ops.pcl_loss(**a, dy=dy, dcol0=a["col0"])
        n = 200
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(n):
            ops.pcl_loss(**a, dy=dy, dcol0=a["col0"])
        t1.record()
        torch.cuda.synchronize()
        print(json.dumps({"K": k, "images": 2, "rows_per_image": s, "us_per_launch": round(t0.elapsed_time(t1) * 1000 / n, 2)}))


if __name__ == "__main__":
    main()
