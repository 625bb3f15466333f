"""RoIPool (csrc/roi_pool.hip) beside RoIAlign (csrc/roi_align.hip) at the bench shapes, and the eager S1 step under either pooler type.

    python tools/roi_pool_time.py kernels [iters=50]     the four launches on the same RoIs
    python tools/roi_pool_time.py step [blocks=5] [steps=10]     the eager R101 S1 step, POOLER_TYPE "ROIAlignV2" / "ROIPool" alternating

kernels: the R101 C4 map of 4 images of 600 x 1000 (38 x 63 x 1024, bf16), 2 x 512 supervised + 2 x 512 weak RoIs in fixed slots (boxes
of 16 .. 616 x 16 .. 416 px inside the image, as tools/roi_bwd_time.py draws them), strided mode (7 x 7 of the 14 x 14 grid). The forward is
timed over all 2048 RoIs in one launch; the backward as the step issues it: one launch per image group (2 images, 1024 RoIs), with the
fused epilogue `+ addend, * (mask_ref > 0)`, bf16 out. HIP events around `iters` back-to-back launches after a warm-up; every line is the
mean per launch, with the bytes the algorithm moves (ops._timed's accounting) over that time. No bar: a measurement for DESIGN.md section 8."""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from unit_amd import config, ops  # noqa: E402
from unit_amd.modeling import build_model  # noqa: E402
from unit_amd.synthetic import init_synthetic_weights, synthetic_batch  # noqa: E402

N, H, W, C, S = 4, 38, 63, 1024, 512
MODE = (14, 7, 2)


def timeit(fn, iters, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3          # us


def bench_rois(g):
    out = []
    for i in range(N):
        wh = torch.rand(S, 2, generator=g) * torch.tensor([600.0, 400.0]) + 16
        xy = torch.rand(S, 2, generator=g) * (torch.tensor([1000.0, 600.0]) - wh).clamp(min=1)
        out.append(torch.cat([torch.full((S, 1), float(i)), xy, xy + wh], 1))
    return torch.cat(out, 0)


def kernels(iters):
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(3)
    pooled, osz, step = MODE
    rois = bench_rois(g).to(dev)
    feat = torch.relu(torch.randn(N, H, W, C, generator=g)).to(dev).bfloat16()          # a res4 output: about half of it zero
    gout = torch.randn(N * S, osz, osz, C, generator=g).to(dev).bfloat16()
    add = torch.randn(N, H, W, C, generator=g).to(dev).bfloat16()
    out = torch.empty(N * S, osz, osz, C, dtype=torch.bfloat16, device=dev)
    am = torch.empty(N * S, osz, osz, C, dtype=torch.int32, device=dev)
    d = torch.empty(N, H, W, C, dtype=torch.bfloat16, device=dev)
    half, rh = N // 2, N // 2 * S
    es = 2
    fwd_bytes = feat.numel() * es + out.numel() * es
    bwd_bytes = rh * osz * osz * C * es + 3 * half * H * W * C * es          # gout + (dfeat, addend, mask_ref) of one image group
    res = {}

    def line(name, us, nbytes):
        res[name] = {"us": round(us, 1), "algorithmic_MB": round(nbytes / 1e6, 1), "GB_per_s": round(nbytes / us / 1e3, 1)}
        print(f"{name:34s} {us:8.1f} us   {nbytes / 1e6:7.1f} MB   {nbytes / us / 1e3:7.1f} GB/s", flush=True)

    line("roi_align_fwd", timeit(lambda: ops.roi_align(feat, rois, pooled, osz, step, 1 / 16, 0, True, out=out), iters), fwd_bytes)
    line("roi_pool_fwd (argmax stored)", timeit(lambda: ops.roi_pool(feat, rois, pooled, osz, step, 1 / 16, out=out, argmax=am), iters),
         fwd_bytes + am.numel() * 4)
    line("roi_pool_fwd (argmax = NULL)", timeit(lambda: ops.roi_pool(feat, rois, pooled, osz, step, 1 / 16, out=out), iters), fwd_bytes)
    ops.roi_pool(feat, rois, pooled, osz, step, 1 / 16, out=out, argmax=am)
    line("roi_align_bwd_gather (1 group)",
         timeit(lambda: ops.roi_align_bwd_gather(gout[:rh], half, H, W, rois[:rh], d[:half], pooled, step, 1 / 16, 0, True, rois_per_image=S,
                                                 addend=add[:half], addend_images=half, mask_ref=feat[:half]), iters), bwd_bytes)
    line("roi_pool_bwd_gather (1 group)",
         timeit(lambda: ops.roi_pool_bwd_gather(gout[:rh], am[:rh], half, H, W, rois[:rh], d[:half], pooled, step, 1 / 16, rois_per_image=S,
                                                addend=add[:half], addend_images=half, mask_ref=feat[:half]), iters),
         bwd_bytes + rh * osz * osz * C * 4)
    sel = (am >= 0).float().mean().item()
    print(json.dumps({"shapes": {"map": [N, H, W, C], "dtype": "bf16", "rois": N * S, "mode": MODE}, "iters": iters,
                      "bins_with_a_selection": round(sel, 4), "kernels": res}))


def step(blocks, steps):
    models = {}
    for pooler in ("ROIAlignV2", "ROIPool"):
        cfg = config.voc_rcnn_c4_split1(101)
        cfg.MODEL.DEVICE = "cuda:0"
        cfg.MODEL.ROI_BOX_HEAD.POOLER_TYPE = pooler
        cfg.SEED = 0
        model = build_model(cfg)
        init_synthetic_weights(model, seed=1)
        model.train()
        model.compute_mode = "bf16"
        batch = model.pack_batch(*synthetic_batch(2, 2, seed=100))
        models[pooler] = (model, batch)

    def run(pooler, n):
        model, batch = models[pooler]
        for _ in range(n):
            model.backward_train(model.forward_train(batch, early_backward=True))
        torch.cuda.synchronize()

    for p in models:
        run(p, 3)
    ms = {p: [] for p in models}
    for _ in range(blocks):
        for p in models:          # alternating: both forms see the same box in the same minutes
            t0 = time.perf_counter()
            run(p, steps)
            ms[p].append((time.perf_counter() - t0) / steps * 1e3)
    out = {p: {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)} for p, v in ms.items()}
    print(json.dumps({"eager_s1_step_ms": out, "blocks": blocks, "steps_per_block": steps,
                      "shapes": {"backbone": "R101", "mode": "bf16", "hw": [600, 1000], "images": "2 supervised + 2 weak", "rois": 2048}}))


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "kernels"
    args = [int(a) for a in sys.argv[2:]]
    if what == "kernels":
        kernels(*(args or [50]))
    elif what == "step":
        step(*(args or [5, 10]))
    else:
        raise SystemExit(__doc__)
