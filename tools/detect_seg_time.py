"""The detect stage (ops.detections: candidates, score sort, NMS stage, finalize) in its two forms, and what the NMS stage needs as scratch.

    python tools/detect_seg_time.py [blocks=5] [iters=10]

Shapes R proposals x K classes with every (RoI, class) pair a candidate (cand_cap = R * K, scores as summed over ten TTA views), one image
of 600 x 1000, topk 100, NMS threshold 0.5: 1000 x 20 in both forms ("full": one all-pairs unit_nms over the class-shifted list;
"segmented": class segments, unit_nms per class, merge), 2000 x 80 and 4000 x 80 in the segmented form only (the full form refuses more
than 65 536 candidates). The forms alternate in blocks of `iters` calls (HIP events around a block, after a warm-up); every line is the
median over the blocks of the mean per call. A record: no decision hangs on it."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from unit_amd import ops  # noqa: E402
from unit_amd._lib import lib  # noqa: E402

HW = (600.0, 1000.0)
WEIGHTS = (10.0, 10.0, 5.0, 5.0)
TOPK, NMS_THRESH = 100, 0.5
SHAPES = [(1000, 20, ("full", "segmented")), (2000, 80, ("segmented",)), (4000, 80, ("segmented",))]


def inputs(r, k, dev, seed=0):
    g = torch.Generator().manual_seed(seed + r + k)
    wh = torch.rand(r, 2, generator=g) * torch.tensor([400.0, 300.0]) + 16
    xy = torch.rand(r, 2, generator=g) * (torch.tensor([HW[1], HW[0]]) - wh)
    props = torch.cat([xy, xy + wh], 1)[None]
    probs = torch.softmax(torch.randn(10, r, k + 1, generator=g), -1).sum(0)          # ten views' probabilities, summed: all far above 0.05
    deltas = torch.randn(r, 4 * k, generator=g)
    return tuple(t.to(dev) for t in (probs, deltas, props, torch.tensor([r], dtype=torch.int32), torch.tensor([HW])))


def block(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3          # us


def main(blocks=5, iters=10):
    dev = torch.device("cuda:0")
    out = []
    for r, k, forms in SHAPES:
        inp = inputs(r, k, dev)
        cap = r * k

        def call(form):
            return ops.detections(*inp, WEIGHTS, 0.05, NMS_THRESH, TOPK, cand_cap=cap, nms=form)
        counts = {}
        for f in forms:
            for _ in range(3):
                res = call(f)
            counts[f] = int(res[4][0])
        us = {f: [] for f in forms}
        for _ in range(blocks):
            for f in forms:          # alternating: both forms see the same box in the same minutes
                us[f].append(block(lambda: call(f), iters))
        ws = {"full": int(lib().unit_nms_workspace_bytes(1, cap)) if cap <= ops.max_detection_candidates() else None,
              "segmented": int(lib().unit_nms_workspace_bytes(k, r)) + int(lib().unit_detection_segments_workspace_bytes(1, cap, k))}
        for f in forms:
            line = {"shape": f"{r} x {k}", "candidates": cap, "form": f, "us_median": round(statistics.median(us[f]), 1),
                    "us_min": round(min(us[f]), 1), "us_max": round(max(us[f]), 1), "nms_workspace_MB": round(ws[f] / 1e6, 2),
                    "detections": counts[f]}
            out.append(line)
            print(f"{line['shape']:10s} {f:10s} {line['us_median']:9.1f} us (min {line['us_min']:.1f}, max {line['us_max']:.1f})   "
                  f"workspace {line['nms_workspace_MB']:8.2f} MB   {counts[f]} detections", flush=True)
        if ws["full"] is None:
            print(f"{r} x {k}: the full form would need {cap * ((cap + 63) // 64) * 8 / 1e6:.0f} MB of mask and is refused above "
                  f"{ops.max_detection_candidates()} candidates", flush=True)
    print(json.dumps({"blocks": blocks, "iters_per_block": iters, "topk": TOPK, "nms_thresh": NMS_THRESH, "lines": out}))


if __name__ == "__main__":
    main(*[int(a) for a in sys.argv[1:]])
