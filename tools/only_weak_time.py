"""Weak-only training (TrainerOnlyWeak, DESIGN.md section 8 "Weak-only training") at the bench shapes: R101, bf16, 600 x 1000.

  python tools/only_weak_time.py [blocks] [steps_per_block] [out.txt]          (default out: profiles/r13_only_weak.txt)

One process, after warm-up, alternating block by block; every figure is the median over the blocks with its min / max beside it:
  step_ms        the eager weak-only step (2 weak images, TrainerOnlyWeak.run_step) against the eager default step of the same session
                 (2 supervised + 2 weak images, TrainerNoMeta.run_step): HIP events around a block of steps
  host_ms        host time until run_step returns, from an idle device (a synchronise before every step)
  update_us      the optimizer update over the whole flat store: unit_sgd_step, unit_sgd_step_masked with an all-live mask, and with the
                 weak-only ("ow") mask -- beside the bytes each moves by its algorithm (5 x 4 bytes per element that is updated)
The default bench line of this commit beside the parent commit's comes from tools/ab_old_new.sh (a worktree of the parent commit with
its own build under _ab_old, `bench.py --no-cpu-baseline --no-roofline --steps 30 --warmup 5` in both trees, alternating); its lines go
under the "## bench.py" heading of the same file, which this tool keeps when it rewrites its own part."""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from unit_amd import config, engine, ops  # noqa: E402
from unit_amd.modeling import build_model  # noqa: E402
from unit_amd.synthetic import init_synthetic_weights, synthetic_batch  # noqa: E402

HW = (600, 1000)
BENCH_SECTION = "## bench.py"


def med(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def make(cls):
    cfg = config.voc_rcnn_c4_split1(101)
    cfg.MODEL.DEVICE = "cuda:0"
    model = build_model(cfg)
    init_synthetic_weights(model, seed=1)
    model.train()
    model.compute_mode = "bf16"
    return cfg, model, cls(cfg, model)


def main(blocks=9, steps=10, out_path=os.path.join(ROOT, "profiles", "r13_only_weak.txt")):
    assert torch.cuda.is_available(), "only_weak_time.py measures on the GPU: there is nothing to fall back to"
    sup, weak = synthetic_batch(2, 2, hw=HW, seed=5, max_gt=8)
    _, m_ow, t_ow = make(engine.TrainerOnlyWeak)
    _, m_df, t_df = make(engine.TrainerNoMeta)
    b_ow, b_df = m_ow.pack_batch(None, weak), m_df.pack_batch(sup, weak)
    pack = {"only_weak": (m_ow, b_ow), "default": (m_df, b_df)}
    for name, (m, b) in pack.items():          # the trainers' steps on device-resident batches: no host-to-device copy in the timed window
        m.pack_batch = (lambda b_: (lambda *a, **k: b_))(b)
    runs = {"only_weak": lambda: t_ow.run_step(None, weak), "default": lambda: t_df.run_step(sup, weak)}
    for fn in runs.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    step_ms, host_ms = {n: [] for n in runs}, {n: [] for n in runs}
    for _ in range(blocks):
        for n, fn in runs.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(steps):
                fn()
            t1.record()
            torch.cuda.synchronize()
            step_ms[n].append(t0.elapsed_time(t1) / steps)
        for n, fn in runs.items():
            h = []
            for _ in range(steps):
                torch.cuda.synchronize()
                a = time.perf_counter()
                fn()
                h.append((time.perf_counter() - a) * 1e3)
            host_ms[n].append(statistics.median(h))
    torch.cuda.synchronize()
    # the optimizer update alone, on the weak-only trainer's store
    opt, st = t_ow.optimizer, m_ow.store
    live = m_ow.live_entries(False, True)
    opt.set_live(live)
    table, live_dev = opt._mask_table, opt._live_dev
    all_live = torch.ones_like(live_dev)
    rows = [(o, e - o) for o, e in zip(opt._row_off, opt._row_end)]
    dead_elems = sum(n for (o, n), l in zip(rows, live) if not l)
    g = torch.randn(st.size, device=st.params.device) * 1e-3
    keep = st.params.clone()
    forms = {
        "sgd_step": lambda: ops.sgd_step(st.params, g, opt._buf, 0, st.size, 1e-7, 0.9, 1e-4),
        "masked_all_live": lambda: ops.sgd_step_masked(st.params, g, opt._buf, 0, st.size, 1e-7, 0.9, 1e-4, table, all_live),
        "masked_ow": lambda: ops.sgd_step_masked(st.params, g, opt._buf, 0, st.size, 1e-7, 0.9, 1e-4, table, live_dev),
    }
    for fn in forms.values():
        for _ in range(5):
            fn()
    upd = {n: [] for n in forms}
    for _ in range(blocks * 3):
        for n, fn in forms.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(steps):
                fn()
            t1.record()
            torch.cuda.synchronize()
            upd[n].append(t0.elapsed_time(t1) * 1e3 / steps)
    st.params.copy_(keep)
    res = {"shapes": {"backbone": "R101", "mode": "bf16", "hw": HW, "weak_images": 2, "default_step_images": "2 supervised + 2 weak"},
           "blocks": blocks, "steps_per_block": steps,
           "step_ms": {n: med(v) for n, v in step_ms.items()}, "host_ms": {n: med(v) for n, v in host_ms.items()},
           "update_us": {n: med(v) for n, v in upd.items()},
           "store_elements": st.size, "dead_elements": dead_elems, "dead_tensors": sum(1 for l in live if not l), "tensors": len(live),
           "bytes_moved": {"sgd_step": 20 * st.size, "masked_all_live": 20 * st.size, "masked_ow": 20 * (st.size - dead_elems)}}
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    kept = ""          # the bench.py section of an earlier file (tools/ab_old_new.sh's lines, see the docstring) is not this tool's to drop
    if os.path.exists(out_path):
        old = open(out_path).read()
        if BENCH_SECTION in old:
            kept = old[old.index(BENCH_SECTION):]
    with open(out_path, "w") as f:
        f.write("# Weak-only training (TrainerOnlyWeak, train_only_weak=True) on the MI355X: tools/only_weak_time.py, alternating forms in one run.\n"
                "# R101, bf16, 600 x 1000; eager steps; every figure a median over the session's blocks with its min / max.\n\n")
        f.write(json.dumps(res) + "\n")
        if kept:
            f.write("\n" + kept)
    print(json.dumps(res))


if __name__ == "__main__":
    a = sys.argv[1:]
    main(*([int(x) for x in a[:2]] + a[2:3]))
