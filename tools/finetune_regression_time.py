"""What WEAK_DETECTOR.REGRESSION_BRANCH costs the SECOND stage at the benchmark's size: the fine-tune step of the VOC fine-tune configuration
(R101, 600 x 1000, 2 supervised images, 512 RoIs per image, bf16; forward + backward + SGD on the two ft heads), eager and replayed
(engine.ReplayedStep), with the switch off, on and off again in one process. HIP events around every step, median of 20 after 5 warm-up steps
(minimum beside it); one JSON line per configuration, then the on - off difference beside the spread of the two off runs. The switch swaps
unit_transfer_predictions for unit_transfer_predictions_ex (one launch either way) and widens the weak head's fused GEMM by two column blocks.

Then the launch itself at the step's shape (1024 rows, K = 20, 15 base / 5 novel classes): unit_transfer_predictions_ex against the two
launches it stands for, unit_transfer_predictions + unit_sup_scores over the 4K delta columns, each form between one pair of HIP events on an
otherwise idle stream (tools/box_loss_time.py's bracket: the pair includes the ~5 us a launch costs there), median and min - max of 50.
No bar: a measurement for DESIGN.md section 8. bench.py itself never turns the switch on.
  python tools/finetune_regression_time.py"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed_ms(fn, n=20, warm=5):
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
    return ts


def build(on):
    from unit_amd import config
    from unit_amd.modeling import build_model
    from unit_amd.synthetic import init_synthetic_weights
    cfg = config.voc_rcnn_c4_split1_ft(101)
    cfg.MODEL.DEVICE = "cuda:0"
    cfg.MODEL.ROI_HEADS.FAST_RCNN.WEAK_DETECTOR.REGRESSION_BRANCH = on
    ft = cfg.MODEL.ROI_HEADS.FINETUNE_TERMS
    ft.CLASSIFIER, ft.BBOX, ft.MASK = ["lingual"], ["lingual"], ["lingual"]          # ("visual" terms are refused under the switch)
    cfg.SEED = 0
    model = build_model(cfg)
    init_synthetic_weights(model, seed=1)
    model.train()
    model.compute_mode = "bf16"
    return cfg, model


def steps():
    from unit_amd import engine
    from unit_amd.solver import FlatSGD
    from unit_amd.synthetic import synthetic_batch
    sup, _ = synthetic_batch(2, 0, seed=100, base_ids=list(range(20)))
    res = {"eager": [], "replayed": []}
    for on in (False, True, False):          # off twice: the second off figure shows the run-to-run spread the on figure sits in
        for mode in ("eager", "replayed"):
            cfg, model = build(on)
            opt = FlatSGD(model, cfg)
            if mode == "eager":
                batch = model.pack_batch(sup, None)

                def step():
                    st = model.forward_train(batch, early_backward=True)
                    model.backward_train(st)
                    opt.step()
                    return st.losses
            else:
                rs = engine.ReplayedStep(model, opt, warmup_steps=1)

                def step():
                    return rs.run(sup, None)
            ts = timed_ms(step)
            losses = step()
            torch.cuda.synchronize()
            assert torch.isfinite(losses).all(), losses
            med = statistics.median(ts)
            res[mode].append(med)
            print(json.dumps({"what": "finetune_step", "mode": mode, "REGRESSION_BRANCH": on, "median_ms": round(med, 3), "min_ms": round(min(ts), 3),
                              "loss_slots": losses.numel()}), flush=True)
            del model, opt, step
            torch.cuda.empty_cache()
    for mode, (off0, on_, off1) in res.items():
        print(json.dumps({"what": "on_minus_off", "mode": mode, "on_minus_mean_off_ms": round(on_ - (off0 + off1) / 2, 3),
                          "off_spread_ms": round(abs(off0 - off1), 3)}), flush=True)


def launch(rows=1024, k=20, n=50):
    from unit_amd import ops
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    base = [0, 1, 3, 4, 6, 7, 8, 10, 11, 12, 14, 15, 16, 18, 19]
    novel = [2, 5, 9, 13, 17]
    role, slot = torch.zeros(k, dtype=torch.int8), torch.zeros(k, dtype=torch.int32)
    for i, c in enumerate(base):
        role[c], slot[c] = 1, i
    for i, c in enumerate(novel):
        role[c], slot[c] = 2, i
    t = dict(base=torch.tensor(base, dtype=torch.int32, device=dev), novel=torch.tensor(novel, dtype=torch.int32, device=dev), role=role.to(dev),
             slot=slot.to(dev))
    kp = (5 * k + 1 + 7) // 8 * 8          # [cls | bbox] padded, the predictors' group layout
    lin, ft = torch.randn(rows, kp, generator=g).to(dev), torch.randn(rows, kp, generator=g).to(dev)
    wcols = 2 * k + 3 * (k + 1)          # classifier, detection and three refinement blocks in front of the regression columns
    weak = torch.randn(rows, (wcols + 5 * k + 1 + 7) // 8 * 8, generator=g).to(dev)
    sim = torch.rand(rows, len(novel), len(base), generator=g)
    sim = (sim / sim.sum(-1, keepdim=True)).to(dev)
    args = (lin, 0, k + 1, k, weak, wcols, 1, sim, sim, t["base"], t["novel"], t["role"], t["slot"])

    def one():
        return ops.transfer_predictions(*args, ft=ft, fccol0=0, fbcol0=k + 1, wbcol0=wcols + k + 1)

    def two():
        s, b = ops.transfer_predictions(*args, ft=ft, fccol0=0, fbcol0=k + 1)
        return s, ops.sup_scores(b, 0, weak, wcols + k + 1, 1, 4 * k)
    for name, fn in (("unit_transfer_predictions_ex", one), ("unit_transfer_predictions + unit_sup_scores", two), ("unit_transfer_predictions_ex", one)):
        us = [v * 1e3 for v in timed_ms(fn, n=n, warm=5)]
        print(json.dumps({"what": "launch", "form": name, "rows": rows, "K": k, "median_us": round(statistics.median(us), 2),
                          "min_us": round(min(us), 2), "max_us": round(max(us), 2)}), flush=True)


if __name__ == "__main__":
    steps()
    launch()
