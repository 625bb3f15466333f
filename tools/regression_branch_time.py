"""What WEAK_DETECTOR.REGRESSION_BRANCH costs at the benchmark's size: the whole training step (R101, 600 x 1000, 2 + 2 images, 512 weak RoIs
per image, bf16, eager; forward + backward + SGD) with the switch off and on, under TYPE "OICR" and "PCL", same build, same process. HIP events
around every step, median of 20 after 5 warm-up steps; one JSON line per configuration. The switch adds two column blocks to the weak head's
fused GEMM and weight-gradient launch, unit_softmax_mean, one *_targets_ex launch and two loss launches (on the side stream beside the MIL
kernel). bench.py itself never turns the switch on.
  python tools/regression_branch_time.py [OICR|PCL ...]"""
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


def main(types):
    from unit_amd import config
    from unit_amd.modeling import build_model
    from unit_amd.solver import FlatSGD
    from unit_amd.synthetic import init_synthetic_weights, synthetic_batch
    for typ in types:
        for on in (False, True, False):          # off twice: the second off figure shows the run-to-run spread the on figure sits in
            cfg = config.voc_rcnn_c4_split1(101)
            cfg.MODEL.DEVICE = "cuda:0"
            wd = cfg.MODEL.ROI_HEADS.FAST_RCNN.WEAK_DETECTOR
            wd.TYPE, wd.REGRESSION_BRANCH = typ, on
            ft = cfg.MODEL.ROI_HEADS.FINETUNE_TERMS
            ft.CLASSIFIER, ft.BBOX, ft.MASK = ["lingual"], ["lingual"], ["lingual"]          # ("visual" terms are refused under the switch)
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
                return st
            med, lo = median_ms(step)
            losses = step().losses
            assert torch.isfinite(losses).all(), losses
            print(json.dumps({"what": "training_step", "TYPE": typ, "REGRESSION_BRANCH": on, "median_ms": med, "min_ms": lo,
                              "loss_slots": losses.numel()}), flush=True)
            del model, opt, batch
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main([a for a in sys.argv[1:] if a in ("OICR", "PCL")] or ["OICR", "PCL"])
