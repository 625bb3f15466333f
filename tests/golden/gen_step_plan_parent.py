"""Writes tests/golden/step_plan_parent.json: what the training step records and computes in three forms of the plan, taken on the commit
BEFORE the settled A/B switches of the step were retired (run on the GPU, on that commit: `python tests/golden/gen_step_plan_parent.py [output path [cases]]`).
tests/test_step_gpu.py::test_step_plan_is_the_parent_commits imports this file for CASES / run_case and compares a fresh run with the fixture.

Per case: the names of the recorded calls in order, for every call the ROLE of the stream it was issued on (main / head / wgrad / rpn /
other; `none` for a call without a stream argument) and the six loss vectors of ReplayedStep(warmup_steps=2) over three batches in the
order 0,1,2,1,0,2. The setup is the small one of tests/test_box_loss_gpu.py::_setup (R50, 32 RoIs per image, 600 -> 100 proposals, PCL)."""
import ctypes
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "step_plan_parent.json")
ORDER = (0, 1, 2, 1, 0, 2)
RAGGED_SIZES = ((128, 192), (112, 160), (96, 176), (128, 144))          # tests/test_step_gpu.py::test_s1_step_mixed_image_sizes_fp32
CASES = ("ragged", "two_pass", "sup_only")
# (no mask-head case: on that commit two EAGER bf16 runs of the C4-segm step -- MASK_ON, single Res5 head, 2 + 2 images -- already disagree in
#  loss_mask on their first step, 0.7189 against 0.7641, and the step dispatches stock ATen clone / copy_ / add calls that a call list does not
#  hold: there is nothing reproducible to pin)


def _setup(case):
    from unit_amd import config
    from unit_amd.modeling import build_model
    from unit_amd.synthetic import init_synthetic_weights
    cfg = config.voc_rcnn_c4_split1(50)
    cfg.MODEL.DEVICE = "cuda"
    cfg.MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE = 32
    cfg.MODEL.RPN.PRE_NMS_TOPK_TRAIN, cfg.MODEL.RPN.POST_NMS_TOPK_TRAIN = 600, 100
    cfg.MODEL.ROI_HEADS.FAST_RCNN.WEAK_DETECTOR.TYPE = "PCL"
    cfg.SOLVER.WARMUP_ITERS = 4
    cfg.SEED = 3
    model = build_model(cfg)
    init_synthetic_weights(model, seed=1)
    model.train()
    model.compute_mode = "bf16"
    if case == "two_pass":
        model.ragged_single_pass = False
    return cfg, model


def _data(case):
    """three distinct batches of one batch key"""
    from unit_amd.synthetic import synthetic_batch
    out = []
    for k in range(3):
        if case in ("ragged", "two_pass"):
            sup, weak = [], []
            for i, hw in enumerate(RAGGED_SIZES):
                s, w = synthetic_batch(1, 1, hw=hw, seed=70 + 10 * k + i, max_gt=3)
                (sup if i < 2 else weak).append(s[0] if i < 2 else w[0])
        else:
            sup, weak = synthetic_batch(2, 0 if case == "sup_only" else 2, hw=(128, 192), seed=50 + k, max_gt=4)
            weak = weak or None
        out.append((sup, weak))
    return out


def _stream_slot():
    """{function: index of its stream among the integer-class argument words of a recorded call}: the parameter named `stream` (`waiter` for
    unit_stream_wait_stream, `compute_stream` for unit_comm_wait) by include/unit_hip.h, floats not counted (UnitCall keeps them apart)"""
    from unit_amd import _lib
    protos, slots = _lib.parse_header(), {}
    for fn, params in _lib.parse_header_names().items():
        at = next((params.index(p) for p in ("stream", "waiter", "compute_stream") if p in params), None)
        if at is not None:
            slots[fn] = sum(1 for t in protos[fn][1][:at] if t is not ctypes.c_float)
    return slots


def plan_of(rs, model):
    """-> (names, stream roles) of the one recorded plan of `rs`"""
    (plan, *_), = rs.plans.values()
    role = {}
    for name, s in (("rpn", model._rpn_stream), ("wgrad", model._wgrad_stream), ("head", model._head_stream), ("main", torch.cuda.current_stream())):
        role[s.cuda_stream] = name          # (in this order: `main` wins a tie, then head, wgrad, rpn)
    slots = _stream_slot()
    names, roles = [], []
    for it in plan.items:
        if it[0] != "calls":
            continue
        for rec, fn in zip(it[1], it[3]):
            names.append(fn)
            roles.append(role.get(rec.i[slots[fn]] & (2 ** 64 - 1), "other") if fn in slots else "none")
    return names, roles


def run_case(case):
    """-> dict(names, streams, eager [6 loss tensors], replayed [6], m_eager, m_replayed, stats)"""
    from unit_amd import engine
    from unit_amd.solver import FlatSGD
    data = _data(case)
    seq = [data[i] for i in ORDER]
    cfg, m1 = _setup(case)
    o1 = FlatSGD(m1, cfg)
    ref = []
    for sup, weak in seq:
        b = m1.pack_batch(sup, weak, gt_buckets=engine.GraphedStep.GT_BUCKETS)
        o1._bind()
        o1.use_device_lr(m1.device)
        step = m1.forward_train(b, early_backward=True)
        m1.backward_train(step)
        o1.step()
        ref.append(step.losses.clone())
    torch.cuda.synchronize()
    cfg, m2 = _setup(case)
    rs = engine.ReplayedStep(m2, FlatSGD(m2, cfg), warmup_steps=2)
    got = [rs.run(sup, weak).clone() for sup, weak in seq]
    torch.cuda.synchronize()
    names, roles = plan_of(rs, m2)
    return dict(names=names, streams=roles, eager=ref, replayed=got, m_eager=m1, m_replayed=m2, stats=dict(rs.stats), form=(step.split, step.ragged))


def main(path=OUT, *cases):
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    out = {}
    for case in cases or CASES:
        r = run_case(case)
        same = all(torch.equal(a, b) for a, b in zip(r["replayed"], r["eager"])) and torch.equal(r["m_replayed"].store.params, r["m_eager"].store.params)
        counts = {k: r["streams"].count(k) for k in sorted(set(r["streams"]))}
        print(f"{case}: {len(r['names'])} calls, streams {counts}, stats {r['stats']}, (split, ragged) {r['form']}, replay == eager: {same}", flush=True)
        assert same, case
        out[case] = dict(names=r["names"], streams=r["streams"], losses=[t.tolist() for t in r["replayed"]])
    with open(path, "w") as f:
        json.dump(out, f)


if __name__ == "__main__":
    main(*sys.argv[1:])          # (optional: another output path, then the cases to write)
