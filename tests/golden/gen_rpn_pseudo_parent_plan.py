"""Writes tests/golden/rpn_pseudo_parent_plan.json: the call list a WeaklySupervisedRCNNNoMeta step records, and the loss vectors it computes,
taken on the commit BEFORE WeaklySupervisedRCNNRPN was added (run on the GPU, from the root of a checkout of that commit, with this file
copied in: `python tests/golden/gen_rpn_pseudo_parent_plan.py [output path]`). tests/test_rpn_pseudo_gpu.py imports this file for `run()` and
compares a fresh run with the fixture: the new class shares forward_train / backward_train / StandardRPNHead.bwd / Conv2d.wgrad /
LinearGroup.bwd with the old one, and none of what it added there may show in the old one's step.

The setup is the "s1" case of tests/golden/gen_ref_step.py (R50, 96 x 128, 300 -> 50 proposals, 16 RoIs per image, 2 + 2 images, K = 20, two
Res5 heads) in bf16, through ReplayedStep(warmup_steps=2) on one batch four times: two eager steps, the recording, one replay."""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "rpn_pseudo_parent_plan.json")


def run():
    """-> dict(names [recorded calls in order], losses [4 loss vectors as lists], stats)"""
    for p in (HERE, os.path.dirname(os.path.dirname(HERE))):
        if p not in sys.path:
            sys.path.insert(0, p)
    import gen_ref_step as S
    from unit_amd import engine
    from unit_amd.solver import FlatSGD
    cfg, model, sup, weak, _, _ = S.step_inputs("s1", device="cuda")
    assert type(model).__name__ == "WeaklySupervisedRCNNNoMeta"
    model.train()
    model.compute_mode = "bf16"
    rs = engine.ReplayedStep(model, FlatSGD(model, cfg), warmup_steps=2)
    losses = [rs.run(sup, weak).clone() for _ in range(4)]
    torch.cuda.synchronize()
    (plan, *_), = rs.plans.values()
    names = [n for it in plan.items if it[0] == "calls" for n in it[3]]
    return dict(names=names, losses=[t.tolist() for t in losses], stats=dict(rs.stats))


if __name__ == "__main__":
    r = run()
    print(len(r["names"]), "calls", r["stats"], r["losses"][-1], flush=True)
    with open(sys.argv[1] if len(sys.argv) > 1 else OUT, "w") as f:
        json.dump(r, f)
