"""Writes tests/golden/load_proposals_parent_plan.json: what the default S1 training step (MODEL.LOAD_PROPOSALS False, TYPE "OICR", equal-size
2 + 2 images) records and computes, taken on the commit BEFORE MODEL.LOAD_PROPOSALS was honoured (run on the GPU, on that commit:
`python tests/golden/gen_load_proposals_parent_plan.py [output path]`). tests/test_load_proposals_gpu.py::
test_default_step_plan_is_the_parent_commits imports this file for run_case and compares a fresh run with the fixture.

The machinery is gen_step_plan_parent.py's (the names of the recorded calls in order, the role of the stream of every call, the six loss
vectors of ReplayedStep(warmup_steps=2) over three batches in the order 0,1,2,1,0,2), whose own cases run TYPE "PCL": this one is the
configuration the benchmark runs, with the OICR targets kernel in the plan."""
import importlib.util
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "load_proposals_parent_plan.json")
CASE = "equal"          # gen_step_plan_parent._data: any other name than its ragged / sup-only cases is 2 + 2 images of 128 x 192


def _machinery():
    spec = importlib.util.spec_from_file_location("_gen_step_plan_parent_lp", os.path.join(HERE, "gen_step_plan_parent.py"))
    gsp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gsp)
    plain = gsp._setup

    def setup(case):
        cfg, model = plain(case)
        assert cfg.MODEL.LOAD_PROPOSALS is False
        cfg.MODEL.ROI_HEADS.FAST_RCNN.WEAK_DETECTOR.TYPE = "OICR"
        from unit_amd.modeling import build_model
        from unit_amd.synthetic import init_synthetic_weights
        model = build_model(cfg)
        init_synthetic_weights(model, seed=1)
        model.train()
        model.compute_mode = "bf16"
        return cfg, model
    gsp._setup = setup
    return gsp


def run_case():
    """-> gen_step_plan_parent.run_case's dict for the default OICR step"""
    return _machinery().run_case(CASE)


def main(path=OUT):
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    r = run_case()
    same = all(torch.equal(a, b) for a, b in zip(r["replayed"], r["eager"])) and torch.equal(r["m_replayed"].store.params, r["m_eager"].store.params)
    print(f"{len(r['names'])} calls, stats {r['stats']}, replay == eager: {same}", flush=True)
    assert same
    with open(path, "w") as f:
        json.dump(dict(names=r["names"], streams=r["streams"], losses=[t.tolist() for t in r["replayed"]]), f)


if __name__ == "__main__":
    main(*sys.argv[1:])
