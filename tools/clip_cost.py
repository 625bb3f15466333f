"""Cost of gradient clipping in the optimizer update (csrc/optim.hip; DESIGN.md section 8 "Gradient clipping and Nesterov").

  python tools/clip_cost.py [blocks] [steps_per_block]

The flat store of the bench workload's model (R101 S1) with a random gradient buffer; four optimizers over it -- clipping disabled (the
`unit_sgd_momentum` launches of before), "value", "norm", "full_model" -- timed in one process after warm-up, alternated block by block.
Two HIP-event times per setting, each the median over the blocks of (time of a block of steps) / steps:
  update_us  the optimizer's own launches (FlatSGD._apply over the whole store): the norm pass, if any, and the SGD launches
  step_us    optimizer.step(): the same plus whatever the model does after an update (its weight re-preparation launch, once a forward
             has made the prepared copies; this tool runs none, so the two figures should agree)
and the bytes each setting moves by its algorithm: 4 bytes x store.size x (p, g, momentum read; p, momentum written; + one more read of
g under the norm types). One JSON line."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from unit_amd import config  # noqa: E402
from unit_amd.modeling import build_model  # noqa: E402
from unit_amd.solver import FlatSGD  # noqa: E402
from unit_amd.synthetic import init_synthetic_weights  # noqa: E402

SETTINGS = {"disabled": None, "value": ("value", 0.01, 2.0), "norm": ("norm", 0.5, 2.0), "full_model": ("full_model", 5.0, 2.0)}


def main(blocks=21, steps=20):
    assert torch.cuda.is_available(), "clip_cost.py measures on the GPU: there is nothing to fall back to"
    cfg = config.voc_rcnn_c4_split1(101)
    cfg.MODEL.DEVICE = "cuda:0"
    model = build_model(cfg)
    init_synthetic_weights(model, seed=1)
    model.train()
    model.compute_mode = "bf16"
    st = model.flatten_parameters()
    st.grads.copy_(torch.randn(st.size, generator=torch.Generator().manual_seed(0)).mul_(1e-3))
    keep = st.params.clone()
    opts = {}
    for name, clip in SETTINGS.items():
        c = cfg.clone()
        c.SOLVER.BASE_LR = 1e-6          # the parameters stay where they are over the few thousand timed updates
        if clip is not None:
            c.SOLVER.CLIP_GRADIENTS = config.CN(ENABLED=True, CLIP_TYPE=clip[0], CLIP_VALUE=clip[1], NORM_TYPE=clip[2])
        opts[name] = FlatSGD(model, c)
        assert opts[name]._bind() is st

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(steps):
            fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) * 1e3 / steps

    forms = {"update_us": lambda o: (lambda: o._apply(st, 0, st.size)), "step_us": lambda o: o.step}
    for o in opts.values():          # warm-up: first launches load the code objects; the first step takes the first-step form of the update
        for _ in range(3):
            o.step()
    torch.cuda.synchronize()
    out = {"store_elements": st.size, "trainable_tensors": len(opts["norm"].names), "hyper_segments": len(opts["norm"]._segments),
           "blocks": blocks, "steps_per_block": steps}
    for form, make in forms.items():
        samples = {n: [] for n in opts}
        for _ in range(blocks):
            for n, o in opts.items():
                samples[n].append(timed(make(o)))
        out[form] = {n: round(statistics.median(v), 2) for n, v in samples.items()}
        out[form + "_min_max"] = {n: [round(min(v), 2), round(max(v), 2)] for n, v in samples.items()}
    out["bytes_moved"] = {n: 4 * st.size * (5 + (1 if SETTINGS[n] and SETTINGS[n][0] != "value" else 0)) for n in opts}
    c = opts["norm"].clip_coefs()
    out["norm_tensors_clipped"] = int((c < 1).sum().item())
    out["full_model_coef"] = round(opts["full_model"].clip_coefs()[0].item(), 6)
    st.params.copy_(keep)
    print(json.dumps(out))


if __name__ == "__main__":
    main(*[int(a) for a in sys.argv[1:3]])
