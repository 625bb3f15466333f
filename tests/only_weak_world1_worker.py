"""The weak-only step with ONE RCCL rank and every collective forced on (tests/test_only_weak_gpu.py starts this as a fresh child
process; the pattern of tests/rccl_world1_worker.py). Three TrainerOnlyWeak steps on the "ow" fixture inputs without collectives, then
the same three with UNIT_FORCE_COLLECTIVES=1: every gradient bucket -- the dead ones too, as the zeros they hold -- is exchanged from
inside the backward and waited for by finish(); a sum over one rank is the identity, so the parameters must end BIT-equal.
usage: python tests/only_weak_world1_worker.py <port> <out.json>"""
import json
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

STEPS = 3


def main():
    port, out = sys.argv[1], sys.argv[2]
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", port
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    import gen_only_weak_golden as W
    from unit_amd import engine

    def run():
        cfg, model, weak = W.only_weak_inputs("ow", device="cuda")
        model.train()
        model.compute_mode = "fp32"
        tr = engine.TrainerOnlyWeak(cfg, model)
        fired = []
        hook = model.on_grad_ready
        if hook is not None:
            model.on_grad_ready = lambda tag: (fired.append(tag), hook(tag))[1]
        for _ in range(STEPS):
            losses = tr.run_step(None, weak)
        torch.cuda.synchronize()
        return model.store.params.clone(), losses.clone(), tr.buckets, fired, model.only_weak_tag_sequence()

    os.environ["UNIT_FORCE_COLLECTIVES"] = "0"
    ref_p, ref_l, b0, _, _ = run()
    assert not b0.active and b0.launched == 0
    os.environ["UNIT_FORCE_COLLECTIVES"] = "1"
    p, l, b, fired, seq = run()
    res = {"bit_equal": bool(torch.equal(p, ref_p)), "max_abs_diff": float((p - ref_p).abs().max()), "loss_equal": bool(torch.equal(l, ref_l)),
           "finite": bool(torch.isfinite(p).all()), "launched": b.launched, "active": bool(b.active), "fired": fired, "sequence": seq,
           "left_waiting": len(b._works)}
    json.dump(res, open(out, "w"))
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
