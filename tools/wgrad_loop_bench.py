"""A/B of the two loop schedules of the 256x256 weight-gradient tile (UNIT_WGRAD_LOOP = 0 / 1, csrc/conv_wgrad256p8.hip) in ONE process, alternating,
per launch: the five Res5 shapes launched alone (policy variant), the grid of one Res5 head, a six-block res4 bucket and the RPN's 3x3.
python tools/wgrad_loop_bench.py [rounds] [alone]   (alone: only the five launched alone; HIP events around 20 back-to-back launches; prints every round and the medians)"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from unit_amd import ops as o
from tools.wgrad_group_bench import layers_of

SH = [("res5 3x3 512->512", 1024, 7, 7, 512, 512, 3, 1, 1), ("res5 1x1 512->2048", 1024, 7, 7, 512, 2048, 1, 1, 0),
      ("res5 1x1 2048->512", 1024, 7, 7, 2048, 512, 1, 1, 0), ("res5 1x1 1024->512 s2", 1024, 14, 14, 1024, 512, 1, 2, 0),
      ("res5 sc 1024->2048 s2", 1024, 14, 14, 1024, 2048, 1, 2, 0)]


def timed(fn, reps=20):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def ab(name, fn, flops, rounds, check):
    res = {0: [], 1: []}
    outs = {}
    for r in range(rounds):
        for loop in (0, 1):
            os.environ["UNIT_WGRAD_LOOP"] = str(loop)
            res[loop].append(timed(fn))
            if r == 0:
                outs[loop] = check()
    same = all(torch.equal(a, b) for a, b in zip(outs[0], outs[1]))
    m0, m1 = statistics.median(res[0]), statistics.median(res[1])
    print(f"{name:26s} loop 0: {m0:8.1f} us {flops / m0 / 1e6:6.0f} TF | loop 1: {m1:8.1f} us {flops / m1 / 1e6:6.0f} TF | {100 * (m1 / m0 - 1):+5.1f} % | slabs equal {same}")
    print("    loop 0 rounds: " + " ".join(f"{v:.1f}" for v in res[0]))
    print("    loop 1 rounds: " + " ".join(f"{v:.1f}" for v in res[1]))


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    dev = torch.device("cuda:0")
    print("default loop:", o.lib().unit_wgrad256_loop(), " build", __import__("unit_amd")._lib.build_hash() if not os.environ.get("UNIT_HIP_LIB") else os.environ["UNIT_HIP_LIB"])
    for name, n, h, w, c, k, r, st, pad in SH:
        x = torch.randn(n, h, w, c, device=dev).bfloat16()
        oh, ow = o.conv_out_size(h, w, r, r, st, pad)
        dy = torch.randn(n, oh, ow, k, device=dev).bfloat16()
        hold = [None]

        def fn():
            hold[0], _ = o.conv2d_wgrad_partial(x, dy, k, r, r, st, pad, hold[0])

        def check():
            fn()
            torch.cuda.synchronize()
            return [hold[0].clone()]

        ab(name, fn, 2.0 * n * oh * ow * k * r * r * c, rounds, check)
    for which in () if "alone" in sys.argv[2:] else ("res5", "res4", "rpn"):
        items, flops = [], 0.0
        for n, h, w, c, k, r, stride, pad in layers_of(which):
            oh, ow = o.conv_out_size(h, w, r, r, stride, pad)
            x = torch.randn(n, h, w, c, device=dev).bfloat16()
            dy = (torch.randn(n, oh, ow, k, device=dev) * 0.1).bfloat16()
            items.append((x, dy, k, r, r, stride, pad))
            flops += 2.0 * n * oh * ow * k * r * r * c
        gs = [None] * len(items)

        def fn():
            out = o.conv2d_wgrad_group(items, gs)
            for i, (s, _) in enumerate(out):
                gs[i] = s

        def check():
            fn()
            torch.cuda.synchronize()
            return [s.clone() for s in gs]

        ab(f"grouped {which} ({len(items)} layers)", fn, flops, rounds, check)


if __name__ == "__main__":
    main()
