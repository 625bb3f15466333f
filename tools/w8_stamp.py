"""Where a 64-pixel step of the 256x256 weight-gradient tile spends its cycles: reads the s_memtime stamps of the diagnostic build
(-DUNIT_W8_STAMP, csrc/conv_wgrad256p8.hip; tools/w8_stamp.sh builds it and runs this) for both loop schedules on two shapes launched alone:
the pointwise 2048 -> 512 and the valid-only 3x3 512 -> 512 on 1024 x 7 x 7. Per wave group (wave 0 / wave 4): the eight barrier intervals of
the middle step (S = staging section, M = MFMA section of phases 0-3; each includes the wait at the barrier that closes it), the loop's
cycles per step, and the tile's fixed cycles in front of and behind the loop. Medians over the stamped workgroups."""
import ctypes
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from unit_amd import ops as o, _lib

L = _lib.lib()
L.unit_debug_read_w8_stamps.argtypes = [ctypes.c_void_p]
buf = (ctypes.c_ulonglong * (64 * 16))()
NAMES = ["S0", "M0", "S1", "M1", "S2", "M2", "S3", "M3"]


def run(name, fn, reps=8):
    for loop in (0, 1):
        os.environ["UNIT_WGRAD_LOOP"] = str(loop)
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        L.unit_debug_read_w8_stamps(buf)
        rows = [list(buf[i * 16:(i + 1) * 16]) for i in range(64)]
        rows = [r for r in rows if r[13] >= 4 and r[9] and r[10]]
        d = lambda a, b: (a - b) & 0xFFFFFFFF          # the stamps are the low 32 bits of s_memtime
        for grp in (0, 1):
            rr = [r for r in rows if (r[15] >> 2) == grp]
            if not rr:
                print(f"{name} loop {loop} group {grp}: no stamps")
                continue
            med = lambda f: statistics.median(f(r) for r in rr)
            iv = [med(lambda r, i=i: d(r[i + 1], r[i])) for i in range(8)]
            print(f"{name:22s} loop {loop} group {grp} ({len(rr):2d} wg, {int(med(lambda r: r[13])):3d} steps) | " +
                  " ".join(f"{n} {int(v):4d}" for n, v in zip(NAMES, iv)) +
                  f" | step {int(sum(iv)):5d} | loop/steps {med(lambda r: d(r[10], r[9]) / r[13]):7.0f} | ramp {int(med(lambda r: d(r[9], r[11]))):6d} | store {int(med(lambda r: d(r[12], r[10]))):6d}")


dev = "cuda"
x = torch.randn(1024, 7, 7, 2048, device=dev).bfloat16(); dy = torch.randn(1024, 7, 7, 512, device=dev).bfloat16()
run("1x1 2048->512", lambda: o.conv2d_wgrad_partial(x, dy, 512, 1, 1, 1, 0))
x3 = torch.randn(1024, 7, 7, 512, device=dev).bfloat16(); dy3 = torch.randn(1024, 7, 7, 512, device=dev).bfloat16()
run("3x3 512->512 valid", lambda: o.conv2d_wgrad_partial(x3, dy3, 512, 3, 3, 1, 1))
run("3x3 512->512 all px", lambda: o.conv2d_wgrad_partial(x3, dy3, 512, 3, 3, 1, 1, variant=3))
