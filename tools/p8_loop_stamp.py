"""Where a k-tile of the 256x256 forward tile (csrc/conv_igemm256p8.hip, RM schedule) spends its cycles: reads the s_memtime stamps of the
diagnostic build (-DUNIT_EPI_STAMP; tools/p8_loop_stamp.sh builds it and runs this) for the kernel's loop schedules on three Res5 launches
issued alone: the 3x3 512 -> 512 on 1024 RoIs (position-class tiles), the pointwise 2048 -> 512 and the pointwise 512 -> 2048 + residual (both
persistent). Per wave group (wave 0 / wave 4): the eight barrier intervals of the middle k-tile (L = load section, M = MFMA section of phases
0-3; each includes the wait at the barrier that closes it), their sum, and the loop's cycles per k-tile. Medians over the stamped workgroups.

What an interval holds (per wave; the same in every schedule unless the schedule's line in conv_igemm256p8.hip says otherwise):
  L0  2 pieces X1(t+1), the k-tile's offsets (scalar), barrier      M0  16 MFMA, 4 ds_read_b128 (W1), lgkmcnt(0), barrier
  L1  2 pieces X0(t+2), barrier                                     M1  16 MFMA, 8 ds_read_b128 (X1), lgkmcnt(0), barrier
  L2  2 pieces W0(t+2), vmcnt(4), barrier                           M2  16 MFMA, barrier
  L3  2 pieces W1(t+2), barrier                                     M3  16 MFMA, 12 ds_read_b128 (W0, X0 of t+1), lgkmcnt(0), barrier

  python tools/p8_loop_stamp.py [variant ...]      variants of unit_conv2d_fwd_big; default: 13 (the first loop) and 0 (the production loop)"""
import ctypes
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from unit_amd import ops as o, _lib

L = _lib.lib()
L.unit_debug_read_loop_stamps.argtypes = [ctypes.c_void_p]
buf = (ctypes.c_ulonglong * (64 * 16))()
NAMES = ["L0", "M0", "L1", "M1", "L2", "M2", "L3", "M3"]
VARIANTS = [int(a) for a in sys.argv[1:]] or [13, 0]


def big(x, w, k, r, pad, residual, variant):
    n, h, wd, c = x.shape
    oh, ow = o.conv_out_size(h, wd, r, r, 1, pad)
    y = torch.empty((n, oh, ow, k), dtype=x.dtype, device=x.device)
    o.check(L.unit_conv2d_fwd_big(o._p(x), o._p(w), o._p(y), None, o._p(residual), None, o.dt(x.dtype), n, h, wd, c, k, r, r, 1, pad, oh, ow, k, 1, oh, ow, 1,
                                  variant, o._s()), "unit_conv2d_fwd_big")
    return y


def run(name, fn, reps=8):
    for v in VARIANTS:
        for _ in range(reps):
            fn(v)
        torch.cuda.synchronize()
        L.unit_debug_read_loop_stamps(buf)
        rows = [list(buf[i * 16:(i + 1) * 16]) for i in range(64)]
        rows = [r for r in rows if r[13] >= 4 and r[9] and r[10]]
        d = lambda a, b: (a - b) & 0xFFFFFFFF          # the stamps are the low 32 bits of s_memtime
        for grp in (0, 1):
            rr = [r for r in rows if (r[15] >> 2) == grp]
            if not rr:
                print(f"{name} variant {v} group {grp}: no stamps")
                continue
            med = lambda f: statistics.median(f(r) for r in rr)
            iv = [med(lambda r, i=i: d(r[i + 1], r[i])) for i in range(8)]
            print(f"{name:24s} variant {v:2d} group {grp} ({len(rr):2d} wg, {int(med(lambda r: r[13])):3d} k-tiles) | " +
                  " ".join(f"{n} {int(x):4d}" for n, x in zip(NAMES, iv)) +
                  f" | k-tile {int(sum(iv)):5d} | loop/k-tiles {med(lambda r: d(r[10], r[9]) / r[13]):7.0f}")


dev = "cuda"
x3 = torch.randn(1024, 7, 7, 512, device=dev).bfloat16(); w3 = (torch.randn(512, 3, 3, 512, device=dev) * 0.05).bfloat16()
run("3x3 512->512 pos-class", lambda v: big(x3, w3, 512, 3, 1, None, v))
x1 = torch.randn(1024, 7, 7, 2048, device=dev).bfloat16(); w1 = (torch.randn(512, 1, 1, 2048, device=dev) * 0.03).bfloat16()
run("1x1 2048->512 pers", lambda v: big(x1, w1, 512, 1, 0, None, v))
x2 = torch.randn(1024, 7, 7, 512, device=dev).bfloat16(); w2 = (torch.randn(2048, 1, 1, 512, device=dev) * 0.05).bfloat16()
res = torch.randn(1024, 7, 7, 2048, device=dev).bfloat16()
run("1x1 512->2048 +res pers", lambda v: big(x2, w2, 2048, 1, 0, res, v))
