"""The forward / dgrad conv launches, bit for bit against the library BEFORE their host side (argument block, checks, launcher tails; the Python
geometry of ops.conv2d / conv2d_x3 / conv2d_pair) was gathered into csrc/conv_args.h and csrc/conv_fwd_host.h: every output tensor of every row of
ROWS is hashed (sha256 of its bytes) and compared with tests/golden/conv_frozen_golden.json.

The golden file was written on an MI355X at the parent commit of that change, with that commit's library built and THIS file copied into its
tests/, by

    import json
    from tests import test_conv_frozen_gpu as t
    json.dump(t.measure(), open(t.GOLDEN, "w"), indent=1)

These kernels use no atomics and a fixed summation order, so the hashes are exact. A mismatch is a change of behaviour to find and fix, never a
reason to re-record. Inputs come from numpy.random.RandomState(seed of the row); every row that can runs with bias, residual, mask_ref and relu
all on ("full"), one row per entry with none ("bare"). The shapes are the smallest that cross the kernels' edges: A partial tiles in M and K and
ldy = 40, B M = 2970 (more than one 256-row tile per XCD), C position-class tiles, D stride 2 and its dgrad form (1x1 scattered with oy_mul = 2
into a zeroed map), E the loader / consumer tiles' case of tests/test_ops_gpu.py, F fp32 in and out."""
import hashlib
import json
import os
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_frozen_golden.json")

# (n, h, w, c, k, r, stride, pad)
A = (2, 9, 9, 64, 40, 1, 1, 0)
B = (3, 30, 33, 256, 256, 3, 1, 1)
C = (70, 7, 7, 64, 512, 3, 1, 1)
D = (2, 19, 23, 64, 320, 1, 2, 0)
E = (3, 30, 33, 256, 200, 3, 1, 1)
F = (2, 13, 17, 16, 24, 3, 1, 1)
HALO = (37, 7, 7, 192, 300, 3, 1, 1)
EX = (37, 7, 7, 128, 256, 1, 1, 0)
PAIR = ((1, 19, 23), (3, 11, 31), 64, 320, 3, 1, 1)
SHAPES = dict(A=A, B=B, C=C, D=D, E=E, F=F, HALO=HALO)
BF, F32 = torch.bfloat16, torch.float32


def ops():
    from unit_amd import ops as o
    return o


def _rows():
    rows = {}
    # unit_conv2d_fwd, tile_cfg 0..4
    for t in range(5):
        rows["fwd F fp32 tile_cfg %d" % t] = ("plain", "fwd", "F", F32, F32, t, True)
        rows["fwd A bf16 tile_cfg %d" % t] = ("plain", "fwd", "A", BF, BF, t, True)
        rows["fwd A bf16->fp32 tile_cfg %d" % t] = ("plain", "fwd", "A", BF, F32, t, True)
    rows["fwd A bf16 bare"] = ("plain", "fwd", "A", BF, BF, 0, False)
    # unit_conv2d_fwd_mid: the 4-wave tiles, the loader / consumer codes
    for t in range(6):
        for s in "AB":
            for od in (BF, F32):
                rows["mid %s tile %d %s" % (s, t, "bf16" if od == BF else "fp32")] = ("plain", "mid", s, BF, od, t, True)
    for code in (142, 164, 1152, 2152, 4152, 8152):
        rows["mid E code %d" % code] = ("plain", "mid", "E", BF, BF, code, True)
    rows["mid B tile 0 bare"] = ("plain", "mid", "B", BF, BF, 0, False)
    # unit_conv2d_fwd_big
    for v in (1, 2, 3, 4, 7, 8, 9, 10, 11, 12):
        for s in "BC":
            rows["big %s variant %d bf16" % (s, v)] = ("plain", "big", s, BF, BF, v, True)
            if v in (4, 8):
                rows["big %s variant %d fp32" % (s, v)] = ("plain", "big", s, BF, F32, v, True)
    rows["big HALO variant 6"] = ("plain", "big", "HALO", BF, BF, 6, True)
    rows["big B variant 0 bare"] = ("plain", "big", "B", BF, BF, 0, False)
    # D and its dgrad form in every family (through ops.conv2d: the policy for tile_cfg 0, ops.TILE_CFG otherwise)
    for cfg in (0, 1, 8, 16):
        rows["conv2d D tile_cfg %d" % cfg] = ("conv2d", cfg, False)
        rows["conv2d D dgrad tile_cfg %d" % cfg] = ("conv2d", cfg, True)
    # ops.conv2d_ex
    for v in (8, 11):
        rows["ex variant %d bits + pool" % v] = ("ex", v, "bits")
        rows["ex variant %d mask_bits" % v] = ("ex", v, "mask")
        rows["ex variant %d x2" % v] = ("ex", v, "x2")
    rows["ex bare"] = ("ex", 0, "bare")
    # ops.conv2d_x3
    for t in (-1, 0, 1, 2, 152):
        rows["x3 B tile %d" % t] = ("x3", "B", t, 3, True)
    for t in (-1, 0):
        rows["x3 B tile %d, 2 segments" % t] = ("x3", "B", t, 2, True)
    rows["x3 C tile -1"] = ("x3", "C", -1, 3, True)
    rows["x3 B tile -1 bare"] = ("x3", "B", -1, 3, False)
    # ops.conv2d_pair
    for force in ((0, 0), (1, 0), (1, 1), (1, 152), (2, 0), (3, -1), (3, 1), (4, -1)):
        rows["pair force %d %d" % force] = ("pair", force, True)
    rows["pair force 1 0 bare"] = ("pair", (1, 0), False)
    rows["pair strided scatter"] = ("pair_scatter",)
    return rows


ROWS = _rows()


class Rand:
    def __init__(self, name, dev):
        self.rs, self.dev = np.random.RandomState(zlib.crc32(name.encode()) & 0x7FFFFFFF), dev

    def __call__(self, *shape, dtype=F32, scale=1.0):
        a = (self.rs.random_sample(shape).astype(np.float32) - 0.5) * np.float32(2.0 * scale)
        return torch.from_numpy(a).to(dtype).to(self.dev)


def _digest(t):
    t = t.as_subclass(torch.Tensor).contiguous()
    t = t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()]) if t.dtype != torch.bool else t.to(torch.uint8)
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def _plain(o, rnd, entry, shape, in_dt, out_dt, code, full):
    from unit_amd._lib import check, lib
    n, h, w, c, k, r, stride, pad = SHAPES[shape]
    oh, ow = o.conv_out_size(h, w, r, r, stride, pad)
    ldy = (k + 7) // 8 * 8 if shape == "HALO" else (k + 3) // 4 * 4
    x, wt = rnd(n, h, w, c, dtype=in_dt), rnd(k, r, r, c, dtype=in_dt, scale=1.0 / np.sqrt(c * r * r))
    bias = rnd(k) if full else None
    res = rnd(n, oh, ow, ldy, dtype=out_dt) if full else None
    msk = rnd(n, oh, ow, ldy, dtype=out_dt) if full else None
    y = torch.zeros(n, oh, ow, ldy, dtype=out_dt, device=x.device)
    geo = (n, h, w, c, k, r, r, stride, pad, oh, ow, ldy, 1, oh, ow, int(full), code, o._s())
    ptrs = (o._p(x), o._p(wt), o._p(y), o._p(bias), o._p(res), o._p(msk))
    if entry == "fwd":
        check(lib().unit_conv2d_fwd(*ptrs, o.dt(in_dt), o.dt(out_dt), *geo), "unit_conv2d_fwd")
    elif entry == "mid":
        check(lib().unit_conv2d_fwd_mid(*ptrs, o.dt(out_dt), *geo), "unit_conv2d_fwd_mid")
    else:
        check(lib().unit_conv2d_fwd_big(*ptrs, o.dt(out_dt), *geo), "unit_conv2d_fwd_big")
    return [y]


def _conv2d(o, rnd, cfg, dgrad):
    n, h, w, c, k, r, stride, pad = D
    oh, ow = o.conv_out_size(h, w, r, r, stride, pad)
    if not dgrad:
        x, wt = rnd(n, h, w, c, dtype=BF), rnd(k, 1, 1, c, dtype=BF, scale=1.0 / 8)
        return [o.conv2d(x, wt, k, 1, 1, stride, pad, bias=rnd(k), residual=rnd(n, oh, ow, k, dtype=BF), mask_ref=rnd(n, oh, ow, k, dtype=BF), relu=True,
                         tile_cfg=cfg)]
    dy, wd = rnd(n, oh, ow, k, dtype=BF), rnd(c, 1, 1, k, dtype=BF, scale=1.0 / 18)
    return [o.conv2d(dy, wd, c, 1, 1, 1, 0, mask_ref=rnd(n, h, w, c, dtype=BF), scatter=(2, h, w), tile_cfg=cfg)]


def _ex(o, rnd, variant, what):
    n, h, w, c, k, r, stride, pad = EX
    x, x2 = rnd(n, h, w, c, dtype=BF), rnd(n, h, w, c, dtype=BF)
    wt = rnd(k, 1, 1, 2 * c if what == "x2" else c, dtype=BF, scale=1.0 / 11)
    if what == "bare":
        return [o.conv2d_ex(x, wt, k, 1, 1, variant=variant)[0]]
    bias, res = rnd(k), rnd(n, h, w, k, dtype=BF)
    y, bits, pooled = o.conv2d_ex(x, wt, k, 1, 1, bias=bias, residual=res, relu=True, want_bits=True, pool_rows=h * w, variant=variant,
                                  x2=x2 if what == "x2" else None)
    if what != "mask":
        return [y, bits.unpack(), pooled]
    g, _, _ = o.conv2d_ex(rnd(n, h, w, c, dtype=BF), wt, k, 1, 1, mask_bits=bits, variant=variant)
    return [g]


def _x3(o, rnd, shape, tile, segs, full):
    n, h, w, c, k, r, stride, pad = SHAPES[shape]
    x = o.x3_split(rnd(n, h, w, c))
    if segs == 3:
        wt, _ = o.weight_prep_x3(rnd(k, r, r, c, scale=1.0 / np.sqrt(c * r * r)), None, k, r, r, c, want_dgrad=False)
    else:          # the two-segment copy is the dgrad one: of a [c][r][r][k] layer, it is a [k][r][r][2 c] weight
        _, wt = o.weight_prep_x3(rnd(c, r, r, k, scale=1.0 / np.sqrt(c * r * r)), None, c, r, r, k, want_fwd=False)
        assert wt.shape == (k, r, r, 2 * c)
    kw = dict(bias=rnd(k), residual=o.x3_split(rnd(n, h, w, k)), mask_ref=o.x3_split(rnd(n, h, w, k)), relu=True) if full else {}
    return [o.conv2d_x3(x, wt, k, r, r, stride, pad, tile=tile, **kw)]


def _pair(o, rnd, force, full):
    d0, d1, c, k, r, stride, pad = PAIR
    x3 = force[0] >= 3
    conv = (lambda t: o.x3_split(t)) if x3 else (lambda t: t.to(BF))
    xs = [conv(rnd(n, h, w, c)) for n, h, w in (d0, d1)]
    wt = rnd(k, r, r, c, scale=1.0 / np.sqrt(c * r * r))
    if force[0] == 3:
        wt, _ = o.weight_prep_x3(wt, None, k, r, r, c, want_dgrad=False)
    elif force[0] == 4:
        _, wt = o.weight_prep_x3(rnd(c, r, r, k, scale=1.0 / np.sqrt(c * r * r)), None, c, r, r, k, want_fwd=False)
        assert wt.shape == (k, r, r, 2 * c)
    else:
        wt = wt.to(BF)
    kw = {}
    if full:
        kw = dict(bias=rnd(k), residuals=[conv(rnd(n, h, w, k)) for n, h, w in (d0, d1)], mask_refs=[conv(rnd(n, h, w, k)) for n, h, w in (d0, d1)], relu=True)
    return list(o.conv2d_pair(xs, wt, k, r, r, stride, pad, force=force, **kw))


def _pair_scatter(o, rnd):
    """tests/test_ragged_gpu.py test_pair_launch_strided_scatter: both problems scatter into the zeroed rows of one flat tensor"""
    dims_in = [(2, 76, 101), (2, 92, 139)]
    c, k = 256, 512
    wd = rnd(c, 1, 1, k, dtype=BF, scale=1.0 / 22)
    dys = [rnd(n, (h - 1) // 2 + 1, (w - 1) // 2 + 1, k, dtype=BF) for n, h, w in dims_in]
    out = o.Ragged.zeros(dims_in, c, dys[0])
    o.conv2d_pair(dys, wd, c, 1, 1, 1, 0, outs=out.groups(), scatters=[(2, h, w) for _, h, w in dims_in])
    return [out.flat]


RUN = dict(plain=_plain, conv2d=_conv2d, ex=_ex, x3=_x3, pair=_pair, pair_scatter=_pair_scatter)


def run_row(name, dev):
    row = ROWS[name]
    outs = RUN[row[0]](ops(), Rand(name, dev), *row[1:])
    return [_digest(t) for t in outs]


def measure(dev="cuda:0"):
    assert "UNIT_P8_PERSIST" not in os.environ and "UNIT_X3_REUSE" not in os.environ
    return {name: run_row(name, dev) for name in ROWS}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        want = json.load(f)
    assert sorted(want) == sorted(ROWS)
    return want


@pytest.mark.parametrize("name", list(ROWS))
def test_outputs_are_the_recorded_bytes(dev, golden, monkeypatch, name):
    monkeypatch.delenv("UNIT_P8_PERSIST", raising=False)          # both switches at their defaults; the launchers read them at every launch
    monkeypatch.delenv("UNIT_X3_REUSE", raising=False)
    assert run_row(name, dev) == golden[name]
