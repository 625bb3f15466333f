"""What the forward / dgrad conv entries answer BEFORE they launch -- every argument check, every "unsupported" return and the empty problems --
as status and unit_last_error() text through the C ABI, checked without a GPU against what the library answered BEFORE the checks and the fill
of the kernels' argument block were gathered into one function (csrc/conv_fwd_host.h: conv_core_fill).

tests/golden/conv_args_golden.json was written at the parent commit of that change, with that commit's library built, by

    import json
    from tests import test_conv_args_cpu as t
    json.dump(t.measure(), open(t.GOLDEN, "w"), indent=1)

`measure()` below only asks the library. Pointers are made-up 16-byte-aligned integers: no row reaches a launch, so they are never read (a row
that answered -2, a launch error, would have reached one and does not belong in the table). Every row breaks exactly ONE rule, so the order of
the checks cannot change its answer. Re-record only when an answer is MEANT to change."""
import ctypes
import json
import os

from unit_amd import _lib, ops

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_args_golden.json")

X, W, Y, X1, Y1, MASK, BITS, POOL = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000, 0x80000
PLAIN = ("fwd", "mid", "big", "x3s")
# base geometry: N = 2, H = W = 9, C = 64, K = 128, 1x1, stride 1, no padding, ldy = K, plain output, bf16; `code` = tile_cfg / tile / variant
BASE = dict(x=X, w=W, y=Y, mask=None, mask_c=0, in_dt=ops.BF16, out_dt=ops.BF16, n=2, h=9, wd=9, c=64, k=128, r=1, stride=1, pad=0, ldy=None,
            doh=0, oy_mul=1, ohf=None, code=0, segs=3, kernel=None, second=None)
SECOND = dict(x=X1, y=Y1, n=1, h=9, wd=9, ohf=9, owf=9)
HUGE = dict(n=4096, h=64, wd=64, c=256)          # 8 GiB of bf16 input


def _common(entry):
    """the rejections every plain entry shares"""
    c_bad = [("C=12 bf16", dict(c=12)), ("C=6 fp32", dict(c=6, in_dt=ops.F32, out_dt=ops.F32))] if entry == "fwd" else [("C=96", dict(c=96))]
    rows = c_bad + [("ldy=K+2", dict(ldy=130)), ("ldy=K-4", dict(ldy=124)), ("OH off by one", dict(doh=1)), ("oy_mul=2, OHf=OH", dict(oy_mul=2)),
                    ("x misaligned", dict(x=X + 8)), ("w misaligned", dict(w=W + 8)), ("y misaligned", dict(y=Y + 8)), ("4 GiB operand", HUGE),
                    ("N=0", dict(n=0)), ("K=0", dict(k=0))]
    if entry == "x3s":
        rows.append(("ldy=K+4", dict(ldy=132)))
    return [("%s: %s" % (entry, name), entry, kw) for name, kw in rows]


ROWS = [r for e in PLAIN for r in _common(e)] + [
    ("mid: tile 6", "mid", dict(code=6)),
    ("mid: tile 99", "mid", dict(code=99)),
    ("mid: tile -1", "mid", dict(code=-1)),
    ("mid: out dtype 2", "mid", dict(out_dt=2)),
    ("mid: loader/consumer code, fp32 out", "mid", dict(code=142, out_dt=ops.F32)),
    ("mid: code 143", "mid", dict(code=143)),
    ("big: variant 6 on a 9x9 map", "big", dict(code=6)),
    ("big: out dtype 2", "big", dict(out_dt=2)),
    ("fwd: fp32 in, bf16 out", "fwd", dict(in_dt=ops.F32, out_dt=ops.BF16)),
    ("x3s: segs=4", "x3s", dict(segs=4)),
    ("x3s: mask_c < ldy", "x3s", dict(mask=MASK, mask_c=64)),
    ("x3s: tile 3", "x3s", dict(code=3)),
    ("x3s: tile 1142", "x3s", dict(code=1142)),
    ("pair: no second problem", "pair", dict(kernel=0, second=None)),
    ("pair: second with null x", "pair", dict(kernel=0, second=dict(x=None))),
    ("pair: second misaligned", "pair", dict(kernel=0, second=dict(y=Y1 + 8))),
    ("pair: second scatter out of range", "pair", dict(kernel=0, second=dict(ohf=4))),
    ("pair: kernel 1, tile 3", "pair", dict(kernel=1, code=3, second={})),
    ("pair: kernel 1, code 2142", "pair", dict(kernel=1, code=2142, second={})),
    ("pair: kernel 2, variant 4", "pair", dict(kernel=2, code=4, second={})),
    ("pair: kernel 2, fp32 out", "pair", dict(kernel=2, out_dt=ops.F32, second={})),
    ("pair: kernel 5", "pair", dict(kernel=5, second={})),
] + [("pair: kernel %d, K=0" % kn, "pair", dict(kernel=kn, k=0, second={})) for kn in range(5)] + \
    [("pair: kernel %d, N=0 twice" % kn, "pair", dict(kernel=kn, n=0, second=dict(n=0))) for kn in range(5)]

# unit_conv2d_fwd_big_ex: N = 4, 7x7, C = 64, K = 128, 1x1 (tests/test_ops_gpu.py test_conv_ex_rejects_what_it_cannot_do)
EX_BASE = dict(y=Y, relu_bits=None, pool=None, pool_rows=0, n=4, h=7, c=64, k=128, r=1, pad=0, ldy=128, x2=None, c2=0, variant=0)
EX_ROWS = [
    ("big_ex: variant 5", dict(variant=5)),
    ("big_ex: no output", dict(y=None)),
    ("big_ex: pool_rows 7", dict(pool=POOL, pool_rows=7)),
    ("big_ex: ldy=132", dict(ldy=132)),
    ("big_ex: bits with ldy=96", dict(relu_bits=BITS, k=96, ldy=96)),
    ("big_ex: C2=96", dict(x2=X1, c2=96)),
    ("big_ex: x2 with 3x3", dict(x2=X1, c2=64, r=3, pad=1)),
    ("big_ex: empty output", dict(h=1, r=3, pad=0)),
    ("big_ex: N=0", dict(n=0)),
    ("big_ex: K=0", dict(k=0, ldy=0)),
]


def _answer(status):
    msg = _lib.lib().unit_last_error() if status != 0 else None
    return [status, msg.decode() if msg else ""]


def _call(entry, kw):
    l = _lib.lib()
    a = dict(BASE)
    a.update(kw)
    oh, ow = ops.conv_out_size(a["h"], a["wd"], a["r"], a["r"], a["stride"], a["pad"])
    oh += a["doh"]
    ldy = a["k"] if a["ldy"] is None else a["ldy"]
    ohf = oh if a["ohf"] is None else a["ohf"]
    geo = (a["n"], a["h"], a["wd"], a["c"], a["k"], a["r"], a["r"], a["stride"], a["pad"], oh, ow, ldy, a["oy_mul"], ohf, ow, 1)
    ptrs = (a["x"], a["w"], a["y"], None, None, a["mask"])
    if entry == "fwd":
        return l.unit_conv2d_fwd(*ptrs, a["in_dt"], a["out_dt"], *geo, a["code"], None)
    if entry == "mid":
        return l.unit_conv2d_fwd_mid(*ptrs, a["out_dt"], *geo, a["code"], None)
    if entry == "big":
        return l.unit_conv2d_fwd_big(*ptrs, a["out_dt"], *geo, a["code"], None)
    if entry == "x3s":
        return l.unit_conv2d_fwd_x3s(*ptrs, a["mask_c"], *geo, a["code"], a["segs"], None)
    assert entry == "pair"
    sec = None
    if a["second"] is not None:
        s = dict(SECOND)
        s.update(a["second"])
        sec = ops.ConvSecond()
        sec.x, sec.y, sec.residual, sec.mask_ref = s["x"], s["y"], None, None
        sec.N, sec.H, sec.W, sec.OHf, sec.OWf = s["n"], s["h"], s["wd"], s["ohf"], s["owf"]
    return l.unit_conv2d_fwd_pair(a["kernel"], *ptrs, a["mask_c"], a["in_dt"], a["out_dt"], *geo, a["code"],
                                  None if sec is None else ctypes.byref(sec), None)


def _call_ex(kw):
    a = dict(EX_BASE)
    a.update(kw)
    return _lib.lib().unit_conv2d_fwd_big_ex(X, W, a["y"], None, None, None, a["relu_bits"], a["pool"], a["pool_rows"], a["n"], a["h"], a["h"], a["c"],
                                             a["k"], a["r"], a["r"], a["pad"], a["ldy"], 0, a["x2"], a["c2"], a["variant"], None)


def measure():
    out = {}
    for name, entry, kw in ROWS:
        out[name] = _answer(_call(entry, kw))
    for name, kw in EX_ROWS:
        out[name] = _answer(_call_ex(kw))
    return out


def test_answers_match_the_recorded_ones():
    with open(GOLDEN) as f:
        want = json.load(f)
    names = [r[0] for r in ROWS] + [r[0] for r in EX_ROWS]
    assert len(set(names)) == len(names) and sorted(want) == sorted(names)
    # the recorded table: no row reached a launch, and every plain entry is seen accepting, rejecting and declining
    assert all(v[0] != -2 for v in want.values())
    for entry in PLAIN:
        seen = {v[0] for name, v in want.items() if name.startswith(entry + ":")}
        assert {0, -1, -4} <= seen, (entry, seen)
    assert all((v[0] == 0) == (v[1] == "") for v in want.values())
    got = measure()
    for name in names:
        assert got[name] == want[name], name
