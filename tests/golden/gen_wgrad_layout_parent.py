"""Writes tests/golden/wgrad_layout_parent.npz: what the host side of the grouped weight-gradient launch decides -- the split plan
(unit_conv2d_wgrad_group_plan) and the unit tables (unit_conv2d_wgrad_group_layout: 9 ints per unit) -- taken on the commit BEFORE that host
side was split into named pieces (no GPU needed: `python tests/golden/gen_wgrad_layout_parent.py [output path]`, on that commit).
tests/test_wgrad_layout_parent_cpu.py imports this file for record() and compares a fresh run with the fixture, entry by entry;
tests/test_wgrad_layout_cpu.py imports it for the problem lists.

Per (list, hint): the (kind, splits) pairs of the problems; per (list, hint, mode): the layout rows. A mode is (UNIT_WGRAD_GANG, UNIT_WGRAD_DEAL),
None = unset. Every (list, mode) is asked twice in a row (the second call is the cache hit wherever tables are cached) and the first list
once more at the end (its cache entry is gone by then): record() asserts that these repeats are equal, and that the lists reach what they were
chosen for -- chunked units, both tile kinds in one call, a second launch forced by the unit table, the "unit by unit" fallback of both
dealers, an XCD with all its 24 entries taken. Per refusal: (status, unit_last_error())."""
import collections
import contextlib
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "wgrad_layout_parent.npz")
MODES = ((None, None), (0, None), (1, None), (2, 0), (0, 1), (1, 0))
SMALL_3X3 = (64, 7, 7, 256, 256, 3, 1, 1)          # 9 tiles of 256, in-map contraction: 9 units per split
# lists whose plan is overwritten to reach the packing limits: {name: (layers, kind or None, splits)}
FORCED = {"full": (20, None, 1),          # 180 units in one launch
          "full2": (11, None, 2),         # 198 units: the unit table (8 x 24) forces a second launch
          "tight": (1, 2, 21)}            # 189 of the 192 table entries from one layer
CASES = (("res5", 0), ("res5", 4), ("res4", 0), ("res4", 3), ("res3", 0), ("long", 0), ("chunk2", 0), ("chunk1", 0), ("mixed", 0),
         ("full", 0), ("full2", 0), ("tight", 0))
U = collections.namedtuple("U", "launch kind xcd start tiles prob tap split tile0")


def layers_of(which):
    """[(N, H, W, C, K, R = S, stride, pad)]"""
    L = []
    if which == "res5":       # one Res5 head on 1024 RoIs: block 0 (stride 2 from 14x14) + 2 identity blocks
        n = 1024
        L += [(n, 14, 14, 1024, 512, 1, 2, 0), (n, 7, 7, 512, 512, 3, 1, 1), (n, 7, 7, 512, 2048, 1, 1, 0), (n, 14, 14, 1024, 2048, 1, 2, 0)]
        for _ in range(2):
            L += [(n, 7, 7, 2048, 512, 1, 1, 0), (n, 7, 7, 512, 512, 3, 1, 1), (n, 7, 7, 512, 2048, 1, 1, 0)]
    elif which == "res4":     # a six-block gradient bucket of res4 on four 600x1000 images
        for _ in range(6):
            L += [(4, 38, 63, 1024, 256, 1, 1, 0), (4, 38, 63, 256, 256, 3, 1, 1), (4, 38, 63, 256, 1024, 1, 1, 0)]
    elif which == "long":     # more layers than one launch holds (WG_GROUP_MAX_PROBLEMS = 20)
        for _ in range(9):
            L += [(4, 38, 63, 1024, 256, 1, 1, 0), (4, 38, 63, 256, 256, 3, 1, 1), (4, 38, 63, 256, 1024, 1, 1, 0)]
    elif which == "res3":     # 128-wide tiles, and one 256 -> 512 shortcut that joins them
        L += [(4, 150, 250, 256, 128, 1, 2, 0), (4, 75, 125, 128, 128, 3, 1, 1), (4, 75, 125, 128, 512, 1, 1, 0), (4, 150, 250, 256, 512, 1, 2, 0)]
        for _ in range(3):
            L += [(4, 75, 125, 512, 128, 1, 1, 0), (4, 75, 125, 128, 128, 3, 1, 1), (4, 75, 125, 128, 512, 1, 1, 0)]
    elif which == "chunk2":   # 64 tiles of 256 in the pointwise layer: its units are cut in chunks, tile0 > 0
        L += [(64, 7, 7, 2048, 2048, 1, 1, 0), (64, 7, 7, 512, 512, 3, 1, 1)]
    elif which == "chunk1":   # 81 tiles of 128: chunked as well
        L += [(1, 20, 20, 384, 384, 3, 1, 1), (1, 20, 20, 128, 128, 1, 1, 0)]
    elif which == "mixed":    # both tile kinds in one call
        L += layers_of("res4") + layers_of("res3")
    else:
        L += [SMALL_3X3] * FORCED[which][0]
    return L


def _unit():
    root = os.path.dirname(os.path.dirname(HERE))
    if root not in sys.path:
        sys.path.insert(0, root)
    from unit_amd import _lib, ops
    return _lib.lib(), ops


def problems(L):
    """the ctypes problem array of a layer list: aligned pointers that the layout call never reads; splits / kind still 0"""
    _, ops = _unit()
    pr = (ops.WgradProblem * len(L))()
    for q, (n, h, w, c, k, r, stride, pad) in zip(pr, L):
        oh, ow = ops.conv_out_size(h, w, r, r, stride, pad)
        q.x, q.dy, q.partial = 0x10000, 0x20000, 0x30000
        q.N, q.H, q.W, q.C, q.K, q.R, q.S, q.stride, q.pad, q.OH, q.OW, q.ldy = n, h, w, c, k, r, r, stride, pad, oh, ow, k
    return pr


def planned(which, hint=0):
    lib, _ = _unit()
    pr = problems(layers_of(which))
    assert lib.unit_conv2d_wgrad_group_plan(pr, len(pr), hint) == 0
    if which in FORCED:
        _, kind, splits = FORCED[which]
        for q in pr:
            q.splits = splits
            if kind is not None:
                q.kind = kind
    return pr


def layout_call(pr, cap=4096):
    """-> (status, [U])"""
    lib, _ = _unit()
    rows = ctypes.c_int(0)
    buf = (ctypes.c_int * (9 * max(cap, 1)))()
    st = lib.unit_conv2d_wgrad_group_layout(pr, len(pr), buf, cap, ctypes.byref(rows))
    return st, [U(*buf[9 * i:9 * i + 9]) for i in range(rows.value if st == 0 else 0)]


@contextlib.contextmanager
def mode_env(mode):
    names = ("UNIT_WGRAD_GANG", "UNIT_WGRAD_DEAL")
    old = [os.environ.get(k) for k in names]
    try:
        for k, v in zip(names, mode):
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        yield
    finally:
        for k, v in zip(names, old):
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _check_reached(which, mode, pr, units):
    """the branches a list was chosen for"""
    per_launch = collections.Counter(u.launch for u in units)
    per_xcd = collections.Counter((u.launch, u.xcd) for u in units)
    if which == "chunk2":
        assert any(u.kind == 2 and u.tile0 > 0 for u in units)
    if which == "chunk1":
        assert all(u.kind == 1 for u in units) and any(u.tile0 > 0 for u in units)
    if which == "mixed":
        assert {u.kind for u in units} == {1, 2}
        assert max(u.launch for u in units if u.kind == 2) < min(u.launch for u in units if u.kind == 1)          # the 256-tile grid first
    if which == "long":
        assert len({u.launch for u in units if u.kind == 2}) >= 2
    if which == "res5":
        assert any(u.tap > 0 for u in units)
    if which == "full":
        assert dict(per_launch) == {0: 180}
        if mode[0] == 1:          # all nine taps of a split are one gang: 16 gangs fit whole, the other 4 go unit by unit (in either dealer)
            where = collections.defaultdict(set)
            for u in units:
                where[(u.prob, u.split)].add(u.xcd)
            assert sum(len(x) > 1 for x in where.values()) == 4
            assert max(per_xcd.values()) == 24
    if which == "full2":
        assert len(units) == 198 and len(per_launch) == 2 and max(per_launch.values()) <= 192
    if which == "tight":
        assert dict(per_launch) == {0: 189} and max(per_xcd.values()) == 24


def _refusals():
    """[(name, problem array, layout_rows)]: each is refused by the layout call (`kind 0`: such a problem belongs to no grid)"""
    def one(layer=(64, 7, 7, 256, 256, 1, 1, 0), kind=2, splits=2, **kw):
        pr = problems([layer])
        pr[0].kind, pr[0].splits = kind, splits
        for k, v in kw.items():
            setattr(pr[0], k, v)
        return pr
    return [("splits 0", one(splits=0), 4096), ("splits 128", one(splits=128), 4096), ("misaligned x", one(x=0x10008), 4096),
            ("x_pitch < C", one(x_pitch=128), 4096), ("N = 0", one(N=0), 4096), ("kind 0", one(kind=0), 4096),
            ("kind 2, C = 384", one(layer=(64, 7, 7, 384, 384, 1, 1, 0)), 4096), ("tight, splits 22", one(layer=SMALL_3X3, splits=22), 4096),
            ("one row short", planned("tight"), 188)]


def record():
    """-> {key: array}: `plan:<list>:<hint>` [n, 2], `rows:<list>:<hint>:<mode index>` [units, 9], refusal_names / _status / _messages"""
    lib, _ = _unit()
    out = {}

    def rows_of(which, hint, mode):
        with mode_env(mode):
            pr = planned(which, hint)
            st, units = layout_call(pr)
            assert st == 0 and units, (which, hint, mode)
        return pr, units

    for which, hint in CASES:
        pr = planned(which, hint)
        out[f"plan:{which}:{hint}"] = np.array([(q.kind, q.splits) for q in pr], dtype=np.int32)
        for mi, mode in enumerate(MODES):
            pr, units = rows_of(which, hint, mode)
            assert rows_of(which, hint, mode)[1] == units, (which, hint, mode)          # (the cache hit, where tables are cached)
            _check_reached(which, mode, pr, units)
            out[f"rows:{which}:{hint}:{mi}"] = np.array(units, dtype=np.int32).reshape(-1, 9)
    which, hint = CASES[0]          # ... and after its cache entry has been replaced
    for mi, mode in enumerate(MODES):
        again = np.array(rows_of(which, hint, mode)[1], dtype=np.int32).reshape(-1, 9)
        assert np.array_equal(again, out[f"rows:{which}:{hint}:{mi}"]), mode
    names, status, messages = [], [], []
    with mode_env((None, None)):
        for name, pr, cap in _refusals():
            st, _ = layout_call(pr, cap)
            msg = lib.unit_last_error() if st != 0 else b""
            assert (st == 0) == (name == "kind 0"), (name, st)
            names.append(name); status.append(st); messages.append((msg or b"").decode())
    out["refusal_names"] = np.array(names, dtype=np.str_)
    out["refusal_status"] = np.array(status, dtype=np.int32)
    out["refusal_messages"] = np.array(messages, dtype=np.str_)
    return out


def main(path=OUT):
    out = record()
    np.savez_compressed(path, **out)
    for n, s, m in zip(out["refusal_names"], out["refusal_status"], out["refusal_messages"]):
        print(f"{n}: {s} {m!r}")
    print(f"{len(CASES)} lists x {len(MODES)} modes, {sum(len(v) for k, v in out.items() if k.startswith('rows:'))} units -> {path}")


if __name__ == "__main__":
    main(*sys.argv[1:])
