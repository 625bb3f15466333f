"""The per-layer decision of the weight gradient -- which kernel family, how many split-M slabs, how large a workspace -- and the grouped
launch's plan, as host arithmetic through the C ABI (csrc/conv_wgrad_host.h: wgrad_select; csrc/conv_wgrad.hip), checked without a GPU against
integers recorded from the library BEFORE the decision was gathered into one function.

tests/golden/wgrad_select_golden.json was written at the parent commit of that change, with that commit's library built, by

    import json
    from tests import test_wgrad_select_cpu as t
    json.dump(t.measure(), open(t.GOLDEN, "w"), indent=1)

`measure()` below only asks the library: the rows of ROWS (one per branch of the decision) through unit_conv2d_wgrad_splits,
unit_conv2d_wgrad_workspace_bytes and unit_conv2d_wgrad_group_supported, and groups of the first 1 / 3 / 10 eligible bf16 rows through
unit_conv2d_wgrad_group_plan with splits_hint 0 and 6. Re-record only when the decision is MEANT to change."""
import json
import os

from unit_amd import _lib, ops

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wgrad_select_golden.json")

# (name, dtype code, N, H, W, C, K, R = S, stride, pad)
ROWS = [
    ("a fp32", ops.F32, 2, 9, 11, 32, 32, 3, 1, 1),
    ("b bf16, C % 128 != 0", ops.BF16, 2, 9, 11, 64, 64, 3, 1, 1),
    ("c ring 128", ops.BF16, 2, 10, 12, 128, 128, 3, 2, 1),
    ("d ring 128, pointwise", ops.BF16, 1, 38, 63, 1024, 256, 1, 1, 0),
    ("e big, M >= 16384, pointwise", ops.BF16, 2, 96, 96, 256, 256, 1, 1, 0),
    ("f big, map > 1024 px", ops.BF16, 2, 96, 96, 256, 256, 3, 1, 1),
    ("g big, 7x7 maps: one spare slab", ops.BF16, 336, 7, 7, 256, 256, 3, 1, 1),
    ("h big, 8192 <= M < 16384, 144 tiles", ops.BF16, 2, 64, 64, 1024, 1024, 3, 1, 1),
    ("i as h, 9 tiles: off the big kernel", ops.BF16, 2, 64, 64, 256, 256, 3, 1, 1),
    ("j M just under 8192", ops.BF16, 2, 64, 63, 1024, 1024, 3, 1, 1),
    ("k res4 1x1 1024->256", ops.BF16, 4, 38, 63, 1024, 256, 1, 1, 0),
    ("k res4 3x3 256->256", ops.BF16, 4, 38, 63, 256, 256, 3, 1, 1),
    ("k res5 3x3 512->512", ops.BF16, 512, 7, 7, 512, 512, 3, 1, 1),
    ("k res5 1x1 2048->512", ops.BF16, 512, 7, 7, 2048, 512, 1, 1, 0),
]
GROUP_SIZES = (1, 3, 10)
GROUP_HINTS = (0, 6)


def _geometry(row):
    _, dtype, n, h, w, c, k, r, stride, pad = row
    oh, ow = ops.conv_out_size(h, w, r, r, stride, pad)
    return dtype, n, h, w, c, k, r, stride, pad, oh, ow


def _plan(rows, hint):
    pr = (ops.WgradProblem * len(rows))()
    for q, row in zip(pr, rows):
        _, n, h, w, c, k, r, stride, pad, oh, ow = _geometry(row)
        q.N, q.H, q.W, q.C, q.K, q.R, q.S, q.stride, q.pad, q.OH, q.OW, q.ldy = n, h, w, c, k, r, r, stride, pad, oh, ow, k
    rc = _lib.lib().unit_conv2d_wgrad_group_plan(pr, len(rows), hint)
    return [rc] + [[q.kind, q.splits] for q in pr]


def measure():
    l = _lib.lib()
    out = {"rows": {}, "plans": {}}
    eligible = []
    for row in ROWS:
        dtype, n, h, w, c, k, r, stride, pad, oh, ow = _geometry(row)
        sup = l.unit_conv2d_wgrad_group_supported(dtype, n, oh, ow, k, r, r, c)
        out["rows"][row[0]] = {"splits": l.unit_conv2d_wgrad_splits(dtype, n, oh, ow, k, r, r, c),
                               "workspace_bytes": l.unit_conv2d_wgrad_workspace_bytes(dtype, n, oh, ow, k, r, r, c),
                               "group_supported": sup}
        if dtype == ops.BF16 and sup:
            eligible.append(row)
    for size in GROUP_SIZES:
        for hint in GROUP_HINTS:
            out["plans"]["first %d, hint %d" % (size, hint)] = _plan(eligible[:size], hint)
    return out


def test_decision_matches_the_recorded_one():
    with open(GOLDEN) as f:
        want = json.load(f)
    got = measure()
    assert sorted(got["rows"]) == sorted(want["rows"]) and len(want["rows"]) == len(ROWS)
    for name in want["rows"]:
        assert got["rows"][name] == want["rows"][name], name
    assert got["plans"] == want["plans"]
    # the table reaches every branch: both dtypes, the three kernel families' eligibility, the spare slab, both M thresholds
    sup = [want["rows"][r[0]]["group_supported"] for r in ROWS]
    assert sup[:3] == [0, 0, 1] and 2 in sup
    assert len(want["plans"]) == len(GROUP_SIZES) * len(GROUP_HINTS) and all(p[0] == 0 for p in want["plans"].values())


def test_workspace_is_splits_times_one_fp32_slab():
    """ops.conv2d_wgrad_partial sizes a part's slabs from the split count alone"""
    l = _lib.lib()
    for row in ROWS:
        dtype, n, h, w, c, k, r, stride, pad, oh, ow = _geometry(row)
        splits = l.unit_conv2d_wgrad_splits(dtype, n, oh, ow, k, r, r, c)
        assert splits >= 1
        assert l.unit_conv2d_wgrad_workspace_bytes(dtype, n, oh, ow, k, r, r, c) == splits * k * r * r * c * 4, row[0]
