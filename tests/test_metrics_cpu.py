"""Training metrics, host side: the C ABI of the three counting kernels, unit_amd.metrics' arithmetic, the CPU restatement the GPU tests
compare against (tests/metrics_ref.py), and the fixture tests/golden/metrics_golden.npz against the step fixture it must agree with."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import metrics_ref as R  # noqa: E402
from unit_amd import _lib, metrics as M  # noqa: E402

GDIR = os.path.join(os.path.dirname(__file__), "golden")
GOLD = np.load(os.path.join(GDIR, "metrics_golden.npz"))
STEP = np.load(os.path.join(GDIR, "ref_step_golden.npz"))
CASES = ("s1", "s2", "mask", "coco_mask")
NAMES = ("unit_metrics_rpn", "unit_metrics_fastrcnn", "unit_metrics_mask")


def test_prototypes_are_declared_exported_and_replay_safe():
    """pointers and ints only, the stream last: what a recorded call list can carry (no double, no struct by value)"""
    protos, params = _lib.parse_header(), _lib.parse_header_names()
    txt = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER).read(), flags=re.S)
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        restype, argtypes = protos[name]
        assert restype is ctypes.c_int
        assert all(t in (ctypes.c_void_p, ctypes.c_int) for t in argtypes), (name, argtypes)
        assert params[name][-1] == "stream" and argtypes[-1] is ctypes.c_void_p
        assert "m" in params[name] and argtypes[params[name].index("m")] is ctypes.c_void_p
        decl = re.search(name + r"\s*\(([^;]*)\)\s*;", txt).group(1)
        assert "double" not in decl and "struct" not in decl and "Unit" not in decl, decl
        assert len(argtypes) <= _lib.UnitCall.INTS
        assert _lib.enqueues(name)
        assert getattr(so, name) is not None
    assert len(_lib.parse_header()["unit_metrics_fastrcnn"][1]) == 8 and len(protos["unit_metrics_mask"][1]) == 9 and len(protos["unit_metrics_rpn"][1]) == 4


def _vec(**kw):
    v = [0] * M.SIZE
    for k, x in kw.items():
        v[M.SLOTS[k]] = x
    return v


def test_slots_are_three_blocks_of_one_vector():
    assert M.SIZE == 16 and len(set(M.SLOTS.values())) == len(M.SLOTS) and max(M.SLOTS.values()) < M.SIZE
    assert (M.RPN, M.FAST_RCNN, M.MASK) == (0, 5, 10)
    assert [M.SLOTS[k] - M.FAST_RCNN for k in ("roi_instances", "roi_correct", "roi_fg", "roi_fg_correct", "roi_fg_as_bg")] == [0, 1, 2, 3, 4]
    assert [M.SLOTS[k] - M.MASK for k in ("mask_elements", "mask_incorrect", "mask_positive", "mask_false_positive", "mask_false_negative")] == [0, 1, 2, 3, 4]
    assert [M.SLOTS[k] - M.RPN for k in ("rpn_pos", "rpn_neg")] == [0, 1]


def test_scalars_on_hand_made_counts():
    full = _vec(rpn_pos=7, rpn_neg=505, roi_instances=32, roi_correct=20, roi_fg=5, roi_fg_correct=3, roi_fg_as_bg=1, mask_elements=980,
                mask_incorrect=98, mask_positive=400, mask_false_positive=58, mask_false_negative=40)
    d = M.scalars(full, 2)
    assert d == {"rpn/num_pos_anchors": 3.5, "rpn/num_neg_anchors": 252.5, "roi_head/num_fg_samples": 2.5, "roi_head/num_bg_samples": 13.5,
                 "fast_rcnn/cls_accuracy": 20 / 32, "fast_rcnn/fg_cls_accuracy": 3 / 5, "fast_rcnn/false_negative": 1 / 5,
                 "mask_rcnn/accuracy": 1 - 98 / 980.0, "mask_rcnn/false_positive": 58 / 580.0, "mask_rcnn/false_negative": 40 / 400.0}
    assert set(d) == set(M.KEYS) and all(type(v) is float for v in d.values())
    # no instances: Detectron2 logs none of the three classifier keys; the sampler's means are zero, not absent
    d = M.scalars(_vec(rpn_pos=1, rpn_neg=2), 1)
    assert d == {"rpn/num_pos_anchors": 1.0, "rpn/num_neg_anchors": 2.0, "roi_head/num_fg_samples": 0.0, "roi_head/num_bg_samples": 0.0}
    # no foreground: cls_accuracy only
    d = M.scalars(_vec(roi_instances=16, roi_correct=16), 1)
    assert d["fast_rcnn/cls_accuracy"] == 1.0 and d["roi_head/num_bg_samples"] == 16.0
    assert "fast_rcnn/fg_cls_accuracy" not in d and "fast_rcnn/false_negative" not in d
    # no mask slots: the three mask keys are absent
    assert not any(k.startswith("mask_rcnn/") for k in M.scalars(_vec(roi_instances=4, roi_fg=4, roi_correct=1, roi_fg_correct=1), 2))
    # mask slots without a positive pixel: Detectron2's max(., 1.0) guards
    d = M.scalars(_vec(mask_elements=196, mask_incorrect=10, mask_false_positive=10), 1)
    assert d["mask_rcnn/false_negative"] == 0.0 and d["mask_rcnn/false_positive"] == 10 / 196.0 and d["mask_rcnn/accuracy"] == 1 - 10 / 196.0
    # ... and all positive
    d = M.scalars(_vec(mask_elements=196, mask_incorrect=6, mask_positive=196, mask_false_negative=6), 1)
    assert d["mask_rcnn/false_positive"] == 0.0 and d["mask_rcnn/false_negative"] == 6 / 196.0
    with pytest.raises(AssertionError):
        M.scalars([0] * 15, 1)


def test_put_scalars_feeds_a_duck_typed_storage():
    class Storage:
        def __init__(self):
            self.got = []

        def put_scalar(self, name, value):
            self.got.append((name, value))
    st = Storage()
    v = _vec(rpn_pos=4, rpn_neg=60, roi_instances=8, roi_correct=2, roi_fg=0)
    d = M.put_scalars(st, v, 2)
    assert dict(st.got) == d == M.scalars(v, 2) and len(st.got) == len(d) == 5


def test_metrics_ref_on_a_hand_computed_case():
    # rpn: two images
    c, s = R.rpn_scalars([torch.tensor([1, 0, -1, 0, 1, 1]), torch.tensor([-1, -1, 0, 0, 0, 1])])
    assert c == [4, 5] and s == {"rpn/num_pos_anchors": 2.0, "rpn/num_neg_anchors": 2.5}
    # sampler: K = 3, background = 3
    c, s = R.roi_head_scalars([torch.tensor([0, 2, 3, 3]), torch.tensor([3, 3, 3, 1])], 3)
    assert c == [3, 5] and s == {"roi_head/num_fg_samples": 1.5, "roi_head/num_bg_samples": 2.5}
    # classifier: K = 2 (+ background). argmax: row0 -> 1, row1 -> 2 (bg), row2 -> 0 (tie: first), row3 -> 1 (NaN wins), row4 -> 2
    nan = float("nan")
    lg = torch.tensor([[0.1, 0.9, 0.0], [0.0, 0.1, 0.5], [0.7, 0.7, 0.7], [5.0, nan, 9.0], [-1.0, -2.0, 3.0]])
    gt = torch.tensor([1, 0, 0, 1, 2])
    c, s = R.log_accuracy(lg, gt)
    assert c == [5, 4, 4, 3, 1]
    assert s == {"fast_rcnn/cls_accuracy": 0.8, "fast_rcnn/fg_cls_accuracy": 0.75, "fast_rcnn/false_negative": 0.25}
    assert R.fastrcnn_counts_with_empty_slots(torch.cat([lg, lg[:1]]), torch.tensor([1, 0, 0, 1, 2, -1], dtype=torch.int32)) == c
    assert R.log_accuracy(lg[:0], gt[:0]) == ([0, 0, 0, 0, 0], {})
    # mask: one slot, K = 2, 2x2; gt class 1. pred = [[1, 0], [0, 1]] (0.0 and -0.0 are not > 0), target [[1, 1], [0, 0]]
    pl = torch.zeros(1, 2, 2, 2)
    pl[0, 1] = torch.tensor([[0.3, 0.0], [-0.0, 2.0]])
    pl[0, 0] = 9.0
    c, s = R.mask_scalars(pl, torch.tensor([1]), torch.tensor([[[True, True], [False, False]]]))
    assert c == [4, 2, 2, 1, 1] and s == {"mask_rcnn/accuracy": 0.5, "mask_rcnn/false_positive": 0.5, "mask_rcnn/false_negative": 0.5}
    # the same slot in the kernels' layout: [S][P][P][4][ldk], tap = (Y&1)*2 + (X&1)
    lay = torch.zeros(4, 8)
    lay[:, 1] = torch.tensor([0.3, 0.0, -0.0, 2.0])
    lay[:, 0] = 9.0
    tg = torch.tensor([[[1, 1], [0, 0]]], dtype=torch.uint8)
    assert R.mask_counts_from_layout(lay, 2, 8, torch.tensor([1], dtype=torch.int32), tg) == c
    assert R.mask_counts_from_layout(lay, 2, 8, torch.tensor([2], dtype=torch.int32), tg) == [0, 0, 0, 0, 0]
    assert R.mask_scalars(pl[:0], torch.tensor([], dtype=torch.long), tg[:0]) == ([0, 0, 0, 0, 0], {})


@pytest.mark.parametrize("name", CASES)
def test_fixture_agrees_with_the_step_fixture(name):
    """the recorded scalars against what ref_step_golden.npz (written by another generator run) holds of the same step: anchor labels
    and sampled RoI classes"""
    counts = GOLD[f"{name}/counts"]
    n = int(GOLD[f"{name}/n_images"])
    got = dict(zip([str(k) for k in GOLD[f"{name}/keys"]], GOLD[f"{name}/values"].tolist()))
    lab = STEP[f"{name}/anchor_labels"]
    assert lab.shape[0] == n
    c, s = R.rpn_scalars([torch.from_numpy(x) for x in lab])
    assert [int(counts[M.SLOTS["rpn_pos"]]), int(counts[M.SLOTS["rpn_neg"]])] == c
    assert got["rpn/num_pos_anchors"] == s["rpn/num_pos_anchors"] and got["rpn/num_neg_anchors"] == s["rpn/num_neg_anchors"]
    K = 80 if name.startswith("coco") else 20
    c, s = R.roi_head_scalars([torch.from_numpy(STEP[f"{name}/roi_classes{i}"]) for i in range(n)], K)
    assert int(counts[M.SLOTS["roi_fg"]]) == c[0] and int(counts[M.SLOTS["roi_instances"]]) - int(counts[M.SLOTS["roi_fg"]]) == c[1]
    assert got["roi_head/num_fg_samples"] == s["roi_head/num_fg_samples"] and got["roi_head/num_bg_samples"] == s["roi_head/num_bg_samples"]
    # the scalars are the counts' ratios, and the undecided counts respect the generator's cap
    assert M.scalars(counts.tolist(), n) == got
    assert ("mask_rcnn/accuracy" in got) == ("mask" in name)
    assert int(GOLD[f"{name}/undecided_rows"]) <= 0.01 * int(GOLD[f"{name}/rows"])
    assert int(GOLD[f"{name}/undecided_elements"]) <= 0.01 * int(GOLD[f"{name}/elements"])
    assert int(GOLD[f"{name}/rows"]) == int(counts[M.SLOTS["roi_instances"]]) and int(GOLD[f"{name}/elements"]) == int(counts[M.SLOTS["mask_elements"]])


def test_fixture_classifier_counts_say_something():
    """a step test against all-zero hit counts could not fail: every case has hits and misses, and one case has both a foreground hit
    and a foreground row called background (metrics_ref.CLS_BIAS_SHIFT sees to it; the generator asserts the same)"""
    sl = M.SLOTS
    for name in CASES:
        c = GOLD[f"{name}/counts"]
        assert 0 < c[sl["roi_correct"]] < c[sl["roi_instances"]], name
    assert any(GOLD[f"{n}/counts"][sl["roi_fg_correct"]] > 0 and GOLD[f"{n}/counts"][sl["roi_fg_as_bg"]] > 0 for n in CASES)
    assert set(R.CLS_BIAS_SHIFT) >= set(CASES)


@pytest.mark.skipif(not os.path.isdir("/root/reference/modeling"), reason="the reference tree exists only in the authoring container")
def test_generator_reproduces_the_committed_fixture(tmp_path):
    out = str(tmp_path / "regen")
    r = subprocess.run([sys.executable, os.path.join(GDIR, "gen_metrics_golden.py"), out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    new = np.load(os.path.join(out, "metrics_golden.npz"))
    assert sorted(new.files) == sorted(GOLD.files)
    for k in GOLD.files:
        a, b = new[k], GOLD[k]
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), k          # ratios of integer counts: exact
