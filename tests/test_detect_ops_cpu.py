"""Preconditions of the exact detection recipe (tests/detect_cases.py), asserted on the CPU reference alone: the GPU parity tests of
test_detect_ops_gpu.py compare decisions bit for bit, and they mean something only if the cases really have candidates, heavy
suppression, ties, every class, more survivors than topk, detections that turn empty after rescaling, and an exact decode."""
import pytest
import torch

import detect_cases as dc
import unit_oracle as orc

CASES = [c[0] for c in dc.SINGLE_CASES] + ["batch_empty", "batch_full"]


def _case(name):
    if name == "batch_empty":
        return dc.batch_case(dc.BATCH_EMPTY_IMAGE)
    if name == "batch_full":
        return dc.batch_case(None)
    return dc.single_case(name)


@pytest.mark.parametrize("name", CASES)
def test_recipe_preconditions(name):
    case = _case(name)
    probs, deltas, props, pcount, image_hw = case["inputs"]
    k, topk, thr = case["k"], case["topk"], case["thresh"]
    cands = dc.candidates(*case["inputs"], thr)
    survivors = dc.ref_detections(*case["inputs"], thr, dc.NMS_THRESH, dc.ALL)
    designed_empty = {1} | ({dc.BATCH_EMPTY_IMAGE} if name == "batch_empty" else set()) if name.startswith("batch") else set()
    for i, ((cb, cs, cc, cr), surv, ref) in enumerate(zip(cands, survivors, case["ref"])):
        n = cs.numel()
        if i in designed_empty:
            assert n == 0 and ref["scores"].numel() == 0
            continue
        assert n > 0
        assert torch.isfinite(cb).all() and bool(ref["valid"].all())
        ns = surv["scores"].numel()
        if int(pcount[i]) > 1:          # (one RoI has nothing to suppress and no room for every tie)
            assert n - ns >= 0.1 * n, (n, ns)                                   # suppression is heavy
            _, mult = torch.unique(cs, return_counts=True)
            assert int(mult[mult > 1].sum()) >= 0.5 * n                        # exact score ties
            assert not bool(ref["nonempty"].all())                             # a kept detection turns empty in detector_postprocess
        assert torch.unique(cc).numel() == k                                   # every class appears
        if name in dc.LARGE_CASES:
            assert ns > topk and ref["scores"].numel() == topk
        # the decode is exact: every decoded coordinate (before clipping) is a multiple of 1/8
        rows = slice(i * props.shape[1], i * props.shape[1] + int(pcount[i]))
        dec = orc.apply_deltas(deltas[rows], props[i, : int(pcount[i])], dc.WEIGHTS) * 8.0
        assert torch.equal(dec, dec.round())
        # and so is the batched_nms class offset: class * (max coordinate + 1) stays a multiple of 1/8 below 2^24 / 8
        assert float(cb.max() + 1) * (k - 1) * 8 < 2 ** 24


def test_batch_shape_and_padding():
    probs, deltas, props, pcount, _ = dc.exact_batch()
    r = dc.BATCH_RCAP
    assert pcount.tolist() == [r, 0, 1, r - 3]
    for i, n in enumerate(pcount.tolist()):
        assert torch.isfinite(probs[i * r: i * r + n]).all() and torch.isnan(probs[i * r + n: (i + 1) * r]).all()
        assert torch.isfinite(deltas[i * r: i * r + n]).all() and torch.isnan(deltas[i * r + n: (i + 1) * r]).all()
        assert torch.isfinite(props[i, :n]).all() and torch.isnan(props[i, n:]).all()
    # the empty image's scores sit AT 3/64: below 0.05, and not above a threshold of exactly 3/64
    empty = probs[dc.BATCH_EMPTY_IMAGE * r: dc.BATCH_EMPTY_IMAGE * r + 1]
    assert bool((empty == 3.0 / 64.0).all())
    for thr in (0.05, 3.0 / 64.0):
        ref = dc.batch_case(dc.BATCH_EMPTY_IMAGE, thr)["ref"]
        assert [d["scores"].numel() for d in ref] == [dc.BATCH_TOPK, 0, 0, dc.BATCH_TOPK]
    assert dc.batch_case(None)["ref"][2]["scores"].numel() > 0          # the one-RoI image detects when its scores are ordinary


def test_nonfinite_reference_drops_whole_rois():
    inp = dc.nonfinite_batch()
    ref = dc.ref_detections(*inp, 0.05, dc.NMS_THRESH, dc.ALL)
    assert sorted((~ref[0]["valid"]).nonzero()[:, 0].tolist()) == sorted(dc.NONFINITE_DROPPED.values())
    assert sorted((~ref[1]["valid"]).nonzero()[:, 0].tolist()) == [5, 14]
    roi0 = set(ref[0]["roi"].tolist())
    assert not roi0 & set(dc.NONFINITE_DROPPED.values())
    # the two controls are finite in the reference, score above the threshold in the affected class and reach the detections
    for row in dc.NONFINITE_KEPT.values():
        hit = (ref[0]["roi"] == row) & (ref[0]["classes"] == dc.NONFINITE_CLASS)
        assert int(hit.sum()) == 1
    wide = ref[0]["boxes"][(ref[0]["roi"] == dc.NONFINITE_KEPT["dw_pos_inf"]) & (ref[0]["classes"] == dc.NONFINITE_CLASS)][0]
    assert wide[0] == 0 and wide[2] == dc.IMAGE_HW[1]                    # clamped to SCALE_CLAMP, clipped to the image: exact
    flat = ref[0]["boxes"][(ref[0]["roi"] == dc.NONFINITE_KEPT["dw_neg_inf"]) & (ref[0]["classes"] == dc.NONFINITE_CLASS)][0]
    assert flat[0] == flat[2]                                             # zero width
    # mapped indices are original rows: past a dropped row they differ from the reference's filtered numbering
    assert max(roi0) > int(ref[0]["valid"].sum()) - 1


def test_general_batch_exceeds_scale_clamp():
    _, deltas, _, _, _ = dc.general_batch()
    dw = deltas.reshape(deltas.shape[0], -1, 4)[..., 2:] / 5.0
    assert float(dw.max()) > orc.SCALE_CLAMP and float(dw.min()) < -2.5
