"""Class-segmented NMS stage, host side: the restatement (tests/detect_seg_ref.py) against the oracle's batched_nms, the promises of the
cases (tests/detect_seg_cases.py), the C-ABI declarations, the two ceilings and the TTA refusal. Indices and bits only: no tolerances."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import detect_cases as dc  # noqa: E402
import detect_seg_cases as sc  # noqa: E402
import detect_seg_ref as sr  # noqa: E402
import tta_ref  # noqa: E402

H, W = 96, 128


# ------------------------------------------------------------------------------------------------ the restatement is the existing rule
@pytest.mark.parametrize("name", sc.SMALL + sc.LARGE)
def test_segmented_rule_equals_batched_nms(name):
    """(the oracle's greedy loop takes the 66 000 and 72 000 candidates of the large cases too: 1.5 to 7 s each on the host)"""
    c = sc.case(name)
    for bx, s, cls, roi in sc.case_candidates(name):
        want = sr.full_keep(bx, s, cls, sc.NMS_THRESH, c["topk"])
        got = sr.segmented_keep(bx, s, cls, c["k"], sc.NMS_THRESH, c["topk"])
        assert torch.equal(got, want)


@pytest.mark.parametrize("name", [n for n, _, _, _, _ in dc.SINGLE_CASES])
def test_segmented_rule_equals_the_reference_chain(name):
    """on the cases of tests/detect_cases.py: the restatement on host_candidates gives ref_detections' rows, and host_candidates is the list
    dc.candidates reads back from the oracle"""
    case = dc.single_case(name)
    cands = sr.host_candidates(*case["inputs"], case["thresh"], dc.WEIGHTS)
    for a, b in zip(cands[0], dc.candidates(*case["inputs"], case["thresh"])[0]):
        assert torch.equal(a, b)
    got = sr.segmented_detections(cands, case["k"], dc.NMS_THRESH, case["topk"])[0]
    for key in ("boxes", "scores", "classes", "roi"):
        assert torch.equal(got[key], case["ref"][0][key]), key


# ------------------------------------------------------------------------------------------------ the cases keep their promises
def _pops(name):
    c = sc.case(name)
    return [torch.bincount(cls, minlength=c["k"]).tolist() for _, _, cls, _ in sc.case_candidates(name)]


def test_class_populations():
    assert _pops("pops") == [[63, 64, 0, 65, 128, 129, 1]]
    assert _pops("empty_class_between") == [[40, 0, 40]]
    assert _pops("one_class_all_rois") == [[1, 1, 150, 1, 1, 1]]
    cands = sc.case_candidates("one_class_all_rois")[0]
    assert sorted(cands[3][cands[2] == 2].tolist()) == list(range(150))          # one candidate of class 2 per RoI
    batch = [sum(p) for p in _pops("batch_empty_image")]
    assert batch[1] == 0 and batch[2] == 0 and batch[0] > 100 and batch[3] > 100 and batch[0] != batch[3]
    assert sc.case("batch_empty_image")["inputs"][3].tolist() == [137, 0, 1, 134]


@pytest.mark.parametrize("name", sc.LARGE)
def test_candidate_counts_above_the_old_limit(name):
    r, k = sc.OVER[name]
    c = sc.case(name)
    assert r * k > sc.OLD_LIMIT and c["cand_cap"] == r * k and c["k"] == k
    probs = c["inputs"][0]
    assert int((probs[:, :k] > c["thresh"]).sum()) == r * k and bool(torch.isfinite(probs).all())          # every (RoI, class) passes
    if name == "long_segment":
        assert (r + 63) // 64 > 256          # per class more words than the decoupled scan takes: the plain scan runs per segment


def test_cap_cases():
    for name, slack in (("count_equals_cap", 0), ("count_cap_minus_1", 1)):
        c = sc.case(name)
        assert sc.case_candidates(name)[0][1].numel() == c["n_cand"] == c["cand_cap"] - slack


def test_topk_cases():
    assert sc.case("topk_1")["topk"] == 1
    assert sc.case("topk_5000")["topk"] > 4096          # NMS_DQ_MAXKEEP (csrc/sort_nms.hip)
    c = sc.case("topk_above_union")
    assert len(sc.case_ref("topk_above_union")[0]["scores"]) == c["survivors"] == c["topk"] - 9


def test_ties_straddle_the_cut():
    c = sc.case("ties_at_cut")
    bx, s, cls, roi = sc.case_candidates("ties_at_cut")[0]
    keep = sr.full_keep(bx, s, cls, sc.NMS_THRESH, dc.ALL)
    t = c["topk"]
    assert t < keep.numel()
    ks, kc, kr = s[keep], cls[keep], roi[keep]
    assert ks[t - 2] == ks[t - 1] == ks[t] == ks[t + 1]          # equal scores on both sides of the cut ...
    assert kc[t - 1] != kc[t] and kr[t - 1] != kr[t]          # ... across classes and across RoIs
    # and the stable order decides: (RoI, class) ascending inside the run
    key = kr * c["k"] + kc
    assert bool((key[t - 2:t + 1] < key[t - 1:t + 2]).all())


@pytest.mark.parametrize("name", sc.SMALL + sc.LARGE)
def test_shifted_classes_are_at_least_one_apart(name):
    """float32: the lowest coordinate of class c + 1 after the shift lies >= 1.0 above the highest of class c, so no cross-class IoU is positive"""
    c = sc.case(name)
    for bx, s, cls, _ in sc.case_candidates(name):
        if s.numel() == 0:
            continue
        sh = sr.shifted(bx, cls)
        assert sh.dtype == torch.float32
        present = sorted(set(cls.tolist()))
        for lo, hi in zip(present[:-1], present[1:]):
            gap = sh[cls == hi].min() - sh[cls == lo].max()
            assert float(gap) >= 1.0, (lo, hi, float(gap))


# ------------------------------------------------------------------------------------------------ declarations and ceilings
def test_exports_declared():
    from unit_amd._lib import parse_header, parse_header_names
    protos, names = parse_header(), parse_header_names()
    for fn in ("unit_detection_class_segments", "unit_detection_merge_keep"):
        assert fn in protos and names[fn][-1] == "stream", fn
    assert names["unit_detection_max_candidates"] == [] and names["unit_detection_segments_check"] == ["B", "cap", "K", "Rseg"]
    assert names["unit_detection_segments_workspace_bytes"] == ["B", "cap", "K"]
    for arg in ("seg_boxes", "seg_scores", "seg_count", "seg_pos", "Rseg"):
        assert arg in names["unit_detection_class_segments"], arg
    for arg in ("seg_keep", "seg_keep_count", "seg_pos", "keep", "keep_count", "topk"):
        assert arg in names["unit_detection_merge_keep"], arg


def test_ceilings():
    from unit_amd import ops
    from unit_amd._lib import lib
    assert ops.max_detection_candidates() == 65536
    assert ops.max_segmented_candidates() >= 320000          # 4000 proposals x 80 classes
    assert ops.max_segmented_candidates() == 1 << 20          # the sorter's 2^20 keys are the smallest limit left
    # the bounds, applied without a launch (the library loads without a device)
    assert lib().unit_detection_segments_check(1, 320000, 80, 4000) == 0
    assert lib().unit_detection_segments_check(1, (1 << 20) + 1, 80, 4000) != 0
    assert lib().unit_detection_segments_check(1, 4 * 65537, 4, 65537) != 0          # one class above unit_nms's capacity
    assert lib().unit_detection_segments_check(1, 100, 97, 10) != 0
    # the mask of 2000 x 80 in class segments: 41 MB, where the full form would need 3.2 GB at 160 000 candidates
    assert lib().unit_nms_workspace_bytes(80, 2000) == 80 * 2000 * 32 * 8


def _aug():
    from unit_amd.config import CN
    sizes, max_size, flip = tta_ref.CASE_AUG["tta"]
    return CN(ENABLED=True, MIN_SIZES=sizes, MAX_SIZE=max_size, FLIP=flip)


def _inp(n):
    from unit_amd.structures import Boxes, Instances
    return {"image": torch.zeros(3, H, W), "height": H, "width": W, "proposals": Instances((H, W), proposal_boxes=Boxes(torch.zeros(n, 4)))}


def test_tta_refusal_moves_to_the_new_ceiling():
    from unit_amd import ops
    from unit_amd.modeling.inference import UnsupportedConfig, tta_candidate_limit, tta_check
    limit = ops.max_segmented_candidates()
    aug = _aug()
    tta_check(aug, [_inp(900)], 80, candidate_limit=limit)          # 72 000 candidates: refused before
    with pytest.raises(UnsupportedConfig):
        tta_check(aug, [_inp(900)], 80)          # (tta_check's own default is still unit_nms's limit)
    tta_check(aug, [_inp(limit // 80)], 80, candidate_limit=limit)
    with pytest.raises(UnsupportedConfig, match=f"exceed the {limit} the NMS kernel takes") as e:
        tta_check(aug, [_inp(limit // 80 + 1)], 80, candidate_limit=limit)
    assert f"at most {limit // 80} proposals" in str(e.value)
    # what inference_tta passes: the ceiling, and no class above one unit_nms problem (every proposal is a candidate of every class)
    assert tta_candidate_limit(80) == tta_candidate_limit(20) == limit and tta_candidate_limit(4) == 4 * 65536


def test_detections_refuses_an_unknown_form_and_a_cap_above_the_ceiling():
    """both before anything is allocated or launched: CPU tensors never reach a kernel"""
    from unit_amd import ops
    from unit_amd._lib import UnitLibError
    inputs = sc.case("topk_1")["inputs"]
    with pytest.raises(ValueError, match="nms must be"):
        ops.detections(*inputs, dc.WEIGHTS, 0.05, 0.5, 10, nms="classwise")
    with pytest.raises(UnitLibError, match="more than 1048576 candidates"):
        ops.detections(*inputs, dc.WEIGHTS, 0.05, 0.5, 10, cand_cap=ops.max_segmented_candidates() + 1)
