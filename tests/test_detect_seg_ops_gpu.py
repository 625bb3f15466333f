"""The class-segmented NMS stage of ops.detections (csrc/detect.hip det_seg_* / det_keep_pos / det_merge_keep, unit_nms per class) on
the device: bit for bit against the full form wherever both run, against the host restatement (tests/detect_seg_ref.py) above 65 536
candidates, its intermediate buffers against numpy, and the refusals. Indices and copies of bits only: no tolerances."""
import numpy as np
import pytest
import torch

import detect_cases as dc
import detect_seg_cases as sc
import detect_seg_ref as sr

pytestmark = pytest.mark.gpu

NAMES = ("boxes", "scores", "classes", "roi", "count")


def ops():
    from unit_amd import ops as o
    return o


def run(dev, inputs, thresh, topk, nms, cand_cap=None, nms_thresh=dc.NMS_THRESH):
    probs, deltas, props, pcount, hw = (t.to(dev) for t in inputs)
    out = ops().detections(probs, deltas, props, pcount, hw, dc.WEIGHTS, thresh, nms_thresh, topk, cand_cap=cand_cap, nms=nms)
    return tuple(t.cpu() for t in out)


def assert_same(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
        if g.dtype == torch.float32:          # copies of bits (a -0.0 or a NaN would count)
            assert torch.equal(g.view(torch.int32), w.view(torch.int32)), (what, name)
        else:
            assert torch.equal(g, w), (what, name)


def existing_cases():
    out = [(n, lambda n=n: dc.single_case(n)) for n, _, _, _, _ in dc.SINGLE_CASES]
    out += [(f"batch_{e}_{t:.4f}", lambda e=e, t=t: dc.batch_case(e, t)) for e, t in ((dc.BATCH_EMPTY_IMAGE, 0.05),
                                                                                    (dc.BATCH_EMPTY_IMAGE, 3.0 / 64.0), (None, 0.05))]
    out.append(("nonfinite", lambda: dict(inputs=dc.nonfinite_batch(), thresh=0.05, topk=60)))
    out.append(("general", lambda: dict(inputs=dc.general_batch(), thresh=0.05, topk=100)))
    return out


# ------------------------------------------------------------------------------------------------ both forms agree
@pytest.mark.parametrize("name,make", existing_cases(), ids=[n for n, _ in existing_cases()])
def test_forms_agree_on_the_existing_cases(dev, name, make):
    case = make()
    full = run(dev, case["inputs"], case["thresh"], case["topk"], "full")
    seg = run(dev, case["inputs"], case["thresh"], case["topk"], "segmented")
    assert_same(seg, full, name)
    assert int(full[4].sum()) > 0
    if "ref" in case:
        assert_same(seg, dc.padded(case["ref"], case["topk"]), name)


@pytest.mark.parametrize("name", sc.SMALL)
def test_forms_agree_on_the_new_cases(dev, name):
    c = sc.case(name)
    full = run(dev, c["inputs"], c["thresh"], c["topk"], "full", c["cand_cap"])
    seg = run(dev, c["inputs"], c["thresh"], c["topk"], "segmented", c["cand_cap"])
    assert_same(seg, full, name)
    assert_same(seg, dc.padded(sc.case_ref(name), c["topk"]), name)
    auto = run(dev, c["inputs"], c["thresh"], c["topk"], None, c["cand_cap"])          # below the limit None is the full form: the same again
    assert_same(auto, full, name)


def test_general_decode_thresholds(dev):
    """fractional boxes (IoUs not on a grid) at three NMS thresholds: the same-class IoU decisions are the same float computation in both forms"""
    inputs = dc.general_batch(seed=35, b=2, r=400, k=6)
    for thr in (0.3, 0.5, 0.7):
        full = run(dev, inputs, 0.05, 100, "full", nms_thresh=thr)
        seg = run(dev, inputs, 0.05, 100, "segmented", nms_thresh=thr)
        assert_same(seg, full, thr)


# ------------------------------------------------------------------------------------------------ above the limit
@pytest.mark.parametrize("name", sc.LARGE)
def test_above_the_old_limit(dev, name):
    """R * K > 65 536 candidates, all passing, cand_cap = R * K: the kept (RoI, class) list, its order, boxes and scores against the host
    restatement of the segmented rule"""
    c = sc.case(name)
    assert c["cand_cap"] > ops().max_detection_candidates()
    got = run(dev, c["inputs"], c["thresh"], c["topk"], None, c["cand_cap"])
    want = dc.padded(sc.case_ref(name), c["topk"])
    assert int(want[4][0]) == c["topk"]
    assert_same(got, want, name)
    forced = run(dev, c["inputs"], c["thresh"], c["topk"], "segmented", c["cand_cap"])
    assert_same(forced, got, name)


# ------------------------------------------------------------------------------------------------ intermediate buffers
@pytest.mark.parametrize("name", ["pops", "batch_empty_image", "count_equals_cap"])
def test_intermediate_buffers(dev, name):
    """segment counts, the in-segment order, the global-position table, the per-class keep lists and the merged keep / keep_count with its
    -1 tail, against the host restatement"""
    o = ops()
    c = sc.case(name)
    probs, deltas, props, pcount, hw = (t.to(dev) for t in c["inputs"])
    b, rcap, k, topk = props.shape[0], props.shape[1], c["k"], c["topk"]
    cap = c["cand_cap"] or rcap * k
    cb, cs, cc, cr, cnt, cmax, order = o.detection_candidates(probs, deltas, props, pcount, hw, dc.WEIGHTS, c["thresh"], cap)
    rseg = min(rcap, cap)
    keep, kc, (sn, sp, skeep, skc) = o.segmented_nms(cb, cs, cc, order, cnt, cmax, k, rseg, sc.NMS_THRESH, topk, want_parts=True)
    order, sn, sp, skeep, skc, keep, kc = (t.cpu().numpy() for t in (order, sn, sp, skeep, skc, keep, kc))
    assert sp.shape == (b * k, rseg) and skeep.shape == (b * k, topk) and keep.shape == (b, topk)
    cands = sc.case_candidates(name)
    for i, (bx, s, cls, roi) in enumerate(cands):
        assert int(cnt[i]) == s.numel()
        _, pos = sr.score_order(s)
        segs = sr.segments(s, cls, k)
        keeps = sr.class_keeps(bx, s, cls, k, sc.NMS_THRESH, topk)
        for q in range(k):
            seg, n = i * k + q, segs[q].numel()
            assert sn[seg] == n, (i, q)
            assert np.array_equal(sp[seg, :n], pos[segs[q]].numpy()), (i, q)          # the global-position table ...
            assert np.array_equal(order[i, sp[seg, :n]], segs[q].numpy()), (i, q)          # ... and through it the in-segment order
            nk = keeps[q].numel()
            assert skc[seg] == nk and np.array_equal(skeep[seg, :nk], keeps[q].numpy()) and (skeep[seg, nk:] == -1).all(), (i, q)
        want = pos[sr.segmented_keep(bx, s, cls, k, sc.NMS_THRESH, topk)].numpy()
        assert kc[i] == want.size and np.array_equal(keep[i, :want.size], want) and (keep[i, want.size:] == -1).all(), i
    assert sorted(sn.tolist()) != [0] * (b * k)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(dev):
    o = ops()
    from unit_amd._lib import UnitLibError
    c = sc.case("topk_1")
    with pytest.raises(UnitLibError, match="more than 1048576 candidates per image"):
        run(dev, c["inputs"], c["thresh"], c["topk"], None, o.max_segmented_candidates() + 1)
    with pytest.raises(UnitLibError, match="more than 1048576 candidates per image"):
        run(dev, c["inputs"], c["thresh"], c["topk"], "segmented", o.max_segmented_candidates() + 1)
    with pytest.raises(UnitLibError, match="nms: more than 65536 candidates per image"):          # the full form's message, as ever
        run(dev, c["inputs"], c["thresh"], c["topk"], "full", o.max_detection_candidates() + 1)
    ok = run(dev, c["inputs"], c["thresh"], c["topk"], None, o.max_detection_candidates() + 1)          # one above: the segmented form takes over
    assert_same(ok, run(dev, c["inputs"], c["thresh"], c["topk"], "full"), "one above the limit")
