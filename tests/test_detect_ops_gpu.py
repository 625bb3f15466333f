"""Direct parity tests of the inference tail's kernels (csrc/detect.hip det_select / det_offset_gather / det_final / postprocess /
compact_detections / gather_rows / gather_blocks / boxes_to_rois5, csrc/losses.hip first_k_rois) and of modeling/inference.build_instances
against the CPU oracle. Decisions (classes, RoI indices, counts, order) and the coordinates of the exact recipe (tests/detect_cases.py)
are compared with torch.equal; the one toleranced check (general decode) derives its bound next to the assertion."""
import ctypes

import pytest
import torch

import detect_cases as dc
import unit_oracle as orc

pytestmark = pytest.mark.gpu


def ops():
    from unit_amd import ops as o
    return o


def run_detections(dev, inputs, thresh, topk, cand_cap=None, nms_thresh=dc.NMS_THRESH):
    o = ops()
    probs, deltas, props, pcount, hw = (t.to(dev) for t in inputs)
    out = o.detections(probs, deltas, props, pcount, hw, dc.WEIGHTS, thresh, nms_thresh, topk, cand_cap=cand_cap)
    return tuple(t.cpu() for t in out)


def assert_detections_equal(got, ref, topk):
    want = dc.padded(ref, topk)
    for name, g, w in zip(("boxes", "scores", "classes", "roi", "count"), got, want):
        assert g.dtype == w.dtype and torch.equal(g, w), name


def raw_candidates(dev, inputs, thresh, cap, extra=64):
    """unit_detection_candidates through the C ABI into buffers `extra` slots longer than B * cap, pre-filled with sentinels"""
    o = ops()
    from unit_amd._lib import check, lib
    probs, deltas, props, pcount, hw = (t.to(dev) for t in inputs)
    b, rcap = props.shape[0], props.shape[1]
    k = deltas.shape[1] // 4
    n = b * cap + extra
    cb = torch.full((n, 4), -7.0, dtype=torch.float32, device=dev)
    cs = torch.full((n,), -7.0, dtype=torch.float32, device=dev)
    cc = torch.full((n,), -77, dtype=torch.int32, device=dev)
    cr = torch.full((n,), -77, dtype=torch.int32, device=dev)
    cnt = torch.full((b,), -77, dtype=torch.int32, device=dev)
    cmax = torch.full((b,), -7.0, dtype=torch.float32, device=dev)
    w = (ctypes.c_float * 4)(*dc.WEIGHTS)
    check(lib().unit_detection_candidates(o._p(probs), probs.shape[1], o._p(deltas), deltas.shape[1], o._p(props), o._p(pcount), b, rcap, k, w,
                                          o.SCALE_CLAMP, o._p(hw), float(thresh), cap, o._p(cb), o._p(cs), o._p(cc), o._p(cr), o._p(cnt),
                                          o._p(cmax), o._s()), "detection_candidates")
    return tuple(t.cpu() for t in (cb, cs, cc, cr, cnt, cmax))


# ------------------------------------------------------------------------------------------------ ops.detections, exact
@pytest.mark.parametrize("name", [c[0] for c in dc.SINGLE_CASES])
def test_detections_exact(dev, name):
    case = dc.single_case(name)
    got = run_detections(dev, case["inputs"], case["thresh"], case["topk"])
    assert_detections_equal(got, case["ref"], case["topk"])


def test_detections_topk_edges(dev):
    """topk = 1, topk equal to the number of NMS survivors, and topk above it (tails -1 / 0 past the count)"""
    case = dc.single_case("r137_k7")
    survivors = dc.ref_detections(*case["inputs"], case["thresh"], dc.NMS_THRESH, dc.ALL)[0]["scores"].numel()
    assert survivors > 50
    for topk in (1, survivors, survivors + 7):
        ref = dc.ref_detections(*case["inputs"], case["thresh"], dc.NMS_THRESH, topk)
        got = run_detections(dev, case["inputs"], case["thresh"], topk)
        assert int(got[4][0]) == min(topk, survivors)
        assert_detections_equal(got, ref, topk)


@pytest.mark.parametrize("empty_image,thresh", [(dc.BATCH_EMPTY_IMAGE, 0.05), (dc.BATCH_EMPTY_IMAGE, 3.0 / 64.0), (None, 0.05)])
def test_detections_ragged_batch(dev, empty_image, thresh):
    """B = 4, pcount = [Rcap, 0, 1, Rcap - 3], per-image image sizes, NaN in every row past pcount; one image without proposals and
    (empty_image) one whose scores all lie below / exactly at the threshold"""
    case = dc.batch_case(empty_image, thresh)
    got = run_detections(dev, case["inputs"], thresh, case["topk"])
    for t in got[:2]:
        assert torch.isfinite(t).all()          # padding reaches no output
    assert_detections_equal(got, case["ref"], case["topk"])
    counts = got[4].tolist()
    assert counts[1] == 0 and (counts[2] == 0) == (empty_image is not None)


def test_detections_cand_cap_exact_fit(dev):
    """a candidate cap equal to the candidate count, and one above it, change nothing"""
    case = dc.single_case("r137_k7")
    n = dc.candidates(*case["inputs"], case["thresh"])[0][1].numel()
    base = run_detections(dev, case["inputs"], case["thresh"], case["topk"])
    assert_detections_equal(base, case["ref"], case["topk"])
    for cap in (n, n + 1):
        got = run_detections(dev, case["inputs"], case["thresh"], case["topk"], cand_cap=cap)
        for g, w in zip(got, base):
            assert torch.equal(g, w), cap


def test_candidate_cap_truncates_in_roi_class_order(dev):
    """more candidates than `cap`: the first `cap` in (RoI, class) order are kept, cand_max covers exactly those, nothing is written past
    the buffers. Two images with different candidate counts, two caps."""
    r, k, thr = 137, 7, 0.05
    a, c = dc.exact_single(r, k, seed=3), dc.exact_single(20, k, seed=4)
    probs, deltas, props = torch.zeros(2 * r, k + 1), torch.zeros(2 * r, 4 * k), torch.zeros(2, r, 4)
    probs[:r], deltas[:r], props[0] = a[0], a[1], a[2][0]
    probs[r: r + 20], deltas[r: r + 20], props[1, :20] = c[0], c[1], c[2][0]
    inputs = (probs, deltas, props, torch.tensor([r, 20], dtype=torch.int32), torch.tensor([dc.IMAGE_HW] * 2, dtype=torch.float32))
    ref = dc.candidates(*inputs, thr)
    n0, n1 = ref[0][1].numel(), ref[1][1].numel()
    assert n0 > 400 and 10 < n1 < 300
    for cap in (300, 10):          # image 0 overflows both caps, image 1 only the small one
        cb, cs, cc, cr, cnt, cmax = raw_candidates(dev, inputs, thr, cap)
        assert cnt.tolist() == [min(cap, n0), min(cap, n1)]
        for i in range(2):
            n = int(cnt[i])
            rb, rs, rc, rr = (t[:n] for t in ref[i])
            s = slice(i * cap, i * cap + n)
            assert torch.equal(cb[s], rb) and torch.equal(cs[s], rs) and torch.equal(cc[s], rc.int()) and torch.equal(cr[s], rr.int())
            assert float(cmax[i]) == float(rb.max())          # over exactly the kept candidates ...
        if cap == 10:
            assert float(cmax[0]) < float(ref[0][0].max())          # ... which here is less than the maximum over all of them
        tail = slice(2 * cap, None)
        assert bool((cb[tail] == -7.0).all()) and bool((cs[tail] == -7.0).all()) and bool((cc[tail] == -77).all()) and bool((cr[tail] == -77).all())


# ------------------------------------------------------------------------------------------------ non-finite predictions
def test_detections_drop_nonfinite_rois_whole(dev):
    """a RoI with ANY non-finite decoded box (before clipping) or score (background included) is dropped whole, like the reference's row
    filter; dw = +inf (clamped) and dw = -inf (zero width) are finite and stay. RoI indices are original rows."""
    inputs = dc.nonfinite_batch()
    topk = dc.NONFINITE_R * dc.NONFINITE_K          # every survivor is compared
    ref = dc.ref_detections(*inputs, 0.05, dc.NMS_THRESH, topk)
    got = run_detections(dev, inputs, 0.05, topk)
    roi0 = set(got[3][0][: int(got[4][0])].tolist())
    assert not roi0 & set(dc.NONFINITE_DROPPED.values()), sorted(roi0 & set(dc.NONFINITE_DROPPED.values()))
    assert set(dc.NONFINITE_KEPT.values()) <= roi0
    assert_detections_equal(got, ref, topk)


# ------------------------------------------------------------------------------------------------ decode with general deltas
def test_candidates_general_decode(dev):
    """fractional proposals, random deltas with dw / dh up to 6 (> SCALE_CLAMP). Classes, RoI indices, scores and counts depend only on the
    scores: exact. Boxes against a float64 decode of the same fp32 inputs, within 8 * 2^-24 * max(|pcx|, |pcy|, pw, ph) per box: expf and
    the reference's exp at about 1 ulp each plus the roundings of the divide, multiply and add (each 2^-24 relative to a quantity no
    larger than that maximum); clipping to the image only shrinks an error."""
    inputs = dc.general_batch()
    probs, deltas, props, pcount, hw = inputs
    b, rcap = props.shape[0], props.shape[1]
    k = deltas.shape[1] // 4
    ref = dc.candidates(*inputs, 0.05)
    cb, cs, cc, cr, cnt, cmax = raw_candidates(dev, inputs, 0.05, rcap * k)
    worst = 0.0
    for i in range(b):
        rb, rs, rc, rr = ref[i]
        n = rs.numel()
        assert n > 100 and int(cnt[i]) == n
        s = slice(i * rcap * k, i * rcap * k + n)
        assert torch.equal(cs[s], rs) and torch.equal(cc[s], rc.int()) and torch.equal(cr[s], rr.int())
        dec = orc.apply_deltas(deltas[i * rcap: (i + 1) * rcap].double(), props[i].double(), dc.WEIGHTS).reshape(rcap, k, 4)[rr, rc]
        pcx, pcy = (dec[:, 0] + dec[:, 2]) / 2, (dec[:, 1] + dec[:, 3]) / 2
        pw, ph = dec[:, 2] - dec[:, 0], dec[:, 3] - dec[:, 1]
        bound = 8.0 * 2.0 ** -24 * torch.stack([pcx.abs(), pcy.abs(), pw, ph]).max(0).values
        clip = dec.clone()
        clip[:, 0::2] = clip[:, 0::2].clamp(0, float(hw[i][1]))
        clip[:, 1::2] = clip[:, 1::2].clamp(0, float(hw[i][0]))
        err = (cb[s].double() - clip).abs().max(1).values
        j = int((err / bound).argmax())
        worst = max(worst, float(err[j] / bound[j]))
        print(f"image {i}: {n} candidates, worst box {j}: error {float(err[j]):.3e}, bound {float(bound[j]):.3e}, ratio {float(err[j] / bound[j]):.3f}")
        assert bool((err <= bound).all()), (i, j, float(err[j]), float(bound[j]))
        assert float(cmax[i]) == float(cb[s].max())
        assert int((deltas[i * rcap: (i + 1) * rcap].reshape(rcap, k, 4)[rr, rc][:, 2:] / 5.0 > orc.SCALE_CLAMP).sum()) > 10
    assert worst > 0.0          # (a general decode does round: the comparison is not vacuous)


# ------------------------------------------------------------------------------------------------ ops.detector_postprocess
def test_detector_postprocess_exact(dev):
    o = ops()
    gen = torch.Generator().manual_seed(5)
    topk = 16
    in_hw = [(96, 160), (100, 200), (90, 150)]
    out_hw = [(192, 480), (50, 100), (120, 100)]          # up-scale, down-scale, anisotropic (4/3 in y, 2/3 in x)
    count = [topk, 5, 0]
    boxes = torch.empty(3, topk, 4)
    for i, (h, w) in enumerate(in_hw):
        x0, y0 = torch.rand(topk, generator=gen) * w, torch.rand(topk, generator=gen) * h
        boxes[i] = torch.stack([x0, y0, x0 + 1 + torch.rand(topk, generator=gen) * 40, y0 + 1 + torch.rand(topk, generator=gen) * 40], 1)
        boxes[i, 1] = torch.tensor([w + 3.0, 10.0, w + 9.0, 20.0])          # clips to zero width
        boxes[i, 3] = torch.tensor([10.0, h + 1.0, 20.0, h + 30.0])         # clips to zero height
        boxes[i, 4] = torch.tensor([-9.0, -8.0, -2.0, 30.0])                # left of the image: zero width at 0
        boxes[i, 6] = torch.tensor([12.0, 7.0, 12.0, 30.0])                 # empty before scaling
    scale = torch.tensor([[o_[1] / s[1], o_[0] / s[0]] for o_, s in zip(out_hw, in_hw)], dtype=torch.float32)
    dboxes = boxes.clone().to(dev)
    nonempty = o.detector_postprocess(dboxes, torch.tensor(count, dtype=torch.int32, device=dev), scale.to(dev),
                                      torch.tensor(out_hw, dtype=torch.float32, device=dev))
    assert nonempty.dtype == torch.uint8
    for i in range(3):
        rb, keep = orc.detector_postprocess(boxes[i], in_hw[i], out_hw[i])
        assert torch.equal(dboxes[i].cpu(), rb)          # rewritten in place, every row
        keep = keep & (torch.arange(topk) < count[i])
        assert torch.equal(nonempty[i].cpu().bool(), keep)
        assert not keep[[1, 3, 4, 6]].any()
    assert int(nonempty[0].sum()) > 4 and int(nonempty[1].sum()) > 0 and int(nonempty[2].sum()) == 0


# ------------------------------------------------------------------------------------------------ ops.compact_detections
@pytest.mark.parametrize("mask_elems", [0, 196, 1])
@pytest.mark.parametrize("topk", [1, 100, 1024])
def test_compact_detections_exact(dev, topk, mask_elems):
    o = ops()
    gen = torch.Generator().manual_seed(topk + mask_elems)
    b = 3
    counts = [0, topk, topk // 2]
    boxes, sc = torch.rand(b, topk, 4, generator=gen), torch.rand(b, topk, generator=gen)
    cls = torch.randint(0, 80, (b, topk), generator=gen, dtype=torch.int32)
    roi = torch.arange(b * topk, dtype=torch.int32).reshape(b, topk)          # distinct: a stable order is visible
    masks = None if mask_elems == 0 else torch.rand((b, topk, 14, 14) if mask_elems == 196 else (b, topk, 1), generator=gen)
    j = torch.arange(topk)
    patterns = {"none": None, "alternating": (j % 2 == 0).expand(b, topk), "all_empty": torch.zeros(b, topk, dtype=torch.bool),
                "holes_past_count": torch.stack([j < c for c in counts])}
    cnt = torch.tensor(counts, dtype=torch.int32, device=dev)
    for pname, ne in patterns.items():
        dne = None if ne is None else ne.to(torch.uint8).contiguous().to(dev)
        ob, osc, ocls, oroi, om, kept = o.compact_detections(boxes.to(dev), sc.to(dev), cls.to(dev), roi.to(dev), cnt, dne,
                                                             None if masks is None else masks.to(dev))
        assert ocls.dtype == torch.int64 and kept.dtype == torch.int32 and (om is None) == (masks is None)
        for i in range(b):
            keep = j < counts[i]
            if ne is not None:
                keep = keep & ne[i]
            n = int(keep.sum())
            assert int(kept[i]) == n, (pname, i)
            assert torch.equal(ob[i, :n].cpu(), boxes[i][keep]) and torch.equal(osc[i, :n].cpu(), sc[i][keep]), (pname, i)
            assert torch.equal(ocls[i, :n].cpu(), cls[i][keep].long()) and torch.equal(oroi[i, :n].cpu(), roi[i][keep]), (pname, i)
            if masks is not None:
                assert torch.equal(om[i, :n].cpu(), masks[i][keep]), (pname, i)


def test_compact_detections_argument_errors(dev):
    """host-side argument checks (no launch): topk above 1024, and masks aliased to their output"""
    o = ops()
    from unit_amd._lib import UnitLibError, check, lib
    topk = 1025
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)
    with pytest.raises(UnitLibError, match="topk"):
        o.compact_detections(z(1, topk, 4), z(1, topk), z(1, topk, dt=torch.int32), z(1, topk, dt=torch.int32), z(1, dt=torch.int32))
    topk = 8
    boxes, sc, cls, roi, cnt, masks = z(1, topk, 4), z(1, topk), z(1, topk, dt=torch.int32), z(1, topk, dt=torch.int32), z(1, dt=torch.int32), z(1, topk, 4)
    ocls, kept = z(1, topk, dt=torch.int64), z(1, dt=torch.int32)
    with pytest.raises(UnitLibError, match="separate output"):
        check(lib().unit_compact_detections(o._p(boxes), o._p(sc), o._p(cls), o._p(roi), o._p(masks), 4, o._p(cnt), None, 1, topk,
                                            o._p(torch.empty_like(boxes)), o._p(torch.empty_like(sc)), o._p(ocls), o._p(torch.empty_like(roi)),
                                            o._p(masks), o._p(kept), o._s()), "compact_detections")


# ------------------------------------------------------------------------------------------------ gathers
@pytest.mark.parametrize("dtype,cols", [(torch.float32, 1), (torch.float32, 3), (torch.float32, 75), (torch.bfloat16, 2), (torch.bfloat16, 6),
                                        (torch.bfloat16, 150)])
def test_gather_rows_exact(dev, dtype, cols):
    """rows of 4, 12 and 300 bytes; an index of -1 reads row 0 of the image's OWN block"""
    o = ops()
    gen = torch.Generator().manual_seed(cols)
    b, t, rcap = 3, 5, 7
    src = torch.randn(b * rcap, cols, generator=gen).to(dtype)
    idx = torch.randint(0, rcap, (b, t), generator=gen, dtype=torch.int32)
    idx[0, 1] = idx[1, 0] = idx[2, 4] = -1
    idx[1, 3], idx[2, 2] = rcap - 1, 0
    out = o.gather_rows(src.to(dev), idx.to(dev), rcap)
    ref = torch.stack([src.view(b, rcap, cols)[i, idx[i].clamp(min=0).long()] for i in range(b)]).reshape(b * t, cols)
    assert out.dtype == dtype and out.shape == ref.shape and torch.equal(out.cpu(), ref)
    assert torch.equal(out[1 * t + 0].cpu(), src[1 * rcap]) and torch.equal(out[2 * t + 4].cpu(), src[2 * rcap])


def test_gather_rows_refuses_partial_words(dev):
    o = ops()
    from unit_amd._lib import UnitLibError
    src = torch.zeros(21, 3, dtype=torch.bfloat16, device=dev)          # 6-byte rows
    with pytest.raises(UnitLibError, match="32-bit words"):
        o.gather_rows(src, torch.zeros(3, 5, dtype=torch.int32, device=dev), 7)


@pytest.mark.parametrize("dtype,cols", [(torch.float32, 8), (torch.float32, 6), (torch.float32, 1024), (torch.float32, 1030), (torch.int32, 4),
                                        (torch.int32, 1), (torch.int64, 2), (torch.int64, 3), (torch.bfloat16, 8), (torch.bfloat16, 6),
                                        (torch.bfloat16, 2048)])
def test_gather_blocks_exact(dev, dtype, cols):
    """row words a multiple of 4 (vector path) and not; rows of >= 4096 bytes (256 threads) and small ones; take in {0, 1, block_rows}; a
    source with more rows than nb * block_rows"""
    o = ops()
    gen = torch.Generator().manual_seed(cols)
    nb, block_rows = 3, 5
    rows = nb * block_rows + 4
    if dtype.is_floating_point:
        src = torch.randn(rows, cols, generator=gen).to(dtype)
    else:
        src = torch.randint(-2 ** 31, 2 ** 31 - 1, (rows, cols), generator=gen).to(dtype) * (2 ** 20 + 1 if dtype == torch.int64 else 1)
    dsrc = src.to(dev)
    for take in (0, 1, block_rows):
        out = o.gather_blocks(dsrc, nb, block_rows, take)
        ref = src[: nb * block_rows].view(nb, block_rows, cols)[:, :take].reshape(nb * take, cols)
        assert out.dtype == dtype and out.shape == ref.shape and torch.equal(out.cpu(), ref), take


def test_gather_blocks_keeps_x3_and_checks_alignment(dev):
    o = ops()
    from unit_amd._lib import UnitLibError
    src = torch.randn(10, 8, generator=torch.Generator().manual_seed(1))
    x3 = src.to(dev).as_subclass(o.X3)
    out = o.gather_blocks(x3, 2, 5, 3)
    assert type(out) is o.X3
    assert torch.equal(out.as_subclass(torch.Tensor).cpu(), src.view(2, 5, 8)[:, :3].reshape(6, 8))
    assert type(o.gather_blocks(src.to(dev), 2, 5, 3)) is torch.Tensor
    flat = torch.zeros(10 * 4 + 4, dtype=torch.float32, device=dev)
    view = flat[1: 1 + 40].view(10, 4)          # 16-byte rows that start 4 bytes past a 16-byte boundary
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    with pytest.raises(UnitLibError, match="alignment"):
        o.gather_blocks(view, 2, 5, 3)


@pytest.mark.parametrize("b,t", [(3, 5), (3, 100), (1, 1)])
def test_boxes_to_rois5_exact(dev, b, t):
    o = ops()
    boxes = torch.rand(b, t, 4, generator=torch.Generator().manual_seed(b * t)) * 100
    out = o.boxes_to_rois5(boxes.to(dev)).cpu()
    ref = torch.cat([torch.arange(b).float().repeat_interleave(t)[:, None], boxes.reshape(b * t, 4)], 1)
    assert out.shape == (b * t, 5) and torch.equal(out, ref)


@pytest.mark.parametrize("s", [4, 6, 9])
def test_first_k_rois_exact(dev, s):
    """S below, equal to and above Pcap; pcount of 0, Pcap, above Pcap and in between; a batch index offset; rois_out as a row slice of a
    larger buffer whose other rows stay untouched"""
    o = ops()
    pcap, b0 = 6, 2
    pcount = [0, pcap, pcap + 3, 3]
    b = len(pcount)
    props = torch.rand(b, pcap, 4, generator=torch.Generator().manual_seed(s)) * 100 + 1
    big = torch.full((b * s + 10, 5), -7.0, dtype=torch.float32, device=dev)
    for rois_out in (None, big[3: 3 + b * s]):
        rois, valid = o.first_k_rois(props.to(dev), torch.tensor(pcount, dtype=torch.int32, device=dev), s, b0, rois_out=rois_out)
        ref = torch.zeros(b, s, 5)
        ok = torch.zeros(b, s, dtype=torch.bool)
        for i, n in enumerate(pcount):
            m = min(n, pcap, s)
            ref[i, :, 0] = i + b0
            ref[i, :m, 1:] = props[i, :m]
            ok[i, :m] = True
        assert torch.equal(rois.cpu(), ref.reshape(b * s, 5))
        assert valid.dtype == torch.int32 and torch.equal(valid.cpu(), torch.where(ok, 0, -1).int().reshape(-1))
    assert rois.data_ptr() == big[3].data_ptr()
    assert bool((big[:3] == -7.0).all()) and bool((big[3 + b * s:] == -7.0).all())


# ------------------------------------------------------------------------------------------------ build_instances
@pytest.mark.parametrize("with_masks", [False, True])
@pytest.mark.parametrize("postprocess", [False, True])
def test_build_instances_from_device_tensors(dev, postprocess, with_masks):
    """ops.detections on the ragged B = 4 batch -> build_instances, against the per-image reference chain (detections, then
    detector_postprocess and its non-empty filter when out_hw is given)"""
    from unit_amd.modeling.inference import build_instances
    case = dc.batch_case(None)
    topk = case["topk"]
    o = ops()
    probs, deltas, props, pcount, hw = (t.to(dev) for t in case["inputs"])
    boxes, sc, cls, roi, cnt = o.detections(probs, deltas, props, pcount, hw, dc.WEIGHTS, case["thresh"], dc.NMS_THRESH, topk)
    masks = torch.rand(len(dc.BATCH_HW), topk, 14, 14, generator=torch.Generator().manual_seed(9))
    out_hw = [dc.OUT_HW] * len(dc.BATCH_HW) if postprocess else None
    res = build_instances(boxes, sc, cls, roi, cnt, masks.to(dev) if with_masks else None, list(dc.BATCH_HW), out_hw)
    assert len(res) == len(dc.BATCH_HW)
    dropped = 0
    for i, (r, ref) in enumerate(zip(res, case["ref"])):
        inst = r["instances"] if postprocess else r
        keep = ref["nonempty"] if postprocess else torch.ones_like(ref["nonempty"])
        dropped += int((~keep).sum())
        n = int(keep.sum())
        assert inst.image_size == (dc.OUT_HW if postprocess else dc.BATCH_HW[i])
        assert len(inst) == n and inst.pred_boxes.tensor.shape == (n, 4)
        assert torch.equal(inst.pred_boxes.tensor.cpu(), (ref["pp_boxes"] if postprocess else ref["boxes"])[keep])
        assert torch.equal(inst.scores.cpu(), ref["scores"][keep])
        assert inst.pred_classes.dtype == torch.int64 and torch.equal(inst.pred_classes.cpu(), ref["classes"][keep])
        assert torch.equal(inst._roi_index.cpu().long(), ref["roi"][keep])
        if with_masks:
            want = masks[i, : ref["scores"].numel()][keep]
            if postprocess:
                assert inst.pred_masks.dtype == torch.bool and inst.pred_masks.shape == (n,) + dc.OUT_HW
                assert torch.equal(inst.pred_mask_probs.cpu(), want[:, None])
            else:
                assert inst.pred_masks.shape == (n, 1, 14, 14) and torch.equal(inst.pred_masks.cpu(), want[:, None])
        else:
            assert "pred_masks" not in inst._fields
    assert len(res[1]["instances"] if postprocess else res[1]) == 0          # the image without proposals: an empty Instances
    assert dropped > 0 if postprocess else dropped == 0
