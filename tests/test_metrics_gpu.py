"""Training metrics on the device: the three counting kernels (csrc/metrics.hip) against the CPU restatement of Detectron2's logging
blocks (tests/metrics_ref.py) -- integer counts, compared with == --, and the fused step with `collect_metrics` against the scalars the
reference's own step logged (tests/golden/metrics_golden.npz), eagerly, from a hipGraph and from a recorded call list."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
GDIR = os.path.join(os.path.dirname(__file__), "golden")
sys.path.insert(0, GDIR)
import metrics_ref as R  # noqa: E402
from unit_amd import _lib, engine, metrics as M, ops  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(GDIR, "metrics_golden.npz"))
NAN, INF = float("nan"), float("inf")


def _zeros(dev, n=5):
    return torch.zeros(n, dtype=torch.int32, device=dev)


# ---------------------------------------------------------------------------------------------------- unit_metrics_fastrcnn
def _score_matrix(r, ncls, seed, pad=11, col0=5):
    """[r, ncls + pad] with the classifier window at col0: what lies outside the window (huge values, NaN) must not matter"""
    g = torch.Generator().manual_seed(seed)
    full = torch.randn(r, ncls + pad, generator=g) * 3.0
    full[:, :col0] = 1e30
    full[:, col0 + ncls:] = NAN
    return full


def _run_fastrcnn(full, col0, ncls, cls, dev, m=None):
    m = _zeros(dev) if m is None else m
    fd, cd = full.to(dev), cls.to(dev)
    ops.metrics_fastrcnn(fd, col0, ncls, cd, m)
    return m.cpu().tolist()


@pytest.mark.parametrize("ncls", [21, 81])
@pytest.mark.parametrize("r", [1, 63, 64, 65, 257])
def test_fastrcnn_counts_equal_detectron2(dev, r, ncls):
    k, col0 = ncls - 1, 5
    full = _score_matrix(r, ncls, 100 * ncls + r)
    g = torch.Generator().manual_seed(r)
    cls = torch.randint(0, ncls, (r,), generator=g).int()
    win = full[:, col0:col0 + ncls]
    hit = torch.rand(r, generator=g) < 0.4          # make a good share of the rows correct: the winning column carries the label
    cls[hit] = win.argmax(1)[hit].int()
    if r > 8:
        cls[3], cls[r - 2] = -1, k + 4          # empty slots (unit_gather_rois writes -1)
    want = R.fastrcnn_counts_with_empty_slots(win, cls)
    assert want[0] > 0 or r == 1
    assert _run_fastrcnn(full, col0, ncls, cls, dev) == want


@pytest.mark.parametrize("ncls", [21, 81])
def test_fastrcnn_ties_nan_and_degenerate_batches(dev, ncls):
    k, col0 = ncls - 1, 5
    rows, expect = [], []

    def row(vals, arg):
        x = torch.full((ncls,), -1.0)
        for c, v in vals.items():
            x[c] = v
        rows.append(x)
        expect.append(arg)
    row({0: 2.0, 7: 2.0}, 0)                               # equal maxima at the first column
    row({5: 2.0, k: 2.0}, 5)                               # ... at the last column
    row({k - 1: 2.0, k: 2.0}, k - 1)
    row({k: 2.0}, k)                                       # the last column alone
    row({c: -1.0 for c in range(ncls)}, 0)                 # every column equal
    row({c: -INF for c in range(ncls)}, 0)                 # all -inf (the novel columns of the base training, on every column)
    row({3: INF, 9: NAN, 15: NAN}, 9)                      # NaN beats +inf, the first NaN wins
    row({c: (0.0 if c == 2 else -0.0 if c == 4 else -5.0) for c in range(ncls)}, 2)          # 0.0 == -0.0: the lower index
    if ncls > 65:
        row({63: 2.0, 64: 2.0}, 63)                        # equal maxima across the lanes' first and second column
        row({64: 2.0, 70: 2.0}, 64)
        row({64: NAN, 63: 7.0, 0: NAN}, 0)
        row({1: 1.0, 65: 1.0}, 1)
    win = torch.stack(rows)
    assert win.argmax(1).tolist() == expect          # (the test's own expectation of torch's rule)
    full = _score_matrix(len(rows), ncls, 7)
    full[:, col0:col0 + ncls] = win
    arg = torch.tensor(expect, dtype=torch.int32)
    for cls in (arg.clone(),                                                        # every row correct
                torch.full_like(arg, k),                                            # an all-background batch
                torch.where(arg == k, torch.zeros_like(arg), arg),                  # a batch with no background
                torch.full_like(arg, -1)):                                          # nothing but empty slots
        want = R.fastrcnn_counts_with_empty_slots(win, cls)
        assert _run_fastrcnn(full, col0, ncls, cls, dev) == want, cls.tolist()
    # R = 0: no launch, counters untouched
    m = torch.arange(5, dtype=torch.int32, device=dev)
    ops.metrics_fastrcnn(torch.empty((0, ncls), device=dev), 0, ncls, torch.empty(0, dtype=torch.int32, device=dev), m)
    assert m.cpu().tolist() == [0, 1, 2, 3, 4]


# ---------------------------------------------------------------------------------------------------- unit_metrics_rpn
def test_rpn_counts(dev):
    g = torch.Generator().manual_seed(5)
    lab = (torch.randint(0, 3, (2, 1007), generator=g) - 1).to(torch.int8)
    assert set(lab.unique().tolist()) == {-1, 0, 1}
    want = R.rpn_scalars(list(lab))[0]
    m = _zeros(dev)
    ops.metrics_rpn(lab.to(dev), m)
    assert m.cpu().tolist() == want + [0, 0, 0]
    # a pointer that is no multiple of four bytes, and a size that is no multiple of four labels
    flat = lab.reshape(-1).to(dev)
    for lo, hi in ((1, 2014), (3, 1000), (2, 5), (0, 3)):
        m = _zeros(dev)
        ops.metrics_rpn(flat[lo:hi], m)
        part = lab.reshape(-1)[lo:hi]
        assert m.cpu().tolist() == [int((part == 1).sum()), int((part == 0).sum()), 0, 0, 0], (lo, hi)
    m = _zeros(dev)
    ops.metrics_rpn(torch.full((2, 1007), -1, dtype=torch.int8, device=dev), m)
    assert m.cpu().tolist() == [0] * 5


# ---------------------------------------------------------------------------------------------------- unit_metrics_mask
@pytest.mark.parametrize("msz", [14, 28])
@pytest.mark.parametrize("s", [0, 1, 5])
def test_mask_counts_equal_detectron2(dev, s, msz):
    k, ldk = 3, 8
    g = torch.Generator().manual_seed(10 * s + msz)
    lg = torch.randn(s * msz * msz, ldk, generator=g)
    tg = (torch.rand(s, msz, msz, generator=g) < 0.4).to(torch.uint8)
    cls = torch.tensor([1, 0, -1, 2, 3][:s], dtype=torch.int32)          # -1 and K: slots that are skipped
    if s > 0:
        # exactly 0.0f and -0.0f on both target values, in the gt-class column of slot 0 (pixels (0,0) (0,1) (1,0) (1,1) = rows 0..3)
        lg[0:4, 1] = torch.tensor([0.0, -0.0, 0.0, -0.0])
        tg[0, 0, 0], tg[0, 0, 1], tg[0, 1, 0], tg[0, 1, 1] = 1, 1, 0, 0
    want = R.mask_counts_from_layout(lg, k, ldk, cls, tg)
    if s > 0:
        assert want[0] == (1 if s == 1 else 3) * msz * msz and want[4] >= 2
    m = _zeros(dev)
    lg_d, cls_d, tg_d = lg.to(dev), cls.to(dev), tg.to(dev)
    ops.metrics_mask(lg_d, k, ldk, cls_d, tg_d, m)
    assert m.cpu().tolist() == want


# ---------------------------------------------------------------------------------------------------- refusals, accumulation
def test_refusals_and_adding_into_nonzero_counters(dev):
    l = _lib.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    sc = torch.zeros(4, 32, device=dev)
    cls = torch.zeros(4, dtype=torch.int32, device=dev)
    lab = torch.zeros(16, dtype=torch.int8, device=dev)
    tg = torch.zeros(1, 14, 14, dtype=torch.uint8, device=dev)
    lg = torch.zeros(196, 8, device=dev)
    m = torch.full((16,), 7, dtype=torch.int32, device=dev)
    s = ops._s()
    bad = [
        l.unit_metrics_fastrcnn(p(sc), 128, 0, 97, p(cls), 4, p(m), s),          # more columns than the loss kernels take
        l.unit_metrics_fastrcnn(p(sc), 32, 0, 21, p(cls), -1, p(m), s),          # negative sizes
        l.unit_metrics_fastrcnn(p(sc), 32, -1, 21, p(cls), 4, p(m), s),
        l.unit_metrics_fastrcnn(p(sc), 32, 12, 21, p(cls), 4, p(m), s),          # col0 + ncls > ld
        l.unit_metrics_fastrcnn(p(sc), 32, 0, 21, p(cls), 4, None, s),           # null output
        l.unit_metrics_rpn(p(lab), -5, p(m), s),
        l.unit_metrics_rpn(p(lab), 16, None, s),
        l.unit_metrics_mask(p(lg), 3, 8, p(cls), p(tg), -1, 14, p(m), s),
        l.unit_metrics_mask(p(lg), 3, 8, p(cls), p(tg), 1, -14, p(m), s),
        l.unit_metrics_mask(p(lg), 9, 8, p(cls), p(tg), 1, 14, p(m), s),          # more classes than the pixel row holds
        l.unit_metrics_mask(p(lg), 3, 8, p(cls), p(tg), 1, 14, None, s),
    ]
    assert all(st < 0 for st in bad), bad
    assert bad[0] == -4 and l.unit_last_error()          # UNIT_ERR_UNSUPPORTED, with a message
    torch.cuda.synchronize()
    assert m.cpu().tolist() == [7] * 16          # a refused call launches nothing
    # the kernels ADD: two calls into pre-loaded counters, neighbours untouched
    g = torch.Generator().manual_seed(3)
    win = torch.randn(70, 21, generator=g)
    c = torch.randint(0, 21, (70,), generator=g).int()
    want = R.fastrcnn_counts_with_empty_slots(win, c)
    wd, cd = win.to(dev), c.to(dev)
    ops.metrics_fastrcnn(wd, 0, 21, cd, m[M.FAST_RCNN:M.FAST_RCNN + 5])
    ops.metrics_fastrcnn(wd, 0, 21, cd, m[M.FAST_RCNN:M.FAST_RCNN + 5])
    labs = torch.tensor([1, 0, 0, -1, 1, 1, 0], dtype=torch.int8, device=dev)
    ops.metrics_rpn(labs, m[M.RPN:M.RPN + 5])
    exp = [7] * 16
    exp[0], exp[1] = 7 + 3, 7 + 3
    for i, w in enumerate(want):
        exp[M.FAST_RCNN + i] = 7 + 2 * w
    assert m.cpu().tolist() == exp


# ---------------------------------------------------------------------------------------------------- step level
_STEPS = {}


def _hip_step(name, dev, collect=True):
    """the fp32 step of tests/test_unit_golden_gpu.py::_hip_step (the reference's permutations) with the metrics switch; run once per case"""
    key = (name, collect)
    if key not in _STEPS:
        import gen_ref_step as G
        from unit_amd.modeling.rcnn import LOSS_NAMES
        cfg, model, sup, weak, perms, masks = G.step_inputs(name, device="cuda")
        R.shift_classifier_bias(model, name)          # as the fixture's generator does: without it no RoI of any case is classified right
        model.train()
        model.compute_dtype = torch.float32
        model.collect_metrics = collect
        batch = model.pack_batch(sup, weak if weak else None)
        model._ensure_ready()
        cap = cfg.MODEL.RPN.POST_NMS_TOPK_TRAIN + batch.gt_boxes.shape[1]
        roi = torch.stack([torch.cat([p, torch.arange(len(p), cap)]) for p in perms["roi"]])
        dperms = {"rpn": torch.stack(perms["rpn"]).int().to(dev), "roi": roi.int().to(dev)}
        step = model.forward_train(batch, dperms, early_backward=True)
        model.backward_train(step)
        torch.cuda.synchronize()
        raw = None if model.last_metrics is None else model.last_metrics.cpu().tolist()
        assert (step.metrics is None) == (not collect) and (step.metrics is model.last_metrics)
        _STEPS[key] = (raw, model.last_metrics_images, step.losses.cpu(), LOSS_NAMES)
    return _STEPS[key]


@pytest.mark.parametrize("name", ["s1", "s2", "mask", "coco_mask"])
def test_step_metrics_vs_reference(dev, name):
    raw, n, _, _ = _hip_step(name, dev)
    ref = GOLD[f"{name}/counts"].tolist()
    assert n == int(GOLD[f"{name}/n_images"])
    print(name, "counts", raw, "reference", ref)
    sl = M.SLOTS
    for k in ("rpn_pos", "rpn_neg", "roi_instances", "roi_fg"):          # index decisions: exact
        assert raw[sl[k]] == ref[sl[k]], (k, raw[sl[k]], ref[sl[k]])
    # a float decision may legitimately fall the other way only on a row / element the reference itself all but tied on
    und_rows, und_el = int(GOLD[f"{name}/undecided_rows"]), int(GOLD[f"{name}/undecided_elements"])
    for k in ("roi_correct", "roi_fg_correct", "roi_fg_as_bg"):
        assert abs(raw[sl[k]] - ref[sl[k]]) <= und_rows, (k, raw[sl[k]], ref[sl[k]], und_rows)
    assert raw[sl["mask_elements"]] == ref[sl["mask_elements"]] and raw[sl["mask_positive"]] == ref[sl["mask_positive"]]
    for k in ("mask_incorrect", "mask_false_positive", "mask_false_negative"):
        assert abs(raw[sl[k]] - ref[sl[k]]) <= und_el, (k, raw[sl[k]], ref[sl[k]], und_el)
    assert raw[2:5] == [0, 0, 0] and raw[15] == 0          # unused slots stay zero
    got = M.scalars(raw, n)
    assert sorted(got) == sorted(str(k) for k in GOLD[f"{name}/keys"])
    if und_rows == 0 and und_el == 0:          # (then the counts are equal, and so are the ratios: same ints, same Python division)
        assert got == dict(zip([str(k) for k in GOLD[f"{name}/keys"]], GOLD[f"{name}/values"].tolist()))


def test_step_metrics_fine_tune_mask_head_has_no_mask_keys(dev):
    raw, n, _, _ = _hip_step("mask_ft", dev)
    got = M.scalars(raw, n)
    assert not any(k.startswith("mask_rcnn/") for k in got) and raw[M.MASK:M.MASK + 5] == [0] * 5
    assert set(got) == set(M.KEYS[:7])


def test_losses_do_not_change_with_the_switch(dev):
    """the nine losses with metrics on are bit-equal to the run without ("s1" and "s2": every loss kernel of these cases is
    bit-reproducible from run to run; unit_mask_bce_loss adds its per-workgroup partial sums with float atomics, in arrival order)"""
    for name in ("s1", "s2"):
        _, _, on, names = _hip_step(name, dev, collect=True)
        raw, _, off, _ = _hip_step(name, dev, collect=False)
        assert raw is None
        assert torch.equal(on, off), (name, dict(zip(names, (on - off).tolist())))
        assert torch.isfinite(on).all()


# ---------------------------------------------------------------------------------------------------- eager / hipGraph / call list
PARENT_N_CALLS = 228          # recorded calls of one step of _setup's configuration on the parent commit (no metrics code anywhere)


def _setup(metrics):
    from unit_amd import config
    from unit_amd.modeling import build_model
    from unit_amd.solver import FlatSGD
    from unit_amd.synthetic import init_synthetic_weights
    cfg = config.voc_rcnn_c4_split1(50)
    cfg.MODEL.DEVICE = "cuda"
    cfg.MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE = 32
    cfg.MODEL.RPN.PRE_NMS_TOPK_TRAIN, cfg.MODEL.RPN.POST_NMS_TOPK_TRAIN = 600, 100
    cfg.SOLVER.WARMUP_ITERS = 4
    cfg.SEED = 3
    model = build_model(cfg)
    init_synthetic_weights(model, seed=1)
    model.train()
    model.collect_metrics = metrics
    return cfg, model, FlatSGD(model, cfg)


def test_eager_graph_and_replay_give_identical_vectors(dev):
    from unit_amd.synthetic import synthetic_batch
    data = [synthetic_batch(2, 2, hw=(128, 192), seed=50 + i, max_gt=4) for i in range(3)]
    seq = [data[i] for i in (0, 1, 2, 1, 0)]          # two eager warm-up steps, the capture / recording, two replays -- with other data
    cfg, m1, o1 = _setup(True)
    ref, ref_losses = [], []
    for d in seq:
        b = m1.pack_batch(*d, gt_buckets=engine.GraphedStep.GT_BUCKETS)
        o1._bind()
        o1.use_device_lr(m1.device)
        step = m1.forward_train(b, early_backward=True)
        m1.backward_train(step)
        o1.step()
        ref.append(m1.last_metrics.clone())
        ref_losses.append(step.losses.clone())
    torch.cuda.synchronize()
    ref = [r.cpu().tolist() for r in ref]
    assert all(r[M.SLOTS["roi_instances"]] > 0 and r[M.SLOTS["rpn_neg"]] > 0 for r in ref) and len({tuple(r) for r in ref}) > 1
    plans = {}
    for kind, cls in (("graph", engine.GraphedStep), ("replay", engine.ReplayedStep)):
        cfg, m2, o2 = _setup(True)
        rs = cls(m2, o2, warmup_steps=2)
        got = []
        for d in seq:
            rs.run(*d)
            got.append(m2.last_metrics.clone())
        torch.cuda.synchronize()
        assert rs.stats == {"eager": 2, "captured": 1, "replayed": 2}
        assert [g.cpu().tolist() for g in got] == ref, kind
        plans[kind] = rs
    # the switch off: no vector, not one call more in the list; on: the fill and the kernels of this configuration (no mask head), nothing else
    cfg, m3, o3 = _setup(False)
    rs = engine.ReplayedStep(m3, o3, warmup_steps=2)
    off_losses = [rs.run(*d).clone() for d in seq]
    torch.cuda.synchronize()
    assert m3.last_metrics is None
    names = lambda plan: sorted(n for it in plan.items if it[0] == "calls" for n in it[3])
    off = next(iter(rs.plans.values()))[0]
    on = next(iter(plans["replay"].plans.values()))[0]
    assert not any(n.startswith("unit_metrics") for n in names(off))
    assert names(on) == sorted(names(off) + ["unit_fill_zero", "unit_metrics_rpn", "unit_metrics_fastrcnn"])
    # the list without the switch has the length it had on the commit before the metrics existed: 228 calls for this configuration
    # (measured on that commit with this very _setup, data sequence and ReplayedStep(warmup_steps=2)); with the switch it is that list
    # plus exactly the fill and the two kernels
    print("recorded calls without metrics:", off.n_calls, "with:", on.n_calls)
    assert off.n_calls == PARENT_N_CALLS
    assert on.n_calls == off.n_calls + 3
    for a, b in zip(off_losses, ref_losses):          # ... and the losses do not know about the switch
        assert torch.equal(a, b)


def test_trainer_metrics_dict(dev):
    from unit_amd.synthetic import synthetic_batch
    cfg, model, _ = _setup(False)
    tr = engine.TrainerNoMeta(cfg, model, metrics=True)
    assert model.collect_metrics is True
    sup, weak = synthetic_batch(2, 2, hw=(96, 128), seed=9, max_gt=3)
    tr.run_step(sup, weak)
    d = tr.metrics_dict()
    raw = model.last_metrics.cpu().tolist()
    assert d == M.scalars(raw, 2) and set(M.KEYS[:5]) <= set(d) and not any(k.startswith("mask_rcnn/") for k in d)
    assert d["rpn/num_pos_anchors"] + d["rpn/num_neg_anchors"] == 256.0          # RPN.BATCH_SIZE_PER_IMAGE anchors are sampled per image
    assert d["roi_head/num_fg_samples"] + d["roi_head/num_bg_samples"] <= 32.0
    # the plugin surface fills it too: model(batched_inputs, weak_batched_inputs=...)
    model.last_metrics = None
    losses = model(sup, weak_batched_inputs=weak)
    assert model.last_metrics is not None and model.last_metrics_images == 2 and "loss_cls" in losses
    seen = []
    M.put_scalars(type("S", (), {"put_scalar": lambda self, k, v: seen.append(k)})(), model.last_metrics.cpu().tolist(), 2)
    assert set(seen) >= set(M.KEYS[:5])
    cfg, model, _ = _setup(True)
    tr = engine.TrainerNoMeta(cfg, model)          # the trainer's default leaves a switch the caller set on the model alone
    assert model.collect_metrics is True
    tr.run_step(sup, weak)
    assert tr.metrics_dict() == M.scalars(model.last_metrics.cpu().tolist(), 2)
    cfg, model, _ = _setup(False)
    tr = engine.TrainerNoMeta(cfg, model)
    assert model.collect_metrics is False
    tr.run_step(sup, weak)
    assert model.last_metrics is None
    with pytest.raises(RuntimeError):
        tr.metrics_dict()
