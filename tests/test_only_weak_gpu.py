"""The weak-only training mode on the device (TrainerOnlyWeak, engine/defaults.py:377-400; `train_only_weak=True`, meta_arch/rcnn.py:433):
unit_sgd_step_masked bit for bit against a NumPy restatement of sgd_step_elem, the fp32 step and three-iteration trajectory against the
reference's own run (tests/golden/only_weak_golden.npz, generator tests/golden/gen_only_weak_golden.py) at the bars existing tests apply
to an fp32 step against a reference fixture, and the other surfaces of the mode."""
import functools
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GDIR = os.path.join(HERE, "golden")
sys.path.insert(0, GDIR)
import gen_only_weak_golden as W  # noqa: E402

FX = np.load(os.path.join(GDIR, "only_weak_golden.npz"))

# the bars of an fp32 step against a reference fixture, restated with the lines they come from
LOSS_BAR = 1e-4          # |got - ref| <= 1e-4 * max(1, |ref|): tests/test_rpn_pseudo_gpu.py:155, tests/test_unit_golden_gpu.py:410 (iterations 0-2)
GRAD_BAR = 2e-3          # gradient norm and head: <= 2e-3 * norm + 1e-8: tests/test_rpn_pseudo_gpu.py:177, :181
TRAJ_RTOL, TRAJ_ATOL, TRAJ_UPD = 1e-4, 2e-6, 1e-2          # final values / total update: tests/test_unit_golden_gpu.py:420
BF16_RTOL, BF16_ATOL = 0.1, 0.05          # a bf16 step beside the fp32 step: tests/test_step_gpu.py:154


# ---------------------------------------------------------------------------------------------------- 1. the kernel
SIZES = (1, 3, 4, 5, 1023, 1024, 1025)
LR, MOM, WD, SCALE, CLIP = 1.5, 0.9, 1e-4, 0.5, 0.4


def _layout():
    """rows of 1, 3, 4, 5, 1023, 1024, 1025 elements, twice, with 0-3 padding elements between them: row borders inside a 4-element vector,
    rows smaller than one, rows larger than a 1024-element workgroup -> (rows, size) with size ~ 6200"""
    rows, off = [], 2
    for k, n in enumerate(SIZES + SIZES):
        rows.append((off, n))
        off += n + k % 4
    return rows, (off + 11) // 4 * 4


def _masks(n_rows):
    return {"alternating": np.arange(n_rows) % 2 == 0, "other_half": np.arange(n_rows) % 2 == 1, "all_dead": np.zeros(n_rows, bool),
            "all_live": np.ones(n_rows, bool)}


def _restate(p, g, b, rows, live, coefs, lo, n, lr, lr_dev, first, nesterov, mode):
    """sgd_step_elem (csrc/optim.hip) in NumPy float32, one rounding per operation (the library is built without contraction), over the
    elements of [lo, lo + n) that lie in a live row or in no row"""
    f = np.float32
    p, b = p.copy(), b.copy()
    on, coef = np.ones(p.size, bool), np.ones(p.size, f)
    for (o, m), l, c in zip(rows, live, coefs):
        on[o:o + m], coef[o:o + m] = l, c
    on[:lo], on[lo + n:] = False, False
    lr = f(lr) * f(lr_dev) if lr_dev is not None else f(lr)
    with np.errstate(all="ignore"):
        x = g[on] * f(SCALE)
        if mode == 1:
            x = np.where(x > f(CLIP), f(CLIP), np.where(x < -f(CLIP), -f(CLIP), x))
        elif mode == 2:
            x = x * coef[on]
        d = x + f(WD) * p[on]
        nb = d if first else f(MOM) * b[on] + d
        b[on] = nb
        p[on] = p[on] - lr * ((d + f(MOM) * nb) if nesterov else nb)
    return p, b


def _bits(t):
    return t.detach().cpu().numpy().view(np.int32)


@pytest.mark.parametrize("nesterov", [0, 1])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_masked_sgd_kernel_bit_for_bit(dev, mode, nesterov):
    """every variant of the issue: clip_mode 0 / 1 / 2, nesterov, first_step, lr_dev set / unset; aligned base pointers (vector path), base
    pointers offset by one float (scalar path), a range that starts and ends inside rows; masks alternating (both phases), all dead, all
    live. Dead rows hold NaN / Inf gradients and keep the bits of p and buf; all live equals unit_sgd_step bit for bit."""
    from unit_amd import ops
    rows, size = _layout()
    assert 6000 <= size <= 6400 and any((o % 4) and ((o + n) % 4) for o, n in rows)
    rng = np.random.default_rng(17 + 2 * mode + nesterov)
    p0, b0, g0 = (rng.standard_normal(size).astype(np.float32) for _ in range(3))
    coefs = rng.uniform(0.3, 1.0, len(rows)).astype(np.float32)
    coefs[::3] = 1.0
    table = torch.tensor(rows, dtype=torch.int64, device=dev)
    coefs_d = torch.from_numpy(coefs).to(dev)
    inner = (rows[4][0] + 5, rows[12][0] + 700 - rows[4][0] - 5)          # starts inside row 4, ends inside row 12
    assert inner[0] % 4 and (inner[0] + inner[1]) % 4
    for name, live in _masks(len(rows)).items():
        live_d = torch.from_numpy(live.astype(np.uint8)).to(dev)
        for first in (0, 1):
            for lr_dev in (None, 0.02):
                lrd = None if lr_dev is None else torch.tensor([lr_dev], device=dev)
                for shift, (lo, n) in ((0, (0, size)), (1, (0, size - 1)), (0, inner), (1, inner)):
                    # shift 1: the buffers are views one float into the allocation -- not 16-byte aligned -- and the table counts from them
                    g = g0.copy()
                    for (o, m), l in zip(rows, live):          # what a dead row's gradient holds must not matter
                        if not l:
                            g[shift + o:shift + o + m:2], g[shift + o + 1:shift + o + m:2] = np.nan, np.inf
                    pd, gd, bd = (torch.from_numpy(a).to(dev)[shift:] for a in (p0, g, b0))
                    ops.sgd_step_masked(pd, gd, bd, lo, n, LR, MOM, WD, table, live_d, SCALE, first_step=first, lr_dev=lrd, nesterov=nesterov,
                                        clip_mode=mode, clip_value=CLIP, coefs=coefs_d)
                    wp, wb = _restate(p0[shift:], g[shift:], b0[shift:], rows, live, coefs, lo, n, LR, lr_dev, first, nesterov, mode)
                    what = (name, first, lr_dev, shift, lo, n)
                    assert np.array_equal(_bits(pd), wp.view(np.int32)), what
                    assert np.array_equal(_bits(bd), wb.view(np.int32)), what
                    assert np.array_equal(_bits(gd), g[shift:].view(np.int32)), what          # the gradients are only read
                    if name == "all_dead":          # only the padding elements moved
                        for o, m in rows:
                            assert np.array_equal(_bits(pd)[o:o + m], p0[shift:][o:o + m].view(np.int32))
                    if name == "all_live":
                        p2, g2, b2 = (torch.from_numpy(a).to(dev)[shift:] for a in (p0, g, b0))
                        ops.sgd_step(p2, g2, b2, lo, n, LR, MOM, WD, SCALE, first_step=first, lr_dev=lrd, nesterov=nesterov, clip_mode=mode,
                                     clip_value=CLIP, table=table, coefs=coefs_d)
                        assert np.array_equal(_bits(pd), _bits(p2)) and np.array_equal(_bits(bd), _bits(b2)), what


def test_masked_sgd_argument_checks_launch_nothing(dev):
    from unit_amd import ops
    from unit_amd._lib import UnitLibError, lib
    rows, size = _layout()
    table = torch.tensor(rows, dtype=torch.int64, device=dev)
    live = torch.ones(len(rows), dtype=torch.uint8, device=dev)
    p, g, b = (torch.randn(size, device=dev) for _ in range(3))
    p0, b0 = p.clone(), b.clone()
    with pytest.raises(UnitLibError, match="one live byte per row"):          # null `live`
        ops.sgd_step_masked(p, g, b, 0, size, LR, MOM, WD, table, None)
    with pytest.raises(ValueError, match="live flags for a table of"):          # the mask and the table disagree about the row count
        ops.sgd_step_masked(p, g, b, 0, size, LR, MOM, WD, table, live[:-1])
    st = lib().unit_sgd_step_masked(ops._p(p), ops._p(g), ops._p(b), 0, size, LR, MOM, WD, 1.0, 0.0, 0, 0, 0, ops._p(table), 0, None, ops._p(live),
                                    None, ops._s())
    assert st != 0 and b"n_seg" in lib().unit_last_error()
    st = lib().unit_sgd_step_masked(ops._p(p), ops._p(g), ops._p(b), 0, size, LR, MOM, WD, 1.0, 0.0, 0, 0, 2, ops._p(table), len(rows), None,
                                    ops._p(live), None, ops._s())
    assert st != 0 and b"coefs" in lib().unit_last_error()          # coefficient mode without coefficients
    torch.cuda.synchronize()
    assert torch.equal(p, p0) and torch.equal(b, b0)


# ---------------------------------------------------------------------------------------------------- 2. the step against the fixture
def _trainable(model):
    return {n: q for n, q in model.named_parameters() if q.requires_grad}


@functools.lru_cache(maxsize=None)
def _run(case, mask=True, dtype="fp32", steps=W.STEPS):
    """`steps` TrainerOnlyWeak.run_step on the fixture inputs -> host copies (computed once per form, shared by the tests below)"""
    from unit_amd import engine
    cfg, model, weak = W.only_weak_inputs(case, device="cuda")
    model.train()
    model.compute_mode = dtype
    tr = engine.TrainerOnlyWeak(cfg, model, metrics=True)
    if not mask:          # test only: every row named live -- the weak-only steps swept like any other step
        named = type(tr.optimizer).set_live
        tr.optimizer.set_live = lambda live: named(tr.optimizer, [True] * len(live))
    model._ensure_ready()
    out = {"start": {n: q.detach().cpu().clone() for n, q in _trainable(model).items()}, "losses": [], "loss_vec": []}
    fired = []
    model.on_grad_ready = fired.append
    for it in range(steps):
        tr.run_step(None, weak)
        out["losses"].append(tr.loss_dict())
        out["loss_vec"].append(dict(zip(model.loss_names, tr.last_losses.cpu().tolist())))
        if it == 0:
            out["grads"] = {n: q.grad.detach().cpu().clone() for n, q in _trainable(model).items()}
            out["metrics"] = tr.metrics_dict()
            out["fired"], out["sequence"] = list(fired), model.only_weak_tag_sequence()
            out["clip_rows"] = list(tr.optimizer.names)
    torch.cuda.synchronize()
    out["final"] = {n: q.detach().cpu().clone() for n, q in _trainable(model).items()}
    out["momentum"] = tr.optimizer.momentum_buffer().cpu().clone()
    out["entries"] = [(e["name"], int(e["offset"]), int(e["numel"])) for e in model.store.entries if e["param"].requires_grad]
    return out


@pytest.mark.parametrize("case", W.CASES)
def test_fp32_step_and_trajectory_vs_the_reference_run(dev, case):
    """iteration-0 losses and gradients, the three-iteration trajectory through TrainerOnlyWeak.run_step, the final parameters: dead tensors
    BIT-equal to their initial values, live tensors at the trajectory bars"""
    r = _run(case)
    names = [str(k) for k in FX[f"{case}/loss_names"]]
    worst = []
    for it in range(W.STEPS):
        got = r["losses"][it]
        assert sorted(got) == names, (it, sorted(got))          # exactly the reference's keys
        for k in set(r["loss_vec"][it]) - set(names):          # slots the reference's dictionary does not have: never written
            assert r["loss_vec"][it][k] == 0.0, k
        worst.append(max(abs(got[k] - v) / max(1.0, abs(v)) for k, v in zip(names, FX[f"{case}/losses"][it])))
        print(case, "iteration", it, {k: (got[k], float(v)) for k, v in zip(names, FX[f"{case}/losses"][it])})
    print(case, "worst loss deviation per iteration", worst)
    pre = f"{case}/it0/gradnorm/"
    keys = [k[len(pre):] for k in FX.files if k.startswith(pre)]
    assert any(k.startswith("backbone.") for k in keys) and any(".res5." in k for k in keys) and any(".weak_detector_head." in k for k in keys)
    gworst = 0.0
    for k in keys:
        g, n = r["grads"][k], float(FX[pre + k])
        ref = torch.from_numpy(FX[f"{case}/it0/gradhead/{k}"])
        e1 = abs(g.double().norm().item() - n)
        assert e1 <= GRAD_BAR * n + 1e-8, (case, k, e1, n)
        if n <= 1e-8:
            # a reference norm below the bar's own absolute term is zero by the bar's standard, and here it is zero by construction:
            # detection_stream.bias shifts every proposal's logit of a class alike, the softmax over proposals (weak_detector_fast_rcnn.py:
            # 206) does not see it, so both sides hold the fp32 rounding residue of a sum that cancels (measured 5e-9 against 1.2e-8) --
            # there is no head to compare element by element
            assert k.endswith("detection_stream.bias"), (case, k, n)
            continue
        e2 = (g.contiguous().reshape(-1)[:ref.numel()] - ref).abs().max().item()
        gworst = max(gworst, e1 / n, e2 / n)
        assert e2 <= GRAD_BAR * n + 1e-8, (case, k, e2, n)
    print(case, "worst gradient deviation / norm", gworst)
    dead = {str(n) for n in FX[f"{case}/dead_names"]}
    for n in dead:          # torch left .grad at None; here the range is cleared -- and the optimizer never touches the tensor
        assert not r["grads"][n].any(), n
        assert torch.equal(r["final"][n].view(torch.int32), r["start"][n].view(torch.int32)), n
    for name, o, m in r["entries"]:          # ... nor its momentum
        if name in dead:
            assert not r["momentum"][o:o + m].any(), name
    bad, worst_rel, worst_upd = [], 0.0, 0.0
    for n in (str(x) for x in FX[f"{case}/names"]):
        if n in dead:
            continue
        ref = torch.from_numpy(FX[f"{case}/final_sample/{n}"])
        got, start = W.sample(r["final"][n]), W.sample(r["start"][n])
        upd, err = (ref - start).norm().item(), (got - ref).norm().item()
        worst_rel = max(worst_rel, ((got - ref).abs() / ref.abs().clamp(min=1e-2)).max().item())
        worst_upd = max(worst_upd, err / (upd + 1e-12))
        if not torch.allclose(got, ref, rtol=TRAJ_RTOL, atol=TRAJ_ATOL) or err > TRAJ_UPD * upd + 1e-9:
            bad.append((n, err, upd, (got - ref).abs().max().item()))
    print(case, "worst parameter deviation (relative, floor 1e-2)", worst_rel, "worst update deviation / update norm", worst_upd)
    for it, d in enumerate(worst):
        assert d <= LOSS_BAR, (case, it, worst)
    assert not bad, bad[:5]


def test_step_reports_every_bucket_and_no_supervised_metric(dev):
    r = _run("ow")
    assert r["fired"] == r["sequence"] and r["fired"][0] == "heads" and set(r["fired"][-2:]) == {"box_head", "rpn"}
    assert not any(k.startswith(("rpn/", "roi_head/", "fast_rcnn/", "mask_rcnn/")) for k in r["metrics"]), r["metrics"]
    assert r["clip_rows"] == [n for n, _, _ in r["entries"]]


def test_same_steps_without_the_mask_move_the_dead_tensors(dev):
    """every row named live (a switch of this test, not of the class): the weak-only steps are swept like any other step. Every dead weight then carries momentum (buf = wd * p: the
    sweep reached it) and the dead tensors no longer hold their initial bits -- the RPN head's and box_head's weights, whose decay of
    lr * wd ~ 5e-8 relative per step reaches the last bit of an fp32 value; the delta predictors' (DELTA_LR_FACTOR 0.25 on 1e-3-sized
    values) stays below half an ulp for three iterations, and a dead bias (WEIGHT_DECAY_BIAS 0, zero gradient) does not move at all. The
    trajectory test can see the mask."""
    r, m = _run("ow", mask=False), _run("ow")
    dead = [str(n) for n in FX["ow/dead_names"]]
    assert any(n.startswith("roi_heads.box_head.") for n in dead)
    where = {name: (o, k) for name, o, k in r["entries"]}
    changed = set()
    for n in dead:
        o, k = where[n]
        assert not m["momentum"][o:o + k].any(), n
        if n.endswith(".weight"):
            assert r["momentum"][o:o + k].any(), n
            assert (r["final"][n].abs() <= r["start"][n].abs()).all(), n          # decay only: no gradient reached it
        if not torch.equal(r["final"][n].view(torch.int32), r["start"][n].view(torch.int32)):
            changed.add(n)
    print("dead tensors that moved without the mask:", sorted(changed))
    assert "proposal_generator.rpn_head.conv.weight" in changed and any(n.startswith("roi_heads.box_head.res5.") for n in changed), sorted(changed)
    assert all(n.endswith(".weight") for n in changed)
    # the first iteration sees the same weights either way; from then on the decayed RPN head proposes other boxes to the weak head
    assert r["losses"][0] == m["losses"][0]


@pytest.mark.parametrize("ctype", ["norm", "full_model"])
def test_dead_rows_add_nothing_to_the_clipping_norms(dev, ctype):
    """SOLVER.CLIP_GRADIENTS under the mask: a dead row's gradient is the zeros the step cleared, so its norm is exactly 0 (its own
    coefficient 1), the full-model coefficient is the one of the live rows' norms alone, and the dead tensors keep their bits"""
    from unit_amd import config, engine
    cfg, model, weak = W.only_weak_inputs("ow", device="cuda")
    model.train()
    model.compute_mode = "fp32"
    start = {n: q.detach().cpu().clone() for n, q in _trainable(model).items()}
    live = model.live_entries(False, True)
    c = cfg.clone()
    clip = 0.05          # below the larger gradient norms of the step (the fixture's iteration-0 norms reach 1 ... 20): the bound is active
    c.SOLVER.CLIP_GRADIENTS = config.CN(ENABLED=True, CLIP_TYPE=ctype, CLIP_VALUE=clip, NORM_TYPE=2.0)
    tr = engine.TrainerOnlyWeak(c, model)
    tr.run_step(None, weak)
    torch.cuda.synchronize()
    norms, coefs = tr.optimizer.grad_norms().cpu(), tr.optimizer.clip_coefs().cpu()
    names = tr.optimizer.names
    assert len(norms) == len(live) == len(names)
    for n, l, nv, cv in zip(names, live, norms.tolist(), coefs.tolist()):
        if not l:
            assert nv == 0.0, (n, nv)
            assert torch.equal(model.state_dict()[n].cpu().view(torch.int32), start[n].view(torch.int32)), n
            if ctype == "norm":
                assert cv == 1.0, (n, cv)
        else:          # (detection_stream.bias: a sum that cancels, see the trajectory test -- its norm is rounding residue, possibly 0)
            assert np.isfinite(nv) and (nv > 0.0 or n.endswith("detection_stream.bias")), (n, nv)
    live_norms = torch.tensor([nv for nv, l in zip(norms.tolist(), live) if l], dtype=torch.float64)
    if ctype == "full_model":
        want = min(1.0, clip / (float(live_norms.pow(2).sum().sqrt()) + 1e-6))
        assert want < 1.0 and all(abs(cv - want) <= 1e-6 * want for cv in coefs.tolist()), (want, coefs[:4])
    else:
        assert (coefs[torch.tensor(live)] < 1).any()          # the bound does clip some live tensor
    assert any(not torch.equal(model.state_dict()[n].cpu(), start[n]) for n, l in zip(names, live) if l)


def test_early_per_bucket_update_follows_the_mask(dev):
    """TrainerOnlyWeak(early_update=True): every bucket -- the dead ones too -- is updated from inside the backward through
    MaskedFlatSGD.step_tag; three steps end bit-equal to the tail update, parameters and momentum, the dead tensors untouched"""
    from unit_amd import engine, ops
    cfg, model, weak = W.only_weak_inputs("ow", device="cuda")
    model.train()
    model.compute_mode = "fp32"
    tr = engine.TrainerOnlyWeak(cfg, model, early_update=True)
    launches = {"masked": 0, "other": 0}
    masked, plain, momentum = ops.sgd_step_masked, ops.sgd_step, ops.sgd_momentum
    monkey = {"sgd_step_masked": lambda *a, **k: (launches.__setitem__("masked", launches["masked"] + 1), masked(*a, **k))[1],
              "sgd_step": lambda *a, **k: (launches.__setitem__("other", launches["other"] + 1), plain(*a, **k))[1],
              "sgd_momentum": lambda *a, **k: (launches.__setitem__("other", launches["other"] + 1), momentum(*a, **k))[1]}
    assert tr.early is not None and tr.early.optimizer is tr.optimizer and type(tr.optimizer).__name__ == "MaskedFlatSGD"
    tagged = []
    step_tag = tr.optimizer.step_tag
    tr.optimizer.step_tag = lambda tag: (tagged.append(tag), step_tag(tag))[1]
    for name, fn in monkey.items():
        setattr(ops, name, fn)
    try:
        for it in range(W.STEPS):
            tr.run_step(None, weak)
    finally:
        ops.sgd_step_masked, ops.sgd_step, ops.sgd_momentum = masked, plain, momentum
    torch.cuda.synchronize()
    assert tagged == model.only_weak_tag_sequence() * W.STEPS
    assert launches["masked"] >= len(tagged) and launches["other"] == 0, launches
    ref = _run("ow")
    for n, q in _trainable(model).items():
        assert torch.equal(q.detach().cpu().view(torch.int32), ref["final"][n].view(torch.int32)), n
    assert torch.equal(tr.optimizer.momentum_buffer().cpu().view(torch.int32), ref["momentum"].view(torch.int32))
    for n in (str(x) for x in FX["ow/dead_names"]):
        assert torch.equal(ref["final"][n].view(torch.int32), ref["start"][n].view(torch.int32)), n


def test_a_mask_belongs_to_one_step_and_one_store(dev):
    from unit_amd.solver import MaskedFlatSGD
    cfg, model, weak = W.only_weak_inputs("ow", device="cuda")
    model.train()
    model.compute_mode = "fp32"
    opt = MaskedFlatSGD(model, cfg)
    batch = model.pack_batch(None, weak)
    model.train_step_only_weak(batch, opt)
    model.backward_train_only_weak(model.forward_train_only_weak(batch))
    before = model.store.params.clone()
    with pytest.raises(RuntimeError, match="before every step"):          # consumed by the step above
        opt.step()
    opt.set_live(model.live_entries(False, True))
    model.flatten_parameters()
    with pytest.raises(RuntimeError, match="re-flattened after set_live"):
        opt.step()
    torch.cuda.synchronize()
    assert torch.equal(model.store.params, before)


# ---------------------------------------------------------------------------------------------------- 3. against the full step
def _typed_model(typ, dtype="fp32"):
    from unit_amd.layers import invalidate_prepared
    from unit_amd.modeling import build_model
    from unit_amd.synthetic import init_synthetic_weights
    cfg = W.only_weak_cfg("ow", "cuda")
    cfg.MODEL.ROI_HEADS.FAST_RCNN.WEAK_DETECTOR.TYPE = typ
    model = build_model(cfg)
    init_synthetic_weights(model, seed=W.WEIGHT_SEED)
    invalidate_prepared()
    model.train()
    model.compute_mode = dtype
    return cfg, model


@pytest.mark.parametrize("typ", ["OICR", "PCL"])
def test_weak_losses_equal_those_of_a_default_step_on_the_same_weak_images(dev, typ):
    """the default supervised + weak step with the supervised images padded to another size runs the weak images as a group of their own:
    its loss_im_cls / loss_oicr_* are the weak-only step's (same weights, same weak images)"""
    from unit_amd.synthetic import synthetic_batch
    _, _, weak = W.only_weak_inputs("ow", device="cuda")
    sup, _ = synthetic_batch(2, 1, hw=(80, 112), num_classes=20, seed=9, max_gt=3)
    cfg, model = _typed_model(typ)
    only = model.forward_train_only_weak(model.pack_batch(None, weak)).losses.cpu().tolist()
    full_step = model.forward_train(model.pack_batch(sup, weak))
    assert full_step.split
    full = full_step.losses.cpu().tolist()
    names = model.loss_names
    for k in ("loss_im_cls", "loss_oicr_1", "loss_oicr_2", "loss_oicr_3"):
        a, b = only[names.index(k)], full[names.index(k)]
        print(typ, k, a, b)
        assert a > 0 and abs(a - b) <= LOSS_BAR * max(1.0, abs(b)), (typ, k, a, b)
    for k in ("loss_cls", "loss_box_reg", "loss_rpn_cls", "loss_rpn_loc"):
        assert only[names.index(k)] == 0.0 and full[names.index(k)] > 0


# ---------------------------------------------------------------------------------------------------- 4. nothing supervised is launched
SUPERVISED_ENTRIES = ("unit_rpn_loss", "unit_rpn_loss_w", "unit_rpn_loss_ex", "unit_iou_match", "unit_subsample_labels", "unit_box_reg_loss",
                      "unit_box_reg_loss_ex", "unit_perm_keys", "unit_counter_bump", "unit_append_gt", "unit_roi_classes", "unit_gather_rois",
                      "unit_sup_scores")


def _meta_ops():
    """the operators tools/stock_ops.py counts as pure metadata / allocation (read from that file: one list)"""
    import ast
    import re
    with open(os.path.join(os.path.dirname(HERE), "tools", "stock_ops.py")) as f:
        m = re.search(r"^META = (\{.*?\})", f.read(), flags=re.S | re.M)
    return ast.literal_eval(m.group(1))


def test_weak_only_step_launches_nothing_supervised_and_no_aten_kernel(dev):
    from torch.utils._python_dispatch import TorchDispatchMode
    from unit_amd._lib import Recorder, enqueues, parse_header_names
    from unit_amd.solver import MaskedFlatSGD
    cfg, model, weak = W.only_weak_inputs("ow", device="cuda")
    model.train()
    model.compute_mode = "fp32"
    opt = MaskedFlatSGD(model, cfg)
    batch = model.pack_batch(None, weak)
    for _ in range(2):          # steady state: constants uploaded, workspaces sized, weight copies refreshed by the multi-tensor launch
        model.train_step_only_weak(batch, opt)
    rpn_bwd = []
    head = model.proposal_generator.rpn_head
    orig_bwd = head.bwd
    head.bwd = lambda *a, **k: rpn_bwd.append(1) or orig_bwd(*a, **k)
    meta, calls = _meta_ops(), []

    class Log(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            parts = str(func).split(".")
            if (parts[1] if len(parts) >= 2 else parts[0]) not in meta:
                calls.append(str(func))
            return func(*args, **(kwargs or {}))
    try:
        with Recorder() as rec, Log():
            model.train_step_only_weak(batch, opt)
        plan = rec.finish()
    finally:
        head.bwd = orig_bwd
    torch.cuda.synchronize()
    names = [n for it in plan.items if it[0] == "calls" for n in it[3]]
    known = parse_header_names()
    assert all(n in known and enqueues(n) for n in SUPERVISED_ENTRIES)          # the entry names as the header declares them
    assert len(names) > 100 and not (set(names) & set(SUPERVISED_ENTRIES)), sorted(set(names) & set(SUPERVISED_ENTRIES))
    assert not rpn_bwd          # no RPN-head backward
    assert "unit_sgd_step_masked" in names and "unit_sgd_momentum" not in names and "unit_sgd_step" not in names
    assert any("roi_align" in n for n in names) and "unit_fill_zero" in names          # the weak half did run; dead ranges cleared by the library
    assert calls == [], sorted(set(calls))


# ---------------------------------------------------------------------------------------------------- 5. other surfaces
def _flat_grads(model):
    return model.store.grads.detach().cpu().clone()


def test_plugin_forward_and_autograd_equal_train_step(dev):
    cfg, model, weak = W.only_weak_inputs("ow", device="cuda")
    model.train()
    model.compute_mode = "fp32"
    batch = model.pack_batch(None, weak)
    want = model.train_step_only_weak(batch).cpu()
    torch.cuda.synchronize()
    g_want = _flat_grads(model)
    model.store.grads.fill_(float("nan"))          # whatever a range held before: produced or cleared
    loss_dict = model(None, weak_batched_inputs=weak, train_only_weak=True)
    assert sorted(loss_dict) == [str(n) for n in FX["ow/loss_names"]]
    sum(loss_dict.values()).backward()
    torch.cuda.synchronize()
    names = model.loss_names
    for k, v in loss_dict.items():
        assert v.item() == want[names.index(k)].item(), k
    g = _flat_grads(model)
    live = torch.zeros(g.numel(), dtype=torch.bool)
    for e in model.store.entries:
        if e["param"].requires_grad:
            live[e["offset"]:e["offset"] + e["numel"]] = True
    assert torch.equal(g[live].view(torch.int32), g_want[live].view(torch.int32))
    with pytest.raises(RuntimeError, match="expects d\\(total\\)/d\\(loss_i\\) == 1"):
        (2.0 * sum(model(None, weak_batched_inputs=weak, train_only_weak=True).values())).backward()


@pytest.mark.parametrize("case", ["ow", "ow_single", "ow_reg"])
def test_module_level_roi_heads_equal_the_fused_step(dev, case):
    """WSROIHeadNoMeta.forward(None, None, None, None, weak_images=..., weak_features=..., weak_proposals=..., weak_targets=...,
    train_only_weak=True) in training mode, driven the way the reference's meta-architecture drives it (rcnn.py:452, :468-470, :482), on the
    fused step's own feature map and proposals: (None, losses) with an autograd graph; losses, head gradients and d(loss)/d(features)
    against the fused weak-only step (the bars of the module-level test of tests/test_unit_golden_gpu.py: 1e-6 / 1e-5 of the largest entry)"""
    from unit_amd import ops
    from unit_amd.structures import Boxes, ImageList, Instances
    cfg, model, weak = W.only_weak_inputs(case, device="cuda")
    model.train()
    model.compute_mode = "fp32"
    rh = model.roi_heads
    rh.compute_dtype = torch.float32
    batch = model.pack_batch(None, weak)
    step = model.forward_train_only_weak(batch)
    model.backward_train_only_weak(step)
    torch.cuda.synchronize()
    fused = dict(zip(model.loss_names, step.losses.cpu().tolist()))
    head_params = {n: q for n, q in rh.named_parameters() if q.requires_grad}
    g_fused = {n: q.grad.detach().clone() for n, q in head_params.items()}
    props, _, pcount = step.proposals
    sizes = step.image_sizes
    feats = ops.nhwc_to_nchw(ops.as_f32(step.feat).contiguous()).requires_grad_(True)
    weak_props = [Instances(tuple(sizes[i]), proposal_boxes=Boxes(props[i, :int(pcount[i])].clone())) for i in range(len(weak))]
    images = ImageList(feats, [tuple(s) for s in sizes])
    for q in head_params.values():
        q.grad.zero_()          # the module-level nodes ACCUMULATE into .grad (torch semantics)
    res, losses = rh(None, None, None, None, weak_images=images, weak_features={"res4": feats}, weak_proposals=weak_props,
                     weak_targets=[x["instances"].gt_classes.to(dev) for x in weak], train_only_weak=True)
    assert res is None and sorted(losses) == [str(n) for n in FX[f"{case}/loss_names"]]
    assert all(v.requires_grad for v in losses.values())
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    for k, v in losses.items():
        assert abs(v.item() - fused[k]) <= 1e-6 * max(1.0, abs(fused[k])), (case, k, v.item(), fused[k])
    dead = {str(n) for n in FX[f"{case}/dead_names"]}
    checked = 0
    for n, q in head_params.items():
        if "roi_heads." + n in dead:
            assert not q.grad.any(), n
            continue
        ref = g_fused[n]
        assert (q.grad - ref).abs().max().item() <= 1e-5 * ref.abs().max().item() + 1e-8, (case, n)
        checked += 1
    assert checked >= 18 and feats.grad is not None and feats.grad.abs().sum().item() > 0


def test_one_bf16_step_beside_the_fp32_step(dev):
    a, b = _run("ow", steps=1), _run("ow", dtype="bf16", steps=1)
    names = [str(n) for n in FX["ow/loss_names"]]
    fa, fb = torch.tensor([a["losses"][0][k] for k in names]), torch.tensor([b["losses"][0][k] for k in names])
    print("fp32", fa.tolist(), "bf16", fb.tolist())
    assert torch.isfinite(fb).all()
    assert torch.allclose(fb, fa, rtol=BF16_RTOL, atol=BF16_ATOL), (fa, fb)
    dead = [str(n) for n in FX["ow/dead_names"]]
    for n in dead:
        assert torch.equal(b["final"][n], b["start"][n]), n


# ---------------------------------------------------------------------------------------------------- 6. edge cases
def _edge_step(weak, post_nms=None, case="ow"):
    cfg, model, _ = W.only_weak_inputs(case, device="cuda")
    if post_nms is not None:
        model.proposal_generator.post_nms_topk = {True: post_nms, False: model.proposal_generator.post_nms_topk[False]}
    model.train()
    model.compute_mode = "fp32"
    batch = model.pack_batch(None, weak)
    step = model.forward_train_only_weak(batch)
    model.backward_train_only_weak(step)
    torch.cuda.synchronize()
    return model, step, dict(zip(model.loss_names, step.losses.cpu().tolist()))


def _finite_and_fed(model, losses, case="ow"):
    dead = {str(n) for n in FX[f"{case}/dead_names"]}
    for k in ("loss_im_cls", "loss_oicr_1", "loss_oicr_2", "loss_oicr_3"):
        assert np.isfinite(losses[k]) and losses[k] > 0, (k, losses[k])
    for n, q in _trainable(model).items():
        assert torch.isfinite(q.grad).all(), n
        assert bool(q.grad.any()) == (n not in dead), n


def test_weak_image_with_fewer_proposals_than_rois(dev):
    """POST_NMS_TOPK_TRAIN 10 < the 16 RoIs per image: the unused RoI slots are invalid rows that feed no loss and no gradient"""
    _, _, weak = W.only_weak_inputs("ow", device="cuda")
    model, step, losses = _edge_step(weak, post_nms=10)
    counts = step.proposals[2].cpu()
    assert (counts <= 10).all() and (counts > 0).all()
    valid = step.weak_valid.cpu().view(2, -1)
    assert valid.shape[1] == 16 and ((valid == 0).sum(1) == counts).all() and ((valid == -1).sum(1) == 16 - counts).all()          # 0 = a RoI, -1 = unused slot
    _finite_and_fed(model, losses)


def test_single_weak_image(dev):
    _, _, weak = W.only_weak_inputs("ow", device="cuda")
    model, step, losses = _edge_step(weak[:1])
    assert step.n_weak == 1 and step.rw == 16 and step.rs == 0
    _finite_and_fed(model, losses)


def test_weak_images_of_two_sizes(dev):
    """a 96 x 128 and an 80 x 112 weak image: padded to the larger one, as ImageList.from_tensors does (rcnn.py:451)"""
    from unit_amd.synthetic import synthetic_batch
    _, _, weak = W.only_weak_inputs("ow", device="cuda")
    _, small = synthetic_batch(1, 1, hw=(80, 112), num_classes=20, seed=31, max_gt=3)
    model, step, losses = _edge_step([weak[0], small[0]])
    assert [tuple(int(v) for v in s) for s in step.image_sizes] == [(96, 128), (80, 112)] and not step.split
    _finite_and_fed(model, losses)
    rois = step.rois.cpu()
    second = rois[rois[:, 0] == 1][step.weak_valid.cpu()[rois[:, 0] == 1] == 0]
    assert len(second) > 0 and (second[:, 3] <= 112).all() and (second[:, 4] <= 80).all()          # clipped to its own size


# ---------------------------------------------------------------------------------------------------- 7. TrainerOnlyWeakFineTune
def test_trainer_only_weak_finetune_is_the_default_step_on_the_classifier_batch(dev):
    """engine/defaults.py:416: the classifier loader's batch as the supervised batch, no weak batch == TrainerNoMeta.run_step(batch, None) bit
    for bit, optimizer state included; both loaders are drawn from"""
    import gen_ref_step as S
    from unit_amd import engine
    res = []
    for cls in (engine.TrainerOnlyWeakFineTune, engine.TrainerNoMeta):
        cfg, model, sup, _, perms, _ = S.step_inputs("s1", device="cuda")
        model.train()
        model.compute_mode = "fp32"
        drawn = []
        base = iter(lambda: drawn.append("base") or "dropped", None)
        classifier = iter(lambda: drawn.append("classifier") or sup, None)
        tr = cls(cfg, model, data_iter=base, weak_data_iter=classifier) if cls is engine.TrainerOnlyWeakFineTune else cls(cfg, model)
        batch = model.pack_batch(sup, None)
        cap = cfg.MODEL.RPN.POST_NMS_TOPK_TRAIN + batch.gt_boxes.shape[1]
        roi = torch.stack([torch.cat([p, torch.arange(len(p), cap)]) for p in perms["roi"]])
        tr.fixed_permutations = {"rpn": torch.stack(perms["rpn"]).int().to(dev), "roi": roi.int().to(dev)}
        for _ in range(2):
            losses = tr.run_step() if cls is engine.TrainerOnlyWeakFineTune else tr.run_step(sup, None)
        torch.cuda.synchronize()
        if cls is engine.TrainerOnlyWeakFineTune:
            assert drawn == ["base", "classifier"] * 2
        res.append((losses.cpu().clone(), model.store.params.cpu().clone(), tr.optimizer.momentum_buffer().cpu().clone(), tr.optimizer.iter))
    a, b = res
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and a[3] == b[3] == 2
    assert a[0][0] > 0 and a[0][6] > 0 and a[0][2] == 0          # supervised and RPN losses, no weak loss


# ---------------------------------------------------------------------------------------------------- 8. data parallel, world size 1
def test_forced_collectives_at_world_1_end_bit_equal(dev, tmp_path):
    """three weak-only steps with every bucket's exchange forced through RCCL (one rank) in a fresh child process: bit-equal to the run
    without collectives; every bucket was announced in the mode's sequence and finish() left nothing waiting"""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out = str(tmp_path / "res.json")
    p = subprocess.run([sys.executable, os.path.join(HERE, "only_weak_world1_worker.py"), str(port), out], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    r = json.load(open(out))
    assert r["active"] and r["launched"] >= 2 + 3 * len(r["sequence"]), r
    assert r["fired"] == r["sequence"] * 3 and r["left_waiting"] == 0
    assert r["finite"] and r["bit_equal"] and r["loss_equal"], r["max_abs_diff"]
