"""The weak-only training mode (TrainerOnlyWeak, engine/defaults.py:377-400; `train_only_weak=True`, meta_arch/rcnn.py:433) without a GPU:
the fixture tests/golden/only_weak_golden.npz (the reference's own forward + solver for three iterations, gen_only_weak_golden.py) and its
preconditions, the CPU oracle's weak half against it, every refusal with its message, the trainers' signatures and data-draw order against
the reference's source text, the live-mask function against the reference's `.grad is None` names, and the gradient buckets of the weak-only
tag sequence on gloo (world size 2)."""
import inspect
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GDIR = os.path.join(ROOT, "tests", "golden")
for p_ in (GDIR, os.path.join(ROOT, "oracle")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)
import gen_only_weak_golden as W  # noqa: E402

FX = np.load(os.path.join(GDIR, "only_weak_golden.npz"))
HAS_REF = os.path.isdir("/root/reference/modeling")
REF_ENGINE = "/root/reference/engine/defaults.py"


# ---------------------------------------------------------------------------------------------------- the fixture
def test_fixture_conditions_hold():
    """every dead tensor bit-equal to its initial value, a live tensor of backbone / Res5 head / weak predictor moved, the dead set holds
    rpn_head and the delta predictors (in "ow" and "ow_reg" also box_head), the reference's loss keys, no permutation drawn"""
    W.check_conditions(FX)
    assert set(W.CASES) == {"ow", "ow_single", "ow_reg"} and W.STEPS == 3
    assert all(FX[k].dtype.kind in "fiuU" for k in FX.files)          # numeric arrays and name lists only


def test_fixture_records_no_gradient_for_a_dead_tensor():
    for case in W.CASES:
        dead = {str(n) for n in FX[f"{case}/dead_names"]}
        for it in range(W.STEPS):
            have = {k.split("/gradnorm/")[1] for k in FX.files if k.startswith(f"{case}/it{it}/gradnorm/")}
            assert not (have & dead), (case, it, have & dead)
            assert "backbone.res4.5.conv1.weight" in have and "backbone.res3.0.conv2.weight" in have
            assert ("roi_heads.weak_box_head.res5.2.conv3.weight" in have) == (case != "ow_single")
            assert ("roi_heads.box_head.res5.0.conv2.weight" in have) == (case == "ow_single")


@pytest.mark.skipif(not HAS_REF, reason="the reference tree exists only in the authoring container")
def test_generator_reproduces_the_committed_fixture(tmp_path):
    out = str(tmp_path / "regen.npz")
    r = subprocess.run([sys.executable, os.path.join(GDIR, "gen_only_weak_golden.py"), out], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    new = np.load(out)
    assert sorted(new.files) == sorted(FX.files)
    for k in FX.files:
        a, b = new[k], FX[k]
        assert a.dtype == b.dtype and a.shape == b.shape, k
        if a.dtype.kind == "f":          # (test_golden_recipe_cpu.py: bit for bit but for torch's thread-pool re-association)
            np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-6, err_msg=k)
        else:
            assert np.array_equal(a, b), k


@pytest.mark.parametrize("case", ["ow", "ow_single", "ow_reg"])
def test_cpu_oracle_weak_half_gives_the_fixture_losses(case):
    """oracle/unit_oracle.py step_losses' weak half (its lines under `if weak_images is not None`) on the fixture inputs, restated with the
    oracle's own functions because step_losses cannot run without supervised images: iteration 0's loss_im_cls and loss_oicr_* (the
    oracle has no regression branch: "ow_reg" is compared on these four, its two further losses against the fixture on the device)"""
    import gen_ref_step as S
    import unit_oracle as orc
    cfg, model, weak = W.only_weak_inputs(case)
    p = S.oracle_params(model)
    o = S.oracle_cfg(cfg)
    with torch.no_grad():
        wx, wsizes = orc.preprocess_image([x["image"] for x in weak], o["pixel_mean"], o["pixel_std"])
        wfeat = orc.resnet_c4(wx, p, o["depth"], "backbone.")
        wlog, wdel = orc.rpn_head(wfeat, p)
        wprops = orc.find_top_rpn_proposals(orc.grid_anchors(*wfeat.shape[-2:]), wlog, wdel, wsizes, pre_nms_topk=o["pre_nms_topk"],
                                            post_nms_topk=o["post_nms_topk"])
        wboxes = [b[:o["rois_per_image"]] for (b, _) in wprops]
        wpooled = orc.roi_align(wfeat, orc.boxes_to_rois(wboxes))
        wbf = orc.res5_head(wpooled, p, "roi_heads.weak_box_head" if o["multi_box_head"] else "roi_heads.box_head")
        cs, ds, oicr = orc.weak_head_forward_train(wbf, p, "roi_heads.box_predictor.weak_detector_head")
        losses = orc.weak_losses(cs, ds, oicr, wboxes, [x["instances"].gt_classes for x in weak], num_classes=o["num_classes"])
    names = [str(n) for n in FX[f"{case}/loss_names"]]
    assert sorted(losses) == [n for n in names if "regression" not in n]
    got = np.array([losses[k].item() for k in sorted(losses)])
    want = np.array([v for n, v in zip(names, FX[f"{case}/losses"][0]) if "regression" not in n])
    print(case, "oracle", got, "fixture", want)
    # the bar at which the fixtures reproduce themselves (tests/test_golden_recipe_cpu.py:28)
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-6)


# ---------------------------------------------------------------------------------------------------- the live mask
@pytest.mark.parametrize("case", W.CASES)
def test_live_entries_are_the_parameters_the_reference_gives_a_gradient(case):
    from unit_amd.solver import clip_table
    cfg, model, _ = W.only_weak_inputs(case)
    model.train()
    live = model.live_entries(False, True)
    names, rows = clip_table(model.store)
    assert len(live) == len(names) == len(rows)
    assert sorted(names) == [str(n) for n in FX[f"{case}/names"]]
    assert sorted(n for n, l in zip(names, live) if not l) == [str(n) for n in FX[f"{case}/dead_names"]]
    # a pure function of (supervised batch?, weak batch?): both batches feed everything, the modes only differ in the flags
    assert all(model.live_entries(True, True))
    no_weak = {n for n, l in zip(names, model.live_entries(True, False)) if not l}
    assert no_weak and all(".weak_detector_head." in n or n.startswith("roi_heads.weak_box_head.") for n in no_weak)
    # every bucket is reported once in the weak-only mode, the fed ones first
    seq = model.only_weak_tag_sequence()
    tags = list(dict.fromkeys(t for t, _, _ in model.store.tags))
    assert sorted(seq) == sorted(tags) and len(set(seq)) == len(seq)
    assert seq[0] == "heads" and seq[-1] == "rpn" and ("box_head" in seq[-2:]) == (case != "ow_single")


def test_masked_sgd_bookkeeping_without_a_device():
    """MaskedFlatSGD.set_live: a wrong length is refused, a mask is uploaded once per distinct value, an update without a mask is an error,
    and FlatSGD itself knows nothing of masks"""
    from unit_amd.solver import FlatSGD, MaskedFlatSGD
    cfg, model, _ = W.only_weak_inputs("ow")
    model.train()
    assert not hasattr(FlatSGD, "set_live") and issubclass(MaskedFlatSGD, FlatSGD)
    opt = MaskedFlatSGD(model, cfg)
    live = model.live_entries(False, True)
    with pytest.raises(ValueError, match="flags for the"):
        opt.set_live(live[:-1])
    with pytest.raises(RuntimeError, match="before every step"):
        opt._apply(opt._bind(), 0, 8)
    opt.set_live(live)
    assert opt._live == tuple(live) and opt._live_dev.dtype == torch.uint8 and opt._live_dev.tolist() == [int(x) for x in live]
    assert opt._mask_table.shape == (len(live), 2) and opt._mask_table[:, 0].tolist() == opt._row_off
    first = opt._live_dev
    opt.set_live(live)
    assert opt._live_dev is first          # uploaded once per distinct mask
    model.flatten_parameters()
    with pytest.raises(RuntimeError, match="re-flattened after set_live"):
        opt._apply(opt._bind(), 0, 8)


def test_header_declares_the_masked_entry():
    from unit_amd import _lib
    protos, names = _lib.parse_header(), _lib.parse_header_names()
    assert names["unit_sgd_step_masked"] == names["unit_sgd_step"][:-2] + ["live"] + names["unit_sgd_step"][-2:]
    assert _lib.enqueues("unit_sgd_step_masked") and len(protos["unit_sgd_step_masked"][1]) == len(protos["unit_sgd_step"][1]) + 1
    hdr = open(_lib.HEADER).read()
    assert ".grad is None" in hdr[hdr.index("unit_sgd_step_masked:"): hdr.index("int unit_grad_clip_chunk")]


# ---------------------------------------------------------------------------------------------------- refusals
def _weak_model(case="s1", meta=None):
    import gen_ref_step as S
    from unit_amd.modeling import build_model
    from unit_amd.synthetic import synthetic_batch
    cfg = S.case_cfg(case)
    if meta:
        cfg.MODEL.META_ARCHITECTURE = meta
    model = build_model(cfg).train()
    sup, weak = synthetic_batch(1, 1, hw=S.HW, num_classes=cfg.MODEL.ROI_HEADS.NUM_CLASSES, seed=5, max_gt=2)
    return cfg, model, sup, weak


def test_refusals_of_the_step_name_the_reference_line():
    from unit_amd.modeling.inference import UnsupportedConfig
    cfg, model, sup, weak = _weak_model()
    with pytest.raises(NotImplementedError, match=r"only the ROI heads read the flag.*rcnn.py:463-464"):
        model(sup, weak_batched_inputs=weak, train_only_weak=True)
    with pytest.raises(ValueError, match="needs weak_batched_inputs"):
        model(None, weak_batched_inputs=None, train_only_weak=True)
    model._x3 = True          # (what compute_mode = "bf16x3" sets; the setter itself re-plans the layers)
    with pytest.raises(NotImplementedError, match="bf16x3"):
        model(None, weak_batched_inputs=weak, train_only_weak=True)
    model._x3 = False
    for case, cls, pat in (("mask", "WSROIHeadNoMetaWithMask", r"_forward_mask\(None, None, box_features=None\).*roi_heads.py:813"),
                           ("mask_ft", "WSROIHeadWithMaskFineTune", r"roi_heads.py:813"),
                           ("s2", "WSROIHeadFineTune", r"get_similarity_matrices\(None\).*roi_heads.py:618")):
        _, m, _, w = _weak_model(case)
        assert type(m.roi_heads).__name__ == cls
        with pytest.raises(UnsupportedConfig, match=pat):
            m(None, weak_batched_inputs=w, train_only_weak=True)
        with pytest.raises(UnsupportedConfig, match=pat):          # the module-level surface refuses the same way
            m.roi_heads(None, None, None, None, weak_images=None, weak_features=torch.zeros(1), weak_proposals=[], weak_targets=[],
                        train_only_weak=True)
    _, rpn, _, w = _weak_model(meta="WeaklySupervisedRCNNRPN")
    with pytest.raises(NotImplementedError, match=r"preprocesses batched_inputs unconditionally.*rcnn.py:550"):
        rpn(None, weak_batched_inputs=w, train_only_weak=True)
    with pytest.raises(NotImplementedError, match="rcnn.py:463-464"):
        model.roi_heads(None, torch.zeros(1), [], [], weak_features=torch.zeros(1), weak_proposals=[], weak_targets=[], train_only_weak=True)


def test_trainers_refuse_graph_and_replay_at_construction():
    from unit_amd import engine
    cfg, model, _, _ = _weak_model()
    for kw in ({"use_graph": True}, {"use_replay": True}):
        with pytest.raises(NotImplementedError, match="runs eagerly only.*GraphedStep / ReplayedStep"):
            engine.TrainerOnlyWeak(cfg, model, **kw)


def test_the_predictor_level_none_input_stays_refused():
    """`_forward_values(None, ...)` of the base predictor keeps its NotImplementedError (tests/test_finetune_regression_cpu.py pins the
    fine-tune class's)"""
    _, model, _, _ = _weak_model()
    with pytest.raises(NotImplementedError, match="train_only_weak"):
        model.roi_heads.box_predictor._forward_values(None, [], [])


def test_run_step_without_a_weak_loader_says_so():
    from unit_amd import engine
    cfg, model, _, _ = _weak_model()
    for cls in (engine.TrainerOnlyWeak, engine.TrainerOnlyWeakFineTune):
        with pytest.raises(ValueError, match="no weak_data_iter to draw one from"):
            cls(cfg, model).run_step()


# ---------------------------------------------------------------------------------------------------- trainers
def test_trainers_are_exported_beside_trainer_finetune_and_documented():
    from unit_amd import engine
    assert issubclass(engine.TrainerOnlyWeak, engine.TrainerNoMeta) and issubclass(engine.TrainerOnlyWeakFineTune, engine.TrainerNoMeta)
    for cls in (engine.TrainerOnlyWeak, engine.TrainerOnlyWeakFineTune):
        assert str(inspect.signature(cls.run_step)) == str(inspect.signature(engine.TrainerNoMeta.run_step))
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "TrainerOnlyWeak" in doc and "TrainerOnlyWeakFineTune" in doc


class _Packed(Exception):
    pass


class _Loader:
    def __init__(self, name, log, item):
        self.name, self.log, self.item = name, log, item

    def __next__(self):
        self.log.append(self.name)
        return self.item


def _draw_order_and_call(cls_name):
    """(order of the two next() calls, the model call) of <cls_name>.run_step in the reference's source text"""
    txt = open(REF_ENGINE).read()
    body = txt[txt.index(f"class {cls_name}("):]
    body = body[:body.index("\nclass ", 10)]
    draws = re.findall(r"next\(self\.(_\w+)\)", body)
    call = re.search(r"self\.model\((.*)\)", body).group(1)
    return draws, call


def test_run_step_draws_from_both_loaders_in_the_reference_order(monkeypatch):
    """engine/defaults.py:387-388 / :412-413: base loader first, then the classifier loader; what reaches the model is :391 / :416"""
    from unit_amd import engine
    cfg, model, sup, weak = _weak_model()
    for cls, want in ((engine.TrainerOnlyWeak, ("weak_only", None, "W")), (engine.TrainerOnlyWeakFineTune, ("default", "W", None))):
        log, seen = [], []
        tr = cls(cfg, model, data_iter=_Loader("base", log, "B"), weak_data_iter=_Loader("classifier", log, "W"))
        def pack_batch(a, b=None, **k):          # the step itself needs the device: stop where the batches reach the model
            seen.append((a, b))
            raise _Packed()
        monkeypatch.setattr(model, "pack_batch", pack_batch)
        with pytest.raises(_Packed):
            tr.run_step()
        assert log == ["base", "classifier"], (cls.__name__, log)
        assert seen == [(want[1], want[2])], (cls.__name__, seen)
        monkeypatch.undo()
    if os.path.isfile(REF_ENGINE):
        draws, call = _draw_order_and_call("TrainerOnlyWeak")
        assert draws == ["_data_loader_iter", "_classifier_data_loader_iter"]
        assert call.replace(" ", "") == "None,weak_batched_inputs=classifier_data,train_only_weak=True"
        draws, call = _draw_order_and_call("TrainerOnlyWeakFineTune")
        assert draws == ["_data_loader_iter", "_classifier_data_loader_iter"]
        assert call.replace(" ", "") == "classifier_data,weak_batched_inputs=None,train_only_weak=False"


def test_returned_loss_names_of_the_mode():
    from unit_amd.modeling.rcnn import PackedBatch
    for case in W.CASES:
        cfg, model, _ = W.only_weak_inputs(case)
        b = PackedBatch([torch.zeros(3, 8, 8)] * 2, None, None, None, 0, multihot=torch.zeros(2, 20, dtype=torch.uint8))
        assert sorted(model.only_weak_loss_names) == [str(n) for n in FX[f"{case}/loss_names"]]
        # a step that merely lacks the supervised batch keeps the dictionary it returned before
        assert model._returned_losses(b) == model.loss_names


# ---------------------------------------------------------------------------------------------------- data parallel on gloo
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from unit_amd.parallel import GradBuckets
        _, model, _ = W.only_weak_inputs("ow")
        model.train()
        st = model.flatten_parameters()
        buckets = GradBuckets(model, bucket_bytes=8 << 20)
        live = model.live_entries(False, True)
        ents = [e for e in st.entries if e["param"].requires_grad]
        pat = torch.arange(st.size, dtype=torch.float32) % 97
        for l, e in zip(live, ents):          # dead ranges travel as the zeros _clear_unproduced wrote
            if not l:
                pat[e["offset"]:e["offset"] + e["numel"]] = 0
        st.grads.copy_(pat * (rank + 1))
        seq = model.only_weak_tag_sequence()
        assert sorted(seq) == sorted(dict.fromkeys(t for t, _, _ in st.tags))
        for tag in seq:
            model.on_grad_ready(tag)
        assert {t for t in buckets._work_tags} == set(seq)          # every bucket was announced: finish() waits for nothing else
        buckets.finish()
        assert buckets._works == [] and buckets._tag_works == {}
        assert torch.equal(st.grads, pat * (world * (world + 1) / 2.0))
        for l, e in zip(live, ents):
            if not l:
                assert not st.grads[e["offset"]:e["offset"] + e["numel"]].any()
        q.put((rank, "ok"))
    except Exception:  # noqa
        import traceback
        q.put((rank, traceback.format_exc()))
    finally:
        dist.destroy_process_group()


def test_grad_buckets_of_the_weak_only_tag_sequence_gloo_world2():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=600) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
    for rank, msg in res:
        assert msg == "ok", f"rank {rank}: {msg}"
