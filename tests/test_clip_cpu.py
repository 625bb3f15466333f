"""Gradient clipping and Nesterov (unit_amd/solver.py, csrc/optim.hip) without a GPU: the cfg keys, what FlatSGD accepts and refuses, the
table of trainable tensors the kernels take, and the replay-safety of the new exports of include/unit_hip.h."""
import ctypes

import pytest

from unit_amd import _lib, config, engine, ops
from unit_amd.modeling import build_model
from unit_amd.solver import FlatSGD, clip_config, clip_table

NEW_EXPORTS = ("unit_grad_clip_coefs", "unit_sgd_step")


def small_cfg():
    c = config.voc_rcnn_c4_split1(50)
    c.MODEL.DEVICE = "cpu"
    c.MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE = 32
    c.MODEL.RPN.PRE_NMS_TOPK_TRAIN, c.MODEL.RPN.POST_NMS_TOPK_TRAIN = 600, 100
    return c


@pytest.fixture(scope="module")
def model():
    m = build_model(small_cfg())
    m.train()
    return m


def test_clip_gradients_defaults_are_detectron2s():
    c = config.voc_rcnn_c4_split1()
    node = c.SOLVER.CLIP_GRADIENTS
    assert dict(node) == dict(ENABLED=False, CLIP_TYPE="value", CLIP_VALUE=1.0, NORM_TYPE=2.0)
    assert clip_config(c) is None
    c.SOLVER.CLIP_GRADIENTS.ENABLED = True
    assert clip_config(c) == ("value", 1.0, 2.0)
    c.merge_from_list(["SOLVER.CLIP_GRADIENTS.CLIP_TYPE", "norm", "SOLVER.CLIP_GRADIENTS.NORM_TYPE", "inf", "SOLVER.CLIP_GRADIENTS.CLIP_VALUE", "5"])
    assert clip_config(c) == ("norm", 5.0, float("inf"))


@pytest.mark.parametrize("key,bad", [("CLIP_TYPE", "foo"), ("NORM_TYPE", 3.0)])
def test_flatsgd_refuses_unknown_clip_and_norm_types(model, key, bad):
    c = small_cfg()
    c.SOLVER.CLIP_GRADIENTS.ENABLED = True
    c.SOLVER.CLIP_GRADIENTS.CLIP_TYPE = "norm"
    c.SOLVER.CLIP_GRADIENTS[key] = bad
    with pytest.raises(ValueError, match=key):
        FlatSGD(model, c)


@pytest.mark.parametrize("ctype", ["value", "norm", "full_model"])
@pytest.mark.parametrize("norm", [1.0, 2.0, float("inf")])
def test_flatsgd_accepts_every_documented_combination(model, ctype, norm):
    c = small_cfg()
    c.SOLVER.CLIP_GRADIENTS = config.CN(ENABLED=True, CLIP_TYPE=ctype, CLIP_VALUE=0.5, NORM_TYPE=norm)
    o = FlatSGD(model, c)
    assert o.clip == (ctype, 0.5, norm)
    assert o._clip_mode == (ops.CLIP_VALUE if ctype == "value" else ops.CLIP_COEF)


def test_cfg_without_the_node_means_disabled(model):
    c = small_cfg()
    del c.SOLVER["CLIP_GRADIENTS"]
    o = FlatSGD(model, c)
    assert o.clip is None and o._clip_mode == ops.CLIP_NONE and not o.nesterov


def test_nesterov_is_accepted_and_needs_momentum(model):
    c = small_cfg()
    c.SOLVER.NESTEROV = True
    assert FlatSGD(model, c).nesterov
    c.SOLVER.MOMENTUM = 0.0
    with pytest.raises(ValueError, match="[Nn]esterov"):
        FlatSGD(model, c)


def test_full_model_refuses_the_early_update(model):
    c = small_cfg()
    c.SOLVER.CLIP_GRADIENTS = config.CN(ENABLED=True, CLIP_TYPE="full_model", CLIP_VALUE=1.0, NORM_TYPE=2.0)
    with pytest.raises(ValueError, match="full_model"):
        engine.TrainerNoMeta(c, model, early_update=True)
    with pytest.raises(ValueError, match="full_model"):
        FlatSGD(model, c).step_tag("heads")


def test_table_rows_are_the_trainable_tensors_inside_one_bucket_each(model):
    st = model.flatten_parameters()
    names, rows = clip_table(st)
    trainable = [e for e in st.entries if e["param"].requires_grad]
    assert names == [e["name"] for e in trainable] and rows == [(e["offset"], e["numel"]) for e in trainable]
    assert set(names) == {n for n, p in model.named_parameters() if p.requires_grad}
    assert len(rows) > 50 and any(o % 4 for o, _ in rows)          # packed fused heads start at any element
    for (o0, n0), (o1, n1) in zip(rows, rows[1:]):
        assert n0 > 0 and n1 > 0 and o0 + n0 <= o1          # strictly increasing, disjoint
    assert rows[-1][0] + rows[-1][1] <= st.size
    for o, n in rows:
        assert sum(a <= o and o + n <= b for _, a, b in st.tags) == 1
    # the optimizer's view of the same store: its row lookup returns whole tensors for every bucket range and refuses a cut
    o = FlatSGD(model, small_cfg())
    assert o._bind() is st and o.names == names and o._chunk_prefix[-1] == sum(ops.clip_chunks(n) for _, n in rows)
    seen = []
    for _, a, b in st.tags:
        r0, r1 = o._rows_in(a, b)
        seen += list(range(r0, r1))
        assert all(a <= rows[r][0] and rows[r][0] + rows[r][1] <= b for r in range(r0, r1))
    assert seen == list(range(len(rows)))
    big = max(range(len(rows)), key=lambda r: rows[r][1])
    with pytest.raises(AssertionError):
        o._rows_in(0, rows[big][0] + 1)


def test_new_exports_are_replay_safe_and_exported():
    """every new export that takes a stream fits the call-list record of csrc/replay.hip (<= 32 integer-class and <= 8 float arguments, no
    double, no struct by value), the recorder treats it as a launch, and the built library exports it"""
    protos = _lib.parse_header()
    with open(_lib.HEADER) as f:
        text = f.read()
    for name in NEW_EXPORTS:
        _, argtypes = protos[name]
        assert argtypes[-1] is ctypes.c_void_p and _lib.enqueues(name), name
        assert ctypes.c_double not in argtypes, name
        n_flt = sum(t is ctypes.c_float for t in argtypes)
        assert n_flt <= _lib.UnitCall.FLOATS and len(argtypes) - n_flt <= _lib.UnitCall.INTS, name
        decl = text[text.index(name + "("):]
        decl = decl[:decl.index(");")]
        assert "struct" not in decl and "double" not in decl, name
    for name in ("unit_grad_clip_workspace_bytes", "unit_grad_clip_chunk"):
        assert name in protos and not _lib.enqueues(name)
    l = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_EXPORTS + ("unit_grad_clip_workspace_bytes", "unit_grad_clip_chunk"):
        assert hasattr(l, name), name
    lib = _lib.lib()
    assert lib.unit_grad_clip_chunk() == ops.CLIP_CHUNK
    assert lib.unit_grad_clip_workspace_bytes(10 * ops.CLIP_CHUNK + 1, 7) >= 8 * (10 + 7)
    # argument errors come back as a status, before any launch
    assert lib.unit_grad_clip_coefs(None, 0, None, 0, 0, 0, 0, 2, 1.0, 1.0, 0, None, None, None, 0, None) == -1
    assert lib.unit_sgd_step(None, None, None, 0, 4, 0.1, 0.9, 0.0, 1.0, 0.0, 0, 0, 0, None, 0, None, None, None) == -1
