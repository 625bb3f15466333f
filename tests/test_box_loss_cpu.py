"""The two switchable box-regression losses (MODEL.RPN.* / MODEL.ROI_BOX_HEAD.BBOX_REG_LOSS_TYPE and SMOOTH_L1_BETA) without a GPU: what the
RPN and the two predictors accept and refuse, the recipe of tests/golden/box_loss_golden.npz, and the replay-safety of the two new exports of
include/unit_hip.h."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from unit_amd import _lib, config, ops
from unit_amd.modeling.fast_rcnn import SupervisedDetectorOutputsBase, SupervisedDetectorOutputsFineTune
from unit_amd.modeling.rpn import WSRPN
from unit_amd.structures import ShapeSpec

GDIR = os.path.join(os.path.dirname(__file__), "golden")
NEW_EXPORTS = ("unit_box_reg_loss_ex", "unit_rpn_loss_ex")
BUILDERS = {"rpn": (lambda c: WSRPN(c), "RPN"),
            "base": (lambda c: SupervisedDetectorOutputsBase(c, ShapeSpec(channels=64)), "ROI_BOX_HEAD"),
            "finetune": (lambda c: SupervisedDetectorOutputsFineTune(c, ShapeSpec(channels=64)), "ROI_BOX_HEAD")}


def small_cfg():
    c = config.voc_rcnn_c4_split1(50)
    c.MODEL.DEVICE = "cpu"
    return c


@pytest.mark.parametrize("which", list(BUILDERS))
@pytest.mark.parametrize("loss_type,beta", [("smooth_l1", 0.0), ("smooth_l1", 1.0 / 9), ("giou", 0.0), ("giou", 0.5)])
def test_both_types_and_a_positive_beta_construct(which, loss_type, beta):
    build, node = BUILDERS[which]
    c = small_cfg()
    c.MODEL[node].BBOX_REG_LOSS_TYPE, c.MODEL[node].SMOOTH_L1_BETA = loss_type, beta
    m = build(c)
    assert m.box_reg_loss_type == loss_type and m.smooth_l1_beta == beta


@pytest.mark.parametrize("which", list(BUILDERS))
def test_the_defaults_are_detectron2s(which):
    m = BUILDERS[which][0](small_cfg())
    assert (m.box_reg_loss_type, m.smooth_l1_beta) == ("smooth_l1", 0.0)


@pytest.mark.parametrize("which,words", [("rpn", "Invalid rpn box reg loss type 'diou'"), ("base", "Invalid bbox reg loss type 'diou'"),
                                         ("finetune", "Invalid bbox reg loss type 'diou'")])
def test_an_unknown_type_raises_with_the_references_words(which, words):
    build, node = BUILDERS[which]
    c = small_cfg()
    c.MODEL[node].BBOX_REG_LOSS_TYPE = "diou"
    with pytest.raises(ValueError, match=words):
        build(c)


@pytest.mark.parametrize("which", list(BUILDERS))
def test_a_negative_beta_is_refused(which):
    build, node = BUILDERS[which]
    c = small_cfg()
    c.MODEL[node].SMOOTH_L1_BETA = -0.5
    with pytest.raises(ValueError, match="SMOOTH_L1_BETA"):
        build(c)


@pytest.mark.parametrize("which", ["base", "finetune"])
def test_class_agnostic_regression_is_still_refused_with_its_reason(which):
    c = small_cfg()
    c.MODEL.ROI_BOX_HEAD.CLS_AGNOSTIC_BBOX_REG = True
    with pytest.raises(AssertionError, match=r"\[R, K, 4\]"):
        BUILDERS[which][0](c)


def test_rpn_weights_other_than_ones_are_still_refused_with_their_reason():
    c = small_cfg()
    c.MODEL.RPN.BBOX_REG_WEIGHTS = (10.0, 10.0, 5.0, 5.0)
    with pytest.raises(AssertionError, match="rpn_decode_select"):
        WSRPN(c)


def test_the_wrappers_refuse_what_the_modules_refuse():
    for fn, words in ((ops.box_reg_loss, "Invalid bbox reg loss type 'l2'"), (ops.rpn_loss, "Invalid rpn box reg loss type 'l2'")):
        with pytest.raises(ValueError, match=words):
            fn(*[None] * (7 if fn is ops.box_reg_loss else 9), loss_type="l2")
    assert ops._box_loss_args("smooth_l1", 0.0, "bbox reg") is None          # Detectron2's default keeps its own export
    assert ops._box_loss_args("smooth_l1", 1e-6, "bbox reg") == (0, 1e-6) and ops._box_loss_args("giou", 0.0, "bbox reg") == (1, 0.0)


@pytest.mark.skipif(not os.path.isdir("/root/reference/modeling"), reason="the reference tree exists only in the authoring container")
def test_the_generator_reproduces_the_committed_fixture(tmp_path):
    out = str(tmp_path / "regen.npz")
    r = subprocess.run([sys.executable, os.path.join(GDIR, "gen_box_loss_golden.py"), out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    new, old = np.load(out), np.load(os.path.join(GDIR, "box_loss_golden.npz"))
    assert sorted(new.files) == sorted(old.files), set(new.files) ^ set(old.files)
    for k in old.files:
        a, b = new[k], old[k]
        assert a.dtype == b.dtype and a.shape == b.shape, k
        if a.dtype.kind == "f":
            np.testing.assert_allclose(a, b, rtol=1e-6, atol=1e-9, err_msg=k)
        else:
            assert np.array_equal(a, b), k


def test_the_fixture_holds_the_cases_the_kernels_can_go_wrong_at():
    g = np.load(os.path.join(GDIR, "box_loss_golden.npz"))
    shapes = sorted({k.split("/")[1] for k in g.files if k.startswith("box/")})
    assert shapes == sorted(["K20_R1", "K20_R65", "K80_R257", "K20_R700", "K20_R65_nofg"])
    for s in shapes:
        lab, K = g[f"box/{s}/labels"], int(g[f"box/{s}/K"])
        assert lab.shape[0] == int(s.split("_")[1][1:])
        if lab.shape[0] > 8 and not s.endswith("nofg"):
            assert (lab == -1).any() and (lab == K).any() and ((lab >= 0) & (lab < K)).any()
        for kind in ("giou", "sl1_b1e-6", "sl1_b0.111", "sl1_b1"):
            assert f"box/{s}/{kind}/grad/f64" in g.files and g[f"box/{s}/{kind}/grad/f64"].dtype == np.float64
    nofg = g["box/K20_R65_nofg/labels"]
    assert not ((nofg >= 0) & (nofg < 20)).any() and float(g["box/K20_R65_nofg/giou/loss"]) == 0.0
    w, h = g["box/K20_R65/gt"][:, 2] - g["box/K20_R65/gt"][:, 0], g["box/K20_R65/gt"][:, 3] - g["box/K20_R65/gt"][:, 1]
    assert (np.maximum(w, h) < 1.0).any()          # a gt box under 1 px
    clamp = np.log(1000.0 / 16)
    d = g["box/K20_R65/giou/deltas"]
    assert (d[:, 2] / 5.0 > clamp).any() and (d[:, 3] / 5.0 > clamp).any()
    lab = g["rpn/labels"]
    assert lab.shape == (2, 525) and set(np.unique(lab).tolist()) == {-1, 0, 1} and not (lab[1] == 1).any() and (lab[0][512:] == 1).any()
    assert g["rpn/gt"].shape == (2, 8, 4) and g["rpn/giou_w/weights"].tolist() == [0.5, 2.0]
    d = g["rpn/giou/deltas"]
    assert (d[..., 2] > clamp).any() and (d[..., 3] > clamp).any()
    for kind, beta in (("sl1_b1e-6", 1e-6), ("sl1_b0.111_w", 1.0 / 9), ("sl1_b1", 1.0)):
        assert abs(float(g[f"rpn/{kind}/beta"]) - beta) < 1e-7 * max(beta, 1e-6) * 10


def test_new_exports_are_replay_safe_and_exported():
    """the two new exports fit the call-list record of csrc/replay.hip (<= 32 integer-class and <= 8 float arguments, no double, no struct by
    value, the stream last), the recorder treats them as launches, the built library exports them, and argument errors come back as a status"""
    protos = _lib.parse_header()
    with open(_lib.HEADER) as f:
        text = f.read()
    for name in NEW_EXPORTS:
        _, argtypes = protos[name]
        assert argtypes[-1] is ctypes.c_void_p and _lib.enqueues(name) and _lib.parse_header_names()[name][-1] == "stream", name
        assert ctypes.c_double not in argtypes, name
        n_flt = sum(t is ctypes.c_float for t in argtypes)
        assert n_flt <= _lib.UnitCall.FLOATS and len(argtypes) - n_flt <= _lib.UnitCall.INTS, name
        decl = text[text.index(name + "("):]
        decl = decl[:decl.index(");")]
        assert "struct" not in decl and "double" not in decl, name
    assert sum(t is ctypes.c_float for t in protos["unit_rpn_loss_ex"][1]) == 5
    # the plain forms' arguments, then (int loss_type, float beta), then the stream
    for ex, plain in (("unit_box_reg_loss_ex", "unit_box_reg_loss"), ("unit_rpn_loss_ex", "unit_rpn_loss_w")):
        assert protos[ex][1] == protos[plain][1][:-1] + [ctypes.c_int, ctypes.c_float, ctypes.c_void_p]
    assert "#define UNIT_BOXLOSS_SMOOTH_L1 0" in text and "#define UNIT_BOXLOSS_GIOU 1" in text
    assert ops.BOX_LOSS_TYPES == {"smooth_l1": 0, "giou": 1}
    l = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_EXPORTS + ("unit_box_reg_loss", "unit_rpn_loss", "unit_rpn_loss_w"):
        assert hasattr(l, name), name
    lib = _lib.lib()
    w = (ctypes.c_float * 4)(10.0, 10.0, 5.0, 5.0)
    for loss_type, beta, words in ((2, 0.0, "loss_type"), (-1, 0.0, "loss_type"), (0, -1.0, "beta"), (1, float("nan"), "beta")):
        assert lib.unit_box_reg_loss_ex(None, 0, 0, 20, None, None, None, w, 0, 1.0, None, None, 0, 0, 0, None, loss_type, beta, None) == -1
        assert words in lib.unit_last_error().decode()
        assert lib.unit_rpn_loss_ex(None, 0, 15, 15, None, None, None, 8, None, 0, 0, 1.0, 1.0, 1.0, 1.0, None, None, 0, None, 0, loss_type, beta,
                                    None) == -1
        assert words in lib.unit_last_error().decode()
