"""PCL targets (weak detector TYPE "PCL") on the host: the numpy restatement of the canonical rule (tests/golden/pcl_targets.py) against
the reference's own recording under a stable argsort (tests/golden/pcl_targets_golden.npz, `stable/...`) and, on tie-free units, against
the unmodified reference (`ref/...`); condition C1 of the fixture; its agreement with pcl_golden.npz; the recipe that regenerates it; the
kernel's draw constants; the replay-safety of the unit_pcl_targets export; and the model switch."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GDIR = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GDIR)
import pcl_kmeans as pk  # noqa: E402
import pcl_targets as pt  # noqa: E402

G = np.load(os.path.join(GDIR, "pcl_targets_golden.npz"))
OLD = np.load(os.path.join(GDIR, "pcl_golden.npz"))
TAGS = pt.tags(G)
SMALL = ("P20", "P20n", "P80", "P20r", "S16", "S40")


def _units(tag):
    sizes = G[f"{tag}/sizes"].tolist()
    return [(it, i) for it in range(3) for i in range(len(sizes))]


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_equals_the_stable_reference(tag):
    """every unit: integers and cls_weights exactly, img_cls_weights / pc_probs within rtol 1e-5; on tie-free units that is the
    unmodified reference too"""
    sizes, K = G[f"{tag}/sizes"].tolist(), int(G[f"{tag}/K"])
    off = np.insert(np.cumsum(sizes), 0, 0)
    for it in range(3):
        p0, p1 = pt.case_probs(G, tag, it)
        for i, n in enumerate(sizes):
            r = slice(off[i], off[i + 1])
            got = pt.image_targets(G[f"{tag}/boxes{i}"], p0[r], p1[r], G[f"{tag}/targets{i}"].tolist(), K)
            assert not got["poisoned"]
            pt.check_unit(got, pt.expected(G, tag, it, i, "stable"), f"{tag} it{it} image {i} (stable)")
            if int(G[f"{tag}/it{it}/tie_free{i}"]):
                pt.check_unit(got, pt.expected(G, tag, it, i, "ref"), f"{tag} it{it} image {i} (ref)")


def test_fixture_condition_c1():
    """at least 36 tie-free units, among them every unit of the six small cases; the flag is what it says; the canonical rule has its own
    test: a case whose every unit depends on the tie order"""
    free = {t: [int(G[f"{t}/it{it}/tie_free{i}"]) for it, i in _units(t)] for t in TAGS}
    assert sum(sum(v) for v in free.values()) >= 36
    assert all(all(free[t]) for t in SMALL)
    assert not any(free["L20u"])
    for t in TAGS:
        for (it, i), f in zip(_units(t), free[t]):
            differs = any(f"{t}/it{it}/ref/{k}{i}" in G.files for k in pt.KEYS)
            assert differs == (not f), (t, it, i)


@pytest.mark.parametrize("tag", pt.SHARED)
def test_shared_cases_equal_the_loss_fixture(tag):
    """`ref/...` of the four cases both fixtures hold is pcl_golden.npz's recording"""
    sizes = G[f"{tag}/sizes"].tolist()
    assert sizes == OLD[f"{tag}/sizes"].tolist()
    for i in range(len(sizes)):
        assert np.array_equal(G[f"{tag}/boxes{i}"], OLD[f"{tag}/boxes{i}"])
    for it, i in _units(tag):
        exp = pt.expected(G, tag, it, i, "ref")
        for k in pt.KEYS:
            a, b = exp[k], OLD[f"{tag}/it{it}/{k}{i}"]
            assert a.shape == b.shape and np.array_equal(a, b.astype(a.dtype), equal_nan=a.dtype.kind == "f"), (tag, it, i, k)
    for it in range(3):
        np.testing.assert_array_equal(G[f"{tag}/it{it}/stable/loss"], OLD[f"{tag}/it{it}/loss"])
        if it > 0:          # the probabilities handed over are the softmax of the recorded logits
            np.testing.assert_allclose(G[f"{tag}/it{it - 1}/probs_next"], pt.softmax(OLD[f"{tag}/it{it - 1}/logits"]), rtol=2e-6, atol=1e-9)


@pytest.mark.skipif(not os.path.isdir("/root/reference/modeling"), reason="the reference tree exists only in the authoring container")
def test_recipe_reproduces_the_committed_fixture(tmp_path):
    out = str(tmp_path / "regen")
    r = subprocess.run([sys.executable, os.path.join(GDIR, "gen_pcl_targets_golden.py"), out], capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    new = np.load(os.path.join(out, "pcl_targets_golden.npz"))
    assert sorted(new.files) == sorted(G.files)
    for k in G.files:
        a, b = new[k], G[k]
        assert a.dtype == b.dtype and a.shape == b.shape, k
        if a.dtype.kind == "f":
            np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-6, err_msg=k)
        else:
            assert np.array_equal(a, b), k


def test_fixture_is_small():
    assert os.path.getsize(os.path.join(GDIR, "pcl_targets_golden.npz")) < 1000000


def test_restatement_rules_for_rejected_inputs():
    """zero-area boxes (no self-edge: the reference raises) poison the image and the loop ends; an image without a class has no cluster"""
    g = np.random.default_rng(5)
    n, K = 24, 20
    b = np.zeros((n, 4), np.float32)
    b[:, :2] = g.random((n, 2)) * 50
    b[:, 2], b[:, 3] = b[:, 0], b[:, 1] + 40            # zero width
    p0, p1 = g.random((n, K)).astype(np.float32), pt.softmax(g.normal(size=(n, K + 1)))
    r = pt.image_targets(b, p0, p1, [3, 8], K)
    assert r["poisoned"] and np.isnan(r["cls_weights"]).all() and len(r["pc_labels"]) == 0 and (r["labels"] == K).all()
    b[:, 2] = b[:, 0] + 30
    r = pt.image_targets(b, p0, p1, [], K)
    assert not r["poisoned"] and len(r["pc_labels"]) == 0 and (r["labels"] == K).all() and (r["cls_weights"] == 0).all()
    r = pt.image_targets(b, p0, p1, [3, 8], K)
    assert not r["poisoned"] and set(r["pc_labels"].tolist()) == {3, 8} and np.isfinite(r["cls_weights"]).all()


def test_kernel_draw_constants_equal_the_restatement():
    """the seven RandomState(3) doubles that csrc/pcl.hip carries as constants (host-only export unit_kmeans_draws), bit for bit"""
    from unit_amd import _lib
    bits = (ctypes.c_ulonglong * 7)()
    assert _lib.lib().unit_kmeans_draws(bits) == 0
    got = np.frombuffer(bytes(bits), dtype=np.float64)
    assert np.array_equal(got.view(np.uint64), pk.draws().view(np.uint64))


def test_pcl_targets_exports_are_replay_safe():
    """test_pcl_cpu.py's check extended to unit_pcl_targets: at most 32 integer-class and 8 float arguments, the stream last, no double and
    no struct by value; its workspace query and the draws export take no stream, so the recorder passes them through"""
    from unit_amd import _lib
    protos, names = _lib.parse_header(), _lib.parse_header_names()
    assert {"unit_pcl_loss", "unit_pcl_targets"} <= {k for k in protos if k.startswith("unit_pcl_")}
    for name in [k for k in protos if k.startswith("unit_pcl_")]:
        _, argtypes = protos[name]
        assert argtypes[-1] is ctypes.c_void_p and names[name][-1] == "stream", name
        assert ctypes.c_double not in argtypes, name
        n_flt = sum(t is ctypes.c_float for t in argtypes)
        assert n_flt <= _lib.UnitCall.FLOATS and len(argtypes) - n_flt <= _lib.UnitCall.INTS, name
    with open(_lib.HEADER) as f:
        text = f.read()
    for name in ("unit_pcl_targets", "unit_workspace_bytes_pcl_targets", "unit_kmeans_draws"):
        decl = text[text.index(name + "("):]
        decl = decl[:decl.index(");")]
        assert "struct" not in decl and "double" not in decl, name
    for name in ("unit_workspace_bytes_pcl_targets", "unit_kmeans_draws"):
        assert "stream" not in names[name]
    assert _lib.lib().unit_workspace_bytes_pcl_targets(2, 512, 3) >= 2 * 3 * 512 * 13 * 4


def _cfg(**kw):
    sys.path.insert(0, GDIR)
    import gen_ref_step as grs
    c = grs.case_cfg("s1")
    wd = c.MODEL.ROI_HEADS.FAST_RCNN.WEAK_DETECTOR
    for k, v in kw.items():
        setattr(wd, k, v)
    return c


def test_build_model_accepts_type_pcl():
    from unit_amd.modeling import build_model
    oicr, pcl = build_model(_cfg()), build_model(_cfg(TYPE="PCL", GRAPH_IOU_THRESHOLD=0.3, MAX_PC_NUM=4))
    assert list(oicr.state_dict().keys()) == list(pcl.state_dict().keys())
    wh = pcl.roi_heads.box_predictor.weak_detector_head
    assert wh.weak_detector_type == "PCL" and wh.graph_iou_threshold == 0.3 and wh.max_pc_num == 4
    assert oicr.roi_heads.box_predictor.weak_detector_head.weak_detector_type == "OICR"
    with pytest.raises(AssertionError, match="NUM_KMEANS_CLUSTER"):
        build_model(_cfg(TYPE="PCL", NUM_KMEANS_CLUSTER=4))
    for branch in ("REGRESSION_BRANCH", "OICR_REGRESSION_BRANCH"):
        for typ in ("PCL", "OICR"):
            with pytest.raises(AssertionError):
                build_model(_cfg(TYPE=typ, **{branch: True}))
    with pytest.raises(AssertionError):
        build_model(_cfg(TYPE="WSDDN"))
