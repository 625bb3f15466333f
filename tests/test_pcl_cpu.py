"""PCL (weak detector TYPE "PCL") on the host: the numpy restatement of the k-means that the reference's get_top_ranking_proposals runs
(tests/golden/pcl_kmeans.py) against scikit-learn itself, the loss fixture's internal consistency, the recipe that regenerates it, and the
replay-safety of the PCL exports of include/unit_hip.h."""
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

GOLD = np.load(os.path.join(GDIR, "pcl_golden.npz"))


def _cases(seed, count, kinds=(0, 1, 2, 3)):
    """random 1-D score vectors, N = 3..1024 (one in three below 40; N > 256 splits sklearn's Lloyd into chunks): uniform; MIL-like
    scores with half of them clamped at 1e-9; four distinct values with a near tie; one softmax column of random logits;
    kind 4: only two distinct values (1e-9 and 0.3)"""
    g = np.random.default_rng(seed)
    for t in range(count):
        n = int(g.integers(3, 1025)) if t % 3 else int(g.integers(3, 40))
        kind = kinds[t % len(kinds)]
        if kind == 0:
            p = g.random(n).astype(np.float32)
        elif kind == 1:
            p = np.clip(g.random(n).astype(np.float32) ** 8, 1e-9, 1 - 1e-9).astype(np.float32)
            p[g.random(n) < 0.5] = np.float32(1e-9)
        elif kind == 2:
            p = g.choice(np.array([1e-9, 0.25, 0.7, 0.7001], np.float32), n)
        elif kind == 3:
            lg = g.normal(size=(n, 21)).astype(np.float32) * 3
            e = np.exp(lg - lg.max(1, keepdims=True))
            p = (e / e.sum(1, keepdims=True))[:, 3].astype(np.float32)
        else:
            p = g.choice(np.array([1e-9, 0.3], np.float32), n)
        yield p


def _mismatches(cases):
    sk = pytest.importorskip("sklearn.cluster")
    import warnings
    bad = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for p in cases:
            km = sk.KMeans(n_clusters=3, random_state=3).fit(p[:, None])
            ref = np.where(km.labels_ == np.argmax(km.cluster_centers_))[0]
            lab, cen = pk.kmeans3(p)
            if not np.array_equal(ref, np.where(lab == int(np.argmax(cen)))[0]):
                bad.append(len(p))
    return bad


def test_kmeans_restatement_matches_sklearn():
    """the top-ranking sets (members of the cluster with the largest centre) of 2000 fits agree with sklearn's"""
    bad = _mismatches(_cases(7, 2000))
    assert not bad, f"top-ranking sets differ from sklearn at N = {bad}"


@pytest.mark.xfail(strict=True, reason="known gap (DESIGN.md section 8): with two distinct values sklearn relocates an empty cluster to "
                   "a point chosen by numpy's SIMD argpartition among equal distances, whose tie order the restatement does not reproduce")
def test_kmeans_restatement_two_valued_inputs():
    bad = _mismatches(_cases(11, 300, kinds=(4,)))
    assert not bad, f"{len(bad)} of 300 two-valued fits differ from sklearn"


def test_kmeans_draws_are_data_independent():
    rs = np.random.RandomState(3)
    u = pk.draws()
    assert u.shape == (7,) and u[0] == rs.random_sample() and np.array_equal(u[1:4], rs.uniform(size=3))
    assert np.array_equal(u[4:], rs.uniform(size=3))


def test_numpy_pairwise_sum_restated():
    g = np.random.default_rng(1)
    for n in (1, 5, 8, 9, 100, 129, 200, 257, 1000, 1024):
        a = g.random(n).astype(np.float32)
        assert pk.np_sum32(a) == np.add.reduce(a.reshape(-1, 1), axis=0)[0], n


@pytest.mark.parametrize("tag,K", [("P20", 20), ("P20n", 20), ("P80", 80), ("P20r", 20)])
def test_pcl_fixture_is_consistent(tag, K):
    """the reference's recorded PCL decisions obey compute_pcl_loss_inputs' bookkeeping, and the recorded loss is PCLFunction's formula"""
    sizes = GOLD[f"{tag}/sizes"].tolist()
    for it in range(3):
        lg = GOLD[f"{tag}/it{it}/logits"]
        assert lg.shape == (sum(sizes), K + 1) and GOLD[f"{tag}/it{it}/grad_logits"].shape == lg.shape
        assert np.isfinite(GOLD[f"{tag}/it{it}/grad_logits"]).all()
        o, total = 0, 0.0
        for i, n in enumerate(sizes):
            f = lambda k: GOLD[f"{tag}/it{it}/{k}{i}"]
            lab, w, ga, pcl, cnt, icw, pcp = (f(k) for k in ("labels", "cls_weights", "gt_assignment", "pc_labels", "pc_count",
                                                               "img_cls_weights", "pc_probs"))
            assert len(lab) == len(w) == len(ga) == n and (w >= 0).all()
            assert set(pcl.tolist()) == set(GOLD[f"{tag}/targets{i}"].tolist())
            assert np.array_equal(np.unique(pcl), pcl[np.sort(np.unique(pcl, return_index=True)[1])])    # clusters in class order
            fg = lab < K
            assert (ga[fg] >= 0).all() and (ga[~fg] == -1).all() and np.array_equal(lab[fg], pcl[ga[fg]])
            assert np.array_equal(cnt, np.bincount(ga[ga >= 0], minlength=len(pcl)))
            np.testing.assert_allclose(icw, np.bincount(ga[fg], weights=w[fg], minlength=len(pcl)), rtol=1e-5, atol=1e-7)
            x = lg[o:o + n].astype(np.float64)
            p = np.exp(x - x.max(1, keepdims=True))
            p /= p.sum(1, keepdims=True)
            with np.errstate(invalid="ignore", divide="ignore"):
                total += -(np.sum(w[~fg] * np.log(p[~fg, K])) + np.sum(icw * np.log(pcp))) / n
            o += n
        np.testing.assert_allclose(total / len(sizes), GOLD[f"{tag}/it{it}/loss"], rtol=1e-5, equal_nan=True)
    if tag == "P20r":                   # two clusters on one box: an empty cluster, NaN as the reference computes it
        assert any((GOLD[f"{tag}/it{it}/pc_count0"] == 0).any() and np.isnan(GOLD[f"{tag}/it{it}/loss"]) for it in range(3))


@pytest.mark.skipif(not os.path.isdir("/root/reference/modeling"), reason="the reference tree exists only in the authoring container")
def test_pcl_recipe_reproduces_the_committed_fixture(tmp_path):
    out = str(tmp_path / "regen")
    r = subprocess.run([sys.executable, os.path.join(GDIR, "gen_pcl_golden.py"), out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    new = np.load(os.path.join(out, "pcl_golden.npz"))
    assert sorted(new.files) == sorted(GOLD.files)
    for k in GOLD.files:
        a, b = new[k], GOLD[k]
        assert a.dtype == b.dtype and a.shape == b.shape, k
        if a.dtype.kind == "f":
            np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-6, err_msg=k)
        else:
            assert np.array_equal(a, b), k


def test_pcl_exports_are_replay_safe():
    """every PCL export that takes a stream fits the call-list record of csrc/replay.hip: at most 32 integer-class and 8 float
    arguments, no double and no struct by value"""
    from unit_amd import _lib
    protos = {k: v for k, v in _lib.parse_header().items() if k.startswith("unit_pcl_")}
    assert "unit_pcl_loss" in protos
    for name, (_, argtypes) in protos.items():
        assert argtypes[-1] is ctypes.c_void_p, name
        assert ctypes.c_double not in argtypes, name
        n_flt = sum(t is ctypes.c_float for t in argtypes)
        assert n_flt <= _lib.UnitCall.FLOATS and len(argtypes) - n_flt <= _lib.UnitCall.INTS, name
    with open(_lib.HEADER) as f:
        text = f.read()
    for name in protos:
        decl = text[text.index(name + "("):]
        decl = decl[:decl.index(");")]
        assert "struct" not in decl and "double" not in decl, name
