"""The similarity terms beyond 'lingual' + 'visual' without a GPU: the plan of every term list of the fixture and every refusal
(modeling/similarity_terms.py, at construction of the ROI heads), the numpy restatement (tests/similarity_terms_ref.py) against every
matrix the reference wrote into tests/golden/similarity_terms_golden.npz, the generator's margins on the committed file, the C ABI."""
import os
import sys

import numpy as np
import pytest

import similarity_terms_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GDIR = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GDIR)
G = np.load(os.path.join(GDIR, "similarity_terms_golden.npz"))


def _plan(terms, combination="Sum", n_base=15):
    from unit_amd.modeling.similarity_terms import parse_terms
    return parse_terms(terms, combination, n_base)


# ---------------------------------------------------------------------------------------------------- the plan
def test_plan_of_every_fixture_list():
    P = {name: _plan(t) for name, t in ref.SUM_CASES.items()}
    flags = lambda p: (p.lingual, p.visual, p.topk, p.wtopk, p.lsda, p.visualk, p.average, p.none)
    assert flags(P["topk3"]) == (False, False, 3, 0, 0, 0, False, False) and P["topk3"].weight == 1.0
    assert flags(P["wtopk3"]) == (False, False, 3, 3, 0, 0, False, False) and P["wtopk3"].weight == 1.0          # "WTopK-3" contains "TopK": both terms
    assert flags(P["lsda4"]) == (False, False, 0, 0, 4, 0, False, False)
    assert flags(P["visualk2"]) == (False, False, 0, 0, 0, 2, False, False) and P["visualk2"].per_roi
    assert flags(P["average"]) == (False, False, 0, 0, 0, 0, True, False) and P["average"].constant and not P["average"].zero
    assert flags(P["none"]) == (False, False, 0, 0, 0, 0, False, True) and P["none"].zero
    assert flags(P["l_topk3"]) == (True, False, 3, 0, 0, 0, False, False) and P["l_topk3"].weight == 0.5
    assert flags(P["l_visualk2"]) == (True, False, 0, 0, 0, 2, False, False) and P["l_visualk2"].weight == 0.5
    assert flags(P["l_v_lsda2"]) == (True, True, 0, 0, 2, 0, False, False) and P["l_v_lsda2"].weight == 1.0 / 3 and P["l_v_lsda2"].per_roi
    assert flags(P["l_average"]) == (True, False, 0, 0, 0, 0, True, False) and not P["l_average"].per_roi
    assert flags(P["l_none"]) == (True, False, 0, 0, 0, 0, False, True) and P["l_none"].zero
    assert flags(P["wtopk5_topk3"]) == (False, False, 5, 5, 0, 0, False, False) and P["wtopk5_topk3"].weight == 0.5          # first-match k
    assert flags(_plan(["TopK-3", "WTopK-5"])) == (False, False, 3, 5, 0, 0, False, False)
    assert not any(p.plain for p in P.values())
    for name, t in ref.PRODUCT_CASES.items():
        p = _plan(t, "Product")
        assert p.product and not p.plain and p.constant and not p.zero and not p.per_roi
    assert [_plan(t).static_key == _plan(ref.MIX["cls"]).static_key for t in (ref.MIX["bbox"], ref.MIX["seg"])] == [False, False]


def test_plain_plans_are_the_two_term_lists_as_before():
    for t, key in ((["lingual", "visual"], (True, True)), (["lingual"], (True, False)), (["visual"], (False, True)), ([], (False, False))):
        p = _plan(t)
        assert p.plain and p.key == key, t
    assert _plan([]).zero and _plan([], "Product").zero and _plan([]).weight == 0.0
    assert not _plan(["lingual", "lingual"]).plain          # weight 1/2 on one term: not what unit_similarity computes
    assert not _plan(["lingual"], "Product").plain


REFUSED = [
    (["lingual", "Visual"], "Sum", "not a similarity term"),
    (["topk-3"], "Sum", "not a similarity term"),
    ([""], "Sum", "not a similarity term"),
    (["TopK"], "Sum", r"k must be an integer in \[1, 15\]"),
    (["TopK-x"], "Sum", "k must be an integer"),
    (["TopK-0"], "Sum", "k must be an integer"),
    (["WTopK-16"], "Sum", "k must be an integer"),
    (["LSDA-2.5"], "Sum", "k must be an integer"),
    (["lingual", "VisualK-99"], "Sum", "k must be an integer"),
    (["visual", "VisualK-2"], "Sum", "4-D tensor"),
    (["lingual"], "Max", "SIMILARITY_COMBINATION 'Max' is not supported"),
    (["Lingual"], "Product", "not a similarity term"),
]


@pytest.mark.parametrize("terms,combination,msg", REFUSED)
def test_parse_terms_refuses(terms, combination, msg):
    from unit_amd.modeling.inference import UnsupportedConfig
    with pytest.raises(UnsupportedConfig, match=msg):
        _plan(terms, combination)


def _cfg(terms, combination="Sum", name="s1", **weak):
    import gen_ref_step as grs
    c = grs.case_cfg(name)
    for k, v in weak.items():
        setattr(c.MODEL.ROI_HEADS.FAST_RCNN.WEAK_DETECTOR, k, v)
    ft = c.MODEL.ROI_HEADS.FINETUNE_TERMS
    ft.CLASSIFIER, ft.BBOX, ft.MASK = list(terms["cls"]), list(terms["bbox"]), list(terms["seg"])
    c.MODEL.ROI_HEADS.VISUAL_ATTENTION_HEAD.SIMILARITY_COMBINATION = combination
    return c


@pytest.mark.parametrize("terms,combination,msg", REFUSED)
def test_refused_at_construction_of_the_roi_heads(terms, combination, msg):
    """today such a yaml builds, trains and evaluates with a zero matrix (or "Sum" for any combination)"""
    from unit_amd.modeling import build_model
    for head in ("cls", "bbox"):
        t = {"cls": ["lingual"], "bbox": ["lingual"], "seg": ["lingual"]}
        t[head] = terms
        with pytest.raises(ValueError, match=msg):
            build_model(_cfg(t, combination))
        with pytest.raises(AssertionError):          # ... like every other refusal at construction
            build_model(_cfg(t, combination))
    t = {"cls": ["lingual"], "bbox": ["lingual"], "seg": terms}          # the mask head's list is read by the ROI heads that have one
    with pytest.raises(ValueError, match=msg):
        build_model(_cfg(t, combination, name="mask"))


def test_visualk_with_the_regression_branch_is_refused():
    from unit_amd.modeling import build_model
    t = {h: ["lingual", "VisualK-2"] for h in ("cls", "bbox", "seg")}
    with pytest.raises(ValueError, match="VisualK.*REGRESSION_BRANCH.*list of refinement streams"):
        build_model(_cfg(t, REGRESSION_BRANCH=True))
    t = {h: ["lingual", "TopK-2", "LSDA-3", "Average"] for h in ("cls", "bbox", "seg")}          # the weight terms do not read evaluation()
    assert build_model(_cfg(t, REGRESSION_BRANCH=True)).roi_heads.term_plans()["cls"].lsda == 3


def test_every_fixture_list_builds_and_keeps_the_combination():
    from unit_amd.modeling import build_model
    m = build_model(_cfg(ref.MIX, name="mask"))
    rh = m.roi_heads
    assert rh.similarity_combination == "Sum" and {h: p.visualk for h, p in rh.term_plans().items()} == {"cls": 2, "bbox": 0, "seg": 0}
    m = build_model(_cfg({h: ["lingual", "visual"] for h in ("cls", "bbox", "seg")}, "Product"))
    assert m.roi_heads.similarity_combination == "Product" and all(p.product for p in m.roi_heads.term_plans().values())


# ---------------------------------------------------------------------------------------------------- the fixture
def _cases():
    for name, t in ref.SUM_CASES.items():
        yield name, name, t, "Sum"
    for name, t in ref.PRODUCT_CASES.items():
        yield name, name, t, "Product"
    for h, t in ref.MIX.items():
        yield f"mix/{h}", f"mix_{h}", t, "Sum"


CASES = list(_cases())


def _inputs(tag):
    return dict(lingual=G[f"{tag}/lingual"], weights=G[f"{tag}/oicr_weight"], logits=G[f"{tag}/logits"], base=G[f"{tag}/base"].tolist(),
                novel=G[f"{tag}/novel"].tolist())


def test_fixture_shapes():
    for tag, s in ref.SIZES.items():
        K, D = s["K"], s["D"]
        n, b = len(G[f"{tag}/novel"]), len(G[f"{tag}/base"])
        assert (n, b) == ((5, 15) if K == 20 else (20, 60))
        assert G[f"{tag}/oicr_weight"].shape == (3, K + 1, D) and G[f"{tag}/logits"].shape == (3, ref.ROWS, K + 1) and G[f"{tag}/lingual"].shape == (n, b)
        kept = n if K == 20 else len(ref.K80_NOVEL_ROWS)
        for key, _, t, comb in CASES:
            rows = ref.per_roi(t) if comb == "Sum" else "visual" in t
            v = G[f"{tag}/sim/{key}"]
            assert v.dtype == np.float32 and v.shape == ((ref.ROWS, kept, b) if rows else (n, b)), (tag, key, v.shape)
            assert G[f"{tag}/sim64/{key}"].dtype == np.float64 and G[f"{tag}/sim64/{key}"].shape == ((1, n, b) if rows else (n, b))
            assert (f"{tag}/sim1/{key}" in G.files) == rows
        for name in ref.GRAD_CASES:
            assert G[f"{tag}/grad/{name}"].shape == (3, ref.ROWS, K + 1)


@pytest.mark.parametrize("tag", list(ref.SIZES))
@pytest.mark.parametrize("key,_id,terms,combination", CASES, ids=[c[1] for c in CASES])
def test_numpy_restatement_reproduces_the_reference(tag, key, _id, terms, combination):
    inp = _inputs(tag)
    want = G[f"{tag}/sim/{key}"]
    got = ref.similarity(terms, combination, **inp)
    if want.ndim == 3 and tag == "K80":
        got = got[:, list(ref.K80_NOVEL_ROWS)]
    assert got.shape == want.shape and got.dtype == np.float32
    assert np.array_equal(got != 0, want != 0)
    if any("WTopK" in x for x in terms):
        # its values are dot products over D, summed here in another order than torch.mm's: 4 x the reference's own fp32 error against
        # the float64 evaluation, floor 1e-6 (the GPU test's rule)
        w64 = G[f"{tag}/sim64/{key}"]
        bound = max(4 * float(np.abs(want - w64).max()), 1e-6)
        assert float(np.abs(got - w64).max()) <= bound, (float(np.abs(got - w64).max()), bound)
    else:
        np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-7)
    one = {**inp, "logits": inp["logits"][:, :1]}
    if want.ndim == 3:
        np.testing.assert_allclose(ref.similarity(terms, combination, **one), G[f"{tag}/sim1/{key}"], rtol=1e-5, atol=1e-7)
    got64 = ref.similarity(terms, combination, **one, dtype=np.float64)
    # (the float64 evaluation computed the refinement logits and the lingual matrix in float64, the restatement reads the fixture's fp32
    #  ones: a 300-term dot product of magnitude <= ~40 in fp32 is off by ~1e-5 absolute, which is the relative error it leaves in a softmax
    #  value; the weight terms read the same fp32 weights on both sides)
    rounded_inputs = want.ndim == 3 or "lingual" in terms
    np.testing.assert_allclose(got64, G[f"{tag}/sim64/{key}"], rtol=1e-4 if rounded_inputs else 1e-12, atol=1e-15)


def test_results_the_issue_names():
    for tag in ref.SIZES:
        b = len(G[f"{tag}/base"])
        for key in ("prod_l", "prod_lv", "average", "l_average"):          # "Product" is softmax(0) whatever the terms; Average overwrites
            np.testing.assert_allclose(G[f"{tag}/sim/{key}"], 1.0 / b, rtol=1e-6)
        for key in ("none", "l_none"):
            assert not G[f"{tag}/sim/{key}"].any()
        assert np.array_equal((G[f"{tag}/sim/topk3"] != 0).sum(-1), np.full(len(G[f"{tag}/novel"]), 3))
        assert np.array_equal((G[f"{tag}/sim/wtopk5_topk3"] != 0).sum(-1), np.full(len(G[f"{tag}/novel"]), 5))


def _margin(values, k, largest=True):
    v = np.sort(np.asarray(values, np.float64), -1)
    v = v[..., ::-1] if largest else v
    return float((np.abs(v[..., k - 1] - v[..., k]) / np.maximum(np.abs(v[..., k - 1]), np.abs(v[..., k]))).min())


@pytest.mark.parametrize("tag", list(ref.SIZES))
def test_fixture_margins(tag):
    """what lets the kernels' decisions compare exactly with the reference's, re-checked on the committed file"""
    K = ref.SIZES[tag]["K"]
    base, novel = G[f"{tag}/base"], G[f"{tag}/novel"]
    W = G[f"{tag}/oicr_weight"].astype(np.float64).mean(0)
    S = W[novel] @ W[base].T
    dist = np.sqrt(((W[novel][:, None] - W[base][None]) ** 2).sum(-1))
    assert min(_margin(S, 3), _margin(S, 5)) >= 1e-4
    assert min(_margin(dist, 2, False), _margin(dist, 4, False)) >= 1e-4
    for k in (3, 5):
        assert np.abs((-np.sort(-S, -1)[:, :k]).sum(-1)).min() >= 0.1
    p = G[f"{tag}/logits"].astype(np.float64).mean(0)
    q = ref._softmax(p[:, :K])[:, base]
    assert _margin(q / q.sum(-1, keepdims=True), 2) >= 1e-5
    q = ref._softmax(p)[:, base]
    assert np.abs(q / q.sum(-1, keepdims=True) - ref.THRESHOLD).min() >= 1e-5


# ---------------------------------------------------------------------------------------------------- the C ABI
def test_header_declares_the_three_entries():
    from unit_amd import _lib
    names = _lib.parse_header_names()
    plan = ["visual_threshold", "weight", "use_visual", "k_visual", "average", "none", "product"]
    rows = ["lin_weak", "ld", "col0", "n_oicr", "ncls", "base_dev", "n_base", "A", "n_novel"]
    assert names["unit_similarity_static"] == ["w_master", "ld", "row0", "n_oicr", "ncls", "D", "base_dev", "n_base", "novel_dev", "n_novel", "lingual",
                                               "weight", "use_lingual", "k_topk", "k_wtopk", "k_lsda", "A", "stream"]
    assert names["unit_similarity_ex"] == rows + plan + ["sim", "R", "stream"]
    assert names["unit_similarity_bwd_ex"] == rows + plan + ["dsim", "dlin", "dlin_dtype", "ldl", "dcol0", "R", "stream"]
    assert all(_lib.enqueues(n) for n in ("unit_similarity_static", "unit_similarity_ex", "unit_similarity_bwd_ex"))
    with open(os.path.join(ROOT, "include", "unit_hip.h")) as f:
        txt = f.read()
    i, j = txt.index("a14, the remaining similarity terms"), txt.index("a15 detections")
    for cite in ("roi_heads.py:270-305", ":273-283", ":284-294", ":295-305", ":306-315", ":318-320", ":321-324", ":325-332", ":852"):
        assert cite in txt[i:j], cite
    old = {n: names[n] for n in ("unit_similarity", "unit_similarity_bwd")}          # the two-term entries keep their signatures
    assert old["unit_similarity"][-5:] == ["use_lingual", "use_visual", "sim", "R", "stream"] and len(old["unit_similarity_bwd"]) == 19
