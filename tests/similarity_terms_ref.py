"""Shared by the similarity-term tests and their fixture's generator: the term lists of tests/golden/similarity_terms_golden.npz, the
upstream gradient of its backward cases, and a numpy restatement of WSROIHead.get_similarity_matrices (the reference's
modeling/roi_heads/roi_heads.py:245-336) that test_similarity_terms_cpu.py holds against every fixture matrix."""
import numpy as np

# name -> one term list for every head, under "Sum"
SUM_CASES = {
    "topk3": ["TopK-3"],
    "wtopk3": ["WTopK-3"],
    "lsda4": ["LSDA-4"],
    "visualk2": ["VisualK-2"],
    "average": ["Average"],
    "none": ["None"],
    "l_topk3": ["lingual", "TopK-3"],
    "l_visualk2": ["lingual", "VisualK-2"],
    "l_v_lsda2": ["lingual", "visual", "LSDA-2"],
    "l_average": ["lingual", "Average"],
    "l_none": ["lingual", "None"],
    "wtopk5_topk3": ["WTopK-5", "TopK-3"],          # first-match k: the TopK term takes k = 5 from "WTopK-5"
}
PRODUCT_CASES = {"prod_l": ["lingual"], "prod_lv": ["lingual", "visual"]}
MIX = {"cls": ["lingual", "VisualK-2"], "bbox": ["TopK-3"], "seg": ["lingual"]}          # stored as mix/<head>
GRAD_CASES = ("visualk2", "l_visualk2", "l_v_lsda2")          # the lists with a per-RoI term: recorded autograd gradients
SIZES = {"K20": dict(K=20, D=48), "K80": dict(K=80, D=200)}
ROWS = 70
THRESHOLD = 0.02
# K80: 20 novel x 60 base x 70 rows is 336 KB per fp32 matrix; the per-RoI matrices of that size are stored for these novel rows only
K80_NOVEL_ROWS = (0, 7, 19)
COCO_NOVEL = [0, 1, 2, 3, 4, 5, 6, 8, 14, 15, 16, 17, 18, 19, 39, 56, 57, 58, 60, 62]          # the 20 classes COCO shares with VOC


def per_roi(terms):
    return "visual" in terms or any("VisualK" in x for x in terms)


def upstream(r, n, b):
    """the upstream gradient d(loss)/d(sim) of the backward cases, fp32 [r, n, b]: a fixed pattern with both signs"""
    i = np.arange(r * n * b, dtype=np.float64)
    return (np.cos(0.37 * i + 0.11) + 0.25 * np.sin(0.013 * i)).astype(np.float32).reshape(r, n, b)


def _softmax(x):
    e = np.exp(x - x.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def _first_k(terms, family):
    hits = [x for x in terms if family in x]
    return int(hits[0].split("-")[1]) if hits else 0


def _top(values, k, largest=True):
    """indices of the k largest (smallest) per row, first index on ties"""
    order = np.argsort(-values if largest else values, axis=-1, kind="stable")
    return order[..., :k]


def _scatter(shape, idx, vals, dtype):
    out = np.zeros(shape, dtype)
    np.put_along_axis(out, idx, vals, -1)
    return out


def similarity(terms, combination, lingual, weights, logits, base, novel, threshold=THRESHOLD, dtype=np.float32):
    """terms: one head's list; lingual [n, b]; weights [streams, K + 1, D]; logits [streams, R, K + 1] -> [n, b], or [R, n, b] with a
    per-RoI term (the reference's shapes)"""
    f = dtype
    n, b = len(novel), len(base)
    lingual, weights, logits = lingual.astype(f), weights.astype(f), logits.astype(f)
    K = weights.shape[1] - 1
    sim = np.zeros((n, b), f)
    if combination != "Sum":
        if "visual" in terms:
            sim = np.zeros((logits.shape[1], n, b), f)
        return _softmax(sim) if terms else sim
    if not terms:
        return sim
    w = f(1.0 / len(terms))
    W = weights.mean(0, dtype=f)
    S = W[novel] @ W[base].T
    if "lingual" in terms:
        sim = sim + w * _softmax(lingual)
    k = _first_k(terms, "TopK")
    if k:
        sim = sim + w * _scatter((n, b), _top(S, k), f(1.0), f) / f(k)
    k = _first_k(terms, "WTopK")
    if k:
        idx = _top(S, k)
        t = _scatter((n, b), idx, np.take_along_axis(S, idx, -1), f)
        sim = sim + w * (t / t.sum(-1, keepdims=True))
    k = _first_k(terms, "LSDA")
    if k:
        dist = np.sqrt(((W[novel][:, None, :] - W[base][None, :, :]) ** 2).sum(-1))
        sim = sim + w * _scatter((n, b), _top(dist, k, largest=False), f(1.0), f) / f(k)
    p = logits.mean(0, dtype=f)
    k = _first_k(terms, "VisualK")
    if k:
        q = _softmax(p[:, :K])[:, base]
        m = q / np.maximum(q.sum(-1, keepdims=True), f(1e-9))
        idx = _top(m, k)
        t = _scatter(m.shape, idx, np.take_along_axis(m, idx, -1), f)
        sim = sim[None] + w * (t / t.sum(-1, keepdims=True))[:, None, :]
    if "visual" in terms:
        q = _softmax(p)[:, base]
        m = q / np.maximum(q.sum(-1, keepdims=True), f(1e-9))
        m = np.where(m < f(threshold), f(0), m)
        sim = sim[None] + w * m[:, None, :]
    if "Average" in terms:
        sim = np.full(sim.shape, f(1.0) / f(b), f)
    if "None" in terms:
        return np.zeros(sim.shape, f)
    return sim / np.maximum(sim.sum(-1, keepdims=True), f(1e-9))
