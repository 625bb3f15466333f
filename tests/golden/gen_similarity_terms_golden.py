"""Generates tests/golden/similarity_terms_golden.npz by RUNNING THE REFERENCE'S OWN WSROIHead.get_similarity_matrices
(modeling/roi_heads/roi_heads.py:245-336) through d2_stubs and gen_unit_golden.bare_roi_head, as gen_unit_golden.py case D does, for
every term list of tests/similarity_terms_ref.py (TopK / WTopK / LSDA / VisualK / Average / None, mixes with lingual and visual, a
per-head mix, and "Product"), at K = 20 (15 base / 5 novel, D = 48) and K = 80 (60 / 20, D = 200), on 70 RoIs and on one.

Per size <S> in (K20, K80):
  <S>/base, novel, coco_indexer, lingual [n, b], oicr_weight [3, K+1, D], oicr_bias [3, K+1], logits [3, 70, K+1] (what evaluation() returns)
  <S>/sim/<case>[/<head>]        fp32, [n, b] or [70, n, b] as the reference returns it (K80 per-RoI matrices: novel rows K80_NOVEL_ROWS only,
                                 the file has to stay under 1 MiB)
  <S>/sim1/<case>[/<head>]       the same call on the first RoI alone, per-RoI lists only
  <S>/sim64/<case>[/<head>]      the same arithmetic in float64 ([n, b]; per-RoI lists: on the first RoI alone)
  <S>/grad/<case>                [3, 70, K+1]: autograd's gradient on each refinement stream's logits (retain_grad on what evaluation() returns,
                                 head in training mode) of sum(sim * upstream(70, n, b)), for the lists with a per-RoI term
The generator ASSERTS the margins that let decisions compare exactly (k-th against (k+1)-th value, distance of every `visual` value from the
threshold, magnitude of WTopK's row sums). Only numeric arrays are written.   Run:  python tests/golden/gen_similarity_terms_golden.py"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import gen_unit_golden as gu  # noqa: E402
import similarity_terms_ref as ref  # noqa: E402
from unit_amd.modeling.roi_heads import _COCO  # noqa: E402

OUT = os.path.join(HERE, "similarity_terms_golden.npz")
RH = gu.REF["roi_heads"]
gu.d2._MetadataCatalog.table["coco_stub_train"] = gu.d2._Metadata(list(_COCO))


def margin(values, k, largest=True):
    """smallest relative gap between the k-th and the (k+1)-th value of a row"""
    v = np.sort(np.asarray(values, np.float64), -1)
    v = v[..., ::-1] if largest else v
    if k >= v.shape[-1]:
        return np.inf
    return float((np.abs(v[..., k - 1] - v[..., k]) / np.maximum(np.abs(v[..., k - 1]), np.abs(v[..., k]))).min())


def check_margins(tag, W, logits, base, novel, K):
    """the decisions of every fixture list, on float64 restatements of the values they are taken on"""
    W64 = W.astype(np.float64).mean(0)
    S = W64[novel] @ W64[base].T
    dist = np.sqrt(((W64[novel][:, None] - W64[base][None]) ** 2).sum(-1))
    for k in (3, 5):
        assert margin(S, k) >= 1e-4, (tag, "TopK", k, margin(S, k))
    for k in (2, 4):
        assert margin(dist, k, largest=False) >= 1e-4, (tag, "LSDA", k, margin(dist, k, False))
    for k in (3, 5):
        top = -np.sort(-S, -1)[:, :k]
        assert np.abs(top.sum(-1)).min() >= 0.1, (tag, "WTopK row sum", k, np.abs(top.sum(-1)).min())
    p = logits.astype(np.float64).mean(0)
    q = ref._softmax(p[:, :K])[:, base]
    m = q / q.sum(-1, keepdims=True)
    assert margin(m, 2) >= 1e-5, (tag, "VisualK", margin(m, 2))
    q = ref._softmax(p)[:, base]
    m = q / q.sum(-1, keepdims=True)
    assert np.abs(m - ref.THRESHOLD).min() >= 1e-5, (tag, "visual threshold", np.abs(m - ref.THRESHOLD).min())


def run(pred, terms, combination, K, base, novel, dataset, bf, train=False, G=None):
    head = gu.bare_roi_head(RH.WSROIHeadNoMeta, pred, terms, K, base, novel, dataset=dataset)
    head.similarity_combination = combination
    if not train:
        head.eval()
        with torch.no_grad():
            return head.get_similarity_matrices(bf)
    head.train()
    wh = pred.weak_detector_head
    orig, seen = wh.evaluation, []

    def spy(x):
        r = orig(x)
        for t in r[0][0]:
            t.retain_grad()
        seen.append(r[0][0])
        return r
    wh.evaluation = spy
    try:
        sim = head.get_similarity_matrices(bf)
    finally:
        del wh.evaluation
    assert len(seen) == 1
    (sim["cls"] * G).sum().backward()
    return sim, torch.stack([t.grad for t in seen[0]], 0)


def case_size(out, tag, K, D, seed):
    g = torch.Generator().manual_seed(seed)
    if K == 20:
        base, novel, dataset = list(gu.VOC_BASE), list(gu.VOC_NOVEL), "voc_stub_train"
    else:
        novel, dataset = list(ref.COCO_NOVEL), "coco_stub_train"
        base = [c for c in range(K) if c not in novel]
    pred = gu.make_predictor("SupervisedDetectorOutputsBase", K, D, g, base, novel)
    bf = torch.randn(ref.ROWS, D, generator=g)
    wh = pred.weak_detector_head
    W = np.stack([gu.npy(l.weight) for l in wh.oicr_predictors], 0)
    with torch.no_grad():
        logits = np.stack([gu.npy(t) for t in wh.evaluation(bf)[0][0]], 0)
    check_margins(tag, W, logits, base, novel, K)
    head = gu.bare_roi_head(RH.WSROIHeadNoMeta, pred, {"cls": ["lingual"]}, K, base, novel, dataset=dataset)
    out[f"{tag}/base"], out[f"{tag}/novel"], out[f"{tag}/coco_indexer"] = np.array(base), np.array(novel), np.asarray(head._coco_indexer)
    with torch.no_grad():
        out[f"{tag}/lingual"] = gu.npy(pred.get_similarity(head._base_classes_tensor, head._novel_classes_tensor, head._coco_indexer_tensor))
    out[f"{tag}/oicr_weight"] = W
    out[f"{tag}/oicr_bias"] = np.stack([gu.npy(l.bias) for l in wh.oicr_predictors], 0)
    out[f"{tag}/logits"] = logits
    pred64 = gu.copy.deepcopy(pred).double()
    G = torch.from_numpy(ref.upstream(ref.ROWS, len(novel), len(base)))
    keep = list(ref.K80_NOVEL_ROWS) if K == 80 else None

    def store(name, terms_by_head, combination):
        sim = run(pred, terms_by_head, combination, K, base, novel, dataset, bf)
        sim1 = run(pred, terms_by_head, combination, K, base, novel, dataset, bf[:1])
        torch.set_default_dtype(torch.float64)
        try:
            sim64 = run(pred64, terms_by_head, combination, K, base, novel, dataset, bf[:1].double())
        finally:
            torch.set_default_dtype(torch.float32)
        for h in terms_by_head:
            sfx = name if len(terms_by_head) == 1 else f"{name}/{h}"
            v = gu.npy(sim[h])
            assert v.dtype == np.float32 and gu.npy(sim64[h]).dtype == np.float64
            if v.ndim == 3:
                out[f"{tag}/sim1/{sfx}"] = gu.npy(sim1[h])
                if keep is not None:
                    v = v[:, keep]
            else:
                assert np.array_equal(v, gu.npy(sim1[h]))
            out[f"{tag}/sim/{sfx}"] = v
            out[f"{tag}/sim64/{sfx}"] = gu.npy(sim64[h])

    for name, terms in ref.SUM_CASES.items():
        store(name, {"cls": terms}, "Sum")
    for name, terms in ref.PRODUCT_CASES.items():
        store(name, {"cls": terms}, "Product")
    store("mix", ref.MIX, "Sum")
    for name in ref.GRAD_CASES:
        sim, grad = run(pred, {"cls": ref.SUM_CASES[name]}, "Sum", K, base, novel, dataset, bf, train=True, G=G)
        v = gu.npy(sim["cls"])
        assert np.array_equal(v if keep is None else v[:, keep], out[f"{tag}/sim/{name}"])
        out[f"{tag}/grad/{name}"] = gu.npy(grad)
        pred.zero_grad()
    print(tag, "ok:", sum(k.startswith(tag) for k in out), "arrays")


def main():
    out = {}
    for i, (tag, s) in enumerate(ref.SIZES.items()):
        case_size(out, tag, s["K"], s["D"], seed=2024 + i * 1007)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
