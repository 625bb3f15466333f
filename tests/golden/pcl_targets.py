"""numpy restatement of the PCL targets (weak detector TYPE "PCL", compute_pcl_loss_inputs weak_detector_fast_rcnn.py:476-507 with
get_graph_centers :415-463) under the project's canonical rule, on top of pcl_kmeans.py. It is what csrc/pcl.hip's unit_pcl_targets
is compared with where no recording of the reference exists.

The canonical rule: the reference's code under a STABLE argsort. In the greedy loop the FIRST node of maximum
degree is taken; the centres kept are those of descending score, and among equal scores the LATER cluster first.

Rules of this project for inputs the reference rejects:
  * a zero-area box has no self-edge; when no edge is left while more than 5 top-ranking rows remain (the reference raises there) the
    class's loop ends and the image is poisoned: every cls_weight and img_cls_weight of the image becomes NaN, so the loss is NaN;
  * an image without classes: every row background with weight 0, no cluster."""
import numpy as np

import pcl_kmeans as pk

F32 = np.float32
EPS = F32(1e-9)
HI = F32(1.0 - 1e-9)          # == 1.0 in float32, as torch's clamp sees it


def clamp(p):
    return np.minimum(np.maximum(np.asarray(p, F32), EPS), HI).astype(F32)


def iou_matrix(a, b):
    """detectron2's pairwise_iou in float32: inter / (area1 + area2 - inter), 0 where inter == 0"""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    area1 = ((a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])).astype(F32)
    area2 = ((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])).astype(F32)
    w = np.minimum(a[:, None, 2], b[None, :, 2]) - np.maximum(a[:, None, 0], b[None, :, 0])
    h = np.minimum(a[:, None, 3], b[None, :, 3]) - np.maximum(a[:, None, 1], b[None, :, 1])
    inter = (np.maximum(w, F32(0)) * np.maximum(h, F32(0))).astype(F32)
    den = ((area1[:, None] + area2[None, :]).astype(F32) - inter).astype(F32)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(inter > 0, (inter / den).astype(F32), F32(0)).astype(F32)


def graph_centers(boxes, probs, classes, graph_iou_thresh=0.4, max_pc_num=5):
    """-> (centre rows [M] into the image's rows, scores [M] float32, classes [M], poisoned). `probs` already clamped."""
    rows = np.arange(len(boxes))
    c_rows, c_scores, c_cls, poisoned = [], [], [], False
    for c in classes:
        if len(rows) == 0:
            break
        p = probs[rows, c]
        top = pk.top_ranking(p)
        g = iou_matrix(boxes[rows[top]], boxes[rows[top]]) > F32(graph_iou_thresh)
        alive = np.ones(len(top), bool)
        count, keep, score = len(top), [], []
        for _ in range(len(top)):
            deg = (g & alive[None, :] & alive[:, None]).sum(1)
            v = int(np.argmax(deg))                              # first maximum
            nb = np.where(g[v] & alive & alive[v])[0]
            if len(nb) == 0:
                poisoned = True
                break
            keep.append(v)
            score.append(p[top][nb].max())
            alive[nb] = False
            count -= len(nb)
            if count <= 5:
                break
        score = np.array(score, F32)
        order = np.argsort(score, kind="stable")[::-1][:max_pc_num]
        sel = rows[top][np.array(keep, np.int64)[order]] if len(keep) else np.zeros(0, np.int64)
        c_rows += sel.tolist()
        c_scores += score[order].tolist()
        c_cls += [c] * len(sel)
        rows = rows[~np.isin(rows, sel)]
    return np.array(c_rows, np.int64), np.array(c_scores, F32), np.array(c_cls, np.int64), poisoned


def image_targets(boxes, probs, probs_next, classes, K, fg_thresh=0.5, bg_thresh=0.1, graph_iou_thresh=0.4, max_pc_num=5):
    """one image -> dict of the seven outputs of compute_pcl_loss_inputs (labels, cls_weights, gt_assignment, pc_labels, pc_count,
    img_cls_weights, pc_probs). probs [n, >= K] and probs_next [n, K + 1] unclamped; classes ascending and unique."""
    boxes = np.asarray(boxes, F32)
    n = len(boxes)
    probs, probs_next = clamp(probs), clamp(probs_next)
    c_rows, c_scores, c_cls, poisoned = graph_centers(boxes, probs, list(classes), graph_iou_thresh, max_pc_num)
    m = len(c_rows)
    if m == 0:
        labels, w, ga = np.full(n, K, np.int64), np.zeros(n, F32), np.full(n, -1, np.int64)
    else:
        q = iou_matrix(boxes[c_rows], boxes)
        ga = np.argmax(q, 0)                                     # first maximum
        val = q[ga, np.arange(n)]
        labels = np.where(val >= F32(0.5), c_cls[ga], K).astype(np.int64)
        w = np.where(val < F32(bg_thresh), F32(0), c_scores[ga]).astype(F32)
        ga = np.where(val < F32(fg_thresh), -1, ga).astype(np.int64)
    cnt = np.array([(ga == j).sum() for j in range(m)], np.int64)
    icw = np.array([w[ga == j].sum(dtype=F32) for j in range(m)], F32)
    with np.errstate(invalid="ignore", divide="ignore"):
        pcp = np.array([probs_next[ga == j, c_cls[j]].sum(dtype=F32) / F32(cnt[j]) for j in range(m)], F32)
    if poisoned:
        w = np.full(n, np.nan, F32)
        icw = np.full(m, np.nan, F32)
    return dict(labels=labels, cls_weights=w, gt_assignment=ga, pc_labels=c_cls, pc_count=cnt, img_cls_weights=icw, pc_probs=pcp,
                poisoned=poisoned)


def softmax(x):
    x = np.asarray(x, np.float64)
    e = np.exp(x - x.max(1, keepdims=True))
    return (e / e.sum(1, keepdims=True)).astype(F32)


# ---- readers of tests/golden/pcl_targets_golden.npz (layout: gen_pcl_targets_golden.py's docstring)
KEYS = ("labels", "cls_weights", "gt_assignment", "pc_labels", "pc_count", "img_cls_weights", "pc_probs")
INT_KEYS = ("labels", "gt_assignment", "pc_labels", "pc_count")
SHARED = ("P20", "P20n", "P80", "P20r")


def tags(G):
    return [str(t) for t in G["tags"]]


def case_probs(G, tag, it):
    """-> (probs [R, K], probs_next [R, K + 1]) as compute_pcl_loss_inputs received them at iteration `it`; for a sparse case only the
    columns of the image's classes are the recorded values, every other entry is 0 (it never enters the targets)"""
    sizes, K = G[f"{tag}/sizes"].tolist(), int(G[f"{tag}/K"])
    if not int(G[f"{tag}/sparse"]):
        p1 = G[f"{tag}/it{it}/probs_next"]
        p0 = G[f"{tag}/it0/probs"] if it == 0 else G[f"{tag}/it{it - 1}/probs_next"]
        return p0, p1
    p0, p1 = np.zeros((sum(sizes), K if it == 0 else K + 1), F32), np.zeros((sum(sizes), K + 1), F32)
    o = 0
    for i, n in enumerate(sizes):
        cols = G[f"{tag}/it{it}/cols{i}"]
        p0[o:o + n, cols] = G[f"{tag}/it0/probs{i}"] if it == 0 else G[f"{tag}/it{it - 1}/probs_next{i}"]
        p1[o:o + n, cols] = G[f"{tag}/it{it}/probs_next{i}"]
        o += n
    return p0, p1


def expected(G, tag, it, i, run="stable"):
    """the seven recorded outputs of unit (it, image i); a `ref/` array that is absent equals the `stable/` one"""
    out = {}
    for key in KEYS:
        name = f"{tag}/it{it}/{run}/{key}{i}"
        out[key] = G[name] if name in G.files else G[f"{tag}/it{it}/stable/{key}{i}"]
    return out


def recorded(G, OLD, tag, it, what, run="stable"):
    """refinement logits / loss / grad_logits of iteration `it`: from pcl_golden.npz for the four shared cases (asserted equal to both runs
    when the fixture was generated), from this fixture otherwise"""
    if tag in SHARED:
        return OLD[f"{tag}/it{it}/{what}"]
    if what == "logits":
        return G[f"{tag}/it{it}/logits"]
    name = f"{tag}/it{it}/{run}/{what}"
    return G[name] if name in G.files else G[f"{tag}/it{it}/stable/{what}"]


def check_unit(got, exp, where=""):
    """integers and cls_weights exactly, the summed floats within rtol 1e-5 (NaN / inf where the recording has them)"""
    for key in INT_KEYS:
        assert np.array_equal(np.asarray(got[key]).astype(np.int64), exp[key].astype(np.int64)), f"{where} {key}"
    assert np.array_equal(np.asarray(got["cls_weights"], F32), exp["cls_weights"].astype(F32), equal_nan=True), f"{where} cls_weights"
    for key in ("img_cls_weights", "pc_probs"):
        np.testing.assert_allclose(np.asarray(got[key], F32), exp[key], rtol=1e-5, atol=0, equal_nan=True, err_msg=f"{where} {key}")
