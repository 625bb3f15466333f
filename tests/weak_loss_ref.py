"""Plain references of the weak-loss kernels (csrc/losses.hip: unit_wsddn_mil, unit_oicr_targets[_ex], unit_softmax_ce, unit_sup_scores,
unit_sum_losses), written from the reference project's formulas (weak_detector_fast_rcnn.py:202-214, 257-268, 353-408; fast_rcnn.py:425-445)
on the kernels' own layout: images in fixed slots of S rows, valid[row] >= 0 for a live row, live columns at an offset inside wider rows.

Pure torch / numpy on the CPU. mil, oicr_targets and softmax_ce evaluate in float64 (`dtype=torch.float32` gives the same formulas in torch
fp32: the yardstick of the tests' tolerance, test_weak_loss_ops_gpu.py). sup_scores and sum_losses are float32 in the kernels' stated order
and are compared bit for bit.

Two things are fp32 by the reference's own definition and stay so in the float64 evaluation:
  * the clamp bounds of the class vector: the reference clamps an fp32 tensor to (1e-6, 1 - 1e-6), i.e. to float32(1e-6) and float32(1 - 1e-6)
    = 1 - 17 * 2^-24; log(1 - hi) differs by 1.3 % between that and the double 1 - 1e-6
  * an IoU is rounded to fp32 before it meets a threshold, itself float32(fg) / float32(bg): the Matcher sees fp32 IoUs
"""
import numpy as np
import torch
import torch.nn.functional as F

P_LO = float(np.float32(1e-6))
P_HI = float(np.float32(1.0) - np.float32(1e-6))


def live_rows(valid, S, b):
    """-> the row numbers (into [B * S]) of image b's live slots, ascending"""
    v = torch.as_tensor(valid)[b * S:(b + 1) * S]
    return b * S + torch.nonzero(v >= 0)[:, 0]


# ---------------------------------------------------------------------------------------------------- MIL
def mil(streams, ccol0, dcol0, K, valid, S, B, multihot, tc, td, mult, gscale, dtype=torch.float64):
    """x_r = softmax(cls / tc, -1) * softmax(det / td, 0) per image over its live rows; p = clamp(sum_r x_r, 1e-6, 1 - 1e-6);
    loss = mult * mean_{image, class} BCE(p, y). -> (loss [], x_r [B*S, K], d_cls [B*S, K], d_det [B*S, K]) with
    d_* = gscale * d loss / d (raw stream columns), by autograd; empty slots give zero rows; an image without a live row has p = 0"""
    cls = streams[:, ccol0:ccol0 + K].to(dtype).clone()
    det = streams[:, dcol0:dcol0 + K].to(dtype).clone()
    rows = [live_rows(valid, S, b) for b in range(B)]
    keep = torch.zeros(B * S, dtype=torch.bool)
    keep[torch.cat(rows)] = True
    cls[~keep], det[~keep] = 0, 0          # whatever an empty slot holds (NaN in the cases) is not an input
    cls.requires_grad_(True)
    det.requires_grad_(True)
    xr = torch.zeros(B * S, K, dtype=dtype)
    pcs = []
    for b in range(B):
        x_b = torch.softmax(cls[rows[b]] / tc, -1) * torch.softmax(det[rows[b]] / td, 0)
        pcs.append(x_b.sum(0))
        xr[rows[b]] = x_b.detach()
    p = torch.stack(pcs)
    loss = F.binary_cross_entropy(p.clamp(P_LO, P_HI), torch.as_tensor(multihot).to(dtype)) * mult
    (loss * gscale).backward()
    return loss.detach(), xr, cls.grad, det.grad


def mil_class_vector(streams, ccol0, dcol0, K, valid, S, B, tc, td):
    """the unclamped p [B, K] in float64"""
    z = torch.zeros(B, K, dtype=torch.uint8)
    xr = mil(streams, ccol0, dcol0, K, valid, S, B, z, tc, td, 1.0, 1.0)[1]
    return xr.reshape(B, S, K).sum(1)


# ---------------------------------------------------------------------------------------------------- OICR targets
def pairwise_iou(gt, boxes):
    """[G, 4] x [N, 4] float64 -> [G, N], the reference's formula; 0 where the intersection is empty"""
    a1 = (gt[:, 2] - gt[:, 0]) * (gt[:, 3] - gt[:, 1])
    a2 = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    w = np.clip(np.minimum(gt[:, None, 2], boxes[None, :, 2]) - np.maximum(gt[:, None, 0], boxes[None, :, 0]), 0, None)
    h = np.clip(np.minimum(gt[:, None, 3], boxes[None, :, 3]) - np.maximum(gt[:, None, 1], boxes[None, :, 1]), 0, None)
    inter = w * h
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(inter > 0, inter / (a1[:, None] + a2[None, :] - inter), 0.0)


def oicr_targets(src, mode, K, rois5, valid, S, B, multihot, fg=0.5, bg=0.1, col0=0, info=None):
    """get_proposal_clusters + Matcher([fg], [0, 1]) + compute_loss_inputs per image, in float64.
    src: mode 0 -> probabilities at columns [col0, col0 + K); mode 1 -> logits at [col0, col0 + K + 1), softmax taken here.
    Per labelled class, ascending: the live row with the largest probability becomes a pseudo-GT (first index on a tie, np.argmax), then that
    row's probabilities are zeroed. Every live row: the pseudo-GT of largest IoU (first on a tie); label = its class if IoU >= fg else K;
    weight = its score, 0 if IoU < bg. Empty slot -> (-1, 0, zeros); image without a label -> (K, 0, zeros).
    -> labels int64 [B*S], weights float64 [B*S], matched boxes float64 [B*S, 4].
    info (a dict, optional) receives 'gap': the smallest relative lead of a chosen maximum over its runner-up (0 for an exact tie), 'picks':
    per image the chosen rows (within the image), 'iou': per image the fp32-rounded best IoU of every live row"""
    x = torch.as_tensor(src)[:, col0:col0 + (K if mode == 0 else K + 1)].double()
    probs = (x if mode == 0 else torch.softmax(x, -1)).numpy()
    boxes = torch.as_tensor(rois5)[:, 1:5].double().numpy()
    mh = torch.as_tensor(multihot).numpy()
    labels = np.full(B * S, -1, dtype=np.int64)
    weights = np.zeros(B * S)
    matched = np.zeros((B * S, 4))
    fg32, bg32 = np.float32(fg), np.float32(bg)
    gap, picks, ious = np.inf, [], []
    for b in range(B):
        rows = live_rows(valid, S, b).numpy()
        classes = np.nonzero(mh[b])[0]
        picks.append([])
        ious.append(None)
        if len(rows) == 0:
            continue
        if len(classes) == 0:
            labels[rows] = K
            continue
        p = probs[rows].copy()
        gtb, gts = [], []
        for c in classes:
            j = int(np.argmax(p[:, c]))
            if len(rows) > 1:
                top, second = p[j, c], np.max(np.delete(p[:, c], j))
                gap = min(gap, (top - second) / top if top > 0 else 0.0)
            gtb.append(boxes[rows[j]])
            gts.append(p[j, c])
            picks[-1].append(j)
            p[j, :] = 0.0
        q = pairwise_iou(np.stack(gtb), boxes[rows]).astype(np.float32)
        m = np.argmax(q, axis=0)
        best = q[m, np.arange(len(rows))]
        ious[-1] = best
        labels[rows] = np.where(best >= fg32, classes[m], K)
        weights[rows] = np.where(best < bg32, 0.0, np.asarray(gts)[m])
        matched[rows] = np.stack(gtb)[m]
    if info is not None:
        info.update(gap=gap, picks=picks, iou=ious)
    return torch.from_numpy(labels), torch.from_numpy(weights), torch.from_numpy(matched)


# ---------------------------------------------------------------------------------------------------- softmax cross-entropy
def softmax_ce(logits, col0, ncls, labels, weights=None, gscale=1.0, dtype=torch.float64):
    """loss = sum_{label >= 0} w_r * (logsumexp(x_r) - x_r[label]) / #{label >= 0}; dy = gscale * d loss / d x (zero rows where label < 0).
    -inf logits in columns that are no label are probabilities 0. All rows ignored -> loss 0, dy 0. -> (loss [], dy [R, ncls])"""
    x = torch.as_tensor(logits)[:, col0:col0 + ncls].to(dtype)
    lab = torch.as_tensor(labels).long()
    live = lab >= 0
    n = int(live.sum())
    dy = torch.zeros(x.shape, dtype=dtype)
    if n == 0:
        return torch.zeros((), dtype=dtype), dy
    w = torch.ones(x.shape[0], dtype=dtype) if weights is None else torch.as_tensor(weights).to(dtype)
    xl, ll, wl = x[live], lab[live], w[live]
    lse = torch.logsumexp(xl, -1)
    loss = ((lse - xl.gather(1, ll[:, None])[:, 0]) * wl).sum() / n
    g = torch.exp(xl - lse[:, None])
    g[torch.arange(n), ll] -= 1.0
    dy[live] = g * (wl * (gscale / n))[:, None]
    return loss, dy


# ---------------------------------------------------------------------------------------------------- score assembly, loss sum
def sup_scores(delta, dcol0, weak, wcol0, n_oicr, ncls, novel_mask=None, extra=None, ecol0=0):
    """float32, in the kernel's order: delta, + (sum of the n_oicr weak streams in order) / n, + extra, then -inf where novel_mask is set
    (never the last column) -> [R, ncls] fp32"""
    f = torch.float32
    v = torch.as_tensor(delta)[:, dcol0:dcol0 + ncls].to(f).clone()
    if weak is not None:
        s = torch.zeros_like(v)
        for k in range(n_oicr):
            s = s + weak[:, wcol0 + k * ncls: wcol0 + (k + 1) * ncls].to(f)
        v = v + s / torch.tensor(float(n_oicr), dtype=f)
    if extra is not None:
        v = v + extra[:, ecol0:ecol0 + ncls].to(f)
    if novel_mask is not None:
        m = torch.as_tensor(novel_mask).bool().clone()
        cols = torch.zeros(ncls, dtype=torch.bool)
        cols[:min(ncls - 1, m.numel())] = m[:ncls - 1]
        v[:, cols] = float("-inf")
    return v


def sum_losses(losses):
    """the sequential fp32 sum, from 0"""
    s = np.float32(0.0)
    for v in np.asarray(losses, dtype=np.float32):
        s = np.float32(s + v)
    return s
