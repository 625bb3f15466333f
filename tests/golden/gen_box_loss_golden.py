"""Generator of tests/golden/box_loss_golden.npz: the reference's two switchable box-regression losses, smooth-L1 with a beta and GIoU.

What RUNS to produce the recorded fp32 values is the reference's own code, imported by file through d2_stubs.load_reference():
  * FastRCNNOutputsReduction.box_reg_loss (modeling/roi_heads/fast_rcnn.py:37-101), both branches of `box_reg_loss_type`;
  * WSRPN.losses (modeling/proposal_generator/rpn.py:55-101), both branches.
Three names those two functions call live in Detectron2 / fvcore, which this image does not have. They are restated HERE (d2_stubs.py stays as
it is), on the same "unpinned, restated from the published API" footing as d2_stubs.smooth_l1_loss and Box2BoxTransform:
  * `giou_loss`: the published fvcore function (eps 1e-7), bound into the globals of the two loaded reference modules;
  * `FastRCNNOutputs._predict_boxes`: Box2BoxTransform.apply_deltas on the deltas of all K classes;
  * `RPN._decode_proposals`: Box2BoxTransform.apply_deltas per image.

Per case the file holds the inputs, the reference's fp32 losses and autograd's gradient with respect to the predicted deltas, the same formulas
evaluated in float64 on the same (fp32) inputs (`*/f64`), and the fp32 reference's own worst deviation from that evaluation (`dev_*`): the
tests take their tolerance from it. Inputs are seeded so that no min / max of the GIoU has equal operands, no dw / dh sits on the decode's clamp
and no |difference| sits on beta -- asserted below with a margin, so that a last-bit difference in exp / log cannot flip a branch.

Layout of a box-head case `box/<shape>/...`: labels [R] (class, K = background, -1 = empty slot), rois5 [R, 5], gt [R, 4], and per loss kind
`<kind>/deltas` [R, 4] = the four columns of the row's gt class (zero elsewhere; every other column of the [R, 4K] prediction is zero),
`<kind>/grad` [R, 4] likewise (autograd's gradient is zero in every other column: asserted). The reference sees the rows with label >= 0 only:
an empty slot is not a proposal. RPN case `rpn/<kind>/...`: logits [B, N], deltas [B, N, 4], labels [B, N], match [B, N], gt [B, Mcap, 4].

Run:  python tests/golden/gen_box_loss_golden.py [out.npz]
"""
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (HERE, ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)
import d2_stubs as d2  # noqa: E402
import unit_oracle as orc  # noqa: E402

OUT = os.path.join(HERE, "box_loss_golden.npz")
SCALE_CLAMP = math.log(1000.0 / 16)
BOX_WEIGHTS = (10.0, 10.0, 5.0, 5.0)
ZERO_ROWS = (5, 6)          # box-head rows (foreground wherever R > 6) whose centre targets are exactly 0
MARGIN = 1e-3          # px (min / max operands, intersection extents), and relative to beta for |difference| against beta
KINDS = (("giou", "giou", 0.0), ("sl1_b1e-6", "smooth_l1", 1e-6), ("sl1_b0.111", "smooth_l1", 1.0 / 9), ("sl1_b1", "smooth_l1", 1.0))
BOX_SHAPES = (("K20_R1", 20, 1, 0), ("K20_R65", 20, 65, 1), ("K80_R257", 80, 257, 2), ("K20_R700", 20, 700, 3), ("K20_R65_nofg", 20, 65, 4))
RPN_B, RPN_A, RPN_H, RPN_W, RPN_MCAP, RPN_BATCH = 2, 15, 5, 7, 8, 64
RPN_KINDS = (("giou", "giou", 0.0, (1.0, 1.0)), ("giou_w", "giou", 0.0, (0.5, 2.0)), ("sl1_b1e-6", "smooth_l1", 1e-6, (1.0, 1.0)),
             ("sl1_b0.111_w", "smooth_l1", 1.0 / 9, (0.5, 2.0)), ("sl1_b1", "smooth_l1", 1.0, (1.0, 1.0)))


def giou_loss(boxes1, boxes2, reduction="none", eps=1e-7):
    """fvcore.nn.giou_loss as published (Generalized IoU, Rezatofighi et al.): restated, see the module docstring"""
    x1, y1, x2, y2 = boxes1.unbind(dim=-1)
    x1g, y1g, x2g, y2g = boxes2.unbind(dim=-1)
    assert (x2 >= x1).all() and (y2 >= y1).all(), "bad box"
    xkis1, ykis1 = torch.max(x1, x1g), torch.max(y1, y1g)
    xkis2, ykis2 = torch.min(x2, x2g), torch.min(y2, y2g)
    intsctk = torch.zeros_like(x1)
    mask = (ykis2 > ykis1) & (xkis2 > xkis1)
    intsctk[mask] = (xkis2[mask] - xkis1[mask]) * (ykis2[mask] - ykis1[mask])
    unionk = (x2 - x1) * (y2 - y1) + (x2g - x1g) * (y2g - y1g) - intsctk
    iouk = intsctk / (unionk + eps)
    xc1, yc1 = torch.min(x1, x1g), torch.min(y1, y1g)
    xc2, yc2 = torch.max(x2, x2g), torch.max(y2, y2g)
    area_c = (xc2 - xc1) * (yc2 - yc1)
    miouk = iouk - ((area_c - unionk) / (area_c + eps))
    loss = 1 - miouk
    if reduction == "mean":
        loss = loss.mean() if loss.numel() > 0 else 0.0 * loss.sum()
    elif reduction == "sum":
        loss = loss.sum()
    return loss


REF = d2.load_reference()
REF["fast_rcnn"].giou_loss = giou_loss
REF["rpn"].giou_loss = giou_loss


class _Outputs(REF["fast_rcnn"].FastRCNNOutputsReduction):
    def _predict_boxes(self):
        return self.box2box_transform.apply_deltas(self.pred_proposal_deltas, self.proposals.tensor)


class _RPN(REF["rpn"].WSRPN):
    def _decode_proposals(self, anchors, pred_anchor_deltas):
        n = pred_anchor_deltas[0].shape[0]
        return [torch.stack([self.box2box_transform.apply_deltas(d[i], a.tensor) for i in range(n)]) for a, d in zip(anchors, pred_anchor_deltas)]


# ------------------------------------------------------------------------------------------------ the same formulas in any dtype (float64)
def get_deltas(src, tgt, w):
    sw, sh = src[:, 2] - src[:, 0], src[:, 3] - src[:, 1]
    sx, sy = src[:, 0] + 0.5 * sw, src[:, 1] + 0.5 * sh
    tw, th = tgt[:, 2] - tgt[:, 0], tgt[:, 3] - tgt[:, 1]
    tx, ty = tgt[:, 0] + 0.5 * tw, tgt[:, 1] + 0.5 * th
    return torch.stack((w[0] * (tx - sx) / sw, w[1] * (ty - sy) / sh, w[2] * torch.log(tw / sw), w[3] * torch.log(th / sh)), dim=1)


def apply_deltas(d, boxes, w):
    bw, bh = boxes[:, 2] - boxes[:, 0], boxes[:, 3] - boxes[:, 1]
    cx, cy = boxes[:, 0] + 0.5 * bw, boxes[:, 1] + 0.5 * bh
    dw, dh = torch.clamp(d[:, 2] / w[2], max=SCALE_CLAMP), torch.clamp(d[:, 3] / w[3], max=SCALE_CLAMP)
    pcx, pcy = d[:, 0] / w[0] * bw + cx, d[:, 1] / w[1] * bh + cy
    pw, ph = torch.exp(dw) * bw, torch.exp(dh) * bh
    return torch.stack((pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw, pcy + 0.5 * ph), dim=1)


def row_terms(d, src, gt, w, loss_type, beta):
    """the per-row loss of the rows given (all of them count), [n]"""
    if loss_type == "giou":
        return giou_loss(apply_deltas(d, src, w), gt)
    return d2.smooth_l1_loss(d, get_deltas(src, gt, w), beta).sum(dim=1)


def check_margins(d, src, gt, w, loss_type, beta, what):
    """no decision of the loss within MARGIN of flipping (fp32 and float64 alike)"""
    for dt in (torch.float32, torch.float64):
        d_, s_, g_ = d.to(dt), src.to(dt), gt.to(dt)
        if loss_type == "giou":
            p = apply_deltas(d_, s_, w)
            assert float((p - g_).abs().min()) > MARGIN, (what, "min/max operands", float((p - g_).abs().min()))
            iw = torch.min(p[:, 2], g_[:, 2]) - torch.max(p[:, 0], g_[:, 0])
            ih = torch.min(p[:, 3], g_[:, 3]) - torch.max(p[:, 1], g_[:, 1])
            assert float(iw.abs().min()) > MARGIN and float(ih.abs().min()) > MARGIN, (what, "intersection extent")
            for c in (2, 3):
                assert float((d_[:, c] / w[c] - SCALE_CLAMP).abs().min()) > 1e-2, (what, "clamp")
        elif beta >= 1e-5:
            n = (d_ - get_deltas(s_, g_, w)).abs()
            assert float((n - beta).abs().min()) > MARGIN * beta, (what, "beta")


def geometry_kinds(d, src, gt, w):
    """-> per row: 0 disjoint, 1 prediction inside gt, 2 prediction contains gt, 3 partial overlap"""
    p = apply_deltas(d.double(), src.double(), w)
    g = gt.double()
    iw = torch.min(p[:, 2], g[:, 2]) - torch.max(p[:, 0], g[:, 0])
    ih = torch.min(p[:, 3], g[:, 3]) - torch.max(p[:, 1], g[:, 1])
    inside = (p[:, 0] > g[:, 0]) & (p[:, 1] > g[:, 1]) & (p[:, 2] < g[:, 2]) & (p[:, 3] < g[:, 3])
    contains = (p[:, 0] < g[:, 0]) & (p[:, 1] < g[:, 1]) & (p[:, 2] > g[:, 2]) & (p[:, 3] > g[:, 3])
    out = torch.full((len(p),), 3, dtype=torch.int64)
    out[(iw <= 0) | (ih <= 0)] = 0
    out[inside], out[contains] = 1, 2
    return out


# ------------------------------------------------------------------------------------------------ inputs
def wanted_boxes(g, gt, rng):
    """a predicted box per gt box, cycling through: disjoint, inside, containing, partly overlapping"""
    n = len(gt)
    gw, gh = gt[:, 2] - gt[:, 0], gt[:, 3] - gt[:, 1]
    gcx, gcy = gt[:, 0] + 0.5 * gw, gt[:, 1] + 0.5 * gh
    u = torch.rand(n, 6, generator=rng, dtype=torch.float64)
    kind = torch.arange(n) % 4
    sgn = torch.where(u[:, 4] < 0.5, -1.0, 1.0), torch.where(u[:, 5] < 0.5, -1.0, 1.0)
    scale = torch.where(kind == 1, 0.3 + 0.4 * u[:, 0], torch.where(kind == 2, 1.4 + 0.8 * u[:, 0], 0.7 + 0.6 * u[:, 0]))
    scale_h = torch.where(kind == 1, 0.3 + 0.4 * u[:, 1], torch.where(kind == 2, 1.4 + 0.8 * u[:, 1], 0.7 + 0.6 * u[:, 1]))
    shift = torch.where(kind == 0, 2.0 + u[:, 2], torch.where(kind == 3, 0.45 + 0.3 * u[:, 2], 0.1 * (u[:, 2] - 0.5)))
    shift_h = torch.where(kind == 0, 0.3 * u[:, 3], torch.where(kind == 3, 0.45 + 0.3 * u[:, 3], 0.1 * (u[:, 3] - 0.5)))
    pcx, pcy = gcx + sgn[0] * shift * gw, gcy + sgn[1] * shift_h * gh
    pw, ph = scale * gw, scale_h * gh
    return torch.stack((pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw, pcy + 0.5 * ph), dim=1)


def giou_deltas(src, gt, w, rng):
    """fp32 deltas that decode (roughly) to wanted_boxes; row 1 has dw past the clamp, row 2 dh, where there are that many rows"""
    d = get_deltas(src.double(), wanted_boxes(None, gt.double(), rng), w)
    if len(d) > 1:
        d[1, 2] = w[2] * (SCALE_CLAMP + 0.5)
    if len(d) > 2:
        d[2, 3] = w[3] * (SCALE_CLAMP + 1.25)
    return d.float()


def sl1_deltas(src, gt, w, beta, rng, zero_rows):
    """target + differences on both sides of beta, of both signs; exactly 0 in the two centre columns of `zero_rows`: rows whose two boxes
    have integer coordinates and one centre, so that those targets are 0 in every precision (a difference that is 0 in fp32 only would have
    no float64 counterpart: the sign of a rounding error)"""
    t = get_deltas(src, gt, w)          # fp32, as the reference computes it
    for tt in (t, get_deltas(src.double(), gt.double(), w)):
        assert not len(zero_rows) or float(tt[zero_rows, 0:2].abs().max()) == 0
    b = beta if beta >= 1e-5 else 0.2
    n = len(t)
    mag = torch.tensor([0.25, 0.6, 1.7, 4.0])[torch.randint(0, 4, (n, 4), generator=rng)] * b
    sgn = torch.where(torch.rand(n, 4, generator=rng) < 0.5, -1.0, 1.0)
    diff = (mag * sgn).float()
    diff[zero_rows, 0:2] = 0.0
    return t + diff


def seeded(seed, what, src, g, w, loss_type, beta, zero_rows):
    """deltas from the first seed of seed, seed + 100000, ... that keeps every decision clear of its threshold (check_margins)"""
    for attempt in range(200):
        rng = torch.Generator().manual_seed(seed + 100000 * attempt)
        d = giou_deltas(src, g, w, rng) if loss_type == "giou" else sl1_deltas(src, g, w, beta, rng, zero_rows)
        try:
            check_margins(d, src, g, w, loss_type, beta, what)
        except AssertionError:
            continue
        return d
    raise AssertionError(f"{what}: no seed keeps the margins")


def box_shape_inputs(K, R, seed, no_fg):
    rng = torch.Generator().manual_seed(1000 + seed)
    u = torch.rand(R, 8, generator=rng, dtype=torch.float64)
    gw, gh = 20 + 200 * u[:, 0], 20 + 150 * u[:, 1]
    gx, gy = 600 * u[:, 2], 400 * u[:, 3]
    gt = torch.stack((gx, gy, gx + gw, gy + gh), 1)
    if R > 3:
        gt[3] = torch.tensor([300.25, 200.5, 300.95, 201.125])          # a gt box under 1 px
    # proposals around the gt box, as foreground RoIs are
    rw, rh = gw * (0.7 + 0.6 * u[:, 4]), gh * (0.7 + 0.6 * u[:, 5])
    rx, ry = gx + gw * 0.3 * (u[:, 6] - 0.5), gy + gh * 0.3 * (u[:, 7] - 0.5)
    if R > 3:
        rx[3], ry[3], rw[3], rh[3] = 290.0, 190.0, 24.0, 20.0
    rois = torch.stack((rx, ry, rx + rw, ry + rh), 1)
    for r, (g_, s_) in ((5, ((100, 50, 180, 110), (90, 40, 190, 120))), (6, ((301, 77, 341, 99), (311, 70, 331, 106)))):
        if R > r:          # ZERO_ROWS: integer coordinates, one centre
            gt[r], rois[r] = torch.tensor(g_, dtype=torch.float64), torch.tensor(s_, dtype=torch.float64)
    labels = torch.randint(0, K, (R,), generator=rng)
    if R > 4:
        kind = torch.randint(0, 10, (R,), generator=rng)
        labels[kind >= 7] = K          # background
        labels[kind == 6] = -1         # empty slot
        labels[:8] = torch.randint(0, K, (8,), generator=rng)          # the special rows are foreground
    if no_fg:
        labels = torch.where(torch.arange(R) % 3 == 0, -1, K)
    rois5 = torch.cat([torch.zeros(R, 1, dtype=torch.float64), rois], 1)
    return labels.int(), rois5.float(), gt.float()


# ------------------------------------------------------------------------------------------------ box head
def box_reference(labels, rois5, gt, d4, K, loss_type, beta):
    """the reference on the rows with label >= 0 -> (loss, gradient [R, 4] of the gt-class columns)"""
    keep = labels >= 0
    lab = labels[keep].long()
    full = torch.zeros(int(keep.sum()), 4 * K)
    fg = (lab < K).nonzero()[:, 0]
    cols = 4 * lab[fg, None] + torch.arange(4)
    full[fg[:, None], cols] = d4[keep][fg]
    full.requires_grad_(True)
    inst = d2.Instances((480, 640), proposal_boxes=d2.Boxes(rois5[keep, 1:]), gt_boxes=d2.Boxes(gt[keep]), gt_classes=lab)
    o = _Outputs(d2.Box2BoxTransform(BOX_WEIGHTS), torch.zeros(len(lab), K + 1), full, [inst], smooth_l1_beta=beta, box_reg_loss_type=loss_type)
    loss = o.box_reg_loss().sum()
    loss.backward()
    grad = torch.zeros(len(labels), 4)
    gk = torch.zeros(len(lab), 4)
    gk[fg] = full.grad[fg[:, None], cols]
    rest = full.grad.clone()
    rest[fg[:, None], cols] = 0
    assert float(rest.abs().max()) == 0 if rest.numel() else True
    grad[keep] = gk
    return loss.detach(), grad


def box_f64(labels, rois5, gt, d4, K, loss_type, beta):
    lab = labels.long()
    fg = ((lab >= 0) & (lab < K)).nonzero()[:, 0]
    d = d4.double().clone().requires_grad_(True)
    n = int((lab >= 0).sum())
    loss = (row_terms(d[fg], rois5.double()[fg, 1:], gt.double()[fg], BOX_WEIGHTS, loss_type, beta) / max(n, 1)).sum()
    if len(fg):
        loss.backward()
    return loss.detach(), d.grad if d.grad is not None else torch.zeros_like(d)


def box_cases(out):
    for name, K, R, seed in BOX_SHAPES:
        labels, rois5, gt = box_shape_inputs(K, R, seed, name.endswith("nofg"))
        fg = ((labels >= 0) & (labels < K)).nonzero()[:, 0]
        pre = f"box/{name}"
        out[f"{pre}/K"], out[f"{pre}/labels"], out[f"{pre}/rois5"], out[f"{pre}/gt"] = np.int32(K), labels.numpy(), rois5.numpy(), gt.numpy()
        zero = [i for i, r in enumerate(fg.tolist()) if r in ZERO_ROWS]
        assert len(zero) == (2 if len(fg) > 6 else 0)
        for j, (kname, loss_type, beta) in enumerate(KINDS):
            d4 = torch.zeros(R, 4)
            if len(fg):
                src, g = rois5[fg, 1:], gt[fg]
                d4[fg] = seeded(2000 + 10 * seed + j, f"{pre}/{kname}", src, g, BOX_WEIGHTS, loss_type, beta, zero)
                if loss_type == "giou" and len(fg) >= 8:
                    kinds = geometry_kinds(d4[fg], src, g, BOX_WEIGHTS)
                    assert set(kinds.tolist()) == {0, 1, 2, 3}, (pre, kinds.bincount())
            loss, grad = box_reference(labels, rois5, gt, d4, K, loss_type, beta)
            l64, g64 = box_f64(labels, rois5, gt, d4, K, loss_type, beta)
            record(out, f"{pre}/{kname}", dict(deltas=d4), dict(loss=loss), dict(grad=grad), dict(loss=l64), dict(grad=g64), beta)


def record(out, pre, inputs, losses, grads, losses64, grads64, beta):
    out[f"{pre}/beta"] = np.float32(beta)
    for k, v in inputs.items():
        out[f"{pre}/{k}"] = v.numpy()
    for k in losses:
        out[f"{pre}/{k}"], out[f"{pre}/{k}/f64"] = losses[k].float().numpy(), losses64[k].numpy()
        out[f"{pre}/dev_{k}"] = (losses[k].double() - losses64[k]).abs().numpy()          # per loss value
    for k in grads:
        out[f"{pre}/{k}"], out[f"{pre}/{k}/f64"] = grads[k].numpy(), grads64[k].numpy()
        out[f"{pre}/dev_{k}"] = np.float64((grads[k].double() - grads64[k]).abs().max()) if grads[k].numel() else np.float64(0)
    print(pre, {k: v.tolist() for k, v in losses.items()}, {k: out[f"{pre}/dev_{k}"].tolist() for k in list(losses) + list(grads)})


# ------------------------------------------------------------------------------------------------ RPN
def rpn_inputs():
    rng = torch.Generator().manual_seed(77)
    n = RPN_H * RPN_W * RPN_A
    anchors = orc.grid_anchors(RPN_H, RPN_W).float()
    gt = torch.zeros(RPN_B, RPN_MCAP, 4)
    gt[0, :3] = torch.tensor([[10.0, 8.0, 70.0, 60.0], [30.0, 20.0, 100.0, 75.0], [40.25, 30.5, 40.95, 31.125]])          # the last one under 1 px
    gt[1, :2] = torch.tensor([[5.0, 5.0, 40.0, 70.0], [50.0, 10.0, 110.0, 40.0]])
    count = (3, 2)
    labels = torch.zeros(RPN_B, n, dtype=torch.int8)
    match = torch.zeros(RPN_B, n, dtype=torch.int64)
    for b in range(RPN_B):
        kind = torch.randint(0, 10, (n,), generator=rng)
        labels[b][kind >= 6] = -1
        match[b] = torch.randint(0, count[b], (n,), generator=rng)
    pos = torch.randperm(n, generator=rng)[:60]
    pos = torch.cat([pos, torch.tensor([0, 255, 256, 511, 512, n - 1])]).unique()          # every workgroup's first and last anchor
    labels[0][pos] = 1          # image 1 keeps no positive
    match[0][pos[:12]] = 2      # some on the tiny box
    # one positive whose centre targets are exactly 0: an anchor with integer coordinates and a gt box around it with the same centre
    i0 = next(i for i in range(200, n) if bool((anchors[i] == anchors[i].round()).all()) and float(anchors[i, 2] - anchors[i, 0]) <= 64)
    gt[0, 3] = anchors[i0] + torch.tensor([-4.0, -6.0, 4.0, 6.0])
    labels[0][i0], match[0][i0] = 1, 3
    return anchors, gt, labels, match, i0


def rpn_reference(anchors, gt, labels, match, logits, deltas, loss_type, beta, weights):
    lg, dl = logits.clone().requires_grad_(True), deltas.clone().requires_grad_(True)
    rpn = _RPN(in_features=["res4"], head=None, anchor_generator=None, box2box_transform=d2.Box2BoxTransform((1.0, 1.0, 1.0, 1.0)),
               batch_size_per_image=RPN_BATCH, smooth_l1_beta=beta, box_reg_loss_type=loss_type,
               loss_weight={"loss_rpn_cls": weights[0], "loss_rpn_loc": weights[1]})
    losses = rpn.losses([d2.Boxes(anchors)], [lg], [labels[b] for b in range(RPN_B)], [dl], [gt[b][match[b]] for b in range(RPN_B)])
    sum(losses.values()).backward()
    return torch.stack([losses["loss_rpn_cls"], losses["loss_rpn_loc"]]).detach(), lg.grad, dl.grad


def rpn_f64(anchors, gt, labels, match, logits, deltas, loss_type, beta, weights):
    lg, dl = logits.double().requires_grad_(True), deltas.double().requires_grad_(True)
    norm = RPN_BATCH * RPN_B
    valid, pos = labels >= 0, labels == 1
    cls = F.binary_cross_entropy_with_logits(lg[valid], labels[valid].double(), reduction="sum") / norm * weights[0]
    gtm = torch.stack([gt[b][match[b]] for b in range(RPN_B)]).double()
    anc = anchors.double()[None].expand(RPN_B, -1, -1)
    loc = row_terms(dl[pos], anc[pos], gtm[pos], (1.0, 1.0, 1.0, 1.0), loss_type, beta).sum() / norm * weights[1]
    (cls + loc).backward()
    return torch.stack([cls, loc]).detach(), lg.grad, dl.grad


def rpn_cases(out):
    anchors, gt, labels, match, i0 = rpn_inputs()
    n = anchors.shape[0]
    out["rpn/anchors"], out["rpn/gt"], out["rpn/labels"], out["rpn/match"] = anchors.numpy(), gt.numpy(), labels.numpy(), match.numpy()
    out["rpn/A"], out["rpn/batch_size_per_image"] = np.int32(RPN_A), np.int32(RPN_BATCH)
    pos = labels == 1
    assert int(pos[1].sum()) == 0 and int(pos[0].sum()) > 40 and bool(pos[0][512:].any())
    src = anchors[None].expand(RPN_B, -1, -1)[pos]
    g = torch.stack([gt[b][match[b]] for b in range(RPN_B)])[pos]
    w1 = (1.0, 1.0, 1.0, 1.0)
    zero = [int(pos[0][:i0].sum())]          # i0's place among the positives (all of them in image 0)
    for j, (kname, loss_type, beta, weights) in enumerate(RPN_KINDS):
        logits = torch.randn(RPN_B, n, generator=torch.Generator().manual_seed(3000 + j)) * 2
        deltas = torch.zeros(RPN_B, n, 4)
        deltas[pos] = seeded(3100 + j, f"rpn/{kname}", src, g, w1, loss_type, beta, zero)
        if loss_type == "giou":
            assert set(geometry_kinds(deltas[pos], src, g, w1).tolist()) == {0, 1, 2, 3}
        l32, gl32, gd32 = rpn_reference(anchors, gt, labels, match, logits, deltas, loss_type, beta, weights)
        l64, gl64, gd64 = rpn_f64(anchors, gt, labels, match, logits, deltas, loss_type, beta, weights)
        out[f"rpn/{kname}/weights"] = np.asarray(weights, dtype=np.float32)
        record(out, f"rpn/{kname}", dict(logits=logits, deltas=deltas), dict(loss=l32), dict(grad_logits=gl32, grad_deltas=gd32),
               dict(loss=l64), dict(grad_logits=gl64, grad_deltas=gd64), beta)


def main(path=OUT):
    torch.manual_seed(0)
    torch.set_num_threads(1)          # torch's CPU reductions re-associate with the thread count; one thread is one order
    out = {}
    box_cases(out)
    rpn_cases(out)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main(*sys.argv[1:2])
