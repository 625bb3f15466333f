"""fp64 restatement (plain torch on the CPU) of what the mask head's training kernels compute, shared by tests/test_mask_ref_cpu.py --
which pins it to oracle/unit_oracle.py -- and tests/test_mask_head_gpu.py, which holds csrc/mask.hip against it:

  pack_logits / unpack_logits   [S, C, M, M] column groups <-> the device layout [S * M * M, kp] of the logits and their gradient
  transfer_logits, mask_loss_ref MaskRCNNConvUpsampleHeadWith{Similarity,FineTune}.forward's transfer (the reference's
                                modeling/roi_heads/mask_head.py:16-31, :74-91) + Detectron2's mask_rcnn_loss, with autograd gradients
  crop_and_resize_ref64         BitMasks.crop_and_resize's ROIAlign averages BEFORE the >= 0.5 threshold
  bitmask_fixture               the ground-truth masks and boxes both test files use for unit_mask_targets
"""
import math

import torch
import torch.nn.functional as F


# ---------------------------------------------------------------------------------------------------- logit layout
def _pack_one(t):
    s, c, m, _ = t.shape
    p = m // 2
    # [S][C][P][2][P][2] -> [S][P][P][2][2][C]: row ((s*P + Y//2)*P + X//2)*4 + (Y%2)*2 + X%2
    return t.reshape(s, c, p, 2, p, 2).permute(0, 2, 4, 3, 5, 1).reshape(s * m * m, c)


def pack_logits(cols3d, kp):
    """cols3d: one [S, C, M, M] tensor or a sequence of them (column groups, side by side from column 0; M even) -> [S * M * M, kp]
    whose row ((s * P + Y // 2) * P + X // 2) * 4 + (Y % 2) * 2 + X % 2 (P = M / 2) holds pixel (Y, X) of slot s; pad columns are zero."""
    if torch.is_tensor(cols3d):
        cols3d = [cols3d]
    s, _, m, _ = cols3d[0].shape
    assert m % 2 == 0 and all(t.shape[0] == s and t.shape[2] == m and t.shape[3] == m for t in cols3d)
    out = torch.zeros(s * m * m, kp, dtype=cols3d[0].dtype)
    c0 = 0
    for t in cols3d:
        out[:, c0:c0 + t.shape[1]] = _pack_one(t)
        c0 += t.shape[1]
    assert c0 <= kp
    return out


def unpack_logits(packed, widths, m):
    """inverse of pack_logits (for gradients): [S * m * m, kp] -> [one [S, C, m, m] per width C], columns taken from column 0 on"""
    p = m // 2
    s = packed.shape[0] // (m * m)
    out, c0 = [], 0
    for c in widths:
        t = packed[:, c0:c0 + c].reshape(s, p, p, 2, 2, c).permute(0, 5, 1, 3, 2, 4).reshape(s, c, m, m)
        out.append(t.contiguous())
        c0 += c
    return out


# ---------------------------------------------------------------------------------------------------- loss
def transfer_logits(lg, delta, sim, rows, base, novel):
    """orc.mask_head_logits after the convs: base columns copied, novel columns = sim[rows[s]] @ base columns, every other column zero
    (no sim: lg itself); + delta when there is one. fp64 in, fp64 out."""
    s = lg.shape[0]
    out = lg
    if sim is not None and lg.numel() > 0:
        b = torch.as_tensor(base, dtype=torch.int64)
        n = torch.as_tensor(novel, dtype=torch.int64)
        mb = lg.index_select(1, b)
        mn = torch.bmm(sim[torch.as_tensor(rows, dtype=torch.int64)], mb.reshape(s, len(b), -1)).view(s, len(n), *lg.shape[2:])
        out = torch.zeros_like(lg).index_copy(1, n, mn).index_copy(1, b, mb)
    if delta is not None:
        out = out + delta
    return out


def mask_loss_ref(lg, delta, cls, tgt, sim, rows, base, novel, gscale):
    """lg [S, K, M, M] `predictor` output, delta [S, K, M, M] `predictor_delta` output or None, cls [S] (outside [0, K): no instance),
    tgt [S, M, M] 0/1, sim [R, n, b] or None, rows [S] (RoI row of every slot), base / novel class lists.
    -> (loss, gscale * dloss/dlg, gscale * dloss/ddelta or None, gscale * dloss/dsim or None), all fp64."""
    lg = lg.detach().double().requires_grad_(True)
    delta = None if delta is None else delta.detach().double().requires_grad_(True)
    sim = None if sim is None else sim.detach().double().requires_grad_(True)
    k = lg.shape[1]
    out = transfer_logits(lg, delta, sim, rows, base, novel)
    cls = torch.as_tensor(cls, dtype=torch.int64)
    fg = ((cls >= 0) & (cls < k)).nonzero().flatten()
    leaves = [t for t in (lg, delta, sim) if t is not None]
    if fg.numel() == 0:
        loss, grads = torch.zeros((), dtype=torch.float64), [torch.zeros_like(t) for t in leaves]
    else:
        loss = F.binary_cross_entropy_with_logits(out[fg, cls[fg]], tgt[fg].double(), reduction="mean")
        grads = [torch.zeros_like(t) if g is None else g for t, g in zip(leaves, torch.autograd.grad(loss, leaves, allow_unused=True))]
    grads = [gscale * g for g in grads]
    it = iter(grads)
    return loss.detach(), next(it), (next(it) if delta is not None else None), (next(it) if sim is not None else None)


# ---------------------------------------------------------------------------------------------------- bitmask targets
def _axis_weights(start, bin_size, grid, m, size):
    """[m, size] fp64: summed linear-interpolation weights of bin p's `grid` samples along one axis (the 1-D half of the oracle's
    bilinear_setup: samples outside [-1, size] are dropped, the rest clamped to [0, size - 1])"""
    w = torch.zeros(m, size, dtype=torch.float64)
    for p in range(m):
        for i in range(grid):
            v = start + p * bin_size + (i + 0.5) * bin_size / grid
            if v < -1.0 or v > size:
                continue
            v = max(v, 0.0)
            lo = int(v)
            if lo >= size - 1:
                lo = hi = size - 1
                v = float(lo)
            else:
                hi = lo + 1
            l = v - lo
            w[p, lo] += 1.0 - l
            w[p, hi] += l
    return w


def crop_and_resize_ref64(masks, boxes, m):
    """masks [N, H, W] 0/1, boxes float32 [N, 4] -> fp64 [N, m, m]: the averages BitMasks.crop_and_resize thresholds at 0.5, i.e.
    ROIAlign((m, m), spatial_scale 1, sampling_ratio 0, aligned=True) as oracle_roi_align_forward samples it, in fp64. The bilinear
    taps are separable, so the average over the gh x gw grid is Wy @ mask @ Wx^T / max(gh * gw, 1)."""
    n, h, w = masks.shape
    out = torch.zeros(n, m, m, dtype=torch.float64)
    for i in range(n):
        x0, y0, x1, y1 = (float(v) for v in boxes[i])
        sw, sh = x0 - 0.5, y0 - 0.5
        rw, rh = (x1 - 0.5) - sw, (y1 - 0.5) - sh
        gh, gw = int(math.ceil(rh / m)), int(math.ceil(rw / m))
        if gh <= 0 or gw <= 0:
            continue
        wy, wx = _axis_weights(sh, rh / m, gh, m, h), _axis_weights(sw, rw / m, gw, m, w)
        out[i] = wy @ masks[i].double() @ wx.t() / max(gh * gw, 1)
    return out


FIXED_BOXES = [
    [3.5, 2.5, 17.5, 16.5],          # 14 x 14 at M = 14: samples on half pixels -> a column of exact 0.5 on the straight-edge mask
    [3.5, 2.5, 31.5, 30.5],          # 28 x 28: a 2 x 2 sampling grid at M = 14, half-pixel samples at M = 28
    [20.0, 15.0, 20.0, 15.0],        # zero area
    [70.0, 50.0, 90.0, 64.0],        # wholly outside the 40 x 56 image
    [30.0, 10.0, 20.0, 25.0],        # inverted: x1 < x0
]
BITMASK_K = 5
BITMASK_SEED = 5


def bitmask_fixture(seed=BITMASK_SEED):
    """-> gt_masks u8 [2, 3, 40, 56] (five random ellipses; the sixth, image 1 instance 2, is the straight edge mask[:, :10] = 1),
    rois5 float32 [71, 5], gt_index int32 [71], cls int32 [71]: 64 random boxes reaching up to 4 px outside the image, FIXED_BOXES (the
    first two on the straight-edge mask), then one cls = -1 and one cls = K slot whose gt_index must never be read."""
    g = torch.Generator().manual_seed(seed)
    b, mcap, h, w = 2, 3, 40, 56
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing="ij")
    masks = torch.zeros(b * mcap, h, w, dtype=torch.uint8)
    for i in range(5):
        r = torch.rand(4, generator=g, dtype=torch.float64)
        cx, cy, ax, ay = 8 + 40 * r[0], 6 + 28 * r[1], 5 + 18 * r[2], 4 + 12 * r[3]
        masks[i] = (((xx - cx) / ax) ** 2 + ((yy - cy) / ay) ** 2 <= 1.0).to(torch.uint8)
    masks[5, :, :10] = 1
    n = 64
    r = torch.rand(n, 4, generator=g)
    x0, y0 = -4 + r[:, 0] * (w - 4), -4 + r[:, 1] * (h - 4)
    x1, y1 = torch.minimum(x0 + 4 + r[:, 2] * 44, torch.tensor(w + 4.0)), torch.minimum(y0 + 4 + r[:, 3] * 32, torch.tensor(h + 4.0))
    boxes = torch.cat([torch.stack([x0, y0, x1, y1], 1), torch.tensor(FIXED_BOXES)]).float()
    inst = torch.cat([torch.randint(0, b * mcap, (n,), generator=g), torch.tensor([5, 5, 0, 1, 4])])
    cls = torch.cat([torch.randint(0, BITMASK_K, (n + 5,), generator=g), torch.tensor([-1, BITMASK_K])]).int()
    boxes = torch.cat([boxes, torch.tensor([[5.0, 5.0, 25.0, 25.0], [8.0, 4.0, 30.0, 20.0]])])
    image = torch.cat([inst // mcap, torch.tensor([0, 1])])
    gt_index = torch.cat([inst % mcap, torch.tensor([1 << 30, -(1 << 30)])]).int()
    rois5 = torch.cat([image[:, None].float(), boxes], 1).contiguous()
    return masks.view(b, mcap, h, w), rois5, gt_index, cls
