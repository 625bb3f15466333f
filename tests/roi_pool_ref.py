"""RoIPool (torchvision.ops.roi_pool, what Detectron2's ROIPooler builds for POOLER_TYPE "ROIPool") restated on the host, numpy only: the
reference for the kernels of csrc/roi_pool.hip.

The operator, in integer arithmetic on the feature grid:
    x1 = round(roi[1] * scale) ... y2 = round(roi[4] * scale)        halves AWAY from zero (C roundf), written out in round_half_away()
    roi_w = max(x2 - x1 + 1, 1), bin_w = float32(roi_w) / float32(P)  (likewise h)
    bin (ph, pw): rows [floor(ph * bin_h), ceil((ph + 1) * bin_h)) + y1, clamped to [0, H]; columns likewise; empty if hend <= hstart or
    wend <= wstart. The window is scanned row-major with a strict `>` starting from -FLT_MAX: the first maximum wins, a NaN is never selected.
    out = the selected element (its bits: -0 stays -0); an empty bin gives +0 and argmax -1; a window that holds no selectable element (only
    NaN) gives -FLT_MAX and argmax -1. argmax = y * W + x inside the RoI's image.
Backward, in the order the gather kernel adds: for a pixel, the RoIs of its image in ascending row order, inside a RoI the produced bins
row-major; where the stored argmax names the pixel, g[r, oph, opw, c] is added to an fp32 accumulator that starts at +0. Then the epilogue
out = cast((acc [+ addend]) [* (mask_ref > 0)]).

Layouts are the kernels': maps [N, H, W, C], RoIs [R, 5] = (batch index, x1, y1, x2, y2), pooled [R, len(bins), len(bins), C]. `bins`: the
bin indices of the P x P grid that are produced (None = all). Values travel as float32 arrays (every bf16 value is one); `to_dtype` makes the
final conversion the way the kernels do (round to nearest even).
"""
import numpy as np
import torch

F32 = np.float32
SCALE = 1.0 / 16
FLT_MAX = np.finfo(np.float32).max


def round_half_away(v):
    """C roundf on a float32: the nearest integer, halves away from zero (numpy's round / rint go to the even neighbour instead)"""
    v = F32(v)
    a = np.floor(np.abs(v) + F32(0.5))          # |v| + 0.5 is exact for every |v| < 2^22 that has a fractional part
    return int(-a if v < 0 else a)


def window(roi, P, scale=SCALE):
    """-> (b, x1, y1, bin_w, bin_h): integer corner and float32 bin sizes"""
    roi = np.asarray(roi, F32)
    s = F32(scale)
    x1, y1, x2, y2 = (round_half_away(F32(v * s)) for v in roi[1:5])
    rw, rh = max(x2 - x1 + 1, 1), max(y2 - y1 + 1, 1)
    return int(roi[0]), x1, y1, F32(F32(rw) / F32(P)), F32(F32(rh) / F32(P))


def bin_range(p, bsz, start, L):
    """rows (columns) [lo, hi) of bin p, clamped to [0, L]"""
    lo = int(np.floor(F32(F32(p) * bsz))) + start
    hi = int(np.ceil(F32(F32(p + 1) * bsz))) + start
    return min(max(lo, 0), L), min(max(hi, 0), L)


def _live(rois, roi_count):
    return len(rois) if roi_count is None else min(int(roi_count), len(rois))


def forward(feat, rois, P=14, scale=SCALE, bins=None, roi_count=None, image_offset=0):
    """-> (out float32 [R, nb, nb, C], argmax int32 [R, nb, nb, C]). feat[0] is image `image_offset` of the batch the RoIs' indices count in;
    the argmax stays local to the RoI's image. Rows at or past roi_count: zeros, argmax -1."""
    feat = np.asarray(feat, F32)
    _, H, W, C = feat.shape
    sel = list(range(P)) if bins is None else list(bins)
    out = np.zeros((len(rois), len(sel), len(sel), C), F32)
    arg = np.full(out.shape, -1, np.int32)
    ch = np.arange(C)
    for r in range(_live(rois, roi_count)):
        b, x1, y1, bw, bh = window(rois[r], P, scale)
        for i, ph in enumerate(sel):
            hs, he = bin_range(ph, bh, y1, H)
            for j, pw in enumerate(sel):
                ws, we = bin_range(pw, bw, x1, W)
                if he <= hs or we <= ws:
                    continue
                w = feat[b - image_offset, hs:he, ws:we].reshape(-1, C)
                with np.errstate(invalid="ignore"):
                    ok = w > -FLT_MAX                                     # NaN, -inf and -FLT_MAX itself never pass the strict `>`
                k = np.argmax(np.where(ok, w, -np.inf), axis=0)           # the FIRST maximum (-0 == +0: the earlier one)
                has = ok.any(0)
                out[r, i, j] = np.where(has, w[k, ch], -FLT_MAX)
                arg[r, i, j] = np.where(has, (hs + k // (we - ws)) * W + ws + k % (we - ws), -1)
    return out, arg


def forward_loops(feat, rois, P=14, scale=SCALE, bins=None, roi_count=None, image_offset=0):
    """forward() as the kernel's loop, element by element: the brute-force second statement"""
    feat = np.asarray(feat, F32)
    _, H, W, C = feat.shape
    sel = list(range(P)) if bins is None else list(bins)
    out = np.zeros((len(rois), len(sel), len(sel), C), F32)
    arg = np.full(out.shape, -1, np.int32)
    for r in range(_live(rois, roi_count)):
        b, x1, y1, bw, bh = window(rois[r], P, scale)
        for i, ph in enumerate(sel):
            hs, he = bin_range(ph, bh, y1, H)
            for j, pw in enumerate(sel):
                ws, we = bin_range(pw, bw, x1, W)
                if he <= hs or we <= ws:
                    continue
                for c in range(C):
                    best, idx = F32(-FLT_MAX), -1
                    for y in range(hs, he):
                        for x in range(ws, we):
                            v = feat[b - image_offset, y, x, c]
                            if v > best:
                                best, idx = v, y * W + x
                    out[r, i, j, c], arg[r, i, j, c] = best, idx
    return out, arg


def empty_bins(rois, hw, P=14, scale=SCALE, bins=None):
    """-> bool [R, nb, nb]: the bins whose clamped window is empty"""
    H, W = hw
    sel = list(range(P)) if bins is None else list(bins)
    e = np.zeros((len(rois), len(sel), len(sel)), bool)
    for r, roi in enumerate(rois):
        _, x1, y1, bw, bh = window(roi, P, scale)
        for i, ph in enumerate(sel):
            hs, he = bin_range(ph, bh, y1, H)
            for j, pw in enumerate(sel):
                ws, we = bin_range(pw, bw, x1, W)
                e[r, i, j] = he <= hs or we <= ws
    return e


def tied_bins(feat, rois, P=14, scale=SCALE, bins=None):
    """-> bool [R, nb, nb]: the bins in which some channel's maximum occurs more than once in the window"""
    feat = np.asarray(feat, F32)
    _, H, W, C = feat.shape
    sel = list(range(P)) if bins is None else list(bins)
    t = np.zeros((len(rois), len(sel), len(sel)), bool)
    for r, roi in enumerate(rois):
        b, x1, y1, bw, bh = window(roi, P, scale)
        for i, ph in enumerate(sel):
            hs, he = bin_range(ph, bh, y1, H)
            for j, pw in enumerate(sel):
                ws, we = bin_range(pw, bw, x1, W)
                if he <= hs or we <= ws:
                    continue
                w = feat[b, hs:he, ws:we].reshape(-1, C)
                t[r, i, j] = ((w == w.max(0)).sum(0) > 1).any()
    return t


def backward_acc(gout, argmax, shape, rois, roi_count=None, image_offset=0):
    """the fp32 accumulator of the gather kernel: shape = (N, H, W) of the slice of the batch that starts at image `image_offset`;
    gout / argmax [R, nb, nb, C] -> float32 [N, H, W, C]. Additions only, per pixel in (RoI ascending, bin row-major) order."""
    gout = np.asarray(gout, F32)
    N, H, W = shape
    C = gout.shape[-1]
    d = np.zeros((N, H * W, C), F32)
    ch = np.arange(C)
    for r in range(_live(rois, roi_count)):
        n = int(np.asarray(rois[r], F32)[0]) - image_offset
        if not 0 <= n < N:
            continue
        for i in range(gout.shape[1]):
            for j in range(gout.shape[2]):
                a = argmax[r, i, j]
                m = a >= 0
                d[n, a[m], ch[m]] += gout[r, i, j][m]          # one pixel per channel: no index repeats inside the statement
    return d.reshape(N, H, W, C)


def backward_loops(gout, argmax, shape, rois, roi_count=None, image_offset=0):
    """backward_acc() as the kernel walks: pixel by pixel, the RoIs of its image ascending, the bins row-major"""
    gout = np.asarray(gout, F32)
    N, H, W = shape
    C = gout.shape[-1]
    d = np.zeros((N, H, W, C), F32)
    live = _live(rois, roi_count)
    for n in range(N):
        for y in range(H):
            for x in range(W):
                for r in range(live):
                    if int(np.asarray(rois[r], F32)[0]) != n + image_offset:
                        continue
                    for i in range(gout.shape[1]):
                        for j in range(gout.shape[2]):
                            m = argmax[r, i, j] == y * W + x
                            d[n, y, x][m] = d[n, y, x][m] + gout[r, i, j][m]
    return d


def epilogue(acc, addend=None, mask_ref=None):
    """float32 (acc [+ addend]) [* (mask_ref > 0)]"""
    acc = np.asarray(acc, F32)
    if addend is not None:
        acc = (acc + np.asarray(addend, F32)).astype(F32)
    if mask_ref is not None:
        with np.errstate(invalid="ignore"):
            acc = np.where(np.asarray(mask_ref, F32) > 0, acc, F32(0))
    return acc


def to_dtype(a, dtype):
    """float32 array -> torch tensor of `dtype` by the kernels' conversion (bf16: round to nearest even; -FLT_MAX becomes -inf)"""
    return torch.from_numpy(np.ascontiguousarray(a, F32)).to(dtype)


class _RoIPoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat, rois, out_size, spatial_scale):
        f = feat.detach().permute(0, 2, 3, 1).contiguous().numpy()
        out, arg = forward(f, rois.numpy(), out_size, spatial_scale)
        ctx.save_for_backward(rois)
        ctx.arg, ctx.shape = arg, tuple(feat.shape)
        return torch.from_numpy(out).permute(0, 3, 1, 2).contiguous()

    @staticmethod
    def backward(ctx, g):
        (rois,) = ctx.saved_tensors
        n, _, h, w = ctx.shape
        d = backward_acc(g.permute(0, 2, 3, 1).contiguous().numpy(), ctx.arg, (n, h, w), rois.numpy())
        return torch.from_numpy(d).permute(0, 3, 1, 2).contiguous(), None, None, None


def roi_pool(feat, rois, out_size=14, spatial_scale=SCALE, sampling_ratio=0, aligned=True):
    """unit_oracle.roi_align's signature (NCHW fp32 maps -> [R, C, out, out]) over RoIPool: monkeypatch.setattr(unit_oracle, "roi_align",
    roi_pool) turns the oracle's steps into POOLER_TYPE "ROIPool" ones. sampling_ratio / aligned are ignored, as Detectron2 ignores them."""
    del sampling_ratio, aligned
    return _RoIPoolFn.apply(feat, rois, out_size, spatial_scale)
