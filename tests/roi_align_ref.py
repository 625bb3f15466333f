"""RoIAlign (Detectron2's ROIAlign) in matrix form, fp64, numpy only: the second source for the kernels of csrc/roi_align.hip
and for the oracle's loop (oracle_c.c), which both walk the samples one by one.

Per RoI the operator is separable. With Wy [P, H] and Wx [P, W], row p = the sum over bin p's samples of the 1-D bilinear weight vector,
    forward   out[r, p, q, :] = sum_y sum_x Wy[p, y] * Wx[q, x] * F[b_r, y, x, :] / count_r           (Wy . F . Wx^T / count)
    backward  dF[b, y, x, :]  = sum_{r: b_r = b} sum_p sum_q Wy[p, y] * Wx[q, x] * g[r, p, q, :] / count_r   (the transpose)
The geometry (start, bin size, grid, count, the sample coordinates) is float32, operation by operation as the kernels and the oracle
evaluate it -- a sample that lands on -1, 0, L-1 or L must land there here as well; from the coordinates on, everything is fp64.
1-D rule: a sample s is invalid if s < -1 or s > L; otherwise s = max(s, 0), lo = int(s), and lo >= L - 1 puts all the weight on L - 1.

Layouts are the kernels': maps [N, H, W, C], RoIs [R, 5] = (batch index, x1, y1, x2, y2), pooled [R, len(bins), len(bins), C].
`bins` is the strided mode: the list of bin indices of the P x P grid that are materialised (None = all P of them).
`forward_abs` / `backward_abs` are the same operators on |F| / |g| (every weight is >= 0): the magnitude the rounding-error bounds of the
tests scale with. `terms_per_pixel` counts the (RoI, bin) pairs with a non-zero weight on a pixel: the length of that pixel's sum.
"""
import numpy as np

F32 = np.float32
SCALE = 1.0 / 16


def _geometry(roi, P, sr, aligned, scale):
    """-> (b, sw, sh, bw, bh, gh, gw, count): roi_geom() of the kernels / oracle_c.c:45-54, float32 operation by operation"""
    roi = np.asarray(roi, F32)
    off, s, p = F32(0.5 if aligned else 0.0), F32(scale), F32(P)
    sw, sh, ew, eh = (F32(F32(v * s) - off) for v in roi[1:5])
    rw, rh = F32(ew - sw), F32(eh - sh)
    if not aligned:
        rw, rh = max(rw, F32(1)), max(rh, F32(1))
    bw, bh = F32(rw / p), F32(rh / p)
    gh = sr if sr > 0 else int(np.ceil(F32(rh / p)))
    gw = sr if sr > 0 else int(np.ceil(F32(rw / p)))
    return int(roi[0]), sw, sh, bw, bh, gh, gw, max(gh * gw, 1)


def grid(roi, P, sr, aligned=True, scale=SCALE):
    """-> (gh, gw), the sampling grid of a bin (<= 0 in an axis: the RoI contributes nothing)"""
    return _geometry(roi, P, sr, aligned, scale)[5:7]


def samples(start, bsz, g, P):
    """-> float32 [P, g]: start + p * bsz + (i + 0.5) * bsz / g, rounded after every operation as the kernels do (empty for g <= 0)"""
    g = max(g, 0)
    p = np.arange(P, dtype=F32)[:, None]
    i = np.arange(g, dtype=F32)[None, :]
    with np.errstate(all="ignore"):
        a = (F32(start) + p * F32(bsz)).astype(F32)
        b = (((i + F32(0.5)).astype(F32) * F32(bsz)).astype(F32) / F32(max(g, 1))).astype(F32)
        return (a + b).astype(F32)


def roi_samples(roi, P, sr, aligned=True, scale=SCALE):
    """-> (ys [P, gh], xs [P, gw]) float32"""
    _, sw, sh, bw, bh, gh, gw, _ = _geometry(roi, P, sr, aligned, scale)
    return samples(sh, bh, gh, P), samples(sw, bw, gw, P)


def weights_1d(s, L):
    """float32 samples [P, g] -> fp64 [P, L]"""
    s = np.asarray(s, F32).astype(np.float64)
    w = np.zeros((s.shape[0], L))
    for p in range(s.shape[0]):
        for v in s[p]:
            if v < -1.0 or v > L:
                continue
            v = max(v, 0.0)
            lo = int(v)
            if lo >= L - 1:
                w[p, L - 1] += 1.0
            else:
                w[p, lo] += 1.0 - (v - lo)
                w[p, lo + 1] += v - lo
    return w


def _matrices(roi, H, W, P, sr, aligned, scale, bins):
    """-> (b, Wy [len(bins), H], Wx [len(bins), W], count)"""
    b, _, _, _, _, gh, gw, count = _geometry(roi, P, sr, aligned, scale)
    ys, xs = roi_samples(roi, P, sr, aligned, scale)
    if gh <= 0 or gw <= 0:
        ys, xs = ys[:, :0], xs[:, :0]
    sel = list(range(P)) if bins is None else list(bins)
    return b, weights_1d(ys, H)[sel], weights_1d(xs, W)[sel], count


def forward(feat, rois, P=14, sr=0, aligned=True, scale=SCALE, bins=None):
    feat = np.asarray(feat, np.float64)
    _, H, W, C = feat.shape
    nb = P if bins is None else len(bins)
    out = np.zeros((len(rois), nb, nb, C))
    for r, roi in enumerate(rois):
        b, wy, wx, count = _matrices(roi, H, W, P, sr, aligned, scale, bins)
        t = np.tensordot(wy, feat[b], axes=(1, 0))                                  # [P, W, C]
        out[r] = np.tensordot(wx, t, axes=(1, 1)).transpose(1, 0, 2) / count          # [Q, P, C] -> [P, Q, C]
    return out


def backward(gout, shape, rois, P=14, sr=0, aligned=True, scale=SCALE, bins=None):
    """shape = (N, H, W); gout [R, len(bins), len(bins), C] -> [N, H, W, C]"""
    gout = np.asarray(gout, np.float64)
    N, H, W = shape
    d = np.zeros((N, H, W, gout.shape[-1]))
    for r, roi in enumerate(rois):
        b, wy, wx, count = _matrices(roi, H, W, P, sr, aligned, scale, bins)
        t = np.tensordot(wy.T, gout[r], axes=(1, 0))                                 # [H, Q, C]
        d[b] += np.tensordot(wx.T, t, axes=(1, 1)).transpose(1, 0, 2) / count         # [W, H, C] -> [H, W, C]
    return d


def forward_abs(feat, rois, P=14, sr=0, aligned=True, scale=SCALE, bins=None):
    return forward(np.abs(np.asarray(feat, np.float64)), rois, P, sr, aligned, scale, bins)


def backward_abs(gout, shape, rois, P=14, sr=0, aligned=True, scale=SCALE, bins=None):
    return backward(np.abs(np.asarray(gout, np.float64)), shape, rois, P, sr, aligned, scale, bins)


def terms_per_pixel(shape, rois, P=14, sr=0, aligned=True, scale=SCALE, bins=None):
    """shape = (N, H, W) -> int64 [N, H, W]: the number of (RoI, bin) pairs whose weight on the pixel is not zero"""
    N, H, W = shape
    n = np.zeros((N, H, W), np.int64)
    for roi in rois:
        b, wy, wx, _ = _matrices(roi, H, W, P, sr, aligned, scale, bins)
        n[b] += np.outer((wy != 0).sum(0), (wx != 0).sum(0))
    return n
