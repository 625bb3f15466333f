"""numpy restatement of `KMeans(n_clusters=3, random_state=3).fit(p[:, None])` (scikit-learn 1.7.2 defaults) on 1-D float32 data:
the k-means that PCL's get_top_ranking_proposals runs per (image, class) (weak_detector_fast_rcnn.py:465-474). It mirrors
sklearn's precision step by step and is what csrc/pcl.hip implements:

  * fit: tol = mean(var(X)) * 1e-4 in float32 (_tolerance); X -= X.mean() (float32, numpy pairwise sum);
  * _kmeans_plusplus with n_local_trials = 3: the first centre is RandomState(3).choice(n, p=1/n) -- a float64 cumulative sum of
    float32(1/n), normalised by its last element, searched with side='right'; every later centre draws uniform(size=3) * potential,
    searched (side='left') in the float64 cumulative sum of the float32 squared distances. Squared distances go through
    _euclidean_distances_upcast: ((-2 c x) + c^2) + x^2 in float64, rounded to float32, clamped at 0. Potentials are float32
    sums (BLAS there, a float64 sum rounded to float32 here); the best candidate is the first minimum;
  * Lloyd (max_iter 300): d_j = c_j^2 + (-2)(x c_j) in float32, first minimum wins; cluster sums in float32, sequential inside
    256-row chunks, the chunk sums added in chunk order; empty clusters relocated to the farthest point (last index among equals)
    unless every point sits on its centre; centres scaled by float32(1 / weight); stop on identical labels (strict) or on
    sum(shift^2) <= tol, then one more assignment step;
  * the reference keeps the members of the cluster whose centre is the largest (first maximum).

The draws of RandomState(3) do not depend on the data: `draws()` is what the host hands the kernel."""
import numpy as np

CHUNK = 256
F32 = np.float32


def draws(seed=3):
    """[random_sample, uniform x3, uniform x3] of a fresh RandomState(seed): the 7 doubles one fit consumes"""
    rs = np.random.RandomState(seed)
    u0 = rs.random_sample()
    return np.array([u0] + list(rs.uniform(size=3)) + list(rs.uniform(size=3)), dtype=np.float64)


def pairwise_sum(a):
    """numpy's float32 add.reduce of a contiguous run (pairwise, 8 accumulators, blocks of 128)"""
    n = len(a)
    if n < 8:
        r = F32(0.0)
        for v in a:
            r = F32(r + v)
        return r
    if n <= 128:
        r = [F32(v) for v in a[:8]]
        i = 8
        while i < n - (n % 8):
            for j in range(8):
                r[j] = F32(r[j] + a[i + j])
            i += 8
        res = F32(F32(F32(r[0] + r[1]) + F32(r[2] + r[3])) + F32(F32(r[4] + r[5]) + F32(r[6] + r[7])))
        while i < n:
            res = F32(res + a[i])
            i += 1
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return F32(pairwise_sum(a[:n2]) + pairwise_sum(a[n2:]))


def np_sum32(a):
    """np.add.reduce of float32 (X.mean(axis=0), np.var(X, axis=0) of an [n, 1] array)"""
    return pairwise_sum(a)


def sqdist(c, x):
    """_euclidean_distances_upcast of one centre against every point"""
    c64, x64 = float(c), x.astype(np.float64)
    d = ((-2.0 * (c64 * x64)) + c64 * c64) + x64 * x64
    return np.maximum(d.astype(F32), F32(0.0))


def pot32(d):
    return F32(np.sum(d.astype(np.float64)))


def kmeans3(p, u=None):
    """-> (labels int32 [n], centres float32 [3] in data units) as KMeans(3, random_state=3).fit(p[:, None]) returns them"""
    u = draws() if u is None else u
    x0 = np.asarray(p, dtype=F32).reshape(-1)
    n = len(x0)
    mean = F32(np_sum32(x0) / F32(n))
    dv = (x0 - mean).astype(F32)
    tol = F32(F32(np_sum32((dv * dv).astype(F32)) / F32(n)) * F32(1e-4))
    x = (x0 - mean).astype(F32)
    # ---- k-means++
    w = float(F32(1.0) / F32(n))
    cdf = np.cumsum(np.full(n, w))
    cdf /= cdf[-1]
    c0 = int(np.searchsorted(cdf, u[0], side="right"))
    centers = np.zeros(3, F32)
    centers[0] = x[c0]
    closest = sqdist(x[c0], x)
    pot = pot32(closest)
    for c in (1, 2):
        rv = u[1 + 3 * (c - 1):4 + 3 * (c - 1)] * float(pot)
        cum = np.cumsum(closest.astype(np.float64))
        cand = np.minimum(np.searchsorted(cum, rv), n - 1)
        best, bd, bp = 0, None, None
        for t in range(3):
            d = np.minimum(closest, sqdist(x[cand[t]], x))
            pt = pot32(d)
            if bp is None or pt < bp:
                best, bd, bp = t, d, pt
        pot, closest = bp, bd
        centers[c] = x[cand[best]]
    # ---- Lloyd
    labels = np.full(n, -1, np.int32)
    labels_old = labels.copy()

    def assign(cen):
        c2 = (cen * cen).astype(F32)
        d = np.stack([(c2[j] + F32(-2.0) * (x * cen[j]).astype(F32)).astype(F32) for j in range(3)], 1)
        lab = np.zeros(n, np.int32)
        best = d[:, 0].copy()
        for j in (1, 2):
            m = d[:, j] < best
            lab[m], best[m] = j, d[m, j]
        return lab

    strict = False
    for _ in range(300):
        labels = assign(centers)
        csum, wsum = np.zeros(3, F32), np.zeros(3, F32)
        for s in range(0, n, CHUNK):
            lc, xc = labels[s:s + CHUNK], x[s:s + CHUNK]
            for j in range(3):
                v = xc[lc == j]
                if len(v):             # float32 add.accumulate is sequential: the chunk's running sum in row order
                    csum[j] = F32(csum[j] + np.cumsum(v, dtype=F32)[-1])
                    wsum[j] = F32(wsum[j] + F32(len(v)))
        empty = np.where(wsum == 0)[0]
        if len(empty):
            dist = ((x - centers[labels]).astype(F32) ** 2).astype(F32)
            if dist.max() != 0:
                order = sorted(range(n), key=lambda i: (-float(dist[i]), -i))
                for e, far in zip(empty, order):
                    old = labels[far]
                    csum[old] = F32(csum[old] - x[far])
                    csum[e] = x[far]
                    wsum[e] = F32(1.0)
                    wsum[old] = F32(wsum[old] - F32(1.0))
                    labels[far] = e
        new = centers.copy()
        for j in range(3):
            new[j] = csum[j]
            if wsum[j] > 0:
                new[j] = F32(csum[j] * F32(1.0 / float(wsum[j])))
        shift = np.sqrt(((new - centers).astype(F32) ** 2).astype(F32)).astype(F32)
        centers = new
        if np.array_equal(labels, labels_old):
            strict = True
            break
        tot = F32(F32(F32(shift[0] * shift[0]) + F32(shift[1] * shift[1])) + F32(shift[2] * shift[2]))
        if tot <= tol:
            break
        labels_old[:] = labels
    if not strict:
        labels = assign(centers)
    return labels, (centers + mean).astype(F32)


def top_ranking(p, num_clusters=3, u=None):
    """get_top_ranking_proposals (weak_detector_fast_rcnn.py:465-474) -> ascending indices"""
    p = np.asarray(p, dtype=F32).reshape(-1)
    if len(p) < num_clusters:
        return np.array([int(np.argmax(p))])
    lab, cen = kmeans3(p, u)
    idx = np.where(lab == int(np.argmax(cen)))[0]
    return idx if len(idx) else np.array([int(np.argmax(p))])
