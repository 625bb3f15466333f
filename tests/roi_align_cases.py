"""Seeded inputs for the RoIAlign tests (test_roi_align_ops_cpu.py / _gpu.py): small maps, RoIs that sit on every edge of the sampling rule.

Maps are [N, H, W, C] with N = 3 and (H, W) from MAPS; no RoI of the list names image 2, so a backward must leave (atomic form) or zero
(gather form) a whole image. Values are normal deviates rounded to bf16, so the same map serves the fp32 and the bf16 kernels without a
second rounding. RoIs are (batch index, x1, y1, x2, y2) in image pixels at scale 1/16: the (9, 13) map is an image of 208 x 144 px.

The named RoIs (NAMED, in list order; rois() appends RANDOM seeded boxes) and what each is for, on the (9, 13) map:
  zero_area     x2 == x1, y2 == y1: grid (0, 0) under the adaptive ratio (output 0, count max(0, 1)); a point sample under a fixed ratio
  reversed      x2 < x1, y2 < y1: grid (0, 0) under the adaptive ratio; a real output with negative bin sizes under a fixed one
  top_left      over the top-left corner: samples below -1 (invalid), in (-1, 0) (valid, clamped to 0) and inside
  bottom_right  over the bottom-right corner: samples in (L-1, L) (valid, all weight on L-1) and beyond L (invalid)
  outside       wholly outside the map: a non-empty grid, every sample invalid
  tenth         a tenth of a feature pixel wide: all samples of a bin share one pixel pair
  whole         the whole map
  grid_1x4      adaptive grid (1, 4) at P = 14: more than 2 samples in x only -- the bf16 row kernel's per-sample loop through one axis
  grid_3x1      adaptive grid (3, 1) at P = 14: the same through y
  grid_2x2      adaptive grid exactly (2, 2) at P = 14: the largest the merged-tap branch takes
  int_y, int_x  the integer-sample RoIs: 224 px = 14 x 16 px a side, starting at 16 k + 12, so that at P = 14, sampling_ratio = 2 the start
                is k + 0.25 and the bin size 1.0 exactly, and the samples are k + p + 0.5 and k + p + 1.0 exactly: the 14 integers
                k + 1 .. k + 14. int_y has k = -2 in y: -1, 0, H-1 = 8 and H = 9 (and on the H = 1 maps -1, 0 = H-1, 1 = H). In x the two
                RoIs share the work, because -1 .. W = 13 are 15 integers and a RoI has 14: int_x (k = -2) reaches -1, 0 and W-1 = 12,
                int_y (k = -1 in x) reaches 0, 12 and W = 13. On the W = 1 maps int_x alone reaches -1, 0 and 1.
"""
import functools

import numpy as np
import torch

N_IMAGES = 3
MAPS = [(9, 13), (1, 13), (9, 1), (1, 1)]
C_MAX = 2112
CHANNELS = [8, 72, 520, 1024]          # 1, 9, 65 and 128 lanes of 8 channels: 520 = two waves with one live lane in the second
# (pooled, out, step): the full grids and the strided modes, whose bins are every other one of the pooled grid
MODES = [(14, 14, 1), (14, 7, 2), (7, 7, 1), (7, 4, 2)]
RANDOM = 40
INT_P, INT_SR = 14, 2          # the (pooled, sampling_ratio) the integer-sample RoIs are built for
INT_K = {"int_y": (-2, -1), "int_x": (-2, -2)}          # name -> (k in y, k in x)

NAMED = {
    "zero_area": [0, 100.0, 50.0, 100.0, 50.0],
    "reversed": [1, 180.0, 130.0, 120.0, 60.0],
    "top_left": [0, -40.0, -30.0, 90.0, 60.0],
    "bottom_right": [1, 100.0, 50.0, 260.0, 190.0],
    "outside": [0, -500.0, -400.0, -300.0, -200.0],
    "tenth": [1, 101.3, 67.7, 102.9, 69.3],
    "whole": [0, 0.0, 0.0, 208.0, 144.0],
    "grid_1x4": [1, -300.0, 10.0, 500.0, 150.0],
    "grid_3x1": [0, 20.0, -200.0, 180.0, 400.0],
    "grid_2x2": [1, -60.0, -80.0, 300.0, 250.0],
    "int_y": [0, 16.0 * INT_K["int_y"][1] + 12, 16.0 * INT_K["int_y"][0] + 12, 16.0 * INT_K["int_y"][1] + 12 + 224, 16.0 * INT_K["int_y"][0] + 12 + 224],
    "int_x": [1, 16.0 * INT_K["int_x"][1] + 12, 16.0 * INT_K["int_x"][0] + 12, 16.0 * INT_K["int_x"][1] + 12 + 224, 16.0 * INT_K["int_x"][0] + 12 + 224],
}
NAMES = list(NAMED)

SLOTS, SLOTS_EMPTY = 70, 9          # the fixed-slot set: 70 slots an image (two 64-RoI chunks of the gather kernel), the last 9 empty


def bins(pooled, out, step):
    return list(range(0, pooled, step))[:out]


def index(name):
    return NAMES.index(name)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _random_boxes(gen, k, n_img):
    """k boxes of 1 .. 150 px a side whose corner is up to 60 px off the (9, 13) map's image on any side -> [k, 5]"""
    x1 = torch.rand(k, generator=gen) * 290 - 60
    y1 = torch.rand(k, generator=gen) * 230 - 60
    bw = torch.rand(k, generator=gen) * 149 + 1
    bh = torch.rand(k, generator=gen) * 149 + 1
    bi = torch.randint(0, n_img, (k,), generator=gen).float()
    return torch.stack([bi, x1, y1, x1 + bw, y1 + bh], 1)


@functools.lru_cache(maxsize=None)
def rois():
    """-> [len(NAMED) + RANDOM, 5] fp32; batch indices 0 and 1 only"""
    named = torch.tensor([NAMED[k] for k in NAMES], dtype=torch.float32)
    return torch.cat([named, _random_boxes(_gen(101), RANDOM, 2)], 0).contiguous()


@functools.lru_cache(maxsize=None)
def slot_rois(empty=SLOTS_EMPTY):
    """-> [3 * SLOTS, 5]: image i owns slots [i * SLOTS, (i + 1) * SLOTS); its last `empty` slots are (i, 0, 0, 0, 0), as gather_rois
    leaves the slots of an image that had fewer samples. The first slots of image 0 / 1 are the named RoIs of that image."""
    out = []
    for i in range(N_IMAGES):
        live = _random_boxes(_gen(211 + i), SLOTS - empty, 1)
        named = torch.tensor([v for v in NAMED.values() if v[0] == i], dtype=torch.float32).reshape(-1, 5)
        live[: len(named)] = named
        live[:, 0] = float(i)
        pad = torch.zeros(empty, 5)
        pad[:, 0] = float(i)
        out += [live, pad]
    return torch.cat(out, 0).contiguous()


@functools.lru_cache(maxsize=None)
def _feat_all(hw):
    h, w = hw
    return torch.randn(N_IMAGES, h, w, C_MAX, generator=_gen(31 + MAPS.index(hw))).bfloat16().float()


def feat(hw, c):
    """-> [3, H, W, c] fp32 NHWC with bf16-representable values (the first c channels of one seeded map per shape)"""
    return _feat_all(tuple(hw))[..., :c].contiguous()


@functools.lru_cache(maxsize=None)
def gout(n_rois, out, c):
    """-> [n_rois, out, out, c] fp32, bf16-representable (one seeded draw per shape; treat as read-only)"""
    return torch.randn(n_rois, out, out, c, generator=_gen(57 + out)).bfloat16().float()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def np_rois(t=None):
    return (rois() if t is None else t).numpy().astype(np.float32)
