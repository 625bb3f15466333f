"""Seeded inputs for the RoIPool tests (test_roi_pool_cpu.py / test_roi_pool_ops_gpu.py / test_pooler_types_gpu.py).

Maps are [N, H, W, C] with N = 2 and (H, W) from MAPS, small on purpose: a bin window is a handful of pixels and every rule of the operator
has a RoI that sits on it. RoIs are (batch index, x1, y1, x2, y2) in image pixels at scale 1/16: the (5, 7) map is an image of 112 x 80 px.

The named RoIs (named_rois(hw), then RANDOM seeded boxes) and what each is for:
  whole         the whole map
  one_pixel     one feature pixel (PIXEL): every bin's window is that pixel -- the backward sums all of gout there, in order
  narrow_x      2 pixels wide, taller than the map: narrower than the 6 and 7 grids in x only (bin_w < 1: a pixel sits in several bins of a row)
  halves        scaled corners exactly on -0.5, 1.5, 3.5 and 2.5: roundf gives -1, 2, 4, 3 where round-half-even gives 0, 2, 4, 2
  reversed      x2 < x1 and y2 < y1: roi_w = roi_h = 1
  partly        over the top-left corner: the bins left of / above the map are empty
  outside       wholly outside the map: every bin empty
Maps (feat(kind, hw, c), values exactly representable in bf16 so that one map serves both kernels without a second rounding):
  random        every channel holds a permutation of distinct values: no window has a tied maximum
  ties          integers 0 .. 2: most windows have one
  zeros         only -0.0 and +0.0: every window is a tie between them, the output bit pattern tells which element was taken
  nan           `random` with NaN at PIXEL of every image: one_pixel's windows hold nothing but NaN, the neighbours' skip it
"""
import functools

import numpy as np
import torch

N_IMAGES = 2
MAPS = [(5, 7), (1, 9)]
C_MAX = 1024
CHANNELS = [8, 64, 72, 1024]          # 1, 8, 9 and 128 lanes of 8 channels
MODES = [(14, 14, 1), (14, 7, 2), (7, 7, 1), (6, 6, 1)]          # (pooled, out, step)
KINDS = ["random", "ties", "zeros", "nan"]
RANDOM = 12
SLOTS, SLOTS_EMPTY = 9, 2          # the fixed-slot set: 9 slots an image, the last 2 unused


def pixel(hw):
    """(y, x) of the one_pixel RoI"""
    return min(2, hw[0] - 1), 3


def named_rois(hw):
    y, x = pixel(hw)
    return {
        "whole": [0, 0.0, 0.0, 16.0 * (hw[1] - 1), 16.0 * (hw[0] - 1)],
        "one_pixel": [1, 16.0 * x, 16.0 * y, 16.0 * x, 16.0 * y],
        "narrow_x": [0, 32.0, -32.0, 48.0, 80.0],
        "halves": [1, -8.0, 24.0, 56.0, 40.0],
        "reversed": [0, 80.0, 48.0, 32.0, 16.0],
        "partly": [1, -48.0, -32.0, 40.0, 30.0],
        "outside": [0, 400.0, 300.0, 500.0, 380.0],
    }


NAMES = list(named_rois(MAPS[0]))


def index(name):
    return NAMES.index(name)


def bins(pooled, out, step):
    return list(range(0, pooled, step))[:out]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _random_boxes(gen, k, n_img):
    """k boxes of 1 .. 250 px a side whose top-left corner lies within (-150, 50) px: most of them overhang the map, so that even bins of
    the 14 grid span several feature pixels (a one-pixel window cannot hold a tie) -> [k, 5]"""
    x1 = torch.rand(k, generator=gen) * 200 - 150
    y1 = torch.rand(k, generator=gen) * 200 - 150
    bw = torch.rand(k, generator=gen) * 249 + 1
    bh = torch.rand(k, generator=gen) * 249 + 1
    bi = torch.randint(0, n_img, (k,), generator=gen).float()
    return torch.stack([bi, x1, y1, x1 + bw, y1 + bh], 1)


@functools.lru_cache(maxsize=None)
def rois(hw):
    """-> [len(NAMES) + RANDOM, 5] fp32, batch indices 0 and 1"""
    named = torch.tensor(list(named_rois(hw).values()), dtype=torch.float32)
    return torch.cat([named, _random_boxes(_gen(101), RANDOM, N_IMAGES)], 0).contiguous()


@functools.lru_cache(maxsize=None)
def rois_one_image(hw, image):
    """rois(hw) with every batch index = image: the other image of the map is named by no RoI"""
    r = rois(hw).clone()
    r[:, 0] = float(image)
    return r.contiguous()


@functools.lru_cache(maxsize=None)
def slot_rois(hw):
    """-> [N_IMAGES * SLOTS, 5]: image i owns slots [i * SLOTS, (i + 1) * SLOTS), its last SLOTS_EMPTY are (i, 0, 0, 0, 0) as gather_rois leaves
    the slots of an image with fewer samples; the live ones are the named RoIs, re-indexed to the image"""
    out = []
    named = torch.tensor(list(named_rois(hw).values()), dtype=torch.float32)
    for i in range(N_IMAGES):
        live = named.clone()[: SLOTS - SLOTS_EMPTY]
        live[:, 0] = float(i)
        pad = torch.zeros(SLOTS_EMPTY, 5)
        pad[:, 0] = float(i)
        out += [live, pad]
    return torch.cat(out, 0).contiguous()


@functools.lru_cache(maxsize=None)
def _feat_all(kind, hw):
    h, w = hw
    n = N_IMAGES * h * w
    g = _gen(31 + 7 * KINDS.index(kind) + MAPS.index(hw))
    if kind in ("random", "nan"):
        # per channel a permutation of the n distinct values (k - n // 2) / 4: among them exactly one zero, no pair equal
        perm = torch.argsort(torch.rand(n, C_MAX, generator=g), dim=0).float()
        f = ((perm - n // 2) / 4).reshape(N_IMAGES, h, w, C_MAX)
        if kind == "nan":
            y, x = pixel(hw)
            f[:, y, x, :] = float("nan")
        return f.contiguous()
    if kind == "ties":
        return torch.randint(0, 3, (N_IMAGES, h, w, C_MAX), generator=g).float()
    if kind == "zeros":
        z = torch.zeros(N_IMAGES, h, w, C_MAX)
        return torch.where(torch.rand(z.shape, generator=g) < 0.5, -z, z).contiguous()
    raise KeyError(kind)


def feat(kind, hw, c=C_MAX):
    """-> [2, H, W, c] fp32 NHWC, bf16-representable (the first c channels of one seeded map per kind and shape; read-only)"""
    return _feat_all(kind, tuple(hw))[..., :c].contiguous()


@functools.lru_cache(maxsize=None)
def gout(n_rois, out):
    """-> [n_rois, out, out, C_MAX] fp32, bf16-representable (one seeded draw per shape; read-only)"""
    return torch.randn(n_rois, out, out, C_MAX, generator=_gen(57 + out)).bfloat16().float()


@functools.lru_cache(maxsize=None)
def addend(hw, n_images=N_IMAGES):
    return torch.randn(n_images, hw[0], hw[1], C_MAX, generator=_gen(77)).bfloat16().float()


@functools.lru_cache(maxsize=None)
def mask_ref(hw, n_images=N_IMAGES):
    """the map whose sign gates the gradient (the res4 output under its ReLU): about half of it is zero"""
    return torch.relu(torch.randn(n_images, hw[0], hw[1], C_MAX, generator=_gen(79))).bfloat16().float()


def np_rois(t):
    return t.numpy().astype(np.float32)


# ---- the step tests' proposals (test_pooler_types_gpu.py): boxes on the 4-px lattice. Scaled by 1/16 their corners end in .0, .25, .5 or
# .75 exactly, so the device and the reference round the same bits: a max pooler is discontinuous in the box, and a last-bit difference
# between two decodings of an RPN output may move a window by a pixel without either side being wrong.
LATTICE = 4


def lattice_proposals(n_images, k, hw_image, seed):
    """-> list of n_images (boxes [k, 4] fp32, logits [k] descending): x1 < x2 <= W, y1 < y2 <= H, every coordinate a multiple of LATTICE px"""
    h, w = hw_image
    g = _gen(seed)
    out = []
    for _ in range(n_images):
        x1 = torch.randint(0, w // LATTICE - 1, (k,), generator=g)
        y1 = torch.randint(0, h // LATTICE - 1, (k,), generator=g)
        x2 = x1 + 1 + (torch.rand(k, generator=g) * (w // LATTICE - x1 - 1)).long().clamp(max=w // LATTICE - x1 - 1)
        y2 = y1 + 1 + (torch.rand(k, generator=g) * (h // LATTICE - y1 - 1)).long().clamp(max=h // LATTICE - y1 - 1)
        boxes = (torch.stack([x1, y1, x2, y2], 1) * LATTICE).float()
        logits = torch.sort(torch.randn(k, generator=g), descending=True).values
        out.append((boxes, logits))
    return out
