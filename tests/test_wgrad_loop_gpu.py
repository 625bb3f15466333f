"""The two loop schedules of the 256x256 weight-gradient tile (csrc/conv_wgrad256p8.hip; UNIT_WGRAD_LOOP, unit_wgrad256_loop) write the
same slabs bit for bit: same m permutation inside a fragment, same order of the 64 MFMAs into every accumulator, same split ranges.

Both launch paths go through the C ABI with problems small enough for a test: the per-layer launch (unit_conv2d_wgrad_big_launch: it
picks the split count itself -- one for the small layers, the valid-only form deals its own) and the grouped launch (unit_conv2d_wgrad_group with kind = 2 and the split count
set by the test, so that a split's range is 1, 2, 3, an odd number or a ragged number of 64-pixel steps). Layers: pointwise; 3x3 over the
valid positions only (7x7); 3x3 through the pixel table (38x63: the grouped kernel's 4096-entry table, division in the per-layer kernel's
1024-entry one); 3x3 on a map wider than both tables (70x80: magic division); 3x3 on a 257x256 map (pixels x map size >= 2^32: plain
division); 1x1 stride 2."""
import ctypes
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

# name: (N, H, W, C, K, R, stride, pad)
LAYERS = {
    "pw_64": (1, 8, 8, 512, 256, 1, 1, 0),            # 1 step
    "pw_98": (2, 7, 7, 512, 256, 1, 1, 0),            # 2 steps, M % 64 != 0
    "pw_192": (3, 8, 8, 256, 512, 1, 1, 0),           # 3 steps
    "pw_420": (1, 20, 21, 256, 256, 1, 1, 0),         # 7 steps, the last one ragged
    "valid_7x7": (8, 7, 7, 256, 256, 3, 1, 1),        # valid-only taps: 36 / 42 / 49 positions per image
    "tab_38x63": (1, 38, 63, 256, 256, 3, 1, 1),
    "wide_70x80": (1, 70, 80, 256, 256, 3, 1, 1),
    "div_257x256": (1, 257, 256, 256, 256, 3, 1, 1),
    "s2_14x14": (4, 14, 14, 256, 256, 1, 2, 0),
}


def _lib():
    from unit_amd import _lib as L
    l = L.lib()
    l.unit_conv2d_wgrad_big_launch.restype = ctypes.c_int
    l.unit_conv2d_wgrad_big_launch.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] * 13 + [ctypes.c_size_t, ctypes.c_void_p]
    l.unit_wgrad_big_splits.restype = ctypes.c_int
    l.unit_wgrad_big_splits.argtypes = [ctypes.c_long] + [ctypes.c_int] * 4
    return l


_inputs = {}


def _operands(name, dev):
    """seeded operands of a layer, made once and shared by every test that uses the layer (never written to)"""
    if name not in _inputs:
        from unit_amd import ops as o
        n, h, w, c, k, r, stride, pad = LAYERS[name]
        oh, ow = o.conv_out_size(h, w, r, r, stride, pad)
        gen = torch.Generator().manual_seed(sum(map(ord, name)))
        x = torch.randn(n, h, w, c, generator=gen).bfloat16().to(dev)
        dy = (torch.randn(n, oh, ow, k, generator=gen) * 0.25).bfloat16().to(dev)
        _inputs[name] = (x, dy, oh, ow)
    return _inputs[name]


class _Loop:
    """UNIT_WGRAD_LOOP / UNIT_WGRAD_GANG for the launches inside the block (both are read at every launch)"""

    def __init__(self, loop, gang=None):
        self.want = {"UNIT_WGRAD_LOOP": str(loop), "UNIT_WGRAD_GANG": None if gang is None else str(gang)}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.want}
        for k, v in self.want.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _per_layer(name, dev, loop, variant):
    l = _lib()
    n, h, w, c, k, r, stride, pad = LAYERS[name]
    x, dy, oh, ow = _operands(name, dev)
    splits = l.unit_wgrad_big_splits(n * oh * ow, (r * r * c // 256) * (k // 256), r, r, oh * ow)      # what the launch will choose
    slab = torch.full((splits * k * r * r * c,), float("nan"), dtype=torch.float32, device=dev)
    with _Loop(loop):
        assert l.unit_wgrad256_loop() == loop
        got = l.unit_conv2d_wgrad_big_launch(x.data_ptr(), dy.data_ptr(), slab.data_ptr(), n, h, w, c, k, r, r, stride, pad, oh, ow, k, variant,
                                             slab.numel() * 4, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert got == splits, (got, splits)
    return slab[:got * k * r * r * c].view(got, k, r, r, c), got


def _grouped(names, splits, dev, loop, gang):
    from unit_amd import ops as o
    l = _lib()
    pr = (o.WgradProblem * len(names))()
    slabs = []
    for q, name, sp in zip(pr, names, splits):
        n, h, w, c, k, r, stride, pad = LAYERS[name]
        x, dy, oh, ow = _operands(name, dev)
        slab = torch.full((sp * k * r * r * c,), float("nan"), dtype=torch.float32, device=dev)
        q.x, q.dy, q.partial = x.data_ptr(), dy.data_ptr(), slab.data_ptr()
        q.N, q.H, q.W, q.C, q.K, q.R, q.S, q.stride, q.pad, q.OH, q.OW, q.ldy = n, h, w, c, k, r, r, stride, pad, oh, ow, k
        q.splits, q.kind = sp, 2
        q.x_pitch = q.x_back = q.dy_back = 0
        slabs.append(slab.view(sp, k, r, r, c))
    with _Loop(loop, gang):
        assert l.unit_wgrad256_loop() == loop
        rc = l.unit_conv2d_wgrad_group(pr, len(names), o.dt(torch.bfloat16), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, l.unit_last_error()
    return slabs


def _reference(name, dev):
    """dW and sum |x| |dy| per entry in float64 from the bf16 operands (im2col + matmul on the device), as [K][R][S][C]"""
    n, h, w, c, k, r, stride, pad = LAYERS[name]
    x, dy, _, _ = _operands(name, dev)
    cols = torch.nn.functional.unfold(x.double().permute(0, 3, 1, 2), r, padding=pad, stride=stride)      # [N][C*R*S][OH*OW]
    cols = cols.permute(0, 2, 1).reshape(-1, c * r * r)
    d = dy.double().reshape(-1, k)
    fold = lambda m: m.view(k, c, r, r).permute(0, 2, 3, 1).contiguous()
    return fold(d.t() @ cols), fold(d.abs().t() @ cols.abs())


@pytest.mark.parametrize("variant", [0, 3])
@pytest.mark.parametrize("name", list(LAYERS))
def test_per_layer_launch_both_loops_write_the_same_slabs(dev, name, variant):
    """variant 0 = the policy (valid-only contraction for the 3x3 layer on 7x7), 3 = the tile over all pixels"""
    a, sa = _per_layer(name, dev, 0, variant)
    b, sb = _per_layer(name, dev, 1, variant)
    assert sa == sb
    assert not torch.isnan(a).any() and torch.equal(a, b)


# split counts per layer: pw_420 has 7 steps -> 7 | 4 + 3 | 3 + 3 + 1 | 2 + 2 + 2 + 1; pw_192 -> 3 | 2 + 1 | 1 + 1 + 1; pw_98 -> 2 (ragged) | 1 + 1 (ragged)
GROUPS = [
    (("pw_420", "pw_192", "pw_98", "pw_64"), (1, 1, 1, 1)),
    (("pw_420", "pw_192", "pw_98"), (2, 2, 2)),
    (("pw_420", "pw_192"), (3, 3)),
    (("pw_420",), (4,)),
    (("valid_7x7", "s2_14x14", "pw_98"), (1, 1, 1)),
    (("valid_7x7", "s2_14x14"), (3, 2)),
    (("tab_38x63", "valid_7x7"), (2, 2)),
    (("wide_70x80", "tab_38x63"), (5, 3)),
    (("div_257x256",), (9,)),
]


@pytest.mark.parametrize("gang", [0, 2])
@pytest.mark.parametrize("gi", range(len(GROUPS)))
def test_grouped_launch_both_loops_write_the_same_slabs(dev, gi, gang):
    names, splits = GROUPS[gi]
    a = _grouped(names, splits, dev, 0, gang)
    b = _grouped(names, splits, dev, 1, gang)
    for name, sa, sb in zip(names, a, b):
        assert not torch.isnan(sa).any(), name
        assert torch.equal(sa, sb), name


@pytest.mark.parametrize("name", ["pw_98", "valid_7x7", "s2_14x14", "tab_38x63"])
def test_new_loop_against_float64(dev, name):
    """the slabs of the new loop sum to the weight gradient. A bf16 x bf16 product is exact in fp32, so the only error is that of adding the
    M products of an entry in fp32 in some order: at most M * 2^-24 * sum |x| |dy| (the worst case of any summation order), entry by entry"""
    n, h, w, c, k, r, stride, pad = LAYERS[name]
    ref, mag = _reference(name, dev)
    sp = 1 if name == "pw_98" else 2
    got = _grouped((name,), (sp,), dev, 1, 2)[0].double().sum(0)
    m = _operands(name, dev)[1].numel() // k
    assert bool(((got - ref).abs() <= m * 2.0 ** -24 * mag).all()), ((got - ref).abs().max().item(), mag.max().item())
    assert ref.abs().max().item() > 0
