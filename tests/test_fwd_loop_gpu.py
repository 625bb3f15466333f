"""The two main loops of the 256x256 forward tile (csrc/conv_igemm256p8.hip, template parameter SCHED): the production loop (variant 0 / 8 of
unit_conv2d_fwd_big, tile_cfg 0 / 5 / 16) against the kernel's first loop (variant 13, tile_cfg 23). Both issue the same MFMAs in the same
order on the same operands -- they differ in how a load section issues its LDS-DMA pieces -- so every output is compared BIT FOR BIT: the
map, the ReLU bit words, the pooled partial sums. The shapes are the smallest at which the loop can go wrong: one, two and three k-tiles
(prologue only / prologue + one steady-state iteration), row and channel tails (rows past M and channels past K are staged as zeros through
the out-of-range marker of their offsets), position-class tiles with partly filled classes and skipped taps, the second input starting at
a k-tile boundary, workgroups that walk one and two tiles, two problems in one grid, strided and scattered pointwise convs."""
import pytest
import torch

pytestmark = pytest.mark.gpu

NEW, FIRST = 0, 13          # variants of unit_conv2d_fwd_big / _ex / _pair
TC_NEW, TC_FIRST, TC_ROW_MAJOR = 5, 23, 22          # tile_cfg codes of ops.conv2d (ops.TILE_CFG)


def ops():
    from unit_amd import ops as o
    return o


def rnd(gen, dev, *shape, scale=1.0):
    return (torch.randn(*shape, generator=gen) * scale).to(dev).bfloat16()


def same(a, b):
    o = ops()
    assert len(a) == len(b)
    for u, v in zip(a, b):
        if u is None:
            assert v is None
            continue
        u = u.data if isinstance(u, o.ReluBits) else u
        v = v.data if isinstance(v, o.ReluBits) else v
        assert u.shape == v.shape and torch.equal(u, v)


def test_tile_cfg_23_is_the_first_loop():
    o = ops()
    assert o.TILE_CFG[TC_FIRST][1] == FIRST and o.TILE_CFG[TC_NEW] == ("big", 0) and o.TILE_CFG[TC_ROW_MAJOR] == ("big", 12)


@pytest.mark.parametrize("c", [64, 128, 192])
def test_pointwise_one_two_three_k_tiles(dev, c):
    o = ops()
    gen = torch.Generator().manual_seed(c)
    x, w = rnd(gen, dev, 1, 10, 30, c), rnd(gen, dev, 256, 1, 1, c, scale=c ** -0.5)
    bias = torch.randn(256, generator=gen).to(dev)
    a = o.conv2d(x, w, 256, 1, 1, bias=bias, relu=True, tile_cfg=TC_NEW)
    b = o.conv2d(x, w, 256, 1, 1, bias=bias, relu=True, tile_cfg=TC_FIRST)
    assert torch.equal(a, b)
    assert torch.allclose(a.float(), torch.relu(x.float() @ w.view(256, c).float().t() + bias), rtol=2e-2, atol=2e-2)


@pytest.mark.parametrize("m", [257, 511])
@pytest.mark.parametrize("k", [256, 320, 250])
def test_pointwise_row_and_channel_tails(dev, m, k):
    """rows past M; the second channel tile partly out of range; K = 250: ldy = 252, the stored columns 250 / 251 are sums over zero-staged channels"""
    o = ops()
    gen = torch.Generator().manual_seed(m + k)
    x, w = rnd(gen, dev, 1, 1, m, 128), rnd(gen, dev, k, 1, 1, 128, scale=0.1)
    res = rnd(gen, dev, 1, 1, m, (k + 3) // 4 * 4)
    for kw in ({}, {"residual": res, "relu": True}, {"out_dtype": torch.float32}):
        a = o.conv2d(x, w, k, 1, 1, tile_cfg=TC_NEW, **kw)
        b = o.conv2d(x, w, k, 1, 1, tile_cfg=TC_FIRST, **kw)
        assert torch.equal(a, b)
    y = o.conv2d(x, w, k, 1, 1, tile_cfg=TC_NEW)
    assert torch.allclose(y[..., :k].float().view(m, k), x.view(m, 128).float() @ w.view(k, 128).float().t(), rtol=2e-2, atol=2e-2)
    assert not y[..., k:].any()


@pytest.mark.parametrize("n,h,w_", [(6, 7, 7), (41, 7, 7), (3, 5, 9)])
def test_3x3_position_class_and_row_major_tiles(dev, n, h, w_):
    """3x3 s1 p1 on small maps: position-class tiles with partly filled classes and skipped taps (class runs of 1 and 3 rows on 5x9), and the
    same call on row-major tiles (tile_cfg 22), whose taps are bounds-tested per row"""
    o = ops()
    gen = torch.Generator().manual_seed(n)
    x, w = rnd(gen, dev, n, h, w_, 64), rnd(gen, dev, 256, 3, 3, 64, scale=1 / 24)
    bias = torch.randn(256, generator=gen).to(dev)
    msk = rnd(gen, dev, n, h, w_, 256)
    for kw in ({"bias": bias, "relu": True}, {"mask_ref": msk}):
        first = o.conv2d(x, w, 256, 3, 3, 1, 1, tile_cfg=TC_FIRST, **kw)
        assert torch.equal(o.conv2d(x, w, 256, 3, 3, 1, 1, tile_cfg=TC_NEW, **kw), first)
        assert torch.equal(o.conv2d(x, w, 256, 3, 3, 1, 1, tile_cfg=TC_ROW_MAJOR, **kw), first)
    ref = torch.nn.functional.conv2d(x.float().permute(0, 3, 1, 2), w.float().permute(0, 3, 1, 2), padding=1).permute(0, 2, 3, 1)
    assert torch.allclose(o.conv2d(x, w, 256, 3, 3, 1, 1, tile_cfg=TC_NEW).float(), ref, rtol=2e-2, atol=2e-2)


@pytest.mark.parametrize("blocks", [1, 3])
@pytest.mark.parametrize("k", [256, 2048])
def test_dual_input_split_on_a_k_tile_boundary(dev, blocks, k):
    """[x | x2] . w with the split after one and after three 64-channel blocks; K = 2048: 400 tiles, the persistent form"""
    o = ops()
    gen = torch.Generator().manual_seed(blocks)
    c = 64 * blocks
    x, x2 = rnd(gen, dev, 256, 7, 7, c), rnd(gen, dev, 256, 7, 7, 2 * c)
    w = rnd(gen, dev, k, 1, 1, 3 * c, scale=(3 * c) ** -0.5)
    bias = torch.randn(k, generator=gen).to(dev)
    a = o.conv2d_ex(x, w, k, 1, 1, 0, bias=bias, relu=True, want_bits=True, x2=x2, variant=NEW)
    b = o.conv2d_ex(x, w, k, 1, 1, 0, bias=bias, relu=True, want_bits=True, x2=x2, variant=FIRST)
    same(a, b)
    if k == 256:
        ref = torch.relu(torch.cat([x, x2], 3).view(-1, 3 * c).float() @ w.view(k, 3 * c).float().t() + bias)
        assert torch.allclose(a[0].view(-1, k).float(), ref, rtol=2e-2, atol=2e-2)


@pytest.mark.parametrize("rois", [37, 256])
def test_extended_epilogue(dev, rois):
    """residual + ReLU + bit words, the fused pool without the map, the bit-mask input (unit_conv2d_fwd_big_ex)"""
    o = ops()
    gen = torch.Generator().manual_seed(rois)
    x, w = rnd(gen, dev, rois, 7, 7, 128), rnd(gen, dev, 256, 1, 1, 128, scale=128 ** -0.5)
    res = rnd(gen, dev, rois, 7, 7, 256)
    bias = torch.randn(256, generator=gen).to(dev)
    out = {}
    for v in (NEW, FIRST):
        y, bits, _ = o.conv2d_ex(x, w, 256, 1, 1, 0, bias=bias, residual=res, relu=True, want_bits=True, variant=v)
        pool = o.conv2d_ex(x, w, 256, 1, 1, 0, bias=bias, residual=res, relu=True, want_bits=True, pool_rows=49, want_y=False, variant=v)
        masked = o.conv2d_ex(x, w, 256, 1, 1, 0, residual=res, mask_bits=bits, variant=v)
        out[v] = (y, bits) + tuple(pool) + tuple(masked)
    same(out[NEW], out[FIRST])


def test_persistent_tiles_one_and_two_per_workgroup(dev):
    """300 x 256 rows, one channel tile, one k-tile: more tiles than CUs -- some workgroups walk two tiles, the others one"""
    o = ops()
    gen = torch.Generator().manual_seed(300)
    x, w = rnd(gen, dev, 1, 300, 256, 64), rnd(gen, dev, 256, 1, 1, 64, scale=0.125)
    bias = torch.randn(256, generator=gen).to(dev)
    res = rnd(gen, dev, 1, 300, 256, 256)
    for kw in ({"bias": bias, "relu": True}, {"residual": res}):
        assert torch.equal(o.conv2d(x, w, 256, 1, 1, tile_cfg=TC_NEW, **kw), o.conv2d(x, w, 256, 1, 1, tile_cfg=TC_FIRST, **kw))
    a = o.conv2d_ex(x, w, 256, 1, 1, 0, bias=bias, residual=res, relu=True, want_bits=True, variant=NEW)
    b = o.conv2d_ex(x, w, 256, 1, 1, 0, bias=bias, residual=res, relu=True, want_bits=True, variant=FIRST)
    same(a, b)
    # three k-tiles, rows past M in the last tile of the walk
    x, w = rnd(gen, dev, 1, 299, 255, 192), rnd(gen, dev, 256, 1, 1, 192, scale=0.07)
    assert torch.equal(o.conv2d(x, w, 256, 1, 1, tile_cfg=TC_NEW), o.conv2d(x, w, 256, 1, 1, tile_cfg=TC_FIRST))


@pytest.mark.parametrize("r", [1, 3])
def test_pair_launch(dev, r):
    """two problems of one layer in one grid, different image counts and map sizes"""
    o = ops()
    gen = torch.Generator().manual_seed(r)
    xs = (rnd(gen, dev, 2, 20, 30, 128), rnd(gen, dev, 1, 17, 23, 128))
    w = rnd(gen, dev, 256, r, r, 128, scale=(128 * r * r) ** -0.5)
    bias = torch.randn(256, generator=gen).to(dev)
    a = o.conv2d_pair(xs, w, 256, r, r, 1, r // 2, bias=bias, relu=True, force=(2, NEW))
    b = o.conv2d_pair(xs, w, 256, r, r, 1, r // 2, bias=bias, relu=True, force=(2, FIRST))
    same(a, b)
    same(a, [o.conv2d(x, w, 256, r, r, 1, r // 2, bias=bias, relu=True, tile_cfg=TC_FIRST) for x in xs])


def test_strided_and_scattered_pointwise(dev):
    """the first Res5 block: its stride-2 pointwise conv, and the dgrad of one, which scatters its rows over the twice larger map (oy_mul 2)"""
    o = ops()
    gen = torch.Generator().manual_seed(2)
    x, w = rnd(gen, dev, 9, 14, 14, 128), rnd(gen, dev, 256, 1, 1, 128, scale=128 ** -0.5)
    assert torch.equal(o.conv2d(x, w, 256, 1, 1, 2, 0, relu=True, tile_cfg=TC_NEW), o.conv2d(x, w, 256, 1, 1, 2, 0, relu=True, tile_cfg=TC_FIRST))
    dy, wd = rnd(gen, dev, 9, 7, 7, 128), rnd(gen, dev, 256, 1, 1, 128, scale=128 ** -0.5)
    a = o.conv2d(dy, wd, 256, 1, 1, 1, 0, scatter=(2, 14, 14), tile_cfg=TC_NEW)
    b = o.conv2d(dy, wd, 256, 1, 1, 1, 0, scatter=(2, 14, 14), tile_cfg=TC_FIRST)
    assert torch.equal(a, b) and a.shape == (9, 14, 14, 256) and not a[:, 1::2].any()
