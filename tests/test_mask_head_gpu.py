"""The training half of the mask head (csrc/mask.hip), kernel by kernel through the C ABI, against tests/mask_ref.py (fp64, pinned to the
CPU oracle by test_mask_ref_cpu.py), the oracle's BitMasks.crop_and_resize, and torch indexing:

  unit_mask_targets            bit-exact with orc.crop_and_resize_bitmasks, exact 0.5 ties included
  unit_mask_bce_loss           loss, gradient (fp32 / bf16), exact zeros off the gt-class channel, the grid-stride branch (S = 1400)
  unit_mask_bce_loss_ft        delta / sim / sim + delta: loss, both gradient groups, d(loss)/d(sim) added into a prefilled buffer
  unit_deconv2x2_weight_prep / _grad_unpack, and the ConvTranspose2x2 module against F.conv_transpose2d
  unit_gather_match_index, unit_mask_probs (role-0 class, empty slots, per-slot sim)

Tolerances: the loss bar (rtol 1e-5, atol 1e-6) and the fp32 gradient bar (rtol 1e-5, atol 1e-8) are the ones the rpn_loss test of
test_unit_golden_gpu.py uses; every other bound is derived next to its check. Pad columns of the logits are NaN throughout: no kernel
may read them."""
import pytest
import torch
import torch.nn.functional as F

import mask_ref as R
import unit_oracle as orc

pytestmark = pytest.mark.gpu

VOC_BASE = [0, 1, 3, 4, 6, 7, 8, 10, 11, 12, 14, 15, 16, 18, 19]
VOC_NOVEL = [2, 5, 9, 13, 17]
K20 = 20
BASE14 = [c for c in VOC_BASE if c != 19]          # class 19 is then neither base nor novel: role 0
U24 = 2.0 ** -24          # fp32 unit roundoff


def _abi():
    from unit_amd import ops
    from unit_amd._lib import UnitLibError, check, lib
    return ops, check, lib, UnitLibError


def close(a, b, rtol=1e-5, atol=1e-6):
    a, b = torch.as_tensor(a).cpu().double(), torch.as_tensor(b).cpu().double()
    assert a.shape == b.shape, (a.shape, b.shape)
    assert torch.allclose(a, b, rtol=rtol, atol=atol), (a - b).abs().max()


def close_bf16(got, ref):
    """a bf16 gradient: the fp32 value (within the fp32 bar, rtol 1e-5 / atol 1e-8) rounded to nearest bf16, i.e. half a bf16 ulp
    = 2^-9 relative, on top: |got - ref| <= 2^-8 |ref| + 1e-8"""
    got, ref = got.cpu().double(), ref.cpu().double()
    err = (got - ref).abs()
    assert bool((err <= 2.0 ** -8 * ref.abs() + 1e-8).all()), (err - 2.0 ** -8 * ref.abs()).max()


def roles(k, base, novel, dev):
    role = torch.zeros(k, dtype=torch.int8)
    slot = torch.zeros(k, dtype=torch.int32)
    for i, c in enumerate(base):
        role[c], slot[c] = 1, i
    for i, c in enumerate(novel):
        role[c], slot[c] = 2, i
    return dict(base=torch.tensor(base, dtype=torch.int32, device=dev), novel=torch.tensor(novel, dtype=torch.int32, device=dev),
                role=role.to(dev), slot=slot.to(dev), role_cpu=role, slot_cpu=slot)


def packed_nan_pad(cols, kp):
    """device layout of the column groups with NaN in the pad columns"""
    lg = R.pack_logits(cols, kp)
    lg[:, sum(c.shape[1] for c in cols):] = float("nan")
    return lg


# ==================================================================================================== a. unit_mask_targets
@pytest.mark.parametrize("m", [14, 28])
def test_mask_targets_bitmask_exact(dev, m):
    """== orc.crop_and_resize_bitmasks bit for bit on tests/mask_ref.bitmask_fixture (two images x three distinct non-square masks: a
    wrong b * Mcap + gt_index stride or swapped H / W picks another mask; boxes across the border, zero-area, outside, inverted; exact 0.5
    averages, which >= 0.5 rounds to 1). The library is built with -ffp-contract=off for this."""
    ops, check, lib, _ = _abi()
    masks, rois5, gt_index, cls = R.bitmask_fixture()
    b, mcap, h, w = masks.shape
    s = rois5.shape[0]
    md, rd, gd, cd = masks.to(dev), rois5.to(dev), gt_index.to(dev), cls.to(dev)
    out = torch.full((s, m, m), 7, dtype=torch.uint8, device=dev)
    check(lib().unit_mask_targets(ops._p(md), mcap, h, w, ops._p(rd), ops._p(gd), ops._p(cd), R.BITMASK_K, s, m, ops._p(out), ops._s()), "mask_targets")
    got = out.cpu()
    fg = ((cls >= 0) & (cls < R.BITMASK_K)).nonzero().flatten()
    sel = masks.view(-1, h, w)[rois5[fg, 0].long() * mcap + gt_index[fg].long()]
    ref = orc.crop_and_resize_bitmasks(sel, rois5[fg, 1:], m)
    assert int(got.max()) <= 1
    bad = (got[fg] != ref.to(torch.uint8)).flatten(1).sum(1)
    assert not bad.any(), [(int(i), int(n)) for i, n in enumerate(bad) if n]
    # the column of exact 0.5 averages (FIXED_BOXES[0] at M = 14, [1] at M = 28, straight edge at x = 10): >= 0.5 says 1
    tie = got[64 + (m == 28)]
    assert bool(tie[:, :7].all()) and not tie[:, 7:].any()
    assert not got[66:69].any()          # zero-area, outside, inverted
    # cls = -1 and cls = K: zero rows, and their gt_index (+-2^30) was never used to address the masks
    assert int(cls[-2]) == -1 and int(cls[-1]) == R.BITMASK_K and not got[-2:].any()
    # the module-level wrapper is the same call
    from unit_amd.modeling import mask_head
    assert torch.equal(mask_head.mask_targets(md, rd, gd, cd, R.BITMASK_K, m).cpu(), got)


def test_mask_targets_no_slots(dev):
    """S = 0 returns before the launch (a zero-sized grid would be a launch error)"""
    from unit_amd.modeling import mask_head
    masks = torch.zeros(1, 1, 8, 8, dtype=torch.uint8, device=dev)
    out = mask_head.mask_targets(masks, torch.zeros(0, 5, device=dev), torch.zeros(0, dtype=torch.int32, device=dev),
                                 torch.zeros(0, dtype=torch.int32, device=dev), 5, 14)
    assert out.shape == (0, 14, 14)
    torch.cuda.synchronize()


# ==================================================================================================== b. unit_mask_bce_loss
def _loss_fixture(s, k, m, seed):
    """logits N(0, 2) with a few +-40 / +-100 on gt-class channels (the stable BCE form; expf overflow in the sigmoid), about a third of
    the slots background (-1 and K alternating), targets 40 % ones"""
    g = torch.Generator().manual_seed(seed)
    lg = torch.randn(s, k, m, m, generator=g) * 2.0
    cls = torch.randint(0, k, (s,), generator=g)
    bg = (torch.rand(s, generator=g) < 1.0 / 3).nonzero().flatten()
    cls[bg[0::2]] = -1
    cls[bg[1::2]] = k
    cls[0] = 3          # (S = 1 stays a foreground slot)
    tgt = (torch.rand(s, m, m, generator=g) < 0.4).to(torch.uint8)
    fg = ((cls >= 0) & (cls < k)).nonzero().flatten()
    for i, v in enumerate((40.0, -40.0, 100.0, -100.0, 40.0, -40.0, 100.0, -100.0)):
        si = int(fg[(i * 7) % len(fg)])
        lg[si, cls[si], (3 * i) % m, (5 * i + 1) % m] = v          # both targets meet both signs over the eight
        tgt[si, (3 * i) % m, (5 * i + 1) % m] = i // 4
    return lg, cls.int(), tgt


@pytest.mark.parametrize("s", [1, 37, 1400])
def test_mask_bce_loss_vs_fp64(dev, s):
    """S = 1400: S * 196 > 1024 * 256, the grid-stride loop runs a second round and a thread sums more than one term."""
    ops, check, lib, _ = _abi()
    k, ldk, m = 5, 8, 14
    lg, cls, tgt = _loss_fixture(s, k, m, 100 + s)
    if s == 1400:
        assert s * m * m > 1024 * 256
    lgd, cd, td = packed_nan_pad([lg], ldk).to(dev), cls.to(dev), tgt.to(dev)
    fg = (cls >= 0) & (cls < k)
    own = torch.zeros(s, k, m, m, dtype=torch.bool)
    own[fg.nonzero().flatten(), cls[fg].long()] = True
    own = R.pack_logits(own.to(torch.uint8), ldk).bool()          # (fg slot, its class column); pad columns False
    loss = torch.full((1,), 7.0, device=dev)

    def run(gscale, dtype, dl=True):
        d = torch.full((s * m * m, ldk), 3.0, dtype=dtype, device=dev) if dl else None
        check(lib().unit_mask_bce_loss(ops._p(lgd), k, ldk, ops._p(cd), ops._p(td), s, m, gscale, ops._p(loss), ops._p(d), ops.dt(dtype),
                                       ops._s()), "mask_bce_loss")
        return loss.cpu()[0].item(), (d.cpu() if dl else None)

    for gscale in (1.0, 0.37):
        lref, dref, _, _ = R.mask_loss_ref(lg, None, cls, tgt, None, None, None, None, gscale)
        for dtype in (torch.float32, torch.bfloat16):
            lgot, d = run(gscale, dtype)
            close(lgot, lref, rtol=1e-5, atol=1e-6)
            assert not d[~own].any()          # exactly 0: pad columns, other classes' columns, every row of a background slot
            got = R.unpack_logits(d, [k], m)[0]
            if dtype == torch.float32:
                close(got, dref, rtol=1e-5, atol=1e-8)
            else:
                close_bf16(got, dref)
    lnull, _ = run(1.0, torch.float32, dl=False)          # dlogits = NULL: the same loss
    close(lnull, R.mask_loss_ref(lg, None, cls, tgt, None, None, None, None, 1.0)[0], rtol=1e-5, atol=1e-6)
    # all slots background: loss exactly 0, gradient all zero
    cd = torch.where(torch.arange(s) % 2 == 0, -1, k).int().to(dev)
    lgot, d = run(1.0, torch.float32)
    assert lgot == 0.0 and not d.any()


# ==================================================================================================== c. unit_mask_bce_loss_ft
FT_CLS = [0, 2, 19, -1, K20, 5, 7, 13, 3, 9, 17, 19, 2, 18, -1, 13, K20, 1, 5, 19, 16, 9, 4]          # base, novel, role 0, both backgrounds


def _ft_fixture(m, seed):
    g = torch.Generator().manual_seed(seed)
    s, r = len(FT_CLS), 40
    lg = torch.randn(s, K20, m, m, generator=g) * 2.0
    delta = torch.randn(s, K20, m, m, generator=g)
    cls = torch.tensor(FT_CLS, dtype=torch.int32)
    tgt = (torch.rand(s, m, m, generator=g) < 0.4).to(torch.uint8)
    sim = torch.randn(r, len(VOC_NOVEL), len(BASE14), generator=g) * 0.4
    rows = torch.randperm(r, generator=g)[:s].int()          # 23 distinct RoI rows, not the identity; 17 rows stay unaddressed
    assert not torch.equal(rows, torch.arange(s, dtype=torch.int32))
    # small against the sums added into it, so that the rounding of `prefill + sum` (2^-24 of the result) stays inside the 16-ulp
    # allowance of the bound below; large against the bound itself (~1e-6), so an `=` in place of `+=` is a thousandfold miss
    prefill = torch.randn(r, len(VOC_NOVEL), len(BASE14), generator=g) * 1e-3
    return lg, delta, cls, tgt, sim, rows, prefill


@pytest.mark.parametrize("m", [2, 14, 16])          # 16: all 256 threads carry a pixel
@pytest.mark.parametrize("variant", ["delta", "sim", "sim_delta"])
def test_mask_bce_loss_ft_vs_fp64(dev, variant, m):
    ops, check, lib, _ = _abi()
    lg, delta, cls, tgt, sim, rows, prefill = _ft_fixture(m, 7 * m + len(variant))
    use_sim, use_delta = variant != "delta", variant != "sim"
    ldk, gscale = (40 if use_delta else 24), 0.37
    s, mm = len(FT_CLS), m * m
    t = roles(K20, BASE14, VOC_NOVEL, dev)
    role = t["role_cpu"]
    assert role[19] == 0
    cols = [lg, delta] if use_delta else [lg]
    lgd, cd, td = packed_nan_pad(cols, ldk).to(dev), cls.to(dev), tgt.to(dev)
    simd, rowsd = (sim.to(dev), rows.to(dev)) if use_sim else (None, None)
    loss = torch.full((1,), 7.0, device=dev)

    def run(dtype, cls_dev=cd):
        d = torch.full((s * mm, ldk), 3.0, dtype=dtype, device=dev)
        ds = prefill.to(dev) if use_sim else None
        check(lib().unit_mask_bce_loss_ft(ops._p(lgd), K20, ldk, K20 if use_delta else -1, ops._p(cls_dev), ops._p(td), ops._p(simd), ops._p(rowsd),
                                          ops._p(t["base"]) if use_sim else None, len(BASE14) if use_sim else 0, len(VOC_NOVEL) if use_sim else 0,
                                          ops._p(t["role"]) if use_sim else None, ops._p(t["slot"]) if use_sim else None, s, m, gscale,
                                          ops._p(loss), ops._p(d), ops.dt(dtype), ops._p(ds), ops._s()), "mask_bce_loss_ft")
        return loss.cpu()[0].item(), d.cpu(), (ds.cpu() if use_sim else None)

    lref, dlg_ref, dd_ref, ds_ref = R.mask_loss_ref(lg, delta if use_delta else None, cls, tgt, sim if use_sim else None, rows, BASE14, VOC_NOVEL,
                                                    gscale)
    lgot, d, ds = run(torch.float32)
    close(lgot, lref, rtol=1e-5, atol=1e-6)
    got = R.unpack_logits(d, [K20, K20] if use_delta else [K20], m)
    close(got[0], dlg_ref, rtol=1e-5, atol=1e-8)
    if use_delta:
        close(got[1], dd_ref, rtol=1e-5, atol=1e-8)

    # where the gradient may land -- everything else is exactly 0 (the buffer was prefilled with 3.0)
    own0, own1 = torch.zeros(s, K20, m, m, dtype=torch.bool), torch.zeros(s, K20, m, m, dtype=torch.bool)
    for si, c in enumerate(FT_CLS):
        if not 0 <= c < K20:
            continue          # background: no column at all
        own1[si, c] = True          # the delta column of the gt class, whatever its role
        if not use_sim or role[c] == 1:
            own0[si, c] = True          # base class (or no transfer): column c
        elif role[c] == 2:
            own0[si, BASE14] = True          # novel class: every base column carries sim * g, column c nothing
    own = R.pack_logits([own0.to(torch.uint8), own1.to(torch.uint8)] if use_delta else [own0.to(torch.uint8)], ldk).bool()
    assert not d[~own].any()
    if use_sim:
        for si, c in enumerate(FT_CLS):
            if 0 <= c < K20 and role[c] == 2:
                assert not got[0][si, c].any() and bool((got[0][si, BASE14] != 0).any(dim=0).all()), (si, c)
            if c == 19:          # role 0: the delta column only
                assert not got[0][si].any(), si
                if use_delta:
                    assert bool((got[1][si, 19] != 0).all()) and not got[1][si, :19].any()

    if use_sim:
        # d(loss)/d(sim)[rows[s]][j][b] = sum over the M*M pixels of t_i = g_i * row_i[base_b], g_i = gscale * dloss/dlogit_i.
        # The kernel forms t_i in fp32 (one rounding, on a g_i that carries its own few roundings: expf, the division, two scalings)
        # and adds the n = M*M <= 256 terms as a tree (in-wave butterfly, four wave sums), then adds the sum to the prefill (one
        # rounding of a result no larger than ~|sum|, see _ft_fixture). Any order of an n-term fp32 sum has the forward error
        # |err| <= (n - 1) u sum|t_i| + O(u^2), u = 2^-24 (Higham, Accuracy and Stability, 4.2); n = 196 for the production mask side,
        # and 16 u sum|t_i| more covers the roundings inside t_i and the final add: |err| <= (196 + 16) 2^-24 sum|t_i|. (A tree's own
        # bound is its depth, ~9 u, so the same figure also holds at M = 16.) sum|t_i| comes from the fp64 reference: a zero delta makes
        # dloss/ddelta the per-pixel g_i.
        g64 = R.mask_loss_ref(lg, torch.zeros_like(lg), cls, tgt, sim, rows, BASE14, VOC_NOVEL, gscale)[2]
        bound = torch.zeros_like(ds_ref)
        addressed = torch.zeros(sim.shape[:2], dtype=torch.bool)
        for si, c in enumerate(FT_CLS):
            if 0 <= c < K20 and role[c] == 2:
                j = int(t["slot_cpu"][c])
                addressed[rows[si].long(), j] = True
                bound[rows[si].long(), j] = (g64[si, c][None] * lg[si, BASE14].double()).abs().flatten(1).sum(1)
        bound = (196 + 16) * U24 * bound
        err = ((ds.double() - prefill.double()) - ds_ref).abs()
        assert int(addressed.sum()) == sum(1 for c in FT_CLS if c in VOC_NOVEL) and bool((ds_ref[addressed].abs().sum(-1) > 0).all())
        assert bool((err[addressed] <= bound[addressed]).all()), (err[addressed] / bound[addressed]).max()
        # rows nobody addresses -- background, base and role-0 slots, the 17 RoI rows `rows` leaves out -- keep the prefill's bits
        assert torch.equal(ds[~addressed].view(torch.int32), prefill[~addressed].view(torch.int32))
        assert not ds_ref[~addressed].any()

    # the same call again: plain adds in a fixed order -> the same bits (the loss is summed with float atomics: not compared)
    _, d2, ds2 = run(torch.float32)
    assert torch.equal(d2.view(torch.int32), d.view(torch.int32))
    if use_sim:
        assert torch.equal(ds2.view(torch.int32), ds.view(torch.int32))

    # bf16 gradient
    lb, db, _ = run(torch.bfloat16)
    close(lb, lref, rtol=1e-5, atol=1e-6)
    assert not db[~own].any()
    gb = R.unpack_logits(db, [K20, K20] if use_delta else [K20], m)
    close_bf16(gb[0], dlg_ref)
    if use_delta:
        close_bf16(gb[1], dd_ref)

    # all slots background: loss 0, no gradient, dsim untouched
    l0, d0, ds0 = run(torch.float32, torch.where(torch.arange(s) % 2 == 0, -1, K20).int().to(dev))
    assert l0 == 0.0 and not d0.any()
    if use_sim:
        assert torch.equal(ds0.view(torch.int32), prefill.view(torch.int32))


# ==================================================================================================== mask side checks
def _side_args(dev, m_alloc, k, ldk, s=3):
    """buffers sized for the even side m_alloc >= the refused side, so that even a launch that slipped through would stay in bounds"""
    g = torch.Generator().manual_seed(3)
    lg = torch.randn(s * m_alloc * m_alloc, ldk, generator=g).to(dev)
    cls = torch.tensor([1, 0, 2], dtype=torch.int32, device=dev)
    tgt = torch.ones(s, m_alloc, m_alloc, dtype=torch.uint8, device=dev)
    return lg, cls, tgt


def test_mask_kernels_refuse_odd_side(dev):
    """logits are [S][M/2][M/2][4][ldk]: an odd M would index past the last slot's rows. M = 13 is an argument error on all three
    entry points, raised before anything is enqueued -- loss, gradient and output buffers keep their contents."""
    ops, check, lib, UnitLibError = _abi()
    k, ldk, s = 5, 8, 3
    lg, cls, tgt = _side_args(dev, 14, k, ldk)
    loss = torch.full((1,), 7.0, device=dev)
    d = torch.full((s * 196, ldk), 3.0, device=dev)
    with pytest.raises(UnitLibError, match="mask side must be even"):
        check(lib().unit_mask_bce_loss(ops._p(lg), k, ldk, ops._p(cls), ops._p(tgt), s, 13, 1.0, ops._p(loss), ops._p(d), ops.dt(torch.float32),
                                       ops._s()), "mask_bce_loss")
    with pytest.raises(UnitLibError, match="mask side must be even"):
        check(lib().unit_mask_bce_loss_ft(ops._p(lg), k, ldk, -1, ops._p(cls), ops._p(tgt), None, None, None, 0, 0, None, None, s, 13, 1.0,
                                          ops._p(loss), ops._p(d), ops.dt(torch.float32), None, ops._s()), "mask_bce_loss_ft")
    out = torch.full((s, 14, 14), 5.0, device=dev)
    with pytest.raises(UnitLibError, match="mask side must be even"):
        check(lib().unit_mask_probs(ops._p(lg), k, ldk, -1, ops._p(cls), None, None, 0, 0, None, None, s, 13, ops._p(out), ops._s()), "mask_probs")
    with pytest.raises(UnitLibError, match="mask side must be even"):
        check(lib().unit_mask_probs(ops._p(lg), k, ldk, -1, ops._p(cls), None, None, 0, 0, None, None, s, 1, ops._p(out), ops._s()), "mask_probs")
    torch.cuda.synchronize()
    assert loss.item() == 7.0 and bool((d == 3.0).all()) and bool((out == 5.0).all())


def test_mask_bce_loss_ft_refuses_side_above_16(dev):
    ops, check, lib, UnitLibError = _abi()
    k, ldk, s = 5, 8, 3
    lg, cls, tgt = _side_args(dev, 18, k, ldk)
    loss = torch.full((1,), 7.0, device=dev)
    d = torch.full((s * 18 * 18, ldk), 3.0, device=dev)
    with pytest.raises(UnitLibError, match="mask side > 16"):
        check(lib().unit_mask_bce_loss_ft(ops._p(lg), k, ldk, -1, ops._p(cls), ops._p(tgt), None, None, None, 0, 0, None, None, s, 18, 1.0,
                                          ops._p(loss), ops._p(d), ops.dt(torch.float32), None, ops._s()), "mask_bce_loss_ft")
    torch.cuda.synchronize()
    assert bool((d == 3.0).all())


# ==================================================================================================== d. deconv layout kernels
@pytest.mark.parametrize("cin,cout", [(8, 8), (24, 16), (2048, 256)])
def test_deconv_weight_prep_and_grad_unpack_exact(dev, cin, cout):
    """pure permutations (and one cast): w[ic][oc][dy][dx] <-> wf[(q * Cout + oc)][ic], wd[ic][q * Cout + oc], q = dy * 2 + dx"""
    ops, check, lib, _ = _abi()
    g = torch.Generator().manual_seed(cin + cout)
    w = torch.randn(cin, cout, 2, 2, generator=g)
    wd_ = w.to(dev)
    for dtype in (torch.float32, torch.bfloat16):
        wf = torch.full((4 * cout, cin), 9.0, dtype=dtype, device=dev)
        wd = torch.full((cin, 4 * cout), 9.0, dtype=dtype, device=dev)
        check(lib().unit_deconv2x2_weight_prep(ops._p(wd_), cin, cout, ops._p(wf), ops._p(wd), ops.dt(dtype), ops._s()), "deconv2x2_weight_prep")
        wq = w.to(dtype)          # round to nearest even, once
        assert torch.equal(wf.cpu(), wq.permute(2, 3, 1, 0).reshape(4 * cout, cin))
        assert torch.equal(wd.cpu(), wq.permute(0, 2, 3, 1).reshape(cin, 4 * cout))
    dwp = torch.randn(4 * cout, cin, generator=g)
    dbp = torch.randn(4 * cout, generator=g)
    dw_ref = dwp.view(2, 2, cout, cin).permute(3, 2, 0, 1).contiguous()
    db_ref = ((dbp[:cout] + dbp[cout:2 * cout]) + dbp[2 * cout:3 * cout]) + dbp[3 * cout:]          # fp32, left to right: the kernel's sum, exact
    dwp_d, dbp_d = dwp.to(dev), dbp.to(dev)
    for with_db in (True, False):
        dw = torch.full((cin, cout, 2, 2), 9.0, device=dev)
        db = torch.full((cout,), 9.0, device=dev)
        check(lib().unit_deconv2x2_grad_unpack(ops._p(dwp_d), ops._p(dbp_d), cin, cout, ops._p(dw), ops._p(db) if with_db else None, ops._s()),
              "deconv2x2_grad_unpack")
        assert torch.equal(dw.cpu(), dw_ref)
        assert torch.equal(db.cpu(), db_ref if with_db else torch.full((cout,), 9.0))


def test_conv_transpose_2x2_module_vs_torch(dev):
    """ConvTranspose2x2 fwd / dgrad / wgrad (fp32 compute) against fp64 F.conv_transpose2d + ReLU under autograd: ties the tap order
    [y][x][q][oc] to the real operator. Tolerances: test_ops_gpu's fp32 ones (test_conv_fwd 2e-5 / 8e-5; test_conv_dgrad_wgrad 5e-5 /
    2e-4 for dgrad, 1e-4 relative to the largest element for wgrad)."""
    from unit_amd.modeling.mask_head import ConvTranspose2x2
    cin, cout, s, p = 32, 16, 3, 7
    g = torch.Generator().manual_seed(5)
    dc = ConvTranspose2x2(cin, cout)
    with torch.no_grad():
        dc.weight.copy_(torch.randn(cin, cout, 2, 2, generator=g) / cin ** 0.5)
        dc.bias.copy_(torch.randn(cout, generator=g) * 0.5)
    dc = dc.to(dev)
    dc.prepare(torch.float32, 0)
    x = torch.randn(s, p, p, cin, generator=g)
    up = torch.randn(s, cout, 2 * p, 2 * p, generator=g)          # upstream gradient of the ReLU output
    xr = x.permute(0, 3, 1, 2).double().requires_grad_(True)
    wr, br = dc.weight.detach().cpu().double().requires_grad_(True), dc.bias.detach().cpu().double().requires_grad_(True)
    yr = F.relu(F.conv_transpose2d(xr, wr, br, stride=2))
    yr.backward(up.double())
    xd = x.to(dev)
    y = dc.fwd(xd)
    assert y.shape == (s, p, p, 4 * cout)
    got = R.unpack_logits(y.cpu().reshape(s * p * p * 4, cout), [cout], 2 * p)[0]          # rows [s][y][x][q], columns oc
    assert 0.3 < (yr > 0).double().mean().item() < 0.7
    close(got, yr.detach(), rtol=2e-5, atol=8e-5)
    dy1 = R.pack_logits((up * (yr.detach() > 0)).float(), cout).view(s, p, p, 4 * cout).to(dev)          # ReLU-masked, as pred.bwd hands it over
    dx = dc.dgrad(dy1)
    close(dx.cpu()[..., :cin].permute(0, 3, 1, 2), xr.grad, rtol=5e-5, atol=2e-4)
    dc.wgrad(xd, dy1)
    close(dc.weight.grad, wr.grad, rtol=1e-4, atol=1e-4 * wr.grad.abs().max().item())
    close(dc.bias.grad, br.grad, rtol=1e-4, atol=1e-4 * br.grad.abs().max().item())


# ==================================================================================================== e. unit_gather_match_index
def test_gather_match_index_exact(dev):
    """two blocks in x, the second partly filled; -1 entries map to 0; int64 match indices"""
    from unit_amd.modeling import mask_head
    b, s, ncap = 3, 300, 700
    g = torch.Generator().manual_seed(9)
    sidx = torch.randint(0, ncap, (b, s), generator=g, dtype=torch.int32)
    sidx[torch.rand(b, s, generator=g) < 0.1] = -1
    midx = torch.randint(1, 50, (b, ncap), generator=g, dtype=torch.int64)
    assert int((sidx < 0).sum()) > 30
    got = mask_head.gather_match_index(sidx.to(dev), midx.to(dev)).cpu()
    ref = torch.where(sidx >= 0, midx.gather(1, sidx.clamp(min=0).long()), torch.zeros((), dtype=torch.int64)).int()
    assert got.dtype == torch.int32 and torch.equal(got.view(b, s), ref)


# ==================================================================================================== f. unit_mask_probs
@pytest.mark.parametrize("use_delta", [False, True])
def test_mask_probs_roles_and_per_slot_sim(dev, use_delta):
    """role-0 class: sigmoid(0 + delta); cls = -1 / K: zero rows; sim [S, n, b] with a different matrix per slot. Bar: the existing
    mask_probs test's (rtol 1e-5, atol 1e-6): the logit is a 14-term fp32 dot product of O(1) terms (<= 14 u sum|t| ~ 1e-5 at worst
    on sum|t| ~ 10, typically 1e-6), and the sigmoid's slope is at most 1/4."""
    ops, check, lib, _ = _abi()
    m = 14
    cls_list = [2, 0, 19, -1, K20, 5, 19, 13, 7, 9, 17]
    s = len(cls_list)
    g = torch.Generator().manual_seed(21 + use_delta)
    lg = torch.randn(s, K20, m, m, generator=g)
    delta = torch.randn(s, K20, m, m, generator=g) if use_delta else None
    sim = torch.rand(s, len(VOC_NOVEL), len(BASE14), generator=g)
    sim = sim / sim.sum(-1, keepdim=True)
    cls = torch.tensor(cls_list, dtype=torch.int32)
    ldk = 40 if use_delta else 24
    t = roles(K20, BASE14, VOC_NOVEL, dev)
    lgd, cd, simd = packed_nan_pad([lg, delta] if use_delta else [lg], ldk).to(dev), cls.to(dev), sim.to(dev)
    out = torch.full((s, m, m), 5.0, device=dev)
    check(lib().unit_mask_probs(ops._p(lgd), K20, ldk, K20 if use_delta else -1, ops._p(cd), ops._p(simd), ops._p(t["base"]), len(BASE14),
                                len(VOC_NOVEL), ops._p(t["role"]), ops._p(t["slot"]), s, m, ops._p(out), ops._s()), "mask_probs")
    got = out.cpu()
    full = R.transfer_logits(lg.double(), None if delta is None else delta.double(), sim.double(), torch.arange(s), BASE14, VOC_NOVEL)
    ref = torch.zeros(s, m, m, dtype=torch.float64)
    for si, c in enumerate(cls_list):
        if 0 <= c < K20:
            ref[si] = torch.sigmoid(full[si, c])
    close(got, ref, rtol=1e-5, atol=1e-6)
    assert not got[3].any() and not got[4].any()          # cls = -1, cls = K
    for si in (2, 6):          # class 19: sigmoid(0 + delta)
        want = torch.sigmoid(delta[si, 19].double()) if use_delta else torch.full((m, m), 0.5, dtype=torch.float64)
        close(got[si], want, rtol=1e-5, atol=1e-6)
    # distinct rows matter: slot 0 and slot 5 are both novel; with slot 0's matrix slot 5 would read differently
    other = torch.sigmoid(R.transfer_logits(lg.double(), None if delta is None else delta.double(), sim[[0] * s].double(), torch.arange(s), BASE14,
                                            VOC_NOVEL)[5, 5])
    assert (other - ref[5]).abs().max() > 1e-3
