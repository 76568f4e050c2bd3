"""Deterministic-mode kernels on the GPU (include/maestro_hip.h): the ordered reduction bit for bit against the numpy
emulation of tests/test_det_host.py, and every atomic-free producer followed by its ordered reduce -- against fp64 under the
fp32-accumulation bound of tests/numerics.py (``gemm_bound``: n addends in any order, 2^-23 per term on the sum of magnitudes),
and bit-equal over three launches.  Operands sit between the poisoned guard bands of tests/guards.py.

The bounds: a sum of n fp32 addends is ``gemm_bound(sum |addend|, n)`` with n the number of addends, unmodified -- also where an
addend is itself the result of a few fp32 operations (a squared difference, dy * z, the weight / count factor of the loss): the
constant of ``gemm_bound`` is 2 u per term where an ordered sum needs u, and the measured worst ratios (printed by every test,
recorded in profiles/determinism.md) stay below 2e-2.
"""

from __future__ import annotations

import numpy as np
import pytest
import torch

from tests import guards, numerics
from tests.test_det_host import order_sensitive, ordered_reduce_emulated

pytestmark = pytest.mark.gpu
F32, BF16 = torch.float32, torch.bfloat16


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _inp(gs, data, ld=None, name="input"):
    """Input between guard bands; returns (view, flat span over rows * ld elements)."""
    view, g = guards.guarded(data.shape, data.dtype, gs.device, ld=ld, data=data, name=name)
    gs.guards.append(g)
    return view, g.span()


def _out(gs, shape, dtype=F32, ld=None, init=None, name="output"):
    view, g = guards.guarded(shape, dtype, gs.device, ld=ld, init=init, name=name)
    gs.guards.append(g)
    return view, g.span()


def _within(got, want64, bound, what):
    err = (got.double().cpu() - want64.cpu()).abs()
    ratio = numerics.worst_ratio(err, bound.cpu())
    print(f"{what}: worst error / bound = {ratio:.3e}")
    assert ratio <= 1.0, f"{what}: error exceeds the fp32-accumulation bound, ratio {ratio}"


def _three_launches(run, outputs):
    """``run()`` three times; the raw bits of every output are the same each time."""
    first = None
    for _ in range(3):
        run()
        torch.cuda.synchronize()
        now = [o.clone() for o in outputs]
        if first is None:
            first = now
        for a, b in zip(first, now):
            assert guards.bits_equal(a, b), "bits differ between launches"


def test_ordered_reduce_descriptor_rejects_malformed_jobs(dev):
    from maestro_amd import hip
    src, dst = torch.zeros(8, 8, device=dev), torch.zeros(8, device=dev)
    with pytest.raises(hip.HipExtensionError, match="does not fit"):
        hip.OrderedReduce([(src, dst, 8, 8, 4)], dev)                     # cols > ld
    with pytest.raises(hip.HipExtensionError, match="does not fit"):
        hip.OrderedReduce([(src, dst, 9, 8, 8)], dev)                     # more rows than the buffer holds
    with pytest.raises(hip.HipExtensionError, match="differ"):
        hip.OrderedReduce([(src, dst, 8, 8, 8), (src, dst, 8, 4, 8)], dev)
    with pytest.raises(hip.HipExtensionError, match="differ"):
        hip.OrderedReduce([(src, dst, 8, 8, 8, False), (src, dst, 8, 8, 8, True)], dev)
    with pytest.raises(hip.HipExtensionError, match="overlap"):
        hip.OrderedReduce([(src, dst, 8, 8, 8), (src, dst[4:], 8, 4, 8)], dev)
    with pytest.raises(hip.HipExtensionError, match="f32"):
        hip.OrderedReduce([(src.to(BF16), dst, 8, 8, 8)], dev)


# ------------------------------------------------------------------------------------------------ guard bands (tests/guards.py)
# The ledger of tests/guards.py counts the calls below this banner: every test from here on keeps its operands in a GuardSet.
# ------------------------------------------------------------------------------------------------ mh_reduce_ordered
@pytest.mark.parametrize("rows,cols,ld", [(1, 4, 4), (16, 256, 256), (17, 260, 264), (33, 4, 12), (100, 516, 520)])
def test_reduce_ordered_matches_the_emulation(dev, rows, cols, ld):
    from maestro_amd import hip
    gs = guards.GuardSet(dev)
    src = order_sensitive(rows, cols, seed=rows * 1000 + cols)
    _, span = _inp(gs, torch.from_numpy(src), ld=ld, name="src")
    dst, dspan = _out(gs, (1, cols), name="dst")
    table = hip.OrderedReduce([(span, dspan, rows, cols, ld)], dev)
    table.launch()
    gs.check()
    want = ordered_reduce_emulated([src])
    assert np.array_equal(dst[0].cpu().numpy().view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("add", [False, True])
def test_reduce_ordered_three_job_chain(dev, add):
    from maestro_amd import hip
    gs = guards.GuardSet(dev)
    shapes = [(17, 260, 264), (33, 260, 260), (5, 260, 300)]
    srcs = [order_sensitive(r, c, seed=70 + i) for i, (r, c, _) in enumerate(shapes)]
    spans = [_inp(gs, torch.from_numpy(s), ld=ld, name=f"src{i}")[1] for i, (s, (_, _, ld)) in enumerate(zip(srcs, shapes))]
    old = order_sensitive(1, 260, seed=79)
    dst, dspan = _out(gs, (1, 260), name="dst")
    dst.copy_(torch.from_numpy(old))
    for g in gs.guards:
        g.arm()
    hip.OrderedReduce([(sp, dspan, r, c, ld, add) for sp, (r, c, ld) in zip(spans, shapes)], dev).launch()
    gs.guards[-1].whole = False
    gs.check()
    want = ordered_reduce_emulated(srcs, dst_old=old[0] if add else None)
    assert np.array_equal(dst[0].cpu().numpy().view(np.uint32), want.view(np.uint32))


def test_reduce_ordered_two_chains_in_one_launch(dev):
    """Two destinations whose jobs arrive interleaved: the descriptor groups them into chains and keeps the caller's order."""
    from maestro_amd import hip
    gs = guards.GuardSet(dev)
    a = [order_sensitive(r, 516, seed=90 + i) for i, r in enumerate((100, 17))]
    b = [order_sensitive(r, 4, seed=95 + i) for i, r in enumerate((33, 16, 1))]
    sa = [_inp(gs, torch.from_numpy(s), ld=520, name="a")[1] for s in a]
    sb = [_inp(gs, torch.from_numpy(s), ld=12, name="b")[1] for s in b]
    da, dsa = _out(gs, (1, 516), name="dst a")
    db, dsb = _out(gs, (1, 4), name="dst b")
    jobs = [(sa[0], dsa, 100, 516, 520), (sb[0], dsb, 33, 4, 12), (sa[1], dsa, 17, 516, 520), (sb[1], dsb, 16, 4, 12),
            (sb[2], dsb, 1, 4, 12)]
    table = hip.OrderedReduce(jobs, dev)
    assert table.n_chains == 2 and table.n == 5
    _three_launches(table.launch, [da, db])
    gs.check()
    assert np.array_equal(da[0].cpu().numpy().view(np.uint32), ordered_reduce_emulated(a).view(np.uint32))
    assert np.array_equal(db[0].cpu().numpy().view(np.uint32), ordered_reduce_emulated(b).view(np.uint32))


# ------------------------------------------------------------------------------------------------ K-slice slab GEMMs
@pytest.mark.parametrize("K", [1024, 2048, 2100, 8200])        # 1, 2 (even), 2 (ragged last slice: 1088 + 1012), 8 slices (1088 x 7 + 584)
def test_gemm_tn_slabs_then_ordered_reduce(dev, K):  # noqa: N803
    """dW[M, N] = A[K, M]^T B[K, N] through ``hip.gemm_tn_slabs`` (plain-store TN GEMMs on consecutive K-slices into private slabs)
    and one ordered job over the slabs.  Every row of K counts exactly once: row k of A is scaled by a weight that differs from row
    to row, so a dropped, repeated or misplaced slice moves the result far outside the accumulation bound."""
    from maestro_amd import hip
    M, N = 64, 72  # noqa: N806
    S = hip.det_slices(K)  # noqa: N806
    assert S == {1024: 1, 2048: 2, 2100: 2, 8200: 8}[K]
    g = torch.Generator().manual_seed(K)
    gs = guards.GuardSet(dev)
    ramp = 0.5 + torch.arange(K, dtype=F32)[:, None] / K
    a_h = numerics.bf16_round(torch.randn(K, M, generator=g) * ramp)
    b_h = numerics.bf16_round(torch.randn(K, N, generator=g) * K ** -0.5)
    a, _ = _inp(gs, a_h.to(BF16), ld=M + 8, name="A")
    b, _ = _inp(gs, b_h.to(BF16), ld=N + 16, name="B")
    slabs, sspan = _out(gs, (S, M * N), name="slabs")
    dst, dspan = _out(gs, (1, M * N), name="dW")
    table = hip.OrderedReduce([(sspan, dspan, S, M * N, M * N)], dev)

    def run():
        hip.gemm_tn_slabs(M, N, K, a, M + 8, b, N + 16, slabs.view(S, M, N))
        table.launch()
    _three_launches(run, [slabs, dst])
    gs.check()
    c64, absprod = numerics.gemm_ref64(a_h.t(), b_h)
    _within(dst[0].view(M, N), c64, numerics.gemm_bound(absprod, K), f"slab GEMM K={K} ({S} slices)")
    # each slab is its own K-slice, nothing else: slice i covers rows [i * step, min(K, (i + 1) * step))
    step = -(-(-(-K // S)) // 64) * 64
    for i in range(S):
        ai, bi = a_h[i * step: (i + 1) * step], b_h[i * step: (i + 1) * step]
        ci, api = numerics.gemm_ref64(ai.t(), bi)
        _within(slabs[i].view(M, N), ci, numerics.gemm_bound(api, ai.shape[0]), f"slab {i} of K={K}")
    # and the last hop is the emulated order, bit for bit
    want = ordered_reduce_emulated([slabs.cpu().numpy()])
    assert np.array_equal(dst[0].cpu().numpy().view(np.uint32), want.view(np.uint32))


# ------------------------------------------------------------------------------------------------ column sums
@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("N", [4, 260])
@pytest.mark.parametrize("M", [1, 256, 257])
def test_colsum_partial_then_ordered_reduce(dev, M, N, dtype):  # noqa: N803
    from maestro_amd import hip
    assert hip.COLSUM_PARTIAL_ROWS == 256 and hip.colsum_partial_rows(256) == 1 and hip.colsum_partial_rows(257) == 2
    gs = guards.GuardSet(dev)
    x = torch.from_numpy(order_sensitive(M, N, seed=M + N)).to(dtype)
    xv, _ = _inp(gs, x, ld=N + 8, name="x")
    rows = hip.colsum_partial_rows(M)
    part, pspan = _out(gs, (rows, N), name="partial")
    dst, dspan = _out(gs, (1, N), name="dst")
    table = hip.OrderedReduce([(pspan, dspan, rows, N, N)], dev)

    def run():
        hip.colsum_partial(xv, part, M, N, N + 8)
        table.launch()
    _three_launches(run, [part, dst])
    gs.check()
    x64 = x.double()
    _within(dst[0], x64.sum(0), numerics.gemm_bound(x64.abs().sum(0), M), f"colsum {M}x{N} {dtype}")
    # the row blocks are what the header says: block i sums rows [256 i, 256 i + 256)
    for i in range(rows):
        blk = x64[256 * i: 256 * (i + 1)]
        _within(part[i], blk.sum(0), numerics.gemm_bound(blk.abs().sum(0), blk.shape[0]), f"colsum block {i}")


# ------------------------------------------------------------------------------------------------ masked loss
def _loss_case(dev, PPC, p, bands, empty):  # noqa: N803
    from maestro_amd import hip
    B, Lm, tok_off, Lg = 2, 9, 2, 14  # noqa: N806
    g = torch.Generator().manual_seed(PPC * 10 + p + 100 * bands)
    gs = guards.GuardSet(dev)
    tgt_C, c0, n_g = (5, 1, 3) if bands else (1, 0, 1)  # noqa: N806
    tgt_cols = PPC // n_g * tgt_C if bands else PPC
    rec_h, tgt_h = torch.randn(B * Lm, PPC, generator=g), torch.randn(B * Lm, tgt_cols, generator=g)
    mask_h = torch.zeros(B, Lg, dtype=torch.uint8) if empty else (torch.rand(B, Lg, generator=g) < 0.6).to(torch.uint8)
    if not empty:
        mask_h[0, tok_off] = 1
    sel = mask_h[:, tok_off: tok_off + Lm].reshape(-1).bool()
    n_tok = int(sel.sum())
    count = n_tok * PPC if bands else n_tok          # the bands form divides by ELEMENTS, the plain one by tokens * PPC
    rec, _ = _inp(gs, rec_h, name="rec")
    tgt, _ = _inp(gs, tgt_h, name="target")
    mask, _ = _inp(gs, mask_h, name="mask")
    cnt = torch.tensor([count], dtype=torch.int32, device=dev)
    weight = 0.625
    n_part = hip.masked_loss_partial_size(B, Lm)
    part, pspan = _out(gs, (1, n_part), name="loss partial")
    drec, _ = _out(gs, (B * Lm, PPC), dtype=BF16, name="drec")
    loss, lspan = _out(gs, (1, 1), name="loss")
    table = hip.OrderedReduce([(pspan, lspan, n_part, 1, 1)], dev)

    def run():
        if bands:
            hip.masked_loss_bands_det(rec, tgt, mask, cnt, weight, part, drec, B, Lm, Lg, tok_off, PPC, p, tgt_C, c0, n_g)
        else:
            hip.masked_loss_det(rec, tgt, mask, cnt, weight, part, drec, B, Lm, Lg, tok_off, PPC, p)
        table.launch()
    _three_launches(run, [part, drec, loss])
    gs.check()
    # drec of the existing kernel, bit for bit
    acc = torch.zeros(1, device=dev)
    drec0 = torch.full((B * Lm, PPC), float("nan"), dtype=BF16, device=dev)
    if bands:
        hip.masked_loss_bands(rec, tgt, mask, cnt, weight, acc, drec0, B, Lm, Lg, tok_off, PPC, p, tgt_C, c0, n_g)
    else:
        hip.masked_loss(rec, tgt, mask, cnt, weight, acc, drec0, B, Lm, Lg, tok_off, PPC, p)
    torch.cuda.synchronize()
    assert guards.bits_equal(drec.contiguous(), drec0), "drec differs from the existing kernel's"
    if empty:
        assert torch.isnan(loss).all() and torch.isnan(acc).all() and (drec.float() == 0).all()
        return
    t64 = tgt_h.double()
    if bands:
        t64 = t64.reshape(B * Lm, PPC // n_g, tgt_C)[:, :, c0: c0 + n_g].reshape(B * Lm, PPC)
    diff = (rec_h.double() - t64)[sel]
    terms = diff.abs() if p == 1 else diff * diff
    coef = weight / (n_tok * PPC)
    want = terms.sum() * coef
    bound = numerics.gemm_bound(terms.sum() * coef, terms.numel())
    _within(loss.reshape(()), want, bound, f"masked loss PPC={PPC} p={p} bands={bands}")
    assert abs(acc.item() - want.item()) <= 1e-5 * abs(want.item())       # the two kernels compute the same loss


@pytest.mark.parametrize("p", [1, 2])
@pytest.mark.parametrize("PPC", [12, 260])
def test_masked_loss_det(dev, PPC, p):  # noqa: N803
    _loss_case(dev, PPC, p, bands=False, empty=False)


@pytest.mark.parametrize("p", [1, 2])
def test_masked_loss_bands_det(dev, p):
    _loss_case(dev, 12, p, bands=True, empty=False)


def test_masked_loss_det_empty_selection_is_nan(dev):
    _loss_case(dev, 12, 2, bands=False, empty=True)


# ------------------------------------------------------------------------------------------------ mask-token gradient
@pytest.mark.parametrize("L", [130, 300])                       # 260 rows: one workgroup; 600 rows: two
@pytest.mark.parametrize("per_sample", [False, True])
def test_unmask_token_grad_det(dev, per_sample, L):  # noqa: N803
    from maestro_amd import hip
    B, Dd, slot = 2, 64, 1  # noqa: N806
    g = torch.Generator().manual_seed(5 + L + per_sample)
    gs = guards.GuardSet(dev)
    dx_h = torch.from_numpy(order_sensitive(B * L, Dd, seed=L))
    mask_h = (torch.rand(B, L, generator=g) < 0.6).to(torch.uint8)
    slots_h = torch.randint(0, 2, (B, L) if per_sample else (L,), generator=g, dtype=torch.int32)
    t_lo, t_hi = (0, L) if per_sample else (3, L - 2)
    dx, _ = _inp(gs, dx_h, name="dx")
    mask, _ = _inp(gs, mask_h, name="mask")
    slots, _ = _inp(gs, slots_h.reshape(-1, L), name="slots")
    rows = hip.unmask_token_grad_partial_rows(B * (t_hi - t_lo))
    assert rows == (1 if L == 130 else 2)
    part, pspan = _out(gs, (rows, Dd), name="partial")
    dst, dspan = _out(gs, (1, Dd), name="dst")
    table = hip.OrderedReduce([(pspan, dspan, rows, Dd, Dd)], dev)

    def run():
        if per_sample:
            hip.unmask_token_grad_per_sample_det(dx, mask, slots, part, B, L, Dd, slot)
        else:
            hip.unmask_token_grad_det(dx, mask, slots, part, B, L, Dd, slot, t_lo, t_hi)
        table.launch()
    _three_launches(run, [part, dst])
    gs.check()
    sl = slots_h if per_sample else slots_h[None].expand(B, L)
    pick = (mask_h.bool() & (sl == slot))
    pick[:, :t_lo] = False
    pick[:, t_hi:] = False
    x64 = dx_h.double().reshape(B, L, Dd)[pick]
    _within(dst[0], x64.sum(0), numerics.gemm_bound(x64.abs().sum(0), max(1, x64.shape[0])), f"token grad L={L}")
    # the existing kernel computes the same sums
    ref = torch.zeros(Dd, device=dev)
    if per_sample:
        hip.unmask_token_grad_per_sample(dx, mask, slots, ref, B, L, Dd, slot)
    else:
        hip.unmask_token_grad(dx, mask, slots, ref, B, L, Dd, slot, t_lo, t_hi)
    _within(ref, x64.sum(0), numerics.gemm_bound(x64.abs().sum(0), max(1, x64.shape[0])), "token grad, existing kernel")


# ------------------------------------------------------------------------------------------------ GroupNorm backward
@pytest.mark.parametrize("E", [64, 192, 1028])      # 1028: two column passes (E > 1024)
def test_embed_finish_bwd_det(dev, E):  # noqa: N803
    from maestro_amd import hip
    B, D, L, tok_off, Lg = 3, 1, 33, 2, 38  # noqa: N806
    BD = B * D  # noqa: N806
    g = torch.Generator().manual_seed(E)
    gs = guards.GuardSet(dev)
    y_h = torch.randn(BD * L, E, generator=g) * 1.7 + 0.3
    gamma_h = 1 + 0.2 * torch.randn(E, generator=g)
    dxg_h = torch.randn(B, Lg, E, generator=g)
    img = y_h.double().reshape(BD, L * E)
    mu, rs = img.mean(1), 1.0 / torch.sqrt(img.var(1, unbiased=False) + 1e-5)
    stats_h = torch.stack([mu, rs], 1).float()
    y, _ = _inp(gs, y_h, name="y")
    gamma, _ = _inp(gs, gamma_h[None], name="gamma")
    dxg, _ = _inp(gs, dxg_h, name="dxg")
    stats, _ = _inp(gs, stats_h, name="stats")
    rows = hip.embed_bwd_partial_rows(BD, L)
    assert rows == 6
    part, pspan = _out(gs, (rows, 2 * E), name="param partial")
    blk, _ = _out(gs, (rows, 2), name="block sums")
    sums, _ = _out(gs, (BD, 2), name="sums")
    dyc, _ = _out(gs, (BD * L, E), dtype=BF16, name="dyc")
    dg, dgs = _out(gs, (1, E), name="dgamma")
    db, dbs = _out(gs, (1, E), name="dbeta")
    table = hip.OrderedReduce([(pspan, dgs, rows, E, 2 * E), (pspan[E:], dbs, rows, E, 2 * E)], dev)

    def run():
        hip.embed_finish_bwd_det(dxg, y, stats, gamma, dyc, part, blk, sums, B, D, L, E, tok_off, Lg)
        table.launch()
    _three_launches(run, [part, blk, sums, dyc, dg, db])
    gs.check()
    # fp64 with the fp32 statistics the kernel was given
    mu32, rs32 = stats_h[:, 0].double()[:, None, None], stats_h[:, 1].double()[:, None, None]
    z = (y_h.double().reshape(BD, L, E) - mu32) * rs32
    d = dxg_h.double()[:, tok_off: tok_off + D * L].reshape(BD, L, E)
    n_terms = BD * L
    _within(dg[0], (d * z).sum((0, 1)), numerics.gemm_bound((d * z).abs().sum((0, 1)), n_terms), f"dgamma E={E}")
    _within(db[0], d.sum((0, 1)), numerics.gemm_bound(d.abs().sum((0, 1)), n_terms), f"dbeta E={E}")
    dz = d * gamma_h.double()
    s1, s2 = dz.sum((1, 2)), (dz * z).sum((1, 2))
    per_img = L * E
    _within(sums[:, 0], s1, numerics.gemm_bound(dz.abs().sum((1, 2)), per_img), "S1")
    _within(sums[:, 1], s2, numerics.gemm_bound((dz * z).abs().sum((1, 2)), per_img), "S2")
    want = rs32 * (dz - s1[:, None, None] / (L * E) - z * s2[:, None, None] / (L * E))
    scale = want.abs().max().item()
    err = (dyc.float().double().cpu().reshape(BD, L, E) - want).abs().max().item()
    print(f"dyc E={E}: max error {err:.3e} of scale {scale:.3e}")
    assert err < 2e-2 * scale                      # the tolerance tests/test_kernels_gpu.py states for dyc
