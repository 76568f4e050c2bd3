"""The ends of the pretraining step's backward (pixelify head, final LayerNorms, enc_to_dec, patch embed) in their batched form:
weight gradients as problems of the grouped TN launch, bias / LayerNorm side reductions as partial rows summed by one batched
column sum, the patch-embed backward through the position map (include/maestro_hip.h).

Bounds are derived, not observed.  u = 2^-24 (fp32 unit roundoff), and:
  * an fp32 sum of n terms, in ANY order (wave tree, LDS, row chunks, atomics):  |err| <= 2 n u sum|term|, sum|term| in fp64
    (first order n u sum|term|; the factor 2 covers the higher orders and the rounding of the terms' own products);
  * a kernel that reads bf16 inputs is compared with fp64 arithmetic on those same bf16 values;
  * a value stored as bf16 (8 significant bits, round to nearest even): |bf16(v) - v| <= 2^-8 |v|.
"""

from __future__ import annotations

import pytest
import torch

from tests import guards

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
F32, BF16, I32, U8 = torch.float32, torch.bfloat16, torch.int32, torch.uint8


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _reduce(dev, src, rows, cols, ld=None):
    """One ``ColsumBatch`` job: the column sums of the partial rows ``src`` [rows, ld] into a zeroed vector."""
    from maestro_amd import hip
    out = torch.zeros(cols, dtype=F32, device=dev)
    hip.ColsumBatch([(src.reshape(-1), out, rows, cols, ld or cols)], dev).launch()
    torch.cuda.synchronize()
    return out


def _assert_colsum(name, got, stored, n_terms):
    """``got`` against the fp64 column sums of the STORED tensor (bf16 or f32 [rows, cols]) within the n-term bound."""
    ref = stored.double().sum(0)
    bound = 2 * n_terms * U * stored.double().abs().sum(0) + 1e-45
    err = (got.double() - ref).abs()
    print(f"{name}: column sums max err {err.max().item():.3e}, max err / bound {(err / bound).max().item():.3f}")
    assert bool((err <= bound).all()), (name, (err / bound).max().item())


# ================================================================================================ guard bands (tests/guards.py)
# The ledger of tests/guards.py counts the calls below this banner: the kernel tests from here on keep their operands in a GuardSet.
# ================================================================================================ 1. LayerNorm backward, new forms
def _ln_reference(dy, x, gamma, mean, rstd):
    """fp64 LayerNorm backward on the operands the kernel reads; rows = leading dimension.  Returns dx and its bound, the three
    reductions and their bounds."""
    dy, x, gamma, mu, rs = dy.double(), x.double(), gamma.double(), mean.double()[:, None], rstd.double()[:, None]
    rows, dim = x.shape
    xh, dz = (x - mu) * rs, dy * gamma
    c1, c2 = dz.mean(1, keepdim=True), (dz * xh).mean(1, keepdim=True)
    dx = rs * (dz - c1 - xh * c2)
    # the two row sums have dim terms each (8 more for the roundings inside a term); then a handful of elementwise roundings
    e_c1 = 2 * (dim + 8) * U * dz.abs().sum(1, keepdim=True) / dim
    e_c2 = 2 * (dim + 8) * U * (dz * xh).abs().sum(1, keepdim=True) / dim
    dx_bound = rs.abs() * (e_c1 + xh.abs() * e_c2 + 8 * U * (dz.abs() + c1.abs() + (xh * c2).abs())) + 1e-45
    dgamma, dbeta, dcol = (dy * xh).sum(0), dy.sum(0), dx.sum(0)
    g_bound = 2 * (rows + 8) * U * (dy * xh).abs().sum(0) + 1e-45
    b_bound = 2 * rows * U * dy.abs().sum(0) + 1e-45
    c_bound = 2 * rows * U * dx.abs().sum(0) + 2 * dx_bound.sum(0)       # the sum's own error + the errors of its terms
    return dx, dx_bound, (dgamma, g_bound), (dbeta, b_bound), (dcol, c_bound)


def _ln_case(dev, B, n, dim, dy_f32, seed):  # noqa: N803
    """Operands in guarded buffers: x / dx rows through the map (x_L > n, x_off > 0), dy through its own map (dy_off > 0)."""
    from maestro_amd import hip
    g = torch.Generator().manual_seed(seed)
    x_L, x_off, dy_L, dy_off = n + 3, 2, n + 2, 1  # noqa: N806
    gs = guards.GuardSet(dev)
    x = gs.inp(torch.randn(B * x_L, dim, generator=g) * 1.5 + 0.3, name="x")
    dy_data = torch.randn(B * dy_L, dim, generator=g)
    dy = gs.inp(dy_data if dy_f32 else dy_data.to(BF16), name="dy")
    gamma = gs.inp(1.0 + 0.2 * torch.randn(dim, generator=g), name="gamma")
    rows_x = torch.cat([torch.arange(b * x_L + x_off, b * x_L + x_off + n) for b in range(B)])
    rows_dy = torch.cat([torch.arange(b * dy_L + dy_off, b * dy_L + dy_off + n) for b in range(B)])
    xs = x[rows_x.to(dev)]
    mean = gs.inp(xs.mean(1).cpu(), name="mean")
    rstd = gs.inp((xs.var(1, unbiased=False) + 1e-5).rsqrt().cpu(), name="rstd")
    dx = gs.out((B * x_L, dim), F32, name="dx")
    dx16 = gs.out((B * x_L, dim), BF16, name="dx_bf16")
    ws_rows = hip.layernorm_bwd_workspace(B * n, dim) // (3 * dim)
    ws = gs.out((ws_rows, 3 * dim), F32, name="workspace")
    return dict(gs=gs, x=x, dy=dy, gamma=gamma, mean=mean, rstd=rstd, dx=dx, dx16=dx16, ws=ws, ws_rows=ws_rows, rows_x=rows_x.to(dev),
                rows_dy=rows_dy.to(dev), maps=(dy_L, dy_off, x_L, x_off))


def _ln_partial(c, B, n, dim):  # noqa: N803
    from maestro_amd import hip
    dy_L, dy_off, x_L, x_off = c["maps"]  # noqa: N806
    hip.layernorm_bwd_partial(c["dy"], dy_L, dy_off, c["x"], x_L, x_off, c["gamma"], c["mean"], c["rstd"], None, c["dx"], c["dx16"],
                              c["ws"].view(-1), B, n, dim)
    c["gs"].check()


def _ln_check(dev, c, B, n, dim):  # noqa: N803
    ref_dx, dx_bound, *reds = _ln_reference(c["dy"][c["rows_dy"]], c["x"][c["rows_x"]], c["gamma"], c["mean"], c["rstd"])
    got = c["dx"][c["rows_x"]].double()
    err = (got - ref_dx).abs()
    print(f"ln_bwd B={B} n={n} dim={dim} {c['dy'].dtype}: dx max err {err.max().item():.3e}, max err / bound {(err / dx_bound).max().item():.3f}")
    assert bool((err <= dx_bound).all()), (err / dx_bound).max().item()
    err16 = (c["dx16"][c["rows_x"]].double() - ref_dx).abs()
    bound16 = dx_bound + 2.0 ** -8 * (ref_dx.abs() + dx_bound) + 1e-40
    assert bool((err16 <= bound16).all()), (err16 / bound16).max().item()
    # rows of the shared sequence buffer that the map does not name keep their poison
    other = torch.ones(c["dx"].shape[0], dtype=torch.bool, device=dev)
    other[c["rows_x"]] = False
    assert bool(torch.isnan(c["dx"][other]).all()) and bool(torch.isnan(c["dx16"][other].float()).all())
    flat = c["ws"].view(-1)
    for k, (name, (ref, bound)) in enumerate(zip(("dgamma", "dbeta", "dcol"), reds)):
        got = _reduce(dev, flat[k * dim:], c["ws_rows"], dim, 3 * dim).double()
        e = (got - ref).abs()
        print(f"   {name}: max err {e.max().item():.3e}, max err / bound {(e / bound).max().item():.3f}")
        assert bool((e <= bound).all()), (name, (e / bound).max().item())


@pytest.mark.parametrize("dy_f32", [False, True], ids=["dy_bf16", "dy_f32"])
@pytest.mark.parametrize("B,n", [(2, 4), (3, 8)])
@pytest.mark.parametrize("dim", [256, 512, 768, 1024])
def test_final_layernorm_backward_forms(dim, B, n, dy_f32):  # noqa: N803
    """The straight-line forms without a residual gradient (bf16 and fp32 dy): rows % 4 == 0, dim = 256 NV for every NV (1024:
    two rows in flight instead of four); 8 rows = one workgroup with two idle waves, 24 rows = two workgroups.  Then the same
    operands without parameter gradients (no workspace: the kernel leaves before its block tail): the same dx, bit for bit."""
    from maestro_amd import hip
    dev = _dev()
    c = _ln_case(dev, B, n, dim, dy_f32, seed=100 + dim + 10 * B + int(dy_f32))
    _ln_partial(c, B, n, dim)
    _ln_check(dev, c, B, n, dim)
    dy_L, dy_off, x_L, x_off = c["maps"]  # noqa: N806
    gs = guards.GuardSet(dev)
    dx, dx16 = gs.out((B * x_L, dim), F32, name="dx (no sums)"), gs.out((B * x_L, dim), BF16, name="dx_bf16 (no sums)")
    hip.layernorm_bwd(c["dy"], dy_L, dy_off, c["x"], x_L, x_off, c["gamma"], c["mean"], c["rstd"], None, dx, dx16, None, None, None, None,
                      B, n, dim)
    gs.check()
    assert guards.bits_equal(dx[c["rows_x"]], c["dx"][c["rows_x"]]) and guards.bits_equal(dx16[c["rows_x"]], c["dx16"][c["rows_x"]])


@pytest.mark.parametrize("dy_f32", [False, True], ids=["dy_bf16", "dy_f32"])
def test_final_layernorm_backward_odd_rows_take_the_generic_kernel(dy_f32):
    """rows % 4 != 0 (1 x 6): a wave's four rows do not all exist, the generic kernel runs -- the same bits as the two-launch
    entry point gives (generic kernel as well), nothing written outside the outputs."""
    from maestro_amd import hip
    dev = _dev()
    B, n, dim = 1, 6, 512  # noqa: N806
    c = _ln_case(dev, B, n, dim, dy_f32, seed=77 + int(dy_f32))
    _ln_partial(c, B, n, dim)
    _ln_check(dev, c, B, n, dim)
    dy_L, dy_off, x_L, x_off = c["maps"]  # noqa: N806
    gs = guards.GuardSet(dev)
    dx, dx16 = gs.out((B * x_L, dim), F32, name="dx (two launches)"), gs.out((B * x_L, dim), BF16, name="dx_bf16 (two launches)")
    ws = gs.out((c["ws_rows"], 3 * dim), F32, name="workspace (two launches)")
    sums = [gs.out((dim,), F32, init=0.0, name=k) for k in ("dgamma", "dbeta", "dcol")]
    hip.layernorm_bwd(c["dy"], dy_L, dy_off, c["x"], x_L, x_off, c["gamma"], c["mean"], c["rstd"], None, dx, dx16, *sums, ws.view(-1),
                      B, n, dim)
    gs.check()
    assert guards.bits_equal(dx[c["rows_x"]], c["dx"][c["rows_x"]]) and guards.bits_equal(dx16[c["rows_x"]], c["dx16"][c["rows_x"]])
    assert guards.bits_equal(ws, c["ws"])          # the same partial rows, hence the same sums up to the order of the last adds


# ================================================================================================ 2. producer-fused column sums
@pytest.mark.parametrize("bands", [False, True], ids=["plain", "band_group"])
@pytest.mark.parametrize("all_visible", [False, True], ids=["mixed", "nothing_masked"])
def test_masked_loss_leaves_its_bias_gradient_as_partial_rows(bands, all_visible):
    """Beff = 2, n_tok = 5, K = 16 (three workgroups of four rows).  "mixed": sample 1 has no masked token (its drec rows are
    zeros); "nothing_masked": no token of the modality is masked -- NaN loss, finite (zero) gradient."""
    from maestro_amd import hip
    dev = _dev()
    B, Lm, K, Lgroup, tok_off, p = 2, 5, 16, 8, 2, 2  # noqa: N806
    n_g, tgt_C, tgt_c0 = (4, 6, 1) if bands else (1, 1, 0)  # noqa: N806
    tgt_cols = K // n_g * tgt_C if bands else K
    mask = torch.zeros(B, Lgroup, dtype=U8)
    if not all_visible:
        mask[0, tok_off + 0] = mask[0, tok_off + 2] = mask[0, tok_off + 3] = 1
    mask[1, 0] = 1                                  # another modality's token: outside [tok_off, tok_off + Lm)
    n_masked = int(mask[:, tok_off: tok_off + Lm].sum())
    cnt = torch.tensor([n_masked * (K if bands else 1)], dtype=I32, device=dev)
    outs = []
    for fused in (False, True):
        gs = guards.GuardSet(dev)
        rec = gs.inp(torch.randn(B * Lm, K, generator=torch.Generator().manual_seed(9)), name="rec")
        tgt = gs.inp(torch.randn(B * Lm, tgt_cols, generator=torch.Generator().manual_seed(10)), name="target")
        msk = gs.inp(mask, fill=0, name="mask")
        acc = gs.out((1,), F32, init=0.0, name="loss")
        drec = gs.out((B * Lm, K), BF16, name="drec")
        rows = hip.masked_loss_cs_rows(B, Lm)
        cs = gs.out((rows, K), F32, name="cs_partial") if fused else None
        args = (B, Lm, Lgroup, tok_off, K, p) + ((tgt_C, tgt_c0, n_g) if bands else ())
        if fused and bands:
            hip.masked_loss_bands_cs(rec, tgt, msk, cnt, 0.7, acc, drec, cs, *args)
        elif fused:
            hip.masked_loss_cs(rec, tgt, msk, cnt, 0.7, acc, drec, cs, *args)
        elif bands:
            hip.masked_loss_bands(rec, tgt, msk, cnt, 0.7, acc, drec, *args)
        else:
            hip.masked_loss(rec, tgt, msk, cnt, 0.7, acc, drec, *args)
        gs.check()
        outs.append((acc.clone(), drec.clone(), cs))
    (loss0, drec0, _), (loss1, drec1, cs) = outs
    assert guards.bits_equal(drec0, drec1)
    assert bool(torch.isfinite(drec1.float()).all())
    if all_visible:
        assert bool(torch.isnan(loss0).all()) and bool(torch.isnan(loss1).all()) and float(drec1.float().abs().max()) == 0.0
    else:
        assert float(drec1.float().abs().max()) > 0 and float(drec1[Lm:].float().abs().max()) == 0.0
        assert abs(loss0.item() - loss1.item()) <= 2 * 3 * U * abs(loss0.item()) * 2     # three workgroups' partial losses, any order
    assert rows == 3
    _assert_colsum("masked_loss", _reduce(dev, cs, rows, K), drec1, B * Lm)


def test_embed_apply_leaves_the_conv_bias_gradient_as_partial_rows():
    """T = 10 tokens (B = 2, D = 1, L = 5) at E = 4, the smallest width the kernels accept; dense gradient (no position map):
    dyc bit for bit what the present launch writes."""
    from maestro_amd import hip
    dev = _dev()
    B, D, L, E, tok_off, Lgroup = 2, 1, 5, 4, 1, 7  # noqa: N806
    g = torch.Generator().manual_seed(21)
    y, dxg = torch.randn(B * D * L, E, generator=g), torch.randn(B * Lgroup, E, generator=g)
    stats = torch.stack([torch.randn(B * D, generator=g) * 0.1, 0.5 + torch.rand(B * D, generator=g)], 1)
    gamma = 1.0 + 0.2 * torch.randn(E, generator=g)
    outs = []
    for fused in (False, True):
        gs = guards.GuardSet(dev)
        a = dict(dxg=gs.inp(dxg, name="dxg"), y=gs.inp(y, name="y"), stats=gs.inp(stats, name="stats"), gamma=gs.inp(gamma, name="gamma"))
        dyc = gs.out((B * D * L, E), BF16, name="dyc")
        dgamma, dbeta = gs.out((E,), F32, init=0.0, name="dgamma"), gs.out((E,), F32, init=0.0, name="dbeta")
        sums = gs.out((B * D, 2), F32, name="sums")
        rows = hip.embed_bwd_cs_rows(B * D * L)
        cs = gs.out((rows, E), F32, name="cs_partial") if fused else None
        if fused:
            hip.embed_finish_bwd_ends(a["dxg"], None, 0, a["y"], a["stats"], a["gamma"], dyc, dgamma, dbeta, sums, cs, B, D, L, E, tok_off, Lgroup)
        else:
            hip.embed_finish_bwd(a["dxg"], a["y"], a["stats"], a["gamma"], dyc, dgamma, dbeta, sums, B, D, L, E, tok_off, Lgroup)
        gs.check()
        outs.append((dyc.clone(), dgamma.clone(), dbeta.clone(), sums.clone(), cs))
    assert guards.bits_equal(outs[0][0], outs[1][0])
    for k in (1, 2, 3):      # one workgroup per image here: the same adds in the same order
        assert guards.bits_equal(outs[0][k], outs[1][k])
    assert rows == 1
    _assert_colsum("embed_bwd_apply", _reduce(dev, outs[1][4], rows, E), outs[1][0], B * D * L)


def test_embed_ends_form_refuses_a_width_above_1024():
    """E = 1028 is a width the plain and deterministic forms take (in two column passes); the ends form keeps its columns' sums in
    registers and refuses it before any launch: the outputs keep the values they were given."""
    from maestro_amd import hip
    dev = _dev()
    B, D, L, E = 1, 1, 3, 1028  # noqa: N806
    g = torch.Generator().manual_seed(22)
    gs = guards.GuardSet(dev)
    dxg, y = gs.inp(torch.randn(B * L, E, generator=g), name="dxg"), gs.inp(torch.randn(B * L, E, generator=g), name="y")
    stats, gamma = gs.inp(torch.tensor([[0.1, 0.9]]), name="stats"), gs.inp(torch.ones(E), name="gamma")
    outs = [gs.out((B * L, E), BF16, init=3.0, name="dyc"), gs.out((E,), F32, init=3.0, name="dgamma"), gs.out((E,), F32, init=3.0, name="dbeta"),
            gs.out((B * D, 2), F32, init=3.0, name="sums"), gs.out((hip.embed_bwd_cs_rows(B * L), E), F32, init=3.0, name="cs_partial")]
    with pytest.raises(hip.HipExtensionError):
        hip.embed_finish_bwd_ends(dxg, None, 0, y, stats, gamma, *outs, B, D, L, E, 0, L)
    torch.cuda.synchronize()
    gs.check()
    assert all(bool((o == 3.0).all()) for o in outs)


def test_gather_writes_the_bf16_rows_and_their_column_sums():
    """M = 6 rows (B = 2, three visible of five) at Dd = 512: dst16 = cast_bf16(gather_rows(src)) bit for bit."""
    from maestro_amd import hip
    dev = _dev()
    B, src_L, n_idx, dim = 2, 5, 3, 512  # noqa: N806
    g = torch.Generator().manual_seed(33)
    gs = guards.GuardSet(dev)
    src = gs.inp(torch.randn(B * src_L, dim, generator=g), name="src")
    idx = gs.inp(torch.tensor([[4, 0, 2], [1, 3, 4]], dtype=I32), fill=0, name="idx")
    dst16 = gs.out((B * n_idx, dim), BF16, name="dst16")
    rows = hip.gather_rows_cs_rows(B * n_idx)
    cs = gs.out((rows, dim), F32, name="cs_partial")
    hip.gather_rows_bf16_cs(src, idx, dst16, cs, B, src_L, n_idx, dim)
    gs.check()
    f32 = torch.empty(B * n_idx, dim, dtype=F32, device=dev)
    want = torch.empty(B * n_idx, dim, dtype=BF16, device=dev)
    hip.gather_rows(src, idx, f32, B, src_L, n_idx, dim, n_idx, 0)
    hip.cast_bf16(f32, want, B * n_idx * dim)
    torch.cuda.synchronize()
    assert guards.bits_equal(dst16, want)
    assert rows == 1
    _assert_colsum("gather_rows_bf16_cs", _reduce(dev, cs, rows, dim), dst16, B * n_idx)


def test_producers_with_several_workgroups_and_column_chunks():
    """T = 200 rows at 768 columns: 50 / 7 / 7 workgroups (the blockIdx -> partial-row indexing, a short last workgroup) and three
    256-column chunks per lane (the j > 0 registers and their LDS layout), which the issue's smallest shapes above do not reach."""
    from maestro_amd import hip
    dev = _dev()
    g = torch.Generator().manual_seed(91)
    B, L, C, T = 2, 100, 768, 200  # noqa: N806
    # ---- masked loss: drec bit for bit what the present launch writes (no sum feeds it), column sums of the stored values
    Lgroup, tok_off = L + 4, 3  # noqa: N806
    mask = (torch.rand(B, Lgroup, generator=g) < 0.5).to(U8)
    cnt = torch.tensor([int(mask[:, tok_off: tok_off + L].sum())], dtype=I32, device=dev)
    rec, tgt = torch.randn(T, C, generator=g), torch.randn(T, C, generator=g)
    outs = []
    for fused in (False, True):
        gs = guards.GuardSet(dev)
        r, t, m = gs.inp(rec, name="rec"), gs.inp(tgt, name="target"), gs.inp(mask, fill=0, name="mask")
        acc, drec = gs.out((1,), F32, init=0.0, name="loss"), gs.out((T, C), BF16, name="drec")
        rows = hip.masked_loss_cs_rows(B, L)
        cs = gs.out((rows, C), F32, name="cs_partial") if fused else None
        if fused:
            hip.masked_loss_cs(r, t, m, cnt, 0.7, acc, drec, cs, B, L, Lgroup, tok_off, C, 2)
        else:
            hip.masked_loss(r, t, m, cnt, 0.7, acc, drec, B, L, Lgroup, tok_off, C, 2)
        gs.check()
        outs.append((drec.clone(), cs))
    assert rows == 50 and guards.bits_equal(outs[0][0], outs[1][0]) and float(outs[1][0].float().abs().max()) > 0
    _assert_colsum("masked_loss 200 x 768", _reduce(dev, outs[1][1], rows, C), outs[1][0], T)
    # ---- gather + cast: bit for bit the two present launches
    src_L, n_idx = 130, L  # noqa: N806
    gs = guards.GuardSet(dev)
    src = gs.inp(torch.randn(B * src_L, C, generator=g), name="src")
    idx = gs.inp(torch.stack([torch.randperm(src_L, generator=g)[:n_idx] for _ in range(B)]).to(I32), fill=0, name="idx")
    dst16 = gs.out((T, C), BF16, name="dst16")
    rows = hip.gather_rows_cs_rows(T)
    cs = gs.out((rows, C), F32, name="cs_partial")
    hip.gather_rows_bf16_cs(src, idx, dst16, cs, B, src_L, n_idx, C)
    gs.check()
    f32, ref16 = torch.empty(T, C, dtype=F32, device=dev), torch.empty(T, C, dtype=BF16, device=dev)
    hip.gather_rows(src, idx, f32, B, src_L, n_idx, C, n_idx, 0)
    hip.cast_bf16(f32, ref16, T * C)
    torch.cuda.synchronize()
    assert rows == 7 and guards.bits_equal(dst16, ref16)
    _assert_colsum("gather 200 x 768", _reduce(dev, cs, rows, C), dst16, T)
    # ---- patch-embed apply through the map (25 visible rows of 100 per sample).  Four workgroups per image add into `sums`
    # atomically here, so dyc is not reproducible to the bit from launch to launch; it is checked against fp64 arithmetic on the
    # kernel's own `sums`: a few fp32 roundings per element (16 u on the magnitudes that enter) and the bf16 store (2^-8).
    N = 25  # noqa: N806
    inv = torch.full((B, L), -1, dtype=I32)
    for b in range(B):
        inv[b, torch.randperm(L, generator=g)[:N].sort().values] = torch.arange(N, dtype=I32)
    gs = guards.GuardSet(dev)
    dx0 = gs.inp(torch.randn(B * N, C, generator=g), name="dx0")
    y = gs.inp(torch.randn(T, C, generator=g), name="y")
    stats = gs.inp(torch.stack([torch.randn(B, generator=g) * 0.1, 0.5 + torch.rand(B, generator=g)], 1), name="stats")
    gamma = gs.inp(1.0 + 0.2 * torch.randn(C, generator=g), name="gamma")
    invd = gs.inp(inv, fill=-1, name="inv")
    dyc = gs.out((T, C), BF16, name="dyc")
    dgamma, dbeta = gs.out((C,), F32, init=0.0, name="dgamma"), gs.out((C,), F32, init=0.0, name="dbeta")
    sums = gs.out((B, 2), F32, name="sums")
    rows = hip.embed_bwd_cs_rows(T)
    cs = gs.out((rows, C), F32, name="cs_partial")
    hip.embed_finish_bwd_ends(dx0, invd, N, y, stats, gamma, dyc, dgamma, dbeta, sums, cs, B, 1, L, C, 0, L)
    gs.check()
    assert rows == 7
    _assert_colsum("embed apply 200 x 768", _reduce(dev, cs, rows, C), dyc, T)
    flat = inv.reshape(-1).to(dev)
    dd = torch.zeros(T, C, dtype=torch.float64, device=dev)
    vis = flat >= 0
    sample = torch.arange(T, device=dev) // L
    dd[vis] = dx0.double()[(sample[vis] * N + flat[vis]).long()]
    mu, rs = stats.double()[sample, 0:1], stats.double()[sample, 1:2]
    c1, c2 = sums.double()[sample, 0:1] / (L * C), sums.double()[sample, 1:2] / (L * C)
    z, dz = (y.double() - mu) * rs, dd * gamma.double()
    ref = rs * (dz - c1 - z * c2)
    bound = 16 * U * rs * (dz.abs() + c1.abs() + (z * c2).abs())
    bound = bound + 2.0 ** -8 * (ref.abs() + bound) + 1e-40
    err = (dyc.double() - ref).abs()
    print(f"embed apply 200 x 768: dyc max err / bound {(err / bound).max().item():.3f}")
    assert bool((err <= bound).all()), (err / bound).max().item()
    # the parameter sums over the visible rows only: n-term bounds (50 visible rows)
    zv = z[vis]
    for name, got, terms in (("dgamma", dgamma, dd[vis] * zv), ("dbeta", dbeta, dd[vis])):
        e = (got.double() - terms.sum(0)).abs()
        bnd = 2 * (terms.shape[0] + 8) * U * terms.abs().sum(0) + 1e-45
        assert bool((e <= bnd).all()), (name, (e / bnd).max().item())


# ================================================================================================ 3. ends as grouped problems
def _int_bf16(shape, g):
    return torch.randint(-3, 4, shape, generator=g).to(BF16)


def test_ends_weight_gradients_as_grouped_problems():
    """dW[M, N] = A[K, M]^T B[K, N] with K no multiple of the kernel's 32-row K step: the K tail reads as zero through the buffer
    descriptor -- the rows behind K are NaN poison here.  Integer-valued bf16 operands (|sum| <= 9 * 70: exact in fp32), so the
    comparison with torch on the same data is exact.  All three problems in ONE table."""
    from maestro_amd import hip
    dev = _dev()
    g = torch.Generator().manual_seed(44)
    gs = guards.GuardSet(dev)
    probs, want = [], []
    for (M, N, K) in ((16, 512, 10), (1024, 512, 70), (768, 1024, 33)):  # noqa: N806
        a, b = _int_bf16((K, M), g), _int_bf16((K, N), g)
        A, Bm = gs.inp(a, name=f"A {M}x{N}x{K}"), gs.inp(b, name=f"B {M}x{N}x{K}")  # noqa: N806
        C = gs.out((M, N), F32, name=f"C {M}x{N}x{K}")  # noqa: N806
        probs.append((A, Bm, C, M, N, K, M, N, N))
        want.append(a.double().t() @ b.double())
    for i, p in enumerate(probs):
        hip.GroupedTN.check(i, p)
    hip.GroupedTN(probs, dev).launch()
    gs.check()
    for p, w in zip(probs, want):
        assert torch.equal(p[2].double().cpu(), w), p[3:6]


def test_a_40_column_band_group_is_exact_on_either_launch():
    """The 40-column band-group of the pixelify head, (M, N) = (40, 512).  The ends keep their split-K launch (fp32 atomics into
    the zeroed slot) for a problem that ``GroupedTN.check`` rejects, and join the grouped launch otherwise.  40 IS a multiple of
    8 -- and the split-K TN launch has the same M, N % 8 rule -- so the check accepts this problem and it joins the grouped launch;
    the rule ``check -> grouped, else split-K`` is followed here as the engine follows it, and BOTH launches must be exact on it
    (integer data), so the problem is right whichever side of the rule it lands on."""
    from maestro_amd import hip
    dev = _dev()
    g = torch.Generator().manual_seed(45)
    M, N, K = 40, 512, 50  # noqa: N806
    a, b = _int_bf16((K, M), g), _int_bf16((K, N), g)
    want = a.double().t() @ b.double()
    gs = guards.GuardSet(dev)
    A, Bm = gs.inp(a, name="A"), gs.inp(b, name="B")  # noqa: N806
    C = gs.out((M, N), F32, init=0.0, name="C (rule)")  # noqa: N806
    C2 = gs.out((M, N), F32, init=0.0, name="C (split-K)")  # noqa: N806
    prob = (A, Bm, C, M, N, K, M, N, N)
    try:
        hip.GroupedTN.check(0, prob)
        grouped = True
    except hip.HipExtensionError:
        grouped = False
    assert grouped == (M % 8 == 0 and N % 8 == 0)
    if grouped:
        hip.GroupedTN([prob], dev).launch()
    else:
        hip.gemm(hip.GEMM_TN, M, N, K, A, M, Bm, N, C, N, hip.OUT_F32 | hip.ATOMIC)
    hip.gemm(hip.GEMM_TN, M, N, K, A, M, Bm, N, C2, N, hip.OUT_F32 | hip.ATOMIC)
    gs.check()
    assert torch.equal(C.double().cpu(), want) and torch.equal(C2.double().cpu(), want)
    with pytest.raises(hip.HipExtensionError):      # what the check does reject: a row count that is no multiple of 8
        hip.GroupedTN.check(0, (A, Bm, C, 36, N, K, M, N, N))


# ================================================================================================ 4. patch embed through the map
def test_patch_embed_backward_through_the_position_map():
    """Beff = 2, group length 12, N = 3 visible, E = 4; two modalities in the group (L = 5 at tok_off 0, L = 7 at tok_off 5).
    Sample 0 sees the first three positions (all in the first modality), sample 1 the last three (all in the second): each
    modality has one sample without a single visible row.  Against the present sequence -- expand_rows, then the two launches
    of the embed-finish backward -- on the same inputs.  The arithmetic per element and its order are kept (a masked row is
    the same zero gradient), so dyc is bit-identical; dgamma / dbeta / sums are the same adds, workgroup by workgroup."""
    from maestro_amd import hip
    dev = _dev()
    B, Lg, N, E = 2, 12, 3, 4  # noqa: N806
    g = torch.Generator().manual_seed(55)
    dx0 = torch.randn(B, N, E, generator=g).to(dev)
    inv = torch.full((B, Lg), -1, dtype=I32)
    inv[0, :3] = torch.arange(3, dtype=I32)
    inv[1, -3:] = torch.arange(3, dtype=I32)
    inv = inv.to(dev)
    dxg = torch.empty(B, Lg, E, dtype=F32, device=dev)
    hip.expand_rows(dx0, inv, dxg, B, Lg, N, E)
    for (L, tok_off) in ((5, 0), (7, 5)):  # noqa: N806
        y = torch.randn(B * L, E, generator=g)
        stats = torch.stack([torch.randn(B, generator=g) * 0.1, 0.5 + torch.rand(B, generator=g)], 1)
        gamma = 1.0 + 0.2 * torch.randn(E, generator=g)
        outs = []
        for mapped in (False, True):
            gs = guards.GuardSet(dev)
            yv, sv, gv = gs.inp(y, name="y"), gs.inp(stats, name="stats"), gs.inp(gamma, name="gamma")
            dyc = gs.out((B * L, E), BF16, name="dyc")
            dgamma, dbeta = gs.out((E,), F32, init=0.0, name="dgamma"), gs.out((E,), F32, init=0.0, name="dbeta")
            sums = gs.out((B, 2), F32, name="sums")
            rows = hip.embed_bwd_cs_rows(B * L)
            cs = gs.out((rows, E), F32, name="cs_partial")
            if mapped:
                hip.embed_finish_bwd_ends(dx0, inv, N, yv, sv, gv, dyc, dgamma, dbeta, sums, cs, B, 1, L, E, tok_off, Lg)
            else:
                hip.embed_finish_bwd(dxg, yv, sv, gv, dyc, dgamma, dbeta, sums, B, 1, L, E, tok_off, Lg)
            gs.check()
            outs.append((dyc.clone(), dgamma.clone(), dbeta.clone(), sums.clone(), cs))
        assert guards.bits_equal(outs[0][0], outs[1][0]), f"dyc differs (L = {L}, tok_off = {tok_off})"
        for k, name in ((1, "dgamma"), (2, "dbeta"), (3, "sums")):
            # one workgroup per image: identical adds (a skipped masked row adds nothing; the dense form adds +-0)
            assert torch.equal(outs[0][k], outs[1][k]), name
        assert float(outs[1][1].abs().max()) > 0
        _assert_colsum(f"embed through the map (L = {L})", _reduce(dev, outs[1][4], rows, E), outs[1][0], B * L)


# ================================================================================================ 5. engine level
def _ends_parameters(eng):
    m, out = eng.model, {}
    for s in eng.mods.values():
        conv = m.embed_to_rec[s.embed].pixelify_bands[s.gi].conv
        out[f"pixelify.{s.name}.weight"], out[f"pixelify.{s.name}.bias"] = conv.weight, conv.bias
        pe = eng.mb[s.name]["pe"]
        out[f"patch_embed.{s.name}.conv.weight"], out[f"patch_embed.{s.name}.conv.bias"] = pe.conv.weight, pe.conv.bias
    for st in eng._all_stacks():
        out[f"{st.tag}.norm.weight"], out[f"{st.tag}.norm.bias"] = st.t.norm.weight, st.t.norm.bias
        if st.depth:
            out[f"{st.tag}.last_fc2.bias"] = st.t.layers[-1][1].net[4].bias
    if not eng.e2d_identity:
        for g in eng.groups:
            lin = m.enc_to_dec[g.model]
            out[f"enc_to_dec.{g.model}.weight"], out[f"enc_to_dec.{g.model}.bias"] = lin.weight, lin.bias
    return out


def _poison_partials(eng) -> int:
    """NaN into every partial-row buffer of the ends: a launch that a later step (a graph replay) leaves out, or a job that reads
    a row nobody wrote, then shows up as NaN in a gradient instead of repeating the previous step's value."""
    bufs = [b.get(k) for b in eng.mb.values() for k in ("drec_cs", "dyc_cs")] + [gb.get("e2d_cs") for gb in eng.gb.values()]
    bufs = [t for t in bufs + list(eng.sites.buffers()) if t is not None]
    for t in bufs:
        t.fill_(float("nan"))
    return len(bufs)


def _det_reference(model, B, dev, batch, noise, struct):  # noqa: N803
    det = model.engine(B, dev, loss="l2_norm", deterministic=True)
    det.forward(batch, noise=noise, struct=struct)
    det.zero_grad()
    det.backward()
    torch.cuda.synchronize()
    return {k: det.store.g(p).double().clone() for k, p in _ends_parameters(det).items()}


def _assert_ends_match(tag, eng, want):
    """Every ends parameter at the bound for reordered fp32 sums (1e-5 relative L2 PER PARAMETER), the ends together at the same
    bound, and 1e-2 per parameter as the separate gross-error statement of tests/test_det_engine_gpu.py."""
    got = {k: eng.store.g(p).double() for k, p in _ends_parameters(eng).items()}
    assert set(got) == set(want) and len(got) >= 9
    num = sum(float((got[k] - want[k]).pow(2).sum()) for k in got) ** 0.5
    den = sum(float(want[k].pow(2).sum()) for k in got) ** 0.5
    rel = {k: float((got[k] - want[k]).norm()) / max(float(want[k].norm()), 1e-30) for k in got}
    worst = max(rel, key=lambda k: rel[k] if rel[k] == rel[k] else float("inf"))
    print(f"{tag}: ends gradients rel L2 {num / den:.3e}; worst parameter {worst} {rel[worst]:.3e}")
    assert den > 0 and num <= 1e-5 * den, (tag, num / den)
    for k in got:
        assert float(want[k].norm()) > 0, k
        assert rel[k] <= 1e-5, (tag, k, rel[k])
        assert rel[k] <= 1e-2, (tag, k, rel[k])


@pytest.mark.parametrize("name", ["c3_aerial_s2", "c3p_dem_s1", "bg_aerial_s2"])
def test_ends_gradients_match_deterministic_mode(golden_dir, name):
    """Tiny golden configurations (a joint encoder; two modalities in one group; band-groups), deferred weight gradients: the
    default-mode gradient of every ends parameter against ``deterministic=True`` -- an independent launch list without atomics --
    on the same weights, inputs and draws, on three consecutive steps (eager run, capture + replay, replay).  Between the steps
    every partial-row buffer of the ends is filled with NaN, so a replay that does not rewrite one cannot pass on stale values.

    The two modes differ by the ORDER of fp32 sums, so every ends parameter is held to the repository's bound for reordered sums
    (1e-5 relative L2: tests/test_det_engine_gpu.py, ``test_gradients_agree_with_default_mode``), one parameter at a time: a
    partial row lost out of 128, or sums taken of unrounded values, moves a bias gradient by 1e-3 ... 1e-2."""
    from tests import test_mae_gpu as T  # noqa: N812
    dev = _dev()
    _, case, _, _, _, model, batch, noise, struct = T._setup(name, golden_dir)
    batch, B = {k: v.to(dev) for k, v in batch.items()}, case["B"]  # noqa: N806
    want = _det_reference(model, B, dev, batch, noise, struct)
    eng = model.engine(B, dev, loss="l2_norm", deterministic=False)
    eng.wgrad_mode = "deferred"
    assert not eng.deterministic and eng._ends_on()
    for step in range(3):
        eng.forward(batch, noise=noise, struct=struct)
        eng.zero_grad()
        eng.backward()
        torch.cuda.synchronize()
        assert eng._plan == "all" and eng._loss_cs
        _assert_ends_match(f"{name} step {step}", eng, want)
        assert _poison_partials(eng) >= 3 * len(eng.mods) + len(eng.groups)     # drec_cs, dyc_cs, decoder LN per modality; encoder LN per group
    assert any(n.startswith("bwd_") for n in eng._graphs), "the backward segments were not captured: no replay was exercised"
    assert not any(eng.gb[g.name].get("dxg") is not None for g in eng.groups), "the expanded group-sequence gradient is back"


def test_a_rejected_ends_problem_keeps_its_split_k_launch_and_its_cleared_buffer(golden_dir, monkeypatch):
    """The fallback branch of part A, which no shipped shape takes: ``GroupedTN.check`` is made to reject the pixelify and the
    patch-embed conv weight gradient of ONE modality.  Those two keep their split-K launches (they are not in the grouped table),
    the rejected ``dw_conv`` stays in the ``zero_grad`` span list while the other modality's leaves it, and every ends gradient
    still matches deterministic mode -- on three steps, i.e. through capture and replay."""
    from maestro_amd import hip
    from tests import test_mae_gpu as T  # noqa: N812
    dev = _dev()
    _, case, _, _, _, model, batch, noise, struct = T._setup("c3_aerial_s2", golden_dir)
    batch, B = {k: v.to(dev) for k, v in batch.items()}, case["B"]  # noqa: N806
    want = _det_reference(model, B, dev, batch, noise, struct)
    eng = model.engine(B, dev, loss="l2_norm", deterministic=False)
    eng.wgrad_mode = "deferred"
    names = list(eng.mods)
    assert len(names) >= 2
    s0 = eng.mods[names[0]]
    rejected = {eng.mb[names[0]]["dw_conv"].data_ptr(), eng._rec_wgrad(s0)[2].data_ptr()}
    real = hip.GroupedTN.check

    def check(i, prob):
        if prob[2].data_ptr() in rejected:
            raise hip.HipExtensionError("rejected by the test")
        return real(i, prob)
    monkeypatch.setattr(hip.GroupedTN, "check", staticmethod(check))
    for step in range(3):
        eng.forward(batch, noise=noise, struct=struct)
        eng.zero_grad()
        eng.backward()
        torch.cuda.synchronize()
        _assert_ends_match(f"rejected problems, step {step}", eng, want)
        _poison_partials(eng)
    assert eng._plan == "all"
    assert not eng._ends_deferred(eng.embed[names[0]].wgrad_problem()) and eng._ends_deferred(eng.embed[names[1]].wgrad_problem())
    base = eng.store.grad.data_ptr()
    spans = eng._zero_lists["all"][0].view(-1, 2).cpu().tolist()
    offs = {o for o, _ in spans}
    assert (eng.mb[names[0]]["dw_conv"].data_ptr() - base) // 4 in offs, "a buffer the split-K atomics add into must be cleared"
    assert (eng.mb[names[1]]["dw_conv"].data_ptr() - base) // 4 not in offs, "a buffer the grouped launch stores needs no clearing"
    (table,) = eng._wgrad_tables.values()
    n_ends = 2 * len(names) + (0 if eng.e2d_identity else len(eng.groups))
    assert table[0].n == sum(len(st.wgrad_problems()) for st in eng._all_stacks()) + n_ends - 2
    assert len(table[2]) == len(names) - 1          # one unpack_rows_add behind the grouped launch: the other modality's


@pytest.mark.parametrize("mode", ["fused", "plan_changes_before_backward"])
def test_the_fused_plan_keeps_its_loss_launch(golden_dir, mode):
    """Under the "fused" plan the forward runs the plain loss launch: the partial rows of the pixelify bias gradient are not
    written (they keep their poison) and the backward takes its column sums as before.  ``plan_changes_before_backward``: the plan
    becomes a deferred one between that forward and its backward -- the backward must not sum partial rows nobody wrote."""
    from tests import test_mae_gpu as T  # noqa: N812
    dev = _dev()
    _, case, _, _, _, model, batch, noise, struct = T._setup("c3_aerial_s2", golden_dir)
    batch, B = {k: v.to(dev) for k, v in batch.items()}, case["B"]  # noqa: N806
    want = _det_reference(model, B, dev, batch, noise, struct)
    eng = model.engine(B, dev, loss="l2_norm", deterministic=False)
    eng.wgrad_mode = "fused"
    for step in range(3):
        _poison_partials(eng)
        eng.wgrad_mode = "fused"
        eng.forward(batch, noise=noise, struct=struct)
        assert not eng._loss_cs
        if mode != "fused":
            eng.wgrad_mode = "deferred"
        eng.zero_grad()
        eng.backward()
        torch.cuda.synchronize()
        assert eng._plan == ("fused" if mode == "fused" else "all")
        for b in eng.mb.values():
            assert b.get("drec_cs") is not None and bool(torch.isnan(b["drec_cs"]).all()), "the loss launch wrote partial rows"
        _assert_ends_match(f"{mode}, step {step}", eng, want)
