"""fp8 path (BASELINE configs[4]): quantisers against torch's OCP float8 casts on random data, the scaled-MFMA GEMM on exact
integer data (operand lane map, K order, tiling: bit-exact vs an fp32 matmul), its epilogues against the bf16 kernel fed with
the SAME (already quantised) values -- fp32 sums and bf16 outputs to a tolerance --, the engine against the oracle, guard bands.
The fp8 BYTES every site writes (both quantisers, the LayerNorm's and the GEMM's output copies in e4m3, e5m2 and MX, the AdamW
shadow) and the scale-update rule are held to bit equality on code values, ties and saturation edges in
tests/test_fp8_codes_gpu.py; the +-1-code comparisons below only keep the copies next to a bf16-rounded reference."""

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _q(x, fmt):
    return x.to(torch.float8_e4m3fn if fmt == 0 else torch.float8_e5m2)


@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_quantiser_matches_torch_float8(dev, fmt, dtype):
    from maestro_amd import hip
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(257, 64, generator=g) * torch.exp(3 * torch.randn(257, 1, generator=g))).to(dtype)   # wide dynamic range
    x[0, :8] = torch.tensor([0.0, -0.0, 1e-9, 447.0, 449.0, -1e6, 0.0019, 0.06], dtype=dtype)
    sc = hip.Fp8Scales(2, dev)
    sc.scale[1] = 0.25
    src = x.to(dev)
    dst, dst_t = torch.zeros(x.shape, dtype=torch.uint8, device=dev), torch.zeros(64, 257, dtype=torch.uint8, device=dev)
    qb = hip.QuantBatch([dict(src=src, dst=dst, dst_t=dst_t, slot=1, format=fmt)], sc, dev)
    qb.launch(2)
    torch.cuda.synchronize()
    lim = hip.FP8_MAX[fmt]
    want = _q((x.float() * 0.25).clamp(-lim, lim), fmt).view(torch.uint8)
    assert torch.equal(dst.cpu(), want), "cast differs from torch's OCP float8 conversion (round to nearest even, saturating)"
    assert torch.equal(dst_t.cpu(), want.t().contiguous())
    assert sc.absmax(1) == float(x.float().abs().max()) and sc.absmax(0) == 0.0      # maximum over the slot's sub-slot row
    sc.update(fmt=fmt, margin=1)
    amax = float(x.float().abs().max())
    import math
    assert float(sc.scale[1]) == 2.0 ** (math.floor(math.log2(lim / amax)) - 1) and sc.absmax(1) == 0.0
    assert float(sc.scale[0]) == 1.0 and float(sc.descale[1]) == 1.0 / float(sc.scale[1])


@pytest.mark.parametrize("tile", ["128", "128d", "256"])
@pytest.mark.parametrize("M,N,K", [(256, 256, 128), (300, 520, 384), (1000, 136, 256), (64, 768, 768), (130, 264, 1152),
                                   (64, 256, 3072)])      # (the last: fc2's depth, 24 K steps; |sums| <= 5 * 4 * 3072 < 2^24)
@pytest.mark.parametrize("a_fmt", [0, 1])
def test_gemm_fp8_integer_exact(dev, M, N, K, a_fmt, tile, monkeypatch):
    """Small integers are exact in e4m3 / e5m2 and every partial sum is exact in fp32: any mistake in the operand lane map,
    the swizzles, the K order or the tiling changes bits."""
    from maestro_amd import hip
    monkeypatch.setenv("MH_FP8_TILE", tile)      # every tile / ring form (the library picks by problem size otherwise)
    g = torch.Generator().manual_seed(M + N + K)
    a = torch.randint(-4, 5, (M, K), generator=g).float()
    b = torch.randint(-4, 5, (N, K), generator=g).float()
    # asymmetric content so that a transposed / permuted fragment cannot hide
    a[:, ::7] += 1.0
    A8, B8 = _q(a, a_fmt).view(torch.uint8).to(dev), _q(b, 0).view(torch.uint8).to(dev)  # noqa: N806
    C = torch.full((M, N), float("nan"), device=dev)  # noqa: N806
    da, db = torch.tensor([0.5], device=dev), torch.tensor([4.0], device=dev)
    hip.gemm_fp8(M, N, K, A8, K, B8, K, C, N, da, db, flags=hip.OUT_F32, a_format=a_fmt)
    torch.cuda.synchronize()
    assert torch.equal(C.cpu(), 2.0 * (a @ b.t()))


def test_gemm_fp8_epilogues_match_bf16_kernel(dev):
    """With operands that are exactly representable in fp8 the fp8 GEMM and the bf16 GEMM see the same numbers; every
    product (<= 8 significant bits) and the fp32 accumulation order per K block differ only in grouping, so outputs agree to
    fp32 rounding; the fused epilogues (bias + GELU + saved GELU', fp32 residual, fp8 copy of the output) must follow."""
    from maestro_amd import hip
    g = torch.Generator().manual_seed(11)
    M, N, K = 640, 1024, 256  # noqa: N806
    a = _q(torch.randn(M, K, generator=g), 0).float()
    b = _q(torch.randn(N, K, generator=g) * 0.1, 0).float()
    A8, B8 = _q(a, 0).view(torch.uint8).to(dev), _q(b, 0).view(torch.uint8).to(dev)  # noqa: N806
    A16, B16 = a.bfloat16().to(dev), b.bfloat16().to(dev)  # noqa: N806
    one = torch.ones(1, device=dev)
    bias, res = torch.randn(N, generator=g).to(dev), torch.randn(M, N, generator=g).to(dev)
    # fc1-style: bias + GELU, saves GELU', bf16 out + fp8 copy
    C8, C16 = (torch.empty(M, N, dtype=torch.bfloat16, device=dev) for _ in range(2))  # noqa: N806
    X8, X16 = (torch.empty(M, N, dtype=torch.bfloat16, device=dev) for _ in range(2))  # noqa: N806
    c8, s8, amax = torch.zeros(M, N, dtype=torch.uint8, device=dev), torch.tensor([8.0], device=dev), torch.zeros(hip.AMAX_PITCH, device=dev)
    fl = hip.BIAS | hip.GELU | hip.AUX_DGELU
    hip.gemm_fp8(M, N, K, A8, K, B8, K, C8, N, one, one, flags=fl, bias=bias, aux_out=X8, ldaux=N, c8=c8, ldc8=N, c8_scale=s8, c8_amax=amax)
    hip.gemm(hip.GEMM_NT, M, N, K, A16, K, B16, K, C16, N, fl, bias=bias, aux_out=X16, ldaux=N)
    torch.cuda.synchronize()
    assert (C8.float() - C16.float()).abs().max() <= 2e-2 * C16.float().abs().max() and (X8.float() - X16.float()).abs().max() < 2e-2
    assert (C8.float() - C16.float()).abs().mean() < 1e-4          # identical but for a few bf16 rounding flips
    # the e4m3 copy is cast from the fp32 epilogue value, C8 from the same value rounded to bf16 first: re-quantising C8 lands
    # on the same code except where the bf16 rounding crossed an e4m3 boundary (neighbouring code, a few per cent at most)
    want8 = _q((C8.float() * 8.0).clamp(-448, 448), 0).view(torch.uint8).cpu().int()
    diff = (c8.cpu().int() - want8).abs()
    assert int(diff.max()) <= 1 and float((diff != 0).float().mean()) < 0.05, (int(diff.max()), float((diff != 0).float().mean()))
    assert abs(float(amax.max()) - float(C8.float().abs().max())) <= 2 ** -7 * float(amax.max())
    # proj / fc2-style: fp32 out + bias + residual
    D8, D16 = torch.empty(M, N, device=dev), torch.empty(M, N, device=dev)  # noqa: N806
    fl = hip.OUT_F32 | hip.BIAS | hip.RESIDUAL
    hip.gemm_fp8(M, N, K, A8, K, B8, K, D8, N, one, one, flags=fl, bias=bias, res=res, ldr=N)
    hip.gemm(hip.GEMM_NT, M, N, K, A16, K, B16, K, D16, N, fl, bias=bias, res=res, ldr=N)
    torch.cuda.synchronize()
    assert (D8 - D16).abs().max() < 1e-3      # fp32 sums of exact products, grouped by 128 instead of 32 along K


COMMON = dict(interpolate="nearest", model="mae", num_levels=1, type_head="attentive", fac_abs_enc=1.0, fac_date_enc=1.0)
# fp8 forward (e4m3, 3 mantissa bits) against the fp32 oracle: observed on MI355X (round 2) loss 4.2e-4, pixels_rec 5.6e-2,
# worst parameter gradient 8.6e-2 (relative L2) -- tolerances <= 2x; the bf16 engine sits at 3.5e-4 / 7e-3 / 1.5e-2
FP8_LOSS_TOL, FP8_PIX_TOL, FP8_GRAD_TOL = 8.4e-4, 1.12e-1, 1.72e-1
FP8_DGRAD_TOL = 0.208    # opt-in e5m2 data-gradient GEMMs (2 mantissa bits): observed worst 0.104


@pytest.mark.parametrize("dgrad", ["0", "1"])
def test_engine_fp8_forward_matches_oracle(dev, observed, monkeypatch, dgrad):
    """The whole step with e4m3 forward GEMMs (maestro_amd/fp8.py) against the fp32 oracle, same weights / inputs / draws:
    masks bit-exact, loss, reconstructions and every parameter gradient within the stated fp8 tolerances; a second forward
    (scales now derived from the first step's absmax) stays as close; one AdamW step refreshes the e4m3 weight shadows.
    ``dgrad`` 1: the opt-in e5m2 data-gradient GEMMs (``MAESTRO_FP8_DGRAD``), checked on the second backward."""
    monkeypatch.setenv("MAESTRO_FP8_DGRAD", dgrad)
    import maestro_amd.conf as conf
    from maestro_amd.ssl import mae as pmae
    from maestro_amd.train.optim import FusedAdamW
    from oracle import mae as om
    from oracle.gen_golden import build_datasets, case_table, init_weights, make_batch
    case = dict(case_table()["c3_aerial_s2"])
    ds = build_datasets(case, conf)
    kw = dict(fusion_mode="group", inter_depth=1, depth=3, **COMMON)
    oracle = om.build_oracle(ds, conf.MaskConfig(), model_size="small", **kw)       # E = 384 = 3 x 128: fp8-eligible widths
    init_weights(oracle, 77)
    model = pmae.mae_small(datasets=ds, mask=conf.MaskConfig(), **kw)
    model.load_state_dict(oracle.state_dict(), strict=True)
    B = 4  # noqa: N806
    batch = make_batch(ds.dataset, B, 5)
    eng = model.engine(B, dev, loss="l2_norm", dtype="fp8")
    assert eng.fp8 is not None and all(st.f8 is not None for st in eng._all_stacks())
    torch.manual_seed(3)
    noise, struct = eng.draw_masks()
    dbatch = {k: v.to(dev) for k, v in batch.items()}
    loss = eng.forward(dbatch, noise=noise, struct=struct).clone()     # (the engine's loss buffer is static: keep the value)
    eng.zero_grad()
    eng.backward()
    torch.cuda.synchronize()
    pixels, masks = eng.reconstructions()
    ob, orec, omsk, _ = oracle({k: v.clone() for k, v in batch.items()}, "pretrain", noise=noise,
                               struct_masks={g: s[:, :, None] for g, s in struct.items()})
    oloss = om.compute_loss_rec(ob, orec, omsk, oracle.out_grid_size, om.norm_bands_of(ds.dataset), "l2_norm")
    oracle.zero_grad()
    oloss.backward()
    rel = lambda a, b: ((a - b).double().norm() / b.double().norm().clamp(min=1e-12)).item()  # noqa: E731
    for m in orec:
        assert torch.equal(masks[m].cpu(), omsk[m])
        e = rel(pixels[m].cpu(), orec[m].detach())
        observed("fp8/small", f"pixels/{m}", e)
        assert e < FP8_PIX_TOL, (m, e)
    e = abs(loss.item() - oloss.item()) / abs(oloss.item())
    observed("fp8/small", "loss", e)
    assert e < FP8_LOSS_TOL, (loss.item(), oloss.item())
    ograds = {k: p.grad for k, p in oracle.named_parameters() if p.grad is not None}
    gmax = max(g.abs().max().item() for g in ograds.values())

    def check_grads(tag, tol):
        worst = (0.0, None)
        for k, p in model.named_parameters():
            if k in ograds:
                got, want = eng.store.g(p).cpu(), ograds[k]
                err, ref = (got - want).double().norm().item(), want.double().norm().item()
                floor = 1e-4 * gmax * want.numel() ** 0.5
                if ref > 10 * floor and err / ref > worst[0]:
                    worst = (err / ref, k)
                assert err <= tol * ref + floor, (tag, k, err / max(ref, 1e-12))
        observed("fp8/small", f"{tag}/{worst[1]}", worst[0])

    assert eng.fp8.dgrad == (dgrad == "1") and (not eng.fp8.dgrad or all(f["dgrad"] for st in eng._all_stacks() for f in st.f8))
    check_grads("grad_worst", FP8_GRAD_TOL)          # (first backward: bf16 dgrads, the e5m2 gradient scales are being calibrated)
    # second forward: activation scales are now derived from the first step's absmax (delayed scaling)
    assert float(eng.fp8.asc.scale.max()) > 1.0 or float(eng.fp8.asc.scale.min()) < 1.0
    loss2 = eng.forward(dbatch, noise=noise, struct=struct).clone()
    e2 = abs(loss2.item() - oloss.item()) / abs(oloss.item())
    observed("fp8/small", "loss_step2", e2)
    assert e2 < FP8_LOSS_TOL
    # an optimizer step rebuilds the e4m3 weight shadows from the updated masters: the next forward must follow the oracle
    # evaluated at the UPDATED weights (a stale shadow or scale would leave it at the old loss)
    w8_before = eng.enc["aerial"].f8[0]["w_qkv"].clone()
    eng.zero_grad()
    eng.backward()
    if eng.fp8.dgrad:
        # second backward, same weights and draws: the four dgrads of every layer now run e5m2 gradients x transposed e4m3
        # weights with the scales calibrated by the first one
        assert eng.fp8.grad_ready and float(eng.fp8.gsc.scale.min()) > 1.0
        f0 = eng.enc["aerial"].f8[0]
        assert torch.equal(f0["wt_fc1"], f0["w_fc1"].t().contiguous()) and torch.equal(f0["wt_qkv"], f0["w_qkv"].t().contiguous())
        check_grads("grad_worst_fp8_dgrad", FP8_DGRAD_TOL)
    FusedAdamW(eng, 1e-3).step()
    loss3 = eng.forward(dbatch, noise=noise, struct=struct).clone()
    torch.cuda.synchronize()
    assert not torch.equal(w8_before, eng.enc["aerial"].f8[0]["w_qkv"])
    oracle.load_state_dict({k: v.detach().cpu() for k, v in model.state_dict().items()}, strict=True)
    ob, orec, omsk, _ = oracle({k: v.clone() for k, v in batch.items()}, "pretrain", noise=noise,
                               struct_masks={g: s[:, :, None] for g, s in struct.items()})
    oloss3 = om.compute_loss_rec(ob, orec, omsk, oracle.out_grid_size, om.norm_bands_of(ds.dataset), "l2_norm")
    assert abs(oloss3.item() - oloss.item()) > 10 * FP8_LOSS_TOL * abs(oloss.item())     # the update moved the loss visibly
    e3 = abs(loss3.item() - oloss3.item()) / abs(oloss3.item())
    observed("fp8/small", "loss_after_update", e3)
    assert e3 < 1.2e-2, (loss3.item(), oloss3.item())     # observed 4.0e-3 (the first Adam step leaves the net at loss 6.5)


@pytest.mark.parametrize("M,dim", [(333, 768), (64, 256), (130, 512), (257, 1024), (100, 384), (50, 192), (7, 2048)])
def test_layernorm_fp8_output(dev, M, dim):  # noqa: N803
    """``mh_layernorm_fwd_fp8``: the bf16 output is the plain kernel's BIT FOR BIT (both entry points run the same kernel: the
    straight-line one at dim = 256 k <= 1024, the generic one elsewhere), the e4m3 copy is the cast of the fp32 value times the
    scale (checked against torch's conversion of an fp32 LayerNorm: equal codes but for roundings of values that sit on a code
    boundary within fp32 noise), absmax recorded."""
    from maestro_amd import hip
    g = torch.Generator().manual_seed(2)
    x = (torch.randn(M, dim, generator=g) * 3 + 0.5).to(dev)
    gamma, beta = (1 + 0.2 * torch.randn(dim, generator=g)).to(dev), (0.1 * torch.randn(dim, generator=g)).to(dev)
    y, y2 = torch.empty(M, dim, dtype=torch.bfloat16, device=dev), torch.empty(M, dim, dtype=torch.bfloat16, device=dev)
    y8 = torch.zeros(M, dim, dtype=torch.uint8, device=dev)
    mean, rstd, scale, amax = (torch.zeros(M, device=dev), torch.zeros(M, device=dev), torch.tensor([16.0], device=dev),
                               torch.zeros(hip.AMAX_PITCH, device=dev))
    hip.layernorm_fwd_fp8(x, M, 0, gamma, beta, y, M, 0, mean, rstd, 1, M, dim, y8, scale, amax)
    hip.layernorm_fwd(x, M, 0, gamma, beta, y2, M, 0, mean, rstd, 1, M, dim)
    torch.cuda.synchronize()
    assert torch.equal(y.view(torch.int16), y2.view(torch.int16))
    ref = torch.nn.functional.layer_norm(x.cpu().double(), (dim,), gamma.cpu().double(), beta.cpu().double()).float()
    want = _q((ref * 16.0).clamp(-448, 448), 0).view(torch.uint8).int()
    diff = (y8.cpu().int() - want).abs()
    assert int(diff.max()) <= 1 and float((diff != 0).float().mean()) < 2e-3
    assert abs(float(amax.max()) - float(ref.abs().max())) < 1e-4 * float(ref.abs().max())


def test_non_finite_values_poison_the_scale(dev):
    """A NaN / inf in a tensor must not vanish in the fp8 bookkeeping (the saturating cast turns it into +-448 and ``fmaxf`` would
    drop it from the absmax): every absmax fold keeps it (integer order on |x| bits, NaN on top), ``mh_fp8_update_scales`` turns
    it into a NaN scale / descale, and the next GEMM's descale makes the loss NaN -- as the bf16 path would show it.  Covers the
    batched quantiser, the LayerNorm's e4m3 output (straight-line and generic kernel) and the fused AdamW's shadow refresh."""
    import math
    from maestro_amd import hip
    g = torch.Generator().manual_seed(4)
    for bad in (float("nan"), float("inf"), -float("inf")):
        # batched quantiser, absmax-only and cast + absmax
        x = torch.randn(130, 64, generator=g)
        x[77, 13] = bad
        for mode in (0, 2):
            sc = hip.Fp8Scales(2, dev)
            dst = torch.zeros(x.shape, dtype=torch.uint8, device=dev)
            hip.QuantBatch([dict(src=x.to(dev), dst=dst, slot=1, format=0)], sc, dev).launch(mode)
            torch.cuda.synchronize()
            a = sc.absmax(1)
            assert (math.isnan(a) if math.isnan(bad) else a == float("inf")) and sc.absmax(0) == 0.0, (bad, mode, a)
            sc.update(fmt=0, margin=1)
            torch.cuda.synchronize()
            assert math.isnan(float(sc.scale[1])) and math.isnan(float(sc.descale[1])), (bad, mode)
            assert float(sc.scale[0]) == 1.0 and sc.absmax(1) == 0.0       # clean slots untouched, the row reset
        # LayerNorm with the e4m3 copy: a non-finite input row gives a NaN output row -> the slot's absmax is NaN
        for M, dim in ((64, 768), (33, 384)):  # noqa: N806
            xx = torch.randn(M, dim, generator=g).to(dev)
            xx[M // 2, 5] = bad
            gamma, beta = torch.ones(dim, device=dev), torch.zeros(dim, device=dev)
            y, y8 = torch.empty(M, dim, dtype=torch.bfloat16, device=dev), torch.zeros(M, dim, dtype=torch.uint8, device=dev)
            mean, rstd = torch.zeros(M, device=dev), torch.zeros(M, device=dev)
            sc = hip.Fp8Scales(1, dev)
            hip.layernorm_fwd_fp8(xx, M, 0, gamma, beta, y, M, 0, mean, rstd, 1, M, dim, y8, sc.scale[0:1], sc.amax[0])
            torch.cuda.synchronize()
            assert math.isnan(sc.absmax(0)), (bad, dim, sc.absmax(0))
            assert bool(torch.isfinite(y.float()[: M // 2]).all())          # the other rows are clean
    # fused AdamW: a NaN gradient makes the updated weight NaN; the weight's slot must report it
    n = 64 * 8
    p, m, v = torch.randn(n, generator=g).to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    grad = torch.randn(n, generator=g)
    grad[200] = float("nan")
    half, p8 = torch.zeros(n, dtype=torch.bfloat16, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev)
    slot_map = torch.zeros(n // 64, dtype=torch.int16)
    slot_map[4:] = 1
    scale, amax = torch.tensor([64.0, 64.0], device=dev), torch.zeros(2, hip.AMAX_PITCH, device=dev)
    hip.adamw_fp8(p, grad.to(dev), m, v, half, p8, slot_map.to(dev), scale, amax, n, 1e-3, 0.9, 0.99, 1e-8, 0.01, 1)
    torch.cuda.synchronize()
    assert bool(torch.isnan(amax[0]).any()) and not bool(torch.isnan(amax[1]).any())


def test_adamw_fp8_refreshes_the_shadows_in_its_own_pass(dev):
    """``mh_adamw_fp8`` = ``mh_adamw`` (bit-identical parameters, moments and bf16 shadow) + the e4m3 shadow of the elements the
    slot map marks, cast with the slot's scale, absmax folded into the slot -- and nothing written where the map says -1."""
    from maestro_amd import hip
    g = torch.Generator().manual_seed(9)
    n = 64 * 40
    p0, grad = torch.randn(n, generator=g) * 0.05, torch.randn(n, generator=g) * 1e-3
    slot_map = torch.full((n // 64,), -1, dtype=torch.int16)
    slot_map[4:20], slot_map[24:40] = 0, 1                    # two "weights", gaps in front, between (biases / norms)
    outs = []
    for fused in (False, True):
        p, m, v = p0.clone().to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
        half = torch.zeros(n, dtype=torch.bfloat16, device=dev)
        p8 = torch.full((n,), 7, dtype=torch.uint8, device=dev)
        scale, amax = torch.tensor([64.0, 128.0], device=dev), torch.zeros(2, hip.AMAX_PITCH, device=dev)
        if fused:
            hip.adamw_fp8(p, grad.to(dev), m, v, half, p8, slot_map.to(dev), scale, amax, n, 1e-3, 0.9, 0.99, 1e-8, 0.01, 1)
        else:
            hip.adamw(p, grad.to(dev), m, v, half, n, 1e-3, 0.9, 0.99, 1e-8, 0.01, 1)
        torch.cuda.synchronize()
        outs.append((p.cpu(), m.cpu(), v.cpu(), half.cpu(), p8.cpu(), amax.cpu()))
    for a, b in zip(outs[0][:4], outs[1][:4]):
        assert torch.equal(a.view(torch.int16) if a.dtype == torch.bfloat16 else a, b.view(torch.int16) if b.dtype == torch.bfloat16 else b)
    p_new, p8, amax = outs[1][0], outs[1][4], outs[1][5]
    for slot, (lo, hi), sc in ((0, (4 * 64, 20 * 64), 64.0), (1, (24 * 64, 40 * 64), 128.0)):
        want = _q((p_new[lo:hi] * sc).clamp(-448, 448), 0).view(torch.uint8)
        assert torch.equal(p8[lo:hi], want) and float(amax[slot].max()) == float(p_new[lo:hi].abs().max())
    assert bool((p8[: 4 * 64] == 7).all()) and bool((p8[20 * 64: 24 * 64] == 7).all())


def test_transpose_u8_batched(dev):
    """``mh_transpose_u8_batched`` (transposed e4m3 weight shadows for the fp8 dgrad): byte-exact for several shapes in one launch."""
    from maestro_amd import hip
    g = torch.Generator().manual_seed(4)
    shapes = [(64, 64), (768, 3072), (2304, 768), (512, 128)]
    srcs = [torch.randint(0, 256, s, generator=g, dtype=torch.uint8).to(dev) for s in shapes]
    dsts = [torch.zeros(s[1], s[0], dtype=torch.uint8, device=dev) for s in shapes]
    hip.TransposeBatch(list(zip(srcs, dsts)), dev).launch()
    torch.cuda.synchronize()
    for s, d in zip(srcs, dsts):
        assert torch.equal(d.cpu(), s.cpu().t().contiguous())
    with pytest.raises(hip.HipExtensionError):
        hip.TransposeBatch([(torch.zeros(65, 64, dtype=torch.uint8, device=dev), torch.zeros(64, 65, dtype=torch.uint8, device=dev))], dev)


def test_gemm_fp8_dgrad_epilogue(dev):
    """The dgrad form of ``mh_gemm_fp8``: e5m2 A operand x e4m3 B, ``MULAUX | COLSUM`` epilogue and an e5m2 copy of the output
    (``MH_GEMM_C8_E5M2``) -- against the bf16 kernel on the same (fp8-representable) operands."""
    from maestro_amd import hip
    g = torch.Generator().manual_seed(6)
    for (M, N, K) in ((320, 768, 384), (1000, 1536, 512)):   # noqa: N806
        a = (torch.randn(M, K, generator=g) * 0.5).to(torch.float8_e5m2)
        b = (torch.randn(N, K, generator=g) * 0.5).to(torch.float8_e4m3fn)
        aux = (torch.rand(M, N, generator=g) * 1.2 - 0.1).to(torch.bfloat16).to(dev)
        A8, B8 = a.view(torch.uint8).to(dev), b.view(torch.uint8).to(dev)   # noqa: N806
        A16, B16 = a.float().to(torch.bfloat16).to(dev), b.float().to(torch.bfloat16).to(dev)   # noqa: N806 -- exact in bf16
        rows = (M + 63) // 64
        C8, C16 = (torch.empty(M, N, dtype=torch.bfloat16, device=dev) for _ in range(2))  # noqa: N806
        cs8, cs16 = torch.zeros(rows, N, device=dev), torch.zeros(rows, N, device=dev)
        c8, s8, amax = torch.zeros(M, N, dtype=torch.uint8, device=dev), torch.tensor([64.0], device=dev), torch.zeros(hip.AMAX_PITCH, device=dev)
        one = torch.ones(1, device=dev)
        fl = hip.MULAUX | hip.COLSUM
        hip.gemm_fp8(M, N, K, A8, K, B8, K, C8, N, one, one, flags=fl | hip.C8_E5M2, a_format=hip.FP8_E5M2, aux_in=aux, ldaux=N,
                     colsum=cs8, c8=c8, ldc8=N, c8_scale=s8, c8_amax=amax)
        hip.gemm(hip.GEMM_NT, M, N, K, A16, K, B16, K, C16, N, fl, aux_in=aux, ldaux=N, colsum=cs16)
        torch.cuda.synchronize()
        assert (C8.float() - C16.float()).abs().max() <= 2e-2 * C16.float().abs().max()
        assert (C8.float() - C16.float()).abs().mean() < 1e-4 * C16.float().abs().max()
        assert (cs8 - cs16).abs().max() < 1e-3 * cs16.abs().max()
        lim = 57344.0
        want = (C8.float() * 64.0).clamp(-lim, lim).to(torch.float8_e5m2).view(torch.uint8).int()
        diff = (c8.int() - want).abs()          # the copy is cast from the fp32 value, the comparison from its bf16 rounding
        assert int(diff.max()) <= 1 and float((diff != 0).float().mean()) < 0.1
        assert abs(float(amax.max()) - float(C8.float().abs().max())) <= 2 ** -7 * float(amax.max())


@pytest.mark.parametrize("dgrad", ["0", "1"])
def test_fp8_under_the_exchange_plan(dev, monkeypatch, dgrad):
    """The fp8 path inside the data-parallel launch plan (gradient hooks, five backward segments, per-segment grouped weight
    gradients, two-part AdamW; no process group: ``exchange=True`` keeps the plan and skips the collectives): every gradient
    slice is reported exactly once per step, and the loss trajectory equals the plain fp8 loop's."""
    import maestro_amd.conf as conf
    from maestro_amd.ssl import mae as pmae
    from maestro_amd.train.trainer import PretrainLoop, synthetic_batch
    from oracle.gen_golden import build_datasets, case_table
    monkeypatch.setenv("MAESTRO_FP8_DGRAD", dgrad)
    case = dict(case_table()["c3_aerial_s2"])
    ds = build_datasets(case, conf)
    kw = dict(fusion_mode="group", inter_depth=1, depth=4, **COMMON)
    runs = []
    for exchange in (False, True):
        torch.manual_seed(5)
        model = pmae.mae_small(datasets=ds, mask=conf.MaskConfig(), **kw)
        loop = PretrainLoop(model, 4, dev, total_steps=8, dtype="fp8", exchange=exchange or None, bucket_mb=1)
        assert loop.engine.fp8 is not None and (loop.sync is not None) == exchange
        batch = synthetic_batch(ds.dataset, 4, dev, seed=3)
        torch.manual_seed(11)
        losses = [float(loop.step(batch).item()) for _ in range(5)]
        if exchange:
            covered = sorted(loop.sync.launched)
            assert covered[0][0] == 0 and covered[-1][1] == loop.engine.store.grad_all.numel()
            assert all(a[1] == b[0] for a, b in zip(covered, covered[1:])), "buckets must tile the gradient buffer"
        runs.append(losses)
    assert all(l == l for l in runs[0] + runs[1])
    assert all(abs(a - b) < 2e-3 * abs(a) for a, b in zip(*runs)), runs      # same arithmetic; the wgrad launches are grouped differently


def test_fp8_on_the_lightning_surface(dev, monkeypatch):
    """``MAESTRO_DTYPE=fp8`` under ``SSLModule`` as Lightning drives it (``training_step`` -> ``loss.backward()`` -> a TORCH
    optimizer that changes the masters behind the engine's back): the e4m3 weight shadows are rebuilt from the updated masters
    with freshly derived scales at the next forward, and training makes progress."""
    from types import SimpleNamespace

    import maestro_amd.conf as conf
    from maestro_amd.train.model import SSLModule
    from maestro_amd.train.trainer import synthetic_batch
    from oracle.gen_golden import build_datasets, case_table
    monkeypatch.setenv("MAESTRO_DTYPE", "fp8")
    ds = build_datasets(dict(case_table()["c3_aerial_s2"]), conf)
    torch.manual_seed(0)
    mod = SSLModule(datasets=ds, mask=conf.MaskConfig(), interpolate="nearest", fusion_mode="group", inter_depth=1, model="mae",
                    model_size="small", loss="l2_norm", use_ema=False)
    mod.trainer = SimpleNamespace(ssl_phase="pretrain", train_dataloader=SimpleNamespace(batch_size=2), accumulate_grad_batches=1,
                                  num_nodes=1, num_devices=1, base_lr=3e-3, wd=0.01, b1=0.9, b2=0.99, final_factor=1e7,
                                  estimated_stepping_batches=20, max_epochs=5)
    batch = synthetic_batch(ds.dataset, 2, dev)
    cfg = mod.configure_optimizers()
    opt, sched = cfg["optimizer"], cfg["lr_scheduler"]["scheduler"]
    losses = []
    for step in range(5):
        torch.manual_seed(11)
        out = mod.training_step(batch, step)
        opt.zero_grad(set_to_none=True)
        out["loss"].backward()
        opt.step()
        sched.step()
        losses.append(out["loss"].item())
    eng = mod.model._engine
    assert eng.fp8 is not None and all(st.f8 is not None for st in eng._all_stacks())
    assert losses[-1] < losses[0], losses
    mod.training_step(batch, 99)            # the forward after the last torch update re-quantises every weight
    torch.cuda.synchronize()
    f0 = eng.enc["aerial"].f8[0]
    w = eng.enc["aerial"].t.layers[0][0].to_qkv.weight.detach()
    scale = float(eng.fp8.wsc.scale[f0["sw_qkv"]])
    amax = float(w.abs().max())
    import math
    assert scale == 2.0 ** (math.floor(math.log2(448.0 / amax)) - 1)
    want = (w.float() * scale).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
    assert torch.equal(f0["w_qkv"], want), "e4m3 weight shadow is stale after a torch optimizer step"


# ---------------------------------------------------------------------------------------------------- guard bands (tests/guards.py)
# The fp8 entry points on operands inside poisoned storage: 0x7F (e4m3 NaN) bands and pad columns around fp8 bytes, NaN around
# floats, pitches above the dense ones, ragged M and N.  See tests/test_guard_bands_gpu.py for the bf16 path.
@pytest.mark.parametrize("tile", ["128", "128d", "256"])
@pytest.mark.parametrize("M,N,K", [(300, 520, 384), (130, 264, 1152)])
def test_gemm_fp8_guarded(dev, M, N, K, tile, monkeypatch):  # noqa: N803
    """``mh_gemm_fp8`` with lda, ldb > K, ldc > N and the fp8 copy with ldc8 > N.  Exact data: test_gemm_fp8_integer_exact; the c8
    copy and its absmax: the bounds of test_gemm_fp8_epilogues_match_bf16_kernel."""
    from maestro_amd import hip
    from tests.guards import GuardSet
    monkeypatch.setenv("MH_FP8_TILE", tile)
    g = torch.Generator().manual_seed(M + N + K)
    a = torch.randint(-4, 5, (M, K), generator=g).float()
    b = torch.randint(-4, 5, (N, K), generator=g).float()
    a[:, ::7] += 1.0
    for a_fmt in (0, 1):
        gs = GuardSet(dev)
        A8 = gs.inp(_q(a, a_fmt).view(torch.uint8), ld=K + 16, fill="fp8", name="A8")  # noqa: N806
        B8 = gs.inp(_q(b, 0).view(torch.uint8), ld=K + 48, fill="fp8", name="B8")  # noqa: N806
        da, db = gs.inp(torch.tensor([0.5]), name="descale_a"), gs.inp(torch.tensor([4.0]), name="descale_b")
        C = gs.out((M, N), torch.float32, ld=N + 8, name="C")  # noqa: N806
        hip.gemm_fp8(M, N, K, A8, K + 16, B8, K + 48, C, N + 8, da, db, flags=hip.OUT_F32, a_format=a_fmt)
        gs.check()
        assert torch.equal(C.cpu(), 2.0 * (a @ b.t()))
        Cb = gs.out((M, N), torch.bfloat16, ld=N + 16, name="C (bf16)")  # noqa: N806
        c8 = gs.out((M, N), torch.uint8, ld=N + 24, fill="fp8", align=8, name="c8")
        s8, amax = gs.inp(torch.tensor([2.0 ** -6]), name="c8_scale"), gs.out((hip.AMAX_PITCH,), init=0.0, name="c8_amax")
        hip.gemm_fp8(M, N, K, A8, K + 16, B8, K + 48, Cb, N + 16, da, db, a_format=a_fmt, c8=c8, ldc8=N + 24, c8_scale=s8, c8_amax=amax)
        gs.check()
        want = (2.0 * (a @ b.t())).bfloat16()
        assert torch.equal(Cb.cpu(), want)
        want8 = _q((want.float() * 2.0 ** -6).clamp(-448, 448), 0).view(torch.uint8).int()
        diff = (c8.cpu().int() - want8).abs()
        assert int(diff.max()) <= 1 and float((diff != 0).float().mean()) < 0.05
        assert abs(float(amax.max()) - float(want.float().abs().max())) <= 2 ** -7 * float(amax.max())


def test_quantisers_and_scale_update_guarded(dev):
    """``mh_quant_batched`` (cast + transposed copy + absmax), ``mh_fp8_update_scales`` on a slice of the tables and
    ``mh_transpose_u8_batched``: references of test_quantiser_matches_torch_float8 / test_transpose_u8_batched."""
    import math

    from maestro_amd import hip
    from tests.guards import GuardSet, bits_equal
    g = torch.Generator().manual_seed(3)
    gs = GuardSet(dev)
    x_h = torch.randn(257, 64, generator=g) * torch.exp(3 * torch.randn(257, 1, generator=g))
    n_slots = 4
    scale = gs.out((n_slots,), init=1.0, name="scale")
    descale = gs.out((n_slots,), init=1.0, name="descale")
    amax = gs.out((n_slots, hip.AMAX_PITCH), init=0.0, name="amax")
    scale[2] = 0.25

    class Tables:                                            # what QuantBatch reads of hip.Fp8Scales
        pass
    sc = Tables()
    sc.scale, sc.amax = scale, amax
    jobs, wants = [], []
    for dtype, fmt, slot in ((torch.float32, 0, 2), (torch.bfloat16, 1, 1)):
        x = x_h.to(dtype)
        src = gs.inp(x, name="src")
        dst = gs.out(x.shape, torch.uint8, fill="fp8", name="dst")
        dst_t = gs.out((64, 257), torch.uint8, fill="fp8", name="dst_t")
        jobs.append(dict(src=src, dst=dst, dst_t=dst_t, slot=slot, format=fmt))
        s = 0.25 if slot == 2 else 1.0
        lim = hip.FP8_MAX[fmt]
        wants.append((dst, dst_t, _q((x.float() * s).clamp(-lim, lim), fmt).view(torch.uint8), slot, float(x.float().abs().max())))
    hip.QuantBatch(jobs, sc, dev).launch(2)
    gs.check()
    for dst, dst_t, want, slot, mx in wants:
        assert torch.equal(dst.cpu(), want) and torch.equal(dst_t.cpu(), want.t().contiguous())
        assert float(amax[slot].max()) == mx
    assert float(amax[0].max()) == 0.0 and float(amax[3].max()) == 0.0
    # scale update of slots [1, 3): slots 0 and 3 keep their bits
    keep = [t.clone() for t in (scale[0:1], scale[3:], descale[0:1], descale[3:], amax[0], amax[3])]
    mx1, mx2 = wants[1][4], wants[0][4]
    hip.call("mh_fp8_update_scales", amax[1:3], scale[1:3], descale[1:3], hip._I(2), hip._F(448.0), hip._I(1))
    gs.check()
    for t, t0 in zip((scale[0:1], scale[3:], descale[0:1], descale[3:], amax[0], amax[3]), keep):
        assert bits_equal(t, t0)
    for slot, mx in ((1, mx1), (2, mx2)):
        assert float(scale[slot]) == 2.0 ** (math.floor(math.log2(448.0 / mx)) - 1) and float(amax[slot].max()) == 0.0
        assert float(descale[slot]) == 1.0 / float(scale[slot])
    shapes = [(64, 64), (768, 1024), (512, 128)]
    pairs = []
    for s in shapes:
        src = gs.inp(torch.randint(0, 256, s, generator=g, dtype=torch.uint8), fill="fp8", name="transpose src")
        pairs.append((src, gs.out((s[1], s[0]), torch.uint8, fill="fp8", name="transpose dst")))
    hip.TransposeBatch(pairs, dev).launch()
    gs.check()
    for s, d in pairs:
        assert torch.equal(d.cpu(), s.cpu().t().contiguous())


def test_adamw_fp8_on_a_slice_of_the_flat_store(dev):
    """``mh_adamw_fp8`` on elements [lo, hi) of the flat p, g, m, v, bf16 and fp8 buffers, lo a multiple of 64 (the slot map's
    granule) and not of 1024, with the slot map offset that goes with it: parameters bit-identical to ``mh_adamw``'s, shadows and
    absmax as in test_adamw_fp8_refreshes_the_shadows_in_its_own_pass; everything outside the slice, NaN / 0x7F, keeps its bits."""
    from maestro_amd import hip
    from tests.guards import GuardSet, bits_equal
    total, lo, n = 64 * 70, 64 * 17, 64 * 40 + 128
    hi = lo + n
    g = torch.Generator().manual_seed(9)
    p0, grad = torch.randn(n, generator=g) * 0.05, torch.randn(n, generator=g) * 1e-3
    smap_h = torch.full((total // 64,), 2, dtype=torch.int16)             # outside the slice: the trap slot (NaN scale)
    smap_h[lo // 64: hi // 64] = -1
    smap_h[lo // 64 + 4: lo // 64 + 20], smap_h[lo // 64 + 24: lo // 64 + 40] = 0, 1
    outs = []
    for fused in (False, True):
        gs = GuardSet(dev)
        p, gr, m, v = (gs.out((total,), name=nm) for nm in "pgmv")
        half = gs.out((total,), torch.bfloat16, name="p_bf16")
        p8 = gs.out((total,), torch.uint8, fill="fp8", align=4, name="p_fp8")
        p[lo:hi], gr[lo:hi], m[lo:hi], v[lo:hi] = p0.to(dev), grad.to(dev), 0.0, 0.0
        p8[lo:hi] = 7
        smap = gs.idx(smap_h, 2, name="slot_map")
        scale = gs.inp(torch.tensor([64.0, 128.0, float("nan")]), name="scale")
        amax = gs.out((3, hip.AMAX_PITCH), init=0.0, name="amax")
        before = [torch.cat([t[:lo], t[hi:]]).clone() for t in (p, gr, m, v, half, p8)]
        if fused:
            hip.adamw_fp8(p[lo:hi], gr[lo:hi], m[lo:hi], v[lo:hi], half[lo:hi], p8[lo:hi], smap[lo // 64:], scale, amax, n, 1e-3, 0.9, 0.99,
                          1e-8, 0.01, 1, 0.5)
        else:
            hip.adamw(p[lo:hi], gr[lo:hi], m[lo:hi], v[lo:hi], half[lo:hi], n, 1e-3, 0.9, 0.99, 1e-8, 0.01, 1, 0.5)
        gs.check()
        for t, t0 in zip((p, gr, m, v, half, p8), before):
            assert bits_equal(torch.cat([t[:lo], t[hi:]]), t0), "an element outside the slice changed"
        outs.append([t[lo:hi].cpu() for t in (p, m, v, half, p8)] + [amax.cpu()])
    for a, b in zip(outs[0][:4], outs[1][:4]):
        assert bits_equal(a, b)
    p_new, p8, amax = outs[1][0], outs[1][4], outs[1][5]
    assert torch.isfinite(p_new).all()
    for slot, (s0, s1), sc in ((0, (4 * 64, 20 * 64), 64.0), (1, (24 * 64, 40 * 64), 128.0)):
        want = _q((p_new[s0:s1] * sc).clamp(-448, 448), 0).view(torch.uint8)
        assert torch.equal(p8[s0:s1], want) and float(amax[slot].max()) == float(p_new[s0:s1].abs().max())
    assert bool((p8[: 4 * 64] == 7).all()) and bool((p8[20 * 64: 24 * 64] == 7).all()) and bool((p8[40 * 64:] == 7).all())
    assert float(amax[2].abs().max()) == 0.0                              # the trap slot saw nothing

