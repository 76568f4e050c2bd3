"""fp8 with MX block scaling (``fp8_scaling="mx"``, include/maestro_hip.h "MX block scaling"): the quantiser bit for bit against a
host emulation of the rule, the block-scaled GEMM on exact data (per-lane scale map, A/B scale swap, every tile), its epilogues
and c8 copy, the LayerNorm's MX output, the weight shadows, the step against the fp32 oracle (small model and C5 at full
width), and the absence of scale state."""

import pytest
import torch

pytestmark = pytest.mark.gpu

# Small model (3 layers, E = 384) and C5 at full width against the fp32 oracle: tolerances <= 2x the MX errors observed on
# MI355X (profiles/mx_observed_errors.md).  Small: loss 4.1e-3, reconstructions 5.5e-2, worst gradient 8.3e-2.  C5 plain / stress:
# loss 7.0e-4 / 1.2e-3, reconstructions 7.1e-2 / 7.2e-2, worst gradient 0.170 / 0.181, worst per-stack hidden state 9.6e-2 / 1.02e-1.
# Per-tensor fp8 on the same cases: tests/test_fp8_gpu.py, test_fullwidth_parity_gpu.py.
MX_LOSS_TOL, MX_PIX_TOL, MX_GRAD_TOL = 8.2e-3, 1.1e-1, 1.66e-1
MX_FW_LOSS_TOL, MX_FW_PIX_TOL, MX_FW_GRAD_TOL, MX_FW_HID_TOL = 2.4e-3, 1.43e-1, 3.6e-1, 2.0e-1
FP8_GRAD_TOL_TENSOR = 0.376      # the per-tensor bound of tests/test_fullwidth_parity_gpu.py: MX must come out below it


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------------- host emulation
from tests.fp8_codes import mx_dequant, mx_ref  # noqa: E402  (the MX rule in exact float64 arithmetic, and its inverse)


def _scales(rows, cols, dev):
    from maestro_amd.fp8 import mx_scale_cols
    return torch.full((rows, mx_scale_cols(cols)), 0xAB, dtype=torch.uint8, device=dev)[:, : cols // 32]


def test_mx_reference_rule():
    """The emulation itself on hand-made blocks: 448 2^k exactly -> 127 + k, one ulp above -> 128 + k, zero -> 127."""
    x = torch.zeros(1, 128, dtype=torch.bfloat16)
    x[0, 0], x[0, 32], x[0, 64] = 448.0, 900.0, 1.0
    _, s, _ = mx_ref(x)
    assert s.tolist() == [[127, 129, 119, 127]]       # 900 > 448 * 2 -> e = 2; 1 <= 448 / 2^8 = 1.75 -> e = -8


def test_quant_mx_matches_the_rule_bit_for_bit(dev):
    from maestro_amd import hip
    g = torch.Generator().manual_seed(5)
    jobs, want = [], []
    for rows, cols, pad_s, pad_d, pad_sc in ((37, 768, 8, 16, 3), (130, 96, 0, 0, 0), (5, 3072, 4, 32, 1)):
        x = torch.randn(rows, cols // 32, 32, generator=g) * torch.exp(3 * torch.randn(rows, cols // 32, 1, generator=g))
        x = x.reshape(rows, cols)
        x[0, :32] = 0.0                                                    # all-zero block
        for k, blk in zip((-3, 0, 5), (1, 2, 3)):                          # amax exactly 448 2^k
            if blk < cols // 32:
                x[1 % rows, 32 * blk: 32 * blk + 32] = torch.linspace(-1, 1, 32) * 448.0 * 2.0 ** k
        x[2 % rows, :32] = torch.tensor(2.0 ** -130) * torch.arange(1, 33)  # bf16 subnormals (the whole block)
        x[3 % rows, 40:72] = torch.tensor(1e-39)                              # subnormals straddling two blocks
        xb = x.bfloat16()
        if cols >= 96:
            xb[rows - 1, 35] = float("nan")                                   # one NaN block
            xb[rows - 1, 64] = float("inf")                                   # one inf block
        src = torch.zeros(rows, cols + pad_s, dtype=torch.bfloat16, device=dev)
        src[:, :cols] = xb.to(dev)
        dst = torch.full((rows, cols + pad_d), 0x5A, dtype=torch.uint8, device=dev)
        sc = torch.full((rows, cols // 32 + pad_sc), 0x5A, dtype=torch.uint8, device=dev)
        jobs.append(dict(src=src[:, :cols], dst=dst[:, :cols], scales=sc[:, : cols // 32]))
        want.append((xb, dst, sc))
    hip.QuantMxBatch(jobs, dev).launch()                 # several jobs, one launch
    torch.cuda.synchronize()
    for (xb, dst, sc), jb in zip(want, jobs):
        rows, cols = xb.shape
        q, s, finite = mx_ref(xb)
        got_q, got_s = dst[:, :cols].cpu(), sc[:, : cols // 32].cpu()
        assert torch.equal(got_s, s), (got_s != s).nonzero()[:8]
        fin = finite.repeat_interleave(32, dim=1)
        assert torch.equal(got_q[fin], q[fin])
        if cols >= 96:
            assert int(got_s[rows - 1, 1]) == 0xFF and int(got_s[rows - 1, 2]) == 0xFF     # NaN and inf blocks poison the scale
        assert int(got_s[0, 0]) == 127
        assert bool((dst[:, cols:].cpu() == 0x5A).all()) and bool((sc[:, cols // 32:].cpu() == 0x5A).all())   # padding untouched


@pytest.mark.parametrize("tile", ["128", "128d", "256"])
@pytest.mark.parametrize("M,N,K", [(256, 256, 128), (300, 520, 384), (1000, 136, 256), (64, 768, 768), (130, 264, 1152),
                                   (64, 256, 3072)])      # (the last: fc2's depth, 24 K steps; sum |terms| = 3.6e4 at most, in units of 2^-5: far below 2^24 units)
def test_gemm_mx_exact_data(dev, M, N, K, tile, monkeypatch):
    """Small integers times independent random power-of-two block scales: every product and partial sum is exact in fp32, so
    any mistake in the per-lane scale map (row, K block), the A/B scale swap or the scale staging changes bits."""
    from maestro_amd import hip
    monkeypatch.setenv("MH_FP8_TILE", tile)
    g = torch.Generator().manual_seed(M + 3 * N + K)
    a = torch.randint(-3, 4, (M, K), generator=g).float()
    b = torch.randint(-3, 4, (N, K), generator=g).float()
    a[:, ::7] += 1.0                                     # asymmetric A and B
    b[::5, :] -= 0.5
    ea = torch.randint(-2, 3, (M, K // 32), generator=g)
    eb = torch.randint(-2, 3, (N, K // 32), generator=g)
    A8 = a.to(torch.float8_e4m3fn).view(torch.uint8).to(dev)  # noqa: N806
    B8 = b.to(torch.float8_e4m3fn).view(torch.uint8).to(dev)  # noqa: N806
    sa, sb = _scales(M, K, dev), _scales(N, K, dev)
    sa.copy_((ea + 127).to(torch.uint8).to(dev))
    sb.copy_((eb + 127).to(torch.uint8).to(dev))
    C = torch.full((M, N), float("nan"), device=dev)  # noqa: N806
    hip.gemm_mx(M, N, K, A8, K, sa, sa.stride(0), B8, K, sb, sb.stride(0), C, N, flags=hip.OUT_F32)
    torch.cuda.synchronize()
    ad = a.double() * torch.exp2(ea.double()).repeat_interleave(32, dim=1)
    bd = b.double() * torch.exp2(eb.double()).repeat_interleave(32, dim=1)
    assert torch.equal(C.cpu(), (ad @ bd.t()).float())


def test_gemm_mx_epilogues_and_c8_copy(dev):
    """Epilogues against the bf16 kernel fed with the DEQUANTISED operands (exact in bf16: 4 significant bits times a power of
    two), tolerances of test_gemm_fp8_epilogues_match_bf16_kernel; the c8 bytes and scales EQUAL quant_mx of the kernel's own
    bf16 output C."""
    from maestro_amd import hip
    g = torch.Generator().manual_seed(11)
    M, N, K = 640, 1024, 256  # noqa: N806
    xa = torch.randn(M, K // 32, 32, generator=g) * torch.exp(torch.randn(M, K // 32, 1, generator=g))   # block-wise ranges
    xa = xa.reshape(M, K).bfloat16().to(dev)
    xb = (torch.randn(N, K, generator=g) * 0.1).bfloat16().to(dev)
    A8, sa = hip.quant_mx(xa)  # noqa: N806
    B8, sb = hip.quant_mx(xb)  # noqa: N806
    A16, B16 = mx_dequant(A8, sa).bfloat16().to(dev), mx_dequant(B8, sb).bfloat16().to(dev)  # noqa: N806
    bias, res = torch.randn(N, generator=g).to(dev), torch.randn(M, N, generator=g).to(dev)
    C8, C16 = (torch.empty(M, N, dtype=torch.bfloat16, device=dev) for _ in range(2))  # noqa: N806
    X8, X16 = (torch.empty(M, N, dtype=torch.bfloat16, device=dev) for _ in range(2))  # noqa: N806
    c8, c8s = torch.zeros(M, N, dtype=torch.uint8, device=dev), _scales(M, N, dev)
    fl = hip.BIAS | hip.GELU | hip.AUX_DGELU
    hip.gemm_mx(M, N, K, A8, K, sa, sa.stride(0), B8, K, sb, sb.stride(0), C8, N, flags=fl, bias=bias, aux_out=X8, ldaux=N,
                c8=c8, ldc8=N, c8_scales=c8s, ldc8s=c8s.stride(0))
    hip.gemm(hip.GEMM_NT, M, N, K, A16, K, B16, K, C16, N, fl, bias=bias, aux_out=X16, ldaux=N)
    torch.cuda.synchronize()
    assert (C8.float() - C16.float()).abs().max() <= 2e-2 * C16.float().abs().max() and (X8.float() - X16.float()).abs().max() < 2e-2
    assert (C8.float() - C16.float()).abs().mean() < 1e-4
    q, s = hip.quant_mx(C8)
    torch.cuda.synchronize()
    assert torch.equal(c8.cpu(), q.cpu()) and torch.equal(c8s.cpu(), s.cpu())
    q_ref, s_ref, _ = mx_ref(C8)
    assert torch.equal(c8.cpu(), q_ref) and torch.equal(c8s.cpu(), s_ref)
    # proj / fc2-style on O(1) operands (the data of the per-tensor test): fp32 sums of exact products, grouped differently
    A8, sa = hip.quant_mx(torch.randn(M, K, generator=g).bfloat16().to(dev))  # noqa: N806
    B8, sb = hip.quant_mx((torch.randn(N, K, generator=g) * 0.1).bfloat16().to(dev))  # noqa: N806
    A16, B16 = mx_dequant(A8, sa).bfloat16().to(dev), mx_dequant(B8, sb).bfloat16().to(dev)  # noqa: N806
    D8, D16 = torch.empty(M, N, device=dev), torch.empty(M, N, device=dev)  # noqa: N806
    fl = hip.OUT_F32 | hip.BIAS | hip.RESIDUAL
    hip.gemm_mx(M, N, K, A8, K, sa, sa.stride(0), B8, K, sb, sb.stride(0), D8, N, flags=fl, bias=bias, res=res, ldr=N)
    hip.gemm(hip.GEMM_NT, M, N, K, A16, K, B16, K, D16, N, fl, bias=bias, res=res, ldr=N)
    torch.cuda.synchronize()
    assert (D8 - D16).abs().max() < 1e-3


@pytest.mark.parametrize("dim", [512, 768, 1024, 384])      # (384: the generic kernel, the small models' width)
def test_layernorm_fwd_mx(dev, dim):
    """Row map (L, off) and a ragged row count: y is layernorm_fwd's bit for bit, y8 and its scales equal quant_mx(y)."""
    from maestro_amd import hip
    g = torch.Generator().manual_seed(dim)
    B, L, off, n = 3, 50, 7, 37  # noqa: N806
    x = (torch.randn(B * L, dim, generator=g) * 3 + 0.5).to(dev)
    gamma, beta = (1 + 0.2 * torch.randn(dim, generator=g)).to(dev), (0.1 * torch.randn(dim, generator=g)).to(dev)
    y, y2 = (torch.zeros(B * L, dim, dtype=torch.bfloat16, device=dev) for _ in range(2))
    y8 = torch.zeros(B * L, dim, dtype=torch.uint8, device=dev)
    ys = _scales(B * L, dim, dev)
    mean, rstd = torch.zeros(B * n, device=dev), torch.zeros(B * n, device=dev)
    hip.layernorm_fwd_mx(x, L, off, gamma, beta, y, L, off, mean, rstd, B, n, dim, y8, ys, ys.stride(0))
    hip.layernorm_fwd(x, L, off, gamma, beta, y2, L, off, mean, rstd, B, n, dim)
    torch.cuda.synchronize()
    assert torch.equal(y.view(torch.int16), y2.view(torch.int16))
    rows = torch.tensor([b * L + off + j for b in range(B) for j in range(n)])
    q, s = hip.quant_mx(y[rows.to(dev)].contiguous())
    torch.cuda.synchronize()
    assert torch.equal(y8.cpu()[rows], q.cpu()) and torch.equal(ys.cpu()[rows], s.cpu())
    untouched = torch.ones(B * L, dtype=torch.bool)
    untouched[rows] = False
    assert bool((y8.cpu()[untouched] == 0).all()) and bool((ys.cpu()[untouched] == 0xAB).all())


# ---------------------------------------------------------------------------------------------------- engine
COMMON = dict(interpolate="nearest", model="mae", num_levels=1, type_head="attentive", fac_abs_enc=1.0, fac_date_enc=1.0)


def _small_case(seed=77):
    import maestro_amd.conf as conf
    from maestro_amd.ssl import mae as pmae
    from oracle import mae as om
    from oracle.gen_golden import build_datasets, case_table, init_weights
    case = dict(case_table()["c3_aerial_s2"])
    ds = build_datasets(case, conf)
    kw = dict(fusion_mode="group", inter_depth=1, depth=3, **COMMON)
    oracle = om.build_oracle(ds, conf.MaskConfig(), model_size="small", **kw)
    init_weights(oracle, seed)

    def model():
        m = pmae.mae_small(datasets=ds, mask=conf.MaskConfig(), **kw)
        m.load_state_dict(oracle.state_dict(), strict=True)
        return m
    return ds, oracle, model


def _check_shadows(eng):
    """Every MX weight shadow and its scales equal quant_mx of the weight's bf16 shadow."""
    from maestro_amd import hip
    n = 0
    for st in eng._all_stacks():
        for l, (attn, ff) in enumerate(st.t.layers):
            f = st.f8[l]
            for key, lin in (("qkv", attn.to_qkv), ("proj", attn.to_out[0]), ("fc1", ff.net[1]), ("fc2", ff.net[4])):
                q, s = hip.quant_mx(eng.store.h(lin.weight))
                assert torch.equal(f["w_" + key], q) and torch.equal(eng.fp8.w_scales(f["sw_" + key]), s), (st.tag, l, key)
                n += 1
    assert n > 0


def _rel(a, b):
    return ((a - b).double().norm() / b.double().norm().clamp(min=1e-12)).item()


def _small_step(dev, model, oracle, ds, scaling, B=4):  # noqa: N803
    """One forward + backward on the small case; returns (engine, errors dict) against the oracle."""
    from oracle import mae as om
    from oracle.gen_golden import make_batch
    batch = make_batch(ds.dataset, B, 5)
    eng = model.engine(B, dev, loss="l2_norm", dtype="fp8", fp8_scaling=scaling)
    assert eng.fp8 is not None and eng.fp8.scaling == scaling and all(st.f8 is not None for st in eng._all_stacks())
    torch.manual_seed(3)
    noise, struct = eng.draw_masks()
    dbatch = {k: v.to(dev) for k, v in batch.items()}
    loss = eng.forward(dbatch, noise=noise, struct=struct).clone()
    eng.zero_grad()
    eng.backward()
    torch.cuda.synchronize()
    pixels, masks = eng.reconstructions()
    ob, orec, omsk, _ = oracle({k: v.clone() for k, v in batch.items()}, "pretrain", noise=noise,
                               struct_masks={g: s[:, :, None] for g, s in struct.items()})
    oloss = om.compute_loss_rec(ob, orec, omsk, oracle.out_grid_size, om.norm_bands_of(ds.dataset), "l2_norm")
    oracle.zero_grad()
    oloss.backward()
    err = {"loss": abs(loss.item() - oloss.item()) / abs(oloss.item())}
    for m in orec:
        assert torch.equal(masks[m].cpu(), omsk[m]), f"{m}: masks differ"
        err[f"pixels/{m}"] = _rel(pixels[m].cpu(), orec[m].detach())
    ograds = {k: p.grad for k, p in oracle.named_parameters() if p.grad is not None}
    gmax = max(g.abs().max().item() for g in ograds.values())
    worst, fails = (0.0, None), []
    for k, p in model.named_parameters():
        if k in ograds:
            got, want = eng.store.g(p).cpu(), ograds[k]
            e, ref = (got - want).double().norm().item(), want.double().norm().item()
            floor = 1e-4 * gmax * want.numel() ** 0.5
            if ref > 10 * floor and e / ref > worst[0]:
                worst = (e / ref, k)
            if e > MX_GRAD_TOL * ref + floor:
                fails.append((k, e / max(ref, 1e-12)))
    err["grad_worst"] = worst[0]
    return eng, err, fails, (dbatch, noise, struct, oloss)


def test_engine_mx_matches_oracle_and_refreshes_shadows(dev, observed):
    from maestro_amd.train.optim import FusedAdamW
    ds, oracle, model = _small_case()
    m_mx, m_t = model(), model()
    eng, err, fails, (dbatch, noise, struct, oloss) = _small_step(dev, m_mx, oracle, ds, "mx")
    _, err_t, _, _ = _small_step(dev, m_t, oracle, ds, "tensor")
    for k, v in err.items():
        observed("mx/small", k, v)
        print(f"[mx/small] {k:24s} mx {v:.3e}   per-tensor {err_t[k]:.3e}")
    assert err["loss"] < MX_LOSS_TOL, err
    assert all(v < MX_PIX_TOL for k, v in err.items() if k.startswith("pixels/")), err
    assert not fails, fails[:5]
    _check_shadows(eng)                                    # after construction
    assert eng.fp8.before_fused_adamw() is False
    FusedAdamW(eng, 1e-3).step()
    torch.cuda.synchronize()
    _check_shadows(eng)                                    # after one optimizer step (plain AdamW, then one quantiser launch)
    loss3 = eng.forward(dbatch, noise=noise, struct=struct).clone()
    assert abs(loss3.item() - oloss.item()) > 10 * MX_LOSS_TOL * abs(oloss.item())      # the update moved the loss


def test_mx_has_no_hidden_state(dev):
    """Two engines with the same weights: one first runs two steps on other batches with 8x weights (loaded through
    load_state_dict, then loaded back).  Same batch, same draws afterwards: bit-identical reconstructions and layer-0 MX copy."""
    from maestro_amd.train.optim import FusedAdamW
    from oracle.gen_golden import make_batch
    ds, _, model = _small_case(seed=21)
    ma, mb = model(), model()
    B = 2  # noqa: N806
    ea = ma.engine(B, dev, loss="l2_norm", dtype="fp8", fp8_scaling="mx")
    eb = mb.engine(B, dev, loss="l2_norm", dtype="fp8", fp8_scaling="mx")
    orig = {k: v.detach().clone() for k, v in ma.state_dict().items()}
    ma.load_state_dict({k: v * 8 if v.is_floating_point() else v for k, v in orig.items()}, strict=True)
    opt = FusedAdamW(ea, 1e-3)
    for seed in (41, 42):
        other = {k: v.to(dev) for k, v in make_batch(ds.dataset, B, seed).items()}
        ea.forward(other)
        ea.zero_grad()
        ea.backward()
        opt.step()
    ma.load_state_dict(orig, strict=True)
    batch = {k: v.to(dev) for k, v in make_batch(ds.dataset, B, 5).items()}
    torch.manual_seed(9)
    noise, struct = ea.draw_masks()
    la = ea.forward(batch, noise=noise, struct=struct).clone()
    lb = eb.forward(batch, noise=noise, struct=struct).clone()
    torch.cuda.synchronize()
    pa, _ = ea.reconstructions()
    pb, _ = eb.reconstructions()
    for m in pa:
        assert torch.equal(pa[m], pb[m]), m
    g = ea.groups[0].name
    fa, fb = ea.enc[g].f8[0], eb.enc[g].f8[0]
    assert torch.equal(fa["h1"], fb["h1"]) and torch.equal(fa["mx_h1"], fb["mx_h1"])
    assert abs(la.item() - lb.item()) <= 1e-6 * abs(lb.item())


@pytest.mark.parametrize("stress", [False, True])
def test_mx_matches_oracle_at_full_width(stress, observed, dev):
    """C5 at ViT-B width (the setup of test_engine_matches_oracle_at_full_width) with fp8_scaling="mx", per-stack hidden states."""
    import bench
    import maestro_amd.conf as conf
    from maestro_amd.ssl import mae as pmae
    from maestro_amd.train.trainer import synthetic_batch
    from oracle import mae as om
    from oracle.gen_golden import init_weights, stress_raster
    assert MX_FW_GRAD_TOL < FP8_GRAD_TOL_TENSOR
    config, B = "c5", 2  # noqa: N806
    w = bench.WORKLOADS[config]
    ds = w["ds"]()
    torch.set_float32_matmul_precision("highest")
    common = dict(interpolate="nearest", fusion_mode="group", inter_depth=3, model="mae", num_levels=1)
    oracle = om.build_oracle(ds, conf.MaskConfig(), model_size=w["size"], **common)
    init_weights(oracle, 100 + len(config))
    model = getattr(pmae, f"mae_{w['size']}")(datasets=ds, mask=conf.MaskConfig(), **common)
    model.load_state_dict(oracle.state_dict(), strict=True)
    batch = synthetic_batch(ds.dataset, B, "cpu", seed=3)
    if stress:
        g = torch.Generator().manual_seed(99)
        for m, c in ds.dataset.inputs.items():
            batch[m] = stress_raster(batch[m], c.patch_size.mae, g)
    eng = model.engine(B, dev, loss="l2_norm", dtype="fp8", fp8_scaling="mx")
    assert eng.fp8.scaling == "mx" and all(st.f8 is not None for st in eng._all_stacks())
    torch.manual_seed(17)
    noise, struct = eng.draw_masks()
    loss = eng.forward({k: v.to(dev) for k, v in batch.items()}, noise=noise, struct=struct)
    eng.zero_grad()
    eng.backward()
    torch.cuda.synchronize()
    pixels, masks = eng.reconstructions()
    hidden = {}

    def grab(name):
        def hook(mod, args):
            hidden.setdefault(name, args[0].detach().clone())
        return hook

    hooks = []
    for g in eng.groups:
        hooks.append(oracle.encoder[g.model].norm.register_forward_pre_hook(grab(f"enc.{g.name}")))
        hooks.append(oracle.decoder[g.model].norm.register_forward_pre_hook(grab(f"dec.{g.name}")))
    if oracle.encoder_inter is not None:
        hooks.append(oracle.encoder_inter.norm.register_forward_pre_hook(grab("joint")))
    ob, orec, omsk, _ = oracle({k: v.clone() for k, v in batch.items()}, "pretrain", noise=noise,
                               struct_masks={g: s[:, :, None] for g, s in struct.items()})
    for h in hooks:
        h.remove()
    oloss = om.compute_loss_rec(ob, orec, omsk, oracle.out_grid_size, om.norm_bands_of(ds.dataset), "l2_norm")
    oracle.zero_grad()
    oloss.backward()
    tag = "fullwidth/c5/mx" + ("/stress" if stress else "")
    for m in orec:
        assert torch.equal(masks[m].cpu(), omsk[m]), f"{m}: mask differs from the oracle"
        e = _rel(pixels[m].cpu(), orec[m].detach())
        observed(tag, f"pixels/{m}", e)
        assert e < MX_FW_PIX_TOL, (m, e)
    stacks = {f"enc.{g.name}": eng.enc[g.name] for g in eng.groups}
    stacks.update({f"dec.{g.name}": eng.dec[g.name] for g in eng.groups})
    if eng.joint is not None:
        stacks["joint"] = eng.joint
    assert set(stacks) == set(hidden)
    worst_h = (0.0, None)
    for name, st in stacks.items():
        want = hidden[name].reshape(-1, hidden[name].shape[-1])
        e = _rel(st.x_last.cpu(), want)
        observed(tag, f"hidden/{name}", e)
        worst_h = max(worst_h, (e, name))
        assert e < MX_FW_HID_TOL, (name, e)
    e = abs(loss.item() - oloss.item()) / abs(oloss.item())
    observed(tag, "loss", e)
    assert e < MX_FW_LOSS_TOL, (loss.item(), oloss.item())
    ograds = {k: p.grad for k, p in oracle.named_parameters() if p.grad is not None}
    gmax = max(g.abs().max().item() for g in ograds.values())
    worst, checked = (0.0, None), 0
    for k, p in model.named_parameters():
        if k not in ograds:
            continue
        got, want = eng.store.g(p).cpu(), ograds[k]
        err, ref = (got - want).double().norm().item(), want.double().norm().item()
        floor = 1e-5 * gmax * want.numel() ** 0.5
        if ref > 10 * floor and err / ref > worst[0]:
            worst = (err / ref, k)
        assert err <= MX_FW_GRAD_TOL * ref + floor, f"{k}: grad rel err {err / max(ref, 1e-12):.3e}"
        checked += 1
    observed(tag, f"grad_worst/{worst[1]}", worst[0])
    assert checked == len(ograds) and checked > 100
    print(f"[{tag}] loss hip={loss.item():.6f} oracle={oloss.item():.6f}; worst gradient {worst}; worst hidden state {worst_h}")


def test_mx_refuses_the_fp8_dgrad(dev, monkeypatch):
    ds, _, model = _small_case()
    monkeypatch.setenv("MAESTRO_FP8_DGRAD", "1")
    with pytest.raises(ValueError, match="MAESTRO_FP8_DGRAD.*mx|mx.*MAESTRO_FP8_DGRAD"):
        model().engine(2, dev, loss="l2_norm", dtype="fp8", fp8_scaling="mx")


# ---------------------------------------------------------------------------------------------------- guard bands (tests/guards.py)
# The MX entry points on operands inside poisoned storage: 0x7F (e4m3 NaN) around element bytes, 0xFF (E8M0 NaN) around scale
# bytes, NaN around floats; operand AND scale pitches above the dense ones, ragged M and N.
@pytest.mark.parametrize("tile", ["128", "128d", "256"])
@pytest.mark.parametrize("M,N,K", [(300, 520, 384), (130, 264, 1152)])
def test_gemm_mx_guarded(dev, M, N, K, tile, monkeypatch):  # noqa: N803
    """``mh_gemm_mx`` on the exact data of test_gemm_mx_exact_data with lda, ldb > K, ldsa, ldsb > K / 32, ldc > N."""
    from maestro_amd import hip
    from tests.guards import GuardSet
    monkeypatch.setenv("MH_FP8_TILE", tile)
    g = torch.Generator().manual_seed(M + 3 * N + K)
    a = torch.randint(-3, 4, (M, K), generator=g).float()
    b = torch.randint(-3, 4, (N, K), generator=g).float()
    a[:, ::7] += 1.0
    b[::5, :] -= 0.5
    ea = torch.randint(-2, 3, (M, K // 32), generator=g)
    eb = torch.randint(-2, 3, (N, K // 32), generator=g)
    gs = GuardSet(dev)
    A8 = gs.inp(a.to(torch.float8_e4m3fn).view(torch.uint8), ld=K + 16, fill="fp8", name="A8")  # noqa: N806
    B8 = gs.inp(b.to(torch.float8_e4m3fn).view(torch.uint8), ld=K + 48, fill="fp8", name="B8")  # noqa: N806
    ldsa, ldsb = (K // 32 + 3) // 4 * 4 + 4, (K // 32 + 3) // 4 * 4 + 12
    sa = gs.inp((ea + 127).to(torch.uint8), ld=ldsa, fill="e8m0", align=4, name="sa")
    sb = gs.inp((eb + 127).to(torch.uint8), ld=ldsb, fill="e8m0", align=4, name="sb")
    C = gs.out((M, N), torch.float32, ld=N + 8, name="C")  # noqa: N806
    hip.gemm_mx(M, N, K, A8, K + 16, sa, ldsa, B8, K + 48, sb, ldsb, C, N + 8, flags=hip.OUT_F32)
    gs.check()
    ad = a.double() * torch.exp2(ea.double()).repeat_interleave(32, dim=1)
    bd = b.double() * torch.exp2(eb.double()).repeat_interleave(32, dim=1)
    assert torch.equal(C.cpu(), (ad @ bd.t()).float())


@pytest.mark.parametrize("M,N,K", [(300, 544, 256), (130, 288, 384)])
def test_gemm_mx_c8_copy_guarded(dev, M, N, K):  # noqa: N803
    """The MX copy of the bf16 output with ldc8 > N and ldc8s > N / 32, ragged M: exact operands, so the bf16 output is exact
    and c8 / c8_scales are the MX rule (mx_ref) applied to it, as in test_gemm_mx_epilogues_and_c8_copy."""
    from maestro_amd import hip
    from tests.guards import GuardSet
    g = torch.Generator().manual_seed(M + N)
    a = torch.randint(-3, 4, (M, K), generator=g).float()
    b = torch.randint(-3, 4, (N, K), generator=g).float()
    ea = torch.randint(-2, 3, (M, K // 32), generator=g)
    eb = torch.randint(-2, 3, (N, K // 32), generator=g)
    gs = GuardSet(dev)
    A8 = gs.inp(a.to(torch.float8_e4m3fn).view(torch.uint8), ld=K + 32, fill="fp8", name="A8")  # noqa: N806
    B8 = gs.inp(b.to(torch.float8_e4m3fn).view(torch.uint8), ld=K + 16, fill="fp8", name="B8")  # noqa: N806
    lds = K // 32 + 4
    sa = gs.inp((ea + 127).to(torch.uint8), ld=lds, fill="e8m0", align=4, name="sa")
    sb = gs.inp((eb + 127).to(torch.uint8), ld=lds, fill="e8m0", align=4, name="sb")
    C = gs.out((M, N), torch.bfloat16, ld=N + 8, name="C")  # noqa: N806
    c8 = gs.out((M, N), torch.uint8, ld=N + 24, fill="fp8", align=8, name="c8")
    ldc8s = N // 32 + 7
    ldc8s += -ldc8s % 4
    c8s = gs.out((M, N // 32), torch.uint8, ld=ldc8s, fill="e8m0", align=4, name="c8_scales")
    hip.gemm_mx(M, N, K, A8, K + 32, sa, lds, B8, K + 16, sb, lds, C, N + 8, c8=c8, ldc8=N + 24, c8_scales=c8s, ldc8s=ldc8s)
    gs.check()
    ad = a.double() * torch.exp2(ea.double()).repeat_interleave(32, dim=1)
    bd = b.double() * torch.exp2(eb.double()).repeat_interleave(32, dim=1)
    want = (ad @ bd.t()).float().bfloat16()
    assert torch.equal(C.cpu(), want)
    q, s, finite = mx_ref(want)
    assert bool(finite.all()) and torch.equal(c8.cpu(), q) and torch.equal(c8s.cpu(), s)


def test_quant_mx_guarded(dev):
    """``mh_quant_mx_batched`` with source, destination and scale pitches above the dense ones: bit for bit the rule."""
    from maestro_amd import hip
    from tests.guards import GuardSet
    g = torch.Generator().manual_seed(5)
    gs = GuardSet(dev)
    jobs, want = [], []
    for rows, cols, pad_s, pad_d, pad_sc in ((37, 768, 8, 16, 3), (130, 96, 4, 4, 1), (5, 3072, 4, 32, 1)):
        x = torch.randn(rows, cols // 32, 32, generator=g) * torch.exp(3 * torch.randn(rows, cols // 32, 1, generator=g))
        xb = x.reshape(rows, cols).bfloat16()
        xb[0, :32] = 0.0
        src = gs.inp(xb, ld=cols + pad_s, align=8, name="src")
        dst = gs.out((rows, cols), torch.uint8, ld=cols + pad_d, fill="fp8", align=4, name="dst")
        sc = gs.out((rows, cols // 32), torch.uint8, ld=cols // 32 + pad_sc, fill="e8m0", align=4, name="scales")
        jobs.append(dict(src=src, dst=dst, scales=sc))
        want.append(xb)
    hip.QuantMxBatch(jobs, dev).launch()
    gs.check()
    for jb, xb in zip(jobs, want):
        q, s, finite = mx_ref(xb)
        assert bool(finite.all()) and torch.equal(jb["dst"].cpu(), q) and torch.equal(jb["scales"].cpu(), s)
