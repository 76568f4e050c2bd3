"""GPU parity of the non-GEMM kernels (through the C ABI) against the oracle / fp32 references on the same inputs."""

import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


# ----------------------------------------------------------------------------------------------- LayerNorm
@pytest.mark.parametrize("dim,B,n,xL,xoff,yL,yoff", [(768, 3, 50, 50, 0, 50, 0), (512, 2, 37, 64, 20, 40, 3),
                                                      (192, 4, 16, 16, 0, 30, 14), (1024, 1, 9, 9, 0, 9, 0),
                                                      # rows % 4 == 0 and dim == 256 k: the straight-line kernels (norm.hip)
                                                      (768, 2, 52, 60, 3, 64, 5), (512, 4, 16, 16, 0, 16, 0),
                                                      (256, 3, 8, 11, 2, 8, 0), (1024, 2, 6, 6, 0, 9, 3)])
@pytest.mark.parametrize("out_f32", [False, True])
def test_layernorm_fwd_bwd(dev, dim, B, n, xL, xoff, yL, yoff, out_f32):
    from maestro_amd import hip
    x = _rand(B, xL, dim, seed=1).to(dev) * 2 + 0.5
    gamma, beta = (1 + 0.2 * _rand(dim, seed=2)).to(dev), (0.1 * _rand(dim, seed=3)).to(dev)
    y = torch.full((B, yL, dim), 7.0, device=dev, dtype=torch.float32 if out_f32 else torch.bfloat16)
    mean, rstd = torch.empty(B * n, device=dev), torch.empty(B * n, device=dev)
    hip.layernorm_fwd(x, xL, xoff, gamma, beta, y, yL, yoff, mean, rstd, B, n, dim)
    xs = x[:, xoff:xoff + n].clone().requires_grad_(True)
    g_ref, b_ref = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    want = F.layer_norm(xs, (dim,), g_ref, b_ref, 1e-5)
    got = y[:, yoff:yoff + n].float()
    assert (got - want).abs().max() < (1e-5 if out_f32 else 3e-2)
    assert (y[:, :yoff].float() == 7).all() and (y[:, yoff + n:].float() == 7).all()
    # backward
    dy = _rand(B, yL, dim, seed=4).to(dev)
    dy_in = dy if out_f32 else dy.bfloat16()
    dres = _rand(B, xL, dim, seed=5).to(dev)
    dx = torch.zeros(B, xL, dim, device=dev)
    dxb = torch.zeros(B, xL, dim, device=dev, dtype=torch.bfloat16)
    dg, db, dc = torch.zeros(dim, device=dev), torch.zeros(dim, device=dev), torch.ones(dim, device=dev)
    ws = torch.zeros(hip.layernorm_bwd_workspace(B * n, dim), device=dev)
    hip.layernorm_bwd(dy_in, yL, yoff, x, xL, xoff, gamma, mean, rstd, dres, dx, dxb, dg, db, dc, ws, B, n, dim)
    want.backward(dy_in[:, yoff:yoff + n].float())
    ref_dx = xs.grad + dres[:, xoff:xoff + n]
    assert (dx[:, xoff:xoff + n] - ref_dx).abs().max() < 2e-4
    assert (dxb[:, xoff:xoff + n].float() - ref_dx).abs().max() < 3e-2
    assert (dg - g_ref.grad).abs().max() < 2e-3 and (db - b_ref.grad).abs().max() < 2e-3
    assert (dc - (1 + ref_dx.sum((0, 1)))).abs().max() < 2e-3


@pytest.mark.parametrize("dim,B,n,xL,xoff,yL,yoff", [(768, 2, 32, 40, 5, 36, 2), (512, 3, 16, 16, 0, 20, 4), (256, 1, 64, 64, 0, 64, 0),
                                                      (1024, 2, 24, 30, 6, 24, 0), (768, 32, 256, 256, 0, 256, 0),
                                                      (512, 32, 1024, 1024, 0, 1024, 0)])
def test_layernorm_straight_line_forms_equal_generic(dev, dim, B, n, xL, xoff, yL, yoff):
    """The straight-line kernels (dim == 256 k, bf16 in / out, rows % 4 == 0: what the transformer blocks launch) against the
    generic kernels on the same values, up to the step's own launch sizes (8192 x 768, 32768 x 512).  Same operations in the
    same order; only the compiler's fma contraction / packing differs between the two forms, so the fp32 results agree to
    a few ulp (1e-5 here; a wrong row, lane or partial would be off by O(1)) and the bf16 ones to one bf16 ulp.  The generic
    forward is reached through an fp32 output, the generic backward through an fp32 dy that holds the bf16 values."""
    from maestro_amd import hip
    x = _rand(B, xL, dim, seed=11).to(dev) * 1.7 - 0.3
    gamma, beta = (1 + 0.2 * _rand(dim, seed=12)).to(dev), (0.1 * _rand(dim, seed=13)).to(dev)
    rows = B * n
    ya = torch.full((B, yL, dim), 7.0, device=dev, dtype=torch.bfloat16)
    yb = torch.full((B, yL, dim), 7.0, device=dev)
    stats = [torch.empty(rows, device=dev) for _ in range(4)]
    hip.layernorm_fwd(x, xL, xoff, gamma, beta, ya, yL, yoff, stats[0], stats[1], B, n, dim)
    hip.layernorm_fwd(x, xL, xoff, gamma, beta, yb, yL, yoff, stats[2], stats[3], B, n, dim)

    def close16(a, b):          # bf16 roundings of fp32 numbers that agree to ~1e-5 of the tensor's scale: one bf16 ulp apart at most
        a, b = a.float(), b.float()
        return bool(((a - b).abs() <= 2.0 ** -7 * b.abs() + 2e-5 * max(1.0, b.abs().max().item())).all())
    assert close16(ya, yb.bfloat16()) and (ya != yb.bfloat16()).float().mean() < 2e-2
    assert torch.allclose(stats[0], stats[2], rtol=1e-5, atol=1e-6) and torch.allclose(stats[1], stats[3], rtol=1e-5, atol=1e-6)
    dy = _rand(B, yL, dim, seed=14).to(dev).bfloat16()
    dres = _rand(B, xL, dim, seed=15).to(dev)
    n_ws = hip.layernorm_bwd_workspace(rows, dim)
    out = []
    for dy_in in (dy, dy.float()):
        dx = torch.full((B, xL, dim), 3.0, device=dev)
        dxb = torch.full((B, xL, dim), 3.0, device=dev, dtype=torch.bfloat16)
        ws = torch.full((n_ws,), float("nan"), device=dev)
        hip.layernorm_bwd_partial(dy_in, yL, yoff, x, xL, xoff, gamma, stats[0], stats[1], dres, dx, dxb, ws, B, n, dim)
        out.append((dx, dxb, ws))
    torch.cuda.synchronize()
    (dx_a, dxb_a, ws_a), (dx_b, dxb_b, ws_b) = out
    err = (dx_a - dx_b).abs().max().item()
    assert err < 1e-5 * max(1.0, dx_b.abs().max().item()), err
    assert close16(dxb_a, dxb_b) and (dxb_a != dxb_b).float().mean() < 2e-2
    assert torch.isfinite(ws_a).all()
    werr = (ws_a - ws_b).abs().max().item()          # sums over 16 rows of O(1) terms
    assert werr < 2e-5 * max(1.0, ws_b.abs().max().item()), werr
    assert (dx_a[:, :xoff] == 3).all() and (dx_a[:, xoff + n:] == 3).all()      # rows outside the map untouched
    assert (dxb_a[:, :xoff] == 3).all() and (dxb_a[:, xoff + n:] == 3).all()


# ----------------------------------------------------------------------------------------------- attention
def _attn_ref(qkv, scale):
    B, N, _, H, D = qkv.shape
    q, k, v = (qkv[:, :, i].transpose(1, 2).float() for i in range(3))
    s = torch.matmul(q, k.transpose(-1, -2)) * scale
    o = torch.matmul(torch.softmax(s, -1), v)
    return o.transpose(1, 2).reshape(B, N, H * D), torch.logsumexp(s, -1)


@pytest.mark.parametrize("B,N,H,D", [(2, 100, 3, 64), (1, 256, 2, 64), (2, 470, 1, 64), (2, 16, 3, 64),
                                     (1, 1024, 2, 32), (3, 50, 4, 32), (2, 225, 2, 32), (1, 129, 1, 32),
                                     (2, 356, 3, 64), (1, 448, 2, 64), (2, 144, 2, 64), (1, 400, 4, 32), (1, 513, 2, 32),
                                     (2, 257, 3, 32), (1, 1000, 1, 32), (1, 33, 2, 32), (1, 288, 1, 64), (2, 64, 2, 32), (1, 96, 1, 32), (1, 768, 3, 32)])
def test_attention_fwd_bwd(dev, B, N, H, D):
    from maestro_amd import hip
    qkv = (_rand(B, N, 3, H, D, seed=N + D) * 1.5).to(dev).bfloat16()
    scale = D**-0.5
    out = torch.zeros(B, N, H * D, device=dev, dtype=torch.bfloat16)
    lse = torch.zeros(B, H, N, device=dev)
    hip.attn_fwd(qkv, out, lse, B, N, H, D, scale)
    ref = qkv.float().requires_grad_(True)
    want, want_lse = _attn_ref(ref, scale)
    # (round 6: the forward no longer normalises the probabilities of a tile by its row maximum -- csrc/attn.hip, LAZY_RANGE -- so a
    #  row's largest probability is a bf16-rounded 2^t instead of exactly 1.0: observed lse 2.0e-3 -> 3.1e-3, output 1.9e-2 -> 2.3e-2)
    assert (out.float() - want).abs().max() < 3e-2, (out.float() - want).abs().max().item()
    assert (lse - want_lse).abs().max() < 5e-3
    dout = _rand(B, N, H * D, seed=7).to(dev).bfloat16()
    delta = torch.zeros(B, H, N, device=dev)
    dqkv = torch.full((B, N, 3, H, D), float("nan"), device=dev, dtype=torch.bfloat16)
    hip.attn_bwd(qkv, out, dout, lse, delta, dqkv, B, N, H, D, scale)
    want.backward(dout.float())
    err = (dqkv.float() - ref.grad).abs().max().item()
    assert err < 3e-2 * max(1.0, ref.grad.abs().max().item()), err
    # per part (a wrong dQ must not hide behind a larger dK): relative L2 per q / k / v
    for i, name in enumerate("qkv"):
        got, ref_i = dqkv[:, :, i].float(), ref.grad[:, :, i]
        rel = ((got - ref_i).norm() / ref_i.norm()).item()
        assert rel < 1.5e-2, (name, rel)
    want_delta = (out.float() * dout.float()).reshape(B, N, H, D).sum(-1).permute(0, 2, 1)
    assert (delta - want_delta).abs().max() < 1e-3 * max(1.0, want_delta.abs().max().item())


def test_attention_softmax_spike(dev):
    """Forces a large running-max jump between KV tiles (online-softmax rescale branch)."""
    from maestro_amd import hip
    B, N, H, D = 1, 200, 1, 64
    qkv = _rand(B, N, 3, H, D, seed=3).to(dev)
    qkv[0, 5, 0] *= 6.0
    qkv[0, 150, 1] = qkv[0, 5, 0] * 2.0  # key 150 (third tile) dominates query 5
    qkv = qkv.bfloat16()
    out = torch.zeros(B, N, H * D, device=dev, dtype=torch.bfloat16)
    lse = torch.zeros(B, H, N, device=dev)
    hip.attn_fwd(qkv, out, lse, B, N, H, D, D**-0.5)
    want, want_lse = _attn_ref(qkv.float(), D**-0.5)
    assert torch.isfinite(out.float()).all()
    assert (out.float() - want).abs().max() < 3e-2
    assert ((lse - want_lse).abs() / want_lse.abs().clamp(min=1)).max() < 2e-3


@pytest.mark.parametrize("case", ["all_low", "all_high", "rising", "low_then_spike_then_low", "short_low"])
def test_attention_reference_exponent_moves(dev, case):
    """The forward keeps a per-query REFERENCE exponent instead of a running maximum and only moves it when a tile's scores leave
    +-LAZY_RANGE around it (csrc/attn.hip): down at the first tile only, up at any tile.  Each case forces one of those moves."""
    from maestro_amd import hip
    B, N, H, D = 1, 64 if case == "short_low" else 320, 2, 32
    g = torch.Generator().manual_seed(11)
    q = torch.randn(B, N, H, D, generator=g)
    k = torch.randn(B, N, H, D, generator=g)
    v = torch.randn(B, N, H, D, generator=g)
    u = torch.zeros(D); u[0] = 1.0
    scale = D**-0.5
    big = 40.0 / scale                        # q.k = +-big^.. : a logit of +-40 (57 in log2 units) from one coordinate
    if case in ("all_low", "short_low"):      # every logit of every row ~ -40: the first tile moves the reference DOWN
        q = q * 0.3 + u * big**0.5; k = k * 0.3 - u * big**0.5
    elif case == "all_high":                  # every logit ~ +40: first tile moves it UP
        q = q * 0.3 + u * big**0.5; k = k * 0.3 + u * big**0.5
    elif case == "rising":                    # the row maximum grows by ~30 from tile to tile (64 keys each)
        q = q * 0.3 + u * big**0.5
        k = k * 0.3 + u[None, None, None, :] * (big**0.5) * (torch.arange(N) // 64).float()[None, :, None, None] * 0.75
    else:                                     # ordinary first tile, one dominating key in the third tile, ordinary tiles after it
        q[0, 7] = q[0, 7] * 0.3 + u * big**0.5
        k[0, 150] = k[0, 150] * 0.3 + u * big**0.5 * 3.0
    qkv = torch.stack([q, k, v], dim=2).to(dev).bfloat16()
    out = torch.zeros(B, N, H * D, device=dev, dtype=torch.bfloat16)
    lse = torch.zeros(B, H, N, device=dev)
    hip.attn_fwd(qkv, out, lse, B, N, H, D, scale)
    want, want_lse = _attn_ref(qkv.float(), scale)
    assert torch.isfinite(out.float()).all() and torch.isfinite(lse).all()
    assert (out.float() - want).abs().max() < 4e-2, (out.float() - want).abs().max().item()
    assert ((lse - want_lse).abs() / want_lse.abs().clamp(min=1)).max() < 5e-3


# ----------------------------------------------------------------------------------------------- patch embed
@pytest.mark.parametrize("BD,C,S,P,norm_bands,elev", [(3, 4, 64, 16, (1, 3), False), (4, 10, 10, 2, (4, 4, 2), False),
                                                       (2, 2, 64, 32, (2,), True), (2, 4, 100, 20, (1, 3), False), (2, 2, 64, 16, (2,), True), (2, 3, 48, 16, (3,), False),
                                                       (1, 1, 32, 16, (1,), False),
                                                       (5, 2, 6, 2, (1, 1), False), (2, 3, 64, 8, (3,), False)])
@pytest.mark.parametrize("normalise", [True, False])
def test_patchify(dev, BD, C, S, P, norm_bands, elev, normalise):
    from maestro_amd import hip
    from oracle import layers as ol
    from oracle import mae as om
    img = torch.rand(BD, C, S, S, generator=torch.Generator().manual_seed(S))
    g = S // P
    K = C * P * P
    Kpad = (K + 31) // 32 * 32
    cols = torch.full((BD * g * g, Kpad), 3.0, device=dev, dtype=torch.bfloat16)
    target = torch.zeros(BD * g * g, K, device=dev)
    nb = torch.tensor(norm_bands, dtype=torch.int32, device=dev)
    hip.patchify(img.to(dev), cols, target, BD, C, S, P, Kpad, nb, len(norm_bands), normalise, elev)
    ref_img = img.clone()
    if elev:
        ref_img[:, 1:] = 30 * (ref_img[:, :1] - ref_img[:, 1:])
    want_cols = ol.im2col_patches(ref_img, P).reshape(-1, K)
    assert torch.equal(cols[:, :K].cpu(), want_cols.bfloat16())
    assert (cols[:, K:] == 0).all()
    tgt = om.patch_view(ref_img[None], g)  # [1, BD, L, PP, C]
    if normalise:
        tgt = om.normalise_target(tgt, norm_bands)
    assert (target.cpu() - tgt.reshape(-1, K)).abs().max() < 2e-4


@pytest.mark.parametrize("B,D,L,E,tok_off,Lg", [(2, 1, 64, 192, 0, 64), (2, 3, 25, 768, 10, 100), (1, 4, 9, 1024, 36, 72), (2, 1, 600, 384, 8, 640),
                                                (1, 2, 9, 1028, 3, 24)])   # E > 1024: two column passes, the last one 4 columns wide
def test_groupnorm_embed_finish_fwd_bwd(dev, B, D, L, E, tok_off, Lg):
    from maestro_amd import hip
    y = (_rand(B * D * L, E, seed=1) * 1.7 + 0.3).to(dev)
    gamma, beta = (1 + 0.2 * _rand(E, seed=2)).to(dev), (0.1 * _rand(E, seed=3)).to(dev)
    pos = _rand(L, E, seed=4).to(dev)
    date = _rand(B * D, 8, seed=5).to(dev)
    partial = torch.zeros(hip.groupnorm_partial_size(B * D, L, E), device=dev)
    stats = torch.zeros(B * D, 2, device=dev)
    hip.groupnorm_stats(y, partial, stats, B * D, L, E)
    xg = torch.full((B, Lg, E), 5.0, device=dev)
    hip.embed_finish(y, stats, gamma, beta, pos, date, D, 0, xg, B, D, L, E, tok_off, Lg)
    yr = y.clone().requires_grad_(True)
    gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    img = yr.reshape(B * D, L, E)
    mu = img.mean(dim=(1, 2), keepdim=True)
    var = ((img - mu) ** 2).mean(dim=(1, 2), keepdim=True)
    z = (img - mu) / torch.sqrt(var + 1e-5) * gr + br
    dpad = torch.cat([torch.zeros(B * D, E - 8, device=dev), date], dim=1)[:, None, :]
    want = (z + pos[None] + dpad).reshape(B, D * L, E)
    got = xg[:, tok_off:tok_off + D * L]
    assert (got - want).abs().max() < 2e-4
    assert (xg[:, :tok_off] == 5).all() and (xg[:, tok_off + D * L:] == 5).all()
    # backward
    dxg = torch.zeros(B, Lg, E, device=dev)
    dxg[:, tok_off:tok_off + D * L] = _rand(B, D * L, E, seed=6).to(dev) * (torch.rand(B, D * L, 1, device=dev) < 0.3)
    dyc = torch.zeros(B * D * L, E, device=dev, dtype=torch.bfloat16)
    dg, db = torch.zeros(E, device=dev), torch.zeros(E, device=dev)
    sums = torch.zeros(B * D, 2, device=dev)
    hip.embed_finish_bwd(dxg, y, stats, gamma, dyc, dg, db, sums, B, D, L, E, tok_off, Lg)
    want.backward(dxg[:, tok_off:tok_off + D * L])
    scale = yr.grad.abs().max().item()
    assert (dyc.float() - yr.grad).abs().max() < 2e-2 * scale
    assert (dg - gr.grad).abs().max() < 1e-3 * max(1, gr.grad.abs().max().item())
    assert (db - br.grad).abs().max() < 1e-3 * max(1, br.grad.abs().max().item())


def test_date_features_and_rescale(dev):
    from maestro_amd import hip
    from oracle import layers as ol
    dates = torch.tensor([[[2019, 100, 10], [2020, 3, 23], [2018, 365, 0]],
                          [[2021, 200, 12], [2019, 182, 0], [2017, 1, 5]]], dtype=torch.int16)
    ref = torch.tensor([[[2019, 182, 0]], [[2020, 1, 0]]], dtype=torch.int16)
    out = torch.zeros(2, 5, 8, device=dev)
    hip.date_features(dates.to(dev), ref.to(dev), out, 2, 3, 5, 2, 0.5)
    want = ol.date_features(dates, ref, 0.5)
    assert (out[:, 2:].cpu() - want).abs().max() < 2e-6 and (out[:, :2] == 0).all()
    img = torch.rand(3, 2, 8, 8)
    res = torch.zeros(3, 2, 8, 8, device=dev)
    hip.rescale_elev(img.to(dev), res, 3, 2, 8)
    ref_img = img.clone()
    ref_img[:, 1:] = 30 * (ref_img[:, :1] - ref_img[:, 1:])
    assert torch.equal(res.cpu(), ref_img)


@pytest.mark.parametrize("mode,name", [(0, "nearest"), (1, "bilinear"), (2, "bicubic")])
@pytest.mark.parametrize("hin,hout", [(32, 64), (64, 64), (100, 60), (6, 10), (37, 128)])
def test_resize_matches_torch_interpolate(dev, mode, name, hin, hout):
    from maestro_amd import hip
    x = torch.rand(3, 2, hin, hin, generator=torch.Generator().manual_seed(hin))
    out = torch.zeros(3, 2, hout, hout, device=dev)
    hip.resize(x.to(dev), out, 6, hin, hin, hout, hout, mode)
    want = F.interpolate(x, size=(hout, hout), mode=name)
    if mode == 0:
        assert torch.equal(out.cpu(), want)
    else:
        assert (out.cpu() - want).abs().max() < (2e-6 if mode == 1 else 5e-6)


def test_depatchify(dev):
    from maestro_amd import hip
    from oracle import mae as om
    BD, C, S, P = 3, 4, 32, 8
    img = torch.rand(BD, C, S, S)
    patches = om.patch_view(img[None], S // P).reshape(-1, P * P * C).to(dev)
    out = torch.zeros(BD, C, S, S, device=dev)
    hip.depatchify(patches, out, BD, C, S, P)
    assert torch.equal(out.cpu(), img)


# ----------------------------------------------------------------------------------------------- masking
@pytest.mark.parametrize("p_struct", [0.45, 0.9])
@pytest.mark.parametrize("B,L,k", [(4, 64, 48), (3, 1024, 768), (2, 225, 169), (5, 400, 300), (2, 72, 54), (2, 2501, 1876), (3, 1030, 772)])
def test_mask_select_matches_oracle(dev, B, L, k, p_struct):
    """``p_struct = 0.9``: more structurally masked tokens than k in every row -- the tie-heavy regime of SURVEY Q5 (the
    noise of those tokens is exactly 0): the build's semantics are the STABLE ones, ties resolve to ascending index."""
    from maestro_amd import hip
    g = torch.Generator().manual_seed(L)
    noise = torch.rand(B, L, generator=g)
    struct = torch.rand(B, L, generator=g) < p_struct
    if p_struct > 0.8:
        assert (struct.sum(1) > k).all()
    vis = torch.zeros(B, L - k, dtype=torch.int32, device=dev)
    msk = torch.zeros(B, k, dtype=torch.int32, device=dev)
    inv = torch.zeros(B, L, dtype=torch.int32, device=dev)
    mask = torch.zeros(B, L, dtype=torch.uint8, device=dev)
    hip.mask_select(noise.to(dev), struct.to(torch.uint8).to(dev), vis, msk, inv, mask, B, L, k)
    nz = noise * (1 - struct.float())
    order = torch.argsort(nz, dim=-1, stable=True)  # oracle semantics (oracle/mae.py mask_indices)
    want_m = order[:, :k].sort(dim=1).values
    want_v = order[:, k:].sort(dim=1).values
    assert torch.equal(msk.cpu().long(), want_m) and torch.equal(vis.cpu().long(), want_v)
    want_mask = torch.zeros(B, L, dtype=torch.bool).scatter_(1, want_m, True)
    assert torch.equal(mask.cpu().bool(), want_mask)
    pos = torch.full((B, L), -1, dtype=torch.long).scatter_(1, want_v, torch.arange(L - k).expand(B, -1))
    assert torch.equal(inv.cpu().long(), pos)


def test_gather_scatter_unmask(dev):
    from maestro_amd import hip
    B, L, n, dim, dst_L, off = 3, 40, 10, 64, 25, 7
    src = _rand(B, L, dim, seed=1).to(dev)
    idx = torch.stack([torch.randperm(L, generator=torch.Generator().manual_seed(b))[:n].sort().values for b in range(B)])
    idx32 = idx.to(torch.int32).to(dev)
    dst = torch.zeros(B, dst_L, dim, device=dev)
    hip.gather_rows(src, idx32, dst, B, L, n, dim, dst_L, off)
    want = src[torch.arange(B)[:, None], idx.to(dev)]
    assert torch.equal(dst[:, off:off + n], want) and (dst[:, :off] == 0).all()
    back = torch.zeros(B, L, dim, device=dev)
    hip.scatter_rows(dst, idx32, back, B, L, n, dim, dst_L, off)
    ref = torch.zeros(B, L, dim, device=dev)
    ref[torch.arange(B)[:, None], idx.to(dev)] = want
    assert torch.equal(back, ref)
    # the same transpose as a gather over every destination row (no pre-zeroed destination needed)
    inv_map = torch.full((B, L), -1, dtype=torch.int32)
    for b in range(B):
        inv_map[b, idx[b]] = torch.arange(n, dtype=torch.int32)
    garbage = torch.full((B, L, dim), float("nan"), device=dev)
    hip.expand_rows(want.contiguous(), inv_map.to(dev), garbage, B, L, n, dim)
    assert torch.equal(garbage, ref)
    # unmask assemble: two modality slots, date rows
    Dd, n_vis = 32, n
    y = _rand(B, n_vis, Dd, seed=2).to(dev)
    inv = torch.full((B, L), -1, dtype=torch.int32)
    for b in range(B):
        inv[b, idx[b]] = torch.arange(n, dtype=torch.int32)
    tok = _rand(2, Dd, seed=3).to(dev)
    slot = (torch.arange(L) >= 24).to(torch.int32).to(dev)
    pos = _rand(L, Dd, seed=4).to(dev)
    date = _rand(B, 5, 8, seed=5).to(dev)
    drow = (torch.arange(L) % 5).to(torch.int32).to(dev)
    xdec = torch.zeros(B, L, Dd, device=dev)
    hip.unmask_assemble(y, inv.to(dev), tok, slot, pos, date, drow, 5, xdec, B, L, n_vis, Dd)
    ref = tok[slot.long()][None].repeat(B, 1, 1)
    ref[torch.arange(B)[:, None], idx.to(dev)] = y
    ref = ref + pos[None]
    ref[:, :, Dd - 8:] += date[:, drow.long()]
    assert (xdec - ref).abs().max() < 1e-6
    mask = (inv < 0).to(torch.uint8).to(dev)
    dtok = torch.zeros(2, Dd, device=dev)
    dx = _rand(B, L, Dd, seed=6).to(dev)
    hip.unmask_token_grad(dx, mask, slot, dtok[0], B, L, Dd, 0, 0, 24)
    hip.unmask_token_grad(dx, mask, slot, dtok[1], B, L, Dd, 1, 24, L)
    m = mask.bool()
    want0 = (dx * (m & (slot == 0)[None])[:, :, None]).sum((0, 1))
    want1 = (dx * (m & (slot == 1)[None])[:, :, None]).sum((0, 1))
    assert (dtok[0] - want0).abs().max() < 1e-4 and (dtok[1] - want1).abs().max() < 1e-4
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    hip.count_masked(mask, B, L, 24, L, cnt)
    assert cnt.item() == int(m[:, 24:].sum())


# ----------------------------------------------------------------------------------------------- loss
@pytest.mark.parametrize("p", [1, 2])
@pytest.mark.parametrize("B,Lm,Lg,off,PPC", [(2, 16, 16, 0, 1024), (3, 36, 72, 36, 8), (2, 400, 400, 0, 40)])
def test_masked_loss(dev, p, B, Lm, Lg, off, PPC):
    from maestro_amd import hip
    rec = _rand(B * Lm, PPC, seed=1).to(dev).requires_grad_(True)
    target = _rand(B * Lm, PPC, seed=2).to(dev)
    mask_group = (torch.rand(B, Lg, generator=torch.Generator().manual_seed(3)) < 0.7).to(torch.uint8).to(dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    hip.count_masked(mask_group, B, Lg, off, off + Lm, cnt)
    acc = torch.zeros(1, device=dev)
    drec = torch.full((B * Lm, PPC), 9.0, device=dev, dtype=torch.bfloat16)
    weight = 0.37
    hip.masked_loss(rec.detach(), target, mask_group, cnt, weight, acc, drec, B, Lm, Lg, off, PPC, p)
    m = mask_group[:, off:off + Lm].reshape(-1).bool()
    err = (target - rec).abs() if p == 1 else (target - rec) ** 2
    want = weight * err[m].mean()
    want.backward()
    assert abs(acc.item() - want.item()) < 1e-5 * max(1, abs(want.item()))
    scale = rec.grad.abs().max().item()
    assert (drec.float() - rec.grad).abs().max() < 1e-2 * scale


@pytest.mark.parametrize("P", [8, 16])       # 16: the one-wave-per-patch kernel (channel windows, rescale against channel 0 of the raster)
@pytest.mark.parametrize("elev", [False, True])
@pytest.mark.parametrize("sizes", [(2, 2), (3, 1), (1, 1, 2)])
def test_patchify_and_loss_over_band_groups(dev, sizes, elev, P):  # noqa: N803
    """Several band-groups per modality (``mh_patchify_bands`` / ``mh_count_masked_elems`` / ``mh_masked_loss_bands``):
    every band-group's im2col rows are the window of the plain kernel's rows, the elevation rescale refers to channel 0 of the
    RASTER, and the modality's loss is ONE mean over the masked elements of all its band-groups, each group's reconstruction
    compared with its (strided) window of the modality-level target."""
    from maestro_amd import hip
    from oracle import layers as ol
    BD, S, C = 3, 32, sum(sizes)  # noqa: N806
    g, PP = S // P, P * P  # noqa: N806
    T = BD * g * g  # noqa: N806
    img = torch.rand(BD, C, S, S, generator=torch.Generator().manual_seed(11))
    ref_img = img.clone()
    if elev:
        ref_img[:, 1:] = 30 * (ref_img[:, :1] - ref_img[:, 1:])
    nb = torch.tensor([1, C - 1], dtype=torch.int32, device=dev)          # norm groups straddling the band-groups
    K = C * PP  # noqa: N806
    target = torch.zeros(T, K, device=dev)
    want_t = torch.zeros(T, K, device=dev)
    cols_full = torch.zeros(T, (K + 31) // 32 * 32, device=dev, dtype=torch.bfloat16)
    hip.patchify_bands(img.to(dev), None, target, BD, C, 0, C, S, P, (K + 7) // 8 * 8, nb, 2, True, elev)
    hip.patchify(img.to(dev), cols_full, want_t, BD, C, S, P, cols_full.shape[1], nb, 2, True, elev)
    assert torch.equal(target, want_t)                                       # target-only mode = the plain kernel's target
    Lg, off = g * g * len(sizes) + 5, 3  # noqa: N806
    mask = (torch.rand(BD, Lg, generator=torch.Generator().manual_seed(5)) < 0.6).to(torch.uint8).to(dev)
    cnt, acc, weight = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, device=dev), 0.41
    recs, drecs, c0, tot, n_el = [], [], 0, 0.0, 0
    for gi, n_g in enumerate(sizes):
        Kg = n_g * PP  # noqa: N806
        cols = torch.full((T, (Kg + 31) // 32 * 32), 3.0, device=dev, dtype=torch.bfloat16)
        hip.patchify_bands(img.to(dev), cols, None, BD, C, c0, n_g, S, P, cols.shape[1], None, 0, False, elev)
        want_cols = ol.im2col_patches(ref_img[:, c0: c0 + n_g], P).reshape(-1, Kg)
        assert torch.equal(cols[:, :Kg].cpu(), want_cols.bfloat16()) and (cols[:, Kg:] == 0).all()
        t_lo = off + gi * g * g
        hip.count_masked_elems(mask, BD, Lg, t_lo, t_lo + g * g, cnt, Kg, gi > 0)
        recs.append(_rand(T, Kg, seed=20 + gi).to(dev))
        drecs.append(torch.full((T, Kg), 9.0, device=dev, dtype=torch.bfloat16))
        c0 += n_g
    # every sample's band-group tokens sit at [off + gi * L, off + (gi + 1) * L) of its row of the group mask: the loss kernel
    # addresses them as "modality" rows b * L + t with tok_off = that start
    c0 = 0
    for gi, n_g in enumerate(sizes):
        Kg, t_lo = n_g * PP, off + gi * g * g  # noqa: N806
        hip.masked_loss_bands(recs[gi], target, mask, cnt, weight, acc, drecs[gi], BD, g * g, Lg, t_lo, Kg, 2, C, c0, n_g)
        m = mask[:, t_lo: t_lo + g * g].reshape(-1).bool().cpu()
        tw = target.view(T, PP, C)[:, :, c0: c0 + n_g].reshape(T, Kg).cpu()
        tot += float(((recs[gi].cpu() - tw) ** 2)[m].double().sum())
        n_el += int(m.sum()) * Kg
        c0 += n_g
    torch.cuda.synchronize()
    assert int(cnt) == n_el
    assert abs(acc.item() - weight * tot / n_el) < 1e-5 * max(1.0, weight * tot / n_el)
    c0 = 0
    for gi, n_g in enumerate(sizes):
        Kg, t_lo = n_g * PP, off + gi * g * g  # noqa: N806
        m = mask[:, t_lo: t_lo + g * g].reshape(-1).bool().cpu()
        tw = target.view(T, PP, C)[:, :, c0: c0 + n_g].reshape(T, Kg).cpu()
        want = 2 * (recs[gi].cpu() - tw) * weight / n_el * m[:, None]
        assert (drecs[gi].float().cpu() - want).abs().max() < 1e-2 * want.abs().max()
        c0 += n_g


# ----------------------------------------------------------------------------------------------- misc
def test_colsum_cast_pack_adamw(dev):
    from maestro_amd import hip
    M, N = 1000, 264
    x = _rand(M, N, seed=1).to(dev)
    out = torch.ones(N, device=dev)
    hip.colsum(x, out, M, N, N)
    assert (out - (1 + x.sum(0))).abs().max() < 1e-3
    xb = x.bfloat16()
    out.zero_()
    hip.colsum(xb, out, M, N, N)
    assert (out - xb.float().sum(0)).abs().max() < 1e-3
    n = 4099
    src = _rand(n, seed=2).to(dev)
    dst = torch.zeros(n, device=dev, dtype=torch.bfloat16)
    hip.cast_bf16(src, dst, n)
    assert torch.equal(dst, src.bfloat16())
    E, K, Kpad = 10, 40, 64
    w = _rand(E, K, seed=3).to(dev)
    wp = torch.ones(E, Kpad, device=dev, dtype=torch.bfloat16)
    hip.pack_rows_bf16(w, wp, E, K, Kpad)
    assert torch.equal(wp[:, :K], w.bfloat16()) and (wp[:, K:] == 0).all()
    acc = torch.ones(E, K, device=dev)
    hip.unpack_rows_add(wp.float().contiguous(), acc, E, K, Kpad)
    assert torch.equal(acc, 1 + w.bfloat16().float())
    # AdamW vs torch.optim.AdamW over 3 steps
    n = 4096
    p0 = _rand(n, seed=4).to(dev)
    p_ref = p0.clone().requires_grad_(True)
    opt = torch.optim.AdamW([p_ref], lr=1e-2, betas=(0.9, 0.99), weight_decay=0.01)
    p, m, v = p0.clone(), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    pb = torch.zeros(n, device=dev, dtype=torch.bfloat16)
    for step in range(1, 4):
        g = _rand(n, seed=10 + step).to(dev)
        p_ref.grad = g.clone()
        opt.step()
        hip.adamw(p, g, m, v, pb, n, 1e-2, 0.9, 0.99, 1e-8, 0.01, step)
    assert (p - p_ref.detach()).abs().max() < 1e-5
    assert torch.equal(pb, p.bfloat16())


def test_layernorm_partial_plus_batched_colsum_equals_fused_reduce():
    """``mh_layernorm_bwd_partial`` + ``mh_colsum_batched`` (the per-segment batched form the engines use) give the same dx
    and the same dgamma / dbeta / dcol as ``mh_layernorm_bwd`` with its own reduce; a second job type (plain matrix) too."""
    from maestro_amd import hip
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(9)
    rows, dim = 403, 192                                      # ragged: not a multiple of the 16 rows per block
    x = torch.randn(rows, dim, generator=g).to(dev)
    dy = torch.randn(rows, dim, generator=g).to(dev).bfloat16()
    dres = torch.randn(rows, dim, generator=g).to(dev)
    gamma = torch.randn(dim, generator=g).to(dev)
    mean, rstd = x.mean(1), (x.var(1, unbiased=False) + 1e-5).rsqrt()
    n_ws = hip.layernorm_bwd_workspace(rows, dim)
    ws_a, ws_b = torch.empty(n_ws, device=dev), torch.full((n_ws,), float("nan"), device=dev)
    dx_a, dx_b = torch.empty_like(x), torch.empty_like(x)
    dg_a, db_a, dc_a = (torch.zeros(dim, device=dev) for _ in range(3))
    hip.layernorm_bwd(dy, rows, 0, x, rows, 0, gamma, mean, rstd, dres, dx_a, None, dg_a, db_a, dc_a, ws_a, 1, rows, dim)
    hip.layernorm_bwd_partial(dy, rows, 0, x, rows, 0, gamma, mean, rstd, dres, dx_b, None, ws_b, 1, rows, dim)
    nblk = n_ws // (3 * dim)
    dg_b, db_b, dc_b = (torch.full((dim,), 0.5, device=dev) for _ in range(3))        # += semantics: starts at 0.5
    mat = torch.randn(37, 100, generator=g).to(dev)
    msum = torch.zeros(64, device=dev)
    flat = ws_b.view(-1)
    batch = hip.ColsumBatch([(flat, dg_b, nblk, dim, 3 * dim), (flat[dim:], db_b, nblk, dim, 3 * dim),
                             (flat[2 * dim:], dc_b, nblk, dim, 3 * dim), (mat, msum, 37, 64, 100)], dev)
    batch.launch()
    torch.cuda.synchronize()
    assert torch.equal(dx_a, dx_b)
    for a, b in ((dg_a, dg_b), (db_a, db_b), (dc_a, dc_b)):
        assert torch.allclose(a + 0.5, b, rtol=1e-5, atol=1e-4), (a - b + 0.5).abs().max()
    assert torch.allclose(msum, mat[:, :64].sum(0), rtol=1e-5, atol=1e-5)
    with pytest.raises(hip.HipExtensionError):
        hip.ColsumBatch([(mat, msum, 37, 128, 100)], dev)                              # cols > ld
