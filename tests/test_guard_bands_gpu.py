"""Every kernel entry point on operands that sit INSIDE poisoned storage (tests/guards.py): NaN bands in front of and behind every
input and output, NaN pad columns between the rows of every matrix that has a leading dimension, ragged shapes, row maps with
offsets, slices of flat buffers.  After each call: (a) the result equals the reference of the kernel's existing test under that
test's tolerance (named in a comment at each compare), (b) it is finite, (c) every band and pad of every buffer, inputs
included, kept its bits.  A store past an output or a load past an input that is only "masked" by arithmetic (0 * NaN) fails here;
in the dense, exactly-sized allocations of the other kernel tests both are silent.

Every size, offset and index passed is in range: only a kernel's own error can leave a view, and the bands (>= 256 rows) keep
such an error inside the test's allocation.
"""

import os

import pytest
import torch
import torch.nn.functional as F  # noqa: N812

from tests.guards import GuardSet, bits_equal

pytestmark = pytest.mark.gpu
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _in_map(rows_total, off, n, data, B):  # noqa: N803
    """[B, rows_total, dim] of NaN with ``data`` [B, n, dim] at rows [off, off + n): the rows of a sequence that belong to others."""
    full = torch.full((B, rows_total, data.shape[-1]), NAN, dtype=data.dtype)
    full[:, off:off + n] = data
    return full


def _outside(t, off, n):
    """The rows of a [B, L, dim] view that the row map (off, n) does not address."""
    return torch.cat([t[:, :off], t[:, off + n:]], dim=1)


def _note(line: str) -> None:
    """Which GEMM tile x layout x leading-dimension combinations were served / declined: printed (``pytest -s`` shows it), and
    appended to the file ``MAESTRO_GUARD_NOTES`` names when that is set (profiles/guard_bands.md was written from such a file)."""
    print(line)
    path = os.environ.get("MAESTRO_GUARD_NOTES")
    if path:
        try:
            with open(path, "a") as f:
                f.write(line + "\n")
        except OSError:
            pass


# ----------------------------------------------------------------------------------------------- bf16 GEMM
_TILES = {"REG_128": 0, "REG_64": 13, "REG_192": 14, "PP_128": 7, "DMA_256": 1, "DMA_256x128": 2, "DMA_128x256": 3, "DMA_128": 4,
          "DMA_128x4": 5, "SK_192": 15, "SK_256": 16, "SK_DMA_256": 17}
_EPILOGUES = ("bf16", "f32_bias_res", "gelu_u8", "mulaux_u8_colsum", "atomic_slice")
# fully ragged (M, N off every tile; K = 104: a K tail for the K-minor operands) / multi-tile, ragged M only: what the ping-pong,
# LDS-DMA and stream-K tiles serve (N % 256 == 0, K % 64 == 0, K >= 512)
_SHAPES = [(200, 72, 104), (1000, 256, 512), (40, 8, 64)]      # (the last: M below a wave tile, N one vector wide)
_SHAPE_TN_KTAIL = (264, 200, 1001)          # K = tokens, a multiple of nothing: the K tail of the K-major operands


def _gemm_guarded(dev, tile, layout, M, N, K, pad, epi):  # noqa: N803
    """One guarded launch; returns 0 (served, verified) or the library's negative code (declined, outputs verified untouched)."""
    from maestro_amd import hip
    from tests.test_gemm_gpu import _operands
    integer = epi in ("bf16", "f32_bias_res", "atomic_slice")      # integer-valued operands: exact results (test_gemm_exact_integers)
    A, B, want = _operands(layout, M, N, K, dev, integer=integer)  # noqa: N806
    gs = GuardSet(dev)
    a = gs.inp(A, ld=A.shape[1] + pad, name="A")
    b = gs.inp(B, ld=B.shape[1] + pad, name="B")
    g = torch.Generator().manual_seed(5)
    bias = res = aux_in = aux_out = colsum = None
    ldr = ldaux = 0
    ldc = N + pad
    neighbours = None
    if epi == "bf16":
        flags, C = 0, gs.out((M, N), torch.bfloat16, ld=ldc, name="C")  # noqa: N806
    elif epi == "f32_bias_res":
        flags = hip.OUT_F32 | hip.BIAS | hip.RESIDUAL
        bias = gs.inp(torch.randint(-4, 5, (N,), generator=g).float(), name="bias")
        res = gs.inp(torch.randint(-9, 10, (M, N), generator=g).float(), ld=N + pad, name="res")
        ldr = N + pad
        C = gs.out((M, N), torch.float32, ld=ldc, name="C")  # noqa: N806
    elif epi == "gelu_u8":
        flags = hip.BIAS | hip.GELU | hip.AUX_DGELU | hip.AUX_U8
        bias = gs.inp(torch.randn(N, generator=g), name="bias")
        C = gs.out((M, N), torch.bfloat16, ld=ldc, name="C")  # noqa: N806
        ldaux = N + pad                                                   # bytes
        aux_out = gs.out((M, N), torch.uint8, ld=ldaux, name="aux_out")
    elif epi == "mulaux_u8_colsum":
        flags = hip.MULAUX | hip.AUX_U8 | hip.COLSUM
        ldaux = N + pad
        aux_in = gs.inp(torch.randint(0, 253, (M, N), generator=g, dtype=torch.uint8), ld=ldaux, name="aux_in")
        C = gs.out((M, N), torch.bfloat16, ld=ldc, name="C")  # noqa: N806
        colsum = gs.out(((M + 63) // 64, N), torch.float32, name="colsum")
    else:
        # the ParamStore situation: C is a slice between two other "weights" of ONE flat gradient buffer, accumulated atomically
        flags, ldc = hip.OUT_F32 | hip.ATOMIC, N
        n0, n1 = 68, 100
        store = gs.out((n0 + M * N + n1,), torch.float32, name="gradient store")
        store[:n0] = torch.arange(n0, device=dev).float() + 0.5
        store[n0 + M * N:] = -torch.arange(n1, device=dev).float() - 0.25
        C = store[n0: n0 + M * N].view(M, N)  # noqa: N806
        C.fill_(1.0)
        neighbours = (store[:n0], store[n0 + M * N:])
    outs = [t for t in (C, aux_out, colsum) if t is not None] + list(neighbours or ())
    before = [t.clone() for t in outs]
    rc = hip._gemm_tile(tile, layout, M, N, K, a, a.stride(0), b, b.stride(0), C, ldc, flags, bias, res, ldr, aux_in, aux_out, ldaux,
                        colsum)
    gs.check()
    if rc != 0:
        assert rc < 0, f"launch error {rc}: {hip.lib().mh_last_error()}"
        for t, t0 in zip(outs, before):                                   # declined = nothing launched: not one output bit moved
            assert bits_equal(t, t0), "a declined problem changed its output"
        return rc
    if epi == "bf16":
        assert torch.equal(C, want.bfloat16())                            # exact: test_gemm_exact_integers
    elif epi == "f32_bias_res":
        assert torch.equal(C, want + bias + res)                          # exact: test_gemm_pp_exact_integers
    elif epi == "gelu_u8":
        pre = (want + bias).requires_grad_(True)
        act = F.gelu(pre)
        act.sum().backward()
        assert torch.isfinite(C.float()).all()
        assert (C.float() - act.detach()).abs().max() < 2e-2              # test_gemm_epilogues
        dec = aux_out.float() / 200.0 - 0.13
        # test_gemm_epilogues bounds the bf16 derivative by 1e-2 against GELU'(x); test_saved_gelu_derivative_as_bytes bounds
        # the decoded byte by 0.0025 + 2^-8 * 1.13 + 1e-6 against that bf16 value: their sum bounds the byte against GELU'(x)
        assert (dec - pre.grad).abs().max() < 1e-2 + 0.0025 + 2 ** -8 * 1.13 + 1e-6
    elif epi == "mulaux_u8_colsum":
        prod = want * (aux_in.float() / 200.0 - 0.13)
        assert torch.isfinite(C.float()).all() and torch.isfinite(colsum).all()
        assert ((C.float() - prod).abs().max() / prod.abs().max()).item() < 1e-2          # test_gemm_epilogues (MULAUX)
        blocks = torch.zeros(((M + 63) // 64) * 64, N, device=dev)
        blocks[:M] = prod
        ref = blocks.view(-1, 64, N).sum(1)
        assert (colsum - ref).abs().max() <= 2e-2 * ref.abs().max()       # test_saved_gelu_derivative_as_bytes (column sums)
    else:
        assert torch.equal(C, want + 1.0)                                 # exact: test_gemm_split_k_atomic
        assert bits_equal(neighbours[0], before[-2]) and bits_equal(neighbours[1], before[-1]), "a neighbouring weight's gradient changed"
    return 0


@pytest.mark.parametrize("tile_name", list(_TILES))
def test_gemm_tiles_on_strided_ragged_operands(dev, tile_name):
    """Every tile x layout x epilogue with ld = cols + 8 and cols + 40 on A, B, C, res, aux; at least one strided, ragged-M problem
    must be SERVED by every tile (a decline passes only with untouched outputs)."""
    tile = _TILES[tile_name]
    served = 0
    for layout in (0, 1, 2):
        shapes = _SHAPES + ([_SHAPE_TN_KTAIL] if layout == 2 else [])
        for (M, N, K) in shapes:  # noqa: N806
            for pad in (8, 40):
                for epi in _EPILOGUES:
                    rc = _gemm_guarded(dev, tile, layout, M, N, K, pad, epi)
                    served += rc == 0
                    _note(f"{tile_name:12s} {'NT NN TN'.split()[layout]} ({M}, {N}, {K}) ld+{pad:<2d} {epi:17s} "
                          f"{'served' if rc == 0 else f'declined ({rc})'}")
    assert served > 0, f"{tile_name} served no strided, ragged-M problem"


def test_gemm_library_rule_on_strided_operands(dev):
    """``mh_gemm_bf16`` itself (MH_TILE_AUTO) on the same guarded operands, called by name through the C ABI."""
    from maestro_amd import hip
    from tests.test_gemm_gpu import _operands
    for layout, (M, N, K) in [(0, (200, 72, 104)), (1, (1000, 256, 512)), (2, (264, 200, 1001))]:  # noqa: N806
        A, B, want = _operands(layout, M, N, K, dev, integer=True)  # noqa: N806
        gs = GuardSet(dev)
        a, b = gs.inp(A, ld=A.shape[1] + 8, name="A"), gs.inp(B, ld=B.shape[1] + 40, name="B")
        C = gs.out((M, N), torch.float32, ld=N + 12, name="C")  # noqa: N806
        z = hip.ptr(None)
        rc = hip.lib().mh_gemm_bf16(layout, M, N, K, hip.ptr(a), a.stride(0), hip.ptr(b), b.stride(0), hip.ptr(C), N + 12, hip.OUT_F32,
                                    z, z, 0, z, z, 0, z, hip.stream())
        assert rc == 0, hip.lib().mh_last_error()
        gs.check()
        assert torch.equal(C, want)                                       # exact: test_gemm_exact_integers


def test_grouped_tn_outputs_are_adjacent_slices(dev):
    """``mh_gemm_grouped_tn``: the weight gradients of three problems are neighbouring slices of one flat buffer, with other
    "weights" between them; operands strided (lda = M + 8, ldb = N + 40), K ragged."""
    from maestro_amd import hip
    probs = [(264, 200, 1001), (72, 136, 300), (256, 256, 64)]
    gs = GuardSet(dev)
    gaps = [36, 4, 100, 12]
    total = sum(gaps) + sum(m * n for m, n, _ in probs)
    store = gs.out((total,), torch.float32, name="gradient store")
    g = torch.Generator().manual_seed(3)
    table, wants, gap_views, o = [], [], [], 0
    for i, (M, N, K) in enumerate(probs):  # noqa: N806
        gap_views.append(store[o: o + gaps[i]])
        gap_views[-1].copy_(torch.arange(gaps[i]).float() + 0.5 + i)
        o += gaps[i]
        C = store[o: o + M * N].view(M, N)  # noqa: N806
        o += M * N
        a = torch.randint(-3, 4, (K, M), generator=g).float().bfloat16()
        b = torch.randint(-2, 3, (K, N), generator=g).float().bfloat16()
        A, B = gs.inp(a, ld=M + 8, name=f"A{i}"), gs.inp(b, ld=N + 40, name=f"B{i}")  # noqa: N806
        table.append((A, B, C, M, N, K, M + 8, N + 40, N))
        wants.append((C, a.float().t().to(dev) @ b.float().to(dev)))
    gap_views.append(store[o:])
    gap_views[-1].fill_(-7.5)
    before = [v.clone() for v in gap_views]
    hip.GroupedTN(table, dev).launch()
    gs.check()
    for C, want in wants:  # noqa: N806
        assert torch.equal(C, want)                                       # exact: test_grouped_tn_exact_and_timed
    for v, v0 in zip(gap_views, before):
        assert bits_equal(v, v0), "a weight between two gradient slices changed"


# ----------------------------------------------------------------------------------------------- attention
@pytest.mark.parametrize("D", [32, 64])
@pytest.mark.parametrize("N", [33, 100, 129, 257])
@pytest.mark.parametrize("B", [1, 2])
def test_attention_between_nan_bands(dev, B, N, D):  # noqa: N803
    """The last KV and Q tiles are partial: the rows past N of the last batch are the NaN back band.  Probabilities of keys >= N
    are zero, so their V rows must not reach the product (0 * NaN).  Tolerances: test_attention_fwd_bwd."""
    from maestro_amd import hip
    from tests.test_kernels_gpu import _attn_ref
    H = 2  # noqa: N806
    scale = D ** -0.5
    gs = GuardSet(dev)
    qkv_h = (_rand(B, N, 3, H, D, seed=N + D) * 1.5).bfloat16()
    qkv = gs.inp(qkv_h.view(B * N, 3 * H * D), name="qkv").view(B, N, 3, H, D)
    out = gs.out((B * N, H * D), torch.bfloat16, name="out").view(B, N, H * D)
    lse = gs.out((B * H, N), torch.float32, name="lse").view(B, H, N)
    hip.attn_fwd(qkv, out, lse, B, N, H, D, scale)
    gs.check()
    ref = qkv_h.to(dev).float().requires_grad_(True)
    want, want_lse = _attn_ref(ref, scale)
    assert torch.isfinite(out.float()).all() and torch.isfinite(lse).all()
    assert (out.float() - want).abs().max() < 3e-2
    assert (lse - want_lse).abs().max() < 5e-3
    dout_h = _rand(B, N, H * D, seed=7).bfloat16()
    dout = gs.inp(dout_h.view(B * N, H * D), name="dout").view(B, N, H * D)
    delta = gs.out((B * H, N), torch.float32, name="delta").view(B, H, N)
    dqkv = gs.out((B * N, 3 * H * D), torch.bfloat16, name="dqkv").view(B, N, 3, H, D)
    gs.arm()                                   # out and lse are inputs now: the backward must not change them
    for gd in gs.guards:
        gd.whole = gd.name not in ("delta", "dqkv")
    hip.attn_bwd(qkv, out, dout, lse, delta, dqkv, B, N, H, D, scale)
    gs.check()
    want.backward(dout_h.to(dev).float())
    assert torch.isfinite(dqkv.float()).all() and torch.isfinite(delta).all()
    err = (dqkv.float() - ref.grad).abs().max().item()
    assert err < 3e-2 * max(1.0, ref.grad.abs().max().item()), err
    for i, name in enumerate("qkv"):
        got, ref_i = dqkv[:, :, i].float(), ref.grad[:, :, i]
        rel = ((got - ref_i).norm() / ref_i.norm()).item()
        assert rel < 1.5e-2, (name, rel)
    want_delta = (out.float() * dout.float()).reshape(B, N, H, D).sum(-1).permute(0, 2, 1)
    assert (delta - want_delta).abs().max() < 1e-3 * max(1.0, want_delta.abs().max().item())


# ----------------------------------------------------------------------------------------------- LayerNorm
# 21 rows (not a multiple of 4) / 12 rows (of 4, not of 16) / 111 and 68 rows: several 16-row blocks, the last one partial
@pytest.mark.parametrize("B,n", [(3, 7), (2, 6), (3, 37), (2, 34)])
@pytest.mark.parametrize("dim", [192, 256, 384, 768, 1024, 2048])
def test_layernorm_row_maps_between_nan_rows(dev, dim, B, n):  # noqa: N803
    """Forward (bf16, f32, fp8 and MX outputs) and both backwards with x_off, y_off > 0 and L > off + n: the rows of the sequence
    that belong to other modalities are NaN on the input side and must keep their bits on the output side.  dim = 2048 is the
    NV = 8 instantiation.  Tolerances: test_layernorm_fwd_bwd; fp8 codes: test_layernorm_fp8_output; MX: the rule (mx_ref)."""
    from maestro_amd import hip
    from tests.test_mx_gpu import mx_ref
    xoff, yoff = 3, 5
    xL, yL = xoff + n + 2, yoff + n + 4  # noqa: N806
    gs = GuardSet(dev)
    xs_h = _rand(B, n, dim, seed=1) * 2 + 0.5
    x = gs.inp(_in_map(xL, xoff, n, xs_h, B), name="x")
    gamma, beta = gs.inp(1 + 0.2 * _rand(dim, seed=2), name="gamma"), gs.inp(0.1 * _rand(dim, seed=3), name="beta")
    xs = xs_h.to(dev).requires_grad_(True)
    g_ref, b_ref = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    want = F.layer_norm(xs, (dim,), g_ref, b_ref, 1e-5)
    ref64 = F.layer_norm(xs_h.double(), (dim,), gamma.cpu().double(), beta.cpu().double()).float()
    mean, rstd = gs.out((B * n,), name="mean"), gs.out((B * n,), name="rstd")
    ys = {}
    for out_f32 in (False, True):
        y = gs.out((B, yL, dim), torch.float32 if out_f32 else torch.bfloat16, name="y")
        y0 = y.clone()
        hip.layernorm_fwd(x, xL, xoff, gamma, beta, y, yL, yoff, mean, rstd, B, n, dim)
        gs.check()
        got = y[:, yoff:yoff + n].float()
        assert torch.isfinite(got).all() and torch.isfinite(mean).all() and torch.isfinite(rstd).all()
        assert (got - want).abs().max() < (1e-5 if out_f32 else 3e-2)
        assert bits_equal(_outside(y, yoff, n), _outside(y0, yoff, n)), "rows outside the map were written"
        ys[out_f32] = y
    # fp8 copy (per-tensor scale): same bf16 y, codes within one of torch's conversion, absmax recorded
    y = gs.out((B, yL, dim), torch.bfloat16, name="y (fp8 call)")
    y8 = gs.out((B, yL, dim), torch.uint8, fill="fp8", align=4, name="y8")
    scale, amax = gs.inp(torch.tensor([16.0]), name="y8_scale"), gs.out((hip.AMAX_PITCH,), init=0.0, name="y8_amax")
    y0, y80 = y.clone(), y8.clone()
    hip.layernorm_fwd_fp8(x, xL, xoff, gamma, beta, y, yL, yoff, mean, rstd, B, n, dim, y8, scale, amax)
    gs.check()
    assert bits_equal(y[:, yoff:yoff + n], ys[False][:, yoff:yoff + n])
    assert bits_equal(_outside(y, yoff, n), _outside(y0, yoff, n)) and bits_equal(_outside(y8, yoff, n), _outside(y80, yoff, n))
    want8 = (ref64 * 16.0).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8).int()
    diff = (y8[:, yoff:yoff + n].cpu().int() - want8).abs()
    assert int(diff.max()) <= 1 and float((diff != 0).float().mean()) < 2e-3
    assert abs(float(amax.max()) - float(ref64.abs().max())) < 1e-4 * float(ref64.abs().max())
    # MX copy: y8 and its E8M0 scales (pitch above dim / 32) are the MX rule applied to the bf16 output
    y = gs.out((B, yL, dim), torch.bfloat16, name="y (mx call)")
    y8 = gs.out((B, yL, dim), torch.uint8, fill="fp8", align=4, name="y8 (mx)")
    ld_s = (dim // 32 + 3) // 4 * 4 + 4
    y8s = gs.out((B, yL, dim // 32), torch.uint8, ld=ld_s, fill="e8m0", align=4, name="y8_scales")
    y0, y80, y8s0 = y.clone(), y8.clone(), y8s.clone()
    hip.layernorm_fwd_mx(x, xL, xoff, gamma, beta, y, yL, yoff, mean, rstd, B, n, dim, y8, y8s, ld_s)
    gs.check()
    assert bits_equal(y[:, yoff:yoff + n], ys[False][:, yoff:yoff + n])
    q, s, finite = mx_ref(y[:, yoff:yoff + n].reshape(B * n, dim))
    assert bool(finite.all())
    assert torch.equal(y8[:, yoff:yoff + n].reshape(B * n, dim).cpu(), q) and torch.equal(y8s[:, yoff:yoff + n].reshape(B * n, -1).cpu(), s)
    for t, t0 in ((y, y0), (y8, y80), (y8s, y8s0)):
        assert bits_equal(_outside(t, yoff, n), _outside(t0, yoff, n))
    # backward: fused reduce and per-block partial rows
    dy_h = _rand(B, n, dim, seed=4)
    dres_h = _rand(B, n, dim, seed=5)
    dres = gs.inp(_in_map(xL, xoff, n, dres_h, B), name="dres")
    n_ws = hip.layernorm_bwd_workspace(B * n, dim)
    for dy_f32 in (False, True):
        dy_m = dy_h if dy_f32 else dy_h.bfloat16()
        dy = gs.inp(_in_map(yL, yoff, n, dy_m, B), name="dy")
        if xs.grad is not None:
            xs.grad, g_ref.grad, b_ref.grad = None, None, None
        F.layer_norm(xs, (dim,), g_ref, b_ref, 1e-5).backward(dy_m.to(dev).float())
        ref_dx = xs.grad + dres_h.to(dev)
        for partial in (False, True):
            dx, dxb = gs.out((B, xL, dim), name="dx"), gs.out((B, xL, dim), torch.bfloat16, name="dx_bf16")
            ws = gs.out((n_ws,), name="workspace")
            dx0, dxb0 = dx.clone(), dxb.clone()
            if partial:
                hip.layernorm_bwd_partial(dy, yL, yoff, x, xL, xoff, gamma, mean, rstd, dres, dx, dxb, ws, B, n, dim)
                gs.check()
                assert torch.isfinite(ws).all()
                dg, db, dc = ws.view(-1, 3 * dim).sum(0).view(3, dim)
                dc = dc + 1
            else:
                dg, db = gs.out((dim,), init=0.0, name="dgamma"), gs.out((dim,), init=0.0, name="dbeta")
                dc = gs.out((dim,), init=1.0, name="dcol")
                hip.layernorm_bwd(dy, yL, yoff, x, xL, xoff, gamma, mean, rstd, dres, dx, dxb, dg, db, dc, ws, B, n, dim)
                gs.check()
            assert torch.isfinite(dx[:, xoff:xoff + n]).all() and torch.isfinite(dxb[:, xoff:xoff + n].float()).all()
            assert (dx[:, xoff:xoff + n] - ref_dx).abs().max() < 2e-4
            assert (dxb[:, xoff:xoff + n].float() - ref_dx).abs().max() < 3e-2
            assert (dg - g_ref.grad).abs().max() < 2e-3 and (db - b_ref.grad).abs().max() < 2e-3
            assert (dc - (1 + ref_dx.sum((0, 1)))).abs().max() < 2e-3
            assert bits_equal(_outside(dx, xoff, n), _outside(dx0, xoff, n)) and bits_equal(_outside(dxb, xoff, n), _outside(dxb0, xoff, n))


# ----------------------------------------------------------------------------------------------- patch embed / staging
@pytest.mark.parametrize("BD,C,S,P,norm_bands,elev", [(5, 2, 6, 2, (1, 1), False), (2, 2, 64, 16, (2,), True), (2, 3, 48, 16, (3,), False)])
def test_patchify_guarded(dev, BD, C, S, P, norm_bands, elev):  # noqa: N803
    """``mh_patchify`` (references and tolerance: test_patchify) and ``mh_patchify_bands`` on a band window with c0 > 0
    (test_patchify_and_loss_over_band_groups)."""
    from maestro_amd import hip
    from oracle import layers as ol
    from oracle import mae as om
    img_h = torch.rand(BD, C, S, S, generator=torch.Generator().manual_seed(S))
    g, K = S // P, C * P * P  # noqa: N806
    Kpad = (K + 31) // 32 * 32 + 32  # noqa: N806
    ref_img = img_h.clone()
    if elev:
        ref_img[:, 1:] = 30 * (ref_img[:, :1] - ref_img[:, 1:])
    gs = GuardSet(dev)
    img = gs.inp(img_h, name="img")
    nb = gs.idx(torch.tensor(norm_bands, dtype=torch.int32), 1, name="norm_bands")        # (bands hold a harmless group size)
    cols = gs.out((BD * g * g, Kpad), torch.bfloat16, name="cols")
    target = gs.out((BD * g * g, K), name="target")
    hip.patchify(img, cols, target, BD, C, S, P, Kpad, nb, len(norm_bands), True, elev)
    gs.check()
    assert torch.equal(cols[:, :K].cpu(), ol.im2col_patches(ref_img, P).reshape(-1, K).bfloat16()) and (cols[:, K:] == 0).all()
    tgt = om.normalise_target(om.patch_view(ref_img[None], g), norm_bands)
    assert torch.isfinite(target).all() and (target.cpu() - tgt.reshape(-1, K)).abs().max() < 2e-4
    if C >= 2:                                    # one band-group: channels [c0, c0 + n_g) with c0 > 0, im2col rows only
        c0, n_g = 1, C - 1
        Kg = n_g * P * P  # noqa: N806
        Kgp = (Kg + 7) // 8 * 8 + 8  # noqa: N806
        cols_g = gs.out((BD * g * g, Kgp), torch.bfloat16, name="cols (band-group)")
        hip.patchify_bands(img, cols_g, None, BD, C, c0, n_g, S, P, Kgp, None, 0, False, elev)
        gs.check()
        want = ol.im2col_patches(ref_img[:, c0:c0 + n_g], P).reshape(-1, Kg)
        assert torch.equal(cols_g[:, :Kg].cpu(), want.bfloat16()) and (cols_g[:, Kg:] == 0).all()
        t2 = gs.out((BD * g * g, K), name="target (bands entry)")         # target-only mode over all channels = mh_patchify's target
        hip.patchify_bands(img, None, t2, BD, C, 0, C, S, P, (K + 7) // 8 * 8, nb, len(norm_bands), True, elev)
        gs.check()
        assert torch.equal(t2, target)


@pytest.mark.parametrize("B,D,L,E,tok_off,Lg", [(2, 3, 25, 768, 10, 100), (1, 4, 9, 1024, 36, 80), (2, 1, 64, 192, 5, 72)])
def test_groupnorm_embed_finish_guarded(dev, B, D, L, E, tok_off, Lg):  # noqa: N803
    """``mh_groupnorm_stats`` -> ``mh_embed_finish`` -> ``mh_embed_finish_bwd`` with the modality's tokens between another's (NaN rows
    of the group sequence on the gradient side), date rows at an offset.  Tolerances: test_groupnorm_embed_finish_fwd_bwd."""
    from maestro_amd import hip
    gs = GuardSet(dev)
    y = gs.inp(_rand(B * D * L, E, seed=1) * 1.7 + 0.3, name="y")
    gamma, beta = gs.inp(1 + 0.2 * _rand(E, seed=2), name="gamma"), gs.inp(0.1 * _rand(E, seed=3), name="beta")
    pos = gs.inp(_rand(L, E, seed=4), name="pos")
    date_rows, date_off = D + 3, 2
    date_h = _rand(B, D, 8, seed=5)
    date = gs.inp(_in_map(date_rows, date_off, D, date_h, B), name="date")
    partial = gs.out((hip.groupnorm_partial_size(B * D, L, E),), init=0.0, name="partial")
    stats = gs.out((B * D, 2), name="stats")
    hip.groupnorm_stats(y, partial, stats, B * D, L, E)
    gs.check()
    xg = gs.out((B, Lg, E), name="xg")
    xg0 = xg.clone()
    hip.embed_finish(y, stats, gamma, beta, pos, date, date_rows, date_off, xg, B, D, L, E, tok_off, Lg)
    gs.check()
    yr = y.clone().requires_grad_(True)
    gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    img = yr.reshape(B * D, L, E)
    mu = img.mean(dim=(1, 2), keepdim=True)
    var = ((img - mu) ** 2).mean(dim=(1, 2), keepdim=True)
    z = (img - mu) / torch.sqrt(var + 1e-5) * gr + br
    dpad = torch.cat([torch.zeros(B * D, E - 8, device=dev), date_h.reshape(B * D, 8).to(dev)], dim=1)[:, None, :]
    want = (z + pos[None] + dpad).reshape(B, D * L, E)
    got = xg[:, tok_off:tok_off + D * L]
    assert torch.isfinite(got).all() and (got - want).abs().max() < 2e-4
    assert bits_equal(_outside(xg, tok_off, D * L), _outside(xg0, tok_off, D * L)), "another modality's tokens were written"
    dsel = _rand(B, D * L, E, seed=6) * (torch.rand(B, D * L, 1, generator=torch.Generator().manual_seed(8)) < 0.3)
    dxg = gs.inp(_in_map(Lg, tok_off, D * L, dsel, B), name="dxg")
    dyc = gs.out((B * D * L, E), torch.bfloat16, name="dyc")
    dg, db = gs.out((E,), init=0.0, name="dgamma"), gs.out((E,), init=0.0, name="dbeta")
    sums = gs.out((B * D, 2), init=0.0, name="sums")
    hip.embed_finish_bwd(dxg, y, stats, gamma, dyc, dg, db, sums, B, D, L, E, tok_off, Lg)
    gs.check()
    want.backward(dsel.to(dev))
    scale = yr.grad.abs().max().item()
    assert torch.isfinite(dyc.float()).all() and (dyc.float() - yr.grad).abs().max() < 2e-2 * scale
    assert (dg - gr.grad).abs().max() < 1e-3 * max(1, gr.grad.abs().max().item())
    assert (db - br.grad).abs().max() < 1e-3 * max(1, br.grad.abs().max().item())


def test_staging_kernels_guarded(dev):
    """``mh_depatchify``, ``mh_date_features`` (row_off > 0), ``mh_rescale_elev``, ``mh_resize``, ``mh_dihedral``: references and
    tolerances of test_depatchify, test_date_features_and_rescale, test_resize_matches_torch_interpolate, test_dihedral_matches_numpy."""
    import numpy as np

    from maestro_amd import hip
    from oracle import layers as ol
    from oracle import mae as om
    from oracle import staging as ost
    gs = GuardSet(dev)
    BD, C, S, P = 3, 4, 32, 8  # noqa: N806
    img_h = torch.rand(BD, C, S, S, generator=torch.Generator().manual_seed(1))
    patches = gs.inp(om.patch_view(img_h[None], S // P).reshape(-1, P * P * C), name="patches")
    out = gs.out((BD, C, S, S), name="image")
    hip.depatchify(patches, out, BD, C, S, P)
    gs.check()
    assert torch.equal(out.cpu(), img_h)
    dates_h = torch.tensor([[[2019, 100, 10], [2020, 3, 23], [2018, 365, 0]], [[2021, 200, 12], [2019, 182, 0], [2017, 1, 5]]], dtype=torch.int16)
    ref_h = torch.tensor([[[2019, 182, 0]], [[2020, 1, 0]]], dtype=torch.int16)
    dates, ref = gs.inp(dates_h, name="dates"), gs.inp(ref_h, name="ref_date")
    feat = gs.out((2, 6, 8), name="date features")
    feat0 = feat.clone()
    hip.date_features(dates, ref, feat, 2, 3, 6, 2, 0.5)
    gs.check()
    assert (feat[:, 2:5].cpu() - ol.date_features(dates_h, ref_h, 0.5)).abs().max() < 2e-6
    assert bits_equal(_outside(feat, 2, 3), _outside(feat0, 2, 3))
    small_h = torch.rand(3, 2, 8, 8, generator=torch.Generator().manual_seed(2))
    small, res = gs.inp(small_h, name="elev in"), gs.out((3, 2, 8, 8), name="elev out")
    hip.rescale_elev(small, res, 3, 2, 8)
    gs.check()
    want = small_h.clone()
    want[:, 1:] = 30 * (want[:, :1] - want[:, 1:])
    assert torch.equal(res.cpu(), want)
    for hin, hout in [(6, 10), (100, 60), (37, 128)]:
        x_h = torch.rand(3, 2, hin, hin, generator=torch.Generator().manual_seed(hin))
        x = gs.inp(x_h, name="resize in")
        for mode, name in [(0, "nearest"), (1, "bilinear"), (2, "bicubic")]:
            o = gs.out((3, 2, hout, hout), name=f"resize out ({name})")
            hip.resize(x, o, 6, hin, hin, hout, hout, mode)
            gs.check()
            want = F.interpolate(x_h, size=(hout, hout), mode=name)
            assert torch.isfinite(o).all()
            assert torch.equal(o.cpu(), want) if mode == 0 else (o.cpu() - want).abs().max() < (2e-6 if mode == 1 else 5e-6)
    for dtype, S in [(torch.float32, 33), (torch.uint8, 10), (torch.int16, 64), (torch.int64, 33)]:  # noqa: N806
        x_h = (torch.rand(8, 3, 2, S, S, generator=torch.Generator().manual_seed(S)) * 200).to(dtype)
        x, flags = gs.inp(x_h, name="raster"), gs.inp(torch.arange(8, dtype=torch.uint8), name="dihedral flags")
        o = gs.out(x_h.shape, dtype, name="raster out")
        hip.dihedral(x, o, flags)
        gs.check()
        for b in range(8):
            assert np.array_equal(o[b].cpu().numpy(), ost.transform_rasters({"r": x_h[b].numpy()}, b)["r"]), (b, dtype, S)


# ----------------------------------------------------------------------------------------------- masking
@pytest.mark.parametrize("B,L,k", [(2, 225, 169), (3, 1030, 772), (2, 72, 54)])
def test_mask_select_guarded(dev, B, L, k):  # noqa: N803
    """Reference: test_mask_select_matches_oracle (stable argsort)."""
    from maestro_amd import hip
    g = torch.Generator().manual_seed(L)
    noise_h = torch.rand(B, L, generator=g)
    struct_h = torch.rand(B, L, generator=g) < 0.45
    gs = GuardSet(dev)
    noise, struct = gs.inp(noise_h, name="noise"), gs.inp(struct_h.to(torch.uint8), name="struct_mask")
    vis, msk = gs.out((B, L - k), torch.int32, name="visible_idx"), gs.out((B, k), torch.int32, name="masked_idx")
    inv, mask = gs.out((B, L), torch.int32, name="inv"), gs.out((B, L), torch.uint8, name="mask")
    hip.mask_select(noise, struct, vis, msk, inv, mask, B, L, k)
    gs.check()
    order = torch.argsort(noise_h * (1 - struct_h.float()), dim=-1, stable=True)
    want_m, want_v = order[:, :k].sort(dim=1).values, order[:, k:].sort(dim=1).values
    assert torch.equal(msk.cpu().long(), want_m) and torch.equal(vis.cpu().long(), want_v)
    assert torch.equal(mask.cpu().bool(), torch.zeros(B, L, dtype=torch.bool).scatter_(1, want_m, True))
    pos = torch.full((B, L), -1, dtype=torch.long).scatter_(1, want_v, torch.arange(L - k).expand(B, -1))
    assert torch.equal(inv.cpu().long(), pos)


def _unmask_ref(y, inv, tok, slot_bl, pos, date, drow, Dd):  # noqa: N803
    """test_gather_scatter_unmask's reference with a [B, L] slot table (the shared-slot form repeats one row)."""
    B, L = inv.shape  # noqa: N806
    ref = tok[slot_bl.long()].clone()
    vis = inv >= 0
    ref[vis] = y[torch.arange(B)[:, None].expand(B, L)[vis], inv.long()[vis]]
    ref = ref + pos[None]
    ref[:, :, Dd - 8:] += date[:, drow.long()]
    return ref


def test_gather_scatter_expand_unmask_guarded(dev):
    """``mh_gather_rows``, ``mh_scatter_rows``, ``mh_expand_rows``, ``mh_unmask_assemble`` / ``_per_sample``, ``mh_unmask_token_grad`` /
    ``_per_sample``, ``mh_count_masked``: references and tolerances of test_gather_scatter_unmask.  Index bands hold a valid index
    that points at a NaN trap row appended to the indexed source (the row counts passed include it)."""
    from maestro_amd import hip
    B, L, n, dim, dst_L, off = 3, 40, 10, 64, 25, 7  # noqa: N806
    gs = GuardSet(dev)
    src_h = torch.cat([_rand(B, L, dim, seed=1), torch.full((B, 1, dim), NAN)], dim=1)          # row L of every sample: the trap
    src = gs.inp(src_h, name="src")
    idx_h = torch.stack([torch.randperm(L, generator=torch.Generator().manual_seed(b))[:n].sort().values for b in range(B)])
    idx = gs.idx(idx_h.to(torch.int32), L, name="idx")
    dst = gs.out((B, dst_L, dim), name="dst")
    dst0 = dst.clone()
    hip.gather_rows(src, idx, dst, B, L + 1, n, dim, dst_L, off)
    gs.check()
    want = src_h[torch.arange(B)[:, None], idx_h]
    assert torch.equal(dst[:, off:off + n].cpu(), want) and bits_equal(_outside(dst, off, n), _outside(dst0, off, n))
    ddst = gs.inp(_in_map(dst_L, off, n, want, B), name="ddst")
    back = gs.out((B, L + 1, dim), init=0.0, name="dsrc")
    hip.scatter_rows(ddst, idx, back, B, L + 1, n, dim, dst_L, off)
    gs.check()
    ref = torch.zeros(B, L + 1, dim)
    ref[torch.arange(B)[:, None], idx_h] = want
    assert torch.equal(back.cpu(), ref)                                   # (the trap row stays zero: no index past the list was used)
    inv_h = torch.full((B, L), -1, dtype=torch.int32)
    for b in range(B):
        inv_h[b, idx_h[b]] = torch.arange(n, dtype=torch.int32)
    vis_rows = gs.inp(torch.cat([want, torch.full((B, 1, dim), NAN)], dim=1), name="visible rows")
    inv = gs.idx(inv_h, n, name="inv")
    full = gs.out((B, L, dim), name="expanded")
    hip.expand_rows(vis_rows, inv, full, B, L, n + 1, dim)
    gs.check()
    assert torch.equal(full.cpu(), ref[:, :L])
    # decoder input assembly: two mask-token slots + a trap slot, date rows + a trap row
    Dd, slots, ndr = 32, 2, 5  # noqa: N806
    y_h = torch.cat([_rand(B, n, Dd, seed=2), torch.full((B, 1, Dd), NAN)], dim=1)
    tok_h = torch.cat([_rand(slots, Dd, seed=3), torch.full((1, Dd), NAN)])
    pos_h = _rand(L, Dd, seed=4)
    date_h = torch.cat([_rand(B, ndr, 8, seed=5), torch.full((B, 1, 8), NAN)], dim=1)
    slot_h = (torch.arange(L) >= 24).to(torch.int32)
    slot_bl_h = torch.stack([slot_h, 1 - slot_h, (torch.arange(L) % 3 == 0).to(torch.int32)])     # differs between the samples
    drow_h = (torch.arange(L) % ndr).to(torch.int32)
    y, tok, pos, date = gs.inp(y_h, name="y"), gs.inp(tok_h, name="mask_token"), gs.inp(pos_h, name="pos"), gs.inp(date_h, name="date")
    slot, slot_bl = gs.idx(slot_h, slots, name="tok_slot"), gs.idx(slot_bl_h, slots, name="tok_slot_bl")
    drow = gs.idx(drow_h, ndr, name="date_row")
    for per_sample in (False, True):
        xdec = gs.out((B, L, Dd), name="xdec")
        if per_sample:
            hip.unmask_assemble_per_sample(y, inv, tok, slot_bl, pos, date, drow, ndr + 1, xdec, B, L, n + 1, Dd)
        else:
            hip.unmask_assemble(y, inv, tok, slot, pos, date, drow, ndr + 1, xdec, B, L, n + 1, Dd)
        gs.check()
        ref = _unmask_ref(y_h, inv_h, tok_h, slot_bl_h if per_sample else slot_h[None].expand(B, L), pos_h, date_h, drow_h, Dd)
        assert torch.isfinite(xdec).all() and (xdec.cpu() - ref).abs().max() < 1e-6
    m_h = inv_h < 0
    mask = gs.inp(m_h.to(torch.uint8), name="mask")
    dx_h = _rand(B, L, Dd, seed=6)
    dx = gs.inp(dx_h, name="dxdec")
    dtok = gs.out((4, Dd), init=0.0, name="dmask_token")
    hip.unmask_token_grad(dx, mask, slot, dtok[0], B, L, Dd, 0, 0, 24)
    hip.unmask_token_grad(dx, mask, slot, dtok[1], B, L, Dd, 1, 24, L)
    hip.unmask_token_grad_per_sample(dx, mask, slot_bl, dtok[2], B, L, Dd, 0)
    hip.unmask_token_grad_per_sample(dx, mask, slot_bl, dtok[3], B, L, Dd, 1)
    gs.check()
    for row, table, s in ((0, slot_h[None].expand(B, L), 0), (1, slot_h[None].expand(B, L), 1), (2, slot_bl_h, 0), (3, slot_bl_h, 1)):
        want_g = (dx_h * (m_h & (table == s))[:, :, None]).sum((0, 1))
        assert (dtok[row].cpu() - want_g).abs().max() < 1e-4, row
    cnt = gs.out((2,), torch.int32, name="counts")
    hip.count_masked(mask, B, L, 24, L, cnt[:1])
    hip.count_masked_elems(mask, B, L, 3, 24, cnt[1:], 12, False)
    hip.count_masked_elems(mask, B, L, 24, L, cnt[1:], 5, True)
    gs.check()
    assert cnt.tolist() == [int(m_h[:, 24:].sum()), 12 * int(m_h[:, 3:24].sum()) + 5 * int(m_h[:, 24:].sum())]


# ----------------------------------------------------------------------------------------------- loss
@pytest.mark.parametrize("p", [1, 2])
@pytest.mark.parametrize("B,Lm,Lg,off,PPC", [(2, 16, 24, 5, 1024), (3, 36, 80, 36, 8), (2, 400, 410, 7, 40)])
def test_masked_loss_guarded(dev, p, B, Lm, Lg, off, PPC):  # noqa: N803
    """tok_off > 0 and Lgroup > tok_off + Lm.  Tolerances: test_masked_loss."""
    from maestro_amd import hip
    gs = GuardSet(dev)
    rec_h, target_h = _rand(B * Lm, PPC, seed=1), _rand(B * Lm, PPC, seed=2)
    mask_h = (torch.rand(B, Lg, generator=torch.Generator().manual_seed(3)) < 0.7).to(torch.uint8)
    rec, target, mask = gs.inp(rec_h, name="rec"), gs.inp(target_h, name="target"), gs.inp(mask_h, name="mask_group")
    cnt = gs.out((1,), torch.int32, name="n_masked")
    hip.count_masked(mask, B, Lg, off, off + Lm, cnt)
    acc = gs.out((1,), init=0.0, name="acc")
    drec = gs.out((B * Lm, PPC), torch.bfloat16, name="drec")
    hip.masked_loss(rec, target, mask, cnt, 0.37, acc, drec, B, Lm, Lg, off, PPC, p)
    gs.check()
    m = mask_h[:, off:off + Lm].reshape(-1).bool()
    r = rec_h.clone().requires_grad_(True)
    err = (target_h - r).abs() if p == 1 else (target_h - r) ** 2
    want = 0.37 * err[m].mean()
    want.backward()
    assert int(cnt) == int(m.sum())
    assert abs(acc.item() - want.item()) < 1e-5 * max(1, abs(want.item()))
    assert torch.isfinite(drec.float()).all() and (drec.float().cpu() - r.grad).abs().max() < 1e-2 * r.grad.abs().max().item()


@pytest.mark.parametrize("P", [8, 16])
def test_masked_loss_bands_guarded(dev, P):  # noqa: N803
    """``mh_masked_loss_bands`` with tok_off > 0, Lgroup > tok_off + Lm, band windows with tgt_c0 > 0.  Tolerances:
    test_patchify_and_loss_over_band_groups."""
    from maestro_amd import hip
    B, Lm, C, sizes, off = 3, 16, 4, (1, 3), 3  # noqa: N806
    PP, T = P * P, B * Lm  # noqa: N806
    Lg = off + Lm * len(sizes) + 5  # noqa: N806
    gs = GuardSet(dev)
    target_h = _rand(T, PP * C, seed=9)
    mask_h = (torch.rand(B, Lg, generator=torch.Generator().manual_seed(5)) < 0.6).to(torch.uint8)
    target, mask = gs.inp(target_h, name="target"), gs.inp(mask_h, name="mask_group")
    cnt, acc = gs.out((1,), torch.int32, name="n_elems"), gs.out((1,), init=0.0, name="acc")
    for gi, n_g in enumerate(sizes):
        hip.count_masked_elems(mask, B, Lg, off + gi * Lm, off + (gi + 1) * Lm, cnt, n_g * PP, gi > 0)
    c0, tot, n_el, checks = 0, 0.0, 0, []
    for gi, n_g in enumerate(sizes):
        Kg, t_lo = n_g * PP, off + gi * Lm  # noqa: N806
        rec_h = _rand(T, Kg, seed=20 + gi)
        rec, drec = gs.inp(rec_h, name=f"rec{gi}"), gs.out((T, Kg), torch.bfloat16, name=f"drec{gi}")
        hip.masked_loss_bands(rec, target, mask, cnt, 0.41, acc, drec, B, Lm, Lg, t_lo, Kg, 2, C, c0, n_g)
        m = mask_h[:, t_lo: t_lo + Lm].reshape(-1).bool()
        tw = target_h.view(T, PP, C)[:, :, c0: c0 + n_g].reshape(T, Kg)
        tot += float(((rec_h - tw) ** 2)[m].double().sum())
        n_el += int(m.sum()) * Kg
        checks.append((drec, rec_h, tw, m))
        c0 += n_g
    gs.check()
    assert int(cnt) == n_el
    assert abs(acc.item() - 0.41 * tot / n_el) < 1e-5 * max(1.0, 0.41 * tot / n_el)
    for drec, rec_h, tw, m in checks:
        want = 2 * (rec_h - tw) * 0.41 / n_el * m[:, None]
        assert torch.isfinite(drec.float()).all() and (drec.float().cpu() - want).abs().max() < 1e-2 * want.abs().max()


# ----------------------------------------------------------------------------------------------- probe / finetune heads
@pytest.mark.parametrize("h,H", [(5, 32), (4, 4), (8, 4), (3, 10)])
def test_token_resize_guarded(dev, h, H):  # noqa: N803
    """in_off, out_off > 0 with rows behind the modality too.  Tolerances: test_token_resize_fwd_bwd."""
    from maestro_amd import hip
    B, D, E, pre, post, opre, opost = 2, 3, 64, 7, 5, 2, 3  # noqa: N806
    g = torch.Generator().manual_seed(h * 100 + H)
    xs_h = torch.randn(B, D * h * h, E, generator=g)
    in_rows, out_rows = pre + D * h * h + post, opre + D * H * H + opost
    gs = GuardSet(dev)
    x = gs.inp(_in_map(in_rows, pre, D * h * h, xs_h, B), name="in")
    out = gs.out((B, out_rows, E), name="out")
    out0 = out.clone()
    hip.token_resize(x, in_rows, pre, out, out_rows, opre, B, D, h, H, E)
    gs.check()
    xr = xs_h.reshape(B * D, h, h, E).permute(0, 3, 1, 2).clone().requires_grad_(True)
    want = F.interpolate(xr, (H, H), mode="bilinear")
    got = out[:, opre:opre + D * H * H].cpu().reshape(B * D, H, H, E).permute(0, 3, 1, 2)
    assert torch.isfinite(got).all() and (got - want.detach()).abs().max() < 1e-5
    assert bits_equal(_outside(out, opre, D * H * H), _outside(out0, opre, D * H * H))
    douts_h = torch.randn(B, D * H * H, E, generator=g)
    want.backward(douts_h.reshape(B * D, H, H, E).permute(0, 3, 1, 2))
    dout = gs.inp(_in_map(out_rows, opre, D * H * H, douts_h, B), name="dout")
    din = gs.out((B, in_rows, E), name="din")
    din[:, pre:pre + D * h * h] = 1.0                                     # accumulate = 1 adds to what the map's rows hold
    din0 = din.clone()
    hip.token_resize_bwd(dout, out_rows, opre, din, in_rows, pre, B, D, h, H, E, accumulate=True)
    gs.check()
    ref = 1 + xr.grad.permute(0, 2, 3, 1).reshape(B, D * h * h, E)
    assert (din[:, pre:pre + D * h * h].cpu() - ref).abs().max() < 1e-4
    assert bits_equal(_outside(din, pre, D * h * h), _outside(din0, pre, D * h * h))


@pytest.mark.parametrize("dim,nb,T,Lr", [(192, 3, 17, 16), (768, 37, 5, 1), (192, 4, 333, 1)])
def test_attentive_reduce_guarded(dev, dim, nb, T, Lr):  # noqa: N803
    """Tolerances: test_attentive_reduce_fwd_bwd."""
    from maestro_amd import hip
    heads, dh = 8, dim // 8
    g = torch.Generator().manual_seed(dim + T)
    kv16 = (torch.randn(nb * T * Lr, 2 * dim, generator=g) * 1.5).bfloat16()
    query_h = torch.randn(dim, generator=g)
    kvf = kv16.float().reshape(nb, T, Lr, 2 * dim).permute(0, 2, 1, 3).reshape(nb * Lr, T, 2 * dim).requires_grad_(True)
    q = query_h.clone().requires_grad_(True)
    k, v = kvf[..., :dim].reshape(-1, T, heads, dh), kvf[..., dim:].reshape(-1, T, heads, dh)
    attn = (torch.einsum("hd,sthd->sht", q.reshape(heads, dh), k) * dh ** -0.5).softmax(-1)
    want = torch.einsum("sht,sthd->shd", attn, v).reshape(-1, dim)
    gs = GuardSet(dev)
    kv, query = gs.inp(kv16, name="kv"), gs.inp(query_h, name="query")
    out, lse = gs.out((nb * Lr, dim), name="out"), gs.out((nb * Lr, heads), name="lse")
    hip.attn_reduce_fwd(kv, query, out, lse, nb, T, Lr, dim)
    gs.check()
    assert torch.isfinite(out).all() and torch.isfinite(lse).all()
    assert (out.cpu() - want.detach()).abs().max() < 2e-4 * max(1.0, want.abs().max().item())
    dout_h = torch.randn(nb * Lr, dim, generator=g)
    want.backward(dout_h)
    dout = gs.inp(dout_h, name="dout")
    dkv = gs.out((nb * T * Lr, 2 * dim), torch.bfloat16, name="dkv")
    part = gs.out((hip.attn_reduce_partial_rows(nb * Lr), dim), name="dq_partial")
    hip.attn_reduce_bwd(kv, query, out, lse, dout, dkv, part, nb, T, Lr, dim)
    gs.check()
    dq = part.sum(0).cpu()
    assert torch.isfinite(dq).all() and (dq - q.grad).abs().max() < 2e-3 * q.grad.abs().max()
    ref = kvf.grad.reshape(nb, Lr, T, 2 * dim).permute(0, 2, 1, 3).reshape(nb * T * Lr, 2 * dim)
    err = (dkv.float().cpu() - ref).abs().max().item()
    assert err < 1e-2 * ref.abs().max().item() + 1e-6, err


def test_mean_reduce_head_linear_losses_guarded(dev):
    """``mh_mean_reduce_fwd`` / ``_bwd``, ``mh_head_linear_fwd`` / ``_bwd`` (test_mean_reduce_and_head_linear), ``mh_count_valid``,
    ``mh_ce_loss`` with ld > P * P * C (test_cross_entropy_patch_layout), ``mh_bce_loss`` (test_bce_with_missing_rows)."""
    from maestro_amd import hip
    nb, T, Lr, dim, C = 3, 7, 5, 192, 15  # noqa: N806
    g = torch.Generator().manual_seed(3)
    gs = GuardSet(dev)
    x_h = torch.randn(nb * T * Lr, dim, generator=g)
    x, out = gs.inp(x_h, name="x"), gs.out((nb * Lr, dim), name="mean")
    hip.mean_reduce_fwd(x, out, nb, T, Lr, dim)
    gs.check()
    assert (out.cpu() - x_h.reshape(nb, T, Lr, dim).mean(1).reshape(nb * Lr, dim)).abs().max() < 1e-6
    dout_h = torch.randn(nb * Lr, dim, generator=g)
    dout, dx = gs.inp(dout_h, name="dout"), gs.out((nb * T * Lr, dim), name="dx")
    hip.mean_reduce_bwd(dout, dx, nb, T, Lr, dim)
    gs.check()
    assert (dx.cpu() - (dout_h.reshape(nb, 1, Lr, dim) / T).expand(nb, T, Lr, dim).reshape(-1, dim)).abs().max() < 1e-7
    B = 6  # noqa: N806
    xb = torch.randn(B, dim, generator=g, requires_grad=True)
    W = torch.randn(C, dim, generator=g, requires_grad=True)  # noqa: N806
    bias = torch.randn(C, generator=g, requires_grad=True)
    xd, Wd, bd = gs.inp(xb.detach(), name="x"), gs.inp(W.detach(), name="W"), gs.inp(bias.detach(), name="bias")  # noqa: N806
    logits = gs.out((B, C), name="logits")
    hip.head_linear_fwd(xd, Wd, bd, logits, B, C, dim)
    gs.check()
    wl = xb @ W.t() + bias
    assert (logits.cpu() - wl.detach()).abs().max() < 1e-4
    dl_h = torch.randn(B, C, generator=g)
    wl.backward(dl_h)
    dl = gs.inp(dl_h, name="dlogits")
    dxg, dW, db = gs.out((B, dim), name="dx"), gs.out((C, dim), init=1.0, name="dW"), gs.out((C,), init=1.0, name="db")  # noqa: N806
    hip.head_linear_bwd(xd, Wd, dl, dxg, dW, db, B, C, dim)
    gs.check()
    assert (dxg.cpu() - xb.grad).abs().max() < 1e-4 and (dW.cpu() - 1 - W.grad).abs().max() < 1e-4
    assert (db.cpu() - 1 - bias.grad).abs().max() < 1e-5
    # cross entropy at patch layout, logits and gradient rows ld apart
    for (Bc, gg, P, Cc, missing, tdtype) in [(2, 4, 8, 15, -1, torch.int64), (3, 2, 4, 19, 19, torch.uint8), (5, 1, 1, 7, -1, torch.int32)]:  # noqa: N806
        S, PPC = gg * P, P * P * Cc  # noqa: N806
        ld = PPC + 12
        gen = torch.Generator().manual_seed(Bc * 10 + Cc)
        patch_h = torch.randn(Bc * gg * gg, PPC, generator=gen) * 2
        target_h = torch.randint(0, Cc, (Bc, S, S), generator=gen)
        target_h[torch.rand(Bc, S, S, generator=gen) < 0.2] = missing
        img = patch_h.reshape(Bc, gg, gg, P, P, Cc).permute(0, 5, 1, 3, 2, 4).reshape(Bc, Cc, S, S).clone().requires_grad_(True)
        tg = target_h.reshape(-1)
        keep = (tg != missing).nonzero().squeeze(1)
        want = F.cross_entropy(img.permute(0, 2, 3, 1).reshape(-1, Cc).index_select(0, keep), tg.index_select(0, keep))
        want.backward()
        ref = img.grad.reshape(Bc, Cc, gg, P, gg, P).permute(0, 2, 4, 3, 5, 1).reshape(Bc * gg * gg, PPC)
        patch, target = gs.inp(patch_h, ld=ld, name="logits"), gs.inp(target_h.to(tdtype), name="target")
        cnt, acc = gs.out((1,), torch.int32, init=0, name="n_valid"), gs.out((1,), init=0.0, name="acc")
        hip.count_valid(target, missing, cnt)
        gs.check()
        assert int(cnt) == len(keep)
        for dt in (torch.float32, torch.bfloat16):
            acc.zero_()
            d = gs.out((Bc * gg * gg, PPC), dt, ld=ld, name="dlogits")
            hip.ce_loss(patch, target, missing, cnt, acc, d, Bc, gg, P, Cc, ld=ld)
            gs.check()
            assert abs(acc.item() - want.item()) < 1e-4 * abs(want.item())
            assert torch.isfinite(d.float()).all()
            assert (d.float().cpu() - ref).abs().max() <= (1e-6 if dt == torch.float32 else 1e-2 * ref.abs().max().item())
    Bb, Cb = 9, 15  # noqa: N806
    gen = torch.Generator().manual_seed(5)
    xl = (torch.randn(Bb, Cb, generator=gen) * 3).requires_grad_(True)
    t = (torch.rand(Bb, Cb, generator=gen) < 0.3).float()
    t[2, 4], t[7, 0] = -1.0, -1.0
    keep = (t != -1).all(dim=1).nonzero().squeeze(1)
    want = F.binary_cross_entropy_with_logits(xl.index_select(0, keep), t.index_select(0, keep))
    want.backward()
    lg, tt = gs.inp(xl.detach(), name="bce logits"), gs.inp(t, name="bce target")
    acc, d = gs.out((1,), init=0.0, name="bce acc"), gs.out((Bb, Cb), name="bce dlogits")
    hip.bce_loss(lg, tt, -1, acc, d, Bb, Cb)
    gs.check()
    assert abs(acc.item() - want.item()) < 1e-5 and (d.cpu() - xl.grad).abs().max() < 1e-6


# ----------------------------------------------------------------------------------------------- misc
def test_colsum_cast_pack_guarded(dev):
    """``mh_colsum`` (ld > N, M over one row block), ``mh_colsum_batched``, ``mh_cast_bf16`` (n % 4 != 0), ``mh_pack_rows_bf16``,
    ``mh_unpack_rows_add``.  Tolerances: test_colsum_cast_pack_adamw, test_layernorm_partial_plus_batched_colsum_equals_fused_reduce."""
    from maestro_amd import hip
    M, N = 1000, 264  # noqa: N806
    gs = GuardSet(dev)
    x_h = _rand(M, N, seed=1)
    for dt in (torch.float32, torch.bfloat16):
        x = gs.inp(x_h.to(dt), ld=N + (12 if dt == torch.float32 else 40), name="x")
        out = gs.out((N,), init=1.0, name="colsum")
        hip.colsum(x, out, M, N, x.stride(0))
        gs.check()
        assert (out.cpu() - (1 + x_h.to(dt).float().sum(0))).abs().max() < 1e-3
    g = torch.Generator().manual_seed(9)
    mats = [torch.randn(37, 64, generator=g), torch.randn(403, 192, generator=g), torch.randn(5, 300, generator=g)]
    jobs, sums = [], []
    for i, mat in enumerate(mats):
        rows, cols = mat.shape
        gs.inp(mat, ld=cols + 36, name=f"colsum_batched src{i}")
        span = gs.guards[-1].span()
        dst = gs.out((cols,), init=0.5, name=f"colsum_batched dst{i}")
        jobs.append((span, dst, rows, cols, cols + 36))
        sums.append((dst, 0.5 + mat.sum(0)))
    hip.ColsumBatch(jobs, dev).launch()
    gs.check()
    for dst, want in sums:
        assert torch.allclose(dst.cpu(), want, rtol=1e-5, atol=1e-4)
    n = 4099
    src_h = _rand(n, seed=2)
    src, dst = gs.inp(src_h, name="cast src"), gs.out((n,), torch.bfloat16, name="cast dst")
    hip.cast_bf16(src, dst, n)
    gs.check()
    assert torch.equal(dst.cpu(), src_h.bfloat16())
    E, K, Kpad = 10, 40, 64  # noqa: N806
    w_h = _rand(E, K, seed=3)
    w, wp = gs.inp(w_h, name="w"), gs.out((E, Kpad), torch.bfloat16, name="packed")
    hip.pack_rows_bf16(w, wp, E, K, Kpad)
    gs.check()
    assert torch.equal(wp[:, :K].cpu(), w_h.bfloat16()) and (wp[:, K:] == 0).all()
    padded = torch.full((E, Kpad), NAN)                                   # the columns behind K are not the gradient's: never added
    padded[:, :K] = w_h
    srcp, acc = gs.inp(padded, name="padded grad"), gs.out((E, K), init=1.0, name="unpacked")
    hip.unpack_rows_add(srcp, acc, E, K, Kpad)
    gs.check()
    assert torch.equal(acc.cpu(), 1 + w_h)


# ----------------------------------------------------------------------------------------------- the flat parameter store
@pytest.mark.parametrize("entry", ["adamw", "adamw_dev"])
def test_adamw_on_a_slice_of_the_flat_store(dev, entry):
    """``mh_adamw`` / ``mh_adamw_dev`` on elements [lo, hi) of flat p, g, m, v, p_bf16 buffers (lo a multiple of 4 but not of 1024,
    hi - lo not a multiple of 1024, grad_scale != 1): three steps against torch.optim.AdamW in fp64 on the slice (1e-5 and the
    exact bf16 shadow: test_colsum_cast_pack_adamw); everything outside the slice is NaN and keeps its bits.  The device-scalar
    form with hyper[4] = 0 changes nothing at all."""
    from maestro_amd import hip
    total, lo, hi = 9000, 1028, 1028 + 4100
    n = hi - lo
    lr, b1, b2, eps, wd, gscale = 1e-2, 0.9, 0.99, 1e-8, 0.01, 0.5
    gs = GuardSet(dev)
    p, g, m, v = (gs.out((total,), name=nm) for nm in "pgmv")
    pb = gs.out((total,), torch.bfloat16, name="p_bf16")
    p0 = _rand(n, seed=4)
    p[lo:hi], m[lo:hi], v[lo:hi] = p0.to(dev), 0.0, 0.0
    p_ref = p0.double().requires_grad_(True)
    opt = torch.optim.AdamW([p_ref], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)

    def outside():
        return [torch.cat([t[:lo], t[hi:]]).clone() for t in (p, g, m, v, pb)]

    for step in range(1, 4):
        grad = _rand(n, seed=10 + step)
        g[lo:hi] = grad.to(dev)
        before = outside()
        p_ref.grad = grad.double() * gscale
        opt.step()
        if entry == "adamw":
            hip.adamw(p[lo:hi], g[lo:hi], m[lo:hi], v[lo:hi], pb[lo:hi], n, lr, b1, b2, eps, wd, step, gscale)
        else:
            bc1, bc2 = hip.adamw_bias_corrections(b1, b2, step)
            hyper = gs.inp(torch.tensor([lr, bc1, bc2, gscale, 1.0]), name="hyper")
            hip.adamw_dev(p[lo:hi], g[lo:hi], m[lo:hi], v[lo:hi], pb[lo:hi], n, b1, b2, eps, wd, hyper)
        gs.check()
        for t, t0 in zip(outside(), before):
            assert bits_equal(t, t0), "an element outside the slice changed"
        assert torch.isfinite(p[lo:hi]).all()
    assert (p[lo:hi].cpu().double() - p_ref.detach()).abs().max() < 1e-5
    assert torch.equal(pb[lo:hi], p[lo:hi].bfloat16())
    if entry == "adamw_dev":
        hyper = gs.inp(torch.tensor([lr, 0.5, 0.5, gscale, 0.0]), name="hyper (inactive)")
        for gd in gs.guards:
            gd.arm(whole=True)
        hip.adamw_dev(p[lo:hi], g[lo:hi], m[lo:hi], v[lo:hi], pb[lo:hi], n, b1, b2, eps, wd, hyper)
        gs.check()                                                        # active == 0: not one bit of p, g, m, v, p_bf16 moved


def test_scale_dev_guarded(dev):
    """``mh_scale_dev``: n % 4 != 0, the scalar read on the device; scale == 1 leaves every bit (a NaN element included) alone."""
    from maestro_amd import hip
    n = 4099
    gs = GuardSet(dev)
    x_h = _rand(n, seed=6)
    x, s = gs.out((n,), name="x"), gs.inp(torch.tensor([0.37]), name="scale")
    x.copy_(x_h)
    hip.scale_dev(x, n, s)
    gs.check()
    assert torch.equal(x.cpu(), x_h * torch.tensor(0.37))                 # one fp32 multiplication: exact
    one = gs.inp(torch.tensor([1.0]), name="scale one")
    x[17] = NAN
    for gd in gs.guards:
        gd.arm(whole=True)
    hip.scale_dev(x, n, one)
    gs.check()


def test_zero_spans_guarded(dev):
    """``mh_zero_spans`` into a NaN-filled buffer: spans of 1, 3, 1023, 1025 and 5000 floats with unaligned starts, two of them
    adjacent; exactly the spans are zero, everything else keeps its bits.  The bands of the span table hold a valid record that
    points at the buffer's last element, which no listed span covers."""
    from maestro_amd import hip
    n = 20000
    spans_h = [(3, 1), (4, 3), (101, 1023), (1124, 1025), (2500, 5000), (9001, 1), (12345, 1023)]
    gs = GuardSet(dev)
    base = gs.out((n,), name="base")
    spans = gs.idx(torch.tensor(spans_h, dtype=torch.int64), [n - 1, 1], name="spans")
    hip.zero_spans(base, spans, len(spans_h), max(ln for _, ln in spans_h))
    gs.check()
    want_zero = torch.zeros(n, dtype=torch.bool)
    for o, ln in spans_h:
        want_zero[o:o + ln] = True
    got = base.cpu()
    assert bool((got[want_zero] == 0).all()) and bits_equal(got[want_zero], torch.zeros(int(want_zero.sum())))
    assert bits_equal(got[~want_zero], torch.full((int((~want_zero).sum()),), NAN)), "an element outside the spans changed"
