"""HIP kernels against fp64 references under a-priori error bounds (tests/numerics.py; their teeth: tests/test_numerics_selfcheck.py).

A  fp32 accumulation of every bf16 GEMM tile, every layout, K = 64 ... 16384, four operand distributions:  |C - C64| <= K 2^-23 |A||B|
B  the bf16 store: that bound + half a bf16 ulp, and bit equality with round-to-nearest-even of the same tile's fp32 output
C  the fused epilogues on exactly known fp32 pre-activations (GELU, saved GELU' as bf16 / byte code, bias + residual, MULAUX /
   DGELU products, 64-row column sums)
D  atomic split-K wgrads at token length onto a preloaded destination; power-of-two operand scaling is bit-exact
E  LayerNorm / GroupNorm(1, E) / patch-target statistics far off-centre against two honest fp32 references

Inputs are seeded on the CPU; references are fp64 on the device.  Worst error / bound ratios go to ``observed`` (profiles/numerics_bounds.md).
The stream-K tiles are not exercised."""

import pytest
import torch

from tests import numerics as nm

pytestmark = pytest.mark.gpu

NT, NN, TN = 0, 1, 2
LAYOUTS = {NT: "NT", NN: "NN", TN: "TN"}
# every tile that serves bf16 GEMMs through mh_gemm_bf16_tile: hip.TILES + the other heights of the register-staged kernel + the persistent tile
TILE_IDS = {"REG_128": 0, "DMA_256": 1, "DMA_256x128": 2, "DMA_128x256": 3, "DMA_128": 4, "DMA_128x4": 5, "REG_64": 13, "REG_192": 14,
            "PP_128": 7}
M0, N0 = 1000, 264          # ragged against every tile (128 / 192 / 256 rows, 128 / 256 columns)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


class Operands:
    """One (a [M, K], b [K, N]) pair on the device in the three physical layouts, with its fp64 reference."""

    def __init__(self, a, b, dev):
        self.M, self.K, self.N = a.shape[0], a.shape[1], b.shape[1]
        a, b = a.to(dev), b.to(dev)
        self.c64, self.absprod = nm.gemm_ref64(a, b)
        a, b = a.bfloat16(), b.bfloat16()
        self.phys = {NT: (a.contiguous(), b.t().contiguous()), NN: (a.contiguous(), b.contiguous()), TN: (a.t().contiguous(), b.contiguous())}

    def run(self, tile, layout, flags, out_dtype, n_cols=None, fill=None, **kw):
        """Launch on the first ``n_cols`` columns; returns C, or None where the tile declines the problem (rc -2: nothing launched)."""
        from maestro_amd import hip
        A, B = self.phys[layout]  # noqa: N806
        N = n_cols or self.N  # noqa: N806
        C = torch.full((self.M, N), float("nan"), device=A.device, dtype=out_dtype) if fill is None else fill  # noqa: N806
        try:
            hip.gemm(layout, self.M, N, self.K, A, A.shape[1], B, B.shape[1], C, N, flags, tile=tile, **kw)
        except hip.HipExtensionError as e:
            if "does not qualify" in str(e):
                return None
            raise
        return C


def _run_f32(op, tile, layout, n_cols=None):
    """The tile's fp32 accumulator.  MH_TILE_PP_128 has no plain fp32 epilogue: it is read through OUT_F32 | BIAS | RESIDUAL with a
    zero bias and a zero residual (adding +0 is exact; the only trace is that a -0 sum would come out as +0, equal in value)."""
    c = op.run(tile, layout, 1, torch.float32, n_cols=n_cols)
    if c is None:
        n = n_cols or op.N
        dev = op.c64.device
        c = op.run(tile, layout, 1 | 2 | 8, torch.float32, n_cols=n_cols, bias=torch.zeros(n, device=dev),
                   res=torch.zeros(op.M, n, device=dev), ldr=n)
    return c


def _check(got, want64, bound, what):
    err = (got.double() - want64).abs()
    ratio = nm.worst_ratio(err, bound)
    print(f"{what}: worst error / bound = {ratio:.3e}")
    assert ratio <= 1.0, f"{what}: error {ratio:.3f} x its bound ({int((err > bound).sum())} of {err.numel()} elements outside)"
    return ratio


# ------------------------------------------------------------------------------------------------ A + B
@pytest.mark.parametrize("K", [64, 768, 3072, 16384])
@pytest.mark.parametrize("dist", nm.DISTRIBUTIONS)
def test_accumulation_and_bf16_store_every_tile(dev, observed, dist, K):  # noqa: N803
    """Parts A and B.  A tile that declines (M0, N0, K) is run on the nearest shape it serves: N = 256 for the persistent tile
    (N % 128), K = 512 where K = 64 is below a tile's minimum; which tile served which shape is recorded."""
    cases = {}

    def case(k):
        if k not in cases:
            cases[k] = Operands(*nm.gemm_operands(dist, M0, N0, k), dev)
        return cases[k]

    for name, tile in TILE_IDS.items():
        worst_a = worst_b = 0.0
        for layout, lname in LAYOUTS.items():
            served = None
            for k, ncols in ((K, None), (K, 256), (max(K, 512), None), (max(K, 512), 256)):
                op = case(k)
                c32 = _run_f32(op, tile, layout, ncols)
                if c32 is not None:
                    served = (k, ncols or N0)
                    break
            if served is None:
                observed("numerics_gpu::served", f"{name}/{lname}/K{K}", -2.0)     # serves none of the nearby shapes: recorded, not silent
                assert name == "PP_128" and layout == TN, f"{name} {lname} declined every shape near K = {K}"
                continue
            observed("numerics_gpu::served", f"{name}/{lname}/K{K}/as_M{M0}_N{served[1]}_K{served[0]}", 0.0)
            k, n = served
            c64, absprod = op.c64[:, :n], op.absprod[:, :n]
            torch.cuda.synchronize()
            worst_a = max(worst_a, _check(c32, c64, nm.gemm_bound(absprod, k), f"A {name} {lname} {dist} K={k}"))
            cb = op.run(tile, layout, 0, torch.bfloat16, n_cols=n if n != N0 else None)
            assert cb is not None, f"{name} {lname}: serves the fp32 output but not the bf16 one"
            torch.cuda.synchronize()
            worst_b = max(worst_b, _check(cb, c64, nm.bf16_store_bound(c64, absprod, k), f"B {name} {lname} {dist} K={k}"))
            # B.2, no tolerance: same launch configuration, same accumulator -> the store is round-to-nearest-even of it
            same = cb.view(torch.int16) == c32.bfloat16().view(torch.int16)
            assert bool(same.all()), f"{name} {lname} {dist} K={k}: bf16 output is not RNE of the fp32 output in {int((~same).sum())} elements"
        observed("numerics_gpu::A_accumulation", f"{name}/{dist}/K{K}", worst_a)
        observed("numerics_gpu::B_bf16_store", f"{name}/{dist}/K{K}", worst_b)


def test_accumulation_persistent_tile_several_tiles_per_workgroup(dev, observed):
    """MH_TILE_PP_128 with three output tiles per workgroup (8192 x 3072: 1536 tiles on 512 workgroup slots): the second accumulator set."""
    M, N, K = 8192, 3072, 768  # noqa: N806
    op = Operands(*nm.gemm_operands("offset", M, N, K), dev)
    for layout in (NT, NN):
        c32 = _run_f32(op, TILE_IDS["PP_128"], layout)
        cb = op.run(TILE_IDS["PP_128"], layout, 0, torch.bfloat16)
        assert c32 is not None and cb is not None
        torch.cuda.synchronize()
        ra = _check(c32, op.c64, nm.gemm_bound(op.absprod, K), f"A PP_128 {LAYOUTS[layout]} 8192x3072")
        rb = _check(cb, op.c64, nm.bf16_store_bound(op.c64, op.absprod, K), f"B PP_128 {LAYOUTS[layout]} 8192x3072")
        assert torch.equal(cb.view(torch.int16), c32.bfloat16().view(torch.int16))
        observed("numerics_gpu::A_accumulation", f"PP_128/{LAYOUTS[layout]}/offset/8192x3072x768", ra)
        observed("numerics_gpu::B_bf16_store", f"PP_128/{LAYOUTS[layout]}/offset/8192x3072x768", rb)


@pytest.mark.parametrize("dist", nm.DISTRIBUTIONS)
def test_accumulation_grouped_tn(dev, observed, dist):
    """Part A for mh_gemm_grouped_tn (plain stores: every problem is the only writer of its output), K = 64 ... 16384 in one launch."""
    from maestro_amd import hip
    ops, probs, outs = [], [], []
    for K in (64, 768, 3072, 16384):  # noqa: N806
        op = Operands(*nm.gemm_operands(dist, M0, N0, K), dev)
        A, B = op.phys[TN]  # noqa: N806
        C = torch.full((M0, N0), float("nan"), device=dev)  # noqa: N806
        ops.append(op), outs.append(C), probs.append((A, B, C, M0, N0, K, M0, N0, N0))
    hip.GroupedTN(probs, dev).launch()
    torch.cuda.synchronize()
    for op, C in zip(ops, outs):  # noqa: N806
        r = _check(C, op.c64, nm.gemm_bound(op.absprod, op.K), f"A grouped_tn {dist} K={op.K}")
        observed("numerics_gpu::A_accumulation", f"GROUPED_TN/{dist}/K{op.K}", r)


# ------------------------------------------------------------------------------------------------ C: epilogues
class Grid:
    """Exactly known pre-activations: K = 8 (512 where a tile needs it), A[m, 0] = a[m] (bf16), B[n, 0] = 1, everything else 0, so the
    accumulator is a[m] exactly and the epilogue's x[m, n] = fl32(a[m] + bias[n]) is ONE correctly rounded fp32 addition, reproduced
    here.  The 107 row values cycle with stride 37 over 520 rows and the 32 bias values repeat over 264 columns (both ragged against
    the tiles; 256 columns for the persistent tile), so that every lane and staging pass of an epilogue meets tail values."""

    def __init__(self, dev, K, N=264):  # noqa: N803
        a, bias = nm.gelu_grid()
        self.M, self.N, self.K = 520, N, K
        rows = a[(torch.arange(self.M) * 37) % a.numel()]
        self.bias = bias[torch.arange(self.N) % 32].to(dev)
        A = torch.zeros(self.M, K)  # noqa: N806
        A[:, 0] = rows
        B = torch.zeros(self.N, K)  # noqa: N806
        B[:, 0] = 1.0
        self.A, self.B = A.to(dev).bfloat16(), B.to(dev).bfloat16()
        self.x = rows.to(dev)[:, None] + self.bias[None, :]          # fp32, as the epilogue forms it
        self.x64 = self.x.double()

    def run(self, tile, flags, **kw):
        from maestro_amd import hip
        C = torch.full((self.M, self.N), float("nan"), device=self.A.device, dtype=torch.bfloat16)  # noqa: N806
        try:
            hip.gemm(NT, self.M, self.N, self.K, self.A, self.K, self.B, self.K, C, self.N, flags, bias=self.bias, tile=tile, **kw)
        except hip.HipExtensionError as e:
            if "does not qualify" in str(e):
                return None
            raise
        torch.cuda.synchronize()
        return C


@pytest.mark.parametrize("name", list(TILE_IDS))
def test_gelu_epilogues_on_exact_preactivations(dev, observed, name):
    from maestro_amd import hip
    tile = TILE_IDS[name]
    ran = []
    for K in (8, 512):  # noqa: N806
        g = Grid(dev, K, 256 if name == "PP_128" else 264)      # (the persistent tile: N % 128 == 0)
        # BIAS | GELU with the saved pre-activation
        aux = torch.zeros(g.M, g.N, device=dev, dtype=torch.bfloat16)
        y = g.run(tile, hip.BIAS | hip.GELU, aux_out=aux, ldaux=g.N)
        if y is not None:
            ran.append(f"gelu@K{K}")
            r = _check(y, nm.gelu64(g.x64), nm.gelu_bound(g.x64), f"C gelu {name} K={K}")
            observed("numerics_gpu::C_gelu", f"{name}/K{K}", r)
            assert torch.equal(aux.view(torch.int16), g.x.bfloat16().view(torch.int16)), "saved pre-activation is not bf16(acc + bias)"
        # ... with GELU' saved as bf16
        d16 = torch.zeros(g.M, g.N, device=dev, dtype=torch.bfloat16)
        y2 = g.run(tile, hip.BIAS | hip.GELU | hip.AUX_DGELU, aux_out=d16, ldaux=g.N)
        if y2 is not None:
            ran.append(f"dgelu16@K{K}")
            _check(y2, nm.gelu64(g.x64), nm.gelu_bound(g.x64), f"C gelu(+aux_dgelu) {name} K={K}")
            r = _check(d16, nm.dgelu64(g.x64), nm.dgelu_bound(g.x64), f"C saved gelu' bf16 {name} K={K}")
            observed("numerics_gpu::C_dgelu_bf16", f"{name}/K{K}", r)
        # ... as a byte code: no wrap at either end of the range
        d8 = torch.full((g.M, g.N), 77, device=dev, dtype=torch.uint8)
        y3 = g.run(tile, hip.BIAS | hip.GELU | hip.AUX_DGELU | hip.AUX_U8, aux_out=d8, ldaux=g.N)
        if y3 is not None:
            ran.append(f"dgelu8@K{K}")
            _check(y3, nm.gelu64(g.x64), nm.gelu_bound(g.x64), f"C gelu(+aux_u8) {name} K={K}")
            r = _check(nm.decode_u8(d8), nm.dgelu64(g.x64), nm.dgelu_bound(g.x64, u8=True), f"C saved gelu' u8 {name} K={K}")
            observed("numerics_gpu::C_dgelu_u8", f"{name}/K{K}", r)
            big = g.x64.abs() >= 20.0      # +-20, +-100, +-1e4: GELU' is 1 / 0 there, codes 226 / 26 (any other code is off by >= a whole step)
            assert bool((d8[big & (g.x64 > 0)] == 226).all()) and bool((d8[big & (g.x64 < 0)] == 26).all())
            print(f"byte codes of {name}: {int(d8.min())} ... {int(d8.max())}")
    observed("numerics_gpu::served", f"{name}/epilogues/" + "+".join(ran), float(len(ran)))
    assert ran, f"{name} served none of the GELU epilogues at K = 8 or K = 512"
    if name == "REG_128":
        assert len(ran) == 6        # the general kernel serves everything


@pytest.mark.parametrize("name", list(TILE_IDS))
def test_bias_residual_fp32_every_tile(dev, observed, name):
    """``BIAS | RESIDUAL | OUT_F32`` on the part-A operands: bound A + two fp32 additions; the residual joins the fp32 accumulator
    (a result that went through bf16 first would sit on a bf16 grid + residual: 2^-9 relative, far outside)."""
    from maestro_amd import hip
    tile = TILE_IDS[name]
    K = 768  # noqa: N806
    g = torch.Generator().manual_seed(5)
    for dist in ("randn", "offset"):
        op = Operands(*nm.gemm_operands(dist, M0, N0, K), dev)
        worst = 0.0
        for layout in (NT, NN, TN):
            n = 256 if name == "PP_128" else N0
            bias = torch.randn(n, generator=g).to(dev)
            res = (torch.randn(M0, n, generator=g) * 3.0).to(dev)
            c = op.run(tile, layout, hip.OUT_F32 | hip.BIAS | hip.RESIDUAL, torch.float32, n_cols=n if n != N0 else None, bias=bias, res=res, ldr=n)
            if c is None:
                assert name == "PP_128" and layout == TN
                continue
            torch.cuda.synchronize()
            acc64, absprod = op.c64[:, :n], op.absprod[:, :n]
            b64, r64 = bias.double()[None].expand(M0, n), res.double()
            bound = nm.bias_residual_bound(acc64, absprod, K, b64, r64)
            worst = max(worst, _check(c, acc64 + b64 + r64, bound, f"C bias+res {name} {LAYOUTS[layout]} {dist}"))
            # same bits: the plain fp32 output of the same tile, plus (bias + res) or ((acc + bias) + res) in fp32, is what was stored
            c32 = _run_f32(op, tile, layout, n if n != N0 else None)
            torch.cuda.synchronize()
            ok = (c == c32 + (bias[None] + res)) | (c == (c32 + bias[None]) + res)
            assert bool(ok.all()), f"{name}: bias / residual are not added to the fp32 accumulator ({int((~ok).sum())} elements)"
        observed("numerics_gpu::C_bias_residual", f"{name}/{dist}", worst)


@pytest.mark.parametrize("name", list(TILE_IDS))
def test_backward_products_and_colsum(dev, observed, name):
    """``MULAUX`` (bf16 and byte-coded derivative), ``DGELU`` (derivative recomputed from the saved bf16 pre-activation) and the
    ``COLSUM`` side output: per 64-row block the fp32 products BEFORE their bf16 rounding are summed (include/maestro_hip.h)."""
    from maestro_amd import hip
    tile = TILE_IDS[name]
    K = 768  # noqa: N806
    n = 256 if name == "PP_128" else N0
    op = Operands(*nm.gemm_operands("randn", M0, N0, K), dev)
    g = torch.Generator().manual_seed(9)
    pre = nm.bf16_round(torch.randn(M0, n, generator=g) * 2.5).to(dev)            # saved pre-activations (bf16 values)
    d_true = nm.dgelu64(pre.double())
    d16 = d_true.float().bfloat16()
    d8 = torch.round(d_true * 200.0 + 26.0).clamp(0, 255).to(torch.uint8)
    acc64, absprod = op.c64[:, :n], op.absprod[:, :n]
    bound_a = nm.gemm_bound(absprod, K)
    nb = (M0 + 63) // 64
    served = 0

    def block_sum(t):
        pad = torch.zeros(nb * 64, n, device=dev, dtype=torch.float64)
        pad[:M0] = t
        return pad.reshape(nb, 64, n).sum(1)

    for layout in (NT, NN):
        for what, flags, aux, d64, d_err in (
                ("mulaux16", hip.MULAUX, d16, d16.double(), 0.0),
                ("mulaux8", hip.MULAUX | hip.AUX_U8, d8, nm.decode_u8(d8), 2.0 ** -23 * 1.13),      # one fp32 fma decodes the byte
                ("dgelu", hip.DGELU, pre.bfloat16(), d_true, None)):
            if d_err is None:
                d_err = nm.dgelu_err(pre.double())
            want = acc64 * d64
            # fp32 product term: (acc + bound A) (d + d_err), one more fp32 rounding
            term_bound = bound_a * (d64.abs() + d_err) + acc64.abs() * d_err + 2.0 ** -23 * want.abs()
            for cs_on in (False, True):
                cs = torch.full((nb, n), float("nan"), device=dev) if cs_on else None
                c = op.run(tile, layout, flags | (hip.COLSUM if cs_on else 0), torch.bfloat16, n_cols=n if n != N0 else None, aux_in=aux, ldaux=n,
                           colsum=cs)
                if c is None:
                    continue
                served += 1
                torch.cuda.synchronize()
                r = _check(c, want, nm.HALF_ULP_BF16 * want.abs() + term_bound, f"C {what} {name} {LAYOUTS[layout]} colsum={cs_on}")
                observed("numerics_gpu::C_backward_product", f"{name}/{LAYOUTS[layout]}/{what}/colsum{int(cs_on)}", r)
                if cs_on:
                    bound_cs = 64 * 2.0 ** -23 * block_sum(want.abs()) + block_sum(term_bound)
                    r = _check(cs, block_sum(want), bound_cs, f"C colsum {what} {name} {LAYOUTS[layout]}")
                    observed("numerics_gpu::C_colsum", f"{name}/{LAYOUTS[layout]}/{what}", r)
    observed("numerics_gpu::served", f"{name}/backward_products", float(served))
    assert served > 0 or name != "REG_128"


# ------------------------------------------------------------------------------------------------ D: atomic split-K
_D_CASES = [(512, 512, 32768), (768, 2304, 32768), (3072, 768, 32768), (768, 2304, 12808)]
_D_TILES = {"AUTO": -1, "REG_128": 0, "DMA_256": 1, "DMA_128x4": 5}


@pytest.mark.parametrize("dist", ["offset", "randn"])
@pytest.mark.parametrize("M,N,K", _D_CASES)
def test_atomic_split_k_at_token_length(dev, observed, M, N, K, dist):  # noqa: N803
    """TN wgrads accumulated atomically into a gradient slice that already holds ~10x the update.  Each launch runs twice from the
    same preload; both results obey the bound (they need not be equal: the atomics commute only in exact arithmetic)."""
    from maestro_amd import hip
    op = Operands(*nm.gemm_operands(dist, M, N, K), dev)
    g = torch.Generator().manual_seed(M + N + K)
    c0 = (torch.randn(M, N, generator=g).to(dev) * 10.0 * op.c64.abs().mean().float())
    want = c0.double() + op.c64
    bound = nm.atomic_bound(op.absprod, c0.double(), K)
    for name, tile in _D_TILES.items():
        worst = 0.0
        for rep in range(2):
            c = op.run(None if tile == -1 else tile, TN, hip.OUT_F32 | hip.ATOMIC, torch.float32, fill=c0.clone())
            assert c is not None, f"{name} declined the TN wgrad {M} x {N} x {K}"
            torch.cuda.synchronize()
            worst = max(worst, _check(c, want, bound, f"D {name} {M}x{N}x{K} {dist} run {rep}"))
        observed("numerics_gpu::D_atomic_split_k", f"{name}/{M}x{N}x{K}/{dist}", worst)
    # grouped TN: two problems (the K range in two parts) sharing one output -> atomic accumulation
    A, B = op.phys[TN]  # noqa: N806
    k1 = (K // 2 + 7) // 8 * 8
    for rep in range(2):
        c = c0.clone()
        probs = [(A[:k1], B[:k1], c, M, N, k1, M, N, N), (A[k1:], B[k1:], c, M, N, K - k1, M, N, N)]
        hip.GroupedTN(probs, dev).launch()
        torch.cuda.synchronize()
        r = _check(c, want, bound, f"D grouped_tn shared output {M}x{N}x{K} {dist} run {rep}")
    observed("numerics_gpu::D_atomic_split_k", f"GROUPED_TN/{M}x{N}x{K}/{dist}", r)


@pytest.mark.parametrize("name", list(TILE_IDS))
def test_gradient_sized_operands_scale_exactly(dev, name):
    """A * 2^-30, B * 2^8: every product and partial sum is the unscaled one times 2^-22 exactly (no underflow at these sizes), so
    both outputs equal ldexp(C, -22) of the unscaled run bit for bit: no flush, no fixed-point assumption anywhere in a tile."""
    tile = TILE_IDS[name]
    K = 768  # noqa: N806
    a, b = nm.gemm_operands("randn", M0, N0, K)
    op, ops = Operands(a, b, dev), Operands(a * 2.0 ** -30, b * 2.0 ** 8, dev)
    n = 256 if name == "PP_128" else None
    for layout in (NT, NN, TN):
        for flags, dt in ((1, torch.float32), (0, torch.bfloat16)):
            if flags:
                c, cs = _run_f32(op, tile, layout, n), _run_f32(ops, tile, layout, n)
            else:
                c, cs = op.run(tile, layout, flags, dt, n_cols=n), ops.run(tile, layout, flags, dt, n_cols=n)
            if c is None:
                assert name == "PP_128" and layout == TN
                continue
            torch.cuda.synchronize()
            assert torch.equal(torch.ldexp(c.float(), torch.tensor(-22, device=dev)), cs.float()), (name, LAYOUTS[layout], dt)


# ------------------------------------------------------------------------------------------------ E: normalisation statistics
def _ceil(observed, key, got, want64, refs, rel=False, extra=0.0):
    """|got - want64| (max; relative for rstd) against 2 x the larger error of the fp32 references (+ ``extra``, elementwise)."""
    f = nm.max_rel_err if rel else nm.max_abs_err
    errs = [f(r, want64) for r in refs]
    ceiling = nm.norm_ceiling(*errs)
    if rel:
        over = (got.double() - want64).abs() / want64.abs() - ceiling
    else:
        over = (got.double() - want64).abs() - ceiling - extra
    err = f(got, want64)
    worst = float(over.max())
    ratio = 1.0 + worst / ceiling if ceiling > 0 else (0.0 if worst <= 0 else float("inf"))   # (error - bf16 half ulp) / ceiling
    print(f"{key}: kernel {err:.3e}, references {errs[0]:.3e} / {errs[1]:.3e}, ceiling {ceiling:.3e}, ratio {ratio:.3f}")
    observed("numerics_gpu::E_norm", key + "/kernel_err", err)
    observed("numerics_gpu::E_norm", key + "/ceiling", ceiling)
    observed("numerics_gpu::E_norm", key + "/ratio", ratio)
    return worst <= 0.0, f"{key}: kernel error {err:.3e} over the ceiling {ceiling:.3e} (fp32 references: {errs[0]:.3e}, {errs[1]:.3e})"


def _ln_refs(x, gamma, beta, dy, eps):
    """fp64 truth and the two fp32 references (torch's own op; two-pass in wave order) of LayerNorm forward + backward, on the CPU."""
    out = {}
    xd = x.double().requires_grad_(True)
    gd, bd = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    m64, _, r64 = nm.stats64(x, eps)
    y64 = torch.nn.functional.layer_norm(xd, x.shape[-1:], gd, bd, eps)
    y64.backward(dy.double())
    out["f64"] = (m64, r64, y64.detach(), xd.grad, gd.grad, bd.grad)
    xt = x.clone().requires_grad_(True)
    gt, bt = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    yt, mt, rt = torch.native_layer_norm(xt, x.shape[-1:], gt, bt, eps)
    yt.backward(dy)
    out["torch"] = (mt.reshape(-1).detach(), rt.reshape(-1).detach(), yt.detach(), xt.grad, gt.grad, bt.grad)
    mw, _, rw = nm.wave_two_pass_stats(x, eps)
    xh = (x - mw[:, None]) * rw[:, None]
    dz = dy * gamma
    dxw = rw[:, None] * (dz - dz.mean(-1, keepdim=True) - xh * (dz * xh).mean(-1, keepdim=True))
    out["wave"] = (mw, rw, xh * gamma + beta, dxw, (dy * xh).sum(0), dy.sum(0))
    return out


@pytest.mark.parametrize("rows", [64, 63])
@pytest.mark.parametrize("dim", [192, 512, 768, 1024])
@pytest.mark.parametrize("kind", nm.NORM_KINDS)
def test_layernorm_off_centre(dev, observed, kind, dim, rows):
    """Generic (fp32 output / fp32 dy; dim 192; rows % 4 != 0) and straight-line (bf16, dim = 256 k, rows % 4 == 0) kernels."""
    from maestro_amd import hip
    eps = 1e-5
    x = nm.norm_inputs(kind, rows, dim)
    g = torch.Generator().manual_seed(dim + rows)
    gamma, beta = 1 + 0.2 * torch.randn(dim, generator=g), 0.1 * torch.randn(dim, generator=g)
    dy = nm.bf16_round(torch.randn(rows, dim, generator=g))
    ref = _ln_refs(x, gamma, beta, dy, eps)
    m64, r64, y64, dx64, dg64, db64 = ref["f64"]
    xd, gd, bd, dyd = x.to(dev), gamma.to(dev), beta.to(dev), dy.to(dev)
    fails = []
    for out_f32 in (True, False):
        tag = f"ln/{kind}/dim{dim}/rows{rows}/{'f32' if out_f32 else 'bf16'}"
        y = torch.full((1, rows, dim), 7.0, device=dev, dtype=torch.float32 if out_f32 else torch.bfloat16)
        mean, rstd = torch.empty(rows, device=dev), torch.empty(rows, device=dev)
        hip.layernorm_fwd(xd, rows, 0, gd, bd, y, rows, 0, mean, rstd, 1, rows, dim, eps)
        dx = torch.zeros(1, rows, dim, device=dev)
        dxb = torch.zeros(1, rows, dim, device=dev, dtype=torch.bfloat16)
        dg, db, dc = torch.zeros(dim, device=dev), torch.zeros(dim, device=dev), torch.zeros(dim, device=dev)
        ws = torch.zeros(hip.layernorm_bwd_workspace(rows, dim), device=dev)
        dres = torch.zeros(1, rows, dim, device=dev)      # (the straight-line backward is chosen only with a residual gradient)
        hip.layernorm_bwd(dyd if out_f32 else dyd.bfloat16(), rows, 0, xd, rows, 0, gd, mean, rstd, dres, dx, dxb, dg, db, dc, ws, 1, rows, dim)
        torch.cuda.synchronize()
        y, dx, dxb = y[0].cpu(), dx[0].cpu(), dxb[0].cpu()
        half = 0.0 if out_f32 else nm.HALF_ULP_BF16
        checks = [_ceil(observed, tag + "/mean", mean.cpu(), m64, (ref["torch"][0], ref["wave"][0])),
                  _ceil(observed, tag + "/rstd", rstd.cpu(), r64, (ref["torch"][1], ref["wave"][1]), rel=True),
                  _ceil(observed, tag + "/y", y, y64, (ref["torch"][2], ref["wave"][2]), extra=half * y64.abs()),
                  _ceil(observed, tag + "/dx", dx, dx64, (ref["torch"][3], ref["wave"][3])),
                  _ceil(observed, tag + "/dx_bf16", dxb, dx64, (ref["torch"][3], ref["wave"][3]), extra=nm.HALF_ULP_BF16 * dx64.abs()),
                  _ceil(observed, tag + "/dgamma", dg.cpu(), dg64, (ref["torch"][4], ref["wave"][4])),
                  _ceil(observed, tag + "/dbeta", db.cpu(), db64, (ref["torch"][5], ref["wave"][5]))]
        fails += [msg for ok, msg in checks if not ok]
        if kind == "const":      # variance 0: the output is beta exactly, the backward finite
            assert torch.equal(y.float(), (beta if out_f32 else beta.bfloat16().float())[None].expand(rows, dim)), tag
            assert bool(torch.isfinite(dx).all() and torch.isfinite(dg.cpu()).all() and torch.isfinite(db.cpu()).all()), tag
    assert not fails, "\n".join(fails)


def _gn_refs(img, gamma, beta, pos, dxg, eps):
    """GroupNorm(1, E) over whole (L x E) images + per-channel affine + positional encoding, forward and backward: fp64 truth and the
    two fp32 references (torch.native_group_norm; two-pass in wave order), on the CPU."""
    BD, L, E = img.shape  # noqa: N806
    out = {}

    def fwd_bwd(x, ga, be, po, dz, stats):
        x = x.clone().requires_grad_(True)
        ga, be = ga.clone().requires_grad_(True), be.clone().requires_grad_(True)
        mean, rstd = stats(x)
        y = (x - mean[:, None, None]) * rstd[:, None, None] * ga + be + po
        y.backward(dz)
        return mean.detach(), rstd.detach(), y.detach(), x.grad, ga.grad, be.grad

    out["f64"] = fwd_bwd(img.double(), gamma.double(), beta.double(), pos.double(), dxg.double(),
                         lambda x: (x.reshape(BD, -1).mean(-1), 1.0 / torch.sqrt(x.reshape(BD, -1).var(-1, unbiased=False) + eps)))
    # torch's own fp32 op: native_group_norm with one group (statistics + normalisation); the affine over E and its autograd in fp32
    xt = img.clone().requires_grad_(True)
    gt, bt = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    zt, mt, rt = torch.native_group_norm(xt.reshape(BD, L, E, 1), None, None, BD, L, E, 1, eps)
    yt = zt.reshape(BD, L, E) * gt + bt + pos
    yt.backward(dxg)
    out["torch"] = (mt.reshape(-1).detach(), rt.reshape(-1).detach(), yt.detach(), xt.grad, gt.grad, bt.grad)
    mw, _, rw = nm.wave_two_pass_stats(img.reshape(BD, -1), eps)
    xh = (img - mw[:, None, None]) * rw[:, None, None]
    dz = dxg * gamma
    dxw = rw[:, None, None] * (dz - dz.mean((1, 2), keepdim=True) - xh * (dz * xh).mean((1, 2), keepdim=True))
    out["wave"] = (mw, rw, xh * gamma + beta + pos, dxw, (dxg * xh).sum((0, 1)), dxg.sum((0, 1)))
    return out


@pytest.mark.parametrize("kind", nm.NORM_KINDS)
def test_groupnorm_embed_off_centre(dev, observed, kind):
    """mh_groupnorm_stats + mh_embed_finish + mh_embed_finish_bwd on 64 x 768 images (six chunks of the partial kernel each)."""
    from maestro_amd import hip
    B, D, L, E, eps = 3, 1, 64, 768, 1e-5  # noqa: N806
    img = nm.norm_inputs(kind, B * D, L * E).reshape(B * D, L, E)
    g = torch.Generator().manual_seed(23)
    gamma, beta = 1 + 0.2 * torch.randn(E, generator=g), 0.1 * torch.randn(E, generator=g)
    pos = torch.randn(L, E, generator=g)
    dxg = torch.randn(B * D, L, E, generator=g)
    ref = _gn_refs(img, gamma, beta, pos, dxg, eps)
    m64, r64, y64, dx64, dg64, db64 = ref["f64"]
    yd, gd, bd = img.reshape(-1, E).to(dev), gamma.to(dev), beta.to(dev)
    partial = torch.zeros(hip.groupnorm_partial_size(B * D, L, E), device=dev)
    stats = torch.zeros(B * D, 2, device=dev)
    hip.groupnorm_stats(yd, partial, stats, B * D, L, E, eps)
    xg = torch.full((B, D * L, E), 5.0, device=dev)
    hip.embed_finish(yd, stats, gd, bd, pos.to(dev), None, 0, 0, xg, B, D, L, E, 0, D * L)
    dyc = torch.zeros(B * D * L, E, device=dev, dtype=torch.bfloat16)
    dg, db, sums = torch.zeros(E, device=dev), torch.zeros(E, device=dev), torch.zeros(B * D, 2, device=dev)
    hip.embed_finish_bwd(dxg.to(dev), yd, stats, gd, dyc, dg, db, sums, B, D, L, E, 0, D * L)
    torch.cuda.synchronize()
    stats = stats.cpu()
    tag = f"gn/{kind}"
    checks = [_ceil(observed, tag + "/mean", stats[:, 0], m64, (ref["torch"][0], ref["wave"][0])),
              _ceil(observed, tag + "/rstd", stats[:, 1], r64, (ref["torch"][1], ref["wave"][1]), rel=True),
              _ceil(observed, tag + "/y", xg.cpu(), y64, (ref["torch"][2], ref["wave"][2])),
              _ceil(observed, tag + "/dx_bf16", dyc.cpu().reshape(B * D, L, E), dx64, (ref["torch"][3], ref["wave"][3]),
                    extra=nm.HALF_ULP_BF16 * dx64.abs()),
              _ceil(observed, tag + "/dgamma", dg.cpu(), dg64, (ref["torch"][4], ref["wave"][4])),
              _ceil(observed, tag + "/dbeta", db.cpu(), db64, (ref["torch"][5], ref["wave"][5]))]
    fails = [msg for ok, msg in checks if not ok]
    if kind == "const":          # variance 0: beta plus the encodings, exactly; finite backward
        assert torch.equal(xg.cpu(), (beta + pos)[None].expand(B * D, L, E)), tag
        assert bool(torch.isfinite(dyc.float()).all() and torch.isfinite(dg).all() and torch.isfinite(db).all()), tag
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("P,C,norm_bands", [(16, 4, (1, 3)), (8, 3, (3,))])
@pytest.mark.parametrize("kind", nm.NORM_KINDS)
def test_patch_target_normalisation_off_centre(dev, observed, kind, P, C, norm_bands):  # noqa: N803
    """mh_patchify with normalise=True: per patch and band group, unbiased variance, eps 1e-6 (two-pass in the kernel)."""
    from maestro_amd import hip
    from oracle import mae as om
    BD, S, eps = 2, 64, 1e-6  # noqa: N806
    gsz = S // P
    K = C * P * P  # noqa: N806
    Kpad = (K + 31) // 32 * 32  # noqa: N806
    img = nm.norm_inputs(kind, BD * C, S * S).reshape(BD, C, S, S)
    if kind == "const":          # constant over the whole band group, not only per channel
        img = nm.norm_inputs(kind, BD, 1).reshape(BD, 1, 1, 1).expand(BD, C, S, S).contiguous()
    target = torch.zeros(BD * gsz * gsz, K, device=dev)
    cols = torch.zeros(BD * gsz * gsz, Kpad, device=dev, dtype=torch.bfloat16)
    nb = torch.tensor(norm_bands, dtype=torch.int32, device=dev)
    hip.patchify(img.to(dev), cols, target, BD, C, S, P, Kpad, nb, len(norm_bands), True, False)
    torch.cuda.synchronize()
    tgt = om.patch_view(img[None], gsz)[0]                 # [BD, L, PP, C]
    want, r_torch, r_wave = [], [], []
    for grp in torch.split(tgt, list(norm_bands), dim=-1):
        flat = grp.reshape(BD, gsz * gsz, -1)
        m64, _, r64 = nm.stats64(flat, eps, unbiased=True)
        want.append((grp.double() - m64[..., None, None]) * r64[..., None, None])
        mt, vt = flat.mean(-1), flat.var(-1, unbiased=True)       # torch's own fp32 reductions (the oracle's form)
        r_torch.append((grp - mt[..., None, None]) / torch.sqrt(vt + eps)[..., None, None])
        mw, _, rw = nm.wave_two_pass_stats(flat, eps, unbiased=True)
        r_wave.append((grp - mw[..., None, None]) * rw[..., None, None])
    want, r_torch, r_wave = (torch.cat(t, -1).reshape(-1, K) for t in (want, r_torch, r_wave))
    ok, msg = _ceil(observed, f"patch_target/{kind}/P{P}", target.cpu(), want, (r_torch, r_wave))
    if kind == "const":
        assert float(target.abs().max()) == 0.0
    assert ok, msg
