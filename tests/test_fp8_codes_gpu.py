"""Every place of the fp8 step where an fp32 value becomes an fp8 byte, held to BIT equality against tests/fp8_codes.py.

The fused sites get inputs whose pre-cast fp32 value is known exactly: ``gamma = 0`` makes a LayerNorm output its ``beta``, zero
operands make a GEMM output its ``bias``, a one-term dot product of powers of two and four-bit values makes it an exact product,
a zero gradient with zero moments makes AdamW return its parameter.  The values are the code values, the ties and their fp32
neighbours of ``boundary_values`` (per-tensor sites) and the blocks of ``mx_edge_blocks`` (MX sites), so a cast of the
bf16-rounded value, another tie rule, a wrong saturation edge or an absmax taken after the scale changes a byte.  Every
comparison is ``torch.equal`` on bytes or on the raw bits of fp32 / bf16 values."""

import numpy as np
import pytest
import torch

from tests import fp8_codes as fc

pytestmark = pytest.mark.gpu

TILES = ["128", "128d", "256"]
SENTINEL = 0x5A


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _bits(t: torch.Tensor) -> torch.Tensor:
    t = t.detach().cpu().contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def _row_bits(amax_row: torch.Tensor) -> int:
    """Bits of the maximum over an amax row (non-negative floats and NaN: the integer order is the kernels' order)."""
    return int(_bits(amax_row).max())


def _nonzero_e4m3_set() -> torch.Tensor:
    b = fc.boundary_values(fc.E4M3)
    return b[b != 0]


def _slices(values: torch.Tensor, width: int, step: int = 1):
    """Successive ``width``-element slices that together hold every element (the last one wraps around)."""
    n = values.numel()
    idx = torch.arange(-(-n // width) * width) % n
    return [values[idx[i: i + width]] for i in range(0, idx.numel(), width * step)]


# ---------------------------------------------------------------------------------------------------- a. mh_quant_batched
@pytest.fixture(scope="module")
def quant_case():
    """Four jobs: the boundary set of each format as an fp32 source, every finite bf16 value as a bf16 source for each format;
    zero-padded to [rows, 36]; per slot another power-of-two scale.  Slots 0 and 5 belong to nobody."""
    jobs = []
    for slot, (kind, fmt, s) in enumerate([("f32", fc.E4M3, 2.0 ** -7), ("f32", fc.E5M2, 2.0 ** 4), ("bf16", fc.E4M3, 2.0 ** 4),
                                           ("bf16", fc.E5M2, 2.0 ** -7)], start=1):
        v = fc.boundary_values(fmt) if kind == "f32" else fc.bf16_finite()
        cols = 36
        rows = -(-v.numel() // cols)
        x = torch.zeros(rows * cols, dtype=v.dtype)
        x[: v.numel()] = v
        x = x.view(rows, cols)
        jobs.append(dict(x=x, fmt=fmt, slot=slot, scale=s, want=fc.quantise(x.float(), s, fmt), amax=fc.absmax_bits(x.float())))
    return jobs


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_quant_batched_codes_and_absmax(dev, quant_case, mode):
    """Mode 0 folds max |x| and writes no byte, mode 1 casts and leaves the amax rows alone, mode 2 does both; ``dst`` and the
    transposed ``dst_t`` equal ``encode(clamp(x * scale[slot]))``; a slot's row maximum has the bits of max |x|."""
    from maestro_amd import hip
    sc = hip.Fp8Scales(6, dev)
    sc.scale.fill_(float("nan"))                                     # a slot nobody may read
    table, outs = [], []
    for jb in quant_case:
        sc.scale[jb["slot"]] = jb["scale"]
        rows, cols = jb["x"].shape
        dst = torch.full((rows, cols), SENTINEL, dtype=torch.uint8, device=dev)
        dst_t = torch.full((cols, rows), SENTINEL, dtype=torch.uint8, device=dev)
        table.append(dict(src=jb["x"].to(dev), dst=dst, dst_t=dst_t, slot=jb["slot"], format=jb["fmt"]))
        outs.append((dst, dst_t))
    hip.QuantBatch(table, sc, dev).launch(mode)
    torch.cuda.synchronize()
    for jb, (dst, dst_t) in zip(quant_case, outs):
        if mode == 0:
            assert bool((dst.cpu() == SENTINEL).all()) and bool((dst_t.cpu() == SENTINEL).all()), "mode 0 wrote bytes"
        else:
            assert torch.equal(dst.cpu(), jb["want"]), (jb["slot"], (dst.cpu() != jb["want"]).nonzero()[:8])
            assert torch.equal(dst_t.cpu(), jb["want"].t().contiguous()), jb["slot"]
        assert _row_bits(sc.amax[jb["slot"]]) == (0 if mode == 1 else jb["amax"]), (jb["slot"], mode)
    assert _row_bits(sc.amax[0]) == 0 and _row_bits(sc.amax[5]) == 0


# ---------------------------------------------------------------------------------------------------- b. mh_layernorm_fwd_fp8
LN_ROWS, LN_XMAP, LN_YMAP = 5, (7, 1), (8, 2)      # 5 rows (4 per workgroup) through row maps (L, off) with off != 0


def _ln_inputs(dev, dim):
    g = torch.Generator().manual_seed(dim)
    x = (torch.randn(LN_XMAP[0], dim, generator=g) * 3 + 0.5).to(dev)                 # finite, non-zero variance in every row
    return x, torch.zeros(dim, device=dev)


@pytest.mark.parametrize("dim", [256, 512, 768, 1024, 192, 384, 2048])      # four straight-line widths, three of the generic kernel
def test_layernorm_fp8_copy_is_the_cast_of_the_fp32_value(dev, dim):
    """``gamma = 0``: ``o = (x - mu) rs 0 + beta`` is ``beta`` exactly for a non-zero beta (with or without fma contraction), so
    ``y8 == encode(clamp(beta s))``, ``y == bf16(beta)`` (round to nearest even) and the amax has the bits of max |beta|.  The
    whole boundary set passes through at dim 1024 and 384 under each scale, one slice per scale elsewhere."""
    from maestro_amd import hip
    x, gamma = _ln_inputs(dev, dim)
    values = _nonzero_e4m3_set()
    every = dim in (1024, 384)
    rows = torch.arange(LN_ROWS) + LN_YMAP[1]
    mean, rstd = torch.zeros(LN_ROWS, device=dev), torch.zeros(LN_ROWS, device=dev)
    for si, s in enumerate(fc.SCALES):
        sl = _slices(values, dim)
        for beta in (sl if every else sl[si % len(sl): si % len(sl) + 1]):
            y = torch.full((LN_YMAP[0], dim), -2.0, dtype=torch.bfloat16, device=dev)
            y8 = torch.full((LN_YMAP[0], dim), SENTINEL, dtype=torch.uint8, device=dev)
            amax, scale = torch.zeros(hip.AMAX_PITCH, device=dev), torch.tensor([s], device=dev)
            hip.layernorm_fwd_fp8(x, LN_XMAP[0], LN_XMAP[1], gamma, beta.to(dev), y, LN_YMAP[0], LN_YMAP[1], mean, rstd, 1, LN_ROWS, dim,
                                  y8, scale, amax)
            torch.cuda.synchronize()
            want8, want16 = fc.quantise(beta, s, fc.E4M3), _bits(fc.bf16_rne(beta))
            y8h, yh = y8.cpu(), _bits(y)
            for r in rows.tolist():
                assert torch.equal(y8h[r], want8), (dim, s, r, (y8h[r] != want8).nonzero()[:8].flatten().tolist())
                assert torch.equal(yh[r], want16), (dim, s, r)
            for r in set(range(LN_YMAP[0])) - set(rows.tolist()):
                assert bool((y8h[r] == SENTINEL).all()) and bool((y[r].cpu() == -2.0).all()), "a row outside the map was written"
            assert _row_bits(amax) == fc.absmax_bits(beta), (dim, s)


# ---------------------------------------------------------------------------------------------------- c. mh_gemm_fp8 output copies
GM, GN, GK = 130, 264, 128          # ragged against every tile


@pytest.mark.parametrize("tile", TILES)
def test_gemm_fp8_e4m3_copy_is_the_cast_of_the_fp32_value(dev, tile, monkeypatch):
    """Forward form (BIAS, bf16 output) with an all-zero A8: the epilogue value is ``0 alpha + bias[n] = bias[n]``.  The whole
    boundary set passes through under each scale: ``c8 == encode(clamp(bias s8))`` in every row, ``C == bf16(bias)``, amax bits
    those of max |bias|."""
    from maestro_amd import hip
    monkeypatch.setenv("MH_FP8_TILE", tile)
    g = torch.Generator().manual_seed(5)
    A8 = torch.zeros(GM, GK, dtype=torch.uint8, device=dev)  # noqa: N806
    finite = torch.cat([torch.arange(0x00, 0x7F), torch.arange(0x80, 0xFF)]).to(torch.uint8)
    B8 = finite[torch.randint(0, finite.numel(), (GN, GK), generator=g)].to(dev)  # noqa: N806
    da, db = torch.tensor([0.5], device=dev), torch.tensor([4.0], device=dev)
    values = _nonzero_e4m3_set()
    for s in fc.SCALES:
        for bias in _slices(values, GN):
            C = torch.full((GM, GN), -2.0, dtype=torch.bfloat16, device=dev)  # noqa: N806
            c8 = torch.full((GM, GN), SENTINEL, dtype=torch.uint8, device=dev)
            amax, s8 = torch.zeros(hip.AMAX_PITCH, device=dev), torch.tensor([s], device=dev)
            hip.gemm_fp8(GM, GN, GK, A8, GK, B8, GK, C, GN, da, db, flags=hip.BIAS, bias=bias.to(dev), c8=c8, ldc8=GN, c8_scale=s8,
                         c8_amax=amax)
            torch.cuda.synchronize()
            want8 = fc.quantise(bias, s, fc.E4M3).expand(GM, GN)
            want16 = _bits(fc.bf16_rne(bias)).expand(GM, GN)
            assert torch.equal(c8.cpu(), want8), (tile, s, (c8.cpu() != want8).nonzero()[:8].tolist())
            assert torch.equal(_bits(C), want16), (tile, s)
            assert _row_bits(amax) == fc.absmax_bits(bias), (tile, s)


# descale_a, descale_b of the dgrad case: powers of two, and a pair whose product 2 (1 + 2^-10) puts an output t (1 + 2^-10) within
# a quarter of a bf16 ulp of an e5m2 tie t -- one bf16 factor alone never comes closer to a tie than half a bf16 ulp, so only this
# pair tells a cast of the bf16-rounded output (which lands ON the tie and goes to the even code) from the cast of the fp32 value
DGRAD_DESCALES = [(0.5, 4.0), (1.0 + 2.0 ** -10, 2.0)]


@pytest.fixture(scope="module", params=DGRAD_DESCALES, ids=["pow2", "near-tie"])
def dgrad_case(request):
    """Operands of the e5m2 dgrad form with an exact accumulator: row m of A8 holds one power of two 2^((m mod 7) - 3) at column
    m mod K, B8 holds non-zero e4m3 code values, aux is bf16 from a short table by (row, column).  Each output is ONE product of
    1 + 4 + 11 + 8 significant bits at most (power of two, e4m3 value, descales, aux): exact in fp32 at every step of the epilogue,
    computed here in float64."""
    da, db = request.param
    g = torch.Generator().manual_seed(8)
    m_idx = torch.arange(GM)
    a_exp = (m_idx % 7) - 3
    A8 = torch.zeros(GM, GK, dtype=torch.uint8)  # noqa: N806
    A8[m_idx, m_idx % GK] = ((a_exp + 15) << 2).to(torch.uint8)                      # e5m2 code of 2^a_exp
    nonzero = torch.cat([torch.arange(0x01, 0x7F), torch.arange(0x81, 0xFF)]).to(torch.uint8)
    B8 = nonzero[torch.randint(0, nonzero.numel(), (GN, GK), generator=g)]  # noqa: N806
    table = torch.tensor([1.0, 1.0 + 2.0 ** -7, 1.0 - 2.0 ** -8, 2.0, -1.0, 0.5, -(1.0 + 2.0 ** -7), 4.0], dtype=torch.float64)
    aux = table[(m_idx[:, None] * 3 + torch.arange(GN)[None, :]) % table.numel()]
    assert torch.equal(torch.from_numpy(fc.decode(A8[m_idx, m_idx % GK], fc.E5M2)).double(), torch.exp2(a_exp.double()))
    b_val = torch.from_numpy(fc.decode(B8, fc.E4M3)).double()                        # [N, K]
    acc = torch.exp2(a_exp.double())[:, None] * b_val[:, m_idx % GK].t()             # what the MFMA leaves: one exact product
    alpha = float(np.float32(da) * np.float32(db))
    assert alpha == da * db and torch.equal((acc * alpha).float().double(), acc * alpha)
    val = acc * alpha * aux
    assert torch.equal(val.float().double(), val) and bool((val != 0).all()) and torch.equal(aux.to(torch.bfloat16).double(), aux)
    return dict(A8=A8, B8=B8, aux=aux.to(torch.bfloat16), val=val.float(), da=da, db=db)


@pytest.mark.parametrize("tile", TILES)
def test_gemm_fp8_e5m2_copy_is_the_cast_of_the_fp32_value(dev, dgrad_case, tile, monkeypatch):
    """Dgrad form (MULAUX | C8_E5M2, e5m2 A operand) on the exact products of ``dgrad_case``: with aux = 1 an output is an e5m2
    code value or a tie (e4m3 has one mantissa bit more), with the neighbours of 1 it sits just beside one; rows differ, so a
    row-index error in the copy shows; with the second descale pair it sits within a quarter of a bf16 ulp of a tie.
    ``c8 == encode(clamp(v s8))``, ``C == bf16(v)``, amax bits those of max |v|."""
    from maestro_amd import hip
    monkeypatch.setenv("MH_FP8_TILE", tile)
    c = dgrad_case
    A8, B8, aux = c["A8"].to(dev), c["B8"].to(dev), c["aux"].to(dev)  # noqa: N806
    da, db = torch.tensor([c["da"]], device=dev), torch.tensor([c["db"]], device=dev)
    want16 = _bits(fc.bf16_rne(c["val"]))
    ties = through_bf16 = 0
    for s in fc.SCALES:
        C = torch.full((GM, GN), -2.0, dtype=torch.bfloat16, device=dev)  # noqa: N806
        c8 = torch.full((GM, GN), SENTINEL, dtype=torch.uint8, device=dev)
        amax, s8 = torch.zeros(hip.AMAX_PITCH, device=dev), torch.tensor([s], device=dev)
        hip.gemm_fp8(GM, GN, GK, A8, GK, B8, GK, C, GN, da, db, flags=hip.MULAUX | hip.C8_E5M2, a_format=hip.FP8_E5M2, aux_in=aux,
                     ldaux=GN, c8=c8, ldc8=GN, c8_scale=s8, c8_amax=amax)
        torch.cuda.synchronize()
        want8 = fc.quantise(c["val"], s, fc.E5M2)
        ties += int((torch.from_numpy(fc._encode(fc.scaled_f32(c["val"], s).clip(-57344, 57344), fc.E5M2, mode="away")) != want8.flatten()).sum())
        through_bf16 += int((fc.quantise(fc.bf16_rne(c["val"]).float(), s, fc.E5M2) != want8).sum())
        assert torch.equal(c8.cpu(), want8), (tile, s, (c8.cpu() != want8).nonzero()[:8].tolist())
        assert torch.equal(_bits(C), want16), (tile, s)
        assert _row_bits(amax) == fc.absmax_bits(c["val"]), (tile, s)
    # the data holds what it claims: exact ties between e5m2 codes with power-of-two descales, values a cast through bf16 gets wrong with the other pair
    assert ties > 1000 if (c["da"], c["db"]) == DGRAD_DESCALES[0] else through_bf16 > 1000


# ---------------------------------------------------------------------------------------------------- d. mh_adamw_fp8
def test_adamw_fp8_shadow_is_the_cast_of_the_parameter(dev):
    """g = 0, m = v = 0, wd = 0: the update is exactly zero, so p comes back bit for bit (both zeros included) and
    ``p8 == encode(clamp(p scale[slot]))``; the set lies once in each of two slots with different scales, a block of the map
    between them says -1 and keeps its bytes; amax bits per slot."""
    from maestro_amd import hip
    values = fc.boundary_values(fc.E4M3)
    span = -(-values.numel() // 64) * 64
    n = 2 * span + 64
    p0 = torch.zeros(n)
    p0[: values.numel()] = values
    p0[span: span + 64] = 3.0                                        # the unmapped block
    p0[span + 64: span + 64 + values.numel()] = values
    slot_map = torch.zeros(n // 64, dtype=torch.int16)
    slot_map[span // 64] = -1
    slot_map[span // 64 + 1:] = 1
    regions = ((0, 0, span), (1, span + 64, n))
    for scales in ((2.0 ** -7, 1.0), (1.0, 2.0 ** 4), (2.0 ** 4, 2.0 ** -7)):
        p, grad, m, v = p0.clone().to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
        half = torch.full((n,), -2.0, dtype=torch.bfloat16, device=dev)
        p8 = torch.full((n,), 7, dtype=torch.uint8, device=dev)
        scale, amax = torch.tensor(scales, device=dev), torch.zeros(2, hip.AMAX_PITCH, device=dev)
        hip.adamw_fp8(p, grad, m, v, half, p8, slot_map.to(dev), scale, amax, n, 1e-3, 0.9, 0.99, 1e-8, 0.0, 1)
        torch.cuda.synchronize()
        assert torch.equal(_bits(p), _bits(p0)), "a zero update changed a parameter's bits"
        assert torch.equal(_bits(half), _bits(fc.bf16_rne(p0)))
        assert not bool(_bits(m).any()) and not bool(_bits(v).any())
        for slot, lo, hi in regions:
            want = fc.quantise(p0[lo:hi], scales[slot], fc.E4M3)
            assert torch.equal(p8[lo:hi].cpu(), want), (scales, slot, (p8[lo:hi].cpu() != want).nonzero()[:8].flatten().tolist())
            assert _row_bits(amax[slot]) == fc.absmax_bits(p0[lo:hi]), (scales, slot)
        assert bool((p8[span: span + 64].cpu() == 7).all())


# ---------------------------------------------------------------------------------------------------- e. mh_fp8_update_scales
N_SLOTS = 403                       # not a multiple of the 4 slots per workgroup


def _amax_values(fmax):
    """fmax 2^-k and its two fp32 neighbours for every k in -130 .. 130 where fmax 2^-k is an fp32 number (across and beyond the
    +-100 clamp of the exponent, down into the fp32 subnormals), then the specials."""
    vals = []
    for k in range(-130, 131):
        with np.errstate(over="ignore", under="ignore"):
            a0 = np.float32(np.ldexp(np.float64(fmax), -k))
        if not np.isfinite(a0) or a0 == 0 or float(a0) != float(np.ldexp(np.float64(fmax), -k)):
            continue
        vals += [a for a in (np.nextafter(a0, np.float32(0)), a0, np.nextafter(a0, np.float32(np.inf))) if np.isfinite(a) and a > 0]
    sub = np.array([1, 2, 0x1234, 1 << 22, (1 << 23) - 1], dtype=np.uint32).view(np.float32)
    vals += list(sub) + [np.float32(0), np.float32(np.inf), np.float32(np.nan), np.finfo(np.float32).max, np.float32(1.0), np.float32(3.0e38)]
    return np.array(vals, dtype=np.float32)


@pytest.mark.parametrize("margin", [0, 1, 2])
@pytest.mark.parametrize("fmt", [fc.E4M3, fc.E5M2])
def test_update_scales_is_the_exact_rule(dev, fmt, margin):
    """403 slots per launch, called on the slice [1, 404) of 405-slot tables.  Each amax sits in another sub-slot of its row with
    smaller decoys beside it.  ``scale`` has the bits of ``scale_rule`` (the exact largest power of two with amax scale <= fmax
    2^-margin, exponent clamped to +-100; 1 for an empty slot), ``descale`` those of 1 / scale, NaN both for an inf / NaN amax;
    the rows are reset; the neighbours of the slice keep their bits."""
    from maestro_amd import hip
    fmax = fc.FMAX[fmt]
    vals = _amax_values(fmax)
    idx = np.arange(-(-vals.size // N_SLOTS) * N_SLOTS) % vals.size
    bad = []
    for chunk in idx.reshape(-1, N_SLOTS):
        a = vals[chunk]
        rows = np.zeros((N_SLOTS + 2, hip.AMAX_PITCH), dtype=np.float32)
        rows[0, ::64], rows[-1, ::64] = 5.0, 6.0                     # the neighbours of the slice
        for i, ai in enumerate(a):
            sub = (7 * i) % 32
            decoy = np.float32(1.0) if not np.isfinite(ai) else np.float32(ai / 2)
            rows[1 + i, ((sub + 5) % 32) * 64] = decoy
            rows[1 + i, ((sub + 17) % 32) * 64] = decoy
            rows[1 + i, sub * 64] = ai
        amax = torch.from_numpy(rows).to(dev)
        scale, descale = torch.full((N_SLOTS + 2,), 7.0, device=dev), torch.full((N_SLOTS + 2,), 9.0, device=dev)
        hip.call("mh_fp8_update_scales", amax[1:-1], scale[1:-1], descale[1:-1], hip._I(N_SLOTS), hip._F(fmax), hip._I(margin))
        torch.cuda.synchronize()
        want = np.array([fc.scale_rule(float(ai), fmax, margin) for ai in a], dtype=np.float32)
        got_s, got_d = scale.cpu().numpy(), descale.cpu().numpy()
        assert got_s[0] == 7.0 and got_s[-1] == 7.0 and got_d[0] == 9.0 and got_d[-1] == 9.0
        after = amax.cpu().numpy()
        assert np.array_equal(after[0].view(np.uint32), rows[0].view(np.uint32)) and np.array_equal(after[-1].view(np.uint32), rows[-1].view(np.uint32))
        assert not after[1:-1].view(np.uint32).any(), "an amax row of the slice was not reset"
        nan = np.isnan(want)
        assert np.isnan(got_s[1:-1][nan]).all() and np.isnan(got_d[1:-1][nan]).all()
        with np.errstate(divide="ignore"):
            want_d = (np.float32(1) / want)
        ok = (got_s[1:-1].view(np.uint32) == want.view(np.uint32)) & (got_d[1:-1].view(np.uint32) == want_d.view(np.uint32))
        bad += [(float(a[i]).hex(), float(got_s[1 + i]), float(want[i])) for i in np.flatnonzero(~ok & ~nan)]
    print(f"[update_scales] format {fmt} margin {margin}: {len(bad)} of {idx.size} slots differ from the exact rule")
    assert not bad, (len(bad), bad[:12])


# ---------------------------------------------------------------------------------------------------- f. MX sites
@pytest.fixture(scope="module")
def mx_case():
    """The edge blocks and their reference, computed once: blocks are quantised independently, so every site's expectation is a
    gather from here."""
    blocks = fc.mx_edge_blocks()
    q, s, finite = fc.mx_ref(blocks)
    assert bool(finite.all()) and int(s.min()) == 0 and int(s.max()) == 247
    return dict(blocks=blocks, q=q, s=s[:, 0])


def _block_slices(n_blocks, per_row, step=1):
    idx = torch.arange(-(-n_blocks // per_row) * per_row) % n_blocks
    return [idx[i: i + per_row] for i in range(0, idx.numel(), per_row * step)]


def test_quant_mx_on_the_edge_blocks(dev, mx_case):
    """Scale bytes 0 .. 247 and the ``m > 1.75`` switch at every bf16 exponent; source pitch above cols, destination and scale
    padding untouched."""
    from maestro_amd import hip
    blocks = mx_case["blocks"]
    per_row = 3
    rows, cols = blocks.shape[0] // per_row, 32 * per_row
    assert rows * per_row == blocks.shape[0]
    src = torch.full((rows, cols + 8), float("nan"), dtype=torch.bfloat16, device=dev)
    src[:, :cols] = blocks.view(rows, cols).to(dev)
    dst = torch.full((rows, cols + 16), SENTINEL, dtype=torch.uint8, device=dev)
    sc = torch.full((rows, per_row + 5), SENTINEL, dtype=torch.uint8, device=dev)
    hip.QuantMxBatch([dict(src=src[:, :cols], dst=dst[:, :cols], scales=sc[:, :per_row])], dev).launch()
    torch.cuda.synchronize()
    got_s, want_s = sc[:, :per_row].cpu(), mx_case["s"].view(rows, per_row)
    assert torch.equal(got_s, want_s), (got_s != want_s).nonzero()[:8].tolist()
    got_q, want_q = dst[:, :cols].cpu(), mx_case["q"].view(rows, cols)
    assert torch.equal(got_q, want_q), (got_q != want_q).nonzero()[:8].tolist()
    assert bool((dst[:, cols:].cpu() == SENTINEL).all()) and bool((sc[:, per_row:].cpu() == SENTINEL).all())


@pytest.mark.parametrize("dim,step", [(1024, 1), (512, 2), (384, 1)])      # straight-line, straight-line, generic kernel
def test_layernorm_mx_copy_on_the_edge_blocks(dev, mx_case, dim, step):
    """The beta construction of the per-tensor test: the values are bf16 numbers, so ``y == beta`` bit for bit and ``y8``,
    ``y8s`` are the MX rule applied to it.  Every block passes through at dim 1024 and 384, every second slice at 512."""
    from maestro_amd import hip
    from maestro_amd.fp8 import mx_scale_cols
    x, gamma = _ln_inputs(dev, dim)
    blocks, nb = mx_case["blocks"], dim // 32
    rows = (torch.arange(LN_ROWS) + LN_YMAP[1]).tolist()
    mean, rstd = torch.zeros(LN_ROWS, device=dev), torch.zeros(LN_ROWS, device=dev)
    lds = mx_scale_cols(dim)
    for idx in _block_slices(blocks.shape[0], nb, step):
        beta16 = blocks[idx].reshape(dim)
        y = torch.full((LN_YMAP[0], dim), -2.0, dtype=torch.bfloat16, device=dev)
        y8 = torch.full((LN_YMAP[0], dim), SENTINEL, dtype=torch.uint8, device=dev)
        ys = torch.full((LN_YMAP[0], lds), SENTINEL, dtype=torch.uint8, device=dev)
        hip.layernorm_fwd_mx(x, LN_XMAP[0], LN_XMAP[1], gamma, beta16.float().to(dev), y, LN_YMAP[0], LN_YMAP[1], mean, rstd, 1, LN_ROWS,
                             dim, y8, ys, lds)
        torch.cuda.synchronize()
        want_q, want_s, want_y = mx_case["q"][idx].reshape(dim), mx_case["s"][idx], _bits(beta16)
        yh, y8h, ysh = _bits(y), y8.cpu(), ys.cpu()
        for r in rows:
            assert torch.equal(yh[r], want_y), (dim, int(idx[0]), r)
            assert torch.equal(ysh[r, :nb], want_s), (dim, int(idx[0]), r, ysh[r, :nb].tolist(), want_s.tolist())
            assert torch.equal(y8h[r], want_q), (dim, int(idx[0]), r, (y8h[r] != want_q).nonzero()[:8].flatten().tolist())
        for r in set(range(LN_YMAP[0])) - set(rows):
            assert bool((y8h[r] == SENTINEL).all()) and bool((ysh[r] == SENTINEL).all())
        assert bool((ysh[:, nb:] == SENTINEL).all())


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("N,step", [(1024, 1), (288, 4)])
def test_gemm_mx_copy_on_the_edge_blocks(dev, mx_case, N, step, tile, monkeypatch):  # noqa: N803
    """The bias construction of the per-tensor test with zero operands under scale bytes 127: ``C == bias`` in bf16, ``c8`` and
    ``c8_scales`` are the MX rule applied to it -- the four-lane block maximum of the GEMM epilogue on extreme exponents.  Every
    block passes through at N = 1024, every fourth slice at N = 288 (ragged against every tile)."""
    from maestro_amd import hip
    from maestro_amd.fp8 import mx_scale_cols
    monkeypatch.setenv("MH_FP8_TILE", tile)
    M, K = GM, GK  # noqa: N806
    A8, B8 = torch.zeros(M, K, dtype=torch.uint8, device=dev), torch.zeros(N, K, dtype=torch.uint8, device=dev)  # noqa: N806
    sa = torch.full((M, mx_scale_cols(K)), 127, dtype=torch.uint8, device=dev)
    sb = torch.full((N, mx_scale_cols(K)), 127, dtype=torch.uint8, device=dev)
    blocks, nb, lds = mx_case["blocks"], N // 32, mx_scale_cols(N)
    for idx in _block_slices(blocks.shape[0], nb, step):
        bias16 = blocks[idx].reshape(N)
        C = torch.full((M, N), -2.0, dtype=torch.bfloat16, device=dev)  # noqa: N806
        c8 = torch.full((M, N), SENTINEL, dtype=torch.uint8, device=dev)
        c8s = torch.full((M, lds), SENTINEL, dtype=torch.uint8, device=dev)
        hip.gemm_mx(M, N, K, A8, K, sa, sa.stride(0), B8, K, sb, sb.stride(0), C, N, flags=hip.BIAS, bias=bias16.float().to(dev),
                    c8=c8, ldc8=N, c8_scales=c8s, ldc8s=lds)
        torch.cuda.synchronize()
        want_q, want_s = mx_case["q"][idx].reshape(1, N).expand(M, N), mx_case["s"][idx].reshape(1, nb).expand(M, nb)
        assert torch.equal(_bits(C), _bits(bias16).reshape(1, N).expand(M, N)), (tile, N, int(idx[0]))
        got_s = c8s.cpu()
        assert torch.equal(got_s[:, :nb], want_s), (tile, N, int(idx[0]), (got_s[:, :nb] != want_s).nonzero()[:8].tolist())
        assert torch.equal(c8.cpu(), want_q), (tile, N, int(idx[0]), (c8.cpu() != want_q).nonzero()[:8].tolist())
        assert bool((got_s[:, nb:] == SENTINEL).all())
