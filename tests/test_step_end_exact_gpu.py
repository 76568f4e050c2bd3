"""The kernels that close a training step against EXACT references: the masked reconstruction loss (all six entries), the column
sums (plain, partial + ordered reduce, batched), the mask-token gradient (four entries) and the masked-token counts.

They sum in an order the hardware chooses, so random operands only admit a bound that grows with the number of terms.  Here
the operands are integer-valued (tests/exact_sums.py): every term and every partial sum is an integer multiple of one power of
two below 2^24 of it, no fp32 addition rounds, and the kernel must equal the int64 / fp64 value bit for bit -- at the shapes
the step launches (several rows per wave in the loss, every ``rows_per_block`` of ``mh_colsum``, several strips and idle
threads in the token gradient), where one dropped, doubled or misplaced row is a failure of any size.  Each test calls
``is_order_free`` on its own inputs, so a case cannot silently lose its exactness.  tests/test_step_end_selfcheck.py checks
the generators and the predicate on the CPU.

One random-valued loss case per norm keeps the rounding of real operands under a derived bound (see ``test_masked_loss_random``).
"""

from __future__ import annotations

import math

import pytest
import torch

from tests import exact_sums as ex
from tests import numerics as nm

pytestmark = pytest.mark.gpu
F32, BF16 = torch.float32, torch.bfloat16
U = nm.U_F32


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _assert_exact(got: torch.Tensor, want64: torch.Tensor, what: str) -> None:
    """``got`` (fp32 / bf16) holds exactly the fp64 / int64 values ``want64``."""
    want = want64.double().to(got.device)
    assert torch.equal(want.to(got.dtype).double(), want), f"{what}: the reference is not representable in {got.dtype}"
    g = got.double()
    if not torch.equal(g, want):
        bad = (g != want) | torch.isnan(g)
        idx = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} values differ, first at {idx}: got "
                             f"{g[tuple(idx)].item()!r}, want {want[tuple(idx)].item()!r}")


# ------------------------------------------------------------------------------------------------ masked loss
def loss_rows_per_wave(rows: int) -> int:
    """The rule of csrc/loss.hip restated: about 1024 workgroups per launch, at most 16 rows per wave."""
    return min(16, max(1, rows // 4096))


LOSS_WEIGHT = {4: 0.5, 260: 260.0 / 512.0, 768: 0.75, 1024: 0.5}       # PPC / 2^s: coef = weight / (2^j PPC) is a power of two
# (B, Lm, PPC, rows per wave)
LOSS_CASES = [(3, 2730, 4, 1), (5, 1639, 4, 2), (5, 2458, 4, 3), (5, 13109, 4, 16), (5, 1639, 260, 2), (3, 13, 768, 1), (3, 13, 1024, 1)]
TOK_OFF, TAIL = 3, 5
WINDOW = (5, 2, 2)          # tgt_C, tgt_c0, n_g: tgt_c0 > 0 and n_g < tgt_C


def _n_selected(rows: int, ppc: int) -> int:
    """The largest 2^j with at most half of the rows selected and ``2^j PPC 49 < 2^24`` (49 / 16 is the largest squared difference)."""
    j = 1
    while 2 * j <= rows // 2 and 2 * j * ppc * ex.DIFF_MAX ** 2 < ex.F32_INTS:
        j *= 2
    return j


def _loss_setup(dev, B, Lm, PPC, p, bands, seed=0):  # noqa: N803
    rows, Lg = B * Lm, TOK_OFF + Lm + TAIL  # noqa: N806
    n_sel = _n_selected(rows, PPC)
    rec, tgt, k = ex.loss_operands(rows, PPC, dev, seed=seed + p, window=WINDOW if bands else None)
    mask, sel = ex.token_mask(B, Lg, TOK_OFF, Lm, n_sel, dev, seed=seed)
    weight = LOSS_WEIGHT[PPC]
    coef = weight / (n_sel * PPC)
    assert ex.is_power_of_two(coef) and nm.f32(weight) == weight
    # the count the kernel divides by: tokens (plain) or elements (bands)
    cnt = torch.tensor([n_sel * PPC if bands else n_sel], dtype=torch.int32, device=dev)
    return dict(B=B, Lm=Lm, Lg=Lg, PPC=PPC, p=p, rows=rows, rec=rec, tgt=tgt, k=k, mask=mask, sel=sel, weight=weight, coef=coef,
                cnt=cnt, n_sel=n_sel, bands=bands)


def _launch_loss(c, entry, acc, drec, cs=None):
    from maestro_amd import hip
    head = (c["rec"], c["tgt"], c["mask"], c["cnt"], c["weight"], acc, drec)
    tail = (c["B"], c["Lm"], c["Lg"], TOK_OFF, c["PPC"], c["p"]) + (WINDOW if c["bands"] else ())
    if entry == "cs":
        head += (cs,)
    name = "masked_loss" + ("_bands" if c["bands"] else "") + {"plain": "", "det": "_det", "cs": "_cs"}[entry]
    getattr(hip, name)(*head, *tail)


@pytest.mark.parametrize("bands", [False, True], ids=["plain", "bands"])
@pytest.mark.parametrize("p", [1, 2])
@pytest.mark.parametrize("B,Lm,PPC,rpw", LOSS_CASES, ids=[f"{b * l}x{ppc}_rpw{r}" for b, l, ppc, r in LOSS_CASES])
def test_masked_loss_exact(dev, B, Lm, PPC, rpw, p, bands):  # noqa: N803
    from maestro_amd import hip
    c = _loss_setup(dev, B, Lm, PPC, p, bands)
    rows, coef = c["rows"], c["coef"]
    assert loss_rows_per_wave(rows) == rpw
    blk_rows = 4 * rpw
    n_blk = -(-rows // blk_rows)
    assert hip.masked_loss_partial_size(B, Lm) == n_blk and hip.masked_loss_cs_rows(B, Lm) == n_blk
    if rpw > 1:
        assert rows % blk_rows != 0 and rows % rpw != 0      # a ragged last block whose last wave stops inside its row loop

    terms, unit = ex.loss_terms(c["k"], c["sel"], p)
    want_d, d_unit = ex.drec_values(c["k"], c["sel"], p, coef)
    acc0 = 16.0 * unit * coef                                            # the loss word is added to, not stored
    assert ex.is_order_free(torch.cat([terms.reshape(-1) * coef, terms.new_tensor([acc0])]), unit * coef)
    assert ex.is_order_free(want_d, d_unit, dim=0)
    assert int(c["sel"].sum()) == c["n_sel"] and bool((c["k"][c["sel"]] == 0).any())
    want_loss = terms.sum() * coef
    want_part = ex.block_sums(terms.sum(1), blk_rows) * coef             # slot i: rows [4 rpw i, 4 rpw (i + 1))
    want_cs = ex.block_sums(want_d, blk_rows)
    assert want_part.shape == (n_blk,) and want_cs.shape == (n_blk, PPC)

    def nan(shape, dtype=F32):
        return torch.full(shape, float("nan"), dtype=dtype, device=dev)

    def check_drec(drec, what):
        _assert_exact(drec, want_d, f"drec {what}")
        assert torch.equal(_bits(drec), _bits(want_d.to(BF16))), f"drec {what}: a zero carries a sign"
        assert float(drec[~c["sel"]].float().abs().max()) == 0.0, f"drec {what}: a visible row is not zero"

    # the atomic entry, with and without drec
    for with_drec in (True, False):
        acc = torch.full((1,), acc0, device=dev)
        drec = nan((rows, PPC), BF16) if with_drec else None
        _launch_loss(c, "plain", acc, drec)
        _assert_exact(acc, want_loss.reshape(1) + acc0, f"loss word (drec {'written' if with_drec else 'None'})")
        if with_drec:
            check_drec(drec, "plain")
    # the deterministic entry: one slot per workgroup, then the ordered sum
    part, drec, total = nan((n_blk,)), nan((rows, PPC), BF16), nan((1,))
    _launch_loss(c, "det", part, drec)
    hip.OrderedReduce([(part, total, n_blk, 1, 1)], dev).launch()
    _assert_exact(part, want_part, "DET partial slots")
    _assert_exact(total, want_loss.reshape(1), "ordered sum of the DET partials")
    check_drec(drec, "det")
    # the column-sum entry
    acc, drec, cs = torch.full((1,), acc0, device=dev), nan((rows, PPC), BF16), nan((n_blk, PPC))
    _launch_loss(c, "cs", acc, drec, cs)
    _assert_exact(acc, want_loss.reshape(1) + acc0, "loss word of the CS entry")
    check_drec(drec, "cs")
    _assert_exact(cs, want_cs, "cs_partial rows")


@pytest.mark.parametrize("p", [1, 2])
def test_masked_loss_random(dev, observed, p):
    """randn operands at 8195 x 260 (two rows per wave, 1025 workgroups), the atomic, the CS and the DET entry.

    Loss: the terms are non-negative, so each addition of a chain loses at most u of the total.  A lane adds ``T_lane = 4 rpw
    ceil(PPC / 256)`` terms, the wave and the workgroup add 6 + 2 levels, and the loss word receives ``n_blocks`` atomic additions one
    after the other: ``(T_lane + 8 + n_blocks) u L``.  ``4 u L`` more for the roundings inside a term (the difference, its square,
    coef and the product with it).  drec = bf16(2 diff coef) resp. +-coef: half a bf16 ulp and six fp32 roundings."""
    from maestro_amd import hip
    B, Lm, PPC = 5, 1639, 260  # noqa: N806
    rows, Lg = B * Lm, TOK_OFF + Lm + TAIL  # noqa: N806
    rpw = loss_rows_per_wave(rows)
    n_blk = -(-rows // (4 * rpw))
    g = torch.Generator(device=dev).manual_seed(40 + p)
    rec, tgt = torch.randn(rows, PPC, device=dev, generator=g), torch.randn(rows, PPC, device=dev, generator=g)
    mask = (torch.rand(B, Lg, device=dev, generator=g) < 0.6).to(torch.uint8)
    sel = mask[:, TOK_OFF: TOK_OFF + Lm].reshape(-1).bool()
    n_tok = int(sel.sum())
    cnt = torch.tensor([n_tok], dtype=torch.int32, device=dev)
    weight = 0.625
    coef = weight / (n_tok * PPC)
    diff = torch.where(sel[:, None], rec.double() - tgt.double(), torch.zeros((), dtype=torch.float64, device=dev))
    L64 = float((diff.abs() if p == 1 else diff * diff).sum() * coef)  # noqa: N806
    want_d = (2.0 * diff if p == 2 else diff.sign()) * coef
    t_lane = 4 * rpw * -(-PPC // 256)
    bound = (t_lane + 8 + n_blk) * U * L64 + 4 * U * L64
    bound_d = nm.HALF_ULP_BF16 * want_d.abs() + 6 * U * want_d.abs()
    args = (B, Lm, Lg, TOK_OFF, PPC, p)
    for entry in ("plain", "cs", "det"):
        acc = torch.zeros(n_blk if entry == "det" else 1, device=dev)
        drec = torch.full((rows, PPC), float("nan"), dtype=BF16, device=dev)
        if entry == "plain":
            hip.masked_loss(rec, tgt, mask, cnt, weight, acc, drec, *args)
        elif entry == "cs":
            hip.masked_loss_cs(rec, tgt, mask, cnt, weight, acc, drec, torch.empty(n_blk, PPC, device=dev), *args)
        else:
            hip.masked_loss_det(rec, tgt, mask, cnt, weight, acc, drec, *args)
            total = torch.zeros(1, device=dev)
            hip.OrderedReduce([(acc, total, n_blk, 1, 1)], dev).launch()
            acc = total
        r_loss = abs(float(acc.double()) - L64) / bound
        r_d = nm.worst_ratio((drec.double() - want_d).abs(), bound_d)
        print(f"masked loss random p={p} {entry}: loss error / bound = {r_loss:.3e}, drec worst error / bound = {r_d:.3e}")
        observed("step_end_exact_gpu::masked_loss_random", f"p{p}/{entry}/loss", r_loss)
        observed("step_end_exact_gpu::masked_loss_random", f"p{p}/{entry}/drec", r_d)
        assert r_loss <= 1.0, (entry, r_loss)
        assert r_d <= 1.0, (entry, r_d)


# ------------------------------------------------------------------------------------------------ column sums
def colsum_rows_per_block(M: int, N: int) -> int:  # noqa: N803
    """The selection rule of ``mh_colsum`` restated: up to 1024 rows per block, fewer while that leaves under 128 blocks."""
    col_blocks, rpb = -(-N // 256), 1024
    while rpb > 128 and col_blocks * -(-M // rpb) < 128:
        rpb >>= 1
    return rpb


COLSUM_CASES = [(1, 4, 128), (129, 264, 128), (4099, 2044, 256), (8195, 2044, 512), (16387, 2044, 1024)]


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("M,N,rpb", COLSUM_CASES, ids=[f"{m}x{n}_rpb{r}" for m, n, r in COLSUM_CASES])
def test_colsum_exact(dev, M, N, rpb, dtype):  # noqa: N803
    from maestro_amd import hip
    assert colsum_rows_per_block(M, N) == rpb
    x, ints = ex.int_rows(M, N, dev, seed=1, ld=N + 8, dtype=dtype)
    out, out_ints = ex.int_vector(N, dev, seed=2)
    assert ex.is_order_free(torch.cat([ints, out_ints[None]]), 1.0, dim=0)
    assert int(ints.abs().max()) == ex.INT_MAX or M * N < 1000
    hip.colsum(x, out, M, N, N + 8)
    _assert_exact(out, ints.sum(0) + out_ints, f"colsum {M}x{N} {dtype}")


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_colsum_partial_exact(dev, dtype):
    from maestro_amd import hip
    M, N = 4099, 2044  # noqa: N806
    x, ints = ex.int_rows(M, N, dev, seed=3, ld=N + 8, dtype=dtype)
    assert ex.is_order_free(ints, 1.0, dim=0)
    rows = hip.colsum_partial_rows(M)
    assert rows == -(-M // 256) == 17
    part = torch.full((rows, N), float("nan"), device=dev)
    dst = torch.full((N,), float("nan"), device=dev)
    hip.colsum_partial(x, part, M, N, N + 8)
    hip.OrderedReduce([(part, dst, rows, N, N)], dev).launch()
    _assert_exact(part, ex.block_sums(ints, 256), "colsum partial rows")
    _assert_exact(dst, ints.sum(0), "ordered reduce of the partial rows")


def test_colsum_batched_exact(dev):
    from maestro_amd import hip
    assert hip.COLSUM_ROWS == 16
    shapes = [(17, 4, 12), (250, 260, 264), (33, 768, 776), (1, 260, 268)]        # rows (no multiple of 16), cols, ld > cols
    jobs, want = [], []
    for i, (rows, cols, ld) in enumerate(shapes):
        assert rows % hip.COLSUM_ROWS != 0 and ld > cols
        x, ints = ex.int_rows(rows, cols, dev, seed=10 + i, ld=ld)
        dst, dst_ints = ex.int_vector(cols, dev, seed=20 + i)
        assert ex.is_order_free(torch.cat([ints, dst_ints[None]]), 1.0, dim=0)
        jobs.append((x.as_strided((rows, ld), (ld, 1)), dst, rows, cols, ld))      # the whole [rows, ld] buffer, NaN pad columns included
        want.append(ints.sum(0) + dst_ints)
    hip.ColsumBatch(jobs, dev).launch()
    for i, (job, w) in enumerate(zip(jobs, want)):
        _assert_exact(job[1], w, f"batched colsum job {i} {shapes[i]}")


# ------------------------------------------------------------------------------------------------ mask-token gradient, counts
TG_B, TG_L, TG_LO, TG_HI = 3, 350, 5, 347          # 3 x 342 = 1026 rows: three 512-row strips, the last holds two rows
UM_ROWS = 512


def _token_case(dev, per_sample):
    g = torch.Generator(device=dev).manual_seed(77 + per_sample)
    mask = (torch.rand(TG_B, TG_L, device=dev, generator=g) < 0.6).to(torch.uint8)
    slots = torch.randint(0, 2, (TG_B, TG_L) if per_sample else (TG_L,), device=dev, generator=g, dtype=torch.int32)
    mask[:, :2] = 1             # masked tokens of either slot in front of TG_LO: outside the range of the shared-slot entries
    slots[..., 0], slots[..., 1] = 0, 1
    return mask, slots


@pytest.mark.parametrize("per_sample", [False, True], ids=["shared_slots", "per_sample"])
@pytest.mark.parametrize("Dd", [4, 32, 384, 512, 1024])
def test_unmask_token_grad_exact(dev, Dd, per_sample):  # noqa: N803
    from maestro_amd import hip
    B, L = TG_B, TG_L  # noqa: N806
    t_lo, t_hi = (0, L) if per_sample else (TG_LO, TG_HI)
    span = t_hi - t_lo
    n_strips = -(-B * span // UM_ROWS)
    assert hip.unmask_token_grad_partial_rows(B * span) == n_strips == 3
    assert (B * span) % UM_ROWS == (26 if per_sample else 2)
    dx, ints = ex.int_rows(B * L, Dd, dev, seed=Dd)
    mask, slots = _token_case(dev, per_sample)
    sl = slots if per_sample else slots[None].expand(B, L)
    assert ex.is_order_free(ints, 1.0, dim=0)
    in_range = torch.zeros(B, L, dtype=torch.bool, device=dev)
    in_range[:, t_lo:t_hi] = True
    for slot in (0, 1):
        pick = mask.bool() & (sl == slot) & in_range
        other = mask.bool() & (sl == 1 - slot) & in_range
        assert bool(pick.any()) and bool(other.any())                 # rows masked in the other slot only are there
        if not per_sample:
            assert bool((mask.bool() & (sl == slot) & ~in_range).any())    # ... and rows of this slot outside [t_lo, t_hi)
        contrib = ints * pick.reshape(-1, 1)                          # [B * L, Dd], zero where the row does not count
        want = contrib.sum(0)
        dst, dst_ints = ex.int_vector(Dd, dev, seed=slot)
        assert ex.is_order_free(torch.cat([contrib, dst_ints[None]]), 1.0, dim=0)
        part = torch.full((n_strips, Dd), float("nan"), device=dev)
        if per_sample:
            hip.unmask_token_grad_per_sample(dx, mask, slots, dst, B, L, Dd, slot)
            hip.unmask_token_grad_per_sample_det(dx, mask, slots, part, B, L, Dd, slot)
        else:
            hip.unmask_token_grad(dx, mask, slots, dst, B, L, Dd, slot, t_lo, t_hi)
            hip.unmask_token_grad_det(dx, mask, slots, part, B, L, Dd, slot, t_lo, t_hi)
        _assert_exact(dst, want + dst_ints, f"token gradient Dd={Dd} slot {slot}")
        # strip i: rows [512 i, 512 (i + 1)) of the (sample, token in [t_lo, t_hi)) enumeration
        ranged = contrib.reshape(B, L, Dd)[:, t_lo:t_hi].reshape(B * span, Dd)
        _assert_exact(part, ex.block_sums(ranged, UM_ROWS), f"token gradient strips Dd={Dd} slot {slot}")


def test_count_masked_exact(dev):
    from maestro_amd import hip
    masks = [(_token_case(dev, False)[0], TG_B, TG_L, TG_LO, TG_HI), (_token_case(dev, True)[0], TG_B, TG_L, 0, TG_L)]
    B, Lm = 5, 13109  # noqa: N806
    big, sel = ex.token_mask(B, TOK_OFF + Lm + TAIL, TOK_OFF, Lm, 32768, dev)
    masks.append((big, B, TOK_OFF + Lm + TAIL, TOK_OFF, TOK_OFF + Lm))
    for mask, B, L, t_lo, t_hi in masks:  # noqa: N806
        want = int(mask[:, t_lo:t_hi].long().sum())
        if (t_lo, t_hi) != (0, L):
            assert want != int(mask.long().sum())                     # ones outside the window would be seen
        out = torch.full((1,), -7, dtype=torch.int32, device=dev)
        hip.count_masked(mask, B, L, t_lo, t_hi, out)
        assert out.item() == want
        out.fill_(-7)
        hip.count_masked_elems(mask, B, L, t_lo, t_hi, out, 768, False)
        assert out.item() == 768 * want
        out.fill_(1000)
        hip.count_masked_elems(mask, B, L, t_lo, t_hi, out, 768, True)
        assert out.item() == 1000 + 768 * want
    assert int(sel.sum()) == 32768 and math.log2(32768) == 15
