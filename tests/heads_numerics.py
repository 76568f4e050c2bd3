"""Operands, expectations, fp64 references, a-priori error bounds and fp32 emulations for the probe / finetune head kernels
(csrc/heads.hip): token-grid resize, attentive and mean reduction, the classification linear, cross entropy and BCE.

Used by tests/test_heads_selfcheck.py (CPU: the honest emulation lies inside every bound and equals every exact expectation, and
every named wrong form is rejected by a case of the lists below) and tests/test_heads_numerics_gpu.py (the HIP kernels on the
very same cases).  Per family ``X`` there is a case list ``X_CASES``, ``x_case(*case)`` (operands and what to expect of them),
``x_emulated(data, form)`` (torch fp32 written as the kernel is; ``form`` names a wrong form from ``X_WRONG``) and
``x_ratios(data, got)`` (per quantity ``max(error / bound)``: 0 or inf where the expectation is exact).  The GPU file hands
``x_ratios`` what the kernels wrote, the self-check what the emulation gives: the two cannot drift.

Exact operands make every result independent of summation order and of every rounding (tests/exact_sums.py); each case asserts
``is_order_free`` on its own terms.  Everything else is held elementwise to a bound derived from the kernel's own sequence of
roundings; u = 2^-24, HB = 2^-8 (bf16 store), FL = 2^-126 (results the hardware flushes), 2^-23 per accumulated fp32 term in
any order (``numerics.gemm_bound``), ``__expf`` / ``__logf`` = v_exp_f32 / v_log_f32 at 2^-22 plus their argument scaling.
Line numbers: csrc/heads.hip.  Nothing here is fitted to what the kernels give; the measured slack is in
profiles/heads_numerics.md.
"""

from __future__ import annotations

import functools
import math

import torch
import torch.nn.functional as F  # noqa: N812

from tests import exact_sums as ex
from tests import numerics as nm
from tests.numerics import FLUSH_F32, HALF_ULP_BF16, U_F32, bf16_round, worst_ratio

U, HB, FL = U_F32, HALF_ULP_BF16, FLUSH_F32
ACC = 2.0 ** -23            # per accumulated fp32 term, any order (gemm_bound's constant)
EXP_ULP = 2.0 ** -22        # v_exp_f32 / v_log_f32 (numerics.py's figure)
INF = math.inf


def exact_ratio(got: torch.Tensor, want64: torch.Tensor) -> float:
    """0 where the fp64 images agree bit for bit, inf otherwise (so that an exact quantity reads like a bounded one)."""
    return 0.0 if got.shape == want64.shape and torch.equal(got.double().cpu(), want64.double().cpu()) else INF


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Bitwise equality (NaN fill included) of two tensors of the same 2- or 4-byte dtype."""
    it = torch.int32 if a.element_size() == 4 else torch.int16
    return a.shape == b.shape and torch.equal(a.contiguous().view(it), b.contiguous().view(it))


def exp_rel(x64: torch.Tensor) -> torch.Tensor:
    """Relative error of ``__expf(fl(a - b))`` at the exact argument x = a - b: the subtraction (u |x|), the product with
    log2(e) and that constant's own rounding (2 u |x|: a relative error of the exponent is an absolute one of the result's
    logarithm), v_exp_f32 (2^-22)."""
    return 3 * U * x64.abs() + EXP_ULP


def expf32(x: torch.Tensor) -> torch.Tensor:
    """``__expf`` as the device forms it: v_exp_f32 of the fp32 product with fl(log2 e)."""
    return torch.exp2(x * torch.tensor(nm.LOG2E, dtype=torch.float32))


def logf32(x: torch.Tensor) -> torch.Tensor:
    """``__logf``: v_log_f32 times fl(ln 2)."""
    return torch.log2(x) * torch.tensor(nm.LN2, dtype=torch.float32)


def _gen(*key) -> torch.Generator:
    s = 0
    for k in key:
        s = (s * 1000003 + (sum(map(ord, k)) if isinstance(k, str) else int(k))) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def _ints(g, shape, r=ex.INT_MAX):
    return torch.randint(-r, r + 1, shape, generator=g).float()


# ================================================================================================ token-grid resize
RESIZE_DYADIC = ((4, 8), (3, 12), (8, 4), (6, 3), (1, 4), (4, 1), (5, 5))
RESIZE_RATIOS = ((3, 10), (5, 32), (7, 3))
RESIZE_LAYOUTS = ((4, 3), (64, 1), (192, 3))                                   # (E, D)
RESIZE_CASES = [("exact", h, H, E, D) for h, H in RESIZE_DYADIC for E, D in RESIZE_LAYOUTS]
RESIZE_CASES += [("randn", h, H, E, D) for h, H in RESIZE_RATIOS for E, D in RESIZE_LAYOUTS]
RESIZE_WRONG = ("align_corners", "no_clamp_low", "no_edge_clamp", "swap_xy", "date_stride_out", "bwd_i0_only",
                "bwd_ignores_accumulate")
RESIZE_B, RESIZE_IN_OFF, RESIZE_OUT_OFF, RESIZE_POST = 2, 7, 2, 5           # the modality sits between other rows
RESIZE_BOUND_TERMS = ("weights", "blend")


def lerp_emulated(n_in: int, n_out: int, form: str = "honest"):
    """``lerp_of`` (:13-21) for every destination index in fp32: ``(i0, i1, l0, l1)``."""
    f32 = torch.float32
    dst = torch.arange(n_out, dtype=f32)
    if form == "align_corners":
        f = dst * (torch.tensor(n_in - 1.0, dtype=f32) / torch.tensor(max(n_out - 1.0, 1.0), dtype=f32))
    else:
        f = (torch.tensor(float(n_in), dtype=f32) / torch.tensor(float(n_out), dtype=f32)) * (dst + 0.5) - 0.5
        if form != "no_clamp_low":
            f = f.clamp_min(0.0)
    i0 = f.to(torch.int64).clamp_max(n_in - 1)                  # a C cast truncates towards zero
    i1 = i0 + 1 if form == "no_edge_clamp" else i0 + (i0 < n_in - 1).long()
    l1 = f - i0.float()
    return i0, i1, 1.0 - l1, l1


def lerp64(n_in: int, n_out: int, alt: bool = False):
    """The true index map in fp64 and ``df``, the bound on the error of the fp32 coordinate f = fl(fl(n_in / n_out) (dst + 0.5)
    - 0.5) (:14-15): the quotient's rounding carried through the product (u r (dst + 0.5)), the product's own (the same again)
    and the subtraction's (u |f|); 0 where the coordinate is clamped, and 0 for a dyadic ratio (f and both weights are multiples
    of 1/8: nothing rounds).  Where the true f lies within 2 df of a source index (7 -> 3: f(1) = 3 exactly, fl(7 / 3) 1.5 is a tie)
    the fp32 floor may fall on either side: the blend is continuous there, but its local differences are those of the
    neighbouring cell.  ``alt`` returns that neighbouring cell for such destinations (the same map elsewhere)."""
    dst = torch.arange(n_out, dtype=torch.float64)
    r = n_in / n_out
    ft = r * (dst + 0.5) - 0.5
    f = ft.clamp_min(0.0)
    exact = bool((ft * 8 == (ft * 8).round()).all())
    df = torch.where(ft > 0, U * (2 * r * (dst + 0.5) + f), torch.zeros_like(f))
    df = torch.zeros_like(df) if exact else df
    assert exact or bool(((ft.abs() > 2 * df) | (ft < 0)).all()), (n_in, n_out)       # the clamp at 0 is never in doubt
    frac = f - f.floor()
    i0 = f.floor().long().clamp_max(n_in - 1)
    if alt:
        below, above = (frac < 2 * df) & (i0 >= 1), (1 - frac < 2 * df) & (i0 < n_in - 1)
        i0 = torch.where(below, i0 - 1, torch.where(above, i0 + 1, i0))
        f = torch.where(below | above, f.round(), f)
    i1 = i0 + (i0 < n_in - 1).long()
    l1 = f - i0
    l1 = torch.where(i0 == i1, torch.zeros_like(l1), l1)          # clamped at the far edge: both taps are the same token
    return i0, i1, 1.0 - l1, l1, df


def _lerp_matrix(n_in: int, n_out: int, alt: bool = False) -> torch.Tensor:
    """[n_in, n_out] fp64: the weight of source y in destination Y."""
    i0, i1, l0, l1, _ = lerp64(n_in, n_out, alt)
    w = torch.zeros(n_in, n_out, dtype=torch.float64)
    w.index_put_((i0, torch.arange(n_out)), l0, accumulate=True)
    w.index_put_((i1, torch.arange(n_out)), l1, accumulate=True)
    return w


def _mod_rows(off: int, D: int, n: int) -> slice:  # noqa: N803
    return slice(off, off + D * n * n)


@functools.lru_cache(maxsize=None)
def resize_case(kind: str, h: int, H: int, E: int, D: int):  # noqa: N803
    """Operands as the kernels take them: ``x`` [B, in_rows, E], ``dout`` [B, out_rows, E], ``pre`` (preload of din), and the
    fp64 expectations ``out`` [B, D, H, H, E], ``din`` (accumulate = 0) -- F.interpolate and its autograd on the true ratio."""
    B = RESIZE_B  # noqa: N806
    g = _gen("resize", kind, h, H, E, D)
    in_rows, out_rows = RESIZE_IN_OFF + D * h * h + RESIZE_POST, RESIZE_OUT_OFF + D * H * H + 3
    draw = (lambda *s: _ints(g, s)) if kind == "exact" else (lambda *s: torch.randn(*s, generator=g))
    x, dout, pre = draw(B, in_rows, E), draw(B, out_rows, E), draw(B, in_rows, E)
    xm = x[:, _mod_rows(RESIZE_IN_OFF, D, h)].double().reshape(B * D, h, h, E).permute(0, 3, 1, 2).clone().requires_grad_(True)
    want = F.interpolate(xm, (H, H), mode="bilinear", align_corners=False)
    dm = dout[:, _mod_rows(RESIZE_OUT_OFF, D, H)].double().reshape(B * D, H, H, E)
    want.backward(dm.permute(0, 3, 1, 2))
    d = dict(kind=kind, h=h, H=H, E=E, D=D, B=B, x=x, dout=dout, pre=pre, in_rows=in_rows, out_rows=out_rows,
             out=want.detach().permute(0, 2, 3, 1).reshape(B, D * H * H, E), din=xm.grad.permute(0, 2, 3, 1).reshape(B, D * h * h, E))
    if kind == "exact":
        i0, i1, l0, l1, _ = lerp64(h, H)
        w = _lerp_matrix(h, H)
        assert ex.is_order_free(w, 0.125, dim=0) and bool((l0 * 8 == (l0 * 8).round()).all())       # every weight a multiple of 1/8
        # forward: the four taps of a destination, each a product of two weights and an integer
        v = x[:, _mod_rows(RESIZE_IN_OFF, D, h)].double().reshape(B, D, h, h, E)
        taps = [wy[:, None, None] * wx[None, :, None] * v[:, :, yi][:, :, :, xi] for yi, wy in ((i0, l0), (i1, l1)) for xi, wx in ((i0, l0), (i1, l1))]
        assert ex.is_order_free(torch.stack(taps), 1.0 / 64, dim=0)
        # backward: all destinations of a source, and the preload
        terms = torch.einsum("yY,xX,bdYXe->YXbdyxe", w, w, dm.reshape(B, D, H, H, E)).reshape(H * H, B, D * h * h, E)
        assert ex.is_order_free(torch.cat([terms, pre[None, :, _mod_rows(RESIZE_IN_OFF, D, h)].double()]), 1.0 / 64, dim=0)
    return d


def resize_bounds(d, drop=()):
    """``(b_out [B, D H H, E], b_din0, b_din1)`` for a non-dyadic case; ``drop``: names of RESIZE_BOUND_TERMS to leave out.

    Forward (:31-38): ``weights`` -- the coordinate's error df (``lerp64``) is the error of l1 (f - i0 is exact) and of l0 (one more
    rounding, counted in ``blend``); it multiplies the local differences d out / d l1 along x and y and their mixed difference.
    ``blend`` -- every tap passes a product, a sum, a product and a sum (4 u) and its two weights 1 - l1 (2 u): 6 u sum w |v|.
    Backward (:52-65): the weight of a destination is l0 or l1 or their sum (df + 2 u where it is not zero), the product wy wx
    and the product with dout (2 u), an fp32 sum over the n destinations that reach the source (n 2^-23), the sum with what
    din holds (u on both)."""
    assert set(drop) <= set(RESIZE_BOUND_TERMS)
    h, H, E, D, B = d["h"], d["H"], d["E"], d["D"], d["B"]  # noqa: N806
    df = lerp64(h, H)[4]
    if "weights" in drop:
        df = torch.zeros_like(df)
    blend = 0.0 if "blend" in drop else 6 * U
    v = d["x"][:, _mod_rows(RESIZE_IN_OFF, D, h)].double().reshape(B, D, h, h, E)
    t = lambda a, b: v[:, :, a][:, :, :, b]  # noqa: E731   [B, D, H(Y), H(X), E]
    dfy, dfx = df[:, None, None], df[None, :, None]

    def fwd(ly, lx):
        (y0, y1, ly0, ly1, _), (x0, x1, lx0, lx1, _) = ly, lx
        v00, v01, v10, v11 = t(y0, x0), t(y0, x1), t(y1, x0), t(y1, x1)
        ly0, ly1, lx0, lx1 = ly0[:, None, None], ly1[:, None, None], lx0[None, :, None], lx1[None, :, None]
        mag = ly0 * (lx0 * v00.abs() + lx1 * v01.abs()) + ly1 * (lx0 * v10.abs() + lx1 * v11.abs())
        ddx = (ly0 * (v01 - v00) + ly1 * (v11 - v10)).abs()
        ddy = (lx0 * (v10 - v00) + lx1 * (v11 - v01)).abs()
        return blend * mag + dfx * ddx + dfy * ddy + dfx * dfy * (v00 - v01 - v10 + v11).abs()

    cells = (lerp64(h, H), lerp64(h, H, alt=True))
    b_out = functools.reduce(torch.maximum, [fwd(ly, lx) for ly in cells for lx in cells]).reshape(B, D * H * H, E)
    w = _lerp_matrix(h, H)
    taps = (w > 0) | (_lerp_matrix(h, H, alt=True) > 0)
    dw = (df[None, :] + (0.0 if "blend" in drop else 2 * U)) * taps
    n = (taps.sum(1)[:, None] * taps.sum(1)[None, :]).double()                       # destinations that may reach source (y, x)
    a = d["dout"][:, _mod_rows(RESIZE_OUT_OFF, D, H)].double().abs().reshape(B, D, H, H, E)
    es = lambda wy, wx: torch.einsum("yY,xX,bdYXe->bdyxe", wy, wx, a)  # noqa: E731
    ww = es(w, w)
    b_acc = es(dw, w) + es(w, dw) + es(dw, dw) + (0.0 if "blend" in drop else 1.0) * (2 * U + n[None, None, :, :, None] * ACC) * ww
    b_acc = b_acc.reshape(B, D * h * h, E)
    pre = d["pre"][:, _mod_rows(RESIZE_IN_OFF, D, h)].double()
    return b_out, b_acc, b_acc + U * (pre.abs() + (pre + d["din"]).abs())


def resize_emulated(d, form: str = "honest"):
    """The two kernels in fp32 on the case's buffers: ``out`` (NaN outside the modality's rows), ``din0`` (accumulate = 0 on a NaN
    fill), ``din1`` (accumulate = 1 on ``pre``)."""
    assert form == "honest" or form in RESIZE_WRONG, form
    h, H, E, D, B, x, dout = d["h"], d["H"], d["E"], d["D"], d["B"], d["x"], d["dout"]  # noqa: N806
    i0, i1, l0, l1 = lerp_emulated(h, H, form)
    dbase = torch.arange(D) * (H * H if form == "date_stride_out" else h * h)
    row = lambda yi, xi: (RESIZE_IN_OFF + dbase[:, None, None] + yi[None, :, None] * h + xi[None, None, :]).clamp(0, d["in_rows"] - 1)  # noqa: E731
    tap = lambda yi, xi: x[:, row(yi, xi)]  # noqa: E731   [B, D, H, H, E]
    ly0, ly1, lx0, lx1 = l0[:, None, None], l1[:, None, None], l0[None, :, None], l1[None, :, None]
    o = ly0 * (lx0 * tap(i0, i0) + lx1 * tap(i0, i1)) + ly1 * (lx0 * tap(i1, i0) + lx1 * tap(i1, i1))
    if form == "swap_xy":
        o = o.transpose(2, 3)
    out = torch.full((B, d["out_rows"], E), float("nan"))
    out[:, _mod_rows(RESIZE_OUT_OFF, D, H)] = o.reshape(B, D * H * H, E)
    # backward: the transposed map as a gather
    w = torch.zeros(h + 1, H)
    w.index_put_((i0, torch.arange(H)), l0, accumulate=True)
    if form != "bwd_i0_only":
        w.index_put_((i1, torch.arange(H)), l1, accumulate=True)        # a tap at index h (no_edge_clamp) reaches no source
    w = w[:h]
    obase = torch.arange(D) * (h * h if form == "date_stride_out" else H * H)
    yy = torch.arange(H)
    orow = (RESIZE_OUT_OFF + obase[:, None, None] + yy[None, :, None] * H + yy[None, None, :]).clamp(0, d["out_rows"] - 1)
    acc = torch.einsum("yY,xX,bdYXe->bdyxe", w, w, dout[:, orow])
    if form == "swap_xy":
        acc = acc.transpose(2, 3)
    acc = acc.reshape(B, D * h * h, E)
    din0 = torch.full((B, d["in_rows"], E), float("nan"))
    din0[:, _mod_rows(RESIZE_IN_OFF, D, h)] = acc
    din1 = d["pre"].clone()
    din1[:, _mod_rows(RESIZE_IN_OFF, D, h)] = acc if form == "bwd_ignores_accumulate" else acc + d["pre"][:, _mod_rows(RESIZE_IN_OFF, D, h)]
    return dict(out=out, din0=din0, din1=din1)


def _outside_unchanged(buf, fill, rows: slice) -> bool:
    keep = torch.ones(buf.shape[1], dtype=torch.bool)
    keep[rows] = False
    return same_bits(buf[:, keep], fill[:, keep])


def resize_ratios(d, got, drop=()):
    """got: ``out`` on a NaN fill, ``din0`` on a NaN fill, ``din1`` on ``pre``.  Rows outside the modality must keep their bits."""
    h, H, D = d["h"], d["H"], d["D"]  # noqa: N806
    mi, mo = _mod_rows(RESIZE_IN_OFF, D, h), _mod_rows(RESIZE_OUT_OFF, D, H)
    pre64 = d["pre"][:, mi].double()
    want = dict(out=d["out"], din0=d["din"], din1=d["din"] + pre64)
    nan_in, nan_out = torch.full_like(d["pre"], float("nan")), torch.full_like(d["dout"], float("nan"))
    r = dict(out_outside=0.0 if _outside_unchanged(got["out"], nan_out, mo) else INF,
             din0_outside=0.0 if _outside_unchanged(got["din0"], nan_in, mi) else INF,
             din1_outside=0.0 if _outside_unchanged(got["din1"], d["pre"], mi) else INF)
    bounds = dict(zip(("out", "din0", "din1"), resize_bounds(d, drop))) if d["kind"] != "exact" else None
    for k, rows in (("out", mo), ("din0", mi), ("din1", mi)):
        g = got[k][:, rows]
        r[k] = exact_ratio(g, want[k]) if bounds is None else _ratio(g, want[k], bounds[k])
    return r


def _ratio(got, want64, bound) -> float:
    got = got.double().cpu()
    if got.shape != want64.shape or not bool(torch.isfinite(got).all()):
        return INF
    return worst_ratio((got - want64).abs(), bound)


# ================================================================================================ attentive reduction
AR_DIMS = (192, 384, 768, 1024)
# (n_batch, T, Lr): one sequence; two keys; odd T; exactly one workgroup (16 sequences); a second workgroup with one live wave;
# Lr > 1 with T > 1 (the row map); a long key axis
AR_SHAPES = ((1, 1, 1), (1, 2, 1), (5, 3, 1), (2, 4, 8), (17, 5, 1), (3, 17, 16), (2, 333, 1))
AR_KINDS = ("randn1.5", "randn4", "offset", "rising", "falling", "spike")
AR_EXACT_KINDS = ("one_key", "equal_keys")
AR_CASES = [(kind, dim, 3, 17, 16) for dim in (192, 384) for kind in AR_KINDS]
AR_CASES += [(kind, dim) + s for dim in AR_DIMS for s in AR_SHAPES for kind in ("randn1.5", "rising")
             if not (dim in (192, 384) and s == (3, 17, 16))]
AR_CASES += [("one_key", dim, 5, 1, 4) for dim in AR_DIMS] + [("equal_keys", dim, 3, 4, 2) for dim in AR_DIMS]
AR_WRONG_FWD = ("scale_dim", "no_scale", "heads_of_16", "no_rescale", "lse_linear", "row_order")
AR_WRONG_BWD = ("dq_unscaled", "dk_unscaled_q", "delta_full_dim")
AR_WRONG = AR_WRONG_FWD + AR_WRONG_BWD
AR_BOUND_TERMS = ("dot", "store")        # the terms the self-check can show to be needed; the others are worst cases
AR_SEQ_PER_BLOCK = 16       # 4 waves x AR_SEQ_PER_WAVE (:72)


def ar_rows(nb: int, T: int, Lr: int, row_order: bool = False) -> torch.Tensor:  # noqa: N803
    """[n_seq, T]: the kv row of token t of sequence s = (b, l) (:110); ``row_order``: the WRONG map (b Lr + l) T + t."""
    b, l, t = torch.arange(nb)[:, None, None], torch.arange(Lr)[None, :, None], torch.arange(T)[None, None, :]  # noqa: E741
    return ((b * Lr + l) * T + t if row_order else (b * T + t) * Lr + l).reshape(nb * Lr, T)


def _scale32(n: int) -> torch.Tensor:
    """1.f / sqrtf((float)n) (:382): both correctly rounded."""
    return 1.0 / torch.sqrt(torch.tensor(float(n), dtype=torch.float32))


@functools.lru_cache(maxsize=None)
def ar_case(kind: str, dim: int, nb: int, T: int, Lr: int):  # noqa: N803
    """``kv`` bf16 [nb T Lr, 2 dim], ``query`` f32 [dim], ``dout`` f32 [n_seq, dim] and the fp64 reference ``ref``.

    The shifted kinds move the logit of key t of head h by c(s, h, t) along the head's own query direction: ``offset`` +40 on all,
    ``rising`` / ``falling`` +- step t with step = min(3, 120 / T) (every key beats, or loses to, all before it: the online softmax
    rescales at every step, resp. never after the first), ``spike`` +40 on one key per (s, h) (a saturated softmax: dp - delta
    cancels).  ``one_key`` (T = 1) and ``equal_keys`` are the exact kinds: see ``ar_ratios``."""
    S, dh = nb * Lr, dim // 8  # noqa: N806
    g = _gen("ar", kind, dim, nb, T, Lr)
    query = torch.randn(dim, generator=g)
    rows = ar_rows(nb, T, Lr)
    if kind in AR_EXACT_KINDS:
        v = _ints(g, (S, T, dim))
        dout = _ints(g, (S, dim))
        k = torch.zeros(S, T, 8, dh)
        j = torch.randint(0, dh, (S, 1, 8, 1), generator=g)
        e = torch.randint(-2, 4, (S, 1, 8, 1), generator=g).float()
        k.scatter_(3, j.expand(S, T, 8, 1), (2.0 ** e).expand(S, T, 8, 1) * (1 - 2 * (j % 2)).float())   # one power of two per head
        if kind == "one_key":
            assert T == 1
        else:
            assert ex.is_power_of_two(T) and ex.is_order_free(v, 1.0, dim=1)
        # delta and dp (:153, :164) are sums of dh integer products, bitwise equal whatever their order
        assert ex.is_order_free((dout[:, None].abs() * v.abs()).reshape(S * T * 8, dh), 1.0, dim=1)
        k = k.reshape(S, T, dim)
    else:
        a = {"randn1.5": 1.5, "randn4": 4.0, "offset": 1.0, "spike": 1.0}.get(kind, 0.1)
        k = (a * torch.randn(S, T, dim, generator=g)).reshape(S, T, 8, dh)
        v = torch.randn(S, T, dim, generator=g)
        dout = torch.randn(S, dim, generator=g)
        shift = torch.zeros(S, T, 8)
        if kind == "offset":
            shift += 40.0
        elif kind in ("rising", "falling"):
            shift += (1.0 if kind == "rising" else -1.0) * min(3.0, 120.0 / T) * torch.arange(T).float()[None, :, None]
        elif kind == "spike":
            at = (torch.arange(S)[:, None] * 7 + torch.arange(8)[None, :] * 3) % T
            shift.scatter_(1, at[:, None, :], 40.0)
        qh = query.reshape(8, dh)
        k = (k + shift[..., None] * (qh / (qh * qh).sum(-1, keepdim=True))[None, None] * dh ** 0.5).reshape(S, T, dim)
    kv = torch.zeros(nb * T * Lr, 2 * dim)
    kv[rows] = torch.cat([k, v], -1)
    d = dict(kind=kind, dim=dim, nb=nb, T=T, Lr=Lr, kv=kv.bfloat16(), query=query, dout=dout)
    d["ref"] = ar_ref64(d)
    return d


def ar_ref64(d):
    """fp64 forward and backward on the bf16 kv and the true scale dh^-1/2."""
    dim, nb, T, Lr = d["dim"], d["nb"], d["T"], d["Lr"]  # noqa: N806
    S, dh = nb * Lr, dim // 8  # noqa: N806
    rows = ar_rows(nb, T, Lr)
    kvs = d["kv"].double()[rows]
    k, v = kvs[..., :dim].reshape(S, T, 8, dh), kvs[..., dim:].reshape(S, T, 8, dh)
    q, g = d["query"].double().reshape(8, dh), d["dout"].double().reshape(S, 8, dh)
    scale = dh ** -0.5
    a = scale * torch.einsum("hd,sthd->sht", q, k)
    aabs = scale * torch.einsum("hd,sthd->sht", q.abs(), k.abs())
    lse = torch.logsumexp(a, -1)
    w = torch.exp(a - lse[..., None])
    out = torch.einsum("sht,sthd->shd", w, v)
    delta = (g * out).sum(-1)
    dp = torch.einsum("shd,sthd->sht", g, v)
    gg = dp - delta[..., None]
    ds = w * gg
    dk = scale * ds.permute(0, 2, 1)[..., None] * q
    dv = w.permute(0, 2, 1)[..., None] * g[:, None]
    dq_seq = scale * torch.einsum("sht,sthd->shd", ds, k).reshape(S, dim)
    return dict(a=a, aabs=aabs, lse=lse, w=w, out=out.reshape(S, dim), delta=delta, dp=dp, G=gg, ds=ds, k=k, v=v, q=q, g=g,
                dk=dk.reshape(S, T, dim), dv=dv.reshape(S, T, dim), dq_seq=dq_seq, dq=ex.block_sums(dq_seq, AR_SEQ_PER_BLOCK), rows=rows)


def ar_bounds(d, lse_err=None, out_err=None, drop=()):
    """Elementwise bounds: ``out`` [S, dim], ``lse`` [S, 8], ``dk``, ``dv`` [S, T, dim], ``dq`` [blocks, dim].  ``lse_err`` [S, 8] /
    ``out_err`` [S, dim]: errors of what the backward is handed (default: the fp32 roundings of the fp64 values).

    ``dot`` (:101, :116-117) -- q' = fl(q fl(scale)) (2 u), every product q' k (u; 24 x 8 bits do not fit), then a sum whose order the
      kernel fixes: VPL = dim / 64 terms per lane one after the other, three xor-shuffles over the head's 8 lanes, so a term
      passes at most VPL + 3 additions ((VPL + 3) 2^-23): ddot on the logit, relative to |q| |k| scale.
    exp (:119) -- key t enters with p = expf(dot - m) and is then multiplied by c = expf(m_old - m_new) at every later step;
      the arguments are all <= 0 and add up to dot_t - m_final, so the argument roundings are 3 u (amax - a_t) in total
      (``exp_rel``) and v_exp_f32 counts once per step, T - t times.
    chain (:120-122) -- sum c + p and acc c + p v round twice per step, so the term of key t collects 2 u at each of the T - t
      steps from its own on; then 1 / sum and the product with it (:125-127, 2 u |out|).
    Together eta_t, the relative error of the weight of key t; the common m cancels in out, and in lse is the largest computed
    dot itself.  lse = m + logf(sum) (:128): the relative error of sum, v_log_f32 and the product with ln 2 (2^-22 log sum + u;
    sum lies in [1, T]), the final sum (u |lse|).
    Backward: delta (:151-155) a sum of dh products of dout with the out it is handed, in the order of the dot; dp (:164) the same with v;
    p = expf(dot - lse) (:166) with the lse it is handed; ds = p (dp - delta) (2 u).  dk = bf16(ds q') and dv = bf16(p g)
    (:169-170): ``store`` -- HB of the value itself, elementwise.  dq (:171-179): per lane an fp32 sum over the 4 T keys of its wave's
    sequences, the product with scale, the LDS sum of four waves.
    FL wherever v_exp_f32 or a bf16 convert may return 0 for a denormal result."""
    assert set(drop) <= set(AR_BOUND_TERMS)
    r, dim, T = d["ref"], d["dim"], d["T"]  # noqa: N806
    S, dh = r["out"].shape[0], dim // 8  # noqa: N806
    scale, depth = dh ** -0.5, dim // 64 + 3
    w, a, aabs = r["w"], r["a"], r["aabs"]
    ddot = (0.0 if "dot" in drop else 1.0) * (3 * U + depth * ACC) * aabs
    amax = a.max(-1, keepdim=True).values
    later = (T - torch.arange(T, dtype=torch.float64))[None, None, :]           # exps / steps that touch key t
    eta = torch.expm1(ddot + ddot.max(-1, keepdim=True).values) + 3 * U * (amax - a) + later * (EXP_ULP + 2 * U)
    v, k, q, g = r["v"].abs(), r["k"].abs(), r["q"].abs(), r["g"].abs()
    num = torch.einsum("sht,sthd->shd", w * eta, v) + T * FL * v.sum(1)
    den = (w * eta).sum(-1)
    o = r["out"].abs().reshape(S, 8, dh)
    b_out = ((num + o * den[..., None]) * (1 + den[..., None]) + 2 * U * o + FL).reshape(S, dim)
    lse = r["lse"]
    b_lse = den + EXP_ULP * (lse - amax[..., 0]).abs() + U + U * lse.abs() + ddot.max(-1).values
    # backward
    le = U * lse.abs() if lse_err is None else lse_err.double()
    oe = U * o if out_err is None else out_err.double().reshape(S, 8, dh)
    b_delta = (g * oe).sum(-1) + (depth + 1) * ACC * (g * o).sum(-1)
    e_dp = (depth + 1) * ACC * torch.einsum("shd,sthd->sht", g, v)
    gabs = r["G"].abs()
    eg = e_dp + b_delta[..., None] + U * gabs
    rho = torch.expm1(ddot + le[..., None] + 3 * U * (a - lse[..., None]).abs()) + EXP_ULP
    mag = (gabs + eg) * (1 + rho)
    E = w * (rho * gabs + (1 + rho) * eg) + U * w * mag + FL * (mag + 1)  # noqa: N806
    Et, wt = E.permute(0, 2, 1), w.permute(0, 2, 1)  # noqa: N806   [S, T, 8]
    st = 0.0 if "store" in drop else HB
    b_dk = scale * Et[..., None] * q * (1 + 3 * U) + 3 * U * r["dk"].abs().reshape(S, T, 8, dh)
    b_dk = b_dk + st * (r["dk"].abs().reshape(S, T, 8, dh) + b_dk) + FL
    b_dv = (wt * rho.permute(0, 2, 1) + FL)[..., None] * g[:, None] + U * r["dv"].abs().reshape(S, T, 8, dh)
    b_dv = b_dv + st * (r["dv"].abs().reshape(S, T, 8, dh) + b_dv) + FL
    dsk = torch.einsum("sht,sthd->shd", r["ds"].abs(), k)
    b_dq_seq = scale * (torch.einsum("sht,sthd->shd", E, k) + (4 * T + 1) * ACC * dsk) + 4 * U * scale * dsk + FL
    return dict(out=b_out, lse=b_lse, dk=b_dk.reshape(S, T, dim), dv=b_dv.reshape(S, T, dim),
                dq=ex.block_sums(b_dq_seq.reshape(S, dim), AR_SEQ_PER_BLOCK))


def _ar_scale(d, form):
    if form == "no_scale":
        return torch.tensor(1.0)
    return _scale32(d["dim"] if form == "scale_dim" else d["dim"] // 8)


def ar_emulated_fwd(d, form: str = "honest"):
    """attn_reduce_fwd_kernel (:93-130) in fp32: ``out`` [S, dim], ``lse`` [S, 8]."""
    assert form == "honest" or form in AR_WRONG, form
    dim, nb, T, Lr = d["dim"], d["nb"], d["T"], d["Lr"]  # noqa: N806
    S = nb * Lr  # noqa: N806
    heads = 16 if form == "heads_of_16" else 8
    kvs = d["kv"].float()[ar_rows(nb, T, Lr, form == "row_order")]
    k, v = kvs[..., :dim].reshape(S, T, heads, -1), kvs[..., dim:].reshape(S, T, heads, -1)
    q = (d["query"] * _ar_scale(d, form)).reshape(heads, -1)
    m, s = torch.full((S, heads), -INF), torch.zeros(S, heads)
    acc = torch.zeros(S, heads, dim // heads)
    for t in range(T):
        dot = (q * k[:, t]).sum(-1)
        m_new = torch.maximum(m, dot)
        c, p = expf32(m - m_new), expf32(dot - m_new)
        if form == "no_rescale":
            c = torch.ones_like(c)
        s = s * c + p
        acc = acc * c[..., None] + p[..., None] * v[:, t]
        m = m_new
    lse = m + (s if form == "lse_linear" else logf32(s))
    return dict(out=(acc * (1.0 / s)[..., None]).reshape(S, dim), lse=lse[:, ::2] if heads == 16 else lse)


def ar_emulated_bwd(d, out, lse, form: str = "honest"):
    """attn_reduce_bwd_kernel (:133-180) in fp32 on the ``out`` / ``lse`` it is handed: ``dkv`` (bf16 values, rows as kv),
    ``dq`` [blocks, dim]."""
    assert form == "honest" or form in AR_WRONG, form
    dim, nb, T, Lr = d["dim"], d["nb"], d["T"], d["Lr"]  # noqa: N806
    S, dh = nb * Lr, dim // 8  # noqa: N806
    rows = ar_rows(nb, T, Lr, form == "row_order")
    kvs = d["kv"].float()[rows]
    k, v = kvs[..., :dim].reshape(S, T, 8, dh), kvs[..., dim:].reshape(S, T, 8, dh)
    scale = _ar_scale(d, form)
    q = (d["query"] * scale).reshape(8, dh)
    g, o = d["dout"].reshape(S, 8, dh), out.float().reshape(S, 8, dh)
    delta = (g * o).sum(-1)
    if form == "delta_full_dim":
        delta = delta.sum(-1, keepdim=True).expand(S, 8)
    dot = (q * k).sum(-1)
    dp = (g[:, None] * v).sum(-1)
    p = expf32(dot - lse.float()[:, None])
    ds = p * (dp - delta[:, None])
    dk = bf16_round(ds[..., None] * (d["query"].reshape(8, dh) if form == "dk_unscaled_q" else q))
    dv = bf16_round(p[..., None] * g[:, None])
    dq = (ds[..., None] * k).sum(1).reshape(S, dim)
    if form != "dq_unscaled":
        dq = dq * scale
    dkv = torch.full((nb * T * Lr, 2 * dim), float("nan"))
    dkv[rows] = torch.cat([dk.reshape(S, T, dim), dv.reshape(S, T, dim)], -1)
    return dict(dkv=dkv, dq=ex.block_sums(dq, AR_SEQ_PER_BLOCK))


def ar_emulated(d, form: str = "honest"):
    """Forward, then the backward chained on the forward's own out / lse (a backward-only form runs on the honest forward)."""
    f = ar_emulated_fwd(d, form if form in AR_WRONG_FWD else "honest")
    b = ar_emulated_bwd(d, f["out"], f["lse"], form if form not in ("heads_of_16", "no_rescale", "lse_linear") else "honest")
    return dict(f, **b)


def ar_ratios(d, got, drop=()):
    """got: ``out``, ``lse``, ``dkv`` [rows, 2 dim], ``dq`` [blocks, dim] (the backward having been handed got's out / lse).

    ``one_key``: softmax over one key is 1, so out == v and dv == bf16(dout) bitwise, lse == fl(q fl(scale)) k (one power-of-two
    key element per head: the dot is one exact product), dk == 0 and dq == 0 (delta and dp are the same integer sum).
    ``equal_keys``: out is the exact mean of the integer v over T = 2^n keys; the rest is held to the bound."""
    r, dim, T, kind = d["ref"], d["dim"], d["T"], d["kind"]  # noqa: N806
    S = r["out"].shape[0]  # noqa: N806
    out, lse, dq = got["out"].double().cpu(), got["lse"].double().cpu(), got["dq"].double().cpu()
    dkv = got["dkv"].double().cpu()[r["rows"]]
    dk, dv = dkv[..., :dim], dkv[..., dim:]
    res = {}
    if not all(bool(torch.isfinite(t).all()) for t in (out, lse, dq, dkv)):
        return dict(finite=INF)
    b = ar_bounds(d, lse_err=(lse - r["lse"]).abs(), out_err=(out - r["out"]).abs(), drop=drop)
    want = dict(out=r["out"], lse=r["lse"], dk=r["dk"], dv=r["dv"], dq=r["dq"])
    have = dict(out=out, lse=lse, dk=dk, dv=dv, dq=dq)
    exact = {}
    if kind == "one_key":
        q32 = d["query"] * _scale32(dim // 8)
        kk = d["kv"].float()[r["rows"]][:, 0, :dim]
        exact = dict(out=r["v"].reshape(S, dim), lse=(q32 * kk).double().reshape(S, 8, -1).sum(-1), dv=bf16_round(d["dout"]).double()[:, None],
                     dk=torch.zeros(S, 1, dim, dtype=torch.float64), dq=torch.zeros_like(r["dq"]))
    elif kind == "equal_keys":
        exact = dict(out=r["v"].reshape(S, T, dim).sum(1) / T)
    for key in want:
        if key in exact:
            res[key] = exact_ratio(have[key], exact[key])
        else:
            res[key] = worst_ratio((have[key] - want[key]).abs(), b[key])
    return res


# ================================================================================================ mean reduction
MEAN_CASES = [("exact", 1, 1, 1, 4), ("exact", 3, 8, 5, 192), ("randn", 3, 7, 5, 768)]


@functools.lru_cache(maxsize=None)
def mean_case(kind: str, nb: int, T: int, Lr: int, dim: int):  # noqa: N803
    g = _gen("mean", kind, nb, T, Lr, dim)
    draw = (lambda *s: _ints(g, s)) if kind == "exact" else (lambda *s: torch.randn(*s, generator=g))
    x, dout = draw(nb * T * Lr, dim), draw(nb * Lr, dim)
    x4 = x.double().reshape(nb, T, Lr, dim)
    if kind == "exact":
        assert ex.is_power_of_two(T) and ex.is_order_free(x4, 1.0, dim=1) and ex.is_order_free(dout, 1.0 / T, dim=None if dout.numel() < 256 else 0)
    return dict(kind=kind, nb=nb, T=T, Lr=Lr, dim=dim, x=x, dout=dout, out=x4.sum(1).reshape(nb * Lr, dim) / T, absum=x4.abs().sum(1).reshape(nb * Lr, dim) / T,
                dx=(dout.double().reshape(nb, 1, Lr, dim) / T).expand(nb, T, Lr, dim).reshape(-1, dim))


def mean_emulated(d, form: str = "honest"):
    assert form == "honest"
    nb, T, Lr, dim = d["nb"], d["T"], d["Lr"], d["dim"]  # noqa: N806
    inv = torch.tensor(1.0) / torch.tensor(float(T))
    x4 = d["x"].reshape(nb, T, Lr, dim)
    acc = torch.zeros(nb, Lr, dim)
    for t in range(T):
        acc = acc + x4[:, t]
    return dict(out=(acc * inv).reshape(nb * Lr, dim), dx=(d["dout"].reshape(nb, 1, Lr, dim) * inv).expand(nb, T, Lr, dim).reshape(-1, dim))


def mean_ratios(d, got):
    """Forward (:189-190): an fp32 sum of T terms (T 2^-23 of the magnitudes), fl(1 / T) and the product (2 u |out|); backward
    (:198): fl(1 / T) and the product (2 u)."""
    if d["kind"] == "exact":
        return dict(out=exact_ratio(got["out"], d["out"]), dx=exact_ratio(got["dx"], d["dx"]))
    return dict(out=_ratio(got["out"], d["out"], d["T"] * ACC * d["absum"] + 2 * U * d["out"].abs()),
                dx=_ratio(got["dx"], d["dx"], 2 * U * d["dx"].abs()))


# ================================================================================================ classification linear
LINEAR_E = (64, 100, 192, 1024)            # 100: a partial last lane stride of the forward's wave
LINEAR_BC = ((6, 15), (40, 7), (1, 1))     # (40, 7): B > C, the launch is sized by B E
LINEAR_CASES = [(kind, E, B, C) for kind in ("exact", "randn") for E in LINEAR_E for B, C in LINEAR_BC]
LINEAR_WRONG = ("no_bias", "dW_overwrite", "db_per_column", "dx_transposed")
LINEAR_BOUND_TERMS = ("acc",)


def linear_range(E: int) -> int:  # noqa: N803
    """Largest r <= 255 with E r^2 + 255 < 2^24: |x|, |W| <= r keeps the forward's sum order-free (255 fits E = 192, not 1024)."""
    return min(ex.INT_MAX, math.isqrt(int((ex.F32_INTS - ex.INT_MAX - 1) // E)))


@functools.lru_cache(maxsize=None)
def linear_case(kind: str, E: int, B: int, C: int):  # noqa: N803
    g = _gen("linear", kind, E, B, C)
    if kind == "exact":
        r = linear_range(E)
        x, W, bias, dout = _ints(g, (B, E), r), _ints(g, (C, E), r), _ints(g, (C,)), _ints(g, (B, C))  # noqa: N806
        pre_w, pre_b = _ints(g, (C, E)), _ints(g, (C,))
        assert ex.is_order_free(torch.cat([(x[:, None] * W[None]).reshape(B * C, E), bias.repeat(B)[:, None]], 1), 1.0, dim=1)
        assert ex.is_order_free(torch.cat([(dout[:, :, None] * x[:, None]).reshape(B, C * E), pre_w.reshape(1, -1)]), 1.0, dim=0)
        assert ex.is_order_free(torch.cat([dout, pre_b[None]]), 1.0, dim=0)
        assert ex.is_order_free((dout[:, :, None] * W[None]).reshape(B, C, E), 1.0, dim=1)
    else:
        x, W, bias, dout = (torch.randn(*s, generator=g) for s in ((B, E), (C, E), (C,), (B, C)))  # noqa: N806
        pre_w, pre_b = torch.randn(C, E, generator=g), torch.randn(C, generator=g)
    x64, w64, d64 = x.double(), W.double(), dout.double()
    return dict(kind=kind, E=E, B=B, C=C, x=x, W=W, bias=bias, dout=dout, pre_w=pre_w, pre_b=pre_b,
                out=x64 @ w64.t() + bias.double(), dx=d64 @ w64, dW=pre_w.double() + d64.t() @ x64, db=pre_b.double() + d64.sum(0))


def linear_bounds(d, drop=()):
    """Forward (:210-212): E rounded products (u); each lane adds ceil(E / 64) of them one after the other, wave_sum six more
    times: a term passes at most ceil(E / 64) + 6 additions -- ``acc`` --; the sum with the bias (u).
    Backward (:223-235): one thread adds the B (dW, db) or C (dx) terms in turn (B 2^-23, C 2^-23), and the sum onto what
    dW / db hold (u on both)."""
    a = 0.0 if "acc" in drop else 1.0
    x, W, dout = d["x"].double().abs(), d["W"].double().abs(), d["dout"].double().abs()  # noqa: N806
    E, B, C = d["E"], d["B"], d["C"]  # noqa: N806
    pw, pb = d["pre_w"].double().abs(), d["pre_b"].double().abs()
    return dict(out=a * ((-(-E // 64) + 6) * ACC + U) * (x @ W.t()) + U * (d["out"].abs() + d["bias"].double().abs()),
                dx=a * (C * ACC + U) * (dout @ W),
                dW=a * (B * ACC + U) * (dout.t() @ x) + U * (pw + d["dW"].abs()),
                db=a * B * ACC * dout.sum(0) + U * (pb + d["db"].abs()))


def linear_emulated(d, form: str = "honest"):
    assert form == "honest" or form in LINEAR_WRONG, form
    x, W, dout = d["x"], d["W"], d["dout"]  # noqa: N806
    out = nm._wave_sum(x[:, None] * W[None])
    if form != "no_bias":
        out = out + d["bias"]
    dx = dout @ W
    if form == "dx_transposed":
        dx = dx.t().reshape(d["B"], d["E"])
    s = dout.t() @ x
    t = dout.sum(0) * (d["E"] if form == "db_per_column" else 1)
    return dict(out=out, dx=dx, dW=s if form == "dW_overwrite" else d["pre_w"] + s, db=d["pre_b"] + t)


def linear_ratios(d, got, drop=()):
    """got: ``out``, ``dx``, ``dW``, ``db`` (on the preloads), and optionally ``dW_nodx``, ``db_nodx``: the run with dx = NULL, which
    must give the same bits."""
    if d["kind"] == "exact":
        r = {k: exact_ratio(got[k], d[k]) for k in ("out", "dx", "dW", "db")}
    else:
        b = linear_bounds(d, drop)
        r = {k: _ratio(got[k], d[k], b[k]) for k in ("out", "dx", "dW", "db")}
    for k in ("dW", "db"):
        if k + "_nodx" in got:
            r[k + "_nodx"] = 0.0 if same_bits(got[k + "_nodx"].cpu(), got[k].cpu()) else INF
    return r


# ================================================================================================ cross entropy
CE_KINDS = ("randn2", "randn30", "offset1e4")
# (kind, C, B, g, P, pad, n_valid mode, dlogits dtype, target bytes).  Modes: "count" (about a fifth missing; the word is the true
# count), "all" (nothing missing), "pow2" (the largest power of two <= 3/4 of the pixels valid), "one", "zero" (all missing),
# "word" (as pow2, but the word handed over is half the true count).  255 / 256 / 257 pixels: the classification layout.
CE_CASES = [
    ("saturated", 2, 1, 1, 1, 0, "one", "f32", 8),
    ("saturated", 19, 5, 1, 1, 12, "pow2", "bf16", 4),
    ("saturated", 19, 255, 1, 1, 0, "pow2", "f32", 2),
    ("saturated", 130, 256, 1, 1, 12, "all", "bf16", 8),
    ("saturated", 2, 257, 1, 1, 0, "pow2", "f32", 1),
    ("saturated", 19, 3, 2, 4, 12, "pow2", "bf16", 1),
    ("saturated", 130, 2, 4, 8, 0, "all", "f32", 4),
    ("saturated", 19, 2, 4, 8, 12, "pow2", "f32", 8),
    ("saturated", 1, 5, 1, 1, 0, "pow2", "f32", 4),
    ("saturated", 19, 3, 2, 4, 0, "word", "f32", 8),
    ("saturated", 19, 3, 2, 4, 12, "word", "bf16", 2),
    ("saturated", 19, 5, 1, 1, 0, "zero", "f32", 8),
    ("saturated", 19, 2, 4, 8, 12, "one", "bf16", 4),
]
for _k in CE_KINDS:
    CE_CASES += [(_k, 19, 3, 2, 4, 12, "count", "f32", 8), (_k, 130, 2, 4, 8, 0, "count", "bf16", 4), (_k, 2, 257, 1, 1, 0, "count", "f32", 2),
                 (_k, 19, 256, 1, 1, 12, "all", "bf16", 1), (_k, 19, 1, 1, 1, 0, "one", "f32", 8)]
CE_CASES += [("randn2", 1, 5, 1, 1, 0, "count", "f32", 4), ("randn2", 19, 255, 1, 1, 0, "pow2", "f32", 2), ("randn30", 19, 5, 1, 1, 12, "zero", "bf16", 8)]
CE_WRONG = ("mean_over_all", "missing_gets_grad", "layout_c_first", "no_max_subtraction", "own_count")
CE_BOUND_TERMS = ("lse_round", "store")
CE_INT = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def ce_index(B: int, g: int, P: int, C: int, ld: int, c_first: bool = False) -> torch.Tensor:  # noqa: N803
    """[n_pix, C] flat indices into the [B g g, ld] patch-layout buffer (:274-275); ``c_first``: the WRONG column order (c p1 p2)."""
    S = g * P  # noqa: N806
    i = torch.arange(B * S * S)
    X, r = i % S, i // S  # noqa: N806
    Y, b = r % S, r // S  # noqa: N806
    tok, pix = b * g * g + (Y // P) * g + X // P, (Y % P) * P + X % P
    c = torch.arange(C)[None]
    col = c * P * P + pix[:, None] if c_first else pix[:, None] * C + c
    return tok[:, None] * ld + col


@functools.lru_cache(maxsize=None)
def ce_case(kind: str, C: int, B: int, g: int, P: int, pad: int, mode: str, dd: str, tbytes: int):  # noqa: N803
    """``logits`` f32 [B g g, ld] (pad columns NaN), ``target`` of ``tbytes`` bytes, ``missing``, the n_valid ``word``, and the
    expectations ``loss`` (fp64 scalar) and ``dl`` [n_pix, C] (fp64; the closed form for ``saturated``, F.cross_entropy's value in
    fp64 arithmetic otherwise, both over the word)."""
    gen = _gen("ce", kind, C, B, g, P, pad, mode, dd, tbytes)
    ld, n_pix = P * P * C + pad, B * g * g * P * P
    missing = C if tbytes == 2 else -1
    idx = ce_index(B, g, P, C, ld)
    t = torch.randint(0, C, (n_pix,), generator=gen)
    perm = torch.randperm(n_pix, generator=gen)
    n_keep = dict(count=None, all=n_pix, pow2=2 ** int(math.log2(max(1, 3 * n_pix // 4))), word=2 ** int(math.log2(max(1, 3 * n_pix // 4))),
                  one=1, zero=0)[mode]
    if n_keep is None:
        t[torch.rand(n_pix, generator=gen) < 0.2] = missing
    else:
        t[perm[n_keep:]] = missing
    valid = t != missing
    count = int(valid.sum())
    word = count // 2 if mode == "word" else count
    assert mode != "word" or (word >= 1 and ex.is_power_of_two(word))
    if kind == "saturated":
        pred = torch.randint(0, C, (n_pix,), generator=gen)
        lg = torch.full((n_pix, C), -128.0)
        lg[torch.arange(n_pix), pred] = 0.0
    else:
        lg = torch.randn(n_pix, C, generator=gen) * (30.0 if kind == "randn30" else 2.0 if kind == "randn2" else 1.0)
        if kind == "offset1e4":
            lg = lg + 1.0e4
    logits = torch.full((B * g * g * ld,), float("nan"))
    logits[idx] = lg
    d = dict(kind=kind, C=C, B=B, g=g, P=P, ld=ld, mode=mode, dd=torch.float32 if dd == "f32" else torch.bfloat16, missing=missing,
             logits=logits.reshape(B * g * g, ld), target=t.to(CE_INT[tbytes]).reshape(B, g * P, g * P), word=word, count=count, idx=idx,
             valid=valid & (word > 0), t=t.clamp(0, C - 1), lg=lg)
    use = d["valid"]
    onehot = F.one_hot(d["t"], C).double()
    if kind == "saturated":
        assert word == 0 or ex.is_power_of_two(word)                # 1 / word, 128 / word and their bf16 images are exact
        wrong = use & (pred != d["t"])
        terms = wrong.double() * 128.0 / max(word, 1)
        assert ex.is_order_free(terms, 128.0 / max(word, 1))
        d["loss"] = terms.sum()
        d["dl"] = (F.one_hot(pred, C).double() - onehot) * use[:, None] / max(word, 1)
    else:
        x = lg.double()
        lse = torch.logsumexp(x, -1)
        per = (lse - x.gather(1, d["t"][:, None])[:, 0]) * use / max(word, 1)
        d.update(loss=per.sum(), per=per, lse=lse, dl=(torch.exp(x - lse[:, None]) - onehot) * use[:, None] / max(word, 1))
    return d


def ce_bounds(d, drop=()):
    """``(b_loss, b_dl [n_pix, C])``.  Per pixel (:280-288): m is a logit itself; s = sum expf(x - m) -- ``exp_rel`` on each term, an fp32
    sum of C terms (C 2^-23); lse = m + logf(s): the relative error of s, v_log_f32 and ln 2 (2^-22 log s + u), and ``lse_round``,
    the sum's own rounding u |lse| -- at logits of 1e4 that is 6e-4, the cancellation this form of the loss has; loss =
    (lse - x_t) fl(1 / n) (3 u).  d = (expf(x - lse) - 1h) inv: the error of lse is a relative error of the exponential, plus
    ``exp_rel``; the subtraction, 1 / n and the product (3 u); ``store``: HB for a bf16 dlogits.  The loss word is an fp32 sum
    of the pixels' terms: six shuffles and two LDS sums in a block, then atomics in any order, one per block: a term passes at
    most 8 + ceil(n_pix / 256) additions, so the term grows with the number of blocks as gemm_bound's does with K; u on acc."""
    assert set(drop) <= set(CE_BOUND_TERMS)
    x, C = d["lg"].double(), d["C"]  # noqa: N806
    inv = d["valid"].double() / max(d["word"], 1)
    m = x.max(-1, keepdim=True).values
    sm = torch.exp(x - d["lse"][:, None])
    sig = (sm * exp_rel(x - m)).sum(-1) + C * ACC
    b_lse = sig + EXP_ULP * (d["lse"] - m[:, 0]).abs() + U + (0.0 if "lse_round" in drop else U) * d["lse"].abs()
    xt = x.gather(1, d["t"][:, None])[:, 0]
    b_per = (b_lse + U * (d["lse"] - xt).abs()) * inv + 2 * U * d["per"].abs()
    n_pix = x.shape[0]
    b_loss = b_per.sum() + (8 + -(-n_pix // 256)) * ACC * d["per"].abs().sum() + U * d["loss"].abs()
    rho = torch.expm1(b_lse[:, None] + 3 * U * (x - d["lse"][:, None]).abs()) + EXP_ULP
    onehot = F.one_hot(d["t"], C).double()
    b_dl = (sm * rho + U * (sm - onehot).abs() + FL) * inv[:, None] + 2 * U * d["dl"].abs()
    if d["dd"] == torch.bfloat16 and "store" not in drop:
        b_dl = b_dl + HB * (d["dl"].abs() + b_dl) + FL * d["valid"][:, None]
    return b_loss, b_dl


def ce_emulated(d, form: str = "honest"):
    """ce_loss_kernel (:264-304) in fp32: ``acc`` (from 0) and the ``dlogits`` buffer [B g g, ld] of the case's dtype on a NaN fill."""
    assert form == "honest" or form in CE_WRONG, form
    C, n = d["C"], d["count"] if form == "own_count" else d["word"]  # noqa: N806   own_count: ignores the word it is handed
    idx = ce_index(d["B"], d["g"], d["P"], C, d["ld"], form == "layout_c_first").clamp_max(d["logits"].numel() - 1)
    x = d["logits"].reshape(-1)[idx]
    m = torch.zeros(x.shape[0], 1) if form == "no_max_subtraction" else x.max(-1, keepdim=True).values
    lse = m[:, 0] + logf32(expf32(x - m).sum(-1))
    inv = torch.tensor(1.0) / torch.tensor(float(x.shape[0] if form == "mean_over_all" else max(n, 1)))
    onehot = F.one_hot(d["t"], C).float()
    valid = d["valid"]
    per = torch.where(valid, (lse - x.gather(1, d["t"][:, None])[:, 0]) * inv, torch.zeros(()))
    dl = torch.where(valid[:, None], (expf32(x - lse[:, None]) - onehot) * inv, torch.zeros(()))
    if form == "missing_gets_grad" and n > 0:
        dl = torch.where(valid[:, None], dl, expf32(x - lse[:, None]) * inv)
    buf = torch.full((d["logits"].numel(),), float("nan"), dtype=d["dd"])
    buf[idx] = dl.to(d["dd"])
    return dict(acc=nm._wave_sum(per[None])[0].reshape(1), dlogits=buf.reshape(d["logits"].shape))


def ce_ratios(d, got, drop=()):
    """got: ``acc`` [1] (preloaded with 0), ``dlogits`` [B g g, ld] written onto a NaN fill: every live column must have been
    written, every pad column must still hold the fill."""
    buf = got["dlogits"].cpu().reshape(-1)
    live = torch.zeros(buf.numel(), dtype=torch.bool)
    live[d["idx"]] = True
    r = dict(pad=0.0 if bool(torch.isnan(buf[~live].float()).all()) else INF)
    dl, acc = buf[d["idx"]], got["acc"].cpu().reshape(())
    if d["kind"] == "saturated":
        r.update(loss=exact_ratio(acc, d["loss"]), dl=exact_ratio(dl, d["dl"]))
        if d["word"] == 0:
            r["zero_sign"] = 0.0 if not bool(torch.signbit(dl.float()).any()) else INF        # +0 on missing pixels
    elif d["word"] == 0:
        r.update(loss=exact_ratio(acc, torch.zeros((), dtype=torch.float64)), dl=exact_ratio(dl, torch.zeros_like(d["dl"])))
    else:
        b_loss, b_dl = ce_bounds(d, drop)
        r.update(loss=_ratio(acc, d["loss"], b_loss), dl=_ratio(dl, d["dl"], b_dl))
    return r


# ================================================================================================ BCE with logits
BCE_KINDS = ("randn2", "randn30", "pm90")
# (kind, B, C, skip): "none"; "some" -- rows 2, 7, 256, 258 and the last one where they exist; "half" -- every odd row; "tail" --
# rows >= 256; "all".  (257, 3) and (300, 16) make both += 256 loops of the kernel wrap (B > 256 and B C > 256).
BCE_CASES = [("saturated", 1, 1, "none"), ("saturated", 256, 1, "none"), ("saturated", 256, 1, "half"), ("saturated", 300, 16, "tail"),
             ("saturated", 300, 16, "all"), ("randn2", 9, 15, "all"), ("randn30", 257, 3, "all")]
BCE_CASES += [(k, B, C, s) for k in BCE_KINDS for B, C, s in ((1, 1, "none"), (9, 15, "some"), (256, 1, "some"), (257, 3, "some"), (300, 16, "some"))]
BCE_WRONG = ("per_element_filter", "mean_over_all_rows", "naive_log1pexp", "first_256_only")
BCE_BOUND_TERMS = ("exp",)
BCE_MISSING = -1.0
BCE_ACC0 = 3.0              # what acc holds before the call


@functools.lru_cache(maxsize=None)
def bce_case(kind: str, B: int, C: int, skip: str):  # noqa: N803
    gen = _gen("bce", kind, B, C, skip)
    t = (torch.rand(B, C, generator=gen) < 0.4).float()
    if kind == "saturated":
        x = 128.0 * (1 - 2 * (torch.rand(B, C, generator=gen) < 0.5).float())
    elif kind == "pm90":
        x = (90.0 + torch.rand(B, C, generator=gen)) * (1 - 2 * (torch.rand(B, C, generator=gen) < 0.5).float())
    else:
        x = torch.randn(B, C, generator=gen) * (30.0 if kind == "randn30" else 2.0)
    rows = dict(none=[], some=[r for r in sorted({2, 7, 256, 258, B - 1}) if r < B and B > 1], half=list(range(1, B, 2)),
                tail=list(range(256, B)), all=list(range(B)))[skip]
    for r in rows:                                    # ONE missing target in the row drops all of it
        t[r, int(torch.randint(0, C, (1,), generator=gen))] = BCE_MISSING
    used = torch.ones(B, dtype=torch.bool)
    used[rows] = False
    n = int(used.sum()) * C
    d = dict(kind=kind, B=B, C=C, skip=skip, x=x, t=t, used=used, n=n)
    x64, t64, m = x.double(), t.double(), used[:, None].double() / max(n, 1)
    if kind == "saturated" or n == 0:
        assert n == 0 or ex.is_power_of_two(n)
        terms = torch.where(t64 == (x64 > 0), torch.zeros_like(x64), x64.abs()) * m
        assert ex.is_order_free(torch.cat([terms.reshape(-1), torch.tensor([BCE_ACC0], dtype=torch.float64)]), min(1.0, 128.0 / max(n, 1)))
        d.update(terms=terms, loss=terms.sum() + BCE_ACC0, dl=((x64 > 0).double() - t64) * m)
    else:
        terms = (x64.clamp_min(0) - x64 * t64 + torch.log1p(torch.exp(-x64.abs()))) * m
        d.update(terms=terms, loss=terms.sum() + BCE_ACC0, dl=(torch.sigmoid(x64) - t64) * m)
    return d


def bce_bounds(d, drop=()):
    """``(b_loss, b_dl)``.  Term (:331): max(x, 0) and x t are exact (t is 0 or 1); e = expf(-|x|) -- ``exp``: ``exp_rel``, carried
    through log1p (e / (1 + e)); log1pf itself 2^-22 of its value; two sums (2 u); inv = 1 / (fl(n_rows) C) and the product
    (3 u).  The word: per thread an fp32 sum of its ceil(B C / 256) terms, six shuffles, two LDS sums: (8 + ceil(B C / 256)) 2^-23
    of the terms -- and u on acc.
    d (:332): e' = expf(-x) (``exp_rel``; inf above x = -88.7, where the true sigmoid is below FL), 1 + e' and the quotient (2 u):
    sig (eps (1 - sig) + 2 u); the subtraction (u |sig - t|); inv and the product (3 u)."""
    assert set(drop) <= set(BCE_BOUND_TERMS)
    x, t, m = d["x"].double(), d["t"].double(), d["used"][:, None].double() / max(d["n"], 1)
    eps = exp_rel(x) if "exp" not in drop else torch.zeros_like(x)
    e = torch.exp(-x.abs())
    l1p = torch.log1p(e)
    lin = (x.clamp_min(0) - x * t).abs()
    b_term = (e * eps / (1 + e) + EXP_ULP * l1p + FL + 2 * U * (lin + l1p)) * m + 3 * U * d["terms"].abs()
    b_loss = b_term.sum() + (8 + -(-d["B"] * d["C"] // 256)) * ACC * d["terms"].abs().sum() + U * (BCE_ACC0 + d["loss"].abs())
    sig = torch.sigmoid(x)
    b_dl = (sig * (eps * (1 - sig) + 2 * U) + U * (sig - t).abs() + FL) * m + 3 * U * d["dl"].abs() + FL
    return b_loss, b_dl


def bce_emulated(d, form: str = "honest"):
    """bce_loss_kernel (:308-340) in fp32: ``acc`` (from BCE_ACC0), ``dlogits`` [B, C] on a NaN fill."""
    assert form == "honest" or form in BCE_WRONG, form
    x, t, B, C = d["x"], d["t"], d["B"], d["C"]  # noqa: N806
    ok_row = (t != BCE_MISSING).all(1)
    if form == "first_256_only":
        ok_row = ok_row & (torch.arange(B) < 256)
    ok = ok_row[:, None].expand(B, C)
    n = float(int(ok_row.sum())) * C
    if form == "per_element_filter":
        ok = t != BCE_MISSING
        n = float(int(ok.sum()))
    if form == "mean_over_all_rows":
        n = float(B * C)
    inv = torch.tensor(1.0) / torch.tensor(n) if n > 0 else torch.tensor(0.0)
    soft = logf32(1.0 + expf32(x)) - x.clamp_min(0) if form == "naive_log1pexp" else torch.log1p(expf32(-x.abs()))
    term = torch.where(ok, (x.clamp_min(0) - x * t + soft) * inv, torch.zeros(()))
    dl = torch.where(ok, (1.0 / (1.0 + expf32(-x)) - t) * inv, torch.zeros(()))
    if form == "first_256_only":
        live = (torch.arange(B * C) < 256).reshape(B, C)
        term, dl = torch.where(live, term, torch.zeros(())), torch.where(live, dl, torch.full((), float("nan")))
    flat = term.reshape(-1)
    flat = torch.cat([flat, flat.new_zeros((-flat.numel()) % 256)]).reshape(-1, 256)
    thread = torch.zeros(256)
    for row in flat:
        thread = thread + row
    return dict(acc=(torch.tensor(BCE_ACC0) + nm._wave_sum(thread[None])[0]).reshape(1), dlogits=dl)


def bce_ratios(d, got, drop=()):
    """got: ``acc`` [1] (preloaded with BCE_ACC0), ``dlogits`` [B, C] on a NaN fill."""
    acc, dl = got["acc"].cpu().reshape(()), got["dlogits"].cpu()
    if d["kind"] == "saturated" or d["n"] == 0:
        r = dict(loss=exact_ratio(acc, d["loss"]), dl=exact_ratio(dl, d["dl"]))
        if d["n"] == 0:
            r["acc_kept"] = 0.0 if float(acc) == BCE_ACC0 else INF
        return r
    b_loss, b_dl = bce_bounds(d, drop)
    return dict(loss=_ratio(acc, d["loss"], b_loss), dl=_ratio(dl, d["dl"], b_dl))


# ================================================================================================ the families, for the self-check
def case_id(case) -> str:
    return "-".join(str(c) for c in case)


FAMILIES = {
    "resize": (RESIZE_CASES, resize_case, resize_emulated, resize_ratios, RESIZE_WRONG),
    "attn_reduce": (AR_CASES, ar_case, ar_emulated, ar_ratios, AR_WRONG),
    "mean_reduce": (MEAN_CASES, mean_case, mean_emulated, mean_ratios, ()),
    "head_linear": (LINEAR_CASES, linear_case, linear_emulated, linear_ratios, LINEAR_WRONG),
    "ce": (CE_CASES, ce_case, ce_emulated, ce_ratios, CE_WRONG),
    "bce": (BCE_CASES, bce_case, bce_emulated, bce_ratios, BCE_WRONG),
}
