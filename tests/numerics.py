"""Operand generators, fp64 references and a-priori error bounds for the numerics tests.

Used by tests/test_numerics_selfcheck.py (CPU: the bounds accept honest fp32 implementations and reject subtly wrong ones) and
tests/test_numerics_gpu.py (the HIP kernels against the same bounds).  Nothing here is fitted to what the kernels give:

* GEMM (``gemm_bound``): bf16 x bf16 products are exact in fp32, so an fp32 accumulation of K of them in ANY order obeys
  |C - C64| <= gamma_K (|A| |B|) with gamma_K ~ K u (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1); the
  constant used is 2 u = 2^-23 per term, which also admits an accumulator that truncates instead of rounding to nearest.
* bf16 store: half a bf16 ulp, 2^-8 relative (8 significand bits).
* GELU: the three-term erf of csrc/common.hpp (Abramowitz-Stegun 7.1.25) is documented at |error| <= 2.5e-5 on erf, i.e. 1.25e-5 on
  the CDF; 2^-22 covers the handful of fp32 roundings of the epilogue's arithmetic.
* Normalisation statistics (``norm_ceiling``): twice the larger error of two honest fp32 algorithms (torch's own op; a two-pass
  reduction in wave order, ``wave_two_pass_stats``) against fp64 on the very inputs of the case.
* Attention (``attn_bounds``): a first-order propagation of every rounding of csrc/attn.hip through softmax and its gradient; the
  derivation stands in front of the function, the measured slack in profiles/attn_numerics.md.
* AdamW (``adamw_bounds``): a first-order propagation of the roundings of ``adamw_update`` (csrc/optim.hip) through the moments, the
  square root and the quotient; used by tests/test_adamw_numerics_gpu.py, checked on the CPU by tests/test_step_end_selfcheck.py,
  measured in profiles/step_end_numerics.md.
"""

from __future__ import annotations

import math

import torch

U_F32 = 2.0 ** -24          # unit roundoff of fp32
HALF_ULP_BF16 = 2.0 ** -8   # relative half ulp of bf16 (8 significand bits)
GELU_CDF_ERR = 1.25e-5      # half of the stated erf error of the three-term form (csrc/common.hpp, A-S 7.1.25: 2.5e-5)
U8_HALF_STEP = 1.0 / 400.0  # half a step of the byte-coded GELU' (code = round((d + 0.13) * 200))

DISTRIBUTIONS = ("randn", "offset", "lognormal", "cancel")


def bf16_round(x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.bfloat16).to(torch.float32)


def bf16_truncate(x: torch.Tensor) -> torch.Tensor:
    """fp32 -> the bf16 value below it in magnitude (what a store without rounding would write)."""
    return (x.contiguous().view(torch.int32) & -65536).view(torch.float32)


# ------------------------------------------------------------------------------------------------ GEMM operands
def gemm_operands(dist: str, M: int, N: int, K: int, seed: int = 0):  # noqa: N803
    """``a [M, K]``, ``b [K, N]`` as fp32 CPU tensors holding bf16-representable values."""
    g = torch.Generator().manual_seed(1000003 * seed + 7 * M + 3 * N + K + 101 * DISTRIBUTIONS.index(dist))
    rs = K ** -0.5
    if dist == "randn":
        a, b = torch.randn(M, K, generator=g), torch.randn(K, N, generator=g) * rs
    elif dist == "offset":      # every product has the same sign: sum |a b| = |sum a b|, the bound is tight
        a, b = torch.randn(M, K, generator=g).abs() + 1.0, (torch.randn(K, N, generator=g) * rs).abs() + 0.02
    elif dist == "lognormal":
        a = torch.randn(M, K, generator=g) * torch.exp(2.0 * torch.randn(M, K, generator=g))
        b = torch.randn(K, N, generator=g) * torch.exp(2.0 * torch.randn(K, N, generator=g))
    elif dist == "cancel":      # the second half of K cancels the first up to a 2^-6 relative perturbation
        h = K // 2
        a1, b1 = torch.randn(M, h, generator=g), torch.randn(h, N, generator=g) * rs
        a2 = -a1 * (1.0 + 2.0 ** -6 * torch.randn(M, h, generator=g))
        a, b = torch.cat([a1, a2], 1), torch.cat([b1, b1], 0)
    else:
        raise ValueError(dist)
    return bf16_round(a), bf16_round(b)


def gemm_ref64(a: torch.Tensor, b: torch.Tensor):
    """``(A B, |A| |B|)`` in fp64 on the operands' device."""
    a64, b64 = a.double(), b.double()
    return a64 @ b64, a64.abs() @ b64.abs()


def gemm_bound(absprod: torch.Tensor, K: int) -> torch.Tensor:  # noqa: N803
    """|C - C64| <= K 2^-23 (|A| |B|) for fp32 accumulation of exact products in any order."""
    return K * 2.0 ** -23 * absprod


def bf16_store_bound(c64: torch.Tensor, absprod: torch.Tensor, K: int) -> torch.Tensor:  # noqa: N803
    return HALF_ULP_BF16 * c64.abs() + gemm_bound(absprod, K)


def bias_residual_bound(acc64, absprod, K, bias64, res64) -> torch.Tensor:  # noqa: N803
    """fp32 output of acc + bias + res: the accumulation bound plus two fp32 additions."""
    return gemm_bound(absprod, K) + 2 * U_F32 * (acc64.abs() + bias64.abs() + res64.abs())


def atomic_bound(absprod, c0_64, K) -> torch.Tensor:  # noqa: N803
    """Split-K partial sums added atomically onto a preloaded destination."""
    return K * 2.0 ** -23 * (absprod + c0_64.abs())


def worst_ratio(err: torch.Tensor, bound: torch.Tensor) -> float:
    """max(err / bound); an error over a zero bound counts as infinite, 0 / 0 as 0."""
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    return float(r.max())


# ------------------------------------------------------------------------------------------------ GELU
def gelu64(x: torch.Tensor) -> torch.Tensor:
    x = x.double()
    return x * 0.5 * torch.erfc(-x / math.sqrt(2.0))


def dgelu64(x: torch.Tensor) -> torch.Tensor:
    x = x.double()
    return 0.5 * torch.erfc(-x / math.sqrt(2.0)) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def gelu_bound(x64: torch.Tensor) -> torch.Tensor:
    """bf16 GELU output against gelu64 of the exact fp32 pre-activation."""
    return HALF_ULP_BF16 * gelu64(x64).abs() + GELU_CDF_ERR * x64.abs() + 2.0 ** -22 * x64.abs()


def dgelu_err(x64: torch.Tensor) -> torch.Tensor:
    """Error of the fp32 GELU' before any storage rounding."""
    return GELU_CDF_ERR + 2.0 ** -22 * (1.0 + x64.abs())


def dgelu_bound(x64: torch.Tensor, u8: bool = False) -> torch.Tensor:
    """Saved GELU' (bf16, or decoded from its byte code) against gelu'64 of the exact fp32 pre-activation."""
    return HALF_ULP_BF16 * dgelu64(x64).abs() + dgelu_err(x64) + (U8_HALF_STEP if u8 else 0.0)


def decode_u8(code: torch.Tensor) -> torch.Tensor:
    return code.double() / 200.0 - 0.13


def gelu_grid():
    """Pre-activations for the epilogue tests as ``(row part a [bf16 values], column part bias [fp32])``: the epilogue sees
    x[m, n] = fl32(a[m] + bias[n]), one correctly rounded fp32 addition of the (exact) accumulator and the bias.

    Rows: every multiple of 1/4 in [-12, 12] and the tails +-20, +-100, +-1e4 (as bf16), +-0, +-2^-100.  Columns (period 32): column 0
    of each period has bias 0 (the row values themselves, tails included), the others (n % 16) 2^-6 plus an fp32 offset below 2^-6,
    so together every multiple of 2^-6 in [-12, 12] appears, with fp32 offsets."""
    coarse = torch.arange(-48, 49, dtype=torch.float32) / 4.0
    tails = torch.tensor([20.0, -20.0, 100.0, -100.0, 1.0e4, -1.0e4, 0.0, -0.0, 2.0 ** -100, -(2.0 ** -100)])
    a = bf16_round(torch.cat([coarse, tails]))
    g = torch.Generator().manual_seed(17)
    n = torch.arange(32)
    bias = (n % 16).float() * 2.0 ** -6 + torch.rand(32, generator=g) * 2.0 ** -6
    bias[0] = 0.0
    return a, bias


def gelu_cdf_pdf4_emulated(x: torch.Tensor, c1: float = 0.7478556):
    """fp32 emulation of ``gelu_cdf_pdf4`` (csrc/common.hpp, the three-term form) as written; ``c1`` is its first coefficient."""
    x = x.float()
    f = torch.float32
    e = torch.exp2((x * x) * torch.tensor(-0.5 * 1.4426950408889634, dtype=f))
    t = 1.0 / (x.abs() * torch.tensor(0.47047 * 0.70710678118654752, dtype=f) + 1.0)
    poly = (torch.tensor(0.5 * c1, dtype=f) * t + torch.tensor(0.5 * -0.0958798, dtype=f)) * t + torch.tensor(0.5 * 0.3480242, dtype=f)
    h = (poly * t) * e
    cdf = torch.where(x >= 0, 1.0 - h, h)
    pdf = e * torch.tensor(0.3989422804014327, dtype=f)
    return cdf, pdf


def encode_u8_emulated(d: torch.Tensor, wrap: bool = False) -> torch.Tensor:
    """The byte code of GELU' as the epilogue forms it (round to nearest of d * 200 + 26, saturating); ``wrap``: a wrong
    implementation that keeps the low eight bits instead."""
    q = torch.round(d.float() * 200.0 + 26.0).to(torch.int64)
    return (q & 255) if wrap else q.clamp(0, 255)


# ------------------------------------------------------------------------------------------------ emulated accumulators (self-check)
def _rtz_to_f32(x64: torch.Tensor) -> torch.Tensor:
    f = x64.float()
    over = f.double().abs() > x64.abs()
    return torch.where(over, torch.nextafter(f, torch.zeros_like(f)), f)


def matmul_chunked(a: torch.Tensor, b: torch.Tensor, chunk: int, mode: str = "rne", bf16_every: int = 0) -> torch.Tensor:
    """Sequential accumulation over K in chunks (the model of an MFMA K loop).  ``mode``: "rne" fp32 accumulator, "rtz" an
    accumulator that truncates; ``bf16_every`` = n > 0: the WRONG form that rounds the running sum to bf16 every n chunks."""
    M, K = a.shape  # noqa: N806
    acc = torch.zeros(M, b.shape[1])
    for i, k0 in enumerate(range(0, K, chunk)):
        if mode == "rtz":
            acc = _rtz_to_f32(acc.double() + a[:, k0:k0 + chunk].double() @ b[k0:k0 + chunk].double())
        else:
            acc = acc + a[:, k0:k0 + chunk] @ b[k0:k0 + chunk]
        if bf16_every and (i + 1) % bf16_every == 0:
            acc = bf16_round(acc)
    return acc


# ------------------------------------------------------------------------------------------------ normalisation statistics
def norm_inputs(kind: str, rows: int, dim: int, seed: int = 0) -> torch.Tensor:
    """fp32 CPU rows for the off-centre statistics tests.  kinds: ``mu0 mu10 mu100 mu1000`` (mean / sigma at sigma 1), ``small`` /
    ``large`` (mean 0, sigma 1e-3 / 1e3), ``outlier`` (one channel of 200 sigma per row), ``const`` (constant rows: dyadic
    values, so that every fp32 summation order gives mean = the value and variance = 0 exactly)."""
    g = torch.Generator().manual_seed(7919 * seed + 31 * rows + dim + sum(map(ord, kind)))
    z = torch.randn(rows, dim, generator=g)
    if kind.startswith("mu"):
        return float(kind[2:]) + z
    if kind == "small":
        return 1e-3 * z
    if kind == "large":
        return 1e3 * z
    if kind == "outlier":
        col = torch.randint(0, dim, (rows,), generator=g)
        z[torch.arange(rows), col] = 200.0
        return z
    if kind == "const":
        vals = torch.tensor([2.5, -7.0, 1024.0, 0.0, -0.375, 96.0])
        return vals[torch.arange(rows) % len(vals)][:, None].expand(rows, dim).contiguous()
    raise ValueError(kind)


NORM_KINDS = ("mu0", "mu10", "mu100", "mu1000", "small", "large", "outlier", "const")


def _wave_sum(v: torch.Tensor) -> torch.Tensor:
    """fp32 sum over the last axis in the order of a 64-lane wave: each lane adds its elements (stride 64) one after the other,
    then a six-step butterfly over the lanes."""
    n = v.shape[-1]
    pad = (-n) % 64
    if pad:
        v = torch.cat([v, v.new_zeros(*v.shape[:-1], pad)], -1)
    v = v.reshape(*v.shape[:-1], -1, 64)
    lane = v[..., 0, :].clone()
    for i in range(1, v.shape[-2]):
        lane = lane + v[..., i, :]
    w = 64
    while w > 1:
        w //= 2
        lane = lane[..., :w] + lane[..., w:2 * w]
    return lane[..., 0]


def wave_two_pass_stats(x: torch.Tensor, eps: float, unbiased: bool = False):
    """Honest fp32 two-pass (mean, variance, rstd) over the last axis, reduced in wave order."""
    x = x.float()
    n = x.shape[-1]
    mean = _wave_sum(x) / n
    d = x - mean[..., None]
    var = _wave_sum(d * d) / (n - 1 if unbiased else n)
    return mean, var, 1.0 / torch.sqrt(var + eps)


def one_pass_stats(x: torch.Tensor, eps: float):
    """The WRONG-at-large-mean form: var = E[x^2] - E[x]^2 from fp32 sums."""
    x = x.float()
    n = x.shape[-1]
    mean = _wave_sum(x) / n
    var = (_wave_sum(x * x) / n - mean * mean).clamp_min(0.0)
    return mean, var, 1.0 / torch.sqrt(var + eps)


def stats64(x: torch.Tensor, eps: float, unbiased: bool = False):
    x = x.double()
    n = x.shape[-1]
    mean = x.mean(-1)
    var = ((x - mean[..., None]) ** 2).sum(-1) / (n - 1 if unbiased else n)
    return mean, var, 1.0 / torch.sqrt(var + eps)


def max_abs_err(got: torch.Tensor, want64: torch.Tensor) -> float:
    return float((got.double() - want64).abs().max())


def max_rel_err(got: torch.Tensor, want64: torch.Tensor) -> float:
    return float(((got.double() - want64).abs() / want64.abs()).max())


def norm_ceiling(err_a: float, err_b: float) -> float:
    """Twice the larger error of two legitimate fp32 algorithms: the kernel may use a third order of the same quality."""
    return 2.0 * max(err_a, err_b)


# ------------------------------------------------------------------------------------------------ attention
# Per head: q, k, v, do [N, D] fp32 tensors holding bf16 values; scale = D^-0.5, c = scale log2(e).  Kernels: csrc/attn.hip.
LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453
FLUSH_F32 = 2.0 ** -126     # smallest normal fp32: v_exp_f32 and the matrix cores return 0 below it
ATTN_TILE = 64              # keys per forward tile
ATTN_RANGE = 24.0           # LAZY_RANGE of csrc/attn.hip
ATTN_KINDS = ("randn1.5", "randn3", "offset", "neg", "rising", "peaked", "spike_late", "low_after_high")
# terms of attn_bounds that the self-check removes one at a time to show that each is needed
ATTN_BOUND_TERMS = ("fold", "fl_E", "fl_EP", "fl_store")
B_FACTOR = 2.0              # criterion B: norm_ceiling's factor (the kernel may use another order of the same quality)
B_FLOOR = 0.02              # criterion B is void where the emulation's own error norm is below this share of the bound's norm


def attn_operands(kind: str, N: int, D: int, seed: int = 0):  # noqa: N803
    """``q, k, v, do`` [N, D].  The shifted kinds put a logit of about +-40 on one direction (amp^2 scale = 40), as
    test_attention_reference_exponent_moves does:

    randn1.5 / randn3   q, k = a randn: logit sigma a^2 (2.25: the regime of test_attention_fwd_bwd; 9: maxima about 45)
    offset / neg        q + amp e0, k +- amp e0: every logit about +-40, the first tile moves the reference exponent up / down
    rising              q = 0.3 q + amp e0, k = 0.3 k + 0.75 amp (j // 64) e0: the reference moves up at every tile; from three tiles
                        on the early keys' probabilities are fp32 denormals
    peaked              q = 0.3 q + amp u_i, k = 0.3 k + amp u_perm(i), u_i random unit vectors: one key at logit about 40 per query,
                        a saturated softmax (dP - delta cancels)
    spike_late          plain randn, but queries 7 and 40 are 0.3 q + amp e0 and key 150 (the last key where N <= 150) is
                        0.3 k + 3 amp e0: one wave leaves the range at a late tile while most of its lanes do not
    low_after_high      q + amp e0; keys >= 64 get - 1.5 amp e0: tiles far below an established reference, which never moves down"""
    g = torch.Generator().manual_seed(2654435 * seed + 131 * N + D + 7919 * ATTN_KINDS.index(kind))
    q, k, v, do = (torch.randn(N, D, generator=g) for _ in range(4))
    amp = (40.0 * D ** 0.5) ** 0.5
    e0 = torch.zeros(D)
    e0[0] = 1.0
    if kind.startswith("randn"):
        a = float(kind[5:])
        q, k = a * q, a * k
    elif kind == "offset":
        q, k = q + amp * e0, k + amp * e0
    elif kind == "neg":
        q, k = q + amp * e0, k - amp * e0
    elif kind == "rising":
        q = 0.3 * q + amp * e0
        k = 0.3 * k + 0.75 * amp * (torch.arange(N) // ATTN_TILE).float()[:, None] * e0
    elif kind == "peaked":
        perm = torch.randperm(N, generator=g)
        u = torch.nn.functional.normalize(torch.randn(N, D, generator=g), dim=-1)
        q, k = 0.3 * q + amp * u, 0.3 * k + amp * u[perm]
    elif kind == "spike_late":
        for i in (7, 40):
            if i < N:
                q[i] = 0.3 * q[i] + amp * e0
        j = 150 if N > 150 else N - 1
        k[j] = 0.3 * k[j] + 3.0 * amp * e0
    elif kind == "low_after_high":
        q = q + amp * e0
        k[ATTN_TILE:] = k[ATTN_TILE:] - 1.5 * amp * e0
    else:
        raise ValueError(kind)
    return bf16_round(q), bf16_round(k), bf16_round(v), bf16_round(do)


def attn_ref64(q, k, v, do):
    """fp64 attention forward and backward of one head on the operands' device (dict): S = q k^T, A = S scale, lse, P, O, delta,
    G = dP - delta, dQ, dK, dV and Sabs = |q| |k|^T."""
    q, k, v, do = (t.double() for t in (q, k, v, do))
    scale = q.shape[-1] ** -0.5
    S = q @ k.T  # noqa: N806
    A = S * scale  # noqa: N806
    lse = torch.logsumexp(A, -1)
    P = torch.exp(A - lse[:, None])  # noqa: N806
    O = P @ v  # noqa: N806, E741
    delta = (O * do).sum(-1)
    G = do @ v.T - delta[:, None]  # noqa: N806
    dSs = P * G  # noqa: N806  (dS / scale)
    return dict(S=S, A=A, lse=lse, P=P, O=O, delta=delta, G=G, dQ=scale * dSs @ k, dK=scale * dSs.T @ q, dV=P.T @ do,
                Sabs=q.abs() @ k.abs().T)


# The error model, to first order (expm1 where an exponent error is exponentiated); u = 2^-24, HB = 2^-8, FL = 2^-126, 2^-23 per
# accumulated fp32 term as in gemm_bound.  Sites of csrc/attn.hip by the name of their helper or statement.
#
# Forward (attn_fwd_kernel).  The exp2 argument of score j of query i is fma(s, c, -m) - mx (fms4 against the reference exponent,
# and fms4 again in the branch that moves it): s is an fp32 sum of D exact products (c D 2^-23 Sabs in log2 units),
# c = fl(scale log2e) (u |A| log2e), the two FMAs round a value of at most (|A| + amax) log2e + 24 (the reference m lies within
# LAZY_RANGE = 24 of a score that was there): together dt.  m itself is common to the row and cancels in P / l; in lse it is
# multiplied by ln 2 once (the lse store).  v_exp_f32 (exp2_4) is good to one ulp (2^-22 covers it), and every move of the
# reference multiplies what was accumulated by alpha = exp2(-mx), one exp2 and one product per tile: nt 2^-22.
# eta is the relative error of an fp32 probability, eta_b = eta + HB (1 + eta) that of its bf16 image (pack_acc of the
# probabilities).  O = (sum_j pb_j v_j) / l: the numerator is an fp32 sum of N exact products of erroneous pb; the denominator is
# the same sum against ones at D = 32 (SUM_MFMA, the MFMAs into ol: eta_b) and an fp32 sum of the unrounded p at D = 64 (the
# p0 .. p3 adds into lsum: eta).  1 / l and the product with it (inv, the argument of store_row) are 2^-22 |O|, the store
# (pack_bf2 in store_row) HB.
# lse = m ln2 + logf(l) (the lse store): the relative error of l, one ulp of logf and of the sum at |lse|, the product m ln2 with
# |m ln2| <= amax + 24: b_lse.  (ocml's logf is stated at 1 ulp; 4 u (|lse| + ...) has room for that, not widened.)
#
# Backward (attn_bwd_dq_kernel / attn_bwd_dkv_kernel).  Both recompute P = exp2(q' k^T - lse log2e) with ONE operand folded:
# q' = bf16(fl(q fl(c))) (scale_frag, called on the Q fragments in the dQ kernel and on the K fragments in the dK / dV kernel):
# HB + 3u relative per product, so (HB + 3u) c Sabs -- the FOLD term.  The MFMA chain starts at -fl(lse log2e) (lse2 and the initial
# s in the dQ kernel, s_lse and nl4 in the dK / dV kernel) and adds D products: (D + 2) 2^-23 of the magnitudes; the lse it is
# given is off by lse_err.  rho is the relative error of a recomputed probability.
# delta (the `part` sum of the dQ kernel) is an fp32 sum of D products of the bf16 out (off from O64 by out_err) with dO.
# dP - delta is a chain that starts at -delta and adds D products (the initial dp and the dP MFMAs): eg.  dS / scale = bf16(p g)
# (mul4 in both kernels, then pack_acc): E.  dQ, dK are fp32 sums over N of exact products, times scale (the argument of dQ's
# store_row, the written-out dK store), stored as bf16.  dV uses bf16(p) (pack_acc into pf of the dK / dV kernel): EP.
# Underflow: a probability, a product p g or a bf16 image below 2^-126 is returned as 0 by the hardware (and an fp64 reference
# keeps it): FL per element of E and EP (fl_E, fl_EP), and FL on each stored gradient / output (fl_store).
def attn_bounds(ref, q, k, v, do, lse_err=None, out_err=None, drop=()):
    """Elementwise a-priori bounds (dict: O, lse, delta, dQ, dK, dV) for ``ref = attn_ref64(q, k, v, do)``.  ``lse_err`` [N] /
    ``out_err`` [N, D]: the errors of the lse / out handed to the backward (default: an fp32-rounded lse64 and a bf16-rounded O64).
    ``drop``: names from ATTN_BOUND_TERMS to leave out (self-check only)."""
    assert set(drop) <= set(ATTN_BOUND_TERMS), drop
    N, D = q.shape  # noqa: N806
    scale = D ** -0.5
    c = scale * LOG2E
    u, HB = U_F32, HALF_ULP_BF16  # noqa: N806
    fl_e = 0.0 if "fl_E" in drop else FLUSH_F32
    fl_ep = 0.0 if "fl_EP" in drop else FLUSH_F32
    fl_st = 0.0 if "fl_store" in drop else FLUSH_F32
    fold = 0.0 if "fold" in drop else HB
    q, k, v, do = (t.double().abs() for t in (q, k, v, do))
    P, O, A, Sabs = ref["P"], ref["O"].abs(), ref["A"].abs(), ref["Sabs"]  # noqa: N806, E741
    lse = ref["lse"].abs()
    amax = A.max(-1, keepdim=True).values
    nt = (N + ATTN_TILE - 1) // ATTN_TILE
    # forward
    dt = c * D * 2.0 ** -23 * Sabs + 2.0 ** -22 * ((A + amax) * LOG2E + ATTN_RANGE)
    eta = torch.expm1(LN2 * dt) + 2.0 ** -22 + nt * 2.0 ** -22
    eta_b = eta + HB * (1 + eta)
    eta_den = eta_b if D == 32 else eta
    num = (P * eta_b) @ v + N * 2.0 ** -23 * (P @ v)
    den = (P * eta_den).sum(-1, keepdim=True) + N * 2.0 ** -23
    bO = (num + O * den) * (1 + den)  # noqa: N806
    bO = bO + HB * (O + bO) + 2.0 ** -22 * O + fl_st  # noqa: N806
    b_lse = den[:, 0] + 2.0 ** -22 + 4 * u * (lse + amax[:, 0] + ATTN_RANGE)
    # backward
    le = u * lse if lse_err is None else lse_err.double()
    dtb = (fold + 3 * u) * c * Sabs + (D + 2) * 2.0 ** -23 * (c * Sabs + lse[:, None] * LOG2E) + LOG2E * le[:, None]
    rho = torch.expm1(LN2 * dtb) + 2.0 ** -22
    OdO = (O * do).sum(-1)  # noqa: N806
    oe = HB * OdO if out_err is None else (out_err.double() * do).sum(-1)
    b_delta = oe + (D + 2) * 2.0 ** -23 * OdO
    eg = b_delta[:, None] + (D + 2) * 2.0 ** -23 * (do @ v.T + ref["delta"].abs()[:, None])
    G = ref["G"].abs()  # noqa: N806
    mag = (G + eg) * (1 + rho)
    E = P * (rho * G + (1 + rho) * eg + 2 * u * (G + eg) + HB * mag) + fl_e * (mag + 1)  # noqa: N806
    b_dq = scale * (E @ k + N * 2.0 ** -23 * ((P * mag) @ k))
    b_dq = b_dq + HB * (ref["dQ"].abs() + b_dq) + 2 * u * ref["dQ"].abs() + fl_st
    b_dk = scale * (E.T @ q + N * 2.0 ** -23 * ((P * mag).T @ q))
    b_dk = b_dk + HB * (ref["dK"].abs() + b_dk) + 2 * u * ref["dK"].abs() + fl_st
    EP = P * (rho + HB * (1 + rho)) + 2 * fl_ep  # noqa: N806
    b_dv = EP.T @ do + N * 2.0 ** -23 * (P.T @ do)
    b_dv = b_dv + HB * (ref["dV"].abs() + b_dv) + fl_st
    return dict(O=bO, lse=b_lse, delta=b_delta, dQ=b_dq, dK=b_dk, dV=b_dv)


def _fma32(a: torch.Tensor, c: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """fl32(a c - b) with one rounding (the product of two fp32 values is exact in fp64)."""
    return (a.double() * c.double() - b.double()).float()


def _flush32(x: torch.Tensor) -> torch.Tensor:
    """What the hardware returns for an fp32 denormal result of v_exp_f32, of a bf16 convert or of a matrix-core sum: zero."""
    return torch.where(x.abs() < FLUSH_F32, torch.zeros_like(x), x)


def _c32(D: int) -> torch.Tensor:  # noqa: N803
    """fl(scale log2e) as the kernels form it: an fp32 product of the fp32 scale and the fp32 constant."""
    return torch.tensor(D ** -0.5, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)


def attn_emulated_fwd(q, k, v, defect=None):
    """torch fp32 emulation of attn_fwd_kernel as written (reference exponent, LAZY_RANGE): groups of 16 queries (one ``qt`` of a wave) over
    64-key tiles, the range test per lane (16 keys of the tile) as in the kernel; returns ``out`` (bf16 values) and ``lse``.  ``defect`` = "p_trunc": the WRONG form that truncates P to bf16."""
    N, D = q.shape  # noqa: N806
    c = _c32(D)
    ng = (N + 15) // 16
    qq = torch.zeros(ng * 16, D)
    qq[:N] = q                                   # rows >= N: zero operands, as frag_global gives them
    qq = qq.view(ng, 16, D)
    m = torch.zeros(ng, 16)
    lsum = torch.zeros(ng, 16)
    o = torch.zeros(ng, 16, D)
    for it, k0 in enumerate(range(0, N, ATTN_TILE)):
        kk, vv = k[k0:k0 + ATTN_TILE], v[k0:k0 + ATTN_TILE]
        s = _fma32(qq @ kk.T, c, m[..., None])
        mx = s.max(-1).values
        first = it == 0
        # a lane holds keys 16 kt + 4 g + r (kt, r < 4) of its query and tests ITS maximum, keys >= N at -inf, before the cross-lane one
        lane = torch.full((ng, 16, ATTN_TILE), -math.inf)
        lane[..., :s.shape[-1]] = s
        lane = lane.view(ng, 16, 4, 4, 4).amax((2, 4))
        leave = (lane > ATTN_RANGE) | (lane < -ATTN_RANGE) if first else lane > ATTN_RANGE
        moved = leave.any(-1).any(-1, keepdim=True)     # the ballot: one lane out of range moves all 16 queries to their row maxima
        if not first:
            mx = mx.clamp_min(0.0)
        shift = torch.where(moved, mx, torch.zeros_like(mx))
        alpha = torch.ones_like(mx) if first else torch.where(moved, torch.exp2(-mx), torch.ones_like(mx))
        m = m + shift
        s = s - shift[..., None]
        lsum, o = lsum * alpha, o * alpha[..., None]
        p = _flush32(torch.exp2(s))
        pb = bf16_truncate(p) if defect == "p_trunc" else _flush32(bf16_round(p))
        lsum = lsum + (pb if D == 32 else p).sum(-1)
        o = o + pb @ vv
    out = bf16_round(o * (1.0 / lsum)[..., None]).view(ng * 16, D)[:N]
    lse = (m * torch.tensor(LN2, dtype=torch.float32) + torch.log(lsum)).view(-1)[:N]
    return out.contiguous(), lse.contiguous()


def attn_emulated_bwd(q, k, v, do, out, lse, fold=True, defect=None, row=0):
    """torch fp32 emulation of attn_bwd_dq_kernel + attn_bwd_dkv_kernel as written; returns ``dq, dk, dv`` (bf16 values) and the
    fp32 ``delta``.  ``fold=False`` applies scale log2(e) in fp32 instead of folding it into a bf16 operand (what the fold costs).
    WRONG forms for the self-check: ``defect`` = "delta_bf16" (delta rounded to bf16), "fold_both" (sqrt(c) folded into Q and K,
    both rounded), "row_lse" (the lse of the single query ``row`` is read 0.2 too high: its recomputed probabilities are 18 % low)."""
    D = q.shape[1]  # noqa: N806
    c = _c32(D)
    scale = torch.tensor(D ** -0.5, dtype=torch.float32)
    delta = (out * do).sum(-1)
    if defect == "delta_bf16":
        delta = bf16_round(delta)
    if defect == "row_lse":
        lse = lse.clone()
        lse[row] += 0.2
    lse2 = (lse * torch.tensor(LOG2E, dtype=torch.float32))[:, None]
    if defect == "fold_both":
        t_q = t_k = bf16_round(q * torch.sqrt(c)) @ bf16_round(k * torch.sqrt(c)).T - lse2
    elif fold:
        t_q = bf16_round(q * c) @ k.T - lse2          # dQ pass
        t_k = q @ bf16_round(k * c).T - lse2          # dK / dV pass
    else:
        t_q = t_k = _fma32(q @ k.T, c, lse2)
    g = do @ v.T - delta[:, None]
    p_q, p_k = _flush32(torch.exp2(t_q)), _flush32(torch.exp2(t_k))
    rb = lambda x: _flush32(bf16_round(x))  # noqa: E731
    dq = rb(_flush32(rb(p_q * g) @ k) * scale)
    dk = rb(_flush32(rb(p_k * g).T @ q) * scale)
    dv = rb(_flush32(rb(p_k).T @ do))
    return dq, dk, dv, delta


def rel_l2(got: torch.Tensor, want64: torch.Tensor) -> float:
    return float((got.double() - want64).norm() / want64.norm().clamp_min(1e-300))


def attn_criterion_b(got, emulated, want64, bound):
    """Criterion B: ``||got - want64|| <= B_FACTOR ||emulated - want64||``.  Returns ``(applies, got_norm, emulated_norm)``;
    ``applies`` is False where the emulation's own error is below B_FLOOR of ``||bound||`` (a saturated softmax: both errors are a
    few roundings of almost nothing, and their quotient says nothing)."""
    e_got = float((got.double() - want64).norm())
    e_emu = float((emulated.double().to(want64.device) - want64).norm())
    return e_emu >= B_FLOOR * float(bound.norm()), e_got, e_emu


# ------------------------------------------------------------------------------------------------ AdamW
# One step of csrc/optim.hip's adamw_update on fp32 p, g, m, v with fp32 scalars (the ABI takes floats):
#   g' = g gs;  p1 = p (1 - lr wd);  m' = b1 m + (1 - b1) g';  v' = b2 v + (1 - b2) g'^2
#   denom = sqrt(v') / bc2_sqrt + eps;  step = (lr / bc1) (m' / denom);  p' = p1 - step
# Error model (u = 2^-24, FL = 2^-126; correctly rounded / and sqrtf: hipcc's default, build.py passes no fast-math flag):
#   m'     two products of an fp32 g' (one rounding inside), one sum, fused or not: 4u on the magnitudes        -> dm
#   v'     g'^2 carries 2u from g', the products and the sum three more: 5u v' (all terms are non-negative)      -> dv
#   sqrt   |sqrt(a) - sqrt(b)| <= min(|a - b| / (2 sqrt b), sqrt |a - b|), and one rounding                     -> dsqrt
#   denom  the division by bc2_sqrt and the sum with eps                                                        -> ddenom
#   step   first order in dm and ddenom; lr / bc1, m' / denom and their product round once each                 -> dstep
#   p'     1 - lr wd (two roundings) and the product: 3u |p|; the final subtraction: u |p'|                     -> dp
# FL wherever an fp32 result may underflow (g'^2 at |g'| of order 1e-25 does).
ADAMW_KINDS = ("unit", "tiny", "huge", "zero", "cancel", "bigp", "p0", "under")
ADAMW_STEPS = ((1, 0.999), (2, 0.95), (1000, 0.999), (100000, 0.999))      # (step, b2)
ADAMW_HYPER = dict(lr=1e-3, b1=0.9, eps=1e-8, wd=0.05, grad_scale=1.0 / 3.0)
ADAMW_WRONG_BC = ("eps_inside_div", "no_bc1", "no_bc2")   # forms that differ from the honest one through a bias correction only
ADAMW_WRONG = ADAMW_WRONG_BC + ("eps_in_sqrt", "wd_after", "wd_l2")


def f32(x: float) -> float:
    """The fp32 value a C float argument receives."""
    return float(torch.tensor(x, dtype=torch.float32))


def adamw_inputs(kind: str, n: int, b1: float = 0.9, grad_scale: float = 1.0 / 3.0, seed: int = 0):
    """fp32 CPU ``(p, g, m, v)`` [n].  kinds: ``unit``; ``tiny`` (g gs, m of order 1e-6: sqrt(v) is of the order of eps); ``huge``
    (1e4); ``zero`` (g = m = v = 0); ``cancel`` (b1 m = -(1 - b1) g gs up to 2^-10 relative); ``bigp`` (|p| of order 1e3); ``p0``
    (p = 0: the bound on p is the bound on the step); ``under`` (|g| of order 1e-25: g^2 underflows)."""
    gen = torch.Generator().manual_seed(6700417 * seed + n + 101 * ADAMW_KINDS.index(kind))
    r = lambda: torch.randn(n, generator=gen)  # noqa: E731
    p, g, m, v = r(), r() / grad_scale, 0.3 * r(), r() ** 2 + 0.01
    if kind == "tiny":
        g, m, v = 1e-6 * g, 1e-6 * m, 1e-12 * v
    elif kind == "huge":
        g, m, v = 1e4 * g, 1e4 * m, 1e8 * v
    elif kind == "zero":
        g, m, v = torch.zeros(n), torch.zeros(n), torch.zeros(n)
    elif kind == "cancel":
        g = -(b1 * m) / ((1.0 - b1) * grad_scale) * (1.0 + 2.0 ** -10 * r())
    elif kind == "bigp":
        p = 1e3 * p
    elif kind == "p0":
        p = torch.zeros(n)
    elif kind == "under":
        g, m, v = 1e-25 * g, 1e-25 * m, torch.zeros(n)
    elif kind != "unit":
        raise ValueError(kind)
    return p.float().contiguous(), g.float().contiguous(), m.float().contiguous(), v.float().contiguous()


def adamw_step64(p, g, m, v, lr, b1, b2, eps, wd, bc1, bc2_sqrt, grad_scale):
    """fp64 arithmetic on the fp32-valued inputs and the fp32-rounded scalars; returns the dict p, m, v, step, denom, p1."""
    lr, b1, b2, eps, wd, bc1, bc2_sqrt, gs = (f32(x) for x in (lr, b1, b2, eps, wd, bc1, bc2_sqrt, grad_scale))
    p, g, m, v = (t.double() for t in (p, g, m, v))
    gg = g * gs
    p1 = p * (1.0 - lr * wd)
    m1 = b1 * m + (1.0 - b1) * gg
    v1 = b2 * v + (1.0 - b2) * gg * gg
    denom = torch.sqrt(v1) / bc2_sqrt + eps
    step = (lr / bc1) * (m1 / denom)
    return dict(p=p1 - step, m=m1, v=v1, step=step, denom=denom, p1=p1, bm=(b1 * m).abs() + ((1.0 - b1) * gg).abs(), p0=p,
                lr_bc1=lr / bc1, bc2_sqrt=bc2_sqrt)


def adamw_bounds(ref):
    """Elementwise bounds (dict: p, m, v, step) for ``ref = adamw_step64(...)``; the derivation stands above."""
    u, FL = U_F32, FLUSH_F32  # noqa: N806
    dm = 4 * u * ref["bm"] + FL
    dv = 5 * u * ref["v"] + FL
    sq = torch.sqrt(ref["v"])
    dsqrt = torch.minimum(dv / (2 * sq), torch.sqrt(dv)) + u * sq
    denom = ref["denom"]
    ddenom = dsqrt / ref["bc2_sqrt"] + 2 * u * denom
    dstep = ref["lr_bc1"] * (dm / denom + ref["m"].abs() * ddenom / denom ** 2) + 3 * u * ref["step"].abs() + FL
    dp = 3 * u * ref["p0"].abs() + dstep + u * ref["p"].abs() + FL
    return dict(p=dp, m=dm, v=dv, step=dstep)


def adamw_emulated(p, g, m, v, lr, b1, b2, eps, wd, bc1, bc2_sqrt, grad_scale, fma: bool = False, form: str = "honest"):
    """fp32 torch written as ``adamw_update`` (csrc/optim.hip) is; returns ``(p, m, v)``.  ``fma``: the moments and the final
    subtraction as the compiler may contract them (one rounding for a product and its sum).  ``form``: "honest", or one of
    ADAMW_WRONG -- eps inside the division by bc2_sqrt, eps inside the square root, a missing bc1 or bc2, weight decay applied
    after the step, weight decay on the gradient (L2)."""
    assert form == "honest" or form in ADAMW_WRONG, form
    t = lambda x: torch.tensor(x, dtype=torch.float32)  # noqa: E731
    lr, b1, b2, eps, wd, bc1, bc2_sqrt, gs = (t(x) for x in (lr, b1, b2, eps, wd, bc1, bc2_sqrt, grad_scale))
    one = t(1.0)
    p, g, m, v = p.float(), g.float() * gs, m.float(), v.float()
    if form == "wd_l2":
        g = g + wd * p
    elif form != "wd_after":
        p = p * (one - lr * wd)
    if fma:
        m = _fma32(b1.expand_as(m), m, -((one - b1) * g))
        v = _fma32((one - b2) * g, g, -(b2 * v))
    else:
        m = b1 * m + (one - b1) * g
        v = b2 * v + (one - b2) * g * g
    if form == "no_bc1":
        bc1 = one
    if form == "no_bc2":
        bc2_sqrt = one
    if form == "eps_inside_div":
        denom = (torch.sqrt(v) + eps) / bc2_sqrt
    elif form == "eps_in_sqrt":
        denom = torch.sqrt(v / (bc2_sqrt * bc2_sqrt) + eps)
    else:
        denom = torch.sqrt(v) / bc2_sqrt + eps
    q = m / denom
    p = -_fma32((lr / bc1).expand_as(q), q, p) if fma else p - (lr / bc1) * q
    if form == "wd_after":
        p = p * (one - lr * wd)
    return p, m, v


ADAMW_TRAJ_STEPS = 20


def adamw_trajectory_case(n: int = 4100, steps: int = ADAMW_TRAJ_STEPS):
    """``steps`` AdamW steps from zero moments on a fixed gradient sequence that shrinks from 1 to 1e-6 (grad_scale 1, the other
    scalars of ADAMW_HYPER, b2 = 0.999).  Returns the dict: ``p0`` [n], ``grads`` [steps, n] (fp32 CPU), ``hyper``, the fp64
    trajectory's end ``ref`` = (p, m, v), and the ends of three fp32 trajectories: ``torch`` (torch.optim.AdamW on the CPU),
    ``emulated`` and ``emulated_fma`` (``adamw_emulated``)."""
    from maestro_amd import hip
    gen = torch.Generator().manual_seed(271828)
    p0 = torch.randn(n, generator=gen)
    shape = torch.randn(n, generator=gen)
    grads = torch.stack([shape * 10.0 ** (-6.0 * t / (steps - 1)) * (1.0 + 0.25 * torch.randn(n, generator=gen)) for t in range(steps)])
    h = dict(ADAMW_HYPER, b2=0.999, grad_scale=1.0)
    bcs = [hip.adamw_bias_corrections(h["b1"], h["b2"], t + 1) for t in range(steps)]
    args = lambda t: (h["lr"], h["b1"], h["b2"], h["eps"], h["wd"], bcs[t][0], bcs[t][1], 1.0)  # noqa: E731
    z = torch.zeros(n)
    ref = (p0.double(), z.double(), z.double())
    emu, emu_fma = (p0.clone(), z.clone(), z.clone()), (p0.clone(), z.clone(), z.clone())
    for t in range(steps):
        r = adamw_step64(*ref[:1], grads[t], *ref[1:], *args(t))
        ref = (r["p"], r["m"], r["v"])
        emu = adamw_emulated(emu[0], grads[t], emu[1], emu[2], *args(t))
        emu_fma = adamw_emulated(emu_fma[0], grads[t], emu_fma[1], emu_fma[2], *args(t), fma=True)
    pt = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([pt], lr=h["lr"], betas=(h["b1"], h["b2"]), eps=h["eps"], weight_decay=h["wd"], foreach=False)
    for t in range(steps):
        pt.grad = grads[t].clone()
        opt.step()
    st = opt.state[pt]
    return dict(p0=p0, grads=grads, hyper=h, steps=steps, ref=ref, torch=(pt.detach(), st["exp_avg"], st["exp_avg_sq"]),
                emulated=emu, emulated_fma=emu_fma)


def adamw_trajectory_errors(case, got):
    """``{p, m, v: (max |got - fp64|, norm_ceiling of the two references' errors)}``."""
    out = {}
    for i, k in enumerate("pmv"):
        want = case["ref"][i]
        out[k] = (max_abs_err(got[i].cpu(), want), norm_ceiling(max_abs_err(case["torch"][i], want), max_abs_err(case["emulated"][i], want)))
    return out
