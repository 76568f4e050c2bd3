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
    """fp32 emulation of ``gelu_cdf_pdf4`` (csrc/common.hpp, MH_GELU_TERMS = 3) as written; ``c1`` is its first coefficient."""
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
