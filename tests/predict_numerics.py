"""Operands, fp64 references, a-priori error bounds and fp32 emulations for the prediction kernels (csrc/predict.hip).

Used by tests/test_predict_selfcheck.py (CPU: fp64 and the honest fp32 emulation lie inside the bound, every named wrong form is
rejected by a case the GPU file also runs) and tests/test_predict_gpu.py (the HIP kernels on the same cases).

Softmax (predict_view_kernel), per pixel with logits l_c, m = max_c l_c, x_c = l_c - m <= 0, all in fp32, u = 2^-24:

* m is one of the logits: exact.
* e_c = __expf(fl(l_c - m)).  ``__expf`` is the device's native exponential, v_exp_f32 of the fp32 product with fl(log2 e) -- the
  function csrc/heads.hip uses, modelled by ``heads_numerics.exp_rel``: the subtraction (u |x|), the product with log2 e and that
  constant's rounding (2 u |x|: a relative error of the exponent is an absolute one of the result's logarithm) and v_exp_f32
  itself at 1 ulp = 2^-23 relative, taken as 2^-22 (``heads_numerics.EXP_ULP``, the figure of tests/numerics.py; the 1 ulp is
  the accuracy the CDNA instruction-set reference states for V_EXP_F32).  r_c = 3 u |x_c| + 2^-22.  A result below
  FL = 2^-126 is flushed: FL absolute.
* s = sum_c e_c, C additions in any order: C 2^-23 relative (all terms are positive; ``gemm_bound``'s constant per term).  The
  errors of the e_c enter s with their weights: rbar = sum_c exp(x_c) r_c / sum_c exp(x_c), plus C FL (s >= 1).
* inv = fl(1 / s), a correctly rounded division: u.  conf = inv.
* p_c = fl(e_c inv): u.

  |conf - conf*| <= conf* (rbar + C 2^-23 + u) (1 + 2^-10) + FL
  |p_c - p_c*|   <= p_c*  (r_c + rbar + C 2^-23 + 2 u) (1 + 2^-10) + 2 FL

  (1 + 2^-10) covers the second-order products: every first-order sum here is below 2^-10.)

Sigmoid (predict_sigmoid_kernel): e = __expf(-l) (the negation is exact: r = 2 u |l| + 2^-22 <= exp_rel), d = fl(1 + e) (u),
sigma = fl(1 / d) (u); d sigma / d e = -sigma^2, so |sigma - sigma*| <= sigma* ((1 - sigma*) r + 2 u) (1 + 2^-10) + FL.  Below
l = -88.7 e overflows and sigma = 0 where sigma* < FL; above l = 87.3 e flushes and sigma = 1 where 1 - sigma* < u.

Nothing here is fitted to what the kernels give; the observed ratio is recorded through conftest's ``observed`` (profiles/predict.md quotes it).
"""

from __future__ import annotations

import numpy as np
import torch

from maestro_amd import hip
from tests.heads_numerics import ACC, FL, U, exp_rel, expf32
from tests.numerics import bf16_round

SECOND_ORDER = 1.0 + 2.0 ** -10

# (kind, B, g, P, C): the cases of the softmax value test; the GPU file and the self-check run the same list
SOFTMAX_KINDS = ("sigma2", "pm60", "dominant", "equal")
SOFTMAX_SHAPES = ((2, 3, 2, 6), (3, 1, 1, 19), (1, 2, 4, 128), (2, 5, 1, 2))
SOFTMAX_WRONG = ("no_max", "class_stride", "bf16")
SIGMOID_SHAPES = ((5, 18), (300, 15), (7, 1))


def softmax_logits(kind: str, B: int, g: int, P: int, C: int, seed: int = 0) -> torch.Tensor:  # noqa: N803
    """fp32 ``[B * g * g, P * P * C]`` (patch layout).  "sigma2": N(0, 2^2).  "pm60": every logit at +60 or -60 (a fair coin) plus
    the sigma-2 noise, so that no two classes share their roundings.  "dominant": sigma 2 with one class per pixel raised by 30.
    "equal": one value per pixel on all its classes."""
    gen = torch.Generator().manual_seed(7919 * seed + 131 * B + 17 * g + 5 * P + C + 1009 * SOFTMAX_KINDS.index(kind))
    n = B * g * g * P * P
    x = 2.0 * torch.randn(n, C, generator=gen)
    if kind == "pm60":
        x = x + 60.0 * (2.0 * torch.randint(0, 2, (n, C), generator=gen) - 1.0)
    elif kind == "dominant":
        x[torch.arange(n), torch.randint(0, C, (n,), generator=gen)] += 30.0
    elif kind == "equal":
        x = x[:, :1].expand(n, C).clone()
    elif kind != "sigma2":
        raise ValueError(kind)
    return x.float().reshape(B * g * g, P * P * C).contiguous()


def softmax_ref64(logits: torch.Tensor, g: int, P: int, C: int, flags=None):  # noqa: N803
    """``(p [B, C, S, S], conf [B, S, S])`` in fp64 from the fp32 logits (``hip.predict_reference``)."""
    p, _, conf = hip.predict_reference(logits.numpy(), flags, hip.PREDICT_SOFTMAX, g=g, P=P, C=C, dtype=np.float64)
    return torch.from_numpy(p), torch.from_numpy(conf)


def softmax_bounds(logits: torch.Tensor, g: int, P: int, C: int, flags=None):  # noqa: N803
    """``(b_p [B, C, S, S], b_conf [B, S, S])``: the module docstring's bounds, per element, in fp64."""
    B = logits.shape[0] // (g * g)  # noqa: N806
    # the logits themselves in raster layout: predict_reference's walk applied to them (probabilities are not needed here)
    S = g * P  # noqa: N806
    x = logits.double().reshape(B, g, g, P, P, C).permute(0, 5, 1, 3, 2, 4).reshape(B, C, S, S)
    if flags is not None:
        moved = torch.empty_like(x)
        for b in range(B):
            y0, x0 = hip.predict_pixel_map(int(flags[b]), S)
            moved[b][:, torch.from_numpy(y0), torch.from_numpy(x0)] = x[b]
        x = moved
    x = x - x.max(dim=1, keepdim=True).values
    r = exp_rel(x)
    w = torch.exp(x)
    rbar = (w * r).sum(dim=1) / w.sum(dim=1)
    p, conf = softmax_ref64(logits, g, P, C, flags)
    b_conf = conf * (rbar + C * ACC + U) * SECOND_ORDER + FL
    b_p = p * (r + rbar[:, None] + C * ACC + 2 * U) * SECOND_ORDER + 2 * FL
    return b_p, b_conf


def softmax_emulated(logits: torch.Tensor, g: int, P: int, C: int, form: str | None = None):  # noqa: N803
    """``(p, conf)`` in torch fp32 written as the kernel is, or one of the wrong forms of ``SOFTMAX_WRONG``: "no_max" (no
    subtraction of the maximum), "class_stride" (class c of pixel q read at column c * P * P + q instead of q * C + c), "bf16" (p
    rounded to bf16); ``form="fp64"`` is the fp64 reference itself."""
    if form == "fp64":
        return softmax_ref64(logits, g, P, C)
    B, S = logits.shape[0] // (g * g), g * P  # noqa: N806
    x = logits.reshape(B, g, g, P * P, C)
    if form == "class_stride":
        x = logits.reshape(B, g, g, C, P * P).transpose(3, 4)
    x = x.reshape(B, g, g, P, P, C).permute(0, 5, 1, 3, 2, 4).reshape(B, C, S, S).contiguous()
    m = torch.zeros_like(x[:, :1]) if form == "no_max" else x.max(dim=1, keepdim=True).values
    e = expf32(x - m)
    s = torch.zeros_like(e[:, 0])
    for c in range(C):                     # the kernel's order; the bound holds for any
        s = s + e[:, c]
    inv = 1.0 / s
    p = e * inv[:, None]
    conf = e.max(dim=1).values * inv if form == "no_max" else inv
    if form == "bf16":
        p = bf16_round(p)
    return p, conf


def softmax_ratios(logits: torch.Tensor, g: int, P: int, C: int, p: torch.Tensor, conf: torch.Tensor, flags=None) -> dict:  # noqa: N803
    """``{"p": max |p - p*| / bound, "conf": ...}``; a non-finite value counts as infinite."""
    p64, c64 = softmax_ref64(logits, g, P, C, flags)
    b_p, b_conf = softmax_bounds(logits, g, P, C, flags)

    def ratio(got, want, bound):
        got = got.double().cpu().reshape(want.shape)
        if not bool(torch.isfinite(got).all()):
            return float("inf")
        return float(((got - want).abs() / bound).max())
    return {"p": ratio(p, p64, b_p), "conf": ratio(conf, c64, b_conf)}


def sigmoid_logits(B: int, C: int, seed: int = 0) -> torch.Tensor:  # noqa: N803
    """fp32 ``[B, C]``: N(0, 3^2), with the first row stepping through -100 ... 100 (both saturated ends)."""
    gen = torch.Generator().manual_seed(104729 * seed + 31 * B + C)
    x = 3.0 * torch.randn(B, C, generator=gen)
    x[0] = torch.linspace(-100.0, 100.0, C) if C > 1 else torch.tensor([0.25])
    return x.float().contiguous()


def sigmoid_ratio(logits: torch.Tensor, got: torch.Tensor) -> float:
    x = logits.double()
    want = 1.0 / (1.0 + torch.exp(-x))
    bound = want * ((1.0 - want) * exp_rel(x) + 2 * U) * SECOND_ORDER + FL
    got = got.double().cpu().reshape(want.shape)
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    return float(((got - want).abs() / bound).max())


def sigmoid_emulated(logits: torch.Tensor) -> torch.Tensor:
    return 1.0 / (1.0 + expf32(-logits))
