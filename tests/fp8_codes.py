"""Exact references and input sets for the places where an fp32 value becomes an fp8 byte.

The fp8 step has seven such places (the two stand-alone quantisers, the LayerNorm's e4m3 / MX copy, the GEMM's e4m3 / e5m2 / MX
output copy, the fused AdamW's shadow) and one scale rule.  A test can hold a fused site to bit equality only if it knows the
fp32 value that entered the cast; the GPU tests arrange that (``gamma = 0`` makes a LayerNorm output its ``beta``, zero operands
make a GEMM output its ``bias``, a zero gradient leaves AdamW's parameter alone), and take the values from the sets below: every
code value, every tie between two codes, and the fp32 neighbours of both -- the inputs on which truncation, ties away from zero,
a cast of the bf16-rounded value or a wrong saturation edge change a byte.

``encode`` is written in integer arithmetic on the fp32 bits and calls no float8 cast of torch; tests/test_fp8_codes_selfcheck.py
holds it against torch's CPU cast, and shows that each of those defects is seen on these sets.  tests/test_fp8_codes_gpu.py uses
it on the device kernels.  No fixtures here; numpy and torch only.
"""

from __future__ import annotations

import math
from fractions import Fraction

import numpy as np
import torch

E4M3, E5M2 = 0, 1                               # MH_FP8_E4M3, MH_FP8_E5M2
FMAX = {E4M3: 448.0, E5M2: 57344.0}
# format -> (mantissa bits, exponent bias, largest finite code)
_FMT = {E4M3: (3, 7, 0x7E), E5M2: (2, 15, 0x7B)}
SCALES = (2.0 ** -7, 1.0, 2.0 ** 4)             # per-tensor scales of the tests: powers of two, so x * s is exact unless it under/overflows


def _f32(x) -> np.ndarray:
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().float().numpy()
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32))


def _encode(x, fmt: int, mode: str = "rne", saturate: bool = True, zero_sign: bool = True) -> np.ndarray:
    """fp32 -> OCP fp8 code, integer arithmetic on the bits.  ``mode``: "rne" (the contract), "trunc" and "away" (ties away from
    zero) are the seeded defects of the selfcheck, as are ``saturate=False`` (NaN above max) and ``zero_sign=False``."""
    mant, bias, top = _FMT[fmt]
    u = _f32(x).reshape(-1).view(np.uint32).astype(np.int64)
    sign, mag = (u >> 31) & 1, u & 0x7FFFFFFF
    e = np.maximum(mag >> 23, 1)                                     # biased fp32 exponent (a subnormal counts as exponent 1)
    sig = (mag & 0x7FFFFF) | np.where((mag >> 23) > 0, 1 << 23, 0)   # |x| = sig * 2^(e - 150)
    emin = 1 - bias
    t = np.maximum(e - 127, emin)                                    # exponent of the fp8 binade (emin for the subnormals)
    shift = np.minimum((t - mant) - (e - 150), 40)                   # |x| = (sig / 2^shift) * 2^(t - mant); shift >= 23 - mant
    k, rem, half = sig >> shift, sig & ((1 << shift) - 1), 1 << (shift - 1)
    if mode == "rne":
        k = k + ((rem > half) | ((rem == half) & ((k & 1) == 1)))
    elif mode == "away":
        k = k + (rem >= half)
    elif mode != "trunc":
        raise ValueError(mode)
    code = ((t - emin) << mant) + k                                  # k == 2^(mant + 1) carries into the next binade by itself
    nan_code = 0x7F
    over = code > top
    code = np.where(over, top if saturate else nan_code, code)
    code = np.where(mag > 0x7F800000, nan_code, code)                # NaN in, NaN out (not part of the sets)
    if not zero_sign:
        sign = np.where(code == 0, 0, sign)
    return (code | (sign << 7)).astype(np.uint8)


def encode(x, fmt: int) -> torch.Tensor:
    """OCP e4m3fn / e5m2 code of every fp32 element: round to nearest even, saturating at +-448 / +-57344, the sign of zero
    kept.  Accepts a tensor or an array; returns a uint8 tensor of the same shape (on the CPU)."""
    shape = tuple(x.shape) if hasattr(x, "shape") else np.shape(x)
    return torch.from_numpy(_encode(x, fmt)).reshape(shape)


def decode(code, fmt: int) -> np.ndarray:
    """fp8 code -> its value as fp32 (exact; NaN / inf codes of e5m2 and the NaN code of e4m3 decode to NaN / inf)."""
    mant, bias, _ = _FMT[fmt]
    c = np.asarray(code.cpu().numpy() if isinstance(code, torch.Tensor) else code).astype(np.int64)
    sign, ex, m = (c >> 7) & 1, (c >> mant) & ((1 << (7 - mant)) - 1), c & ((1 << mant) - 1)
    v = np.where(ex == 0, np.ldexp(m.astype(np.float64), 1 - bias - mant), np.ldexp((m + (1 << mant)).astype(np.float64), ex - bias - mant))
    if fmt == E4M3:
        v = np.where((c & 0x7F) == 0x7F, np.nan, v)
    else:
        v = np.where((c & 0x7F) == 0x7C, np.inf, np.where((c & 0x7F) > 0x7C, np.nan, v))
    return (np.where(sign == 1, -v, v)).astype(np.float32)


def code_values(fmt: int) -> np.ndarray:
    """The non-negative finite code values in increasing order (fp32): 127 for e4m3, 124 for e5m2."""
    return decode(np.arange(_FMT[fmt][2] + 1), fmt)


def boundary_values(fmt: int) -> torch.Tensor:
    """The fp32 inputs on which a cast can go wrong, both signs, sorted by bit pattern: every finite code value, every midpoint
    between neighbouring codes (the one between 0 and the smallest subnormal and the one between the two largest codes
    included), each with its fp32 predecessor and successor, the saturation edge (max, its successor, max + half a step,
    2 max, a value near fp32's largest), +-0 and a few fp32 subnormals."""
    cv = code_values(fmt).astype(np.float64)
    mids = (cv[:-1] + cv[1:]) / 2                                    # exact: one more significant bit than the codes
    core = np.concatenate([cv, mids]).astype(np.float32)
    assert np.array_equal(core.astype(np.float64), np.concatenate([cv, mids]))
    inf = np.float32(np.inf)
    pts = [core, np.nextafter(core, inf), np.nextafter(core, -inf)]
    fmax = np.float32(FMAX[fmt])
    step = float(cv[-1] - cv[-2])
    pts.append(np.array([fmax, np.nextafter(fmax, inf), float(fmax) + step / 2, np.nextafter(np.float32(float(fmax) + step / 2), -inf),
                         np.nextafter(np.float32(float(fmax) + step / 2), inf), 2 * float(fmax), 3.0e38, np.finfo(np.float32).max], dtype=np.float32))
    sub = np.array([1, 2, 3, 1 << 22, (1 << 23) - 1], dtype=np.uint32).view(np.float32)      # fp32 subnormals
    pts.append(sub)
    pos = np.concatenate(pts)
    pos = pos[pos >= 0]                                              # (the predecessor of +0 comes back with the negatives)
    bits = np.unique(np.concatenate([pos, -pos, np.array([0.0, -0.0], dtype=np.float32)]).view(np.uint32))
    return torch.from_numpy(bits.view(np.float32).copy())


def bf16_finite() -> torch.Tensor:
    """All 65 280 finite bf16 bit patterns (both zeros and the subnormals included) as a bf16 tensor."""
    u = np.arange(1 << 16, dtype=np.int64)
    u = u[((u >> 7) & 0xFF) != 0xFF]
    return torch.from_numpy(u.astype(np.uint16).view(np.int16).copy()).view(torch.bfloat16)


def scaled_f32(x, s: float) -> np.ndarray:
    """``float32(x) * float32(s)`` in IEEE fp32 (numpy keeps denormals), clamped to nothing yet."""
    with np.errstate(over="ignore", under="ignore"):
        return _f32(x) * np.float32(s)


def quantise(x, s: float, fmt: int) -> torch.Tensor:
    """The per-tensor contract: ``encode(clamp(float32(x) * float32(s), -max, max))``."""
    lim = np.float32(FMAX[fmt])
    shape = tuple(x.shape)
    return encode(np.clip(scaled_f32(x, s), -lim, lim), fmt).reshape(shape)


def absmax_bits(x) -> int:
    """Bits of ``max |x|`` over all elements, in the order the kernels keep (unsigned order of the |x| bits)."""
    return int((_f32(x).reshape(-1).view(np.uint32) & 0x7FFFFFFF).max())


def bf16_rne(x) -> torch.Tensor:
    """Round-to-nearest-even bf16 of fp32 values, on the bits (finite inputs), as a bf16 tensor of the same shape."""
    a = _f32(x)
    u = a.reshape(-1).view(np.uint32).astype(np.int64)
    r = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    return torch.from_numpy(r.astype(np.uint16).view(np.int16).copy()).view(torch.bfloat16).reshape(a.shape)


# ---------------------------------------------------------------------------------------------------- the per-tensor scale rule
def scale_exponent(amax: float, fmax: float) -> int:
    """The largest integer e with ``amax * 2^e <= fmax``, i.e. floor(log2(fmax / amax)), in exact rational arithmetic."""
    r = Fraction(fmax) / Fraction(amax)
    e = r.numerator.bit_length() - r.denominator.bit_length()
    return e if Fraction(2) ** e <= r else e - 1


def scale_rule(amax_f32: float, fmax: float, margin: int) -> float:
    """``mh_fp8_update_scales`` as include/maestro_hip.h states it: ``2^(floor(log2(fmax / amax)) - margin)`` with the exponent
    clamped to [-100, 100]; 1 for amax == 0; NaN for a non-finite amax."""
    a = float(amax_f32)
    if a == 0.0:
        return 1.0
    if not math.isfinite(a):
        return float("nan")
    return 2.0 ** max(-100, min(100, scale_exponent(a, fmax) - margin))


def scale_rule_log2f(amax_f32, fmax: float, margin: int) -> float:
    """The float32 evaluation ``floorf(log2f(fmax / a))`` with a correctly rounded quotient and logarithm (the seeded defect of
    the selfcheck): an amax one ulp above ``fmax 2^-k`` gives a quotient just below ``2^k`` whose log2 rounds up to k."""
    a = np.float32(amax_f32)
    if a == 0:
        return 1.0
    if not np.isfinite(a):
        return float("nan")
    with np.errstate(over="ignore"):
        q = np.float32(fmax) / a
    if not np.isfinite(q):
        return 2.0 ** 100
    e = int(np.floor(np.float32(np.log2(np.float64(q))))) - margin
    return 2.0 ** max(-100, min(100, e))


# ---------------------------------------------------------------------------------------------------- MX block scaling
def mx_ref(x: torch.Tensor):
    """The MX rule in exact float64 arithmetic: bf16 [rows, cols] -> (e4m3 bytes [rows, cols], E8M0 bytes [rows, cols / 32],
    finite-block mask [rows, cols / 32])."""
    rows, cols = x.shape
    v = x.cpu().double().view(rows, cols // 32, 32)
    amax = v.abs().amax(-1)
    finite = torch.isfinite(v).all(-1)
    m, E = torch.frexp(torch.where(finite, amax, torch.ones_like(amax)))   # amax = m 2^E, m in [0.5, 1)  # noqa: N806
    e = torch.where(m <= 0.875, E - 9, E - 8)                               # smallest e with amax <= 448 2^e = 0.875 2^(e + 9)
    byte = torch.where(amax == 0, torch.full_like(e, 127), (127 + e).clamp(0, 254))
    byte = torch.where(finite, byte, torch.full_like(byte, 255))
    scaled = torch.ldexp(v, (127 - byte.clamp(max=254)).double()[..., None].expand_as(v))
    q = encode(scaled.float(), E4M3).view(rows, cols)
    return q, byte.to(torch.uint8), finite


def mx_dequant(q: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    rows, cols = q.shape
    v = torch.from_numpy(decode(q.cpu(), E4M3)).double().view(rows, cols // 32, 32)
    return torch.ldexp(v, (s.cpu().long() - 127).double()[..., None].expand_as(v)).view(rows, cols)


MX_ANCHOR_MANTISSAS = (1.0, 1.75 - 2.0 ** -7, 1.75, 1.75 + 2.0 ** -7, 2.0 - 2.0 ** -7)   # around the m > 1.75 switch (448 = 1.75 * 2^8)


def _mx_pool() -> np.ndarray:
    """Element candidates in the scaled domain (|v| <= 448, float64): e4m3 code values, ties, and a tie +- one bf16 ulp; both
    signs (no -0: a LayerNorm's ``0 * x + beta`` would not keep it)."""
    cv = code_values(E4M3).astype(np.float64)
    ties = (cv[:-1] + cv[1:]) / 2
    ulp = np.ldexp(1.0, np.floor(np.log2(ties)).astype(np.int64) - 7)
    mag = np.concatenate([cv[1:], ties, ties - ulp, ties + ulp])
    pool = np.empty(2 * mag.size)
    pool[0::2], pool[1::2] = mag, -mag
    return np.concatenate([[0.0], pool])


def mx_edge_blocks() -> torch.Tensor:
    """bf16 [blocks, 32]: one block per anchor.  Element 0 is the block's largest magnitude ``m 2^E``, m around the ``m > 1.75``
    switch of the rule and E every bf16 exponent -126 .. 127 (scale bytes 0 .. 247), then a few bf16-subnormal anchors (byte 0)
    and the all-zero block (byte 127).  The other 31 elements walk through e4m3 code values, ties and their bf16 neighbours
    scaled by the block's 2^e, kept where bf16 holds them exactly and they do not exceed the anchor, zero elsewhere."""
    pool = _mx_pool()
    anchors = [m * 2.0 ** E for E in range(-126, 128) for m in MX_ANCHOR_MANTISSAS]   # noqa: N806
    anchors += [2.0 ** -133, 3 * 2.0 ** -133, 2.0 ** -127, 127 * 2.0 ** -133, 0.0]
    out = np.zeros((len(anchors), 32))
    for b, a in enumerate(anchors):
        if a == 0.0:
            continue
        out[b, 0] = -a if b % 2 else a
        m, E = math.frexp(a)   # noqa: N806
        e = max((E - 9 if m <= 0.875 else E - 8), -127)
        v = np.ldexp(pool[(31 * b + np.arange(31)) % pool.size], e)
        for _ in range(20):                    # (once, but for the byte-0 blocks, whose scaled anchor lies below 224)
            v = np.where(np.abs(v) > a, v / 2, v)
        out[b, 1:] = v
    t = torch.from_numpy(out)
    tb = t.bfloat16()
    exact = tb.double() == t
    tb = torch.where(exact, tb, torch.zeros_like(tb))
    assert bool((tb[:, 1:].double().abs().amax(-1) <= tb[:, 0].double().abs()).all())
    return tb
