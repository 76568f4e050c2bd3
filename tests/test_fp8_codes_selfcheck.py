"""CPU self-check of tests/fp8_codes.py: the integer ``encode`` equals torch's OCP float8 casts byte for byte, the scale rule
holds its defining inequality in exact arithmetic, and each defect a fused cast site could have (truncation, ties away from
zero, a cast of the bf16-rounded value, NaN instead of saturation, a lost sign of zero, an absmax taken after the scale, the
float32 ``floor(log2(.))`` scale rule, ``m >= 1.75`` in the MX rule) changes a byte somewhere on the input sets -- so the
bit-equality assertions of tests/test_fp8_codes_gpu.py would see it."""

from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import fp8_codes as fc

FORMATS = [fc.E4M3, fc.E5M2]
_T8 = {fc.E4M3: torch.float8_e4m3fn, fc.E5M2: torch.float8_e5m2}


def _torch_cast(x_f32: np.ndarray, fmt):
    lim = fc.FMAX[fmt]
    return torch.from_numpy(np.ascontiguousarray(x_f32)).clamp(-lim, lim).to(_T8[fmt]).view(torch.uint8)


@pytest.mark.parametrize("fmt", FORMATS)
def test_boundary_set_has_what_it_promises(fmt):
    b = fc.boundary_values(fmt).numpy()
    cv = fc.code_values(fmt)
    assert 1400 <= b.size <= 2100 and np.isfinite(b).all()
    have = set(b.view(np.uint32).tolist())
    mids = ((cv[:-1].astype(np.float64) + cv[1:]) / 2).astype(np.float32)
    for v in np.concatenate([cv, mids]):
        for w in (v, np.nextafter(v, np.float32(np.inf)), np.nextafter(v, np.float32(-np.inf))):
            for sgn in (1, -1):
                assert int(np.float32(sgn * w).view(np.uint32)) in have, (v, w, sgn)
    assert {0x00000000, 0x80000000, 0x00000001, 0x80000001} <= have
    assert np.float32(2 * fc.FMAX[fmt]) in b and np.finfo(np.float32).max in b
    assert fc.bf16_finite().numel() == 65280 and bool(torch.isfinite(fc.bf16_finite().float()).all())


@pytest.mark.parametrize("fmt", FORMATS)
def test_encode_equals_torch_cpu_cast(fmt):
    b = fc.boundary_values(fmt)
    for s in fc.SCALES:
        xs = fc.scaled_f32(b, s)
        assert torch.equal(fc.quantise(b, s, fmt), _torch_cast(xs, fmt)), s
    h = fc.bf16_finite().float()
    for s in fc.SCALES:
        assert torch.equal(fc.quantise(h, s, fmt), _torch_cast(fc.scaled_f32(h, s), fmt)), s
    assert torch.equal(fc.bf16_rne(b).view(torch.int16), b.bfloat16().view(torch.int16))


@pytest.mark.parametrize("fmt", FORMATS)
def test_decode_inverts_encode_on_every_code(fmt):
    top = fc._FMT[fmt][2]
    codes = np.concatenate([np.arange(top + 1), 0x80 + np.arange(top + 1)]).astype(np.uint8)
    v = fc.decode(codes, fmt)
    assert np.isfinite(v).all() and float(np.abs(v).max()) == fc.FMAX[fmt]
    assert np.array_equal(fc.encode(v, fmt).numpy(), codes)                       # the sign of zero included
    assert np.array_equal(fc.decode(fc.encode(v, fmt), fmt).view(np.uint32), v.view(np.uint32))
    assert torch.equal(torch.from_numpy(v).to(_T8[fmt]).view(torch.uint8), torch.from_numpy(codes))


def _sweep(fmax, ks):
    """(k, amax) for amax = fmax 2^-k and its two fp32 neighbours, where fmax 2^-k is an fp32 number."""
    for k in ks:
        exact = Fraction(fmax) / Fraction(2) ** k
        with np.errstate(over="ignore", under="ignore"):
            a0 = np.float32(np.ldexp(np.float64(fmax), -k))
        if not np.isfinite(a0) or a0 == 0 or Fraction(float(a0)) != exact:
            continue
        for a in (np.nextafter(a0, np.float32(0)), a0, np.nextafter(a0, np.float32(np.inf))):
            if np.isfinite(a) and a > 0:
                yield k, a0, a


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("margin", [0, 1, 2])
def test_scale_rule_holds_its_inequality_exactly(fmt, margin):
    fmax = fc.FMAX[fmt]
    n = 0
    for k, a0, a in _sweep(fmax, range(-130, 131)):
        s = fc.scale_rule(a, fmax, margin)
        raw = fc.scale_exponent(float(a), fmax) - margin
        if a == a0:
            assert raw == k - margin
        if -100 <= raw <= 100:
            assert s == 2.0 ** raw
            lhs, bound = Fraction(float(a)) * Fraction(s), Fraction(fmax) / 2 ** margin
            assert lhs <= bound < 2 * lhs, (k, float(a), s)
            n += 1
        else:
            assert s == 2.0 ** (100 if raw > 0 else -100)
    assert n > 500
    assert fc.scale_rule(0.0, fmax, margin) == 1.0
    assert all(np.isnan(fc.scale_rule(bad, fmax, margin)) for bad in (float("inf"), float("nan")))
    assert fc.scale_rule(float(np.finfo(np.float32).max), fmax, margin) == 2.0 ** -100       # finite: the rule, clamped


# ---------------------------------------------------------------------------------------------------- teeth
def _all_inputs(fmt):
    """Every (x, s) the GPU tests cast: the boundary set and all finite bf16 values under the three scales."""
    for src in (fc.boundary_values(fmt), fc.bf16_finite().float()):
        for s in fc.SCALES:
            yield src, s


def _count(fmt, defect):
    n = 0
    for x, s in _all_inputs(fmt):
        n += int((defect(x, s) != fc.quantise(x, s, fmt)).sum())
    return n


def _clamped(x, s, fmt):
    lim = np.float32(fc.FMAX[fmt])
    return np.clip(fc.scaled_f32(x, s), -lim, lim)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("name", ["truncation", "ties away from zero", "cast of the bf16-rounded value", "NaN above max",
                                  "sign of zero dropped"])
def test_seeded_cast_defects_are_seen(fmt, name):
    defects = {
        "truncation": lambda x, s: torch.from_numpy(fc._encode(_clamped(x, s, fmt), fmt, mode="trunc")),
        "ties away from zero": lambda x, s: torch.from_numpy(fc._encode(_clamped(x, s, fmt), fmt, mode="away")),
        "cast of the bf16-rounded value": lambda x, s: fc.quantise(fc.bf16_rne(x).float(), s, fmt),
        "NaN above max": lambda x, s: torch.from_numpy(fc._encode(fc.scaled_f32(x, s), fmt, saturate=False)),
        "sign of zero dropped": lambda x, s: torch.from_numpy(fc._encode(_clamped(x, s, fmt), fmt, zero_sign=False)),
    }
    n = _count(fmt, defects[name])
    print(f"[fp8 codes] {name}, format {fmt}: {n} bytes differ from the reference")
    assert n > 0


@pytest.mark.parametrize("fmt", FORMATS)
def test_absmax_after_the_scale_is_seen(fmt):
    b = fc.boundary_values(fmt)
    n = sum(fc.absmax_bits(fc.scaled_f32(b, s)) != fc.absmax_bits(b) for s in fc.SCALES)
    print(f"[fp8 codes] absmax after the scale, format {fmt}: {n} of {len(fc.SCALES)} scales give other bits")
    assert n > 0 and fc.absmax_bits(b) == int(np.finfo(np.float32).max.view(np.uint32))


def test_float32_log2_scale_rule_is_seen():
    n = total = 0
    for fmt in FORMATS:
        fmax = fc.FMAX[fmt]
        for k, a0, a in _sweep(fmax, range(-100, 101)):
            if a > a0:                                               # one ulp above fmax 2^-k
                total += 1
                n += fc.scale_rule_log2f(a, fmax, 0) != fc.scale_rule(float(a), fmax, 0)
    print(f"[fp8 codes] float32 floor(log2(fmax / amax)): {n} of {total} amax values one ulp above fmax 2^-k give another scale")
    assert total == 402 and n > 0


def test_mx_rule_with_a_weak_comparison_is_seen():
    blocks = fc.mx_edge_blocks()
    assert 1200 <= blocks.shape[0] <= 1400
    _, want, finite = fc.mx_ref(blocks)
    assert bool(finite.all()) and int(want.min()) == 0 and int(want.max()) == 247 and int(want[-1, 0]) == 127
    amax = blocks.double().abs().amax(-1, keepdim=True)
    m, E = torch.frexp(amax)   # noqa: N806
    e = torch.where(m < 0.875, E - 9, E - 8)                         # the defect: m >= 1.75 switches
    byte = torch.where(amax == 0, torch.full_like(e, 127), (127 + e).clamp(0, 254)).to(torch.uint8)
    n = int((byte != want).sum())
    print(f"[fp8 codes] MX rule with m >= 1.75: {n} of {blocks.shape[0]} scale bytes differ")
    assert n > 0
    # the blocks are what they claim: the anchor is the largest magnitude, both signs occur, ties and code values among the elements
    q, s, _ = fc.mx_ref(blocks)
    back = fc.mx_dequant(q, s)
    assert bool((blocks[:, 0] < 0).any()) and bool((blocks[:, 0] > 0).any()) and bool((blocks[:, 1:] < 0).any())
    assert 0.2 < float((back == blocks.double()).double().mean()) < 0.9        # code values decode to themselves, ties and neighbours do not
