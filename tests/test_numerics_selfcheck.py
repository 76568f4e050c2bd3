"""The error bounds of tests/numerics.py have teeth (CPU only): each bound accepts honest fp32 implementations of the operation and
rejects an emulation of the subtly wrong kernel it exists to catch.  tests/test_numerics_gpu.py applies the same functions to the
HIP kernels."""

import pytest
import torch

from tests import numerics as nm

M = N = 96
KS = (64, 768, 3072, 16384)


def _case(dist, K):  # noqa: N803
    a, b = nm.gemm_operands(dist, M, N, K)
    c64, absprod = nm.gemm_ref64(a, b)
    return a, b, c64, absprod


def _ratio(c, c64, bound):
    return nm.worst_ratio((c.double() - c64).abs(), bound)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("dist", nm.DISTRIBUTIONS)
def test_fp32_accumulation_is_accepted(dist, K):  # noqa: N803
    a, b, c64, absprod = _case(dist, K)
    bound = nm.gemm_bound(absprod, K)
    impls = {"torch": a @ b, "chunk16": nm.matmul_chunked(a, b, 16), "chunk32": nm.matmul_chunked(a, b, 32)}
    if K <= 3072 or dist == "offset":
        impls["rtz"] = nm.matmul_chunked(a, b, 16, mode="rtz")
    for name, c in impls.items():
        r = _ratio(c, c64, bound)
        assert r <= 0.25, (name, dist, K, r)       # honest accumulators sit far inside the bound (measured <= 0.08)


@pytest.mark.parametrize("K", [768, 3072, 16384])
def test_bf16_partials_are_rejected(K):  # noqa: N803
    """Partials rounded to bf16 every 8 chunks: far outside on same-sign terms; on `randn` the error hides in the bound's slack
    (the reason `offset` is a mandatory distribution)."""
    a, b, c64, absprod = _case("offset", K)
    r = _ratio(nm.matmul_chunked(a, b, 16, bf16_every=8), c64, nm.gemm_bound(absprod, K))
    assert r > 5.0, (K, r)


def test_bf16_store_rounding_mode():
    a, b, c64, absprod = _case("randn", 768)
    c32 = a @ b
    bound = nm.bf16_store_bound(c64, absprod, 768)
    assert _ratio(nm.bf16_round(c32), c64, bound) <= 1.0
    trunc = nm.bf16_truncate(c32)
    assert _ratio(trunc, c64, bound) > 1.5
    # the tolerance-free form of the same check: the truncated store differs from round-to-nearest-even in about half the elements
    assert 0.3 < float((trunc != nm.bf16_round(c32)).float().mean()) < 0.7


def test_bias_after_bf16_rounding_is_rejected():
    a, b, c64, absprod = _case("randn", 768)
    g = torch.Generator().manual_seed(3)
    bias, res = torch.randn(N, generator=g), torch.randn(M, N, generator=g)
    c32 = a @ b
    want = c64 + bias.double() + res.double()
    bound = nm.bias_residual_bound(c64, absprod, 768, bias.double()[None].expand(M, N), res.double())
    assert _ratio((c32 + bias) + res, want, bound) <= 1.0
    assert _ratio(c32 + (bias + res), want, bound) <= 1.0
    assert _ratio((nm.bf16_round(c32) + bias) + res, want, bound) > 1.0
    # and the saved pre-activation: bf16(acc + bias) is not bf16(bf16(acc) + bias)
    assert not torch.equal(nm.bf16_round(c32 + bias), nm.bf16_round(nm.bf16_round(c32) + bias))


def _grid_x():
    a, bias = nm.gelu_grid()
    return (a[:, None] + bias[None, :]).reshape(-1)      # one fp32 addition per element, as in the epilogue


def test_gelu_three_term_form_is_accepted_and_a_wrong_constant_rejected():
    x = _grid_x()
    x64 = x.double()
    cdf, pdf = nm.gelu_cdf_pdf4_emulated(x)
    y = nm.bf16_round(x * cdf)
    d = x * pdf + cdf
    assert nm.worst_ratio((y.double() - nm.gelu64(x64)).abs(), nm.gelu_bound(x64)) <= 1.0
    assert nm.worst_ratio((nm.bf16_round(d).double() - nm.dgelu64(x64)).abs(), nm.dgelu_bound(x64)) <= 1.0
    raw = float(((x * cdf).double() - nm.gelu64(x64)).abs().div(x64.abs().clamp_min(1e-30)).max())
    assert raw <= nm.GELU_CDF_ERR, raw                    # the fp32 form itself: measured 1.094e-5 |x| at x ~ 2.39
    cdf_w, pdf_w = nm.gelu_cdf_pdf4_emulated(x, c1=0.7478556 + 1e-3)
    assert nm.worst_ratio((nm.bf16_round(x * cdf_w).double() - nm.gelu64(x64)).abs(), nm.gelu_bound(x64)) > 1.0
    assert nm.worst_ratio((nm.bf16_round(x * pdf_w + cdf_w).double() - nm.dgelu64(x64)).abs(), nm.dgelu_bound(x64)) > 1.0


def test_byte_code_range_and_wrap():
    x = _grid_x()
    x64 = x.double()
    cdf, pdf = nm.gelu_cdf_pdf4_emulated(x)
    d = x * pdf + cdf
    raw = torch.round(d * 200.0 + 26.0)
    assert 0 <= float(raw.min()) and float(raw.max()) <= 255, (float(raw.min()), float(raw.max()))   # 0 ... 252: nothing to saturate
    code = nm.encode_u8_emulated(d)
    assert nm.worst_ratio((nm.decode_u8(code) - nm.dgelu64(x64)).abs(), nm.dgelu_bound(x64, u8=True)) <= 1.0
    # a derivative just past the coded range (an implementation whose GELU' overshoots): saturation stays within the bound's
    # neighbourhood, a wrap at 256 lands a whole range away
    over = torch.tensor([1.15, -0.135])
    assert (nm.decode_u8(nm.encode_u8_emulated(over)) - over.double()).abs().max() < 0.01
    wrapped = nm.decode_u8(nm.encode_u8_emulated(over, wrap=True))
    assert (wrapped - over.double()).abs().min() > 1.0
    x_over = torch.tensor([1.0e4, -1.0e4]).double()       # decoded +-1e4 must be 1 and 0 within half a step
    assert nm.worst_ratio((wrapped - nm.dgelu64(x_over)).abs(), nm.dgelu_bound(x_over, u8=True)) > 1.0


@pytest.mark.parametrize("kind", ["mu0", "mu10", "mu100", "mu1000", "outlier", "small", "large"])
def test_two_pass_variance_is_accepted_one_pass_rejected(kind):
    x = nm.norm_inputs(kind, 64, 768)
    eps = 1e-5
    m64, v64, r64 = nm.stats64(x, eps)
    mw, vw, rw = nm.wave_two_pass_stats(x, eps)
    _, mt, rt = torch.native_layer_norm(x, (768,), None, None, eps)
    ceil_r = nm.norm_ceiling(nm.max_rel_err(rw, r64), nm.max_rel_err(rt.reshape(-1), r64))
    assert ceil_r < (2e-6 if kind != "mu1000" else 1e-4), ceil_r   # (torch's own op loses some digits at 1000 sigma, the two-pass form none)
    # each reference sits under the ceiling the other one sets (the 2x margin is not vacuous)
    assert nm.max_rel_err(rw, r64) <= ceil_r and nm.max_rel_err(rt.reshape(-1), r64) <= ceil_r
    _, _, r1 = nm.one_pass_stats(x, eps)
    if kind in ("mu100", "mu1000"):
        assert nm.max_rel_err(r1, r64) > 10 * ceil_r, (nm.max_rel_err(r1, r64), ceil_r)


def test_constant_rows_have_zero_variance_in_any_order():
    x = nm.norm_inputs("const", 12, 768)
    m, v, _ = nm.wave_two_pass_stats(x, 1e-5)
    assert torch.equal(m, x[:, 0]) and float(v.abs().max()) == 0.0
