"""CPU self-check of tests/heads_numerics.py, the helpers behind tests/test_heads_numerics_gpu.py.  No GPU, no HIP library.

On the very case lists the GPU file runs: the honest fp32 emulation of every head kernel lies inside every bound and equals
every exact expectation bit for bit; every named wrong form is rejected by at least one listed case (a form that none rejects
means a case is missing); a bound without one of its named terms no longer holds the honest emulation; the exact generators
pass ``is_order_free`` (asserted inside every ``*_case``), which refuses an over-range head-linear operand.
"""

from __future__ import annotations

import pytest
import torch
import torch.nn.functional as F  # noqa: N812

from tests import exact_sums as ex
from tests import heads_numerics as hn

# the attentive cases are the many: the honest sweep runs them all, the wrong forms look at the smaller ones first
_FORMS = [(fam, form) for fam, spec in hn.FAMILIES.items() for form in spec[4]]


def _cases(fam):
    cases = hn.FAMILIES[fam][0]
    if fam == "attn_reduce":       # cheapest first; all of them remain candidates
        return sorted(cases, key=lambda c: c[1] * c[2] * c[3] * c[4])
    return cases


@pytest.mark.parametrize("fam", sorted(hn.FAMILIES))
def test_honest_emulation_is_inside_every_bound_and_equals_every_exact_expectation(fam):
    cases, make, emulate, ratios, _ = hn.FAMILIES[fam]
    worst = {}
    for case in cases:
        d = make(*case)
        for key, r in ratios(d, emulate(d)).items():
            assert r <= 1.0, f"{fam} {hn.case_id(case)} {key}: honest emulation at {r:.3f} x its bound"
            worst[(case[0], key)] = max(worst.get((case[0], key), 0.0), r)
    for (kind, key), r in sorted(worst.items()):
        print(f"{fam} {kind} {key}: worst honest ratio {r:.3g}")


@pytest.mark.parametrize("fam,form", _FORMS, ids=[f"{a}-{b}" for a, b in _FORMS])
def test_every_wrong_form_is_rejected_by_a_listed_case(fam, form):
    _, make, emulate, ratios, _ = hn.FAMILIES[fam]
    for case in _cases(fam):
        d = make(*case)
        bad = {k: r for k, r in ratios(d, emulate(d, form)).items() if not r <= 1.0}
        if bad:
            print(f"{fam} {form}: rejected by {hn.case_id(case)}: {bad}")
            return
    pytest.fail(f"{fam}: no listed case rejects the wrong form {form!r}")


# (family, term, a case of the list at which the honest emulation needs it)
_TERMS = [
    ("resize", "weights", ("randn", 3, 10, 64, 1)),
    ("resize", "blend", ("randn", 7, 3, 192, 3)),
    ("attn_reduce", "dot", ("rising", 192, 3, 17, 16)),
    ("attn_reduce", "store", ("randn1.5", 192, 3, 17, 16)),
    ("head_linear", "acc", ("randn", 1024, 40, 7)),
    ("ce", "lse_round", ("offset1e4", 19, 3, 2, 4, 12, "count", "f32", 8)),
    ("ce", "store", ("randn2", 130, 2, 4, 8, 0, "count", "bf16", 4)),
    ("bce", "exp", ("randn30", 300, 16, "some")),
]


@pytest.mark.parametrize("fam,term,case", _TERMS, ids=[f"{a}-{b}" for a, b, _ in _TERMS])
def test_a_bound_without_one_of_its_terms_rejects_the_honest_emulation(fam, term, case):
    cases, make, emulate, ratios, _ = hn.FAMILIES[fam]
    assert case in cases
    d = make(*case)
    got = emulate(d)
    assert all(r <= 1.0 for r in ratios(d, got).values())
    assert any(not r <= 1.0 for r in ratios(d, got, drop=(term,)).values()), f"{fam}: the bound holds without its term {term!r}"


def test_resize_fp32_and_fp64_interpolate_agree_exactly_on_the_dyadic_operands():
    for h, H in hn.RESIZE_DYADIC:  # noqa: N806
        d = hn.resize_case("exact", h, H, 64, 3)
        B, D, E = d["B"], d["D"], d["E"]  # noqa: N806
        xm = d["x"][:, hn.RESIZE_IN_OFF: hn.RESIZE_IN_OFF + D * h * h].reshape(B * D, h, h, E).permute(0, 3, 1, 2).clone().requires_grad_(True)
        out32 = F.interpolate(xm, (H, H), mode="bilinear", align_corners=False)
        out32.backward(d["dout"][:, hn.RESIZE_OUT_OFF: hn.RESIZE_OUT_OFF + D * H * H].reshape(B * D, H, H, E).permute(0, 3, 1, 2))
        assert torch.equal(out32.detach().permute(0, 2, 3, 1).reshape(B, -1, E).double(), d["out"]), (h, H)
        assert torch.equal(xm.grad.permute(0, 2, 3, 1).reshape(B, -1, E).double(), d["din"]), (h, H)
        assert not torch.equal(d["x"][0, hn.RESIZE_IN_OFF: hn.RESIZE_IN_OFF + h * h], d["x"][0, hn.RESIZE_IN_OFF + h * h: hn.RESIZE_IN_OFF + 2 * h * h])


def test_saturated_cross_entropy_closed_form_is_the_fp64_value_to_1e_57():
    assert float(torch.exp(torch.tensor(-128.0))) == 0.0                    # fp32: the other classes vanish
    d = hn.ce_case("saturated", 19, 3, 2, 4, 12, "pow2", "bf16", 1)
    keep = d["valid"]
    want = F.cross_entropy(d["lg"].double()[keep], d["t"][keep], reduction="sum") / d["word"]
    assert abs(float(want - d["loss"])) <= 18 * 4e-58 * 128 and float(d["loss"]) > 0
    # the word, not the count, is the divisor
    w = hn.ce_case("saturated", 19, 3, 2, 4, 0, "word", "f32", 8)
    assert w["word"] * 2 == w["count"] and float(w["dl"].abs().max()) == 1.0 / w["word"]


def test_exact_generators_and_the_over_range_head_linear_operand():
    assert hn.linear_range(192) == 255 and hn.linear_range(1024) == 127 and hn.linear_range(64) == 255
    for E in hn.LINEAR_E:  # noqa: N806
        r = hn.linear_range(E)
        assert ex.is_order_free(torch.full((E,), float(r * r)), 1.0)
    with pytest.raises(AssertionError):                                      # |x|, |W| <= 255 does not fit E = 1024
        ex.is_order_free(torch.full((1024,), 255.0 * 255.0), 1.0)
    for cases, make, *_rest in hn.FAMILIES.values():                         # every *_case asserts is_order_free on its own terms
        for case in cases:
            if case[0] in ("exact", "saturated", "one_key", "equal_keys"):
                make(*case)


def test_case_lists_cover_what_the_kernels_branch_on():
    ar = hn.AR_CASES
    for dim in hn.AR_DIMS:                                                  # every VPL: exact and bounded
        assert any(c[1] == dim and c[0] in hn.AR_EXACT_KINDS for c in ar) and any(c[1] == dim and c[0] not in hn.AR_EXACT_KINDS for c in ar)
        for shape in hn.AR_SHAPES:
            assert any(c[1] == dim and c[2:] == shape for c in ar)
    assert all((k, d, 3, 17, 16) in ar for k in hn.AR_KINDS for d in (192, 384))
    assert any(B > 256 for _, B, C, _ in hn.BCE_CASES) and any(B * C > 256 for _, B, C, _ in hn.BCE_CASES)
    assert any(B > C for _, _, B, C in hn.LINEAR_CASES) and {c[1] for c in hn.LINEAR_CASES} == set(hn.LINEAR_E)
    assert {c[1] for c in hn.CE_CASES} == {1, 2, 19, 130} and {c[8] for c in hn.CE_CASES} == {1, 2, 4, 8}
    assert {c[2] * c[3] ** 2 * c[4] ** 2 for c in hn.CE_CASES} >= {1, 5, 255, 256, 257, 192, 2048}
    assert {c[6] for c in hn.CE_CASES} >= {"zero", "one", "pow2", "all", "word"} and {c[5] for c in hn.CE_CASES} == {0, 12}
    assert {(h, H) for _, h, H, _, _ in hn.RESIZE_CASES} == set(hn.RESIZE_DYADIC) | set(hn.RESIZE_RATIOS)
