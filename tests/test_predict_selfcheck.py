"""The bound of tests/predict_numerics.py has teeth (CPU): the fp64 softmax and the honest fp32 emulation pass it on every case the
GPU file runs, and each named wrong form fails it on one of those cases."""

import pytest
import torch

from tests import predict_numerics as pn

CASES = [(kind, *shape) for kind in pn.SOFTMAX_KINDS for shape in pn.SOFTMAX_SHAPES]


def _worst(form, kind, B, g, P, C):  # noqa: N803
    x = pn.softmax_logits(kind, B, g, P, C)
    p, conf = pn.softmax_emulated(x, g, P, C, form)
    r = pn.softmax_ratios(x, g, P, C, p, conf)
    return max(r.values())


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_fp64_and_the_honest_emulation_lie_inside_the_bound(case):
    assert _worst("fp64", *case) == 0.0
    assert _worst(None, *case) <= 1.0


def test_the_logits_stay_finite_and_the_hard_cases_are_hard():
    for case in CASES:
        x = pn.softmax_logits(*case)
        assert bool(torch.isfinite(x).all())
    x = pn.softmax_logits("pm60", 2, 3, 2, 6)
    assert float(x.max()) > 55 and float(x.min()) < -55
    x = pn.softmax_logits("equal", 2, 3, 2, 6).reshape(-1, 6)
    assert bool((x == x[:, :1]).all())


# the case that rejects each wrong form: one of CASES, so the GPU file runs it too
REJECTS = {"no_max": ("pm60", 2, 3, 2, 6), "class_stride": ("sigma2", 2, 3, 2, 6), "bf16": ("sigma2", 3, 1, 1, 19)}


@pytest.mark.parametrize("form", pn.SOFTMAX_WRONG)
def test_every_wrong_form_is_rejected_by_a_case_of_the_gpu_file(form):
    assert REJECTS[form] in CASES
    assert _worst(form, *REJECTS[form]) > 1.0, form


@pytest.mark.parametrize("shape", pn.SIGMOID_SHAPES, ids=str)
def test_sigmoid_emulation_lies_inside_its_bound_and_bf16_does_not(shape):
    x = pn.sigmoid_logits(*shape)
    assert pn.sigmoid_ratio(x, pn.sigmoid_emulated(x)) <= 1.0
    assert pn.sigmoid_ratio(x, 1.0 / (1.0 + torch.exp(-x.double()))) == 0.0
    assert pn.sigmoid_ratio(x, pn.bf16_round(pn.sigmoid_emulated(x))) > 1.0
