"""CPU self-check of the step-end test helpers: the exact-sum generators of tests/exact_sums.py really are free of summation
order, the AdamW bounds of tests/numerics.py accept honest fp32 forms and reject the named wrong ones, and the host-side bias
corrections obey their own rounding bound.  No GPU, no HIP library: this is what makes tests/test_step_end_exact_gpu.py and
tests/test_adamw_numerics_gpu.py mean something.
"""

from __future__ import annotations

import math

import pytest
import torch

from tests import exact_sums as ex
from tests import numerics as nm

U = nm.U_F32


# ------------------------------------------------------------------------------------------------ exact sums
def _sum_sequential(x32: torch.Tensor) -> torch.Tensor:
    acc = torch.zeros_like(x32[0])
    for row in x32:
        acc = acc + row
    return acc


def _three_orders(x32: torch.Tensor):
    """fp32 column sums of ``x32 [rows, cols]``: rows first to last, last to first, and in the order of a 64-lane wave."""
    return _sum_sequential(x32), _sum_sequential(x32.flip(0)), nm._wave_sum(x32.t().contiguous())


@pytest.mark.parametrize("name", sorted(ex.GENERATORS))
def test_generators_are_order_free(name):
    for seed in range(3):
        terms, unit = ex.GENERATORS[name](seed)
        assert terms.dtype == torch.float64 and terms.dim() == 2 and terms.abs().sum() > 0
        assert ex.is_order_free(terms, unit, dim=0) and ex.is_order_free(terms, unit)
        x32 = terms.float()
        assert torch.equal(x32.double(), terms)                                  # the operands themselves are fp32 values
        want = terms.sum(0)
        for got in _three_orders(x32):
            assert got.dtype == torch.float32 and torch.equal(got.double(), want), name
        # ... and as ONE sum over all elements (the loss word), again in three orders
        flat = x32.reshape(-1, 1)
        for got in _three_orders(flat):
            assert torch.equal(got.double(), terms.sum().reshape(1)), name


@pytest.mark.parametrize("name", sorted(ex.GENERATORS))
def test_a_dropped_or_doubled_row_changes_the_sum(name):
    terms, _ = ex.GENERATORS[name](0)
    x32 = terms.float()
    r = int(terms.abs().sum(1).argmax())
    dropped = torch.cat([x32[:r], x32[r + 1:]])
    doubled = torch.cat([x32, x32[r: r + 1]])
    want = terms.sum(0)
    for wrong in (dropped, doubled):
        for got in _three_orders(wrong):
            assert not torch.equal(got.double(), want), name
    if name.startswith("loss"):          # the scalar the loss kernels form: its terms are non-negative, so every row counts
        for wrong in (dropped, doubled):
            assert float(_sum_sequential(wrong.reshape(-1, 1))) != float(terms.sum())


def test_the_predicate_refuses_what_is_not_order_free():
    ok = torch.tensor([1.0, -2.0, 3.0])
    assert ex.is_order_free(ok, 1.0)
    with pytest.raises(AssertionError):
        ex.is_order_free(torch.tensor([1.0, 0.5]), 1.0)                  # not a multiple of the unit
    with pytest.raises(AssertionError):
        ex.is_order_free(ok, 3.0)                                        # the unit is no power of two
    with pytest.raises(AssertionError):
        ex.is_order_free(torch.full((2 ** 12,), 2.0 ** 12), 1.0)        # sum |terms| = 2^24: one addition may round
    assert ex.is_order_free(torch.full((2 ** 12,), 2.0 ** 12)[:-1], 1.0)
    # per column (dim = 0) a tall matrix passes where its grand total does not
    tall = torch.full((2 ** 12, 2), 2.0 ** 11)
    assert ex.is_order_free(tall, 1.0, dim=0)
    with pytest.raises(AssertionError):
        ex.is_order_free(tall, 1.0)
    # an order-dependent sum really is one: 2^24 + 1 + 1 in two orders
    a = torch.tensor([2.0 ** 24, 1.0, 1.0])
    assert float(_sum_sequential(a.reshape(-1, 1))) != float(_sum_sequential(a.flip(0).reshape(-1, 1)))


def test_generator_shapes_and_references():
    rec, tgt, k = ex.loss_operands(24, 20, seed=1)
    assert torch.equal((rec.double() - tgt.double()) * 4, k.double()) and int(k.abs().max()) == ex.DIFF_MAX and bool((k == 0).any())
    rec, tgt, k = ex.loss_operands(24, 20, seed=1, window=(5, 2, 2))
    assert tgt.shape == (24, 50)
    paired = tgt.reshape(24, 10, 5)[:, :, 2:4].reshape(24, 20)
    assert torch.equal((rec.double() - paired.double()) * 4, k.double())
    mask, sel = ex.token_mask(3, 13, 2, 8, 16, seed=2)
    assert int(sel.sum()) == 16 and int(mask[:, 2:10].sum()) == 16 and bool(mask[:, :2].all()) and bool(mask[:, 10:].all())
    assert torch.equal(mask[:, 2:10].reshape(-1).bool(), sel)
    view, ints = ex.int_rows(5, 8, ld=12, dtype=torch.bfloat16, seed=3)
    assert torch.equal(view.double(), ints.double()) and view.stride(0) == 12
    d, unit = ex.drec_values(k, sel, 2, 2.0 ** -9)
    assert torch.equal(d.to(torch.bfloat16).double(), d) and unit == 2.0 ** -10 and bool((d[~sel] == 0).all())
    d1, _ = ex.drec_values(k, sel, 1, 2.0 ** -9)
    assert bool((d1[sel][k[sel] == 0] == 0).all()) and set(d1.unique().tolist()) == {-(2.0 ** -9), 0.0, 2.0 ** -9}
    x = torch.arange(10.0)[:, None]
    assert ex.block_sums(x, 4).reshape(-1).tolist() == [6.0, 22.0, 17.0]


# ------------------------------------------------------------------------------------------------ AdamW bounds
def _hyper(step, b2):
    from maestro_amd import hip
    h = nm.ADAMW_HYPER
    bc1, bc2_sqrt = hip.adamw_bias_corrections(h["b1"], b2, step)
    return (h["lr"], h["b1"], b2, h["eps"], h["wd"], bc1, bc2_sqrt, h["grad_scale"])


def _ratio(kind, step, b2, **emu):
    """Worst error / bound over p, m, v of the emulation against the fp64 step."""
    args = _hyper(step, b2)
    p, g, m, v = nm.adamw_inputs(kind, 4100)
    ref = nm.adamw_step64(p, g, m, v, *args)
    bound = nm.adamw_bounds(ref)
    got = nm.adamw_emulated(p, g, m, v, *args, **emu)
    assert all(bool(torch.isfinite(t).all()) for t in got)
    return max(nm.worst_ratio((t.double() - ref[k]).abs(), bound[k]) for t, k in zip(got, "pmv"))


@pytest.mark.parametrize("step,b2", nm.ADAMW_STEPS)
@pytest.mark.parametrize("kind", nm.ADAMW_KINDS)
def test_adamw_bounds_accept_the_honest_forms(kind, step, b2):
    for fma in (False, True):
        r = _ratio(kind, step, b2, fma=fma)
        print(f"adamw {kind} step {step} fma={fma}: worst error / bound = {r:.3f}")
        assert r <= 1.0, (kind, step, fma, r)


@pytest.mark.parametrize("step,b2", nm.ADAMW_STEPS[:2])
@pytest.mark.parametrize("form", nm.ADAMW_WRONG_BC + ("eps_in_sqrt",))
def test_adamw_bounds_reject_misplaced_eps_and_bias_corrections_early(form, step, b2):
    """``tiny``: sqrt(v) is within two orders of eps and the bias corrections are far from 1, so each of these forms moves the step
    by a relative 1e-3 or more where the bound allows 1e-7: rejected by four orders of magnitude."""
    r = _ratio("tiny", step, b2, form=form)
    print(f"adamw tiny step {step} {form}: worst error / bound = {r:.3g}")
    assert r > 1e4, (form, step, r)


@pytest.mark.parametrize("form", nm.ADAMW_WRONG_BC)
def test_adamw_bias_correction_forms_coincide_late(form):
    """At step 100000 both corrections are 1 in fp32: the forms that differ through them alone are the honest form again."""
    step, b2 = nm.ADAMW_STEPS[3]
    assert _hyper(step, b2)[5:7] == (1.0, 1.0)
    for kind in nm.ADAMW_KINDS:
        assert _ratio(kind, step, b2, form=form) <= 1.0, (form, kind)


def test_eps_inside_the_square_root_is_rejected_at_every_step():
    """sqrt(v / bc2 + eps) is not sqrt(v) / bc2_sqrt + eps whatever the corrections are: ``tiny`` sees it late as well."""
    for step, b2 in nm.ADAMW_STEPS:
        assert _ratio("tiny", step, b2, form="eps_in_sqrt") > 1e4, step


@pytest.mark.parametrize("form", nm.ADAMW_WRONG)
def test_every_wrong_adamw_form_is_rejected_somewhere(form):
    rejected = [(kind, step) for kind in nm.ADAMW_KINDS for step, b2 in nm.ADAMW_STEPS if _ratio(kind, step, b2, form=form) > 1.0]
    print(f"{form}: rejected in {len(rejected)} of {len(nm.ADAMW_KINDS) * len(nm.ADAMW_STEPS)} cases")
    assert rejected, form
    if form == "wd_after":       # differs by lr wd |step|: seen where the step is large against p, as in p0
        assert ("p0", 1) in rejected
    if form == "wd_l2":          # the decay passes through the moments: seen wherever p is not 0
        assert ("bigp", 1) in rejected and ("p0", 1) not in rejected


def test_adamw_zero_gradient_and_moments_give_a_zero_step():
    args = _hyper(1, 0.999)
    p, g, m, v = nm.adamw_inputs("zero", 4100)
    ref = nm.adamw_step64(p, g, m, v, *args)
    assert bool((ref["step"] == 0).all()) and bool((ref["m"] == 0).all()) and bool((ref["v"] == 0).all())
    bound = nm.adamw_bounds(ref)
    assert all(bool(torch.isfinite(b).all()) for b in bound.values())
    assert float(bound["step"].max()) < 1e-30         # FL / eps and nothing else: a zero step stays a zero step


# ------------------------------------------------------------------------------------------------ bias corrections
BC_STEPS = tuple(range(1, 200)) + (1000, 4096, 10 ** 4, 10 ** 5, 10 ** 6)


@pytest.mark.parametrize("b1,b2", [(0.9, 0.999), (0.9, 0.95)])
def test_host_bias_corrections_within_their_rounding_bound(b1, b2):
    """``bc1 = fl(1 - fl(powf(b, t)))``: powf is good to an ulp (2u b^t), the subtraction rounds once (u (1 - b^t)).  bc2_sqrt is
    the correctly rounded square root of such a value: the image of that bound under sqrt, plus its own rounding."""
    from maestro_amd import hip
    worst = 0.0
    for step in BC_STEPS:
        bc1, bc2_sqrt = hip.adamw_bias_corrections(b1, b2, step)
        for b, got, root in ((nm.f32(b1), bc1, False), (nm.f32(b2), bc2_sqrt, True)):
            bt = b ** step                       # fp64 power of the fp32 base
            want = 1.0 - bt
            bound = 2 * U * bt + U * want
            if root:
                bound = bound / (2 * math.sqrt(want)) + U * math.sqrt(want)
                want = math.sqrt(want)
            assert abs(got - want) <= bound, (step, b, got, want, bound)
            worst = max(worst, abs(got - want) / bound)
    print(f"bias corrections b1={b1} b2={b2}: worst error / bound = {worst:.3f}")


# ------------------------------------------------------------------------------------------------ trajectory
def test_the_emulated_trajectory_is_of_the_quality_of_torch_adamw():
    """The criterion of tests/test_adamw_numerics_gpu.py's trajectory test, applied to the FMA-contracted emulation with the
    plain emulation and torch.optim.AdamW as the two references: another order of the same quality passes."""
    case = nm.adamw_trajectory_case()
    errs = nm.adamw_trajectory_errors(case, case["emulated_fma"])
    for k in "pmv":
        got, ceiling = errs[k]
        print(f"trajectory {k}: emulated-fma error {got:.3e}, ceiling {ceiling:.3e}")
        assert got <= ceiling, (k, got, ceiling)
