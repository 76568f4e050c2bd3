"""Gradient guard on the GPU: ``mh_grad_sumsq_partial`` / ``mh_grad_guard_finish`` against the numpy restatement of their
contract (``hip.grad_guard_reference``) -- exact sums on integers, fp64 under the bound derived in tests/grad_guard_cases.py,
non-finite inputs, the coefficient, the bias corrections, poisoned guard bands --, ``FusedAdamW.step(guard=...)`` against the
unguarded optimizer, the guarded training loops (poisoned batch, accumulation, resume, deterministic repeats, the one-rank
exchange plan), the launch ledger of default and guarded loops, and the ``clip_grad_norm_`` helper of the Lightning surface.

Sizes (C = MH_GUARD_CHUNK): 4, 8, C - 4, C, C + 4, 3 C + 260 and 257 C + 12 -- the last has more partial rows than the finish
kernel has threads (17 MB; nothing here needs more).  NaN / inf below are DATA in float buffers: no test leaves its buffers."""

from __future__ import annotations

import copy

import numpy as np
import pytest
import torch

from tests import grad_guard_cases as G
from tests import guards
from tests import mask_rng_cases as MC

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
HYPER = dict(lr=1e-3, b1=0.9, b2=0.99)


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _ulp(x) -> float:
    return float(np.spacing(np.abs(np.float32(x))))


def _launch(dev, g, grad_scale=1.0, max_norm=None, skip=True, t=0, skipped=0, **hyper):
    """One guard launch over ``g`` (numpy f32): ``(stats, partial, bad, hyper)`` on the host and the restatement's dict."""
    from maestro_amd import hip
    h = {**HYPER, **hyper}
    guard = hip.GradGuard(g.size, dev, max_norm=max_norm, skip_nonfinite=skip)
    guard.load_state_dict({"t": t, "skipped": skipped})
    guard.launch(torch.from_numpy(g).to(dev), h["lr"], h["b1"], h["b2"], grad_scale)
    torch.cuda.synchronize()
    ref = hip.grad_guard_reference(g, grad_scale, max_norm, skip, h["lr"], h["b1"], h["b2"], t, skipped)
    return guard.stats(), guard.partial.cpu().numpy(), guard.bad.cpu().numpy(), guard.hyper.cpu().numpy(), ref


def _same_decision(stats, hyper, ref):
    assert stats["finite"] == ref["finite"] and stats["bad"] == ref["bad"]
    assert (stats["t"], stats["skipped"]) == (ref["t"], ref["skipped"])
    assert hyper[4] == (1.0 if ref["apply"] else 0.0) and hyper[0] == ref["hyper"][0]
    assert np.isfinite(hyper).all()


# ------------------------------------------------------------------------------------------------ exact sums
@pytest.mark.parametrize("n", G.SIZES)
def test_integer_gradients_sum_exactly(n):
    """|g| <= 8, integers: a chunk's sum of squares is <= 2^20 and exact in fp32 in any order -> bit-equal partials."""
    dev = _dev()
    g = G.integer_gradient(n, seed=n)
    for grad_scale in (1.0, 1.0 / 3.0):
        stats, partial, bad, hyper, ref = _launch(dev, g, grad_scale=grad_scale, t=3, skipped=1)
        exact = G.exact_partials(g)
        assert partial.shape == (G.rows_of(n),) and np.array_equal(partial, exact.astype(np.float32))
        assert np.array_equal(partial.astype(np.int64), exact) and not bad.any()
        want = np.float32(abs(float(np.float32(grad_scale))) * np.sqrt(float(exact.sum())))
        assert abs(stats["norm"] - float(want)) <= _ulp(want), (stats["norm"], want)
        assert abs(stats["norm"] - float(ref["norm"])) <= _ulp(want)
        _same_decision(stats, hyper, ref)
        assert stats["coef"] == 1.0 and hyper[3] == np.float32(grad_scale) and stats["t"] == 4


# ------------------------------------------------------------------------------------------------ error bound
@pytest.mark.parametrize("scale", G.SCALES)
@pytest.mark.parametrize("n", G.SIZES)
def test_partials_and_norm_stay_inside_the_derived_bound(n, scale, observed):
    """Normal draws scaled by 2^-40, 1, 2^50 (every square in the normal range) against fp64 under GAMMA (28 roundings: one per
    square + the longest chain of additions) per chunk and NORM_BOUND for the norm: the derivation is the docstring of
    tests/grad_guard_cases.py; tests/test_grad_guard_host.py shows that two mutated trees leave the bound."""
    dev = _dev()
    g = G.normal_draws(n, scale, seed=n % 1000)
    stats, partial, bad, hyper, ref = _launch(dev, g, grad_scale=0.5)
    ratio = G.partial_error_ratio(partial, g)
    exact = 0.5 * float(np.sqrt(ref["partial"].sum()))
    norm_ratio = abs(stats["norm"] - exact) / (G.NORM_BOUND * exact)
    print(f"grad guard n={n} scale={scale:g}: partial error / bound = {ratio:.4f}, norm error / bound = {norm_ratio:.4f}")
    observed("grad_guard_gpu::error_bound", f"n{n}/scale{scale:g}/partial", ratio)
    observed("grad_guard_gpu::error_bound", f"n{n}/scale{scale:g}/norm", norm_ratio)
    assert not bad.any() and np.isfinite(partial).all()
    assert ratio <= 1.0 and norm_ratio <= 1.0, (ratio, norm_ratio)
    _same_decision(stats, hyper, ref)


# ------------------------------------------------------------------------------------------------ non-finite inputs
@pytest.mark.parametrize("poison", [float("nan"), float("inf"), float("-inf")])
@pytest.mark.parametrize("n", [G.C + 4, 3 * G.C + 260])
def test_one_non_finite_element_skips_the_step(n, poison):
    dev = _dev()
    for pos in (0, G.C - 1, G.C, n - 1):
        g = G.normal_draws(n, 1.0)
        g[pos] = poison
        stats, partial, bad, hyper, ref = _launch(dev, g, max_norm=1.0, t=5, skipped=2)
        want_bad = np.zeros(G.rows_of(n), dtype=np.int64)
        want_bad[pos // G.C] = 1
        assert np.array_equal(bad, want_bad) and np.array_equal(bad, ref["bad_rows"]), (pos, bad)
        assert not stats["finite"] and stats["bad"] == 1 and hyper[4] == 0.0 and stats["coef"] == 1.0
        assert (stats["t"], stats["skipped"]) == (5, 3)
        _same_decision(stats, hyper, ref)
        ok = np.delete(np.arange(G.rows_of(n)), pos // G.C)             # the other chunks are untouched by the poison
        assert np.isfinite(partial[ok]).all() and not np.isfinite(partial[pos // G.C])


def test_overflow_zeros_and_the_switch():
    dev = _dev()
    n = G.C + 4
    stats, partial, bad, hyper, ref = _launch(dev, np.full(n, 2.0 ** 70, dtype=np.float32), max_norm=1.0)
    assert not bad.any() and stats["bad"] == 0 and np.isinf(stats["norm"]) and not stats["finite"]
    assert (stats["t"], stats["skipped"]) == (0, 1) and hyper[4] == 0.0 and hyper[1] == 0.0     # t = 0: still finite numbers
    _same_decision(stats, hyper, ref)
    stats, partial, bad, hyper, ref = _launch(dev, np.zeros(n, dtype=np.float32), max_norm=1.0)
    assert stats["norm"] == 0.0 and stats["coef"] == 1.0 and stats["finite"] and (stats["t"], stats["skipped"]) == (1, 0)
    assert hyper[4] == 1.0 and not partial.any()
    _same_decision(stats, hyper, ref)
    g = G.normal_draws(n, 1.0)
    g[7] = float("nan")
    stats, partial, bad, hyper, ref = _launch(dev, g, max_norm=1.0, skip=False, t=2)
    assert not stats["finite"] and stats["bad"] == 1 and stats["coef"] == 1.0 and hyper[4] == 1.0 and hyper[3] == 1.0
    assert (stats["t"], stats["skipped"]) == (3, 0)
    _same_decision(stats, hyper, ref)


# ------------------------------------------------------------------------------------------------ coefficient
@pytest.mark.parametrize("n", [8, 3 * G.C + 260])
def test_the_coefficient_is_torchs_rule(n):
    """The reference's coefficient is computed from ITS norm; the kernel's norm may differ from it by a few ulps (both are inside
    NORM_BOUND), so the kernel's coefficient is held to 1 ulp of the rule applied to the kernel's own norm, and to
    (2 NORM_BOUND + 2 u) of the reference's."""
    dev = _dev()
    g = G.normal_draws(n, 1.0, seed=5)
    true = float(np.sqrt((g.astype(np.float64) ** 2).sum()))
    for max_norm, clipped in ((0.5 * true, True), (2.0 * true, False), (true, None), (0.0, False), (-1.0, False), (None, False)):
        stats, _, _, hyper, ref = _launch(dev, g, grad_scale=1.0, max_norm=max_norm)
        if not max_norm or max_norm <= 0:
            assert stats["coef"] == 1.0 and ref["coef"] == 1.0
            continue
        rule = min(np.float32(1.0), np.float32(max_norm) / np.float32(np.float32(stats["norm"]) + np.float32(1e-6)))
        assert abs(stats["coef"] - float(rule)) <= _ulp(rule), (stats["coef"], rule)
        assert abs(stats["coef"] - float(ref["coef"])) <= (2 * G.NORM_BOUND + 2 * U) * float(ref["coef"])
        assert hyper[3] == np.float32(stats["coef"]) and stats["coef"] <= 1.0
        if clipped is not None:
            assert (stats["coef"] < 1.0) == clipped
        else:
            assert stats["coef"] >= 1.0 - 4 * G.NORM_BOUND


# ------------------------------------------------------------------------------------------------ bias corrections
@pytest.mark.parametrize("b1,b2", [(0.9, 0.99), (0.9, 0.999)])
def test_bias_corrections_for_early_and_late_steps(b1, b2):
    from maestro_amd import hip
    dev = _dev()
    guard = hip.GradGuard(4, dev)
    g = torch.ones(4, device=dev)
    got = {}
    for t in list(range(1, 65)) + [10 ** 4, 10 ** 6]:
        guard.load_state_dict({"t": t - 1, "skipped": 0})
        guard.launch(g, 1e-3, b1, b2, 1.0)
        got[t] = guard.hyper.clone()
    torch.cuda.synchronize()
    fb1, fb2 = float(np.float32(b1)), float(np.float32(b2))
    for t, h in got.items():
        h = h.cpu().numpy()
        want1, want2 = np.float32(1.0 - fb1 ** t), np.float32(np.sqrt(1.0 - fb2 ** t))
        assert abs(float(h[1]) - float(want1)) <= _ulp(want1) and abs(float(h[2]) - float(want2)) <= _ulp(want2), (t, h, want1, want2)
        assert h[4] == 1.0 and h[3] == 1.0


# ------------------------------------------------------------------------------------------------ guard bands (tests/guards.py)
@pytest.mark.parametrize("n", [4, G.C + 4, 3 * G.C + 260])
def test_nothing_outside_the_views_changes(n):
    """Every operand in the middle of a poisoned allocation; the gradient starts 4 elements (16 bytes, not 32) behind a 256-byte
    boundary, which is what probe's ``trainable_span`` produces.  Outputs start as poison: every row is written."""
    from maestro_amd import hip
    dev = _dev()
    data = G.normal_draws(n, 1.0, seed=9)
    gs = guards.GuardSet(dev)
    g = gs.inp(torch.from_numpy(data), align=16, name="g")
    rows = hip.grad_sumsq_partial_rows(n)
    partial = gs.out((rows,), torch.float32, name="partial")
    bad = gs.out((rows,), torch.int32, name="bad")
    hyper = gs.out((5,), torch.float32, name="hyper")
    state = gs.out((32,), torch.uint8, init=0, name="state")
    assert g.data_ptr() % 32 == 16
    hip.grad_sumsq_partial(g, n, partial, bad)
    hip.grad_guard_finish(partial, bad, rows, 1.0, 0.0, True, 1e-3, 0.9, 0.99, hyper, state)
    gs.check()
    ref = hip.grad_guard_reference(data, 1.0, 0.0, True, 1e-3, 0.9, 0.99, 0, 0)
    assert G.partial_error_ratio(partial.cpu().numpy(), data) <= 1.0 and not bad.cpu().numpy().any()
    got = hyper.cpu().numpy()
    assert np.isfinite(got).all() and got[0] == ref["hyper"][0] and got[3] == 1.0 and got[4] == 1.0
    assert abs(float(got[1]) - float(ref["hyper"][1])) <= _ulp(got[1]) and abs(float(got[2]) - float(ref["hyper"][2])) <= _ulp(got[2])
    st = hip._MhGuardState.from_buffer_copy(bytes(state.cpu().numpy()))
    assert (st.finite, st.bad, st.t, st.skipped, st.coef) == (1, 0, 1, 0, 1.0) and abs(st.norm - float(ref["norm"])) <= G.NORM_BOUND * 2 * st.norm


# ------------------------------------------------------------------------------------------------ optimizer level
def _engine_with_gradients(dev, seed=0):
    model, batch, B = MC.build_model("group", seed=seed)  # noqa: N806
    model._engine = None
    eng = model.engine(B, dev, loss="l2_norm")
    eng.forward({k: v.to(dev) for k, v in batch.items()})
    eng.zero_grad()
    eng.backward()
    torch.cuda.synchronize()
    return eng


def _snapshot(eng):
    st = eng.store
    return st.flat.detach().clone(), st.half.detach().clone()


def _restore(eng, snap):
    eng.store.flat.detach().copy_(snap[0])
    eng.store.half.copy_(snap[1])


def _update_bound(p_before, p_after, lr, wd, delta):
    """Elementwise bound on the difference of two AdamW updates whose step sizes differ by the relative ``delta``.

    adamw_update (csrc/optim.hip): p' = fl(fl(p (1 - lr wd)) - fl(fl(lr / bc1) fl(m / fl(fl(sqrt(v) / bc2) + eps)))).  With equal
    moments and gradient the step s = (lr / bc1) (m / denom) of the two runs differs by the relative change of bc1, of denom
    (at most that of bc2) and of the gradient scale -- their sum is ``delta`` -- plus the five roundings of either run (10 u); the
    decayed parameter and the final subtraction round once in either run (4 u |p|).  |s| is taken from the reference run:
    |s| <= |p' - p| + lr wd |p| + 2 u |p|."""
    p0, p1 = p_before.double().cpu().numpy(), p_after.double().cpu().numpy()
    pmax = np.maximum(np.abs(p0), np.abs(p1))
    s = np.abs(p1 - p0) + lr * wd * np.abs(p0) + 2 * U * pmax
    return s * (delta + 10 * U) * 1.01 + 4 * U * pmax


def test_a_guard_without_clipping_is_the_unguarded_optimizer():
    """Three steps on identical gradients.  hyper[3] = 1 * 1 and the moments do not see the correction terms: m and v are
    bit-equal.  The parameters see 1 - b1^t and sqrt(1 - b2^t) computed in double by the guard and with fp32 powf by mh_adamw
    (``hip.adamw_bias_corrections``): the relative difference of the two forms (host arithmetic on both sides, 0 to 2 ulps)
    enters ``_update_bound``; the per-step bounds add up (the decay factor is < 1)."""
    from maestro_amd import hip
    from maestro_amd.train.optim import FusedAdamW
    dev = _dev()
    eng = _engine_with_gradients(dev)
    st, start = eng.store, _snapshot(eng)
    lr, wd = 1e-3, 0.01
    plain = FusedAdamW(eng, lr, weight_decay=wd)
    track = [start[0]]
    for _ in range(3):
        plain.step()
        track.append(st.flat.detach().clone())
    _restore(eng, start)
    guarded = FusedAdamW(eng, lr, weight_decay=wd)
    guard = hip.GradGuard(guarded.hi - guarded.lo, dev, max_norm=None, skip_nonfinite=True)
    bound = 0.0
    for t in range(1, 4):
        guarded.step(guard=guard)
        k1, k2 = hip.adamw_bias_corrections(0.9, 0.99, t)
        h = hip.grad_guard_reference(np.ones(4, np.float32), 1.0, None, True, lr, 0.9, 0.99, t - 1, 0)["hyper"]
        delta = abs(float(h[1]) - k1) / k1 + abs(float(h[2]) - k2) / k2
        bound += _update_bound(track[t - 1], track[t], lr, wd, delta)
    torch.cuda.synchronize()
    assert guards.bits_equal(guarded.m, plain.m) and guards.bits_equal(guarded.v, plain.v), "the moments must be bit-equal"
    diff = (st.flat.detach().double() - track[3].double()).abs().cpu().numpy()
    lo, hi = guarded.lo, guarded.hi
    assert (diff[lo:hi] <= bound[lo:hi]).all(), float((diff[lo:hi] / np.maximum(bound[lo:hi], 1e-300)).max())
    assert float((track[3] - track[0]).abs().max()) > 0
    assert guards.bits_equal(st.half[lo:hi], st.flat.detach()[lo:hi].bfloat16())
    s = guard.stats()
    assert s["t"] == 3 and s["skipped"] == 0 and s["finite"] and guarded.state_dict()["t"] == 3 and guarded.guard is guard


def test_a_poisoned_gradient_leaves_every_buffer_untouched():
    from maestro_amd import hip
    from maestro_amd.train.optim import FusedAdamW
    dev = _dev()
    eng = _engine_with_gradients(dev)
    st = eng.store
    opt = FusedAdamW(eng, 1e-3)
    guard = hip.GradGuard(opt.hi - opt.lo, dev, max_norm=1.0, skip_nonfinite=True)
    opt.step(guard=guard)                                   # a clean step first: non-zero moments
    torch.cuda.synchronize()
    clean = st.grad[st.total // 2].clone()
    before = (st.flat.detach().clone(), opt.m.clone(), opt.v.clone(), st.half.clone())
    st.grad[st.total // 2] = float("nan")
    opt.step(guard=guard)
    torch.cuda.synchronize()
    after = (st.flat.detach(), opt.m, opt.v, st.half)
    for a, b, name in zip(after, before, ("flat", "m", "v", "half")):
        assert guards.bits_equal(a, b), f"{name} changed on a skipped step"
    s = guard.stats()
    assert (s["t"], s["skipped"], s["bad"], s["finite"]) == (1, 1, 1, False) and opt.state_dict()["t"] == 1
    st.grad[st.total // 2] = clean
    opt.step(guard=guard)
    torch.cuda.synchronize()
    s = guard.stats()
    assert (s["t"], s["skipped"], s["finite"]) == (2, 1, True) and not guards.bits_equal(st.flat.detach(), before[0])
    assert torch.isfinite(st.flat.detach()).all()
    sd = opt.state_dict()
    guard.load_state_dict({"t": 0, "skipped": 0})
    opt.load_state_dict(sd)                                 # writes t back into the device counter; the skip count stays
    assert guard.state_dict() == {"t": 2, "skipped": 0}


def test_probe_phase_does_not_look_below_its_span():
    import maestro_amd.conf as conf
    from maestro_amd.ssl import mae as pmae
    from maestro_amd.train.trainer import SupervisedLoop
    from oracle.gen_golden import build_datasets, make_batch, make_targets
    from tests.test_oracle_sup import CASES
    dev = _dev()
    case = CASES["sup_treesat_mlc"]
    ds = build_datasets(case, conf)
    torch.manual_seed(0)
    model = pmae.mae_tiny(datasets=ds, mask=conf.MaskConfig(), interpolate="nearest", fusion_mode="group", inter_depth=1,
                          model="mae", num_levels=1, type_head="attentive")
    batch = make_batch(ds.dataset, 4, 1)
    batch.update(make_targets(ds.dataset, 4, 1))
    batch = {k: v.to(dev) for k, v in batch.items()}
    loop = SupervisedLoop(model, 4, dev, phase="probe", base_lr=3e-3, total_steps=40, max_grad_norm=1.0, skip_nonfinite=True)
    eng, st = loop.engine, loop.engine.store
    lo, hi = eng.trainable_span
    assert lo > 0 and lo % 4 == 0 and loop.guard.n == hi - lo
    assert torch.isfinite(loop.step(batch)).all()
    eng.forward(batch)
    eng.zero_grad()
    eng.backward()
    st.grad[lo - 1] = float("nan")                          # the frozen encoder's slice: not the guard's business
    before = st.flat.detach().clone()
    loop.opt.step(lr=1e-3, guard=loop.guard)
    torch.cuda.synchronize()
    s = loop.guard.stats()
    assert s["finite"] and s["bad"] == 0 and (s["t"], s["skipped"]) == (2, 0) and loop.skipped_steps == 0
    assert guards.bits_equal(st.flat.detach()[:lo], before[:lo]) and not guards.bits_equal(st.flat.detach()[lo:hi], before[lo:hi])
    st.grad[lo] = float("inf")                              # the first element of the span is
    loop.opt.step(lr=1e-3, guard=loop.guard)
    assert loop.skipped_steps == 1 and not np.isfinite(float(loop.grad_norm))


def test_clipping_is_an_unguarded_step_with_the_host_coefficient():
    """max_grad_norm = half the measured norm against mh_adamw with grad_scale = coef, coef from the fp64 norm on the host.  The
    kernel's coefficient differs from the host's by at most dc = NORM_BOUND + 3 u (its norm, the + 1e-6, the division); the
    first moment then differs by dc, the second by 2 dc, the step s = (lr / bc1) m / (sqrt(v) / bc2 + eps) by at most 2 dc, and
    the correction terms by their own delta -- ``_update_bound``.  One step from zero moments."""
    from maestro_amd import hip
    from maestro_amd.train.optim import FusedAdamW
    dev = _dev()
    eng = _engine_with_gradients(dev)
    st, start = eng.store, _snapshot(eng)
    lr, wd = 1e-3, 0.01
    norm64 = float(st.grad[: st.total].double().norm())
    max_norm = 0.5 * norm64
    coef = float(min(np.float32(1.0), np.float32(max_norm) / np.float32(np.float32(norm64) + np.float32(1e-6))))
    plain = FusedAdamW(eng, lr, weight_decay=wd)
    plain.step(grad_scale=coef)
    want = st.flat.detach().clone()
    _restore(eng, start)
    guarded = FusedAdamW(eng, lr, weight_decay=wd)
    guard = hip.GradGuard(guarded.hi - guarded.lo, dev, max_norm=max_norm, skip_nonfinite=True)
    guarded.step(guard=guard)
    torch.cuda.synchronize()
    s = guard.stats()
    dc = G.NORM_BOUND + 3 * U
    assert abs(s["norm"] - norm64) <= G.NORM_BOUND * norm64 and abs(s["coef"] - coef) <= dc * coef and 0.49 < s["coef"] < 0.51
    k1, k2 = hip.adamw_bias_corrections(0.9, 0.99, 1)
    h = guard.hyper.cpu().numpy()
    delta = abs(float(h[1]) - k1) / k1 + abs(float(h[2]) - k2) / k2 + 2 * dc + 8 * U
    bound = _update_bound(start[0], want, lr, wd, delta)
    diff = (st.flat.detach().double() - want.double()).abs().cpu().numpy()
    assert (diff <= bound).all(), float((diff / np.maximum(bound, 1e-300)).max())
    m_diff = (guarded.m.double() - plain.m.double()).abs()
    v_diff = (guarded.v.double() - plain.v.double()).abs()
    tiny = 1e-37                                             # (below the normal range a rounding is absolute)
    assert bool((m_diff <= (dc + 4 * U) * plain.m.double().abs() + tiny).all())
    assert bool((v_diff <= (2 * dc + 6 * U) * plain.v.double().abs() + tiny).all())
    assert float((want - start[0]).abs().max()) > 0


# ------------------------------------------------------------------------------------------------ loop level
def _loop(dev, seed=0, **kw):
    from maestro_amd.train.trainer import PretrainLoop
    model, batch, B = MC.build_model("group", seed=seed)  # noqa: N806
    model._engine = None
    loop = PretrainLoop(model, B, dev, loss="l2_norm", base_lr=3e-3, total_steps=20, **kw)
    return loop, {k: v.to(dev) for k, v in batch.items()}


def _poisoned(batch, every_sample=False):
    """One NaN pixel in the first raster [B, D, C, S, S] (``every_sample``: one per sample -- the supervised loss leaves samples
    with a missing target out, and which ones those are is the target generator's business)."""
    bad = {k: v.clone() for k, v in batch.items()}
    first = next(k for k, v in bad.items() if v.is_floating_point())
    if every_sample:
        bad[first][:, 0, 0, 0, 5] = float("nan")
    else:
        bad[first].view(-1)[5] = float("nan")
    return bad


def test_a_poisoned_batch_is_survived_with_graphs_on():
    """Steps: clean (eager), clean (capture), POISONED (replay), clean (replay)."""
    dev = _dev()
    loop, batch = _loop(dev, max_grad_norm=1.0, skip_nonfinite=True)
    st = loop.engine.store
    assert loop.engine.use_graphs and loop.guard is not None and loop.opt.guard is loop.guard
    for _ in range(2):
        assert torch.isfinite(loop.step(batch)).all()
    torch.cuda.synchronize()
    assert loop.engine._graphs, "nothing was captured: replays were not exercised"
    before = (st.flat.detach().clone(), loop.opt.m.clone(), loop.opt.v.clone(), st.half.clone())
    loss = loop.step(_poisoned(batch))
    torch.cuda.synchronize()
    assert not torch.isfinite(loss).all()
    for a, b, name in zip((st.flat.detach(), loop.opt.m, loop.opt.v, st.half), before, ("flat", "m", "v", "half")):
        assert guards.bits_equal(a, b), f"{name} changed on the poisoned step"
    assert loop.skipped_steps == 1 and loop.it == 3 and loop.guard.stats()["t"] == 2      # OneCycle advances, Adam's t does not
    loss = loop.step(batch)
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all() and torch.isfinite(st.flat.detach()).all() and not guards.bits_equal(st.flat.detach(), before[0])
    assert loop.skipped_steps == 1 and loop.guard.stats()["t"] == 3 and torch.isfinite(loop.grad_norm).all()
    assert loop.grad_norm.is_cuda and loop.grad_norm.numel() == 1 and float(loop.grad_norm) > 0
    assert sorted(loop.state_dict()) == ["exchange_mode", "guard", "it", "optimizer", "params", "world"]
    assert loop.state_dict()["guard"] == {"t": 3, "skipped": 1} and loop.state_dict()["optimizer"]["t"] == 3


def test_supervised_loop_survives_a_poisoned_batch():
    import maestro_amd.conf as conf
    from maestro_amd.ssl import mae as pmae
    from maestro_amd.train.trainer import SupervisedLoop
    from oracle.gen_golden import build_datasets, make_batch, make_targets
    from tests.test_oracle_sup import CASES
    dev = _dev()
    case = CASES["sup_treesat_mlc"]
    ds = build_datasets(case, conf)
    torch.manual_seed(0)
    model = pmae.mae_tiny(datasets=ds, mask=conf.MaskConfig(), interpolate="nearest", fusion_mode="group", inter_depth=1,
                          model="mae", num_levels=1, type_head="attentive")
    batch = make_batch(ds.dataset, 4, 1)
    batch.update(make_targets(ds.dataset, 4, 1))
    batch = {k: v.to(dev) for k, v in batch.items()}
    loop = SupervisedLoop(model, 4, dev, phase="finetune", base_lr=3e-3, total_steps=40, max_grad_norm=1.0, skip_nonfinite=True)
    st = loop.engine.store
    for _ in range(2):
        assert torch.isfinite(loop.step(batch)).all()
    torch.cuda.synchronize()
    before = (st.flat.detach().clone(), loop.opt.m.clone(), loop.opt.v.clone(), st.half.clone())
    assert not torch.isfinite(loop.step(_poisoned(batch, every_sample=True))).all()
    torch.cuda.synchronize()
    for a, b, name in zip((st.flat.detach(), loop.opt.m, loop.opt.v, st.half), before, ("flat", "m", "v", "half")):
        assert guards.bits_equal(a, b), f"{name} changed on the poisoned step"
    assert loop.skipped_steps == 1 and loop.it == 3
    assert torch.isfinite(loop.step(batch)).all()
    torch.cuda.synchronize()
    assert torch.isfinite(st.flat.detach()).all() and not guards.bits_equal(st.flat.detach(), before[0]) and loop.skipped_steps == 1


def test_resume_restores_the_counters_and_the_next_step():
    dev = _dev()
    kw = dict(max_grad_norm=1.0, skip_nonfinite=True, deterministic=True, mask_rng="device", mask_seed=11)
    loop, batch = _loop(dev, seed=0, **kw)
    loop.step(batch)
    loop.step(_poisoned(batch))
    loop.step(batch)
    sd = copy.deepcopy(loop.state_dict())
    assert sd["guard"] == {"t": 2, "skipped": 1} and sd["optimizer"]["t"] == 2 and sd["it"] == 3
    loop.step(batch)
    torch.cuda.synchronize()
    want, want_norm = loop.engine.store.flat.detach().clone(), loop.grad_norm.clone()
    resumed, _ = _loop(dev, seed=1, **kw)                    # other initial weights: everything comes from the state dict
    resumed.load_state_dict(sd)
    assert resumed.guard.state_dict() == {"t": 2, "skipped": 1} and resumed.skipped_steps == 1
    resumed.step(batch)
    torch.cuda.synchronize()
    assert guards.bits_equal(resumed.engine.store.flat.detach(), want), "the resumed step differs from the uninterrupted run's"
    assert guards.bits_equal(resumed.grad_norm, want_norm) and resumed.guard.state_dict() == {"t": 3, "skipped": 1}


def test_deterministic_guarded_loops_are_bit_equal():
    dev = _dev()
    runs = []
    for _ in range(2):
        loop, batch = _loop(dev, seed=0, max_grad_norm=1e-3, skip_nonfinite=True, deterministic=True, mask_rng="device", mask_seed=3)
        norms = []
        for _ in range(3):
            loop.step(batch)
            norms.append(loop.grad_norm.clone())
        torch.cuda.synchronize()
        runs.append((loop.engine.store.flat.detach().clone(), torch.cat(norms), loop.guard.stats()))
    assert guards.bits_equal(runs[0][0], runs[1][0]) and guards.bits_equal(runs[0][1], runs[1][1])
    assert runs[0][2] == runs[1][2] and runs[0][2]["t"] == 3 and torch.isfinite(runs[0][1]).all()


def test_the_one_rank_exchange_plan_takes_the_finish_path(monkeypatch):
    """No process group: ``exchange=True`` keeps the launch plan and skips the collectives.  Under a guard the loop must call
    ``finish()``, never ``finish_split()``; the update agrees with the loop without an exchange within the tolerance
    tests/test_ddp_gpu.py uses for its one-process comparison (relative L2 of the update < 2e-2)."""
    from maestro_amd.train.ddp import GradSync
    dev = _dev()
    calls = []
    finish, finish_split = GradSync.finish, GradSync.finish_split
    monkeypatch.setattr(GradSync, "finish", lambda self: (calls.append("finish"), finish(self))[1])
    monkeypatch.setattr(GradSync, "finish_split", lambda self: (calls.append("finish_split"), finish_split(self))[1])
    kw = dict(max_grad_norm=1.0, skip_nonfinite=True, mask_rng="device", mask_seed=7)
    flats = []
    for exchange in (True, False):
        loop, batch = _loop(dev, seed=0, exchange=exchange, **kw)
        init = loop.engine.store.flat.detach().clone()
        for _ in range(3):
            assert torch.isfinite(loop.step(batch)).all()
        torch.cuda.synchronize()
        flats.append((loop.engine.store.flat.detach() - init).double())
        assert (loop.sync is not None) == exchange and loop.guard.stats()["t"] == 3
    assert calls == ["finish"] * 3
    rel = float((flats[0] - flats[1]).norm() / flats[1].norm())
    assert float(flats[1].abs().max()) > 0 and rel < 2e-2, rel


# ------------------------------------------------------------------------------------------------ launch ledger
NEW = ("mh_grad_sumsq_partial_rows", "mh_grad_sumsq_partial", "mh_grad_guard_finish")


def _traced(monkeypatch):
    from maestro_amd import hip
    calls, call = [], hip.call

    def traced_call(entry, *args):
        calls.append(entry)
        return call(entry, *args)

    monkeypatch.setattr(hip, "call", traced_call)
    return calls


def test_a_default_loop_issues_todays_launches(monkeypatch):
    from maestro_amd import hip
    dev = _dev()
    for v in ("MAESTRO_MAX_GRAD_NORM", "MAESTRO_SKIP_NONFINITE"):
        monkeypatch.delenv(v, raising=False)
    calls = _traced(monkeypatch)
    built = []

    def no_guard(*args, **kw):
        built.append(args)
        raise AssertionError("a default loop built a gradient guard")

    monkeypatch.setattr(hip, "GradGuard", no_guard)
    loop, batch = _loop(dev)
    for _ in range(3):
        loop.step(batch)
    loop.step([batch, batch])
    torch.cuda.synchronize()
    assert loop.guard is None and loop.opt.guard is None and not built and loop.skipped_steps == 0
    assert not set(calls) & set(NEW) and "mh_adamw_dev" not in calls and calls.count("mh_adamw") == 4
    assert "guard" not in loop.state_dict()
    with pytest.raises(RuntimeError, match="no gradient guard"):
        loop.grad_norm


@pytest.mark.parametrize("how", ["kwargs", "environment"])
def test_a_guarded_loop_issues_the_guard_and_the_device_scalar_update(how, monkeypatch):
    dev = _dev()
    kw = {}
    if how == "environment":
        monkeypatch.setenv("MAESTRO_MAX_GRAD_NORM", "1.0")
        monkeypatch.setenv("MAESTRO_SKIP_NONFINITE", "1")
    else:
        kw = dict(max_grad_norm=1.0, skip_nonfinite=True)
    calls = _traced(monkeypatch)
    loop, batch = _loop(dev, **kw)
    assert loop.guard is not None and loop.guard.max_norm == 1.0 and loop.guard.skip_nonfinite
    for _ in range(3):
        loop.step(batch)
    loop.step([batch, batch])                                # _step_accumulated: one optimizer step
    torch.cuda.synchronize()
    assert calls.count("mh_grad_sumsq_partial") == 4 and calls.count("mh_grad_guard_finish") == 4
    assert calls.count("mh_adamw_dev") == 4 and "mh_adamw" not in calls and "mh_adamw_fp8" not in calls
    assert loop.guard.stats()["t"] == 4 and loop.it == 4 and loop.skipped_steps == 0
    assert abs(float(loop.guard.hyper[3]) - 0.5 * loop.guard.stats()["coef"]) <= U      # 1 / len(micro) rides in the gradient scale


# ------------------------------------------------------------------------------------------------ Lightning surface
def test_clip_grad_norm_helper_is_torchs():
    from maestro_amd.train.optim import clip_grad_norm_
    dev = _dev()
    eng = _engine_with_gradients(dev)
    st = eng.store
    lo, hi = getattr(eng, "trainable_span", (0, st.total))
    g0 = st.grad[lo:hi].clone()
    norm64 = float(g0.double().norm())
    for max_norm in (0.5 * norm64, 2.0 * norm64):
        st.grad[lo:hi].copy_(g0)
        clones = [torch.nn.Parameter(torch.empty_like(p)) for p in st.params if lo <= st.offset[id(p)] < hi]
        for c, p in zip(clones, [p for p in st.params if lo <= st.offset[id(p)] < hi]):
            c.grad = st.g(p).clone()
        tnorm = float(torch.nn.utils.clip_grad_norm_(clones, max_norm))
        norm = clip_grad_norm_(eng, max_norm)
        torch.cuda.synchronize()
        assert norm.is_cuda and norm.dim() == 0
        assert abs(float(norm) - norm64) <= G.NORM_BOUND * norm64 and abs(tnorm - norm64) <= 1e-5 * norm64
        coef = float(eng._clip_guard.coef)
        assert (coef < 1.0) == (max_norm < norm64)
        own = g0 * coef                                      # the product in fp32: what mh_scale_dev computes
        assert guards.bits_equal(st.grad[lo:hi], own)
        slack = abs(float(norm) - tnorm) / norm64 + 6 * U    # the norms' difference moves the coefficient by as much; 6 roundings
        for c, p in zip(clones, [p for p in st.params if lo <= st.offset[id(p)] < hi]):
            d = (st.g(p).double() - c.grad.double()).abs()
            assert bool((d <= slack * c.grad.double().abs() + 1e-45).all()), float(d.max())
    st.grad[lo:hi].copy_(g0)


def test_configure_gradient_clipping_routes_norm_to_the_helper(monkeypatch):
    from types import SimpleNamespace

    import maestro_amd.conf as conf
    import maestro_amd.train.optim as O
    from maestro_amd.train.model import SSLModule
    from oracle.gen_golden import build_datasets, make_batch, make_targets
    from tests.test_oracle_sup import CASES
    dev = _dev()
    case = CASES["sup_treesat_mlc"]
    ds = build_datasets(case, conf)
    torch.manual_seed(0)
    module = SSLModule(datasets=ds, mask=conf.MaskConfig(), interpolate="nearest", fusion_mode="group", inter_depth=1,
                       model="mae", model_size="tiny", type_head="attentive", loss="l2_norm")
    module.trainer = SimpleNamespace(ssl_phase="finetune")
    optimizer = SimpleNamespace(param_groups=[{"params": [p for n, p in module.named_parameters() if n != "_anchor"]}])
    routed = []
    helper = O.clip_grad_norm_
    monkeypatch.setattr(O, "clip_grad_norm_", lambda eng, v: (routed.append(v), helper(eng, v))[1])
    assert float(module.configure_gradient_clipping(optimizer, 1.0, "norm")) == 0.0 and not routed     # no engine yet: torch's
    batch = make_batch(ds.dataset, 4, 1)
    batch.update(make_targets(ds.dataset, 4, 1))
    module.training_step({k: v.to(dev) for k, v in batch.items()}, 0)["loss"].backward()
    eng = module.model._sup_engine
    lo, hi = eng.trainable_span
    norm64 = float(eng.store.grad[lo:hi].double().norm())
    assert module.configure_gradient_clipping(optimizer, None, "norm") is None and not routed
    norm = module.configure_gradient_clipping(optimizer, 0.5 * norm64, None)                             # Lightning's default
    torch.cuda.synchronize()
    assert routed == [0.5 * norm64] and abs(float(norm) - norm64) <= G.NORM_BOUND * norm64
    after = float(eng.store.grad[lo:hi].double().norm())
    assert abs(after - 0.5 * norm64) <= 1e-5 * norm64
    module.configure_gradient_clipping(optimizer, 1e-4, "value")                                         # falls back to torch
    assert len(routed) == 1 and float(eng.store.grad[lo:hi].abs().max()) <= 1e-4
