"""``mh_adamw_groups`` / ``mh_adamw_groups_dev`` (include/maestro_hip.h) and the two surfaces built on them.

The main check is bit identity: one grouped launch equals one ``mh_adamw`` launch per span with that span's
``lr_g = float32(lr) * float32(scale)`` (one fp32 product, numpy's) and weight decay -- on a buffer whose group boundaries fall
inside a wave, on a workgroup edge, inside a workgroup off a wave edge, and whose last span holds the 4-element tail.  The fp64
check uses the bounds of tests/numerics.py (``adamw_bounds``) per group: there is no new tolerance in this file.  Then slices of
the flat layout with the map offset, poisoned guard bands around every operand (tests/guards.py), the built-in finetune loop
against one ``hip.adamw`` launch per parameter, and the Lightning surface.
"""

from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import guards
from tests import numerics as nm

pytestmark = pytest.mark.gpu

N = 64 * 67 + 4                      # 4292: four workgroups of 1024 and a fifth of 196; the last block holds 4 elements
BLOCKS = (0, 1, 16, 17, 50, 68)      # span k = blocks [BLOCKS[k], BLOCKS[k + 1]): boundaries inside a wave (element 64), on a
#                                      workgroup edge (1024), inside a workgroup off a wave edge (1088), at 3200; the tail is in the last
IDS = (3, 0, 5, 3, 1)                # unsorted, id 3 on two separated spans; ids 2 and 4 never appear in the map
SCALE = [0.75 ** k for k in range(6)]
WD = [0.05, 0.0, 0.07, 0.02, 0.09, 0.01]       # distinct, one of them 0
STEPS = ((1, 0.999), (1000, 0.999))
R = 0.75


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _tables(dev, scale=SCALE, wd=WD):
    ls, w = torch.zeros(256), torch.zeros(256)
    ls[: len(scale)] = torch.tensor(scale, dtype=torch.float64).float()
    w[: len(wd)] = torch.tensor(wd, dtype=torch.float64).float()
    return ls.to(dev), w.to(dev)


def _map(dev):
    m = torch.zeros(BLOCKS[-1], dtype=torch.uint8)
    for k, gid in enumerate(IDS):
        m[BLOCKS[k]: BLOCKS[k + 1]] = gid
    return m.to(dev)


def _spans():
    """``(lo, hi, lr_g, wd)`` in elements, ``lr_g`` the fp32 product as a Python float."""
    lr = np.float32(nm.ADAMW_HYPER["lr"])
    return [(64 * BLOCKS[k], min(64 * BLOCKS[k + 1], N), float(lr * np.float32(SCALE[gid])), WD[gid]) for k, gid in enumerate(IDS)]


def _fresh(dev, p, g, m, v):
    return (p.to(dev).clone(), g.to(dev), m.to(dev).clone(), v.to(dev).clone(),
            torch.full((p.numel(),), float("nan"), dtype=torch.bfloat16, device=dev))


_CASES: dict = {}


def _case(dev, kind, step, b2):
    """Inputs, the grouped launch, its device-scalar form and the per-span reference of one (kind, step), computed once."""
    from maestro_amd import hip
    key = (kind, step, b2)
    if key in _CASES:
        return _CASES[key]
    h = nm.ADAMW_HYPER
    host = nm.adamw_inputs(kind, N)
    gmap, (ls, wd) = _map(dev), _tables(dev)
    p, g, m, v, pb = _fresh(dev, *host)
    hip.adamw_groups(p, g, m, v, pb, gmap, ls, wd, N, h["lr"], h["b1"], b2, h["eps"], step, h["grad_scale"])
    got = (p, m, v, pb)
    p, g, m, v, pb = _fresh(dev, *host)
    bc1, bc2_sqrt = hip.adamw_bias_corrections(h["b1"], b2, step)
    hyper = torch.tensor([h["lr"], bc1, bc2_sqrt, h["grad_scale"], 1.0], dtype=torch.float32, device=dev)
    hip.adamw_groups_dev(p, g, m, v, pb, gmap, ls, wd, N, h["b1"], b2, h["eps"], hyper)
    got_dev = (p, m, v, pb)
    p, g, m, v, pb = _fresh(dev, *host)
    for lo, hi, lr_g, wd_g in _spans():
        hip.adamw(p[lo:hi], g[lo:hi], m[lo:hi], v[lo:hi], pb[lo:hi], hi - lo, lr_g, h["b1"], b2, h["eps"], wd_g, step, h["grad_scale"])
    torch.cuda.synchronize()
    _CASES[key] = dict(host=host, got=got, got_dev=got_dev, want=(p, m, v, pb))
    return _CASES[key]


def test_the_layout_of_the_case():
    spans = _spans()
    assert [s[:2] for s in spans] == [(0, 64), (64, 1024), (1024, 1088), (1088, 3200), (3200, N)] and N == 4292 and N % 64 == 4
    assert 64 % 256 != 0 and 1024 % 1024 == 0 and 1088 % 1024 == 64 and spans[-1][1] - 64 * 67 == 4
    assert len(set(WD)) == len(WD) and 0.0 in WD and list(IDS) != sorted(IDS) and IDS.count(3) == 2
    assert spans[0][2] == spans[3][2] == float(np.float32(1e-3) * np.float32(0.75 ** 3))


@pytest.mark.parametrize("step,b2", STEPS)
@pytest.mark.parametrize("kind", nm.ADAMW_KINDS)
def test_one_grouped_launch_is_one_adamw_launch_per_span_bit_for_bit(dev, kind, step, b2):
    c = _case(dev, kind, step, b2)
    for name, a, b, w in zip(("p", "m", "v", "p_bf16"), c["got"], c["got_dev"], c["want"]):
        assert guards.bits_equal(a, w), f"mh_adamw_groups: {name} differs from the per-span mh_adamw launches ({kind}, step {step})"
        assert guards.bits_equal(b, w), f"mh_adamw_groups_dev: {name} differs from the per-span mh_adamw launches ({kind}, step {step})"
    assert guards.bits_equal(c["got"][3], c["got"][0].bfloat16()), "p_bf16 is not p.bfloat16()"
    if kind != "zero":
        assert not guards.bits_equal(c["got"][1], c["host"][2].to(dev)), "nothing moved"


def test_inactive_device_form_keeps_every_bit(dev):
    from maestro_amd import hip
    h = nm.ADAMW_HYPER
    host = nm.adamw_inputs("unit", N)
    p, g, m, v, pb = _fresh(dev, *host)
    g = g.clone()
    before = [t.clone() for t in (p, g, m, v, pb)]
    gmap, (ls, wd) = _map(dev), _tables(dev)
    hyper = torch.tensor([h["lr"], 0.5, 0.5, h["grad_scale"], 0.0], dtype=torch.float32, device=dev)
    hip.adamw_groups_dev(p, g, m, v, pb, gmap, ls, wd, N, h["b1"], 0.999, h["eps"], hyper)
    torch.cuda.synchronize()
    for name, a, b in zip(("p", "g", "m", "v", "p_bf16"), (p, g, m, v, pb), before):
        assert guards.bits_equal(a, b), f"{name} changed with active == 0"
    assert bool(torch.isnan(pb.float()).all())               # the NaN-filled shadow is still NaN


@pytest.mark.parametrize("step,b2", STEPS)
def test_a_single_group_of_scale_one_is_mh_adamw(dev, step, b2):
    from maestro_amd import hip
    h = nm.ADAMW_HYPER
    groups = hip.ParamGroups([(0, 64 * 68, 1.0, h["wd"])], dev)
    assert groups.group_of.numel() == 68 and int(groups.group_of.max()) == 0 and groups.lr_scale.numel() == 256
    for kind in ("unit", "cancel"):
        host = nm.adamw_inputs(kind, N)
        p, g, m, v, pb = _fresh(dev, *host)
        hip.adamw_groups(p, g, m, v, pb, groups.map_at(0), groups.lr_scale, groups.wd, N, h["lr"], h["b1"], b2, h["eps"], step,
                         h["grad_scale"])
        q, g2, m2, v2, qb = _fresh(dev, *host)
        hip.adamw(q, g2, m2, v2, qb, N, h["lr"], h["b1"], b2, h["eps"], h["wd"], step, h["grad_scale"])
        torch.cuda.synchronize()
        for name, a, b in zip(("p", "m", "v", "p_bf16"), (p, m, v, pb), (q, m2, v2, qb)):
            assert guards.bits_equal(a, b), (kind, name)


@pytest.mark.parametrize("step,b2", STEPS)
@pytest.mark.parametrize("kind", nm.ADAMW_KINDS)
def test_every_group_is_inside_the_fp64_bound(dev, observed, kind, step, b2):
    from maestro_amd import hip
    h = nm.ADAMW_HYPER
    c = _case(dev, kind, step, b2)
    p, g, m, v = c["host"]
    bc1, bc2_sqrt = hip.adamw_bias_corrections(h["b1"], b2, step)
    got = [t.double().cpu() for t in c["got"][:3]]
    worst = {}
    for lo, hi, lr_g, wd_g in _spans():
        ref = nm.adamw_step64(p[lo:hi], g[lo:hi], m[lo:hi], v[lo:hi], lr_g, h["b1"], b2, h["eps"], wd_g, bc1, bc2_sqrt, h["grad_scale"])
        bound = nm.adamw_bounds(ref)
        for t, k in zip(got, "pmv"):
            assert bool(torch.isfinite(t[lo:hi]).all()), f"{k} is not finite"
            worst[k] = max(worst.get(k, 0.0), nm.worst_ratio((t[lo:hi] - ref[k]).abs(), bound[k]))
    for k, r in worst.items():
        print(f"adamw_groups {kind} step {step} {k}: worst error / bound = {r:.3f}")
        observed("adamw_groups_gpu::fp64_bound", f"{kind}/step{step}/{k}", r)
        assert r <= 1.0, (kind, step, k, r)


def test_a_slice_with_the_map_offset_is_the_whole_launch_on_that_range(dev):
    from maestro_amd import hip
    h = nm.ADAMW_HYPER
    a, b = 64 * 3, 64 * 52 + 8                                # a is no multiple of 1024; b ends inside a block, past three boundaries
    assert a % 1024 and (b - a) % 4 == 0 and b % 64 and b < N
    host = nm.adamw_inputs("unit", N)
    gmap, (ls, wd) = _map(dev), _tables(dev)
    whole = _fresh(dev, *host)
    hip.adamw_groups(whole[0], whole[1], whole[2], whole[3], whole[4], gmap, ls, wd, N, h["lr"], h["b1"], 0.999, h["eps"], 7,
                     h["grad_scale"])
    part = _fresh(dev, *host)
    start = [t.clone() for t in part]
    p, g, m, v, pb = part
    hip.adamw_groups(p[a:b], g[a:b], m[a:b], v[a:b], pb[a:b], gmap[a // 64:], ls, wd, b - a, h["lr"], h["b1"], 0.999, h["eps"], 7,
                     h["grad_scale"])
    torch.cuda.synchronize()
    for name, t, w, s in zip(("p", "g", "m", "v", "p_bf16"), part, whole, start):
        assert guards.bits_equal(t[a:b], w[a:b]), f"{name}: the slice launch differs from the whole-buffer launch on [a, b)"
        assert guards.bits_equal(t[:a], s[:a]) and guards.bits_equal(t[b:], s[b:]), f"{name}: a byte outside [a, b) changed"
    assert not guards.bits_equal(part[0][a:b], start[0][a:b])
    groups = hip.ParamGroups([(64 * BLOCKS[k], 64 * BLOCKS[k + 1], SCALE[gid], WD[gid]) for k, gid in enumerate(IDS)], dev)
    assert groups.map_at(a).data_ptr() == groups.group_of.data_ptr() + a // 64       # what FusedAdamW passes for a slice
    again = _fresh(dev, *host)                                 # ParamGroups renumbers the ids: same pairs, same bits
    hip.adamw_groups(again[0][a:b], again[1][a:b], again[2][a:b], again[3][a:b], again[4][a:b], groups.map_at(a), groups.lr_scale,
                     groups.wd, b - a, h["lr"], h["b1"], 0.999, h["eps"], 7, h["grad_scale"])
    torch.cuda.synchronize()
    for t, w in zip(again, part):
        assert guards.bits_equal(t, w)


# ------------------------------------------------------------------------------------------------ the built-in loop
def _finetune_setup(dev, **loop_kw):
    import maestro_amd.conf as conf
    from maestro_amd.ssl import mae as pmae
    from maestro_amd.train.trainer import SupervisedLoop
    from oracle.gen_golden import build_datasets, make_batch, make_targets
    from tests.test_oracle_sup import CASES
    ds = build_datasets(CASES["sup_treesat_mlc"], conf)
    torch.manual_seed(0)
    model = pmae.mae_tiny(datasets=ds, mask=conf.MaskConfig(), interpolate="nearest", fusion_mode="group", inter_depth=1,
                          model="mae", num_levels=1, type_head="attentive", depth=3)
    batch = make_batch(ds.dataset, 4, 1)
    batch.update(make_targets(ds.dataset, 4, 1))
    batch = {k: v.to(dev) for k, v in batch.items()}
    loop = SupervisedLoop(model, 4, dev, phase="finetune", base_lr=3e-3, weight_decay=0.05, total_steps=40, lw_decay=R,
                          no_decay_1d=True, **loop_kw)
    return loop, batch


def _per_parameter(loop):
    """``(name, lo, hi, scale, wd)`` per parameter from the layer rule, independent of the loop's ParamGroups."""
    from maestro_amd.train.optim import layer_scale
    st, m = loop.engine.store, loop.engine.model
    offs = [st.offset[id(p)] for p in st.params] + [st.total]
    return [(n, offs[k], offs[k + 1], layer_scale(n, m.depth, m.inter_depth, R), 0.0 if p.ndim <= 1 else 0.05)
            for k, (n, p) in enumerate(zip(st.names, st.params))]


@pytest.mark.parametrize("guarded", [False, True])
def test_finetune_loop_equals_one_adamw_launch_per_parameter(dev, guarded):
    """One optimizer step of ``SupervisedLoop(lw_decay=0.75, no_decay_1d=True)`` against ``hip.adamw`` per parameter on copies,
    each with the rule's ``lr_g`` and weight decay; under a clipping gradient guard the reference is ``hip.adamw_dev`` with the
    guard's own scalars (coefficient in the gradient scale) and ``lr_g`` in place of the base rate."""
    from maestro_amd import hip
    loop, batch = _finetune_setup(dev, **(dict(max_grad_norm=1e-3) if guarded else {}))
    eng, st, opt = loop.engine, loop.engine.store, loop.opt
    assert opt.groups is loop.groups and loop.groups is not None and (loop.guard is not None) == guarded
    assert torch.isfinite(loop.step(batch)).all()             # a first step: non-zero moments
    eng.forward(batch)
    eng.zero_grad()
    eng.backward()
    torch.cuda.synchronize()
    flat, grad, m, v = st.flat.detach().clone(), st.grad.clone(), opt.m.clone(), opt.v.clone()
    half = torch.full_like(st.half, float("nan"))
    lr = loop.sched.lr(loop.it)
    opt.step(lr=lr, grad_scale=1.0, guard=loop.guard)
    torch.cuda.synchronize()
    params = _per_parameter(loop)
    assert params[0][1] == 0 and params[-1][2] == st.total and (opt.lo, opt.hi) == (0, st.total)
    scales = {s for _, _, _, s, _ in params}
    assert len(scales) >= 5 and {w for *_, w in params} == {0.0, 0.05}
    b1, b2 = opt.betas
    if guarded:
        s = loop.guard.stats()
        assert s["t"] == 2 and s["finite"] and 0.0 < s["coef"] < 1.0, s         # the guard clips
        hyper = loop.guard.hyper.clone()
        base = np.float32(float(hyper[0]))
        assert float(base) == float(np.float32(lr)) and float(hyper[3]) == float(np.float32(s["coef"]))
    else:
        assert opt.t == 2
    for _, lo, hi, scale, wd in params:
        if guarded:
            hyper[0] = float(base * np.float32(scale))
            hip.adamw_dev(flat[lo:hi], grad[lo:hi], m[lo:hi], v[lo:hi], half[lo:hi], hi - lo, b1, b2, opt.eps, wd, hyper)
        else:
            lr_g = float(np.float32(lr) * np.float32(scale))
            hip.adamw(flat[lo:hi], grad[lo:hi], m[lo:hi], v[lo:hi], half[lo:hi], hi - lo, lr_g, b1, b2, opt.eps, wd, 2, 1.0)
    torch.cuda.synchronize()
    for name, a, b in zip(("flat", "m", "v", "half"), (st.flat.detach(), opt.m, opt.v, st.half), (flat, m, v, half)):
        assert guards.bits_equal(a, b), f"{name}: the grouped step differs from one launch per parameter"
    assert bool(torch.isfinite(st.flat.detach()).all()) and sorted(opt.state_dict()) == \
        ["exchange_mode", "lr", "m", "span", "t", "v", "world"]


# ------------------------------------------------------------------------------------------------ the Lightning surface
def test_lightning_surface_binds_the_grouped_path_and_leaves_it_when_the_ratio_breaks(dev, observed):
    import maestro_amd.conf as conf
    from maestro_amd import hip
    from maestro_amd.train.model import SSLModule
    from maestro_amd.train.optim import layer_scale
    from oracle.gen_golden import build_datasets, make_batch, make_targets
    from tests.test_oracle_sup import CASES
    ds = build_datasets(CASES["sup_treesat_mlc"], conf)
    torch.manual_seed(0)
    module = SSLModule(datasets=ds, mask=conf.MaskConfig(), interpolate="nearest", fusion_mode="group", inter_depth=1,
                       model="mae", model_size="tiny", type_head="attentive", loss="l2_norm")
    module.trainer = SimpleNamespace(ssl_phase="finetune", lw_decay=R, train_dataloader=SimpleNamespace(batch_size=4),
                                     accumulate_grad_batches=1, num_nodes=1, num_devices=1, base_lr=3e-3, wd=0.05, b1=0.9, b2=0.99,
                                     final_factor=1e7, estimated_stepping_batches=40, max_epochs=5)
    batch = make_batch(ds.dataset, 4, 1)
    batch.update(make_targets(ds.dataset, 4, 1))
    batch = {k: v.to(dev) for k, v in batch.items()}
    cfg = module.configure_optimizers()
    opt, sched = cfg["optimizer"], cfg["lr_scheduler"]["scheduler"]
    assert len(opt.param_groups) > 10 and opt.param_groups[-1]["name"] == "heads"

    def backward(i):
        out = module.training_step(batch, i)
        opt.zero_grad(set_to_none=True)
        out["loss"].backward()

    backward(0)
    opt.step()
    sched.step()
    assert opt._fused is not None and opt._fused.groups is not None and opt._fused.t == 1, "the fused grouped path was not bound"
    backward(1)
    eng = module.model._sup_engine
    st, fused = eng.store, opt._fused
    torch.cuda.synchronize()
    snap = [t.detach().cpu().clone() for t in (st.flat, st.grad, fused.m, fused.v)]
    lr_last = float(opt.param_groups[-1]["lr"])
    opt.step()
    sched.step()
    torch.cuda.synchronize()
    assert fused.t == 2 and opt._fused is fused and opt._bound is eng
    got = st.flat.detach().double().cpu()
    m_depth, inter = module.model.depth, module.model.inter_depth
    bc1, bc2_sqrt = hip.adamw_bias_corrections(0.9, 0.99, 2)
    offs = [st.offset[id(p)] for p in st.params] + [st.total]
    worst = 0.0
    for k, (name, p) in enumerate(zip(st.names, st.params)):
        lo, hi = offs[k], offs[k + 1]
        scale, wd = fused.groups.of(lo)                       # the fp32 table entries of this parameter's group ...
        want_scale = layer_scale(name, m_depth, inter, R)     # ... which are the rule's up to the rounding of lr_g / lr_last
        assert abs(scale - want_scale) <= 1e-6 * want_scale and wd == float(np.float32(0.05)), name
        lr_g = float(np.float32(lr_last) * np.float32(scale))
        ref = nm.adamw_step64(snap[0][lo:hi], snap[1][lo:hi], snap[2][lo:hi], snap[3][lo:hi], lr_g, 0.9, 0.99, 1e-8, wd, bc1, bc2_sqrt, 1.0)
        worst = max(worst, nm.worst_ratio((got[lo:hi] - ref["p"]).abs(), nm.adamw_bounds(ref)["p"]))
    print(f"lightning grouped step: worst error / bound = {worst:.3f}")
    observed("adamw_groups_gpu::lightning", "p", worst)
    assert worst <= 1.0, worst
    # one group's lr leaves the ratio: torch's step runs and still updates every parameter
    opt.param_groups[0]["max_lr"] *= 2.0
    opt.param_groups[0]["initial_lr"] *= 2.0
    sched.step()
    backward(2)
    torch.cuda.synchronize()
    before = st.flat.detach().clone()
    has_grad = [bool((st.g(p) != 0).any()) for p in st.params]
    opt.step()
    torch.cuda.synchronize()
    assert opt._bound is None and fused.t == 2, "the grouped launch ran although one group's lr had left the ratio"
    moved = [not torch.equal(st.flat.detach()[offs[k]: offs[k] + p.numel()], before[offs[k]: offs[k] + p.numel()])
             for k, p in enumerate(st.params)]
    assert all(mv for mv, hg in zip(moved, has_grad) if hg) and sum(has_grad) >= 0.9 * len(has_grad)
    assert bool(torch.isfinite(st.flat.detach()).all())


# ------------------------------------------------------------------------------------------------ guard bands (tests/guards.py)
@pytest.mark.parametrize("entry", ["adamw_groups", "adamw_groups_dev"])
def test_guard_bands_around_every_operand_the_map_and_both_tables(dev, entry):
    from maestro_amd import hip
    h = nm.ADAMW_HYPER
    host = nm.adamw_inputs("unit", N)
    gs = guards.GuardSet(dev)
    p, m, v = (gs.out((N,), name=k) for k in "pmv")
    pb = gs.out((N,), torch.bfloat16, align=8, name="p_bf16")
    g = gs.inp(host[1], name="g")
    gmap = gs.inp(_map(dev).cpu(), fill="e8m0", align=1, name="group map")           # bands of 0xFF, an odd base address
    ls_h, wd_h = (t.cpu() for t in _tables(dev))
    ls, wd = gs.inp(ls_h, name="lr_scale"), gs.inp(wd_h, name="wd")
    assert ls.numel() == 256 and wd.numel() == 256 and gmap.numel() == 68 and gmap.data_ptr() % 2 == 1
    p.copy_(host[0])
    m.copy_(host[2])
    v.copy_(host[3])
    gs.arm()
    if entry == "adamw_groups":
        hip.adamw_groups(p, g, m, v, pb, gmap, ls, wd, N, h["lr"], h["b1"], 0.999, h["eps"], 3, h["grad_scale"])
    else:
        bc1, bc2_sqrt = hip.adamw_bias_corrections(h["b1"], 0.999, 3)
        hyper = gs.inp(torch.tensor([h["lr"], bc1, bc2_sqrt, h["grad_scale"], 1.0]), name="hyper")
        hip.adamw_groups_dev(p, g, m, v, pb, gmap, ls, wd, N, h["b1"], 0.999, h["eps"], hyper)
    gs.check()
    q, g2, m2, v2, qb = _fresh(dev, *host)
    for lo, hi, lr_g, wd_g in _spans():
        hip.adamw(q[lo:hi], g2[lo:hi], m2[lo:hi], v2[lo:hi], qb[lo:hi], hi - lo, lr_g, h["b1"], 0.999, h["eps"], wd_g, 3, h["grad_scale"])
    torch.cuda.synchronize()
    for name, a, b in zip(("p", "m", "v", "p_bf16"), (p, m, v, pb), (q, m2, v2, qb)):
        assert guards.bits_equal(a, b), name
