"""Device-side mask draws on the GPU: ``mh_mask_draw`` against the numpy restatement of its contract bit for bit (plain buffers
and between poisoned guard bands), the engine in ``mask_rng="device"`` mode (the draws of four consecutive steps through the
start-up passes, the capture run and the replays; nothing downstream changes; split invariance; no pinned ring) and the
resumed training loop."""

from __future__ import annotations

import copy

import pytest
import torch

from maestro_amd.layers.utils import mask_draw_jobs, mask_draw_reference
from tests import guards
from tests import mask_rng_cases as C

pytestmark = pytest.mark.gpu

SEED = (0xC0FFEE << 40) | 0x1234567        # high bits set
STEPS = (0, 1, 2 ** 32 - 1)
ROW_BASE = 5


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _rows_of(draws, g):
    from maestro_amd.engine import MAEEngine
    return MAEEngine._rows_of(draws, g)


def _check_against_reference(groups, mods, B, bufs, seed, step, row_base, what):  # noqa: N803
    noise, struct = mask_draw_reference(groups, mods, B, seed, step, row_base)
    for g in groups:
        n_dev, s_dev = bufs[g.name]
        want = _rows_of(noise, g).contiguous()
        assert guards.bits_equal(n_dev.cpu(), want), f"{what}: noise of {g.name} differs from the restatement (step {step})"
        assert torch.equal(s_dev.cpu(), struct[g.name].to(torch.uint8)), f"{what}: struct of {g.name} differs (step {step})"


def _set_beff(groups, mods, B):  # noqa: N803
    for m in mods.values():
        m.Beff = B * m.Dates // m.D
    for g in groups:
        g.Beff = g.mods[0].Beff


def _specs(kind, L, kinds="mbdl"):  # noqa: N803
    if kind == "folded":
        return C.hand_built_folded(L)
    return C.hand_built(L, kinds=kinds, p_mod=0.9, two_mods=kind == "two_mods")


# ------------------------------------------------------------------------------------------------ kernel = restatement
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("L", [1, 9, 25, 64])
@pytest.mark.parametrize("kind", ["plain", "two_mods", "folded"])
def test_kernel_is_the_restatement_bit_for_bit(kind, L, B):  # noqa: N803
    """D = 2 dates, two band-groups, (``two_mods``) a group of two modalities with different L; every kind alone and all
    together; p_mod = 0.9: several attempts per row, and with mod alone rows that exhaust the bound."""
    from maestro_amd import hip
    dev = _dev()
    for kinds in (("",) if kind == "folded" else ("m", "b", "d", "l", "mbdl")):
        groups, mods = _specs(kind, L, kinds)
        _set_beff(groups, mods, B)
        jobs = mask_draw_jobs(groups, mods, B)
        bufs = {j["name"]: (torch.full((j["Beff"], j["L"]), float("nan"), device=dev),
                            torch.full((j["Beff"], j["L"]), 7, dtype=torch.uint8, device=dev)) for j in jobs}
        table = hip.MaskDraw(jobs, bufs, dev)
        for step in STEPS:
            table.launch(SEED, step, ROW_BASE)
            torch.cuda.synchronize()
            _check_against_reference(groups, mods, B, bufs, SEED, step, ROW_BASE, f"{kind} L={L} B={B} kinds={kinds!r}")


def test_the_bound_is_exercised():
    """p_mod = 0.9 on both band-groups of one modality (one mod draw for the group): 64 rows, most need a later attempt; p_mod = 1
    cannot come from the engine but the kernel still ends, all-clear."""
    from maestro_amd import hip
    dev = _dev()
    for p_mod in (0.9, 1.0):
        groups, mods = C.hand_built(9, kinds="ml", p_mod=p_mod)
        _set_beff(groups, mods, 64)
        jobs = mask_draw_jobs(groups, mods, 64)
        bufs = {j["name"]: (torch.empty((j["Beff"], j["L"]), device=dev), torch.full((j["Beff"], j["L"]), 7, dtype=torch.uint8, device=dev))
                for j in jobs}
        hip.MaskDraw(jobs, bufs, dev).launch(SEED, 2, 0)
        torch.cuda.synchronize()
        _check_against_reference(groups, mods, 64, bufs, SEED, 2, 0, f"p_mod={p_mod}")
        s = bufs["ga"][1].cpu()
        assert not s.bool().all(dim=1).any()
        if p_mod == 1.0:
            assert not s.any()


# ------------------------------------------------------------------------------------------------ guard bands (tests/guards.py)
@pytest.mark.parametrize("kind,L,B", [("plain", 9, 3), ("plain", 25, 3), ("two_mods", 1, 1), ("two_mods", 25, 3), ("two_mods", 64, 3),
                                      ("folded", 9, 3), ("folded", 64, 1)])
def test_nothing_outside_the_views_changes(kind, L, B):  # noqa: N803
    """Outputs start as poison (NaN / a byte pattern) between poisoned bands: every element of the [Beff, L] views is written,
    nothing around them is.  Row lengths 18, 50, 13, 109 are no multiples of 4 (scalar noise stores), 36, 256 + 9 ... are mixed."""
    from maestro_amd import hip
    dev = _dev()
    groups, mods = _specs(kind, L)
    _set_beff(groups, mods, B)
    jobs = mask_draw_jobs(groups, mods, B)
    gs = guards.GuardSet(dev)
    bufs = {j["name"]: (gs.out((j["Beff"], j["L"]), torch.float32, name=f"noise {j['name']}"),
                        gs.out((j["Beff"], j["L"]), torch.uint8, name=f"struct {j['name']}")) for j in jobs}
    assert any(j["L"] % 4 for j in jobs) or kind == "folded"
    hip.MaskDraw(jobs, bufs, dev).launch(SEED, 3, ROW_BASE)
    gs.check()
    for n, s in bufs.values():
        assert torch.isfinite(n).all() and int(s.max()) <= 1
    _check_against_reference(groups, mods, B, bufs, SEED, 3, ROW_BASE, f"guarded {kind} L={L} B={B}")


# ------------------------------------------------------------------------------------------------ engine
def _engine(model, B, dev, **kw):  # noqa: N803
    model._engine = None
    return model.engine(B, dev, loss="l2_norm", **kw)


def _token_masks(noise, struct, g):
    """mh_mask_select (include/maestro_hip.h): the k smallest of noise * (1 - struct), ties to the lowest index."""
    order = torch.argsort(noise * (1 - struct.float()), dim=1, stable=True)
    masked = torch.zeros(noise.shape, dtype=torch.bool)
    masked.scatter_(1, order[:, : g.k], True)
    return masked


def _check_engine_draws(eng, step, row_base=0):
    noise, struct = mask_draw_reference(eng.groups, eng.mods, eng.B, eng.mask_seed, step, row_base)
    masks = eng.token_masks()
    for g in eng.groups:
        n, s = _rows_of(noise, g).contiguous(), struct[g.name]
        assert guards.bits_equal(eng.gb[g.name]["noise"].cpu(), n), f"step {step}: noise of {g.name}"
        assert torch.equal(eng.gb[g.name]["struct"].cpu(), s.to(torch.uint8)), f"step {step}: struct of {g.name}"
        assert torch.equal(masks[g.name].cpu(), _token_masks(n, s, g)), f"step {step}: token masks of {g.name}"


@pytest.mark.parametrize("name", list(C.ENGINE_CASES))
def test_engine_draws_are_the_restatement(name, monkeypatch):
    """Four consecutive training forwards: start-up passes + eager run, capture run, two replays."""
    import maestro_amd.engine as E
    dev = _dev()
    model, batch, B = C.build_model(name)  # noqa: N806
    batch = {k: v.to(dev) for k, v in batch.items()}
    monkeypatch.setattr(E, "_PROCESS_WARMED", False)
    eng = _engine(model, B, dev, mask_rng="device", mask_seed=SEED)
    assert eng.mask_rng == "device" and eng.mask_step == 0 and eng.use_graphs
    eng.warm_passes = 2
    for step in range(4):
        eng.forward(batch)
        eng.zero_grad()
        eng.backward()
        torch.cuda.synchronize()
        assert eng.mask_step == step + 1
        _check_engine_draws(eng, step)
    assert eng.warm_passes_run == 2, "the start-up passes did not run: their draws were not exercised"
    assert "forward" in eng._graphs, "the forward was not captured: replays were not exercised"
    eng.mask_step, eng.row_base = 2 ** 32 - 1, ROW_BASE        # settable; the last step a 32-bit counter word can hold
    eng.forward(batch)
    torch.cuda.synchronize()
    _check_engine_draws(eng, 2 ** 32 - 1, ROW_BASE)


def test_the_environment_switch_reaches_the_engine(monkeypatch):
    dev = _dev()
    model, batch, B = C.build_model("group")  # noqa: N806
    monkeypatch.setenv("MAESTRO_MASK_RNG", "device")
    eng = _engine(model, B, dev)
    assert eng.mask_rng == "device" and eng.mask_seed == 0
    assert model.engine(B, dev, loss="l2_norm") is eng
    assert model.engine(B, dev, loss="l2_norm", mask_seed=0) is eng
    other = model.engine(B, dev, loss="l2_norm", mask_seed=1)              # the seed is part of the engine's identity
    assert other is not eng and other.mask_seed == 1 and model.engine(B, dev, loss="l2_norm") is other
    host = model.engine(B, dev, loss="l2_norm", mask_rng="host")
    assert host is not other and host.mask_rng == "host"
    monkeypatch.delenv("MAESTRO_MASK_RNG")
    assert model.engine(B, dev, loss="l2_norm") is host
    other.tie_order = "torch"                                              # assigned after construction: refused at the draw
    with pytest.raises(ValueError, match="tie_order"):
        other.forward({k: v.to(dev) for k, v in batch.items()})


def test_no_pinned_mask_ring_in_device_mode():
    dev = _dev()
    model, batch, B = C.build_model("group")  # noqa: N806
    batch = {k: v.to(dev) for k, v in batch.items()}
    eng = _engine(model, B, dev, mask_rng="device", mask_seed=SEED, deterministic=True)
    for _ in range(2):
        eng.forward(batch)
    torch.cuda.synchronize()
    assert eng._mask_host is None and eng._mask_stage is None and eng._upload_stream is None
    assert not [k for g in eng.groups for k in eng.gb[g.name] if k.endswith("_h")]
    # explicit draws keep the host path for that call (the ring is built then) and leave mask_step alone
    noise, struct = mask_draw_reference(eng.groups, eng.mods, B, SEED, 7, 0)
    loss = eng.forward(batch, noise=noise, struct=struct).clone()
    torch.cuda.synchronize()
    assert eng._mask_host is not None and eng.mask_step == 2
    eng.mask_step = 7
    assert guards.bits_equal(eng.forward(batch).clone(), loss)             # the same draws, made on the device
    host = _engine(model, B, dev, mask_rng="host")
    assert host._mask_host is not None and "noise_h" in host.gb[host.groups[0].name]


@pytest.mark.parametrize("name", ["group", "bg_ts_monotemp"])
def test_nothing_downstream_changes(name):
    """A device-mode engine against a host-mode engine that is handed the restatement's draws: same weights, same batch,
    deterministic mode -> the same loss and gradient bits, eager run, capture run and replay."""
    dev = _dev()
    model, batch, B = C.build_model(name)  # noqa: N806
    batch = {k: v.to(dev) for k, v in batch.items()}
    runs = {}
    for mode in ("device", "host"):
        eng = _engine(model, B, dev, deterministic=True, mask_rng=mode, mask_seed=SEED)
        assert eng.mask_rng == mode and eng.deterministic
        out = []
        for step in range(3):
            draws = {} if mode == "device" else dict(zip(("noise", "struct"), mask_draw_reference(eng.groups, eng.mods, B, SEED, step, 0)))
            loss = eng.forward(batch, **draws)
            eng.zero_grad()
            eng.backward()
            torch.cuda.synchronize()
            out.append((loss.clone(), eng.store.grad.clone()))
        runs[mode] = out
    for step, ((l_d, g_d), (l_h, g_h)) in enumerate(zip(runs["device"], runs["host"])):
        assert torch.isfinite(l_d).all() and float(g_d.abs().max()) > 0
        assert guards.bits_equal(l_d, l_h), f"step {step}: loss {l_d.item()!r} vs {l_h.item()!r}"
        diff = int((g_d.view(torch.int32) != g_h.view(torch.int32)).sum())
        assert diff == 0, f"step {step}: {diff} gradient elements differ in their bits"
    assert not guards.bits_equal(runs["device"][0][0], runs["device"][1][0]), "two steps drew the same masks"


@pytest.mark.parametrize("name", ["group", "ts_shared", "bg_ts_monotemp"])
def test_split_invariance(name):
    """B = 4 at row_base 0 = the concatenation of B = 2 at row_base 0 and 2."""
    dev = _dev()
    model, batch, _ = C.build_model(name, B=4)
    batch = {k: v.to(dev) for k, v in batch.items()}

    def draws(B, row_base, part):  # noqa: N803
        eng = _engine(model, B, dev, mask_rng="device", mask_seed=SEED)
        eng.row_base, eng.mask_step = row_base, 3
        eng.forward({k: v[part] for k, v in batch.items()})
        torch.cuda.synchronize()
        masks = eng.token_masks()
        return {g.name: (eng.gb[g.name]["noise"].cpu().clone(), eng.gb[g.name]["struct"].cpu().clone(), masks[g.name].cpu().clone(),
                         g.Beff // B) for g in eng.groups}

    halves = [draws(2, 0, slice(0, 2)), draws(2, 2, slice(2, 4))]
    whole = draws(4, 0, slice(0, 4))
    for gname, (noise, struct, mask, rows) in whole.items():
        for i, part in enumerate((noise, struct, mask)):
            # folded groups: rows (b, d) -- a sample's rows are adjacent, so the halves concatenate
            cat = torch.cat([h[gname][i] for h in halves])
            assert guards.bits_equal(part, cat) if part.dtype == torch.float32 else torch.equal(part, cat), (gname, i)
        assert noise.shape[0] == 4 * rows


# ------------------------------------------------------------------------------------------------ resume
def test_a_resumed_loop_sees_the_masks_of_the_uninterrupted_one():
    from maestro_amd.train.trainer import PretrainLoop
    dev = _dev()

    def fresh(seed):
        model, batch, B = C.build_model("group", seed=seed)  # noqa: N806
        loop = PretrainLoop(model, B, dev, loss="l2_norm", total_steps=10, mask_rng="device", mask_seed=SEED, deterministic=True)
        return loop, {k: v.to(dev) for k, v in batch.items()}

    loop, batch = fresh(0)
    assert loop.engine.mask_rng == "device" and loop.engine.deterministic and loop.engine.row_base == 0
    losses, sd = [], None
    for step in range(3):
        losses.append(loop.step(batch).clone())
        if step == 0:
            sd = copy.deepcopy(loop.state_dict())
    torch.cuda.synchronize()
    assert sd["mask_step"] == 1 and sd["mask_seed"] == SEED and loop.engine.mask_step == 3
    resumed, _ = fresh(1)                            # other initial weights: everything comes from the state dict
    resumed.load_state_dict(sd)
    assert resumed.engine.mask_step == 1 and resumed.it == 1
    again = [resumed.step(batch).clone() for _ in range(2)]
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(again, losses[1:]), 2):
        assert torch.isfinite(a).all() and guards.bits_equal(a, b), f"step {i}: {a.item()!r} vs {b.item()!r}"
    assert not guards.bits_equal(losses[1], losses[2])
    # host mode keeps exactly today's keys
    model, _, B = C.build_model("group")  # noqa: N806
    host = PretrainLoop(model, B, dev, loss="l2_norm", total_steps=10, mask_rng="host")
    assert sorted(host.state_dict()) == ["exchange_mode", "it", "optimizer", "params", "world"]
    assert sorted(sd) == ["exchange_mode", "it", "mask_seed", "mask_step", "optimizer", "params", "world"]
    host2 = PretrainLoop(model, B, dev, loss="l2_norm", total_steps=10, mask_rng="host", row_base=6)
    assert host2.engine.row_base == 6
