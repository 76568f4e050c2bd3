"""Deterministic mode of the pretraining step (``MAEEngine(deterministic=True)``) on the GPU: parity with the reference under the
existing tolerances, bit-identical repeats (eager run, capture run, graph replays; group streams and one stream), bit-identical
fresh training loops, closeness to the default mode, a ledger of the entry points a deterministic step may not call, and the
refusals."""

from __future__ import annotations

import pytest
import torch

import maestro_amd.conf as conf
from tests import guards
from tests import test_mae_gpu as T

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ (a) parity
@pytest.mark.parametrize("name", list(T.CASES))
def test_goldens_in_deterministic_mode(golden_dir, name, observed, monkeypatch):
    """The 11 reference goldens with the switch on through the environment.  ``_check_case`` assigns ``eng.wgrad_mode``: "fused"
    (in-line split-K atomics in default mode) must not bring the atomics back."""
    monkeypatch.setenv("MAESTRO_DETERMINISTIC", "1")
    T._check_case(golden_dir, name, "fused", observed, f"tiny_det/{name}")


# ------------------------------------------------------------------------------------------------ (b) repeat stability
def _synthetic(dev, B=8):  # noqa: N803
    """The aerial raster at image 64, patch 8 (beside the data set's default Sentinel series).  B = 8: 512 aerial decoder tokens, so the decoder's LayerNorm partial rows (one per 16 tokens)
    span two 16-row chunks of the ordered reduce and its columns more than one 256-column block.  B = 32: 2048 aerial tokens, so
    its pixelify and patch-embed conv weight gradients run as two K-slice slab GEMMs (``hip.det_slices(2048) == 2``)."""
    from maestro_amd.ssl.mae import mae_tiny
    from maestro_amd.train.trainer import synthetic_batch
    ds = conf.DatasetsConfig(name_dataset="treesatai_ts", treesatai_ts=conf.TreeSatAITSConfig(
        filter_targets=[], aerial=conf.InputRasterConfig(image_size=64, patch_size=conf.PatchSizeConfig(mae=8), bands=4,
                                                         norm_bands=[1, 3], norm_fac=255.0)))
    torch.manual_seed(3)
    model = mae_tiny(datasets=ds, mask=conf.MaskConfig(), interpolate="nearest", fusion_mode="group", inter_depth=1, model="mae",
                     num_levels=1, depth=2)
    batch = synthetic_batch(ds.dataset, B, dev, seed=5)
    return model, batch, B


def _case(name, golden_dir, dev):
    if name.startswith("synthetic_"):
        model, batch, B = _synthetic(dev, int(name.split("_")[1]) // 64)  # noqa: N806
        return model, batch, B, None, None
    _, case, _, _, _, model, batch, noise, struct = T._setup(name, golden_dir)
    return model, {k: v.to(dev) for k, v in batch.items()}, case["B"], noise, struct


def _five_steps(eng, batch, noise, struct):
    out = []
    for _ in range(5):
        loss = eng.forward(batch, noise=noise, struct=struct)
        eng.zero_grad()
        eng.backward()
        torch.cuda.synchronize()
        out.append((loss.clone(), eng.store.grad.clone()))
    return out


@pytest.mark.parametrize("name", ["c5_s2naip_stress", "ts_shared", "bg_ts_monotemp", "synthetic_512"])
def test_repeats_are_bit_identical(golden_dir, name):
    dev = _dev()
    model, batch, B, noise, struct = _case(name, golden_dir, dev)  # noqa: N806
    eng = model.engine(B, dev, loss="l2_norm", deterministic=True)
    assert eng.deterministic and eng.use_graphs and eng.multi_stream
    if noise is None:
        torch.manual_seed(11)
        noise, struct = eng.draw_masks()
    runs = _five_steps(eng, batch, noise, struct)          # eager, capture + first replay, three replays
    assert len(eng._graphs) >= 3, "the segments were not captured: replays were not exercised"
    model._engine = None
    one = model.engine(B, dev, loss="l2_norm", deterministic=True)
    assert one is not eng
    one.multi_stream = False
    runs += _five_steps(one, batch, noise, struct)
    loss0, grad0 = runs[0]
    assert torch.isfinite(loss0).all() and float(grad0.abs().max()) > 0
    for i, (loss, grad) in enumerate(runs[1:], 1):
        assert guards.bits_equal(loss, loss0), f"run {i}: loss bits differ ({loss.item()!r} vs {loss0.item()!r})"
        diff = int((grad.view(torch.int32) != grad0.view(torch.int32)).sum())
        assert diff == 0, f"run {i}: {diff} gradient elements differ in their bits"


# ------------------------------------------------------------------------------------------------ (c) fresh loops
def test_fresh_loops_are_bit_identical():
    from maestro_amd.ssl.mae import mae_tiny
    from maestro_amd.train.trainer import PretrainLoop, synthetic_batch
    dev = _dev()
    ds = conf.DatasetsConfig(name_dataset="treesatai_ts", treesatai_ts=conf.TreeSatAITSConfig(
        filter_targets=[], aerial=conf.InputRasterConfig(image_size=60, patch_size=conf.PatchSizeConfig(mae=20), bands=4,
                                                         norm_bands=[1, 3], norm_fac=255.0)))
    batches = [synthetic_batch(ds.dataset, 2, dev, seed=s) for s in (1, 2, 3)]
    flats, losses = [], []
    for _ in range(2):
        torch.manual_seed(0)
        model = mae_tiny(datasets=ds, mask=conf.MaskConfig(), interpolate="nearest", fusion_mode="group", inter_depth=1,
                         model="mae", num_levels=1, depth=2)
        loop = PretrainLoop(model, 2, dev, loss="l2_norm", total_steps=10, deterministic=True)
        assert loop.engine.deterministic
        torch.manual_seed(40)                      # the mask draws of the three steps
        losses.append([loop.step(b).clone() for b in batches])
        torch.cuda.synchronize()
        flats.append(loop.engine.store.flat.clone())
    assert not guards.bits_equal(flats[0], torch.zeros_like(flats[0]))
    assert all(guards.bits_equal(a, b) for a, b in zip(*losses)), "losses differ between two fresh loops"
    diff = int((flats[0].view(torch.int32) != flats[1].view(torch.int32)).sum())
    assert diff == 0, f"{diff} parameters differ in their bits after three optimizer steps"


# ------------------------------------------------------------------------------------------------ (d) closeness
@pytest.mark.parametrize("name", ["c5_s2naip_stress", "synthetic_2048"])
def test_gradients_agree_with_default_mode(golden_dir, name):
    """Deterministic and default gradients of one step differ by summation order only: 1e-5 relative L2 over the flat buffer, the
    bound ``test_gradient_accumulation_sums_micro_batches`` uses for reordered sums.  ``synthetic_2048``: 2048 tokens, the
    smallest size at which the weight gradients outside the stacks are cut into more than one K-slice."""
    from maestro_amd import hip
    dev = _dev()
    model, batch, B, noise, struct = _case(name, golden_dir, dev)  # noqa: N806
    if noise is None:
        assert hip.det_slices(B * 64) == 2
        torch.manual_seed(12)
        noise, struct = model.engine(B, dev, loss="l2_norm", deterministic=False).draw_masks()
    grads, losses = [], []
    for det in (False, True):
        eng = model.engine(B, dev, loss="l2_norm", deterministic=det)
        assert eng.deterministic is det
        losses.append(eng.forward(batch, noise=noise, struct=struct).clone())
        eng.zero_grad()
        eng.backward()
        torch.cuda.synchronize()
        grads.append(eng.store.grad.clone())
    rel = ((grads[0] - grads[1]).double().norm() / grads[0].double().norm()).item()
    print(f"{name}: deterministic vs default: grad rel L2 {rel:.3e}, loss {losses[0].item()!r} vs {losses[1].item()!r}")
    assert rel <= 1e-5, rel
    assert abs(losses[0].item() - losses[1].item()) <= 1e-5 * abs(losses[0].item())
    if name == "synthetic_2048":
        # the slab sites really have two slices here.  Their two weight gradients are also compared one by one, as a GROSS-error
        # check: a lost, doubled or misplaced K-slice changes half of a weight gradient's addends (relative error of order 1) and
        # could hide in the flat buffer's norm, while a reordered fp32 sum moves it by about 1e-6; 1e-2 only has to separate the two.
        sites = {key: bufs["slabs"].shape[0] for key, bufs in eng.sites.items("bwd") if key[0] in ("rec", "embed")}
        assert sites[("rec", "aerial")] == 2 and sites[("embed", "aerial")] == 2, sites
        st, m, checked = eng.store, eng.model, 0
        for s in eng.mods.values():
            for kind, w in (("rec", m.embed_to_rec[s.embed].pixelify_bands[s.gi].conv.weight),
                            ("embed", m.patch_embed[s.embed].patchify_bands[s.gi].conv.weight)):
                if sites[(kind, s.name)] < 2:
                    continue
                o = st.offset[id(w)]
                a, b = grads[0][o: o + w.numel()].double(), grads[1][o: o + w.numel()].double()
                assert float(a.norm()) > 0 and (a - b).norm() <= 1e-2 * a.norm(), (kind, s.name, ((a - b).norm() / a.norm()).item())
                checked += 1
        assert checked >= 2


def test_changing_tie_order_rebuilds_the_mask_token_site(golden_dir):
    """A deterministic engine whose ``tie_order`` changes after a backward: the mask-token sites are rebuilt in place (one site per
    modality), so the buffer of the launch form that no longer runs is not summed into the gradient."""
    dev = _dev()
    _, case, _, _, _, model, batch, noise, struct = T._setup("ties_c3p_dem_s1", golden_dir, table=T.TIE_CASES)
    batch, B = {k: v.to(dev) for k, v in batch.items()}, case["B"]  # noqa: N806

    def step(eng):
        eng.forward(batch, noise=noise, struct=struct)
        eng.zero_grad()
        eng.backward()
        torch.cuda.synchronize()
        return eng.store.grad.clone()

    eng = model.engine(B, dev, loss="l2_norm", deterministic=True)
    eng.use_graphs = False
    step(eng)
    n_sites = len(eng.sites.items("bwd"))
    eng.tie_order = "torch"
    with pytest.warns(RuntimeWarning):
        switched = step(eng)
    assert len(eng.sites.items("bwd")) == n_sites and not [k for k, _ in eng.sites.items("bwd") if k[0] == "tok" and len(k) != 2]
    model._engine = None
    fresh = model.engine(B, dev, loss="l2_norm", deterministic=True)
    fresh.use_graphs, fresh.tie_order = False, "torch"
    assert guards.bits_equal(step(fresh), switched)


# ------------------------------------------------------------------------------------------------ (e) entry-point ledger
FORBIDDEN = ("mh_colsum", "mh_colsum_batched", "mh_layernorm_bwd", "mh_masked_loss", "mh_masked_loss_bands", "mh_unmask_token_grad",
             "mh_unmask_token_grad_per_sample", "mh_embed_finish_bwd")


@pytest.mark.parametrize("name,tie", [("ts_shared", "stable"), ("c5_s2naip_stress", "stable"), ("ties_c3p_dem_s1", "torch")])
def test_deterministic_step_calls_no_atomic_entry_point(golden_dir, name, tie, monkeypatch):
    from maestro_amd import hip
    dev = _dev()
    if name in T.CASES:
        model, batch, B, noise, struct = _case(name, golden_dir, dev)  # noqa: N806
    else:
        _, case, _, _, _, model, batch, noise, struct = T._setup(name, golden_dir, table=T.TIE_CASES)
        batch, B = {k: v.to(dev) for k, v in batch.items()}, case["B"]  # noqa: N806
    calls, gemm_flags, grouped = [], [], []
    call, gemm_tile, grouped_cls = hip.call, hip._gemm_tile, hip.GroupedTN

    def traced_call(entry, *args):
        calls.append(entry)
        return call(entry, *args)

    def traced_gemm_tile(*args):
        gemm_flags.append(args[11])                # (tile, layout, M, N, K, A, lda, B, ldb, C, ldc, flags, ...)
        return gemm_tile(*args)

    class TracedGrouped(grouped_cls):
        def __init__(self, problems, device):
            grouped.append(list(problems))
            super().__init__(problems, device)

    monkeypatch.setattr(hip, "call", traced_call)
    monkeypatch.setattr(hip, "_gemm_tile", traced_gemm_tile)
    monkeypatch.setattr(hip, "GroupedTN", TracedGrouped)
    eng = model.engine(B, dev, loss="l2_norm", deterministic=True)
    eng.tie_order = tie
    eng.wgrad_mode = "fused"
    for _ in range(2):                             # the eager run and the capture run both go through the Python launch code
        eng.forward(batch, noise=noise, struct=struct)
        eng.zero_grad()
        eng.backward()
    torch.cuda.synchronize()
    assert "mh_layernorm_bwd_partial" in calls and ("mh_masked_loss_det" in calls or "mh_masked_loss_bands_det" in calls)
    hit = sorted(set(calls) & set(FORBIDDEN))
    assert not hit, f"a deterministic step called {hit}"
    assert gemm_flags and not [f for f in gemm_flags if f & hip.ATOMIC], "a GEMM ran with the atomic epilogue"
    assert grouped, "no grouped weight-gradient launch was built"
    for problems in grouped:
        dsts = [p[2].data_ptr() for p in problems]
        assert len(dsts) == len(set(dsts)), "a grouped weight-gradient problem would accumulate atomically (shared destination)"


# ------------------------------------------------------------------------------------------------ (f) refusals
def test_refusals(golden_dir):
    from maestro_amd.engine import MAEEngine
    from maestro_amd.train.optim import FusedAdamW
    from maestro_amd.train.trainer import PretrainLoop
    dev = _dev()
    model, batch, B, noise, struct = _case("c1_spot", golden_dir, dev)  # noqa: N806
    with pytest.raises(ValueError, match="fp8"):
        MAEEngine(model, B, dev, dtype="fp8", deterministic=True)
    with pytest.raises(ValueError, match="fp8"):
        model.engine(B, dev, dtype="fp8", deterministic=True)
    with pytest.raises(ValueError, match="overlap_optimizer"):
        PretrainLoop(model, B, dev, deterministic=True, overlap_optimizer=True)
    with pytest.raises(ValueError, match="exchange"):
        PretrainLoop(model, B, dev, deterministic=True, exchange=True)
    with pytest.raises(ValueError, match="deterministic"):
        model.sup_engine(B, dev, "finetune", deterministic=True)
    eng = model.engine(B, dev, loss="l2_norm", deterministic=True)
    with pytest.raises(ValueError, match="gradient hook"):
        eng.grad_hook = lambda lo, hi: None
    assert eng.grad_hook is None
    with pytest.raises(ValueError, match="overlap_optimizer"):
        eng.attach_optimizer(FusedAdamW(eng, 1e-4))
    # tuning cannot come back, whatever is assigned afterwards
    eng.tune_gemm, eng.instep_tune, eng.wgrad_mode = True, True, "fused"
    eng.forward(batch, noise=noise, struct=struct)
    assert eng.tune_gemm is False and eng.instep_tune is False and eng._wgrad_plan() == "all"
    # the flag is part of the engine's identity: a change rebuilds it, no change keeps it
    assert model.engine(B, dev, loss="l2_norm", deterministic=True) is eng
    other = model.engine(B, dev, loss="l2_norm", deterministic=False)
    assert other is not eng and other.deterministic is False
