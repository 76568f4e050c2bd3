"""AdamW parameter groups, the parts that need no GPU: the layer rule (``optim.layer_scale`` / ``layer_groups``) on tiny models of
three fusion modes, ``hip.ParamGroups`` (validation, merging, the map and the tables), the scalar schedule against torch's
per-group ``OneCycleLR``, ``SSLModule.configure_optimizers`` with and without ``lw_decay``, the refusals of the loop and the
optimizer, and the header against the library."""

from __future__ import annotations

import ctypes
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "maestro_hip.h"
NAMES = ["mh_adamw_groups", "mh_adamw_groups_dev"]
R = 0.75

MODELS = {"mod": dict(fusion_mode="mod", inter_depth=1, depth=3),
          "group": dict(fusion_mode="group", inter_depth=0, depth=2),
          "shared": dict(fusion_mode="shared", inter_depth=0, depth=2)}


def _datasets():
    import maestro_amd.conf as conf
    from oracle.gen_golden import build_datasets
    from tests.test_oracle_sup import CASES
    return build_datasets(CASES["sup_treesat_mlc"], conf)


def _model(kind, seed=0):
    import maestro_amd.conf as conf
    from maestro_amd.ssl import mae as pmae
    torch.manual_seed(seed)
    return pmae.mae_tiny(datasets=_datasets(), mask=conf.MaskConfig(), interpolate="nearest", model="mae", num_levels=1,
                         type_head="attentive", **MODELS[kind])


def _cpu_engine(model):
    """What ``layer_groups`` reads of an engine: the model and a flat store in the supervised engine's order (on the CPU)."""
    from maestro_amd.engine import ParamStore
    from maestro_amd.engine_sup import ordered_parameters
    ordered, _ = ordered_parameters(model)
    return SimpleNamespace(model=model, store=ParamStore(ordered, "cpu"))


# ------------------------------------------------------------------------------------------------ the layer rule
@pytest.mark.parametrize("kind", list(MODELS))
def test_layer_rule_per_name(kind):
    from maestro_amd.train.optim import layer_groups, layer_scale
    model = _model(kind)
    eng = _cpu_engine(model)
    st = eng.store
    D, inter = MODELS[kind]["depth"], MODELS[kind]["inter_depth"]  # noqa: N806
    d = D - inter
    assert model.depth == D and (model.encoder_inter is not None) == bool(inter)
    groups = layer_groups(eng, R, 0.05)
    assert groups.total == st.total and groups.group_of.dtype == torch.uint8 and groups.group_of.numel() == st.total // 64
    assert groups.lr_scale.numel() == 256 and groups.wd.numel() == 256 and groups.lr_scale.dtype == torch.float32
    seen = set()
    for name, p in zip(st.names, st.params):
        part = name.split(".")
        if part[0] == "heads":
            want = 1.0
        elif part[0] == "patch_embed":
            want = R ** (D + 1)
        elif part[0] == "encoder" and part[2] == "layers":
            assert 0 <= int(part[3]) < d
            want = R ** (D - int(part[3]))
        elif part[0] == "encoder" and part[2] == "norm":
            want = R ** (D - d)                  # e = d blocks below it
        elif part[0] == "encoder_inter" and part[1] == "layers":
            assert 0 <= int(part[2]) < inter
            want = R ** (D - (d + int(part[2])))
        else:
            assert part[:2] == ["encoder_inter", "norm"], name
            want = 1.0                           # e = D: the last stack
        seen.add(part[0])
        assert layer_scale(name, D, inter, R) == want, name
        o = st.offset[id(p)]
        for i in (o, o + p.numel() - 1, o + (p.numel() + 63) // 64 * 64 - 1):     # first, last, last of the padding
            s, wd = groups.of(i)
            assert s == float(np.float32(want)) and wd == float(np.float32(0.05)), (name, i)
        g = int(groups.group_of[o // 64])
        assert float(groups.lr_scale[g]) == float(np.float32(want)) and bool((groups.group_of[o // 64: (o + p.numel() + 63) // 64] == g).all())
    assert {"heads", "patch_embed", "encoder"} <= seen and ("encoder_inter" in seen) == bool(inter)
    # a stack norm equals its consumer's scale: the first joint block, or -- the last stack -- the heads
    consumer = layer_scale("encoder_inter.layers.0.0.norm.weight", D, inter, R) if inter else layer_scale("heads.x.w", D, inter, R)
    enc = next(iter(model.encoder))
    assert layer_scale(f"encoder.{enc}.norm.weight", D, inter, R) == consumer
    assert layer_scale("encoder_inter.norm.bias", D, inter, R) == 1.0
    # monotone non-decreasing with depth, from the patch embed to the heads
    chain = [layer_scale(f"patch_embed.{enc}.conv.weight", D, inter, R)]
    chain += [layer_scale(f"encoder.{enc}.layers.{i}.0.norm.weight", D, inter, R) for i in range(d)]
    chain += [layer_scale(f"encoder.{enc}.norm.weight", D, inter, R)]
    chain += [layer_scale(f"encoder_inter.layers.{j}.1.net.0.weight", D, inter, R) for j in range(inter)]
    chain += [1.0]
    assert chain == sorted(chain) and chain[0] == R ** (D + 1) and chain[1] == R ** D and chain[-2] <= 1.0
    # unused table entries
    n_used = len(groups.pairs)
    assert n_used == len({float(np.float32(layer_scale(n, D, inter, R))) for n in st.names})
    assert float(groups.lr_scale[n_used:].abs().max()) == 0.0 and float(groups.wd[n_used:].abs().max()) == 0.0
    with pytest.raises(ValueError, match="no parameter"):
        layer_scale("decoder.aerial.layers.0.0.norm.weight", D, inter, R)


def test_no_groups_means_none_and_no_decay_alone_keeps_scale_one():
    from maestro_amd.train.optim import layer_groups
    eng = _cpu_engine(_model("mod"))
    assert layer_groups(eng, None, 0.05) is None and layer_groups(eng, None, 0.05, no_decay_1d=False) is None
    groups = layer_groups(eng, None, 0.05, no_decay_1d=True)
    assert sorted(groups.pairs) == [(1.0, 0.0), (1.0, float(np.float32(0.05)))]
    one = layer_groups(eng, 1.0, 0.05)                        # decay 1: one group, scale 1
    assert one.pairs == [(1.0, float(np.float32(0.05)))] and int(one.group_of.max()) == 0


@pytest.mark.parametrize("kind", list(MODELS))
def test_no_decay_1d_zeroes_wd_exactly_on_the_1d_parameters(kind):
    from maestro_amd.train.optim import layer_groups
    eng = _cpu_engine(_model(kind))
    st = eng.store
    groups = layer_groups(eng, R, 0.05, no_decay_1d=True)
    plain = layer_groups(eng, R, 0.05)
    n1 = 0
    for name, p in zip(st.names, st.params):
        o = st.offset[id(p)]
        s, wd = groups.of(o)
        assert wd == (0.0 if p.ndim <= 1 else float(np.float32(0.05))), name
        assert (s, float(np.float32(0.05))) == plain.of(o), name          # the scales are untouched
        n1 += p.ndim <= 1
    assert 0 < n1 < len(st.params)
    assert any(n.endswith("bias") for n, p in zip(st.names, st.params) if p.ndim <= 1)
    assert any("norm" in n and n.endswith("weight") for n, p in zip(st.names, st.params) if p.ndim <= 1)


# ------------------------------------------------------------------------------------------------ ParamGroups
def test_param_groups_rejections():
    from maestro_amd import hip
    ok = [(0, 64, 1.0, 0.1), (64, 192, 0.5, 0.0)]
    assert hip.ParamGroups(ok, "cpu").total == 192
    with pytest.raises(ValueError, match="aligned"):
        hip.ParamGroups([(0, 60, 1.0, 0.1), (60, 128, 0.5, 0.0)], "cpu")
    with pytest.raises(ValueError, match="aligned"):
        hip.ParamGroups([(0, 64, 1.0, 0.1), (64, 100, 0.5, 0.0)], "cpu")
    with pytest.raises(ValueError, match="gap"):
        hip.ParamGroups([(0, 64, 1.0, 0.1), (128, 192, 0.5, 0.0)], "cpu")
    with pytest.raises(ValueError, match="gap"):
        hip.ParamGroups([(64, 128, 1.0, 0.1)], "cpu")         # does not start at 0
    with pytest.raises(ValueError, match="overlap"):
        hip.ParamGroups([(0, 128, 1.0, 0.1), (64, 192, 0.5, 0.0)], "cpu")
    with pytest.raises(ValueError, match="empty"):
        hip.ParamGroups([(0, 64, 1.0, 0.1), (64, 64, 0.5, 0.0)], "cpu")
    with pytest.raises(ValueError, match="no spans"):
        hip.ParamGroups([], "cpu")
    with pytest.raises(ValueError, match="non-finite"):
        hip.ParamGroups([(0, 64, float("nan"), 0.1)], "cpu")
    many = [(64 * k, 64 * (k + 1), 1.0 / (k + 1), 0.0) for k in range(257)]
    with pytest.raises(ValueError, match="257 distinct"):
        hip.ParamGroups(many, "cpu")
    assert len(hip.ParamGroups(many[:256], "cpu").pairs) == 256
    g = hip.ParamGroups(ok, "cpu")
    for bad in (1, 63, 65, -64, 192, 256):
        with pytest.raises(ValueError, match="map_at"):
            g.map_at(bad)
    assert g.map_at(0).numel() == 3 and g.map_at(64).tolist() == [1, 1] and g.map_at(128).data_ptr() == g.group_of.data_ptr() + 2


def test_param_groups_merge_equal_pairs():
    from maestro_amd import hip
    spans = [(256, 320, 0.75, 0.0), (0, 64, 0.75, 0.05), (64, 192, 1.0, 0.05), (192, 256, 0.75, 0.05),      # any order
             (320, 384, float(np.float32(0.75)) + 1e-12, 0.0)]                                            # equal AS fp32
    g = hip.ParamGroups(spans, "cpu")
    assert g.pairs == [(0.75, float(np.float32(0.05))), (1.0, float(np.float32(0.05))), (0.75, 0.0)]
    assert g.group_of.tolist() == [0, 1, 1, 0, 2, 2] and g.spans == [(0, 64, 0), (64, 192, 1), (192, 256, 0), (256, 320, 2), (320, 384, 2)]
    assert g.lr_scale[:3].tolist() == [0.75, 1.0, 0.75] and g.wd[:3].tolist() == [float(np.float32(0.05))] * 2 + [0.0]
    assert g.lr_scale.numel() == g.wd.numel() == 256 and float(g.lr_scale[3:].abs().max()) == 0.0 and float(g.wd[3:].abs().max()) == 0.0
    assert g.of(0) == g.of(255) != g.of(64) and g.total == 384
    same = hip.ParamGroups([(64 * k, 64 * (k + 1), 0.5, 0.01) for k in range(300)], "cpu")       # 300 spans, ONE pair
    assert len(same.pairs) == 1 and int(same.group_of.max()) == 0


def test_wrappers_check_map_and_tables_before_any_launch():
    from maestro_amd import hip
    z = torch.zeros(128)
    tab, gmap = torch.zeros(256), torch.zeros(2, dtype=torch.uint8)
    with pytest.raises(hip.HipExtensionError, match="ceil"):
        hip.adamw_groups(z, z, z, z, None, gmap[:1], tab, tab, 128, 1e-3, 0.9, 0.99, 1e-8, 1)
    with pytest.raises(hip.HipExtensionError, match="256 entries"):
        hip.adamw_groups(z, z, z, z, None, gmap, tab[:255], tab, 128, 1e-3, 0.9, 0.99, 1e-8, 1)
    with pytest.raises(hip.HipExtensionError, match="256 entries"):
        hip.adamw_groups_dev(z, z, z, z, None, gmap, tab, torch.zeros(257), 128, 0.9, 0.99, 1e-8, torch.zeros(5))
    with pytest.raises(hip.HipExtensionError, match="uint8"):
        hip.adamw_groups(z, z, z, z, None, gmap.to(torch.int32), tab, tab, 128, 1e-3, 0.9, 0.99, 1e-8, 1)
    with pytest.raises(hip.HipExtensionError, match="GPU"):           # CPU tensors: no fallback
        hip.adamw_groups(z, z, z, z, None, gmap, tab, tab, 128, 1e-3, 0.9, 0.99, 1e-8, 1)


# ------------------------------------------------------------------------------------------------ the schedule
def test_scalar_onecycle_times_scale_is_torchs_per_group_onecycle():
    """``OneCycleLR`` is linear in ``max_lr``: per group and step, torch's rate equals ``OneCycle.lr(t) * scale_g`` to 1e-12."""
    from maestro_amd.train.optim import OneCycle
    lr, total, final_factor = 3.7e-4, 40, 1e7
    scales = [R ** k for k in (13, 12, 7, 1, 0)]
    params = [{"params": [torch.nn.Parameter(torch.zeros(1))], "lr": lr * s} for s in scales]
    opt = torch.optim.AdamW(params, lr=lr)
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=[lr * s for s in scales], total_steps=total, pct_start=0.2,
                                                cycle_momentum=False, div_factor=1000, final_div_factor=final_factor / 1000.0)
    ours = OneCycle(lr, total, pct_start=0.2, div_factor=1000.0, final_div_factor=final_factor / 1000.0)
    boundary = int(ours.end1)                  # the last step of the warm-up phase
    checked = 0
    for t in range(total):
        if t in (0, 1, boundary - 1, boundary, boundary + 1, total // 2, total - 2, total - 1):
            for g, s in zip(opt.param_groups, scales):
                want = ours.lr(t) * s
                assert abs(g["lr"] - want) <= 1e-12 * want, (t, s, g["lr"], want)
            checked += 1
        opt.step()
        if t < total - 1:
            sched.step()
    assert checked == 8 and boundary == 7


def _trainer(**kw):
    return SimpleNamespace(train_dataloader=SimpleNamespace(batch_size=4), accumulate_grad_batches=1, num_nodes=1, num_devices=1,
                           base_lr=3e-3, wd=0.05, b1=0.9, b2=0.99, estimated_stepping_batches=40, final_factor=1e7, **kw)


def _module(kind="mod", seed=0):
    import maestro_amd.conf as conf
    from maestro_amd.train.model import SSLModule
    torch.manual_seed(seed)
    return SSLModule(datasets=_datasets(), mask=conf.MaskConfig(), interpolate="nearest", fusion_mode=MODELS[kind]["fusion_mode"],
                     inter_depth=MODELS[kind]["inter_depth"], model="mae", model_size="tiny", type_head="attentive", loss="l2_norm")


def test_configure_optimizers_with_lw_decay_yields_the_rules_groups():
    from maestro_amd.train.optim import EngineAdamW, layer_group_name, layer_scale
    module = _module("mod")
    m = module.model
    D, inter = m.depth, m.inter_depth  # noqa: N806
    assert (D, inter) == (12, 1)
    module.trainer = _trainer(ssl_phase="finetune", lw_decay=R)
    cfg = module.configure_optimizers()
    opt, sched = cfg["optimizer"], cfg["lr_scheduler"]["scheduler"]
    assert isinstance(opt, EngineAdamW) and cfg["lr_scheduler"]["name"] == "finetune_AdamW_lr"
    lr = 3e-3 * (4 / 3.0) ** 0.5
    names = [g["name"] for g in opt.param_groups]
    assert names[-1] == "heads" and names[-2] == "other" and len(set(names)) == len(names)
    mods = list(m.patch_embed)
    want = {f"patch_embed.{k}": R ** (D + 1) for k in mods}
    for k in m.encoder:
        want.update({f"encoder.{k}.{i}": R ** (D - i) for i in range(D - inter)})
        want[f"encoder.{k}.norm"] = R ** (D - (D - inter))
    want.update({f"encoder_inter.{j}": R ** (D - (D - inter + j)) for j in range(inter)})
    want.update({"encoder_inter.norm": 1.0, "other": 1.0, "heads": 1.0})
    assert set(names) == set(want)
    assert sched.optimizer is opt
    for g in opt.param_groups:
        assert g["max_lr"] == lr * want[g["name"]] and g["initial_lr"] == g["max_lr"] / 1000, g["name"]
        assert abs(g["lr"] - g["initial_lr"]) <= 1e-12 * g["initial_lr"]          # (the scheduler's first value: its cosine at 0)
        assert g["weight_decay"] == 0.05 and g["betas"] == (0.9, 0.99)
    # every parameter once, in the group its name says
    by_id = {id(p): g["name"] for g in opt.param_groups for p in g["params"]}
    named = [(n, p) for n, p in module.named_parameters() if n != "_anchor"]
    assert len(by_id) == len(named) == sum(len(g["params"]) for g in opt.param_groups)
    for n, p in named:
        inner = n.split(".", 1)[1]
        if n.startswith("model.") and inner.split(".")[0] in ("patch_embed", "encoder", "encoder_inter", "heads"):
            assert by_id[id(p)] == layer_group_name(inner), n
            assert want[by_id[id(p)]] == layer_scale(inner, D, inter, R)
        else:
            assert by_id[id(p)] == "other", n
    # out of finetune, or with the attribute None, the one group of before
    for tr in (_trainer(ssl_phase="pretrain", lw_decay=R), _trainer(ssl_phase="finetune", lw_decay=None)):
        module.trainer = tr
        assert len(module.configure_optimizers()["optimizer"].param_groups) == 1
    module.trainer = _trainer(ssl_phase="finetune", lw_decay=1.5)
    with pytest.raises(ValueError, match="lw_decay"):
        module.configure_optimizers()


def test_configure_optimizers_without_the_attribute_is_the_single_group():
    module = _module("group")
    module.trainer = _trainer(ssl_phase="finetune")              # existing callers' namespaces carry no lw_decay
    cfg = module.configure_optimizers()
    opt = cfg["optimizer"]
    lr = 3e-3 * (4 / 3.0) ** 0.5
    assert len(opt.param_groups) == 1 and "name" not in opt.param_groups[0]
    g = opt.param_groups[0]
    assert g["max_lr"] == lr and g["weight_decay"] == 0.05
    assert len(g["params"]) == len([n for n, _ in module.named_parameters() if n != "_anchor"])


def test_engine_adamw_expresses_proportional_groups_only():
    """The host side of the several-group eligibility: one base rate and constant scales, agreeing betas / eps."""
    from maestro_amd.train.optim import EngineAdamW
    w = [torch.nn.Parameter(torch.ones(64)), torch.nn.Parameter(torch.ones(64))]
    eng = SimpleNamespace(store=SimpleNamespace(params=w, offset={id(w[0]): 0, id(w[1]): 64}, total=128, fresh=False))
    opt = EngineAdamW([{"params": [w[0]], "lr": 0.075}, {"params": [w[1]]}], lambda: eng, lr=0.1)
    assert opt._groups_expressible(eng)
    opt._bound, opt._scales = eng, [(0.75, 0.01), (1.0, 0.01)]
    assert opt._groups_expressible(eng)
    for g in opt.param_groups:                                    # the whole schedule moves: the ratio holds
        g["lr"] *= 0.123
    assert opt._groups_expressible(eng)
    opt.param_groups[0]["lr"] *= 1.0 + 1e-5                        # one group leaves it
    assert not opt._groups_expressible(eng)
    opt.param_groups[0]["lr"] = opt.param_groups[1]["lr"] * 0.75
    opt.param_groups[0]["weight_decay"] = 0.0                      # a changed weight decay is not what was bound
    assert not opt._groups_expressible(eng)
    opt.param_groups[0]["weight_decay"] = 0.01
    assert opt._groups_expressible(eng)
    opt.param_groups[0]["betas"] = (0.8, 0.99)
    assert not opt._groups_expressible(eng)
    opt.param_groups[0]["betas"] = opt.param_groups[1]["betas"]
    opt.param_groups[1]["lr"] = 0.0                                # no base rate to scale
    assert not opt._groups_expressible(eng)
    opt.param_groups[1]["lr"] = 0.1
    eng.fp8 = object()                                             # mh_adamw_fp8 has no grouped form
    assert not opt._groups_expressible(eng)


# ------------------------------------------------------------------------------------------------ the refusals
def test_loop_refusals(monkeypatch):
    """All ValueErrors raised before anything is built (the model is None: what follows an accepted configuration is the
    AttributeError of building an engine from it)."""
    from maestro_amd.train.optim import resolve_lw_decay
    from maestro_amd.train.trainer import SupervisedLoop
    for v in ("MAESTRO_LW_DECAY", "MAESTRO_MAX_GRAD_NORM", "MAESTRO_SKIP_NONFINITE"):
        monkeypatch.delenv(v, raising=False)
    with pytest.raises(ValueError, match="probe"):
        SupervisedLoop(None, 1, "cpu", phase="probe", lw_decay=0.75)
    for bad in (0.0, -0.5, 1.5, float("nan"), float("inf"), "0.75", True):
        with pytest.raises(ValueError, match="lw_decay"):
            SupervisedLoop(None, 1, "cpu", lw_decay=bad)
    for ok in (dict(lw_decay=0.75), dict(lw_decay=1.0), dict(no_decay_1d=True), dict(lw_decay=0.5, no_decay_1d=True),
               dict(phase="probe", no_decay_1d=True), dict()):
        with pytest.raises(AttributeError):
            SupervisedLoop(None, 1, "cpu", **ok)
    assert resolve_lw_decay() is None and resolve_lw_decay(0.75) == 0.75 and resolve_lw_decay(1) == 1.0
    monkeypatch.setenv("MAESTRO_LW_DECAY", "")
    assert resolve_lw_decay() is None
    monkeypatch.setenv("MAESTRO_LW_DECAY", "0.8")
    assert resolve_lw_decay() == 0.8 and resolve_lw_decay(0.5) == 0.5          # an explicit value wins
    with pytest.raises(ValueError, match="probe"):
        SupervisedLoop(None, 1, "cpu", phase="probe")
    for bad in ("2", "0", "-1", "nan", "abc"):
        monkeypatch.setenv("MAESTRO_LW_DECAY", bad)
        with pytest.raises(ValueError, match="lw_decay"):
            SupervisedLoop(None, 1, "cpu")


def _stub_engine(**kw):
    flat = torch.zeros(128)
    return SimpleNamespace(store=SimpleNamespace(flat=flat, grad=flat.clone(), half=flat.bfloat16(), total=128), **kw)


def test_fused_adamw_refuses_groups_with_fp8_and_with_step_sharded():
    from maestro_amd import hip
    from maestro_amd.train.optim import FusedAdamW, refuse_group_conflicts
    groups = hip.ParamGroups([(0, 64, 0.75, 0.0), (64, 128, 1.0, 0.05)], "cpu")
    opt = FusedAdamW(_stub_engine(fp8=object()), 1e-3, groups=groups)
    with pytest.raises(ValueError, match="fp8"):
        opt.step()
    with pytest.raises(ValueError, match="fp8"):
        opt.step(guard=SimpleNamespace(n=128))
    assert opt.t == 0
    opt = FusedAdamW(_stub_engine(), 1e-3, groups=groups)
    with pytest.raises(ValueError, match="step_sharded"):
        opt.step_sharded(SimpleNamespace())                       # before the exchange plan is even looked at
    with pytest.raises(ValueError, match="128"):
        FusedAdamW(_stub_engine(), 1e-3, groups=hip.ParamGroups([(0, 64, 1.0, 0.0)], "cpu"))
    assert FusedAdamW(_stub_engine(), 1e-3).groups is None
    refuse_group_conflicts(False, dtype="fp8", sharded=True)       # without groups nothing is refused
    assert sorted(FusedAdamW(_stub_engine(), 1e-3, groups=groups).state_dict()) == \
        sorted(FusedAdamW(_stub_engine(), 1e-3).state_dict())     # the state-dict layout is the ungrouped one


# ------------------------------------------------------------------------------------------------ header + ABI
@pytest.fixture(scope="module")
def lib():
    from maestro_amd.csrc.build import LIB, build
    if not LIB.exists():
        build()
    handle = ctypes.CDLL(str(LIB))
    handle.mh_last_error.restype = ctypes.c_char_p
    return handle


def test_library_exports_what_the_header_declares(lib):
    import inspect

    from maestro_amd import hip
    from maestro_amd.csrc import build as B
    text = HEADER.read_text()
    assert sorted(p.name for p in (ROOT / "include").iterdir()) == ["maestro_hip.h"]
    assert not [n for n in NAMES if not re.search(rf"^int {n}\(", text, re.M)]
    assert not [n for n in NAMES if not hasattr(lib, n)]
    for cite in ("maestro/conf/opt.py:51", "maestro/train/trainer.py:43-52", "maestro/train/baseline.py:110-131",
                 "maestro/baselines/dinov2.py:312-373"):
        assert cite in text, cite
    assert f"#define MH_ADAMW_GROUP_BLOCK {hip.GROUP_BLOCK}" in text and f"#define MH_ADAMW_GROUP_TABLE {hip.GROUP_TABLE}" in text
    assert '"maestro_hip.h"' in inspect.getsource(B._digest) and inspect.getsource(B._digest).count("maestro_hip") == 1
    optim = (B.CSRC / "optim.hip").read_text()
    assert '#include "../../include/maestro_hip.h"' in optim and not [n for n in NAMES if f'extern "C" int {n}(' not in optim]


def test_bad_arguments_are_refused_before_the_gpu_is_touched(lib):
    """Device pointers are never dereferenced on the host and a refused call launches nothing: any non-null value will do."""
    vp, cl, cf, ci = ctypes.c_void_p, ctypes.c_long, ctypes.c_float, ctypes.c_int
    lib.mh_adamw_groups.argtypes = [vp] * 8 + [cl, cf, cf, cf, cf, ci, cf, vp]
    lib.mh_adamw_groups_dev.argtypes = [vp] * 8 + [cl, cf, cf, cf, vp, vp]

    def by_value(p=0x1000, g=0x2000, m=0x3000, v=0x4000, pb=0x5000, gm=0x6001, ls=0x7000, wd=0x8000, n=64, step=1):
        return lib.mh_adamw_groups(p, g, m, v, pb, gm, ls, wd, n, 1e-3, 0.9, 0.99, 1e-8, step, 1.0, None)

    def by_dev(p=0x1000, g=0x2000, m=0x3000, v=0x4000, pb=0x5000, gm=0x6001, ls=0x7000, wd=0x8000, n=64, h=0x9000):
        return lib.mh_adamw_groups_dev(p, g, m, v, pb, gm, ls, wd, n, 0.9, 0.99, 1e-8, h, None)

    for call in (by_value, by_dev):
        for null in ("p", "g", "m", "v"):
            assert call(**{null: 0}) == -1 and b"bad arguments" in lib.mh_last_error()
        for null in ("gm", "ls", "wd"):
            assert call(**{null: 0}) == -1 and b"null" in lib.mh_last_error()
        for n in (0, -4, 6, 63):
            assert call(n=n) == -1 and b"n % 4" in lib.mh_last_error(), n
        for mis in (dict(p=0x1004), dict(g=0x2008), dict(m=0x3004), dict(v=0x400c), dict(pb=0x5004)):
            assert call(**mis) == -1 and b"aligned" in lib.mh_last_error(), mis
    assert by_value(step=0) == -1 and b"step >= 1" in lib.mh_last_error()
    assert by_dev(h=0) == -1 and b"bad arguments" in lib.mh_last_error()
