"""Scene prediction on the GPU: ``mh_window_gather`` against torch slicing, ``mh_predict_blend`` / ``mh_predict_blend_finish``
against ``hip.scene_blend_reference`` / ``hip.scene_finish_reference``, and ``SupervisedEngine.predict_scene`` against per-window
``predict`` calls fed to that reference -- all bit for bit: the gather is data movement and the blend's sum order is specified.

Kernel operands sit in the poisoned allocations of tests/guards.py; every size and index passed is in range.  Shapes are the
smallest at which each path can go wrong: 16-byte and 4-byte paths of the gather, window columns that are no multiple of 4, a
window of more than one workgroup, more slots than one wave lists at once, pad slots, equal windows, two scenes in one batch."""

import functools
import os

import numpy as np
import pytest
import torch

from maestro_amd import hip
from tests.guards import GuardSet, bits_equal

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
I32 = torch.int32


# ----------------------------------------------------------------------------------------------------- guard bands (tests/guards.py)
def gather_call(scene, rows, S, q, align=16):  # noqa: N803
    gs = GuardSet(DEV)
    N, planes, Hs, Ws = scene.shape  # noqa: N806
    B = len(rows)  # noqa: N806
    d_scene = gs.inp(scene, align=align, name="scene")
    d_tab = gs.inp(torch.tensor(rows, dtype=I32), name="table")
    out = gs.out((B, planes, S, S), align=align, name="out")
    hip.window_gather(d_scene, out, d_tab, np.asarray(rows, dtype=np.int32), B, N, planes, Hs, Ws, S, q)
    gs.check()
    return out.cpu()


def blend_call(prob, scale, profile, rows, acc, wsum, q):
    """``hip.predict_blend`` on guarded operands; ``acc`` / ``wsum``: the canvas so far (CPU).  Returns the new CPU ``(acc, wsum)``."""
    gs = GuardSet(DEV)
    B, C, S, _ = prob.shape  # noqa: N806
    N, _, Hc, Wc = acc.shape  # noqa: N806
    d_prob = gs.inp(prob, name="prob")
    d_prof = gs.inp(torch.from_numpy(profile), name="profile")
    d_tab = gs.inp(torch.tensor(rows, dtype=I32), name="table")
    d_acc, d_wsum = gs.out(acc.shape, name="acc"), gs.out(wsum.shape, name="wsum")
    d_acc.copy_(acc)
    d_wsum.copy_(wsum)
    gs.arm()
    hip.predict_blend(d_prob, scale, d_prof, d_tab, np.asarray(rows, dtype=np.int32), d_acc, d_wsum, B, N, C, S, q, Hc, Wc)
    gs.check()
    return d_acc.cpu(), d_wsum.cpu()


def finish_call(acc, wsum, outputs=("cls", "conf", "mean"), alias=False):
    gs = GuardSet(DEV)
    N, C, n_pix = acc.shape  # noqa: N806
    d_wsum = gs.inp(wsum, name="wsum")
    if alias:
        d_acc = gs.out(acc.shape, name="acc")
        d_acc.copy_(acc)
        gs.arm()
    else:
        d_acc = gs.inp(acc, name="acc")
    cls = gs.out((N, n_pix), dtype=torch.uint8, align=4, name="cls") if "cls" in outputs else None
    conf = gs.out((N, n_pix), align=4, name="conf") if "conf" in outputs else None
    mean = d_acc if alias else (gs.out(acc.shape, align=4, name="mean") if "mean" in outputs else None)
    hip.predict_blend_finish(d_acc, d_wsum, cls, conf, mean, N, C, n_pix)
    gs.check()
    return tuple(None if t is None else t.cpu() for t in (cls, conf, mean))


# ----------------------------------------------------------------------------------------------------- gather
@pytest.mark.parametrize("align", [16, 4])
@pytest.mark.parametrize("planes", [1, 3])
@pytest.mark.parametrize("S", [5, 16])
@pytest.mark.parametrize("q", [1, 5, 32])
def test_window_gather_equals_torch_slicing(q, S, planes, align):  # noqa: N803
    N, Hs, Ws = 2, 3 * q + S, 4 * q + S  # noqa: N806
    scene = torch.arange(N * planes * Hs * Ws, dtype=torch.float32).reshape(N, planes, Hs, Ws) + 0.5
    rows = [(0, 0, 0, 1), (1, 3, 4, 1),           # a window that ends exactly at the scene's last row and column
            (1, 1, 2, 1), (1, 1, 2, 1),           # two equal windows
            (0, 2, 1, 0),                         # a pad slot: gathered like any other
            (0, 1, 3, 1)]
    out = gather_call(scene, rows, S, q, align=align)
    for b, (n, y0, x0, _) in enumerate(rows):
        assert bits_equal(out[b], scene[n, :, y0 * q: y0 * q + S, x0 * q: x0 * q + S]), (b, n, y0, x0)


# ----------------------------------------------------------------------------------------------------- blend
def _canvas(N, C, Hc, Wc, rows_list, S, q, seed):  # noqa: N803
    """A canvas with finite random values where some window of ``rows_list`` will land and NaN poison everywhere else."""
    g = torch.Generator().manual_seed(seed)
    acc, wsum = torch.rand(N, C, Hc, Wc, generator=g), torch.rand(N, Hc, Wc, generator=g) + 0.5
    hit = torch.zeros(N, Hc, Wc, dtype=torch.bool)
    for rows in rows_list:
        for n, y0, x0, on in rows:
            if on:
                hit[n, y0 * q: y0 * q + S, x0 * q: x0 * q + S] = True
    acc[~hit[:, None].expand_as(acc)] = float("nan")
    wsum[~hit] = float("nan")
    return acc, wsum, hit


def _check_blend(prob, scale, profile, rows, acc, wsum, q):
    got = blend_call(prob, scale, profile, rows, acc, wsum, q)
    want = hip.scene_blend_reference(prob.numpy(), scale, profile, rows, q, acc.numpy(), wsum.numpy())
    for name, g, w in zip(("acc", "wsum"), got, want):
        assert bits_equal(g, torch.from_numpy(w)), f"{name}: {int((g.view(I32) != torch.from_numpy(w).view(I32)).sum())} elements differ"
    return got


@pytest.mark.parametrize("kind", ["linear", "flat"])
@pytest.mark.parametrize("C", [2, 19])
@pytest.mark.parametrize("S", [4, 6, 16, 40])
def test_blend_equals_the_reference(S, C, kind):  # noqa: N803
    """W = 2 units, stride 1: the four windows of scene 0 overlap each other; pad slots in the middle and at the end; scene 1 in the
    same batch; then a launch of B = 1 onto the canvas the first left; NaN poison wherever no window lands."""
    q, N = S // 2, 2  # noqa: N806
    Hc, Wc = 3 * q, 4 * q  # noqa: N806
    first = [(0, 0, 0, 1), (0, 0, 1, 1), (1, 1, 1, 0), (0, 1, 0, 1), (0, 1, 1, 1), (1, 0, 0, 1), (1, 0, 0, 0)]
    second = [(1, 0, 1, 1)]
    third = [(0, 1, 2, 1), (0, 1, 2, 1), (0, 1, 2, 0), (1, 1, 0, 1)]          # two equal windows: both are added, in slot order
    acc, wsum, hit = _canvas(N, C, Hc, Wc, [first, second, third], S, q, seed=S * C)
    assert not hit.all() and hit.any()
    profile = hip.blend_profile(S, kind)
    g = torch.Generator().manual_seed(7 + S + C)
    for rows, scale in ((first, 1.0), (second, 1.0 / 3.0), (third, 0.125)):
        prob = torch.rand(len(rows), C, S, S, generator=g)
        acc, wsum = _check_blend(prob, scale, profile, rows, acc, wsum, q)
    assert bool(torch.isnan(acc[~hit[:, None].expand_as(acc)]).all()) and bool(torch.isnan(wsum[~hit]).all())
    assert bool(torch.isfinite(wsum[hit]).all())


def test_blend_does_not_depend_on_the_batch_size():
    """64 windows (more than one wave lists at once, with the pads), fed as one launch of B = 70 and as batches of 7."""
    S, q, C, U, W = 4, 2, 3, 9, 2  # noqa: N806
    wins = hip.scene_windows(U, U, W, 1)
    assert len(wins) == 64
    profile = hip.blend_profile(S, "linear")
    prob = torch.rand(70, C, S, S, generator=torch.Generator().manual_seed(3))
    zero = torch.zeros(1, C, U * q, U * q), torch.zeros(1, U * q, U * q)
    one = _check_blend(prob, 1.0, profile, hip.scene_table(1, wins, 70)[0].tolist(), *zero, q)
    acc, wsum = zero
    batches = hip.scene_table(1, wins, 7)
    assert batches.shape == (10, 7, 4) and batches[-1, :, 3].tolist() == [1, 0, 0, 0, 0, 0, 0]
    for i, rows in enumerate(batches.tolist()):          # (rows 64 .. 69 of prob sit in pad slots both times)
        acc, wsum = _check_blend(prob[i * 7: (i + 1) * 7], 1.0, profile, rows, acc, wsum, q)
    assert bits_equal(acc, one[0]) and bits_equal(wsum, one[1])
    assert bool((wsum > 0).all())


# ----------------------------------------------------------------------------------------------------- finish
@pytest.mark.parametrize("alias", [False, True])
@pytest.mark.parametrize("C", [2, 19])
def test_finish_equals_the_reference(C, alias):  # noqa: N803
    N, n_pix = 2, 37  # noqa: N806
    g = torch.Generator().manual_seed(C)
    acc = torch.rand(N, C, n_pix, generator=g)
    wsum = torch.rand(N, n_pix, generator=g) + 0.25
    acc[0, :, 1] = 0.5                                   # an exact tie over all classes -> class 0
    acc[0, C - 1, 2] = acc[0, 0, 2] = 2.0               # the first and the last class tie -> 0
    acc[1, C - 1, 3] = float("nan")                     # a NaN is the maximum
    acc[1, :, 4] = float("nan")                         # the first NaN wins
    wsum[0, 5] = wsum[1, 36] = 0.0                      # no window reached the pixel
    acc[1, :, 6] = 0.0
    cls, conf, mean = finish_call(acc, wsum, alias=alias)
    wc, wf, wm = hip.scene_finish_reference(acc.numpy(), wsum.numpy())
    assert torch.equal(cls, torch.from_numpy(wc)) and bits_equal(conf, torch.from_numpy(wf)) and bits_equal(mean, torch.from_numpy(wm))
    assert cls[0, 1] == 0 and cls[0, 2] == 0 and cls[1, 3] == C - 1 and cls[1, 4] == 0 and cls[1, 6] == 0
    assert cls[0, 5] == cls[1, 36] == hip.SCENE_UNCOVERED and conf[0, 5] == 0 and bool((mean[1, :, 36] == 0).all())
    if not alias:                                        # every output alone
        for k, want in (("cls", cls), ("conf", conf), ("mean", mean)):
            got = dict(zip(("cls", "conf", "mean"), finish_call(acc, wsum, outputs=(k,))))
            assert bits_equal(got[k], want) and all(v is None for kk, v in got.items() if kk != k)


# ----------------------------------------------------------------------------------------------------- engine
@functools.lru_cache(maxsize=None)
def _engine(name):
    from tests.test_sup_gpu import _setup
    dev, case, ds, oracle, model, batch = _setup(name)
    eng = model.sup_engine(case["B"], dev, "finetune")
    return eng, ds, {k: v.to(dev) for k, v in batch.items()}


def _sources(eng):
    return [parts[0] for parts in eng.model.src_specs.values()]


def _scene(eng, dbatch, N, Hu, Wu):  # noqa: N803
    """``N`` scenes of ``Hu x Wu`` units: the golden windows tiled over the scene (every modality at its own pixel scale), each tile
    scaled differently so that no two windows see the same data; the golden dates."""
    geo = eng.scene_geometry()
    W = geo["W"]  # noqa: N806
    scene = {"ref_date": dbatch["ref_date"][:N].contiguous()}
    ty, tx = -(-Hu // W), -(-Wu // W)
    for s in _sources(eng):
        q = geo["q"][s.src]
        img = dbatch[s.src][:N]
        tiles = torch.cat([torch.cat([img * (1.0 + 0.0625 * ((3 * i + j) % 5)) for j in range(tx)], dim=-1) for i in range(ty)], dim=-2)
        scene[s.src] = tiles[..., : Hu * q, : Wu * q].contiguous()
        scene[f"{s.src}_dates"] = dbatch[f"{s.src}_dates"][:N].contiguous()
    return scene


def _window_batch(eng, scene, rows):
    """The batch of one table batch cut with torch, in the planner's slot order."""
    geo = eng.scene_geometry()
    n_idx = torch.tensor([r[0] for r in rows], device=DEV)
    batch = {"ref_date": scene["ref_date"][n_idx].contiguous()}
    for s in _sources(eng):
        q = geo["q"][s.src]
        batch[s.src] = torch.stack([scene[s.src][n, :, :, y0 * q: y0 * q + s.S, x0 * q: x0 * q + s.S] for n, y0, x0, _ in rows]).contiguous()
        batch[f"{s.src}_dates"] = scene[f"{s.src}_dates"][n_idx].contiguous()
    return batch


def _per_window(eng, scene, table, views):
    """``{target: [(cls, conf, probs) per slot, CPU]}`` of ``eng.predict`` on every batch of ``table``, pad slots included."""
    out = {t: [] for t in eng.hb}
    for rows in table.tolist():
        pred = eng.predict(_window_batch(eng, scene, rows), views=views, probs=True)
        torch.cuda.synchronize()
        for t, p in pred.items():
            out[t] += [tuple(x[b].cpu().clone() for x in p) for b in range(eng.B)]
    return out


def _plan(eng, scene, stride):
    geo = eng.scene_geometry()
    first = _sources(eng)[0]
    N, Hu, Wu = scene[first.src].shape[0], scene[first.src].shape[3] // geo["q"][first.src], scene[first.src].shape[4] // geo["q"][first.src]  # noqa: N806
    wins = hip.scene_windows(Hu, Wu, geo["W"], stride)
    return geo, N, Hu, Wu, wins, hip.scene_table(N, wins, eng.B)


def _cpu(out):
    torch.cuda.synchronize()
    return {t: tuple(None if x is None else x.cpu().clone() for x in p) for t, p in out.items()}


def _same(a, b):
    return all((x is None and y is None) or bits_equal(x, y) for t in a for x, y in zip(a[t], b[t]))


GEOMETRY = {"sup_flair_seg": dict(W=2, q={"aerial": 32, "s2": 5}, qt={"cosia": 128}),
            "sup_pastis_two": dict(W=16, q={"s2": 1, "s1_asc": 1}, qt={"pastis_seg": 1})}


@pytest.mark.parametrize("name", list(GEOMETRY))
def test_engine_geometry(name):
    eng, _, _ = _engine(name)
    assert eng.scene_geometry() == GEOMETRY[name]


@pytest.mark.parametrize("views", [(0,), "d4"], ids=["identity", "d4"])
@pytest.mark.parametrize("name", list(GEOMETRY))
def test_engine_one_window_scenes_equal_predict(name, views):
    """(a) The golden batch as ``B`` scenes of one window each, flat profile: the canvas IS the prediction of ``predict``."""
    eng, ds, dbatch = _engine(name)
    nolabel = {k: v for k, v in dbatch.items() if k not in ds.dataset.targets}
    want = _cpu(eng.predict(nolabel, views=views, probs=True))
    got = _cpu(eng.predict_scene(nolabel, blend="flat", views=views, probs=True))
    assert set(got) == set(want)
    for t, hb in eng.hb.items():
        cls, conf, probs = got[t]
        wcls, wconf, wprobs = want[t]
        if hb["kind"] == "segment":
            assert bits_equal(probs, wprobs[:, 0]) and torch.equal(cls, wcls), t
            assert bits_equal(conf, wprobs[:, 0].max(dim=1).values), t
        else:
            assert cls.shape[:3] == (eng.B, 1, 1)
            assert bits_equal(cls[:, 0, 0], wcls) and bits_equal(conf[:, 0, 0], wconf) and bits_equal(probs[:, 0, 0], wprobs), t
    bare = _cpu(eng.predict_scene(nolabel, blend="flat", views=views))                 # without probs: the same maps, no probabilities
    assert all(p[2] is None and bits_equal(p[0], got[t][0]) and bits_equal(p[1], got[t][1]) for t, p in bare.items())


@pytest.mark.parametrize("name,units", [("sup_flair_seg", 4), ("sup_pastis_two", 24)])
def test_engine_stride_of_one_window(name, units):
    """(b) stride = W, flat profile.  On FLAIR (4 = 2 W units) the windows tile the scene and every window's block is its
    ``predict``.  On PASTIS 24 units are 1.5 windows: the plan's last window is clamped to [8, 24) and shares [8, 16) with the
    first, so a block can equal its window's ``predict`` only where that window is alone; the shared band is the mean of two
    windows and is held to the reference instead."""
    eng, _, dbatch = _engine(name)
    scene = _scene(eng, dbatch, 1, units, units)
    geo, N, Hu, Wu, wins, table = _plan(eng, scene, eng.scene_geometry()["W"])  # noqa: N806
    assert len(wins) == 4 and table.shape[0] == 2
    per = _per_window(eng, scene, table, (0,))
    got = _cpu(eng.predict_scene(scene, stride=geo["W"], blend="flat", probs=True))
    for t, hb in eng.hb.items():
        cls, conf, probs = got[t]
        if hb["kind"] != "segment":
            for k, (n, y0, x0, _) in enumerate(table.reshape(-1, 4).tolist()):
                iy, ix = divmod(k, 2)
                assert all(bits_equal(g[n, iy, ix], w) for g, w in zip(got[t], per[t][k])), (t, k)
            continue
        q, S = geo["qt"][t], geo["W"] * geo["qt"][t]  # noqa: N806
        depth = torch.zeros(Hu * q, Wu * q)
        for _, y0, x0, _ in table.reshape(-1, 4).tolist():
            depth[y0 * q: y0 * q + S, x0 * q: x0 * q + S] += 1
        assert (depth.max() == 1) == (name == "sup_flair_seg")
        for k, (n, y0, x0, _) in enumerate(table.reshape(-1, 4).tolist()):
            alone = depth[y0 * q: y0 * q + S, x0 * q: x0 * q + S] == 1
            wcls, _, wprobs = per[t][k]
            block = (slice(y0 * q, y0 * q + S), slice(x0 * q, x0 * q + S))
            assert alone.any() and torch.equal(cls[n][block][alone], wcls[alone]), (t, k)
            assert bits_equal(probs[n][(slice(None),) + block][:, alone], wprobs[0][:, alone]), (t, k)
            assert bits_equal(conf[n][block][alone], wprobs[0].max(dim=0).values[alone]), (t, k)
        _against_reference(eng, t, got[t], per[t], table, geo, "flat", N, Hu, Wu)


def _against_reference(eng, t, got, per, table, geo, blend, N, Hu, Wu):  # noqa: N803
    hb = eng.hb[t]
    q, C = geo["qt"][t], hb["C"]  # noqa: N806
    S, B = geo["W"] * q, eng.B  # noqa: N806
    acc, wsum = np.zeros((N, C, Hu * q, Wu * q), np.float32), np.zeros((N, Hu * q, Wu * q), np.float32)
    profile = hip.blend_profile(S, blend)
    for i, rows in enumerate(table):
        prob = np.stack([per[i * B + b][2][0].numpy() for b in range(B)])
        acc, wsum = hip.scene_blend_reference(prob, 1.0, profile, rows, q, acc, wsum)
    wcls, wconf, wmean = hip.scene_finish_reference(acc, wsum)
    cls, conf, probs = got
    assert torch.equal(cls, torch.from_numpy(wcls)), f"{t}: {int((cls != torch.from_numpy(wcls)).sum())} classes differ"
    assert bits_equal(conf, torch.from_numpy(wconf)) and bits_equal(probs, torch.from_numpy(wmean)), t
    assert int(cls.max()) < C


@pytest.mark.parametrize("name,units,stride", [("sup_flair_seg", 4, 1), ("sup_pastis_two", 24, 5)])
def test_engine_overlapping_windows_equal_the_reference(name, units, stride):
    """(c) Half-window stride on FLAIR, stride 5 on PASTIS (a clamped edge window): 9 windows in batches of 2, the last batch padded;
    linear profile; the canvas against ``scene_blend_reference`` fed the per-window probabilities of ``predict``; the multilabel
    head's window grid against ``predict`` itself.  (d) Two more calls -- the captured and the replayed segment -- give the same
    bits."""
    eng, _, dbatch = _engine(name)
    scene = _scene(eng, dbatch, 1, units, units)
    geo, N, Hu, Wu, wins, table = _plan(eng, scene, stride)  # noqa: N806
    assert len(wins) == 9 and table.shape == (5, 2, 4) and table[-1, 1, 3] == 0
    per = _per_window(eng, scene, table, (0,))
    got = _cpu(eng.predict_scene(scene, stride=stride, blend="linear", probs=True))
    for t, hb in eng.hb.items():
        if hb["kind"] == "segment":
            _against_reference(eng, t, got[t], per[t], table, geo, "linear", N, Hu, Wu)
            continue
        assert got[t][0].shape == (1, 3, 3, hb["C"])
        for k in range(9):
            iy, ix = divmod(k, 3)
            assert all(bits_equal(g[0, iy, ix], w) for g, w in zip(got[t], per[t][k])), (t, k)
    assert _same(_cpu(eng.predict_scene(scene, stride=stride, blend="linear", probs=True)), got)
    assert _same(_cpu(eng.predict_scene(scene, stride=stride, blend="linear", probs=True)), got)
    if os.environ.get("MAESTRO_GRAPHS", "1") != "0":         # (the engine clears use_graphs itself when a capture fails)
        assert eng.use_graphs and "sup_predict_scene" in eng._graphs, "no segment of predict_scene was captured"
    d4 = _cpu(eng.predict_scene(scene, stride=stride, views=(0, 3, 5)))
    assert _same(_cpu(eng.predict_scene(scene, stride=stride, views=(0, 3, 5))), d4)
    assert all(p[2] is None for p in d4.values())


@pytest.mark.parametrize("name", list(GEOMETRY))
def test_engine_leaves_the_training_state_alone(name):
    """(e) Parameters, the gradient buffer and ``loss_acc`` keep their bits; ``backward()`` raises until the next ``forward``."""
    eng, ds, dbatch = _engine(name)
    eng.forward(dbatch)
    eng.zero_grad()
    eng.backward()
    torch.cuda.synchronize()
    state = [eng.store.flat.clone(), eng.store.grad.clone(), eng.loss_acc.clone()]
    units = 2 * eng.scene_geometry()["W"] - 1
    eng.predict_scene(_scene(eng, dbatch, 2, units, units))
    torch.cuda.synchronize()
    for was, now in zip(state, (eng.store.flat, eng.store.grad, eng.loss_acc)):
        assert bits_equal(was, now)
    with pytest.raises(RuntimeError, match="forward"):
        eng.backward()
    eng.forward(dbatch)
    eng.zero_grad()
    eng.backward()
    nolabel = {k: v for k, v in dbatch.items() if k not in ds.dataset.targets}
    assert _same(_cpu(eng.predict(nolabel)), _cpu(eng.predict(nolabel)))             # predict still works beside it


def test_engine_refuses_bad_scenes_before_any_launch():
    eng, _, dbatch = _engine("sup_pastis_two")
    scene = _scene(eng, dbatch, 1, 24, 24)
    with pytest.raises(ValueError, match="disagree"):
        eng.predict_scene(dict(scene, s1_asc=scene["s1_asc"][..., :20].contiguous()))
    with pytest.raises(ValueError, match="below one window"):
        eng.predict_scene({k: (v[..., :8, :].contiguous() if v.dim() == 5 else v) for k, v in scene.items()})
    with pytest.raises(ValueError, match="stride"):
        eng.predict_scene(scene, stride=17)
    with pytest.raises(ValueError, match="blend"):
        eng.predict_scene(scene, blend="gauss")
    with pytest.raises(ValueError, match="GPU"):
        eng.predict_scene(dict(scene, s2=scene["s2"].cpu()))


def test_module_and_loop_pass_through():
    """``SSLModule.predict_scene`` and ``SupervisedLoop.predict_scene`` are the engine's call with their own weights / thresholds."""
    from types import SimpleNamespace

    import maestro_amd.conf as conf
    from maestro_amd.ssl import mae as pmae
    from maestro_amd.train.model import SSLModule
    from maestro_amd.train.trainer import SupervisedLoop
    from tests.test_oracle_sup import build_sup_case
    case, ds, oracle, _, batch = build_sup_case("sup_pastis_two")
    module = SSLModule(datasets=ds, mask=conf.MaskConfig(), interpolate="nearest", fusion_mode=case["fusion"],
                       inter_depth=case["inter_depth"], model="mae", model_size=case["size"], type_head=case["type_head"])
    model = getattr(pmae, f"mae_{case['size']}")(
        datasets=ds, mask=conf.MaskConfig(), interpolate="nearest", fusion_mode=case["fusion"], inter_depth=case["inter_depth"],
        model="mae", num_levels=1, type_head=case["type_head"], fac_abs_enc=1.0, fac_date_enc=1.0, **case["model_kw"])
    model.load_state_dict(oracle.state_dict(), strict=True)
    module.model = model
    module.trainer = SimpleNamespace(ssl_phase="probe")
    eng = model.sup_engine(case["B"], DEV, "probe")
    scene = _scene(eng, {k: v.to(DEV) for k, v in batch.items()}, 1, 24, 16)
    want = _cpu(eng.predict_scene(scene, stride=8, probs=True))
    got = _cpu(module.predict_scene(scene, stride=8, probs=True))
    assert model._sup_engine is eng and _same({"pastis_seg": got["pastis_seg"]}, {"pastis_seg": want["pastis_seg"]})
    assert all(bits_equal(g, w) for g, w in zip(got["pastis_mlc"][1:], want["pastis_mlc"][1:]))       # (cls: the metric's threshold)
    assert got["pastis_seg"][0].shape == (1, 24, 16) and got["pastis_mlc"][0].shape[:3] == (1, 2, 1)
    # the loop's method on a stand-in that holds only `.engine`: every argument arrives, none swapped (non-default values throughout)
    kw = dict(stride=5, blend="flat", views=(3, 0), probs=True, threshold=0.25)
    want = _cpu(eng.predict_scene(scene, **kw))
    assert _same(_cpu(SupervisedLoop.predict_scene(SimpleNamespace(engine=eng), scene, **kw)), want)
    assert _same(_cpu(SupervisedLoop.predict_scene(SimpleNamespace(engine=eng), scene, *kw.values())), want)     # positionally
    bare = SupervisedLoop.predict_scene(SimpleNamespace(engine=eng), scene)                      # defaults: stride W // 2, no probs
    assert bare["pastis_seg"].probs is None and bare["pastis_mlc"].cls.shape[:3] == (1, 2, 1)
