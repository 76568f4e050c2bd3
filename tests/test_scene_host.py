"""Scene prediction without a GPU: its three entry points of include/maestro_hip.h (declared, exported, bound, bad arguments refused
before any launch), the window plan, ``hip.scene_blend_reference`` (the statement the kernels are held to bit for bit in
tests/test_scene_gpu.py) and the argument checks of ``predict_scene``."""

import ctypes
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import maestro_amd.conf as conf
from maestro_amd import hip
from maestro_amd.engine_sup import check_scene, scene_unit

ROOT = Path(__file__).resolve().parents[1]
NAMES = ("mh_window_gather", "mh_predict_blend", "mh_predict_blend_finish")
FAKE = ctypes.c_void_p(0x10000)      # never dereferenced: every call below is rejected before any launch
NULL = ctypes.c_void_p(0)


# ------------------------------------------------------------------------------------------------------------- C ABI
def test_scene_names_are_declared_exported_bound_and_wrapped():
    header = (ROOT / "include" / "maestro_hip.h").read_text()
    declared = set(re.findall(r"\b(mh_[a-z0-9_]+)\s*\(", header))
    assert set(NAMES) <= declared
    assert 'extern "C"' in header
    for ref in ("maestro/dataset/dataset.py:86-105", "maestro/conf/dataset/utils.py:99-109"):
        assert ref in header
    lib = hip.lib()
    for name in NAMES:
        assert hasattr(lib, name), f"{name} is declared but not exported"
        assert getattr(lib, name).argtypes is not None and callable(getattr(hip, name[3:]))
    for fn in ("blend_profile", "scene_windows", "scene_table", "scene_blend_reference", "scene_finish_reference"):
        assert callable(getattr(hip, fn))
    assert (hip.SCENE_MAX_SLOTS, hip.SCENE_MAX_S, hip.SCENE_UNCOVERED) == tuple(
        int(re.search(rf"#define MH_SCENE_{k}\s+(\d+)", header).group(1)) for k in ("MAX_SLOTS", "MAX_S", "UNCOVERED"))


def _err():
    return hip.lib().mh_last_error().decode()


GOOD = np.array([[0, 0, 0, 1], [1, 2, 2, 1], [1, 2, 2, 0]], dtype=np.int32)       # N = 2 scenes of 4 x 4 units, W = 2


def _table(rows):
    t = np.ascontiguousarray(rows, dtype=np.int32)
    return t, ctypes.c_void_p(t.ctypes.data)


def _gather(scene=FAKE, out=FAKE, tdev=FAKE, rows=GOOD, host=True, B=3, N=2, planes=3, Hs=20, Ws=20, S=10, q=5):  # noqa: N803
    keep, thost = _table(rows)
    return hip.lib().mh_window_gather(scene, out, tdev, thost if host else NULL, B, N, planes, Hs, Ws, S, q, NULL)


def _blend(prob=FAKE, scale=1.0, profile=FAKE, tdev=FAKE, rows=GOOD, host=True, acc=FAKE, wsum=FAKE, B=3, N=2, C=5, S=10, q=5, Hc=20,  # noqa: N803
           Wc=20):
    keep, thost = _table(rows)
    return hip.lib().mh_predict_blend(prob, scale, profile, tdev, thost if host else NULL, acc, wsum, B, N, C, S, q, Hc, Wc, NULL)


def _finish(acc=FAKE, wsum=FAKE, cls=FAKE, conf=FAKE, mean=NULL, N=2, C=5, n_pix=16):  # noqa: N803
    return hip.lib().mh_predict_blend_finish(acc, wsum, cls, conf, mean, N, C, n_pix, NULL)


def _rows(b, **kw):
    r = GOOD.copy()
    for k, v in kw.items():
        r[b, "nyx".index(k)] = v
    return r


def _id(kw):
    return "-".join(f"{k}={'null' if v is NULL else ('rows' if isinstance(v, np.ndarray) else v)}" for k, v in kw.items())


TABLE_BAD = [dict(rows=_rows(1, n=2)), dict(rows=_rows(0, n=-1)), dict(rows=_rows(1, y=3)), dict(rows=_rows(1, x=3)),
             dict(rows=_rows(0, y=-1)), dict(rows=_rows(2, x=3))]          # (the last one: a pad slot is gathered, so it is checked too)


@pytest.mark.parametrize("kw", [dict(scene=NULL), dict(out=NULL), dict(tdev=NULL), dict(host=False), dict(B=0), dict(N=0), dict(planes=0),
                                dict(S=0), dict(q=0), dict(Hs=0), dict(B=hip.SCENE_MAX_SLOTS + 1), dict(Hs=19), dict(Ws=19)] + TABLE_BAD,
                         ids=_id)
def test_window_gather_rejects_bad_arguments_before_any_launch(kw):
    assert _gather(**kw) < 0
    assert "mh_window_gather" in _err()


@pytest.mark.parametrize("kw", [dict(prob=NULL), dict(profile=NULL), dict(tdev=NULL), dict(host=False), dict(acc=NULL), dict(wsum=NULL),
                                dict(B=0), dict(N=0), dict(C=0), dict(C=1), dict(C=129), dict(S=0), dict(q=0), dict(Hc=0),
                                dict(S=hip.SCENE_MAX_S + 1), dict(scale=0.0), dict(scale=2.0), dict(Hc=19), dict(Wc=19)] + TABLE_BAD,
                         ids=_id)
def test_predict_blend_rejects_bad_arguments_before_any_launch(kw):
    assert _blend(**kw) < 0
    assert "mh_predict_blend" in _err() and "mh_predict_blend_finish" not in _err()


@pytest.mark.parametrize("kw", [dict(acc=NULL), dict(wsum=NULL), dict(cls=NULL, conf=NULL), dict(N=0), dict(C=0), dict(C=1), dict(C=129),
                                dict(n_pix=0)], ids=_id)
def test_predict_blend_finish_rejects_bad_arguments_before_any_launch(kw):
    assert _finish(**kw) < 0
    assert "mh_predict_blend_finish" in _err()


def test_wrappers_check_their_tensors_and_have_no_cpu_fallback():
    tab = torch.zeros(1, 4, dtype=torch.int32)
    rows = np.array([[0, 0, 0, 1]], dtype=np.int32)
    with pytest.raises(hip.HipExtensionError, match="out"):
        hip.window_gather(torch.zeros(1, 2, 4, 4), torch.zeros(1, 2, 2, 3), tab, rows, 1, 1, 2, 4, 4, 2, 1)
    with pytest.raises(hip.HipExtensionError, match="scene"):
        hip.window_gather(torch.zeros(1, 2, 4, 4).double(), torch.zeros(1, 2, 2, 2), tab, rows, 1, 1, 2, 4, 4, 2, 1)
    with pytest.raises(hip.HipExtensionError, match="host window table"):
        hip.window_gather(torch.zeros(1, 2, 4, 4), torch.zeros(1, 2, 2, 2), tab, rows[:0], 1, 1, 2, 4, 4, 2, 1)
    with pytest.raises(hip.HipExtensionError, match="profile"):
        hip.predict_blend(torch.zeros(1, 2, 2, 2), 1.0, torch.zeros(3), tab, rows, torch.zeros(1, 2, 4, 4), torch.zeros(1, 4, 4), 1, 1, 2, 2,
                          1, 4, 4)
    with pytest.raises(hip.HipExtensionError, match="cls"):
        hip.predict_blend_finish(torch.zeros(1, 2, 16), torch.zeros(1, 16), torch.zeros(16), None, None, 1, 2, 16)
    with pytest.raises(hip.HipExtensionError, match="GPU"):       # well-formed CPU tensors: no fallback exists
        hip.window_gather(torch.zeros(1, 2, 4, 4), torch.zeros(1, 2, 2, 2), tab, rows, 1, 1, 2, 4, 4, 2, 1)


# ------------------------------------------------------------------------------------------------------------- the window plan
@pytest.mark.parametrize("U,W,s,starts", [(2, 2, 1, [0]), (4, 2, 1, [0, 1, 2]), (4, 2, 2, [0, 2]), (5, 2, 2, [0, 2, 3]),
                                          (24, 16, 5, [0, 5, 8]), (16, 16, 8, [0])])
def test_scene_windows_counts_starts_and_cover(U, W, s, starts):  # noqa: N803
    assert hip.scene_axis_starts(U, W, s) == starts
    wins = hip.scene_windows(U, U, W, s)
    assert wins == [(y, x) for y in starts for x in starts] and len(wins) == len(starts) ** 2      # row-major
    covered = np.zeros((U, U), dtype=int)
    for y, x in wins:
        assert 0 <= y and y + W <= U and 0 <= x and x + W <= U
        covered[y: y + W, x: x + W] += 1
    assert covered.min() >= 1, "a unit no window covers"
    assert starts.count(U - W) == 1 and starts == sorted(set(starts))        # the clamped last start, exactly once
    assert all(b - a == s for a, b in zip(starts[:-2], starts[1:-1])) and starts[-1] - starts[-2] <= s if len(starts) > 1 else True
    # rectangular scenes: the two axes are planned on their own
    assert hip.scene_windows(U, W, W, s) == [(y, 0) for y in starts]


def test_scene_windows_default_stride_and_refusals():
    assert hip.scene_windows(4, 2, 2) == hip.scene_windows(4, 2, 2, 1)                 # max(1, W // 2)
    assert hip.scene_axis_starts(40, 16) == hip.scene_axis_starts(40, 16, 8) == [0, 8, 16, 24]
    assert hip.scene_axis_starts(3, 1) == [0, 1, 2]
    for U, W, s in ((1, 2, 1), (15, 16, 8), (4, 2, 0), (4, 2, 3), (4, 2, -1), (4, 2, 1.0), (4, 2, True)):  # noqa: N806
        with pytest.raises(ValueError):
            hip.scene_windows(U, U, W, s)
    with pytest.raises(ValueError):
        hip.scene_windows(4, 1, 2, 1)                                                  # one axis below a window


def test_scene_table_is_scene_major_and_pads_with_the_batch_first_window():
    wins = hip.scene_windows(4, 4, 2, 2)                                               # 4 windows per scene
    t = hip.scene_table(3, wins, 5)                                                    # 12 windows in batches of 5
    assert t.dtype == np.int32 and t.shape == (3, 5, 4)
    flat = t.reshape(-1, 4)
    assert flat[:12].tolist() == [[n, y, x, 1] for n in range(3) for (y, x) in wins]
    assert flat[12:].tolist() == [flat[10].tolist()[:3] + [0]] * 3                      # the LAST batch's first window, on = 0
    assert hip.scene_table(1, wins, 4).shape == (1, 4, 4) and hip.scene_table(1, wins, 4)[..., 3].all()
    with pytest.raises(ValueError):
        hip.scene_table(1, [], 4)


def test_blend_profile():
    assert hip.blend_profile(6, "flat").tolist() == [1.0] * 6 and hip.blend_profile(6, "flat").dtype == np.float32
    for S in (1, 4, 5, 6, 16, 255):  # noqa: N806
        p = hip.blend_profile(S, "linear")
        want = (np.minimum(np.arange(S) + 1, S - np.arange(S)).astype(np.float32) / np.float32((S + 1) // 2))
        assert p.dtype == np.float32 and np.array_equal(p, want) and p.min() > 0 and p.max() == 1.0
        assert np.array_equal(p, p[::-1])
    assert hip.blend_profile(4, "linear").tolist() == [0.5, 1.0, 1.0, 0.5]
    with pytest.raises(ValueError, match="blend"):
        hip.blend_profile(4, "cosine")


# ------------------------------------------------------------------------------------------------------------- the numpy restatement
def _plan(Hu, Wu, W, stride, B):  # noqa: N803
    return hip.scene_table(1, hip.scene_windows(Hu, Wu, W, stride), B)


def _run(prob, profile, batches, q, canvas, scale=1.0):
    """Feed the rows of ``batches`` ``[n_batches, B, 4]`` (``prob`` holds one entry per row) to the reference, batch after batch."""
    acc, wsum = np.zeros(canvas, np.float32), np.zeros((canvas[0],) + canvas[2:], np.float32)
    B = batches.shape[1]  # noqa: N806
    for i, rows in enumerate(batches):
        acc, wsum = hip.scene_blend_reference(prob[i * B: (i + 1) * B], scale, profile, rows, q, acc, wsum)
    return acc, wsum


def _ulps(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


@pytest.mark.parametrize("kind", ["flat", "linear"])
@pytest.mark.parametrize("S,q,stride,U,deep", [(4, 2, 2, 4, 1), (5, 5, 1, 3, 1), (16, 1, 16, 32, 1),      # every pixel under ONE window
                                               (4, 2, 1, 5, 4), (6, 3, 1, 5, 4), (16, 1, 5, 33, 16)])      # up to `deep` windows
def test_reference_constant_probabilities_come_back(kind, S, q, stride, U, deep):  # noqa: N803
    """Windows that all hold the same probabilities blend to those probabilities, for both profiles: within ONE ulp wherever at
    most four windows cover a pixel -- one window per pixel, and the half-window stride the feature runs at (2 x 2 windows deep).
    Deeper overlap cannot be held to 1 ulp under the sum order the kernels are specified with: acc is a sequential fp32 sum of k
    rounded terms (relative error <= k u to first order, u = 2^-24), wsum a sequential sum of the same k weights (<= (k - 1) u),
    the quotient adds u, and u |v| < ulp(v): |mean - v| < 2 k ulp.  That derived bound is what pixels under more than four
    windows are held to (depth 16 here: 2 ulp observed with the flat profile, 3 with the linear one); cls is exact in all."""
    W, C = S // q, 3  # noqa: N806
    batches = _plan(U, U, W, stride, 4)
    const = np.array([0.2, 0.7, 0.1], dtype=np.float32)
    prob = np.broadcast_to(const[None, :, None, None], (batches.shape[0] * 4, C, S, S)).copy()
    acc, wsum = _run(prob, hip.blend_profile(S, kind), batches, q, (1, C, U * q, U * q))
    depth = _run(np.ones_like(prob), np.ones(S, np.float32), batches, q, (1, C, U * q, U * q))[1].astype(np.int64)
    cls, conf, mean = hip.scene_finish_reference(acc, wsum)
    assert (wsum > 0).all() and (cls == 1).all()
    want = np.broadcast_to(const[None, :, None, None], mean.shape).copy()
    off = _ulps(mean, want)
    print(f"S={S} q={q} stride={stride} {kind}: depth <= {int(depth.max())}, |mean - const| <= {int(off.max())} ulp")
    assert depth.min() >= 1 and depth.max() == deep
    assert (off <= np.where(depth <= 4, 1, 2 * depth)[:, None]).all(), int(off.max())
    assert np.array_equal(conf, mean[:, 1])


def test_reference_integer_probabilities_with_dyadic_weights_are_exact():
    S, q, W, U, C = 4, 2, 2, 5, 3  # noqa: N806
    batches = _plan(U, U, W, 1, 4)                                                      # 16 windows, up to 4 deep
    rng = np.random.default_rng(11)
    prob = rng.integers(0, 1000, size=(16, C, S, S)).astype(np.float32)
    profile = hip.blend_profile(S, "linear")                                            # 0.5, 1, 1, 0.5
    acc, wsum = _run(prob, profile, batches, q, (1, C, U * q, U * q), scale=0.5)
    want = np.zeros((C, U * q, U * q), dtype=np.int64)                                  # 8 * acc, in integers
    wwant = np.zeros((U * q, U * q), dtype=np.int64)                                    # 4 * wsum
    w2 = (2 * profile).astype(np.int64)
    for b, (n, y0, x0, on) in enumerate(batches.reshape(-1, 4).tolist()):
        want[:, y0 * q: y0 * q + S, x0 * q: x0 * q + S] += prob[b].astype(np.int64) * (w2[:, None] * w2[None, :])[None]
        wwant[y0 * q: y0 * q + S, x0 * q: x0 * q + S] += w2[:, None] * w2[None, :]
    assert np.array_equal(acc[0].astype(np.float64) * 8, want.astype(np.float64))
    assert np.array_equal(wsum[0].astype(np.float64) * 4, wwant.astype(np.float64))
    cls, conf, mean = hip.scene_finish_reference(acc, wsum)
    assert np.array_equal(cls[0], hip.argmax_reference(want.astype(np.float64), 0))
    assert np.array_equal(mean, (acc / wsum[:, None]).astype(np.float32)) and np.array_equal(conf, mean.max(axis=1))


def test_reference_pad_slots_uncovered_pixels_and_batching():
    S, q, W, U, C = 4, 2, 2, 4, 2  # noqa: N806
    rng = np.random.default_rng(12)
    wins = hip.scene_windows(U, U, W, 1)                                                # 9 windows
    prob = rng.random((9, C, S, S), dtype=np.float32)
    profile = hip.blend_profile(S, "linear")
    canvas = (1, C, U * q, U * q)
    one = _run(prob, profile, hip.scene_table(1, wins, 9), q, canvas)
    # the same bits when the 9 windows come as batches of 2 (the last one padded)
    two = hip.scene_table(1, wins, 2)
    assert two.shape == (5, 2, 4) and two[-1, 1].tolist() == two[-1, 0].tolist()[:3] + [0]
    padded = np.concatenate([prob, rng.random((1, C, S, S), dtype=np.float32)])        # the pad slot's values must not matter
    for got, want in zip(_run(padded, profile, two, q, canvas), one):
        assert np.array_equal(got.view(np.int32), want.view(np.int32))
    # a pad slot in the middle changes nothing; the input canvas is not modified
    rows = np.array([[0, 0, 0, 1], [0, 1, 1, 0], [0, 2, 2, 1]], dtype=np.int32)
    acc0, w0 = np.zeros(canvas, np.float32), np.zeros((1, U * q, U * q), np.float32)
    a3, w3 = hip.scene_blend_reference(prob[:3], 1.0, profile, rows, q, acc0, w0)
    a2, w2 = hip.scene_blend_reference(prob[[0, 2]], 1.0, profile, rows[[0, 2]], q, acc0, w0)
    assert np.array_equal(a3, a2) and np.array_equal(w3, w2) and not acc0.any() and not w0.any()
    # windows (0, 0) and (2, 2) leave the two off-diagonal corners uncovered: 255 / 0 / 0
    cls, conf, mean = hip.scene_blend_reference(prob[:3], 1.0, profile, rows, q, acc0, w0, finish=True)
    hole = w3[0] == 0
    assert hole[0, -1] and hole[-1, 0] and not hole[0, 0] and hole.sum() == 2 * 16
    assert (cls[0][hole] == hip.SCENE_UNCOVERED).all() and (conf[0][hole] == 0).all() and (mean[0][:, hole] == 0).all()
    assert (cls[0][~hole] < C).all() and (conf[0][~hole] > 0).all()
    with pytest.raises(ValueError, match="leaves the canvas"):
        hip.scene_blend_reference(prob[:1], 1.0, profile, np.array([[0, 3, 0, 1]]), q, acc0, w0)


def test_reference_finish_ties_nans_and_order_of_operations():
    nan = np.float32("nan")
    acc = np.array([[[1.0, 2.0, 3.0, nan, 0.0], [1.0, 2.0, 1.0, 5.0, 0.0], [0.5, 1.0, 3.0, nan, 0.0]]], dtype=np.float32)   # [1, C = 3, 5]
    wsum = np.array([[2.0, 3.0, 0.0, 1.0, 1.0]], dtype=np.float32)
    cls, conf, mean = hip.scene_finish_reference(acc, wsum)
    assert cls.tolist() == [[0, 0, hip.SCENE_UNCOVERED, 0, 0]]                           # ties -> lowest index; the first NaN wins
    assert conf[0, :3].tolist() == [0.5, np.float32(2.0) / np.float32(3.0), 0.0] and np.isnan(conf[0, 3]) and conf[0, 4] == 0
    assert np.array_equal(mean[0, :, 1], acc[0, :, 1] / np.float32(3.0)) and (mean[0, :, 2] == 0).all()
    # the blend rounds (prob * scale) first, then * w, then the sum: pick values where any other order differs
    S = 16  # noqa: N806
    s, profile = np.float32(1.0 / 3.0), hip.blend_profile(S, "linear") * np.float32(0.7)
    prob = np.random.default_rng(13).random((1, 2, S, S), dtype=np.float32)
    acc0, w0 = np.full((1, 2, S, S), 0.01, np.float32), np.ones((1, S, S), np.float32)
    w = profile[:, None] * profile[None, :]
    a, ws = hip.scene_blend_reference(prob, s, profile, [[0, 0, 0, 1]], 1, acc0, w0)
    assert np.array_equal(a[0], acc0[0] + (prob[0] * s) * w[None]) and np.array_equal(ws[0], w0[0] + w)
    assert not np.array_equal(a[0], acc0[0] + prob[0] * (s * w)[None])                        # another association: other bits
    assert not np.array_equal(a[0], (acc0[0].astype(np.float64) + (prob[0] * s).astype(np.float64) * w[None]).astype(np.float32))  # an FMA


# ------------------------------------------------------------------------------------------------------------- Python surfaces
FLAIR = {"aerial": (64, 1, 4), "s2": (10, 2, 10)}       # name -> (image_size, dates, channels); with a 256-pixel target W = 2


def _scene(Hu=4, Wu=4, N=2, rasters=FLAIR, W=2):  # noqa: N803
    out = {"ref_date": torch.zeros(N, 1, 3, dtype=torch.int16)}
    for src, (S, D, C) in rasters.items():  # noqa: N806
        q = S // W
        out[src] = torch.zeros(N, D, C, Hu * q, Wu * q)
        out[f"{src}_dates"] = torch.zeros(N, D, 3, dtype=torch.int16)
    return out


def test_scene_unit_is_the_gcd_of_the_model_sizes():
    assert scene_unit([64, 10, 256]) == 2 and scene_unit([16, 16, 16]) == 16 and scene_unit([512, 10, 512]) == 2
    assert scene_unit([60]) == 60 and scene_unit([64, 32, 9]) == 1


def test_predict_scene_refusals_on_cpu_tensors():
    ok = _scene()
    with pytest.raises(ValueError, match="GPU"):                       # everything else is fine: the device is what is wrong
        check_scene(ok, FLAIR, 2)
    bad = dict(ok, s2=torch.zeros(2, 2, 10, 25, 20))
    with pytest.raises(ValueError, match="disagree"):
        check_scene(bad, FLAIR, 2)
    with pytest.raises(ValueError, match="disagree"):
        check_scene(dict(ok, s2=ok["s2"][:1].contiguous(), s2_dates=ok["s2_dates"][:1].contiguous()), FLAIR, 2)
    with pytest.raises(ValueError, match="pixels per unit"):
        check_scene(dict(ok, s2=torch.zeros(2, 2, 10, 21, 20)), FLAIR, 2)
    with pytest.raises(ValueError, match="below one window"):
        check_scene(_scene(Hu=1), FLAIR, 2)
    with pytest.raises(ValueError, match="below one window"):
        check_scene(_scene(Hu=8, Wu=15, rasters={"s2": (16, 1, 3)}, W=16), {"s2": (16, 1, 3)}, 16)
    for stride in (0, 3, -1, 1.5, True):
        with pytest.raises(ValueError, match="stride"):
            check_scene(ok, FLAIR, 2, stride=stride)
    with pytest.raises(ValueError, match="blend"):
        check_scene(ok, FLAIR, 2, blend="cosine")
    with pytest.raises(ValueError, match="float32"):
        check_scene(dict(ok, aerial=ok["aerial"].double()), FLAIR, 2)
    with pytest.raises(ValueError, match="contiguous"):
        check_scene(dict(ok, aerial=torch.zeros(2, 1, 4, 128, 256)[..., ::2]), FLAIR, 2)
    with pytest.raises(ValueError, match="aerial"):
        check_scene({k: v for k, v in ok.items() if k != "aerial"}, FLAIR, 2)
    with pytest.raises(ValueError, match="int16"):
        check_scene(dict(ok, s2_dates=ok["s2_dates"].int()), FLAIR, 2)
    with pytest.raises(ValueError, match="ref_date"):
        check_scene(dict(ok, ref_date=torch.zeros(1, 1, 3, dtype=torch.int16)), FLAIR, 2)
    with pytest.raises(ValueError, match="ref_date.*int16"):          # the date kernel reads int16_t
        check_scene(dict(ok, ref_date=ok["ref_date"].long()), FLAIR, 2)


def test_module_predict_scene_refuses_the_pretrain_phase():
    from maestro_amd.train.model import SSLModule
    ds = conf.DatasetsConfig(name_dataset="s2_naip", s2_naip=conf.S2NAIPConfig(filter_inputs=["spot"]))
    module = SSLModule(datasets=ds, mask=conf.MaskConfig(), interpolate="nearest", fusion_mode="group", inter_depth=1, model="mae",
                       model_size="tiny")
    module.trainer = SimpleNamespace(ssl_phase="pretrain")
    with pytest.raises(ValueError, match="predict_scene"):
        module.predict_scene({"spot": torch.zeros(1, 1, 3, 256, 256)})
