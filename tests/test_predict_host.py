"""The prediction path without a GPU: its two entry points of include/maestro_hip.h (declared, exported, bound, bad arguments
refused before any launch), ``hip.predict_reference`` against torch on the CPU, and the argument checks of the Python surfaces."""

import ctypes
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import maestro_amd.conf as conf
from maestro_amd import hip
from maestro_amd.engine_sup import parse_views

ROOT = Path(__file__).resolve().parents[1]
NAMES = ("mh_predict_view", "mh_predict_finish")
FAKE = ctypes.c_void_p(0x10000)      # never dereferenced: every call below is rejected before any launch
NULL = ctypes.c_void_p(0)


# ------------------------------------------------------------------------------------------------------------- C ABI
def test_predict_names_are_declared_exported_and_bound():
    header = (ROOT / "include" / "maestro_hip.h").read_text()
    declared = set(re.findall(r"\b(mh_[a-z0-9_]+)\s*\(", header))
    assert set(NAMES) <= declared
    assert 'extern "C"' in header
    for ref in ("maestro/layers/head.py:116-130", "maestro/layers/overlay.py:11-23", "maestro/dataset/dataset.py:224-257"):
        assert ref in header
    lib = hip.lib()
    for name in NAMES:
        assert hasattr(lib, name), f"{name} is declared but not exported"
        assert getattr(lib, name).argtypes is not None and callable(getattr(hip, name[3:]))
    assert callable(hip.predict_reference)


def _err():
    return hip.lib().mh_last_error().decode()


def _view(logits=FAKE, flags=NULL, act=hip.PREDICT_SOFTMAX, thr=0.0, prob=FAKE, acc=0, cls=FAKE, conf=FAKE, B=2, g=2, P=2, C=5, ld=20):  # noqa: N803
    return hip.lib().mh_predict_view(logits, flags, act, thr, prob, acc, cls, conf, B, g, P, C, ld, NULL)


def _finish(prob=FAKE, inv_views=1 / 3, act=hip.PREDICT_SOFTMAX, thr=0.5, cls=FAKE, conf=FAKE, mean=NULL, B=2, C=5, n_pix=16):  # noqa: N803
    return hip.lib().mh_predict_finish(prob, inv_views, act, thr, cls, conf, mean, B, C, n_pix, NULL)


SIG = dict(act=hip.PREDICT_SIGMOID, g=1, P=1, C=18, ld=18)
VIEW_BAD = [dict(logits=NULL), dict(prob=NULL, cls=NULL, conf=NULL), dict(C=1), dict(C=129), dict(ld=19), dict(B=0), dict(g=0), dict(act=2),
            dict(SIG, g=2), dict(SIG, P=2, ld=72), dict(SIG, C=0), dict(SIG, C=1025, ld=1025), dict(SIG, ld=17)]


def _id(kw):
    return "-".join(f"{k}={'null' if v is NULL else v}" for k, v in kw.items())


@pytest.mark.parametrize("kw", VIEW_BAD, ids=_id)
def test_predict_view_rejects_bad_arguments_before_any_launch(kw):
    assert _view(**kw) < 0
    assert "mh_predict_view" in _err()


@pytest.mark.parametrize("kw", [dict(prob=NULL), dict(cls=NULL, conf=NULL), dict(C=1), dict(C=129), dict(inv_views=0.0), dict(inv_views=2.0), dict(B=0), dict(n_pix=0),
                                dict(act=hip.PREDICT_SIGMOID, n_pix=4), dict(act=hip.PREDICT_SIGMOID, n_pix=1, C=1025)], ids=_id)
def test_predict_finish_rejects_bad_arguments_before_any_launch(kw):
    assert _finish(**kw) < 0
    assert "mh_predict_finish" in _err()


def test_wrappers_check_their_tensors_and_have_no_cpu_fallback():
    x = torch.zeros(4, 8)
    with pytest.raises(hip.HipExtensionError, match="cls"):
        hip.predict_view(x, None, hip.PREDICT_SOFTMAX, None, False, torch.zeros(3, dtype=torch.uint8), None, 1, 2, 1, 8)
    with pytest.raises(hip.HipExtensionError, match="float32"):
        hip.predict_view(x.double(), None, hip.PREDICT_SOFTMAX, None, False, torch.zeros(4, dtype=torch.uint8), None, 1, 2, 1, 8)
    with pytest.raises(hip.HipExtensionError, match="prob"):
        hip.predict_finish(torch.zeros(5), 2, hip.PREDICT_SOFTMAX, None, torch.zeros(4), 1, 8, 4)
    with pytest.raises(hip.HipExtensionError, match="GPU"):       # well-formed CPU tensors: no fallback exists
        hip.predict_view(x, None, hip.PREDICT_SOFTMAX, None, False, torch.zeros(4, dtype=torch.uint8), None, 1, 2, 1, 8)


# ------------------------------------------------------------------------------------------------------------- the numpy restatement
def _raster(x, B, g, P, C):  # noqa: N803
    """Patch layout -> ``[B, C, S, S]`` with einops-free torch (head.py:116-130 read backwards)."""
    return x.reshape(B, g, g, P, P, C).permute(0, 5, 1, 3, 2, 4).reshape(B, C, g * P, g * P)


def _dihedral(r, f):
    """dataset.py:224-257 on ``[..., S, S]``: flip the rows, flip the columns, swap the axes, in this order."""
    if f & 1:
        r = torch.flip(r, dims=(-2,))
    if f & 2:
        r = torch.flip(r, dims=(-1,))
    if f & 4:
        r = r.transpose(-1, -2)
    return r.contiguous()


@pytest.mark.parametrize("g,P", [(5, 1), (1, 5)])
def test_reference_undoes_all_eight_flags_on_an_odd_raster(g, P):  # noqa: N803
    B, C, S = 8, 3, 5  # noqa: N806
    # a distinct value per pixel and class, the largest class decided by the pixel's position
    orig = torch.arange(C * S * S, dtype=torch.float32).reshape(1, C, S, S).expand(B, C, S, S).clone()
    orig[:, 1] += 5.0 * ((torch.arange(S)[:, None] + 2 * torch.arange(S)[None, :]) % 3 == 0) * 100
    flags = np.arange(8, dtype=np.uint8)
    views = torch.stack([_dihedral(orig[b], int(flags[b])) for b in range(B)])       # what the model sees
    # raster [B, C, S, S] -> patch layout
    x = views.reshape(B, C, g, P, g, P).permute(0, 2, 4, 3, 5, 1).reshape(B * g * g, P * P * C)
    assert torch.equal(_raster(x, B, g, P, C), views)
    prob, cls, conf = hip.predict_reference(x.numpy(), flags, hip.PREDICT_SOFTMAX, g=g, P=P, C=C)
    assert np.array_equal(cls, orig.argmax(dim=1).numpy().astype(np.uint8))
    want = torch.softmax(orig.double(), dim=1)
    assert np.abs(prob - want.numpy()).max() < 1e-6 and np.abs(conf - want.max(dim=1).values.numpy()).max() < 1e-6
    # placement alone, exactly: "logits" whose soft-max is not needed -- the class map of a one-hot-by-position raster
    for b in range(B):
        y0, x0 = hip.predict_pixel_map(int(flags[b]), S)
        ident = torch.arange(S * S).reshape(S, S)
        assert torch.equal(_dihedral(ident, int(flags[b])), ident[torch.from_numpy(y0), torch.from_numpy(x0)])


def test_reference_argmax_rule_ties_and_nans():
    nan = float("nan")
    rows = torch.tensor([[1.0, 1.0, 0.0, 1.0],          # tie at first / middle / last -> first
                         [0.0, 2.0, 2.0, 1.0],          # tie in the middle
                         [0.0, 1.0, 3.0, 3.0],          # tie at the end
                         [5.0, nan, 9.0, 1.0],          # a NaN is the maximum
                         [5.0, 9.0, nan, nan],          # the first NaN wins
                         [nan, nan, nan, nan],
                         [-1.0, -1.0, -1.0, -1.0]])
    _, cls, _ = hip.predict_reference(rows.numpy(), None, hip.PREDICT_SOFTMAX, C=4)
    cls = cls.reshape(-1)                                        # [B, 1, 1]: classification heads are 1 x 1 rasters
    assert cls.tolist() == [0, 1, 2, 1, 2, 0, 0]
    assert cls.tolist() == rows.argmax(dim=1).tolist()          # torch's own rule
    assert hip.argmax_reference(rows.numpy().T, 0).tolist() == cls.tolist()


def test_reference_accumulates_views_as_the_sequential_fp32_sum():
    B, g, P, C = 2, 2, 2, 5  # noqa: N806
    gen = torch.Generator().manual_seed(5)
    acc, want = None, None
    for v in (0, 3, 5, 6):
        x = torch.randn(B * g * g, P * P * C, generator=gen).numpy()
        flags = np.full(B, v, dtype=np.uint8)
        single, _, _ = hip.predict_reference(x, flags, hip.PREDICT_SOFTMAX, g=g, P=P, C=C)
        acc, _, _ = hip.predict_reference(x, flags, hip.PREDICT_SOFTMAX, g=g, P=P, C=C, prob=acc)
        want = single if want is None else (want + single).astype(np.float32)
        assert single.dtype == np.float32 and acc.dtype == np.float32
    assert np.array_equal(acc, want)


def test_reference_sigmoid_decides_on_the_logit():
    x = torch.tensor([[-2.0, 0.0, 0.5, -0.84729786, -0.8473, 3.0]])
    prob, cls, conf = hip.predict_reference(x.numpy(), None, hip.PREDICT_SIGMOID, threshold=0.3)
    assert cls.tolist() == (x > hip.logit_threshold(0.3)).to(torch.uint8).tolist()
    assert np.allclose(prob, torch.sigmoid(x).numpy(), atol=1e-7) and np.array_equal(prob, conf)
    with pytest.raises(ValueError):
        hip.predict_reference(np.zeros((4, 3), np.float32), None, hip.PREDICT_SIGMOID, g=2)


# ------------------------------------------------------------------------------------------------------------- Python surfaces
def test_views_argument():
    assert parse_views((0,)) == (0,) and parse_views([7, 1]) == (7, 1) and parse_views(range(8)) == tuple(range(8))
    assert parse_views("d4") == tuple(range(8))
    for bad in ((), [], (0, 0), (8,), (-1,), (1.0,), (True,), "all", "0", 3, None, (0, "1")):
        with pytest.raises(ValueError):
            parse_views(bad)


def test_predict_step_refuses_the_pretrain_phase():
    from maestro_amd.train.model import SSLModule
    ds = conf.DatasetsConfig(name_dataset="s2_naip", s2_naip=conf.S2NAIPConfig(filter_inputs=["spot"]))
    module = SSLModule(datasets=ds, mask=conf.MaskConfig(), interpolate="nearest", fusion_mode="group", inter_depth=1, model="mae",
                       model_size="tiny")
    assert module.predict_views == (0,)
    module.trainer = SimpleNamespace(ssl_phase="pretrain")
    with pytest.raises(ValueError, match="predict_step"):
        module.predict_step({"spot": torch.zeros(1, 1, 3, 128, 128)}, 0)
