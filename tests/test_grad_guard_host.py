"""Gradient guard, the parts that need no GPU: the header against the library and the binding, the argument checks of the
three entry points, the switches and refusals of the loops, the numpy restatement of the contract (``hip.grad_guard_reference``)
against ``torch.nn.utils.clip_grad_norm_``, and the teeth of the error bound the GPU tests use (tests/grad_guard_cases.py)."""

from __future__ import annotations

import ctypes
import math
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import grad_guard_cases as G

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "maestro_hip.h"
NAMES = ["mh_grad_guard_finish", "mh_grad_sumsq_partial", "mh_grad_sumsq_partial_rows"]


# ------------------------------------------------------------------------------------------------ header + ABI
@pytest.fixture(scope="module")
def lib():
    from maestro_amd.csrc.build import LIB, build
    if not LIB.exists():
        build()
    handle = ctypes.CDLL(str(LIB))
    handle.mh_last_error.restype = ctypes.c_char_p
    vp, ci, cl, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float
    handle.mh_grad_sumsq_partial_rows.argtypes, handle.mh_grad_sumsq_partial_rows.restype = [cl], cl
    handle.mh_grad_sumsq_partial.argtypes, handle.mh_grad_sumsq_partial.restype = [vp, cl, vp, vp, vp], ci
    handle.mh_grad_guard_finish.argtypes = [vp, vp, cl, cf, cf, ci, cf, cf, cf, vp, vp, vp]
    handle.mh_grad_guard_finish.restype = ci
    return handle


def _declared():
    return sorted(n for n in set(re.findall(r"\b(mh_[a-z0-9_]+)\s*\(", HEADER.read_text())) if n.startswith("mh_grad_"))


def test_every_declared_symbol_is_exported(lib):
    assert _declared() == NAMES
    assert not [n for n in NAMES if not hasattr(lib, n)]


def test_guard_names_are_declared_in_the_one_header():
    text = HEADER.read_text()
    assert sorted(p.name for p in (ROOT / "include").iterdir()) == ["maestro_hip.h"]
    assert not [n for n in NAMES if not re.search(rf"^(int|long) {n}\(", text, re.M)]
    for cite in ("maestro/conf/trainer.py:13", "maestro/train/model.py:135-140", "clip_grad_norm_"):
        assert cite in text, cite


def test_struct_and_chunk_match_the_header():
    from maestro_amd import hip
    text = HEADER.read_text()
    body = re.search(r"typedef struct \{([^}]*)\} MhGuardState;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decls = [d.strip() for d in body.split(";") if d.strip()]
    ctype = {"float": ctypes.c_float, "int": ctypes.c_int, "unsigned": ctypes.c_uint, "long long": ctypes.c_longlong}
    fields = [(d.rsplit(" ", 1)[1], ctype[d.rsplit(" ", 1)[0]]) for d in decls]
    assert fields == list(hip._MhGuardState._fields_)
    assert ctypes.sizeof(hip._MhGuardState) == 32 and hip._MhGuardState.t.offset == 16 and hip._MhGuardState.skipped.offset == 24
    assert f"#define MH_GUARD_CHUNK {hip.GUARD_CHUNK}" in text and hip.GUARD_CHUNK == G.C


def test_the_header_is_hashed_by_the_build():
    """csrc/build.py keys every object by its source and the shared headers: the one C header is among them, and the source that
    defines the entries includes it."""
    import inspect

    from maestro_amd.csrc import build as B
    assert '"maestro_hip.h"' in inspect.getsource(B._digest) and inspect.getsource(B._digest).count("maestro_hip") == 1
    assert (B.CSRC / "grad_guard.hip").exists() and '#include "../../include/maestro_hip.h"' in (B.CSRC / "grad_guard.hip").read_text()


def test_partial_rows_depend_on_n_alone(lib):
    assert [lib.mh_grad_sumsq_partial_rows(n) for n in (-4, 0, 4, G.C - 4, G.C, G.C + 4, 257 * G.C + 12, 1 << 34)] == \
        [0, 0, 1, 1, 1, 2, 258, 1 << 20]
    assert [G.rows_of(n) for n in G.SIZES] == [lib.mh_grad_sumsq_partial_rows(n) for n in G.SIZES]


def test_bad_arguments_are_refused_before_the_gpu_is_touched(lib):
    """Device pointers are never dereferenced on the host and a refused call launches nothing: any non-null value will do."""
    vp = ctypes.c_void_p

    def partial(g=0x1000, n=64, p=0x2000, b=0x3000):
        return lib.mh_grad_sumsq_partial(vp(g), n, vp(p), vp(b), vp(0))

    for null in ("g", "p", "b"):
        assert partial(**{null: 0}) == -1 and b"null" in lib.mh_last_error()
    for n in (0, -4, 6, 63, G.C + 1):
        assert partial(n=n) == -1 and b"multiple of 4" in lib.mh_last_error(), n
    assert partial(g=0x1004) == -1 and b"16-byte" in lib.mh_last_error()

    def finish(p=0x1000, b=0x2000, rows=1, gs=1.0, mx=1.0, skip=1, lr=1e-3, b1=0.9, b2=0.99, h=0x3000, s=0x4000):
        return lib.mh_grad_guard_finish(vp(p), vp(b), rows, gs, mx, skip, lr, b1, b2, vp(h), vp(s), vp(0))

    for null in ("p", "b", "h", "s"):
        assert finish(**{null: 0}) == -1 and b"null" in lib.mh_last_error()
    for rows in (0, -1, (1 << 24) + 1):
        assert finish(rows=rows) == -1 and b"rows" in lib.mh_last_error()
    for bad in (dict(gs=float("nan")), dict(gs=float("inf")), dict(mx=float("nan")), dict(mx=float("inf")), dict(lr=float("nan"))):
        assert finish(**bad) == -1 and b"finite" in lib.mh_last_error(), bad
    for bad in (dict(b1=1.0), dict(b1=-0.1), dict(b2=1.5), dict(b2=float("nan"))):
        assert finish(**bad) == -1 and b"[0, 1)" in lib.mh_last_error(), bad


def test_wrapper_wants_a_gpu_and_whole_quads():
    from maestro_amd import hip
    with pytest.raises(hip.HipExtensionError, match="multiple of 4"):
        hip.GradGuard(6, "cpu")
    with pytest.raises(hip.HipExtensionError, match="multiple of 4"):
        hip.GradGuard(0, "cpu")
    with pytest.raises(hip.HipExtensionError, match="needs a GPU"):
        hip.GradGuard(64, "cpu")


# ------------------------------------------------------------------------------------------------ the switches, the refusals
def test_switch_resolution(monkeypatch):
    from maestro_amd.train.optim import resolve_grad_guard
    monkeypatch.delenv("MAESTRO_MAX_GRAD_NORM", raising=False)
    monkeypatch.delenv("MAESTRO_SKIP_NONFINITE", raising=False)
    assert resolve_grad_guard() == (None, False) and resolve_grad_guard(None, None) == (None, False)
    assert resolve_grad_guard(1.5, True) == (1.5, True) and resolve_grad_guard(0.0, False) == (None, False)
    monkeypatch.setenv("MAESTRO_MAX_GRAD_NORM", "2.5")
    monkeypatch.setenv("MAESTRO_SKIP_NONFINITE", "1")
    assert resolve_grad_guard() == (2.5, True)
    assert resolve_grad_guard(1.0, False) == (1.0, False) and resolve_grad_guard(0.0, None) == (None, True)   # an explicit value wins
    monkeypatch.setenv("MAESTRO_SKIP_NONFINITE", "true")         # only "1" means on
    monkeypatch.setenv("MAESTRO_MAX_GRAD_NORM", "")
    assert resolve_grad_guard() == (None, False)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="max_grad_norm"):
            resolve_grad_guard(bad)
    monkeypatch.setenv("MAESTRO_MAX_GRAD_NORM", "-3")
    with pytest.raises(ValueError, match="max_grad_norm"):
        resolve_grad_guard()


GUARD_KW = (dict(max_grad_norm=1.0), dict(skip_nonfinite=True), dict(max_grad_norm=1.0, skip_nonfinite=True))


def test_refusals_that_need_no_gpu(monkeypatch):
    """All of them are ValueErrors raised before anything is built (the model is None: what follows an accepted configuration
    is the AttributeError of building an engine from it)."""
    from maestro_amd.train.trainer import PretrainLoop, SupervisedLoop
    for v in ("MAESTRO_MAX_GRAD_NORM", "MAESTRO_SKIP_NONFINITE", "MAESTRO_DTYPE", "MAESTRO_EXCHANGE", "MAESTRO_DETERMINISTIC"):
        monkeypatch.delenv(v, raising=False)
    for kw in GUARD_KW:
        with pytest.raises(ValueError, match="overlap_optimizer"):
            PretrainLoop(None, 1, "cpu", overlap_optimizer=True, **kw)
        with pytest.raises(ValueError, match="fp8"):
            PretrainLoop(None, 1, "cpu", dtype="fp8", **kw)
        with pytest.raises(ValueError, match="rs_ag"):
            PretrainLoop(None, 1, "cpu", exchange_mode="rs_ag", **kw)
        with pytest.raises(AttributeError):                      # accepted -- also in deterministic mode
            PretrainLoop(None, 1, "cpu", deterministic=True, **kw)
        with pytest.raises(AttributeError):
            SupervisedLoop(None, 1, "cpu", **kw)
    for loop in (PretrainLoop, SupervisedLoop):
        with pytest.raises(ValueError, match="max_grad_norm"):
            loop(None, 1, "cpu", max_grad_norm=-1.0)
    # without a guard none of the three is refused here (the loop goes on to build its engine)
    for kw in (dict(overlap_optimizer=True), dict(exchange_mode="rs_ag")):
        with pytest.raises(AttributeError):
            PretrainLoop(None, 1, "cpu", **kw)
    # the environment switches refuse the same way, and the environment's dtype / exchange mode count
    monkeypatch.setenv("MAESTRO_MAX_GRAD_NORM", "1.0")
    with pytest.raises(ValueError, match="overlap_optimizer"):
        PretrainLoop(None, 1, "cpu", overlap_optimizer=True)
    with pytest.raises(AttributeError):
        PretrainLoop(None, 1, "cpu", overlap_optimizer=True, max_grad_norm=0.0)      # an explicit 0 switches the guard off
    monkeypatch.delenv("MAESTRO_MAX_GRAD_NORM")
    monkeypatch.setenv("MAESTRO_SKIP_NONFINITE", "1")
    with pytest.raises(ValueError, match="rs_ag"):
        PretrainLoop(None, 1, "cpu", exchange_mode="rs_ag")
    monkeypatch.setenv("MAESTRO_EXCHANGE", "rs_ag")
    with pytest.raises(ValueError, match="rs_ag"):
        PretrainLoop(None, 1, "cpu")
    monkeypatch.delenv("MAESTRO_EXCHANGE")
    monkeypatch.setenv("MAESTRO_DTYPE", "fp8")
    with pytest.raises(ValueError, match="fp8"):
        PretrainLoop(None, 1, "cpu")
    monkeypatch.setenv("MAESTRO_MAX_GRAD_NORM", "nan")
    with pytest.raises(ValueError, match="max_grad_norm"):
        SupervisedLoop(None, 1, "cpu")


def test_fused_adamw_refuses_a_guard_with_an_fp8_plan():
    from types import SimpleNamespace

    from maestro_amd.train.optim import FusedAdamW
    flat = torch.zeros(8)
    eng = SimpleNamespace(store=SimpleNamespace(flat=flat, grad=flat.clone(), half=flat.bfloat16(), total=8), fp8=object())
    opt = FusedAdamW(eng, 1e-3)
    assert opt.guard is None
    with pytest.raises(ValueError, match="fp8"):
        opt.step(guard=SimpleNamespace(n=8))


# ------------------------------------------------------------------------------------------------ the restatement
def _torch_clip(g, max_norm, error_if_nonfinite=False):
    p = torch.nn.Parameter(torch.zeros(g.size))
    p.grad = torch.from_numpy(g.copy())
    norm = torch.nn.utils.clip_grad_norm_([p], max_norm, error_if_nonfinite=error_if_nonfinite)
    return float(norm), p.grad.numpy()


@pytest.mark.parametrize("n", [4, G.C - 4, G.C + 4, 3 * G.C + 260])
def test_reference_against_torch_clip_grad_norm(n):
    from maestro_amd import hip
    g = G.normal_draws(n, 1.0, seed=n)
    true = float(np.sqrt((g.astype(np.float64) ** 2).sum()))
    for max_norm in (0.5 * true, true, 2.0 * true):
        ref = hip.grad_guard_reference(g, 1.0, max_norm, True, 1e-3, 0.9, 0.99, 0, 0)
        tnorm, tgrad = _torch_clip(g, max_norm)
        assert ref["finite"] and ref["apply"] and ref["bad"] == 0 and (ref["t"], ref["skipped"]) == (1, 0)
        assert abs(float(ref["norm"]) - tnorm) <= 4 * 2.0 ** -24 * tnorm            # torch's norm is an fp32 reduction of its own
        want = min(1.0, max_norm / (tnorm + 1e-6))
        assert abs(float(ref["coef"]) - want) <= 6 * 2.0 ** -24
        assert (float(ref["coef"]) < 1.0) == (max_norm < true) or max_norm == true
        np.testing.assert_allclose(g * ref["coef"], tgrad, rtol=1e-6, atol=0)
        assert ref["hyper"].dtype == np.float32 and ref["hyper"][4] == 1.0 and ref["hyper"][3] == ref["coef"]
    off = hip.grad_guard_reference(g, 0.25, None, False, 1e-3, 0.9, 0.99, 7, 2)
    assert off["coef"] == 1.0 and abs(float(off["norm"]) - 0.25 * true) <= 2 * 2.0 ** -24 * true and off["hyper"][3] == np.float32(0.25)
    assert (off["t"], off["skipped"]) == (8, 2) and hip.grad_guard_reference(g, 1.0, -1.0, True, 1e-3, 0.9, 0.99, 0, 0)["coef"] == 1.0


@pytest.mark.parametrize("poison", [float("nan"), float("inf"), float("-inf")])
def test_reference_on_non_finite_gradients_is_torchs_error_if_nonfinite(poison):
    from maestro_amd import hip
    g = G.normal_draws(G.C + 4, 1.0)
    g[G.C] = poison
    with pytest.raises(RuntimeError, match="non-finite"):
        _torch_clip(g, 1.0, error_if_nonfinite=True)
    ref = hip.grad_guard_reference(g, 1.0, 1.0, True, 1e-3, 0.9, 0.99, 5, 1)
    assert not ref["finite"] and not ref["apply"] and ref["bad"] == 1 and list(ref["bad_rows"]) == [0, 1]
    assert ref["coef"] == 1.0 and (ref["t"], ref["skipped"]) == (5, 2) and ref["hyper"][4] == 0.0 and np.isfinite(ref["hyper"][:4]).all()
    keep = hip.grad_guard_reference(g, 1.0, 1.0, False, 1e-3, 0.9, 0.99, 5, 1)
    assert not keep["finite"] and keep["apply"] and keep["coef"] == 1.0 and (keep["t"], keep["skipped"]) == (6, 1) and keep["hyper"][4] == 1.0


def test_reference_counts_an_fp32_overflow_as_non_finite():
    from maestro_amd import hip
    g = np.full(64, 2.0 ** 70, dtype=np.float32)
    with pytest.raises(RuntimeError, match="non-finite"):
        _torch_clip(g, 1.0, error_if_nonfinite=True)
    ref = hip.grad_guard_reference(g, 1.0, 1.0, True, 1e-3, 0.9, 0.99, 0, 0)
    assert ref["bad"] == 0 and np.isinf(ref["norm"]) and not ref["finite"] and not ref["apply"] and np.isfinite(ref["hyper"]).all()
    zero = hip.grad_guard_reference(np.zeros(8, dtype=np.float32), 1.0, 1.0, True, 1e-3, 0.9, 0.99, 0, 0)
    assert zero["norm"] == 0 and zero["coef"] == 1.0 and zero["apply"] and np.isfinite(zero["hyper"]).all()


def test_reference_bias_corrections():
    from maestro_amd import hip
    g = np.ones(4, dtype=np.float32)
    for b1, b2 in ((0.9, 0.99), (0.9, 0.999)):
        for t in (1, 2, 64, 10 ** 4, 10 ** 6):
            h = hip.grad_guard_reference(g, 1.0, None, True, 1e-3, b1, b2, t - 1, 0)["hyper"]
            fb1, fb2 = float(np.float32(b1)), float(np.float32(b2))
            want1, want2 = -math.expm1(t * math.log(fb1)), math.sqrt(-math.expm1(t * math.log(fb2)))      # another route in fp64
            assert abs(float(h[1]) - want1) <= np.spacing(np.float32(want1)) and abs(float(h[2]) - want2) <= np.spacing(np.float32(want2))
            assert h[0] == np.float32(1e-3) and h[3] == 1.0 and h[4] == 1.0


# ------------------------------------------------------------------------------------------------ the teeth of the error bound
@pytest.mark.parametrize("scale", G.SCALES)
@pytest.mark.parametrize("n", [G.C - 4, G.C + 4, 3 * G.C + 260])
def test_the_emulated_tree_stays_inside_the_bound_and_mutations_leave_it(n, scale):
    g = G.normal_draws(n, scale)
    assert (g.astype(np.float64) ** 2 >= 2.0 ** -126).all() and np.isfinite(g.astype(np.float64) ** 2 * n).all()
    ratio = G.partial_error_ratio(G.emulate_partials(g), g)
    assert ratio <= 1.0, ratio
    for mutation in ("drop_lane", "bf16_squares"):
        broken = G.partial_error_ratio(G.emulate_partials(g, mutation), g)
        assert broken > 1.0, (mutation, broken)


def test_the_emulated_tree_is_exact_on_integers():
    for n in (4, G.C - 4, 3 * G.C + 260):
        g = G.integer_gradient(n)
        assert np.array_equal(G.emulate_partials(g).astype(np.int64), G.exact_partials(g))
    assert G.DEPTH == 28 and G.GAMMA < 1.7e-6
