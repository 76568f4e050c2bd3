"""Median-date selection, the parts that need no GPU: the argument checks of mh_select_dates, the window plan and the random_dates
draws of maestro_amd/train/staging.py, and the numpy restatements of tests/date_select_ref.py against each other and against
the reference's recording (tests/golden/date_select.npz, scripts/gen_date_select_golden.py)."""

import ctypes
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import date_select_ref as ref

ROOT = Path(__file__).resolve().parent.parent
F32_MARGIN = 1e-3


@pytest.fixture(scope="module")
def lib():
    from maestro_amd.csrc.build import LIB, build
    if not LIB.exists():
        build()
    handle = ctypes.CDLL(str(LIB))
    handle.mh_last_error.restype = ctypes.c_char_p
    return handle


@pytest.fixture(scope="module")
def golden():
    g = np.load(ROOT / "tests" / "golden" / "date_select.npz")
    cases = {}
    for name in map(str, g["names"]):
        c = {k.split("__", 1)[1]: g[k] for k in g.files if k.startswith(name + "__")}
        c["start"], c["W"], c["nd"] = map(int, c["plan"])
        thr, log, nf, seed = c["params"]
        c.update(thr=float(thr), log=bool(log), nf=float(nf) if nf > 0 else None, seed=int(seed) if seed >= 0 else None)
        c.setdefault("mask", None)
        cases[name] = c
    assert len(cases) >= 12
    return cases


def _abi_call(lib, raw=0x1000, code=1, w_max=4, nd=2, Tmax=16):  # noqa: N803
    """Pointers are never dereferenced on the host and a refused call launches nothing: any non-null value will do."""
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.mh_select_dates.argtypes = [vp, ci, vp, ci, ci, vp, vp, vp, ci, vp, vp, vp, vp, ci, ci, ci, ctypes.c_long, ci, ci,
                                    ctypes.c_float, vp]
    lib.mh_select_dates.restype = ci
    p = vp(0x1000)
    return lib.mh_select_dates(vp(raw), code, vp(0), 0, 0, p, p, p, w_max, vp(0), p, p, p, 2, Tmax, nd, 75, 25, 0, 0.0, vp(0))


def test_bad_arguments_are_refused_before_the_gpu_is_touched(lib):
    assert _abi_call(lib, w_max=0) == -1 and b"window of 0" in lib.mh_last_error()
    assert _abi_call(lib, w_max=65) == -1 and b"window of 65" in lib.mh_last_error()
    assert _abi_call(lib, code=4) == -1 and b"element code 4" in lib.mh_last_error()
    assert _abi_call(lib, code=-1) == -1
    assert _abi_call(lib, raw=0) == -1 and b"null" in lib.mh_last_error()
    assert _abi_call(lib, w_max=4, nd=5, Tmax=16) == -1 and b"do not fit" in lib.mh_last_error()


def test_wrapper_validates_the_window_plan_from_host_copies():
    """CPU tensors: a call that got past the validation would raise "need GPU tensors" instead."""
    from maestro_amd import hip
    raw = torch.zeros(2, 16, 3, 5, 5, dtype=torch.int16)
    dates = torch.zeros(2, 16, 3, dtype=torch.int16)
    with pytest.raises(hip.HipExtensionError, match=r"windows of 0 \.\.\. 4 dates"):
        hip.select_dates(raw, dates, [0, 0], [4, 0], 2)
    with pytest.raises(hip.HipExtensionError, match=r"windows of 4 \.\.\. 65 dates"):
        hip.select_dates(raw, dates, [0, 0], [4, 65], 2)
    with pytest.raises(hip.HipExtensionError, match="reach outside"):
        hip.select_dates(raw, dates, [0, 9], [4, 4], 2)           # 9 + 2 * 4 > 16
    with pytest.raises(hip.HipExtensionError, match="reach outside"):
        hip.select_dates(raw, dates, [-1, 0], [4, 4], 2)
    with pytest.raises(hip.HipExtensionError, match="raw dtype"):
        hip.select_dates(raw.to(torch.int32), dates, [0, 0], [4, 4], 2)
    with pytest.raises(hip.HipExtensionError, match="one value per sample"):
        hip.select_dates(raw, dates, [0], [4], 2)
    with pytest.raises(hip.HipExtensionError, match="GPU tensors"):
        hip.select_dates(raw, dates, [0, 8], [4, 4], 2, t_start_dev=torch.zeros(2, dtype=torch.int32),
                         t_win_dev=torch.zeros(2, dtype=torch.int32))


def test_window_plan_is_the_reference_s(golden):
    """dataset.py:92-104: start in 0 ... T % nd, end = start + nd * (T // nd) <= T."""
    from maestro_amd.train.staging import window_plan
    for T, nd in ((26, 3), (17, 2), (9, 4), (31, 3), (64, 16), (16, 16), (130, 16)):  # noqa: N806
        for start in range(T % nd + 1):
            ts, tw = window_plan([T], nd, [start])
            assert ts.dtype == tw.dtype == torch.int32
            assert (int(ts), int(tw)) == (start, T // nd) and start + nd * (T // nd) <= T
        with pytest.raises(ValueError):
            window_plan([T], nd, [T % nd + 1])
    ts, tw = window_plan([26, 17, 31], 3, [2, 0, 1])
    assert ts.tolist() == [2, 0, 1] and tw.tolist() == [8, 5, 10]
    with pytest.raises(ValueError):
        window_plan([2], 3, [0])
    for c in golden.values():        # the plans the reference ran with
        ts, tw = window_plan([len(c["raw"])], c["nd"], [c["start"]])
        assert (int(ts), int(tw)) == (c["start"], c["W"])


def test_date_select_from_config():
    import maestro_amd.conf as conf
    from maestro_amd.train.staging import DateSelect
    s2 = conf.DatasetsConfig(name_dataset="treesatai_ts").dataset.inputs["s2"]
    sel = DateSelect.from_config(s2)
    assert (sel.num_dates, sel.mask_threshold, sel.log_scale, sel.norm_fac) == (s2.num_dates, s2.mask_threshold, s2.log_scale, s2.norm_fac)
    assert sel.use_mask and sel.mask_floor == 0
    assert not DateSelect(4, mask_threshold=100.0).use_mask and DateSelect(4, mask_threshold=99.5).use_mask
    assert DateSelect(4, mask_threshold=30.5).mask_floor == 30 and DateSelect(4, mask_threshold=-0.5).mask_floor == -1


def test_draw_date_scores_reproduces_the_reference_s_draw(golden):
    from maestro_amd.train.staging import draw_date_scores
    seeded = {n: c for n, c in golden.items() if c["seed"] is not None}
    assert {c["raw"].dtype.kind for c in seeded.values()} >= {"i", "u", "f"}
    for name, c in seeded.items():
        _, C, S, _ = c["raw"].shape  # noqa: N806
        got = draw_date_scores(np.random.default_rng(c["seed"]), c["nd"], c["W"], C, S, c["raw"].dtype)
        assert got.dtype == np.float64 and got.shape == (c["nd"], c["W"])
        clean = ~np.isnan(c["ref_scores"])          # the reference's score of a dirty date is NaN
        assert clean.sum() >= c["nd"] and np.array_equal(got[clean], c["ref_scores"][clean]), name


def _golden_kwargs(c, with_scores=True):
    scores = None
    if c["seed"] is not None and with_scores:
        scores = np.full(len(c["raw"]), np.nan)
        flat = c["ref_scores"].reshape(-1)
        scores[c["start"]: c["start"] + flat.size] = np.where(np.isnan(flat), 0.0, flat)      # a dirty date's score must not matter
    return dict(mask=c["mask"], scores=scores, log_scale=c["log"], norm_fac=c["nf"])


def test_both_forms_reproduce_the_integer_golden_cases(golden):
    ints = {n: c for n, c in golden.items() if c["raw"].dtype.kind in "iu"}
    assert {c["raw"].dtype for c in ints.values()} == {np.dtype(np.uint8), np.dtype(np.int16), np.dtype(np.uint16)}
    for name, c in ints.items():
        a = ref.select_reference(c["raw"], c["dates"], c["start"], c["W"], c["nd"], mask_threshold=c["thr"], **_golden_kwargs(c))
        b = ref.select_device(c["raw"], c["dates"], c["start"], c["W"], c["nd"], mask_floor=int(np.floor(c["thr"])), **_golden_kwargs(c))
        for form in (a, b):
            assert np.array_equal(form[0], c["index"]), name
            assert form[1].tobytes() == c["out"].tobytes(), name
            assert np.array_equal(form[2], c["out_dates"]), name


def random_integer_window(rng):
    """One window with everything that can go wrong for an integer median: tiny value ranges (ties), offsets, masks with clean,
    dirty and all-dirty windows, one or two mask channels."""
    dtype = [np.uint8, np.int16, np.uint16][rng.integers(0, 3)]
    W, C, S, nd = int(rng.integers(1, 10)), int(rng.integers(1, 4)), int(rng.integers(1, 5)), int(rng.integers(1, 3))  # noqa: N806
    start, tail = int(rng.integers(0, 3)), int(rng.integers(0, 3))
    T = start + nd * W + tail  # noqa: N806
    info = np.iinfo(dtype)
    span = [1, 2, 5, 300, 70000][rng.integers(0, 5)]
    lo = int(rng.integers(info.min, max(info.min + 1, info.max - span)))
    raw = rng.integers(lo, min(info.max, lo + span) + 1, size=(T, C, S, S)).astype(dtype)
    dates = rng.integers(0, 3000, size=(T, 3)).astype(np.int16)
    mask = None
    if rng.integers(0, 3):
        Cm = int(rng.integers(1, 3))  # noqa: N806
        density = [0.0, 0.02, 0.2, 1.0][rng.integers(0, 4)]
        mask = (rng.random((T, Cm, S, S)) < density).astype(np.uint8) * rng.integers(1, 101, size=(T, Cm, S, S)).astype(np.uint8)
    return raw, dates, start, W, nd, mask


def test_device_form_equals_reference_form_on_random_integer_windows():
    rng = np.random.default_rng(20240607)
    n, masked, ignored, tied = 0, 0, 0, 0
    while n < 600:
        raw, dates, start, W, nd, mask = random_integer_window(rng)  # noqa: N806
        thr = [0.0, 30.5, 99.0][rng.integers(0, 3)]
        a = ref.select_reference(raw, dates, start, W, nd, mask=mask, mask_threshold=thr, norm_fac=255.0)
        b = ref.select_device(raw, dates, start, W, nd, mask=mask, mask_floor=int(np.floor(thr)), norm_fac=255.0)
        assert np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes() and np.array_equal(a[2], b[2])
        n += nd
        if mask is not None:
            dirty = (mask[start: start + nd * W] > thr).reshape(nd, W, -1).any(axis=2)
            masked += int((dirty.any(axis=1) & ~dirty.all(axis=1)).sum())
            ignored += int(dirty.all(axis=1).sum())
        tied += int((b[0] > 0).sum())
    assert masked >= 50 and ignored >= 50 and tied >= 100      # the generator reaches the cases it is meant to


def test_f32_golden_cases_meet_the_margin_condition(golden):
    """The device sums float scores in fp64, the reference in fp32: they must agree wherever the winner is clear, and the fixture
    holds only such windows (W >= 3, winner below the runner-up by more than 1e-3 relative)."""
    floats = {n: c for n, c in golden.items() if c["raw"].dtype == np.float32}
    assert len(floats) >= 2 and any(c["log"] for c in floats.values())
    for name, c in floats.items():
        assert c["W"] >= 3, name
        for j in range(c["nd"]):
            s = np.sort(c["ref_scores"][j][~np.isnan(c["ref_scores"][j])])
            assert len(s) >= 1 and (len(s) == 1 or s[1] - s[0] > F32_MARGIN * s[1]), (name, j)
        if c["seed"] is None:        # and the device's form picks the reference's dates
            b = ref.select_device(c["raw"], c["dates"], c["start"], c["W"], c["nd"], mask_floor=int(np.floor(c["thr"])),
                                  **_golden_kwargs(c))
            assert np.array_equal(b[0], c["index"]) and b[1].tobytes() == c["out"].tobytes(), name
