"""Median-date selection on the GPU (csrc/staging.hip, include/maestro_hip.h) against the device-form numpy restatement
of tests/date_select_ref.py and against the reference's recording (tests/golden/date_select.npz).

Every call goes through ``run``: each operand sits in the middle of a poisoned allocation (tests/guards.py), the dates of a
sample before ``t_start`` and behind its last window hold poison (NaN for f32 data and scores, 0x7fff / 0xff for integers, masks
and dates), and the bands around inputs and outputs are compared bit for bit after the call.

Measured on an MI355X (worst error of the log path in float32 ulps of the result, against fp64): see profiles/date_select.md.
"""

from pathlib import Path

import numpy as np
import pytest
import torch

from tests import date_select_ref as ref
from tests import guards

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
ND, WINDOWS, CHANNELS, SIDES = (1, 3), (1, 2, 3, 8, 64), (1, 3), (1, 3, 5)
MASK_FLOOR = 30


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _poison(dtype):
    dtype = np.dtype(dtype)
    if dtype.kind == "f":
        return np.nan
    return 0xFF if dtype.itemsize == 1 else 0x7FFF


def _guard_in(gs, arr, name):
    """A numpy input as a guarded device view (uint16 travels as its bytes: torch has few uint16 kernels)."""
    if arr.dtype == np.uint16:
        return gs.inp(torch.from_numpy(arr.view(np.int16)), name=name).view(torch.uint16)
    return gs.inp(torch.from_numpy(arr), name=name)


def test_stager_selects_before_the_flips():
    """``BatchStager.stage(batch, flags, select=...)`` on a two-modality batch = the selection followed by the reference's flips
    (oracle.staging.transform_rasters) with the same flags; without ``select`` the call returns what it always did.  (Dense
    operands: the one test of this file above the guard-band banner.)"""
    from maestro_amd import hip
    from maestro_amd.train.staging import BatchStager, DateSelect, window_plan
    from oracle import staging as ost
    dev = _dev()
    rng = np.random.default_rng(21)
    B = 4  # noqa: N806
    s2 = make_batch(rng, np.uint16, 3, 8, 3, 5, 2)
    s1 = make_batch(rng, np.float32, 2, 3, 2, 5, 0)
    n_s2 = [s + 3 * w for s, w in zip(s2["t_start"], s2["t_win"])]
    ts, tw = window_plan(n_s2, 3, s2["t_start"])
    assert ts.tolist() == s2["t_start"] and tw.tolist() == s2["t_win"]
    select = {"s2": DateSelect(3, mask_threshold=MASK_FLOOR + 0.5, norm_fac=5000.0), "s1": DateSelect(2, norm_fac=5.0)}
    aerial = torch.rand(B, 1, 4, 12, 12)
    batch = {"aerial": aerial, "aerial_dates": torch.zeros(B, 1, 3, dtype=torch.int16),
             "s2": torch.from_numpy(s2["raw"].view(np.int16)).view(torch.uint16), "s2_dates": torch.from_numpy(s2["dates"]),
             "s2_t_start": ts, "s2_t_win": tw, "s2_mask": torch.from_numpy(s2["mask"]),
             "s1": torch.from_numpy(s1["raw"]), "s1_dates": torch.from_numpy(s1["dates"]),
             "s1_t_start": torch.tensor(s1["t_start"], dtype=torch.int32), "s1_t_win": torch.tensor(s1["t_win"], dtype=torch.int32),
             "label": torch.rand(B, 15)}
    flags = torch.tensor([0, 3, 5, 7], dtype=torch.uint8)
    stager = BatchStager(dev, rasters=["aerial", "s2", "s1"])
    for _ in range(3):       # laps the pinned ring
        out = stager.stage(batch, flags, select=select)
    torch.cuda.synchronize()
    assert set(out) == {"aerial", "aerial_dates", "s2", "s2_dates", "s1", "s1_dates", "label"}
    want = {"s2": expect(s2, mask_floor=MASK_FLOOR, norm_fac=5000.0), "s1": expect(s1, norm_fac=5.0)}
    for name, w in want.items():
        assert out[name].dtype == torch.float32 and out[f"{name}_dates"].dtype == torch.int16
        assert np.array_equal(out[f"{name}_dates"].cpu().numpy(), w[2]), name
        for b in range(B):
            flipped = ost.transform_rasters({name: w[1][b]}, int(flags[b]))[name]
            assert out[name][b].cpu().numpy().tobytes() == flipped.tobytes(), (name, b)
    # the wrapper on its own gives the un-flipped selection
    direct, _, _ = hip.select_dates(batch["s1"].to(dev), batch["s1_dates"].to(dev), s1["t_start"], s1["t_win"], 2, norm_fac=5.0)
    assert direct.cpu().numpy().tobytes() == want["s1"][1].tobytes()
    for b in range(B):
        assert np.array_equal(out["aerial"][b].cpu().numpy(), ost.transform_rasters({"a": aerial[b].numpy()}, int(flags[b]))["a"])
    assert torch.equal(out["label"].cpu(), batch["label"])
    # without `select`: today's behaviour, on a wire-format batch
    wire = {"aerial": aerial, "aerial_dates": batch["aerial_dates"], "s1": torch.from_numpy(want["s1"][1]), "label": batch["label"]}
    plain = stager.stage(wire, flags)
    torch.cuda.synchronize()
    assert set(plain) == set(wire)
    for key in ("aerial", "s1"):
        for b in range(B):
            assert np.array_equal(plain[key][b].cpu().numpy(), ost.transform_rasters({"r": wire[key][b].numpy()}, int(flags[b]))["r"])
    assert torch.equal(stager.stage(wire, None)["aerial"].cpu(), aerial) and torch.equal(plain["label"].cpu(), batch["label"])


# ------------------------------------------------------------------------------------------------ guard bands (tests/guards.py)
# The ledger of tests/guards.py counts the calls below this banner: every test below reaches the kernel through ``run``, whose
# operands sit in a GuardSet.
def run(dev, raw, dates, t_start, t_win, nd, mask=None, mask_floor=0, scores=None, log_scale=False, norm_fac=None):
    """hip.select_dates on guarded operands, bands checked -> (index, raster, dates) as numpy."""
    from maestro_amd import hip
    B, _, C, S, _ = raw.shape  # noqa: N806
    gs = guards.GuardSet(dev)
    d_raw = _guard_in(gs, raw, "raw")
    d_dates = _guard_in(gs, dates, "dates")
    d_mask = None if mask is None else _guard_in(gs, mask, "mask")
    d_scores = None if scores is None else _guard_in(gs, scores, "scores")
    d_ts = gs.inp(torch.tensor(t_start, dtype=torch.int32), fill=0, name="t_start")      # (a band value that is a VALID plan)
    d_tw = gs.inp(torch.tensor(t_win, dtype=torch.int32), fill=1, name="t_win")
    out = gs.out((B, nd, C, S, S), torch.float32, name="out")
    out_dates = gs.out((B, nd, 3), torch.int16, name="out_dates")
    out_index = gs.out((B, nd), torch.int32, name="out_index")
    hip.select_dates(d_raw, d_dates, t_start, t_win, nd, mask=d_mask, mask_floor=mask_floor, scores=d_scores, log_scale=log_scale,
                     norm_fac=norm_fac, t_start_dev=d_ts, t_win_dev=d_tw, out=out, out_dates=out_dates, out_index=out_index)
    gs.check()
    return out_index.cpu().numpy(), out.cpu().numpy(), out_dates.cpu().numpy()


def make_batch(rng, dtype, nd, W, C, S, Cm, padding="poison"):  # noqa: N803
    """Four samples with their own t_start / W_b: sample 0 has a tiny value range (ties -> lowest index); with a mask, sample 0 is
    sparsely clouded, sample 1 has exactly one clean date per window (different pixels masked per date), sample 2's window 0 is
    dirty throughout (mask ignored), sample 3 has ONE pixel masked in all dates but one.  Mask values at or below MASK_FLOOR are
    sprinkled everywhere: they mask nothing."""
    dtype = np.dtype(dtype)
    t_win = [W, W, max(1, W - 1), W]
    t_start = [int(rng.integers(0, 3)) for _ in range(4)]
    Tmax = max(s + nd * w for s, w in zip(t_start, t_win)) + 2  # noqa: N806
    B = 4  # noqa: N806
    pad = _poison(dtype) if padding == "poison" else 0
    raw = np.full((B, Tmax, C, S, S), pad, dtype=dtype)
    dates = np.full((B, Tmax, 3), 0x7FFF if padding == "poison" else 0, dtype=np.int16)
    mask = None if not Cm else np.full((B, Tmax, Cm, S, S), 0xFF if padding == "poison" else 0, dtype=np.uint8)
    for b in range(B):
        sl = slice(t_start[b], t_start[b] + nd * t_win[b])
        n = nd * t_win[b]
        if dtype.kind == "f":
            x = np.exp(rng.uniform(-3.0, 6.0, size=(n, C, S, S))) if b else rng.integers(0, 3, size=(n, C, S, S))
        else:
            info = np.iinfo(dtype)
            x = rng.integers(info.min, info.max + 1, size=(n, C, S, S)) if b else rng.integers(0, 3, size=(n, C, S, S))
        raw[b, sl] = x.astype(dtype)
        dates[b, sl] = rng.integers(-3000, 3000, size=(n, 3))
        if mask is None:
            continue
        m = (rng.random((n, Cm, S, S)) < 0.3) * rng.integers(0, MASK_FLOOR + 1, size=(n, Cm, S, S))      # harmless values
        hot = lambda k: rng.integers(MASK_FLOOR + 1, 101, size=k)  # noqa: E731
        if b == 0:
            m = np.where(rng.random(m.shape) < 0.04, hot(m.shape), m)
        for j in range(nd):
            w0 = j * t_win[b]
            keep = w0 + int(rng.integers(0, t_win[b]))
            for w in range(w0, w0 + t_win[b]):
                if b == 1 and w != keep:
                    m[w, rng.integers(0, Cm), rng.integers(0, S), rng.integers(0, S)] = hot(1)[0]
                if b == 2 and j == 0:
                    m[w, rng.integers(0, Cm), rng.integers(0, S), rng.integers(0, S)] = hot(1)[0]
                if b == 3 and w != keep:
                    m[w, Cm - 1, S - 1, 0] = hot(1)[0]
        mask[b, sl] = m
    return dict(raw=raw, dates=dates, mask=mask, t_start=t_start, t_win=t_win, nd=nd)


def expect(batch, **kw):
    return ref.select_batch(ref.select_device, batch["raw"], batch["dates"], batch["t_start"], batch["t_win"], batch["nd"],
                            mask=batch["mask"], **kw)


def shape_grid():
    """Every (nd, W) with the channel counts, raster sides and mask channels cycling through all their values."""
    k = 0
    for nd in ND:
        for W in WINDOWS:  # noqa: N806
            for C in CHANNELS:  # noqa: N806
                for S in SIDES:  # noqa: N806
                    yield nd, W, C, S, (0, 1, 2)[k % 3]
                    k += 1


@pytest.mark.parametrize("dtype", [np.uint8, np.int16, np.uint16])
def test_integer_types_match_the_device_form_bit_for_bit(dtype):
    dev = _dev()
    rng = np.random.default_rng(np.dtype(dtype).itemsize * 7 + np.dtype(dtype).kind.encode()[0])
    seen_ignored = 0
    for nd, W, C, S, Cm in shape_grid():  # noqa: N806
        bt = make_batch(rng, dtype, nd, W, C, S, Cm)
        want = expect(bt, mask_floor=MASK_FLOOR, norm_fac=5000.0)
        got = run(dev, bt["raw"], bt["dates"], bt["t_start"], bt["t_win"], nd, mask=bt["mask"], mask_floor=MASK_FLOOR, norm_fac=5000.0)
        where = (np.dtype(dtype).name, nd, W, C, S, Cm)
        assert np.array_equal(got[0], want[0]), where
        assert got[1].tobytes() == want[1].tobytes(), where
        assert np.array_equal(got[2], want[2]), where
        if Cm:
            m = bt["mask"][2, bt["t_start"][2]: bt["t_start"][2] + bt["t_win"][2]] > MASK_FLOOR
            seen_ignored += int(m.reshape(m.shape[0], -1).any(axis=1).all())
    assert seen_ignored >= 10


def test_f32_index_and_plain_output_match_the_device_form():
    """fp32 median and deviations, fp64 sum in element order: the index is form (b)'s bit for bit (W = 2 and the tiny-range
    sample are ties or near-ties), and without log the raster is numpy's division bit for bit."""
    dev = _dev()
    rng = np.random.default_rng(32)
    for nd, W, C, S, Cm in shape_grid():  # noqa: N806
        bt = make_batch(rng, np.float32, nd, W, C, S, Cm)
        for nf in (None, 5.0):
            want = expect(bt, mask_floor=MASK_FLOOR, norm_fac=nf)
            got = run(dev, bt["raw"], bt["dates"], bt["t_start"], bt["t_win"], nd, mask=bt["mask"], mask_floor=MASK_FLOOR, norm_fac=nf)
            assert np.array_equal(got[0], want[0]), (nd, W, C, S, Cm)
            assert got[1].tobytes() == want[1].tobytes() and np.array_equal(got[2], want[2]), (nd, W, C, S, Cm, nf)


def _log_errors(chosen, got32, numpy32, norm_fac):
    """Worst error of the device's and of numpy's float32 ``log(max(x, 1e-10)) / norm_fac`` in ulps of the fp64 result."""
    x = np.maximum(chosen.astype(np.float32), np.float32(1e-10)).astype(np.float64)
    exact = np.log(x) / (1.0 if norm_fac is None else float(norm_fac))
    return float(ref.ulp_error(got32, exact).max()), float(ref.ulp_error(numpy32, exact).max())


def _log_bound(numpy_worst):
    return max(2.0, 2.0 * numpy_worst)


def test_log_scale_is_as_accurate_as_numpy(observed):
    """``logf(max(x, 1e-10f)) / norm_fac`` against fp64 on the same inputs: the device's worst error may be at most twice numpy's
    own float32 error (floor 2 ulp).  Inputs are log-uniform in [e^-23, e^12] with zeros, negatives and values below the clamp."""
    dev = _dev()
    rng = np.random.default_rng(5)
    B, nd, W, C, S = 8, 3, 3, 3, 37  # noqa: N806
    raw = np.exp(rng.uniform(-23.0, 12.0, size=(B, nd * W, C, S, S))).astype(np.float32)
    raw[:, :, 0, 0, :8] = np.array([0.0, -1.0, 1e-11, 1e-10, 1.0, 1e-30, 9.9e-11, 3.0e38], dtype=np.float32)
    dates = rng.integers(0, 3000, size=(B, nd * W, 3)).astype(np.int16)
    worst = {}
    for nf in (5.0, None):
        want = ref.select_batch(ref.select_device, raw, dates, [0] * B, [W] * B, nd, log_scale=True, norm_fac=nf)
        got = run(dev, raw, dates, [0] * B, [W] * B, nd, log_scale=True, norm_fac=nf)
        assert np.array_equal(got[0], want[0])
        mine, numpys = _log_errors(want[3], got[1], want[1], nf)
        print(f"log_scale, norm_fac {nf}: device {mine:.3f} ulp, numpy {numpys:.3f} ulp on {want[3].size} values")
        observed("test_log_scale_is_as_accurate_as_numpy", f"device_ulp_norm_fac_{nf}", mine)
        observed("test_log_scale_is_as_accurate_as_numpy", f"numpy_ulp_norm_fac_{nf}", numpys)
        worst[nf] = (mine, numpys)
    for nf, (mine, numpys) in worst.items():
        assert mine <= _log_bound(numpys), (nf, mine, numpys)
    # integer data takes the same path: u16 with zeros (clamped)
    raw16 = rng.integers(0, 65536, size=(2, 6, 2, 5, 5)).astype(np.uint16)
    raw16[:, :, 0, 0, 0] = 0
    want = ref.select_batch(ref.select_device, raw16, dates[:2, :6], [0, 0], [3, 3], 2, log_scale=True, norm_fac=5.0)
    got = run(dev, raw16, dates[:2, :6], [0, 0], [3, 3], 2, log_scale=True, norm_fac=5.0)
    mine, numpys = _log_errors(want[3], got[1], want[1], 5.0)
    assert np.array_equal(got[0], want[0]) and mine <= _log_bound(numpys), (mine, numpys)


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
    return cases


def test_golden_cases_reproduce_the_reference(golden, observed):
    """Index, dates and raster as ``GenericDataset.preprocess_raster`` recorded them (u8 / i16 / u16 with and without masks,
    random_dates, f32 with log_scale); the loader-side parameters go through ``DateSelect`` and ``draw_date_scores``."""
    from maestro_amd.train.staging import DateSelect, draw_date_scores
    dev = _dev()
    assert len(golden) >= 12
    for name, c in golden.items():
        T, C, S, _ = c["raw"].shape  # noqa: N806
        sel = DateSelect(num_dates=c["nd"], mask_threshold=c["thr"], log_scale=c["log"], norm_fac=c["nf"])
        scores = None
        if c["seed"] is not None:
            scores = np.full((1, T), np.nan)
            drawn = draw_date_scores(np.random.default_rng(c["seed"]), c["nd"], c["W"], C, S, c["raw"].dtype)
            scores[0, c["start"]: c["start"] + drawn.size] = drawn.reshape(-1)
        mask = c["mask"][None] if c["mask"] is not None and sel.use_mask else None
        idx, out, dates = run(dev, c["raw"][None], c["dates"][None], [c["start"]], [c["W"]], c["nd"], mask=mask,
                              mask_floor=sel.mask_floor, scores=scores, log_scale=sel.log_scale, norm_fac=sel.norm_fac)
        assert np.array_equal(idx[0], c["index"]), name
        assert np.array_equal(dates[0], c["out_dates"]), name
        if not c["log"]:
            assert out[0].tobytes() == c["out"].tobytes(), name
        else:
            chosen = c["raw"][c["start"]: c["start"] + c["nd"] * c["W"]].reshape(c["nd"], c["W"], C, S, S)[np.arange(c["nd"]), c["index"]]
            mine, numpys = _log_errors(chosen, out[0], c["out"], c["nf"])
            print(f"{name}: device {mine:.3f} ulp, the reference's numpy {numpys:.3f} ulp")
            observed("test_golden_cases_reproduce_the_reference", f"{name}_device_ulp", mine)
            assert mine <= _log_bound(numpys), (name, mine, numpys)


@pytest.mark.parametrize("dtype", [np.int16, np.float32])
def test_given_scores_choose_the_lowest_clean_score(dtype):
    """random_dates: the median is not consulted -- every date but the expected one holds poison (NaN / 0x7fff), the lowest score
    of all sits on a dirty date, and one window is dirty throughout (its mask is ignored)."""
    dev = _dev()
    rng = np.random.default_rng(9)
    B, nd, W, C, S, Cm = 3, 3, 8, 3, 5, 2  # noqa: N806
    Tmax = nd * W + 3  # noqa: N806
    t_start, t_win = [0, 2, 3], [W, W, W]
    raw = np.full((B, Tmax, C, S, S), _poison(dtype), dtype=dtype)
    dates = rng.integers(0, 3000, size=(B, Tmax, 3)).astype(np.int16)
    mask = np.zeros((B, Tmax, Cm, S, S), dtype=np.uint8)
    scores = np.full((B, Tmax), np.nan)
    want_idx = np.zeros((B, nd), dtype=np.int32)
    for b in range(B):
        for j in range(nd):
            t0 = t_start[b] + j * W
            s = rng.permutation(W).astype(np.float64) / W + 0.01
            order = np.argsort(s)
            if j == 1 and b == 1:                        # all dirty: the mask is ignored, the lowest score wins
                mask[b, t0: t0 + W, 1, 2, 2] = 100
                pick = order[0]
            else:                                        # the two lowest are dirty: the third wins
                mask[b, t0 + order[0], 0, 0, 0] = 1
                mask[b, t0 + order[1], Cm - 1, S - 1, S - 1] = 77
                pick = order[2]
            scores[b, t0: t0 + W] = s
            raw[b, t0 + pick] = (rng.uniform(1, 100, size=(C, S, S))).astype(dtype)
            want_idx[b, j] = pick
    idx, out, odates = run(dev, raw, dates, t_start, t_win, nd, mask=mask, mask_floor=0, scores=scores, norm_fac=5000.0)
    assert np.array_equal(idx, want_idx)
    for b in range(B):
        for j in range(nd):
            t = t_start[b] + j * W + want_idx[b, j]
            assert out[b, j].tobytes() == (raw[b, t].astype(np.float32) / np.float32(5000.0)).tobytes()
            assert np.array_equal(odates[b, j], dates[b, t])
    want = ref.select_batch(ref.select_device, raw, dates, t_start, t_win, nd, mask=mask, scores=scores, mask_floor=0, norm_fac=5000.0)
    assert np.array_equal(idx, want[0])


@pytest.mark.parametrize("dtype", [np.uint8, np.int16, np.float32])
def test_poisoned_padding_changes_nothing_and_bands_stay_intact(dtype):
    """``run`` puts every operand between poisoned bands and checks them (inputs bit for bit, the bands behind ``out``,
    ``out_dates`` and ``out_index``); here the SAME windows are run once with poison and once with zeros in the dates before
    ``t_start`` and behind the last window: the outputs must agree bit for bit and hold no poison."""
    dev = _dev()
    for nd, W, C, S, Cm in ((3, 8, 3, 5, 2), (1, 64, 1, 3, 1), (3, 3, 3, 3, 0)):  # noqa: N806
        a = make_batch(np.random.default_rng(77), dtype, nd, W, C, S, Cm, padding="poison")
        b = make_batch(np.random.default_rng(77), dtype, nd, W, C, S, Cm, padding="zeros")
        ra = run(dev, a["raw"], a["dates"], a["t_start"], a["t_win"], nd, mask=a["mask"], mask_floor=MASK_FLOOR, norm_fac=255.0)
        rb = run(dev, b["raw"], b["dates"], b["t_start"], b["t_win"], nd, mask=b["mask"], mask_floor=MASK_FLOOR, norm_fac=255.0)
        for x, y in zip(ra, rb):
            assert x.tobytes() == y.tobytes()
        assert np.isfinite(ra[1]).all() and (ra[0] >= 0).all() and (ra[0] < W).all()


def test_same_call_twice_gives_identical_bytes():
    dev = _dev()
    for dtype in (np.uint16, np.float32):
        bt = make_batch(np.random.default_rng(4), dtype, 3, 64, 3, 5, 2)
        first = run(dev, bt["raw"], bt["dates"], bt["t_start"], bt["t_win"], 3, mask=bt["mask"], mask_floor=MASK_FLOOR, log_scale=True,
                    norm_fac=5.0)
        again = run(dev, bt["raw"], bt["dates"], bt["t_start"], bt["t_win"], 3, mask=bt["mask"], mask_floor=MASK_FLOOR, log_scale=True,
                    norm_fac=5.0)
        for x, y in zip(first, again):
            assert x.tobytes() == y.tobytes()


def test_more_than_one_chunk_per_raster():
    """C * S * S beyond one chunk of elements (the PASTIS-HD shape: 10 x 16 x 16 = 2560), masked, int16 and f32."""
    dev = _dev()
    rng = np.random.default_rng(16)
    for dtype in (np.int16, np.float32):
        bt = make_batch(rng, dtype, 2, 4, 10, 16, 1)
        want = expect(bt, mask_floor=MASK_FLOOR, norm_fac=10000.0)
        got = run(dev, bt["raw"], bt["dates"], bt["t_start"], bt["t_win"], 2, mask=bt["mask"], mask_floor=MASK_FLOOR, norm_fac=10000.0)
        assert np.array_equal(got[0], want[0]) and got[1].tobytes() == want[1].tobytes() and np.array_equal(got[2], want[2])
