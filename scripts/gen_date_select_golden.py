"""Generate tests/golden/date_select.npz by running the REFERENCE's own ``GenericDataset.preprocess_raster``
(maestro/dataset/dataset.py:125-222) on small synthetic time series.  TEST INFRASTRUCTURE; run where the reference is at hand:

    PYTHONDONTWRITEBYTECODE=1 python scripts/gen_date_select_golden.py

The reference is imported with the non-arithmetic stubs of oracle/gen_golden.py.  Unmasked cases go through its ``.npy`` branch
(real files in a temporary directory); masked cases through its ``.h5`` branch, whose mask is 4-D, with an in-memory stand-in
for ``h5py.File`` (a dict of arrays: it computes nothing).  ``numpy.nanargmin`` is wrapped for the duration of a call so that
the scores the reference compares, and the indices it picks, are recorded as it computed them.

Only arrays are stored: per case the cropped raw series, mask and dates (what a loader would hand to the stager), the window
plan, the parameters, and the reference's scores, chosen indices, output raster and output dates.
"""

from __future__ import annotations

import sys
import tempfile
from pathlib import Path

sys.dont_write_bytecode = True
REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

import numpy as np  # noqa: E402

OUT = REPO / "tests" / "golden" / "date_select.npz"
F32_MARGIN = 1e-3          # f32 cases: in every window the winner is below the runner-up by more than this, relative


def import_dataset_class():
    from oracle.gen_golden import REFERENCE, _install_stubs
    _install_stubs()
    if str(REFERENCE) not in sys.path:
        sys.path.insert(0, str(REFERENCE))
    from maestro.dataset.dataset import GenericDataset
    return GenericDataset


class MemoryH5:
    """What the ``.h5`` branch needs of ``h5py.File``: a context manager that maps names to arrays."""
    store: dict = {}

    def __init__(self, path, mode="r"):
        self.path = path

    def __enter__(self):
        return MemoryH5.store

    def __exit__(self, *exc):
        return False


def case_table():
    """name -> dtype, T raw dates, nd, C, S, Cm (0 = unmasked), start offset, mask_threshold, random_dates seed (None = off),
    log_scale, norm_fac, value range."""
    c = {}

    def add(name, dtype, T, nd, C, S, Cm=0, start=0, thr=0.0, seed=None, log=False, nf=None, lo=0, hi=255):  # noqa: N803
        c[name] = dict(dtype=np.dtype(dtype), T=T, nd=nd, C=C, S=S, Cm=Cm, start=start, thr=thr, seed=seed, log=log, nf=nf, lo=lo, hi=hi)

    add("u8_plain", np.uint8, 26, 3, 3, 5, start=1, nf=255.0)
    add("u8_mask", np.uint8, 26, 3, 3, 5, Cm=2, start=2, thr=0.0, nf=255.0)
    add("u8_ties", np.uint8, 20, 4, 2, 3, lo=0, hi=3)
    add("u8_ties_mask", np.uint8, 24, 4, 2, 3, Cm=1, lo=0, hi=2, thr=30.5)
    add("i16_plain", np.int16, 17, 2, 3, 5, start=1, nf=5000.0, lo=-3000, hi=12000)
    add("i16_mask", np.int16, 31, 3, 10, 6, Cm=2, start=1, thr=0.0, nf=5000.0, lo=-3000, hi=12000)
    add("u16_plain", np.uint16, 9, 4, 1, 3, start=1, nf=10000.0, lo=0, hi=65535)
    add("u16_mask", np.uint16, 64, 1, 2, 3, Cm=1, thr=50.0, nf=10000.0, lo=20000, hi=65535)
    add("i16_random", np.int16, 17, 3, 3, 5, start=2, seed=11, nf=5000.0, lo=0, hi=9000)
    add("u8_random_mask", np.uint8, 24, 3, 2, 5, Cm=2, seed=12, nf=255.0)
    add("f32_log", np.float32, 13, 4, 2, 6, start=1, log=True, nf=5.0)
    add("f32_mask", np.float32, 21, 4, 3, 5, Cm=1, start=1, thr=0.0, nf=20.0)
    add("f32_random_log", np.float32, 16, 4, 2, 6, seed=13, log=True, nf=5.0)
    return c


def make_inputs(name, k):
    rng = np.random.default_rng(abs(hash_name(name)))
    T, C, S, H = k["T"], k["C"], k["S"], k["S"] + 2  # noqa: N806
    if k["dtype"].kind == "f":       # log-uniform backscatter-like values with a per-date level: scores are well separated
        level = np.exp(rng.uniform(-6.0, 2.0, size=(T, 1, 1, 1)))
        full = (level * np.exp(rng.normal(0.0, 0.5, size=(T, C, H, H)))).astype(np.float32)
    else:
        full = rng.integers(k["lo"], k["hi"] + 1, size=(T, C, H, H)).astype(k["dtype"])
    dates = np.stack([rng.integers(2015, 2024, T), rng.integers(1, 13, T), rng.integers(1, 29, T)], axis=1).astype(np.int16)
    mask = None
    if k["Cm"]:
        W = T // k["nd"]  # noqa: N806
        mask = np.zeros((T, k["Cm"], H, H), dtype=np.uint8)
        for t in range(T):
            j = (t - k["start"]) // W
            kind = rng.integers(0, 4)
            if j == 1 or kind == 0:                 # window 1: every date dirty (the mask is then ignored); others: one in four
                n = int(rng.integers(1, 4))
                mask[t, rng.integers(0, k["Cm"], n), rng.integers(1, H - 1, n), rng.integers(1, H - 1, n)] = rng.integers(60, 101, n)
            elif kind == 1:                         # below or at the threshold, and outside the crop: masks nothing
                mask[t, 0, 1, 1] = int(min(k["thr"], 100))
                mask[t, 0, 0, :] = 100
        if k["nd"] == 1:                            # a single window: exactly one clean date
            mask[:, 0, 2, 2] = 100
            mask[k["start"] + 5, :, 1:-1, 1:-1] = 0
    return full, mask, dates


def hash_name(name):
    return int.from_bytes(name.encode(), "little") % (2 ** 31)


def run_case(dataset_cls, name, k, tmp):
    full, mask, dates = make_inputs(name, k)
    T, nd, S = k["T"], k["nd"], k["S"]  # noqa: N806
    W = T // nd  # noqa: N806
    start = (1, 1, k["start"])
    end = (1 + S, 1 + S, k["start"] + nd * W)
    ds = dataset_cls(dataset=None, stage="train", use_transform=False, random_dates=k["seed"] is not None)
    if k["seed"] is not None:
        ds.rng = np.random.default_rng(k["seed"])
    if mask is None:
        path = Path(tmp) / f"{name}.npy"
        np.save(path, full)
        names = (None, None)
    else:
        import h5py
        h5py.File = MemoryH5
        MemoryH5.store = {"data": full, "mask": mask}
        path, names = Path(f"{name}.h5"), ("data", "mask")
    seen = {}
    real = np.nanargmin

    def recording_nanargmin(a, *args, **kw):
        r = real(a, *args, **kw)
        seen["scores"], seen["index"] = np.array(a), np.array(r)
        return r

    np.nanargmin = recording_nanargmin
    try:
        out, out_dates = ds.preprocess_raster(path, dates, None, names[0], names[1], start, end, bands=k["C"], num_dates=nd,
                                              mask_threshold=k["thr"], norm_fac=k["nf"], log_scale=k["log"])
    finally:
        np.nanargmin = real
    scores = seen["scores"].reshape(nd, W).astype(np.float64)
    index = seen["index"].reshape(nd).astype(np.int32)
    assert out.dtype == np.float32 and out.shape == (nd, k["C"], S, S)
    if k["dtype"].kind == "f":
        assert W >= 3
        for j in range(nd):
            s = np.sort(scores[j][~np.isnan(scores[j])])
            assert len(s) == 1 or (s[1] - s[0]) > F32_MARGIN * s[1], (name, j, s[:2])
    rec = {"raw": np.ascontiguousarray(full[:, :, 1:1 + S, 1:1 + S]), "dates": dates,
           "plan": np.array([k["start"], W, nd], dtype=np.int32),
           "params": np.array([k["thr"], float(k["log"]), 0.0 if k["nf"] is None else k["nf"],
                               -1.0 if k["seed"] is None else float(k["seed"])], dtype=np.float64),
           "ref_scores": scores, "index": index, "out": out, "out_dates": np.asarray(out_dates).astype(np.int16)}
    if mask is not None:
        rec["mask"] = np.ascontiguousarray(mask[:, :, 1:1 + S, 1:1 + S])
    return {f"{name}__{key}": v for key, v in rec.items()}


def main() -> None:
    dataset_cls = import_dataset_class()
    cases = case_table()
    arrays = {"names": np.array(sorted(cases))}
    with tempfile.TemporaryDirectory() as tmp:
        for name in sorted(cases):
            arrays.update(run_case(dataset_cls, name, cases[name], tmp))
    OUT.parent.mkdir(exist_ok=True)
    np.savez_compressed(OUT, **arrays)
    print(f"{OUT}: {len(cases)} cases, {OUT.stat().st_size} bytes")


if __name__ == "__main__":
    main()
