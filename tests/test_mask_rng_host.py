"""Device-side mask draws, the parts that need no GPU: the numpy Philox against the published Random123 vectors, the
restatement of the draw contract (``maestro_amd.layers.utils.mask_draw_reference``: sensitivity to every argument, batch-size
invariance, the counted rejection loop, its distribution against the host drawer, uniformity), the header, the argument
checks of ``mh_mask_draw``, the switch and the refusals."""

from __future__ import annotations

import ctypes
import math
import re
import statistics
from pathlib import Path

import numpy as np
import pytest
import torch

from maestro_amd.layers import utils as U
from tests import mask_rng_cases as C

ROOT = Path(__file__).resolve().parent.parent
SEED = (0xC0FFEE << 40) | 0x1234567        # high bits set


# ------------------------------------------------------------------------------------------------ Philox
@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, want):
    """Random123's kat_vectors for philox4x32-10."""
    got = U.philox4x32([np.uint32(c) for c in counter], key)
    assert " ".join(f"{int(w):08x}" for w in got) == want


def test_uniform_is_24_bits_of_the_selected_word():
    i = np.arange(8)
    u = U.mask_uniform(SEED, 7, 3, U.MASK_LOC, 11, 2, i)
    assert u.dtype == np.float32 and ((u >= 0) & (u < 1)).all()
    for k in range(8):
        w = U.philox4x32([np.uint32(k >> 2), np.uint32(11), np.uint32(7), np.uint32(U.MASK_LOC | 3 << 4 | 2 << 16)],
                         (SEED & 0xFFFFFFFF, SEED >> 32))
        assert u[k] == np.float32((int(w[k & 3]) >> 8) * 2.0 ** -24)
    assert np.array_equal(u * np.float32(2 ** 24), np.floor(u * np.float32(2 ** 24)))      # the value set of torch.rand
    with pytest.raises(ValueError):
        U.mask_uniform(SEED, 1 << 32, 0, 0, 0, 0, 0)
    with pytest.raises(ValueError):
        U.mask_uniform(SEED, -1, 0, 0, 0, 0, 0)


def test_every_argument_changes_the_draw():
    base = dict(seed=SEED, step=5, stream=1, kind=U.MASK_LOC, row=np.arange(4).reshape(4, 1), attempt=0, i=np.arange(64).reshape(1, 64))
    u0 = U.mask_uniform(**base)
    for key, other in (("seed", SEED ^ 1), ("seed", SEED ^ (1 << 63)), ("step", 6), ("stream", 2), ("kind", U.MASK_DATES),
                       ("attempt", 1), ("row", np.arange(4).reshape(4, 1) + 4)):
        u1 = U.mask_uniform(**{**base, key: other})
        assert (u0 != u1).mean() > 0.9, key
    # ... and so does the restatement: seed, step and row_base each change noise and structural masks
    groups, mods = C.hand_built(25)
    n0, s0 = U.mask_draw_reference(groups, mods, 3, SEED, 5, 5)
    for args in ((SEED + 1, 5, 5), (SEED, 6, 5), (SEED, 5, 6)):
        n1, s1 = U.mask_draw_reference(groups, mods, 3, *args)
        assert all(not torch.equal(n0[k], n1[k]) for k in n0) and any(not torch.equal(s0[k], s1[k]) for k in s0), args
    # two modalities, two groups: different streams
    assert not torch.equal(n0["ga"][:, :50], n0["gc"])


@pytest.mark.parametrize("spec", ["plain", "two_mods", "folded"])
def test_a_row_does_not_depend_on_the_batch_size(spec):
    groups, mods = C.hand_built_folded(9) if spec == "folded" else C.hand_built(9, two_mods=spec == "two_mods")
    whole = U.mask_draw_reference(groups, mods, 4, SEED, 3, 0)
    halves = [U.mask_draw_reference(groups, mods, 2, SEED, 3, rb) for rb in (0, 2)]
    for d in (0, 1):
        for k in whole[d]:
            assert torch.equal(whole[d][k], torch.cat([h[d][k] for h in halves])), (spec, d, k)
    shifted = U.mask_draw_reference(groups, mods, 2, SEED, 3, 1)
    for d in (0, 1):
        for k in whole[d]:
            rows = whole[d][k].shape[0] // 4
            assert torch.equal(shifted[d][k], whole[d][k][rows: 3 * rows])


def test_the_attempt_bound_ends_the_loop_all_clear():
    groups, mods = C.hand_built(9, kinds="m", p_mod=1.0)
    noise, struct = U.mask_draw_reference(groups, mods, 3, SEED, 0, 0)
    assert struct["ga"].shape == (3, 36) and not struct["ga"].any()      # every attempt is all-masked: all-clear after 64
    assert not struct["gc"].any()                                          # (no active kind)
    with pytest.raises(ValueError, match="p_mod >= 1"):
        U.check_device_mask_config(groups)
    U.check_device_mask_config(C.hand_built(9)[0])
    # p_mod = 0.9: most rows need several attempts; every row against a scalar walk of the loop
    groups, mods = C.hand_built(4, kinds="ml", p_mod=0.9)
    _, struct = U.mask_draw_reference(groups, mods, 64, SEED, 1, 0)
    assert not struct["ga"].all(dim=1).any()
    later = 0
    for r in range(64):
        want = np.zeros(16, dtype=bool)
        for a in range(U.MASK_MAX_ATTEMPTS):
            mod = U.mask_uniform(SEED, 1, 0, U.MASK_MOD, r, a, 0) < np.float32(0.9)
            loc = U.mask_uniform(SEED, 1, 0, U.MASK_LOC, r, a, np.arange(4)) < np.float32(0.6)
            row = np.tile(loc | mod, 4)                  # (band-group, date, l)
            if not row.all():
                want, later = row, later + (a > 0)
                break
        assert np.array_equal(struct["ga"][r].numpy(), want), r
    assert later > 32


# ------------------------------------------------------------------------------------------------ distribution
N_ROWS, HOST_SEEDS, DEVICE_SEED = 4096, (1, 2), 3


def _rates(struct):
    return {k: v.double().mean(dim=0).numpy() for k, v in struct.items()}


def _agree(r1, r2, n1, n2):
    """Per token: |difference of the rates| <= 5 standard errors of the difference (pooled rate)."""
    for k in r1:
        p = (r1[k] * n1[k] + r2[k] * n2[k]) / (n1[k] + n2[k])
        se = np.sqrt(p * (1 - p) * (1 / n1[k] + 1 / n2[k]))
        bad = np.abs(r1[k] - r2[k]) > 5 * se
        assert not bad.any(), (k, np.abs(r1[k] - r2[k])[bad], se[bad])


@pytest.mark.parametrize("name", ["group", "bg_ts_monotemp", "bg_aerial_s2"])
def test_structural_rates_match_the_host_drawer(name):
    """N = 4096 samples per drawer; host generator seeds 1 and 2, device seed 3.  The two host runs pass the same criterion."""
    model, _, _ = C.build_model(name)
    groups, mods = C.set_beff(model, N_ROWS)
    host = []
    for s in HOST_SEEDS:
        host.append(U.draw_struct_masks(groups, mods, torch.Generator().manual_seed(s)))
    _, dev = U.mask_draw_reference(groups, mods, N_ROWS, DEVICE_SEED, 0, 0)
    n = {g.name: g.Beff for g in groups}
    assert {k: tuple(v.shape) for k, v in dev.items()} == {k: tuple(v.shape) for k, v in host[0].items()}
    _agree(_rates(host[0]), _rates(host[1]), n, n)
    _agree(_rates(dev), _rates(host[0]), n, n)
    _agree(_rates(dev), _rates(host[1]), n, n)
    if name != "bg_ts_monotemp":          # (the folded modes have no structural masks: 0 == 0 there)
        assert any(v.any() for v in dev.values())


def _chi2_quantile(df: int, q: float) -> float:
    try:
        from scipy.stats import chi2
        return float(chi2.ppf(q, df))
    except ImportError:                   # Wilson-Hilferty
        z = statistics.NormalDist().inv_cdf(q)
        return df * (1 - 2 / (9 * df) + z * math.sqrt(2 / (9 * df))) ** 3


def test_noise_is_uniform():
    groups, mods = C.hand_built(64)                      # ga: L = 256 tokens
    noise, _ = U.mask_draw_reference(groups, mods, 256, SEED, 9, 0)
    x = noise["ga"].numpy().ravel()
    assert x.size == 1 << 16
    counts = np.bincount((x * 16).astype(int), minlength=16)
    chi = float(((counts - x.size / 16) ** 2 / (x.size / 16)).sum())
    bound = _chi2_quantile(15, 1 - 1e-6)
    assert 45 < bound < 58 and chi <= bound, (chi, bound)


# ------------------------------------------------------------------------------------------------ header + ABI
@pytest.fixture(scope="module")
def lib():
    from maestro_amd.csrc.build import LIB, build
    if not LIB.exists():
        build()
    handle = ctypes.CDLL(str(LIB))
    handle.mh_last_error.restype = ctypes.c_char_p
    return handle


HEADER = ROOT / "include" / "maestro_hip.h"


def _declared():
    return sorted(n for n in set(re.findall(r"\b(mh_[a-z0-9_]+)\s*\(", HEADER.read_text())) if n.startswith("mh_mask_draw"))


def test_every_declared_symbol_is_exported(lib):
    assert _declared() == ["mh_mask_draw"]
    assert not [n for n in _declared() if not hasattr(lib, n)]


def test_rng_names_are_declared_in_the_one_header():
    import inspect

    from maestro_amd.csrc import build as B
    text = HEADER.read_text()
    assert sorted(p.name for p in (ROOT / "include").iterdir()) == ["maestro_hip.h"]
    assert re.search(r"^int mh_mask_draw\(", text, re.M) and "maestro/ssl/mae.py:178-246" in text
    for layout in ("c0 = i >> 2,   c1 = global row,   c2 = step,   c3 = kind | stream << 4 | attempt << 16", "0xD2511F53 / 0xCD9E8D57",
                   "0x9E3779B9 /", "(float)(word[i & 3] >> 8) * 2^-24"):
        assert layout in text, layout
    assert '"maestro_hip.h"' in inspect.getsource(B._digest) and inspect.getsource(B._digest).count("maestro_hip") == 1
    assert '#include "../../include/maestro_hip.h"' in (B.CSRC / "mask_rng.hip").read_text()


def test_structs_match_the_header():
    from maestro_amd import hip
    text = HEADER.read_text()
    for cls, name in ((hip._MhMaskSeg, "MhMaskSeg"), (hip._MhMaskJob, "MhMaskJob")):
        body = re.search(r"typedef struct \{([^}]*)\} " + name + ";", text).group(1)
        fields = [f.strip().lstrip("*") for decl in body.split(";") if decl.strip()
                  for f in re.sub(r"^\s*(unsigned char|float|int)\s*\*?", "", decl.strip()).split(",")]
        assert fields == [f[0] for f in cls._fields_], name
    assert ctypes.sizeof(hip._MhMaskSeg) == 40 and ctypes.sizeof(hip._MhMaskJob) == 56
    assert f"#define MH_MASK_MAX_ATTEMPTS {U.MASK_MAX_ATTEMPTS}" in text and f"#define MH_MASK_MAX_L {hip.MASK_MAX_L}" in text


def _abi_call(lib, jobs=None, segs=None, n_jobs=1, step=0, row_base=0, null=None, **over):
    """Device pointers are never dereferenced on the host and a refused call launches nothing: any non-null value will do."""
    from maestro_amd import hip
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.mh_mask_draw.argtypes = [vp, vp, ci, vp, vp, ci, ctypes.c_uint64, ctypes.c_longlong, ctypes.c_longlong, vp]
    lib.mh_mask_draw.restype = ci
    seg = dict(tok_off=0, D=2, L=9, gi=0, G=1, stream=0, p_mod=-1.0, p_bands=-1.0, p_dates=0.5, p_loc=0.5)
    job = dict(noise=0x1000, strct=0x2000, Beff=3, L=18, noise_stream=0, noise_rpb=1, struct_rpb=1, row_div=1, row_mul=1, row_add=0,
               seg0=0, n_segs=1)
    for k, v in over.items():
        if k.startswith("seg_"):
            seg[k[4:]] = v
        else:
            job[k] = v
    jarr, sarr = (hip._MhMaskJob * 1)(hip._MhMaskJob(**job)), (hip._MhMaskSeg * 1)(hip._MhMaskSeg(**seg))
    p = [ctypes.cast(jarr, vp), vp(0x3000), ctypes.cast(sarr, vp), vp(0x4000)]
    if null is not None:
        p[null] = vp(0)
    return lib.mh_mask_draw(p[0], p[1], n_jobs, p[2], p[3], 1, SEED, step, row_base, vp(0))


def test_bad_arguments_are_refused_before_the_gpu_is_touched(lib):
    for null in range(4):
        assert _abi_call(lib, null=null) == -1 and b"null" in lib.mh_last_error()
    assert _abi_call(lib, noise=0) == -1 and b"null" in lib.mh_last_error()
    assert _abi_call(lib, strct=0) == -1 and b"null" in lib.mh_last_error()
    assert _abi_call(lib, n_jobs=0) == -1 and b"n_jobs" in lib.mh_last_error()
    assert _abi_call(lib, n_jobs=-3) == -1
    assert _abi_call(lib, L=8193, seg_L=8193, seg_D=1) == -1 and b"L 8193" in lib.mh_last_error()
    assert _abi_call(lib, L=0) == -1
    assert _abi_call(lib, step=1 << 32) == -1 and b"step" in lib.mh_last_error()
    assert _abi_call(lib, step=-1) == -1 and b"step" in lib.mh_last_error()
    assert _abi_call(lib, row_base=-1) == -1 and b"row_base" in lib.mh_last_error()
    assert _abi_call(lib, row_base=0xFFFFFFFF) == -1 and b"32 bits" in lib.mh_last_error()
    assert _abi_call(lib, L=19) == -1 and b"cover" in lib.mh_last_error()          # the segments do not tile the row
    assert _abi_call(lib, L=17) == -1 and b"cover" in lib.mh_last_error()
    assert _abi_call(lib, seg_tok_off=1) == -1 and b"tok_off" in lib.mh_last_error()
    assert _abi_call(lib, seg_stream=4096) == -1 and b"stream" in lib.mh_last_error()
    assert _abi_call(lib, noise_stream=-1) == -1
    assert _abi_call(lib, seg_gi=1) == -1 and b"band-group" in lib.mh_last_error()
    assert _abi_call(lib, row_div=0) == -1 and b"draw-row map" in lib.mh_last_error()
    assert _abi_call(lib, row_div=2, row_mul=4, row_add=3) == -1
    assert _abi_call(lib, Beff=0) == -1
    assert _abi_call(lib, seg_p_loc=float("nan")) == -1 and b"NaN" in lib.mh_last_error()
    assert _abi_call(lib, n_segs=2) == -1 and b"segments" in lib.mh_last_error()


def test_wrapper_wants_dense_device_buffers():
    from maestro_amd import hip
    groups, mods = C.hand_built(9)
    jobs = U.mask_draw_jobs(groups, mods, 2)
    assert [j["name"] for j in jobs] == ["ga", "gc"] and [j["noise_stream"] for j in jobs] == [0, 1]
    assert [s["stream"] for s in jobs[0]["segs"]] == [0, 0] and jobs[1]["segs"][0]["stream"] == 1
    assert jobs[0]["segs"][1]["p"] == (pytest.approx(0.9), pytest.approx(0.4), 0.5, pytest.approx(0.6)) and jobs[1]["segs"][0]["p"][:2] == (-1.0, -1.0)
    bufs = {j["name"]: (torch.zeros(j["Beff"], j["L"]), torch.zeros(j["Beff"], j["L"], dtype=torch.uint8)) for j in jobs}
    with pytest.raises(hip.HipExtensionError, match="device tensors"):
        hip.MaskDraw(jobs, bufs, "cpu")
    with pytest.raises(hip.HipExtensionError, match="no jobs"):
        hip.MaskDraw([], {}, "cpu")
    fold = U.mask_draw_jobs(*C.hand_built_folded(9), 2)
    assert [(j["Beff"], j["noise_rpb"], j["struct_rpb"], j["row_div"], j["row_mul"], j["row_add"]) for j in fold] == \
        [(4, 4, 2, 2, 4, 0), (4, 4, 2, 2, 4, 2)] and [j["noise_stream"] for j in fold] == [0, 0]


# ------------------------------------------------------------------------------------------------ the switch, the refusals
def test_resolve_mask_rng(monkeypatch):
    from maestro_amd.engine import resolve_mask_rng
    monkeypatch.delenv("MAESTRO_MASK_RNG", raising=False)
    assert resolve_mask_rng() == "host" and resolve_mask_rng(None) == "host"
    assert resolve_mask_rng("device") == "device" and resolve_mask_rng("host") == "host"
    monkeypatch.setenv("MAESTRO_MASK_RNG", "device")
    assert resolve_mask_rng() == "device" and resolve_mask_rng("host") == "host"
    monkeypatch.setenv("MAESTRO_MASK_RNG", "gpu")
    with pytest.raises(ValueError, match="mask_rng"):
        resolve_mask_rng()
    with pytest.raises(ValueError, match="mask_rng"):
        resolve_mask_rng("philox")


def test_refusals(monkeypatch):
    """All of them are ValueErrors raised before the device is looked at (a CPU device here: what follows them is the
    "needs a GPU" error of an accepted configuration)."""
    from maestro_amd import hip
    from maestro_amd.engine import MAEEngine
    monkeypatch.delenv("MAESTRO_MASK_RNG", raising=False)
    monkeypatch.delenv("MAESTRO_TIE_ORDER", raising=False)
    model, _, B = C.build_model("group")  # noqa: N806
    with pytest.raises(ValueError, match="mask_rng"):
        MAEEngine(model, B, "cpu", mask_rng="cuda")
    with pytest.raises(ValueError, match="mask_rng"):
        model.engine(B, "cpu", mask_rng="cuda")
    with pytest.raises(ValueError, match="mask_seed"):
        MAEEngine(model, B, "cpu", mask_rng="device", mask_seed=-1)
    with pytest.raises(hip.HipExtensionError, match="needs a GPU"):
        MAEEngine(model, B, "cpu", mask_rng="device", mask_seed=SEED)
    monkeypatch.setenv("MAESTRO_TIE_ORDER", "torch")
    with pytest.raises(ValueError, match="tie_order"):
        MAEEngine(model, B, "cpu", mask_rng="device")
    with pytest.raises(hip.HipExtensionError, match="needs a GPU"):
        MAEEngine(model, B, "cpu", mask_rng="host")
    monkeypatch.delenv("MAESTRO_TIE_ORDER")
    grp = next(g for g in model.group_specs.values() if len(g.mods) > 1)
    for m in grp.mods:
        m.p_mod = 1.0
    with pytest.raises(ValueError, match="p_mod >= 1"):
        MAEEngine(model, B, "cpu", mask_rng="device")
    with pytest.raises(hip.HipExtensionError, match="needs a GPU"):
        MAEEngine(model, B, "cpu", mask_rng="host")
