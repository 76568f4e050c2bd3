"""AdamW with bf16 moments, the parts that need no GPU: the header against the library and its bad-argument refusals, the
stochastic rounding restated on integers (``hip.sr_bf16_round``), the counter layout of its random words
(``hip.sr_bf16_words``), the unbiasedness of the reference, and the surface (``MAESTRO_MOMENT_DTYPE``, the refusals of the
loops and of the optimizer)."""

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
NAMES = ["mh_adamw_bf16m", "mh_adamw_bf16m_dev", "mh_adamw_groups_bf16m", "mh_adamw_groups_bf16m_dev"]


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
    for layout in ("c0 = (elem_base + i) / 4 (low 32 bits),   c1 = step (low 32 bits),   c2 = 0,   c3 = MH_ADAMW_SR_TAG",
                   "m:  (w[e >> 1] >> 16 * (e & 1)) & 0xffff        v:  (w[2 + (e >> 1)] >> 16 * (e & 1)) & 0xffff",
                   "else t = u + r:  t carried into an all-ones exponent -> store u >> 16 (stays finite), else store t >> 16"):
        assert layout in text, layout
    assert f"#define MH_ADAMW_SR_TAG 0x{hip.ADAMW_SR_TAG:08X}u" in text
    assert '"maestro_hip.h"' in inspect.getsource(B._digest) and inspect.getsource(B._digest).count("maestro_hip") == 1
    optim = (B.CSRC / "optim.hip").read_text()
    assert '#include "../../include/maestro_hip.h"' in optim and not [n for n in NAMES if f'extern "C" int {n}(' not in optim]


def test_bad_arguments_are_refused_before_the_gpu_is_touched(lib):
    """Device pointers are never dereferenced on the host and a refused call launches nothing: any non-null value will do."""
    vp, cl, cf, ci, u64 = ctypes.c_void_p, ctypes.c_long, ctypes.c_float, ctypes.c_int, ctypes.c_uint64
    lib.mh_adamw_bf16m.argtypes = [vp] * 5 + [cl, cl, u64, cf, cf, cf, cf, cf, ci, cf, vp]
    lib.mh_adamw_bf16m_dev.argtypes = [vp] * 5 + [cl, cl, u64, cf, cf, cf, cf, vp, vp, vp]
    lib.mh_adamw_groups_bf16m.argtypes = [vp] * 8 + [cl, cl, u64, cf, cf, cf, cf, ci, cf, vp]
    lib.mh_adamw_groups_bf16m_dev.argtypes = [vp] * 8 + [cl, cl, u64, cf, cf, cf, vp, vp, vp]

    def plain(p=0x1000, g=0x2000, m=0x3008, v=0x4008, pb=0x5008, n=64, base=4, step=1):
        return lib.mh_adamw_bf16m(p, g, m, v, pb, n, base, 7, 1e-3, 0.9, 0.99, 1e-8, 0.01, step, 1.0, None)

    def plain_dev(p=0x1000, g=0x2000, m=0x3008, v=0x4008, pb=0x5008, n=64, base=4, h=0x9000, sd=0xa000):
        return lib.mh_adamw_bf16m_dev(p, g, m, v, pb, n, base, 7, 0.9, 0.99, 1e-8, 0.01, h, sd, None)

    def grouped(p=0x1000, g=0x2000, m=0x3008, v=0x4008, pb=0x5008, gm=0x6001, ls=0x7000, wd=0x8000, n=64, base=64, step=1):
        return lib.mh_adamw_groups_bf16m(p, g, m, v, pb, gm, ls, wd, n, base, 7, 1e-3, 0.9, 0.99, 1e-8, step, 1.0, None)

    def grouped_dev(p=0x1000, g=0x2000, m=0x3008, v=0x4008, pb=0x5008, gm=0x6001, ls=0x7000, wd=0x8000, n=64, base=64, h=0x9000,
                    sd=0xa000):
        return lib.mh_adamw_groups_bf16m_dev(p, g, m, v, pb, gm, ls, wd, n, base, 7, 0.9, 0.99, 1e-8, h, sd, None)

    for call in (plain, plain_dev, grouped, grouped_dev):
        for null in ("p", "g", "m", "v"):
            assert call(**{null: 0}) == -1 and b"null pointer" in lib.mh_last_error(), (call.__name__, null)
        for n in (0, -4, 6, 63):
            assert call(n=n) == -1 and b"n % 4" in lib.mh_last_error(), (call.__name__, n)
        for base in (2, 5, -4, -64):
            assert call(base=base) == -1 and b"elem_base" in lib.mh_last_error(), (call.__name__, base)
        for mis in (dict(p=0x1008), dict(g=0x2004), dict(m=0x3004), dict(v=0x400c), dict(pb=0x5004), dict(m=0x3002)):
            assert call(**mis) == -1 and b"aligned" in lib.mh_last_error(), (call.__name__, mis)
    for call in (grouped, grouped_dev):
        for base in (4, 32, 96):                             # a multiple of 4 is not enough: the map has one byte per 64 elements
            assert call(base=base) == -1 and b"elem_base" in lib.mh_last_error(), (call.__name__, base)
        for null in ("gm", "ls", "wd"):
            assert call(**{null: 0}) == -1 and b"null" in lib.mh_last_error(), (call.__name__, null)
    for call in (plain, grouped):
        for step in (0, -1):
            assert call(step=step) == -1 and b"step >= 1" in lib.mh_last_error(), (call.__name__, step)
    for call in (plain_dev, grouped_dev):
        for null in ("h", "sd"):
            assert call(**{null: 0}) == -1 and b"null pointer" in lib.mh_last_error(), (call.__name__, null)


def test_wrappers_check_the_moment_buffers_before_any_launch():
    from maestro_amd import hip
    z, h = torch.zeros(128), torch.zeros(128, dtype=torch.bfloat16)
    with pytest.raises(hip.HipExtensionError, match="bfloat16"):          # fp32 moments handed to the bf16 entry
        hip.adamw_bf16m(z, z, z, z, None, 128, 0, 0, 1e-3, 0.9, 0.99, 1e-8, 0.01, 1)
    with pytest.raises(hip.HipExtensionError, match="at least n"):
        hip.adamw_bf16m(z, z, h[:64], h, None, 128, 0, 0, 1e-3, 0.9, 0.99, 1e-8, 0.01, 1)
    with pytest.raises(hip.HipExtensionError, match="int64"):
        hip.adamw_bf16m_dev(z, z, h, h, None, 128, 0, 0, 0.9, 0.99, 1e-8, 0.01, torch.zeros(5), torch.zeros(1))
    with pytest.raises(hip.HipExtensionError, match="GPU"):               # CPU tensors: no fallback
        hip.adamw_bf16m(z, z, h, h, None, 128, 0, 0, 1e-3, 0.9, 0.99, 1e-8, 0.01, 1)


# ------------------------------------------------------------------------------------------------ the rounding rule, on integers
ALL_R = np.arange(65536, dtype=np.uint32)
PATTERNS = [0x3F800001, 0x3F80FFFF, 0x3F808000, 0x00000001, 0x0000FFFF, 0x007FFFFF, 0x3EAAAAAB, 0x7F7E1234, 0x00812345]


def test_a_representable_value_is_unchanged():
    from maestro_amd import hip
    for hi in (0x0000, 0x8000, 0x3F80, 0xBF80, 0x0001, 0x8001, 0x7F7F, 0xFF7F, 0x0080, 0x7F80, 0xFF80, 0x7FC0):
        out = hip.sr_bf16_round(np.full(65536, hi << 16, dtype=np.uint32), ALL_R)
        assert (out == hi).all(), hex(hi)
    assert hip.sr_bf16_round(np.uint32(0x3F800000), np.uint32(0xFFFF)).dtype == np.uint16


@pytest.mark.parametrize("u", PATTERNS)
def test_every_word_gives_a_neighbour_and_rounds_up_low16_times(u):
    from maestro_amd import hip
    down, low = u >> 16, u & 0xFFFF
    out = hip.sr_bf16_round(np.full(65536, u, dtype=np.uint32), ALL_R).astype(np.int64)
    assert set(np.unique(out).tolist()) <= {down, down + 1}
    assert int((out == down + 1).sum()) == low and int((out == down).sum()) == 65536 - low
    assert (np.diff(out) >= 0).all()                         # monotone in r: the carry appears once
    neg = hip.sr_bf16_round(np.full(65536, u | 0x80000000, dtype=np.uint32), ALL_R).astype(np.int64)
    assert (neg == (out | 0x8000)).all()                     # negative values mirror positive ones


def test_inf_and_nan_pass_through_and_a_nan_stays_a_nan():
    from maestro_amd import hip
    for u, want in ((0x7F800000, 0x7F80), (0xFF800000, 0xFF80), (0x7FC00000, 0x7FC0), (0xFFC12345, 0xFFC1),
                    (0x7F800001, 0x7FC0), (0xFF80FFFF, 0xFFC0), (0x7F810000, 0x7F81), (0x7FFFFFFF, 0x7FFF)):
        out = hip.sr_bf16_round(np.full(65536, u, dtype=np.uint32), ALL_R)
        assert (out == want).all(), (hex(u), hex(int(out[0])))
        if u & 0x007FFFFF:
            assert want & 0x7F80 == 0x7F80 and want & 0x007F, hex(u)      # still a NaN in bf16


def test_a_finite_value_next_to_the_largest_bf16_never_becomes_inf():
    from maestro_amd import hip
    for u in (0x7F7F0001, 0x7F7F8000, 0x7F7FFFFF, 0xFF7FFFFF, 0xFF7F0001):
        out = hip.sr_bf16_round(np.full(65536, u, dtype=np.uint32), ALL_R)
        assert (out == u >> 16).all(), hex(u)
    below = hip.sr_bf16_round(np.full(65536, 0x7F7EFFFF, dtype=np.uint32), ALL_R)      # one bf16 further down still rounds up
    assert set(np.unique(below).tolist()) == {0x7F7E, 0x7F7F}
    with pytest.raises(ValueError, match="16-bit"):
        hip.sr_bf16_round(np.uint32(1), np.uint32(0x10000))


# ------------------------------------------------------------------------------------------------ the counter layout
def test_a_split_range_draws_the_words_of_the_whole():
    from maestro_amd import hip
    n, seed, step = 2048 + 12, 0x1234567887654321, 7
    rng = np.random.default_rng(0)
    bits = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    for which in ("m", "v"):
        whole = hip.sr_bf16_reference(bits, np.arange(n), seed, step, which)
        for a in (4, 1024, 1028, n - 4):
            parts = [hip.sr_bf16_reference(bits[:a], np.arange(a), seed, step, which),
                     hip.sr_bf16_reference(bits[a:], a + np.arange(n - a), seed, step, which)]      # elem_base = a
            assert (np.concatenate(parts) == whole).all(), (which, a)
    # four elements, one Philox call: the layout of the eight words
    from maestro_amd.layers.utils import philox4x32
    w = philox4x32((np.uint64(5), np.uint64(step), np.uint64(0), np.uint64(hip.ADAMW_SR_TAG)), (seed & 0xFFFFFFFF, seed >> 32))
    w = [int(x) for x in w]
    assert hip.sr_bf16_words(np.arange(20, 24), seed, step, "m").tolist() == [w[0] & 0xFFFF, w[0] >> 16, w[1] & 0xFFFF, w[1] >> 16]
    assert hip.sr_bf16_words(np.arange(20, 24), seed, step, "v").tolist() == [w[2] & 0xFFFF, w[2] >> 16, w[3] & 0xFFFF, w[3] >> 16]
    with pytest.raises(ValueError, match="which"):
        hip.sr_bf16_words(np.arange(4), 0, 1, "p")


def test_words_differ_between_steps_seeds_and_moments():
    from maestro_amd import hip
    idx = np.arange(4096)
    base = hip.sr_bf16_words(idx, 0, 1, "m")
    assert base.dtype == np.uint32 and int(base.max()) <= 0xFFFF and len(np.unique(base)) > 3000
    for other in (hip.sr_bf16_words(idx, 0, 2, "m"), hip.sr_bf16_words(idx, 1, 1, "m"), hip.sr_bf16_words(idx, 1 << 32, 1, "m"),
                  hip.sr_bf16_words(idx, 0, 1, "v"), hip.sr_bf16_words(idx + 4096, 0, 1, "m")):
        assert float((other == base).mean()) < 0.01          # chance agreement of 16-bit words: 2^-16
    assert (hip.sr_bf16_words(idx, 0, 1 + (1 << 32), "m") == base).all()      # the low 32 bits of the step, as on the device


def test_no_counter_collides_with_a_mask_draw_counter():
    """Counters are (c0, c1, c2, c3) under the key of the seed.  The mask draws put ``kind | stream << 4 | attempt << 16`` into c3
    (``layers.utils.mask_uniform``, include/maestro_hip.h): kind <= 4 in four bits, stream < 4096, attempt < 64, so c3 < 2^22.
    The rounding draws put the tag there."""
    from maestro_amd import hip
    from maestro_amd.layers import utils
    rng_h = HEADER.read_text()
    streams = int(re.search(r"#define MH_MASK_MAX_STREAMS (\d+)", rng_h).group(1))
    attempts = int(re.search(r"#define MH_MASK_MAX_ATTEMPTS (\d+)", rng_h).group(1))
    kinds = [utils.MASK_NOISE, utils.MASK_MOD, utils.MASK_BANDS, utils.MASK_DATES, utils.MASK_LOC]
    assert attempts == utils.MASK_MAX_ATTEMPTS and max(kinds) < 16 and streams <= 1 << 12
    largest = max(kinds) | (streams - 1) << 4 | (attempts - 1) << 16
    assert largest < 1 << 22 <= hip.ADAMW_SR_TAG < 1 << 32
    assert (hip.ADAMW_SR_TAG & 0xF) not in kinds             # not even a draw kind in the low four bits
    # the same key, the same (c0, c1, c2) and only c3 apart: other words
    from maestro_amd.layers.utils import philox4x32
    a = philox4x32((np.arange(64), np.uint64(3), np.uint64(0), np.uint64(hip.ADAMW_SR_TAG)), (9, 0))
    b = philox4x32((np.arange(64), np.uint64(3), np.uint64(0), np.uint64(largest)), (9, 0))
    assert not any((x == y).any() for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ unbiasedness of the reference
def test_the_rounded_mean_is_the_value():
    """One fp32 value with a non-trivial low half at 65536 consecutive indices, default seed: every rounding is a Bernoulli draw
    with p = low16 / 65536 between two neighbours one bf16 ulp apart, so the mean of N draws has standard deviation
    ulp * sqrt(p (1 - p) / N).  Six of them (checked on the CPU for these constants: the mean lies +0.84 sigma from the value for
    ``m`` and -0.53 sigma for ``v``).  A property of the reference alone."""
    from maestro_amd import hip
    value, n = np.float32(0.0123456789), 65536
    u = int(value.view(np.uint32))
    low = u & 0xFFFF
    assert 0x1000 < low < 0xF000
    p = low / 65536.0
    down = np.array([u & 0xFFFF0000], dtype=np.uint32).view(np.float32)[0].astype(np.float64)
    up = np.array([(u & 0xFFFF0000) + 0x10000], dtype=np.uint32).view(np.float32)[0].astype(np.float64)
    sigma = (up - down) * np.sqrt(p * (1 - p) / n)
    for which in ("m", "v"):
        out = hip.sr_bf16_reference(np.full(n, u, dtype=np.uint32), np.arange(n), 0, 1, which)
        vals = (out.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
        assert set(np.unique(vals).tolist()) == {float(down), float(up)}
        print(f"{which}: (mean - value) / sigma = {(vals.mean() - float(value)) / sigma:+.3f}")
        assert abs(vals.mean() - float(value)) <= 6 * sigma, (which, (vals.mean() - float(value)) / sigma)


# ------------------------------------------------------------------------------------------------ the surface
def test_switch_resolution(monkeypatch):
    from maestro_amd.train.optim import resolve_moment_dtype
    monkeypatch.delenv("MAESTRO_MOMENT_DTYPE", raising=False)
    assert resolve_moment_dtype() == "fp32" and resolve_moment_dtype("bf16") == "bf16" and resolve_moment_dtype("fp32") == "fp32"
    monkeypatch.setenv("MAESTRO_MOMENT_DTYPE", "")
    assert resolve_moment_dtype() == "fp32"
    monkeypatch.setenv("MAESTRO_MOMENT_DTYPE", "fp32")
    assert resolve_moment_dtype() == "fp32"
    monkeypatch.setenv("MAESTRO_MOMENT_DTYPE", "bf16")
    assert resolve_moment_dtype() == "bf16" and resolve_moment_dtype("fp32") == "fp32"      # an explicit kwarg wins
    for bad in ("fp16", "BF16", "1", "bfloat16"):
        monkeypatch.setenv("MAESTRO_MOMENT_DTYPE", bad)
        with pytest.raises(ValueError, match="moment_dtype"):
            resolve_moment_dtype()
        assert resolve_moment_dtype("bf16") == "bf16"
    with pytest.raises(ValueError, match="moment_dtype"):
        resolve_moment_dtype("half")


def test_loop_refusals_that_need_no_gpu(monkeypatch):
    """All ValueErrors raised before anything is built (the model is None: what follows an accepted configuration is the
    AttributeError of building an engine from it)."""
    from maestro_amd.train.trainer import PretrainLoop, SupervisedLoop
    for v in ("MAESTRO_MOMENT_DTYPE", "MAESTRO_DTYPE", "MAESTRO_EXCHANGE", "MAESTRO_MAX_GRAD_NORM", "MAESTRO_SKIP_NONFINITE",
              "MAESTRO_LW_DECAY", "MAESTRO_DETERMINISTIC"):
        monkeypatch.delenv(v, raising=False)
    with pytest.raises(ValueError, match="moment_dtype='bf16'.*fp8"):
        PretrainLoop(None, 1, "cpu", moment_dtype="bf16", dtype="fp8")
    with pytest.raises(ValueError, match="moment_dtype='bf16'.*rs_ag"):
        PretrainLoop(None, 1, "cpu", moment_dtype="bf16", exchange_mode="rs_ag")
    with pytest.raises(ValueError, match="moment_dtype='bf16'.*overlap_optimizer"):
        PretrainLoop(None, 1, "cpu", moment_dtype="bf16", overlap_optimizer=True)
    for loop in (PretrainLoop, SupervisedLoop):
        with pytest.raises(ValueError, match="moment_dtype"):
            loop(None, 1, "cpu", moment_dtype="fp16")
    # allowed: what follows is the AttributeError of building an engine from None
    for ok in (dict(moment_dtype="bf16"), dict(moment_dtype="bf16", deterministic=True), dict(moment_dtype="fp32", overlap_optimizer=True),
               dict(moment_dtype="bf16", max_grad_norm=1.0, skip_nonfinite=True), dict(moment_dtype="bf16", moment_seed=5), dict()):
        with pytest.raises(AttributeError):
            PretrainLoop(None, 1, "cpu", **ok)
    for ok in (dict(moment_dtype="bf16"), dict(moment_dtype="bf16", lw_decay=0.75, max_grad_norm=1.0), dict()):
        with pytest.raises(AttributeError):
            SupervisedLoop(None, 1, "cpu", **ok)
    # the environment reaches both loops, and an explicit kwarg wins over it
    monkeypatch.setenv("MAESTRO_MOMENT_DTYPE", "bf16")
    with pytest.raises(ValueError, match="moment_dtype='bf16'.*rs_ag"):
        PretrainLoop(None, 1, "cpu", exchange_mode="rs_ag")
    monkeypatch.setenv("MAESTRO_EXCHANGE", "rs_ag")
    with pytest.raises(ValueError, match="moment_dtype='bf16'.*rs_ag"):
        PretrainLoop(None, 1, "cpu")
    with pytest.raises(AttributeError):
        PretrainLoop(None, 1, "cpu", moment_dtype="fp32")
    monkeypatch.delenv("MAESTRO_EXCHANGE")
    monkeypatch.setenv("MAESTRO_DTYPE", "fp8")
    with pytest.raises(ValueError, match="moment_dtype='bf16'.*fp8"):
        PretrainLoop(None, 1, "cpu")
    monkeypatch.setenv("MAESTRO_MOMENT_DTYPE", "int8")
    for loop in (PretrainLoop, SupervisedLoop):
        with pytest.raises(ValueError, match="moment_dtype"):
            loop(None, 1, "cpu")


def _stub_engine(**kw):
    flat = torch.zeros(128)
    return SimpleNamespace(store=SimpleNamespace(flat=flat, grad=flat.clone(), half=flat.bfloat16(), total=128), **kw)


def test_fused_adamw_holds_bf16_moments_and_refuses_what_has_no_bf16_form():
    from maestro_amd.train.optim import FusedAdamW
    plain = FusedAdamW(_stub_engine(), 1e-3)
    assert plain.moment_dtype == "fp32" and plain.m.dtype == torch.float32 and not plain.bf16_moments
    assert "moment_dtype" not in plain.state_dict()            # an fp32-moment state keeps the keys it always had
    opt = FusedAdamW(_stub_engine(), 1e-3, moment_dtype="bf16", moment_seed=-1)
    assert opt.m.dtype == opt.v.dtype == torch.bfloat16 and opt.m.numel() == 128 and opt.moment_seed == 0xFFFFFFFFFFFFFFFF
    assert opt.m.numel() * opt.m.element_size() * 2 == plain.m.numel() * plain.m.element_size()
    with pytest.raises(ValueError, match="moment_dtype"):
        FusedAdamW(_stub_engine(), 1e-3, moment_dtype="fp16")
    with pytest.raises(ValueError, match="fp8"):
        FusedAdamW(_stub_engine(fp8=object()), 1e-3, moment_dtype="bf16").step()
    with pytest.raises(ValueError, match="rs_ag"):
        opt.step_sharded(SimpleNamespace())                       # before the exchange plan is even looked at
    assert opt.t == 0
    # the state dict: fp32 moments (exact upcast) + the two new keys; fp32 states load into bf16 by round-to-nearest-even
    g = torch.Generator().manual_seed(0)
    opt.m.copy_(torch.randn(128, generator=g))
    opt.v.copy_(torch.rand(128, generator=g))
    sd = opt.state_dict()
    assert sd["m"].dtype == sd["v"].dtype == torch.float32 and sd["moment_dtype"] == "bf16" and sd["moment_seed"] == 0xFFFFFFFFFFFFFFFF
    assert torch.equal(sd["m"].bfloat16().view(torch.int16), opt.m.view(torch.int16))
    assert sorted(set(sd) - set(plain.state_dict())) == ["moment_dtype", "moment_seed"]
    again = FusedAdamW(_stub_engine(), 1e-3, moment_dtype="bf16")
    again.load_state_dict(sd)
    assert torch.equal(again.m.view(torch.int16), opt.m.view(torch.int16)) and torch.equal(again.v.view(torch.int16), opt.v.view(torch.int16))
    full = torch.randn(128, generator=g)
    plain.m.copy_(full)
    plain.v.copy_(full.abs())
    again.load_state_dict(plain.state_dict())                  # an fp32 optimizer's state
    assert torch.equal(again.m.view(torch.int16), full.bfloat16().view(torch.int16))
    plain2 = FusedAdamW(_stub_engine(), 1e-3)
    plain2.load_state_dict(again.state_dict())                 # and back: the bf16 values, exactly
    assert plain2.m.dtype == torch.float32 and torch.equal(plain2.m, again.m.float()) and torch.equal(plain2.v, again.v.float())
