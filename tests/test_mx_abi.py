"""MX block scaling (fp8_scaling="mx"): the three entry points are declared and exported, reject bad arguments before any
launch, and the engine refuses an unknown scaling mode on any machine (no GPU needed)."""

import ctypes
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("mh_gemm_mx", "mh_layernorm_fwd_mx", "mh_quant_mx_batched")


@pytest.fixture(scope="module")
def lib():
    from maestro_amd.csrc.build import LIB, build
    if not LIB.exists():
        build()
    handle = ctypes.CDLL(str(LIB))
    handle.mh_last_error.restype = ctypes.c_char_p
    return handle


def test_mx_entry_points_are_declared_and_exported(lib):
    header = (ROOT / "include" / "maestro_hip.h").read_text()
    declared = set(re.findall(r"\b(mh_[a-z0-9_]+)\s*\(", header))
    for name in NAMES:
        assert name in declared, name
        assert hasattr(lib, name), name
    assert "MX block scaling" in header and "0xFF" in header     # the numerics contract, written once


I, P = ctypes.c_int, ctypes.c_void_p
FAKE = P(0x100000)        # a plausible, 256-B aligned address: never dereferenced, the checks fail first


def _gemm_mx(lib, M=256, N=256, K=256, lda=256, sa=FAKE, ldsa=8, ldb=256, sb=FAKE, ldsb=8, flags=0, c8=P(0), ldc8=0,  # noqa: N803
             c8_scales=P(0), ldc8s=0):
    return lib.mh_gemm_mx(I(M), I(N), I(K), FAKE, I(lda), sa, I(ldsa), FAKE, I(ldb), sb, I(ldsb), FAKE, I(N), I(flags), P(0), P(0),
                          I(0), P(0), P(0), I(0), P(0), c8, I(ldc8), c8_scales, I(ldc8s), P(0))


@pytest.mark.parametrize("kw,msg", [
    (dict(K=200, lda=208, ldb=208), b"multiple of 128"),
    (dict(sa=P(0)), b"null scale"),
    (dict(sb=P(0)), b"null scale"),
    (dict(ldsa=6), b"ldsa"),
    (dict(ldsb=10), b"ldsa"),
    (dict(ldsa=4), b"ldsa"),                                          # < K / 32
    (dict(c8=FAKE, ldc8=256, ldc8s=8), b"c8_scales"),                 # c8 without its scales
    (dict(c8=FAKE, ldc8=256, c8_scales=FAKE, ldc8s=6), b"ldc8s"),
    (dict(flags=1, c8=FAKE, ldc8=256, c8_scales=FAKE, ldc8s=8), b"bf16-output"),
])
def test_gemm_mx_rejects_bad_arguments_before_touching_the_gpu(lib, kw, msg):
    assert _gemm_mx(lib, **kw) == -1
    err = lib.mh_last_error()
    assert err.startswith(b"mh_gemm_mx") and msg in err, err


def test_layernorm_fwd_mx_rejects_bad_arguments_before_touching_the_gpu(lib):
    def ln(y8s=FAKE, ld=32, dim=768):
        return lib.mh_layernorm_fwd_mx(FAKE, I(4), I(0), FAKE, FAKE, FAKE, I(4), I(0), FAKE, FAKE, I(1), I(4), I(dim),
                                       ctypes.c_float(1e-5), FAKE, y8s, I(ld), P(0))
    assert ln(y8s=P(0)) == -1 and b"null scale" in lib.mh_last_error()
    assert ln(ld=26) == -1 and b"ld_y8s" in lib.mh_last_error()
    assert ln(ld=20) == -1 and b"ld_y8s" in lib.mh_last_error()      # < dim / 32
    assert ln(dim=400, ld=16) == -1 and b"dim" in lib.mh_last_error()  # not a multiple of 32


class _Job(ctypes.Structure):
    _fields_ = [("src", P), ("dst", P), ("scales", P), ("rows", I), ("cols", I), ("ld_src", I), ("ld_dst", I), ("ld_s", I),
                ("reserved", I)]


def test_quant_mx_rejects_bad_jobs_before_touching_the_gpu(lib):
    def q(**kw):
        f = dict(src=0x100000, dst=0x200000, scales=0x300000, rows=4, cols=64, ld_src=64, ld_dst=64, ld_s=4)
        f.update(kw)
        jobs = (_Job * 2)(_Job(0x100000, 0x200000, 0x300000, 4, 64, 64, 64, 4, 0), _Job(**f, reserved=0))
        return lib.mh_quant_mx_batched(jobs, I(2), FAKE, FAKE, I(1), P(0))
    assert q(cols=48, ld_src=48, ld_dst=48) == -1 and b"cols % 32" in lib.mh_last_error()
    assert q(scales=0) == -1 and b"null" in lib.mh_last_error()
    assert q(ld_src=62) == -1 and b"ld_src" in lib.mh_last_error()
    assert q(ld_s=1) == -1 and b"ld_s" in lib.mh_last_error()
    assert lib.mh_quant_mx_batched(None, I(0), FAKE, FAKE, I(1), P(0)) == -1 and b"host copy" in lib.mh_last_error()


def test_unknown_fp8_scaling_is_a_value_error_on_any_machine(monkeypatch):
    import maestro_amd.conf as conf
    from maestro_amd.engine import MAEEngine
    from maestro_amd.ssl.mae import mae_tiny
    ds = conf.DatasetsConfig(name_dataset="s2_naip", s2_naip=conf.S2NAIPConfig(filter_inputs=["spot"]))
    model = mae_tiny(datasets=ds, mask=conf.MaskConfig(), interpolate="nearest", fusion_mode="group", inter_depth=1,
                     model="mae", num_levels=1, depth=2)
    with pytest.raises(ValueError, match="bogus"):
        MAEEngine(model, 1, "cpu", dtype="fp8", fp8_scaling="bogus")
    monkeypatch.setenv("MAESTRO_FP8_SCALING", "mxfp4")
    with pytest.raises(ValueError, match="mxfp4"):
        MAEEngine(model, 1, "cpu", dtype="fp8")


def test_mx_scale_pitch_and_mode_resolution(monkeypatch):
    from maestro_amd.fp8 import mx_scale_cols, resolve_scaling
    assert [mx_scale_cols(c) for c in (32, 128, 384, 768, 3072, 160)] == [4, 4, 12, 24, 96, 8]
    monkeypatch.delenv("MAESTRO_FP8_SCALING", raising=False)
    assert resolve_scaling(None) == "tensor" and resolve_scaling("mx") == "mx"
    monkeypatch.setenv("MAESTRO_FP8_SCALING", "mx")
    assert resolve_scaling(None) == "mx" and resolve_scaling("tensor") == "tensor"
