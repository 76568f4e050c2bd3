"""The C-ABI library builds, loads, and exports every symbol include/maestro_hip.h declares (no GPU needed)."""

import ctypes
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def lib():
    from maestro_amd.csrc.build import LIB, build
    if not LIB.exists():
        build()
    return ctypes.CDLL(str(LIB))


def test_every_declared_symbol_is_exported(lib):
    header = (ROOT / "include" / "maestro_hip.h").read_text()
    names = sorted(set(re.findall(r"\b(mh_[a-z0-9_]+)\s*\(", header)))
    assert len(names) >= 108
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing


def test_header_cites_reference_lines():
    header = (ROOT / "include" / "maestro_hip.h").read_text()
    for ref in ("maestro/ssl/mae.py", "maestro/layers/embed.py", "maestro/train/model.py", "maestro/ssl/mim.py",
                "maestro/layers/utils.py", "maestro/dataset/dataset.py", "maestro/layers/head.py", "maestro/layers/overlay.py",
                "maestro/conf/dataset/utils.py"):
        assert ref in header


def test_bad_arguments_are_rejected_before_touching_the_gpu(lib):
    lib.mh_last_error.restype = ctypes.c_char_p
    null = ctypes.c_void_p(0)
    rc = lib.mh_gemm_bf16(ctypes.c_int(7), ctypes.c_int(8), ctypes.c_int(8), ctypes.c_int(8), null, ctypes.c_int(8), null,
                          ctypes.c_int(8), null, ctypes.c_int(8), ctypes.c_int(0), null, null, ctypes.c_int(0), null, null,
                          ctypes.c_int(0), null)
    assert rc < 0 and b"layout" in lib.mh_last_error()
    rc = lib.mh_attn_fwd(null, null, null, ctypes.c_int(1), ctypes.c_int(1), ctypes.c_int(1), ctypes.c_int(64),
                         ctypes.c_float(1.0), null)
    assert rc < 0 and b"null" in lib.mh_last_error()
    assert lib.mh_version() >= 1


def test_product_fails_loudly_without_gpu_or_library(monkeypatch):
    import torch

    import maestro_amd.conf as conf
    from maestro_amd import hip
    from maestro_amd.ssl.mae import mae_tiny
    ds = conf.DatasetsConfig(name_dataset="s2_naip", s2_naip=conf.S2NAIPConfig(filter_inputs=["spot"]))
    model = mae_tiny(datasets=ds, mask=conf.MaskConfig(), interpolate="nearest", fusion_mode="group", inter_depth=1,
                     model="mae", num_levels=1, depth=2)
    batch = {"spot": torch.rand(1, 1, 3, 128, 128), "spot_dates": torch.zeros(1, 1, 3, dtype=torch.int16),
             "ref_date": torch.zeros(1, 1, 3, dtype=torch.int16)}
    with pytest.raises(hip.HipExtensionError):      # CPU tensors: no fallback path exists
        model(batch, ssl_phase="pretrain")
    monkeypatch.setattr(hip, "_lib", None)
    monkeypatch.setattr(hip, "_LIB_PATH", Path("/nonexistent/libmaestro_hip.so"))
    with pytest.raises(hip.HipExtensionError):
        hip.lib()


def test_product_never_imports_the_oracle():
    for py in (ROOT / "maestro_amd").rglob("*.py"):
        text = py.read_text()
        assert not re.search(r"^\s*(from|import)\s+oracle\b", text, re.M), f"{py} imports the oracle"


def test_library_reads_no_environment():
    """include/maestro_hip.h promises "no global mutable state": every tile / ring choice is an argument, the experiment
    switches (MH_GEMM_TILE, MH_GEMM_DMA, MH_GEMM_PP, MH_DMA_STAGGER, MH_FP8_TILE) are parsed on the host side (maestro_amd/hip.py)."""
    for src in list((ROOT / "maestro_amd" / "csrc").glob("*.hip")) + list((ROOT / "maestro_amd" / "csrc").glob("*.hpp")):
        assert "getenv" not in src.read_text(), f"{src.name} reads the environment"


def test_retired_experiment_switches_are_refused(monkeypatch):
    """Round 6: MAESTRO_GROUPED / MH_GEMM_SPLITK / MH_ATTN_BWD / MAESTRO_CU_MASK selected code that no longer exists; a run
    that sets one must fail loudly instead of measuring the default path under the variant's name."""
    import pytest

    from maestro_amd import hip
    monkeypatch.setattr(hip, "_lib", None)
    monkeypatch.setenv("MH_GEMM_SPLITK", "1")
    with pytest.raises(hip.HipExtensionError, match="retired"):
        hip.lib()
    monkeypatch.delenv("MH_GEMM_SPLITK")
    monkeypatch.setattr(hip, "_lib", None)
    assert hip.lib() is not None


def test_every_entry_point_has_a_guard_band_test_or_a_reason():
    """The ledger of tests/guards.py: every ``mh_*`` name of the header is in exactly one of ``GUARDED`` (called by a guard-band
    test) and ``EXEMPT`` (with a reason); a guarded name really occurs -- by name, through the hip.py wrapper of the same name, or
    through the wrapper listed in ``VIA`` -- in one of the guard-test files; besides the seventeen calls that touch no device buffer
    (a literal list: a reason string alone exempts nothing) at most ``MAX_OTHER_EXEMPT`` names are exempt."""
    from tests import guards
    header = (ROOT / "include" / "maestro_hip.h").read_text()
    names = set(re.findall(r"\b(mh_[a-z0-9_]+)\s*\(", header))
    both = guards.GUARDED & set(guards.EXEMPT)
    assert not both, f"in GUARDED and in EXEMPT: {sorted(both)}"
    neither = names - guards.GUARDED - set(guards.EXEMPT)
    assert not neither, f"entry points without a guard-band test or an exemption: {sorted(neither)}"
    unknown = (guards.GUARDED | set(guards.EXEMPT)) - names
    assert not unknown, f"not declared in include/maestro_hip.h: {sorted(unknown)}"
    no_buffer = {"mh_version", "mh_last_error", "mh_gemm_sk_workspace", "mh_gemm_bf16_resolve_tile", "mh_groupnorm_partial_size",
                 "mh_layernorm_bwd_workspace", "mh_attn_reduce_partial_rows", "mh_colsum_partial_rows", "mh_masked_loss_partial_size",
                 "mh_embed_bwd_partial_rows", "mh_unmask_token_grad_partial_rows", "mh_masked_loss_cs_rows", "mh_gather_rows_cs_rows",
                 "mh_embed_bwd_cs_rows", "mh_grad_sumsq_partial_rows", "mh_knn_splits", "mh_knn_workspace_bytes"}
    other = {n: r for n, r in guards.EXEMPT.items() if n not in no_buffer}
    assert guards.MAX_OTHER_EXEMPT == 6 and len(other) <= 6, f"{len(other)} exemptions besides the seventeen size / rule / version calls: {sorted(other)}"
    for n, reason in guards.EXEMPT.items():
        assert isinstance(reason, str) and reason.strip() and "\n" not in reason, f"{n}: a one-line reason is required"
    # outside test_guard_bands_gpu.py a guard section starts at the file's "guard bands" banner: only calls below it count there
    parts = []
    for f in guards.GUARD_TEST_FILES:
        body = (ROOT / "tests" / f).read_text()
        parts.append(body if f == "test_guard_bands_gpu.py" else body.partition("guard bands (tests/guards.py)")[2])
    text = re.sub(r"#[^\n]*", "", re.sub(r'"""[\s\S]*?"""', "", "\n".join(parts)))      # code only: no docstrings, no comments
    absent = []
    for n in sorted(guards.GUARDED):
        forms = [rf"\b{n}\b", rf"\bhip\.{n[3:]}\(", re.escape(guards.VIA[n])] if n in guards.VIA else [rf"\b{n}\b", rf"\bhip\.{n[3:]}\("]
        if not any(re.search(form, text) for form in forms):
            absent.append(n)
    assert not absent, f"in GUARDED but called by no guard test: {absent}"
