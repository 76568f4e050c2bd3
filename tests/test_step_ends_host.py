"""Properties of the step-ends kernels that need no GPU: the straight-line LayerNorm backward forms for the final norms are in
the library without scratch, issue every load of a wave before their first ``s_waitcnt vmcnt`` and never wait for ``vmcnt(0)``
inside the pipeline (the helpers and the method are those of tests/test_kernel_resources.py); the step-end entry points are declared
in include/maestro_hip.h, exported by the library and bound."""

import re
import shutil
import subprocess
import sys
from pathlib import Path

import pytest

from tests.test_kernel_resources import _kernel_bodies, _loads_before_first_vm_wait

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "scripts"))


def test_final_layernorm_forms_are_in_the_library_without_scratch():
    import kernel_resources as kr
    if not kr.LLVM.exists() or not list((ROOT / "maestro_amd" / "csrc" / "build").glob("*.o")):
        pytest.skip("needs the built objects (python -m maestro_amd.csrc.build) and the ROCm LLVM tools")
    names = {k["kernel"]: k for k in kr.library_kernels()}
    for nv, depth in ((1, 4), (2, 4), (3, 4), (4, 2)):
        for f32 in ("false", "true"):
            form = f"ln_bwd_fast_kernel<{nv}, {depth}, {f32}, false>"
            assert form in names, form
            k = names[form]
            assert k["vgpr_count"] <= 256 and k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, k
    for form, k in names.items():       # the producers with fused column sums and the position-map forms
        if any(t in form for t in ("masked_loss_kernel", "gather_rows_bf16_cs_kernel", "embed_bwd_apply_kernel", "embed_bwd_stats_kernel")):
            assert k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0 and k["vgpr_count"] <= 256, k


def test_final_layernorm_forms_issue_their_loads_before_the_first_wait():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not Path(hipcc).exists():
        pytest.skip("needs hipcc")
    from maestro_amd.csrc import build as B
    flags = [f for f in B.FLAGS if f != "-fPIC"]
    r = subprocess.run([hipcc, *flags, "--cuda-device-only", "-S", "-o", "-", str(B.CSRC / "norm.hip")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    bodies = _kernel_bodies(r.stdout)
    for nv, depth in ((1, 4), (2, 4), (3, 4), (4, 2)):
        for f32 in (0, 1):
            hits = [b for n, b in bodies.items() if f"ln_bwd_fast_kernelILi{nv}ELi{depth}ELb{f32}ELb0E" in n]
            assert len(hits) == 1
            # gamma (NV) + 4 rows x (x, dy) x NV chunks in flight before anything is waited for; every later wait is counted
            assert _loads_before_first_vm_wait(hits[0]) >= 9 * nv, (nv, f32)
            assert not any("s_waitcnt vmcnt(0)" in ln for ln in hits[0]), (nv, f32)


ENDS_NAMES = ("mh_masked_loss_cs_rows", "mh_masked_loss_cs", "mh_masked_loss_bands_cs", "mh_gather_rows_cs_rows",
              "mh_gather_rows_bf16_cs", "mh_embed_bwd_cs_rows", "mh_embed_finish_bwd_ends")


def test_ends_entry_points_are_declared_exported_and_bound():
    import ctypes

    from maestro_amd import hip
    from maestro_amd.csrc.build import LIB
    if not LIB.exists():
        pytest.skip("needs the built library")
    declared = set(re.findall(r"\b(mh_[a-z0-9_]+)\s*\(", (ROOT / "include" / "maestro_hip.h").read_text()))
    handle = ctypes.CDLL(str(LIB))
    binding = (ROOT / "maestro_amd" / "hip.py").read_text()
    for n in ENDS_NAMES:
        assert n in declared, f"{n} is not declared in include/maestro_hip.h"
        assert hasattr(handle, n), n
        assert n in binding, f"{n} is not bound in maestro_amd/hip.py"
    assert hip.COLSUM_ROWS == 16


def test_plain_embed_backward_checks_its_sizes_like_its_siblings():
    """``mh_embed_finish_bwd`` refuses a modality that does not fit its group sequence, and sizes that are not positive, as the
    deterministic and ends forms do.  Every call here fails its check: nothing is launched, the pointers are host addresses that
    nothing dereferences."""
    import ctypes

    from maestro_amd.csrc.build import LIB
    if not LIB.exists():
        pytest.skip("needs the built library")
    lib = ctypes.CDLL(str(LIB))
    lib.mh_last_error.restype = ctypes.c_char_p
    buf = (ctypes.c_float * 16)()
    p, i = ctypes.c_void_p(ctypes.addressof(buf)), ctypes.c_int

    def call(B, D, L, E, tok_off, Lgroup):  # noqa: N803
        return lib.mh_embed_finish_bwd(p, p, p, p, p, p, p, p, i(B), i(D), i(L), i(E), i(tok_off), i(Lgroup), None)

    assert call(1, 2, 3, 8, 1, 6) < 0 and b"mh_embed_finish_bwd: bad sizes" in lib.mh_last_error()        # 1 + 2 * 3 > 6
    for bad in ((0, 2, 3, 8, 0, 6), (1, 0, 3, 8, 0, 6), (1, 2, 0, 8, 0, 6), (1, 2, 3, 0, 0, 6), (1, 2, 3, 6, 0, 6), (1, 2, 3, 8, -1, 6)):
        assert call(*bad) < 0 and b"bad sizes" in lib.mh_last_error(), bad
    assert lib.mh_embed_finish_bwd(None, p, p, p, p, p, p, p, i(1), i(2), i(3), i(8), i(0), i(6), None) < 0 and b"null" in lib.mh_last_error()
