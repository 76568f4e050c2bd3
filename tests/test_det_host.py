"""Deterministic mode without a GPU: the deterministic forms of include/maestro_hip.h (exports, argument checks of the ordered reduction),
the numpy float32 emulation of its summation order -- shared with tests/test_det_kernels_gpu.py, and shown here to have teeth --
and how the public surface resolves the ``deterministic`` switch."""

from __future__ import annotations

import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
LIB = ROOT / "maestro_amd" / "lib" / "libmaestro_hip.so"
ORDERED_ROWS = 16

pytestmark = pytest.mark.skipif(not LIB.exists(), reason="libmaestro_hip.so not built")


# ------------------------------------------------------------------------------------------------ the emulation
def ordered_total(src: np.ndarray, chunk: int = ORDERED_ROWS, reverse: bool = False) -> np.ndarray:
    """``job_total`` of mh_reduce_ordered (include/maestro_hip.h) for ``src`` float32 [rows, cols]: chunk sums (sequential, from +0) summed
    sequentially from +0, every add an IEEE float32 add (numpy float32 arrays add elementwise in float32).  ``chunk`` /
    ``reverse``: deliberately different orders, for the teeth tests."""
    src = np.ascontiguousarray(src, dtype=np.float32)
    if reverse:
        src = src[::-1]
    rows, cols = src.shape
    total = np.zeros(cols, dtype=np.float32)
    for r0 in range(0, rows, chunk):
        s = np.zeros(cols, dtype=np.float32)
        for r in range(r0, min(rows, r0 + chunk)):
            s = s + src[r]
        total = total + s
    assert total.dtype == np.float32
    return total


def ordered_reduce_emulated(srcs, dst_old: np.ndarray | None = None) -> np.ndarray:
    """One chain: ``dst = (ADD ? dst_old : +0) + job_total_0 + job_total_1 + ...`` left to right."""
    cols = srcs[0].shape[1]
    acc = np.zeros(cols, dtype=np.float32) if dst_old is None else np.asarray(dst_old, dtype=np.float32).copy()
    for src in srcs:
        acc = acc + ordered_total(src)
    return acc


def order_sensitive(rows: int, cols: int, seed: int) -> np.ndarray:
    """Normal values scaled per row over about 2^+-12: sums of such rows depend on the order of the adds."""
    rng = np.random.default_rng(seed)
    scale = np.exp2(rng.uniform(-12.0, 12.0, size=(rows, 1)))
    return (rng.standard_normal((rows, cols)) * scale).astype(np.float32)


def bits(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_emulation_matches_a_hand_computed_case():
    f = np.float32
    src = np.array([[1.0], [2.0 ** -24], [2.0 ** -24]] + [[0.0]] * 14 + [[2.0 ** -24]], dtype=np.float32)    # 18 rows: chunks 16 + 2
    # chunk 0: ((1 + 2^-24) + 2^-24) = 1 (each add rounds back to 1, ties to even); chunk 1: 0 + 2^-24; total 1 + 2^-24 -> 1
    assert ordered_total(src)[0] == f(1.0)
    # reversed rows: chunk 0 = 2^-24 + 0 ... + 2^-24 = 2^-23 (the small terms meet before the 1 arrives), chunk 1 = 2^-24 + 1 = 1;
    # total 2^-23 + 1 is representable
    assert ordered_total(src, reverse=True)[0] == f(1.0) + f(2.0 ** -23)


def test_emulation_is_sensitive_to_row_order():
    src = order_sensitive(100, 516, seed=11)
    assert (bits(ordered_total(src)) != bits(ordered_total(src, reverse=True))).any()


def test_emulation_is_sensitive_to_the_chunk_boundary():
    src = order_sensitive(100, 516, seed=12)
    assert (bits(ordered_total(src, chunk=16)) != bits(ordered_total(src, chunk=8))).any()


def test_emulation_chain_order_and_add_flag():
    a, b, c = (order_sensitive(r, 64, seed=20 + i) for i, r in enumerate((17, 33, 5)))
    old = order_sensitive(1, 64, seed=30)[0]
    plain = ordered_reduce_emulated([a, b, c])
    assert (bits(plain) != bits(ordered_reduce_emulated([c, b, a]))).any()
    assert (bits(plain) != bits(ordered_reduce_emulated([a, b, c], dst_old=old))).any()
    assert np.array_equal(bits(ordered_reduce_emulated([a])), bits(np.float32(0.0) + ordered_total(a)))


# ------------------------------------------------------------------------------------------------ the C ABI
class Job(ctypes.Structure):
    _fields_ = [("src", ctypes.c_void_p), ("dst", ctypes.c_void_p), ("rows", ctypes.c_int), ("cols", ctypes.c_int),
                ("ld", ctypes.c_int), ("flags", ctypes.c_int)]


@pytest.fixture(scope="module")
def lib():
    handle = ctypes.CDLL(str(LIB))
    handle.mh_last_error.restype = ctypes.c_char_p
    handle.mh_reduce_ordered.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    return handle


DET_NAMES = ("mh_reduce_ordered", "mh_colsum_partial", "mh_colsum_partial_rows", "mh_masked_loss_det", "mh_masked_loss_bands_det",
             "mh_masked_loss_partial_size", "mh_unmask_token_grad_det", "mh_unmask_token_grad_per_sample_det",
             "mh_unmask_token_grad_partial_rows", "mh_embed_finish_bwd_det", "mh_embed_bwd_partial_rows")


def test_det_entry_points_are_declared_and_exported(lib):
    header = (ROOT / "include" / "maestro_hip.h").read_text()
    assert set(DET_NAMES) <= set(re.findall(r"\b(mh_[a-z0-9_]+)\s*\(", header))
    missing = [n for n in DET_NAMES if not hasattr(lib, n)]
    assert not missing, f"declared in include/maestro_hip.h but not exported: {missing}"


def _table(rows):
    arr = (Job * len(rows))()
    for i, r in enumerate(rows):
        arr[i] = Job(*r)
    return arr


def test_reduce_ordered_rejects_bad_arguments_before_any_launch(lib):
    """No GPU is touched: every call fails its argument check.  The pointers are host addresses that nothing dereferences
    except ``jobs_host`` (the table), which the call reads on the host."""
    buf = (ctypes.c_float * 64)()
    a, b, c = ctypes.addressof(buf), ctypes.addressof(buf) + 64, ctypes.addressof(buf) + 128
    blocks = (ctypes.c_uint64 * 4)()
    good = _table([(a, b, 4, 4, 4, 0)])

    def call(table, n_jobs, n_blocks=1, dev=True, blk=True):
        dev_ptr = ctypes.cast(table, ctypes.c_void_p) if dev and table is not None else None
        return lib.mh_reduce_ordered(ctypes.cast(table, ctypes.c_void_p) if table is not None else None, dev_ptr, n_jobs,
                                     ctypes.cast(blocks, ctypes.c_void_p) if blk else None, n_blocks, None)

    for rc, word in ((call(None, 1), b"null"), (call(good, 1, dev=False), b"null"), (call(good, 1, blk=False), b"null")):
        assert rc < 0 and word in lib.mh_last_error(), lib.mh_last_error()
    for n_jobs, n_blocks in ((0, 1), (-1, 1), (1, 0), (1, -3)):
        assert call(good, n_jobs, n_blocks) < 0 and b"positive" in lib.mh_last_error()
    assert call(_table([(None, b, 4, 4, 4, 0)]), 1) < 0 and b"null" in lib.mh_last_error()
    assert call(_table([(a, None, 4, 4, 4, 0)]), 1) < 0 and b"null" in lib.mh_last_error()
    assert call(_table([(a, b, 4, 8, 4, 0)]), 1) < 0 and b"cols 8 > ld 4" in lib.mh_last_error()
    assert call(_table([(a, b, 0, 4, 4, 0)]), 1) < 0 and b"rows" in lib.mh_last_error()
    # a chain that is split apart: dst b, dst c, dst b again
    split = _table([(a, b, 4, 4, 4, 0), (a, c, 4, 4, 4, 0), (a, b, 4, 4, 4, 0)])
    assert call(split, 3) < 0 and b"split" in lib.mh_last_error()
    split4 = _table([(a, b, 4, 4, 4, 0), (a, c, 4, 4, 4, 0), (a, b, 4, 4, 4, 0), (a, c, 4, 4, 4, 0)])
    assert call(split4, 4) < 0 and b"split" in lib.mh_last_error()
    # members of one chain must agree in cols and flags
    assert call(_table([(a, b, 4, 4, 4, 0), (a, b, 4, 8, 8, 0)]), 2) < 0 and b"chain" in lib.mh_last_error()
    assert call(_table([(a, b, 4, 4, 4, 0), (a, b, 4, 4, 4, 1)]), 2) < 0 and b"chain" in lib.mh_last_error()


def test_first_phase_entry_points_reject_bad_arguments(lib):
    null = ctypes.c_void_p(0)
    i = ctypes.c_int
    assert lib.mh_colsum_partial(null, i(0), null, i(4), i(4), i(4), null) < 0 and b"null" in lib.mh_last_error()
    assert lib.mh_masked_loss_det(null, null, null, null, ctypes.c_float(1.0), null, null, i(1), i(1), i(1), i(0), i(4), i(2), null) < 0
    assert b"null" in lib.mh_last_error()
    assert lib.mh_unmask_token_grad_det(null, null, null, null, i(1), i(4), i(64), i(0), i(0), i(4), null) < 0
    assert lib.mh_embed_finish_bwd_det(null, null, null, null, null, null, null, null, i(1), i(1), i(4), i(64), i(0), i(4), null) < 0
    assert b"null" in lib.mh_last_error()


def test_partial_sizes_depend_on_shapes_alone(lib):
    lib.mh_unmask_token_grad_partial_rows.argtypes = [ctypes.c_long]
    assert [lib.mh_colsum_partial_rows(m) for m in (1, 256, 257, 32768)] == [1, 1, 2, 128]
    assert lib.mh_masked_loss_partial_size(2, 9) == 5 and lib.mh_masked_loss_partial_size(0, 9) == 0
    assert [lib.mh_unmask_token_grad_partial_rows(n) for n in (1, 512, 513)] == [1, 1, 2]
    assert lib.mh_embed_bwd_partial_rows(3, 33) == 6 and lib.mh_embed_bwd_partial_rows(3, 32) == 3


# ------------------------------------------------------------------------------------------------ the switch
def test_switch_resolution(monkeypatch):
    from maestro_amd.engine import resolve_deterministic
    monkeypatch.delenv("MAESTRO_DETERMINISTIC", raising=False)
    assert resolve_deterministic(None) is False and resolve_deterministic(True) is True
    monkeypatch.setenv("MAESTRO_DETERMINISTIC", "1")
    assert resolve_deterministic(None) is True and resolve_deterministic(False) is False     # an explicit kwarg wins
    monkeypatch.setenv("MAESTRO_DETERMINISTIC", "0")
    assert resolve_deterministic(None) is False
    monkeypatch.setenv("MAESTRO_DETERMINISTIC", "true")          # only "1" means on
    assert resolve_deterministic(None) is False


def test_refusals_that_need_no_gpu(monkeypatch):
    from maestro_amd.engine import MAEEngine
    from maestro_amd.engine_sup import SupervisedEngine
    from maestro_amd.train.trainer import PretrainLoop
    with pytest.raises(ValueError, match="fp8"):
        MAEEngine(None, 1, "cpu", dtype="fp8", deterministic=True)
    with pytest.raises(ValueError, match="deterministic"):
        SupervisedEngine(None, 1, "cpu", deterministic=True)
    with pytest.raises(ValueError, match="overlap_optimizer"):
        PretrainLoop(None, 1, "cpu", deterministic=True, overlap_optimizer=True)
    with pytest.raises(ValueError, match="exchange"):
        PretrainLoop(None, 1, "cpu", deterministic=True, exchange=True)
    with pytest.raises(ValueError, match="exchange"):
        PretrainLoop(None, 1, "cpu", deterministic=True, world_size=2)
    monkeypatch.setenv("MAESTRO_DETERMINISTIC", "1")             # the environment switch refuses the same way
    with pytest.raises(ValueError, match="overlap_optimizer"):
        PretrainLoop(None, 1, "cpu", overlap_optimizer=True)


def test_ordered_reduce_descriptor_rejects_malformed_jobs():
    """``hip.OrderedReduce`` checks its jobs before it touches the device: CPU tensors are the first thing it refuses."""
    import torch

    from maestro_amd import hip
    with pytest.raises(hip.HipExtensionError, match="no jobs"):
        hip.OrderedReduce([], "cpu")
    with pytest.raises(hip.HipExtensionError, match="device tensors"):
        hip.OrderedReduce([(torch.zeros(4, 4), torch.zeros(4), 4, 4, 4)], "cpu")
    with pytest.raises(hip.HipExtensionError, match="expected"):
        hip.OrderedReduce([(torch.zeros(4, 4), torch.zeros(4), 4, 4)], "cpu")
