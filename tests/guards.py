"""Poisoned guard bands for kernel tests (a plain helper module: no fixtures, no plugin).

The product hands the kernels views into shared storage: ``ParamStore`` keeps all weights, gradients and bf16 shadows as adjacent
slices of three flat buffers, sequence buffers are shared through row maps, and every matrix of the C ABI has a leading dimension.
A store one row, column or vector past an output, or a load past an input that is "masked" by arithmetic (``0 * NaN``), is
silent when every test operand is a private, dense, exactly-sized allocation.  ``guarded`` puts the operand in the MIDDLE of one
flat allocation instead:

    [ front band | row 0 .. cols | pad | row 1 .. cols | pad | ... | back band ]

Bands and pad columns are poison: NaN for floats (inputs and outputs alike), ``0x7F`` (e4m3 NaN) for fp8 bytes, ``0xFF`` (E8M0
NaN) for MX scale bytes, a fixed odd byte pattern for other integers, or -- for index tensors, ``trap_index`` -- a VALID index
that points at a NaN "trap row" the test appends to the indexed source, so an over-read index shows up as NaN in the output
and never as an out-of-range access.  After the call the checker compares the RAW BITS of everything around the view (and, for
inputs, of the view itself) with a copy saved before the call (``NaN != NaN``, so never a float compare) and names the first
changed element relative to the view.

SAFETY.  Each band is the larger of 64 KiB and 256 rows of ``ld`` elements.  The size is not about detection, it is about the
card: any overrun bounded by one tile (the tallest tile here is 256 rows) stays inside the test's OWN allocation, so a wrong
kernel fails an assertion and does not fault a GPU that others share.  Tests built on this module must never be shaped to reach
outside their allocation: every size, offset and index they pass is in range, and only the kernel's own error can leave the view.
"""

from __future__ import annotations

import math

import torch

BAND_BYTES = 64 * 1024
BAND_ROWS = 256
_ALIGN_UNIT = 256          # bands are whole multiples of this many bytes, so the view's alignment is decided by `align` alone
INT_PATTERN = 0x5B         # "other integer buffers": a fixed odd byte
FP8_NAN, E8M0_NAN = 0x7F, 0xFF

_BITS = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _fill_value(dtype: torch.dtype, fill):
    """The poison for ``dtype``: ``fill`` = None (by type), "fp8", "e8m0", "int", or a number / list of numbers (tiled)."""
    if fill is None:
        fill = "nan" if dtype.is_floating_point else "int"
    if isinstance(fill, str):
        if fill == "nan":
            if not dtype.is_floating_point:
                raise ValueError("NaN poison needs a float dtype")
            return [float("nan")]
        if dtype.is_floating_point:
            raise ValueError(f"fill {fill!r} is for integer buffers")
        byte = {"fp8": FP8_NAN, "e8m0": E8M0_NAN, "int": INT_PATTERN}[fill]
        if fill != "int" and dtype != torch.uint8:
            raise ValueError(f"fill {fill!r} is for uint8 buffers")
        size = torch.empty(0, dtype=dtype).element_size()
        return [int.from_bytes(bytes([byte]) * size, "little", signed=False) if dtype == torch.uint8
                else int.from_bytes(bytes([byte]) * size, "little", signed=True)]
    if isinstance(fill, (int, float)):
        return [fill]
    return list(fill)


class Guard:
    """The checker ``guarded`` returns next to the view.  ``arm()`` (re)saves the bits; calling the object asserts that bands and
    pads (and the view itself when ``whole``: an input) still hold them."""

    def __init__(self, flat, view, front, rows, cols, ld, name, whole):
        self.flat, self.view, self.front, self.rows, self.cols, self.ld = flat, view, front, rows, cols, ld
        self.name, self.whole = name, whole
        self.saved = None
        self.arm()

    def _bits(self):
        return self.flat.view(_BITS[self.flat.element_size()])

    def arm(self, whole: bool | None = None) -> None:
        if whole is not None:
            self.whole = whole
        self.saved = self._bits().clone()

    def span(self):
        """The flat 1-D tensor over the view's rows INCLUDING their pad columns (``rows * ld`` elements): for wrappers that size-check
        a buffer by ``numel``."""
        return self.flat[self.front: self.front + self.rows * self.ld]

    def _interior(self):
        """Boolean mask over the flat buffer: the elements of the view."""
        m = torch.zeros(self.flat.numel(), dtype=torch.bool, device=self.flat.device)
        body = m[self.front: self.front + self.rows * self.ld].view(self.rows, self.ld)
        body[:, : self.cols] = True
        return m

    def where(self, flat_index: int) -> str:
        """Location of a flat element relative to the view, in the words of the C ABI (row M+0 = the first row behind the view)."""
        o = flat_index - self.front
        r, c = o // self.ld, o % self.ld          # floor division: rows in front of the view are negative
        col = f"pad col N+{c - self.cols}" if c >= self.cols else f"col {c}"
        if r < 0:
            return f"front band: row {r}, {col}"
        if r >= self.rows:
            return f"back band: row M+{r - self.rows}, {col}"
        if c >= self.cols:
            return f"{col} of row {r}"
        return f"row {r}, {col}"

    def first_change(self):
        """None, or (location string, flat index) of the first element whose bits changed."""
        diff = self._bits() != self.saved
        if not self.whole:
            diff &= ~self._interior()
        if not bool(diff.any()):
            return None
        i = int(diff.nonzero()[0, 0])
        return self.where(i), i

    def __call__(self) -> None:
        hit = self.first_change()
        assert hit is None, (f"{self.name}: {'input' if self.whole else 'guard band'} changed at {hit[0]} "
                             f"(view [{self.rows}, {self.cols}], ld {self.ld})")


def guarded(shape, dtype, device, ld=None, fill=None, *, data=None, init=None, align=16, name="buffer"):
    """One flat allocation with a view of ``shape`` in its middle; returns ``(view, checker)``.

    ``shape``  the last dimension is the row (``cols``); all leading dimensions together are the rows, ``ld`` elements apart
               (default ``cols``: dense).  ``ld > cols`` puts ``ld - cols`` poisoned pad columns behind every row.
    ``fill``   the poison of bands and pads: by default NaN for floats and ``INT_PATTERN`` bytes for integers; "fp8" = 0x7F,
               "e8m0" = 0xFF (uint8 only); a number or a list of numbers is tiled from the view's origin (``trap_index``).
    ``data``   copied into the view: the buffer is an INPUT and the checker also requires the view itself to keep its bits.
    ``init``   outputs: what the view holds before the call (default: the poison, so an element the kernel forgets is not finite).
    ``align``  the view's base is a multiple of ``align`` bytes and NOT of ``2 * align``: exactly what the entry point documents.

    Band size: the larger of 64 KiB and 256 rows of ``ld`` elements on each side -- see the module docstring: a one-tile overrun
    of a wrong kernel stays inside this allocation and fails the checker instead of faulting the card.
    """
    shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
    cols = shape[-1]
    rows = math.prod(shape[:-1])
    ld = cols if ld is None else int(ld)
    if ld < cols or min(shape) <= 0:
        raise ValueError(f"guarded: shape {shape} with ld {ld}")
    esz = torch.empty(0, dtype=dtype).element_size()
    if align % esz or _ALIGN_UNIT % (2 * align):
        raise ValueError(f"guarded: align {align} for {esz}-byte elements")
    unit = _ALIGN_UNIT // esz
    band = -(-max(BAND_BYTES // esz, BAND_ROWS * ld) // unit) * unit
    pattern = _fill_value(dtype, fill)
    if band % len(pattern) or (align // esz) % len(pattern):
        raise ValueError("guarded: the fill pattern does not tile the bands")
    front = band + align // esz            # an odd multiple of `align`: no stricter alignment than documented
    total = front + rows * ld + band
    flat = torch.tensor(pattern, dtype=dtype).repeat(-(-total // len(pattern)))[:total].to(device).contiguous()
    assert flat.data_ptr() % _ALIGN_UNIT == 0 or flat.device.type == "cpu", "allocator gave an unaligned buffer"
    strides = [1] * len(shape)
    strides[-1] = 1
    if len(shape) > 1:
        strides[-2] = ld
        for i in range(len(shape) - 3, -1, -1):
            strides[i] = strides[i + 1] * shape[i + 1]
    view = flat.as_strided(shape, strides, front)
    if data is not None:
        view.copy_(data.to(dtype).reshape(shape))
    elif init is not None:
        view.fill_(init)
    return view, Guard(flat, view, front, rows, cols, ld, name, whole=data is not None)


def trap_index(values, trap, device, ld=None, *, align=16, name="index"):
    """An index INPUT (``idx``, ``inv``, ``tok_slot``, ``date_row``, ``slot_map``, ``spans``) whose bands and pads hold ``trap``: a
    VALID index (or, for ``spans``, a list = one valid record, tiled) that points at a NaN trap row / trap region the test has
    appended to the indexed source.  A kernel that reads an index past the view then produces a NaN (or changes the trap region)
    inside the test's own buffers; no out-of-range index exists anywhere.  Returns ``(view, checker)``."""
    return guarded(values.shape, values.dtype, device, ld=ld, fill=trap, data=values, align=align, name=name)


class GuardSet:
    """Collects the buffers of one kernel call: ``inp`` / ``out`` / ``idx`` return views, ``check()`` runs every checker."""

    def __init__(self, device):
        self.device, self.guards = device, []

    def _add(self, pair):
        self.guards.append(pair[1])
        return pair[0]

    def inp(self, data, ld=None, fill=None, align=16, name="input"):
        return self._add(guarded(data.shape, data.dtype, self.device, ld=ld, fill=fill, data=data, align=align, name=name))

    def out(self, shape, dtype=torch.float32, ld=None, fill=None, init=None, align=16, name="output"):
        return self._add(guarded(shape, dtype, self.device, ld=ld, fill=fill, init=init, align=align, name=name))

    def idx(self, values, trap, ld=None, align=16, name="index"):
        return self._add(trap_index(values, trap, self.device, ld=ld, align=align, name=name))

    def arm(self) -> None:
        """Re-save every buffer's bits (after the test has written more inputs into the views)."""
        for g in self.guards:
            g.arm()

    def check(self) -> None:
        if self.device.type == "cuda":
            torch.cuda.synchronize()
        for g in self.guards:
            g()


def bits_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Bit compare of two tensors of one dtype and shape (NaN-safe)."""
    a, b = a.contiguous(), b.contiguous()
    return bool(torch.equal(a.view(_BITS[a.element_size()]), b.view(_BITS[b.element_size()])))


# ---------------------------------------------------------------------------------------------------- the ledger
# Every mh_* entry point of include/maestro_hip.h is in exactly one of GUARDED (called by a guard-band test: tests/
# test_guard_bands_gpu.py, or the guard section -- the text below the "guard bands (tests/guards.py)" banner -- of the other
# files listed here) and EXEMPT; tests/test_abi.py enforces it, so a new entry point cannot arrive without a decision.
GUARD_TEST_FILES = ("test_guard_bands_gpu.py", "test_fp8_gpu.py", "test_mx_gpu.py", "test_det_kernels_gpu.py",
                    "test_step_ends_gpu.py", "test_metrics_gpu.py", "test_date_select_gpu.py", "test_mask_rng_gpu.py",
                    "test_grad_guard_gpu.py", "test_adamw_groups_gpu.py", "test_adamw_moments_gpu.py", "test_predict_gpu.py",
                    "test_scene_gpu.py", "test_knn_gpu.py")

# name -> how a guard test reaches it when not by its own name or the hip.py wrapper of the same name (hip.<name without mh_>)
VIA = {
    "mh_gemm_bf16_tile": "hip._gemm_tile(",
    "mh_gemm_bf16_sk": "hip._gemm_tile(",          # hip._gemm_tile routes the MH_TILE_SK_* ids to hip.gemm_sk = mh_gemm_bf16_sk
    "mh_gemm_grouped_tn": "hip.GroupedTN(",
    "mh_colsum_batched": "hip.ColsumBatch(",
    "mh_quant_batched": "hip.QuantBatch(",
    "mh_quant_mx_batched": "hip.QuantMxBatch(",
    "mh_transpose_u8_batched": "hip.TransposeBatch(",
    "mh_reduce_ordered": "hip.OrderedReduce(",
    "mh_mask_draw": "hip.MaskDraw(",
}

GUARDED = {
    "mh_gemm_bf16", "mh_gemm_bf16_tile", "mh_gemm_bf16_sk", "mh_gemm_grouped_tn",
    "mh_attn_fwd", "mh_attn_bwd",
    "mh_layernorm_fwd", "mh_layernorm_fwd_fp8", "mh_layernorm_fwd_mx", "mh_layernorm_bwd", "mh_layernorm_bwd_partial",
    "mh_patchify", "mh_patchify_bands", "mh_groupnorm_stats", "mh_embed_finish", "mh_embed_finish_bwd", "mh_depatchify",
    "mh_date_features", "mh_resize", "mh_rescale_elev", "mh_dihedral",
    "mh_mask_select", "mh_gather_rows", "mh_scatter_rows", "mh_expand_rows", "mh_unmask_assemble", "mh_unmask_token_grad",
    "mh_unmask_assemble_per_sample", "mh_unmask_token_grad_per_sample", "mh_count_masked", "mh_count_masked_elems",
    "mh_masked_loss", "mh_masked_loss_bands",
    "mh_token_resize", "mh_token_resize_bwd", "mh_attn_reduce_fwd", "mh_attn_reduce_bwd", "mh_mean_reduce_fwd", "mh_mean_reduce_bwd",
    "mh_head_linear_fwd", "mh_head_linear_bwd", "mh_count_valid", "mh_ce_loss", "mh_bce_loss",
    "mh_colsum", "mh_colsum_batched", "mh_cast_bf16", "mh_pack_rows_bf16", "mh_unpack_rows_add",
    "mh_adamw", "mh_adamw_dev", "mh_scale_dev", "mh_zero_spans",
    "mh_gemm_fp8", "mh_gemm_mx", "mh_quant_batched", "mh_quant_mx_batched", "mh_transpose_u8_batched", "mh_fp8_update_scales",
    "mh_adamw_fp8",
    "mh_adamw_groups", "mh_adamw_groups_dev", "mh_adamw_bf16m", "mh_adamw_bf16m_dev", "mh_adamw_groups_bf16m", "mh_adamw_groups_bf16m_dev",
    "mh_mask_draw", "mh_grad_sumsq_partial", "mh_grad_guard_finish",
    "mh_reduce_ordered", "mh_colsum_partial", "mh_masked_loss_det", "mh_masked_loss_bands_det", "mh_unmask_token_grad_det",
    "mh_unmask_token_grad_per_sample_det", "mh_embed_finish_bwd_det",
    "mh_masked_loss_cs", "mh_masked_loss_bands_cs", "mh_gather_rows_bf16_cs", "mh_embed_finish_bwd_ends",
    "mh_confusion_ce", "mh_confusion_bce", "mh_select_dates",
    "mh_predict_view", "mh_predict_finish", "mh_window_gather", "mh_predict_blend", "mh_predict_blend_finish",
    "mh_l2_normalize", "mh_knn_topk", "mh_knn_vote",
}

# The calls that touch no device buffer (sizes, version, error text) are exempt as such; at most MAX_OTHER_EXEMPT further names
# may be added, each with a reason that is a property of the entry point.
NO_DEVICE_BUFFER = "touches no device buffer"
EXEMPT = {
    "mh_version": NO_DEVICE_BUFFER,
    "mh_last_error": NO_DEVICE_BUFFER,
    "mh_gemm_sk_workspace": NO_DEVICE_BUFFER,
    "mh_gemm_bf16_resolve_tile": NO_DEVICE_BUFFER,
    "mh_groupnorm_partial_size": NO_DEVICE_BUFFER,
    "mh_layernorm_bwd_workspace": NO_DEVICE_BUFFER,
    "mh_attn_reduce_partial_rows": NO_DEVICE_BUFFER,
    "mh_colsum_partial_rows": NO_DEVICE_BUFFER,
    "mh_masked_loss_partial_size": NO_DEVICE_BUFFER,
    "mh_embed_bwd_partial_rows": NO_DEVICE_BUFFER,
    "mh_unmask_token_grad_partial_rows": NO_DEVICE_BUFFER,
    "mh_masked_loss_cs_rows": NO_DEVICE_BUFFER,
    "mh_gather_rows_cs_rows": NO_DEVICE_BUFFER,
    "mh_embed_bwd_cs_rows": NO_DEVICE_BUFFER,
    "mh_grad_sumsq_partial_rows": NO_DEVICE_BUFFER,
    "mh_knn_splits": NO_DEVICE_BUFFER,
    "mh_knn_workspace_bytes": NO_DEVICE_BUFFER,
}
MAX_OTHER_EXEMPT = 6
