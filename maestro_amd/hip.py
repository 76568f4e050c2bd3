"""ctypes binding of libmaestro_hip.so (the C ABI in include/maestro_hip.h) for torch device tensors.

There is NO fallback: if the library is missing or a tensor is not on the GPU the call raises.  PyTorch is used
only for device memory and the current HIP stream.  ``KernelTimer`` (bottom of the file) brackets the MFMA kernels
with HIP events on their launch stream for bench.py's roofline leg.
"""

from __future__ import annotations

import contextlib
import ctypes
import math
import os
from pathlib import Path

import torch

_LIB_PATH = Path(__file__).resolve().parent / "lib" / "libmaestro_hip.so"
_lib = None

GEMM_NT, GEMM_NN, GEMM_TN = 0, 1, 2
OUT_F32, BIAS, GELU, RESIDUAL, DGELU, ATOMIC, COLSUM, AUX_DGELU, MULAUX, C8_E5M2, AUX_U8 = 1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024


class HipExtensionError(RuntimeError):
    pass


def lib() -> ctypes.CDLL:
    """Load the HIP extension; fail loudly when it is absent (no CPU/PyTorch fallback exists)."""
    global _lib
    if _lib is None:
        if not _LIB_PATH.exists():
            raise HipExtensionError(
                f"{_LIB_PATH} not found: build it with `python -m maestro_amd.csrc.build` "
                "(or __graft_entry__.build()).  The MAE hot path has no fallback implementation.")
        retired = [v for v in ("MAESTRO_GROUPED", "MH_GEMM_SPLITK", "MH_ATTN_BWD", "MAESTRO_CU_MASK") if os.environ.get(v)]
        if retired:     # their kernels / code paths were removed (rounds 5-6): refuse instead of silently running the default path
            raise HipExtensionError(f"{', '.join(retired)}: retired experiment switch(es) -- the variant no longer exists, this run "
                                    "would measure the default path (INTEGRATION.md, profiles/r05_experiments.md, r06_experiments.md)")
        _lib = ctypes.CDLL(str(_LIB_PATH))
        _lib.mh_last_error.restype = ctypes.c_char_p
        _lib.mh_layernorm_bwd_workspace.restype = _lib.mh_gemm_sk_workspace.restype = ctypes.c_long     # the size calls that return long
        _lib.mh_attn_reduce_partial_rows.restype = ctypes.c_long
        vp, ci = ctypes.c_void_p, ctypes.c_int          # confusion matrices
        _lib.mh_confusion_ce.argtypes = [vp, vp, ci, ctypes.c_long, vp, ci, ci, ci, ci, ci, vp]
        _lib.mh_confusion_bce.argtypes = [vp, vp, ctypes.c_float, ctypes.c_float, vp, ci, ci, vp]
        _lib.mh_confusion_ce.restype = _lib.mh_confusion_bce.restype = ci
        _lib.mh_predict_view.argtypes = [vp, vp, ci, ctypes.c_float, vp, ci, vp, vp, ci, ci, ci, ci, ci, vp]     # predictions
        _lib.mh_predict_finish.argtypes = [vp, ctypes.c_float, ci, ctypes.c_float, vp, vp, vp, ci, ci, ctypes.c_long, vp]
        _lib.mh_predict_view.restype = _lib.mh_predict_finish.restype = ci
        _lib.mh_window_gather.argtypes = [vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, vp]                          # scene prediction
        _lib.mh_predict_blend.argtypes = [vp, ctypes.c_float, vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, vp]
        _lib.mh_predict_blend_finish.argtypes = [vp, vp, vp, vp, vp, ci, ci, ctypes.c_long, vp]
        _lib.mh_window_gather.restype = _lib.mh_predict_blend.restype = _lib.mh_predict_blend_finish.restype = ci
        _lib.mh_knn_splits.argtypes = [ci, ci, ci, ci]                                                                # nearest neighbours
        _lib.mh_knn_workspace_bytes.argtypes = [ci, ci, ci]
        _lib.mh_knn_workspace_bytes.restype = ctypes.c_long
        _lib.mh_l2_normalize.argtypes = [vp, ctypes.c_long, ctypes.c_float, vp, ctypes.c_long, vp, ctypes.c_long, ctypes.c_long, ci, vp]
        _lib.mh_knn_topk.argtypes = [vp, ctypes.c_long, vp, ctypes.c_long, ctypes.c_long, vp, vp, ci, vp, ctypes.c_long, ci, ci, ci, ci, ci, vp]
        _lib.mh_knn_vote.argtypes = [vp, vp, vp, ctypes.c_long, ci, ctypes.c_float, ci, ci, vp, ctypes.c_long, vp, ci, ci, vp]
        _lib.mh_knn_splits.restype = _lib.mh_l2_normalize.restype = _lib.mh_knn_topk.restype = _lib.mh_knn_vote.restype = ci
        _lib.mh_reduce_ordered.argtypes = [vp, vp, ci, vp, ci, vp]          # deterministic forms
        _lib.mh_colsum_partial_rows.argtypes = [ci]
        _lib.mh_masked_loss_partial_size.argtypes = _lib.mh_embed_bwd_partial_rows.argtypes = [ci, ci]
        _lib.mh_unmask_token_grad_partial_rows.argtypes = [ctypes.c_long]
        _lib.mh_masked_loss_cs_rows.argtypes = [ci, ci]                     # step ends
        _lib.mh_gather_rows_cs_rows.argtypes = _lib.mh_embed_bwd_cs_rows.argtypes = [ctypes.c_long]
        _lib.mh_select_dates.argtypes = [vp, ci, vp, ci, ci, vp, vp, vp, ci, vp, vp, vp, vp, ci, ci, ci, ctypes.c_long, ci, ci,
                                         ctypes.c_float, vp]               # input staging
        _lib.mh_select_dates.restype = ci
        _lib.mh_mask_draw.argtypes = [vp, vp, ci, vp, vp, ci, ctypes.c_uint64, ctypes.c_longlong, ctypes.c_longlong, vp]   # device-side draws
        _lib.mh_mask_draw.restype = ci
        cl, cf, u64 = ctypes.c_long, ctypes.c_float, ctypes.c_uint64
        _lib.mh_grad_sumsq_partial_rows.argtypes = [cl]                     # gradient guard
        _lib.mh_grad_sumsq_partial_rows.restype = cl
        _lib.mh_grad_sumsq_partial.argtypes = [vp, cl, vp, vp, vp]
        _lib.mh_grad_guard_finish.argtypes = [vp, vp, cl, cf, cf, ci, cf, cf, cf, vp, vp, vp]
        _lib.mh_grad_sumsq_partial.restype = _lib.mh_grad_guard_finish.restype = ci
        # AdamW: {plain | grouped} x {host | device scalars}, fp32 moments, then the same four with bf16 moments (elem_base, seed)
        _lib.mh_adamw_groups.argtypes = [vp] * 8 + [cl, cf, cf, cf, cf, ci, cf, vp]
        _lib.mh_adamw_groups_dev.argtypes = [vp] * 8 + [cl, cf, cf, cf, vp, vp]
        _lib.mh_adamw_bf16m.argtypes = [vp] * 5 + [cl, cl, u64, cf, cf, cf, cf, cf, ci, cf, vp]
        _lib.mh_adamw_bf16m_dev.argtypes = [vp] * 5 + [cl, cl, u64, cf, cf, cf, cf, vp, vp, vp]
        _lib.mh_adamw_groups_bf16m.argtypes = [vp] * 8 + [cl, cl, u64, cf, cf, cf, cf, ci, cf, vp]
        _lib.mh_adamw_groups_bf16m_dev.argtypes = [vp] * 8 + [cl, cl, u64, cf, cf, cf, vp, vp, vp]
        for name in ("groups", "groups_dev", "bf16m", "bf16m_dev", "groups_bf16m", "groups_bf16m_dev"):
            getattr(_lib, "mh_adamw_" + name).restype = ci
    return _lib


def _check(rc: int, what: str) -> None:
    if rc != 0:
        msg = lib().mh_last_error().decode(errors="replace")
        raise HipExtensionError(f"{what} failed (rc={rc}): {msg}")


def ptr(t: torch.Tensor | None):
    if t is None:
        return ctypes.c_void_p(0)
    if not t.is_cuda:
        raise HipExtensionError("maestro_amd kernels need GPU tensors (no CPU fallback)")
    return ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


_I, _F, _L = ctypes.c_int, ctypes.c_float, ctypes.c_long


# ---- GEMM: kernel / tile choice (include/maestro_hip.h MH_TILE_*)
TILE_AUTO, TILE_REG_128, TILE_DMA_256, TILE_DMA_256x128, TILE_DMA_128x256, TILE_DMA_128, TILE_DMA_128x4 = -1, 0, 1, 2, 3, 4, 5
TILE_DMA_256_LOCKSTEP = 6   # MH_TILE_DMA_256 without the wave-group stagger (A/B experiments)
TILE_REG_64, TILE_REG_192 = 13, 14   # the register-staged kernel with 64 x 128 / 192 x 128 tiles
TILE_SK_192, TILE_SK_256, TILE_SK_DMA_256 = 15, 16, 17   # stream-K tiles (gemm_sk.hip, gemm_sk_dma.hip): routed to mh_gemm_bf16_sk with a per-stream workspace
SK_TILES = (TILE_SK_192, TILE_SK_256, TILE_SK_DMA_256)
TILE_PP_128 = 7             # persistent 128x128 tile, epilogue of tile t inside the main loop of tile t + 1 (gemm_pp.hip)
TILES = (TILE_REG_128, TILE_DMA_256, TILE_DMA_256x128, TILE_DMA_128x256, TILE_DMA_128, TILE_DMA_128x4)
_LAYOUT_NAME = {0: "NT", 1: "NN", 2: "TN"}
_TILE_NAME = {TILE_REG_128: "gemm_kernel<{}>", TILE_DMA_256: "gemm_dma_kernel<256x256,{}>",
              TILE_DMA_256x128: "gemm_dma_kernel<256x128,{}>", TILE_DMA_128x256: "gemm_dma_kernel<128x256,{}>",
              TILE_DMA_128: "gemm_dma_kernel<128x128,{}>", TILE_DMA_128x4: "gemm_dma_kernel<128x128q,{}>",
              TILE_DMA_256_LOCKSTEP: "gemm_dma_kernel<256x256,{}>", TILE_PP_128: "gemm_pp_kernel<{}>",
              TILE_REG_64: "gemm_kernel<{},64x128>", TILE_REG_192: "gemm_kernel<{},192x128>",
              TILE_SK_192: "gemm_sk_kernel<{},192x128>", TILE_SK_256: "gemm_sk_kernel<{},256x128>",
              TILE_SK_DMA_256: "gemm_sk_dma_kernel<256x256,{}>"}
_tile_choice: dict = {}     # (layout, M, N, K, flags) -> fastest tile, filled while tuning is on
_tuning = False


def set_gemm_tuning(on: bool) -> None:
    """While on, the first call of every distinct (layout, M, N, K, flags) times each eligible tile on the call's own
    operands (device-synchronising: eager launches only, never inside a hipGraph capture) and keeps the fastest."""
    global _tuning
    _tuning = bool(on)


def gemm_tile_choices() -> dict:
    return dict(_tile_choice)


class InStepTuner:
    """Picks, per GEMM signature of a step, the tile that is fastest INSIDE the step.

    Round 3 finding (profiles/README.md): the fastest tile in an isolated loop (hot operands, nothing else on the chip) is often
    not the fastest between the step's other kernels -- the isolated ranking cost the probe step 2.5 % -- while HIP-event times
    of the step's own eager launches predicted the whole-step A/B.  So the engine runs its first step several times with the
    same inputs and draws, one candidate tile per pass for every signature at once (``begin``), each launch bracketed by events on
    its stream; ``finish`` keeps a candidate only where it beats the library's rule (MH_TILE_AUTO) by ``margin`` over all
    launches of that signature, else the rule stays.  Choices land in the process-wide table ``_pick_tile`` consults."""

    CANDIDATES = (TILE_AUTO, TILE_REG_128, TILE_PP_128, TILE_REG_64, TILE_REG_192, TILE_DMA_256) + (
        (TILE_SK_DMA_256, TILE_SK_192, TILE_SK_256) if os.environ.get("MAESTRO_INSTEP_SK") == "1" else ())   # round 6: the stream-K tiles

    def __init__(self) -> None:
        self.cand, self.ev, self.bad = None, {}, set()

    def begin(self, cand) -> None:
        """``None``: launches run under the rule and are not timed (the warm-up pass)."""
        self.cand = cand

    def open(self, key):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        self.ev.setdefault(key, {}).setdefault(self.cand, []).append((e0, e1))
        return e0, e1

    def reject(self, key) -> None:
        self.bad.add((key, self.cand))

    def finish(self, margin: float = 0.03) -> dict:
        torch.cuda.synchronize()
        report = {}
        for key, per in self.ev.items():
            base_n = len(per.get(TILE_AUTO, ()))
            ms = {c: sum(a.elapsed_time(b) for a, b in evs) for c, evs in per.items()
                  if (key, c) not in self.bad and len(evs) == base_n and base_n}
            if TILE_AUTO not in ms:
                continue
            best = min(ms, key=ms.get)
            pick = best if ms[best] < (1.0 - margin) * ms[TILE_AUTO] else TILE_AUTO
            _tile_choice[key] = pick
            report[key] = (pick, ms)
        return report


_instep: InStepTuner | None = None


def set_instep_tuner(t: InStepTuner | None) -> None:
    global _instep
    _instep = t


# ---- stream-K GEMM (mh_gemm_bf16_sk): one workspace per (stream, tile, grid) -- launches on different streams may overlap and must not
# share flag words or partial slots.  Zeroed once at allocation; the kernel leaves its flag words zero.  Allocated on first use, so the
# first call of a new (stream, tile, grid) must be an eager one (the engine's warm-up passes run before any hipGraph capture).
_sk_ws: dict = {}
_sk_grid = None


def sk_grid() -> int:
    """Persistent workgroups of a stream-K launch: one per CU (MH_SK_GRID overrides, e.g. the CU count of a masked stream)."""
    global _sk_grid
    if _sk_grid is None:
        env = os.environ.get("MH_SK_GRID")
        _sk_grid = int(env) if env else torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    return _sk_grid


def sk_workspace(tile: int, grid: int) -> torch.Tensor:
    key = (torch.cuda.current_stream().cuda_stream, tile, grid)
    ws = _sk_ws.get(key)
    if ws is None:
        nbytes = lib().mh_gemm_sk_workspace(_I(tile), _I(grid))
        if nbytes <= 0:
            raise HipExtensionError(f"mh_gemm_sk_workspace({tile}, {grid}) = {nbytes}")
        if torch.cuda.is_current_stream_capturing():
            raise HipExtensionError("stream-K workspace requested for the first time inside a hipGraph capture: run the step eagerly once first")
        ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        _sk_ws[key] = ws
    return ws


def sk_error_flag(ws: torch.Tensor) -> int:
    """1 if a finisher's wait for a partial ran into its bound in any launch that used this workspace (results are then wrong)."""
    return int(ws[4092:4096].view(torch.int32).item())


def gemm_sk(tile: int, layout: int, M: int, N: int, K: int, A, lda: int, B, ldb: int, C, ldc: int, flags: int = 0, bias=None,  # noqa: N803
            res=None, ldr: int = 0, grid: int | None = None) -> int:
    """Returns the library's code: 0 launched, -2 the problem is not served by the stream-K kernel (nothing launched)."""
    grid = grid or sk_grid()
    ws = sk_workspace(tile, grid)
    return lib().mh_gemm_bf16_sk(_I(tile), _I(layout), _I(M), _I(N), _I(K), ptr(A), _I(lda), ptr(B), _I(ldb), ptr(C), _I(ldc),
                                 _I(flags), ptr(bias), ptr(res), _I(ldr), ptr(ws), _L(ws.numel()), _I(grid), stream())


def _gemm_tile(tile, layout, M, N, K, A, lda, B, ldb, C, ldc, flags, bias, res, ldr, aux_in, aux_out, ldaux, colsum) -> int:  # noqa: N803
    if tile in SK_TILES:
        return gemm_sk(tile, layout, M, N, K, A, lda, B, ldb, C, ldc, flags, bias, res, ldr)
    return lib().mh_gemm_bf16_tile(_I(tile), _I(layout), _I(M), _I(N), _I(K), ptr(A), _I(lda), ptr(B), _I(ldb), ptr(C),
                                   _I(ldc), _I(flags), ptr(bias), ptr(res), _I(ldr), ptr(aux_in), ptr(aux_out), _I(ldaux),
                                   ptr(colsum), stream())


FAMILY_DMA, FAMILY_PP, FAMILY_192, FAMILY_ALL = 1, 2, 4, 7   # MH_GEMM_FAMILY_*: what MH_TILE_AUTO may choose besides TILE_REG_128


def resolve_tile(tile, layout, M, N, K, lda, ldb, ldc, ldr, ldaux, flags, families=FAMILY_ALL) -> int:  # noqa: N803
    """mh_gemm_bf16_resolve_tile: the TILE_* that ``mh_gemm_bf16_tile(tile, ...)`` runs for this problem -- the library's own rule, asked
    instead of copied; nothing is launched.  -2: the explicit DMA / ping-pong ``tile`` does not serve the problem."""
    rc = lib().mh_gemm_bf16_resolve_tile(_I(tile), _I(families), _I(layout), _I(M), _I(N), _I(K), _I(lda), _I(ldb), _I(ldc), _I(ldr),
                                         _I(ldaux), _I(flags))
    if rc == -1:
        _check(rc, "mh_gemm_bf16_resolve_tile")
    return rc


def _resolve(tile, args, families=FAMILY_ALL) -> int:
    layout, M, N, K, _, lda, _, ldb, _, ldc, flags, _, _, ldr, _, _, ldaux, _ = args  # noqa: N806
    return resolve_tile(tile, layout, M, N, K, lda, ldb, ldc, ldr, ldaux, flags, families)


def _tune_gemm(key, args) -> int:
    best, best_ms = TILE_REG_128, float("inf")
    for tile in TILES:
        rc = _gemm_tile(tile, *args)
        if rc == -2:
            continue
        _check(rc, "mh_gemm_bf16_tile")
        _gemm_tile(tile, *args)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(4):
            _gemm_tile(tile, *args)
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1)
        if ms < best_ms:
            best, best_ms = tile, ms
    _tile_choice[key] = best
    return best


_shape_only = 0


@contextlib.contextmanager
def shape_only_tiles():
    """Deterministic mode: inside the block every GEMM without an explicit tile runs the library's own rule (MH_TILE_AUTO, a
    function of shapes, strides and flags) -- neither the process-wide table of tuned tiles nor the MH_GEMM_* experiment
    switches are consulted, so the kernel that runs does not depend on a measured time or on the environment."""
    global _shape_only
    _shape_only += 1
    try:
        yield
    finally:
        _shape_only -= 1


def _pick_tile(layout, M, N, K, flags, args) -> int:  # noqa: N803
    if _shape_only:
        return TILE_AUTO
    tflags = flags & ~COLSUM                 # the column-sum side output does not change the kernel's cost profile
    key = (layout, M, N, K, tflags)
    tile = _tile_choice.get(key)
    if tile is None:
        # Experiment switches are resolved HERE, on the host side: the C library reads no environment (its header promises no
        # process-global state).  MH_GEMM_TILE=<id> forces one tile; MH_GEMM_DMA=0 keeps everything on the register-staged
        # kernel, =1 sends every eligible problem to the 256x256 LDS-DMA tile; MH_DMA_STAGGER=0 picks its lockstep form.  Where a
        # switch needs the library's rule (MH_GEMM_PP=0, MH_DMA_STAGGER=0) it asks mh_gemm_bf16_resolve_tile for it.
        forced = os.environ.get("MH_GEMM_TILE")
        if forced is not None:
            t = int(forced)
            # MH_TILE_PP_128_DIAG1..5: retired ids of ablation builds of the ping-pong tile; every library declines them (-2)
            if TILE_PP_128 < t <= TILE_PP_128 + 5:
                raise HipExtensionError(f"MH_GEMM_TILE={t} is a retired id (a diagnostic build of the ping-pong tile that wrote wrong "
                                        "outputs): no library contains that kernel")
            return t
        dma = os.environ.get("MH_GEMM_DMA", "")[:1]
        if os.environ.get("MH_GEMM_PP", "")[:1] == "0" and dma == "":   # A/B: the round-2 rule (no persistent ping-pong tile)
            return _resolve(TILE_AUTO, args, FAMILY_DMA)
        if dma == "0":
            return TILE_REG_128
        lockstep = os.environ.get("MH_DMA_STAGGER", "")[:1] == "0"
        if (dma == "1" and layout != GEMM_TN and not (flags & ATOMIC)) or (
                lockstep and _resolve(TILE_AUTO, args, FAMILY_DMA) == TILE_DMA_256):
            return TILE_DMA_256_LOCKSTEP if lockstep else TILE_DMA_256
        if _tuning and not (flags & ATOMIC):   # accumulating outputs cannot be re-run for timing: the library's rule decides
            targs = list(args)
            targs[10], targs[17] = tflags, None
            tile = _tune_gemm(key, tuple(targs))
        else:
            tile = TILE_AUTO
    return tile


def gemm(layout: int, M: int, N: int, K: int, A, lda: int, B, ldb: int, C, ldc: int, flags: int = 0, bias=None,  # noqa: N803
         res=None, ldr: int = 0, aux_in=None, aux_out=None, ldaux: int = 0, colsum=None, tile: int | None = None) -> None:
    """``tile``: one of TILE_* to force a kernel (tests / micro-benchmarks); default = the tuned choice for this problem
    signature if there is one, else the library's own rule (MH_TILE_AUTO)."""
    args = (layout, M, N, K, A, lda, B, ldb, C, ldc, flags, bias, res, ldr, aux_in, aux_out, ldaux, colsum)
    explicit = tile is not None
    if _instep is not None and _instep.cand is not None and not explicit and not (flags & ATOMIC):
        key = (layout, M, N, K, flags & ~COLSUM)
        e0, e1 = _instep.open(key)
        e0.record()
        rc = _gemm_tile(_instep.cand, *args)
        if rc == -2:                   # the candidate does not serve this problem: not a contender for this signature
            _instep.reject(key)
            rc = _gemm_tile(TILE_AUTO, *args)
        _check(rc, "mh_gemm_bf16_tile")
        e1.record()
        return
    if not explicit:
        tile = _pick_tile(layout, M, N, K, flags, args)
    ev = None
    if _timer is not None:
        named = tile if tile in SK_TILES else _resolve(tile, args)   # the kernel the library will run for `tile`
        if named == -2:                # a forced tile that does not serve the problem: the launch below falls back or raises
            named = tile
        ev = _timer.record(_TILE_NAME[named].format(_LAYOUT_NAME[layout]), 2.0 * M * N * K, (M, N, K))
        ev[0].record()
    rc = _gemm_tile(tile, *args)
    if rc == -2 and not explicit:      # e.g. MH_GEMM_TILE / MH_GEMM_DMA=1 forced a DMA tile onto a problem with a K tail
        # the A/B switches that exist to keep a kernel family OUT of the run (MH_GEMM_DMA=1: everything on the DMA tile or the
        # register tile; MH_GEMM_PP=0: the round-2 dispatch) must not fall back to MH_TILE_AUTO, whose rule may pick that family
        pinned = os.environ.get("MH_GEMM_DMA", "")[:1] == "1" or os.environ.get("MH_GEMM_PP", "")[:1] == "0"
        rc = _gemm_tile(TILE_REG_128 if pinned else TILE_AUTO, *args)
    if rc == -2:
        raise HipExtensionError(f"mh_gemm_bf16_tile: problem ({M}, {N}, {K}) does not qualify for tile {tile}")
    _check(rc, "mh_gemm_bf16_tile")
    if ev is not None:
        ev[1].record()


def call(name: str, *args) -> None:
    """Generic checked call: tensors -> device pointers, ints/floats passed through as given ctypes."""
    conv = []
    for a in args:
        if a is None or isinstance(a, torch.Tensor):
            conv.append(ptr(a))
        else:
            conv.append(a)
    _check(getattr(lib(), name)(*conv, stream()), name)


def _hbm_call(kind: str, nbytes: float, name: str, *args) -> None:
    """``call`` bracketed by HIP events when a ``KernelTimer`` is active: the HBM-bound sub-stages report achieved GB/s on
    their ALGORITHMIC bytes (bench.py's ``hbm_substages``)."""
    if _timer is None:
        return call(name, *args)
    e0, e1 = _timer.record_bytes(kind, nbytes)
    e0.record()
    call(name, *args)
    e1.record()


def _flop_call(kind: str, flops: float, shape, name: str, *args) -> None:
    """``call`` bracketed by HIP events when a ``KernelTimer`` is active: an MFMA kernel's launch under its kind, algorithmic
    FLOPs and shape (bench.py's roofline leg)."""
    if _timer is None:
        return call(name, *args)
    e0, e1 = _timer.record(kind, flops, shape)
    e0.record()
    call(name, *args)
    e1.record()


def _esz(t) -> int:
    return 0 if t is None else t.element_size()


# ------------------------------------------------------------------------------------------------ typed wrappers
def layernorm_fwd(x, x_L, x_off, gamma, beta, y, y_L, y_off, mean, rstd, B, n, dim, eps=1e-5):
    _hbm_call(f"ln_fwd<{dim}>", float(B) * n * dim * (4 + _esz(y)), "mh_layernorm_fwd", x, _I(x_L), _I(x_off), gamma, beta, y, _I(y_L),
              _I(y_off), _I(1 if y.dtype == torch.float32 else 0), mean, rstd, _I(B), _I(n), _I(dim), _F(eps))


def layernorm_fwd_fp8(x, x_L, x_off, gamma, beta, y, y_L, y_off, mean, rstd, B, n, dim, y8, y8_scale, y8_amax, eps=1e-5):
    """LayerNorm forward writing the bf16 output AND its e4m3 copy (times ``y8_scale``), absmax folded into ``y8_amax``."""
    call("mh_layernorm_fwd_fp8", x, _I(x_L), _I(x_off), gamma, beta, y, _I(y_L), _I(y_off), mean, rstd, _I(B), _I(n), _I(dim),
         _F(eps), y8, y8_scale, y8_amax)


def layernorm_fwd_mx(x, x_L, x_off, gamma, beta, y, y_L, y_off, mean, rstd, B, n, dim, y8, y8_scales, ld_y8s, eps=1e-5):
    """LayerNorm forward writing the bf16 output AND its MX copy (e4m3 ``y8`` + E8M0 ``y8_scales`` [rows, dim/32], pitch ``ld_y8s``)."""
    call("mh_layernorm_fwd_mx", x, _I(x_L), _I(x_off), gamma, beta, y, _I(y_L), _I(y_off), mean, rstd, _I(B), _I(n), _I(dim),
         _F(eps), y8, y8_scales, _I(ld_y8s))


def layernorm_bwd_workspace(rows, dim) -> int:
    return int(lib().mh_layernorm_bwd_workspace(_I(rows), _I(dim)))


def layernorm_bwd(dy, dy_L, dy_off, x, x_L, x_off, gamma, mean, rstd, dres, dx, dx_bf16, dgamma, dbeta, dcol, workspace,
                  B, n, dim):
    _hbm_call(f"ln_bwd<{dim}>", float(B) * n * dim * (_esz(dy) + 4 + _esz(dres) + 4 + _esz(dx_bf16)), "mh_layernorm_bwd", dy, _I(dy_L),
              _I(dy_off), _I(1 if dy.dtype == torch.float32 else 0), x, _I(x_L), _I(x_off), gamma, mean, rstd, dres, dx, dx_bf16,
              dgamma, dbeta, dcol, workspace, _I(B), _I(n), _I(dim))


def layernorm_bwd_partial(dy, dy_L, dy_off, x, x_L, x_off, gamma, mean, rstd, dres, dx, dx_bf16, workspace, B, n, dim):
    """LayerNorm backward that leaves (dgamma | dbeta | colsum(dx)) as per-block partial rows in ``workspace`` (see ColsumBatch)."""
    _hbm_call(f"ln_bwd<{dim}>", float(B) * n * dim * (_esz(dy) + 4 + _esz(dres) + 4 + _esz(dx_bf16)), "mh_layernorm_bwd_partial", dy,
              _I(dy_L), _I(dy_off), _I(1 if dy.dtype == torch.float32 else 0), x, _I(x_L), _I(x_off), gamma, mean, rstd, dres, dx,
              dx_bf16, workspace, _I(B), _I(n), _I(dim))


COLSUM_ROWS = 16   # MH_COLSUM_ROWS in include/maestro_hip.h


class _MhColsumJob(ctypes.Structure):
    _fields_ = [("src", ctypes.c_void_p), ("dst", ctypes.c_void_p), ("rows", ctypes.c_int), ("cols", ctypes.c_int),
                ("ld", ctypes.c_int), ("reserved", ctypes.c_int)]


class ColsumBatch:
    """Descriptor table (built once: all buffers are static) for ``mh_colsum_batched``: jobs ``(src f32 [rows, ld], dst f32
    [cols], rows, cols, ld)`` -> ``dst += column sums of src``, all in one launch."""

    def __init__(self, jobs, device) -> None:
        if not jobs:
            raise HipExtensionError("ColsumBatch: no jobs")
        arr = (_MhColsumJob * len(jobs))()
        for i, (src, dst, rows, cols, ld) in enumerate(jobs):
            if src.dtype != torch.float32 or dst.dtype != torch.float32 or not src.is_cuda or not dst.is_cuda:
                raise HipExtensionError("ColsumBatch: f32 device tensors expected")
            if rows <= 0 or cols <= 0 or ld < cols or src.numel() < (rows - 1) * ld + cols or dst.numel() < cols:
                raise HipExtensionError(f"ColsumBatch job {i}: shape ({rows}, {cols}, ld {ld}) does not fit its buffers")
            arr[i] = _MhColsumJob(src.data_ptr(), dst.data_ptr(), rows, cols, ld, 0)
        self.keep = [t for job in jobs for t in job[:2]]     # the descriptors hold raw pointers
        self.table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(device)
        blocks = []                                          # one work item per workgroup: job << 48 | column block << 32 | row chunk
        for i, (_, _, rows, cols, _) in enumerate(jobs):
            if cols > 65535 * 256 or len(jobs) > 32767:
                raise HipExtensionError("ColsumBatch: too many jobs / columns for the work-item encoding")
            for cb in range(-(-cols // 256)):
                blocks += [(i << 48) | (cb << 32) | rc for rc in range(-(-rows // COLSUM_ROWS))]
        self.blocks = torch.tensor(blocks, dtype=torch.int64).to(device)
        self.n, self.n_blocks = len(jobs), len(blocks)

    def launch(self) -> None:
        call("mh_colsum_batched", self.table, _I(self.n), self.blocks, _I(self.n_blocks))


# ---- deterministic mode (include/maestro_hip.h): atomic-free first phases + the ordered reduction that finishes them
ORDERED_ROWS, ORDERED_ADD = 16, 1     # MH_ORDERED_ROWS, MH_ORDERED_ADD
COLSUM_PARTIAL_ROWS = 256             # MH_COLSUM_PARTIAL_ROWS


class _MhOrderedJob(ctypes.Structure):
    _fields_ = [("src", ctypes.c_void_p), ("dst", ctypes.c_void_p), ("rows", ctypes.c_int), ("cols", ctypes.c_int),
                ("ld", ctypes.c_int), ("flags", ctypes.c_int)]


class OrderedReduce:
    """Descriptor table (built once: all buffers are static) for ``mh_reduce_ordered``: jobs ``(src f32 [rows, ld], dst f32 [cols],
    rows, cols, ld[, add])`` -> ``dst = (add ? dst : 0) + ordered column sums of src`` in one launch, without atomics.  Jobs that
    share a ``dst`` form a chain: the table lists chains in the order of their first job and keeps the caller's order inside a
    chain, which is the order in which their totals are added.  ``add`` must agree inside a chain."""

    def __init__(self, jobs, device) -> None:
        if not jobs:
            raise HipExtensionError("OrderedReduce: no jobs")
        chains: dict = {}
        for i, job in enumerate(jobs):
            if len(job) not in (5, 6):
                raise HipExtensionError(f"OrderedReduce job {i}: (src, dst, rows, cols, ld[, add]) expected")
            src, dst, rows, cols, ld = job[:5]
            add = bool(job[5]) if len(job) == 6 else False
            if not (isinstance(src, torch.Tensor) and isinstance(dst, torch.Tensor)) or src.dtype != torch.float32 \
                    or dst.dtype != torch.float32 or not src.is_cuda or not dst.is_cuda:
                raise HipExtensionError(f"OrderedReduce job {i}: f32 device tensors expected")
            if rows <= 0 or cols <= 0 or ld < cols or src.numel() < (rows - 1) * ld + cols or dst.numel() < cols:
                raise HipExtensionError(f"OrderedReduce job {i}: shape ({rows}, {cols}, ld {ld}) does not fit its buffers")
            chain = chains.setdefault(dst.data_ptr(), [])
            if chain and (chain[0][3] != cols or chain[0][5] != add):
                raise HipExtensionError(f"OrderedReduce job {i}: cols / add differ from the other jobs of its destination")
            chain.append((src, dst, rows, cols, ld, add))
        spans = sorted((c[0][1].data_ptr(), c[0][1].data_ptr() + 4 * c[0][3]) for c in chains.values())
        if any(a[1] > b[0] for a, b in zip(spans, spans[1:])):
            raise HipExtensionError("OrderedReduce: two destinations overlap without being the same")
        flat = [j for chain in chains.values() for j in chain]
        arr = (_MhOrderedJob * len(flat))()
        blocks, i = [], 0
        for chain in chains.values():
            blocks += [(i << 32) | cb for cb in range(-(-chain[0][3] // 256))]
            for src, dst, rows, cols, ld, add in chain:
                arr[i] = _MhOrderedJob(src.data_ptr(), dst.data_ptr(), rows, cols, ld, ORDERED_ADD if add else 0)
                i += 1
        self.keep = [t for j in flat for t in j[:2]]         # the descriptors hold raw pointers
        self.host = arr
        self.table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(device)
        self.blocks = torch.tensor(blocks, dtype=torch.int64).to(device)
        self.n, self.n_blocks, self.n_chains = len(flat), len(blocks), len(chains)
        self.nbytes = 4.0 * (sum(j[2] * j[3] for j in flat) + sum(c[0][3] for c in chains.values()))     # algorithmic: partial rows read, outputs written

    def launch(self) -> None:
        ev = _timer.record_bytes("reduce_ordered", self.nbytes) if _timer is not None else None
        if ev is not None:
            ev[0].record()
        _check(lib().mh_reduce_ordered(ctypes.byref(self.host), ptr(self.table), _I(self.n), ptr(self.blocks), _I(self.n_blocks),
                                       stream()), "mh_reduce_ordered")
        if ev is not None:
            ev[1].record()


# ---- device-side mask draws
MASK_MAX_L, MASK_MAX_STREAMS = 8192, 4096     # MH_MASK_MAX_L, MH_MASK_MAX_STREAMS


class _MhMaskSeg(ctypes.Structure):
    _fields_ = [("tok_off", ctypes.c_int), ("D", ctypes.c_int), ("L", ctypes.c_int), ("gi", ctypes.c_int), ("G", ctypes.c_int),
                ("stream", ctypes.c_int), ("p_mod", ctypes.c_float), ("p_bands", ctypes.c_float), ("p_dates", ctypes.c_float),
                ("p_loc", ctypes.c_float)]


class _MhMaskJob(ctypes.Structure):
    _fields_ = [("noise", ctypes.c_void_p), ("strct", ctypes.c_void_p), ("Beff", ctypes.c_int), ("L", ctypes.c_int),
                ("noise_stream", ctypes.c_int), ("noise_rpb", ctypes.c_int), ("struct_rpb", ctypes.c_int),
                ("row_div", ctypes.c_int), ("row_mul", ctypes.c_int), ("row_add", ctypes.c_int), ("seg0", ctypes.c_int),
                ("n_segs", ctypes.c_int)]


class MaskDraw:
    """Descriptor tables (built once: the mask buffers are static) for ``mh_mask_draw``: all groups' structural masks and noise
    of a step in one launch.  ``jobs``: the dicts of ``layers.utils.mask_draw_jobs``; ``bufs``: ``{group: (noise f32 [Beff, L],
    struct u8 [Beff, L])}``, dense device tensors.  ``launch(seed, step, row_base)``: by-value, nothing of a step is in the tables."""

    def __init__(self, jobs, bufs, device) -> None:
        if not jobs:
            raise HipExtensionError("MaskDraw: no jobs")
        n_segs = sum(len(j["segs"]) for j in jobs)
        jarr, sarr, k = (_MhMaskJob * len(jobs))(), (_MhMaskSeg * max(n_segs, 1))(), 0
        self.keep = []
        for i, j in enumerate(jobs):
            noise, struct = bufs[j["name"]]
            shape = (j["Beff"], j["L"])
            if not (isinstance(noise, torch.Tensor) and isinstance(struct, torch.Tensor)) or noise.dtype != torch.float32 \
                    or struct.dtype != torch.uint8 or not noise.is_cuda or not struct.is_cuda:
                raise HipExtensionError(f"MaskDraw job {i}: noise f32 and struct u8 device tensors expected")
            if tuple(noise.shape) != shape or tuple(struct.shape) != shape or not noise.is_contiguous() or not struct.is_contiguous():
                raise HipExtensionError(f"MaskDraw job {i}: dense [{shape[0]}, {shape[1]}] buffers expected")
            if not 1 <= j["L"] <= MASK_MAX_L:
                raise HipExtensionError(f"MaskDraw job {i}: L {j['L']} (1 ... {MASK_MAX_L})")
            jarr[i] = _MhMaskJob(noise.data_ptr(), struct.data_ptr(), j["Beff"], j["L"], j["noise_stream"], j["noise_rpb"],
                                 j["struct_rpb"], j["row_div"], j["row_mul"], j["row_add"], k, len(j["segs"]))
            for s in j["segs"]:
                sarr[k] = _MhMaskSeg(s["tok_off"], s["D"], s["L"], s["gi"], s["G"], s["stream"], *s["p"])
                k += 1
            self.keep += [noise, struct]                     # the descriptors hold raw pointers
        self.jobs_host, self.segs_host = jarr, sarr
        self.jobs = torch.frombuffer(bytearray(bytes(jarr)), dtype=torch.uint8).to(device)
        self.segs = torch.frombuffer(bytearray(bytes(sarr)), dtype=torch.uint8).to(device)
        self.n, self.n_segs = len(jobs), n_segs
        self.nbytes = 5.0 * sum(j["Beff"] * j["L"] for j in jobs)      # algorithmic: f32 noise + u8 struct written

    def launch(self, seed: int, step: int, row_base: int = 0) -> None:
        if not 0 <= int(seed) < 1 << 64:
            raise HipExtensionError(f"MaskDraw: seed {seed} is not an unsigned 64-bit value")
        if not -(1 << 63) <= int(step) < 1 << 63 or not -(1 << 63) <= int(row_base) < 1 << 63:
            raise HipExtensionError(f"MaskDraw: step {step} / row_base {row_base} out of range")
        _check(lib().mh_mask_draw(ctypes.byref(self.jobs_host), ptr(self.jobs), _I(self.n), ctypes.byref(self.segs_host),
                                  ptr(self.segs), _I(self.n_segs), ctypes.c_uint64(int(seed)), ctypes.c_longlong(int(step)),
                                  ctypes.c_longlong(int(row_base)), stream()), "mh_mask_draw")


def mask_draw_reference(groups, mods, B, seed, step, row_base=0):  # noqa: N803
    """What ``MaskDraw.launch(seed, step, row_base)`` writes, computed in numpy on the host: ``(noise, struct)`` dicts shaped like
    ``MAEEngine.draw_masks()`` (the restatement lives next to the host drawer, ``layers.utils.mask_draw_reference``)."""
    from maestro_amd.layers.utils import mask_draw_reference as reference
    return reference(groups, mods, B, seed, step, row_base)


# ---- gradient guard
GUARD_CHUNK = 16384     # MH_GUARD_CHUNK


class _MhGuardState(ctypes.Structure):
    _fields_ = [("norm", ctypes.c_float), ("coef", ctypes.c_float), ("finite", ctypes.c_int), ("bad", ctypes.c_uint),
                ("t", ctypes.c_longlong), ("skipped", ctypes.c_longlong)]


def grad_sumsq_partial_rows(n) -> int:
    return int(lib().mh_grad_sumsq_partial_rows(_L(n)))


def grad_sumsq_partial(g, n, partial, bad):
    """First phase of the guard: ``partial[i]`` = sum of squares, ``bad[i]`` = inf / NaN count of chunk ``i`` of ``g[:n]`` (f32,
    16-byte aligned, ``n % 4 == 0``); ``partial`` f32 / ``bad`` int32 of ``grad_sumsq_partial_rows(n)`` rows, plain stores."""
    _hbm_call("grad_sumsq", 4.0 * n, "mh_grad_sumsq_partial", g, _L(n), partial, bad)


def grad_guard_finish(partial, bad, rows, grad_scale, max_norm, skip_nonfinite, lr, b1, b2, hyper, state):
    """Second phase: the partials -> ``hyper`` (the five device scalars of ``adamw_dev``) and the 32-byte ``MhGuardState``."""
    call("mh_grad_guard_finish", partial, bad, _L(rows), _F(grad_scale), _F(max_norm), _I(1 if skip_nonfinite else 0), _F(lr), _F(b1),
         _F(b2), hyper, state)


class GradGuard:
    """Device-side global gradient norm, clipping coefficient and non-finite skip over a flat f32 gradient of ``n`` elements
    (include/maestro_hip.h).  Owns the partial rows, the five scalars ``hyper`` that ``adamw_dev`` reads and the device
    ``MhGuardState`` (Adam's step count ``t`` lives THERE: a skipped step does not advance it).  ``launch`` issues the two
    kernels; ``norm`` / ``coef`` / ``hyper`` are device views, nothing on the step path reads them on the host.  ``max_norm``
    None or <= 0: no clipping.  No atomics and one fixed order of additions: the same gradient gives the same bits."""

    def __init__(self, n: int, device, max_norm: float | None = None, skip_nonfinite: bool = True) -> None:
        n = int(n)
        if n <= 0 or n % 4:
            raise HipExtensionError(f"GradGuard: n {n} must be positive and a multiple of 4")
        if torch.device(device).type != "cuda":
            raise HipExtensionError("GradGuard needs a GPU (no CPU fallback)")
        self.n, self.max_norm, self.skip_nonfinite = n, float(max_norm or 0.0), bool(skip_nonfinite)
        self.rows = grad_sumsq_partial_rows(n)
        self.partial = torch.zeros(self.rows, dtype=torch.float32, device=device)
        self.bad = torch.zeros(self.rows, dtype=torch.int32, device=device)
        self.hyper = torch.zeros(5, dtype=torch.float32, device=device)
        self.state = torch.zeros(ctypes.sizeof(_MhGuardState), dtype=torch.uint8, device=device)
        self.norm = self.state[0:4].view(torch.float32)
        self.coef = self.state[4:8].view(torch.float32)
        self._counters = self.state[16:32].view(torch.int64)      # t, skipped
        self.t_dev = self._counters[:1]      # Adam's t as a device word: what ``adamw_bf16m_dev`` reads after ``launch``

    def launch(self, grad, lr: float, b1: float, b2: float, grad_scale: float = 1.0) -> None:
        if grad.dtype != torch.float32 or grad.numel() != self.n or not grad.is_contiguous():
            raise HipExtensionError(f"GradGuard.launch: a dense f32 gradient of {self.n} elements expected")
        grad_sumsq_partial(grad, self.n, self.partial, self.bad)
        grad_guard_finish(self.partial, self.bad, self.rows, grad_scale, self.max_norm, self.skip_nonfinite, lr, b1, b2,
                          self.hyper, self.state)

    def stats(self) -> dict:
        """ONE host read (synchronises): the state of the last launch."""
        s = _MhGuardState.from_buffer_copy(bytes(self.state.cpu().numpy()))
        return {"norm": float(s.norm), "coef": float(s.coef), "finite": bool(s.finite), "bad": int(s.bad), "t": int(s.t),
                "skipped": int(s.skipped)}

    def state_dict(self) -> dict:
        t, skipped = self._counters.tolist()
        return {"t": int(t), "skipped": int(skipped)}

    def load_state_dict(self, sd: dict) -> None:
        """``t`` and, when given, ``skipped`` (otherwise the count stays)."""
        skipped = int(sd["skipped"]) if "skipped" in sd else int(self._counters[1])
        self._counters.copy_(torch.tensor([int(sd["t"]), skipped], dtype=torch.int64))


def grad_guard_reference(g, grad_scale, max_norm, skip_nonfinite, lr, b1, b2, t, skipped):
    """The contract of ``mh_grad_sumsq_partial`` + ``mh_grad_guard_finish`` restated in numpy / fp64 (runs on any machine; the
    tests compare the kernels against it).  ``g``: the flat gradient (array or CPU tensor); ``t`` / ``skipped``: the state's
    counters before the call.  Returns ``partial`` (fp64, per chunk, exact up to fp64), ``bad_rows``, ``S`` (the sum of the
    partials AS f32 rows: a chunk whose sum overflows fp32 is inf, as on the device), ``norm`` / ``coef`` (float32), ``bad``,
    ``finite``, ``apply``, ``t`` / ``skipped`` after the call and ``hyper`` (float32[5])."""
    import numpy as np
    g = g.detach().cpu().numpy() if isinstance(g, torch.Tensor) else np.asarray(g)
    g = g.astype(np.float32).ravel()
    f32, f64 = np.float32, np.float64
    rows = -(-g.size // GUARD_CHUNK)
    pad = np.zeros(rows * GUARD_CHUNK, dtype=f64)
    with np.errstate(all="ignore"):
        pad[: g.size] = g.astype(f64) ** 2
        partial = pad.reshape(rows, GUARD_CHUNK).sum(axis=1)
        bad_rows = np.zeros(rows * GUARD_CHUNK, dtype=np.int64)
        bad_rows[: g.size] = ~np.isfinite(g)
        bad_rows = bad_rows.reshape(rows, GUARD_CHUNK).sum(axis=1)
        S = partial.astype(f32).astype(f64).sum()  # noqa: N806
        norm = f32(abs(f64(f32(grad_scale))) * np.sqrt(S))
        bad = int(min(int(bad_rows.sum()), 0xFFFFFFFF))
        finite = bool(np.isfinite(norm)) and bad == 0
        max_norm = f32(max_norm or 0.0)
        coef = min(f32(1.0), f32(max_norm / f32(norm + f32(1e-6)))) if (max_norm > 0 and finite) else f32(1.0)
    apply = finite or not skip_nonfinite
    t, skipped = (int(t) + 1, int(skipped)) if apply else (int(t), int(skipped) + 1)
    hyper = np.array([f32(lr), f32(1.0 - f64(f32(b1)) ** t), f32(np.sqrt(1.0 - f64(f32(b2)) ** t)), f32(grad_scale) * f32(coef),
                      1.0 if apply else 0.0], dtype=f32)
    return {"partial": partial, "bad_rows": bad_rows, "S": S, "norm": norm, "coef": f32(coef), "bad": bad, "finite": finite,
            "apply": apply, "t": t, "skipped": skipped, "hyper": hyper}


def colsum_partial_rows(M) -> int:  # noqa: N803
    return int(lib().mh_colsum_partial_rows(_I(M)))


def colsum_partial(x, partial, M, N, ld):  # noqa: N803
    """Per-row-block column sums of ``x`` (bf16 / f32 [M, ld]) into ``partial`` f32 [colsum_partial_rows(M), N], plain stores."""
    call("mh_colsum_partial", x, _I(1 if x.dtype == torch.float32 else 0), partial, _I(M), _I(N), _I(ld))


def masked_loss_partial_size(B, Lm) -> int:  # noqa: N803
    return int(lib().mh_masked_loss_partial_size(_I(B), _I(Lm)))


def masked_loss_det(rec, target, mask_group, n_masked, weight, loss_partial, drec, B, Lm, Lgroup, tok_off, PPC, p):  # noqa: N803
    """``masked_loss`` whose workgroups store their partial losses to ``loss_partial`` [masked_loss_partial_size(B, Lm)]."""
    _hbm_call("masked_loss", float(B) * Lm * (PPC * (_esz(rec) + 4 + _esz(drec)) + 1), "mh_masked_loss_det", rec, target, mask_group,
              n_masked, _F(weight), loss_partial, drec, _I(B), _I(Lm), _I(Lgroup), _I(tok_off), _I(PPC), _I(p))


def masked_loss_bands_det(rec, target, mask_group, n_elems, weight, loss_partial, drec, B, Lm, Lgroup, tok_off, PPC, p, tgt_C,  # noqa: N803
                          tgt_c0, n_g):
    call("mh_masked_loss_bands_det", rec, target, mask_group, n_elems, _F(weight), loss_partial, drec, _I(B), _I(Lm), _I(Lgroup),
         _I(tok_off), _I(PPC), _I(p), _I(tgt_C), _I(tgt_c0), _I(n_g))


def unmask_token_grad_partial_rows(n_rows) -> int:
    return int(lib().mh_unmask_token_grad_partial_rows(_L(n_rows)))


def unmask_token_grad_det(dxdec, mask, tok_slot, partial, B, L, Dd, slot, t_lo, t_hi):  # noqa: N803
    """``unmask_token_grad`` into per-workgroup rows ``partial`` [unmask_token_grad_partial_rows(B * (t_hi - t_lo)), Dd]."""
    call("mh_unmask_token_grad_det", dxdec, mask, tok_slot, partial, _I(B), _I(L), _I(Dd), _I(slot), _I(t_lo), _I(t_hi))


def unmask_token_grad_per_sample_det(dxdec, mask, tok_slot_bl, partial, B, L, Dd, slot):  # noqa: N803
    """``unmask_token_grad_per_sample`` into per-workgroup rows ``partial`` [unmask_token_grad_partial_rows(B * L), Dd]."""
    call("mh_unmask_token_grad_per_sample_det", dxdec, mask, tok_slot_bl, partial, _I(B), _I(L), _I(Dd), _I(slot))


def embed_bwd_partial_rows(BD, L) -> int:  # noqa: N803
    return int(lib().mh_embed_bwd_partial_rows(_I(BD), _I(L)))


def embed_finish_bwd_det(dxg, y, stats, gamma, dyc, param_partial, blk_sums, sums, B, D, L, E, tok_off, Lgroup):  # noqa: N803
    """``embed_finish_bwd`` without atomics: ``param_partial`` [embed_bwd_partial_rows(B * D, L), 2 E] keeps the dgamma | dbeta rows
    for an ``OrderedReduce``, ``blk_sums`` [embed_bwd_partial_rows(B * D, L), 2] is scratch of the call."""
    call("mh_embed_finish_bwd_det", dxg, y, stats, gamma, dyc, param_partial, blk_sums, sums, _I(B), _I(D), _I(L), _I(E),
         _I(tok_off), _I(Lgroup))


# ---- step ends (include/maestro_hip.h): producers that leave their bias gradient as partial rows for a ColsumBatch job
def masked_loss_cs_rows(B, Lm) -> int:  # noqa: N803
    return int(lib().mh_masked_loss_cs_rows(_I(B), _I(Lm)))


def masked_loss_cs(rec, target, mask_group, n_masked, weight, acc, drec, cs_partial, B, Lm, Lgroup, tok_off, PPC, p):  # noqa: N803
    """``masked_loss`` that also stores the per-workgroup column sums of ``drec`` to ``cs_partial`` [masked_loss_cs_rows(B, Lm), PPC]."""
    _hbm_call("masked_loss", float(B) * Lm * (PPC * (_esz(rec) + 4 + _esz(drec)) + 1), "mh_masked_loss_cs", rec, target, mask_group,
              n_masked, _F(weight), acc, drec, cs_partial, _I(B), _I(Lm), _I(Lgroup), _I(tok_off), _I(PPC), _I(p))


def masked_loss_bands_cs(rec, target, mask_group, n_elems, weight, acc, drec, cs_partial, B, Lm, Lgroup, tok_off, PPC, p, tgt_C,  # noqa: N803
                         tgt_c0, n_g):
    call("mh_masked_loss_bands_cs", rec, target, mask_group, n_elems, _F(weight), acc, drec, cs_partial, _I(B), _I(Lm), _I(Lgroup),
         _I(tok_off), _I(PPC), _I(p), _I(tgt_C), _I(tgt_c0), _I(n_g))


def gather_rows_cs_rows(rows) -> int:
    return int(lib().mh_gather_rows_cs_rows(_L(rows)))


def gather_rows_bf16_cs(src, idx, dst16, cs_partial, B, src_L, n_idx, dim):  # noqa: N803
    """``gather_rows`` + ``cast_bf16`` in one pass (no f32 intermediate) + the per-workgroup column sums of ``dst16`` to ``cs_partial``
    [gather_rows_cs_rows(B * n_idx), dim]."""
    call("mh_gather_rows_bf16_cs", src, idx, dst16, cs_partial, _I(B), _I(src_L), _I(n_idx), _I(dim))


def embed_bwd_cs_rows(rows) -> int:
    return int(lib().mh_embed_bwd_cs_rows(_L(rows)))


def embed_finish_bwd_ends(dx, inv, n_vis, y, stats, gamma, dyc, dgamma, dbeta, sums, cs_partial, B, D, L, E, tok_off, Lgroup):  # noqa: N803
    """``embed_finish_bwd`` reading the gradient of the visible rows ``dx`` [B, n_vis, E] through the position map ``inv`` [B, Lgroup]
    (``inv`` None: ``dx`` is the dense [B, Lgroup, E] gradient) + the per-workgroup column sums of ``dyc`` to ``cs_partial``
    [embed_bwd_cs_rows(B * D * L), E]."""
    call("mh_embed_finish_bwd_ends", dx, inv, _I(n_vis), y, stats, gamma, dyc, dgamma, dbeta, sums, cs_partial, _I(B), _I(D), _I(L),
         _I(E), _I(tok_off), _I(Lgroup))


def det_slices(K: int) -> int:  # noqa: N803
    """Number of K-slices of a weight-gradient GEMM outside the transformer stacks in deterministic mode: a function of the
    shape alone (one slice per 1024 rows of K, at most 8)."""
    return max(1, min(8, K // 1024))


def gemm_tn_slabs(M, N, K, A, lda, B, ldb, slabs):  # noqa: N803
    """dW[M, N] = A[K, M]^T B[K, N] as ``det_slices(K)`` plain-store TN GEMMs on consecutive K-slices, slice i into the private
    fp32 slab ``slabs[i]`` ([M, N] dense); an ``OrderedReduce`` job (rows = slices, cols = M N, ld = M N) sums them."""
    S = slabs.shape[0]  # noqa: N806
    step = -(-(-(-K // S)) // 64) * 64
    for i in range(S):
        k0 = i * step
        kn = min(K, k0 + step) - k0
        if kn <= 0:                      # (cannot happen for det_slices: K // S >= 1024 > 64)
            raise HipExtensionError(f"gemm_tn_slabs: empty K-slice {i} of {S} (K = {K})")
        gemm(GEMM_TN, M, N, kn, A[k0:], lda, B[k0:], ldb, slabs[i], N, OUT_F32)


def attn_fwd(qkv, out, lse, B, N, H, D, scale):
    _flop_call("attn_fwd", 4.0 * B * H * N * N * D, (B, N, H, D), "mh_attn_fwd", qkv, out, lse, _I(B), _I(N), _I(H), _I(D), _F(scale))


def attn_bwd(qkv, out, dout, lse, delta, dqkv, B, N, H, D, scale):
    # algorithmic 5 matmuls (the two-kernel form recomputes 2 more)
    _flop_call("attn_bwd", 10.0 * B * H * N * N * D, (B, N, H, D), "mh_attn_bwd", qkv, out, dout, lse, delta, dqkv, _I(B), _I(N), _I(H),
               _I(D), _F(scale))


def patchify(img, cols, target, BD, Ctot, S, P, Kpad, norm_bands, n_groups, normalise, rescale_elev):
    # 4 B read per pixel + the bf16 GEMM columns (K padded to Kpad) + the fp32 loss target
    nb = float(BD) * S * S * Ctot * 4 + float(BD) * (S // P) ** 2 * (Kpad * 2 * (cols is not None) + Ctot * P * P * 4 * (target is not None))
    _hbm_call("patchify", nb, "mh_patchify", img, cols, target, _I(BD), _I(Ctot), _I(S), _I(P), _I(Kpad), norm_bands, _I(n_groups),
              _I(int(normalise)), _I(int(rescale_elev)))


def patchify_bands(img, cols, target, BD, Csrc, c0, Ctot, S, P, Kpad, norm_bands, n_groups, normalise, rescale_elev):
    """``patchify`` of channels ``c0 .. c0 + Ctot - 1`` of an image with ``Csrc`` channels (one band-group); ``cols`` or
    ``target`` may be None."""
    call("mh_patchify_bands", img, cols, target, _I(BD), _I(Csrc), _I(c0), _I(Ctot), _I(S), _I(P), _I(Kpad), norm_bands,
         _I(n_groups), _I(int(normalise)), _I(int(rescale_elev)))


def groupnorm_partial_size(BD, L, E) -> int:
    return int(lib().mh_groupnorm_partial_size(_I(BD), _I(L), _I(E)))


def groupnorm_stats(y, partial, stats, BD, L, E, eps=1e-5):
    call("mh_groupnorm_stats", y, partial, stats, _I(BD), _I(L), _I(E), _F(eps))


def embed_finish(y, stats, gamma, beta, pos, date, date_rows, date_off, xg, B, D, L, E, tok_off, Lgroup):
    call("mh_embed_finish", y, stats, gamma, beta, pos, date, _I(date_rows), _I(date_off), xg, _I(B), _I(D), _I(L), _I(E),
         _I(tok_off), _I(Lgroup))


def date_features(dates, ref_date, out, B, D, rows, row_off, fac):
    call("mh_date_features", dates, ref_date, out, _I(B), _I(D), _I(rows), _I(row_off), _F(fac))


def resize(src, dst, planes, Hin, Win, Hout, Wout, mode):
    call("mh_resize", src, dst, _L(planes), _I(Hin), _I(Win), _I(Hout), _I(Wout), _I(mode))


def rescale_elev(img, out, BD, C, S):
    call("mh_rescale_elev", img, out, _I(BD), _I(C), _I(S))


def embed_finish_bwd(dxg, y, stats, gamma, dyc, dgamma, dbeta, sums, B, D, L, E, tok_off, Lgroup):
    call("mh_embed_finish_bwd", dxg, y, stats, gamma, dyc, dgamma, dbeta, sums, _I(B), _I(D), _I(L), _I(E), _I(tok_off),
         _I(Lgroup))


def depatchify(patches, img, BD, C, S, P):
    call("mh_depatchify", patches, img, _I(BD), _I(C), _I(S), _I(P))


def mask_select(noise, struct_mask, visible_idx, masked_idx, inv, mask, B, L, k):
    call("mh_mask_select", noise, struct_mask, visible_idx, masked_idx, inv, mask, _I(B), _I(L), _I(k))


def gather_rows(src, idx, dst, B, src_L, n_idx, dim, dst_L, dst_off):
    call("mh_gather_rows", src, idx, dst, _I(B), _I(src_L), _I(n_idx), _I(dim), _I(dst_L), _I(dst_off))


def scatter_rows(ddst, idx, dsrc, B, src_L, n_idx, dim, dst_L, dst_off):
    call("mh_scatter_rows", ddst, idx, dsrc, _I(B), _I(src_L), _I(n_idx), _I(dim), _I(dst_L), _I(dst_off))


def expand_rows(src, inv, dst, B, L, n, dim):
    call("mh_expand_rows", src, inv, dst, _I(B), _I(L), _I(n), _I(dim))


def unmask_assemble(y, inv, mask_token, tok_slot, pos, date, date_row, n_date_rows, xdec, B, L, n_vis, Dd):
    call("mh_unmask_assemble", y, inv, mask_token, tok_slot, pos, date, date_row, _I(n_date_rows), xdec, _I(B), _I(L),
         _I(n_vis), _I(Dd))


def unmask_token_grad(dxdec, mask, tok_slot, dmask_token, B, L, Dd, slot, t_lo, t_hi):
    call("mh_unmask_token_grad", dxdec, mask, tok_slot, dmask_token, _I(B), _I(L), _I(Dd), _I(slot), _I(t_lo), _I(t_hi))


def unmask_assemble_per_sample(y, inv, mask_token, tok_slot_bl, pos, date, date_row, n_date_rows, xdec, B, L, n_vis, Dd):
    call("mh_unmask_assemble_per_sample", y, inv, mask_token, tok_slot_bl, pos, date, date_row, _I(n_date_rows), xdec, _I(B), _I(L),
         _I(n_vis), _I(Dd))


def unmask_token_grad_per_sample(dxdec, mask, tok_slot_bl, dmask_token, B, L, Dd, slot):
    call("mh_unmask_token_grad_per_sample", dxdec, mask, tok_slot_bl, dmask_token, _I(B), _I(L), _I(Dd), _I(slot))


def count_masked(mask, B, L, t_lo, t_hi, out):
    call("mh_count_masked", mask, _I(B), _I(L), _I(t_lo), _I(t_hi), out)


def count_masked_elems(mask, B, L, t_lo, t_hi, out, mult, accumulate):
    call("mh_count_masked_elems", mask, _I(B), _I(L), _I(t_lo), _I(t_hi), out, _I(mult), _I(int(accumulate)))


def masked_loss_bands(rec, target, mask_group, n_elems, weight, acc, drec, B, Lm, Lgroup, tok_off, PPC, p, tgt_C, tgt_c0, n_g):  # noqa: N803
    call("mh_masked_loss_bands", rec, target, mask_group, n_elems, _F(weight), acc, drec, _I(B), _I(Lm), _I(Lgroup),
         _I(tok_off), _I(PPC), _I(p), _I(tgt_C), _I(tgt_c0), _I(n_g))


def masked_loss(rec, target, mask_group, n_masked, weight, acc, drec, B, Lm, Lgroup, tok_off, PPC, p):
    # per element: reconstruction (bf16) + target (f32) read, d loss / d rec (bf16) written; + one mask byte per token
    _hbm_call("masked_loss", float(B) * Lm * (PPC * (_esz(rec) + 4 + _esz(drec)) + 1), "mh_masked_loss", rec, target, mask_group,
              n_masked, _F(weight), acc, drec, _I(B), _I(Lm), _I(Lgroup), _I(tok_off), _I(PPC), _I(p))


def dihedral(x, out, flags):
    """Per-sample flips / transpose of square rasters ``x [B, ..., S, S]`` into ``out`` (same shape); ``flags`` uint8 [B]."""
    if x.shape != out.shape or x.dtype != out.dtype or x.shape[-1] != x.shape[-2] or not x.is_contiguous():
        raise HipExtensionError("dihedral: contiguous square rasters of equal shape and dtype expected")
    B, S = x.shape[0], x.shape[-1]  # noqa: N806
    planes = x.numel() // (B * S * S)
    call("mh_dihedral", x, out, flags, _I(B), _L(planes), _I(S), _I(x.element_size()))


# ---- input staging: median-date selection (csrc/staging.hip, include/maestro_hip.h)
RAW_U8, RAW_I16, RAW_U16, RAW_F32 = 0, 1, 2, 3
SELECT_MAX_WINDOW = 64
_RAW_CODE = {torch.uint8: RAW_U8, torch.int16: RAW_I16, torch.uint16: RAW_U16, torch.float32: RAW_F32}


def select_dates(raw, dates, t_start, t_win, num_dates, *, mask=None, mask_floor=0, scores=None, log_scale=False, norm_fac=None,
                 t_start_dev=None, t_win_dev=None, out=None, out_dates=None, out_index=None):
    """Median-date selection of one modality of one batch (``maestro/dataset/dataset.py:188-220``).

    ``raw`` ``[B, Tmax, C, S, S]`` uint8 / int16 / uint16 (passed through as its bytes) / float32, ``dates`` int16 ``[B, Tmax, 3]``,
    optional ``mask`` uint8 ``[B, Tmax, Cm, S, S]`` and ``scores`` float64 ``[B, Tmax]``: device tensors.  ``t_start`` / ``t_win``
    are the HOST copies (CPU tensors or sequences) of the per-sample window plan: they are validated here, before anything is
    launched, because the kernel trusts them; ``t_start_dev`` / ``t_win_dev`` are their int32 device copies (uploaded when None).
    Returns ``(out [B, nd, C, S, S] f32, out_dates [B, nd, 3] i16, out_index [B, nd] i32)``."""
    code = _RAW_CODE.get(raw.dtype)
    if code is None:
        raise HipExtensionError(f"select_dates: raw dtype {raw.dtype} (uint8, int16, uint16 or float32)")
    if raw.dim() != 5 or raw.shape[-1] != raw.shape[-2] or not raw.is_contiguous():
        raise HipExtensionError("select_dates: a contiguous [B, Tmax, C, S, S] raster expected")
    B, Tmax, C, S, _ = raw.shape  # noqa: N806
    nd = int(num_dates)
    ts = torch.as_tensor(t_start).to("cpu", torch.int64).reshape(-1)
    tw = torch.as_tensor(t_win).to("cpu", torch.int64).reshape(-1)
    if ts.numel() != B or tw.numel() != B or nd < 1 or B < 1 or C * S * S < 1:
        raise HipExtensionError(f"select_dates: t_start / t_win must hold one value per sample (B = {B}), num_dates >= 1")
    if int(tw.min()) < 1 or int(tw.max()) > SELECT_MAX_WINDOW:
        raise HipExtensionError(f"select_dates: windows of {int(tw.min())} ... {int(tw.max())} dates (1 ... {SELECT_MAX_WINDOW} are supported)")
    if int(ts.min()) < 0 or int((ts + nd * tw).max()) > Tmax:
        raise HipExtensionError(f"select_dates: a sample's {nd} windows reach outside its {Tmax} padded dates")
    if dates.dtype != torch.int16 or tuple(dates.shape) != (B, Tmax, 3) or not dates.is_contiguous():
        raise HipExtensionError(f"select_dates: dates must be a contiguous int16 [{B}, {Tmax}, 3] tensor")
    Cm = 0  # noqa: N806
    if mask is not None:
        if mask.dtype != torch.uint8 or mask.dim() != 5 or tuple(mask.shape[:2]) + tuple(mask.shape[3:]) != (B, Tmax, S, S) \
                or mask.shape[2] < 1 or not mask.is_contiguous():
            raise HipExtensionError(f"select_dates: mask must be a contiguous uint8 [{B}, {Tmax}, Cm, {S}, {S}] tensor")
        Cm = mask.shape[2]  # noqa: N806
    if scores is not None and (scores.dtype != torch.float64 or tuple(scores.shape) != (B, Tmax) or not scores.is_contiguous()):
        raise HipExtensionError(f"select_dates: scores must be a contiguous float64 [{B}, {Tmax}] tensor")
    if norm_fac is not None and not float(norm_fac) > 0.0:
        raise HipExtensionError(f"select_dates: norm_fac {norm_fac} (a positive number, or None for no division)")
    dev = raw.device
    if t_start_dev is None:
        t_start_dev = ts.to(torch.int32).to(dev)
    if t_win_dev is None:
        t_win_dev = tw.to(torch.int32).to(dev)
    for name, t in (("t_start_dev", t_start_dev), ("t_win_dev", t_win_dev)):
        if t.dtype != torch.int32 or t.numel() != B or not t.is_contiguous():
            raise HipExtensionError(f"select_dates: {name} must be a contiguous int32 [{B}] tensor")
    if out is None:
        out = torch.empty((B, nd, C, S, S), dtype=torch.float32, device=dev)
    if out_dates is None:
        out_dates = torch.empty((B, nd, 3), dtype=torch.int16, device=dev)
    if out_index is None:
        out_index = torch.empty((B, nd), dtype=torch.int32, device=dev)
    for name, t, shape, dt in (("out", out, (B, nd, C, S, S), torch.float32), ("out_dates", out_dates, (B, nd, 3), torch.int16),
                               ("out_index", out_index, (B, nd), torch.int32)):
        if t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
            raise HipExtensionError(f"select_dates: {name} must be a contiguous {dt} {list(shape)} tensor")
    call("mh_select_dates", raw, _I(code), mask, _I(Cm), _I(int(mask_floor)), dates, t_start_dev, t_win_dev, _I(int(tw.max())),
         scores, out, out_dates, out_index, _I(B), _I(Tmax), _I(nd), _L(C * S * S), _I(S * S), _I(int(bool(log_scale))),
         _F(float(norm_fac) if norm_fac is not None else 0.0))
    return out, out_dates, out_index


# ---- probe / finetune heads (csrc/heads.hip)
def token_resize(x, in_rows, in_off, out, out_rows, out_off, B, D, h, H, E):  # noqa: N803
    call("mh_token_resize", x, _L(in_rows), _I(in_off), out, _L(out_rows), _I(out_off), _I(B), _I(D), _I(h), _I(H), _I(E))


def token_resize_bwd(dout, out_rows, out_off, din, in_rows, in_off, B, D, h, H, E, accumulate=False):  # noqa: N803
    call("mh_token_resize_bwd", dout, _L(out_rows), _I(out_off), din, _L(in_rows), _I(in_off), _I(B), _I(D), _I(h), _I(H),
         _I(E), _I(int(accumulate)))


def attn_reduce_partial_rows(n_seq: int) -> int:
    return int(lib().mh_attn_reduce_partial_rows(_I(n_seq)))


def attn_reduce_fwd(kv, query, out, lse, n_batch, T, Lr, dim, heads=8):  # noqa: N803
    call("mh_attn_reduce_fwd", kv, query, out, lse, _I(n_batch), _I(T), _I(Lr), _I(dim), _I(heads))


def attn_reduce_bwd(kv, query, out, lse, dout, dkv, dq_partial, n_batch, T, Lr, dim, heads=8):  # noqa: N803
    call("mh_attn_reduce_bwd", kv, query, out, lse, dout, dkv, dq_partial, _I(n_batch), _I(T), _I(Lr), _I(dim), _I(heads))


def mean_reduce_fwd(x, out, n_batch, T, Lr, dim):  # noqa: N803
    call("mh_mean_reduce_fwd", x, out, _I(n_batch), _I(T), _I(Lr), _I(dim))


def mean_reduce_bwd(dout, dx, n_batch, T, Lr, dim):  # noqa: N803
    call("mh_mean_reduce_bwd", dout, dx, _I(n_batch), _I(T), _I(Lr), _I(dim))


def head_linear_fwd(x, W, bias, out, B, C, E):  # noqa: N803
    call("mh_head_linear_fwd", x, W, bias, out, _I(B), _I(C), _I(E))


def head_linear_bwd(x, W, dout, dx, dW, db, B, C, E):  # noqa: N803
    call("mh_head_linear_bwd", x, W, dout, dx, dW, db, _I(B), _I(C), _I(E))


def integer_targets(target: torch.Tensor) -> torch.Tensor:
    """Class-id targets as the kernels read them: signed integers of 1, 2, 4 or 8 bytes (``load_int`` sign-extends, so a ``uint8``
    id of 128 or more, or ``missing_val = 255``, would arrive negative).  Signed tensors pass without a copy; unsigned, bool and
    anything else are widened with ``.long()``, the reference's own cast (``base.py:113-118``)."""
    if target.dtype in (torch.int8, torch.int16, torch.int32, torch.int64):
        return target.contiguous()
    return target.long().contiguous()


def count_valid(target, missing_val, count):
    target = integer_targets(target)
    call("mh_count_valid", target, _I(target.element_size()), _L(target.numel()), _L(int(missing_val)), count)


def ce_loss(logits, target, missing_val, n_valid, acc, dlogits, B, g, P, C, ld=None):  # noqa: N803
    target = integer_targets(target)
    call("mh_ce_loss", logits, target, _I(target.element_size()), _L(int(missing_val)), n_valid, acc, dlogits,
         _I(1 if dlogits.dtype == torch.float32 else 0), _I(B), _I(g), _I(P), _I(C), _I(P * P * C if ld is None else ld))


def bce_loss(logits, target, missing_val, acc, dlogits, B, C):  # noqa: N803
    call("mh_bce_loss", logits, target, _F(float(missing_val)), acc, dlogits, _I(B), _I(C))


def confusion_ce(logits, target, missing_val, cm, B, g, P, C, ld=None):  # noqa: N803
    """``cm[t, argmax]`` += 1 over the valid pixels (int64 ``[C, C]``; operands as ``ce_loss``; include/maestro_hip.h)."""
    if cm.dtype != torch.int64 or cm.numel() != C * C or not cm.is_contiguous():
        raise HipExtensionError(f"confusion_ce: cm must be a contiguous int64 [{C}, {C}] tensor")
    target = integer_targets(target)
    call("mh_confusion_ce", logits, target, _I(target.element_size()), _L(int(missing_val)), cm, _I(B), _I(g), _I(P), _I(C),
         _I(P * P * C if ld is None else ld))


def logit_threshold(threshold: float) -> float:
    """``sigmoid(x) > threshold``  <=>  ``x > log(threshold / (1 - threshold))`` (0 for the reference's 0.5)."""
    import math
    if not 0.0 < threshold < 1.0:
        raise ValueError(f"detection threshold {threshold} outside (0, 1)")
    return math.log(threshold / (1.0 - threshold))


def confusion_bce(logits, target, missing_val, threshold, cm, B, C):  # noqa: N803
    """``cm[l, target > 0.5, sigmoid(logit) > threshold]`` += 1 over the used rows (int64 ``[C, 2, 2]``; operands as ``bce_loss``)."""
    if cm.dtype != torch.int64 or cm.numel() != C * 4 or not cm.is_contiguous():
        raise HipExtensionError(f"confusion_bce: cm must be a contiguous int64 [{C}, 2, 2] tensor")
    call("mh_confusion_bce", logits, target, _F(float(missing_val)), _F(logit_threshold(threshold)), cm, _I(B), _I(C))


# ---- predictions (csrc/predict.hip, include/maestro_hip.h)
PREDICT_SOFTMAX, PREDICT_SIGMOID = 0, 1


def _predict_out(what, name, t, dtype, numel):
    if t is not None and (t.dtype != dtype or t.numel() != numel or not t.is_contiguous()):
        raise HipExtensionError(f"{what}: {name} must be a contiguous {str(dtype).split('.')[-1]} tensor of {numel} elements")


def predict_view(logits, flags, act, prob, accumulate, cls, conf, B, g, P, C, ld=None, threshold=0.5):  # noqa: N803
    """One view of the batch from the head logits (f32 patch layout ``[B * g * g, ld >= P * P * C]``, the operand of ``ce_loss``).

    ``act = PREDICT_SOFTMAX``: ``prob`` f32 ``[B, C, S, S]`` (+)= the class probabilities, ``cls`` u8 ``[B, S, S]`` = ``torch.argmax``
    of the logits, ``conf`` f32 ``[B, S, S]`` = the largest probability, each pixel written where the ``mh_dihedral`` flag byte
    ``flags[b]`` (u8 ``[B]``; ``None`` = identity) took it from (``predict_pixel_map``).  ``act = PREDICT_SIGMOID`` (``g = P = 1``):
    ``prob`` / ``conf`` ``[B, C]`` = the sigmoid, ``cls`` = ``sigmoid > threshold``, decided on the logit as ``confusion_bce`` does.
    Any of ``prob``, ``cls``, ``conf`` may be ``None``, not all three."""
    ld = P * P * C if ld is None else ld
    if logits.dtype != torch.float32 or logits.stride(-1) != 1:
        raise HipExtensionError("predict_view: logits must be float32 with unit column stride")
    if logits.dim() == 2 and (logits.shape[0] != B * g * g or (logits.shape[0] > 1 and logits.stride(0) != ld)):
        raise HipExtensionError(f"predict_view: logits must be [{B * g * g}, >= {P * P * C}] with row stride ld = {ld}")
    n_map = B * C if act == PREDICT_SIGMOID else B * g * P * g * P
    _predict_out("predict_view", "prob", prob, torch.float32, B * C * g * P * g * P)
    _predict_out("predict_view", "cls", cls, torch.uint8, n_map)
    _predict_out("predict_view", "conf", conf, torch.float32, n_map)
    _predict_out("predict_view", "flags", flags, torch.uint8, B)
    thr = logit_threshold(threshold) if act == PREDICT_SIGMOID else 0.0
    call("mh_predict_view", logits, flags, _I(act), _F(thr), prob, _I(1 if accumulate else 0), cls, conf, _I(B), _I(g), _I(P), _I(C),
         _I(ld))


def predict_finish(prob, n_views, act, cls, conf, B, C, n_pix, threshold=0.5, mean=None):  # noqa: N803
    """After ``n_views`` accumulated ``predict_view`` calls on ``prob`` ``[B, C, n_pix]``: softmax -- ``cls`` = arg-max over the classes
    (the rule of ``torch.argmax``), ``conf`` = the largest sum times ``fl(1 / n_views)``; sigmoid (``n_pix = 1``) -- ``conf`` = the sum
    times ``fl(1 / n_views)``, ``cls`` = ``conf > threshold``.  ``mean`` (the shape of ``prob``, or ``prob`` itself) = ``prob`` times
    ``fl(1 / n_views)``: the mean probabilities."""
    if n_views < 1:
        raise ValueError(f"predict_finish: {n_views} views")
    n_map = B * C if act == PREDICT_SIGMOID else B * n_pix
    _predict_out("predict_finish", "prob", prob, torch.float32, B * C * n_pix)
    _predict_out("predict_finish", "cls", cls, torch.uint8, n_map)
    _predict_out("predict_finish", "conf", conf, torch.float32, n_map)
    _predict_out("predict_finish", "mean", mean, torch.float32, B * C * n_pix)
    call("mh_predict_finish", prob, _F(1.0 / n_views), _I(act), _F(float(threshold)), cls, conf, mean, _I(B), _I(C), _L(n_pix))


def predict_pixel_map(flag: int, S: int):  # noqa: N803
    """``(y0, x0)``, two int ``[S, S]`` numpy arrays: where pixel ``(y, x)`` of a view made with dihedral flag byte ``flag`` (bit 0
    flipped the rows, bit 1 the columns, bit 2 then swapped the axes: ``dataset.py:224-257``) lies in the untransformed raster."""
    import numpy as np
    y, x = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
    y0, x0 = (x, y) if flag & 4 else (y, x)
    if flag & 2:
        x0 = S - 1 - x0
    if flag & 1:
        y0 = S - 1 - y0
    return y0, x0


def argmax_reference(x, axis: int):
    """``torch.argmax`` as the kernels state it, in numpy: the lowest index among equal maxima; a NaN is the maximum and the first NaN
    wins."""
    import numpy as np
    nan = np.isnan(x)
    return np.where(nan.any(axis=axis), nan.argmax(axis=axis), np.where(nan, -np.inf, x).argmax(axis=axis)).astype(np.uint8)


def predict_reference(logits, flags, act, *, g=1, P=1, C=None, threshold=0.5, prob=None, dtype=None):  # noqa: N803
    """``predict_view`` restated in numpy (no GPU): the layout walk, the inverse dihedral map, the arg-max rule and the formulas, in
    fp32 (or ``dtype=np.float64``: the reference the kernels' rounding is bounded against).  ``logits``: array ``[B * g * g, >= P * P * C]``
    (further columns are padding and ignored); ``flags``: ``B`` flag bytes or ``None``; ``prob``: an earlier sum to accumulate onto.
    Returns ``(prob, cls, conf)`` shaped as the kernel writes them (``[B, C, S, S]``, ``[B, S, S]``, ``[B, S, S]``; sigmoid: ``[B, C]``)."""
    import numpy as np
    dtype = np.float32 if dtype is None else dtype
    logits = np.asarray(logits)
    C = logits.shape[1] if C is None else C  # noqa: N806
    S, rows = g * P, logits.shape[0]  # noqa: N806
    B = rows // (g * g)  # noqa: N806
    if act == PREDICT_SIGMOID:
        if g != 1 or P != 1:
            raise ValueError("predict_reference: the sigmoid is for classification heads (g = P = 1)")
        x = logits[:, :C].astype(np.float32)
        with np.errstate(over="ignore"):
            p = (1 / (1 + np.exp(-x.astype(dtype)))).astype(dtype)
        cls = (x > np.float32(logit_threshold(threshold))).astype(np.uint8)
        return (p if prob is None else (prob + p).astype(dtype)), cls, p
    if rows != B * g * g or logits.shape[1] < P * P * C:
        raise ValueError(f"predict_reference: logits {logits.shape} for g = {g}, P = {P}, C = {C}")
    # column (p1 * P + p2) * C + c of token row (b * g + ty) * g + tx  ->  view raster [B, C, ty * P + p1, tx * P + p2]
    view = logits[:, : P * P * C].astype(np.float32).reshape(B, g, g, P, P, C).transpose(0, 5, 1, 3, 2, 4).reshape(B, C, S, S)
    raster = np.empty_like(view)
    for b in range(B):
        y0, x0 = predict_pixel_map(0 if flags is None else int(flags[b]), S)
        raster[b][:, y0, x0] = view[b]
    cls = argmax_reference(raster, 1)
    x = raster.astype(dtype)
    with np.errstate(invalid="ignore"):
        e = np.exp(x - x.max(axis=1, keepdims=True)).astype(dtype)      # (a NaN pixel is NaN throughout, as on the device)
        s = e.sum(axis=1, dtype=dtype)
        p = (e * (1 / s)[:, None]).astype(dtype) if dtype == np.float32 else e / s[:, None]
        conf = (1 / s).astype(dtype)
    return (p if prob is None else (prob + p).astype(dtype)), cls, conf


# ---- scene prediction (csrc/scene.hip, include/maestro_hip.h)
SCENE_MAX_SLOTS, SCENE_MAX_S, SCENE_UNCOVERED = 1024, 4096, 255      # MH_SCENE_MAX_SLOTS, MH_SCENE_MAX_S, MH_SCENE_UNCOVERED


def scene_axis_starts(U: int, W: int, stride: int | None = None) -> list:  # noqa: N803
    """Window starts along one axis of ``U`` units for windows of ``W`` units: ``0, stride, 2 stride, ...`` while
    ``start + W < U``, then one last start at ``U - W`` (the clamped window: it reaches the edge whatever the stride)."""
    stride = max(1, W // 2) if stride is None else stride
    if W < 1 or U < W:
        raise ValueError(f"scene_windows: an extent of {U} units is below one window of {W}")
    if isinstance(stride, bool) or not isinstance(stride, int) or not 1 <= stride <= W:
        raise ValueError(f"scene_windows: stride={stride!r} (1 ... W = {W} units: a larger stride would leave units uncovered)")
    starts = list(range(0, U - W, stride))
    return starts + [U - W]


def scene_windows(Hu: int, Wu: int, W: int, stride: int | None = None) -> list:  # noqa: N803
    """The windows ``(y0, x0)`` of one ``Hu x Wu``-unit scene in row-major order (a pure host function): ``scene_axis_starts`` on
    both axes.  ``stride`` in ``1 .. W``, default ``max(1, W // 2)``."""
    ys, xs = scene_axis_starts(Hu, W, stride), scene_axis_starts(Wu, W, stride)
    return [(y, x) for y in ys for x in xs]


def scene_table(N: int, windows, B: int):  # noqa: N803
    """The window table of ``N`` equally sized scenes as int32 ``[n_batches, B, 4]`` rows ``(n, y0, x0, on)``: scene-major, then the
    order of ``windows``; batches are ``B`` consecutive windows and the last batch is padded with slots that repeat ITS first
    window with ``on = 0`` (gathered like any other, so the model sees finite data; blended nowhere)."""
    import numpy as np
    if N < 1 or B < 1 or not windows:
        raise ValueError(f"scene_table: N = {N}, B = {B}, {len(windows)} windows")
    rows = [(n, y, x, 1) for n in range(N) for (y, x) in windows]
    n_batches = -(-len(rows) // B)
    first = rows[(n_batches - 1) * B]
    rows += [(first[0], first[1], first[2], 0)] * (n_batches * B - len(rows))
    return np.asarray(rows, dtype=np.int32).reshape(n_batches, B, 4)


def blend_profile(S: int, kind: str = "linear"):  # noqa: N803
    """The separable window weight as numpy f32 ``[S]`` (a pixel weighs ``profile[y] * profile[x]``): ``"flat"`` all ones,
    ``"linear"`` the tent ``min(i + 1, S - i) / ceil(S / 2)`` -- 1 in the middle, never zero at the rim."""
    import numpy as np
    if S < 1:
        raise ValueError(f"blend_profile: S = {S}")
    if kind == "flat":
        return np.ones(S, dtype=np.float32)
    if kind == "linear":
        i = np.arange(S)
        return np.minimum(i + 1, S - i).astype(np.float32) / np.float32(-(-S // 2))
    raise ValueError(f"blend={kind!r}: \"flat\" or \"linear\"")


def _scene_host_table(what, table_host, B):  # noqa: N803
    import numpy as np
    t = np.ascontiguousarray(table_host, dtype=np.int32)
    if t.size != 4 * B:
        raise HipExtensionError(f"{what}: the host window table must hold {B} rows (n, y0, x0, on)")
    return t


def scene_blend_bytes(table, C, S, q) -> float:  # noqa: N803
    """Algorithmic bytes of one ``predict_blend`` launch: every ``on`` window's probabilities read once (``4 C`` per window pixel),
    every canvas pixel under at least one of them read and written once (``8 (C + 1)``: the classes and the weight sum)."""
    import numpy as np
    rows = np.asarray(table).reshape(-1, 4)
    rows = rows[rows[:, 3] != 0]
    W = -(-S // q)  # noqa: N806
    units = {(n, y, x) for n, y0, x0, _ in rows.tolist() for y in range(y0, y0 + W) for x in range(x0, x0 + W)}
    return 4.0 * C * len(rows) * S * S + 8.0 * (C + 1) * min(len(units) * q * q, len(rows) * S * S)


def window_gather(scene, out, table_dev, table_host, B, N, planes, Hs, Ws, S, q):  # noqa: N803
    """``out[b, p, y, x] = scene[n_b, p, y0_b * q + y, x0_b * q + x]`` for the ``B`` rows ``(n, y0, x0, on)`` of the window table
    (``table_dev`` int32 ``[B, 4]`` on the device, ``table_host`` the same rows on the host: checked before the launch).  ``scene``
    f32 ``[N, planes, Hs, Ws]``, ``out`` f32 ``[B, planes, S, S]``; bit-exact data movement, pad slots (``on = 0``) included."""
    _predict_out("window_gather", "scene", scene, torch.float32, N * planes * Hs * Ws)
    _predict_out("window_gather", "out", out, torch.float32, B * planes * S * S)
    _predict_out("window_gather", "table_dev", table_dev, torch.int32, 4 * B)
    host = _scene_host_table("window_gather", table_host, B)
    _hbm_call("window_gather", 8.0 * B * planes * S * S, "mh_window_gather", scene, out, table_dev, ctypes.c_void_p(host.ctypes.data),
              _I(B), _I(N), _I(planes), _I(Hs), _I(Ws), _I(S), _I(q))


def predict_blend(prob, scale, profile, table_dev, table_host, acc, wsum, B, N, C, S, q, Hc, Wc):  # noqa: N803
    """The ``B`` windows of one batch onto the canvas: ``prob`` f32 ``[B, C, S, S]`` (the sum over views ``predict_view`` leaves) times
    ``scale`` times the window weight ``profile[y] * profile[x]`` is added into ``acc`` f32 ``[N, C, Hc, Wc]`` and the weight into
    ``wsum`` f32 ``[N, Hc, Wc]`` at the window's place, slot after slot in ascending order, every product and sum rounded on its own
    (``scene_blend_reference`` states it).  Pad slots add nothing; pixels that no window of the batch covers are not touched."""
    _predict_out("predict_blend", "prob", prob, torch.float32, B * C * S * S)
    _predict_out("predict_blend", "profile", profile, torch.float32, S)
    _predict_out("predict_blend", "table_dev", table_dev, torch.int32, 4 * B)
    _predict_out("predict_blend", "acc", acc, torch.float32, N * C * Hc * Wc)
    _predict_out("predict_blend", "wsum", wsum, torch.float32, N * Hc * Wc)
    host = _scene_host_table("predict_blend", table_host, B)
    nbytes = scene_blend_bytes(host, C, S, q) if _timer is not None else 0.0      # (only a KernelTimer reads them)
    _hbm_call("predict_blend", nbytes, "mh_predict_blend", prob, _F(float(scale)), profile, table_dev,
              ctypes.c_void_p(host.ctypes.data), acc, wsum, _I(B), _I(N), _I(C), _I(S), _I(q), _I(Hc), _I(Wc))


def predict_blend_finish(acc, wsum, cls, conf, mean, N, C, n_pix):  # noqa: N803
    """After the last batch: ``cls`` u8 ``[N, n_pix]`` = the arg-max over the classes of ``acc`` f32 ``[N, C, n_pix]`` (the rule of
    ``predict_view``), ``conf`` = that maximum / ``wsum``, ``mean`` (the shape of ``acc``, or ``acc`` itself) = ``acc / wsum``,
    correctly rounded; where ``wsum == 0``: ``SCENE_UNCOVERED``, 0, 0.  Any of ``cls``, ``conf``, ``mean`` may be ``None``, not all."""
    _predict_out("predict_blend_finish", "acc", acc, torch.float32, N * C * n_pix)
    _predict_out("predict_blend_finish", "wsum", wsum, torch.float32, N * n_pix)
    _predict_out("predict_blend_finish", "cls", cls, torch.uint8, N * n_pix)
    _predict_out("predict_blend_finish", "conf", conf, torch.float32, N * n_pix)
    _predict_out("predict_blend_finish", "mean", mean, torch.float32, N * C * n_pix)
    nbytes = N * n_pix * (4.0 * (C + 1) + (1 if cls is not None else 0) + (4 if conf is not None else 0) + (4 * C if mean is not None else 0))
    _hbm_call("predict_blend_finish", nbytes, "mh_predict_blend_finish", acc, wsum, cls, conf, mean, _I(N), _I(C), _L(n_pix))


def scene_finish_reference(acc, wsum):
    """``predict_blend_finish`` restated in numpy f32: ``(cls, conf, mean)`` of ``acc [N, C, ...]`` and ``wsum [N, ...]``."""
    import numpy as np
    acc, wsum = np.asarray(acc, dtype=np.float32), np.asarray(wsum, dtype=np.float32)
    covered = wsum != 0
    w = np.where(covered, wsum, np.float32(1))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        mean = np.where(covered[:, None], acc / w[:, None], np.float32(0)).astype(np.float32)
        arg = argmax_reference(acc, 1)
        best = np.take_along_axis(acc, arg[:, None].astype(np.int64), axis=1)[:, 0]
        conf = np.where(covered, best / w, np.float32(0)).astype(np.float32)
    cls = np.where(covered, arg, SCENE_UNCOVERED).astype(np.uint8)
    return cls, conf, mean


def scene_blend_reference(prob, scale, profile, table, q, acc, wsum, finish=False):
    """``predict_blend`` restated in numpy f32 (no GPU).  ``prob [B, C, S, S]``, ``profile [S]``, ``table`` the ``B`` rows
    ``(n, y0, x0, on)``, ``acc [N, C, Hc, Wc]`` and ``wsum [N, Hc, Wc]`` the canvas so far (not modified).  The ``on`` slots are added
    one after the other in ascending order -- for a pixel, ``wsum = ((wsum + w_b1) + w_b2) ...`` and per class ``acc = ((acc +
    (prob_b1 * scale) * w_b1) + ...)``, ``w_b = profile[Y - y0_b q] * profile[X - x0_b q]``, each product and sum one fp32 operation.
    Returns the new ``(acc, wsum)``, or with ``finish`` the ``(cls, conf, mean)`` of ``scene_finish_reference`` on them."""
    import numpy as np
    prob, profile = np.asarray(prob, dtype=np.float32), np.asarray(profile, dtype=np.float32)
    acc, wsum = np.array(acc, dtype=np.float32), np.array(wsum, dtype=np.float32)
    S = prob.shape[-1]  # noqa: N806
    w = profile[:, None] * profile[None, :]
    scale = np.float32(scale)
    for b, (n, y0, x0, on) in enumerate(np.asarray(table).reshape(-1, 4).tolist()):
        if not on:
            continue
        ys, xs = slice(y0 * q, y0 * q + S), slice(x0 * q, x0 * q + S)
        if not 0 <= n < acc.shape[0] or y0 < 0 or x0 < 0 or ys.stop > acc.shape[2] or xs.stop > acc.shape[3]:
            raise ValueError(f"scene_blend_reference: slot {b} = ({n}, {y0}, {x0}) leaves the canvas {acc.shape}")
        wsum[n, ys, xs] = wsum[n, ys, xs] + w
        acc[n, :, ys, xs] = acc[n, :, ys, xs] + (prob[b] * scale) * w[None]
    return scene_finish_reference(acc, wsum) if finish else (acc, wsum)


# ---- nearest neighbours of encoder features (csrc/knn.hip, include/maestro_hip.h)
KNN_MAX_K = 128      # MH_KNN_MAX_K
_knn_ws = {}         # (device index, Nq, k, splits) -> workspace of knn_topk


def _knn_check(what, name, t, dtype, shape=None):
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or (shape is not None and tuple(t.shape) != tuple(shape)):
        want = "" if shape is None else f" of shape {list(shape)}"
        raise HipExtensionError(f"{what}: {name} must be a {str(dtype).split('.')[-1]} tensor{want}")
    if t.dim() and t.stride(-1) != 1:
        raise HipExtensionError(f"{what}: {name} must have unit column stride")


def _knn_rows(what, name, t, dtype):
    """A ``[rows, E]`` operand with unit column stride: ``(rows, E, ld)``."""
    _knn_check(what, name, t, dtype)
    if t.dim() != 2:
        raise HipExtensionError(f"{what}: {name} must be 2-dimensional [rows, E]")
    return t.shape[0], t.shape[1], (t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1]))


def _knn_gpu(what, *tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise HipExtensionError(f"{what}: maestro_amd kernels need GPU tensors (no CPU fallback)")


def knn_splits(Nq: int, Nb: int, E: int, k: int) -> int:  # noqa: N803
    """The bank-split rule of ``knn_topk`` (``mh_knn_splits``): a pure function of the shape."""
    s = int(lib().mh_knn_splits(Nq, Nb, E, k))
    if s < 1:
        raise HipExtensionError(f"knn_splits: refused shape Nq = {Nq}, Nb = {Nb}, E = {E}, k = {k}")
    return s


def knn_workspace_bytes(Nq: int, k: int, splits: int) -> int:  # noqa: N803
    n = int(lib().mh_knn_workspace_bytes(Nq, k, splits))
    if n < 0:
        raise HipExtensionError(f"knn_workspace_bytes: refused arguments Nq = {Nq}, k = {k}, splits = {splits}")
    return n


def l2_normalize(x, y=None, y16=None, eps: float = 1e-12):
    """``y = x / max(||x||_2, eps)`` per row of ``x`` f32 ``[rows, E]`` (``F.normalize``); ``y`` f32 (may be ``x``) and / or ``y16``
    bf16, the round-to-nearest-even copy of the fp32 result.  Row pitches are taken from the tensors."""
    rows, E, ldx = _knn_rows("l2_normalize", "x", x, torch.float32)  # noqa: N806
    if y is None and y16 is None:
        raise HipExtensionError("l2_normalize: no output (y and y16 are both None)")
    ldy = ldy16 = 0
    if y is not None:
        r, e, ldy = _knn_rows("l2_normalize", "y", y, torch.float32)
        if (r, e) != (rows, E):
            raise HipExtensionError(f"l2_normalize: y must be [{rows}, {E}]")
    if y16 is not None:
        r, e, ldy16 = _knn_rows("l2_normalize", "y16", y16, torch.bfloat16)
        if (r, e) != (rows, E):
            raise HipExtensionError(f"l2_normalize: y16 must be [{rows}, {E}]")
    _knn_gpu("l2_normalize", x, y, y16)
    call("mh_l2_normalize", x, _L(ldx), _F(float(eps)), y, _L(ldy), y16, _L(ldy16), _L(rows), _I(E))


def knn_topk(q, bank, k: int, sims=None, idx=None, index_base: int = 0, accumulate: bool = False, splits: int | None = None):
    """The ``k`` nearest rows of ``bank`` bf16 ``[Nb, E]`` for every row of ``q`` bf16 ``[Nq, E]`` under the order rule of
    include/maestro_hip.h (``knn_reference`` states it): ``(sims f32 [Nq, k], idx i32 [Nq, k])``, sorted, global indices
    ``index_base + row``, unfilled slots ``(-inf, -1)``.  ``sims`` / ``idx`` are allocated when not given; with ``accumulate`` the
    given ones are merged as further candidates (a bank streamed in chunks).  ``splits=None`` takes ``knn_splits``.  The workspace is
    allocated once per ``(Nq, k, splits)`` and cached: call once eagerly before capturing a graph."""
    Nq, E, ldq = _knn_rows("knn_topk", "q", q, torch.bfloat16)  # noqa: N806
    Nb, Eb, ldb = _knn_rows("knn_topk", "bank", bank, torch.bfloat16)  # noqa: N806
    if Eb != E:
        raise HipExtensionError(f"knn_topk: q has {E} columns, bank {Eb}")
    if accumulate and (sims is None or idx is None):
        raise HipExtensionError("knn_topk: accumulate needs the sims and idx of the earlier calls")
    if sims is not None or idx is not None:
        _knn_check("knn_topk", "sims", sims, torch.float32, (Nq, k))
        _knn_check("knn_topk", "idx", idx, torch.int32, (Nq, k))
        if not sims.is_contiguous() or not idx.is_contiguous():
            raise HipExtensionError("knn_topk: sims and idx must be contiguous")
    _knn_gpu("knn_topk", q, bank, sims, idx)
    if sims is None:
        sims = torch.empty(Nq, k, dtype=torch.float32, device=q.device)
        idx = torch.empty(Nq, k, dtype=torch.int32, device=q.device)
    splits = knn_splits(Nq, Nb, E, k) if splits is None else int(splits)
    nbytes = knn_workspace_bytes(Nq, k, splits)
    key = (q.device.index, Nq, k, splits)
    ws = _knn_ws.get(key)
    if ws is None:
        if torch.cuda.is_current_stream_capturing():
            raise HipExtensionError(f"knn_topk: workspace for {key[1:]} first needed inside a hipGraph capture")
        ws = _knn_ws[key] = torch.empty(nbytes, dtype=torch.uint8, device=q.device)
    _flop_call("knn_topk", 2.0 * Nq * Nb * E, (Nq, Nb, E), "mh_knn_topk", q, _L(ldq), bank, _L(ldb), _L(int(index_base)), sims, idx,
               _I(1 if accumulate else 0), ws, _L(nbytes), _I(splits), _I(Nq), _I(Nb), _I(E), _I(k))
    return sims, idx


def knn_vote(sims, idx, labels, num_classes: int, T: float = 0.07, k_eval: int | None = None, missing_val: int = -1, scores=None,  # noqa: N803
             cls=None, want_scores: bool = True, want_cls: bool = True):
    """The weighted vote of include/maestro_hip.h over the first ``k_eval`` entries of the sorted lists ``sims`` / ``idx`` ``[Nq, k]``:
    ``(scores f32 [Nq, C], cls i32 [Nq])``; ``labels`` i32 ``[n_labels]``.  ``knn_vote_reference`` states it.  ``scores`` / ``cls`` are
    allocated when not given, unless ``want_scores`` / ``want_cls`` is off (that output is then None; not both)."""
    _knn_check("knn_vote", "sims", sims, torch.float32)
    if sims.dim() != 2 or not sims.is_contiguous():
        raise HipExtensionError("knn_vote: sims must be a contiguous [Nq, k] tensor")
    Nq, k = sims.shape  # noqa: N806
    _knn_check("knn_vote", "idx", idx, torch.int32, (Nq, k))
    _knn_check("knn_vote", "labels", labels, torch.int32)
    if not idx.is_contiguous() or labels.dim() != 1 or not labels.is_contiguous():
        raise HipExtensionError("knn_vote: idx must be contiguous and labels a contiguous 1-dimensional tensor")
    if not T > 0:
        raise ValueError(f"knn_vote: temperature T = {T} (must be positive)")
    C = int(num_classes)  # noqa: N806
    k_eval = k if k_eval is None else int(k_eval)
    lds = C
    if scores is not None:
        r, c, lds = _knn_rows("knn_vote", "scores", scores, torch.float32)
        if (r, c) != (Nq, C):
            raise HipExtensionError(f"knn_vote: scores must be [{Nq}, {C}]")
    if cls is not None:
        _knn_check("knn_vote", "cls", cls, torch.int32, (Nq,))
    _knn_gpu("knn_vote", sims, idx, labels, scores, cls)
    if scores is None and want_scores:
        scores = torch.empty(Nq, C, dtype=torch.float32, device=sims.device)
    if cls is None and want_cls:
        cls = torch.empty(Nq, dtype=torch.int32, device=sims.device)
    call("mh_knn_vote", sims, idx, labels, _L(labels.numel()), _I(int(missing_val)), _F(1.0 / float(T)), _I(k), _I(k_eval), scores, _L(lds),
         cls, _I(Nq), _I(C))
    return scores, cls


def bf16_values(x):
    """The values of bf16 operands as numpy f64: a ``torch.bfloat16`` tensor, or an array of raw bf16 bit patterns (uint16)."""
    import numpy as np
    if isinstance(x, torch.Tensor):
        return x.detach().cpu().to(torch.float64).numpy()
    x = np.asarray(x)
    if x.dtype == np.uint16:
        return (x.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    return x.astype(np.float64)


def knn_order(sims, idx):
    """The order rule of include/maestro_hip.h as a permutation of candidates (numpy arrays): larger similarity first, then the smaller
    index; the caller has removed NaN similarities and negative indices."""
    import numpy as np
    return np.lexsort((np.asarray(idx), -np.asarray(sims)))


def knn_reference(q, bank, k: int, index_base: int = 0, init=None, sims=None):
    """``knn_topk`` restated in numpy (no GPU).  ``q`` ``[Nq, E]`` and ``bank`` ``[Nb, E]`` hold bf16 VALUES (``bf16_values`` takes
    what the kernel takes); the similarity of a pair is their dot product in fp64 (exact wherever the kernel's fp32 sum is, e.g. for
    small integers), or the given ``sims`` ``[Nq, Nb]`` (the tests pass measured or emulated similarities to state the rule alone).
    Per query the candidates are the pairs ``(similarity, index_base + row)`` with a non-NaN similarity and, with ``init = (sims,
    idx)`` of earlier calls, its entries with ``idx >= 0`` and a non-NaN similarity.  They are ordered by larger similarity first,
    then smaller index; the first ``k`` are returned, sorted, as ``(f32 [Nq, k], i32 [Nq, k])``, unfilled slots ``(-inf, -1)``."""
    import numpy as np
    if sims is None:
        q, bank = bf16_values(q), bf16_values(bank)
        s_all = q @ bank.T if bank.shape[0] else np.zeros((q.shape[0], 0))
    else:
        s_all = np.asarray(sims, dtype=np.float64)
    Nq, Nb = s_all.shape  # noqa: N806
    out_s, out_i = np.full((Nq, k), -np.inf, dtype=np.float32), np.full((Nq, k), -1, dtype=np.int32)
    gidx = index_base + np.arange(Nb, dtype=np.int64)
    for n in range(Nq):
        s, i = s_all[n], gidx
        if init is not None:
            s0, i0 = np.asarray(init[0][n], dtype=np.float64), np.asarray(init[1][n], dtype=np.int64)
            s, i = np.concatenate([s0[i0 >= 0], s]), np.concatenate([i0[i0 >= 0], i])
        keep = ~np.isnan(s)
        s, i = s[keep], i[keep]
        order = knn_order(s, i)[:k]
        out_s[n, : len(order)], out_i[n, : len(order)] = s[order], i[order]
    return out_s, out_i


def knn_vote_reference(sims, idx, labels, num_classes: int, T: float = 0.07, k_eval: int | None = None, missing_val: int = -1,  # noqa: N803
                       dtype=None):
    """``knn_vote`` restated in numpy (no GPU): ``(scores [Nq, C], cls i32 [Nq])``.  In fp32 (the default) the kernel's operation
    order: ``inv_T = fl(1 / T)``; per entry ``j < k_eval`` ``w_j = 1`` where ``sims[j] == sims[0]``, else ``exp(fl(fl(sims[j] -
    sims[0]) * inv_T))`` (the exponential taken in fp64 and rounded to fp32: the one place the device differs, by its own
    exponential's error); per class the
    weights of the entries that vote for it are added one by one in ascending ``j`` from 0.  An entry votes when ``0 <= idx <
    len(labels)``, its label is not ``missing_val`` and lies in ``[0, C)``.  ``cls`` = the lowest class among equal maxima of the
    scores, -1 when no entry voted.  ``dtype=np.float64``: the same sums in fp64 from the fp32 similarities."""
    import numpy as np
    dtype = np.float32 if dtype is None else dtype
    sims, idx, labels = np.asarray(sims, dtype=np.float32), np.asarray(idx, dtype=np.int64), np.asarray(labels, dtype=np.int64)
    Nq, k = sims.shape  # noqa: N806
    k_eval = k if k_eval is None else k_eval
    if not 1 <= k_eval <= k:
        raise ValueError(f"knn_vote_reference: k_eval = {k_eval} outside 1 ... k = {k}")
    C = int(num_classes)  # noqa: N806
    inv_t = dtype(np.float32(1.0 / float(T)))
    scores, cls = np.zeros((Nq, C), dtype=dtype), np.full(Nq, -1, dtype=np.int32)
    for n in range(Nq):
        voted = False
        s0 = sims[n, 0].astype(dtype)
        for j in range(k_eval):
            i = idx[n, j]
            if not 0 <= i < len(labels):
                continue
            lab = labels[i]
            if lab == missing_val or not 0 <= lab < C:
                continue
            s = sims[n, j].astype(dtype)
            with np.errstate(invalid="ignore", over="ignore", under="ignore"):
                w = dtype(1) if s == s0 else dtype(np.exp(np.float64(dtype(dtype(s - s0) * inv_t))))
            scores[n, lab] = dtype(scores[n, lab] + w)
            voted = True
        if voted:
            cls[n] = int(np.argmax(scores[n]))          # (numpy: the first of equal maxima; no NaN can arise)
    return scores, cls


def zero_spans(base, spans, n_spans, max_len):
    call("mh_zero_spans", base, spans, _I(n_spans), _L(max_len))


def colsum(x, out, M, N, ld):
    call("mh_colsum", x, _I(1 if x.dtype == torch.float32 else 0), out, _I(M), _I(N), _I(ld))


def scale_dev(x, n, scale):
    """``x[:n] *= scale`` with ``scale`` a 1-element f32 device tensor (read on the device; no-op when it is 1)."""
    call("mh_scale_dev", x, _L(n), scale)


def cast_bf16(src, dst, n):
    call("mh_cast_bf16", src, dst, _L(n))


def pack_rows_bf16(w, dst, E, K, Kpad):
    call("mh_pack_rows_bf16", w, dst, _I(E), _I(K), _I(Kpad))


def unpack_rows_add(src, dst, E, K, Kpad):
    call("mh_unpack_rows_add", src, dst, _I(E), _I(K), _I(Kpad))


GROUP_BLOCK, GROUP_TABLE = 64, 256      # MH_ADAMW_GROUP_BLOCK, MH_ADAMW_GROUP_TABLE
ADAMW_SR_TAG = 0x5352424D               # MH_ADAMW_SR_TAG: c3 of every rounding draw
_U64 = ctypes.c_uint64


def _adamw(p, g, m, v, p_bf16, n, b1, b2, eps, *, wd=None, groups=None, scalars=None, hyper=None, draws=None, step_dev=None):
    """The eight forms {fp32 | bf16 moments} x {plain | grouped} x {host | device scalars} of ``mh_adamw`` behind the wrappers
    below; what is given selects the entry.  ``groups = (group_of, lr_scale, wd)`` in place of ``wd``; ``scalars = (lr, step,
    grad_scale)`` or the device tensor ``hyper``; ``draws = (elem_base, seed)``: m and v are bf16 (then the device form also takes
    ``step_dev``).  Algorithmic bytes per parameter: 30, or 22 with bf16 moments, minus an absent shadow."""
    what = "adamw" + ("_groups" if groups is not None else "") + ("_bf16m" if draws is not None else "") + ("_dev" if scalars is None else "")
    if groups is not None:      # the sizes the kernel relies on: one map byte per 64-element block of [0, n), two tables of 256 floats
        group_of, lr_scale, wd_of = groups
        if group_of.dtype != torch.uint8 or not group_of.is_contiguous() or group_of.numel() < -(-int(n) // GROUP_BLOCK):
            raise HipExtensionError(f"{what}: the group map must be a dense uint8 tensor of at least ceil(n / {GROUP_BLOCK}) = "
                                    f"{-(-int(n) // GROUP_BLOCK)} bytes")
        for name, t in (("lr_scale", lr_scale), ("wd", wd_of)):
            if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != GROUP_TABLE:
                raise HipExtensionError(f"{what}: {name} must be a dense f32 table of exactly {GROUP_TABLE} entries")
    if draws is not None:       # a fp32 buffer handed to these entries would be read as twice as many bf16
        for name, t in (("m16", m), ("v16", v)):
            if t.dtype != torch.bfloat16 or not t.is_contiguous() or t.numel() < int(n):
                raise HipExtensionError(f"{what}: {name} must be a dense bfloat16 tensor of at least n = {int(n)} elements")
        if scalars is None and (step_dev.dtype != torch.int64 or step_dev.numel() < 1):
            raise HipExtensionError(f"{what}: step_dev must be an int64 tensor")
    args = [p, g, m, v, p_bf16, *(groups or ()), _L(n)]
    if draws is not None:
        args += [_L(draws[0]), _U64(int(draws[1]) & 0xFFFFFFFFFFFFFFFF)]
    args += ([] if scalars is None else [_F(scalars[0])]) + [_F(b1), _F(b2), _F(eps)] + ([] if groups is not None else [_F(wd)])
    args += [_I(scalars[1]), _F(scalars[2])] if scalars is not None else [hyper] + ([step_dev] if draws is not None else [])
    _hbm_call("adamw", float(n) * ((22 if draws is not None else 30) - 2 + _esz(p_bf16)), "mh_" + what, *args)


def adamw(p, g, m, v, p_bf16, n, lr, b1, b2, eps, wd, step, grad_scale=1.0):
    _adamw(p, g, m, v, p_bf16, n, b1, b2, eps, wd=wd, scalars=(lr, step, grad_scale))


def adamw_fp8(p, g, m, v, p_bf16, p_fp8, slot_map, scale, amax, n, lr, b1, b2, eps, wd, step, grad_scale=1.0):
    """AdamW that also writes the e4m3 weight shadows (delayed scaling; see ``mh_adamw_fp8``)."""
    call("mh_adamw_fp8", p, g, m, v, p_bf16, p_fp8, slot_map, scale, amax, _L(n), _F(lr), _F(b1), _F(b2), _F(eps), _F(wd), _I(step),
         _F(grad_scale))


_libm = None


def adamw_bias_corrections(b1: float, b2: float, step: int) -> tuple[float, float]:
    """``(1 - b1^t, sqrt(1 - b2^t))`` in the float32 arithmetic ``mh_adamw`` uses on the host (libm ``powf``), so that the
    device-scalar variant applies bit-identical updates."""
    import numpy as np
    global _libm
    if _libm is None:
        _libm = ctypes.CDLL("libm.so.6")
        _libm.powf.restype = ctypes.c_float
        _libm.powf.argtypes = [ctypes.c_float, ctypes.c_float]
    libm = _libm
    f = np.float32
    bc1 = f(1.0) - f(libm.powf(float(f(b1)), float(step)))
    bc2 = np.sqrt(f(1.0) - f(libm.powf(float(f(b2)), float(step))), dtype=np.float32)
    return float(bc1), float(bc2)


def adamw_dev(p, g, m, v, p_bf16, n, b1, b2, eps, wd, hyper):
    """AdamW with {lr, 1 - b1^t, sqrt(1 - b2^t), grad_scale, active} read from the device tensor ``hyper`` (graph-capturable)."""
    _adamw(p, g, m, v, p_bf16, n, b1, b2, eps, wd=wd, hyper=hyper)


def adamw_groups(p, g, m, v, p_bf16, group_of, lr_scale, wd, n, lr, b1, b2, eps, step, grad_scale=1.0):
    """``adamw`` with per-group hyper-parameters: element ``i`` is updated with ``lr * lr_scale[group_of[i // 64]]`` (one fp32
    product) and ``wd[group_of[i // 64]]``; ``group_of`` uint8 (``p`` starts on a 64-element block of the layout the map was
    built for), ``lr_scale`` / ``wd`` f32 tables of 256 entries (``ParamGroups`` owns all three)."""
    _adamw(p, g, m, v, p_bf16, n, b1, b2, eps, groups=(group_of, lr_scale, wd), scalars=(lr, step, grad_scale))


def adamw_groups_dev(p, g, m, v, p_bf16, group_of, lr_scale, wd, n, b1, b2, eps, hyper):
    """``adamw_groups`` with {lr, 1 - b1^t, sqrt(1 - b2^t), grad_scale, active} read from the device tensor ``hyper``."""
    _adamw(p, g, m, v, p_bf16, n, b1, b2, eps, groups=(group_of, lr_scale, wd), hyper=hyper)


def adamw_bf16m(p, g, m16, v16, p_bf16, n, elem_base, seed, lr, b1, b2, eps, wd, step, grad_scale=1.0):
    """``adamw`` with both moments held as bf16: upcast exactly, updated in fp32 (``p`` moves by the unrounded moments), stored by
    stochastic rounding with the words of ``sr_bf16_reference`` at indices ``elem_base + i`` (``elem_base``: the offset of
    ``p[0]`` in the flat layout, a multiple of 4).  22 bytes per parameter instead of 30."""
    _adamw(p, g, m16, v16, p_bf16, n, b1, b2, eps, wd=wd, scalars=(lr, step, grad_scale), draws=(elem_base, seed))


def adamw_bf16m_dev(p, g, m16, v16, p_bf16, n, elem_base, seed, b1, b2, eps, wd, hyper, step_dev):
    """``adamw_dev`` with bf16 moments; ``step_dev``: a 1-element int64 DEVICE tensor holding Adam's ``t`` (the guard's counter,
    read by the kernel after ``grad_guard_finish`` wrote it)."""
    _adamw(p, g, m16, v16, p_bf16, n, b1, b2, eps, wd=wd, hyper=hyper, draws=(elem_base, seed), step_dev=step_dev)


def adamw_groups_bf16m(p, g, m16, v16, p_bf16, group_of, lr_scale, wd, n, elem_base, seed, lr, b1, b2, eps, step, grad_scale=1.0):
    """``adamw_groups`` with bf16 moments (``elem_base`` a multiple of 64: the map has one byte per 64 elements)."""
    _adamw(p, g, m16, v16, p_bf16, n, b1, b2, eps, groups=(group_of, lr_scale, wd), scalars=(lr, step, grad_scale),
           draws=(elem_base, seed))


def adamw_groups_bf16m_dev(p, g, m16, v16, p_bf16, group_of, lr_scale, wd, n, elem_base, seed, b1, b2, eps, hyper, step_dev):
    """``adamw_groups_dev`` with bf16 moments (``step_dev`` as in ``adamw_bf16m_dev``)."""
    _adamw(p, g, m16, v16, p_bf16, n, b1, b2, eps, groups=(group_of, lr_scale, wd), hyper=hyper,
           draws=(elem_base, seed), step_dev=step_dev)


def sr_bf16_words(index, seed, step, which):
    """The 16-bit random word of the stochastic rounding at flat element ``index`` (array), for moment ``which`` ("m" / "v"):
    Philox4x32-10, key ``(seed & 0xffffffff, seed >> 32)``, counter ``(index // 4, step, 0, ADAMW_SR_TAG)`` (each the low 32
    bits); element ``e = index % 4`` takes ``(w[e >> 1] >> 16 * (e & 1)) & 0xffff`` for ``m`` and the same of ``w[2 + (e >> 1)]``
    for ``v``.  uint32 array."""
    import numpy as np

    from maestro_amd.layers.utils import philox4x32
    if which not in ("m", "v"):
        raise ValueError(f"which={which!r}: expected 'm' or 'v'")
    index = np.asarray(index).astype(np.uint64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    w = philox4x32((index >> np.uint64(2), np.uint64(int(step) & 0xFFFFFFFF), np.uint64(0), np.uint64(ADAMW_SR_TAG)),
                   (seed & 0xFFFFFFFF, seed >> 32))
    e = (index & np.uint64(3)).astype(np.intp)
    word = np.choose((e >> 1) + (2 if which == "v" else 0), w)
    return (word >> (np.uint32(16) * (e & 1).astype(np.uint32))) & np.uint32(0xFFFF)


def sr_bf16_round(bits_f32, r):
    """The rounding rule alone, on integers: fp32 bit patterns ``bits_f32`` and 16-bit words ``r`` (arrays) -> bf16 bit patterns
    (uint16).  inf / NaN: the upper half (a NaN whose surviving mantissa bits are zero gets the quiet bit); else ``t = u + r``,
    and ``t >> 16`` unless ``t`` carried into an all-ones exponent, then ``u >> 16``."""
    import numpy as np
    u = np.asarray(bits_f32).astype(np.uint64) & np.uint64(0xFFFFFFFF)
    r = np.asarray(r).astype(np.uint64)
    if r.size and int(r.max()) > 0xFFFF:
        raise ValueError("sr_bf16_round: r must be a 16-bit word")
    exp = np.uint64(0x7F800000)
    special = (u & exp) == exp
    nan_lost = special & ((u & np.uint64(0x007FFFFF)) != 0) & ((u & np.uint64(0x007F0000)) == 0)
    t = u + r
    keep = (t & exp) == exp
    out = np.where(special, (u >> np.uint64(16)) | np.where(nan_lost, np.uint64(0x40), np.uint64(0)),
                   np.where(keep, u, t) >> np.uint64(16))
    return out.astype(np.uint16)


def sr_bf16_reference(bits_f32, index, seed, step, which):
    """What ``adamw_bf16m`` stores for a new fp32 moment: ``bits_f32`` (uint32 array: the fp32 bit patterns) at flat element
    indices ``index`` (``elem_base + i``) -> bf16 bit patterns (uint16), the contract of include/maestro_hip.h restated in
    numpy integers (runs on any machine).  ``which``: "m" or "v"."""
    return sr_bf16_round(bits_f32, sr_bf16_words(index, seed, step, which))


class ParamGroups:
    """Per-group ``(lr_scale, wd)`` over a flat parameter layout, in the form ``adamw_groups`` reads: a uint8 map with one byte per
    64-element block and two f32 tables of 256 entries (unused entries ``lr_scale = 0``, ``wd = 0``: a stray map byte would freeze
    its block, not move it).  ``spans``: ``(lo, hi, lr_scale, wd)`` in any order; every boundary a multiple of 64, together they
    tile ``[0, total)`` without gap or overlap.  Spans whose ``(lr_scale, wd)`` agree AS fp32 share one group id (ids in order of
    first appearance from the front of the layout); at most 256 distinct pairs.  ``ValueError`` otherwise.  ``pairs[g]``: the
    fp32 ``(lr_scale, wd)`` of group ``g`` as Python floats; ``spans``: the sorted ``(lo, hi, group id)``."""

    def __init__(self, spans, device) -> None:
        import numpy as np
        spans = sorted((int(lo), int(hi), float(np.float32(s)), float(np.float32(w))) for lo, hi, s, w in spans)
        if not spans:
            raise ValueError("ParamGroups: no spans")
        ids, out, end = {}, [], 0
        for lo, hi, s, w in spans:
            if lo % GROUP_BLOCK or hi % GROUP_BLOCK:
                raise ValueError(f"ParamGroups: span [{lo}, {hi}) is not aligned to {GROUP_BLOCK} elements")
            if hi <= lo:
                raise ValueError(f"ParamGroups: span [{lo}, {hi}) is empty")
            if lo > end:
                raise ValueError(f"ParamGroups: gap [{end}, {lo}) -- the spans must tile the layout from 0")
            if lo < end:
                raise ValueError(f"ParamGroups: overlap -- span [{lo}, {hi}) starts before {end}")
            if not (math.isfinite(s) and math.isfinite(w)):
                raise ValueError(f"ParamGroups: span [{lo}, {hi}) has a non-finite lr_scale / wd")
            gid = ids.setdefault((s, w), len(ids))
            out.append((lo, hi, gid))
            end = hi
        if len(ids) > GROUP_TABLE:
            raise ValueError(f"ParamGroups: {len(ids)} distinct (lr_scale, wd) pairs, at most {GROUP_TABLE} fit the tables")
        self.total, self.spans, self.pairs = end, out, list(ids)
        group_of = np.zeros(end // GROUP_BLOCK, dtype=np.uint8)
        for lo, hi, gid in out:
            group_of[lo // GROUP_BLOCK: hi // GROUP_BLOCK] = gid
        table = np.zeros((2, GROUP_TABLE), dtype=np.float32)
        table[:, : len(ids)] = np.array(self.pairs, dtype=np.float32).T
        self.group_of = torch.from_numpy(group_of).to(device)
        self.lr_scale, self.wd = torch.from_numpy(table[0].copy()).to(device), torch.from_numpy(table[1].copy()).to(device)

    def map_at(self, a: int) -> torch.Tensor:
        """The map for a slice of the layout that starts at element ``a`` (a multiple of 64, ``0 <= a < total``)."""
        a = int(a)
        if a % GROUP_BLOCK or not 0 <= a < self.total:
            raise ValueError(f"ParamGroups.map_at: offset {a} must be a multiple of {GROUP_BLOCK} inside [0, {self.total})")
        return self.group_of[a // GROUP_BLOCK:]

    def of(self, i: int) -> tuple[float, float]:
        """``(lr_scale, wd)`` of element ``i`` (host lookup, for tests and tools)."""
        for lo, hi, gid in self.spans:
            if lo <= i < hi:
                return self.pairs[gid]
        raise IndexError(i)


# ------------------------------------------------------------------------------------------------ kernel timing
class KernelTimer:
    """HIP-event timing of the MFMA kernels on the stream they are launched on (bench.py's roofline leg)."""

    def __init__(self) -> None:
        self.events: dict[str, list] = {}
        self.flops: dict[str, float] = {}
        self.count: dict[str, int] = {}
        self.shapes: dict = {}
        self.hbm: dict[str, list] = {}      # HBM-bound sub-stages: kind -> [(e0, e1, algorithmic bytes)]

    def record(self, kind: str, flops: float, shape=None):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        self.events.setdefault(kind, []).append((e0, e1))
        if shape is not None:
            self.shapes.setdefault((kind, shape), []).append((e0, e1, flops))
        self.flops[kind] = self.flops.get(kind, 0.0) + flops
        self.count[kind] = self.count.get(kind, 0) + 1
        return e0, e1

    def record_bytes(self, kind: str, nbytes: float):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        self.hbm.setdefault(kind, []).append((e0, e1, nbytes))
        return e0, e1

    def hbm_substages(self, peak_gbs: float) -> dict:
        """Per HBM-bound kernel: achieved GB/s = algorithmic bytes / HIP-event duration, summed over its launches."""
        torch.cuda.synchronize()
        out = {}
        for kind, evs in sorted(self.hbm.items()):
            ms = sum(a.elapsed_time(b) for a, b, _ in evs)
            nb = sum(n for _, _, n in evs)
            if ms > 0:
                out[kind] = {"gb_s": round(nb / ms / 1e6, 1), "frac": round(nb / ms / 1e6 / peak_gbs, 3), "launches": len(evs),
                             "avg_us": round(1e3 * ms / len(evs), 2), "mb_per_launch": round(nb / len(evs) / 1e6, 2)}
        return out

    def totals(self) -> dict[str, float]:
        torch.cuda.synchronize()
        return {k: sum(a.elapsed_time(b) for a, b in v) for k, v in self.events.items()}  # ms

    def summary(self, steps: int) -> dict:
        return {k: round(v / steps, 3) for k, v in self.totals().items()}

    def by_shape(self, steps: int) -> list:
        torch.cuda.synchronize()
        rows = []
        for (kind, shape), evs in self.shapes.items():
            ms = sum(a.elapsed_time(b) for a, b, _ in evs)
            fl = sum(f for _, _, f in evs)
            rows.append((ms / steps, kind, shape, len(evs) // steps, fl / (ms * 1e-3) / 1e12))
        return sorted(rows, reverse=True)

    def roofline(self, peak_tflops: float) -> dict:
        tot = self.totals()
        kind = max(tot, key=tot.get)
        achieved = self.flops[kind] / (tot[kind] * 1e-3) / 1e12
        return {"bound": "mfma", "kernel": kind, "achieved": round(achieved, 1), "peak": peak_tflops, "unit": "TFLOP/s",
                "frac": round(achieved / peak_tflops, 4), "launches": self.count[kind],
                "avg_launch_us": round(1e3 * tot[kind] / self.count[kind], 2),
                "flops_per_launch": round(self.flops[kind] / self.count[kind]), "traffic": None}


_timer: KernelTimer | None = None


def set_kernel_timer(t: KernelTimer | None) -> None:
    global _timer
    _timer = t


def kernel_timer_active() -> bool:
    return _timer is not None


# ------------------------------------------------------------------------------------------------ grouped wgrad
class _MhGroupedGemm(ctypes.Structure):
    _fields_ = [("A", ctypes.c_void_p), ("B", ctypes.c_void_p), ("C", ctypes.c_void_p), ("M", ctypes.c_int),
                ("N", ctypes.c_int), ("K", ctypes.c_int), ("lda", ctypes.c_int), ("ldb", ctypes.c_int), ("ldc", ctypes.c_int),
                ("reserved", ctypes.c_int), ("accumulate", ctypes.c_int)]


class GroupedTN:
    """Descriptor table (built once: all buffers are static) for ``mh_gemm_grouped_tn``: every entry is one
    dW[M, N] (f32) = A[K, M]^T B[K, N] problem; the launch covers all their 256x256 tiles.  A dW written by a single
    problem is stored; one shared by several problems (same encoder on several groups) is accumulated atomically."""

    @staticmethod
    def check(i, prob) -> int:
        """Validates one problem against the kernel's addressing limits; returns its number of 256x256 tiles."""
        A, B, C, M, N, K, lda, ldb, ldc = prob  # noqa: N806
        if M % 8 or N % 8 or lda % 8 or ldb % 8 or ldc % 4 or min(M, N, K) <= 0:
            raise HipExtensionError(f"grouped wgrad problem {i}: M, N, lda, ldb must be multiples of 8 ({M}, {N}, {lda}, {ldb})")
        if C.dtype != torch.float32 or A.dtype != torch.bfloat16 or B.dtype != torch.bfloat16:
            raise HipExtensionError("grouped wgrad: A, B bf16 and C f32 expected")
        if (-(-K // 32) * 32) * max(lda, ldb) * 2 + 65536 >= 1 << 31:
            raise HipExtensionError(f"grouped wgrad problem {i}: operand beyond the 2 GiB buffer-descriptor range")
        return -(-M // 256) * -(-N // 256)

    @staticmethod
    def count_tiles(problems) -> int:
        return sum(GroupedTN.check(i, p) for i, p in enumerate(problems))

    N_XCD = 8

    def __init__(self, problems, device) -> None:
        arr = (_MhGroupedGemm * len(problems))()
        self.keep = []
        writers = {}
        for prob in problems:
            writers[prob[2].data_ptr()] = writers.get(prob[2].data_ptr(), 0) + 1
        units = []   # (work, problem index, tiles_m, tiles_n)
        for i, prob in enumerate(problems):
            A, B, C, M, N, K, lda, ldb, ldc = prob  # noqa: N806
            n = self.check(i, prob)
            shared = int(writers[C.data_ptr()] > 1)   # several problems add into one (zeroed) dW: atomic epilogue
            arr[i] = _MhGroupedGemm(A.data_ptr(), B.data_ptr(), C.data_ptr(), M, N, K, lda, ldb, ldc, 0, shared)
            units.append((n * K, i, -(-M // 256), -(-N // 256)))
            self.keep += [A, B, C]
        # One tile queue per XCD.  Whole problems go to the least-loaded queue, largest first (work = tiles x K), so that a
        # problem's tiles run under one L2 at the same time and share their dY / X panels; a problem bigger than half a
        # queue's fair share is dealt out by rows of tiles (one dY panel each) instead.
        fair = sum(u[0] for u in units) / self.N_XCD
        pieces = []  # (work, K, [tile ids])
        for work, i, tm, tn in units:
            K = problems[i][5]  # noqa: N806
            rows = [[(i << 16) | (r << 8) | c for c in range(tn)] for r in range(tm)]
            if work > 0.5 * fair and tm > 1:
                pieces += [(tn * K, K, row) for row in rows]
            else:
                pieces.append((work, K, [t for row in rows for t in row]))
        load = [0.0] * self.N_XCD
        queues = [[] for _ in range(self.N_XCD)]
        for work, K, ids in sorted(pieces, key=lambda p: -p[0]):  # noqa: N806
            x = min(range(self.N_XCD), key=load.__getitem__)
            load[x] += work
            queues[x].append((K, ids))
        qlen = max(sum(len(ids) for _, ids in q) for q in queues)
        flat = torch.full((self.N_XCD, qlen), 0xFFFFFFFF, dtype=torch.int64)
        for x, q in enumerate(queues):
            ids = [t for _, tiles in sorted(q, key=lambda e: -e[0]) for t in tiles]   # longest tiles first
            flat[x, : len(ids)] = torch.tensor(ids, dtype=torch.int64)
        self.queues = flat.to(torch.uint32).to(device)
        raw = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
        self.table = raw.to(device)
        self.n, self.queue_len = len(problems), qlen
        self.tiles = sum(u[2] * u[3] for u in units)
        self.balance = max(load) / max(fair, 1e-9)       # 1.0 = perfectly even queues
        self.flops = sum(2.0 * M * N * K for (_, _, _, M, N, K, _, _, _) in problems)

    def launch(self) -> None:
        if _timer is None:
            call("mh_gemm_grouped_tn", self.table, _I(self.n), self.queues, _I(self.queue_len))
            return
        e0, e1 = _timer.record("gemm_dma_grouped_tn_kernel", self.flops, ("grouped", self.n, self.tiles))
        e0.record()
        call("mh_gemm_grouped_tn", self.table, _I(self.n), self.queues, _I(self.queue_len))
        e1.record()


# ------------------------------------------------------------------------------------------------ fp8 path (C5)
FP8_E4M3, FP8_E5M2 = 0, 1
FP8_MAX = {FP8_E4M3: 448.0, FP8_E5M2: 57344.0}
QCHUNK = 4096   # elements per work item of mh_quant_batched (csrc/quant.hip)


_FP8_TILE_HINT = {"256": 2048, "128": 4096, "128d": 8192}   # MH_GEMM_FP8_TILE_* (include/maestro_hip.h)


def gemm_fp8(M, N, K, A8, lda, B8, ldb, C, ldc, descale_a, descale_b, flags=0, a_format=FP8_E4M3, bias=None, res=None, ldr=0,  # noqa: N803
             aux_in=None, aux_out=None, ldaux=0, colsum=None, c8=None, ldc8=0, c8_scale=None, c8_amax=None) -> None:
    """``C = descale_a * descale_b * A8 @ B8^T`` (+ epilogue): A8 ``[M, K]`` / B8 ``[N, K]`` uint8 tensors holding OCP fp8."""
    ev = None
    if _timer is not None:
        ev = _timer.record("gemm_fp8_kernel", 2.0 * M * N * K, (M, N, K))
        ev[0].record()
    flags |= _FP8_TILE_HINT.get(os.environ.get("MH_FP8_TILE", ""), 0)      # (experiments / tests; the library reads no environment)
    _check(lib().mh_gemm_fp8(_I(M), _I(N), _I(K), ptr(A8), _I(lda), _I(a_format), ptr(B8), _I(ldb), ptr(C), _I(ldc), _I(flags),
                             ptr(descale_a), ptr(descale_b), ptr(bias), ptr(res), _I(ldr), ptr(aux_in), ptr(aux_out), _I(ldaux),
                             ptr(colsum), ptr(c8), _I(ldc8), ptr(c8_scale), ptr(c8_amax), stream()), "mh_gemm_fp8")
    if ev is not None:
        ev[1].record()


class _MhQuantJob(ctypes.Structure):
    _fields_ = [("src", ctypes.c_void_p), ("dst", ctypes.c_void_p), ("dst_t", ctypes.c_void_p), ("n", ctypes.c_long),
                ("rows", ctypes.c_int), ("cols", ctypes.c_int), ("slot", ctypes.c_int), ("is_f32", ctypes.c_int),
                ("format", ctypes.c_int), ("reserved", ctypes.c_int)]


AMAX_PITCH = 32 * 64   # MH_FP8_AMAX_SUBSLOTS * MH_FP8_AMAX_STRIDE


class Fp8Scales:
    """Scale / descale / amax tables (one slot per quantised tensor), all on the device.  ``amax`` is [n_slots, AMAX_PITCH]: the
    kernels fold into one of 32 sub-slots of a slot's row (``MH_FP8_AMAX_PITCH`` in the header: same-line atomics are slow);
    ``absmax(slot)`` is the maximum over the row."""

    def __init__(self, n_slots: int, device) -> None:
        self.n = n_slots
        self.scale = torch.ones(n_slots, dtype=torch.float32, device=device)
        self.descale = torch.ones(n_slots, dtype=torch.float32, device=device)
        self.amax = torch.zeros(n_slots, AMAX_PITCH, dtype=torch.float32, device=device)

    def absmax(self, slot: int) -> float:
        return float(self.amax[slot].max())

    def update(self, lo: int = 0, hi: int | None = None, fmt: int = FP8_E4M3, margin: int = 1) -> None:
        """``scale = 2^(floor(log2(max / amax)) - margin)`` for slots ``lo .. hi-1``; resets their amax."""
        hi = self.n if hi is None else hi
        call("mh_fp8_update_scales", self.amax[lo:hi], self.scale[lo:hi], self.descale[lo:hi], _I(hi - lo), _F(FP8_MAX[fmt]),
             _I(margin))


class _MhTransposeJob(ctypes.Structure):
    _fields_ = [("src", ctypes.c_void_p), ("dst", ctypes.c_void_p), ("rows", ctypes.c_int), ("cols", ctypes.c_int)]


class TransposeBatch:
    """``mh_transpose_u8_batched``: ``pairs`` = (src uint8 [rows, cols], dst uint8 [cols, rows]), rows and cols multiples of 64."""

    def __init__(self, pairs, device) -> None:
        arr = (_MhTransposeJob * len(pairs))()
        items, self.keep = [], []
        for i, (src, dst) in enumerate(pairs):
            rows, cols = src.shape
            if rows % 64 or cols % 64 or tuple(dst.shape) != (cols, rows) or not (src.is_contiguous() and dst.is_contiguous()) \
                    or src.dtype != torch.uint8 or dst.dtype != torch.uint8 or (src.data_ptr() | dst.data_ptr()) % 16:
                raise HipExtensionError("TransposeBatch: contiguous 16-byte aligned uint8 [rows, cols] -> [cols, rows], multiples of 64")
            arr[i] = _MhTransposeJob(src.data_ptr(), dst.data_ptr(), rows, cols)
            items += [(i << 32) | t for t in range((rows // 64) * (cols // 64))]
            self.keep += [src, dst]
        self.table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(device)
        self.items = torch.tensor(items, dtype=torch.int64).to(device)
        self.n_items = len(items)

    def launch(self) -> None:
        call("mh_transpose_u8_batched", self.table, self.items, _I(self.n_items))


class QuantBatch:
    """Job table for ``mh_quant_batched``: ``jobs`` = dicts(src, dst=None, dst_t=None, slot, format=FP8_E4M3); a transposed copy
    needs a 2-D ``src``.  ``launch(mode)``: 0 absmax only, 1 cast, 2 cast + absmax (delayed scaling)."""

    def __init__(self, jobs, scales: Fp8Scales, device) -> None:
        arr = (_MhQuantJob * len(jobs))()
        items, self.keep = [], []
        for i, jb in enumerate(jobs):
            src, dst, dst_t = jb["src"], jb.get("dst"), jb.get("dst_t")
            n = src.numel()
            if n % 4 or not src.is_contiguous() or src.dtype not in (torch.float32, torch.bfloat16):
                raise HipExtensionError("QuantBatch: contiguous f32 / bf16 sources with numel % 4 == 0 expected")
            rows, cols = (src.shape[0], n // src.shape[0]) if src.dim() >= 2 else (1, n)
            if dst_t is not None and (cols % 4 or dst_t.numel() != n):
                raise HipExtensionError("QuantBatch: the transposed copy needs cols % 4 == 0 and as many bytes as elements")
            if dst is not None and dst.numel() != n:
                raise HipExtensionError("QuantBatch: dst must hold one byte per source element")
            arr[i] = _MhQuantJob(src.data_ptr(), dst.data_ptr() if dst is not None else None,
                                 dst_t.data_ptr() if dst_t is not None else None, n, rows, cols, jb["slot"],
                                 int(src.dtype == torch.float32), jb.get("format", FP8_E4M3), 0)
            items += [(i << 32) | c for c in range(-(-n // QCHUNK))]
            self.keep += [t for t in (src, dst, dst_t) if t is not None]
        self.table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(device)
        self.items = torch.tensor(items, dtype=torch.int64).to(device)
        self.scales, self.n_items = scales, len(items)

    def launch(self, mode: int) -> None:
        call("mh_quant_batched", self.table, self.items, _I(self.n_items), self.scales.scale, self.scales.amax, _I(mode))


# ------------------------------------------------------------------------------------------------ MX block scaling (fp8 `mx`)
MX_BLOCK = 32          # elements per E8M0 scale along K
MX_CHUNK = 4096        # elements per work item of mh_quant_mx_batched (csrc/quant.hip)


def gemm_mx(M, N, K, A8, lda, sa, ldsa, B8, ldb, sb, ldsb, C, ldc, flags=0, bias=None, res=None, ldr=0,  # noqa: N803
            aux_in=None, aux_out=None, ldaux=0, colsum=None, c8=None, ldc8=0, c8_scales=None, ldc8s=0) -> None:
    """``C = (A8 x 2^sa) @ (B8 x 2^sb)^T`` (+ epilogue): e4m3 A8 ``[M, K]`` / B8 ``[N, K]`` uint8 with E8M0 scales ``[M, K/32]`` /
    ``[N, K/32]``; ``c8`` / ``c8_scales``: the MX copy of the bf16 output.  Timed as ``gemm_fp8_kernel`` (same kernel body)."""
    ev = None
    if _timer is not None:
        ev = _timer.record("gemm_fp8_kernel", 2.0 * M * N * K, (M, N, K))
        ev[0].record()
    flags |= _FP8_TILE_HINT.get(os.environ.get("MH_FP8_TILE", ""), 0)      # (experiments / tests; the library reads no environment)
    _check(lib().mh_gemm_mx(_I(M), _I(N), _I(K), ptr(A8), _I(lda), ptr(sa), _I(ldsa), ptr(B8), _I(ldb), ptr(sb), _I(ldsb), ptr(C),
                            _I(ldc), _I(flags), ptr(bias), ptr(res), _I(ldr), ptr(aux_in), ptr(aux_out), _I(ldaux), ptr(colsum),
                            ptr(c8), _I(ldc8), ptr(c8_scales), _I(ldc8s), stream()), "mh_gemm_mx")
    if ev is not None:
        ev[1].record()


class _MhQuantMxJob(ctypes.Structure):
    _fields_ = [("src", ctypes.c_void_p), ("dst", ctypes.c_void_p), ("scales", ctypes.c_void_p), ("rows", ctypes.c_int),
                ("cols", ctypes.c_int), ("ld_src", ctypes.c_int), ("ld_dst", ctypes.c_int), ("ld_s", ctypes.c_int),
                ("reserved", ctypes.c_int)]


class QuantMxBatch:
    """Job table for ``mh_quant_mx_batched``: ``jobs`` = dicts(src bf16 [rows, cols], dst uint8 [rows, cols], scales uint8
    [rows, cols/32]); 2-D views with unit column stride (row pitches are taken from the views).  ``launch()``: one launch for all."""

    def __init__(self, jobs, device) -> None:
        arr = (_MhQuantMxJob * len(jobs))()
        items, self.keep = [], []
        for i, jb in enumerate(jobs):
            src, dst, sc = jb["src"], jb["dst"], jb["scales"]
            if src.dim() != 2 or src.dtype != torch.bfloat16 or dst.dtype != torch.uint8 or sc.dtype != torch.uint8:
                raise HipExtensionError("QuantMxBatch: bf16 [rows, cols] source, uint8 destination and scales expected")
            rows, cols = src.shape
            if tuple(dst.shape) != (rows, cols) or tuple(sc.shape) != (rows, cols // MX_BLOCK) or \
                    1 not in (src.stride(1), cols) or 1 not in (dst.stride(1), cols) or 1 not in (sc.stride(1), cols // MX_BLOCK):
                raise HipExtensionError("QuantMxBatch: dst [rows, cols] and scales [rows, cols / 32] with unit column stride")
            arr[i] = _MhQuantMxJob(src.data_ptr(), dst.data_ptr(), sc.data_ptr(), rows, cols, src.stride(0), dst.stride(0),
                                   sc.stride(0), 0)
            items += [(i << 32) | c for c in range(-(-(rows * cols) // MX_CHUNK))]
            self.keep += [src, dst, sc]
        self.host = arr
        self.n_jobs = len(jobs)
        self.table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(device)
        self.items = torch.tensor(items, dtype=torch.int64).to(device)
        self.n_items = len(items)

    def launch(self) -> None:
        _check(lib().mh_quant_mx_batched(ctypes.byref(self.host), _I(self.n_jobs), ptr(self.table), ptr(self.items),
                                         _I(self.n_items), stream()), "mh_quant_mx_batched")


def quant_mx(src: torch.Tensor, dst: torch.Tensor | None = None, scales: torch.Tensor | None = None):
    """MX quantisation of one bf16 [rows, cols] tensor (cols % 32 == 0) -> (e4m3 uint8 [rows, cols], E8M0 uint8 [rows, cols/32])."""
    rows, cols = src.shape
    dst = torch.empty(rows, cols, dtype=torch.uint8, device=src.device) if dst is None else dst
    if scales is None:
        scales = torch.empty(rows, -(-(cols // MX_BLOCK) // 4) * 4, dtype=torch.uint8, device=src.device)[:, : cols // MX_BLOCK]
    QuantMxBatch([dict(src=src, dst=dst, scales=scales)], src.device).launch()
    return dst, scales
