"""Input staging for the MI355X path: host batch -> pinned memory -> asynchronous H2D on a copy stream
-> the dataset's flips / transposes on the GPU (``maestro/dataset/dataset.py:224-257``; the raster resize to ``image_size``
and the elevation rescale of ``maestro/ssl/mim.py:425-437`` happen inside the engine).

The reference augments each sample on the CPU inside ``__getitem__``; here the loader hands over un-augmented samples and
the three per-sample booleans are drawn on the host in the reference's order (``rng.choice([True, False])`` x 3 per
sample), so that with the same generator state the staged batch is bit-identical to the reference's.

Median-date selection (``maestro/dataset/dataset.py:188-220``) moves the same way: for a modality named in ``select`` the loader
hands over the RAW window of dates it has read (padded to a common ``Tmax``), the per-sample window plan (``window_plan``: the
start offset the reference draws at ``dataset.py:92-95``, and ``W = T // num_dates``) and, when the dataset has one, the cloud
mask; ``BatchStager.stage`` picks one date per window on the GPU (``hip.select_dates``), before the flips.  ``random_dates``
keeps its draws on the host in the reference's order (``draw_date_scores``).
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np
import torch

from .. import hip


@dataclass(frozen=True)
class DateSelect:
    """How one modality picks its dates: the four fields of ``conf.datasets.RasterConfig`` that ``preprocess_raster`` reads."""
    num_dates: int
    mask_threshold: float = 0.0
    log_scale: bool = False
    norm_fac: float | None = None

    @classmethod
    def from_config(cls, input_cfg) -> "DateSelect":
        return cls(num_dates=int(input_cfg.num_dates), mask_threshold=float(input_cfg.mask_threshold),
                   log_scale=bool(input_cfg.log_scale), norm_fac=None if input_cfg.norm_fac is None else float(input_cfg.norm_fac))

    @property
    def use_mask(self) -> bool:
        """``dataset.py:152``: a threshold of 100 % (or more) masks nothing, the mask is not read at all."""
        return (self.mask_threshold / 100.0) < 1.0

    @property
    def mask_floor(self) -> int:
        """Mask values are integers: ``m > mask_threshold``  <=>  ``m > floor(mask_threshold)``."""
        return int(math.floor(self.mask_threshold))


def window_plan(n_dates, num_dates: int, start) -> tuple[torch.Tensor, torch.Tensor]:
    """The windows of ``dataset.py:92-104``: a sample with ``T`` raw dates keeps dates ``start ... start + num_dates * (T //
    num_dates) - 1`` and cuts them into ``num_dates`` windows of ``W = T // num_dates``; ``start`` is the reference's draw
    ``rng.integers(0, T % num_dates + 1)`` (made by the caller, in the reference's order).  ``n_dates`` and ``start`` are
    per-sample sequences (or scalars); returns int32 ``(t_start [B], t_win [B])`` host tensors."""
    T = np.atleast_1d(np.asarray(n_dates, dtype=np.int64))  # noqa: N806
    s = np.broadcast_to(np.atleast_1d(np.asarray(start, dtype=np.int64)), T.shape)
    nd = int(num_dates)
    if nd < 1 or (T < nd).any():
        raise ValueError(f"window_plan: {nd} dates out of {T.tolist()} raw dates")
    if (s < 0).any() or (s > T % nd).any():
        raise ValueError(f"window_plan: start {s.tolist()} outside 0 ... T % num_dates = {(T % nd).tolist()}")
    return torch.from_numpy(s.astype(np.int32)), torch.from_numpy((T // nd).astype(np.int32))


def draw_date_scores(rng: np.random.Generator, nd: int, W: int, C: int, S: int, dtype) -> np.ndarray:  # noqa: N803
    """The per-date scores of ``random_dates`` (``dataset.py:204-208``) for one sample of one modality: the reference draws
    ``rng.random([nd, W, C, S, S])``, casts it to the dtype of its deviations -- float64 for integer raw data, the raw dtype for
    floats -- and takes ``mean(axis=(2, 3, 4))``.  Returns float64 ``[nd, W]`` (a float32 mean widened: the same order).

    The mean's rounding depends on the memory order numpy sums in.  Every reader of the reference ends with the band selection
    ``input_mod[:, bands]`` (``dataset.py:166, 175, 181``), an advanced index whose result numpy lays out with the band axis
    outermost; the window reshape and the elementwise steps that follow keep that layout, so the reference's deviations lie in
    memory as ``[C, nd, W, S, S]``.  The draw is put into the same layout before the mean."""
    dt = np.dtype(dtype)
    dt = dt if dt.kind == "f" else np.dtype(np.float64)
    laid = np.empty((C, nd, W, S, S), dtype=dt).transpose(1, 2, 0, 3, 4)
    laid[...] = rng.random((nd, W, C, S, S)).astype(dt)
    return laid.mean(axis=(2, 3, 4)).astype(np.float64)


def draw_transform_flags(rng: np.random.Generator, batch_size: int, use_transform: bool = True) -> torch.Tensor:
    """uint8 [B]: bit0 = flip axis 2 (rows), bit1 = flip axis 3 (columns), bit2 = swap axes 2 and 3."""
    flags = np.zeros(batch_size, dtype=np.uint8)
    if use_transform:
        for b in range(batch_size):
            for bit in range(3):
                if rng.choice([True, False]):
                    flags[b] |= 1 << bit
    return torch.from_numpy(flags)


class BatchStager:
    """Double-buffered pinned staging: ``stage(batch)`` returns GPU tensors whose copies (and augmentation) run on a private
    stream; the caller's stream waits for them, the host never blocks except when it laps the ring."""

    def __init__(self, device, rasters: list[str], depth: int = 2) -> None:
        device = torch.device(device)
        if device.type != "cuda":
            raise hip.HipExtensionError("BatchStager needs a GPU device")
        hip.lib()
        self.device, self.rasters, self.depth = device, list(rasters), depth
        self.stream = torch.cuda.Stream(device=device)
        self._pinned = [dict() for _ in range(depth)]   # the stager's own pinned buffers, per ring slot
        self._held = [dict() for _ in range(depth)]     # loader-owned pinned tensors kept alive until their copy is done
        self._done = [None] * depth
        self._n = 0

    def _pin(self, slot: int, key: str, t: torch.Tensor) -> torch.Tensor:
        if t.is_pinned():      # a DataLoader(pin_memory=True) batch: copy straight from it, keep it alive with the slot
            self._held[slot][key] = t
            return t
        self._held[slot].pop(key, None)
        buf = self._pinned[slot].get(key)
        if buf is None or buf.shape != t.shape or buf.dtype != t.dtype:
            buf = self._pinned[slot][key] = torch.empty(t.shape, dtype=t.dtype).pin_memory()
        buf.copy_(t)
        return buf

    def _h2d(self, slot: int, key: str, t: torch.Tensor) -> torch.Tensor:
        if t.dtype == torch.uint16:             # moved as its bytes
            return self._pin(slot, key, t.contiguous().view(torch.int16)).to(self.device, non_blocking=True).view(torch.uint16)
        return self._pin(slot, key, t.contiguous()).to(self.device, non_blocking=True)

    def _select(self, slot: int, batch: dict, name: str, sel: DateSelect) -> tuple[torch.Tensor, torch.Tensor]:
        """Raw dates of modality ``name`` -> ``(raster [B, nd, C, S, S] f32, dates [B, nd, 3])`` on the stager's stream."""
        for key in (name, f"{name}_dates", f"{name}_t_start", f"{name}_t_win"):
            if not isinstance(batch.get(key), torch.Tensor):
                raise hip.HipExtensionError(f"BatchStager: date selection of {name!r} needs the host tensor {key!r}")
        t_start, t_win = batch[f"{name}_t_start"].to(torch.int32), batch[f"{name}_t_win"].to(torch.int32)
        mask = batch.get(f"{name}_mask") if sel.use_mask else None
        scores = batch.get(f"{name}_scores")
        raster, dates, _ = hip.select_dates(
            self._h2d(slot, name, batch[name]), self._h2d(slot, f"{name}_dates", batch[f"{name}_dates"]), t_start, t_win,
            sel.num_dates, mask=None if mask is None else self._h2d(slot, f"{name}_mask", mask), mask_floor=sel.mask_floor,
            scores=None if scores is None else self._h2d(slot, f"{name}_scores", scores.to(torch.float64)),
            log_scale=sel.log_scale, norm_fac=sel.norm_fac, t_start_dev=self._h2d(slot, f"{name}_t_start", t_start),
            t_win_dev=self._h2d(slot, f"{name}_t_win", t_win))
        return raster, dates

    def stage(self, batch: dict, flags: torch.Tensor | None = None, select: dict | None = None) -> dict:
        """``batch``: host tensors in the wire format (rasters ``[B, D, C, S, S]``, dates int16, targets).  ``flags``
        (uint8 [B], see ``draw_transform_flags``) applies the per-sample flips / transposes to every raster in
        ``self.rasters`` on the GPU; None = no augmentation.

        ``select`` (name -> ``DateSelect``): for these modalities the batch carries the RAW dates instead -- ``name``
        ``[B, Tmax, C, S, S]`` (uint8 / int16 / uint16 / float32), ``f"{name}_dates"`` ``[B, Tmax, 3]``, the window plan
        ``f"{name}_t_start"`` / ``f"{name}_t_win"`` (``window_plan``) and optionally ``f"{name}_mask"`` (uint8 ``[B, Tmax, Cm, S,
        S]``) and ``f"{name}_scores"`` (float64 ``[B, Tmax]``, ``draw_date_scores`` laid at the windows' dates).  One date per
        window is picked on the GPU, before the flips; the staged batch holds ``name`` ``[B, nd, C, S, S]`` float32 and its
        ``[B, nd, 3]`` dates, without the helper keys.  None = no selection."""
        slot = self._n % self.depth
        self._n += 1
        if self._done[slot] is not None:
            self._done[slot].synchronize()      # the copies that last read this slot's pinned buffers
        out = {}
        picked, helpers = {}, set()
        with torch.cuda.stream(self.stream):
            dflags = None
            if flags is not None:
                dflags = self._pin(slot, "__flags__", flags.to(torch.uint8)).to(self.device, non_blocking=True)
            for name, sel in (select or {}).items():
                picked[name], picked[f"{name}_dates"] = self._select(slot, batch, name, sel)
                helpers.update(f"{name}_{k}" for k in ("t_start", "t_win", "mask", "scores"))
            for key, t in batch.items():
                if key in helpers:
                    continue
                if key in picked:
                    dev = picked[key]
                    if dflags is not None and key in self.rasters:
                        aug = torch.empty_like(dev)
                        hip.dihedral(dev, aug, dflags)
                        dev = aug
                    out[key] = dev
                    continue
                if not isinstance(t, torch.Tensor):
                    out[key] = t
                    continue
                dev = self._pin(slot, key, t.contiguous()).to(self.device, non_blocking=True)
                if dflags is not None and key in self.rasters:
                    aug = torch.empty_like(dev)
                    hip.dihedral(dev, aug, dflags)
                    dev = aug
                out[key] = dev
            ev = torch.cuda.Event()
            ev.record(self.stream)
        self._done[slot] = ev
        torch.cuda.current_stream().wait_event(ev)
        for t in out.values():
            if isinstance(t, torch.Tensor):
                t.record_stream(torch.cuda.current_stream())
        return out
