"""Host-side (init-time) helpers: positional tables, their pooling to a modality grid, structural-mask draws.

These run once at construction or once per step on the HOST (index/RNG logic); the per-token arithmetic of the
hot path lives in the HIP kernels.  References: ``maestro/layers/utils.py:103-125,176-198`` (tables) and
``maestro/ssl/mae.py:178-226`` (structural masks).  The second half restates the same draws on the counter-based generator of the
device mode (``mask_rng="device"``, include/maestro_hip.h) in numpy: the contract ``mh_mask_draw`` is tested against.
"""

from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F  # noqa: N812
from torch import Tensor


def posemb_sincos_2d(h: int, w: int, dim: int, date_dim: int, temperature: float = 10000.0) -> Tensor:
    """``[h, w, dim]`` table: sin/cos of x then y frequencies, zeros in the last ``date_dim`` channels."""
    if dim % 4 or date_dim % 4:
        raise ValueError(f"Invalid embedding dimensions {dim}, {date_dim}. Expected multiples of 4")
    n = (dim - date_dim) // 4
    omega = 1.0 / (temperature ** (torch.arange(n) / (n - 1)))
    ys, xs = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    ya, xa = ys[..., None] * omega, xs[..., None] * omega
    return torch.cat([xa.sin(), xa.cos(), ya.sin(), ya.cos(), torch.zeros(h, w, date_dim)], dim=-1).float()


def pool_pos_table(table: Tensor, grid: int) -> Tensor:
    """Constant per-modality positional rows ``[grid*grid, dim]`` (block mean, bilinear pre-resize if needed).

    The reference recomputes this every step; it only depends on the geometry, so it is built once.
    """
    G = table.shape[0]  # noqa: N806
    if G % grid:
        G = grid * round(G / float(grid))  # noqa: N806
        table = F.interpolate(table.permute(2, 0, 1)[None], (G, G), mode="bilinear")[0].permute(1, 2, 0)
    r = G // grid
    return table.reshape(grid, r, grid, r, -1).mean(dim=(1, 3)).reshape(grid * grid, -1).contiguous()


def draw_struct_masks(groups, mods, generator=None) -> dict[str, Tensor]:
    """Structural Bernoulli masks per group, ``{group: bool [Beff, L]}``, drawn on the HOST generator.

    ``groups``: list of ``GroupSpec``; ``mods``: dict of ``ModSpec`` (see maestro_amd/ssl/mae.py).  Draw order per
    rejection-loop iteration = modalities in ``dataset.inputs`` order, each: mod, bands, dates, loc (only the active
    ones) -- exactly the reference's order so that a fixed seed gives bit-identical masks on the CPU generator.
    """
    # The random numbers come from torch (the reference's generator and draw order); the boolean bookkeeping around them runs
    # in numpy: these arrays are a few KiB, and torch's reductions over them go through the intra-op thread pool -- with the
    # default pool of a many-core host inside a container that may schedule a fraction of those cores, ONE ``.all(dim=1)`` was
    # measured at 6 ms (12 ms per step: more than half of the GPU's step time, spent on the host before the first launch).
    pending = {g.name: np.ones(g.Beff, dtype=bool) for g in groups}
    out = {g.name: np.ones((g.Beff, g.L), dtype=bool) for g in groups}
    while any(p.any() for p in pending.values()):
        draw = {}
        for m in mods.values():
            if m.gi:                     # band-groups 1.. of a modality: drawn together with its group 0
                continue
            B, D, L, G = m.Beff, m.D, m.L, m.G  # noqa: N806
            mk = np.zeros((B, G, D, L), dtype=bool)
            if m.p_mod:
                mk = mk | (torch.rand((B, 1, 1, 1), generator=generator) < m.p_mod).numpy()
            if m.p_bands:
                mk = mk | (torch.rand((B, G, 1, 1), generator=generator) < m.p_bands).numpy()
            if m.p_dates:
                mk = mk | (torch.rand((B, 1, D, 1), generator=generator) < m.p_dates).numpy()
            if m.p_loc:
                mk = mk | (torch.rand((B, 1, 1, L), generator=generator) < m.p_loc).numpy()
            for gi in range(G):          # the specs of one modality are named <modality>#<g> when there are several
                draw[m.name if G == 1 else f"{m.src}#{gi}"] = mk[:, gi].reshape(B, D * L)
        for g in groups:
            new = np.concatenate([draw[m.name] for m in g.mods], axis=1)
            take = pending[g.name]
            out[g.name] = np.where(take[:, None], new, out[g.name])
            pending[g.name] = out[g.name].all(axis=1)
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in out.items()}


# ---------------------------------------------------------------------------------------------------- device-side draws
# The counter-based form of the draws above (include/maestro_hip.h, csrc/mask_rng.hip): Philox4x32-10, a draw is a pure
# function of (seed, step, stream, kind, global row, attempt, i).  What follows is the numpy restatement of that contract --
# the reference the kernel is tested against bit for bit, and what a user calls to know the masks of a step without a GPU.
MASK_NOISE, MASK_MOD, MASK_BANDS, MASK_DATES, MASK_LOC = range(5)     # MH_MASK_KIND_*
MASK_MAX_ATTEMPTS = 64                                                 # MH_MASK_MAX_ATTEMPTS
_M32 = 0xFFFFFFFF


def philox4x32(counter, key, rounds: int = 10):
    """Philox4x32 (Salmon et al., SC'11): ``counter`` = four broadcastable uint32 arrays, ``key`` = two ints -> four uint32 arrays."""
    c = [np.asarray(x).astype(np.uint64) & np.uint64(_M32) for x in np.broadcast_arrays(*counter)]
    k0, k1 = int(key[0]) & _M32, int(key[1]) & _M32
    m32 = np.uint64(_M32)
    for _ in range(rounds):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]          # 32 x 32 -> 64 bits: exact in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & m32]
        k0, k1 = (k0 + 0x9E3779B9) & _M32, (k1 + 0xBB67AE85) & _M32
    return [x.astype(np.uint32) for x in c]


def mask_uniform(seed: int, step: int, stream, kind: int, row, attempt, i) -> np.ndarray:
    """``U(seed, step, stream, kind, row, attempt, i)``: float32, 24 bits in [0, 1); ``stream``, ``row``, ``attempt`` and ``i``
    broadcast."""
    if not 0 <= int(step) <= _M32:
        raise ValueError(f"step {step} is not an unsigned 32-bit value")
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    i = np.asarray(i).astype(np.uint64)
    c3 = np.uint64(kind) | np.asarray(stream).astype(np.uint64) << np.uint64(4) | np.asarray(attempt).astype(np.uint64) << np.uint64(16)
    w = philox4x32((i >> np.uint64(2), np.asarray(row).astype(np.uint64), np.uint64(step), c3), (seed & _M32, seed >> 32))
    word = np.choose((i & np.uint64(3)).astype(np.intp), w)
    return (word >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def mask_streams(groups, mods) -> tuple[dict, dict]:
    """Stream ids of the draws: ``({reference draw group: id}, {modality (ModSpec.src): id})``, both in order of first appearance
    (engine order of the groups, ``dataset.inputs`` order of the modalities)."""
    noise, mod = {}, {}
    for g in groups:
        noise.setdefault(g.draw or g.name, len(noise))
    for m in mods.values():
        mod.setdefault(m.src or m.name, len(mod))
    return noise, mod


def _beff(spec, B: int) -> int:  # noqa: N803
    return B * spec.Dates // spec.D          # dates folded into the batch (D == 1): B * Dates sequences, else B


def check_device_mask_config(groups) -> None:
    """The counted rejection loop needs a chance to end: a group whose modalities are ALL dropped with probability 1 is refused
    (the host loop never ends there either)."""
    for g in groups:
        if g.mods and all(m.p_mod is not None and m.p_mod >= 1 for m in g.mods):
            raise ValueError(f"mask_rng='device': group {g.name!r} has p_mod >= 1 on all its modalities (every draw is all-masked)")


def mask_draw_jobs(groups, mods, B: int) -> list[dict]:  # noqa: N803
    """The job table of ``mh_mask_draw`` as plain dicts, one per group (``hip.MaskDraw`` adds the destination pointers)."""
    noise_id, mod_id = mask_streams(groups, mods)
    jobs = []
    for g in groups:
        beff = _beff(g.mods[0], B)
        D = g.mods[0].Dates  # noqa: N806
        folded = g.draw_G > 1
        segs = [dict(tok_off=m.tok_off, D=m.D, L=m.L, gi=m.gi, G=m.G, stream=mod_id[m.src or m.name],
                     p=tuple(float(p) if p else -1.0 for p in (m.p_mod, m.p_bands, m.p_dates, m.p_loc))) for m in g.mods]
        jobs.append(dict(name=g.name, Beff=beff, L=g.L, noise_stream=noise_id[g.draw or g.name], noise_rpb=beff * g.draw_G // B,
                         struct_rpb=beff // B, row_div=D if folded else 1, row_mul=g.draw_G * D if folded else 1,
                         row_add=g.draw_g * D if folded else 0, segs=segs))
    return jobs


def mask_draw_reference(groups, mods, B: int, seed: int, step: int, row_base: int = 0):  # noqa: N803
    """``(noise, struct)`` of one step as the device draws them, shaped like ``MAEEngine.draw_masks()``: ``noise[draw group]``
    float32 ``[Beff * draw_G, L]``, ``struct[group]`` bool ``[Beff, L]``.  ``draw_struct_masks`` with ``U`` in place of the
    generator: attempt ``a`` of the rejection loop draws with ``attempt = a``, a row keeps the first attempt that is not
    all-masked, and a row that is all-masked ``MASK_MAX_ATTEMPTS`` times is all-clear.  ``row_base``: global index of the first
    sample (``rank * batch_size``); a row's draws depend on its global index only, not on ``B``."""
    noise_id, mod_id = mask_streams(groups, mods)
    pending = {g.name: np.ones(_beff(g.mods[0], B), dtype=bool) for g in groups}
    out = {g.name: np.ones((_beff(g.mods[0], B), g.L), dtype=bool) for g in groups}
    for a in range(MASK_MAX_ATTEMPTS):
        if not any(p.any() for p in pending.values()):
            break
        draw = {}
        for m in mods.values():
            if m.gi:
                continue
            Bm, D, L, G = _beff(m, B), m.D, m.L, m.G  # noqa: N806
            row = (row_base * (Bm // B) + np.arange(Bm)).reshape(Bm, 1, 1, 1)
            st = mod_id[m.src or m.name]
            mk = np.zeros((Bm, G, D, L), dtype=bool)
            if m.p_mod:
                mk = mk | (mask_uniform(seed, step, st, MASK_MOD, row, a, 0) < np.float32(m.p_mod))
            if m.p_bands:
                mk = mk | (mask_uniform(seed, step, st, MASK_BANDS, row, a, np.arange(G).reshape(1, G, 1, 1)) < np.float32(m.p_bands))
            if m.p_dates:
                mk = mk | (mask_uniform(seed, step, st, MASK_DATES, row, a, np.arange(D).reshape(1, 1, D, 1)) < np.float32(m.p_dates))
            if m.p_loc:
                mk = mk | (mask_uniform(seed, step, st, MASK_LOC, row, a, np.arange(L).reshape(1, 1, 1, L)) < np.float32(m.p_loc))
            for gi in range(G):
                draw[m.name if G == 1 else f"{m.src}#{gi}"] = mk[:, gi].reshape(Bm, D * L)
        for g in groups:
            new = np.concatenate([draw[m.name] for m in g.mods], axis=1)
            out[g.name] = np.where(pending[g.name][:, None], new, out[g.name])
            pending[g.name] = out[g.name].all(axis=1)
    for g in groups:                         # the bound is exhausted: all-clear
        out[g.name][pending[g.name]] = False
    noise = {}
    for g in groups:
        key = g.draw or g.name
        if key not in noise:
            rows = _beff(g.mods[0], B) * g.draw_G
            row = (row_base * (rows // B) + np.arange(rows)).reshape(rows, 1)
            noise[key] = torch.from_numpy(mask_uniform(seed, step, noise_id[key], MASK_NOISE, row, 0, np.arange(g.L).reshape(1, g.L)))
    return noise, {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in out.items()}
