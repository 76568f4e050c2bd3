"""Integer-valued operands for the step-end kernels: sums that every summation order gets right to the last bit.

The masked loss, the column sums and the mask-token gradient add their terms in an order the hardware chooses (atomics, wave
shuffles, LDS trees), so a random-valued test can only hold them to a bound that grows with the number of terms.  If every term
is an integer multiple of one power of two ``unit`` and ``sum |terms| < 2^24 unit``, every partial sum of every order is such
a multiple below ``2^24 unit`` too, hence exactly representable in fp32: no addition ever rounds, and the kernel must equal the
fp64 (or int64) value bit for bit.  One dropped, doubled or misplaced row is then a failure of any size.

``is_order_free`` asserts that condition; every GPU test calls it on its own inputs.  The generators build on any device with
torch ops.  tests/test_step_end_selfcheck.py checks both on the CPU; tests/test_step_end_exact_gpu.py uses them.
"""

from __future__ import annotations

import math

import torch

F32_INTS = 2.0 ** 24        # integers below this magnitude are exact in fp32
DIFF_UNIT = 0.25            # rec, target and their difference are multiples of this
DIFF_MAX = 7                # |diff| <= DIFF_MAX * DIFF_UNIT: diff^2 = k^2 / 16 with k^2 <= 49
INT_MAX = 255               # integer rows: every one of the eight bf16 significand bits is used


def is_power_of_two(x: float) -> bool:
    return x > 0 and math.frexp(x)[0] == 0.5


def is_order_free(terms: torch.Tensor, unit: float, dim=None) -> bool:
    """Asserts that ``terms`` summed over ``dim`` (None: all of it) give the same fp32 bits in every order: ``unit`` is a power
    of two, every term is an integer multiple of it, and ``sum |terms| < 2^24 unit``.  Returns True (for use in ``assert``)."""
    assert is_power_of_two(unit), f"unit {unit} is not a power of two"
    q = terms.double() / unit
    assert bool((q == q.round()).all()), f"a term is not a multiple of {unit}"
    total = q.abs().sum() if dim is None else q.abs().sum(dim).max()
    assert float(total) < F32_INTS, f"sum |terms| = {float(total)} units of {unit}: not below 2^24"
    return True


def _gen(device, seed: int) -> torch.Generator:
    return torch.Generator(device=device).manual_seed(seed)


def int_rows(rows: int, cols: int, device="cpu", seed: int = 0, ld=None, dtype=torch.float32, pad=float("nan")):
    """``[rows, cols]`` integers in [-INT_MAX, INT_MAX] as ``dtype`` (exact in bf16 and fp32), a view into a ``[rows, ld]`` buffer
    whose pad columns hold ``pad``; returns ``(view, int64 copy)``."""
    k = torch.randint(-INT_MAX, INT_MAX + 1, (rows, cols), device=device, generator=_gen(device, 7919 * seed + 31 * rows + cols))
    ld = cols if ld is None else ld
    buf = torch.full((rows, ld), pad, dtype=dtype, device=device)
    buf[:, :cols] = k.to(dtype)
    return buf[:, :cols], k


def int_vector(n: int, device="cpu", seed: int = 0):
    """Integer preload of an accumulated destination: ``(fp32 [n], int64 [n])``."""
    k = torch.randint(-INT_MAX, INT_MAX + 1, (n,), device=device, generator=_gen(device, 104729 * seed + n))
    return k.float(), k


def loss_operands(rows: int, ppc: int, device="cpu", seed: int = 0, window=None):
    """``rec`` fp32 [rows, ppc], ``target`` fp32 [rows, tgt_ld] and the int64 ``k`` [rows, ppc] with ``rec - target = k / 4`` on the
    columns the loss pairs, ``|k| <= 7``, about one ``k`` in eight zero.  ``window`` = (tgt_C, tgt_c0, n_g): the band window of the
    ``_bands`` entries -- rec column ``pix * n_g + c`` pairs with target column ``pix * tgt_C + tgt_c0 + c``."""
    g = _gen(device, 2654435 * seed + 131 * rows + ppc)
    k = torch.randint(-DIFF_MAX, DIFF_MAX + 1, (rows, ppc), device=device, generator=g)
    k = torch.where(torch.randint(0, 8, (rows, ppc), device=device, generator=g) == 0, torch.zeros_like(k), k)
    if window is None:
        t = torch.randint(-32, 33, (rows, ppc), device=device, generator=g)
        paired = t
    else:
        tgt_c, c0, n_g = window
        assert ppc % n_g == 0 and 0 <= c0 and c0 + n_g <= tgt_c
        t = torch.randint(-32, 33, (rows, ppc // n_g, tgt_c), device=device, generator=g)
        paired = t[:, :, c0: c0 + n_g].reshape(rows, ppc)
        t = t.reshape(rows, -1)
    rec = (paired + k).float() * DIFF_UNIT
    target = t.float() * DIFF_UNIT
    return rec.contiguous(), target.contiguous(), k


def token_mask(B: int, Lgroup: int, tok_off: int, Lm: int, n_sel: int, device="cpu", seed: int = 0):  # noqa: N803
    """uint8 [B, Lgroup] with exactly ``n_sel`` ones inside the window ``[tok_off, tok_off + Lm)`` (random places, the first and
    the last token of the window among them) and ones everywhere outside it; returns ``(mask, bool selection [B * Lm])``."""
    assert 2 <= n_sel <= B * Lm and tok_off + Lm <= Lgroup
    perm = torch.randperm(B * Lm - 2, device=device, generator=_gen(device, 15485863 * seed + B * Lm + n_sel)) + 1
    sel = torch.zeros(B * Lm, dtype=torch.bool, device=device)
    sel[perm[: n_sel - 2]] = True
    sel[0] = sel[-1] = True
    mask = torch.ones(B, Lgroup, dtype=torch.uint8, device=device)
    mask[:, tok_off: tok_off + Lm] = sel.view(B, Lm).to(torch.uint8)
    return mask, sel


def loss_terms(k: torch.Tensor, sel: torch.Tensor, p: int):
    """The loss's addends before ``coef`` as ``(fp64 terms [rows, ppc], unit)``: ``|k| / 4`` (p = 1) or ``k^2 / 16`` (p = 2) on the
    selected rows, 0 elsewhere."""
    kk = torch.where(sel[:, None], k, torch.zeros_like(k))
    if p == 1:
        return kk.abs().double() * DIFF_UNIT, DIFF_UNIT
    return (kk * kk).double() * DIFF_UNIT ** 2, DIFF_UNIT ** 2


def drec_values(k: torch.Tensor, sel: torch.Tensor, p: int, coef: float):
    """d loss / d rec as ``(fp64 [rows, ppc], unit)``: ``2 (k / 4) coef`` (p = 2) or ``sign(k) coef`` (p = 1, 0 at ``k == 0`` as
    torch's L1 gradient) on the selected rows, 0 on the visible ones.  Exact in bf16 for a power-of-two ``coef``: |k| <= 7 is three
    bits."""
    assert is_power_of_two(coef)
    kk = torch.where(sel[:, None], k, torch.zeros_like(k))
    if p == 1:
        return kk.sign().double() * coef, coef
    return kk.double() * (0.5 * coef), 0.5 * coef


def block_sums(x: torch.Tensor, rows_per_block: int) -> torch.Tensor:
    """``[ceil(rows / rows_per_block), ...]``: block i sums rows ``[i rows_per_block, (i + 1) rows_per_block)`` of ``x``."""
    rows = x.shape[0]
    n = -(-rows // rows_per_block)
    if n * rows_per_block != rows:
        x = torch.cat([x, x.new_zeros((n * rows_per_block - rows,) + tuple(x.shape[1:]))])
    return x.reshape((n, rows_per_block) + tuple(x.shape[1:])).sum(1)


# ------------------------------------------------------------------------------------------------ the self-check's view
def _selfcheck_loss(p: int, seed: int, window=None):
    rows, ppc = 24, 20
    _, _, k = loss_operands(rows, ppc, seed=seed, window=window)
    _, sel = token_mask(3, 13, 2, 8, 16, seed=seed)
    return loss_terms(k, sel, p)


def _selfcheck_drec(p: int, seed: int):
    _, _, k = loss_operands(24, 20, seed=seed)
    _, sel = token_mask(3, 13, 2, 8, 16, seed=seed)
    return drec_values(k, sel, p, 2.0 ** -9)


# name -> fn(seed) -> (terms [rows, cols] whose rows are summed, unit): one entry per generator and per form of its terms
GENERATORS = {
    "int_rows_f32": lambda seed: (int_rows(300, 12, seed=seed)[0].double(), 1.0),
    "int_rows_bf16": lambda seed: (int_rows(300, 12, seed=seed, dtype=torch.bfloat16, ld=20)[0].double(), 1.0),
    "int_vector": lambda seed: (int_vector(300, seed=seed)[0].double()[:, None], 1.0),
    "loss_p1": lambda seed: _selfcheck_loss(1, seed),
    "loss_p2": lambda seed: _selfcheck_loss(2, seed),
    "loss_p2_bands": lambda seed: _selfcheck_loss(2, seed, window=(5, 2, 2)),
    "drec_p1": lambda seed: _selfcheck_drec(1, seed),
    "drec_p2": lambda seed: _selfcheck_drec(2, seed),
    "token_mask": lambda seed: (token_mask(3, 13, 2, 8, 16, seed=seed)[0].double(), 1.0),
}
