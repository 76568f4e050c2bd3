"""Shared by tests/test_grad_guard_host.py and tests/test_grad_guard_gpu.py (a plain helper module): the sizes, the inputs, the
fp32 emulation of the addition tree of ``mh_grad_sumsq_partial`` and the error bound derived from that tree.

THE TREE (include/maestro_hip.h).  A chunk is C = MH_GUARD_CHUNK = 16384 elements for one workgroup of 256 lanes; lane l
holds four accumulators acc[c], c = 0 ... 3, and for k = 0 ... 15 in order does acc[c] = fma(g, g, acc[c]) with g = element
4 * (256 * k + l) + c of the chunk (elements past n count as +0).  Then (acc[0] + acc[1]) + (acc[2] + acc[3]); then six
butterfly steps over the 64 lanes of a wave (v += v[lane ^ o], o = 32, 16, ... 1); then ((w0 + w1) + w2) + w3 over the four waves.

THE BOUND.  Every term is >= 0, so each fp32 operation on a partial sum multiplies it by (1 + d), |d| <= u = 2^-24, and an
element's square reaches the result through at most
    1 (its square, had it been rounded on its own; the fma folds it into the first addition)
  + 16 (the lane's accumulations) + 2 (the lane's four accumulators) + 6 (butterfly) + 3 (waves)            = D = 28
roundings.  Hence |partial - exact| <= gamma_D * exact with gamma_D = D u / (1 - D u) (Higham, Accuracy and Stability of Numerical
Algorithms, lemma 3.1), for a whole or a ragged chunk alike.  The finish kernel adds the rows in double (rows * 2^-53, nothing),
the square root halves the relative error, |grad_scale| * sqrt(S) costs two double roundings and the result is rounded to float
once: |norm - exact| <= (gamma_D / 2 + u + 2^-50) * exact.  Underflow: the inputs of the bounded tests keep every square in the
normal range (``normal_draws`` clamps |x| >= 2^-10 before scaling).
"""

from __future__ import annotations

import numpy as np

C = 16384                       # MH_GUARD_CHUNK (tests/test_grad_guard_host.py checks it against the header)
LANES, QUADS = 256, C // (4 * 256)
U = 2.0 ** -24
DEPTH = 1 + QUADS + 2 + 6 + 3
GAMMA = DEPTH * U / (1 - DEPTH * U)
NORM_BOUND = GAMMA / 2 + U + 2.0 ** -50

SIZES = (4, 8, C - 4, C, C + 4, 3 * C + 260, 257 * C + 12)
SCALES = (2.0 ** -40, 1.0, 2.0 ** 50)


def rows_of(n: int) -> int:
    return -(-n // C)


def integer_gradient(n: int, seed: int = 0) -> np.ndarray:
    """Integer values in [-8, 8]: a chunk's sum of squares is <= 2^20, exact in fp32 in any order."""
    return np.random.default_rng(seed).integers(-8, 9, size=n).astype(np.float32)


def normal_draws(n: int, scale: float, seed: int = 1) -> np.ndarray:
    x = np.random.default_rng(seed).standard_normal(n)
    x = np.where(np.abs(x) < 2.0 ** -10, 2.0 ** -10, x)
    return (x * scale).astype(np.float32)


def exact_partials(g: np.ndarray) -> np.ndarray:
    """Per-chunk sums of squares in int64 (integer inputs) -- exact."""
    pad = np.zeros(rows_of(g.size) * C, dtype=np.int64)
    pad[: g.size] = g.astype(np.int64) ** 2
    return pad.reshape(-1, C).sum(axis=1)


def emulate_partials(g: np.ndarray, mutation: str | None = None) -> np.ndarray:
    """The kernel's addition tree in numpy fp32, chunk by chunk.  ``mutation``: None, "drop_lane" (one lane's sum never reaches
    the wave reduction) or "bf16_squares" (every square is rounded to bf16 before it is accumulated)."""
    f32, f64 = np.float32, np.float64
    rows = rows_of(g.size)
    pad = np.zeros(rows * C, dtype=f32)
    pad[: g.size] = g
    x = pad.reshape(rows, QUADS, LANES, 4)                      # element 4 * (256 * k + l) + c of the chunk
    acc = np.zeros((rows, LANES, 4), dtype=f32)
    for k in range(QUADS):
        sq = x[:, k].astype(f64) ** 2                            # exact: 48 bits
        if mutation == "bf16_squares":
            bits = sq.astype(f32).view(np.uint32).astype(np.uint64)
            bits = ((bits + 0x7FFF + ((bits >> 16) & 1)) >> 16) << 16
            sq = bits.astype(np.uint32).view(f32).astype(f64)
        acc = (acc.astype(f64) + sq).astype(f32)                 # fma: one rounding
    v = (acc[..., 0] + acc[..., 1]) + (acc[..., 2] + acc[..., 3])
    if mutation == "drop_lane":
        v[:, 2 * 64 + 17] = 0
    v = v.reshape(rows, 4, 64)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, :, lane ^ o]
    w = v[:, :, 0]
    return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def partial_error_ratio(got: np.ndarray, g: np.ndarray) -> float:
    """max over the chunks of |got - exact| / (GAMMA * exact), exact in fp64 (its own error, 2^-53 * 14 levels, is nothing)."""
    pad = np.zeros(rows_of(g.size) * C, dtype=np.float64)
    pad[: g.size] = g.astype(np.float64) ** 2
    exact = pad.reshape(-1, C).sum(axis=1)
    return float(np.max(np.abs(got.astype(np.float64) - exact) / (GAMMA * exact)))
