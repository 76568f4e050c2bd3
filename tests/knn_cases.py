"""Cases, wrong forms and derived error bounds for the nearest-neighbour kernels (include/maestro_hip.h), shared by
tests/test_knn_host.py (no GPU: the references' own teeth) and tests/test_knn_gpu.py (the kernels on the same cases).

Bounds (u = 2^-24, the unit roundoff of fp32; derived, not fitted):

* similarity: fp32 accumulation of exact bf16 products in any order: ``numerics.gemm_bound(|q| |bank|, E)``.
* normalisation ``y = x / max(sqrt(S), eps)``, ``S = sum x^2``: E fused multiply-adds and the butterfly's additions of positive
  terms give ``|S^ - S| <= E u S``; the square root halves that and adds its own rounding, the division adds one more:
  ``|y^ - y| <= (E / 2 + 3) u |y|`` (the 3 covers sqrt, division and the second-order terms), plus one denormal step.
* vote weight ``w = exp(t)``, ``t = (s - s0) inv_T``: the subtraction and the product are one rounding each, ``|t^ - t| <= 2 u |t|``,
  which the exponential amplifies to a relative ``2 u |t|``; the device's ``expf`` is documented at 1 ulp (<= 2 u relative) in the
  HIP math API; results below the smallest normal number may be flushed (2^-126 absolute).  A class score is a sequential sum
  of at most ``k_eval`` such weights: ``(k_eval - 1) u`` times the sum of the weights on top.
"""

from __future__ import annotations

import numpy as np
import torch

from maestro_amd import hip
from tests.numerics import gemm_bound

U = 2.0 ** -24
BANK_ORDERS = ("random", "ascending", "descending", "equal")


def int_operands(Nq, Nb, E, seed, order="random"):  # noqa: N803
    """Integer-valued bf16 operands with entries in {-2 .. 2}: every dot product is an exact fp32 integer and ties are plentiful.
    ``order``: the bank rows sorted by their similarity to query 0 ("ascending": every tile inserts; "descending": none after the
    list has filled), or all rows equal."""
    rng = np.random.default_rng(seed)
    q = rng.integers(-2, 3, size=(Nq, E)).astype(np.float32)
    bank = rng.integers(-2, 3, size=(Nb, E)).astype(np.float32)
    if order == "equal":
        bank[:] = bank[0]
    elif order != "random":
        s = bank @ q[0]
        bank = bank[np.argsort(s if order == "ascending" else -s, kind="stable")]
    return torch.from_numpy(q).to(torch.bfloat16), torch.from_numpy(np.ascontiguousarray(bank)).to(torch.bfloat16)


def tie_case():
    """A hand-made case: E = 32, one query of ones; bank similarities 3, 5, 5, 1, 5, 3 -> top-4 = rows 1, 2, 4 (5, ascending
    index) then row 0 (the first 3)."""
    q = torch.ones(1, 32)
    bank = torch.zeros(6, 32)
    for r, s in enumerate((3, 5, 5, 1, 5, 3)):
        bank[r, :s] = 1
    want_s = np.array([[5, 5, 5, 3]], dtype=np.float32)
    want_i = np.array([[1, 2, 4, 0]], dtype=np.int32)
    return q.to(torch.bfloat16), bank.to(torch.bfloat16), 4, want_s, want_i


def lists_equal(got, want) -> bool:
    """Bit for bit: sims (as int32 bit patterns) and idx."""
    gs, gi = (np.asarray(t.cpu() if isinstance(t, torch.Tensor) else t) for t in got)
    ws, wi = (np.asarray(t) for t in want)
    return bool(np.array_equal(gs.astype(np.float32).view(np.int32), ws.astype(np.float32).view(np.int32)) and np.array_equal(gi, wi))


def wrong_topk(form, q, bank, k, index_base=0):
    """Named wrong forms of the order rule, each rejected by ``lists_equal`` on a tied case."""
    s_all = hip.bf16_values(q) @ hip.bf16_values(bank).T
    Nq, Nb = s_all.shape  # noqa: N806
    out_s, out_i = np.full((Nq, k), -np.inf, np.float32), np.full((Nq, k), -1, np.int32)
    for n in range(Nq):
        idx = index_base + np.arange(Nb)
        if form == "larger_index_wins":
            order = np.lexsort((-idx, -s_all[n]))[:k]
        elif form == "unsorted":                       # the right set, in bank order
            order = np.sort(hip.knn_order(s_all[n], idx)[:k])
        else:
            raise ValueError(form)
        out_s[n, : len(order)], out_i[n, : len(order)] = s_all[n][order], idx[order]
    return out_s, out_i


TOPK_WRONG = ("larger_index_wins", "unsorted")


def sorted_under_rule(sims, idx) -> bool:
    """Every list is sorted under the order rule on its own values (unfilled slots last)."""
    sims, idx = np.asarray(sims, dtype=np.float64), np.asarray(idx, dtype=np.int64)
    key_i = np.where(idx < 0, np.iinfo(np.int64).max, idx)
    a_s, b_s, a_i, b_i = sims[:, :-1], sims[:, 1:], key_i[:, :-1], key_i[:, 1:]
    return bool(((a_s > b_s) | ((a_s == b_s) & (a_i <= b_i))).all())


# ------------------------------------------------------------------------------------------------ similarity
def sim_ref64(q, bank):
    """``(q bank^T, |q| |bank|^T)`` in fp64 from the bf16 values (numpy)."""
    q64, b64 = hip.bf16_values(q), hip.bf16_values(bank)
    return q64 @ b64.T, np.abs(q64) @ np.abs(b64).T


def sim_bound(absprod, E):  # noqa: N803
    return np.asarray(gemm_bound(torch.as_tensor(absprod), E))


def check_bounded_topk(sims, idx, s64, bound, index_base=0):
    """The three properties of the bounded test; returns the worst error-to-bound ratio of the returned similarities."""
    sims, idx = np.asarray(sims, dtype=np.float64), np.asarray(idx, dtype=np.int64) - index_base
    Nq, k = idx.shape  # noqa: N806
    assert (idx >= 0).all() and sorted_under_rule(sims, idx)
    rows = np.arange(Nq)[:, None]
    ref, b = s64[rows, idx], bound[rows, idx]
    err = np.abs(sims - ref)
    assert (err <= b).all(), float((err / np.maximum(b, 1e-300)).max())
    chosen = np.zeros_like(s64, dtype=bool)
    chosen[rows, idx] = True
    assert (chosen.sum(axis=1) == k).all(), "an index returned twice"
    lo_out = np.where(chosen, -np.inf, s64 - bound).max(axis=1)             # the best a row left out could be worth, at least
    hi_in = (ref + b).min(axis=1)
    assert (lo_out <= hi_in).all(), "a row left out beats a returned one beyond both error bounds"
    return float((err / np.maximum(b, 1e-300)).max())


# ------------------------------------------------------------------------------------------------ normalisation
def norm_inputs(E, seed):  # noqa: N803
    """Rows of scale 1, 1e-3 and 1e3, a zero row, a row below eps (1e-20) and a one-hot row."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(9, E, generator=g)
    x[1] *= 1e-3
    x[2] *= 1e3
    x[3] = 0
    x[4] = 1e-20 * torch.sign(x[4])
    x[5] = 0
    x[5, E // 2] = -3.0
    return x


def norm_ref64(x, eps=1e-12, eps_rule=True):
    x64 = np.asarray(x, dtype=np.float64)
    n = np.sqrt((x64 * x64).sum(axis=1, keepdims=True))
    d = np.maximum(n, eps) if eps_rule else n
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(d > 0, x64 / np.where(d > 0, d, 1), 0.0)


def norm_bound(y64, E):  # noqa: N803
    return (E / 2 + 3) * U * np.abs(y64) + 2.0 ** -149


def norm_f32(x, eps=1e-12):
    """An honest fp32 restatement in ANOTHER order than the kernel's (numpy's pairwise sum): inside the bound all the same."""
    x = np.asarray(x, dtype=np.float32)
    d = np.maximum(np.sqrt((x * x).sum(axis=1, keepdims=True, dtype=np.float32)), np.float32(eps))
    return np.where(d > 0, x / np.where(d > 0, d, np.float32(1)), np.float32(0)).astype(np.float32)


def bf16_rne(y32):
    """Round-to-nearest-even bf16 bits (uint16) of fp32 values (finite inputs)."""
    b = np.asarray(y32, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)


# ------------------------------------------------------------------------------------------------ vote
def vote_case(Nq, k, C, n_labels, seed, scale=1.0, spread=0.1):  # noqa: N803
    """Sorted cosine-like similarity lists in ``scale * [1 - spread, 1]`` (neighbours are close to each other: at T = 0.01 the last
    of them still weighs in) with -1 slots at some tails, indices that reach past ``n_labels``, labels with missing (-1) and
    out-of-range entries."""
    rng = np.random.default_rng(seed)
    sims = -np.sort(-(1 - spread * rng.random((Nq, k))).astype(np.float32) * np.float32(scale), axis=1)
    idx = rng.integers(0, n_labels + 3, size=(Nq, k)).astype(np.int32)             # (a few >= n_labels: they add nothing)
    for n in range(0, Nq, 3):                                                        # unfilled tails
        cut = int(rng.integers(1, k + 1))
        sims[n, cut:], idx[n, cut:] = -np.inf, -1
    labels = rng.integers(0, C, size=n_labels).astype(np.int32)
    labels[::5] = -1                                                                 # missing_val
    labels[1::7] = C + 2                                                             # outside [0, C)
    return sims, idx, labels


def vote_bound(sims, idx, labels, C, T, k_eval, missing_val=-1):  # noqa: N803
    """``(scores64, bound)`` per the module docstring, from the fp32 similarities and the fp32 ``inv_T`` the kernel is handed."""
    sims, idx = np.asarray(sims, dtype=np.float32), np.asarray(idx, dtype=np.int64)
    inv_t = np.float64(np.float32(1.0 / T))
    Nq, k = sims.shape  # noqa: N806
    s64, bound = np.zeros((Nq, C)), np.zeros((Nq, C))
    for n in range(Nq):
        tot = 0.0
        for j in range(k_eval):
            i = idx[n, j]
            if not 0 <= i < len(labels) or labels[i] == missing_val or not 0 <= labels[i] < C:
                continue
            t = (np.float64(sims[n, j]) - np.float64(sims[n, 0])) * inv_t
            w = 1.0 if sims[n, j] == sims[n, 0] else float(np.exp(t))
            s64[n, labels[i]] += w
            bound[n, labels[i]] += w * (2 * abs(t) + 2) * U * 1.001 + 2.0 ** -126
            tot += w
        bound[n] += (k_eval - 1) * U * tot
    return s64, bound


def wrong_vote(form, sims, idx, labels, C, T, k_eval, missing_val=-1):  # noqa: N803
    """Named wrong forms of the vote, each rejected by the bound (or by exact equality on integer counts)."""
    sims = np.asarray(sims, dtype=np.float32)
    if form == "k_not_k_eval":
        return hip.knn_vote_reference(sims, idx, labels, C, T, None, missing_val)[0]
    if form == "missing_counted":
        lab = np.where(np.asarray(labels) == missing_val, 0, labels)
        return hip.knn_vote_reference(sims, idx, lab, C, T, k_eval, missing_val)[0]
    if form == "no_shift":                             # exp(sim / T) itself: overflows fp32 at T = 0.01
        scores = np.zeros((sims.shape[0], C), dtype=np.float32)
        with np.errstate(over="ignore", invalid="ignore"):
            w = np.exp((sims * np.float32(1.0 / T)).astype(np.float64)).astype(np.float32)
        for n in range(sims.shape[0]):
            for j in range(k_eval):
                i = idx[n, j]
                if 0 <= i < len(labels) and labels[i] != missing_val and 0 <= labels[i] < C:
                    scores[n, labels[i]] = np.float32(scores[n, labels[i]] + w[n, j])
        return scores
    raise ValueError(form)


VOTE_WRONG = ("k_not_k_eval", "missing_counted", "no_shift")


def argmax_rule(scores, voted):
    """The lowest class among equal maxima, -1 where nothing voted."""
    return np.where(voted, np.argmax(np.asarray(scores), axis=1), -1).astype(np.int32)
