"""Numpy restatements of the median-date selection for the tests (a plain helper module: no tests, no fixtures).

Written from the rule in include/maestro_hip.h, one sample at a time:

(a) ``select_reference``: the reference's form -- masked pixels become NaN, ``nanmedian`` over the window, ``mean`` of the
    absolute deviations over the raster, ``nanargmin`` over the window.
(b) ``select_device``: the device's form -- per element the two middle values of the unmasked dates from a sort; integers:
    ``|2x - (a + b)|`` summed in int64; float32: ``|x - (a + b) / 2|`` in float32, added one element after the other in float64;
    dirty dates are out, the lowest score wins, the first index among equals.

Both return ``(index [nd], raster [nd, C, S, S] float32, dates [nd, 3], chosen [nd, C, S, S] in the raw dtype)``; the raster
has numpy's float32 ``log`` and ``/ norm_fac`` applied, ``chosen`` is the picked raw data (for fp64 comparisons of the log).
"""

from __future__ import annotations

import numpy as np


def _windows(raw, mask, dates, scores, t_start, W, nd):  # noqa: N803
    sl = slice(t_start, t_start + nd * W)
    win = raw[sl].reshape(nd, W, *raw.shape[1:])
    mwin = None if mask is None else mask[sl].reshape(nd, W, *mask.shape[1:])
    swin = None if scores is None else np.asarray(scores, dtype=np.float64)[sl].reshape(nd, W)
    return win, mwin, dates[sl].reshape(nd, W, 3), swin


def _finish(win, dwin, idx, log_scale, norm_fac):
    nd = win.shape[0]
    chosen = win[np.arange(nd), idx]
    out = chosen.astype(np.float32)
    if log_scale:
        out = np.log(np.maximum(out, np.float32(1e-10)))
    if norm_fac is not None:
        out = out / np.float32(norm_fac)
    assert out.dtype == np.float32
    return idx.astype(np.int32), out, dwin[np.arange(nd), idx], chosen


def select_reference(raw, dates, t_start, W, nd, mask=None, mask_threshold=0.0, scores=None, log_scale=False, norm_fac=None):  # noqa: N803
    """Form (a).  ``raw`` [T, C, S, S], ``mask`` [T, Cm, S, S] or None, ``dates`` [T, 3], ``scores`` [T] or None."""
    win, mwin, dwin, swin = _windows(raw, mask, dates, scores, t_start, W, nd)
    x = win
    if mwin is not None:
        m = (mwin > mask_threshold).any(axis=2, keepdims=True)                     # [nd, W, 1, S, S]
        every_date_dirty = m.any(axis=(2, 3, 4), keepdims=True).all(axis=1, keepdims=True)
        m = m & ~every_date_dirty
        x = np.where(m, np.nan, win)
    score = np.abs(x - np.nanmedian(x, axis=1, keepdims=True)).mean(axis=(2, 3, 4))       # NaN for a date with a masked pixel
    if swin is not None:
        score = np.where(np.isnan(score), np.nan, swin)                            # random_dates: "0 * dev" keeps the NaNs
    idx = np.nanargmin(score, axis=1)
    return _finish(win, dwin, idx, log_scale, norm_fac)


def device_scores(vals, valid):
    """One window: ``vals`` [W, N] raw values, ``valid`` [W, N] bool -> per-date scores (int64, or float64 for float32 data)."""
    W, N = vals.shape  # noqa: N806
    n = valid.sum(axis=0)
    assert (n >= 1).all()
    cols = np.arange(N)
    if vals.dtype.kind in "iu":
        v = vals.astype(np.int64)
        srt = np.sort(np.where(valid, v, np.iinfo(np.int64).max), axis=0)
        a, b = srt[(n - 1) // 2, cols], srt[n // 2, cols]
        return np.where(valid, np.abs(2 * v - (a + b)), 0).sum(axis=1, dtype=np.int64)
    assert vals.dtype == np.float32
    srt = np.sort(np.where(valid, vals, np.float32(np.inf)), axis=0)
    a, b = srt[(n - 1) // 2, cols], srt[n // 2, cols]
    with np.errstate(invalid="ignore", over="ignore"):      # (a + b of an odd count is computed and dropped)
        med = np.where(n % 2 == 1, a, (a + b) / np.float32(2))
        dev = np.where(valid, np.abs(vals - med), np.float32(0))
    assert med.dtype == np.float32 and dev.dtype == np.float32
    acc = np.zeros(W, dtype=np.float64)
    for e in range(N):                                                             # float64, element order
        acc = acc + dev[:, e].astype(np.float64)
    return acc


def select_device(raw, dates, t_start, W, nd, mask=None, mask_floor=0, scores=None, log_scale=False, norm_fac=None):  # noqa: N803
    """Form (b).  Operands as ``select_reference``; ``mask_floor`` is the integer the device compares mask values with."""
    win, mwin, dwin, swin = _windows(raw, mask, dates, scores, t_start, W, nd)
    C = raw.shape[1]  # noqa: N806
    idx = np.zeros(nd, dtype=np.int64)
    for j in range(nd):
        masked = np.zeros((W, 1) + raw.shape[2:], dtype=bool)
        if mwin is not None:
            masked = (mwin[j].astype(np.int64) > int(mask_floor)).any(axis=1, keepdims=True)      # [W, 1, S, S]
        dirty = masked.reshape(W, -1).any(axis=1)
        if dirty.all():
            masked, dirty = np.zeros_like(masked), np.zeros(W, dtype=bool)
        if swin is not None:
            s = swin[j]
        else:
            valid = np.broadcast_to(~masked, (W, C) + raw.shape[2:]).reshape(W, -1)
            s = device_scores(win[j].reshape(W, -1), valid)
        best = -1
        for w in range(W):
            if dirty[w] or s[w] != s[w]:
                continue
            if best < 0 or s[w] < s[best]:
                best = w
        idx[j] = max(best, 0)
    return _finish(win, dwin, idx, log_scale, norm_fac)


def select_batch(form, raw, dates, t_start, t_win, nd, mask=None, scores=None, **kw):
    """``form`` = ``select_reference`` or ``select_device`` over a padded batch ``raw`` [B, Tmax, C, S, S]; stacks the results."""
    res = [form(raw[b], dates[b], int(t_start[b]), int(t_win[b]), nd, mask=None if mask is None else mask[b],
                scores=None if scores is None else scores[b], **kw) for b in range(raw.shape[0])]
    return tuple(np.stack([r[i] for r in res]) for i in range(4))


def ulp_error(got32, exact64):
    """|got - exact| in units of the float32 spacing at ``exact`` (float64 arithmetic)."""
    exact64 = np.asarray(exact64, dtype=np.float64)
    return np.abs(np.asarray(got32, dtype=np.float64) - exact64) / np.spacing(np.abs(exact64).astype(np.float32)).astype(np.float64)
