"""Median-date selection: what the device side costs against the numpy form of the reference's lines on the same host.

    python scripts/bench_date_select.py [--out FILE.md]

For B = 32 samples at the TreeSatAI-TS and PASTIS-HD Sentinel-2 shapes (raw [T, C, S, S] -> 16 dates, masked, int16):
  * kernel time of ``hip.select_dates``: HIP events around one launch, median of 20 after 5 warm-up launches, and the mean of
    100 launches enqueued back to back (what a launch costs when the stream is busy);
  * H2D time of the raw batch and its mask from pinned memory (HIP events, median of 20 after 5);
  * ms / sample of the numpy restatement of maestro/dataset/dataset.py:188-220 (tests/date_select_ref.select_reference: nanmedian,
    mean, nanargmin), one thread, median over 8 samples;
  * the device's choice is compared with the restatement's on the timed batch first.
There is no pass / fail number; the last column says whether H2D + kernel for the batch is below 32 x numpy / 16 threads.
Needs a GPU: there is no fallback.
"""

from __future__ import annotations

import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from maestro_amd import hip  # noqa: E402
from tests import date_select_ref as ref  # noqa: E402

SHAPES = [("TreeSatAI-TS S2", 128, 10, 6, 16), ("PASTIS-HD S2", 64, 10, 16, 16)]
B, THREADS = 32, 16


def make(rng, T, C, S, nd):  # noqa: N803
    raw = rng.integers(0, 10000, size=(B, T, C, S, S)).astype(np.int16)
    cloudy = rng.random((B, T, 1, 1, 1)) < 0.3                                     # three dates in ten have clouds, over a fifth of their pixels
    mask = (cloudy * (rng.random((B, T, 1, S, S)) < 0.2) * 100).astype(np.uint8)
    dates = rng.integers(0, 3000, size=(B, T, 3)).astype(np.int16)
    return raw, mask, dates, [0] * B, [T // nd] * B


def event_ms(fn, warmup=5, reps=20):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the table to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_date_select.py needs a GPU")
    torch.set_num_threads(1)
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    rows = []
    for name, T, C, S, nd in SHAPES:  # noqa: N806
        raw, mask, dates, t_start, t_win = make(rng, T, C, S, nd)
        h_raw, h_mask = torch.from_numpy(raw).pin_memory(), torch.from_numpy(mask).pin_memory()
        d_raw, d_mask, d_dates = h_raw.to(dev), h_mask.to(dev), torch.from_numpy(dates).to(dev)
        d_ts, d_tw = torch.tensor(t_start, dtype=torch.int32, device=dev), torch.tensor(t_win, dtype=torch.int32, device=dev)
        out = torch.empty((B, nd, C, S, S), dtype=torch.float32, device=dev)
        od, oi = torch.empty((B, nd, 3), dtype=torch.int16, device=dev), torch.empty((B, nd), dtype=torch.int32, device=dev)

        def launch():
            hip.select_dates(d_raw, d_dates, t_start, t_win, nd, mask=d_mask, mask_floor=0, norm_fac=5000.0, t_start_dev=d_ts,
                             t_win_dev=d_tw, out=out, out_dates=od, out_index=oi)

        launch()
        torch.cuda.synchronize()
        want = ref.select_batch(ref.select_reference, raw[:4], dates[:4], t_start[:4], t_win[:4], nd, mask=mask[:4],
                                mask_threshold=0.0, norm_fac=5000.0)
        assert np.array_equal(oi[:4].cpu().numpy(), want[0]) and out[:4].cpu().numpy().tobytes() == want[1].tobytes(), name
        dirty = float((mask.reshape(B, T, -1) > 0).any(axis=2).mean())

        kernel_ms = event_ms(launch)
        for _ in range(5):
            launch()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(100):
            launch()
        e1.record()
        e1.synchronize()
        back_to_back_ms = e0.elapsed_time(e1) / 100

        def h2d():
            d_raw.copy_(h_raw, non_blocking=True)
            d_mask.copy_(h_mask, non_blocking=True)

        h2d_ms = event_ms(h2d)

        cpu = []
        for b in range(8):
            t0 = time.perf_counter()
            ref.select_reference(raw[b], dates[b], 0, T // nd, nd, mask=mask[b], mask_threshold=0.0, norm_fac=5000.0)
            cpu.append((time.perf_counter() - t0) * 1e3)
        numpy_ms = statistics.median(cpu)
        budget_ms = B * numpy_ms / THREADS
        rows.append((name, f"{T} x {C} x {S} x {S} -> {nd}", raw.nbytes + mask.nbytes, dirty, kernel_ms, back_to_back_ms, h2d_ms,
                     numpy_ms, budget_ms, h2d_ms + kernel_ms < budget_ms))

    lines = [f"device: {torch.cuda.get_device_name(0)}; B = {B}, int16 raw data, one mask channel",
             "",
             "| shape | raw + mask bytes | dirty dates | kernel ms (median of 20) | kernel ms (100 back to back) | H2D ms | numpy ms / sample | "
             f"{B} x numpy / {THREADS} threads, ms | H2D + kernel below it |",
             "|---|---|---|---|---|---|---|---|---|"]
    for name, shape, nbytes, dirty, k, bb, h, n, bud, ok in rows:
        lines.append(f"| {name}: {shape} | {nbytes} | {dirty:.0%} | {k:.4f} | {bb:.4f} | {h:.4f} | {n:.2f} | {bud:.2f} | {'yes' if ok else 'NO'} |")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
