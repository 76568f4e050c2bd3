"""Mask draws of the pretraining step: host time in front of the step's first launch, host drawer against device draws, and
the time of the ``mh_mask_draw`` launch.

    python scripts/bench_mask_rng.py [--config c3] [--batch 32] [--out FILE.md]

For each ``mask_rng`` mode, on the flagship engine (bench.py's model, bf16, graphs on):
  * host ms from the entry of ``MAEEngine.forward`` to the point where the forward segment is handed to the runtime (everything
    a step does on the host before its first forward kernel can be issued: the draws, the ring copies and their events in host
    mode, the one launch in device mode) -- ``time.perf_counter``, median / max of 50 steps after 10, device idle at each entry,
    torch pinned to 4 threads as bench.py pins it and, for comparison, left at the process default;
  * device mode only: HIP events around one ``MaskDraw.launch``, median of 20 after 5, and the mean of 100 launches enqueued
    back to back; bytes written.
There is no pass / fail number.  Needs a GPU: there is no fallback.
"""

from __future__ import annotations

import argparse
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import bench  # noqa: E402
from maestro_amd.train.trainer import synthetic_batch  # noqa: E402


def host_prefix_ms(eng, batch, steps=50, warmup=10):
    """ms between the entry of forward() and the entry of the forward segment, per step."""
    seg, mark = eng._forward_segment, [0.0]

    def traced(b):
        mark[0] = time.perf_counter()
        return seg(b)

    eng._forward_segment = traced
    out = []
    try:
        for i in range(warmup + steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.forward(batch)
            if i >= warmup:
                out.append(1e3 * (mark[0] - t0))
    finally:
        del eng._forward_segment
    torch.cuda.synchronize()
    return statistics.median(out), max(out)


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
    ap.add_argument("--config", default="c3")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--out", default=None, help="also write the tables to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mask_rng.py needs a GPU")
    dev = torch.device("cuda:0")
    default_threads = torch.get_num_threads()
    torch.manual_seed(42)
    ds, model = bench.build_model(args.config, "pretrain")
    batch = synthetic_batch(ds.dataset, args.batch, dev, seed=0)
    lines = [f"config {args.config}, B = {args.batch}; host ms before the forward segment (median / max of 50 steps)", "",
             "| mask_rng | torch threads | median ms | max ms |", "|---|---|---|---|"]
    for mode in ("host", "device"):
        model._engine = None
        eng = model.engine(args.batch, dev, loss="l2_norm", mask_rng=mode)
        for threads in (min(4, bench.host_cores()), default_threads):
            torch.set_num_threads(threads)
            med, worst = host_prefix_ms(eng, batch)
            lines.append(f"| {mode} | {threads} | {med:.3f} | {worst:.3f} |")
    draw = eng._mask_draw
    one = event_ms(lambda: draw.launch(eng.mask_seed, 1, 0))
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(100):
        draw.launch(eng.mask_seed, i, 0)
    e1.record()
    e1.synchronize()
    rows = sum(g.Beff for g in eng.groups)
    lines += ["", f"`mh_mask_draw`: {len(eng.groups)} groups, {rows} workgroups, {draw.nbytes / 1024:.0f} KiB written: "
              f"{1e3 * one:.1f} us per launch (events around one launch, median of 20), "
              f"{1e3 * e0.elapsed_time(e1) / 100:.1f} us per launch enqueued back to back (mean of 100)"]
    text = "\n".join(lines)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
