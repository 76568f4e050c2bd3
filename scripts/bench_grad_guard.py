"""Cost of the gradient guard (include/maestro_hip.h): the streaming kernel alone, and the training step with it.

    python scripts/bench_grad_guard.py [--config c3] [--batch 32] [--variant NAME=LIB.so ...] [--out FILE.md]

1. ``mh_grad_sumsq_partial`` alone (HIP events around one launch, median and min / max of 30 after 5) over the flagship model's
   gradient buffer and over a tiny model's, with ``mh_adamw`` over the same buffer measured in the same rounds (alternating: one
   launch of each per round) -- the side-by-side bytes/s is the yardstick, not a quoted peak.  Bytes are ALGORITHMIC: 4 per
   element for the guard, 30 for AdamW (p, g, m, v read, p, m, v, bf16 shadow written).  Nothing else touches the buffers
   between the timed launches: what the caches hold is what the previous launch of the round left.
   ``--variant NAME=LIB`` adds the same kernel from another build of the library (scripts/build_variant.py, e.g. the plain-load
   form, ``--flags -DMH_GUARD_NT_LOADS=0 --only grad_guard.hip``) to the rounds.
2. The training step (bench.py's model and batch, bf16, graphs on): guard off / guard on (/ guard on with each variant's
   kernel), ONE loop whose optimizer is handed the guard or not -- rounds of ``--steps`` steps each, alternating, wall time per
   step with the device idle at both ends; median of the rounds with min / max.
There is no pass / fail number.  Needs a GPU: there is no fallback.
"""

from __future__ import annotations

import argparse
import ctypes
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import bench  # noqa: E402
from maestro_amd import hip  # noqa: E402
from maestro_amd.train.trainer import PretrainLoop, synthetic_batch  # noqa: E402


def event_ms(fn) -> float:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def load_variant(path: str):
    lib = ctypes.CDLL(str(Path(path).resolve()))
    vp, cl = ctypes.c_void_p, ctypes.c_long
    lib.mh_grad_sumsq_partial.argtypes, lib.mh_grad_sumsq_partial.restype = [vp, cl, vp, vp, vp], ctypes.c_int
    return lib


def variant_partial(lib, g, n, partial, bad) -> None:
    rc = lib.mh_grad_sumsq_partial(hip.ptr(g), n, hip.ptr(partial), hip.ptr(bad), hip.stream())
    if rc:
        raise RuntimeError(f"variant mh_grad_sumsq_partial failed (rc={rc})")


class VariantGuard(hip.GradGuard):
    """The library's guard with the first phase taken from another build."""

    def __init__(self, lib, *a, **k) -> None:
        super().__init__(*a, **k)
        self.lib = lib

    def launch(self, grad, lr, b1, b2, grad_scale=1.0) -> None:
        variant_partial(self.lib, grad, self.n, self.partial, self.bad)
        hip.grad_guard_finish(self.partial, self.bad, self.rows, grad_scale, self.max_norm, self.skip_nonfinite, lr, b1, b2,
                              self.hyper, self.state)


def fmt(ts) -> str:
    return f"{statistics.median(ts):.4f} ({min(ts):.4f} - {max(ts):.4f})"


def isolated(n: int, dev, variants: dict, label: str, rounds: int = 30, warmup: int = 5) -> list[str]:
    g = torch.randn(n, device=dev)
    p, m, v = torch.randn(n, device=dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    half = torch.empty(n, dtype=torch.bfloat16, device=dev)
    rows = hip.grad_sumsq_partial_rows(n)
    partial, bad = torch.empty(rows, device=dev), torch.empty(rows, dtype=torch.int32, device=dev)
    forms = {"mh_grad_sumsq_partial": lambda: hip.grad_sumsq_partial(g, n, partial, bad)}
    for name, lib in variants.items():
        forms[f"mh_grad_sumsq_partial [{name}]"] = lambda lib=lib: variant_partial(lib, g, n, partial, bad)
    forms["mh_adamw"] = lambda: hip.adamw(p, g, m, v, half, n, 1e-4, 0.9, 0.99, 1e-8, 0.01, 10, 1.0)
    nbytes = {k: 4.0 * n for k in forms}
    nbytes["mh_adamw"] = 30.0 * n
    times = {k: [] for k in forms}
    for r in range(warmup + rounds):
        for k, fn in forms.items():
            t = event_ms(fn)
            if r >= warmup:
                times[k].append(t)
    lines = [f"{label}: n = {n} elements ({4 * n / 1e6:.1f} MB of gradient, {rows} partial rows); ms per launch, median (min - max) of {rounds}", "",
             "| kernel | ms | algorithmic bytes | TB/s at the median |", "|---|---|---|---|"]
    for k, ts in times.items():
        lines.append(f"| `{k}` | {fmt(ts)} | {nbytes[k] / 1e6:.1f} MB | {nbytes[k] / (statistics.median(ts) * 1e-3) / 1e12:.2f} |")
    return lines + [""]


def step_rounds(loop, batch, guards: dict, steps: int, rounds: int) -> dict:
    """ms per step for every entry of ``guards`` (name -> guard or None), alternating round by round on ONE loop."""
    times = {k: [] for k in guards}
    for r in range(rounds + 1):                  # round 0 warms every form up
        for k, guard in guards.items():
            loop.guard = loop.opt.guard = guard
            loop.step(batch)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                loop.step(batch)
            torch.cuda.synchronize()
            if r:
                times[k].append(1e3 * (time.perf_counter() - t0) / steps)
    loop.guard = loop.opt.guard = None
    return times


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--variant", action="append", default=[], metavar="NAME=LIB.so")
    ap.add_argument("--out", default=None, help="also write the tables to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_grad_guard.py needs a GPU")
    dev = torch.device("cuda:0")
    torch.set_num_threads(min(4, bench.host_cores()))
    variants = {name: load_variant(path) for name, path in (v.split("=", 1) for v in args.variant)}

    torch.manual_seed(42)
    ds, model = bench.build_model(args.config, "pretrain")
    batch = synthetic_batch(ds.dataset, args.batch, dev, seed=0)
    loop = PretrainLoop(model, args.batch, dev, total_steps=10_000)
    n = loop.opt.hi - loop.opt.lo
    lines = [f"device: {torch.cuda.get_device_name(0)}; config {args.config}, B = {args.batch}", ""]
    lines += isolated(n, dev, variants, f"{args.config} gradient span")
    lines += isolated(2_000_000, dev, variants, "tiny model's size (cache-resident: 8 MB)")

    guards = {"guard off": None,
              "guard on": hip.GradGuard(n, dev, max_norm=1.0, skip_nonfinite=True)}
    for name, lib in variants.items():
        guards[f"guard on [{name}]"] = VariantGuard(lib, n, dev, max_norm=1.0, skip_nonfinite=True)
    for _ in range(10):
        loop.step(batch)
    times = step_rounds(loop, batch, guards, args.steps, args.rounds)
    off = statistics.median(times["guard off"])
    lines += [f"training step, {args.rounds} alternating rounds of {args.steps} steps; ms per step, median (min - max) of the rounds", "",
              "| form | ms per step | over guard off |", "|---|---|---|"]
    for k, ts in times.items():
        lines.append(f"| {k} | {fmt(ts)} | {statistics.median(ts) - off:+.4f} ms |")
    skipped = {k: g.stats()["skipped"] for k, g in guards.items() if g is not None}
    lines += ["", f"skipped steps per guard: {skipped}; last norm {float(guards['guard on'].norm):.4g}, "
                  f"coefficient {float(guards['guard on'].coef):.4g}"]
    text = "\n".join(lines)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
