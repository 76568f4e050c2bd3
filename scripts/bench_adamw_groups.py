"""Cost of AdamW parameter groups (include/maestro_hip.h): ``mh_adamw_groups`` beside ``mh_adamw`` over one buffer.

    python scripts/bench_adamw_groups.py [--n 176200000] [--groups 1 14 52] [--rounds 20] [--warmup 5] [--out FILE.md]

One process, one set of buffers of ``--n`` elements (default: C3's parameter count, the size ``scripts/micro_adamw.hip`` and
``profiles/r05_experiments.md`` used for AdamW).  Every round issues one launch of each form, alternating -- ``mh_adamw``, then
``mh_adamw_groups`` with 1, 14 and 52 groups -- each timed by HIP events around the single launch; the table is the median
(min - max) of ``--rounds`` rounds after ``--warmup``.  Nothing else touches the buffers between the timed launches: what the
caches hold is what the previous launch of the round left.  Bytes are ALGORITHMIC: 30 per element (p, g, m, v read; p, m, v and
the bf16 shadow written); the map (1 byte per 64 elements) and the tables (2 KiB) are listed, not counted.

The group layouts imitate the layer rule: G groups over parameter-sized spans (a few hundred thousand elements each, 64-aligned),
group ids cycling, scales ``0.75^k``; 14 = a 12-block encoder + patch embed + heads, 52 = the 26 scales of a 24-block encoder, each
with and without weight decay (``no_decay_1d``).  Before timing, one launch of each form from the same inputs is compared: with every scale 1 and one weight decay
the grouped form must give the bits of ``mh_adamw``.  There is no pass / fail number.  Needs a GPU: there is no fallback.
"""

from __future__ import annotations

import argparse
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from maestro_amd import hip  # noqa: E402

HYPER = dict(lr=1e-4, b1=0.9, b2=0.99, eps=1e-8, wd=0.01)


def event_ms(fn) -> float:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def layout(n: int, n_groups: int, uniform: bool = False):
    """Spans of 64 * 4099 elements (a 512 x 512 weight matrix and change) over ``[0, ceil64(n))``, ids cycling through the groups."""
    total = -(-n // 64) * 64
    span = 64 * 4099
    spans, lo, k = [], 0, 0
    while lo < total:
        hi = min(lo + span, total)
        g = k % n_groups
        split = n_groups > 26 and not uniform          # above 26 groups: every scale once with and once without weight decay
        scale = 1.0 if uniform else 0.75 ** (g // 2 if split else g)
        spans.append((lo, hi, scale, 0.0 if (split and g % 2) else HYPER["wd"]))
        lo, k = hi, k + 1
    return spans


def fmt(ts) -> str:
    return f"{statistics.median(ts):.4f} ({min(ts):.4f} - {max(ts):.4f})"


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=176200000 // 1024 * 1024)
    ap.add_argument("--groups", type=int, nargs="+", default=[1, 14, 52])
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_adamw_groups.py needs a GPU")
    if args.n <= 0 or args.n % 4:
        raise SystemExit("--n must be a positive multiple of 4")
    dev = torch.device("cuda:0")
    n, h = args.n, HYPER
    g = torch.randn(n, device=dev)
    p, m, v = torch.randn(n, device=dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    half = torch.empty(n, dtype=torch.bfloat16, device=dev)

    # the same inputs through both forms once: all scales 1 and one weight decay must give mh_adamw's bits
    check_n = min(n, 1 << 22)
    uniform = hip.ParamGroups(layout(check_n, 7, uniform=True), dev)
    a = [t[:check_n].clone() for t in (p, m, v)] + [half[:check_n].clone()]
    b = [t[:check_n].clone() for t in (p, m, v)] + [half[:check_n].clone()]
    hip.adamw(a[0], g[:check_n], a[1], a[2], a[3], check_n, h["lr"], h["b1"], h["b2"], h["eps"], h["wd"], 10, 1.0)
    hip.adamw_groups(b[0], g[:check_n], b[1], b[2], b[3], uniform.map_at(0), uniform.lr_scale, uniform.wd, check_n, h["lr"], h["b1"],
                     h["b2"], h["eps"], 10, 1.0)
    torch.cuda.synchronize()
    same = all(torch.equal(x.view(torch.int16 if x.element_size() == 2 else torch.int32),
                           y.view(torch.int16 if y.element_size() == 2 else torch.int32)) for x, y in zip(a, b))
    del a, b

    forms = {"mh_adamw": lambda: hip.adamw(p, g, m, v, half, n, h["lr"], h["b1"], h["b2"], h["eps"], h["wd"], 10, 1.0)}
    tables = {}
    for k in args.groups:
        gr = tables[k] = hip.ParamGroups(layout(n, k), dev)
        forms[f"mh_adamw_groups, {k} group{'s' if k > 1 else ''}"] = lambda gr=gr: hip.adamw_groups(
            p, g, m, v, half, gr.map_at(0), gr.lr_scale, gr.wd, n, h["lr"], h["b1"], h["b2"], h["eps"], 10, 1.0)
    times = {k: [] for k in forms}
    for r in range(args.warmup + args.rounds):
        for k, fn in forms.items():
            t = event_ms(fn)
            if r >= args.warmup:
                times[k].append(t)
    base = statistics.median(times["mh_adamw"])
    lines = [f"device: {torch.cuda.get_device_name(0)}", "",
             f"n = {n} elements ({30.0 * n / 1e9:.2f} GB of algorithmic traffic per launch; group map {-(-n // 64) / 1e6:.2f} MB, tables 2 KiB); "
             f"ms per launch, median (min - max) of {args.rounds} alternating rounds after {args.warmup} warm-up rounds", "",
             f"all scales 1, one weight decay: bits of mh_adamw over {check_n} elements: {'equal' if same else 'DIFFERENT'}", "",
             "| kernel | distinct (lr_scale, wd) pairs | ms | TB/s at the median | over mh_adamw |", "|---|---|---|---|---|"]
    for k, ts in times.items():
        med = statistics.median(ts)
        pairs = "-" if k == "mh_adamw" else str(len(tables[int(k.split(",")[1].split()[0])].pairs))
        lines.append(f"| `{k}` | {pairs} | {fmt(ts)} | {30.0 * n / (med * 1e-3) / 1e12:.2f} | {100.0 * (med / base - 1.0):+.2f} % |")
    text = "\n".join(lines)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
