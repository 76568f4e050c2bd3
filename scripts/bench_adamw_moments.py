"""Cost of AdamW with bf16 moments (include/maestro_hip.h): ``mh_adamw_bf16m`` beside ``mh_adamw``, and the guarded
(device-scalar) and grouped pairs, over one buffer.

    python scripts/bench_adamw_moments.py [--n 176200000 898300000] [--rounds 20] [--warmup 5] [--out FILE.md]

One process; per size one set of buffers of ``--n`` elements (defaults: the flat parameter counts of C3 and C4).  Every round
issues one launch of each form, alternating -- fp32 moments, bf16 moments, then the same for the device-scalar and the grouped
(14 groups) forms -- each timed by HIP events around the single launch; the table is the median (min - max) of ``--rounds``
rounds after ``--warmup``.  Bytes are ALGORITHMIC: 30 per element with fp32 moments (p, g, m, v read; p, m, v and the bf16 shadow
written), 22 with bf16 moments.  Before timing, one launch of each kind from the same inputs is compared: the parameters of the
bf16-moment form must be the bits of ``mh_adamw`` started from the upcast moments.  There is no pass / fail number.  Needs a
GPU: there is no fallback.
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
N_GROUPS = 14


def event_ms(fn) -> float:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def layout(n: int):
    """Spans of 64 * 4099 elements over ``[0, ceil64(n))``, ids cycling through ``N_GROUPS`` groups of scale ``0.75^k``."""
    total, span = -(-n // 64) * 64, 64 * 4099
    return [(lo, min(lo + span, total), 0.75 ** (k % N_GROUPS), HYPER["wd"]) for k, lo in enumerate(range(0, total, span))]


def bench(n: int, rounds: int, warmup: int, dev) -> list[str]:
    h = HYPER
    g = torch.randn(n, device=dev) * 1e-2
    p, m, v = torch.randn(n, device=dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    m16, v16 = torch.zeros(n, dtype=torch.bfloat16, device=dev), torch.zeros(n, dtype=torch.bfloat16, device=dev)
    half = torch.empty(n, dtype=torch.bfloat16, device=dev)
    bc1, bc2 = hip.adamw_bias_corrections(h["b1"], h["b2"], 10)
    hyper = torch.tensor([h["lr"], bc1, bc2, 1.0, 1.0], dtype=torch.float32, device=dev)
    t_dev = torch.tensor([10], dtype=torch.int64, device=dev)
    gr = hip.ParamGroups(layout(n), dev)

    # the same inputs through both kinds once: the parameters must agree bit for bit
    cn = min(n, 1 << 22)
    start16 = (torch.randn(cn, device=dev) * 1e-3).bfloat16(), (torch.rand(cn, device=dev) * 1e-4).bfloat16()
    a = [p[:cn].clone(), start16[0].float(), start16[1].float(), half[:cn].clone()]
    b = [p[:cn].clone(), start16[0].clone(), start16[1].clone(), half[:cn].clone()]
    hip.adamw(a[0], g[:cn], a[1], a[2], a[3], cn, h["lr"], h["b1"], h["b2"], h["eps"], h["wd"], 10, 1.0)
    hip.adamw_bf16m(b[0], g[:cn], b[1], b[2], b[3], cn, 0, 0, h["lr"], h["b1"], h["b2"], h["eps"], h["wd"], 10, 1.0)
    torch.cuda.synchronize()
    same = torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[3].view(torch.int16), b[3].view(torch.int16))
    del a, b, start16

    args = (h["b1"], h["b2"], h["eps"])
    forms = {
        "mh_adamw": (30, lambda: hip.adamw(p, g, m, v, half, n, h["lr"], *args, h["wd"], 10, 1.0)),
        "mh_adamw_bf16m": (22, lambda: hip.adamw_bf16m(p, g, m16, v16, half, n, 0, 0, h["lr"], *args, h["wd"], 10, 1.0)),
        "mh_adamw_dev": (30, lambda: hip.adamw_dev(p, g, m, v, half, n, *args, h["wd"], hyper)),
        "mh_adamw_bf16m_dev": (22, lambda: hip.adamw_bf16m_dev(p, g, m16, v16, half, n, 0, 0, *args, h["wd"], hyper, t_dev)),
        f"mh_adamw_groups, {N_GROUPS} groups": (30, lambda: hip.adamw_groups(p, g, m, v, half, gr.map_at(0), gr.lr_scale, gr.wd, n,
                                                                              h["lr"], *args, 10, 1.0)),
        f"mh_adamw_groups_bf16m, {N_GROUPS} groups": (22, lambda: hip.adamw_groups_bf16m(p, g, m16, v16, half, gr.map_at(0), gr.lr_scale,
                                                                                        gr.wd, n, 0, 0, h["lr"], *args, 10, 1.0)),
    }
    times = {k: [] for k in forms}
    for r in range(warmup + rounds):
        for k, (_, fn) in forms.items():
            t = event_ms(fn)
            if r >= warmup:
                times[k].append(t)
    lines = [f"### n = {n} elements", "",
             f"{30.0 * n / 1e9:.2f} GB of algorithmic traffic per launch with fp32 moments, {22.0 * n / 1e9:.2f} GB with bf16 moments; "
             f"optimizer state {8.0 * n / 1e9:.2f} GB -> {4.0 * n / 1e9:.2f} GB.  us per launch, median (min - max) of {rounds} alternating "
             f"rounds after {warmup} warm-up rounds.", "",
             f"parameters and shadow of `mh_adamw_bf16m` against `mh_adamw` from the upcast moments over {cn} elements: "
             f"{'bit-equal' if same else 'DIFFERENT'}", "",
             "| kernel | bytes / element | us | spread (max - min) / median | TB/s at the median | time over its fp32 form |",
             "|---|---|---|---|---|---|"]
    base = None
    for k, ts in times.items():
        nbytes, med = forms[k][0], statistics.median(ts)
        if nbytes == 30:
            base = med
        lines.append(f"| `{k}` | {nbytes} | {1e3 * med:.1f} ({1e3 * min(ts):.1f} - {1e3 * max(ts):.1f}) | "
                     f"{100.0 * (max(ts) - min(ts)) / med:.1f} % | {nbytes * n / (med * 1e-3) / 1e12:.2f} | "
                     f"{'-' if nbytes == 30 else f'{med / base:.3f} x'} |")
    return lines + [""]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[176200000 // 1024 * 1024, 898300000 // 1024 * 1024])
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the tables to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_adamw_moments.py needs a GPU")
    if any(n <= 0 or n % 4 for n in args.n):
        raise SystemExit("--n must be positive multiples of 4")
    dev = torch.device("cuda:0")
    lines = [f"device: {torch.cuda.get_device_name(0)}", ""]
    for n in args.n:
        lines += bench(n, args.rounds, args.warmup, dev)
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
