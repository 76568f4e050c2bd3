"""``mh_knn_topk`` in isolation at ``E = 768, k = 20`` against what a user writes without it, ``torch.topk(q @ bank.T, k)`` on the
same bf16 operands (torch leaves the product in bf16: its cheapest form, half the bytes of an fp32 matrix and coarser
similarities than the kernel's fp32 ones), same card, same process.  DEVICE time from HIP events after a warm-up, medians of runs taken in ALTERNATING
rounds, min / max as spread:

  Nq = 32,   Nb = 131072   one batch of sample features against a bank
  Nq = 4096, Nb = 131072   a validation set against a bank
  Nq = 3200, Nb = 262144   per-cell features of one batch (32 x 100 cells)

Per shape: both times, the achieved TFLOP/s on ``2 Nq Nb E``, the kernel's workspace bytes against the ``4 Nq Nb`` bytes of an
fp32 similarity matrix (``2 Nq Nb`` as torch holds it in bf16), and the share of the kernel's indices that an fp32
``torch.topk`` agrees with.  ``--out FILE`` appends the JSON line (the source of profiles/knn.md)."""
import argparse, json, os, statistics, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from maestro_amd import hip

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--dim", type=int, default=768)
ap.add_argument("--k", type=int, default=20)
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_knn.py measures on the GPU; there is nothing to measure without one")
dev = torch.device("cuda:0")
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def alternate(runs, rounds, warm=3):
    for fn in runs.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    for _ in range(rounds):
        for k, fn in runs.items():
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1))
    return {k: dict(median_ms=round(statistics.median(v), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4)) for k, v in times.items()}


E, k = args.dim, args.k
g = torch.Generator(device=dev).manual_seed(0)
out = {"E": E, "k": k, "shapes": []}
for Nq, Nb in ((32, 131072), (4096, 131072), (3200, 262144)):
    q = torch.nn.functional.normalize(torch.randn(Nq, E, device=dev, generator=g), dim=1).to(torch.bfloat16)
    bank = torch.nn.functional.normalize(torch.randn(Nb, E, device=dev, generator=g), dim=1).to(torch.bfloat16)
    sims = torch.empty(Nq, k, device=dev)
    idx = torch.empty(Nq, k, dtype=torch.int32, device=dev)
    splits = hip.knn_splits(Nq, Nb, E, k)
    res = alternate({
        "knn_topk": lambda: hip.knn_topk(q, bank, k, sims=sims, idx=idx),
        "torch_topk": lambda: torch.topk(q @ bank.t(), k),
    }, args.rounds)
    want = torch.topk(torch.mm(q.float(), bank.float().t()), k)
    agree = float((idx.long() == want.indices).float().mean())
    flops = 2.0 * Nq * Nb * E
    for r in res.values():
        r["TFLOPs"] = round(flops / r["median_ms"] / 1e9, 1)
    out["shapes"].append(dict(Nq=Nq, Nb=Nb, splits=splits, workspace_bytes=hip.knn_workspace_bytes(Nq, k, splits),
                              matrix_bytes=4 * Nq * Nb, idx_agree_with_fp32_topk=round(agree, 6), **res))
    del q, bank, want
    torch.cuda.empty_cache()
line = json.dumps(out)
print(line, flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")
