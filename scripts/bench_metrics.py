"""Confusion-matrix kernel at the fine-tune bench shape (``bench.py --phase finetune --config c3``: the segmentation head's logits,
B = 32): DEVICE time per launch from HIP events, after a warm-up, median of ROUNDS launches taken in alternating rounds of
  (a) mh_confusion_ce                               reads the logits once, writes nothing but the C x C matrix
  (b) mh_ce_loss on the same operands               reads the logits and writes a gradient of the same extent
  (c) the torch path (a) replaces                   engine.logits() = depatchify into a second buffer, then argmax(1) + bincount
and (a)'s GB/s on its algorithmic bytes 4 * B * g^2 * ld.  Before timing, (a)'s matrix is compared for equality with (c)'s.
The condition that needs no measurement: (a) <= (b) in the same run.  ``--out FILE`` appends the result as a markdown table row
source (JSON line) for profiles/metrics_confusion.md."""
import argparse, json, os, statistics, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import maestro_amd.conf as conf
from maestro_amd import hip

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--rounds", type=int, default=30)
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_metrics.py measures on the GPU; there is nothing to measure without one")
dev = torch.device("cuda:0")

# the shape of bench.py's SUP_WORKLOADS["c3"]: FLAIR aerial grid, target cosia
ds = conf.DatasetsConfig(name_dataset="flair", flair=conf.FLAIRConfig(filter_inputs=["aerial", "s2"], filter_targets=["cosia"]))
tgt = ds.dataset.targets["cosia"]
ref = ds.dataset.inputs[ds.dataset.ref_input]
g = ref.image_size // ref.patch_size.mae                          # reference grid (ssl/mae.py: out_grid_size, PixelifyHead)
S = round(ds.dataset.crop_meters / tgt.resolution_meters)         # target raster
P, C, B, missing = S // g, tgt.num_classes, args.batch, tgt.missing_val
PPC = P * P * C
ld = (PPC + 7) // 8 * 8                 # SupervisedEngine's PPCp
R = B * g * g
torch.manual_seed(0)
logits = torch.randn(R, ld, device=dev)
target = torch.randint(0, C, (B, 1, 1, S, S), device=dev)
target[torch.rand(B, 1, 1, S, S, device=dev) < 0.1] = missing
cm = torch.zeros(C, C, dtype=torch.int64, device=dev)
cnt, acc = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, device=dev)
dlogits = torch.zeros(R, ld, dtype=torch.bfloat16, device=dev)
img = torch.empty(B, C, S, S, device=dev)


def run_a():
    hip.confusion_ce(logits, target, missing, cm, B, g, P, C, ld)


def run_b():
    hip.ce_loss(logits, target, missing, cnt, acc, dlogits, B, g, P, C, ld=ld)


def run_c():
    lg = logits if ld == PPC else logits[:, :PPC].contiguous()
    hip.depatchify(lg, img, B, C, S, P)                       # SupervisedEngine.logits()
    pred, t = img.argmax(1).reshape(-1), target.reshape(-1)
    valid = (t != missing) & (t >= 0) & (t < C)
    return torch.bincount(t[valid] * C + pred[valid], minlength=C * C).view(C, C)


hip.count_valid(target, missing, cnt)
run_a()
want = run_c()
torch.cuda.synchronize()
assert torch.equal(cm, want), "mh_confusion_ce disagrees with argmax + bincount"
runs = {"a_confusion_ce": run_a, "b_ce_loss": run_b, "c_torch_logits_argmax_bincount": run_c}
for fn in runs.values():                                       # warm-up: code objects, allocator
    for _ in range(3):
        fn()
torch.cuda.synchronize()
times = {k: [] for k in runs}
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
for _ in range(max(20, args.rounds)):                          # alternating: a drift of the card hits all three alike
    for k, fn in runs.items():
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times[k].append(e0.elapsed_time(e1) * 1e3)
nbytes = 4 * B * g * g * ld
res = {"shape": dict(B=B, g=g, P=P, C=C, ld=ld, logits_MB=round(nbytes / 1e6, 1)), "launches": len(times["a_confusion_ce"])}
for k, v in times.items():
    res[k] = dict(median_us=round(statistics.median(v), 1), min_us=round(min(v), 1), max_us=round(max(v), 1))
res["a_GBps"] = round(nbytes / res["a_confusion_ce"]["median_us"] / 1e3, 1)
res["a_le_b"] = res["a_confusion_ce"]["median_us"] <= res["b_ce_loss"]["median_us"]
line = json.dumps(res)
print(line, flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")
