"""Prediction kernels and ``SupervisedEngine.predict`` at the fine-tune bench shape (``bench.py --phase finetune --config c3``: FLAIR
aerial + Sentinel-2, the cosia segmentation head, B = 32).  DEVICE time from HIP events after a warm-up, medians of launches taken
in ALTERNATING rounds inside one process, with min / max as the spread of every entry:

kernels (the head's logits shape, random operands)
  view        mh_predict_view, identity view, cls + conf       reads 4 C bytes per pixel, writes 5
  ce_loss     mh_ce_loss on the same logits                    reads 4 C, writes 2 C (bf16 gradient)
  confusion   mh_confusion_ce on the same logits               reads 4 C
  view_acc    mh_predict_view accumulating into prob           reads 4 C, read-modify-writes 8 C
  finish      mh_predict_finish (cls + conf)                   reads 4 C, writes 5
engine (``--engine``; the c3 model itself)
  predict          predict(batch)                              against the path it replaces:
  forward_argmax   forward(batch_with_targets) + logits() + argmax + softmax().max()
  predict_d4       predict(batch, views="d4")                  against
  predict_8x1      eight single-view predict(batch, views=(v,)) calls

GB/s are on the algorithmic bytes above.  ``--out FILE`` appends the JSON line (the source of profiles/predict.md)."""
import argparse, json, os, statistics, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import maestro_amd.conf as conf
from maestro_amd import hip

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--rounds", type=int, default=30)
ap.add_argument("--engine", action="store_true", help="also time SupervisedEngine.predict on the c3 model")
ap.add_argument("--engine-rounds", type=int, default=6)
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_predict.py measures on the GPU; there is nothing to measure without one")
dev = torch.device("cuda:0")

# the shape of bench.py's SUP_WORKLOADS["c3"]: FLAIR aerial grid, target cosia (scripts/bench_metrics.py)
ds = conf.DatasetsConfig(name_dataset="flair", flair=conf.FLAIRConfig(filter_inputs=["aerial", "s2"], filter_targets=["cosia"]))
tgt = ds.dataset.targets["cosia"]
ref = ds.dataset.inputs[ds.dataset.ref_input]
g = ref.image_size // ref.patch_size.mae
S = round(ds.dataset.crop_meters / tgt.resolution_meters)
P, C, B, missing = S // g, tgt.num_classes, args.batch, tgt.missing_val
PPC = P * P * C
ld = (PPC + 7) // 8 * 8
R, n_pix = B * g * g, B * S * S
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
            times[k].append(e0.elapsed_time(e1) * 1e3)
    return {k: dict(median_us=round(statistics.median(v), 1), min_us=round(min(v), 1), max_us=round(max(v), 1)) for k, v in times.items()}


def kernels():
    torch.manual_seed(0)
    logits = torch.randn(R, ld, device=dev)
    target = torch.randint(0, C, (B, 1, 1, S, S), device=dev)
    target[torch.rand(B, 1, 1, S, S, device=dev) < 0.1] = missing
    cm = torch.zeros(C, C, dtype=torch.int64, device=dev)
    cnt, acc = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, device=dev)
    dlogits = torch.zeros(R, ld, dtype=torch.bfloat16, device=dev)
    cls = torch.empty(B, S, S, dtype=torch.uint8, device=dev)
    cf = torch.empty(B, S, S, device=dev)
    prob = torch.zeros(B, C, S, S, device=dev)
    hip.count_valid(target, missing, cnt)
    hip.predict_view(logits, None, hip.PREDICT_SOFTMAX, None, False, cls, cf, B, g, P, C, ld=ld)
    img = torch.empty(B, C, S, S, device=dev)
    hip.depatchify(logits[:, :PPC].contiguous() if ld != PPC else logits, img, B, C, S, P)
    torch.cuda.synchronize()
    assert torch.equal(cls.long(), img.argmax(1)), "mh_predict_view disagrees with depatchify + argmax"
    del img
    runs = {
        "view": lambda: hip.predict_view(logits, None, hip.PREDICT_SOFTMAX, None, False, cls, cf, B, g, P, C, ld=ld),
        "ce_loss": lambda: hip.ce_loss(logits, target, missing, cnt, acc, dlogits, B, g, P, C, ld=ld),
        "confusion": lambda: hip.confusion_ce(logits, target, missing, cm, B, g, P, C, ld),
        "view_acc": lambda: hip.predict_view(logits, None, hip.PREDICT_SOFTMAX, prob, True, None, None, B, g, P, C, ld=ld),
        "finish": lambda: hip.predict_finish(prob, 8, hip.PREDICT_SOFTMAX, cls, cf, B, C, S * S),
    }
    res = alternate(runs, max(20, args.rounds))
    alg = {"view": 4 * C + 5, "ce_loss": 6 * C, "confusion": 4 * C, "view_acc": 12 * C, "finish": 4 * C + 5}
    for k, per_pixel in alg.items():
        res[k]["GBps"] = round(per_pixel * n_pix / res[k]["median_us"] / 1e3, 1)
    res["view_le_ce_loss"] = res["view"]["median_us"] <= res["ce_loss"]["median_us"]
    return res


def engine():
    import bench
    from maestro_amd.train.trainer import synthetic_batch
    _, model = bench.build_model("c3", "finetune")
    eng = model.sup_engine(B, dev, "finetune")
    batch = synthetic_batch(model.dataset, B, dev)
    labelled = dict(batch)
    labelled.update(bench.synthetic_targets(model.dataset, B, dev))

    def forward_argmax():
        eng.forward(labelled)
        out = {}
        for t, lg in eng.logits().items():
            out[t] = (lg.argmax(dim=2), lg.softmax(dim=2).max(dim=2).values)
        return out

    runs = {
        "predict": lambda: eng.predict(batch),
        "forward_argmax": forward_argmax,
        "predict_d4": lambda: eng.predict(batch, views="d4"),
        "predict_8x1": lambda: [eng.predict(batch, views=(v,)) for v in range(8)],
    }
    return alternate(runs, args.engine_rounds, warm=3)


out = {"shape": dict(B=B, g=g, P=P, C=C, ld=ld, S=S, logits_MB=round(4 * R * ld / 1e6, 1)), "kernels": kernels()}
if args.engine:
    out["engine"] = engine()
line = json.dumps(out)
print(line, flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")
