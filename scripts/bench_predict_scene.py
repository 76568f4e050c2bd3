"""``SupervisedEngine.predict_scene`` at the fine-tune bench shape (``bench.py --phase finetune --config c3``: FLAIR aerial +
Sentinel-2, the cosia segmentation head, B = 32): one scene of 8 x 8 windows at half-window stride (9 x 9 units, two batches).
DEVICE time from HIP events after a warm-up, medians of runs taken in ALTERNATING rounds inside one process, min / max as spread:

whole scene
  scene          predict_scene(scene)                            against what a user writes without it:
  torch_glue     per batch: the windows cut with torch slicing + stack, ``predict(batch, probs=True)``, the probabilities
                 weighted and ``add_``-ed onto the canvas window by window; then the division, the arg-max and the maximum
  predict        ``predict(batch, probs=True)`` alone (one forward and its softmax: the floor of a batch of either path)
the three new launches, on the engine's own operands of that scene
  gather         mh_window_gather, all rasters of one batch      reads and writes 4 bytes per window pixel
  blend          mh_predict_blend, one batch                     reads 4 C per window pixel, read-modify-writes 8 (C + 1) per
                                                                 canvas pixel under the batch (hip.scene_blend_bytes)
  finish         mh_predict_blend_finish (cls, conf, mean)       reads 4 (C + 1) per canvas pixel, writes 4 C + 5
  view           mh_predict_view (prob + cls + conf), one batch  reads 4 C per window pixel, writes 4 C + 5: the yardstick

GB/s are on the algorithmic bytes above; ``share`` is (batches x (gather + blend) + finish) / scene.  ``--out FILE`` appends the
JSON line (the source of profiles/predict_scene.md)."""
import argparse, json, os, statistics, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from maestro_amd import hip

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--windows", type=int, default=8, help="windows per axis at half-window stride")
ap.add_argument("--rounds", type=int, default=6)
ap.add_argument("--kernel-rounds", type=int, default=20)
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_predict_scene.py measures on the GPU; there is nothing to measure without one")
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
    return {k: dict(median_ms=round(statistics.median(v), 3), min_ms=round(min(v), 3), max_ms=round(max(v), 3)) for k, v in times.items()}


import bench  # noqa: E402
from maestro_amd.train.trainer import synthetic_batch  # noqa: E402

_, model = bench.build_model("c3", "finetune")
B = args.batch
eng = model.sup_engine(B, dev, "finetune")
geo = eng.scene_geometry()
W, half = geo["W"], max(1, geo["W"] // 2)
U = half * (args.windows - 1) + W                        # units per axis: `windows` starts at half-window stride
sources = [parts[0] for parts in model.src_specs.values()]
batch = synthetic_batch(model.dataset, B, dev)
g = torch.Generator(device=dev).manual_seed(0)
scene = {"ref_date": batch["ref_date"][:1].contiguous()}
for s in sources:
    q = geo["q"][s.src]
    scene[s.src] = torch.rand(1, s.Dates, s.C_src, U * q, U * q, device=dev, generator=g)
    scene[f"{s.src}_dates"] = batch[f"{s.src}_dates"][:1].contiguous()
table = hip.scene_table(1, hip.scene_windows(U, U, W, half), B)
n_batches = table.shape[0]
(t, hb), = [(t, hb) for t, hb in eng.hb.items() if hb["kind"] == "segment"]
C, S, qt = hb["C"], eng.ref["G"] * hb["P"], geo["qt"][t]
Hc = U * qt
profile = torch.from_numpy(hip.blend_profile(S, "linear")).to(dev)
w2d = profile[:, None] * profile[None, :]
acc_t, wsum_t = torch.zeros(1, C, Hc, Hc, device=dev), torch.zeros(1, Hc, Hc, device=dev)


def torch_glue():
    acc_t.zero_()
    wsum_t.zero_()
    for rows in table.tolist():
        wb = {"ref_date": scene["ref_date"].expand(B, 1, 3).contiguous()}
        for s in sources:
            q = geo["q"][s.src]
            wb[s.src] = torch.stack([scene[s.src][n, :, :, y * q: y * q + s.S, x * q: x * q + s.S] for n, y, x, _ in rows])
            wb[f"{s.src}_dates"] = scene[f"{s.src}_dates"].expand(B, -1, 3).contiguous()
        prob = eng.predict(wb, probs=True)[t].probs
        for b, (n, y, x, on) in enumerate(rows):
            if on:
                acc_t[n, :, y * qt: y * qt + S, x * qt: x * qt + S].add_(prob[b, 0] * w2d)
                wsum_t[n, y * qt: y * qt + S, x * qt: x * qt + S].add_(w2d)
    mean = acc_t / wsum_t[:, None]
    conf, cls = mean.max(dim=1)
    return cls.to(torch.uint8), conf, mean


whole = alternate({"scene": lambda: eng.predict_scene(scene, probs=True), "torch_glue": torch_glue,
                   "predict": lambda: eng.predict(batch, probs=True)}, args.rounds)     # (the glue's own call: one captured segment serves both)
got, want = eng.predict_scene(scene, probs=True)[t], torch_glue()
agree = float((got.cls == want[0]).float().mean())
max_diff = float((got.probs - want[2]).abs().max())

# the three launches on the engine's own operands of that scene (the canvas keeps accumulating: values do not matter here)
ps, pb = eng._ps, eng._pb[t]
cv = ps["canvas"][t]
rows0 = table[0]
_, g_, P, ld, _, _ = eng._head_geometry(hb)


def gather():
    for s in sources:
        img = scene[s.src]
        hip.window_gather(img, ps["win"][s.src], ps["cur"], rows0, B, 1, s.Dates * s.C_src, img.shape[3], img.shape[4], s.S, geo["q"][s.src])


ps["cur"].copy_(torch.from_numpy(rows0).to(dev))
kern = alternate({
    "gather": gather,
    "blend": lambda: hip.predict_blend(pb["prob"], 1.0, profile, ps["cur"], rows0, cv["acc"], cv["wsum"], B, 1, C, S, qt, Hc, Hc),
    "finish": lambda: hip.predict_blend_finish(cv["acc"], cv["wsum"], cv["cls"], cv["conf"], cv["acc"], 1, C, Hc * Hc),
    "view": lambda: hip.predict_view(hb["logits"], None, hip.PREDICT_SOFTMAX, pb["prob"], False, pb["cls"], pb["conf"], B, g_, P, C, ld=ld),
}, args.kernel_rounds)
win_pix = B * S * S
nbytes = {"gather": 8 * sum(B * s.Dates * s.C_src * s.S * s.S for s in sources), "blend": hip.scene_blend_bytes(rows0, C, S, qt),
          "finish": Hc * Hc * (4 * (C + 1) + 4 * C + 5), "view": win_pix * (8 * C + 5)}
for k, nb in nbytes.items():
    kern[k]["MB"] = round(nb / 1e6, 1)
    kern[k]["GBps"] = round(nb / kern[k]["median_ms"] / 1e6, 1)
new_ms = n_batches * (kern["gather"]["median_ms"] + kern["blend"]["median_ms"]) + kern["finish"]["median_ms"]
out = {"shape": dict(B=B, W=W, units=U, windows=args.windows ** 2, batches=n_batches, C=C, S=S, canvas=Hc,
                     canvas_MB=round(4 * C * Hc * Hc / 1e6, 1), q=geo["q"], qt=geo["qt"]),
       "whole": whole, "ms_per_batch": {k: round(whole[k]["median_ms"] / n_batches, 3) for k in ("scene", "torch_glue")},
       "predict_ms_per_batch": whole["predict"]["median_ms"],
       "kernels": kern, "new_launches_ms": round(new_ms, 3), "share": round(new_ms / whole["scene"]["median_ms"], 4),
       "vs_torch_glue": dict(cls_agree=round(agree, 6), probs_max_abs_diff=max_diff)}
line = json.dumps(out)
print(line, flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")
