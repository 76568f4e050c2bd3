"""GroupNorm backward of the patch embed (statistics pass + apply pass) at the C3 step's two launches and a 1024-wide one, us per
call, in its three forms: mh_embed_finish_bwd (plain), mh_embed_finish_bwd_det (deterministic mode) and mh_embed_finish_bwd_ends (the
default step: gradient of the visible rows through the position map, a quarter of the rows visible, conv bias partial rows).
The last line is the same numbers as JSON ({"form B D L E": us}), for A/B runs through scripts/ab_lib.py."""
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from maestro_amd import hip  # noqa: E402

dev = torch.device("cuda:0")


def timed(fn, reps=100, windows=5):
    """Median over `windows` of the device time of `reps` back-to-back calls."""
    for _ in range(10):
        fn()
    out = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / reps)
    return sorted(out)[len(out) // 2]


results = {}
for (B, D, L, E) in ((32, 1, 1024, 768), (32, 16, 25, 768), (32, 4, 225, 1024)):
    Lg, BD = D * L, B * D
    g = torch.Generator(device=dev).manual_seed(L)
    dxg = torch.randn(B, Lg, E, device=dev, generator=g)
    y = torch.randn(BD, L, E, device=dev, generator=g)
    stats = torch.rand(BD, 2, device=dev, generator=g) + 0.5
    gamma = torch.randn(E, device=dev, generator=g)
    dyc = torch.empty(BD * L, E, dtype=torch.bfloat16, device=dev)
    dg, db, sums = torch.zeros(E, device=dev), torch.zeros(E, device=dev), torch.zeros(BD, 2, device=dev)
    rows = hip.embed_bwd_partial_rows(BD, L)
    part, blk = torch.empty(rows, 2 * E, device=dev), torch.empty(rows, 2, device=dev)
    n_vis = Lg // 4                       # the visible rows of a sample: every fourth group position
    inv = torch.full((B, Lg), -1, dtype=torch.int32, device=dev)
    inv[:, ::4][:, :n_vis] = torch.arange(n_vis, dtype=torch.int32, device=dev)
    dx = dxg[:, ::4][:, :n_vis].contiguous()
    cs = torch.empty(hip.embed_bwd_cs_rows(BD * L), E, device=dev)
    forms = {
        "plain": lambda: hip.embed_finish_bwd(dxg, y, stats, gamma, dyc, dg, db, sums, B, D, L, E, 0, Lg),
        "det": lambda: hip.embed_finish_bwd_det(dxg, y, stats, gamma, dyc, part, blk, sums, B, D, L, E, 0, Lg),
        "ends": lambda: hip.embed_finish_bwd_ends(dx, inv, n_vis, y, stats, gamma, dyc, dg, db, sums, cs, B, D, L, E, 0, Lg),
    }
    for name, fn in forms.items():
        t = timed(fn)
        vis = 0.25 if name == "ends" else 1.0       # bytes over both passes: y twice, the gradient rows twice, bf16 dyc once
        mb = BD * L * E * (4 + 4 + 2 + vis * (4 + 4)) / 1e6
        results[f"{name} {B} {D} {L} {E}"] = round(t, 2)
        print(f"{name:5s} B {B} D {D} L {L} E {E}: {t:7.1f} us  ({mb:.0f} MB over both passes: {mb / t * 1e3:.0f} GB/s)", flush=True)
print(json.dumps(results))
