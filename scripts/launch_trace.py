"""Launch trace of a tiny golden case: one JSON line per device operation of three training steps, for comparing two
checkouts.  Host-side refactors of the engines must leave it byte-identical (profiles/HISTORY.md).

    MAESTRO_WGRAD=deferred python scripts/launch_trace.py c3_aerial_s2 --out a.jsonl
    python scripts/launch_trace.py sup_flair_seg --phase finetune --out b.jsonl

Sequence (eager launches, MAESTRO_GRAPHS=0): forward, zero_grad, backward; the same again; forward, backward without a
zero_grad.  A record holds the stream (numbered by first appearance) and either the C entry name with every scalar argument
(``hip.call`` / ``hip._gemm_tile`` / an ``OrderedReduce`` launch), the problem list handed to a ``GroupedTN`` / ``ColsumBatch`` /
``OrderedReduce`` constructor, or a torch operator touching device memory (``TorchDispatchMode``; views are not device operations
and are left out).  Tensors are described by dtype, shape, strides, storage offset and their storage numbered by first appearance:
addresses differ between runs, the order in which buffers are first used does not.
"""

from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
from pathlib import Path

os.environ["MAESTRO_GRAPHS"] = "0"
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402
from torch.utils._python_dispatch import TorchDispatchMode  # noqa: E402
from torch.utils._pytree import tree_flatten  # noqa: E402

import maestro_amd.conf as conf  # noqa: E402
from maestro_amd import hip  # noqa: E402
from maestro_amd.ssl import mae as pmae  # noqa: E402
from oracle import mae as om  # noqa: E402
from oracle.gen_golden import build_datasets, case_table, init_weights, make_batch, resize_case_table  # noqa: E402


class Trace:
    def __init__(self, out) -> None:
        self.out, self.storages, self.streams, self.on = out, {}, {}, False

    def tensor(self, t: torch.Tensor) -> dict:
        d = {"dtype": str(t.dtype), "shape": list(t.shape), "strides": list(t.stride()), "offset": t.storage_offset()}
        if t.is_cuda:
            d["storage"] = self.storages.setdefault(t.untyped_storage().data_ptr(), len(self.storages))
        else:
            d["storage"] = "host"
        return d

    def value(self, a):
        if isinstance(a, torch.Tensor):
            return self.tensor(a)
        if isinstance(a, ctypes._SimpleCData):
            return a.value
        if a is None or isinstance(a, (bool, int, float, str)):
            return a
        if isinstance(a, (list, tuple)):
            return [self.value(v) for v in a]
        return str(a)

    def write(self, **rec) -> None:
        if self.on:
            s = torch.cuda.current_stream().cuda_stream
            rec["stream"] = self.streams.setdefault(s, len(self.streams))
            self.out.write(json.dumps(rec, sort_keys=True) + "\n")

    def mark(self, what: str) -> None:
        self.out.write(json.dumps({"mark": what}) + "\n")


class DeviceOps(TorchDispatchMode):
    def __init__(self, trace: Trace) -> None:
        super().__init__()
        self.trace = trace

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        if not func.is_view:
            flat_in, flat_out = tree_flatten((args, kwargs or {}))[0], tree_flatten(out)[0]
            if any(isinstance(t, torch.Tensor) and t.is_cuda for t in flat_in + flat_out):
                self.trace.write(op=str(func), args=[self.trace.value(a) for a in flat_in],
                                 out=[self.trace.value(a) for a in flat_out])
        return out


def install(trace: Trace) -> None:
    call, gemm_tile = hip.call, hip._gemm_tile

    def traced_call(name, *args):
        trace.write(entry=name, args=[trace.value(a) for a in args])
        return call(name, *args)

    def traced_gemm_tile(*args):
        trace.write(entry="_gemm_tile", args=[trace.value(a) for a in args])
        return gemm_tile(*args)

    hip.call, hip._gemm_tile = traced_call, traced_gemm_tile
    for cls in (hip.GroupedTN, hip.ColsumBatch, hip.OrderedReduce):
        def init(self, problems, device, _cls=cls, _init=cls.__init__):
            trace.write(ctor=_cls.__name__, problems=[trace.value(p) for p in problems])
            _init(self, problems, device)
        cls.__init__ = init
    launch = hip.OrderedReduce.launch           # (binds the library itself, not hip.call)

    def traced_launch(self):
        trace.write(entry="mh_reduce_ordered", args=[trace.value(a) for a in (self.table, self.n, self.blocks, self.n_blocks)])
        return launch(self)

    hip.OrderedReduce.launch = traced_launch


def pretrain_case(name: str, dev):
    case = {**case_table(), **resize_case_table()}[name]
    ds = build_datasets(case, conf)
    kw = dict(fusion_mode=case["fusion"], inter_depth=case["inter_depth"], model="mae", num_levels=1, type_head="attentive",
              fac_abs_enc=1.0, fac_date_enc=1.0, interpolate=case.get("interpolate", "nearest"), **case["model_kw"])
    mask_cfg = conf.MaskConfig(**case.get("mask_kw", {}))
    oracle = om.build_oracle(ds, mask_cfg, model_size=case["size"], **kw)
    init_weights(oracle, case["seed"])
    model = getattr(pmae, f"mae_{case['size']}")(datasets=ds, mask=mask_cfg, **kw)
    model.load_state_dict(oracle.state_dict(), strict=True)
    batch = make_batch(ds.dataset, case["B"], case["seed"], stress=case.get("stress", False), sizes=case.get("raster_size"))
    eng = model.engine(case["B"], dev, loss="l2_norm")
    torch.manual_seed(7)
    noise, struct = eng.draw_masks()
    dbatch = {k: v.to(dev) for k, v in batch.items()}
    return eng, lambda: eng.forward(dbatch, noise=noise, struct=struct)


def supervised_case(name: str, phase: str, dev):
    from tests.test_oracle_sup import build_sup_case
    case, ds, oracle, _, batch = build_sup_case(name)
    model = getattr(pmae, f"mae_{case['size']}")(
        datasets=ds, mask=conf.MaskConfig(), interpolate="nearest", fusion_mode=case["fusion"], inter_depth=case["inter_depth"],
        model="mae", num_levels=1, type_head=case["type_head"], fac_abs_enc=1.0, fac_date_enc=1.0, **case["model_kw"])
    model.load_state_dict(oracle.state_dict(), strict=True)
    eng = model.sup_engine(case["B"], dev, phase)
    dbatch = {k: v.to(dev) for k, v in batch.items()}
    return eng, lambda: eng.forward(dbatch)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("case")
    ap.add_argument("--phase", choices=("probe", "finetune"), help="supervised cases (sup_*)")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    if a.case.startswith("sup_"):
        eng, forward = supervised_case(a.case, a.phase or "finetune", dev)
    else:
        eng, forward = pretrain_case(a.case, dev)
    with open(a.out, "w") as out:
        trace = Trace(out)
        install(trace)
        with DeviceOps(trace):
            trace.on = True
            for it, zero in enumerate((True, True, False)):
                trace.mark(f"step {it}: forward")
                forward()
                if zero:
                    trace.mark(f"step {it}: zero_grad")
                    eng.zero_grad()
                trace.mark(f"step {it}: backward")
                eng.backward()
            torch.cuda.synchronize()
            trace.on = False
    print(f"{a.case}{'/' + a.phase if a.phase else ''}: trace written to {a.out}")


if __name__ == "__main__":
    main()
