"""Prediction metrics without a GPU: the confusion-matrix calls of include/maestro_hip.h (exports, argument checks), the arithmetic of
``MonoLabelMetric`` / ``MultiLabelMetric.compute`` against values worked out here, the state dict, and ``compute`` over two gloo
ranks."""

import ctypes
import math
import os
import re
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import maestro_amd.conf as conf
from maestro_amd import hip
from maestro_amd.train.metric import MonoLabelMetric, MultiLabelMetric, average_precision

ROOT = Path(__file__).resolve().parents[1]
NAMES = ("mh_confusion_ce", "mh_confusion_bce")


# ------------------------------------------------------------------------------------------------------------- C ABI
def test_metrics_names_are_declared_and_exported():
    header = (ROOT / "include" / "maestro_hip.h").read_text()
    declared = set(re.findall(r"\b(mh_[a-z0-9_]+)\s*\(", header))
    lib = hip.lib()
    for name in NAMES:
        assert name in declared, f"{name} is not declared in include/maestro_hip.h"
        assert hasattr(lib, name), f"{name} is declared but not exported"


def _err():
    return hip.lib().mh_last_error().decode()


FAKE = ctypes.c_void_p(0x10000)      # never dereferenced: every call below is rejected before any launch
NULL = ctypes.c_void_p(0)


def _ce(logits=FAKE, target=FAKE, tbytes=8, missing=-1, cm=FAKE, B=2, g=2, P=2, C=5, ld=20):  # noqa: N803
    return hip.lib().mh_confusion_ce(logits, target, tbytes, missing, cm, B, g, P, C, ld, NULL)


def _bce(logits=FAKE, target=FAKE, missing=-1.0, thr=0.0, cm=FAKE, B=3, C=4):  # noqa: N803
    return hip.lib().mh_confusion_bce(logits, target, missing, thr, cm, B, C, NULL)


@pytest.mark.parametrize("kw", [dict(logits=NULL), dict(target=NULL), dict(cm=NULL), dict(C=1), dict(C=129), dict(C=0),
                                dict(tbytes=3), dict(tbytes=0), dict(tbytes=16), dict(ld=19), dict(B=0), dict(g=0), dict(P=0)],
                         ids=lambda kw: "-".join(f"{k}={'null' if v is NULL else v}" for k, v in kw.items()))
def test_confusion_ce_rejects_bad_arguments_before_any_launch(kw):
    assert _ce(**kw) == -1
    assert "mh_confusion_ce" in _err()


@pytest.mark.parametrize("kw", [dict(logits=NULL), dict(target=NULL), dict(cm=NULL), dict(C=0), dict(C=1025), dict(B=0)],
                         ids=lambda kw: "-".join(f"{k}={'null' if v is NULL else v}" for k, v in kw.items()))
def test_confusion_bce_rejects_bad_arguments_before_any_launch(kw):
    assert _bce(**kw) == -1
    assert "mh_confusion_bce" in _err()


def test_wrappers_have_no_cpu_fallback():
    m = MonoLabelMetric("classif", 4)
    with pytest.raises(hip.HipExtensionError):
        m.update(torch.zeros(3, 4), torch.zeros(3, dtype=torch.long))
    ml = MultiLabelMetric(3)
    with pytest.raises(hip.HipExtensionError):
        ml.update(torch.zeros(2, 3), torch.zeros(2, 3))
    assert hip.logit_threshold(0.5) == 0.0 and abs(hip.logit_threshold(0.3) - math.log(3 / 7)) < 1e-15


# ------------------------------------------------------------------------------------------------------------- mono-label compute
def test_mono_compute_excludes_classes_absent_from_the_targets():
    m = MonoLabelMetric("segment", 3)
    # rows = targets, columns = predictions; class 2 never occurs as a target (but is predicted twice)
    m.cm.copy_(torch.tensor([[5, 1, 2], [3, 4, 0], [0, 0, 0]]))
    out = m.compute()
    assert list(out) == ["overall_accuracy", "average_f1", "average_iou", "confusion_matrix"]
    # class 0: TP 5, FP 3, FN 3;  class 1: TP 4, FP 1, FN 3;  class 2 (TP + FN = 0) is left out of the means
    f1 = (10 / 16 + 8 / 12) / 2
    iou = (5 / 11 + 4 / 8) / 2
    assert out["overall_accuracy"].dtype == torch.float64
    assert abs(float(out["overall_accuracy"]) - 9 / 15) < 1e-15
    assert abs(float(out["average_f1"]) - f1) < 1e-15 and abs(float(out["average_iou"]) - iou) < 1e-15
    assert out["confusion_matrix"].dtype == torch.int64 and torch.equal(out["confusion_matrix"], m.cm)


def test_mono_compute_counts_a_class_that_is_never_predicted():
    m = MonoLabelMetric("segment", 3)
    m.cm.copy_(torch.tensor([[4, 0, 0], [1, 3, 0], [2, 1, 0]]))     # class 2: targets exist, no prediction -> F1 = IoU = 0, counted
    out = m.compute()
    f1 = (8 / 11 + 6 / 8 + 0.0) / 3
    iou = (4 / 7 + 3 / 5 + 0.0) / 3
    assert abs(float(out["average_f1"]) - f1) < 1e-15 and abs(float(out["average_iou"]) - iou) < 1e-15
    assert abs(float(out["overall_accuracy"]) - 7 / 11) < 1e-15


def test_mono_compute_classif_keys_change_detect_and_empty_matrix():
    m = MonoLabelMetric("classif", 4)
    m.cm.copy_(torch.diag(torch.tensor([1, 2, 3, 4])))
    out = m.compute()
    assert list(out) == ["overall_accuracy", "confusion_matrix"] and float(out["overall_accuracy"]) == 1.0
    m.reset()
    assert int(m.cm.sum()) == 0
    out = m.compute()                                               # 0 / 0: NaN, not an exception
    assert math.isnan(float(out["overall_accuracy"]))
    e = MonoLabelMetric("segment", 3).compute()
    assert math.isnan(float(e["overall_accuracy"])) and math.isnan(float(e["average_f1"])) and math.isnan(float(e["average_iou"]))
    cd = MonoLabelMetric("change_detect", None, threshold_detect=0.4)
    assert cd.num_classes == 2 and tuple(cd.cm.shape) == (2, 2) and "average_iou" in cd.metric_names
    cd.cm.copy_(torch.tensor([[6, 2], [1, 3]]))                      # [[TN, FP], [FN, TP]]
    out = cd.compute()
    assert abs(float(out["average_iou"]) - (6 / 9 + 3 / 6) / 2) < 1e-15
    with pytest.raises(ValueError):
        MonoLabelMetric("multilabel_classif", 3)


# ------------------------------------------------------------------------------------------------------------- multilabel compute
def _ap_numpy(scores, y):
    """fp64 loop over the distinct thresholds, highest first: AP = sum (R_k - R_{k-1}) P_k."""
    scores, y = np.asarray(scores, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n_pos = y.sum()
    if n_pos == 0:
        return float("nan")
    ap, r_prev = 0.0, 0.0
    for thr in sorted(set(scores.tolist()), reverse=True):
        sel = scores >= thr
        tp = y[sel].sum()
        prec, rec = tp / sel.sum(), tp / n_pos
        ap += (rec - r_prev) * prec
        r_prev = rec
    return ap


def _multilabel_case():
    g = torch.Generator().manual_seed(5)
    n = 41
    preds = torch.rand(n, 4, generator=g)
    preds[:, 0] = (preds[:, 0] * 5).round() / 5             # label 0: heavily tied scores
    target = (torch.rand(n, 4, generator=g) > 0.6).long()
    target[:, 1] = 0                                       # label 1: no positive -> AP NaN, F1 0 / 0 = NaN when never predicted
    target[:, 2] = 1                                       # label 2: all positives -> AP 1
    return preds, target


def _multilabel_expected(preds, target, thr=0.5):
    p, t = preds.numpy().astype(np.float64), target.numpy()
    cm = np.zeros((p.shape[1], 2, 2), dtype=np.int64)
    for lbl in range(p.shape[1]):
        for ti, pi in zip(t[:, lbl], p[:, lbl] > thr):
            cm[lbl, ti, int(pi)] += 1
    tp, fp, fn = cm[:, 1, 1].astype(np.float64), cm[:, 0, 1].astype(np.float64), cm[:, 1, 0].astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        f1 = 2 * tp / (2 * tp + fp + fn)
        w = (tp + fn) / (tp + fn).sum()
        ap = np.array([_ap_numpy(p[:, lbl], t[:, lbl]) for lbl in range(p.shape[1])])
        want = {"average_f1": np.nanmean(f1), "average_ap": np.nanmean(ap), "weighted_f1": np.nansum(f1 * w),
                "weighted_ap": np.nansum(ap * w)}
    return cm, ap, want


def test_multilabel_compute_matches_an_fp64_loop_over_distinct_thresholds():
    preds, target = _multilabel_case()
    preds[:, 1] = preds[:, 1] * 0.4                        # label 1 is never predicted either: its F1 is NaN and is skipped too
    cm, ap, want = _multilabel_expected(preds, target)
    assert math.isnan(ap[1]) and ap[2] == 1.0 and len(set(preds[:, 0].tolist())) <= 6
    got_ap = average_precision(preds, target)
    assert got_ap.dtype == torch.float64 and math.isnan(float(got_ap[1]))
    for lbl in (0, 2, 3):
        assert abs(float(got_ap[lbl]) - ap[lbl]) < 1e-12
    m = MultiLabelMetric(4)
    m.cm.copy_(torch.from_numpy(cm))
    m.preds, m.target = [preds[:17], preds[17:]], [target[:17], target[17:]]      # two updates' worth
    out = m.compute()
    assert list(out) == ["average_f1", "average_ap", "weighted_f1", "weighted_ap"]
    for k, v in want.items():
        assert abs(float(out[k]) - v) < 1e-12, (k, float(out[k]), v)
    m.reset()
    assert int(m.cm.sum()) == 0 and m.preds == [] and m.target == []
    out = m.compute()                                      # nothing seen: NaN means, zero sums, no exception
    assert math.isnan(float(out["average_ap"])) and float(out["weighted_ap"]) == 0.0


def test_average_precision_small_cases_by_hand():
    # scores 0.9 (+), 0.8 (-), 0.8 (+), 0.1 (-): thresholds 0.9 -> P 1, R 1/2; 0.8 -> P 2/3, R 1; 0.1 -> P 1/2, R 1
    ap = average_precision(torch.tensor([[0.9], [0.8], [0.8], [0.1]]), torch.tensor([[1], [0], [1], [0]]))
    assert abs(float(ap[0]) - (0.5 * 1.0 + 0.5 * 2 / 3)) < 1e-15
    assert math.isnan(float(average_precision(torch.zeros(0, 1), torch.zeros(0, 1, dtype=torch.long))[0]))


# ------------------------------------------------------------------------------------------------------------- module surface
def test_ssl_module_has_the_reference_metrics_and_no_metric_key_in_its_state_dict():
    from maestro_amd.train.model import MeanMetric, SSLModule
    ds = conf.DatasetsConfig(root_dir=None, name_dataset="treesatai_ts", treesatai_ts=conf.TreeSatAITSConfig(rel_dir=""))
    assert ds.dataset.targets, "a supervised dataset config is needed here"
    mod = SSLModule(datasets=ds, mask=conf.MaskConfig(), interpolate="nearest", fusion_mode="group", inter_depth=0, model="mae",
                    model_size="tiny")
    for name, target in ds.dataset.targets.items():
        for stage in ("train", "val", "test"):
            metric = mod.metrics[f"{name}_{stage}"]
            want = MultiLabelMetric if target.type_target == "multilabel_classif" else MonoLabelMetric
            assert isinstance(metric, want) and metric.cm.dtype == torch.int64 and int(metric.cm.sum()) == 0
    assert all(isinstance(mod.metrics[f"loss_{k}_{s}"], MeanMetric) for k in ("rec", "pred") for s in ("train", "val", "test"))
    assert len({id(m) for m in mod.metrics.values()}) == len(mod.metrics)      # one object per target and stage
    keys = list(mod.state_dict())
    assert keys and not [k for k in keys if k.startswith("metrics") or k.endswith(".cm")]


# ------------------------------------------------------------------------------------------------------------- two gloo ranks
def _free_port() -> int:
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank_states(rank):
    """Hand-made states of one rank: unequal list lengths (rank 1 holds one update only, and a mono matrix of its own)."""
    preds, target = _multilabel_case()
    cut = 29
    p, t = (preds[:cut], target[:cut]) if rank == 0 else (preds[cut:], target[cut:])
    cm, _, _ = _multilabel_expected(p, t)
    mono = torch.tensor([[5, 1, 2], [3, 4, 0], [0, 0, 0]]) if rank == 0 else torch.tensor([[1, 0, 0], [0, 2, 1], [1, 0, 3]])
    lists = ([p[:11], p[11:]], [t[:11], t[11:]]) if rank == 0 else ([p], [t])
    return torch.from_numpy(cm), lists, mono


def _metric_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    cm, (preds, target), mono = _rank_states(rank)
    ml = MultiLabelMetric(4)
    ml.cm.copy_(cm)
    ml.preds, ml.target = preds, target
    mm = MonoLabelMetric("segment", 3)
    mm.cm.copy_(mono)
    got_ml = {k: float(v) for k, v in ml.compute().items()}
    got_mm = mm.compute()
    out.put((rank, got_ml, {k: (v.tolist() if k == "confusion_matrix" else float(v)) for k, v in got_mm.items()},
             mm.cm.tolist() == mono.tolist()))
    dist.destroy_process_group()


def test_compute_over_two_gloo_ranks_equals_the_single_process_answer():
    preds, target = _multilabel_case()
    cm, _, want_ml = _multilabel_expected(preds, target)
    single = MonoLabelMetric("segment", 3)
    single.cm.copy_(_rank_states(0)[2] + _rank_states(1)[2])
    want_mm = single.compute()
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_metric_worker, args=(r, 2, port, out)) for r in range(2)]
    for p in procs:
        p.start()
    res = [out.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert sorted(r[0] for r in res) == [0, 1]
    for rank, got_ml, got_mm, local_kept in res:
        for k, v in want_ml.items():
            assert abs(got_ml[k] - v) < 1e-12, (rank, k, got_ml[k], v)
        assert got_mm["confusion_matrix"] == want_mm["confusion_matrix"].tolist()
        for k in ("overall_accuracy", "average_f1", "average_iou"):
            assert abs(got_mm[k] - float(want_mm[k])) < 1e-15, (rank, k)
        assert local_kept, "compute() must not fold the other ranks' counts into the local state"
