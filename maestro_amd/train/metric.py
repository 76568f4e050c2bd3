"""Prediction metrics of the probe / finetune branch: ``maestro/train/metric.py`` on device-side confusion matrices.

The reference keeps, per target and stage (``maestro/train/base.py:32-50``), a torchmetrics ``Metric`` whose ``update`` turns the
selected logits into predictions and adds ``torchmetrics.functional.confusion_matrix`` to an int64 state (``metric.py:63-77`` and
``132-160``).  Here ``update`` is ONE kernel launch on logits that are already resident (``mh_confusion_ce`` / ``mh_confusion_bce``,
``include/maestro_hip.h``): no host read, no synchronisation, no intermediate tensor.  ``compute`` is the reference's
arithmetic on that matrix, in fp64.  Like ``MeanMetric`` (``train/model.py``) the classes are ``nn.Module`` stand-ins: torchmetrics
is not a dependency.  ``cm`` is a non-persistent buffer, so ``state_dict()`` keeps exactly the reference's keys (torchmetrics'
states are not persistent either).
"""

from __future__ import annotations

import torch
from torch import nn

from maestro_amd import hip


def _dist_world() -> int:
    import torch.distributed as dist
    return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1


def _dist_device(fallback: torch.device) -> torch.device:
    """The device collectives run on.  NCCL (= RCCL) groups only reduce device tensors: always this rank's current GPU, also for a
    rank whose states are still on the CPU (the rule ``MeanMetric.compute`` states); other backends (gloo) take the CPU."""
    import torch.distributed as dist
    if dist.get_backend() == "nccl":
        return torch.device("cuda", torch.cuda.current_device())
    return torch.device("cpu") if fallback.type != "cpu" else fallback


def _reduced_cm(cm: torch.Tensor) -> torch.Tensor:
    """``dist_reduce_fx="sum"`` (``metric.py:57-61, 126-130``)."""
    if _dist_world() == 1:
        return cm
    import torch.distributed as dist
    t = cm.detach().to(_dist_device(cm.device), copy=True)
    dist.all_reduce(t)
    return t


def _gathered_rows(rows: torch.Tensor) -> torch.Tensor:
    """``dist_reduce_fx="cat"`` (``metric.py:124-125``) for ``[n_rank, C]`` states with a different ``n`` on every rank: exchange
    the lengths, pad to the longest, all-gather, trim."""
    if _dist_world() == 1:
        return rows
    import torch.distributed as dist
    dev = _dist_device(rows.device)
    rows = rows.to(dev)
    world = dist.get_world_size()
    lens = [torch.zeros(1, dtype=torch.int64, device=dev) for _ in range(world)]
    dist.all_gather(lens, torch.tensor([rows.shape[0]], dtype=torch.int64, device=dev))
    lens = [int(n) for n in lens]
    padded = torch.zeros(max(max(lens), 1), rows.shape[1], dtype=rows.dtype, device=dev)
    padded[: rows.shape[0]] = rows
    parts = [torch.empty_like(padded) for _ in range(world)]
    dist.all_gather(parts, padded)
    return torch.cat([p[:n] for p, n in zip(parts, lens)])


_integer_targets = hip.integer_targets     # the one widening rule, shared with hip.count_valid / ce_loss / confusion_ce


class MonoLabelMetric(nn.Module):
    """``maestro/train/metric.py:19-108``: a ``[num_classes, num_classes]`` int64 confusion matrix, rows = targets, columns =
    predictions (torchmetrics' orientation: ``metric.py:83-84`` sums over dim 0 for the false positives)."""

    def __init__(self, type_target: str, num_classes: int | None, threshold_detect: float = 0.5) -> None:
        super().__init__()
        self.type_target, self.threshold_detect = type_target, threshold_detect
        if type_target == "classif":                                                  # metric.py:34-37
            self.task, self.num_classes = "multiclass", num_classes
            self.metric_names = ["overall_accuracy", "confusion_matrix"]
        elif type_target == "segment":                                                # metric.py:38-46
            self.task, self.num_classes = "multiclass", num_classes
            self.metric_names = ["overall_accuracy", "average_f1", "average_iou", "confusion_matrix"]
        elif type_target == "change_detect":                                          # metric.py:47-55
            self.task, self.num_classes = "binary", 2
            self.metric_names = ["overall_accuracy", "average_f1", "average_iou", "confusion_matrix"]
        else:
            raise ValueError(f"Invalid target type {type_target!r}. Expected 'classif', 'segment' or 'change_detect'")
        # metric.py:57-61 (add_state: not part of the state dict)
        self.register_buffer("cm", torch.zeros(self.num_classes, self.num_classes, dtype=torch.long), persistent=False)

    def update(self, logits: torch.Tensor, targets: torch.Tensor, *, g: int = 1, P: int = 1, ld: int | None = None,  # noqa: N803
               missing_val=None) -> None:
        """``metric.py:63-77`` as one launch that adds to ``cm`` (which moves to the logits' device first).

        Engine form: ``logits`` is the head's patch-layout buffer ``[B*g*g, ld >= P*P*C]`` fp32 and ``targets`` the ``[B, S, S]``
        raster (``S = g*P``, any leading 1-dimensions), with the target's ``missing_val``: the selection of ``base.py:120-138`` happens
        in the kernel.  Reference form (``g = P = 1``): ``logits [N, C]``, ``targets [N]``, already selected.  Targets outside
        ``[0, C)`` are never counted.  ``change_detect``: ``logits [N]`` (or ``[N, 1]``), ``targets [N]`` in {0, 1}."""
        if self.cm.device != logits.device:
            self.cm = self.cm.to(logits.device)
        if logits.dtype != torch.float32:
            raise ValueError("MonoLabelMetric.update: fp32 logits expected")
        if self.task == "binary":                                                    # metric.py:68-69
            n = targets.numel()
            if logits.numel() != n or not logits.is_contiguous():
                raise ValueError("change_detect: one contiguous logit per target expected")
            tgt = targets.to(torch.float32).contiguous()
            hip.confusion_bce(logits, tgt, float("nan") if missing_val is None else missing_val, self.threshold_detect, self.cm, n, 1)
            return
        C = self.num_classes  # noqa: N806
        ld = logits.stride(0) if ld is None else ld
        S = g * P  # noqa: N806
        if targets.numel() % (S * S) or logits.stride(-1) != 1:
            raise ValueError(f"MonoLabelMetric.update: targets of {targets.numel()} entries are not [B, {S}, {S}] rasters")
        B = targets.numel() // (S * S)  # noqa: N806
        need = (B * g * g - 1) * ld + P * P * C
        if ld < P * P * C or logits.numel() and (logits.storage_offset() + need > logits.untyped_storage().nbytes() // 4):
            raise ValueError(f"MonoLabelMetric.update: logits do not hold [{B * g * g}, {P * P * C}] at ld {ld}")
        hip.confusion_ce(logits, _integer_targets(targets), C if missing_val is None else missing_val, self.cm, B, g, P, C, ld)

    def compute(self) -> dict:
        """``metric.py:79-108``; the divisions in fp64 (``0 / 0 = NaN`` as in the reference, never an exception)."""
        cm_int = _reduced_cm(self.cm)
        cm = cm_int.double()
        overall_acc = cm.trace() / cm.sum()                              # OA       metric.py:81
        true_pos = torch.diag(cm)                                        # TP       metric.py:82
        false_pos = cm.sum(0) - true_pos                                 # FP       metric.py:83
        false_neg = cm.sum(1) - true_pos                                 # FN       metric.py:84
        per_class_f1 = (2 * true_pos) / (2 * true_pos + false_pos + false_neg)      # metric.py:86
        per_class_iou = true_pos / (true_pos + false_pos + false_neg)               # metric.py:87
        valid = (true_pos + false_neg).nonzero().squeeze(dim=1)                     # metric.py:89
        metrics = {"overall_accuracy": overall_acc,
                   "average_f1": torch.index_select(per_class_f1, 0, valid).mean(),    # metric.py:92-96
                   "average_iou": torch.index_select(per_class_iou, 0, valid).mean(),  # metric.py:97-101
                   "confusion_matrix": cm_int}
        return {k: v for k, v in metrics.items() if k in self.metric_names}          # metric.py:104-108

    def reset(self) -> None:
        self.cm.zero_()


def average_precision(preds: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """Per-label average precision of scores ``preds [N, L]`` against ``target [N, L]`` in {0, 1}; fp64 ``[L]``.

    The exact-curve definition (torchmetrics' ``thresholds=None``): per label, with the DISTINCT scores in descending order,
    ``AP = sum_k (R_k - R_{k-1}) P_k``, ``R_0 = 0``, where ``P_k`` / ``R_k`` are precision / recall of "score >= k-th distinct
    value" -- equal scores form one threshold.  A label without a positive gives NaN.  Plain torch ops on the tensors' device."""
    n, n_labels = preds.shape
    if n == 0:
        return torch.full((n_labels,), float("nan"), dtype=torch.float64, device=preds.device)
    score, order = torch.sort(preds, dim=0, descending=True, stable=True)
    hit = torch.gather(target, 0, order).double()
    tps = hit.cumsum(0)                                                        # true positives among the i + 1 highest scores
    rank = torch.arange(1, n + 1, dtype=torch.float64, device=preds.device).unsqueeze(1)
    last = torch.ones_like(score, dtype=torch.bool)                            # the last entry of every run of equal scores
    last[:-1] = score[:-1] != score[1:]
    at_thr = torch.where(last, tps, torch.zeros_like(tps))
    prev = torch.zeros_like(tps)
    prev[1:] = torch.cummax(at_thr, dim=0).values[:-1]                         # tps at the previous threshold (tps never decreases)
    n_pos = tps[-1]
    terms = torch.where(last, (tps - prev) / n_pos * (tps / rank), torch.zeros_like(tps))
    ap = terms.sum(0)
    return torch.where(n_pos > 0, ap, torch.full_like(ap, float("nan")))


class MultiLabelMetric(nn.Module):
    """``maestro/train/metric.py:111-182``: per-label 2x2 confusion matrices ``cm [L, 2, 2]`` (``[l, target, prediction]``) and the
    scores / targets of every used row for the precision-recall curves."""

    def __init__(self, num_labels: int, threshold_detect: float = 0.5) -> None:
        super().__init__()
        self.num_labels, self.threshold_detect = num_labels, threshold_detect
        self.preds: list = []                                                        # metric.py:124-125 (lists of [n, L] tensors)
        self.target: list = []
        self._pending: list = []       # engine-form updates: (scores, targets, used-row mask), compacted by ``compute``
        self.register_buffer("cm", torch.zeros(num_labels, 2, 2, dtype=torch.long), persistent=False)   # metric.py:126-130

    def update(self, logits: torch.Tensor, targets: torch.Tensor, *, missing_val=None) -> None:
        """``metric.py:132-160``: one launch adds the used rows to ``cm``; their ``torch.sigmoid(logits)`` (fp32) and int64 targets
        are appended on the device.  ``missing_val`` given (engine form): rows holding it are skipped (``base.py:120-123``) -- in the
        kernel for ``cm``, and for the lists by a row mask that ``compute`` applies, so that no update reads a count back."""
        if logits.dtype != torch.float32 or logits.dim() != 2 or logits.shape[1] != self.num_labels or logits.shape != targets.shape:
            raise ValueError(f"MultiLabelMetric.update: fp32 logits and targets [N, {self.num_labels}] expected")
        if self.cm.device != logits.device:
            self.cm = self.cm.to(logits.device)
        logits, tgt = logits.contiguous(), targets.to(torch.float32).contiguous()
        hip.confusion_bce(logits, tgt, float("nan") if missing_val is None else missing_val, self.threshold_detect, self.cm,
                          logits.shape[0], self.num_labels)
        scores = torch.sigmoid(logits)                                                # metric.py:134
        if missing_val is None:
            self.preds.append(scores)                                                 # metric.py:151-152
            self.target.append(tgt.long())
        else:
            self._pending.append((scores, tgt.long(), (tgt != missing_val).all(dim=1)))

    def _compact(self) -> None:
        for scores, tgt, used in self._pending:
            self.preds.append(scores[used])
            self.target.append(tgt[used])
        self._pending = []

    def compute(self) -> dict:
        """``metric.py:162-182``, fp64."""
        self._compact()
        cm = _reduced_cm(self.cm).double()
        dev = cm.device
        empty = torch.zeros(0, self.num_labels, device=dev)
        preds = _gathered_rows(torch.cat([p.to(dev) for p in self.preds]) if self.preds else empty.float())   # dim_zero_cat
        target = _gathered_rows(torch.cat([t.to(dev) for t in self.target]) if self.target else empty.long())
        true_pos, false_pos, false_neg = cm[:, 1, 1], cm[:, 0, 1], cm[:, 1, 0]       # metric.py:164-166
        label_weights = (true_pos + false_neg) / (true_pos + false_neg).sum()        # metric.py:167
        per_label_f1 = (2 * true_pos) / (2 * true_pos + false_pos + false_neg)       # metric.py:169
        per_label_ap = average_precision(preds, target).to(dev)                      # metric.py:170-176
        return {"average_f1": per_label_f1.nanmean(),                                # metric.py:178-181
                "average_ap": per_label_ap.nanmean(),
                "weighted_f1": (per_label_f1 * label_weights).nansum(),
                "weighted_ap": (per_label_ap * label_weights).nansum()}

    def reset(self) -> None:
        self.cm.zero_()
        self.preds, self.target, self._pending = [], [], []
