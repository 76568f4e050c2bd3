"""Label-cheap evaluation of an encoder: a device-resident bank of labelled features and the weighted k-nearest-neighbour
classifier over it (the DINO protocol: cosine similarity of L2-normalised features, ``k`` neighbours, votes weighted by
``exp(sim / T)``).  The reference has no such path; include/maestro_hip.h states what the three kernels compute, ``hip.knn_reference``
and ``hip.knn_vote_reference`` restate it in numpy.

    engine = model.sup_engine(B, device, "encode")
    bank = FeatureBank(n_train, model.embed_dim, device)
    for batch in train_batches:
        bank.add(engine.encode(batch).bf16, batch["label"])
    knn = KNNClassifier(bank, num_classes, k=20, T=0.07)
    for batch in val_batches:
        knn.update_metric(metric, engine.encode(batch).bf16, batch["label"])

Out of scope: merging the lists of several ranks (each rank scores against its own bank), dihedral views of features,
multilabel votes.  No CPU fallback.
"""

from __future__ import annotations

import torch

from maestro_amd import hip


class FeatureBank:
    """``capacity`` preallocated bf16 feature rows ``[capacity, E]`` with ``n_label_cols`` int32 label columns; ``add`` appends on the
    device and never reads anything back (the fill count lives on the host: the shapes of the added tensors give it)."""

    def __init__(self, capacity: int, E: int, device, n_label_cols: int = 1) -> None:  # noqa: N803
        if isinstance(capacity, bool) or not isinstance(capacity, int) or capacity < 1:
            raise ValueError(f"FeatureBank: capacity={capacity!r} (a positive int)")
        if not isinstance(E, int) or E < 32 or E > 1024 or E % 32:
            raise ValueError(f"FeatureBank: E={E!r} (a multiple of 32 in 32 ... 1024: the operand width of mh_knn_topk)")
        if not isinstance(n_label_cols, int) or n_label_cols < 1:
            raise ValueError(f"FeatureBank: n_label_cols={n_label_cols!r} (a positive int)")
        self.capacity, self.E, self.n_label_cols, self.rows = capacity, E, n_label_cols, 0
        self.device = torch.device(device)
        self.features = torch.zeros(capacity, E, dtype=torch.bfloat16, device=self.device)
        self.labels = torch.full((n_label_cols, capacity), -1, dtype=torch.int32, device=self.device)     # column-major: one row per label column

    def add(self, features_bf16: torch.Tensor, labels: torch.Tensor) -> None:
        """Append ``features_bf16`` ``[..., E]`` (bf16, e.g. ``Features.bf16`` of ``encode``) and one label per feature row:
        ``labels`` with as many entries as rows (``n_label_cols == 1``) or ``[rows, n_label_cols]``; any integer dtype."""
        if not isinstance(features_bf16, torch.Tensor) or features_bf16.dtype != torch.bfloat16 or features_bf16.shape[-1] != self.E:
            raise ValueError(f"FeatureBank.add: features must be a bfloat16 tensor [..., {self.E}]")
        n = features_bf16.numel() // self.E
        if not isinstance(labels, torch.Tensor) or labels.dtype.is_floating_point or labels.numel() != n * self.n_label_cols:
            raise ValueError(f"FeatureBank.add: labels must be an integer tensor of {n} x {self.n_label_cols} entries")
        if self.rows + n > self.capacity:
            raise ValueError(f"FeatureBank.add: {n} rows onto {self.rows} overflow the capacity of {self.capacity}")
        if features_bf16.device != self.features.device or labels.device != self.features.device:
            raise ValueError(f"FeatureBank.add: features and labels must be on {self.features.device}")
        self.features[self.rows: self.rows + n].copy_(features_bf16.reshape(n, self.E))
        self.labels[:, self.rows: self.rows + n].copy_(labels.reshape(n, self.n_label_cols).t())
        self.rows += n

    def label_column(self, col: int = 0) -> torch.Tensor:
        """The labels of the filled rows in column ``col``: a contiguous int32 view ``[rows]``."""
        return self.labels[col, : self.rows]

    def reset(self) -> None:
        self.rows = 0


def check_knn_args(num_classes, k, T, chunk_rows) -> None:  # noqa: N803
    """The argument checks of ``KNNClassifier`` (no GPU needed)."""
    if isinstance(num_classes, bool) or not isinstance(num_classes, int) or not 2 <= num_classes <= 1024:
        raise ValueError(f"KNNClassifier: num_classes={num_classes!r} (2 ... 1024)")
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= hip.KNN_MAX_K:
        raise ValueError(f"KNNClassifier: k={k!r} (1 ... {hip.KNN_MAX_K})")
    if isinstance(T, bool) or not isinstance(T, (int, float)) or not T > 0:
        raise ValueError(f"KNNClassifier: T={T!r} (a positive temperature)")
    if chunk_rows is not None and (isinstance(chunk_rows, bool) or not isinstance(chunk_rows, int) or chunk_rows < 1):
        raise ValueError(f"KNNClassifier: chunk_rows={chunk_rows!r} (None or a positive int)")


class KNNClassifier:
    """Weighted k-NN over a ``FeatureBank``.  ``k`` neighbours are kept per query; ``scores(k_eval=...)`` votes with the first
    ``k_eval`` of them, so one top-k pass serves several ``k``.  ``chunk_rows``: stream the bank through ``mh_knn_topk`` in chunks
    of that many rows (``accumulate``); the result has the bits of one call."""

    def __init__(self, bank: FeatureBank, num_classes: int, k: int = 20, T: float = 0.07, missing_val: int = -1,  # noqa: N803
                 chunk_rows: int | None = None, label_col: int = 0) -> None:
        if not isinstance(bank, FeatureBank):
            raise ValueError("KNNClassifier: bank must be a FeatureBank")
        check_knn_args(num_classes, k, T, chunk_rows)
        if not 0 <= label_col < bank.n_label_cols:
            raise ValueError(f"KNNClassifier: label_col={label_col!r} outside the bank's {bank.n_label_cols} label columns")
        self.bank, self.num_classes, self.k, self.T, self.missing_val = bank, num_classes, k, float(T), int(missing_val)
        self.chunk_rows, self.label_col = chunk_rows, label_col

    def _queries(self, queries_bf16: torch.Tensor) -> torch.Tensor:
        if not isinstance(queries_bf16, torch.Tensor) or queries_bf16.dtype != torch.bfloat16 or queries_bf16.shape[-1] != self.bank.E:
            raise ValueError(f"KNNClassifier: queries must be a bfloat16 tensor [..., {self.bank.E}]")
        if self.bank.rows < 1:
            raise ValueError("KNNClassifier: the bank is empty")
        return queries_bf16.reshape(-1, self.bank.E)

    def topk(self, queries_bf16: torch.Tensor):
        """``(sims f32 [Nq, k], idx i32 [Nq, k])``: the ``k`` nearest filled bank rows of every query row, sorted."""
        q = self._queries(queries_bf16)
        feats, rows = self.bank.features, self.bank.rows
        if self.chunk_rows is None or self.chunk_rows >= rows:
            return hip.knn_topk(q, feats[:rows], self.k)
        sims = idx = None
        for lo in range(0, rows, self.chunk_rows):
            hi = min(rows, lo + self.chunk_rows)
            sims, idx = hip.knn_topk(q, feats[lo:hi], self.k, sims=sims, idx=idx, index_base=lo, accumulate=lo > 0)
        return sims, idx

    def scores(self, queries_bf16: torch.Tensor, k_eval: int | None = None):
        """``(scores f32 [Nq, num_classes], cls i32 [Nq])`` of the weighted vote over the first ``k_eval`` neighbours."""
        sims, idx = self.topk(queries_bf16)
        return hip.knn_vote(sims, idx, self.bank.label_column(self.label_col), self.num_classes, T=self.T, k_eval=k_eval,
                            missing_val=self.missing_val)

    def update_metric(self, metric, queries_bf16: torch.Tensor, targets: torch.Tensor, k_eval: int | None = None) -> None:
        """Feed a ``MonoLabelMetric`` with the vote's scores as logits: its own arg-max (the lowest class among equal maxima) is
        the vote's, so OA / F1 / IoU of the k-NN evaluation come from the device confusion matrix.  ``targets``: one integer per
        query row; entries equal to ``missing_val`` are not counted."""
        scores, _ = self.scores(queries_bf16, k_eval)
        if targets.numel() != scores.shape[0]:
            raise ValueError(f"KNNClassifier.update_metric: {targets.numel()} targets for {scores.shape[0]} queries")
        metric.update(scores, targets.reshape(-1), missing_val=self.missing_val)
