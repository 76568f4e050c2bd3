"""Nearest neighbours without a GPU: their entry points of include/maestro_hip.h (declared, exported, bound, bad arguments refused
before any launch), the split rule, ``hip.knn_reference`` / ``hip.knn_vote_reference`` (the statements the kernels are held to in
tests/test_knn_gpu.py) with their own teeth, the derived bounds of tests/knn_cases.py, and the argument checks of ``encode``,
``FeatureBank`` and ``KNNClassifier``."""

import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import maestro_amd.conf as conf
from maestro_amd import hip
from tests import knn_cases as kc
from tests.numerics import gemm_operands

ROOT = Path(__file__).resolve().parents[1]
NAMES = ("mh_knn_splits", "mh_knn_workspace_bytes", "mh_l2_normalize", "mh_knn_topk", "mh_knn_vote")
FAKE = ctypes.c_void_p(0x10000)      # never dereferenced: every call below is rejected before any launch
NULL = ctypes.c_void_p(0)


# ------------------------------------------------------------------------------------------------------------- C ABI
def test_knn_names_are_declared_exported_bound_and_wrapped():
    header = (ROOT / "include" / "maestro_hip.h").read_text()
    declared = set(re.findall(r"\b(mh_[a-z0-9_]+)\s*\(", header))
    assert set(NAMES) <= declared
    assert 'extern "C"' in header and "maestro/layers/head.py:116-130" in header
    lib = hip.lib()
    for name in NAMES:
        assert hasattr(lib, name), f"{name} is declared but not exported"
        assert getattr(lib, name).argtypes is not None and callable(getattr(hip, name[3:]))
    for fn in ("knn_reference", "knn_vote_reference"):
        assert callable(getattr(hip, fn))
    assert hip.KNN_MAX_K == int(re.search(r"#define MH_KNN_MAX_K\s+(\d+)", header).group(1))


def _err():
    return hip.lib().mh_last_error().decode()


def _id(kw):
    return "-".join(f"{k}={'null' if v is NULL else v}" for k, v in kw.items())


def _topk(q=FAKE, ldq=64, bank=FAKE, ldb=64, index_base=0, sims=FAKE, idx=FAKE, accumulate=0, ws=FAKE, ws_bytes=None, splits=2,  # noqa: N803
          Nq=5, Nb=300, E=64, k=4):
    need = max(0, hip.lib().mh_knn_workspace_bytes(Nq, k, max(splits, 1)))
    return hip.lib().mh_knn_topk(q, ldq, bank, ldb, index_base, sims, idx, accumulate, ws, need if ws_bytes is None else need + ws_bytes,
                                 splits, Nq, Nb, E, k, NULL)


def _vote(sims=FAKE, idx=FAKE, labels=FAKE, n_labels=10, missing_val=-1, inv_T=10.0, k=8, k_eval=8, scores=FAKE, lds=4, cls=FAKE,  # noqa: N803
          Nq=3, C=4):
    return hip.lib().mh_knn_vote(sims, idx, labels, n_labels, missing_val, inv_T, k, k_eval, scores, lds, cls, Nq, C, NULL)


def _norm(x=FAKE, ldx=32, eps=1e-12, y=FAKE, ldy=32, y16=FAKE, ldy16=32, rows=3, E=32):  # noqa: N803
    return hip.lib().mh_l2_normalize(x, ldx, eps, y, ldy, y16, ldy16, rows, E, NULL)


@pytest.mark.parametrize("kw", [dict(q=NULL), dict(bank=NULL), dict(sims=NULL), dict(idx=NULL), dict(ws=NULL), dict(k=0),
                                dict(k=hip.KNN_MAX_K + 1), dict(E=48, ldq=48, ldb=48), dict(E=1056, ldq=1056, ldb=1056), dict(Nq=0),
                                dict(Nb=0), dict(ldq=56), dict(ldb=56), dict(splits=0), dict(ws_bytes=-1),
                                dict(index_base=2 ** 31 - 300), dict(index_base=-1), dict(ldq=68), dict(accumulate=2)], ids=_id)
def test_knn_topk_rejects_bad_arguments_before_any_launch(kw):
    assert _topk(**kw) == -1
    assert "mh_knn_topk" in _err()


@pytest.mark.parametrize("kw", [dict(sims=NULL), dict(idx=NULL), dict(labels=NULL), dict(scores=NULL, cls=NULL), dict(C=1, lds=1),
                                dict(C=1025, lds=1025), dict(inv_T=0.0), dict(inv_T=-1.0), dict(inv_T=float("nan")), dict(k_eval=9),
                                dict(k_eval=0), dict(k=0, k_eval=0), dict(k=hip.KNN_MAX_K + 1), dict(lds=3), dict(Nq=0),
                                dict(n_labels=0)], ids=_id)
def test_knn_vote_rejects_bad_arguments_before_any_launch(kw):
    assert _vote(**kw) == -1
    assert "mh_knn_vote" in _err()


@pytest.mark.parametrize("kw", [dict(x=NULL), dict(y=NULL, y16=NULL), dict(eps=-1e-12), dict(rows=0), dict(E=0), dict(ldx=31),
                                dict(ldy=31), dict(ldy16=31)], ids=_id)
def test_l2_normalize_rejects_bad_arguments_before_any_launch(kw):
    assert _norm(**kw) == -1
    assert "mh_l2_normalize" in _err()


def test_splits_rule_is_a_pure_function_within_the_bank_tiles():
    lib = hip.lib()
    for Nq, Nb, E, k in [(1, 1, 32, 1), (32, 131072, 768, 20), (4096, 131072, 768, 20), (3200, 262144, 768, 20), (65, 805, 192, 5),  # noqa: N806
                         (17, 127, 1024, 128), (1, 300, 64, 8)]:
        s = [lib.mh_knn_splits(Nq, Nb, E, k) for _ in range(3)]
        assert s[0] == s[1] == s[2] == hip.knn_splits(Nq, Nb, E, k)
        assert 1 <= s[0] <= -(-Nb // 128)
        assert hip.knn_workspace_bytes(Nq, k, s[0]) == 8 * s[0] * Nq * k           # O(splits Nq k): no [Nq, Nb] buffer
    assert hip.knn_splits(65, 805, 192, 5) >= 3 and hip.knn_splits(32, 131072, 768, 20) > 64
    for bad in [(0, 10, 32, 1), (1, 10, 48, 1), (1, 10, 32, 0), (1, 10, 32, 129), (1, -1, 32, 1)]:
        assert lib.mh_knn_splits(*bad) == 0
    assert lib.mh_knn_workspace_bytes(1, 1, 0) == -1 and lib.mh_knn_workspace_bytes(0, 1, 1) == -1


def test_wrappers_check_their_tensors_and_have_no_cpu_fallback():
    q, bank = torch.zeros(3, 32, dtype=torch.bfloat16), torch.zeros(7, 32, dtype=torch.bfloat16)
    with pytest.raises(hip.HipExtensionError, match="bank"):
        hip.knn_topk(q, bank.float(), 2)
    with pytest.raises(hip.HipExtensionError, match="columns"):
        hip.knn_topk(q, torch.zeros(7, 64, dtype=torch.bfloat16), 2)
    with pytest.raises(hip.HipExtensionError, match="accumulate"):
        hip.knn_topk(q, bank, 2, accumulate=True)
    with pytest.raises(hip.HipExtensionError, match="sims"):
        hip.knn_topk(q, bank, 2, sims=torch.zeros(3, 3), idx=torch.zeros(3, 2, dtype=torch.int32))
    with pytest.raises(hip.HipExtensionError, match="GPU"):          # well-formed CPU tensors: no fallback exists
        hip.knn_topk(q, bank, 2)
    with pytest.raises(hip.HipExtensionError, match="y16"):
        hip.l2_normalize(torch.zeros(3, 32), y16=torch.zeros(3, 32))
    with pytest.raises(hip.HipExtensionError, match="no output"):
        hip.l2_normalize(torch.zeros(3, 32))
    with pytest.raises(hip.HipExtensionError, match="GPU"):
        hip.l2_normalize(torch.zeros(3, 32), y=torch.zeros(3, 32))
    with pytest.raises(hip.HipExtensionError, match="labels"):
        hip.knn_vote(torch.zeros(3, 2), torch.zeros(3, 2, dtype=torch.int32), torch.zeros(5), 4)
    with pytest.raises(hip.HipExtensionError, match="GPU"):
        hip.knn_vote(torch.zeros(3, 2), torch.zeros(3, 2, dtype=torch.int32), torch.zeros(5, dtype=torch.int32), 4)


# ------------------------------------------------------------------------------------------------------------- the references' teeth
def test_knn_reference_equals_torch_topk_on_tie_free_inputs():
    a, b = gemm_operands("randn", 9, 301, 64, seed=1)
    q, bank = a.to(torch.bfloat16), b.t().contiguous().to(torch.bfloat16)
    s64 = q.double() @ bank.double().t()
    want = torch.topk(s64, 7, dim=1)
    assert len(torch.unique(s64)) == s64.numel()
    sims, idx = hip.knn_reference(q, bank, 7, index_base=1000)
    assert np.array_equal(idx, want.indices.numpy() + 1000) and np.array_equal(sims, want.values.float().numpy())
    # raw bf16 bit patterns are taken as well as tensors
    bits = lambda t: t.view(torch.int16).numpy().view(np.uint16)  # noqa: E731
    assert kc.lists_equal(hip.knn_reference(bits(q), bits(bank), 7, index_base=1000), (sims, idx))


def test_knn_reference_on_the_hand_made_tie_case_and_its_wrong_forms():
    q, bank, k, want_s, want_i = kc.tie_case()
    assert kc.lists_equal(hip.knn_reference(q, bank, k), (want_s, want_i))
    for form in kc.TOPK_WRONG:
        assert not kc.lists_equal(kc.wrong_topk(form, q, bank, k), (want_s, want_i)), form
    # fewer candidates than k: (-inf, -1) behind them; a NaN similarity is never selected
    s, i = hip.knn_reference(q, bank[:2], 4, index_base=7)
    assert s.tolist() == [[5.0, 3.0, -np.inf, -np.inf]] and i.tolist() == [[8, 7, -1, -1]]
    s, i = hip.knn_reference(None, None, 2, sims=np.array([[np.nan, 1.0, np.nan]]))
    assert s.tolist() == [[1.0, -np.inf]] and i.tolist() == [[1, -1]]


@pytest.mark.parametrize("order", kc.BANK_ORDERS)
def test_knn_reference_chunked_equals_whole(order):
    q, bank = kc.int_operands(5, 300, 32, seed=3, order=order)
    whole = hip.knn_reference(q, bank, 9)
    init = None
    for lo, hi in ((0, 37), (37, 200), (200, 300)):
        init = hip.knn_reference(q, bank[lo:hi], 9, index_base=lo, init=init)
    assert kc.lists_equal(init, whole) and kc.sorted_under_rule(*whole)
    if order == "equal":
        assert whole[1].tolist() == [list(range(9))] * 5
    # plenty of ties: both wrong forms give other lists (equal rows: the right list IS in bank order, only the tie rule shows)
    for form in kc.TOPK_WRONG[:1] if order == "equal" else kc.TOPK_WRONG:
        assert not kc.lists_equal(kc.wrong_topk(form, q, bank, 9), whole), form


def test_vote_reference_counts_ties_k_eval_and_missing_labels():
    # all-zero similarities: the scores are integer counts
    idx = np.array([[0, 1, 2, 3, 4, 5], [5, 4, -1, -1, -1, -1], [6, 7, 6, 7, 6, 7], [9, 2, 0, 2, 3, 1]], dtype=np.int32)
    sims = np.zeros(idx.shape, dtype=np.float32)
    sims[1, 2:] = -np.inf
    labels = np.array([2, 2, 1, 1, 0, 3, -1, 9], dtype=np.int32)          # 6 missing, 7 outside [0, 4); index 9 past the labels
    scores, cls = hip.knn_vote_reference(sims, idx, labels, 4, T=0.07)
    assert scores.tolist() == [[1, 2, 2, 1], [1, 0, 0, 1], [0, 0, 0, 0], [0, 3, 2, 0]]
    assert cls.tolist() == [1, 0, -1, 1]                                   # lowest class among equal maxima; -1: nobody voted
    scores, cls = hip.knn_vote_reference(sims, idx, labels, 4, T=0.07, k_eval=2)
    assert scores.tolist() == [[0, 0, 2, 0], [1, 0, 0, 1], [0, 0, 0, 0], [0, 1, 0, 0]] and cls.tolist() == [2, 0, -1, 1]
    with pytest.raises(ValueError):
        hip.knn_vote_reference(sims, idx, labels, 4, k_eval=7)


@pytest.mark.parametrize("T", [0.07, 0.01])
def test_vote_bound_accepts_the_fp32_restatement_and_rejects_the_wrong_forms(T):  # noqa: N803
    sims, idx, labels = kc.vote_case(24, 12, 7, 40, seed=5)
    s64, bound = kc.vote_bound(sims, idx, labels, 7, T, 8)
    got, cls = hip.knn_vote_reference(sims, idx, labels, 7, T, 8)
    err = np.abs(got.astype(np.float64) - s64)
    print(f"T={T}: fp32 restatement worst err / bound = {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
    assert (err <= bound).all()
    assert np.array_equal(cls, kc.argmax_rule(got, cls >= 0)) and (cls >= 0).any()
    caught = []
    for form in kc.VOTE_WRONG:
        with np.errstate(invalid="ignore"):
            bad = np.abs(kc.wrong_vote(form, sims, idx, labels, 7, T, 8).astype(np.float64) - s64)
        if not (bad <= bound).all():
            caught.append(form)
    assert caught == list(kc.VOTE_WRONG)              # (the unshifted weight: another scale at T = 0.07, inf at T = 0.01)


def test_similarity_bound_accepts_fp32_and_rejects_a_bf16_rounded_similarity():
    a, b = gemm_operands("offset", 8, 64, 192, seed=2)
    q, bank = a.to(torch.bfloat16), b.t().contiguous().to(torch.bfloat16)
    s64, absprod = kc.sim_ref64(q, bank)
    bound = kc.sim_bound(absprod, 192)
    s32 = (q.float() @ bank.float().t()).numpy().astype(np.float64)
    assert (np.abs(s32 - s64) <= bound).all()
    s16 = torch.from_numpy(s64).to(torch.bfloat16).double().numpy()
    assert not (np.abs(s16 - s64) <= bound).all()


@pytest.mark.parametrize("E", [32, 192, 1024])
def test_normalise_bound_accepts_fp32_and_rejects_a_norm_without_the_eps_rule(E):  # noqa: N803
    x = kc.norm_inputs(E, seed=E).numpy()
    y64 = kc.norm_ref64(x)
    bound = kc.norm_bound(y64, E)
    y32 = kc.norm_f32(x)
    assert (np.abs(y32.astype(np.float64) - y64) <= bound).all()
    assert (y64[3] == 0).all() and np.allclose(y64[4], x[4].astype(np.float64) / 1e-12)
    assert not (np.abs(kc.norm_ref64(x, eps_rule=False) - y64) <= bound).all()          # row 4: unit norm instead of x / eps
    # the bf16 copy: round to nearest even, ties included
    y = np.array([1.0, 1.00390625, 1.01171875, -1.00390625, 0.0], dtype=np.float32)       # 1 + 2^-8 (tie -> even), 1 + 3 * 2^-8
    assert np.array_equal(kc.bf16_rne(y), torch.from_numpy(y).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16))


# ------------------------------------------------------------------------------------------------------------- Python surfaces
def test_encode_argument_checks_and_phase_refusals():
    from maestro_amd.engine_sup import FEATURE_LEVELS, Features, SupervisedEngine, check_encode_args
    assert FEATURE_LEVELS == ("sample", "grid") and Features._fields == ("f32", "bf16")
    for level, normalize in (("token", True), ("sample", 1), (None, True)):
        with pytest.raises(ValueError):
            check_encode_args(level, normalize)
    check_encode_args("grid", False)
    with pytest.raises(ValueError, match="Invalid ssl phase"):
        SupervisedEngine(None, 2, "cpu", phase="pretrain")
    with pytest.raises(hip.HipExtensionError, match="GPU"):               # "encode" is a phase; the device is what is wrong
        SupervisedEngine(None, 2, "cpu", phase="encode")


def test_feature_bank_and_classifier_argument_checks():
    from maestro_amd.train.knn import FeatureBank, KNNClassifier
    bank = FeatureBank(5, 32, "cpu")
    assert bank.rows == 0 and bank.features.shape == (5, 32) and bank.features.dtype == torch.bfloat16 and bank.labels.dtype == torch.int32
    bank.add(torch.ones(3, 32, dtype=torch.bfloat16), torch.tensor([4, 5, 6]))
    assert bank.rows == 3 and bank.label_column().tolist() == [4, 5, 6]
    with pytest.raises(ValueError, match="overflow"):
        bank.add(torch.ones(3, 32, dtype=torch.bfloat16), torch.tensor([1, 2, 3]))
    bank.add(torch.ones(1, 2, 32, dtype=torch.bfloat16), torch.tensor([[7], [8]]))        # [B, cells, E] features
    assert bank.rows == 5 and bank.label_column().tolist() == [4, 5, 6, 7, 8]
    with pytest.raises(ValueError, match="overflow"):
        bank.add(torch.ones(1, 32, dtype=torch.bfloat16), torch.tensor([1]))
    for bad in (dict(features_bf16=torch.ones(1, 32), labels=torch.tensor([1])),
                dict(features_bf16=torch.ones(1, 64, dtype=torch.bfloat16), labels=torch.tensor([1])),
                dict(features_bf16=torch.ones(1, 32, dtype=torch.bfloat16), labels=torch.tensor([1.0])),
                dict(features_bf16=torch.ones(1, 32, dtype=torch.bfloat16), labels=torch.tensor([1, 2]))):
        with pytest.raises(ValueError):
            FeatureBank(5, 32, "cpu").add(**bad)
    for kw in (dict(capacity=0, E=32), dict(capacity=4, E=48), dict(capacity=4, E=2048), dict(capacity=4, E=32, n_label_cols=0)):
        with pytest.raises(ValueError):
            FeatureBank(device="cpu", **kw)
    two = FeatureBank(4, 32, "cpu", n_label_cols=2)
    two.add(torch.ones(2, 32, dtype=torch.bfloat16), torch.tensor([[1, 10], [2, 20]]))
    assert two.label_column(1).tolist() == [10, 20] and two.label_column(1).is_contiguous()
    for kw in (dict(num_classes=1), dict(num_classes=1025), dict(num_classes=4, k=0), dict(num_classes=4, k=hip.KNN_MAX_K + 1),
               dict(num_classes=4, T=0.0), dict(num_classes=4, chunk_rows=0), dict(num_classes=4, label_col=1)):
        with pytest.raises(ValueError):
            KNNClassifier(bank, **kw)
    with pytest.raises(ValueError, match="FeatureBank"):
        KNNClassifier(bank.features, 4)
    knn = KNNClassifier(bank, 4, k=3)
    with pytest.raises(ValueError, match="bfloat16"):
        knn.topk(torch.ones(2, 32))
    with pytest.raises(ValueError, match="empty"):
        KNNClassifier(FeatureBank(5, 32, "cpu"), 4).topk(torch.ones(2, 32, dtype=torch.bfloat16))
    with pytest.raises(hip.HipExtensionError, match="GPU"):                               # well-formed CPU tensors: no fallback
        knn.topk(torch.ones(2, 32, dtype=torch.bfloat16))


def test_module_encode_step_refuses_an_unknown_phase():
    from types import SimpleNamespace

    from maestro_amd.train.model import SSLModule
    ds = conf.DatasetsConfig(name_dataset="s2_naip", s2_naip=conf.S2NAIPConfig(filter_inputs=["spot"]))
    module = SSLModule(datasets=ds, mask=conf.MaskConfig(), interpolate="nearest", fusion_mode="group", inter_depth=1, model="mae",
                       model_size="tiny")
    module.trainer = SimpleNamespace(ssl_phase="distill")
    with pytest.raises(ValueError, match="Invalid ssl phase"):
        module.encode_step({"spot": torch.zeros(1, 1, 3, 256, 256)}, 0)
    module.trainer = SimpleNamespace(ssl_phase="pretrain")                 # the pretrain phase still refuses predict_step
    with pytest.raises(ValueError, match="no heads"):
        module.predict_step({"spot": torch.zeros(1, 1, 3, 256, 256)}, 0)
