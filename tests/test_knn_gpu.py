"""The nearest-neighbour kernels on the GPU (csrc/knn.hip): ``mh_knn_topk`` bit for bit against ``hip.knn_reference`` on exact
(integer) operands, independent of splits, chunks and row position, and within the derived bounds of tests/knn_cases.py on real
operands; ``mh_knn_vote`` and ``mh_l2_normalize`` against fp64 under their bounds; ``SupervisedEngine.encode``,
``SSLModule.encode_step`` and a k-NN evaluation end to end.

Every kernel call goes through the guarded callers below: operands in the middle of poisoned allocations (tests/guards.py), NaN
pad columns behind every operand row, outputs misaligned by 4 bytes where the contract allows; every size and index passed is in
range.  The observed share of each bound is printed before it is asserted."""

from types import SimpleNamespace

import numpy as np
import pytest
import torch

import maestro_amd.conf as conf
from maestro_amd import hip
from tests import knn_cases as kc
from tests.guards import GuardSet, bits_equal
from tests.numerics import gemm_operands

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


# ----------------------------------------------------------------------------------- guarded callers: guard bands (tests/guards.py)
def topk_call(q, bank, k, index_base=0, init=None, splits=None, pad=8):
    """``hip.knn_topk`` on guarded operands (``pad`` NaN columns behind every row; sims / idx dense at a 4-byte aligned base).
    ``init``: CPU ``(sims, idx)`` of earlier chunks (accumulate).  Returns CPU numpy ``(sims, idx)``."""
    gs = GuardSet(DEV)
    E = q.shape[1]  # noqa: N806
    qd = gs.inp(q, ld=E + pad, name="q")
    bd = gs.inp(bank, ld=E + pad, name="bank") if bank.shape[0] else torch.zeros(0, E, dtype=torch.bfloat16, device=DEV)
    sims = gs.out((q.shape[0], k), align=4, name="sims")
    idx = gs.out((q.shape[0], k), dtype=torch.int32, align=4, name="idx")
    if init is not None:
        sims.copy_(torch.as_tensor(init[0]))
        idx.copy_(torch.as_tensor(init[1]))
    gs.arm()
    hip.knn_topk(qd, bd, k, sims=sims, idx=idx, index_base=index_base, accumulate=init is not None, splits=splits)
    gs.check()
    return sims.cpu().numpy(), idx.cpu().numpy()


def vote_call(sims, idx, labels, C, T, k_eval=None, missing_val=-1, outputs=("scores", "cls"), pad=3):  # noqa: N803
    gs = GuardSet(DEV)
    Nq = sims.shape[0]  # noqa: N806
    s = gs.inp(torch.as_tensor(sims), align=4, name="sims")
    i = gs.inp(torch.as_tensor(idx), align=4, name="idx")
    lab = gs.inp(torch.as_tensor(labels), align=4, name="labels")
    scores = gs.out((Nq, C), ld=C + pad, align=4, name="scores") if "scores" in outputs else None
    cls = gs.out((Nq,), dtype=torch.int32, align=4, name="cls") if "cls" in outputs else None
    gs.arm()
    hip.knn_vote(s, i, lab, C, T=T, k_eval=k_eval, missing_val=missing_val, scores=scores, cls=cls, want_scores=scores is not None,
                 want_cls=cls is not None)
    gs.check()
    return (None if scores is None else scores.cpu().numpy()), (None if cls is None else cls.cpu().numpy())


def norm_call(x, eps=1e-12, in_place=False, outputs=("y", "y16"), pad=5):
    gs = GuardSet(DEV)
    rows, E = x.shape  # noqa: N806
    if in_place:
        xd = y = gs.out((rows, E), ld=E + pad, align=4, name="x=y")
        xd.copy_(x)
    else:
        xd = gs.inp(x, ld=E + pad, align=4, name="x")
        y = gs.out((rows, E), ld=E + 2 * pad, align=4, name="y") if "y" in outputs else None
    y16 = gs.out((rows, E), dtype=torch.bfloat16, ld=E + pad, align=2, name="y16") if "y16" in outputs else None
    gs.arm()
    hip.l2_normalize(xd, y=y, y16=y16, eps=eps)
    gs.check()
    return (None if y is None else y.cpu().numpy()), (None if y16 is None else y16.cpu().view(torch.int16).numpy().view(np.uint16))


# ----------------------------------------------------------------------------------------------------- exact
BIG_NB = 805          # 7 bank tiles of 128 rows, the last one partial: the split rule cuts it 3 ways


@pytest.mark.parametrize("E", [32, 192, 1024])
@pytest.mark.parametrize("k", [1, 5, 32, 128])
def test_topk_exact_over_query_and_bank_sizes(E, k):  # noqa: N803
    """Integer operands: bit for bit against the reference for Nq in {1, 17, 65} x Nb in {1, k - 1, 127, 805}."""
    for Nq in (1, 17, 65):  # noqa: N806
        for Nb in sorted({1, max(1, k - 1), 127, BIG_NB}):  # noqa: N806
            q, bank = kc.int_operands(Nq, Nb, E, seed=Nq + Nb + E + k)
            got = topk_call(q, bank, k, index_base=11)
            assert kc.lists_equal(got, hip.knn_reference(q, bank, k, index_base=11)), (Nq, Nb)
            if Nb < k:
                assert (got[1][:, Nb:] == -1).all() and np.isneginf(got[0][:, Nb:]).all()
    assert hip.knn_splits(65, BIG_NB, E, k) >= 3


@pytest.mark.parametrize("order", ["ascending", "descending", "equal"])
@pytest.mark.parametrize("k", [5, 128])
def test_topk_exact_on_sorted_and_equal_banks(order, k):
    q, bank = kc.int_operands(17, BIG_NB, 192, seed=7 + k, order=order)
    got = topk_call(q, bank, k)
    want = hip.knn_reference(q, bank, k)
    assert kc.lists_equal(got, want)
    if order == "equal":
        assert got[1].tolist() == [list(range(k))] * 17
    for form in kc.TOPK_WRONG[:1] if order == "equal" else kc.TOPK_WRONG:           # the wrong forms the host file names
        assert not kc.lists_equal(got, kc.wrong_topk(form, q, bank, k)), form


def test_topk_on_the_hand_made_tie_case():
    q, bank, k, want_s, want_i = kc.tie_case()
    assert kc.lists_equal(topk_call(q, bank, k), (want_s, want_i))
    assert kc.lists_equal(topk_call(q, bank[:2], k, index_base=7), hip.knn_reference(q, bank[:2], k, index_base=7))


# ----------------------------------------------------------------------------------------------------- independence
@pytest.mark.parametrize("k", [5, 128])
def test_topk_is_independent_of_splits_chunks_and_row_position(k):
    Nq, E = 65, 192  # noqa: N806
    q, bank = kc.int_operands(Nq, BIG_NB, E, seed=21 + k)
    want = hip.knn_reference(q, bank, k, index_base=3)
    for splits in (1, 2, 7, None, 9):                        # None: the rule's own value; 9: more splits than bank tiles
        assert kc.lists_equal(topk_call(q, bank, k, index_base=3, splits=splits), want), splits
    init = None
    for lo, hi in ((0, 37), (37, 600), (600, BIG_NB)):       # three uneven chunks, ascending index_base
        init = topk_call(q, bank[lo:hi], k, index_base=3 + lo, init=init)
    assert kc.lists_equal(init, want)
    assert kc.lists_equal(topk_call(q, bank[:0], k, index_base=3 + BIG_NB, init=init), want)         # an empty last chunk
    perm = torch.randperm(Nq, generator=torch.Generator().manual_seed(5))
    got = topk_call(q[perm], bank, k, index_base=3)
    assert kc.lists_equal(got, (want[0][perm.numpy()], want[1][perm.numpy()]))


def test_topk_real_operands_agree_bit_for_bit_across_splits_chunks_and_positions():
    """The similarity of a pair is one fp32 sum whatever tile, split, chunk or query row it falls in."""
    a, b = gemm_operands("randn", 65, BIG_NB, 192, seed=4)
    q, bank = a.to(torch.bfloat16), b.t().contiguous().to(torch.bfloat16)
    base = topk_call(q, bank, 20, splits=1)
    for splits in (2, 7, None):
        assert kc.lists_equal(topk_call(q, bank, 20, splits=splits), base), splits
    init = None
    for lo, hi in ((0, 130), (130, 131), (131, BIG_NB)):
        init = topk_call(q, bank[lo:hi], 20, index_base=lo, init=init)
    assert kc.lists_equal(init, base)
    perm = torch.randperm(65, generator=torch.Generator().manual_seed(6))
    assert kc.lists_equal(topk_call(q[perm], bank, 20), (base[0][perm.numpy()], base[1][perm.numpy()]))


# ----------------------------------------------------------------------------------------------------- bounded
@pytest.mark.parametrize("dist", ["randn", "lognormal", "cancel"])
def test_topk_within_the_similarity_bound(dist):
    E, k = 192, 20  # noqa: N806
    a, b = gemm_operands(dist, 65, BIG_NB, E, seed=9)
    q, bank = a.to(torch.bfloat16), b.t().contiguous().to(torch.bfloat16)
    s64, absprod = kc.sim_ref64(q, bank)
    sims, idx = topk_call(q, bank, k, index_base=100)
    worst = kc.check_bounded_topk(sims, idx, s64, kc.sim_bound(absprod, E), index_base=100)
    print(f"{dist}: worst |sim - sim64| / bound = {worst:.4f}")


# ----------------------------------------------------------------------------------------------------- vote
def test_vote_counts_exactly_on_equal_similarities():
    idx = np.array([[0, 1, 2, 3, 4, 5], [5, 4, -1, -1, -1, -1], [6, 7, 6, 7, 6, 7], [9, 2, 0, 2, 3, 1], [-1] * 6], dtype=np.int32)
    sims = np.zeros(idx.shape, dtype=np.float32)
    sims[1, 2:], sims[4] = -np.inf, -np.inf
    labels = np.array([2, 2, 1, 1, 0, 3, -1, 9], dtype=np.int32)
    for k_eval in (None, 2, 1):
        want_s, want_c = hip.knn_vote_reference(sims, idx, labels, 4, T=0.07, k_eval=k_eval)
        scores, cls = vote_call(sims, idx, labels, 4, 0.07, k_eval=k_eval)
        assert np.array_equal(scores, want_s) and np.array_equal(cls, want_c), k_eval
    assert cls.tolist() == [2, 3, -1, -1, -1] and scores[0].tolist() == [0, 0, 1, 0]      # k_eval = 1
    scores, cls = vote_call(sims, idx, labels, 4, 0.07)
    assert cls.tolist() == [1, 0, -1, 1, -1]                                                # lowest class on ties; -1: no voter
    assert np.array_equal(vote_call(sims, idx, labels, 4, 0.07, outputs=("cls",))[1], cls)
    assert np.array_equal(vote_call(sims, idx, labels, 4, 0.07, outputs=("scores",))[0], scores)
    for form in ("k_not_k_eval", "missing_counted"):
        assert not np.array_equal(kc.wrong_vote(form, sims, idx, labels, 4, 0.07, 2), vote_call(sims, idx, labels, 4, 0.07, k_eval=2)[0])


@pytest.mark.parametrize("T", [0.07, 0.01])
@pytest.mark.parametrize("Nq,k,k_eval,C", [(24, 12, 8, 7), (5, 128, 128, 1024), (130, 20, 20, 2), (3, 1, 1, 65)])
def test_vote_within_its_bound_and_cls_is_the_argmax_of_the_scores(T, Nq, k, k_eval, C):  # noqa: N803
    sims, idx, labels = kc.vote_case(Nq, k, C, 40, seed=5 + Nq)
    s64, bound = kc.vote_bound(sims, idx, labels, C, T, k_eval)
    scores, cls = vote_call(sims, idx, labels, C, T, k_eval=k_eval)
    err = np.abs(scores.astype(np.float64) - s64)
    print(f"T={T} Nq={Nq} k={k} C={C}: worst |score - score64| / bound = {float((err / np.maximum(bound, 1e-300)).max()):.4f}")
    assert np.isfinite(scores).all() and (err <= bound).all()
    voted = hip.knn_vote_reference(sims, idx, labels, C, T, k_eval)[1] >= 0
    assert np.array_equal(cls, kc.argmax_rule(scores, voted))           # of the scores just written, no exclusions
    if T == 0.01 and Nq == 24:                                          # the wrong forms of the host file, on the kernel's output
        for form in kc.VOTE_WRONG:
            with np.errstate(invalid="ignore"):
                bad = np.abs(kc.wrong_vote(form, sims, idx, labels, C, T, k_eval).astype(np.float64) - s64)
            assert not (bad <= bound).all(), form


def test_vote_does_not_overflow_for_any_scale_of_the_features():
    sims, idx, labels = kc.vote_case(9, 10, 5, 40, seed=2, scale=3.0e4)         # un-normalised features: sim / T ~ 3e6
    scores, cls = vote_call(sims, idx, labels, 5, 0.01)
    s64, bound = kc.vote_bound(sims, idx, labels, 5, 0.01, 10)
    assert np.isfinite(scores).all() and (np.abs(scores - s64) <= bound).all()


# ----------------------------------------------------------------------------------------------------- normalise
@pytest.mark.parametrize("E", [32, 192, 1024, 7])
def test_normalise_within_its_bound_and_the_bf16_copy_is_its_rne(E):  # noqa: N803
    x = kc.norm_inputs(E, seed=E)
    y64 = kc.norm_ref64(x.numpy())
    y, y16 = norm_call(x)
    err = np.abs(y.astype(np.float64) - y64)
    print(f"E={E}: worst |y - y64| / bound = {float((err / kc.norm_bound(y64, E)).max()):.4f}")
    assert (err <= kc.norm_bound(y64, E)).all()
    assert (y[3] == 0).all() and np.array_equal(y[4], (x[4] / np.float32(1e-12)).numpy())        # a zero row; a row below eps
    assert np.array_equal(y16, kc.bf16_rne(y))
    nrm = np.sqrt((y.astype(np.float64) ** 2).sum(axis=1))
    assert (np.abs(nrm[[0, 1, 2, 5, 6, 7, 8]] - 1) <= (E / 2 + 3) * kc.U * 2).all()
    yi, yi16 = norm_call(x, in_place=True)                                                        # y == x
    assert np.array_equal(yi.view(np.int32), y.view(np.int32)) and np.array_equal(yi16, y16)
    assert np.array_equal(norm_call(x, outputs=("y16",))[1], y16)
    assert np.array_equal(norm_call(x, outputs=("y",))[0].view(np.int32), y.view(np.int32))
    y0, _ = norm_call(x, eps=0.0)                                                                 # eps = 0: the zero row stays zero
    assert (y0[3] == 0).all() and np.isfinite(y0).all()
    assert not (np.abs(kc.norm_ref64(x.numpy(), eps_rule=False) - y.astype(np.float64)) <= kc.norm_bound(y64, E)).all()


# ----------------------------------------------------------------------------------------------------- engine
def _model(targets=("cosia",), seed=3):
    from maestro_amd.ssl import mae as pmae
    from oracle.gen_golden import build_datasets, make_batch, sup_case_table
    case = dict(sup_case_table()["sup_flair_seg"])
    case["ds_kwargs"] = dict(case["ds_kwargs"], filter_targets=list(targets))
    ds = build_datasets(case, conf)
    torch.manual_seed(seed)
    model = pmae.mae_tiny(datasets=ds, mask=conf.MaskConfig(), interpolate="nearest", fusion_mode="group", inter_depth=1, model="mae",
                          num_levels=1, type_head="attentive", fac_abs_enc=1.0, fac_date_enc=1.0, depth=2)
    batch = {k: v.to(DEV) for k, v in make_batch(ds.dataset, 2, 1).items()}
    return ds, model, batch


def _clone(f):
    torch.cuda.synchronize()
    return f.f32.clone(), f.bf16.clone()


def test_encode_equals_the_means_of_the_engines_own_tokens():
    ds, model, batch = _model()
    eng = model.sup_engine(2, DEV, "probe")
    B, E, JL = 2, eng.E, eng.JL  # noqa: N806
    flat, grad, loss = eng.store.flat.clone(), eng.store.grad.clone(), eng.loss_acc.clone()
    raw = _clone(eng.encode(batch, "sample", normalize=False))
    xenc = eng.xenc.double().cpu().numpy()
    want = xenc.mean(axis=1)
    bound = (JL + 2) * kc.U * np.abs(xenc).sum(axis=1) / JL + 2.0 ** -149          # JL - 1 additions, fl(1 / JL) and one product, any order
    err = np.abs(raw[0].double().cpu().numpy() - want)
    print(f"sample mean: worst err / bound = {float((err / bound).max()):.4f}")
    assert raw[0].shape == (B, E) and raw[1].dtype == torch.bfloat16 and (err <= bound).all()
    assert bits_equal(raw[1], raw[0].to(torch.bfloat16))
    # grid: mean_reduce_fwd of the resized tokens (this model has a segment target: the engine's own reference-grid buffer)
    grid = _clone(eng.encode(batch, "grid", normalize=False))
    r = eng.ref
    want_g = torch.empty(B, r["Lr"], E, device=DEV)
    hip.mean_reduce_fwd(r["x"], want_g, B, r["TD"], r["Lr"], E)
    assert grid[0].shape == (B, r["Lr"], E) and bits_equal(grid[0], want_g) and bits_equal(grid[1], want_g.to(torch.bfloat16))
    # normalised rows: unit norm, the normalisation of the raw means, bf16 = RNE; two calls (eager, then captured) give the same bits
    for level, base in (("sample", raw), ("grid", grid)):
        one = _clone(eng.encode(batch, level))
        rows = base[0].reshape(-1, E).cpu().numpy()
        y64 = kc.norm_ref64(rows)
        assert (np.abs(one[0].reshape(-1, E).double().cpu().numpy() - y64) <= kc.norm_bound(y64, E)).all()
        nrm = one[0].double().norm(dim=-1)
        assert float((nrm - 1).abs().max()) <= (E / 2 + 3) * kc.U * 2
        assert bits_equal(one[1], one[0].to(torch.bfloat16))
        for _ in range(3):
            again = _clone(eng.encode(batch, level))
            assert bits_equal(again[0], one[0]) and bits_equal(again[1], one[1])
    assert bits_equal(eng.store.flat, flat) and bits_equal(eng.store.grad, grad) and bits_equal(eng.loss_acc, loss)
    with pytest.raises(ValueError, match="level"):
        eng.encode(batch, "token")
    with pytest.raises(RuntimeError, match="forward"):           # the saved activations are not a forward's any more
        eng.backward()


def test_encode_phase_matches_probe_phase_and_refuses_the_head_paths():
    ds, model, batch = _model()
    probe = model.sup_engine(2, DEV, "probe")
    want = {level: _clone(probe.encode(batch, level)) for level in ("sample", "grid")}
    enc = model.sup_engine(2, DEV, "encode")                      # re-homes the same weights
    assert enc is model.sup_engine(2, DEV, "encode") and enc.phase == "encode" and enc.hb == {} and enc.ref is None
    for level in ("sample", "grid"):
        got = _clone(enc.encode(batch, level))
        assert bits_equal(got[0], want[level][0]) and bits_equal(got[1], want[level][1]), level
    for call in (lambda: enc.forward(batch), enc.backward, lambda: enc.predict(batch), lambda: enc.predict_scene(batch)):
        with pytest.raises(ValueError, match="encode"):
            call()


def test_encode_phase_builds_with_no_target_selected():
    from maestro_amd.engine_sup import SupervisedEngine
    ds, model, batch = _model(targets=())
    assert not len(model.heads)
    with pytest.raises(ValueError, match="no target"):           # the existing phases keep their refusal
        SupervisedEngine(model, 2, DEV, phase="probe")
    eng = model.sup_engine(2, DEV, "encode")
    f = _clone(eng.encode(batch, "sample"))
    g = _clone(eng.encode(batch, "grid"))
    G = model.out_grid_size[ds.dataset.ref_input]  # noqa: N806
    assert f[0].shape == (2, eng.E) and g[0].shape == (2, G * G, eng.E) and eng.ref is None
    assert bool(torch.isfinite(f[0]).all()) and bool(torch.isfinite(g[0]).all())
    assert float((g[0].double().norm(dim=-1) - 1).abs().max()) < 1e-4


def test_encode_step_in_finetune_uses_the_ema_weights():
    from maestro_amd.train.model import SSLModule
    from oracle.gen_golden import build_datasets, make_batch
    from tests.test_oracle_sup import CASES
    ds = build_datasets(CASES["sup_treesat_mlc"], conf)
    batch = {k: v.to(DEV) for k, v in make_batch(ds.dataset, 4, 1).items()}
    torch.manual_seed(3)
    module = SSLModule(datasets=ds, mask=conf.MaskConfig(), interpolate="nearest", fusion_mode="group", inter_depth=1,
                       model="mae", model_size="tiny", type_head="attentive", use_ema=True)
    module.trainer = SimpleNamespace(ssl_phase="finetune", max_epochs=10)
    base = _clone(module.encode_step(batch, 0))              # EMA == model right after construction
    eng = module.model._sup_engine
    before = eng.store.flat.clone()
    with torch.no_grad():                                    # perturb the live model: the features must not move
        for p in module.model.parameters():
            p.mul_(0.5)
    live = eng.store.flat.clone()
    assert not bits_equal(live, before)
    same = _clone(module.encode_step(batch, 0))
    assert bits_equal(same[0], base[0]) and bits_equal(same[1], base[1])
    assert bits_equal(eng.store.flat, live), "the live weights must be back after the EMA encoding"
    with torch.no_grad():                                    # perturb the EMA copy: the features move
        for p in module.ema_model.parameters():
            p.mul_(0.5)
    assert not bits_equal(_clone(module.encode_step(batch, 0))[0], base[0])
    module.trainer = SimpleNamespace(ssl_phase="pretrain")   # valid in the pretrain phase, on an encoders-only engine
    f = module.encode_step(batch, 0)
    assert module.model._sup_engine.phase == "encode" and f.f32.shape == (4, module.model.embed_dim)


# ----------------------------------------------------------------------------------------------------- end to end
def test_knn_evaluation_end_to_end():
    from maestro_amd.train.knn import FeatureBank, KNNClassifier
    from maestro_amd.train.metric import MonoLabelMetric
    from oracle.gen_golden import make_batch
    ds, model, _ = _model(targets=())
    eng = model.sup_engine(2, DEV, "encode")
    C, n_batches = 3, 4  # noqa: N806
    bank = FeatureBank(2 * n_batches, eng.E, DEV)
    rng = np.random.default_rng(8)
    for i in range(n_batches):
        batch = {k: v.to(DEV) for k, v in make_batch(ds.dataset, 2, 10 + i).items()}
        labels = torch.as_tensor(rng.integers(-1, C, size=2), device=DEV)                        # -1: missing
        bank.add(eng.encode(batch).bf16, labels)
    assert bank.rows == 8
    with pytest.raises(ValueError, match="overflow"):
        bank.add(eng.encode(batch).bf16, labels)
    queries = torch.cat([eng.encode({k: v.to(DEV) for k, v in make_batch(ds.dataset, 2, 30 + i).items()}).bf16.clone() for i in range(3)])
    targets = torch.as_tensor(rng.integers(-1, C, size=6), device=DEV)
    knn = KNNClassifier(bank, C, k=5, T=0.07)
    sims, idx = knn.topk(queries)
    s64q, absprod = kc.sim_ref64(queries, bank.features)
    kc.check_bounded_topk(sims.cpu().numpy(), idx.cpu().numpy(), s64q, kc.sim_bound(absprod, eng.E))
    chunked = KNNClassifier(bank, C, k=5, T=0.07, chunk_rows=3).topk(queries)
    assert bits_equal(chunked[0], sims) and bits_equal(chunked[1], idx)
    scores, cls = knn.scores(queries)
    want_s, want_c = hip.knn_vote_reference(sims.cpu().numpy(), idx.cpu().numpy(), bank.label_column().cpu().numpy(), C, T=0.07)
    s64, bound = kc.vote_bound(sims.cpu().numpy(), idx.cpu().numpy(), bank.label_column().cpu().numpy(), C, 0.07, 5)
    assert (np.abs(scores.cpu().numpy() - s64) <= bound).all() and (np.abs(want_s - s64) <= bound).all()
    voted = want_c >= 0
    assert np.array_equal(cls.cpu().numpy(), kc.argmax_rule(scores.cpu().numpy(), voted))
    metric, ref_metric = MonoLabelMetric("classif", C), MonoLabelMetric("classif", C)
    knn.update_metric(metric, queries, targets)
    onehot = torch.zeros(6, C, device=DEV)                      # the metric on the predicted classes themselves
    onehot[torch.arange(6), torch.as_tensor(kc.argmax_rule(scores.cpu().numpy(), np.ones(6, bool)), device=DEV).long()] = 1
    ref_metric.update(onehot, targets, missing_val=-1)
    assert torch.equal(metric.cm, ref_metric.cm) and int(metric.cm.sum()) == int((targets >= 0).sum())
