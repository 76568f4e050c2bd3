"""Device confusion matrices (include/maestro_hip.h) on the GPU.  The results are integers: every comparison is
``torch.equal`` against torch on the CPU working from the same bits -- gather the logits out of the patch layout,
``argmax(dim=-1)``, ``bincount(t * C + pred)`` over the valid pixels.  No tolerance anywhere."""

import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import maestro_amd.conf as conf
from maestro_amd import hip
from maestro_amd.ssl import mae as pmae
from maestro_amd.train.metric import MonoLabelMetric, MultiLabelMetric
from tests.guards import GuardSet
from tests.test_oracle_sup import build_sup_case

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
INT = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _logits(rows, cols, ld, seed):
    """randn rounded to multiples of 2^-6 (exact ties occur) in [rows, cols] of a [rows, ld] buffer whose pad columns are NaN."""
    g = torch.Generator().manual_seed(seed)
    buf = torch.full((rows, ld), float("nan"))
    buf[:, :cols] = (torch.randn(rows, cols, generator=g) * 64).round() / 64
    return buf


def _raster_logits(buf, B, g, P, C):  # noqa: N803
    """[B*g*g, >= P*P*C] patch layout -> [B, S, S, C] (token (Y/P)*g + X/P, column ((Y%P)*P + X%P)*C + c)."""
    S = g * P  # noqa: N806
    return buf[:, : P * P * C].reshape(B, g, g, P, P, C).permute(0, 1, 3, 2, 4, 5).reshape(B, S, S, C)


def _expected_ce(buf, target, missing, B, g, P, C):  # noqa: N803
    pred = _raster_logits(buf, B, g, P, C).argmax(dim=-1).reshape(-1)
    t = target.reshape(-1).long()
    valid = (t != missing) & (t >= 0) & (t < C)
    return torch.bincount(t[valid] * C + pred[valid], minlength=C * C).view(C, C)


def _run_ce(buf, target, missing, B, g, P, C, ld, cm=None):  # noqa: N803
    cm = torch.zeros(C, C, dtype=torch.int64, device=DEV) if cm is None else cm
    hip.confusion_ce(buf.to(DEV), target.to(DEV), missing, cm, B, g, P, C, ld)
    torch.cuda.synchronize()
    return cm.cpu()


# ----------------------------------------------------------------------------------------------------- mh_confusion_ce: the grid
@pytest.mark.parametrize("BgP", [(1, 1, 1), (3, 1, 1), (1, 3, 2), (2, 2, 4), (2, 8, 16)], ids=lambda v: "B%d-g%d-P%d" % v)
@pytest.mark.parametrize("C", [2, 6, 19, 74, 128])
def test_confusion_ce_equals_torch(C, BgP):  # noqa: N803
    B, g, P = BgP  # noqa: N806
    S, cols = g * P, P * P * C  # noqa: N806
    tg = torch.Generator().manual_seed(1000 * C + B * g * P)
    for ld in (cols, (cols + 7) // 8 * 8 + 8):
        buf = _logits(B * g * g, cols, ld, seed=C * 131 + ld)
        for tbytes in (1, 2, 4, 8):
            target = torch.randint(-1, min(C, 127) + 1, (B, S, S), generator=tg).to(INT[tbytes])     # -1 and C occur: both skipped
            for missing in (-1, C):
                want = _expected_ce(buf, target, missing, B, g, P, C)
                got = _run_ce(buf, target, missing, B, g, P, C, ld)
                assert torch.equal(got, want), (ld, tbytes, missing, int((got - want).abs().sum()))
                assert int(want.sum()) == int(((target.long() >= 0) & (target.long() < C)).sum())


def test_confusion_ce_missing_out_of_range_and_accumulation():
    B, g, P, C = 2, 3, 4, 6  # noqa: N806
    S, cols = g * P, P * P * C  # noqa: N806
    buf = _logits(B * g * g, cols, cols, seed=7)
    pre = (2**33 + torch.arange(C * C)).view(C, C)                        # the adds are 64-bit
    # a raster that is all missing leaves cm bit-unchanged, for either convention
    for missing in (-1, C):
        cm = pre.clone().to(DEV)
        got = _run_ce(buf, torch.full((B, S, S), missing, dtype=torch.int64), missing, B, g, P, C, cols, cm=cm)
        assert torch.equal(got, pre)
    # targets outside [0, C) are skipped whatever missing_val is
    target = torch.randint(0, C, (B, S, S), generator=torch.Generator().manual_seed(8))
    wild = target.clone()
    wild[0, 0, :5] = torch.tensor([-7, C, C + 1, 1000, -1])
    wild[1, 5, 5] = 2**40
    want = _expected_ce(buf, wild, -1, B, g, P, C)
    assert int(want.sum()) == B * S * S - 6
    assert torch.equal(_run_ce(buf, wild, -1, B, g, P, C, cols), want)
    # two calls accumulate, on top of 2^33 + k per cell
    cm = pre.clone().to(DEV)
    _run_ce(buf, target, -1, B, g, P, C, cols, cm=cm)
    got = _run_ce(buf, wild, -1, B, g, P, C, cols, cm=cm)
    assert torch.equal(got, pre + _expected_ce(buf, target, -1, B, g, P, C) + want)


def test_confusion_ce_ties_and_nan_follow_torch_argmax():
    B, g, P, C = 1, 2, 2, 19  # noqa: N806
    S, cols = g * P, P * P * C  # noqa: N806
    dense = _logits(B * g * g, cols, cols, seed=11)
    px = dense.view(-1, C)                                                # one row per pixel, in memory order
    px[0] = 0.25                                                          # all equal -> class 0
    px[1] = -3.0
    px[1, 4] = px[1, 17] = 2.0                                            # exact two-way tie -> the lower index
    px[2, 9] = float("nan")                                               # one NaN among finite values is the arg-max
    px[3, 12] = px[3, 3] = float("nan")                                   # the first NaN wins
    px[4] = float("-inf")
    px[5, 18] = float("inf")
    px[6, 0], px[6, 7] = 0.0, -0.0                                        # equal for argmax
    px[6, 1:7] = -1.0
    px[6, 8:] = -1.0
    pred = px.argmax(dim=-1)
    assert pred[:7].tolist() == [0, 4, 9, 3, 0, 18, 0]
    buf = torch.full((B * g * g, cols + 5), float("nan"))                 # odd ld: NaN pad columns, 4-byte aligned rows
    buf[:, :cols] = dense
    target = torch.randint(0, C, (B, S, S), generator=torch.Generator().manual_seed(12), dtype=torch.int32)
    want = _expected_ce(buf, target, -1, B, g, P, C)
    assert torch.equal(_run_ce(buf, target, -1, B, g, P, C, cols + 5), want)


def test_confusion_ce_contention_on_one_cell():
    B, g, P, C = 1, 32, 16, 6  # noqa: N806           2^18 pixels, every one (target 4, prediction 2)
    cols = P * P * C
    buf = torch.zeros(B * g * g, cols).view(-1, C)
    buf[:, 2] = 1.0
    target = torch.full((B, g * P, g * P), 4, dtype=torch.int8)
    got = _run_ce(buf.view(B * g * g, cols), target, -1, B, g, P, C, cols)
    want = torch.zeros(C, C, dtype=torch.int64)
    want[4, 2] = 262144
    assert torch.equal(got, want)


# ----------------------------------------------------------------------------------------------------- mh_confusion_bce
def _bce_case(B, C, thr, seed):  # noqa: N803
    g = torch.Generator().manual_seed(seed)
    lt = math.log(thr / (1 - thr))
    x = torch.randn(B, C, generator=g)
    x = (lt + torch.where(x >= 0, x + 2e-3, x - 2e-3)).float()            # |x - logit_threshold| >= 1e-3 after the fp32 rounding
    assert bool(((x.double() - lt).abs() >= 1e-3).all())
    t = (torch.rand(B, C, generator=g) > 0.5).float()
    miss = torch.rand(B, generator=g) < 0.3                               # these rows carry ONE missing entry
    cols = torch.randint(0, C, (B,), generator=g)
    t[miss, cols[miss]] = -1.0
    return x, t


def _expected_bce(x, t, missing, thr):
    used = (t != missing).all(dim=1)
    pred = (torch.sigmoid(x[used]) > thr).long()
    tt = (t[used] > 0.5).long()
    C = x.shape[1]  # noqa: N806
    lbl = torch.arange(C).expand_as(tt)
    return torch.bincount((lbl * 4 + tt * 2 + pred).reshape(-1), minlength=4 * C).view(C, 2, 2)


@pytest.mark.parametrize("thr", [0.5, 0.3])
@pytest.mark.parametrize("C", [1, 15, 18])
@pytest.mark.parametrize("B", [1, 5, 300])
def test_confusion_bce_equals_torch(B, C, thr):  # noqa: N803
    x, t = _bce_case(B, C, thr, seed=B * 100 + C)
    want = _expected_bce(x, t, -1.0, thr)
    cm = torch.zeros(C, 2, 2, dtype=torch.int64, device=DEV)
    hip.confusion_bce(x.to(DEV), t.to(DEV), -1.0, thr, cm, B, C)
    hip.confusion_bce(x.to(DEV), t.to(DEV), -1.0, thr, cm, B, C)              # the call adds
    torch.cuda.synchronize()
    assert torch.equal(cm.cpu(), 2 * want)
    assert int(want.sum()) == int((t != -1.0).all(dim=1).sum()) * C


def test_metric_classes_on_reference_shaped_tensors():
    """The engine-free form: ``update(logits [N, C], targets [N])`` and the multilabel ``update(logits, targets)``; change_detect."""
    C, N = 6, 777  # noqa: N806
    buf = _logits(N, C, C, seed=21)
    target = torch.randint(0, C, (N,), generator=torch.Generator().manual_seed(22))
    m = MonoLabelMetric("classif", C)
    m.update(buf.to(DEV), target.to(DEV))
    m.update(buf.to(DEV), target.to(DEV))
    want = 2 * _expected_ce(buf, target, -1, N, 1, 1, C)
    out = m.compute()
    assert torch.equal(out["confusion_matrix"].cpu(), want)
    assert float(out["overall_accuracy"]) == float(want.trace().double() / want.sum().double())
    m.reset()
    assert int(m.cm.sum()) == 0
    x, t = _bce_case(40, 15, 0.5, seed=23)
    ml = MultiLabelMetric(15)
    ml.update(x.to(DEV), t.clamp(min=0).to(DEV))                              # reference form: rows already selected
    ml.update(x.to(DEV), t.to(DEV), missing_val=-1.0)                          # engine form: rows with a missing entry skipped
    used = (t != -1.0).all(dim=1)
    out = ml.compute()
    assert torch.equal(ml.cm.cpu(), _expected_bce(x, t.clamp(min=0), -1.0, 0.5) + _expected_bce(x, t, -1.0, 0.5))
    assert [tuple(p.shape) for p in ml.preds] == [(40, 15), (int(used.sum()), 15)] and ml.target[1].dtype == torch.int64
    assert torch.equal(ml.target[1].cpu(), t[used].long()) and all(math.isfinite(float(v)) for v in out.values())
    cd = MonoLabelMetric("change_detect", None, threshold_detect=0.3)
    xb, tb = _bce_case(300, 1, 0.3, seed=24)
    tb = tb.clamp(min=0)
    cd.update(xb.view(-1).to(DEV), tb.view(-1).long().to(DEV))
    assert torch.equal(cd.cm.cpu(), _expected_bce(xb, tb, -1.0, 0.3)[0])


# ----------------------------------------------------------------------------------------------------- guard bands (tests/guards.py)
# The ledger of tests/guards.py counts the calls below this banner: operands in the middle of poisoned allocations, NaN pad
# columns, bands / pads / inputs bit-identical afterwards, the result equal to the dense-operand answer.  Every size and index
# passed is in range.  Nothing below may name a wrapper without calling it on guarded operands.
@pytest.mark.parametrize("case", [dict(B=2, g=3, P=2, C=6, tbytes=8, align=16), dict(B=1, g=2, P=4, C=128, tbytes=1, align=16),
                                  dict(B=3, g=1, P=1, C=19, tbytes=4, align=16), dict(B=2, g=2, P=4, C=74, tbytes=2, align=4)],
                         ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_guard_bands_confusion_ce(case):
    B, g, P, C = case["B"], case["g"], case["P"], case["C"]  # noqa: N806
    S, cols = g * P, P * P * C  # noqa: N806
    ld = (cols + 7) // 8 * 8 + 8                                          # NaN pad columns behind every row
    dense = _logits(B * g * g, cols, cols, seed=31 + C)
    # (int8 band bytes 0x5B = 91 are a VALID class for C = 128: a target read past the raster would be counted and show in cm)
    target = torch.randint(-1, min(C, 127) + 1, (B, S, S), generator=torch.Generator().manual_seed(32)).to(INT[case["tbytes"]])
    missing = -1                                                          # != the INT_PATTERN bytes of the target's bands
    gs = GuardSet(DEV)
    lg = gs.inp(dense, ld=ld, align=case["align"], name="logits")
    tg = gs.inp(target.view(B * S, S), fill="int", align=case["tbytes"] if case["tbytes"] > 2 else 4, name="target")
    cm = gs.out((C, C), dtype=torch.int64, init=0, name="cm")
    gs.arm()
    hip.confusion_ce(lg, tg, missing, cm, B, g, P, C, ld)
    gs.check()
    assert torch.equal(cm.cpu(), _expected_ce(dense, target, missing, B, g, P, C))


@pytest.mark.parametrize("B,C", [(5, 18), (300, 15), (7, 1)])
def test_guard_bands_confusion_bce(B, C):  # noqa: N803
    x, t = _bce_case(B, C, 0.3, seed=41 + B)
    gs = GuardSet(DEV)
    xg = gs.inp(x, align=4, name="logits")
    tg = gs.inp(t, align=4, name="target")
    cm = gs.out((C * 2, 2), dtype=torch.int64, init=0, name="cm")
    gs.arm()
    hip.confusion_bce(xg, tg, -1.0, 0.3, cm, B, C)
    gs.check()
    assert torch.equal(cm.cpu().view(C, 2, 2), _expected_bce(x, t, -1.0, 0.3))


# ----------------------------------------------------------------------------------------------------- end to end
def _ap_numpy(scores, y):
    scores, y = np.asarray(scores, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n_pos = y.sum()
    if n_pos == 0:
        return float("nan")
    ap, r_prev = 0.0, 0.0
    for thr in sorted(set(scores.tolist()), reverse=True):
        sel = scores >= thr
        tp = y[sel].sum()
        ap += (tp / n_pos - r_prev) * (tp / sel.sum())
        r_prev = tp / n_pos
    return ap


def _close(got, want):
    got, want = float(got), float(want)
    return (math.isnan(got) and math.isnan(want)) or abs(got - want) <= 1e-12


@pytest.mark.parametrize("name", ["sup_flair_seg", "sup_treesat_mlc", "sup_pastis_two"])
def test_validation_steps_fill_the_metrics_from_the_engines_logits(name):
    from maestro_amd.train.model import SSLModule
    case, ds, oracle, _, batch = build_sup_case(name)
    module = SSLModule(datasets=ds, mask=conf.MaskConfig(), interpolate="nearest", fusion_mode=case["fusion"],
                       inter_depth=case["inter_depth"], model="mae", model_size=case["size"], type_head=case["type_head"])
    model = getattr(pmae, f"mae_{case['size']}")(
        datasets=ds, mask=conf.MaskConfig(), interpolate="nearest", fusion_mode=case["fusion"], inter_depth=case["inter_depth"],
        model="mae", num_levels=1, type_head=case["type_head"], fac_abs_enc=1.0, fac_date_enc=1.0, **case["model_kw"])
    model.load_state_dict(oracle.state_dict(), strict=True)
    module.model = model                                   # the golden case's (shallower) network, as tests/test_sup_gpu.py::_setup
    module.trainer = SimpleNamespace(ssl_phase="probe")
    dbatch = {k: v.to(DEV) for k, v in batch.items()}
    targets = ds.dataset.targets
    want = {}
    for _ in range(3):                                     # eager, hipGraph capture, replay
        module.validation_step(dbatch, 0)
        logits = module.model._sup_engine.logits()
        torch.cuda.synchronize()
        for t, c in targets.items():
            lg, y = logits[t].cpu(), batch[t]
            if c.type_target == "multilabel_classif":
                step = _expected_bce(lg, y.float().reshape(lg.shape), float(c.missing_val), 0.5)
            else:
                C = c.num_classes  # noqa: N806
                pred = lg.movedim(-3, -1).argmax(dim=-1).reshape(-1) if c.type_target == "segment" else lg.argmax(dim=1)
                tt = y.reshape(-1).long()
                valid = (tt != c.missing_val) & (tt >= 0) & (tt < C)
                step = torch.bincount(tt[valid] * C + pred[valid], minlength=C * C).view(C, C)
            want[t] = want.get(t, 0) + step
    for t, c in targets.items():
        metric = module.metrics[f"{t}_val"]
        assert int(module.metrics[f"{t}_train"].cm.sum()) == 0 and int(module.metrics[f"{t}_test"].cm.sum()) == 0
        assert int(want[t].sum()) > 0
        assert torch.equal(metric.cm.cpu(), want[t]), t
        out = metric.compute()
        cm = want[t].double()
        if c.type_target == "multilabel_classif":
            tp, fp, fn = cm[:, 1, 1], cm[:, 0, 1], cm[:, 1, 0]
            f1, w = 2 * tp / (2 * tp + fp + fn), (tp + fn) / (tp + fn).sum()
            scores, ys = torch.cat(metric.preds).cpu(), torch.cat(metric.target).cpu()
            used = (batch[t].float().reshape(-1, c.num_classes) != c.missing_val).all(dim=1)
            lg = module.model._sup_engine.logits()[t].cpu()
            assert scores.shape[0] == 3 * int(used.sum()) and torch.equal(ys[: int(used.sum())], batch[t].reshape(-1, c.num_classes)[used].long())
            assert torch.allclose(scores[: int(used.sum())], torch.sigmoid(lg[used]), atol=1e-6, rtol=0)
            ap = torch.tensor([_ap_numpy(scores[:, i].numpy(), ys[:, i].numpy()) for i in range(c.num_classes)], dtype=torch.float64)
            exp = {"average_f1": f1.nanmean(), "average_ap": ap.nanmean(), "weighted_f1": (f1 * w).nansum(),
                   "weighted_ap": (ap * w).nansum()}
            assert list(out) == list(exp)
            for k in exp:
                assert _close(out[k], exp[k]), (t, k, float(out[k]), float(exp[k]))
        else:
            tp = cm.diag()
            fp, fn = cm.sum(0) - tp, cm.sum(1) - tp
            valid = (tp + fn) != 0
            assert torch.equal(out["confusion_matrix"].cpu(), want[t])
            assert _close(out["overall_accuracy"], cm.trace() / cm.sum())
            if c.type_target == "segment":
                assert _close(out["average_f1"], (2 * tp / (2 * tp + fp + fn))[valid].mean())
                assert _close(out["average_iou"], (tp / (tp + fp + fn))[valid].mean())
            else:
                assert list(out) == ["overall_accuracy", "confusion_matrix"]
