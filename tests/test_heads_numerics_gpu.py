"""The probe / finetune head kernels (csrc/heads.hip) on exact operands and against fp64 references under derived bounds.

Every case, expectation and bound comes from tests/heads_numerics.py; tests/test_heads_selfcheck.py shows on the CPU that those
very cases reject every named wrong form and accept the honest fp32 emulation.  Outputs are NaN-filled (or preloaded with known
values) before each call; a quantity passes at ``ratio = max(error / bound) <= 1`` (exact quantities: 0 or inf), and every ratio
goes to ``observed`` first (profiles/heads_numerics.md).  Nothing is excluded and nothing skipped: the shapes are the smallest
at which each path of each kernel can still go wrong, and the fp64 references are computed on the CPU once per case.
"""

import pytest
import torch

from tests import heads_numerics as hn

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _nan(shape, dev, dtype=torch.float32):
    return torch.full(shape, float("nan"), device=dev, dtype=dtype)


def _settle(observed, family, case, ratios, prefix=""):
    """Record every ratio, print it, then assert."""
    bad = []
    for key, r in ratios.items():
        observed("heads_numerics_gpu", f"{family}/{hn.case_id(case)}/{prefix}{key}", r)
        print(f"{family} {hn.case_id(case)} {prefix}{key}: {r:.4g}")
        if not r <= 1.0:
            bad.append(f"{prefix}{key}: {r:.4g} x its bound" if r != hn.INF else f"{prefix}{key}: differs from its exact expectation (or is not finite)")
    assert not bad, f"{family} {hn.case_id(case)}: " + "; ".join(bad)


def _unchanged(dev_tensors, host_tensors):
    return all(hn.same_bits(a.cpu(), b) for a, b in zip(dev_tensors, host_tensors))


# ------------------------------------------------------------------------------------------------ resize
@pytest.mark.parametrize("case", hn.RESIZE_CASES, ids=hn.case_id)
def test_token_resize(dev, observed, case):
    from maestro_amd import hip
    d = hn.resize_case(*case)
    B, D, h, H, E = d["B"], d["D"], d["h"], d["H"], d["E"]  # noqa: N806
    x, dout = d["x"].to(dev), d["dout"].to(dev)
    out = _nan((B, d["out_rows"], E), dev)
    hip.token_resize(x, d["in_rows"], hn.RESIZE_IN_OFF, out, d["out_rows"], hn.RESIZE_OUT_OFF, B, D, h, H, E)
    din0, din1 = _nan((B, d["in_rows"], E), dev), d["pre"].to(dev)
    hip.token_resize_bwd(dout, d["out_rows"], hn.RESIZE_OUT_OFF, din0, d["in_rows"], hn.RESIZE_IN_OFF, B, D, h, H, E, accumulate=False)
    hip.token_resize_bwd(dout, d["out_rows"], hn.RESIZE_OUT_OFF, din1, d["in_rows"], hn.RESIZE_IN_OFF, B, D, h, H, E, accumulate=True)
    torch.cuda.synchronize()
    assert _unchanged((x, dout), (d["x"], d["dout"]))
    _settle(observed, "resize", case, hn.resize_ratios(d, dict(out=out.cpu(), din0=din0.cpu(), din1=din1.cpu())))


# ------------------------------------------------------------------------------------------------ attentive reduction
def _ar_backward(hip, d, kv, query, out, lse, dout, dev):
    nb, T, Lr, dim = d["nb"], d["T"], d["Lr"], d["dim"]  # noqa: N806
    dkv = _nan(tuple(kv.shape), dev, torch.bfloat16)
    part = _nan((hip.attn_reduce_partial_rows(nb * Lr), dim), dev)          # every row must be written, idle waves' too
    hip.attn_reduce_bwd(kv, query, out, lse, dout, dkv, part, nb, T, Lr, dim)
    torch.cuda.synchronize()
    return dict(out=out.cpu(), lse=lse.cpu(), dkv=dkv.float().cpu(), dq=part.cpu())


@pytest.mark.parametrize("case", hn.AR_CASES, ids=hn.case_id)
def test_attentive_reduce(dev, observed, case):
    """Forward, then the backward twice: chained on the forward kernel's own out / lse (their measured errors go into the
    bounds), and standalone on the fp32 images of the fp64 out / lse."""
    from maestro_amd import hip
    d = hn.ar_case(*case)
    nb, T, Lr, dim = d["nb"], d["T"], d["Lr"], d["dim"]  # noqa: N806
    assert hip.attn_reduce_partial_rows(nb * Lr) == d["ref"]["dq"].shape[0]
    kv, query, dout = d["kv"].to(dev), d["query"].to(dev), d["dout"].to(dev)
    out, lse = _nan((nb * Lr, dim), dev), _nan((nb * Lr, 8), dev)
    hip.attn_reduce_fwd(kv, query, out, lse, nb, T, Lr, dim)
    chained = _ar_backward(hip, d, kv, query, out, lse, dout, dev)
    alone = _ar_backward(hip, d, kv, query, d["ref"]["out"].float().to(dev), d["ref"]["lse"].float().to(dev), dout, dev)
    assert _unchanged((kv, query, dout), (d["kv"], d["query"], d["dout"]))
    r = hn.ar_ratios(d, chained)
    if d["kind"] not in hn.AR_EXACT_KINDS:      # exact kinds: out / lse are exact themselves, the chained run is the standalone one
        r.update({"alone_" + k: v for k, v in hn.ar_ratios(d, alone).items() if k in ("dk", "dv", "dq", "finite")})
    _settle(observed, "attn_reduce", case, r)


# ------------------------------------------------------------------------------------------------ mean reduction
@pytest.mark.parametrize("case", hn.MEAN_CASES, ids=hn.case_id)
def test_mean_reduce(dev, observed, case):
    from maestro_amd import hip
    d = hn.mean_case(*case)
    nb, T, Lr, dim = d["nb"], d["T"], d["Lr"], d["dim"]  # noqa: N806
    out, dx = _nan((nb * Lr, dim), dev), _nan((nb * T * Lr, dim), dev)
    hip.mean_reduce_fwd(d["x"].to(dev), out, nb, T, Lr, dim)
    hip.mean_reduce_bwd(d["dout"].to(dev), dx, nb, T, Lr, dim)
    torch.cuda.synchronize()
    _settle(observed, "mean_reduce", case, hn.mean_ratios(d, dict(out=out.cpu(), dx=dx.cpu())))


# ------------------------------------------------------------------------------------------------ classification linear
@pytest.mark.parametrize("case", hn.LINEAR_CASES, ids=hn.case_id)
def test_head_linear(dev, observed, case):
    """Forward; backward with dx; backward with dx = NULL, which must leave the same bits in dW / db and touch nothing else."""
    from maestro_amd import hip
    d = hn.linear_case(*case)
    B, C, E = d["B"], d["C"], d["E"]  # noqa: N806
    x, W, bias, dout = (d[k].to(dev) for k in ("x", "W", "bias", "dout"))  # noqa: N806
    out, dx = _nan((B, C), dev), _nan((B, E), dev)
    hip.head_linear_fwd(x, W, bias, out, B, C, E)
    dW, db = d["pre_w"].to(dev), d["pre_b"].to(dev)  # noqa: N806
    hip.head_linear_bwd(x, W, dout, dx, dW, db, B, C, E)
    dW2, db2 = d["pre_w"].to(dev), d["pre_b"].to(dev)  # noqa: N806
    hip.head_linear_bwd(x, W, dout, None, dW2, db2, B, C, E)
    torch.cuda.synchronize()
    assert _unchanged((x, W, bias, dout), (d["x"], d["W"], d["bias"], d["dout"]))
    got = dict(out=out.cpu(), dx=dx.cpu(), dW=dW.cpu(), db=db.cpu(), dW_nodx=dW2.cpu(), db_nodx=db2.cpu())
    _settle(observed, "head_linear", case, hn.linear_ratios(d, got))


# ------------------------------------------------------------------------------------------------ cross entropy
@pytest.mark.parametrize("case", hn.CE_CASES, ids=hn.case_id)
def test_cross_entropy(dev, observed, case):
    """The n_valid word is written by the test, not by mh_count_valid (checked beside it): the kernel must divide by the word."""
    from maestro_amd import hip
    d = hn.ce_case(*case)
    logits, target = d["logits"].to(dev), d["target"].to(dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    hip.count_valid(target, d["missing"], cnt)
    assert int(cnt.item()) == d["count"]
    word = torch.tensor([d["word"]], dtype=torch.int32, device=dev)
    acc, dl = torch.zeros(1, device=dev), _nan(tuple(logits.shape), dev, d["dd"])
    hip.ce_loss(logits, target, d["missing"], word, acc, dl, d["B"], d["g"], d["P"], d["C"], ld=d["ld"])
    torch.cuda.synchronize()
    assert hn.same_bits(logits.cpu(), d["logits"]) and torch.equal(target.cpu(), d["target"]) and int(word.item()) == d["word"]
    _settle(observed, "ce", case, hn.ce_ratios(d, dict(acc=acc.cpu(), dlogits=dl.cpu())))


# ------------------------------------------------------------------------------------------------ BCE with logits
@pytest.mark.parametrize("case", hn.BCE_CASES, ids=hn.case_id)
def test_bce(dev, observed, case):
    from maestro_amd import hip
    d = hn.bce_case(*case)
    x, t = d["x"].to(dev), d["t"].to(dev)
    acc, dl = torch.full((1,), hn.BCE_ACC0, device=dev), _nan((d["B"], d["C"]), dev)
    hip.bce_loss(x, t, hn.BCE_MISSING, acc, dl, d["B"], d["C"])
    torch.cuda.synchronize()
    assert _unchanged((x, t), (d["x"], d["t"]))
    _settle(observed, "bce", case, hn.bce_ratios(d, dict(acc=acc.cpu(), dlogits=dl.cpu())))
