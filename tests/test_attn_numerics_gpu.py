"""mh_attn_fwd / mh_attn_bwd against an fp64 reference under the a-priori error model of tests/numerics.py (``attn_bounds``; its
teeth: tests/test_numerics_selfcheck.py), across logit scales.

A  elementwise: |got - ref64| <= bound for out, lse, delta, dQ, dK, dV.  The backward runs twice: standalone on bf16(O64) and
   f32(lse64), and chained on the forward kernel's own out / lse with their measured errors handed to the bounds.
B  in norm: ||got - ref64|| <= 2 ||emulated - ref64|| against the torch fp32 emulation of the kernels' arithmetic on the same
   inputs (out, dQ, dK, dV; lse at D = 32 only: at D = 64 its error is fp32 summation order, where a factor 2 means nothing).
   B is skipped only for the (kind, tensor) pairs of B_EXEMPT, and only where the emulation's own error is below 2 % of the
   bound's norm.  Other pairs fall below that share too (the bound is a worst case over signs, the error a random sum: `rising`
   dQ 0.5 %, `neg` / `offset` / `low_after_high` / `spike_late` dK, dV 1.2 ... 2 %, self-check) and stay under B: their error is
   the fold's, which is the same rounding of the same operand in the kernel and in the emulation.

Inputs are seeded on the CPU, the fp64 reference runs on the device, the emulation on the CPU.  A ratios and relative L2 errors
(kernel, emulation, emulation without the bf16 fold) go to ``observed`` (profiles/attn_numerics.md)."""

import pytest
import torch

from tests import numerics as nm

pytestmark = pytest.mark.gpu

# (kind, tensor) pairs for which criterion B may be skipped: a saturated softmax leaves out = one row of v, lse = one logit and
# dQ = dK = 0 up to a few roundings of almost nothing, whose quotient says nothing
B_EXEMPT = frozenset(("peaked", t) for t in ("O", "lse", "dQ", "dK"))
B_TENSORS = {32: ("O", "lse", "dQ", "dK", "dV"), 64: ("O", "dQ", "dK", "dV")}

# N = 200: every kind.  N = 16 less than one wave of queries, 64 exactly one tile, 65 one key in the tail tile, 129 a last
# 128-block that holds a single query (its other waves, q0 >= N, only stage data), 320 five full tiles without a tail.
CASES = [(kind, 200, D, 1, 2) for D in (32, 64) for kind in nm.ATTN_KINDS]
CASES += [(kind, N, D, 1, 2) for D in (32, 64) for N in (16, 64, 65, 129, 320) for kind in ("randn1.5", "offset")]
CASES += [("randn3", 129, 32, 2, 3)]      # D = 32: neighbouring heads share 128-byte lines


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def pack_heads(ops, B, N, H, D, dev):  # noqa: N803
    """ops[b][h] = (q, k, v, do) -> qkv bf16 [B, N, 3, H, D], dout bf16 [B, N, H * D] on the device."""
    qkv = torch.empty(B, N, 3, H, D)
    dout = torch.empty(B, N, H, D)
    for b in range(B):
        for h in range(H):
            q, k, v, do = ops[b][h]
            qkv[b, :, 0, h], qkv[b, :, 1, h], qkv[b, :, 2, h], dout[b, :, h] = q, k, v, do
    return qkv.to(dev).bfloat16(), dout.reshape(B, N, H * D).to(dev).bfloat16()


def run_fwd(qkv, B, N, H, D):  # noqa: N803
    from maestro_amd import hip
    out = torch.full((B, N, H * D), float("nan"), device=qkv.device, dtype=torch.bfloat16)
    lse = torch.full((B, H, N), float("nan"), device=qkv.device)
    hip.attn_fwd(qkv, out, lse, B, N, H, D, D ** -0.5)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out.float()).all()) and bool(torch.isfinite(lse).all()), "forward left NaN / inf"
    return out, lse


def run_bwd(qkv, out, dout, lse, B, N, H, D):  # noqa: N803
    from maestro_amd import hip
    dqkv = torch.full((B, N, 3, H, D), float("nan"), device=qkv.device, dtype=torch.bfloat16)
    delta = torch.full((B, H, N), float("nan"), device=qkv.device)
    hip.attn_bwd(qkv, out, dout, lse, delta, dqkv, B, N, H, D, D ** -0.5)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dqkv.float()).all()) and bool(torch.isfinite(delta).all()), "backward left NaN / inf"
    return dqkv, delta


class Tally:
    """Worst A ratio over the heads of a case and error norms summed over them, per tensor; asserts at the end so that every
    figure is printed and recorded first."""

    def __init__(self, case, kind, D):  # noqa: N803
        self.case, self.kind, self.D = case, kind, D
        self.a, self.sq, self.fails = {}, {}, []

    def add(self, name, tensor, got, emu, nofold, want64, bound):
        err = (got.double() - want64).abs()
        r = nm.worst_ratio(err, bound)
        self.a[name] = max(self.a.get(name, 0.0), r)
        if r > 1.0:
            i = int((err / bound.clamp_min(1e-300)).argmax())
            self.fails.append(f"A {name}: error {r:.3f} x its bound, {int((err > bound).sum())} of {err.numel()} elements outside, worst at "
                              f"flat index {i}: got {float(got.reshape(-1)[i]):.6g}, want {float(want64.reshape(-1)[i]):.6g}")
        applies, e_got, e_emu = nm.attn_criterion_b(got, emu, want64, bound)
        e_nof = float((nofold.double().to(want64.device) - want64).norm())
        s = self.sq.setdefault(name, [0.0, 0.0, 0.0, 0.0])
        for j, e in enumerate((e_got, e_emu, e_nof, float(want64.norm()))):
            s[j] += e * e
        if tensor in B_TENSORS[self.D]:
            if not applies and (self.kind, tensor) in B_EXEMPT:
                print(f"{self.case} {name}: B skipped (emulation error {e_emu:.3e} below 2 % of the bound's norm)")
            elif e_got > nm.B_FACTOR * e_emu:
                self.fails.append(f"B {name}: ||error|| {e_got:.4e} > 2 x the emulation's {e_emu:.4e}")

    def finish(self, observed):
        for name, r in self.a.items():
            g, e, n, w = (x ** 0.5 for x in self.sq[name])
            w = max(w, 1e-300)
            print(f"{self.case} {name}: A {r:.3f}  rel L2 kernel {g / w:.3e}  emulated {e / w:.3e}  without fold {n / w:.3e}")
            for key, val in (("A", r), ("kernel_l2", g / w), ("emulated_l2", e / w), ("nofold_l2", n / w)):
                observed("attn_numerics_gpu", f"{self.case}/{name}/{key}", val)
        assert not self.fails, "\n".join(self.fails)


@pytest.mark.parametrize("kind,N,D,B,H", CASES, ids=[f"{k}-N{n}-D{d}-B{b}H{h}" for k, n, d, b, h in CASES])
def test_attention_error_model(dev, observed, kind, N, D, B, H):  # noqa: N803
    ops = [[nm.attn_operands(kind, N, D, seed=1 + b * H + h) for h in range(H)] for b in range(B)]
    qkv, dout = pack_heads(ops, B, N, H, D, dev)
    refs = [[nm.attn_ref64(*(t.to(dev) for t in ops[b][h])) for h in range(H)] for b in range(B)]
    out, lse = run_fwd(qkv, B, N, H, D)
    out64 = torch.stack([torch.stack([refs[b][h]["O"] for h in range(H)], 1) for b in range(B)]).reshape(B, N, H * D)
    lse64 = torch.stack([torch.stack([refs[b][h]["lse"] for h in range(H)]) for b in range(B)])
    d_s, delta_s = run_bwd(qkv, out64.float().bfloat16(), dout, lse64.float(), B, N, H, D)      # standalone
    d_c, delta_c = run_bwd(qkv, out, dout, lse, B, N, H, D)                                      # chained
    tally = Tally(f"{kind}/N{N}/D{D}/B{B}H{H}", kind, D)
    for b in range(B):
        for h in range(H):
            q, k, v, do = ops[b][h]
            ref = refs[b][h]
            dops = tuple(t.to(dev) for t in ops[b][h])
            o_k = out[b].reshape(N, H, D)[:, h].float()
            l_k = lse[b, h]
            bnd = nm.attn_bounds(ref, *dops)
            o_e, l_e = nm.attn_emulated_fwd(q, k, v)
            tally.add("O", "O", o_k, o_e, o_e, ref["O"], bnd["O"])
            tally.add("lse", "lse", l_k, l_e, l_e, ref["lse"], bnd["lse"])
            runs = (("s_", d_s, delta_s, bnd, nm.bf16_round(ref["O"].float()).cpu(), ref["lse"].float().cpu()),
                    ("c_", d_c, delta_c,
                     nm.attn_bounds(ref, *dops, lse_err=(l_k.double() - ref["lse"]).abs() + nm.U_F32 * ref["lse"].abs(),
                                    out_err=(o_k.double() - ref["O"]).abs()), o_k.cpu(), l_k.cpu()))
            for pre, dqkv, delta, bd, o_in, l_in in runs:
                emu = nm.attn_emulated_bwd(q, k, v, do, o_in, l_in)
                nof = nm.attn_emulated_bwd(q, k, v, do, o_in, l_in, fold=False)
                got = (dqkv[b, :, 0, h].float(), dqkv[b, :, 1, h].float(), dqkv[b, :, 2, h].float(), delta[b, h])
                for i, t in enumerate(("dQ", "dK", "dV", "delta")):
                    tally.add(pre + t, t, got[i], emu[i], nof[i], ref[t], bd[t])
    tally.finish(observed)


@pytest.mark.parametrize("D", [32, 64])
def test_attention_power_of_two_scaling_is_exact(dev, D):  # noqa: N803
    """No tolerance: the backward is linear in dO and the forward's output linear in V, and a power of two commutes with every
    rounding (nothing here comes near underflow), so any absolute epsilon or threshold in the kernels would show as a bit."""
    B, N, H = 1, 129, 2  # noqa: N806
    ops = [[nm.attn_operands("randn1.5", N, D, seed=11 + h) for h in range(H)]]
    qkv, dout = pack_heads(ops, B, N, H, D, dev)
    out, lse = run_fwd(qkv, B, N, H, D)
    dqkv, delta = run_bwd(qkv, out, dout, lse, B, N, H, D)
    dqkv2, delta2 = run_bwd(qkv, out, (dout.float() * 2.0 ** -14).bfloat16(), lse, B, N, H, D)
    assert torch.equal(dqkv2.float(), dqkv.float() * 2.0 ** -14), int((dqkv2.float() != dqkv.float() * 2.0 ** -14).sum())
    assert torch.equal(delta2, delta * 2.0 ** -14)
    qkv8 = qkv.clone()
    qkv8[:, :, 2] = (qkv[:, :, 2].float() * 8.0).bfloat16()
    out8, lse8 = run_fwd(qkv8, B, N, H, D)
    assert torch.equal(out8.float(), out.float() * 8.0), int((out8.float() != out.float() * 8.0).sum())
    assert torch.equal(lse8, lse)
