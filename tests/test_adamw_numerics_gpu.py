"""``mh_adamw`` / ``mh_adamw_dev`` against fp64 under the elementwise bounds of tests/numerics.py (``adamw_bounds``: derived
from the roundings of ``adamw_update``, csrc/optim.hip; accepted and rejected forms in tests/test_step_end_selfcheck.py).

Single steps from given ``(p, g, m, v)``: eight kinds of operands (eps visible, cancelling and underflowing moments, large and
zero parameters) crossed with early and late steps at a ``grad_scale`` that is no power of two; ``p``, ``m`` and ``v`` are all
compared, ``p_bf16`` is ``p.bfloat16()`` bit for bit, and the device-scalar entry gives the bits of the by-value one.  Then twenty
steps from zero moments on a shrinking gradient sequence against the fp64 trajectory, held to ``norm_ceiling`` over
torch.optim.AdamW (fp32, CPU) and the emulation.

The bounds assume correctly rounded ``/`` and ``sqrtf`` (hipcc's default; build.py passes no fast-math flag).
"""

from __future__ import annotations

import pytest
import torch

from tests import numerics as nm

pytestmark = pytest.mark.gpu
N = 4100            # four workgroups of 1024 elements and a tail of four


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _run(dev, p, g, m, v, step, b2, device_scalars):
    from maestro_amd import hip
    h = nm.ADAMW_HYPER
    p, m, v = p.to(dev).clone(), m.to(dev).clone(), v.to(dev).clone()
    pb = torch.full((N,), float("nan"), dtype=torch.bfloat16, device=dev)
    if device_scalars:
        bc1, bc2_sqrt = hip.adamw_bias_corrections(h["b1"], b2, step)
        hyper = torch.tensor([h["lr"], bc1, bc2_sqrt, h["grad_scale"], 1.0], dtype=torch.float32, device=dev)
        hip.adamw_dev(p, g.to(dev), m, v, pb, N, h["b1"], b2, h["eps"], h["wd"], hyper)
    else:
        hip.adamw(p, g.to(dev), m, v, pb, N, h["lr"], h["b1"], b2, h["eps"], h["wd"], step, h["grad_scale"])
    return p, m, v, pb


@pytest.mark.parametrize("step,b2", nm.ADAMW_STEPS)
@pytest.mark.parametrize("kind", nm.ADAMW_KINDS)
def test_adamw_single_step(dev, observed, kind, step, b2):
    from maestro_amd import hip
    h = nm.ADAMW_HYPER
    p, g, m, v = nm.adamw_inputs(kind, N)
    got = _run(dev, p, g, m, v, step, b2, device_scalars=False)
    got_dev = _run(dev, p, g, m, v, step, b2, device_scalars=True)
    for a, b, name in zip(got, got_dev, ("p", "m", "v", "p_bf16")):
        assert torch.equal(_bits(a), _bits(b)), f"mh_adamw_dev: {name} differs from mh_adamw's"
    bc1, bc2_sqrt = hip.adamw_bias_corrections(h["b1"], b2, step)
    ref = nm.adamw_step64(p, g, m, v, h["lr"], h["b1"], b2, h["eps"], h["wd"], bc1, bc2_sqrt, h["grad_scale"])
    bound = nm.adamw_bounds(ref)
    for t, k in zip(got[:3], "pmv"):
        assert bool(torch.isfinite(t).all()), f"{k} is not finite"
        r = nm.worst_ratio((t.double().cpu() - ref[k]).abs(), bound[k])
        print(f"adamw {kind} step {step} {k}: worst error / bound = {r:.3f}")
        observed("adamw_numerics_gpu::single_step", f"{kind}/step{step}/{k}", r)
        assert r <= 1.0, (kind, step, k, r)
    assert torch.equal(_bits(got[3]), _bits(got[0].bfloat16())), "p_bf16 is not p.bfloat16()"
    if kind == "zero":      # nothing to move by: the moments stay zero and p only decays
        assert float(got[1].abs().max()) == 0.0 and float(got[2].abs().max()) == 0.0
        assert bool((ref["step"] == 0).all())


def test_adamw_trajectory(dev, observed):
    from maestro_amd import hip
    case = nm.adamw_trajectory_case(N)
    h = case["hyper"]
    p, m, v = case["p0"].to(dev).clone(), torch.zeros(N, device=dev), torch.zeros(N, device=dev)
    grads = case["grads"].to(dev)
    for t in range(case["steps"]):
        hip.adamw(p, grads[t], m, v, None, N, h["lr"], h["b1"], h["b2"], h["eps"], h["wd"], t + 1, 1.0)
    errs = nm.adamw_trajectory_errors(case, (p, m, v))
    for k in "pmv":
        got, ceiling = errs[k]
        print(f"adamw trajectory {k}: error {got:.3e}, ceiling {ceiling:.3e} (ratio {got / ceiling:.3f})")
        observed("adamw_numerics_gpu::trajectory", k, got / ceiling)
        assert got <= ceiling, (k, got, ceiling)
