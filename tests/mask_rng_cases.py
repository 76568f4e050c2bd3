"""Shared by tests/test_mask_rng_host.py and tests/test_mask_rng_gpu.py (a plain helper module): the tiny product models
behind the goldens, built without the oracle, and hand-built ``GroupSpec`` / ``ModSpec`` tables for ``mh_mask_draw``."""

from __future__ import annotations

import torch

import maestro_amd.conf as conf
from maestro_amd.ssl import mae as pmae
from maestro_amd.ssl.mae import GroupSpec, ModSpec
from oracle.gen_golden import build_datasets, case_table, make_batch

COMMON = dict(interpolate="nearest", model="mae", num_levels=1, type_head="attentive", fac_abs_enc=1.0, fac_date_enc=1.0)
# "group": the dem + s1_asc / s1_des case (group fusion; a group of two modalities, mask_mod / mask_dates / mask_loc active)
ENGINE_CASES = {"group": "c3p_dem_s1", "ts_shared": "ts_shared", "ts_mod": "ts_mod", "ts_monotemp": "ts_monotemp",
                "bg_ts_monotemp": "bg_ts_monotemp"}


def build_model(name: str, B: int | None = None, depth: int = 2, seed: int = 0):  # noqa: N803
    """``(model, batch, B)`` of a golden's tiny configuration with the depth cut to ``depth`` (CPU tensors; random weights)."""
    case = case_table()[ENGINE_CASES.get(name, name)]
    ds = build_datasets(case, conf)
    kw = dict(fusion_mode=case["fusion"], inter_depth=min(case["inter_depth"], depth - 1), **COMMON, **{**case["model_kw"], "depth": depth})
    torch.manual_seed(100 + seed)
    model = getattr(pmae, f"mae_{case['size']}")(datasets=ds, mask=conf.MaskConfig(**case.get("mask_kw", {})), **kw)
    B = case["B"] if B is None else B  # noqa: N806
    return model, make_batch(ds.dataset, B, case["seed"]), B


def set_beff(model, B: int):  # noqa: N803
    """What ``MAEEngine.__init__`` does to the specs: sequences per step."""
    fold = model.fusion_mode in ("shared", "monotemp")
    for s in model.mod_specs.values():
        s.Beff = B * s.Dates if fold else B
    groups = list(model.group_specs.values())
    for g in groups:
        g.Beff = g.mods[0].Beff
    return groups, model.mod_specs


def _mod(name, group, L, D, Dates, tok_off, p, src=None, gi=0, G=1):  # noqa: N803
    g = int(round(L ** 0.5))
    return ModSpec(name=name, embed=src or name, group=group, C=1, S=g, P=1, g=g, L=L, D=D, Dates=Dates, tok_off=tok_off,
                   p_mod=p[0], p_bands=p[1], p_dates=p[2], p_loc=p[3], src=src or name, gi=gi, G=G)


def hand_built(L: int, kinds: str = "mbdl", p_mod: float = 0.9, two_mods: bool = False):  # noqa: N803
    """Unfolded groups (Beff = B): ``ga`` = both band-groups of modality ``a`` (D = 2 dates, ``L`` tokens per date; with
    ``two_mods`` also modality ``b`` with D = 1 and another L), ``gc`` = modality ``c`` alone (D = 2).  ``kinds``: which of
    mod / bands / dates / loc are active."""
    p = (p_mod if "m" in kinds else None, 0.4 if "b" in kinds else None, 0.5 if "d" in kinds else None, 0.6 if "l" in kinds else None)
    a0 = _mod("a#0", "ga", L, 2, 2, 0, p, src="a", gi=0, G=2)
    a1 = _mod("a#1", "ga", L, 2, 2, 2 * L, p, src="a", gi=1, G=2)
    mods = [a0, a1]
    if two_mods:
        Lb = 9 if L != 9 else 4  # noqa: N806   (4 L + Lb: no multiple of 4 unless L = 9)
        mods.append(_mod("b", "ga", Lb, 1, 1, 4 * L, (p[0], None, None, 0.3 if "l" in kinds else None)))
    c = _mod("c", "gc", L, 2, 2, 0, (None, None, p[2], p[3]))
    ga = GroupSpec(name="ga", model="ga", mods=mods, L=sum(m.n_tok for m in mods), draw="ga")
    gc = GroupSpec(name="gc", model="gc", mods=[c], L=c.n_tok, draw="gc")
    return [ga, gc], {m.name: m for m in [*mods, c]}


def hand_built_folded(L: int):  # noqa: N803
    """Dates AND band-groups folded into the batch (Beff = B * 2 dates): two band-groups of modality ``a`` as sequence sets of
    their own that take rows (b, draw_g, d) of ONE noise draw; no structural masks (as the product's folded modes)."""
    none = (None, None, None, None)
    a0 = _mod("a#0", "a#0", L, 1, 2, 0, none, src="a", gi=0, G=2)
    a1 = _mod("a#1", "a#1", L, 1, 2, 0, none, src="a", gi=1, G=2)
    g0 = GroupSpec(name="a#0", model="a", mods=[a0], L=L, draw="a", draw_g=0, draw_G=2)
    g1 = GroupSpec(name="a#1", model="a", mods=[a1], L=L, draw="a", draw_g=1, draw_G=2)
    return [g0, g1], {"a#0": a0, "a#1": a1}
