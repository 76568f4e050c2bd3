"""Fused AdamW over the engine's flat parameter buffer + the reference's OneCycle schedule.

Reference: ``maestro/train/model.py:120-158`` (AdamW(lr, betas, wd) + OneCycleLR(pct_start .2, div_factor 1000,
final_div_factor final_factor/1000, cosine annealing, stepped every batch) and the sqrt LR scaling rule).
"""

from __future__ import annotations

import math

import torch

from maestro_amd import hip


def scaled_lr(base_lr: float, batch_size: int, accumulate: int = 1, num_nodes: int = 1, num_devices: int = 1) -> float:
    """``lr = base_lr * sqrt(B * accum * nodes * devices / 3)`` (model.py:122-133; the /3 is historical)."""
    return base_lr * (batch_size * accumulate * num_nodes * num_devices / 3.0) ** 0.5


class OneCycle:
    """Value-for-value ``torch.optim.lr_scheduler.OneCycleLR`` (cos anneal, two phases, cycle_momentum=False)."""

    def __init__(self, max_lr: float, total_steps: int, pct_start: float = 0.2, div_factor: float = 1000.0,
                 final_div_factor: float = 1e4) -> None:
        self.max_lr, self.total = max_lr, total_steps
        self.initial = max_lr / div_factor
        self.min_lr = self.initial / final_div_factor
        self.end1 = float(pct_start * total_steps) - 1
        self.end2 = total_steps - 1

    @staticmethod
    def _cos(start, end, pct):
        return end + (start - end) / 2.0 * (math.cos(math.pi * pct) + 1)

    def lr(self, step_num: int) -> float:
        if step_num <= self.end1:
            return self._cos(self.initial, self.max_lr, step_num / self.end1 if self.end1 > 0 else 1.0)
        return self._cos(self.max_lr, self.min_lr, (step_num - self.end1) / (self.end2 - self.end1))


def resolve_grad_guard(max_grad_norm: float | None = None, skip_nonfinite: bool | None = None) -> tuple[float | None, bool]:
    """The gradient-guard switches of the loops: explicit values win; None reads ``MAESTRO_MAX_GRAD_NORM`` (a positive float;
    unset / empty / 0 = no clipping) and ``MAESTRO_SKIP_NONFINITE`` ("1" = on).  Returns ``(max_norm or None, skip)``: a guard
    exists iff either is set.  A negative or non-finite norm is a ``ValueError``."""
    import os
    if max_grad_norm is None:
        text = os.environ.get("MAESTRO_MAX_GRAD_NORM", "").strip()
        max_grad_norm = float(text) if text else None
    if skip_nonfinite is None:
        skip_nonfinite = os.environ.get("MAESTRO_SKIP_NONFINITE", "0") == "1"
    if max_grad_norm is not None:
        max_grad_norm = float(max_grad_norm)
        if not math.isfinite(max_grad_norm) or max_grad_norm < 0:
            raise ValueError(f"max_grad_norm={max_grad_norm!r}: expected a finite number >= 0 (0 = no clipping)")
    return (max_grad_norm or None), bool(skip_nonfinite)


def refuse_guard_conflicts(guarded: bool, overlap_optimizer: bool = False, dtype: str | None = None,
                           exchange_mode: str = "all_reduce") -> None:
    """What a gradient guard excludes, as ``ValueError``s raised before anything is built."""
    if not guarded:
        return
    if overlap_optimizer:
        raise ValueError("a gradient guard (max_grad_norm / skip_nonfinite) excludes overlap_optimizer: the update waits for the "
                         "norm of the whole gradient")
    if dtype == "fp8":
        raise ValueError("a gradient guard (max_grad_norm / skip_nonfinite) is not available with dtype='fp8': mh_adamw_fp8 has "
                         "no device-scalar form")
    if exchange_mode == "rs_ag":
        raise ValueError("a gradient guard (max_grad_norm / skip_nonfinite) excludes exchange_mode='rs_ag': a rank holds only "
                         "its chunks of the reduced gradient there")


def resolve_lw_decay(lw_decay: float | None = None) -> float | None:
    """The layer-wise learning-rate decay of the finetune loop: an explicit value wins; None reads ``MAESTRO_LW_DECAY`` (unset or
    empty = off).  A float in ``(0, 1]`` is accepted, anything else is a ``ValueError``."""
    import os
    if lw_decay is None:
        text = os.environ.get("MAESTRO_LW_DECAY", "").strip()
        if not text:
            return None
        try:
            lw_decay = float(text)
        except ValueError:
            raise ValueError(f"MAESTRO_LW_DECAY={text!r}: lw_decay must be a number in (0, 1]") from None
    if isinstance(lw_decay, bool) or not isinstance(lw_decay, (int, float)) or not 0.0 < float(lw_decay) <= 1.0:
        raise ValueError(f"lw_decay={lw_decay!r}: expected a number in (0, 1] (None = off)")
    return float(lw_decay)


def refuse_group_conflicts(grouped: bool, dtype: str | None = None, sharded: bool = False, phase: str | None = None,
                           lw_decay: float | None = None) -> None:
    """What AdamW parameter groups (``lw_decay`` / ``no_decay_1d``) exclude, as ``ValueError``s raised before anything is
    launched."""
    if phase == "probe" and lw_decay is not None:
        raise ValueError("lw_decay is a finetune option: in phase='probe' only the heads train (all at the base rate), and the "
                         "reference's trainer gives probe no lw_decay")
    if not grouped:
        return
    if dtype == "fp8":
        raise ValueError("AdamW parameter groups (lw_decay / no_decay_1d) are not available with dtype='fp8': mh_adamw_fp8 has no "
                         "grouped form")
    if sharded:
        raise ValueError("AdamW parameter groups (lw_decay / no_decay_1d) exclude step_sharded (exchange_mode='rs_ag'): the chunks "
                         "of a bucket are not 64-element aligned by construction")


def resolve_moment_dtype(moment_dtype: str | None = None) -> str:
    """How the loops' AdamW holds its two moments: an explicit value wins; None reads ``MAESTRO_MOMENT_DTYPE`` (unset, empty or
    "fp32" = off).  Returns "fp32" or "bf16"; anything else is a ``ValueError``."""
    import os
    if moment_dtype is None:
        moment_dtype = os.environ.get("MAESTRO_MOMENT_DTYPE", "").strip() or "fp32"
    if moment_dtype not in ("fp32", "bf16"):
        raise ValueError(f"moment_dtype={moment_dtype!r}: expected 'fp32' or 'bf16'")
    return moment_dtype


def refuse_moment_conflicts(bf16_moments: bool, overlap_optimizer: bool = False, dtype: str | None = None,
                            exchange_mode: str = "all_reduce") -> None:
    """What bf16 moments (``moment_dtype="bf16"``) exclude, as ``ValueError``s raised before anything is built."""
    if not bf16_moments:
        return
    if dtype == "fp8":
        raise ValueError("moment_dtype='bf16' is not available with dtype='fp8': mh_adamw_fp8 has no bf16-moment form")
    if exchange_mode == "rs_ag":
        raise ValueError("moment_dtype='bf16' excludes exchange_mode='rs_ag': the sharded moments and gather_state are fp32")
    if overlap_optimizer:
        raise ValueError("moment_dtype='bf16' excludes overlap_optimizer: the per-layer deferred stages launch the fp32-moment update")


def layer_scale(name: str, depth: int, inter_depth: int, lw_decay: float | None) -> float:
    """The learning-rate scale of the supervised engine's parameter ``name`` under layer-wise decay ``r = lw_decay`` -- the
    baselines' rule (``maestro/baselines/dinov2.py:312-373``: patch_embed ``r^(depth + 1)``, block ``i`` ``r^(depth - i)``, heads
    and the last LayerNorm 1) restated for this model, whose encoder is ``d = depth - inter_depth`` blocks per modality / group
    followed by ``inter_depth`` joint blocks (``D = depth`` in total):

        patch_embed.*                    r^(D + 1)
        encoder.<name>.layers.<i>.*      r^(D - i)
        encoder_inter.layers.<j>.*       r^(D - (d + j))
        encoder.<name>.norm.*            r^(D - d)     the scale of the block that consumes it (1 without joint blocks)
        encoder_inter.norm.*             1
        heads.*                          1

    Python floats; None = no decay (1 everywhere).  A name outside this list is a ``ValueError``."""
    if lw_decay is None:
        return 1.0
    r, D, d = float(lw_decay), int(depth), int(depth) - int(inter_depth)  # noqa: N806
    part = name.split(".")
    if part[0] == "heads":
        return 1.0
    if part[0] == "patch_embed":
        return r ** (D + 1)
    if part[0] == "encoder" and len(part) > 3 and part[2] == "layers":
        return r ** (D - int(part[3]))
    if part[0] == "encoder" and len(part) > 2 and part[2] == "norm":
        return r ** (D - d)
    if part[0] == "encoder_inter" and len(part) > 2 and part[1] == "layers":
        return r ** (D - (d + int(part[2])))
    if part[0] == "encoder_inter" and part[1] == "norm":
        return 1.0
    raise ValueError(f"layer_scale: {name!r} is no parameter of the probe / finetune model")


def layer_group_name(name: str) -> str:
    """The parameter group ``name`` belongs to on the ``torch.optim`` surface: one per patch embed, encoder block, stack norm, and
    one for all heads (the baselines' ``patch_embed.<mod>`` / ``encoder.<mod>.<i>`` / ``heads``)."""
    part = name.split(".")
    if part[0] == "heads":
        return "heads"
    if part[0] == "patch_embed":
        return ".".join(part[:2])
    if part[0] == "encoder":
        return f"encoder.{part[1]}.{part[3]}" if part[2] == "layers" else f"encoder.{part[1]}.norm"
    if part[0] == "encoder_inter":
        return f"encoder_inter.{part[2]}" if part[1] == "layers" else "encoder_inter.norm"
    raise ValueError(f"layer_group_name: {name!r} is no parameter of the probe / finetune model")


def layer_groups(engine, lw_decay: float | None, weight_decay: float, no_decay_1d: bool = False):
    """``hip.ParamGroups`` over the engine's flat layout by the layer rule (:func:`layer_scale`), from ``engine.store``'s names and
    offsets: one span per parameter (its 64-element padding included), scale from its name, weight decay ``weight_decay`` -- or 0
    for every parameter with ``ndim <= 1`` (biases, LayerNorm / GroupNorm gains, 1-d head parameters) when ``no_decay_1d``.
    ``lw_decay=None`` with ``no_decay_1d=False`` returns None: no groups, the ungrouped launches."""
    if lw_decay is None and not no_decay_1d:
        return None
    st, model = engine.store, engine.model
    offs = [st.offset[id(p)] for p in st.params] + [st.total]
    spans = []
    for k, (name, p) in enumerate(zip(st.names, st.params)):
        wd = 0.0 if (no_decay_1d and p.ndim <= 1) else float(weight_decay)
        spans.append((offs[k], offs[k + 1], layer_scale(name, model.depth, model.inter_depth or 0, lw_decay), wd))
    return hip.ParamGroups(spans, st.flat.device)


class FusedAdamW:
    """One ``mh_adamw`` launch over all trainable parameters; also refreshes the bf16 weight shadows.

    ``guard`` (a ``hip.GradGuard`` over the trainable span, attribute or ``step`` argument; default None = exactly the launches
    above): the step becomes norm + finish + ONE ``mh_adamw_dev`` that reads its scalars -- clipping coefficient folded into the
    gradient scale, ``active`` = 0 on a skipped step -- from the guard; Adam's step count then lives in the guard's device
    state (``t`` property, ``state_dict``).

    ``groups`` (a ``hip.ParamGroups`` over the store's whole flat layout, e.g. :func:`layer_groups`; default None = exactly the
    launches above): every launch becomes its grouped form -- ``mh_adamw_groups`` on the slices where ``mh_adamw`` ran,
    ``mh_adamw_groups_dev`` under a guard -- with the map offset to the slice; ``lr`` is then the BASE rate and ``weight_decay`` is
    not read (each group carries its own).  Excludes an fp8 plan and ``step_sharded`` (``refuse_group_conflicts``).  The
    ``state_dict`` layout is the ungrouped one.

    ``moment_dtype`` ("fp32", the default = exactly the launches above; "bf16"), ``moment_seed``: with "bf16" ``m`` / ``v`` are
    bf16 tensors (half the optimizer state, 22 instead of 30 bytes per parameter and step) and every launch of ``step`` -- plain,
    split, guarded, grouped -- takes its ``_bf16m`` form (include/maestro_hip.h) with ``elem_base`` = the slice's offset in
    the flat layout: the parameters move by the unrounded fp32 moments, which are then stored by stochastic rounding with words
    that are a function of ``(moment_seed, t, flat index)``, so a split step, a resumed run and every rank store the same bits.
    ``state_dict`` hands the moments out upcast to fp32 (exact); ``load_state_dict`` takes fp32 moments from either kind and
    rounds them to nearest-even into a bf16 optimizer (what a bf16 optimizer saved reloads bit for bit).  Excludes an fp8 plan,
    ``step_sharded`` and the deferred per-layer stages (``refuse_moment_conflicts``)."""

    def __init__(self, engine, lr: float, betas=(0.9, 0.99), eps: float = 1e-8, weight_decay: float = 0.01, groups=None,
                 moment_dtype: str = "fp32", moment_seed: int = 0) -> None:
        import torch

        if moment_dtype not in ("fp32", "bf16"):
            raise ValueError(f"FusedAdamW: moment_dtype={moment_dtype!r}: expected 'fp32' or 'bf16'")
        self.engine, self.lr, self.betas, self.eps, self.wd = engine, lr, betas, eps, weight_decay
        self.moment_dtype, self.moment_seed = moment_dtype, int(moment_seed) & 0xFFFFFFFFFFFFFFFF
        st = engine.store
        if groups is not None and groups.total != st.total:
            raise ValueError(f"FusedAdamW: parameter groups over {groups.total} elements, flat layout of {st.total}")
        self.groups = groups
        # the engine's trainable slice of the flat buffer (probe phase: the heads only -- frozen parameters must not even
        # see weight decay, as torch.optim.AdamW skips parameters without a gradient)
        self.lo, self.hi = getattr(engine, "trainable_span", (0, st.total))
        self.m = torch.zeros(self.hi - self.lo, dtype=torch.bfloat16 if self.bf16_moments else st.flat.dtype, device=st.flat.device)
        self.v = torch.zeros_like(self.m)
        self.t = 0
        self.guard = None

    @property
    def bf16_moments(self) -> bool:
        return self.moment_dtype == "bf16"

    def _refuse_moment_conflicts(self) -> None:
        refuse_moment_conflicts(self.bf16_moments, dtype="fp8" if getattr(self.engine, "fp8", None) is not None else None)

    def _update(self, a: int, b: int, lr: float | None = None, grad_scale: float | None = None, *, guard=None, fp8=None) -> None:
        """The one launch on ``[a, b)`` of the flat layout, in the form the optimizer's state selects: grouped with ``self.groups``
        (the map offset to ``a``), bf16 moments (``elem_base = a``), the scalars ``(lr, self.t, grad_scale)`` -- or, under
        ``guard``, its device scalars ``hyper`` and Adam's ``t`` from its device counter, written by its finish launch --, and with
        ``fp8`` (the engine's fp8 plan, when it fuses) ``mh_adamw_fp8``, which refreshes the e4m3 shadows as well."""
        st, gr, lo = self.engine.store, self.groups, self.lo
        ops = (st.flat[a:b], st.grad[a:b], self.m[a - lo: b - lo], self.v[a - lo: b - lo], st.half[a:b])
        if fp8 is not None:
            return hip.adamw_fp8(*ops, fp8.w8_flat[a:b], fp8.slot_map[a // 64:], fp8.wsc.scale, fp8.wsc.amax, b - a, lr, self.betas[0],
                                 self.betas[1], self.eps, self.wd, self.t, grad_scale)
        hip._adamw(*ops, b - a, self.betas[0], self.betas[1], self.eps,
                   wd=self.wd if gr is None else None, groups=None if gr is None else (gr.map_at(a), gr.lr_scale, gr.wd),
                   scalars=(lr, self.t, grad_scale) if guard is None else None, hyper=None if guard is None else guard.hyper,
                   draws=(a, self.moment_seed) if self.bf16_moments else None,
                   step_dev=guard.t_dev if guard is not None and self.bf16_moments else None)

    def _step_guarded(self, guard, lr: float, grad_scale: float, between) -> None:
        st, lo, hi = self.engine.store, self.lo, self.hi
        if getattr(self.engine, "fp8", None) is not None:
            raise ValueError("FusedAdamW.step: a gradient guard is not available with dtype='fp8' (mh_adamw_fp8 has no "
                             "device-scalar form)")
        if guard.n != hi - lo:
            raise hip.HipExtensionError(f"FusedAdamW.step: guard over {guard.n} elements, trainable span of {hi - lo}")
        self.guard = guard
        if between is not None:
            between()
        guard.launch(st.grad[lo:hi], lr, self.betas[0], self.betas[1], grad_scale)
        self._update(lo, hi, guard=guard)
        st.mark_synced()
        self.engine._pack_conv_weights()

    def step(self, lr: float | None = None, grad_scale: float = 1.0, split: int = 0, between=None, guard=None) -> None:
        """``split`` / ``between``: update ``[split, hi)`` first, call ``between()`` (e.g. wait for the last gradient bucket),
        then update ``[lo, split)`` -- the data-parallel loop hides its exposed all-reduce under the first launch.

        ``guard`` (default: ``self.guard``): ``between()`` runs FIRST -- the norm needs the whole reduced gradient, so the
        tail-bucket overlap is given up --, then ``guard.launch`` over ``grad[lo:hi]`` and one ``mh_adamw_dev`` over ``[lo, hi)``
        with ``guard.hyper``.  The gradient buffer is NOT rewritten: the clipping coefficient rides in ``hyper[3]`` next to
        ``grad_scale``; on a skipped step (``hyper[4] == 0``) the kernel returns before it touches memory, and the shadows and
        packed weights that are rebuilt afterwards are rebuilt from unchanged masters.  ``ValueError`` with an fp8 plan."""
        import os
        import torch
        refuse_group_conflicts(self.groups is not None, dtype="fp8" if getattr(self.engine, "fp8", None) is not None else None)
        self._refuse_moment_conflicts()
        roctx = os.environ.get("MAESTRO_ROCTX", "0") == "1"
        if roctx:
            torch.cuda.nvtx.range_push("maestro:adamw")
        guard = self.guard if guard is None else guard
        if guard is not None:
            try:
                return self._step_guarded(guard, self.lr if lr is None else lr, grad_scale, between)
            finally:
                if roctx:
                    torch.cuda.nvtx.range_pop()
        st = self.engine.store
        self.t += 1
        lr = self.lr if lr is None else lr
        lo, hi = self.lo, self.hi
        plan = getattr(self.engine, "fp8", None)
        fused8 = plan is not None and plan.before_fused_adamw()     # e4m3 weight shadows refreshed by the update itself
        split = min(max(split, lo), hi) // 64 * 64
        for a, b in ((split, hi), (lo, split)):
            if a == lo and between is not None:
                between()
            if b > a:
                fused8 = fused8 and a % 64 == 0        # one plain launch: the e4m3 shadows are then cast from the masters afterwards
                self._update(a, b, lr, grad_scale, fp8=plan if fused8 else None)
        st.mark_synced()               # bf16 shadows were refreshed by the kernel itself
        if plan is not None:
            self.engine._pack_conv_weights(fp8_done=fused8)  # K-padded patch-embed weights (+ e4m3 shadows unless fused above)
        else:
            self.engine._pack_conv_weights()                 # patch-embed weights live in a K-padded bf16 layout
        if roctx:
            torch.cuda.nvtx.range_pop()

    def step_sharded(self, sync, lr: float | None = None, grad_scale: float = 1.0) -> None:
        """The update under ``GradSync(mode="rs_ag")`` (after ``sync.finish()``): this rank holds the reduced gradient only on its
        chunk of every bucket, updates exactly those chunks -- 1 / world of AdamW's 30 bytes per parameter --, then the updated fp32
        masters are all-gathered in place and the bf16 shadows of the chunks that arrived from other ranks are re-cast locally.
        The moments of a chunk live on its owner only (``gather_state`` assembles them for a checkpoint).  Parameters after the
        step are bit-identical on every rank, and equal to the all-reduce plan's up to the summation order inside the collective."""
        st = self.engine.store
        refuse_group_conflicts(self.groups is not None, sharded=True)
        refuse_moment_conflicts(self.bf16_moments, exchange_mode="rs_ag")
        if getattr(self.engine, "fp8", None) is not None:
            raise hip.HipExtensionError("FusedAdamW.step_sharded: not available with dtype='fp8' (the e4m3 shadows of chunks owned "
                                        "by other ranks would need their scales: use the all-reduce plan)")
        owned = sync.owned()
        if getattr(self, "_owned", None) not in (None, owned):
            raise hip.HipExtensionError("FusedAdamW.step_sharded: the bucket plan changed between steps -- the moments of a chunk "
                                        "would move to another rank")
        self._owned, self._sharded_world, self._gathered = owned, sync.world, False
        self.t += 1
        lr = self.lr if lr is None else lr
        lo, hi = self.lo, self.hi
        for _, _, a, b in owned:
            a, b = max(a, lo), min(b, hi)
            if b > a:
                self._update(a, b, lr, grad_scale)
        for a, b in sync.gather_params(st.flat):
            a, b = max(a, lo), min(b, hi)
            if b > a:
                hip.cast_bf16(st.flat[a:b], st.half[a:b], b - a)
        st.mark_synced()
        self.engine._pack_conv_weights()

    def gather_state(self, sync, base: int = 0) -> None:
        """Under ``rs_ag``: assemble the full moments on every rank (a COLLECTIVE: all-gather of the owned chunks; for checkpoints).
        ``base``: offset of ``sync``'s buffer inside the store's flat layout (``SupervisedLoop`` hands ``GradSync`` the slice
        ``grad_all[lo:]``); the moments cover ``[self.lo, self.hi)`` of that layout, wherever the span starts."""
        for buf in (self.m, self.v):
            sync.gather_pieces(buf, shift=self.lo - base)
        self._gathered = True

    def state_dict(self) -> dict:
        """The optimizer state for a checkpoint.  Under ``exchange_mode="rs_ag"`` a rank holds real moments only on its own chunks
        (zeros elsewhere): saving that as it stands would silently drop (world - 1) / world of the Adam state, so an ungathered
        sharded state is REFUSED here -- call ``gather_state(sync)`` on every rank first (``PretrainLoop.state_dict()`` does)."""
        sharded = getattr(self, "_owned", None) is not None and getattr(self, "_sharded_world", 1) > 1
        if sharded and not getattr(self, "_gathered", False):
            raise hip.HipExtensionError("FusedAdamW.state_dict: the moments are sharded over the ranks (exchange_mode='rs_ag') and have "
                                        "not been gathered since the last step: call gather_state(sync) on EVERY rank first "
                                        "(PretrainLoop.state_dict() does)")
        # Sharded: hand out COPIES.  The live tensors stop being a whole state at the next step_sharded (owned chunks advance, the
        # chunks gathered from other ranks go stale), and a deferred / asynchronous checkpoint writer holding them would save a
        # mixed-step Adam state without any error.  ("t" stamps the step the copies belong to.)
        m, v = (self.m.clone(), self.v.clone()) if sharded else (self.m, self.v)
        if self.bf16_moments:          # bf16 -> fp32 is exact: a checkpoint holds fp32 moments whichever optimizer wrote it
            m, v = m.float(), v.float()
        if self.guard is not None:     # Adam's step count lives in the guard's device state (a skipped step does not advance it)
            self.t = self.guard.state_dict()["t"]
        sd = {"m": m, "v": v, "t": self.t, "lr": self.lr, "span": (self.lo, self.hi),
              "exchange_mode": "rs_ag" if sharded else "all_reduce", "world": getattr(self, "_sharded_world", 1)}
        if self.bf16_moments:          # (an fp32-moment optimizer's state keeps the keys it always had)
            sd.update(moment_dtype=self.moment_dtype, moment_seed=self.moment_seed)
        return sd

    def load_state_dict(self, sd: dict) -> None:
        if "span" in sd and tuple(sd["span"]) != (self.lo, self.hi):
            raise hip.HipExtensionError(f"FusedAdamW.load_state_dict: state of span {tuple(sd['span'])}, optimizer of span {(self.lo, self.hi)}")
        self.m.copy_(sd["m"])          # fp32 moments into a bf16 optimizer: copy_ rounds to nearest-even (exact for what a bf16
        self.v.copy_(sd["v"])          # optimizer saved); the rounding words follow THIS optimizer's moment_seed
        self.t, self.lr = sd["t"], sd["lr"]
        if self.guard is not None:
            self.guard.load_state_dict({"t": self.t})
        self._gathered = True      # full moments on this rank: under rs_ag the next step simply keeps using its own chunks


def clip_grad_norm_(engine, max_norm: float) -> torch.Tensor:
    """``torch.nn.utils.clip_grad_norm_`` (L2) over the engine's trainable span of the flat gradient buffer, without torch's
    multi-tensor norm over several hundred views: the two guard launches, then ``mh_scale_dev`` of the span by the device
    coefficient ``min(1, max_norm / (norm + 1e-6))``.  Returns the total norm as a 0-dim DEVICE tensor (no host read).  This is
    the one place where the gradient buffer itself is scaled: ``torch.optim`` semantics (the optimizer reads ``p.grad``) demand
    it; the built-in loops fold the coefficient into AdamW's gradient scale instead.  A non-finite norm leaves the gradients as
    they are (coefficient 1)."""
    st = engine.store
    lo, hi = getattr(engine, "trainable_span", (0, st.total))
    guard = getattr(engine, "_clip_guard", None)
    if guard is None or guard.n != hi - lo:
        guard = engine._clip_guard = hip.GradGuard(hi - lo, st.grad.device, skip_nonfinite=False)
    guard.max_norm = float(max_norm)
    guard.launch(st.grad[lo:hi], 0.0, 0.0, 0.0, 1.0)
    hip.scale_dev(st.grad[lo:hi], hi - lo, guard.coef)
    return guard.norm.reshape(())


class EngineAdamW(torch.optim.AdamW):
    """The optimizer ``SSLModule.configure_optimizers`` hands to Lightning: a ``torch.optim.AdamW`` (same constructor, same
    ``param_groups`` for ``OneCycleLR``, same ``state_dict`` layout -- ``state[p] = {step, exp_avg, exp_avg_sq}`` -- so optimizer
    states interchange with the reference's checkpoints, ``maestro/train/model.py:135-140``) whose ``step()`` is ONE ``mh_adamw``
    launch over the engine's flat buffer instead of torch's multi-tensor loop: the moments of all parameters live in two flat
    buffers in the engine's layout (``state[p]`` holds VIEWS of them), the bf16 weight shadows are refreshed by the same pass.
    Measured on C3, B = 32, Lightning-style step: torch's foreach AdamW 15 ms of host time and 1479 tiles/s -> see
    ``profiles/README.md``.

    ``engine_of()`` returns the engine that owns the parameters right now (or None before the first ``training_step``).  The
    fused launch is used when the optimizer has ONE parameter group (the reference's case) with plain AdamW options and covers
    every parameter of the engine's trainable span; otherwise ``torch.optim.AdamW.step`` runs unchanged.

    SEVERAL groups (layer-wise lr decay, ``maestro/train/baseline.py:110-131``; no weight decay on 1-d parameters) stay fused as
    one ``mh_adamw_groups`` launch when they agree in betas, eps and flags and every parameter of the span is in one of them: the
    last group's lr is the kernel's scalar, every group's ``lr / lr_last`` and ``weight_decay`` go into a ``hip.ParamGroups``
    when the engine is bound (``_groups_expressible`` re-checks the ratios every step; when they no longer hold torch's step
    runs, as for anything not eligible)."""

    def __init__(self, params, engine_of, **kw) -> None:
        super().__init__(params, **kw)
        self._engine_of, self._bound, self._fused, self._scales = engine_of, None, None, None

    def load_state_dict(self, state_dict) -> None:
        super().load_state_dict(state_dict)
        self._bound = None            # the loaded moments are fresh tensors: adopt them into the flat buffers at the next step

    def state_dict(self) -> dict:
        """torch's layout.  Internally every parameter's ``step`` is ONE shared tensor (the fused launch has one step count);
        a checkpoint must not carry that sharing -- ``torch.save`` preserves tensor identity, and torch's multi-tensor AdamW
        increments every parameter's ``step`` tensor: a shared one would advance by the number of parameters per step in the
        optimizer that loads it -- so each parameter gets its own copy here."""
        sd = super().state_dict()
        sd["state"] = {k: {n: (t.clone() if n == "step" and isinstance(t, torch.Tensor) else t) for n, t in v.items()}
                       for k, v in sd["state"].items()}
        return sd

    def _eligible(self, eng) -> bool:
        groups = self.param_groups
        if eng is None:
            return False
        for g in groups:
            if g.get("amsgrad") or g.get("maximize") or g.get("capturable") or g.get("differentiable") or isinstance(g["lr"], torch.Tensor):
                return False
        if len(groups) > 1 and not self._groups_expressible(eng):
            return False
        mine = {id(p) for g in groups for p in g["params"]}
        st = eng.store
        lo, hi = getattr(eng, "trainable_span", (0, st.total))
        span = [p for p in st.params if lo <= st.offset[id(p)] < hi]
        if not all(id(p) in mine for p in span) or getattr(st, "fresh", True):
            return False
        # ... and the reverse: a parameter of a group OUTSIDE the span that carries a gradient (stale from an earlier phase with
        # set_to_none=False, or a module parameter the engine does not own) would be updated and decayed by torch.optim.AdamW.step
        # but not by the fused launch -- behaviour must not depend on the path taken, so torch's step runs in that case
        inside = {id(p) for p in span}
        if any(p.grad is not None for g in groups for p in g["params"] if id(p) not in inside):
            return False
        # every gradient of the span must BE the flat buffer's slice (the autograd bridge attaches them)
        return all(p.grad is not None and p.grad.data_ptr() == st.g(p).data_ptr() for p in span)

    def _groups_expressible(self, eng) -> bool:
        """Several groups as ONE base rate and constant per-group scales: they agree in betas and eps, the LAST group's lr is the
        scalar handed to the kernel, and every other group's lr is that scalar times the scale captured when the groups were
        bound -- re-checked here on every step, a few dozen floats on the host (``1e-6`` relative: the ratio is exact in real
        arithmetic, a scheduler that scales every ``max_lr`` by one factor keeps it up to float roundoff)."""
        groups = self.param_groups
        last = groups[-1]
        if any(g["betas"] != last["betas"] or g["eps"] != last["eps"] for g in groups):
            return False
        lr_last = float(last["lr"])
        if not (math.isfinite(lr_last) and lr_last > 0.0) or getattr(eng, "fp8", None) is not None:
            return False
        if len({(float(g["lr"]), float(g["weight_decay"])) for g in groups}) > hip.GROUP_TABLE:
            return False
        if self._bound is eng and self._scales is not None:
            if len(self._scales) != len(groups):
                return False
            for g, (scale, wd) in zip(groups, self._scales):
                if abs(float(g["lr"]) - lr_last * scale) > 1e-6 * lr_last or float(g["weight_decay"]) != wd:
                    return False
        return True

    def _bind(self, eng) -> None:
        """Moments into the engine's layout (adopting whatever per-parameter state exists: a loaded checkpoint, steps done by
        torch's implementation, a previous engine of another batch size) and ``state[p]`` re-pointed at views of them."""
        g = self.param_groups[-1]
        st = eng.store
        groups, self._scales = None, None
        if len(self.param_groups) > 1:      # scale_g = lr_g / lr_last, captured once; parameters of no group are never touched
            lr_last = float(g["lr"])
            self._scales = [(float(q["lr"]) / lr_last, float(q["weight_decay"])) for q in self.param_groups]
            pair = {id(p): self._scales[k] for k, q in enumerate(self.param_groups) for p in q["params"]}
            offs = [st.offset[id(p)] for p in st.params] + [st.total]
            groups = hip.ParamGroups([(offs[k], offs[k + 1], *pair.get(id(p), (0.0, 0.0))) for k, p in enumerate(st.params)],
                                     st.flat.device)
        fused = FusedAdamW(eng, g["lr"], betas=g["betas"], eps=g["eps"], weight_decay=g["weight_decay"], groups=groups)
        lo, hi = fused.lo, fused.hi
        t = 0
        with torch.no_grad():
            for p in st.params:
                o = st.offset[id(p)]
                if not lo <= o < hi:
                    continue
                mv = fused.m[o - lo: o - lo + p.numel()].view(p.shape)
                vv = fused.v[o - lo: o - lo + p.numel()].view(p.shape)
                old = self.state.get(p)
                if old and "exp_avg" in old:
                    mv.copy_(old["exp_avg"])
                    vv.copy_(old["exp_avg_sq"])
                    t = max(t, int(float(old["step"])))
                self.state[p] = {"exp_avg": mv, "exp_avg_sq": vv}
            self._step = torch.tensor(float(t))      # ONE step counter shared by every parameter's state (torch: one each)
            for p in st.params:
                if p in self.state and "step" not in self.state[p]:
                    self.state[p]["step"] = self._step
        fused.t = t
        self._fused, self._bound = fused, eng

    def step(self, closure=None):
        loss = None
        if closure is not None:        # Lightning's automatic optimization runs training_step + backward in here
            with torch.enable_grad():
                loss = closure()
        eng = self._engine_of()
        if not self._eligible(eng):
            if self._bound is not None:     # back to torch's implementation: it advances every parameter's OWN step tensor
                for st in self.state.values():
                    if "step" in st:
                        st["step"] = st["step"].clone()
                self._bound = None          # (the moments stay where they are: views of the flat buffers are ordinary tensors)
            super().step()
            return loss
        if self._bound is not eng:
            self._bind(eng)
        g, f = self.param_groups[-1], self._fused      # (with several groups: the base rate; f.wd is not read then)
        f.betas, f.eps, f.wd = g["betas"], g["eps"], g["weight_decay"]
        f.step(lr=float(g["lr"]))
        self._step.fill_(float(f.t))
        return loss
