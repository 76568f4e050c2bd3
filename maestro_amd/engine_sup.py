"""Probe / finetune step engine: unmasked encoders + heads + ``loss_pred`` on the HIP kernels.

Reference path: ``BaseMIM.forward`` with ``ssl_phase in ("probe", "finetune")`` (``maestro/ssl/mim.py:473-505``):
embed -> encodings -> per-group encoders (+ final LN) -> joint encoder (+ final LN) on the FULL sequences ->
``compute_logits`` (``mim.py:343-394``: token grids bilinearly resized onto the reference grid and stacked on the date
axis for raster targets, all tokens for classification targets) -> heads (``maestro/layers/head.py``) ->
``compute_loss_pred`` (``maestro/train/base.py:98-151``).  ``probe`` detaches the encoder features (head.py:17-25): only the
head parameters receive gradients and the encoder backward is skipped; ``finetune`` runs the whole backward.

Buffers are static (allocated once for a batch size), the forward / backward launch sequences are captured into hipGraphs
on their second run like the pretrain engine's, groups run on parallel HIP streams.  No CPU fallback.
"""

from __future__ import annotations

import math
import os
from typing import NamedTuple

import torch

from maestro_amd import hip
from maestro_amd.engine import BF16, F32, I32, EngineBase, ParamStore, Stack


def ordered_parameters(m):
    """``(ordered, head_params)``: the named parameters of the probe / finetune model in the order of the flat store -- patch
    embeds, per-modality / per-group encoders, the joint encoder, heads last -- and the heads' entries alone.  The names are
    those of ``model.named_parameters()``; the layer rule of ``train/optim.py`` reads them."""
    ordered = []
    for name in m.patch_embed:
        ordered += [(f"patch_embed.{name}.{k}", p) for k, p in m.patch_embed[name].named_parameters()]
    for name in m.encoder:
        ordered += [(f"encoder.{name}.{k}", p) for k, p in m.encoder[name].named_parameters()]
    if m.encoder_inter is not None:
        ordered += [(f"encoder_inter.{k}", p) for k, p in m.encoder_inter.named_parameters()]
    head_params = [(f"heads.{t}.{k}", p) for t in m.heads for k, p in m.heads[t].named_parameters()]
    return ordered + head_params, head_params


class Prediction(NamedTuple):
    """One target's prediction (``SupervisedEngine.predict``): device tensors, engine-owned -- valid until the next ``predict``."""
    cls: torch.Tensor
    conf: torch.Tensor
    probs: torch.Tensor | None


class Features(NamedTuple):
    """Encoder features (``SupervisedEngine.encode``): device tensors, engine-owned -- valid until the next ``encode``.  ``bf16`` is
    the round-to-nearest-even copy of ``f32``, the operand of ``hip.knn_topk``."""
    f32: torch.Tensor
    bf16: torch.Tensor


FEATURE_LEVELS = ("sample", "grid")


def check_encode_args(level, normalize) -> None:
    """The argument checks of ``SupervisedEngine.encode``, before any launch."""
    if level not in FEATURE_LEVELS:
        raise ValueError(f"level={level!r}: \"sample\" (one feature per batch element) or \"grid\" (one per cell of the reference grid)")
    if not isinstance(normalize, bool):
        raise ValueError(f"normalize={normalize!r}: True or False")


def parse_views(views) -> tuple:
    """``views`` of ``SupervisedEngine.predict`` as a tuple of dihedral flag bytes: a non-empty sequence of distinct values 0..7
    (bit 0 flips the rows, bit 1 the columns, bit 2 then swaps the axes: ``dataset.py:224-257``), or ``"d4"`` for all eight."""
    if isinstance(views, str):
        if views != "d4":
            raise ValueError(f"views={views!r}: a sequence of dihedral flags 0..7 or \"d4\"")
        return tuple(range(8))
    try:
        out = tuple(views)
    except TypeError:
        raise ValueError(f"views={views!r}: a sequence of dihedral flags 0..7 or \"d4\"") from None
    if not out or any(isinstance(v, bool) or not isinstance(v, int) or not 0 <= v <= 7 for v in out) or len(set(out)) != len(out):
        raise ValueError(f"views={views!r}: a non-empty sequence of distinct dihedral flags 0..7 or \"d4\"")
    return out


BLENDS = ("flat", "linear")


def scene_unit(sizes) -> int:
    """Side of the prediction window in UNITS: the greatest common divisor of the model's raster sizes -- every input's
    ``image_size`` and every segment target's ``G * P`` -- so that a raster of size ``S`` has ``S / W`` whole pixels per unit
    (the reference's ``size_gcd`` / ``crop_gcd`` rule, ``conf/dataset/utils.py:99-109``, stated on the model's own sizes)."""
    return math.gcd(*[int(s) for s in sizes])


def check_scene(scene: dict, rasters: dict, W: int, stride=None, blend: str = "linear", device=None) -> tuple:  # noqa: N803
    """The argument checks of ``SupervisedEngine.predict_scene``, all before any launch: ``rasters`` is ``{name: (image_size, dates,
    channels)}``, ``device`` the engine's GPU (None: any GPU).  Returns ``(N, Hu, Wu, stride)``: the number of scenes, their
    extent in units and the stride in units."""
    extent = None
    for src, (S, D, C) in rasters.items():  # noqa: N806
        img, dates = scene.get(src), scene.get(f"{src}_dates")
        if not isinstance(img, torch.Tensor) or img.dtype != F32 or not img.is_contiguous():
            raise ValueError(f"scene[{src!r}] must be a contiguous float32 GPU tensor [N, {D}, {C}, Hu * q, Wu * q]")
        q = S // W
        if img.dim() != 5 or tuple(img.shape[1:3]) != (D, C) or img.shape[3] % q or img.shape[4] % q:
            raise ValueError(f"scene[{src!r}] is {tuple(img.shape)}: expected [N, {D}, {C}, Hu * {q}, Wu * {q}] ({q} pixels per unit)")
        here = (img.shape[0], img.shape[3] // q, img.shape[4] // q)
        if extent is not None and here != extent[1]:
            raise ValueError(f"scene[{src!r}] covers {here[0]} scenes of {here[1]} x {here[2]} units, scene[{extent[0]!r}] "
                             f"{extent[1][0]} of {extent[1][1]} x {extent[1][2]}: the extents of the modalities disagree")
        extent = extent or (src, here)
        if not isinstance(dates, torch.Tensor) or dates.dtype != torch.int16 or not dates.is_contiguous() \
                or tuple(dates.shape) != (here[0], D, 3):
            raise ValueError(f"scene['{src}_dates'] must be a contiguous int16 tensor [{here[0]}, {D}, 3]")
    if extent is None:
        raise ValueError("the model has no input raster")
    N, Hu, Wu = extent[1]  # noqa: N806
    ref = scene.get("ref_date")
    if not isinstance(ref, torch.Tensor) or ref.dtype != torch.int16 or not ref.is_contiguous() or tuple(ref.shape) != (N, 1, 3):
        raise ValueError(f"scene['ref_date'] must be a contiguous int16 tensor [{N}, 1, 3]")     # (mh_date_features reads int16_t)
    if N < 1 or Hu < W or Wu < W:
        raise ValueError(f"a scene of {Hu} x {Wu} units is below one window of {W} x {W} units")
    stride = max(1, W // 2) if stride is None else stride
    if isinstance(stride, bool) or not isinstance(stride, int) or not 1 <= stride <= W:
        raise ValueError(f"stride={stride!r}: 1 ... {W} units (a larger stride would leave units uncovered)")
    if blend not in BLENDS:
        raise ValueError(f"blend={blend!r}: \"flat\" or \"linear\"")
    for k in [k for src in rasters for k in (src, f"{src}_dates")] + ["ref_date"]:
        if not scene[k].is_cuda:
            raise ValueError(f"scene[{k!r}] must be on the GPU; there is no CPU fallback")
        index = None if device is None else torch.device(device).index
        if device is not None and scene[k].device.index != (torch.cuda.current_device() if index is None else index):
            raise ValueError(f"scene[{k!r}] is on {scene[k].device}, the engine on {device}: the kernels read it by address")
    return N, Hu, Wu, stride


class SupervisedEngine(EngineBase):
    def __init__(self, model, batch_size: int, device, phase: str = "finetune", deterministic: bool = False) -> None:
        if phase not in ("probe", "finetune", "encode"):
            raise ValueError(f"Invalid ssl phase {phase}. Expected 'probe' or 'finetune'")
        if deterministic:
            raise ValueError("deterministic=True is not available for the probe / finetune step: the loss accumulators and the "
                             "head reductions of SupervisedEngine still use floating-point atomics (pretraining only)")
        device = torch.device(device)
        if device.type != "cuda":
            raise hip.HipExtensionError("SupervisedEngine needs a GPU device; there is no CPU fallback")
        hip.lib()
        m = self.model = model
        fold = m.fusion_mode in ("shared", "monotemp")   # dates folded into the batch (utils.py:26-37): Beff = B * dates
        if fold and m.encoder_inter is not None:
            raise NotImplementedError(
                f"Simultaneous encoding of all mods not yet compatible with fusion mode: {m.fusion_mode}.")  # model.py:65-67
        if not len(m.heads) and phase != "encode":     # ("encode" runs the encoders alone: no head is needed, none is built)
            raise ValueError("the dataset config selects no target (filter_targets): nothing to probe / finetune")
        self.B, self.phase, self.E = batch_size, phase, m.embed_dim
        self._init_runtime(device, len(m.group_specs) - 1)
        self.mods, self.groups = m.mod_specs, list(m.group_specs.values())
        for s in self.mods.values():
            s.Beff = batch_size * s.Dates if fold else batch_size
        for g in self.groups:
            g.Beff = g.mods[0].Beff
        # full-sequence geometry: group g occupies rows [goff, goff + Lb) of the JL tokens of one batch element, Lb = L
        # (or dates * L when the dates are folded: the [B * dates, L, E] sequences ARE [B, dates * L, E] in memory)
        self.goff, self.Lb, off = {}, {}, 0
        for g in self.groups:
            self.goff[g.name], self.Lb[g.name] = off, g.L * (g.Beff // batch_size)
            off += self.Lb[g.name]
        self.JL = off
        # ---- flat parameter store: encoder side first, heads last (probe trains the contiguous tail only)
        ordered, head_params = ordered_parameters(m)
        self.store = ParamStore(ordered, device)
        if phase == "encode":
            self.trainable_span = (self.store.total, self.store.total)      # nothing is trained
        else:
            lo, _ = self.store.span([p for _, p in head_params])
            self.trainable_span = (lo, self.store.total) if phase == "probe" else (0, self.store.total)
        m.enc_pos_encoding = m.enc_pos_encoding.to(device)
        self._alloc()
        self.store.refresh_half(force=True)
        self._pack_conv_weights()

    # ------------------------------------------------------------------------------------------ allocation
    def _alloc(self) -> None:
        m, dev, E, B = self.model, self.device, self.E, self.B  # noqa: N806
        e = lambda *s, dt=F32: torch.empty(*s, dtype=dt, device=dev)  # noqa: E731
        z = lambda *s, dt=F32: torch.zeros(*s, dtype=dt, device=dev)  # noqa: E731
        self.gb, self.enc = {}, {}
        self._alloc_embed()
        ws_rows = B * self.JL
        for g in self.groups:
            n_dates = sum(s.D for s in g.mods)
            self.enc[g.name] = Stack(self, m.encoder[g.model], g.Beff, g.L, f"sup.enc.{g.name}")
            self.gb[g.name] = dict(dates=z(g.Beff, n_dates, 8), n_dates=n_dates, mean_e=e(g.Beff * g.L), rstd_e=e(g.Beff * g.L))
        self.joint = Stack(self, m.encoder_inter, B, self.JL, "sup.joint") if m.encoder_inter is not None else None
        self.xenc, self.dxenc = e(B, self.JL, E), e(B, self.JL, E)        # encoded tokens (after the last final LN) and their gradient
        self.mean_j, self.rstd_j = e(B * self.JL), e(B * self.JL)
        self.loss_acc = z(1)
        # ---- heads
        ds = m.dataset
        self.hb = {}
        self.ref = None
        targets = {} if self.phase == "encode" else ds.targets      # "encode": encoders only, no head buffers
        seg = [t for t, c in targets.items() if c.type_target == "segment"]
        if seg:
            G = m.out_grid_size[ds.ref_input]  # noqa: N806
            TD = sum(s.Dates for s in self.mods.values())  # noqa: N806
            self.ref = dict(G=G, Lr=G * G, TD=TD, x=e(B, TD * G * G, E), dx=e(B, TD * G * G, E))
            ws_rows = max(ws_rows, B * TD * G * G)
        for t, c in targets.items():
            head = m.heads[t]
            attentive = hasattr(head, "reduce")
            if c.type_target == "segment":
                T, Lr, P, C = self.ref["TD"], self.ref["Lr"], head.patch_size, c.num_classes  # noqa: N806
                PPC = P * P * C  # noqa: N806
                PPCp = (PPC + 7) // 8 * 8     # GEMM operand width: padded copies of the conv weight / bias when PPC % 8  # noqa: N806
                hb = dict(kind="segment", T=T, Lr=Lr, P=P, C=C, PPC=PPC, PPCp=PPCp, logits=z(B * Lr, PPCp),
                          dlogits=z(B * Lr, PPCp, dt=BF16), hfc=e(B * Lr, E, dt=BF16), cnt=z(1, dt=I32))
                if PPCp != PPC:
                    hb.update(w16p=z(PPCp, E, dt=BF16), dWp=z(PPCp, E), biasp=z(PPCp), dbp=z(PPCp))
            else:
                T, Lr, C = self.JL, 1, c.num_classes  # noqa: N806
                hb = dict(kind=c.type_target, T=T, Lr=1, C=C, logits=e(B, C), dlogits=e(B, C), h=e(B, E), dh=e(B, E),
                          cnt=z(1, dt=I32))
            R = B * T * Lr  # noqa: N806
            hb.update(attentive=attentive, R=R, red=e(B * Lr, E), dred=e(B * Lr, E), missing=c.missing_val)
            if attentive:
                hb.update(mean_n=e(R), rstd_n=e(R), xn=e(R, E, dt=BF16), kv=e(R, 2 * E, dt=BF16), dkv=e(R, 2 * E, dt=BF16),
                          dxn=e(R, E, dt=BF16), lse=e(B * Lr, 8), mean_f=e(B * Lr), rstd_f=e(B * Lr),
                          dq_part=e(hip.attn_reduce_partial_rows(B * Lr), E))
            else:
                hb.update(tmp=e(R, E))
            self.hb[t] = hb
        self.ln_ws = e(max(1, hip.layernorm_bwd_workspace(ws_rows, E)))
        self.scratch = e(ws_rows, E)      # LayerNorm-backward dx sink when the features are detached (probe)

    # ------------------------------------------------------------------------------------------ forward
    def _refuse_encode_phase(self, what: str) -> None:
        if self.phase == "encode":
            raise ValueError(f"{what}() needs a 'probe' or 'finetune' engine: phase 'encode' runs the encoders alone and has no heads "
                             "(use encode())")

    def forward(self, batch: dict) -> torch.Tensor:
        """Forward + ``loss_pred``; returns the loss as a 1-element device tensor (no host sync)."""
        self._refuse_encode_phase("forward")
        if self.store.refresh_half():
            self._pack_conv_weights()

        def one_pass():
            self.forward(batch)
            self.zero_grad()
            self.backward()
        self._first_step_passes(one_pass)
        batch = dict(batch)
        for t, c in self.model.dataset.targets.items():
            y = batch[t]
            if not y.is_cuda or not y.is_contiguous():
                raise ValueError(f"batch[{t!r}] must be a contiguous GPU tensor")
            if c.type_target == "multilabel_classif" and y.dtype != F32:
                batch[t] = y.float()
            elif c.type_target != "multilabel_classif" and y.dtype.is_floating_point:
                batch[t] = y.long()
        batch = self._stage_inputs(batch)
        with self._tuning_pass("forward"):
            self._segment("sup_forward", self._cur_key, lambda: self._forward_launches(batch))
        self._saved_for_backward = True
        return self.loss_acc

    def _embed_encode(self, g, batch) -> None:
        E, B = self.E, self.B  # noqa: N806
        gbuf, st = self.gb[g.name], self.enc[g.name]
        xg = st.x0.view(g.Beff, g.L, E)       # the embedding is written straight into the encoder's input (no masking)
        Lb = self.Lb[g.name]  # noqa: N806
        for s in g.mods:
            self.embed[s.name].forward(batch, gbuf, xg, g.L)
        st.forward()
        nrm = st.t.norm
        dst = self.joint.x0 if self.joint is not None else self.xenc
        hip.layernorm_fwd(st.x_last, Lb, 0, nrm.weight, nrm.bias, dst, self.JL, self.goff[g.name], gbuf["mean_e"], gbuf["rstd_e"],
                          B, Lb, E)

    def _encode_launches(self, batch: dict) -> None:
        """Embed + encoders (+ the joint encoder) + the token grids on the reference grid: everything in front of the heads."""
        E, B = self.E, self.B  # noqa: N806
        self._run_parallel([lambda g=g: self._embed_encode(g, batch) for g in self.groups])
        if self.joint is not None:
            self.joint.forward()
            jn, R = self.joint.t.norm, B * self.JL  # noqa: N806
            hip.layernorm_fwd(self.joint.x_last, R, 0, jn.weight, jn.bias, self.xenc, R, 0, self.mean_j, self.rstd_j, 1, R, E)
        if self.ref is not None:          # compute_logits: every modality's token grid on the reference grid (mim.py:351-373)
            self._tokens_on_ref_grid(self.ref)

    def _tokens_on_ref_grid(self, r: dict) -> None:
        d0 = 0
        for s in self.mods.values():
            hip.token_resize(self.xenc, self.JL, self.goff[s.group] + s.tok_off, r["x"], r["TD"] * r["Lr"], d0 * r["Lr"], self.B,
                             s.Dates, s.g, r["G"], self.E)
            d0 += s.Dates

    def _head_logits(self, t: str) -> None:
        """Head ``t`` from the encoded tokens up to and including its logits buffer."""
        m, E, B, ps = self.model, self.E, self.B, self.store  # noqa: N806
        hb, head = self.hb[t], m.heads[t]
        x = self.ref["x"] if hb["kind"] == "segment" else self.xenc
        R, n = hb["R"], B * hb["Lr"]  # noqa: N806
        if hb["attentive"]:
            red = head.reduce
            hip.layernorm_fwd(x, R, 0, red.norm.weight, red.norm.bias, hb["xn"], R, 0, hb["mean_n"], hb["rstd_n"], 1, R, E)
            hip.gemm(hip.GEMM_NT, R, 2 * E, E, hb["xn"], E, ps.h(red.to_kv.weight), E, hb["kv"], 2 * E)
            hip.attn_reduce_fwd(hb["kv"], red.query, hb["red"], hb["lse"], B, hb["T"], hb["Lr"], E, red.heads)
            out = hb["hfc"] if hb["kind"] == "segment" else hb["h"]
            hip.layernorm_fwd(hb["red"], n, 0, red.norm_fc.weight, red.norm_fc.bias, out, n, 0, hb["mean_f"], hb["rstd_f"], 1, n, E)
        else:
            hip.mean_reduce_fwd(x, hb["red"], B, hb["T"], hb["Lr"], E)
            if hb["kind"] == "segment":
                hip.cast_bf16(hb["red"], hb["hfc"], n * E)
        if hb["kind"] == "segment":
            W = hb["PPCp"]  # noqa: N806
            if "w16p" in hb:
                hip.cast_bf16(head.conv.weight, hb["w16p"], hb["PPC"] * E)
                hb["biasp"][: hb["PPC"]].copy_(head.conv.bias)
                w16, bias = hb["w16p"], hb["biasp"]
            else:
                w16, bias = ps.h(head.conv.weight).view(W, E), head.conv.bias
            hip.gemm(hip.GEMM_NT, n, W, E, hb["hfc"], E, w16, E, hb["logits"], W, hip.OUT_F32 | hip.BIAS, bias=bias)
        else:
            feat = hb["h"] if hb["attentive"] else hb["red"]
            hip.head_linear_fwd(feat, head.linear.weight, head.linear.bias, hb["logits"], B, hb["C"], E)

    def _forward_launches(self, batch: dict) -> None:
        B = self.B  # noqa: N806
        self.loss_acc.zero_()
        self._encode_launches(batch)
        for t, hb in self.hb.items():
            self._head_logits(t)
            tgt = batch[t]
            if hb["kind"] == "multilabel_classif":
                hip.bce_loss(hb["logits"], tgt, hb["missing"], self.loss_acc, hb["dlogits"], B, hb["C"])
                continue
            hb["cnt"].zero_()
            hip.count_valid(tgt, hb["missing"], hb["cnt"])
            if hb["kind"] == "segment":
                hip.ce_loss(hb["logits"], tgt, hb["missing"], hb["cnt"], self.loss_acc, hb["dlogits"], B, self.ref["G"], hb["P"], hb["C"],
                            ld=hb["PPCp"])
            else:
                hip.ce_loss(hb["logits"], tgt, hb["missing"], hb["cnt"], self.loss_acc, hb["dlogits"], B, 1, 1, hb["C"])

    # ------------------------------------------------------------------------------------------ prediction
    def _head_geometry(self, hb) -> tuple:
        """``(act, g, P, ld, map shape, prob shape)`` of a head's logits buffer as ``hip.predict_view`` takes it."""
        B, C = self.B, hb["C"]  # noqa: N806
        if hb["kind"] == "segment":
            G, P = self.ref["G"], hb["P"]  # noqa: N806
            return hip.PREDICT_SOFTMAX, G, P, hb["PPCp"], (B, G * P, G * P), (B, 1, C, G * P, G * P)
        if hb["kind"] == "multilabel_classif":
            return hip.PREDICT_SIGMOID, 1, 1, C, (B, C), (B, C)
        return hip.PREDICT_SOFTMAX, 1, 1, C, (B,), (B, C)

    def _predict_buffers(self, t: str, probs: bool) -> dict:
        """Engine-owned outputs of ``predict`` (stable addresses for the captured segments), allocated when first needed."""
        if not hasattr(self, "_pb"):
            self._pb = {}
        pb = self._pb.setdefault(t, {})
        _, _, _, _, map_shape, prob_shape = self._head_geometry(self.hb[t])
        if "cls" not in pb:
            pb["cls"] = torch.empty(map_shape, dtype=torch.uint8, device=self.device)
            pb["conf"] = torch.empty(map_shape, dtype=F32, device=self.device)
        if probs and "prob" not in pb:
            pb["prob"] = torch.empty(prob_shape, dtype=F32, device=self.device)
        return pb

    def _predict_view_launches(self, batch: dict, view: dict | None, mode: str, probs: bool, thr: dict) -> None:
        """One view: the rasters under the view's flags (``view``: flag tensor and destination rasters; None = the batch as it
        is), the forward up to every head's logits, ``mh_predict_view``.  ``mode``: "one" writes cls, conf (and prob when
        ``probs``) at once, "first" / "acc" start / continue the accumulation in prob."""
        flags = None
        if view is not None:
            flags, batch = view["flags"], dict(batch)
            for src, dst in view["rasters"].items():
                hip.dihedral(batch[src], dst, flags)
                batch[src] = dst
        self._encode_launches(batch)
        for t, hb in self.hb.items():
            self._head_logits(t)
            act, g, P, ld, _, _ = self._head_geometry(hb)  # noqa: N806
            pb = self._pb[t]
            one = mode == "one"
            hip.predict_view(hb["logits"], flags if act == hip.PREDICT_SOFTMAX else None, act, pb["prob"] if probs else None,
                             mode == "acc", pb["cls"] if one else None, pb["conf"] if one else None, self.B, g, P, hb["C"], ld=ld,
                             threshold=thr[t])

    def predict(self, batch: dict, views=(0,), probs: bool = False, threshold=0.5) -> dict:
        """Predictions ``{target: Prediction(cls, conf, probs)}`` for a batch WITHOUT labels: the rasters, their dates and
        ``ref_date``; target keys are ignored.  Nothing is read on the host.

        segment: ``cls`` u8 ``[B, S, S]`` (``torch.argmax`` of the logits), ``conf`` f32 ``[B, S, S]`` (the largest class
        probability), ``probs`` f32 ``[B, 1, C, S, S]`` (the layout of ``logits()``) or None; classif: ``[B]``, ``[B]``,
        ``[B, C]``; multilabel: ``cls`` u8 ``[B, C]`` = ``sigmoid > threshold`` (``threshold``: a float or ``{target: float}``,
        the metric's ``threshold_detect``), ``conf`` = the sigmoid ``[B, C]``, ``probs`` the same values.

        ``views``: dihedral flag bytes (``parse_views``; ``"d4"`` = all eight) for test-time augmentation -- every raster of the
        batch is transformed by ``mh_dihedral`` under one flag byte per view, the class probabilities of the views are summed at
        their places in the untransformed raster and ``cls`` / ``conf`` / ``probs`` are the arg-max, the largest mean and the mean.
        The launch list is the forward's up to the logits and nothing after (no loss, no target count, no start-up passes); one
        captured segment per kind of view.

        The returned tensors are the engine's own buffers: the next ``predict`` overwrites them.  Weights, gradients,
        ``loss_acc``, optimizer and metric state are untouched; the saved activations and ``logits()`` are those of the LAST
        view, in that view's orientation, so ``backward()`` raises until the next ``forward``."""
        self._refuse_encode_phase("predict")
        views = parse_views(views)
        ds = self.model.dataset
        thr = {t: float(threshold[t] if isinstance(threshold, dict) else threshold) for t in self.hb}
        if self.store.refresh_half():
            self._pack_conv_weights()
        batch = self._stage_inputs({k: v for k, v in batch.items() if k not in ds.targets})
        self._saved_for_backward = False
        direct = views == (0,)
        need_prob = probs or len(views) > 1
        for t in self.hb:
            self._predict_buffers(t, need_prob)
        view = None if direct else self._view_buffers(batch)
        key = (self._cur_key, probs, tuple(sorted(thr.items())))
        for i, v in enumerate(views):
            mode = "one" if len(views) == 1 else ("first" if i == 0 else "acc")
            if view is not None:
                view["flags"].fill_(v)       # in front of the segment: a replayed graph reads the flags of THIS view
            name = f"sup_predict:{'direct' if direct else mode}"
            self._segment(name, key, lambda mode=mode: self._predict_view_launches(batch, view, mode, need_prob, thr))
        out = {}
        for t, hb in self.hb.items():
            act, _, _, _, _, _ = self._head_geometry(hb)
            pb = self._pb[t]
            if len(views) > 1:
                C = hb["C"]  # noqa: N806
                hip.predict_finish(pb["prob"], len(views), act, pb["cls"], pb["conf"], self.B, C, pb["prob"].numel() // (self.B * C),
                                   threshold=thr[t], mean=pb["prob"] if probs else None)
            out[t] = Prediction(pb["cls"], pb["conf"], pb["prob"] if probs else None)
        return out

    # ------------------------------------------------------------------------------------------ features
    def _feature_buffers(self, level: str) -> dict:
        """Engine-owned outputs of ``encode`` (stable addresses for the captured segments), allocated when first needed; for
        ``"grid"`` on a model without a segment target also the token grids on the reference grid (``self.ref`` stays None: the
        forward's launch list does not change)."""
        if not hasattr(self, "_fb"):
            self._fb = {}
        fb = self._fb.get(level)
        if fb is not None:
            return fb
        B, E, dev = self.B, self.E, self.device  # noqa: N806
        if level == "sample":
            fb = dict(rows=B, f32=torch.empty(B, E, dtype=F32, device=dev), bf16=torch.empty(B, E, dtype=BF16, device=dev), ref=None)
        else:
            ref = self.ref
            if ref is None:
                ds = self.model.dataset
                if ds.ref_input is None:
                    raise ValueError("encode(level='grid'): the dataset names no ref_input, so there is no reference grid")
                G = self.model.out_grid_size[ds.ref_input]  # noqa: N806
                TD = sum(s.Dates for s in self.mods.values())  # noqa: N806
                ref = dict(G=G, Lr=G * G, TD=TD, x=torch.empty(B, TD * G * G, E, dtype=F32, device=dev))
            fb = dict(rows=B * ref["Lr"], f32=torch.empty(B, ref["Lr"], E, dtype=F32, device=dev),
                      bf16=torch.empty(B, ref["Lr"], E, dtype=BF16, device=dev), ref=ref)
        self._fb[level] = fb
        return fb

    def _feature_launches(self, batch: dict, level: str, normalize: bool, fb: dict) -> None:
        B, E = self.B, self.E  # noqa: N806
        self._encode_launches(batch)
        if level == "sample":
            hip.mean_reduce_fwd(self.xenc, fb["f32"], B, self.JL, 1, E)
        else:
            r = fb["ref"]
            if r is not self.ref:
                self._tokens_on_ref_grid(r)
            hip.mean_reduce_fwd(r["x"], fb["f32"], B, r["TD"], r["Lr"], E)
        f32, b16 = fb["f32"].view(fb["rows"], E), fb["bf16"].view(fb["rows"], E)
        if normalize:
            hip.l2_normalize(f32, y=f32, y16=b16, eps=1e-12)
        else:
            hip.cast_bf16(f32, b16, fb["rows"] * E)

    def encode(self, batch: dict, level: str = "sample", normalize: bool = True) -> Features:
        """Encoder features ``Features(f32, bf16)`` of a batch WITHOUT labels (target keys are ignored), in every phase: embed,
        encoders and the joint encoder as the forward runs them, nothing after.

        ``level="sample"``: the mean over all ``JL`` encoded tokens, ``[B, E]`` (``mh_mean_reduce_fwd`` with ``T = JL, Lr = 1``);
        ``level="grid"``: every modality's token grid on the reference grid ``G = out_grid_size[ref_input]`` (``mh_token_resize``),
        mean over the ``TD`` date slices, ``[B, G * G, E]``.  ``normalize``: rows divided by ``max(||row||_2, 1e-12)``
        (``mh_l2_normalize``, the rule of ``F.normalize``) with the bf16 copy rounded from the normalised fp32 row; off: the means
        themselves and their ``mh_cast_bf16`` copy.  One captured segment per ``(level, normalize)``.

        The returned tensors are the engine's own buffers: the next ``encode`` of the same level overwrites them.  Weights,
        gradients, ``loss_acc``, optimizer and metric state are untouched; like ``predict`` it overwrites the encoders' saved
        activations, so ``backward()`` raises until the next ``forward``."""
        check_encode_args(level, normalize)
        ds = self.model.dataset
        fb = self._feature_buffers(level)
        if self.store.refresh_half():
            self._pack_conv_weights()
        batch = self._stage_inputs({k: v for k, v in batch.items() if k not in ds.targets})
        self._saved_for_backward = False
        self._segment(f"sup_encode:{level}:{int(normalize)}", self._cur_key, lambda: self._feature_launches(batch, level, normalize, fb))
        return Features(fb["f32"], fb["bf16"])

    def _view_buffers(self, batch: dict) -> dict:
        """The flag bytes and the transformed rasters of a dihedral view (engine-owned, allocated when first needed)."""
        view = getattr(self, "_pv", None)
        if view is None:
            sources = [parts[0] for parts in self.model.src_specs.values()]
            view = self._pv = dict(flags=torch.zeros(self.B, dtype=torch.uint8, device=self.device),
                                   rasters={s.src: torch.empty_like(batch[s.src]) for s in sources})
        return view

    # ------------------------------------------------------------------------------------------ scene prediction
    def scene_geometry(self) -> dict:
        """``W`` (the window side in units, ``scene_unit`` of this model's sizes), ``q`` = pixels per unit of every input raster
        and ``qt`` = pixels per unit of every segment target."""
        sources = [parts[0] for parts in self.model.src_specs.values()]
        seg = {t: self.ref["G"] * hb["P"] for t, hb in self.hb.items() if hb["kind"] == "segment"}
        W = scene_unit([s.S for s in sources] + list(seg.values()))  # noqa: N806
        return dict(W=W, q={s.src: s.S // W for s in sources}, qt={t: S // W for t, S in seg.items()})

    def _scene_buffers(self, scene: dict, sources, table, N: int, Hu: int, Wu: int, blend: str) -> dict:  # noqa: N803
        """Engine-owned state of ``predict_scene``: the window batch the gather writes, the uploaded window table and the fixed
        rows of the current batch, the blend profiles, the canvases and the window grids.  Whatever depends on the scene's
        extent is allocated again when that changes."""
        dev, B, geo = self.device, self.B, self.scene_geometry()  # noqa: N806
        ps = self.__dict__.setdefault("_ps", dict(win={}, profile={}, canvas={}, grid={}))
        for k in [k for s in sources for k in (s.src, f"{s.src}_dates")] + ["ref_date"]:
            shape = (B,) + tuple(scene[k].shape[1:])
            if k in geo["q"]:                                              # a raster: one window of it per slot
                shape = shape[:3] + (geo["W"] * geo["q"][k],) * 2
            if k not in ps["win"] or ps["win"][k].shape != shape or ps["win"][k].dtype != scene[k].dtype:
                ps["win"][k] = torch.empty(shape, dtype=scene[k].dtype, device=dev)
        if "cur" not in ps:
            ps["cur"], ps["cur_n"] = torch.zeros(B, 4, dtype=I32, device=dev), torch.zeros(B, dtype=torch.int64, device=dev)
        ps["table"] = torch.from_numpy(table).to(dev)                  # the whole plan, uploaded once
        ps["table_n"] = ps["table"][:, :, 0].to(torch.int64).contiguous()
        n_rows = table.shape[0] * B
        for t, hb in self.hb.items():
            C = hb["C"]  # noqa: N806
            if hb["kind"] == "segment":
                S, q = self.ref["G"] * hb["P"], geo["qt"][t]  # noqa: N806
                if (S, blend) not in ps["profile"]:
                    ps["profile"][S, blend] = torch.from_numpy(hip.blend_profile(S, blend)).to(dev)
                cv = ps["canvas"].get(t)
                if cv is None or cv["acc"].shape != (N, C, Hu * q, Wu * q):
                    e = lambda *s, dt=F32: torch.empty(*s, dtype=dt, device=dev)  # noqa: E731
                    cv = ps["canvas"][t] = dict(acc=e(N, C, Hu * q, Wu * q), wsum=e(N, Hu * q, Wu * q),
                                                cls=e(N, Hu * q, Wu * q, dt=torch.uint8), conf=e(N, Hu * q, Wu * q))
            else:
                pb = self._pb[t]
                gr = ps["grid"].get(t)
                if gr is None or gr["cls"].shape[0] != n_rows:
                    gr = ps["grid"][t] = {k: torch.empty((n_rows,) + tuple(pb[k].shape[1:]), dtype=pb[k].dtype, device=dev)
                                          for k in ("cls", "conf", "prob")}
        return ps

    def predict_scene(self, scene: dict, stride: int | None = None, blend: str = "linear", views=(0,), probs: bool = False,
                      threshold=0.5) -> dict:
        """Predictions ``{target: Prediction(cls, conf, probs)}`` for whole SCENES: rasters larger than the model's window, cut
        into sliding windows on the device, predicted ``B`` windows at a time and blended into one canvas per segment target.

        ``scene`` is a batch without targets whose rasters are ``[N, D, C, Hu * q, Wu * q]`` (float32, contiguous, on the GPU):
        ``N`` scenes of ``Hu x Wu`` UNITS, a unit being ``1 / W`` of the model's window (``scene_geometry``: ``W`` is the greatest
        common divisor of every ``image_size`` and every segment target's size, ``q = image_size / W`` the raster's pixels per
        unit), with ``<m>_dates`` ``[N, D, 3]`` int16 and ``ref_date`` ``[N, 1, 3]``; ``Hu, Wu >= W``.  Rasters are taken at the
        model's own pixel scale: resampling a scene is the caller's job.

        Windows (``hip.scene_windows``): starts ``0, stride, 2 stride, ...`` along each axis and one last, clamped window that
        ends at the edge; ``stride`` in units, ``1 .. W``, default ``max(1, W // 2)``; scene-major, row-major; the last batch is
        padded with slots that blend nothing.  Per batch ONE captured segment: ``mh_window_gather`` per raster into the
        engine's window batch, the date rows by the slot's scene, the launch list of ``predict`` for every view of ``views``,
        ``mh_predict_blend`` per segment target with ``scale = 1 / len(views)``.  ``blend``: ``"linear"`` (a separable tent,
        ``hip.blend_profile``) or ``"flat"``; a canvas pixel is the weighted mean of the windows that cover it, summed in window
        order whatever ``B`` is (include/maestro_hip.h).  One ``mh_predict_blend_finish`` per segment target after the last batch.

        segment: ``cls`` u8 ``[N, Hc, Wc]``, ``conf`` f32 ``[N, Hc, Wc]``, ``probs`` f32 ``[N, C, Hc, Wc]`` or None, ``Hc = Hu * q_t``
        -- ``N * C * Hc * Wc * 4`` bytes of canvas per target, resident for the call: cutting a mosaic into scenes that fit is the
        caller's job.  classif / multilabel targets are not blended: the per-window results of ``predict`` on the window grid,
        ``[N, ny, nx]`` (``probs`` ``[N, ny, nx, C]``) / ``[N, ny, nx, C]``.

        Nothing is read on the host.  The returned tensors are the engine's own buffers (the next ``predict_scene`` overwrites
        them); weights, gradients, ``loss_acc``, optimizer and metric state are untouched; ``backward()`` raises until the next
        ``forward``.  ValueError before any launch: extents that disagree between the rasters, an extent below one window, a
        stride outside ``1 .. W``, a raster that is not float32 / contiguous / on the GPU, an unknown ``blend``."""
        self._refuse_encode_phase("predict_scene")
        views = parse_views(views)
        sources = [parts[0] for parts in self.model.src_specs.values()]
        geo = self.scene_geometry()
        W, B = geo["W"], self.B  # noqa: N806
        N, Hu, Wu, stride = check_scene(scene, {s.src: (s.S, s.Dates, s.C_src) for s in sources}, W, stride, blend, self.device)  # noqa: N806
        thr = {t: float(threshold[t] if isinstance(threshold, dict) else threshold) for t in self.hb}
        ys, xs = hip.scene_axis_starts(Hu, W, stride), hip.scene_axis_starts(Wu, W, stride)
        table = hip.scene_table(N, [(y, x) for y in ys for x in xs], B)
        if self.store.refresh_half():
            self._pack_conv_weights()
        self._saved_for_backward = False
        for t in self.hb:
            self._predict_buffers(t, True)
        ps = self._scene_buffers(scene, sources, table, N, Hu, Wu, blend)
        win, cur, cur_n = ps["win"], ps["cur"], ps["cur_n"]
        view = None if views == (0,) else self._view_buffers(win)
        seg = {t: (ps["canvas"][t], ps["profile"][self.ref["G"] * hb["P"], blend]) for t, hb in self.hb.items()
               if hb["kind"] == "segment"}
        for cv, _ in seg.values():
            cv["acc"].zero_()
            cv["wsum"].zero_()

        def launches(rows):
            for s in sources:
                img = scene[s.src]
                hip.window_gather(img, win[s.src], cur, rows, B, N, s.Dates * s.C_src, img.shape[3], img.shape[4], s.S, geo["q"][s.src])
                torch.index_select(scene[f"{s.src}_dates"], 0, cur_n, out=win[f"{s.src}_dates"])
            torch.index_select(scene["ref_date"], 0, cur_n, out=win["ref_date"])
            batch = self._staged = self._resize_inputs(dict(win), sources)
            for i, v in enumerate(views):
                if view is not None:
                    view["flags"].fill_(v)
                mode = "one" if len(views) == 1 else ("first" if i == 0 else "acc")
                self._predict_view_launches(batch, view, mode, True, thr)
            for t, hb in self.hb.items():
                pb = self._pb[t]
                if t in seg:
                    cv, profile = seg[t]
                    S = self.ref["G"] * hb["P"]  # noqa: N806
                    hip.predict_blend(pb["prob"], 1.0 / len(views), profile, cur, rows, cv["acc"], cv["wsum"], B, N, hb["C"], S,
                                      geo["qt"][t], cv["acc"].shape[2], cv["acc"].shape[3])
                elif len(views) > 1:
                    hip.predict_finish(pb["prob"], len(views), self._head_geometry(hb)[0], pb["cls"], pb["conf"], B, hb["C"], 1,
                                       threshold=thr[t], mean=pb["prob"])

        # the addresses the captured segment bakes in, and everything that shapes its launch list
        key = (tuple((scene[k].data_ptr(), win[k].data_ptr()) for k in sorted(win)), tuple(cv["acc"].data_ptr() for cv, _ in seg.values()),
               tuple(p.data_ptr() for _, p in seg.values()), N, Hu, Wu, views, tuple(sorted(thr.items())))
        for i in range(table.shape[0]):
            cur.copy_(ps["table"][i])         # in front of the segment: a replayed graph reads the rows of THIS batch
            cur_n.copy_(ps["table_n"][i])
            self._segment("sup_predict_scene", key, lambda i=i: launches(table[i]))
            for t, gr in ps["grid"].items():  # per-window results onto the window grid (pad slots land behind its end)
                for k in ("cls", "conf") + (("prob",) if probs else ()):
                    gr[k][i * B: (i + 1) * B].copy_(self._pb[t][k])
        out = {}
        ny, nx = len(ys), len(xs)
        for t, hb in self.hb.items():
            C = hb["C"]  # noqa: N806
            if t in seg:
                cv = seg[t][0]
                hip.predict_blend_finish(cv["acc"], cv["wsum"], cv["cls"], cv["conf"], cv["acc"] if probs else None, N, C,
                                         cv["wsum"][0].numel())
                out[t] = Prediction(cv["cls"], cv["conf"], cv["acc"] if probs else None)
                continue
            gr = ps["grid"][t]
            per = (C,) if hb["kind"] == "multilabel_classif" else ()
            out[t] = Prediction(gr["cls"][: N * ny * nx].view(N, ny, nx, *per), gr["conf"][: N * ny * nx].view(N, ny, nx, *per),
                                gr["prob"][: N * ny * nx].view(N, ny, nx, C) if probs else None)
        return out

    # ------------------------------------------------------------------------------------------ backward
    def zero_grad(self) -> None:
        self.store.grad.zero_()

    def backward(self, grad_scale: float = 1.0) -> None:
        """Backward of the last ``forward`` (d loss = 1) into the flat grad buffer (zero it first).  probe: heads only."""
        self._refuse_encode_phase("backward")
        if grad_scale != 1.0:
            raise NotImplementedError("loss scaling is not needed for bf16")
        if not getattr(self, "_saved_for_backward", True):
            raise RuntimeError("backward() after predict(): the saved activations are a prediction view's; run forward() first")
        key = getattr(self, "_cur_key", None)
        with self._tuning_pass("backward"):
            self._segment(f"sup_bwd_heads:{self.phase}", key, self._bwd_heads)
            if self.phase == "finetune":
                # with a gradient hook (data parallel) the joint encoder is a launch segment of its own: its finished slice --
                # and the heads' -- go to the all-reduce while the group encoders' backward still runs
                if self.grad_hook is not None and self.joint is not None:
                    self._segment("sup_bwd_joint:h", key, lambda: self._bwd_encoder("joint"))
                    self._segment("sup_bwd_encoder:h", key, lambda: self._bwd_encoder("groups"))
                else:
                    self._segment("sup_bwd_encoder", key, lambda: self._bwd_encoder("all"))

    def _bwd_heads(self) -> None:
        m, E, B, ps = self.model, self.E, self.B, self.store  # noqa: N806
        AT = hip.OUT_F32 | hip.ATOMIC  # noqa: N806
        fine = self.phase == "finetune"
        if fine:
            self.dxenc.zero_()
        first_ref = True
        head_wgrads = []     # (A = dY, B = X, dW, M, N, K = token rows, lda, ldb, ldc): issued as one grouped launch below
        for t, hb in self.hb.items():
            head = m.heads[t]
            seg = hb["kind"] == "segment"
            R, n = hb["R"], B * hb["Lr"]  # noqa: N806
            x = self.ref["x"] if seg else self.xenc
            # ---- through the output layer: gradient w.r.t. the reduced features
            if seg:
                W = hb["PPCp"]  # noqa: N806
                padded = "w16p" in hb
                w16 = hb["w16p"] if padded else ps.h(head.conv.weight).view(W, E)
                if hb["attentive"]:     # bf16 d(norm_fc output), parked in the head of dxn (rewritten by the to_kv dgrad later)
                    dfc = hb["dxn"][:n]
                    hip.gemm(hip.GEMM_NN, n, E, W, hb["dlogits"], W, w16, E, dfc, E)
                else:                   # mean reduction: the reduced features feed the conv directly
                    dfc = hb["dred"]
                    hip.gemm(hip.GEMM_NN, n, E, W, hb["dlogits"], W, w16, E, dfc, E, hip.OUT_F32)
                if padded:
                    hb["dWp"].zero_()
                    hb["dbp"].zero_()
                    hip.gemm(hip.GEMM_TN, W, E, n, hb["dlogits"], W, hb["hfc"], E, hb["dWp"], E, AT)
                    hip.unpack_rows_add(hb["dWp"], ps.g(head.conv.weight), 1, hb["PPC"] * E, W * E)
                    hip.colsum(hb["dlogits"], hb["dbp"], n, W, W)
                    hip.unpack_rows_add(hb["dbp"], ps.g(head.conv.bias), 1, hb["PPC"], W)
                else:
                    head_wgrads.append((hb["dlogits"], hb["hfc"], ps.g(head.conv.weight).view(W, E), W, E, n, W, E, E))
                    hip.colsum(hb["dlogits"], ps.g(head.conv.bias), n, W, W)
            else:
                feat = hb["h"] if hb["attentive"] else hb["red"]
                dfc = hb["dh"] if hb["attentive"] else hb["dred"]
                hip.head_linear_bwd(feat, head.linear.weight, hb["dlogits"], dfc, ps.g(head.linear.weight), ps.g(head.linear.bias),
                                    B, hb["C"], E)
            # ---- through the reduction: gradient w.r.t. the head's input tokens x
            if seg:
                dx, dres = self.ref["dx"], (None if first_ref else self.ref["dx"])
            else:
                dx, dres = (self.dxenc, self.dxenc) if fine else (self.scratch, None)
            if hb["attentive"]:
                red = head.reduce
                hip.layernorm_bwd(dfc, n, 0, hb["red"], n, 0, red.norm_fc.weight, hb["mean_f"], hb["rstd_f"], None, hb["dred"], None,
                                  ps.g(red.norm_fc.weight), ps.g(red.norm_fc.bias), None, self.ln_ws, 1, n, E)
                hip.attn_reduce_bwd(hb["kv"], red.query, hb["red"], hb["lse"], hb["dred"], hb["dkv"], hb["dq_part"], B, hb["T"],
                                    hb["Lr"], E, red.heads)
                hip.colsum(hb["dq_part"], ps.g(red.query), hb["dq_part"].shape[0], E, E)
                head_wgrads.append((hb["dkv"], hb["xn"], ps.g(red.to_kv.weight), 2 * E, E, R, 2 * E, E, E))
                hip.gemm(hip.GEMM_NN, R, E, 2 * E, hb["dkv"], 2 * E, ps.h(red.to_kv.weight), E, hb["dxn"], E)
                hip.layernorm_bwd(hb["dxn"], R, 0, x, R, 0, red.norm.weight, hb["mean_n"], hb["rstd_n"], dres, dx, None,
                                  ps.g(red.norm.weight), ps.g(red.norm.bias), None, self.ln_ws, 1, R, E)
            elif fine:
                if dres is None:
                    hip.mean_reduce_bwd(hb["dred"], dx, B, hb["T"], hb["Lr"], E)
                else:
                    hip.mean_reduce_bwd(hb["dred"], hb["tmp"], B, hb["T"], hb["Lr"], E)
                    dx.view(-1, E)[:R].add_(hb["tmp"])
            if seg:
                first_ref = False
            self._grads_ready(head)
        self._launch_head_wgrads(head_wgrads)
        if fine and self.ref is not None and not first_ref:      # transposed resize: reference grid -> each modality's tokens
            r, d0 = self.ref, 0
            for s in self.mods.values():
                hip.token_resize_bwd(r["dx"], r["TD"] * r["Lr"], d0 * r["Lr"], self.dxenc, self.JL, self.goff[s.group] + s.tok_off, B,
                                     s.Dates, s.g, r["G"], E, accumulate=True)
                d0 += s.Dates

    HEAD_K_CHUNK = 32768   # token rows per grouped-GEMM problem: a head sees up to B * dates * L_ref = 557 k rows

    def _launch_head_wgrads(self, probs) -> None:
        """The heads' weight gradients (few output tiles, very long K = token rows) as ONE grouped launch: every problem is
        cut along K into chunks that accumulate atomically into the zeroed gradient slot -- the grouped kernel's own form of
        split-K, at its ~1 PFLOP/s instead of the per-GEMM split-K launches."""
        if not probs:
            return
        if not hasattr(self, "_head_table"):
            chunks = []
            for (A, B, C, M, N, K, lda, ldb, ldc) in probs:  # noqa: N806
                nchunk = max(2, -(-K // self.HEAD_K_CHUNK))  # >= 2 problems per dW -> atomic accumulation into the zeroed slot
                step = -(-K // nchunk)
                for k0 in range(0, K, step):
                    k1 = min(K, k0 + step)
                    chunks.append((A[k0:k1], B[k0:k1], C, M, N, k1 - k0, lda, ldb, ldc))
            try:
                self._head_table = hip.GroupedTN(chunks, self.device)
            except hip.HipExtensionError:
                self._head_table = None
        if self._head_table is not None:
            self._head_table.launch()
            return
        AT = hip.OUT_F32 | hip.ATOMIC  # noqa: N806
        for (A, B, C, M, N, K, lda, ldb, ldc) in probs:  # noqa: N806
            hip.gemm(hip.GEMM_TN, M, N, K, A, lda, B, ldb, C, ldc, AT)

    def _wgrad_deferred(self) -> bool:
        if os.environ.get("MAESTRO_WGRAD") == "fused":
            return False
        if not hasattr(self, "_defer"):
            stacks = list(self.enc.values()) + ([self.joint] if self.joint is not None else [])
            try:
                tiles = sum(hip.GroupedTN.count_tiles(st.wgrad_problems()) for st in stacks)
                self._defer = tiles >= 512 or os.environ.get("MAESTRO_WGRAD") == "deferred"
            except hip.HipExtensionError:
                self._defer = False
        return self._defer

    def _bwd_encoder(self, part: str = "all") -> None:
        """``part``: "all" (one segment), or "joint" followed by "groups" (two segments, see ``backward``)."""
        m, E, B, ps = self.model, self.E, self.B, self.store  # noqa: N806
        defer = self._wgrad_deferred()
        if part in ("all", "joint"):
            self._src = self.dxenc
            if self.joint is not None:
                jt, R = self.joint, B * self.JL  # noqa: N806
                jn = jt.t.norm
                hip.layernorm_bwd(self.dxenc, R, 0, jt.x_last, R, 0, jn.weight, self.mean_j, self.rstd_j, None, jt.dxa, jt.top16,
                                  ps.g(jn.weight), ps.g(jn.bias), jt.top_bias_grad(), self.ln_ws, 1, R, E)
                self._src, _ = jt.backward(jt.dxa, defer=defer, ready=not defer)
                self._grads_ready(jn)
            if part == "joint":
                if defer:
                    self._launch_wgrads([(self.joint, 0, self.joint.depth)])
                    self._grads_ready(m.encoder_inter)
                return
        src = self._src

        def side(g):
            def run():
                gbuf, st = self.gb[g.name], self.enc[g.name]
                nrm, Lb = st.t.norm, self.Lb[g.name]  # noqa: N806
                hip.layernorm_bwd(src, self.JL, self.goff[g.name], st.x_last, Lb, 0, nrm.weight, gbuf["mean_e"], gbuf["rstd_e"],
                                  None, st.dxa, st.top16, ps.g(nrm.weight), ps.g(nrm.bias), st.top_bias_grad(), st.ln_ws, B, Lb, E)
                dx0, _ = st.backward(st.dxa, defer=defer, ready=False)
                dxg = dx0.view(g.Beff, g.L, E)
                for s in g.mods:    # (this engine's zero_grad leaves the conv-gradient staging buffers alone: cleared here, every time)
                    self.embed[s.name].backward(dxg, g.L, not self._dw_conv_clear)
            return run

        self._run_parallel([side(g) for g in self.groups])
        if defer:
            stacks = list(self.enc.values()) + ([self.joint] if (self.joint is not None and part == "all") else [])
            self._launch_wgrads([(st, 0, st.depth) for st in stacks])   # deferred LayerNorm / bias parameter + weight gradients
        for name in m.patch_embed:
            self._grads_ready(m.patch_embed[name])
        for name in m.encoder:
            self._grads_ready(m.encoder[name])
        if m.encoder_inter is not None and part == "all":
            self._grads_ready(m.encoder_inter)

    # ------------------------------------------------------------------------------------------ outputs
    def logits(self) -> dict:
        """Logits in the reference's layout: raster targets ``[B, 1, C, S, S]`` (head.py:116-130), others ``[B, C]``.  After
        ``predict`` they are those of its LAST view, in that view's orientation (not moved back to the untransformed raster)."""
        out = {}
        for t, hb in self.hb.items():
            if hb["kind"] == "segment":
                S = self.ref["G"] * hb["P"]  # noqa: N806
                img = torch.empty(self.B, hb["C"], S, S, dtype=F32, device=self.device)
                lg = hb["logits"] if hb["PPCp"] == hb["PPC"] else hb["logits"][:, : hb["PPC"]].contiguous()
                hip.depatchify(lg, img, self.B, hb["C"], S, hb["P"])
                out[t] = img.view(self.B, 1, hb["C"], S, S)
            else:
                out[t] = hb["logits"].clone()
        return out

    def update_metric(self, name_target: str, metric, batch: dict | None = None) -> None:
        """Feed the prediction metric of ``name_target`` (``maestro_amd/train/metric.py``) from the last ``forward``
        (``base.py:143-146``): the head's confusion kernel on the logits buffer and the staged target, with the arguments
        ``_forward_launches`` hands to ``hip.ce_loss`` / ``hip.bce_loss``.  One eager launch on the current stream, behind the
        forward segment and outside the captured graphs (the destination depends on the stage); nothing is read back.  A batch
        without a valid entry adds nothing (``base.py:126-127``)."""
        hb = self.hb[name_target]
        if batch is not None and name_target not in batch:
            raise KeyError(f"batch has no target {name_target!r}")
        tgt = self._staged[name_target]
        if hb["kind"] == "multilabel_classif":
            metric.update(hb["logits"], tgt, missing_val=hb["missing"])
        elif hb["kind"] == "segment":
            metric.update(hb["logits"], tgt, g=self.ref["G"], P=hb["P"], ld=hb["PPCp"], missing_val=hb["missing"])
        else:
            metric.update(hb["logits"], tgt, missing_val=hb["missing"])

    def logged_class_map(self, t: str) -> torch.Tensor:
        """Arg-max class map ``[S, S]`` of sample 0 of a raster target (the image logs of ``base.py:58-96`` keep only that
        sample): ``mh_predict_view`` on that sample's g x g token rows of the logits buffer."""
        hb = self.hb[t]
        G, S = self.ref["G"], self.ref["G"] * hb["P"]  # noqa: N806
        cls = torch.empty(1, S, S, dtype=torch.uint8, device=self.device)
        hip.predict_view(hb["logits"][: G * G], None, hip.PREDICT_SOFTMAX, None, False, cls, None, 1, G, hb["P"], hb["C"], ld=hb["PPCp"])
        return cls[0].long()
