"""Generate golden vectors by running the REFERENCE ITSELF (imported from /root/reference) on CPU.

TEST INFRASTRUCTURE ONLY.  Run in the build container (the reference does not exist on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python -m oracle.gen_golden            # writes tests/golden/*.npz

What it does
  * injects NON-ARITHMETIC stubs for packages the image lacks (dotenv, hydra_zen, rasterio, h5py, geopandas,
    pytorch_lightning, torchmetrics, torchvision, clearml, dacite) -- none of them computes anything on the path;
  * plugs this repo's restatement of ``vit_pytorch.vit.Transformer`` (oracle/vit.py) into ``sys.modules``
    (the real package is third-party, not vendored, not installed: SURVEY.md §8c);
  * resets ``torch.set_float32_matmul_precision("highest")`` after importing ``maestro.train.model`` (which sets
    "medium", reference ``maestro/train/model.py:15``);
  * for each case builds the reference model and the oracle with IDENTICAL weights, seeds the global CPU generator,
    runs the reference forward + ``compute_loss_rec`` + backward, records the RNG draws, and stores the reference's
    outputs.  Nothing from the reference's source is stored -- only inputs/outputs (data).

Weights and inputs are regenerated from seeds inside the tests (same torch build on every box); a checksum of the
weights is stored so a silent RNG change is detected instead of producing a false mismatch.
"""

from __future__ import annotations

import sys
import types
from pathlib import Path
from types import SimpleNamespace

sys.dont_write_bytecode = True

import numpy as np  # noqa: E402
import torch  # noqa: E402

REPO = Path(__file__).resolve().parent.parent
REFERENCE = Path("/root/reference")
import json  # noqa: E402
import os  # noqa: E402

GOLDEN = Path(os.environ.get("MAESTRO_GOLDEN_DIR", REPO / "tests" / "golden"))   # (tests redirect it to a temp directory)


# ----------------------------------------------------------------------------- stubs
def _install_stubs() -> None:
    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    mod("dotenv", load_dotenv=lambda *a, **k: None)

    class _Store:
        def __call__(self, *a, **k):
            return self if not a else a[0]

        def add_to_hydra_store(self, *a, **k):
            return None

    def _store(*a, **k):
        return _Store()

    mod("hydra_zen", MISSING=None, store=_store, builds=lambda *a, **k: None,
        make_custom_builds_fn=lambda *a, **k: (lambda *x, **y: None), zen=lambda *a, **k: None)
    rio = mod("rasterio")
    rio.errors = mod("rasterio.errors", NotGeoreferencedWarning=type("NotGeoreferencedWarning", (Warning,), {}))
    rio.windows = mod("rasterio.windows", Window=object)
    mod("h5py")
    mod("geopandas")
    mod("clearml", Task=object)
    dac = mod("dacite")
    dac.core = mod("dacite.core", from_dict=lambda *a, **k: None)

    class LightningModule(torch.nn.Module):
        def save_hyperparameters(self, *a, **k):
            return None

        def log(self, *a, **k):
            return None

    pl = mod("pytorch_lightning", LightningModule=LightningModule, Callback=object, Trainer=object,
             LightningDataModule=object, seed_everything=lambda *a, **k: None)
    pl.callbacks = mod("pytorch_lightning.callbacks", Callback=object, EarlyStopping=object,
                       LearningRateMonitor=object, ModelCheckpoint=object, TQDMProgressBar=object)
    pl.loggers = mod("pytorch_lightning.loggers", TensorBoardLogger=object)
    pl.utilities = mod("pytorch_lightning.utilities", rank_zero_only=lambda f: f)

    class Metric(torch.nn.Module):
        def __init__(self, *a, **k):
            super().__init__()

        def add_state(self, *a, **k):
            return None

        def update(self, *a, **k):
            return None

    nop = lambda *a, **k: None  # noqa: E731
    tm = mod("torchmetrics", Metric=Metric, MeanMetric=Metric)
    tm.functional = mod("torchmetrics.functional", confusion_matrix=nop)
    tm.functional.classification = mod("torchmetrics.functional.classification")
    mod("torchmetrics.functional.classification.average_precision", _multilabel_average_precision_compute=nop)
    mod("torchmetrics.functional.classification.precision_recall_curve",
        _multilabel_precision_recall_curve_format=nop, _multilabel_precision_recall_curve_update=nop)
    tm.utilities = mod("torchmetrics.utilities")
    mod("torchmetrics.utilities.data", dim_zero_cat=nop)
    mpl = mod("matplotlib", cm=None)
    mpl.colors = mod("matplotlib.colors", to_hex=nop)
    tv = mod("torchvision")
    tv.utils = mod("torchvision.utils", draw_segmentation_masks=lambda *a, **k: None)

    from oracle import vit as ovit

    vp = mod("vit_pytorch")
    vp.vit = mod("vit_pytorch.vit", Transformer=ovit.Transformer)


def import_reference():
    """Import the reference packages (read-only; no bytecode is written)."""
    _install_stubs()
    if str(REFERENCE) not in sys.path:
        sys.path.insert(0, str(REFERENCE))
    import maestro.train.model as ref_model  # noqa: F401  (sets matmul precision "medium")
    from maestro.conf.dataset import flair as rflair
    from maestro.conf.dataset import pastis_hd as rpastis
    from maestro.conf.dataset import s2_naip as rs2
    from maestro.conf.dataset import treesatai_ts as rts
    from maestro.conf.dataset.utils import InputRasterConfig, PatchSizeConfig
    from maestro.conf.datasets import DatasetsConfig
    from maestro.conf.mask import MaskConfig
    from maestro.layers import embed as rembed
    from maestro.layers import utils as rutils
    from maestro.ssl import mae as rmae

    torch.set_float32_matmul_precision("highest")
    return SimpleNamespace(model=ref_model, flair=rflair, pastis=rpastis, s2=rs2, ts=rts, mae=rmae,
                           InputRasterConfig=InputRasterConfig, PatchSizeConfig=PatchSizeConfig,
                           DatasetsConfig=DatasetsConfig, MaskConfig=MaskConfig, embed=rembed, utils=rutils)


# ----------------------------------------------------------------------------- cases
def case_table():
    """Case definitions shared with tests (tests rebuild OUR configs from the same table)."""
    return {
        # C1-shaped: single modality 3-band 64x64, patch 8 (BASELINE configs[0])
        "c1_spot": dict(
            dataset="s2_naip", ds_kwargs=dict(filter_inputs=["spot"]),
            mods=dict(spot=dict(image_size=64, patch=8, bands=3, norm_fac=255.0)),
            size="tiny", model_kw=dict(depth=4), inter_depth=1, fusion="group", B=2, seed=11),
        # C3-shaped (aerial + S2 time series), reduced aerial raster
        "c3_aerial_s2": dict(
            dataset="flair", ds_kwargs=dict(filter_inputs=["aerial", "s2"], filter_targets=[]),
            mods=dict(aerial=dict(image_size=64, patch=16, bands=[[3, 0, 1, 2]], norm_bands=[1, 3], norm_fac=255.0)),
            size="tiny", model_kw=dict(depth=4), inter_depth=2, fusion="group", B=2, seed=23),
        # C3'-shaped: dem (rescale_elev) + s1 group with two modalities (tie-dependent unmask)
        "c3p_dem_s1": dict(
            dataset="flair", ds_kwargs=dict(filter_inputs=["dem", "s1_asc", "s1_des"], filter_targets=[], ref_input=None),
            mods=dict(dem=dict(image_size=64, patch=32, bands=2, norm_fac=1000.0, rescale_elev=True)),
            size="tiny", model_kw=dict(depth=3), inter_depth=1, fusion="group", B=2, seed=5),
        # C4-shaped: TreeSatAI-TS, aerial grid 5 -> bilinear pos-enc resize branch (96 % 5 != 0)
        "c4_treesat": dict(
            dataset="treesatai_ts", ds_kwargs=dict(filter_targets=[]),
            mods=dict(aerial=dict(image_size=100, patch=20, bands=4, norm_bands=[1, 3], norm_fac=255.0)),
            size="tiny", model_kw=dict(depth=3), inter_depth=1, fusion="group", B=2, seed=7),
        # other fusion modes (tie-free by construction: no structural masking)
        "ts_shared": dict(
            dataset="treesatai_ts", ds_kwargs=dict(filter_targets=[]),
            mods=dict(aerial=dict(image_size=60, patch=20, bands=4, norm_bands=[1, 3], norm_fac=255.0)),
            size="tiny", model_kw=dict(depth=2), inter_depth=0, fusion="shared", B=2, seed=3),
        "ts_monotemp": dict(
            dataset="treesatai_ts", ds_kwargs=dict(filter_targets=[]),
            mods=dict(aerial=dict(image_size=60, patch=20, bands=4, norm_bands=[1, 3], norm_fac=255.0)),
            size="tiny", model_kw=dict(depth=2), inter_depth=0, fusion="monotemp", B=2, seed=4),
        "ts_mod": dict(
            dataset="treesatai_ts", ds_kwargs=dict(filter_targets=[]),
            mods=dict(aerial=dict(image_size=60, patch=20, bands=4, norm_bands=[1, 3], norm_fac=255.0)),
            size="tiny", model_kw=dict(depth=2), inter_depth=1, fusion="mod", B=2, seed=9),
        # C5-shaped (S2-NAIP urban: aerial + spot + s2 + s1, four groups) with the SURVEY §8d "patch-group-wise norm stress"
        # inputs: constant patches (sigma^2 -> 0 exercises the +1e-6 of model.py:226-229) and heavy-tailed exp(3 randn) bands
        "c5_s2naip_stress": dict(
            dataset="s2_naip", ds_kwargs=dict(),
            mods=dict(aerial=dict(image_size=64, patch=16, bands=4, norm_bands=[1, 3], norm_fac=255.0),
                      spot=dict(image_size=32, patch=16, bands=3, norm_fac=255.0)),
            size="tiny", model_kw=dict(depth=3), inter_depth=1, fusion="group", B=2, seed=43, stress=True),   # (seed 41 has #struct-masked > k in one sample: tie-dependent)
        # several band-groups per modality (embed.py:18-34, mim.py:49-57; no shipped config has them): every band-group has its
        # own patch-embed / pixelify conv and mask token and sits on the date axis in (g, d) order; mask_bands draws per
        # (sample, band-group); the norm_bands groups [1, 3] of the loss target STRADDLE the band-groups [2, 2]
        "bg_aerial_s2": dict(
            dataset="flair", ds_kwargs=dict(filter_inputs=["aerial", "s2"], filter_targets=[]),
            mods=dict(aerial=dict(image_size=64, patch=16, bands=[[3, 0], [1, 2]], norm_bands=[1, 3], norm_fac=255.0)),
            size="tiny", model_kw=dict(depth=3), inter_depth=1, fusion="group", B=2, seed=52, mask_kw=dict(mask_bands=0.3)),
        # band-groups of different sizes ([1] and [1] of a 2-band elevation raster: rescale_elev refers to channel 0 of the
        # RASTER, i.e. across the band-groups), one encoder per modality
        "bg_dem_mod": dict(
            dataset="flair", ds_kwargs=dict(filter_inputs=["dem", "s1_asc"], filter_targets=[], ref_input=None),
            mods=dict(dem=dict(image_size=64, patch=32, bands=[[0], [1]], norm_fac=1000.0, rescale_elev=True)),
            size="tiny", model_kw=dict(depth=2), inter_depth=1, fusion="mod", B=2, seed=61, mask_kw=dict(mask_bands=0.4)),
        # band-groups AND dates folded into the batch (utils.py:26-37: sequence index (b, g, d)), one encoder per modality
        "bg_ts_monotemp": dict(
            dataset="treesatai_ts", ds_kwargs=dict(filter_targets=[]),
            mods=dict(aerial=dict(image_size=60, patch=20, bands=[[0, 1, 2], [3]], norm_bands=[1, 3], norm_fac=255.0)),
            size="tiny", model_kw=dict(depth=2), inter_depth=0, fusion="monotemp", B=2, seed=71),
    }


def sup_case_table():
    """Probe / finetune cases: dataset with targets, head type; each runs in both phases."""
    return {
        # FLAIR-shaped segmentation on the aerial grid; s2 tokens are bilinearly resized 5x5 -> 4x4 onto it
        "sup_flair_seg": dict(
            dataset="flair", ds_kwargs=dict(filter_inputs=["aerial", "s2"], filter_targets=["cosia"], crop_meters=51.2),
            mods=dict(aerial=dict(image_size=64, patch=16, bands=[[3, 0, 1, 2]], norm_bands=[1, 3], norm_fac=255.0)),
            size="tiny", model_kw=dict(depth=3), inter_depth=1, fusion="group", type_head="attentive", B=2, seed=31),
        # TreeSatAI-TS-shaped multilabel classification over all tokens, attentive and mean ("linear") reductions
        "sup_treesat_mlc": dict(
            dataset="treesatai_ts", ds_kwargs=dict(filter_targets=["treesat_mlc_thresh"]),
            mods=dict(aerial=dict(image_size=60, patch=20, bands=4, norm_bands=[1, 3], norm_fac=255.0)),
            size="tiny", model_kw=dict(depth=3), inter_depth=1, fusion="group", type_head="attentive", B=3, seed=32),
        "sup_treesat_mean": dict(
            dataset="treesatai_ts", ds_kwargs=dict(filter_targets=["treesat_mlc_thresh"]),
            mods=dict(aerial=dict(image_size=60, patch=20, bands=4, norm_bands=[1, 3], norm_fac=255.0)),
            size="tiny", model_kw=dict(depth=2), inter_depth=0, fusion="mod", type_head="linear", B=3, seed=33),
        # PASTIS-HD-shaped: two targets at once (segmentation with missing_val = 19 on the s2 grid + multilabel)
        "sup_pastis_two": dict(
            dataset="pastis_hd", ds_kwargs=dict(filter_inputs=["s2", "s1_asc"], filter_targets=["pastis_seg", "pastis_mlc"]),
            mods=dict(), size="tiny", model_kw=dict(depth=2), inter_depth=1, fusion="group", type_head="attentive",
            B=2, seed=34),
        # two band-groups of different sizes in the reference input of a segmentation target: the heads see G * D date slots
        "sup_flair_bands": dict(
            dataset="flair", ds_kwargs=dict(filter_inputs=["aerial", "s2"], filter_targets=["cosia"], crop_meters=51.2),
            mods=dict(aerial=dict(image_size=64, patch=16, bands=[[3, 0, 1], [2]], norm_bands=[1, 3], norm_fac=255.0)),
            size="tiny", model_kw=dict(depth=2), inter_depth=1, fusion="group", type_head="attentive", B=2, seed=37),
        "sup_bands_shared": dict(
            dataset="flair", ds_kwargs=dict(filter_inputs=["aerial", "s2"], filter_targets=["cosia"], crop_meters=51.2),
            mods=dict(aerial=dict(image_size=64, patch=16, bands=[[3, 0], [1, 2]], norm_bands=[1, 3], norm_fac=255.0)),
            size="tiny", model_kw=dict(depth=2), inter_depth=0, fusion="shared", type_head="attentive", B=2, seed=38),
        # dates folded into the batch (utils.py:26-37): ONE encoder for every modality and date / one per modality;
        # the heads still see [B, sum(dates) * L] tokens (segmentation: every date's grid resized to the reference grid)
        "sup_flair_shared": dict(
            dataset="flair", ds_kwargs=dict(filter_inputs=["aerial", "s2"], filter_targets=["cosia"], crop_meters=51.2),
            mods=dict(aerial=dict(image_size=64, patch=16, bands=[[3, 0, 1, 2]], norm_bands=[1, 3], norm_fac=255.0)),
            size="tiny", model_kw=dict(depth=2), inter_depth=0, fusion="shared", type_head="attentive", B=2, seed=35),
        "sup_treesat_monotemp": dict(
            dataset="treesatai_ts", ds_kwargs=dict(filter_targets=["treesat_mlc_thresh"]),
            mods=dict(aerial=dict(image_size=60, patch=20, bands=4, norm_bands=[1, 3], norm_fac=255.0)),
            size="tiny", model_kw=dict(depth=2), inter_depth=0, fusion="monotemp", type_head="attentive", B=2, seed=36),
    }


def make_targets(dataset, B: int, seed: int) -> dict:  # noqa: N803
    """Synthetic targets of the wire format: raster targets int64 [B, 1, 1, H, W] (about 10 % missing_val pixels),
    multilabel targets float32 [B, C] in {0, 1} (sample 0 carries a missing_val entry), classif int64 [B]."""
    out = {}
    for i, (t, c) in enumerate(dataset.targets.items()):
        g = torch.Generator().manual_seed(777 + 31 * seed + i)
        if c.type_target == "segment":
            H = round(dataset.crop_meters / c.resolution_meters)  # noqa: N806
            y = torch.randint(0, c.num_classes, (B, 1, 1, H, H), generator=g)
            y[torch.rand(B, 1, 1, H, H, generator=g) < 0.1] = c.missing_val
        elif c.type_target == "multilabel_classif":
            y = (torch.rand(B, c.num_classes, generator=g) < 0.3).float()
            if B > 1:
                y[0, 1] = c.missing_val
        else:
            y = torch.randint(0, c.num_classes, (B,), generator=g)
        out[t] = y
    return out


def token_masks(pixel_mask: torch.Tensor, mod) -> torch.Tensor:
    """Token-level view ``[B, G * D, L]`` of a pixel-level ``mask_rec`` ``[B, D, C, S, S]`` (the pixel mask is the token mask
    repeated over the patch and over the channels of a band-group): top-left pixel of every patch, first channel of every
    band-group, band-groups stacked on the date axis in (g, d) order as ``Patchify`` does (embed.py:31-34)."""
    P = mod.patch_size.mae  # noqa: N806
    sizes = [mod.bands] if isinstance(mod.bands, int) else [len(b) for b in mod.bands]
    firsts = [sum(sizes[:i]) for i in range(len(sizes))]
    return torch.cat([pixel_mask[:, :, c, ::P, ::P].flatten(2) for c in firsts], dim=1)


def build_datasets(case: dict, ns) -> object:
    """Instantiate a DatasetsConfig from a case with either the reference's or this repo's classes (``ns``)."""
    cls = {"flair": ns.FLAIRConfig, "treesatai_ts": ns.TreeSatAITSConfig, "pastis_hd": ns.PASTISHDConfig,
           "s2_naip": ns.S2NAIPConfig}[case["dataset"]]
    kw = dict(case["ds_kwargs"])
    for name, m in case["mods"].items():
        m = dict(m)
        kw[name] = ns.InputRasterConfig(image_size=m.pop("image_size"),
                                        patch_size=ns.PatchSizeConfig(mae=m.pop("patch")), **m)
    return ns.DatasetsConfig(root_dir=None, name_dataset=case["dataset"], **{case["dataset"]: cls(**kw)})


def stress_raster(x: torch.Tensor, patch: int, g: torch.Generator) -> torch.Tensor:
    """SURVEY §8d norm-stress variant of a raster [B, D, C, S, S]: sample 0 gets per-patch CONSTANT tiles in its first
    band (every norm group containing only that band has sigma^2 = 0 exactly), the last band of every sample is
    heavy-tailed, exp(3 randn)."""
    x = x.clone()
    B, D, C, S, _ = x.shape  # noqa: N806
    n = S // patch
    const = torch.rand(D, n, n, generator=g)
    x[0, :, 0] = const.repeat_interleave(patch, dim=1).repeat_interleave(patch, dim=2)
    x[:, :, C - 1] = torch.exp(3.0 * torch.randn(B, D, S, S, generator=g))
    return x


def make_batch(dataset, B: int, seed: int, stress: bool = False, sizes: dict | None = None) -> dict:  # noqa: N803
    """Synthetic batch of the wire format: rasters fp32 [B,D,C,S,S], dates int16 [B,D,3].  ``sizes``: modality ->
    raster edge when the data does NOT arrive at ``image_size`` (resize_and_rescale then interpolates, mim.py:425-437)."""
    batch = {}
    for i, (m, c) in enumerate(dataset.inputs.items()):
        g = torch.Generator().manual_seed(1234 + 97 * seed + i)
        C = c.bands if isinstance(c.bands, int) else sum(len(b) for b in c.bands)  # noqa: N806
        S = (sizes or {}).get(m, c.image_size)  # noqa: N806
        batch[m] = torch.rand(B, c.num_dates, C, S, S, generator=g)
        if stress:
            batch[m] = stress_raster(batch[m], c.patch_size.mae, g)
        d = torch.arange(c.num_dates)
        dates = torch.stack([torch.full_like(d, 2019), 100 + 7 * d + i, torch.full_like(d, 10)], dim=-1)
        batch[f"{m}_dates"] = dates[None].expand(B, -1, -1).clone().to(torch.int16)
        batch[f"{m}_dates"][1:, :, 1] += 3  # make samples differ
    batch["ref_date"] = torch.tensor([[[2019, 182, 0]]], dtype=torch.int16).expand(B, 1, 3).clone()
    return batch


def init_weights(model: torch.nn.Module, seed: int) -> float:
    """Deterministic non-trivial weights (incl. LayerNorm/GroupNorm affine and biases); returns a checksum."""
    g = torch.Generator().manual_seed(seed)
    chk = 0.0
    with torch.no_grad():
        for name, p in sorted(model.state_dict().items()):
            if not p.dtype.is_floating_point:
                continue
            if name.endswith("norm.weight") or name.endswith("norm_fc.weight") or ".net.0.weight" in name:
                p.copy_(1.0 + 0.2 * torch.randn(p.shape, generator=g))
            elif p.ndim <= 1 or name.endswith("bias"):
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
            elif "mask_token" in name:
                p.copy_(torch.randn(p.shape, generator=g))
            else:
                fan_in = p[0].numel()
                p.copy_(torch.randn(p.shape, generator=g) * (1.0 / fan_in**0.5))
            chk += float(p.double().abs().sum())
    return chk


class _RandRecorder:
    """Records every ``torch.rand`` draw (value) while the reference runs -- data, not code."""

    def __init__(self):
        self.draws, self._orig = [], torch.rand

    def __enter__(self):
        def rec(*a, **k):
            t = self._orig(*a, **k)
            self.draws.append(t.detach().clone())
            return t

        torch.rand = rec
        return self

    def __exit__(self, *exc):
        torch.rand = self._orig


def tie_case_table():
    """Tie-DEPENDENT cases, kept apart from ``case_table``: in at least one (sample, group) more than k tokens are
    structurally masked, so WHICH of them the reference masks -- and, in the two-modality s1 group, which mask token lands
    where -- is decided by the tie order of torch's unstable CPU sorts.  They pin ``MAEEngine.tie_order = "torch"`` and the
    oracle's ``reference_tie_order`` (which reissue the reference's own calls) against the reference itself."""
    base = case_table()
    return {
        # the seed that case_table avoids for c5 (one sample with #struct-masked > k), plain inputs
        "ties_c5_s2naip": dict(base["c5_s2naip_stress"], seed=41, stress=False),
        # heavy structural masking on the C3'-shaped case: ties in the masked set AND the two-modality s1 group
        "ties_c3p_dem_s1": dict(base["c3p_dem_s1"], seed=6, mask_kw=dict(mask_mod=0.5, mask_dates=0.5, mask_loc=0.5)),
    }


def resize_case_table():
    """Cases whose rasters do NOT arrive at ``image_size`` (round 6): the non-identity branch of
    ``resize_and_rescale`` (mim.py:425-437) with the interpolation modes the reference's own tests sweep (tests/test_model.py:8-132),
    a ``dem`` modality included so that ``rescale_elev`` follows the resize; the resized, rescaled raster (the returned batch = the
    loss target) is stored for every modality."""
    return {
        # aerial arrives larger (80 -> 64: down-sampling), dem smaller (48 -> 64: up-sampling, then 30 (ch0 - ch1))
        "rs_bilinear_aerial_dem": dict(
            dataset="flair", ds_kwargs=dict(filter_inputs=["aerial", "dem"], filter_targets=[]),
            mods=dict(aerial=dict(image_size=64, patch=16, bands=4, norm_bands=[1, 3], norm_fac=255.0),
                      dem=dict(image_size=64, patch=32, bands=2, norm_fac=1000.0, rescale_elev=True)),
            size="tiny", model_kw=dict(depth=3), inter_depth=1, fusion="group", B=2, seed=83,
            interpolate="bilinear", raster_size=dict(aerial=80, dem=48)),
        # bicubic (overshoots: values leave [0, 1]); aerial up-sampled 40 -> 64, dem down-sampled 96 -> 64, s2 at its native size
        "rs_bicubic_aerial_dem_s2": dict(
            dataset="flair", ds_kwargs=dict(filter_inputs=["aerial", "dem", "s2"], filter_targets=[]),
            mods=dict(aerial=dict(image_size=64, patch=16, bands=4, norm_bands=[1, 3], norm_fac=255.0),
                      dem=dict(image_size=64, patch=32, bands=2, norm_fac=1000.0, rescale_elev=True)),
            size="tiny", model_kw=dict(depth=3), inter_depth=1, fusion="group", B=2, seed=89,
            interpolate="bicubic", raster_size=dict(aerial=40, dem=96)),
    }


def _tie_free(noise: torch.Tensor, struct: torch.Tensor, k: int) -> bool:
    return bool((struct.reshape(noise.shape).sum(dim=1) <= k).all())


def run_case(name: str, case: dict, ref, ours) -> dict:
    from oracle import mae as omae

    ds_ref = build_datasets(case, SimpleNamespace(
        FLAIRConfig=ref.flair.FLAIRConfig, TreeSatAITSConfig=ref.ts.TreeSatAITSConfig,
        PASTISHDConfig=ref.pastis.PASTISHDConfig, S2NAIPConfig=ref.s2.S2NAIPConfig,
        InputRasterConfig=ref.InputRasterConfig, PatchSizeConfig=ref.PatchSizeConfig,
        DatasetsConfig=lambda root_dir, name_dataset, **kw: ref.DatasetsConfig(
            root_dir=root_dir, name_dataset=name_dataset,
            **{k: kw.get(k, d()) for k, d in dict(
                treesatai_ts=ref.ts.TreeSatAITSConfig, pastis_hd=ref.pastis.PASTISHDConfig,
                flair=ref.flair.FLAIRConfig, s2_naip=ref.s2.S2NAIPConfig).items()})))
    ds_our = build_datasets(case, ours)
    mask_ref, mask_our = ref.MaskConfig(**case.get("mask_kw", {})), ours.MaskConfig(**case.get("mask_kw", {}))

    torch.manual_seed(1000 + case["seed"])
    interp = case.get("interpolate", "nearest")
    ssl = ref.model.SSLModule(datasets=ds_ref, mask=mask_ref, interpolate=interp, fusion_mode=case["fusion"],
                              inter_depth=case["inter_depth"], model="mae", model_size=case["size"],
                              loss="l2_norm", use_ema=False)
    common = dict(interpolate=interp, fusion_mode=case["fusion"], inter_depth=case["inter_depth"], model="mae",
                  num_levels=1, type_head="attentive", fac_abs_enc=1.0, fac_date_enc=1.0)
    ssl.model = getattr(ref.mae, f"mae_{case['size']}")(datasets=ds_ref, mask=mask_ref, **common, **case["model_kw"])
    oracle = omae.build_oracle(ds_our, mask_our, model_size=case["size"], **common, **case["model_kw"])
    chk = init_weights(oracle, case["seed"])
    missing, unexpected = ssl.model.load_state_dict(oracle.state_dict(), strict=False)
    assert not unexpected, unexpected
    assert all(k.startswith("heads.") for k in missing), missing
    ssl.trainer = SimpleNamespace(ssl_phase="pretrain")

    batch = make_batch(ds_our.dataset, case["B"], case["seed"], stress=case.get("stress", False), sizes=case.get("raster_size"))
    out = {"weights_checksum": np.float64(chk)}

    # ---- reference forward/backward with recorded RNG draws
    torch.manual_seed(4242 + case["seed"])
    rb = {k: v.clone() for k, v in batch.items()}
    with _RandRecorder() as rr:
        rb, rec, msk, _ = ssl.model(rb, ssl_phase="pretrain")
    groups = list(oracle.mask_ratio.keys()) if case["fusion"] in ("group", "mod") else None
    losses = {}
    for loss in ("l2_norm", "l1_norm", "l2", "l1"):
        ssl.norm_pix_loss = loss.endswith("_norm")
        ssl.loss_fn = torch.abs if loss.startswith("l1") else torch.square
        losses[loss] = ssl.compute_loss_rec(rb, rec, msk, stage="train")
        out[f"loss_{loss}"] = np.float64(losses[loss].item())
    # image-log tensors of sample [0, 0] (model.py:160-193), as the reference's pretrain_step returns them every step
    with torch.no_grad():
        for logs in ssl.compute_logs_rec(rb, rec, msk, ssl_phase="pretrain", stage="train"):
            for key, img in logs.items():
                out[f"logs/{key}"] = img.detach().numpy().astype(np.float32)
    ssl.model.zero_grad()
    losses["l2_norm"].backward()
    grads = {k: p.grad for k, p in ssl.model.named_parameters() if p.grad is not None}
    for k in sorted(grads):
        out[f"gradnorm/{k}"] = np.float64(grads[k].double().norm().item())
    # a few full small gradients
    for k in grads:
        if "mask_token" in k or k.endswith("enc_to_dec.%s.bias" % next(iter(oracle.enc_to_dec))):
            out[f"grad/{k}"] = grads[k].numpy().copy()

    # ---- oracle on the same inputs with the SAME global-RNG seed (draw order must coincide)
    torch.manual_seed(4242 + case["seed"])
    ob = {k: v.clone() for k, v in batch.items()}
    with _RandRecorder() as ro:
        ob, orec, omsk, _, internals = oracle(ob, "pretrain", return_internals=True)
    assert len(rr.draws) == len(ro.draws), (name, len(rr.draws), len(ro.draws))
    for a, b in zip(rr.draws, ro.draws):
        assert a.shape == b.shape and torch.equal(a, b), f"{name}: RNG draw order differs"

    # last len(groups) draws of the reference are the per-group noise [B, L] (mae.py:239)
    gnames = list(internals["mask_tok"].keys())
    noise = {g: rr.draws[len(rr.draws) - len(gnames) + i] for i, g in enumerate(gnames)}
    tie_free = {}
    for g in gnames:
        k = oracle.num_masked(oracle.mask_ratio[g], noise[g].shape[1])
        tie_free[g] = _tie_free(noise[g], internals["struct_masks"][g], k)
        out[f"noise/{g}"] = noise[g].numpy().copy()
        out[f"struct/{g}"] = np.packbits(internals["struct_masks"][g].reshape(noise[g].shape).numpy(), axis=1)
        out[f"tie_free/{g}"] = np.bool_(tie_free[g])
    for m in rec:
        out[f"pixels_rec/{m}"] = rec[m].detach().numpy().astype(np.float32)
        # reference's token-level mask (pixel mask is its repeat): take the top-left pixel of each patch, channel 0
        out[f"mask_tok/{m}"] = np.packbits(token_masks(msk[m], ds_our.dataset.inputs[m]).numpy(), axis=2)
        # the returned batch (= the loss target) where the reference changed it: elevation rescale and / or a real resize
        out[f"target/{m}"] = rb[m].detach().numpy().astype(np.float32) \
            if (ds_our.dataset.inputs[m].rescale_elev or m in case.get("raster_size", {})) else np.zeros(0, np.float32)

    # ---- report oracle-vs-reference agreement now (the tests re-check from the stored vectors)
    report = {}
    for m in rec:
        report[m] = (float((rec[m] - orec[m]).detach().abs().max()), bool(torch.equal(msk[m], omsk[m])))
    if not all(r[0] < 1e-4 for r in report.values()):
        oracle.reference_tie_order = True
        torch.manual_seed(4242 + case["seed"])
        qb = {k: v.clone() for k, v in batch.items()}
        _, qrec, _, _ = oracle(qb, "pretrain")
        oracle.reference_tie_order = False
        quirk = {m: float((rec[m] - qrec[m]).detach().abs().max()) for m in rec}
        print(f"[{name}] reference-tie-order mode: max|rec diff| per mod = {quirk}")
        assert all(v < 1e-4 for v in quirk.values())
    from oracle.mae import compute_loss_rec, norm_bands_of
    ol = compute_loss_rec(ob, orec, omsk, oracle.out_grid_size, norm_bands_of(oracle.dataset), "l2_norm")
    print(f"[{name}] tie_free={tie_free} loss_ref={out['loss_l2_norm']:.8f} loss_oracle={ol.item():.8f} "
          f"draws={len(rr.draws)} max|rec diff|,mask equal per mod={report}")
    return out


def run_sup_case(name: str, case: dict, ref, ours) -> dict:
    """Reference probe / finetune forward + loss_pred + backward on seeded weights and inputs -> stored vectors."""
    from collections import defaultdict

    from oracle import heads as oheads
    from oracle import mae as omae

    ns_ref = SimpleNamespace(
        FLAIRConfig=ref.flair.FLAIRConfig, TreeSatAITSConfig=ref.ts.TreeSatAITSConfig,
        PASTISHDConfig=ref.pastis.PASTISHDConfig, S2NAIPConfig=ref.s2.S2NAIPConfig,
        InputRasterConfig=ref.InputRasterConfig, PatchSizeConfig=ref.PatchSizeConfig,
        DatasetsConfig=lambda root_dir, name_dataset, **kw: ref.DatasetsConfig(
            root_dir=root_dir, name_dataset=name_dataset,
            **{k: kw.get(k, d()) for k, d in dict(
                treesatai_ts=ref.ts.TreeSatAITSConfig, pastis_hd=ref.pastis.PASTISHDConfig,
                flair=ref.flair.FLAIRConfig, s2_naip=ref.s2.S2NAIPConfig).items()}))
    ds_ref, ds_our = build_datasets(case, ns_ref), build_datasets(case, ours)
    torch.manual_seed(1000 + case["seed"])
    ssl = ref.model.SSLModule(datasets=ds_ref, mask=ref.MaskConfig(), interpolate="nearest", fusion_mode=case["fusion"],
                              inter_depth=case["inter_depth"], model="mae", model_size=case["size"],
                              type_head=case["type_head"], loss="l2_norm", use_ema=False)
    common = dict(interpolate="nearest", fusion_mode=case["fusion"], inter_depth=case["inter_depth"], model="mae",
                  num_levels=1, type_head=case["type_head"], fac_abs_enc=1.0, fac_date_enc=1.0)
    ssl.model = getattr(ref.mae, f"mae_{case['size']}")(datasets=ds_ref, mask=ref.MaskConfig(), **common, **case["model_kw"])
    oracle = omae.build_oracle(ds_our, ours.MaskConfig(), model_size=case["size"], **common, **case["model_kw"])
    chk = init_weights(oracle, case["seed"])
    missing, unexpected = ssl.model.load_state_dict(oracle.state_dict(), strict=True)   # heads included: key-for-key
    assert not missing and not unexpected

    class _NoMetric:   # the metric updates of compute_loss_pred are logging, not arithmetic of the loss
        def update(self, *a, **k):
            pass

    ssl._modules.pop("metrics", None)
    ssl.metrics = defaultdict(_NoMetric)

    batch = make_batch(ds_our.dataset, case["B"], case["seed"])
    batch.update(make_targets(ds_our.dataset, case["B"], case["seed"]))
    out = {"weights_checksum": np.float64(chk)}
    for phase in ("probe", "finetune"):
        ssl.trainer = SimpleNamespace(ssl_phase=phase)
        rb = {k: v.clone() for k, v in batch.items()}
        rb, _, _, logits = ssl.model(rb, ssl_phase=phase)
        loss = ssl.compute_loss_pred(rb, logits, stage="train")
        ssl.model.zero_grad()
        loss.backward()
        out[f"{phase}/loss"] = np.float64(loss.item())
        for k, p in ssl.model.named_parameters():
            if p.grad is not None:
                out[f"{phase}/gradnorm/{k}"] = np.float64(p.grad.double().norm().item())
        for t, lg in logits.items():
            flat = lg.detach().reshape(lg.shape[0], -1)
            stride = max(1, flat.shape[1] // 4096)
            out[f"{phase}/logits/{t}"] = flat[:, ::stride].numpy().astype(np.float32)   # strided sample of every logit map
            out[f"{phase}/logits_sum/{t}"] = np.float64(lg.detach().double().sum().item())
        # oracle on the same inputs
        ob = {k: v.clone() for k, v in batch.items()}
        ob, _, _, ologits = oracle(ob, phase)
        oloss = oheads.compute_loss_pred(oracle.dataset, ob, ologits)
        worst = max(float((logits[t] - ologits[t]).detach().abs().max()) for t in logits)
        print(f"[{name}/{phase}] loss_ref={loss.item():.8f} loss_oracle={oloss.item():.8f} max|logit diff|={worst:.2e} "
              f"params with grad={sum(1 for k in out if k.startswith(phase + '/gradnorm/'))}")
        assert worst < 1e-4 and abs(loss.item() - oloss.item()) < 1e-5
    return out


CKPT_CASE = dict(dataset="s2_naip", ds_kwargs=dict(filter_inputs=["spot"]),
                 mods=dict(spot=dict(image_size=64, patch=8, bands=3, norm_fac=255.0)))
CKPT_HP = dict(interpolate="nearest", fusion_mode="group", inter_depth=3, model="mae", model_size="tiny",
               type_head="attentive", loss="l1_norm", use_date_enc=True, use_ema=True)
CKPT_MASK = dict(mask_ratio=0.6, mask_loc=0.1)


def ckpt_value(key: str, salt: int = 0) -> float:
    """Constant fill value of checkpoint tensor ``key`` (low entropy on purpose: the gzip'ed fixture stays a few tens of KB
    although the tiny model + its EMA copy hold 15 M parameters; what the fixture pins are keys, shapes, the pickled
    hyper-parameters and that every tensor lands in its own slot)."""
    import zlib
    return (zlib.crc32(f"{salt}:{key}".encode()) % 251) / 256.0 - 0.5


def _ref_namespace(ref):
    return SimpleNamespace(
        FLAIRConfig=ref.flair.FLAIRConfig, TreeSatAITSConfig=ref.ts.TreeSatAITSConfig,
        PASTISHDConfig=ref.pastis.PASTISHDConfig, S2NAIPConfig=ref.s2.S2NAIPConfig,
        InputRasterConfig=ref.InputRasterConfig, PatchSizeConfig=ref.PatchSizeConfig,
        DatasetsConfig=lambda root_dir, name_dataset, **kw: ref.DatasetsConfig(
            root_dir=root_dir, name_dataset=name_dataset,
            **{k: kw.get(k, d()) for k, d in dict(
                treesatai_ts=ref.ts.TreeSatAITSConfig, pastis_hd=ref.pastis.PASTISHDConfig,
                flair=ref.flair.FLAIRConfig, s2_naip=ref.s2.S2NAIPConfig).items()}))


def run_ckpt(ref, ours) -> None:
    """Checkpoint interchange (``maestro/run_experiment.py:66-74``, ``maestro/train/model.py:118``).

    (1) The REFERENCE ``SSLModule`` (tiny, ``use_ema=True``) is saved in Lightning's ``.ckpt`` layout with
        ``hyper_parameters`` exactly as ``save_hyperparameters(ignore=["datasets"])`` records them -- ``mask`` is the
        reference's own ``maestro.conf.mask.MaskConfig`` instance -> ``tests/golden/ref_written.ckpt.gz`` (data only).
    (2) A checkpoint written by ``maestro_amd`` is loaded into the reference module with ``strict=True`` the way
        ``LightningModule.load_from_checkpoint`` does it (``cls(**hyper_parameters, datasets=...)`` + ``load_state_dict``)."""
    import gzip
    import io
    import tempfile

    from maestro_amd.train.model import SSLModule as OurModule

    ds_ref, ds_our = build_datasets(CKPT_CASE, _ref_namespace(ref)), build_datasets(CKPT_CASE, ours)
    mask_ref = ref.MaskConfig(**CKPT_MASK)
    ssl = ref.model.SSLModule(datasets=ds_ref, mask=mask_ref, **CKPT_HP)
    with torch.no_grad():
        for k, v in ssl.state_dict().items():
            v.fill_(ckpt_value(k))
    ckpt = {"epoch": 3, "global_step": 120, "pytorch-lightning_version": "2.5.0", "state_dict": ssl.state_dict(),
            "loops": {}, "callbacks": {}, "optimizer_states": [], "lr_schedulers": [], "hparams_name": "kwargs",
            "hyper_parameters": dict(mask=mask_ref, **CKPT_HP)}
    buf = io.BytesIO()
    torch.save(ckpt, buf)
    with gzip.GzipFile(GOLDEN / "ref_written.ckpt.gz", "wb", compresslevel=9, mtime=0) as f:
        f.write(buf.getvalue())
    n_keys = len(ckpt["state_dict"])
    print(f"[ckpt] reference-written checkpoint: {n_keys} tensors ({sum(k.startswith('ema_model.') for k in ckpt['state_dict'])} "
          f"ema), {len(buf.getvalue()) / 1e6:.1f} MB raw -> {(GOLDEN / 'ref_written.ckpt.gz').stat().st_size / 1e3:.1f} KB gz")

    # (2) ours -> reference
    mod = OurModule(datasets=ds_our, mask=ours.MaskConfig(**CKPT_MASK), **CKPT_HP)
    with torch.no_grad():
        for k, v in mod.state_dict().items():
            v.fill_(ckpt_value(k, salt=1))
    with tempfile.TemporaryDirectory() as tmp:
        path = Path(tmp) / "ours.ckpt"
        mod.save_checkpoint(path)
        back = torch.load(path, map_location="cpu", weights_only=False)     # the real maestro.conf.mask resolves here
    assert type(back["hyper_parameters"]["mask"]) is ref.MaskConfig, type(back["hyper_parameters"]["mask"])
    again = ref.model.SSLModule(datasets=ds_ref, **back["hyper_parameters"])
    res = again.load_state_dict(back["state_dict"], strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for k, v in again.state_dict().items():
        assert float(v.flatten()[0]) == np.float32(ckpt_value(k, salt=1)), k
    assert again.model.mask_ratio and vars(back["hyper_parameters"]["mask"]) == vars(ours.MaskConfig(**CKPT_MASK))
    print(f"[ckpt] maestro_amd-written checkpoint loaded into the reference SSLModule with strict=True "
          f"({len(back['state_dict'])} tensors, mask = {back['hyper_parameters']['mask']})")

    # (3) the one-line swap of maestro/run_experiment.py:39-40: OUR SSLModule built from the REFERENCE's own config objects
    #     (DatasetsConfig / MaskConfig / ModelConfig instances, exactly what run_experiment passes) -- duck-typed, no conversion
    from maestro.conf.model import ModelConfig as RefModelConfig
    shapes = {}
    for fusion, inter in (("group", 3), ("mod", 1), ("shared", 0), ("monotemp", 0)):
        cfg = RefModelConfig(model_size="tiny", fusion_mode=fusion, inter_depth=inter, use_ema=False)
        theirs = ref.model.SSLModule(datasets=ds_ref, mask=mask_ref, **vars(cfg))
        swapped = OurModule(datasets=ds_ref, mask=mask_ref, **vars(cfg))
        a = {k: tuple(v.shape) for k, v in theirs.state_dict().items()}
        b = {k: tuple(v.shape) for k, v in swapped.state_dict().items()}
        assert a == b, (fusion, sorted(set(a) ^ set(b))[:5])
        assert swapped.norm_bands == theirs.norm_bands and swapped.model.mask_ratio == theirs.model.mask_ratio
        assert swapped.model.grid_size == theirs.model.grid_size and swapped.model.len_bands == theirs.model.len_bands
        shapes[fusion] = {k: list(v) for k, v in a.items()}
    # the reference module's state-dict keys and shapes per fusion mode, for the test that runs without the reference
    (GOLDEN / "ref_ckpt_shapes.json").write_text(json.dumps(shapes, sort_keys=True) + "\n")
    print(f"[ckpt] maestro_amd SSLModule built from the reference's config objects: state-dict keys and shapes equal the "
          f"reference module's for all four fusion modes ({len(a)} tensors)")


def layer_vectors(ref) -> dict:
    """Known-answer vectors for the directly importable reference layers (embed.py / utils.py)."""
    out = {}
    torch.manual_seed(77)
    out["posemb_12_12_40"] = ref.utils.posemb_sincos_2d(12, 12, 40, 8).numpy()
    tab = ref.utils.posemb_sincos_2d(96, 96, 24, 8)
    for grid in (3, 5, 15, 96):
        out[f"pool_96_{grid}"] = ref.utils.reshape_encoding(tab, grid)[0, 0].numpy()
    dates = torch.tensor([[[2019, 100, 10], [2020, 3, 23], [2018, 365, 0]],
                          [[2021, 200, 12], [2019, 182, 0], [2017, 1, 5]]], dtype=torch.int16)
    ref_date = torch.tensor([[[2019, 182, 0]], [[2020, 1, 0]]], dtype=torch.int16)
    out["dates_in"], out["ref_date_in"] = dates.numpy(), ref_date.numpy()
    out["encode_dates_g2_lb1"] = ref.utils.encode_dates(dates, ref_date, dim=16, date_dim=8, fac_date_enc=1.0,
                                                        grid_size=2, len_bands=1).numpy()
    out["encode_dates_g1_lb2"] = ref.utils.encode_dates(dates, ref_date, dim=12, date_dim=8, fac_date_enc=0.5,
                                                        grid_size=1, len_bands=2).numpy()
    # Patchify / Pixelify with two band-groups (len_bands > 1 is unused by shipped configs)
    pat = ref.embed.Patchify([[0, 1], [2]], 16, 4)
    pix = ref.embed.Pixelify(16, [[0, 1], [2]], 4)
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for p in list(pat.parameters()) + list(pix.parameters()):
            p.copy_(torch.randn(p.shape, generator=g) * 0.3)
    x = torch.rand(2, 3, 3, 8, 8, generator=g)
    y = pat(x)
    tok = torch.randn(2, 6, 4, 16, generator=g)
    mk = torch.rand(2, 6, 4, 1, generator=g) < 0.5
    img, mimg = pix(tok, mk)
    out["patchify_params"] = np.concatenate([p.detach().numpy().ravel() for p in pat.parameters()])
    out["pixelify_params"] = np.concatenate([p.detach().numpy().ravel() for p in pix.parameters()])
    out["patchify_in"], out["patchify_out"] = x.numpy(), y.detach().numpy()
    out["pixelify_in"], out["pixelify_mask_in"] = tok.numpy(), mk.numpy()
    out["pixelify_out"], out["pixelify_mask_out"] = img.detach().numpy(), mimg.numpy()
    return out


def main() -> None:
    sys.path.insert(0, str(REPO))
    import maestro_amd.conf as ours

    ref = import_reference()
    GOLDEN.mkdir(parents=True, exist_ok=True)
    meta = dict(torch=torch.__version__, threads=torch.get_num_threads())
    which = sys.argv[1] if len(sys.argv) > 1 else "all"      # all | pretrain | sup | ckpt  [case,case…]
    only = set(sys.argv[2].split(",")) if len(sys.argv) > 2 else None   # optional: comma-separated case names
    if which in ("all", "pretrain"):
        np.savez_compressed(GOLDEN / "layers.npz", **layer_vectors(ref))
        for name, case in {**case_table(), **tie_case_table(), **resize_case_table()}.items():
            if only is not None and name not in only:
                continue
            out = run_case(name, case, ref, ours)
            np.savez_compressed(GOLDEN / f"{name}.npz", torch_version=np.array(meta["torch"]), **out)
    if which in ("all", "ckpt"):
        run_ckpt(ref, ours)
    for name, case in (sup_case_table().items() if which in ("all", "sup") else ()):
        if only is not None and name not in only:
            continue
        out = run_sup_case(name, case, ref, ours)
        np.savez_compressed(GOLDEN / f"{name}.npz", torch_version=np.array(meta["torch"]), **out)
    pyc = [p for p in REFERENCE.rglob("__pycache__")]
    assert not pyc, f"bytecode was written into the reference tree: {pyc}"
    print("golden vectors written to", GOLDEN)


if __name__ == "__main__":
    main()
