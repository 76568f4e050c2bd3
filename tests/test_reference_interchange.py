"""Checkpoint interchange with the reference, checked against what the reference itself recorded (runs without it).

``oracle/gen_golden.py ckpt`` runs the reference once and stores what its side of the interchange needs under ``tests/golden/``:
the checkpoint its ``SSLModule`` writes (``ref_written.ckpt.gz``: keys, shapes, dtypes, pickled hyper-parameters) and its
module's state-dict keys and shapes for the four fusion modes (``ref_ckpt_shapes.json``).  The reference's
``load_from_checkpoint`` builds ``cls(**hyper_parameters, datasets=...)`` and loads the state dict with ``strict=True``
(``maestro/run_experiment.py:66-74``): a checkpoint written by ``maestro_amd`` loads there exactly when its hyper-parameters
are the reference's and its state dict has the reference module's keys and shapes -- which is what this test asserts."""

import gzip
import io
import json

import torch

import maestro_amd.conf as conf
from maestro_amd.train.model import SSLModule, _RenamingPickle
from oracle.gen_golden import CKPT_CASE, CKPT_HP, CKPT_MASK, build_datasets, ckpt_value


def _load(raw: bytes) -> dict:
    return torch.load(io.BytesIO(raw), map_location="cpu", weights_only=False, pickle_module=_RenamingPickle)


def _layout(sd: dict) -> dict:
    return {k: (tuple(v.shape), v.dtype) for k, v in sd.items()}


def test_checkpoints_go_both_ways(tmp_path, golden_dir):
    ref = _load(gzip.decompress((golden_dir / "ref_written.ckpt.gz").read_bytes()))     # what the reference wrote
    ds = build_datasets(CKPT_CASE, conf)

    # ours -> reference: the same hyper-parameters (mask under the reference's class path) and the same state-dict layout
    mod = SSLModule(datasets=ds, mask=conf.MaskConfig(**CKPT_MASK), **CKPT_HP)
    with torch.no_grad():
        for k, v in mod.state_dict().items():
            v.fill_(ckpt_value(k, salt=1))
    path = tmp_path / "ours.ckpt"
    mod.save_checkpoint(path)
    raw = path.read_bytes()
    assert b"maestro.conf.mask" in raw and b"maestro_amd" not in raw
    back = _load(raw)
    hp, ref_hp = dict(back["hyper_parameters"]), dict(ref["hyper_parameters"])
    assert vars(hp.pop("mask")) == vars(ref_hp.pop("mask")) == vars(conf.MaskConfig(**CKPT_MASK))
    assert hp == ref_hp
    assert _layout(back["state_dict"]) == _layout(ref["state_dict"])
    for k, v in back["state_dict"].items():
        assert float(v.flatten()[0]) == float(torch.tensor(ckpt_value(k, salt=1), dtype=v.dtype)), k

    # the module built from the reference's ModelConfig fields has the reference module's keys and shapes in every fusion mode
    want = json.loads((golden_dir / "ref_ckpt_shapes.json").read_text())
    mask = conf.MaskConfig(**CKPT_MASK)
    for fusion, inter in (("group", 3), ("mod", 1), ("shared", 0), ("monotemp", 0)):
        cfg = conf.ModelConfig(model_size="tiny", fusion_mode=fusion, inter_depth=inter, use_ema=False)
        ours = SSLModule(datasets=ds, mask=mask, **vars(cfg))
        got = {k: list(v.shape) for k, v in ours.state_dict().items() if k != "_anchor"}
        assert got == want[fusion], (fusion, sorted(set(got) ^ set(want[fusion]))[:5])
