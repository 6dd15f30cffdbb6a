"""Experiment configuration for the benchmark harness.

Only the keys the hot path's callers read are kept (model + loss + the
optimiser/step keys of the train section); values are those of the
reference's JSON configs:

* ``kitti_base()``  — configs/kitti_base.json:27-43 (loss, model), :46-70 (train)
* ``sintel_base()`` — configs/sintel_base.json (same loss/model/train keys)
* ``sintel_mf()``   — configs/sintel_aug+hg+mf.json:3-6 on top of sintel_base
  (mask-feature correlation branch, ``aggregation_type="concat"``)
* ``kitti_stage1()`` / ``sintel_stage1()`` — the base config with its
  ``train.stage1.loss`` overrides applied (from epoch 50 of 200: the census
  term alone, bidirectional occlusion check)
* ``kitti_stage1_ar()`` / ``sintel_stage1_ar()`` — the stage-1 config with its
  ``train.stage1.train`` overrides applied as well (``run_atst``, ``run_st``,
  ``run_ot``, ``ot_size``) and the train keys the augmentation branch reads
  (``w_ar``, ``ar_eps``, ``ar_q``, ``mask_st``, ``st_cfg``): the step of
  epochs 50-200 (unsamflow_amd.ar, harness.TrainStep)
* ``kitti_stage2_hg()`` / ``sintel_stage2_hg()`` — the stage-1 AR config with
  the ``train.stage2`` overrides of configs/kitti_aug+hg.json /
  configs/sintel_aug+hg.json applied (from epoch 150): the homography
  smoothness loss (``smooth_type "homography"``, ``w_sm 0.1``, KITTI
  ``ransac_threshold 0.5``; Sintel leaves it to unFlowLoss's default of 3) and
  ``w_ar 0.1``; ``key_obj_aug`` stays ``False`` here (unsamflow_amd.homography,
  flow_loss.unFlowLoss)
* ``kitti_aug()`` / ``sintel_aug()`` and ``kitti_aug_hg()`` / ``sintel_aug_hg()``
  — the stage-1 AR config and the stage-2 homography config with the rest of
  ``train.stage2`` of configs/*_aug.json / configs/*_aug+hg.json applied:
  ``key_obj_aug true``, ``key_obj_count 3``, ``w_ar 0.1`` (from epoch 150: the
  key-object augmentation of the third pass, unsamflow_amd.fake_object)

``load_json`` reads a reference-format JSON file with the one-level
``base_configs`` inheritance + recursive merge of utils/config_parser.py:11-33.
"""
from __future__ import annotations

import copy
import json
import os


class AttrDict(dict):
    """dict with attribute access (the reference uses EasyDict)."""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e

    def __setattr__(self, k, v):
        self[k] = v

    def __delattr__(self, k):
        del self[k]

    @classmethod
    def wrap(cls, obj):
        if isinstance(obj, dict):
            return cls({k: cls.wrap(v) for k, v in obj.items()})
        if isinstance(obj, list):
            return [cls.wrap(v) for v in obj]
        return obj


def merge(base: dict, new: dict) -> dict:
    """Recursive override of ``base`` by ``new`` (config_parser.update_config)."""
    for k, v in new.items():
        if k in base and isinstance(base[k], dict) and isinstance(v, dict):
            merge(base[k], v)
        else:
            base[k] = v
    return base


def load_json(path: str) -> AttrDict:
    with open(path) as f:
        cfg = json.load(f)
    if "base_configs" in cfg:
        with open(os.path.join(os.path.dirname(path), cfg["base_configs"])) as f:
            base = json.load(f)
        cfg = merge(base, cfg)
    return AttrDict.wrap(cfg)


_LOSS = {
    "edge_aware_alpha": 10,
    "occ_from_back": True,
    "smooth_type": "2nd",
    "smooth_edge": "image",
    "type": "unflow",
    "w_l1": 0.15,
    "w_ph_scales": [1.0, 1.0, 1.0, 1.0, 0.0],
    "w_sm": 0,
    "w_ssim": 0.85,
    "w_ternary": 0.0,
    "warp_pad": "border",
    "with_bk": True,
}
_MODEL = {"learned_upsampler": True, "reduce_dense": True, "type": "pwclite"}
_TRAIN = {
    "batch_size": 8,
    "beta": 0.999,
    "bias_decay": 0,
    "lr": 0.0002,
    "max_grad_norm": 10,
    "momentum": 0.9,
    "optim": "adam",
    "weight_decay": 1e-06,
    "lr_scheduler": {
        "module": "OneCycleLR",
        "params": {"max_lr": 0.0004, "pct_start": 0.05, "cycle_momentum": False, "anneal_strategy": "linear"},
    },
    "epoch_num": 200,
    "epoch_size": 1000,
}


def kitti_base() -> AttrDict:
    return AttrDict.wrap({
        "data": {"train_shape": [256, 832], "test_shape": [256, 832]},
        "loss": copy.deepcopy(_LOSS),
        "model": copy.deepcopy(_MODEL),
        "seed": 42,
        "train": copy.deepcopy(_TRAIN),
    })


def sintel_base() -> AttrDict:
    cfg = kitti_base()
    cfg.data = AttrDict.wrap({"test_shape": [448, 1024]})
    return cfg


def sintel_mf() -> AttrDict:
    cfg = sintel_base()
    cfg.model.add_mask_corr = True
    cfg.model.aggregation_type = "concat"
    return cfg


# train.stage1.loss of configs/kitti_base.json and configs/sintel_base.json
_STAGE1_LOSS = {"occ_from_back": False, "w_l1": 0.0, "w_ssim": 0.0, "w_ternary": 1.0}


def kitti_stage1() -> AttrDict:
    cfg = kitti_base()
    cfg.loss.update(_STAGE1_LOSS)
    return cfg


def sintel_stage1() -> AttrDict:
    cfg = sintel_base()
    cfg.loss.update(_STAGE1_LOSS)
    return cfg


# the train keys the augmentation branch reads (configs/*_base.json "train") with
# train.stage1.train applied; st_cfg and ot_size differ between the data sets
_AR_TRAIN = {"ar_eps": 0.0, "ar_q": 1.0, "key_obj_aug": False, "mask_st": True, "run_atst": True, "run_ot": True,
             "run_st": True, "w_ar": 0.02}
_ST_CFG_KITTI = {"add_noise": True, "hflip": True, "rotate": [-0.01, 0.01, -0.01, 0.01],
                 "squeeze": [1.0, 1.0, 1.0, 1.0], "trans": [0.04, 0.005], "vflip": False,
                 "zoom": [1.0, 1.4, 0.99, 1.01]}
_ST_CFG_SINTEL = {"add_noise": True, "hflip": True, "rotate": [-0.2, 0.2, -0.015, 0.015],
                  "squeeze": [0.86, 1.16, 1.0, 1.0], "trans": [0.2, 0.015], "vflip": True,
                  "zoom": [1.0, 1.5, 0.985, 1.015]}


def kitti_stage1_ar() -> AttrDict:
    cfg = kitti_stage1()
    cfg.train.update(AttrDict.wrap(dict(copy.deepcopy(_AR_TRAIN), ot_size=[192, 640],
                                        st_cfg=copy.deepcopy(_ST_CFG_KITTI))))
    return cfg


def sintel_stage1_ar() -> AttrDict:
    cfg = sintel_stage1()
    cfg.train.update(AttrDict.wrap(dict(copy.deepcopy(_AR_TRAIN), ot_size=[320, 704],
                                        st_cfg=copy.deepcopy(_ST_CFG_SINTEL))))
    return cfg


# train.stage2 of configs/kitti_aug+hg.json and configs/sintel_aug+hg.json (key_obj_aug aside)
_STAGE2_HG_LOSS = {"smooth_type": "homography", "w_sm": 0.1}


def kitti_stage2_hg() -> AttrDict:
    cfg = kitti_stage1_ar()
    cfg.loss.update(dict(_STAGE2_HG_LOSS, ransac_threshold=0.5))
    cfg.train.w_ar = 0.1
    return cfg


def sintel_stage2_hg() -> AttrDict:
    cfg = sintel_stage1_ar()
    cfg.loss.update(_STAGE2_HG_LOSS)
    cfg.train.w_ar = 0.1
    return cfg


# the key-object part of train.stage2 of configs/*_aug.json and configs/*_aug+hg.json
_KEY_OBJ_TRAIN = {"key_obj_aug": True, "key_obj_count": 3, "w_ar": 0.1}


def kitti_aug() -> AttrDict:
    cfg = kitti_stage1_ar()
    cfg.train.update(_KEY_OBJ_TRAIN)
    return cfg


def sintel_aug() -> AttrDict:
    cfg = sintel_stage1_ar()
    cfg.train.update(_KEY_OBJ_TRAIN)
    return cfg


def kitti_aug_hg() -> AttrDict:
    cfg = kitti_stage2_hg()
    cfg.train.update(_KEY_OBJ_TRAIN)
    return cfg


def sintel_aug_hg() -> AttrDict:
    cfg = sintel_stage2_hg()
    cfg.train.update(_KEY_OBJ_TRAIN)
    return cfg
