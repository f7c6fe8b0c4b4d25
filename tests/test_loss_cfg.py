"""CPU tests of the loss definition settings: cfg -> MaskRCNN keyword arguments (engine/defaults.py loss_kwargs: MODEL.RPN.{LOSS_WEIGHT,
BBOX_REG_LOSS_TYPE, BBOX_REG_LOSS_WEIGHT, SMOOTH_L1_BETA, BBOX_REG_WEIGHTS}, MODEL.ROI_BOX_HEAD.{SMOOTH_L1_BETA, BBOX_REG_LOSS_TYPE,
BBOX_REG_LOSS_WEIGHT, BBOX_REG_WEIGHTS, CLS_AGNOSTIC_BBOX_REG, TRAIN_ON_PRED_BOXES}), the refusals, the ctypes mirror of amp_loss_opts and the
exported symbols.  The device side is tests/test_loss_cfg_gpu.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg():
    from ampis_amd import model_zoo
    from ampis_amd.config import get_cfg
    cfg = get_cfg()
    cfg.merge_from_file(model_zoo.get_config_file("COCO-InstanceSegmentation/mask_rcnn_R_50_FPN_3x.yaml"))
    return cfg


def _struct_dict(o):
    return {n: getattr(o, n) for n, _ in type(o)._fields_}


def test_default_cfg_maps_to_todays_loss():
    from ampis_amd import _lib
    from ampis_amd.engine.defaults import loss_kwargs, train_model_kwargs
    kw = loss_kwargs(_cfg())
    assert set(kw) == {"loss", "bbox_reg_weights"}
    assert kw["bbox_reg_weights"] == (10.0, 10.0, 5.0, 5.0)
    dflt = _lib.LossOpts()
    _lib.check(_lib.lib().amp_loss_opts_default(C.byref(dflt)), "amp_loss_opts_default")
    assert _struct_dict(_lib.loss_opts(kw["loss"])) == _struct_dict(dflt)
    assert _struct_dict(dflt) == dict(rpn_loss_type=0, rpn_smooth_l1_beta=0.0, rpn_loss_weight=1.0, rpn_bbox_reg_loss_weight=1.0, box_loss_type=0,
                                      box_smooth_l1_beta=0.0, box_bbox_reg_loss_weight=1.0)
    tk = train_model_kwargs(_cfg(), 2)
    assert tk["loss"] == kw["loss"] and tk["bbox_reg_weights"] == kw["bbox_reg_weights"]
    # get_cfg() alone carries detectron2's defaults for the new keys
    from ampis_amd.config import get_cfg
    m = get_cfg().MODEL
    assert (m.RPN.LOSS_WEIGHT, m.RPN.BBOX_REG_LOSS_TYPE, m.RPN.BBOX_REG_LOSS_WEIGHT, m.RPN.SMOOTH_L1_BETA) == (1.0, "smooth_l1", 1.0, 0.0)
    assert tuple(m.RPN.BBOX_REG_WEIGHTS) == (1.0, 1.0, 1.0, 1.0)
    h = m.ROI_BOX_HEAD
    assert (h.SMOOTH_L1_BETA, h.BBOX_REG_LOSS_TYPE, h.BBOX_REG_LOSS_WEIGHT, h.CLS_AGNOSTIC_BBOX_REG, h.TRAIN_ON_PRED_BOXES) == \
        (0.0, "smooth_l1", 1.0, False, False)


def test_an_older_cfg_without_the_keys_gets_the_defaults():
    from ampis_amd.config import CfgNode
    from ampis_amd.engine.defaults import loss_kwargs
    old = CfgNode({"MODEL": {"RPN": {"BATCH_SIZE_PER_IMAGE": 256}, "ROI_BOX_HEAD": {"BBOX_REG_WEIGHTS": [10.0, 10.0, 5.0, 5.0]}}})
    assert loss_kwargs(old) == loss_kwargs(_cfg())
    assert loss_kwargs(CfgNode({"MODEL": {}})) == loss_kwargs(_cfg())


def test_non_default_keys_reach_the_constructor_keywords():
    from ampis_amd import _lib
    from ampis_amd.engine.defaults import train_model_kwargs
    cfg = _cfg()
    r, h = cfg.MODEL.RPN, cfg.MODEL.ROI_BOX_HEAD
    r.LOSS_WEIGHT, r.BBOX_REG_LOSS_TYPE, r.BBOX_REG_LOSS_WEIGHT, r.SMOOTH_L1_BETA = 0.5, "giou", 2.0, 1.0 / 9
    h.SMOOTH_L1_BETA, h.BBOX_REG_LOSS_TYPE, h.BBOX_REG_LOSS_WEIGHT, h.BBOX_REG_WEIGHTS = 0.5, "smooth_l1", 3, [5.0, 5.0, 2.5, 2.5]
    kw = train_model_kwargs(cfg, 1)
    assert kw["loss"] == dict(rpn_loss_type="giou", rpn_smooth_l1_beta=1.0 / 9, rpn_loss_weight=0.5, rpn_bbox_reg_loss_weight=2.0,
                              box_loss_type="smooth_l1", box_smooth_l1_beta=0.5, box_bbox_reg_loss_weight=3.0)
    assert kw["bbox_reg_weights"] == (5.0, 5.0, 2.5, 2.5)
    o = _lib.loss_opts(kw["loss"])
    F = lambda v: float(np.float32(v))
    assert _struct_dict(o) == dict(rpn_loss_type=_lib.BOXLOSS_GIOU, rpn_smooth_l1_beta=F(1.0 / 9), rpn_loss_weight=0.5, rpn_bbox_reg_loss_weight=2.0,
                                   box_loss_type=_lib.BOXLOSS_SMOOTH_L1, box_smooth_l1_beta=0.5, box_bbox_reg_loss_weight=3.0)
    # the constructor takes both keywords (signature only: no device here)
    import inspect
    from ampis_amd.model import MaskRCNN
    params = inspect.signature(MaskRCNN.__init__).parameters
    assert "loss" in params and "bbox_reg_weights" in params and params["loss"].default is None and params["bbox_reg_weights"].default is None


@pytest.mark.parametrize("section,key,value", [
    ("RPN", "BBOX_REG_LOSS_TYPE", "diou"), ("RPN", "BBOX_REG_LOSS_TYPE", "ciou"), ("RPN", "BBOX_REG_LOSS_TYPE", "l2"), ("RPN", "BBOX_REG_LOSS_TYPE", 1),
    ("ROI_BOX_HEAD", "BBOX_REG_LOSS_TYPE", "diou"), ("ROI_BOX_HEAD", "BBOX_REG_LOSS_TYPE", "ciou"), ("ROI_BOX_HEAD", "BBOX_REG_LOSS_TYPE", None),
    ("ROI_BOX_HEAD", "CLS_AGNOSTIC_BBOX_REG", True), ("ROI_BOX_HEAD", "TRAIN_ON_PRED_BOXES", True), ("ROI_BOX_HEAD", "CLS_AGNOSTIC_BBOX_REG", 0),
    ("RPN", "BBOX_REG_WEIGHTS", [1.0, 1.0, 2.0, 2.0]), ("RPN", "BBOX_REG_WEIGHTS", [1.0, 1.0, 1.0]), ("RPN", "BBOX_REG_WEIGHTS", [True, 1, 1, 1]),
    ("RPN", "LOSS_WEIGHT", True), ("RPN", "LOSS_WEIGHT", -1.0), ("RPN", "LOSS_WEIGHT", float("nan")), ("RPN", "LOSS_WEIGHT", "1.0"),
    ("RPN", "BBOX_REG_LOSS_WEIGHT", False), ("RPN", "BBOX_REG_LOSS_WEIGHT", float("inf")), ("RPN", "BBOX_REG_LOSS_WEIGHT", -0.5),
    ("RPN", "SMOOTH_L1_BETA", -0.1), ("RPN", "SMOOTH_L1_BETA", True), ("RPN", "SMOOTH_L1_BETA", float("nan")),
    ("ROI_BOX_HEAD", "SMOOTH_L1_BETA", -1), ("ROI_BOX_HEAD", "SMOOTH_L1_BETA", False), ("ROI_BOX_HEAD", "SMOOTH_L1_BETA", float("inf")),
    ("ROI_BOX_HEAD", "BBOX_REG_LOSS_WEIGHT", True), ("ROI_BOX_HEAD", "BBOX_REG_LOSS_WEIGHT", -2), ("ROI_BOX_HEAD", "BBOX_REG_LOSS_WEIGHT", None),
    ("ROI_BOX_HEAD", "BBOX_REG_WEIGHTS", [10.0, 10.0, 5.0]), ("ROI_BOX_HEAD", "BBOX_REG_WEIGHTS", [10.0, 10.0, 0.0, 5.0]),
    ("ROI_BOX_HEAD", "BBOX_REG_WEIGHTS", [10.0, True, 5.0, 5.0]), ("ROI_BOX_HEAD", "BBOX_REG_WEIGHTS", [10.0, 10.0, float("nan"), 5.0]),
    ("ROI_BOX_HEAD", "BBOX_REG_WEIGHTS", [10.0, 10.0, -5.0, 5.0]),
])
def test_unrepresentable_settings_are_refused_naming_the_key(section, key, value):
    from ampis_amd.engine.defaults import loss_kwargs, train_model_kwargs
    cfg = _cfg()
    setattr(getattr(cfg.MODEL, section), key, value)
    for fn in (loss_kwargs, lambda c: train_model_kwargs(c, 1)):
        with pytest.raises(ValueError, match=re.escape(f"MODEL.{section}.{key}")):
            fn(cfg)


def test_the_loss_dict_of_the_model_is_validated():
    from ampis_amd import _lib
    from ampis_amd.model import box_weights
    for bad in (dict(rpn_loss_type="diou"), dict(box_loss_type=2), dict(box_loss_type=True), dict(rpn_loss_weight=-1.0), dict(rpn_loss_weight=True),
                dict(box_smooth_l1_beta=float("nan")), dict(rpn_bbox_reg_loss_weight=float("inf")), dict(beta=1.0)):
        with pytest.raises(ValueError, match=re.escape(next(iter(bad)))):
            _lib.loss_opts(bad)
    assert _lib.loss_opts(dict(rpn_loss_type="GIoU", box_loss_type=1)).rpn_loss_type == _lib.BOXLOSS_GIOU
    assert box_weights([10, 10.0, np.float32(5), 5]) == (10.0, 10.0, 5.0, 5.0)
    for bad in ((10, 10, 5), "10,10,5,5", (10, 10, 5, 0), (10, 10, 5, float("inf")), (10, 10, 5, False)):
        with pytest.raises(ValueError, match="bbox_reg_weights"):
            box_weights(bad)


def _header_struct_fields(name):
    src = open(os.path.join(ROOT, "include", "ampis_hip.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            out += [(n.strip(), ctype) for n in names.split(",")]
    return out


def test_ctypes_loss_opts_mirrors_the_header():
    from ampis_amd import _lib
    hdr = _header_struct_fields("amp_loss_opts")
    assert [n for n, _ in hdr] == ["rpn_loss_type", "rpn_smooth_l1_beta", "rpn_loss_weight", "rpn_bbox_reg_loss_weight", "box_loss_type",
                                   "box_smooth_l1_beta", "box_bbox_reg_loss_weight"]
    assert [n for n, _ in _lib.LossOpts._fields_] == [n for n, _ in hdr]
    assert [t for _, t in _lib.LossOpts._fields_] == [{"int": C.c_int, "float": C.c_float}[t] for _, t in hdr]
    assert C.sizeof(_lib.LossOpts) == 4 * len(hdr) == 28
    assert [getattr(_lib.LossOpts, n).offset for n, _ in _lib.LossOpts._fields_] == [4 * i for i in range(len(hdr))]
    src = open(os.path.join(ROOT, "include", "ampis_hip.h")).read()
    vals = dict(re.findall(r"(AMP_BOXLOSS_[A-Z0-9_]+) = (\d)", src))
    assert (int(vals["AMP_BOXLOSS_SMOOTH_L1"]), int(vals["AMP_BOXLOSS_GIOU"])) == (_lib.BOXLOSS_SMOOTH_L1, _lib.BOXLOSS_GIOU) == (0, 1)
    # amp_model_cfg keeps its layout (tests/test_sampling_cfg.py mirrors it): the options live in a struct of their own
    assert "loss" not in " ".join(n for n, _ in _lib.ModelCfg._fields_)


def test_loss_opts_default_and_the_bound_symbols():
    """amp_loss_opts_default needs no device, writes every field and nothing past the struct; the header declares every new function _lib.py
    binds and the library exports it; the stage entry points refuse a bad option naming its field before they look at anything else."""
    from ampis_amd import _lib
    pad = 32
    size = C.sizeof(_lib.LossOpts)
    buf = (C.c_ubyte * (size + pad))(*([0xA5] * (size + pad)))
    o = _lib.LossOpts.from_buffer(buf)
    _lib.check(_lib.lib().amp_loss_opts_default(C.byref(o)), "amp_loss_opts_default")
    assert bytes(buf[size:]) == b"\xa5" * pad
    assert _struct_dict(o) == dict(rpn_loss_type=0, rpn_smooth_l1_beta=0.0, rpn_loss_weight=1.0, rpn_bbox_reg_loss_weight=1.0, box_loss_type=0,
                                   box_smooth_l1_beta=0.0, box_bbox_reg_loss_weight=1.0)
    src = open(os.path.join(ROOT, "include", "ampis_hip.h")).read()
    for name in ("amp_loss_opts_default", "amp_model_set_loss_opts", "amp_model_get_loss_opts", "amp_rpn_sample_loss_ex", "amp_box_loss_ex"):
        assert re.search(r"^int\s+%s\s*\(" % name, src, re.M), name
        assert name in _lib.lib()._amp_sig and hasattr(_lib.lib(), name), name
    for name in ("amp_rpn_sample_loss", "amp_box_loss"):          # the old entry points stay
        assert name in _lib.lib()._amp_sig and hasattr(_lib.lib(), name), name
    L = _lib.lib()
    for field, value in (("rpn_smooth_l1_beta", -1.0), ("rpn_loss_weight", float("nan")), ("rpn_bbox_reg_loss_weight", float("inf")),
                         ("box_smooth_l1_beta", float("nan")), ("box_bbox_reg_loss_weight", -0.5), ("rpn_loss_type", 2), ("box_loss_type", -1)):
        bad = _lib.LossOpts()
        L.amp_loss_opts_default(C.byref(bad))
        setattr(bad, field, value)
        for call in (lambda: L.amp_rpn_sample_loss_ex(None, None, None, 1, None, None, None, None, None, 256, 128, 0, None, None, None, C.byref(bad)),
                     lambda: L.amp_box_loss_ex(None, 1, 512, 1, None, 8, None, None, None, None, None, None, None, 0, None, C.byref(bad))):
            assert call() == -1                                 # AMP_ERR_ARG
            assert f"amp_loss_opts.{field}" in L.amp_last_error().decode(), (field, L.amp_last_error().decode())
    assert L.amp_model_set_loss_opts(None, C.byref(o)) == -1     # no model: refused, not a crash
