"""DefaultPredictor / DefaultTrainer façade over the C-ABI model (notebook cells 22-28).

DefaultPredictor(cfg)(img) follows detectron2's DefaultPredictor.__call__: BGR uint8 HxWx3 -> ResizeShortestEdge
(INPUT.MIN_SIZE_TEST / MAX_SIZE_TEST, PIL bilinear on uint8, exactly detectron2's CPU-side transform) -> the HIP hot path
(amp_model_infer) -> {'instances': Instances(image_size=(H, W), pred_boxes, scores, pred_classes, pred_masks)} rescaled to
the original image.  There is no CPU fallback: cfg.MODEL.DEVICE must name a HIP device.
"""
import logging
import os

import numpy as np
import torch

from .. import _lib, checkpoint, params as P
from ..model import MaskRCNN
from ..structures import Boxes, Instances, RLEBitMasks

logger = logging.getLogger("ampis_amd")


FPN_RPN_FEATURES = ("p2", "p3", "p4", "p5", "p6")
_anchor_warned = set()


def anchor_kwargs(cfg):
    """The MaskRCNN keyword arguments for MODEL.ANCHOR_GENERATOR: anchor_sizes / aspect_ratios, five lists each (detectron2's
    DefaultAnchorGenerator: one inner list is broadcast to p2..p6; offset 0; ANGLES belongs to rotated boxes and is ignored).  The keys
    are read only when MODEL.RPN.IN_FEATURES names the five FPN levels: a cfg without a zoo merge carries detectron2's C4 defaults (one
    level, five sizes), which this project has always replaced by the zoo's FPN architecture -- then {} (the FPN zoo anchors), with one
    logged warning.  Raises ValueError naming the cfg key for what the native path cannot represent, before any device work."""
    from ..model import anchor_lists
    feats = tuple(cfg.MODEL.RPN.get("IN_FEATURES", ()))
    if feats != FPN_RPN_FEATURES:
        if feats not in _anchor_warned:
            _anchor_warned.add(feats)
            logger.warning(f"MODEL.RPN.IN_FEATURES = {list(feats)!r} is not the FPN level set p2..p6: the model is the zoo's R-FPN architecture and "
                           "MODEL.ANCHOR_GENERATOR is not read (sizes 32..512, aspect ratios 0.5, 1, 2); merge a zoo config to set the anchors")
        return {}
    g = cfg.MODEL.get("ANCHOR_GENERATOR", None) or {}
    name = g.get("NAME", "DefaultAnchorGenerator")
    if name != "DefaultAnchorGenerator":
        raise ValueError(f"MODEL.ANCHOR_GENERATOR.NAME = {name!r}: only 'DefaultAnchorGenerator' has a native path")
    off = g.get("OFFSET", 0.0)
    if isinstance(off, bool) or not isinstance(off, (int, float, np.integer, np.floating)) or float(off) != 0.0:
        raise ValueError(f"MODEL.ANCHOR_GENERATOR.OFFSET = {off!r}: the native anchors sit at offset 0")
    unwrap = lambda v: [list(x) if isinstance(x, (list, tuple)) else x for x in v] if isinstance(v, (list, tuple)) else v
    sizes, ratios = anchor_lists(unwrap(g.get("SIZES", None)), unwrap(g.get("ASPECT_RATIOS", None)))
    return dict(anchor_sizes=[list(s) for s in sizes], aspect_ratios=[list(r) for r in ratios])


def _num_anchors(anchor_kw):
    """Anchors per location of anchor_kwargs' result ({} = the default 3)."""
    if not anchor_kw:
        return P.NUM_ANCHORS
    return len(anchor_kw["anchor_sizes"][0]) * len(anchor_kw["aspect_ratios"][0])


def train_model_kwargs(cfg, per_rank):
    """The MaskRCNN keyword arguments a training net takes from cfg (the trainer adds classes, capacity and backbone): batch size per
    rank, training top-k, pixel statistics, every sampling setting of MODEL.RPN / MODEL.ROI_HEADS, the anchors and the loss definition
    (loss_kwargs).  Refuses (ValueError naming the
    key) what the native sampler cannot represent, before any device work."""
    from ..model import sampling_caps
    r, h = cfg.MODEL.RPN, cfg.MODEL.ROI_HEADS
    seq = lambda v: tuple(v) if isinstance(v, (list, tuple)) else v
    kw = dict(max_batch=int(per_rank), train=True, max_gt=int(per_rank) * 2048, max_poly_doubles=int(per_rank) * 2048 * 128,
              pre_nms_topk_train=int(r.PRE_NMS_TOPK_TRAIN), post_nms_topk_train=int(r.POST_NMS_TOPK_TRAIN),
              pixel_mean=tuple(cfg.MODEL.PIXEL_MEAN), pixel_std=tuple(cfg.MODEL.PIXEL_STD),
              rpn_batch=r.BATCH_SIZE_PER_IMAGE, rpn_pos_frac=r.POSITIVE_FRACTION, rpn_iou=seq(r.IOU_THRESHOLDS),
              roi_batch=h.BATCH_SIZE_PER_IMAGE, roi_fg_frac=h.POSITIVE_FRACTION, roi_iou=seq(h.IOU_THRESHOLDS))
    sampling_caps(kw["rpn_batch"], kw["rpn_pos_frac"], kw["rpn_iou"], kw["roi_batch"], kw["roi_fg_frac"], kw["roi_iou"])
    kw.update(anchor_kwargs(cfg))
    kw.update(loss_kwargs(cfg))
    return kw


_SOLVER_DEFAULTS = {"NESTEROV": False, "BIAS_LR_FACTOR": 1.0, "WEIGHT_DECAY_BIAS": None, "LR_SCHEDULER_NAME": "WarmupMultiStepLR",
                    "WARMUP_METHOD": "linear"}
_CLIP_DEFAULTS = {"ENABLED": False, "CLIP_TYPE": "value", "CLIP_VALUE": 1.0, "NORM_TYPE": 2.0}


def _number(v, key):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v):
        raise ValueError(f"{key} = {v!r}: a finite number is required")
    return float(v)


def _positive(v, key):
    v = _number(v, key)
    if v <= 0:
        raise ValueError(f"{key} = {v!r}: must be positive")
    return v


def solver_kwargs(cfg):
    """The keyword arguments MaskRCNN.sgd_step takes from cfg.SOLVER beyond lr / MOMENTUM / WEIGHT_DECAY, as detectron2's build_optimizer
    reads them: NESTEROV, BIAS_LR_FACTOR and WEIGHT_DECAY_BIAS (None = WEIGHT_DECAY) for the tensors named *.bias, and CLIP_GRADIENTS
    (ENABLED, CLIP_TYPE "value" | "norm", CLIP_VALUE, NORM_TYPE 1 | 2 | inf; clipping is per parameter tensor, as in detectron2).  A
    cfg without these keys (a hand-built CfgNode) gets detectron2's defaults.  WEIGHT_DECAY_NORM is accepted and has no effect: every norm
    layer here is FrozenBN and has no trainable parameter.  Raises ValueError naming the cfg key for what the native step cannot
    represent, before any device work."""
    s = cfg.SOLVER
    get = lambda k: s.get(k, _SOLVER_DEFAULTS[k])
    nesterov = get("NESTEROV")
    if not isinstance(nesterov, (bool, np.bool_)):
        raise ValueError(f"SOLVER.NESTEROV = {nesterov!r}: True or False is required")
    blf = _number(get("BIAS_LR_FACTOR"), "SOLVER.BIAS_LR_FACTOR")
    if blf < 0:
        raise ValueError(f"SOLVER.BIAS_LR_FACTOR = {blf!r}: must not be negative")
    wdb = get("WEIGHT_DECAY_BIAS")
    wdb = None if wdb is None else _number(wdb, "SOLVER.WEIGHT_DECAY_BIAS")
    kw = dict(nesterov=bool(nesterov), bias_lr_factor=blf, weight_decay_bias=wdb, clip=None)
    c = s.get("CLIP_GRADIENTS", None) or {}
    cget = lambda k: c.get(k, _CLIP_DEFAULTS[k])
    enabled = cget("ENABLED")
    if not isinstance(enabled, (bool, np.bool_)):
        raise ValueError(f"SOLVER.CLIP_GRADIENTS.ENABLED = {enabled!r}: True or False is required")
    if enabled:
        kind = cget("CLIP_TYPE")
        if not isinstance(kind, str) or kind.lower() not in ("value", "norm"):
            raise ValueError(f"SOLVER.CLIP_GRADIENTS.CLIP_TYPE = {kind!r}: 'value' or 'norm' (per-parameter clipping, as detectron2 core)")
        value = _positive(cget("CLIP_VALUE"), "SOLVER.CLIP_GRADIENTS.CLIP_VALUE")
        if kind.lower() == "value":
            kw["clip"] = ("value", value)
        else:
            nt = cget("NORM_TYPE")
            if isinstance(nt, str) and nt.lower() in ("inf", "+inf", "infinity"):
                nt = float("inf")
            if isinstance(nt, bool) or not isinstance(nt, (int, float, np.integer, np.floating)) or float(nt) not in (1.0, 2.0, float("inf")):
                raise ValueError(f"SOLVER.CLIP_GRADIENTS.NORM_TYPE = {nt!r}: 1, 2 or inf")
            kw["clip"] = ("norm", value, float(nt))
    return kw


_RPN_LOSS_DEFAULTS = {"LOSS_WEIGHT": 1.0, "BBOX_REG_LOSS_TYPE": "smooth_l1", "BBOX_REG_LOSS_WEIGHT": 1.0, "SMOOTH_L1_BETA": 0.0,
                      "BBOX_REG_WEIGHTS": (1.0, 1.0, 1.0, 1.0)}
_BOX_LOSS_DEFAULTS = {"SMOOTH_L1_BETA": 0.0, "BBOX_REG_LOSS_TYPE": "smooth_l1", "BBOX_REG_LOSS_WEIGHT": 1.0, "CLS_AGNOSTIC_BBOX_REG": False,
                      "TRAIN_ON_PRED_BOXES": False, "BBOX_REG_WEIGHTS": (10.0, 10.0, 5.0, 5.0)}


def box_head_weights(cfg):
    """MODEL.ROI_BOX_HEAD.BBOX_REG_WEIGHTS as the `bbox_reg_weights=` keyword of MaskRCNN (the predictor and the trainer both read it): four
    positive finite numbers, ValueError naming the key otherwise."""
    from ..model import box_weights
    v = (cfg.MODEL.get("ROI_BOX_HEAD", None) or {}).get("BBOX_REG_WEIGHTS", _BOX_LOSS_DEFAULTS["BBOX_REG_WEIGHTS"])
    return box_weights(tuple(v) if isinstance(v, (list, tuple)) else v, "MODEL.ROI_BOX_HEAD.BBOX_REG_WEIGHTS")


def loss_kwargs(cfg):
    """The MaskRCNN keyword arguments for the loss definition of MODEL.RPN and MODEL.ROI_BOX_HEAD as detectron2's RPN.from_config and
    FastRCNNOutputLayers.from_config read it: dict(loss={the fields of amp_loss_opts}, bbox_reg_weights=(wx, wy, ww, wh)).
    BBOX_REG_LOSS_TYPE "smooth_l1" (with SMOOTH_L1_BETA; 0 = L1) or "giou" on either head; loss_rpn_cls carries RPN.LOSS_WEIGHT,
    loss_rpn_loc RPN.LOSS_WEIGHT x RPN.BBOX_REG_LOSS_WEIGHT, loss_box_reg ROI_BOX_HEAD.BBOX_REG_LOSS_WEIGHT.  A cfg without these keys (an
    older yaml, a hand-built CfgNode) gets detectron2's defaults: the losses this project has always computed.  Raises ValueError naming
    the cfg key for what the native losses cannot represent -- "diou" / "ciou", CLS_AGNOSTIC_BBOX_REG, TRAIN_ON_PRED_BOXES, RPN box
    weights other than ones (they also enter the proposal decoding) -- before any device work."""
    r = cfg.MODEL.get("RPN", None) or {}
    h = cfg.MODEL.get("ROI_BOX_HEAD", None) or {}
    rget = lambda k: r.get(k, _RPN_LOSS_DEFAULTS[k])
    hget = lambda k: h.get(k, _BOX_LOSS_DEFAULTS[k])

    def weight(v, key):
        v = _number(v, key)
        if v < 0:
            raise ValueError(f"{key} = {v!r}: must not be negative")
        return v

    def kind(v, key):
        if not isinstance(v, str) or v not in _lib.BOXLOSS_TYPES:
            raise ValueError(f"{key} = {v!r}: 'smooth_l1' or 'giou' have a native path")
        return v

    for k in ("CLS_AGNOSTIC_BBOX_REG", "TRAIN_ON_PRED_BOXES"):
        v = hget(k)
        if not isinstance(v, (bool, np.bool_)):
            raise ValueError(f"MODEL.ROI_BOX_HEAD.{k} = {v!r}: True or False is required")
        if v:
            raise ValueError(f"MODEL.ROI_BOX_HEAD.{k} = True has no native path (False only)")
    rw = rget("BBOX_REG_WEIGHTS")
    if isinstance(rw, (str, bytes)) or not hasattr(rw, "__len__") or len(rw) != 4 or \
            any(isinstance(x, bool) or not isinstance(x, (int, float, np.integer, np.floating)) or float(x) != 1.0 for x in rw):
        raise ValueError(f"MODEL.RPN.BBOX_REG_WEIGHTS = {rw!r}: the native RPN decodes and regresses with (1, 1, 1, 1)")
    loss = dict(rpn_loss_type=kind(rget("BBOX_REG_LOSS_TYPE"), "MODEL.RPN.BBOX_REG_LOSS_TYPE"),
                rpn_smooth_l1_beta=weight(rget("SMOOTH_L1_BETA"), "MODEL.RPN.SMOOTH_L1_BETA"),
                rpn_loss_weight=weight(rget("LOSS_WEIGHT"), "MODEL.RPN.LOSS_WEIGHT"),
                rpn_bbox_reg_loss_weight=weight(rget("BBOX_REG_LOSS_WEIGHT"), "MODEL.RPN.BBOX_REG_LOSS_WEIGHT"),
                box_loss_type=kind(hget("BBOX_REG_LOSS_TYPE"), "MODEL.ROI_BOX_HEAD.BBOX_REG_LOSS_TYPE"),
                box_smooth_l1_beta=weight(hget("SMOOTH_L1_BETA"), "MODEL.ROI_BOX_HEAD.SMOOTH_L1_BETA"),
                box_bbox_reg_loss_weight=weight(hget("BBOX_REG_LOSS_WEIGHT"), "MODEL.ROI_BOX_HEAD.BBOX_REG_LOSS_WEIGHT"))
    return dict(loss=loss, bbox_reg_weights=box_head_weights(cfg))


_CROP_DEFAULTS = {"ENABLED": False, "TYPE": "relative_range", "SIZE": [0.9, 0.9]}
_CROP_TYPES = ("relative_range", "relative", "absolute", "absolute_range")


def input_kwargs(cfg):
    """The train-time augmentations of cfg.INPUT as detectron2's DatasetMapper.from_config reads them for a Mask R-CNN config:
    dict(sizes, sampling "choice" | "range", flip "horizontal" | "vertical" | "none", crop None | (TYPE, (s0, s1)) with SIZE as (h, w),
    recompute_boxes = crop enabled: a mask head is always present here).  A cfg without these keys (a hand-built CfgNode) gets detectron2's
    defaults.  Raises ValueError naming the cfg key for what the mapper cannot honour, before any device work."""
    c = cfg.INPUT
    sizes = c.MIN_SIZE_TRAIN
    sizes = (int(sizes),) if isinstance(sizes, (int, np.integer)) else tuple(int(v) for v in sizes)
    sampling = c.get("MIN_SIZE_TRAIN_SAMPLING", "choice")
    if sampling not in ("choice", "range"):
        raise ValueError(f"INPUT.MIN_SIZE_TRAIN_SAMPLING = {sampling!r}: 'choice' or 'range'")
    if sampling == "range" and (len(sizes) != 2 or sizes[0] > sizes[1]):
        raise ValueError(f"INPUT.MIN_SIZE_TRAIN = {sizes!r}: exactly two values (min, max) are required with INPUT.MIN_SIZE_TRAIN_SAMPLING = 'range'")
    if len(sizes) == 0:
        raise ValueError("INPUT.MIN_SIZE_TRAIN = (): at least one size is required")
    flip = c.get("RANDOM_FLIP", "horizontal")
    if flip not in ("horizontal", "vertical", "none"):
        raise ValueError(f"INPUT.RANDOM_FLIP = {flip!r}: 'horizontal', 'vertical' or 'none'")
    cr = c.get("CROP", None) or {}
    cget = lambda k: cr.get(k, _CROP_DEFAULTS[k])
    enabled = cget("ENABLED")
    if not isinstance(enabled, (bool, np.bool_)):
        raise ValueError(f"INPUT.CROP.ENABLED = {enabled!r}: True or False is required")
    crop = None
    if enabled:
        kind = cget("TYPE")
        if kind not in _CROP_TYPES:
            raise ValueError(f"INPUT.CROP.TYPE = {kind!r}: one of {', '.join(_CROP_TYPES)}")
        size = cget("SIZE")
        if not isinstance(size, (list, tuple)) or len(size) != 2:
            raise ValueError(f"INPUT.CROP.SIZE = {size!r}: two numbers (h, w) are required")
        s0, s1 = (_positive(v, "INPUT.CROP.SIZE") for v in size)
        if kind.startswith("relative") and (s0 > 1 or s1 > 1):
            raise ValueError(f"INPUT.CROP.SIZE = {size!r}: a relative size lies in (0, 1]")
        if kind.startswith("absolute"):
            if s0 != int(s0) or s1 != int(s1):
                raise ValueError(f"INPUT.CROP.SIZE = {size!r}: an absolute size is a whole number of pixels")
            s0, s1 = int(s0), int(s1)
        if kind == "absolute_range" and s0 > s1:
            raise ValueError(f"INPUT.CROP.SIZE = {size!r}: INPUT.CROP.TYPE = 'absolute_range' draws both extents from [SIZE[0], SIZE[1]], so SIZE[0] <= SIZE[1]")
        crop = (kind, (s0, s1))
    return dict(sizes=sizes, sampling=sampling, flip=flip, crop=crop, recompute_boxes=crop is not None)


def crop_extent_bounds(crop, h, w):
    """((ch_min, ch_max), (cw_min, cw_max)) of the windows `crop_window` can return on an h x w image."""
    kind, (s0, s1) = crop
    clamp = lambda v, n: max(1, min(int(v), n))
    if kind == "relative":
        a = clamp(h * s0 + 0.5, h), clamp(w * s1 + 0.5, w)
        return (a[0], a[0]), (a[1], a[1])
    if kind == "relative_range":
        return (clamp(h * s0 + 0.5, h), h), (clamp(w * s1 + 0.5, w), w)
    if kind == "absolute":
        return (min(s0, h), min(s0, h)), (min(s1, w), min(s1, w))
    return (min(h, s0), min(h, s1)), (min(w, s0), min(w, s1))


def crop_window(crop, h, w, u):
    """detectron2 RandomCrop.get_crop_size + get_transform on an h x w image, from four uniform numbers u in [0, 1) (drawn by
    DatasetMapper.draw: extent h, extent w, origin y, origin x): the window (y0, x0, ch, cw).
      relative: int(h * s0 + 0.5), int(w * s1 + 0.5) | relative_range: the same with s = SIZE + u * (1 - SIZE) | absolute: min(s0, h), min(s1, w)
      | absolute_range: uniform integers in [min(h, s0), min(h, s1)] and [min(w, s0), min(w, s1)]; the origin is a uniform integer in
    [0, h - ch] x [0, w - cw]."""
    kind, (s0, s1) = crop
    (hlo, hhi), (wlo, whi) = crop_extent_bounds(crop, h, w)
    pick = lambda u_, n: min(int(u_ * n), n - 1)          # a uniform integer in [0, n)
    if kind == "relative_range":
        ch = max(1, min(int(h * (s0 + u[0] * (1.0 - s0)) + 0.5), h))
        cw = max(1, min(int(w * (s1 + u[1] * (1.0 - s1)) + 0.5), w))
    else:
        ch, cw = hlo + pick(u[0], hhi - hlo + 1), wlo + pick(u[1], whi - wlo + 1)
    return pick(u[2], h - ch + 1), pick(u[3], w - cw + 1), ch, cw


def read_image_bgr(path):
    """cv2.imread stand-in (notebook cells 26/28): 8-bit image -> HxWx3 BGR uint8 (grayscale replicated)."""
    from PIL import Image
    im = Image.open(str(path))
    im = im.convert("RGB")
    return np.ascontiguousarray(np.asarray(im)[:, :, ::-1])


def resize_shortest_edge(img, min_size, max_size):
    """detectron2 ResizeShortestEdge.get_transform + ResizeTransform.apply_image (PIL bilinear on uint8)."""
    h, w = img.shape[:2]
    if min_size == 0:
        return img
    scale = min_size * 1.0 / min(h, w)
    newh, neww = (min_size, scale * w) if h < w else (scale * h, min_size)
    if max(newh, neww) > max_size:
        s = max_size * 1.0 / max(newh, neww)
        newh, neww = newh * s, neww * s
    neww, newh = int(neww + 0.5), int(newh + 0.5)
    if (newh, neww) == (h, w):
        return img
    from PIL import Image
    return np.asarray(Image.fromarray(img).resize((neww, newh), Image.BILINEAR))


def shortest_edge_size(h, w, min_size, max_size):
    """Output size of detectron2 ResizeShortestEdge.get_transform (same rounding)."""
    if min_size == 0:
        return h, w
    scale = min_size * 1.0 / min(h, w)
    newh, neww = (min_size, scale * w) if h < w else (scale * h, min_size)
    if max(newh, neww) > max_size:
        s = max_size * 1.0 / max(newh, neww)
        newh, neww = newh * s, neww * s
    return int(newh + 0.5), int(neww + 0.5)


def device_resize_shortest_edge(ctx, img, min_size, max_size, bufs):
    """Upload `img` (uint8 HxWx3) and resize it on the device with the PIL-exact kernel.  Returns (device pointer of the network
    input, (h, w), bufs); `bufs` caches the device buffers between calls."""
    import ctypes as C
    img = np.ascontiguousarray(img, dtype=np.uint8)
    H, W = img.shape[:2]
    h, w = shortest_edge_size(H, W, min_size, max_size)
    need = {"src": img.nbytes, "dst": h * w * 3, "tmp": int(_lib.lib().amp_resize_scratch_bytes(H, W, h, w))}
    for k, n in need.items():
        if bufs.get(k + "_n", 0) < n:
            if bufs.get(k):
                _lib.check(_lib.lib().amp_free(ctx.handle, C.c_void_p(bufs[k])), "amp_free")
            bufs[k] = ctx.malloc(n)
            bufs[k + "_n"] = n
    ctx.h2d(bufs["src"], img)
    if (h, w) == (H, W):
        return bufs["src"], (h, w), bufs
    _lib.check(_lib.lib().amp_resize_bilinear_u8(ctx.handle, C.c_void_p(bufs["src"]), H, W, C.c_void_p(bufs["dst"]), h, w, C.c_void_p(bufs["tmp"])),
               "amp_resize_bilinear_u8")
    return bufs["dst"], (h, w), bufs


def _device_index(dev):
    dev = str(dev)
    if dev.startswith("cpu"):
        raise _lib.AmpError("cfg.MODEL.DEVICE='cpu': ampis_amd has no CPU path for the Mask R-CNN hot path "
                            "(the CPU restatement under oracle/ is test infrastructure only)")
    return int(dev.split(":")[1]) if ":" in dev else 0


class DefaultPredictor:
    def __init__(self, cfg):
        self.cfg = cfg.clone()
        if len(cfg.DATASETS.TEST) == 0:
            logger.warning("cfg.DATASETS.TEST is empty")
        assert cfg.INPUT.FORMAT in ("RGB", "BGR"), cfg.INPUT.FORMAT
        self.input_format = cfg.INPUT.FORMAT
        self.num_classes = int(cfg.MODEL.ROI_HEADS.NUM_CLASSES)
        self.ctx = _lib.Context(_device_index(cfg.MODEL.DEVICE))
        w = str(cfg.MODEL.WEIGHTS)
        self.arch = P.arch_from_cfg(cfg)
        self._anchor_kw = anchor_kwargs(cfg)               # an anchor setting the native path cannot represent fails here, naming its key
        self.num_anchors = _num_anchors(self._anchor_kw)
        self._box_weights = box_head_weights(cfg)          # MODEL.ROI_BOX_HEAD.BBOX_REG_WEIGHTS decodes the detections
        if w:
            self.params = checkpoint.load_checkpoint(w, self.num_classes, self.arch, num_anchors=self.num_anchors)
        else:
            logger.warning("cfg.MODEL.WEIGHTS is empty: using seeded random initialisation (like an un-loaded detectron2 model)")
            self.params = P.init_params(self.num_classes, seed=0, style="d2", arch=self.arch, num_anchors=self.num_anchors)
        self._model = None
        self._cap = (0, 0, 0)

    def _ensure(self, h, w, out_hw):
        hp, wp = (h + 31) // 32 * 32, (w + 31) // 32 * 32
        if self._model is None or hp > self._cap[0] or wp > self._cap[1] or out_hw > self._cap[2]:
            if self._model is not None:
                self._model.close()
            c = self.cfg
            cap = (max(hp, self._cap[0]), max(wp, self._cap[1]), max(out_hw, self._cap[2], 64))
            self._model = MaskRCNN(self.ctx, self.num_classes, max_batch=1, max_h=cap[0], max_w=cap[1], max_out_hw=cap[2],
                                   detections_per_image=int(c.TEST.DETECTIONS_PER_IMAGE),
                                   pre_nms_topk=int(c.MODEL.RPN.PRE_NMS_TOPK_TEST), post_nms_topk=int(c.MODEL.RPN.POST_NMS_TOPK_TEST),
                                   rpn_nms_thresh=float(c.MODEL.RPN.NMS_THRESH), score_thresh=float(c.MODEL.ROI_HEADS.SCORE_THRESH_TEST),
                                   nms_thresh=float(c.MODEL.ROI_HEADS.NMS_THRESH_TEST), pixel_mean=tuple(c.MODEL.PIXEL_MEAN),
                                   pixel_std=tuple(c.MODEL.PIXEL_STD), arch=self.arch, bbox_reg_weights=self._box_weights, **self._anchor_kw)
            self._model.load_params(self.params)
            self._cap = cap
        return self._model

    def __call__(self, original_image):
        original_image = np.asarray(original_image)
        assert original_image.ndim == 3 and original_image.shape[2] == 3 and original_image.dtype == np.uint8, \
            "DefaultPredictor expects an HxWx3 uint8 image"
        if self.input_format == "RGB":
            original_image = original_image[:, :, ::-1]
        height, width = original_image.shape[:2]
        # ResizeShortestEdge on the device (PIL-exact bilinear, amp_resize_bilinear_u8): the image goes up once, as uint8
        dptr, (h, w), self._bufs = device_resize_shortest_edge(self.ctx, original_image, int(self.cfg.INPUT.MIN_SIZE_TEST),
                                                               int(self.cfg.INPUT.MAX_SIZE_TEST), getattr(self, "_bufs", {}))
        model = self._ensure(h, w, max(height, width))
        r = model.infer(device_ptr=dptr, shape=(1, h, w), out_sizes=[(height, width)])[0]
        inst = Instances((height, width))
        inst.pred_boxes = Boxes(torch.from_numpy(r["boxes"]))
        inst.scores = torch.from_numpy(r["scores"])
        inst.pred_classes = torch.from_numpy(r["classes"])
        inst.pred_masks = RLEBitMasks(r["masks"], (height, width))
        return {"instances": inst}


    def close(self):
        """Free the device side of the predictor (model, the stream() lanes, context)."""
        if getattr(self, "_pipe", None) is not None:
            self._pipe.close()
            self._pipe = None
            self._pipe_key = None
        if self._model is not None:
            self._model.close()
            self._model = None
        if self.ctx is not None:
            self.ctx.close()
            self.ctx = None

    def _model_kwargs(self):
        c = self.cfg
        return dict(detections_per_image=int(c.TEST.DETECTIONS_PER_IMAGE), pre_nms_topk=int(c.MODEL.RPN.PRE_NMS_TOPK_TEST),
                    post_nms_topk=int(c.MODEL.RPN.POST_NMS_TOPK_TEST), rpn_nms_thresh=float(c.MODEL.RPN.NMS_THRESH),
                    score_thresh=float(c.MODEL.ROI_HEADS.SCORE_THRESH_TEST), nms_thresh=float(c.MODEL.ROI_HEADS.NMS_THRESH_TEST),
                    pixel_mean=tuple(c.MODEL.PIXEL_MEAN), pixel_std=tuple(c.MODEL.PIXEL_STD), arch=self.arch, bbox_reg_weights=self._box_weights,
                    **self._anchor_kw)

    def stream(self, images, depth=2):
        """`predictor(img)` for every image of an iterable, with `depth` images in flight on the GPU (amp_pipeline: the next image's
        convolutions run while the previous one is in its selection / NMS / paste tail and its results travel to the host).  Yields
        the same dicts `__call__` returns, in order, bit for bit (ResizeShortestEdge here is the PIL resize the device kernel reproduces
        exactly).  The lanes are sized for the largest frame cfg.INPUT.{MIN,MAX}_SIZE_TEST allows and kept for later calls."""
        from ..model import InferPipeline
        c = self.cfg
        mx = (int(c.INPUT.MAX_SIZE_TEST) + 31) // 32 * 32
        key = (int(depth), mx)
        if getattr(self, "_pipe_key", None) != key:
            if getattr(self, "_pipe", None) is not None:
                self._pipe.close()
            self._pipe = InferPipeline(self.ctx.device if hasattr(self.ctx, "device") else _device_index(c.MODEL.DEVICE), self.num_classes, depth=int(depth),
                                       max_batch=1, max_h=mx, max_w=mx, max_out_hw=4096, **self._model_kwargs())
            self._pipe.load_params(self.params)
            self._pipe_key = key
        pipe = self._pipe
        pending = []

        def finish(entry):
            ticket, (height, width) = entry
            r = pipe.wait(ticket)[0]
            inst = Instances((height, width))
            inst.pred_boxes = Boxes(torch.from_numpy(r["boxes"]))
            inst.scores = torch.from_numpy(r["scores"])
            inst.pred_classes = torch.from_numpy(r["classes"])
            inst.pred_masks = RLEBitMasks(r["masks"], (height, width))
            return {"instances": inst}

        for original_image in images:
            original_image = np.asarray(original_image)
            assert original_image.ndim == 3 and original_image.shape[2] == 3 and original_image.dtype == np.uint8, \
                "DefaultPredictor expects HxWx3 uint8 images"
            if self.input_format == "RGB":
                original_image = original_image[:, :, ::-1]
            height, width = original_image.shape[:2]
            small = resize_shortest_edge(np.ascontiguousarray(original_image), int(c.INPUT.MIN_SIZE_TEST), int(c.INPUT.MAX_SIZE_TEST))
            if len(pending) == pipe.depth:
                yield finish(pending.pop(0))
            pending.append((pipe.submit(small[None], out_sizes=[(height, width)]), (height, width)))
        while pending:
            yield finish(pending.pop(0))


class TrainModel:
    """What `trainer.model` is: callable on a batch (list of mapped dicts).  In training mode (the default, and what
    LossEvalHook relies on: ampis/data_utils.py:116) it returns the dict of the five losses as floats."""

    def __init__(self, net, ctx, ensure=None):
        self.net, self.ctx = net, ctx
        self.training = True
        self._seed = 0
        self._ensure = ensure          # callable (h, w): makes sure `net` exists and can take a batch of that frame (DefaultTrainer._ensure_net)

    def train(self, mode=True):
        self.training = mode
        return self

    def eval(self):
        return self.train(False)

    @staticmethod
    def stack(batch):
        from ..data import mapped_hw
        if all("device_plan" in d for d in batch):      # deferred: the uploader builds the frame on the device (no host copy of 3 MB per image)
            hw = [mapped_hw(d) for d in batch]
            H, W = max(h for h, _ in hw), max(w for _, w in hw)
            return None, (None if all(h == H and w == W for h, w in hw) else hw)
        assert not any("device_plan" in d for d in batch), "a batch mixes deferred and host-resized images"
        hs = [d["image_bgr"].shape[0] for d in batch]
        ws = [d["image_bgr"].shape[1] for d in batch]
        H, W = max(hs), max(ws)
        imgs = np.zeros((len(batch), H, W, 3), dtype=np.uint8)
        for i, d in enumerate(batch):
            imgs[i, : hs[i], : ws[i]] = d["image_bgr"]
        sizes = None if (min(hs) == H and min(ws) == W) else list(zip(hs, ws))
        return imgs, sizes

    @staticmethod
    def collate(batch):
        """Common frame + per-image sizes + flattened annotations of a batch (what the C ABI takes).  The train loader does this in
        its worker threads and leaves the result on the batch (`CollatedBatch.collated`); `__call__` does it itself otherwise."""
        from ..model import PackedGt
        imgs, sizes = TrainModel.stack(batch)
        return imgs, sizes, PackedGt([d["gt"] for d in batch])

    def __call__(self, batch, backward=False, seed=None):
        assert self.training, "TrainModel is the training-mode surface; use DefaultPredictor for inference"
        imgs, sizes, gt = getattr(batch, "collated", None) or self.collate(batch)
        dev = getattr(batch, "device", None)          # the loader's collating thread has put the frame into HBM already (_Uploader)
        assert imgs is not None or dev is not None, "a deferred batch (device_plan) needs the loader's uploader"
        if self._ensure is not None:   # a validation batch (LossEvalHook, ampis/data_utils.py:116) may be larger than every training batch so far
            self._ensure(*(dev[1][1:] if imgs is None else imgs.shape[1:3]))
        self.net.set_image_sizes(sizes)
        if seed is None:
            self._seed += 1
            seed = 0x5EED0000 + self._seed
        if dev is not None:
            return self.net.forward_losses(None, gt, seed=seed, backward=backward, device_ptr=dev[0], shape=dev[1])
        return self.net.forward_losses(imgs, gt, seed=seed, backward=backward)


class _Uploader:
    """H2D of the next batches off the training thread: a context of its own (its own HIP stream, non-blocking) and a ring of device
    buffers; the train loader's collating thread calls it, the training thread passes the pointer to amp_model_forward_backward.
    The copy is complete (stream-synchronised) when __call__ returns, so the compute stream needs no event.  A buffer is re-used after
    `nbuf` batches: the loader holds at most PREFETCH_DEPTH finished batches plus the one being collated, the trainer one."""

    device_resize = True      # the train loader defers ResizeShortestEdge + flip + stacking to `frames` (AMP_HOST_TRAIN_INPUT=1: the host path)

    def __init__(self, device, nbuf):
        import threading
        self.ctx = _lib.Context(device)
        self.bufs = [(0, 0)] * nbuf       # (pointer, bytes)
        self.k = 0
        self._lock = threading.Lock()     # close() may come from the training thread while the collating thread is uploading
        self._stage = {}                  # "src" / "tmp": device staging of one decoded image and the resize scratch
        if os.environ.get("AMP_HOST_TRAIN_INPUT"):
            self.device_resize = False

    def _scratch(self, key, nbytes):
        ptr, cap = self._stage.get(key, (0, 0))
        if cap < nbytes:
            if ptr:
                self.ctx.free(ptr)
            ptr, cap = self.ctx.malloc(nbytes), nbytes
            self._stage[key] = (ptr, cap)
        return ptr

    def frames(self, batch):
        """The stacked frame of a deferred batch, built in HBM: every decoded image goes up once as it is (under a crop: the rows of its
        window), amp_crop_resize_flip_u8 (window + PIL-exact resize + mirrors) writes it into its slot of the zeroed frame -- what DatasetMapper +
        ImageList.from_tensors do on the host, byte for byte (tests/test_train_input_gpu.py, tests/test_input_aug_gpu.py).  An image that needs
        neither crop, resize nor flip and fills the frame is copied straight into it."""
        import ctypes as C
        from ..data import mapped_hw
        hw = [mapped_hw(d) for d in batch]
        B, H, W = len(batch), max(h for h, _ in hw), max(w for _, w in hw)
        nbytes = B * H * W * 3
        with self._lock:
            if self.ctx is None:
                return None
            ptr, cap = self.bufs[self.k]
            if cap < nbytes:
                if ptr:
                    self.ctx.free(ptr)
                ptr, cap = self.ctx.malloc(nbytes), nbytes
                self.bufs[self.k] = (ptr, cap)
            L = _lib.lib()
            if any((h, w) != (H, W) for h, w in hw):
                _lib.check(L.amp_memset(self.ctx.handle, C.c_void_p(ptr), 0, nbytes), "amp_memset")       # the padding of the smaller images
            for b, d in enumerate(batch):
                img = np.ascontiguousarray(d["image_bgr"], dtype=np.uint8)
                w0 = img.shape[1]
                plan = d["device_plan"]
                (h, w), bits = hw[b], int(plan[2])                            # bit 0 left-right, bit 1 up-down (a plain bool: left-right)
                y0, x0, ch, cw = plan[3:7] if len(plan) > 3 else (0, 0) + img.shape[:2]
                assert 0 <= y0 <= img.shape[0] - ch and 0 <= x0 <= w0 - cw and ch > 0 and cw > 0, f"crop window {plan[3:7]} leaves the {img.shape[:2]} image"
                rows = img[y0:y0 + ch]                                        # whole rows of the window: contiguous, pitch w0
                slot = ptr + b * H * W * 3
                if (h, w) == (ch, cw) and not bits and w == W and cw == w0:
                    self.ctx.h2d(slot, rows)                                  # rows contiguous in the slot: no kernel
                    continue
                src = self._scratch("src", rows.nbytes)
                self.ctx.h2d(src, rows)
                tmp = self._scratch("tmp", int(L.amp_resize_scratch_bytes(ch, cw, h, w))) if (h, w) != (ch, cw) else 0
                _lib.check(L.amp_crop_resize_flip_u8(self.ctx.handle, C.c_void_p(src + 3 * x0), w0, ch, cw, C.c_void_p(slot), W, h, w, bits,
                                                     C.c_void_p(tmp) if tmp else None), "amp_crop_resize_flip_u8")
                self.ctx.sync()                                               # `src` is re-used by the next image
            self.ctx.sync()
            self.k = (self.k + 1) % len(self.bufs)
            return ptr, (B, H, W)

    def __call__(self, imgs):
        imgs = np.ascontiguousarray(imgs, dtype=np.uint8)
        with self._lock:
            if self.ctx is None:          # closed: the batch stays on the host (nobody will consume it)
                return None
            ptr, cap = self.bufs[self.k]
            if cap < imgs.nbytes:
                if ptr:
                    self.ctx.free(ptr)
                ptr, cap = self.ctx.malloc(imgs.nbytes), imgs.nbytes
                self.bufs[self.k] = (ptr, cap)
            self.ctx.h2d(ptr, imgs)           # returns when the bytes are in HBM
            self.k = (self.k + 1) % len(self.bufs)
            return ptr, tuple(int(v) for v in imgs.shape[:3])

    def close(self):
        with self._lock:
            if self.ctx is None:
                return
            for ptr, _ in list(self.bufs) + list(self._stage.values()):
                if ptr:
                    self.ctx.free(ptr)
            self.bufs, self._stage = [], {}
            self.ctx.close()
            self.ctx = None


def comm_backend_is_rccl():
    from ..utils import comm
    return comm.backend() == "rccl"


class DefaultTrainer:
    """detectron2's DefaultTrainer surface (notebook cell 22; subclassed by AmpisTrainer, ampis/data_utils.py:135-177):
    DefaultTrainer(cfg) -> .resume_or_load(resume=False) -> .train(); .model, .cfg, .iter, .max_iter, .storage, build_hooks().
    One process per GPU (engine.launch starts them); with torch.distributed initialised each rank trains on its shard of the
    global batch, and the gradient arena is all-reduced bucket by bucket over RCCL while the backward pass is still running
    (utils/comm.py; torch.distributed only hands the RCCL id to the ranks)."""

    def __init__(self, cfg):
        from ..data import build_detection_train_loader
        from ..utils import comm
        self.cfg = cfg
        input_kwargs(cfg)                    # an INPUT augmentation the mapper cannot honour fails here, naming its key, before the device is touched
        self.iter = self.start_iter = 0
        self.max_iter = int(cfg.SOLVER.MAX_ITER)
        self.storage = None
        self.is_main_process = comm.is_main_process()
        self.world_size = comm.get_world_size()
        self.num_classes = int(cfg.MODEL.ROI_HEADS.NUM_CLASSES)
        dev = _device_index(cfg.MODEL.DEVICE) if ":" in str(cfg.MODEL.DEVICE) else (int(os.environ.get("LOCAL_RANK", "0")) if not str(cfg.MODEL.DEVICE).startswith("cpu") else _device_index(cfg.MODEL.DEVICE))
        self.ctx = _lib.Context(dev)
        if self.world_size > 1 and comm.backend() == "rccl":
            comm.attach_rccl(self.ctx)       # the gradient exchange and synchronize() run on RCCL inside the library from here on
        self.arch = P.arch_from_cfg(cfg)     # a grouped (ResNeXt) backbone is inference-only: amp_model_create refuses to train it
        self.num_anchors = _num_anchors(anchor_kwargs(cfg))      # an anchor setting the native path cannot represent fails here, naming its key
        self.params = P.init_params(self.num_classes, seed=max(int(cfg.get("SEED", -1)), 0), style="d2", arch=self.arch, num_anchors=self.num_anchors)
        self._net = None
        self._momentum = None                              # SGD velocity carried over a re-created net / read from a checkpoint
        self.model = TrainModel(None, self.ctx, ensure=self._ensure_net)
        self._cap = self._capacity_from_cfg()              # one allocation for everything the loaders can produce
        self._per_rank = int(cfg.SOLVER.IMS_PER_BATCH) // self.world_size
        train_model_kwargs(cfg, self._per_rank)            # a sampling setting the native path cannot represent fails here, naming its key
        self._solver_kw = solver_kwargs(cfg)               # ... and so does an optimizer setting
        self.lr_at(0)                                      # ... and an unknown LR_SCHEDULER_NAME / WARMUP_METHOD
        from ..data import PREFETCH_DEPTH
        workers = int(cfg.DATALOADER.get("NUM_WORKERS", 0)) if "DATALOADER" in cfg else 0
        self._dev, self._workers, self._loader_epoch = dev, workers, 0
        self._uploader = self.data_loader = None
        self._build_loader()
        self._hooks = []
        self._need_broadcast = self.world_size > 1 and comm.backend() == "rccl"     # rank 0's weights and momentum win (DDP's constructor)
        self.register_hooks(self.build_hooks())

    def _build_loader(self):
        from ..data import build_detection_train_loader, PREFETCH_DEPTH
        from ..utils import comm
        # batches arrive in HBM (48 MB / step otherwise copied by the training thread)
        self._uploader = _Uploader(self._dev, PREFETCH_DEPTH + 3) if self._workers > 0 else None
        self.data_loader = build_detection_train_loader(self.cfg, rank=comm.get_rank(), world_size=self.world_size,
                                                        seed=max(int(self.cfg.get("SEED", -1)), 0) + 7919 * self._loader_epoch, upload=self._uploader)
        self._loader_epoch += 1

    def close(self):
        """Stop the loader threads and free what the trainer holds on the device (uploader ring, net, context).  train() releases the
        loader and the uploader itself; the net stays until close() so that `trainer.model` can still be evaluated after training."""
        self._release_loader()
        if self._net is not None:
            self._sync_params()
            self._net.close()
            self._net = None
            self.model.net = None
        from ..utils import comm
        if comm._rccl_ctx is self.ctx:
            comm.detach_rccl()
        if self.ctx is not None:
            self.ctx.close()
            self.ctx = None

    def _release_loader(self):
        dl, self.data_loader = self.data_loader, None
        if dl is not None and hasattr(dl, "close"):
            dl.close()                       # generator: runs the loader's `finally` (stops the producer, shuts the pools down)
        if self._uploader is not None:
            self._uploader.close()           # serialised against an upload still running in the collating thread
            self._uploader = None

    def _broadcast_if_needed(self):
        if self._need_broadcast and self._net is not None:
            self._net.broadcast_params(0)
            self._need_broadcast = False

    # ---- model / weights ----
    def _capacity_from_cfg(self):
        """Upper bound (padded h, w) of every frame the train mapper can produce from cfg.DATASETS.TRAIN + TEST (the validation-loss
        hook maps TEST images with the same augmentation): ResizeShortestEdge of each image's (height, width) -- under INPUT.CROP of its
        extreme crop windows -- for every MIN_SIZE_TRAIN choice (or both ends of the range), both orientations kept apart.  Falls back to MAX_SIZE_TRAIN x MAX_SIZE_TRAIN when a dataset does not
        say how large its images are.  Sized once, the net is never re-created mid-run (which would reset nothing any more -- the
        momentum arena is carried over -- but costs seconds)."""
        from ..data import DatasetCatalog
        c = self.cfg
        kw = input_kwargs(c)
        mins = [int(v) for v in kw["sizes"]]       # "range" draws between its two values: the frame grows with the scale, the ends bound it
        mx = int(c.INPUT.MAX_SIZE_TRAIN)
        hmax = wmax = 0
        try:
            for name in tuple(c.DATASETS.TRAIN) + tuple(c.DATASETS.TEST):
                for d in DatasetCatalog.get(name):
                    if "height" in d and "width" in d:
                        h0, w0 = int(d["height"]), int(d["width"])
                    elif "image_bgr" in d:
                        h0, w0 = d["image_bgr"].shape[:2]
                    else:
                        raise KeyError("height")
                    # INPUT.CROP: the frame's height grows with the window's height and shrinks with its width (and the other way round),
                    # so the extreme windows bound every frame a drawn one can give; a deterministic crop type has one extent
                    hs, ws = ((h0,), (w0,)) if kw["crop"] is None else (sorted(set(v)) for v in crop_extent_bounds(kw["crop"], h0, w0))
                    for ch in hs:
                        for cw in ws:
                            for m_ in mins:
                                h, w = shortest_edge_size(ch, cw, m_, mx)
                                hmax, wmax = max(hmax, h), max(wmax, w)
        except Exception:          # unknown dataset / no sizes: the square bound
            hmax = wmax = mx
        pad = lambda v: (int(v) + 31) // 32 * 32
        return (pad(max(hmax, 32)), pad(max(wmax, 32)))

    def _ensure_net(self, h, w):
        hp, wp = (h + 31) // 32 * 32, (w + 31) // 32 * 32
        cap = self._cap
        if self._net is not None and hp <= cap[0] and wp <= cap[1]:
            return
        if self._net is not None:
            logger.warning(f"a {h}x{w} batch exceeds the capacity {cap} derived from cfg: re-creating the net (weights and SGD momentum are carried over)")
            self._sync_params()
            self._momentum = self._net.momentum()
            self._net.close()
        c = self.cfg
        cap = (max(hp, cap[0]), max(wp, cap[1]))
        self._net = MaskRCNN(self.ctx, self.num_classes, max_h=cap[0], max_w=cap[1], max_out_hw=max(cap), arch=self.arch,
                             **train_model_kwargs(c, self._per_rank))
        self._net.load_params(self.params)
        self._restore_momentum()
        self._broadcast_if_needed()
        self._cap = cap
        self.model.net = self._net

    def _restore_momentum(self):
        """self._momentum: a flat arena (carried over a re-created net of the same configuration) or a dict of per-parameter buffers
        in torch layout (a checkpoint)."""
        mom, self._momentum = self._momentum, None
        if mom is None:
            return
        if isinstance(mom, dict) and set(mom) == {"arena"}:       # files written before the per-name format: this build's flat arena
            mom = mom["arena"]
        if isinstance(mom, dict):
            unknown = self._net.load_momentum_dict(mom)
            if unknown:
                logger.warning(f"momentum buffers of {len(unknown)} tensors the model does not train were ignored: {', '.join(unknown[:6])}")
        else:
            self._net.momentum(mom)

    def _sync_params(self):
        if self._net is not None:
            self.params.update(self._net.state_dict())

    def resume_or_load(self, resume=True):
        """detectron2 DefaultTrainer.resume_or_load: resume=True continues from OUTPUT_DIR/last_checkpoint when there is one (weights,
        iteration, SGD momentum); otherwise (and with resume=False) cfg.MODEL.WEIGHTS is loaded with DetectionCheckpointer semantics
        -- tensors missing from the file or of another shape (the COCO heads under NUM_CLASSES = 1, everything but the backbone for an
        ImageNet R-50.pkl) keep their detectron2-style initialisation, with a warning naming them -- and training starts at iteration 0.
        A detectron2:// or http(s) path cannot be fetched here (no network): training then starts from the initialisation, with a warning."""
        w = str(self.cfg.MODEL.WEIGHTS)
        resumed = False
        if resume:
            last = os.path.join(self.cfg.OUTPUT_DIR, "last_checkpoint")
            if os.path.isfile(last):
                w = os.path.join(self.cfg.OUTPUT_DIR, open(last).read().strip())
                resumed = True
        if w and not w.startswith(("detectron2://", "http://", "https://")):
            self.params, self.load_report = checkpoint.load_checkpoint(w, self.num_classes, self.arch, init=self.params, strict=resumed, with_report=True,
                                                                           num_anchors=self.num_anchors)
            if resumed:
                it = checkpoint.checkpoint_iteration(w)
                self.start_iter = self.iter = (it + 1) if it is not None else 0
                mom = checkpoint.checkpoint_momentum(w)
                if mom:
                    self._momentum = mom            # per-parameter buffers, torch layout
        elif w:
            logger.warning(f"cfg.MODEL.WEIGHTS={w!r} needs a download; no network: training from the seeded random initialisation")
        self._need_broadcast = self.world_size > 1 and comm_backend_is_rccl()
        if self._net is not None:
            self._net.load_params(self.params)
            self._restore_momentum()
            self._broadcast_if_needed()

    def save_checkpoint(self, path):
        self._sync_params()
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        mom = self._net.momentum_dict() if self._net is not None else None      # under the parameters' names, torch layout
        checkpoint.save_checkpoint(path, self.params, iteration=self.iter, optimizer=mom)
        with open(os.path.join(os.path.dirname(path) or ".", "last_checkpoint"), "w") as f:
            f.write(os.path.basename(path))

    # ---- hooks ----
    def build_hooks(self):
        """[PeriodicCheckpointer, PeriodicWriter]: the writer is last (AmpisTrainer does hooks.insert(-1, LossEvalHook(...)))."""
        from .train_loop import PeriodicCheckpointer, PeriodicWriter
        out = str(self.cfg.OUTPUT_DIR)
        return [PeriodicCheckpointer(int(self.cfg.SOLVER.CHECKPOINT_PERIOD), out), PeriodicWriter(out, period=20)]

    def register_hooks(self, hooks):
        for h in hooks:
            if h is not None:
                h.trainer = self
        self._hooks.extend([h for h in hooks if h is not None])

    # ---- loop ----
    def lr_at(self, it):
        """The learning rate of iteration `it`: SOLVER.LR_SCHEDULER_NAME = WarmupMultiStepLR (STEPS, GAMMA) or WarmupCosineLR (MAX_ITER), with
        the WARMUP_METHOD ("linear" | "constant") warm-up of WARMUP_ITERS iterations starting at WARMUP_FACTOR."""
        from .train_loop import warmup_cosine_lr, warmup_multistep_lr
        s = self.cfg.SOLVER
        name = s.get("LR_SCHEDULER_NAME", _SOLVER_DEFAULTS["LR_SCHEDULER_NAME"])
        method = s.get("WARMUP_METHOD", _SOLVER_DEFAULTS["WARMUP_METHOD"])
        iters, factor = int(s.WARMUP_ITERS), float(s.WARMUP_FACTOR)
        if name == "WarmupMultiStepLR":
            return warmup_multistep_lr(it, float(s.BASE_LR), tuple(s.STEPS), float(s.GAMMA), iters, factor, method)
        if name == "WarmupCosineLR":
            return warmup_cosine_lr(it, float(s.BASE_LR), int(s.MAX_ITER), iters, factor, method)
        raise ValueError(f"Unknown LR scheduler: {name}")

    def run_step(self):
        from ..utils import comm
        if self.data_loader is None:
            self._build_loader()
        from ..data import mapped_hw
        batch = next(self.data_loader)
        h = max(mapped_hw(d)[0] for d in batch)
        w = max(mapped_hw(d)[1] for d in batch)
        self._ensure_net(h, w)
        losses = self.model(batch, backward=True, seed=(self.iter * 7919 + comm.get_rank()) & 0x7FFFFFFF)
        scale = comm.all_reduce_gradients(self._net, self.ctx)
        lr = self.lr_at(self.iter)
        s = self.cfg.SOLVER
        self._net.sgd_step(lr, float(s.MOMENTUM), float(s.WEIGHT_DECAY), grad_scale=scale, **self._solver_kw)
        total = sum(losses.values())
        if not np.isfinite(total):
            raise FloatingPointError(f"Loss became infinite or NaN at iteration={self.iter}!\nloss_dict = {losses}")
        self.storage.put_scalars(total_loss=total, lr=lr, **losses)

    def train(self):
        from .train_loop import EventStorage
        os.makedirs(str(self.cfg.OUTPUT_DIR), exist_ok=True)
        logger.info(f"Starting training from iteration {self.start_iter}")
        self.storage = EventStorage(self.start_iter)
        self.iter = self.start_iter
        for h in self._hooks:
            h.before_train()
        # The loader threads run Python between their numpy / PIL calls; a training thread that comes back from the library waits for the
        # interpreter lock for up to one switch interval (5 ms by default) per call -- several calls per step.  0.2 ms while training.
        import sys
        switch = sys.getswitchinterval()
        if self._uploader is not None:
            sys.setswitchinterval(min(switch, 2e-4))
        try:
            for self.iter in range(self.start_iter, self.max_iter):
                for h in self._hooks:
                    h.before_step()
                self.run_step()
                for h in self._hooks:
                    h.after_step()
                self.storage.step()
            # detectron2 TrainerBase.train: "self.iter == max_iter can be used by `after_train` to tell whether the training successfully
            # finished or failed due to exceptions" -- after a complete run trainer.iter is max_iter, not max_iter - 1
            if self.max_iter > self.start_iter:
                self.iter += 1
        finally:
            sys.setswitchinterval(switch)
            try:
                for h in self._hooks:
                    h.after_train()
            finally:
                self._release_loader()          # loader threads, pools and the uploader's device ring live for one train() only
        self._sync_params()
