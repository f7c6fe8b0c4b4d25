"""InstanceSet and RLEMasks: the two containers of ampis/structures.py (:24-95, :98-200, :516-533) that `analyze.seg_perf_iset` and
`analyze.det_perf_iset` hand back.  Minimal on purpose: the constructor's fields as attributes and copy(); the readers (read_from_ddict,
read_from_model_out), the filters and compute_rprops stay served by the reference's own class on the façade (analyze.compute_rprops is the
function form of the last).

The reference's consumers dispatch on the EXACT type of what they are given -- visualize.display_iset: `type(masks) == structures.RLEMasks`,
structures.masks_to_bitmask_array: `type(masks) == InstanceSet` -- so an object of a class of this package would fall through to
NotImplementedError however well it quacks.  The two classes therefore compare EQUAL, as types, to the class of the same name in
`ampis.structures` (and to nothing else): that is all _SameAsReference does."""
import copy

import numpy as np
import torch


class _SameAsReference(type):
    def __eq__(cls, other):
        return other is cls or (isinstance(other, type) and other.__name__ == cls.__name__ and other.__module__ == "ampis.structures")

    def __ne__(cls, other):
        return not cls.__eq__(other)

    __hash__ = type.__hash__


class RLEMasks(metaclass=_SameAsReference):
    """A list of RLE dicts (`.rle`) that an Instances can hold as a field: len() and selection by int, slice, bool mask or index list."""

    def __init__(self, rle):
        self.rle = rle

    def __len__(self):
        return len(self.rle)

    def __getitem__(self, item):
        if isinstance(item, (int, np.integer)):
            return RLEMasks([self.rle[int(item)]])
        if isinstance(item, slice):
            return RLEMasks(self.rle[item])
        idx = np.asarray(item.cpu() if isinstance(item, torch.Tensor) else item)
        if idx.dtype == bool:
            assert len(idx) == len(self)
            idx = np.flatnonzero(idx)
        return RLEMasks([self.rle[int(i)] for i in idx])


class InstanceSet(metaclass=_SameAsReference):
    """The instances of one image (ampis/structures.py:98-200): the reference constructor's arguments, stored as attributes."""

    def __init__(self, mask_format=None, bbox_mode=None, filepath=None, annotations=None, instances=None, img=None, dataset_class=None,
                 pred_or_gt=None, HFW=None, HFW_units=None, randomstate=None):
        self.mask_format = mask_format
        self.bbox_mode = bbox_mode
        self.img = img
        self.filepath = filepath
        self.dataset_class = dataset_class
        self.pred_or_gt = pred_or_gt
        self.HFW = HFW
        self.HFW_units = HFW_units
        self.rprops = None
        self.instances = instances
        self.annotations = annotations
        self.randomstate = int(np.random.randint(2 ** 32 - 1)) if randomstate is None else randomstate
        self.colors = None

    def copy(self):
        return copy.deepcopy(self)
