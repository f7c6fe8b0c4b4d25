"""Golden vectors of `ampis.analyze.seg_perf_iset` and `det_perf_iset` (ampis/analyze.py:502-699) made BY THE REFERENCE ITSELF, run in the build
container (where /root/reference exists) in the manner of make_powder_vectors.py: the reference is imported UNMODIFIED on the façade.  Only
data is written, to tests/golden/seg_perf_vectors.json.gz; tests/test_seg_perf.py holds the product to it.

    python tests/golden/make_seg_perf_vectors.py        # needs /root/reference and the built library

Inputs are NOT copied: the two images of tests/golden/via_subset.json (polygon ground truth) and the reference's particle predictions for the
same files in tests/golden/rle_pickles.json.gz, read through tests/seg_perf_data.py.  Both sides reach the reference as RLE -- the ground
truth through masks_to_rle first, wrapped as the reference's RLEMasks -- so it takes its RLE.decode path and needs no skimage.  The reference
decodes every mask to the full image and forms three more [pairs, H, W] arrays: N_INSTANCES = 100, the FIRST 100 instances a side of each
image, keeps its peak below 1.5 GB (100 x 1024 x 1536 bools = 157 MB an array)."""
import base64
import gzip
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REFERENCE = "/root/reference"
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("MPLBACKEND", "Agg")

import numpy as np  # noqa: E402

import ampis_amd  # noqa: E402

ampis_amd.install_as_detectron2()
for name, attrs in (("skimage", {}), ("skimage.io", {}), ("skimage.measure", {}), ("skimage.draw", {"polygon2mask": lambda shape, poly: None}), ("cv2", {})):
    if name not in sys.modules:
        m = types.ModuleType(name); m.__dict__.update(attrs); m.__path__ = []
        sys.modules[name] = m
for alias, t in (("int", int), ("float", float), ("bool", bool)):
    if not hasattr(np, alias):
        setattr(np, alias, t)
sys.path.insert(0, REFERENCE)
from ampis import analyze  # noqa: E402
from ampis.structures import InstanceSet, RLEMasks  # noqa: E402
from detectron2.structures import Instances  # noqa: E402

import seg_perf_data as data  # noqa: E402

LIMIT = 523152          # the largest fixture so far (rle_pickles.json.gz)
N_INSTANCES = 100       # the first N_INSTANCES instances a side of each image


def b64(rles):
    return [base64.b64encode(r["counts"] if isinstance(r["counts"], bytes) else r["counts"].encode("ascii")).decode("ascii") for r in rles]


def plain(v):
    return np.asarray(v).tolist()


def main():
    images = []
    for name in data.file_names():
        gt = data.gt_rles(name)[:N_INSTANCES]
        pred, pred_boxes = data.pred_rles(name)
        pred, pred_boxes = pred[:N_INSTANCES], pred_boxes[:N_INSTANCES]
        gt_boxes = data.gt_polygons(name)[1][:N_INSTANCES]
        rec = {"file_name": name, "gt_indices": list(range(len(gt))), "pred_indices": list(range(len(pred)))}
        match = analyze.rle_instance_matcher(RLEMasks(gt), RLEMasks(pred))
        rec["match_results"] = {k: plain(v) for k, v in match.items()}
        for mode in ("reduced", "all"):
            iset, (colors, labels) = analyze.seg_perf_iset(RLEMasks(gt), RLEMasks(pred), mode=mode)
            assert len(iset.instances.masks.rle) == len(colors) and iset.instances.image_size == list(data.SIZE)
            rec[mode] = {"counts_b64": b64(iset.instances.masks.rle), "colors": plain(colors), "labels": list(labels),
                         "boxes": plain(iset.instances.boxes)}
        gi = InstanceSet(instances=Instances(data.SIZE, masks=RLEMasks(gt), boxes=gt_boxes), randomstate=0)
        pi = InstanceSet(instances=Instances(data.SIZE, masks=RLEMasks(pred), boxes=pred_boxes), randomstate=0)
        for key, tp_gt in (("det", False), ("det_tp_gt", True)):
            iset, colormap = analyze.det_perf_iset(gi, pi, tp_gt=tp_gt)
            rec[key] = {"counts_b64": b64(iset.instances.masks.rle), "boxes": plain(iset.instances.boxes), "colors": plain(iset.instances.colors),
                        "colormap": {k: plain(v) for k, v in colormap.items()}}
        print(name, len(gt), "gt", len(pred), "pred", len(match["tp"]), "tp", len(match["fn"]), "fn", len(match["fp"]), "fp")
        images.append(rec)
    out = {"made_by": "tests/golden/make_seg_perf_vectors.py: ampis.analyze of rccohn/AMPIS imported unmodified on the ampis_amd facade",
           "inputs": "tests/golden/via_subset.json (polygons through masks_to_rle) and 'particle-results' of tests/golden/rle_pickles.json.gz",
           "n_instances": N_INSTANCES, "images": images}
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "seg_perf_vectors.json.gz")
    with gzip.open(dst, "wt", compresslevel=9) as f:
        json.dump(out, f, separators=(",", ":"))
    size = os.path.getsize(dst)
    print("wrote", dst, size, "bytes")
    assert size < LIMIT, f"{size} bytes: not below the largest fixture ({LIMIT})"


if __name__ == "__main__":
    main()
