"""The micrograph inputs of the segmentation-performance tests, from committed fixtures only: the polygon ground truth of the two images of
tests/golden/via_subset.json and the reference's particle predictions for the same files (tests/golden/rle_pickles.json.gz, file
'particle-results').  Used by tests/test_seg_perf.py, the GPU tests, tools/bench_seg_perf.py and tests/golden/make_seg_perf_vectors.py."""
import base64
import functools
import gzip
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PARTICLES = "examples/powder/data/particle-results.pickle"
SIZE = (1024, 1536)


@functools.lru_cache(maxsize=None)
def _via():
    with open(os.path.join(GOLDEN, "via_subset.json")) as f:
        return json.load(f)["via"]["_via_img_metadata"]


@functools.lru_cache(maxsize=None)
def _particles():
    with gzip.open(os.path.join(GOLDEN, "rle_pickles.json.gz"), "rt") as f:
        gold = json.load(f)
    return {im["file_name"]: im for fl in gold["files"] if fl["path"] == PARTICLES for im in fl["images"]}


def file_names():
    """the images that have both ground truth and predictions, in the order of the VIA file"""
    return [v["filename"] for v in _via().values() if v["filename"] in _particles()]


def gt_polygons(file_name):
    """(list of per-instance polygon lists [[x0, y0, x1, y1, ...]], [n, 4] XYXY boxes, (h, w))"""
    img = next(v for v in _via().values() if v["filename"] == file_name)
    w, h = (int(x) for x in img["file_attributes"]["Size (width, height)"].split(","))
    polys, boxes = [], []
    for r in img["regions"]:
        x, y = np.asarray(r["shape_attributes"]["all_points_x"], np.float64), np.asarray(r["shape_attributes"]["all_points_y"], np.float64)
        polys.append([np.stack([x, y], axis=1).reshape(-1)])
        boxes.append([x.min(), y.min(), x.max(), y.max()])
    return polys, np.asarray(boxes, np.float64), (h, w)


@functools.lru_cache(maxsize=None)
def gt_rles(file_name):
    from ampis_amd import analyze
    from ampis_amd.structures import PolygonMasks
    polys, _, size = gt_polygons(file_name)
    return analyze.masks_to_rle(PolygonMasks(polys), size)


def pred_rles(file_name):
    """(list of RLE dicts, [n, 4] float32 boxes)"""
    im = _particles()[file_name]
    h, w = im["image_size"]
    return ([{"size": [h, w], "counts": base64.b64decode(c)} for c in im["counts_b64"]], np.asarray(im["boxes"], np.float32).reshape(-1, 4))
