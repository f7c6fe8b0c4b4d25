"""Instance matching and detection / segmentation scores on RLE masks -- the "mask IoU vs ref" half of the benchmark metric
(SURVEY.md §8 f3).  Same entry points, arguments and result keys as ampis/analyze.py (`rle_instance_matcher` :184-223,
`det_seg_scores` :226-339), so notebooks call it unchanged; the computation is laid out for the C-ABI RLE codec instead of for
pycocotools:

  * ONE `amp_rle_iou_matrix` call gives every (ground truth, prediction) IoU.  (The reference walks 80-wide blocks because
    pycocotools.mask.iou has a size limit, ampis/analyze.py:54-112; the C routine has none, so there is nothing to walk.)
  * The matching rule is stated as array semantics rather than as a loop:
      - a ground-truth instance g is assigned the prediction of maximal IoU, the FIRST one among equals (lowest index);
      - g is a true positive iff that IoU is strictly greater than `iou_thresh`, otherwise a false negative;
      - assignment is not exclusive: two ground-truth instances may take the same prediction (a prediction covering two particles
        counts as two true positives -- the reference's behaviour);
      - a prediction no ground-truth instance took is a false positive.
  * Pixel-level scores come from ONE `amp_rle_pair_overlap` call over the matched pairs (|g and p|, |g minus p|, |p minus g|) instead
    of a merge + three area calls per pair.
  * `mask_edge_distance` (ampis/analyze.py:416-499; helpers `merge_boxes` :342) measures how far the disagreeing pixels of every matched pair
    lie from the other mask: ONE `amp_mask_edge_distance` call for all pairs, on the device or on the host.  The reference broadcasts
    [queries x targets x 2] doubles per pair and takes torch.sqrt; here the exact integer squared distance comes back (an exact nearest-pixel
    search on bit planes, csrc/edge_distance.hip) and the root is numpy's correctly rounded one.
  * `region_properties`, `compute_rprops`, `regionprops_table` (ampis/structures.py:474-514, InstanceSet.compute_rprops on
    skimage.measure.regionprops_table): ONE `amp_mask_region_props` call gives 13 exact integers per mask from the run lists, on the device
    (csrc/region_props.hip) or on the host, and `region_floats` derives every column from them.  The reference decodes each mask to the full
    image first.
  * `overlap_matrix` (the all-pairs RLE.merge(intersect=True) + RLE.area loop of ampis/applications/powder.py:82) and `mask_areas`
    (ampis/structures.py:536-583): ONE `amp_rle_overlap_groups` call gives the exact pixel count of every pair of masks of an image, or of
    every image of a sample (ampis_amd/applications/powder.py), on the device (csrc/rle_overlap.hip) or on the host.
  * `render_instances` (detectron2 Visualizer.overlay_instances, what visualize.display_iset / display_ddicts end in): ONE `amp_render_instances`
    call draws the fill, the edge and the box frame of every instance of an image in draw order from the run lists, on the device
    (csrc/render.hip) or on the host; the blend arrives as a lookup table built with the dense path's own NumPy expression, so the bytes equal
    the per-instance full-image passes of utils/visualizer.py.
  * `mask_topology`, `clean_masks` and the `euler_number` / `filled_area` columns of `region_properties` (what users do today with
    skimage.morphology.remove_small_objects / remove_small_holes and scipy.ndimage.binary_fill_holes on one decoded array per mask): `amp_mask_parts`
    calls give the connected components of the ones or of the zeros of every mask of an image from the run lists -- a lock-free union-find
    over vertical pieces on the device (csrc/mask_parts.hip) or a sequential one on the host --, flip the components a rule picks and return
    canonical run lists; no mask is decoded.
  * `resolve_overlaps` and `instances_to_label_image` (what users do today with a loop of decoded masks, labels[mask_i] = i + 1 in score
    order, and an encode of labels == i + 1 per instance): ONE `amp_flatten_instances` call gives every pixel that several masks cover to
    one of them -- the highest score, the smallest area, the first in the list or the smallest given rank -- and returns the disjoint masks
    as canonical run lists, the int32 label image, the visible areas and boxes; one wave per 64 x 64 tile claims the pixels in priority
    order on the device (csrc/flatten.hip), a sweep over the sorted run ends on the host; no mask is decoded.  It is the inverse of
    `label_image_to_rle`.
  * `mask_contours` and `masks_to_polygons` (what users do today with cv2.findContours / detectron2's GenericMask.mask_to_polygons on one
    decoded array per mask): ONE `amp_mask_contours` call gives the boundary rings of every mask of an image from the run lists as exact
    crack rings on pixel corners -- the cycles of a successor permutation over the top and bottom edges of vertical pieces, found by pointer
    jumping on the device (csrc/contours.hip) or by a sequential walk on the host --; no mask is decoded.  It is the inverse of
    `masks_to_rle(PolygonMasks, ...)`.
  * `dilate_masks`, `erode_masks`, `open_masks`, `close_masks`, `boundary_bands`, `boundary_iou` and `near_pairs` (what users do today with
    scipy.ndimage.binary_dilation / binary_erosion / binary_opening / binary_closing or cv2.erode on one decoded array per mask): ONE
    `amp_mask_morphology` call changes the shape of every mask of an image by a distance on its run list -- every vertical piece sends a
    grown or shrunk interval to the columns within the radius, and a pixel's class follows from the integer cover of those intervals, found
    by a sort and a scan of +1 / -1 events on the device (csrc/morphology.hip) or by a sweep per column on the host --; no mask is decoded.
  * `mask_distance_maps`, `inscribed_circles`, `erosion_curve` and the `inscribed_radius` column of `region_properties` (what users do today
    with scipy.ndimage.distance_transform_edt on one decoded array per mask): ONE `amp_mask_distance` call gives the exact squared distance
    of every mask pixel to the nearest pixel outside its mask, the deepest pixel, the sums and the erosion curve of every mask of an image
    from the run lists -- every pixel walks the columns outwards from its own and looks up the vertical piece that holds its row, one wave
    per 64 rows of a piece on the device (csrc/mask_distance.hip), the same walk in a loop on the host --; no mask is decoded to the image.
  * `intensity_properties`, `intensity_histograms`, `intensity_quantiles` and the intensity columns of `region_properties` (what users do
    today with skimage's regionprops(..., intensity_image=img) or img[RLE.decode(m)] per instance): ONE `amp_mask_intensity` call gives the
    exact integer sums, extremes and histograms of the micrograph's grey levels under every mask of an image from the run lists -- in a
    column-major plane of the image every run is one contiguous range, so the device transposes the image once and reduces the runs
    (csrc/mask_intensity.hip), the host cuts the runs at the column ends --; no mask is decoded.
With no prediction at all the detection precision is 0/0: like the reference this raises ZeroDivisionError.
The independent checker is oracle/matcher.py (a loop-for-loop restatement of the reference, pinned by its known-answer test)."""
import numpy as np

from . import rle
from .structures import BitMasks, Instances, InstanceSet, PolygonMasks, RLEBitMasks, RLEMasks


def masks_to_rle(masks, size=None, device='auto'):
    """list of RLE dicts | RLEBitMasks | object with .rle | PolygonMasks (needs size=(h,w)) | BitMasks / bool ndarray [N,H,W].  Polygon masks
    become run lists in ONE amp_polygons_to_rle call for all instances (csrc/polygon_runs.hip, or polygon_runs_host.hip on the host: identical
    bytes, those of rle.merge(rle.frPyObjects(...)) per instance); device: 'cpu', 'cuda' or 'auto' (the device when one is visible)."""
    if isinstance(masks, RLEBitMasks) or hasattr(masks, "rle"):
        return list(masks.rle)
    if isinstance(masks, (list, tuple)) and (len(masks) == 0 or isinstance(masks[0], dict)):
        return list(masks)
    if isinstance(masks, PolygonMasks):
        assert size is not None, "size=(height, width) is required for polygon masks"
        return rle.polygons_to_rle(masks.polygons, size[0], size[1], ctx=_device_context("masks_to_rle", device, len(masks.polygons)))
    arr = masks.tensor.numpy() if isinstance(masks, BitMasks) else np.asarray(masks)
    if arr.ndim == 3:
        return [rle.encode(np.asfortranarray(m)) for m in arr.astype(bool)]
    raise NotImplementedError(f"unsupported mask type {type(masks)}")


def iou_matrix(gt, pred):
    """[len(gt), len(pred)] float64 IoU of every ground-truth / prediction pair (no crowd regions), one C call."""
    if len(gt) == 0 or len(pred) == 0:
        return np.zeros((len(gt), len(pred)))
    return np.ascontiguousarray(rle.iou(pred, gt, np.zeros(len(gt), bool)).T)


def match_instances(iou, iou_thresh=0.5):
    """The matching rule of the module docstring on a [G, P] IoU matrix -> {'tp': [n,2] (gt, pred) index pairs in gt order,
    'fn': gt indices, 'fp': pred indices, 'iou': IoU of each true positive}."""
    assert iou_thresh >= 0, "iou_thresh must not be negative"
    G, P = iou.shape
    if P == 0:
        return {"tp": np.zeros((0, 2), int), "fn": np.arange(G), "fp": np.zeros(0, int), "iou": np.zeros(0)}
    taken = iou.argmax(axis=1)                               # first maximum of each row
    best = iou[np.arange(G), taken]
    hit = best > iou_thresh                                  # strict
    unclaimed = np.ones(P, bool)
    unclaimed[taken[hit]] = False
    return {"tp": np.stack([np.flatnonzero(hit), taken[hit]], axis=1).astype(int).reshape(-1, 2), "fn": np.flatnonzero(~hit),
            "fp": np.flatnonzero(unclaimed), "iou": best[hit]}


def rle_instance_matcher(gt, pred, iou_thresh=0.5, size=None, device='auto'):
    gt, pred = masks_to_rle(gt, size, device), masks_to_rle(pred, size, device)
    return match_instances(iou_matrix(gt, pred), iou_thresh)


def det_seg_scores(gt, pred, iou_thresh=0.5, size=None, device='auto'):
    gt, pred = masks_to_rle(gt, size, device), masks_to_rle(pred, size, device)
    m = match_instances(iou_matrix(gt, pred), iou_thresh)
    n_tp, n_fn, n_fp = len(m["tp"]), len(m["fn"]), len(m["fp"])
    both, gt_only, pred_only = rle.pair_overlap(gt, pred, m["tp"])       # per matched pair: pixels in both / missed / spurious
    with np.errstate(divide="ignore", invalid="ignore"):
        seg_precision, seg_recall = both / (both + pred_only), both / (both + gt_only)
    return {"det_precision": n_tp / (n_tp + n_fp), "det_recall": n_tp / (n_tp + n_fn), "seg_precision": seg_precision, "seg_recall": seg_recall,
            "det_tp": m["tp"], "det_fn": m["fn"], "det_fp": m["fp"], "seg_tp": both, "seg_fn": gt_only, "seg_fp": pred_only, "det_tp_iou": m["iou"]}


def merge_boxes(box1, box2):
    """The smallest index box [r1, r2, c1, c2] (the region im[r1:r2, c1:c2]) that holds box1 and box2 (ampis/analyze.py:342)."""
    r11, r12, c11, c12 = box1
    r21, r22, c21, c22 = box2
    return np.array([min(r11, r21), max(r12, r22), min(c11, c21), max(c12, c22)])


def _index_boxes(boxes, masks, name):
    """[len(masks), 4] int64 index boxes of argument `name`: the caller's, checked, or (None) the tight boxes of the runs."""
    if boxes is None:
        tight = [rle.bbox(m) for m in masks]                      # (x0, y0, x1, y1), None for an empty mask
        return np.array([(0, 0, 0, 0) if b is None else (b[1], b[3], b[0], b[2]) for b in tight], dtype=np.int64).reshape(-1, 4)
    out = np.zeros((len(boxes), 4), dtype=np.int64)
    for i, b in enumerate(boxes):
        try:
            v = [x for x in np.asarray(b).reshape(-1).tolist()]
            ok = len(v) == 4 and all(not isinstance(x, bool) and float(x) == int(x) for x in v)
        except (TypeError, ValueError, OverflowError):
            ok = False
        if not ok:
            raise ValueError(f"mask_edge_distance: {name}[{i}] = {b!r} is not four integers [r1, r2, c1, c2]")
        r1, r2, c1, c2 = (int(x) for x in v)
        if min(r1, r2, c1, c2) < 0 or r1 > r2 or c1 > c2:
            raise ValueError(f"mask_edge_distance: {name}[{i}] = {[r1, r2, c1, c2]}: indices must not be negative and r1 <= r2, c1 <= c2")
        out[i] = (r1, r2, c1, c2)
    return out


_device_ctx = {}


def _current_device_context(who):
    """The context of the device path: one per HIP device, with a stream of its own (the call uploads, computes and downloads by itself)."""
    import torch
    from . import _lib
    if not torch.cuda.is_available():
        raise _lib.AmpError(f"{who}(device='cuda'): no HIP device is visible (device='cpu' computes on the host)")
    dev = torch.cuda.current_device()
    if dev not in _device_ctx:
        _device_ctx[dev] = _lib.Context(dev)
    return _device_ctx[dev]


def _device_context(who, device, work):
    """The context of `device` for function `who`: None for the host -- 'cpu', or 'auto' with no visible device or nothing to do (`work`
    false) --, the current device's context for 'cuda' (an error without one) and for 'auto' otherwise.  ValueError for any other value."""
    import torch
    dev = str(device).lower()
    if dev not in ("auto", "cpu", "cuda"):
        raise ValueError(f"{who}: device = {device!r} ('auto', 'cpu' or 'cuda')")
    return _current_device_context(who) if dev == "cuda" or (dev == "auto" and work and torch.cuda.is_available()) else None


def mask_edge_distance(gt_mask, pred_mask, gt_box, pred_box, matches, device='auto', squared=False, size=None):
    """For every matched pair matches[i] = (gt index, pred index): the distance in pixels from each false-positive pixel (pred & ~gt) to the nearest
    ground-truth pixel and from each false-negative pixel (gt & ~pred) to the nearest predicted pixel, inside the pair's merged box
    (ampis/analyze.py:416-499: same arguments, same two lists of CPU float64 tensors, pixels in torch.where order).

    gt_mask, pred_mask: anything masks_to_rle accepts (size=(h, w) for polygons); gt_box, pred_box: one index box [r1, r2, c1, c2] per mask, or None
    for the tight box of each mask; device: 'cpu' (host), 'cuda' (HIP device, an error without one) or 'auto' (the device when one is visible);
    squared=True returns the exact squared distances as int64 tensors.  ValueError for a malformed box, a match index out of range, masks of
    different sizes, and a pair with disagreeing pixels whose other mask has no pixel in the box (the reference fails there too)."""
    import torch
    gt, pred = masks_to_rle(gt_mask, size, device), masks_to_rle(pred_mask, size, device)
    m = np.asarray(matches)
    if m.size and (m.ndim != 2 or m.shape[1] != 2 or not np.issubdtype(m.dtype, np.integer)):
        raise ValueError(f"mask_edge_distance: matches must be an [n, 2] integer array of (gt, pred) indices, got shape {m.shape} {m.dtype}")
    m = m.reshape(-1, 2).astype(np.int64)
    for i, (g, p) in enumerate(m.tolist()):
        if not (0 <= g < len(gt) and 0 <= p < len(pred)):
            raise ValueError(f"mask_edge_distance: matches[{i}] = ({g}, {p}) is outside the {len(gt)} ground-truth and {len(pred)} predicted masks")
    sizes = {tuple(int(v) for v in r["size"]) for r in gt + pred}
    if len(sizes) > 1:
        raise ValueError(f"mask_edge_distance: gt_mask / pred_mask hold masks of different sizes {sorted(sizes)}")
    gb, pb = _index_boxes(gt_box, gt, "gt_box"), _index_boxes(pred_box, pred, "pred_box")
    if len(gb) < len(gt) and len(m) and m[:, 0].max() >= len(gb):
        raise ValueError(f"mask_edge_distance: gt_box has {len(gb)} boxes, matches name ground-truth mask {int(m[:, 0].max())}")
    if len(pb) < len(pred) and len(m) and m[:, 1].max() >= len(pb):
        raise ValueError(f"mask_edge_distance: pred_box has {len(pb)} boxes, matches name predicted mask {int(m[:, 1].max())}")
    boxes = np.array([merge_boxes(gb[g], pb[p]) for g, p in m.tolist()], dtype=np.int64).reshape(-1, 4)
    boxes = np.minimum(boxes, 1 << 30)                            # beyond any image: the slice ends at the image's border
    ctx = _device_context("mask_edge_distance", device, len(m))
    fp, fn = rle.edge_distance(gt, pred, m, boxes, ctx=ctx)
    if squared:
        conv = lambda d: torch.from_numpy(d.astype(np.int64))
    else:
        conv = lambda d: torch.from_numpy(np.sqrt(d.astype(np.float64)))
    return [conv(d) for d in fp], [conv(d) for d in fn]


# ---- region properties (ampis/structures.py:474-514, InstanceSet.compute_rprops) ----------------------------------------------------------------

RPROPS_DEFAULT_KEYS = ["area", "equivalent_diameter", "major_axis_length", "perimeter", "solidity", "orientation"]       # ampis/structures.py:505
RPROPS_KEYS = ("area", "bbox", "bbox_area", "centroid", "convex_area", "eccentricity", "equivalent_diameter", "extent", "major_axis_length",
               "minor_axis_length", "orientation", "perimeter", "solidity")
RPROPS_TOPOLOGY_KEYS = ("euler_number", "filled_area")            # from mask_topology at connectivity 2: the mask as a shape with pieces
RPROPS_DISTANCE_KEYS = ("inscribed_radius",)                      # from inscribed_circles at border_value 0: the largest circle inside the mask


def region_floats(bbox, vals):
    """THE derivation of the region-property floats from the exact integers of amp_mask_region_props (bbox: 4 ints, vals: 13 ints of one mask)
    -> dict of every supported column.  Both the device and the host path go through here, so they return identical bytes.  The differences
    that cancel (A, B, C, A - C, A C - B^2) are formed in Python integers, which may pass 64 bits, and rounded to float64 once.  B is an exact
    integer, so a zero is a true zero: atan2 gets +0.0 for it (a mask symmetric about a column wider than tall: +pi/2, never -pi/2 from the
    sign of a float zero)."""
    import math
    N, sr, sc, srr, src, scc, p1, p2, p3, hull = (int(v) for v in vals[:10])
    r0, c0, r1, c1 = (int(v) for v in bbox)
    nan = float("nan")
    out = {"area": N, "bbox-0": r0, "bbox-1": c0, "bbox-2": r1, "bbox-3": c1, "bbox_area": (r1 - r0) * (c1 - c0), "convex_area": hull,
           "perimeter": p1 + p2 * math.sqrt(2.0) + p3 * ((1.0 + math.sqrt(2.0)) / 2.0), "equivalent_diameter": math.sqrt(4 * N / math.pi)}
    if N == 0:
        out.update({k: nan for k in ("centroid-0", "centroid-1", "eccentricity", "extent", "major_axis_length", "minor_axis_length", "orientation",
                                     "solidity")})
        return out
    A, Cc, B = N * scc - sc * sc, N * srr - sr * sr, -(N * src - sr * sc)      # N^2 times the inertia tensor [[a, b], [b, c]]
    N2 = N * N
    b = B / N2
    root = math.sqrt(b * b + ((A - Cc) / (2 * N2)) ** 2)
    l1 = (A + Cc) / (2 * N2) + root
    l2 = ((A * Cc - B * B) / (N2 * N2)) / l1 if l1 else 0.0
    out.update({"centroid-0": sr / N, "centroid-1": sc / N, "extent": N / out["bbox_area"], "solidity": N / hull,
                "major_axis_length": 4.0 * math.sqrt(l1), "minor_axis_length": 4.0 * math.sqrt(l2),
                "eccentricity": math.sqrt(2.0 * root / l1) if l1 else 0.0,
                "orientation": (-math.pi / 4 if B < 0 else math.pi / 4) if A == Cc else 0.5 * math.atan2(-2.0 * b if B else 0.0, (Cc - A) / N2)})
    return out


def _rprops_columns(keys, channels=0):
    """regionprops_table's column names of `keys` (None: the reference's default list); ValueError naming a key this module does not have.
    channels: those of the intensity image (0: none; the intensity keys are then refused by the caller); their columns are
    _intensity_columns'."""
    keys = list(RPROPS_DEFAULT_KEYS if keys is None else keys)
    cols = []
    for k in keys:
        if k in RPROPS_INTENSITY_KEYS:
            cols += [c[0] for c in _intensity_columns("region_properties", [k], max(channels, 1))]
            continue
        if k not in RPROPS_KEYS and k not in RPROPS_TOPOLOGY_KEYS and k not in RPROPS_DISTANCE_KEYS:
            raise ValueError(f"region_properties: unsupported key {k!r} (supported: "
                             f"{', '.join(RPROPS_KEYS + RPROPS_TOPOLOGY_KEYS + RPROPS_DISTANCE_KEYS + RPROPS_INTENSITY_KEYS)})")
        cols += [f"bbox-{i}" for i in range(4)] if k == "bbox" else [f"centroid-{i}" for i in range(2)] if k == "centroid" else [k]
    return cols


def region_properties(masks, keys=None, size=None, device='auto', intensity_image=None):
    """Shape measurements of every mask, the table skimage.measure.regionprops_table gives InstanceSet.compute_rprops (ampis/structures.py:474-514):
    a dict of column name -> np.ndarray [N], columns named like regionprops_table ('bbox-0' .. 'bbox-3', 'centroid-0', 'centroid-1', the rest by
    key).  A region is ALL set pixels of one mask (holes and disconnected parts included), coordinates are (row, column) of the full image.

    masks: anything masks_to_rle accepts (size=(h, w) for polygons); keys: any of RPROPS_KEYS, RPROPS_TOPOLOGY_KEYS ('euler_number' and
    'filled_area', int64, 0 for an empty mask: skimage's -- foreground 8-connected, holes 4-connected -- from mask_topology at connectivity 2 on
    the same path) and RPROPS_DISTANCE_KEYS ('inscribed_radius', float64, 0 for an empty mask: inscribed_circles' radius at border_value 0
    on the same path), None for the reference's default list; device:
    'cpu' (host), 'cuda' (HIP device, an error without one) or 'auto' (the device when one is visible).  One amp_mask_region_props call returns
    13 exact integers per mask (csrc/region_props.hip, or mask_analysis_host.hip on the host); region_floats derives the floats from them for both
    paths, so they agree bit for bit.  An empty mask: area, perimeter, convex_area, equivalent_diameter 0, bbox (0, 0, 0, 0), NaN elsewhere.

    UNPINNED PARITY: skimage is not part of this environment and the reference stores no region-property output, so no vector of the reference's
    pins this function.  The definitions are skimage's regionprops (rc coordinates, 0.16 and later) restated in DESIGN §7e; the tests hold
    the integers to an independent scipy / brute-force evaluation of those definitions and the floats to their exact-rational value.
    ValueError for an unknown key (before any device work), a bad `device`, masks of different sizes.

    intensity_image: the micrograph under the masks, as intensity_properties takes it.  With it the keys of RPROPS_INTENSITY_KEYS
    ('intensity_mean', 'intensity_min', 'intensity_max', 'intensity_std', 'centroid_weighted' and their older names) are intensity_properties'
    columns of the same masks on the same path; without it such a key is a ValueError before any device work."""
    wanted = [k for k in (keys or ()) if k in RPROPS_INTENSITY_KEYS]
    if wanted and intensity_image is None:
        raise ValueError(f"region_properties: the key {wanted[0]!r} needs an intensity_image")
    channels = rle.intensity_image("region_properties", intensity_image)[0].shape[2] if wanted else 0
    cols = _rprops_columns(keys, channels)
    rles = masks_to_rle(masks, size, device)
    sizes = {tuple(int(v) for v in r["size"]) for r in rles}
    if len(sizes) > 1:
        raise ValueError(f"region_properties: masks of different sizes {sorted(sizes)}")
    if wanted:
        grey = intensity_properties(rles, intensity_image, wanted, device=device)      # refuses an image of another size before any device work
    ctx = _device_context("region_properties", device, len(rles))
    bbox, vals = rle.region_props(rles, ctx=ctx)
    rows = [region_floats(b, v) for b, v in zip(bbox.tolist(), vals.tolist())]
    ints = ("area", "bbox_area", "convex_area", "bbox-0", "bbox-1", "bbox-2", "bbox-3")
    topo = mask_topology(rles, 2, device=device) if any(c in RPROPS_TOPOLOGY_KEYS for c in cols) else {}
    if any(c in RPROPS_DISTANCE_KEYS for c in cols):
        topo = dict(topo, inscribed_radius=inscribed_circles(rles, 0, device=device)["radius"])
    if wanted:
        topo = dict(topo, **grey)
    return {c: topo[c] if c in topo else np.array([r[c] for r in rows], dtype=np.int64 if c in ints else np.float64) for c in cols}


def compute_rprops(iset, keys=None, return_df=False, device='auto', intensity_image=None):
    """InstanceSet.compute_rprops (ampis/structures.py:474-514) as a function: stores in iset.rprops a pandas DataFrame with one row per instance
    -- the region_properties columns of `keys` plus 'class_idx' -- and returns it when return_df.  Duck-typed: iset.instances.masks,
    iset.instances.image_size (for polygon masks), iset.instances.class_idx.  Unlike the reference, whose cells are the one-element arrays of
    one regionprops_table call per mask, the cells here are scalars.  intensity_image: the image of the RPROPS_INTENSITY_KEYS; None: iset.img,
    and a ValueError before any device work when such a key is asked for and there is neither."""
    import pandas as pd
    inst = iset.instances
    if intensity_image is None and any(k in RPROPS_INTENSITY_KEYS for k in (keys or ())):
        intensity_image = getattr(iset, "img", None)
    table = region_properties(inst.masks, keys, size=tuple(int(v) for v in inst.image_size), device=device, intensity_image=intensity_image)
    df = pd.DataFrame(table)
    df["class_idx"] = np.asarray(inst.class_idx).reshape(-1)
    iset.rprops = df
    return df if return_df else None


# ---- parts and holes: mask topology and repair (skimage.morphology.remove_small_objects / remove_small_holes, scipy.ndimage.binary_fill_holes) -

def _parts_input(who, masks, connectivity, size, device):
    """(rles, ctx) of a mask_topology / clean_masks call; ValueError for a bad connectivity or device and for masks of different sizes"""
    if connectivity not in (1, 2):
        raise ValueError(f"{who}: connectivity = {connectivity!r} (1: 4 neighbours, 2: 8 neighbours)")
    rles = masks_to_rle(masks, size, device)
    sizes = {tuple(int(v) for v in r["size"]) for r in rles}
    if len(sizes) > 1:
        raise ValueError(f"{who}: masks of different sizes {sorted(sizes)}")
    return rles, _device_context(who, device, len(rles))


def mask_topology(masks, connectivity=2, size=None, device='auto'):
    """Every mask as a shape with pieces: a dict of int64 [N] arrays 'n_parts', 'n_holes', 'euler_number' (parts - holes), 'area',
    'filled_area' (area + the pixels of all holes) and 'largest_part_area'.  Parts are the connected components of the ones -- connectivity 2:
    8 neighbours, 1: 4 neighbours; holes the components of the zeros under the dual neighbourhood (4 neighbours for connectivity 2, 8 for 1)
    with no pixel in the first or last row or column of the image: background that reaches the border is the outside, as in
    scipy.ndimage.binary_fill_holes.  Connectivity 2 gives skimage.measure.regionprops' euler_number and filled_area.  An empty mask has no
    part and no hole.

    masks: anything masks_to_rle accepts (size=(h, w) for polygons); device: 'cpu' (host), 'cuda' (HIP device, an error without one) or 'auto'
    (the device when one is visible).  Two statistics-only amp_mask_parts calls on the run lists (csrc/mask_parts.hip, or mask_parts_host.hip on the
    host: identical bytes), no mask is decoded.  ValueError for a bad connectivity or device and for masks of different sizes."""
    rles, ctx = _parts_input("mask_topology", masks, connectivity, size, device)
    parts, _ = rle.mask_parts(rles, 1, connectivity, ctx=ctx, emit=False)
    holes, _ = rle.mask_parts(rles, 0, connectivity, ctx=ctx, emit=False)
    return {"n_parts": parts[:, 0].copy(), "n_holes": holes[:, 0].copy(), "euler_number": parts[:, 0] - holes[:, 0], "area": parts[:, 1].copy(),
            "filled_area": parts[:, 1] + holes[:, 1], "largest_part_area": parts[:, 2].copy()}


def clean_masks(masks, min_size=0, area_threshold=0, keep_largest=False, connectivity=2, size=None, device='auto', return_stats=False):
    """Repairs every mask on its run list, in two steps one after the other:
      1. parts: with keep_largest only the part of largest area stays (among equals the one whose first pixel in column-major order comes
         first); then parts of area < min_size are removed (skimage.morphology.remove_small_objects: strict);
      2. holes, of the result of step 1: holes of area < area_threshold are filled (remove_small_holes: strict); None fills every hole
         (scipy.ndimage.binary_fill_holes), 0 none.
    So a speck inside a ring's hole is removed first and the hole that grows by it is judged as a whole.  Parts, holes and connectivity as in
    mask_topology.  Returns the list of RLE dicts in canonical form (what rle.encode gives for the dense result), length and order unchanged;
    a mask may come back empty.  return_stats: also a dict of int64 [N] arrays 'parts_removed', 'pixels_removed', 'holes_filled',
    'pixels_filled'.

    At most two emitting amp_mask_parts calls (csrc/mask_parts.hip, or mask_parts_host.hip on the host: identical bytes); a step whose
    arguments change nothing is skipped.  return_stats adds one statistics-only call behind each step that ran: the call reports the pixels it
    flipped, the number of flipped components is the difference of the counts before and after.  ValueError for a negative threshold, a bad
    connectivity or device and for masks of different sizes."""
    if min_size is None or int(min_size) < 0:
        raise ValueError(f"clean_masks: min_size = {min_size!r} (a pixel count, not negative)")
    if area_threshold is not None and int(area_threshold) < 0:
        raise ValueError(f"clean_masks: area_threshold = {area_threshold!r} (a pixel count, not negative; None fills every hole)")
    rles, ctx = _parts_input("clean_masks", masks, connectivity, size, device)
    n = len(rles)
    stats = {k: np.zeros(n, np.int64) for k in ("parts_removed", "pixels_removed", "holes_filled", "pixels_filled")}
    steps = []
    if keep_largest or int(min_size) > 1:                            # no part has fewer pixels than one
        steps.append((1, int(min_size), bool(keep_largest), "parts_removed", "pixels_removed"))
    if area_threshold is None or int(area_threshold) > 1:
        steps.append((0, area_threshold, False, "holes_filled", "pixels_filled"))
    canonical = False
    for colour, thr, keep, k_count, k_pixels in steps:
        if n == 0:
            break
        st, counts = rle.mask_parts(rles, colour, connectivity, thr, keep, ctx=ctx)
        pool, off, ln = rle._pool(counts)
        rles = [{"size": list(r["size"]), "counts": c} for r, c in zip(rles, rle.counts_to_strings(pool, off, ln))]
        canonical = True
        stats[k_pixels] = st[:, 3].copy()
        if return_stats:
            after, _ = rle.mask_parts(rles, colour, connectivity, ctx=ctx, emit=False)
            stats[k_count] = st[:, 0] - after[:, 0]
    if not canonical and n:                                          # nothing to do: the canonical form of the input, by a call that flips nothing
        _, counts = rle.mask_parts(rles, 1, connectivity, ctx=ctx)
        pool, off, ln = rle._pool(counts)
        rles = [{"size": list(r["size"]), "counts": c} for r, c in zip(rles, rle.counts_to_strings(pool, off, ln))]
    return (rles, stats) if return_stats else rles


# ---- boundary rings: masks back to polygons (cv2.findContours / detectron2's GenericMask.mask_to_polygons on one decoded array per mask) --------

def _contours_call(who, masks, connectivity, size, device):
    """(rle.mask_contours' arrays, the number of masks) of a mask_contours / masks_to_polygons call"""
    rles, ctx = _parts_input(who, masks, connectivity, size, device)
    if not rles:                                                     # no mask: no ring, whatever the size
        z = np.zeros(0, np.int64)
        return (np.zeros(1, np.int64), z, z, z, z, np.zeros((0, 2), np.int32)), 0
    return rle.mask_contours(rles, connectivity, ctx=ctx), len(rles)


def mask_contours(masks, connectivity=2, size=None, device='auto'):
    """The boundary rings of every mask: a list with, per mask, the list of its rings as dicts {'xy': int32 [k, 2] corners (x, y), 'hole': bool,
    'area': int, 'length': int}.  Exact crack rings on pixel corners: pixel (r, c) is the square [c, c + 1] x [r, r + 1], a vertex an integer
    corner 0 <= x <= w, 0 <= y <= h -- the coordinates PolygonMasks and polygons_to_rle use, no half-pixel shift --, every ring has the mask on
    its right hand (outer rings clockwise on screen, hole rings the other way) and lists its corners only, from its smallest corner by x, then
    y; the rings of a mask are ordered by that corner.  connectivity 2 joins diagonal ones into one ring (and keeps diagonal zeros apart), 1
    the other way round, so the outer rings are mask_topology's parts and the hole rings its holes (an island in a hole is a part).  'area' is
    the pixels the ring encloses, 'length' its crack length.  The parity (XOR) of all rings through polygons_to_rle is the mask again, bit for
    bit.  UNPINNED PARITY with cv2.findContours, which is not part of this environment and returns pixel-centre chains, not cracks.

    masks: anything masks_to_rle accepts (size=(h, w) for polygons); device: 'cpu' (host), 'cuda' (HIP device, an error without one) or 'auto'
    (the device when one is visible).  One amp_mask_contours call on the run lists (csrc/contours.hip, or contours_host.hip on the host:
    identical bytes), no mask is decoded.  ValueError for a bad connectivity or device and for masks of different sizes."""
    (first, off, ln, area2, length, xy), n = _contours_call("mask_contours", masks, connectivity, size, device)
    return [[{"xy": xy[off[r]: off[r] + ln[r]].copy(), "hole": bool(area2[r] < 0), "area": abs(int(area2[r])) // 2, "length": int(length[r])}
             for r in range(first[i], first[i + 1])] for i in range(n)]


def masks_to_polygons(masks, connectivity=2, size=None, device='auto', return_has_holes=False):
    """Every mask as polygons: per mask the list of its outer rings as flat float64 arrays [x0, y0, x1, y1, ...] -- what structures.PolygonMasks
    and a dataset dict's 'segmentation' hold, so masks_to_rle(PolygonMasks(result), size) gives the masks back with their holes filled.  Holes
    are dropped, as in detectron2's GenericMask.mask_to_polygons; return_has_holes: also a bool [N] array that says which masks had one.  An
    empty mask has no polygon.  Rings, coordinates, masks, connectivity and device as in mask_contours (one amp_mask_contours call)."""
    (first, off, ln, area2, length, xy), n = _contours_call("masks_to_polygons", masks, connectivity, size, device)
    polys = [[xy[off[r]: off[r] + ln[r]].astype(np.float64).reshape(-1) for r in range(first[i], first[i + 1]) if area2[r] > 0] for i in range(n)]
    if not return_has_holes:
        return polys
    return polys, np.array([bool((area2[first[i]: first[i + 1]] < 0).any()) for i in range(n)], dtype=bool)


# ---- morphology: a mask's shape changed by a distance (scipy.ndimage.binary_dilation / binary_erosion / binary_opening / binary_closing on one
# ---- decoded array per mask; Boundary IoU's cv2.erode) -------------------------------------------------------------------------------------------

def _morphology(who, masks, op, shape, radius, border_value, size, device, return_stats):
    """One rle.morphology call for a public function; every argument is checked before anything else happens"""
    if shape not in rle.MORPH_SHAPES:
        raise ValueError(f"{who}: shape = {shape!r} ('square', 'diamond' or 'disk')")
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not 0 <= int(radius) <= rle.MORPH_MAX_RADIUS:
        raise ValueError(f"{who}: radius = {radius!r} (an integer 0 .. {rle.MORPH_MAX_RADIUS})")
    if isinstance(border_value, bool) or border_value not in (0, 1):
        raise ValueError(f"{who}: border_value = {border_value!r} (0 or 1)")
    if str(device).lower() not in ("auto", "cpu", "cuda"):
        raise ValueError(f"{who}: device = {device!r} ('auto', 'cpu' or 'cuda')")
    masks, size = _unwrap_masks(masks, size)
    rles = masks_to_rle(masks, size, device)
    sizes = {tuple(int(v) for v in r["size"]) for r in rles}
    if len(sizes) > 1:
        raise ValueError(f"{who}: masks of different sizes {sorted(sizes)}")
    out, boxes, areas = rle.morphology(rles, op, shape, int(radius), int(border_value), ctx=_device_context(who, device, len(rles)),
                                       size=size if not rles else None, return_stats=True)
    return (out, {"area": areas, "bbox": boxes}) if return_stats else out


def dilate_masks(masks, shape='disk', radius=1, border_value=0, size=None, device='auto', return_stats=False):
    """Every mask grown by `radius` pixels: a pixel is set where a pixel of the mask lies within the structuring element -- 'square': Chebyshev
    distance <= radius (the 3 x 3 ones element iterated radius times), 'diamond': city-block distance (the 3 x 3 cross iterated), 'disk':
    Euclidean distance, dx^2 + dy^2 <= radius^2 (skimage.morphology.disk).  What scipy.ndimage.binary_dilation gives per decoded mask; the image
    clips the result and border_value plays no part.  Returns the list of RLE dicts in canonical form (what rle.encode gives for the dense
    result), length and order unchanged; return_stats: also a dict of 'area' int64 [N] and 'bbox' int64 [N, 4] = {r0, c0, r1, c1}, ends
    exclusive, zeros for an empty result.

    masks: anything masks_to_rle accepts (size=(h, w) for polygons), an Instances or an InstanceSet; radius: an integer 0 .. 1024, 0 returns the
    canonical form of the input; device: 'cpu' (host), 'cuda' (HIP device, an error without one) or 'auto' (the device when one is visible).
    One amp_mask_morphology call on the run lists (csrc/morphology.hip, or morphology_host.hip on the host: identical bytes), no mask is
    decoded.  ValueError before any device work for a bad shape, radius, border value or device and for masks of different sizes."""
    return _morphology("dilate_masks", masks, "dilate", shape, radius, border_value, size, device, return_stats)


def erode_masks(masks, shape='disk', radius=1, border_value=0, size=None, device='auto', return_stats=False):
    """Every mask shrunk by `radius` pixels: a pixel stays where the whole structuring element around it lies in the mask.  border_value is
    what the outside of the image counts as: 0 (scipy.ndimage.binary_erosion's default) erodes a mask from the image's sides, 1 (cv2.erode's
    default) does not.  A mask may come back empty.  Shapes, masks, radius, device, result and errors as in dilate_masks."""
    return _morphology("erode_masks", masks, "erode", shape, radius, border_value, size, device, return_stats)


def open_masks(masks, shape='disk', radius=1, border_value=0, size=None, device='auto', return_stats=False):
    """The opening of every mask, the dilation of its erosion: what the structuring element cannot enter is removed -- specks, spurs and the
    thin bridge that joins two particles predicted as one (mask_topology then counts two parts).  border_value is the erosion's.  Both passes
    run inside one amp_mask_morphology call; on the device the eroded masks never leave it.  Shapes, masks, radius, device, result and errors
    as in dilate_masks."""
    return _morphology("open_masks", masks, "open", shape, radius, border_value, size, device, return_stats)


def close_masks(masks, shape='disk', radius=1, border_value=1, size=None, device='auto', return_stats=False):
    """The closing of every mask, the erosion of its dilation: gaps the structuring element cannot enter are filled -- cracks, pinholes, narrow
    bays.  border_value is the erosion's and defaults to 1 HERE, unlike everywhere else: the dilation is clipped by the image, and an erosion
    that took the outside for background would then eat into a mask that touches the image's side; with 1 the closing is extensive, every
    mask is contained in its closing, at the border too.  border_value=0 is scipy.ndimage.binary_closing's default.  Both passes run inside
    one amp_mask_morphology call.  Shapes, masks, radius, device, result and errors as in dilate_masks."""
    return _morphology("close_masks", masks, "close", shape, radius, border_value, size, device, return_stats)


def boundary_bands(masks, width, side='inner', shape='square', border_value=0, size=None, device='auto', return_stats=False):
    """The band of `width` pixels along every mask's outline: side 'inner' = the mask minus its erosion (the pixels of the mask within `width`
    of a pixel outside it; with border_value 0 the outside of the image counts), 'outer' = its dilation minus the mask.  One pass of one
    amp_mask_morphology call.  width is the radius of dilate_masks; shapes, masks, device, result and errors as there."""
    if side not in ("inner", "outer"):
        raise ValueError(f"boundary_bands: side = {side!r} ('inner' or 'outer')")
    return _morphology("boundary_bands", masks, "band_in" if side == "inner" else "band_out", shape, width, border_value, size, device, return_stats)


def boundary_iou(gt, pred, matches=None, dilation_ratio=0.02, distance=None, size=None, device='auto'):
    """Boundary IoU (Cheng et al. 2021) of every matched pair: |band(g) AND band(p)| / |band(g) OR band(p)|, band(M) = M minus its erosion by the
    3 x 3 ones element iterated d times with the outside of the image as background -- boundary_bands(M, d, 'inner', 'square', 0), the published
    definition -- at d = `distance`, or max(1, round(dilation_ratio * sqrt(h^2 + w^2))).  Large instances score well on mask IoU whatever
    their outline; this score looks at the outline only.  matches: the dict of rle_instance_matcher or an [n, 2] array of (gt, pred) index
    pairs, None to take the true positives at IoU 0.5.  Returns {'boundary_iou': float64 [n] (NaN for a pair whose bands are both empty),
    'inter': int64 [n], 'union': int64 [n], 'distance': d}.

    gt, pred: anything masks_to_rle accepts (size=(h, w) for polygons and when both sides are empty), an Instances or an InstanceSet; device:
    'cpu', 'cuda' or 'auto'.  One amp_mask_morphology call for the matched ground-truth masks, one for the matched predictions, one
    amp_rle_pair_overlap; no mask is decoded.  ValueError for a bad distance, ratio, pair or device and for masks of different sizes."""
    if str(device).lower() not in ("auto", "cpu", "cuda"):
        raise ValueError(f"boundary_iou: device = {device!r} ('auto', 'cpu' or 'cuda')")
    if distance is not None and (isinstance(distance, bool) or not isinstance(distance, (int, np.integer)) or not 1 <= int(distance) <= rle.MORPH_MAX_RADIUS):
        raise ValueError(f"boundary_iou: distance = {distance!r} (an integer 1 .. {rle.MORPH_MAX_RADIUS}, or None for the ratio)")
    if distance is None and not (isinstance(dilation_ratio, (int, float, np.integer, np.floating)) and 0 <= float(dilation_ratio) < float("inf")):
        raise ValueError(f"boundary_iou: dilation_ratio = {dilation_ratio!r} (a finite share of the image diagonal, not negative)")
    gm, size = _unwrap_masks(gt, size)
    pm, size = _unwrap_masks(pred, size)
    g, p = masks_to_rle(gm, size, device), masks_to_rle(pm, size, device)
    h, w = _image_size("boundary_iou", g + p, size)
    d = int(distance) if distance is not None else max(1, int(round(float(dilation_ratio) * float(np.sqrt(float(h * h + w * w))))))
    if d > rle.MORPH_MAX_RADIUS:
        raise ValueError(f"boundary_iou: the band width {d} of a {h} x {w} image at ratio {dilation_ratio!r} exceeds {rle.MORPH_MAX_RADIUS}; pass distance=")
    if matches is None:
        matches = match_instances(iou_matrix(g, p), 0.5)
    pairs = np.asarray(matches["tp"] if isinstance(matches, dict) else matches, dtype=np.int64).reshape(-1, 2)
    for i, (a, b) in enumerate(pairs.tolist()):
        if not (0 <= a < len(g) and 0 <= b < len(p)):
            raise ValueError(f"boundary_iou: pair {i} = ({a}, {b}) is outside the {len(g)} ground-truth and {len(p)} predicted masks")
    n = len(pairs)
    ctx = _device_context("boundary_iou", device, n)
    bg = rle.morphology([g[a] for a in pairs[:, 0].tolist()], "band_in", "square", d, 0, ctx=ctx, size=(h, w))
    bp = rle.morphology([p[b] for b in pairs[:, 1].tolist()], "band_in", "square", d, 0, ctx=ctx, size=(h, w))
    inter, g_only, p_only = rle.pair_overlap(bg, bp, np.stack([np.arange(n), np.arange(n)], axis=1))
    union = inter + g_only + p_only
    with np.errstate(divide="ignore", invalid="ignore"):
        biou = inter.astype(np.float64) / union.astype(np.float64)
    return {"boundary_iou": biou, "inter": inter, "union": union, "distance": d}


def near_pairs(masks, gap=1, shape='disk', size=None, device='auto'):
    """Which instances touch or lie close together: the int64 [k, 2] index pairs i < j, in lexicographic order, of masks with a pixel of one
    within `gap` of a pixel of the other -- Euclidean distance for 'disk', Chebyshev for 'square', city-block for 'diamond'; exact for integer
    pixel offsets.  gap = 1 with 'square' is 8-touching, with 'diamond' 4-touching, gap = 0 overlapping.  The contact graph of a powder image,
    the near-neighbour graph of a set of carbides.  Pair (i, j) is reported where dilate(masks[i], gap) meets masks[j]; the distance is
    symmetric, so nothing is lost by looking at i < j only.

    One amp_mask_morphology call (the dilation) and one amp_rle_overlap_groups call (overlap_matrix) on the run lists.  masks, shape, device
    and errors as in dilate_masks; gap is its radius."""
    grown = _morphology("near_pairs", masks, "dilate", shape, gap, 0, size, device, False)
    if len(grown) < 2:
        return np.zeros((0, 2), np.int64)
    masks, size = _unwrap_masks(masks, size)
    meets = overlap_matrix(grown, masks_to_rle(masks, size, device), device=device) > 0
    return np.argwhere(np.triu(meets, 1)).astype(np.int64).reshape(-1, 2)


# ---- distance inside a mask (scipy.ndimage.distance_transform_edt on one decoded array per mask) ------------------------------------------------

def _mask_distance(who, masks, border_value, ncurve, want_map, size, device):
    """One rle.mask_distance call for a public function; every argument is checked before anything else happens"""
    if isinstance(border_value, bool) or border_value not in (0, 1):
        raise ValueError(f"{who}: border_value = {border_value!r} (0 or 1)")
    if str(device).lower() not in ("auto", "cpu", "cuda"):
        raise ValueError(f"{who}: device = {device!r} ('auto', 'cpu' or 'cuda')")
    masks, size = _unwrap_masks(masks, size)
    rles = masks_to_rle(masks, size, device)
    sizes = {tuple(int(v) for v in r["size"]) for r in rles}
    if len(sizes) > 1:
        raise ValueError(f"{who}: masks of different sizes {sorted(sizes)}")
    res = rle.mask_distance(rles, int(border_value), ncurve, want_map, ctx=_device_context(who, device, len(rles)),
                            size=size if not rles else None)
    return res + (int(rles[0]["size"][0]) if rles else 1,)            # and the image height: what a position col * h + row is split by


def mask_distance_maps(masks, border_value=0, squared=False, size=None, device='auto'):
    """How far inside its mask every pixel lies: per mask a dict {'bbox': (r0, c0, r1, c1), 'distance': array [r1 - r0, c1 - c0]} with the
    Euclidean distance of every mask pixel of the tight box (ends exclusive; zeros and an empty array for an empty mask) to the nearest pixel
    that is not in the mask, 0 outside the mask -- scipy.ndimage.distance_transform_edt on the decoded mask, cut to the box.  border_value 0:
    the pixels just outside the image are background as well (the mask padded by one zero on every side); 1: only pixels of the image count
    (scipy on the undecorated array).  squared=True gives the exact uint32 squared distances; otherwise float64, numpy's correctly rounded
    root of them.  A mask without background (border_value 1 and the full image) has rle.DIST_NONE, or inf, on every pixel: scipy leaves that
    case undefined.

    masks: anything masks_to_rle accepts (size=(h, w) for polygons), an Instances or an InstanceSet; device: 'cpu' (host), 'cuda' (HIP device,
    an error without one) or 'auto' (the device when one is visible).  One amp_mask_distance call on the run lists (csrc/mask_distance.hip, or
    mask_distance_host.hip on the host: identical bytes), no mask is decoded to the image; a pixel costs about as many steps as its distance.
    ValueError before any device work for a bad border value or device and for masks of different sizes."""
    _, boxes, _, maps, _ = _mask_distance("mask_distance_maps", masks, border_value, 0, True, size, device)
    out = []
    for b, m in zip(boxes.tolist(), maps):
        if not squared:
            none = m == rle.DIST_NONE
            m = np.sqrt(m.astype(np.float64))
            m[none] = np.inf
        out.append({"bbox": tuple(int(v) for v in b), "distance": m})
    return out


def inscribed_circles(masks, border_value=0, size=None, device='auto'):
    """The largest circle that fits into every mask, centred on a pixel: a dict of [N] arrays 'd2' (int64, the largest squared distance of a
    mask pixel to the nearest pixel outside the mask), 'radius' (float64, its root: the circle of that radius about the pixel's centre reaches
    the centre of the nearest outside pixel), 'row', 'col' (int64, the pixel that attains it, among equals the first in column-major order)
    and 'center_xy' ([N, 2] float64, (col + 0.5, row + 0.5) in the corner coordinates of mask_contours).  The particle size that a satellite
    or a ragged outline does not inflate; 2 * radius across a neck is its width.  An empty mask: d2 0, radius 0, row and col -1, center_xy
    NaN; a mask without background (border_value 1 and the full image): d2 rle.DIST_NONE, radius inf, pixel (0, 0).  A statistics-only
    amp_mask_distance call: no map, no curve.  masks, border_value, device and errors as in mask_distance_maps."""
    stats, _, _, _, h = _mask_distance("inscribed_circles", masks, border_value, 0, False, size, device)
    return _circles(stats, h)


def _circles(stats, h):
    """inscribed_circles' dict from amp_mask_distance's stats of masks of image height h"""
    d2, pos, area = stats[:, 0].copy(), stats[:, 1], stats[:, 3]
    some = area > 0
    radius = np.sqrt(d2.astype(np.float64))
    radius[d2 == rle.DIST_NONE] = np.inf
    row = np.where(some, pos % h, -1).astype(np.int64)
    col = np.where(some, pos // h, -1).astype(np.int64)
    xy = np.stack([col + 0.5, row + 0.5], axis=1).astype(np.float64).reshape(-1, 2)
    xy[~some] = np.nan
    return {"d2": d2.astype(np.int64), "radius": radius, "row": row, "col": col, "center_xy": xy}


def erosion_curve(masks, max_radius, border_value=0, size=None, device='auto'):
    """How many pixels of every mask lie deeper than r, for every r at once: int64 [N, max_radius + 1], column r = the pixels whose distance
    to the nearest pixel outside the mask exceeds r.  Column 0 is the area; with border_value 0 column r is the area of
    erode_masks(masks, 'disk', r, border_value=0) -- a pixel survives the disk of radius r exactly when no outside pixel lies within r of it
    --, the granulometry that costs one erode_masks call per radius otherwise.  max_radius: an integer 0 .. 1024.  One amp_mask_distance call
    with a curve, no map.  masks, border_value, device and errors as in mask_distance_maps; ValueError for a bad max_radius as well."""
    if isinstance(max_radius, bool) or not isinstance(max_radius, (int, np.integer)) or not 0 <= int(max_radius) <= rle.MORPH_MAX_RADIUS:
        raise ValueError(f"erosion_curve: max_radius = {max_radius!r} (an integer 0 .. {rle.MORPH_MAX_RADIUS})")
    return _mask_distance("erosion_curve", masks, border_value, int(max_radius) + 1, False, size, device)[2]


# ---- grey levels under a mask (skimage.measure.regionprops(..., intensity_image=img); img[RLE.decode(m)] per instance) ----------------------------

INTENSITY_KEYS = ("intensity_mean", "intensity_min", "intensity_max", "intensity_std", "centroid_weighted")
INTENSITY_ALIASES = {"mean_intensity": "intensity_mean", "min_intensity": "intensity_min", "max_intensity": "intensity_max",
                     "weighted_centroid": "centroid_weighted"}          # skimage's names before 0.19
RPROPS_INTENSITY_KEYS = INTENSITY_KEYS + tuple(INTENSITY_ALIASES)    # what region_properties takes with an intensity_image


def intensity_floats(vals):
    """THE derivation of the intensity columns from the exact integers of amp_mask_intensity (vals: the 8 ints {N, sum v, sum v^2, sum r v,
    sum c v, min, max, 0} of one mask and channel) -> dict of 'intensity_mean', 'intensity_min', 'intensity_max', 'intensity_std',
    'centroid_weighted-0', 'centroid_weighted-1'.  Both the device and the host path go through here, so they return identical bytes.  The
    mean sum v / N and the weighted centroid (sum r v / sum v, sum c v / sum v) are quotients of Python integers, rounded once; the standard
    deviation is the population's, sqrt((N sum v^2 - (sum v)^2) / N^2), with the difference that cancels formed in Python integers and the
    quotient rounded once before the root.  min and max stay integers.  An empty mask: NaN, and min / max 0; sum v = 0: a NaN centroid."""
    import math
    from fractions import Fraction
    N, sv, svv, srv, scv, mn, mx = (int(v) for v in vals[:7])
    nan = float("nan")
    out = {"intensity_mean": nan, "intensity_min": mn, "intensity_max": mx, "intensity_std": nan, "centroid_weighted-0": nan, "centroid_weighted-1": nan}
    if N:
        out["intensity_mean"] = sv / N
        out["intensity_std"] = math.sqrt(float(Fraction(N * svv - sv * sv, N * N)))
    if sv:
        out["centroid_weighted-0"], out["centroid_weighted-1"] = srv / sv, scv / sv
    return out


def _intensity_columns(who, keys, channels):
    """[(column name, intensity_floats' name, channel)] of `keys` (None: INTENSITY_KEYS) for an image of `channels` channels: named like
    regionprops_table, a column by the key as it was given, 'centroid_weighted-0', '-1', and with more than one channel a trailing '-ch'"""
    cols = []
    for k in (INTENSITY_KEYS if keys is None else keys):
        if k not in RPROPS_INTENSITY_KEYS:
            raise ValueError(f"{who}: unsupported key {k!r} (supported: {', '.join(RPROPS_INTENSITY_KEYS)})")
        base = INTENSITY_ALIASES.get(k, k)
        parts = [(f"{k}-{i}", f"{base}-{i}") for i in range(2)] if base == "centroid_weighted" else [(k, base)]
        for col, src in parts:
            cols += [(col, src, 0)] if channels == 1 else [(f"{col}-{ch}", src, ch) for ch in range(channels)]
    return cols


def _intensity_input(who, masks, img, size, device):
    """(rles, ctx) of an intensity call on img, the image as rle.intensity_image returns it; the device and the sizes are checked before
    anything else happens"""
    if str(device).lower() not in ("auto", "cpu", "cuda"):
        raise ValueError(f"{who}: device = {device!r} ('auto', 'cpu' or 'cuda')")
    masks, size = _unwrap_masks(masks, size)
    rles = masks_to_rle(masks, size if size is not None else img.shape[:2], device)
    sizes = {tuple(int(v) for v in r["size"]) for r in rles}
    if sizes - {img.shape[:2]}:
        raise ValueError(f"{who}: masks of sizes {sorted(sizes)} on an image of size {img.shape[:2]}")
    return rles, _device_context(who, device, len(rles))


def _intensity_table(cols, vals):
    rows = [[intensity_floats(v) for v in m] for m in vals.tolist()]
    return {col: np.array([r[ch][src] for r in rows], dtype=np.int64 if src in ("intensity_min", "intensity_max") else np.float64)
            for col, src, ch in cols}


def intensity_properties(masks, image, keys=None, size=None, device='auto'):
    """The grey levels of the micrograph under every mask, the intensity columns skimage.measure.regionprops_table(..., intensity_image=image)
    gives: a dict of column name -> np.ndarray [N].  keys: any of INTENSITY_KEYS -- 'intensity_mean', 'intensity_min', 'intensity_max',
    'intensity_std' (the population's), 'centroid_weighted' (columns '-0' row and '-1' column, in the full image's coordinates) -- or their
    older names 'mean_intensity', 'min_intensity', 'max_intensity', 'weighted_centroid' (the columns then carry the name that was given); None:
    all five.  With an image of C > 1 channels every column has a trailing '-ch' as skimage appends it: 'intensity_mean-0',
    'centroid_weighted-0-2'.  min and max are int64, the rest float64; an empty mask has NaN, and min / max 0; a mask over zeros only has a
    NaN centroid.  A region is ALL set pixels of one mask; overlapping masks do not see each other.

    masks: anything masks_to_rle accepts, an Instances or an InstanceSet; image: uint8, uint16 or bool (read as uint8) of shape [h, w] or
    [h, w, C], C <= 4, the masks' size.  A DEPARTURE FROM SKIMAGE: a float or signed image is a ValueError that names the dtype -- every
    number here derives from exact integer sums; quantise first.  device: 'cpu' (host), 'cuda' (HIP device, an error without one) or 'auto'
    (the device when one is visible).  One amp_mask_intensity call on the run lists (csrc/mask_intensity.hip, or mask_intensity_host.hip on
    the host: identical bytes), no mask is decoded; intensity_floats derives the floats for both paths.  UNPINNED PARITY: skimage is not part
    of this environment; the definitions are restated in DESIGN §7p and the tests hold the integers to NumPy and scipy.ndimage on decoded masks.
    ValueError before any device work for an unknown key, a bad image or device and an image of another size than the masks."""
    img, _ = rle.intensity_image("intensity_properties", image)
    cols = _intensity_columns("intensity_properties", keys, img.shape[2])
    rles, ctx = _intensity_input("intensity_properties", masks, img, size, device)
    vals, _ = rle.mask_intensity(rles, img, None, ctx=ctx)
    return _intensity_table(cols, vals)


def intensity_histograms(masks, image, bins=None, size=None, device='auto'):
    """The grey-level histogram of the micrograph under every mask: (hist, bin_edges) = uint32 [N, bins] (or [N, C, bins] for an image of
    shape [h, w, C]) counts and the int64 [bins + 1] edges; bin b holds the values bin_edges[b] <= v < bin_edges[b + 1], equal bins over the
    dtype's whole range.  bins: a power of two, at most 4096 and at most the dtype's levels; None: 256 for uint8, 1024 for uint16.  masks,
    image, device and errors as in intensity_properties; the same amp_mask_intensity call with a histogram."""
    img0 = np.asarray(image)
    img, depth = rle.intensity_image("intensity_histograms", image)
    bins = (256 if depth == 8 else 1024) if bins is None else bins
    if isinstance(bins, bool) or not isinstance(bins, (int, np.integer)) or not 1 <= int(bins) <= min(rle.INTENSITY_MAX_BINS, 1 << depth) or int(bins) & (int(bins) - 1):
        raise ValueError(f"intensity_histograms: bins = {bins!r} (a power of two, at most {min(rle.INTENSITY_MAX_BINS, 1 << depth)} for {img.dtype})")
    rles, ctx = _intensity_input("intensity_histograms", masks, img, size, device)
    shift = depth - (int(bins).bit_length() - 1)
    _, hist = rle.mask_intensity(rles, img, shift, ctx=ctx)
    return (hist[:, 0, :].copy() if img0.ndim == 2 else hist), np.arange(int(bins) + 1, dtype=np.int64) << shift


def intensity_quantiles(masks, image, q, size=None, device='auto'):
    """Quantiles of the grey levels under every mask, from the histogram: float64 [N] for a number q, [N, len(q)] for a sequence, with a
    trailing C for an image of shape [h, w, C].  The inverted-CDF rule, exact: the value of rank k = max(1, ceil(q N)) among the mask's N
    sorted values -- np.sort(img[mask])[k - 1] --, with q taken as the exact rational of the float; q = 0.5 is the (lower) median, 0 the
    minimum, 1 the maximum.  NaN for an empty mask.  uint8 images are resolved fully.  A uint16 image has more levels than the 4096 bins of a
    call: the result is then THE LOWER EDGE OF THE BIN of 16 levels that holds the quantile, a multiple of 16 at most 15 below the value.
    masks, image, device and errors as in intensity_properties; ValueError for a q outside [0, 1]."""
    from fractions import Fraction
    import math
    qs = np.asarray(q, dtype=np.float64)
    if qs.ndim > 1 or not np.all((qs >= 0) & (qs <= 1)):             # a NaN fails the comparison
        raise ValueError(f"intensity_quantiles: q = {q!r} (a number or a sequence of numbers in [0, 1])")
    img0 = np.asarray(image)
    img, depth = rle.intensity_image("intensity_quantiles", image)
    rles, ctx = _intensity_input("intensity_quantiles", masks, img, size, device)
    shift = max(depth - 12, 0)
    _, hist = rle.mask_intensity(rles, img, shift, ctx=ctx)
    cum = np.cumsum(hist.astype(np.int64), axis=2)
    out = np.full((len(rles), qs.size, img.shape[2]), np.nan)
    for j, qv in enumerate(qs.reshape(-1).tolist()):
        f = Fraction(qv)
        for i in range(len(rles)):
            N = int(cum[i, 0, -1])
            if N:
                k = max(1, math.ceil(f * N))
                for ch in range(img.shape[2]):
                    out[i, j, ch] = int(np.searchsorted(cum[i, ch], k, side="left")) << shift      # the first bin whose cumulated count reaches k
    out = out if img0.ndim == 3 else out[:, :, 0]
    return out[:, 0] if qs.ndim == 0 else out


# ---- overlap-free instances: the owner of every pixel (the labels[mask_i] = i + 1 loop over decoded masks) ---------------------------------------

def flatten_ranks(who, priority, n, scores=None, areas=None):
    """The uint32 ranks amp_flatten_instances orders the n instances by (the smallest rank owns a pixel, ties go to the lower index), None for
    index order.  priority 'score': higher score on top (scores required, NaN refused); 'area': smaller area on top (areas: a callable that
    returns them); 'index'; or an integer array of ranks, any integers.  Stable NumPy sorts on the host."""
    if isinstance(priority, str):
        p = priority.lower()
        if p == "index":
            return None
        if p == "score":
            if scores is None:
                raise ValueError(f"{who}: priority='score' needs scores (scores=..., or an Instances with a scores field)")
            s = np.asarray(scores.numpy() if hasattr(scores, "numpy") else scores, dtype=np.float64).reshape(-1)
            if len(s) != n:
                raise ValueError(f"{who}: {len(s)} scores for {n} masks")
            if np.isnan(s).any():
                raise ValueError(f"{who}: scores[{int(np.flatnonzero(np.isnan(s))[0])}] is NaN")
            key = -s
        elif p == "area":
            key = np.asarray(areas(), dtype=np.int64).reshape(-1)
        else:
            raise ValueError(f"{who}: priority = {priority!r} ('score', 'area', 'index' or an integer array of ranks)")
    else:
        key = np.asarray(priority)
        if key.ndim != 1 or len(key) != n or not (n == 0 or (np.issubdtype(key.dtype, np.integer) and key.dtype != bool)):
            raise ValueError(f"{who}: priority = {priority!r} ('score', 'area', 'index' or an array of {n} integer ranks)")
    rank = np.empty(n, dtype=np.uint32)
    rank[np.argsort(key, kind="stable")] = np.arange(n, dtype=np.uint32)          # the place in the order: equal keys keep their index order
    return rank


def _flatten_input(who, masks, priority, scores, size, device):
    """(rles, rank, (h, w), ctx) of a resolve_overlaps / instances_to_label_image call"""
    inst = masks.instances if hasattr(masks, "instances") and masks.instances is not None else masks
    if scores is None and hasattr(inst, "masks") and hasattr(inst, "image_size"):
        scores = getattr(inst, "scores", None)
    m, size = _unwrap_masks(masks, size)
    _device_context(who, device, 0)                                   # a bad device is refused before anything is computed
    rles = masks_to_rle(m, size, device)
    h, w = _image_size(who, rles, size)
    rles = [{"size": r["size"], "counts": rle._counts(r)} for r in rles]               # the strings are read once: the call takes the arrays

    def areas():                                                      # the odd counts of every list, summed without a loop over the masks
        if not rles:
            return np.zeros(0, np.int64)
        pool, off, ln = rle._pool([r["counts"] for r in rles])
        owner = np.repeat(np.arange(len(rles)), ln)
        odd = (np.arange(len(owner)) - np.repeat(off.astype(np.int64), ln)) & 1
        return np.bincount(owner, weights=pool[:len(owner)].astype(np.int64) * odd, minlength=len(rles)).astype(np.int64)

    rank = flatten_ranks(who, priority, len(rles), scores, areas)
    return rles, rank, (h, w), _device_context(who, device, len(rles))


def resolve_overlaps(masks, priority='score', scores=None, size=None, device='auto', return_stats=False):
    """The instances of an image made disjoint: every pixel several masks cover goes to ONE of them, the rest lose it.  Returns the list of RLE
    dicts in canonical form (what rle.encode gives for the dense result), length and order unchanged -- a mask may come back empty --; no two
    share a pixel, and their union is the union of the input.

    priority: which covering instance owns a pixel.  'score': the one of highest score (scores=..., or the `scores` field of an Instances /
    InstanceSet; NaN is refused); 'area': the one of smallest input area, so a satellite keeps its pixels on its particle; 'index': the first
    in the list; or an integer array of ranks, smallest on top.  Ties always go to the lower index.
    masks: anything masks_to_rle accepts (size=(h, w) for polygons and for no mask at all), an Instances or an InstanceSet; device: 'cpu'
    (host), 'cuda' (HIP device, an error without one) or 'auto' (the device when one is visible).  return_stats: also a dict of int64 arrays
    'area' [N] (of the input masks), 'visible_area' [N], 'bbox' [N, 4] ({r0, c0, r1, c1} of the visible pixels, ends exclusive, zeros for
    none) and 'pixels' [3]: the pixels of the image covered by no mask, by one, by two or more.

    One amp_flatten_instances call on the run lists (csrc/flatten.hip, or flatten_host.hip on the host: identical bytes); no mask is decoded.
    Pass the result to psd, mask_areas or region_properties to count every pixel once.  ValueError for a bad priority or device and for masks
    of different sizes."""
    rles, rank, (h, w), ctx = _flatten_input("resolve_overlaps", masks, priority, scores, size, device)
    stats, boxes, pixels, counts = rle.flatten_instances(rles, rank, ctx=ctx, size=(h, w))
    pool, off, ln = rle._pool(counts)
    out = [{"size": [h, w], "counts": c} for c in rle.counts_to_strings(pool, off, ln)]
    if not return_stats:
        return out
    return out, {"area": stats[:, 0].copy(), "visible_area": stats[:, 1].copy(), "bbox": boxes, "pixels": pixels}


def instances_to_label_image(masks, priority='score', scores=None, size=None, device='auto'):
    """The instances of an image as ONE int32 [H, W] label image: instance i's visible pixels hold i + 1, pixels no mask covers 0 -- the form
    ImageJ, skimage and get_ddicts('label') read; label_image_to_rle(result, 'label') returns the non-empty visible masks in index order.
    masks, priority, scores, device: as resolve_overlaps; size=(h, w) is required when there is no mask.  One amp_flatten_instances
    call that emits no list (csrc/flatten.hip: one launch; or flatten_host.hip on the host: identical bytes)."""
    rles, rank, (h, w), ctx = _flatten_input("instances_to_label_image", masks, priority, scores, size, device)
    return rle.flatten_instances(rles, rank, ctx=ctx, emit=False, return_labels=True, size=(h, w))[4]


def _label_runs_input(who, image, kind):
    """The image of label_image_to_rle as amp_label_runs takes it -- uint8 foreground flags or int32 ids -- and whether id 0 is background."""
    img = np.asarray(image)
    if img.ndim != 2:
        raise ValueError(f"{who}: a 2-D image is required, got shape {img.shape}")
    if kind == "binary":
        return np.ascontiguousarray(img != 0, dtype=np.uint8), True
    if not np.issubdtype(img.dtype, np.integer):
        raise ValueError(f"{who}: kind='label' takes an integer image, got {img.dtype}")
    if img.size and (int(img.min()) < -2 ** 31 or int(img.max()) > 2 ** 31 - 1):
        raise ValueError(f"{who}: ids {int(img.min())} .. {int(img.max())} do not fit int32")
    return np.ascontiguousarray(img, dtype=np.int32), not (img.size and int(img.min()) < 0)       # the reference skips unique[0] only if it is 0


def label_image_to_rle(image, kind='label', connectivity=2, device='auto', return_labels=False):
    """The instances of an annotation image in one call: what get_ddicts('binary' | 'label') makes of it (ampis/data_utils.py:412-428 -- label
    the foreground, one dense `ann == u` mask per instance, a box and an encode of each) without the dense masks.

    kind 'binary': nonzero pixels are foreground and the instances are its connected components -- connectivity 1: 4 neighbours, 2: 8
    neighbours, the default of skimage.measure.label in 2-D -- numbered 1 .. K by the row-major position of their first pixel, the numbering of
    scipy.ndimage.label and skimage.measure.label.  kind 'label': an integer image of ids, one instance per distinct id in ascending order
    (disconnected parts belong together); id 0 is background unless a negative id occurs, as in the reference.

    Returns (rles, boxes, areas, ids): COCO dicts {'size': [h, w], 'counts': bytes}, float64 [N, 4] boxes [x1, y1, x2, y2] with inclusive
    maxima exactly as data_utils.extract_boxes gives, int64 [N] pixel counts and int64 [N] component numbers or ids; with return_labels also the
    int32 label image (instance number 1 .. N, 0 for background).  device: 'cpu' (host), 'cuda' (HIP device, an error without one) or 'auto'
    (the device when one is visible).  One amp_label_runs evaluation (csrc/label_runs.hip, or label_runs_host.hip on the host): the same bytes
    on both.  UNPINNED PARITY: skimage is not part of this environment and the reference stores no output of this path; the tests pin it to
    scipy.ndimage.label plus the host codec.
    ValueError for an image that is not 2-D, a non-integer image or ids beyond int32 in 'label' kind, a bad kind, connectivity or device."""
    k = kind.lower() if isinstance(kind, str) else kind
    if k not in ("binary", "label"):
        raise ValueError(f"label_image_to_rle: kind = {kind!r} ('binary' or 'label')")
    if connectivity not in (1, 2):
        raise ValueError(f"label_image_to_rle: connectivity = {connectivity!r} (1: 4 neighbours, 2: 8 neighbours)")
    img, zero_bg = _label_runs_input("label_image_to_rle", image, k)
    ctx = _device_context("label_image_to_rle", device, img.size)
    if img.size == 0:
        empty = ([], np.zeros((0, 4)), np.zeros(0, np.int64), np.zeros(0, np.int64))
        return empty + (np.zeros(img.shape, np.int32),) if return_labels else empty
    res = rle.label_runs(img, k, connectivity, zero_bg, ctx=ctx, return_labels=return_labels)
    ids, bx, areas, pool, off, ln = res[:6]
    size = [int(img.shape[0]), int(img.shape[1])]
    rles = [{"size": list(size), "counts": s} for s in rle.counts_to_strings(pool, off, ln)]
    boxes = np.stack([bx[:, 1], bx[:, 0], bx[:, 3] - 1, bx[:, 2] - 1], axis=1).astype(np.float64) if len(ids) else np.zeros((0, 4))
    out = (rles, boxes, areas.astype(np.int64), ids.astype(np.int64))
    return out + (res[6],) if return_labels else out


def label_components(image, connectivity=2, device='auto'):
    """The import swap for skimage.measure.label on a 2-D image: nonzero pixels are foreground, the int32 image of their connected components
    (connectivity 1: 4 neighbours, 2: 8 neighbours) numbered from 1 by the row-major position of their first pixel, 0 for background -- what
    scipy.ndimage.label gives with the cross or the full 3 x 3 structure.  device: as label_image_to_rle."""
    if connectivity not in (1, 2):
        raise ValueError(f"label_components: connectivity = {connectivity!r} (1: 4 neighbours, 2: 8 neighbours)")
    img, _ = _label_runs_input("label_components", image, "binary")
    ctx = _device_context("label_components", device, img.size)
    if img.size == 0:
        return np.zeros(img.shape, np.int32)
    return rle.label_runs(img, "binary", connectivity, True, ctx=ctx, return_labels=True)[6]


def regionprops_table(label_image, properties=RPROPS_DEFAULT_KEYS):
    """The import swap for the one use AMPIS makes of skimage.measure.regionprops_table: a 2-D integer label image (0 = background) -> dict of
    column -> array with one entry per label in ascending order.  The run lists of all labels come from one label_image_to_rle call."""
    cols = _rprops_columns(properties)
    lab = np.asarray(label_image)
    if lab.ndim != 2 or not np.issubdtype(lab.dtype, np.integer):
        raise ValueError(f"regionprops_table: a 2-D integer label image is required, got shape {lab.shape} {lab.dtype}")
    if lab.size and (int(lab.min()) < -2 ** 31 or int(lab.max()) > 2 ** 31 - 1):       # ids beyond int32: one encode per label
        rles = [rle.encode(np.asfortranarray(lab == v)) for v in np.unique(lab) if v != 0]
    else:
        rles, _, _, ids = label_image_to_rle(lab, "label") if lab.size else ([], None, None, [])
        rles = [r for r, v in zip(rles, ids) if v != 0]              # 0 is an instance of its own beside negative ids; never a label here
    if not rles:
        return {c: np.zeros(0) for c in cols}
    return region_properties(rles, properties)


# ---- all-pairs overlap and mask areas (ampis/applications/powder.py:80-83, ampis/structures.py:536-583) -----------------------------------------

def overlap_matrix(a, b, device='auto', size=None):
    """[len(a), len(b)] int64: the exact pixel count of a[i] AND b[j] for every pair of masks of one image -- what the reference gets from one
    RLE.merge(intersect=True) + RLE.area per pair (ampis/applications/powder.py:82).  One amp_rle_overlap_groups call with one group.  a, b:
    anything masks_to_rle accepts (size=(h, w) for polygons); device: 'cpu' (host), 'cuda' (HIP device, an error without one) or 'auto' (the
    device when one is visible); the paths return identical bytes.  ValueError for a bad `device` and for masks of different sizes."""
    ra, rb = masks_to_rle(a, size, device), masks_to_rle(b, size, device)
    ctx = _device_context("overlap_matrix", device, len(ra) and len(rb))
    try:
        return rle.overlap_groups([ra], [rb], ctx=ctx)[0][0]
    except ValueError as e:
        raise ValueError(str(e).replace("overlap_groups: group 0 holds", "overlap_matrix: a / b hold")) from None


def _shoelace_area(x, y):
    """Area of a simple polygon from its vertices (ampis/structures.py:586-610)."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    return 0.5 * np.abs(np.dot(x, np.roll(y, 1)) - np.dot(y, np.roll(x, 1)))


def mask_areas(masks):
    """Area in pixels of every mask, with the reference's dispatch (ampis/structures.py:536-583): an ndarray [N, H, W] -> its pixel sums
    (unsigned); PolygonMasks -> the shoelace area of each instance's FIRST polygon (float64, as the reference: further polygons of an instance
    are not counted); a list of RLE dicts, RLEBitMasks or anything with .rle -> the run sums (uint32, like pycocotools' area); an object with
    .masks or .instances -> the areas of those; any other list -> the list of its elements' areas."""
    if isinstance(masks, np.ndarray):
        return masks.sum(axis=(1, 2), dtype=np.uint)
    if isinstance(masks, PolygonMasks):
        return np.asarray([_shoelace_area(np.asarray(inst[0]).reshape(-1)[::2], np.asarray(inst[0]).reshape(-1)[1::2]) for inst in masks.polygons])
    if isinstance(masks, RLEBitMasks) or hasattr(masks, "rle"):
        return rle.area(list(masks.rle))
    if isinstance(masks, (list, tuple)) and len(masks) and isinstance(masks[0], dict):
        return rle.area(list(masks))
    if isinstance(masks, BitMasks):
        return mask_areas(masks.tensor.numpy().astype(bool))
    if hasattr(masks, "masks"):
        return mask_areas(masks.masks)
    if hasattr(masks, "instances"):
        return mask_areas(masks.instances)
    if isinstance(masks, (list, tuple)):
        return [mask_areas(x) for x in masks]
    raise NotImplementedError(f"Not implemented for type {type(masks)}")


# ---- detection / segmentation performance overlays (ampis/analyze.py:19-51, 502-699; ampis/structures.py:717-774) ------------------------------

def align_instance_sets(a, b):
    """Lists of instance sets a, b -> (a_ordered, b_ordered): the items of `a` whose file NAME (the last part of .filepath) some item of `b`
    carries, in the order of `a`, and beside each the item of `b` of that name (ampis/analyze.py:19-51).  Items of either list without a partner
    are left out -- the tutorial uses exactly that to drop images labelled in one dataset only --; of several items of `b` with one name the
    last is taken."""
    from pathlib import Path
    by_name = {Path(item.filepath).name: item for item in b}
    a_ordered, b_ordered = [], []
    for item in a:
        x = by_name.get(Path(item.filepath).name, None)
        if x is not None:
            a_ordered.append(item)
            b_ordered.append(x)
    return a_ordered, b_ordered


def _unwrap_masks(obj, size):
    """(masks, size) of an InstanceSet-like (.instances), an Instances-like (.masks, .image_size) or the masks themselves"""
    if hasattr(obj, "instances") and obj.instances is not None:
        obj = obj.instances
    if hasattr(obj, "masks") and hasattr(obj, "image_size"):
        return obj.masks, (tuple(int(v) for v in obj.image_size) if size is None else size)
    return obj, size


def _image_size(who, rles, size):
    sizes = {tuple(int(v) for v in r["size"]) for r in rles}
    if size is not None:
        sizes.add(tuple(int(v) for v in size))
    if len(sizes) > 1:
        raise ValueError(f"{who}: masks of different sizes {sorted(sizes)}")
    if not sizes:
        raise ValueError(f"{who}: size=(height, width) is required when there is no mask to take it from")
    return sizes.pop()


def masks_to_bitmask_array(masks, size=None):
    """Any of the mask forms -> bool ndarray [N, H, W] (ampis/structures.py:717-774): the decode for callers that really want the dense array.
    masks: a bool ndarray (returned as it is), anything masks_to_rle accepts (size=(h, w) for polygons), an Instances or an InstanceSet.  Polygons
    are rasterised like everywhere in this module (masks_to_rle), not by skimage.  Nothing in this package calls it."""
    if isinstance(masks, np.ndarray):
        assert masks.dtype == bool, "a mask array must be boolean"
        return masks
    m, size = _unwrap_masks(masks, size)
    rles = masks_to_rle(m, size)
    h, w = _image_size("masks_to_bitmask_array", rles, size)
    if not rles:
        return np.zeros((0, h, w), dtype=bool)
    return np.stack([rle.decode(r).astype(bool) for r in rles])


SEG_LABELS = {"reduced": ["TP", "FN", "FP", "other"],                                             # ampis/analyze.py:675, 689: the 'all' list names
              "all": ["Other", "TP", "FN", "TP+FN", "FP", "TP+FP", "FN+FP", "TP+FN+FP"]}          # code 0 as well, one more than the classes
SEG_COLORS = {"reduced": [[0.5, 0., 1.], [1., 0., 0.], [0., 1., 1.], [1., 1., 0.]],               # ampis/analyze.py:664-672, 685-688
              "all": [[0.153, 0.153, 0.000], [0.286, 1., 0.], [1., 0.857, 0.], [1., 0., 0.], [0., 0.571, 1.], [0., 1., 0.571], [0.285, 0., 1.]]}


def seg_class_map(gt, pred, match_results=None, mode='reduced', size=None, device='auto'):
    """Every pixel of the image classed by the matched pairs (the computation of ampis/analyze.py:626-692): for the pairs match_results['tp']
    TP = OR (g & p), FN = OR (g & ~p), FP = OR (~g & p), code = TP + 2 FN + 4 FP.  mode 'reduced': the classes TP only, FN only, FP only and
    'other' (more than one of them); 'all': the seven codes 1 .. 7.  Returns {'masks': K RLE dicts over the whole image, 'labels', 'colors'
    ([K, 3], the reference's tables), 'pixel_counts': int64 [8] pixels of every code, 'match_results'}.

    gt, pred: anything masks_to_rle accepts (size=(h, w) for polygons and for two empty sides), an Instances or an InstanceSet; match_results:
    the dict of rle_instance_matcher, None to call it at the default threshold; device: 'cpu' (host), 'cuda' (HIP device, an error without one)
    or 'auto' (the device when one is visible).  One amp_seg_class_map call on the run lists (csrc/seg_class_map.hip, or mask_analysis_host.hip on the
    host: identical bytes); no mask is decoded.  ValueError for an unknown mode or device and for masks of different sizes."""
    mode = str(mode).lower()
    if mode not in SEG_LABELS:
        raise ValueError(f"seg_class_map: mode = {mode!r} ('reduced' or 'all')")
    gm, size = _unwrap_masks(gt, size)
    pm, size = _unwrap_masks(pred, size)
    g, p = masks_to_rle(gm, size, device), masks_to_rle(pm, size, device)
    h, w = _image_size("seg_class_map", g + p, size)
    if match_results is None:
        match_results = match_instances(iou_matrix(g, p), 0.5)
    pairs = np.asarray(match_results["tp"], dtype=np.int64).reshape(-1, 2)
    for i, (a, b) in enumerate(pairs.tolist()):
        if not (0 <= a < len(g) and 0 <= b < len(p)):
            raise ValueError(f"seg_class_map: match_results['tp'][{i}] = ({a}, {b}) is outside the {len(g)} ground-truth and {len(p)} predicted masks")
    ctx = _device_context("seg_class_map", device, len(pairs))
    counts, pixels = rle.seg_class_map(g, p, pairs, mode, ctx=ctx, size=(h, w))
    return {"masks": [{"size": [h, w], "counts": rle.counts_to_string(c)} for c in counts], "labels": list(SEG_LABELS[mode]),
            "colors": np.array(SEG_COLORS[mode]), "pixel_counts": pixels, "match_results": match_results}


def seg_perf_iset(gt_masks, pred_masks, match_results=None, mode='reduced', size=None, device='auto'):
    """ampis/analyze.py:589-699 with its arguments and its return: (iset, [colors, labels]) -- an InstanceSet whose instances hold the class masks
    of seg_class_map ('masks': RLEMasks, 'colors', 'boxes': zeros [K, 4]) for visualize.display_iset, and the colour table and labels of the
    mode.  size, device: as seg_class_map.  Departures from the reference are listed in DESIGN 7g."""
    r = seg_class_map(gt_masks, pred_masks, match_results, mode, size, device)
    masks = RLEMasks(r["masks"])
    colors = [r["colors"], r["labels"]]
    iset = InstanceSet()
    iset.instances = Instances(image_size=masks.rle[0]["size"], **{"masks": masks, "colors": colors[0], "boxes": np.zeros((len(masks), 4))})
    return iset, colors


def _xyxy_boxes(inst, rles):
    """[N, 4] boxes of an Instances-like (its `boxes` field, an ndarray or a Boxes) or, without one, the tight XYXY boxes of the run lists"""
    if inst is not None and hasattr(inst, "boxes"):
        b = inst.boxes
        return b if type(b) == np.ndarray else b.tensor.numpy()
    tight = [rle.bbox(m) for m in rles]
    return np.array([(0, 0, 0, 0) if b is None else b for b in tight], dtype=np.float64).reshape(-1, 4)


def det_perf_iset(gt, pred, match_results=None, colormap=None, tp_gt=False, size=None):
    """ampis/analyze.py:502-586 with its arguments and its return convention: an InstanceSet of the true-positive, false-positive and false-negative
    INSTANCES in that order ('masks': RLEMasks, 'boxes', 'colors': the class colour tiled per instance) for visualize.display_iset; returned as
    (iset, colormap) when `colormap` is None -- the default {'TP', 'FP', 'FN'} table -- and alone when the caller gave one.  True positives are
    shown by their predicted mask and box, by the ground truth's with tp_gt.  gt, pred: InstanceSets or Instances (masks, boxes, image size) or
    anything masks_to_rle accepts (the boxes are then the tight boxes of the masks; size=(h, w) for polygons)."""
    gi = gt.instances if hasattr(gt, "instances") else (gt if hasattr(gt, "masks") and hasattr(gt, "image_size") else None)
    pi = pred.instances if hasattr(pred, "instances") else (pred if hasattr(pred, "masks") and hasattr(pred, "image_size") else None)
    gm, size = _unwrap_masks(gt, size)
    pm, size = _unwrap_masks(pred, size)
    gt_masks, pred_masks = masks_to_rle(gm, size), masks_to_rle(pm, size)
    h, w = _image_size("det_perf_iset", gt_masks + pred_masks, size)
    if match_results is None:
        match_results = match_instances(iou_matrix(gt_masks, pred_masks), 0.5)
    return_colormap = colormap is None
    gt_bbox, pred_bbox = _xyxy_boxes(gi, gt_masks), _xyxy_boxes(pi, pred_masks)
    if colormap is None:
        colormap = {"TP": np.asarray([0.5, 0., 1.], float), "FP": np.asarray([0., 1., 1.], float), "FN": np.asarray([1., 0., 0.], float)}
    tp = np.asarray(match_results["tp"], dtype=np.int64).reshape(-1, 2)
    tp_idx = tp[:, 0] if tp_gt else tp[:, 1]
    tp_src, tp_box = (gt_masks, gt_bbox) if tp_gt else (pred_masks, pred_bbox)
    fp_idx, fn_idx = np.asarray(match_results["fp"], dtype=np.int64).reshape(-1), np.asarray(match_results["fn"], dtype=np.int64).reshape(-1)
    parts = [([tp_src[i] for i in tp_idx], tp_box[tp_idx], colormap["TP"]), ([pred_masks[i] for i in fp_idx], pred_bbox[fp_idx], colormap["FP"]),
             ([gt_masks[i] for i in fn_idx], gt_bbox[fn_idx], colormap["FN"])]
    masks = RLEMasks([m for part in parts for m in part[0]])
    bbox = np.concatenate([part[1] for part in parts], axis=0)
    colors = np.concatenate([np.tile(part[2], (len(part[0]), 1)) for part in parts], axis=0)
    iset = InstanceSet()
    iset.instances = Instances(image_size=[h, w], **{"masks": masks, "boxes": bbox, "colors": colors})
    if return_colormap:
        return iset, colormap
    return iset


# ---- instance overlays (detectron2 Visualizer.overlay_instances: utils/visualizer.py draw_binary_mask + draw_box per instance) -----------------

def render_order(boxes, n):
    """The Visualizer's draw order of n instances: large boxes first so that small instances stay visible, the given order without boxes."""
    return np.argsort(-np.prod(boxes[:, 2:] - boxes[:, :2], axis=1)) if boxes is not None else np.arange(n)


def render_inputs(colors, alpha, boxes, h, w):
    """What amp_render_instances looks up, built with the expressions of Visualizer.draw_binary_mask / draw_box so that the bytes agree by
    construction: (tables uint8 [n, 256, 3] -- the blend of every pixel value --, edge colours uint8 [n, 3], int32 [n, 4] boxes rounded and
    clipped to the h x w image or None, box colours uint8 [n, 3]).  colors: [n, 3] in [0, 1]; 0 <= alpha <= 1."""
    col = np.asarray(colors, dtype=np.float64).reshape(-1, 3) * 255.0
    tables = (np.arange(256.)[None, :, None] * (1.0 - alpha) + (col * alpha)[:, None, :] + 0.5).astype(np.uint8)
    edge_rgb = np.clip(col * 0.7, 0, 255).astype(np.uint8)
    box_rgb = np.clip(col, 0, 255).astype(np.uint8)
    ibox = None
    if boxes is not None:
        b = np.rint(np.asarray(boxes, dtype=np.float64).reshape(-1, 4))           # round half to even, like round() in draw_box
        if not np.isfinite(b).all():
            raise ValueError("render_instances: boxes must be finite")
        ibox = np.stack([np.clip(b[:, 0], 0, w - 1), np.clip(b[:, 1], 0, h - 1), np.clip(b[:, 2], 0, w - 1), np.clip(b[:, 3], 0, h - 1)],
                        axis=1).astype(np.int32)
    return tables, edge_rgb, ibox, box_rgb


def render_instances(image, masks=None, boxes=None, colors=None, alpha=0.5, edge=True, order=None, line_width=None, size=None, device='auto'):
    """The overlay of Visualizer.overlay_instances at image scale without its labels, as a new uint8 [H, W, 3] array: for every instance in draw
    order the mask's pixels blended with its colour (uint8(v (1 - alpha) + 255 colour alpha + 0.5), rounded once per covering instance), its edge
    pixels -- a 4-neighbour outside the mask, or the image's border -- set to 0.7 of the colour when `edge`, then its XYXY box framed
    `line_width` wide (None: max(1, round(max(H, W) / 600))).  Byte for byte what Visualizer.draw_binary_mask + draw_box give per instance.

    image: [H, W, 3] (or grey [H, W]); masks: anything masks_to_rle accepts (size=(h, w) defaults to the image's), None for boxes only; boxes:
    [n, 4] XYXY, a Boxes, or None; colors: [n, 3] in [0, 1], None for the Visualizer's palette; order: the draw order, None for the
    Visualizer's rule (large boxes first); device: 'cpu' (host), 'cuda' (HIP device, an error without one) or 'auto' (the device when one is
    visible).  One amp_render_instances call on the run lists (csrc/render.hip, or mask_analysis_host.hip on the host: identical bytes); no
    mask is decoded.  ValueError for alpha or a colour outside [0, 1], masks of another size than the image, a bad `device`."""
    from .utils.visualizer import Visualizer, _palette
    img = np.asarray(image)
    if img.ndim == 2:
        img = img[:, :, None]
    if img.shape[2] == 1:
        img = np.repeat(img, 3, axis=2)
    img = np.ascontiguousarray(np.clip(img[:, :, :3], 0, 255).astype(np.uint8))
    h, w = img.shape[:2]
    rles = masks_to_rle(masks, (h, w) if size is None else size, device) if masks is not None else None
    bx = Visualizer._box_array(boxes)
    n = len(bx) if bx is not None else (len(rles) if rles is not None else 0)
    if rles is not None and len(rles) != n:
        raise ValueError(f"render_instances: {len(rles)} masks for {n} boxes")
    if not 0.0 <= alpha <= 1.0:
        raise ValueError(f"render_instances: alpha = {alpha!r} (0 .. 1)")
    col = _palette(n) if colors is None else np.asarray(colors, dtype=np.float64).reshape(n, -1)[:, :3]
    if n and not (np.isfinite(col).all() and col.min() >= 0.0 and col.max() <= 1.0):
        raise ValueError("render_instances: colours must lie in [0, 1]")
    ctx = _device_context("render_instances", device, n)
    if n == 0:
        return img.copy()
    order = render_order(bx, n) if order is None else np.asarray(order, dtype=np.int64).reshape(-1)
    lw = int(line_width if line_width is not None else max(1, round(max(h, w) / 600)))
    tables, edge_rgb, ibox, box_rgb = render_inputs(col[order], alpha, bx[order] if bx is not None else None, h, w)
    return rle.render_instances(img, [rles[i] for i in order] if rles is not None else None, tables, edge_rgb if edge else None, ibox, box_rgb, lw, ctx=ctx)
