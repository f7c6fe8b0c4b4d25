"""Golden vectors of `ampis.applications.powder` (_rle_satellite_match, PowderSatelliteImage.compute_satellite_metrics, satellite_measurements,
psd) made BY THE REFERENCE ITSELF, run in the build container (where /root/reference exists) in the manner of make_edge_distance_vectors.py:
the reference is imported UNMODIFIED on the façade.  Only data is written, to tests/golden/powder_vectors.json.gz; tests/test_powder.py and
tests/test_powder_gpu.py hold the product to it.

    python tests/golden/make_powder_vectors.py        # needs /root/reference and the built library

Inputs are NOT copied: they are the five images that 'particle-results' and 'satellite-results' of tests/golden/rle_pickles.json.gz share by
file_name, named here by file and image index.  The horizontal field widths are this generator's own (the pickles carry none): a different
one per image, so that a per-image c differs from a common one.  Floats are written as JSON numbers, which Python reads back bit for bit.
"""
import base64
import contextlib
import gzip
import io
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REFERENCE = "/root/reference"
sys.path.insert(0, ROOT)
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
from ampis.applications import powder  # noqa: E402
from ampis.structures import InstanceSet, RLEMasks  # noqa: E402
from detectron2.structures import Instances  # noqa: E402

from ampis_amd import analyze  # noqa: E402

LIMIT = 523152          # the largest fixture so far (rle_pickles.json.gz)
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "rle_pickles.json.gz")
PARTICLES, SATELLITES = "examples/powder/data/particle-results.pickle", "examples/powder/data/satellite-results.pickle"
THRESHOLDS = (0.5, 0.9)
HFW = lambda k: 768.0 + 12.5 * k          # um, image k of the five
C_FLOAT = 0.37


def shared_images(gold):
    """[(file index, image index) of the particles, (file index, image index) of the satellites] of every shared file_name, in particle order"""
    files = {f["path"]: (i, f) for i, f in enumerate(gold["files"])}
    (pi, pf), (si, sf) = files[PARTICLES], files[SATELLITES]
    sat = {im["file_name"]: k for k, im in enumerate(sf["images"])}
    return [((pi, k), (si, sat[im["file_name"]])) for k, im in enumerate(pf["images"]) if im["file_name"] in sat]


def iset(gold, ref, hfw):
    im = gold["files"][ref[0]]["images"][ref[1]]
    h, w = im["image_size"]
    rles = [{"size": [h, w], "counts": base64.b64decode(c)} for c in im["counts_b64"]]
    inst = Instances((h, w), masks=RLEMasks(rles), boxes=np.asarray(im["boxes"], np.float32).reshape(-1, 4), class_idx=np.asarray(im["classes"]))
    return InstanceSet(mask_format="bitmask", filepath=im["file_name"], instances=inst, HFW=hfw, HFW_units="um", randomstate=0)


def plain(v):
    if isinstance(v, dict):
        return [[int(k), plain(x)] for k, x in v.items()]
    if isinstance(v, np.ndarray):
        return v.tolist()
    if isinstance(v, (list, tuple)):
        return [plain(x) for x in v]
    return v.item() if isinstance(v, np.generic) else v


def main():
    with gzip.open(GOLD, "rt") as f:
        gold = json.load(f)
    refs = shared_images(gold)
    assert len(refs) == 5, refs
    psis = [powder.PowderSatelliteImage(iset(gold, p, HFW(k)), iset(gold, s, HFW(k))) for k, (p, s) in enumerate(refs)]
    images, ties, empties = [], 0, 0
    for (p, s), psi in zip(refs, psis):
        rec = {"particles": list(p), "satellites": list(s), "matches": {}}
        for t in THRESHOLDS:
            with np.errstate(all="ignore"):
                m = powder._rle_satellite_match(psi.particles.instances, psi.satellites.instances, t)
            rec["matches"][repr(t)] = {k: plain(v) for k, v in m.items()}
            if t == 0.5:
                assert len(m["satellite_matches"]) >= 100, len(m["satellite_matches"])
                psi.matches = m
        rec["metrics"] = {k: plain(v) for k, v in psi.compute_satellite_metrics().items()}
        inter = analyze.overlap_matrix(psi.satellites.instances.masks, psi.particles.instances.masks, device="cpu")
        best = inter.max(axis=1)
        ties += int(((inter == best[:, None]).sum(axis=1)[best > 0] > 1).sum())
        empties += int((analyze.mask_areas(psi.particles.instances.masks) == 0).sum() + (analyze.mask_areas(psi.satellites.instances.masks) == 0).sum())
        print(p, s, len(psi.particles.instances), "particles", len(psi.satellites.instances), "satellites", len(m["satellite_matches"]), "matches at", t)
        images.append(rec)
    assert ties >= 1 and empties >= 1, (ties, empties)
    sink = io.StringIO()
    with contextlib.redirect_stdout(sink):
        meas = powder.satellite_measurements(psis, print_summary=True, output_dict=True)
    cl = [HFW(k) / 1536 * (1 + 0.01 * k) for k in range(5)]
    cs = [("float", C_FLOAT, "length"), ("list", cl, "length"), ("tuple", (cl, "um"), "length"), ("pixels", None, "pixels")]
    psd = []
    with contextlib.redirect_stdout(io.StringIO()):
        for xv in ("d_eq", "area"):
            for yv in ("cvf", "counts"):
                for name, c, dist in cs + ([("hfw", None, "length")] if (xv, yv) == ("d_eq", "cvf") else []):
                    r = powder.psd(psis, xvals=xv, yvals=yv, c=c, distance=dist, plot=False, return_results=True)
                    psd.append({"xvals": xv, "yvals": yv, "c_kind": name, "c": plain(c), "distance": dist, "x": plain(r["x"]), "y": plain(r["y"]),
                                "x_label": r["x_label"], "y_label": r["y_label"]})
    out = {"made_by": "tests/golden/make_powder_vectors.py: ampis.applications.powder of rccohn/AMPIS imported unmodified on the ampis_amd facade",
           "inputs": "tests/golden/rle_pickles.json.gz, [file index, image index]", "hfw": [HFW(k) for k in range(5)], "hfw_units": "um",
           "ties_for_the_maximum": ties, "empty_masks": empties, "images": images,
           "measurements": {k: plain(v) for k, v in meas.items()}, "measurements_printed": sink.getvalue(), "psd": psd}
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "powder_vectors.json.gz")
    with gzip.open(dst, "wt", compresslevel=9) as f:
        json.dump(out, f, separators=(",", ":"))
    size = os.path.getsize(dst)
    print("wrote", dst, size, "bytes;", ties, "ties,", empties, "empty masks")
    assert size < LIMIT, f"{size} bytes: not below the largest fixture ({LIMIT})"


if __name__ == "__main__":
    main()
