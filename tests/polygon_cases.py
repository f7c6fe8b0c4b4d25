"""The polygon inputs of the polygons_to_rle tests (tests/test_polygons_to_rle.py on the host, tests/test_polygons_to_rle_gpu.py on the device):
named hand cases, each on the smallest image that shows it, a seeded generator, and the two references every result is held to, byte for byte:

  (a) ref_oracle       oracle.train.fr_poly (a loop-for-loop restatement of pycocotools rleFrPoly) per polygon, united with oracle.rle.merge (dense
                       decode, OR, encode): shares no code with the library;
  (b) ref_composition  rle.merge(rle.frPyObjects(...)) per instance: the per-polygon path amp_polygons_to_rle replaces and is defined by.

A case is (name, h, w, instances), instances a list of per-instance polygon lists, a polygon flat [x0, y0, x1, y1, ...]."""
import functools

import numpy as np

SEEDS = 300
SEED_SIZES = ((37, 53), (64, 64), (1, 40), (40, 1), (130, 70), (65, 129))


def _rect(x0, y0, x1, y1):
    return [x0, y0, x1, y0, x1, y1, x0, y1]


def zigzag(h=128, w=512, k=48):
    """k vertices alternating x = 1.5 / w - 1.5 over y = 2.25 .. h - 2.25: every edge crosses all columns -- 19 571 runs in one polygon on 128 x 512"""
    ys = np.linspace(2.25, h - 2.25, k)
    xy = np.empty(2 * k)
    xy[0::2] = np.where(np.arange(k) % 2 == 0, 1.5, w - 1.5)
    xy[1::2] = ys
    return xy.tolist()


def many_triangles(n=5000, h=64, w=96):
    rng = np.random.default_rng(5000)
    c = rng.uniform([-2, -2], [w + 2, h + 2], size=(n, 1, 2))
    return [[np.round((c[i] + rng.uniform(-4, 4, size=(3, 2))) * 4) .reshape(-1) / 4] for i in range(n)]


def _grid_of_squares(count, h, w):
    """count squares of side 4.5 on a lattice of pitch 3.25 columns x 3.5 rows: neighbours overlap, the last ones leave the image"""
    per_row = 12
    return [_rect(1.0 + 3.25 * (i % per_row), 0.5 + 3.5 * (i // per_row), 5.5 + 3.25 * (i % per_row), 5.0 + 3.5 * (i // per_row)) for i in range(count)]


def hand_cases():
    tri, sq = [2, 2, 5, 2, 5, 5], [1, 1, 8, 1, 8, 8, 1, 8]
    star = [8, 1.5, 9.75, 6, 14.5, 6.25, 10.5, 9, 12.25, 14, 8, 10.75, 3.5, 14.25, 5.5, 9, 1.25, 6.5, 6.25, 6]
    cases = [
        ("ingest_two_instances", 10, 10, [[sq], [tri]]),
        ("ingest_one_instance", 10, 10, [[sq, tri]]),
        ("rect_covers_pixel_0", 8, 8, [[_rect(-1, -1, 4, 4)]]),
        ("rect_reaches_last_pixel", 8, 8, [[_rect(3, 3, 9, 9)]]),
        ("overhang_left", 37, 53, [[_rect(-10, 10, 8, 20)]]),
        ("overhang_right", 37, 53, [[_rect(45, 10, 70, 20)]]),
        ("overhang_top", 37, 53, [[_rect(10, -10, 20, 8)]]),
        ("overhang_bottom", 37, 53, [[_rect(10, 30, 20, 50)]]),
        ("overhang_all", 37, 53, [[_rect(-10, -10, 70, 50)]]),
        ("triangle_leaves_sideways", 37, 53, [[[40.3, 5.2, 80.7, 18.1, 44.9, 30.6]], [[-30.2, 3.1, 12.6, 17.7, -8.4, 33.3]]]),
        ("entirely_outside", 37, 53, [[_rect(100, 100, 120, 120)], [_rect(-40, -40, -20, -20)], [_rect(60, 5, 80, 25)]]),
        ("half_and_quarter_pixels", 16, 16, [[[1.5, 2.25, 9.75, 3.5, 7.25, 11.5, 2.5, 8.75]], [[0.5, 0.5, 15.5, 0.5, 15.5, 15.5, 0.5, 15.5]],
                                             [[0.25, 0.75, 15.75, 0.25, 15.25, 15.75, 0.75, 15.25]]]),
        ("one_vertex", 12, 12, [[[3, 4]], [[3.5, 4.5]]]),
        ("two_vertices", 12, 12, [[[2, 2, 9, 7]], [[2, 3, 2, 9]], [[1, 5, 10, 5]]]),
        ("repeated_vertices", 12, 12, [[[2, 2, 2, 2, 9, 2, 9, 9, 9, 9, 2, 9]], [[2, 2, 9, 2, 9, 9, 2, 9, 2, 2, 9, 2, 9, 9, 2, 9]]]),
        ("zero_area_sliver", 16, 16, [[[2, 3, 12, 9, 7, 6]], [[2, 3, 12, 3, 2, 3]], [[4, 1, 4, 13, 4, 1]]]),
        ("horizontal_and_vertical_edges", 16, 16, [[[2, 2, 13, 2, 13, 6, 7, 6, 7, 13, 2, 13]]]),
        ("bow_tie", 16, 16, [[[2, 2, 12, 12, 12, 2, 2, 12]], [[1.5, 3, 14, 11.5, 14, 3, 1.5, 11.5]]]),
        ("same_polygon_twice", 16, 16, [[star, star]], ),
        ("same_polygon_three_times", 16, 16, [[star, star, star]]),
        ("nested_overlapping_disjoint", 24, 24, [[_rect(2, 2, 20, 20), _rect(6, 6, 12, 12)], [_rect(2, 2, 12, 12), _rect(8, 8, 20, 20)],
                                                 [_rect(1, 1, 6, 6), _rect(14, 15, 22, 23)], [star, _rect(0, 0, 23, 23), [20, 20, 23, 20, 21.5, 23.5]]]),
        ("seventy_polygons", 37, 53, [_grid_of_squares(70, 37, 53), [_rect(3, 3, 9, 9)]]),
        ("image_1x40", 1, 40, [[_rect(3, -1, 17, 2)], [[5, 0, 30, 0, 18, 1]], [_rect(-3, -3, 50, 3)]]),
        ("image_40x1", 40, 1, [[_rect(-1, 3, 2, 17)], [[0, 5, 0, 30, 1, 18]], [_rect(-3, -3, 3, 50)]]),
        ("image_65x129", 65, 129, [[_rect(0.5, 0.5, 128.5, 64.5)], [[3, 60, 126, 2, 127.5, 64, 64.25, 10.5]], [_rect(63, -5, 66, 70), _rect(-5, 31, 140, 34)]]),
        ("zigzag", 128, 512, [[zigzag()]]),
        ("many_instances", 64, 96, many_triangles()),
    ]
    return [(name, h, w, [[np.asarray(p, np.float64).reshape(-1) for p in inst] for inst in insts]) for name, h, w, insts in cases]


def seeded_case(i):
    """seed i: one instance of 1-4 star polygons of 1-12 vertices around centres in and around the image"""
    rng = np.random.default_rng(i)
    h, w = SEED_SIZES[i % len(SEED_SIZES)]
    polys = []
    for _ in range(int(rng.integers(1, 5))):
        k = int(rng.integers(1, 13))
        cx, cy = rng.uniform(-0.2, 1.2) * w, rng.uniform(-0.2, 1.2) * h
        ang = np.sort(rng.uniform(0, 2 * np.pi, k))
        if rng.random() < 0.3:
            rng.shuffle(ang)
        r = rng.uniform(0, 0.6 * max(h, w), k)
        xy = np.stack([cx + r * np.cos(ang), cy + r * np.sin(ang)], axis=1).reshape(-1)
        step = (1.0, 0.5, 0.25, 0.1, None)[int(rng.integers(0, 5))]
        if step is not None:
            xy = np.round(xy / step) * step
        polys.append(np.ascontiguousarray(xy, np.float64))
    return f"seed_{i}", h, w, [polys]


def seeded_cases():
    return [seeded_case(i) for i in range(SEEDS)]


def micrograph_cases():
    """all instances of both fixture micrographs (tests/golden/via_subset.json), 1024 x 1536"""
    import seg_perf_data as D
    out = []
    for fn in D.file_names():
        polys, _, (h, w) = D.gt_polygons(fn)
        out.append((fn, h, w, polys))
    return out


def ref_oracle(instances, h, w):
    """(a): the counts strings from oracle.train.fr_poly per polygon and oracle.rle.merge"""
    from oracle import rle as orle
    from oracle.train import fr_poly
    out = []
    for inst in instances:
        parts = [{"size": [h, w], "counts": orle.counts_to_string(fr_poly([float(v) for v in p], h, w))} for p in inst]
        out.append(bytes(orle.merge(parts)["counts"]))
    return out


def ref_composition(instances, h, w):
    """(b): the counts strings of today's per-polygon composition"""
    from ampis_amd import rle
    return [bytes(rle.merge(rle.frPyObjects([np.asarray(p).reshape(-1).tolist() for p in inst], h, w))["counts"]) for inst in instances]


@functools.lru_cache(maxsize=None)
def all_cases():
    """name -> (h, w, instances) of every hand, seeded and micrograph case"""
    return {name: (h, w, insts) for name, h, w, insts in hand_cases() + seeded_cases() + micrograph_cases()}


@functools.lru_cache(maxsize=None)
def references(name):
    """((a), (b)) of a case, computed once and shared by the tests that need them"""
    h, w, insts = all_cases()[name]
    return ref_oracle(insts, h, w), ref_composition(insts, h, w)


def box_and_area(r):
    """({r0, c0, r1, c1}, area) of an RLE dict the way amp_polygons_to_rle reports them: rle.bbox / rle.area, zeros for an empty mask"""
    from ampis_amd import rle
    b = rle.bbox(r)
    return ([0, 0, 0, 0] if b is None else [b[1], b[0], b[3], b[2]]), rle.area(r)
