"""The references of amp_mask_distance hold each other (no GPU needed): scipy's transform with integer squared distances from its indices
against the all-pairs evaluation on every case small enough for it, the Python transcription of the rule of csrc/mask_distance.h against
scipy on every hand case and a share of the seeded ones -- and the references tell the three seeded defects from the rule: an off-by-one in the
column distance, the border ignored, the tie taken in row-major order."""
import numpy as np
import pytest

import mask_distance_cases as cs
import mask_distance_ref as ref

SMALL = [name for name in cs.HAND + cs.SEEDED[:60] if max(cs.size(name)) <= 12]


def test_there_are_small_cases_of_every_kind():
    assert len(SMALL) >= 12 and {"image_1x1", "square_2x2", "full_image", "checkerboard", "rectangles_3x5_and_5x3"} <= set(SMALL)


@pytest.mark.parametrize("b", cs.BORDERS)
def test_scipy_equals_the_all_pairs_evaluation(b):
    for name in SMALL:
        for m in cs.get(name)["masks"]:
            assert ref.scipy_d2(m, b).tolist() == ref.brute_d2(m, b).tolist(), (name, b)


@pytest.mark.parametrize("b", cs.BORDERS)
def test_the_rule_of_the_header_equals_scipy(b):
    for name in cs.HAND + cs.SEEDED[:40]:
        for m in cs.get(name)["masks"]:
            assert ref.walk_d2(m, b).tolist() == ref.scipy_d2(m, b).tolist(), (name, b)


def test_the_sentinel_and_the_empty_mask():
    full, none = np.ones((3, 4), bool), np.zeros((3, 4), bool)
    for fn in (ref.scipy_d2, ref.brute_d2, ref.walk_d2):
        assert fn(full, 1).tolist() == [[ref.NONE] * 4] * 3 and fn(none, 1).tolist() == [[0] * 4] * 3
        assert fn(full, 0).tolist() == [[1, 1, 1, 1], [1, 4, 4, 1], [1, 1, 1, 1]]
    out = ref.outputs(full, ref.scipy_d2(full, 1), (3,))
    assert out["stats"] == [ref.NONE, 0, 0, 12] and out["box"] == [0, 0, 3, 4] and out["curve"] == {3: [12, 12, 12]}
    assert out["map"].dtype == np.uint32 and out["map"].tolist() == [[ref.NONE] * 4] * 3
    assert ref.outputs(none, ref.scipy_d2(none, 0), (2,))["stats"] == [0, 0, 0, 0] and ref.outputs(none, none * 1, (2,))["curve"] == {2: [0, 0]}


def caught(defect):
    """the (case, border value) pairs on which the defective evaluation differs from the reference"""
    out = []
    for name in cs.HAND:
        for b in cs.BORDERS:
            for m in cs.get(name)["masks"]:
                good = ref.outputs(m, ref.scipy_d2(m, b), (9,))
                if defect == "tie":
                    bad = ref.outputs(m, ref.scipy_d2(m, b), (9,), row_major_tie=True)
                else:
                    bad = ref.outputs(m, ref.walk_d2(m, b, g_off_by_one=defect == "g", ignore_border=defect == "border"), (9,))
                if good["stats"] != bad["stats"] or good["curve"] != bad["curve"] or good["map"].tobytes() != bad["map"].tobytes():
                    out.append((name, b))
                    break
    return out


def test_an_off_by_one_in_the_column_distance_is_caught():
    hit = caught("g")
    assert ("rectangles_3x5_and_5x3", 0) in hit and ("disk", 1) in hit and len(hit) >= 20


def test_an_ignored_border_is_caught():
    hit = caught("border")
    assert all(b == 0 for _, b in hit)                               # the defect is the rule at border_value 1
    assert {"full_image", "touching_all_four_sides", "single_row_image", "single_column_image", "image_1x1"} <= {name for name, _ in hit}


def test_a_row_major_tie_is_caught():
    # ties within one row or one column have the same first pixel in both orders (the 2 x 2 square, the rectangles); the second checkerboard
    # mask has d2 = 1 everywhere and starts at (1, 0) by columns, at (0, 1) by rows
    assert {("ring", 0), ("ring", 1), ("checkerboard", 0), ("checkerboard", 1)} <= set(caught("tie"))
    m = cs.get("checkerboard")["masks"][1]
    assert ref.outputs(m, ref.scipy_d2(m, 1))["stats"][:2] == [1, 1] and ref.outputs(m, ref.scipy_d2(m, 1), row_major_tie=True)["stats"][:2] == [1, 7]
    m = cs.get("square_2x2")["masks"][0]                             # rows 2 .. 3 of columns 3 .. 4 of a 5 x 6 image: (2, 3) is the first of four equals
    assert ref.outputs(m, ref.scipy_d2(m, 0))["stats"] == [1, 3 * 5 + 2, 4, 4]
