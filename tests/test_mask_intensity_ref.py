"""The references of amp_mask_intensity hold each other (no GPU needed): img[mask] with exact integer sums against scipy.ndimage's sum / minimum /
maximum / histogram over a label array on every hand case and a share of the seeded ones, the Python transcription of the host path's rule
against both -- and the references tell the three seeded defects from the rule: the row and the column swapped, a column taken to end one
pixel late, v * v formed in 32 bits."""
import pytest

import mask_intensity_cases as cs
import mask_intensity_ref as ref

SHARE = cs.HAND + cs.SEEDED[:90]


@pytest.mark.parametrize("part", range(3))
def test_indexing_equals_ndimage(part):
    for name in SHARE[part::3]:
        c = cs.get(name)
        want = cs.expected(name)
        for i, m in enumerate(c["masks"]):
            assert ref.ndimage_vals(m, c["img"]) == want["vals"][i], (name, i)
            for s in want["hist"]:
                assert ref.ndimage_hist(m, c["img"], s) == want["hist"][s][i], (name, i, s)


def test_the_rule_of_the_host_path_equals_both():
    from ampis_amd import rle
    for name in cs.HAND + cs.SEEDED[:30]:
        if cs.get(name)["masks"].size > 3 * 70 * 70:                 # the Python loop is slow: the two cases of many pixels are left to the others
            continue
        c = cs.get(name)
        for i, r in enumerate(cs.rles(name)):
            assert ref.walk_vals(rle._counts(r), c["img"]) == cs.expected(name)["vals"][i], (name, i)


def test_the_empty_mask_and_one_pixel():
    import numpy as np
    img = np.array([[3, 7], [11, 200]], np.uint8)
    none, one = np.zeros((2, 2), bool), np.array([[False, False], [False, True]])
    for fn in (ref.index_vals, ref.ndimage_vals):
        assert fn(none, img) == [[0] * 8] and fn(one, img) == [[1, 200, 40000, 200, 200, 200, 200, 0]]
    for fn in (ref.index_hist, ref.ndimage_hist):
        assert fn(none, img, 7) == [[0, 0]] and fn(one, img, 7) == [[0, 1]] and fn(np.ones((2, 2), bool), img, 2)[0][:3] == [1, 1, 1]
    assert ref.walk_vals([3, 1], img) == [[1, 200, 40000, 200, 200, 200, 200, 0]] and ref.walk_vals([4], img) == [[0] * 8]


def caught(**defect):
    """the cases on which the defective evaluation differs from the reference"""
    from ampis_amd import rle
    out = []
    for name in cs.HAND:
        c = cs.get(name)
        if c["masks"].size > 3 * 70 * 70:
            continue
        for i, r in enumerate(cs.rles(name)):
            if ref.walk_vals(rle._counts(r), c["img"], **defect) != cs.expected(name)["vals"][i]:
                out.append(name)
                break
    return out


def test_a_swap_of_row_and_column_is_caught():
    hit = caught(swap_rc=True)
    assert {"image_1x65", "image_65x1", "tile_63x65", "runs_at_column_ends", "channels_3", "overlapping_masks"} <= set(hit) and len(hit) >= 20
    assert "constant_0_u8" not in hit and "image_1x1" not in hit    # nothing to weigh, nowhere to go


def test_a_column_taken_to_end_one_pixel_late_is_caught():
    hit = caught(column_end_off_by_one=True)
    assert {"runs_at_column_ends", "runs_at_column_ends_u16", "tile_64x64", "zero_length_runs"} <= set(hit)
    assert "an_empty_mask_between_two_others" not in hit and "min_on_the_first_and_max_on_the_last_pixel" not in hit      # no run reaches a column end


def test_a_square_formed_in_32_bits_is_caught():
    hit = caught(square_in_32_bits=True)
    assert {"constant_65535", "max_on_the_first_and_min_on_the_last_pixel", "runs_starting_at_odd_positions_u16", "image_1x65"} <= set(hit)
    assert all(cs.depth(name) == 16 for name in hit)                 # 255^2 fits
