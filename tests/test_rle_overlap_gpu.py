"""amp_rle_overlap_groups on the device (csrc/rle_overlap.hip): every case of tests/rle_overlap_cases.py against the brute-force reference,
the device's bytes against the host's and against its own second call, the five fixture micrographs in one grouped call, the refusals (made
before any device work), analyze.overlap_matrix(device='cuda' / 'auto'), and calls with nothing to do."""
import numpy as np
import pytest

from ampis_amd import analyze, rle

import rle_overlap_cases as cs
from test_powder import fixture_images
from test_rle_overlap import HOSTILE, check_hostile, raw_call

pytestmark = pytest.mark.gpu


def _bytes(res):
    return [x.tobytes() for part in res for x in part]


@pytest.mark.parametrize("name", cs.NAMES)
def test_device_counts_equal_the_brute_force_and_the_host_and_repeat(gpu_ctx, name):
    dev = cs.check_case(name, ctx=gpu_ctx)
    groups = cs.cases()[name]
    a, b = [g[0] for g in groups], [g[1] for g in groups]
    assert _bytes(dev) == _bytes(rle.overlap_groups(a, b)) == _bytes(rle.overlap_groups(a, b, ctx=gpu_ctx))


def test_all_small_cases_as_groups_of_one_call(gpu_ctx):
    """every 40 x 50 case and the three-group case as the groups of ONE call: tiles of many groups share the launch"""
    names = [n for n in cs.NAMES if n not in ("large_offsets", "full_image_at_the_limit")]
    groups = [g for n in names for g in cs.cases()[n]]
    inters, aa, ab = rle.overlap_groups([g[0] for g in groups], [g[1] for g in groups], ctx=gpu_ctx)
    for k, g in enumerate(groups):
        assert np.array_equal(inters[k], g[2]) and np.array_equal(aa[k], g[3]) and np.array_equal(ab[k], g[4]), k


def test_raw_bytes_of_the_device_equal_the_host(gpu_ctx):
    a = [[0, 6], [1, 2, 3], [1, 2, 1]]
    b = [[0, 1, 5], [6], [2, 4], [0, 4], [2, 1, 1]]
    host = raw_call(a, b, [0, 2, 3], [0, 3, 5], [2, 4], [3, 1])
    dev = raw_call(a, b, [0, 2, 3], [0, 3, 5], [2, 4], [3, 1], ctx=gpu_ctx)
    assert host[0] == dev[0] == 0 and dev[1].tolist() == [1, 0, 4, 0, 0, 1, 2, 1]
    assert all(h.tobytes() == d.tobytes() for h, d in zip(host[1:], dev[1:]))


def test_fixture_micrographs_in_one_grouped_call_equal_the_host(gpu_ctx):
    psis = fixture_images()
    sats, parts = [list(p.satellites.instances.masks.rle) for p in psis], [list(p.particles.instances.masks.rle) for p in psis]
    host, dev, again = rle.overlap_groups(sats, parts), rle.overlap_groups(sats, parts, ctx=gpu_ctx), rle.overlap_groups(sats, parts, ctx=gpu_ctx)
    assert _bytes(host) == _bytes(dev) == _bytes(again)
    assert [i.shape for i in dev[0]] == [(len(s), len(p)) for s, p in zip(sats, parts)]
    live = sum(int((i > 0).sum()) for i in dev[0])
    assert 500 < live < 2000                                       # a few hundred overlapping pairs an image, of about 30 000
    for i, a_s, a_p in zip(*dev):                                  # an intersection is no larger than either mask
        assert (i <= a_s[:, None]).all() and (i <= a_p[None, :]).all()


@pytest.mark.parametrize("what, kw", HOSTILE, ids=[f"{i}-{h[0][:24]}" for i, h in enumerate(HOSTILE)])
def test_hostile_arguments_are_refused_before_any_device_work(gpu_ctx, what, kw):
    check_hostile(what, kw, ctx=gpu_ctx)


def test_overlap_matrix_on_the_device(gpu_ctx):
    g = cs.cases()["dense_stripes"][0]
    cpu, gpu, auto = (analyze.overlap_matrix(g[0], g[1], device=d) for d in ("cpu", "cuda", "auto"))
    assert cpu.dtype == gpu.dtype == np.int64 and cpu.tobytes() == gpu.tobytes() == auto.tobytes() and np.array_equal(gpu, g[2])


def test_nothing_to_do(gpu_ctx):
    assert rle.overlap_groups([], [], ctx=gpu_ctx) == ([], [], [])
    g = cs.cases()["tile_3x67"][0]
    inters, aa, ab = rle.overlap_groups([[], g[0]], [g[1], []], ctx=gpu_ctx)                    # groups without a pair
    assert [i.shape for i in inters] == [(0, 67), (3, 0)] and np.array_equal(aa[1], g[3]) and np.array_equal(ab[0], g[4])
    empty = [cs.enc(np.zeros((33, 17), bool))] * 5
    inters, aa, ab = rle.overlap_groups([empty], [empty], ctx=gpu_ctx)                          # masks without a pixel
    assert inters[0].shape == (5, 5) and not inters[0].any() and not aa[0].any() and not ab[0].any()
    assert analyze.overlap_matrix([], g[1], device="cuda").shape == (0, 67)
