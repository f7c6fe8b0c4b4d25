"""amp_mask_distance on the device (csrc/mask_distance.hip): every case of tests/mask_distance_cases.py -- both border values, ncurve 0, 1, 9
and 1025, with and without the map -- against scipy on the decoded masks and against the host path, byte for byte; the device's bytes against
its own second call; the largest sides; the capacity protocol and the refusals with a context (made before any device work); the Python
callers on the device.  The cases are the smallest at which the kernel can go wrong: pieces that cross the 64-row tiles, the ends of the binary
search in a column slice, both border rules, ties, the sentinel."""
import pytest

import mask_distance_cases as cs
from test_mask_distance import (N_CHUNKS, PER_CHUNK, PUBLIC, REFUSALS, check_capacity_protocol, check_largest, check_public_functions, check_refusal,
                                check_the_2_30_image, public_bytes, public_results)

pytestmark = pytest.mark.gpu


def check_on_the_device(gpu_ctx, name):
    for b in cs.BORDERS:
        dev = cs.check_case(name, b, ctx=gpu_ctx)
        assert dev == cs.check_case(name, b), (name, b)
        assert dev == cs.check_case(name, b, ctx=gpu_ctx), (name, b)                     # its own second call


@pytest.mark.parametrize("name", cs.HAND)
def test_device_equals_the_reference_and_the_host(gpu_ctx, name):
    check_on_the_device(gpu_ctx, name)


@pytest.mark.parametrize("chunk", range(N_CHUNKS))
def test_device_equals_the_reference_and_the_host_on_seeded_cases(gpu_ctx, chunk):
    for name in cs.SEEDED[chunk * PER_CHUNK: (chunk + 1) * PER_CHUNK]:
        check_on_the_device(gpu_ctx, name)


@pytest.mark.parametrize("name", cs.LARGEST)
def test_the_largest_sides_on_the_device(gpu_ctx, name):
    assert check_largest(name, ctx=gpu_ctx) == check_largest(name) == check_largest(name, ctx=gpu_ctx)


def test_the_2_30_image_on_the_device(gpu_ctx):
    assert check_the_2_30_image(ctx=gpu_ctx) == check_the_2_30_image() == check_the_2_30_image(ctx=gpu_ctx)


def test_capacity_protocol_on_the_device(gpu_ctx):
    for kw in (dict(), dict(name="checkerboard", b=1, ncurve=1)):
        dev = check_capacity_protocol(ctx=gpu_ctx, **kw)
        host = check_capacity_protocol(**kw)
        assert all(dev[key].tobytes() == host[key].tobytes() for key in dev)            # the words behind the result are untouched on both paths


@pytest.mark.parametrize("what, kw", REFUSALS, ids=[f"{i}-{r[0][:28]}" for i, r in enumerate(REFUSALS)])
def test_bad_arguments_are_refused_before_any_device_work(gpu_ctx, what, kw):
    check_refusal(what, kw, ctx=gpu_ctx)


def test_public_functions_on_the_device(gpu_ctx):
    check_public_functions("cuda")
    for name in PUBLIC:                                              # 'auto' takes the device: the same bytes as the host
        for b in cs.BORDERS:
            host = public_bytes(public_results(name, "cpu", b))
            assert public_bytes(public_results(name, "auto", b)) == host and public_bytes(public_results(name, "cuda", b)) == host
