"""amp_mask_intensity on the device (csrc/mask_intensity.hip): every case of tests/mask_intensity_cases.py -- without a histogram and at two
hist_shifts of its depth -- against img[mask] with exact integer sums and against the host path, byte for byte; the device's bytes against its
own second call; the large sums; the capacity protocol and the refusals with a context (made before any device work); the Python callers on
the device.  The cases are the smallest at which the kernels can go wrong: the edges of the 64 x 64 transpose tile in both directions, runs
across column ends, the cut between two work items, runs at odd positions at both depths, one to four channels."""
import pytest

import mask_intensity_cases as cs
from test_mask_intensity import (N_CHUNKS, PER_CHUNK, PUBLIC, REFUSALS, check_capacity_protocol, check_large_sums, check_public_functions, check_refusal,
                                 public_bytes, public_pool, public_results)

pytestmark = pytest.mark.gpu


def check_on_the_device(gpu_ctx, name):
    dev = cs.check_case(name, ctx=gpu_ctx)
    assert dev == cs.check_case(name), name
    assert dev == cs.check_case(name, ctx=gpu_ctx), name                                 # its own second call


@pytest.mark.parametrize("name", cs.HAND)
def test_device_equals_the_reference_and_the_host(gpu_ctx, name):
    check_on_the_device(gpu_ctx, name)


@pytest.mark.parametrize("chunk", range(N_CHUNKS))
def test_device_equals_the_reference_and_the_host_on_seeded_cases(gpu_ctx, chunk):
    for name in cs.SEEDED[chunk * PER_CHUNK: (chunk + 1) * PER_CHUNK]:
        check_on_the_device(gpu_ctx, name)


def test_large_sums_on_the_device(gpu_ctx):
    assert check_large_sums(ctx=gpu_ctx) == check_large_sums() == check_large_sums(ctx=gpu_ctx)


def test_capacity_protocol_on_the_device(gpu_ctx):
    for kw in (dict(), dict(name="tile_65x64", shift=15)):
        dev = check_capacity_protocol(ctx=gpu_ctx, **kw)
        host = check_capacity_protocol(**kw)
        assert all(dev[key].tobytes() == host[key].tobytes() for key in dev)            # the words behind the result are untouched on both paths


@pytest.mark.parametrize("what, kw", REFUSALS, ids=[f"{i}-{r[0][:28]}" for i, r in enumerate(REFUSALS)])
def test_bad_arguments_are_refused_before_any_device_work(gpu_ctx, what, kw):
    check_refusal(what, kw, ctx=gpu_ctx)


def test_public_functions_on_the_device(gpu_ctx):
    check_public_functions("cuda")
    for name in PUBLIC:                                              # 'auto' takes the device: the same bytes as the host
        for kind in public_pool()[1]:
            host = public_bytes(public_results(name, "cpu", kind))
            assert public_bytes(public_results(name, "auto", kind)) == host and public_bytes(public_results(name, "cuda", kind)) == host
