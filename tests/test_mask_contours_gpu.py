"""amp_mask_contours on the device (csrc/contours.hip): every case of tests/contours_cases.py at both connectivities against the dense edge walk
and against the host path, byte for byte; the device's bytes against its own second call; the capacity protocol and the refusals with a
context (made before any device work); the largest sides; the Python callers on the device."""
import pytest

import contours_cases as cs
from test_mask_contours import (PUBLIC, REFUSALS, check_capacity_protocol, check_public_functions, check_refusal, public_bytes, public_results)

pytestmark = pytest.mark.gpu


def check_on_the_device(gpu_ctx, name, connectivity):
    dev = cs.check_case(name, connectivity, ctx=gpu_ctx)
    assert cs.result_bytes(dev) == cs.result_bytes(cs.run(name, connectivity)), (name, connectivity)
    assert cs.result_bytes(dev) == cs.result_bytes(cs.run(name, connectivity, ctx=gpu_ctx)), (name, connectivity)    # its own second call


@pytest.mark.parametrize("connectivity", cs.CONNECTIVITIES)
@pytest.mark.parametrize("name", cs.HAND)
def test_device_equals_the_reference_and_the_host(gpu_ctx, name, connectivity):
    check_on_the_device(gpu_ctx, name, connectivity)


@pytest.mark.parametrize("connectivity", cs.CONNECTIVITIES)
@pytest.mark.parametrize("chunk", range(8))
def test_device_equals_the_reference_and_the_host_on_seeded_cases(gpu_ctx, chunk, connectivity):
    for name in cs.SEEDED[chunk * 25: chunk * 25 + 25]:
        check_on_the_device(gpu_ctx, name, connectivity)


@pytest.mark.parametrize("connectivity", cs.CONNECTIVITIES)
@pytest.mark.parametrize("name", cs.LARGEST)
def test_the_largest_sides_on_the_device(gpu_ctx, name, connectivity):
    check_on_the_device(gpu_ctx, name, connectivity)


def test_capacity_protocol_on_the_device(gpu_ctx):
    for name, k in (("seed_7", 2), ("checkerboard_7x7", 1)):
        dev = check_capacity_protocol(ctx=gpu_ctx, name=name, connectivity=k)
        host = check_capacity_protocol(name=name, connectivity=k)
        assert all(dev[key].tobytes() == host[key].tobytes() for key in dev)            # the words behind the result are untouched on both paths


@pytest.mark.parametrize("what, kw", REFUSALS, ids=[f"{i}-{r[0][:28]}" for i, r in enumerate(REFUSALS)])
def test_bad_arguments_are_refused_before_any_device_work(gpu_ctx, what, kw):
    check_refusal(what, kw, ctx=gpu_ctx)


def test_public_functions_on_the_device(gpu_ctx):
    check_public_functions(PUBLIC, "cuda")
    for name in PUBLIC:                                              # 'auto' takes the device: the same bytes as the host
        for k in cs.CONNECTIVITIES:
            host = public_bytes(public_results(name, k, "cpu"))
            assert public_bytes(public_results(name, k, "auto")) == host and public_bytes(public_results(name, k, "cuda")) == host
