"""amp_mask_morphology on the device (csrc/morphology.hip): every case of tests/morphology_cases.py -- three shapes, the case's radii, both
border values, all six ops -- against scipy on the decoded masks and against the host path, byte for byte; the device's bytes against its
own second call; the capacity protocol and the refusals with a context (made before any device work); the largest sides; the Python callers
on the device."""
import pytest

import morphology_cases as cs
from test_morphology import (N_CHUNKS, PER_CHUNK, PUBLIC, REFUSALS, check_boundary_iou, check_capacity_protocol, check_largest, check_near_pairs,
                             check_public_functions, check_refusal, public_bytes, public_results)

pytestmark = pytest.mark.gpu


def check_on_the_device(gpu_ctx, name, shape, r, b):
    dev = cs.check_case(name, shape, r, b, ctx=gpu_ctx)
    for op in cs.OPS:
        where = (name, op, shape, r, b)
        assert cs.result_bytes(dev[op]) == cs.result_bytes(cs.run(name, op, shape, r, b)), where
        assert cs.result_bytes(dev[op]) == cs.result_bytes(cs.run(name, op, shape, r, b, ctx=gpu_ctx)), where         # its own second call


@pytest.mark.parametrize("name", cs.HAND)
def test_device_equals_the_reference_and_the_host(gpu_ctx, name):
    for shape, r, b in cs.combos(name):
        check_on_the_device(gpu_ctx, name, shape, r, b)


@pytest.mark.parametrize("shape", cs.SHAPES)
@pytest.mark.parametrize("chunk", range(N_CHUNKS))
def test_device_equals_the_reference_and_the_host_on_seeded_cases(gpu_ctx, chunk, shape):
    for name in cs.SEEDED[chunk * PER_CHUNK: (chunk + 1) * PER_CHUNK]:
        for r in cs.RADII:
            for b in cs.BORDERS:
                check_on_the_device(gpu_ctx, name, shape, r, b)


@pytest.mark.parametrize("name", list(cs.LARGEST))
def test_the_largest_sides_on_the_device(gpu_ctx, name):
    assert check_largest(name, ctx=gpu_ctx) == check_largest(name) == check_largest(name, ctx=gpu_ctx)


def test_capacity_protocol_on_the_device(gpu_ctx):
    for kw in (dict(), dict(name="checkerboard_7x7", op="band_out", shape="diamond", radius=1)):
        dev = check_capacity_protocol(ctx=gpu_ctx, **kw)
        host = check_capacity_protocol(**kw)
        assert all(dev[key].tobytes() == host[key].tobytes() for key in dev)            # the words behind the result are untouched on both paths


@pytest.mark.parametrize("what, kw", REFUSALS, ids=[f"{i}-{r[0][:28]}" for i, r in enumerate(REFUSALS)])
def test_bad_arguments_are_refused_before_any_device_work(gpu_ctx, what, kw):
    check_refusal(what, kw, ctx=gpu_ctx)


def test_public_functions_on_the_device(gpu_ctx):
    check_public_functions(PUBLIC, "cuda")
    for name in PUBLIC:                                              # 'auto' takes the device: the same bytes as the host
        host = public_bytes(public_results(name, "cpu"))
        assert public_bytes(public_results(name, "auto")) == host and public_bytes(public_results(name, "cuda")) == host


def test_boundary_iou_and_near_pairs_on_the_device(gpu_ctx):
    check_boundary_iou("cuda")
    check_near_pairs("cuda")
