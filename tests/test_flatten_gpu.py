"""amp_flatten_instances on the device (csrc/flatten.hip): every case of tests/flatten_cases.py against the dense-loop reference and against the
host path, byte for byte; the device's bytes against its own second call; the capacity protocol and the refusals with a context (made before
any device work); the largest sides; the spheroidite round trip; the Python callers on the device."""
import numpy as np
import pytest

from ampis_amd import analyze

import flatten_cases as cs
from test_flatten import PUBLIC, REFUSALS, check_annotation_round_trip, check_capacity_protocol, check_public_functions, check_refusal

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", cs.HAND)
def test_device_equals_the_reference_and_the_host(gpu_ctx, name):
    dev = cs.check_case(name, ctx=gpu_ctx)
    assert cs.result_bytes(dev) == cs.result_bytes(cs.run(name))
    assert cs.result_bytes(dev) == cs.result_bytes(cs.run(name, ctx=gpu_ctx))                         # its own second call


@pytest.mark.parametrize("chunk", range(8))
def test_device_equals_the_reference_and_the_host_on_seeded_cases(gpu_ctx, chunk):
    for i in range(chunk * 25, chunk * 25 + 25):
        dev = cs.check_case(f"seed_{i}", ctx=gpu_ctx)
        assert cs.result_bytes(dev) == cs.result_bytes(cs.run(f"seed_{i}")), i
        assert cs.result_bytes(dev) == cs.result_bytes(cs.run(f"seed_{i}", ctx=gpu_ctx)), i


@pytest.mark.parametrize("name", cs.LARGEST)
def test_the_largest_sides_on_the_device(gpu_ctx, name):
    dev = cs.check_case(name, ctx=gpu_ctx)
    assert cs.result_bytes(dev) == cs.result_bytes(cs.run(name))


def test_capacity_protocol_on_the_device(gpu_ctx):
    for name in ("seed_7", "checkerboard_66x3"):
        dev = check_capacity_protocol(ctx=gpu_ctx, name=name)
        host = check_capacity_protocol(name=name)
        assert all(dev[k] is host[k] is None or dev[k].tobytes() == host[k].tobytes() for k in dev)   # the words behind the result are untouched on both paths


@pytest.mark.parametrize("what, kw", REFUSALS, ids=[f"{i}-{r[0][:28]}" for i, r in enumerate(REFUSALS)])
def test_bad_arguments_are_refused_before_any_device_work(gpu_ctx, what, kw):
    check_refusal(what, kw, ctx=gpu_ctx)


def test_spheroidite_annotation_round_trip_on_the_device(gpu_ctx):
    check_annotation_round_trip("cuda")


def test_public_functions_on_the_device(gpu_ctx):
    check_public_functions(PUBLIC, "cuda")
    for name in PUBLIC:                                              # 'auto' takes the device: the same bytes as the host
        masks, size = cs.get(name)["masks"], cs.size(name)
        auto, stats = analyze.resolve_overlaps(masks, "area", size=size, return_stats=True)
        host, hstats = analyze.resolve_overlaps(masks, "area", size=size, device="cpu", return_stats=True)
        assert auto == host and all(stats[k].tobytes() == hstats[k].tobytes() for k in hstats)
        assert analyze.instances_to_label_image(masks, "area", size=size).tobytes() == analyze.instances_to_label_image(masks, "area", size=size, device="cpu").tobytes()
