"""amp_mask_parts on the device (csrc/mask_parts.hip): every case of tests/mask_parts_cases.py against the scipy reference and against the host path,
byte for byte; the device's bytes against its own second call; the capacity protocol and the refusals with a context (made before any device
work); one spheroidite annotation as one mask; the Python callers on the device."""
import numpy as np
import pytest

from ampis_amd import analyze

import mask_parts_cases as cs
from test_mask_parts import (REFUSALS, check_annotation_as_one_mask, check_capacity_protocol, check_largest_image, check_refusal,
                             check_topology_and_cleaning)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", cs.HAND)
def test_device_equals_the_reference_and_the_host(gpu_ctx, name):
    dev = cs.check_case(name, ctx=gpu_ctx)
    assert cs.result_bytes(dev) == cs.result_bytes(cs.check_case(name))
    assert cs.result_bytes(dev) == cs.result_bytes(cs.run(name, ctx=gpu_ctx))                         # its own second call


@pytest.mark.parametrize("chunk", range(8))
def test_device_equals_the_reference_and_the_host_on_seeded_cases(gpu_ctx, chunk):
    for i in range(chunk * 25, chunk * 25 + 25):
        dev = cs.check_case(f"seed_{i}", ctx=gpu_ctx)
        assert cs.result_bytes(dev) == cs.result_bytes(cs.run(f"seed_{i}")), i
        assert cs.result_bytes(dev) == cs.result_bytes(cs.run(f"seed_{i}", ctx=gpu_ctx)), i


def test_capacity_protocol_on_the_device(gpu_ctx):
    dev = check_capacity_protocol(ctx=gpu_ctx)
    host = check_capacity_protocol()
    assert all(dev[k].tobytes() == host[k].tobytes() for k in dev)   # the words behind the result are untouched on both paths


@pytest.mark.parametrize("what, kw", REFUSALS, ids=[f"{i}-{r[0][:28]}" for i, r in enumerate(REFUSALS)])
def test_bad_arguments_are_refused_before_any_device_work(gpu_ctx, what, kw):
    check_refusal(what, kw, ctx=gpu_ctx)


def test_the_largest_image_on_the_device(gpu_ctx):
    check_largest_image(ctx=gpu_ctx)


def test_spheroidite_annotation_as_one_mask_on_the_device(gpu_ctx):
    check_annotation_as_one_mask("cuda")


def test_public_functions_on_the_device(gpu_ctx):
    names = ["ring_in_ring_clean", "twelve_masks_4", "board_130x40_4", "empty", "seed_1", "seed_2"]
    check_topology_and_cleaning(names, "cuda")
    for name in names:                                               # 'auto' takes the device: the same bytes as the host
        c = cs.get(name)
        auto = analyze.clean_masks(c["masks"], c["min_size"], c["area_threshold"], c["keep_largest"], c["connectivity"])
        assert auto == analyze.clean_masks(c["masks"], c["min_size"], c["area_threshold"], c["keep_largest"], c["connectivity"], device="cpu")
        topo, host = analyze.mask_topology(c["masks"], c["connectivity"]), analyze.mask_topology(c["masks"], c["connectivity"], device="cpu")
        assert all(topo[k].tobytes() == host[k].tobytes() for k in host)
        table = analyze.region_properties(c["masks"], ["euler_number", "filled_area"])
        assert table["euler_number"].dtype == np.int64 and len(table["filled_area"]) == len(c["masks"])
