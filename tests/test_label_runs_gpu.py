"""amp_label_runs on the device (csrc/label_runs.hip): every case of tests/label_runs_cases.py against the scipy / host-codec reference and
against the host path, byte for byte; the device's bytes against its own second call; one spheroidite annotation at both connectivities; the
capacity protocol and the refusals with a context (made before any device work); the Python callers on the device."""
import numpy as np
import pytest

from ampis_amd import analyze, data_utils

import label_runs_cases as cs
from test_label_runs import (ANNOTATIONS, REFUSALS, annotation, check_annotation, check_capacity_protocol, check_refusal, make_dataset,
                             previous_ddict_instances, same_ddicts)

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


def test_spheroidite_annotation_at_both_connectivities(gpu_ctx):
    name, n8, n4 = ANNOTATIONS[0]
    dev = check_annotation(name, n8, n4, ctx=gpu_ctx)
    fg = annotation(name)
    for conn, d in zip((2, 1), dev):
        for device in ("cpu", "cuda"):                               # the host path, and the device's second call
            again = analyze.label_image_to_rle(fg, "binary", conn, device=device, return_labels=True)
            assert again[0] == d[0] and all(a.tobytes() == b.tobytes() for a, b in zip(again[1:], d[1:]))


def test_capacity_protocol_on_the_device(gpu_ctx):
    dev = check_capacity_protocol(ctx=gpu_ctx)
    host = check_capacity_protocol()
    assert all(dev[k].tobytes() == host[k].tobytes() for k in dev)   # the words behind the result are untouched on both paths


@pytest.mark.parametrize("what, kw", REFUSALS, ids=[f"{i}-{r[0][:28]}" for i, r in enumerate(REFUSALS)])
def test_bad_arguments_are_refused_before_any_device_work(gpu_ctx, what, kw):
    check_refusal(what, kw, ctx=gpu_ctx)


@pytest.mark.parametrize("fmt", ["binary", "label"])
def test_get_ddicts_on_the_device(gpu_ctx, tmp_path, fmt):
    im_root, ann_root, anns = make_dataset(tmp_path, fmt)
    for device in ("cuda", "auto"):
        dd = data_utils.get_ddicts(fmt, im_root, ann_root, device=device)
        assert len(dd) == 3
        for d in dd:
            stem = d["file_name"].replace("\\", "/").split("/")[-1][:-4]
            same_ddicts(d, previous_ddict_instances(anns[stem], fmt), anns[stem].shape[:2])


def test_label_components_and_regionprops_table_on_the_device(gpu_ctx):
    fg = annotation(ANNOTATIONS[2][0])
    for conn in (1, 2):
        host = analyze.label_components(fg, conn, device="cpu")
        assert host.tobytes() == analyze.label_components(fg, conn, device="cuda").tobytes()
    lab = analyze.label_components(fg, 2, device="cuda")[:200, :240]
    got = analyze.regionprops_table(lab)                             # device='auto': the device
    labels = [int(v) for v in np.unique(lab) if v != 0]
    from ampis_amd import rle
    want = analyze.region_properties([rle.encode(np.asfortranarray(lab == v)) for v in labels], analyze.RPROPS_DEFAULT_KEYS, device="cpu")
    assert all(got[k].tobytes() == want[k].tobytes() for k in want)
