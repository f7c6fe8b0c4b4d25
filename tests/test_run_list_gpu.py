"""The shared case set of the run-list layer (tests/run_list_cases.py) on the device: all four mask analyses give the host path's bytes, and
the same bytes again on a second call.  What the bytes must be is held to the dense references by tests/test_run_list.py."""
import pytest

from ampis_amd._lib import AmpError
from run_list_cases import ENTRY_POINTS, FAULTS, SIZES, masks, run_all, same

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("h, w", SIZES)
def test_device_gives_the_host_bytes_twice(gpu_ctx, h, w):
    gt, pred = masks(h, w)
    host, dev = run_all(gt, pred), run_all(gt, pred, gpu_ctx)
    assert same(dev, host), [k for k in host if not same({k: dev[k]}, {k: host[k]})]
    assert same(run_all(gt, pred, gpu_ctx), dev)


@pytest.mark.parametrize("fault", sorted(FAULTS))
@pytest.mark.parametrize("entry", sorted(ENTRY_POINTS))
def test_refusals_come_before_any_device_work(gpu_ctx, entry, fault):
    bad, what = FAULTS[fault]
    with pytest.raises(AmpError, match=what.replace("(", r"\(")):
        ENTRY_POINTS[entry](bad, gpu_ctx)
