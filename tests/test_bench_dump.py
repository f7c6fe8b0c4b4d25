"""bench.py --dump-outputs, on the host: dump_outputs turns a Dets view (what amp_model_infer hands back) into fixed-shape float arrays --
boxes / scores / classes / mask areas per detection slot, zeros past each image's count, and a seeded sample of masks decoded to pixels.
The Dets here is built by hand from masks encoded with the library's own RLE codec (host C++, no GPU needed)."""
import ctypes as C
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return b


def test_dump_outputs_writes_fixed_shape_float_arrays(tmp_path):
    from ampis_amd import rle
    from ampis_amd._lib import Dets
    b = _bench()
    B, D, H, W = 2, 3, 12, 20
    r = np.random.default_rng(5)
    n = np.array([3, 1], np.int32)
    boxes = r.uniform(0, 10, (B, D, 4)).astype(np.float32)
    scores = r.uniform(0, 1, (B, D)).astype(np.float32)
    classes = r.integers(0, 2, (B, D)).astype(np.int32)
    dense = r.integers(0, 2, (B, D, H, W)).astype(np.uint8)
    strs = [rle.encode(dense[i, j])["counts"] for i in range(B) for j in range(D)]
    raw = C.create_string_buffer(b"".join(strs))
    slen = np.array([len(s) for s in strs], np.int32).reshape(B, D)
    soff = np.concatenate([[0], np.cumsum(slen.reshape(-1))[:-1]]).astype(np.uint64).reshape(B, D)
    oh, ow = np.full(B, H, np.int32), np.full(B, W, np.int32)
    P = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    d = Dets(B=B, D=D, n=P(n, C.c_int), boxes=P(boxes, C.c_float), scores=P(scores, C.c_float), classes=P(classes, C.c_int),
             out_h=P(oh, C.c_int), out_w=P(ow, C.c_int), rle_str=C.cast(raw, C.c_void_p),
             rle_str_off=P(soff, C.c_ulonglong), rle_str_len=P(slen, C.c_int))

    b.dump_outputs(str(tmp_path / "out"), d)
    got = {f[:-4]: np.load(tmp_path / "out" / f) for f in os.listdir(tmp_path / "out")}
    assert set(got) == {"num_detections", "boxes", "scores", "classes", "mask_areas", "mask_sample", "mask_sample_index"}
    assert all(v.dtype in (np.float32, np.float64) for v in got.values())
    assert np.array_equal(got["num_detections"], n)
    live = np.arange(D)[None, :] < n[:, None]
    assert np.array_equal(got["boxes"], np.where(live[..., None], boxes, 0)) and np.array_equal(got["scores"], np.where(live, scores, 0))
    assert np.array_equal(got["classes"], np.where(live, classes, 0))
    assert np.array_equal(got["mask_areas"], np.where(live, dense.sum(axis=(2, 3)), 0))
    assert got["mask_sample"].shape == (B, H, W)
    pick = np.random.default_rng(0).integers(0, D, size=B)
    for i in range(B):
        assert tuple(got["mask_sample_index"][i]) == (i, pick[i])
        want = dense[i, pick[i]] if pick[i] < n[i] else np.zeros((H, W))
        assert np.array_equal(got["mask_sample"][i], want)
