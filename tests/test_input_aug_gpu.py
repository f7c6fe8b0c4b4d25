"""INPUT.CROP, the vertical RANDOM_FLIP and range scale sampling on the device input path: amp_crop_resize_flip_u8 reads the crop window out
of the uploaded image, resizes it with Pillow's arithmetic and mirrors it where the last pass writes.  The frames must be byte for byte what the
host path stacks (and what numpy slicing + PIL give from the plan alone), the losses on augmented batches must be the oracle's, and a training
run must not notice which path built its frames."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LOSSES = ("loss_rpn_cls", "loss_rpn_loc", "loss_cls", "loss_box_reg", "loss_mask")


def _cfg(sizes, max_size, flip="horizontal", sampling="choice", crop=None):
    from ampis_amd import model_zoo
    from ampis_amd.config import get_cfg
    cfg = get_cfg()
    cfg.merge_from_file(model_zoo.get_config_file("COCO-InstanceSegmentation/mask_rcnn_R_50_FPN_3x.yaml"))
    cfg.INPUT.MIN_SIZE_TRAIN, cfg.INPUT.MAX_SIZE_TRAIN = tuple(sizes), max_size
    cfg.INPUT.RANDOM_FLIP, cfg.INPUT.MIN_SIZE_TRAIN_SAMPLING = flip, sampling
    if crop is not None:
        cfg.INPUT.CROP.ENABLED, cfg.INPUT.CROP.TYPE, cfg.INPUT.CROP.SIZE = True, crop[0], list(crop[1])
    return cfg


def _dd(i, h, w, n=40):
    from ampis_amd import synth
    img, gt = synth.micrograph(i, h, w, seed=5)
    annos = [{"bbox": [float(v) for v in b], "bbox_mode": 0, "segmentation": [[float(v) for v in p]], "category_id": 0}
             for b, p in list(zip(gt["boxes"], gt["polygons"]))[:n]]
    return {"file_name": f"s{i}.png", "image_bgr": img, "height": h, "width": w, "image_id": i, "annotations": annos}


def _frame_from_plans(dev):
    """The stacked frame from the deferred plans alone: numpy slicing, PIL, numpy flips, zero padding."""
    from PIL import Image
    outs = []
    for d in dev:
        plan, img = d["device_plan"], d["image_bgr"]
        nh, nw, bits = plan[:3]
        y0, x0, ch, cw = plan[3:7] if len(plan) > 3 else (0, 0) + img.shape[:2]
        o = np.ascontiguousarray(img[y0:y0 + ch, x0:x0 + cw])
        if (nh, nw) != (ch, cw):
            o = np.asarray(Image.fromarray(o).resize((nw, nh), Image.BILINEAR))
        if int(bits) & 1:
            o = o[:, ::-1]
        if int(bits) & 2:
            o = o[::-1]
        outs.append(o)
    H, W = max(o.shape[0] for o in outs), max(o.shape[1] for o in outs)
    frame = np.zeros((len(outs), H, W, 3), np.uint8)
    for i, o in enumerate(outs):
        frame[i, :o.shape[0], :o.shape[1]] = o
    return frame


def test_device_built_frames_equal_host_frames_under_crop_flips_and_range_sampling():
    from ampis_amd.data import DatasetMapper
    from ampis_amd.engine.defaults import TrainModel, _Uploader
    up = _Uploader(0, 2)
    try:
        cases = [   # shapes, MIN_SIZE_TRAIN, MAX_SIZE_TRAIN, flip axis, sampling, crop
            ([(300, 420)] * 3, (200, 232, 264), 333, "vertical", "choice", ("relative_range", (0.8, 0.7))),          # down-scaling, the max-size clamp
            ([(192, 256), (256, 192), (224, 224)], (256, 288), 512, "horizontal", "range", ("relative", (0.75, 0.5))),   # up-scaling, portrait + landscape
            ([(256, 320), (256, 320)], (0,), 1000, "vertical", "choice", ("absolute", (200, 260))),                  # no resize: (mirrored) copies out of a pitched window
            ([(300, 420), (420, 300)], (180, 260), 300, "horizontal", "range", ("absolute_range", (150, 250))),      # up and down in one batch
            ([(300, 420), (420, 300)], (200, 330), 420, "vertical", "range", ("absolute_range", (150, 250))),
            ([(256, 320), (256, 320)], (256,), 320, "vertical", "choice", None),                                      # no crop, no resize: straight and up-down copies
            ([(200, 280), (280, 200)], (150, 230), 300, "vertical", "range", None),                                   # the vertical flip alone, both passes
        ]
        seen = dict(up=0, down=0, same=0, v=0, h=0, one_pass=0)
        for shapes, sizes, max_size, flip, sampling, crop in cases:
            cfg = _cfg(sizes, max_size, flip, sampling, crop)
            dicts = [_dd(i, h, w) for i, (h, w) in enumerate(shapes)]
            m = DatasetMapper(cfg, True, seed=3)
            for rep in range(4):
                plans = [(d,) + tuple(m.draw()) for d in dicts]
                host = [m.apply(*p) for p in plans]
                dev = [m.apply(*p, True) for p in plans]
                imgs, sizes_h, gt_h = TrainModel.collate(host)
                none, sizes_d, gt_d = TrainModel.collate(dev)
                assert none is None and sizes_d == sizes_h
                for p, a, b in zip(plans, host, dev):
                    assert b["image_bgr"] is p[0]["image_bgr"] and b["device_plan"][:2] == a["image_bgr"].shape[:2] and len(b["device_plan"]) == 7
                    assert np.array_equal(a["gt"]["boxes"], b["gt"]["boxes"]) and np.array_equal(a["gt"]["poly_flat"], b["gt"]["poly_flat"])
                    nh, nw, bits, _, _, ch, cw = b["device_plan"]
                    seen["up"] += int(nh > ch); seen["down"] += int(nh < ch); seen["same"] += int((nh, nw) == (ch, cw))
                    seen["one_pass"] += int((nh == ch) != (nw == cw))
                    seen["h"] += bits & 1; seen["v"] += (bits >> 1) & 1
                own = _frame_from_plans(dev)
                assert own.shape == imgs.shape and np.array_equal(own, imgs), "the host mapping is not slicing + PIL + flips of its own plan"
                ptr, shp = up.frames(dev)
                assert shp == imgs.shape[:3]
                got = np.empty_like(imgs)
                up.ctx.d2h(got, ptr)
                assert np.array_equal(got, imgs), f"{int((got != imgs).sum())} bytes differ ({crop}, {flip}, plans {[d['device_plan'] for d in dev]})"
                assert np.array_equal(got, own)
        assert all(v > 0 for k, v in seen.items() if k != "one_pass"), seen
    finally:
        up.close()


def test_crop_entry_point_without_a_window_is_the_resize_entry_point_byte_for_byte():
    """amp_crop_resize_flip_u8(src_pitch = W, flip in {0, 1}) against amp_resize_flip_u8 on the same buffers: two-pass resizes, one-pass resizes,
    copies and mirrored copies, into a wider frame whose padding must stay untouched; then a window of a wider image against the window copied
    out on the host first, with all four flips."""
    from ampis_amd import _lib
    ctx = _lib.Context(0)
    L = _lib.lib()
    rng = np.random.default_rng(0)
    held = []

    def dev(nbytes):
        p = ctx.malloc(nbytes)
        held.append(p)
        return p

    def run(fn, src_img, src_off, args, h, w, pitch):
        src = dev(src_img.nbytes)
        ctx.h2d(src, np.ascontiguousarray(src_img))
        dst = dev(h * pitch * 3)
        _lib.check(L.amp_memset(ctx.handle, C.c_void_p(dst), 0x5A, h * pitch * 3), "amp_memset")
        H, W = args[-2:]
        nb = int(L.amp_resize_scratch_bytes(H, W, h, w))
        tmp = dev(nb) if (h, w) != (H, W) else 0
        _lib.check(fn(C.c_void_p(src + src_off), C.c_void_p(dst), C.c_void_p(tmp) if tmp else None), fn.__name__)
        ctx.sync()
        out = np.empty((h, pitch, 3), np.uint8)
        ctx.d2h(out, dst)
        return out

    try:
        shapes = [(240, 300, 160, 200), (97, 131, 200, 251), (64, 64, 64, 48), (50, 70, 20, 70), (33, 45, 33, 45), (120, 90, 151, 90)]
        for H, W, h, w in shapes:
            img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
            for pitch in (w, w + 5):
                for flip in (0, 1):
                    def old(s, d, t, flip=flip, pitch=pitch): return L.amp_resize_flip_u8(ctx.handle, s, H, W, d, pitch, h, w, flip, t)
                    def new(s, d, t, flip=flip, pitch=pitch): return L.amp_crop_resize_flip_u8(ctx.handle, s, W, H, W, d, pitch, h, w, flip, t)
                    a, b = run(old, img, 0, (H, W), h, w, pitch), run(new, img, 0, (H, W), h, w, pitch)
                    assert np.array_equal(a, b), (H, W, h, w, pitch, flip)
                    assert (a[:, w:] == 0x5A).all()
        # a window inside a wider image == the window copied out first
        big = rng.integers(0, 256, (150, 211, 3), dtype=np.uint8)
        for (y0, x0, ch, cw), (h, w) in (((10, 21, 120, 160), (90, 120)), ((0, 0, 150, 100), (150, 100)), ((30, 111, 100, 100), (100, 77)),
                                         ((149, 210, 1, 1), (1, 1)), ((5, 7, 60, 200), (77, 200))):
            win = np.ascontiguousarray(big[y0:y0 + ch, x0:x0 + cw])
            for flip in range(4):
                def packed(s, d, t, flip=flip): return L.amp_crop_resize_flip_u8(ctx.handle, s, cw, ch, cw, d, w + 3, h, w, flip & 1, t)
                def pitched(s, d, t, flip=flip): return L.amp_crop_resize_flip_u8(ctx.handle, s, big.shape[1], ch, cw, d, w + 3, h, w, flip, t)
                a = run(packed, win, 0, (ch, cw), h, w, w + 3)
                b = run(pitched, big, (y0 * big.shape[1] + x0) * 3, (ch, cw), h, w, w + 3)
                want = a[:, :w][::-1] if flip & 2 else a[:, :w]
                assert np.array_equal(b[:, :w], want) and (b[:, w:] == 0x5A).all(), ((y0, x0, ch, cw), (h, w), flip)
        img = rng.integers(0, 256, (8, 8, 3), dtype=np.uint8)
        src, dst = dev(img.nbytes), dev(img.nbytes)
        for bad in (dict(pitch=7), dict(flip=4), dict(flip=-1)):           # a pitch shorter than the window, a flip outside the two bits: refused, nothing launched
            st = L.amp_crop_resize_flip_u8(ctx.handle, C.c_void_p(src), bad.get("pitch", 8), 8, 8, C.c_void_p(dst), 8, 8, 8, bad.get("flip", 0), None)
            assert st != 0
    finally:
        ctx.sync()
        for p in held:
            ctx.free(p)
        ctx.close()


@pytest.mark.parametrize("mask_format", ["polygon", "bitmask"])
def test_losses_on_mapper_augmented_batches_match_the_oracle(gpu_ctx, mask_format):
    """The 256 x 320 batch of tests/test_train_fwd_gpu.py through the mapper with INPUT.CROP relative_range + vertical flip: the device-built
    frame and the transformed ground truth go to the model and to oracle.train.forward_losses alike; the five losses agree within the bound
    test_losses_match_oracle holds (rel 2e-4, abs 1e-6)."""
    from ampis_amd import params as P, rle, synth
    from ampis_amd.data import DatasetMapper
    from ampis_amd.engine.defaults import TrainModel, _Uploader
    from ampis_amd.model import MaskRCNN
    from oracle import maskrcnn as M, train as T
    K, B, H, W = 2, 2, 256, 320
    imgs, gts = synth.batch(B, H, W, seed=5)
    dicts = []
    for i, (img, g) in enumerate(zip(imgs, gts)):
        annos = []
        for b, c, p in list(zip(g["boxes"], g["classes"], g["polygons"]))[:60]:
            seg = [[float(v) for v in p]]
            if mask_format == "bitmask":
                seg = rle.merge(rle.frPyObjects(seg, H, W))
            annos.append({"bbox": [float(v) for v in b], "bbox_mode": 0, "segmentation": seg, "category_id": int(c)})
        dicts.append({"file_name": f"b{i}.png", "image_bgr": np.ascontiguousarray(img), "height": H, "width": W, "image_id": i, "annotations": annos})
    cfg = _cfg((256,), 320, "vertical", "choice", ("relative_range", (0.9, 0.9)))
    cfg.INPUT.MASK_FORMAT = mask_format
    m = DatasetMapper(cfg, True, seed=2)
    plans = [(d,) + tuple(m.draw()) for d in dicts]
    for _ in range(8):                       # the first drawn batch that flips one image and leaves the other
        if sorted(p[2][1] for p in plans) == [False, True]:
            break
        plans = [(d,) + tuple(m.draw()) for d in dicts]
    assert sorted(p[2][1] for p in plans) == [False, True]
    dev = [m.apply(*p, True) for p in plans]
    assert all(len(d["device_plan"]) == 7 and d["device_plan"][5:] != (H, W) for d in dev)
    _, sizes, packed = TrainModel.collate(dev)
    up = _Uploader(0, 1)
    try:
        ptr, shp = up.frames(dev)
        frame = np.empty(shp + (3,), np.uint8)
        up.ctx.d2h(frame, ptr)
    finally:
        up.close()
    assert frame.shape[1] <= H and frame.shape[2] <= W and frame.any()
    gt = [{k: d["gt"][k] for k in ("boxes", "classes", "polygons", "masks_rle") if k in d["gt"]} for d in dev]
    assert all(20 < len(g["boxes"]) <= 60 for g in gt)
    npp = P.init_params(K, seed=1, style="spread")
    ref = T.forward_losses(frame, gt, M.to_torch_params(npp), T.TrainCfg(num_classes=K, seed=7), image_sizes=sizes)
    model = MaskRCNN(gpu_ctx, K, max_batch=B, max_h=H, max_w=W, max_out_hw=max(H, W), train=True, max_gt=4096, max_poly_doubles=4096 * 64)
    try:
        model.load_params(npp)
        model.set_image_sizes(sizes)
        got = model.forward_losses(frame, packed, seed=7)
        model.set_image_sizes(None)
    finally:
        model.close()
    for k in LOSSES:
        print(mask_format, k, got[k], float(ref[k]))
    for k in LOSSES:
        assert got[k] == pytest.approx(float(ref[k]), rel=2e-4, abs=1e-6), (k, got[k], float(ref[k]))


def test_trainer_with_crop_vertical_flip_and_range_sampling(tmp_path, monkeypatch):
    """DefaultTrainer, INPUT.CROP + vertical flip + range scale sampling, NUM_WORKERS = 2, six iterations: finite losses, bit for bit the same
    whether the frames are built on the device or on the host (AMP_HOST_TRAIN_INPUT=1), the net sized once from cfg -- and a run without
    the augmentations trains on something else."""
    from ampis_amd import checkpoint, params as P
    from ampis_amd.data import DatasetCatalog, MetadataCatalog
    from ampis_amd.engine import DefaultTrainer
    dicts = [_dd(i, 288, 352) for i in range(6)]
    checkpoint.save_checkpoint(str(tmp_path / "init.pth"), P.init_params(1, seed=4, style="spread"))
    runs = {}
    for mode in ("device", "host", "plain"):
        if mode == "host":
            monkeypatch.setenv("AMP_HOST_TRAIN_INPUT", "1")
        else:
            monkeypatch.delenv("AMP_HOST_TRAIN_INPUT", raising=False)
        DatasetCatalog.clear()
        DatasetCatalog.register("particle_Train", lambda: dicts)
        MetadataCatalog.get("particle_Train").set(thing_classes=["particle"])
        if mode == "plain":
            cfg = _cfg((224, 288), 352, "none", "range")
        else:
            cfg = _cfg((224, 288), 352, "vertical", "range", ("relative_range", (0.8, 0.8)))
        cfg.DATASETS.TRAIN, cfg.DATASETS.TEST = ("particle_Train",), ("particle_Train",)
        cfg.SOLVER.IMS_PER_BATCH, cfg.SOLVER.MAX_ITER, cfg.SOLVER.CHECKPOINT_PERIOD, cfg.SOLVER.BASE_LR = 3, 6, 10 ** 6, 1e-3
        cfg.MODEL.WEIGHTS, cfg.MODEL.ROI_HEADS.NUM_CLASSES = str(tmp_path / "init.pth"), 1
        cfg.DATALOADER.NUM_WORKERS = 2
        cfg.OUTPUT_DIR = str(tmp_path / mode)
        tr = DefaultTrainer(cfg)
        tr.resume_or_load(resume=False)
        seen, nets = [], []

        class Rec:
            trainer = None
            def before_train(self): pass
            def after_train(self): pass
            def before_step(self): pass
            def after_step(self):
                seen.append(dict(tr.storage.latest()))
                nets.append((id(tr._net), tr._cap))
        tr.register_hooks([Rec()])
        assert (tr._uploader is not None) and tr._uploader.device_resize == (mode != "host")
        cap0 = tr._cap
        tr.train()
        assert len(set(nets)) == 1 and nets[0][1] == cap0, "the net was re-created mid-run: _capacity_from_cfg did not bound a frame"
        runs[mode] = seen
        tr.close()
        del tr
    DatasetCatalog.clear()
    assert len(runs["device"]) == 6 and runs["device"] == runs["host"], (runs["device"][-1], runs["host"][-1])
    for s in runs["device"]:
        assert all(np.isfinite(float(v[0] if isinstance(v, tuple) else v)) for k, v in s.items() if "loss" in k) and any("loss" in k for k in s)
    assert runs["plain"] != runs["device"]
