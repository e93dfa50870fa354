"""GPU: raw images of any size -> objects in original-image coordinates (ModelRunner.predict_images) against the reference's own
host chain: Pillow BICUBIC resize (+ convert('L') for grey nets) under _rescale_image_and_markup's size rule, one uint8 batch per
resized shape, ModelRunner.predict(..., rescale=True, meta_infos=MetaInfo scales) -- and prepare_batch_on_device against
prepare_image_and_target + convert('L') + build_segmentation_maps_on_device."""
import numpy as np
import pytest
import torch
from PIL import Image

from ubdvss_amd import NetConfig, Model, ModelRunner, Trainer, Adam, PreprocessingType, SegmapManager, synthetic
from ubdvss_amd.data_markup import ObjectMarkup, ClassifiedObjectMarkup

pytestmark = pytest.mark.gpu

RAW_SIZES = [(1080, 1920), (720, 1280), (480, 640), (555, 777), (256, 512), (1080, 1920), (333, 1001), (480, 640)]


class _Meta:                                                      # MetaInfo's scales (data_generators.py:42-55), read by rescale
    def __init__(self, xs, ys): self.xscale, self.yscale = xs, ys


def _trained_model(cfg, seed):
    c = 1 if cfg.is_grey() else 3
    n_cls = cfg.get_n_classes() if cfg.is_classification_supported() else 0
    model = Model(cfg, seed=seed)
    tr = Trainer(model, Adam(lr=3e-3))
    labels = synthetic.rectangle_maps(seed, 16, 64, 64, n_classes=n_cls)
    x = synthetic.textured_images(seed + 1, labels, 4, c).astype(np.float32) / 127.5 - 1.0
    xt, yt = torch.from_numpy(x).cuda(), torch.from_numpy(labels).cuda()
    for _ in range(150):
        tr.train_step_on_device(xt, yt)
    torch.cuda.synchronize()
    return model


def _raw_images(seed):
    """textured rectangles at the raw size (RGB), every other one as a PIL image"""
    out = []
    for k, (h, w) in enumerate(RAW_SIZES):
        hh, ww = -(-h // 4) * 4, -(-w // 4) * 4
        lab = synthetic.rectangle_maps(seed + k, 1, hh // 4, ww // 4)
        a = synthetic.textured_images(seed + 50 + k, lab, 4, 3)[0, :h, :w]
        a = (a.astype(np.int32) * np.array([1.0, 0.8, 0.6])).astype(np.uint8)
        out.append(Image.fromarray(a) if k % 2 else a)
    return out


def _host_chain(runner, model, cfg, images):
    """the reference's chain on the host: per image .convert('RGB') -> Pillow resize -> convert('L') (grey); per resized shape
    one batch through ModelRunner.predict with the MetaInfo scales; results back in input order"""
    prepared = []
    for im in images:
        pil = (im if isinstance(im, Image.Image) else Image.fromarray(im)).convert("RGB")
        w, h = pil.size
        r, _ = SegmapManager._rescale_image_and_markup(pil, None, cfg)
        if cfg.is_grey():
            r = r.convert("L")
        a = np.asarray(r)
        prepared.append((a[..., None] if a.ndim == 2 else a, _Meta(w / r.size[0], h / r.size[1])))
    found, logits = [None] * len(images), [None] * len(images)
    groups = {}
    for k, (a, _) in enumerate(prepared):
        groups.setdefault(a.shape, []).append(k)
    for idx in groups.values():
        batch = np.stack([prepared[k][0] for k in idx])
        _, _, objs = runner.predict(model, batch, rescale=True, meta_infos=[prepared[k][1] for k in idx])
        lg = model.predict_on_device(torch.from_numpy(batch).cuda()).cpu().numpy()
        for j, k in enumerate(idx):
            found[k], logits[k] = objs[j], lg[j]
    return found, logits, [p[0] for p in prepared]


def _key(objs):
    return [(tuple(int(v) for v in o.bbox), int(getattr(o, "object_type", -1))) for o in objs]


@pytest.mark.parametrize("grey,n_cls", [(True, 0), (False, 0), (True, 2)])
def test_predict_images_equals_the_host_chain(grey, n_cls):
    cfg = NetConfig(grey=grey, class_names=[f"c{i}" for i in range(n_cls)] if n_cls else None,
                    preprocessing=PreprocessingType.MOBILENET_LIKE)
    model = _trained_model(cfg, 60 + n_cls + int(grey))
    runner = ModelRunner(cfg, pixel_threshold=0.5, max_objects_per_image=512)
    images = _raw_images(80)
    want, want_logits, want_x = _host_chain(runner, model, cfg, images)
    # the device-resized batches: same bytes, so the same logits, bit for bit
    for shape in {x.shape for x in want_x}:
        idx = [k for k, x in enumerate(want_x) if x.shape == shape]
        x, metas = SegmapManager.rescale_images_on_device([images[k] for k in idx], cfg)
        assert np.array_equal(x.cpu().numpy(), np.stack([want_x[k] for k in idx]))
        lg = model.predict_on_device(x).cpu().numpy()
        for j, k in enumerate(idx):
            assert np.array_equal(lg[j], want_logits[k])
    got = runner.predict_images(model, images)
    assert len(got) == len(images)
    n_obj = 0
    for k in range(len(images)):
        assert _key(got[k]) == _key(want[k]), (k, _key(got[k]), _key(want[k]))
        n_obj += len(got[k])
    assert n_obj >= 4, n_obj                                        # the comparison covers real objects
    got2 = runner.predict_images(model, images, batch_size=1)
    assert [_key(o) for o in got2] == [_key(o) for o in want]
    print(f"grey={grey} n_cls={n_cls}: {n_obj} objects in original coordinates identical to the host chain")


def test_prepare_batch_equals_the_host_preparation():
    rng = np.random.default_rng(12)
    for cfg in (NetConfig(), NetConfig(grey=False)):
        images, markups = [], []
        for k, (h, w) in enumerate([(1080, 1920), (720, 1280), (300, 600), (1079, 1921)]):
            a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
            images.append(Image.fromarray(a) if k % 2 else a)
            objs = []
            for q in synthetic.random_quads(rng, h, w, 1, 5):
                q = np.asarray(q).reshape(-1)
                objs.append(ClassifiedObjectMarkup(q, int(rng.integers(0, 3))) if k % 2 else ObjectMarkup(q))
            markups.append(objs if k != 2 else [])
        x, labels, rescaled = SegmapManager.prepare_batch_on_device(images, markups, cfg)
        for k, im in enumerate(images):
            pil = (im if isinstance(im, Image.Image) else Image.fromarray(im)).convert("RGB")
            r, m, target = SegmapManager.prepare_image_and_target(pil, markups[k], cfg)
            if cfg.is_grey():
                r = r.convert("L")
            a = np.asarray(r)
            assert np.array_equal(x[k].cpu().numpy(), a[..., None] if a.ndim == 2 else a), k
            assert np.array_equal(labels[k].cpu().numpy(), np.asarray(target).astype(np.int32)), k
            assert len(m) == len(rescaled[k])
            for o1, o2 in zip(m, rescaled[k]):
                assert type(o1) is type(o2) and np.array_equal(o1.bbox, o2.bbox)
                assert getattr(o1, "object_type", None) == getattr(o2, "object_type", None)
        ref = SegmapManager.build_segmentation_maps_on_device((x.shape[2], x.shape[1]), rescaled, scale=cfg.get_scale())
        assert torch.equal(ref, labels)
