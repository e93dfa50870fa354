"""CPU: the size rule of the device resize (SegmapManager.target_size, factored out of _rescale_image_and_markup,
segmap_manager.py:135-173) and the refusal of the new entry points without a GPU (no CPU fallback)."""
import ctypes
import itertools

import numpy as np
import pytest
from PIL import Image

from ubdvss_amd import NetConfig, SegmapManager, ModelRunner, ObjectMarkup


def test_target_size_is_the_size_rescale_produces():
    sides = [1, 2, 31, 32, 33, 63, 64, 95, 96, 97, 160, 255, 256, 257, 480, 511, 512, 513, 640, 720, 767, 1000, 1080, 1280, 1920]
    n = 0
    for multiple, max_side in ((64, 512), (32, 512), (4, 640), (64, 1024), (16, 300)):
        cfg = NetConfig.from_others(NetConfig(), side_multiple=multiple, max_image_side=max_side)
        for w, h in itertools.product(sides, sides):
            img = Image.new("L", (w, h))
            for ms in (None, 384):
                resized, markup = SegmapManager._rescale_image_and_markup(img, [ObjectMarkup([0, 0, w, 0, w, h, 0, h])], cfg, max_side=ms)
                assert SegmapManager.target_size(w, h, cfg, max_side=ms) == resized.size, (w, h, multiple, max_side, ms)
                nw, nh = resized.size
                assert np.array_equal(markup[0].bbox, np.array([0, 0, w, 0, w, h, 0, h], np.float64) * np.tile([nw / w, nh / h], 4))
                n += 1
    assert n > 6000


def test_no_cpu_fallback_for_the_resize():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from ubdvss_amd import _lib
    lib = _lib.load()
    offs, hw = np.zeros(1, np.int64), np.full(2, 8, np.int32)
    assert lib.ubd_resize_images(ctypes.c_void_p(16), offs.ctypes.data, hw.ctypes.data, 3, 1, ctypes.c_void_p(16), 4, 4, 1, None) != 0
    img = np.zeros((40, 60, 3), np.uint8)
    with pytest.raises(RuntimeError):
        SegmapManager.rescale_images_on_device([img], NetConfig())
    with pytest.raises(RuntimeError):
        SegmapManager.prepare_batch_on_device([img], [[]], NetConfig())
    with pytest.raises(RuntimeError):
        ModelRunner(NetConfig()).predict_images(None, [img])
