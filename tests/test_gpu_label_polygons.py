"""GPU: ubd_build_label_maps_polygons (label maps from polygon markup of 3..64 vertices) against Pillow's ImageDraw.polygon itself,
0 differing pixels, and against ubd_build_label_maps on the quads of a mixed batch, bit for bit."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))          # the helper modules beside this file
import segmap_cases as sc  # noqa: E402
from ubdvss_amd import _lib, markup_readers, ObjectMarkup, ClassifiedObjectMarkup  # noqa: E402
from ubdvss_amd.segmap_manager import SegmapManager  # noqa: E402

pytestmark = pytest.mark.gpu


def _pillow(size, markup, scale):
    return np.asarray(SegmapManager.build_segmentation_map(Image.new('L', size), markup, scale=scale)).astype(np.int32)


def _raw_polygons(markups, size, scale, max_verts):
    """ubd_build_label_maps_polygons itself, whatever the vertex counts of the batch"""
    lib = _lib.load()
    n, cap = len(markups), max(1, max(len(m) for m in markups))
    verts = np.zeros((n, cap, max_verts, 2), np.float64)
    nverts = np.zeros((n, cap), np.int32)
    values = np.zeros((n, cap), np.int32)
    counts = np.array([len(m) for m in markups], np.int32)
    for i, m in enumerate(markups):
        for j, obj in enumerate(m):
            b = np.asarray(obj.bbox, np.float64).reshape(-1, 2)
            verts[i, j, :len(b)] = b
            nverts[i, j] = len(b)
            values[i, j] = obj.object_type + 1 if isinstance(obj, ClassifiedObjectMarkup) else 1
    dev = [torch.from_numpy(a).cuda() for a in (verts, nverts, values, counts)]
    labels = torch.full((n, size[1] // scale, size[0] // scale), -1, dtype=torch.int32, device="cuda")
    rc = lib.ubd_build_label_maps_polygons(*(d.data_ptr() for d in dev), n, cap, max_verts, size[1] // scale, size[0] // scale, scale,
                                           labels.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.ubd_last_error()
    return labels.cpu().numpy()


def test_hulls_of_segmentation_maps_after_the_rescale_equal_pillow():
    """part-1 hulls of four 136 x 200 maps, rescaled to the 128 x 192 network size as _rescale_image_and_markup does (fractional
    float64 markup), drawn at scale 4 on (4, 32, 48) maps"""
    h, w, new_h, new_w = 136, 200, 128, 192
    rng = np.random.default_rng(21)
    maps = np.zeros((4, h, w), np.uint8)
    for i in range(4):
        for _ in range(4):
            cx, cy = rng.uniform(20, w - 20), rng.uniform(20, h - 20)
            mask = (sc.rotated_rect_mask(h, w, cx, cy, rng.uniform(8, 40), rng.uniform(4, 14), rng.uniform(0, np.pi)) if rng.integers(2)
                    else sc.ellipse_mask(h, w, cx, cy, rng.uniform(6, 30), rng.uniform(5, 16), rng.uniform(0, np.pi)))
            maps[i][mask] = 255
    markups = [SegmapManager._rescale_markup(m, w, h, new_w, new_h) for m in markup_readers.segmap_polygons(maps)]
    sizes = [np.asarray(o.bbox).size // 2 for m in markups for o in m]
    assert len(sizes) >= 8 and max(sizes) > 8 and any(s != 4 for s in sizes)
    got = SegmapManager.build_segmentation_maps_on_device((new_w, new_h), markups, scale=4).cpu().numpy()
    assert got.shape == (4, 32, 48)
    for i, m in enumerate(markups):
        want = _pillow((new_w, new_h), m, 4)
        assert np.array_equal(got[i], want), (i, int((got[i] != want).sum()))
        assert set(np.unique(want)) == {0, 6}


def _mixed_batch(triangle=True):
    """with ``triangle`` for the C call; SegmapManager's device form refuses three points (tests/test_gpu_raster.py), so its batch
    has a pentagon there"""
    tri = ClassifiedObjectMarkup([20.0, 90.5, 150.25, 20.0, 170.0, 110.0] + ([] if triangle else [100.0, 125.0, 40.0, 118.0]), 1)
    octagon = ClassifiedObjectMarkup([60, 10, 100, 10, 130, 40, 130, 80, 100, 110, 60, 110, 30, 80, 30, 40], 2)
    quad_a = ClassifiedObjectMarkup([40.3, 30.1, 160.7, 50.2, 150.0, 100.9, 30.2, 80.6], 0)
    quad_b = ObjectMarkup([100, 5, 185, 30, 170, 70, 90, 40])
    ring = [100 + 60 * np.cos(a) for a in np.linspace(0, 2 * np.pi, 40, endpoint=False)]
    ring_y = [64 + 50 * np.sin(a) for a in np.linspace(0, 2 * np.pi, 40, endpoint=False)]
    gon40 = ClassifiedObjectMarkup(np.stack([ring, ring_y], axis=1).reshape(-1), 3)
    fold = ObjectMarkup([40, 40, 80, 60, 40, 40, 60, 100])            # opposite corners coincide: the documented exception
    return [[gon40, quad_a, tri, quad_b, octagon],                    # mixed, overlapping, later over earlier
            [quad_a, quad_b],                                         # quads only
            [quad_b, fold, quad_a],                                   # quads only, with a fold
            [octagon, tri]]                                           # polygons only


def test_mixed_quads_and_polygons_in_painters_order():
    size, scale = (192, 128), 4
    batch = _mixed_batch(triangle=False)
    got = SegmapManager.build_segmentation_maps_on_device(size, batch, scale=scale).cpu().numpy()
    raw = _raw_polygons(batch, size, scale, 40)
    assert np.array_equal(got, raw)
    with_tri = _mixed_batch()
    raw_tri = _raw_polygons(with_tri, size, scale, 40)
    for i in (0, 3):
        want = _pillow(size, with_tri[i], scale)
        assert np.array_equal(raw_tri[i], want), (i, int((raw_tri[i] != want).sum()))
    for i in (0, 1, 3):
        want = _pillow(size, batch[i], scale)
        assert np.array_equal(got[i], want), (i, int((got[i] != want).sum()))
    assert len(np.unique(raw_tri[0])) == 5 and len(np.unique(got[0])) >= 4     # every object of the mixed image shows
    # the quad-only images: exactly the pixels of ubd_build_label_maps, the fold included
    quads_only = SegmapManager.build_segmentation_maps_on_device(size, [batch[1], batch[2]], scale=scale).cpu().numpy()
    assert np.array_equal(got[1], quads_only[0]) and np.array_equal(got[2], quads_only[1])
    # and a whole map width that is no multiple of the block: 47 columns
    odd = _raw_polygons(with_tri, (188, 116), scale, 64)
    for i in (0, 1, 3):
        assert np.array_equal(odd[i], _pillow((188, 116), with_tri[i], scale)), i


def test_an_image_without_objects_is_all_background():
    size, scale = (192, 128), 4
    batch = [[], _mixed_batch()[3], []]
    got = _raw_polygons(batch, size, scale, 8)
    assert not got[0].any() and not got[2].any() and got[1].any()
    assert np.array_equal(got[1], _pillow(size, batch[1], scale))


def test_unsupported_vertex_counts():
    two = ObjectMarkup([1, 1, 30, 30])
    with pytest.raises(ValueError, match="image 0, object 0"):
        SegmapManager.build_segmentation_maps_on_device((64, 64), [[two]], scale=4)
    big = ObjectMarkup(np.arange(130, dtype=np.float64))
    with pytest.raises(ValueError, match="image 0, object 0"):
        SegmapManager.build_segmentation_maps_on_device((64, 64), [[big]], scale=4)
    tri = ObjectMarkup([1, 1, 30, 30, 5, 40])
    with pytest.raises(ValueError, match="image 0, object 0"):          # three points: refused as before (tests/test_gpu_raster.py)
        SegmapManager.build_segmentation_maps_on_device((64, 64), [[tri]], scale=4)
    pent = ObjectMarkup([1, 1, 30, 5, 40, 30, 20, 50, 2, 30])
    with pytest.raises(ValueError, match="augmentation of polygon markup"):
        SegmapManager.prepare_batches_on_device([np.zeros((64, 64, 3), np.uint8)], [[pent]], None, augment=True)
    lib = _lib.load()
    assert lib.ubd_build_label_maps_polygons(None, None, None, None, 1, 1, 8, 8, 8, 4, None, None) != 0
    x = torch.zeros(64, dtype=torch.float64, device="cuda")
    assert lib.ubd_build_label_maps_polygons(x.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), 1, 1, 65, 8, 8, 4, x.data_ptr(), None) != 0
    assert b"max_verts" in lib.ubd_last_error()
