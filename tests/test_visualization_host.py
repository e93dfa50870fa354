"""CPU: the arithmetic the device visualisations rest on, the argument checks of ubd_visualize_images (they run before any HIP
call), ImageResultCategories and ResultSaver.  All comparisons are of uint8 integers and exact."""
import os
import sys

import numpy as np
import pytest
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))          # the helper modules beside this file
import visualization_oracle as vo  # noqa: E402
from ubdvss_amd import _lib, ImageResultCategories, ObjectMarkup, ClassifiedObjectMarkup, ResultSaver  # noqa: E402
from ubdvss_amd.evaluation import FtMetrics  # noqa: E402


def _image_with_every_value(rng, h, w, c, mask_up):
    """random image in which every value 0..255 occurs in a masked and in an unmasked pixel, in every channel"""
    img = rng.integers(0, 256, (h, w, c), dtype=np.uint8)
    for sel in (mask_up, ~mask_up):
        ys, xs = np.nonzero(sel)
        assert len(ys) >= 256
        pick = rng.permutation(len(ys))[:256]
        for ch in range(c):
            img[ys[pick], xs[pick], ch] = np.roll(np.arange(256, dtype=np.uint8), 37 * ch)
    return img


@pytest.mark.parametrize("channels", [3, 1])
@pytest.mark.parametrize("s", [1, 2, 3, 4])
def test_closed_form_equals_pillow(channels, s):
    rng = np.random.default_rng(10 * s + channels)
    mh, mw = 40, 52
    target = (rng.random((mh, mw)) > 0.5).astype(np.float32)
    up = vo.closed_upscale(target > 0.5, mh * s, mw * s)
    img = _image_with_every_value(rng, mh * s, mw * s, channels, up)
    for ch in range(channels):
        for sel in (up, ~up):
            assert len(np.unique(img[..., ch][sel])) == 256
    assert np.array_equal(vo.closed_segmentation(img, target), vo.pillow_segmentation(img, target))
    # both colours: the classification overlay, two Pillow passes against the single pass
    cls = rng.integers(-1, 2, (mh, mw)).astype(np.int8)
    assert np.array_equal(vo.closed_classification(img, cls), vo.pillow_classification(img, cls))


def test_to_uint8_is_the_float32_denorm():
    u = np.arange(256, dtype=np.float32)
    x = (u - np.float32(127.5)) / np.float32(127.5)
    want = (x.astype(np.float32) * np.float32(127.5) + np.float32(127.5)).astype(np.uint8)     # in range: numpy's own cast
    assert np.array_equal(vo.to_uint8(x, mobilenet=True), want)
    assert vo.to_uint8(np.float32([-1.5, 1.5]), mobilenet=True).tolist() == [0, 255]
    assert vo.to_uint8(np.float32([-3.0, 0.99, 254.99, 300.0])).tolist() == [0, 0, 254, 255]


class _Args:
    """ubd_visualize_images with every argument under the test's control; the pointers are never followed on the host"""

    def __init__(self):
        self.lib = _lib.load()
        self.buf = np.zeros(64, dtype=np.uint8)
        p = self.buf.ctypes.data
        self.a = dict(images=p, in_dtype=_lib.UBD_IN_U8, pre=_lib.UBD_PRE_NONE, n=1, h=8, w=12, c=3, mh=2, mw=3, gt=p, seg=p, quads=p,
                      counts=p, cap=1, cls=p, o_gt=p, o_seg=p, o_post=p, o_cls=p)

    def __call__(self, **kw):
        a = dict(self.a)
        a.update(kw)
        return self.lib.ubd_visualize_images(a["images"], a["in_dtype"], a["pre"], a["n"], a["h"], a["w"], a["c"], a["mh"], a["mw"], a["gt"],
                                             a["seg"], a["quads"], a["counts"], a["cap"], a["cls"], a["o_gt"], a["o_seg"], a["o_post"],
                                             a["o_cls"], None)


BAD_CALLS = [
    ("null images", dict(images=None), b"null images"),
    ("out_gt without gt_labels", dict(gt=None), b"out_gt given without"),
    ("out_seg_map without binary_map", dict(seg=None), b"out_seg_map given without"),
    ("out_postprocessed without quads", dict(quads=None), b"out_postprocessed given without"),
    ("out_postprocessed without counts", dict(counts=None), b"out_postprocessed given without"),
    ("out_classification_gt without cls_mask", dict(cls=None), b"out_classification_gt given without"),
    ("channels = 2", dict(c=2), b"channels"),
    ("height != s * map_h", dict(h=9), b"integer multiple"),
    ("ratios differ on the two axes", dict(h=8, mh=2, w=12, mw=4), b"integer multiple"),
    ("a side of 0", dict(h=0), b"bad sizes"),
    ("a map side of 0", dict(mw=0), b"bad sizes"),
    ("a side above 16384", dict(w=16388, mw=4097, h=4, mh=1), b"too large"),
    ("n * H * W * 3 >= 2^31", dict(n=3, h=16384, w=16384, mh=4096, mw=4096), b"2^31"),
    ("n = 0", dict(n=0), b"n must be"),
    ("unknown input type", dict(in_dtype=7), b"in_dtype"),
    ("cap = 0", dict(cap=0), b"cap"),
]


@pytest.mark.parametrize("name,kw,msg", BAD_CALLS, ids=[b[0] for b in BAD_CALLS])
def test_contract_violations_are_refused_before_any_launch(name, kw, msg):
    call = _Args()
    assert call(**kw) != 0, name
    err = call.lib.ubd_last_error()
    assert err.startswith(b"ubd_visualize_images") and msg in err, (name, err)


def test_largest_accepted_product_is_below_2_pow_31():
    """the size limit is on n * H * W * 3 itself: two images of 16384 x 16384 (3 * 2^29 bytes) pass, three do not (sizes only:
    no output is asked for, so the accepted call returns before any launch)"""
    call = _Args()
    none = dict(o_gt=None, o_seg=None, o_post=None, o_cls=None)
    assert call(n=2, h=16384, w=16384, mh=4096, mw=4096, **none) == 0           # 3 * 2^29 < 2^31
    assert call(n=3, h=16384, w=16384, mh=4096, mw=4096, **none) != 0


def _metrics(tp, fp, fn, detection_rate):
    m = FtMetrics()
    m.tp, m.fp, m.fn, m.detection_rate = tp, fp, fn, detection_rate
    return m


def test_image_result_categories():
    C = ImageResultCategories
    assert (C.RECALL_ERROR, C.PRECISION_ERROR, C.DETECTION_RATE_ERROR, C.ALL) == ('errors/recall', 'errors/precision', 'errors/detection_rate', 'all')
    assert C.SUITABLE_CATEGORIES == (C.RECALL_ERROR, C.DETECTION_RATE_ERROR, C.ALL) == C.get_folders()
    assert C.get_categories(_metrics(3, 0, 0, 1)) == [C.ALL]                                        # perfect
    assert C.get_categories(_metrics(2, 0, 1, 1)) == [C.RECALL_ERROR, C.ALL]                        # recall < 1
    assert C.get_categories(_metrics(3, 2, 0, 1)) == [C.ALL]                                        # precision < 1 only: not suitable
    assert C.get_categories(_metrics(3, 0, 0, 0)) == [C.DETECTION_RATE_ERROR, C.ALL]                # detection rate < 1
    assert C.get_categories(_metrics(1, 1, 1, 0)) == [C.DETECTION_RATE_ERROR, C.RECALL_ERROR, C.ALL]
    assert C.get_errors([C.DETECTION_RATE_ERROR, C.RECALL_ERROR, C.ALL]) == [C.DETECTION_RATE_ERROR, C.RECALL_ERROR]
    assert C.get_errors([C.ALL]) == []


class _Meta:
    def __init__(self, filename):
        self.filename, self.xscale, self.yscale = filename, 1.0, 1.0


def test_result_saver_writes_the_reference_tree(tmp_path):
    rng = np.random.default_rng(4)
    C = ImageResultCategories
    save_dir = str(tmp_path / "run")
    saver = ResultSaver(save_dir, save_visualizations=True)
    assert saver.save_dir == save_dir
    for folder in ("markup", "predictions", "images/all", "images/errors/recall", "images/errors/detection_rate"):
        assert os.path.isdir(os.path.join(save_dir, folder)), folder
    assert not os.path.exists(os.path.join(save_dir, "images", "errors", "precision"))
    metas = [_Meta("a.jpg"), _Meta("b"), _Meta("c")]
    gt = [[ObjectMarkup([1, 2, 9, 2, 9, 8, 1, 8])], [ClassifiedObjectMarkup([0, 0, 4, 0, 4, 4, 0, 4], 2)], []]
    found = [[ObjectMarkup([1, 2, 9, 2, 9, 7, 1, 7]), ObjectMarkup([3, 3, 5, 3, 5, 5, 3, 5])], [], []]
    saver.save_gt_and_prediction(gt, found, metas)
    assert open(os.path.join(save_dir, "markup", "a.jpg.txt")).read() == '1,2,9,2,9,8,1,8,""\n'
    assert open(os.path.join(save_dir, "markup", "b.txt")).read() == '0,0,4,0,4,4,0,4,"",2\n'
    assert open(os.path.join(save_dir, "predictions", "a.jpg.txt")).read() == '1,2,9,2,9,7,1,7,""\n3,3,5,3,5,5,3,5,""\n'
    assert open(os.path.join(save_dir, "predictions", "c.txt")).read() == ''
    vis = {tag: rng.integers(0, 256, (3, 6, 10, 3), dtype=np.uint8) for tag in ("gt", "seg_map", "postprocessed", "classification_gt")}
    categories = [[C.RECALL_ERROR, C.ALL], [], [C.ALL]]
    saver.save_visualizations(categories, metas, vis)
    written = sorted(os.path.relpath(os.path.join(d, f), os.path.join(save_dir, "images")) for d, _, fs in os.walk(os.path.join(save_dir, "images")) for f in fs)
    want = sorted(os.path.join(cat, f"{m.filename}.{tag}.png") for m, cats in zip(metas, categories) for cat in cats for tag in vis)
    assert written == want and len(written) == 12
    for i, (m, cats) in enumerate(zip(metas, categories)):
        for cat in cats:
            for tag in vis:
                back = np.array(Image.open(os.path.join(save_dir, "images", cat, f"{m.filename}.{tag}.png")))
                assert back.dtype == np.uint8 and np.array_equal(back, vis[tag][i]), (m.filename, cat, tag)
    # without save_dir nothing is made and nothing is written; without save_visualizations no images folder
    assert ResultSaver(None, True).save_dir is None
    ResultSaver(None, True).save_visualizations(categories, metas, vis)
    plain = ResultSaver(str(tmp_path / "plain"), False)
    plain.save_visualizations(categories, metas, vis)
    assert sorted(os.listdir(str(tmp_path / "plain"))) == ["markup", "predictions"]


def _gpu_present():
    import torch
    return torch.cuda.is_available()


@pytest.mark.skipif(_gpu_present(), reason="GPU present: the refusal to run without one cannot be seen")
def test_visualizer_has_no_cpu_fallback():
    from ubdvss_amd import Visualizer
    img = np.zeros((1, 8, 8, 3), np.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Visualizer.compute_visualizations(img, np.zeros((1, 2, 2)), np.zeros((1, 2, 2)), [[]])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Visualizer.visualize_segmentation_map(img[0], np.zeros((2, 2)))
