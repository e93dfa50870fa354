"""GPU: ubd_visualize_images and ubdvss_amd.visualizations against the Pillow calls of tests/visualization_oracle.py.

Every comparison is of uint8 images and bit-identical: the blend is exact integer arithmetic, the polygon rule is pinned to
Pillow, the fp32 denorm is exact once product and sum are rounded separately.  Each case names what it is there to catch.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))          # the helper modules beside this file
import visualization_oracle as vo  # noqa: E402
from ubdvss_amd import NetConfig, Model, ModelRunner, ClassifiedObjectMarkup, ObjectMarkup, Visualizer, _lib  # noqa: E402
from ubdvss_amd import evaluation as ev  # noqa: E402
from ubdvss_amd.net import PreprocessingType  # noqa: E402

pytestmark = pytest.mark.gpu

KEYS = ("gt", "seg_map", "postprocessed", "classification_gt")
POISON = 0xA5


def _sources(seed, n, mh, mw, s, channels, cap=3, dtype=np.uint8):
    """random images, label maps, binary maps, classification masks and a few boxes per image"""
    rng = np.random.default_rng(seed)
    h, w = mh * s, mw * s
    images = rng.integers(0, 256, (n, h, w, channels), dtype=np.uint8).astype(dtype)
    gt = rng.integers(-1, 3, (n, mh, mw)).astype(np.int32)                       # negative and 0: background
    seg = rng.integers(0, 2, (n, mh, mw)).astype(np.int32)
    cls = rng.integers(-1, 2, (n, mh, mw)).astype(np.int8)
    quads = np.zeros((n, cap, 8), np.int32)
    counts = rng.integers(0, cap + 1, n).astype(np.int32)
    for i in range(n):
        for j in range(cap):
            x0, y0 = int(rng.integers(-2, w)), int(rng.integers(-2, h))
            bw, bh = int(rng.integers(1, max(2, w // 2))), int(rng.integers(1, max(2, h // 2)))
            quads[i, j] = [x0, y0, x0 + bw, y0 + 1, x0 + bw - 1, y0 + bh, x0 - 1, y0 + bh - 1]
    return images, gt, seg, quads, counts, cls


class _Raw:
    """the C entry point on device copies of host sources; outputs are poisoned before the call and longer than needed"""
    EXTRA = 2                                                                    # images of room behind the n the call gets

    def __init__(self, images, gt, seg, quads, counts, cls):
        self.lib = _lib.load()
        self.host = dict(images=images, gt=gt, seg=seg, quads=quads, counts=counts, cls=cls)
        self.n, self.h, self.w, self.c = images.shape
        self.mh, self.mw = gt.shape[1:]
        self.cap = quads.shape[1]
        self.d = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in self.host.items()}
        self.out = {k: torch.full((self.n + self.EXTRA, self.h, self.w, 3), POISON, dtype=torch.uint8, device="cuda") for k in KEYS}

    def __call__(self, keys=KEYS, pre=_lib.UBD_PRE_NONE, n=None, **kw):
        a = dict(images=self.d["images"].data_ptr(), n=self.n if n is None else n, gt=self.d["gt"].data_ptr(), seg=self.d["seg"].data_ptr(),
                 quads=self.d["quads"].data_ptr(), counts=self.d["counts"].data_ptr(), cap=self.cap, cls=self.d["cls"].data_ptr())
        a.update(kw)
        o = [self.out[k].data_ptr() if k in keys else None for k in KEYS]
        in_dtype = _lib.UBD_IN_U8 if self.host["images"].dtype == np.uint8 else _lib.UBD_IN_F32
        return self.lib.ubd_visualize_images(a["images"], in_dtype, pre, a["n"], self.h, self.w, self.c, self.mh, self.mw, a["gt"], a["seg"],
                                             a["quads"], a["counts"], a["cap"], a["cls"], o[0], o[1], o[2], o[3],
                                             torch.cuda.current_stream().cuda_stream)

    def oracle(self, mobilenet=False):
        h = self.host
        return vo.pillow_all(h["images"], h["gt"], h["seg"], h["quads"], h["counts"], h["cls"], mobilenet=mobilenet)

    def check(self, want, keys=KEYS, n=None, where=""):
        """the asked outputs equal the oracle on the first n images; everything else still holds the poison"""
        n = self.n if n is None else n
        torch.cuda.synchronize()
        for k in KEYS:
            got = self.out[k].cpu().numpy()
            if k in keys:
                diff = int((got[:n] != want[k][:n]).sum())
                assert diff == 0, f"{where} {k}: {diff} bytes differ, first at {np.argwhere(got[:n] != want[k][:n])[0].tolist()}"
                assert (got[n:] == POISON).all(), f"{where} {k}: bytes behind image {n} were written"
            else:
                assert (got == POISON).all(), f"{where} {k}: written although its pointer was NULL"


def _all_at_once_and_each_alone(raw, want, where, **kw):
    assert raw(**kw) == 0, raw.lib.ubd_last_error()
    raw.check(want, where=where + " all four")
    for k in KEYS:
        for o in raw.out.values():
            o.fill_(POISON)
        assert raw(keys=(k,), **kw) == 0, raw.lib.ubd_last_error()
        raw.check(want, keys=(k,), where=where + " alone")


# (name, n, map_h, map_w, s, channels): what each shape is there to catch
SHAPES = [
    ("s4_rgb_8x12_partial_last_block", 2, 2, 3, 4, 3),          # one lane run per map entry; the last block is partial
    ("s1_rgb_5x7_unaligned_rows", 3, 5, 7, 1, 3),               # 21-byte row pitch: byte stores, row tail; image 1 starts at parity 1
    ("s2_runs_straddle_map_entries", 2, 6, 10, 2, 3),           # a run of four pixels covers two map entries
    ("s3_runs_straddle_map_entries", 2, 6, 10, 3, 3),           # 30-pixel rows: entries change inside a run, tail of 2
    ("s4_grey_64x64_channel_replication", 2, 16, 16, 4, 1),
    ("s1_grey_5x7_unaligned_grey_loads", 3, 5, 7, 1, 1),
    ("s4_rgb_wide_rows_two_tiles_across", 1, 3, 80, 4, 3),      # 320-pixel rows: 80 runs, more than one 64-run tile across
]


@pytest.mark.parametrize("name,n,mh,mw,s,channels", SHAPES, ids=[c[0] for c in SHAPES])
def test_shapes_against_pillow(name, n, mh, mw, s, channels):
    raw = _Raw(*_sources(len(name), n, mh, mw, s, channels))
    _all_at_once_and_each_alone(raw, raw.oracle(), name)


def _quad_case():
    """64 x 64, N = 3, cap = 4, counts (0, 2, 6): an empty image and one over cap (clamped to 4: the first four are drawn)"""
    rng = np.random.default_rng(8)
    images = rng.integers(0, 256, (3, 64, 64, 3), dtype=np.uint8)
    z = np.zeros((3, 16, 16), np.int32)
    quads = np.zeros((3, 4, 8), np.int32)
    quads[0, 0] = [5, 5, 30, 5, 30, 20, 5, 20]                   # not drawn: count 0
    quads[1, 0] = [10, 12, 40, 12, 40, 33, 10, 33]               # axis-aligned box
    quads[1, 1] = [31, 4, 58, 22, 44, 43, 17, 25]                # rotated box
    quads[1, 2] = [0, 0, 63, 0, 63, 63, 0, 63]                   # not drawn: behind the count
    quads[2, 0] = [8, 8, 40, 30, 40, 8, 8, 30]                   # self-intersecting ("bow tie")
    quads[2, 1] = [-20, 40, 30, 35, 90, 70, 10, 75]              # corners left of, right of and below the image
    quads[2, 2] = [50, 3, 50, 28, 50, 28, 50, 3]                 # one pixel wide
    quads[2, 3] = [20, 20, 45, 22, 43, 50, 18, 47]               # overlaps the bow tie and the wide quad
    counts = np.array([0, 2, 6], np.int32)
    return images, z, z.copy(), quads, counts, z.astype(np.int8)


def test_quads_drawn_with_pillows_polygon_rule():
    raw = _Raw(*_quad_case())
    want = raw.oracle()
    assert (want["postprocessed"][0] == raw.host["images"][0]).all() and (want["postprocessed"][2] != raw.host["images"][2]).any()
    _all_at_once_and_each_alone(raw, want, "quads")
    # wholly outside on every side, and more quads than one staging round holds (cap = 70)
    rng = np.random.default_rng(9)
    images = rng.integers(0, 256, (2, 40, 52, 3), dtype=np.uint8)
    quads = np.zeros((2, 70, 8), np.int32)
    quads[0, :4] = [[-30, -30, -5, -30, -5, -5, -30, -5], [60, 5, 90, 5, 90, 30, 60, 30], [5, 45, 30, 45, 30, 70, 5, 70], [-9, 3, -1, 3, -1, 30, -9, 30]]
    for j in range(70):
        x0, y0 = int(rng.integers(0, 48)), int(rng.integers(0, 36))
        quads[1, j] = [x0, y0, x0 + 3, y0, x0 + 3, y0 + 2, x0, y0 + 2]
    z = np.zeros((2, 40, 52), np.int32)
    raw = _Raw(images, z, z.copy(), quads, np.array([4, 70], np.int32), z.astype(np.int8))
    want = raw.oracle()
    assert (want["postprocessed"][0] == images[0]).all()
    assert raw(keys=("postprocessed",)) == 0, raw.lib.ubd_last_error()
    raw.check(want, keys=("postprocessed",), where="outside / 70 quads")


def test_float_inputs_denorm_and_clamp():
    # every u in 0..255 as (u - 127.5) / 127.5 in fp32, then -1.5 and 1.5 (clamped), padded to 8 x 36 x 3 with repeats
    u = np.arange(256, dtype=np.float32)
    vals = np.concatenate([(u - np.float32(127.5)) / np.float32(127.5), np.float32([-1.5, 1.5])]).astype(np.float32)
    _, gt, seg, quads, counts, cls = _sources(5, 1, 8, 36, 1, 3)
    images = np.resize(vals, (1, 8, 36, 3)).astype(np.float32)
    raw = _Raw(images, gt, seg, quads, counts, cls)
    want = raw.oracle(mobilenet=True)
    assert set(np.unique(vo.to_uint8(images, True))) == set(range(256))
    assert raw(pre=_lib.UBD_PRE_MOBILENET) == 0, raw.lib.ubd_last_error()
    raw.check(want, where="mobilenet denorm")
    # UBD_PRE_NONE: fractional values truncate toward zero, values outside [0, 255] clamp; grey, odd width (unaligned float rows)
    rng = np.random.default_rng(6)
    _, gt, seg, quads, counts, cls = _sources(7, 2, 6, 7, 1, 1)
    images = rng.uniform(-20, 280, (2, 6, 7, 1)).astype(np.float32)
    images[0, 0, :4, 0] = [254.999, 255.0, 0.999, -0.5]
    raw = _Raw(images, gt, seg, quads, counts, cls)
    assert raw() == 0, raw.lib.ubd_last_error()
    raw.check(raw.oracle(), where="no preprocessing")


def test_fewer_images_than_the_buffers_hold_and_offset_outputs():
    images, gt, seg, quads, counts, cls = _sources(11, 3, 5, 7, 1, 3)
    raw = _Raw(images, gt, seg, quads, counts, cls)
    want = raw.oracle()
    assert raw(n=2) == 0, raw.lib.ubd_last_error()
    raw.check(want, n=2, where="n = 2 of 3")
    # outputs that start at an odd byte: every run takes the byte path or the dword path by its own address
    flat = torch.full((3 * 5 * 7 * 3 + 9,), POISON, dtype=torch.uint8, device="cuda")
    lib = raw.lib
    assert lib.ubd_visualize_images(raw.d["images"].data_ptr(), _lib.UBD_IN_U8, 0, 3, 5, 7, 3, 5, 7, raw.d["gt"].data_ptr(), None, None, None, 0, None,
                                    flat.data_ptr() + 3, None, None, None, torch.cuda.current_stream().cuda_stream) == 0, lib.ubd_last_error()
    torch.cuda.synchronize()
    got = flat.cpu().numpy()
    assert (got[:3] == POISON).all() and (got[-6:] == POISON).all()
    assert np.array_equal(got[3:-6].reshape(3, 5, 7, 3), want["gt"])


def test_capture_in_a_hip_graph():
    raw = _Raw(*_sources(12, 2, 6, 10, 4, 3))
    want = raw.oracle()
    assert raw() == 0 and raw() == 0, raw.lib.ubd_last_error()
    raw.check(want, where="direct")
    direct = {k: raw.out[k].clone() for k in KEYS}
    for o in raw.out.values():
        o.fill_(POISON)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        assert raw() == 0, raw.lib.ubd_last_error()
    for o in raw.out.values():
        o.fill_(POISON)
    g.replay()
    torch.cuda.synchronize()
    for k in KEYS:
        assert torch.equal(raw.out[k], direct[k]), k


def test_public_wrappers():
    images, gt, seg, quads, counts, cls = _sources(13, 2, 4, 6, 4, 3, cap=2)
    want = vo.pillow_all(images, gt, seg, quads, counts, cls)
    dev = [torch.from_numpy(a).cuda() for a in (images, gt, seg, quads, counts, cls)]
    out = Visualizer.compute_visualizations_on_device(dev[0], dev[1][..., None], dev[2], (dev[3], None, dev[4]), dev[5])
    assert sorted(out) == sorted(KEYS)
    for k in KEYS:
        assert out[k].is_cuda and out[k].dtype == torch.uint8 and np.array_equal(out[k].cpu().numpy(), want[k]), k
    assert "classification_gt" not in Visualizer.compute_visualizations_on_device(dev[0], dev[1], dev[2], (dev[3], dev[4]))
    # numpy in, numpy out, markup lists; float maps are thresholded at 0.5
    markups = [[ObjectMarkup(quads[i, j]) for j in range(min(int(counts[i]), 2))] for i in range(2)]
    host = Visualizer.compute_visualizations(images, gt.astype(np.float32) * 0.6, seg[..., None], markups, cls.astype(np.float32))
    assert np.array_equal(host["gt"], vo.pillow_all(images, gt=gt.astype(np.float32) * 0.6)["gt"])
    for k in ("seg_map", "postprocessed", "classification_gt"):
        assert isinstance(host[k], np.ndarray) and np.array_equal(host[k], want[k]), k
    prob = np.random.default_rng(1).random((4, 6)).astype(np.float32)
    assert np.array_equal(Visualizer.visualize_segmentation_map(images[0], prob, threshold=0.3), vo.pillow_segmentation(images[0], prob, 0.3))
    assert np.array_equal(Visualizer.visualize_segmentation_maps(images, seg), want["seg_map"])
    assert np.array_equal(Visualizer.visualize_classification_mask(images[1], cls[1]), want["classification_gt"][1])
    assert np.array_equal(Visualizer.visualize_classification_masks(images, cls), want["classification_gt"])
    assert np.array_equal(Visualizer.draw_bboxes(images, markups), want["postprocessed"])
    assert np.array_equal(Visualizer.draw_markup(images[0], markups[0]), want["postprocessed"][0])
    with pytest.raises(ValueError, match="device tensor"):
        Visualizer.compute_visualizations_on_device(torch.from_numpy(images), dev[1], dev[2], (dev[3], dev[4]))
    with pytest.raises(ValueError, match="device tensor"):
        Visualizer.compute_visualizations_on_device(images, dev[1], dev[2], (dev[3], dev[4]))
    # mobilenet-preprocessed float images are drawn as the pixels they came from
    x = ((images.astype(np.float32) - 127.5) / 127.5).astype(np.float32)
    out = Visualizer.compute_visualizations_on_device(torch.from_numpy(x).cuda(), dev[1], dev[2], (dev[3], dev[4]),
                                                      preprocessing=PreprocessingType.MOBILENET_LIKE)
    assert np.array_equal(out["seg_map"].cpu().numpy(), vo.pillow_all(x, seg=seg, mobilenet=True)["seg_map"])


class _Meta:
    def __init__(self, filename):
        self.filename, self.xscale, self.yscale = filename, 1.0, 1.0


def test_end_to_end_through_the_model_runner(tmp_path):
    cfg = NetConfig(class_names=["a", "b", "c"], grey=False)
    rng = np.random.default_rng(21)
    images = rng.integers(0, 256, (2, 64, 64, 3), dtype=np.uint8)
    labels = np.zeros((2, 16, 16), np.int32)
    labels[0, 3:9, 2:12] = 1
    labels[1, 5:14, 6:10] = 3
    gt_objects = [[ClassifiedObjectMarkup([8, 12, 48, 12, 48, 36, 8, 36], 0)], [ClassifiedObjectMarkup([24, 20, 40, 20, 40, 56, 24, 56], 2)]]
    model = Model(cfg, seed=0)
    runner = ModelRunner(cfg)
    x, lab = torch.from_numpy(images).cuda(), torch.from_numpy(labels).cuda()
    logits, bmap, quads, classes, counts = runner.predict_on_device(model, x)
    rec, mask = ev.DatasetMetricCalculator(cfg).evaluate_batch(gt_objects, (quads, classes, counts), gt_segmap=lab, classification_logits=logits)
    out = Visualizer.compute_visualizations_on_device(x, lab, bmap, (quads, classes, counts), mask)
    torch.cuda.synchronize()
    want = vo.pillow_all(images, labels, bmap.cpu().numpy(), quads.cpu().numpy(), counts.cpu().numpy(), mask.cpu().numpy())
    assert sorted(out) == sorted(KEYS)
    for k in KEYS:
        assert np.array_equal(out[k].cpu().numpy(), want[k]), k
    categories = ev.ImageResultCategories.get_batch_categories(rec)
    assert len(categories) == 2 and all(c[-1] == "all" for c in categories)
    # ModelRunner.run: saves the CSVs and every categorised image, returns the last batch drawn
    metas = [_Meta("first.png"), _Meta("second")]
    save_dir = str(tmp_path / "out")
    logs, vis = ModelRunner(cfg).run(model, [(images, gt_objects, metas, labels)], 2, save_dir=save_dir, save_visualizations=True)
    assert sorted(vis) == sorted(KEYS) and "f1_iou0.50" in logs and "classification_pixel_acc_total" in logs
    for k in KEYS:
        assert np.array_equal(vis[k].cpu().numpy(), want[k]), k
    for m, i in ((metas[0], 0), (metas[1], 1)):
        for k in KEYS:
            path = os.path.join(save_dir, "images", "all", f"{m.filename}.{k}.png")
            assert os.path.isfile(path), path
        from PIL import Image
        assert np.array_equal(np.array(Image.open(os.path.join(save_dir, "images", "all", f"{m.filename}.gt.png"))), want["gt"][i])
        assert os.path.isfile(os.path.join(save_dir, "markup", m.filename + ".txt")) and os.path.isfile(os.path.join(save_dir, "predictions", m.filename + ".txt"))
    # without save_dir: the batch that holds the drawn index is visualised; the index comes from the generator given
    batches = [(images[:1], gt_objects[:1], None, labels[:1]), (images[1:], gt_objects[1:], None, labels[1:])]
    pick = int(np.random.default_rng(5).integers(0, 2))
    logs2, vis2 = ModelRunner(cfg).run(model, batches, 2, rng=np.random.default_rng(5))
    assert sorted(vis2) == sorted(KEYS) and tuple(vis2["gt"].shape) == (1, 64, 64, 3)
    assert np.array_equal(vis2["gt"].cpu().numpy()[0], want["gt"][pick])
    assert set(logs2) == set(logs)
