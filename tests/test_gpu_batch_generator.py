"""GPU: BatchGenerator (the contract of data_generators.py:57-212) on a small data set of Image/ + Detection/ folders: every image
once per pass, one shape per batch, incomplete batches kept or skipped, pixels and label maps bit-equal to
prepare_batch_on_device on the same files, MetaInfo scales, the cache of the second pass; and with augmentation on an in-memory
quad reader."""
import os
import random

import numpy as np
import pytest
import torch
from PIL import Image

from ubdvss_amd import NetConfig, ObjectMarkup, SegmapManager
from ubdvss_amd.data_generators import BatchGenerator, MetaInfo

pytestmark = pytest.mark.gpu

# (w, h) of the source files, in name order: four map to 64 x 64 (side multiple 64), two to 64 high x 128 wide
SIZES = [(64, 64), (128, 64), (70, 60), (50, 80), (120, 70), (90, 40)]
SMALL, WIDE = ["img0", "img2", "img3", "img5"], ["img1", "img4"]


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    root = tmp_path_factory.mktemp("segmap_dataset")
    os.makedirs(root / "Image")
    os.makedirs(root / "Detection")
    rng = np.random.default_rng(8)
    for k, (w, h) in enumerate(SIZES):
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(root / "Image" / f"img{k}.png")
        seg = np.zeros((h, w), np.uint8)
        seg[h // 4:h // 4 + h // 3, w // 5:w // 5 + w // 2] = 255
        Image.fromarray(seg).save(root / "Detection" / f"img{k}.png")
    return str(root)


def _config():
    return NetConfig(grey=False, class_names=[f"t{i}" for i in range(6)])      # the reader labels every object type 5 (EAN13)


def _take(generator, n_batches):
    return [next(generator) for _ in range(n_batches)]


def test_one_pass_batches_and_bit_equal_pixels(dataset):
    cfg = _config()
    gen = BatchGenerator(dataset, 3, "BarcodeSegmap", cfg)
    assert (gen.get_images_per_epoch(), gen.get_epoch_size(), gen.is_augmentation_used()) == (6, 2, False)
    batches = _take(gen.generate(add_metainfo=True), 3)
    # sorted by element count (stable), grouped by shape, cut into threes: the 64 x 64 group first, its tail of one, then the wide pair
    assert [[m.filename for m in b[2]] for b in batches] == [SMALL[:3], SMALL[3:], WIDE]
    assert [tuple(b[0].shape) for b in batches] == [(3, 64, 64, 3), (1, 64, 64, 3), (2, 64, 128, 3)]
    assert [tuple(b[1].shape) for b in batches] == [(3, 16, 16, 1), (1, 16, 16, 1), (2, 16, 32, 1)]
    for x, y, _ in batches:
        assert x.is_cuda and x.dtype == torch.uint8 and y.is_cuda and y.dtype == torch.int32
    reader = gen._reader
    for names, got in ((SMALL, batches[:2]), (WIDE, batches[2:])):
        x, labels, _ = SegmapManager.prepare_batch_on_device([reader.get_image(n) for n in names],
                                                             [reader.get_image_markup(n) for n in names], cfg)
        assert torch.equal(torch.cat([b[0] for b in got]), x)
        assert torch.equal(torch.cat([b[1] for b in got])[..., 0], labels)
        assert int(labels.max()) == 6 and int((labels > 0).sum()) > 0           # type 5 -> label 6: the maps are not empty
    sizes = dict(zip([f"img{k}" for k in range(6)], SIZES))
    for x, _, metas in batches:
        for m in metas:
            w, h = sizes[m.filename]
            assert isinstance(m, MetaInfo) and m.xscale == w / x.shape[2] and m.yscale == h / x.shape[1]
            assert m.markup is reader.get_image_markup(m.filename)              # the markup on the ORIGINAL image
    # without metainfo: pairs, the same tensors
    plain = _take(BatchGenerator(dataset, 3, "BarcodeSegmap", cfg).generate(), 3)
    assert all(len(b) == 2 for b in plain)
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(plain, batches))


def test_incomplete_batches_are_skipped_on_request(dataset):
    gen = BatchGenerator(dataset, 3, "BarcodeSegmap", _config(), yield_incomplete_batches=False)
    batches = _take(gen.generate(add_metainfo=True), 3)                         # three PASSES: one full batch each
    assert [[m.filename for m in b[2]] for b in batches] == [SMALL[:3]] * 3
    assert all(tuple(b[0].shape) == (3, 64, 64, 3) for b in batches)


def test_second_pass_comes_from_the_cache(dataset, monkeypatch):
    gen = BatchGenerator(dataset, 3, "BarcodeSegmap", _config())
    calls = []
    original = gen._reader.get_image
    monkeypatch.setattr(gen._reader, "get_image", lambda name: (calls.append(name), original(name))[1])
    g = gen.generate()
    first = _take(g, 3)
    assert sorted(calls) == [f"img{k}" for k in range(6)]
    second, third = _take(g, 3), _take(g, 3)
    assert len(calls) == 6                                                      # nothing is read or prepared again
    for a, b, c in zip(first, second, third):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[0], c[0])
    first[0][0].zero_()                                                         # a consumer's write does not reach the cache
    assert torch.equal(_take(g, 1)[0][0], second[0][0])
    # a chunk smaller than the data set is never cached: every pass reads again
    gen2 = BatchGenerator(dataset, 3, "BarcodeSegmap", _config(), prepare_batch_size=4)
    calls2 = []
    original2 = gen2._reader.get_image
    monkeypatch.setattr(gen2._reader, "get_image", lambda name: (calls2.append(name), original2(name))[1])
    names = [[m.filename for m in b[2]] for b in _take(gen2.generate(add_metainfo=True), 6)]
    # chunks img0..3 and img4..5: [img0, img2, img3], [img1], then [img5], [img4]; then the next pass
    assert names == [["img0", "img2", "img3"], ["img1"], ["img5"], ["img4"], ["img0", "img2", "img3"], ["img1"]]
    assert len(calls2) == 6 + 4


def test_unreadable_image_is_skipped(dataset, monkeypatch):
    gen = BatchGenerator(dataset, 3, "BarcodeSegmap", _config())
    original = gen._reader.get_image

    def flaky(name):
        if name == "img2":
            raise OSError("truncated file")
        return original(name)

    monkeypatch.setattr(gen._reader, "get_image", flaky)
    names = [[m.filename for m in b[2]] for b in _take(gen.generate(add_metainfo=True), 2)]
    assert names == [["img0", "img3", "img5"], WIDE]


class _QuadReader:
    def __init__(self, sizes, vertices=4):
        rng = np.random.default_rng(17)
        self._images, self._markup = {}, {}
        for k, (w, h) in enumerate(sizes):
            self._images[f"q{k}"] = Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
            x0, y0, x1, y1 = w // 4, h // 4, 3 * w // 4, 3 * h // 4
            pts = [x0, y0, x1, y0, x1, y1, x0, y1]
            if vertices == 5:
                pts = [x0, y0, (x0 + x1) // 2, y0 - 3, x1, y0, x1, y1, x0, y1]
            self._markup[f"q{k}"] = [ObjectMarkup(np.array(pts))]

    def read_markup(self):
        pass

    def get_list_of_images(self):
        return list(self._images)

    def get_image_markup(self, name):
        return self._markup[name]

    def get_image(self, name):
        return self._images[name]


def test_augmented_pass_on_an_in_memory_reader():
    random.seed(4)
    np.random.seed(4)
    cfg = NetConfig(grey=True)
    gen = BatchGenerator("ignored", 2, _QuadReader([(100, 80), (100, 80), (160, 120), (90, 200), (100, 80)]), cfg, use_augmentation=True)
    with pytest.raises(AssertionError):
        next(gen.generate(add_metainfo=True))                                   # scales of augmented images would be wrong
    g = gen.generate()
    seen = 0
    while seen < gen.get_images_per_epoch():
        x, y = next(g)
        n, h, w, c = x.shape
        assert 1 <= n <= 2 and c == 1 and h % 64 == 0 and w % 64 == 0 and x.dtype == torch.uint8
        assert tuple(y.shape) == (n, h // 4, w // 4, 1) and y.dtype == torch.int32
        seen += n
    assert seen == gen.get_images_per_epoch()                                   # a pass ends on a batch boundary


def test_augmenting_polygon_markup_raises_with_the_file_name():
    gen = BatchGenerator("ignored", 2, _QuadReader([(100, 80), (100, 80)], vertices=5), NetConfig(grey=False), use_augmentation=True)
    with pytest.raises(ValueError, match="augmentation of polygon markup is not supported.*q0"):
        next(gen.generate())
    plain = BatchGenerator("ignored", 2, _QuadReader([(100, 80), (100, 80)], vertices=5), NetConfig(grey=False))
    x, y = next(plain.generate())                                               # without augmentation polygons are fine
    assert tuple(x.shape) == (2, 64, 128, 3) and int(y.max()) == 1
