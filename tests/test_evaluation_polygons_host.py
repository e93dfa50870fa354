"""CPU: the host side of polygon ground truth -- the committed cases of tests/eval_polygon_cases.py keep clear of every decision
threshold (so the GPU test may compare integers exactly), check_ground_truth_polygon with the 64-vertex limit, and the filtering
and the errors of ubdvss_amd.markup_readers with the device call replaced by arrays."""
import logging
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))          # the helper modules beside this file
import eval_oracle as eo  # noqa: E402
import eval_polygon_cases as pc  # noqa: E402
from ubdvss_amd import _lib, markup_readers  # noqa: E402
from ubdvss_amd import evaluation as ev  # noqa: E402

THR = ev.DatasetMetricCalculator.IOU_THRESHOLDS


def test_committed_cases_keep_clear_of_every_threshold_and_groups_stay_small():
    imgs = pc.batch()
    assert len(imgs) == 6
    sizes = [len(p) // 2 for g, _ in imgs for p in g]
    assert min(sizes) >= 9 and max(sizes) <= _lib.UBD_POLY_MAX_VERTS and max(sizes) >= 32, sizes
    kinds = dict(one_to_one=0, one_to_many=0, many_to_one=0, collinear=0)
    for variant in (imgs, pc.scaled(imgs)):
        for i, (g, f) in enumerate(variant):
            ev.pack_found_objects([f])                                   # integer convex quads
            T = eo.Tables([eo.poly(p) for p in g], [eo.poly(p) for p in f])
            for v in T.decision_values():
                for t in [0.05] + [float(x) for x in THR]:
                    assert abs(v - Fraction(t)) >= Fraction(1, 10 ** 6), (i, float(v), t)
            for members in [m[1] for m in T.one_to_manys] + [m[0] for m in T.many_to_ones]:
                assert len(members) + 1 <= 6, (i, members)
            kinds["one_to_one"] += len(T.one_to_ones)
            kinds["one_to_many"] += len(T.one_to_manys)
            kinds["many_to_one"] += len(T.many_to_ones)
    # edges of found boxes collinear with hull edges: the chamfered box of image 3 and its bounding box (unscaled variant)
    g, f = imgs[3]
    box = [q for q in f if len(set(q[0::2])) == 2 and len(set(q[1::2])) == 2]
    for q in box:
        for p in g:
            xs, ys = p[0::2], p[1::2]
            for k in range(len(xs)):
                k1 = (k + 1) % len(xs)
                if (ys[k] == ys[k1] and ys[k] in q[1::2]) or (xs[k] == xs[k1] and xs[k] in q[0::2]):
                    kinds["collinear"] += 1
    assert all(v >= 1 for v in kinds.values()) and kinds["collinear"] >= 4, kinds


def test_ground_truth_polygon_check_with_the_64_vertex_limit():
    ang = np.linspace(0, 2 * np.pi, 64, endpoint=False)
    gon64 = np.stack([500 + 400 * np.cos(ang), 500 + 300 * np.sin(ang)], axis=1).reshape(-1)
    assert ev.check_ground_truth_polygon(gon64, max_vertices=64).shape == (64, 2)
    assert ev.check_ground_truth_polygon(gon64[::-1].reshape(-1, 2)[:, ::-1].reshape(-1), max_vertices=64).shape == (64, 2)
    with pytest.raises(ValueError, match="64 vertices, the limit is 8"):
        ev.check_ground_truth_polygon(gon64)                            # the default stays UBD_EVAL_MAX_VERTS
    ang = np.linspace(0, 2 * np.pi, 65, endpoint=False)
    gon65 = np.stack([500 + 400 * np.cos(ang), 500 + 300 * np.sin(ang)], axis=1).reshape(-1)
    with pytest.raises(ValueError, match="image 3, object 1: 65 vertices, the limit is 64"):
        ev.check_ground_truth_polygon(gon65, 3, 1, max_vertices=64)
    dent = gon64.copy().reshape(-1, 2)
    dent[10] = (500, 500)
    with pytest.raises(ValueError, match="not convex"):
        ev.check_ground_truth_polygon(dent.reshape(-1), max_vertices=64)
    xy, first, _, image_first, max_gt = ev.pack_ground_truth([[gon64, [0, 0, 4, 0, 0, 4]], [[0, 0, 9, 0, 9, 9, 0, 9]]])
    assert np.diff(first).tolist() == [64, 3, 4] and image_first.tolist() == [0, 2, 3] and max_gt == 2 and xy.shape == (71, 2)
    with pytest.raises(ValueError, match="image 0, object 0: 65 vertices"):
        ev.pack_ground_truth([[gon65]])


def _arrays(objects_per_image, cap=4):
    """the outputs of ubd_segmap_polygons for lists of (k, 2) vertex arrays; an int entry k stands for a hull of k vertices of
    which only the first 64 are stored"""
    n = len(objects_per_image)
    verts = np.zeros((n, cap, _lib.UBD_POLY_MAX_VERTS, 2), np.int32)
    nverts = np.zeros((n, cap), np.int32)
    counts = np.zeros(n, np.int32)
    for i, objs in enumerate(objects_per_image):
        counts[i] = len(objs)
        for o, p in enumerate(objs[:cap]):
            if isinstance(p, int):
                nverts[i, o] = p
            else:
                verts[i, o, :len(p)] = p
                nverts[i, o] = len(p)
    return verts, nverts, counts


def test_reader_filtering_and_errors_with_the_device_call_stubbed(monkeypatch, caplog):
    tri = np.array([[9, 9], [2, 9], [5, 1]])
    quad = np.array([[8, 7], [1, 7], [1, 2], [8, 2]])
    line, dot = np.array([[7, 3], [2, 3]]), np.array([[4, 4]])
    arrays = _arrays([[tri, line, quad], [dot], [], [line, dot, tri]])
    monkeypatch.setattr(markup_readers, "_segmap_polygons_device", lambda maps, device=None: arrays)
    with caplog.at_level(logging.INFO):
        markup = markup_readers.segmap_polygons(np.zeros((4, 10, 10), np.uint8))
    assert [len(m) for m in markup] == [2, 0, 0, 1]
    assert "4 component(s)" in caplog.text
    assert [np.asarray(o.bbox).tolist() for o in markup[0]] == [[9, 9, 2, 9, 5, 1], [8, 7, 1, 7, 1, 2, 8, 2]]
    assert all(o.object_type == 5 and np.asarray(o.bbox).dtype.kind == "i" for m in markup for o in m)
    assert markup_readers.segmap_polygons(np.zeros((4, 10, 10), np.uint8), object_type=2)[3][0].object_type == 2
    with pytest.raises(ValueError, match="image 1, object 2.*72 vertices, the limit is 64"):
        markup_readers._markup_from_arrays(*_arrays([[tri], [tri, quad, 72]]))
    with pytest.raises(ValueError, match="image 1: 5 objects, the limit is 4"):
        markup_readers._markup_from_arrays(*_arrays([[tri], [tri, quad, tri, quad, tri]]))


def test_reader_shell_groups_by_size_and_keeps_the_interface(monkeypatch, tmp_path):
    from PIL import Image
    os.makedirs(tmp_path / "Image")
    os.makedirs(tmp_path / "Detection")
    sizes = {"a": (12, 10), "b": (16, 8), "c": (12, 10)}
    for name, (w, h) in sizes.items():
        Image.new("RGB", (w, h), (10, 20, 30)).save(tmp_path / "Image" / f"{name}.jpg")
        Image.new("L", (w, h), 0).save(tmp_path / "Detection" / f"{name}.png")
    Image.new("L", (4, 4), 0).save(tmp_path / "Detection" / "orphan.png")     # no image: logged and skipped, as in the reference
    (tmp_path / "Detection" / "notes.txt").write_text("not a map")
    calls = []

    def stub(maps, device=None):
        calls.append(maps.shape)
        tri = np.array([[9, 7], [2, 7], [5, 1]])
        return _arrays([[tri]] * len(maps))
    monkeypatch.setattr(markup_readers, "_segmap_polygons_device", stub)
    reader = markup_readers.SegmentationMapMarkupReader(str(tmp_path), None)
    reader.read_markup()
    assert sorted(calls) == [(1, 8, 16), (2, 10, 12)]
    assert sorted(reader.get_list_of_images()) == ["a", "b", "c"]
    assert np.asarray(reader.get_image_markup("b")[0].bbox).tolist() == [9, 7, 2, 7, 5, 1]
    im = reader.get_image("c")
    assert im.mode == "RGB" and im.size == (12, 10)
