"""GPU: ubd_segmap_polygons (segmentation maps -> hull polygons) against the sequential restatement of cv2's contour tracing
and convex hull (oracle/cv_post.c), and ubdvss_amd.markup_readers.segmap_polygons on top of it.  Integers, so everything is
compared exactly: the objects, their order, the vertex counts and the vertex cycles."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))          # the helper modules beside this file
import segmap_cases as sc  # noqa: E402
from ubdvss_amd import _lib, markup_readers  # noqa: E402

pytestmark = pytest.mark.gpu
MAXV = _lib.UBD_POLY_MAX_VERTS


def _raw(maps, cap, workspace_bytes=None, n=None, h=None, w=None):
    """one call; returns (rc, verts, nverts, counts) with the outputs pre-filled with -7 (what a call that launches nothing leaves)"""
    lib = _lib.load()
    m = torch.from_numpy(np.ascontiguousarray(maps)).cuda()
    n0, h0, w0 = maps.shape
    n, h, w = n0 if n is None else n, h0 if h is None else h, w0 if w is None else w
    need = int(lib.ubd_segmap_polygons_workspace_bytes(n0, h0, w0, min(max(cap, 1), _lib.UBD_EVAL_MAX_GT)))
    ws = torch.empty(max(need, 256), dtype=torch.uint8, device="cuda")
    alloc = max(cap, 1)
    verts = torch.full((n0, alloc, MAXV, 2), -7, dtype=torch.int32, device="cuda")
    nverts = torch.full((n0, alloc), -7, dtype=torch.int32, device="cuda")
    counts = torch.full((n0,), -7, dtype=torch.int32, device="cuda")
    rc = lib.ubd_segmap_polygons(m.data_ptr(), n, h, w, verts.data_ptr(), nverts.data_ptr(), counts.data_ptr(), cap, ws.data_ptr(),
                                 need if workspace_bytes is None else workspace_bytes,
                                 ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, verts.cpu().numpy(), nverts.cpu().numpy(), counts.cpu().numpy()


def _check(maps, cap=64):
    rc, verts, nverts, counts = _raw(maps, cap)
    assert rc == 0, _lib.load().ubd_last_error()
    sizes = []
    for i, m in enumerate(maps):
        want = sc.expected_polygons(m)
        assert counts[i] == len(want), (i, counts[i], len(want))
        for o, p in enumerate(want):
            assert nverts[i, o] == len(p), (i, o, nverts[i, o], len(p))
            k = min(len(p), MAXV)
            assert np.array_equal(verts[i, o, :k], p[:k]), (i, o, verts[i, o, :k].tolist(), p.tolist())
            sizes.append(len(p))
    return sizes


def test_odd_sized_maps_objects_order_and_vertex_cycles():
    maps = sc.odd_maps()
    assert set(np.unique(maps)) == {0, 1, 200, 255}
    sizes = _check(maps)
    assert 1 in sizes and 2 in sizes and max(sizes) >= 10       # a single pixel, straight lines, rotated rectangles


def test_all_zero_and_all_ones_maps():
    maps = np.stack([np.zeros((37, 53), np.uint8), np.ones((37, 53), np.uint8)])
    rc, verts, nverts, counts = _raw(maps, 8)
    assert rc == 0 and counts.tolist() == [0, 1] and nverts[1, 0] == 4
    assert verts[1, 0, :4].tolist() == [[52, 36], [0, 36], [0, 0], [52, 0]]
    _check(maps, 8)


def test_a_map_above_the_size_at_which_the_labellings_change_path():
    m = sc.large_map()
    assert m.size > 16384
    sizes = _check(m[None])
    assert max(sizes) >= 28


def test_a_hull_above_the_limit_reports_its_true_size_and_the_reader_raises():
    m = sc.big_ellipse_map()
    want = sc.expected_polygons(m)
    assert len(want) == 1 and len(want[0]) > MAXV
    rc, verts, nverts, counts = _raw(m[None], 4)
    assert rc == 0 and counts[0] == 1 and nverts[0, 0] == len(want[0])
    assert np.array_equal(verts[0, 0], want[0][:MAXV])          # the first 64 vertices are stored
    with pytest.raises(ValueError, match=f"image 0, object 0.*{len(want[0])} vertices"):
        markup_readers.segmap_polygons(m[None])


def test_truncated_list_is_reported_through_counts():
    maps = sc.odd_maps()[2:3]
    total = len(sc.expected_polygons(maps[0]))
    rc, verts, nverts, counts = _raw(maps, 5)
    assert rc == 0 and total > 5 and counts[0] == total
    assert ((nverts[0] >= 1) & (nverts[0] <= MAXV)).all()


def test_the_python_entry_drops_small_hulls_and_keeps_order(caplog):
    maps = sc.odd_maps()
    import logging
    with caplog.at_level(logging.INFO):
        markup = markup_readers.segmap_polygons(maps, object_type=5)
    dropped = 0
    for i, m in enumerate(maps):
        want = [p for p in sc.expected_polygons(m)]
        dropped += sum(len(p) < 3 for p in want)
        kept = [p for p in want if len(p) >= 3]
        assert len(markup[i]) == len(kept)
        for obj, p in zip(markup[i], kept):
            assert obj.object_type == 5 and np.asarray(obj.bbox).tolist() == p.reshape(-1).tolist()
    assert dropped > 0 and f"{dropped} component(s)" in caplog.text


def test_bad_arguments_launch_nothing():
    lib = _lib.load()
    maps = sc.odd_maps()
    cases = [dict(cap=0), dict(cap=_lib.UBD_EVAL_MAX_GT + 1), dict(cap=4, n=0), dict(cap=4, h=0), dict(cap=4, w=32768),
             dict(cap=4, workspace_bytes=16)]
    for kw in cases:
        rc, verts, nverts, counts = _raw(maps, **kw)
        assert rc != 0 and lib.ubd_last_error().startswith(b"ubd_segmap_polygons"), kw
        assert (counts == -7).all() and (nverts == -7).all() and (verts == -7).all(), kw
    assert lib.ubd_segmap_polygons_workspace_bytes(1, 40000, 4, 4) == 0 and lib.ubd_segmap_polygons_workspace_bytes(1, 4, 4, 0) == 0
    assert lib.ubd_segmap_polygons(None, 1, 4, 4, None, None, None, 4, None, 0, None) != 0
