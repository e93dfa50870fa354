"""Segmentation maps for the polygon ground-truth tests and their expected hull polygons (helper module, not collected).

The expected value of ubd_segmap_polygons is ``oracle.cv_post.find_contours`` followed by ``convex_hull``, the cycle reversed and
rotated to start at the vertex with the greatest x (the greatest y among equals): the cycle of cv2.convexHull with its defaults.
"""
import numpy as np

from oracle import cv_post


def expected_polygons(seg_map):
    """list (cv2's contour order) of (k, 2) int arrays"""
    out = []
    for cnt in cv_post.find_contours(np.asarray(seg_map)):
        hull = cv_post.convex_hull(cnt)[::-1]
        start = max(range(len(hull)), key=lambda k: (hull[k][0], hull[k][1]))
        out.append(np.roll(hull, -start, axis=0).astype(np.int32))
    return out


def rotated_rect_mask(h, w, cx, cy, a, b, angle):
    ys, xs = np.mgrid[0:h, 0:w]
    u = (xs - cx) * np.cos(angle) + (ys - cy) * np.sin(angle)
    v = -(xs - cx) * np.sin(angle) + (ys - cy) * np.cos(angle)
    return (np.abs(u) <= a) & (np.abs(v) <= b)


def ellipse_mask(h, w, cx, cy, a, b, angle=0.0):
    ys, xs = np.mgrid[0:h, 0:w]
    u = (xs - cx) * np.cos(angle) + (ys - cy) * np.sin(angle)
    v = -(xs - cx) * np.sin(angle) + (ys - cy) * np.cos(angle)
    return (u / a) ** 2 + (v / b) ** 2 <= 1.0


def odd_maps():
    """(3, 37, 53) uint8 with bytes from {0, 1, 200, 255}: rows do not line up with waves"""
    h, w = 37, 53
    maps = np.zeros((3, h, w), np.uint8)
    # 0: rotated rectangles, the reference's plus sign (markup_readers.py:276-281), a single pixel, a one-pixel-wide line
    maps[0][rotated_rect_mask(h, w, 14, 10, 9, 4, 0.5)] = 255
    maps[0][rotated_rect_mask(h, w, 38, 24, 11, 3, 2.1)] = 200
    maps[0, 24:29, 8] = 1
    maps[0, 26, 6:11] = 1
    maps[0, 34, 20] = 255
    maps[0, 2, 30:45] = 200
    maps[0, 30:36, 50] = 1                       # vertical line
    # 1: a ring with a component in its hole (not an object), diagonal-only contacts, components on the frame
    maps[1, 5:20, 5:25] = 255
    maps[1, 8:17, 8:22] = 0
    maps[1, 11:14, 12:17] = 200                  # inside the hole
    for k in range(6):
        maps[1, 24 + k, 30 + k] = 1              # a diagonal chain: one 8-connected component
    maps[1, 22, 40:44] = 255
    maps[1, 23, 44:48] = 255                     # two runs touching by a corner
    maps[1, 0, 0:7] = 1
    maps[1, 0:5, w - 1] = 200
    maps[1, h - 1, 20:31] = 255
    maps[1, h - 3:h, 0:2] = 1
    # 2: random blobs of all four byte values
    rng = np.random.default_rng(3)
    blob = rng.random((h, w)) < 0.42
    maps[2] = np.where(blob, rng.choice(np.array([1, 200, 255], np.uint8), (h, w)), 0)
    return maps


def large_map():
    """130 x 131: above the 16384 pixels at which the existing labellings change path"""
    h, w = 130, 131
    m = np.zeros((h, w), np.uint8)
    m[rotated_rect_mask(h, w, 40, 35, 30, 12, 0.3)] = 255
    m[rotated_rect_mask(h, w, 90, 90, 35, 9, 1.2)] = 1
    m[ellipse_mask(h, w, 100, 30, 20, 14, 0.4)] = 200
    m[ellipse_mask(h, w, 30, 100, 22, 18)] = 255
    m[ellipse_mask(h, w, 30, 100, 12, 9)] = 0      # a hole ...
    m[98:103, 27:34] = 1                            # ... with a component inside
    m[h - 1, 60:80] = 255
    m[64, 0] = 1
    return m


def big_ellipse_map():
    """semi-axes 110 x 88 on 240 x 200: a hull of more than 64 vertices"""
    return ellipse_mask(200, 240, 120, 100, 110, 88).astype(np.uint8) * 255
