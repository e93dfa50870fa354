"""Exact oracle of the object-level evaluation (helper module of the tests, not collected).

Areas are exact rationals (``fractions.Fraction``): the plane is cut into vertical slabs at every vertex abscissa and at the
abscissa of every crossing of two edges of the polygons involved.  Inside a slab no two boundary lines cross, so every convex
polygon is a trapezoid (or absent) and the measure of a set expression -- a union, or a union intersected with a union -- on a
vertical line is a linear function of x: its value at the slab's middle times the slab's width is the exact area.  Nothing here
clips a polygon or integrates along a boundary, which is what the device does.

The matching rule restates FtMetricsCalculator.analyze of the reference (evaluation.py:229-328, confusion matrix :330-362) in
plain Python over those exact tables; every ``>`` and ``>=`` is decided exactly.
"""
from fractions import Fraction

ADJ = Fraction(0.05)          # the double the reference compares with (iou_precision_threshold = 0.05)


def poly(coords):
    """flat x1, y1, ... (ints, floats -- taken exactly --, Fractions) -> list of (Fraction, Fraction)"""
    c = [Fraction(v) for v in coords]
    return [(c[i], c[i + 1]) for i in range(0, len(c), 2)]


def _edges(p):
    return [(p[i], p[(i + 1) % len(p)]) for i in range(len(p))]


def _cuts(polys):
    xs = set()
    edges = []
    for p in polys:
        for a, b in _edges(p):
            xs.add(a[0])
            if a != b:
                edges.append((a, b))
    for i in range(len(edges)):
        (ax, ay), (bx, by) = edges[i]
        for j in range(i + 1, len(edges)):
            (cx, cy), (dx, dy) = edges[j]
            den = (bx - ax) * (dy - cy) - (by - ay) * (dx - cx)
            if den == 0:
                continue
            t = ((cx - ax) * (dy - cy) - (cy - ay) * (dx - cx)) / den
            u = ((cx - ax) * (by - ay) - (cy - ay) * (bx - ax)) / den
            if 0 <= t <= 1 and 0 <= u <= 1:
                xs.add(ax + t * (bx - ax))
    return sorted(xs)


def _span(p, x):
    """(low, high) of the vertical line at x inside the convex polygon p, or None"""
    ys = []
    for (ax, ay), (bx, by) in _edges(p):
        if ax != bx and min(ax, bx) < x < max(ax, bx):
            ys.append(ay + (x - ax) * (by - ay) / (bx - ax))
    if len(ys) < 2:
        return None
    lo, hi = min(ys), max(ys)
    return (lo, hi) if hi > lo else None


def _merge(spans):
    out = []
    for lo, hi in sorted(spans):
        if out and lo <= out[-1][1]:
            if hi > out[-1][1]:
                out[-1][1] = hi
        else:
            out.append([lo, hi])
    return out


def _measure(a, b=None):
    """length of the merged span list a, or of its intersection with the merged span list b"""
    if b is None:
        return sum((hi - lo for lo, hi in a), Fraction(0))
    tot = Fraction(0)
    for lo, hi in a:
        for lo2, hi2 in b:
            l, h = max(lo, lo2), min(hi, hi2)
            if h > l:
                tot += h - l
    return tot


def area_sets(group_a, group_b=None):
    """area of the union of group_a, or (group_b given) of union(group_a) intersected with union(group_b)"""
    polys = list(group_a) + (list(group_b) if group_b is not None else [])
    if not polys or (group_b is not None and (not group_a or not group_b)):
        return Fraction(0)
    xs = _cuts(polys)
    tot = Fraction(0)
    for x0, x1 in zip(xs, xs[1:]):
        xm = (x0 + x1) / 2
        sa = _merge([s for s in (_span(p, xm) for p in group_a) if s])
        if group_b is None:
            tot += _measure(sa) * (x1 - x0)
        else:
            sb = _merge([s for s in (_span(p, xm) for p in group_b) if s])
            tot += _measure(sa, sb) * (x1 - x0)
    return tot


def area(p):
    return area_sets([p])


def intersection(p, q):
    return area_sets([p], [q])


def iou_of(a1, a2, inter):
    u = a1 + a2 - inter
    return inter / u if u > 0 else Fraction(0)


def is_convex(p):
    """strictly positive area, no turn against the winding, and the turns sum to one revolution (no self-intersection)"""
    n = len(p)
    if n < 3:
        return False
    sign = 0
    for i in range(n):
        (ax, ay), (bx, by), (cx, cy) = p[i], p[(i + 1) % n], p[(i + 2) % n]
        cr = (bx - ax) * (cy - by) - (by - ay) * (cx - bx)
        if cr != 0:
            s = 1 if cr > 0 else -1
            if sign and s != sign:
                return False
            sign = s
    return sign != 0


class Tables:
    """what FtMetricsCalculator.__init__ builds (evaluation.py:210-227), exactly"""

    def __init__(self, gts, founds):
        self.gts, self.founds = gts, founds
        self.area_g = [area(p) for p in gts]
        self.area_f = [area(p) for p in founds]
        self.inter = [[intersection(g, f) for f in founds] for g in gts]
        self.iou = [[iou_of(self.area_g[i], self.area_f[j], self.inter[i][j]) for j in range(len(founds))] for i in range(len(gts))]
        G, F = len(gts), len(founds)
        self.gt_to_found = [[j for j in range(F) if self.iou[i][j] > ADJ] for i in range(G)]
        self.found_to_gt = [[i for i in range(G) if self.iou[i][j] > ADJ] for j in range(F)]
        self.one_to_ones, self.one_to_manys, self.many_to_ones = [], [], []
        for g, idx in enumerate(self.gt_to_found):
            if len(idx) == 1:
                if len(self.found_to_gt[idx[0]]) == 1:
                    self.one_to_ones.append((g, idx[0], self.iou[g][idx[0]]))
            elif len(idx) > 1 and all(len(self.found_to_gt[j]) == 1 for j in idx):
                grp = [founds[j] for j in idx]
                a_grp = area_sets(grp)
                self.one_to_manys.append((g, idx, iou_of(a_grp, self.area_g[g], area_sets(grp, [gts[g]]))))
        for f, idx in enumerate(self.found_to_gt):
            if len(idx) > 1 and all(len(self.gt_to_found[i]) == 1 for i in idx):
                grp = [gts[i] for i in idx]
                a_grp = area_sets(grp)
                self.many_to_ones.append((idx, f, iou_of(a_grp, self.area_f[f], area_sets(grp, [founds[f]]))))
        a_g, a_f = area_sets(gts), area_sets(founds)
        it = area_sets(gts, founds)
        self.precision_by_area = it / a_f if a_f > 0 else Fraction(0)
        self.recall_by_area = it / a_g if a_g > 0 else Fraction(0)
        self.iou_by_area = iou_of(a_g, a_f, it)
        # a ground truth touched by several found quads of which one also touches another ground truth: neither kind of group
        self.broken_one_to_many = sum(1 for idx in self.gt_to_found
                                      if len(idx) > 1 and not all(len(self.found_to_gt[j]) == 1 for j in idx))

    def decision_values(self):
        """every exact value that is compared with 0.05 or with a threshold"""
        v = [x for row in self.iou for x in row]
        v += [m[2] for m in self.one_to_manys] + [m[2] for m in self.many_to_ones] + [self.iou_by_area]
        return v

    def analyze(self, thr, gt_cls=None, found_cls=None, n_classes=0):
        """FtMetricsCalculator.analyze(thr) as a dict of exact values; thr: the double of the caller, taken exactly"""
        thr = Fraction(thr)
        C = n_classes if (gt_cls is not None and found_cls is not None) else 0
        cm = [[Fraction(0)] * C for _ in range(C)]
        o2o = [(g, f, v) for g, f, v in self.one_to_ones if v >= thr]
        matched_gt = matched_found = boxes = len(o2o)
        iou_sum = sum((v for _, _, v in o2o), Fraction(0))
        for g, f, _ in o2o:
            if C:
                cm[gt_cls[g]][found_cls[f]] += 1
        o2m = m2o = 0
        for g, idx, v in self.one_to_manys:
            if v >= thr:
                matched_gt += 1; o2m += 1; matched_found += len(idx); boxes += 1; iou_sum += v
                if C:
                    tot = sum((self.inter[g][j] for j in idx), Fraction(0))
                    for j in idx:
                        cm[gt_cls[g]][found_cls[j]] += self.inter[g][j] / tot
        for idx, f, v in self.many_to_ones:
            if v >= thr:
                matched_gt += len(idx); m2o += len(idx); matched_found += 1; boxes += 1; iou_sum += v
                if C:
                    for i in idx:
                        cm[gt_cls[i]][found_cls[f]] += 1
        return dict(tp=matched_gt, fp=len(self.founds) - matched_found, fn=len(self.gts) - matched_gt, one_to_one=len(o2o),
                    one_to_many=o2m, many_to_one=m2o, matched_boxes_count=boxes, iou_sum=iou_sum,
                    detection_rate=1 if self.iou_by_area > thr else 0, precision_by_area=self.precision_by_area,
                    recall_by_area=self.recall_by_area, iou_by_area=self.iou_by_area, confusion=cm)


def rescale_quad(q, xscale, yscale):
    """utils.py:67-69: int(coordinate * scale) in double arithmetic"""
    return [int(v * (xscale if k % 2 == 0 else yscale)) for k, v in enumerate(q)]
