"""Numpy restatements of the object scores, the greedy ranking and the average precision (no reference counterpart: the
definitions are the project's, include/ubd.h).  Sequential, one object / detection / cut at a time."""
import numpy as np

from oracle import label_raster

Q = 16777216.0                                   # 2^24: the quantisation step of a probability


def region_mask(quad, scale, map_h, map_w):
    """the map pixels build_label_map paints for one quad: proper_round(quad / scale), Pillow's polygon rule, clipped to the map"""
    m = np.zeros((map_h, map_w), np.int32)
    label_raster.fill_polygon(m, label_raster.proper_round(quad, scale), 1)
    return m > 0


def score_objects(det_logits, quads, counts, scale):
    """det_logits (n, h, w) float32, quads (n, cap, 8), counts (n) -> float32 (n, cap): fp64 sigmoid, rint(p * 2^24) as integers
    (NaN counts as 0), the integer sum over the region, (float32)(sum / (2^24 * count)); 0 for an empty region and behind the list"""
    n, cap = quads.shape[:2]
    h, w = det_logits.shape[1:]
    with np.errstate(over="ignore", invalid="ignore"):
        p = 1.0 / (1.0 + np.exp(-det_logits.astype(np.float64)))
    q = np.where(np.isnan(p), 0.0, np.rint(p * Q)).astype(np.int64)
    out = np.zeros((n, cap), np.float32)
    for i in range(n):
        for o in range(min(int(counts[i]), cap)):
            m = region_mask(quads[i, o], scale, h, w)
            count = int(m.sum())
            if count:
                out[i, o] = np.float32(float(int(q[i][m].sum())) / (Q * float(count)))
    return out


def rank_order(scores):
    """indices in descending score, ties to the lower index, NaN last"""
    idx = list(range(len(scores)))
    return sorted(idx, key=lambda k: (1, 0.0, k) if np.isnan(scores[k]) else (0, -float(scores[k]), k))


def rank_image(scores, iou, n_gt, thresholds):
    """One image: scores (count) float32, iou (rows >= n_gt, cap) float64.  Returns [(score, tp_mask)] in ranked order: per
    threshold a detection takes the not-yet-taken ground truth of the largest IoU (lowest g of equals, NaN never); IoU >= t makes
    it a true positive and takes the ground truth."""
    order = rank_order(scores)
    masks = [0] * len(order)
    columns = {f: [float(v) for v in np.asarray(iou)[:n_gt, f]] for f in order}
    for j, t in enumerate(thresholds):
        taken = [False] * n_gt
        for r, f in enumerate(order):
            best, best_g = None, -1
            for g, v in enumerate(columns[f]):
                if taken[g] or v != v:
                    continue
                if best_g < 0 or v > best:
                    best, best_g = v, g
            if best_g >= 0 and best >= t:
                taken[best_g] = True
                masks[r] |= 1 << j
    return [(scores[f], masks[r]) for r, f in enumerate(order)]


class RankBuffer:
    """the epoch buffer of ubd_rank_detections as a host object: header counters and the record bytes"""

    def __init__(self, capacity):
        self.capacity = capacity
        self.head = np.zeros(8, np.int64)
        self.scores, self.masks = [], []

    def add(self, scores, counts, cap, iou_tables, gt_counts, thresholds, max_gt=256):
        """scores (n, cap), counts (n), iou_tables: per image (rows, cap), gt_counts (n)"""
        for i in range(len(counts)):
            if counts[i] > cap or gt_counts[i] > max_gt:
                self.head[4] += 1
                continue
            self.head[2] += max(int(gt_counts[i]), 0)
            self.head[3] += 1
            for s, m in rank_image(scores[i, :max(int(counts[i]), 0)], iou_tables[i], max(int(gt_counts[i]), 0), thresholds):
                if self.head[0] < self.capacity:
                    self.scores.append(s); self.masks.append(m)
                    self.head[0] += 1
                else:
                    self.head[1] += 1

    def tobytes(self):
        rec = np.zeros(self.capacity, np.dtype([("score", np.float32), ("tp_mask", np.uint32)]))
        rec["score"][:len(self.scores)] = np.asarray(self.scores, np.float32)
        rec["tp_mask"][:len(self.masks)] = np.asarray(self.masks, np.uint32)
        return self.head.tobytes() + rec.tobytes()


def average_precision_brute(scores, tp_flags, n_gt):
    """AP by recomputing precision and recall at every cut of the ranked list from scratch"""
    s = [float(v) for v in scores]
    order = sorted(range(len(s)), key=lambda k: (1, 0.0, k) if np.isnan(s[k]) else (0, -s[k], k))
    flags = [bool(tp_flags[k]) for k in order]
    prec, rec = [], []
    for k in range(1, len(flags) + 1):
        tp = sum(1 for f in flags[:k] if f)
        prec.append(tp / k)
        rec.append(tp / n_gt)
    ap, prev = 0.0, 0.0
    for k in range(len(flags)):
        ap += (rec[k] - prev) * max(prec[k:])
        prev = rec[k]
    return ap
