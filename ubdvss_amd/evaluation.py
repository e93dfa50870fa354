"""Object-level evaluation -- host mirror of semantic_segmentation/evaluation.py (FtMetrics :22-165, FtMetricsCalculator
:168-429, DatasetMetricCalculator :432-544).

The reference builds shapely polygons image by image on the host.  Here the areas, the IoU tables, the 1-1 / 1-many / many-1
matching, the group and by-area unions and the counters at every IoU threshold are computed on the MI355X by
``ubd_evaluate_objects`` (include/ubd.h) from the object lists ``ubd_postprocess`` left in device memory, and summed into a
device accumulator: a validation epoch is any number of ``evaluate_batch`` calls and ONE small read in ``get_metrics``.
The pixel classification accuracies of ``_calc_pixel_classification_correctness_mask`` (:546-575) come from
``ubd_evaluate_pixels`` in the same way: the class logits of the forward pass and the label maps stay on the device, the
sums go to a second small accumulator and the correctness mask comes back as a device tensor.
Beyond the reference (it has no counterpart): with ``average_precision=True`` every batch is also ranked by
``ubd_rank_detections`` -- COCO's greedy matching of the detections in descending score (``Model.score_objects_on_device``) at every
threshold, not the reference's 1-1 / 1-many / many-1 analysis -- into a device record buffer, and ``average_precision`` forms
``ap_iou*`` and ``map`` from the one read of that buffer.
There is no CPU path: without a GPU the entry points raise ``RuntimeError``.

``ImageResultCategories`` (:579-628) sorts an image's result into the folders the result saver writes; the overlays themselves
are ``ubdvss_amd.visualizations``.  Ground truth of up to 8 vertices goes through ``ubd_evaluate_objects``; as soon as a
polygon of a call has more (hulls read from segmentation maps, ``ubdvss_amd.markup_readers``: up to 64) the call goes through
``ubd_evaluate_polygons``, which gives the same bits on common ground.  Not here: non-convex outlines as such.
"""
import ctypes
import functools
import math

import numpy as np

from . import _lib

IOU_PRECISION_THRESHOLD = 0.05
_REC_BYTES = ctypes.sizeof(_lib.UbdEvalRecord)
_REC_DTYPE = np.dtype([(k, np.int32) for k in ("tp", "fp", "fn", "one_to_one", "one_to_many", "many_to_one",
                                               "matched_boxes_count", "detection_rate", "n_gt", "n_found", "flags", "reserved")] +
                      [(k, np.float64) for k in ("iou_sum", "precision_by_area", "recall_by_area", "iou_by_area")])
assert _REC_DTYPE.itemsize == _REC_BYTES == 80


def _ratio(numerator, denominator):
    """numerator / denominator, and 0 where there is nothing to divide by (the reference's convention for every quotient)"""
    return numerator / denominator if denominator > 0 else 0


def detection_scores(tp, fp, fn):
    """(precision, recall, F1) of object counts; F1 is the harmonic mean of the two quotients as they were rounded"""
    precision, recall = _ratio(tp, tp + fp), _ratio(tp, tp + fn)
    return precision, recall, _ratio(2 * precision * recall, precision + recall)


def _pooled_mean(mean_a, n_a, mean_b, n_b):
    """mean of the union of two samples known by (mean, size)"""
    return _ratio(mean_a * n_a + mean_b * n_b, n_a + n_b)


_OBJECT_COUNTERS = ("tp", "fp", "fn", "one_to_one", "one_to_many", "many_to_one")
_IMAGE_MEANS = ("average_iou_by_area", "average_precision_by_area", "average_recall_by_area", "detection_rate")
_ACC_EPS = 1e-5               # added to a class's row sum in get_types_acc (evaluation.py:147), so a class never seen scores 0


class FtMetrics:
    """The public record of evaluation.py:22-165: object counters, the mean IoU over ``matched_boxes_count`` matches, the by-area
    means and the detection rate over ``matched_images_count`` images, and the confusion matrix [actual, predicted] when
    classification is scored.  One image at one IoU threshold, or (after ``append``) a data set."""

    def __init__(self, all_type_names=None, compute_classification_metrics=False):
        for name in _OBJECT_COUNTERS + _IMAGE_MEANS + ("average_iou", "matched_boxes_count", "matched_images_count"):
            setattr(self, name, 0)
        self.all_type_names = all_type_names
        self.confusion_matrix = None
        if compute_classification_metrics and all_type_names is not None:
            self.confusion_matrix = np.zeros((len(all_type_names),) * 2, dtype=np.float64)   # fp64 like the device sums (reference: float32)

    def append(self, other):
        """Pools ``other`` into this record: counters add, means are re-weighted by the number of matches / images behind them."""
        for name in _OBJECT_COUNTERS:
            setattr(self, name, getattr(self, name) + getattr(other, name))
        self.average_iou = _pooled_mean(self.average_iou, self.matched_boxes_count, other.average_iou, other.matched_boxes_count)
        self.matched_boxes_count += other.matched_boxes_count
        for name in _IMAGE_MEANS:
            setattr(self, name, _pooled_mean(getattr(self, name), self.matched_images_count, getattr(other, name), other.matched_images_count))
        self.matched_images_count += other.matched_images_count
        if self.confusion_matrix is not None:
            self.confusion_matrix += other.confusion_matrix

    def get_metrics(self):
        return detection_scores(self.tp, self.fp, self.fn)

    def get_report(self):
        """the reference's report line (evaluation.py:108-110), character for character"""
        template = ('pr = {:.4f}, r = {:.4f}, f1 = {:.4f} '
                    '[tp = {} = {} (1-1) + {} (1-m) + {} (m-1); fp = {}; fn = {}];'
                    ' iou boxes = {:.2f}  >>> by area: pr = {:.4f}, r = {:.4f}, iou = {:.4f}, rate = {:.4f}')
        return template.format(*self.get_metrics(), self.tp, self.one_to_one, self.one_to_many, self.many_to_one, self.fp, self.fn,
                               self.average_iou, self.average_precision_by_area, self.average_recall_by_area,
                               self.average_iou_by_area, self.detection_rate)

    def _confusion(self):
        if self.confusion_matrix is None or self.all_type_names is None:
            raise AssertionError("confusion matrix undefined in report")
        return np.asarray(self.confusion_matrix, dtype=np.float64)

    def get_confusion_matrix_report(self):
        """Plain text (the reference prints pandas frames): accuracy per actual class, the average, the matrix predicted \\ actual."""
        cm = self._confusion()
        acc = np.diag(cm) / np.maximum(cm.sum(axis=1), 1)
        names = [str(n) for n in self.all_type_names]
        wide = max([len(n) for n in names] + [8])
        lines = ["{:<{w}}  Accuracy".format("", w=wide)]
        lines += ["{:<{w}}  {:.3f}".format(n, a, w=wide) for n, a in zip(names, acc)]
        lines.append("Average accuracy: {:.3f}".format(self.get_average_acc()))
        lines.append("")
        lines.append("Confusion matrix (predicted \\ actual):")
        table = cm.T.astype(int)
        col = max([wide] + [len(str(v)) for v in table.ravel()])
        lines.append("{:<{w}}  ".format("", w=wide) + "  ".join("{:>{c}}".format(n, c=col) for n in names))
        for n, row in zip(names, table):
            lines.append("{:<{w}}  ".format(n, w=wide) + "  ".join("{:>{c}}".format(v, c=col) for v in row))
        return "\n".join(lines)

    def get_types_acc(self):
        """{type name: share of the objects of that actual type whose predicted type is the same}"""
        cm = self._confusion()
        seen = cm.sum(axis=1)
        return {name: cm[k, k] / (seen[k] + _ACC_EPS) for k, name in enumerate(self.all_type_names)}

    def get_average_acc(self):
        cm = self._confusion()
        return np.trace(cm) / max(cm.sum(), 1)


# ---- host-side validation and packing ---------------------------------------------------------------------------------------------
def _is_convex(p):
    """(k, 2) vertices: every vertex on the inner side of (or on) every edge, for either winding.  Rules out reflex corners and
    self-intersecting (bow-tie, star) outlines; collinear and repeated vertices and zero-area slivers pass."""
    q = np.roll(p, -1, axis=0)
    e = q - p
    signed = 0.5 * float(np.sum(p[:, 0] * q[:, 1] - p[:, 1] * q[:, 0]))
    s = 1.0 if signed >= 0 else -1.0
    d = p[None, :, :] - p[:, None, :]
    side = s * (e[:, None, 0] * d[:, :, 1] - e[:, None, 1] * d[:, :, 0])
    span = float(np.abs(d).max())
    return not (side < -1e-9 * max(span * span, 1e-300)).any()


def _check_class_ids(ids, n_classes, where):
    for c in ids:
        if not 0 <= int(c) < n_classes:
            raise ValueError(f"{where}: object type id {int(c)} is outside 0..{n_classes - 1}")


def check_ground_truth_polygon(coords, image_idx=0, object_idx=0, max_vertices=_lib.UBD_EVAL_MAX_VERTS):
    """A ground-truth polygon the device accepts: 3..max_vertices vertices (8 for ubd_evaluate_objects, up to 64 for
    ubd_evaluate_polygons), finite, convex (either winding; collinear vertices allowed).
    Returns the (k, 2) float64 vertices; raises ValueError naming the image and the object otherwise."""
    where = f"ground truth of image {image_idx}, object {object_idx}"
    p = np.asarray(coords, dtype=np.float64).reshape(-1)
    if p.size % 2 or p.size < 6:
        raise ValueError(f"{where}: a polygon needs at least 3 vertices (x, y pairs), got {p.size} numbers")
    p = p.reshape(-1, 2)
    if len(p) > max_vertices:
        raise ValueError(f"{where}: {len(p)} vertices, the limit is {max_vertices}")
    if not np.isfinite(p).all():
        raise ValueError(f"{where}: coordinates are not finite")
    if not _is_convex(p):
        raise ValueError(f"{where}: the polygon is not convex (non-convex or self-intersecting outlines are not supported)")
    return p


_require_gpu = functools.partial(_lib.require_gpu, "ubdvss_amd.evaluation")      # a name of its own: a host test replaces it


def pack_ground_truth(gt_polygons, gt_classes=None, image_offset=0, n_classes=None):
    """gt_polygons: per image a list of flat coordinate lists.  Returns host arrays (xy float64 (V, 2), first int32 (P + 1),
    cls int32 (P) or None, image_first int32 (n + 1), max_gt).  Raises ValueError for an image without ground truth
    (evaluation.py:482), too many polygons in one image, a polygon the device does not accept (more than 64 vertices, not
    convex, ...), or (n_classes given) a class id outside 0..n_classes-1.  Which entry point takes the call follows from the
    data: ``np.diff(first).max()`` is the most vertices a polygon has."""
    xy, first, cls, image_first = [], [0], [], [0]
    max_gt = 1
    for i, polys in enumerate(gt_polygons):
        if len(polys) == 0:
            raise ValueError(f"empty gt bboxes in image {image_offset + i} (it should contain at least one bbox)")
        if len(polys) > _lib.UBD_EVAL_MAX_GT:
            raise ValueError(f"image {image_offset + i} has {len(polys)} ground-truth objects, the limit is {_lib.UBD_EVAL_MAX_GT}")
        max_gt = max(max_gt, len(polys))
        for o, c in enumerate(polys):
            p = check_ground_truth_polygon(c, image_offset + i, o, _lib.UBD_POLY_MAX_VERTS)
            xy.append(p)
            first.append(first[-1] + len(p))
        if gt_classes is not None:
            if len(gt_classes[i]) != len(polys):
                raise ValueError(f"image {image_offset + i}: {len(polys)} ground-truth boxes but {len(gt_classes[i])} types")
            if n_classes is not None:
                _check_class_ids(gt_classes[i], n_classes, f"ground truth of image {image_offset + i}")
            cls.extend(int(c) for c in gt_classes[i])
        image_first.append(image_first[-1] + len(polys))
    return (np.ascontiguousarray(np.concatenate(xy, axis=0)), np.asarray(first, dtype=np.int32),
            np.asarray(cls, dtype=np.int32) if gt_classes is not None else None, np.asarray(image_first, dtype=np.int32), max_gt)


def accumulator_bytes(n_thresholds, n_classes):
    return int(_lib.load().ubd_evaluate_accumulator_bytes(int(n_thresholds), int(n_classes)))


def evaluate_objects(quads, classes, counts, gt_polygons, gt_classes, thresholds, n_classes, accumulator, scales=None,
                     per_image=True, return_tables=False, max_gt=None, image_offset=0):
    """One ubd_evaluate_objects call on the current stream.  quads (n, cap, 8) int32, classes (n, cap) int32 or None,
    counts (n) int32: device tensors (the outputs of ubd_postprocess).  gt_polygons / gt_classes: host lists per image.
    scales: None, or (n, 2) xscale, yscale (host or device).  accumulator: device uint8 tensor of accumulator_bytes().
    Returns the (n, T) records as a device uint8 tensor (n, T, 80) (None with per_image=False); with return_tables also
    (workspace, offset_bytes, stride_doubles, max_gt) of the diagnostics tables.  Nothing is copied to the host, so the device
    tensors are taken as ubd_postprocess makes them: convex quads (minAreaRect boxes) and class ids 0..n_classes-1 (an argmax
    over the class channels).  Tensors from elsewhere must keep to that: the device clips against convex outlines only and leaves
    a pair with a class id outside the range out of the confusion matrix.  Host lists are checked (ValueError)."""
    torch = _require_gpu()
    lib = _lib.load()
    dev = quads.device
    n, cap = int(quads.shape[0]), int(quads.shape[1])
    if len(gt_polygons) != n:
        raise ValueError(f"{len(gt_polygons)} ground-truth lists for {n} images")
    C = int(n_classes)
    xy, first, cls, image_first, mg = pack_ground_truth(gt_polygons, gt_classes if C > 0 else None, image_offset, C if C > 0 else None)
    max_gt = mg if max_gt is None else max(int(max_gt), mg)
    thr = np.ascontiguousarray(np.asarray(thresholds, dtype=np.float64))
    T = len(thr)
    xy_d = torch.from_numpy(xy).to(dev)
    first_d = torch.from_numpy(first).to(dev)
    cls_d = torch.from_numpy(cls).to(dev) if cls is not None else None
    if scales is not None and not hasattr(scales, "data_ptr"):
        scales = torch.from_numpy(np.ascontiguousarray(np.asarray(scales, dtype=np.float64).reshape(n, 2))).to(dev)
    # by data: ground truth of at most 8 vertices takes ubd_evaluate_objects as ever, anything larger ubd_evaluate_polygons
    most_verts = int(np.diff(first).max())
    polygons = most_verts > _lib.UBD_EVAL_MAX_VERTS
    need = int(lib.ubd_evaluate_polygons_workspace_bytes(n, max_gt, cap, T, C, most_verts) if polygons
               else lib.ubd_evaluate_workspace_bytes(n, max_gt, cap, T, C))
    if need == 0:
        raise ValueError(f"evaluation sizes outside the limits: n={n} max_gt={max_gt} cap={cap} thresholds={T} classes={C} "
                         f"(cap <= {_lib.UBD_EVAL_MAX_FOUND}, thresholds <= {_lib.UBD_EVAL_MAX_THRESHOLDS})")
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    rec = torch.empty((n, T, _REC_BYTES), dtype=torch.uint8, device=dev) if per_image else None
    head = (quads.data_ptr(), classes.data_ptr() if (classes is not None and C > 0) else None, counts.data_ptr(), n, cap,
            scales.data_ptr() if scales is not None else None, xy_d.data_ptr(), int(len(xy)), first_d.data_ptr(),
            cls_d.data_ptr() if cls_d is not None else None, image_first.ctypes.data, max_gt, thr.ctypes.data, T, C)
    tail = (rec.data_ptr() if rec is not None else None, accumulator.data_ptr(), ws.data_ptr(), need)
    if polygons:
        _lib.launch("ubd_evaluate_polygons", dev, *head, most_verts, *tail)
    else:
        _lib.launch("ubd_evaluate_objects", dev, *head, *tail)
    # the inputs and the workspace were allocated on this stream: the caching allocator reuses them in stream order
    if return_tables:
        off, stride = ctypes.c_int64(), ctypes.c_int64()
        if polygons:
            _lib.call("ubd_evaluate_polygons_tables_layout", n, max_gt, cap, T, C, most_verts, ctypes.byref(off), ctypes.byref(stride))
        else:
            _lib.call("ubd_evaluate_tables_layout", n, max_gt, cap, T, C, ctypes.byref(off), ctypes.byref(stride))
        return rec, (ws, off.value, stride.value, max_gt)
    return rec


# ---- pixel classification accuracy (ubd_evaluate_pixels) ----------------------------------------------------------------------------
_PIX_REC_BYTES = ctypes.sizeof(_lib.UbdPixelRecord)
_PIX_REC_DTYPE = np.dtype([("n_correct", np.int64), ("n_total", np.int64), ("n_objects", np.int64), ("object_acc_sum", np.float64)])
assert _PIX_REC_DTYPE.itemsize == _PIX_REC_BYTES == 32


def pixel_accumulator_bytes():
    return int(_lib.load().ubd_evaluate_pixels_accumulator_bytes())


def unpack_pixel_accumulator(acc_host):
    """host bytes of a pixel accumulator -> dict(n_correct, n_total, n_objects, object_acc_sum, images)"""
    raw = np.ascontiguousarray(acc_host).view(np.uint8).reshape(-1)
    i64, f64 = raw.view(np.int64), raw.view(np.float64)
    return dict(n_correct=int(i64[0]), n_total=int(i64[1]), n_objects=int(i64[2]), object_acc_sum=float(f64[3]), images=int(i64[4]))


def pixel_logs_from_sums(n_correct, n_total, n_objects, object_acc_sum):
    """The two pixel entries of the reference's ``scalar_logs`` (evaluation.py:526-530) from the sums of an epoch.  A zero
    denominator gives nan, as the reference's numpy division (0 / 0) and its mean of an empty list do."""
    nan = float("nan")
    return {"classification_pixel_acc_total": n_correct / n_total if n_total > 0 else nan,
            "classification_pixel_acc_object": object_acc_sum / n_objects if n_objects > 0 else nan}


def _pixel_stride(t):
    """(N, h, w, C) float32 tensor -> floats between consecutive pixels when the view is one regular pixel grid (the class
    slice of the net's contiguous output is), else None"""
    n, h, w, c = (int(v) for v in t.shape)
    if c > 1 and t.stride(3) != 1:
        return None
    units = ((w, t.stride(2), 1), (h, t.stride(1), w), (n, t.stride(0), h * w))
    ps = None
    for size, stride, pixels in units:
        if size > 1:
            if stride % pixels:
                return None
            if ps is None:
                ps = stride // pixels
            if stride != ps * pixels:
                return None
    if ps is None:
        ps = c
    return ps if ps >= c else None


def evaluate_pixels(class_logits, labels, accumulator, want_mask=False, n_classes=None, per_image=True):
    """One ubd_evaluate_pixels call on the current stream.  class_logits: float32 device tensor, either the net's full output
    (N, h, w, n_classes + 1) or a class slice (N, h, w, n_classes); with n_classes given the two are told apart by the last
    dimension, without it the tensor is a class slice.  A full tensor (and any view that is a regular pixel grid) is passed as
    it lies, without a copy.  labels: (N, h, w) or (N, h, w, 1), int32 device tensor or numpy array (the y_true of the loss).
    accumulator: device uint8 tensor of pixel_accumulator_bytes(), zeroed before the first call.  Returns (records, mask):
    the per-image records as a device uint8 tensor (N, 32) (None with per_image=False) and the correctness mask, an int8
    device tensor (N, h, w) of -1 / 0 / 1 (None unless want_mask)."""
    torch = _require_gpu()
    lib = _lib.load()
    if not torch.is_tensor(class_logits):
        class_logits = torch.from_numpy(np.ascontiguousarray(np.asarray(class_logits, dtype=np.float32))).to(accumulator.device)
    if class_logits.dim() != 4 or class_logits.dtype != torch.float32:
        raise ValueError(f"class logits must be a float32 (N, h, w, C) tensor, got {tuple(class_logits.shape)} {class_logits.dtype}")
    dev = class_logits.device
    last = int(class_logits.shape[3])
    if n_classes is None:
        C = last
    else:
        C = int(n_classes)
        if last == C + 1:
            class_logits = class_logits[..., 1:]
        elif last != C:
            raise ValueError(f"class logits have {last} channels: expected {C} (a class slice) or {C + 1} (the net's output)")
    n, h, w = (int(v) for v in class_logits.shape[:3])
    stride = _pixel_stride(class_logits)
    if stride is None:
        class_logits = class_logits.contiguous()
        stride = C
    if not torch.is_tensor(labels):
        labels = torch.from_numpy(np.ascontiguousarray(np.asarray(labels).astype(np.int32, copy=False)))
    if labels.dim() == 4 and labels.shape[3] == 1:
        labels = labels[..., 0]
    if tuple(labels.shape) != (n, h, w):
        raise ValueError(f"labels {tuple(labels.shape)} do not match the logits' maps {(n, h, w)}")
    if labels.dtype != torch.int32:
        raise ValueError(f"labels must be int32, got {labels.dtype}")
    labels = labels.to(dev).contiguous()
    need = int(lib.ubd_evaluate_pixels_workspace_bytes(n, h, w)) if 1 <= C <= _lib.UBD_MAX_CLASSES else 0
    if need == 0:
        raise ValueError(f"pixel evaluation sizes outside the limits: n={n} h={h} w={w} classes={C} "
                         f"(n >= 1, sides 1..32767, classes 1..{_lib.UBD_MAX_CLASSES})")
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    rec = torch.empty((n, _PIX_REC_BYTES), dtype=torch.uint8, device=dev) if per_image else None
    mask = torch.empty((n, h, w), dtype=torch.int8, device=dev) if want_mask else None
    _lib.launch("ubd_evaluate_pixels", dev, class_logits.data_ptr(), int(stride), C, labels.data_ptr(), n, h, w,
                mask.data_ptr() if mask is not None else None, rec.data_ptr() if rec is not None else None,
                accumulator.data_ptr(), ws.data_ptr(), need)
    # the inputs and the workspace were allocated on this stream: the caching allocator reuses them in stream order
    return rec, mask


def pixel_records_to_numpy(records):
    """device (n, 32) uint8 pixel records -> host structured array (n) (synchronises)"""
    h = records.cpu().numpy()
    return h.reshape(-1).view(_PIX_REC_DTYPE)


def records_to_numpy(records):
    """device (n, T, 80) uint8 records -> host structured array (n, T) (synchronises)"""
    h = records.cpu().numpy()
    return h.reshape(h.shape[0], h.shape[1] * _REC_BYTES).view(_REC_DTYPE).reshape(h.shape[0], h.shape[1])


def tables_to_numpy(tables, n, cap):
    """the diagnostics of evaluate_objects(return_tables=True) -> list per image of (area_gt [max_gt], area_found [cap],
    inter [max_gt, cap], iou [max_gt, cap]) host arrays (synchronises)"""
    ws, off, stride, max_gt = tables
    flat = ws[off:off + n * stride * 8].cpu().numpy().view(np.float64).reshape(n, stride)
    out = []
    for i in range(n):
        r = flat[i]
        o = max_gt + cap
        out.append((r[:max_gt], r[max_gt:o], r[o:o + max_gt * cap].reshape(max_gt, cap),
                    r[o + max_gt * cap:o + 2 * max_gt * cap].reshape(max_gt, cap)))
    return out


def unpack_accumulator(acc_host, n_thresholds, n_classes):
    """host bytes of an accumulator -> dict(images, flagged, sums_by_area (3), counters int64 (T, 8), iou_sum (T), confusion (T, C, C))"""
    T, C = int(n_thresholds), int(n_classes)
    raw = np.ascontiguousarray(acc_host).view(np.uint8).reshape(-1)
    i64, f64 = raw.view(np.int64), raw.view(np.float64)
    per = i64[8:8 + 10 * T].reshape(T, 10)
    return dict(images=int(i64[0]), flagged=int(i64[1]), sums_by_area=f64[2:5].copy(), counters=per[:, :8].copy(),
                iou_sum=f64[8:8 + 10 * T].reshape(T, 10)[:, 8].copy(),
                confusion=f64[8 + 10 * T:8 + 10 * T + T * C * C].reshape(T, C, C).copy())


# ---- ranked detections and average precision (ubd_rank_detections; no reference counterpart) -----------------------------------------
_RANK_HEADER_BYTES = 64
_RANK_DTYPE = np.dtype([("score", np.float32), ("tp_mask", np.uint32)])
assert _RANK_DTYPE.itemsize == 8


def rank_buffer_bytes(capacity):
    """bytes of an epoch's rank buffer for ``capacity`` records (0 for capacity < 1); the caller zeroes it once"""
    return int(_lib.load().ubd_rank_buffer_bytes(int(capacity)))


def rank_detections(scores, counts, gt_polygons, tables, thresholds, rank_buffer):
    """One ubd_rank_detections call on the current stream, behind the ``evaluate_objects(..., return_tables=True)`` call whose
    second result is ``tables``: COCO's greedy matching of every image's detections, in descending score, against its ground truth
    at every threshold at once, appended to ``rank_buffer`` (device uint8 tensor of rank_buffer_bytes(capacity), zeroed once per
    epoch).  scores (n, cap) float32 and counts (n) int32: device tensors (``Model.score_objects_on_device`` and the postprocess);
    gt_polygons: the per-image lists the evaluate call was given (only their lengths are used), or the lengths themselves.
    The rule is not the reference's 1-1 / 1-many / many-1 analysis.  Nothing is copied to the host."""
    torch = _require_gpu()
    ws, off, stride, max_gt = tables
    n, cap = int(scores.shape[0]), int(scores.shape[1])
    if scores.dtype != torch.float32 or counts.dtype != torch.int32 or int(counts.numel()) != n:
        raise ValueError(f"scores must be float32 (n, cap) and counts int32 (n), got {tuple(scores.shape)} {scores.dtype}, "
                         f"{tuple(counts.shape)} {counts.dtype}")
    if len(gt_polygons) != n:
        raise ValueError(f"{len(gt_polygons)} ground-truth lists for {n} images")
    gt_counts = np.asarray([g if isinstance(g, (int, np.integer)) else len(g) for g in gt_polygons], dtype=np.int32)
    if gt_counts.max(initial=0) > max_gt:
        raise ValueError(f"an image has {int(gt_counts.max())} ground-truth objects, the tables hold {max_gt}")
    thr = np.ascontiguousarray(np.asarray(thresholds, dtype=np.float64))
    capacity = (int(rank_buffer.numel()) - _RANK_HEADER_BYTES) // _RANK_DTYPE.itemsize
    dev = scores.device
    gt_d = torch.from_numpy(gt_counts).to(dev)
    scores, counts = scores.contiguous(), counts.contiguous()
    iou_ptr = ws.data_ptr() + int(off) + (max_gt + cap + max_gt * cap) * 8          # the IoU table follows the areas and the intersections
    _lib.launch("ubd_rank_detections", dev, scores.data_ptr(), counts.data_ptr(), n, cap, iou_ptr, int(stride), gt_d.data_ptr(),
                thr.ctypes.data, len(thr), rank_buffer.data_ptr(), capacity)
    # gt_d was allocated on this stream: the caching allocator reuses it in stream order


def unpack_rank_buffer(host_bytes):
    """host bytes of a rank buffer -> dict(written, dropped, n_gt, images, flagged, scores float32 (written), tp_mask uint32 (written)):
    the records in the order they were appended; bit j of tp_mask = true positive at threshold j"""
    raw = np.ascontiguousarray(host_bytes).view(np.uint8).reshape(-1)
    head = raw[:_RANK_HEADER_BYTES].view(np.int64)
    written = int(head[0])
    rec = raw[_RANK_HEADER_BYTES:_RANK_HEADER_BYTES + written * _RANK_DTYPE.itemsize].view(_RANK_DTYPE)
    return dict(written=written, dropped=int(head[1]), n_gt=int(head[2]), images=int(head[3]), flagged=int(head[4]),
                scores=rec["score"].copy(), tp_mask=rec["tp_mask"].copy())


def average_precision(scores, tp_flags, n_gt):
    """Area under the precision envelope of a ranked detection list, in fp64: stable sort by descending score (record order on
    ties, NaN last), cumulative true positives, recall = ctp / n_gt, precision = ctp / rank, precision made non-increasing from the
    right, AP = sum over the ranks of (recall_k - recall_{k-1}) * precision_k.  An empty list gives 0.  n_gt < 1: ValueError."""
    if int(n_gt) < 1:
        raise ValueError(f"average precision needs at least one ground-truth object, got {n_gt}")
    s = np.asarray(scores, dtype=np.float64).reshape(-1)
    tp = np.asarray(tp_flags).reshape(-1).astype(bool)
    if s.shape != tp.shape:
        raise ValueError(f"{s.size} scores for {tp.size} flags")
    if s.size == 0:
        return 0.0
    order = np.argsort(-s, kind="stable")
    ctp = np.cumsum(tp[order].astype(np.float64))
    recall = ctp / float(int(n_gt))
    precision = ctp / np.arange(1, s.size + 1, dtype=np.float64)
    envelope = np.maximum.accumulate(precision[::-1])[::-1]
    return float(np.sum(np.diff(recall, prepend=0.0) * envelope))


def pack_found_objects(found_boxes_per_image, found_classes_per_image=None, n_classes=0, image_offset=0):
    """host lists of integer quads -> host arrays (quads (n, cap, 8), classes (n, cap), counts (n)) int32 in the layout of the
    ubd_postprocess outputs.  ValueError for a found object that is not a convex quadrilateral with integer coordinates, or
    whose class id is outside 0..n_classes-1."""
    n = len(found_boxes_per_image)
    cap = max([1] + [len(b) for b in found_boxes_per_image])
    if cap > _lib.UBD_EVAL_MAX_FOUND:
        raise ValueError(f"{cap} found objects in one image, the limit is {_lib.UBD_EVAL_MAX_FOUND}")
    quads = np.zeros((n, cap, 8), dtype=np.int32)
    classes = np.zeros((n, cap), dtype=np.int32)
    counts = np.zeros(n, dtype=np.int32)
    for i, boxes in enumerate(found_boxes_per_image):
        counts[i] = len(boxes)
        for j, b in enumerate(boxes):
            a = np.asarray(b, dtype=np.float64).reshape(-1)
            if a.size != 8 or not np.array_equal(a, np.trunc(a)):
                raise ValueError(f"found object {j} of image {image_offset + i}: found boxes are quadrilaterals with integer coordinates")
            if not _is_convex(a.reshape(4, 2)):
                raise ValueError(f"found object {j} of image {image_offset + i}: the quadrilateral is not convex "
                                 "(non-convex or self-intersecting outlines are not supported)")
            quads[i, j] = a.astype(np.int32)
        if found_classes_per_image is not None:
            if len(found_classes_per_image[i]) != len(boxes):
                raise ValueError(f"image {image_offset + i}: {len(boxes)} found boxes but {len(found_classes_per_image[i])} types")
            _check_class_ids(found_classes_per_image[i], n_classes, f"found objects of image {image_offset + i}")
            classes[i, :len(boxes)] = np.asarray(found_classes_per_image[i], dtype=np.int32).reshape(-1)
    return quads, classes, counts


def _found_to_device(found_boxes_per_image, found_classes_per_image, device, n_classes=0, image_offset=0):
    torch = _require_gpu()
    arrays = pack_found_objects(found_boxes_per_image, found_classes_per_image, n_classes, image_offset)
    return tuple(torch.from_numpy(a).to(device) for a in arrays)


def _metrics_from_record(r, confusion, all_type_names, with_cls):
    m = FtMetrics(all_type_names=all_type_names, compute_classification_metrics=with_cls)
    for k in ("tp", "fp", "fn", "one_to_one", "one_to_many", "many_to_one", "matched_boxes_count", "detection_rate"):
        setattr(m, k, int(r[k]))
    m.average_iou = float(r["iou_sum"]) / m.matched_boxes_count if m.matched_boxes_count > 0 else 0
    m.average_precision_by_area = float(r["precision_by_area"])
    m.average_recall_by_area = float(r["recall_by_area"])
    m.average_iou_by_area = float(r["iou_by_area"])
    m.matched_images_count = 1
    if m.confusion_matrix is not None:
        m.confusion_matrix = np.array(confusion, dtype=np.float64)
    return m


class FtMetricsCalculator:
    """evaluation.py:168-328 for one image through the device call.  gt_boxes: convex polygons of 3..64 vertices (flat
    coordinate lists); found_boxes: integer quadrilaterals.  The types are names out of all_object_types."""

    def __init__(self, gt_boxes, found_boxes, gt_object_types=None, found_object_types=None, all_object_types=None,
                 compute_classification_metrics=True):
        self._with_cls = (gt_object_types is not None and found_object_types is not None and all_object_types is not None
                          and compute_classification_metrics)
        self._all_types = all_object_types
        self._gt = [list(np.asarray(b, dtype=np.float64).reshape(-1)) for b in gt_boxes]
        if len(self._gt) == 0:
            raise ValueError("empty gt bboxes in image 0 (it should contain at least one bbox)")
        for o, b in enumerate(self._gt):
            check_ground_truth_polygon(b, 0, o, _lib.UBD_POLY_MAX_VERTS)
        self._found = [np.asarray(b).reshape(-1) for b in found_boxes]
        self._gt_ids = self._found_ids = None
        if self._with_cls:
            if len(gt_object_types) != len(gt_boxes) or len(found_object_types) != len(found_boxes):
                raise AssertionError("uneq len")
            ids = dict((t, i) for i, t in enumerate(all_object_types))
            if any(t not in ids for t in list(gt_object_types) + list(found_object_types)):
                raise AssertionError("other types")
            self._gt_ids = [ids[t] for t in gt_object_types]
            self._found_ids = [ids[t] for t in found_object_types]

    def analyze(self, iou_threshold):
        torch = _require_gpu()
        dev = torch.device("cuda", torch.cuda.current_device())
        C = len(self._all_types) if self._with_cls else 0
        quads, classes, counts = _found_to_device([self._found], [self._found_ids] if self._with_cls else None, dev, C)
        acc = torch.zeros(accumulator_bytes(1, C), dtype=torch.uint8, device=dev)
        rec = evaluate_objects(quads, classes, counts, [self._gt], [self._gt_ids] if self._with_cls else None,
                               [float(iou_threshold)], C, acc)
        r = records_to_numpy(rec)[0, 0]
        a = unpack_accumulator(acc.cpu().numpy(), 1, C)
        return _metrics_from_record(r, a["confusion"][0], self._all_types, self._with_cls)


class DatasetMetricCalculator:
    """evaluation.py:432-544 with the sums kept on the device."""
    IOU_THRESHOLDS = np.arange(0.4, 1, 0.05)
    ERROR_IOU_THRESHOLD = 0.5

    def __init__(self, net_config, average_precision=False, rank_capacity=1 << 20):
        """average_precision: every batch is also ranked (``ubd_rank_detections``) into a device buffer of ``rank_capacity``
        records, ``evaluate_batch`` then needs the objects' scores, and ``get_metrics`` adds the keys of ``get_average_precision``."""
        self._net_config = net_config
        self._with_cls = bool(net_config.is_classification_supported())
        self._n_classes = net_config.get_n_classes() if self._with_cls else 0
        self._acc = None
        self._pix_acc = None
        self._images = 0
        self._with_ap = bool(average_precision)
        self._rank_capacity = int(rank_capacity)
        if self._with_ap and self._rank_capacity < 1:
            raise ValueError(f"rank_capacity must be positive, got {rank_capacity}")
        self._rank_buf = None

    def _accumulator(self, device):
        torch = _require_gpu()
        if self._acc is None:
            self._acc = torch.zeros(accumulator_bytes(len(self.IOU_THRESHOLDS), self._n_classes), dtype=torch.uint8, device=device)
        return self._acc

    def _split_gt(self, gt_objects):
        polys = [[np.asarray(o.bbox, dtype=np.float64).reshape(-1) for o in objs] for objs in gt_objects]
        cls = [[int(o.object_type) for o in objs] for objs in gt_objects] if self._with_cls else None
        return polys, cls

    def evaluate_batch(self, gt_objects, found_objects, gt_segmap=None, classification_logits=None, meta_infos=None, scales=None,
                       scores=None):
        """gt_objects: per image a list of markup records (``bbox``, ``object_type`` id).  found_objects: the same kind of
        lists (integer quads), or the device triple (quads, classes, counts) of ``ModelRunner.predict_on_device``.  scales:
        (n, 2) xscale, yscale applied to the found quads on the device (model_runner.py:140-148), or None.  Adds the batch
        to the device sums and returns (records, mask): the per-image records of every threshold as a device tensor -- no
        host copy is made here -- and the pixel classification correctness mask.  With a classification config and both
        gt_segmap (the label maps, (N, h, w) or (N, h, w, 1) int32) and classification_logits (the net's output or its class
        slice, see ``evaluate_pixels``) the pixel accuracies of evaluation.py:546-575 are added to their device sums too and
        mask is an int8 device tensor (N, h, w) of -1 / 0 / 1; in every other case mask is None.  scores: with
        ``average_precision=True`` required (ValueError without), the objects' confidences as a float32 device tensor (n, cap)
        (``Model.score_objects_on_device``) or per image a sequence in the order of ``found_objects[i]``; the batch is then
        ranked on the device behind its evaluation.  Without the flag ``scores`` is not looked at."""
        if self._with_ap and scores is None:
            raise ValueError("this calculator was made with average_precision=True: evaluate_batch needs the objects' scores")
        torch = _require_gpu()
        for i, objs in enumerate(gt_objects):
            if len(objs) == 0:
                raise ValueError(f"empty gt bboxes in image {self._images + i} (it should contain at least one bbox)")
        polys, cls = self._split_gt(gt_objects)
        if isinstance(found_objects, tuple) and len(found_objects) == 3 and hasattr(found_objects[0], "data_ptr"):
            quads, classes, counts = found_objects
        else:
            dev = torch.device("cuda", torch.cuda.current_device())
            boxes = [[o.bbox for o in objs] for objs in found_objects]
            fcls = [[int(o.object_type) for o in objs] for objs in found_objects] if self._with_cls else None
            quads, classes, counts = _found_to_device(boxes, fcls, dev, self._n_classes, self._images)
        if len(gt_objects) != int(quads.shape[0]):
            raise ValueError(f"{len(gt_objects)} ground-truth lists for {int(quads.shape[0])} images")
        if not self._with_ap:
            rec = evaluate_objects(quads, classes, counts, polys, cls, self.IOU_THRESHOLDS, self._n_classes,
                                   self._accumulator(quads.device), scales=scales, image_offset=self._images)
        else:                                           # the same call, keeping the workspace with the IoU tables for the ranking
            rec, tables = evaluate_objects(quads, classes, counts, polys, cls, self.IOU_THRESHOLDS, self._n_classes,
                                           self._accumulator(quads.device), scales=scales, image_offset=self._images, return_tables=True)
            if self._rank_buf is None:
                self._rank_buf = torch.zeros(rank_buffer_bytes(self._rank_capacity), dtype=torch.uint8, device=quads.device)
            rank_detections(self._scores_to_device(scores, quads), counts, polys, tables, self.IOU_THRESHOLDS, self._rank_buf)
        mask = None
        if self._with_cls and gt_segmap is not None and classification_logits is not None:
            if self._pix_acc is None:
                self._pix_acc = torch.zeros(pixel_accumulator_bytes(), dtype=torch.uint8, device=quads.device)
            _, mask = evaluate_pixels(classification_logits, gt_segmap, self._pix_acc, want_mask=True, n_classes=self._n_classes,
                                      per_image=False)
        self._images += len(gt_objects)
        return rec, mask

    @staticmethod
    def _scores_to_device(scores, quads):
        """scores as evaluate_batch takes them -> float32 device tensor (n, cap) beside ``quads``"""
        torch = _require_gpu()
        n, cap = int(quads.shape[0]), int(quads.shape[1])
        if not hasattr(scores, "data_ptr"):
            if len(scores) != n:
                raise ValueError(f"{len(scores)} score lists for {n} images")
            packed = np.zeros((n, cap), dtype=np.float32)
            for i, row in enumerate(scores):
                row = np.asarray(row, dtype=np.float32).reshape(-1)
                if len(row) > cap:
                    raise ValueError(f"image {i}: {len(row)} scores for at most {cap} found objects")
                packed[i, :len(row)] = row
            scores = torch.from_numpy(packed)
        if tuple(scores.shape) != (n, cap) or scores.dtype != torch.float32:
            raise ValueError(f"scores must be float32 {(n, cap)}, got {tuple(scores.shape)} {scores.dtype}")
        return scores.to(quads.device)

    def get_average_precision(self):
        """{"ap_iou0.40": ..., ..., "map": their mean over IOU_THRESHOLDS} after ONE read of the rank buffer.  COCO's greedy
        matching in descending score (``ubd_rank_detections``), not the reference's analysis: an ``ap_*`` and the ``pr_*`` /
        ``recall_*`` at the same threshold need not lie on one curve.  RuntimeError when records were dropped for lack of
        ``rank_capacity`` or an image was not ranked."""
        if not self._with_ap:
            raise RuntimeError("this calculator was made without average_precision=True")
        if self._rank_buf is None:
            raise RuntimeError("no batch has been evaluated")
        r = unpack_rank_buffer(self._rank_buf.cpu().numpy())
        if r["dropped"]:
            raise RuntimeError(f"{r['dropped']} detection record(s) were dropped: more than rank_capacity={self._rank_capacity} "
                               "detections in the epoch; raise the capacity")
        if r["flagged"]:
            raise RuntimeError(f"{r['flagged']} image(s) were not ranked: more found objects than max_objects_per_image "
                               f"(or more than {_lib.UBD_EVAL_MAX_GT} ground-truth objects); raise the capacity")
        out = {}
        for j, thr in enumerate(self.IOU_THRESHOLDS):
            out["ap_iou{:.2f}".format(thr)] = average_precision(r["scores"], (r["tp_mask"] >> np.uint32(j)) & np.uint32(1), r["n_gt"])
        out["map"] = float(np.mean([out["ap_iou{:.2f}".format(thr)] for thr in self.IOU_THRESHOLDS]))
        return out

    def get_per_threshold_metrics(self):
        """The one read of the epoch: {threshold: FtMetrics} from the device sums.  Raises RuntimeError when an image was
        not scored (more objects than the postprocess capacity: a truncated list is never scored)."""
        if self._acc is None:
            raise RuntimeError("no batch has been evaluated")
        T = len(self.IOU_THRESHOLDS)
        a = unpack_accumulator(self._acc.cpu().numpy(), T, self._n_classes)
        if a["flagged"]:
            raise RuntimeError(f"{a['flagged']} image(s) were not scored: more found objects than max_objects_per_image "
                               "(or malformed ground truth); raise the capacity")
        n = a["images"]
        out = {}
        for t, thr in enumerate(self.IOU_THRESHOLDS):
            m = FtMetrics(all_type_names=self._net_config.get_class_names(), compute_classification_metrics=self._with_cls)
            c = a["counters"][t]
            m.tp, m.fp, m.fn, m.one_to_one, m.one_to_many, m.many_to_one, m.matched_boxes_count = (int(v) for v in c[:7])
            m.average_iou = float(a["iou_sum"][t]) / m.matched_boxes_count if m.matched_boxes_count > 0 else 0
            m.matched_images_count = n
            if n > 0:
                m.average_precision_by_area, m.average_recall_by_area, m.average_iou_by_area = (float(v) / n for v in a["sums_by_area"])
                m.detection_rate = int(c[7]) / n
            if m.confusion_matrix is not None:
                m.confusion_matrix = a["confusion"][t].copy()
            out[thr] = m
        return out

    def get_metrics(self):
        """``scalar_logs`` of the epoch; with pixel sums (a classification config whose batches came with label maps and
        logits) also classification_pixel_acc_total and classification_pixel_acc_object (evaluation.py:526-530)."""
        logs = self.scalar_logs(self.get_per_threshold_metrics(), self._net_config)
        if self._pix_acc is not None:
            p = unpack_pixel_accumulator(self._pix_acc.cpu().numpy())
            if p["images"] > 0:
                logs.update(pixel_logs_from_sums(p["n_correct"], p["n_total"], p["n_objects"], p["object_acc_sum"]))
        if self._with_ap:
            logs.update(self.get_average_precision())
        return logs

    @classmethod
    def scalar_logs(cls, per_iou_metrics, net_config):
        """{threshold: FtMetrics} -> the flat dict of the reference's ``scalar_logs`` (evaluation.py:509-544; the key strings
        are the interface), without the two pixel accuracies (``get_metrics`` adds them from the pixel sums).  Per-type accuracies are logged at the threshold 0.5 only."""
        with_types = bool(net_config.is_classification_supported())
        logs = {}
        for thr in cls.IOU_THRESHOLDS:
            m = per_iou_metrics[thr]
            tag = "_iou{:.2f}".format(thr)
            entries = list(zip(("pr", "recall", "f1"), m.get_metrics())) + [("detection_rate", m.detection_rate)]
            if with_types and math.isclose(thr, cls.ERROR_IOU_THRESHOLD):
                entries.append(("types_avg_acc", m.get_average_acc()))
                entries += [(f"acc_{name}", value) for name, value in m.get_types_acc().items()]
            logs.update((prefix + tag, value) for prefix, value in entries)
        lowest = per_iou_metrics[cls.IOU_THRESHOLDS[0]]                 # the by-area means do not depend on the threshold
        for name in ("average_iou_by_area", "average_precision_by_area", "average_recall_by_area"):
            logs[name] = getattr(lowest, name)
        return logs


class ImageResultCategories:
    """The folders a result saver sorts an image's result into (the role of evaluation.py:579-628; the four names, the tuple
    SUITABLE_CATEGORIES and the three getters are the interface).  A category applies to an image when its test holds at
    ERROR_IOU_THRESHOLD and it is one of SUITABLE_CATEGORIES: precision errors are tested but not saved at present."""
    RECALL_ERROR = 'errors/recall'
    PRECISION_ERROR = 'errors/precision'
    DETECTION_RATE_ERROR = 'errors/detection_rate'
    ALL = 'all'

    SUITABLE_CATEGORIES = (RECALL_ERROR, DETECTION_RATE_ERROR, ALL)

    @classmethod
    def _from_scores(cls, detection_rate, precision, recall):
        """the applicable categories, in the order detection rate, precision, recall, all"""
        tests = ((cls.DETECTION_RATE_ERROR, detection_rate < 1), (cls.PRECISION_ERROR, precision < 1),
                 (cls.RECALL_ERROR, recall < 1), (cls.ALL, True))
        return [name for name, applies in tests if applies and name in cls.SUITABLE_CATEGORIES]

    @classmethod
    def get_categories(cls, metrics):
        """metrics: the FtMetrics of one image"""
        precision, recall, _ = metrics.get_metrics()
        return cls._from_scores(metrics.detection_rate, precision, recall)

    @classmethod
    def get_batch_categories(cls, records, iou_threshold=None):
        """The categories of every image of a batch from the device records ``evaluate_batch`` returned ((n, T, 80) uint8), at
        ``iou_threshold`` (default DatasetMetricCalculator.ERROR_IOU_THRESHOLD, the threshold evaluation.py:498 selects), with ONE
        read of the records.  An image that was not scored (flags != 0) raises RuntimeError, as ``get_metrics`` does."""
        wanted = DatasetMetricCalculator.ERROR_IOU_THRESHOLD if iou_threshold is None else iou_threshold
        columns = [t for t, value in enumerate(DatasetMetricCalculator.IOU_THRESHOLDS) if math.isclose(value, wanted)]
        if len(columns) != 1:
            raise ValueError(f"{wanted} is not one of the evaluated IoU thresholds")
        per_image = []
        for i, r in enumerate(records_to_numpy(records)[:, columns[0]]):
            if r["flags"]:
                raise RuntimeError(f"image {i} of the batch was not scored (flags {int(r['flags'])}): more found objects than "
                                   "max_objects_per_image, or malformed ground truth")
            precision, recall, _ = detection_scores(int(r["tp"]), int(r["fp"]), int(r["fn"]))
            per_image.append(cls._from_scores(int(r["detection_rate"]), precision, recall))
        return per_image

    @classmethod
    def get_errors(cls, visualization_categories):
        """the categories given without ALL: the error folders only"""
        return list(filter(lambda name: name != cls.ALL, visualization_categories))

    @classmethod
    def get_folders(cls):
        return cls.SUITABLE_CATEGORIES
