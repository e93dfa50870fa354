"""Visualisations -- host mirror of semantic_segmentation/visualizations.py (Visualizer, :14-151).

The reference draws every image of a batch three or four times with Pillow on the host.  Here the four overlays are one
``ubd_visualize_images`` call (include/ubd.h) over what the forward pass, the postprocess and the evaluation left in device
memory: the images, the label maps, the binary map, the found quads and the pixel classification mask.  The images returned
match the reference's pixel for pixel (tests/visualization_oracle.py restates them with the Pillow calls).
There is no CPU path: without a GPU the entry points raise ``RuntimeError``.

Maps must be an integer factor smaller than the images (1 and the net's scale 4 are the cases of the reference's run loop).
"""
import numpy as np

from . import _lib
from .net import PreprocessingType


def _pre_code(preprocessing):
    if preprocessing is None or preprocessing in (PreprocessingType.NONE, _lib.UBD_PRE_NONE, "none"):
        return _lib.UBD_PRE_NONE
    if preprocessing in (PreprocessingType.MOBILENET_LIKE, "mobilenet_like") or (isinstance(preprocessing, int) and preprocessing == _lib.UBD_PRE_MOBILENET):
        return _lib.UBD_PRE_MOBILENET
    raise ValueError(f"unknown preprocessing {preprocessing!r}")


def _map(torch, t, n, dtype, device, what):
    """(N, h, w) or (N, h, w, 1) tensor / array -> contiguous (N, h, w) device tensor of ``dtype``"""
    if not torch.is_tensor(t):
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(t)))
    if t.dim() == 4 and t.shape[3] == 1:
        t = t[..., 0]
    if t.dim() != 3 or int(t.shape[0]) != n:
        raise ValueError(f"{what} must be (N, h, w) or (N, h, w, 1) with N = {n}, got {tuple(t.shape)}")
    return t.to(device=device, dtype=dtype).contiguous()


def _draw(images, preprocessing=None, gt=None, seg=None, found=None, cls=None):
    """One ubd_visualize_images call on the current stream; a source that is None is not drawn.  gt / seg: int32 maps whose
    positive entries are drawn, found: (quads, counts) int32, cls: int8 mask.  Returns {key: (N, H, W, 3) uint8 tensor}."""
    torch = _lib.require_gpu("ubdvss_amd.visualizations")
    if not torch.is_tensor(images) or not images.is_cuda:
        raise ValueError("images must be a device tensor (the numpy entry points upload them: compute_visualizations, draw_bboxes, ...)")
    if images.dim() == 3:
        images = images[..., None]
    if images.dim() != 4 or int(images.shape[3]) not in (1, 3):
        raise ValueError(f"images must be (N, H, W, 1 or 3), got {tuple(images.shape)}")
    if images.dtype == torch.uint8:
        in_dtype = _lib.UBD_IN_U8
    else:
        in_dtype = _lib.UBD_IN_F32
        images = images.to(torch.float32)
    images = images.contiguous()
    dev = images.device
    n, hh, ww, c = (int(v) for v in images.shape)
    maps = {}
    for key, src, dtype in (("gt", gt, torch.int32), ("seg_map", seg, torch.int32), ("classification_gt", cls, torch.int8)):
        if src is not None:
            maps[key] = _map(torch, src, n, dtype, dev, key)
    shapes = set(tuple(m.shape[1:]) for m in maps.values())
    if len(shapes) > 1:
        raise ValueError(f"the maps differ in size: {sorted(shapes)}")
    mh, mw = shapes.pop() if shapes else (hh, ww)
    quads = counts = None
    cap = 0
    if found is not None:
        quads, counts = found
        quads = quads.to(device=dev, dtype=torch.int32).contiguous()
        counts = counts.to(device=dev, dtype=torch.int32).contiguous()
        if quads.dim() != 3 or int(quads.shape[0]) != n or int(quads.shape[2]) != 8 or tuple(counts.shape) != (n,):
            raise ValueError(f"found objects must be quads (N, cap, 8) and counts (N) with N = {n}, got {tuple(quads.shape)}, {tuple(counts.shape)}")
        cap = int(quads.shape[1])
    out = {}
    for key, present in (("gt", "gt" in maps), ("seg_map", "seg_map" in maps), ("postprocessed", found is not None),
                         ("classification_gt", "classification_gt" in maps)):
        if present:
            out[key] = torch.empty((n, hh, ww, 3), dtype=torch.uint8, device=dev)

    def ptr(t):
        return t.data_ptr() if t is not None else None
    _lib.launch(
        "ubd_visualize_images", dev, images.data_ptr(), in_dtype, _pre_code(preprocessing), n, hh, ww, c, int(mh), int(mw),
        ptr(maps.get("gt")), ptr(maps.get("seg_map")), ptr(quads), ptr(counts), cap, ptr(maps.get("classification_gt")),
        ptr(out.get("gt")), ptr(out.get("seg_map")), ptr(out.get("postprocessed")), ptr(out.get("classification_gt")))
    # the inputs were allocated (or are used) on this stream: the caching allocator reuses them in stream order
    return out


def _positive(torch, target, threshold):
    """target > threshold as an int32 map (a float map is thresholded with torch, integer labels > 0.5 are labels > 0)"""
    if target is None:
        return None
    if not torch.is_tensor(target):
        target = torch.from_numpy(np.ascontiguousarray(np.asarray(target)))
    if not target.is_floating_point() and target.dtype != torch.bool and 0 <= threshold < 1:
        return target                                   # integer labels: the kernel draws the positive entries
    return (target > threshold).to(torch.int32)


def _device_images(torch, images):
    if torch.is_tensor(images):
        return images if images.is_cuda else images.cuda()
    x = np.asarray(images)
    if x.dtype != np.uint8:
        x = x.astype(np.float32, copy=False)
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _found_pair(found_objects):
    """(quads, classes, counts) of predict_on_device, or (quads, counts)"""
    if len(found_objects) == 3:
        return found_objects[0], found_objects[2]
    quads, counts = found_objects
    return quads, counts


def _pack_markup(torch, image_markups):
    """lists of markup records -> (quads, counts) host tensors in the layout of ubd_postprocess, through
    ``evaluation.pack_found_objects``: integer convex quadrilaterals, what the postprocess finds (ValueError otherwise)"""
    from .evaluation import pack_found_objects
    quads, _, counts = pack_found_objects([[o.bbox for o in objs] for objs in image_markups])
    return torch.from_numpy(quads), torch.from_numpy(counts)


class Visualizer:
    """The public names of the reference's Visualizer; the ``*_on_device`` form keeps everything in device memory."""

    @staticmethod
    def compute_visualizations_on_device(images, gt_segmap, predicted_segmap, found_objects, pixel_classification_mask=None,
                                         preprocessing=None):
        """images: device tensor (N, H, W, C), uint8 (raw pixels) or float (then ``preprocessing``, a PreprocessingType, names
        the denorm applied before the cast to uint8).  gt_segmap / predicted_segmap: device maps (N, h, w) or (N, h, w, 1),
        drawn where > 0.5.  found_objects: the (quads, classes, counts) triple of ``ModelRunner.predict_on_device``, or
        (quads, counts), in the coordinates of ``images``.  pixel_classification_mask: the int8 mask of ``evaluate_batch`` or
        None.  Returns {'gt', 'seg_map', 'postprocessed'[, 'classification_gt']}: device uint8 tensors (N, H, W, 3).
        One kernel launch; nothing leaves the device.  ``images`` must be a device tensor (ValueError otherwise).  The maps,
        the mask and the found objects are expected on the device too; a host array or CPU tensor among them is accepted
        and costs one upload each (``ModelRunner.run`` passes numpy label maps this way)."""
        torch = _lib.require_gpu("ubdvss_amd.visualizations")
        return _draw(images, preprocessing, gt=_positive(torch, gt_segmap, 0.5), seg=_positive(torch, predicted_segmap, 0.5),
                     found=_found_pair(found_objects), cls=pixel_classification_mask)

    @staticmethod
    def compute_visualizations(images, gt_segmap, predicted_segmap, found_objects, pixel_classification_mask=None, preprocessing=None):
        """visualizations.py:20-49 with numpy in and numpy out: ``images`` are the original pictures (uint8, or floats that are
        cast as ``astype(np.uint8)`` after the denorm ``preprocessing`` names), ``found_objects`` lists of markup records per image.
        One transfer each way.  Returns a dict of (N, H, W, 3) uint8 arrays (indexable per image like the reference's lists)."""
        torch = _lib.require_gpu("ubdvss_amd.visualizations")
        x = _device_images(torch, images)
        quads, counts = _pack_markup(torch, found_objects)
        out = Visualizer.compute_visualizations_on_device(x, gt_segmap, predicted_segmap, (quads, counts), pixel_classification_mask,
                                                          preprocessing)
        keys = list(out)
        host = torch.stack([out[k] for k in keys]).cpu().numpy()
        return {k: host[i] for i, k in enumerate(keys)}

    @staticmethod
    def visualize_segmentation_maps(images, targets, threshold=0.5):
        """visualizations.py:52-68: green where target > threshold; (N, H, W, 3) uint8 array"""
        torch = _lib.require_gpu("ubdvss_amd.visualizations")
        if len(images) != len(targets):
            raise AssertionError("one target per image is required")
        return _draw(_device_images(torch, images), gt=_positive(torch, targets, threshold))["gt"].cpu().numpy()

    @staticmethod
    def visualize_segmentation_map(image, target, threshold=0.5):
        """visualizations.py:108-123 for one image"""
        return Visualizer.visualize_segmentation_maps(np.asarray(image)[None], np.asarray(target)[None], threshold)[0]

    @staticmethod
    def visualize_classification_masks(images, targets):
        """visualizations.py:71-79: green where the mask is 1, red where it is -1"""
        torch = _lib.require_gpu("ubdvss_amd.visualizations")
        if len(images) != len(targets):
            raise AssertionError("one target per image is required")
        if not torch.is_tensor(targets):
            targets = torch.from_numpy(np.ascontiguousarray(np.asarray(targets)))
        cls = (targets == 1).to(torch.int8) - (targets == -1).to(torch.int8)
        return _draw(_device_images(torch, images), cls=cls)["classification_gt"].cpu().numpy()

    @staticmethod
    def visualize_classification_mask(image, is_pixel_correct):
        """visualizations.py:82-91 for one image"""
        return Visualizer.visualize_classification_masks(np.asarray(image)[None], np.asarray(is_pixel_correct)[None])[0]

    @staticmethod
    def draw_bboxes(images, image_markups):
        """visualizations.py:94-105: every markup quad filled green at image resolution"""
        torch = _lib.require_gpu("ubdvss_amd.visualizations")
        if len(images) != len(image_markups):
            raise AssertionError("one markup list per image is required")
        return _draw(_device_images(torch, images), found=_pack_markup(torch, image_markups))["postprocessed"].cpu().numpy()

    @staticmethod
    def draw_markup(image, markup):
        """visualizations.py:126-135 for one image (a PIL image or an array); returns the (H, W, 3) uint8 array"""
        return Visualizer.draw_bboxes(np.asarray(image)[None], [markup])[0]
