"""SegmapManager.postprocess -- host mirror of semantic_segmentation/segmap_manager.py:41-69.

Same static-method signature as the reference; the work (external components, contourArea
filter, minAreaRect, boxPoints, class vote) runs in libubd_hip.so on the MI355X.
"""
import collections
import ctypes
import logging
import os

import numpy as np
import torch
from PIL import Image, ImageDraw

from . import _lib
from .data_markup import ObjectMarkup, ClassifiedObjectMarkup

_reset_handles = _lib.reset_static_handles      # the reset under its earlier name here: callers written against that name keep working
_workspaces = _lib.StreamWorkspaces()   # (device, stream) -> uint8 tensor: the static entry points reuse their scratch between calls (LRU-bounded)


# per image: the scales of the reference's MetaInfo (data_generators.py:42-55, :189), original / rescaled, read by ModelRunner.rescale
ResizeMeta = collections.namedtuple("ResizeMeta", ["xscale", "yscale"])
_staging = {}   # device -> [pinned uint8 tensor, event of the transfer that last read it]


def _image_source(image, device):
    """One source image as an (H, W, C) uint8 array: numpy on the host, or a tensor on ``device`` (read in place)."""
    if isinstance(image, Image.Image):
        return np.asarray(image.convert("RGB"))          # the reference's readers (markup_readers.py:97,170)
    if isinstance(image, torch.Tensor) and image.is_cuda:
        if image.device != device:
            raise ValueError(f"image tensor on {image.device}, expected {device}")
        a = image
    else:
        a = image.numpy() if isinstance(image, torch.Tensor) else np.asarray(image)
    if a.dtype not in (np.uint8, torch.uint8):
        raise ValueError(f"images must be uint8, got {a.dtype}")
    if a.ndim == 2:
        a = a[:, :, None]
    if a.ndim != 3 or a.shape[2] not in (1, 3):
        raise ValueError(f"images must be HxW, HxWx1 or HxWx3, got shape {tuple(a.shape)}")
    return a.contiguous() if isinstance(a, torch.Tensor) else np.ascontiguousarray(a)


def _stage_host(arrays, device):
    """Host arrays -> one device buffer through one pinned staging buffer (filled by native threads) and one transfer.
    Returns (device buffer, byte offsets)."""
    lib = _lib.load()
    offsets = np.cumsum([0] + [a.nbytes for a in arrays])
    total = int(offsets[-1])
    entry = _staging.get(str(device))
    if entry is None or entry[0].numel() < total:
        entry = [torch.empty(max(total, 1 << 20), dtype=torch.uint8, pin_memory=True), None]
        _staging[str(device)] = entry
    elif entry[1] is not None:
        entry[1].synchronize()                           # the previous transfer out of the staging buffer is over
    base = entry[0].numpy().ctypes.data
    try:
        threads = max(1, min(8, len(os.sched_getaffinity(0)) // 2))
    except (AttributeError, OSError):
        threads = 1
    for a, off in zip(arrays, offsets):
        lib.ubd_host_memcpy_mt(base + int(off), a.ctypes.data, a.nbytes, threads)
    buf = torch.empty(max(total, 1), dtype=torch.uint8, device=device)
    buf[:total].copy_(entry[0][:total], non_blocking=True)
    entry[1] = torch.cuda.Event()
    entry[1].record(torch.cuda.current_stream(device))
    return buf, offsets[:-1]


def _stage_sources(srcs, device):
    """The sources of ``_image_source`` as ONE descriptor set over device memory: host arrays are staged (``_stage_host``),
    device tensors are read in place.  Returns (base address, int64 byte offsets from it, int32 (rows, cols) per image,
    channels, the tensors that hold the bytes -- keep them while the descriptors are in use)."""
    src_c = 3 if any(s.shape[2] == 3 for s in srcs) else 1
    if src_c == 3:                                       # a grey source among RGB ones: convert('RGB') replicates it
        srcs = [s if s.shape[2] == 3 else (s.expand(-1, -1, 3).contiguous() if isinstance(s, torch.Tensor) else np.repeat(s, 3, axis=2))
                for s in srcs]
    host = [k for k, s in enumerate(srcs) if not isinstance(s, torch.Tensor)]
    ptrs = [s.data_ptr() if isinstance(s, torch.Tensor) else 0 for s in srcs]
    keep = [s for s in srcs if isinstance(s, torch.Tensor)]
    if host:
        staged, offs = _stage_host([srcs[k] for k in host], device)
        keep.append(staged)
        for k, off in zip(host, offs):
            ptrs[k] = staged.data_ptr() + int(off)
    base = min(ptrs)
    offsets = np.array([p - base for p in ptrs], np.int64)
    hw = np.array([[s.shape[0], s.shape[1]] for s in srcs], np.int32)
    return base, offsets, hw, src_c, keep


def _resize_staged(stage, new_h, new_w, dst_c, device):
    """ubd_resize_images of every staged source into one (N, new_h, new_w, dst_c) tensor."""
    base, offsets, hw, src_c, _ = stage
    out = torch.empty((len(offsets), new_h, new_w, dst_c), dtype=torch.uint8, device=device)
    _lib.launch("ubd_resize_images", device, ctypes.c_void_p(base), offsets.ctypes.data, hw.ctypes.data, src_c, len(offsets),
                out.data_ptr(), new_h, new_w, dst_c)
    return out


def _resize_sources(srcs, new_h, new_w, dst_c, device):
    """ubd_resize_images of every source (host arrays and device tensors alike) into one (N, new_h, new_w, dst_c) tensor."""
    return _resize_staged(_stage_sources(srcs, device), new_h, new_w, dst_c, device)


class SegmapManager:
    @staticmethod
    def postprocess(seg_map, seg_map_class_logits=None, scale=1, min_area_threshold=5, max_objects=1024):
        """seg_map: (h,w,1) or (h,w) array of {0,1}; seg_map_class_logits: (h,w,n_cls) or None.
        Returns list[ObjectMarkup] / list[ClassifiedObjectMarkup] like the reference."""
        _lib.require_gpu("SegmapManager.postprocess")
        lib = _lib.load()
        device = torch.device(f"cuda:{torch.cuda.current_device()}")
        m = np.asarray(seg_map)
        m = m.reshape(m.shape[0], m.shape[1])
        h, w = m.shape
        n_cls = 0 if seg_map_class_logits is None else int(np.shape(seg_map_class_logits)[-1])
        # pack (map, class logits) as a (1,h,w,1+n_cls) logits tensor; map != 0 <=> "logit" 1 > 0.5
        lg = np.zeros((1, h, w, 1 + n_cls), np.float32)
        lg[0, :, :, 0] = (m != 0)
        if n_cls:
            lg[0, :, :, 1:] = np.asarray(seg_map_class_logits, np.float32)
        lgt = torch.from_numpy(lg).to(device)
        hd = _lib.static_handle(n_cls, device)
        cap = max_objects
        quads = torch.empty((1, cap, 8), dtype=torch.int32, device=device)      # the library writes the count and the list's first entries
        classes = torch.empty((1, cap), dtype=torch.int32, device=device)
        counts = torch.empty((1,), dtype=torch.int32, device=device)
        # one scratch per (device, stream): calls on one stream are ordered, two streams never share one (grown on demand, never shrunk)
        stream = _lib.current_stream(device)
        ws = _workspaces.get(device, stream, lib.ubd_postprocess_workspace_bytes(hd, 1, h, w, cap))
        _lib.launch("ubd_postprocess", device, hd, lgt.data_ptr(), 1, h, w, 0.5, int(scale), float(min_area_threshold),
                    None, quads.data_ptr(), classes.data_ptr(), counts.data_ptr(), cap, ws.data_ptr(), ws.numel(), stream=stream)
        n = int(counts.cpu()[0])
        if n > cap:
            raise RuntimeError(f"more than max_objects={cap} objects found ({n})")
        q = quads.cpu().numpy()[0, :n].astype(int)
        if seg_map_class_logits is None:
            return [ObjectMarkup(bbox) for bbox in q]
        c = classes.cpu().numpy()[0, :n]
        return [ClassifiedObjectMarkup(bbox, class_id) for bbox, class_id in zip(q, c)]

    @staticmethod
    def prepare_image_and_target(image, markup, net_config, augment=False, photo_rng=None, photo_extended=False,
                                 photo_noise_alpha=False):
        """segmap_manager.py:24-39: with ``augment``, the geometric chain of the reference's augmentation first (one PIL image
        through ``SegLinksImageAugmentation``: parameters from ``random`` / ``numpy.random``, pixels warped on the MI355X,
        bit-identical to Pillow; with ``photo_rng``, a ``numpy.random.Generator``, also the built operations of the imgaug
        photometric stage, with ``photo_extended`` MedianBlur, AddToHueAndSaturation and ElasticTransformation among them,
        with ``photo_noise_alpha`` SimplexNoiseAlpha and FrequencyNoiseAlpha too --
        which are built, which are not, and that parity with imgaug / OpenCV is unpinned: ubdvss_amd/augmentation.py), then rescale image + markup to the network's size rule, build the label map at
        ``net_config.get_scale()``.  Returns (image, markup, label map) like the reference."""
        if augment:
            from .augmentation import SegLinksImageAugmentation
            aug = SegLinksImageAugmentation(image, markup, net_config, photo_rng=photo_rng, photo_extended=photo_extended,
                                            photo_noise_alpha=photo_noise_alpha)
            image, markup = aug.get_modified_image(), aug.get_modified_markup()
        image, markup = SegmapManager._rescale_image_and_markup(image, markup, net_config)
        return image, markup, SegmapManager.build_segmentation_map(image, markup, scale=net_config.get_scale())

    @staticmethod
    def build_segmentation_map(image, markup, scale=1, for_drawing=False):
        """Training label map (behaviour of segmap_manager.py:81-104): every quad is divided by ``scale``, its
        corners are snapped outward (``_proper_round``; a polygon of another vertex count, 3..64 -- markup read from
        segmentation maps -- is truncated instead, as the reference does) and the polygon is filled, later objects over earlier
        ones, with 255 (``for_drawing``), class id + 1 (classified markup) or 1.  Returns a PIL 'L' image of
        size (W/scale, H/scale)."""
        width, height = image.size
        if width % scale or height % scale:
            raise AssertionError("image size must be a multiple of the map scale")
        canvas = Image.new('L', (width // scale, height // scale), 0)
        pen = ImageDraw.Draw(canvas)
        for obj in markup:
            value = 255 if for_drawing else (getattr(obj, "object_type", 0) + 1 if isinstance(obj, ClassifiedObjectMarkup) else 1)
            if value > 255:
                raise AssertionError("No more than 255 classes are supported")
            corners = SegmapManager._proper_round(np.asarray(obj.bbox, dtype=np.float64) / scale)
            pen.polygon([int(v) for v in corners], fill=int(value))
        return canvas

    @staticmethod
    def build_segmentation_maps_on_device(image_size, markups, scale=1, for_drawing=False, device=None, strict_markup=False):
        """Batch form of ``build_segmentation_map`` on the MI355X (ubd_build_label_maps; ubd_build_label_maps_polygons when an
        object is not a quad but a polygon of 5..64 vertices, markup read from segmentation maps; a triangle raises ValueError as
        it did before polygons were accepted): ``markups`` is a list (one entry
        per image) of lists of ObjectMarkup / ClassifiedObjectMarkup, ``image_size`` = (width, height) like ``PIL.Image.size``.
        Returns an int32 device tensor (N, height/scale, width/scale) -- the y_true layout of the loss / train step.
        Degenerate quads whose OPPOSITE corners coincide on the map (a point or a folded segment -- a labelling error) are drawn
        like every other quad and logged; ``strict_markup=True`` refuses them instead (see ``_check_folded_quads``)."""
        _lib.require_gpu("SegmapManager.build_segmentation_maps_on_device")
        device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        width, height = image_size
        if width % scale or height % scale:
            raise AssertionError("image size must be a multiple of the map scale")
        n = len(markups)
        cap = max(1, max((len(m) for m in markups), default=1))
        # float64 markup, as it reaches the reference's `object_markup.bbox / scale` (segmap_manager.py:96): rescaled or
        # augmented quads are fractional, and _proper_round floors / ceils the QUOTIENT -- truncating the markup first
        # would move a corner by a whole map pixel (12.3 / 4 ceils to 4, 12 / 4 to 3)
        sizes = [[np.asarray(obj.bbox).size for obj in objs] for objs in markups]
        for i, row in enumerate(sizes):
            for j, size in enumerate(row):
                # three points stay refused here, as they always were (tests/test_gpu_raster.py pins it); the device call draws them
                if size % 2 or not 8 <= size <= 2 * _lib.UBD_POLY_MAX_VERTS:
                    raise ValueError(f"object markup must be a quadrilateral (8 numbers) or a polygon of 5..{_lib.UBD_POLY_MAX_VERTS} "
                                     f"vertices, got {size} numbers (image {i}, object {j})")
        max_verts = max([4] + [size // 2 for row in sizes for size in row])
        polygons = any(size != 8 for row in sizes for size in row)      # a batch of quads only still takes ubd_build_label_maps
        verts = np.zeros((n, cap, max_verts * 2), np.float64)
        nverts = np.zeros((n, cap), np.int32)
        values = np.zeros((n, cap), np.int32)
        counts = np.zeros((n,), np.int32)
        for i, objs in enumerate(markups):
            counts[i] = len(objs)
            for j, obj in enumerate(objs):
                value = 255 if for_drawing else (getattr(obj, "object_type", 0) + 1 if isinstance(obj, ClassifiedObjectMarkup) else 1)
                if value > 255:
                    raise AssertionError("No more than 255 classes are supported")
                bbox = np.asarray(obj.bbox, dtype=np.float64).reshape(-1)
                verts[i, j, :bbox.size] = bbox
                nverts[i, j] = bbox.size // 2
                values[i, j] = value
        quads = np.ascontiguousarray(verts[:, :, :8])
        SegmapManager._check_folded_quads(quads, counts, scale, strict_markup, nverts == 4)
        labels = torch.empty((n, height // scale, width // scale), dtype=torch.int32, device=device)
        if not polygons:
            qd, vd, cd = (torch.from_numpy(a).to(device) for a in (quads, values, counts))
            _lib.launch("ubd_build_label_maps", device, qd.data_ptr(), vd.data_ptr(), cd.data_ptr(), n, cap, height // scale, width // scale,
                        int(scale), labels.data_ptr())
            return labels
        pd, nd, vd, cd = (torch.from_numpy(a).to(device) for a in (verts, nverts, values, counts))
        _lib.launch("ubd_build_label_maps_polygons", device, pd.data_ptr(), nd.data_ptr(), vd.data_ptr(), cd.data_ptr(), n, cap, max_verts,
                    height // scale, width // scale, int(scale), labels.data_ptr())
        return labels

    @staticmethod
    def _check_folded_quads(quads, counts, scale, strict=False, is_quad=None):
        """The device fill rule is Pillow's for every quadrilateral except a zero-area fold whose OPPOSITE corners coincide
        after snapping (four edges in one point: Pillow's corner joining there depends on its internal edge order and is not
        restated, oracle/label_raster.py).  The reference draws whatever ``ImageDraw.polygon`` draws for such markup
        (segmap_manager.py:93-103) and carries on; so does this builder -- the device rule gives Pillow's pixels for ~96 % of random such
        quads and differs inside ONE row (a fragment of that row's span: median 2 pixels, 90th percentile 10) for the rest
        (tests/test_gpu_raster.py measures both) -- and logs
        a warning, because such an object is a labelling error.  ``strict``: raise instead.  Returns the number found."""
        pts = (quads / float(scale)).reshape(quads.shape[0], quads.shape[1], 4, 2)
        n_larger = (pts[:, :, None, :, :] > pts[:, :, :, None, :]).sum(axis=3)
        snapped = np.where(n_larger > 1, np.floor(pts), np.ceil(pts))
        folded = ((snapped[:, :, 0] == snapped[:, :, 2]).all(-1) | (snapped[:, :, 1] == snapped[:, :, 3]).all(-1))
        folded &= np.arange(quads.shape[1])[None, :] < np.asarray(counts)[:, None]
        if is_quad is not None:                              # polygon markup in the batch: the rule concerns its quads only
            folded &= is_quad
        if folded.any():
            i, j = np.argwhere(folded)[0]
            msg = (f"{int(folded.sum())} object(s) whose opposite corners coincide on the label map, first: object {j} of image {i} "
                   f"({quads[i, j].tolist()} at scale {scale})")
            if strict:
                raise ValueError(msg + "; fix the markup")
            logging.warning("label maps: %s -- drawn as a degenerate polygon (may differ from Pillow inside the fold point's row)", msg)
        return int(folded.sum())

    @staticmethod
    def target_size(w, h, net_config, max_side=None):
        """The size rule of ``_rescale_image_and_markup`` (segmap_manager.py:135-173) for an image of w x h pixels: if the
        longer side exceeds ``max_side`` (default ``net_config.get_max_side()``) it becomes exactly ``max_side`` and the other
        side is scaled in proportion and rounded to a multiple of ``net_config.get_side_multiple()``; otherwise both sides are
        rounded to that multiple.  Rounding is Python 3's ``round`` (half to even), at least one multiple.  Returns (new_w, new_h)."""
        multiple = net_config.get_side_multiple()
        if max_side is None:
            max_side = net_config.get_max_side()

        def to_multiple(side):
            return max(1, round(side / multiple)) * multiple

        if max(w, h) > max_side:
            shrink = max_side / max(h, w)
            return (max_side, to_multiple(h * shrink)) if w > h else (to_multiple(w * shrink), max_side)
        return to_multiple(w), to_multiple(h)

    @staticmethod
    def _rescale_image_and_markup(image, markup, net_config, max_side=None):
        """Image and markup at the size the network wants (behaviour of segmap_manager.py:135-173): the size is
        ``target_size``'s, the image is resampled with ``Image.BICUBIC``; every quad is multiplied by (new_w / w, new_h / h)
        and rewrapped with ``create_same_markup`` (so it stays fractional, float64).  Empty / None markup is returned as it
        is.  A PIL image in, a PIL image out, like the reference; ``rescale_images_on_device`` is the batch form on the MI355X."""
        w, h = image.size
        new_w, new_h = SegmapManager.target_size(w, h, net_config, max_side)
        resized = image.resize(size=(new_w, new_h), resample=Image.BICUBIC)
        return resized, SegmapManager._rescale_markup(markup, w, h, new_w, new_h)

    @staticmethod
    def _rescale_markup(markup, w, h, new_w, new_h):
        if not markup:
            return markup
        factors = np.array([[new_w / w, new_h / h]])
        return [m.create_same_markup((np.array(m.bbox).reshape((-1, 2)) * factors).reshape((-1,))) for m in markup]

    @staticmethod
    def rescale_images_on_device(images, net_config, device=None, max_side=None):
        """Batch form of the image half of ``_rescale_image_and_markup`` + the ``convert('L')`` of grey nets
        (data_generators.py:164-180) on the MI355X (ubd_resize_images, bit-identical to Pillow's BICUBIC resize).
        ``images``: PIL images (taken through ``.convert('RGB')`` like the reference's readers), HxW / HxWx1 / HxWx3 uint8
        numpy arrays or uint8 device tensors of those shapes (read in place, no copy), of any sizes that share one
        ``target_size``.  Host images are staged through one pinned buffer and one transfer.
        Returns (uint8 device tensor (N, new_h, new_w, c_in of the net), [ResizeMeta(xscale, yscale)] per image) where
        xscale = w / new_w and yscale = h / new_h: the ``MetaInfo`` scales of data_generators.py:189 that ``ModelRunner.rescale``
        reads.  Raises ValueError if the images do not share one target size."""
        out, sizes = SegmapManager._rescale_images(images, net_config, device, max_side)
        new_h, new_w = int(out.shape[1]), int(out.shape[2])
        return out, [ResizeMeta(w / new_w, h / new_h) for w, h in sizes]

    @staticmethod
    def _rescale_images(images, net_config, device, max_side=None):
        """rescale_images_on_device -> (device tensor, [(w, h) of every source image])"""
        return SegmapManager._rescale_images_staged(images, net_config, device, max_side)[:2]

    @staticmethod
    def _rescale_images_staged(images, net_config, device, max_side=None):
        """_rescale_images that also hands back the staged sources (``_stage_sources``) it resized: the raw frames as they lie
        in device memory, for a second reader (ModelRunner.predict_patches cuts the found objects out of them)."""
        _lib.require_gpu("SegmapManager.rescale_images_on_device")
        device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        srcs = [_image_source(im, device) for im in images]
        if not srcs:
            raise ValueError("no images")
        sizes = [(int(s.shape[1]), int(s.shape[0])) for s in srcs]
        targets = {SegmapManager.target_size(w, h, net_config, max_side) for w, h in sizes}
        if len(targets) != 1:
            raise ValueError(f"the images do not share one target size ({sorted(targets)}); group them by "
                             "SegmapManager.target_size first (ModelRunner.predict_images does)")
        new_w, new_h = targets.pop()
        stage = _stage_sources(srcs, device)
        return _resize_staged(stage, new_h, new_w, 1 if net_config.is_grey() else 3, device), sizes, stage

    @staticmethod
    def prepare_batch_on_device(images, markups, net_config, device=None):
        """Training form of ``prepare_image_and_target`` (+ ``convert('L')`` for grey nets) for a batch on the MI355X:
        returns (uint8 images (N, h, w, c_in) of ``rescale_images_on_device``, int32 label maps (N, h/scale, w/scale) of
        ``build_segmentation_maps_on_device``, the markups scaled by (new_w / w, new_h / h) exactly as
        ``_rescale_image_and_markup`` scales them).  Images as in ``rescale_images_on_device``."""
        _lib.require_gpu("SegmapManager.prepare_batch_on_device")
        if len(images) != len(markups):
            raise ValueError("one markup per image is required")
        x, sizes = SegmapManager._rescale_images(images, net_config, device)
        new_h, new_w = int(x.shape[1]), int(x.shape[2])
        rescaled = [SegmapManager._rescale_markup(m, w, h, new_w, new_h) for m, (w, h) in zip(markups, sizes)]
        labels = SegmapManager.build_segmentation_maps_on_device((new_w, new_h), [m or [] for m in rescaled],
                                                                 scale=net_config.get_scale(), device=x.device)
        return x, labels, rescaled

    @staticmethod
    def prepare_batches_on_device(images, markups, net_config, augment=True, plans=None, device=None, photo_rng=None,
                                  photo_extended=False, photo_noise_alpha=False):
        """Training form of ``prepare_image_and_target(..., augment=True)`` (+ ``convert('L')`` for grey nets) for a batch on
        the MI355X.  Augmented images no longer share one size, and the reference groups a batch by resized shape
        (data_generators.py:133-140), so the result is a list with one entry per target size, in order of first appearance:
        (indices into ``images``, uint8 images (n, h, w, c_in), int32 label maps (n, h/scale, w/scale), the augmented and
        rescaled markups, the plans), every list in the order of ``indices``.
        Chain: the raw images are staged once -> the warp passes of all images (``ubd_warp_images``: every rotation, then every
        perspective / final copy; crops and quarter turns are views) -> the photometric stages of the plans
        (``ubd_photometric_images`` and ``ubd_noise_alpha_images``, one call each per slot) -> ``ubd_resize_images`` per group ->
        ``ubd_build_label_maps`` per group; no host synchronisation and no device-to-host copy in between.
        ``plans``: one ``AugmentationPlan`` per image to replay (tests, reproducibility); otherwise ``augment=True`` draws them
        with ``augmentation.sample_plan`` from ``random`` / ``numpy.random`` in image order, ``augment=False`` uses empty plans.
        ``photo_rng``: a ``numpy.random.Generator`` handed to ``sample_plan`` for the imgaug photometric stage (None: the stage's
        draw is consumed and recorded, no pixels change); ``photo_extended``: handed to ``sample_plan`` too, the stage then also
        draws MedianBlur, AddToHueAndSaturation and ElasticTransformation (off: they stay recorded no-ops); ``photo_noise_alpha``: likewise for
        SimplexNoiseAlpha and FrequencyNoiseAlpha -- with both flags the whole stage of the reference runs.  What of that stage is built, what is not, and that parity with imgaug /
        OpenCV is unpinned: ubdvss_amd/augmentation.py.  Images as in ``rescale_images_on_device``."""
        _lib.require_gpu("SegmapManager.prepare_batches_on_device")
        from . import augmentation
        if len(images) != len(markups):
            raise ValueError("one markup per image is required")
        if plans is not None and len(plans) != len(images):
            raise ValueError("one plan per image is required")
        if not len(images):
            raise ValueError("no images")
        if augment or plans is not None:                       # the augmentation moves quads; polygon markup is out of scope
            for i, m in enumerate(markups):
                for j, obj in enumerate(m or []):
                    if np.asarray(obj.bbox).size != 8:
                        raise ValueError(f"augmentation of polygon markup is not supported: object {j} of image {i} has "
                                         f"{np.asarray(obj.bbox).size // 2} vertices (use augment=False)")
        device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        srcs = [_image_source(im, device) for im in images]
        if any(s.shape[2] == 3 for s in srcs):                 # a grey source among RGB ones: convert('RGB') replicates it
            srcs = [s if s.shape[2] == 3 else (s.expand(-1, -1, 3).contiguous() if isinstance(s, torch.Tensor) else np.repeat(s, 3, axis=2))
                    for s in srcs]
        if plans is None:
            plans = [augmentation.sample_plan((s.shape[1], s.shape[0]), m, photo_rng=photo_rng, photo_extended=photo_extended,
                                             photo_noise_alpha=photo_noise_alpha) if augment
                     else augmentation.identity_plan((s.shape[1], s.shape[0]))
                     for s, m in zip(srcs, markups)]
        warped = augmentation.augment_arrays_on_device(srcs, plans, device)
        moved = [augmentation.apply_plan_to_markup(p, m) for p, m in zip(plans, markups)]
        groups = collections.OrderedDict()
        for i, t in enumerate(warped):
            groups.setdefault(SegmapManager.target_size(int(t.shape[1]), int(t.shape[0]), net_config), []).append(i)
        out = []
        for (new_w, new_h), idx in groups.items():
            x = _resize_sources([warped[i] for i in idx], new_h, new_w, 1 if net_config.is_grey() else 3, device)
            rescaled = [SegmapManager._rescale_markup(moved[i], int(warped[i].shape[1]), int(warped[i].shape[0]), new_w, new_h) for i in idx]
            labels = SegmapManager.build_segmentation_maps_on_device((new_w, new_h), [m or [] for m in rescaled],
                                                                     scale=net_config.get_scale(), device=device)
            out.append((idx, x, labels, rescaled, [plans[i] for i in idx]))
        return out

    @staticmethod
    def _proper_round(markup_bbox):
        """Outward snapping of a quad's corners (behaviour of segmap_manager.py:106-133): a coordinate is floored
        when at least two of the four coordinates on the same axis are strictly larger (the object extends to
        the larger side), otherwise it is ceiled; anything that is not 4 points (a hull read from a segmentation map) is
        truncated to int32, as the reference does (segmap_manager.py:114-116)."""
        pts = np.asarray(markup_bbox, dtype=np.float64)
        if pts.size != 8:
            return np.asarray(markup_bbox).astype(np.int32)
        pts = pts.reshape(4, 2)
        n_larger = (pts[None, :, :] > pts[:, None, :]).sum(axis=1)          # per corner, per axis
        snapped = np.where(n_larger > 1, np.floor(pts), np.ceil(pts))
        return snapped.reshape(-1).astype(np.int32)
