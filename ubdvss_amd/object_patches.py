"""Rectified patches of the found objects, cut out of the original frames on the MI355X (``ubd_extract_objects``, include/ubd.h):
the hand-over to a decoder, which on the host is one ``Image.transform((w, h), Image.QUAD, data, Image.BILINEAR)`` per object
on frames copied back first.  Bit-identical to that Pillow call (tests/test_object_patches_host.py pins the restatement,
tests/test_gpu_object_patches.py the device against it).

Orientation: the corners are taken clockwise on the screen, and the patch's top edge is a LONG side of the quad, so a patch is
a rotation of its object, never a mirror image; which long side is on top stays open (a half turn), decoders read both ways.
The order in which a quad lists its vertices does not matter."""
import ctypes

import numpy as np
import torch

from . import _lib
from .segmap_manager import _image_source, _stage_sources


def _extract_staged(stage, quads, counts, scales, patch_size, expand, return_quads, device, zero=True):
    """``ubd_extract_objects`` over the staged sources of ``segmap_manager._stage_sources``; quads (n, cap, 8) and counts (n)
    are int32 tensors on ``device``.  zero: slots that hold no object read as 0 (else they are left as allocated)."""
    base, offsets, hw, c, _ = stage
    n = len(offsets)
    if quads.dim() != 3 or quads.shape[0] != n or quads.shape[2] != 8 or tuple(counts.shape) != (n,):
        raise ValueError(f"quads must be ({n}, cap, 8) and counts ({n},), got {tuple(quads.shape)} and {tuple(counts.shape)}")
    cap = int(quads.shape[1])
    ph, pw = int(patch_size[0]), int(patch_size[1])
    src_bytes = int(max(int(o) + int(h) * int(w) * c for o, (h, w) in zip(offsets, hw)))
    offs_d = torch.from_numpy(offsets).to(device, non_blocking=True)
    hw_d = torch.from_numpy(hw).to(device, non_blocking=True)
    scales_d = None
    if scales is not None:
        if len(scales) != n:
            raise ValueError(f"one (xscale, yscale) per image is required, got {len(scales)} for {n} images")
        scales_d = torch.from_numpy(np.array([[float(s[0]), float(s[1])] for s in scales], np.float64)).to(device, non_blocking=True)
    patches = (torch.zeros if zero else torch.empty)((n, cap, ph, pw, c), dtype=torch.uint8, device=device)
    pq = (torch.zeros if zero else torch.empty)((n, cap, 8), dtype=torch.int32, device=device) if return_quads else None
    _lib.launch("ubd_extract_objects", device, ctypes.c_void_p(base), src_bytes, offs_d.data_ptr(), hw_d.data_ptr(), c, quads.data_ptr(),
                counts.data_ptr(), n, cap, None if scales_d is None else scales_d.data_ptr(), float(expand),
                patches.data_ptr(), ph, pw, None if pq is None else pq.data_ptr())
    return (patches, pq) if return_quads else patches


def extract_objects_on_device(sources, quads, counts, scales=None, patch_size=(64, 256), expand=1.0, return_quads=False):
    """One upright patch of ``patch_size`` = (patch_h, patch_w) per found object, in one launch.
    ``sources``: one image per row of ``quads`` -- PIL images (through ``.convert('RGB')``), HxW / HxWx1 / HxWx3 uint8 numpy
    arrays (staged through one pinned buffer and one transfer) or uint8 device tensors of those shapes (read in place); a grey
    image among RGB ones is replicated to three channels.  ``quads`` (n, cap, 8) and ``counts`` (n): int32, as the postprocess
    leaves them (device tensors are read where they lie; slots j >= min(counts[i], cap) are not read).  ``scales``: per image
    (xscale, yscale), e.g. the ``ResizeMeta`` list of ``rescale_images_on_device``, applied to the corners exactly as
    ``ModelRunner.rescale`` applies them; None: the quads are in the sources' coordinates already.  ``expand``: > 0, scales
    every quad about the mean of its corners (1.25 leaves a quiet zone around a code).
    Returns the uint8 device tensor (n, cap, patch_h, patch_w, c), zero in the slots that hold no object; with ``return_quads``
    also the int32 (n, cap, 8) corners NW, NE, SE, SW of every patch in source coordinates (rescaled, before expansion).
    Nothing is read back: the call enqueues on the current stream and returns."""
    _lib.require_gpu("extract_objects_on_device")
    if isinstance(quads, torch.Tensor) and quads.is_cuda:
        device = quads.device
    else:
        device = torch.device(f"cuda:{torch.cuda.current_device()}")
    srcs = [_image_source(im, device) for im in sources]
    if not srcs:
        raise ValueError("no images")
    quads = _lib.to_device(quads, torch.int32, device, non_blocking=True)
    counts = _lib.to_device(counts, torch.int32, device, non_blocking=True)
    return _extract_staged(_stage_sources(srcs, device), quads, counts, scales, patch_size, expand, return_quads, device)
