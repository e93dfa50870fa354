"""Ground truth read from segmentation maps -- host mirror of SegmentationMapMarkupReader
(semantic_segmentation/markup_readers.py:257-285).

The reference reads the public barcode data sets this way: the map image -> ``findContours(RETR_EXTERNAL)`` -> ``cv2.convexHull`` of
every contour -> ``ClassifiedObjectMarkup(hull, 5)`` (every object is an EAN13 there).  Here the components, their hulls and the
order of the list come from ``ubd_segmap_polygons`` (include/ubd.h) on the MI355X, for a whole batch of maps at once; there is
no CPU path.  Parity with cv2 itself is unpinned, as for the rest of the postprocess.

Deviation: the reference drops hulls of one point and keeps hulls of two (a straight one-pixel line), which then fail inside
shapely when they are evaluated.  Here hulls with fewer than 3 vertices are dropped, and counted in a log line.
"""
import collections
import logging
import os

import numpy as np
from PIL import Image

from . import _lib
from .data_markup import ClassifiedObjectMarkup

IMAGE_EXTENSIONS = ('.jpg', '.jpeg', '.png', '.bmp', '.tif', '.tiff', '.gif')
_MAX_OBJECTS = _lib.UBD_EVAL_MAX_GT
_MAX_VERTS = _lib.UBD_POLY_MAX_VERTS


def _segmap_polygons_device(maps, device=None):
    """One ubd_segmap_polygons call: uint8 (n, h, w) array or tensor -> host int32 arrays verts (n, cap, 64, 2), nverts (n, cap),
    counts (n)."""
    torch = _lib.require_gpu("ubdvss_amd.markup_readers")
    lib = _lib.load()
    device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
    if not torch.is_tensor(maps):
        maps = torch.from_numpy(np.ascontiguousarray(maps))
    if maps.dim() != 3 or maps.dtype != torch.uint8:
        raise ValueError(f"segmentation maps must be a uint8 (n, h, w) array, got {tuple(maps.shape)} {maps.dtype}")
    maps = maps.to(device).contiguous()
    n, h, w = (int(v) for v in maps.shape)
    cap = _MAX_OBJECTS
    need = int(lib.ubd_segmap_polygons_workspace_bytes(n, h, w, cap))
    if need == 0:
        raise ValueError(f"segmentation maps outside the limits: n={n} h={h} w={w} (n >= 1, sides 1..32767, n * h * w < 2^31)")
    ws = torch.empty(need, dtype=torch.uint8, device=device)
    verts = torch.zeros((n, cap, _MAX_VERTS, 2), dtype=torch.int32, device=device)
    nverts = torch.zeros((n, cap), dtype=torch.int32, device=device)
    counts = torch.zeros((n,), dtype=torch.int32, device=device)
    _lib.launch("ubd_segmap_polygons", device, maps.data_ptr(), n, h, w, verts.data_ptr(), nverts.data_ptr(), counts.data_ptr(), cap,
                ws.data_ptr(), need)
    return verts.cpu().numpy(), nverts.cpu().numpy(), counts.cpu().numpy()


def _markup_from_arrays(verts, nverts, counts, object_type=5, image_offset=0):
    """The host half of ``segmap_polygons``: the arrays of ubd_segmap_polygons -> (per image a list of ClassifiedObjectMarkup
    with a flat int bbox x1, y1, ..., number of hulls dropped for having fewer than 3 vertices).  ValueError for a truncated
    list or a hull of more than 64 vertices, naming the image and the object."""
    cap = int(nverts.shape[1])
    out, dropped = [], 0
    for i in range(len(counts)):
        found = int(counts[i])
        if found > cap:
            raise ValueError(f"segmentation map of image {image_offset + i}: {found} objects, the limit is {cap}")
        objs = []
        for o in range(found):
            k = int(nverts[i, o])
            if k > _MAX_VERTS:
                raise ValueError(f"segmentation map of image {image_offset + i}, object {o}: its hull has {k} vertices, the limit is "
                                 f"{_MAX_VERTS} (a round blob is not a barcode outline)")
            if k < 3:
                dropped += 1
                continue
            objs.append(ClassifiedObjectMarkup(np.asarray(verts[i, o, :k], dtype=np.int64).reshape(-1).astype(int), object_type))
        out.append(objs)
    return out, dropped


def segmap_polygons(maps, object_type=5, device=None):
    """Segmentation maps -> ground-truth markup.  maps: uint8 array or tensor (n, h, w), foreground is a byte that is not 0.
    Returns, per image, a list of ``ClassifiedObjectMarkup(hull, object_type)``: one convex hull (flat ints x1, y1, ..., 3..64
    vertices, in map pixels) per external 8-connected component, in the order and with the vertex cycle of
    ``ubd_segmap_polygons``.  Hulls with fewer than 3 vertices (single pixels, straight one-pixel lines) are dropped and
    counted in a log line.  ValueError for a hull of more than 64 vertices or more than 256 objects in one map."""
    markup, dropped = _markup_from_arrays(*_segmap_polygons_device(maps, device), object_type=object_type)
    if dropped:
        logging.info("segmentation maps: %d component(s) with a hull of fewer than 3 vertices dropped", dropped)
    return markup


def _is_image_extension(ext):
    return ext.lower() in IMAGE_EXTENSIONS


class SegmentationMapMarkupReader:
    """The reference's reader for data sets whose markup is a folder of segmentation maps (markup_readers.py:257-285), with its
    interface: ``read_markup``, ``get_list_of_images``, ``get_image_markup``, ``get_image``.  Images are named by the markup
    file's name without its extension.  A host shell: the files are opened with Pillow (``convert('L')``), the maps are grouped by
    size and every group is one device call (several for a large group)."""
    OBJECT_TYPE = 5                                  # EAN13: the one type of the public data sets (markup_readers.py:260)

    def __init__(self, path, net_config, images_folder='Image', markup_folder='Detection', device=None):
        self._path = path
        self._net_config = net_config
        self._images_folder_path = os.path.join(path, images_folder)
        self._markup_folder_path = os.path.join(path, markup_folder)
        self._device = device
        self._markup = dict()
        self._full_filename = dict()

    def _find_corresponding_image(self, fname):
        for image_file in sorted(os.listdir(self._images_folder_path)):
            name, ext = os.path.splitext(image_file)
            if name == fname and _is_image_extension(ext):
                return image_file
        raise ValueError("Image corresponding to fname {} not found (skipping markup)".format(fname))

    def read_markup(self):
        n_errors = 0
        logging.info("Reading markup from {}".format(self._images_folder_path))
        groups = collections.OrderedDict()           # (h, w) -> [(name, map)]
        for markup_filename in sorted(os.listdir(self._markup_folder_path)):
            fname, ext = os.path.splitext(markup_filename)
            if not _is_image_extension(ext):
                continue
            try:
                image_filename = self._find_corresponding_image(fname)
                seg_map = np.asarray(Image.open(os.path.join(self._markup_folder_path, markup_filename)).convert('L'), dtype=np.uint8)
                groups.setdefault(seg_map.shape, []).append((fname, image_filename, seg_map))
            except Exception as e:                   # the reference logs and goes on (markup_readers.py:131-133)
                n_errors += 1
                logging.error("{} can't read {}".format(n_errors, e))
        n_read = 0
        for (h, w), group in groups.items():
            step = max(1, min(64, (1 << 26) // (h * w)))          # maps per device call: bounds the call's workspace
            chunks = [group[k:k + step] for k in range(0, len(group), step)]
            markup = [objs for c in chunks for objs in segmap_polygons(np.stack([m for _, _, m in c]), self.OBJECT_TYPE, self._device)]
            for (fname, image_filename, _), objs in zip(group, markup):
                self._markup[fname] = objs
                self._full_filename[fname] = image_filename
                n_read += 1
        logging.info("{}/{} files read successfully".format(n_read, n_read + n_errors))

    def get_list_of_images(self):
        return list(self._markup.keys())

    def get_image_markup(self, image_name):
        return self._markup[image_name]

    def get_image(self, image_name):
        return Image.open(os.path.join(self._images_folder_path, self._full_filename[image_name])).convert('RGB')
