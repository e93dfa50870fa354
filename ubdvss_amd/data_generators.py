"""Batch generator of the training run -- host mirror of semantic_segmentation/data_generators.py:57-212 on top of
``SegmapManager.prepare_batches_on_device``.

The reference prepares ``prepare_batch_size`` images at a time in worker processes (read, augment, resize, label map, all on the
host), sorts them by size, groups equal shapes and cuts the groups into batches.  Here a chunk of names is read on the host and
goes through ONE ``prepare_batches_on_device`` call -- warps, photometric stages, resize and label maps on the MI355X -- and the
batches are cut from the device tensors it returns: a batch is ``(uint8 images (n, h, w, c), int32 targets (n, h/4, w/4, 1))`` on
the device.  Images stay raw uint8 pixels: ``NetConfig``'s preprocessing is fused into the network's first layer, the package's
rule for every entry point (the reference applies ``preprocessing_fn`` here, data_generators.py:148).

Built: the ``"BarcodeSegmap"`` reader (``markup_readers.SegmentationMapMarkupReader``), or any reader object handed in.  The XML
readers of the reference and a ``train.py`` command line are not built.
"""
import logging

import numpy as np
import torch

from .markup_readers import SegmentationMapMarkupReader
from .segmap_manager import SegmapManager

_READERS = {"BarcodeSegmap": SegmentationMapMarkupReader}      # markup_type name -> reader class; the one reader the package has
_READER_METHODS = ("read_markup", "get_list_of_images", "get_image_markup", "get_image")


class MetaInfo:
    """data_generators.py:42-55: what validation needs to know about an image beyond its pixels.  ``filename``: the image's name
    (of a ``(_, name)`` pair, the name); ``markup``: the markup on the ORIGINAL image, neither resized nor augmented;
    ``xscale`` = original width / resized width, ``yscale`` = original height / resized height -- the factors that take a found
    box back to the original (``ModelRunner.rescale``)."""

    def __init__(self, filename, original_markup, xscale, yscale):
        if isinstance(filename, (tuple, list)):
            filename = filename[1]
        self.filename, self.markup = filename, original_markup
        self.xscale, self.yscale = xscale, yscale


class _Prepared:
    """one prepared image: row ``row`` of a chunk's per-size device tensors"""
    __slots__ = ("images", "targets", "row", "shape", "size", "meta_info")

    def __init__(self, images, targets, row, meta_info):
        self.images, self.targets, self.row, self.meta_info = images, targets, row, meta_info
        self.shape = tuple(int(v) for v in images.shape[1:])
        self.size = int(np.prod(self.shape))


def _is_polygon(markup):
    return any(np.asarray(obj.bbox).size != 8 for obj in markup or [])


class BatchGenerator:
    """data_generators.py:57-212.  ``markup_type``: ``"BarcodeSegmap"``, or a reader instance with ``read_markup``,
    ``get_list_of_images``, ``get_image_markup`` and ``get_image`` (``path`` is then ignored; ``read_markup`` is called here as
    for a named reader).  ``photo_rng`` / ``photo_extended`` / ``photo_noise_alpha`` are handed to
    ``prepare_batches_on_device`` (the imgaug photometric stage, ubdvss_amd/augmentation.py).  There are no worker processes:
    the chunk's device work is one call.  A data set without images raises ValueError here, and a pass of ``generate`` that
    yields no batch at all raises RuntimeError there: an endless generator that never yields would hang its consumer."""

    def __init__(self, path, batch_size, markup_type, net_config, use_augmentation=False, yield_incomplete_batches=True,
                 prepare_batch_size=1000, name="TrainGenerator", photo_rng=None, photo_extended=False, photo_noise_alpha=False,
                 device=None):
        if int(batch_size) < 1 or int(prepare_batch_size) < 1:
            raise ValueError("batch_size and prepare_batch_size must be at least 1")
        self._batch_size = int(batch_size)
        self._net_config = net_config
        self._use_augmentation = bool(use_augmentation)
        self._name = name
        self._prepare_batch_size = int(prepare_batch_size)
        self._yield_incomplete_batches = bool(yield_incomplete_batches)
        self._photo = dict(photo_rng=photo_rng, photo_extended=photo_extended, photo_noise_alpha=photo_noise_alpha)
        self._device = device
        if isinstance(markup_type, str):
            if markup_type not in _READERS:
                raise ValueError(f"markup_type {markup_type!r} is not supported: the package reads {sorted(_READERS)} "
                                 "(or takes a reader instance); the XML readers of the reference are not built")
            self._reader = _READERS[markup_type](path, net_config, device=device)
        else:
            missing = [m for m in _READER_METHODS if not callable(getattr(markup_type, m, None))]
            if missing:
                raise ValueError(f"markup_type must be one of {sorted(_READERS)} or a reader instance; "
                                 f"{type(markup_type).__name__} has no {', '.join(missing)}")
            self._reader = markup_type
        reader = self._reader
        reader.read_markup()
        self._image_names = list(reader.get_list_of_images())
        if not self._image_names:
            raise ValueError(f"generator {name}: the reader found no image with markup"
                             + (f" under {path!r}" if isinstance(markup_type, str) else ""))
        logging.info("generator %s: %d images", name, len(self._image_names))

    def get_images_per_epoch(self):
        """the size of the data set"""
        return len(self._image_names)

    def get_epoch_size(self):
        """whole batches in one pass over the data set (the short last batch not counted)"""
        return len(self._image_names) // self._batch_size

    def is_augmentation_used(self):
        return self._use_augmentation

    def generate(self, add_metainfo=False):
        """Endless generator of ``(images, targets)`` or, with ``add_metainfo``, ``(images, targets, [MetaInfo])``.  A pass takes
        the names ``prepare_batch_size`` at a time (shuffled first under augmentation); a chunk's prepared images are ordered by
        element count (stable), runs of one shape are cut into batches of ``batch_size``, and a run's short tail is yielded or,
        with ``yield_incomplete_batches=False``, skipped.  Without augmentation a chunk that holds the whole data set is
        prepared once and served again on every later pass."""
        if add_metainfo and self._use_augmentation:
            raise AssertionError("MetaInfo describes the image as it was read; an augmented image has no such scales")
        kept = None                                                 # the one prepared chunk that is the whole data set
        while True:
            if self._use_augmentation:
                np.random.shuffle(self._image_names)
            n_batches = 0
            for start in range(0, len(self._image_names), self._prepare_batch_size):
                chunk = kept
                if chunk is None:
                    chunk = self._prepare_chunk(self._image_names[start:start + self._prepare_batch_size], add_metainfo)
                    chunk.sort(key=lambda p: p.size)
                    if not self._use_augmentation and len(chunk) == len(self._image_names):
                        kept = chunk
                        logging.info("generator %s keeps its %d prepared images for the passes to come", self._name, len(chunk))
                for run in self._runs_of_one_shape(chunk):
                    for first in range(0, len(run), self._batch_size):
                        part = run[first:first + self._batch_size]
                        if len(part) == self._batch_size or self._yield_incomplete_batches:
                            n_batches += 1
                            yield self._batch(part, add_metainfo)
            if n_batches == 0:
                raise RuntimeError(f"generator {self._name}: a whole pass over {len(self._image_names)} images gave no batch "
                                   "(every image failed, or no shape has batch_size images and incomplete batches are off)")

    @staticmethod
    def _runs_of_one_shape(chunk):
        """consecutive prepared images of equal shape, as lists"""
        runs = []
        for p in chunk:
            if runs and runs[-1][0].shape == p.shape:
                runs[-1].append(p)
            else:
                runs.append([p])
        return runs

    @staticmethod
    def _batch(part, add_metainfo):
        # consecutive items of one shape come from one per-size tensor of the chunk; rows are gathered (a copy: the kept chunk stays intact)
        pieces = [(p.images, p.targets) for p in part]
        if all(im is pieces[0][0] for im, _ in pieces):
            rows = torch.tensor([p.row for p in part], dtype=torch.int64, device=pieces[0][0].device)
            images, targets = pieces[0][0].index_select(0, rows), pieces[0][1].index_select(0, rows)
        else:                                                       # equal shapes from several prepare calls (images prepared one by one)
            images = torch.stack([p.images[p.row] for p in part])
            targets = torch.stack([p.targets[p.row] for p in part])
        targets = targets.unsqueeze(-1)
        if add_metainfo:
            return images, targets, [p.meta_info for p in part]
        return images, targets

    def _prepare(self, images, markups):
        return SegmapManager.prepare_batches_on_device(images, markups, self._net_config, augment=self._use_augmentation,
                                                       device=self._device, **self._photo)

    def _skip(self, image_name, error):
        logging.error("generator %s leaves out image %s: %s", self._name, image_name, error)

    def _prepare_chunk(self, chunk_names, with_meta):
        """A chunk of names -> the list of prepared images, in the order of the names.  An image that cannot be read, or that the
        device chain refuses, is logged and left out (data_generators.py:192-194)."""
        names, images, markups = [], [], []
        for image_name in chunk_names:
            try:
                image, markup = self._reader.get_image(image_name), self._reader.get_image_markup(image_name)
            except Exception as e:                                  # noqa: BLE001
                self._skip(image_name, e)
                continue
            if self._use_augmentation and _is_polygon(markup):
                # a property of the data set and the run's settings, not one bad file: let prepare_batches_on_device's refusal
                # surface, with the file's name
                try:
                    self._prepare([image], [markup])
                except ValueError as e:
                    raise ValueError(f"{e} [image '{image_name}' of generator {self._name}]") from None
            names.append(image_name)
            images.append(image)
            markups.append(markup)
        if not names:
            return []
        try:
            results = [(list(range(len(names))), self._prepare(images, markups))]
        except Exception as e:                                      # noqa: BLE001 -- find the image(s) at fault: one call per image
            logging.error("generator %s: preparing %d images in one call failed (%s); taking them one by one", self._name, len(names), e)
            results = []
            for k in range(len(names)):
                try:
                    results.append(([k], self._prepare([images[k]], [markups[k]])))
                except Exception as e1:                             # noqa: BLE001
                    self._skip(names[k], e1)
        out = [None] * len(names)
        for positions, groups in results:
            for idx, x, labels, _, _ in groups:
                for row, i in enumerate(idx):
                    k = positions[i]
                    meta = None
                    if with_meta:
                        original_w, original_h = images[k].size if hasattr(images[k], "size") and not hasattr(images[k], "shape") \
                            else (int(images[k].shape[1]), int(images[k].shape[0]))
                        meta = MetaInfo(names[k], markups[k], original_w / int(x.shape[2]), original_h / int(x.shape[1]))
                    out[k] = _Prepared(x, labels, row, meta)
        return [p for p in out if p is not None]
