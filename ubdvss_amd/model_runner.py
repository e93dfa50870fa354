"""ModelRunner.predict -- host mirror of semantic_segmentation/model_runner.py:31-38, :105-148.

The reference runs ``model.predict`` on the device, then thresholds with numpy and calls
``SegmapManager.postprocess`` (OpenCV) image by image on the host.  Here the forward pass, the
threshold, the component labelling and the box fitting all run on the MI355X; only the final
(count, quads, classes) lists cross PCIe.
"""
import os

import numpy as np
import torch

from . import _lib, utils
from .data_markup import ObjectMarkup, ClassifiedObjectMarkup


class ModelRunner:
    def __init__(self, net_config, pixel_threshold=0.5, max_objects_per_image=256, pipelined=False, slots=2):
        """model_runner.py:31-38: pixel_probability > pixel_threshold is positive.
        pipelined=True: the postprocess of batch k is enqueued together with the forward pass of batch k+1 -- inside the
        first blocks of that pass's stem kernel (ubd_forward_postprocess), on the same stream, without events.  The result
        tensors a call returns are therefore COMPLETE only after the next call (or ``flush()``) has been enqueued and the
        stream has been waited for; ``synchronize()`` does both.  Logits / results are double-buffered: they stay valid until
        the second call after the one that returned them (``slots`` = 3: until the third -- ``predict_stream`` copies a batch's
        results to the host while the next two batches are in flight)."""
        self._net_config = net_config
        eps = 1e-9
        self._logit_threshold = - np.log(1 / np.clip(pixel_threshold, eps, 1 - eps) - 1)
        self._cap = max_objects_per_image
        self._pipelined = pipelined
        self._nslots = max(2, int(slots))
        self._slots = {}
        self._step = 0
        self._pending = None            # (model, slot): logits whose postprocess has not been enqueued yet

    def _job(self, slot):
        return {"logits": slot["logits"], "logit_threshold": self._logit_threshold, "scale": self._net_config.get_scale(),
                "min_area": self._net_config.get_min_pixels_for_detection(), "cap": self._cap, "outputs": slot["out"]}

    def flush(self):
        """Enqueues the postprocess that is still owed (the last batch's), as a launch of its own on the current stream."""
        if self._pending is not None:
            model, slot = self._pending
            self._pending = None
            job = self._job(slot)
            model.postprocess_on_device(job["logits"], job["logit_threshold"], job["scale"], job["min_area"], cap=job["cap"],
                                        outputs=job["outputs"])

    def synchronize(self):
        """All results returned so far are complete after this."""
        model = self._pending[0] if self._pending is not None else None
        self.flush()
        torch.cuda.current_stream(model.device if model is not None else None).synchronize()

    @property
    def logit_threshold(self):
        return self._logit_threshold

    def predict_on_device(self, model, images):
        """images: device tensor (N,H,W,C).  Returns device tensors
        (logits, binary_map (N,h,w) int32, quads (N,cap,8), classes or None, counts (N))."""
        scale = self._net_config.get_scale()
        min_area = self._net_config.get_min_pixels_for_detection()
        if not self._pipelined:
            logits = model.predict_on_device(images)
            bmap, quads, classes, counts = model.postprocess_on_device(logits, self._logit_threshold, scale, min_area, cap=self._cap)
            return logits, bmap, quads, classes, counts
        # ---- pipeline on ONE stream: this call = forward(batch k+1) + postprocess(batch k) in the same launches
        n, hh, ww, _ = images.shape
        key = (self._step % self._nslots, n, hh, ww, id(model))
        self._step += 1
        slot = self._slots.get(key)
        if slot is None:
            slot = {"logits": torch.empty((n, hh // 4, ww // 4, model.k_out), dtype=torch.float32, device=model.device),
                    "out": model.alloc_postprocess_outputs(n, hh // 4, ww // 4, self._cap)}
            self._slots[key] = slot
        if self._pending is not None and (self._pending[0] is not model or self._pending[1] is slot):
            self.flush()                                # another model's logits (its own handle), or the slot about to be overwritten
        job = self._job(self._pending[1]) if self._pending is not None else None
        logits = model.predict_on_device(images, out=slot["logits"], postprocess=job)
        self._pending = (model, slot)
        bmap, quads, classes, counts = slot["out"]
        return logits, bmap, quads, classes, counts

    def evaluate_batches(self, model, batches, average_precision=False):
        """The device form of the evaluation loop of ModelRunner.run (model_runner.py:60-75, :102): for every
        (images, gt_objects, meta_infos) batch the forward pass, the postprocess and the object-level evaluation
        (ubd_evaluate_objects) are enqueued on the current stream -- the found objects never leave the device; the quads are
        rescaled to the original images there with meta.xscale / meta.yscale (meta_infos may be None: no rescale) -- and
        the ``scalar_logs`` of DatasetMetricCalculator.get_metrics are returned after ONE read of the device sums.
        images: (N,H,W,C) numpy array or device tensor; gt_objects: per image a list of markup records.
        A batch may also be (images, gt_objects, meta_infos, gt_segmap), gt_segmap the label maps (N,h,w) or (N,h,w,1) int32
        (device tensor or numpy, e.g. of ``prepare_batch_on_device``): on a classification config the logits the forward pass
        just wrote are then scored in place (ubd_evaluate_pixels) and the two pixel accuracies join the result.
        average_precision=True: every found object is also given its confidence (ubd_score_objects) and every batch is ranked
        behind its evaluation (ubd_rank_detections), all on the device; the result gains ``ap_iou*`` and ``map``
        (DatasetMetricCalculator.get_average_precision) and keeps every other key and value."""
        from .evaluation import DatasetMetricCalculator
        evaluator = DatasetMetricCalculator(self._net_config, average_precision=average_precision)
        for batch in batches:
            images, gt_objects, meta_infos = batch[:3]
            gt_segmap = batch[3] if len(batch) > 3 else None
            if not torch.is_tensor(images):
                x = np.asarray(images)
                if x.dtype != np.uint8:
                    x = x.astype(np.float32, copy=False)
                images = torch.from_numpy(np.ascontiguousarray(x))
            images = images.to(model.device)
            if meta_infos is not None and len(meta_infos) != len(images):
                raise AssertionError("one meta_info per image is required")
            logits, _, quads, classes, counts = self.predict_on_device(model, images)
            self.flush()                                # pipelined runner: this batch's postprocess before its evaluation
            scales = None if meta_infos is None else np.array([[m.xscale, m.yscale] for m in meta_infos], dtype=np.float64)
            scores = model.score_objects_on_device(logits, quads, counts, self._net_config.get_scale()) if average_precision else None
            evaluator.evaluate_batch(gt_objects, (quads, classes, counts), gt_segmap=gt_segmap,
                                     classification_logits=logits if gt_segmap is not None else None,
                                     meta_infos=meta_infos, scales=scales, scores=scores)
        return evaluator.get_metrics()

    def run(self, model, batches, n_images, save_dir=None, save_visualizations=False, rng=None, average_precision=False):
        """The contract of the reference's ModelRunner.run (model_runner.py:40-103): metrics, saved results and visualisations
        of up to ``n_images`` images.  ``batches``: an iterable of batches in the form ``evaluate_batches`` takes,
        (images, gt_objects, meta_infos[, gt_segmap]); it is read until ``n_images`` images have been seen (or it ends).  Per
        batch the forward pass, the postprocess, the evaluation and -- where a batch is drawn -- the four overlays
        (ubd_visualize_images) run on the device; the found objects are drawn in the coordinates of the images given and scored
        in the originals' (meta.xscale / meta.yscale).  gt_segmap may be a host array: it is uploaded once per use.
        Without ``save_dir`` the one batch that holds a randomly drawn image index is visualised; the index comes from ``rng``, a
        numpy.random.Generator (unseeded when None, as the reference's np.random.randint).  With ``save_dir`` (then meta_infos
        are required: they name the files) the ground truth and the found objects of every image are written as CSV and, with
        ``save_visualizations``, every image is saved into the folders of its ImageResultCategories at ERROR_IOU_THRESHOLD.
        Returns (scalar_logs, visualizations): the dict of ``get_metrics`` and the last batch drawn as {'gt' (with label maps),
        'seg_map', 'postprocessed'[, 'classification_gt']} of device uint8 tensors (N, H, W, 3) ({} when none was drawn).
        average_precision=True: the objects are scored and every batch ranked on the device as in ``evaluate_batches``; the
        logs gain ``ap_iou*`` and ``map``."""
        from .evaluation import DatasetMetricCalculator, ImageResultCategories
        from .result_saver import ResultSaver
        from .visualizations import Visualizer
        metrics = DatasetMetricCalculator(self._net_config, average_precision=average_precision)
        writer = ResultSaver(save_dir, save_visualizations)
        generator = np.random.default_rng() if rng is None else rng
        preview_index = int(generator.integers(0, n_images))       # drawn even when save_dir makes it unused: one draw per run
        drawn = {}
        first = 0                                                   # index of the batch's first image in the run
        for batch in batches:
            if first >= n_images:
                break
            images, gt_objects, meta_infos = batch[:3]
            labels = batch[3] if len(batch) > 3 else None
            if save_dir and meta_infos is None:
                raise AssertionError("save_dir needs meta_infos: they name the files")
            if meta_infos is not None and len(meta_infos) != len(images):
                raise AssertionError("one meta_info per image is required")
            x = self._batch_to_device(model, images)
            logits, binary_map, quads, classes, counts = self.predict_on_device(model, x)
            self.flush()                                # pipelined runner: this batch's postprocess before its evaluation
            scales = None if meta_infos is None else np.array([[m.xscale, m.yscale] for m in meta_infos], dtype=np.float64)
            scores = model.score_objects_on_device(logits, quads, counts, self._net_config.get_scale()) if average_precision else None
            records, mask = metrics.evaluate_batch(gt_objects, (quads, classes, counts), gt_segmap=labels,
                                                   classification_logits=logits if labels is not None else None,
                                                   meta_infos=meta_infos, scales=scales, scores=scores)
            folders = None
            if save_dir:
                writer.save_gt_and_prediction(gt_objects, self.rescale(self._found_lists(quads, classes, counts), meta_infos), meta_infos)
                folders = ImageResultCategories.get_batch_categories(records)
                draw_it = bool(save_visualizations) and any(len(f) > 0 for f in folders)
            else:
                draw_it = first <= preview_index < first + len(x)
            if draw_it:
                drawn = Visualizer.compute_visualizations_on_device(x, labels, binary_map, (quads, counts), mask,
                                                                    preprocessing=self._net_config.get_preprocessing_type())
                if folders is not None:
                    writer.save_visualizations(folders, meta_infos, drawn)
            first += len(x)
        return metrics.get_metrics(), drawn

    @staticmethod
    def _batch_to_device(model, images):
        """a batch as ``predict`` takes it (numpy or tensor; uint8 raw pixels, anything else float32) on the model's device"""
        if not torch.is_tensor(images):
            x = np.asarray(images)
            if x.dtype != np.uint8:
                x = x.astype(np.float32, copy=False)
            images = torch.from_numpy(np.ascontiguousarray(x))
        return images.to(model.device)

    def _found_lists(self, quads, classes, counts):
        """device results -> host object lists (one read of each tensor); raises when an image overflowed the capacity"""
        counts_h = counts.cpu().numpy()
        if (counts_h > self._cap).any():
            raise RuntimeError(f"more than max_objects_per_image={self._cap} objects in an image "
                               f"(max found {int(counts_h.max())}); raise the capacity")
        return self._object_lists(counts_h, quads.cpu().numpy(), classes.cpu().numpy() if classes is not None else None)

    def predict(self, model, images, rescale=False, meta_infos=None):
        """Same contract as the reference (model_runner.py:105-138): returns
        (detection map (N,h,w,1) of {0,1}, classification_logits (N,h,w,n_cls), found_objects)."""
        assert not rescale or (meta_infos is not None and len(images) == len(meta_infos))
        x = np.asarray(images)
        if x.dtype != np.uint8:
            x = x.astype(np.float32, copy=False)        # no second 100-MB host copy when the batch is float32 already
        # float images arrive already preprocessed, as in the reference; uint8 images are raw pixels and take the
        # NetConfig preprocessing fused into the first layer (one rule for every entry point)
        xt = torch.from_numpy(np.ascontiguousarray(x)).to(model.device)
        logits, bmap, quads, classes, counts = self.predict_on_device(model, xt)
        self.flush()                                    # pipelined runner: this batch's postprocess now, the copies below wait for it
        return self._assemble(counts.cpu().numpy(), quads.cpu().numpy(), classes.cpu().numpy() if classes is not None else None,
                              logits.cpu().numpy(), bmap.cpu().numpy(), rescale, meta_infos)

    def predict_scored(self, model, images, rescale=False, meta_infos=None, min_score=None):
        """``predict`` plus the confidence of every found object (no reference counterpart): returns ``predict``'s triple and
        ``scores``, per image a float32 array in the order of ``found_objects[i]`` -- the mean detection probability over the
        map pixels of the found box (``Model.score_objects_on_device``; the box, not the component's filled contour).  The scores
        travel beside the markup records, not inside them.  ``min_score``: objects (and scores) below it are dropped, on the host.
        A pipelined runner is flushed before the objects are scored."""
        assert not rescale or (meta_infos is not None and len(images) == len(meta_infos))
        x = np.asarray(images)
        if x.dtype != np.uint8:
            x = x.astype(np.float32, copy=False)
        xt = torch.from_numpy(np.ascontiguousarray(x)).to(model.device)
        logits, bmap, quads, classes, counts = self.predict_on_device(model, xt)
        self.flush()                                    # pipelined runner: this batch's postprocess before its objects are scored
        scores_h = model.score_objects_on_device(logits, quads, counts, self._net_config.get_scale()).cpu().numpy()
        counts_h = counts.cpu().numpy()
        det, cls_logits, found = self._assemble(counts_h, quads.cpu().numpy(), classes.cpu().numpy() if classes is not None else None,
                                                logits.cpu().numpy(), bmap.cpu().numpy(), rescale, meta_infos)
        scores = [np.array(scores_h[i, :int(counts_h[i])]) for i in range(len(counts_h))]
        if min_score is not None:
            keep = [s >= min_score for s in scores]
            found = [[o for o, k in zip(objs, kept) if k] for objs, kept in zip(found, keep)]
            scores = [s[k] for s, k in zip(scores, keep)]
        return det, cls_logits, found, scores

    def _assemble(self, counts_h, quads_h, classes_h, logits_h, bmap_h, rescale, meta_infos, copy=False):
        """Host arrays -> the reference's return triple (model_runner.py:121-138).  copy: the arrays are reused staging buffers."""
        if (counts_h > self._cap).any():
            raise RuntimeError(f"more than max_objects_per_image={self._cap} objects in an image "
                               f"(max found {int(counts_h.max())}); raise the capacity")
        detection_logits = bmap_h.astype(np.int64)[..., None]
        classification_logits = np.array(logits_h[..., 1:]) if copy else logits_h[..., 1:]
        found_objects = self._object_lists(counts_h, quads_h, classes_h)
        if rescale:
            found_objects = self.rescale(found_objects, meta_infos)
        return detection_logits, classification_logits, found_objects

    def _object_lists(self, counts_h, quads_h, classes_h):
        with_cls = self._net_config.is_classification_supported()
        found_objects = []
        for i in range(len(counts_h)):
            n = int(counts_h[i])
            boxes = quads_h[i, :n].astype(int)              # one conversion per image (a fresh array: the rows are views of it)
            if with_cls:
                found_objects.append([ClassifiedObjectMarkup(boxes[j], classes_h[i, j]) for j in range(n)])
            else:
                found_objects.append([ObjectMarkup(boxes[j]) for j in range(n)])
        return found_objects

    def predict_images(self, model, images, batch_size=None):
        """Raw images of any sizes -> found objects in ORIGINAL-image coordinates, in input order: the lists the reference's
        ``run`` evaluates (model_runner.py:65-72) after its host chain reader -> resize -> convert('L') -> predict -> rescale.
        ``images``: PIL images, HxW / HxWx3 uint8 numpy arrays or uint8 device tensors (SegmapManager.rescale_images_on_device).
        The images are grouped by ``SegmapManager.target_size`` (the reference batches by resized shape,
        data_generators.py:133-140); per group (and per ``batch_size`` images of it) they are resized on the device
        (ubd_resize_images, Pillow's BICUBIC bit for bit) and fed as uint8 to ``predict_on_device`` (the NetConfig
        preprocessing fused into the first layer); the boxes are scaled back by the MetaInfo scales (``rescale``)."""
        _lib.require_gpu("ModelRunner.predict_images")
        return self._predict_images(model, images, batch_size, None)[0]

    def predict_patches(self, model, images, patch_size=(64, 256), expand=1.0, batch_size=None):
        """``predict_images`` plus what a decoder wants of every found object: one upright uint8 patch of ``patch_size`` =
        (patch_h, patch_w), sampled from the ORIGINAL frame (``ubd_extract_objects``: Pillow's Image.transform(size, QUAD, data,
        BILINEAR) bit for bit; the orientation rule and ``expand`` as in ``object_patches.extract_objects_on_device``).
        Grouping and chain of ``predict_images``; the raw sources of a group are staged ONCE and the same device bytes feed the
        resize and then the extraction, with the group's ``ResizeMeta`` scales.  Returns (found, patches): ``found`` is exactly
        ``predict_images``' result, ``patches[k]`` a uint8 host array (len(found[k]), patch_h, patch_w, c) in the order of
        ``found[k]`` (c = 3 unless every image of the group is grey).  One device-to-host copy of the patches per group."""
        _lib.require_gpu("ModelRunner.predict_patches")
        return self._predict_images(model, images, batch_size, (int(patch_size[0]), int(patch_size[1]), float(expand)))

    def predict_decoded(self, model, images, patch_size=(64, 256), expand=1.25, batch_size=None, **params):
        """``predict_images`` plus the digits of every found object that is an EAN-13, UPC-A or EAN-8 symbol: the patches of
        ``predict_patches`` stay on the device and are decoded there (``barcode_decoder.decode_patches_on_device``; ``params``
        are its keywords).  ``expand`` 1.25 leaves the quiet zone around a tightly found code.  Returns (found, decoded):
        ``found`` is exactly ``predict_images``' result, ``decoded[k][j]`` a ``DecodedBarcode`` or None for ``found[k][j]``.
        The only extra read per group is the int32 result tensor (n, fullest list of the group, 16).
        With bit 2 of ``symbologies`` (``barcode_decoder.CODE128``; 7 reads every family) the same device patches also go through
        ``decode_text_patches_on_device``, the retail kernel running only if bit 0 or 1 is set: ``decoded[k][j]`` is the retail
        record if there is one, else the ``DecodedText``, else None, and the uint8 results (n, fullest list, 128) are read too.
        Bits 3 and 4 (``barcode_decoder.ITF``, ``CODE39``; 31 reads every family) add ``decode_width_patches_on_device`` in the
        same way: every requested kernel is launched before the first result is read, and ``decoded[k][j]`` is the retail record,
        else the ``DecodedText``, else the ``DecodedWidth``, else None.  Bits 6, 7 and 8 (``UPCE``, ``CODE93``, ``CODABAR``) are
        further symbologies of the retail, the text and the two-width kernel, so 479 reads every run-width code.  Bits 10..13
        (``POSTNET``, ``PLANET``, ``RM4SCC``, ``KIX``; ``POSTAL_SYMBOLOGIES`` = 15360) add ``decode_postal_patches_on_device`` in
        the same way, one more launch and one more read of (n, fullest list, 128) bytes per group: a ``DecodedPostal`` is taken
        where the older families gave None, and 479 | 15360 reads every linear code.  Bit 15 (``DATAMATRIX`` = 32768) adds
        ``decode_matrix_patches_on_device`` in the same way, a fifth launch before any read: a ``DecodedMatrix`` is taken where
        the older families gave None.  A Data Matrix is square and its kernel takes patch sides of 32..128, so a call with bit 15
        wants ``patch_size=(128, 128)`` (a ValueError beyond 128); a mask without the bit launches and reads what it did before.
        Bits 5, 9 and 14 are unassigned: they and every bit beyond 15 are a ValueError."""
        _lib.require_gpu("ModelRunner.predict_decoded")
        from .barcode_decoder import make_params
        symbologies = make_params(**params).symbologies     # an unknown keyword fails before any work
        if symbologies & ~(479 | 15360 | 32768):
            raise ValueError(f"symbologies {symbologies}: bits 0..4, 6..8, 10..13 and 15 (EAN-13, EAN-8, Code 128, ITF, Code 39; UPC-E, Code 93, "
                             "Codabar; POSTNET, PLANET, RM4SCC, KIX; Data Matrix) are the known symbologies, 479 | 15360 | 32768 in all; "
                             "bits 5, 9 and 14 are unassigned")
        if symbologies & 32768 and not (32 <= int(patch_size[0]) <= 128 and 32 <= int(patch_size[1]) <= 128):
            raise ValueError(f"patch_size {tuple(patch_size)}: the Data Matrix decoder (bit 15) takes patch sides of 32..128; use (128, 128)")
        return self._predict_images(model, images, batch_size, (int(patch_size[0]), int(patch_size[1]), float(expand)), decode=params)

    def _predict_images(self, model, images, batch_size, patch, decode=None):
        """The loop of ``predict_images``; patch = (patch_h, patch_w, expand): also the patches of ``predict_patches``, else None;
        decode = the decoder's keywords: the patches are decoded on the device and the records returned in their place."""
        from .object_patches import _extract_staged
        from .segmap_manager import SegmapManager, ResizeMeta
        groups = {}
        for k, im in enumerate(images):
            if isinstance(im, torch.Tensor) or isinstance(im, np.ndarray):
                h, w = int(im.shape[0]), int(im.shape[1])
            else:
                w, h = im.size
            groups.setdefault(SegmapManager.target_size(w, h, self._net_config), []).append(k)
        found = [None] * len(images)
        patches = [None] * len(images) if patch else None
        for idx in groups.values():
            step = len(idx) if not batch_size else int(batch_size)
            for b0 in range(0, len(idx), step):
                part = idx[b0:b0 + step]
                # the staged raw sources stay: the extraction reads the same device bytes the resize read
                x, sizes, stage = SegmapManager._rescale_images_staged([images[k] for k in part], self._net_config, model.device)
                metas = [ResizeMeta(w / int(x.shape[2]), h / int(x.shape[1])) for w, h in sizes]
                _, _, quads, classes, counts = self.predict_on_device(model, x)
                self.flush()                            # pipelined runner: this batch's postprocess now, the copies below wait for it
                counts_h = counts.cpu().numpy()
                if (counts_h > self._cap).any():
                    raise RuntimeError(f"more than max_objects_per_image={self._cap} objects in an image "
                                       f"(max found {int(counts_h.max())}); raise the capacity")
                objs = self._object_lists(counts_h, quads.cpu().numpy(), classes.cpu().numpy() if classes is not None else None)
                for k, o in zip(part, self.rescale(objs, metas)):
                    found[k] = o
                if patch:
                    ph, pw, expand = patch
                    most = int(counts_h.max())
                    on_device = None
                    if most:                            # the patch tensor holds the fullest list of the group, not the capacity
                        on_device = _extract_staged(stage, quads[:, :most].contiguous(), counts, metas, (ph, pw), expand, False,
                                                    model.device, zero=False)
                    if decode is not None:              # the patches stay on the device: one read of (n, most, 16) integers
                        records = self._decode_records(on_device, counts, counts_h, decode) if most else [[] for _ in part]
                        for j, k in enumerate(part):
                            patches[k] = records[j]
                        continue
                    host = on_device.cpu().numpy() if most else np.zeros((len(part), 0, ph, pw, stage[3]), np.uint8)
                    for j, k in enumerate(part):
                        patches[k] = np.array(host[j, :len(found[k])])
        return found, patches

    @staticmethod
    def _decode_records(on_device, counts, counts_h, decode):
        """the records of one group's device patches; bits 2 and 7 of ``symbologies`` add the text kernel on the same patches,
        bits 3, 4 and 8 the two-width kernel, bits 10..13 the postal kernel, bit 15 the Data Matrix kernel"""
        from .barcode_decoder import decode_patches_on_device, results_to_records, decode_text_patches_on_device, \
            text_results_to_records, decode_width_patches_on_device, width_results_to_records, decode_postal_patches_on_device, \
            postal_results_to_records, decode_matrix_patches_on_device, matrix_results_to_records, DEFAULT_PARAMS, EAN13, EAN8, \
            CODE128, ITF, CODE39, UPCE, CODE93, CODABAR, POSTAL_SYMBOLOGIES, MATRIX_SYMBOLOGIES
        symbologies = int(decode.get("symbologies", DEFAULT_PARAMS["symbologies"]))
        if not symbologies & (CODE128 | CODE93 | ITF | CODE39 | CODABAR | POSTAL_SYMBOLOGIES | MATRIX_SYMBOLOGIES):
            return results_to_records(decode_patches_on_device(on_device, counts, **decode), counts_h)
        launched = []                                   # every kernel is launched before the first result is read
        for bits, launch, to_records in (((EAN13 | EAN8 | UPCE), decode_patches_on_device, results_to_records),
                                         ((CODE128 | CODE93), decode_text_patches_on_device, text_results_to_records),
                                         ((ITF | CODE39 | CODABAR), decode_width_patches_on_device, width_results_to_records),
                                         (POSTAL_SYMBOLOGIES, decode_postal_patches_on_device, postal_results_to_records),
                                         (MATRIX_SYMBOLOGIES, decode_matrix_patches_on_device, matrix_results_to_records)):
            if symbologies & bits:
                launched.append((launch(on_device, counts, **dict(decode, symbologies=symbologies & bits)), to_records))
        records = None
        for results, to_records in launched:            # in the order of preference: retail, text, two-width, postal, Data Matrix
            more = to_records(results, counts_h)
            records = more if records is None else [[a if a is not None else b for a, b in zip(ra, rb)] for ra, rb in zip(records, more)]
        return records

    def predict_stream(self, model, batches, rescale=False, meta_infos=None, copy_threads=8):
        """The loop of the reference's ``ModelRunner.run`` (model_runner.py:60-67: ``predict`` batch after batch) as ONE pipeline:
        generator over ``predict``'s return triple, one per batch of ``batches`` (an iterable of numpy (N,H,W,C) arrays, uint8 or
        float32), in order.  Batch k + 1 is staged and transferred while batch k computes:
          staging thread: the batch is copied into one of three PINNED staging buffers by ``copy_threads`` native threads (one foreign call,
            ``ubd_host_memcpy_mt``) -- the transfer of pageable memory would otherwise be staged by the runtime, synchronously;
          copy-in stream: pinned -> device (three device input buffers), enqueued as soon as the batch is staged and BEFORE the
            consumer blocks on an older batch's results; an event hands the buffer to the compute stream;
          compute stream: the pipelined runner -- forward pass of batch k with the postprocess of batch k - 1 inside its stem kernel;
          copy-out stream: (logits, map, quads, classes, counts) of batch k - 1 -> pinned host memory behind an event;
          consumer (this generator): the object lists of batch k - 2 are built while all of that is in flight.
        ``meta_infos``: one list per batch when ``rescale``.  Results are identical to calling ``predict`` per batch
        (tests/test_gpu_end_to_end.py::test_predict_stream_equals_predict)."""
        import queue
        import threading
        import time
        dev = model.device
        runner = ModelRunner(self._net_config, max_objects_per_image=self._cap, pipelined=True, slots=3)
        runner._logit_threshold = self._logit_threshold
        s_main = torch.cuda.current_stream(dev)
        s_in, s_out = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
        lib = _lib.load()
        try:                                            # never more staging threads than half of the CPUs this process may run on
            copy_threads = max(1, min(int(copy_threads), len(os.sched_getaffinity(0)) // 2))
        except (AttributeError, OSError):
            copy_threads = max(1, int(copy_threads))
        NPIN, NDEV, NRES = 3, 3, 3
        pinned, dev_in, host_res = [None] * NPIN, [None] * NDEV, [None] * NRES
        fwd_done, d2h_done = [None] * NDEV, [None] * NRES
        inflight = []                                   # [batch index, device results, d2h event or None, meta]
        if rescale and meta_infos is None:
            raise AssertionError("rescale=True needs meta_infos (one list of meta_info per batch)")     # predict()'s rule (model_runner.py:116-117)
        metas = iter(meta_infos) if meta_infos is not None else None
        _MISSING = object()
        free_slots, staged = queue.Queue(), queue.Queue(maxsize=NPIN - 1)
        for slot in range(NPIN):
            free_slots.put((slot, None))
        stop = threading.Event()
        stats = {"wait_staged_s": 0.0, "enqueue_s": 0.0, "deliver_s": 0.0, "deliver_wait_s": 0.0, "stager_copy_s": 0.0, "batches": 0}
        self.last_stream_stats = stats                  # where the consumer thread's time went (tools/bench_host_stream.py prints it)

        def stager():
            """host side of the copy-in, its own thread: batch -> pinned staging buffer, ahead of the stream work"""
            try:
                torch.cuda.set_device(dev)              # a new thread starts on cuda:0: pinned allocations / event waits belong to the model's device
                for k, x in enumerate(batches):
                    if stop.is_set():
                        return
                    x = np.asarray(x)
                    if x.dtype != np.uint8:
                        x = x.astype(np.float32, copy=False)
                    x = np.ascontiguousarray(x)
                    tdt = torch.uint8 if x.dtype == np.uint8 else torch.float32
                    slot, ev = free_slots.get()
                    if ev is not None:
                        ev.synchronize()                # the transfer that last read this staging buffer is over
                    if pinned[slot] is None or tuple(pinned[slot].shape) != x.shape or pinned[slot].dtype != tdt:
                        pinned[slot] = torch.empty(x.shape, dtype=tdt, pin_memory=True)
                    dst = pinned[slot].numpy()
                    tc = time.perf_counter()
                    # one foreign call (ctypes drops the GIL), native threads inside: as `copy_threads` python pool tasks the copy took the
                    # interpreter away from the consumer thread at every hand-over (enqueue 0.15 -> 0.35 -> 0.8 ms at 2 / 4 / 8 threads)
                    lib.ubd_host_memcpy_mt(dst.ctypes.data, x.ctypes.data, x.nbytes, int(copy_threads))
                    stats["stager_copy_s"] += time.perf_counter() - tc       # the staging thread's own time (not the consumer's)
                    meta = None
                    if metas is not None:
                        meta = next(metas, _MISSING)
                        if meta is _MISSING:
                            raise ValueError(f"meta_infos ended before the batches did (batch {k} has none)")
                    staged.put((k, slot, meta))
                staged.put(None)
            except Exception as e:                      # noqa: BLE001 -- re-raised by the consumer
                staged.put(e)

        def copy_in(item):
            """pinned -> device on the copy-in stream; returns (k, device buffer index, event, meta)"""
            k, slot, meta = item
            d, src = k % NDEV, pinned[slot]
            if dev_in[d] is None or dev_in[d].shape != src.shape or dev_in[d].dtype != src.dtype:
                dev_in[d] = torch.empty(src.shape, dtype=src.dtype, device=dev)
            with torch.cuda.stream(s_in):
                if fwd_done[d] is not None:
                    s_in.wait_event(fwd_done[d])        # the forward pass that last read this device buffer is over
                dev_in[d].copy_(src, non_blocking=True)
                ev = torch.cuda.Event(); ev.record(s_in)
            free_slots.put((slot, ev))                  # the stager waits for the event before it writes the buffer again
            return k, d, ev, meta

        def fetch(entry):
            """device results of batch entry[0] -> its pinned host set on the copy-out stream, behind everything enqueued on the compute stream so far"""
            r, res = entry[0] % NRES, entry[1]
            if host_res[r] is None or any((h is None) != (t is None) or (t is not None and (h.shape != t.shape or h.dtype != t.dtype)) for h, t in zip(host_res[r], res)):
                host_res[r] = [None if t is None else torch.empty(t.shape, dtype=t.dtype, pin_memory=True) for t in res]
            ev_c = torch.cuda.Event(); ev_c.record(s_main)
            with torch.cuda.stream(s_out):
                s_out.wait_event(ev_c)
                for h, t in zip(host_res[r], res):
                    if t is not None:
                        h.copy_(t, non_blocking=True)
                ev = torch.cuda.Event(); ev.record(s_out)
            d2h_done[r] = ev
            entry[2] = ev

        def deliver(entry):
            tw = time.perf_counter()
            entry[2].synchronize()
            stats["deliver_wait_s"] += time.perf_counter() - tw     # of deliver_s: blocked on the device (results not there yet)
            logits_h, bmap_h, quads_h, classes_h, counts_h = [None if h is None else h.numpy() for h in host_res[entry[0] % NRES]]
            return self._assemble(counts_h, quads_h, classes_h, logits_h, bmap_h, rescale, entry[3], copy=True)

        th = threading.Thread(target=stager, daemon=True)
        th.start()
        try:
            ahead = None                                # batch k + 1, already on its way to the device
            done = False
            while True:
                t0 = time.perf_counter()
                if ahead is None:
                    if done:
                        break
                    item = staged.get()
                    if item is None:
                        break
                    if isinstance(item, BaseException):
                        raise item
                    ahead = copy_in(item)
                k, d, ev, meta = ahead
                ahead = None
                t1 = time.perf_counter()
                stats["wait_staged_s"] += t1 - t0
                s_main.wait_event(ev)
                if d2h_done[k % NRES] is not None:
                    s_main.wait_event(d2h_done[k % NRES])           # the runner's result slot k % 3 is about to be overwritten: batch k - 3 has left it (long ago)
                res = runner.predict_on_device(model, dev_in[d])   # forward of batch k + postprocess of batch k - 1, one stream
                fe = torch.cuda.Event(); fe.record(s_main)
                fwd_done[d] = fe
                if inflight:                                        # batch k - 1 is complete behind this call: copy its results out
                    fetch(inflight[-1])
                inflight.append([k, res, None, meta])
                if not done:                                        # batch k + 1: start its transfer NOW, before blocking on older results
                    try:
                        item = staged.get_nowait()
                        if item is None:
                            done = True
                        elif isinstance(item, BaseException):
                            raise item
                        else:
                            ahead = copy_in(item)
                    except queue.Empty:
                        pass
                t2 = time.perf_counter()
                stats["enqueue_s"] += t2 - t1
                stats["batches"] += 1
                while len(inflight) > 2:                            # build batch k - 2's lists while k - 1 copies out and k computes
                    out = deliver(inflight.pop(0))
                    stats["deliver_s"] += time.perf_counter() - t2
                    yield out
            if inflight:
                runner.flush()                                      # the last batch's postprocess, a launch of its own
                fetch(inflight[-1])
            while inflight:
                yield deliver(inflight.pop(0))
        finally:
            stop.set()
            # An early exit (the consumer stopped, the stager failed, _assemble raised) can leave a prefetched host -> device copy or a
            # device -> host copy in flight on the side streams.  The buffers they touch were allocated on the compute stream: once this
            # frame drops them the caching allocator may hand the blocks to the next allocation on that stream, and the late copy would
            # write into an unrelated tensor.  Drain both side streams before anything goes out of scope.
            s_in.synchronize()
            s_out.synchronize()
            for _ in range(40):                                     # a consumer that stopped early: unblock the stager (bounded: the thread is a
                if not th.is_alive():                               # daemon, and one that is blocked inside next(batches) cannot see `stop`)
                    break
                try:
                    staged.get_nowait()
                except queue.Empty:
                    pass
                th.join(timeout=0.05)

    @staticmethod
    def rescale(found_objects, meta_infos):
        """Boxes back to the coordinates of the original images (behaviour of model_runner.py:140-148): per image,
        multiply x by meta.xscale and y by meta.yscale and truncate toward zero (utils.rescale_bbox)."""
        if len(found_objects) != len(meta_infos):
            raise AssertionError("one meta_info per image is required")
        rescaled = []
        for objects, meta in zip(found_objects, meta_infos):
            rescaled.append([obj.create_same_markup(utils.rescale_bbox(obj.bbox, xscale=meta.xscale, yscale=meta.yscale))
                             for obj in objects])
        return rescaled
