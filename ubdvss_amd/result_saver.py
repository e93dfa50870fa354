"""Result output of predict.py -- host mirror of semantic_segmentation/model_runner.py:215-228 (CSV of the found
quadrilaterals), of the rescale step model_runner.py:140-148 / utils.py:67-69 and of ResultSaver (:154-212): the folders
markup/, predictions/ and images/<category>/ of a run."""
import os

import numpy as np

from .data_markup import ClassifiedObjectMarkup


def markup_csv_string(markups):
    """One line per object: x1,y1,...,x4,y4,""[,type]  (model_runner.py:215-228)."""
    out = ''
    for markup in markups:
        out += '{:d},{:d},{:d},{:d},{:d},{:d},{:d},{:d},""'.format(*[int(xy) for xy in markup.bbox])
        if isinstance(markup, ClassifiedObjectMarkup):
            out += f',{markup.object_type}\n'
        else:
            out += '\n'
    return out


def save_markup_csv(filename, markups):
    with open(filename, "w") as text_file:
        text_file.write(markup_csv_string(markups))


class ResultSaver:
    """Writes a run's results: ground truth and found objects as CSV, visualisations as PNG (the role of the reference's
    ResultSaver, model_runner.py:154-212; only its public contract is kept).  Tree under ``save_dir``:
        markup/<filename>.txt, predictions/<filename>.txt, images/<category>/<filename>.<tag>.png
    with one images/ folder per entry of ImageResultCategories.get_folders().  The PNGs are written with Pillow from the
    RGB arrays: the same pixels the reference's cv2.imwrite of the BGR copy stores.  Without ``save_dir`` nothing is ever
    written; the images/ tree exists only when visualisations were asked for."""

    _CSV_FOLDERS = {"gt": "markup", "found": "predictions"}
    _IMAGE_ROOT = "images"

    def __init__(self, save_dir=None, save_visualizations=False):
        from .evaluation import ImageResultCategories
        self.save_dir = save_dir
        self.writes_images = save_dir is not None and bool(save_visualizations)
        if not save_dir:
            return
        wanted = list(self._CSV_FOLDERS.values())
        if self.writes_images:
            wanted += [os.path.join(self._IMAGE_ROOT, folder) for folder in ImageResultCategories.get_folders()]
        for relative in wanted:
            os.makedirs(os.path.join(save_dir, relative), exist_ok=True)

    def _csv_path(self, kind, meta):
        return os.path.join(self.save_dir, self._CSV_FOLDERS[kind], meta.filename + ".txt")

    def save_gt_and_prediction(self, gt_objects, found_objects, meta_infos):
        """One CSV per image and side, named after meta.filename"""
        if not self.save_dir:
            return
        for meta, truth, found in zip(meta_infos, gt_objects, found_objects):
            save_markup_csv(self._csv_path("gt", meta), truth)
            save_markup_csv(self._csv_path("found", meta), found)

    def save_visualizations(self, need_visualize_categories, meta_infos, visualizations):
        """need_visualize_categories: per image the folders to save it in (an empty list: not saved); visualizations:
        {tag: per-image RGB uint8 arrays} -- host arrays or device tensors (copied once per tag)."""
        from PIL import Image
        if not self.writes_images:
            return
        on_host = {tag: (v.cpu().numpy() if hasattr(v, "cpu") else v) for tag, v in visualizations.items()}
        for k, (meta, folders) in enumerate(zip(meta_infos, need_visualize_categories)):
            if not folders:
                continue
            pictures = {tag: Image.fromarray(np.ascontiguousarray(stack[k], dtype=np.uint8)) for tag, stack in on_host.items()}
            for folder in folders:
                for tag, picture in pictures.items():
                    picture.save(os.path.join(self.save_dir, self._IMAGE_ROOT, folder, f"{meta.filename}.{tag}.png"))

    save_markup_csv = staticmethod(save_markup_csv)
