"""Callbacks of the training run -- host mirror of semantic_segmentation/keras_callbacks.py, plus the two Keras callbacks that file
imports (``ModelCheckpoint``, ``ReduceLROnPlateau``), for ``Trainer.fit``.

A callback is a plain class with ``set_trainer(trainer)``, ``on_train_begin()`` and ``on_epoch_end(epoch, logs)``; ``epoch`` counts
from 0 and ``logs`` is the dict ``Trainer.fit`` built from the epoch's device sums (training means, ``val_`` means, ``lr``).  The
callbacks run on the host between epochs; whatever they read from the device (a checkpoint's weights, an evaluation's sums) is
outside the epoch's one-read rule, which concerns the steps.

The rules of ``ModelCheckpoint`` and ``ReduceLROnPlateau`` are restated from Keras 2.2.4 from knowledge of that release, not
compared against an installed Keras: like the rest of the oracle they are parity-unpinned.  The defaults of ``ReduceLROnPlateau``
here are the values ``build_callbacks_list`` passes (factor 0.1, patience 20, min_lr 1e-4) on top of Keras' min_delta 1e-4,
cooldown 0, mode 'min'; only the 'min' modes are built (every monitored value of the reference is a loss).

TensorBoard event files need TensorFlow and are out of scope: ``SingleSplitLogCallback`` writes the scalars it would have sent to
TensorBoard as one JSON line per epoch into ``<log_dir>/scalars.jsonl``, and ``EvaluationCallback`` saves its images as PNG files
(off by default) instead of image summaries.

In a data-parallel run every rank gets the same logs (``distributed.allreduce_epoch_sums``), so every rank takes the same
learning-rate and best-checkpoint decisions; only rank 0 writes files.
"""
import json
import logging
import os

import numpy as np

from .model_runner import ModelRunner


class Callback:
    def __init__(self):
        self.trainer = None

    def set_trainer(self, trainer):
        self.trainer = trainer

    @property
    def model(self):
        return self.trainer.model

    def _writes_files(self):
        chief = getattr(self.trainer, "_is_chief", None)
        return True if chief is None else bool(chief())

    def on_train_begin(self):
        pass

    def on_epoch_end(self, epoch, logs=None):
        pass


class ModelCheckpoint(Callback):
    """keras.callbacks.ModelCheckpoint (period 1, mode 'min'): after every epoch the whole model goes to
    ``filepath.format(epoch=epoch + 1, **logs)`` through ``Model.save_keras_h5`` (the optimiser's moments are not written, as
    everywhere in this package); with ``save_best_only`` only when ``logs[monitor]`` is strictly below the best value so far
    (+inf at the start of training).  A missing monitor value is logged and skips the save, as Keras does."""

    def __init__(self, filepath, monitor='val_loss', save_best_only=False):
        super().__init__()
        self.filepath, self.monitor, self.save_best_only = filepath, monitor, save_best_only
        self.best = np.inf

    def on_train_begin(self):
        pass                                    # Keras keeps `best` across fit calls of one callback object; so does this

    def on_epoch_end(self, epoch, logs=None):
        logs = {} if logs is None else logs
        filepath = self.filepath.format(epoch=epoch + 1, **logs)
        if self.save_best_only:
            current = logs.get(self.monitor)
            if current is None:
                logging.warning("ModelCheckpoint: the logs hold no %s, so there is no best model to judge; nothing saved", self.monitor)
                return
            if not current < self.best:
                return
            self.best = current
        if self._writes_files():
            self.model.save_keras_h5(filepath)


class ReduceLROnPlateau(Callback):
    """keras.callbacks.ReduceLROnPlateau, mode 'min'.  Per epoch: ``logs['lr']`` is set to the current rate; while in cooldown the
    counter goes down and ``wait`` is 0; ``current < best - min_delta`` is an improvement (new best, ``wait = 0``); otherwise,
    outside cooldown, ``wait += 1`` and at ``wait >= patience`` a rate above ``min_lr`` becomes ``max(lr * factor, min_lr)``, the
    cooldown restarts and ``wait = 0``.  The new rate is written to ``trainer.opt.lr``: the next ``ubd_adam_step`` uses it."""

    def __init__(self, monitor='val_loss', factor=0.1, patience=20, min_lr=1e-4, min_delta=1e-4, cooldown=0):
        super().__init__()
        if factor >= 1.0:
            raise ValueError(f'a factor of {factor} would never lower the learning rate; it must be below 1')
        self.monitor, self.factor, self.patience, self.min_lr = monitor, factor, patience, min_lr
        self.min_delta, self.cooldown = min_delta, cooldown
        self._reset()

    def _reset(self):
        self.best, self.wait, self.cooldown_counter = np.inf, 0, 0

    def on_train_begin(self):
        self._reset()

    def in_cooldown(self):
        return self.cooldown_counter > 0

    def on_epoch_end(self, epoch, logs=None):
        logs = logs if logs is not None else {}
        opt = self.trainer.opt
        logs['lr'] = float(opt.lr)
        current = logs.get(self.monitor)
        if current is None:
            logging.warning("ReduceLROnPlateau: the logs hold no %s; the learning rate stays", self.monitor)
            return
        if self.in_cooldown():
            self.cooldown_counter -= 1
            self.wait = 0
        if current < self.best - self.min_delta:
            self.best = current
            self.wait = 0
        elif not self.in_cooldown():
            self.wait += 1
            if self.wait >= self.patience:
                old_lr = float(opt.lr)
                if old_lr > self.min_lr:
                    opt.lr = max(old_lr * self.factor, self.min_lr)
                    logging.info("ReduceLROnPlateau: learning rate %g after epoch %d", opt.lr, epoch + 1)
                    self.cooldown_counter = self.cooldown
                    self.wait = 0


class SingleSplitLogCallback(Callback):
    """keras_callbacks.py:16-50: one half of an epoch's logs, so that training and validation curves can share an axis.  Mode
    'train' keeps the keys that do not start with ``val``; mode 'valid' keeps the keys that do and drops everything up to and
    including their first underscore.  The kept scalars are appended to ``<log_dir>/scalars.jsonl`` as one line
    ``{"epoch": epoch, name: value, ...}`` per epoch."""
    ONLY_TRAIN_LOGS_MODE = 'train'
    ONLY_VALID_LOGS_MODE = 'valid'
    SCALARS_FILENAME = "scalars.jsonl"

    def __init__(self, log_dir, mode=ONLY_TRAIN_LOGS_MODE):
        super().__init__()
        if mode not in (self.ONLY_TRAIN_LOGS_MODE, self.ONLY_VALID_LOGS_MODE):
            raise AssertionError(f"mode is '{self.ONLY_TRAIN_LOGS_MODE}' or '{self.ONLY_VALID_LOGS_MODE}', got {mode!r}")
        self.log_dir = log_dir
        self.mode = mode

    def is_train_log_mode(self):
        return self.mode == self.ONLY_TRAIN_LOGS_MODE

    def filter_logs(self, logs):
        kept = {}
        for key, value in logs.items():
            validation_key = key.startswith('val')
            if self.is_train_log_mode():
                if not validation_key:
                    kept[key] = value
            elif validation_key:
                kept[key.partition('_')[2]] = value
        return kept

    def on_epoch_end(self, epoch, logs=None):
        record = {"epoch": int(epoch)}
        for key, value in self.filter_logs(logs or {}).items():
            record[key] = float(value)
        if self._writes_files():
            os.makedirs(self.log_dir, exist_ok=True)
            with open(os.path.join(self.log_dir, self.SCALARS_FILENAME), "a") as f:
                f.write(json.dumps(record) + "\n")

    @classmethod
    def get_callbacks(cls, train_log_dir, valid_log_dir):
        folders = {cls.ONLY_TRAIN_LOGS_MODE: train_log_dir, cls.ONLY_VALID_LOGS_MODE: valid_log_dir}
        return [cls(folder, mode) for mode, folder in folders.items()]


class EvaluationCallback(SingleSplitLogCallback):
    """keras_callbacks.py:53-113: after every epoch the object-level metrics of ``ModelRunner.run`` over images of
    ``batch_generator`` (a ``BatchGenerator``) -- all of them when ``max_evaluated_images`` is negative, otherwise at most that
    many -- merged with the epoch's logs and written through the split rule above.  The callback draws from ONE
    ``generate(add_metainfo=True)`` iterator for as long as it lives, so successive epochs continue where the last one stopped.
    ``save_images``: the first ten images of every visualisation of the epoch's drawn batch are saved as
    ``<log_dir>/images/epoch_XXX/<mode>_<key>_<i>.png`` (the reference sends them to TensorBoard as image summaries)."""
    MAX_SAVED_IMAGES = 10

    def __init__(self, log_dir, net_config, batch_generator, max_evaluated_images=-1,
                 mode=SingleSplitLogCallback.ONLY_TRAIN_LOGS_MODE, save_images=False, average_precision=False):
        SingleSplitLogCallback.__init__(self, log_dir, mode)
        available = batch_generator.get_images_per_epoch()
        self._n_evaluated_images = available if max_evaluated_images < 0 else min(available, max_evaluated_images)
        self._runner = ModelRunner(net_config, pixel_threshold=0.5)
        self._save_images = bool(save_images)
        self._average_precision = bool(average_precision)       # opt-in: the epoch's logs gain ap_iou* and map (ModelRunner.run)
        self._batches = self._run_batches(batch_generator.generate(add_metainfo=True))

    @staticmethod
    def _run_batches(generator):
        """the generator's (images, targets, meta) as ModelRunner.run takes a batch: images, the ground truth on the ORIGINAL
        images, the meta infos (their scales take found boxes back there), the label maps"""
        for images, targets, meta in generator:
            yield images, [m.markup for m in meta], meta, targets

    def on_epoch_end(self, epoch, logs=None):
        measured, pictures = {}, {}
        if self._n_evaluated_images > 0:
            measured, pictures = self._runner.run(self.model, self._batches, self._n_evaluated_images,   # no save_dir: nothing is written there
                                                  average_precision=self._average_precision)
        # a validation callback files its own metrics under val_ so that the split rule keeps them and drops the training logs
        prefix = "" if self.is_train_log_mode() else "val_"
        merged = {prefix + name: value for name, value in measured.items()}
        merged.update(logs or {})                                   # the epoch's logs win over a metric of the same name
        if self._save_images and self._writes_files():
            self._write_images(epoch, pictures)
        SingleSplitLogCallback.on_epoch_end(self, epoch, merged)

    def _write_images(self, epoch, pictures_by_key):
        from PIL import Image
        folder = os.path.join(self.log_dir, "images", f"epoch_{epoch + 1:03d}")
        os.makedirs(folder, exist_ok=True)
        for key in pictures_by_key:
            pictures = pictures_by_key[key][:self.MAX_SAVED_IMAGES]
            pictures = pictures.cpu().numpy() if hasattr(pictures, "cpu") else np.asarray(pictures)
            for i, picture in enumerate(pictures):
                Image.fromarray(picture).save(os.path.join(folder, f"{self.mode}_{key}_{i}.png"))

    @classmethod
    def get_callbacks(cls, net_config, train_log_dir, valid_log_dir, train_generator, valid_generator, max_evaluated_images):
        sides = ((cls.ONLY_TRAIN_LOGS_MODE, train_log_dir, train_generator), (cls.ONLY_VALID_LOGS_MODE, valid_log_dir, valid_generator))
        return [cls(folder, net_config, generator, max_evaluated_images, mode=mode) for mode, folder, generator in sides]


def build_callbacks_list(log_dir, net_config, training_generator, validation_generator, max_evaluated_images=-1):
    """keras_callbacks.py:116-146, the same files, constants and order.  In list order: ``model.h5`` (every epoch),
    ``model_best.h5`` (on a new lowest ``val_loss``), ``backup/model_{epoch:03d}.h5`` (every epoch, kept),
    ReduceLROnPlateau(val_loss, factor 0.1, patience 20, min_lr 1e-4), the evaluation callbacks on ``train/`` and ``valid/``."""
    os.makedirs(os.path.join(log_dir, "backup"), exist_ok=True)
    checkpoints = [ModelCheckpoint(os.path.join(log_dir, "model.h5")),
                   ModelCheckpoint(os.path.join(log_dir, "model_best.h5"), save_best_only=True),
                   ModelCheckpoint(os.path.join(log_dir, "backup", "model_{epoch:03d}.h5"))]
    plateau = ReduceLROnPlateau(monitor='val_loss', factor=0.1, patience=20, min_lr=1e-4)
    evaluations = EvaluationCallback.get_callbacks(net_config, os.path.join(log_dir, "train"), os.path.join(log_dir, "valid"),
                                                   training_generator, validation_generator, max_evaluated_images)
    return checkpoints + [plateau] + evaluations
