"""CPU: the host rules of the training loop -- ReduceLROnPlateau and ModelCheckpoint against hand-derived tables, the file
order of build_callbacks_list, the split-log key filter, and keras_metrics.epoch_logs_from_sums against a direct size-weighted
mean.  A fake trainer / model records ``save_keras_h5`` calls; nothing here touches a GPU."""
import json
import os

import numpy as np
import pytest

from ubdvss_amd import keras_callbacks as kc, keras_metrics
from ubdvss_amd.data_generators import BatchGenerator


class _FakeModel:
    def __init__(self):
        self.saved = []

    def save_keras_h5(self, path, whole_model=True):
        self.saved.append((path, whole_model))


class _FakeOpt:
    def __init__(self, lr):
        self.lr = lr


class _FakeTrainer:
    def __init__(self, lr=1e-2):
        self.model, self.opt = _FakeModel(), _FakeOpt(lr)


class _FakeGenerator:
    def get_images_per_epoch(self):
        return 7

    def generate(self, add_metainfo=False):
        assert add_metainfo
        return iter(())


def _drive(cb, trainer, series, key="val_loss"):
    """on_epoch_end for every value of the series -> (logs['lr'] of every epoch, trainer.opt.lr after every epoch)"""
    cb.set_trainer(trainer)
    cb.on_train_begin()
    logged, after = [], []
    for epoch, value in enumerate(series):
        logs = {key: value, "loss": 1.0}
        cb.on_epoch_end(epoch, logs)
        logged.append(logs.get("lr"))
        after.append(trainer.opt.lr)
    return logged, after


def test_plateau_rule_table():
    """patience 2, factor 0.1, min_lr 1e-4, min_delta 1e-4, from lr 1e-2.  By hand: epoch 0 improves on +inf; epochs 1, 2 do not
    (wait 1, 2 -> reduce to 1e-3, wait 0); 0.99995 is NOT below best - min_delta = 0.9999, so epoch 3 counts as no improvement
    (wait 1); 0.5 improves (wait 0); epochs 5, 6 do not (wait 1, 2 -> reduce to 1e-4); from there the rate sits at min_lr whatever
    the wait.  logs['lr'] is the rate the epoch ran with, i.e. the rate before that epoch's decision."""
    series = [1.0, 1.0, 1.0, 0.99995, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5]
    tr = _FakeTrainer(1e-2)
    cb = kc.ReduceLROnPlateau(monitor="val_loss", factor=0.1, patience=2, min_lr=1e-4, min_delta=1e-4)
    logged, after = _drive(cb, tr, series)
    assert after == pytest.approx([1e-2, 1e-2, 1e-3, 1e-3, 1e-3, 1e-3, 1e-4, 1e-4, 1e-4, 1e-4, 1e-4, 1e-4], rel=1e-12)
    assert logged == pytest.approx([1e-2, 1e-2, 1e-2, 1e-3, 1e-3, 1e-3, 1e-3, 1e-4, 1e-4, 1e-4, 1e-4, 1e-4], rel=1e-12)
    assert all(lr >= 1e-4 for lr in after)                    # never below min_lr, not by a rounding error either
    assert after[-1] == 1e-4


def test_plateau_within_min_delta_is_no_improvement():
    """a series that creeps down by less than min_delta per epoch never improves after the first epoch"""
    tr = _FakeTrainer(1.0)
    cb = kc.ReduceLROnPlateau(factor=0.5, patience=3, min_lr=0.0, min_delta=1e-4)
    _, after = _drive(cb, tr, [1.0, 0.99995, 0.99992, 0.99991, 0.9998, 0.9998, 0.9998, 0.9998])
    # waits: 0, 1, 2, 3 -> reduce; 0.9998 < 1.0 - 1e-4 improves (best was still 1.0): wait 0; then 1, 2, 3 -> reduce
    assert after == [1.0, 1.0, 1.0, 0.5, 0.5, 0.5, 0.5, 0.25]


def test_plateau_cooldown_table():
    """patience 1, cooldown 2, factor 0.5, min_lr 0.1, constant series.  Epoch 1 reduces and starts the cooldown (counter 2);
    epoch 2: counter 1, still cooling: no wait; epoch 3: counter 0, wait 1 -> reduce; and so on every second epoch down to min_lr."""
    tr = _FakeTrainer(1.0)
    cb = kc.ReduceLROnPlateau(factor=0.5, patience=1, min_lr=0.1, cooldown=2)
    _, after = _drive(cb, tr, [1.0] * 11)
    assert after == [1.0, 0.5, 0.5, 0.25, 0.25, 0.125, 0.125, 0.1, 0.1, 0.1, 0.1]


def test_plateau_missing_monitor_changes_nothing():
    tr = _FakeTrainer(1e-2)
    cb = kc.ReduceLROnPlateau(patience=1)
    logged, after = _drive(cb, tr, [1.0, 1.0, 1.0], key="other")
    assert after == [1e-2] * 3 and logged == [1e-2] * 3


def test_checkpoint_names_and_best_only(tmp_path):
    tr = _FakeTrainer()
    every = kc.ModelCheckpoint(str(tmp_path / "model_{epoch:03d}.h5"))
    best = kc.ModelCheckpoint(str(tmp_path / "model_best.h5"), save_best_only=True)
    for cb in (every, best):
        cb.set_trainer(tr)
        cb.on_train_begin()
    series = [1.0, 1.0, 0.9, 0.95, 0.9, 0.8]
    for epoch, v in enumerate(series):
        before = len(tr.model.saved)
        every.on_epoch_end(epoch, {"val_loss": v})
        assert tr.model.saved[before:] == [(str(tmp_path / f"model_{epoch + 1:03d}.h5"), True)]
        before = len(tr.model.saved)
        best.on_epoch_end(epoch, {"val_loss": v})
        saved_best = len(tr.model.saved) > before
        assert saved_best == (epoch in (0, 2, 5)), epoch        # strict decrease only: the equal values of epochs 1 and 4 do not save
    assert best.best == 0.8
    tr.model.saved.clear()
    best.on_epoch_end(6, {"loss": 0.1})                         # no monitor value: nothing saved
    assert tr.model.saved == []
    best.on_epoch_end(7, {"val_loss": float("nan")})            # NaN is not below anything
    assert tr.model.saved == []


def test_build_callbacks_list_order_and_files(tmp_path):
    log_dir = str(tmp_path / "run")
    os.makedirs(log_dir)
    cbs = kc.build_callbacks_list(log_dir, net_config=_net_config(), training_generator=_FakeGenerator(),
                                  validation_generator=_FakeGenerator(), max_evaluated_images=3)
    assert [type(c) for c in cbs] == [kc.ModelCheckpoint, kc.ModelCheckpoint, kc.ModelCheckpoint, kc.ReduceLROnPlateau,
                                      kc.EvaluationCallback, kc.EvaluationCallback]
    assert [(c.filepath, c.save_best_only, c.monitor) for c in cbs[:3]] == [
        (os.path.join(log_dir, "model.h5"), False, "val_loss"),
        (os.path.join(log_dir, "model_best.h5"), True, "val_loss"),
        (os.path.join(log_dir, "backup", "model_{epoch:03d}.h5"), False, "val_loss")]
    assert os.path.isdir(os.path.join(log_dir, "backup"))
    r = cbs[3]
    assert (r.monitor, r.factor, r.patience, r.min_lr, r.min_delta, r.cooldown) == ("val_loss", 0.1, 20, 1e-4, 1e-4, 0)
    assert [(c.log_dir, c.mode) for c in cbs[4:]] == [(os.path.join(log_dir, "train"), "train"), (os.path.join(log_dir, "valid"), "valid")]
    assert [c._n_evaluated_images for c in cbs[4:]] == [3, 3]
    # one epoch through the four host callbacks: the order the files are written in
    tr = _FakeTrainer()
    for c in cbs[:4]:
        c.set_trainer(tr)
        c.on_train_begin()
    logs = {"loss": 2.0, "val_loss": 1.5}
    for c in cbs[:4]:
        c.on_epoch_end(0, logs)
    assert [p for p, _ in tr.model.saved] == [os.path.join(log_dir, "model.h5"), os.path.join(log_dir, "model_best.h5"),
                                              os.path.join(log_dir, "backup", "model_001.h5")]
    assert logs["lr"] == 1e-2


def _net_config():
    from ubdvss_amd import NetConfig
    return NetConfig(grey=False)


def test_split_log_key_filter_and_file(tmp_path):
    logs = {"loss": 1.0, "detection_pixel_f1": 0.5, "lr": 1e-3, "val_loss": 2.0, "val_detection_pixel_f1": 0.25, "val_f1_iou0.50": 0.75,
            "value_head": 3.0}
    train = kc.SingleSplitLogCallback(str(tmp_path / "train"), "train")
    valid = kc.SingleSplitLogCallback(str(tmp_path / "valid"), "valid")
    # the reference's rule is startswith('val'), not startswith('val_'): 'value_head' goes to the validation side as 'head'
    assert train.filter_logs(logs) == {"loss": 1.0, "detection_pixel_f1": 0.5, "lr": 1e-3}
    assert valid.filter_logs(logs) == {"loss": 2.0, "detection_pixel_f1": 0.25, "f1_iou0.50": 0.75, "head": 3.0}
    for cb in (train, valid):
        cb.set_trainer(_FakeTrainer())
        cb.on_epoch_end(0, logs)
        cb.on_epoch_end(1, logs)
    lines = [json.loads(s) for s in open(tmp_path / "valid" / "scalars.jsonl")]
    assert lines == [{"epoch": e, "loss": 2.0, "detection_pixel_f1": 0.25, "f1_iou0.50": 0.75, "head": 3.0} for e in (0, 1)]
    lines = [json.loads(s) for s in open(tmp_path / "train" / "scalars.jsonl")]
    assert lines == [{"epoch": e, "loss": 1.0, "detection_pixel_f1": 0.5, "lr": 1e-3} for e in (0, 1)]
    with pytest.raises(AssertionError):
        kc.SingleSplitLogCallback(str(tmp_path), "test")


def _random_loss_vectors(rng, count):
    out = []
    for _ in range(count):
        n_pix = int(rng.integers(64, 4096))
        n_pos = int(rng.integers(0, n_pix))
        tp = int(rng.integers(0, n_pos + 1))
        fn = n_pos - tp
        fp = int(rng.integers(0, n_pix - n_pos + 1))
        tn = n_pix - n_pos - fp
        cls_ok = int(rng.integers(0, n_pos + 1))
        det, cls = rng.random(2) * 3
        out.append(np.array([det + cls, det, cls, rng.integers(0, 99), *rng.random(3), n_pos, tp, tn, fp, fn, cls_ok, n_pix, 0, 0], np.float32))
    return out


@pytest.mark.parametrize("classification_mode", [False, True])
def test_epoch_logs_are_the_size_weighted_mean(classification_mode):
    rng = np.random.default_rng(11)
    vectors = _random_loss_vectors(rng, 9)
    sizes = [int(s) for s in rng.integers(1, 9, len(vectors))]
    acc = np.zeros(2 + len(keras_metrics.EPOCH_VALUES))
    per_batch = []
    for v, n in zip(vectors, sizes):
        full = keras_metrics.metrics_from_loss_vector(v, True)          # all eleven are always accumulated
        acc[0] += n
        for i, name in enumerate(keras_metrics.EPOCH_VALUES):
            acc[2 + i] = acc[2 + i] + full[name] * n
        per_batch.append(keras_metrics.metrics_from_loss_vector(v, classification_mode))
    logs = keras_metrics.epoch_logs_from_sums(acc, classification_mode, prefix="val_")
    names = ["loss"] + keras_metrics.get_all_metrics(classification_mode)
    assert list(logs) == ["val_" + n for n in names]                    # exactly the names Keras reports for this mode, in its order
    assert ("val_classification_loss" in logs) == classification_mode
    for name in names:
        direct = 0.0
        for m, n in zip(per_batch, sizes):
            direct = direct + m[name] * n
        assert logs["val_" + name] == direct / sum(sizes), name
    assert set(keras_metrics.EPOCH_VALUES) == set(["loss"] + keras_metrics.get_all_metrics(True))


def test_epoch_logs_without_a_step_raise():
    with pytest.raises(ValueError, match="seen no image"):
        keras_metrics.epoch_logs_from_sums(np.zeros(13), False)
    with pytest.raises(ValueError, match="slots"):
        keras_metrics.epoch_logs_from_sums(np.ones(12), False)


def test_batch_generator_refuses_unknown_markup_types():
    with pytest.raises(ValueError, match="not supported"):
        BatchGenerator("nowhere", 2, "Barcode", _net_config())          # the XML readers of the reference are not built
    with pytest.raises(ValueError, match="reader instance"):
        BatchGenerator("nowhere", 2, object(), _net_config())


class _BrokenReader:
    def __init__(self, names):
        self._names = names

    def read_markup(self):
        pass

    def get_list_of_images(self):
        return list(self._names)

    def get_image_markup(self, name):
        return []

    def get_image(self, name):
        raise OSError("unreadable")


def test_batch_generator_never_hangs_without_data():
    with pytest.raises(ValueError, match="no image"):
        BatchGenerator(None, 2, _BrokenReader([]), _net_config())
    gen = BatchGenerator(None, 2, _BrokenReader(["a", "b", "c"]), _net_config(), prepare_batch_size=2)
    with pytest.raises(RuntimeError, match="gave no batch"):
        next(gen.generate())                                    # every image fails to read: an error, not an endless loop
