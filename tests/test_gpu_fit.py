"""GPU: the training loop.  (a) ubd_epoch_accumulate against the float64 restatement built from metrics_from_loss_vector, bit for
bit; (b) Trainer.fit against the same steps made by hand -- parameters bit-equal, epoch logs exactly the size-weighted means of the
per-step metrics, val_ logs exactly forward + loss with the end-of-epoch parameters; (c) a learning rate set by a callback reaches
Adam; (d) fit reads the device once per epoch and never synchronises; (e) the files of build_callbacks_list.
Exact comparisons throughout: the train step is deterministic (tests/test_gpu_train.py::test_gradients_repeat_bit_for_bit) and the
accumulator's arithmetic is restated operation for operation in float64."""
import json
import os

import numpy as np
import pytest
import torch

from ubdvss_amd import NetConfig, Model, Trainer, Adam, ObjectMarkup, losses, keras_metrics, _lib, synthetic
from ubdvss_amd import keras_callbacks as kc
from ubdvss_amd.data_generators import BatchGenerator

pytestmark = pytest.mark.gpu

SLOTS = 2 + len(keras_metrics.EPOCH_VALUES)


def _host_accumulate(acc, loss16, n):
    """the float64 restatement of ubd_epoch_accumulate (include/ubd.h)"""
    v = np.asarray(loss16, dtype=np.float32)
    m = keras_metrics.metrics_from_loss_vector(v, True)
    acc[0] = acc[0] + n
    if not np.isfinite(float(v[0])):
        acc[1] = acc[1] + 1
    for i, name in enumerate(keras_metrics.EPOCH_VALUES):
        acc[2 + i] = acc[2 + i] + np.float64(m[name]) * np.float64(n)
    return acc


def _device_accumulate(acc_dev, loss_dev, n):
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.ubd_epoch_accumulate(loss_dev.data_ptr(), n, acc_dev.data_ptr(), stream), "ubd_epoch_accumulate")


def _labels(rng, n, mh, mw, ncls, kind="mixed"):
    if kind == "no_positive":
        return np.zeros((n, mh, mw), np.int32)
    if kind == "no_negative":
        return rng.integers(1, max(ncls, 1) + 1, (n, mh, mw)).astype(np.int32)
    lab = np.zeros((n, mh, mw), np.int32)
    for i in range(n):
        y0, x0 = int(rng.integers(0, mh // 2)), int(rng.integers(0, mw // 2))
        lab[i, y0:y0 + mh // 3 + 1, x0:x0 + mw // 3 + 1] = int(rng.integers(1, max(ncls, 1) + 1))
    return lab


def test_epoch_accumulate_equals_host_restatement():
    lib = _lib.load()
    assert _lib.UBD_EPOCH_VALUES == len(keras_metrics.EPOCH_VALUES) and lib.ubd_epoch_accumulator_bytes() == 8 * SLOTS
    rng = np.random.default_rng(3)
    cases = [(2, 16, 16, 0, "mixed", 1), (2, 16, 16, 3, "mixed", 2), (3, 24, 40, 0, "mixed", 3), (3, 24, 40, 3, "mixed", 5),
             (2, 16, 24, 3, "no_positive", 8), (2, 20, 16, 0, "no_negative", 2)]
    acc_dev = torch.zeros(SLOTS, dtype=torch.float64, device="cuda")
    acc = np.zeros(SLOTS)
    for n, mh, mw, ncls, kind, n_images in cases:
        logits = (rng.standard_normal((n, mh, mw, 1 + ncls)) * 3).astype(np.float32)
        loss, _ = losses.loss_and_grad(_labels(rng, n, mh, mw, ncls, kind), torch.from_numpy(logits).cuda(), want_grad=False)
        _device_accumulate(acc_dev, loss, n_images)
        v = loss.cpu().numpy()
        m = keras_metrics.metrics_from_loss_vector(v, True)
        if kind == "no_positive":                      # the denominators clamp to 1 and f1 is 0, nothing divides by zero
            assert v[7] == 0 and m["detection_pixel_precision"] == 0 and m["detection_pixel_f1"] == 0 and m["classification_pixel_acc"] == 0
        if kind == "no_negative":
            assert v[7] == v[13] and v[9] == 0 and v[10] == 0
        _host_accumulate(acc, v, n_images)
        assert np.array_equal(acc_dev.cpu().numpy(), acc), (kind, n, mh, mw, ncls, acc_dev.cpu().numpy(), acc)
    assert acc[0] == 1 + 2 + 3 + 5 + 8 + 2 and acc[1] == 0 and np.isfinite(acc).all() and (acc[2:6] > 0).all()
    # a step whose total is NaN: counted, propagated into the sums it touches, the counter-only sums stay finite and exact
    bad = np.array([np.nan, 1.5, np.nan, 3, 0.1, 0.2, 0.3, 10, 8, 80, 2, 2, 7, 92, 0, 0], np.float32)
    _device_accumulate(acc_dev, torch.from_numpy(bad).cuda(), 3)
    _host_accumulate(acc, bad, 3)
    got = acc_dev.cpu().numpy()
    assert got[1] == 1 and got[0] == 24
    names = keras_metrics.EPOCH_VALUES
    assert np.isnan(got[2 + names.index("loss")]) and np.isnan(got[2 + names.index("classification_loss")])
    finite = [2 + names.index(k) for k in names if k not in ("loss", "classification_loss")]
    assert np.isfinite(got[finite]).all() and np.array_equal(got[finite], acc[finite])
    assert np.array_equal(got, acc, equal_nan=True)
    # an infinite total counts too
    bad[0] = np.inf
    _device_accumulate(acc_dev, torch.from_numpy(bad).cuda(), 1)
    assert acc_dev.cpu().numpy()[1] == 2


def test_epoch_accumulate_refuses_bad_arguments():
    lib = _lib.load()
    acc = torch.zeros(SLOTS, dtype=torch.float64, device="cuda")
    loss = torch.zeros(16, dtype=torch.float32, device="cuda")
    assert lib.ubd_epoch_accumulate(loss.data_ptr(), 0, acc.data_ptr(), None) != 0
    assert lib.ubd_epoch_accumulate(None, 1, acc.data_ptr(), None) != 0
    assert lib.ubd_epoch_accumulate(loss.data_ptr(), 1, None, None) != 0
    torch.cuda.synchronize()
    assert not acc.cpu().numpy().any()


# ------------------------------------------------------------------------------------------------ fit
def _config(ncls):
    return NetConfig(class_names=[f"c{i}" for i in range(ncls)] if ncls else None, grey=False)


def _batches(seed, sizes, ncls, side=32):
    """uint8 image batches (n, side, side, 3) with their label maps (n, side/4, side/4, 1), one per entry of sizes"""
    rng = np.random.default_rng(seed)
    out = []
    for k, n in enumerate(sizes):
        lab = _labels(rng, n, side // 4, side // 4, ncls)
        x = synthetic.textured_images(seed * 100 + k, lab, 4, 3)
        out.append((x, lab[..., None]))
    return out


def _cuda(batch):
    return torch.from_numpy(batch[0]).cuda(), torch.from_numpy(batch[1]).cuda()


def _expected_logs(records, cls_mode, prefix=""):
    acc = np.zeros(SLOTS)
    for v, n in records:
        _host_accumulate(acc, v, n)
    return keras_metrics.epoch_logs_from_sums(acc, cls_mode, prefix)


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("ncls", [0, 2])
def test_fit_equals_manual_steps(ncls, dtype):
    cfg = _config(ncls)
    steps, epochs, val_steps = 3, 2, 2
    train = _batches(5 + ncls, [2, 1, 2, 1, 2, 2], ncls)              # batch sizes 2 and 1 inside one epoch: the weighting matters
    val = _batches(9 + ncls, [2, 1, 1, 2], ncls)
    # --- fit: numpy batches for training, device tensors for validation
    tr = Trainer(Model(cfg, dtype=dtype, seed=0), Adam(1e-3))
    seen_logs = []

    class Recorder:
        def on_epoch_end(self, epoch, logs):
            seen_logs.append((epoch, dict(logs)))

    history = tr.fit(iter(train), steps, epochs, validation_data=iter([_cuda(b) for b in val]), validation_steps=val_steps,
                     callbacks=[Recorder()])
    # --- the same by hand
    m2 = Model(cfg, dtype=dtype, seed=0)
    tr2 = Trainer(m2, Adam(1e-3))
    expected = []
    for epoch in range(epochs):
        records = []
        for b in train[epoch * steps:(epoch + 1) * steps]:
            x, y = _cuda(b)
            records.append((tr2.train_step_on_device(x, y).cpu().numpy().copy(), x.shape[0]))
        logs = _expected_logs(records, ncls > 0)
        records = []
        for b in val[epoch * val_steps:(epoch + 1) * val_steps]:
            x, y = _cuda(b)
            loss, _ = losses.loss_and_grad(y, m2.predict_on_device(x), want_grad=False)
            records.append((loss.cpu().numpy().copy(), x.shape[0]))
        logs.update(_expected_logs(records, ncls > 0, "val_"))
        logs["lr"] = 1e-3
        expected.append(logs)
    assert torch.equal(tr.model.params, tr2.model.params)
    assert torch.equal(tr.m, tr2.m) and torch.equal(tr.v, tr2.v) and tr.iterations == tr2.iterations == 6
    assert [e for e, _ in seen_logs] == [0, 1] and history.epoch == [0, 1]
    for (_, got), want in zip(seen_logs, expected):
        assert list(got) == list(want)                              # loss + get_all_metrics, then the val_ names, then lr
        assert got == want, {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert ("classification_loss" in expected[0]) == (ncls > 0) and "val_detection_pixel_f1" in expected[0]
    assert history.history == {k: [e[k] for e in expected] for k in expected[0]}
    assert all(np.isfinite(v) for e in expected for v in e.values())
    # evaluate(): the validation logs of the last epoch again, without a prefix (the parameters have not moved since)
    again = tr.evaluate(iter(val[2:]), 2)
    assert again == {k[4:]: v for k, v in expected[1].items() if k.startswith("val_")}


def test_fit_float_images_and_initial_epoch():
    """float images are fed as they are; initial_epoch skips epochs, not data"""
    cfg = _config(0)
    data = [((x.astype(np.float32) / 127.5 - 1.0), y) for x, y in _batches(21, [2, 2, 2], 0)]
    tr = Trainer(Model(cfg, seed=0), Adam(1e-3))
    h = tr.fit(iter(data), 1, 3, initial_epoch=1)
    tr2 = Trainer(Model(cfg, seed=0), Adam(1e-3))
    for b in data[:2]:
        tr2.train_step_on_device(*_cuda(b))
    assert h.epoch == [1, 2] and torch.equal(tr.model.params, tr2.model.params)
    with pytest.raises(ValueError, match="validation_steps"):
        tr.fit(iter(data), 1, 1, validation_data=iter(data))


def test_lr_set_by_a_callback_reaches_adam():
    cfg = _config(0)
    data = _batches(31, [2, 2, 2, 2], 0)

    class SetLR:
        def set_trainer(self, trainer):
            self.trainer = trainer

        def on_epoch_end(self, epoch, logs):
            if epoch == 0:
                self.trainer.opt.lr = 3e-4

    tr = Trainer(Model(cfg, seed=0), Adam(1e-2))
    h = tr.fit(iter(data), 2, 2, callbacks=[SetLR()])
    assert h.history["lr"] == [1e-2, 3e-4] and tr.opt.lr == 3e-4
    finals = {}
    for change in (True, False):
        t = Trainer(Model(cfg, seed=0), Adam(1e-2))
        for k, b in enumerate(data):
            if k == 2 and change:
                t.opt.lr = 3e-4
            t.train_step_on_device(*_cuda(b))
        finals[change] = t.model.params.clone()
    assert torch.equal(tr.model.params, finals[True])
    assert not torch.equal(finals[True], finals[False])            # the rate matters at these steps: the comparison above can fail


@pytest.mark.parametrize("with_validation", [False, True])
def test_fit_reads_the_device_once_per_epoch(monkeypatch, with_validation):
    """Tensor.item / cpu / tolist on a device tensor are the reads counted, and so are the other ways a device value reaches the
    host: Tensor.to with a host result, float() / int() / bool() / an index made of a device tensor.  None of
    torch.cuda.synchronize, Stream.synchronize, Event.synchronize may be called."""
    cfg = _config(2)
    data = [_cuda(b) for b in _batches(41, [2] * 8, 2)]
    val = [_cuda(b) for b in _batches(43, [2] * 4, 2)]
    tr = Trainer(Model(cfg, dtype="bfloat16", seed=0), Adam(1e-3))
    tr.fit(iter(data[:1]), 1, 1)                                    # first use: workspaces, weight packing
    torch.cuda.synchronize()
    counts = {"item": 0, "cpu": 0, "tolist": 0, "other": 0, "sync": 0}
    per_epoch = []

    def counting(name, original):
        def wrapper(self, *a, **k):
            if self.is_cuda:
                counts[name] += 1
            return original(self, *a, **k)
        return wrapper

    def sync_counting(original):
        def wrapper(*a, **k):
            counts["sync"] += 1
            return original(*a, **k)
        return wrapper

    for name in ("item", "cpu", "tolist"):
        monkeypatch.setattr(torch.Tensor, name, counting(name, getattr(torch.Tensor, name)))
    for name in ("__float__", "__int__", "__bool__", "__index__", "__complex__"):
        monkeypatch.setattr(torch.Tensor, name, counting("other", getattr(torch.Tensor, name)))
    original_to = torch.Tensor.to

    def counting_to(self, *a, **k):
        out = original_to(self, *a, **k)
        if self.is_cuda and not out.is_cuda:
            counts["other"] += 1
        return out

    monkeypatch.setattr(torch.Tensor, "to", counting_to)
    monkeypatch.setattr(torch.cuda, "synchronize", sync_counting(torch.cuda.synchronize))
    monkeypatch.setattr(torch.cuda.Stream, "synchronize", sync_counting(torch.cuda.Stream.synchronize))
    monkeypatch.setattr(torch.cuda.Event, "synchronize", sync_counting(torch.cuda.Event.synchronize))

    class Snapshot:
        def on_epoch_end(self, epoch, logs):
            per_epoch.append(dict(counts))

    kwargs = dict(validation_data=iter(val), validation_steps=2) if with_validation else {}
    h = tr.fit(iter(data), 4, 2, callbacks=[Snapshot()], **kwargs)  # the snapshot callback reads nothing itself
    monkeypatch.undo()
    assert per_epoch == [{"item": 0, "cpu": 1, "tolist": 0, "other": 0, "sync": 0},
                         {"item": 0, "cpu": 2, "tolist": 0, "other": 0, "sync": 0}], per_epoch
    assert counts == {"item": 0, "cpu": 2, "tolist": 0, "other": 0, "sync": 0}
    assert len(h.history["loss"]) == 2 and ("val_loss" in h.history) == with_validation


# ------------------------------------------------------------------------------------------------ checkpoints and logs
class _QuadReader:
    """in-memory data set: textured RGB images with one quad each"""

    def __init__(self, seed, count, side=64):
        rng = np.random.default_rng(seed)
        self._images, self._markup = {}, {}
        from PIL import Image
        for k in range(count):
            x0, y0 = int(rng.integers(4, side // 2 - 8)), int(rng.integers(4, side // 2 - 8))
            x1, y1 = x0 + int(rng.integers(16, side // 2)), y0 + int(rng.integers(16, side // 2))
            lab = np.zeros((1, side, side), np.int32)
            lab[0, y0:y1, x0:x1] = 1
            self._images[f"im{k}"] = Image.fromarray(synthetic.textured_images(seed + k, lab, 1, 3)[0])
            self._markup[f"im{k}"] = [ObjectMarkup(np.array([x0, y0, x1, y0, x1, y1, x0, y1]))]

    def read_markup(self):
        pass

    def get_list_of_images(self):
        return list(self._images)

    def get_image_markup(self, name):
        return self._markup[name]

    def get_image(self, name):
        return self._images[name]


def test_fit_writes_the_reference_files(tmp_path):
    cfg = _config(0)
    log_dir = str(tmp_path)
    train_gen = BatchGenerator(None, 2, _QuadReader(1, 6), cfg, name="train")
    train_eval_gen = BatchGenerator(None, 2, _QuadReader(1, 6), cfg, name="train_eval")
    val_gen = BatchGenerator(None, 2, _QuadReader(2, 4), cfg, name="valid")
    snapshots = []

    class Recorder:
        def set_trainer(self, trainer):
            self.trainer = trainer

        def on_epoch_end(self, epoch, logs):
            snapshots.append((logs["val_loss"], self.trainer.model.params.clone()))

    tr = Trainer(Model(cfg, seed=0), Adam(1e-3))
    callbacks = kc.build_callbacks_list(log_dir, cfg, train_eval_gen, val_gen, max_evaluated_images=4) + [Recorder()]
    tr.fit(train_gen.generate(), train_gen.get_epoch_size(), 2, validation_data=val_gen.generate(), validation_steps=2,
           callbacks=callbacks)
    for name in ("model.h5", "model_best.h5", os.path.join("backup", "model_001.h5"), os.path.join("backup", "model_002.h5")):
        assert os.path.isfile(os.path.join(log_dir, name)), name
    assert sorted(os.listdir(os.path.join(log_dir, "backup"))) == ["model_001.h5", "model_002.h5"]

    def load(name):
        m = Model(cfg, seed=1)
        m.load_keras_h5(os.path.join(log_dir, name))
        return m.params

    assert torch.equal(load("model.h5"), tr.model.params)
    assert torch.equal(load(os.path.join("backup", "model_001.h5")), snapshots[0][1])
    best = 0 if not snapshots[1][0] < snapshots[0][0] else 1          # strict decrease only
    assert torch.equal(load("model_best.h5"), snapshots[best][1])
    assert not torch.equal(snapshots[0][1], snapshots[1][1])
    metric_names = ["loss"] + keras_metrics.get_all_metrics(False)
    for mode in ("train", "valid"):
        lines = [json.loads(s) for s in open(os.path.join(log_dir, mode, "scalars.jsonl"))]
        assert [ln["epoch"] for ln in lines] == [0, 1]
        for ln in lines:
            keys = set(ln)
            assert not any(k.startswith("val") for k in keys)
            assert set(metric_names) <= keys and ("lr" in keys) == (mode == "train")
            # the object-level keys of ModelRunner.run
            assert {"f1_iou0.50", "pr_iou0.50", "recall_iou0.50", "detection_rate_iou0.50", "average_iou_by_area"} <= keys
    valid_lines = [json.loads(s) for s in open(os.path.join(log_dir, "valid", "scalars.jsonl"))]
    assert [ln["loss"] for ln in valid_lines] == [s[0] for s in snapshots]
