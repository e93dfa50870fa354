"""Train step -- host mirror of ``model.compile(Adam(lr), loss)`` + the per-step body of
``fit_generator`` (train.py:110-112, :176-188): forward, loss, backward, (data-parallel gradient
all-reduce), Adam.

Multi-GPU: one process per GPU; when ``torch.distributed`` is initialised the flat fp32 gradient
vector (33 028 floats for the RGB model) is summed with ONE all-reduce over RCCL/xGMI and divided
by the world size inside the fused Adam kernel.  The loss (incl. its batch-global top-k) is
evaluated per replica (option 1).

``Trainer.fit`` / ``Trainer.evaluate`` are the loop itself (``fit_generator`` / ``evaluate_generator`` as train.py:176-188 uses
them): every step adds its loss vector to a device accumulator (``ubd_epoch_accumulate``) and the host reads the two
accumulators -- training and validation -- ONCE per epoch; nothing inside an epoch waits for the device.

A ``MultiscaleModel`` is trained through the multi-scale graph (train.py fits whichever model ``build_model`` returns): its train
steps are ``ubd_train_step_multiscale``, its validation steps the multi-scale forward, so ``loss`` and ``val_loss`` belong to one model.
With a native communicator the multi-scale step needs the explicit mode (``attach_native_comm(model, fused=False)``).
"""
import logging

import numpy as np
import torch

from . import _lib, distributed, keras_metrics
from .net import MultiscaleModel, PreprocessingType


class History:
    """keras.callbacks.History: ``epoch`` numbers and ``history[name]`` = the value of every epoch's log."""

    def __init__(self):
        self.epoch, self.history = [], {}

    def on_epoch_end(self, epoch, logs):
        self.epoch.append(epoch)
        for k, v in logs.items():
            self.history.setdefault(k, []).append(v)


class Adam:
    """keras.optimizers.Adam defaults (train.py:110): beta1 .9, beta2 .999, epsilon 1e-7."""

    def __init__(self, lr=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-7):
        self.lr, self.beta_1, self.beta_2, self.epsilon = lr, beta_1, beta_2, epsilon


class Trainer:
    def __init__(self, model, optimizer=None, process_group=None):
        self.model = model
        self.opt = optimizer or Adam()
        self._lib = _lib.load()
        n = model.count_params()
        dev = model.device
        self.grads = torch.zeros(n, dtype=torch.float32, device=dev)
        self.m = torch.zeros(n, dtype=torch.float32, device=dev)
        self.v = torch.zeros(n, dtype=torch.float32, device=dev)
        self.loss = torch.zeros(16, dtype=torch.float32, device=dev)
        self.iterations = 0
        self._ws = None
        self._pg = process_group
        # epoch logs: row 0 the training sums, row 1 the validation sums (include/ubd.h, ubd_epoch_accumulate); one tensor, one read
        self._epoch_slots = int(self._lib.ubd_epoch_accumulator_bytes()) // 8
        self._epoch_acc = torch.zeros((2, self._epoch_slots), dtype=torch.float64, device=dev)
        self._val_loss = torch.zeros(_lib.UBD_LOSS_FLOATS, dtype=torch.float32, device=dev)
        self._loss_ws = None

    def broadcast_weights(self, src=0):
        if getattr(self.model, "_native_comm", None):           # the handle's own RCCL communicator (ubd_broadcast_params)
            _lib.launch("ubd_broadcast_params", self.model.device, self.model._h, self.model.params.data_ptr(), self.model.params.numel(), src)
        else:
            if self._pg is not False:
                distributed.broadcast_parameters(self.model.params, src=src, group=self._pg)
        # c10d writes the tensor without bumping its version counter: invalidate the packed weight fragments
        self.model.invalidate_packed_weights()

    def backward_on_device(self, images, targets):
        """images: device tensor (N,H,W,C) float32 or uint8; targets: device int32 (N,H/4,W/4[,1]).
        Leaves gradients in self.grads and [total, det, cls, k] in self.loss.  A ``MultiscaleModel`` is trained through its own
        graph (``ubd_train_step_multiscale``: the loss of the mean map, the gradients of every level summed); height and width must
        then be multiples of ``model.side_multiple``."""
        mdl = self.model
        power = mdl.max_scale_power if isinstance(mdl, MultiscaleModel) else None
        images = images.contiguous()
        n, hh, ww, _ = images.shape
        if power is not None:
            if hh % mdl.side_multiple or ww % mdl.side_multiple:      # Model._input_form's wording with MultiscaleModel.predict_on_device's suffix
                raise ValueError(f"image height and width must be multiples of {mdl.side_multiple} "
                                 f"(4 * 2**max_scale_power, max_scale_power = {power})")
            if images.data_ptr() % 16:                              # an offset view: the pyramid gather loads 16-byte pieces
                images = images.clone()
        targets = targets.reshape(n, hh // 4, ww // 4).to(torch.int32).contiguous()
        if images.dtype == torch.uint8:
            in_dtype = _lib.UBD_IN_U8
            pre = _lib.UBD_PRE_MOBILENET if mdl.net_config.get_preprocessing_type() == PreprocessingType.MOBILENET_LIKE else _lib.UBD_PRE_NONE
        else:
            in_dtype, pre = _lib.UBD_IN_F32, _lib.UBD_PRE_NONE
        if power is None:
            nbytes = self._lib.ubd_train_workspace_bytes(mdl._h, n, hh, ww)
        else:
            nbytes = self._lib.ubd_train_multiscale_workspace_bytes(mdl._h, in_dtype, n, hh, ww, power)
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = torch.empty(int(nbytes), dtype=torch.uint8, device=mdl.device)
        if power is None:
            _lib.launch("ubd_train_step", mdl.device, mdl._h, mdl.params.data_ptr(), images.data_ptr(), in_dtype, pre,
                        targets.data_ptr(), n, hh, ww, self.grads.data_ptr(),
                        self.loss.data_ptr(), self._ws.data_ptr(), self._ws.numel())
        else:
            _lib.launch("ubd_train_step_multiscale", mdl.device, mdl._h, mdl.params.data_ptr(), images.data_ptr(), in_dtype, pre,
                        targets.data_ptr(), n, hh, ww, power, self.grads.data_ptr(),
                        self.loss.data_ptr(), self._ws.data_ptr(), self._ws.numel())

    def apply_gradients(self):
        native = getattr(self.model, "_native_comm", None)
        if native:                                              # C-ABI collective: fused into ubd_train_step, or explicit here
            world = self._lib.ubd_comm_world(self.model._h)
            if native == "explicit":
                _lib.launch("ubd_allreduce_grads", self.model.device, self.model._h, self.grads.data_ptr(), self.grads.numel())
            # per-replica losses are averaged; the batch-global loss (UBD_COMM_GLOBAL_LOSS) is ONE objective whose parameter
            # gradient is the sum of the ranks' contributions
            grad_scale = 1.0 if getattr(self.model, "_global_loss", False) else 1.0 / world
        elif self._pg is False:                                 # process_group=False: no collective at all, whatever torch.distributed holds
            grad_scale = 1.0                                    # (the timing reference of tools/dist_rccl_check.py: one GPU on its shard alone)
        else:
            grad_scale = distributed.allreduce_gradients(self.grads, group=self._pg)
        self.iterations += 1
        o = self.opt
        _lib.launch("ubd_adam_step", self.model.device, self.model.params.data_ptr(), self.grads.data_ptr(), self.m.data_ptr(),
                    self.v.data_ptr(), self.grads.numel(), self.iterations, o.lr, o.beta_1, o.beta_2, o.epsilon, grad_scale)
        self.model.invalidate_packed_weights()    # parameters changed behind torch's version counter

    def train_step_on_device(self, images, targets):
        self.backward_on_device(images, targets)
        self.apply_gradients()
        return self.loss

    def train_on_batch(self, images, targets):
        """Keras ``train_on_batch``: numpy batch in, scalar loss out.  Float images are fed as they are (already
        preprocessed, data_generators.py:113,148); uint8 images are raw pixels and get ``NetConfig``'s preprocessing
        fused into the first layer -- the same rule as every other entry point (Model.predict, ModelRunner.predict,
        *_on_device)."""
        dev = self.model.device
        x = np.asarray(images)
        if x.dtype != np.uint8:
            x = x.astype(np.float32)
        xt = torch.from_numpy(np.ascontiguousarray(x)).to(dev)     # uint8 stays uint8: NetConfig preprocessing fused on device
        yt = torch.from_numpy(np.ascontiguousarray(np.asarray(targets)).astype(np.int32)).to(dev)
        return float(self.train_step_on_device(xt, yt)[0].item())

    # ---------------------------------------------------------------- the loop (train.py:176-188)
    def _batch_on_device(self, images, targets):
        """One generator batch, numpy or tensors, on the model's device: uint8 images stay raw pixels (NetConfig's preprocessing
        is fused into the first layer), anything else is fed as float32 -- the rule of every other entry point."""
        dev = self.model.device
        if not torch.is_tensor(images):
            x = np.asarray(images)
            if x.dtype != np.uint8:
                x = x.astype(np.float32, copy=False)
            images = torch.from_numpy(np.ascontiguousarray(x))
        elif images.dtype != torch.uint8:
            images = images.to(torch.float32)
        if not torch.is_tensor(targets):
            targets = torch.from_numpy(np.ascontiguousarray(np.asarray(targets)).astype(np.int32))
        return images.to(dev, non_blocking=True), targets.to(device=dev, dtype=torch.int32, non_blocking=True)

    def _accumulate(self, loss, n_images, row):
        _lib.launch("ubd_epoch_accumulate", self.model.device, loss.data_ptr(), int(n_images), self._epoch_acc[row].data_ptr())

    def test_step_on_device(self, images, targets):
        """Keras' test-mode step: the inference forward pass and the loss without its gradient.  Leaves the 16 floats in the
        returned device vector (valid until the next call); no gradient, no Adam."""
        mdl = self.model
        logits = mdl.predict_on_device(images)
        n, mh, mw, _ = logits.shape
        targets = targets.reshape(n, mh, mw).to(torch.int32).contiguous()
        nbytes = int(self._lib.ubd_loss_workspace_bytes(mdl._h, n, mh, mw))
        if self._loss_ws is None or self._loss_ws.numel() < nbytes:
            self._loss_ws = torch.empty(nbytes, dtype=torch.uint8, device=mdl.device)
        _lib.launch("ubd_loss", mdl.device, mdl._h, logits.data_ptr(), targets.data_ptr(), n, mh, mw, self._val_loss.data_ptr(), None,
                    self._loss_ws.data_ptr(), self._loss_ws.numel())
        return self._val_loss

    def _run_steps(self, generator, steps, row, train):
        for _ in range(int(steps)):
            batch = next(generator)
            x, y = self._batch_on_device(batch[0], batch[1])
            loss = self.train_step_on_device(x, y) if train else self.test_step_on_device(x, y)
            self._accumulate(loss, x.shape[0], row)

    def _read_epoch_sums(self, rows=slice(0, 2)):
        """THE device-to-host read of an epoch: the accumulator rows asked for in one transfer, summed over the ranks first."""
        acc = self._epoch_acc[rows]
        if self._pg is not False and distributed.world_size(self._pg) > 1:     # also with a native communicator: it carries fp32 gradients only
            acc = distributed.allreduce_epoch_sums(acc, group=self._pg)
        return acc.cpu().numpy()

    def _is_chief(self):
        return self._pg is False or distributed.rank(self._pg) == 0

    def evaluate(self, generator, steps):
        """keras ``evaluate_generator``: ``steps`` batches of ``(images, targets)`` through the test-mode step; returns
        {name: size-weighted mean of the per-batch values} for ``loss`` and ``get_all_metrics`` (no prefix).  One read."""
        generator = iter(generator)
        self._epoch_acc[1].zero_()
        self._run_steps(generator, steps, 1, train=False)
        sums = self._read_epoch_sums(slice(1, 2))                   # the validation row alone
        return keras_metrics.epoch_logs_from_sums(sums[0], self.model.n_classes > 0)

    def fit(self, generator, steps_per_epoch, epochs, validation_data=None, validation_steps=None, callbacks=(), initial_epoch=0):
        """keras ``fit_generator`` as train.py:176-188 calls it.  ``generator`` / ``validation_data``: endless iterators of
        ``(images, targets)`` batches (numpy or device tensors; uint8 or float images), never restarted between epochs.  Per epoch:
        ``steps_per_epoch`` train steps, then ``validation_steps`` test-mode steps with the parameters the epoch ended with, then
        one read of the two device accumulators, then ``callback.on_epoch_end(epoch, logs)`` with the training means, the
        ``val_`` means and ``lr`` (a callback may change ``self.opt.lr``: the next ``ubd_adam_step`` takes it).  Within an
        epoch nothing reads the device or synchronises with it.  Returns a ``History``."""
        if validation_data is not None and not validation_steps:
            raise ValueError("validation_data needs validation_steps: the generators are endless")
        generator = iter(generator)
        validation_data = iter(validation_data) if validation_data is not None else None
        cls_mode = self.model.n_classes > 0
        history = History()
        callbacks = list(callbacks)

        def notify(method, *args):                               # every callback method is optional: a callback has the ones it needs
            for cb in callbacks:
                if hasattr(cb, method):
                    getattr(cb, method)(*args)

        notify("set_trainer", self)
        notify("on_train_begin")
        for epoch in range(int(initial_epoch), int(epochs)):
            self._epoch_acc.zero_()                              # on the stream, ahead of the epoch's first accumulate
            self._run_steps(generator, steps_per_epoch, 0, train=True)
            if validation_data is not None:
                self._run_steps(validation_data, validation_steps, 1, train=False)
            sums = self._read_epoch_sums()
            logs = keras_metrics.epoch_logs_from_sums(sums[0], cls_mode)
            if validation_data is not None:
                logs.update(keras_metrics.epoch_logs_from_sums(sums[1], cls_mode, prefix="val_"))
            for row, what in ((0, "training"), (1, "validation")):
                if sums[row][1] != 0:
                    logging.warning("epoch %d: the total loss of %d %s step(s) was not finite", epoch + 1, int(sums[row][1]), what)
            logs["lr"] = float(self.opt.lr)
            notify("on_epoch_end", epoch, logs)
            history.on_epoch_end(epoch, dict(logs))
        return history
