"""Training objectives -- host mirror of semantic_segmentation/losses.py:13-24.

``get_loss(classification_mode)`` returns a callable ``f(y_true, y_pred) -> scalar`` like the
reference; it evaluates the fused HIP loss kernel (weighted sigmoid-BCE with batch-global
hard-negative top-k, plus masked softmax-CE in classification mode) on the MI355X.
``loss_and_grad`` additionally returns d loss / d y_pred (what TF autodiff would produce).
"""
import torch

from . import _lib

# losses.py:13-17
L_POSITIVE_WEIGHT = 15.
L_NEGATIVE_WEIGHT = 1.
L_HARD_NEGATIVE_WEIGHT = 5.
L_DETECTION_WEIGHT = 1.
L_CLASSIFICATION_WEIGHT = 1.

_handles = _lib._static_handles        # the cache under its earlier name here: callers written against that name keep working
_workspaces = _lib.StreamWorkspaces()   # (device, stream) -> uint8 scratch reused between calls on that stream (grown on demand, LRU-bounded)


def loss_and_grad(y_true, y_pred, want_grad=True):
    """y_true (N,h,w,1) or (N,h,w) labels 0..n_cls; y_pred (N,h,w,1+n_cls) logits.
    Returns (loss4 device tensor [total, detection, classification, k], dlogits or None)."""
    _lib.require_gpu("ubdvss_amd.losses")
    lib = _lib.load()
    device = y_pred.device if isinstance(y_pred, torch.Tensor) and y_pred.is_cuda else torch.device(
        f"cuda:{torch.cuda.current_device()}")
    yp = _lib.to_device(y_pred, torch.float32, device)
    n, h, w, k = yp.shape
    yt = _lib.to_device(y_true, torch.int32, device).reshape(n, h, w)
    hd = _lib.static_handle(k - 1, device)
    loss = torch.zeros(16, dtype=torch.float32, device=device)
    grad = torch.empty_like(yp) if want_grad else None
    nbytes = int(lib.ubd_loss_workspace_bytes(hd, n, h, w))
    # one scratch per (device, stream): calls on one stream are ordered, two streams never share header / histograms
    stream = _lib.current_stream(device)
    ws = _workspaces.get(device, stream, nbytes)
    _lib.launch("ubd_loss", device, hd, yp.data_ptr(), yt.data_ptr(), n, h, w, loss.data_ptr(),
                grad.data_ptr() if grad is not None else None, ws.data_ptr(), ws.numel(), stream=stream)
    return loss, grad


def detection_loss(y_true, y_pred):
    """losses.py:33-44 (only channel 0 of y_pred is used)."""
    yp = y_pred[..., :1]
    return loss_and_grad(y_true, yp, want_grad=False)[0][1]


def detection_and_classification_loss(y_true, y_pred):
    """losses.py:47-62."""
    return loss_and_grad(y_true, y_pred, want_grad=False)[0][0]


def get_loss(classification_mode=False):
    """losses.py:20-24."""
    if classification_mode:
        return detection_and_classification_loss
    return detection_loss
