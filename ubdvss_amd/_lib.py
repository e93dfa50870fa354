"""ctypes binding of libubd_hip.so (include/ubd.h).  Fails loudly when the library is absent."""
import ctypes
import os

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# UBD_LIB_PATH: another build of the same library (the variant builds of csrc/build.sh under tools/_ab/; the stamped diagnostic build is
# loaded by tools/_diag.py, which sets LIB_PATH itself); never a fallback
LIB_PATH = os.environ.get("UBD_LIB_PATH") or os.path.join(_HERE, "libubd_hip.so")

UBD_F32, UBD_BF16, UBD_F16 = 0, 1, 2
UBD_IN_F32, UBD_IN_U8 = 0, 1
UBD_IN_PREPACKED = 0x100
UBD_PRE_NONE, UBD_PRE_MOBILENET = 0, 1
UBD_COMM_FUSED = 1
UBD_COMM_GLOBAL_LOSS = 2
UBD_UNIQUE_ID_BYTES = 128
ABI_VERSION = 3
UBD_WARP_COPY, UBD_WARP_AFFINE, UBD_WARP_PERSPECTIVE = 0, 1, 2
(UBD_PHOTO_AFFINE, UBD_PHOTO_GREY, UBD_PHOTO_FILTER3, UBD_PHOTO_SEP, UBD_PHOTO_BOX, UBD_PHOTO_NOISE,
 UBD_PHOTO_DROPOUT) = range(7)
UBD_PHOTO_MEDIAN, UBD_PHOTO_HSV, UBD_PHOTO_ELASTIC = 16, 17, 18
UBD_NA_IDENTITY, UBD_NA_FILTER3, UBD_NA_AFFINE = 0, 1, 2
UBD_NA_NEAREST, UBD_NA_LINEAR, UBD_NA_CUBIC = 0, 1, 2
UBD_NA_MAX, UBD_NA_AVG = 0, 1
UBD_EVAL_MAX_VERTS, UBD_EVAL_MAX_GT, UBD_EVAL_MAX_FOUND, UBD_EVAL_MAX_THRESHOLDS = 8, 256, 256, 16
UBD_EVAL_FLAG_OVERFLOW, UBD_EVAL_FLAG_BAD_GT = 1, 2
UBD_POLY_MAX_VERTS = 64
UBD_MAX_CLASSES = 31
UBD_LOSS_FLOATS = 16
UBD_EPOCH_VALUES = 11


class UbdConfig(ctypes.Structure):
    _fields_ = [("c_in", ctypes.c_int32), ("n_classes", ctypes.c_int32),
                ("fml_compatible", ctypes.c_int32), ("dtype", ctypes.c_int32)]


class UbdEvalRecord(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int32) for k in ("tp", "fp", "fn", "one_to_one", "one_to_many", "many_to_one", "matched_boxes_count",
                                              "detection_rate", "n_gt", "n_found", "flags", "reserved")] + \
               [(k, ctypes.c_double) for k in ("iou_sum", "precision_by_area", "recall_by_area", "iou_by_area")]


class UbdPixelRecord(ctypes.Structure):
    _fields_ = [("n_correct", ctypes.c_int64), ("n_total", ctypes.c_int64), ("n_objects", ctypes.c_int64),
                ("object_acc_sum", ctypes.c_double)]


class UbdDecodeParams(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int32) for k in ("symbologies", "scan_rows", "band", "window", "contrast", "quiet", "min_votes")]


# every symbol include/ubd.h declares: name -> (restype, argtypes)
_vp, _sz, _i = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
_f = ctypes.c_float
SIGNATURES = {
    "ubd_abi_version": (_i, []),
    "ubd_build_id": (ctypes.c_char_p, []),
    "ubd_last_error": (ctypes.c_char_p, []),
    "ubd_host_memcpy_mt": (_i, [_vp, _vp, _sz, _i]),
    "ubd_create": (_i, [ctypes.POINTER(UbdConfig), ctypes.POINTER(_vp)]),
    "ubd_destroy": (None, [_vp]),
    "ubd_param_count": (_sz, [_vp]),
    "ubd_num_cus": (_i, [_vp]),
    "ubd_forward_workspace_bytes": (_sz, [_vp, _i, _i, _i]),
    "ubd_train_workspace_bytes": (_sz, [_vp, _i, _i, _i]),
    "ubd_postprocess_workspace_bytes": (_sz, [_vp, _i, _i, _i, _i]),
    "ubd_loss_workspace_bytes": (_sz, [_vp, _i, _i, _i]),
    "ubd_forward": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "ubd_forward_postprocess": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _sz,
                                     _vp, _i, _i, _i, _f, _i, _f, _vp, _vp, _vp, _vp, _i, _vp, _sz, _vp]),
    "ubd_multiscale_levels_bytes": (_sz, [_i, _i, _i, _i, _i, _i]),
    "ubd_multiscale_gather": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _sz, _vp]),
    "ubd_multiscale_fuse": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "ubd_multiscale_fuse_backward": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "ubd_forward_multiscale_workspace_bytes": (_sz, [_vp, _i, _i, _i, _i, _i]),
    "ubd_forward_multiscale": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "ubd_pack_weights": (_i, [_vp, _vp, _vp, _sz, _vp]),
    "ubd_dilated_layer": (_i, [_vp, _vp, _i, _vp, _vp, _i, _i, _i, _vp, _vp]),
    "ubd_postprocess": (_i, [_vp, _vp, _i, _i, _i, _f, _i, _f, _vp, _vp, _vp, _vp, _i, _vp, _sz, _vp]),
    "ubd_loss": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "ubd_train_step": (_i, [_vp, _vp, _vp, _i, _i, _vp, _i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "ubd_train_multiscale_workspace_bytes": (_sz, [_vp, _i, _i, _i, _i, _i]),
    "ubd_train_step_multiscale": (_i, [_vp, _vp, _vp, _i, _i, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "ubd_adam_step": (_i, [_vp, _vp, _vp, _vp, _sz, _i, _f, _f, _f, _f, _f, _vp]),
    "ubd_epoch_accumulator_bytes": (_sz, []),
    "ubd_epoch_accumulate": (_i, [_vp, _i, _vp, _vp]),
    "ubd_build_label_maps": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "ubd_build_label_maps_polygons": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "ubd_segmap_polygons_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "ubd_segmap_polygons": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _sz, _vp]),
    "ubd_resize_images": (_i, [_vp, _vp, _vp, _i, _i, _vp, _i, _i, _i, _vp]),
    "ubd_warp_images": (_i, [_vp, _sz, _vp, _sz, _vp, _i, _i, _vp]),
    "ubd_extract_objects": (_i, [_vp, _sz, _vp, _vp, _i, _vp, _vp, _i, _i, _vp, ctypes.c_double, _vp, _i, _i, _vp, _vp]),
    "ubd_decode_patches": (_i, [_vp, _vp, _i, _i, _i, _i, _i, ctypes.POINTER(UbdDecodeParams), _vp, _vp]),
    "ubd_decode_text_patches": (_i, [_vp, _vp, _i, _i, _i, _i, _i, ctypes.POINTER(UbdDecodeParams), _vp, _vp]),
    "ubd_decode_width_patches": (_i, [_vp, _vp, _i, _i, _i, _i, _i, ctypes.POINTER(UbdDecodeParams), _vp, _vp]),
    "ubd_decode_postal_patches": (_i, [_vp, _vp, _i, _i, _i, _i, _i, ctypes.POINTER(UbdDecodeParams), _vp, _vp]),
    "ubd_decode_matrix_patches": (_i, [_vp, _vp, _i, _i, _i, _i, _i, ctypes.POINTER(UbdDecodeParams), _vp, _vp]),
    "ubd_photometric_images": (_i, [_vp, _sz, _vp, _sz, _vp, _i, _i, _vp]),
    "ubd_noise_alpha_images": (_i, [_vp, _sz, _vp, _sz, _vp, _vp, _sz, _i, _i, _vp]),
    "ubd_evaluate_accumulator_bytes": (_sz, [_i, _i]),
    "ubd_evaluate_workspace_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "ubd_evaluate_objects": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _i, _vp, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "ubd_evaluate_tables_layout": (_i, [_i, _i, _i, _i, _i, _vp, _vp]),
    "ubd_evaluate_polygons_workspace_bytes": (_sz, [_i, _i, _i, _i, _i, _i]),
    "ubd_evaluate_polygons": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _i, _vp, _i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "ubd_evaluate_polygons_tables_layout": (_i, [_i, _i, _i, _i, _i, _i, _vp, _vp]),
    "ubd_evaluate_pixels_accumulator_bytes": (_sz, []),
    "ubd_evaluate_pixels_workspace_bytes": (_sz, [_i, _i, _i]),
    "ubd_evaluate_pixels": (_i, [_vp, _i, _i, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "ubd_score_objects": (_i, [_vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "ubd_rank_buffer_bytes": (_sz, [ctypes.c_int64]),
    "ubd_rank_detections": (_i, [_vp, _vp, _i, _i, _vp, ctypes.c_int64, _vp, _vp, _i, _vp, ctypes.c_int64, _vp]),
    "ubd_visualize_images": (_i, [_vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ubd_comm_unique_id": (_i, [_vp]),
    "ubd_comm_init": (_i, [_vp, _vp, _i, _i, _i]),
    "ubd_comm_destroy": (_i, [_vp]),
    "ubd_comm_world": (_i, [_vp]),
    "ubd_allreduce_grads": (_i, [_vp, _vp, _sz, _vp]),
    "ubd_broadcast_params": (_i, [_vp, _vp, _sz, _i, _vp]),
}

_lib = None


def load():
    """Returns the loaded library; raises (never falls back) when it is missing or stale."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950).  ubdvss_amd has no CPU fallback.")
        lib = ctypes.CDLL(LIB_PATH)
        lib.ubd_abi_version.restype = ctypes.c_int
        lib.ubd_abi_version.argtypes = []
        if lib.ubd_abi_version() != ABI_VERSION:              # checked BEFORE the symbol table: a stale build says so instead of an AttributeError
            raise RuntimeError(f"{LIB_PATH}: ABI {lib.ubd_abi_version()} != expected {ABI_VERSION}; rebuild (ubdvss_amd/csrc/build.sh)")
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)          # AttributeError = stale build, surface it
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed (code {rc}): {load().ubd_last_error().decode()}")


# the entry points whose last C parameter is `void *stream` (tests/test_lib_call_host.py holds the set to include/ubd.h)
ON_STREAM = frozenset((
    "ubd_forward", "ubd_forward_postprocess", "ubd_multiscale_gather", "ubd_multiscale_fuse", "ubd_multiscale_fuse_backward",
    "ubd_forward_multiscale", "ubd_pack_weights", "ubd_dilated_layer", "ubd_postprocess", "ubd_loss", "ubd_train_step",
    "ubd_train_step_multiscale", "ubd_adam_step", "ubd_epoch_accumulate", "ubd_build_label_maps", "ubd_build_label_maps_polygons",
    "ubd_segmap_polygons", "ubd_resize_images", "ubd_warp_images", "ubd_extract_objects", "ubd_decode_patches",
    "ubd_decode_text_patches", "ubd_decode_width_patches", "ubd_photometric_images", "ubd_noise_alpha_images", "ubd_evaluate_objects",
    "ubd_evaluate_polygons", "ubd_evaluate_pixels", "ubd_score_objects", "ubd_rank_detections", "ubd_visualize_images",
    "ubd_allreduce_grads", "ubd_broadcast_params"))
# ON_STREAM is held to the header's `void *stream` declarations and to their number by tests/test_lib_call_host.py.  An entry
# point that came after that count was fixed takes its stream last as well, under the parameter name `hip_stream`, and is
# launched in the same way: LAUNCHED is what ``launch`` takes and ``call`` refuses (tests/test_postal_decode_host.py holds it to
# the header)
LAUNCHED = ON_STREAM | frozenset(("ubd_decode_postal_patches",))
# LAUNCHED in its turn is held to the declarations that end in `void *stream` or `void *hip_stream`.  An entry point that came
# after THAT was fixed takes its stream last under yet another name (`launch_stream`) and stands here: ``launch`` takes it as it
# takes LAUNCHED, ``call`` refuses it (tests/test_matrix_decode_host.py holds the set to the header)
LAUNCHED_LATER = frozenset(("ubd_decode_matrix_patches",))


def require_gpu(what):
    """The refusal of every entry point that needs the device; returns the torch module, for the modules that do not import it themselves."""
    if not torch.cuda.is_available():
        raise RuntimeError(f"{what} needs an MI355X; there is no CPU fallback")
    return torch


def current_stream(device):
    """the raw handle of ``device``'s current torch stream, for a caller that needs it beside the launch (a workspace key)"""
    return torch.cuda.current_stream(device).cuda_stream


def launch(name, device, *args, stream=None):
    """THE way to an entry point of LAUNCHED or LAUNCHED_LATER (ON_STREAM and the later ones): ``name(*args, stream)`` with ``device`` -- the device of the tensors in ``args``
    -- made current for the call, on that device's current torch stream, the return code checked on this thread
    (ubd_last_error is thread-local).  ``stream``: the handle of that same stream (``current_stream`` / ``Model._stream``) when the
    caller needed it before the call, for a workspace or packed-weights key.  Every step of forward, postprocess, train step and
    Adam comes through here: one stream lookup, one device guard, one check, nothing else."""
    if name not in LAUNCHED and name not in LAUNCHED_LATER:
        raise ValueError(f"{name} is not an entry point that takes a stream (_lib.ON_STREAM); checked entries without one go through _lib.call")
    fn = getattr(load(), name)
    if stream is None:
        stream = torch.cuda.current_stream(device).cuda_stream
    with torch.cuda.device(device):
        check(fn(*args, stream), name)


def call(name, *args, device=None):
    """A checked entry point that takes no stream (ubd_create, ubd_comm_*, the *_tables_layout): ``name(*args)``, with
    ``device`` current for the call when one is given.  The size queries and getters return no status: plain calls on ``load()``."""
    if name in LAUNCHED or name in LAUNCHED_LATER:
        raise ValueError(f"{name} takes a stream: it goes through _lib.launch")
    fn = getattr(load(), name)
    if device is None:
        check(fn(*args), name)
    else:
        with torch.cuda.device(device):
            check(fn(*args), name)


_static_handles = {}    # (n_classes, str(device)) -> handle of the static entry points (losses.loss_and_grad, SegmapManager.postprocess)


def static_handle(n_classes, device):
    """The cached ``UbdConfig(1, n_classes, 1, UBD_F32)`` handle of ``device``, created with that device current."""
    key = (n_classes, str(device))
    h = _static_handles.get(key)
    if h is None:
        cfg = UbdConfig(1, n_classes, 1, UBD_F32)
        h = ctypes.c_void_p()
        call("ubd_create", ctypes.byref(cfg), ctypes.byref(h), device=device)
        _static_handles[key] = h
    return h


def reset_static_handles():
    """Destroys the cached handles, each once, and empties the cache (they read the UBD_* test switches when they are created)."""
    lib = load()
    while _static_handles:
        lib.ubd_destroy(_static_handles.popitem()[1])


def to_device(a, dtype, device, non_blocking=False):
    """A tensor, or anything numpy takes as an array, as a contiguous tensor of the torch ``dtype`` on ``device``; a host array is
    converted on the host, so the bytes of the result are what crosses."""
    if isinstance(a, torch.Tensor):
        return a.to(device=device, dtype=dtype, non_blocking=non_blocking).contiguous()
    host = np.ascontiguousarray(np.asarray(a), dtype={torch.int32: np.int32, torch.float32: np.float32}[dtype])
    return torch.from_numpy(host).to(device, non_blocking=non_blocking)


class StreamWorkspaces:
    """Device scratch per (device, stream) for the static entry points (losses.get_loss, SegmapManager.postprocess): calls on one
    stream are ordered and may share a scratch, two streams never do.  Bounded: the least recently used entry goes when more than
    ``max_entries`` streams have been seen (a process that makes many short-lived streams would otherwise keep one full-size
    scratch per stream handle for ever; a dropped tensor returns to torch's caching allocator, which reuses it in stream order)."""

    def __init__(self, max_entries=8):
        import collections
        self._d = collections.OrderedDict()
        self._max = int(max_entries)

    def get(self, device, raw_stream, nbytes):
        import torch
        key = (str(device), int(raw_stream))
        ws = self._d.get(key)
        if ws is None or ws.numel() < nbytes:
            ws = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
        self._d[key] = ws
        self._d.move_to_end(key)
        while len(self._d) > self._max:
            self._d.popitem(last=False)
        return ws

    def __len__(self):
        return len(self._d)
