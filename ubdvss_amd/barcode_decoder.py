"""The digits of the retail symbols (EAN-13, UPC-A, EAN-8) in the object patches, decoded on the MI355X where
``extract_objects_on_device`` left them (``ubd_decode_patches``, include/ubd.h): 64 bytes per object come back instead of the
patch.  The rules are written out in include/ubd.h; tests/decode_oracle.py restates them and the device matches it bit for bit.
A patch may be the half-turned one (object_patches.py): both reading directions are tried and the result says which one read."""
import collections
import ctypes

import numpy as np
import torch

from . import _lib

EAN13, EAN8 = 1, 2                                       # bits of ``symbologies``
DEFAULT_PARAMS = dict(symbologies=EAN13 | EAN8, scan_rows=8, band=1, window=16, contrast=24, quiet=3, min_votes=2)
RESULT_INTS = 16

DecodedBarcode = collections.namedtuple("DecodedBarcode", ["symbology", "text", "votes", "upside_down", "is_upc_a"])
DecodedBarcode.__doc__ = """One decoded object.  symbology: 'EAN-13' or 'EAN-8'; text: all its digits, the check digit included;
votes: the (scan line, direction) readings that agreed; upside_down: the patch was read right to left only (it is the half-turned
one); is_upc_a: an EAN-13 whose first digit is 0 (its UPC-A number is text[1:])."""


def make_params(**params):
    """keyword parameters over DEFAULT_PARAMS -> the ``UbdDecodeParams`` of the C entry point; an unknown name is an error"""
    unknown = sorted(set(params) - set(DEFAULT_PARAMS))
    if unknown:
        raise TypeError(f"unknown decoder parameters {unknown}; known: {sorted(DEFAULT_PARAMS)}")
    merged = dict(DEFAULT_PARAMS, **params)
    return _lib.UbdDecodeParams(*[int(merged[k]) for k, _ in _lib.UbdDecodeParams._fields_])


def decode_patches_on_device(patches, counts, **params):
    """``patches``: uint8 device tensor (n, cap, patch_h, patch_w, c) and ``counts``: int32 (n), as ``extract_objects_on_device``
    writes and takes them (counts may be a host array).  ``params``: symbologies, scan_rows, band, window, contrast, quiet,
    min_votes (DEFAULT_PARAMS; ranges in include/ubd.h).  Returns the int32 device tensor (n, cap, 16) of ``ubd_decode_patches``:
    [symbology 0 / 13 / 8, votes, direction mask, 13 digits or -1]; rows of slots that hold no object are all zero.
    One launch on the current stream; nothing is read back."""
    if not torch.cuda.is_available():
        raise RuntimeError("decode_patches_on_device needs an MI355X; there is no CPU fallback")
    if not (isinstance(patches, torch.Tensor) and patches.is_cuda and patches.dtype == torch.uint8 and patches.dim() == 5):
        raise ValueError("patches must be a uint8 device tensor (n, cap, patch_h, patch_w, c)")
    lib = _lib.load()
    p = make_params(**params)
    device = patches.device
    patches = patches.contiguous()
    n, cap, ph, pw, c = (int(v) for v in patches.shape)
    if isinstance(counts, torch.Tensor):
        counts = counts.to(device=device, dtype=torch.int32, non_blocking=True).contiguous()
    else:
        counts = torch.from_numpy(np.ascontiguousarray(np.asarray(counts), dtype=np.int32)).to(device, non_blocking=True)
    if tuple(counts.shape) != (n,):
        raise ValueError(f"counts must be ({n},), got {tuple(counts.shape)}")
    results = torch.zeros((n, cap, RESULT_INTS), dtype=torch.int32, device=device)
    stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    with torch.cuda.device(device):
        _lib.check(lib.ubd_decode_patches(patches.data_ptr(), counts.data_ptr(), n, cap, ph, pw, c, ctypes.byref(p), results.data_ptr(),
                                          stream), "ubd_decode_patches")
    return results


def results_to_records(results, counts):
    """(n, cap, 16) results (device tensor or array) and counts (n) -> per image a list of min(counts[i], cap) entries, a
    ``DecodedBarcode`` or None where nothing was read"""
    r = results.cpu().numpy() if isinstance(results, torch.Tensor) else np.asarray(results)
    c = counts.cpu().numpy() if isinstance(counts, torch.Tensor) else np.asarray(counts)
    out = []
    for i in range(r.shape[0]):
        row = []
        for j in range(min(int(c[i]), r.shape[1])):
            code, votes, mask = (int(v) for v in r[i, j, :3])
            if code == 0:
                row.append(None)
                continue
            text = "".join(str(int(d)) for d in r[i, j, 3:3 + code])
            row.append(DecodedBarcode("EAN-13" if code == 13 else "EAN-8", text, votes, mask == 2, code == 13 and text[0] == "0"))
        out.append(row)
    return out
