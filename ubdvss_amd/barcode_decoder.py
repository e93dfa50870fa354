"""The digits of the retail symbols (EAN-13, UPC-A, EAN-8) in the object patches, decoded on the MI355X where
``extract_objects_on_device`` left them (``ubd_decode_patches``, include/ubd.h): 64 bytes per object come back instead of the
patch.  The rules are written out in include/ubd.h; tests/decode_oracle.py restates them and the device matches it bit for bit.
A patch may be the half-turned one (object_patches.py): both reading directions are tried and the result says which one read.
The text of Code 128 / GS1-128 symbols is a second kernel with a result row of its own (``ubd_decode_text_patches``, 128 bytes
per object; tests/text_decode_oracle.py): ``decode_text_patches_on_device`` and ``text_results_to_records``.  The two-width codes,
ITF and Code 39, are a third (``ubd_decode_width_patches``, 128 bytes per object; tests/width_decode_oracle.py):
``decode_width_patches_on_device`` and ``width_results_to_records``."""
import collections
import ctypes

import numpy as np
import torch

from . import _lib

EAN13, EAN8 = 1, 2                                       # bits of ``symbologies``
CODE128 = 4                                              # bit 2: read by ubd_decode_text_patches, not by ubd_decode_patches
ITF, CODE39 = 8, 16                                      # bits 3 and 4: read by ubd_decode_width_patches
DEFAULT_PARAMS = dict(symbologies=EAN13 | EAN8, scan_rows=8, band=1, window=16, contrast=24, quiet=3, min_votes=2)
RESULT_INTS = 16
TEXT_RESULT_BYTES = 128
WIDTH_RESULT_BYTES = 128
FNC1, FNC2, FNC3, FNC4 = 0xF1, 0xF2, 0xF3, 0xF4          # text elements of a Code 128 result beside the ASCII codes 0..127

DecodedBarcode = collections.namedtuple("DecodedBarcode", ["symbology", "text", "votes", "upside_down", "is_upc_a"])
DecodedBarcode.__doc__ = """One decoded object.  symbology: 'EAN-13' or 'EAN-8'; text: all its digits, the check digit included;
votes: the (scan line, direction) readings that agreed; upside_down: the patch was read right to left only (it is the half-turned
one); is_upc_a: an EAN-13 whose first digit is 0 (its UPC-A number is text[1:])."""

DecodedText = collections.namedtuple("DecodedText", ["symbology", "text", "votes", "upside_down", "gs1", "elements"])
DecodedText.__doc__ = """One decoded Code 128 object.  symbology: 'Code 128'; text: its ASCII elements as a str, a leading FNC1 dropped
(it sets gs1), any later FNC1 as '\\x1d', FNC2..FNC4 left out; votes and upside_down as in DecodedBarcode; gs1: the first data
character is FNC1 (GS1-128); elements: every text element as a tuple of integers, ASCII codes 0..127 and 0xF1..0xF4 for FNC1..FNC4."""

DecodedWidth = collections.namedtuple("DecodedWidth", ["symbology", "text", "votes", "upside_down", "checked"])
DecodedWidth.__doc__ = """One decoded two-width object.  symbology: 'ITF' or 'Code 39'; text: its digits or characters (of a Code 39
the data between the two '*'; Full ASCII pairs are left as they are); votes and upside_down as in DecodedBarcode; checked: the
last element is the optional check character of the rest (GS1's modulo 10 for ITF, modulo 43 for Code 39) -- it stays in text."""


def make_params(**params):
    """keyword parameters over DEFAULT_PARAMS -> the ``UbdDecodeParams`` of the C entry point; an unknown name is an error"""
    unknown = sorted(set(params) - set(DEFAULT_PARAMS))
    if unknown:
        raise TypeError(f"unknown decoder parameters {unknown}; known: {sorted(DEFAULT_PARAMS)}")
    merged = dict(DEFAULT_PARAMS, **params)
    return _lib.UbdDecodeParams(*[int(merged[k]) for k, _ in _lib.UbdDecodeParams._fields_])


def _device_arguments(what, patches, counts):
    """the checks and conversions the entry points share -> (contiguous patches, device counts, shape)"""
    _lib.require_gpu(what)
    if not (isinstance(patches, torch.Tensor) and patches.is_cuda and patches.dtype == torch.uint8 and patches.dim() == 5):
        raise ValueError("patches must be a uint8 device tensor (n, cap, patch_h, patch_w, c)")
    device = patches.device
    patches = patches.contiguous()
    n = int(patches.shape[0])
    counts = _lib.to_device(counts, torch.int32, device, non_blocking=True)
    if tuple(counts.shape) != (n,):
        raise ValueError(f"counts must be ({n},), got {tuple(counts.shape)}")
    return patches, counts, tuple(int(v) for v in patches.shape)


def _launch(entry, patches, counts, params, row, dtype, fill_from=None):
    """one launch of the C entry point ``entry`` (ubd_X; its public function here is X_on_device) with the keyword ``params`` on
    the current stream -> its (n, cap, row) device results of ``dtype``; the rows start as zeros, with 0xFF from element
    ``fill_from`` on if that is given, which is what an unused slot keeps"""
    patches, counts, (n, cap, ph, pw, c) = _device_arguments(entry[len("ubd_"):] + "_on_device", patches, counts)
    p = make_params(**params)
    device = patches.device
    results = torch.zeros((n, cap, row), dtype=dtype, device=device)
    if fill_from is not None:
        results[:, :, fill_from:] = 0xFF
    _lib.launch(entry, device, patches.data_ptr(), counts.data_ptr(), n, cap, ph, pw, c, ctypes.byref(p), results.data_ptr())
    return results


def decode_patches_on_device(patches, counts, **params):
    """``patches``: uint8 device tensor (n, cap, patch_h, patch_w, c) and ``counts``: int32 (n), as ``extract_objects_on_device``
    writes and takes them (counts may be a host array).  ``params``: symbologies, scan_rows, band, window, contrast, quiet,
    min_votes (DEFAULT_PARAMS; ranges in include/ubd.h).  Returns the int32 device tensor (n, cap, 16) of ``ubd_decode_patches``:
    [symbology 0 / 13 / 8, votes, direction mask, 13 digits or -1]; rows of slots that hold no object are all zero.
    One launch on the current stream; nothing is read back."""
    return _launch("ubd_decode_patches", patches, counts, params, RESULT_INTS, torch.int32)


def decode_text_patches_on_device(patches, counts, **params):
    """``patches`` and ``counts`` as for ``decode_patches_on_device``; ``params`` the same keywords, ``symbologies`` defaulting to
    CODE128 (the only value ``ubd_decode_text_patches`` takes).  Returns the uint8 device tensor (n, cap, 128) of
    ``ubd_decode_text_patches``: [128 or 0, votes, direction mask, T, flags, D, start value, check value, T text elements, 0xFF..];
    rows of slots that hold no object read as "none": bytes 0..7 zero, the rest 0xFF.  One launch on the current stream;
    nothing is read back."""
    return _launch("ubd_decode_text_patches", patches, counts, dict({"symbologies": CODE128}, **params), TEXT_RESULT_BYTES, torch.uint8,
                   fill_from=8)


def decode_width_patches_on_device(patches, counts, **params):
    """``patches`` and ``counts`` as for ``decode_patches_on_device``; ``params`` the same keywords, ``symbologies`` defaulting to
    ITF | CODE39 (``ubd_decode_width_patches`` takes 8, 16 or 24).  Returns the uint8 device tensor (n, cap, 128) of
    ``ubd_decode_width_patches``: [25, 39 or 0, votes, direction mask, T, flags, 0, 0, 0, T ASCII codes, 0xFF..]; rows of slots
    that hold no object read as "none": bytes 0..7 zero, the rest 0xFF.  One launch on the current stream; nothing is read back."""
    return _launch("ubd_decode_width_patches", patches, counts, dict({"symbologies": ITF | CODE39}, **params), WIDTH_RESULT_BYTES,
                   torch.uint8, fill_from=8)


def _records(results, counts, parse):
    """per image the list of ``parse(row)`` over its min(counts[i], cap) result rows; ``parse`` gives None where nothing was read"""
    r = results.cpu().numpy() if isinstance(results, torch.Tensor) else np.asarray(results)
    c = counts.cpu().numpy() if isinstance(counts, torch.Tensor) else np.asarray(counts)
    return [[parse(r[i, j]) for j in range(min(int(c[i]), r.shape[1]))] for i in range(r.shape[0])]


def _text_record(row):
    code, votes, mask, t, flags = (int(v) for v in row[:5])
    if code == 0:
        return None
    elements = tuple(int(v) for v in row[8:8 + t])
    gs1 = bool(flags & 1)
    text = "".join("\x1d" if v == FNC1 else chr(v) for v in elements[1 if gs1 else 0:] if v < 128 or v == FNC1)
    return DecodedText("Code 128", text, votes, mask == 2, gs1, elements)


def _width_record(row):
    code, votes, mask, t, flags = (int(v) for v in row[:5])
    if code == 0:
        return None
    return DecodedWidth("ITF" if code == 25 else "Code 39", "".join(chr(int(v)) for v in row[8:8 + t]), votes, mask == 2, bool(flags & 1))


def _retail_record(row):
    code, votes, mask = (int(v) for v in row[:3])
    if code == 0:
        return None
    text = "".join(str(int(d)) for d in row[3:3 + code])
    return DecodedBarcode("EAN-13" if code == 13 else "EAN-8", text, votes, mask == 2, code == 13 and text[0] == "0")


def text_results_to_records(results, counts):
    """(n, cap, 128) results of ``decode_text_patches_on_device`` (device tensor or array) and counts (n) -> per image a list of
    min(counts[i], cap) entries, a ``DecodedText`` or None where nothing was read"""
    return _records(results, counts, _text_record)


def width_results_to_records(results, counts):
    """(n, cap, 128) results of ``decode_width_patches_on_device`` (device tensor or array) and counts (n) -> per image a list of
    min(counts[i], cap) entries, a ``DecodedWidth`` or None where nothing was read"""
    return _records(results, counts, _width_record)


def results_to_records(results, counts):
    """(n, cap, 16) results (device tensor or array) and counts (n) -> per image a list of min(counts[i], cap) entries, a
    ``DecodedBarcode`` or None where nothing was read"""
    return _records(results, counts, _retail_record)
