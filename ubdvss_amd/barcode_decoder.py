"""The digits of the retail symbols (EAN-13, UPC-A, EAN-8) in the object patches, decoded on the MI355X where
``extract_objects_on_device`` left them (``ubd_decode_patches``, include/ubd.h): 64 bytes per object come back instead of the
patch.  The rules are written out in include/ubd.h; tests/decode_oracle.py restates them and the device matches it bit for bit.
A patch may be the half-turned one (object_patches.py): both reading directions are tried and the result says which one read.
The text of Code 128 / GS1-128 symbols is a second kernel with a result row of its own (``ubd_decode_text_patches``, 128 bytes
per object; tests/text_decode_oracle.py): ``decode_text_patches_on_device`` and ``text_results_to_records``.  The two-width codes,
ITF and Code 39, are a third (``ubd_decode_width_patches``, 128 bytes per object; tests/width_decode_oracle.py):
``decode_width_patches_on_device`` and ``width_results_to_records``.  UPC-E, Code 93 and Codabar are further symbologies of the
three kernels (bits 6, 7 and 8; tests/extra_decode_oracle.py).  Beside the records stand three host helpers for what the device
leaves uninterpreted: ``upce_to_upca``, ``full_ascii`` (the shift pairs of Code 39 and Code 93) and ``code32_to_digits``.
The postal height-modulated codes POSTNET, PLANET, RM4SCC and KIX are a fourth kernel (``ubd_decode_postal_patches``, 128 bytes per
object; tests/postal_decode_oracle.py): ``decode_postal_patches_on_device``, ``postal_results_to_records`` and the helper
``kix_half_turned``.  Intelligent Mail and Australia Post are not read.
Data Matrix (ECC 200, the square sizes 10 x 10 to 26 x 26, Reed-Solomon corrected) is a fifth kernel (``ubd_decode_matrix_patches``,
128 bytes per object; tests/matrix_decode_oracle.py): ``decode_matrix_patches_on_device`` and ``matrix_results_to_records``.  It
wants square patches of at most 128 x 128.  The other 2-D codes are not read."""
import collections
import ctypes

import numpy as np
import torch

from . import _lib

EAN13, EAN8 = 1, 2                                       # bits of ``symbologies``
CODE128 = 4                                              # bit 2: read by ubd_decode_text_patches, not by ubd_decode_patches
ITF, CODE39 = 8, 16                                      # bits 3 and 4: read by ubd_decode_width_patches
UPCE, CODE93, CODABAR = 64, 128, 256                     # bits 6, 7, 8: read by the retail, the text and the two-width entry point; bit 5 is unassigned
ALL_SYMBOLOGIES = 479                                    # the run-width families; the postal family is beside it
POSTNET, PLANET, RM4SCC, KIX = 1024, 2048, 4096, 8192    # bits 10..13: read by ubd_decode_postal_patches; bit 9 is unassigned
POSTAL_SYMBOLOGIES = 15360
DATAMATRIX = 32768                                       # bit 15: read by ubd_decode_matrix_patches; bit 14 is unassigned
MATRIX_SYMBOLOGIES = DATAMATRIX
DEFAULT_PARAMS = dict(symbologies=EAN13 | EAN8, scan_rows=8, band=1, window=16, contrast=24, quiet=3, min_votes=2)
RESULT_INTS = 16
TEXT_RESULT_BYTES = 128
WIDTH_RESULT_BYTES = 128
POSTAL_RESULT_BYTES = 128
MATRIX_RESULT_BYTES = 128
FNC1, FNC2, FNC3, FNC4 = 0xF1, 0xF2, 0xF3, 0xF4          # text elements of a Code 128 result beside the ASCII codes 0..127
SHIFT1, SHIFT2, SHIFT3, SHIFT4 = 0xE1, 0xE2, 0xE3, 0xE4  # text elements of a Code 93 result: the shifts ($) (%) (/) (+)

DecodedBarcode = collections.namedtuple("DecodedBarcode", ["symbology", "text", "votes", "upside_down", "is_upc_a"])
DecodedBarcode.__doc__ = """One decoded object.  symbology: 'EAN-13', 'EAN-8' or 'UPC-E'; text: all its digits, the check digit included
(of a UPC-E the eight: number system, six digits, check digit; ``upce_to_upca`` gives its UPC-A number);
votes: the (scan line, direction) readings that agreed; upside_down: the patch was read right to left only (it is the half-turned
one); is_upc_a: an EAN-13 whose first digit is 0 (its UPC-A number is text[1:])."""

DecodedText = collections.namedtuple("DecodedText", ["symbology", "text", "votes", "upside_down", "gs1", "elements"])
DecodedText.__doc__ = """One decoded Code 128 or Code 93 object.  symbology: 'Code 128' or 'Code 93' (of a Code 93 text holds the data
characters, a shift as '\\xe1'..'\\xe4' for ($) (%) (/) (+), which ``full_ascii`` resolves; gs1 is False); text: its ASCII elements as a str, a leading FNC1 dropped
(it sets gs1), any later FNC1 as '\\x1d', FNC2..FNC4 left out; votes and upside_down as in DecodedBarcode; gs1: the first data
character is FNC1 (GS1-128); elements: every text element as a tuple of integers, ASCII codes 0..127 and 0xF1..0xF4 for FNC1..FNC4."""

DecodedWidth = collections.namedtuple("DecodedWidth", ["symbology", "text", "votes", "upside_down", "checked"])
DecodedWidth.__doc__ = """One decoded two-width object.  symbology: 'ITF', 'Code 39' or 'Codabar'; text: its digits or characters (of a Code 39
the data between the two '*'; Full ASCII pairs are left as they are; of a Codabar every character, its start and stop A..D included,
and checked says that all their values sum to 0 modulo 16); votes and upside_down as in DecodedBarcode; checked: the
last element is the optional check character of the rest (GS1's modulo 10 for ITF, modulo 43 for Code 39) -- it stays in text."""

DecodedPostal = collections.namedtuple("DecodedPostal", ["symbology", "text", "votes", "upside_down", "checked", "bars"])
DecodedPostal.__doc__ = """One decoded postal object.  symbology: 'POSTNET', 'PLANET', 'RM4SCC' or 'KIX'; text: its digits or characters,
the check digit or check character included (a KIX has none); votes and upside_down as in DecodedBarcode -- a KIX is never
upside_down: it is read as the patch lies, and of a half-turned one text is ``kix_half_turned`` of what it says; checked: the
symbol carries a check and it held (False only for a KIX); bars: the number of its bars."""

DecodedMatrix = collections.namedtuple("DecodedMatrix", ["symbology", "text", "size", "turns", "corrected", "gs1", "complete", "raw"])
DecodedMatrix.__doc__ = """One decoded Data Matrix object.  symbology: 'Data Matrix'; text: its elements as a str, each byte decoded as
Latin-1 (a FNC1 behind the first position is '\\x1d'); size: the modules per side, 10..26; turns: the quarter turns (counter-clockwise)
by which the patch shows the symbol turned; corrected: the codewords Reed-Solomon corrected; gs1: FNC1 stands in first position;
complete: the whole data was text -- False where a codeword outside the ASCII encodation (a latch to C40, Text, X12, EDIFACT or
Base 256, a macro, ECI, structured append) ended it; raw: that codeword and the data codewords behind it, as bytes (b'' if complete)."""


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
    CODE128 (``ubd_decode_text_patches`` takes CODE128, CODE93 or both; a Code 93 row is [93, votes, mask, D, 0, D, C, K, D elements]).  Returns the uint8 device tensor (n, cap, 128) of
    ``ubd_decode_text_patches``: [128 or 0, votes, direction mask, T, flags, D, start value, check value, T text elements, 0xFF..];
    rows of slots that hold no object read as "none": bytes 0..7 zero, the rest 0xFF.  One launch on the current stream;
    nothing is read back."""
    return _launch("ubd_decode_text_patches", patches, counts, dict({"symbologies": CODE128}, **params), TEXT_RESULT_BYTES, torch.uint8,
                   fill_from=8)


def decode_width_patches_on_device(patches, counts, **params):
    """``patches`` and ``counts`` as for ``decode_patches_on_device``; ``params`` the same keywords, ``symbologies`` defaulting to
    ITF | CODE39 (``ubd_decode_width_patches`` takes any of ITF, CODE39, CODABAR; byte 0 of a Codabar row is 27).  Returns the uint8 device tensor (n, cap, 128) of
    ``ubd_decode_width_patches``: [25, 39 or 0, votes, direction mask, T, flags, 0, 0, 0, T ASCII codes, 0xFF..]; rows of slots
    that hold no object read as "none": bytes 0..7 zero, the rest 0xFF.  One launch on the current stream; nothing is read back."""
    return _launch("ubd_decode_width_patches", patches, counts, dict({"symbologies": ITF | CODE39}, **params), WIDTH_RESULT_BYTES,
                   torch.uint8, fill_from=8)


def decode_postal_patches_on_device(patches, counts, **params):
    """``patches`` and ``counts`` as for ``decode_patches_on_device``; ``params`` the same keywords, ``symbologies`` defaulting to
    POSTAL_SYMBOLOGIES (``ubd_decode_postal_patches`` takes any of POSTNET, PLANET, RM4SCC, KIX).  Returns the uint8 device tensor
    (n, cap, 128) of ``ubd_decode_postal_patches``: [80, 76, 82, 75 or 0, votes, direction mask, T, flags, B bars, 0, 0,
    T ASCII codes, 0xFF..]; rows of slots that hold no object read as "none": bytes 0..7 zero, the rest 0xFF.  One launch on the
    current stream; nothing is read back."""
    return _launch("ubd_decode_postal_patches", patches, counts, dict({"symbologies": POSTAL_SYMBOLOGIES}, **params), POSTAL_RESULT_BYTES,
                   torch.uint8, fill_from=8)


def decode_matrix_patches_on_device(patches, counts, **params):
    """``patches`` and ``counts`` as for ``decode_patches_on_device``, the patch sides 32..128 (a square symbol wants a square
    patch: extract with ``patch_size=(128, 128)``); ``params`` the same keywords, ``symbologies`` defaulting to DATAMATRIX, the only
    value ``ubd_decode_matrix_patches`` takes; band is 0..2 here, and scan_rows, quiet and min_votes are checked but unused.
    Returns the uint8 device tensor (n, cap, 128) of ``ubd_decode_matrix_patches``: [68 or 0, modules per side, quarter turns, T,
    flags, corrected codewords, finder mismatches, U, T text elements, U raw codewords, 0xFF..]; rows of slots that hold no object
    read as "none": bytes 0..7 zero, the rest 0xFF.  One launch on the current stream; nothing is read back."""
    return _launch("ubd_decode_matrix_patches", patches, counts, dict({"symbologies": DATAMATRIX}, **params), MATRIX_RESULT_BYTES,
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
    if code == 93:
        return DecodedText("Code 93", "".join(chr(v) for v in elements), votes, mask == 2, False, elements)
    gs1 = bool(flags & 1)
    text = "".join("\x1d" if v == FNC1 else chr(v) for v in elements[1 if gs1 else 0:] if v < 128 or v == FNC1)
    return DecodedText("Code 128", text, votes, mask == 2, gs1, elements)


def _width_record(row):
    code, votes, mask, t, flags = (int(v) for v in row[:5])
    if code == 0:
        return None
    return DecodedWidth({25: "ITF", 39: "Code 39", 27: "Codabar"}[code], "".join(chr(int(v)) for v in row[8:8 + t]), votes, mask == 2, bool(flags & 1))


def _postal_record(row):
    code, votes, mask, t, flags, bars = (int(v) for v in row[:6])
    if code == 0:
        return None
    return DecodedPostal({80: "POSTNET", 76: "PLANET", 82: "RM4SCC", 75: "KIX"}[code], "".join(chr(int(v)) for v in row[8:8 + t]), votes,
                         mask == 2, bool(flags & 1), bars)


def _matrix_record(row):
    code, size, turns, t, flags, corrected, _, u = (int(v) for v in row[:8])
    if code == 0:
        return None
    return DecodedMatrix("Data Matrix", bytes(int(v) for v in row[8:8 + t]).decode("latin-1"), size, turns, corrected, bool(flags & 1),
                         not flags & 2, bytes(int(v) for v in row[8 + t:8 + t + u]))


def _retail_record(row):
    code, votes, mask = (int(v) for v in row[:3])
    if code == 0:
        return None
    text = "".join(str(int(d)) for d in row[3:3 + (8 if code == 6 else code)])
    return DecodedBarcode({13: "EAN-13", 8: "EAN-8", 6: "UPC-E"}[code], text, votes, mask == 2, code == 13 and text[0] == "0")


def text_results_to_records(results, counts):
    """(n, cap, 128) results of ``decode_text_patches_on_device`` (device tensor or array) and counts (n) -> per image a list of
    min(counts[i], cap) entries, a ``DecodedText`` or None where nothing was read"""
    return _records(results, counts, _text_record)


def width_results_to_records(results, counts):
    """(n, cap, 128) results of ``decode_width_patches_on_device`` (device tensor or array) and counts (n) -> per image a list of
    min(counts[i], cap) entries, a ``DecodedWidth`` or None where nothing was read"""
    return _records(results, counts, _width_record)


def postal_results_to_records(results, counts):
    """(n, cap, 128) results of ``decode_postal_patches_on_device`` (device tensor or array) and counts (n) -> per image a list of
    min(counts[i], cap) entries, a ``DecodedPostal`` or None where nothing was read"""
    return _records(results, counts, _postal_record)


def matrix_results_to_records(results, counts):
    """(n, cap, 128) results of ``decode_matrix_patches_on_device`` (device tensor or array) and counts (n) -> per image a list of
    min(counts[i], cap) entries, a ``DecodedMatrix`` or None where nothing was read"""
    return _records(results, counts, _matrix_record)


def results_to_records(results, counts):
    """(n, cap, 16) results (device tensor or array) and counts (n) -> per image a list of min(counts[i], cap) entries, a
    ``DecodedBarcode`` or None where nothing was read"""
    return _records(results, counts, _retail_record)


def upce_to_upca(text):
    """the eight digits of a UPC-E (number system, six digits, check digit; ``DecodedBarcode.text``) or its six middle digits with
    number system 0 -> the twelve digits of the UPC-A number it stands for, the check digit computed.  ValueError for anything else."""
    text = str(text)
    if not text.isdigit() or len(text) not in (6, 8) or (len(text) == 8 and text[0] not in "01"):
        raise ValueError(f"a UPC-E is six digits, or number system 0 / 1, six digits and a check digit; got {text!r}")
    ns, d = (text[0], text[1:7]) if len(text) == 8 else ("0", text)
    if d[5] in "012":
        body = d[0:2] + d[5] + "0000" + d[2:5]
    elif d[5] == "3":
        body = d[0:3] + "00000" + d[3:5]
    elif d[5] == "4":
        body = d[0:4] + "00000" + d[4]
    else:
        body = d[0:5] + "0000" + d[5]
    eleven = ns + body
    check = (10 - (3 * sum(int(c) for c in eleven[0::2]) + sum(int(c) for c in eleven[1::2])) % 10) % 10
    if len(text) == 8 and int(text[7]) != check:
        raise ValueError(f"the check digit of {text!r} should be {check}")
    return eleven + str(check)


_C39_SHIFTS = "$%/+"                                     # the four shift characters of Code 39 in the order of Code 93's SHIFT1..SHIFT4
_PERCENT = {**{chr(65 + k): chr(27 + k) for k in range(5)}, **{chr(70 + k): chr(59 + k) for k in range(5)},
            **{chr(75 + k): chr(91 + k) for k in range(5)}, **{chr(80 + k): chr(123 + k) for k in range(5)},
            "U": "\x00", "V": "@", "W": "`", "X": "\x7f", "Y": "\x7f", "Z": "\x7f"}


def full_ascii(text_or_elements):
    """The Full ASCII reading of a Code 39 text (``DecodedWidth.text``: the pairs $A %A /A +A are written with the data characters
    $ % / +) or of a Code 93 (``DecodedText.text`` or ``.elements``: the shifts are SHIFT1..SHIFT4, '\\xe1'..'\\xe4').  $A..$Z are
    the control characters 1..26, %A..%E 27..31, %F..%J ; < = > ?, %K..%O [ \\ ] ^ _, %P..%T { | } ~ DEL, %U NUL, %V @, %W `,
    %X..%Z DEL, /A../O ! .. /, /Z :, +A..+Z a..z.  In a str without SHIFT elements every $ % / + is a shift (Code 39); with
    elements, or a str that holds '\\xe1'..'\\xe4', only those are.  Returns the str, or None on an invalid pair."""
    items = [ord(c) for c in text_or_elements] if isinstance(text_or_elements, str) else [int(v) for v in text_or_elements]
    code93 = not isinstance(text_or_elements, str) or any(SHIFT1 <= v <= SHIFT4 for v in items)
    out, k = [], 0
    while k < len(items):
        v = items[k]
        shift = v - SHIFT1 if SHIFT1 <= v <= SHIFT4 else _C39_SHIFTS.find(chr(v)) if not code93 and v < 128 else -1
        if shift < 0:
            if v >= 128:
                return None
            out.append(chr(v))
            k += 1
            continue
        if k + 1 >= len(items) or not 65 <= items[k + 1] <= 90:
            return None
        letter = chr(items[k + 1])
        if shift == 0:
            out.append(chr(ord(letter) - 64))
        elif shift == 1:
            out.append(_PERCENT[letter])
        elif shift == 2:
            if letter <= "O":
                out.append(chr(ord(letter) - 32))
            elif letter == "Z":
                out.append(":")
            else:
                return None
        else:
            out.append(letter.lower())
        k += 2
    return "".join(out)


_CODE32 = "0123456789BCDFGHJKLMNPQRSTUVWXYZ"            # base 32 without the vowels


def code32_to_digits(text):
    """Code 32, the Italian pharmacode carried by a Code 39 of six characters: ``DecodedWidth.text`` -> its nine digits (eight and
    a check digit, printed behind an 'A'), or None where the text is no Code 32: another length or alphabet, a value of nine
    digits or more, or a check digit that does not hold (every second digit doubled, the digits of the products summed, modulo 10)."""
    text = str(text)
    if len(text) != 6 or any(c not in _CODE32 for c in text):
        return None
    value = 0
    for c in text:
        value = value * 32 + _CODE32.index(c)
    if value >= 10 ** 9:
        return None
    digits = f"{value:09d}"
    total = 0
    for k, c in enumerate(digits[:8]):
        v = int(c) * (2 if k % 2 else 1)
        total += v // 10 + v % 10
    return digits if total % 10 == int(digits[8]) else None


_FOUR_STATE = "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ"     # value = 6 * (ascender pattern) + (descender pattern)
_FOUR_TURNED = (5, 4, 2, 3, 1, 0)                        # a pattern of two long bars among four, read backwards: 0011 <-> 1100, 0101 <-> 1010


def kix_half_turned(text):
    """The text a KIX reads as when it lies half-turned: the characters in reverse order, and in each character the bars in
    reverse order with ascenders and descenders swapped.  That is always a valid KIX text, so the decoder cannot tell which way
    up a KIX is: it reads the patch as it lies, and the caller who knows the symbol to be half-turned takes this of the text.
    ValueError for a character outside 0-9 A-Z."""
    text = str(text)
    if any(ch not in _FOUR_STATE for ch in text):
        raise ValueError(f"a KIX holds the characters 0-9 and A-Z; got {text!r}")
    out = []
    for ch in reversed(text):
        up, down = divmod(_FOUR_STATE.index(ch), 6)
        out.append(_FOUR_STATE[6 * _FOUR_TURNED[down] + _FOUR_TURNED[up]])
    return "".join(out)
