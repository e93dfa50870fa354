"""CPU: the scale rule and the two-piece fp16 split of ubdvss_amd/csrc/split2h.h, built for the host.

The header's rule and rounding are plain C++ (the device-only helpers are compiled out), and the weight pack of the Winograd layer
(pack_wino6h_kernel) uses exactly that text, so a small program around it checks, on 1e5 random fp32 values and the corner values:
  * under the scale s of the set's largest magnitude the two pieces reproduce x s to 2^-22 |x s| + 2^-25 and are finite fp16 values;
  * multiplying the inputs by 2^k changes the scale and nothing else: the pieces are the same bits;
  * the scale and its inverse are finite normal numbers for 0 (where both are 1), subnormals, 3e38, Inf and NaN patterns;
  * the rounding is numpy's float32 -> float16 (round to nearest even, subnormals kept).
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "split2h.h"
// in: int32 top, int32 lo, uint32 maxbits, int32 count, float32 x[count];  out: uint32 s_bits, inv_bits, then float32 h1, h2 per value
int main(int argc, char **argv)
{
    FILE *f = fopen(argv[1], "rb");
    int top, lo, count; unsigned maxbits;
    if (!f || fread(&top, 4, 1, f) != 1 || fread(&lo, 4, 1, f) != 1 || fread(&maxbits, 4, 1, f) != 1 || fread(&count, 4, 1, f) != 1) return 2;
    std::vector<float> x(count), out(2 * (size_t)count);
    if (count && fread(x.data(), 4, count, f) != (size_t)count) return 2;
    fclose(f);
    unsigned sb[2];
    split2h_scale(maxbits, top, lo, sb[0], sb[1]);
    const float s = split2h_float(sb[0]);
    for (int i = 0; i < count; ++i) split2h_pieces(x[i] * s, out[2 * i], out[2 * i + 1]);
    f = fopen(argv[2], "wb");
    fwrite(sb, 4, 2, f);
    fwrite(out.data(), 4, out.size(), f);
    fclose(f);
    return 0;
}
"""

TOPS = {"sample": (13, 40), "weight": (12, 90)}          # SPLIT2H_*_TOP / _LO


@pytest.fixture(scope="module")
def split(tmp_path_factory):
    work = tmp_path_factory.mktemp("split2h")
    compiler = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert compiler, "a host C++ compiler is needed to build split2h.h for the CPU"
    (work / "split.cpp").write_text(PROGRAM)
    subprocess.check_call([compiler, "-O1", "-std=c++17", "-I", os.path.join(ROOT, "ubdvss_amd", "csrc"), "-o", str(work / "split"), str(work / "split.cpp")])

    def run(kind, x, maxbits=None):
        """(s, 1 / s, h1, h2) for the values x under the scale of their largest magnitude (or of the given bit pattern)"""
        x = np.asarray(x, np.float32)
        top, lo = TOPS[kind]
        if maxbits is None:
            maxbits = int(np.abs(x).max().view(np.uint32)) if x.size else 0
        with open(work / "in.bin", "wb") as f:
            f.write(np.array([top, lo], np.int32).tobytes() + np.array([maxbits], np.uint32).tobytes() + np.array([x.size], np.int32).tobytes() + x.tobytes())
        subprocess.check_call([str(work / "split"), str(work / "in.bin"), str(work / "out.bin")])
        raw = np.fromfile(str(work / "out.bin"), np.uint32)
        s, inv = raw[:2].view(np.float32)
        h = raw[2:].view(np.float32).reshape(-1, 2)
        return float(s), float(inv), h[:, 0], h[:, 1]
    return run


def _values(seed):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(100000) * np.exp2(rng.integers(-12, 1, 100000))).astype(np.float32)        # thirteen binades below the largest
    x[:4] = (0.0, -0.0, x.max(), -x.max())
    return x


def _is_f16(h):
    with np.errstate(over="ignore"):
        return np.array_equal(h.astype(np.float16).astype(np.float32), h)


@pytest.mark.parametrize("kind", ["sample", "weight"])
def test_two_pieces_reproduce_the_scaled_value(split, kind):
    x = _values(1)
    s, inv, h1, h2 = split(kind, x)
    top = TOPS[kind][0]
    assert s * inv == 1.0 and 2.0 ** top <= float(np.abs(x).max()) * s < 2.0 ** (top + 1)
    assert np.isfinite(h1).all() and np.isfinite(h2).all() and _is_f16(h1) and _is_f16(h2)
    xs = x.astype(np.float64) * s
    err = np.abs(xs - (h1.astype(np.float64) + h2.astype(np.float64)))
    assert (err <= 2.0 ** -22 * np.abs(xs) + 2.0 ** -25).all(), float((err - 2.0 ** -22 * np.abs(xs)).max())
    # the rounding is numpy's: h1 = f16(x s), h2 = f16(x s - h1)
    xs32 = x * np.float32(s)
    assert np.array_equal(h1, xs32.astype(np.float16).astype(np.float32))
    assert np.array_equal(h2, (xs32 - h1).astype(np.float16).astype(np.float32))


def test_largest_sample_after_the_transform_stays_finite(split):
    """the kernel scales by max |T| and splits V with |V| <= 2 max |T|: twice the largest value is still a finite fp16 value"""
    x = np.array([1.9999999, -3.9999998, 3.9999998], np.float32)
    s, _, h1, h2 = split("sample", x, maxbits=int(np.float32(1.9999999).view(np.uint32)))
    assert s == 2.0 ** 13 and np.isfinite(h1).all() and np.isfinite(h2).all() and float(np.abs(h1).max()) == 32768.0


@pytest.mark.parametrize("k", [-30, -2, 1, 30])
def test_power_of_two_inputs_change_only_the_scale(split, k):
    x = _values(2)
    s0, inv0, a1, a2 = split("sample", x)
    s1, inv1, b1, b2 = split("sample", x * np.float32(2.0 ** k))
    assert s1 == s0 * 2.0 ** -k and inv1 == inv0 * 2.0 ** k
    assert np.array_equal(a1.view(np.uint32), b1.view(np.uint32)) and np.array_equal(a2.view(np.uint32), b2.view(np.uint32))


@pytest.mark.parametrize("kind", ["sample", "weight"])
def test_scale_is_finite_and_normal_for_every_bit_pattern_of_the_maximum(split, kind):
    tiny = float(np.finfo(np.float32).tiny)
    for bits in (0, 1, 0x007fffff, 0x00800000, int(np.float32(1e-30).view(np.uint32)), int(np.float32(3e38).view(np.uint32)), 0x7f7fffff,
                 0x7f800000, 0x7fc00000):
        s, inv, _, _ = split(kind, [], maxbits=bits)
        assert np.isfinite(s) and np.isfinite(inv) and s >= tiny and inv >= tiny and s * inv == 1.0, hex(bits)
        if bits == 0:
            assert s == 1.0 and inv == 1.0
    # the smallest inverse scales of the two factors multiply to an fp32 number (the kernel forms that product)
    assert split("sample", [], maxbits=1)[1] * split("weight", [], maxbits=1)[1] == 2.0 ** -149
