"""Oracle of the multi-scale model (reference net.py:44-59 ImageScaler, :368-389 _build_multiscale_model), in numpy.

* ``resize_bilinear_tf1``: TF1's legacy ``tf.image.resize_images`` (bilinear, align_corners=False) restated in fp32 in its GENERAL
  form -- in = out_index * (in_size / out_size), lo = floor(in), hi = min(ceil(in), in_size - 1), lerp = in - lo, rows then columns.
  Restated from the documented kernel; TensorFlow is not available where this runs, so parity with TF itself is unpinned.
* ``upsample_nearest``: Keras ``UpSampling2D(f)``, y[i // f, j // f].
* ``fuse_mean_f32``: the mean of the levels per channel, with the arithmetic the device fixes: fp32, acc = y_0, then += the
  upsampled levels in level order, then ONE division by float32(P + 1).
* ``fuse_mean_f64``, ``forward_f64``: the same in fp64 (no order to speak of), end to end on ``oracle.net_numpy.forward``.
"""
import numpy as np


def _resize_axis_tf1(x, out_size, axis):
    """one axis of the legacy bilinear resize, fp32: out = lo_value + (hi_value - lo_value) * lerp"""
    in_size = x.shape[axis]
    scale = np.float32(in_size) / np.float32(out_size)
    pos = np.arange(out_size, dtype=np.float32) * scale                  # fp32 product, as the kernel's float in = out * scale
    lo = np.floor(pos).astype(np.int64)
    hi = np.minimum(np.ceil(pos).astype(np.int64), in_size - 1)
    lerp = (pos - lo.astype(np.float32)).astype(np.float32)
    shape = [1] * x.ndim
    shape[axis] = out_size
    lerp = lerp.reshape(shape)
    a = np.take(x, lo, axis=axis).astype(np.float32)
    b = np.take(x, hi, axis=axis).astype(np.float32)
    return (a + (b - a) * lerp).astype(np.float32)


def resize_bilinear_tf1(x, out_h, out_w):
    """x: (N, H, W, C), any real dtype (uint8 is cast to fp32 as tf.image.resize_images does) -> fp32 (N, out_h, out_w, C).
    The legacy kernel interpolates along x inside a row pair first, then between the two rows; with the weights kept per axis the
    two orders are the same products here (a row's interpolation does not depend on the other axis)."""
    x = np.asarray(x).astype(np.float32)
    top = _resize_axis_tf1(x, out_w, axis=2)
    return _resize_axis_tf1(top, out_h, axis=1)


def pyramid_tf1(x, max_scale_power):
    """[x, x // 2, ..., x // 2**P] as the reference's ImageScaler builds them (integer division of the sizes), fp32"""
    n, h, w, _ = x.shape
    return [np.asarray(x).astype(np.float32)] + [resize_bilinear_tf1(x, h // 2 ** s, w // 2 ** s) for s in range(1, max_scale_power + 1)]


def decimate(x, s):
    return np.ascontiguousarray(np.asarray(x)[:, ::2 ** s, ::2 ** s, :])


def upsample_nearest(y, factor):
    return np.repeat(np.repeat(y, factor, axis=1), factor, axis=2)


def fuse_mean_f32(levels):
    """levels[s]: fp32 (N, h >> s, w >> s, K).  The device's arithmetic, operation for operation."""
    acc = np.asarray(levels[0], dtype=np.float32).copy()
    for s in range(1, len(levels)):
        acc = (acc + upsample_nearest(np.asarray(levels[s], dtype=np.float32), 2 ** s)).astype(np.float32)
    return (acc / np.float32(len(levels))).astype(np.float32)


def fuse_mean_f64(levels):
    acc = np.asarray(levels[0], dtype=np.float64).copy()
    for s in range(1, len(levels)):
        acc = acc + upsample_nearest(np.asarray(levels[s], dtype=np.float64), 2 ** s)
    return acc / float(len(levels))


def forward_f64(x, weights, max_scale_power, fml_compatible=True, preprocess=None):
    """x: (N, H, W, C), preprocessed -- or raw with ``preprocess`` (a per-pixel function, applied in fp64 to every level AFTER the
    resize: at the sizes the model accepts the resize only picks samples, so the order does not matter, and raw uint8 values
    are exact in the resize's fp32).  Returns (fused fp64 logits, the list of per-level fp64 logits).  The pyramid is the GENERAL
    bilinear resize (what the reference's graph does), not the slice."""
    from oracle import net_numpy as onet
    levels = []
    for xs in pyramid_tf1(np.asarray(x, dtype=np.float32), max_scale_power):
        xs = np.asarray(xs, dtype=np.float64)
        levels.append(onet.forward(preprocess(xs) if preprocess is not None else xs, weights, fml_compatible))
    return fuse_mean_f64(levels), levels
