"""Oracle of the visualisations (semantic_segmentation/visualizations.py:20-151), not imported by the product.

Two statements of the same four overlays:
  * ``pillow_*``: the reference's own Pillow calls -- Image.blend with a solid colour at alpha 0.5, Image.composite through the
    mask, Image.resize(NEAREST) of a map to the image size, ImageDraw.polygon of every found quad.  Pillow is the third party
    that defines the numbers.
  * ``closed_*``: plain numpy, out = (in + color) >> 1 where the mask is set and out = in elsewhere, the mask of an integer
    ratio s taken as mask[y // s, x // s].
tests/test_visualization_host.py shows the two equal; the device is compared with the Pillow form.
"""
import numpy as np
from PIL import Image, ImageDraw

GREEN, RED = (0, 255, 0), (255, 0, 0)


def to_uint8(images, mobilenet=False):
    """denorm(images).astype(np.uint8) in float32, with the project's definition for values outside [0, 255]: clamped"""
    x = np.asarray(images)
    if x.dtype == np.uint8:
        return x
    x = x.astype(np.float32)
    if mobilenet:
        x = x * np.float32(127.5) + np.float32(127.5)      # two float32 roundings: product, then sum
    return np.clip(x, np.float32(0), np.float32(255)).astype(np.uint8)


def rgb(image):
    """(H, W, 3), (H, W, 1) or (H, W) uint8 -> PIL RGB image (a grey image through convert('RGB'))"""
    a = np.asarray(image, dtype=np.uint8)
    if a.ndim == 3 and a.shape[2] == 3:
        return Image.fromarray(np.ascontiguousarray(a))
    if a.ndim == 3:
        a = a[..., 0]
    return Image.fromarray(np.ascontiguousarray(a)).convert('RGB')


def pillow_draw(pil_image, mask_u8, color=GREEN):
    """draw_segmentation_map: mask_u8 (h, w) of 0 / 255, resized with NEAREST when smaller than the image"""
    m = Image.fromarray(np.ascontiguousarray(mask_u8, dtype=np.uint8))
    if m.size != pil_image.size:
        m = m.resize(pil_image.size, resample=Image.NEAREST)
    return Image.composite(Image.blend(pil_image, Image.new('RGB', pil_image.size, color=color), alpha=0.5), pil_image, m)


def pillow_segmentation(image, target, threshold=0.5):
    return np.array(pillow_draw(rgb(image), np.where(np.squeeze(np.asarray(target)) > threshold, 255, 0).astype(np.uint8)))


def pillow_classification(image, mask):
    """two passes, as the reference: green where the mask is 1, then red where it is -1"""
    mask = np.squeeze(np.asarray(mask))
    out = rgb(image)
    for value, color in ((1, GREEN), (-1, RED)):
        out = pillow_draw(out, np.where(mask == value, 255, 0).astype(np.uint8), color)
    return np.array(out)


def pillow_boxes(image, quads):
    """quads: iterable of 8 integers; every one filled with 255 at image resolution, then drawn green"""
    im = rgb(image)
    seg = Image.new(mode='L', size=im.size, color=0)
    draw = ImageDraw.Draw(seg)
    for q in quads:
        draw.polygon([int(v) for v in q], fill=255)
    return np.array(pillow_draw(im, np.asarray(seg)))


def pillow_all(images, gt=None, seg=None, quads=None, counts=None, cls=None, mobilenet=False):
    """The dict of Visualizer.compute_visualizations for the sources given (a source that is None gives no key).
    quads (n, cap, 8), counts (n): the first min(counts[i], cap) quads of image i are drawn."""
    u8 = to_uint8(images, mobilenet)
    out = {}
    if gt is not None:
        out["gt"] = np.stack([pillow_segmentation(im, t) for im, t in zip(u8, gt)])
    if seg is not None:
        out["seg_map"] = np.stack([pillow_segmentation(im, t) for im, t in zip(u8, seg)])
    if quads is not None:
        cap = quads.shape[1]
        out["postprocessed"] = np.stack([pillow_boxes(im, q[:min(int(c), cap)]) for im, q, c in zip(u8, quads, counts)])
    if cls is not None:
        out["classification_gt"] = np.stack([pillow_classification(im, m) for im, m in zip(u8, cls)])
    return out


# ---- the closed form ----------------------------------------------------------------------------------------------------------------
def closed_blend(image_rgb, mask, color=GREEN):
    """image_rgb (H, W, 3) uint8, mask (H, W) bool"""
    half = ((image_rgb.astype(np.int32) + np.asarray(color, dtype=np.int32)) >> 1).astype(np.uint8)
    return np.where(mask[..., None], half, image_rgb)


def closed_upscale(mask, height, width):
    """nearest for an integer ratio: mask[y // s, x // s]"""
    s = height // mask.shape[0]
    assert mask.shape[0] * s == height and mask.shape[1] * s == width
    return mask[np.arange(height)[:, None] // s, np.arange(width)[None, :] // s]


def closed_rgb(image):
    a = np.asarray(image, dtype=np.uint8)
    if a.ndim == 2:
        a = a[..., None]
    return np.repeat(a, 3, axis=2) if a.shape[2] == 1 else a


def closed_segmentation(image, target, threshold=0.5):
    im = closed_rgb(image)
    return closed_blend(im, closed_upscale(np.squeeze(np.asarray(target)) > threshold, im.shape[0], im.shape[1]))


def closed_classification(image, mask):
    """one pass: the +1 and the -1 pixels are disjoint"""
    im = closed_rgb(image)
    m = closed_upscale(np.squeeze(np.asarray(mask)), im.shape[0], im.shape[1])
    return closed_blend(closed_blend(im, m == 1, GREEN), m == -1, RED)
