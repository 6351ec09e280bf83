"""Test helper: a plain-numpy restatement of sanitiseRoadImage's morphology (functions.py:346-358).

The four operations the reference asks OpenCV for, with OpenCV's default morphology borders (pixels outside the
image count as clear for a dilation and as set for an erosion, so the border never sets or clears a pixel):

    1. close by a 9 x 9 rectangle   = dilate radius 4, then erode radius 4
    2. erode by 9 x 9, twice        = one erosion by 17 x 17 (radius 8)
    3. AND with mask != 0           (cv2.bitwise_and(img, img, mask=m); 128 keeps a pixel)
    4. close by 9 x 9 again

Every operation is rectangular, so it is done separably by shifted ORs / ANDs: along the rows first, then along
the columns. ParticleCleansing (functions.py:378-384) is the identity on the result (the property is
checked in tests/test_morph_cpu.py), so `sanitise` is the image sanitiseRoadImage returns, and `walk` its pixel
walk (functions.py:359-365). The oracle of tests/test_morph_cpu.py and tests/test_gpu_sanitise.py.
"""
import numpy as np


def _shifted(a, k, axis, fill):
    """b with b[i] = a[i + k] along `axis`, `fill` where i + k leaves the image."""
    out = np.full_like(a, fill)
    n = a.shape[axis]
    if abs(k) >= n:
        return out
    src = [slice(None)] * a.ndim
    dst = [slice(None)] * a.ndim
    if k >= 0:
        src[axis], dst[axis] = slice(k, n), slice(0, n - k)
    else:
        src[axis], dst[axis] = slice(0, n + k), slice(-k, n)
    out[tuple(dst)] = a[tuple(src)]
    return out


def _rect(a, r, erode):
    """Dilation (erode=False) or erosion by the (2r+1) x (2r+1) rectangle anchored at its centre."""
    for axis in (1, 0):   # rows first, then columns
        acc = a.copy()
        for k in range(1, r + 1):
            for s in (k, -k):
                t = _shifted(a, s, axis, erode)
                acc = (acc & t) if erode else (acc | t)
        a = acc
    return a


def dilate(a, r):
    return _rect(np.asarray(a, bool), r, False)


def erode(a, r):
    return _rect(np.asarray(a, bool), r, True)


def close(a, r):
    return erode(dilate(a, r), r)


def sanitise(img, mask=None):
    """Steps 1-4 on an H x W image (non-zero = set) and an optional H x W mask: H x W uint8 of 0 / 255."""
    b = np.asarray(img) != 0
    b = close(b, 4)
    b = erode(b, 8)
    if mask is not None:
        b = b & (np.asarray(mask) != 0)
    b = close(b, 4)
    return np.where(b, 255, 0).astype(np.uint8)


def walk(img, size=None):
    """[j, i] of every non-zero pixel in raster order (functions.py:359-365), (K, 2) int32; size = (height,
    width) restricts the walk to img[0:height, 0:width]."""
    a = np.asarray(img)
    if size is not None:
        a = a[: size[0], : size[1]]
    ys, xs = np.nonzero(a)
    return np.stack([xs, ys], axis=1).astype(np.int32)


def rectangles(rng, H, W, n, hmin=10, hmax=40, wmin=10, wmax=60, noise=0.002, anchors=()):
    """A seeded test image: n filled rectangles of hmin..hmax x wmin..wmax pixels at random places (they may hang
    over the frame's edges), further ones with their top-left corner at each (y, x) of `anchors` (so that a test can
    make them straddle a word, a band or the frame's edge), and `noise` of the pixels set at random."""
    img = np.zeros((H, W), np.uint8)
    spots = [(int(rng.integers(-hmax // 2, H)), int(rng.integers(-wmax // 2, W))) for _ in range(n)] + list(anchors)
    for y, x in spots:
        h, w = int(rng.integers(hmin, hmax + 1)), int(rng.integers(wmin, wmax + 1))
        img[max(y, 0): max(y + h, 0), max(x, 0): max(x + w, 0)] = 255
    img[rng.random((H, W)) < noise] = 255
    return img


def random_mask(rng, H, W):
    """A mask holding 0, 128 and 255 in large blocks (like road_threshold_mask.png: a region kept, a region cut)."""
    m = np.full((H, W), 255, np.uint8)
    m[:, : W // 5] = 0
    m[: H // 6, :] = 0
    m[H // 2:, W // 2:] = 128
    for _ in range(3):
        y, x = int(rng.integers(0, H)), int(rng.integers(0, W))
        m[y: y + H // 8 + 1, x: x + W // 8 + 1] = 0
    return m
