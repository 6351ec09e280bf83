"""NumPy oracle of the image tile: batchImages (functions.py:456-501) for the five pictures stereovision.py:216
passes, all of the frame's size.

`tile` restates the function literally: grey -> BGR, hstack / vstack, then two calls of `resize_linear_u8`, OpenCV's
classic 8-bit INTER_LINEAR path for any scale (11-bit fixed-point coefficients rounded half to even in float32, an
int32 horizontal pass, the vertical pass's two >> 16 products and the final + 2 >> 2). `tile_closed` is the closed
form that path has at the two scales of the tile (include/svx.h, sv_image_tile): every weight is exactly 1/4, so the
byte is the mean of four samples rounded half up. tests/test_tile_cpu.py checks one against the other; cv2 itself is
absent here, so neither is pinned to it.
"""
import numpy as np

COEF_BITS = 11
COEF_ONE = 1 << COEF_BITS   # OpenCV's INTER_RESIZE_COEF_SCALE


def _coefficients(dn, sn):
    """Per destination index: the source index, the clamped next one and the two int16 coefficients."""
    scale = 1.0 / (dn / sn)                                        # double
    f = ((np.arange(dn, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(np.float32)).astype(np.float32)
    low, high = s < 0, s >= sn - 1
    f[low | high] = 0
    s[low] = 0
    s[high] = sn - 1
    one = np.float32(1.0)
    c0 = np.rint((one - f) * np.float32(COEF_ONE)).astype(np.int16)   # rint: half to even, in float32
    c1 = np.rint(f * np.float32(COEF_ONE)).astype(np.int16)
    return s, np.minimum(s + 1, sn - 1), c0.astype(np.int32), c1.astype(np.int32)


def resize_linear_u8(src, dw, dh):
    """cv2.resize(src, (dw, dh), interpolation=INTER_LINEAR) of a uint8 (H, W) or (H, W, C) image, OpenCV's 8-bit
    fixed-point path without its scale-2 area shortcut."""
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim in (2, 3)
    sh, sw = src.shape[:2]
    sx, sx1, a0, a1 = _coefficients(dw, sw)
    sy, sy1, b0, b1 = _coefficients(dh, sh)
    s = src.astype(np.int32)
    ext = (slice(None), slice(None)) + (None,) * (src.ndim - 2)
    a0, a1 = a0[None, :][ext], a1[None, :][ext]
    rows = s[:, sx] * a0 + s[:, sx1] * a1                          # the horizontal pass, int32
    b0, b1 = b0[:, None][ext], b1[:, None][ext]
    out = (((b0 * (rows[sy] >> 4)) >> 16) + ((b1 * (rows[sy1] >> 4)) >> 16) + 2) >> 2
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def _bgr(img):
    """cv2.cvtColor(img, COLOR_GRAY2BGR) of a grey image; a BGR one as it is."""
    return img if img.ndim == 3 else np.repeat(img[:, :, None], 3, axis=2)


def tile(disp, road_map, road, cleaned, result):
    """batchImages([.. five images ..], (H, W)), literally."""
    H, W = disp.shape
    images = [_bgr(resize_linear_u8(i, W, H)) for i in (disp, road_map, road, cleaned, result)]   # resizeImage
    stack = np.vstack((np.hstack((images[0], images[1])), np.hstack((images[2], images[3]))))
    left = resize_linear_u8(stack, int(round(stack.shape[1] * 0.25)), int(round(stack.shape[0] * 0.25)))
    right = resize_linear_u8(images[4], int(round(W * 0.5)), int(round(H * 0.5)))
    return np.hstack((left, right))


def road_map(bgr, road):
    """stereovision.py:131-133: the BGR with (0, 255, 0) at the road image's non-zero pixels."""
    out = bgr.copy()
    out[road != 0] = (0, 255, 0)
    return out


def mean4(a, b, c, d):
    return ((a.astype(np.int32) + b + c + d + 2) >> 2).astype(np.uint8)


def tile_closed(disp, road_map, road, cleaned, result):
    """The closed form (H and W multiples of 4): the stack at columns 4 dx + 1, 4 dx + 2 of rows 4 dy + 1, 4 dy + 2,
    the result's 2 x 2 blocks, each mean rounded half up."""
    H, W = disp.shape
    assert H % 4 == 0 and W % 4 == 0 and H >= 4 and W >= 4
    s = np.vstack((np.hstack((_bgr(disp), road_map)), np.hstack((_bgr(road), _bgr(cleaned)))))
    left = mean4(s[1::4, 1::4], s[1::4, 2::4], s[2::4, 1::4], s[2::4, 2::4])
    right = mean4(result[0::2, 0::2], result[0::2, 1::2], result[1::2, 0::2], result[1::2, 1::2])
    return np.hstack((left, right))
