"""NumPy oracle of batchImages (functions.py:456-501) for one to five pictures of any shapes, written out literally
over tests/tile_numpy.py's `resize_linear_u8` (OpenCV's 8-bit INTER_LINEAR path at any scale) and `_bgr`
(COLOR_GRAY2BGR). cv2.resize(stack, (0, 0), fx=s, fy=s) is restated as OpenCV computes its size:
dsize = (int(round(cols * fx)), int(round(rows * fy))), and then by the same path. That holds only where the stack's
size is an exact multiple of the scale (include/svx.h, sv_images_tile): elsewhere OpenCV takes its scale from fx and
not from the rounded dsize. tests/test_resize_cpu.py pins this oracle against tile_numpy's `tile` and `tile_closed`;
cv2 itself is absent here, so nothing is pinned to it.
"""
import numpy as np

import tile_numpy as tn


def resize_image(image, height, width):
    """functions.py:452-454: cv2.resize(image, (width, height))."""
    return tn.resize_linear_u8(image, width, height)


def _scaled(img, fx, fy):
    """cv2.resize(img, (0, 0), fx=fx, fy=fy)."""
    rows, cols = img.shape[:2]
    return tn.resize_linear_u8(img, int(round(cols * fx)), int(round(rows * fy)))


def batch_images(imgs, size):
    """batchImages([("", i) for i in imgs], size), size = (H, W), for 1 to 5 uint8 pictures (h, w) or (h, w, 3)."""
    counts = len(imgs)
    assert 1 <= counts <= 5
    images = [tn._bgr(resize_image(np.asarray(i), size[0], size[1])) for i in imgs]
    if counts == 1:
        return images[0]
    if counts == 2:
        return _scaled(np.hstack((images[0], images[1])), 0.5, 0.5)
    p1 = np.hstack((images[0], images[1]))
    p2 = np.hstack((images[2], images[2] if counts == 3 else images[3]))
    stack = np.vstack((p1, p2))
    if counts < 5:
        return _scaled(stack, 0.5, 0.5)
    return np.hstack((_scaled(stack, 0.25, 0.25), _scaled(images[4], 0.5, 0.5)))
