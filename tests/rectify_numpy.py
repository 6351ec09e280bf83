"""Oracle of the stereo rectification: the remap of 8-bit pictures through OpenCV's fixed-point map
pair, and the maker of that pair. numpy only; tests/test_rectify_cpu.py pins it against closed forms, and the C map
maker (csrc/svx_rectify_host.h) and the kernel (csrc/kernels/remap.hip) are compared with it entry for entry.

The map format is cv2.initUndistortRectifyMap(..., m1type=CV_16SC2)'s: xy int16 (dh, dw, 2) holding (sx, sy), frac
uint16 (dh, dw) holding fy * 32 + fx with 0 <= fx, fy < 32 (INTER_BITS = 5).

remap() restates cv2.remap(src, xy, frac, INTER_LINEAR, borderMode=BORDER_CONSTANT, borderValue=0) for 8-bit
pictures: OpenCV's 2-D bilinear table at 5 fractional bits holds, for every (fx, fy), the four float products
(1 - fx/32)(1 - fy/32) ... scaled by INTER_REMAP_COEF_SCALE = 32768 and rounded to int16; each product is a multiple of
1/1024, so the scaled values 32 (32 - fx)(32 - fy), ... are whole numbers, they sum to 32768 exactly and the table's
sum correction (which moves a rounding residue into the largest weight) never fires. The pixel is
(w00 S00 + w10 S10 + w01 S01 + w11 S11 + 16384) >> 15 in int32, a tap outside the source counting as 0. cv2 is absent
here, so parity with cv2.remap itself is unpinned: this formula is what the device is held to.

rectify_map() restates initUndistortRectifyMap in float64 with every operation written once, in the order the C code
mirrors (both without fused multiply-adds), so the two agree bit for bit; the inverse of P R is the adjugate over the
determinant, and parity with OpenCV's LU inverse to the last ulp is unpinned.
"""
import numpy as np

MAX_DIM = 8192                       # source and destination dimensions: 1 .. 8192
IU_MIN, IU_MAX = -32768 * 32, 32767 * 32 + 31


def weights(fx, fy):
    """The four int32 weights (w00, w10, w01, w11) of (fx, fy): they sum to 32768."""
    fx, fy = np.asarray(fx, np.int32), np.asarray(fy, np.int32)
    return 32 * (32 - fx) * (32 - fy), 32 * fx * (32 - fy), 32 * (32 - fx) * fy, 32 * fx * fy


def check_maps(xy, frac):
    xy, frac = np.asarray(xy), np.asarray(frac)
    if xy.dtype != np.int16 or xy.ndim != 3 or xy.shape[2] != 2:
        raise ValueError(f"xy must be int16 (dh, dw, 2), got {xy.dtype} {xy.shape}")
    if frac.dtype != np.uint16 or frac.shape != xy.shape[:2]:
        raise ValueError(f"frac must be uint16 {xy.shape[:2]}, got {frac.dtype} {frac.shape}")
    if not (1 <= xy.shape[0] <= MAX_DIM and 1 <= xy.shape[1] <= MAX_DIM):
        raise ValueError("destination dimensions in 1 .. 8192")
    if frac.size and int(frac.max()) >= 1024:
        raise ValueError("frac entries are fy * 32 + fx < 1024")
    return xy, frac


def remap(src, xy, frac):
    """src: uint8 (sh, sw) or (sh, sw, 3); returns uint8 of the map's shape (and the source's channels)."""
    src = np.asarray(src)
    if src.dtype != np.uint8 or src.ndim not in (2, 3) or (src.ndim == 3 and src.shape[2] != 3):
        raise ValueError(f"src must be uint8 (sh, sw) or (sh, sw, 3), got {src.dtype} {src.shape}")
    xy, frac = check_maps(xy, frac)
    sh, sw = src.shape[:2]
    if not (1 <= sh <= MAX_DIM and 1 <= sw <= MAX_DIM):
        raise ValueError("source dimensions in 1 .. 8192")
    sx, sy = xy[..., 0].astype(np.int32), xy[..., 1].astype(np.int32)
    fx, fy = (frac & 31).astype(np.int32), (frac >> 5).astype(np.int32)
    s3 = src.reshape(sh, sw, -1).astype(np.int32)
    acc = np.zeros(xy.shape[:2] + (s3.shape[2],), np.int32)
    for (i, j), w in zip(((0, 0), (1, 0), (0, 1), (1, 1)), weights(fx, fy)):
        x, y = sx + i, sy + j
        inside = (x >= 0) & (x < sw) & (y >= 0) & (y < sh)
        tap = np.where(inside[..., None], s3[np.clip(y, 0, sh - 1), np.clip(x, 0, sw - 1)], 0)
        acc += w[..., None] * tap
    out = ((acc + 16384) >> 15).astype(np.uint8)
    return out[..., 0] if src.ndim == 2 else out


def taps_inside(xy, sh, sw):
    """How many of an entry's four taps lie inside an sh x sw source: (dh, dw) of 0 .. 4."""
    sx, sy = xy[..., 0].astype(np.int32), xy[..., 1].astype(np.int32)
    n = np.zeros(sx.shape, np.int32)
    for i, j in ((0, 0), (1, 0), (0, 1), (1, 1)):
        n += ((sx + i >= 0) & (sx + i < sw) & (sy + j >= 0) & (sy + j < sh))
    return n


def inverse_3x3(M):
    """The adjugate over the determinant, every product and difference written once (the C code's order). None for a
    zero or non-finite determinant."""
    M = np.asarray(M, np.float64).reshape(3, 3)
    (a, b, c), (d, e, f), (g, h, i) = ((np.float64(v) for v in row) for row in M)
    with np.errstate(all="ignore"):
        A00, A01, A02 = e * i - f * h, c * h - b * i, b * f - c * e
        A10, A11, A12 = f * g - d * i, a * i - c * g, c * d - a * f
        A20, A21, A22 = d * h - e * g, b * g - a * h, a * e - b * d
        det = (a * A00 + b * A10) + c * A20
        if not np.isfinite(det) or det == 0.0:
            return None
        return np.array([[A00 / det, A01 / det, A02 / det], [A10 / det, A11 / det, A12 / det],
                         [A20 / det, A21 / det, A22 / det]], np.float64)


def product_3x3(P, R):
    """P R with each entry (p0 r0 + p1 r1) + p2 r2."""
    P, R = np.asarray(P, np.float64).reshape(3, 3), np.asarray(R, np.float64).reshape(3, 3)
    M = np.empty((3, 3), np.float64)
    with np.errstate(all="ignore"):
        for i in range(3):
            for j in range(3):
                M[i, j] = (P[i, 0] * R[0, j] + P[i, 1] * R[1, j]) + P[i, 2] * R[2, j]
    return M


def rectify_map(K, D, R, P, shape):
    """(xy, frac) of `shape` = (dh, dw) for the raw camera K (3 x 3: fx, fy, u0, v0 are read), its distortion D
    (k1, k2, p1, p2, k3, k4, k5, k6), the rectifying rotation R and the new camera matrix P (3 x 3). ValueError for a
    singular or non-finite P R or a shape outside 1 .. 8192."""
    K = np.asarray(K, np.float64).reshape(3, 3)
    D = np.asarray(D, np.float64).reshape(-1)
    if D.size != 8:
        raise ValueError("D holds the 8 coefficients k1, k2, p1, p2, k3, k4, k5, k6")
    dh, dw = (int(v) for v in shape)
    if not (1 <= dh <= MAX_DIM and 1 <= dw <= MAX_DIM):
        raise ValueError("destination dimensions in 1 .. 8192")
    inv = inverse_3x3(product_3x3(P, R))
    if inv is None:
        raise ValueError("P R is singular or not finite")
    fxk, fyk, u0, v0 = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    k1, k2, p1, p2, k3, k4, k5, k6 = (np.float64(v) for v in D)
    u = np.arange(dw, dtype=np.float64)[None, :]
    v = np.arange(dh, dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        X = (inv[0, 0] * u + inv[0, 1] * v) + inv[0, 2]
        Y = (inv[1, 0] * u + inv[1, 1] * v) + inv[1, 2]
        W = (inv[2, 0] * u + inv[2, 1] * v) + inv[2, 2]
        x, y = X / W, Y / W
        r2 = x * x + y * y
        kr = (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1.0 + ((k6 * r2 + k5) * r2 + k4) * r2)
        xy2 = 2.0 * x * y
        xd = (x * kr + p1 * xy2) + p2 * (r2 + 2.0 * x * x)
        yd = (y * kr + p1 * (r2 + 2.0 * y * y)) + p2 * xy2
        mu = fxk * xd + u0
        mv = fyk * yd + v0
        iu, iv = np.rint(32.0 * mu), np.rint(32.0 * mv)      # half to even
    out = []
    for t in (iu, iv):
        t = np.where(np.isfinite(t), np.clip(t, IU_MIN, IU_MAX), IU_MIN)
        out.append(np.broadcast_to(t, (dh, dw)).astype(np.int64))
    iu, iv = out
    xy = np.stack([iu >> 5, iv >> 5], -1).astype(np.int16)
    frac = ((iv & 31) * 32 + (iu & 31)).astype(np.uint16)
    return xy, frac


def camera_from_projection(P_left, P_right):
    """(f, B, cw, ch) of the rectified pair: f = P[0][0], B = -P_right[0][3] / f, cw = P[0][2], ch = P[1][2]; P_left
    3 x 3 or 3 x 4, P_right 3 x 4 (stereoRectify's P1, P2)."""
    P1, P2 = np.asarray(P_left, np.float64), np.asarray(P_right, np.float64)
    f = P1[0, 0]
    return (float(f), float(-P2[0, 3] / f), float(P1[0, 2]), float(P1[1, 2]))


# ---- the models the tests share ----------------------------------------------------------------------------------
def rot(axis, deg):
    c, s = np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))
    return {"x": np.array([[1, 0, 0], [0, c, -s], [0, s, c]], np.float64),
            "y": np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], np.float64),
            "z": np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], np.float64)}[axis]


def camera_matrix(f, u0, v0, fy=None):
    return np.array([[f, 0, u0], [0, f if fy is None else fy, v0], [0, 0, 1]], np.float64)


def models(shape):
    """name -> (K, D, R, P) for a destination of `shape`: the camera sits in its middle."""
    dh, dw = shape
    f = 0.8 * max(dw, 2)
    K = camera_matrix(f, (dw - 1) / 2.0, (dh - 1) / 2.0, 0.97 * f)
    Z, I = np.zeros(8), np.eye(3)
    barrel = np.array([-0.3, 0, 0, 0, 0, 0, 0, 0], np.float64)
    full = np.array([-0.28, 0.09, 0.0013, -0.0021, -0.012, 0.02, -0.006, 0.0011], np.float64)
    out = {"identity": (K, Z, I, K), "barrel": (K, barrel, I, K), "rational": (K, full, I, K),
           "rot_x": (K, barrel, rot("x", 2.0), K), "rot_y": (K, barrel, rot("y", 2.0), K),
           "rot_z": (K, barrel, rot("z", 2.0), K),
           # the new camera sees twice as wide, and the view is turned: the corners leave the source
           "corners": (K, barrel, rot("z", 5.0), camera_matrix(0.45 * f, (dw - 1) / 2.0 + 3.3, (dh - 1) / 2.0 - 2.1)),
           # the probe's: barrel plus 1 degree about y
           "barrel_rot1": (K, barrel, rot("y", 1.0), K)}
    return out
