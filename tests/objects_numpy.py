"""The obstacle list in plain numpy / Python, as the oracle of kernels/objects.hip. Slow and literal on purpose:
include/svx.h (sv_obstacle_list) states the semantics, tests/test_objects_cpu.py pins this file (its partition
against scipy.ndimage.label, closed forms).

  label(img)                          (labels int32, k): 8-connected components of img != 0 by flood fill from every
                                      set pixel in raster order, so label i + 1 is the i-th component by first pixel
  components(img, disp=None)          one dict per component, in that order
  lower_median(values)                sorted(values)[(len - 1) // 2]
  obstacle_list(img, disp, min_area, cap)   (n, entries): what dropin.obstacle_list / Batch.read_obstacle_list return
  obstacle_xyz(entry, camera)         (X, Y, Z) of an entry, functions.py:191-193 at the box's centre, or None
  cases(H, W)                         the named test images
"""
import numpy as np

FIELDS = ("x0", "y0", "x1", "y1", "area", "first", "nd", "dmax", "dmed", "reserved", "sx", "sy")


def label(img):
    a = np.asarray(img) != 0
    H, W = a.shape
    lab = np.zeros((H, W), np.int32)
    k = 0
    for p in np.flatnonzero(a):          # raster order
        y, x = divmod(int(p), W)
        if lab[y, x]:
            continue
        k += 1
        lab[y, x] = k
        stack = [(y, x)]
        while stack:
            cy, cx = stack.pop()
            for ny in (cy - 1, cy, cy + 1):
                for nx in (cx - 1, cx, cx + 1):
                    if 0 <= ny < H and 0 <= nx < W and a[ny, nx] and not lab[ny, nx]:   # outside: background
                        lab[ny, nx] = k
                        stack.append((ny, nx))
    return lab, k


def lower_median(values):
    v = sorted(int(x) for x in values)
    return v[(len(v) - 1) // 2]


def components(img, disp=None):
    lab, k = label(img)
    W = lab.shape[1]
    out = []
    for i in range(1, k + 1):
        ys, xs = np.nonzero(lab == i)    # raster order
        c = {"x0": int(xs.min()), "y0": int(ys.min()), "x1": int(xs.max()), "y1": int(ys.max()),
             "area": int(len(xs)), "first": int(ys[0]) * W + int(xs[0]), "nd": 0, "dmax": 0, "dmed": 0,
             "reserved": 0, "sx": int(xs.astype(np.int64).sum()), "sy": int(ys.astype(np.int64).sum())}
        if disp is not None:
            d = np.asarray(disp)[ys, xs]
            d = d[d > 0]
            if len(d):
                c["nd"], c["dmax"], c["dmed"] = int(len(d)), int(d.max()), lower_median(d)
        out.append(c)
    return out


def obstacle_list(img, disp=None, min_area=70, cap=16):
    keep = [c for c in components(img, disp) if c["area"] >= min_area]
    keep.sort(key=lambda c: (-c["area"], c["first"]))
    return len(keep), keep[:cap]


def as_dicts(entries):
    """A structured array of entries (or a list of dicts) as a list of dicts of Python ints."""
    return [{k: int(e[k]) for k in FIELDS} for e in entries]


def obstacle_xyz(entry, camera):
    f, B, cw, ch = (float(v) for v in camera)
    if int(entry["dmed"]) == 0:
        return None
    z = (f * B) / int(entry["dmed"])
    cx = (int(entry["x0"]) + int(entry["x1"])) / 2.0
    cy = (int(entry["y0"]) + int(entry["y1"])) / 2.0
    return ((cx - cw) * z) / f, ((cy - ch) * z) / f, z


def _ring(a, y0, x0, y1, x1):
    a[y0, x0:x1 + 1] = 1
    a[y1, x0:x1 + 1] = 1
    a[y0:y1 + 1, x0] = 1
    a[y0:y1 + 1, x1] = 1


def cases(H, W):
    """The named images (uint8, 0 / 255) at H x W; a pattern that needs more room than the shape has is left out."""
    yy, xx = np.mgrid[0:H, 0:W]
    c = {}
    c["empty"] = np.zeros((H, W), bool)
    c["full"] = np.ones((H, W), bool)
    c["checkerboard"] = (yy + xx) % 2 == 0
    # lines through the frame, wrapping down the rows so that they cross x = 31 | 32 and 63 | 64 at any height
    c["diagonal"] = (xx % H) == yy if H > 1 else xx == 0
    c["anti_diagonal"] = ((W - 1 - xx) % H) == yy if H > 1 else xx == W - 1
    c["stripes"] = np.broadcast_to(xx % 2 == 0, (H, W))
    comb = xx % 2 == 0
    c["comb"] = comb | (yy == H - 1)          # the teeth join only in the last row
    c["comb_mirror"] = comb | (yy == 0)       # ... or only in the first
    # one one-pixel-wide path over the whole image: every other row full, joined at alternating ends
    s = yy % 2 == 0
    odd = yy % 2 == 1
    s = s | (odd & (yy % 4 == 1) & (xx == W - 1)) | (odd & (yy % 4 == 3) & (xx == 0))
    c["serpentine"] = s
    if H >= 9 and W >= 9:
        r = np.zeros((H, W), bool)
        _ring(r, 0, 0, H - 1, W - 1)
        _ring(r, 2, 2, H - 3, W - 3)           # a pixel of background between them: two components
        c["rings"] = r
    e = np.zeros((H, W), bool)                 # components on the four edges and corners
    e[0, 0] = e[0, W - 1] = e[H - 1, 0] = e[H - 1, W - 1] = True
    if H >= 5 and W >= 8:
        e[0, W // 2 - 1:W // 2 + 1] = True
        e[H - 1, W // 2 - 1:W // 2 + 2] = True
        e[H // 2 - 1:H // 2 + 1, 0] = True
        e[H // 2 - 1:H // 2 + 2, W - 1] = True
    c["edges"] = e
    return {k: v.astype(np.uint8) * 255 for k, v in c.items()}


def holed_frame(H, W):
    """A disparity that is road everywhere but in three rectangular holes (200 / 0): two of 30 x 40, one of 34 x 48,
    each large enough to survive sanitiseRoadImage's 9 x 9 close, and far enough apart to stay three obstacles after
    its 17 x 17 erode."""
    d = np.full((H, W), 200, np.uint8)
    y = H // 2 - 15
    for x, h, w in ((W // 8, 30, 40), (W // 2 - 20, 30, 40), (W - W // 8 - 48, 34, 48)):
        d[y:y + h, x:x + w] = 0
    return d


def two_blob_frame(H, W):
    """Two road blobs in opposite corners (the two-blob frame of tests/test_gpu_hull.py): the hull between them is
    all obstacle."""
    d = np.zeros((H, W), np.uint8)
    d[2:2 + H // 3, 5:5 + W // 4] = 200
    d[H - 4 - H // 3:H - 4, W - 9 - W // 3:W - 9] = 200
    return d


def batch_frames(H, W):
    """The batch tests' disparities: the holed road, an empty frame, the holed road again, two blobs. With a plane
    that keeps every pixel with d > 0 the road image is d > 0."""
    return [holed_frame(H, W), np.zeros((H, W), np.uint8), holed_frame(H, W), two_blob_frame(H, W)]


def limit_rectangles():
    """40 x 70 with rectangles of areas 12, 12, 11, 6, 6, 6, 2 and 1, none touching another."""
    a = np.zeros((40, 70), np.uint8)
    for y, x, h, w in ((1, 40, 3, 4), (1, 2, 2, 6), (6, 30, 1, 11), (10, 60, 2, 3), (10, 5, 3, 2), (20, 33, 6, 1),
                       (30, 62, 1, 2), (38, 31, 1, 1)):
        a[y:y + h, x:x + w] = 255
    return a
