/*
 * svx — MI355X-native disparity -> 3D point-cloud hot path (C ABI).
 *
 * Drop-in boundary for thien/stereo.vision. The reference has no native/FFI
 * API: its boundary is the Python module `functions`, whose attributes
 * stereovision.py resolves at call time (stereovision.py:3, :84-113). The
 * Python binding (stereo.vision_amd/svx/_abi.py, ctypes) binds exactly these
 * symbols and re-exposes the reference's signatures (svx/dropin.py).
 *
 * Conventions
 *   - every entry point returns 0 on success, a negative SV_E* code on error;
 *     sv_last_error() gives a thread-local message. The Python wrapper raises
 *     RuntimeError(message), which lands in the reference's own try/except
 *     (stereovision.py:92-126) exactly like a reference exception would.
 *   - host buffers are allocated by the caller; device buffers are owned by
 *     the library (sv_batch) and stay resident in HBM.
 *   - the "host" entry points (sv_project_frame, sv_backproject,
 *     sv_pipeline_frame) are synchronous: they return after the D2H copy.
 *   - plain pointers and sizes only; no torch / no C++ types.
 */
#ifndef SVX_H
#define SVX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SV_OK 0
#define SV_E_ARG -1     /* bad argument / unsupported shape                */
#define SV_E_HIP -2     /* HIP runtime error                               */
#define SV_E_CAP -3     /* caller's output capacity too small              */
#define SV_E_STATE -4   /* not initialised / wrong object                  */
#define SV_E_COMM -5    /* RCCL error                                      */
#define SV_E_DEVICE -6  /* a kernel reported an internal failure (timeout) */
#define SV_E_RANGE -7   /* input outside the supported value range          */

/* functions.py:15,19,21,22 — focal length (px), baseline (m), image centre. */
typedef struct { double f, B, cw, ch; } sv_camera;
/* Plane a*X + b*Y + c*Z = 1 (functions.py:267, consumed at :300-312). */
typedef struct { double a, b, c; } sv_plane;

/* ---- library / device ------------------------------------------------- */
const char* sv_version(void);
const char* sv_last_error(void);
int sv_device_count(int* n);
int sv_init(int device);                 /* select + warm the device          */

/* ---- drop-in (host buffers, synchronous) -------------------------------- */

/* Replaces functions.py:178-198 projectDisparityTo3d(disparity, max_disparity,
 * rgb=[]). Grid y in range(0,H-1,step) x range(0,W-1,step), raster order,
 * d == 0 skipped, fp64 X,Y,Z bit-identical to the reference arithmetic.
 * bgr may be NULL (the `rgb=[]` case, stereovision.py:85); out_rgb receives
 * (R,G,B) = bgr[...,2], bgr[...,1], bgr[...,0] (functions.py:195).
 * cap = rows available in out_xyz/out_rgb; *out_n = rows written. */
int sv_project_frame(const uint8_t* disp, int H, int W, int64_t ld_disp,
                     const uint8_t* bgr, int64_t ld_bgr, int step, const sv_camera* cam,
                     double* out_xyz, uint8_t* out_rgb, int64_t cap, int64_t* out_n);

/* projectDisparityTo3d's rows as the drop-in returns them (functions.py:178-198, the same points and bits as
 * sv_project_frame): out_rows holds cap rows of `cols` doubles — X, Y, Z (cols 3; bgr may be NULL) or X, Y, Z, R,
 * G, B (cols 6, bgr required) — laid out on the device and copied back in one transfer, a direct DMA when out_rows
 * is page-locked (sv_host_alloc). *out_n = rows written. */
int sv_project_rows(const uint8_t* disp, int H, int W, int64_t ld_disp, const uint8_t* bgr, int64_t ld_bgr,
                    int step, const sv_camera* cam, double* out_rows, int cols, int64_t cap, int64_t* out_n);

/* Page-locked host memory for drop-in outputs (hipHostMalloc / hipHostFree): the Python binding pools these blocks
 * and hands them out as numpy arrays that return to the pool when the last view is gone (svx/_abi.py). */
int sv_host_alloc(int64_t bytes, void** out);
int sv_host_free(void* p);

/* Replaces functions.py:201-209 project3DPointsTo2DImagePoints(points):
 * x = ((X*f)/Z)+cw, y = ((Y*f)/Z)+ch in fp64, bit-identical. xyz rows have
 * stride ld (>= 3) doubles; out_xy is n x 2. */
int sv_backproject(const double* xyz, int64_t n, int64_t ld, const sv_camera* cam, double* out_xy);

/* Fused chain of stereovision.py:84,97-113 for one host frame: projection ->
 * calculatePointErrors (functions.py:300-312) -> computePlanarThreshold
 * (:314-323) -> calculateColourHistogram (:215-226) -> filterPointsByHistogram
 * (:228-230) -> back-projection + int32 trunc (stereovision.py:111-113).
 * out_counts[3] = N_valid, N_kept, N_kept2; out_hist[1024] = hue-bin counts of
 * the plane-kept points (bin k <-> key str(k/1000)); out_xyz (cap x 3, fp32,
 * NULL ok) and out_pts (cap x 2 int32) hold the N_kept2 surviving points in
 * reference order. Any W >= 2 (rows are staged at a stride rounded up to 8). */
int sv_pipeline_frame(const uint8_t* disp, const uint8_t* bgr, int H, int W, int step,
                      const sv_camera* cam, const sv_plane* plane, double point_thr, int hist_thr,
                      int64_t* out_counts, uint32_t* out_hist, float* out_xyz, int32_t* out_pts,
                      int64_t cap);

/* ---- disparity pre-pass, host frames, synchronous ---- */

/* Replaces functions.py:141-148 fillDisparity(disparity, previousDisparity):
 * out = d > 2 ? d : min(255, d + prev) per pixel (cv2.threshold BINARY at 2,
 * bitwise_not, masked copy of prev, saturating cv2.add); prev NULL -> copy. */
int sv_fill_previous(const uint8_t* disp, const uint8_t* prev, int H, int W, uint8_t* out);
/* Replaces functions.py:150-162 fillAltDisparity(disparity), IN PLACE like the
 * reference: pixels < 2 of each row <- trunc(mean of the row's non-zero values). */
int sv_fill_mean(uint8_t* disp, int H, int W);
/* Replaces functions.py:169-172 maskDisparity(disparity) with the caller's
 * carmask (functions.py:35): out = mask != 0 ? d : 0. */
int sv_mask_disparity(const uint8_t* disp, const uint8_t* mask, int H, int W, uint8_t* out);

/* ---- road raster + non-zero walk, host, synchronous -- */

/* Replaces functions.py:339-344 generatePointsAsImage(points): an H x W grey
 * image, 0 except 255 at every [x, y] of pts (n x 2 int32, the planePoints of
 * stereovision.py:112-113). Negative indices wrap like numpy's; a point past
 * [-W, W) x [-H, H) fails with SV_E_ARG (numpy raises IndexError). */
int sv_road_raster(const int32_t* pts, int64_t n, int H, int W, uint8_t* out_img);
/* The pixel walk at the end of functions.py:355-366 (sanitiseRoadImage):
 * out = [j, i] (int32) of every non-zero pixel, raster order. W <= 4096. */
int sv_nonzero_points(const uint8_t* img, int H, int W, int32_t* out, int64_t cap, int64_t* out_n);
/* Replaces functions.py:346-366 sanitiseRoadImage(img, size): the road image's clean-up and its pixel walk.
 * img: H x W u8, non-zero pixels are "set"; mask: H x W u8 (road_threshold_mask, functions.py:31), NULL = all
 * ones. out_img (nullable): H x W u8 holding only 0 or 255. The steps, exactly:
 *   1. close by a 9 x 9 rectangle (cv2.morphologyEx MORPH_CLOSE, :351): dilate with radius 4, then erode with
 *      radius 4, anchor at the centre, OpenCV's default morphology borders — for the dilation pixels outside
 *      the image count as clear, for the erosion they count as set, so the border never clears a pixel;
 *   2. erode by 9 x 9 twice (:353), which with that border is one erosion by 17 x 17 (radius 8);
 *   3. AND with mask != 0 (cv2.bitwise_and(img, img, mask=m), :355: a mask pixel of 128 keeps the pixel);
 *   4. close by 9 x 9 again (:356);
 *   5. ParticleCleansing (:358, :378-384) is the identity on step 4's result (it fills external contours of
 *      area < 70; a hole that survives a 9 x 9 close holds a full 9 x 9 block of zeros, so its contour's area
 *      is above 81: DESIGN.md) and has no kernel;
 *   6. the walk (:359-365): out_pts (nullable, cap x 2 int32) = [j, i] of every non-zero pixel in raster order,
 *      *out_n (nullable) their number; SV_E_CAP when out_pts holds fewer (as sv_nonzero_points).
 * All four operations are rectangular, done separably on a bitmap (rows, then columns); the chain's vertical
 * reach is 4 + 4 + 8 + 4 + 4 = 24 rows. The steps restate cv2 calls (cv2 is absent here): their parity with the
 * reference's OpenCV is unpinned, like fillDisparity / maskDisparity. 2 <= W <= 4096, H * W < 2^28. Host,
 * synchronous. */
int sv_sanitise_road(const uint8_t* img, const uint8_t* mask, int H, int W, uint8_t* out_img, int32_t* out_pts,
                     int64_t cap, int64_t* out_n);

/* ---- the obstacle stage (stereovision.py:170-189, functions.py:396-421) ---- */

/* What the reference derives from the cleaned road image: cv2.convexHull(resultingPoints), the hull filled as a
 * mask, obstacles = hull & ~road, getCenterPoint(hull) and getNormalVectorLine(centre, abc, disparity). The
 * device works on the cleaned image as a bitmap (H rows of ceil(W / 32) words, pixel x at bit x & 31 of word
 * x >> 5, pad bits zero, as csrc/svx_morph.h); the entry points below take and return u8 images.
 *  - hull: the STRICT vertices of the convex hull of all set pixels (x, y) (no vertex collinear with its
 *    neighbours), int32 (x, y) pairs, at most 2 H of them. Order: from the vertex with the smallest (y, then x)
 *    down the left side with y increasing, then back up the right side; on each side the vertices have distinct
 *    y apart from the top and bottom rows. No set pixel: n = 0; one pixel: n = 1; all pixels collinear: n = 2,
 *    the two ends.
 *  - hull mask: pixel (x, y) is set exactly when it lies in the closed hull, decided by exact integer
 *    half-plane tests; per row that is every integer x with ceil(xl(y)) <= x <= floor(xr(y)), xl and xr the
 *    rational crossings of the left and right chains (integer floor division, right for negative numerators).
 *    For n <= 2 the mask is the lattice points of the point or segment.
 *  - obstacles: hull mask & ~cleaned (stereovision.py:174-180, before the colouring).
 *  - centre (cx, cy): the centre of the EXACT minimum enclosing circle of the hull's vertices, truncated toward
 *    zero; n = 1: the point, n = 2: the midpoint truncated. The centre is a rational p / q with |q| < 2^26,
 *    computed in 64-bit integers with 128-bit containment tests; bit 0 of `valid` is clear when n = 0, and
 *    also, with n > 0 and the hull in place, should the circle's iteration reach its bound of 4 n + 64 exchanges
 *    (it does not in exact arithmetic; the bound keeps a fault from spinning): then there is no centre and no tip.
 *  - tip (tipx, tipy): getNormalVectorLine((cx, cy), abc, disparity) in fp64, the reference's operation order,
 *    no contraction, truncated as int64. Bit 1 of `valid` is clear when there is no centre, no disparity or no
 *    plane, when disparity[cy, cx] == 0, or when a result is not finite or does not fit an int64 (where the
 *    reference raises inside its try).
 * Parity with OpenCV (cv2 is absent here, as for sv_sanitise_road): cv2.convexHull's start vertex and
 * orientation are unpinned (its consumers do not depend on them); cv2.drawContours(.., -100) also lights the
 * Bresenham pixels of the hull's edges, which can lie outside the closed polygon by less than a pixel (in the
 * reference they sit under the 5-pixel hull line drawRoadLine draws next); cv2.minEnclosingCircle is a float32
 * approximation that depends on the version. getNormalVectorLine is pure Python and pinned by fixtures. */
typedef struct {
    int32_t n, cx, cy, valid;
    int64_t tipx, tipy;
} sv_hull_info;
/* One host frame. cleaned: H x W u8, non-zero = road; disp (nullable): H x W u8; plane (nullable): abc; without
 * disp or plane bit 1 of info->valid is clear. hull_pts: cap x 2 int32, SV_E_CAP (info->n set) when cap <
 * info->n. hull_mask, obstacles (nullable): H x W u8 of 0 / 255. 2 <= W <= 4096, 1 <= H <= 4096. Synchronous. */
int sv_road_obstacles(const uint8_t* cleaned, const uint8_t* disp, const sv_plane* plane, int H, int W,
                      const sv_camera* cam, int32_t* hull_pts, int64_t cap, uint8_t* hull_mask, uint8_t* obstacles,
                      sv_hull_info* info);
/* The centre alone (functions.py:418-421 getCenterPoint with the exact circle): pts = n x 2 int32 (any points,
 * |x|, |y| <= 16383, 1 <= n <= 8192: the circle is computed by one lane, so pass a hull, not a cloud),
 * out_xy[2] = the centre truncated toward zero. */
int sv_min_circle_centre(const int32_t* pts, int64_t n, int32_t* out_xy);

/* ---- the obstacle list: the components of the obstacle image, with box and range ---- */

/* What the obstacle image holds, as a list (the reference stops at the picture; its brief asks for "detecting
 * objects on the road"). Everything is an integer and exact.
 *  - components: the 8-connected components of the non-zero pixels (cv2.connectedComponentsWithStats' default
 *    connectivity; scipy.ndimage.label with a 3 x 3 structure of ones); pixels outside the image are background.
 *  - per component: area = its pixels; x0, y0, x1, y1 = its inclusive box; first = y * W + x of its first pixel in
 *    raster order; sx, sy = the sums of its pixels' x and of their y (the centroid is sx / area, sy / area, divided
 *    by the caller).
 *  - disparity, over the component's pixels with d > 0 (any u8 value counts): nd = their number, dmax = the
 *    largest (the nearest point), dmed = the lower median, sorted(values)[(nd - 1) / 2]. All three are 0 when
 *    nd == 0 or no disparity is given.
 *  - the list: n = the number of components with area >= min_area, in full even when it exceeds cap; the list holds
 *    the first min(n, cap) of them ordered by area descending, then by first ascending. Entries past the list's
 *    length are not written. reserved is written as 0.
 * No floating point on the device: metres are the caller's, Z = f B / dmed and X, Y those of the box's centre at
 * that Z (functions.py:191-193; svx.dropin.obstacle_xyz). cv2's label numbering is not reproduced (cv2 is absent
 * here; the list has the order above). The device labels runs of set bits of the packed bitmap by union-find
 * (csrc/kernels/objects.hip). */
typedef struct sv_obstacle {
    int32_t x0, y0, x1, y1, area, first, nd, dmax, dmed, reserved;
    int64_t sx, sy;
} sv_obstacle;   /* 56 bytes */
/* One host frame, synchronous. obstacles: H x W u8, non-zero = obstacle; disp (nullable): H x W u8; out: cap
 * entries; *n as above. 2 <= W <= 4096, 1 <= H <= 4096, min_area >= 1, 1 <= cap <= 32; SV_E_ARG otherwise and for
 * null obstacles, out or n, before anything is launched. */
int sv_obstacle_list(const uint8_t* obstacles, const uint8_t* disp /* nullable */, int H, int W, int min_area,
                     sv_obstacle* out, int cap, int32_t* n);

/* ---- the ground grid: top-down occupancy of obstacles and road ---- */

/* The obstacle image and the cleaned road image laid out on the ground plane (the reference stops at the picture;
 * a planner, a logger or a display asks, for each lateral position, what is occupied and how near). A grid is nz
 * rows of nx square cells of `cell` metres: cell (iz, ix) covers X in [x0 + ix cell, x0 + (ix + 1) cell) and Z in
 * [z0 + iz cell, z0 + (iz + 1) cell); row 0 is the nearest. cell finite and > 0, x0 and z0 finite, nx, nz >= 1,
 * nx * nz <= 8192 (two uint32 planes of the cells live in 64 KB of LDS). The default (a null grid) is 16 m across
 * and 32 m ahead in cells of 0.25 m: x0 = -8, z0 = 0, cell = 0.25, nx = 64, nz = 128.
 *  - a pixel (y, x) with d = disp[y, x] > 0 lies, in float64 and in the order of functions.py:191-192, at
 *    Z = (f * B) / d, X = ((x - cw) * Z) / f; iz = floor((Z - z0) / cell), ix = floor((X - x0) / cell); it is in the
 *    grid iff 0 <= ix < nx and 0 <= iz < nz, compared as doubles (floor, not truncation: a negative quotient is
 *    outside, not cell 0). x and y are indices of the frame as given (a cropped frame: the crop's own).
 *  - obst[iz * nx + ix]: the obstacle image's non-zero pixels with d > 0 in the cell; road[..]: the same count for
 *    the road image. Full 32-bit counts.
 *  - nearest[ix]: the smallest iz with obst[iz * nx + ix] >= min_count (min_count >= 1), else -1.
 *  - info[4]: obstacle pixels in the grid; obstacle pixels with d > 0 outside it; obstacle pixels with d == 0; road
 *    pixels in the grid. So sum(obst) == info[0], info[0] + info[1] + info[2] == the obstacle image's non-zero
 *    pixels, sum(road) == info[3].
 * The device does no floating point: the host builds the mapping (d, x) -> ix and d -> iz once per (camera, grid,
 * W) in float64 (csrc/svx_ground_host.h), cached per device, and the kernel (csrc/kernels/ground.hip) looks it up.
 * Metres are the caller's (svx.dropin.ground_grid_axes gives the cells' centres). */
typedef struct sv_grid {
    double x0, z0, cell;
    int32_t nx, nz;
} sv_grid;   /* 32 bytes */
/* One host frame, synchronous. obstacles: H x W u8, non-zero = obstacle; road (nullable): H x W u8, non-zero = road;
 * disp: H x W u8; grid (nullable: the default). Outputs: obst, road_out (nullable): nz x nx uint32; nearest: nx int32;
 * info: 4 int32. 2 <= W <= 4096, 1 <= H <= 4096; SV_E_ARG otherwise, for a null obstacles, disp, cam, obst, nearest or
 * info, a grid out of range, min_count < 1 or a camera whose f or B is not finite and positive, before anything is
 * launched. */
int sv_ground_grid(const uint8_t* obstacles, const uint8_t* road /* nullable */, const uint8_t* disp, int H, int W,
                   const sv_camera* cam, const sv_grid* grid /* nullable */, int min_count, uint32_t* obst,
                   uint32_t* road_out /* nullable */, int32_t* nearest, int32_t* info);

/* ---- the result image (stereovision.py:181-209, functions.py:390-394, :424-431) ---- */

/* The picture performStereoVision shows per frame: the left image dimmed with its obstacles tinted yellow
 * (cv2.addWeighted), the road hull outlined in red (drawRoadLine) and the road-normal glyph drawn from the hull's
 * centre (drawNormalLine). Inputs: the BGR, the obstacle image, the hull's n vertices in outline order and the
 * sv_hull_info of the obstacle stage (centre, tip, valid). Output: H x W x 3 u8, (B, G, R) per pixel.
 * Every predicate is exact integer arithmetic on pixel coordinates p = (x, y); D(p; a, b) is the squared Euclidean
 * distance from p to the closed segment ab (a point when a = b). Later layers overwrite earlier ones:
 *  0. n = 0 (the reference's cv2.convexHull raises inside both try blocks): the BGR unchanged.
 *  1. overlay, n >= 1: every channel value i becomes rint(0.6 i) = floor((6 i + 5) / 10); on obstacle pixels G and
 *     R get 102 more. This is cv2.addWeighted(obst, 0.4, img, 0.6, 0) with obst in {0, 255}: 3 i / 5 is never a
 *     tie, the fp32 error is about 1e-5 and the maximum is 255, so every evaluation order gives the same byte.
 *  2. hull outline, n >= 1, whatever `valid` says: (0, 0, 255) where 4 D(p; v_k, v_k+1) <= 25 for some edge of the
 *     closed polygon v_0 .. v_n-1 -> v_0 in the stored order; n = 1: the 21 pixels with dx^2 + dy^2 <= 6; n = 2:
 *     the one segment.
 *  3. glyph line, when bit 1 of `valid` is set and |tipx|, |tipy| <= 2^31 - 1 (cv2 takes no larger point, and the
 *     reference's try swallows the error): (204, 185, 22) where D(p; centre, tip) <= 1.
 *  4. glyph head, under the same condition: (214, 195, 32) where |p - tip|^2 <= 49 (cv2.circle with radius 2 and
 *     thickness 10 covers radii 0-7).
 * Strokes are clipped to the image; a tip far outside still draws the visible part of its line.
 * Parity with OpenCV: layer 1 is pinned (tests/test_result_cpu.py: all 512 (obst, i) pairs under four fp32
 * evaluation orders). Layers 2-4 are unpinned: cv2 is absent here, and its thick line is a fixed-point polygon with
 * round caps whose rim pixels depend on the version; the capsule and the disc above are the shapes it approximates.
 * The vertices must be a convex polygon in outline order (either orientation; what sv_road_obstacles returns):
 * the device plans the outline as at most two pixel runs a row. */
/* One host frame, synchronous. bgr: H x W x 3 u8; obstacles: H x W u8, non-zero = obstacle; hull_pts: n x 2 int32
 * (x, y), 0 <= n <= 8192, |coordinate| <= 16383; info (nullable = no glyph): cx, cy, valid, tipx, tipy are read
 * (|cx|, |cy| <= 16383 when bit 1 of valid is set), info->n is not; out: H x W x 3 u8, not overlapping bgr.
 * 2 <= W <= 4096, 1 <= H <= 4096. SV_E_ARG for anything else, a polygon that is not convex included. */
int sv_result_image(const uint8_t* bgr, const uint8_t* obstacles, const int32_t* hull_pts, int64_t n,
                    const sv_hull_info* info, int H, int W, uint8_t* out);

/* ---- the image tile (stereovision.py:216, functions.py:452-499 batchImages) ---- */

/* The picture performStereoVision returns as img_tile, shows and records: batchImages of [Disparity, ImageRoadMap,
 * RoadImage, FilteredRoadImage, Result] with size = (H, W), every picture of the frame's size, so that resizeImage
 * is a copy and a grey picture becomes BGR by repeating its byte:
 *   S    = vstack(hstack(Disparity, ImageRoadMap), hstack(RoadImage, FilteredRoadImage))      2 H x 2 W x 3
 *   l    = cv2.resize(S, (0, 0), fx=0.25, fy=0.25):
 *          l[dy, dx, c] = (S[4dy+1, 4dx+1, c] + S[4dy+1, 4dx+2, c] + S[4dy+2, 4dx+1, c] + S[4dy+2, 4dx+2, c] + 2) >> 2
 *   r    = cv2.resize(Result, (0, 0), fx=0.5, fy=0.5):
 *          r[dy, dx, c] = (R[2dy, 2dx, c] + R[2dy, 2dx+1, c] + R[2dy+1, 2dx, c] + R[2dy+1, 2dx+1, c] + 2) >> 2
 *   tile = hstack(l, r)                                                                        H / 2 x W x 3
 * ImageRoadMap[y, x] = (0, 255, 0) where RoadImage[y, x] != 0, else the BGR (stereovision.py:131-133): it is not an
 * input, its quadrant is painted from the road picture. H and W must be multiples of 4, 4 <= H, W <= 4096: the
 * quadrants then meet on output-pixel boundaries (H / 4, W / 4) and no output pixel mixes two pictures. A road or
 * cleaned picture of 0 and 255 gives quadrant bytes of {0, 64, 128, 191, 255}, by the number of its four samples
 * that are set; other bytes are averaged as they are.
 * Not built by this entry point: tiles of frames whose H or W is no multiple of 4, pictures of other shapes than
 * the frame's (the 390 x 889 cropped disparity, which the reference first resizes to 544 x 1024 with cv2.resize's
 * general-scale bilinear filter) and lists of one to four pictures. Those go through the general-scale resize
 * below: sv_resize_linear_u8 for a picture, sv_images_tile for a list, sv_batch_resize_disp for a batch's
 * disparity. The whole tile of a cropped batch on the device is not built: that batch runs its road chain on the
 * 390 x 889 grid, while the reference in that mode cleans, hulls and draws 544 x 1024 pictures.
 * Parity with OpenCV is unpinned: cv2 is absent here. The argument for equality: INTER_LINEAR at scale 4 samples at
 * 4 dx + 1.5, so both weights are 1/2 = 1024 / 2048 in its 11-bit fixed point, and at scale 2 it is the 2 x 2 area
 * mean; all four weights are exactly 1/4, so any fixed-point or float implementation that rounds to nearest with
 * ties up gives this byte (tests/tile_numpy.py restates the 8-bit fixed-point path for any scale and
 * tests/test_tile_cpu.py checks it against the closed form). An implementation that rounds ties to even would
 * differ where the sum mod 4 is 2. */
/* One host frame, synchronous. disparity, road, cleaned: H x W u8; bgr, result: H x W x 3 u8; out: H / 2 x W x 3
 * u8, (B, G, R) per pixel, overlapping no input. SV_E_ARG for a NULL pointer, an overlap, or H or W that is not a
 * multiple of 4 in 4 .. 4096. */
int sv_image_tile(const uint8_t* disparity, const uint8_t* bgr, const uint8_t* road, const uint8_t* cleaned,
                  const uint8_t* result, int H, int W, uint8_t* out);

/* ---- general-scale bilinear resize (functions.py:452-454 resizeImage, :456-501 batchImages) ---- */

/* ---- the MJPG recording (loop.py:49-54,82-89: cv2.VideoWriter(name, MJPG, 8, (1024, 272)), write(image),
 * release()) ---- */
/* The picture the loop records leaves the device as a baseline JPEG stream, made on the GPU (kernels/jpeg.hip;
 * svx.video.VideoWriter puts the streams into the AVI). The stream of a BGR u8 picture of h x w, 1 .. 4096 each way
 * (tests/jpeg_numpy.py restates it): SOI, JFIF APP0, DQT x 2 (Annex K.1 / K.2 under the IJG quality
 * rule), SOF0 (Y 2 x 2, Cb and Cr 1 x 1), DHT x 4 (Annex K.3 - K.6), DRI = ceil(w / 16), SOS, one interleaved scan
 * with RSTn between the MCU rows, EOI. Colour, the 2 x 2 chroma means, the slow-integer DCT, the quantiser and the
 * entropy coder are libjpeg's, so the scan's bytes equal libjpeg's at the same quality with 4:2:0 and a restart
 * interval of one MCU row (checked against Pillow / libjpeg-turbo on the test list). Parity with OpenCV's own MJPG
 * encoder, a different one inside cv2, is unpinned.
 *
 * sv_jpeg_bound (loop.py:49-54,82-89): a capacity no stream of this definition exceeds: 640 bytes for the header
 * (it is 629), and for each of the ceil(h / 16) restart intervals its ceil(w / 16) MCUs at their worst code lengths
 * - 4 (20 + 63 * 26) + 2 (22 + 63 * 26) bits = 1244 bytes an MCU: a DC code with its bits is at most 9 + 11 bits
 * (luma) or 11 + 11 (chroma), an AC one 16 + 10 - every byte of them stuffed (x 2), and 2 bytes of RSTn or EOI.
 * 0 for dimensions outside 1 .. 4096. */
int64_t sv_jpeg_bound(int h, int w);
/* One host picture (loop.py:49-54,82-89, VideoWriter.write): rows ld >= 3 w bytes apart, quality 1 .. 100 (75 is
 * the writer's default). *size = the stream's length. SV_E_ARG for nulls, dimensions outside 1 .. 4096, quality
 * outside 1 .. 100, ld < 3 w or cap < 0. A stream longer than cap: SV_E_CAP with *size = the length it needs;
 * nothing is written to out then (and never past out + cap). */
int sv_jpeg_encode(const uint8_t* bgr, int h, int w, int64_t ld, int quality, uint8_t* out, int64_t cap,
                   int64_t* size);

/* The decoder of the MJPG playback (svx.video.VideoCapture, the counterpart of the cv2.VideoWriter of
 * loop.py:49-54,82-89; DESIGN §7.12, restated in tests/jpeg_decode_numpy.py): a baseline stream to the BGR picture
 * libjpeg-turbo's default path decodes from it (slow-integer IDCT, "fancy" h2v2 chroma upsampling, table colour
 * conversion), byte for byte for streams an encoder made from 8-bit pictures (checked against Pillow on the test
 * list; samples far out of range are clamped, as libjpeg's SIMD code does). Accepted: SOF0, 8 bit, three components
 * at 2 x 2, 1 x 1, 1 x 1 (4:2:0), one interleaved scan (Ss 0, Se 63, Ah = Al = 0), h and w 1 .. 4096, any 8-bit DQT
 * (ids 0 .. 3), any baseline DHT (the Annex K tables when the stream has none, as MJPG frames of other writers),
 * any DRI (without one the scan is a single interval: correct, and decoded by one lane), APPn and COM skipped.
 * Everything else - progressive, arithmetic, 12 bit, one or four components, 4:2:2 / 4:4:4, several scans, 16-bit
 * DQT, a segment that runs past the buffer - is refused by the host parser with SV_E_ARG and a message that names
 * what was met, before anything is launched. Malformed entropy-coded data never faults: the frame's status is one
 * of 1 a code in no table, 2 a DC size above 11 or an AC size above 10, 3 a run past coefficient 63, 4 a wrong
 * number of RSTn, 5 RSTn out of sequence, 6 no EOI (the largest that applies; 0: decoded), and the pixels of a
 * frame with a status are unspecified. */
typedef struct sv_jpeg_desc {
    int32_t h, w;
    int32_t restart_interval; /* MCUs; 0: the stream has no DRI */
    int32_t header_len;       /* SOI .. SOS: the entropy-coded bytes start here */
} sv_jpeg_desc;
/* On the host: what a stream of n bytes holds, or SV_E_ARG when it is not of the accepted kind. */
int sv_jpeg_info(const uint8_t* stream, int64_t n, sv_jpeg_desc* desc);
/* One host stream to one host picture of h x w (the stream's own size, else SV_E_ARG), rows ld >= 3 w bytes apart,
 * decoded on the device; *status as above. SV_E_ARG for nulls, dimensions outside 1 .. 4096 or ld < 3 w. */
int sv_jpeg_decode(const uint8_t* stream, int64_t n, uint8_t* bgr_out, int h, int w, int64_t ld, int32_t* status);
/* `count` streams packed back to back (as sv_batch_read_jpeg_packed writes them; offsets: count + 1 ascending
 * positions in packed, the last the end of the run) to count x h x w x 3 bytes of `out` and count statuses, on
 * `device`: one upload of the streams, one read-back of the pictures. Every stream must be h x w, else SV_E_ARG. */
int sv_jpeg_decode_many(int device, const uint8_t* packed, const int64_t* offsets, int count, int h, int w,
                        uint8_t* out, int32_t* status);
/* ms of the four kernels (marker scan, entropy walk, chroma planes, picture) of the device's last
 * sv_jpeg_decode_many, from HIP events, added up over its chunks; SV_E_STATE before the first. */
int sv_jpeg_decode_stage_ms(int device, float* ms4);

/* cv2.resize's 8-bit INTER_LINEAR path at any scale, as tests/tile_numpy.py restates it (resize_linear_u8): a
 * float32 source coordinate, int16 coefficients of 11-bit fixed point rounded half to even, an int32 horizontal
 * pass, the vertical pass's two >> 16 products and a final + 2 >> 2. Parity with OpenCV itself is unpinned: cv2 is
 * absent here; every result is bit for bit the restatement's.
 * The coefficient table of one axis, dn destination indices over sn source ones (host code, no device): with
 * scale = 1.0 / ((double)dn / sn) and f = (float)((dx + 0.5) * scale - 0.5), s = floor(f), f -= s; s < 0 gives
 * s = 0, f = 0 and s >= sn - 1 gives s = sn - 1, f = 0; s0[dx] = s, s1[dx] = min(s + 1, sn - 1),
 * c0[dx] = rint((1.f - f) * 2048.f), c1[dx] = rint(f * 2048.f), both half to even in float32. Fills dn entries of
 * each table. SV_E_ARG for a NULL table or dn or sn outside 1 .. 8192. The device reads these tables as they are. */
int sv_resize_coefficients(int dn, int sn, int32_t* s0, int32_t* s1, int16_t* c0, int16_t* c1);
/* n packed images of sh x sw x channels in, n packed images of dh x dw x channels out, one launch, synchronous:
 * cv2.resize(src[i], (dw, dh)). channels is 1 or 3; source dimensions 1 .. 8192, destination dimensions 1 .. 4096.
 * SV_E_ARG for a NULL pointer, dst overlapping src, n < 1 or a dimension out of range. */
int sv_resize_linear_u8(const uint8_t* src, int n, int sh, int sw, int channels, uint8_t* dst, int dh, int dw);

/* One picture of a batchImages list: h x w x channels u8, packed; channels 1 (grey) or 3 (BGR). */
typedef struct {
    const uint8_t* data;
    int h, w, channels;
} sv_picture;
/* batchImages(imgList, (H, W)) (functions.py:456-501) for count = 1 .. 5 pictures of any shapes within 1 .. 4096,
 * composed on the device as the reference composes it: every picture is resized to H x W by the resize above (one
 * already of that size too: the filter is then the identity), a grey one becomes BGR by repeating its byte, the
 * stack is built in device memory and resized by the same kernel:
 *   count 1: the resized picture                                                          H x W x 3
 *   count 2: resize(hstack(0, 1), fx = fy = 0.5)                                          H / 2 x W x 3, H even
 *   count 3: resize(vstack(hstack(0, 1), hstack(2, 2)), 0.5)                              H x W x 3
 *   count 4: resize(vstack(hstack(0, 1), hstack(2, 3)), 0.5)                              H x W x 3
 *   count 5: hstack(resize(that stack, 0.25), resize(picture 4, 0.5))                     H / 2 x W x 3, H, W even
 * H and W need not be multiples of 4: an output pixel of the left part may mix two pictures, and it is right
 * because the stack really exists. The fx / fy resize is built only where the stack's size is an exact multiple of
 * the scale, hence the even H (count 2) and the even H and W (count 5): elsewhere OpenCV takes its scale from fx
 * and not from the rounded dsize, and its scale-2 area path has a tail that is restated nowhere. For the list
 * sv_image_tile takes the two entry points give the same bytes.
 * sv_images_tile_shape: the output's rows and columns. sv_images_tile: out of that shape x 3, overlapping no
 * picture; one host call, synchronous. SV_E_ARG for a NULL pointer, an overlap, count outside 1 .. 5, channels
 * other than 1 or 3, a dimension out of range or an odd H or W excluded above. */
int sv_images_tile_shape(int count, int H, int W, int* oh, int* ow);
int sv_images_tile(const sv_picture* pics, int count, int H, int W, uint8_t* out);

/* ---- stereo rectification: the map pair and the remap (no reference function: its dataset ships rectified) ---- */
/* The maps are OpenCV's fixed-point pair, so cv2.initUndistortRectifyMap(..., m1type=CV_16SC2)'s can be handed in as
 * they are: xy is dh x dw x 2 int16 holding (sx, sy), frac is dh x dw uint16 holding fy * 32 + fx, 0 <= fx, fy < 32;
 * a frac entry >= 1024 is SV_E_ARG wherever a map is taken. The remap is cv2.remap's 8-bit INTER_LINEAR path with
 * BORDER_CONSTANT 0 as tests/rectify_numpy.py restates it: per destination pixel and channel, in int32,
 *   S(i, j) = src[sy + j][sx + i] inside the source, else 0                                  (i, j in {0, 1})
 *   dst = (w00 S(0,0) + w10 S(1,0) + w01 S(0,1) + w11 S(1,1) + 16384) >> 15
 *   w00 = 32 (32 - fx)(32 - fy), w10 = 32 fx (32 - fy), w01 = 32 (32 - fx) fy, w11 = 32 fx fy   (their sum is 32768)
 * Parity with OpenCV itself is unpinned: cv2 is absent here; every result is bit for bit the restatement's.
 * sv_rectify_map: initUndistortRectifyMap on the host in float64 (no device): K9 the raw camera's 3 x 3 matrix (fx,
 * fy, u0, v0 are read), D8 its distortion k1, k2, p1, p2, k3, k4, k5, k6 (the rational model with tangential terms),
 * R9 the rectifying rotation, P9 the new 3 x 3 camera matrix. Per destination (u, v): [X Y W] = inv(P R) [u v 1],
 * x = X / W, y = Y / W, r2 = x x + y y, kr = (1 + ((k3 r2 + k2) r2 + k1) r2) / (1 + ((k6 r2 + k5) r2 + k4) r2),
 * xd = x kr + p1 (2 x y) + p2 (r2 + 2 x x), yd = y kr + p1 (r2 + 2 y y) + p2 (2 x y), mu = fx xd + u0,
 * mv = fy yd + v0; iu = rint(32 mu), iv = rint(32 mv) half to even, clamped to [-32768 * 32, 32767 * 32 + 31], a
 * non-finite value becoming the lower bound; sx = iu >> 5, fx = iu & 31, likewise y. The inverse is the adjugate over
 * the determinant (parity with OpenCV's LU inverse to the last ulp is unpinned). SV_E_ARG for a NULL pointer, dh or dw
 * outside 1 .. 8192, or a zero or non-finite determinant of P R; nothing is written then. */
int sv_rectify_map(const double* K9, const double* D8, const double* R9, const double* P9, int dh, int dw, int16_t* xy,
                   uint16_t* frac);
/* n packed pictures of sh x sw x channels remapped through one map into n packed pictures of dh x dw x channels, one
 * launch, synchronous. channels is 1 or 3; source and destination dimensions 1 .. 8192; the destination has the map's
 * shape, which need not be the source's. SV_E_ARG for a NULL pointer, dst overlapping src, n < 1, channels other than
 * 1 or 3, a dimension out of range or a frac entry >= 1024, with nothing launched. */
int sv_remap_u8(const uint8_t* src, int n, int sh, int sw, int channels, const int16_t* xy, const uint16_t* frac,
                int dh, int dw, uint8_t* dst);

/* ---- the stages a2-a6 one by one (the stage drop-ins) ---------------------- */

/* calculatePointErrors (functions.py:300-312): out[i] = |(P_i . abc - 1) / d|
 * in fp64 with P.abc = fma(z, c, fma(x, a, y * b)) (OpenBLAS dgemv's order for
 * (N,3) x (3,1)); abcd = {a, b, c, d}, d as the reference's
 * math.sqrt computes it. xyz: n rows of stride ld >= 3 doubles. */
int sv_point_errors(const double* xyz, int64_t n, int64_t ld, const double* abcd, double* out);
/* BGRtoHSVHue + calculateColourHistogram (functions.py:73-78, :215-226): the
 * hue bin rint(h * 1000) of every (R, G, B) row (stride ld bytes; out_bins
 * nullable), the count of every bin (out_hist[1000]) and the index of its
 * first row (out_first[1000], -1 if empty; the dict's insertion order). */
int sv_hue_histogram(const uint8_t* rgb, int64_t n, int64_t ld, int16_t* out_bins, uint32_t* out_hist,
                     int64_t* out_first);
/* computePlanarThreshold (functions.py:314-323): indices i with vals[i] < thr
 * (NaN never), in order. filterPointsByHistogram (functions.py:228-230): indices
 * i with ok[bins[i]] != 0 (ok[1000] = hist[bin] > threshold), in order. */
int sv_select_less(const double* vals, int64_t n, double thr, int64_t* out_idx, int64_t* out_n);
int sv_select_bins(const int16_t* bins, int64_t n, const uint8_t* ok, int64_t* out_idx, int64_t* out_n);

/* ---- RANSAC plane fit --------------------------------- */

/* The draws of functions.py:278-298 RANSAC(points, trials), replayed exactly
 * as CPython's `random` makes them (MT19937, _randbelow, random.sample's pool
 * and set branches; per trial sample(points, k) then the non-collinear
 * triple of functions.py:240-260), starting from mt_state = random.getstate()'s
 * 624 words + index (advanced in place, for random.setstate). pts: n rows of
 * stride ld >= 3 doubles (X, Y, Z first). Outputs per trial: sidx (k indices),
 * tri (3 indices). *out_trials = trials, or 0 when n < k (sample raises before
 * drawing, so no trial runs and the state is untouched). Host only. */
int sv_ransac_draw(uint32_t* mt_state, const double* pts, int64_t n, int64_t ld, int trials, int k, int32_t* sidx,
                   int32_t* tri, int* out_trials);
/* sv_ransac_draw, then every trial on the GPU: out_abc (trials x 3) =
 * inv([P1;P2;P3]) 1 (functions.py:267), out_err = mean |P.abc - 1| / |abc| over
 * the trial's sample (functions.py:269-275, :289), out_flag = 0 ok, 1 singular,
 * 2 ill-conditioned (the caller re-decides flagged trials and the near-best
 * ones with the reference's own numpy calls). */
int sv_ransac(uint32_t* mt_state, const double* pts, int64_t n, int64_t ld, int trials, int k, int32_t* sidx,
              int32_t* tri, double* out_abc, double* out_err, uint8_t* out_flag, int* out_trials);

/* ---- disparity stage, host images, synchronous ------ */

/* cv2.StereoSGBM_create(minDisparity, numDisparities, blockSize, P1, P2,
 * disp12MaxDiff, preFilterCap, uniquenessRatio) — functions.py:26 creates it
 * as (0, 128, 21) with the other fields 0. OpenCV's substitutions for zero
 * fields are applied (P1 -> 2, P2 -> max(5, P1 + 1), preFilterCap ->
 * max(cap, 15) | 1, disp12MaxDiff -> 1, uniquenessRatio < 0 -> 10); mode is
 * MODE_SGBM, speckleWindowSize 0. Supported: min_disp 0, num_disp 128, odd
 * block <= 63, 128 + block/2 < W <= 2048. */
typedef struct {
    int min_disp, num_disp, block, P1, P2, disp12_max_diff, prefilter_cap, uniqueness;
} sv_sgbm_params;

/* cv2.LUT(image, table) of gammaChange (functions.py:61-67): out[i] = lut[in[i]]
 * over n bytes (any channel count; the table is built by the caller, as the
 * reference builds it in numpy). */
int sv_lut_u8(const uint8_t* in, int64_t n, const uint8_t* lut, uint8_t* out);
/* One image of greyscale (functions.py:89-97): cv2.cvtColor(BGR2GRAY)
 * (fixed point, (B*1868 + G*9617 + R*4899 + 2^13) >> 14) then
 * cv2.equalizeHist. bgr: H x W x 3 contiguous. */
int sv_grey_equalize(const uint8_t* bgr, int H, int W, uint8_t* out);
/* stereoProcessor.compute(grayL, grayR) (functions.py:108): H x W int16
 * disparity x16, -16 where invalid — computeDisparitySGBM followed, as in
 * OpenCV's StereoSGBM::compute, by medianBlur(disp, disp, 3) (exact 3 x 3
 * median, replicated border). SV_E_RANGE when a path cost leaves int16
 * (block cost sums above 32,763; OpenCV's int16 buffers would truncate). */
int sv_sgbm_compute(const uint8_t* L, const uint8_t* R, int H, int W, const sv_sgbm_params* prm, int16_t* out);
/* cv2.filterSpeckles(img, newVal, maxSpeckleSize, maxDiff) on int16, in place
 * (functions.py:111): 4-connected regions of pixels != newVal joined where
 * neighbours differ by <= maxDiff; regions of <= maxSpeckleSize pixels are set
 * to newVal. */
int sv_filter_speckles(int16_t* img, int H, int W, int new_val, int max_size, int max_diff);
/* functions.py:104-128 disparity(grayL, grayR, max_disparity, crop_disparity):
 * SGBM -> filterSpeckles(0, 4000, max_disparity - 5) -> threshold TOZERO at 0
 * -> (d / 16.).astype(uint8) -> crop [0:390, 135:W] when crop != 0 ->
 * (x * (256. / max_disparity)).astype(uint8). out: rows x cols u8 with rows =
 * crop ? min(390, H) : H, cols = crop ? W - 135 : W. raw16 / filt16 (nullable,
 * H x W): the compute() result (after its medianBlur) before / after
 * filterSpeckles. */
int sv_disparity(const uint8_t* L, const uint8_t* R, int H, int W, const sv_sgbm_params* prm, int max_disparity,
                 int crop, uint8_t* out, int16_t* raw16, int16_t* filt16);

/* ---- batched, device-resident API ------------- */
typedef struct sv_batch sv_batch;

/* frames x H x W uint8 disparity (+ frames x H x W x 3 BGR if with_bgr) in
 * HBM. Any W >= 2: rows are stored at a stride of round_up(W, 8) bytes (the
 * pad columns lie outside every grid; uploads and read-backs use W), so the
 * 390 x 889 frames of crop_disparity=True (functions.py:122-124) run fused;
 * sv_batch_synth / the batched SGBM need W % 8 == 0. Dense outputs: 3 fp32 planes (X, Y, Z) of
 * frames x Hg x pitch, pitch = round_up(Wg, 4); Z == 0 marks d == 0 / pad. */
int sv_batch_create(int device, int frames, int H, int W, int step, int with_bgr,
                    int with_points, sv_batch** out);
int sv_batch_destroy(sv_batch* b);
int sv_batch_info(const sv_batch* b, int64_t* out8); /* Hg, Wg, pitch, Ng, bytes, frames, H, W */
/* K1 launch shape: qpl = quads (4 grid points) per lane, 1, 2 or 4 (0 = 1);
 * nontemporal = 1 for non-temporal (streaming) stores, 2 for the same kernel
 * (qpl 1, non-temporal) as a separately named instance: a profiler keeps its
 * launches in a statistics row of their own. */
int sv_batch_tune(sv_batch* b, int qpl, int nontemporal);

/* Counter-based synthetic frames for global frame ids first..first+frames-1
 * (SURVEY §8d), generated on the device: inputs never cross PCIe. */
int sv_batch_synth(sv_batch* b, int64_t first_frame_id);
/* Upload one host frame (tests / real data). bgr may be NULL. */
int sv_batch_upload(sv_batch* b, int frame, const uint8_t* disp, const uint8_t* bgr);

/* K1: dense projection of every frame (configs 2/3). Asynchronous on the
 * batch stream unless sync != 0. */
int sv_batch_project(sv_batch* b, const sv_camera* cam, int sync);

/* K2+K3: plane threshold + hue histogram + stable compaction + int32
 * back-projection for every frame (config 4). chunk = frames per
 * histogram/compaction wave (0 = library default). */
int sv_batch_pipeline(sv_batch* b, const sv_camera* cam, const sv_plane* plane,
                      double point_thr, int hist_thr, int chunk, int sync);

/* The pipeline with every frame's own plane: the plane the last
 * sv_batch_ransac found for it (stereovision.py:94-113 per frame). A frame
 * without a plane (trial -1: the reference's plane step raises) keeps no
 * points. Same kernel families as sv_batch_pipeline (the frame-resident
 * kernel reads each frame's plane). sv_batch_read_frame_plane: a, b, c and
 * |abc| (-1 without a plane) as the kernels use them. */
int sv_batch_pipeline_planes(sv_batch* b, const sv_camera* cam, double point_thr, int hist_thr, int chunk,
                             int sync);
/* sv_batch_pipeline with the plane in DEVICE memory (3 doubles a, b, c on the
 * batch's device, e.g. the buffer an RCCL broadcast wrote): read by the
 * device, so the call needs no host copy of the plane and no host sync. */
int sv_batch_pipeline_dev(sv_batch* b, const sv_camera* cam, const double* dplane, double point_thr, int hist_thr,
                          int chunk, int sync);
int sv_batch_read_frame_plane(sv_batch* b, int frame, double* out4);

/* Pipeline kernel family: 0 = auto (frame-resident for >= 512 frames when the
 * frame fits, else tiled), 1 = tiled (tiles of 4096 points across workgroups,
 * offsets kernel between the passes), 2 = frame-resident (one workgroup per
 * frame, LDS histogram; frames of <= 1M grid points and <= 2048 grid points a
 * side, else SV_E_ARG; chunks the plane rules out are skipped; both passes
 * prefetch the next chunk; no host sync), 3 = frame-resident without prefetch,
 * 4 = frame-resident with the pass-2 prefetch only. Results are identical;
 * only the speed differs. */
int sv_batch_pipeline_mode(sv_batch* b, int mode);

/* Pre-pass over the batch's frames in order (stereovision.py:53-76): option
 * 1 = fillDisparity with the previous CLEANED frame (frame 0 uses prev0, or is
 * left as is when prev0 is NULL), 2 = fillAltDisparity, 0 = none. The cleaned
 * disparity replaces the batch's; with a mask set (sv_batch_set_mask, the grey
 * carmask, NULL clears it) the masked disparity of functions.py:169-172 is
 * also written (sv_batch_read_disp). capDisparity (functions.py:164-167)
 * returns its input unchanged, so it has no kernel. */
int sv_batch_set_mask(sv_batch* b, const uint8_t* mask);
int sv_batch_prepass(sv_batch* b, int option, const uint8_t* prev0, int sync);
int sv_batch_read_disp(sv_batch* b, int frame, uint8_t* disp, uint8_t* masked);

/* Road images of the pipeline's int32 points (generatePointsAsImage per
 * frame), their raster-order non-zero walks, and read-back (img and/or the
 * walk; n receives the walk's length). sv_batch_road_raster writes the images
 * and their walks in one pass, so the walks are already current and
 * sv_batch_nonzero only orders/syncs. */
int sv_batch_road_raster(sv_batch* b, int sync);
int sv_batch_nonzero(sv_batch* b, int sync);
int sv_batch_read_road(sv_batch* b, int frame, uint8_t* img, int32_t* nzpts, int64_t cap, int64_t* n);
/* stereovision.py:131-133 imageRoadMap: with enable != 0, later
 * sv_batch_road_raster calls also write, in the same pass, a copy of each
 * frame's BGR (the corrected imgL the pipeline read its colours from) with
 * [0, 255, 0] at every [x, y] of its int32 planePoints (numpy's negative
 * indices wrap as in the road image). Needs a with_bgr batch. For a batch of
 * crop_disparity=True frames the map covers the batch's H x W (the top-left of
 * the 544 x 1024 imgL; the rest of imgL is unpainted, as the pipeline's points
 * never leave the disparity's own grid). Read-back: H x W x 3 u8. */
int sv_batch_road_map(sv_batch* b, int enable);
/* With enable != 0, later frame-resident pipeline calls on 1024-wide frames at step 1 also write a bitmap of
 * the pixels their int32 points mark (pass 2 marks them as it makes the points; 68 KB a frame), and the next
 * sv_batch_road_raster builds the images, walks and imageRoadMap from it — one wave a row — instead of
 * re-reading the points (8 B each). The outputs are the same either way; other shapes and the tiled kernels
 * keep the points path. */
int sv_batch_road_bits(sv_batch* b, int enable);
int sv_batch_read_road_map(sv_batch* b, int frame, uint8_t* out);
/* sanitiseRoadImage's clean-up (sv_sanitise_road's steps 1-6) of every frame's road image, on the device.
 * sv_batch_road_mask: the H x W road_threshold_mask of step 3 (NULL clears it to all ones).
 * sv_batch_road_clean needs a current road pass (sv_batch_road_raster after the last pipeline call, else
 * SV_E_STATE); it reads the pipeline's road bitmap when that is fresh (sv_batch_road_bits) and packs the road
 * images otherwise, and writes the cleaned images and their walks into buffers of its own:
 * sv_batch_read_road keeps returning the raw image and walk, sv_batch_read_road_clean (same contract) the
 * cleaned ones. 1024-wide frames of up to 1024 rows get image and walk from the bitmap road pass, others from
 * an unpack kernel and the non-zero walk. */
int sv_batch_road_mask(sv_batch* b, const uint8_t* mask);
int sv_batch_road_clean(sv_batch* b, int sync);
int sv_batch_read_road_clean(sv_batch* b, int frame, uint8_t* img, int32_t* nzpts, int64_t cap, int64_t* n);
/* ms of the last sv_batch_road_clean from HIP events on the batch stream: *kernel_ms the clean-up kernel alone,
 * *total_ms the whole call's device work (pack, clean-up, image + walk). Synchronises the batch stream. */
int sv_batch_road_clean_ms(sv_batch* b, float* kernel_ms, float* total_ms);
/* The obstacle stage (sv_road_obstacles) of every frame's cleaned image, on the device: one kernel that reads the
 * clean-up's bitmaps. SV_E_STATE unless a clean-up is current (sv_batch_road_clean after the last road pass); any
 * call that invalidates the clean-up invalidates the hull too. disparity = the batch's cleaned, unmasked frames
 * (what sv_batch_read_disp returns); abc = the plane the frame's last pipeline call used: the frame's own RANSAC
 * plane (sv_batch_pipeline_planes; none found: bit 1 of valid clear), else the call's shared plane.
 * 1 <= H <= 4096. */
int sv_batch_road_hull(sv_batch* b, int sync);
/* One frame's results; every pointer is nullable. hull_pts: cap x 2 int32 (SV_E_CAP, info->n set, when cap <
 * n); hull_mask, obstacles: H x W u8 of 0 / 255. */
int sv_batch_read_road_hull(sv_batch* b, int frame, int32_t* hull_pts, int64_t cap, uint8_t* hull_mask,
                            uint8_t* obstacles, sv_hull_info* info);
/* ms of the last sv_batch_road_hull from HIP events on the batch stream. Synchronises the batch stream. */
int sv_batch_road_hull_ms(sv_batch* b, float* ms);
/* The obstacle list (sv_obstacle_list) of every frame, on the device: one kernel that reads the obstacle stage's
 * bitmaps and the batch's cleaned, unmasked disparity (what sv_batch_read_disp returns), and writes frames x cap
 * entries and the counts into a buffer of its own. A side branch of the road chain: it needs a current obstacle
 * stage (SV_E_STATE without sv_batch_road_hull after the last clean-up) and raises no level, so the result image
 * and the tile neither need it nor undo it; a new sv_batch_road_hull, and whatever invalidates the obstacle stage,
 * invalidates the list. min_area >= 1, 1 <= cap <= 32 (SV_E_ARG). The labelling scratch is sized by the frame's
 * shape alone (csrc/svx_objects_host.h: at most 2 GiB, 1024 workgroups' worth), allocated by the first call. */
int sv_batch_obstacle_list(sv_batch* b, int min_area, int cap, int sync);
/* One frame's list: *n = its count in full, out (cap entries) = the first min(*n, cap) entries. A cap below the
 * call's gives the head of the list; one above it is SV_E_ARG. SV_E_STATE without a current list. The first read
 * after a call synchronises the batch stream and copies every frame's list to the host at once (56 cap + 4 bytes a
 * frame); later reads of that call's lists touch no device. */
int sv_batch_read_obstacle_list(sv_batch* b, int frame, sv_obstacle* out, int cap, int32_t* n);
/* ms of the last sv_batch_obstacle_list from HIP events on the batch stream. Synchronises the batch stream. */
int sv_batch_obstacle_list_ms(sv_batch* b, float* ms);
/* The ground grid (sv_ground_grid) of every frame, on the device: one kernel that reads the obstacle stage's
 * obstacle bitmap, the clean-up's cleaned bitmap and the batch's cleaned, unmasked disparity (what
 * sv_batch_read_disp returns; x and y are the batch's own indices), and writes a buffer of its own, frames x
 * (2 nx nz + nx + 4) x 4 bytes, allocated by the first call: every frame's two planes, then every frame's nearest
 * profile, then every frame's info. grid: nullable (the default). A side branch of the road chain with the obstacle
 * list's state rules: it needs a current obstacle stage (SV_E_STATE without sv_batch_road_hull after the last
 * clean-up) and raises no level, so the result image, the tile, the JPEG streams and the list neither need it nor
 * undo it; a new sv_batch_road_hull, and whatever invalidates the obstacle stage, invalidates the grid. SV_E_ARG as
 * for sv_ground_grid. */
int sv_batch_ground_grid(sv_batch* b, const sv_camera* cam, const sv_grid* grid, int min_count, int sync);
/* One frame's grid; every pointer is nullable. obst, road: nz x nx uint32; nearest: nx int32; info: 4 int32, of the
 * last sv_batch_ground_grid's grid. SV_E_STATE without a current grid. Synchronises the batch stream. */
int sv_batch_read_ground_grid(sv_batch* b, int frame, uint32_t* obst, uint32_t* road, int32_t* nearest,
                              int32_t* info);
/* Every frame's nearest profile in one copy: out = frames x nx int32. */
int sv_batch_read_ground_nearest(sv_batch* b, int32_t* out);
/* ms of the last sv_batch_ground_grid from HIP events on the batch stream. Synchronises the batch stream. */
int sv_batch_ground_grid_ms(sv_batch* b, float* ms);
/* The result image (sv_result_image) of every frame, on the device: one kernel that reads the batch's BGR (the
 * image the pipeline read its colours from; left unchanged) and the obstacle stage's bitmaps, vertices and infos,
 * and writes a buffer of its own (frames x H x W x 3 bytes, allocated by the first call). SV_E_STATE without a
 * current obstacle stage (sv_batch_road_hull after the last clean-up) or on a batch created without BGR; whatever
 * invalidates the obstacle stage invalidates the result. For a batch of cropped frames (sv_batch_pair_shape) the
 * result covers the batch's H x W, like sv_batch_road_map. H, W <= 4096. */
int sv_batch_result(sv_batch* b, int sync);
/* One frame's result image, H x W x 3 u8. */
int sv_batch_read_result(sv_batch* b, int frame, uint8_t* out);
/* ms of the last sv_batch_result from HIP events on the batch stream. Synchronises the batch stream. */
int sv_batch_result_ms(sv_batch* b, float* ms);
/* The image tile (sv_image_tile) of every frame, on the device: one kernel that reads the batch's cleaned
 * disparity (what sv_batch_read_disp returns), its BGR, the road picture, the cleaned road picture and the result
 * image, and writes a buffer of its own. imageRoadMap's quadrant is painted from the road picture as it is read,
 * so sv_batch_road_map need not be on. The two road pictures are read as packed bitmaps where the batch holds
 * current ones (the clean-up's always, the pipeline's own after sv_batch_road_bits on 1024-wide frames), else as
 * the u8 images; the bytes written are the same. The buffer holds frames x H / 2 rows of 3 W bytes with no
 * padding, so one copy reads a tile or a run of tiles; it is allocated by the first call and takes 3.4 GB per
 * 4096 frames of 544 x 1024. SV_E_STATE without a current result image (sv_batch_result after the last obstacle
 * stage) or on a batch created without BGR; whatever invalidates the result invalidates the tile. SV_E_ARG unless
 * H and W are multiples of 4 (4 .. 4096). */
int sv_batch_tile(sv_batch* b, int sync);
/* One frame's tile, H / 2 x W x 3 u8. */
int sv_batch_read_tile(sv_batch* b, int frame, uint8_t* out);
/* ms of the last sv_batch_tile from HIP events on the batch stream. Synchronises the batch stream. */
int sv_batch_tile_ms(sv_batch* b, float* ms);
/* The JPEG stream (sv_jpeg_encode; loop.py:49-54,82-89) of every frame's tile, on the device, each into a slot of
 * cap_per_frame bytes (0: half the raw tile, at least 2048; noise at quality 75 takes 0.20 of the raw bytes, at 100
 * 0.66). The coefficients go through a scratch of 3 B a pixel in chunks of frames sized from the free memory. A frame
 * whose stream is longer than the slot is flagged in its size and not written; the call still succeeds. SV_E_STATE
 * without a current tile (sv_batch_tile); whatever invalidates the tile invalidates the streams. SV_E_ARG for a
 * quality outside 1 .. 100 or a capacity outside 0 .. 2^31 - 1. */
int sv_batch_jpeg(sv_batch* b, int quality, int64_t cap_per_frame, int sync);
/* The lengths of the streams of sv_batch_jpeg (loop.py:49-54,82-89), frames x int32; negative: the frame
 * overflowed its slot, minus the length it needs. */
int sv_batch_jpeg_sizes(sv_batch* b, int32_t* out);
/* One frame's stream (loop.py:49-54,82-89: what VideoWriter.write would encode of that frame's tile). *size = its
 * length; SV_E_CAP when the frame overflowed its slot or cap is smaller than the stream (*size = what it needs). */
int sv_batch_read_jpeg(sv_batch* b, int frame, uint8_t* out, int64_t cap, int64_t* size);
/* The batch's streams back to back in frame order (loop.py:49-54,82-89, a batch's worth of write calls): an
 * exclusive scan of the sizes and one copy kernel on the device, then sv_batch_read_jpeg_packed copies exactly their
 * bytes in one transfer. offsets: frames x int64, each frame's start (a frame that overflowed its slot contributes
 * nothing: its offset equals the next one's); *total = the bytes of the run. SV_E_STATE before sv_batch_jpeg_pack of
 * the current streams; SV_E_CAP (with *total set) when cap < total. */
int sv_batch_jpeg_pack(sv_batch* b, int sync);
int sv_batch_read_jpeg_packed(sv_batch* b, uint8_t* out, int64_t cap, int64_t* offsets, int64_t* total);
/* ms of the last sv_batch_jpeg (loop.py:49-54,82-89's encode) from HIP events on the batch stream. Synchronises
 * the batch stream. */
int sv_batch_jpeg_ms(sv_batch* b, float* ms);
/* The cleaned disparity of every frame (what sv_batch_read_disp returns) at a display size, on the device:
 * cv2.resize(disp, (dw, dh)) by sv_resize_linear_u8's kernel in one launch over the resident frames, read at the
 * batch's row stride, into a buffer of its own (frames x dh x dw bytes, packed; allocated by the first call). For a
 * crop_disparity batch of 390 x 889 and (544, 1024) it is the Disparity picture of that mode's tile. Whatever
 * replaces the cleaned disparity (an upload, synthetic frames, SGBM, a pre-pass) makes it stale: reads and _ms then
 * give SV_E_STATE, as before the first call. SV_E_ARG for dh or dw outside 1 .. 4096 or frames beyond 8192 x 8192. */
int sv_batch_resize_disp(sv_batch* b, int dh, int dw, int sync);
/* One frame's resized disparity, dh x dw u8. */
int sv_batch_read_resized_disp(sv_batch* b, int frame, uint8_t* out);
/* ms of the last sv_batch_resize_disp from HIP events on the batch stream. Synchronises the batch stream. */
int sv_batch_resize_disp_ms(sv_batch* b, float* ms);

/* Batched RANSAC (stereovision.py:84-94 for every frame):
 * maskpoints = the fp64 step-2 projection of the batch's disparity under the
 * mask set by sv_batch_set_mask (functions.py:169-172, :178-198), then
 * RANSAC(maskpoints, trials) (functions.py:278-298) with the draws CPython
 * makes after random.seed(seed_base + first_frame + frame) — replayed on the
 * device, one workgroup per frame. Per frame: abc (the plane), err (its mean
 * distance), trial (the winning trial, -1 when fewer than k points: the
 * reference returns (None, None)), flags (1: a trial was singular and
 * skipped; 2: unused since round 3; 4: the runner-up's error is within 1e-9
 * relative, information only: planes, errors and the choice are computed with
 * numpy's rounding — LAPACK dgesv + dot, gemv, pairwise mean — so abc, err and
 * trial equal the reference's bit for bit; 8: every triple drawn in 65,536 attempts was collinear
 * — the reference never returns there — trial = -1; 16: more than 2^28
 * draws in one frame, trial = -1; 32: a frame above the launch's size bound,
 * trial = -1 — cannot happen while the bound holds). Step-2 grids of
 * <= 163,840 points, frames up to 4096 x 4096; 1 <= k <= 1024. The kernels'
 * LDS is sized for the largest frame: with a mask set (the reference always
 * masks, stereovision.py:74-85) from the mask's own step-2 points, an upper
 * bound of every frame's count, so the call enqueues everything without a
 * host wait; without a mask (or a mask too large for 8 KiB of sample LDS) it
 * waits for the maskpoints counts (one small read-back). `sync` then applies
 * to the RANSAC kernels. */
int sv_batch_ransac(sv_batch* b, const sv_camera* cam, uint64_t seed_base, int64_t first_frame, int trials, int k,
                    int sync);
int sv_batch_read_ransac(sv_batch* b, int frame, double* abc, double* err, int32_t* trial, uint32_t* flags);
int sv_batch_read_maskpoints(sv_batch* b, int frame, double* xyz, int64_t cap, int64_t* n);
/* Draw-level verification: record the first `trials` trials' drawn indices of
 * every frame in later sv_batch_ransac calls (0 = off); read one frame's as
 * trials x (k + 3) int32 (the sample, then P1..P3 of the accepted triple;
 * -1 where a trial did not run), trials and k being those of the last
 * sv_batch_ransac (*out_trials, *out_k; out NULL: sizes only; cap = int32
 * capacity of out, SV_E_CAP if smaller). */
int sv_batch_ransac_trace(sv_batch* b, int trials);
int sv_batch_read_ransac_trace(sv_batch* b, int frame, int32_t* out, int64_t cap, int* out_trials, int* out_k);

/* Stereo pairs resident in HBM (frames x Hp x Wp grey left / right) and the
 * batched disparity stage: sv_batch_sgbm runs functions.py:104-128 on every
 * pair and writes the batch's disparity (frames x H x W u8), the input of the
 * pre-pass, K1 and the pipeline. The pairs have the batch's shape (no crop)
 * unless sv_batch_pair_shape(b, Hp, Wp) sets the uncropped one: then the batch
 * (H = min(390, Hp), W = Wp - 135) receives disparity_scaled[0:390, 135:Wp],
 * crop_disparity=True (functions.py:122-124). Wp % 8 == 0. chunk = frames per
 * cost-volume chunk (0 = 32; 4 x 125 MB of int16 volumes per 1024 x 544
 * frame). Synchronous per chunk (the int16 range flags are read back).
 * sv_batch_synth_pair: synthetic rectified pairs for global frame ids
 * first.., generated on the device (row y's true disparity is the synthetic
 * road's, halved: clamp(floor(3(y - 200) / 10), 0, 127)). */
int sv_batch_pair_shape(sv_batch* b, int H, int W);
/* The front end of performStereoVision (stereovision.py:44-46) for the batch:
 * BGR stereo pairs (frames x Hp x Wp x 3, the pair shape above) uploaded or
 * generated on the device, then sv_batch_preprocess applies the gamma table
 * `lut` (256 bytes: functions.py:61-67's table for gamma 1.4, built by the
 * caller) to both images in place (preProcessImages, :81-87), writes
 * BGR2GRAY + equalizeHist of both (greyscale, :89-97) as the SGBM pairs, and,
 * for a batch with BGR, copies the corrected left image's top-left H x W into
 * the batch's BGR (the colours projectDisparityTo3d reads at the disparity's
 * own (y, x), cropped or not). */
int sv_batch_upload_bgr_pair(sv_batch* b, int frame, const uint8_t* L, const uint8_t* R);
int sv_batch_synth_bgr_pair(sv_batch* b, int64_t first_frame_id);
/* The same storage filled from JPEG streams (sv_jpeg_decode_many's kind and layout: two packed runs of `count`
 * streams of the pair shape, offsets of count + 1 entries each) decoded on the device into frames first ..
 * first + count - 1: a tenth of sv_batch_upload_bgr_pair's bytes over the host link. status: count statuses of the
 * left streams, then count of the right ones (sv_jpeg_decode). It invalidates what an upload invalidates (nothing:
 * sv_batch_preprocess reads the pairs anew). sv_batch_decode_ms: the ms of the last call's kernels from HIP events.
 * sv_batch_read_bgr_pair: one frame's stored pair back (2 x Hp x Wp x 3 bytes). */
int sv_batch_decode_bgr_pair(sv_batch* b, int first, int count, const uint8_t* packedL, const int64_t* offsL,
                             const uint8_t* packedR, const int64_t* offsR, int32_t* status);
int sv_batch_decode_ms(sv_batch* b, float* ms);
int sv_batch_read_bgr_pair(sv_batch* b, int frame, uint8_t* L, uint8_t* R);
/* Rectification of the stored BGR pairs, between upload / decode / synth and sv_batch_preprocess, for cameras that
 * deliver distorted, unaligned pictures (the maps and the remap: sv_rectify_map, sv_remap_u8 above).
 * sv_batch_rectify_maps: the two eyes' maps of the pair shape (Hp x Wp x 2 int16 and Hp x Wp uint16 each), uploaded
 * and kept until replaced; sv_batch_pair_shape with a new shape drops them. SV_E_ARG for a NULL pointer or a frac
 * entry >= 1024.
 * sv_batch_rectify: every frame's pair through its eye's map, both eyes in one launch. The gather cannot run in
 * place: the first call allocates a second store of the pairs' size (2 x frames x Hp x Wp x 3 bytes) and the two
 * change places, so afterwards sv_batch_read_bgr_pair returns the rectified pairs and sv_batch_preprocess consumes
 * them, while the pictures as they came are kept: a pair written later lands beside them, and the next call
 * rectifies every frame from its raw picture. SV_E_STATE without maps of the current pair shape, without a BGR pair
 * store, or when no pair was uploaded, decoded or generated since the last call (the pairs are rectified already).
 * The stores change back when a write of a pair BEGINS (once its arguments are accepted), not when it succeeds: after
 * an upload whose copy fails, or a decode whose streams give statuses or that fails midway, sv_batch_read_bgr_pair
 * and sv_batch_preprocess see the raw pictures of every frame until the next sv_batch_rectify, which is allowed.
 * The camera to hand to the later stages is the rectified pair's: f = P[0][0], B = -P_right[0][3] / f, cw = P[0][2],
 * ch = P[1][2] of stereoRectify's projections. A batch that never calls it behaves as before.
 * sv_batch_rectify_ms: the ms of the last call's kernel from HIP events; SV_E_STATE before the first. */
int sv_batch_rectify_maps(sv_batch* b, const int16_t* xyL, const uint16_t* fracL, const int16_t* xyR,
                          const uint16_t* fracR);
int sv_batch_rectify(sv_batch* b, int sync);
int sv_batch_rectify_ms(sv_batch* b, float* ms);
int sv_batch_preprocess(sv_batch* b, const uint8_t* lut, int sync);
int sv_batch_synth_pair(sv_batch* b, int64_t first_frame_id);
int sv_batch_upload_pair(sv_batch* b, int frame, const uint8_t* L, const uint8_t* R);
int sv_batch_sgbm(sv_batch* b, const sv_sgbm_params* prm, int max_disparity, int chunk);

int sv_batch_sync(sv_batch* b);
/* ms of the last sv_batch_project / sv_batch_pipeline / sv_batch_sgbm, from
 * HIP events recorded on the batch stream around the kernels. which: 0 =
 * project, 1 = pipeline, 2 = sgbm. */
int sv_batch_last_ms(sv_batch* b, int which, float* ms);
/* Sum of the per-launch durations (HIP events on the batch stream around each
 * K1 launch / each pipeline call) since the last reset, and their count.
 * Synchronises the batch stream. */
int sv_batch_timing(sv_batch* b, int which, double* total_ms, int64_t* count);
int sv_batch_timing_reset(sv_batch* b);
/* The placement probe of a large batch's first call (which: 0 = K1's X/Y/Z planes, k1_place; 1 = the resident
 * pipeline's four output planes (X, Y, Z and the packed planePoints word), pipe_place; 2 = the SGBM cost volumes, sgbm_place): up to 3 (SGBM: 2) sets are
 * allocated and one call is timed on each (the pipeline: the faster of two passes; SGBM: the first chunk's
 * compute, the second of two runs); the fastest set is kept. ms[0..n-1] = each set's timed call, *kept = the
 * kept set's index (-1 when no probe ran: small batch or chunk, too little free memory). */
int sv_batch_placement(sv_batch* b, int which, float* ms, int cap, int* n, int* kept);
/* The kernel instance the last sv_batch_project (which 0) / sv_batch_pipeline* (1) call launched, as rocprofv3
 * names it (e.g. "svx::resident_fused_kernel<1, 4, true, true, true, false>"; the tiled pipeline's two kernels;
 * 2: "sgbm stage"), NUL-terminated into buf[cap]: a PMC profile of that name is the timed kernel's. SV_E_STATE
 * before the first call. */
int sv_batch_kernel_name(sv_batch* b, int which, char* buf, int cap);
/* sha256 (16 hex) of the sources this library's K1 (which 0: kernels/project.hip + the device headers) or resident
 * pipeline (1: kernels/resident.hip, kernels/tables.hip + the device headers) was compiled from, fixed at build time:
 * a PMC profile records it, and a profile counts for the timed kernel only when the ids agree. */
int sv_source_id(int which, char* buf, int cap);

/* Read back. */
int sv_batch_read_dense(sv_batch* b, int frame, float* X, float* Y, float* Z);
int sv_batch_read_counts(sv_batch* b, int64_t* counts /* frames x 3 */);
int sv_batch_read_hist(sv_batch* b, int frame, uint32_t* hist /* 1024 */);
int sv_batch_read_points(sv_batch* b, int frame, float* xyz, int32_t* pts, int64_t cap, int64_t* n);

/* ---- software-pipelined frame loop (stereovision.py:53-136, minus the cv2 drawing) -------------- */
/* The reference's per-frame loop (loop.py:59-78 -> performStereoVision) over a SEQUENCE of device batches:
 * every batch goes through input -> pre-pass (functions.py:130-172) -> maskpoints (stereovision.py:74-85) ->
 * RANSAC (functions.py:278-298, stereovision.py:94) -> the pipeline with each frame's own plane
 * (stereovision.py:97-113) -> road raster + non-zero walk (+ imageRoadMap) (stereovision.py:131-156,
 * functions.py:339-365), on its slot's stream; RANSAC runs as two stages (the draw replay, the evaluation).
 * Each stage of batch k also waits for the same stage of batch k - 1, and the evaluation for batch k - 1's
 * road pass, so with slots = 2 the draw of batch k + 1 (one wave's dependent chain per frame) runs beside the
 * HBM-bound pipeline and road pass of batch k, and the evaluation of batch k + 1 (a CU's LDS per frame)
 * beside the pre-pass and maskpoints of batch k + 2. fillDisparity's previous cleaned frame is carried from batch to
 * batch, so the results equal one long batch's (frame g draws after random.seed(seed_base + g)). */
typedef struct {
    int frames;          /* frames per batch                                                          */
    int H, W, step;      /* frame shape; pipeline grid step (1, or the reference's 2)                  */
    int slots;           /* batches in flight (1..8; 2 = the software pipeline)                        */
    int source;          /* 0: the caller fills each batch (sv_loop_acquire + sv_batch_upload / sv_batch_sgbm);
                            1: synthetic frames of the batch's global ids, generated on the device      */
    int prepass;         /* 0 none, 1 fillDisparity with the previous cleaned frame, 2 fillAltDisparity */
    int trials, k;       /* RANSAC trials and sample size (600, 600)                                    */
    uint64_t seed_base;  /* frame g draws what CPython draws after random.seed(seed_base + g)           */
    double point_thr;    /* computePlanarThreshold threshold (0.05)                                    */
    int hist_thr;        /* filterPointsByHistogram threshold (10)                                     */
    int road;            /* 0 none, 1 road raster + walk, 2 + imageRoadMap, 3 road raster + walk + the
                            clean-up (sv_batch_road_clean; its mask: sv_loop_road_mask), 4 all of 3 + the
                            obstacle stage (sv_batch_road_hull; results: sv_batch_read_road_hull of the
                            batch sv_loop_batch returns), 5 all of 4 + the result image
                            (sv_batch_result; sv_batch_read_result), 6 all of 5 + the image tile
                            (sv_batch_tile; sv_batch_read_tile; H and W multiples of 4, checked by
                            sv_loop_create), 7 "video": all of 6 + the tiles' JPEG streams and their pack
                            (loop.py:49-54,82-89; sv_batch_jpeg, sv_batch_jpeg_pack; quality and slot:
                            sv_loop_jpeg; sv_batch_read_jpeg, sv_batch_read_jpeg_packed), inside the timeline's
                            "road" stage */
} sv_loop_params;
typedef struct sv_loop sv_loop;
/* carmask: the grey H x W mask of maskDisparity (functions.py:35, :169-172), NULL for none. */
int sv_loop_create(int device, const sv_loop_params* prm, const sv_camera* cam, const uint8_t* carmask,
                   sv_loop** out);
int sv_loop_destroy(sv_loop* L);
/* road = 3: the road stage of every batch also runs sanitiseRoadImage's clean-up (it counts inside the
 * timeline's "road" stage); the cleaned images and walks are on the batch sv_loop_batch returns
 * (sv_batch_read_road_clean). mask: the H x W road_threshold_mask for every slot, NULL = all ones (the default);
 * it applies to the batches whose road stage is enqueued after the call. */
int sv_loop_road_mask(sv_loop* L, const uint8_t* mask);
/* road = 7 (loop.py:49-54,82-89): the quality (1 .. 100; 75 unless set) and the slot capacity (0 = the default of
 * sv_batch_jpeg) of every batch's streams. SV_E_STATE after the first sv_loop_submit. sv_loop_params keeps its
 * layout. */
int sv_loop_jpeg(sv_loop* L, int quality, int64_t cap_per_frame);
/* The batch the next sv_loop_submit runs (waits on the host until its slot's previous batch is done): with
 * source 0 the caller uploads its frames (or runs sv_batch_sgbm on it) before submitting. */
int sv_loop_acquire(sv_loop* L, sv_batch** out);
/* Enqueue one batch (global frame ids first_frame_id..) through every stage; returns its sequence number. With a
 * carmask the host waits for nothing (the mask's step-2 points bound every frame's maskpoints count and size the
 * RANSAC launches); without one it waits for this batch's maskpoint counts, whose copy is enqueued on the slot's
 * stream behind the slot's earlier work (with two slots: batch k - 2's pipeline and road pass, and batch k - 1's
 * pre-pass). Batch k's own pipeline and road pass are enqueued by the next submit (or by sv_loop_wait / _batch /
 * _timeline). */
int sv_loop_submit(sv_loop* L, int64_t first_frame_id, int64_t* out_seq);
/* Wait for batch seq's last stage. sv_loop_batch: the batch holding seq's results (sv_batch_read_* work on it)
 * until batch seq + slots is acquired or submitted; it enqueues seq's pending stages and waits for them first. sv_loop_timeline: the start and end of each of the seven
 * stages (input, pre-pass, maskpoints, RANSAC draw, RANSAC evaluation, pipeline, road) in ms since the loop's
 * first submit, 14 doubles. */
int sv_loop_wait(sv_loop* L, int64_t seq);
int sv_loop_batch(sv_loop* L, int64_t seq, sv_batch** out, int64_t* first_frame_id);
int sv_loop_timeline(sv_loop* L, int64_t seq, double* out);

/* ---- verification helpers (device computes, host compares) -------------- */
/* Per-frame verification digests of the batch's current outputs (test and
 * bench support, not timed): which = 0 checks the K1 dense planes, 1 the
 * pipeline outputs. out = frames x 8 uint64: n_valid, n_kept, n_kept2,
 * disp_hash, hist_hash, pts_hash, bad, 0 — the definitions of
 * oracle/svx_oracle.c svo_frame_digest, recomputed on the device from the
 * outputs (kernels/digest.hip); `bad` counts outputs outside 1e-5 relative of
 * the fp64 reference values or inconsistent with the disparity. Synchronous. */
int sv_batch_digest(sv_batch* b, const sv_camera* cam, int which, uint64_t* out);


/* Hue bin of all 2^24 colours, index R<<16|G<<8|B (for exhaustive tests):
 * sv_hue_lut the exact device function (stage kernels, tiled pipeline);
 * sv_hue_lut_variant 0 the same, 1 the resident pipeline's fp32 path
 * (hue_bin_sel: rcp + rint, the exact path in the tie band). */
int sv_hue_lut(int device, int16_t* out_lut);
int sv_hue_lut_variant(int device, int variant, int16_t* out_lut);
/* Back-projection delta tables as computed on the device: dx[d][x], dy[d][y]. */
int sv_delta_tables(int device, int H, int W, const sv_camera* cam, int8_t* dx, int8_t* dy);
/* Regenerate one synthetic frame on the device and copy it back. */
int sv_synth_frame(int device, int64_t frame_id, int H, int W, uint8_t* disp, uint8_t* bgr);

/* ---- image I/O (host only): PNG ingest of the stereo pairs and masks ---------
 * Replaces cv2.imread at functions.py:29-34 (the masks) and :52-55 (loadImages)
 * for 8-bit non-interlaced PNGs; svx.io.imread inflates the IDAT stream (zlib) and
 * this undoes the scanline filters: `in` holds H rows of 1 filter byte + rowbytes,
 * `out` H x rowbytes; bpp = bytes a pixel (the filters' left neighbour). SV_E_ARG
 * on a filter type above 4 (a corrupt stream). No device work. */
int sv_png_unfilter(const uint8_t* in, int H, int rowbytes, int bpp, uint8_t* out);

/* ---- stage drop-ins: host-side row gathers (no device work) ---------------
 * The one-by-one drop-ins of stereovision.py:97-113 hold their points as an index
 * selection of projectDisparityTo3d's (N, ld) float64 rows (svx/points.py); these
 * gather the columns a stage uploads from rows[0..nrows); idx NULL = rows 0..n-1;
 * an index outside [0, nrows) is SV_E_ARG (nothing read).
 * sv_gather_rgb_u8: columns 3..5 (R, G, B) as uint8, n x 3; SV_E_ARG if a value is
 *   not an integer in [0, 255] (the colour stages' input check, svx/stages.py).
 *   Replaces the row conversion inside calculateColourHistogram /
 *   filterPointsByHistogram (functions.py:215-230).
 * sv_gather_f64: columns c0..c0+nc-1, n x nc (project3DPointsTo2DImagePoints'
 *   X, Y, Z, functions.py:201-209). */
int sv_gather_rgb_u8(const double* rows, int64_t nrows, int64_t ld, const int64_t* idx, int64_t n, uint8_t* out);
int sv_gather_f64(const double* rows, int64_t nrows, int64_t ld, const int64_t* idx, int64_t n, int c0, int nc,
                  double* out);

/* ---- multi-GPU: RCCL over xGMI ----------------------------- */
/* Frames shard by contiguous global-id ranges (one sv_batch per GPU); the only
 * device-data collective is the broadcast of the plane. Two drivers:
 *   one process per GPU: rank 0's sv_comm_unique_id, handed to every rank
 *     (svx/control.py), then sv_comm_init on each rank;
 *   one process, every GPU: sv_comm_init_all, then
 *     sv_multi_pipeline (or sv_comm_group_start / .._end around the per-device
 *     sv_comm_broadcast_plane_dev calls). */
typedef struct sv_comm sv_comm;
#define SV_UNIQUE_ID_BYTES 128
int sv_comm_unique_id(uint8_t* out_id /* SV_UNIQUE_ID_BYTES */);
int sv_comm_init(int nranks, int rank, const uint8_t* id, int device, sv_comm** out);
/* ncclCommInitAll over devices[0..n-1] (rank i on devices[i]); out[n]. */
int sv_comm_init_all(int n, const int* devices, sv_comm** out);
int sv_comm_destroy(sv_comm* c);
/* ncclGroupStart / ncclGroupEnd (one process issuing the collectives of several devices). */
int sv_comm_group_start(void);
int sv_comm_group_end(void);
/* Broadcast the plane coefficients from root over RCCL and back to the host
 * (synchronous; reporting and tests). */
int sv_comm_broadcast_plane(sv_comm* c, sv_plane* inout, int root);
/* Broadcast the plane from root into device memory, ordered on batch b's
 * stream (b on the comm's device): the root passes its host plane, the other
 * ranks NULL. *out_dplane = batch b's own device slot (3 doubles a, b, c;
 * one per batch, so batches in flight on other streams and the comm's
 * synchronous calls never overwrite it), valid for stream-ordered use on b's
 * stream (sv_batch_pipeline_dev) until b's next broadcast. No host
 * sync. Inside a group, the broadcast is enqueued at sv_comm_group_end: enqueue
 * the pipelines after it. */
int sv_comm_broadcast_plane_dev(sv_comm* c, sv_batch* b, const sv_plane* plane, int root, const double** out_dplane);
/* One process, n GPUs (SURVEY §8b sv_multi_pipeline): one grouped broadcast
 * of the root's plane to every device, then sv_batch_pipeline_dev on every
 * batches[i] (comms[i]'s device) with that device's copy of the plane.
 * Asynchronous unless sync != 0 (then every batch is synchronised). */
int sv_multi_pipeline(int n, sv_comm* const* comms, sv_batch* const* batches, const sv_camera* cam,
                      const sv_plane* plane, int root, double point_thr, int hist_thr, int sync);
/* Sum int64 counters over ranks (reporting only; host buffers, synchronous). */
int sv_comm_allreduce_i64(sv_comm* c, int64_t* inout, int n);

#ifdef __cplusplus
}
#endif
#endif /* SVX_H */
