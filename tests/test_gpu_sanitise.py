"""GPU: sanitiseRoadImage's clean-up (functions.py:346-366) — kernels/morph.hip behind sv_sanitise_road, the batch
path (Batch.road_clean), the frame loop (road="clean") and the drop-in — bit for bit against the numpy oracle
tests/morph_numpy.py (pinned by tests/test_morph_cpu.py), image and walk."""
import os
import types

import numpy as np
import pytest

import morph_numpy as mn
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

MASK_PNG = os.path.join(GOLDEN, "masks", "road_threshold_mask.png")


@pytest.fixture(scope="module")
def sv():
    import svx
    from svx import batch, dropin, io, loop
    if svx.device_count() < 1:
        pytest.skip("no GPU")
    return types.SimpleNamespace(svx=svx, batch=batch, dropin=dropin, io=io, loop=loop)


@pytest.fixture(scope="module")
def road_mask(sv):
    m = sv.io.imread(MASK_PNG, sv.io.IMREAD_GRAYSCALE)
    assert m is not None and m.shape == (544, 1024) and set(np.unique(m).tolist()) == {0, 128, 255}
    return m


def check(sv, img, mask=None):
    """sv_sanitise_road(img, mask) == the oracle, image and walk; returns the oracle's image."""
    ref = mn.sanitise(img, mask)
    got, pts = sv.dropin.sanitise_road(img, mask)
    assert got.dtype == np.uint8 and got.shape == img.shape and pts.dtype == np.int32
    bad = np.argwhere(got != ref)
    assert len(bad) == 0, (img.shape, len(bad), bad[:5].tolist())
    assert np.array_equal(pts, mn.walk(ref)), img.shape
    return ref


# ---- the closed-form cases of tests/test_morph_cpu.py, 40 x 64, all-ones mask ---------------------------------
def _img(*blocks, shape=(40, 64)):
    a = np.zeros(shape, np.uint8)
    for y0, y1, x0, x1 in blocks:
        a[y0:y1, x0:x1] = 255
    return a


HAND = {
    "all_set": (np.full((40, 64), 255, np.uint8), 40 * 64),
    "empty": (np.zeros((40, 64), np.uint8), 0),
    "one_pixel": (_img((20, 21, 30, 31)), 0),
    "block_17x17": (_img((10, 27, 20, 37)), 1),
    "block_16x17": (_img((10, 26, 20, 37)), 0),
    "corner_25x25": (_img((0, 25, 0, 25)), 289),
    "bars_8_apart": (_img((5, 35, 10, 27), (5, 35, 35, 52)), 364),
    "bars_9_apart": (_img((5, 35, 10, 27), (5, 35, 36, 53)), 28),
    "near_every_edge": (_img((2, 38, 4, 60)), 40 * 64),
}


@pytest.mark.parametrize("name", list(HAND))
def test_hand_cases(sv, name):
    img, count = HAND[name]
    ref = check(sv, img)
    assert int((ref != 0).sum()) == count
    check(sv, img, np.full(img.shape, 255, np.uint8))   # an all-ones mask is no mask
    if name == "block_17x17":
        got, pts = sv.dropin.sanitise_road(img)
        assert pts.tolist() == [[28, 18]] and got[18, 28] == 255


def test_non_zero_values_are_set_and_mask_128_keeps(sv):
    img = np.zeros((40, 64), np.uint8)
    img[5:35, 10:52] = 1            # any non-zero value is a set pixel
    m = np.zeros((40, 64), np.uint8)
    m[:, :30] = 128
    ref = check(sv, img, m)
    assert ref.any() and set(np.unique(ref).tolist()) == {0, 255}


# ---- seeded rectangles + noise, a {0, 128, 255} mask ----------------------------------------------------------
# Anchored rectangles straddle what the kernel treats specially: word boundaries (x = 32 k), the frame's first
# and last row and column, and the band edges of the one-workgroup-per-band layout (544 x 1024: bands of 136
# rows; 17 x 4096: 9 rows; 390 x 889: 130 rows — morph_band_rows in kernels/morph.hip).
def _case(H, W, seed, with_mask=True):
    rng = np.random.default_rng(1000 * seed + H + W)
    anchors = [(-6, 20), (H - 12, W // 2 - 7), (H // 3, -9), (H // 2, W - 21), (3, 32 * (W // 64) - 9)]
    for edge in (9, 130, 136, 260, 272, 408):
        if edge < H:
            anchors += [(edge - 11, int(rng.integers(0, max(W - 40, 1)))), (edge - 2, int(rng.integers(0, max(W - 40, 1))))]
    if W < 40:     # narrower than two rectangles: a block that touches the border survives the 17 x 17 erosion
        img = mn.rectangles(rng, H, W, 0, noise=0.01)
        img[:, : (2 * W) // 3] = 255
        img[H // 2, W // 3] = 0
    elif H < 40:   # lower than 24 rows: only rectangles that reach the top or the bottom row survive
        img = mn.rectangles(rng, H, W, max(4, W // 60), hmin=10, hmax=20,
                            anchors=[(-4, 20), (H - 12, W // 2 - 7), (2, W - 21), (3, 32 * (W // 64) - 9)])
    elif H * W < 10000:
        img = mn.rectangles(rng, H, W, 2, hmin=18, hmax=30, wmin=18, wmax=40, anchors=[(-6, 20), (H - 12, W // 2 - 7)])
    else:
        img = mn.rectangles(rng, H, W, max(4, H * W // 2500), anchors=anchors)
    return img, (mn.random_mask(rng, H, W) if with_mask else None)


SHAPES = [(40, 64), (20, 33), (61, 889), (17, 4096)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_random_rectangles(sv, shape):
    """W % 32 != 0 (pad bits), H < 24 (the whole frame is halo), one word column of 128 (17 x 4096, two bands)."""
    H, W = shape
    for seed in (0, 1):
        img, mask = _case(H, W, seed)
        ref = check(sv, img, mask)
        d = float((ref != 0).mean())
        assert 0.005 < d < 0.6, (shape, seed, d)   # neither empty nor full
        check(sv, img)


def test_544x1024_with_the_reference_mask(sv, road_mask):
    """The reference's shape and its road_threshold_mask.png (0 / 128 / 255); four bands of 136 rows; image and
    walk come from the bitmap road pass."""
    img, _ = _case(544, 1024, 0, with_mask=False)
    ref = check(sv, img, road_mask)
    d = float((ref != 0).mean())
    assert 0.005 < d < 0.6, d
    assert (ref[road_mask == 0] == 0).all() and ref[road_mask == 128].any()


def test_arguments(sv):
    with pytest.raises(sv.svx.SvxError):
        sv.dropin.sanitise_road(np.zeros((4, 1), np.uint8))          # W < 2
    with pytest.raises(sv.svx.SvxError):
        sv.dropin.sanitise_road(np.zeros((2, 4097), np.uint8))       # W > 4096
    with pytest.raises(ValueError):
        sv.dropin.sanitise_road(np.zeros((4, 8), np.uint8), np.zeros((4, 9), np.uint8))
    with pytest.raises(TypeError):
        sv.dropin.sanitise_road(np.zeros((4, 8), np.float32))


# ---- the batch path --------------------------------------------------------------------------------------------
def _batch_clean(sv, H, W, step, mode, bits, mask, frames=5, first=20):
    with sv.batch.Batch(frames, H, W, step=step, with_bgr=True, with_points=True) as b:
        b.pipeline_mode(mode)
        b.road_bits(bits)
        if W % 8 == 0:
            b.synth(first)
        else:
            import oracle
            for f in range(frames):
                b.upload(f, *oracle.synth_frame(first + f, H, W))
        b.pipeline()
        with pytest.raises(sv.svx.SvxError):   # no current road pass yet
            b.road_clean()
        b.road_raster()
        raw = [b.read_road(f, walk=True) for f in range(frames)]
        b.road_mask(mask)
        b.road_clean()
        for f in range(frames):
            rimg, rwalk = raw[f]
            ref = mn.sanitise(rimg, mask)
            img, walk = b.read_road_clean(f, walk=True)
            assert np.array_equal(img, ref), (f, int((img != ref).sum()))
            assert np.array_equal(walk, mn.walk(ref)), f
            assert np.array_equal(b.read_road_clean(f), ref)
            img2, walk2 = b.read_road(f, walk=True)    # the raw image and walk are left alone
            assert np.array_equal(img2, rimg) and np.array_equal(walk2, rwalk), f
            assert rimg.any() and 0.005 < (ref != 0).mean() < 0.9, (f, (ref != 0).mean())
        assert any(not np.array_equal(raw[0][0], raw[f][0]) for f in range(1, frames))
        b.road_mask(None)                               # back to all ones
        b.road_clean()
        assert np.array_equal(b.read_road_clean(frames - 1), mn.sanitise(raw[frames - 1][0]))
        b.pipeline()                                    # new points: the road pass is no longer current
        with pytest.raises(sv.svx.SvxError):
            b.road_clean()
        with pytest.raises(sv.svx.SvxError):
            b.read_road_clean(0)


def test_batch_from_the_pipeline_bitmap(sv, road_mask):
    """5 frames of 544 x 1024 at step 1, the resident pipeline writing the road bitmap: the clean-up reads it."""
    _batch_clean(sv, 544, 1024, 1, "resident", True, road_mask)


def test_batch_step2_packs_the_road_images(sv, road_mask):
    """Step 2: no bitmap, the road images (from the points) are packed first."""
    _batch_clean(sv, 544, 1024, 2, "auto", True, road_mask)


def test_batch_390x889(sv, road_mask):
    """crop_disparity=True frames: W % 32 != 0, row stride 896; pack, unpack and the non-zero walk."""
    _batch_clean(sv, 390, 889, 1, "auto", False, np.ascontiguousarray(road_mask[:390, :889]))


def test_frames_do_not_leak_into_each_other(sv):
    """An all-set road image between empty ones, and an empty one between all-set ones: rows above or below a
    frame are "outside" (clear for the dilations, set for the erosions), never the neighbouring frame's rows. The
    road images come from the pipeline (every grid point kept / no disparity at all); both ways into the clean-up
    (the pipeline's bitmap, the packed road image)."""
    H, W = 72, 1024
    full = np.full((H, W), 200, np.uint8)
    zero = np.zeros((H, W), np.uint8)
    bgr = np.full((H, W, 3), 90, np.uint8)
    order = [full, zero, full, zero, zero, full]
    for mode, bits in (("resident", True), ("tiled", False)):
        with sv.batch.Batch(len(order), H, W, step=1, with_bgr=True, with_points=True) as b:
            b.pipeline_mode(mode)
            b.road_bits(bits)
            for f, d in enumerate(order):
                b.upload(f, d, bgr)
            b.pipeline(plane=(0.0, 0.0, 0.01), point_thr=1e9, hist_thr=2)
            b.road_raster()
            b.road_clean()
            for f, d in enumerate(order):
                raw = b.read_road(f)
                ref = mn.sanitise(raw)
                got = b.read_road_clean(f)
                if d is zero:
                    assert not raw.any() and not got.any(), (mode, f)
                else:
                    assert (raw != 0).mean() > 0.5 and (ref != 0).mean() > 0.9, (mode, f)
                assert np.array_equal(got, ref), (mode, f, int((got != ref).sum()))
    # the host entry, frame by frame: the same answers
    assert sv.dropin.sanitise_road(np.full((H, W), 255, np.uint8))[0].all()
    assert not sv.dropin.sanitise_road(zero)[0].any()


# ---- the frame loop ---------------------------------------------------------------------------------------------
def test_frame_loop_road_clean(sv, road_mask):
    from svx.loop import STAGES, FrameLoop
    frames = 4
    raws, kept = {}, []
    with FrameLoop(frames, slots=2, source="synth", road="clean", road_mask=road_mask) as loop:
        def verify(seq):
            b, first = loop.batch(seq)
            for f in range(frames):
                rimg, rwalk = b.read_road(f, walk=True)
                raws[first + f] = (rimg, rwalk)
                ref = mn.sanitise(rimg, road_mask)
                img, walk = b.read_road_clean(f, walk=True)
                assert rimg.any(), (seq, f)
                assert np.array_equal(img, ref) and np.array_equal(walk, mn.walk(ref)), (seq, f)
                kept.append(int((ref != 0).sum()))
        s0 = loop.submit(0)
        s1 = loop.submit(frames)
        verify(s0)
        s2 = loop.submit(2 * frames)
        verify(s1)
        verify(s2)
        assert len(kept) == 3 * frames and min(kept) > 0, kept   # the clean-up left something of every frame
        tl = loop.timeline(s2)
        assert tuple(tl) == STAGES and len(tl) == 7
        assert tl["pipeline"][1] - 1e-3 <= tl["road"][0] <= tl["road"][1]
    with FrameLoop(frames, slots=2, source="synth", road="walk") as loop:   # the same frames without the clean-up
        seqs = [loop.submit(0), loop.submit(frames)]
        for seq in seqs:
            b, first = loop.batch(seq)
            for f in range(frames):
                rimg, rwalk = b.read_road(f, walk=True)
                assert np.array_equal(rimg, raws[first + f][0]) and np.array_equal(rwalk, raws[first + f][1])
            with pytest.raises(sv.svx.SvxError):
                b.read_road_clean(0)


# ---- the drop-in ------------------------------------------------------------------------------------------------
def test_dropin_sanitise_road_image(sv, road_mask):
    dropin = sv.dropin

    def orig(img, size):
        return "original"
    m = types.SimpleNamespace(road_threshold_mask=road_mask, sanitiseRoadImage=orig)
    assert dropin.MORPHOLOGY == ("sanitiseRoadImage",) and "sanitiseRoadImage" not in dropin.PATCHED
    dropin.install(m)
    try:
        assert m.sanitiseRoadImage is orig          # not without the flag
    finally:
        dropin.uninstall()
    img, _ = _case(544, 1024, 1, with_mask=False)
    dropin.install(m, morphology=True)
    try:
        assert m.sanitiseRoadImage is dropin.sanitiseRoadImage
        before = img.copy()
        out, pts = m.sanitiseRoadImage(img, (544, 1024))
        assert np.array_equal(img, before)
        ref = mn.sanitise(img, road_mask)
        want = []
        for i in range(544):                        # functions.py:359-365, literally
            row = ref[i]
            for j in range(1024):
                if row[j] != 0:
                    want.append([j, i])
        want = np.matrix(want)
        assert len(want) > 1000
        assert np.array_equal(out, ref) and out.dtype == np.uint8
        assert type(pts) is np.matrix and pts.dtype == want.dtype == np.int64 and pts.shape == want.shape
        assert np.array_equal(pts, want)
        # a smaller size restricts the walk, not the image
        out2, pts2 = m.sanitiseRoadImage(img, (300, 500))
        sel = np.asarray(want)
        sel = sel[(sel[:, 1] < 300) & (sel[:, 0] < 500)]
        assert np.array_equal(out2, ref) and 0 < len(sel) < len(want) and np.array_equal(pts2, np.matrix(sel))
        # no points: np.matrix([]) as the reference's np.matrix(list) gives it
        out3, pts3 = m.sanitiseRoadImage(np.zeros((544, 1024), np.uint8), (544, 1024))
        empty = np.matrix([])
        assert not out3.any() and type(pts3) is np.matrix and pts3.shape == empty.shape == (1, 0)
        assert pts3.dtype == empty.dtype == np.float64
    finally:
        dropin.uninstall()
    assert m.sanitiseRoadImage is orig
    with pytest.raises(RuntimeError):               # no installed module: no road_threshold_mask
        dropin.sanitiseRoadImage(img, (544, 1024))
