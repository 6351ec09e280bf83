"""GPU: the validity of a batch's road chain (pipeline -> road_raster -> road_clean -> road_hull -> result) as one
ordered level. A table of calls is walked; after every call, every stage's run, `_ms` and `read_*`
either raises SvxError or succeeds as the table says, and what a read returns is the chain of the oracles
morph_numpy -> hull_numpy -> result_numpy on the raw road image, bit for bit."""
import types

import numpy as np
import pytest

import hull_numpy as hn
import morph_numpy as mn
import result_numpy as rn

pytestmark = pytest.mark.gpu

NONE, IMAGES, CLEANED, OBSTACLES, RESULT = range(5)
PLANE = (0.0, 0.0, 0.01)

# call -> (the level it needs, the level it leaves given the level before)
TABLE = {
    "pipeline":        (NONE, lambda lv: NONE),
    "pipeline_planes": (NONE, lambda lv: NONE),
    "road_raster":     (NONE, lambda lv: IMAGES),
    "road_mask":       (NONE, lambda lv: min(lv, IMAGES)),
    "road_mask_none":  (NONE, lambda lv: min(lv, IMAGES)),
    "road_clean":      (IMAGES, lambda lv: CLEANED),
    "road_hull":       (CLEANED, lambda lv: OBSTACLES),
    "result":          (OBSTACLES, lambda lv: RESULT),
}
# The walk: up the chain; each of road_mask(...), road_mask(None) and road_raster() alone after a result drops it
# to the road images; a stage run again drops what stands on it; the mask calls below the images change nothing;
# each pipeline entry starts over. (sv_batch_pipeline_dev, the third entry, needs a plane in device memory and
# shares the other two's implementation: it is not walked.)
WALK = ["pipeline", "road_mask_none", "road_raster", "road_clean", "road_hull", "result",
        "road_mask", "road_clean", "road_hull", "result",
        "road_mask_none", "road_clean", "road_hull", "result",
        "road_raster", "road_clean", "road_hull", "result",
        "road_hull", "result", "road_clean", "road_mask",
        "pipeline", "road_mask", "road_raster", "road_clean", "road_hull", "result",
        "pipeline_planes", "road_raster", "road_clean", "road_hull", "result"]


@pytest.fixture(scope="module")
def sv():
    import svx
    from svx import batch
    if svx.device_count() < 1:
        pytest.skip("no GPU")
    return types.SimpleNamespace(svx=svx, batch=batch)


def _frames(H, W):
    """Two disparities whose road images differ: every pixel, and a filled ring with steep and shallow sides."""
    ring = (hn.fill_polygon((H, W), hn.polygon_steep_shallow(H, W)) != 0).astype(np.uint8) * 200
    return [np.full((H, W), 200, np.uint8), ring]


class Chain:
    """The batch under test, the level the table predicts, and the oracles of the current points and mask."""

    def __init__(self, sv, b, disps, bgrs, mask):
        self.sv, self.b, self.disps, self.bgrs, self.mask = sv, b, disps, bgrs, mask
        self.level, self.cur_mask, self.kind, self.refs = NONE, None, None, {}
        self.hull_sizes = set()

    def call(self, name):
        b = self.b
        if name == "pipeline":
            b.pipeline(plane=PLANE, point_thr=1e9, hist_thr=2)
        elif name == "pipeline_planes":
            b.ransac(seed_base=3, trials=20, k=40)
            b.pipeline_planes(point_thr=1e9, hist_thr=2)
        elif name == "road_mask":
            b.road_mask(self.mask)
        elif name == "road_mask_none":
            b.road_mask(None)
        else:
            getattr(b, name)()
        if name.startswith("pipeline"):
            self.kind = name
        if name.startswith("road_mask"):
            self.cur_mask = self.mask if name == "road_mask" else None

    def climb(self, level):
        """Back to `level` by the stages' own runs (their outputs are functions of the points and the mask)."""
        for name in ("pipeline",) if level == NONE else ("road_raster", "road_clean", "road_hull", "result")[:level]:
            self.call(self.kind if name == "pipeline" else name)

    def ref(self, f):
        """(cleaned, obstacle stage, result image) of frame f for the current points and mask, computed once."""
        key = (self.kind, self.cur_mask is not None, f)
        if key not in self.refs:
            raw, walk = self.b.read_road(f, walk=True)
            assert np.array_equal(walk, mn.walk(raw)), key
            plane = PLANE
            if self.kind == "pipeline_planes":
                pl = self.b.read_frame_plane(f)
                plane = tuple(pl[:3]) if pl[3] >= 0 else None
            clean = mn.sanitise(raw, self.cur_mask)
            r = hn.obstacles(clean, self.disps[f], plane)
            pic = rn.result(self.bgrs[f], r["obstacles"], r["hull"], r["centre"], r["tip"], r["valid"])
            self.refs[key] = (clean, r, pic)
        return self.refs[key]

    def check(self, where):
        """Every stage's run, _ms and read_* at the predicted level."""
        b, lv, err = self.b, self.level, self.sv.svx.SvxError
        for need, ms, read in ((CLEANED, b.road_clean_ms, lambda: b.read_road_clean(0)),
                               (OBSTACLES, b.road_hull_ms, lambda: b.read_road_hull(0)),
                               (RESULT, b.result_ms, lambda: b.read_result(0))):
            for fn in (ms, read):
                if lv >= need:
                    fn()
                else:
                    with pytest.raises(err):
                        fn()
        for f in range(len(self.disps)):
            if lv >= IMAGES:
                clean, r, pic = self.ref(f)
            if lv >= CLEANED:
                img, walk = b.read_road_clean(f, walk=True)
                assert np.array_equal(img, clean) and np.array_equal(walk, mn.walk(clean)), (where, f)
            if lv >= OBSTACLES:
                got = b.read_road_hull(f)
                assert got["hull"].tolist() == r["hull"].tolist(), (where, f)
                assert np.array_equal(got["hull_mask"], r["hull_mask"]), (where, f)
                assert np.array_equal(got["obstacles"], r["obstacles"]), (where, f)
                assert (got["centre"], got["tip"], got["valid"]) == (r["centre"], r["tip"], r["valid"]), (where, f)
                self.hull_sizes.add(len(r["hull"]))
            if lv >= RESULT:
                assert np.array_equal(b.read_result(f), pic), (where, f)
        # the runs last: one that succeeds moves the chain, which then climbs back to where the walk stands
        for name in ("road_raster", "road_clean", "road_hull", "result"):
            if lv >= TABLE[name][0]:
                self.call(name)
                self.climb(lv)
            else:
                with pytest.raises(err):
                    self.call(name)


def _walk(sv, H, W, mode, bits):
    disps = _frames(H, W)
    rng = np.random.default_rng(H + W)
    bgrs = []
    for _ in disps:   # one hue (the pipeline's histogram filter keeps every point), the brightness random
        bgrs.append(np.repeat(rng.integers(0, 256, (H, W, 1)).astype(np.uint8), 3, axis=2))
    with sv.batch.Batch(len(disps), H, W, step=1, with_bgr=True, with_points=True) as b:
        b.pipeline_mode(mode)
        b.road_bits(bits)
        for f, d in enumerate(disps):
            b.upload(f, d, bgrs[f])
        c = Chain(sv, b, disps, bgrs, mn.random_mask(rng, H, W))
        for i, name in enumerate(WALK):
            need, after = TABLE[name]
            assert c.level >= need, (i, name)       # the walk itself only makes calls that succeed
            c.call(name)
            c.level = after(c.level)
            c.check((i, name))
        assert set(WALK) == set(TABLE)
    return c


def test_walk_40x70(sv):
    """A row stride of 72: the unpack-and-walk clean-up and the result's 8-pixel path."""
    c = _walk(sv, 40, 70, "auto", False)
    assert max(c.hull_sizes) >= 3, c.hull_sizes


def test_walk_72x1024_from_the_bitmap(sv):
    """The resident pipeline's road bitmap feeds the raster and the clean-up; the clean-up's bitmap road pass."""
    c = _walk(sv, 72, 1024, "resident", True)
    assert max(c.hull_sizes) >= 3, c.hull_sizes
