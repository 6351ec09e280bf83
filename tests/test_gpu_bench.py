"""bench.py's N-GPU drivers on the one-GPU box (the driver's 8-GPU run must not
be their first execution): the in-process bench in "multi" mode (one process,
ncclCommInitAll over devices [0], the grouped plane broadcast of
sv_multi_pipeline inside the timed steps) and in "ranks" mode (torchrun's
RANK / WORLD_SIZE / LOCAL_RANK at world size 1: the TCP control plane, an RCCL
communicator per rank, sv_comm_broadcast_plane_dev + sv_batch_pipeline_dev).
Small settings; every frame's K1 and pipeline digests are checked by the bench
itself against tests/golden/frame_digests.npz (parity.pass)."""
import pytest

pytestmark = pytest.mark.gpu

ARGS = ["--gpus", "1", "--frames", "512", "--steps", "2", "--warmup", "1", "--ramp-ms", "20",
        "--full", "--no-extras", "--no-cpu", "--no-latency"]


def _check(out):
    assert out["n_gpus"] == 1
    assert out["parity"]["pass"], out["parity"]
    assert out["parity"]["k1"]["frames_checked"] == 512
    assert out["parity"]["pipeline"]["frames_checked"] == 512
    assert out["value"] > 0 and out["pipeline"]["value"] > 0


def test_bench_multi_driver(monkeypatch):
    import bench
    from svx import dist
    calls = []
    orig = dist.MultiComm.pipeline

    def counting(self, *a, **k):
        calls.append(len(a[0]))
        return orig(self, *a, **k)

    monkeypatch.setattr(dist.MultiComm, "pipeline", counting)
    for v in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(v, raising=False)
    out = bench.main(ARGS + ["--driver", "multi"])
    _check(out)
    assert "ncclCommInitAll" in out["config"]["parallelism"]
    assert out["pipeline"]["plane_broadcast"].startswith("RCCL grouped")
    assert len(calls) >= 3 and set(calls) == {1}   # warm-up + 2 timed steps, one batch each


def test_bench_ranks_driver(monkeypatch):
    import bench
    from svx import dist
    calls = []
    orig = dist.RcclComm.broadcast_plane_dev

    def counting(self, *a, **k):
        calls.append(1)
        return orig(self, *a, **k)

    monkeypatch.setattr(dist.RcclComm, "broadcast_plane_dev", counting)
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setenv("WORLD_SIZE", "1")
    monkeypatch.setenv("LOCAL_RANK", "0")
    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
    monkeypatch.setenv("MASTER_PORT", "29531")
    out = bench.main(ARGS)
    _check(out)
    assert "torchrun" in out["config"]["parallelism"]
    assert out["pipeline"]["plane_broadcast"].startswith("RCCL ncclBroadcast")
    assert len(calls) >= 3


def test_bench_plain_run_and_dump_outputs(monkeypatch, tmp_path):
    """A plain run (no --full) times the headline alone: no pipeline, parity, latency, extras or CPU records in its
    line. --dump-outputs writes the last timed step's K1 planes for the fixed frame sample (16 frames of 6.7 MB do
    not fit the 64 MB limit, so the seeded draw is taken): the same files from two runs, each frame's planes the
    oracle's projection of that frame within fp32 rounding."""
    import os

    import numpy as np

    import bench
    import oracle
    for v in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(v, raising=False)
    args = ["--gpus", "1", "--frames", "16", "--steps", "3", "--warmup", "1", "--ramp-ms", "20"]
    outs = [bench.main(args + ["--dump-outputs", str(tmp_path / d)]) for d in ("a", "b")]
    for out in outs:
        assert out["steps"] == 3 and out["value"] > 0 and out["ms_per_step"] > 0
        for k in ("metric", "unit", "higher_is_better", "dtype", "roofline"):
            assert k in out, k
        for k in ("pipeline", "parity", "latency_1frame_us", "extras", "cpu_baseline"):
            assert k not in out, k
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    ids = bench.dump_frames(16, 3 * 4 * 543 * 1024)
    assert names == [f"k1_xyz_frame{f:07d}.npy" for f in ids] and 1 < len(ids) < 16
    total = 0
    for f, name in zip(ids, names):
        a = np.load(tmp_path / "a" / name)
        assert a.dtype == np.float32 and a.shape == (3, 543, 1024)
        assert np.array_equal(a.view(np.uint32), np.load(tmp_path / "b" / name).view(np.uint32))
        total += a.nbytes
        disp, _ = oracle.synth_frame(f)
        ref = oracle.project_dense(disp, 1)
        assert np.array_equal(a[2] == 0, ref[2] == 0)
        for got, want in zip(a, ref):
            np.testing.assert_allclose(got, want, rtol=1e-5, atol=0)
    assert total <= bench.DUMP_LIMIT


def test_bench_strong_scaling_flag(monkeypatch):
    """--global-frames (SURVEY §8d config 5's strong scaling): the given frames in all, split over the GPUs;
    at one GPU the whole batch, reported as strong scaling, with every frame's digests checked."""
    import bench
    for v in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(v, raising=False)
    out = bench.main([a for a in ARGS if a not in ("--frames", "512")] + ["--global-frames", "512"])
    _check(out)
    assert out["scaling"] == "strong" and out["config"]["global_frames"] == 512


def test_bench_ranks_without_rccl(monkeypatch):
    """"ranks" mode when the RCCL communicator cannot be made (every rank fails alike, a collective init): the
    bench still measures, with rank 0's plane over the host control plane, and says so in its line."""
    import bench
    from svx import SvxError, dist

    def fail(self, *a, **k):
        raise SvxError("simulated ncclCommInitRank failure")

    monkeypatch.setattr(dist.RcclComm, "__init__", fail)
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setenv("WORLD_SIZE", "1")
    monkeypatch.setenv("LOCAL_RANK", "0")
    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
    monkeypatch.setenv("MASTER_PORT", "29532")
    out = bench.main(ARGS)
    _check(out)
    assert out["pipeline"]["plane_broadcast"].startswith("RCCL communicator unavailable")
