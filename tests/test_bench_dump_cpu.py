"""bench.py --dump-outputs on the CPU: the files a dump holds, their rows in list order, the fixed sample that keeps a large
scene under 64 MB, and the options that keep a plain run lean."""
import os
import sys

import numpy as np

import bench


def dump(buf, d, **kw):
    bench.dump_outputs(str(d), buf, **kw)
    return {n: np.load(os.path.join(str(d), n + ".npy")) for n in ("particles", "beams", "counts")}


def test_small_scene_is_written_whole_in_list_order(sb, tmp_path):
    buf = sb.scenes.lattice_buffers(12, 9, d=30.0, origin=(1000.0, 1000.0), jitter=1.0, layout=2)
    P, B, maxP = buf.particle_count, buf.beam_count, buf.max_particles
    perm = np.random.default_rng(5).permutation(P)          # a mapping that is not the identity
    buf.mapping[:P] = buf.mapping[:P][perm]
    got = dump(buf, tmp_path)
    assert sorted(os.listdir(str(tmp_path))) == ["beams.npy", "counts.npy", "particles.npy"]
    assert got["counts"].dtype == np.float64 and got["counts"].tolist() == [P, B]
    assert got["particles"].dtype == np.float32 and np.array_equal(got["particles"], buf.particles[buf.mapping[:P].astype(np.int64)])
    rec = buf.beams[buf.mapping[maxP:maxP + B].astype(np.int64)]
    assert got["beams"].dtype == np.float32 and got["beams"].shape == (B, 11)
    assert np.array_equal(got["beams"][:, 0], rec["a"]) and np.array_equal(got["beams"][:, 1], rec["b"])
    for i, f in enumerate(sb.layout.BEAM_FLOATS):
        assert np.array_equal(got["beams"][:, 2 + i], rec[f]), f


def test_owned_rows_only(sb, tmp_path):
    buf = sb.scenes.lattice_buffers(12, 9, layout=2)
    got = dump(buf, tmp_path, particles=[3, 1, 7], beams=[0, 5])
    assert got["counts"].tolist() == [3, 2]
    assert np.array_equal(got["particles"], buf.particles[[3, 1, 7]]) and got["beams"].shape == (2, 11)


def test_default_scene_fits_64_mb_with_the_same_sample_every_time(sb, tmp_path):
    """BASELINE config 2 (1 M particles, 3 M beams): every particle, a seeded sample of the beams, under 64 MB, twice the same."""
    buf = sb.scenes.lattice_buffers(1000, 1000, d=30.0, origin=(1000.0, 1000.0), jitter=1.0, layout=2)
    a = dump(buf, tmp_path / "a")
    total = sum(os.path.getsize(str(tmp_path / "a" / n)) for n in os.listdir(str(tmp_path / "a")))
    assert total <= 64_000_000
    assert a["particles"].shape == (1_000_000, 6) and a["counts"].tolist() == [1_000_000, 2_996_001]
    n = a["beams"].shape[0]
    assert 500_000 < n < 2_996_001
    idx = bench.dump_sample(2_996_001, 44, bench.DUMP_BEAM_BYTES, 2)
    assert idx.size == n and (np.diff(idx) > 0).all()
    assert np.array_equal(a["beams"][:, 2], buf.beams["length"][idx])
    b = dump(buf, tmp_path / "b")
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


def test_plain_run_options(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "3"])
    a = bench.parse()
    assert a.steps == 7 and a.warmup == 3 and not a.full and a.dump_outputs is None
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "out"
