"""bench.py's host-side pieces that need no GPU: the per-env action streams (drawn as the launches consume them, the same actions as
drawing each stream whole) and the --dump-outputs writer (float32 / float64 files, a seeded sample of the envs above the size cap)."""
import os

import numpy as np


def test_action_streams_equal_the_streams_drawn_whole():
    import bench
    E, n = 7, 300
    whole = np.stack([np.random.RandomState(2000 + 3 + e).uniform(-1, 1, size=(n, 4)) for e in range(E)])
    s = bench.ActionStreams(3, E, n0=5)
    rs = np.random.RandomState(1)
    cnt = np.zeros(E, dtype=np.int64)
    for k in range(30):                                   # uneven consumption, as in the time-sliced launches
        slots = int(rs.randint(1, 12))
        if k == 10:
            s.reserve(int(cnt.max()) + 40)
        tbl = s.table(cnt, slots)
        assert tbl.shape == (slots, E, 4)
        for e in range(E):
            assert np.array_equal(tbl[:, e], whole[e, cnt[e]:cnt[e] + slots])
        cnt += rs.randint(0, slots + 1, size=E)


def test_dump_arrays_types_and_sample(tmp_path, monkeypatch):
    import bench
    E = 40
    obs = np.arange(E * 6, dtype=np.float32).reshape(E, 6)
    rew = np.linspace(0, 1, 3 * E).reshape(3, E)
    done = np.zeros((3, E), dtype=bool)
    done[1, ::3] = True
    executed = np.arange(3 * E, dtype=np.int64).reshape(3, E)
    arrays = {"obs": (obs, 0), "rew": (rew, 1), "done": (done, 1), "executed": (executed, 1)}
    full = tmp_path / "full"
    bench.dump_arrays(str(full), arrays, E)
    got = {f[:-4]: np.load(str(full / f)) for f in os.listdir(str(full))}
    assert set(got) == {"obs", "rew", "done", "executed", "env_index"}
    assert got["obs"].dtype == np.float32 and np.array_equal(got["obs"], obs)
    for k in ("rew", "done", "executed", "env_index"):
        assert got[k].dtype == np.float64, k
    assert np.array_equal(got["done"], done) and np.array_equal(got["executed"], executed) and np.array_equal(got["env_index"], np.arange(E))
    # above the cap: the same seeded sample of envs in every file, and the files within the cap
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 1024 * 6 + 1500)
    for d in ("a", "b"):
        bench.dump_arrays(str(tmp_path / d), arrays, E)
    a = {f[:-4]: np.load(str(tmp_path / "a" / f)) for f in os.listdir(str(tmp_path / "a"))}
    b = {f[:-4]: np.load(str(tmp_path / "b" / f)) for f in os.listdir(str(tmp_path / "b"))}
    keep = a["env_index"].astype(np.int64)
    assert 0 < len(keep) < E and np.all(np.diff(keep) > 0)
    assert np.array_equal(a["obs"], obs[keep]) and np.array_equal(a["rew"], rew[:, keep]) and np.array_equal(a["done"], done[:, keep])
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert sum(os.path.getsize(str(tmp_path / "a" / f)) for f in os.listdir(str(tmp_path / "a"))) <= bench.DUMP_MAX_BYTES
