"""bench.py --dump-outputs and --full.

A plain run times its steps and prints the result line; `--dump-outputs DIR`
adds the last timed step's outputs as DIR/<name>.npy (float64 / float32, a
fixed sample of the larger ones), and only `--full` runs the CPU baseline and
the checks against the oracle.  The GPU test runs C1 (160 MB) once and
compares the dumped tables with the oracle's results for the same arena."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def run_bench(*argv, timeout=300):
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=timeout)
    return p.returncode, [ln for ln in p.stdout.splitlines() if ln.startswith("{")], p.stderr


def test_dump_sample_is_fixed_and_bounded():
    assert np.array_equal(bench.dump_sample(5), np.arange(5))
    assert np.array_equal(bench.dump_sample(bench.DUMP_BATCHES), np.arange(bench.DUMP_BATCHES))
    n = 1 << 20
    a, b = bench.dump_sample(n), bench.dump_sample(n)
    assert np.array_equal(a, b)
    assert bench.DUMP_BATCHES - 2 <= len(a) <= bench.DUMP_BATCHES
    assert a[0] == 0 and a[-1] == n - 1 and (np.diff(a) > 0).all()


def test_fields_f64_keeps_field_order_and_values():
    from redpanda_amd import abi

    r = np.zeros(3, dtype=abi.RESULT_DTYPE)
    r["verdict"] = (0, -1, 7)
    r["crc"] = (0, 0xFFFFFFFF, 5)
    r["base_offset"] = (1 << 52, -3, 9)
    t = bench.fields_f64(r)
    names = list(abi.RESULT_DTYPE.names)
    assert t.dtype == np.float64 and t.shape == (3, len(names))
    for f in ("verdict", "crc", "base_offset"):
        assert t[:, names.index(f)].tolist() == [float(v) for v in r[f]]
    assert bench.fields_f64(r[:0]).shape == (0, len(names))


def test_dump_outputs_writes_float_arrays_within_the_limit(tmp_path):
    arrays = {"a": np.arange(6, dtype=np.float64).reshape(2, 3), "b": np.ones(4, dtype=np.float32)}
    bench.dump_outputs(str(tmp_path / "d"), arrays)
    assert sorted(os.listdir(tmp_path / "d")) == ["a.npy", "b.npy"]
    for k, v in arrays.items():
        got = np.load(tmp_path / "d" / (k + ".npy"))
        assert got.dtype == v.dtype and np.array_equal(got, v)
    big = {"x": np.lib.stride_tricks.as_strided(np.zeros(1), (bench.DUMP_LIMIT // 8 + 1,), (0,))}
    with pytest.raises(SystemExit):
        bench.dump_outputs(str(tmp_path / "e"), big)
    assert not (tmp_path / "e").exists()


def test_full_check_is_behind_full():
    rc, lines, err = run_bench("--full-check", "1", "--dry-run")
    assert rc == 2 and not lines and "--full" in err
    rc, lines, err = run_bench("--steps", "0", "--dry-run")
    assert rc == 2 and not lines


@pytest.mark.gpu
def test_plain_run_dumps_what_the_oracle_computes(built, tmp_path):
    import oracle.oracle as orc
    from redpanda_amd import abi, engine, shard

    n, steps = 10_000, 2  # C1 at its full size: more index entries than the dump's index table holds
    out_dir = tmp_path / "dump"
    rc, lines, err = run_bench("--gpus", "1", "--config", "c1", "--batches", str(n), "--steps", str(steps),
                               "--warmup", "1", "--dump-outputs", str(out_dir))
    assert rc == 0, err[-3000:]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == steps and line["ms_per_step"] > 0 and line["unit"] == "GB/s"
    # a plain run: no CPU baseline, no comparison with the oracle
    assert line["cpu_baseline"] is None and "gpu_matches_oracle_on_sample" not in line and "full_check" not in line

    got = {f[:-4]: np.load(out_dir / f) for f in sorted(os.listdir(out_dir))}
    assert set(got) == {"summaries", "batch_ids", "results", "index_used", "index", "index_batches"}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20

    # the same arena as the run's (bench.main: seed, spec, first batch 0)
    cfg = bench.CONFIGS["c1"]
    spec = engine.make_spec(seed=0x5EED0001, partitions=cfg["partitions"], **cfg["spec"])
    data, descs = engine.build_arena(spec, n)
    wres, widx, wused = orc.validate_arena(data, descs)
    assert np.array_equal(got["batch_ids"], np.arange(n))
    names = list(abi.RESULT_DTYPE.names)
    for f in names:
        if f != "index_first":  # the two sides may lay the index slices out differently
            assert np.array_equal(got["results"][:, names.index(f)], wres[f].astype(np.float64)), f
    assert int(got["index_used"][0]) == int(wused)
    k = int(got["index_batches"][0])
    # 16 records per batch: the index table ends before the batch that would not fit whole
    assert k == bench.DUMP_INDEX_ENTRIES // 16 < n
    want_rows = np.concatenate([widx[int(a):int(a) + int(c)]
                                for a, c in zip(wres["index_first"][:k], wres["index_count"][:k])])
    assert np.array_equal(got["index"], bench.fields_f64(want_rows))
    assert np.array_equal(got["summaries"],
                          shard.summaries_numpy(wres, descs["partition"], 0, 1).astype(np.float64))
