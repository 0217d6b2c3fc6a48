"""bench.py prints ONE JSON line with the contract's keys (run on a reduced batch so that it takes seconds): a plain run the
headline alone, --full the other legs too; --dump-outputs writes the last timed step's rows."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_line_has_the_contract_fields():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--reads-per-gpu",
                        str(2 ** 21), "--cpu-seconds", "1", "--e2e-pairs", str(2 ** 20), "--full"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-800:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
              "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["unit"] == "reads/s" and d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["higher_is_better"] is True
    assert d["scaling"] == "weak" and d["vs_baseline"] is None and d["data"] == "synthetic" and "workload" in d["config"]
    assert abs(d["value"] - d["config"]["reads_per_gpu"] / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-3
    rf = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in rf, k
    assert rf["bound"] in ("hbm", "mfma") and rf["unit"] == "GB/s" and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-4
    assert rf["kernel"] in rf["kernel_ms"] and rf["kernel_ms"][rf["kernel"]] == max(rf["kernel_ms"].values())
    assert d["config"]["last_step_equals_synchronous_pass"] is True
    e2e = d["end_to_end"]
    assert e2e["reads"] == 2 ** 21 and e2e["call_rc"] == 0 and e2e["merge_rc"] == 0 and e2e["check"]["ok"] and e2e["check"]["treads_checked"] > 1000
    assert e2e["value"] > 1e6 and e2e["reads_per_s_extract_plus_call"] > 1e5 and e2e["runs"][0]["device_mem_GB"] > 0
    cb = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in cb, k
    assert cb["kind"] in ("reference", "port") and cb["cores"] == 1 and cb["value"] > 1e5


def _plain(out_dir):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "2", "--reads-per-gpu", str(2 ** 21),
                        "--dump-outputs", str(out_dir)], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-800:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_is_the_headline_and_dumps_the_same_rows_twice(tmp_path):
    d = _plain(tmp_path / "a")
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d, k
    assert d["unit"] == "reads/s" and d["higher_is_better"] is True and d["steps"] == 4 and d["warmup"] == 2
    assert abs(d["value"] - d["config"]["reads_per_gpu"] / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-3
    for k in ("roofline", "cpu_baseline", "end_to_end", "build"):           # the legs of --full
        assert k not in d, k
    a = {os.path.basename(f): np.load(f) for f in glob.glob(str(tmp_path / "a" / "*.npy"))}
    assert all(v.dtype in (np.float32, np.float64) for v in a.values()) and sum(v.nbytes for v in a.values()) <= 64 << 20
    assert a["treads.position.npy"].size == d["config"]["str_reads_clustered"] > 1000 and "treads.rows.npy" not in a
    assert a["bounds.left.npy"].size == d["config"]["bounds"] > 10
    assert a["treads.repeat.npy"].shape == (d["config"]["str_reads_clustered"], 6)
    _plain(tmp_path / "b")                                                  # same arguments: the same inputs, the same rows
    b = {os.path.basename(f): np.load(f) for f in glob.glob(str(tmp_path / "b" / "*.npy"))}
    assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)


def test_dump_outputs_fits_the_cap_with_a_seeded_sample(tmp_path):
    sys.path.insert(0, ROOT)
    import bench
    from strling_amd import api
    rng = np.random.default_rng(5)
    t = np.zeros(900_000, api.TREAD_DTYPE)
    t["position"] = rng.integers(0, 2 ** 32 - 1, t.size, dtype=np.uint64)
    t["qname_id"] = np.arange(t.size) * 3
    t["repeat"] = [b"CAG", b"AT", b"AAAAAT"] * (t.size // 3)
    b = np.zeros(5000, api.BOUNDS_DTYPE)
    b["left"] = np.arange(b.size)
    u = np.zeros(40, api.UNPLACED_DTYPE)
    u["count"] = 7
    for sub in ("a", "b"):
        bench.dump_outputs(str(tmp_path / sub), {"treads": t, "bounds": b, "unplaced": u})
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(os.listdir(tmp_path / "b"))
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 << 20
    assert all(np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)) for f in files)   # the sample is fixed
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in files}
    assert "treads.rows" in got and "bounds.rows" not in got and "unplaced.rows" not in got
    rows = got["treads.rows"].astype(np.int64)
    assert 0 < rows.size < t.size and np.all(np.diff(rows) > 0)
    assert np.array_equal(got["treads.position"], t["position"][rows].astype(np.float64))
    assert np.array_equal(got["treads.qname_id"], t["qname_id"][rows].astype(np.float64))
    rep = got["treads.repeat"]
    assert rep.dtype == np.float32 and rep.shape == (rows.size, 6)
    assert bytes(rep[0].astype(np.uint8)).rstrip(b"\0") == t["repeat"][rows[0]]
    assert np.array_equal(got["bounds.left"], np.arange(b.size, dtype=np.float64)) and np.all(got["unplaced.count"] == 7)
    assert all(v.dtype in (np.float32, np.float64) for v in got.values())
