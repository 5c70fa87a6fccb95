"""bench.py's command line: a plain run is the headline alone, --full chooses the other legs, and
--dump-outputs writes the last timed step's records as float64 columns (host logic; one plain run on the GPU)."""
import importlib.util
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _parse(bench, monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_and_full_options(bench, monkeypatch):
    a = _parse(bench, monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    a = _parse(bench, monkeypatch, "--full", "--e2e", "--dump-outputs", "d")
    assert a.full and a.e2e and a.dump_outputs == "d"
    # the options that choose among --full's legs are an error without it, not silently ignored
    for opt in ("--e2e", "--stream-ceiling-only"):
        with pytest.raises(SystemExit):
            _parse(bench, monkeypatch, opt)
    with pytest.raises(SystemExit):
        _parse(bench, monkeypatch, "--steps", "0")


@pytest.mark.gpu
def test_plain_run_is_the_headline_alone_and_dumps_its_records(bench, tmp_path):
    """`bench.py --gpus 1 --steps 5 --warmup 1 --dump-outputs DIR`: one JSON line with the headline's keys and none
    of --full's legs; the dumped records are those of the last timed step (step 4 of 4 rotating batches = batch 0,
    global frames [0, 1 Mi)), which hash to the committed oracle digest of those frames."""
    import hashlib
    import json
    import subprocess

    import pollnet_amd as pa

    d = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "1",
                        "--dump-outputs", str(d)], capture_output=True, text=True, timeout=120,
                       env={k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK")})
    assert p.returncode == 0, p.stderr[-3000:]
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 1, lines
    line = json.loads(lines[0])
    assert line["metric"] == bench.METRIC and line["unit"] == "Gbit/s" and line["higher_is_better"] is True
    assert line["steps"] == 5 and line["warmup"] == 1 and line["n_gpus"] == 1 and line["full"] is False
    assert line["value"] > 0 and line["ms_per_step"] > 0 and "integer" in line["dtype"]
    # the timed window's own arithmetic: value = wire bits of one step / ms_per_step (the line rounds ms_per_step to
    # 1e-4 ms, 2.5e-4 of a 0.2-ms step)
    wire_bits = 8 * 1514 * (1 << 20)
    assert abs(line["value"] - wire_bits / (line["ms_per_step"] * 1e-3) / 1e9) <= 1e-3 * line["value"]
    for k in ("secondary", "cpu_baseline", "e2e_host_ring", "e2e_pinned_host", "e2e_zero_copy_pinned_host"):
        assert k not in line, k
    assert "same_run_ceilings" not in line["roofline"] and line["verified_vs_oracle"] is None
    assert list(line)[-1] == "summary"
    assert sorted(os.listdir(d)) == ["records.npy"]
    cols = np.load(d / "records.npy")
    assert cols.dtype == np.float64 and cols.shape == (1 << 20, 6) and cols.nbytes <= 64e6
    rec = np.empty(len(cols), pa.RESULT_DTYPE)
    for c, f in enumerate(pa.RESULT_DTYPE.names):
        rec[f] = cols[:, c]
    assert hashlib.sha256(rec.tobytes()).hexdigest() == bench.golden_digest(2, 0, 1 << 20)["records_sha256"]


def _records(n):
    import pollnet_amd as pa

    rng = np.random.default_rng(7)
    rec = np.zeros(n, pa.RESULT_DTYPE)
    rec["conn_id"] = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    rec["seq"] = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    rec["payload_off"] = rng.integers(0, 1 << 16, n)
    rec["payload_len"] = rng.integers(-(1 << 15), 1 << 15, n)
    rec["flags"] = rng.integers(0, 1 << 16, n)
    rec["tcp_fold"] = rng.integers(0, 1 << 16, n)
    rec[0] = (0xFFFFFFFF, 0xFFFFFFFF, 0xFFFF, -32768, 0xFFFF, 0xFFFF)  # every field's extreme survives a float64
    return rec


def test_dump_outputs_whole(bench, tmp_path):
    import torch

    import pollnet_amd as pa

    n = 64
    rec = _records(n)
    res = torch.from_numpy(rec.view(np.uint8).copy())
    info = bench.dump_outputs(str(tmp_path / "d"), res, n, 0, 1)
    assert sorted(os.listdir(tmp_path / "d")) == ["records.npy"] and info["rows"] == n
    got = np.load(tmp_path / "d" / "records.npy")
    assert got.dtype == np.float64 and got.shape == (n, 6) and info["columns"] == list(pa.RESULT_DTYPE.names)
    for c, f in enumerate(pa.RESULT_DTYPE.names):
        assert np.array_equal(got[:, c].astype(np.int64), rec[f].astype(np.int64)), f


def test_dump_outputs_sample_is_fixed(bench, tmp_path, monkeypatch):
    import torch

    n = 100
    rec = _records(n)
    res = torch.from_numpy(rec.view(np.uint8).copy())
    monkeypatch.setattr(bench, "DUMP_ROWS", 32)
    for d, rank, world, name, rows in (("a", 0, 1, "records", 32), ("b", 0, 1, "records", 32),
                                       ("c", 1, 2, "records_rank1", 16)):
        bench.dump_outputs(str(tmp_path / d), res, n, rank, world)
        idx = np.load(tmp_path / d / (name + "_rows.npy")).astype(np.int64)
        assert len(idx) == rows and np.all(np.diff(idx) > 0) and 0 <= idx[0] and idx[-1] < n
        got = np.load(tmp_path / d / (name + ".npy"))
        assert got.shape == (rows, 6) and np.array_equal(got[:, 1].astype(np.int64), rec["seq"][idx].astype(np.int64))
    assert np.array_equal(np.load(tmp_path / "a" / "records_rows.npy"), np.load(tmp_path / "b" / "records_rows.npy"))
    # the real limit keeps a dump within 64 MB: rows x 6 float64 + the row indices
    monkeypatch.undo()
    assert bench.DUMP_ROWS * (6 + 1) * 8 <= 64e6
