"""bench.py's plain run, --full and --dump-outputs: the dump holds exactly the bits the decode left
(u32 words in float64, bytes in float32), a batch past the limits is sampled the same way in every
run, and a plain run's line carries the headline alone while --full adds the other legs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
HEADLINE_KEYS = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus"}
FULL_ONLY_KEYS = {"encode", "copy_ref", "parity", "host_e2e", "split_gather", "snappy", "cpu_baseline"}


def _buffers(n, n_elems, nb, seed=5):
    import torch
    rng = np.random.default_rng(seed)
    vals = rng.integers(0, 256, n * 16, dtype=np.uint8)
    elems = rng.integers(0, 256, (n_elems + 7) * 16, dtype=np.uint8)   # capacity past the count
    arena = rng.integers(0, 256, (nb + 15) & ~15, dtype=np.uint8)
    tot = np.array([n_elems, nb, 0, 2 ** 40 + 3], np.uint64)
    return torch, tot, vals, elems, arena


def test_dump_is_bit_exact_and_typed(tmp_path):
    n, ne, nb = 300, 1234, 16 * 500 + 9
    torch, tot, vals, elems, arena = _buffers(n, ne, nb)
    bench.dump_outputs(str(tmp_path), torch, tot, torch.from_numpy(vals), torch.from_numpy(elems),
                       torch.from_numpy(arena), n, ne, nb)
    got = {f[:-4]: np.load(tmp_path / f) for f in sorted(os.listdir(tmp_path))}
    assert sorted(got) == ["arena", "elems", "totals", "values"]
    assert got["totals"].dtype == np.float64 and got["totals"].tolist() == [ne, nb, 0, 2 ** 40 + 3]
    assert got["values"].dtype == np.float64 and got["values"].shape == (n, 4)
    assert np.array_equal(got["values"].astype("<u4").view(np.uint8).ravel(), vals)
    assert got["elems"].dtype == np.float64 and got["elems"].shape == (ne, 4)   # the written ones only
    assert np.array_equal(got["elems"].astype("<u4").view(np.uint8).ravel(), elems[: ne * 16])
    # every decoded arena byte, the 9-byte tail included; the tail row's padding is zero whatever
    # the buffer holds past the blob bytes
    assert got["arena"].dtype == np.float32 and got["arena"].shape == (nb // 16 + 1, 16)
    assert np.array_equal(got["arena"].astype(np.uint8).ravel()[:nb], arena[:nb])
    assert arena[nb:].any() and not got["arena"].ravel()[nb:].any()


def test_dump_samples_large_outputs_reproducibly(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_VALUES", 64)
    monkeypatch.setattr(bench, "DUMP_ELEMS", 128)
    monkeypatch.setattr(bench, "DUMP_ARENA", 32)
    n, ne, nb = 1000, 5000, 16 * 900 + 5
    torch, tot, vals, elems, arena = _buffers(n, ne, nb)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), torch, tot, torch.from_numpy(vals), torch.from_numpy(elems),
                           torch.from_numpy(arena), n, ne, nb)
    for name, rows in (("values", 64), ("elems", 128), ("arena", 32 + 1)):   # (+ the arena's tail row)
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert len(a) == rows and np.array_equal(a, b)
    assert np.array_equal(a[-1, :5].astype(np.uint8), arena[16 * 900: nb]) and not a[-1, 5:].any()
    # every sampled row is a row of the buffer, in buffer order
    rec = vals.view("<u4").reshape(n, 4).astype(np.float64)
    at = [int(np.flatnonzero((rec == r).all(axis=1))[0]) for r in np.load(tmp_path / "a" / "values.npy")]
    assert at == sorted(at)


def test_dump_past_every_limit_stays_under_64_mb(tmp_path):
    """Outputs past all three limits (with an arena tail): everything the dump writes, summed."""
    import torch
    n, ne, nb = bench.DUMP_VALUES + 1, bench.DUMP_ELEMS + 1, 16 * (bench.DUMP_ARENA + 1) + 3
    tot = np.array([ne, nb, 0, 0], np.uint64)
    bench.dump_outputs(str(tmp_path), torch, tot, torch.zeros(n * 16, dtype=torch.uint8),
                       torch.zeros(ne * 16, dtype=torch.uint8), torch.zeros((nb + 15) & ~15, dtype=torch.uint8),
                       n, ne, nb)
    files = sorted(os.listdir(tmp_path))
    assert files == ["arena.npy", "elems.npy", "totals.npy", "values.npy"]
    assert sum(os.path.getsize(tmp_path / f) for f in files) <= 64 * 10 ** 6
    assert len(np.load(tmp_path / "values.npy")) == bench.DUMP_VALUES
    assert len(np.load(tmp_path / "elems.npy")) == bench.DUMP_ELEMS
    assert len(np.load(tmp_path / "arena.npy")) == bench.DUMP_ARENA + 1


N_BENCH = 6000   # past the one-launch kernels' 4096 values, and small enough that nothing is sampled


def _bench_line(args):
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--n", str(N_BENCH), "--steps", "3", "--warmup", "1"] + args,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0]), r.stderr


@pytest.mark.gpu
def test_plain_run_is_the_headline_alone_and_dumps_the_decode(tmp_path):
    """A plain run times --steps decode steps and nothing else; its dump is the oracle's decode of
    the same seeded batch, bit for bit."""
    import redrock_old_amd as rr
    from oracle import cpu
    out, err = _bench_line(["--dump-outputs", str(tmp_path), "--no-snappy"])
    assert HEADLINE_KEYS <= set(out) and not (FULL_ONLY_KEYS & set(out))
    assert "--no-snappy: only --full" in err   # an option that trims --full's legs is named, not silently dropped
    assert out["steps"] == 3 and out["warmup"] == 1 and out["ms_per_step"] > 0 and out["unit"] == "GiB/s"
    data, offs = rr.gen_batch(4, N_BENCH, int(rr.lib().rr_gen_default_seed(4)))
    ov, oe, oa, ot = cpu.decode(data, offs)
    nb = int(offs[-1])
    assert N_BENCH <= bench.DUMP_VALUES and ot["n_elems"] <= bench.DUMP_ELEMS and nb // 16 <= bench.DUMP_ARENA
    assert out["config"]["blob_bytes_per_gpu"] == nb and out["config"]["descriptors_per_gpu"] == ot["n_elems"]
    assert np.load(tmp_path / "totals.npy")[0] == ot["n_elems"] and np.load(tmp_path / "totals.npy")[2] == 0
    assert np.array_equal(np.load(tmp_path / "values.npy").astype("<u4").view(rr.VALUE_DT).ravel(), ov)
    assert np.array_equal(np.load(tmp_path / "elems.npy").astype("<u4").view(rr.ELEM_DT).ravel(), oe)
    got = np.load(tmp_path / "arena.npy").astype(np.uint8).ravel()
    assert len(got) == (nb + 15) // 16 * 16 and np.array_equal(got[:nb], oa[:nb]) and not got[nb:].any()


@pytest.mark.gpu
def test_full_run_adds_the_other_legs():
    out, err = _bench_line(["--full", "--cpu-seconds", "1"])
    assert "only --full" not in err
    assert HEADLINE_KEYS <= set(out) and FULL_ONLY_KEYS <= set(out)
    assert out["parity"] == {"roundtrip_bit_exact": True, "n_bad": 0, "decode_vs_oracle_bit_exact": True}
    assert out["copy_ref"]["bit_exact"] and out["snappy"]["roundtrip_bit_exact"]
    assert out["split_gather"]["gather_bit_exact"] and out["host_e2e"]["matches_device_decode"]
