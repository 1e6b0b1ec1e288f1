"""bench.py --dump-outputs: what the last timed step computed, as float .npy files (at most 64 MB), from inputs that are the same
on every run (seeds 0..batch-1 of the config-C generator)."""
import hashlib
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["n_nodes.npy", "prg_digest.npy", "prg_length.npy", "sample_offsets.npy", "sample_seeds.npy", "sample_text.npy"]


def _load(d):
    return {n[:-4]: np.load(os.path.join(d, n)) for n in NAMES}


def test_dump_sample_is_fixed():
    import bench
    assert bench.dump_sample(30000) == bench.dump_sample(30000)
    assert len(bench.dump_sample(30000)) == bench.DUMP_SAMPLE and bench.dump_sample(5) == {0, 1, 2, 3, 4}


def test_write_outputs_layout_and_size_bound(tmp_path):
    import bench
    batch = 30000
    sample = bench.dump_sample(batch)
    rng = np.random.default_rng(3)
    per_seed = {}
    for sd in range(batch):
        if sd == 7:
            per_seed[sd] = (-1, 0, b"", None)          # a locus without a PRG
            continue
        # the worst case for the bound: every sampled PRG longer than its share of the text budget
        p = bytes(rng.integers(65, 91, 200_000 if sd in sample else 16, dtype=np.uint8)) if sd in sample else b"ACGT" * 4
        per_seed[sd] = (len(p), sd % 13 + 1, hashlib.sha256(p).digest()[:8], p if sd in sample else None)
    info = bench.write_outputs(str(tmp_path), batch, per_seed, sample)
    assert sorted(os.listdir(tmp_path)) == NAMES == info["files"]
    a = _load(str(tmp_path))
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(os.path.getsize(os.path.join(tmp_path, n)) for n in NAMES) <= 64 << 20
    assert a["prg_length"].shape == a["n_nodes"].shape == (batch,) and a["prg_digest"].shape == (batch, 2)
    assert a["prg_length"][7] == -1 and not a["prg_digest"][7].any()
    for sd in (0, 8, batch - 1):
        ln, nn, dg, _ = per_seed[sd]
        assert a["prg_length"][sd] == ln and a["n_nodes"][sd] == nn
        assert struct.pack(">II", *a["prg_digest"][sd].astype(np.uint32)) == dg
    assert list(a["sample_seeds"]) == sorted(sample)
    cap = bench.DUMP_TEXT_CAP // len(sample)
    for j, sd in enumerate(sorted(sample)[:5]):
        lo, hi = int(a["sample_offsets"][j]), int(a["sample_offsets"][j + 1])
        assert bytes(a["sample_text"][lo:hi].astype(np.uint8)) == per_seed[sd][3][:cap]


@pytest.mark.gpu
def test_bench_dumps_what_its_last_timed_step_built(tmp_path):
    """A small bench run: the dumped digests and node counts are the oracle's (tests/golden/config_c_digests.bin), the sampled
    text is the PRG those digests describe, and the line reports the steps asked for."""
    import bench
    from tests.config_c_full import REC, load_digests
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--batch", "300", "--steps", "2", "--warmup", "1", "--workers", "1",
           "--no-cpu-baseline", "--no-end-to-end", "--no-cli-leg", "--no-single-worker-leg", "--no-shard-projection", "--no-deep-leg",
           "--dump-outputs", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["steps"] == 2 and line["ms_per_step"] > 0 and line["config"]["dumped_outputs"]["files"] == NAMES
    a = _load(str(out))
    blob = load_digests()
    for sd in range(300):
        rec = blob[REC * sd:REC * (sd + 1)]
        assert struct.pack(">II", *a["prg_digest"][sd].astype(np.uint32)) == rec[:8], sd
        assert int(a["n_nodes"][sd]) == struct.unpack("<I", rec[8:])[0], sd
    assert len(a["sample_seeds"]) == 256
    cap = bench.DUMP_TEXT_CAP // bench.DUMP_SAMPLE
    for j, sd in enumerate(a["sample_seeds"].astype(int)):
        lo, hi = int(a["sample_offsets"][j]), int(a["sample_offsets"][j + 1])
        text = bytes(a["sample_text"][lo:hi].astype(np.uint8))
        assert len(text) == min(a["prg_length"][sd], cap), sd
        assert len(text) == cap or hashlib.sha256(text).digest()[:8] == blob[REC * sd:REC * sd + 8], sd
