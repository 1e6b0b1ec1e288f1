"""The banded pair DP of `from_msa --unaligned --band` on the MI355X, through both backends: 240 config-C-shaped loci through
star_msas(band=True) against star_msas(), align_batch with and without the band on edge, random, leaf-shaped and large pairs, the
second pass, the fall-back and the pair that only the band can hold, and the command line with --band against without."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

from make_prg_amd.from_msa import star_align as sa
from make_prg_amd.msa import encode
from make_prg_amd.update import profile_align as pa
from tests import align_ref as ar
from tests import star_ref as sr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", params=["runtime", "torch"])
def backend(request):
    import torch  # noqa: F401  (before the library: HipBackend needs torch's HIP runtime to be the one the library binds)
    from make_prg_amd import backend as b
    return b.HipRuntimeBackend(0) if request.param == "runtime" else b.HipBackend(0)


def records(seqs):
    return [(f"r{i} desc {i}", s) for i, s in enumerate(seqs)]


def leaf_codes(rows):
    return encode(np.frombuffer("".join(rows).encode(), np.uint8).reshape(len(rows), -1))


def test_config_c_shaped_loci_with_and_without_the_band(backend):
    """240 config-C-shaped loci (S ~ 100, C 1 000-3 000) with their gaps removed, in several locus chunks and pair launches: the
    rows of star_msas(band=True) are star_msas()'s; every pair is certified by the band alone, at a fraction of the cells."""
    recs = [records(seqs) for _, seqs in sr.synthetic_loci(range(240))]
    timings = {}
    banded = sa.star_msas(backend, recs, chunk_bytes=1 << 27, band=True, timings=timings)
    plain = sa.star_msas(backend, recs, chunk_bytes=1 << 27)
    assert len(banded) == len(plain) == 240
    for k, (m, q) in enumerate(zip(banded, plain)):
        assert m.rows_as_strings() == q.rows_as_strings(), k
        assert m.ids == q.ids and m.descriptions == q.descriptions
    print("band counters:", {k: v for k, v in timings.items() if k.startswith("band_")})
    assert timings["band_pairs"] > 20_000 and timings["band_full_pairs"] == 0
    assert timings["band_cells"] < 0.2 * timings["band_full_cells"]
    small = sa.star_msas(backend, recs[:40], budget_bytes=4 * 200 * pa.band_workspace_words(3000, 3000, -64, 64), band=16)
    for m, q in zip(small, plain):                                # pass 1 narrower, dozens of launches
        assert m.rows_as_strings() == q.rows_as_strings()


def test_align_batch_with_and_without_the_band(backend):
    """Edge cases, strip and ring boundaries, random multi-row leaves, 2 000 leaf-shaped pairs and three large pairs (one of
    unrelated sequences): ops and scores equal, for several w0; the large pairs also equal the spec's DP."""
    probs = ar.random_pairs(21)
    rng = np.random.default_rng(5)
    big = []
    for C, n in ((3000, 3100), (3200, 3000), (4000, 3500)):
        rows = ["".join(rng.choice(list("ACGT"), C))]
        s = rows[0][:n] + "".join(rng.choice(list("ACGT"), max(0, n - C)))
        s = s[:700] + s[760:2000] + "".join(rng.choice(list("ACGT"), 45)) + s[2000:]
        big.append((rows, [s, "".join(rng.choice(list("ACGT"), n))]))
    leaves = [leaf_codes(r) for r, _ in probs + big]
    seqs = [[pa._codes(s, "t") for s in ss] for _, ss in probs + big]
    syn_leaves, syn_seqs = ar.synth_leaf_batch(2, 2000)
    leaves, seqs = leaves + syn_leaves, seqs + syn_seqs
    plain = pa.align_batch(backend, leaves, seqs)
    for w0 in (0, 16, True):
        counters = {}
        assert pa.align_batch(backend, leaves, seqs, band=w0, counters=counters) == plain, w0
        assert counters["band_pairs"] == sum(map(len, seqs)) and counters["band_second_passes"] > 0 and counters["band_full_pairs"] > 0
    for k, (rows, ss) in enumerate(big):
        for s, (ops, score) in zip(ss, plain[len(probs) + k]):
            assert (ops.decode(), score) == ar.align_pair_np(rows, s)


def test_second_pass_fall_back_and_the_pair_only_the_band_holds(backend):
    from tests.test_band_emulated import excursion_pair
    rng = np.random.default_rng(11)
    base, other = excursion_pair(rng, 4000, 100)
    x, y = ("".join(rng.choice(list("ACGT"), 200)) for _ in range(2))
    leaves, seqs = [leaf_codes([base]), leaf_codes([x])], [[pa._codes(other, "t"), pa._codes(base[:300] + base[310:], "t")], [pa._codes(y, "t")]]
    counters = {}
    got = pa.align_batch(backend, leaves, seqs, band=16, counters=counters)
    assert got == pa.align_batch(backend, leaves, seqs)
    assert (counters["band_pairs"], counters["band_second_passes"], counters["band_full_pairs"]) == (3, 1, 1)
    assert (got[0][0][0].decode(), got[0][0][1]) == ar.align_pair_np([base], other) and b"I" * 100 in got[0][0][0]
    # a pair whose full traceback exceeds the 1 GB budget: 60 000 x 60 000 needs 1.8 GB, its certified band well under a tenth of that
    L = 60_000
    long_base = rng.integers(0, 4, L).astype(np.uint8)
    s = long_base.copy()
    snp = rng.random(L) < 0.02
    s[snp] = rng.integers(0, 4, int(snp.sum()))
    s = np.concatenate([s[:20_000], rng.integers(0, 4, 30).astype(np.uint8), s[20_000:41_000], s[41_020:]])
    with pytest.raises(pa.ProfileAlignError, match="more than the workspace budget"):
        pa.pairs_on_device(backend, [long_base.reshape(1, -1)], [[s]])
    counters = {}
    (ops, score), = pa.align_batch(backend, [long_base.reshape(1, -1)], [[s]], band=True, counters=counters)[0]
    assert counters["band_full_pairs"] == 0 and counters["band_cells"] < 0.05 * counters["band_full_cells"]
    assert ar.score_of_ops_np(long_base.reshape(1, -1), s, ops) == score
    assert ops.count(b"I") - ops.count(b"D") == 10
    # the same ops as the full DP computes where it fits: the middle of the pair around both indels is too long, so compare a cut
    cut_base, cut_s = long_base[15_000:45_000], s[15_000:45_010]
    assert pa.align_batch(backend, [cut_base.reshape(1, -1)], [[cut_s]], band=True) == pa.align_batch(backend, [cut_base.reshape(1, -1)], [[cut_s]])


def run_cli(args):
    env = dict(os.environ, PYTHONPATH=ROOT)
    res = subprocess.run([sys.executable, "-m", "make_prg_amd"] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-3000:]
    return res


def test_command_line_band(tmp_path):
    from make_prg_amd.utils.synthetic import synth_rows
    src = tmp_path / "unaligned"
    src.mkdir()
    for seed in range(6):
        rows = synth_rows(seed, 30 + 5 * seed, 600 + 300 * seed, 3)
        recs = [(f"s{i} sample {i}", r.decode().replace("-", "")) for i, r in enumerate(rows)]
        text = "".join(f">{t}\n{s[:70]}\n{s[70:]}\n" for t, s in recs)
        name = f"gene{seed}.fa" + (".gz" if seed % 2 else "")
        (src / name).write_bytes(gzip.compress(text.encode()) if seed % 2 else text.encode())
    a, b = str(tmp_path / "A" / "a"), str(tmp_path / "B" / "b")
    run_cli(["from_msa", "--unaligned", "--msa-dir", str(tmp_path / "ma"), "-i", str(src), "-o", a])
    res = run_cli(["from_msa", "--unaligned", "--band", "--msa-dir", str(tmp_path / "mb"), "-i", str(src), "-o", b])
    assert "--band:" in res.stderr + res.stdout
    assert sorted(os.listdir(tmp_path / "ma")) == sorted(os.listdir(tmp_path / "mb")) == sorted(f"gene{k}.fa" for k in range(6))
    for f in os.listdir(tmp_path / "ma"):
        assert (tmp_path / "ma" / f).read_bytes() == (tmp_path / "mb" / f).read_bytes(), f
    for suffix in (".prg.fa", ".prg.bin.zip", ".prg.gfa.zip", ".update_DS.zip"):
        assert open(a + suffix, "rb").read() == open(b + suffix, "rb").read(), suffix
    env = dict(os.environ, PYTHONPATH=ROOT)
    res = subprocess.run([sys.executable, "-m", "make_prg_amd", "from_msa", "--band", "-i", str(src), "-o", str(tmp_path / "C" / "c")],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert res.returncode == 2 and "--band needs --unaligned" in res.stderr
