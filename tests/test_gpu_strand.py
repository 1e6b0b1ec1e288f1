"""`from_msa --unaligned --adjust-direction` on the MI355X, through both backends: canonical centres, strand evidence, reverse
complements, decisions and MSAs byte-equal to the spec's statement (tests/strand_ref.py) on edge, random and golden loci with a
seeded half of the records flipped; config-C-shaped loci in several locus chunks and pair launches, whose flips must be found and
whose MSAs must equal the flag-off MSAs of the unflipped records; and the command line end to end."""
import gzip
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from make_prg_amd.from_msa import star_align as sa
from make_prg_amd.update import profile_align as pa
from tests import star_ref as sr
from tests import strand_ref as st

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module", params=["runtime", "torch"])
def backend(request):
    import torch  # noqa: F401  (before the library: HipBackend needs torch's HIP runtime to be the one the library binds)
    from make_prg_amd import backend as b
    return b.HipRuntimeBackend(0) if request.param == "runtime" else b.HipBackend(0)


def records(seqs):
    return [(f"r{i} desc {i}", s) for i, s in enumerate(seqs)]


def golden_loci():
    with gzip.open(os.path.join(HERE, "golden", "integration.json.gz"), "rt") as fh:
        cases = json.load(fh)["cases"]
    from make_prg_amd.msa import _parse_fasta
    loci = [[s.replace("-", "") for _, s in _parse_fasta(l["fasta"])] for c in cases for l in c["loci"]]
    return [l for l in loci if set("".join(l).upper()) <= sr.ALLOWED]      # (one case holds a letter outside the alphabet)


def test_edge_random_and_golden_loci_equal_the_spec(backend):
    rng = random.Random(31)
    loci = sr.edge_loci() + st.strand_edge_loci() + [st.flip(rng, l, keep_first=False)[0] for l in sr.random_loci(11, 60) + golden_loci()]
    assert len(loci) >= 100
    codes = [sa.locus_codes(str(i), records(l)) for i, l in enumerate(loci)]
    norm = [[sr.normalise(s) for s in l] for l in loci]
    cent = sa.canonical_centres(backend, codes).tolist()
    assert cent == [st.canonical_centre(l) for l in norm]
    ev = sa.strand_evidence(backend, codes, cent)
    assert ev.tolist() == [list(st.evidence(l[c], s)) for l, c in zip(norm, cent) for s in l]
    flat = [c for cs in codes for c in cs]
    total = sum(len(c) for c in flat)
    off = np.concatenate([[0], np.cumsum([len(c) for c in flat])]).astype(np.int64)
    d = backend.upload(np.concatenate(flat + [np.zeros(total, np.uint8)]))
    sa.revcomp_on_device(backend, d, 2 * total, np.stack([off[:-1], np.diff(off), total + off[:-1]], 1))
    got = backend.download(d, np.uint8, 2 * total)
    assert got.tobytes() == np.concatenate(flat + [sa.revcomp(c) for c in flat]).tobytes()
    ori = []
    msas = sa.star_msas(backend, [records(l) for l in loci], adjust_direction=True, orientation=ori)
    for l, m, (rev, how) in zip(loci, msas, ori):
        want_rev, want_how, _, want_rows = st.star_rows(l)
        assert (rev, how) == (want_rev, want_how), l
        assert m.rows_as_strings() == want_rows, l
        assert m.descriptions == st.titles(records(l), want_rev), l
        assert m.ids == [("_R_" if f else "") + f"r{i}" for i, f in enumerate(want_rev)]
    hows = "".join(how for _, how in ori)
    assert all(hows.count(h) >= 3 for h in "-kdt"), {h: hows.count(h) for h in "-kdt"}


def test_config_c_shaped_loci_with_half_of_the_records_flipped(backend):
    """240 config-C-shaped loci (S ~ 100, C 1 000-3 000) with their gaps removed and a random half of all records but the first
    reverse-complemented, in several locus chunks and pair launches: the flips are what comes back as `reversed`, and the MSAs are
    the flag-off MSAs of the same backend on the unflipped records (rows; the titles differ by _R_ exactly where flipped)."""
    rng = random.Random(7)
    plain = [seqs for _, seqs in sr.synthetic_loci(range(240))]
    mixed, flags = zip(*(st.flip(rng, l) for l in plain))
    budget = 4 * 600 * pa.workspace_words(3000, 3000)            # ~600 long pairs per launch: dozens of launches
    ori = []
    on = sa.star_msas(backend, [records(l) for l in mixed], budget_bytes=budget, chunk_bytes=1 << 27, adjust_direction=True, orientation=ori)
    off = sa.star_msas(backend, [records(l) for l in plain], budget_bytes=budget, chunk_bytes=1 << 27)
    n = sum(len(l) for l in plain)
    assert sum(map(sum, flags)) > n // 3
    assert [rev for rev, _ in ori] == [list(f) for f in flags]
    assert sum(how.count("d") + how.count("t") for _, how in ori) <= n // 100
    for k, (m, w, f) in enumerate(zip(on, off, flags)):
        assert np.array_equal(m.data, w.data), k
        assert m.descriptions == [("_R_" if x else "") + t for t, x in zip(w.descriptions, f)]


def run_cli(args):
    env = dict(os.environ, PYTHONPATH=ROOT)
    res = subprocess.run([sys.executable, "-m", "make_prg_amd"] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-3000:]
    return res


def test_command_line_adjust_direction(tmp_path):
    from make_prg_amd.utils.synthetic import synth_rows
    rng = random.Random(13)
    plain, mixed = tmp_path / "plain", tmp_path / "mixed"
    plain.mkdir()
    mixed.mkdir()
    want, n_flipped = {}, 0
    for seed in range(6):
        seqs = [r.decode().replace("-", "") for r in synth_rows(seed, 30 + 5 * seed, 300 + 40 * seed, 3)]
        flipped, flags = st.flip(rng, seqs)
        n_flipped += sum(flags)
        name = f"gene{seed}.fa" + (".gz" if seed % 2 else "")
        for d, ss in ((plain, seqs), (mixed, flipped)):
            text = "".join(f">s{i} sample {i}\n{s[:70]}\n{s[70:]}\n" for i, s in enumerate(ss))
            (d / name).write_bytes(gzip.compress(text.encode()) if seed % 2 else text.encode())
        want[f"gene{seed}"] = st.star_fasta([(f"s{i} sample {i}", s) for i, s in enumerate(flipped)])
    assert n_flipped >= 60
    msa_dir, a, b, c = tmp_path / "msas", str(tmp_path / "A" / "a"), str(tmp_path / "B" / "b"), str(tmp_path / "C" / "c")
    res = run_cli(["from_msa", "--unaligned", "--adjust-direction", "--msa-dir", str(msa_dir), "-i", str(mixed), "-o", a])
    assert f"{n_flipped} records reverse-complemented" in res.stderr + res.stdout
    run_cli(["from_msa", "-i", str(msa_dir), "-o", b])
    run_cli(["from_msa", "--unaligned", "-i", str(plain), "-o", c])
    assert sorted(os.listdir(msa_dir)) == sorted(f"{l}.fa" for l in want)
    for locus, text in want.items():
        assert (msa_dir / f"{locus}.fa").read_text() == text, locus
    assert sum(t.count(">_R_") for t in want.values()) == n_flipped
    for suffix in (".prg.fa", ".prg.bin.zip", ".prg.gfa.zip", ".update_DS.zip"):
        assert open(a + suffix, "rb").read() == open(b + suffix, "rb").read(), suffix
    assert open(a + ".prg.fa", "rb").read() == open(c + ".prg.fa", "rb").read()
    # the flag needs --unaligned
    env = dict(os.environ, PYTHONPATH=ROOT)
    res = subprocess.run([sys.executable, "-m", "make_prg_amd", "from_msa", "--adjust-direction", "-i", str(msa_dir), "-o", str(tmp_path / "D" / "d")],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert res.returncode == 2 and "--adjust-direction needs --unaligned" in res.stderr
