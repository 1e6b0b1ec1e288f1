"""Centre-star MSAs of `from_msa --unaligned` on the MI355X, through both backends: centres and MSAs byte-equal to the spec's
statement (tests/star_ref.py) on random, edge and golden loci and on config-C-shaped synthetic loci (several pair launches and
locus chunks), the merge and centre entries called directly on hand-built tables (tests/star_common.py), and the command line: the MSAs it writes, the PRG outputs identical to from_msa on those MSAs, and `update
--aligner builtin` on its update_DS.zip."""
import gzip
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from make_prg_amd.from_msa import star_align as sa
from make_prg_amd.update import profile_align as pa
from tests import align_ref as ar
from tests import star_common as sc
from tests import star_ref as sr

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


def test_random_edge_and_golden_loci_equal_the_spec(backend):
    loci = sr.edge_loci() + sr.random_loci(11, 60) + golden_loci()
    codes = [sa.locus_codes(str(i), records(l)) for i, l in enumerate(loci)]
    got_c = sa.centres(backend, codes).tolist()
    msas = sa.star_msas(backend, [records(l) for l in loci])
    assert len(msas) == len(loci) >= 90
    for l, c, m in zip(loci, got_c, msas):
        want_c, want_rows = sr.star_rows(l)
        assert c == want_c, l
        assert m.rows_as_strings() == want_rows, l


def test_config_c_shaped_loci(backend):
    """240 config-C-shaped loci (S ~ 100, C 1 000-3 000) with their gaps removed, in several locus chunks and pair launches.
    Centres: the spec's.  MSAs: the spec's merge of the device's pairs (whose ops k_align_pairs' own tests pin to the spec's DP),
    and the spec's DP itself on a sample of the pairs."""
    loci = [seqs for _, seqs in sr.synthetic_loci(range(240))]
    recs = [records(l) for l in loci]
    budget = 4 * 600 * pa.workspace_words(3000, 3000)            # ~600 long pairs per launch: dozens of launches
    msas = sa.star_msas(backend, recs, budget_bytes=budget, chunk_bytes=1 << 27)
    codes = [sa.locus_codes(str(i), r) for i, r in enumerate(recs)]
    cent = [sr.centre(l) for l in loci]
    assert sa.centres(backend, codes).tolist() == cent
    others = [[a for a in range(len(l)) if a != c] for l, c in zip(loci, cent)]
    res = pa.align_batch(backend, [codes[k][c].reshape(1, -1) for k, c in enumerate(cent)],
                         [[codes[k][a] for a in others[k]] for k in range(len(loci))])
    rng = np.random.default_rng(3)
    checked = 0
    for k, (l, c, m) in enumerate(zip(loci, cent, msas)):
        merged = ar.merge([l[c]], [l[a] for a in others[k]], [ops.decode() for ops, _ in res[k]])
        want = [None] * len(l)
        want[c] = merged[0]
        for a, r in zip(others[k], merged[1:]):
            want[a] = r
        assert m.rows_as_strings() == want, k
        if k % 40 == 0:
            for q in rng.choice(len(others[k]), 2, replace=False):
                assert (res[k][q][0].decode(), res[k][q][1]) == ar.align_pair_np([l[c]], l[others[k][q]])
                checked += 1
    assert checked == 12


def test_merge_entries_on_hand_built_ops(backend):
    sc.check_merge(backend)


def test_merge_entries_refuse_bad_rows_and_loci(backend):
    sc.check_merge_statuses(backend)


def test_centre_entries_directly(backend):
    sc.check_centres(backend)


def run_cli(args):
    env = dict(os.environ, PYTHONPATH=ROOT)
    res = subprocess.run([sys.executable, "-m", "make_prg_amd"] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-3000:]
    return res


def test_command_line_unaligned(tmp_path):
    from make_prg_amd.utils.synthetic import synth_rows
    src = tmp_path / "unaligned"
    src.mkdir()
    want = {}
    for seed in range(6):
        rows = synth_rows(seed, 30 + 5 * seed, 300 + 40 * seed, 3)
        recs = [(f"s{i} sample {i}", r.decode().replace("-", "")) for i, r in enumerate(rows)]
        text = "".join(f">{t}\n{s[:70]}\n{s[70:]}\n" for t, s in recs)
        name = f"gene{seed}.fa" + (".gz" if seed % 2 else "")
        (src / name).write_bytes(gzip.compress(text.encode()) if seed % 2 else text.encode())
        want[f"gene{seed}"] = sr.star_fasta(recs)
    msa_dir, a, b = tmp_path / "msas", str(tmp_path / "A" / "a"), str(tmp_path / "B" / "b")
    run_cli(["from_msa", "--unaligned", "--msa-dir", str(msa_dir), "-i", str(src), "-o", a])
    run_cli(["from_msa", "-i", str(msa_dir), "-o", b])
    assert sorted(os.listdir(msa_dir)) == sorted(f"{l}.fa" for l in want)
    for locus, text in want.items():
        assert (msa_dir / f"{locus}.fa").read_text() == text, locus
    for suffix in (".prg.fa", ".prg.bin.zip", ".prg.gfa.zip", ".update_DS.zip"):
        assert open(a + suffix, "rb").read() == open(b + suffix, "rb").read(), suffix
    # existing MSAs are not overwritten without -F; the temporary directory of a run without --msa-dir is gone afterwards
    env = dict(os.environ, PYTHONPATH=ROOT)
    res = subprocess.run([sys.executable, "-m", "make_prg_amd", "from_msa", "--unaligned", "--msa-dir", str(msa_dir), "-i", str(src),
                          "-o", str(tmp_path / "C" / "c")], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert res.returncode != 0 and "already exists" in res.stderr
    run_cli(["from_msa", "--unaligned", "-i", str(src), "-o", str(tmp_path / "D" / "d")])
    assert sorted(os.listdir(tmp_path / "D")) == ["d.prg.bin.zip", "d.prg.fa", "d.prg.gfa.zip", "d.update_DS.zip"]
    assert open(str(tmp_path / "D" / "d.prg.fa"), "rb").read() == open(a + ".prg.fa", "rb").read()


def test_update_aligner_builtin_on_an_unaligned_run(tmp_path):
    from tests import update_common as uc
    case = next(c for c in uc.load_cases()["cases"] if c["case"] == "sample_example_update")
    from make_prg_amd.msa import _parse_fasta
    src = tmp_path / "unaligned"
    src.mkdir()
    for f in case["inputs"]:
        (src / f["name"]).write_text("".join(f">{t}\n{s.replace('-', '')}\n" for t, s in _parse_fasta(f["fasta"])))
    (tmp_path / "denovo_paths.txt").write_text(case["denovo_paths"])
    base = str(tmp_path / "base" / "sample")
    run_cli(["from_msa", "--unaligned", "-i", str(src), "-o", base])
    run_cli(["update", "-u", base + ".update_DS.zip", "-d", str(tmp_path / "denovo_paths.txt"), "-o", str(tmp_path / "out" / "u"),
             "-D", str(case["long_deletion_threshold"]), "--aligner", "builtin"])
    assert os.path.exists(str(tmp_path / "out" / "u") + ".prg.fa")
