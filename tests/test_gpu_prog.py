"""Progressive MSAs of `from_msa --unaligned --progressive` on the MI355X, through both backends: the 6-mer distances, the
profile-profile DP (ops and score, bit for bit, at the widths around the 64-column strip and the 128-column ring, mostly-gap
columns, ambiguity codes, one side much longer than the other), whole MSAs on the edge, special, random and the 18 table loci in
one call and once more with a small budget, the compositions with --adjust-direction and --refine (with and without --band), all
against the spec's plain-Python statement (tests/prog_ref.py); the status codes of the new entries; the command line."""
import os
import subprocess
import sys

import pytest

from make_prg_amd.update import profile_align as pa
from tests import prog_common as pc
from tests import prog_ref as pr
from tests import refine_ref as rr
from tests import star_ref as sr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", params=["runtime", "torch"])
def backend(request):
    import torch  # noqa: F401  (before the library: HipBackend needs torch's HIP runtime to be the one the library binds)
    from make_prg_amd import backend as b
    return b.HipRuntimeBackend(0) if request.param == "runtime" else b.HipBackend(0)


def test_distances_equal_the_spec(backend):
    loci = sr.edge_loci() + rr.special_loci()
    for seed in (5, 6):
        loci += sr.random_loci(seed)
    pc.check_distances(backend, loci + pr.table_loci()[::6])


def test_profile_pairs_equal_the_spec(backend):
    pc.check_dp(backend)


def test_profile_pairs_in_split_launches(backend):
    pc.check_dp(backend, budget_bytes=4 * pa.workspace_words(200, 300))


def test_tall_profiles_equal_the_spec(backend):
    pc.check_tall_dp(backend)


def test_columns_of_tall_texts(backend):
    pc.check_tall_columns(backend)


def test_planes_agree(backend):
    pc.check_planes_agree(backend)


def test_msas_equal_the_spec(backend):
    pc.check_msas(backend)


def test_msas_with_a_small_budget(backend):
    pc.check_msas(backend, budget_bytes=4 * pa.workspace_words(420, 420), chunk_bytes=1 << 14)


def test_adjust_direction_refine_and_band(backend):
    pc.check_compositions(backend)


def test_abi_statuses(backend):
    pc.check_abi_statuses(backend)


def test_command_line_progressive(tmp_path):
    src = tmp_path / "unaligned"
    src.mkdir()
    want = {}
    for k in range(6):
        recs = [(f"s{i} sample {i}", s) for i, s in enumerate(pr.clade_locus(40 + k, 8))]
        (src / f"gene{k}.fa").write_text("".join(f">{t}\n{s}\n" for t, s in recs))
        want[f"gene{k}.fa"] = pr.progressive_fasta(recs)
    msa_dir = tmp_path / "msas"
    env = dict(os.environ, PYTHONPATH=ROOT)
    res = subprocess.run([sys.executable, "-m", "make_prg_amd", "from_msa", "--unaligned", "--progressive", "--msa-dir", str(msa_dir), "-i",
                          str(src), "-o", str(tmp_path / "A" / "a")], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-3000:]
    assert "--progressive: 6 loci built, 42 merges" in res.stderr + res.stdout and "0 loci left to the star pass" in res.stderr + res.stdout
    assert {p: (msa_dir / p).read_text() for p in os.listdir(msa_dir)} == want
