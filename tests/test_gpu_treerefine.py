"""Tree refinement, `from_msa --unaligned --progressive --refine-tree`, on the MI355X, through both backends: mprg_tree_split and
mprg_tree_objective called directly (texts of 2 to 257 rows and 1 to 600 columns around the 256-column tile, every status code),
whole MSAs on the edge, special and 18 table loci against the spec's plain-Python statement (tests/treerefine_ref.py) with one
and two passes, the same bytes under --band, --device-tree and a small budget, --collapse-identical, the cap, the compositions with
--adjust-direction and --refine; the command line (tests/treerefine_common.py holds the checks)."""
import os
import subprocess
import sys

import pytest

from tests import prog_ref as pr
from tests import treerefine_common as tc
from tests import treerefine_ref as tr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", params=["runtime", "torch"])
def backend(request):
    import torch  # noqa: F401  (before the library: HipBackend needs torch's HIP runtime to be the one the library binds)
    from make_prg_amd import backend as b
    return b.HipRuntimeBackend(0) if request.param == "runtime" else b.HipBackend(0)


def test_split_equals_numpy(backend):
    tc.check_split(backend)


def test_split_statuses(backend):
    tc.check_split_statuses(backend)


def test_objective_equals_the_expanded_text(backend):
    tc.check_objective(backend)


def test_objective_statuses(backend):
    tc.check_objective_statuses(backend)


@pytest.mark.parametrize("passes", [1, 2])
def test_msas_equal_the_spec(backend, passes):
    tc.check_counts()
    tc.check_msas(backend, passes)


def test_band_gives_the_same_bytes(backend):
    tc.check_same_bytes(backend, band=True)


def test_device_tree_gives_the_same_bytes(backend):
    tc.check_same_bytes(backend, device_tree=True)


def test_small_budget_gives_the_same_bytes(backend):
    tc.check_same_bytes(backend, **tc.SMALL_BUDGET)


def test_collapse(backend):
    tc.check_collapse(backend)


def test_cap(backend):
    tc.check_cap(backend)


def test_adjust_direction_and_refine(backend):
    tc.check_compositions(backend)


def test_flag_off(backend):
    tc.check_flag_off(backend)


def test_command_line_refine_tree(tmp_path):
    src = tmp_path / "unaligned"
    src.mkdir()
    want, steps, accepted, changed = {}, 0, 0, 0
    for k in range(6):
        seqs = pr.clade_locus(40 + k, 8)
        recs = [(f"s{i} sample {i}", s) for i, s in enumerate(seqs)]
        (src / f"gene{k}.fa").write_text("".join(f">{t}\n{s}\n" for t, s in recs))
        want[f"gene{k}.fa"] = tr.fasta(recs, 2)
        info = tr.progressive(seqs, 2)[1]
        steps, accepted, changed = steps + info[0], accepted + info[1], changed + bool(info[1])
    assert accepted > 0
    msa_dir = tmp_path / "msas"
    env = dict(os.environ, PYTHONPATH=ROOT)
    res = subprocess.run([sys.executable, "-m", "make_prg_amd", "from_msa", "--unaligned", "--progressive", "--refine-tree", "2", "--msa-dir",
                          str(msa_dir), "-i", str(src), "-o", str(tmp_path / "A" / "a")], cwd=ROOT, env=env, capture_output=True, text=True,
                         timeout=900)
    assert res.returncode == 0, res.stderr[-3000:]
    assert (f"--refine-tree 2: {changed} loci refined, {steps} steps tried, {accepted} accepted, 0 skipped, 0 loci above the cap"
            in res.stderr + res.stdout)
    assert {p: (msa_dir / p).read_text() for p in os.listdir(msa_dir)} == want
