"""The guide tree on the device, `from_msa --unaligned --progressive --device-tree`, on the MI355X through both backends:
mprg_prog_tree against the spec's plain statements and the host's tree (small trees; the wavefront, the workgroup's thread count
and the LDS limit of 512 records from both sides; weighted; several loci per launch and launches in budget groups), exactness
where float64 quotients tie, the limit and the refusals, whole MSAs against the flag-off run and the references, what moves between
host and device, and the command line (tests/tree_common.py holds the checks)."""
import os
import subprocess
import sys

import pytest

from make_prg_amd.update import profile_align as pa
from tests import prog_ref as pr
from tests import tree_common as tc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", params=["runtime", "torch"])
def backend(request):
    import torch  # noqa: F401  (before the library: HipBackend needs torch's HIP runtime to be the one the library binds)
    from make_prg_amd import backend as b
    return b.HipRuntimeBackend(0) if request.param == "runtime" else b.HipBackend(0)


def test_small_trees_equal_the_plain_statement(backend):
    tc.check_small(backend)


def test_edges_equal_the_host_tree(backend):
    tc.check_edges(backend)


def test_weighted_edges_equal_the_host_tree(backend):
    tc.check_edges(backend, weighted=True)


def test_edges_in_budget_groups(backend):
    tc.check_edges_in_groups(backend)


def test_trees_from_sequences(backend):
    tc.check_prog_trees(backend)


def test_exact_where_float64_quotients_tie(backend):
    tc.check_exact(backend)


def test_limit_and_refusals(backend):
    tc.check_refusals(backend)


def test_msas_equal_the_flag_off_run(backend):
    tc.check_msas(backend)


def test_msas_with_a_small_budget(backend):
    tc.check_msas(backend, budget_bytes=4 * pa.workspace_words(420, 420), chunk_bytes=1 << 14)


def test_adjust_direction_refine_and_band(backend):
    tc.check_compositions(backend)


def test_collapse_gives_the_weighted_tree(backend):
    tc.check_collapse(backend)


def test_what_moves_between_host_and_device(backend):
    tc.check_trace(backend)


def test_command_line_device_tree(tmp_path):
    src = tmp_path / "unaligned"
    src.mkdir()
    want = {}
    for k in range(6):
        recs = [(f"s{i} sample {i}", s) for i, s in enumerate(pr.clade_locus(40 + k, 8))]
        (src / f"gene{k}.fa").write_text("".join(f">{t}\n{s}\n" for t, s in recs))
        want[f"gene{k}.fa"] = pr.progressive_fasta(recs)
    msa_dir = tmp_path / "msas"
    env = dict(os.environ, PYTHONPATH=ROOT)
    res = subprocess.run([sys.executable, "-m", "make_prg_amd", "from_msa", "--unaligned", "--progressive", "--device-tree", "--msa-dir",
                          str(msa_dir), "-i", str(src), "-o", str(tmp_path / "A" / "a")], cwd=ROOT, env=env, capture_output=True, text=True,
                         timeout=900)
    assert res.returncode == 0, res.stderr[-3000:]
    log = res.stderr + res.stdout
    assert "--progressive: 6 loci built, 42 merges" in log and "--device-tree: 6 loci's trees built on the device" in log
    assert {p: (msa_dir / p).read_text() for p in os.listdir(msa_dir)} == want
    res = subprocess.run([sys.executable, "-m", "make_prg_amd", "from_msa", "--unaligned", "--device-tree", "-i", str(src), "-o",
                          str(tmp_path / "B" / "b")], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert res.returncode == 2 and "--device-tree needs --progressive" in res.stderr
