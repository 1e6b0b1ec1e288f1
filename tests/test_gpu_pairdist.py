"""Pair distances, `from_msa --unaligned --progressive --pair-distances`, on the MI355X through both backends:
mprg_align_pair_scores and mprg_align_pair_scores_banded against the plain DPs and against mprg_align_pairs on the same tables (the
shapes around the 64-row strip and the 128-column ring, leaves of 1 and 3 rows, guard words), their refusals, the host's two passes,
the tables through mprg_prog_tree, mprg_prog_tree_wide and mprg_prog_leaf_weights, the saturated locus, whole MSAs against
tests/pairdist_ref.py, the compositions with the other flags, what moves between host and device, and the command line
(tests/pairdist_common.py holds the checks)."""
import os
import subprocess
import sys

import pytest

from tests import pairdist_common as pc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", params=["runtime", "torch"])
def backend(request):
    import torch  # noqa: F401  (before the library: HipBackend needs torch's HIP runtime to be the one the library binds)
    from make_prg_amd import backend as b
    return b.HipRuntimeBackend(0) if request.param == "runtime" else b.HipBackend(0)


def test_score_kernel_equals_the_dp(backend):
    pc.check_kernel(backend)


def test_banded_score_kernel_equals_the_banded_dp(backend):
    pc.check_banded_kernel(backend)


def test_two_passes_return_the_full_scores(backend):
    pc.check_two_pass(backend)


def test_refusals(backend):
    pc.check_refusals(backend)


def test_tables_feed_the_trees_unchanged(backend):
    pc.check_trees(backend)


def test_the_saturated_locus(backend):
    pc.check_saturated(backend)


def test_msas_equal_the_statement(backend):
    pc.check_msas(backend)


def test_band_device_tree_and_small_budgets_give_the_same_bytes(backend):
    pc.check_same_bytes(backend)


def test_adjust_direction(backend):
    pc.check_adjust_direction(backend)


def test_collapse(backend):
    pc.check_collapse(backend)


def test_large_loci(backend):
    pc.check_large_loci(backend)


def test_seq_weights(backend):
    pc.check_seq_weights(backend)


def test_pair_scores_are_computed_once(backend):
    pc.check_pairs_once(backend)


def test_retree_refine_tree_and_refine_after_it(backend):
    pc.check_after(backend)


def test_a_locus_above_the_cap(backend):
    pc.check_cap(backend)


def test_what_moves_between_host_and_device(backend):
    pc.check_trace(backend)


def test_parameters(backend):
    pc.check_parameters(backend)


def test_the_counters_the_command_line_logs(backend):
    pc.check_cli_counts(backend)


def test_command_line_pair_distances(tmp_path):
    src = tmp_path / "unaligned"
    src.mkdir()
    want = pc.write_inputs(src)
    msa_dir = tmp_path / "msas"
    env = dict(os.environ, PYTHONPATH=ROOT)
    res = subprocess.run([sys.executable, "-m", "make_prg_amd", "from_msa", "--unaligned", "--progressive", "--pair-distances", "--msa-dir",
                          str(msa_dir), "-i", str(src), "-o", str(tmp_path / "A" / "a")], cwd=ROOT, env=env, capture_output=True, text=True,
                         timeout=900)
    assert res.returncode == 0, res.stderr[-3000:]
    log = res.stderr + res.stdout
    assert "--progressive: 6 loci built, 42 merges" in log and pc.log_line() in log
    assert {p: (msa_dir / p).read_text() for p in os.listdir(msa_dir)} == want
    res = subprocess.run([sys.executable, "-m", "make_prg_amd", "from_msa", "--unaligned", "--pair-distances", "-i", str(src), "-o",
                          str(tmp_path / "B" / "b")], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert res.returncode == 2 and "--pair-distances needs --progressive" in res.stderr
