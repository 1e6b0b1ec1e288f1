"""Retree, `from_msa --unaligned --progressive --retree`, on the MI355X through both backends: mprg_prog_identities against the plain
statement (the shapes around the row block and the LDS column tile, odd offsets, two buffers, permuted leaves, poisoned tables),
its refusals, its tables through mprg_prog_tree and mprg_prog_tree_wide, whole MSAs against tests/retree_ref.py, the compositions
with the other flags, what moves between host and device, and the command line (tests/retree_common.py holds the checks)."""
import os
import subprocess
import sys

import pytest

from tests import retree_common as rc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", params=["runtime", "torch"])
def backend(request):
    import torch  # noqa: F401  (before the library: HipBackend needs torch's HIP runtime to be the one the library binds)
    from make_prg_amd import backend as b
    return b.HipRuntimeBackend(0) if request.param == "runtime" else b.HipBackend(0)


def test_kernel_equals_the_plain_statement(backend):
    rc.check_kernel(backend)


def test_refusals(backend):
    rc.check_refusals(backend)


def test_tables_feed_the_tree_unchanged(backend):
    rc.check_trees(backend)


def test_msas_equal_the_statement(backend):
    rc.check_msas(backend)


def test_one_rebuild(backend):
    rc.check_one_rebuild(backend)


def test_band_device_tree_and_small_budgets_give_the_same_bytes(backend):
    rc.check_same_bytes(backend)


def test_adjust_direction(backend):
    rc.check_adjust_direction(backend)


def test_collapse(backend):
    rc.check_collapse(backend)


def test_large_loci(backend):
    rc.check_large_loci(backend)


def test_refine_tree_and_refine_after_it(backend):
    rc.check_refine_after(backend)


def test_a_merge_beyond_the_limit_ends_the_locus_s_retree(backend):
    rc.check_limit(backend)


def test_what_moves_between_host_and_device(backend):
    rc.check_trace(backend)


def test_parameters(backend):
    rc.check_parameters(backend)


def test_the_counters_the_command_line_logs(backend):
    rc.check_cli_counts(backend)


def test_command_line_retree(tmp_path):
    src = tmp_path / "unaligned"
    src.mkdir()
    want = rc.write_inputs(src)
    msa_dir = tmp_path / "msas"
    env = dict(os.environ, PYTHONPATH=ROOT)
    res = subprocess.run([sys.executable, "-m", "make_prg_amd", "from_msa", "--unaligned", "--progressive", "--retree", "2", "--msa-dir",
                          str(msa_dir), "-i", str(src), "-o", str(tmp_path / "A" / "a")], cwd=ROOT, env=env, capture_output=True, text=True,
                         timeout=900)
    assert res.returncode == 0, res.stderr[-3000:]
    log = res.stderr + res.stdout
    assert "--progressive: 6 loci built, 42 merges" in log and rc.log_line() in log
    assert {p: (msa_dir / p).read_text() for p in os.listdir(msa_dir)} == want
    res = subprocess.run([sys.executable, "-m", "make_prg_amd", "from_msa", "--unaligned", "--retree", "-i", str(src), "-o",
                          str(tmp_path / "B" / "b")], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert res.returncode == 2 and "--retree needs --progressive" in res.stderr
