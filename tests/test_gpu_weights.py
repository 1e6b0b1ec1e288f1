"""Sequence weights, `from_msa --unaligned --progressive --seq-weights`, on the MI355X through both backends:
mprg_prog_leaf_weights against the plain statement on hand-written tables (the shapes around a wavefront and a workgroup, empty
records, poisoned tables, guard words, multiplicities up to 2^20, 4 096 leaves), its refusals, whole MSAs against
tests/weights_ref.py, the compositions with the other flags, what moves between host and device, and the command line
(tests/weights_common.py holds the checks)."""
import os
import subprocess
import sys

import pytest

from tests import weights_common as wc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", params=["runtime", "torch"])
def backend(request):
    import torch  # noqa: F401  (before the library: HipBackend needs torch's HIP runtime to be the one the library binds)
    from make_prg_amd import backend as b
    return b.HipRuntimeBackend(0) if request.param == "runtime" else b.HipBackend(0)


def test_kernel_equals_the_plain_statement(backend):
    wc.check_kernel(backend)


def test_all_distances_zero_and_all_distances_largest(backend):
    wc.check_extremes(backend)


def test_multiplicities_up_to_two_to_the_twenty(backend):
    wc.check_heavy(backend)


def test_four_thousand_and_ninety_six_leaves(backend):
    wc.check_most_leaves(backend)


def test_refusals(backend):
    wc.check_refusals(backend)


def test_msas_equal_the_statement(backend):
    wc.check_msas(backend)


def test_band_device_tree_and_small_budgets_give_the_same_bytes(backend):
    wc.check_same_bytes(backend)


def test_flag_off_is_today_s_bytes_and_trace(backend):
    wc.check_flag_off(backend)


def test_a_constant_factor_on_the_weights_changes_nothing(backend):
    wc.check_scaling(backend)


def test_over_sampled_loci(backend):
    wc.check_oversampled(backend)


def test_collapse(backend):
    wc.check_collapse(backend)


def test_large_loci(backend):
    wc.check_large_loci(backend)


def test_adjust_direction(backend):
    wc.check_adjust_direction(backend)


def test_retree_refine_tree_and_refine(backend):
    wc.check_retree_and_refine_tree(backend)


def test_what_moves_between_host_and_device(backend):
    wc.check_trace(backend)


def test_parameters(backend):
    wc.check_parameters(backend)


def test_command_line_seq_weights(tmp_path):
    src = tmp_path / "unaligned"
    src.mkdir()
    want = wc.write_inputs(src)
    msa_dir = tmp_path / "msas"
    env = dict(os.environ, PYTHONPATH=ROOT)
    res = subprocess.run([sys.executable, "-m", "make_prg_amd", "from_msa", "--unaligned", "--progressive", "--seq-weights", "--msa-dir",
                          str(msa_dir), "-i", str(src), "-o", str(tmp_path / "A" / "a")], cwd=ROOT, env=env, capture_output=True, text=True,
                         timeout=900)
    assert res.returncode == 0, res.stderr[-3000:]
    log = res.stderr + res.stdout
    assert "--progressive: 6 loci built, 42 merges" in log and wc.log_line() in log
    assert {p: (msa_dir / p).read_text() for p in os.listdir(msa_dir)} == want
    res = subprocess.run([sys.executable, "-m", "make_prg_amd", "from_msa", "--unaligned", "--seq-weights", "-i", str(src), "-o",
                          str(tmp_path / "B" / "b")], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert res.returncode == 2 and "--seq-weights needs --progressive" in res.stderr
