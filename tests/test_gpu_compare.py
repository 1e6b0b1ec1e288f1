"""`compare_msa` on the MI355X through both backends: mprg_msa_compare_map and mprg_msa_compare_columns against the plain statement
(the P classes, the 64-column chunks, 8 192 and 8 193 rows, odd offsets, two buffers, poisoned outputs, both tmap layouts, small
budgets), their refusals, the properties, star MSAs against their truth, and the command line in a process of its own
(tests/compare_common.py holds the checks)."""
import os
import subprocess
import sys

import pytest

from tests import compare_common as cc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", params=["runtime", "torch"])
def backend(request):
    import torch  # noqa: F401  (before the library: HipBackend needs torch's HIP runtime to be the one the library binds)
    from make_prg_amd import backend as b
    return b.HipRuntimeBackend(0) if request.param == "runtime" else b.HipBackend(0)


def test_kernels_equal_the_statement(backend):
    cc.check_kernel(backend)


def test_an_msa_against_itself(backend):
    cc.check_identity(backend)


def test_8192_rows_and_one_more(backend):
    cc.check_tall(backend)


def test_reversed_rows(backend):
    cc.check_reversed(backend)


def test_entry_points_called_directly(backend):
    cc.check_direct(backend)


def test_refusals(backend):
    cc.check_refusals(backend)


def test_bad_ranges_give_a_status_and_write_nothing(backend):
    cc.check_bad_ranges(backend)


def test_properties(backend):
    cc.check_properties(backend)


def test_star_msas_against_their_truth(backend):
    cc.check_integration(backend)


def test_adjust_direction_matches_through_the_prefix(backend):
    cc.check_flipped(backend)


def test_command_line(tmp_path):
    td, rd, want = cc.cli_files(tmp_path)
    env = dict(os.environ, PYTHONPATH=ROOT)
    base = [sys.executable, "-m", "make_prg_amd", "compare_msa"]
    res = subprocess.run(base + ["-i", str(td), "-r", str(rd)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    cc.check_tsv(res.stdout, want)
    out = tmp_path / "one.tsv"
    res = subprocess.run(base + ["-i", str(td / "b.fa.gz"), "-r", str(rd / "b.fa"), "-o", str(out)], cwd=ROOT, env=env, capture_output=True,
                         text=True, timeout=600)
    assert res.returncode == 0 and res.stdout == "", res.stderr[-3000:]
    cc.check_tsv(out.read_text(), {"b": want["b"]})
    rows = [l for l in (td / "c.fa").read_text().splitlines() if not l.startswith(">")]
    aln = tmp_path / "c.aln"
    aln.write_text(cc.clustal_text([f"r{i}" for i in range(6)], rows))
    res = subprocess.run(base + ["-i", str(aln), "-r", str(rd / "c.fa"), "-f", "clustal,fasta"], cwd=ROOT, env=env, capture_output=True,
                         text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    assert tuple(int(v) for v in cc.parse_tsv(res.stdout)["c.aln"][:6]) == want["c"]
    (td / "only_here.fa").write_text(">a\nA\n")
    res = subprocess.run(base + ["-i", str(td), "-r", str(rd)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 2 and "only_here.fa" in res.stderr and res.stdout == ""
