"""`from_msa --unaligned --collapse-identical` on the MI355X, through both backends: mprg_star_identical and
mprg_prog_columns_weighted called directly (classes at every hash filter width, refusals with guard words, weighted planes against
the unweighted call on the expanded text), whole MSAs against the spec's plain-Python statement (tests/collapse_ref.py) and the
flag-off run, with band, refine and adjust-direction; the command line."""
import os
import subprocess
import sys

import pytest

from tests import collapse_common as cc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", params=["runtime", "torch"])
def backend(request):
    import torch  # noqa: F401  (before the library: HipBackend needs torch's HIP runtime to be the one the library binds)
    from make_prg_amd import backend as b
    return b.HipRuntimeBackend(0) if request.param == "runtime" else b.HipBackend(0)


def test_identical_classes(backend):
    cc.check_identical(backend)


def test_identical_refusals(backend):
    cc.check_identical_refusals(backend)


def test_weighted_columns(backend):
    cc.check_weighted_columns(backend)


def test_weighted_columns_refusals(backend):
    cc.check_weighted_refusals(backend)


def test_star_bytes_are_the_flag_off_bytes(backend):
    cc.check_star(backend)


def test_progressive_equals_the_spec(backend):
    cc.check_progressive(backend)


def test_adjust_direction(backend):
    cc.check_adjust_direction(backend)


def test_leaf_limit_counts_records(backend):
    cc.check_leaf_limit(backend)


def test_command_line_collapse(tmp_path):
    src = tmp_path / "unaligned"
    src.mkdir()
    want = cc.write_inputs(src)
    msa_dir = tmp_path / "msas"
    env = dict(os.environ, PYTHONPATH=ROOT)
    res = subprocess.run([sys.executable, "-m", "make_prg_amd", "from_msa", "--unaligned", "--progressive", "--collapse-identical", "--msa-dir",
                          str(msa_dir), "-i", str(src), "-o", str(tmp_path / "A" / "a")], cwd=ROOT, env=env, capture_output=True, text=True,
                         timeout=900)
    assert res.returncode == 0, res.stderr[-3000:]
    records = sum(cc.n_classes(l)[0] for l in cc.loci()[:2] + cc.loci()[4:7])
    classes = sum(cc.n_classes(l)[1] for l in cc.loci()[:2] + cc.loci()[4:7])
    assert f"--collapse-identical: {records} records, {classes} classes" in res.stderr + res.stdout
    assert {p: (msa_dir / p).read_text() for p in os.listdir(msa_dir)} == want
