"""Progressive MSAs past 4 096 records, `from_msa --unaligned --progressive --collapse-identical --large-loci`, on the MI355X through
both backends: mprg_prog_tree_wide against mprg_prog_tree, the spec's plain statements and the host's tree (the wavefront, the
workgroup's thread count and the LDS limit of 512 records from both sides), scale invariance, exactness where float64 quotients tie
and where the cross products leave 64 bits, the limit and the refusals; whole MSAs of thousands of records over a dozen alleles
against tests/large_ref.py, the compositions, the limits by parameter, what moves between host and device, and the command line
(tests/large_common.py holds the checks)."""
import os
import subprocess
import sys

import pytest

from tests import large_common as lc
from tests import large_ref as lr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", params=["runtime", "torch"])
def backend(request):
    import torch  # noqa: F401  (before the library: HipBackend needs torch's HIP runtime to be the one the library binds)
    from make_prg_amd import backend as b
    return b.HipRuntimeBackend(0) if request.param == "runtime" else b.HipBackend(0)


@pytest.mark.parametrize("weighted", [False, True])
def test_same_trees_below_the_old_limit(backend, weighted):
    lc.check_same_below_limit(backend, weighted)


def test_scale_invariance_across_the_old_limit(backend):
    lc.check_scale_invariance(backend)


def test_exact_where_float64_quotients_tie(backend):
    lc.check_exact(backend)


def test_products_that_leave_64_bits(backend):
    lc.check_overflow(backend)


def test_limit_and_refusals(backend):
    lc.check_refusals(backend)


def test_prog_trees_routes_by_weight_sum(backend):
    lc.check_prog_trees(backend)


def test_bytes_and_counters(backend):
    lc.check_bytes_and_counters(backend)


def test_device_tree_band_and_budget_groups(backend):
    lc.check_compositions(backend)


def test_adjust_direction(backend):
    lc.check_adjust_direction(backend)


def test_refine_tree(backend):
    lc.check_refine_tree(backend)


def test_refine(backend):
    lc.check_refine(backend)


def test_limits_by_parameter(backend):
    lc.check_limits(backend)


def test_what_moves_between_host_and_device(backend):
    lc.check_trace(backend)


def test_command_line_large_loci(tmp_path):
    src = tmp_path / "unaligned"
    src.mkdir()
    want = {}
    for k, l in enumerate(lc.loci()):
        recs = [(f"s{i} sample {i}", s) for i, s in enumerate(l)]
        (src / f"gene{k}.fa").write_text("".join(f">{t}\n{s}\n" for t, s in recs))
        want[f"gene{k}.fa"] = "".join(f">{t}\n{r}\n" for (t, _), r in zip(recs, lc.spec()[k][0]))
    assert want["gene2.fa"] == lr.progressive_fasta([(f"s{i} sample {i}", s) for i, s in enumerate(lc.loci()[2])])
    msa_dir = tmp_path / "msas"
    env = dict(os.environ, PYTHONPATH=ROOT)
    base = [sys.executable, "-m", "make_prg_amd", "from_msa", "--unaligned", "-i", str(src)]
    res = subprocess.run(base + ["--progressive", "--collapse-identical", "--device-tree", "--large-loci", "--msa-dir", str(msa_dir),
                                 "-o", str(tmp_path / "A" / "a")], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-3000:]
    log = res.stderr + res.stdout
    assert "--large-loci: 2 loci of more than 4096 records built progressively (10100 records), 0 over a limit" in log
    assert "--progressive: 3 loci built, 26 merges" in log and "--device-tree: 3 loci's trees built on the device" in log
    assert {p: (msa_dir / p).read_text() for p in os.listdir(msa_dir)} == want
    for flags, needs in ((["--collapse-identical", "--large-loci"], "--progressive"), (["--progressive", "--large-loci"], "--collapse-identical")):
        res = subprocess.run(base + flags + ["-o", str(tmp_path / "B" / "b")], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
        assert res.returncode == 2 and f"--large-loci needs {needs}" in res.stderr
