"""GPU twin of tests/test_cluster_front_emulated.py: mprg_ungap_dedupe, mprg_kmer_dictionary / mprg_kmer_counts with their _parts forms and
mprg_split_children on the MI355X, the same hand-built tables (tests/cluster_front_cases.py) against the same plain restatements, every
output exactly; the library's row-kernel switches in child processes.  A case's docstring or name says which kernel form its shape is
placed for (asserted from the restated predicates in the cases module); which kernel ran is not observed.  Run with `-m gpu`."""
import os
import subprocess
import sys

import pytest

from tests import cluster_front_cases as cf

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rt():
    import torch  # noqa: F401  (before the library: a later HipBackend needs torch's HIP runtime to be the one the library binds)
    from make_prg_amd.backend import HipRuntimeBackend
    return HipRuntimeBackend(0)


def child(code, **env):
    run = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, sys.argv[1]); from tests import cluster_front_cases as cf; "
                          "from make_prg_amd.backend import HipRuntimeBackend; be = HipRuntimeBackend(0); " + code, ROOT],
                         env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-3000:]
    return run.stdout


@pytest.mark.parametrize("k", cf.K_ROWS)
def test_row_groups(rt, k):
    """mprg_ungap_dedupe, one call over every view of cluster_front_cases.row_inputs — a wavefront per view (k_rows_wave: 64 x 64 and
    smaller), k_rows_narrow_s (to 128 rows), k_rows_narrow (to 512 rows x 64 columns), the general launches (65 columns; 8-row chunks
    beyond 4 096 columns) and k_dedupe_scan_big (513 rows and more) side by side —: all eleven outputs against the restatement."""
    cf.check_rows(rt, k)


@pytest.mark.parametrize("env", [dict(MPRG_ROW_VIEWS="0"), dict(MPRG_WAVE_VIEWS="0"), dict(MPRG_ROW_VIEWS="0", MPRG_WAVE_VIEWS="0")],
                         ids=["k_dedupe_wave for the small views", "a workgroup per small view", "the general launches for every view"])
def test_row_groups_other_forms(env):
    """The same calls (k = 1, 7, 20) with the lane-per-row kernels off (small views: k_dedupe_wave, narrow ones: the general launches),
    with the wavefront kernels off (small views: k_rows_narrow_s) and with both off: the same outputs, bit for bit."""
    child("cf.check_rows_all(be)", **env)


@pytest.mark.parametrize("k", cf.K_KMERS)
def test_kmer_ids_and_counts(rt, k):
    """mprg_kmer_dictionary / mprg_kmer_counts and (k <= 16) their _parts forms with 1, 3, 7, 64 and 1 024 workgroups per problem: V, the
    first-appearance flags and the whole count matrix of every problem against a dict in first-appearance order.  k <= 8: T = 2 048 is
    built in LDS, T = 2 049 in global memory; 9 .. 16: packed keys in global memory; 17, 31: hashed keys.  Every seed is 0.
    Not run here: the rebuild of a hashed dictionary with the next seed — no product build has the weak hash of the emulation's test
    variant, and a collision of the real 64-bit hash cannot be constructed —, and the saturation of out_V at 0xffffff (16 million
    distinct k-mers)."""
    cf.check_kmers(rt, k)


def test_kmer_refusals(rt):
    cf.check_kmer_refusals(rt)


def test_children(rt):
    """mprg_split_children on hand-written labels: the wavefront form up to 1 024 ranks (exactly 1 024 among the cases), the one-lane form
    beyond (1 025), 63 / 64 / 65 / 200 rows, index lists, the first row's cluster last, in the middle and a short row's, an empty child."""
    cf.check_children(rt)
