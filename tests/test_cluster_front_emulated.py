"""The chain around the KMeans fits, entry point by entry point (tests/cluster_front_cases.py), on the emulation backend: mprg_ungap_dedupe,
mprg_kmer_dictionary / mprg_kmer_counts with their _parts forms and mprg_split_children on hand-built tables against plain restatements
of the reference — every output, exactly.  The library's row-kernel switches run in child processes (they are read once, when the library
loads); the MPRG_TEST_WEAK_HASH build, where every row hash and (under the first two seeds) every k-mer hash collides, leaves the exact
comparisons to decide alone.  A case's docstring or name says which kernel form its shape is placed for (asserted from the restated
predicates in the cases module); which kernel ran is not observed."""
import os
import subprocess
import sys

import pytest

from tests import cluster_front_cases as cf
from tests.emu.backend import EmuBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def emu():
    return EmuBackend()


@pytest.fixture(scope="module")
def weak():
    return EmuBackend(defines=("MPRG_TEST_WEAK_HASH",), tag="_weakhash")


def child(code, **env):
    run = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, sys.argv[1]); from tests import cluster_front_cases as cf; "
                          "from tests.emu.backend import EmuBackend; be = EmuBackend(); " + code, ROOT],
                         env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-3000:]
    return run.stdout


@pytest.mark.parametrize("k", cf.K_ROWS)
def test_row_groups(emu, k):
    """mprg_ungap_dedupe, one call over every view of cluster_front_cases.row_inputs — a wavefront per view (k_rows_wave: 64 x 64 and
    smaller), k_rows_narrow_s (to 128 rows), k_rows_narrow (to 512 rows x 64 columns), the general launches (65 columns; 8-row chunks
    beyond 4 096 columns) and k_dedupe_scan_big (513 rows and more) side by side —: all eleven outputs against the restatement."""
    cf.check_rows(emu, k)


@pytest.mark.parametrize("env", [dict(MPRG_ROW_VIEWS="0"), dict(MPRG_WAVE_VIEWS="0"), dict(MPRG_ROW_VIEWS="0", MPRG_WAVE_VIEWS="0")],
                         ids=["k_dedupe_wave for the small views", "a workgroup per small view", "the general launches for every view"])
def test_row_groups_other_forms(env):
    """The same calls (k = 1, 7, 20) with the lane-per-row kernels off (small views: k_dedupe_wave, narrow ones: the general launches),
    with the wavefront kernels off (small views: k_rows_narrow_s) and with both off: the same outputs, bit for bit."""
    child("cf.check_rows_all(be)", **env)


@pytest.mark.parametrize("k", cf.K_ROWS)
def test_row_groups_when_every_hash_collides(weak, k):
    """MPRG_TEST_WEAK_HASH: every nominee of the LDS tables is refuted (the exact all-pairs search decides) and k_dedupe_scan_big compares
    the symbols of every pair."""
    cf.check_rows(weak, k)


@pytest.mark.parametrize("k", cf.K_KMERS)
def test_kmer_ids_and_counts(emu, k):
    """mprg_kmer_dictionary / mprg_kmer_counts and (k <= 16) their _parts forms with 1, 3, 7, 64 and 1 024 workgroups per problem: V, the
    first-appearance flags and the whole count matrix of every problem against a dict in first-appearance order.  k <= 8: T = 2 048 is
    built in LDS, T = 2 049 in global memory; 9 .. 16: packed keys in global memory; 17, 31: hashed keys.  Every seed is 0.
    Untested: the saturation of out_V at 0xffffff (it takes 16 million distinct k-mers)."""
    cf.check_kmers(emu, k)


@pytest.mark.parametrize("k", [16, 17, 31])
def test_kmer_ids_when_hashes_collide(weak, k):
    """MPRG_TEST_WEAK_HASH: beyond k = 16 every k-mer collides under seeds 0 and 1, so the dictionary is rebuilt twice and reports seed 2
    (seed 0 where a problem has one distinct k-mer: nothing to refute); k = 16 has packed keys and seed 0.  All answers stay exact."""
    cf.check_kmers(weak, k, weak=True)


def test_kmer_refusals(emu):
    cf.check_kmer_refusals(emu)


def test_children(emu):
    """mprg_split_children on hand-written labels: the wavefront form up to 1 024 ranks (exactly 1 024 among the cases), the one-lane form
    beyond (1 025), 63 / 64 / 65 / 200 rows, index lists, the first row's cluster last, in the middle and a short row's, an empty child."""
    cf.check_children(emu)
