"""Position-specific gap opens of `from_msa --unaligned --progressive --position-gaps` (star_align.py "Position gaps",
csrc/pg_pairs.inc, csrc/pg_pairs_band.inc, csrc/pg_band_widths.inc) on the CPU emulation build: the plain-Python statement
(tests/posgap_ref.py) against itself and against prog_ref, then tests/posgap_common.py's checks of the new entries, the two-pass
host passes, whole MSAs, the flag compositions, the finding and the command line."""
import random

import numpy as np
import pytest

from tests import band_ref as br
from tests import collapse_ref as cr
from tests import posgap_common as pgc
from tests import posgap_ref as pg
from tests import prog_common as pc
from tests import prog_ref as pr
from tests import progband_ref as pbr
from tests.emu.backend import EmuBackend


@pytest.fixture(scope="module")
def emu():
    return EmuBackend()


# ---- 1. the reference against itself
def test_row_form_equals_cell_form_full_and_banded():
    rng = random.Random(1)
    differ = 0
    for k in range(40):
        X = pr.random_profiles(rng, rng.choice(pc.ROWS), rng.randint(1, 30), rng.choice([0.1, 0.7]), rng.choice([0.0, 0.2]))
        Y = pr.random_profiles(rng, rng.choice(pc.ROWS), rng.randint(1, 30), rng.choice([0.1, 0.7]), rng.choice([0.0, 0.2]))
        n, C = len(X[0]), len(Y[0])
        want = pg.align_profiles(X, Y)
        assert want == pg.align_profiles_np(X, Y) == pg.align_profiles_banded(X, Y, -n, C)
        band = (min(0, C - n) - rng.choice([0, 1, 2, 5, 100]), max(0, C - n) + rng.choice([0, 1, 2, 5, 100]))
        assert pg.align_profiles_banded(X, Y, *band) == pg.align_profiles_banded_np(X, Y, *band)
        differ += want != pr.align_profiles(X, Y)
    assert differ >= 10


def test_gap_free_sides_give_prog_ref_exactly():
    rng = random.Random(2)
    for k in range(20):
        X = pr.random_profiles(rng, rng.choice(pc.ROWS), rng.randint(1, 30), 0.0, 0.2)
        Y = pr.random_profiles(rng, rng.choice(pc.ROWS), rng.randint(1, 30), 0.0, 0.2)
        Oc, Ox = pg.opens(X, Y)
        assert set(Oc) == set(Ox) == {-704}
        assert pg.align_profiles(X, Y) == pg.align_profiles_np(X, Y) == pr.align_profiles(X, Y)


def test_weighted_form_equals_the_expanded_rows():
    rng = random.Random(3)
    for k in range(20):
        X = pr.random_profiles(rng, rng.choice(pc.ROWS), rng.randint(1, 30), rng.choice([0.1, 0.7]), 0.1)
        Y = pr.random_profiles(rng, rng.choice(pc.ROWS), rng.randint(1, 30), rng.choice([0.1, 0.7]), 0.1)
        wx, wy = [rng.randint(1, 5) for _ in X], [rng.randint(1, 5) for _ in Y]
        ex, ey = cr.expanded(X, wx), cr.expanded(Y, wy)
        assert pg.align_profiles_np(X, Y, wx, wy) == pg.align_profiles_np(ex, ey) == pg.align_profiles(ex, ey)
        for a, b in zip(pg.tables(X, Y, wx, wy), pg.tables(ex, ey)):
            assert a == b if isinstance(a, int) else all(np.array_equal(a[x], b[x]) for x in a) if isinstance(a, dict) else np.array_equal(a, b)


def test_new_u_equals_the_old_u_on_one_row_acgt_sides_and_never_rises():
    rng = random.Random(4)
    for _ in range(12):
        X = ["".join(rng.choice("ACGT") for _ in range(rng.randint(2, 60)))]
        Y = ["".join(rng.choice("ACGT") for _ in range(rng.randint(2, 60)))]
        n, C = len(X[0]), len(Y[0])
        b = pg.bounds(X, Y)
        assert b[3:] == (-704, -704)
        assert all(pg.U(*b, n, C, w) == pbr.U(*b[:3], n, C, w) for w in range(min(n, C) + 1))
    for k in range(12):
        X = pr.random_profiles(rng, 7, rng.randint(2, 60), 0.7)
        Y = pr.random_profiles(rng, 7, rng.randint(2, 60), 0.7)
        n, C = len(X[0]), len(Y[0])
        b = pg.bounds(X, Y)
        us = [pg.U(*b, n, C, w) for w in range(min(n, C) + 1)]
        assert all(x >= y for x, y in zip(us, us[1:])) and all(u >= pbr.U(*b[:3], n, C, w) for w, u in enumerate(us))
        s = rng.randint(us[-1] - 5, us[0] + 5)
        w = pg.wstar(*b, n, C, s)
        assert (w == min(n, C) or us[w] < s) and all(u >= s for u in us[:w])
    assert br.clamp(3, 4, -10, 10) == (-3, 4)


def test_the_finding_through_the_reference():
    pgc.check_finding_reference()


# ---- 2. the kernels against the reference
def test_dp_kernel_equals_the_reference(emu):
    pgc.check_dp(emu)


def test_gap_free_sides_equal_the_fixed_open_entry(emu):
    pgc.check_gap_free(emu)


def test_tall_profiles_and_opens_that_do_not_divide(emu):
    pgc.check_tall_and_divisors(emu)


def test_seventh_plane_and_unchanged_kinds(emu):
    pgc.check_planes(emu)


# ---- 3. band
def test_banded_kernel_equals_the_reference_banded_dp(emu):
    pgc.check_kernel(emu)


def test_widths_kernel_equals_the_linear_search(emu):
    pgc.check_widths(emu)


def test_two_pass_merges_equal_the_unbanded_results(emu):
    pgc.check_two_pass_merges(emu)


def test_certified_bands_give_the_full_dp(emu):
    pgc.check_property(emu)


# ---- 4. whole MSAs
def test_msas_equal_the_reference_with_band_and_device_tree(emu):
    pgc.check_same_bytes(emu)


def test_compositions_with_collapse_seq_weights_retree_and_refine_tree(emu):
    pgc.check_compositions(emu)


def test_refine_afterwards_is_refine_ref_on_the_new_rows(emu):
    pgc.check_refine_afterwards(emu)


def test_flag_off_gives_prog_ref(emu):
    pgc.check_flag_off(emu)


def test_the_finding_on_the_device(emu):
    pgc.check_finding(emu)


def test_position_gaps_needs_progressive(emu):
    from make_prg_amd.from_msa import star_align as sa
    with pytest.raises(ValueError, match="position_gaps: only with progressive"):
        sa.star_msas(emu, [pc.records(["ACGT", "ACGA"])], position_gaps=True)


# ---- 6. status codes
def test_abi_statuses(emu):
    pgc.check_abi_statuses(emu)


# ---- 7. the command line
def test_parser(capsys):
    pgc.check_parser(capsys)


def test_from_msa_position_gaps_writes_the_reference_files(emu, tmp_path, caplog):
    pgc.check_cli(emu, tmp_path, caplog)
