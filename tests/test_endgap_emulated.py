"""Free end gaps of `from_msa --unaligned --progressive --free-end-gaps` (star_align.py "Free end gaps", csrc/pg_pairs.inc,
csrc/pg_pairs_band.inc, csrc/pg_band_widths.inc) on the CPU emulation build: the plain-Python statement (tests/endgap_ref.py)
against itself, against the overlap optimum by its definition and against prog_ref / posgap_ref, then tests/endgap_common.py's
checks of the five new entries, the two-pass host passes, whole MSAs, the flag compositions, the finding and the command line."""
import random

import pytest

from tests import collapse_ref as cr
from tests import endgap_common as egc
from tests import endgap_ref as eg
from tests import posgap_ref as pg
from tests import prog_common as pc
from tests import prog_ref as pr
from tests.emu.backend import EmuBackend

OPENS = pytest.mark.parametrize("posgap", [False, True], ids=["fixed", "posgap"])


@pytest.fixture(scope="module")
def emu():
    return EmuBackend()


def _random_pair(rng, widest=30):
    X = pr.random_profiles(rng, rng.choice(pc.ROWS), rng.randint(1, widest), rng.choice([0.1, 0.7]), rng.choice([0.0, 0.2]))
    Y = pr.random_profiles(rng, rng.choice(pc.ROWS), rng.randint(1, widest), rng.choice([0.1, 0.7]), rng.choice([0.0, 0.2]))
    return X, Y


# ---- 1. the reference against itself
@OPENS
def test_cell_form_row_form_overlap_optimum_and_whole_band_agree(posgap):
    rng = random.Random(1)
    differ = 0
    for k in range(40):
        X, Y = _random_pair(rng)
        n, C = len(X[0]), len(Y[0])
        want = eg.align_profiles(X, Y, posgap)
        assert want == eg.align_profiles_np(X, Y, posgap=posgap) == eg.align_profiles_banded(X, Y, -n, C, posgap)
        assert want == eg.align_profiles_banded_np(X, Y, -n - 5, C + 5, posgap)
        assert want[1] == eg.overlap_score(X, Y, posgap) >= 0
        assert want[0].count("M") + want[0].count("I") == n and want[0].count("M") + want[0].count("D") == C
        band = (min(0, C - n) - rng.choice([0, 1, 2, 5, 100]), max(0, C - n) + rng.choice([0, 1, 2, 5, 100]))
        assert eg.align_profiles_banded(X, Y, *band, posgap) == eg.align_profiles_banded_np(X, Y, *band, posgap)
        differ += want != (pg.align_profiles(X, Y) if posgap else pr.align_profiles(X, Y))
    assert differ >= 20
    assert eg.align_profiles(("", ""), ("ACG-", "AC-T"), posgap) == ("DDDD", 0)           # n = 0: C D ops, score 0


@OPENS
def test_flag_off_form_is_prog_ref_and_posgap_ref(posgap):
    rng = random.Random(2)
    for k in range(25):
        X, Y = _random_pair(rng)
        want = pg.align_profiles(X, Y) if posgap else pr.align_profiles(X, Y)
        assert eg.align_profiles(X, Y, posgap, endgap=False) == eg.align_profiles_np(X, Y, posgap=posgap, endgap=False) == want
        assert want == (pg.align_profiles_np(X, Y) if posgap else pr.align_profiles_np(X, Y))


@OPENS
def test_weighted_form_equals_the_expanded_rows(posgap):
    rng = random.Random(3)
    for k in range(20):
        X, Y = _random_pair(rng)
        wx, wy = [rng.randint(1, 5) for _ in X], [rng.randint(1, 5) for _ in Y]
        ex, ey = cr.expanded(X, wx), cr.expanded(Y, wy)
        assert eg.align_profiles_np(X, Y, wx, wy, posgap=posgap) == eg.align_profiles_np(ex, ey, posgap=posgap) == eg.align_profiles(ex, ey, posgap)


@OPENS
def test_u_never_rises_and_a_band_it_certifies_gives_the_full_result(posgap):
    rng = random.Random(4)
    certified = narrow = 0
    for k in range(40):
        g = (0.1, 0.7)[k % 2]
        if k % 4 < 2:
            X = pr.random_profiles(rng, rng.choice(pc.ROWS), rng.randint(2, 40), g)
            Y = pr.random_profiles(rng, rng.choice(pc.ROWS), rng.randint(2, 40), g)
        else:                                            # sides that do share an alignment: some band below min(n, C) is certified
            rows = pr.random_profiles(rng, 6, rng.randint(20, 40), g)
            X, Y = [tuple(pr.progressive_rows([r.replace("-", "") or "A" for r in part])) for part in (rows[:2], rows[2:])]
        n, C = len(X[0]), len(Y[0])
        SB, loss = eg.bounds(X, Y)
        us = [eg.U(SB, loss, n, C, w) for w in range(min(n, C) + 2)]
        assert all(a >= b for a, b in zip(us, us[1:])) and us[0] <= SB
        whole = eg.align_profiles_np(X, Y, posgap=posgap)
        for w in range(min(n, C) + 1):
            got = eg.align_profiles_banded_np(X, Y, min(0, C - n) - w, max(0, C - n) + w, posgap)
            assert got[1] <= whole[1]
            narrow += got[1] < whole[1]
            if us[w] < got[1]:
                certified += w < min(n, C)
                assert got == whole, (k, w)
        s = rng.randint(us[-1] - 5, us[0] + 5)
        w = eg.wstar(SB, loss, n, C, s)
        assert (w == min(n, C) or us[w] < s) and all(u >= s for u in us[:w])
    assert certified >= 20 and narrow >= 20, (certified, narrow)


def test_the_finding_through_the_reference():
    egc.check_finding_reference()


# ---- 2. the kernels against the reference
@OPENS
def test_dp_kernel_equals_the_reference(emu, posgap):
    egc.check_dp(emu, posgap)


@OPENS
def test_tall_profiles(emu, posgap):
    egc.check_tall(emu, posgap)


# ---- 3. band
@OPENS
def test_banded_kernel_equals_the_reference_banded_dp(emu, posgap):
    egc.check_kernel(emu, posgap)


def test_widths_kernel_equals_the_linear_search(emu):
    egc.check_widths(emu)


@OPENS
def test_two_pass_merges_equal_the_unbanded_results(emu, posgap):
    egc.check_two_pass_merges(emu, posgap)


# ---- 6. whole MSAs
@OPENS
def test_msas_equal_the_reference_with_band_and_device_tree(emu, posgap):
    egc.check_same_bytes(emu, posgap)


@OPENS
def test_compositions_with_collapse_seq_weights_retree_refine_tree_and_large_loci(emu, posgap):
    egc.check_compositions(emu, posgap)


@OPENS
def test_refine_afterwards_is_refine_ref_on_the_new_rows(emu, posgap):
    egc.check_refine_afterwards(emu, posgap)


def test_flag_off_gives_prog_ref(emu):
    egc.check_flag_off(emu)


def test_the_finding_on_the_device(emu):
    egc.check_finding(emu)


def test_free_end_gaps_needs_progressive(emu):
    from make_prg_amd.from_msa import star_align as sa
    with pytest.raises(ValueError, match="free_end_gaps: only with progressive"):
        sa.star_msas(emu, [pc.records(["ACGT", "ACGA"])], free_end_gaps=True)


# ---- 8. status codes
def test_abi_statuses(emu):
    egc.check_abi_statuses(emu)


# ---- 9. the command line
def test_parser(capsys):
    egc.check_parser(capsys)


def test_from_msa_free_end_gaps_writes_the_reference_files(emu, tmp_path, caplog):
    egc.check_cli(emu, tmp_path, caplog)
