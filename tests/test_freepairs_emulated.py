"""Free end pairs of `from_msa --unaligned --free-end-pairs` (star_align.py "Free end pairs", csrc/al_pairs.inc,
csrc/al_pairs_band.inc, k_align_bounds_endgap in csrc/k_align.inc) on the CPU emulation build: the plain-Python statement
(tests/freepairs_ref.py) against itself, against endgap_ref with the sequence as a one-row side, against the overlap optimum by its
definition and against align_ref / band_ref, then tests/freepairs_common.py's checks of the three new entries, the two passes of
pairs_on_device, whole loci, the flag compositions, the finding and the command line."""
import random

import pytest

from tests import align_ref as ar
from tests import band_ref as br
from tests import endgap_ref as eg
from tests import freepairs_common as fpc
from tests import freepairs_ref as fp
from tests import prog_ref as pr
from tests.emu.backend import EmuBackend


@pytest.fixture(scope="module")
def emu():
    return EmuBackend()


def _random_pair(rng, widest=30):
    R = rng.choice([1, 1, 3, 6])
    C, n = rng.randint(1, widest), rng.randint(1, widest)
    rows = pr.random_profiles(rng, R, C, rng.choice([0.1, 0.7]), 0.1) if R > 1 else ["".join(rng.choice("ACGTN") for _ in range(C))]
    return rows, "".join(rng.choice("ACGTRN") for _ in range(n))


# ---- 1. the reference against itself
def test_cell_form_row_form_endgap_ref_and_overlap_optimum_agree():
    rng = random.Random(1)
    differ = 0
    for k in range(60):
        rows, s = _random_pair(rng)
        n, C = len(s), len(rows[0])
        want = fp.align_pair(rows, s)
        assert want == fp.align_pair_np(rows, s) == fp.align_pair(rows, s, -n, C) == fp.align_pair_banded_np(rows, s, -n - 5, C + 5)
        assert want == eg.align_profiles([s], rows)                           # the spec's identity: the sequence as a one-row X
        assert want[1] == eg.overlap_score([s], rows) >= 0
        assert want[0].count("M") + want[0].count("I") == n and want[0].count("M") + want[0].count("D") == C
        band = (min(0, C - n) - rng.choice([0, 1, 2, 5, 100]), max(0, C - n) + rng.choice([0, 1, 2, 5, 100]))
        assert fp.align_pair(rows, s, *band) == fp.align_pair_banded_np(rows, s, *band) == eg.align_profiles_banded([s], rows, *band)
        differ += want != ar.align_pair(rows, s)
    assert differ >= 30


def test_flag_off_form_is_align_ref_and_band_ref():
    rng = random.Random(2)
    for k in range(30):
        rows, s = _random_pair(rng)
        n, C = len(s), len(rows[0])
        want = ar.align_pair(rows, s)
        assert fp.align_pair(rows, s, endgap=False) == fp.align_pair_np(rows, s, endgap=False) == want == ar.align_pair_np(rows, s)
        band = (min(0, C - n) - rng.choice([0, 1, 3]), max(0, C - n) + rng.choice([0, 2, 7]))
        assert fp.align_pair(rows, s, *band, endgap=False) == fp.align_pair_banded_np(rows, s, *band, endgap=False) == br.align_pair_banded(rows, s, *band)


def test_u_never_rises_and_a_band_it_certifies_gives_the_full_result():
    rng = random.Random(4)
    certified = narrow = lower = 0
    for k in range(60):
        if k % 3 == 0:
            rows, s = _random_pair(rng, 40)
        else:                                            # a sequence that does share an alignment with the profile: narrow bands are certified
            root = "".join(rng.choice("ACGT") for _ in range(rng.randint(20, 50)))
            rows = [root] if k % 3 == 1 else pr.random_profiles(rng, 4, len(root), 0.1, 0.02)
            base = rows[0].replace("-", "") or "A"
            a = rng.randint(0, len(base) // 2)
            s = fpc.sr.mutate(rng, base[a:a + rng.randint(5, len(base))], 0.03, 0.02) or "A"
        n, C = len(s), len(rows[0])
        b = fp.bounds(rows)
        us = [fp.U(*b, n, C, w) for w in range(min(n, C) + 2)]
        assert all(x >= y for x, y in zip(us, us[1:])) and us[0] <= b[0]
        assert all(fp.U(*b, n, C, w) >= fp.U_sorted(rows, n, w) for w in range(min(n, C)))
        whole = fp.align_pair_np(rows, s)
        assert whole[1] <= b[0]
        for w in range(min(n, C) + 1):
            got = fp.align_pair_banded_np(rows, s, min(0, C - n) - w, max(0, C - n) + w)
            assert got[1] <= whole[1]
            lower += got[1] < whole[1]
            if us[w] < got[1]:
                narrow += w < min(n, C)
                certified += 1
                assert got == whole, (k, w)
        x = rng.randint(us[-1] - 5, us[0] + 5)
        w = fp.wstar(*b, n, C, x)
        assert (w == min(n, C) or us[w] < x) and all(u >= x for u in us[:w])
    assert narrow >= 100 and lower >= 20, (certified, narrow, lower)


def test_host_widths_equal_the_linear_search():
    fpc.check_widths_formula()


def test_two_pass_inputs_meet_every_branch_in_the_reference_alone():
    _, kinds, helped, _ = fpc.two_pass_spec()
    assert kinds["first"] >= 3 and kinds["second"] >= 3 and kinds["full"] >= 3, kinds


def test_the_finding_through_the_reference():
    fpc.check_finding_reference()


# ---- 2. - 6. the entries
def test_dp_kernel_equals_the_reference_and_the_profile_pair_entry(emu):
    fpc.check_dp(emu)


def test_banded_kernel_equals_the_reference_banded_dp(emu):
    fpc.check_banded(emu)


def test_bounds_kernel_equals_python(emu):
    fpc.check_bounds(emu)


def test_two_passes_equal_the_unbanded_results(emu):
    fpc.check_two_pass(emu)


def test_abi_statuses(emu):
    fpc.check_abi_statuses(emu)


# ---- 7. - 9. whole loci
def test_star_msas_equal_the_reference_with_band_collapse_and_adjust_direction(emu):
    fpc.check_star(emu)


def test_refine_rounds_and_objective_are_the_references(emu):
    fpc.check_refine(emu)


def test_progressive_with_free_end_gaps_and_refine_and_the_star_fallback(emu):
    fpc.check_progressive(emu)


def test_a_unique_substring_of_the_centre_lies_in_place(emu):
    fpc.check_unique_substring(emu)


def test_flag_off_gives_star_ref_and_refine_ref(emu):
    fpc.check_flag_off(emu)


def test_the_finding_on_the_device(emu):
    fpc.check_finding(emu)


# ---- 10. the command line
def test_parser(capsys):
    fpc.check_parser(capsys)


def test_from_msa_free_end_pairs_writes_the_reference_files(emu, tmp_path, caplog):
    fpc.check_cli(emu, tmp_path, caplog)
