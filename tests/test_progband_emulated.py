"""Banded profile-profile merges of `from_msa --unaligned --progressive --band` (star_align.py "Progressive, band",
csrc/k_prog_band.inc) on the CPU emulation build: the plain-Python statement (tests/progband_ref.py) against itself and against
prog_ref and band_ref, then tests/progband_common.py's checks of the two device entries, the two-pass host passes, whole MSAs, the
flag compositions and the command line."""
import logging
import random

import pytest

from make_prg_amd.from_msa import star_align as sa
from tests import band_ref as br
from tests import prog_common as pc
from tests import prog_ref as pr
from tests import progband_common as pbc
from tests import progband_ref as pbr
from tests.emu.backend import EmuBackend


@pytest.fixture(scope="module")
def emu():
    return EmuBackend()


def test_row_form_equals_cell_form_and_the_full_band_is_the_full_dp():
    rng = random.Random(1)
    for k in range(40):
        X = pr.random_profiles(rng, rng.choice(pc.ROWS), rng.randint(1, 30), rng.choice([0.1, 0.7]), rng.choice([0.0, 0.2]))
        Y = pr.random_profiles(rng, rng.choice(pc.ROWS), rng.randint(1, 30), rng.choice([0.1, 0.7]), rng.choice([0.0, 0.2]))
        n, C = len(X[0]), len(Y[0])
        band = (min(0, C - n) - rng.choice([0, 1, 2, 5, 100]), max(0, C - n) + rng.choice([0, 1, 2, 5, 100]))
        assert pbr.align_profiles_banded(X, Y, *band) == pbr.align_profiles_banded_np(X, Y, *band)
        assert pbr.align_profiles_banded(X, Y, -n, C) == pr.align_profiles(X, Y)


def test_one_row_acgt_x_is_the_pair_certificate_in_its_sorted_form():
    """R_X = 1 over ACGT: every ins_i is 640, so U(w) is band_ref's ub_plus / ub_minus(sorted_sum=True) on both sides, and the
    banded DP is band_ref's."""
    rng = random.Random(2)
    for _ in range(12):
        Y = pr.random_profiles(rng, rng.choice(pc.ROWS), rng.randint(2, 60), rng.choice([0.1, 0.6]))
        seq = "".join(rng.choice("ACGT") for _ in range(rng.randint(2, 60)))
        n, C = len(seq), len(Y[0])
        SB, loss, ins = pbr.bounds([seq], Y)
        assert (SB, loss) == br.bounds(Y) and ins == [640] * n
        for w in range(min(n, C)):
            dlo, dhi = min(0, C - n) - w, max(0, C - n) + w
            u = pbr.U(SB, loss, ins, n, C, w)
            assert u == br.ub_plus(SB, loss, n, C, dhi + 1, sorted_sum=True) == br.ub_minus(SB, loss, n, C, dlo - 1, sorted_sum=True)
        band = br.band(n, C, 3, 5)
        assert pbr.align_profiles_banded([seq], Y, *band) == br.align_pair_banded(Y, seq, *band)


def test_u_does_not_rise_and_wstar_is_its_first_crossing():
    rng = random.Random(3)
    for X, Y in pbc.width_cases():
        n, C = len(X[0]), len(Y[0])
        SB, loss, ins = pbr.bounds(X, Y)
        assert 0 <= loss[0] and loss[-1] <= 1920 and 0 <= ins[0] and ins[-1] <= 640
        us = [pbr.U(SB, loss, ins, n, C, w) for w in range(min(n, C) + 1)]
        assert all(a >= b for a, b in zip(us, us[1:]))
        for _ in range(5):
            s = rng.randint(us[-1] - 5, us[0] + 5)
            w = pbr.wstar(SB, loss, ins, n, C, s)
            assert (w == min(n, C) or us[w] < s) and all(u >= s for u in us[:w])


def test_banded_kernel_equals_the_reference_banded_dp(emu):
    pbc.check_kernel(emu)


def test_widths_kernel_equals_the_linear_search(emu):
    pbc.check_widths(emu)


def test_two_pass_merges_equal_the_unbanded_results(emu):
    pbc.check_two_pass_merges(emu)


def test_tall_profiles_equal_the_unbanded_results(emu):
    pc.check_tall_dp(emu, band=True)


def test_msas_and_counters_equal_the_references(emu):
    pbc.check_msas(emu)


def test_compositions_with_adjust_direction_and_refine(emu):
    pbc.check_compositions(emu)


def test_certified_bands_give_the_full_dp(emu):
    pbc.check_property(emu)


def test_abi_statuses(emu):
    pbc.check_abi_statuses(emu)


def test_the_four_entries_of_the_sweep_agree_on_a_one_row_x(emu):
    pbc.check_forms_agree(emu)


def test_constants_and_a_negative_half_width():
    assert sa.PROG_BAND_W0 == pbr.W0 == 64 and sa.PG_BAND_PAIR_FIELDS == 8
    with pytest.raises(sa.StarAlignError, match="negative half-width"):
        list(sa._prog_groups(*[__import__("numpy").array([5])] * 2, sa._Merge(-1, 1 << 20)))


def test_from_msa_unaligned_progressive_band_writes_the_same_files_and_logs_the_counters(emu, tmp_path, caplog):
    """from_msa.run with --unaligned --progressive --band (in process, on the emulation build): the MSAs written are prog_ref's,
    and the log has the line of the banded merges' counters; with --progressive alone it has not."""
    from argparse import Namespace
    from make_prg_amd.subcommands import from_msa
    from make_prg_amd.subcommands.output_type import OutputType
    src = tmp_path / "in"
    src.mkdir()
    want = {}
    loci = pbc.near_loci() + [pr.clade_locus(0, 6), ["ACGTACGTTGCA", "ACGTTCGTTGCA"], ["ACGTACGTTGCA"]]
    for k, l in enumerate(loci):
        recs = [(f"s{i} x", s) for i, s in enumerate(l)]
        (src / f"g{k}.fasta").write_text("".join(f">{t}\n{s}\n" for t, s in recs))
        want[f"g{k}.fa"] = pr.progressive_fasta(recs)

    def opts(**kw):
        base = dict(input=str(src), suffix="", output_prefix="", alignment_format="fasta", max_nesting=5, min_match_length=7,
                    output_type=OutputType("a"), force=False, threads=1, unaligned=True, msa_dir=None, progressive=True)
        base.update(kw)
        return Namespace(**base)
    merges = sum(len(l) - 1 for l in loci)
    for band in (True, False):
        caplog.clear()
        d = tmp_path / f"msas{band}"
        with caplog.at_level(logging.INFO):
            from_msa.run(opts(output_prefix=str(tmp_path / f"o{band}" / "a"), msa_dir=str(d), band=band), emu)
        assert {p.name: p.read_text() for p in d.iterdir()} == want
        lines = [r.getMessage() for r in caplog.records if "--progressive --band:" in r.getMessage()]
        assert len(lines) == (1 if band else 0)
        if band:
            assert f"--progressive --band: {merges} merges, " in lines[0] and " DP cells computed" in lines[0]
