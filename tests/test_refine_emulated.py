"""Leave-one-out refinement of `from_msa --unaligned --refine` (make_prg_amd/from_msa/star_align.py "Refinement",
csrc/k_refine.inc) on the CPU emulation build: refined MSAs and S byte-equal to the spec's plain-Python statement
(tests/refine_ref.py), the leave-one-out profiles against mprg_align_profiles, the invariants and the S properties, six
diverged loci (refine_ref.diverged_locus, seeds 0-5), the parser's refusals and the command line."""
import random

import pytest

from make_prg_amd.from_msa import star_align as sa
from make_prg_amd.update import profile_align as pa
from tests import refine_common as rc
from tests import refine_ref as rr
from tests import star_ref as sr
from tests.emu.backend import EmuBackend


@pytest.fixture(scope="module")
def emu():
    return EmuBackend()


def spec_loci():
    return sr.edge_loci() + rr.special_loci() + sr.random_loci(3) + [rr.diverged_locus(s) for s in (0, 2)]


@pytest.fixture(scope="module")
def spec_results():
    """refine_ref on spec_loci() for N = 1, 2, 3 (shared by the tests below: the plain-Python DP takes seconds)."""
    return {n: [rr.refined_star_rows(l, n) for l in spec_loci()] for n in (1, 2, 3)}


@pytest.mark.parametrize("band", [False, True])
@pytest.mark.parametrize("n", [1, 2, 3])
def test_refined_msas_equal_the_spec(emu, spec_results, n, band):
    loci = spec_loci()
    info = []
    msas = sa.star_msas(emu, [rc.records(l) for l in loci], refine=n, refinement=info, band=band)
    assert len(info) == len(loci)
    for l, m, got, (rows, acc, trail) in zip(loci, msas, info, spec_results[n]):
        assert m.rows_as_strings() == rows, l
        assert got == (acc, trail[0], trail[-1]), l
        assert m.descriptions == [t for t, _ in rc.records(l)]
    assert sum(a for a, _, _ in info) >= 3 and max(a for a, _, _ in info) == min(n, 3)      # (rounds really are accepted, up to N)


def test_small_budget_and_chunks_give_the_same_msas(emu, spec_results):
    """Several chunks, several pair launches and several refinement groups (the budget holds one locus's profiles at most)."""
    loci = spec_loci()
    budget = 4 * pa.workspace_words(360, 420)
    for band in (False, True):
        timings = {}
        msas = sa.star_msas(emu, [rc.records(l) for l in loci], refine=2, band=band, budget_bytes=budget, timings=timings)
        assert [m.rows_as_strings() for m in msas] == [rows for rows, _, _ in spec_results[2]]
        assert timings["refine_s"] > 0 and (not band or timings["band_pairs"] > sum(len(l) - 1 for l in loci))
        msas = sa.star_msas(emu, [rc.records(l) for l in loci], refine=2, band=band, budget_bytes=budget, chunk_bytes=1)
        assert [m.rows_as_strings() for m in msas] == [rows for rows, _, _ in spec_results[2]]


def test_counts_profiles_and_compaction(emu):
    rng = random.Random(5)
    msas = [sr.star_rows(l)[1] for l in sr.edge_loci() + rr.special_loci() + sr.random_loci(8, 12)]
    msas.append(sr.star_rows(rr.diverged_locus(1))[1])                       # more than 256 columns: two tiles
    holed = []
    for m in msas:                                                           # the same MSAs with all-gap columns put in
        cuts = sorted(rng.randrange(len(m[0]) + 1) for _ in range(3))
        holed.append(["-" * (cuts[0] == 0) + "".join(ch + "-" * cuts.count(j + 1) for j, ch in enumerate(r)) for r in m])
    assert max(len(m[0]) for m in msas) > 256
    rc.check_counts_profiles_and_compaction(emu, msas + holed + [["--", "--"], ["-A-", "---", "-C-"]])


def test_leave_one_out_profile_is_the_spec_profile(emu):
    """mprg_refine_profiles against align_ref.profile of the matrix without the row, where leaving the row out makes a column
    all-gap (P = -640, Dc = 0 there)."""
    import numpy as np
    from tests import align_ref as ar
    msa = ["AC-GT", "A--GA", "ACT-T", "AN-TT"]
    d_text, nbytes, toff, R, W = rc.upload_msas(emu, [msa])
    rtab, d_counts, _, n_cols, _, _ = sa.refine_counts(emu, d_text, nbytes, toff, R, W)
    d_prof, poff, words = sa.refine_profiles(emu, d_text, nbytes, rtab, d_counts, n_cols, np.zeros(4, np.int64), np.arange(4))
    prof = emu.download(d_prof, np.int32, words).reshape(4, 6, 5)
    for r in range(4):
        P, Dc = ar.profile([x for i, x in enumerate(msa) if i != r])
        assert prof[r, :4].T.tolist() == [[p[x] for x in "ACGT"] for p in P] and prof[r, 4].tolist() == [p["N"] for p in P]
        assert prof[r, 5].tolist() == Dc
    assert prof[2, :5, 2].tolist() == [-640] * 5 and prof[2, 5, 2] == 0


def test_a_locus_too_long_for_a_round_keeps_its_msa(emu):
    """A budget that holds the star pairs (n x C) but not a realignment over the star MSA's W columns: no error, the locus is
    left as the star MSA; with room it is refined."""
    l = rr.diverged_locus(0)
    star = sr.star_rows(l)[1]
    need = pa.workspace_words(max(len(s) for s in l), len(star[0]))
    assert need > max(pa.workspace_words(len(s), len(l[sr.centre(l)])) for s in l)
    for band in (False, True):
        info = []
        msas = sa.star_msas(emu, [rc.records(l)], refine=2, refinement=info, band=band, budget_bytes=4 * (need - 64))
        assert msas[0].rows_as_strings() == star and info == [(0, rr.objective(star), rr.objective(star))]
        info = []
        sa.star_msas(emu, [rc.records(l)], refine=2, refinement=info, band=band, budget_bytes=4 * (need + 4096))
        assert info[0][0] >= 1


def test_invariants_and_objective(emu):
    loci = spec_loci() + [rr.diverged_locus(7, 6) * 2]                       # (the last one: every sequence twice)
    rng = random.Random(2)
    flipped = [[rc.revcomp(s) if i and rng.random() < 0.4 else s for i, s in enumerate(l)] for l in loci]
    for given, adjust in ((loci, False), (flipped, True)):
        recs = [rc.records(l) for l in given]
        star = sa.star_msas(emu, recs, adjust_direction=adjust)
        for band in (False, True):
            info = []
            msas = sa.star_msas(emu, recs, adjust_direction=adjust, refine=3, refinement=info, band=band)
            rc.check_invariants(given, msas, info, star)
            assert any(a for a, _, _ in info) and any(not a for a, _, _ in info)
            if adjust:
                assert any(t.startswith(sa.REVERSED_PREFIX) for m in msas for t in m.descriptions)
    # a flag that is off changes nothing, and a refused first round is the star MSA
    assert [m.rows_as_strings() for m in sa.star_msas(emu, recs, adjust_direction=True, refine=0)] == [m.rows_as_strings() for m in star]


def test_the_six_diverged_loci(emu):
    """Seeds 0-5 (refine_ref.DIVERGED_SEEDS): 12 sequences by star_ref.mutate(sub=0.06, indel=0.03) from a root of 150-300 nt.
    One round raises S on all six under the plain-Python statement; with N = 3 no locus ends below its best accepted round."""
    loci = [rr.diverged_locus(s) for s in rr.DIVERGED_SEEDS]
    want = [rr.refined_star_rows(l, 3) for l in loci]
    for rows, acc, trail in want:
        assert acc >= 1 and trail[1] > trail[0]
    for n in (1, 3):
        info = []
        msas = sa.star_msas(emu, [rc.records(l) for l in loci], refine=n, refinement=info, band=True)
        for m, got, (rows, acc, trail), l in zip(msas, info, want, loci):
            k = min(acc, n)
            assert got == (k, trail[0], trail[k]) and got[2] == max(trail[:k + 1]) > trail[0]
            if n == 3:
                assert m.rows_as_strings() == rows
            assert rr.objective(m.rows_as_strings()) == got[2]


def test_abi_statuses(emu):
    rc.check_abi_statuses(emu)


def test_refine_argument_is_checked(emu):
    for bad in (-1, 17, 1.5, True):
        with pytest.raises(ValueError, match="refine"):
            sa.star_msas(emu, [rc.records(["ACGT"])], refine=bad)


def test_parser_refusals(capsys):
    from make_prg_amd.__main__ import main
    for argv, msg in ((["from_msa", "-i", "d", "-o", "o", "--refine"], "--refine needs --unaligned"),
                      (["from_msa", "-i", "d", "-o", "o", "--unaligned", "--refine", "0"], "--refine takes 1 to 16 rounds, not 0"),
                      (["from_msa", "-i", "d", "-o", "o", "--unaligned", "--refine", "17"], "--refine takes 1 to 16 rounds, not 17"),
                      (["from_msa", "-i", "d", "-o", "o", "--unaligned", "--refine", "two"], "argument --refine: invalid int value")):
        with pytest.raises(SystemExit) as exc:
            main(argv)
        assert exc.value.code == 2
        assert msg in capsys.readouterr().err


def test_parser_accepts_the_flag():
    import argparse
    from make_prg_amd.subcommands import from_msa
    sub = argparse.ArgumentParser().add_subparsers()
    p = from_msa.register_parser(sub)
    for argv, n in ((["--refine"], 2), (["--refine", "5"], 5), ([], None), (["--refine", "--band"], 2)):
        args = p.parse_args(["-i", "d", "-o", "o", "--unaligned"] + argv)
        from_msa.check_options(args, p)
        assert args.refine == n


def test_from_msa_unaligned_refine_hands_off_to_from_msa(emu, tmp_path):
    """from_msa.run with --unaligned --refine (in process, on the emulation build): the MSAs written are the spec's refined ones
    (some of them changed by it), and every output equals from_msa's on those MSAs."""
    from argparse import Namespace
    from make_prg_amd.subcommands import from_msa
    from make_prg_amd.subcommands.output_type import OutputType
    src = tmp_path / "in"
    src.mkdir()
    want, changed = {}, 0
    loci = [rr.diverged_locus(s, 6) for s in (0, 1, 2)] + [["ACGTACGTTGCA", "ACGTTCGTTGCA"]]
    for k, l in enumerate(loci):
        recs = [(f"s{i} x", s) for i, s in enumerate(l)]
        (src / f"g{k}.fasta").write_text("".join(f">{t}\n{s}\n" for t, s in recs))
        rows, acc, _ = rr.refined_star_rows(l, 2)
        changed += acc > 0
        want[f"g{k}.fa"] = "".join(f">{t}\n{r}\n" for (t, _), r in zip(recs, rows))
    assert changed >= 1

    def opts(**kw):
        base = dict(input=str(src), suffix="", output_prefix="", alignment_format="fasta", max_nesting=5, min_match_length=7,
                    output_type=OutputType("a"), force=False, threads=1, unaligned=True, msa_dir=None, refine=2)
        base.update(kw)
        return Namespace(**base)
    d = tmp_path / "msas"
    from_msa.run(opts(output_prefix=str(tmp_path / "a" / "a"), msa_dir=str(d)), emu)
    assert {p.name: p.read_text() for p in d.iterdir()} == want
    from_msa.run(opts(input=str(d), output_prefix=str(tmp_path / "b" / "b"), unaligned=False, refine=None), emu)
    for suffix in (".prg.fa", ".prg.bin.zip", ".prg.gfa.zip", ".update_DS.zip"):
        assert (tmp_path / "a" / ("a" + suffix)).read_bytes() == (tmp_path / "b" / ("b" + suffix)).read_bytes(), suffix
    d2 = tmp_path / "msas_band"
    from_msa.run(opts(output_prefix=str(tmp_path / "c" / "c"), msa_dir=str(d2), band=True), emu)
    assert {p.name: p.read_text() for p in d2.iterdir()} == want
