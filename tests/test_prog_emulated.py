"""Progressive MSAs of `from_msa --unaligned --progressive` (make_prg_amd/from_msa/star_align.py "Progressive", csrc/k_prog.inc) on
the CPU emulation build: the spec's plain-Python statement (tests/prog_ref.py) against itself (cell form and row form, R_X = 1
against align_ref, the tree's tie rule, the invariants, S against the star MSA on the 18 loci of the issue's table), the device
entry points and whole MSAs against it, the leaf limit, the parser, and the flag-off bytes."""
import random

import numpy as np
import pytest

from make_prg_amd.from_msa import star_align as sa
from make_prg_amd.update import profile_align as pa
from tests import align_ref as ar
from tests import prog_common as pc
from tests import prog_ref as pr
from tests import refine_ref as rr
from tests import star_ref as sr
from tests.emu.backend import EmuBackend


@pytest.fixture(scope="module")
def emu():
    return EmuBackend()


def nested(merges):
    """prog_tree's merges as prog_ref.upgma's nested pairs."""
    tree = {}
    for u, v in merges:
        tree[u] = (tree.get(u, u), tree.pop(v, v))
    assert len(tree) == 1
    return next(iter(tree.values()))


def test_row_form_equals_cell_form():
    rng = random.Random(1)
    for _ in range(40):
        X = pr.random_profiles(rng, rng.choice(pc.ROWS), rng.randint(1, 30), rng.choice([0.1, 0.7]), rng.choice([0.0, 0.2]))
        Y = pr.random_profiles(rng, rng.choice(pc.ROWS), rng.randint(1, 30), rng.choice([0.1, 0.7]), rng.choice([0.0, 0.2]))
        assert pr.align_profiles(X, Y) == pr.align_profiles_np(X, Y)
    for rx, ry, w in ((1, 10, 17), (10, 9, 30), (8, 3, 5), (7, 10, 64)):      # ... and over matrices of cell codes, as the tall cases hand them in
        X, Y = pr.random_profiles(rng, rx, w + rx, 0.3, 0.2), pr.random_profiles(rng, ry, w, 0.2, 0.1)
        assert pr.align_profiles_np(pc.codes(X), pc.codes(Y)) == pr.align_profiles_np(pc.codes(X), Y) == pr.align_profiles(X, Y)


def test_one_row_x_is_the_pair_dp(emu):
    rng = random.Random(2)
    pairs = []
    for _ in range(12):
        Y = pr.random_profiles(rng, rng.choice(pc.ROWS), rng.randint(1, 90), rng.choice([0.1, 0.6]))
        seq = "".join(rng.choice("ACGTACGTN") for _ in range(rng.randint(1, 90)))
        want = ar.align_pair(Y, seq)
        assert pr.align_profiles([seq], Y) == want == pr.align_profiles_np([seq], Y)
        pairs.append(((seq,), Y, want))
    got = sa.merge_profiles(emu, [(pc.codes(x), pc.codes(y)) for x, y, _ in pairs])
    assert [(o.decode(), s) for o, s in got] == [w for _, _, w in pairs]


def test_tree_ties_resolve_by_key():
    for seqs, want in ((["ACGTAC", "TTTTTT", "ACGTAC", "TTTTTT"], ((0, 2), (1, 3))),
                       (["ACG", "ACGT", "AC", "ACGTA"], (((0, 1), 2), 3))):        # every D is 65 536
        D = pr.distances(seqs)[0]
        if len(seqs[0]) < 6:
            assert all(D[a][b] == 65536 for a in range(4) for b in range(4) if a != b)
        assert pr.upgma(D, range(4)) == want
        assert nested(sa.prog_tree(np.array(D, np.int64), list(range(4)))) == want


def test_host_tree_is_the_exact_upgma():
    """Random small-integer distances (ties everywhere) and distances whose averages differ only far behind a float's first
    digits: the host's shortlist-then-exact rule picks what the plain statement picks."""
    rng = random.Random(3)
    for n, top in ((5, 3), (9, 4), (14, 2), (12, 65536), (20, 7)):
        for _ in range(6):
            D = np.zeros((n, n), np.int64)
            for a in range(n):
                for b in range(a + 1, n):
                    D[a, b] = D[b, a] = rng.randint(0, top)
            leaves = sorted(rng.sample(range(n), rng.randint(2, n)))
            assert nested(sa.prog_tree(D, leaves)) == pr.upgma(D.tolist(), leaves)


def test_division_by_multiplication_is_exact():
    """k_prog.inc's pg_div, restated: floor(v / R) = (2 v M) >> (32 + s) for 0 <= v <= 1 280 R."""
    for R in (1, 2, 3, 5, 7, 12, 64, 100, 1000, 2047, 2048, 4095, 4096):
        s = 0 if R == 1 else (R - 1).bit_length()
        M = (1 << (31 + s)) // R + 1
        assert M < 1 << 32
        v = np.arange(0, 1280 * R + 1, dtype=np.uint64)
        assert (v << np.uint64(1)).max() < 1 << 32
        assert ((((v << np.uint64(1)) * np.uint64(M)) >> np.uint64(32 + s)) == v // np.uint64(R)).all(), R


def test_invariants_on_the_spec_loci():
    for l, (rows, (n, rounds, star)) in zip(pc.msa_loci(), pc.msa_spec()):
        assert [r.replace("-", "") for r in rows] == [sr.normalise(s) for s in l]
        assert len({len(r) for r in rows}) == 1 and all(any(r[j] != "-" for r in rows) for j in range(len(rows[0])))
        assert not star and n == sum(1 for s in l if sr.normalise(s)) and (rounds > 0) == (n > 1)
    assert pr.progressive_rows(["ACGTACGTTGCA"]) == ["ACGTACGTTGCA"]
    with pytest.raises(ValueError):
        pr.progressive_rows(["", "--"])


def test_progressive_scores_above_star_on_the_table_loci():
    for l in pr.table_loci():
        assert rr.objective(pr.progressive_rows(l)) > rr.objective(sr.star_rows(l)[1])


def test_dp_equals_the_spec(emu):
    pc.check_dp(emu)
    pc.check_dp(emu, budget_bytes=4 * pa.workspace_words(200, 300))          # one merge per launch at the top, several below


def test_tall_profiles_equal_the_spec(emu):
    pc.check_tall_dp(emu)


def test_columns_of_tall_texts(emu):
    pc.check_tall_columns(emu)


def test_planes_agree(emu):
    pc.check_planes_agree(emu)


def test_distances_equal_the_spec(emu):
    pc.check_distances(emu, sr.edge_loci() + rr.special_loci() + sr.random_loci(5, 25))


def test_msas_equal_the_spec(emu):
    pc.check_msas(emu)


def test_small_budget_and_chunks_give_the_same_msas(emu):
    pc.check_msas(emu, budget_bytes=4 * pa.workspace_words(420, 420), chunk_bytes=1 << 14)


def test_compositions_with_adjust_direction_refine_and_band(emu):
    pc.check_compositions(emu)


def test_leaf_limit_falls_back_to_the_star_bytes(emu):
    loci = sr.edge_loci() + sr.random_loci(3, 12)
    recs = [pc.records(l) for l in loci]
    info, orient = [], []
    msas = sa.star_msas(emu, recs, progressive=True, progression=info, max_leaves=3, adjust_direction=True, orientation=orient)
    star = sa.star_msas(emu, recs, adjust_direction=True)
    n_star = 0
    for l, m, s, got, o in zip(loci, msas, star, info, orient):
        n = sum(1 for x in l if sr.normalise(x))
        assert got[0] == n and got[2] == (n > 3) and len(o[0]) == len(l)
        if n > 3:
            n_star += 1
            assert sa.msa_fasta(m) == sa.msa_fasta(s) and got[1] == 0
    assert 3 <= n_star < len(loci)
    for l in loci[:12]:
        rows, (n, _, fell) = pr.progressive(l, max_leaves=3)
        assert fell == (n > 3) and (not fell or rows == sr.star_rows(l)[1])
    assert sa.PROG_MAX_LEAVES == pr.MAX_LEAVES == 4096


def test_failures_are_todays(emu):
    from make_prg_amd.subcommands.from_msa import EmptyMSAError
    with pytest.raises(EmptyMSAError):
        sa.star_msas(emu, [[]], progressive=True)
    for kw in (dict(), dict(progressive=True)):
        with pytest.raises(sa.StarAlignError, match="locus g7: every sequence is empty"):
            sa.star_msas(emu, [pc.records(["ACGT"]), pc.records(["", "--"])], names=["g1", "g7"], **kw)


def test_flag_off_bytes_are_the_star_bytes(emu):
    loci = sr.edge_loci() + sr.random_loci(9, 10)
    recs = [pc.records(l) for l in loci]
    want = [sr.star_fasta(r) for r in recs]
    assert [sa.msa_fasta(m) for m in sa.star_msas(emu, recs)] == want
    timings, info = {}, []
    assert [sa.msa_fasta(m) for m in sa.star_msas(emu, recs, progressive=False, progression=info, timings=timings)] == want
    assert info == [] and "tree_s" not in timings and "progressive_s" not in timings


def test_abi_statuses(emu):
    pc.check_abi_statuses(emu)


def test_parser(capsys):
    import argparse
    from make_prg_amd.__main__ import main
    from make_prg_amd.subcommands import from_msa
    with pytest.raises(SystemExit) as exc:
        main(["from_msa", "-i", "d", "-o", "o", "--progressive"])
    assert exc.value.code == 2 and "--progressive needs --unaligned" in capsys.readouterr().err
    p = from_msa.register_parser(argparse.ArgumentParser().add_subparsers())
    for argv, on in (([], False), (["--progressive"], True), (["--progressive", "--band", "--refine", "--adjust-direction"], True)):
        args = p.parse_args(["-i", "d", "-o", "o", "--unaligned"] + argv)
        from_msa.check_options(args, p)
        assert args.progressive is on


def test_from_msa_unaligned_progressive_hands_off_to_from_msa(emu, tmp_path, caplog):
    """from_msa.run with --unaligned --progressive (in process, on the emulation build): the MSAs written are prog_ref's, and
    every output equals from_msa's on those MSAs."""
    from argparse import Namespace
    from make_prg_amd.subcommands import from_msa
    from make_prg_amd.subcommands.output_type import OutputType
    src = tmp_path / "in"
    src.mkdir()
    want = {}
    loci = [pr.clade_locus(s, 6) for s in (0, 1)] + [["ACGTACGTTGCA", "ACGTTCGTTGCA"], ["ACGTACGTTGCA"]]
    for k, l in enumerate(loci):
        recs = [(f"s{i} x", s) for i, s in enumerate(l)]
        (src / f"g{k}.fasta").write_text("".join(f">{t}\n{s}\n" for t, s in recs))
        want[f"g{k}.fa"] = pr.progressive_fasta(recs)
    assert any(want[f"g{k}.fa"] != sr.star_fasta([(f"s{i} x", s) for i, s in enumerate(l)]) for k, l in enumerate(loci))

    def opts(**kw):
        base = dict(input=str(src), suffix="", output_prefix="", alignment_format="fasta", max_nesting=5, min_match_length=7,
                    output_type=OutputType("a"), force=False, threads=1, unaligned=True, msa_dir=None, progressive=True)
        base.update(kw)
        return Namespace(**base)
    d = tmp_path / "msas"
    from_msa.run(opts(output_prefix=str(tmp_path / "a" / "a"), msa_dir=str(d)), emu)
    assert {p.name: p.read_text() for p in d.iterdir()} == want
    from_msa.run(opts(input=str(d), output_prefix=str(tmp_path / "b" / "b"), unaligned=False, progressive=False), emu)
    for suffix in (".prg.fa", ".prg.bin.zip", ".prg.gfa.zip", ".update_DS.zip"):
        assert (tmp_path / "a" / ("a" + suffix)).read_bytes() == (tmp_path / "b" / ("b" + suffix)).read_bytes(), suffix
