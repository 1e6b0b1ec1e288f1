"""`from_msa --unaligned --collapse-identical` (make_prg_amd/from_msa/star_align.py "Collapse", csrc/k_collapse.inc) on the CPU
emulation build: the spec's plain-Python statement (tests/collapse_ref.py) against prog_ref where they must agree, the two device
entry points called directly, whole MSAs against the statement and against the flag-off run, the parser and the command."""
import random

import numpy as np
import pytest

from make_prg_amd.from_msa import star_align as sa
from tests import collapse_common as cc
from tests import collapse_ref as cr
from tests import prog_ref as pr
from tests import star_ref as sr
from tests.emu.backend import EmuBackend


@pytest.fixture(scope="module")
def emu():
    return EmuBackend()


def nested(merges):
    tree = {}
    for u, v in merges:
        tree[u] = (tree.get(u, u), tree.pop(v, v))
    assert len(tree) == 1
    return next(iter(tree.values()))


def test_reference_without_duplicates_is_prog_ref():
    for l in pr.table_loci()[::5] + [l for l in sr.edge_loci() if len({sr.normalise(s) for s in l}) == len(l)]:
        rows, info, merges = cr.progressive(l)
        assert (rows, info) == pr.progressive(l) and merges == info[0] - 1


def test_weighted_tree_is_the_tree_of_the_copies():
    """prog_tree with weights and collapse_ref.upgma against prog_ref.upgma on the leaves written w times: the same tree once the
    copies (which join first, at distance 0, by key) are folded back into their leaf."""
    rng = random.Random(5)
    for n, top in ((4, 3), (6, 9), (7, 65536), (9, 2)):
        for _ in range(5):
            D = np.zeros((n, n), np.int64)
            for a in range(n):
                for b in range(a + 1, n):
                    D[a, b] = D[b, a] = rng.randint(1, top)
            w = [rng.randint(1, 4) for _ in range(n)]
            got = nested(sa.prog_tree(D, list(range(n)), np.array(w)))
            assert got == cr.upgma(D.tolist(), range(n), w)
            assert nested(sa.prog_tree(D, list(range(n)), np.ones(n, np.int64))) == nested(sa.prog_tree(D, list(range(n)))) == pr.upgma(D.tolist(), range(n))


def test_identical_classes(emu):
    cc.check_identical(emu)


def test_identical_refusals(emu):
    cc.check_identical_refusals(emu)


def test_weighted_columns(emu):
    cc.check_weighted_columns(emu)


def test_weighted_columns_refusals(emu):
    cc.check_weighted_refusals(emu)


def test_star_bytes_are_the_flag_off_bytes(emu):
    cc.check_star(emu)


def test_progressive_equals_the_spec(emu):
    cc.check_progressive(emu)


def test_progressive_with_a_small_budget(emu):
    from make_prg_amd.update import profile_align as pa
    recs = [cc.pc.records(l) for l in cc.loci()]
    msas = sa.star_msas(emu, recs, progressive=True, collapse=True, budget_bytes=4 * pa.workspace_words(420, 420), chunk_bytes=1 << 14)
    assert [m.rows_as_strings() for m in msas] == [rows for rows, _, _ in cc.spec()]


def test_adjust_direction(emu):
    cc.check_adjust_direction(emu)


def test_leaf_limit_counts_records(emu):
    cc.check_leaf_limit(emu)


def test_flag_off_launches_nothing_new(emu):
    recs = [cc.pc.records(l) for l in cc.loci()[:3]]
    for kw in (dict(), dict(progressive=True)):
        timings = {}
        sa.star_msas(emu, recs, timings=timings, **kw)
        assert not [k for k in timings if k.startswith("collapse")]


def test_parser(capsys):
    import argparse
    from make_prg_amd.__main__ import main
    from make_prg_amd.subcommands import from_msa
    with pytest.raises(SystemExit) as exc:
        main(["from_msa", "-i", "d", "-o", "o", "--collapse-identical"])
    assert exc.value.code == 2 and "--collapse-identical needs --unaligned" in capsys.readouterr().err
    p = from_msa.register_parser(argparse.ArgumentParser().add_subparsers())
    for argv, on in (([], False), (["--collapse-identical"], True),
                     (["--collapse-identical", "--progressive", "--band", "--refine", "--adjust-direction"], True)):
        args = p.parse_args(["-i", "d", "-o", "o", "--unaligned"] + argv)
        from_msa.check_options(args, p)
        assert args.collapse_identical is on


def test_from_msa_unaligned_collapse_writes_the_spec_msas(emu, tmp_path):
    from argparse import Namespace
    from make_prg_amd.subcommands import from_msa
    from make_prg_amd.subcommands.output_type import OutputType
    src = tmp_path / "in"
    src.mkdir()
    want = cc.write_inputs(src)

    def opts(**kw):
        base = dict(input=str(src), suffix="", output_prefix="", alignment_format="fasta", max_nesting=5, min_match_length=7,
                    output_type=OutputType("a"), force=False, threads=1, unaligned=True, msa_dir=None, progressive=True, collapse_identical=True)
        base.update(kw)
        return Namespace(**base)
    d = tmp_path / "msas"
    from_msa.run(opts(output_prefix=str(tmp_path / "a" / "a"), msa_dir=str(d)), emu)
    assert {p.name: p.read_text() for p in d.iterdir()} == want
    d2 = tmp_path / "star"
    from_msa.run(opts(output_prefix=str(tmp_path / "b" / "b"), msa_dir=str(d2), progressive=False), emu)
    d3 = tmp_path / "star_off"
    from_msa.run(opts(output_prefix=str(tmp_path / "c" / "c"), msa_dir=str(d3), progressive=False, collapse_identical=False), emu)
    assert {p.name: p.read_text() for p in d2.iterdir()} == {p.name: p.read_text() for p in d3.iterdir()} != want
