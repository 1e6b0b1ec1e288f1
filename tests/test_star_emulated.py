"""Centre-star MSAs of `from_msa --unaligned` (make_prg_amd/from_msa/star_align.py, csrc/k_star.inc) on the CPU emulation build:
centres and MSAs byte-equal to the spec's plain-Python statement (tests/star_ref.py), the spec's invariants, its quality on
synthetic loci of known alignment, the merge and centre entries called directly on hand-built tables (tests/star_common.py), and the
command line's refusals."""
import random

import numpy as np
import pytest

from make_prg_amd.from_msa import star_align as sa
from tests import align_ref as ar
from tests import star_common as sc
from tests import star_ref as sr
from tests.emu.backend import EmuBackend


@pytest.fixture(scope="module")
def emu():
    return EmuBackend()


def records(seqs):
    return [(f"r{i} desc {i}", s) for i, s in enumerate(seqs)]


def test_centres_and_msas_equal_the_spec(emu):
    loci = sr.edge_loci() + sr.random_loci(3)
    codes = [sa.locus_codes(str(i), records(l)) for i, l in enumerate(loci)]
    got_c = sa.centres(emu, codes).tolist()
    msas = sa.star_msas(emu, [records(l) for l in loci])
    for l, c, m in zip(loci, got_c, msas):
        want_c, want_rows = sr.star_rows(l)
        assert c == want_c, l
        assert m.rows_as_strings() == want_rows, l
        assert m.descriptions == [t for t, _ in records(l)] and m.ids == [f"r{i}" for i in range(len(l))]


def test_merge_entries_on_hand_built_ops(emu):
    sc.check_merge(emu)


def test_merge_entries_refuse_bad_rows_and_loci(emu):
    sc.check_merge_statuses(emu)


def test_centre_entries_directly(emu):
    sc.check_centres(emu)


def test_small_chunks_and_budget_give_the_same_msas(emu):
    loci = [records(l) for l in sr.random_loci(4, 12)]
    whole = [m.rows_as_strings() for m in sa.star_msas(emu, loci)]
    small = sa.star_msas(emu, loci, budget_bytes=4 * pa_words(200, 160), chunk_bytes=1)
    assert [m.rows_as_strings() for m in small] == whole


def pa_words(n, C):
    from make_prg_amd.update.profile_align import workspace_words
    return workspace_words(n, C)


def test_score_ties_take_the_smallest_index():
    assert sr.centre(["ACGTAC", "TTTTTT", "ACGTAC", "TTTTTT"]) == 0
    assert sr.centre(["", "TTTTTT", "ACGTAC"]) == 1
    assert sr.centre(["ACG", "ACGT"]) == 0
    assert sr.scores(["ACGTACGT", "ACGTACGT", "TTTTTTTT"]) == [3, 3, 0]


def test_input_errors(emu):
    from make_prg_amd.subcommands.from_msa import EmptyMSAError
    with pytest.raises(sa.StarAlignError, match=r"locus geneX, record 2 \(b\).*'X'"):
        sa.star_msas(emu, [[("a", "ACGT"), ("b", "ACXT")]], names=["geneX"])
    with pytest.raises(EmptyMSAError, match="geneY"):
        sa.star_msas(emu, [[]], names=["geneY"])
    with pytest.raises(sa.StarAlignError, match="geneZ: every sequence is empty"):
        sa.star_msas(emu, [[("a", "--"), ("b", "")]], names=["geneZ"])


def test_invariants_on_the_spec():
    rng = random.Random(9)
    for seqs in sr.edge_loci() + sr.random_loci(5, 60):
        _, rows = sr.star_rows(seqs)
        norm = [sr.normalise(s) for s in seqs]
        for r, s in zip(rows, norm):
            assert r.replace("-", "") == s
        assert len({len(r) for r in rows}) == 1
        assert all(any(r[j] != "-" for r in rows) for j in range(len(rows[0])))
        for a in range(len(norm)):
            for b in range(len(norm)):
                if norm[a] == norm[b]:
                    assert rows[a] == rows[b]
    for _ in range(40):
        L = rng.randint(2, 120)
        s = "".join(rng.choice("ACGT") for _ in range(L))
        p = rng.randrange(L)
        t = s[:p] + rng.choice([x for x in "ACGT" if x != s[p]]) + s[p + 1:]
        _, rows = sr.star_rows([s, t])
        assert rows == [s, t]
        ops, score = ar.align_pair([s], t)
        assert ops == "M" * L and score >= (L - 1) * 1280 - 576


def test_quality_on_config_c_shaped_loci():
    """The star alignment of config-C-shaped loci with their gaps removed recovers most of the true alignment's residue pairs
    (each row against the centre row).  Measured: 0.9991 on this subset, 0.9996 over all rows of seeds 0-7;
    asserted with margin."""
    hit = tot = 0
    for true_rows, seqs in sr.synthetic_loci(range(2)):
        sub = list(range(0, len(seqs), 8))                        # every 8th row: ~13 rows, the CPU DP stays in seconds
        c, rows = sr.star_rows([seqs[i] for i in sub])
        h, t = sr.pair_recovery([true_rows[i] for i in sub], rows, c)
        hit, tot = hit + h, tot + t
    assert tot > 10_000
    assert hit / tot >= 0.99, hit / tot


def test_parser_refusals(capsys):
    from make_prg_amd.__main__ import main
    for argv, msg in ((["from_msa", "-i", "d", "-o", "o", "-f", "stockholm", "--unaligned"], "--unaligned"),
                      (["from_msa", "-i", "d", "-o", "o", "--msa-dir", "m"], "--msa-dir")):
        with pytest.raises(SystemExit) as exc:
            main(argv)
        assert exc.value.code == 2
        assert msg in capsys.readouterr().err


def test_unaligned_reader_and_writer(tmp_path):
    import gzip
    (tmp_path / "a.fa.gz").write_bytes(gzip.compress(b">x one\nAC GT\nac\n>y\n\n>z two  \nA-C\n"))
    recs = sa.read_unaligned(tmp_path / "a.fa.gz")
    assert recs == [("x one", "ACGTac"), ("y", ""), ("z two", "A-C")]
    from make_prg_amd.msa import MSA
    m = MSA.from_strings(["AC", "-C"], ids=["x", "y"], descriptions=["x one", "y"])
    assert sa.msa_fasta(m) == ">x one\nAC\n>y\n-C\n"


def test_from_msa_unaligned_hands_off_to_from_msa(emu, tmp_path):
    """from_msa.run with --unaligned (in process, on the emulation build): the MSAs written are the spec's, and every output equals
    from_msa's on those MSAs; an existing MSA is not overwritten without -F; two inputs of one locus name are refused."""
    from argparse import Namespace
    from make_prg_amd.subcommands import from_msa
    from make_prg_amd.subcommands.output_type import OutputType
    from make_prg_amd.utils.synthetic import synth_rows
    src = tmp_path / "in"
    src.mkdir()
    want = {}
    for seed in range(3):
        recs = [(f"s{i} x", r.decode().replace("-", "")) for i, r in enumerate(synth_rows(seed, 6, 90, 2))]
        (src / f"g{seed}.fasta").write_text("".join(f">{t}\n{s}\n" for t, s in recs))
        want[f"g{seed}"] = sr.star_fasta(recs)

    def opts(**kw):
        base = dict(input=str(src), suffix="", output_prefix="", alignment_format="fasta", max_nesting=5, min_match_length=7,
                    output_type=OutputType("a"), force=False, threads=1, unaligned=True, msa_dir=None)
        base.update(kw)
        return Namespace(**base)
    d = tmp_path / "msas"
    from_msa.run(opts(output_prefix=str(tmp_path / "a" / "a"), msa_dir=str(d)), emu)
    assert {p.name: p.read_text() for p in d.iterdir()} == {f"{l}.fa": t for l, t in want.items()}
    from_msa.run(opts(input=str(d), output_prefix=str(tmp_path / "b" / "b"), unaligned=False), emu)
    for suffix in (".prg.fa", ".prg.bin.zip", ".prg.gfa.zip", ".update_DS.zip"):
        assert (tmp_path / "a" / ("a" + suffix)).read_bytes() == (tmp_path / "b" / ("b" + suffix)).read_bytes(), suffix
    with pytest.raises(RuntimeError, match="already exists"):
        from_msa.run(opts(output_prefix=str(tmp_path / "c" / "c"), msa_dir=str(d)), emu)
    from_msa.run(opts(output_prefix=str(tmp_path / "e" / "e")), emu)
    assert sorted(p.name for p in (tmp_path / "e").iterdir()) == ["e.prg.bin.zip", "e.prg.fa", "e.prg.gfa.zip", "e.update_DS.zip"]
    (src / "g0.fa").write_text(">a\nACGT\n")
    with pytest.raises(ValueError, match="same locus name g0"):
        from_msa.run(opts(output_prefix=str(tmp_path / "f" / "f")), emu)
