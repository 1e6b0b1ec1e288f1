"""`from_msa --unaligned --adjust-direction` (the Orientation step of make_prg_amd/from_msa/star_align.py; k_star_kmer_centre_canonical,
k_star_strand, k_star_revcomp in csrc/k_star.inc) on the CPU emulation build: every intermediate and the MSAs byte-equal to the
spec's plain-Python statement (tests/strand_ref.py), the spec's properties P1-P4 on the statement and through the kernels, the
recovery of known orientations on config-C-shaped loci, and the refusals."""
import random

import numpy as np
import pytest

from make_prg_amd.from_msa import star_align as sa
from tests import star_ref as sr
from tests import strand_ref as st
from tests.emu.backend import EmuBackend


@pytest.fixture(scope="module")
def emu():
    return EmuBackend()


def records(seqs):
    return [(f"r{i} desc {i}", s) for i, s in enumerate(seqs)]


def codes_of(loci):
    return [sa.locus_codes(str(i), records(l)) for i, l in enumerate(loci)]


def as_text(codes):
    return sa._ASCII[codes].tobytes().decode()


def mixed_loci(seed, n_random=30):
    """Edge loci as they are, and random loci (some with N runs: star_ref.random_loci) with a random half of ALL records flipped."""
    rng = random.Random(seed)
    return sr.edge_loci() + st.strand_edge_loci() + [st.flip(rng, l, keep_first=False)[0] for l in sr.random_loci(seed, n_random)]


def test_kernels_and_msas_equal_the_spec(emu):
    loci = mixed_loci(3)
    codes = codes_of(loci)
    norm = [[sr.normalise(s) for s in l] for l in loci]
    cent = sa.canonical_centres(emu, codes).tolist()
    assert cent == [st.canonical_centre(l) for l in norm]
    # the triples against the centre AS STORED, for every sequence of the locus (the centre and empty ones included)
    ev = sa.strand_evidence(emu, codes, cent)
    assert ev.tolist() == [list(st.evidence(l[c], s)) for l, c in zip(norm, cent) for s in l]
    # the reverse complements, written by the device into the tail of the same buffer
    flat = [c for cs in codes for c in cs]
    total = sum(len(c) for c in flat)
    off = np.concatenate([[0], np.cumsum([len(c) for c in flat])]).astype(np.int64)
    d = emu.upload(np.concatenate(flat + [np.zeros(total, np.uint8)]))
    sa.revcomp_on_device(emu, d, 2 * total, np.stack([off[:-1], np.diff(off), total + off[:-1]], 1))
    got = emu.download(d, np.uint8, 2 * total)
    assert got[:total].tobytes() == np.concatenate(flat).tobytes()
    for c, o in zip(flat, off[:-1]):
        assert as_text(got[total + o:total + o + len(c)]) == st.rc(as_text(c))
        assert np.array_equal(sa.revcomp(c), got[total + o:total + o + len(c)])
    # decisions and MSAs
    ori = []
    msas = sa.star_msas(emu, [records(l) for l in loci], adjust_direction=True, orientation=ori)
    assert sa.orientations(emu, codes) == ori
    hows = ""
    for l, m, (rev, how) in zip(loci, msas, ori):
        want_rev, want_how, _, want_rows = st.star_rows(l)
        assert (rev, how) == (want_rev, want_how), l
        assert m.rows_as_strings() == want_rows, l
        assert m.descriptions == st.titles(records(l), want_rev), l
        assert m.ids == [("_R_" if f else "") + f"r{i}" for i, f in enumerate(want_rev)]
        assert sa.msa_fasta(m) == st.star_fasta(records(l))
        hows += how
    assert all(hows.count(h) >= 3 for h in "-kdt"), {h: hows.count(h) for h in "-kdt"}     # every way of deciding occurs
    assert sum(any(rev) for rev, _ in ori) >= 20


def test_rc6_and_canonical_counts():
    k = np.arange(4096)
    assert np.array_equal(st.rc6(st.rc6(k)), k)
    for s in ("ACGTTG", "AAAAAA", "GATTACA" * 3):
        assert st.kmers(st.rc(s)).tolist() == st.rc6(st.kmers(s))[::-1].tolist()
        assert np.array_equal(st.canonical_counts(s), st.canonical_counts(st.rc(s)))
    assert st.rc("ACGTRYKMSWN") == "NWSKMRYACGT"


def check_p4(seqs, rev, rows):
    norm = [sr.normalise(s) for s in seqs]
    first = next(a for a, s in enumerate(norm) if s)
    assert not rev[first]
    for s, f, r in zip(norm, rev, rows):
        assert r.replace("-", "") == (st.rc(s) if f else s)
    assert len({len(r) for r in rows}) == 1
    assert all(any(r[j] != "-" for r in rows) for j in range(len(rows[0])))
    for a in range(len(norm)):
        for b in range(len(norm)):
            if norm[a] == norm[b]:
                assert rows[a] == rows[b] and rev[a] == rev[b]


def test_properties_on_the_spec():
    rng = random.Random(17)
    clean = 0
    for seqs in sr.edge_loci() + st.strand_edge_loci() + sr.random_loci(5, 40):
        rev, how, c, rows = st.star_rows(seqs)
        ori = st.oriented(seqs)[2]
        assert (c, rows) == sr.star_rows(ori)                                  # P1: the pinned spec on the oriented records
        if not any(rev):                                                         # P2
            assert (c, rows) == sr.star_rows(seqs)
            clean += 1
        check_p4(seqs, rev, rows)                                                # P4
        mixed, flags = st.flip(rng, seqs)                                        # P3
        rev2, _, c2, rows2 = st.star_rows(mixed)
        assert (c2, rows2) == (c, rows), (seqs, flags)
        proper = [bool(s) and s != st.rc(s) for s in mixed]                      # (a record that is its own reverse complement has no strand)
        assert [r for r, p in zip(rev2, proper) if p] == [f != g for f, g, p in zip(rev, flags, proper) if p]
    assert clean >= 40


def test_properties_through_the_kernels(emu):
    rng = random.Random(23)
    loci = sr.edge_loci() + st.strand_edge_loci() + sr.random_loci(7, 30)
    recs = [records(l) for l in loci]
    ori = []
    on = sa.star_msas(emu, recs, adjust_direction=True, orientation=ori)
    off = sa.star_msas(emu, recs)
    # P1: flag-off on the records with the flags applied and _R_ prefixed
    applied = [[("_R_" + t if f else t, st.rc(sr.normalise(s)) if f else s) for (t, s), f in zip(r, rev)] for r, (rev, _) in zip(recs, ori)]
    for m, w, a in zip(on, sa.star_msas(emu, applied), applied):
        assert sa.msa_fasta(m) == sa.msa_fasta(w)
        assert m.rows_as_strings() == sr.star_rows([s for _, s in a])[1]
    clean = 0
    for l, m, f, (rev, _) in zip(loci, on, off, ori):
        if not any(rev):                                                         # P2: byte-identical files
            assert sa.msa_fasta(m) == sa.msa_fasta(f)
            clean += 1
        check_p4(l, rev, m.rows_as_strings())                                    # P4
    assert clean >= 30
    flipped = [st.flip(rng, l) for l in loci]                                    # P3
    ori2 = []
    on2 = sa.star_msas(emu, [records(m) for m, _ in flipped], adjust_direction=True, orientation=ori2)
    assert sum(any(f) for _, f in flipped) >= 25
    for m, m2 in zip(on, on2):
        assert m.rows_as_strings() == m2.rows_as_strings()


def test_small_chunks_and_budget_give_the_same_msas(emu):
    from make_prg_amd.update.profile_align import workspace_words
    loci = [records(l) for l in mixed_loci(4, 12)]
    ori, ori_small = [], []
    whole = [sa.msa_fasta(m) for m in sa.star_msas(emu, loci, adjust_direction=True, orientation=ori)]
    small = sa.star_msas(emu, loci, budget_bytes=4 * workspace_words(200, 160), chunk_bytes=1, adjust_direction=True, orientation=ori_small)
    assert [sa.msa_fasta(m) for m in small] == whole and ori_small == ori


def test_flag_off_is_untouched(emu):
    """Without the flag: no orientation, no timing entry, the titles as they are; an orientation list stays empty."""
    loci = [records(l) for l in mixed_loci(6, 5)]
    timings, ori = {}, []
    msas = sa.star_msas(emu, loci, timings=timings, orientation=ori)
    assert ori == [] and sorted(timings) == ["centre_s", "merge_s", "pairs_s"]
    for l, m in zip(loci, msas):
        assert m.rows_as_strings() == sr.star_rows([s for _, s in l])[1] and m.descriptions == [t for t, _ in l]
    timings = {}
    sa.star_msas(emu, loci, timings=timings, adjust_direction=True)
    assert sorted(timings) == ["centre_s", "merge_s", "orient_s", "pairs_s"]


def test_orientation_recovery_on_config_c_shaped_loci(emu):
    """Config-C-shaped loci (seeds 100-129 of the 100-159 the spec was checked on: 5 878 of 5 878 recovered, 0 left to the DP)
    with a random half of all records but the first reverse-complemented: the statement and the kernels recover every
    orientation, and the k-mers leave at most 1 % of the sequences to the DP."""
    rng = random.Random(5)
    loci, flags = [], []
    for _, seqs in sr.synthetic_loci(range(100, 130)):
        m, f = st.flip(rng, seqs)
        loci.append(m)
        flags.append(f)
    ori = sa.orientations(emu, codes_of(loci))
    n = sum(len(l) for l in loci)
    assert n > 2500 and sum(map(sum, flags)) > n // 3
    assert [rev for rev, _ in ori] == flags
    assert sum(how.count("d") + how.count("t") for _, how in ori) <= n // 100
    for l, f, (_, how) in zip(loci[:6], flags, ori):
        _, rev, want_how = st.orient(l)
        assert rev == f and want_how == how


def test_parser_refusal(capsys):
    from make_prg_amd.__main__ import main
    with pytest.raises(SystemExit) as exc:
        main(["from_msa", "-i", "d", "-o", "o", "--adjust-direction"])
    assert exc.value.code == 2
    assert "--adjust-direction needs --unaligned" in capsys.readouterr().err


def test_tables_out_of_range_give_the_status_not_a_write(emu):
    codes = np.arange(40, dtype=np.uint8) % 4
    for job in ([0, 10, 35], [35, 10, 0], [-1, 5, 20], [0, 5, -1], [0, -2, 20], [0, 10, 5], [5, 10, 0], [0, 41, 0]):
        d = emu.upload(codes)
        jobs = np.array([[0, 4, 20], job, [4, 3, 30]], np.int64)
        d_jobs, d_status = emu.upload(jobs), emu.empty(12)
        emu.call("mprg_star_revcomp", emu.ptr(d), 40, emu.ptr(d_jobs), 3, emu.ptr(d_status), emu.stream)
        assert emu.download(d_status, np.int32, 3).tolist() == [0, 1, 0], job
        want = codes.copy()
        want[20:24], want[30:33] = sa.revcomp(codes[0:4]), sa.revcomp(codes[4:7])
        assert np.array_equal(emu.download(d, np.uint8, 40), want), job          # the good jobs ran, the bad one wrote nothing
        with pytest.raises(sa.StarAlignError, match="mprg_star_revcomp"):
            sa.revcomp_on_device(emu, emu.upload(codes), 40, jobs)
    # mprg_star_strand: a sequence outside the codes, a locus outside the sequence table, a centre outside the locus
    seqs = np.array([[0, 10], [10, 12], [22, 18]], np.int64)
    for seq_tab, ltab, centre in ((np.array([[0, 10], [10, 12], [22, 19]]), [[0, 2, 0, 0], [2, 1, 0, 0]], [0, 0]),
                                  (seqs, [[0, 2, 0, 0], [2, 2, 0, 0]], [0, 0]),
                                  (seqs, [[0, 2, 0, 0], [2, 1, 0, 0]], [1, 1]),
                                  (seqs, [[0, 2, 0, 0], [2, 1, 0, 0]], [1, -1])):
        d_ev, d_status = emu.full(24 * 3, 0x5A), emu.empty(8)
        d_in = [emu.upload(codes), emu.upload(np.asarray(seq_tab, np.int64)), emu.upload(np.asarray(ltab, np.int64)),
                emu.upload(np.asarray(centre, np.int32))]
        emu.call("mprg_star_strand", emu.ptr(d_in[0]), 40, emu.ptr(d_in[1]), 3, emu.ptr(d_in[2]), 2, emu.ptr(d_in[3]), emu.ptr(d_ev),
                 emu.ptr(d_status), emu.stream)
        assert emu.download(d_status, np.int32, 2).tolist() == [0, sa.CENTRE_BAD]
        ev = emu.download(d_ev, np.uint8, 72)
        assert (ev[48:] == 0x5A).all() and not (ev[:48] == 0x5A).all()           # the bad locus's triple is not written
    with pytest.raises(sa.StarAlignError, match="mprg_star_strand"):
        sa.strand_evidence(emu, codes_of([["ACGTACGT", "ACGT"]]), [2])


def test_from_msa_adjust_direction_in_process(emu, tmp_path, caplog):
    """from_msa.run with --unaligned --adjust-direction on the emulation build: the MSAs written are the statement's (with the _R_
    titles), every output equals from_msa's on those MSAs, the PRGs equal those of the unflipped directory without the flag, and
    the run logs how many records it reversed."""
    import logging
    from argparse import Namespace
    from make_prg_amd.subcommands import from_msa
    from make_prg_amd.subcommands.output_type import OutputType
    from make_prg_amd.utils.synthetic import synth_rows
    rng = random.Random(2)
    plain, mixed = tmp_path / "plain", tmp_path / "mixed"
    plain.mkdir()
    mixed.mkdir()
    want, n_flipped = {}, 0
    for seed in range(3):
        seqs = [r.decode().replace("-", "") for r in synth_rows(seed, 6, 90, 2)]
        flipped, flags = st.flip(rng, seqs)
        n_flipped += sum(flags)
        for d, ss in ((plain, seqs), (mixed, flipped)):
            (d / f"g{seed}.fasta").write_text("".join(f">s{i} x\n{s}\n" for i, s in enumerate(ss)))
        want[f"g{seed}.fa"] = st.star_fasta([(f"s{i} x", s) for i, s in enumerate(flipped)])
    assert n_flipped >= 5

    def opts(**kw):
        base = dict(suffix="", alignment_format="fasta", max_nesting=5, min_match_length=7, output_type=OutputType("a"), force=False,
                    threads=1, unaligned=True, msa_dir=None, adjust_direction=False)
        base.update(kw)
        return Namespace(**base)
    d = tmp_path / "msas"
    with caplog.at_level(logging.INFO, logger="make_prg_amd"):
        from_msa.run(opts(input=str(mixed), output_prefix=str(tmp_path / "a" / "a"), msa_dir=str(d), adjust_direction=True), emu)
    assert f"--adjust-direction: {n_flipped} records reverse-complemented, 0 settled by DP" in caplog.text
    assert {p.name: p.read_text() for p in d.iterdir()} == want
    assert sum(t.count(">_R_") for t in want.values()) == n_flipped
    from_msa.run(opts(input=str(d), output_prefix=str(tmp_path / "b" / "b"), unaligned=False), emu)
    for suffix in (".prg.fa", ".prg.bin.zip", ".prg.gfa.zip", ".update_DS.zip"):
        assert (tmp_path / "a" / ("a" + suffix)).read_bytes() == (tmp_path / "b" / ("b" + suffix)).read_bytes(), suffix
    from_msa.run(opts(input=str(plain), output_prefix=str(tmp_path / "c" / "c")), emu)
    assert (tmp_path / "a" / "a.prg.fa").read_bytes() == (tmp_path / "c" / "c.prg.fa").read_bytes()
