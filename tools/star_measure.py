"""GPU-box helper: `from_msa --unaligned` stage by stage on N config-C-shaped loci (utils/synthetic.py, seeds 0..N-1) with their
gaps removed, written as unaligned FASTA files into a temporary directory first.  Prints one JSON line: wall seconds of reading
the files, the centre, pair and merge stages (star_align.star_msas; each ends at a download), writing the MSAs, and the PRG build
(from_msa's pipeline over the MSAs written), plus the DP cells (sum of n x C over the pairs).  Kernel times: run it under
`rocprofv3 --kernel-trace --stats -- python tools/star_measure.py N`.
`--flip SHARE` (after N): `--adjust-direction` on, with that share of each locus's records but the first reverse-complemented in the
files (seeded); the line then also gives orient_s, the records reversed, how many of them were flipped, and the number the DP settled.
`--band [W0]`: the pairs over a certified band (`from_msa --unaligned --band`; W0: pass 1's half-width, default
profile_align.BAND_W0); the line then also gives the band's counters (pairs, second passes, pairs sent to the full DP, DP cells
computed and of the full matrices).  msa_md5: a digest of the MSAs' text, to compare runs.
`--refine [N]`: leave-one-out refinement (`from_msa --unaligned --refine`; N rounds, default 2); the line then also gives refine_s,
the rounds accepted, the loci changed and the total objective S before and after.
`--diverged R`: instead of the config-C-shaped loci, loci of R sequences mutated from one random root of 800-1200 nt each by the
model of tests/star_ref.py's mutate(sub=0.06, indel=0.03), restated here (the tool does not import the tests): per root base 1.5 %
deleted, 6 % substituted, 1.5 % followed by an insertion of 1-4 nt.
`--progressive`: guide-tree MSAs (`from_msa --unaligned --progressive`); the line then also gives tree_s and progressive_s, the
loci built, their merges, the most and the mean rounds of a locus and the loci left to the star pass.  With `--band [W0]` as well the merges run
over certified bands (W0 then is pass 1's half-width of both stages) and the line also gives prog_band_merges,
prog_band_second_passes, prog_band_full_merges (sent to the full DP), prog_band_cells and prog_band_full_cells.
`--objective` (implied by --progressive): the line also gives s_total, the objective S of the MSAs written, summed over the loci
(mprg_refine_counts over the MSAs, after the timed part): to compare a star run and a progressive run of the same loci.
`--collapse-identical`: every distinct sequence of a locus aligned once (`from_msa --unaligned --collapse-identical`); the line then
also gives collapse_s, collapse_records, collapse_classes and collapse_pairs or collapse_merges (the alignments made).  Every line
gives dup_share: the share of the records whose sequence an earlier record of their locus has.
`--dup FRACTION`: after a locus's sequences are made, each record but the first is replaced, with that probability, by a copy of
an earlier record of the locus picked at random (seeded): loci with a known share of exact copies.
`--device-tree` (with --progressive): the guide trees on the device (`from_msa --unaligned --progressive --device-tree`); the line
then also gives tree_device_loci.  Every --progressive line gives tree_plan_s, the part of tree_s spent on the host's plan (without
--device-tree: the host's UPGMA and the plan).
`--refine-tree [N]` (with --progressive): tree-dependent refinement (`from_msa --unaligned --progressive --refine-tree`; N passes,
default 1); the line then also gives tree_refine_s, the loci with a step, the steps tried, accepted and skipped, the loci above the
cap, the loci changed and the total objective S before and after the stage.
`--retree [N]` (with --progressive): the guide tree rebuilt from the MSA (`from_msa --unaligned --progressive --retree`; N rebuilds,
default 1); the line then also gives retree_s, the loci iterated, rebuilt, accepted, refused and with the same tree, the loci changed
and the total objective S before and after the stage.
`--records N` (with --diverged A): loci of many records over few alleles: every locus has N records, each of the locus's A diverged
sequences once and then seeded picks among them, shuffled: the pan-genome core gene `--large-loci` is for.
`--large-loci` (with --progressive --collapse-identical): the leaf limit counts distinct sequences (`from_msa --unaligned
--progressive --collapse-identical --large-loci`); the line then also gives large_loci, large_records and large_fallbacks.
`--seq-weights` (with --progressive): tree weights (`from_msa --unaligned --progressive --seq-weights`); the line then also gives
seq_weight_s (the stage's wall seconds: its launches and downloads; without --device-tree the distances launched again too),
seq_weight_loci, seq_weight_min_q, and, from an untimed run of the same loci without the flag afterwards, seq_weight_loci_changed
(the loci whose MSA differs) and s_total_unweighted beside s_total.
`--pair-distances` (with --progressive): the first guide trees from the pair DP's scores (`from_msa --unaligned --progressive
--pair-distances`); the line then also gives pair_dist_s (part of tree_s), pair_dist_loci, pair_dist_pairs, pair_dist_cells,
pair_dist_above_cap, pair_dist_limit (with --band pair_dist_second_passes and pair_dist_full_pairs) and, from an untimed run of the
same loci without the flag afterwards, pair_dist_loci_changed (the loci whose MSA differs), pair_dist_loci_higher and
pair_dist_loci_lower (by the locus's objective S) and s_total_kmer beside s_total.
`--position-gaps` (with --progressive): the merges' opens by occupancy (`from_msa --unaligned --progressive --position-gaps`); the
line then also gives position_gap_merges.
`--free-end-gaps` (with --progressive): the merges as overlap alignments (`from_msa --unaligned --progressive --free-end-gaps`); the
line then also gives free_end_gap_merges.
`--free-end-pairs`: the pairs of the star pass and the realignments of --refine as overlap alignments (`from_msa --unaligned
--free-end-pairs`), with or without --progressive; the line then also gives free_end_pair_alignments.
`--free-end-distances` (with --progressive --pair-distances): the pair scores as overlap scores (`from_msa --unaligned --progressive
--pair-distances --free-end-distances`); the line then also gives free_end_distance_pairs.
`--fragments SHARE` (with --diverged): that share of each locus's records but the first is cut to a piece of 30-80 % of its length
at either end or inside (utils/synthetic.py's fragment_locus, seeded); the truth keeps the cut residues out.
`--truth`: the MSAs written are scored against the alignment that is true by construction (`compare_msa`'s counts,
make_prg_amd/from_msa/msa_compare.py, after the timed part): synth_rows' own rows for the config-C-shaped loci, diverged_locus'
true_rows with --diverged; the line then also gives truth_shared, truth_ref_pairs, truth_test_pairs, truth_ref_columns, truth_kept,
truth_identical (summed over the loci) and compare_s, the wall seconds of the compare stage.  With --flip the truth holds every
record in the family's orientation, so a row is matched as a reversed row (the `_R_` prefix) exactly where the aligner's choice and
the file's flip disagree.  Not with --records or --dup.
`--no-prg`: the PRG build over the MSAs written is left out (no prg_build_s): for runs that compare the alignment stages only."""
import hashlib
import json
import os
import random
import shutil
import sys
import tempfile
import time
from argparse import Namespace
from pathlib import Path

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from make_prg_amd.device import get_backend  # noqa: E402
from make_prg_amd.from_msa import star_align as sa  # noqa: E402
from make_prg_amd.subcommands import from_msa  # noqa: E402
from make_prg_amd.subcommands.output_type import OutputType  # noqa: E402
from make_prg_amd.utils.synthetic import config_shape, diverged_locus, fragment_locus, synth_rows  # noqa: E402

n_loci = int(sys.argv[1]) if len(sys.argv) > 1 and not sys.argv[1].startswith("--") else 1000
COMPLEMENT = str.maketrans("ACGTRYKMSWN", "TGCAYRMKSWN")
flip = float(sys.argv[sys.argv.index("--flip") + 1]) if "--flip" in sys.argv else None
band = False
if "--band" in sys.argv:
    nxt = sys.argv[sys.argv.index("--band") + 1:][:1]
    band = int(nxt[0]) if nxt and nxt[0].isdigit() else True
refine = 0
if "--refine" in sys.argv:
    nxt = sys.argv[sys.argv.index("--refine") + 1:][:1]
    refine = int(nxt[0]) if nxt and nxt[0].isdigit() else sa.REFINE_DEFAULT
progressive = "--progressive" in sys.argv
objective = progressive or "--objective" in sys.argv
diverged = int(sys.argv[sys.argv.index("--diverged") + 1]) if "--diverged" in sys.argv else 0
collapse = "--collapse-identical" in sys.argv
dup = float(sys.argv[sys.argv.index("--dup") + 1]) if "--dup" in sys.argv else 0.0
device_tree = "--device-tree" in sys.argv
if device_tree and not progressive:
    sys.exit("--device-tree needs --progressive")
refine_tree = None
if "--refine-tree" in sys.argv:
    nxt = sys.argv[sys.argv.index("--refine-tree") + 1:][:1]
    refine_tree = int(nxt[0]) if nxt and nxt[0].isdigit() else sa.TREE_REFINE_DEFAULT
    if not progressive:
        sys.exit("--refine-tree needs --progressive")
retree = None
if "--retree" in sys.argv:
    nxt = sys.argv[sys.argv.index("--retree") + 1:][:1]
    retree = int(nxt[0]) if nxt and nxt[0].isdigit() else sa.RETREE_DEFAULT
    if not progressive:
        sys.exit("--retree needs --progressive")
seq_weights = "--seq-weights" in sys.argv
if seq_weights and not progressive:
    sys.exit("--seq-weights needs --progressive")
pair_distances = "--pair-distances" in sys.argv
if pair_distances and not progressive:
    sys.exit("--pair-distances needs --progressive")
position_gaps = "--position-gaps" in sys.argv
if position_gaps and not progressive:
    sys.exit("--position-gaps needs --progressive")
free_end_gaps = "--free-end-gaps" in sys.argv
if free_end_gaps and not progressive:
    sys.exit("--free-end-gaps needs --progressive")
free_end_pairs = "--free-end-pairs" in sys.argv
free_end_distances = "--free-end-distances" in sys.argv
if free_end_distances and not (progressive and pair_distances):
    sys.exit("--free-end-distances needs --progressive and --pair-distances")
fragments = float(sys.argv[sys.argv.index("--fragments") + 1]) if "--fragments" in sys.argv else None
if fragments is not None and not diverged:
    sys.exit("--fragments needs --diverged")
records = int(sys.argv[sys.argv.index("--records") + 1]) if "--records" in sys.argv else 0
if records and not diverged:
    sys.exit("--records needs --diverged")
truth = "--truth" in sys.argv
if truth and (records or dup):
    sys.exit("--truth does not go with --records or --dup")
large_loci = "--large-loci" in sys.argv
if large_loci and not (progressive and collapse):
    sys.exit("--large-loci needs --progressive and --collapse-identical")
prog_kw = dict(progressive=True, **(dict(device_tree=True) if device_tree else {}), **(dict(large_loci=True) if large_loci else {}),
               **(dict(refine_tree=refine_tree) if refine_tree else {}), **(dict(retree=retree) if retree else {}),
               **(dict(seq_weights=True) if seq_weights else {}), **(dict(pair_distances=True) if pair_distances else {}),
               **(dict(position_gaps=True) if position_gaps else {}),
               **(dict(free_end_gaps=True) if free_end_gaps else {}),
               **(dict(free_end_distances=True) if free_end_distances else {})) if progressive else {}
if free_end_pairs:
    prog_kw = dict(prog_kw, free_end_pairs=True)             # (not an option of progressive, but handed on with them to every run)


def objectives(be, msas):
    """The objective S of every MSA (mprg_refine_counts over their text)."""
    import numpy as np
    out = []
    for lo in range(0, len(msas), 64):
        part = msas[lo:lo + 64]
        R, W = np.array([m.data.shape[0] for m in part], np.int64), np.array([m.data.shape[1] for m in part], np.int64)
        toff = np.concatenate([[0], np.cumsum(R * W)[:-1]]).astype(np.int64)
        text = np.concatenate([np.ascontiguousarray(m.data).reshape(-1) for m in part])
        out.extend(int(v) for v in sa.refine_counts(be, be.upload(text), len(text), toff, R, W)[4])
    return out


def objective_total(be, msas):
    """The objective S of the MSAs, summed over the loci."""
    return sum(objectives(be, msas))


work = Path(tempfile.mkdtemp(prefix="star_measure_"))
try:
    src, msa_dir = work / "unaligned", work / "msas"
    src.mkdir()
    msa_dir.mkdir()
    t0 = time.perf_counter()
    rng, flipped, true_rows = random.Random(1), [], []
    for seed in range(n_loci):
        if diverged:
            seqs, rows = diverged_locus(seed, diverged) if fragments is None else fragment_locus(seed, diverged, share=fragments)
        else:
            rows = [r.decode() for r in synth_rows(seed, *config_shape("C", seed))]
            seqs = [r.replace("-", "") for r in rows]
        if truth:
            true_rows.append(rows)
        if records:
            rrng = random.Random(2000003 + seed)
            seqs = seqs + [rrng.choice(seqs) for _ in range(records - len(seqs))]
            rrng.shuffle(seqs)
        if dup:
            drng = random.Random(1000003 + seed)
            for i in range(1, len(seqs)):
                if drng.random() < dup:
                    seqs[i] = seqs[drng.randrange(i)]
        if flip is not None:
            flags = [i > 0 and rng.random() < flip for i in range(len(seqs))]
            seqs = [s.translate(COMPLEMENT)[::-1] if f else s for s, f in zip(seqs, flags)]
            flipped.append(flags)
        (src / f"gene{seed:05d}.fa").write_text("".join(f">s{i}\n{s}\n" for i, s in enumerate(seqs)))
    t_gen = time.perf_counter() - t0
    files = sorted(src.iterdir())
    be = get_backend("runtime")
    sa.star_msas(be, [sa.read_unaligned(f) for f in files[:4]], adjust_direction=flip is not None, band=band, refine=refine,
                 **prog_kw, **(dict(collapse=True) if collapse else {}))   # warm-up: first launches
    t0 = time.perf_counter()
    recs = [sa.read_unaligned(f) for f in files]
    t_read = time.perf_counter() - t0
    timings = {}
    t0 = time.perf_counter()
    orientation = []
    refinement = []
    progression = []
    tree_refinement = []
    retreeing = []
    msas = sa.star_msas(be, recs, timings=timings, adjust_direction=flip is not None, orientation=orientation, band=band, refine=refine,
                        refinement=refinement, **(dict(prog_kw, progression=progression) if progressive else prog_kw),
                        **(dict(tree_refinement=tree_refinement) if refine_tree else {}), **(dict(retreeing=retreeing) if retree else {}),
                        **(dict(collapse=True) if collapse else {}))
    t_star = time.perf_counter() - t0
    t0 = time.perf_counter()
    written, digest = [], hashlib.md5()
    for f, m in zip(files, msas):
        p = msa_dir / f.name
        text = sa.msa_fasta(m)
        p.write_text(text)
        digest.update(text.encode())
        written.append(p)
    t_write = time.perf_counter() - t0
    codes = [sa.locus_codes(f.name, r) for f, r in zip(files, recs)]
    extra = dict(dup_share=round(sum(len(r) - len({s for _, s in r}) for r in recs) / max(1, sum(len(r) for r in recs)), 4))
    if collapse:
        extra.update(collapse=True)
    if dup:
        extra.update(dup=dup)
    if flip is not None:
        codes = [[sa.revcomp(c) if f else c for c, f in zip(cs, rev)] for cs, (rev, _) in zip(codes, orientation)]
        extra.update(flip=flip, reversed=sum(sum(rev) for rev, _ in orientation),
                     reversed_as_flipped=sum(sum(a and b for a, b in zip(rev, fl)) for (rev, _), fl in zip(orientation, flipped)),
                     flipped=sum(map(sum, flipped)), settled_by_dp=sum(how.count("d") + how.count("t") for _, how in orientation))
    if refine:
        extra.update(refine=refine, rounds_accepted=sum(a for a, _, _ in refinement), loci_changed=sum(1 for a, _, _ in refinement if a),
                     s_before=sum(s for _, s, _ in refinement), s_after=sum(s for _, _, s in refinement))
    if progressive:
        built = [(n, r) for n, r, star in progression if not star]
        extra.update(progressive=True, device_tree=device_tree, loci_built=len(built), merges=sum(n - 1 for n, _ in built), max_rounds=max((r for _, r in built), default=0), mean_rounds=round(sum(r for _, r in built) / max(1, len(built)), 2),
                     loci_left_to_star=len(progression) - len(built), **(dict(large_loci_flag=True) if large_loci else {}))
    if refine_tree:
        done = [t for t in tree_refinement if t]
        extra.update(refine_tree=refine_tree, tree_loci_changed=sum(1 for t in done if t[1]), tree_s_before=sum(t[3] for t in done),
                     tree_s_after=sum(t[4] for t in done))
    if retree:
        done = [t for t in retreeing if t]
        extra.update(retree=retree, retree_loci_changed=sum(1 for t in done if t[1]), retree_s_before=sum(t[3] for t in done),
                     retree_s_after=sum(t[4] for t in done))
    if objective:
        extra.update(s_total=objective_total(be, msas))
    if seq_weights:
        plain = sa.star_msas(be, recs, adjust_direction=flip is not None, band=band, refine=refine, **dict(prog_kw, seq_weights=False),
                             **(dict(collapse=True) if collapse else {}))
        extra.update(seq_weights=True, seq_weight_loci_changed=sum(1 for a, b in zip(msas, plain) if sa.msa_fasta(a) != sa.msa_fasta(b)),
                     s_total_unweighted=objective_total(be, plain))
    if pair_distances:
        plain = sa.star_msas(be, recs, adjust_direction=flip is not None, band=band, refine=refine, **dict(prog_kw, pair_distances=False, free_end_distances=False),
                             **(dict(collapse=True) if collapse else {}))
        s_on, s_off = objectives(be, msas), objectives(be, plain)
        extra.update(pair_distances=True, pair_dist_loci_changed=sum(1 for a, b in zip(msas, plain) if sa.msa_fasta(a) != sa.msa_fasta(b)),
                     pair_dist_loci_higher=sum(1 for a, b in zip(s_on, s_off) if a > b), pair_dist_loci_lower=sum(1 for a, b in zip(s_on, s_off) if a < b),
                     s_total_kmer=sum(s_off))
    if position_gaps:
        extra.update(position_gaps=True)
    if free_end_gaps:
        extra.update(free_end_gaps=True)
    if free_end_pairs:
        extra.update(free_end_pairs=True)
    if free_end_distances:
        extra.update(free_end_distances=True)
    if fragments is not None:
        extra.update(fragments=fragments)
    if truth:
        from make_prg_amd.from_msa import msa_compare as mc
        from make_prg_amd.msa import MSA
        t0 = time.perf_counter()
        ids = [[f"s{i}" for i in range(len(rows))] for rows in true_rows]
        tests = msas
        if flip is not None:          # (a row holds the reverse complement of its truth row where the aligner and the file disagree)
            tests = [MSA(_data=m.data, _ids=[(sa.REVERSED_PREFIX if a != b else "") + i for i, a, b in zip(ii, rev, fl)], _descs=m.descriptions)
                     for m, ii, (rev, _), fl in zip(msas, ids, orientation, flipped)]
        scored = mc.total(mc.compare_msas(be, tests, [MSA.from_strings(rows, ii) for rows, ii in zip(true_rows, ids)],
                                          names=[f.name for f in files]))
        extra.update(truth_shared=scored.shared, truth_ref_pairs=scored.ref_pairs, truth_test_pairs=scored.test_pairs,
                     truth_ref_columns=scored.ref_columns, truth_kept=scored.kept_columns, truth_identical=scored.identical_columns,
                     compare_s=round(time.perf_counter() - t0, 3))
    cent = sa.centres(be, codes)
    cells = sum(len(c) * len(cs[int(k)]) for cs, k in zip(codes, cent) for a, c in enumerate(cs) if a != int(k))
    opts = Namespace(input=str(msa_dir), suffix="", output_prefix=str(work / "out" / "prg"), alignment_format="fasta",
                     max_nesting=5, min_match_length=7, output_type=OutputType("a"), force=False, threads=16)
    t_prg = None
    if "--no-prg" not in sys.argv:
        t0 = time.perf_counter()
        from_msa._run(opts, None, None, 1, msa_files=written)
        t_prg = time.perf_counter() - t0
    print(json.dumps(dict(loci=n_loci, pairs=sum(len(r) - 1 for r in recs), residues=sum(len(s) for r in recs for _, s in r),
                          generate_s=round(t_gen, 2), read_s=round(t_read, 3), star_s=round(t_star, 3),
                          **{k: round(v, 3) for k, v in timings.items()}, write_s=round(t_write, 3), **({} if t_prg is None else dict(prg_build_s=round(t_prg, 3))),
                          dp_cells=cells, msa_md5=digest.hexdigest(), **extra)))
finally:
    shutil.rmtree(work, ignore_errors=True)
