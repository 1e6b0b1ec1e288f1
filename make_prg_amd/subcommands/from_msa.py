"""`from_msa` sub-command: same flags and output files as make_prg/subcommands/from_msa.py:18-198.

Instead of one worker process per alignment, the input list is sharded over the ranks of the job (one process per
GPU; a single process when run plainly) and each rank streams its shard through the file -> file pipeline on its device
(make_prg_amd/pipeline.py).  Per-locus policy is the reference's: a SequenceCurationError skips the locus with a
warning, an empty alignment aborts the run (EmptyMSAError).  Under several ranks every rank writes segment files, rank 0 gathers
the segments' INDEX (the job's one collective) and merges their byte ranges into <prefix>.prg.fa (loci in sorted order),
<prefix>.prg.bin(.zip), <prefix>.prg.gfa(.zip), <prefix>.update_DS.zip (utils/segments.py).
"""
import logging
import os
import pickle
from pathlib import Path
from typing import Dict, List, Optional

import numpy as np

from ..engine import BatchEngine, SequenceCurationError, build_prg
from ..from_msa import MIN_MATCH_LEN, NESTING_LVL
from ..msa import load_alignment_file
from ..utils.gfa import GFA_Output
from ..utils.io_utils import output_files_already_exist, remove_known_input_extensions, zip_bytes
from ..utils.prg_encoder import PrgEncoder

logger = logging.getLogger("make_prg_amd")


class EmptyMSAError(Exception):
    pass


def register_parser(subparsers):
    p = subparsers.add_parser("from_msa", usage="make_prg from_msa", help="Make PRG from multiple sequence alignment")
    p.add_argument("-i", "--input", action="store", type=str, required=True,
                   help="Multiple sequence alignment file or a directory containing such files")
    p.add_argument("-s", "--suffix", action="store", type=str, default="",
                   help="If the input parameter (-i, --input) is a directory, then filter for files with this suffix. "
                        "If this parameter is not given, all files in the input directory is considered.")
    p.add_argument("-o", "--output-prefix", dest="output_prefix", action="store", type=str, required=True,
                   help="Prefix for the output files")
    p.add_argument("-f", "--alignment-format", dest="alignment_format", action="store", default="fasta",
                   help="Alignment format of MSA. fasta (default: %(default)s) is read exactly as the reference reads it (every golden file of "
                        "the reference is FASTA).  clustal, stockholm, phylip, phylip-sequential, phylip-relaxed are BEST-EFFORT restatements of "
                        "Biopython's readers (not pinned against Bio.AlignIO: record ids of unusual files may differ); any other AlignIO format "
                        "is an error")
    p.add_argument("-N", "--max-nesting", dest="max_nesting", action="store", type=int, default=NESTING_LVL,
                   help="Maximum number of levels to use for nesting. Default: %(default)d")
    p.add_argument("-L", "--min-match-length", dest="min_match_length", action="store", type=int, default=MIN_MATCH_LEN,
                   help="Minimum number of consecutive characters which must be identical for a match. Default: %(default)d")
    p.add_argument("--unaligned", action="store_true", default=False,
                   help="(this implementation) the input files are UNALIGNED FASTA(.gz), one locus per file: each locus's MSA is built on "
                        "the GPU first, a centre-star alignment with the package's own aligner (make_prg_amd/from_msa/star_align.py) — NOT "
                        "MAFFT, so the PRGs differ from those of a MAFFT alignment — and written as <locus>.fa; the PRGs are then built "
                        "from those files exactly as from_msa -i on them would.  Only with -f fasta")
    p.add_argument("--msa-dir", dest="msa_dir", action="store", type=str, default=None,
                   help="(this implementation) with --unaligned: keep the MSAs in this directory (existing files are not overwritten "
                        "without -F); default: a private temporary directory beside the output prefix, removed at the end")
    p.add_argument("--adjust-direction", dest="adjust_direction", action="store_true", default=False,
                   help="(this implementation) with --unaligned: records on the opposite strand are detected on the GPU and "
                        "reverse-complemented before the alignment; the first non-empty record of a locus keeps its orientation, the "
                        "title of a reversed record gets the prefix _R_ (as MAFFT's --adjustdirection does; the method is the "
                        "package's own, star_align.py)")
    p.add_argument("--band", dest="band", action="store_true", default=False,
                   help="(this implementation) with --unaligned: the pair alignments are computed over a band of diagonals that a "
                        "certificate proves wide enough (two passes; make_prg_amd/update/profile_align.py): the same MSAs and PRGs, "
                        "byte for byte, from a fraction of the DP cells and of the traceback memory, and pairs too long for the "
                        "full matrix are accepted; with --progressive the profile-profile merges run over certified bands too "
                        "(star_align.py, Progressive, band).  Off by default")
    p.add_argument("--refine", dest="refine", action="store", type=int, nargs="?", const=2, default=None, metavar="N",
                   help="(this implementation) with --unaligned: every locus's centre-star MSA gets up to N rounds (1-16; --refine "
                        "alone: 2) of leave-one-out refinement on the GPU before it is written: every row is realigned against the "
                        "profile of all the others, and a round is kept only if it raises the locus's sum-of-pairs objective "
                        "(star_align.py, Refinement), so a locus the rounds do not improve keeps its star MSA byte for byte; a locus too long for a "
                        "round's DP over its MSA's columns (star_align.py, Limit) is left as it is.  "
                        "Off by default")
    p.add_argument("--progressive", dest="progressive", action="store_true", default=False,
                   help="(this implementation) with --unaligned: every locus's MSA is built progressively on the GPU instead of "
                        "centre-star: an exact UPGMA guide tree from 6-mer distances, then profile-profile merges up the tree "
                        "(star_align.py, Progressive); NOT MAFFT.  --adjust-direction runs first, --refine afterwards, --band computes "
                        "the merges (and the refinement's realignments) over certified bands, the same bytes; a locus of more than 4096 non-empty records gets the centre-star MSA "
                        "(with --collapse-identical --large-loci: of more than 4096 distinct sequences, or more than 1048576 records).  "
                        "Off by default")
    p.add_argument("--collapse-identical", dest="collapse_identical", action="store_true", default=False,
                   help="(this implementation) with --unaligned: the records of a locus whose sequences are identical (after "
                        "--adjust-direction: a record and a reverse-complemented copy of it are) are found on the GPU and aligned "
                        "once; every copy gets its representative's row (star_align.py, Collapse).  The centre-star MSAs are the "
                        "same bytes from fewer pair alignments; with --progressive the tree has one weighted leaf per distinct "
                        "sequence, so equal sequences get equal rows (also after --refine), and a locus without duplicates keeps "
                        "its --progressive bytes.  Combines with --adjust-direction, --band, --refine and --progressive.  Off by default")
    p.add_argument("--device-tree", dest="device_tree", action="store_true", default=False,
                   help="(this implementation) with --unaligned --progressive: the guide trees of the loci of three or more leaves "
                        "are built on the GPU too (csrc/k_prog_tree.inc: the same exact UPGMA with the same tie rule, weighted with "
                        "--collapse-identical), on the distance tables where they are; only the merges come back.  The same bytes.  "
                        "Off by default")
    p.add_argument("--large-loci", dest="large_loci", action="store_true", default=False,
                   help="(this implementation) with --unaligned --progressive --collapse-identical: the leaf limit of --progressive "
                        "counts distinct sequences, not records: a locus of up to 1048576 records over at most 4096 distinct non-empty "
                        "sequences is built progressively (star_align.py, Large loci; with --device-tree its tree by "
                        "csrc/k_prog_tree_wide.inc, which compares the averages in 128-bit integers); a locus over either limit gets the "
                        "centre-star MSA as before, and a locus of at most 4096 records keeps its bytes.  Off by default")
    from ..from_msa import star_align                   # (its constants: the parser states them, it launches nothing)
    p.add_argument("--refine-tree", dest="refine_tree", action="store", type=int, nargs="?", const=star_align.TREE_REFINE_DEFAULT, default=None,
                   metavar="N",
                   help=f"(this implementation) with --unaligned --progressive: after the last merge every locus of "
                        f"{star_align.TREE_REFINE_MIN_LEAVES} to {star_align.TREE_REFINE_MAX_LEAVES} leaves gets up to N passes "
                        f"(1-{star_align.TREE_REFINE_MAX}; --refine-tree alone: {star_align.TREE_REFINE_DEFAULT}) of tree-dependent "
                        "refinement on the GPU: the MSA is cut at "
                        "an edge of its guide tree, the two halves are realigned as profiles, and the result is kept only if it "
                        "raises the locus's sum-of-pairs objective (star_align.py, Tree refinement), so a locus no step improves "
                        "keeps its --progressive bytes.  --refine runs after it, --band and --device-tree give the same bytes, with "
                        "--collapse-identical equal sequences keep equal rows.  Off by default")
    p.add_argument("--retree", dest="retree", action="store", type=int, nargs="?", const=star_align.RETREE_DEFAULT, default=None, metavar="N",
                   help="(this implementation) with --unaligned --progressive: after the last merge every locus of 3 or more leaves gets "
                        f"up to N rebuilds (1-{star_align.RETREE_MAX}; --retree alone: {star_align.RETREE_DEFAULT}) of its guide tree on "
                        "the GPU: pairwise identities over the shorter sequence are taken from the rows of the MSA (all pairs, "
                        "csrc/k_prog_retree.inc), a new tree is built from them and the locus is aligned again up that tree; the new "
                        "MSA is kept only if it raises the locus's sum-of-pairs objective (star_align.py, Retree), so a locus whose "
                        "tree comes out the same or whose rebuild is refused keeps its --progressive bytes.  --refine-tree and "
                        "--refine run after it, --band and --device-tree give the same bytes.  Off by default")
    p.add_argument("--seq-weights", dest="seq_weights", action="store_true", default=False,
                   help="(this implementation) with --unaligned --progressive: every leaf of a guide tree gets a weight from 1 to 256, "
                        "its share of the tree's edge lengths (ClustalW's scheme in integers; node heights from the tree's own "
                        "distances on the GPU, csrc/k_prog_weights.inc), and counts that often in every profile merge, so an "
                        "over-sampled clade counts about as much as a lonely one (star_align.py, Sequence weights).  The tree, the "
                        "row order and the objective are unchanged; with --collapse-identical a class's weight replaces its size in "
                        "the merges.  --retree and --refine-tree use the weights of the tree that built the MSA, --refine runs "
                        "after it unweighted, --band and --device-tree give the same bytes.  Off by default")
    p.add_argument("--pair-distances", dest="pair_distances", action="store_true", default=False,
                   help="(this implementation) with --unaligned --progressive: the first guide tree of every locus of 3 to "
                        f"{star_align.PAIR_DIST_MAX_LEAVES} leaves is built from the scores of the pair DP over all pairs of its leaves "
                        "(ClustalW's pairwise mode, MAFFT's --globalpair; a score-only sweep on the GPU, csrc/k_align_scores.inc) "
                        "instead of from 6-mer counts, which saturate on diverged sub-families (star_align.py, Pair distances).  A "
                        "locus with more leaves keeps the 6-mer tree and is reported.  Everything after the tree is unchanged; "
                        "--band computes the same scores over certified bands, --device-tree keeps the tables on the GPU, --retree, "
                        "--refine-tree and --refine run after it.  Off by default")
    p.add_argument("--position-gaps", dest="position_gaps", action="store_true", default=False,
                   help="(this implementation) with --unaligned --progressive: a profile merge charges the opening of a gap run by "
                        "the occupancy of the column the run starts at, -704 times the share of rows with a residue there (ClustalW, "
                        "MUSCLE and MAFFT scale a profile position's gap open the same way), instead of -704 whatever the column; "
                        "so skipping a column in which one row of fifty has a residue costs about as little to open as to extend, and "
                        "independent insertions are no longer pushed into one column (star_align.py, Position gaps; "
                        "csrc/pg_pairs.inc).  The tree, the row order and the objective are unchanged; the merges of --retree and "
                        "--refine-tree use the same opens, --refine runs afterwards with the fixed open, --band and --device-tree "
                        "give the same bytes.  Off by default")
    p.add_argument("--free-end-gaps", dest="free_end_gaps", action="store_true", default=False,
                   help="(this implementation) with --unaligned --progressive: a profile merge is an overlap (semi-global) "
                        "alignment: the run of one side's columns alone at either end of it costs neither an open nor its "
                        "columns, instead of being charged like an internal deletion (star_align.py, Free end gaps; "
                        "csrc/pg_pairs.inc).  For loci with partial records: genes cut at a contig edge, truncated hits.  The tree, "
                        "the row order and the objective (which keeps charging end runs) are unchanged; the merges of --retree and "
                        "--refine-tree use the same boundaries, --position-gaps keeps its opens inside, --refine runs afterwards "
                        "with charged ends, --band and --device-tree give the same bytes.  Off by default")
    p.add_argument("--free-end-pairs", dest="free_end_pairs", action="store_true", default=False,
                   help="(this implementation) with --unaligned, with or without --progressive: every sequence-against-profile "
                        "alignment is an overlap (semi-global) alignment: the pairs of the star pass (also of the loci a "
                        "progressive run leaves to it) and every realignment of --refine (star_align.py, Free end pairs; "
                        "csrc/al_pairs.inc).  For loci with partial records: a fragment's missing end is no longer billed as a "
                        "deletion of hundreds of columns.  --progressive --free-end-gaps --refine wants it: without it --refine "
                        "realigns every row with charged ends.  The centre, the merges, the objective and --adjust-direction are "
                        "unchanged; --band and --collapse-identical give the same bytes.  Off by default")
    p.add_argument("--free-end-distances", dest="free_end_distances", action="store_true", default=False,
                   help="(this implementation) with --unaligned --progressive --pair-distances: the pair scores the first guide tree "
                        "is built from are overlap (semi-global) scores: end gaps cost nothing in the score-only sweep, as in "
                        "--free-end-pairs' DP (star_align.py, Free end distances; csrc/al_scores.inc).  For loci with partial "
                        "records: with charged ends a fragment that is an exact copy of less than a third of a record is as far from "
                        "it as a random sequence; with free ends its distance is 0 and the tree puts it beside its relatives.  "
                        "Everything after the distances is unchanged; independent of --free-end-gaps and --free-end-pairs; --band "
                        "and --device-tree give the same bytes.  Off by default")
    p.set_defaults(func=run, check=check_options)
    return p


def check_options(args, parser):
    """The combinations argparse cannot refuse by itself (called by the command line right after parsing)."""
    if args.unaligned and args.alignment_format.lower() != "fasta":
        parser.error("--unaligned reads FASTA only: it cannot be combined with -f " + args.alignment_format)
    if args.msa_dir is not None and not args.unaligned:
        parser.error("--msa-dir needs --unaligned")
    if args.adjust_direction and not args.unaligned:
        parser.error("--adjust-direction needs --unaligned")
    if getattr(args, "band", False) and not args.unaligned:
        parser.error("--band needs --unaligned")
    if getattr(args, "progressive", False) and not args.unaligned:
        parser.error("--progressive needs --unaligned")
    if getattr(args, "collapse_identical", False) and not args.unaligned:
        parser.error("--collapse-identical needs --unaligned")
    if getattr(args, "device_tree", False) and not getattr(args, "progressive", False):
        parser.error("--device-tree needs --progressive")
    if getattr(args, "large_loci", False):
        if not getattr(args, "progressive", False):
            parser.error("--large-loci needs --progressive")
        if not getattr(args, "collapse_identical", False):
            parser.error("--large-loci needs --collapse-identical")
    if getattr(args, "refine_tree", None) is not None:
        if not getattr(args, "progressive", False):
            parser.error("--refine-tree needs --progressive")
        from ..from_msa import star_align
        if not 1 <= args.refine_tree <= star_align.TREE_REFINE_MAX:
            parser.error(f"--refine-tree takes 1 to {star_align.TREE_REFINE_MAX} passes, not {args.refine_tree}")
    if getattr(args, "retree", None) is not None:
        if not getattr(args, "progressive", False):
            parser.error("--retree needs --progressive")
        from ..from_msa import star_align
        if not 1 <= args.retree <= star_align.RETREE_MAX:
            parser.error(f"--retree takes 1 to {star_align.RETREE_MAX} rebuilds, not {args.retree}")
    if getattr(args, "seq_weights", False) and not getattr(args, "progressive", False):
        parser.error("--seq-weights needs --progressive")
    if getattr(args, "pair_distances", False) and not getattr(args, "progressive", False):
        parser.error("--pair-distances needs --progressive")
    if getattr(args, "position_gaps", False) and not getattr(args, "progressive", False):
        parser.error("--position-gaps needs --progressive")
    if getattr(args, "free_end_gaps", False) and not getattr(args, "progressive", False):
        parser.error("--free-end-gaps needs --progressive")
    if getattr(args, "free_end_pairs", False) and not args.unaligned:
        parser.error("--free-end-pairs needs --unaligned")
    if getattr(args, "free_end_distances", False):
        if not getattr(args, "progressive", False):
            parser.error("--free-end-distances needs --progressive")
        if not getattr(args, "pair_distances", False):
            parser.error("--free-end-distances needs --pair-distances")
    if getattr(args, "refine", None) is not None:
        if not args.unaligned:
            parser.error("--refine needs --unaligned")
        if not 1 <= args.refine <= 16:
            parser.error(f"--refine takes 1 to 16 rounds, not {args.refine}")


def get_all_input_files(input_path: str, suffix: str) -> List[Path]:
    path = Path(input_path)
    if not path.exists():
        raise FileNotFoundError(f"{path} does not exist")
    if path.is_file():
        return [path]
    root = path.resolve()
    with os.scandir(root) as it:          # (one directory read; Path.resolve() / is_file() per entry cost 0.5 s per 30 000 files)
        return [root / e.name for e in it if e.name.endswith(suffix) and e.is_file()]


def _dist():
    """(rank, world, dist module or None): a torch.distributed job if the launcher set one up."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    # MPRG_DIST_FORCE=1: a process group (and the multi-rank path: segments, index all-gather, placement) also for ONE rank — what a box
    # with one GPU can show of the multi-GPU job: the library's kernels, RCCL's communicator and one HIP runtime in one process
    if world == 1 and (os.environ.get("MPRG_DIST_FORCE", "0") == "0" or "MASTER_ADDR" not in os.environ):
        return 0, 1, None
    import torch
    import torch.distributed as dist
    if not dist.is_initialized():
        backend = os.environ.get("MPRG_DIST_BACKEND", "nccl")
        if backend == "nccl":
            torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
        dist.init_process_group(backend)
        _dist.we_initialised = True
    return dist.get_rank(), dist.get_world_size(), dist


_dist.we_initialised = False


def balanced_parts(files: List[Path], n_parts: int) -> List[List[Path]]:
    """Cost-balanced split: longest-processing-time greedy on file size (gene sizes are skewed), every file stat-ed once,
    one pass with a heap of part loads.  Deterministic (ties by path and part number)."""
    import heapq
    sized = sorted(((-f.stat().st_size, str(f), f) for f in files))
    heap = [(0, p) for p in range(n_parts)]
    parts: List[List[Path]] = [[] for _ in range(n_parts)]
    for neg, _, f in sized:
        load, p = heapq.heappop(heap)
        parts[p].append(f)
        heapq.heappush(heap, (load - neg, p))
    return parts


def shard_files(files: List[Path], rank: int, world: int) -> List[Path]:
    """This rank's shard of the input list: a CONTIGUOUS stretch of the run's sorted loci (the order of every output file,
    utils/input_output_files.py:89), cut where the cumulative file size crosses rank / world of the total — so a rank's part of every
    output file is one byte range (utils/segments.py: every rank places its own bytes), and the shards are balanced by size to
    within one file (a 30 000-gene pan-genome: thousands of files per rank)."""
    from ..pipeline import sort_key
    ordered = sorted(files, key=sort_key)
    sizes = np.asarray([f.stat().st_size for f in ordered], np.float64)
    total = float(sizes.sum())
    if total <= 0:
        return ordered[rank::world]
    mid = np.cumsum(sizes) - sizes / 2.0                   # a file belongs to the rank its midpoint falls into
    owner = np.minimum((mid * world / total).astype(np.int64), world - 1)
    return [f for f, o in zip(ordered, owner.tolist()) if o == rank]


def _load_one(args):
    path, fmt = args
    try:
        return load_alignment_file(path, fmt, defer_n=True)      # N columns are counted on the device, batch-wise
    except ValueError as err:
        return err


def load_many(files: List[Path], alignment_format: str, procs: int = 1) -> list:
    """Parse + upper-case + N-replace every file (utils/io_utils.py:17-49), with `procs` worker processes.
    Must run before the GPU is initialised when procs > 1 (the workers are forked)."""
    jobs = [(f, alignment_format) for f in files]
    if procs > 1 and len(files) >= 32:
        import multiprocessing as mp
        with mp.get_context("fork").Pool(procs) as pool:
            return pool.map(_load_one, jobs, chunksize=16)
    return [_load_one(j) for j in jobs]


BATCH = int(os.environ.get("MPRG_BATCH", "4096"))          # alignments per resident batch
_CHECK_TREES = os.environ.get("MPRG_CHECK", "") not in ("", "0")


def build_shard(files: List[Path], options, backend=None) -> Dict[str, dict]:
    """All loci of this rank: {locus: {prg, bin, gfa, pickle}}; loci skipped by the curation policy are absent.
    Ingest runs in `-t` worker processes (the reference's -t starts that many per-alignment workers); the build runs
    in resident batches of MPRG_BATCH alignments on this rank's GPU."""
    loaded = load_many(files, options.alignment_format, max(1, int(getattr(options, "threads", 1) or 1)))
    out: Dict[str, dict] = {}
    for lo in range(0, len(files), BATCH):
        chunk_files = files[lo:lo + BATCH]
        msas, loci = [], []
        for f, m in zip(chunk_files, loaded[lo:lo + BATCH]):
            locus = remove_known_input_extensions(f.name)
            if isinstance(m, ValueError):
                if "No records found in handle" in str(m.args[0]):
                    raise EmptyMSAError(f"No records found in MSA of locus {locus}")
                raise m
            msas.append(m)
            loci.append(locus)
        _build_batch(msas, loci, options, backend, out)
    return out


def locus_record(locus: str, prg: str, builder, output_type) -> dict:
    """The per-locus output bytes of a run: PRG text, pickled builder (update_DS member), binary PRG, GFA — what the
    reference writes to per-locus temp files (subcommands/from_msa.py:114-133, subcommands/update.py:128-141)."""
    rec = dict(prg=prg)
    if output_type.prg:
        rec["pickle"] = pickle.dumps(builder, protocol=4)
    if output_type.binary:
        enc = PrgEncoder()
        arr = enc.encode_array(prg)
        rec["bin"] = (arr if arr is not None else np.asarray(enc.encode(prg))).astype("<u4").tobytes()
    if output_type.gfa:
        rec["gfa"] = GFA_Output.gfa_bytes(prg)
    return rec


def _build_batch(msas, loci, options, backend, out: Dict[str, dict], ring: int = 0):
    """ring: the set of pinned download buffers of the backend this batch's copies use (forest.assemble_prgs)."""
    from ..device import get_backend
    from ..prg_builder import PrgBuilder
    from ..recursion_tree import materialise
    if not msas:
        return
    be = backend or get_backend()
    ot = options.output_type

    def new_builder(locus, root_factory):
        return PrgBuilder(locus, None, options.alignment_format, options.max_nesting, options.min_match_length,
                          _root_factory=root_factory)

    # the array-at-a-time host assumes unique row ids inside an alignment; the rest keeps the id-based node host
    is_uniq = [len(set(m.ids)) == len(m.ids) for m in msas]
    uniq = [i for i, u in enumerate(is_uniq) if u]
    dup = [i for i, u in enumerate(is_uniq) if not u]
    if uniq:
        from ..forest import ForestEngine
        from ..recursion_tree import materialise_forest
        eng = ForestEngine(be, options.max_nesting, options.min_match_length)
        eng.load([msas[i] for i in uniq])
        eng.run_forest()
        prgs = eng.assemble_prgs(want_index=ot.prg, ring=ring)
        for j, i in enumerate(uniq):
            if prgs[j] is None:
                err = eng.errors[j]
                if not isinstance(err, SequenceCurationError):
                    raise err
                logger.warning(f"Skipping building PRG for {loci[i]}. Error: {err}")
                continue
            logger.info(f"Writing output files of locus {loci[i]}")
            builder = None
            if ot.prg:
                # the pickled builder must be what the reference serialises AFTER build_prg() (subcommands/from_msa.py:
                # 123-127): site counter advanced, every leaf allele in prg_index and in its leaf's indexed intervals —
                # `update` looks leaves up by these keys.  They come from the batch's index arrays, not from a second
                # traversal of the node objects.
                leaf_of = {}
                builder = new_builder(loci[i], lambda b, j=j, i=i: materialise_forest(eng, j, msas[i], b, leaf_of))
                builder.site_num = 5 + 2 * int(eng.site_count[j])
                for a, e, nid in eng.prg_index_entries(j).tolist():
                    builder.update_PRG_index(a, e, leaf_of[nid])
                if _CHECK_TREES:          # MPRG_CHECK=1: re-derive everything from the node objects (slow; tests do)
                    index, site = dict(builder.prg_index), builder.site_num
                    builder.clear_PRG_index()
                    assert builder.build_prg() == prgs[j] and builder.prg_index == index and builder.site_num == site
            out[loci[i]] = locus_record(loci[i], prgs[j], builder, ot)
    if dup:
        eng2 = BatchEngine(be, options.max_nesting, options.min_match_length)
        results = eng2.build([msas[i] for i in dup])
        for i, res in zip(dup, results):
            if res.error is not None:
                if not isinstance(res.error, SequenceCurationError):
                    raise res.error
                logger.warning(f"Skipping building PRG for {loci[i]}. Error: {res.error}")
                continue
            prg, _, _ = build_prg(eng2, res)
            builder = None
            if ot.prg:
                builder = new_builder(loci[i], lambda b, res=res, i=i: materialise(eng2, res, msas[i], b, None))
                assert builder.build_prg() == prg          # fills prg_index / site_num as the reference's build_prg() does
            out[loci[i]] = locus_record(loci[i], prg, builder, ot)


def _build_part(job):
    """One host worker process of `-t`: its share of the rank's files, built on the rank's GPU."""
    files, options = job
    options.threads = 1
    return build_shard(files, options)


def split_for_workers(files: List[Path], n: int) -> List[List[Path]]:
    """Size-balanced split of a rank's files over its host worker processes (same greedy rule as shard_files)."""
    return [p for p in balanced_parts(files, n) if p]


def _write_one(all_loci: Dict[str, dict], kind: str, output_prefix: str):
    single = len(all_loci) == 1
    if kind == "fa":
        with open(output_prefix + ".prg.fa", "w") as fh:
            for locus in sorted(all_loci, key=lambda l: l + ".prg.fa"):       # sorted temp-file paths in the reference
                fh.write(f">{locus}\n{all_loci[locus]['prg']}\n")
    elif kind == "pickle":
        zip_bytes(Path(output_prefix + ".update_DS.zip"), {l: all_loci[l]["pickle"] for l in all_loci})
    elif single:
        with open(f"{output_prefix}.prg.{kind}", "wb") as fh:
            fh.write(next(iter(all_loci.values()))[kind])
    else:
        zip_bytes(Path(f"{output_prefix}.prg.{kind}.zip"), {f"{l}.{kind}": all_loci[l][kind] for l in all_loci})


def write_final_files(all_loci: Dict[str, dict], output_type, output_prefix: str, parallel: bool = False):
    """reference utils/input_output_files.py:73-162.  parallel: one writer THREAD per output file — the containers are
    independent and a stored (uncompressed) zip member is a CRC-32 plus a write, both of which release the GIL; threads
    (not forked processes) so that a rank that has initialised the GPU can use them too."""
    kinds = (["fa", "pickle"] if output_type.prg else []) + (["bin"] if output_type.binary else []) + \
            (["gfa"] if output_type.gfa else [])
    if parallel and len(kinds) > 1 and len(all_loci) >= 256:
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(len(kinds)) as pool:
            list(pool.map(lambda k: _write_one(all_loci, k, output_prefix), kinds))
    else:
        for k in kinds:
            _write_one(all_loci, k, output_prefix)


# ---- the job's single exchange: every rank's segment INDEX to rank 0
GATHER_ROUND_BYTES = int(os.environ.get("MPRG_GATHER_ROUND_BYTES", str(1 << 30)))


def allgather_bytes(payload: bytes, dist, rank: int, world: int):
    """all_gather of the ranks' byte counts, then of the payloads as uint8 (RCCL moves device tensors, gloo host tensors), in rounds
    of at most GATHER_ROUND_BYTES per rank.  Returns the list of the ranks' payloads, on every rank.
    What travels is each rank's segment index (loci, record lengths, members' CRC / size / offset: ~100 bytes per locus) — the
    outputs themselves stay in the files the ranks wrote (utils/segments.py)."""
    import torch
    on_device = dist.get_backend() == "nccl"
    dev = torch.device("cuda", torch.cuda.current_device()) if on_device else torch.device("cpu")
    payload = np.frombuffer(payload, dtype=np.uint8)
    sizes = [torch.zeros(1, dtype=torch.int64, device=dev) for _ in range(world)]
    dist.all_gather(sizes, torch.tensor([payload.size], dtype=torch.int64, device=dev))
    sizes = [int(t.item()) for t in sizes]
    cap = max(max(sizes), 1)
    host = [np.empty(n, np.uint8) for n in sizes]
    for lo in range(0, cap, GATHER_ROUND_BYTES):
        n = min(GATHER_ROUND_BYTES, cap - lo)
        mine = torch.zeros(n, dtype=torch.uint8, device=dev)
        seg = payload[lo:lo + n]
        if seg.size:
            mine[:seg.size] = torch.from_numpy(seg.copy()).to(dev)
        parts = [torch.empty(n, dtype=torch.uint8, device=dev) for _ in range(world)]
        dist.all_gather(parts, mine)
        for r, t in enumerate(parts):
            take = max(0, min(sizes[r] - lo, n))
            if take:
                host[r][lo:lo + take] = t[:take].cpu().numpy()
        del parts, mine
    return [h.tobytes() for h in host]


def hip_runtimes_mapped() -> List[str]:
    """The distinct HIP runtime libraries mapped into this process (/proc/self/maps).  A rank runs the library's kernels AND
    torch.distributed (RCCL): both must sit on ONE copy of the runtime — two copies mean two sets of streams, devices and contexts
    that know nothing of each other."""
    seen = set()
    try:
        with open("/proc/self/maps") as fh:
            for line in fh:
                path = line.rsplit(None, 1)[-1] if "/" in line else ""
                if "libamdhip64" in os.path.basename(path):
                    seen.add(os.path.realpath(path))
    except OSError:
        pass
    return sorted(seen)


SHM_FRACTION = float(os.environ.get("MPRG_SEGMENT_SHM_FRACTION", "0.3"))          # of what /dev/shm and MemAvailable leave, all local ranks together
_SEGMENT_DIRS: List[str] = []                         # private in-memory directories of this process (removed at exit and on SIGTERM / SIGINT)


def _remove_segment_dirs():
    import shutil
    while _SEGMENT_DIRS:
        shutil.rmtree(_SEGMENT_DIRS.pop(), ignore_errors=True)


def _sweep_stale_segment_dirs(root: str = "/dev/shm"):
    """Directories of earlier runs of this user whose process is gone (a rank that was killed outright): their files are memory."""
    import shutil
    tag = f"mprg_{os.getuid()}_"
    try:
        names = [n for n in os.listdir(root) if n.startswith(tag)]
    except OSError:
        return
    for name in names:
        parts = name.split("_")
        try:
            pid = int(parts[2])
            os.kill(pid, 0)                           # (raises when no such process)
        except (IndexError, ValueError):
            continue
        except ProcessLookupError:
            path = os.path.join(root, name)
            if os.path.isdir(path) and not os.path.islink(path) and os.stat(path).st_uid == os.getuid():
                shutil.rmtree(path, ignore_errors=True)
        except PermissionError:
            pass


def _private_shm_dir() -> str:
    """A directory of this process alone in /dev/shm (mode 0700, name unpredictable: mkdtemp), removed when the process ends —
    normally, by an exception, or by the SIGTERM torchrun sends the peers of a rank that failed."""
    import atexit
    import signal
    import tempfile
    _sweep_stale_segment_dirs()
    path = tempfile.mkdtemp(prefix=f"mprg_{os.getuid()}_{os.getpid()}_", dir="/dev/shm")
    if not _SEGMENT_DIRS:
        atexit.register(_remove_segment_dirs)
        for sig in (signal.SIGTERM, signal.SIGINT):
            prev = signal.getsignal(sig)

            def handler(signum, frame, prev=prev):
                _remove_segment_dirs()
                if callable(prev):
                    prev(signum, frame)
                else:
                    signal.signal(signum, signal.SIG_DFL)
                    os.kill(os.getpid(), signum)
            try:
                signal.signal(sig, handler)
            except ValueError:                        # (not the main thread: atexit still runs)
                pass
    _SEGMENT_DIRS.append(path)
    return path


def segment_prefix(options, rank: int, files: List[Path]) -> str:
    """Where this rank writes its segment files: in memory when the shard's outputs fit comfortably (they are ~4x the inputs with
    -O a) — a PRIVATE directory under /dev/shm (_private_shm_dir), at most SHM_FRACTION of what is free there and in memory for all
    local ranks together —, else next to the run's output.  MPRG_SEGMENT_DIR overrides (MPRG_SEGMENT_DIR=/dev/shm forces the
    in-memory directory, any other value is used as it is)."""
    base = f"{os.path.basename(options.output_prefix)}.rank{rank}"
    seg_dir = os.environ.get("MPRG_SEGMENT_DIR")
    if seg_dir is None:
        seg_dir = os.path.dirname(os.path.abspath(options.output_prefix))
        try:
            need = 6 * sum(f.stat().st_size for f in files)
            st = os.statvfs("/dev/shm")
            avail_kib = int(next(l for l in open("/proc/meminfo") if l.startswith("MemAvailable")).split()[1])
            world_local = max(1, int(os.environ.get("LOCAL_WORLD_SIZE", os.environ.get("WORLD_SIZE", "1"))))
            if need * world_local < SHM_FRACTION * min(st.f_bavail * st.f_frsize, avail_kib * 1024):
                seg_dir = "/dev/shm"
        except Exception:
            pass
    if seg_dir == "/dev/shm":
        seg_dir = _private_shm_dir()
    return os.path.join(seg_dir, base)


def run_ranks(mine: List[Path], options, backend, dist, rank: int, world: int) -> int:
    """A rank of a multi-GPU run: its shard — a contiguous stretch of the run's sorted loci — through the streamed one-GPU pipeline
    into SEGMENT files of its own; the segment indexes all-gathered (the job's one collective); then every rank copies ITS bytes to
    their final offsets in the run's files, which rank 0 created and closes with the central directories (utils/segments.py) — in
    the reference's order: every output lists the loci sorted (utils/input_output_files.py:89).  Returns the number of loci built."""
    import copy
    import time
    from ..device import get_backend
    from ..pipeline import run_pipeline
    from ..utils import segments
    opts = copy.copy(options)
    opts.output_prefix = segment_prefix(options, rank, mine)
    t0 = time.perf_counter()

    def agree(ok: bool) -> bool:
        """AND over the ranks (a MIN all-reduce): a rank that failed on its own tells the others before the next collective."""
        import torch
        dev = torch.device("cuda", torch.cuda.current_device()) if dist.get_backend() == "nccl" else torch.device("cpu")
        flag = torch.tensor([1 if ok else 0], dtype=torch.int32, device=dev)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        return bool(int(flag.item()))

    try:
        idx, err = None, None
        try:
            idx = run_pipeline(mine, opts, backend or (lambda: get_backend("runtime")), segment=True)
            libs = hip_runtimes_mapped()
            if len(libs) > 1:
                raise RuntimeError("two HIP runtimes are mapped into this rank (" + ", ".join(libs) + "): the kernels' library and "
                                   "torch.distributed must share one — import torch before the backend is made")
        except Exception as e:          # noqa: BLE001 — told to the other ranks first
            err = e
        if not agree(err is None):
            raise err if err is not None else RuntimeError(f"rank {rank}: another rank failed while building its shard")
        t1 = time.perf_counter()
        got = allgather_bytes(segments.pack_index(idx), dist, rank, world)
        t2 = time.perf_counter()
        n = segments.merge_segments([segments.unpack_index(b) for b in got], options.output_prefix,
                                    sort_key=lambda locus: locus + ".prg.fa", rank=rank, world=world, barrier=dist.barrier, agree=agree)
        t3 = time.perf_counter()
        logger.info(f"rank {rank}: segments built and written in {t1 - t0:.2f}s, index exchange {t2 - t1:.2f}s, placed in the run's files in {t3 - t2:.2f}s")
        run_ranks.timings = dict(build_write_s=t1 - t0, exchange_s=t2 - t1, place_s=t3 - t2)
    finally:
        for suffix in (".prg.fa", ".prg.bin.zip", ".prg.gfa.zip", ".update_DS.zip"):          # (an error on the way: no stray segment)
            try:
                os.remove(opts.output_prefix + suffix)
            except OSError:
                pass
        _remove_segment_dirs()
    return n


def run(cl_options, backend=None):
    options = cl_options
    # `-t N`: the reference starts N per-alignment worker processes; here N host worker processes share the rank's GPU,
    # each building its part of the shard in resident batches (the array-at-a-time host control of one batch overlaps
    # the kernels of the others).  They are forked before this process touches the GPU (a forked HIP context is
    # unusable); with an explicit backend (tests) everything runs in-process.
    n_workers = max(1, int(getattr(options, "threads", 1) or 1)) if backend is None else 1
    pool = None
    # the streamed pipeline (one GPU, or every rank of several) runs its host stages on `-t` THREADS of this process; only the
    # object path (MPRG_PIPELINE=0, one rank) forks worker processes
    pipeline = int(os.environ.get("WORLD_SIZE", "1")) > 1 or os.environ.get("MPRG_PIPELINE", "1") != "0"
    if n_workers > 1 and not pipeline:
        import multiprocessing as mp
        pool = mp.get_context("fork").Pool(n_workers)
    tmp_dir = []
    try:
        if getattr(options, "unaligned", False):
            # the MSAs first (this rank's shard, on the GPU), then the unchanged path over the files written
            files = align_unaligned_inputs(options, backend, tmp_dir)
            return _run(options, backend, pool, n_workers, msa_files=files)
        return _run(options, backend, pool, n_workers)
    finally:
        if pool is not None:
            pool.close()
            pool.join()
        if tmp_dir:
            import shutil
            shutil.rmtree(tmp_dir[0], ignore_errors=True)


STAR_CHUNK = int(os.environ.get("MPRG_STAR_CHUNK", "2048"))          # loci read, aligned and written per round of --unaligned


def align_unaligned_inputs(options, backend, tmp_dir: list) -> List[Path]:
    """--unaligned: this rank's shard of the input files (unaligned FASTA), their centre-star MSAs built on the GPU in chunks of
    loci and written as <locus>.fa into --msa-dir, or into a private temporary directory beside the output prefix (appended to
    tmp_dir; the caller removes it).  Returns the files written, in the shard's order."""
    import tempfile
    import time
    from ..device import get_backend
    from ..from_msa import star_align
    rank, world, _ = _dist()
    input_files = get_all_input_files(options.input, options.suffix)
    if len(input_files) == 0:
        raise FileNotFoundError(f"No input files found in {options.input}")
    seen: Dict[str, Path] = {}
    for f in input_files:
        locus = remove_known_input_extensions(f.name)
        if locus in seen:
            raise ValueError(f"{seen[locus]} and {f} map to the same locus name {locus}")
        seen[locus] = f
    if not options.force and output_files_already_exist(options.output_type, options.output_prefix):
        raise RuntimeError("One or more output files already exists, aborting run...")
    mine = shard_files(input_files, rank, world) if world > 1 else input_files
    loci = [remove_known_input_extensions(f.name) for f in mine]
    Path(options.output_prefix).parent.mkdir(parents=True, exist_ok=True)
    if getattr(options, "msa_dir", None) is not None:
        out_dir = Path(options.msa_dir)
        out_dir.mkdir(parents=True, exist_ok=True)
        if not options.force:
            clash = [l for l in loci if (out_dir / f"{l}.fa").exists()]
            if clash:
                raise RuntimeError(f"{out_dir / (clash[0] + '.fa')} already exists (and {len(clash) - 1} more): aborting run (-F overwrites)")
    else:
        parent = os.path.dirname(os.path.abspath(options.output_prefix))
        tmp_dir.append(tempfile.mkdtemp(prefix=f".{os.path.basename(options.output_prefix)}.msa.rank{rank}.", dir=parent))
        out_dir = Path(tmp_dir[0])
    be = backend or get_backend("runtime")
    t_read = t_align = t_write = 0.0
    written = []
    counters: Dict[str, float] = {}
    # (argparse attribute, star_msas keyword, kind: a flag is passed as True, a count as its number); each only when set, a keyword of
    # `lists` with the list that receives its per-locus reports, and timings when an option with counters of its own is set
    table = (("adjust_direction", "adjust_direction", "flag"), ("band", "band", "flag"), ("collapse_identical", "collapse", "flag"),
             ("refine", "refine", "count"), ("progressive", "progressive", "flag"), ("device_tree", "device_tree", "flag"),
             ("large_loci", "large_loci", "flag"), ("refine_tree", "refine_tree", "count"), ("retree", "retree", "count"),
             ("seq_weights", "seq_weights", "flag"), ("pair_distances", "pair_distances", "flag"), ("position_gaps", "position_gaps", "flag"),
             ("free_end_gaps", "free_end_gaps", "flag"), ("free_end_pairs", "free_end_pairs", "flag"),
             ("free_end_distances", "free_end_distances", "flag"))
    lists = dict(adjust_direction="orientation", refine="refinement", progressive="progression", refine_tree="tree_refinement")
    on = {key: bool(getattr(options, attr, False)) if kind == "flag" else int(getattr(options, attr, None) or 0) for attr, key, kind in table}
    kw = {key: value for key, value in on.items() if value}
    if any(key not in ("adjust_direction", "refine", "progressive", "large_loci") for key in kw):
        kw["timings"] = counters
    kw.update({lists[key]: [] for key in lists if key in kw})
    adjust, band, progressive, refine, refine_tree, retree = (on[key] for key in ("adjust_direction", "band", "progressive", "refine", "refine_tree", "retree"))
    orientation, refinement, progression, tree_refinement = (kw.get(name, []) for name in lists.values())
    for lo in range(0, len(mine), STAR_CHUNK):
        t0 = time.perf_counter()
        recs = [star_align.read_unaligned(f) for f in mine[lo:lo + STAR_CHUNK]]
        t1 = time.perf_counter()
        msas = star_align.star_msas(be, recs, names=loci[lo:lo + STAR_CHUNK], **kw)
        t2 = time.perf_counter()
        for locus, m in zip(loci[lo:lo + STAR_CHUNK], msas):
            path = out_dir / f"{locus}.fa"
            with open(path, "w") as fh:
                fh.write(star_align.msa_fasta(m))
            written.append(path)
        t_read, t_align, t_write = t_read + t1 - t0, t_align + t2 - t1, t_write + time.perf_counter() - t2
    logger.info(f"rank {rank}: {len(written)} centre-star MSAs: read {t_read:.2f}s, aligned {t_align:.2f}s, written {t_write:.2f}s "
                f"into {out_dir}")
    if adjust:
        logger.info(f"rank {rank}: --adjust-direction: {sum(sum(rev) for rev, _ in orientation)} records reverse-complemented, "
                    f"{sum(how.count('d') + how.count('t') for _, how in orientation)} settled by DP")
    if band:
        logger.info(f"rank {rank}: --band: {counters.get('band_pairs', 0)} pairs, {counters.get('band_second_passes', 0)} second passes, "
                    f"{counters.get('band_full_pairs', 0)} sent to the full DP, {counters.get('band_cells', 0)} of "
                    f"{counters.get('band_full_cells', 0)} DP cells computed")
    if band and progressive:
        logger.info(f"rank {rank}: --progressive --band: {counters.get('prog_band_merges', 0)} merges, "
                    f"{counters.get('prog_band_second_passes', 0)} second passes, {counters.get('prog_band_full_merges', 0)} sent to the "
                    f"full DP, {counters.get('prog_band_cells', 0)} of {counters.get('prog_band_full_cells', 0)} DP cells computed")
    if on["position_gaps"]:
        logger.info(f"rank {rank}: --position-gaps: {counters.get('position_gap_merges', 0)} merges with opens by occupancy")
    if on["free_end_gaps"]:
        logger.info(f"rank {rank}: --free-end-gaps: {counters.get('free_end_gap_merges', 0)} merges with free end gaps")
    if on["free_end_pairs"]:
        logger.info(f"rank {rank}: --free-end-pairs: {counters.get('free_end_pair_alignments', 0)} pair alignments with free ends")
    if on["free_end_distances"]:
        logger.info(f"rank {rank}: --free-end-distances: {counters.get('free_end_distance_pairs', 0)} pair scores with free ends")
    if on["pair_distances"]:
        logger.info(f"rank {rank}: --pair-distances: {counters.get('pair_dist_loci', 0)} loci, {counters.get('pair_dist_pairs', 0)} pairs, "
                    f"{counters.get('pair_dist_cells', 0)} DP cells, {counters.get('pair_dist_above_cap', 0)} above the cap, "
                    f"{counters.get('pair_dist_limit', 0)} beyond the limit")
    if on["seq_weights"]:
        logger.info(f"rank {rank}: --seq-weights: {counters.get('seq_weight_loci', 0)} loci weighted, "
                    f"smallest weight {counters.get('seq_weight_min_q', 1)}")
    if retree:
        logger.info(f"rank {rank}: --retree {retree}: {counters.get('retree_rebuilds', 0)} loci rebuilt, "
                    f"{counters.get('retree_accepted', 0)} accepted, {counters.get('retree_same_tree', 0)} same tree, "
                    f"{counters.get('retree_refused', 0)} refused")
    if refine_tree:
        logger.info(f"rank {rank}: --refine-tree {refine_tree}: {sum(1 for t in tree_refinement if t and t[1])} loci refined, "
                    f"{counters.get('tree_refine_steps', 0)} steps tried, {counters.get('tree_refine_accepted', 0)} accepted, "
                    f"{counters.get('tree_refine_skipped', 0)} skipped, {counters.get('tree_refine_above_cap', 0)} loci above the cap of "
                    f"{star_align.TREE_REFINE_MAX_LEAVES} leaves")
    if refine:
        logger.info(f"rank {rank}: --refine {refine}: {sum(1 for a, _, _ in refinement if a)} loci refined, "
                    f"{sum(a for a, _, _ in refinement)} rounds accepted, {sum(1 for a, _, _ in refinement if not a)} loci left as the star MSA")
    if on["collapse"]:
        logger.info(f"rank {rank}: --collapse-identical: {counters.get('collapse_records', 0)} records, "
                    f"{counters.get('collapse_classes', 0)} classes")
    if progressive:
        built = [(n, r) for n, r, star in progression if not star]
        logger.info(f"rank {rank}: --progressive: {len(built)} loci built, {sum(n - 1 for n, _ in built)} merges, "
                    f"{max((r for _, r in built), default=0)} rounds at most, {len(progression) - len(built)} loci left to the star pass")
    if on["device_tree"]:
        logger.info(f"rank {rank}: --device-tree: {counters.get('tree_device_loci', 0)} loci's trees built on the device")
    if on["large_loci"]:
        logger.info(f"rank {rank}: --large-loci: {counters.get('large_loci', 0)} loci of more than {star_align.PROG_MAX_LEAVES} records built "
                    f"progressively ({counters.get('large_records', 0)} records), {counters.get('large_fallbacks', 0)} over a limit")
    align_unaligned_inputs.timings = dict(read_s=t_read, align_s=t_align, write_s=t_write)
    return written


def _run(options, backend, pool, n_workers, msa_files: Optional[List[Path]] = None):
    """msa_files: the inputs are these files, already this rank's shard (--unaligned); else options.input / suffix, sharded."""
    rank, world, dist = _dist()
    input_files = get_all_input_files(options.input, options.suffix) if msa_files is None else msa_files
    if len(input_files) == 0:
        raise FileNotFoundError(f"No input files found in {options.input}")
    if not options.force and output_files_already_exist(options.output_type, options.output_prefix):
        raise RuntimeError("One or more output files already exists, aborting run...")
    Path(options.output_prefix).parent.mkdir(parents=True, exist_ok=True)
    mine = shard_files(input_files, rank, world) if world > 1 and msa_files is None else input_files
    import time
    t0 = time.time()
    if dist is None and len(mine) > 1 and os.environ.get("MPRG_PIPELINE", "1") != "0":
        # one GPU: the streamed file -> file pipeline (native batch parser and encoders with `-t` threads, chunks of
        # alignments resident on the device, containers written while the next chunk builds); make_prg_amd/pipeline.py
        from ..device import get_backend
        from ..pipeline import run_pipeline
        n_built = run_pipeline(mine, options, backend or (lambda: get_backend("runtime")))
        logger.info(f"{n_built} of {len(mine)} loci built and written in {time.time() - t0:.1f}s ({max(1, int(getattr(options, 'threads', 1) or 1))} host threads)")
        if n_built == 0:
            logger.error("No PRGs were built, please check errors")
        return
    if dist is not None:
        # several GPUs: every rank streams its shard into segment files, rank 0 merges them by an index (run_ranks)
        import torch
        n_built = run_ranks(mine, options, backend, dist, rank, world)
        logger.info(f"rank {rank}: shard of {len(mine)} loci built and written in {time.time() - t0:.1f}s")
        if dist.get_backend() == "nccl":
            torch.cuda.synchronize()
        dist.barrier()          # (the segments are merged and removed: every rank may leave)
        if rank == 0:
            logger.info(f"{n_built} loci in the merged output files after {time.time() - t0:.1f}s ({world} ranks)")
            if n_built == 0:
                logger.error("No PRGs were built, please check errors")
        if _dist.we_initialised:
            dist.destroy_process_group()
        return
    if pool is not None and len(mine) >= 2 * n_workers:
        # several parts per worker, collected as they finish: the writer-side unpickling of one part overlaps the
        # building of the others (the per-locus outputs are ~0.5 MB each)
        n_parts = max(n_workers, min(4 * n_workers, len(mine) // 256))
        local = {}
        for part in pool.imap_unordered(_build_part, [(p, options) for p in split_for_workers(mine, n_parts)]):
            local.update(part)
    else:
        local = build_shard(mine, options, backend)
    logger.info(f"rank {rank}: {len(local)} of {len(mine)} loci built in {time.time() - t0:.1f}s ({n_workers} host workers)")
    t0 = time.time()
    if not local:
        logger.error("No PRGs were built, please check errors")
        return
    write_final_files(local, options.output_type, options.output_prefix, parallel=True)
    logger.info(f"output files written in {time.time() - t0:.1f}s")
