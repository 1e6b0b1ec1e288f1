"""`compare_msa` sub-command (this implementation; the reference has no counterpart): test MSAs scored against reference MSAs of
the same records on the GPU (make_prg_amd/from_msa/msa_compare.py holds the statement): the aligned residue pairs and the columns
the two alignments share, as FastSP, qscore and bali_score report them.

    python -m make_prg_amd compare_msa -i TEST -r REF [-s SUFFIX] [-f FORMAT] [-o TSV]

TEST and REF are two files, or two directories whose files are paired by name (a trailing .gz is ignored).  The output is a TSV:
a header, one line per locus and a `total` line, each with the six counts, the four ratios to six decimals (NA: the denominator
is 0) and why the locus was not scored (-: it was)."""
import logging
import sys
from pathlib import Path
from typing import Dict, List, Tuple

from ..msa import load_alignment_file
from ..utils.io_utils import remove_known_input_extensions

logger = logging.getLogger("make_prg_amd")
HEADER = ("locus", "shared", "ref_pairs", "test_pairs", "ref_columns", "kept_columns", "identical_columns", "SP", "Modeler", "TC", "CS",
          "skipped")


def register_parser(subparsers):
    p = subparsers.add_parser("compare_msa", usage="make_prg compare_msa -i TEST -r REF [-s SUFFIX] [-f FORMAT] [-o TSV]",
                              help="(this implementation) Score MSAs against reference MSAs of the same records on the GPU")
    p.add_argument("-i", "--input", action="store", type=str, required=True,
                   help="The test MSA: a file, or a directory containing such files")
    p.add_argument("-r", "--reference", action="store", type=str, required=True,
                   help="The reference MSA: a file if the input is a file, else a directory whose files have the input files' names "
                        "(a trailing .gz is ignored when pairing)")
    p.add_argument("-s", "--suffix", action="store", type=str, default="",
                   help="With directories: only the files with this suffix (before a trailing .gz) are considered")
    p.add_argument("-f", "--alignment-format", dest="alignment_format", action="store", default="fasta",
                   help="Alignment format of both sides, or TEST_FORMAT,REF_FORMAT: every format from_msa -f reads. Default: %(default)s")
    p.add_argument("-o", "--output", action="store", type=str, default=None, help="The TSV file to write. Default: stdout")
    p.add_argument("-v", "--verbose", action="count", default=0, help="Increase output verbosity")
    p.add_argument("--log", help="Path to write log to. Default is stderr")
    p.set_defaults(func=run, check=lambda args, _from_msa_parser: check_options(args, p))
    return p


def _key(name: str) -> str:
    return name[:-3] if name.endswith(".gz") else name


def _side(path: Path, suffix: str) -> Dict[str, Path]:
    return {_key(f.name): f for f in sorted(path.iterdir()) if f.is_file() and _key(f.name).endswith(suffix)}


def check_options(args, parser):
    """What argparse cannot refuse by itself: the formats, and the pairing of the two sides (args.pairs: (locus, test, reference))."""
    from ..utils.align_formats import FORMATS
    fmts = args.alignment_format.lower().split(",")
    if len(fmts) > 2 or any(f != "fasta" and f not in FORMATS for f in fmts):
        parser.error(f"-f takes FORMAT or TEST_FORMAT,REF_FORMAT over fasta, {', '.join(sorted(FORMATS))}, not {args.alignment_format}")
    args.formats = (fmts[0], fmts[-1])
    test, ref = Path(args.input), Path(args.reference)
    for p in (test, ref):
        if not p.exists():
            parser.error(f"{p} does not exist")
    if test.is_dir() != ref.is_dir():
        parser.error("-i and -r take two files or two directories")
    if not test.is_dir():
        args.pairs = [(remove_known_input_extensions(test.name), test, ref)]
        return
    a, b = _side(test, args.suffix), _side(ref, args.suffix)
    only = [f"{n} (only in {test})" for n in sorted(set(a) - set(b))] + [f"{n} (only in {ref})" for n in sorted(set(b) - set(a))]
    if only:
        parser.error("files without a partner: " + ", ".join(only))
    if not a:
        parser.error(f"no input files found in {test}")
    args.pairs = [(remove_known_input_extensions(n), a[n], b[n]) for n in sorted(a)]


def _cell(x) -> str:
    return "NA" if x is None else f"{x:.6f}"


def tsv_line(name: str, c) -> str:
    return "\t".join([name, *(str(int(v)) for v in c[:6]), _cell(c.sp), _cell(c.modeler), _cell(c.tc), _cell(c.cs), c.skipped or "-"])


def tsv(names: List[str], comparisons) -> str:
    from ..from_msa.msa_compare import total
    return "".join(line + "\n" for line in ["\t".join(HEADER)] + [tsv_line(n, c) for n, c in zip(names, comparisons)] +
                   [tsv_line("total", total(comparisons))])


def run(args, backend=None):
    from ..device import get_backend
    from ..from_msa.msa_compare import compare_msas
    pairs: List[Tuple[str, Path, Path]] = args.pairs
    names = [n for n, _, _ in pairs]
    # (defer_n: an N stays an N: it is a residue here, not a base to be guessed from its column)
    tests = [load_alignment_file(t, args.formats[0], defer_n=True) for _, t, _ in pairs]
    refs = [load_alignment_file(r, args.formats[1], defer_n=True) for _, _, r in pairs]
    be = backend or get_backend("runtime")
    comparisons = compare_msas(be, tests, refs, names=names)
    text = tsv(names, comparisons)
    if args.output is None:
        sys.stdout.write(text)
    else:
        Path(args.output).parent.mkdir(parents=True, exist_ok=True)
        Path(args.output).write_text(text)
    skipped = sum(1 for c in comparisons if c.skipped)
    logger.info(f"{len(pairs) - skipped} loci compared, {skipped} skipped")
