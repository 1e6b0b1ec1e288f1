"""Centre-star MSAs of `from_msa --unaligned`: every locus's unaligned sequences aligned on the GPU against one of them, the
centre, and the insertions merged (kernels: csrc/k_star.inc for the centre and the merge, csrc/k_align.inc for the pairs; C ABI:
mprg_star_centres / mprg_star_merge_columns / mprg_star_merge_rows / mprg_align_profiles / mprg_align_pairs in include/mprg.h).

It is NOT MAFFT.  PRGs built from these alignments differ from PRGs built from a MAFFT alignment of the same sequences.

Spec (the kernels and tests/star_ref.py follow it bit for bit)
  Input.    A locus is the records of one FASTA(.gz) file, in file order.  Each sequence is upper-cased and every '-' removed.
            Only ACGT-RYKMSWN are allowed; any other character is an error that names the locus and the record.
  Centre.   k-mers of k = 6 over ACGT only (a window with any other code is skipped).  c_a: the 4 096 counts of sequence a;
            T = sum over b of c_b; score(a) = <c_a, T> - <c_a, c_a> in int64 (= sum over b != a of <c_a, c_b>).  The centre is the
            smallest index a of a NON-EMPTY sequence that maximises score.  A locus with no records raises from_msa's
            EmptyMSAError; a locus whose sequences are all empty is an error that names it.
  Pairs.    The centre is a 1-row leaf; every other non-empty sequence is aligned against it with exactly the DP, scores and tie
            order of make_prg_amd/update/profile_align.py.  An empty sequence aligns as C deletions, no launch.
  Merge.    As profile_align.merge: boundary j (0..C) gets max_k ins_k(j) new columns, each sequence's inserted residues
            left-justified in them.  Rows in INPUT order (the centre stays at its own index), letters upper case, titles the
            records' original header lines.  (So a locus of one record is that record.)
  Invariants (tested):
            - every row with its gaps removed is its input sequence;
            - no column is all gaps;
            - identical input sequences give identical rows;
            - two equal-length sequences that differ by one substitution align without gaps: a gap-free alignment scores at
              least (L - 1) * 1280 - 576, any gapped one needs an insertion and a deletion, so at most (L - 1) * 1280 - 2688.

Host side: loci in chunks (CHUNK_BYTES of estimated ops and output per chunk); per chunk the centres in one launch, the pairs
through profile_align.pairs_on_device (longest first, workspace-budget launches, ops left on the device), the widths and column
starts in one call, the output size downloaded (one int64 per locus), the rows in one more launch, the MSAs downloaded.
"""
from typing import List, Optional, Sequence, Tuple

import numpy as np

from ..msa import MSA, encode
from ..update import profile_align as pa

K = 6
LOCUS_FIELDS, ROW_FIELDS = 4, 6           # MPRG_ST_LOCUS_FIELDS, MPRG_ST_ROW_FIELDS
CENTRE_BAD = -2                           # MPRG_ST_CENTRE_BAD
ROW_STATUS = {1: "row fields or ops inconsistent with the buffers", 2: "output row outside the buffer"}
CHUNK_BYTES = 1 << 29                     # estimated ops + output bytes of the loci of one chunk
_GAP = ord("-")
_ASCII = np.frombuffer(b"ACGT-RYKMSWN", np.uint8)


class StarAlignError(ValueError):
    pass


def locus_codes(name: str, records: Sequence[Tuple[str, str]]) -> List[np.ndarray]:
    """The locus's sequences as gap-free cell codes (upper-cased, '-' removed); a character outside ACGT-RYKMSWN is an error."""
    out = []
    for i, (title, seq) in enumerate(records):
        raw = np.frombuffer(seq.encode(), np.uint8)
        raw = np.where((raw >= ord("a")) & (raw <= ord("z")), raw - 32, raw).astype(np.uint8)
        raw = raw[raw != _GAP]
        codes = encode(raw)
        if (codes == 255).any():
            bad = chr(raw[int(np.argmax(codes == 255))]) if raw.max() < 128 else "non-ASCII"
            raise StarAlignError(f"locus {name}, record {i + 1} ({title}): character {bad!r} outside ACGT-RYKMSWN")
        out.append(codes)
    return out


def _chunks(codes: List[List[np.ndarray]], limit: int):
    lo, used = 0, 0
    for k, cs in enumerate(codes):
        longest = max((len(c) for c in cs), default=0)
        est = 3 * len(cs) * (2 * longest + 1)
        if k > lo and used + est > limit:
            yield lo, k
            lo, used = k, 0
        used += est
    if lo < len(codes):
        yield lo, len(codes)


def star_msas(backend, loci: Sequence[Sequence[Tuple[str, str]]], names: Optional[Sequence[str]] = None,
              budget_bytes: int = pa.DEFAULT_BUDGET_BYTES, chunk_bytes: int = CHUNK_BYTES, timings: Optional[dict] = None) -> List[MSA]:
    """loci: per locus its records as (title, sequence).  Returns the loci's centre-star MSAs (ids: the titles' first words,
    descriptions: the titles).  names: the loci's names for error messages (default: their indices).  timings: a dict that
    receives the wall seconds of the stages (centre, pairs, merge: each ends at a download, so includes its kernels)."""
    names = [str(i) for i in range(len(loci))] if names is None else list(names)
    for name, recs in zip(names, loci):
        if not len(recs):
            from ..subcommands.from_msa import EmptyMSAError
            raise EmptyMSAError(f"No records found in MSA of locus {name}")
    codes = [locus_codes(n, recs) for n, recs in zip(names, loci)]
    out: List[MSA] = []
    for lo, hi in _chunks(codes, chunk_bytes):
        out.extend(_star_chunk(backend, loci[lo:hi], codes[lo:hi], names[lo:hi], budget_bytes, timings))
    return out


def centres(backend, codes: Sequence[Sequence[np.ndarray]]) -> np.ndarray:
    """mprg_star_centres over the loci (per locus its gap-free code arrays): the centre index per locus, -1 if all are empty."""
    return _centres(backend, *_pack(backend, codes))[0]


def _pack(be, codes):
    flat = [c for cs in codes for c in cs]
    lens = np.array([len(c) for c in flat], np.int64)
    seq_off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    counts = np.array([len(cs) for cs in codes], np.int64)
    first = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)
    host = np.concatenate(flat + [np.zeros(1, np.uint8)]).astype(np.uint8)
    return host, lens, seq_off, first, counts


def _centres(be, host, lens, seq_off, first, counts):
    for l in range(len(counts)):
        if int(lens[first[l]:first[l] + counts[l]].sum()) >= 1 << 32:
            raise StarAlignError("a locus of 2^32 residues or more")
    d_codes = be.upload(host)
    d_seqs = be.upload(np.stack([seq_off, lens], 1).reshape(-1))
    ltab = np.zeros((len(counts), LOCUS_FIELDS), np.int64)
    ltab[:, 0], ltab[:, 1] = first, counts
    d_loci = be.upload(ltab)
    d_centre = be.empty(4 * len(counts))
    be.call("mprg_star_centres", be.ptr(d_codes), len(host), be.ptr(d_seqs), len(lens), be.ptr(d_loci), len(counts),
            be.ptr(d_centre), be.stream, work=float(3 * lens.sum()))
    centre = be.download(d_centre, np.int32, len(counts)).astype(np.int64)
    if (centre == CENTRE_BAD).any():
        raise StarAlignError("mprg_star_centres: a locus's sequences lie outside the buffers")
    return centre, d_codes


def _star_chunk(be, loci, codes, names, budget_bytes, timings=None) -> List[MSA]:
    import time
    t0 = time.perf_counter()
    host, lens, seq_off, first, counts = _pack(be, codes)
    centre, d_codes = _centres(be, host, lens, seq_off, first, counts)
    t1 = time.perf_counter()
    for l in np.nonzero(centre < 0)[0]:
        raise StarAlignError(f"locus {names[l]}: every sequence is empty")
    n_loci = len(codes)
    C = np.array([len(codes[l][centre[l]]) for l in range(n_loci)], np.int64)
    # the pairs: the centre as a 1-row leaf, every other non-empty sequence against it
    leaves = [codes[l][centre[l]].reshape(1, -1) for l in range(n_loci)]
    others = [[a for a in range(len(cs)) if a != centre[l] and len(cs[a])] for l, cs in enumerate(codes)]
    dp = pa.pairs_on_device(be, leaves, [[codes[l][a] for a in others[l]] for l in range(n_loci)], budget_bytes)
    t2 = time.perf_counter()
    # rows in input order: {locus, sequence offset, n, ops offset, ops count (-1: residue i in column i), output offset}
    rows = np.zeros((int(counts.sum()), ROW_FIELDS), np.int64)
    rows[:, 0] = np.repeat(np.arange(n_loci), counts)
    rows[:, 1], rows[:, 2], rows[:, 4] = seq_off, lens, -1
    if dp is not None:
        r = first[dp.leaf] + np.array([others[l][i] for l, i in zip(dp.leaf.tolist(), dp.index.tolist())], np.int64)
        rows[r, 3], rows[r, 4] = dp.ops_off, dp.count
    d_ops = dp.d_ops if dp is not None else be.empty(16)
    ops_bytes = dp.ops_bytes if dp is not None else 0
    woff = np.concatenate([[0], np.cumsum(C + 1)[:-1]]).astype(np.int64)
    n_width = int((C + 1).sum())
    ltab = np.stack([first, counts, C, woff], 1).astype(np.int64)
    d_loci, d_rows = be.upload(ltab), be.upload(rows)
    d_width, d_start = be.zeros(4 * n_width), be.empty(8 * n_width)
    d_w, d_status = be.empty(8 * n_loci), be.empty(4 * len(rows))
    be.call("mprg_star_merge_columns", be.ptr(d_ops), ops_bytes, be.ptr(d_rows), len(rows), be.ptr(d_loci), n_loci, be.ptr(d_width),
            be.ptr(d_start), n_width, len(host), be.ptr(d_w), be.ptr(d_status), be.stream, work=float(ops_bytes))
    W = be.download(d_w, np.int64, n_loci)
    _check(be.download(d_status, np.int32, len(rows)), "mprg_star_merge_columns")
    if (W < C).any():
        raise StarAlignError("mprg_star_merge_columns: a locus's boundaries lie outside the buffers")
    base = np.concatenate([[0], np.cumsum(counts * W)[:-1]]).astype(np.int64)
    rank = np.arange(len(rows)) - np.repeat(first, counts)
    rows[:, 5] = np.repeat(base, counts) + rank * np.repeat(W, counts)
    out_bytes = int((counts * W).sum())
    d_rows, d_out = be.upload(rows), be.empty(max(out_bytes, 1))
    be.call("mprg_star_merge_rows", be.ptr(d_codes), len(host), be.ptr(d_ops), ops_bytes, be.ptr(d_rows), len(rows), be.ptr(d_loci),
            n_loci, be.ptr(d_width), be.ptr(d_start), n_width, be.ptr(d_w), be.ptr(d_out), max(out_bytes, 1), be.ptr(d_status),
            be.stream, work=float(out_bytes + ops_bytes))
    _check(be.download(d_status, np.int32, len(rows)), "mprg_star_merge_rows")
    text = be.download(d_out, np.uint8, out_bytes)
    msas = []
    for l, recs in enumerate(loci):
        data = text[base[l]:base[l] + counts[l] * W[l]].reshape(int(counts[l]), int(W[l]))
        titles = [t for t, _ in recs]
        msas.append(MSA(_data=data, _ids=[(t.split(None, 1) or [""])[0] for t in titles], _descs=titles))
    if timings is not None:
        for k, v in (("centre_s", t1 - t0), ("pairs_s", t2 - t1), ("merge_s", time.perf_counter() - t2)):
            timings[k] = timings.get(k, 0.0) + v
    return msas


def _check(status: np.ndarray, what: str):
    bad = np.nonzero(status)[0]
    if len(bad):
        raise StarAlignError(f"{what}: row {bad[0]}: {ROW_STATUS.get(int(status[bad[0]]), int(status[bad[0]]))}")


# ---- files
def read_unaligned(path) -> List[Tuple[str, str]]:
    """The records of an unaligned FASTA(.gz) file as (title: the header line without '>', sequence: its lines joined, white
    space removed), in file order."""
    import gzip
    from ..msa import _parse_fasta
    path = str(path)
    opener = gzip.open if path.endswith(".gz") else open
    with opener(path, "rt") as fh:
        return list(_parse_fasta(fh.read()))


def msa_fasta(msa: MSA) -> str:
    """One header line (the record's title) and one sequence line per row."""
    return "".join(f">{t}\n{msa.data[i].tobytes().decode()}\n" for i, t in enumerate(msa.descriptions))
