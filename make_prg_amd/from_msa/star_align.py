"""Centre-star MSAs of `from_msa --unaligned`: every locus's unaligned sequences aligned on the GPU against one of them, the
centre, and the insertions merged (kernels: csrc/k_star.inc for the centre and the merge, csrc/k_align.inc for the pairs; C ABI:
mprg_star_centres / mprg_star_merge_columns / mprg_star_merge_rows / mprg_align_profiles / mprg_align_pairs in include/mprg.h).
With `--band` the pairs are computed over a certified band of diagonals in two passes (the spec and the proof that the ops are the
full DP's: make_prg_amd/update/profile_align.py, "Band"; C ABI: mprg_align_bounds / mprg_align_pairs_banded): the same MSAs, byte
for byte, from a fraction of the cells and of the traceback memory.
With `--adjust-direction`, records on the opposite strand are found and reverse-complemented first (Orientation below; kernels in
csrc/k_star.inc, C ABI: mprg_star_centres_canonical / mprg_star_strand / mprg_star_revcomp).

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

Orientation (only with adjust_direction; integers only; tests/strand_ref.py follows it bit for bit).  Per locus, after Input:
  rc(s).    s reversed, with A<->T, C<->G, R<->Y, K<->M, and S, W, N unchanged (cell codes 0<->3, 1<->2, 5<->6, 7<->8).  For a 6-mer
            index k (12 bits, the first base in the top two bits), rc6(k): 4095 - k, then its six 2-bit groups in reverse order.
  Centre^.  The Centre rule over CANONICAL counts: every valid window counts in bin min(k, rc6(k)); the same score and the same
            lowest-index tie rule.  It does not change when any subset of the records is reverse-complemented.
  ref.      The lexicographically smaller (in cell codes) of the sequence of Centre^ and its rc: independent of the orientation in
            which that record arrived.
  Evidence  of every other non-empty sequence a, with h the forward 6-mer counts of ref: fwd = sum of h[k_w], rev = sum of
            h[rc6(k_w)] over a's valid windows w, nw their number (int64).
  Decision  opp(a): a lies on the strand opposite to ref.  By k-mers when 8 |fwd - rev| >= max(nw, 1): opp = rev > fwd.  Else by
            DP: a and rc(a) are both aligned against ref as a 1-row leaf with the DP of Pairs, only the scores are used:
            opp = score(rc(a)) > score(a); on equal scores opp = rc(a) < a (cell codes).  (A pair and its joint reverse
            complement have the same optimal score, so this keeps the result independent of a's input orientation.)
            opp(Centre^) = its sequence is not ref.  An empty sequence is never reversed.
  Anchor.   reversed(a) = opp(a) XOR opp(first), first = the first non-empty record: it always keeps its input orientation
            (MAFFT's --adjustdirection convention), everything else follows it.
  Then      Centre, Pairs and Merge above, unchanged, on the oriented sequences (rc(s_a) where reversed(a)); rows stay in input
            order; the title of a reversed record gets the prefix _R_ (the id is the new title's first word).
  how.      Per sequence one of: - not examined (Centre^, an empty sequence, a single record), k k-mers, d DP, t DP tie.
  The constants (k = 6, the factor 8) are design choices: 6 reuses the 4 096-bin tables that fit LDS; the factor only decides who
  pays for two extra small DPs, never correctness, because an undecided sequence is settled by the alignment scores.
  Properties (tested): the output equals the flag-off output on the records with `reversed` applied and _R_ prefixed; an input
  in which nothing is reversed gives the flag-off bytes; reverse-complementing any records but the first non-empty one changes no
  row; every row with its gaps removed is its input sequence or, exactly where the title starts with _R_, its rc.

Host side: loci in chunks (CHUNK_BYTES of estimated ops and output per chunk); per chunk the centres in one launch, the pairs
through profile_align.pairs_on_device (longest first, workspace-budget launches, ops left on the device), the widths and column
starts in one call, the output size downloaded (one int64 per locus), the rows in one more launch, the MSAs downloaded.
With adjust_direction, per chunk in front of that: the residues uploaded once, the canonical centres and the evidence in two
launches (the centres stay on the device between them), the decisions in NumPy, one small pairs_on_device call for the undecided
sequences in both orientations (none when there are none), one mprg_star_revcomp launch that writes the reversed records into a
tail of the code buffer, to which the sequence table then points: the centre and merge kernels read oriented sequences from that
buffer.  The pair stage uploads its sequences from host arrays, so it gets the host-side rc of the reversed records only.
"""
from typing import List, Optional, Sequence, Tuple

import numpy as np

from ..msa import MSA, encode
from ..update import profile_align as pa

K = 6
LOCUS_FIELDS, ROW_FIELDS = 4, 6           # MPRG_ST_LOCUS_FIELDS, MPRG_ST_ROW_FIELDS
CENTRE_BAD = -2                           # MPRG_ST_CENTRE_BAD
REVERSED_PREFIX = "_R_"                   # of the title of a record that --adjust-direction reverse-complemented
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
              budget_bytes: int = pa.DEFAULT_BUDGET_BYTES, chunk_bytes: int = CHUNK_BYTES, timings: Optional[dict] = None,
              adjust_direction: bool = False, orientation: Optional[list] = None, band=False) -> List[MSA]:
    """loci: per locus its records as (title, sequence).  Returns the loci's centre-star MSAs (ids: the titles' first words,
    descriptions: the titles).  names: the loci's names for error messages (default: their indices).  timings: a dict that
    receives the wall seconds of the stages (orient, centre, pairs, merge: each ends at a download, so includes its kernels).
    adjust_direction: the spec's Orientation step first; the title of a reversed record gets the prefix _R_.  orientation: a list
    that then receives per locus (reversed: a bool per record, how: a string of one of "-kdt" per record).
    band: the pairs over a certified band (True: profile_align.BAND_W0, or pass 1's half-width); the same MSAs.  timings then also
    receives profile_align.pairs_on_device's counters (band_pairs, band_second_passes, band_full_pairs, band_cells, band_full_cells).
    The score-only DP of adjust_direction keeps the full form."""
    names = [str(i) for i in range(len(loci))] if names is None else list(names)
    for name, recs in zip(names, loci):
        if not len(recs):
            from ..subcommands.from_msa import EmptyMSAError
            raise EmptyMSAError(f"No records found in MSA of locus {name}")
    codes = [locus_codes(n, recs) for n, recs in zip(names, loci)]
    out: List[MSA] = []
    for lo, hi in _chunks(codes, chunk_bytes):
        out.extend(_star_chunk(backend, loci[lo:hi], codes[lo:hi], names[lo:hi], budget_bytes, timings, adjust_direction, orientation, band))
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
    _check_sizes(lens, first, counts)
    d_codes = be.upload(host)
    return _centre_launch(be, "mprg_star_centres", d_codes, len(host), lens, seq_off, first, counts)[0], d_codes


def _check_sizes(lens, first, counts):
    for l in range(len(counts)):
        if int(lens[first[l]:first[l] + counts[l]].sum()) >= 1 << 32:
            raise StarAlignError("a locus of 2^32 residues or more")


def _centre_launch(be, call, d_codes, codes_bytes, lens, seq_off, first, counts):
    """mprg_star_centres or mprg_star_centres_canonical over sequence and locus tables uploaded here: (the centres, the device
    buffers of the sequence table, the locus table and the centres)."""
    d_seqs = be.upload(np.stack([seq_off, lens], 1).reshape(-1))
    ltab = np.zeros((len(counts), LOCUS_FIELDS), np.int64)
    ltab[:, 0], ltab[:, 1] = first, counts
    d_loci = be.upload(ltab)
    d_centre = be.empty(4 * len(counts))
    be.call(call, be.ptr(d_codes), codes_bytes, be.ptr(d_seqs), len(lens), be.ptr(d_loci), len(counts),
            be.ptr(d_centre), be.stream, work=float(3 * lens.sum()))
    centre = be.download(d_centre, np.int32, len(counts)).astype(np.int64)
    if (centre == CENTRE_BAD).any():
        raise StarAlignError(f"{call}: a locus's sequences lie outside the buffers")
    return centre, (d_seqs, d_loci, d_centre)


_COMP = np.array([3, 2, 1, 0, 4, 6, 5, 8, 7, 9, 10, 11], np.uint8)


def revcomp(codes: np.ndarray) -> np.ndarray:
    """The reverse complement of a gap-free code array (A<->T, C<->G, R<->Y, K<->M; S, W, N unchanged)."""
    return _COMP[codes[::-1]]


def _lex_less(x: np.ndarray, y: np.ndarray) -> bool:
    """x < y in cell codes, for arrays of one length."""
    d = np.nonzero(x != y)[0]
    return bool(len(d)) and bool(x[d[0]] < y[d[0]])


def canonical_centres(backend, codes: Sequence[Sequence[np.ndarray]]) -> np.ndarray:
    """mprg_star_centres_canonical over the loci: the orientation centre per locus, -1 if all its sequences are empty."""
    host, lens, seq_off, first, counts = _pack(backend, codes)
    _check_sizes(lens, first, counts)
    return _centre_launch(backend, "mprg_star_centres_canonical", backend.upload(host), len(host), lens, seq_off, first, counts)[0]


def strand_evidence(backend, codes: Sequence[Sequence[np.ndarray]], centre: Sequence[int]) -> np.ndarray:
    """mprg_star_strand over the loci against the given centre per locus, AS STORED (no swap): {fwd, rev, nw} per sequence, all
    loci's sequences in one (n, 3) int64 array."""
    host, lens, seq_off, first, counts = _pack(backend, codes)
    ltab = np.zeros((len(counts), LOCUS_FIELDS), np.int64)
    ltab[:, 0], ltab[:, 1] = first, counts
    d = (backend.upload(np.stack([seq_off, lens], 1).reshape(-1)), backend.upload(ltab), backend.upload(np.asarray(centre, np.int32)))
    return _evidence(backend, backend.upload(host), len(host), len(lens), len(counts), d)


def _evidence(be, d_codes, codes_bytes, n_seqs, n_loci, tables):
    d_seqs, d_loci, d_centre = tables
    d_ev, d_status = be.empty(24 * n_seqs), be.empty(4 * n_loci)
    be.call("mprg_star_strand", be.ptr(d_codes), codes_bytes, be.ptr(d_seqs), n_seqs, be.ptr(d_loci), n_loci, be.ptr(d_centre),
            be.ptr(d_ev), be.ptr(d_status), be.stream, work=float(codes_bytes))
    if be.download(d_status, np.int32, n_loci).any():
        raise StarAlignError("mprg_star_strand: a locus's sequences or its centre lie outside the buffers")
    return be.download(d_ev, np.int64, 3 * n_seqs).reshape(-1, 3)


def revcomp_on_device(be, d_codes, codes_bytes: int, jobs: np.ndarray):
    """mprg_star_revcomp: jobs (n, 3) int64 {source offset, n, destination offset} inside the device buffer."""
    d_jobs, d_status = be.upload(jobs.astype(np.int64)), be.empty(4 * len(jobs))
    be.call("mprg_star_revcomp", be.ptr(d_codes), codes_bytes, be.ptr(d_jobs), len(jobs), be.ptr(d_status), be.stream,
            work=float(2 * jobs[:, 1].sum()))
    if len(jobs) and be.download(d_status, np.int32, len(jobs)).any():
        raise StarAlignError("mprg_star_revcomp: a job's ranges lie outside the buffer or overlap")


def orientations(backend, codes: Sequence[Sequence[np.ndarray]], names: Optional[Sequence[str]] = None,
                 budget_bytes: int = pa.DEFAULT_BUDGET_BYTES) -> List[Tuple[List[bool], str]]:
    """The spec's Orientation step alone over the loci (per locus its gap-free code arrays): per locus (reversed, how)."""
    names = [str(i) for i in range(len(codes))] if names is None else names
    return _orient(backend, codes, names, *_pack(backend, codes), budget_bytes)[4]


def _orient(be, codes, names, host, lens, seq_off, first, counts, budget_bytes):
    """The spec's Orientation step for one chunk.  The residues are uploaded once; the reverse complements of the records it
    reverses are written by the device into a tail of that buffer, and the sequence table points there.  Returns the oriented
    code arrays per locus (host side: what the pair stage uploads), the sequence offsets, the device buffer and its size, and per
    locus (reversed flags, how codes)."""
    _check_sizes(lens, first, counts)
    n_loci, n_seqs = len(counts), len(lens)
    d_codes = be.upload(host)
    centre, tables = _centre_launch(be, "mprg_star_centres_canonical", d_codes, len(host), lens, seq_off, first, counts)
    for l in np.nonzero(centre < 0)[0]:
        raise StarAlignError(f"locus {names[l]}: every sequence is empty")
    ev = _evidence(be, d_codes, len(host), n_seqs, n_loci, tables)
    flat = [c for cs in codes for c in cs]
    locus_of = np.repeat(np.arange(n_loci), counts)
    cidx = first + centre
    # the reference orientation: the smaller of the centre and its reverse complement; against the latter fwd and rev swap
    refs, c_opp = [], np.zeros(n_loci, bool)
    for l in range(n_loci):
        s = flat[cidx[l]]
        r = revcomp(s)
        c_opp[l] = _lex_less(r, s)
        refs.append(r if c_opp[l] else s)
    swap = c_opp[locus_of]
    fwd, rev, nw = np.where(swap, ev[:, 1], ev[:, 0]), np.where(swap, ev[:, 0], ev[:, 1]), ev[:, 2]
    nonempty = lens > 0
    other = nonempty & (np.arange(n_seqs) != cidx[locus_of])
    by_k = other & (8 * np.abs(fwd - rev) >= np.maximum(nw, 1))
    opp = by_k & (rev > fwd)
    opp[cidx] = c_opp
    how = np.full(n_seqs, ord("-"), np.uint8)
    how[by_k] = ord("k")
    und = np.nonzero(other & ~by_k)[0]
    if len(und):
        # both orientations of every undecided sequence against its locus's reference: one small batch of pairs, scores only
        und_loci = np.unique(locus_of[und])
        dp = pa.pairs_on_device(be, [refs[l].reshape(1, -1) for l in und_loci],
                                [[x for u in und[locus_of[und] == l] for x in (flat[u], revcomp(flat[u]))] for l in und_loci], budget_bytes)
        score = dp.score.reshape(-1, 2)                  # (pairs come back in leaf order, then sequence order: und's order)
        opp[und], how[und] = score[:, 1] > score[:, 0], ord("d")
        for i in np.nonzero(score[:, 1] == score[:, 0])[0]:
            opp[und[i]], how[und[i]] = _lex_less(revcomp(flat[und[i]]), flat[und[i]]), ord("t")
    # the first non-empty record keeps its orientation, everything else follows it
    anchor = np.minimum.reduceat(np.where(nonempty, np.arange(n_seqs), n_seqs), first)
    rev_flag = nonempty & (opp != opp[anchor[locus_of]])
    rv = np.nonzero(rev_flag)[0]
    codes_bytes = len(host)
    if len(rv):
        dst = len(host) + np.concatenate([[0], np.cumsum(lens[rv])[:-1]]).astype(np.int64)
        codes_bytes = len(host) + int(lens[rv].sum())
        d_codes = be.grown(d_codes, len(host), codes_bytes)
        revcomp_on_device(be, d_codes, codes_bytes, np.stack([seq_off[rv], lens[rv], dst], 1))
        seq_off = seq_off.copy()
        seq_off[rv] = dst
        flat = list(flat)
        for u in rv:
            flat[u] = revcomp(flat[u])
    oriented = [flat[first[l]:first[l] + counts[l]] for l in range(n_loci)]
    result = [(rev_flag[first[l]:first[l] + counts[l]].tolist(), how[first[l]:first[l] + counts[l]].tobytes().decode()) for l in range(n_loci)]
    return oriented, seq_off, d_codes, codes_bytes, result


def _star_chunk(be, loci, codes, names, budget_bytes, timings=None, adjust_direction=False, orientation=None, band=False) -> List[MSA]:
    import time
    t0 = time.perf_counter()
    host, lens, seq_off, first, counts = _pack(be, codes)
    titles = [[t for t, _ in recs] for recs in loci]
    if adjust_direction:
        codes, seq_off, d_codes, codes_bytes, result = _orient(be, codes, names, host, lens, seq_off, first, counts, budget_bytes)
        titles = [[REVERSED_PREFIX + t if r else t for t, r in zip(ts, rev)] for ts, (rev, _) in zip(titles, result)]
        if orientation is not None:
            orientation.extend(result)
        t_or = time.perf_counter()
        if timings is not None:
            timings["orient_s"] = timings.get("orient_s", 0.0) + t_or - t0
        t0 = t_or
        centre = _centre_launch(be, "mprg_star_centres", d_codes, codes_bytes, lens, seq_off, first, counts)[0]
    else:
        centre, d_codes = _centres(be, host, lens, seq_off, first, counts)
        codes_bytes = len(host)
    t1 = time.perf_counter()
    for l in np.nonzero(centre < 0)[0]:
        raise StarAlignError(f"locus {names[l]}: every sequence is empty")
    n_loci = len(codes)
    C = np.array([len(codes[l][centre[l]]) for l in range(n_loci)], np.int64)
    # the pairs: the centre as a 1-row leaf, every other non-empty sequence against it
    leaves = [codes[l][centre[l]].reshape(1, -1) for l in range(n_loci)]
    others = [[a for a in range(len(cs)) if a != centre[l] and len(cs[a])] for l, cs in enumerate(codes)]
    dp = pa.pairs_on_device(be, leaves, [[codes[l][a] for a in others[l]] for l in range(n_loci)], budget_bytes,
                            None if band is False or band is None else band, timings)
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
            be.ptr(d_start), n_width, codes_bytes, be.ptr(d_w), be.ptr(d_status), be.stream, work=float(ops_bytes))
    W = be.download(d_w, np.int64, n_loci)
    _check(be.download(d_status, np.int32, len(rows)), "mprg_star_merge_columns")
    if (W < C).any():
        raise StarAlignError("mprg_star_merge_columns: a locus's boundaries lie outside the buffers")
    base = np.concatenate([[0], np.cumsum(counts * W)[:-1]]).astype(np.int64)
    rank = np.arange(len(rows)) - np.repeat(first, counts)
    rows[:, 5] = np.repeat(base, counts) + rank * np.repeat(W, counts)
    out_bytes = int((counts * W).sum())
    d_rows, d_out = be.upload(rows), be.empty(max(out_bytes, 1))
    be.call("mprg_star_merge_rows", be.ptr(d_codes), codes_bytes, be.ptr(d_ops), ops_bytes, be.ptr(d_rows), len(rows), be.ptr(d_loci),
            n_loci, be.ptr(d_width), be.ptr(d_start), n_width, be.ptr(d_w), be.ptr(d_out), max(out_bytes, 1), be.ptr(d_status),
            be.stream, work=float(out_bytes + ops_bytes))
    _check(be.download(d_status, np.int32, len(rows)), "mprg_star_merge_rows")
    text = be.download(d_out, np.uint8, out_bytes)
    msas = []
    for l in range(n_loci):
        data = text[base[l]:base[l] + counts[l] * W[l]].reshape(int(counts[l]), int(W[l]))
        msas.append(MSA(_data=data, _ids=[(t.split(None, 1) or [""])[0] for t in titles[l]], _descs=titles[l]))
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
