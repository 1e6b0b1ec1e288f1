"""`compare_msa`: a test MSA scored against a reference MSA of the same records, on the GPU (csrc/k_msa_compare.inc; C ABI
mprg_msa_compare_map and mprg_msa_compare_columns; DESIGN.md §3b, "Truth recovery").  What FastSP, qscore and bali_score report:
the aligned residue pairs and the columns two alignments share.  This docstring is the specification; tests/compare_ref.py
restates it in plain Python.

The statement (integers only)
-----------------------------
A test MSA T and a reference MSA Ref hold the same records; their widths W_T and W_R may differ, either may have all-gap columns
and all-gap rows.  A residue is any cell that is not '-': the ambiguity codes and N count as residues.

Rows.  If the ids of both MSAs are unique and equal as sets, rows are matched by id; otherwise by position, and the row counts
must be equal.  Reversed records: a test id that is `_R_` + a reference id, where the unprefixed id is not itself a test id,
matches that reference row as a REVERSED row (the title `--adjust-direction` gives a reverse-complemented record).

Same sequences (checked on the device).  A row has n_k residues in both MSAs, with equal cell codes in order; for a reversed
row residue p of Ref must be the complement (star_align.revcomp's table) of residue n_k - 1 - p of T.  A row that fails either
check is an error that names the locus and the record, and nothing is reported for that locus.

Map.  t(k, p) is the test column of residue p of row k, in the reference's numbering (so through the reversal above).  For a
reference cell (k, c) that holds the row's p-th residue, v(k, c) = t(k, p).

Counts per locus.  n_c: the residues of reference column c; n_{c,t}: those of them with v = t; m_t: the residues of test
column t.
    shared            = sum over c, t of C(n_{c,t}, 2)      the residue pairs aligned in both MSAs
    ref_pairs         = sum over c of C(n_c, 2)
    test_pairs        = sum over t of C(m_t, 2)
    ref_columns       = the reference columns with n_c >= 2
    kept_columns      = those of them whose residues all share one v
    identical_columns = those kept columns with m_v = n_c: the test column holds exactly those residues
The contract is these six int64 counts per locus.  The ratios are presentation, None when the denominator is 0:
SP = shared / ref_pairs, Modeler = shared / test_pairs, TC = identical_columns / ref_columns, CS = kept_columns / ref_columns.

Worked example.  T = AC-GT, ACG-T, A-CGT; Ref = ACGT-, ACGT-, AC-GT: (shared, ref_pairs, test_pairs, ref_columns, kept,
identical) = (5, 10, 9, 4, 1, 1).

Limit.  A locus of more than CMP_MAX_ROWS = 8 192 rows is not scored: it is reported as skipped ("rows") and left out of the
totals.  Widths are below 2^31 - 1; with these limits every count stays below 2^57.

On the device
-------------
compare_msas matches the rows on the host and runs the loci in groups whose tmap (4 bytes per reference cell) and tpos (4 bytes
per residue) fit the budget; a locus that alone exceeds it is a group of its own.  Per group: one upload of the texts and the
tables (and the 16 bytes that name that buffer), the two launches, and the counters and the status words back.  tmap is stored
TMAP_LAYOUT (DESIGN.md §3b says what was measured).  Nothing here answers in the device's place."""
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from ..msa import MSA, encode
from ..update import profile_align as pa
from ..update.profile_align import _ranges, exclusive_sum
from .star_align import REVERSED_PREFIX

CMP_LOCUS_FIELDS, CMP_ROW_FIELDS, CMP_COUNTS = 10, 6, 6      # MPRG_CMP_LOCUS_FIELDS, MPRG_CMP_ROW_FIELDS, MPRG_CMP_COUNTS
CMP_MAX_ROWS = 8192                                          # MPRG_CMP_MAX_ROWS
CMP_TILE = 8192                                              # CC_TILE of csrc/k_msa_compare.inc: the words of a column block
CMP_BAD_ITEM, CMP_COUNT, CMP_CODE = 1, 2, 3                  # MPRG_CMP_BAD_ITEM, MPRG_CMP_COUNT, MPRG_CMP_CODE
ROW_MAJOR, COLUMN_MAJOR = 0, 1
TMAP_LAYOUT = ROW_MAJOR                                      # how compare_msas stores tmap (measured: DESIGN.md §3b)
_GAP_CODE = 4


class CompareError(ValueError):
    """compare_msa: the two MSAs cannot be compared."""


class RowMatchError(CompareError):
    """The rows of the two MSAs of a locus cannot be matched."""


class SequenceMismatchError(CompareError):
    """A record does not hold the same sequence in the two MSAs of a locus."""


def _ratio(a: int, b: int) -> Optional[float]:
    return a / b if b else None


class Comparison(NamedTuple):
    """The six counts of a locus (the spec's Counts), and why it was not scored (None, or "rows")."""
    shared: int
    ref_pairs: int
    test_pairs: int
    ref_columns: int
    kept_columns: int
    identical_columns: int
    skipped: Optional[str] = None

    @property
    def sp(self) -> Optional[float]:
        return _ratio(self.shared, self.ref_pairs)

    @property
    def modeler(self) -> Optional[float]:
        return _ratio(self.shared, self.test_pairs)

    @property
    def tc(self) -> Optional[float]:
        return _ratio(self.identical_columns, self.ref_columns)

    @property
    def cs(self) -> Optional[float]:
        return _ratio(self.kept_columns, self.ref_columns)


def total(comparisons: Sequence[Comparison]) -> Comparison:
    """The sums of the counts over the loci that were scored."""
    done = [c for c in comparisons if c.skipped is None]
    return Comparison(*(sum(int(c[f]) for c in done) for f in range(CMP_COUNTS)))


def match_rows(test_ids: Sequence[str], ref_ids: Sequence[str], name="?") -> Tuple[List[int], List[bool]]:
    """The spec's Rows: per reference row its test row, and whether it is a reversed row."""
    have = set(test_ids)
    keys, rev = [], []
    for t in test_ids:
        r = t.startswith(REVERSED_PREFIX) and t[len(REVERSED_PREFIX):] not in have
        keys.append(t[len(REVERSED_PREFIX):] if r else t)
        rev.append(r)
    if len(set(keys)) == len(keys) and len(set(ref_ids)) == len(ref_ids) and set(keys) == set(ref_ids):
        at = {k: i for i, k in enumerate(keys)}
        rows = [at[r] for r in ref_ids]
        return rows, [rev[i] for i in rows]
    if len(test_ids) != len(ref_ids):
        raise RowMatchError(f"locus {name}: the ids do not match and the row counts differ ({len(test_ids)} test rows, {len(ref_ids)} "
                            "reference rows)")
    return list(range(len(ref_ids))), [rev[i] and keys[i] == ref_ids[i] for i in range(len(ref_ids))]


def _codes(msa: MSA, name, which: str) -> np.ndarray:
    data = np.ascontiguousarray(msa.data, np.uint8)
    if data.ndim != 2:
        data = data.reshape(len(msa.ids), -1)
    codes = encode(data)
    bad = np.nonzero((codes == 255).any(axis=1))[0]
    if len(bad):
        i = int(bad[0])
        ch = data[i][int(np.argmax(codes[i] == 255))]
        raise CompareError(f"locus {name}, record {i + 1} ({msa.ids[i]}) of the {which} MSA: character {chr(ch) if ch < 128 else 'non-ASCII'!r} "
                           "outside ACGT-RYKMSWN")
    if codes.shape[1] == 0:                                  # (an all-gap column changes nothing)
        codes = np.full((codes.shape[0], 1), _GAP_CODE, np.uint8)
    return codes


def column_blocks(R: np.ndarray, W_R: np.ndarray) -> np.ndarray:
    """The work items of mprg_msa_compare_columns per locus: P the next power of two >= R, CMP_TILE / P columns a block."""
    P = np.array([1 << max(0, int(r) - 1).bit_length() for r in R], np.int64)
    G = CMP_TILE // np.maximum(P, 1)
    return -(-np.asarray(W_R, np.int64) // np.maximum(G, 1))


def launch(be, d_bufs, n_bufs: int, loci: np.ndarray, rows: np.ndarray, tpos_words: int, tmap_words: int, m_words: int,
           d_tables=None):
    """The two launches over a locus table (n, CMP_LOCUS_FIELDS) and a row table (n_rows, CMP_ROW_FIELDS), both int64.  d_tables:
    (buffer, byte offset of the locus table, of the row table, of the work table in it) when they are on the device already.
    Returns (counts, the map's status words, the columns' status words: device buffers, the number of work items)."""
    n, n_rows = len(loci), len(rows)
    blocks = column_blocks(loci[:, 6], loci[:, 5])
    n_work = int(blocks.sum())
    if d_tables is None:
        work = np.stack([np.repeat(np.arange(n), blocks), _ranges(np.zeros(n, np.int64), blocks)], 1).astype(np.int32)
        d_tables = (be.upload(loci), be.upload(rows), be.upload(work))          # (held until the launches are enqueued)
        p_loci, p_rows, p_work = (be.ptr(d) for d in d_tables)
    else:
        base = be.ptr(d_tables[0])
        p_loci, p_rows, p_work = (base + int(o) for o in d_tables[1:])
    d_tpos, d_tmap, d_m = be.empty(4 * tpos_words), be.empty(4 * tmap_words), be.zeros(4 * m_words)
    d_counts = be.zeros(8 * CMP_COUNTS * n)
    d_st_map, d_st_cols = be.full(4 * n_rows, 0xFF), be.full(4 * n_work, 0xFF)
    cells = float((loci[:, 6] * (loci[:, 2] + loci[:, 5])).sum())
    be.call("mprg_msa_compare_map", be.ptr(d_bufs), n_bufs, p_loci, n, p_rows, n_rows, be.ptr(d_tpos), tpos_words, be.ptr(d_tmap),
            tmap_words, be.ptr(d_m), m_words, be.ptr(d_st_map), be.stream, work=cells + 4.0 * tmap_words)
    be.call("mprg_msa_compare_columns", p_loci, n, p_work, n_work, be.ptr(d_tmap), tmap_words, be.ptr(d_m), m_words, be.ptr(d_counts),
            be.ptr(d_st_cols), be.stream, work=4.0 * (tmap_words + m_words))
    return d_counts, d_st_map, d_st_cols, n_work


def _group(be, items, layout) -> List[Comparison]:
    """One group of loci: items are (name, reference ids, test codes, reference codes, test row per reference row, reversed flags)."""
    n = len(items)
    R = np.array([len(x[3]) for x in items], np.int64)
    WT = np.array([x[2].shape[1] for x in items], np.int64)
    WR = np.array([x[3].shape[1] for x in items], np.int64)
    res = [(x[3] != _GAP_CODE).sum(axis=1).astype(np.int64) for x in items]          # the rows' tpos capacities: the reference's n_k
    texts = [t for x in items for t in (x[2], x[3])]
    sizes = np.array([t.size for t in texts], np.int64)
    toff = exclusive_sum(sizes)
    tmap_off, m_off = exclusive_sum(R * WR), exclusive_sum(WT)
    loci = np.stack([np.zeros(n, np.int64), toff[0::2], WT, np.zeros(n, np.int64), toff[1::2], WR, R, tmap_off,
                     np.full(n, layout, np.int64), m_off], 1).astype(np.int64)
    cap = np.concatenate(res)
    rows = np.stack([np.repeat(np.arange(n), R), _ranges(np.zeros(n, np.int64), R), np.concatenate([np.asarray(x[4], np.int64) for x in items]),
                     np.concatenate([np.asarray(x[5], np.int64) for x in items]), exclusive_sum(cap), cap], 1).astype(np.int64)
    blocks = column_blocks(R, WR)
    work = np.stack([np.repeat(np.arange(n), blocks), _ranges(np.zeros(n, np.int64), blocks)], 1).astype(np.int32)
    # one upload: the texts, then the three tables, each at a multiple of 8 bytes
    text_bytes = int(sizes.sum())
    parts, offs, at = [], [], -(-text_bytes // 8) * 8
    for tab in (loci, rows, work):
        raw = np.ascontiguousarray(tab).view(np.uint8).reshape(-1)
        offs.append(at)
        parts.append(raw)
        at += -(-raw.size // 8) * 8
    blob = np.zeros(at, np.uint8)
    for t, o in zip(texts, toff):
        blob[o:o + t.size] = t.reshape(-1)
    for raw, o in zip(parts, offs):
        blob[o:o + raw.size] = raw
    d_blob = be.upload(blob)
    d_bufs = be.upload(np.array([[be.ptr(d_blob), text_bytes]], np.int64))
    d_counts, d_st_map, d_st_cols, n_work = launch(be, d_bufs, 1, loci, rows, int(cap.sum()), int((R * WR).sum()), int(WT.sum()),
                                                   d_tables=(d_blob, *offs))
    counts = be.download(d_counts, np.int64, CMP_COUNTS * n).reshape(n, CMP_COUNTS)
    st_map, st_cols = be.download(d_st_map, np.int32, len(rows)), be.download(d_st_cols, np.int32, n_work)
    bad = np.nonzero(st_map)[0]
    if len(bad):
        q = int(bad[0])
        l, k, st = int(rows[q, 0]), int(rows[q, 1]), int(st_map[q])
        where = f"locus {items[l][0]}, record {k + 1} ({items[l][1][k]})"
        if st == CMP_COUNT:
            raise SequenceMismatchError(f"{where}: the two MSAs do not hold the same number of residues")
        if st == CMP_CODE:
            raise SequenceMismatchError(f"{where}: the two MSAs do not hold the same sequence" +
                                        (" (the test row is reversed: compared as its reverse complement)" if rows[q, 3] else ""))
        raise CompareError(f"mprg_msa_compare_map: {where}: status {st}: a range outside its table or buffer")
    bad = np.nonzero(st_cols)[0]
    if len(bad):
        raise CompareError(f"mprg_msa_compare_columns: locus {items[int(work[bad[0], 0])][0]}, work item {int(bad[0])}: status "
                           f"{int(st_cols[bad[0]])}: a range outside its table or buffer")
    return [Comparison(*(int(v) for v in counts[k])) for k in range(n)]


def compare_msas(backend, tests: Sequence[MSA], refs: Sequence[MSA], names: Optional[Sequence[str]] = None,
                 budget_bytes: int = pa.DEFAULT_BUDGET_BYTES, layout: int = TMAP_LAYOUT) -> List[Comparison]:
    """Per locus the spec's six counts of tests[l] against refs[l] (names: the loci's names for error messages, default: their
    indices).  A locus of more than CMP_MAX_ROWS rows comes back skipped, with zero counts; a locus without rows has zero counts."""
    if len(tests) != len(refs):
        raise CompareError(f"{len(tests)} test MSAs against {len(refs)} reference MSAs")
    names = list(range(len(tests))) if names is None else list(names)
    out: List[Optional[Comparison]] = [None] * len(tests)
    group, used = [], 0

    def flush():
        nonlocal group, used
        if group:
            for (l, *_), c in zip(group, _group(backend, [g[1:] for g in group], layout)):
                out[l] = c
        group, used = [], 0

    for l, (t, r) in enumerate(zip(tests, refs)):
        rows, rev = match_rows(list(t.ids), list(r.ids), names[l])
        if len(r.ids) > CMP_MAX_ROWS:
            out[l] = Comparison(0, 0, 0, 0, 0, 0, "rows")
            continue
        if len(r.ids) == 0:
            out[l] = Comparison(0, 0, 0, 0, 0, 0)
            continue
        tc, rc = _codes(t, names[l], "test"), _codes(r, names[l], "reference")
        need = 4 * rc.size + 4 * int((rc != _GAP_CODE).sum())
        if group and used + need > budget_bytes:
            flush()
        group.append((l, names[l], list(r.ids), tc, rc, rows, rev))
        used += need
    flush()
    return out
