"""What the emulated and the GPU tests of the star kernels (csrc/k_star.inc) share: mprg_star_merge_columns / mprg_star_merge_rows
and mprg_star_centres / mprg_star_centres_canonical called directly through the C ABI on tables built by hand, which the host
never builds: ops written as strings (not taken from a DP), rows and loci that point outside their buffers, scores beyond 32 bits.
The references are align_ref.merge, star_ref.centre and strand_ref.canonical_centre.  Every buffer a call reads or writes lies
between GUARD poisoned bytes on either side, and every check reads the guards back."""
import functools
import random
from types import SimpleNamespace

import numpy as np

from make_prg_amd.from_msa import star_align as sa
from tests import align_ref as ar
from tests import star_ref as sr
from tests import strand_ref as st

POISON, GUARD = 0x5C, 64                  # ('\\': no byte of an MSA, no status code, no width)
ABC = "ACGT-RYKMSWN"
RESIDUES = "ACGTRYKMSWN"
NOT_A_CODE = (12, 255, 64)                # '?' in a test sequence: a byte of the code buffer that is no cell code; comes out as '-'
OK, BAD_ROW, NO_SPACE = 0, 1, 2           # MPRG_ST_OK, MPRG_ST_BAD_ROW, MPRG_ST_NO_SPACE
CS = (1, 2, 63, 64, 65, 127, 128, 129, 200)   # merge_columns scans j <= C in steps of 64
RUNS = (1, 63, 64, 65, 128, 130, 200)         # insertion runs around the 64-op chunk


# ---- guarded buffers
def guarded(be, a):
    """(device buffer, address of the payload, payload bytes): the bytes of `a` between GUARD poisoned bytes on either side."""
    a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    buf = np.full(2 * GUARD + len(a), POISON, np.uint8)
    buf[GUARD:GUARD + len(a)] = a
    d = be.upload(buf)
    return d, be.ptr(d) + GUARD, len(a)


def poisoned(be, nbytes):
    return guarded(be, np.full(int(nbytes), POISON, np.uint8))


def fetch(be, g, dtype=np.uint8):
    """The payload of a guarded buffer; both guards must be as they were."""
    d, _, n = g
    whole = be.download(d, np.uint8, n + 2 * GUARD)
    assert (whole[:GUARD] == POISON).all() and (whole[GUARD + n:] == POISON).all(), "a write outside the buffer"
    return whole[GUARD:GUARD + n].copy().view(dtype)


def poison_of(dtype):
    return np.full(np.dtype(dtype).itemsize, POISON, np.uint8).view(dtype)[0]


# ---- hand-built merge tables
def equivalent_ops(seq, ops, C):
    """A row's ops; of a row without ops (k = -1: residue i in column i) the ops that say the same."""
    return ops if ops is not None else "M" * len(seq) + "D" * (C - len(seq))


def expect(loci):
    """Per locus (C, [(sequence, ops or None)]) the reference: (width per boundary, start per boundary, W, the rows' text).  The
    widths are counted here, the text is align_ref.merge's behind a centre row of C columns; '?' comes out as '-'."""
    out = []
    for C, rows in loci:
        ops = [equivalent_ops(s, o, C) for s, o in rows]
        width = [0] * (C + 1)
        for o in ops:
            j = run = 0
            for op in o:
                run = run + 1 if op == "I" else 0
                j += op != "I"
                if op == "I":
                    width[j] = max(width[j], run)
        start = [sum(w + 1 for w in width[:j]) for j in range(C + 1)]
        W = C + sum(width)
        text = [r.replace("?", "-") for r in ar.merge(["A" * C], [s for s, _ in rows], ops)[1:]]
        assert all(len(r) == W for r in text)
        out.append((width, start, W, text))
    return out


def encode_seq(seq):
    return [ABC.index(ch) if ch != "?" else NOT_A_CODE[i % 3] for i, ch in enumerate(seq)]


def pack(loci, order=None, gap=0, tail=0):
    """The buffers and tables of a launch.  codes: the rows' sequences with a byte of another code between them; ops: the rows' ops
    REVERSED, as the header says, with a byte that is no op between them; both end in `tail` spare bytes (valid codes, valid ops).
    The loci's C + 1 boundaries lie in `width` / `start` in `order`, `gap` unused words between them.
    rows: {locus, sequence offset, n, ops offset, k (-1 without ops), 0}; ltab: {first row, rows, C, woff}."""
    order = list(range(len(loci))) if order is None else order
    woff, at = [0] * len(loci), gap
    for l in order:
        woff[l] = at
        at += loci[l][0] + 1 + gap
    codes, ops, rows, ltab = [], [], [], []
    for l, (C, lrows) in enumerate(loci):
        ltab.append([len(rows), len(lrows), C, woff[l]])
        for seq, o in lrows:
            rows.append([l, len(codes), len(seq), len(ops) if o is not None else 0, len(o) if o is not None else -1, 0])
            codes += encode_seq(seq) + [9]
            if o is not None:
                ops += list(o[::-1].encode()) + [ord("X")]
    return SimpleNamespace(codes=np.array(codes + [0] * tail, np.uint8), ops=np.array(ops + [ord("M")] * tail, np.uint8),
                           rows=np.array(rows, np.int64).reshape(-1, sa.ROW_FIELDS), ltab=np.array(ltab, np.int64).reshape(-1, sa.LOCUS_FIELDS),
                           n_width=at)


def merge_columns(be, t):
    """mprg_star_merge_columns over a packed table: (width, start, out_width, status) and the device buffers for merge_rows."""
    dev = SimpleNamespace(ops=guarded(be, t.ops), loci=guarded(be, t.ltab), width=guarded(be, np.zeros(t.n_width, np.int32)),
                          start=poisoned(be, 8 * t.n_width), out_width=poisoned(be, 8 * len(t.ltab)))
    g_rows, g_status = guarded(be, t.rows), poisoned(be, 4 * len(t.rows))
    be.call("mprg_star_merge_columns", dev.ops[1], len(t.ops), g_rows[1], len(t.rows), dev.loci[1], len(t.ltab), dev.width[1], dev.start[1],
            t.n_width, len(t.codes), dev.out_width[1], g_status[1], be.stream)
    return (fetch(be, dev.width, np.int32), fetch(be, dev.start, np.int64), fetch(be, dev.out_width, np.int64),
            fetch(be, g_status, np.int32).tolist(), dev)


def merge_rows(be, t, dev, alloc_bytes, out_bytes=None, out_width=None):
    """mprg_star_merge_rows over the table and what merge_columns left (out_width: another table than the one it wrote) into
    alloc_bytes poisoned bytes of which the call is told out_bytes: (the alloc_bytes, status)."""
    g_codes, g_rows, g_out, g_status = guarded(be, t.codes), guarded(be, t.rows), poisoned(be, alloc_bytes), poisoned(be, 4 * len(t.rows))
    g_w = dev.out_width if out_width is None else guarded(be, np.array(out_width, np.int64))
    be.call("mprg_star_merge_rows", g_codes[1], len(t.codes), dev.ops[1], len(t.ops), g_rows[1], len(t.rows), dev.loci[1], len(t.ltab),
            dev.width[1], dev.start[1], t.n_width, g_w[1], g_out[1], alloc_bytes if out_bytes is None else out_bytes, g_status[1], be.stream)
    for g in (dev.ops, dev.loci, dev.width, dev.start, g_w, g_codes, g_rows):          # (the guards of what the call only reads)
        fetch(be, g)
    return fetch(be, g_out), fetch(be, g_status, np.int32).tolist()


def _check_columns(t, loci, want, width, start, out_width):
    """width, start and out_width per locus; the words between the loci: width as zeroed, start never written."""
    owned = np.zeros(t.n_width, bool)
    for l, ((C, _), (w, s, W, _)) in enumerate(zip(loci, want)):
        o = int(t.ltab[l, 3])
        owned[o:o + C + 1] = True
        assert width[o:o + C + 1].tolist() == w, (l, C)
        assert start[o:o + C + 1].tolist() == s, (l, C)
        assert out_width[l] == W, (l, C)
    assert not width[~owned].any() and (start[~owned] == poison_of(np.int64)).all()


def _residues(rng, n, spoil=0.0):
    return "".join("?" if rng.random() < spoil else rng.choice(RESIDUES) for _ in range(n))


def _columns(rng, c, deleted=0.3):
    return "".join("D" if rng.random() < deleted else "M" for _ in range(c))


def _row(rng, ops, C, spoil=0.0):
    """(a sequence of as many residues as the ops consume, ops); the ops must be possible for that n against C columns."""
    n, cols, k = sum(op != "D" for op in ops), sum(op != "I" for op in ops), len(ops)
    assert cols == C and max(n, C) <= k <= n + C and set(ops) <= set("MID")
    return _residues(rng, n, spoil), ops


@functools.lru_cache(maxsize=None)
def merge_loci():
    """The hand-built loci of check_merge with their reference, as (loci, expect(loci))."""
    rng = random.Random(23)
    loci = []
    for C in CS:
        rows = [(_residues(rng, C), None),                                        # k = -1, n = C: the centre row
                ("", None),                                                       # k = -1, n = 0: an empty sequence
                _row(rng, "M" * C, C), _row(rng, "D" * C, C),                     # all M; all D (n = 0, k = C)
                _row(rng, "I" + "MI" * C, C, spoil=0.1),                          # an I at every boundary
                _row(rng, "I" + "DI" * C, C)]                                     # ... with every column deleted: k = n + C
        if C > 1:
            rows.append((_residues(rng, max(1, C // 2)), None))                   # k = -1, 0 < n < C
        for run in RUNS:                                                          # one run at boundary 0, in the middle, at boundary C
            for j in (0, C // 2, C):
                rows.append(_row(rng, _columns(rng, j) + "I" * run + _columns(rng, C - j), C, spoil=0.02))
        for k in (64, 65, 128):                                                   # op counts of exactly 64, 65 and 128
            if k >= C:
                rows.append(_row(rng, _columns(rng, 1) + "I" * (k - C) + _columns(rng, C - 1), C))
        at = sorted({0, C // 3, 2 * C // 3, C})                                   # several long runs in one row
        ops = "".join("I" * run + _columns(rng, (at + [C])[i + 1] - j) for i, (j, run) in enumerate(zip(at, (70, 129, 64, 66))))
        rows.append(_row(rng, ops, C))
        loci.append((C, rows))
    # one locus of 320 rows whose widest insertions all sit at boundaries 0, 33 and C: per boundary every row's run has another
    # length and the longest is on one of the last rows.  On the GPU the rows' wavefronts atomicMax the same three words.
    C, R = 70, 320
    lengths = []
    for b in range(3):
        v = list(range(1, R))
        rng.shuffle(v)
        i = v.index(R - 1)
        v[i], v[R - 2 - b] = v[R - 2 - b], v[i]
        lengths.append(v)
    rows = [(_residues(rng, C), None)]
    for r in range(R - 1):
        rows.append(_row(rng, "I" * lengths[0][r] + _columns(rng, 33) + "I" * lengths[1][r] + _columns(rng, C - 33) + "I" * lengths[2][r], C))
    loci.append((C, rows))
    return loci, expect(loci)


def _has_chunk_of_insertions_only(ops):
    """A 64-op chunk of I's alone whose run began in an earlier chunk, behind a column op: its ranks rest on c_last alone."""
    return any(set(ops[q:q + 64]) == {"I"} and ops[q - 1] == "I" and set(ops[:q]) != {"I"} for q in range(64, len(ops) - 63, 64))


def check_merge(be):
    """mprg_star_merge_columns, then mprg_star_merge_rows, on hand-built ops, all loci in one launch: width and start per boundary,
    out_width per locus, every status MPRG_ST_OK, and the text byte for byte: all R W bytes of every locus written, no byte
    beside them."""
    loci, want = merge_loci()
    # what the tables hold (properties of the input)
    all_ops = [(C, s, o) for C, rows in loci for s, o in rows if o is not None]
    assert {64, 65, 128} <= {len(o) for _, _, o in all_ops} and any(len(o) == len(s) + C for C, s, o in all_ops if C > 2)
    assert any(_has_chunk_of_insertions_only(o) for _, _, o in all_ops) and any(o[:128] == "I" * 128 for _, _, o in all_ops)
    assert any(0 < len(s) < C for C, rows in loci for s, o in rows if o is None)
    assert set(RESIDUES + "?") <= set("".join(s for C, rows in loci for s, _ in rows))
    assert len(loci[-1][1]) >= 300 and max(want[-1][0]) == len(loci[-1][1]) - 1
    order = list(range(len(loci)))
    random.Random(5).shuffle(order)
    t = pack(loci, order, gap=3)
    assert sorted(t.ltab[:, 3].tolist()) != t.ltab[:, 3].tolist()
    width, start, out_width, status, dev = merge_columns(be, t)
    assert status == [OK] * len(t.rows)
    _check_columns(t, loci, want, width, start, out_width)
    text = "".join("".join(rows) for _, _, _, rows in want).encode()
    t.rows[:, 5] = sa.exclusive_sum([W for (_, rows), (_, _, W, _) in zip(loci, want) for _ in rows])
    out, status = merge_rows(be, t, dev, len(text))
    assert status == [OK] * len(t.rows)
    assert POISON not in text and out.tobytes() == text


# ---- refusals of the merge entries
SLOT = 16                                 # an output slot per row, wider than any row of the status tables


def _status_loci(victim_ops="MIMMM", with_victim=True):
    """Two loci: a good one (C = 5; the centre row and a row with an insertion) and the victim's (C = 4; the centre row and the
    victim: n = 5, k = 5, so that max(n, C) = 5 <= k <= n + C = 9)."""
    return [(5, [("ACGTA", None), ("ACGGTA", "MMIMMM")]), (4, [("ACGT", None)] + [("ACNGT", victim_ops)] * with_victim)]


def _status_run(be, loci, victim=None, locus=None, rows_only=None, out_bytes=4 * SLOT, out_width=None):
    """Both calls over the status table with the victim row's fields / its locus's fields replaced (rows_only: for merge_rows
    alone, after a clean merge_columns): the two calls' results."""
    t = pack(loci, tail=8)
    t.rows[:, 5] = SLOT * np.arange(len(t.rows))
    if victim is not None:
        t.rows[3] = victim
    if locus is not None:
        t.ltab[1] = locus
    width, start, ow, cstatus, dev = merge_columns(be, t)
    if rows_only is not None:
        t.rows[3] = rows_only
    out, rstatus = merge_rows(be, t, dev, 4 * SLOT, out_bytes, out_width)
    return t, width, start, ow, cstatus, out, rstatus


def _slots(texts):
    """The output buffer with these rows' texts (None: nothing written) at their slots."""
    out = np.full(SLOT * len(texts), POISON, np.uint8)
    for r, text in enumerate(texts):
        if text is not None:
            out[SLOT * r:SLOT * r + len(text)] = np.frombuffer(text.encode(), np.uint8)
    return out.tobytes()


def check_merge_statuses(be):
    """One good table, then one defect at a time in the victim row (row 3, beside three good rows) or in its locus: the status
    codes of both calls, the good rows' results, and what a refused row leaves unwritten."""
    good = _status_loci()
    want = expect(good)
    rows_of = lambda w: [r for _, _, _, rows in w for r in rows]      # noqa: E731
    t, width, start, ow, cstatus, out, rstatus = _status_run(be, good)
    assert cstatus == rstatus == [OK] * 4 and out.tobytes() == _slots(rows_of(want))
    _check_columns(t, good, want, width, start, ow)
    L, soff, n, opo, k, o = t.rows[3].tolist()
    assert (L, n, k, o) == (1, 5, 5, 3 * SLOT) and soff + n + 9 == len(t.codes) and opo + k + 9 == len(t.ops) and t.n_width == 11   # (the last row)
    C, codes_bytes, ops_bytes = 4, len(t.codes), len(t.ops)

    # 1. MPRG_ST_BAD_ROW by the row's fields, a clause of st_row_ok each: the row updates no width and writes no byte
    alone = _status_loci(with_victim=False)
    want_alone = expect(alone)
    for clause, victim in (("l < 0", [-1, soff, n, opo, k, o]),
                           ("l >= n_loci", [2, soff, n, opo, k, o]),
                           ("n < 0", [L, soff, -1, opo, k, o]),
                           ("soff < 0", [L, -1, n, opo, k, o]),
                           ("soff + n > codes_bytes, by one byte", [L, codes_bytes - n + 1, n, opo, k, o]),
                           ("k < 0 with n > C", [L, soff, n, opo, -1, o]),
                           ("ops_off < 0", [L, soff, n, -1, k, o]),
                           ("ops_off + k > ops_bytes, by one byte", [L, soff, n, ops_bytes - k + 1, k, o]),
                           ("k < max(n, C), n the larger", [L, soff, n, opo, n - 1, o]),
                           ("k < max(n, C), C the larger", [L, soff, 2, opo, C - 1, o]),
                           ("k > n + C", [L, soff, n, opo, n + C + 1, o])):
        t, width, start, ow, cstatus, out, rstatus = _status_run(be, good, victim=victim)
        assert cstatus == rstatus == [OK, OK, OK, BAD_ROW], clause
        _check_columns(t, alone, want_alone, width, start, ow)
        assert out.tobytes() == _slots(rows_of(want_alone) + [None]), clause
    # ... and by its locus's fields: both rows of that locus, and out_width = -1 for it
    first, R = t.ltab[1, :2].tolist()
    for clause, locus in (("C < 1", [first, R, 0, 6]),
                          ("woff < 0", [first, R, C, -1]),
                          ("woff + C + 1 > n_width, by one word", [first, R, C, 7])):
        t, width, start, ow, cstatus, out, rstatus = _status_run(be, good, locus=locus)
        assert cstatus == rstatus == [OK, OK, BAD_ROW, BAD_ROW], clause
        assert ow.tolist() == [want[0][2], -1], clause
        assert width[:6].tolist() == want[0][0] and not width[6:].any() and start[:6].tolist() == want[0][1], clause
        assert (start[6:] == poison_of(np.int64)).all(), clause
        assert out.tobytes() == _slots(rows_of(want[:1]) + [None, None]), clause

    # 2. MPRG_ST_BAD_ROW by ops that do not fit n and C (the fields pass st_row_ok): k_star_merge_widths' checks of every op and
    #    its closing c_col != C || c_res != n, and the same in k_star_merge_rows.  The row may be written in part, inside its W bytes.
    for clause, ops in (("a byte that is none of M, I, D", "MIXMM"),
                        ("a column op too few: c_col < C", "MIIMM"),
                        ("a column op too many: a column op at col >= C", "MIMMMD"),
                        ("a residue more than n: res >= n", "MIIMMM"),
                        ("a residue fewer than n: c_res < n", "MIDMM")):
        loci = _status_loci(ops)
        assert sum(x != "I" for x in ops) != C or sum(x != "D" for x in ops) != n or not set(ops) <= set("MID")
        assert max(n, C) <= len(ops) <= n + C
        t, width, start, ow, cstatus, out, rstatus = _status_run(be, loci)
        assert cstatus == rstatus == [OK, OK, OK, BAD_ROW], clause
        W = int(ow[1])
        assert C <= W <= SLOT and width[:6].tolist() == want[0][0] and start[:6].tolist() == want[0][1] and ow[0] == want[0][2], clause
        got = out.tobytes()
        assert got[:2 * SLOT] == _slots(want[0][3]), clause
        centre = got[2 * SLOT:2 * SLOT + W].decode()                # (the victim may have widened its locus before it was found out)
        assert centre.replace("-", "") == "ACGT" and got[2 * SLOT + W:3 * SLOT] == bytes([POISON]) * (SLOT - W), clause
        assert got[3 * SLOT + W:] == bytes([POISON]) * (SLOT - W), clause

    # 3. MPRG_ST_NO_SPACE from merge_rows (merge_columns saw a good table): nothing of the row is written
    W1 = want[1][2]
    for clause, kw, bad in (("ooff < 0", dict(rows_only=[L, soff, n, opo, k, -1]), [3]),
                            ("ooff + W > out_bytes, by one byte", dict(out_bytes=3 * SLOT + W1 - 1), [3]),
                            ("out_width < C", dict(out_width=[want[0][2], C - 1]), [2, 3])):
        t, width, start, ow, cstatus, out, rstatus = _status_run(be, good, **kw)
        assert cstatus == [OK] * 4 and rstatus == [NO_SPACE if r in bad else OK for r in range(4)], clause
        assert out.tobytes() == _slots([None if r in bad else text for r, text in enumerate(rows_of(want))]), clause


# ---- the centre entries
ENTRIES = (("mprg_star_centres", sr.centre), ("mprg_star_centres_canonical", st.canonical_centre))
WIDE_WINDOWS = (36000, 27000, 51000, 68000)        # homopolymers of so many windows: the scores n (T - n) lie around 2^32


def pack_seqs(loci, tail=0):
    """(codes, seqs {offset, n}, loci {first, count, 0, 0}) of loci of normalised sequences, a byte of another code between them."""
    codes, stab, ltab = [], [], []
    for l in loci:
        ltab.append([len(stab), len(l), 0, 0])
        for s in l:
            stab.append([len(codes), len(s)])
            codes += [ABC.index(ch) for ch in s] + [4]
    return (np.array(codes + [0] * tail, np.uint8), np.array(stab, np.int64).reshape(-1, 2), np.array(ltab, np.int64).reshape(-1, sa.LOCUS_FIELDS))


def centres(be, entry, codes, stab, ltab):
    g_codes, g_seqs, g_loci, g_centre = guarded(be, codes), guarded(be, stab), guarded(be, ltab), poisoned(be, 4 * len(ltab))
    be.call(entry, g_codes[1], len(codes), g_seqs[1], len(stab), g_loci[1], len(ltab), g_centre[1], be.stream)
    for g in (g_codes, g_seqs, g_loci):
        fetch(be, g)
    return fetch(be, g_centre, np.int32).tolist()


@functools.lru_cache(maxsize=None)
def centre_loci():
    """Degenerate loci, window edges and the locus of wide scores, with both references: (loci, star_ref's centres, the canonical)."""
    rng = random.Random(41)
    seq = lambda n, abc="ACGT": "".join(rng.choice(abc) for _ in range(n))      # noqa: E731
    base = seq(267)
    around = [base[:260 + a] for a in (3, 0, 7, 1, 6, 2, 5, 4)]                 # 255 .. 262 windows: one pass of the 256 threads and one more
    short = seq(20)
    loci = [[], ["", "", ""],                                                    # no sequence; every sequence empty: -1
            ["ACGTA", "ACGTAC", "ACGTACG", "CGTACG"],                            # 0, 1 and 2 windows
            ["", "ACGTACG", "ACGTAC"],
            around, around[::-1], [s[::-1] for s in around],
            [base[:261], base[:261][:255] + "N" + base[256:261], base[:130] + "R" + base[131:261], "N" * 261],   # codes that break windows
            ["ACGTACNACGTAC", "ACGTACGTACGT", "NNNNNNNNNNNN", "ACGTASWKMYRAC", "ACGTACGTACNN"],
            [sr.mutate(rng, short, 0.1, 0.1)[:rng.randint(0, 20)] for _ in range(300)],                           # 300 short sequences
            ["A" * (n + 5) for n in WIDE_WINDOWS]]
    return loci, [sr.centre(l) for l in loci], [st.canonical_centre(l) for l in loci]


def _winner(scores):
    return max(range(len(scores)), key=lambda a: (scores[a], -a))


def check_centres(be):
    """mprg_star_centres and mprg_star_centres_canonical called directly: degenerate loci, window edges, scores beyond 32 bits,
    MPRG_ST_CENTRE_BAD for tables outside their buffers, and the canonical centre's invariance under reverse complements."""
    loci, want, want_canonical = centre_loci()
    assert want[:2] == [-1, -1] and {len(s) - 5 for s in loci[4]} == set(range(255, 263))
    # the locus of wide scores (a property of the input): the exact winner is neither the winner of the scores mod 2^32 nor of
    # their low 32 bits read as signed, with plain and with canonical bins, and a bin lies beyond 16 bits
    wide = loci[-1]
    canonical_scores = [int(c @ sum(map(st.canonical_counts, wide)) - c @ c) for c in map(st.canonical_counts, wide)]
    for exact, winner in ((sr.scores(wide), want[-1]), (canonical_scores, want_canonical[-1])):
        low = [s % (1 << 32) for s in exact]
        signed = [s - (1 << 32) if s >= 1 << 31 else s for s in low]
        assert _winner(exact) == winner and len({winner, _winner(low), _winner(signed)}) == 3 and max(exact) >= 1 << 32
    assert max(sr.kmer_counts(s).max() for s in wide) > 65535
    tables = pack_seqs(loci)
    for (entry, _), w in zip(ENTRIES, (want, want_canonical)):
        assert centres(be, entry, *tables) == w, entry

    # the canonical centre does not move when any subset of a locus is reverse-complemented
    rng = random.Random(43)
    some = [[sr.normalise(s) for s in l] for l in sr.edge_loci() + st.strand_edge_loci() + sr.random_loci(45, 12)] + loci[2:9]
    plain = centres(be, ENTRIES[1][0], *pack_seqs(some))
    assert plain == [st.canonical_centre(l) for l in some]
    flipped = 0
    for _ in range(3):
        flips = [st.flip(rng, l, keep_first=False) for l in some]
        flipped += sum(any(f) and not all(f) for _, f in flips)
        assert centres(be, ENTRIES[1][0], *pack_seqs([l for l, _ in flips])) == plain
    assert flipped >= len(some)

    # MPRG_ST_CENTRE_BAD for the second locus, its neighbour in the same launch right
    pair = [["ACGTACGTAC", "ACGTTCGTAC", "ACGTACGTTT"], ["TTGACCATGA", "TTGACCTTGA", "TTGACCATGG"]]
    codes, stab, ltab = pack_seqs(pair, tail=8)
    off, n = stab[4].tolist()
    for entry, ref in ENTRIES:
        assert centres(be, entry, codes, stab, ltab) == [ref(pair[0]), ref(pair[1])]
        for clause, locus, seq in (("first < 0", [-1, 3, 0, 0], None),
                                   ("count < 0", [3, -1, 0, 0], None),
                                   ("first + count > n_seqs, by the count", [3, 4, 0, 0], None),
                                   ("first + count > n_seqs, by the first", [4, 3, 0, 0], None),
                                   ("a sequence with a negative offset", None, [-1, n]),
                                   ("a sequence with a negative length", None, [off, -1]),
                                   ("a sequence one byte outside codes_bytes", None, [len(codes) - n + 1, n])):
            s2, l2 = stab.copy(), ltab.copy()
            if locus is not None:
                l2[1] = locus
            if seq is not None:
                s2[4] = seq
            assert centres(be, entry, codes, s2, l2) == [ref(pair[0]), sa.CENTRE_BAD], (entry, clause)
