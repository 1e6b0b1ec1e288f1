"""What the emulated and the GPU tests of `from_msa --unaligned --refine` share: MSAs put on a backend as the merge kernel leaves
them, the device entry points called one by one against tests/refine_ref.py and mprg_align_profiles, the spec's invariants, and
the status codes of the new C ABI entries for tables that point outside their buffers."""
import numpy as np

from make_prg_amd.from_msa import star_align as sa
from make_prg_amd.msa import encode
from tests import refine_ref as rr

COMPLEMENT = str.maketrans("ACGTRYKMSWN", "TGCAYRMKSWN")


def records(seqs):
    return [(f"r{i} desc {i}", s) for i, s in enumerate(seqs)]


def revcomp(s: str) -> str:
    return s.translate(COMPLEMENT)[::-1]


def upload_msas(be, msas):
    """msas: lists of equal-length row strings.  (device text, its bytes, offsets, R, W) as star_align.refine_counts takes them."""
    R = np.array([len(m) for m in msas], np.int64)
    W = np.array([len(m[0]) for m in msas], np.int64)
    toff = np.concatenate([[0], np.cumsum(R * W)[:-1]]).astype(np.int64)
    text = np.frombuffer("".join("".join(m) for m in msas).encode(), np.uint8).copy()
    return be.upload(text), len(text), toff, R, W


def align_profiles(be, rows):
    """mprg_align_profiles on one matrix of row strings: 6 x C int32."""
    cells = encode(np.frombuffer("".join(rows).encode(), np.uint8))
    R, C = len(rows), len(rows[0])
    tiles = -(-C // 256)
    d_cells, d_leaves = be.upload(cells), be.upload(np.array([[0, R, C, 0]], np.int64))
    d_work, d_prof = be.upload(np.stack([np.zeros(tiles), np.arange(tiles)], 1).astype(np.int32)), be.empty(24 * C)
    be.call("mprg_align_profiles", be.ptr(d_cells), be.ptr(d_leaves), be.ptr(d_work), tiles, be.ptr(d_prof), be.stream)
    return be.download(d_prof, np.int32, 6 * C).reshape(6, C)


def check_counts_profiles_and_compaction(be, msas):
    """On MSAs that may hold all-gap columns: the counts, keep flags, S and kept columns of mprg_refine_counts; every row's
    leave-one-out profile against mprg_align_profiles on the matrix without it; mprg_refine_compact against the spec."""
    d_text, nbytes, toff, R, W = upload_msas(be, msas)
    rtab, d_counts, d_keep, n_cols, S, kept = sa.refine_counts(be, d_text, nbytes, toff, R, W)
    counts = be.download(d_counts, np.int32, 5 * n_cols)
    keep = be.download(d_keep, np.uint8, n_cols)
    for k, m in enumerate(msas):
        a = np.frombuffer("".join(m).encode(), np.uint8).reshape(len(m), -1)
        want = np.stack([(a == ord(x)).sum(0) for x in "ACGT-"])
        c0 = int(rtab[k, 3])
        assert (counts[5 * c0:5 * c0 + 5 * W[k]].reshape(5, -1) == want).all(), k
        assert (keep[c0:c0 + W[k]] == (want[4] < len(m))).all(), k
        assert kept[k] == len(rr.drop_empty_columns(m)[0]), k
        if kept[k] == W[k]:
            assert S[k] == rr.objective(m) == rr.objective_by_pairs(m), k
    multi = [k for k, m in enumerate(msas) if len(m) >= 2]
    row_locus = np.concatenate([np.full(len(msas[k]), k, np.int64) for k in multi])
    row_in = np.concatenate([np.arange(len(msas[k])) for k in multi]).astype(np.int64)
    d_prof, poff, words = sa.refine_profiles(be, d_text, nbytes, rtab, d_counts, n_cols, row_locus, row_in)
    prof = be.download(d_prof, np.int32, words)
    for k, r, p in zip(row_locus.tolist(), row_in.tolist(), poff.tolist()):
        m = msas[k]
        want = align_profiles(be, [x for i, x in enumerate(m) if i != r])
        assert (prof[p:p + 6 * len(m[0])].reshape(6, -1) == want).all(), (k, r)
    d_out = sa.refine_compact(be, d_text, nbytes, rtab, d_keep, n_cols, toff, nbytes)
    out = be.download(d_out, np.uint8, nbytes)
    compact = []
    for k, m in enumerate(msas):
        want = rr.drop_empty_columns(m)
        got = out[toff[k]:toff[k] + len(m) * kept[k]].reshape(len(m), int(kept[k]))
        assert [r.tobytes().decode() for r in got] == want, k
        compact.append(want)
    d_text2, nbytes2, toff2, R2, W2 = upload_msas(be, compact)
    _, _, _, _, S2, kept2 = sa.refine_counts(be, d_text2, nbytes2, toff2, R2, W2)
    assert S2.tolist() == [rr.objective(m) for m in msas] and (kept2 == W2).all()


def check_invariants(loci, msas, refinement, star):
    """The spec's invariants and S properties of refined MSAs: loci as lists of raw sequences (as given to star_msas through
    records()), star the MSAs of the same call without refine."""
    from tests import star_ref as sr
    for l, m, (acc, s0, s1), st in zip(loci, msas, refinement, star):
        rows = m.rows_as_strings()
        assert m.descriptions[0].replace(sa.REVERSED_PREFIX, "") == "r0 desc 0" and len(rows) == len(l)
        assert len({len(r) for r in rows}) == 1
        assert all(any(r[j] != "-" for r in rows) for j in range(len(rows[0])))
        norm = [sr.normalise(s) for s in l]
        for i, (r, s, t) in enumerate(zip(rows, norm, m.descriptions)):
            assert t in (f"r{i} desc {i}", f"{sa.REVERSED_PREFIX}r{i} desc {i}")
            assert r.replace("-", "") == (revcomp(s) if t.startswith(sa.REVERSED_PREFIX) else s)
        for a in range(len(l)):
            for b in range(a):
                if norm[a] == norm[b] and m.descriptions[a][:3] == m.descriptions[b][:3]:
                    assert rows[a] == rows[b]
        assert m.descriptions == st.descriptions and m.ids == st.ids
        assert s0 == rr.objective(st.rows_as_strings()) and s1 == rr.objective(rows) and s1 >= s0
        assert (acc > 0) == (s1 > s0)
        if acc == 0 or not rr.refinable(st.rows_as_strings()):
            assert acc == 0 and rows == st.rows_as_strings()


def check_abi_statuses(be):
    """Every new entry, handed a table that points outside a buffer, reports its status code and writes nothing else."""
    msa = ["ACGT-A", "AC-T-A", "A-GT-C"]
    d_text, nbytes, toff, R, W = upload_msas(be, [msa])
    POISON = 0x5C

    def untouched(buf, n):
        return (be.download(buf, np.uint8, n) == POISON).all()

    def counts_call(rtab, work, n_cols=6):
        d_counts, d_keep, d_sums, d_status = be.full(20 * 6, POISON), be.full(16, POISON), be.zeros(16), be.full(4 * len(work), POISON)
        d_rtab, d_work = be.upload(np.array(rtab, np.int64)), be.upload(np.array(work, np.int32))
        be.call("mprg_refine_counts", be.ptr(d_text), nbytes, be.ptr(d_rtab), len(rtab), be.ptr(d_work), len(work), be.ptr(d_counts),
                be.ptr(d_keep), n_cols, be.ptr(d_sums), be.ptr(d_status), be.stream)
        return (be.download(d_status, np.int32, len(work)).tolist(), untouched(d_counts, 120) and untouched(d_keep, 6),
                be.download(d_sums, np.int64, 2).tolist(), d_counts)
    good = [[0, 3, 6, 0]]
    st, clean, sums, d_counts = counts_call(good, [[0, 0]])
    assert st == [0] and not clean and sums == [rr.objective_by_pairs([r[:4] + r[5:] for r in msa]) - 11 * 2 * 3, 5]
    for rtab, work in (([[1, 3, 6, 0]], [[0, 0]]),          # the last row ends one byte outside the text
                       ([[0, 4, 6, 0]], [[0, 0]]),          # a row too many
                       ([[-1, 3, 6, 0]], [[0, 0]]),
                       ([[0, 3, 6, 1]], [[0, 0]]),          # the columns end outside the column tables
                       ([[0, 3, 0, 0]], [[0, 0]]),
                       (good, [[1, 0]]), (good, [[-1, 0]]), # no such locus
                       (good, [[0, 1]]), (good, [[0, -1]])):  # no such tile
        st, clean, sums, _ = counts_call(rtab, work)
        assert st == [1] and clean and sums == [0, 0], (rtab, work)

    def profiles_call(rtab, rows, work, words=36):
        d_prof, d_status = be.full(4 * 36, POISON), be.full(4 * len(work), POISON)
        d_rtab, d_rows, d_work = be.upload(np.array(rtab, np.int64)), be.upload(np.array(rows, np.int64)), be.upload(np.array(work, np.int32))
        be.call("mprg_refine_profiles", be.ptr(d_text), nbytes, be.ptr(d_rtab), len(rtab), be.ptr(d_counts), 6, be.ptr(d_rows), len(rows),
                be.ptr(d_work), len(work), be.ptr(d_prof), words, be.ptr(d_status), be.stream)
        return be.download(d_status, np.int32, len(work)).tolist(), untouched(d_prof, 144)
    assert profiles_call(good, [[0, 1, 0]], [[0, 0]]) == ([0], False)
    for rtab, rows, work, words, code in ((good, [[0, 1, 1]], [[0, 0]], 36, 3),        # the profile ends one word outside
                                          (good, [[0, 1, 0]], [[0, 0]], 35, 3),
                                          (good, [[0, 1, -1]], [[0, 0]], 36, 3),
                                          (good, [[0, 3, 0]], [[0, 0]], 36, 2),         # no such row in the locus
                                          (good, [[0, -1, 0]], [[0, 0]], 36, 2),
                                          (good, [[0, 1, 0]], [[1, 0]], 36, 2),         # no such row in the table
                                          (good, [[0, 1, 0]], [[0, 1]], 36, 2),         # no such tile
                                          ([[0, 1, 6, 0]], [[0, 0, 0]], [[0, 0]], 36, 2),   # one row: nothing to leave out
                                          (good, [[1, 1, 0]], [[0, 0]], 36, 1),         # no such locus
                                          ([[1, 3, 6, 0]], [[0, 1, 0]], [[0, 0]], 36, 1)):
        assert profiles_call(rtab, rows, work, words) == ([code], True), (rtab, rows, work, words)

    d_keep = be.upload(np.array([1, 1, 1, 1, 0, 1], np.uint8))

    def compact_call(rtab, rows, out_bytes=15, n_cols=6):
        d_dest, d_nw, d_out, d_status = be.full(24, POISON), be.full(8 * len(rtab), POISON), be.full(15, POISON), be.full(4 * len(rows), POISON)
        d_rtab, d_rows = be.upload(np.array(rtab, np.int64)), be.upload(np.array(rows, np.int64))
        be.call("mprg_refine_compact", be.ptr(d_text), nbytes, be.ptr(d_rtab), len(rtab), be.ptr(d_keep), n_cols, be.ptr(d_dest),
                be.ptr(d_nw), be.ptr(d_rows), len(rows), be.ptr(d_out), out_bytes, be.ptr(d_status), be.stream)
        return (be.download(d_status, np.int32, len(rows)).tolist(), be.download(d_nw, np.int64, len(rtab)).tolist(),
                be.download(d_out, np.uint8, 15).tobytes())
    rows3 = [[0, 0, 0], [0, 1, 0], [0, 2, 0]]
    assert compact_call(good, rows3) == ([0, 0, 0], [5], b"ACGTAAC-TAA-GTC")
    blank = bytes([POISON]) * 15
    assert compact_call(good, rows3, out_bytes=14) == ([3, 3, 3], [5], blank)           # the output ends one byte outside
    assert compact_call(good, [[0, 0, 1]]) == ([3], [5], blank)
    assert compact_call(good, [[0, 0, -1]]) == ([3], [5], blank)
    assert compact_call(good, [[0, 3, 0]]) == ([2], [5], blank)                          # no such row
    assert compact_call(good, [[1, 0, 0]]) == ([1], [5], blank)                          # no such locus
    assert compact_call([[1, 3, 6, 0]], rows3) == ([1, 1, 1], [-1], blank)               # the text ends outside
    assert compact_call(good, rows3, n_cols=5) == ([1, 1, 1], [-1], blank)               # the columns end outside the tables
