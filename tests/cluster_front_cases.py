"""The chain around the KMeans fits, entry point by entry point, against plain restatements of the reference:
mprg_ungap_dedupe (K3: ungap the rows, group identical ones — cluster_sequences.py:220-233, seq_utils.py:58-70), mprg_kmer_dictionary /
mprg_kmer_counts and their _parts forms (K4 / K5: k-mer ids in first-appearance order, the count matrix — cluster_sequences.py:26-56) and
mprg_split_children (K9b: the children's row lists — cluster_sequences.py:287-296, recursion_tree.py:558-572).  Tables, arena and work
items are built by hand as include/mprg.h lays them out; the references are dicts and lists over `bytes` and share nothing with the hosts
(make_prg_amd.engine / .forest are thin wrappers over the code under test).  Every comparison is exact: all values are integers.
The form a shape takes is restated from the predicates of mprg_api.hip / k_rows.inc / k_kmer.inc / k_cluster.inc and ASSERTED here, so a
case cannot drift off its edge; which kernel ran is not observed.  Inputs: numpy.random.default_rng with fixed seeds, no files.
Shared by tests/test_cluster_front_emulated.py and tests/test_gpu_cluster_front.py."""
import functools

import numpy as np

VF = PF = 12
GAP = 4
GUARD = 0xA5
GUARD_WORD = -0x5A5A5A5B          # four guard bytes read as an int32
K_ROWS = (1, 7, 20)                      # k-mer sizes of the row-group calls
K_KMERS = (1, 7, 8, 9, 16, 17, 31)       # ... of the dictionary / count calls: both sides of k <= 8 (LDS) and k <= 16 (packed keys)
PARTS = (1, 3, 7, 64)


def up(x, m):
    return (int(x) + m - 1) // m * m


def as_bytes(a):
    return [bytes(r) for r in np.ascontiguousarray(a, np.uint8)]


# =============================================================================================================================
# 1. row groups: mprg_ungap_dedupe
# =============================================================================================================================
# the limits of k_rows.inc (DW_ROWS / DW_COLS, RV_ROWS_S, DD_ROWS / RV_COLS, UG_WIDE) restated
def row_form(S, n):
    """The launch that takes a view with every switch on: a wavefront (k_rows_wave; k_dedupe_wave with MPRG_ROW_VIEWS=0), a workgroup
    with a lane per row (k_rows_narrow_s, k_rows_narrow), the general launches (k_ungap_hash, k_ungap_hash_u, k_ungap_dedupe) and, for
    more rows than the LDS table holds, k_dedupe_scan_big before the last of them."""
    if S <= 64 and n <= 64:
        return "wave"
    if n <= 64 and S <= 128:
        return "narrow_s"
    if n <= 64 and S <= 512:
        return "narrow"
    return "big" if S > 512 else "general"


def chunk_rows(n):
    return 8 if n > 4096 else 256


SHORT_LENS = (0, 1, 6, 7, 8, 19, 20, 21)          # ungapped lengths on both sides of k = 1, 7 and 20


def family(rng, R, C, n_hap, alphabet=(0, 1, 2, 3), p_gap=0.15, edges=()):
    """R rows drawn from n_hap related haplotypes (so rows repeat, gaps included), then per row one of: nothing; one cell changed at a
    column of `edges` (the first / last column of a view, or the column just outside it: rows that differ only there are equal inside);
    a gap swapped with the base next to it (equal ungapped, different gapped); all but a few cells gapped (a short row)."""
    alphabet, edges = np.array(alphabet, np.uint8), [e for e in edges if e < C]
    haps = np.tile(rng.choice(alphabet, C), (n_hap, 1))
    mut = rng.random((n_hap, C)) < 0.02
    haps[mut] = rng.choice(alphabet, int(mut.sum()))
    haps[rng.random((n_hap, C)) < p_gap] = GAP
    rows = haps[rng.integers(0, n_hap, R)].copy()
    kinds = rng.integers(0, 8, R)
    for i in range(R):
        if kinds[i] == 0 and len(edges):
            c = int(edges[rng.integers(len(edges))])
            others = [x for x in (*alphabet.tolist(), GAP) if x != rows[i, c]]
            rows[i, c] = others[rng.integers(len(others))]
        elif kinds[i] == 1:
            at = np.nonzero((rows[i, :-1] == GAP) != (rows[i, 1:] == GAP))[0]
            if len(at):
                c = int(at[rng.integers(len(at))])
                rows[i, c], rows[i, c + 1] = rows[i, c + 1], rows[i, c]
        elif kinds[i] == 2:
            keep = rng.choice(C, min(C, SHORT_LENS[rng.integers(len(SHORT_LENS))]), replace=False)
            kept = rows[i, keep]
            kept[kept == GAP] = alphabet[0]
            rows[i] = GAP
            rows[i, keep] = kept
    return rows


def view_edges(*views):
    out = []
    for col0, n in views:
        out += [col0, col0 + n - 1] + ([col0 - 1] if col0 else []) + [col0 + n]
    return out


@functools.lru_cache(maxsize=None)
def row_inputs():
    """(alignments by name, views).  A view: dict(name, msa, S, n, col0, rows = None (identity) or the int32 index list, form)."""
    rng = np.random.default_rng(20240)
    msas, views = {}, []

    def view(name, msa, S, n, col0, rows=None, form=None, chunk=256):
        R, C = msas[msa].shape
        if isinstance(rows, str):
            pick = np.sort(rng.choice(R, S, replace=False))[::-1] if rows == "desc" else rng.permutation(R)[:S]
            if rows == "twice":
                pick[S // 2] = pick[3]
                pick[S - 1] = pick[0]
            rows = pick.astype(np.int32)
        assert col0 + n <= C and (S <= R if rows is None else (len(rows) == S and rows.max() < R))
        # the arithmetic that places the case: a later change of shape cannot move it off its edge
        assert row_form(S, n) == form and chunk_rows(n) == chunk, (name, row_form(S, n), chunk_rows(n))
        views.append(dict(name=name, msa=msa, S=S, n=n, col0=col0, rows=rows, form=form))

    # a wavefront per view: 64 rows and 64 columns, one more of either
    msas["a64"] = family(rng, 70, 70, 9, edges=view_edges((0, 64), (1, 64), (2, 65)))
    view("64x64", "a64", 64, 64, 0, form="wave")
    view("65x64 descending list", "a64", 65, 64, 1, rows="desc", form="narrow_s")
    view("64x65", "a64", 64, 65, 2, form="general")
    view("70x1 one column", "a64", 70, 1, 3, form="narrow_s")
    view("3x1", "a64", 3, 1, 0, form="wave")
    # k_rows_narrow_s against k_rows_narrow: 128 rows
    msas["a33"] = family(rng, 135, 40, 30, edges=view_edges((3, 33), (5, 33)))
    view("128x33", "a33", 128, 33, 3, form="narrow_s")
    view("129x33 list, a row twice", "a33", 129, 33, 5, rows="twice", form="narrow")
    # narrow against general: 512 rows, 64 columns
    msas["a512"] = family(rng, 520, 70, 150, edges=view_edges((0, 64), (2, 64), (1, 65)))
    view("512x64", "a512", 512, 64, 0, form="narrow")
    view("513x64 descending list", "a512", 513, 64, 2, rows="desc", form="big")
    view("512x65", "a512", 512, 65, 1, form="general")
    # big views: more rows than the LDS table of k_ungap_dedupe holds (k_dedupe_scan_big: three row chunks for 600 rows)
    msas["a80"] = family(rng, 600, 85, 170, edges=view_edges((3, 80), (4, 80)))
    view("513x80 list, a row twice", "a80", 513, 80, 3, rows="twice", form="big")
    view("600x80", "a80", 600, 80, 4, form="big")
    # wide views: the chunk of a work item is 8 rows beyond 4 096 columns
    msas["wide"] = family(rng, 130, 4100, 40, edges=view_edges((1, 4096), (3, 4097)))
    view("130x4096", "wide", 130, 4096, 1, form="general", chunk=256)
    view("130x4097", "wide", 130, 4097, 3, form="general", chunk=8)
    # contents
    msas["gaps"] = np.full((40, 20), GAP, np.uint8)
    view("all gaps", "gaps", 40, 20, 0, form="wave")
    view("all gaps, 100 rows of a list", "gaps", 100, 17, 2, rows=rng.integers(0, 40, 100).astype(np.int32), form="narrow_s")
    msas["iupac"] = family(rng, 100, 50, 25, alphabet=(5, 6, 7, 8, 9, 10, 11, 0, 3), edges=view_edges((0, 50), (7, 40)))
    view("codes 5 to 11", "iupac", 100, 50, 0, form="narrow_s")
    view("codes 5 to 11, 60 rows", "iupac", 60, 40, 7, form="wave")
    digits = np.array([[(i >> (2 * j)) & 3 for j in range(40)] for i in range(700)], np.uint8)
    msas["distinct"] = np.concatenate([digits[:, :30], rng.integers(0, 4, (700, 10)).astype(np.uint8)], axis=1)[:, ::-1].copy()
    view("every row distinct", "distinct", 100, 40, 0, form="narrow_s")
    view("every row distinct, 700 rows", "distinct", 700, 37, 3, form="big")          # (the row number sits in the LAST columns)
    msas["equal"] = np.tile(family(rng, 1, 90, 1)[0], (530, 1))
    view("all rows equal", "equal", 90, 30, 1, form="narrow_s")
    view("all rows equal, 530 rows", "equal", 530, 90, 0, form="big")
    # rows 0 / 1: equal ungapped, different gapped.  The reverse — equal gapped, different ungapped — cannot exist; what comes nearest:
    # rows 0 / 2 equal both ways, rows 0 / 3 the same gap pattern and different bases, rows 4 / 5 different patterns and lengths
    msas["pairs"] = np.array([[0, 1, 4, 2, 3, 4, 4, 4], [0, 4, 1, 2, 3, 4, 4, 4], [0, 1, 4, 2, 3, 4, 4, 4], [0, 1, 4, 2, 0, 4, 4, 4],
                              [4, 4, 4, 4, 4, 4, 4, 0], [0, 4, 4, 4, 4, 4, 4, 4], [4, 0, 1, 2, 3, 4, 4, 4]], np.uint8)
    view("pairs", "pairs", 7, 8, 0, form="wave")
    assert {v["col0"] % 4 for v in views} == {0, 1, 2, 3}
    assert {v["form"] for v in views} == {"wave", "narrow_s", "narrow", "general", "big"}
    return msas, views


def view_cells(msas, v):
    m = msas[v["msa"]]
    rows = np.arange(v["S"]) if v["rows"] is None else v["rows"]
    return m[rows, v["col0"]:v["col0"] + v["n"]]


def ref_rows(rows, k):
    """The reference's row groups of one view, restated.  rows: the view's gapped rows as bytes."""
    S = len(rows)
    ung = [r.replace(bytes([GAP]), b"") for r in rows]
    seen_u, seen_g = {}, {}
    rep_u = [seen_u.setdefault(u, i) for i, u in enumerate(ung)]          # (insertion-ordered dictionaries: cluster_sequences.py:220-233)
    rep_g = [seen_g.setdefault(g, i) for i, g in enumerate(rows)]
    reps = [i for i in range(S) if rep_u[i] == i]
    long_rows, short_rows = [i for i in reps if len(ung[i]) >= k], [i for i in reps if len(ung[i]) < k]
    d_at, s_at = {i: d for d, i in enumerate(long_rows)}, {i: s for s, i in enumerate(short_rows)}
    occ = [0]
    for i in long_rows:
        occ.append(occ[-1] + len(ung[i]) - k + 1)
    return dict(ung=ung, ulen=[len(u) for u in ung], rep_u=rep_u, rep_g=rep_g, reps_pos=reps, reps_len=[len(ung[i]) for i in reps],
                seqrow=long_rows, d_of_row=[d_at.get(r, -1) for r in rep_u], s_of_row=[s_at.get(r, -1) for r in rep_u], occ_off=occ,
                summary=[len(reps), len(seen_g), len(long_rows), occ[-1], sum(len(ung[i]) for i in reps), len(short_rows), 0, 0])


@functools.lru_cache(maxsize=None)
def row_expected(k):
    msas, views = row_inputs()
    want = [ref_rows(as_bytes(view_cells(msas, v)), k) for v in views]
    by = {v["name"]: w for v, w in zip(views, want)}
    # the contents the cases are there for
    assert by["all gaps"]["summary"] == [1, 1, 0, 0, 0, 1, 0, 0] and not any(by["all gaps"]["ulen"])
    assert by["every row distinct"]["summary"][:2] == [100, 100] and by["every row distinct, 700 rows"]["summary"][:2] == [700, 700]
    assert by["all rows equal"]["summary"][:2] == [1, 1] and by["all rows equal, 530 rows"]["summary"][:2] == [1, 1]
    p = by["pairs"]
    assert p["rep_u"][:4] == [0, 0, 0, 3] and p["rep_g"][:4] == [0, 1, 0, 3] and p["rep_u"][6] == 0 and p["rep_g"][6] == 6
    assert max(int(view_cells(msas, v).max()) for v in views if v["msa"] == "iupac") == 11
    for v, w in zip(views, want):
        if v["msa"] in ("a64", "a33", "a512", "a80", "wide") and v["n"] > 1 and v["S"] > 3:
            # repeats, rows equal ungapped only, and (k > 1) long and short rows side by side
            assert w["summary"][0] < w["summary"][1] < v["S"], v["name"]
            assert k == 1 or (w["summary"][2] > 2 and w["summary"][5] > 1), v["name"]
    return want


def build_arena(msas):
    """Every alignment twice, as include/mprg.h lays the arena out; 256 bytes behind the last (the row kernels load whole words)."""
    meta, off = {}, 0
    for name, m in msas.items():
        R, C = m.shape
        pc, ps = up(C, 16), up(R, 16)
        rm = off
        cm = up(rm + R * pc, 256)
        off = up(cm + C * ps, 256)
        meta[name] = (rm, cm, pc, ps)
    arena = np.full(off + 256, 15, np.uint8)
    for name, m in msas.items():
        R, C = m.shape
        rm, cm, pc, ps = meta[name]
        arena[rm:rm + R * pc].reshape(R, pc)[:, :C] = m
        arena[cm:cm + C * ps].reshape(C, ps)[:, :R] = m.T
    return arena, meta


@functools.lru_cache(maxsize=None)
def row_tables():
    msas, views = row_inputs()
    arena, meta = build_arena(msas)
    tab = np.zeros((len(views), VF), np.int64)
    rowidx, work = [np.array([7, 7, 7], np.int32)], []          # (no list starts at offset 0)
    n_idx, row_off, col_off, aux0 = 3, 0, 0, 0
    for q, v in enumerate(views):
        rm, cm, pc, ps = meta[v["msa"]]
        rows_off = -1
        if v["rows"] is not None:
            rows_off = n_idx
            rowidx.append(v["rows"])
            n_idx += len(v["rows"])
        tab[q] = [rm, cm, pc, ps, rows_off, v["S"], v["col0"], v["n"], col_off, row_off, aux0, 0]
        work += [(q, c) for c in range((v["S"] + chunk_rows(v["n"]) - 1) // chunk_rows(v["n"]))]
        row_off += v["S"]
        col_off += v["n"]
        aux0 += v["S"] * up(v["n"], 16)
    assert max(arena.nbytes, aux0) < 2 << 20
    return arena, tab, np.concatenate(rowidx), np.array(work, np.int32), row_off, aux0


def run_rows(be, k):
    """One mprg_ungap_dedupe call over all views: neighbouring views of different forms share every output array."""
    arena, tab, rowidx, work, R, U = row_tables()
    nv = len(tab)
    d_arena, d_tab, d_idx, d_work = be.upload(arena), be.upload(tab), be.upload(rowidx), be.upload(work)
    names = ("ulen", "rep_u", "rep_g", "d_of_row", "s_of_row", "reps_pos", "reps_len", "seqrow")
    d = {name: be.full(4 * R, GUARD) for name in names}
    d_u, d_g, d_hash = be.full(U, GUARD), be.full(U, GUARD), be.full(16 * R, GUARD)
    d_occ, d_sum = be.full(8 * (R + nv), GUARD), be.full(64 * nv, GUARD)
    be.call("mprg_ungap_dedupe", be.ptr(d_arena), be.ptr(d_tab), be.ptr(d_idx), nv, k, be.ptr(d_work), len(work), be.ptr(d_u), be.ptr(d_hash),
            *[be.ptr(d[name]) for name in names], be.ptr(d_occ), be.ptr(d_sum), be.ptr(d_g), be.stream)
    be.synchronize()
    out = {name: be.download(d[name], np.int32, R) for name in names}
    out.update(ucodes=be.download(d_u, np.uint8, U), gcodes=be.download(d_g, np.uint8, U), occ_off=be.download(d_occ, np.int64, R + nv),
               summary=be.download(d_sum, np.int64, 8 * nv).reshape(nv, 8))
    return out


def check_rows(be, k):
    """Every output of every view against the restatement.  Not asserted: bytes of a row of ucodes / gcodes past its length inside the
    pitch, list entries past a list's length, `hashes` (scratch)."""
    msas, views = row_inputs()
    _, tab, _, _, _, _ = row_tables()
    want, got = row_expected(k), run_rows(be, k)
    for q, (v, w) in enumerate(zip(views, want)):
        tag = f"k = {k}, view {q} ({v['name']}, {v['form']})"
        S, n, ro, aux0 = v["S"], v["n"], int(tab[q, 9]), int(tab[q, 10])
        pitch = up(n, 16)
        assert got["summary"][q].tolist() == w["summary"], f"{tag}: summary {got['summary'][q].tolist()} != {w['summary']}"
        for name in ("ulen", "rep_u", "rep_g", "d_of_row", "s_of_row"):
            assert got[name][ro:ro + S].tolist() == w[name], f"{tag}: {name}"
        for name in ("reps_pos", "reps_len", "seqrow"):
            assert got[name][ro:ro + len(w[name])].tolist() == w[name], f"{tag}: {name}"
        assert got["occ_off"][ro + q:ro + q + len(w["occ_off"])].tolist() == w["occ_off"], f"{tag}: occ_off"
        cells = view_cells(msas, v)
        G = got["gcodes"][aux0:aux0 + S * pitch].reshape(S, pitch)
        assert (G[:, :n] == cells).all(), f"{tag}: gcodes"
        Uc = got["ucodes"][aux0:aux0 + S * pitch].reshape(S, pitch)
        for i, u in enumerate(w["ung"]):
            assert bytes(Uc[i, :len(u)]) == u, f"{tag}: ucodes row {i}"


def check_rows_all(be):
    for k in K_ROWS:
        check_rows(be, k)


# =============================================================================================================================
# 2. k-mer ids and counts: mprg_kmer_dictionary(_parts), mprg_kmer_counts(_parts)
# =============================================================================================================================
def table_cap(T):
    cap = 16
    while cap < 2 * T:
        cap *= 2
    return cap


def dict_form(k, T):
    """k_kmer_dictionary builds the table in LDS when k <= 8 and cap <= 4 096 slots; keys are packed up to k = 16, hashed beyond."""
    return ("lds" if k <= 8 and table_cap(T) <= 4096 else "global") + (", hashed" if k > 16 else ", packed")


assert table_cap(2048) == 4096 and table_cap(2049) == 8192 and table_cap(3) == 16 and table_cap(8) == 16 and table_cap(9) == 32
assert dict_form(8, 2048) == "lds, packed" and dict_form(8, 2049) == "global, packed" and dict_form(9, 2048) == "global, packed"
assert dict_form(16, 3) == "global, packed" and dict_form(17, 3) == "global, hashed"


def seqs_with_T(rng, T, k, D, alphabet=(0, 1, 2, 3)):
    """D sequences with exactly T k-mer occurrences between them, cut from one periodic, lightly mutated base: k-mers repeat inside a
    sequence and between sequences, and differ from each other in single characters at any place."""
    cuts = np.sort(rng.choice(np.arange(1, T), D - 1, replace=False)) if D > 1 else np.zeros(0, np.int64)
    lens = np.diff(np.concatenate([[0], cuts, [T]])) + k - 1
    L = int(lens.max()) + 4
    base = np.tile(rng.choice(alphabet, 37), L // 37 + 1)[:L].astype(np.uint8)
    m = rng.random(L) < 0.05
    base[m] = rng.choice(alphabet, int(m.sum()))
    out = []
    for n in lens:
        o = int(rng.integers(0, 4))
        s = base[o:o + n].copy()
        m = rng.random(n) < 0.02
        s[m] = rng.choice(alphabet, int(m.sum()))
        out.append(bytes(s))
    assert sum(len(s) - k + 1 for s in out) == T and min(len(s) for s in out) >= k
    return out


def edge_kmers(rng, k):
    """k-mers that differ only in their first character (3 / 11 and 1 / 2) or only in their last (1 / 5 and 0 / 3): what a key that lost
    its top or its bottom bits would merge."""
    core = bytes(rng.integers(0, 4, k - 1).astype(np.uint8))
    f = lambda *c: bytes(c)
    seqs = [f(3) + core, f(11) + core, core + f(1), core + f(5), f(1) + core + f(0), f(2) + core + f(3), f(3) + core + f(1)]
    if k > 1:
        assert len({s[:k] for s in seqs[:2]}) == 2 and seqs[0][1:k] == seqs[1][1:k] and seqs[2][:k - 1] == seqs[3][:k - 1]
    return seqs + seqs_with_T(rng, 40, k, 3)


@functools.lru_cache(maxsize=None)
def kmer_calls(k):
    """{call: [problem = list of sequences]}.  T = 2 048 / 2 049 sit on the two sides of the in-LDS rule at k <= 8 (cap 4 096 / 8 192,
    asserted above); beyond k = 8 every problem takes the global-memory form, beyond 16 with hashed keys."""
    rng = np.random.default_rng(5000 + k)
    T_of = lambda seqs: sum(len(s) - k + 1 for s in seqs)
    main = [seqs_with_T(rng, 3, k, 3),                                        # D = 3 sequences of length k: most of 64 parts are empty
            seqs_with_T(rng, 511, k, 5), seqs_with_T(rng, 512, k, 1), seqs_with_T(rng, 513, k, 9),          # the 512-occurrence chunks of the id scan
            seqs_with_T(rng, 2048, k, 11), seqs_with_T(rng, 2049, k, 7),
            seqs_with_T(rng, 5003, k, 13, alphabet=tuple(x for x in range(12) if x != GAP)),
            [bytes([2]) * (300 + k - 1), bytes([2]) * k, bytes([2]) * (k + 5)],          # one distinct k-mer; a count of 300 in one cell
            edge_kmers(rng, k)]
    assert [T_of(p) for p in main[:7]] == [3, 511, 512, 513, 2048, 2049, 5003] and all(len(s) == k for s in main[0])
    assert dict_form(k, 2048) == ("lds" if k <= 8 else "global") + (", hashed" if k > 16 else ", packed")
    assert dict_form(k, 2049).startswith("global") and dict_form(k, T_of(main[8])).startswith("lds" if k <= 8 else "global")
    return dict(main=main, small=[edge_kmers(rng, k), seqs_with_T(rng, 3, k, 3)])


def pack(kmer):
    """The key of a k-mer of at most 16 characters: 4 bits per character, the first character in the highest bits."""
    key = 0
    for c in kmer:
        key = key << 4 | c
    return key


def ref_kmers(seqs, k):
    """count_distinct_kmers / count_kmer_occurrences restated: ids by first appearance over the sequences in order, positions left to right."""
    ids, flags, rows = {}, [], []
    for s in seqs:
        row = {}
        for p in range(len(s) - k + 1):
            km = s[p:p + k]
            flags.append(0 if km in ids else 1)
            j = ids.setdefault(km, len(ids))
            row[j] = row.get(j, 0) + 1
        rows.append(row)
    X = np.zeros((len(seqs), len(ids)))
    for d, row in enumerate(rows):
        for j, c in row.items():
            X[d, j] = c
    return len(ids), np.array(flags, np.uint8), X, ids


@functools.lru_cache(maxsize=None)
def kmer_expected(k, call):
    want = [ref_kmers(seqs, k) for seqs in kmer_calls(k)[call]]
    if call == "main":
        assert want[7][0] == 1 and want[7][2].max() == 300
        assert all(1 < w[0] < len(w[1]) for i, w in enumerate(want) if i not in (0, 7) and k > 1)          # (repeats and news in every problem)
    return want


def kmer_tables(probs, k, seed):
    """The problem table, the views and ucodes of a call by hand.  Problem b reads view nP - 1 - b; its sequences sit at increasing row
    positions of the view with other rows between them."""
    rng = np.random.default_rng(seed)
    nP = len(probs)
    views, prob = np.zeros((nP, VF), np.int64), np.zeros((nP, PF), np.int64)
    lay = []
    for seqs in probs:
        pos, r = [], int(rng.integers(0, 3))
        for _ in seqs:
            pos.append(r)
            r += 1 + int(rng.integers(0, 3))
        lay.append((pos, r, max(len(s) for s in seqs) + int(rng.integers(0, 6))))
    regions, ulen, aux0, row_off = [], [], 0, 0
    for q in range(nP):
        b = nP - 1 - q
        pos, R, n_cols = lay[b]
        pitch = up(n_cols, 16)
        U = np.full((R, pitch), 15, np.uint8)
        U[:, :n_cols] = rng.integers(0, 12, (R, n_cols))          # (the rows between: sequences of other problems, as far as this one knows)
        lens = np.full(R, n_cols, np.int32)
        for s, r in zip(probs[b], pos):
            U[r, :] = 15
            U[r, :len(s)] = np.frombuffer(s, np.uint8)
            lens[r] = len(s)
        views[q, 5], views[q, 7], views[q, 9], views[q, 10] = R, n_cols, row_off, aux0
        regions.append(U.reshape(-1)); ulen.append(lens)
        aux0 += U.size; row_off += R
    seqrow, occ, so, oo, to, fo = [], [], 0, 0, 0, 0
    for b, seqs in enumerate(probs):
        T = sum(len(s) - k + 1 for s in seqs)
        cap = table_cap(T)
        prob[b, 0], prob[b, 1], prob[b, 2], prob[b, 3], prob[b, 4], prob[b, 5], prob[b, 6], prob[b, 11] = nP - 1 - b, len(seqs), so, T, to, cap, oo, fo
        seqrow.append(np.array(lay[b][0], np.int32))
        occ.append(np.concatenate([[0], np.cumsum([len(s) - k + 1 for s in seqs])]).astype(np.int64))
        so += len(seqs); oo += len(seqs) + 1; to += 16 * cap; fo += up(T, 16)
    return views, prob, np.concatenate(regions), np.concatenate(ulen), np.concatenate(seqrow), np.concatenate(occ), to, fo


def check_kmer_call(be, probs, k, want, tag, parts=0, seed=1, weak=False):
    """The dictionary call, then — as the hosts do — the seed from bits 24-30 of out_V into bits 40+ of TABLE_CAP, V and X_OFF set,
    xcounts zeroed, and the counts call.  parts = 0: mprg_kmer_dictionary / mprg_kmer_counts, else the _parts entries.
    V, the seeds, the flags and (packed keys) the table's keys and ids are compared BEFORE the counts call, which looks every k-mer up
    in the table the dictionary left and would search a table without its key for ever: it is only given a dictionary that is right.
    The matrices are compared after it.  Guards: the pad bytes of every flag region, the word behind out_V,
    a spare double behind every matrix.  weak: the library is the MPRG_TEST_WEAK_HASH build (seed 2 holds beyond k = 16)."""
    nP = len(probs)
    views, prob, ucodes, ulen, seqrow, occ, table_bytes, flag_bytes = kmer_tables(probs, k, seed)
    d_views, d_u, d_ulen, d_seqrow, d_occ = be.upload(views), be.upload(ucodes), be.upload(ulen), be.upload(seqrow), be.upload(occ)
    d_table, d_flag, d_V = be.full(table_bytes, GUARD), be.full(flag_bytes, GUARD), be.full(4 * (nP + 1), GUARD)
    d_prob = be.upload(prob)
    head = lambda d_p: [be.ptr(d_views), be.ptr(d_p), nP, k, be.ptr(d_u), be.ptr(d_ulen), be.ptr(d_seqrow), be.ptr(d_occ), be.ptr(d_table)]
    if parts:
        d_pc = be.full(4 * nP * parts, GUARD)
        be.call("mprg_kmer_dictionary_parts", *head(d_prob), be.ptr(d_flag), be.ptr(d_V), parts, be.ptr(d_pc), be.stream)
    else:
        be.call("mprg_kmer_dictionary", *head(d_prob), be.ptr(d_flag), be.ptr(d_V), be.stream)
    be.synchronize()
    outV = be.download(d_V, np.int32, nP + 1).astype(np.int64)
    assert outV[nP] == GUARD_WORD, f"{tag}: the word behind out_V"
    seeds, V = (outV[:nP] >> 24) & 0x7f, outV[:nP] & 0xffffff
    flags, table = be.download(d_flag, np.uint8, flag_bytes), be.download(d_table, np.uint8, table_bytes)
    xo = 0
    for b, (wV, wflags, _, wids) in enumerate(want):
        T, fo = int(prob[b, 3]), int(prob[b, 11])
        assert V[b] == wV, f"{tag}, problem {b}: V {V[b]} != {wV}"
        assert seeds[b] == (2 if weak and k > 16 and wV >= 2 else 0), f"{tag}, problem {b}: seed {seeds[b]}"
        got = flags[fo:fo + T]
        assert (got == wflags).all(), f"{tag}, problem {b}: first_flag at occurrence {int(np.nonzero(got != wflags)[0][0])}"
        assert (flags[fo + T:fo + up(T, 16)] == GUARD).all(), f"{tag}, problem {b}: the pad bytes of its flags"
        if k <= 16:          # packed keys: the table itself, as include/mprg.h lays it out — every distinct k-mer once, with its id
            cap, to = int(prob[b, 5]), int(prob[b, 4])
            tb = table[to:to + 16 * cap]
            keys, kid = tb[:8 * cap].view(np.uint64).tolist(), tb[12 * cap:].view(np.uint32).tolist()
            got = {key: i for key, i in zip(keys, kid) if key != 0xffffffffffffffff}
            assert len(got) == wV and got == {pack(km): i for km, i in wids.items()}, f"{tag}, problem {b}: table"
        prob[b, 5] |= int(seeds[b]) << 40
        prob[b, 7], prob[b, 8] = V[b], xo
        xo += int(prob[b, 1] * V[b]) + 1          # (a spare double behind every matrix)
    x = np.zeros(xo)
    for b in range(nP):
        x[int(prob[b, 8] + prob[b, 1] * V[b])] = np.frombuffer(bytes([GUARD]) * 8, np.float64)[0]
    d_x, d_prob = be.upload(x), be.upload(prob)
    if parts:
        be.call("mprg_kmer_counts_parts", *head(d_prob), be.ptr(d_x), parts, be.stream)
    else:
        be.call("mprg_kmer_counts", *head(d_prob), be.ptr(d_x), be.stream)
    be.synchronize()
    xb = be.download(d_x, np.uint8, 8 * xo)
    for b, (wV, _, wX, _) in enumerate(want):
        D, x0 = int(prob[b, 1]), int(prob[b, 8])
        X = xb[8 * x0:8 * (x0 + D * wV)].view(np.float64).reshape(D, wV)
        assert (X == wX).all(), f"{tag}, problem {b}: X"
        assert (xb[8 * (x0 + D * wV):8 * (x0 + D * wV + 1)] == GUARD).all(), f"{tag}, problem {b}: the double behind its matrix"


def check_kmers(be, k, weak=False):
    """V, the flags and the whole matrix of every problem through the one-workgroup entries and (k <= 16) 1, 3, 7 and 64 workgroups per
    problem, 1 024 on the call of two small problems.  weak: the library is the MPRG_TEST_WEAK_HASH build (k > 16: seed 2 holds)."""
    for call, probs in kmer_calls(k).items():
        want = kmer_expected(k, call)
        check_kmer_call(be, probs, k, want, f"k = {k}, call {call}", weak=weak)
        if k <= 16:
            for parts in (PARTS if call == "main" else (3, 1024)):
                check_kmer_call(be, probs, k, want, f"k = {k}, call {call}, {parts} parts", parts=parts, seed=parts, weak=weak)


def check_kmer_refusals(be):
    """kmer_size = 0, parts = 0 / 1 025 and hashed keys through the _parts dictionary are refused; a valid call then still passes."""
    probs, raised = kmer_calls(7)["small"], 0
    views, prob, ucodes, ulen, seqrow, occ, table_bytes, flag_bytes = kmer_tables(probs, 7, 1)
    bufs = [be.upload(a) for a in (views, prob, ucodes, ulen, seqrow, occ)]
    d_table, d_flag, d_V, d_pc, d_x = be.zeros(table_bytes), be.zeros(flag_bytes), be.zeros(64), be.zeros(4 * 2 * 1025), be.zeros(1 << 16)
    p = [be.ptr(b) for b in bufs]
    head = lambda k: [p[0], p[1], len(probs), k, p[2], p[3], p[4], p[5], be.ptr(d_table)]
    bad = [("mprg_kmer_dictionary", head(0) + [be.ptr(d_flag), be.ptr(d_V), be.stream]),
           ("mprg_kmer_counts", head(0) + [be.ptr(d_x), be.stream]),
           ("mprg_kmer_dictionary_parts", head(0) + [be.ptr(d_flag), be.ptr(d_V), 3, be.ptr(d_pc), be.stream]),
           ("mprg_kmer_counts_parts", head(0) + [be.ptr(d_x), 3, be.stream]),
           ("mprg_kmer_dictionary_parts", head(17) + [be.ptr(d_flag), be.ptr(d_V), 3, be.ptr(d_pc), be.stream])]
    for parts in (0, 1025):
        bad += [("mprg_kmer_dictionary_parts", head(7) + [be.ptr(d_flag), be.ptr(d_V), parts, be.ptr(d_pc), be.stream]),
                ("mprg_kmer_counts_parts", head(7) + [be.ptr(d_x), parts, be.stream])]
    for name, args in bad:
        try:
            be.call(name, *args)
        except Exception:
            raised += 1
    be.synchronize()
    assert raised == len(bad) == 9
    check_kmer_call(be, probs, 7, kmer_expected(7, "small"), "after the refusals")
    check_kmer_call(be, probs, 7, kmer_expected(7, "small"), "after the refusals, 3 parts", parts=3)


# =============================================================================================================================
# 3. children: mprg_split_children
# =============================================================================================================================
SC_RANKS = 1024          # k_cluster.inc: the wavefront form keeps so many ranks' offsets in LDS; more take the one-lane form
SPLIT_K = 7


def split_case(rng, name, n_long, n_short, extra, kfin, first, unused=None, listed=False, form="wavefront"):
    """A view of n_long distinct long rows, n_short distinct short rows (shorter than SPLIT_K = 7) and `extra` repeats, shuffled, with row 0
    of the kind `first` asks for, and hand-written labels: first = ("label", c): row 0 is long and its sequence carries label c;
    ("short",): row 0 is a short row.  unused: a label no sequence carries.  listed: the view's rows are an index list."""
    longs = []
    while len(longs) < n_long:
        s = bytes(rng.integers(0, 4, SPLIT_K + 3).astype(np.uint8))
        if s not in longs:
            longs.append(s)
    shorts = [bytes((j >> (2 * t)) & 3 for t in range(6)) for j in rng.choice(4096, n_short, replace=False)]
    body = longs + shorts
    rows = body + [body[j] for j in rng.integers(0, len(body), extra)]
    rows = [rows[j] for j in rng.permutation(len(rows))]
    j0 = next(j for j, r in enumerate(rows) if (len(r) < SPLIT_K) == (first[0] == "short"))
    rows[0], rows[j0] = rows[j0], rows[0]
    w = ref_rows(rows, SPLIT_K)
    D = w["summary"][2]
    assert D == n_long and w["summary"][5] == n_short and w["d_of_row"][0] == (-1 if first[0] == "short" else 0)
    assign = [(5 * d + 2) % kfin for d in range(D)]
    if unused is not None:
        assign = [(a + 1) % kfin if a == unused else a for a in assign]
    if first[0] == "label":
        assign[0] = first[1]
    assert unused is None or unused not in assign
    assert D >= kfin and (kfin + n_short > SC_RANKS) == (form == "one lane")
    S = len(rows)
    msa_rows = (rng.permutation(3 * S)[:S] if listed else np.arange(S)).astype(np.int32)
    return dict(name=name, S=S, kfin=kfin, dor=w["d_of_row"], sor=w["s_of_row"], n_short=n_short, assign=assign, msa_rows=msa_rows,
                listed=listed)


@functools.lru_cache(maxsize=None)
def split_cases():
    rng = np.random.default_rng(909)
    c = [split_case(rng, "63 rows, row 0 in the last label", 12, 5, 46, 5, ("label", 4)),
         split_case(rng, "64 rows, row 0 in a middle label, label 3 empty", 11, 6, 47, 5, ("label", 2), unused=3),
         split_case(rng, "65 rows, row 0 short", 9, 7, 49, 4, ("short",)),
         split_case(rng, "200 rows of a list, row 0 in label 0, label 7 empty", 40, 30, 130, 10, ("label", 0), unused=7, listed=True),
         split_case(rng, "1 024 ranks, row 0 in a middle label", 14, 1015, 90, 9, ("label", 5)),
         split_case(rng, "1 025 ranks, row 0 in the last label", 14, 1016, 90, 9, ("label", 8), form="one lane"),
         split_case(rng, "1 025 ranks of a list, row 0 short, label 2 empty", 14, 1016, 33, 9, ("short",), unused=2, listed=True, form="one lane")]
    assert [x["S"] for x in c[:4]] == [63, 64, 65, 200]
    assert [x["kfin"] + x["n_short"] for x in c[4:]] == [1024, 1025, 1025] and SC_RANKS == 1024
    return c


def ref_children(case):
    """extract_clusters + merge_clusters restated: the cluster of every row; the children are the cluster holding row 0, then the others by
    cluster number (KMeans labels, then one per distinct short sequence in first-appearance order); a child keeps its rows in view order."""
    kfin, dor, sor, assign = case["kfin"], case["dor"], case["sor"], case["assign"]
    cluster = [assign[dor[i]] if dor[i] >= 0 else kfin + sor[i] for i in range(case["S"])]
    members = {}
    for i, c in enumerate(cluster):
        members.setdefault(c, []).append(int(case["msa_rows"][i]))
    order = [cluster[0]] + [c for c in range(kfin + case["n_short"]) if c != cluster[0]]
    return [members.get(c, []) for c in order]


def check_children(be):
    """All cases in one call: view b of the table belongs to problem nP - 1 - b, every offset but the first problem's is non-zero, a guard
    word stands behind every problem's slice of pool_out and of child_sizes."""
    cases = split_cases()
    nP = len(cases)
    views, prob, info = np.zeros((nP, VF), np.int64), np.zeros((nP, PF), np.int64), np.zeros((nP, 3), np.int64)
    rowidx, dor, sor, n_idx, row_off = [np.array([9], np.int32)], [], [], 1, 0
    for q in range(nP):
        c = cases[nP - 1 - q]
        views[q, 4], views[q, 5], views[q, 9] = (n_idx if c["listed"] else -1), c["S"], row_off
        if c["listed"]:
            rowidx.append(c["msa_rows"]); n_idx += c["S"]
        dor.append(c["dor"]); sor.append(c["sor"])
        row_off += c["S"]
    assign, lo, po, co = [], 0, 0, 0
    for b, c in enumerate(cases):
        prob[b, 0], prob[b, 1], prob[b, 10] = nP - 1 - b, len(c["assign"]), lo
        info[b] = [c["kfin"], po, co]
        assign.append(c["assign"])
        lo += len(c["assign"]); po += c["S"] + 1; co += c["kfin"] + c["n_short"] + 1
    d = [be.upload(a) for a in (views, np.concatenate(rowidx), prob, info, np.concatenate(dor).astype(np.int32),
                                np.concatenate(sor).astype(np.int32), np.concatenate(assign).astype(np.int32))]
    d_pool, d_sizes = be.full(4 * po, GUARD), be.full(4 * co, GUARD)
    be.call("mprg_split_children", be.ptr(d[0]), be.ptr(d[1]), be.ptr(d[2]), nP, *[be.ptr(x) for x in d[3:]], be.ptr(d_pool), be.ptr(d_sizes),
            be.stream)
    be.synchronize()
    pool, sizes = be.download(d_pool, np.int32, po), be.download(d_sizes, np.int32, co)
    for b, c in enumerate(cases):
        want = ref_children(c)
        nc = c["kfin"] + c["n_short"]
        assert len(want) == nc
        p0, c0 = int(info[b, 1]), int(info[b, 2])
        assert sizes[c0:c0 + nc].tolist() == [len(x) for x in want], f"{c['name']}: child_sizes"
        assert pool[p0:p0 + c["S"]].tolist() == [r for x in want for r in x], f"{c['name']}: pool_out"
        assert sizes[c0 + nc] == GUARD_WORD and pool[p0 + c["S"]] == GUARD_WORD, f"{c['name']}: the words behind its slices"
    assert any(0 in [len(x) for x in ref_children(c)] for c in cases)
