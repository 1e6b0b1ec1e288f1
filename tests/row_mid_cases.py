"""Mid-width views of mprg_ungap_dedupe (k_rows_mid: RV_COLS = 64 < n <= RM_COLS = 1 024 columns, 1 <= S <= RV_ROWS_S = 128 rows; one
workgroup per view, a group of 8 .. 64 lanes per row, 16 cells per lane, two row batches per wavefront in flight).  One-alignment cases
as in tests/row_view_cases.py (`block`, `text_of`: a conserved left flank, a variable block of n columns, a right flank), used twice:
  * the entry point itself on hand-built tables (include/mprg.h) — the alignment's coded cells as the arena, ONE view per alignment:
    the block, at column `left` —, every output array of the call, compared between the library as it is and the same library with
    MPRG_ROW_MID=0 (a child process: the switch is read once) and against the plain restatement of tests/cluster_front_cases.py;
  * two alignments of every batch through the forest host against the CPU oracle.
The shapes walk the predicate from both sides and every size at which the kernel's lanes regroup (asserted below from the restated
rule).  Shared by tests/test_row_mid_emulated.py and tests/test_gpu_row_mid.py.  Inputs: numpy.random.default_rng, fixed seeds."""
import numpy as np

from tests import cluster_front_cases as cf
from tests.row_view_cases import ACGT, GAP, block, text_of

RV_COLS, RM_COLS, RV_ROWS_S = 64, 1024, 128
WIDTHS = (64, 65, 66, 79, 80, 81, 127, 128, 129, 255, 256, 257, 511, 512, 513, RM_COLS - 1, RM_COLS, RM_COLS + 1)
HEIGHTS = (1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129)
COL0_MODS = (0, 1, 5, 8, 15)           # the block's first column mod 16: the 16-byte loads are unaligned
HEIGHT_WIDTHS = (100, 200, 300, 600)   # 8, 16, 32 and 64 lanes per row: a wavefront holds 8, 4, 2 rows and 1 row per batch
ARRAYS = ("hashes", "ulen", "ucodes", "gcodes", "rep_u", "rep_g", "d_of_row", "s_of_row", "reps_pos", "reps_len", "seqrow", "occ_off", "summary")


def is_mid(S, n):
    return RV_COLS < n <= RM_COLS and 1 <= S <= RV_ROWS_S


def lanes_per_row(n):
    G = 64
    while G > 8 and 16 * (G // 2) >= n:
        G //= 2
    return G


assert [lanes_per_row(n) for n in (65, 128, 129, 256, 257, 512, 513, 1024)] == [8, 8, 16, 16, 32, 32, 64, 64]
assert [lanes_per_row(n) for n in HEIGHT_WIDTHS] == [8, 16, 32, 64]
assert [is_mid(70, n) for n in (64, 65, RM_COLS, RM_COLS + 1)] == [False, True, True, False] and is_mid(128, 100) and not is_mid(129, 100)


def left_flank(L, col0_mod, end_mod=None, n=0):
    """The shortest flank of at least L + 1 columns that puts the block at a column = col0_mod (mod 16) — or, with end_mod, the block's
    END at a column = end_mod (mod 16)."""
    left = L + 1
    while (left + n) % 16 != end_mod if end_mod is not None else left % 16 != col0_mod:
        left += 1
    return left


def case(cells, left, right=9, seed=0):
    """(FASTA text, the block's first column, its columns)"""
    return text_of(cells, left, right, seed), left, cells.shape[1]


def widths(col0_mod, L=7, S=70):
    """One alignment per width, the block at a column = col0_mod (mod 16); half the rows carry a run of gaps."""
    rng = np.random.default_rng(1300 + col0_mod)
    return [case(block(rng, S, n, p_gap=0.5), left_flank(L, col0_mod), seed=n) for n in WIDTHS], 5, L


def heights(n, L=7):
    """One alignment per height; the block's column walks COL0_MODS."""
    rng = np.random.default_rng(1400 + n)
    return [case(block(rng, S, n, p_gap=0.5), left_flank(L, COL0_MODS[j % 5]), seed=S) for j, S in enumerate(HEIGHTS)], 5, L


def block_ends_the_alignment(L=7):
    """The block's last column is the alignment's last (no right flank) and the alignment's width a multiple of 16 (its rows have no
    padding): the last lane's load of the last row reaches as far behind the row-major copy as a load can, 15 bytes.  One row and many
    rows; a width that ends the lane's 16 cells one column into the load and one that fills it."""
    rng = np.random.default_rng(1500)
    out = []
    for S, n in ((1, 65), (1, 130), (100, 65), (100, 81), (128, 200), (3, 1024), (100, 80)):
        left = left_flank(L, None, end_mod=0, n=n)
        assert (left + n) % 16 == 0
        out.append(case(block(rng, S, n, p_gap=0.3), left, right=0, seed=S + n))
    return out, 5, L


def row_content(L=7, n=200, S=100):
    """n = 200: 16 lanes per row, 4 rows per batch, 8 per wavefront and trip.  Rows that are all gaps; ungapped lengths 0, 7, 8, 9, 15, 16
    and 17 (the 8-byte words of the ungapped hash and the 16-byte stores just short of full, full and one over) with the kept cells
    first, last and around a hole; a gap at each of the 16 byte positions of a lane (first lane, second, last); gap runs across a lane
    boundary; a run that ends one row and begins the next where those sit in different batches and different wavefronts; rows whose
    only kept cell is the last / the first column."""
    rng = np.random.default_rng(1600 + L)
    out = []
    for col0_mod in COL0_MODS:
        cells = block(rng, S, n, p_gap=0.0)
        r = 9
        for _ in range(2):
            cells[r] = GAP; r += 1                                   # ulen 0
        for keep in (7, 8, 9, 15, 16, 17):
            cells[r, keep:] = GAP; r += 1                            # the kept cells first ...
            cells[r, :n - keep] = GAP; r += 1                        # ... and last
            cells[r, 1:1 + n - keep] = GAP; r += 1                   # ... and around a hole
        for byte in range(16):
            cells[r, byte] = GAP; cells[r, 16 + (byte + 3) % 16] = GAP; cells[r, 16 * ((n - 1) // 16) + byte % (n % 16 or 16)] = GAP; r += 1
        for a, b in ((14, 18), (15, 16), (31, 49), (1, n - 1)):
            cells[r, a:b] = GAP; r += 1                              # runs across lane boundaries
        for i in (3, 7, 31, 63):                                     # rows i / i + 1: different batches, trips, wavefronts
            cells[i, n - 5:] = GAP
            cells[i + 1, :6] = GAP
        cells[r, :n - 1] = GAP; r += 1                               # only the last column is kept
        cells[r, 1:] = GAP; r += 1                                   # only the first
        assert r <= S
        out.append(case(cells, left_flank(L, col0_mod), seed=col0_mod))
    return out, 5, L


def identical_rows(L=7, S=90):
    """Rows equal without gaps but different with them (rep_u != rep_g), rows equal gaps included, identical rows at positions 0 and
    S - 1 (and the same alignment upside down: a distinct row first and only as the last), at 8, 16 and 64 lanes per row."""
    rng = np.random.default_rng(1700)
    out = []
    for j, n in enumerate((70, 130, 520)):
        cells = block(rng, S, n, p_gap=0.0)
        twin = cells[4].copy()
        for i, at in ((10, 3), (11, 4), (12, 17), (40, n - 2)):          # the same ungapped row, the gap column elsewhere
            cells[i] = np.concatenate([twin[:at], [GAP], twin[at:n - 1]])
        cells[41] = cells[11]                                            # ... and a repeat gaps included
        cells[30] = cells[0]; cells[S - 1] = cells[0]                    # identical rows at 0 and S - 1
        last = cells[1].copy()
        last[n // 2] = ACGT[(int(np.nonzero(ACGT == last[n // 2])[0][0]) + 1) % 4]
        last[2] = GAP
        cells[S - 2] = last
        out += [case(cells, left_flank(L, COL0_MODS[j]), seed=j), case(cells[::-1].copy(), left_flank(L, COL0_MODS[j + 2]), seed=10 + j)]
    return out, 5, L


# ---- the entry point on hand-built tables -------------------------------------------------------------------------------------------------
CODE = np.full(256, 255, np.uint8)
for _c, _v in zip(b"ACGT-", range(5)):
    CODE[_c] = _v


def coded(text):
    rows = [np.frombuffer(l.encode(), np.uint8) for l in text.split("\n") if l and not l.startswith(">")]
    m = CODE[np.array(rows)]
    assert m.max() <= 4
    return m


def run_views(be, cases, k=7):
    """One mprg_ungap_dedupe call: view q = the block of alignment q (all rows).  Every output array, whole."""
    msas = {q: coded(text) for q, (text, _, _) in enumerate(cases)}
    arena, meta = cf.build_arena(msas)
    nv = len(cases)
    tab = np.zeros((nv, cf.VF), np.int64)
    work, row_off, col_off, aux0 = [], 0, 0, 0
    for q, (_, col0, n) in enumerate(cases):
        S, C = msas[q].shape
        assert col0 + n <= C
        rm, cm, pc, ps = meta[q]
        tab[q] = [rm, cm, pc, ps, -1, S, col0, n, col_off, row_off, aux0, 0]
        work += [(q, c) for c in range((S + 255) // 256)]          # (no case is wider than 4 096 columns)
        row_off += S; col_off += n; aux0 += S * cf.up(n, 16)
    R, U, work = row_off, aux0, np.array(work, np.int32)
    d_arena, d_tab, d_idx, d_work = be.upload(arena), be.upload(tab), be.upload(np.zeros(4, np.int32)), be.upload(work)
    names = ("ulen", "rep_u", "rep_g", "d_of_row", "s_of_row", "reps_pos", "reps_len", "seqrow")
    d = {name: be.full(4 * R, cf.GUARD) for name in names}
    d_u, d_g, d_hash = be.full(U, cf.GUARD), be.full(U, cf.GUARD), be.full(16 * R, cf.GUARD)
    d_occ, d_sum = be.full(8 * (R + nv), cf.GUARD), be.full(64 * nv, cf.GUARD)
    be.call("mprg_ungap_dedupe", be.ptr(d_arena), be.ptr(d_tab), be.ptr(d_idx), nv, k, be.ptr(d_work), len(work), be.ptr(d_u), be.ptr(d_hash),
            *[be.ptr(d[name]) for name in names], be.ptr(d_occ), be.ptr(d_sum), be.ptr(d_g), be.stream)
    be.synchronize()
    out = {name: be.download(d[name], np.int32, R) for name in names}
    out.update(ucodes=be.download(d_u, np.uint8, U), gcodes=be.download(d_g, np.uint8, U), hashes=be.download(d_hash, np.uint64, 2 * R),
               occ_off=be.download(d_occ, np.int64, R + nv), summary=be.download(d_sum, np.int64, 8 * nv).reshape(nv, 8))
    return out, tab, msas


def defined(out, tab):
    """The defined part of every output, per view: name -> list of arrays.  Left out: the bytes of a row of ucodes behind its length and
    of gcodes behind its columns, list entries behind a list's length."""
    res = {name: [] for name in ARRAYS}
    for q in range(len(tab)):
        S, n, ro, aux0 = (int(tab[q, j]) for j in (5, 7, 9, 10))
        pitch = cf.up(n, 16)
        sm = out["summary"][q]
        ulen = out["ulen"][ro:ro + S]
        assert 0 <= ulen.min() and ulen.max() <= n and 0 <= sm[2] <= sm[0] <= S
        res["summary"].append(sm)
        res["hashes"].append(out["hashes"][2 * ro:2 * (ro + S)])
        for name in ("ulen", "rep_u", "rep_g", "d_of_row", "s_of_row"):
            res[name].append(out[name][ro:ro + S])
        for name in ("reps_pos", "reps_len"):
            res[name].append(out[name][ro:ro + int(sm[0])])
        res["seqrow"].append(out["seqrow"][ro:ro + int(sm[2])])
        res["occ_off"].append(out["occ_off"][ro + q:ro + q + int(sm[2]) + 1])
        Uc = out["ucodes"][aux0:aux0 + S * pitch].reshape(S, pitch)
        res["ucodes"].append(np.concatenate([Uc[i, :ulen[i]] for i in range(S)]))
        res["gcodes"].append(out["gcodes"][aux0:aux0 + S * pitch].reshape(S, pitch)[:, :n].copy())
    return res


def check_restated(out, tab, msas, cases, k=7):
    """... against the dictionaries of tests/cluster_front_cases.ref_rows (everything but `hashes`)."""
    got = defined(out, tab)
    for q, (_, col0, n) in enumerate(cases):
        cells = msas[q][:, col0:col0 + n]
        w = cf.ref_rows(cf.as_bytes(cells), k)
        tag = f"view {q} ({cells.shape[0]} x {n} at column {col0})"
        assert got["summary"][q].tolist() == w["summary"], f"{tag}: summary"
        for name in ("ulen", "rep_u", "rep_g", "d_of_row", "s_of_row", "reps_pos", "reps_len", "seqrow", "occ_off"):
            assert got[name][q].tolist() == w[name], f"{tag}: {name}"
        assert bytes(got["ucodes"][q]) == b"".join(w["ung"]), f"{tag}: ucodes"
        assert (got["gcodes"][q] == cells).all(), f"{tag}: gcodes"


def dump(be, batch: str, path: str, k=7):
    """(child process) the defined outputs of a batch, flattened per array, into an .npz"""
    cases = eval(batch)[0]
    out, tab, _ = run_views(be, cases, k)
    np.savez(path, **{name: np.concatenate([np.asarray(a).reshape(-1).view(np.uint8) for a in v]) for name, v in defined(out, tab).items()})


def check_views(be, batch: str, off_path: str, k=7):
    """The batch's call here against the restatement and against what the child with MPRG_ROW_MID=0 left in off_path: every array."""
    cases = eval(batch)[0]
    out, tab, msas = run_views(be, cases, k)
    check_restated(out, tab, msas, cases, k)
    off = np.load(off_path)
    for name, v in defined(out, tab).items():
        on = np.concatenate([np.asarray(a).reshape(-1).view(np.uint8) for a in v])
        assert on.shape == off[name].shape and (on == off[name]).all(), f"{batch}: {name} differs from the launches with MPRG_ROW_MID=0"
    return sum(is_mid(int(tab[q, 5]), int(tab[q, 7])) for q in range(len(tab)))


BATCHES = [f"widths({m})" for m in COL0_MODS] + [f"heights({n})" for n in HEIGHT_WIDTHS] + ["block_ends_the_alignment()", "row_content()",
                                                                                            "identical_rows()"]
# the two alignments of a batch that go through the forest host against the oracle (mid-width blocks of moderate size)
ORACLE_PICK = {"widths": (1, 8), "heights": (4, 5), "block_ends_the_alignment": (2, 4), "row_content": (0, 3), "identical_rows": (0, 3)}


def oracle_texts(batch: str):
    cases, N, L = eval(batch)
    pick = (3, 4) if batch == "heights(600)" else ORACLE_PICK[batch.split("(")[0]]          # (63 rows x 600 columns: 17 s on the emulator)
    return [cases[j][0] for j in pick], N, L


# ---- alignments ---------------------------------------------------------------------------------------------------------------------------
def forest_digest(be, seeds) -> dict:
    """PRGs and tree dumps of config-C alignments through the per-step host and through mprg_forest_level (the second forest of a
    resident batch)."""
    import hashlib
    import json
    from make_prg_amd import forest
    from make_prg_amd.msa import load_alignment_text
    from make_prg_amd.utils.synthetic import synth_config_fasta
    msas = [load_alignment_text(synth_config_fasta("C", s), defer_n=True) for s in seeds]
    sha = lambda parts: hashlib.sha256(b"\n".join(parts)).hexdigest()

    def digest(eng):
        return dict(prgs=sha([(p or "<none>").encode() for p in eng.assemble_prgs()]),
                    trees=sha([json.dumps(eng.tree_dump(i, m.ids), sort_keys=True).encode() for i, m in enumerate(msas)]))
    eng = forest.ForestEngine(be, 5, 7)
    eng.load(msas)
    eng.run_forest()
    out = dict(per_step=digest(eng))
    syncs = eng.counters["syncs"]
    eng.run_forest()
    assert eng.counters["syncs"] == syncs + 1 and eng.counters.get("plan_misses", 0) == 0          # (enqueued from the plan: mprg_forest_level)
    out["level"] = digest(eng)
    return out
