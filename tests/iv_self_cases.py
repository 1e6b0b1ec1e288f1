"""Shared cases of tests/test_iv_self_emulated.py and tests/test_gpu_iv_self.py: bit 2 of a triple's type word (MPRG_IV_SELF) must be
set exactly when the interval's columns, taken as a view of their own with the same rows, partition into one non-match interval —
the oracle's partition_intervals of the sub-view says so —, and bits 0 and 1 are what they were.  Thousands of small views go through
mprg_partition in one call per min_match_length and form: `workgroup` (k_partition: masks and gap runs from their own launches),
`lists` (every view in the fused list: the small ones by k_partition_wave, the others by k_partition_fused) and, in a process that
was started with MPRG_WAVE_VIEWS=0, `lists` again (k_partition_fused for all)."""
import numpy as np

import oracle.from_msa_oracle as orc
from make_prg_amd.engine import BatchEngine, NodeRec
from make_prg_amd.msa import MSA

IV_PURE, IV_SELF = 2, 4
LS = (1, 2, 3, 7)
WAVE, PW_ROWS, PW_CELLS, PW_STACK = 64, 256, 4096, 32         # csrc/k_partition.inc
PT_STACK = 512
NOT_FAST_L1 = PT_STACK - 4 + 1          # smallest width with n / max(L - 1, 1) + 4 > PT_STACK at L = 1: the scan on global scratch


def pf_pitch(n: int) -> int:
    p = (n + 3) & ~3
    return p + 4 if ((p >> 2) & 1) == 0 else p


def takes_wave_form(S: int, n: int, L: int) -> bool:
    """pw_is_small (csrc/k_partition.inc)."""
    return S >= 1 and 1 <= n <= WAVE and S <= PW_ROWS and S * pf_pitch(n) <= PW_CELLS and n // max(L - 1, 1) + 4 <= PW_STACK


def random_view(rng, L: int, n: int):
    """2-12 rows over ACGT-: a base row, point changes in a few columns, gap stretches (often a row that is all gaps over a long
    stretch, so that has_empty_sequence fires and match runs of about L columns sit between them)."""
    S = int(rng.integers(2, 13))
    base = rng.integers(0, 4, n)
    rows = np.tile(base, (S, 1))
    style = int(rng.integers(0, 4))
    p_col = (0.05, 0.15, 0.3, 0.5)[style]
    for c in np.nonzero(rng.random(n) < p_col)[0]:
        r = rng.integers(0, S, max(1, S // 3))
        rows[r, c] = rng.integers(0, 4, len(r))
    for _ in range(int(rng.integers(0, 2 + S // 2))):          # gap stretches
        r, a = int(rng.integers(0, S)), int(rng.integers(0, n))
        ln = int(rng.integers(1, n + 1)) if rng.random() < 0.4 else int(rng.integers(1, 2 * L + 3))
        rows[r, a:a + ln] = 4
    if rng.random() < 0.2:                                      # an all-gap column or two
        rows[:, rng.integers(0, n, 2)] = 4
    return ["".join("ACGT-"[x] for x in row) for row in rows]


def random_cases(seed: int = 5, per_L: int = 700):
    """[(rows, L)]: widths 1-80, and L - 1, L, L + 1 many times over."""
    rng = np.random.default_rng(seed)
    out = []
    for L in LS:
        widths = [w for w in (L - 1, L, L + 1) if w >= 1] * 40 + list(range(1, 81)) * 2
        widths += [int(x) for x in rng.integers(1, 81, per_L - len(widths))]
        out += [(random_view(rng, L, n), L) for n in widths]
    return out


def hand_cases():
    """[(name, rows, L)].  M = columns that agree, x = columns that differ, '-' stretches in one row."""
    out = []
    for L in LS:
        m = "ACGTACGTAC"[:L]                      # a match run of exactly L
        mm = "ACGTACGTACGTACGTACGT"[:2 * L + 2]   # a long one
        x = ("A", "C", "G")                       # a column that differs
        def rows3(parts):
            # parts: ("m", text) all rows equal; ("x", k) k differing columns; ("g", text, k) text in rows 0 and 1, gaps in row 2;
            # ("xg", k) k differing columns, row 2 gaps
            r = ["", "", ""]
            for p in parts:
                if p[0] == "m":
                    r = [a + p[1] for a in r]
                elif p[0] == "x":
                    r = [a + x[i] * p[1] for i, a in enumerate(r)]
                elif p[0] == "xg":
                    r = [r[0] + "A" * p[1], r[1] + "C" * p[1], r[2] + "-" * p[1]]
            return r
        # a match run of exactly L swallowed after an all-gap row stretch: in the middle, at the first and at the last interval
        out.append((f"swallowed_mid_L{L}", rows3([("m", mm), ("x", 2), ("m", m), ("xg", 3), ("m", mm)]), L))
        out.append((f"swallowed_first_L{L}", rows3([("m", m), ("xg", 3), ("m", mm), ("x", 1), ("m", mm)]), L))
        out.append((f"swallowed_last_L{L}", rows3([("m", mm), ("x", 1), ("m", mm), ("x", 2), ("m", m), ("xg", 3)]), L))
        # a long match run gives its last column to the gap stretch behind it
        out.append((f"shrunk_L{L}", rows3([("m", mm), ("xg", 2), ("m", mm), ("xg", 1)]), L))
        # the swallowing repeated: stretch after stretch, each behind a run of exactly L (the hint's stacks pop and merge)
        out.append((f"swallowed_chain_L{L}", rows3([("m", mm), ("x", 1)] + [("m", m), ("xg", 2)] * 4 + [("m", mm)]), L))
        if L > 1:
            s = m[:L - 1]
            out.append((f"short_at_end_L{L}", rows3([("m", mm), ("x", 2), ("m", s)]), L))
            out.append((f"short_at_start_L{L}", rows3([("m", s), ("x", 2), ("m", mm)]), L))
            out.append((f"short_between_L{L}", rows3([("m", mm), ("x", 1), ("m", s), ("xg", 2), ("m", s), ("x", 1), ("m", mm)]), L))
        out.append((f"one_column_L{L}", rows3([("m", mm), ("x", 1), ("m", mm)]), L))
        out.append((f"one_column_view_L{L}", rows3([("x", 1)]), L))
        out.append((f"narrower_than_L_L{L}", rows3([("x", 1), ("m", m[:max(L - 2, 0)])]), L))
    return out


def expected_self(rows, L: int, s: int, e: int) -> bool:
    sub = [r[s:e + 1] for r in rows]
    _, _, ivs = orc.partition_intervals(orc.consensus_string(sub), L, sub)
    return ivs == [(0, e - s, orc.NON)]


def expected_types(rows, L: int):
    """The oracle's intervals of the view as (start, stop, type & 1)."""
    _, _, ivs = orc.partition_intervals(orc.consensus_string(rows), L, rows)
    return [(a, b, 1 if t == orc.NON else 0) for a, b, t in ivs]


def run_partition(be, views, L: int, form: str, n_rows=None):
    """views: list of row lists (one alignment each).  n_rows[i] (optional): the view takes only the first n_rows[i] rows (0: a view
    without rows).  Returns per view the list of (start, stop, type word) and its status."""
    eng = BatchEngine(be, 5, L)
    eng.load([MSA.from_strings(r) for r in views])
    nodes = []
    for i, r in enumerate(views):
        rows = None if n_rows is None or n_rows[i] is None else np.arange(n_rows[i], dtype=np.int32)
        nodes.append(NodeRec(i, -1, 0, rows, 0, len(r[0])))
    idxs = list(range(len(nodes)))
    tab, rowidx, total_cols, _ = eng._view_table(nodes, idxs)
    n = len(idxs)
    d_views, d_rowidx = be.upload(tab), be.upload(rowidx)
    d_mask = be.zeros(4 * total_cols)
    d_maxrun, d_stack, d_ivflag = be.zeros(4 * total_cols), be.empty(16 * total_cols), be.zeros(8 * total_cols)
    d_iv, d_niv, d_status = be.empty(12 * total_cols), be.empty(4 * n), be.empty(4 * n)
    if form == "workgroup":
        work, rpc = eng._mask_work(tab)
        wr = eng._gap_run_work(tab)
        d_work, d_wr = be.upload(work), be.upload(wr)
        be.call("mprg_column_masks", be.ptr(eng.d_arena), be.ptr(d_views), be.ptr(d_rowidx), be.ptr(d_work), work.shape[0], rpc,
                be.ptr(d_mask), be.stream)
        be.call("mprg_partition", be.ptr(eng.d_arena), be.ptr(d_views), be.ptr(d_rowidx), n, be.ptr(d_mask), L, be.ptr(d_wr), len(wr),
                be.ptr(d_maxrun), be.ptr(d_stack), be.ptr(d_ivflag), be.ptr(d_iv), be.ptr(d_niv), be.ptr(d_status), None, None, None,
                None, 0, None, 0, be.stream)
    else:
        assert form == "lists"
        d_fl, d_ol = be.upload(np.arange(n, dtype=np.int32)), be.empty(16)
        be.call("mprg_partition", be.ptr(eng.d_arena), be.ptr(d_views), be.ptr(d_rowidx), n, be.ptr(d_mask), L, None, 0,
                be.ptr(d_maxrun), be.ptr(d_stack), be.ptr(d_ivflag), be.ptr(d_iv), be.ptr(d_niv), be.ptr(d_status), None, None, None,
                be.ptr(d_fl), n, be.ptr(d_ol), 0, be.stream)
    n_iv, status = be.download(d_niv, np.int32, n), be.download(d_status, np.int32, n)
    iv = be.download(d_iv, np.int32, 3 * total_cols).reshape(-1, 3)
    out = []
    for j in range(n):
        o = int(tab[j, 8])
        out.append([tuple(int(x) for x in iv[o + q]) for q in range(int(n_iv[j]))])
    return out, status


def check_cases(be, cases, form: str) -> dict:
    """The hint = the scan, for every non-match triple of every case; bits 0 and 1 as before.  Returns counts:
    {yes, no, wave, fused} — hinted / not hinted non-match intervals, views by the form that `lists` gives them."""
    stats = dict(yes=0, no=0, wave=0, fused=0)
    for L in LS:
        group = [(name, rows) for name, rows, l in cases if l == L]
        if not group:
            continue
        got, status = run_partition(be, [rows for _, rows in group], L, form)
        for (name, rows), ivs, st in zip(group, got, status):
            assert st == 0, (name, L, form, int(st))
            want = expected_types(rows, L)
            assert [(a, b, t & 1) for a, b, t in ivs] == want, (name, L, form, rows, ivs, want)
            stats["wave" if takes_wave_form(len(rows), len(rows[0]), L) else "fused"] += 1
            for a, b, t in ivs:
                assert t & ~7 == 0, (name, L, form, ivs)
                if t & 1:
                    assert not t & IV_PURE, (name, L, form, ivs)
                    exp = expected_self(rows, L, a, b)
                    assert bool(t & IV_SELF) == exp, (name, L, form, rows, (a, b, t), exp)
                    stats["yes" if exp else "no"] += 1
                else:
                    assert t in (0, IV_PURE), (name, L, form, ivs)      # (0: a non-match interval of one distinct sequence, retyped)
    return stats


def all_cases():
    return [(f"random{i}", rows, L) for i, (rows, L) in enumerate(random_cases())] + hand_cases()


def no_hint_cases():
    """[(name, rows, L, n_rows)]: views that must not carry bit 2 anywhere — an N, an ambiguity code, no rows."""
    body = ["ACGTACGTACAAGTACGTACGT", "ACGTACGTACCAGTACGTACGT", "ACGTACGTACG-GTACGTACGT", "ACGTACGTAC--GTACGTACGT"]
    with_n = [body[0][:3] + "N" + body[0][4:]] + body[1:]
    with_r = [body[0][:3] + "R" + body[0][4:]] + body[1:]
    return [("plain", body, 3, None), ("with_N", with_n, 3, None), ("with_IUPAC", with_r, 3, None), ("no_rows", body, 3, 0)]


def check_no_hint(be, form: str):
    cases = [c for c in no_hint_cases() if form == "workgroup" or c[3] != 0]          # (the fused launch shape has no view without rows)
    got, status = run_partition(be, [c[1] for c in cases], 3, form, n_rows=[c[3] for c in cases])
    by = {c[0]: ivs for c, ivs in zip(cases, got)}
    assert any(t & IV_SELF for _, _, t in by["plain"]), by["plain"]          # (the control: the same view without the N has the hint)
    for name in ("with_N", "with_IUPAC"):
        assert any(t & 1 for _, _, t in by[name]) and not any(t & (IV_SELF | IV_PURE) for _, _, t in by[name]), (name, form, by[name])
    if "no_rows" in by:          # (without rows the masks are empty: every column is a non-match column)
        assert any(t & 1 for _, _, t in by["no_rows"]) and not any(t & IV_SELF for _, _, t in by["no_rows"]), by["no_rows"]


def check_not_fast(be):
    """The smallest view that takes the scan on global scratch at min_match_length 1 (workgroup form; the fused launch shape ends
    far below): non-match intervals, none with bit 2; one column narrower: the LDS path, with the hint."""
    rng = np.random.default_rng(9)
    def view(n):
        rows = np.tile(rng.integers(0, 4, n), (4, 1))
        cols = np.arange(5, n, 7)
        rows[1, cols] = (rows[0, cols] + 1) % 4
        return ["".join("ACGT"[x] for x in r) for r in rows]
    wide, narrow = view(NOT_FAST_L1), view(NOT_FAST_L1 - 1)
    got, status = run_partition(be, [wide, narrow], 1, "workgroup")
    assert list(status) == [0, 0]
    for rows, ivs in zip((wide, narrow), got):
        assert [(a, b, t & 1) for a, b, t in ivs] == expected_types(rows, 1)
    assert sum(t & 1 for _, _, t in got[0]) > 10 and not any(t & IV_SELF for _, _, t in got[0])
    assert all(bool(t & IV_SELF) == expected_self(narrow, 1, a, b) for a, b, t in got[1] if t & 1) and any(t & IV_SELF for _, _, t in got[1])


# ---- the forest with the switch on and off ---------------------------------------------------------------------------------------
BATCH = 300


def forest_digest(be, kloop: str, n: int = BATCH, texts=None) -> list:
    """Config-C alignments (or `texts`) through ForestEngine.  kloop "rounds": one forest, the per-step host with per-round launches.
    kloop "fused": two forests of the same engine, the second one sized from the first one's plan and enqueued by mprg_forest_level.
    Per forest: PRGs and tree dumps (not raw node tables: a level's nodes sit in the order in which workgroups reserved their places),
    and per recursion level the views S1 made and those it handed to the partition lists (header words 0 and 3 + 4), beside what the
    node table says: the level's nodes that are not MPRG_NF_PURE, those that are neither that nor MPRG_NF_SELF (`part`), the children
    of multi-interval nodes among the latter, and those of them that turned out to be one non-match interval (MPRG_NF_CAND)."""
    import hashlib
    import json
    from make_prg_amd import forest
    from make_prg_amd.msa import load_alignment_text
    from make_prg_amd.utils.synthetic import synth_config_fasta
    texts = [synth_config_fasta("C", s) for s in range(n)] if texts is None else texts
    msas = [load_alignment_text(t, defer_n=True) for t in texts]
    eng = forest.ForestEngine(be, 5, 7)
    eng.load(msas)
    sha = lambda parts: hashlib.sha256(b"\n".join(parts)).hexdigest()
    out = []
    seen = []
    orig = forest.ForestEngine._step
    def step(self, name, *a, **kw):
        h = orig(self, name, *a, **kw)
        if name == "frontier_count":
            seen.append((int(h[0]), int(h[3]) + int(h[4])))
        return h
    saved, forest.KLOOP = forest.KLOOP, kloop
    forest.ForestEngine._step = step
    try:
        for _ in range(1 if kloop == "rounds" else 2):
            del seen[:]
            eng.run_forest()
            per_step = bool(seen)
            hdr = list(seen) if per_step else [(int(r[0][0]), int(r[0][3]) + int(r[0][4])) for r in eng._plan["levels"]]
            nodes = be.download(eng.d_nodes, np.int64, eng.n_nodes * forest.NODE_FIELDS).reshape(-1, forest.NODE_FIELDS)
            levels = []
            for li, lv in enumerate(eng.levels):
                fr = nodes[lv["f0"]:lv["f0"] + lv["n"]]
                flags, parent = fr[:, forest.N_FLAGS], fr[:, forest.N_PARENT]
                of_interval = (parent >= 0) & (nodes[np.maximum(parent, 0), forest.N_KIND] == 1)
                part = (flags & (1 | 64)) == 0
                levels.append(dict(views=hdr[li][0], listed=hdr[li][1], not_pure=int(((flags & 1) == 0).sum()), part=int(part.sum()),
                                   part_of_interval=int((part & of_interval).sum()), of_interval=int(of_interval.sum()),
                                   part_cand_of_interval=int((part & of_interval & ((flags & 8) != 0)).sum())))
            assert all(v == 0 and l == 0 for v, l in hdr[len(eng.levels):])
            prgs = eng.assemble_prgs()
            out.append(dict(host="per-step" if per_step else "level", prgs=sha([(p or "<none>").encode() for p in prgs]),
                            trees=sha([json.dumps(eng.tree_dump(i, m.ids), sort_keys=True).encode() for i, m in enumerate(msas)]),
                            levels=levels, cells_all=float(eng.counters["cells_all"]), first_prgs=prgs[:4]))
    finally:
        forest.KLOOP = saved
        forest.ForestEngine._step = orig
    return out


def check_forest(on: list, off: list, texts=None):
    """on / off: forest_digest with the switch on / off (MPRG_IV_SELF=0 in a child process)."""
    from make_prg_amd.utils.synthetic import synth_config_fasta
    assert len(on) == len(off)
    for a, b in zip(on, off):
        assert a["host"] == b["host"]
        assert a["prgs"] == b["prgs"] and a["trees"] == b["trees"], a["host"]
        assert len(a["levels"]) == len(b["levels"]) > 2
        skipped = 0
        for la, lb in zip(a["levels"], b["levels"]):
            # the same frontier either way, and a view for every node that is not a pure match interval
            assert la["views"] == lb["views"] == la["not_pure"] == lb["not_pure"] and la["of_interval"] == lb["of_interval"]
            # off: every view goes to a partition list.  on: level 0 and the children of cluster nodes all the same; of the children of
            # multi-interval nodes only those without a hint, and none of those is a non-match interval that partitions into itself
            # (these alignments hold no N) — what is left are the intervals of ONE distinct sequence, which phase 3 retyped to match
            # intervals (type word 0, neither MPRG_IV_PURE nor MPRG_IV_SELF): their own partition is not known beforehand
            assert lb["listed"] == lb["views"] == lb["part"]
            assert la["listed"] == la["part"] and la["part_cand_of_interval"] == 0
            assert la["listed"] - la["part_of_interval"] == lb["listed"] - lb["part_of_interval"]
            assert la["part_of_interval"] == lb["part_of_interval"] - lb["part_cand_of_interval"]
            skipped += lb["listed"] - la["listed"]
        assert skipped > 0
    for i, prg in enumerate(on[0]["first_prgs"]):
        text = synth_config_fasta("C", i) if texts is None else texts[i]
        assert prg == orc.build_locus_from_text(text, 5, 7)[0], i


def check_golden_n(be):
    """The alignments with N of tests/golden/integration.json.gz (the reference's recorded answers) through the forest with the hint in
    use: unchanged output."""
    import gzip
    import json
    import os
    from tests import parity_common as pc
    with gzip.open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "integration.json.gz"), "rt") as fh:
        cases = [c for c in json.load(fh)["cases"] if c["case"].startswith("contains_n")]
    assert len(cases) >= 3
    for c in cases:
        texts = [l["fasta"] for l in c["loci"]]
        assert all("N" in "".join(x for x in t.splitlines() if not x.startswith(">")) for t in texts)
        got, _ = pc.run_batch(be, texts, c["N"], c["L"], "forest")
        for g, l in zip(got, c["loci"]):
            assert "error" not in g, (c["case"], g)
            assert g["prg"] == l["expect"]["prg"] and pc.sha(g["tree"]) == l["expect"]["tree_sha256"], c["case"]
            assert (g["next_node_id"], g["site_num"]) == (l["expect"]["next_node_id"], l["expect"]["site_num"])
