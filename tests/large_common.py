"""What the emulated and the GPU tests of `from_msa --unaligned --progressive --collapse-identical --large-loci` share
(make_prg_amd/from_msa/star_align.py, "Large loci"; csrc/k_prog_tree_wide.inc): mprg_prog_tree_wide called directly through the C
ABI on tree_common's hand-built tables, against mprg_prog_tree, the spec's plain statements and the host's tree; whole MSAs of loci
of thousands of records over a dozen alleles against tests/large_ref.py and the star pass; what moves between host and device.
Every reference is computed once per process."""
import functools
import random

import numpy as np

from make_prg_amd.from_msa import star_align as sa
from make_prg_amd.update import profile_align as pa
from tests import collapse_common as cc
from tests import collapse_ref as cr
from tests import large_ref as lr
from tests import prog_common as pc
from tests import prog_ref as pr
from tests import star_ref as sr
from tests import star_trace as tr
from tests import strand_ref as st
from tests import tree_common as tc

WIDE = "mprg_prog_tree_wide"
TOP = 1 << 20                              # PROG_MAX_RECORDS: the largest weight sum mprg_prog_tree_wide builds
SCALE = 256                                # takes tree_common's weight sums (at most 4 096) up to 2^20 at the most


# ---- the call
def call(be, t, entry=WIDE):
    """tree_common.call through `entry`: (status words, per locus its merges as written: BLANK where nothing was); the guard bytes
    around the merges are checked."""
    d_shared, d_nw, d_seqs, d_loci = be.upload(t["shared"]), be.upload(t["nw"]), be.upload(t["seqs"]), be.upload(t["loci"])
    d_weights = None if t["weights"] is None else be.upload(t["weights"])
    n_loci, n_words = len(t["loci"]), 2 * int(t["n_merges"].sum())
    d_ws, d_merges, d_status = be.empty(8 * t["ws_alloc"]), be.full(4 * n_words + 2 * tc.GUARD, tc.POISON), be.full(4 * n_loci, tc.POISON)
    be.call(entry, be.ptr(d_shared), t["shared_words"], be.ptr(d_nw), be.ptr(d_seqs), len(t["nw"]), be.ptr(d_loci), n_loci,
            0 if d_weights is None else be.ptr(d_weights), be.ptr(d_ws), t["ws_words"], be.ptr(d_merges) + tc.GUARD, t["merges_words"],
            be.ptr(d_status), be.stream)
    raw = be.download(d_merges, np.uint8, 4 * n_words + 2 * tc.GUARD)
    assert (raw[:tc.GUARD] == tc.POISON).all() and (raw[tc.GUARD + 4 * n_words:] == tc.POISON).all()
    flat = raw[tc.GUARD:tc.GUARD + 4 * n_words].view(np.int32)
    off = 2 * sa.exclusive_sum(t["n_merges"])
    got = [[tuple(p) for p in flat[o:o + 2 * n].reshape(-1, 2).tolist()] for o, n in zip(off.tolist(), t["n_merges"].tolist())]
    return be.download(d_status, np.int32, n_loci).tolist(), got


def trees(be, loci, weighted, entry=WIDE):
    status, got = call(be, tc.tables(loci, weighted), entry)
    assert status == [0] * len(loci)
    return got


def scaled(l, k=SCALE):
    """The locus with every weight k times what it was."""
    return tc.Locus(l.D, l.leaf, l.w * k)


# ---- 1. the same trees below the old limit
def check_same_below_limit(be, weighted):
    """tree_common's small and edge loci (the wavefront, the 256 threads and TR_LDS_M = 512 from both sides) through the wide
    entry: mprg_prog_tree's merges, the host's and the plain statement's.  (Unweighted, the host's tree is there for every edge
    locus, and tree_common pins mprg_prog_tree to it; weighted it is there for three m, so mprg_prog_tree is run beside it.)"""
    small, edge = tc.small_loci(), tc.edge_loci()
    assert {l.m for l in edge} == set(tc.EDGE_M)
    got = trees(be, small, weighted)
    assert got == trees(be, small, weighted, "mprg_prog_tree")
    for l, g, want in zip(small, got, tc.small_spec(weighted)):
        assert tc.nested(g) == want and g == l.host(weighted), (l.m, weighted)
    got = trees(be, edge, weighted)                                      # loci of different m in one launch
    if weighted:
        assert got == trees(be, edge, weighted, "mprg_prog_tree")
    hosts = [g == s for g, s in zip(got, tc.edge_spec(weighted)) if s is not None]
    assert all(hosts) and len(hosts) == (2 * len(tc.WEIGHTED_EDGE_M) if weighted else len(edge))


# ---- 2. scale invariance across the old limit
def check_scale_invariance(be):
    """The weighted edge loci with every weight x 256: weight sums above 4 096 and at most 2^20, the merges of the unscaled loci."""
    picked = [(l, s) for l, s in zip(tc.edge_loci(), tc.edge_spec(True)) if s is not None]
    assert {l.m for l, _ in picked} == set(tc.WEIGHTED_EDGE_M)
    sums = [int(l.w.sum()) * SCALE for l, _ in picked]
    assert all(sa.PROG_MAX_LEAVES < s <= TOP for s in sums) and max(sums) > TOP // 2
    assert trees(be, [scaled(l) for l, _ in picked], True) == [s for _, s in picked]


# ---- 3. exactness where float64 ties
def check_exact(be):
    """tree_common.exact_loci with every weight x 256: the cross products of the fifth merge are above 2^85 and differ by g 2^32,
    their float64 quotients are equal as before (a power of two scales exactly): (4, 6) is merged, not (0, 2)."""
    loci = tc.exact_loci()
    for l in loci:
        w = (l.w * SCALE).tolist()
        q1, q2 = (w[0] + w[1]) * (w[2] + w[3]), (w[4] + w[5]) * (w[6] + w[7])
        p1 = sum(w[a] * w[b] * int(l.D[a, b]) for a in (0, 1) for b in (2, 3))
        p2 = sum(w[a] * w[b] * int(l.D[a, b]) for a in (4, 5) for b in (6, 7))
        assert p2 * q1 > 1 << 85 and p1 * q2 - p2 * q1 == int(np.gcd(q1, q2)) * SCALE ** 2 > 0 and p1 / q1 == p2 / q2 and sum(w) <= TOP
    got = trees(be, [scaled(l) for l in loci], True)
    for l, g in zip(loci, got):
        assert tc.nested(g) == l.plain(True) and g[:5] == [(0, 1), (2, 3), (4, 5), (6, 7), (4, 6)], l.w
        assert g == scaled(l).host(True)


# ---- 4. products that leave 64 bits
def _wrap(x):
    """x as a signed 64-bit integer holds it."""
    return (x + (1 << 63)) % (1 << 64) - (1 << 63)


def upgma_wrapped(D, leaves, w):
    """collapse_ref.upgma with every cross product wrapped to int64: what a kernel that multiplies in 64 bits computes."""
    members = {i: [i] for i in leaves}
    tree = {i: i for i in leaves}
    while len(members) > 1:
        keys = sorted(members)
        best = None
        for x, u in enumerate(keys):
            for v in keys[x + 1:]:
                s = sum(w[a] * w[b] * D[a][b] for a in members[u] for b in members[v])
                n = sum(w[a] for a in members[u]) * sum(w[b] for b in members[v])
                if best is None or _wrap(s * best[1]) < _wrap(best[0] * n):
                    best = (s, n, u, v)
        _, _, u, v = best
        members[u] += members.pop(v)
        tree[u] = (tree[u], tree.pop(v))
    return tree[min(tree)]


@functools.lru_cache(maxsize=None)
def overflow_loci():
    """Random loci of 8 to 17 leaves (18 leaves of 60 000 or more are over 2^20) with weights drawn from 60 000 .. 131 072, the sum at
    or below 2^20, D from 0 .. 65 536, an empty record in front and one inside; per locus the exact tree."""
    rng = np.random.default_rng(3)
    out = []
    for n in (8, 8, 9, 11, 13, 15, 17, 17):
        l = tc.random_locus(rng, n, tc.NW, [0, 3])
        hi = min(131072, 60000 + 2 * (TOP - 60000 * n) // n)
        while True:
            w = rng.integers(60000, hi + 1, n)
            if int(w.sum()) <= TOP:
                break
        l.w[l.leaf] = w
        out.append((l, cr.upgma(l.D.tolist(), l.leaves, l.w.tolist())))
    return out


def check_overflow(be):
    loci = overflow_loci()
    for l, want in loci:                                                 # the condition on the inputs: 64-bit products give another tree
        assert want != upgma_wrapped(l.D.tolist(), l.leaves, l.w.tolist()), l.w
        assert l.w[l.leaf].min() >= 60000 and l.w.max() <= 131072 and sa.PROG_MAX_LEAVES < int(l.w.sum()) <= TOP
    got = trees(be, [l for l, _ in loci], True)
    for (l, want), g in zip(loci, got):
        assert tc.nested(g) == want and g == l.host(True), l.w


# ---- 5. the limit and the refusals
def check_refusals(be):
    rng = np.random.default_rng(8)
    a, c = tc.random_locus(rng, 5, 3, [2]), tc.random_locus(rng, 6, tc.NW, [0, 3])
    b = tc.random_locus(rng, 4, 100, [1])
    loci = [a, b, c]
    blank = [(tc.BLANK, tc.BLANK)] * 3
    want_a, want_c = a.host(True), c.host(True)
    for w in ([TOP // 4, TOP // 4, TOP // 4, TOP // 4 + 1], [TOP + 1, 1, 1, 1], [TOP, 1, 1, 1]):   # a sum of 2^20 + 1; one weight of it
        b.w[b.leaf] = w
        assert call(be, tc.tables(loci, True)) == ([0, 1, 0], [want_a, blank, want_c]), w
    b.w[b.leaf] = [TOP // 4 + 3, TOP // 4, TOP // 4 - 1, TOP // 4 - 2]                           # ... and exactly 2^20 is built
    assert int(b.w.sum()) == TOP
    want_b = b.host(True)
    assert tc.nested(want_b) == b.plain(True)
    assert call(be, tc.tables(loci, True)) == ([0, 0, 0], [want_a, want_b, want_c])

    def tripped(code, **change):
        t = tc.tables(loci, True)
        for key, value in change.items():
            if key in ("toff", "woff", "moff", "first", "m"):
                t["loci"][1, ("first", "m", "toff", "woff", "moff").index(key)] = value(t) if callable(value) else value
            else:
                t[key] = value(t) if callable(value) else value
        assert call(be, t) == ([0, code, 0], [want_a, blank, want_c]), change
    tripped(1, toff=lambda t: t["shared_words"] - b.m * b.m + 1)             # the table ends one word outside shared_words
    tripped(1, toff=-1)
    tripped(1, moff=lambda t: t["merges_words"] - 6 + 1)                     # the merges end one element outside merges_words
    tripped(1, moff=-2)
    tripped(1, first=lambda t: len(t["nw"]) - b.m + 1)                       # the sequences end outside n_seqs
    tripped(1, m=0)
    tripped(3, woff=lambda t: t["ws_words"] - sa.prog_tree_words(b.m) + 1)   # the workspace one word short
    tripped(3, woff=-1)
    leaf = int(sum(l.m for l in loci[:1])) + b.leaves[2]
    for low in (0, -3):
        def weights(t, low=low):
            t["weights"][leaf] = low
            return t["weights"]
        tripped(1, weights=weights)                                          # a leaf's weight below 1
    t = tc.tables(loci, True)                                                # the last locus's table one word outside: the others are built
    t["shared_words"] -= 1
    assert call(be, t) == ([0, 0, 1], [want_a, want_b, [(tc.BLANK, tc.BLANK)] * 5])
    t = tc.tables(loci, True)
    t["ws_words"] -= 1
    assert call(be, t) == ([0, 0, 3], [want_a, want_b, [(tc.BLANK, tc.BLANK)] * 5])


def check_prog_trees(be):
    """star_align.prog_trees routes by weight sum: a locus of weights x 1 024 through the wide entry, its tree unchanged, next to
    one left as it is; a weight sum above 2^20 raises."""
    ls = [pr.clade_locus(31, 9, L=(50, 72)), pr.clade_locus(32, 7, L=(50, 72))]
    codes = [sa.locus_codes(str(k), pc.records(l)) for k, l in enumerate(ls)]
    w = [np.arange(1, 10), np.arange(1, 8)]
    want = sa.prog_trees(be, codes, w)
    wrapped = tr.TraceBackend(be)
    assert sa.prog_trees(wrapped, codes, [w[0] * 1024, w[1]]) == want
    calls = [line.split()[1] for line in wrapped.lines if line.startswith("call ")]
    assert calls == ["mprg_prog_distances", "mprg_prog_tree", "mprg_prog_distances", WIDE]
    try:
        sa.prog_trees(be, codes, [w[0] * 1024 * 32, w[1]])
    except sa.StarAlignError as e:
        assert WIDE in str(e)
    else:
        raise AssertionError("a weight sum above 2^20 was built")


# ---- whole MSAs
def _copies(rng, alleles, n, singles=()):
    """n records over the alleles, every allele at least once, those of `singles` exactly once, in random order."""
    many = [a for k, a in enumerate(alleles) if k not in singles]
    out = list(alleles) + [rng.choice(many) for _ in range(n - len(alleles))]
    rng.shuffle(out)
    return out


@functools.lru_cache(maxsize=None)
def loci():
    """4 097 records over ten alleles of two clades (one past the old limit); 6 003 records over eleven diverged alleles of which
    one has a single record, five empty records among them; an ordinary locus of ten records.  50 to 80 nt."""
    rng = random.Random(41)
    first = _copies(rng, pr.clade_locus(21, 10, L=(50, 72)), 4097)
    root = "".join(rng.choice("ACGT") for _ in range(66))
    fam = [sr.mutate(rng, root, 0.06, 0.03) for _ in range(11)]
    second = _copies(rng, fam, 5998, singles=(4,))
    for at in (0, 17, 3000, 3001, 6002):
        second.insert(at, "--" if at == 17 else "")
    third = pr.clade_locus(22, 8, L=(50, 72))
    third = third[:5] + [third[1]] + third[5:] + [third[6]]
    out = [first, second, third]
    assert [len(l) for l in out] == [4097, 6003, 10] and max(len(s) for l in out for s in l) <= 80
    assert [cc.n_classes(l)[2] for l in out] == [10, 11, 8] and second.count(fam[4]) == 1
    return out


@functools.lru_cache(maxsize=None)
def spec():
    """Per locus large_ref's (rows, progression, merges)."""
    return [lr.progressive(l) for l in loci()]


def fasta(msas):
    return [sa.msa_fasta(m) for m in msas]


@functools.lru_cache(maxsize=None)
def _host_tree_fasta(be):
    """The MSAs with the flag on and the host's tree, once per backend: what the compositions are compared with."""
    return fasta(sa.star_msas(be, [pc.records(l) for l in loci()], progressive=True, collapse=True, large_loci=True))


def check_bytes_and_counters(be):
    """The flag on: large_ref's rows and progression; off: the star bytes for the two big loci; the small locus the same in both."""
    recs = [pc.records(l) for l in loci()]
    info, timings = [], {}
    on = sa.star_msas(be, recs, progressive=True, collapse=True, large_loci=True, progression=info, timings=timings)
    for l, m, got, (rows, want, _) in zip(loci(), on, info, spec()):
        assert m.rows_as_strings() == rows and got == want and not want[2]
        assert m.descriptions == [t for t, _ in pc.records(l)]
        cc.invariants(l, rows)                                           # gaps removed: the input; equal sequences: equal rows
    assert fasta(on) == _host_tree_fasta(be)
    assert timings["large_loci"] == 2 and timings["large_records"] == 4097 + 6003 and timings["large_fallbacks"] == 0
    assert timings["collapse_merges"] == sum(m for _, _, m in spec()) == 9 + 10 + 7
    info = []
    off = sa.star_msas(be, recs, progressive=True, collapse=True, progression=info)
    star = sa.star_msas(be, recs, collapse=True)                         # (its pair stage runs once per class)
    assert fasta(off)[:2] == fasta(star)[:2] and fasta(off)[:2] != fasta(on)[:2]
    assert info[:2] == [(4097, 0, True), (5998, 0, True)] and info[2] == spec()[2][1]
    assert fasta(off)[2] == fasta(on)[2] != fasta(star)[2]
    assert off[2].rows_as_strings() == cr.progressive(loci()[2])[0]


def check_compositions(be):
    """device_tree, band, a budget that forces groups: the host tree's bytes."""
    recs = [pc.records(l) for l in loci()]
    want = _host_tree_fasta(be)
    kw = dict(progressive=True, collapse=True, large_loci=True)
    timings = {}
    assert fasta(sa.star_msas(be, recs, device_tree=True, timings=timings, **kw)) == want and timings["tree_device_loci"] == 3
    assert fasta(sa.star_msas(be, recs, band=True, **kw)) == want
    assert fasta(sa.star_msas(be, recs, band=True, device_tree=True, **kw)) == want
    plain, grouped = tr.TraceBackend(be), tr.TraceBackend(be)
    assert fasta(sa.star_msas(plain, recs, device_tree=True, **kw)) == want
    assert fasta(sa.star_msas(grouped, recs, device_tree=True, budget_bytes=4 * pa.workspace_words(90, 90), **kw)) == want
    n = [sum(line.startswith("call mprg_prog_columns_weighted ") for line in b.lines) for b in (plain, grouped)]
    assert n[1] > n[0]


@functools.lru_cache(maxsize=None)
def flipped():
    """The 4 097-record locus with a seeded half of its records reverse-complemented: (the records' sequences, strand_ref's reversed
    flags, the oriented sequences, large_ref's rows and progression of those)."""
    l, _ = st.flip(random.Random(43), loci()[0], 0.5)
    rev, _, ori = st.oriented(l)
    assert 1500 < sum(rev) < 2600 and cc.n_classes(l)[2] > cc.n_classes(ori)[2] == 10
    return (l, rev, ori) + lr.progressive(ori)[:2]


def check_adjust_direction(be):
    """Classes that exist only after the orientation: the rows of the oriented records, _R_ titles, with either tree."""
    l, rev, ori, rows, want = flipped()
    recs = pc.records(l)
    for device_tree in (False, True):
        info = []
        m, = sa.star_msas(be, [recs], progressive=True, collapse=True, large_loci=True, adjust_direction=True, device_tree=device_tree,
                          progression=info)
        assert m.descriptions == st.titles(recs, rev) and m.rows_as_strings() == rows
        assert info == [want] and want[0] == 10 and not want[2]
        cc.invariants(ori, rows)


def _objective(rows):
    """The spec's S (Refinement, Objective) of an MSA's rows, by column counts."""
    R, runs, total = len(rows), 0, 0
    for r in rows:
        runs += sum(1 for j, x in enumerate(r) if x == "-" and (j == 0 or r[j - 1] != "-"))
    for j in range(len(rows[0])):
        col = [r[j] for r in rows]
        c = [col.count(x) for x in "ACGT"]
        g = col.count("-")
        total += 20 * sum(x * (x - 1) // 2 for x in c) - 9 * sum(c[i] * c[k] for i in range(4) for k in range(i + 1, 4)) - 10 * g * (R - g)
    return 2 * total - 11 * (R - 1) * runs


def check_refine_tree(be):
    """refine_tree=1 on all three loci: S never falls (and is the S of the rows that come back), equal sequences keep equal rows,
    band and device_tree give the same bytes."""
    recs = [pc.records(l) for l in loci()]
    kw = dict(progressive=True, collapse=True, large_loci=True, refine_tree=1)
    info, timings = [], {}
    msas = sa.star_msas(be, recs, tree_refinement=info, timings=timings, **kw)
    before = sa.star_msas(be, recs, progressive=True, collapse=True, large_loci=True)
    for l, m, b, (tried, accepted, skipped, s0, s1) in zip(loci(), msas, before, info):
        cc.invariants(l, m.rows_as_strings())
        assert tried > 0 and skipped == 0 and s1 >= s0 and (s1 > s0) == (accepted > 0)
        assert s0 == _objective(b.rows_as_strings()) and s1 == _objective(m.rows_as_strings())
    assert timings["tree_refine_loci"] == 3 and "tree_refine_over_bound" not in timings
    assert fasta(sa.star_msas(be, recs, band=True, device_tree=True, **kw)) == fasta(msas)


def check_refine(be):
    """refine=1 on the 4 097-record locus alone: the rows are the input, equal sequences keep equal rows, S does not fall."""
    l = loci()[0]
    info = []
    m, = sa.star_msas(be, [pc.records(l)], progressive=True, collapse=True, large_loci=True, device_tree=True, refine=1, refinement=info)
    cc.invariants(l, m.rows_as_strings())
    assert info[0][2] >= info[0][1] == _objective(spec()[0][0]) and info[0][2] == _objective(m.rows_as_strings())


@functools.lru_cache(maxsize=None)
def limit_loci():
    """60 records over five alleles; 12 records over three."""
    rng = random.Random(47)
    return [_copies(rng, pr.clade_locus(23, 5, L=(50, 72)), 60), _copies(rng, pr.clade_locus(24, 3, L=(50, 72)), 12)]


def check_limits(be):
    """max_records and max_leaves by parameter: a locus over either falls back to the star bytes and is counted."""
    ls = limit_loci()
    assert [cc.n_classes(l)[2] for l in ls] == [5, 3]
    recs = [pc.records(l) for l in ls]
    star = fasta(sa.star_msas(be, recs, collapse=True))
    want = [lr.progressive(l)[0] for l in ls]
    assert fasta(sa.star_msas(be, recs, progressive=True, collapse=True, large_loci=True))[0] != star[0]
    for limit, n_large in ((dict(max_records=50), 0), (dict(max_leaves=3), 1)):
        for device_tree in (False, True):
            info, timings = [], {}
            msas = sa.star_msas(be, recs, progressive=True, collapse=True, large_loci=True, device_tree=device_tree, progression=info,
                                timings=timings, **limit)
            assert fasta(msas)[0] == star[0] and msas[1].rows_as_strings() == want[1], limit
            assert info == [(60, 0, True), lr.progressive(ls[1], **limit)[1]] and info[1][:1] + info[1][2:] == (3, False)
            assert lr.progressive(ls[0], **limit)[1] == (60, 0, True)
            assert timings["large_fallbacks"] == 1 and timings["large_loci"] == n_large and timings["large_records"] == 12 * n_large
    # without the flag max_leaves counts records: both fall back
    info = []
    sa.star_msas(be, recs, progressive=True, collapse=True, max_leaves=3, progression=info)
    assert info == [(60, 0, True), (12, 0, True)]


def check_parameters(be):
    for kw in (dict(large_loci=True), dict(large_loci=True, progressive=True), dict(large_loci=True, collapse=True),
               dict(progressive=True, collapse=True, max_records=50)):
        try:
            sa.star_msas(be, [[("a", "ACGT")]], **kw)
        except ValueError as e:
            assert "large_loci" in str(e), kw
        else:
            raise AssertionError(f"accepted: {kw}")
    assert sa.PROG_MAX_RECORDS == TOP == lr.MAX_RECORDS


# ---- what moves between host and device
def check_trace(be):
    """With large_loci and device_tree: mprg_prog_tree_wide for the two big loci only, right behind their mprg_prog_distances call;
    the small locus through mprg_prog_tree; no uint32 table comes back.  Without large_loci neither big locus has a tree."""
    recs = [pc.records(l) for l in loci()]
    wrapped = tr.TraceBackend(be)
    msas = sa.star_msas(wrapped, recs, progressive=True, collapse=True, large_loci=True, device_tree=True)
    assert fasta(msas) == _host_tree_fasta(be)
    calls = [line.split() for line in wrapped.lines if line.startswith("call ")]
    names = [c[1] for c in calls]
    assert names.count(WIDE) == 1 and names.count("mprg_prog_tree") == 1 and names.count("mprg_prog_distances") == 2
    at = names.index(WIDE)
    assert names[at - 1] == "mprg_prog_distances" and names[names.index("mprg_prog_tree") - 1] == "mprg_prog_distances"
    assert calls[at][2 + 6] == "2" and calls[names.index("mprg_prog_tree")][2 + 6] == "1"       # n_loci
    assert not any(line.startswith("download uint32") for line in wrapped.lines)
    wrapped = tr.TraceBackend(be)
    sa.star_msas(wrapped, recs, progressive=True, collapse=True, device_tree=True)
    names = [line.split()[1] for line in wrapped.lines if line.startswith("call ")]
    assert WIDE not in names and names.count("mprg_prog_tree") == 1
