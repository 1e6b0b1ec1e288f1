"""mprg_cluster_further's one-workgroup form admits a view by its REPRESENTATIVES when the call has rep_g (the form stages only their
cells): tables by the S rows, k majority strings, G rows of cells, G = distinct gapped rows.  Hand-built tables through
mprg_cluster_further_bounded (no rep_g: the rule by S) and mprg_cluster_further_classes against the restatement of the reference in
tests/cf_classes_cases.py, and WHICH side took a view, read from the work lists: the tiled kernels only ever see the views their lists
name, so a call whose lists leave a view out shows what the one-workgroup form does with it alone (the right answer, or nothing).
Shared by tests/test_cf_rep_rule_emulated.py and tests/test_gpu_cf_rep_rule.py."""
import itertools

import numpy as np

from tests import cf_classes_cases as cc

VF = PF = 12
POOL = cc.POOL
KMAX = 10              # KM_KMAX: G of a view that asks for it sits behind the view's KMAX majority strings in `scratch`


def tables(S):
    return ((S + 3) & ~3) + ((2 * S + 3) & ~3) + 4 * S


def bytes_by_reps(S, n, k, G):
    cp = (n + 3) & ~3
    return tables(S) + k * cp + G * cp


def one_takes(S, n, k, G, cls, by_reps):
    """The rule, restated: without rep_g by the rows and the narrow tables; with it by the rows (switch off) or the representatives."""
    if not cls:
        return cc.one_fits(S, n, k, False)
    return 1 <= S < 65536 and n >= 1 and bytes_by_reps(S, n, k, G if by_reps else S) <= POOL


def reps_of(p):
    rg = cc.rep_g_of(p["rows"])
    return int((rg == np.arange(len(rg))).sum())


# ---- the problems -----------------------------------------------------------------------------------------------------------
def classes_problem(rng, S, n, G, alphabet=(1, 2, 3, 4), spread=False, min_len=1, short_rows=0):
    """S rows in exactly G gapped classes (+ one class of short rows, which sit out: d_of_row = -1).  Class 0 holds every row beyond the
    first G, or (spread) the rows are dealt out evenly.  No symbol is code 0 unless the alphabet has it: a majority string that was written
    differs from the zeroed scratch."""
    if len(alphabet) ** n <= 4 * G:
        pool = [np.array(t, np.uint8) for t in itertools.product(alphabet, repeat=n)]
        pool = [pool[0]] + [pool[i] for i in 1 + rng.permutation(len(pool) - 1)]
        if alphabet[0] == 0:                               # (class 0, the heavy one, without a zero)
            pool.sort(key=lambda r: 0 if (r != 0).all() else 1)
        cls_rows = pool[:G]
    else:
        seen, cls_rows = set(), []
        while len(cls_rows) < G:
            r = rng.choice(alphabet, n).astype(np.uint8)
            if r.tobytes() not in seen:
                seen.add(r.tobytes()); cls_rows.append(r)
    assert len(cls_rows) == G
    pick = np.concatenate([np.arange(G), (rng.integers(0, G, S - G) if spread else np.zeros(S - G, np.int64))])
    rows = np.array([cls_rows[c] for c in pick], np.uint8)
    if short_rows:
        short = np.array([alphabet[-1]] + [4] * (n - 1), np.uint8)
        assert short.tobytes() not in {r.tobytes() for r in cls_rows}
        rows[rng.choice(np.arange(G, S), short_rows, replace=False)] = short
    p = cc.problem(rows, min_len=min_len)
    assert reps_of(p) == G + (1 if short_rows else 0)
    return p


def at_the_bound(k):
    """1 000 rows x 4 columns: tables 7 000 bytes, 4 per string and per representative — 8 192 exactly at G = 298 - k, 8 196 one above."""
    G = 298 - k
    assert bytes_by_reps(1000, 4, k, G) == 8192 and bytes_by_reps(1000, 4, k, G + 1) == 8196
    rng = np.random.default_rng(40 + k)
    return [classes_problem(rng, 1000, 4, G, alphabet=(0, 1, 2, 3, 4)), classes_problem(rng, 1000, 4, G + 1, alphabet=(0, 1, 2, 3, 4))]


def cases(k):
    """[(name, problem)]; every view's expected side is asserted in check_split from the restated rule, and here for the named shapes."""
    rng = np.random.default_rng(100 + k)
    out = [("120x80 G=1", classes_problem(rng, 120, 80, 1)), ("120x80 G=2", classes_problem(rng, 120, 80, 2)),
           ("120x80 G=40", classes_problem(rng, 120, 80, 40, spread=True)),
           ("120x80 G=40 root-like", cc.problem(cc.random_rows(rng, 120, 80, 40, alphabet=(1, 2, 3, 4), p_mut=0.05))),
           ("120x80 G=100: by neither", classes_problem(rng, 120, 80, 100, spread=True)),
           ("20x20: by S as before", classes_problem(rng, 20, 20, 9, spread=True)),
           ("120x80 G=30, rows sit out", classes_problem(rng, 120, 80, 30, spread=True, min_len=5, short_rows=17)),
           ("103x80 G=48", classes_problem(rng, 103, 80, 48, spread=True)),
           ("1025x20 G=3: tall", classes_problem(rng, 1025, 20, 3, spread=True)),
           ("1025x20 G=60: tall, by neither", classes_problem(rng, 1025, 20, 60, spread=True))]
    a, b = at_the_bound(k)
    out += [("1000x4 at 8192", a), ("1000x4 at 8196", b)]
    side = {name: one_takes(*p["rows"].shape, k, reps_of(p), True, True) for name, p in out}
    assert side["120x80 G=1"] and side["120x80 G=2"] and side["120x80 G=40"] and side["103x80 G=48"] and side["1000x4 at 8192"]
    assert side["20x20: by S as before"] and side["1025x20 G=3: tall"] and side["120x80 G=30, rows sit out"]
    assert not side["120x80 G=100: by neither"] and not side["1000x4 at 8196"] and not side["1025x20 G=60: tall, by neither"]
    assert sum(one_takes(*p["rows"].shape, k, reps_of(p), True, False) for _, p in out) == 1          # (by S: the 20 x 20 view alone)
    return out


# ---- packing and the call (cf_classes_cases.run with work lists of the caller's choice) ---------------------------------------
def run(be, probs, k, entry, listed, gcodes=True):
    """listed: the problems the tiled kernels' work lists name (never empty).  Returns (out_further, [assign], [scratch bytes of the view's
    k majority strings], [the two bytes behind its KMAX strings])."""
    nP = len(probs)
    views, prob = np.zeros((nP, VF), np.int64), np.zeros((nP, PF), np.int64)
    g_parts, dor_parts, rg_parts, lab_parts, wc, wr = [], [], [], [], [], []
    goff = roff = coff = loff = 0
    cls = entry == "classes"
    for b, p in enumerate(probs):
        S, n = p["rows"].shape
        pitch = (n + 15) // 16 * 16
        g = np.full((S, pitch), 0xEE, np.uint8)
        g[:, :n] = p["rows"]
        views[b] = [0, 0, pitch, 0, -1, S, 0, n, coff, roff, goff, 0]
        prob[b, 0], prob[b, 1], prob[b, 7], prob[b, 10] = b, p["D"], 1, loff
        g_parts.append(g.reshape(-1)); dor_parts.append(p["dor"]); rg_parts.append(cc.rep_g_of(p["rows"]))
        lab = p["labels"] if p["labels"] is not None else np.zeros(max(p["D"], 1), np.int32)
        lab_parts.append(lab)
        if b in listed:
            tile, chunk = (32 if S > 1024 else 256), (16 if (n >= 512 and S > 1024) else 256)
            wc += [(b, t) for t in range((n + tile - 1) // tile)]
            wr += [(b, t) for t in range((S + chunk - 1) // chunk)]
        goff += g.size; roff += S; coff += n; loff += len(lab)
    assert wc and wr
    labels = np.concatenate(lab_parts)
    d_views, d_prob = be.upload(views), be.upload(prob)
    d_g = be.upload(np.concatenate(g_parts + [np.zeros(64, np.uint8)]))
    d_dor, d_rg = be.upload(np.concatenate(dor_parts)), be.upload(np.concatenate(rg_parts))
    d_lab = be.upload(labels) if k > 1 else None
    d_assign = be.upload(np.full(len(labels), cc.POISON, np.int32)) if k > 1 else None
    d_wc, d_wr = be.upload(np.array(wc, np.int32)), be.upload(np.array(wr, np.int32))
    d_scr, d_out = be.zeros(12 * coff + 64), be.full(4 * nP, 0x55)
    d_dummy = be.zeros(64)
    P = lambda x: be.ptr(x) if x is not None else None
    args = [be.ptr(d_dummy), be.ptr(d_views), be.ptr(d_dummy), be.ptr(d_prob), nP, k, be.ptr(d_dor), P(d_lab), P(d_assign), be.ptr(d_wc), len(wc),
            be.ptr(d_wr), len(wr), be.ptr(d_scr), be.ptr(d_out), None, be.ptr(d_g) if gcodes else None, None, 0]
    be.call("mprg_cluster_further_" + entry, *args, *([be.ptr(d_rg)] if cls else []), be.stream)
    be.synchronize()
    out = be.download(d_out, np.int32, nP)
    asg = be.download(d_assign, np.int32, len(labels)) if k > 1 else np.zeros(0, np.int32)
    scr = be.download(d_scr, np.uint8, 12 * coff + 64)
    assigns, majs, slots = [], [], []
    for b, p in enumerate(probs):
        S, n = p["rows"].shape
        lo, co = int(prob[b, 10]), int(views[b, 8])
        assigns.append(asg[lo:lo + max(p["D"], 1)] if k > 1 else None)
        majs.append(scr[12 * co:12 * co + k * n].reshape(k, n).copy())
        slots.append(int(scr[12 * co + KMAX * n]) | int(scr[12 * co + KMAX * n + 1]) << 8)
    return out, assigns, majs, slots


def check_split(be, named, k, entry, by_reps=True):
    """Three calls on the same tables: work lists naming every view, only the tiled side's views, only the one-workgroup side's.  Every view
    gets the reference's answer from the side the rule names — alone — and nothing from the other.
    What this cannot see: the tiled side walking a view the one-workgroup form admitted by its representatives as well (it would write the
    same strings and the same flag; tried by making the tiled kernels keep the rule by rows: nothing fails).  For the views that fit by
    their rows the zeroed strings show it; a view neither side takes, and a one-workgroup form that admits by G + 1, fail."""
    rng = np.random.default_rng(7 * k)
    named = named + [("(a view both lists can always name)", cc.problem(np.full((2, 2), 1, np.uint8)))]
    probs = [cc.with_labels(p, k, rng) if k > 1 else p for _, p in named]
    nP, last = len(probs), len(probs) - 1
    cls = entry == "classes"
    want = [cc.expect(p, k) for p in probs]
    one = [one_takes(*p["rows"].shape, k, reps_of(p), cls, by_reps) for p in probs]
    by_s = [one_takes(*p["rows"].shape, k, reps_of(p), cls, False) for p in probs]
    assert one[last] and any(one[:last]) and not all(one[:last])
    lists = dict(every=set(range(nP)), tiled={b for b in range(nP) if not one[b]} | {last}, one={b for b in range(nP) if one[b]})
    for which, listed in lists.items():
        out, assigns, majs, slots = run(be, probs, k, entry, listed)
        for b, p in enumerate(probs):
            tag = f"{entry}, k = {k}, lists of {which}, {named[b][0]}"
            lab = p["labels"] if k > 1 else None
            used = {0 if lab is None else int(lab[d]) for d in p["dor"] if d >= 0}
            if which == "one" and not one[b]:
                # the tiled side's view, left out of its lists: nobody answers — the one-workgroup form did not claim it
                assert out[b] == 0 and not majs[b].any() and (k == 1 or (assigns[b] == cc.POISON).all()), tag
                assert any(want[b][1][cl].any() for cl in used), tag          # (its strings, had they been written, are not all zero)
                continue
            assert bool(out[b]) == want[b][0], tag
            if k > 1:
                assert (assigns[b][:p["D"]] == p["labels"][:p["D"]]).all(), tag
            if one[b] and by_s[b]:
                assert not majs[b].any(), tag          # (as before the rule: the one-workgroup form keeps its strings in LDS; the tiled side left the view alone)
            else:
                for cl in used:
                    assert (majs[b][cl] == want[b][1][cl]).all(), f"{tag}: majority string of cluster {cl}"
            S, n = p["rows"].shape
            asks = cls and by_reps and not by_s[b] and bytes_by_reps(S, n, k, 1) <= POOL and S < 65536
            assert slots[b] == (reps_of(p) if asks else 0), tag          # (G is counted only where the rule turns on it)
    return one


def check_all(be, by_reps=True, classes=True):
    """k = 1, 2, 10 through both entry points.  by_reps / classes: what the library's switches say (MPRG_CF_REP_RULE, MPRG_CF_CLASSES)."""
    for k in (1, 2, 10):
        named = cases(k)
        check_split(be, named, k, "bounded")
        # (MPRG_CF_CLASSES=0: the library drops rep_g — the rule and the split are mprg_cluster_further_bounded's)
        one = check_split(be, named, k, "classes" if classes else "bounded", by_reps)
        if not classes:
            out_c = run(be, [cc.with_labels(p, k, np.random.default_rng(7 * k)) if k > 1 else p for _, p in named], k, "classes", set(range(len(named))))
            out_b = run(be, [cc.with_labels(p, k, np.random.default_rng(7 * k)) if k > 1 else p for _, p in named], k, "bounded", set(range(len(named))))
            assert (out_c[0] == out_b[0]).all() and all((a == b).all() for a, b in zip(out_c[2], out_b[2])) and not any(out_c[3])
        moved = [name for (name, p), o in zip(named, one) if o and not one_takes(*p["rows"].shape, k, reps_of(p), True, False)]
        assert (len(moved) >= 6) == (by_reps and classes), moved


# ---- alignments -------------------------------------------------------------------------------------------------------------
def batch_digest(be, seeds) -> dict:
    """PRGs and tree dumps of config-C alignments through the per-step host with per-round launches (every mprg_cluster_further call is the
    entry point's), the per-step host with the fused loops, and mprg_forest_level (the second forest of a resident batch)."""
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
    out = {}
    eng = forest.ForestEngine(be, 5, 7)
    eng.load(msas)
    kloop, forest.KLOOP = forest.KLOOP, "rounds"
    try:
        eng.run_forest()
    finally:
        forest.KLOOP = kloop
    out["rounds"] = digest(eng)
    eng = forest.ForestEngine(be, 5, 7)
    eng.load(msas)
    kloop, forest.KLOOP = forest.KLOOP, "fused"
    try:
        eng.run_forest()
        out["per_step"] = digest(eng)
        syncs = eng.counters["syncs"]
        eng.run_forest()
        assert eng.counters["syncs"] == syncs + 1 and eng.counters.get("plan_misses", 0) == 0          # (enqueued from the plan: mprg_forest_level)
        out["level"] = digest(eng)
    finally:
        forest.KLOOP = kloop
    return out
