"""Hand-built tables for mprg_cluster_further_bounded / mprg_cluster_further_classes (the same call with mprg_ungap_dedupe's rep_g: every
class of identical gapped rows counted once, by its size) and a plain restatement of cluster_sequences.py:59-111 to hold both against.
A problem here is {rows: S x n cell codes, dor: distinct-sequence index per row (-1: a short sequence), labels: cluster per distinct
sequence}; run() packs a list of them into the device tables (dense gapped copies only: the kernels never touch the arena then),
calls one entry point and returns out_further, assign and — for the problems the tiled kernels take — the majority strings.
Shared by tests/test_cf_classes_emulated.py and tests/test_gpu_cf_classes.py."""
import numpy as np

VF = PF = 12
POOL = 8192            # CFO_POOL (csrc/k_cluster.inc)
POISON = -7


def lds_bytes(S, n, k, cls):
    cp = (n + 3) & ~3
    return ((S + 3) & ~3) + ((2 * S + 3) & ~3) + k * cp + S * cp + (4 * S if cls else 0)


def one_fits(S, n, k, cls):
    return 1 <= S < 65536 and n >= 1 and lds_bytes(S, n, k, cls) <= POOL


def rep_g_of(rows):
    seen, out = {}, np.empty(len(rows), np.int32)
    for i, r in enumerate(rows):
        out[i] = seen.setdefault(r.tobytes(), i)
    return out


def problem(rows, min_len=1, labels=None, dor=None):
    """dor by first appearance of the ungapped content (cluster_sequences.py:220-233) unless given; rows shorter than min_len are short."""
    rows = np.ascontiguousarray(rows, np.uint8)
    if dor is None:
        seen, dor = {}, np.empty(len(rows), np.int32)
        for i, r in enumerate(rows):
            u = r[r != 4].tobytes()
            dor[i] = -1 if len(u) < min_len else seen.setdefault(u, len(seen))
    dor = np.asarray(dor, np.int32)
    D = int(dor.max()) + 1 if len(dor) and dor.max() >= 0 else 0
    return dict(rows=rows, dor=dor, D=D, labels=None if labels is None else np.asarray(labels, np.int32))


def with_labels(p, k, rng, distinct=None):
    """Random clusters 0..k-1 per distinct sequence (distinct: use only that many of them)."""
    q = dict(p)
    q["labels"] = rng.integers(0, distinct or k, max(p["D"], 1)).astype(np.int32)
    return q


# ---- the reference, restated ------------------------------------------------------------------------------------------------
def expect(p, k):
    """(further, majority strings k x n) of one problem: Counter.most_common per column over the cluster's rows in the reference's order
    (distinct sequence, then row), ties to the symbol seen first; threshold 1 below 5 columns, else int(0.2 n)."""
    rows, dor = p["rows"], p["dor"]
    S, n = rows.shape
    lab = p["labels"] if k > 1 else None          # (k = 1: the check before any KMeans, one cluster)
    maj = np.zeros((k, n), np.uint8)
    thresh = 1 if n < 5 else int(0.2 * n)
    further = False
    for cl in range(k):
        mem = sorted((int(dor[i]), i) for i in range(S) if dor[i] >= 0 and (0 if lab is None else lab[dor[i]]) == cl)
        if not mem:
            continue
        sub = rows[[i for _, i in mem]] & 15
        for c in range(n):
            cnt, order = {}, []
            for x in sub[:, c]:
                if x < 12:
                    if x not in cnt:
                        cnt[x] = 0
                        order.append(x)
                    cnt[x] += 1
            best = max(cnt.values()) if cnt else 0
            maj[cl, c] = next((x for x in order if cnt[x] == best), 0)
        further = further or bool(((sub != maj[cl]).sum(axis=1) > thresh).any())
    return further, maj


# ---- packing and the call ---------------------------------------------------------------------------------------------------
def run(be, probs, k, entry, sat_out=(), not_accepted=(), use_info=False):
    """entry: "bounded" or "classes".  sat_out: problems whose kinfo says k = 0; not_accepted: problems whose km_info reports k - 1 distinct
    labels.  Returns (out_further, [assign of every problem], [majority strings (k x n) or None where the one-workgroup form ran])."""
    nP = len(probs)
    views, prob = np.zeros((nP, VF), np.int64), np.zeros((nP, PF), np.int64)
    g_parts, dor_parts, rg_parts, lab_parts, wc, wr = [], [], [], [], [], []
    goff = roff = coff = loff = 0
    cls = entry == "classes"
    for b, p in enumerate(probs):
        S, n = p["rows"].shape
        pitch = (n + 15) // 16 * 16
        g = np.full((S, pitch), 0xEE, np.uint8)          # (padding: the kernels mask what they read beyond a row)
        g[:, :n] = p["rows"]
        views[b] = [0, 0, pitch, 0, -1, S, 0, n, coff, roff, goff, 0]
        prob[b, 0], prob[b, 1], prob[b, 7], prob[b, 10] = b, p["D"], 1, loff
        g_parts.append(g.reshape(-1)); dor_parts.append(p["dor"]); rg_parts.append(rep_g_of(p["rows"]))
        lab = p["labels"] if p["labels"] is not None else np.zeros(max(p["D"], 1), np.int32)
        lab_parts.append(lab)
        tile, chunk = (32 if S > 1024 else 256), (16 if (n >= 512 and S > 1024) else 256)
        wc += [(b, t) for t in range((n + tile - 1) // tile)]
        wr += [(b, t) for t in range((S + chunk - 1) // chunk)]
        goff += g.size; roff += S; coff += n; loff += len(lab)
    labels = np.concatenate(lab_parts)
    d_views, d_prob = be.upload(views), be.upload(prob)
    d_g = be.upload(np.concatenate(g_parts + [np.zeros(64, np.uint8)]))
    d_dor, d_rg = be.upload(np.concatenate(dor_parts)), be.upload(np.concatenate(rg_parts))
    d_lab = be.upload(labels) if k > 1 else None
    d_assign = be.upload(np.full(len(labels), POISON, np.int32)) if k > 1 else None
    d_wc, d_wr = be.upload(np.array(wc, np.int32)), be.upload(np.array(wr, np.int32))
    d_scr, d_out = be.zeros(12 * coff + 64), be.full(4 * nP, 0x55)
    d_dummy = be.zeros(64)
    info = np.zeros((nP, 8)); info[:, 3] = k
    info[list(not_accepted), 3] = k - 1
    kinfo = np.zeros((nP, 5), np.int32); kinfo[:, 1] = k
    kinfo[list(sat_out), 1] = 0
    d_info, d_kinfo = (be.upload(info), be.upload(kinfo)) if use_info else (None, None)
    P = lambda x: be.ptr(x) if x is not None else None
    args = [be.ptr(d_dummy), be.ptr(d_views), be.ptr(d_dummy), be.ptr(d_prob), nP, k, be.ptr(d_dor), P(d_lab), P(d_assign), be.ptr(d_wc), len(wc),
            be.ptr(d_wr), len(wr), be.ptr(d_scr), be.ptr(d_out), P(d_info), be.ptr(d_g), P(d_kinfo), 0]
    be.call("mprg_cluster_further_" + entry, *args, *([be.ptr(d_rg)] if cls else []), be.stream)
    be.synchronize()
    out = be.download(d_out, np.int32, nP)
    asg = be.download(d_assign, np.int32, len(labels)) if k > 1 else np.zeros(0, np.int32)
    scr = be.download(d_scr, np.uint8, 12 * coff + 64)
    assigns, majs = [], []
    for b, p in enumerate(probs):
        S, n = p["rows"].shape
        lo, co = int(prob[b, 10]), int(views[b, 8])
        assigns.append(asg[lo:lo + max(p["D"], 1)] if k > 1 else None)
        majs.append(None if one_fits(S, n, k, cls) else scr[12 * co:12 * co + k * n].reshape(k, n).copy())
    return out, assigns, majs


def check(be, probs, k, sat_out=(), not_accepted=(), use_info=False):
    """Both entry points on the same tables against the restated reference and against each other."""
    want = [expect(p, k) for p in probs]
    res = {e: run(be, probs, k, e, sat_out, not_accepted, use_info) for e in ("bounded", "classes")}
    for e, (out, assigns, majs) in res.items():
        for b, p in enumerate(probs):
            tag = f"{e}, k = {k}, problem {b} ({p['rows'].shape[0]} x {p['rows'].shape[1]})"
            if b in sat_out:
                assert out[b] == 0, tag
                assert k == 1 or (assigns[b] == POISON).all(), tag
                continue
            assert bool(out[b]) == want[b][0], tag
            if k > 1:
                if b in not_accepted:
                    assert (assigns[b] == POISON).all(), tag
                else:
                    assert (assigns[b][:p["D"]] == p["labels"][:p["D"]]).all(), tag
            if majs[b] is not None:
                # (a cluster without rows leaves its string as it is; only the clusters that have members are compared)
                lab = p["labels"] if k > 1 else None
                used = {0 if lab is None else int(lab[d]) for d in p["dor"] if d >= 0}
                for cl in used:
                    assert (majs[b][cl] == want[b][1][cl]).all(), f"{tag}: majority string of cluster {cl}"
    assert (res["bounded"][0] == res["classes"][0]).all()


# ---- the cases --------------------------------------------------------------------------------------------------------------
def random_rows(rng, S, n, n_classes, alphabet=(0, 1, 2, 3, 4), p_mut=0.15):
    """S rows of n cells in n_classes gapped classes (class 0 the largest), each a root row mutated in a few columns."""
    root = rng.choice(alphabet, n)
    cls_rows = [root] + [np.where(rng.random(n) < p_mut, rng.choice(alphabet, n), root) for _ in range(n_classes - 1)]
    pick = np.minimum(rng.geometric(0.35, S) - 1, n_classes - 1)
    return np.array([cls_rows[c] for c in pick], np.uint8)


def all_identical():
    rng = np.random.default_rng(1)
    out = []
    for S in (1, 2, 63, 64, 65, 128, 129, 300, 302, 303, 355, 356, 1023, 1024, 1025):       # (302 | 303, 355 | 356: the two bounds of the one-workgroup form at 20 columns)
        out.append(problem(np.tile(rng.integers(0, 4, 20).astype(np.uint8), (S, 1))))
    out.append(problem(np.tile(rng.integers(0, 4, 300).astype(np.uint8), (65, 1))))           # (wide: the tiled kernels at few rows)
    return out


def no_identical():
    rng = np.random.default_rng(2)
    out = []
    for S, n in ((5, 9), (64, 20), (129, 33), (400, 20), (40, 300)):
        rows = rng.integers(0, 5, (S, n)).astype(np.uint8)
        rows[:, 0] = np.arange(S) % 4
        rows[:, 1] = (np.arange(S) // 4) % 4
        rows[:, 2] = (np.arange(S) // 16) % 4
        rows[:, 3] = (np.arange(S) // 64) % 4
        rows[:, 4] = (np.arange(S) // 256) % 4
        out.append(problem(rows))
    return out


def gapped_twins():
    """Rows equal without gaps, differently gapped: one distinct sequence (one cluster), separate classes."""
    A, C, G, T, _ = 0, 1, 2, 3, 4
    a, b, c = [A, C, _, G, T, A, _, C], [A, _, C, G, T, A, C, _], [_, A, C, G, _, T, A, C]
    small = problem(np.array([a, a, b, a, c, b, a, a], np.uint8))
    assert small["D"] == 1
    big = problem(np.array(([a] * 5 + [b] * 3 + [c]) * 120, np.uint8))                          # (1 080 x 8: tiled)
    return [small, big]


def ties():
    """Two symbols tie in weighted count; the key (distinct sequence, row) of the first row holding one of them decides."""
    A, C = 0, 1
    base = [2, 2, 3, 3, 2, 3, 2, 3, 2]                                                          # 10 columns: threshold 2
    r = lambda x, *mut: np.array([x] + [b ^ 1 if q in mut else b for q, b in enumerate(base)], np.uint8)
    # the deciding row represents a large class (rows 0-2, distinct sequence 0): A wins
    p1 = problem(np.array([r(A), r(A), r(A), r(C, 0), r(C, 1), r(C, 2)], np.uint8), dor=[0, 0, 0, 1, 2, 3])
    # ... is a singleton with a smaller distinct-sequence index than the class's (given out of row order on purpose): C wins
    p2 = problem(np.array([r(A), r(A), r(A), r(C, 0), r(C, 1), r(C, 2)], np.uint8), dor=[2, 2, 2, 1, 0, 3])
    # the same with the tie deciding the flag: 4 columns -> threshold 1; the loser's rows are then 2 away where they differ once more
    q = lambda x, y: np.array([x, 2, 3, y], np.uint8)
    p3 = problem(np.array([q(A, 2), q(A, 2), q(C, 3), q(C, 2)], np.uint8), dor=[0, 0, 1, 2])   # A wins, row 2 is (C, 3): 2 away
    p4 = problem(np.array([q(A, 2), q(A, 2), q(C, 3), q(C, 2)], np.uint8), dor=[1, 1, 0, 2])   # C wins: every row within 1
    tall = lambda p: problem(np.tile(p["rows"], (200, 1)), dor=np.tile(p["dor"], 200))          # (tiled; same ties at 200 x the weights)
    return [p1, p2, p3, p4, tall(p1), tall(p2), tall(p3), tall(p4)]


def widths():
    rng = np.random.default_rng(3)
    out = []
    for n in (1, 3, 4, 5, 63, 64, 65, 255, 256, 257):
        for S, ncl in ((6, 3), (40, 7), (700, 30)):
            out.append(problem(random_rows(rng, S, n, ncl), min_len=3 if n >= 63 else 1))
    return out


def thresholds():
    """A class exactly at the threshold (not further) and one past it (further): 4 columns -> 1, 10 -> 2, 23 -> int(4.6) = 4."""
    out = []
    for n in (4, 10, 23):
        t = 1 if n < 5 else int(0.2 * n)
        for pad in (1, 140):                    # (140: 980 rows, the tiled kernels)
            for d in (t, t + 1):
                maj, far = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
                far[:d] = 1
                out.append(problem(np.array(([maj] * 5 + [far] * 2) * pad, np.uint8)))
    return out


def shorts():
    """Short sequences (d_of_row = -1) as representatives and as copies, beside members."""
    rng = np.random.default_rng(4)
    out = []
    for S, n in ((30, 12), (500, 12), (90, 40)):
        rows = random_rows(rng, S, n, 8, p_mut=0.3)
        rows[rng.random(S) < 0.3] = np.array([0, 1] + [4] * (n - 2), np.uint8)                 # copies of one short row
        rows[1] = np.array([2, 4, 3] + [4] * (n - 3), np.uint8)                                # a short row of its own
        out.append(problem(rows, min_len=5))
        assert (out[-1]["dor"] < 0).sum() >= 2
    return out


def small_random(count=150):
    """Many small problems over two symbols: ties and classes everywhere, the flag often decided by one of them."""
    rng = np.random.default_rng(5)
    out = []
    for _ in range(count):
        S, n = int(rng.integers(2, 14)), int(rng.integers(1, 9))
        p = problem(random_rows(rng, S, n, int(rng.integers(1, 6)), alphabet=(0, 1, 4), p_mut=0.4), min_len=int(rng.integers(0, 3)))
        if rng.random() < 0.5:                  # (any order of the distinct sequences: the tie-break reads it)
            perm = rng.permutation(max(p["D"], 1)).astype(np.int32)
            p["dor"] = np.where(p["dor"] >= 0, perm[np.maximum(p["dor"], 0)], -1).astype(np.int32)
        out.append(p)
    return out


def families():
    return dict(all_identical=all_identical(), no_identical=no_identical(), gapped_twins=gapped_twins(), ties=ties(), widths=widths(),
                thresholds=thresholds(), shorts=shorts(), small_random=small_random())
