"""Built-in aligner of `update --aligner builtin`: new sequences added to leaf alignments by a batched, integer, deterministic
profile alignment on the GPU (kernels: csrc/k_align.inc; C ABI: mprg_align_profiles / mprg_align_pairs in include/mprg.h).

It is NOT MAFFT.  Its alignments, and so the PRGs an update builds from them, can differ from what `--aligner mafft` (and the
reference) gives; byte-identity with the reference holds only for the MAFFT and replay paths.

Spec (the kernels and tests/align_ref.py follow it bit for bit)
  Inputs.   A leaf alignment A of R rows and C columns (codes ACGT-RYKMSWN, msa.py) and new sequences S_1..S_m, taken in
            sorted(new_sequences) order (the order the MAFFT wrapper writes them); a '-' in a new sequence is dropped.
  Pair score sigma.  Identical ACGT +20, different ACGT -9, any pair that involves R Y K M S W N 0, a residue against '-' -10.
  Profile, in 1/64 row, C's truncating division:
            residue x against column j:  P[j][x] = (64 * sum_r sigma(x, A[r][j])) / R
            gap in the new sequence at j: Dc[j] = (64 * -10 * r_j) / R, r_j = the rows of j that are not '-' (all-gap: 0)
            inserted residue (a new column): -640;  every maximal run of deletions or insertions pays -704 more to open.
  DP.       Global, three Gotoh states (H, D: column skipped, I: residue inserted), end gaps charged like any other gap,
            int32 accumulators; a pair with n + C >= 10^6 is refused (the scores could overflow).
  Ties.     Trace back from (n, C) in state H.  At an H cell take the diagonal if it gives H, else the deletion state if it
            equals H, else the insertion state.  In a gap state extend if extending gives the state's value, else open from H.
  Merge.    Every new sequence is aligned on its own against the profile of the original A.  Boundary j (0..C) gets
            max_k ins_k(j) new columns (ins_k(j): residues sequence k inserts there); each sequence's inserted residues are
            left-justified in them, every other row has '-' there.
  Output.   The original rows, then Denovo_path_{i}, with the ids and descriptions that load_alignment_file gives for the
            MAFFT wrapper's FASTA; letters upper case.

Band (opt-in: pairs_on_device(band=...), `from_msa --unaligned --band`; tests/band_ref.py states it in plain Python;
kernel: k_align_pairs_banded, C ABI: mprg_align_bounds / mprg_align_pairs_banded).  The same alignments from a fraction of the cells.
  Band.     The diagonal of cell (i, j) is d = j - i; a path starts on d = 0 and ends on Delta = C - n.  The band [dlo, dhi] keeps
            the cells with dlo <= d <= dhi in all three states; every cell outside it has the value minus infinity and is never
            computed.  Half-widths (w-, w+) give dlo = min(0, Delta) - w-, dhi = max(0, Delta) + w+ (clamped to [-n, C], the
            matrix).  Recurrence, scores, int32 arithmetic and tie order are the DP's above.  A gap state of an in-band cell whose
            two predecessors lie outside is minus infinity plus one penalty; the H of an in-band cell is always a real score (its
            diagonal predecessor lies on the same diagonal), so such a gap state is never chosen and nothing accumulates on it.
  Bounds.   Per leaf: B_j = max(max_x P[j][x], Dc[j]) (the most column j can contribute), SB = sum_j B_j, loss_j = B_j - Dc[j] >= 0
            (what deleting column j costs against B_j), m = min_j loss_j.  (Computed on the device, mprg_align_bounds: two int64
            per leaf come back instead of a profile.)
  Certificate.  An alignment scores  sum_matched P + sum_deleted Dc - 640 #inserted - 704 #gap runs.  A deletion moves a path one
            diagonal up, an insertion one down.  A path that touches a diagonal d* > max(0, Delta) has at least d* deleted columns
            (0 -> d*), at least d* - Delta > 0 inserted residues (d* -> Delta) and so at least one run of each; its columns
            contribute at most SB - sum_deleted loss_j <= SB - m d*.  So its score is at most
                UB+(d*) = SB - m d* - 640 (d* - Delta) - 1408,
            and a path that touches d* < min(0, Delta) has at least -d* insertions and Delta - d* > 0 deletions:
                UB-(d*) = SB - m (Delta - d*) - 640 (-d*) - 1408.
            (m d* is the issue's weaker form of "the d* smallest loss_j": no sort; for a 1-row ACGT leaf both are 1 920 d*.)
            Both fall strictly as d* moves away from the corridor.  Let S be the banded DP's score; a side is CLOSED when
            S > UB+(dhi + 1) (resp. S > UB-(dlo - 1)) or the band reaches the matrix's edge there (dhi = C, dlo = -n).  With both
            sides closed every optimal path of the full DP lies inside the band: S is the score of a real path, so optimum >= S,
            and a path that leaves the band touches dhi + 1 or dlo - 1 and scores <= UB < S.  Then every state on an optimal path
            has its full-DP value in the banded DP (induction along the path: all its predecessors' optimal sub-paths lie inside
            too), every other candidate has a value no larger than its full-DP value, so every forward tie decision and every
            traceback step on the path is the full DP's: ops and score are identical.
  Two passes, never a loop.  Pass 1 runs the pair with w- = w+ = w0 (BAND_W0; a tuning constant, not part of the result) and
            gives S0 <= optimum.  w*+ = the smallest w >= 0 with UB+(max(0, Delta) + w + 1) < S0, capped where the band reaches
            the edge: max(0, floor((SB - 1408 + 640 Delta - S0) / (m + 640)) - max(0, Delta)); w*- likewise:
            max(0, floor((SB - m Delta - 1408 - S0) / (m + 640)) + min(0, Delta)).  If w*- <= w0 and w*+ <= w0 pass 1 is certified.
            Otherwise the pair runs once more with (w*-, w*+): the pass-1 path scores S0 > UB beyond those widths, so it lies
            inside the new band, S >= S0, and both sides are closed by construction.  A pair whose band (of pass 1, or of pass 2)
            needs no less workspace than the full matrix, in total or in the traceback alone (W + 63 >= C with W = dhi - dlo + 1:
            the strips then sweep every column anyway), goes to the full DP instead (short pairs, unrelated sequences, sparse
            multi-row profiles whose m is small).  `update --aligner builtin` and the score-only DP of --adjust-direction keep
            the full form.

Free ends (opt-in: pairs_on_device(free_ends=True), `from_msa --unaligned --free-end-pairs`): the DP above as an overlap alignment,
with its own band certificate.  The spec and the proof: make_prg_amd/from_msa/star_align.py, "Free end pairs"; tests/freepairs_ref.py
states it in plain Python; kernels: k_align_pairs_endgap, k_align_pairs_endgap_banded, k_align_bounds_endgap (csrc/al_pairs.inc,
csrc/al_pairs_band.inc, csrc/k_align.inc).

Host side: leaves and sequences packed once, the profiles built for the whole batch in one launch, the pairs sorted by cell
count (longest first) and launched in chunks that fit a workspace budget (a pair whose traceback alone exceeds the budget is an
error), every pair's ops into one device buffer (pairs_on_device; from_msa --unaligned merges them there, csrc/k_star.inc);
the merge of `update` is NumPy over the downloaded ops.
"""
from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np

from ..msa import MSA, _fasta_title, encode

LEAF_FIELDS, PAIR_FIELDS = 4, 5          # MPRG_AL_LEAF_FIELDS, MPRG_AL_PAIR_FIELDS
MAX_LEN = 1_000_000                      # MPRG_AL_MAX_LEN
STATUS = {1: "n + C >= 10^6 (int32 scores could overflow)", 2: "workspace or ops range outside the buffers",
          3: "bad leaf (index, rows or columns)"}
DEFAULT_BUDGET_BYTES = 1 << 30           # traceback + row buffers of one launch
BAND_PAIR_FIELDS = 7                     # MPRG_AL_BAND_PAIR_FIELDS
BAND_W0 = 64                             # pass 1's half-width (what was tried)
_GAP = ord("-")


class ProfileAlignError(ValueError):
    pass


def exclusive_sum(x) -> np.ndarray:
    """0, x[0], x[0] + x[1], ...: where each of consecutive items of these sizes begins (int64, as long as x)."""
    x = np.asarray(x, np.int64)
    return np.cumsum(x) - x


def add_to(totals: Optional[dict], key: str, value):
    """totals[key] += value, from 0; nothing without a dict (the timings and counters a caller may ask for)."""
    if totals is not None:
        totals[key] = totals.get(key, 0) + value


def _ranges(start: np.ndarray, n: np.ndarray) -> np.ndarray:
    """start[0], start[0] + 1, ... (n[0] of them), start[1], ...: the concatenated ranges, without a Python loop."""
    n = np.asarray(n, np.int64)
    return np.repeat(np.asarray(start, np.int64) - (np.cumsum(n) - n), n) + np.arange(int(n.sum()), dtype=np.int64)


def _tile_work(widths: np.ndarray) -> np.ndarray:
    """{item, 256-column tile} for items of these widths."""
    tiles = -(-widths // 256)
    return np.stack([np.repeat(np.arange(len(widths)), tiles), _ranges(np.zeros(len(widths), np.int64), tiles)], 1).astype(np.int32)


def workspace_words(n, C):
    """int32 words of workspace a pair needs (include/mprg.h, mprg_align_pairs); plain integers or arrays."""
    return (2 * (C + 1) + 63) // 64 * 64 + (n + 63) // 64 * ((C + 70) // 8) * 64


workspace_words_v = workspace_words


def band_limits(n, C, w_minus, w_plus):
    """(dlo, dhi) of the band of half-widths (w-, w+), clamped to the matrix; scalars or arrays."""
    delta = C - n
    return np.maximum(np.minimum(0, delta) - w_minus, -n), np.minimum(np.maximum(0, delta) + w_plus, C)


def band_workspace_words(n, C, dlo, dhi):
    """int32 words of workspace a banded pair needs (include/mprg.h, mprg_align_pairs_banded); dlo, dhi clamped to [-n, C]."""
    W = dhi - dlo + 1
    return (2 * W + 63) // 64 * 64 + (n + 63) // 64 * ((np.minimum(C, W + 63) + 70) // 8) * 64


def band_helps(n, C, dlo, dhi):
    """The spec's rule for the full DP, negated: the band needs less workspace than the full matrix, in total and in its traceback."""
    return (band_workspace_words(n, C, dlo, dhi) < workspace_words_v(n, C)) & (dhi - dlo + 1 + 63 < C)


def band_cells(n, C, dlo, dhi):
    """The DP cells (i >= 1, j >= 1) inside the band: n C less the two corner triangles it cuts off; dlo, dhi clamped."""
    def tri(x):
        x = np.maximum(x, 0)
        return x * (x + 1) // 2
    below, above = n + dlo - 1, C - dhi - 1          # cells with j - i < dlo: sum_j max(0, n + dlo - j); with j - i > dhi likewise
    return n * C - (tri(below) - tri(below - C)) - (tri(above) - tri(above - n))


def sweep_work(n, C, dlo=None, dhi=None):
    """The cells the DP kernels sweep for items of n rows against C columns (whole 64-row strips; banded: over the strip's columns),
    summed: the `work=` of a launch."""
    return float(((n + 63) // 64 * 64 * (C if dlo is None else np.minimum(C, dhi - dlo + 64))).sum())


_ITEM = {"pair": "a pair of {} residues against {} columns", "merge": "a merge of {} columns against {}"}


def budget_launches(order, words, budget_bytes, error, noun, n, C, also=None):
    """The work items `order` (indices; words[k]: the int32 words of workspace item k needs), in that order, in launches whose
    workspace fits the budget: yields (the launch's items, each one's offset in the launch's workspace, the words used).  An item
    that alone exceeds the budget is refused before the first launch, as `error`, named as a `noun` ("pair", "merge") of n[k]
    against C[k].  It only packs: the caller uploads the table, launches and keeps the results per yielded launch.  also: a second need per item (int32 words) that has to fit the budget as well, save for a launch's first item."""
    budget_words = max(64, int(budget_bytes) // 4)
    if len(order) and words[order].max() > budget_words:
        # the item named: the lowest index among the largest, which is what pairs_on_device and _prog_groups named before they shared
        # this loop (they looked in index order); _prog_pairs looked in launch order, so between two merges of different shape that
        # tie for the largest need its message can now name the other one
        k = order[words[order] == words[order].max()].min()
        raise error(f"{_ITEM[noun].format(n[k], C[k])} needs {4 * words[k]} bytes of traceback, more than the workspace "
                    f"budget of {budget_bytes}")
    pos = 0
    while pos < len(order):
        end, used, used_also = pos, 0, 0
        while end < len(order) and used + words[order[end]] <= budget_words and (
                also is None or end == pos or used_also + also[order[end]] <= budget_words):
            used += int(words[order[end]])
            used_also += 0 if also is None else int(also[order[end]])
            end += 1
        sel = order[pos:end]
        yield sel, exclusive_sum(words[sel]), used
        pos = end


def budget_groups(need_bytes, budget_bytes):
    """(lo, hi) of consecutive groups of the items, in the order given, whose bytes fit the budget.  Not budget_launches: it never
    refuses (an item that alone exceeds the budget is a group of its own) and has no second need."""
    pos = 0
    while pos < len(need_bytes):
        end = pos + max(1, int(np.searchsorted(np.cumsum(need_bytes[pos:]), budget_bytes, side="right")))
        yield pos, end
        pos = end


def band_first(n, C, w0):
    """Pass 1's bands (dlo, dhi) of half-width w0 and, per item, whether the band helps (band_helps; no: the full DP)."""
    dlo, dhi = band_limits(n, C, w0, w0)
    return dlo, dhi, band_helps(n, C, dlo, dhi)


def band_plan(n, C, w0, pass1):
    """The spec's two passes over items of n rows against C columns (arrays).  pass1(first, dlo, dhi) runs pass 1 over the items
    `first` with the bands dlo, dhi (arrays over all items) and returns the certified half-widths (w-, w+) per item (read for
    `first` only); it works by side effect on its caller's state: it makes the pass-1 launches there and leaves their scores where the
    caller's later launches and downloads find them.  Returns (second, rest, dlo, dhi, counts): the items of pass 2 and of the full DP, each in launch order (most
    cells first), the final bands, and (items, second passes, items sent to the full DP, DP cells computed, n C summed)."""
    dlo, dhi, helps = band_first(n, C, w0)
    full = ~helps
    cells = band_cells(n, C, dlo, dhi)
    first = np.nonzero(~full)[0]
    first = first[np.argsort(-cells[first], kind="stable")]
    w_minus, w_plus = pass1(first, dlo, dhi)
    again = ~full & ((w_minus > w0) | (w_plus > w0))
    dlo2, dhi2 = band_limits(n, C, w_minus, w_plus)
    dlo, dhi = np.where(again, dlo2, dlo), np.where(again, dhi2, dhi)
    full |= again & ~band_helps(n, C, dlo, dhi)
    second = np.nonzero(again & ~full)[0]
    cells2 = band_cells(n, C, dlo, dhi)
    second = second[np.argsort(-cells2[second], kind="stable")]
    rest = np.nonzero(full)[0]
    rest = rest[np.argsort(-((n[rest] + 1) * C[rest]), kind="stable")]
    counts = (len(n), len(second), len(rest), cells[first].sum() + cells2[second].sum() + (n[rest] * C[rest]).sum(), (n * C).sum())
    return second, rest, dlo, dhi, counts


def certified_widths(n, C, SB, m, S0):
    """(w*-, w*+) of the spec's two-pass rule from pass 1's score S0: the smallest half-widths whose band is closed on each side."""
    delta, q = C - n, m + 640
    w_plus = np.maximum(0, (SB - 1408 + 640 * delta - S0) // q - np.maximum(0, delta))
    w_minus = np.maximum(0, (SB - m * delta - 1408 - S0) // q + np.minimum(0, delta))
    return np.minimum(w_minus, n + np.minimum(0, delta)), np.minimum(w_plus, C - np.maximum(0, delta))


def certified_widths_endgap(n, C, SB, m, z, S0):
    """(w*-, w*+) of the two-pass rule of "Free end pairs" (star_align.py) from pass 1's score S0 and mprg_align_bounds_endgap's
    {SB', m', z}: the smallest w >= 0 with U(w) = SB' - m' max(0, max(0, Delta) + w + 1 - z) < S0, the same on both sides, clamped
    as certified_widths clamps; with m' = 0 no band is certified below min(n, C)."""
    up = np.maximum(0, C - n)
    w = np.maximum(0, (SB - S0) // np.maximum(m, 1) + z - up)
    w = np.where(S0 > SB, 0, np.where(m > 0, w, np.minimum(n, C)))      # (S0 > SB': no path scores that; U(0) <= SB' < S0)
    return np.minimum(w, n + np.minimum(0, C - n)), np.minimum(w, C - up)


def _codes(seq: str, what: str) -> np.ndarray:
    raw = np.frombuffer(seq.upper().encode(), np.uint8)
    raw = raw[raw != _GAP]
    codes = encode(raw)
    if (codes == 255).any():
        raise ProfileAlignError(f"{what}: a character outside ACGT-RYKMSWN")
    return codes


def align_batch(backend, leaves: Sequence[np.ndarray], seqs: Sequence[Sequence[np.ndarray]],
                budget_bytes: int = DEFAULT_BUDGET_BYTES, band=None, counters: Optional[dict] = None,
                free_ends: bool = False) -> List[List[Tuple[bytes, int]]]:
    """leaves: R x C uint8 cell-code matrices; seqs[k]: the gap-free code arrays to align against leaf k.
    Returns, per leaf, per sequence, (ops as bytes over b"MID" in forward order, score).  band, counters, free_ends: as
    pairs_on_device."""
    out: List[List[Optional[Tuple[bytes, int]]]] = [[None] * len(s) for s in seqs]
    dp = pairs_on_device(backend, leaves, seqs, budget_bytes, band, counters, free_ends=free_ends)
    if dp is None:
        return out
    ops = backend.download(dp.d_ops, np.uint8, dp.ops_bytes)
    for p in range(len(dp.leaf)):
        o = int(dp.ops_off[p])
        out[dp.leaf[p]][dp.index[p]] = (ops[o:o + int(dp.count[p])][::-1].tobytes(), int(dp.score[p]))
    return out


class DevicePairs:
    """What pairs_on_device leaves: every pair's ops in one device buffer, as mprg_align_pairs wrote them (REVERSED, the last op
    first) at ops_off[p], count[p] of them; per pair (in leaf order, then sequence order) its leaf, index within the leaf and score."""

    def __init__(self, d_ops, ops_bytes, leaf, index, ops_off, count, score):
        self.d_ops, self.ops_bytes = d_ops, ops_bytes
        self.leaf, self.index, self.ops_off, self.count, self.score = leaf, index, ops_off, count, score


class PreparedProfiles:
    """Profiles the caller wrote on the device itself, for pairs_on_device(prepared=...): d_prof, the profile buffer as
    mprg_align_profiles lays it out (6 x C int32 per leaf); shapes, an (n_leaves, 2) array of {R, C}; prof_off, each leaf's offset
    in d_prof (int32 elements).  d_seqs / seq_off / seq_len: optionally the sequences already on the device, ONE per leaf: a buffer
    of cell codes and per leaf its sequence's offset there and its length (`seqs` is then not read)."""

    def __init__(self, d_prof, shapes, prof_off, d_seqs=None, seq_off=None, seq_len=None):
        self.d_prof, self.shapes, self.prof_off, self.d_seqs, self.seq_off, self.seq_len = d_prof, shapes, prof_off, d_seqs, seq_off, seq_len


def pairs_on_device(backend, leaves: Optional[Sequence[np.ndarray]], seqs: Sequence[Sequence[np.ndarray]],
                    budget_bytes: int = DEFAULT_BUDGET_BYTES, band=None, counters: Optional[dict] = None,
                    prepared: Optional[PreparedProfiles] = None, free_ends: bool = False) -> Optional[DevicePairs]:
    """The pairs of align_batch on the device: the profiles in one launch, the pairs longest first in launches that fit the
    workspace budget, every pair's ops into one buffer that stays on the device.  None when there is no pair.
    band: None: the full DP.  True or a half-width w0: the spec's Band, two passes: the same ops, counts and scores from the
    cells of a certified band (launches sized by the banded need; a pair the band does not help goes to the full DP).
    counters: a dict that then receives (added up) band_pairs, band_second_passes, band_full_pairs (pairs sent to the full DP),
    band_cells (DP cells computed, all passes and the full form) and band_full_cells (n C summed: what the full DP computes).
    prepared: the leaves' profiles are already on the device (PreparedProfiles; `leaves` is then not read and no profile launch is
    made): the leave-one-out profiles of from_msa --unaligned --refine.
    free_ends: the pairs as overlap alignments (star_align.py, "Free end pairs"): the _endgap form of the three entries and
    certified_widths_endgap; nothing else in the launches, the sizing or the counters changes.  False: the calls, uploads and
    downloads are what they are without it."""
    be = backend
    n_leaves = len(leaves) if prepared is None else len(prepared.shapes)
    if not n_leaves:
        return None
    shapes = (np.array([m.shape for m in leaves], np.int64) if prepared is None else np.asarray(prepared.shapes, np.int64)).reshape(-1, 2)
    if (shapes < 1).any():
        raise ProfileAlignError("a leaf alignment with no rows or no columns")
    R, C = shapes[:, 0], shapes[:, 1]
    prof_off = exclusive_sum(6 * C) if prepared is None else np.asarray(prepared.prof_off, np.int64)
    leaf_tab = np.stack([exclusive_sum(R * C), R, C, prof_off], 1).astype(np.int64)
    work = _tile_work(C)
    # pairs: (leaf, index within the leaf, n)
    on_device = prepared is not None and prepared.d_seqs is not None
    if on_device:
        pl, pi, pn = np.arange(n_leaves, dtype=np.int64), np.zeros(n_leaves, np.int64), np.asarray(prepared.seq_len, np.int64)
    else:
        pl = np.array([k for k, s in enumerate(seqs) for _ in s], np.int64)
        pi = np.array([i for s in seqs for i in range(len(s))], np.int64)
        pn = np.array([len(x) for s in seqs for x in s], np.int64)
    if not len(pl):
        return None
    pc = C[pl]
    too_long = np.nonzero(pn + pc >= MAX_LEN)[0]
    if len(too_long):
        k = too_long[0]
        raise ProfileAlignError(f"a pair of {pn[k]} residues against {pc[k]} columns: n + C must stay below {MAX_LEN}")
    seq_off = np.asarray(prepared.seq_off, np.int64) if on_device else exclusive_sum(pn)
    need = workspace_words_v(pn, pc)

    def packed(order, words):
        return budget_launches(order, words, budget_bytes, ProfileAlignError, "pair", pn, pc)
    if band is None:
        full_plan = list(packed(np.argsort(-((pn + 1) * pc), kind="stable"), need))       # longest first; refuses before anything is uploaded
    ops_len = pn + pc
    ops_off = exclusive_sum(ops_len)
    ops_bytes = max(int(ops_len.sum()), 1)
    count = np.zeros(len(pl), np.int64)
    score = np.zeros(len(pl), np.int64)
    if prepared is None:
        d_cells = be.upload(np.concatenate([m.reshape(-1) for m in leaves]).astype(np.uint8))
        d_leaves = be.upload(leaf_tab)
        d_work = be.upload(work)
        d_prof = be.empty(4 * int((6 * C).sum()))
        be.call("mprg_align_profiles", be.ptr(d_cells), be.ptr(d_leaves), be.ptr(d_work), len(work), be.ptr(d_prof), be.stream,
                work=float((R * C).sum()))
    else:
        d_leaves, d_prof = be.upload(leaf_tab), prepared.d_prof
    d_seqs = prepared.d_seqs if on_device else be.upload(np.concatenate([x for s in seqs for x in s] + [np.zeros(1, np.uint8)]).astype(np.uint8))
    d_ops = be.empty(ops_bytes)

    def launches(call, plan, dlo=None, dhi=None):
        """The launches of `plan` (packed) through `call`."""
        for idx, ws_off, used in plan:
            band_cols = () if dlo is None else (dlo[idx], dhi[idx])
            d_pairs = be.upload(np.stack([pl[idx], seq_off[idx], pn[idx], ws_off, ops_off[idx], *band_cols], 1).astype(np.int64))
            d_ws = be.empty(4 * used)
            d_out = be.empty(12 * len(idx))
            be.call(call, be.ptr(d_prof), be.ptr(d_leaves), n_leaves, be.ptr(d_seqs), be.ptr(d_pairs), len(idx),
                    be.ptr(d_ws), used, be.ptr(d_ops), ops_bytes, be.ptr(d_out), be.stream,
                    work=sweep_work(pn[idx], pc[idx], *band_cols))
            res = be.download(d_out, np.int32, 3 * len(idx)).reshape(-1, 3)
            bad = np.nonzero(res[:, 0])[0]
            if len(bad):
                raise ProfileAlignError(f"{call}: {STATUS.get(int(res[bad[0], 0]), int(res[bad[0], 0]))}")
            score[idx] = res[:, 1]
            count[idx] = res[:, 2]
    full_call, band_call = ("mprg_align_pairs_endgap", "mprg_align_pairs_endgap_banded") if free_ends else ("mprg_align_pairs", "mprg_align_pairs_banded")
    if band is None:
        launches(full_call, full_plan)
        return DevicePairs(d_ops, ops_bytes, pl, pi, ops_off, count, score)
    # the spec's Band: pass 1 with w0, the certificate over the downloaded scores, pass 2 with the certified widths; the full DP
    # for the pairs whose band needs no less workspace than the full matrix
    w0 = BAND_W0 if band is True else int(band)
    if w0 < 0:
        raise ProfileAlignError("band: a negative half-width")
    n_bounds = 3 if free_ends else 2
    d_bounds = be.empty(8 * n_bounds * n_leaves)
    be.call("mprg_align_bounds_endgap" if free_ends else "mprg_align_bounds", be.ptr(d_prof), be.ptr(d_leaves), n_leaves, be.ptr(d_bounds),
            be.stream, work=float((6 * C).sum()))
    bounds = be.download(d_bounds, np.int64, n_bounds * n_leaves).reshape(-1, n_bounds)[pl]

    def pass1(first, dlo, dhi):
        launches(band_call, packed(first, band_workspace_words(pn, pc, dlo, dhi)), dlo, dhi)
        return (certified_widths_endgap if free_ends else certified_widths)(pn, pc, *bounds.T, score)
    second, rest, dlo, dhi, counts = band_plan(pn, pc, w0, pass1)
    launches(band_call, packed(second, band_workspace_words(pn, pc, dlo, dhi)), dlo, dhi)
    launches(full_call, packed(rest, need))
    for key, v in zip(("band_pairs", "band_second_passes", "band_full_pairs", "band_cells", "band_full_cells"), counts):
        add_to(counters, key, int(v))
    return DevicePairs(d_ops, ops_bytes, pl, pi, ops_off, count, score)


def merge(rows: np.ndarray, seqs: Sequence[np.ndarray], ops_list: Sequence[bytes]) -> np.ndarray:
    """The updated R + m rows (ASCII) of one leaf: rows as R x C ASCII, seqs as gap-free cell codes, their ops."""
    R, C = rows.shape
    m = len(seqs)
    ins = np.zeros((m, C + 1), np.int64)
    opa = [np.frombuffer(o, np.uint8) for o in ops_list]
    for k, o in enumerate(opa):
        is_i = o == ord("I")
        col = np.cumsum(~is_i) - (~is_i)            # the boundary an op sits at: columns consumed before it
        np.add.at(ins[k], col[is_i], 1)
    width = ins.max(0) if m else np.zeros(C + 1, np.int64)
    start = exclusive_sum(width + 1)          # output column where boundary j's insertions begin
    W = int(width.sum()) + C
    out = np.full((R + m, W), _GAP, np.uint8)
    out[:R, start[:C] + width[:C]] = rows
    alphabet = np.frombuffer(b"ACGT-RYKMSWN", np.uint8)
    for k, o in enumerate(opa):
        is_i = o == ord("I")
        consumes_col = ~is_i
        col = np.cumsum(consumes_col) - consumes_col              # boundary / column index of each op
        is_res = o != ord("D")
        res = alphabet[seqs[k]]
        # rank of an inserted residue within its boundary's run
        run_start = np.zeros(len(o), np.int64)
        if len(o):
            new_run = np.concatenate([[True], col[1:] != col[:-1]]) | consumes_col
            first = np.maximum.accumulate(np.where(new_run, np.arange(len(o)), 0))
            run_start = np.arange(len(o)) - first
        dest = np.where(is_i, start[col] + run_start, start[np.minimum(col, C)] + width[np.minimum(col, C)])
        sel = is_res
        out[R + k, dest[sel]] = res
    return out


def updated_alignments(backend, items: Iterable[Tuple[MSA, Iterable[str]]],
                       budget_bytes: int = DEFAULT_BUDGET_BYTES) -> List[MSA]:
    """[(current alignment, new sequences), ...] -> the alignments with the new sequences added, one batch on the device."""
    items = list(items)
    leaves, leaf_rows, seqs = [], [], []
    for aln, new_sequences in items:
        data = np.ascontiguousarray(aln.data)
        lower = (data >= ord("a")) & (data <= ord("z"))
        upper = np.where(lower, data - 32, data).astype(np.uint8)
        codes = encode(upper)
        if (codes == 255).any():
            raise ProfileAlignError("leaf alignment: a character outside ACGT-RYKMSWN")
        leaves.append(codes)
        leaf_rows.append(upper)
        ordered = sorted(new_sequences)
        seqs.append([_codes(s, f"new sequence {i}") for i, s in enumerate(ordered)])
    res = align_batch(backend, leaves, seqs, budget_bytes)
    out = []
    for (aln, _), rows, sq, r in zip(items, leaf_rows, seqs, res):
        data = merge(rows, sq, [ops for ops, _ in r])
        titles = [_fasta_title(i, d).rstrip() for i, d in zip(aln.ids, aln.descriptions)]
        titles += [f"Denovo_path_{i}" for i in range(len(sq))]
        ids = [(t.split(None, 1) or [""])[0] for t in titles]
        out.append(MSA(_data=data, _ids=ids, _descs=titles))
    return out
