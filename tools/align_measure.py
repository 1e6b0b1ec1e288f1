"""GPU-box helper: the built-in profile aligner (update --aligner builtin) on a synthetic leaf-shaped batch (tests/align_ref.py,
synth_leaf_batch: R 2-200, C 20-3 000).  Prints one JSON line: the DP cells (sum of n x C over the pairs, from the shapes), the
wall time of align_batch (profiles + fill + walk + downloads, after a warm-up run) and of the whole aligner stage of an update
(BuiltinAligner.get_updated_alignments: packing, launches, merge, MSAs) for the same leaves.  Kernel time: run it under
`rocprofv3 --kernel-trace --stats -- python tools/align_measure.py` and divide the cells by k_align_pairs' total.
A second leg runs the same pairs, on the same profiles, through mprg_align_pair_scores (the score-only sweep of `from_msa --unaligned
--progressive --pair-distances`) and through mprg_align_pairs, each longest first in launches that fit the workspace budget, each
between two synchronisations after a warm-up pass: scores_ms / scores_gcups against pairs_ms / pairs_gcups (uploads of the pair
tables and the allocations included), the launches each needed, and scores_equal: both gave the same score for every pair."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from make_prg_amd.backend import make_backend  # noqa: E402
from make_prg_amd.msa import MSA  # noqa: E402
from make_prg_amd.update import profile_align as pa  # noqa: E402
from tests.align_ref import synth_leaf_batch  # noqa: E402

n_pairs = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000
be = make_backend(None, 0)
leaves, seqs = synth_leaf_batch(1, n_pairs)
cells = int(sum(m.shape[1] * len(s) for m, ss in zip(leaves, seqs) for s in ss))
pa.align_batch(be, leaves[:50], seqs[:50])                        # warm-up: first launches
t0 = time.perf_counter()
pa.align_batch(be, leaves, seqs)
t_batch = time.perf_counter() - t0
ascii_ = np.frombuffer(b"ACGT-RYKMSWN", np.uint8)
reqs = [(MSA(_data=ascii_[m], _ids=[f"r{i}" for i in range(len(m))], _descs=[f"r{i}" for i in range(len(m))]),
         {ascii_[s].tobytes().decode() for s in ss}) for m, ss in zip(leaves, seqs)]
t0 = time.perf_counter()
pa.updated_alignments(be, reqs)
t_stage = time.perf_counter() - t0


def sweep_leg(call, fields, words, result_words):
    """The batch's pairs through `call` (longest first, workspace-budget launches): (wall ms, launches, the scores)."""
    score = np.zeros(len(pl), np.int64)
    outs = []
    be.synchronize()
    t0 = time.perf_counter()
    for idx, ws_off, used in pa.budget_launches(order, words, pa.DEFAULT_BUDGET_BYTES, pa.ProfileAlignError, "pair", pn, pc):
        d_pairs = be.upload(np.stack([pl[idx], seq_off[idx], pn[idx], ws_off, fields[idx]], 1).astype(np.int64))
        d_ws, d_out = be.empty(4 * used), be.empty(4 * result_words * len(idx))
        be.call(call, be.ptr(d_prof), be.ptr(d_leaves), len(leaves), be.ptr(d_seqs), be.ptr(d_pairs), len(idx), be.ptr(d_ws), used,
                be.ptr(d_second), second_size, be.ptr(d_out), be.stream, work=pa.sweep_work(pn[idx], pc[idx]))
        outs.append((idx, d_out))
    be.synchronize()
    ms = 1e3 * (time.perf_counter() - t0)
    for idx, d_out in outs:
        res = be.download(d_out, np.int32, result_words * len(idx)).reshape(-1, result_words)
        assert not res[:, 0].any(), (call, res[res[:, 0] != 0][:3])
        score[idx] = res[:, 1]
    return ms, len(outs), score


shapes = np.array([m.shape for m in leaves], np.int64)
R, C = shapes[:, 0], shapes[:, 1]
d_leaves = be.upload(np.stack([pa.exclusive_sum(R * C), R, C, pa.exclusive_sum(6 * C)], 1).astype(np.int64))
tiles = pa._tile_work(C)
d_cells, d_work, d_prof = be.upload(np.concatenate([m.reshape(-1) for m in leaves]).astype(np.uint8)), be.upload(tiles), be.empty(4 * int((6 * C).sum()))
be.call("mprg_align_profiles", be.ptr(d_cells), be.ptr(d_leaves), be.ptr(d_work), len(tiles), be.ptr(d_prof), be.stream, work=float((R * C).sum()))
pl = np.array([k for k, ss in enumerate(seqs) for _ in ss], np.int64)
pn = np.array([len(x) for ss in seqs for x in ss], np.int64)
pc = C[pl]
seq_off = pa.exclusive_sum(pn)
d_seqs = be.upload(np.concatenate([x for ss in seqs for x in ss] + [np.zeros(1, np.uint8)]).astype(np.uint8))
order = np.argsort(-((pn + 1) * pc), kind="stable")
legs = {}
for name, call, fields, words, result_words, second in (
        ("scores", "mprg_align_pair_scores", np.arange(len(pl), dtype=np.int64), (2 * (pc + 1) + 63) // 64 * 64, 2, 4 * len(pl)),
        ("pairs", "mprg_align_pairs", pa.exclusive_sum(pn + pc), pa.workspace_words_v(pn, pc), 3, int((pn + pc).sum()))):
    d_second, second_size = be.empty(second), (len(pl) if name == "scores" else second)     # the table of s'', or the ops
    sweep_leg(call, fields, words, result_words)                   # warm-up: first launches, the allocator's first blocks
    legs[name] = sweep_leg(call, fields, words, result_words)
print(json.dumps(dict(pairs=sum(len(s) for s in seqs), leaves=len(leaves), cells=cells, align_batch_s=round(t_batch, 3),
                      gcups_wall=round(cells / t_batch / 1e9, 1), aligner_stage_s=round(t_stage, 3),
                      **{f"{k}_ms": round(v[0], 2) for k, v in legs.items()}, **{f"{k}_gcups": round(cells / v[0] / 1e6, 1) for k, v in legs.items()},
                      **{f"{k}_launches": v[1] for k, v in legs.items()}, scores_equal=bool((legs["scores"][2] == legs["pairs"][2]).all()))))
