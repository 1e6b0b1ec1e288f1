"""GPU-box helper: the built-in profile aligner (update --aligner builtin) on a synthetic leaf-shaped batch (tests/align_ref.py,
synth_leaf_batch: R 2-200, C 20-3 000).  Prints one JSON line: the DP cells (sum of n x C over the pairs, from the shapes), the
wall time of align_batch (profiles + fill + walk + downloads, after a warm-up run) and of the whole aligner stage of an update
(BuiltinAligner.get_updated_alignments: packing, launches, merge, MSAs) for the same leaves.  Kernel time: run it under
`rocprofv3 --kernel-trace --stats -- python tools/align_measure.py` and divide the cells by k_align_pairs' total."""
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
print(json.dumps(dict(pairs=sum(len(s) for s in seqs), leaves=len(leaves), cells=cells, align_batch_s=round(t_batch, 3),
                      gcups_wall=round(cells / t_batch / 1e9, 1), aligner_stage_s=round(t_stage, 3))))
