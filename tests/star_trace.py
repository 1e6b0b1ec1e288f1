"""What star_align.star_msas asks of a backend, as a trace: a wrapper that forwards everything to any backend and records one line
per entry-point call, upload and download, the scenarios whose traces are pinned, and their digests (tests/golden/star_trace.json).
A host-side refactor of star_align / profile_align has to leave every line as it is: the same launches with the same arguments
and work, the same tables uploaded, the same downloads, in the same order.  The wrapper uses the backends' public methods only,
so this file runs unchanged on the commit a change is compared with:
    python tests/star_trace.py --write [--backend emu|runtime|torch] [--key KEY]    writes the golden file's KEY (default "digests")
    python tests/star_trace.py --check [--backend ...] [--key KEY]                  compares with it, exit status 1 on a difference
    python tests/star_trace.py --lines SCENARIO [--backend ...]                     prints the scenario's lines, to diff two commits
    python tests/star_trace.py --reports SCENARIO [--backend ...]                   prints what its `reports` digests, likewise
An entry's `reports` digests what the launch trace cannot see: the six per-locus lists star_msas fills for its caller and the counters.
The golden file is generated at the PARENT of a refactoring commit, never from the refactored code."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "star_trace.json")
PTR = 1 << 40                              # an integer this large is an address: it differs from run to run


class TraceBackend:
    """Forwards every attribute to `inner`; call, upload and download also append a line to `lines`."""

    def __init__(self, inner):
        self.inner, self.lines = inner, []

    def __getattr__(self, name):
        return getattr(self.inner, name)

    def call(self, name, *args, work=0.0, **kw):
        # (every entry point's last argument is the stream: a backend's own handle, not part of what the host asked for)
        shown = ["ptr" if not isinstance(a, (int, np.integer)) or abs(int(a)) >= PTR else str(int(a)) for a in args[:-1]]
        self.lines.append(f"call {name} {' '.join(shown)} stream work={float(work)!r}")
        return self.inner.call(name, *args, work=work, **kw)

    def upload(self, arr):
        a = np.ascontiguousarray(arr)
        if a.dtype == np.int64:                                 # (a table of device addresses: star_align._bufs_table)
            a = np.where(np.abs(a) >= PTR, -1, a)
        self.lines.append(f"upload {a.nbytes} {hashlib.sha256(a.tobytes()).hexdigest()}")
        return self.inner.upload(arr)

    def download(self, buf, dtype, count):
        self.lines.append(f"download {np.dtype(dtype).name} {int(count)}")
        return self.inner.download(buf, dtype, count)


def loci():
    from tests import prog_ref, refine_ref, star_ref, strand_ref
    every = star_ref.edge_loci() + star_ref.random_loci(3, 8) + refine_ref.special_loci() + prog_ref.table_loci() + strand_ref.strand_edge_loci()
    return [[(f"s{i} d", s) for i, s in enumerate(l)] for l in every if any(star_ref.normalise(s) for s in l)]


def scenarios():
    from make_prg_amd.update import profile_align as pa
    everything = dict(progressive=True, band=8, refine=2, adjust_direction=True)
    # the options of --progressive, with caps low enough that over loci() every path is taken (the counters of each are non-zero)
    prog = {"collapse": dict(collapse=True), "device_tree": dict(device_tree=True), "max_leaves": dict(max_leaves=4),
            "large_loci": dict(collapse=True, large_loci=True, max_leaves=4, max_records=8, device_tree=True),
            "retree": dict(retree=2), "refine_tree": dict(refine_tree=2, tree_refine_max_leaves=6), "seq_weights": dict(seq_weights=True),
            "seq_weights_device": dict(seq_weights=True, device_tree=True, retree=1, refine_tree=1),
            "pair_distances": dict(pair_distances=True, pair_dist_max_leaves=6, band=8), "position_gaps": dict(position_gaps=True),
            "free_end_gaps": dict(free_end_gaps=True, position_gaps=True, band=8),
            "all_progressive": dict(adjust_direction=True, band=8, refine=1, collapse=True, device_tree=True, large_loci=True, max_leaves=6,
                                    max_records=12, retree=1, refine_tree=1, tree_refine_max_leaves=6, seq_weights=True, pair_distances=True,
                                    pair_dist_max_leaves=5, position_gaps=True, free_end_gaps=True, chunk_bytes=1 << 14)}
    return {"star": {}, "adjust_direction": dict(adjust_direction=True), "band": dict(band=True), "refine": dict(refine=2),
            "progressive": dict(progressive=True), "everything": everything,
            "everything_small_budget": dict(everything, budget_bytes=4 * pa.workspace_words(420, 420), chunk_bytes=1 << 14),
            "collapse_star": dict(collapse=True), **{name: dict(kw, progressive=True) for name, kw in prog.items()}}


REPORTS = ("orientation", "refinement", "progression", "tree_refinement", "retreeing", "pair_distancing")


def _plain(x):
    """x as JSON takes it: tuples as lists, NumPy scalars as Python's."""
    if isinstance(x, (list, tuple)):
        return [_plain(v) for v in x]
    return x.item() if isinstance(x, np.generic) else x


def run(backend, name, reports=None):
    """The scenario on the backend: (its lines, its digest entry).  reports: a dict that receives what the entry's `reports` digests:
    the caller's six per-locus lists and every counter of timings that is no wall time (its key does not end in _s)."""
    from make_prg_amd.from_msa import star_align as sa
    be = TraceBackend(backend)
    timings, lists = {}, {key: [] for key in REPORTS}
    msas = sa.star_msas(be, loci(), timings=timings, **lists, **scenarios()[name])
    calls = {}
    for line in be.lines:
        if line.startswith("call "):
            calls[line.split()[1]] = calls.get(line.split()[1], 0) + 1
    seen = _plain(dict(lists, counters={k: v for k, v in timings.items() if not k.endswith("_s")}))
    if reports is not None:
        reports.update(seen)
    return be.lines, dict(events=len(be.lines), calls=dict(sorted(calls.items())), sha256=hashlib.sha256("\n".join(be.lines).encode()).hexdigest(),
                          msa_md5=hashlib.md5("".join(sa.msa_fasta(m) for m in msas).encode()).hexdigest(),
                          reports=hashlib.sha256(json.dumps(seen, sort_keys=True, separators=(",", ":")).encode()).hexdigest())


def golden(key="digests"):
    with open(GOLDEN) as fh:
        return json.load(fh)[key]


def _backend(kind):
    if kind == "emu":
        from tests.emu.backend import EmuBackend
        return EmuBackend()
    import torch  # noqa: F401  (before the library: HipBackend needs torch's HIP runtime to be the one the library binds)
    from make_prg_amd import backend as b
    return b.HipRuntimeBackend(0) if kind == "runtime" else b.HipBackend(0)


def main(argv):
    def opt(flag, default):
        return argv[argv.index(flag) + 1] if flag in argv else default
    be, key = _backend(opt("--backend", "emu")), opt("--key", "digests")
    if "--lines" in argv:
        print("\n".join(run(be, opt("--lines", None))[0]))
        return 0
    if "--reports" in argv:
        seen = {}
        run(be, opt("--reports", None), seen)
        print(json.dumps(seen, indent=1, sort_keys=True))
        return 0
    got = {name: run(be, name)[1] for name in scenarios()}
    if "--write" in argv:
        data = {}
        if os.path.exists(GOLDEN):
            with open(GOLDEN) as fh:
                data = json.load(fh)
        data[key] = got
        with open(GOLDEN, "w") as fh:
            json.dump(data, fh, indent=1, sort_keys=True)
            fh.write("\n")
        return 0
    want = golden(key)
    for name in got:
        print(name, "equal" if got[name] == want[name] else f"DIFFERS: {got[name]} != {want[name]}")
    return int(got != want)


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
