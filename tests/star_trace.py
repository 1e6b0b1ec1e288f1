"""What star_align.star_msas asks of a backend, as a trace: a wrapper that forwards everything to any backend and records one line
per entry-point call, upload and download, the scenarios whose traces are pinned, and their digests (tests/golden/star_trace.json).
A host-side refactor of star_align / profile_align has to leave every line as it is: the same launches with the same arguments
and work, the same tables uploaded, the same downloads, in the same order.  The wrapper uses the backends' public methods only,
so this file runs unchanged on the commit a change is compared with:
    python tests/star_trace.py --write [--backend emu|runtime|torch] [--key KEY]    writes the golden file's KEY (default "digests")
    python tests/star_trace.py --check [--backend ...] [--key KEY]                  compares with it, exit status 1 on a difference
    python tests/star_trace.py --lines SCENARIO [--backend ...]                     prints the scenario's lines, to diff two commits
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
    return {"star": {}, "adjust_direction": dict(adjust_direction=True), "band": dict(band=True), "refine": dict(refine=2),
            "progressive": dict(progressive=True), "everything": everything,
            "everything_small_budget": dict(everything, budget_bytes=4 * pa.workspace_words(420, 420), chunk_bytes=1 << 14)}


def run(backend, name):
    """The scenario on the backend: (its lines, its digest entry)."""
    from make_prg_amd.from_msa import star_align as sa
    be = TraceBackend(backend)
    msas = sa.star_msas(be, loci(), **scenarios()[name])
    calls = {}
    for line in be.lines:
        if line.startswith("call "):
            calls[line.split()[1]] = calls.get(line.split()[1], 0) + 1
    return be.lines, dict(events=len(be.lines), calls=dict(sorted(calls.items())), sha256=hashlib.sha256("\n".join(be.lines).encode()).hexdigest(),
                          msa_md5=hashlib.md5("".join(sa.msa_fasta(m) for m in msas).encode()).hexdigest())


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
