"""Container-only: KMeans fits across the whole range of the LDS form of the fit (k_kmeans_fit_lds, every class 0..5) with
scikit-learn's answers, cross-checked against the oracle's C restatement (oracle/kmeans_oracle.c); any disagreement aborts.
Writes tests/golden/kmeans_lds_edges.json.gz (records of kmeans.json.gz's layout plus n_init).

    python -m oracle.tools.gen_kmeans_edges

The pinned configuration is set here, before NumPy is imported: OpenBLAS's Haswell kernels, one thread, and NumPy's SIMD sort
dispatch disabled (the relocation's np.argpartition is then NumPy's generic arg-introselect, the one the reference's locked
NumPy 1.24 runs and the oracle restates; NumPy 2.x's x86-simd-sort breaks ties differently).
Shapes: D in {3, 4, 8, 9, 63, 64} (k < D), V in {1..5, 127..129, 255, 256, 511, 1023, 1024}, k = 2..10, n_init in {1, 2, 3, 7, 10};
at least FITS_PER_CLASS fits of every LDS class at n_init = 10; three kinds of matrix (clustered, noise 0..2, few distinct rows)
and a few with counts above 255.
"""
import os
import sys

os.environ["OPENBLAS_CORETYPE"] = "Haswell"
os.environ["OMP_NUM_THREADS"] = "1"
os.environ["NPY_DISABLE_CPU_FEATURES"] = "AVX512F AVX512CD AVX512_SKX AVX512_CLX AVX512_CNL AVX512_ICL AVX512_SPR AVX2"
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import gzip
import io
import json
import platform
import warnings

import numpy as np
import scipy
import sklearn
import sklearn.cluster._kmeans as skm
import threadpoolctl
from sklearn.cluster import KMeans

import oracle.from_msa_oracle as orc

OUT = os.path.join(ROOT, "tests", "golden", "kmeans_lds_edges.json.gz")
DS = (3, 4, 8, 9, 63, 64)
VS = (1, 2, 3, 4, 5, 127, 128, 129, 255, 256, 511, 1023, 1024)
N_INITS = (1, 2, 3, 7)                  # (beside 10)
FITS_PER_CLASS = 24                     # n_init = 10, every LDS class
FITS_PER_N_INIT = 20                    # every other n_init
KINDS = ("clustered", "noise", "few-distinct")

_pp = []
_orig_pp = skm._kmeans_plusplus


def _pp_hook(*a, **k):
    c, i = _orig_pp(*a, **k)
    _pp.append([int(x) for x in i])
    return c, i


skm._kmeans_plusplus = _pp_hook


def lds_class(D, V, k, n_init):
    """kml_class of make_prg_amd/csrc/k_kmeans_lds.inc, asked through the library the tests use (the CPU emulation build)."""
    import ctypes
    from make_prg_amd.backend import bind
    from tests.emu.backend import build_emu
    global _LIB
    if "_LIB" not in globals():
        _LIB = bind(ctypes.CDLL(build_emu()))
    return int(_LIB.mprg_kmeans_lds_class(D, V, k, n_init))


def matrix(rng, D, V, kind, big):
    top = 400 if big else 6
    if kind == "clustered":
        centres = rng.integers(0, top, (int(rng.integers(2, 6)), V))
        M = centres[rng.integers(0, len(centres), D)] + rng.integers(0, 2, (D, V))
    elif kind == "noise":
        M = rng.integers(0, 3, (D, V)) + (rng.integers(250, 300, (D, V)) if big else 0)
    else:                               # few distinct rows: k beyond them empties clusters (the relocation)
        base = rng.integers(0, top, (int(rng.integers(2, 4)), V))
        M = base[rng.integers(0, len(base), D)]
    return M.astype(np.float64)


def fit_record(M, k, n_init):
    D, V = M.shape
    _pp.clear()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        km = KMeans(n_clusters=k, random_state=2, algorithm="elkan", n_init=n_init).fit(M)
        labels = km.predict(M)
    rec = dict(shape=[D, V], counts_i16_hex=M.astype("<i2").tobytes().hex(), k=k, n_init=n_init, labels=[int(v) for v in labels],
               fit_labels=[int(v) for v in km.labels_], pp=str(_pp), inertia=float(km.inertia_).hex(), n_iter=int(km.n_iter_))
    o_lab, dbg = orc.kmeans_fit_predict(M, k, n_init=n_init, want_debug=True)
    got = (o_lab.tolist(), dbg["fit_labels"].tolist(), str(dbg["pp"].tolist()), float(dbg["inertia"]).hex(), dbg["n_iter"])
    want = (rec["labels"], rec["fit_labels"], rec["pp"], rec["inertia"], rec["n_iter"])
    if got != want:
        raise SystemExit(f"oracle != scikit-learn at D={D} V={V} k={k} n_init={n_init}: {got[3:]} vs {want[3:]}")
    return rec


def plan():
    """(D, V, k, n_init) of every fit: FITS_PER_CLASS per LDS class at n_init = 10 (k = 10 and the largest shapes first), then
    FITS_PER_N_INIT per other n_init, drawn without repeats."""
    rng = np.random.default_rng(2024)
    shapes = [(D, V, k) for D in DS for V in VS for k in range(2, min(D - 1, 10) + 1)]
    out = []
    by_class = {}
    for D, V, k in shapes:
        by_class.setdefault(lds_class(D, V, k, 10), []).append((D, V, k))
    for c in range(6):
        cand = by_class[c]
        pick = [cand[i] for i in rng.permutation(len(cand))]
        must = [s for s in cand if s[2] == 10][:2] + [s for s in cand if s[1] in (1023, 1024)][:2]
        chosen = list(dict.fromkeys(must + pick))[:FITS_PER_CLASS]
        out += [(D, V, k, 10) for D, V, k in chosen]
    out += [(D, V, k, 10) for D, V, k in by_class.get(-1, [])[:4]]        # beyond the LDS form: the lds path's other forms
    for n_init in N_INITS:
        for i in rng.permutation(len(shapes))[:FITS_PER_N_INIT]:
            out.append(shapes[i] + (n_init,))
    return out


def main():
    rng = np.random.default_rng(7)
    fits = []
    for i, (D, V, k, n_init) in enumerate(plan()):
        kind = KINDS[i % 3]
        big = i % 17 == 5                # counts above 255 (beyond the byte form of the counts in LDS)
        fits.append(fit_record(matrix(rng, D, V, kind, big), k, n_init))
    meta = dict(sklearn=sklearn.__version__, numpy=np.__version__, scipy=scipy.__version__, n_init=sorted({f["n_init"] for f in fits}),
                OMP_NUM_THREADS=os.environ["OMP_NUM_THREADS"], OPENBLAS_CORETYPE=os.environ["OPENBLAS_CORETYPE"],
                NPY_DISABLE_CPU_FEATURES=os.environ["NPY_DISABLE_CPU_FEATURES"],
                blas=[{k: d.get(k) for k in ("internal_api", "version", "architecture", "prefix")} for d in threadpoolctl.threadpool_info()],
                python=platform.python_version())
    raw = json.dumps(dict(fits=fits, meta=meta), sort_keys=True, separators=(",", ":")).encode()
    buf = io.BytesIO()
    with gzip.GzipFile(fileobj=buf, mode="wb", mtime=0, compresslevel=9) as gz:
        gz.write(raw)
    with open(OUT, "wb") as fh:
        fh.write(buf.getvalue())
    print(f"{len(fits)} fits, {len(buf.getvalue())} bytes -> {OUT}")


if __name__ == "__main__":
    main()
