"""KMeans fits across the whole range of the LDS form of the fit (k_kmeans_fit_lds: D 2..64, V 1..1 024, k 2..10, n_init 1..10, every
dynamic-LDS class 0..5) with scikit-learn's answers (tests/golden/kmeans_lds_edges.json.gz, oracle/tools/gen_kmeans_edges.py): the
oracle and the emulation build of every fit form against them; the routing of fits into the LDS form's launch lists and the fit body's
guard against fits it does not hold.  The GPU twins are in tests/test_gpu_edges.py."""
import gzip
import json
import os

import numpy as np
import pytest

import oracle.from_msa_oracle as orc
from tests.emu.backend import EmuBackend
from tests.kmeans_direct import run_kmeans_fits

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kmeans_lds_edges.json.gz")
EDGE_VS = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 511, 512, 1023, 1024, 1025)
MPRG_KM_UNSUPPORTED = 2
# synthetic config-C alignments (make_prg_amd.utils.synthetic.synth_config_fasta) whose oracle run holds fits of LDS class 4
# (73.5 KB) and class 5 (128 KB) — the classes beyond 64 KB of LDS per workgroup — from a scan of seeds 0..999
CLASS45_SEEDS = (2, 5, 8, 13, 16, 183, 246, 721, 863, 931)          # (every seed of the scan with a class-5 fit, and five with class 4)


def load_fits():
    with gzip.open(GOLDEN, "rt") as fh:
        return json.load(fh)


def matrix(f):
    D, V = f["shape"]
    return np.frombuffer(bytes.fromhex(f["counts_i16_hex"]), dtype="<i2").reshape(D, V).astype(np.float64)


def check_fits(backend, fits, path, n_slots=3):
    """Every fit through one form (kmeans_direct.run_kmeans_fits takes one n_init per call): labels, inertia bits, iterations."""
    by_n = {}
    for f in fits:
        by_n.setdefault(f["n_init"], []).append(f)
    n = 0
    for n_init, group in sorted(by_n.items()):
        got = run_kmeans_fits(backend, group, n_init=n_init, path=path, n_slots=n_slots)
        for g, f in zip(got, group):
            tag = (path, f["shape"], f["k"], n_init)
            assert not g["status"] & MPRG_KM_UNSUPPORTED, tag
            assert g["labels"] == f["labels"], tag
            assert g["inertia_hex"] == f["inertia"], tag
            assert g["n_iter"] == f["n_iter"], tag
            n += 1
    return n


@pytest.fixture(scope="module")
def edges():
    return load_fits()


@pytest.fixture(scope="module")
def emu():
    return EmuBackend()


def test_meta_records_pinned_configuration(edges):
    m = edges["meta"]
    assert m["OMP_NUM_THREADS"] == "1" and m["OPENBLAS_CORETYPE"] == "Haswell"
    assert "AVX2" in m["NPY_DISABLE_CPU_FEATURES"].split() and "AVX512_SKX" in m["NPY_DISABLE_CPU_FEATURES"].split()
    assert m["n_init"] == [1, 2, 3, 7, 10]


def test_oracle_equals_scikit_learn(edges):
    for f in edges["fits"]:
        labels, dbg = orc.kmeans_fit_predict(matrix(f), f["k"], n_init=f["n_init"], want_debug=True)
        assert labels.tolist() == f["labels"]
        assert dbg["fit_labels"].tolist() == f["fit_labels"]
        assert str(dbg["pp"].tolist()) == f["pp"]
        assert float(dbg["inertia"]).hex() == f["inertia"]
        assert dbg["n_iter"] == f["n_iter"]


def test_fixture_fills_every_lds_class(edges, emu):
    """At least 20 fits of every LDS class at n_init = 10 (the hosts' value), so that the fixture cannot drift out of classes 4 / 5;
    the edges of the class rule's range; matrices that empty clusters and counts beyond a byte."""
    fits = edges["fits"]
    cls = [int(emu.lib.mprg_kmeans_lds_class(*f["shape"], f["k"], f["n_init"])) for f in fits]
    for c in range(6):
        assert sum(1 for f, x in zip(fits, cls) if x == c and f["n_init"] == 10) >= 20, c
    assert {f["shape"][0] for f in fits} >= {3, 4, 8, 9, 63, 64} and {f["shape"][1] for f in fits} >= {1, 3, 255, 1023, 1024}
    assert {f["k"] for f in fits} == set(range(2, 11)) and {f["n_init"] for f in fits} == {1, 2, 3, 7, 10}
    assert sum(int(matrix(f).max()) > 255 for f in fits) >= 5
    assert sum(orc.kmeans_fit_predict(matrix(f), f["k"], n_init=f["n_init"], want_debug=True)[1]["flags"] & 1 for f in fits) >= 20


@pytest.mark.parametrize("path,n_slots", [("lds", 0), ("one-launch", 0), ("fit", 5), ("wide", 0), ("global", 3)])
def test_fit_forms_equal_scikit_learn(edges, emu, path, n_slots):
    assert check_fits(emu, edges["fits"], path, n_slots) == len(edges["fits"])


def test_every_fit_of_the_small_form_has_an_lds_class(emu):
    """With KM_MODE bit 2 the control steps file a fit without an LDS class with the general form, never in the small form's list
    slots (the hosts launch those as LDS classes 4 / 5).  At the hosts' n_init every fit the small form admits has an LDS class anyway:
    the rule changes nothing the product runs."""
    for D in range(2, 301):
        for V in EDGE_VS:
            for k in range(2, 11):
                if emu.lib.mprg_kmeans_small_class(D, V, k, 10) >= 0:
                    assert emu.lib.mprg_kmeans_lds_class(D, V, k, 10) >= 0, (D, V, k)
    assert emu.lib.mprg_kmeans_lds_class(65, 1, 2, 10) < 0 and emu.lib.mprg_kmeans_lds_class(64, 1025, 2, 10) < 0
    assert emu.lib.mprg_kmeans_small_class(70, 4, 3, 2) >= 0          # (through the ABI's n_init: a small class beyond D = 64)


class _LibWithClass:
    """The library with mprg_kmeans_lds_class answering `cls` for every fit (a host that files fits in the wrong list)."""
    def __init__(self, lib, cls):
        self._lib, self._cls = lib, cls

    def mprg_kmeans_lds_class(self, D, V, k, n_init):
        return self._cls

    def __getattr__(self, name):
        return getattr(self._lib, name)


def test_lds_fit_refuses_fits_its_launch_does_not_hold(emu):
    """mprg_kmeans_fit_lds given, in a class-0 launch, fits of D = 65 and 70 (beyond the body's 64-sample arrays) and a fit of class 5:
    all report MPRG_KM_UNSUPPORTED and leave their labels alone; the class-0 fits of the same launches are scikit-learn's."""
    rng = np.random.default_rng(4)
    shapes = [(8, 4, 3), (70, 6, 3), (65, 4, 3), (9, 3, 6), (64, 5, 6)]          # class 0, none, none, 0, 5 (n_init = 10)
    assert [emu.lib.mprg_kmeans_lds_class(D, V, k, 10) for D, V, k in shapes] == [0, -1, -1, 0, 5]
    fits = []
    for D, V, k in shapes:
        M = rng.integers(0, 4, (D, V)).astype(np.float64)
        lab, dbg = orc.kmeans_fit_predict(M, k, want_debug=True)
        fits.append(dict(shape=[D, V], counts_i16_hex=M.astype("<i2").tobytes().hex(), k=k, labels=lab.tolist(),
                         inertia=float(dbg["inertia"]).hex(), n_iter=dbg["n_iter"]))
    wrong = emu.clone()
    wrong.lib = _LibWithClass(emu.lib, 0)
    got = run_kmeans_fits(wrong, fits, path="lds")
    poison = int(np.frombuffer(b"\xa5" * 4, np.int32)[0])          # (EmuBackend.empty: unwritten bytes are 0xA5)
    for g, f, (D, V, k) in zip(got, fits, shapes):
        if D in (70, 65, 64):
            assert g["status"] & MPRG_KM_UNSUPPORTED, (D, V, k)
            assert g["labels"] == [poison] * D
        else:
            assert not g["status"] & MPRG_KM_UNSUPPORTED
            assert g["labels"] == f["labels"] and g["inertia_hex"] == f["inertia"] and g["n_iter"] == f["n_iter"]


def lds_classes_of_oracle_run(lib, texts, N=5, L=7):
    """The LDS class (n_init = 10) of every KMeans fit the oracle runs while it builds `texts`."""
    cls = []

    def kmeans(M, k, *a, **kw):
        cls.append(int(lib.mprg_kmeans_lds_class(M.shape[0], M.shape[1], k, 10)))
        return orc.kmeans_fit_predict(M, k, *a, **kw)
    for t in texts:
        orc.build_locus(orc.load_alignment_text(t), N, L, kmeans=kmeans)
    return cls


def test_class45_seeds_still_hold_fits_of_the_largest_classes(emu):
    """tests/test_gpu_edges.py runs CLASS45_SEEDS through the forest's fused and per-round loops: they must hold fits of class 4 and 5."""
    from make_prg_amd.utils.synthetic import synth_config_fasta
    cls = lds_classes_of_oracle_run(emu.lib, [synth_config_fasta("C", s) for s in CLASS45_SEEDS])
    assert cls.count(4) >= 20 and cls.count(5) >= 6
