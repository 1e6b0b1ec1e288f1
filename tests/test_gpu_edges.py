"""GPU twins of the emulator-only edge tests: the rare paths of the forest's kernels (tests/view_edges.py, as
tests/test_random_emulated.py forces them) and the KMeans fits across the whole range of the LDS form of the fit
(tests/golden/kmeans_lds_edges.json.gz, tests/test_kmeans_relocation.py's wide shapes), on the MI355X against the oracle and
scikit-learn's answers.  The emulator runs one workgroup at a time with its threads switching only at barriers, ballots and
shuffles: a missing barrier, cross-workgroup atomics, wave64 lock-step and dynamic LDS above 64 KB are only seen here.
Run on the MI355X box with `-m gpu`."""
import numpy as np
import pytest

from tests import parity_common as pc
from tests import view_edges as ve
from tests.view_edges import RANDOM_WITH_N

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rt():
    """The runtime backend (the library's own mprg_rt_* plumbing; what the command line uses): every case."""
    from make_prg_amd.backend import HipRuntimeBackend
    return HipRuntimeBackend(0)


@pytest.fixture(scope="module", params=["torch", "runtime"])
def hip(request, rt):
    """Both product backends over the same library: the cheap cases."""
    from make_prg_amd.backend import HipBackend
    return HipBackend(0) if request.param == "torch" else rt


def _record_calls(be, monkeypatch):
    calls = []
    orig = be.call
    monkeypatch.setattr(be, "call", lambda name, *a, **k: (calls.append((name, a)), orig(name, *a, **k))[1])
    return calls


def test_library_is_the_hip_build(rt):
    assert b"hip gfx950" in rt.lib.mprg_version()


# ---------------------------------------------------------------- the forest's rare paths (tests/test_random_emulated.py)
@pytest.mark.parametrize("N,L,S,C,p", ve.WIDE_VIEWS)
def test_wide_views_take_the_fallback_paths(rt, N, L, S, C, p, monkeypatch):
    monkeypatch.setattr(pc, "ENGINE", "forest")
    pc.check_vs_oracle(rt, *ve.wide_view(N, L, S, C, p))


def test_gap_runs_reach_across_column_segments(hip, monkeypatch):
    monkeypatch.setattr(pc, "ENGINE", "forest")
    for N, L in ve.GAP_RUN_NL:
        pc.check_vs_oracle(hip, *ve.gap_runs_across_segments(N, L))


def test_leaf_of_many_alleles_is_laid_out_by_its_wavefront(hip, monkeypatch):
    monkeypatch.setattr(pc, "ENGINE", "forest")
    eng = pc.check_vs_oracle(hip, *ve.leaf_of_many_alleles())
    assert int(eng.tab["nseq"].max()) > 128


def test_tall_view_takes_the_wide_majority_workgroups(hip, monkeypatch):
    monkeypatch.setattr(pc, "ENGINE", "forest")
    pc.check_vs_oracle(hip, *ve.tall_view())


def test_more_clusters_than_the_lds_offsets_of_split_children(rt, monkeypatch):
    monkeypatch.setattr(pc, "ENGINE", "forest")
    eng = pc.check_vs_oracle(rt, *ve.many_short_clusters())
    assert np.bincount(eng.tab["parent"][eng.tab["parent"] >= 0]).max() > 1024      # a cluster node with > 1024 children


def test_wide_and_tall_view_shares_a_rows_candidates_among_threads(rt, monkeypatch):
    monkeypatch.setattr(pc, "ENGINE", "forest")
    pc.check_vs_oracle(rt, *ve.wide_and_tall_view())


def test_problems_prepared_without_tables_stay_with_the_wide_fits(rt, monkeypatch):
    import make_prg_amd.forest as F
    monkeypatch.setattr(F, "KM_BIG_BYTES", 1)
    monkeypatch.setattr(F, "KM_NO_TABLES_BYTES", 1)
    monkeypatch.setattr(pc, "ENGINE", "forest")
    texts, N, L = ve.clades_without_tables()
    eng = pc.check_vs_oracle(rt, texts, N, L)
    assert eng._big_seen and int(eng.counters.get("max_problem_bytes", 0)) > 156 * 1024
    assert rt.lib.mprg_kmeans_lds_class(44, 744, 2, 10) >= 0
    monkeypatch.setattr(F, "KM_NO_TABLES_BYTES", 4 << 30)
    pc.check_vs_oracle(rt, texts, N, L)


@pytest.mark.parametrize("km_mode", [0, 2])
def test_every_round_of_a_big_level_at_once(rt, monkeypatch, golden_integration, km_mode):
    from tests.random_msas import random_cases
    import make_prg_amd.forest as F
    monkeypatch.setattr(F, "KM_BIG_BYTES", 1)
    monkeypatch.setattr(F, "KM_SPEC_PROBLEMS", 1 << 30)
    monkeypatch.setattr(F, "KM_MODE", km_mode)
    monkeypatch.setattr(pc, "ENGINE", "forest")
    eng = pc.check_vs_oracle(rt, random_cases(53, 24), 5, 7)
    assert eng._big_seen and eng.counters.get("speculative_levels", 0) >= 1
    assert pc.check_integration(rt, golden_integration) >= 30


@pytest.mark.parametrize("no_tables_from", [1, 1 << 40])
def test_big_problem_through_the_byte_matrix(rt, monkeypatch, no_tables_from):
    import make_prg_amd.forest as F
    monkeypatch.setattr(F, "KM_BIG_BYTES", 200_000)
    monkeypatch.setattr(F, "KM_NO_TABLES_BYTES", no_tables_from)
    monkeypatch.setattr(pc, "ENGINE", "forest")
    eng = pc.check_vs_oracle(rt, *ve.byte_matrix_problem())
    assert eng._big_seen and eng.counters["max_problem_bytes"] > 156 * 1024


# ---------------------------------------------------------------- the same paths over ambiguity codes (tests/view_edges.sprinkle)
@pytest.mark.parametrize("N,L,S,C,p", ve.WIDE_VIEWS)
def test_wide_views_with_ambiguity_codes(rt, N, L, S, C, p, monkeypatch):
    monkeypatch.setattr(pc, "ENGINE", "forest")
    eng = pc.check_vs_oracle(rt, *ve.sprinkled(ve.wide_view(N, L, S, C, p), ve.SEED_AMB_WIDE, ve.P_AMB_WIDE))
    assert eng.tab["special"].any()


def test_gap_runs_across_column_segments_with_ambiguity_codes(rt, monkeypatch):
    monkeypatch.setattr(pc, "ENGINE", "forest")
    for N, L in ve.GAP_RUN_NL:
        eng = pc.check_vs_oracle(rt, *ve.sprinkled(ve.gap_runs_across_segments(N, L), ve.SEED_AMB, ve.P_AMB))
        assert eng.tab["special"].any()


def test_leaf_of_many_alleles_with_ambiguity_codes(rt, monkeypatch):
    monkeypatch.setattr(pc, "ENGINE", "forest")
    eng = pc.check_vs_oracle(rt, *ve.sprinkled(ve.leaf_of_many_alleles(), ve.SEED_AMB, ve.P_AMB))
    assert eng.tab["special"].any()
    assert int(eng.tab["nseq"][ve.special_leaves(eng)].max()) > 128


def test_tall_view_with_ambiguity_codes(rt, monkeypatch):
    monkeypatch.setattr(pc, "ENGINE", "forest")
    eng = pc.check_vs_oracle(rt, *ve.sprinkled(ve.tall_view(), ve.SEED_AMB, ve.P_AMB))
    assert eng.tab["special"].any()


def test_more_clusters_than_the_lds_offsets_with_ambiguity_codes(rt, monkeypatch):
    """The codes only in the columns between the two match intervals (ve.SHORT_CLUSTER_COLS): the node of more than 1 024 clusters
    stays, and some of its one-sequence clusters are leaves that the host expands."""
    monkeypatch.setattr(pc, "ENGINE", "forest")
    eng = pc.check_vs_oracle(rt, *ve.sprinkled(ve.many_short_clusters(), ve.SEED_AMB, ve.P_AMB, cols=ve.SHORT_CLUSTER_COLS))
    assert eng.tab["special"].any()
    assert np.bincount(eng.tab["parent"][eng.tab["parent"] >= 0]).max() > 1024


def test_wide_and_tall_view_with_ambiguity_codes_against_the_oracles_record(rt):
    """k_dedupe_scan_big / k_ungap_hash over 530 x 4 200 cells with codes 5..10 in the rows.  The oracle needs 15 s for this one: its
    answer is tests/golden/rare_paths_codes.json (oracle/tools/gen_rare_paths_golden.py; tests/test_oracle_golden.py holds the record
    against the oracle)."""
    import json
    import os
    from make_prg_amd.utils.gfa import GFA_Output
    name = "wide_and_tall_view"
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rare_paths_codes.json")) as fh:
        g = json.load(fh)[name]
    texts, N, L = ve.sprinkled(getattr(ve, name)(), g["seed"], g["p"])
    assert pc.sha(texts[0]) == g["fasta_sha256"] and (N, L) == (g["N"], g["L"]), "the builder changed under the record"
    got, eng = pc.run_batch(rt, texts, N, L, "forest")
    got, e = got[0], g["expect"]
    assert "error" not in got, got
    assert (len(got["prg"]), pc.sha(got["prg"])) == (e["prg_len"], e["prg_sha256"])
    assert pc.sha(pc.product_bin_bytes(got["prg"])) == e["bin_sha256"]
    assert pc.sha(GFA_Output.gfa_text(got["prg"])) == e["gfa_sha256"]
    assert pc.sha(got["tree"]) == e["tree_sha256"], "recursion tree differs from the oracle's"
    assert pc.sha(got["prg_index"]) == e["prg_index_sha256"]
    assert (got["next_node_id"], got["site_num"]) == (e["next_node_id"], e["site_num"])
    assert eng.tab["special"].any()


@pytest.mark.parametrize("N,L,S,C,p", ve.WIDE_VIEWS)
def test_wide_views_with_n_through_the_loader(rt, N, L, S, C, p, monkeypatch):
    monkeypatch.setattr(pc, "ENGINE", "forest")
    pc.check_vs_oracle(rt, *ve.sprinkled(ve.wide_view(N, L, S, C, p), ve.SEED_AMB_WIDE, ve.P_AMB_WIDE, "N"))


def test_more_special_leaves_than_the_first_capacity(rt, monkeypatch):
    monkeypatch.setattr(pc, "ENGINE", "forest")
    eng = pc.check_vs_oracle(rt, *ve.many_special_leaves())
    assert int(ve.special_leaves(eng).sum()) > 1024


# ---------------------------------------------------------------- alignments that still hold N, through the object path
@pytest.mark.parametrize("host", ["forest", "nodes"])
@pytest.mark.parametrize("N,L,seed,want", RANDOM_WITH_N)
def test_random_alignments_that_hold_n(rt, N, L, seed, want, host):
    from tests.random_msas import random_cases
    c, _ = pc.check_objects_vs_oracle(rt, random_cases(seed, 150), N, L, host)
    assert (c["matched"], c["errors"], c["matched_with_n"]) == want


@pytest.mark.parametrize("host", ["forest", "nodes"])
def test_views_on_the_rare_paths_that_hold_n(rt, host):
    got = []
    for w in ve.WIDE_VIEWS:
        got.append(pc.check_objects_vs_oracle(rt, *ve.sprinkled(ve.wide_view(*w), ve.SEED_AMB_WIDE, ve.P_N_WIDE, "N"), host)[0])
    got.append(pc.check_objects_vs_oracle(rt, *ve.sprinkled(ve.tall_view(), ve.SEED_AMB, ve.P_N_TALL, "N"), host)[0])
    got.append(pc.check_objects_vs_oracle(rt, *ve.sprinkled(ve.leaf_of_many_alleles(), ve.SEED_AMB, ve.P_N_LEAF, "N"), host)[0])
    assert [(c["matched_with_n"], c["errors"]) for c in got] == ve.N_VIEWS_ORACLE


@pytest.mark.parametrize("host", ["forest", "nodes"])
def test_n_by_hand(rt, host):
    names = sorted(ve.N_BY_HAND)
    got, _ = pc.run_msas(rt, [pc.msa_as_it_is(ve.N_BY_HAND[n][0]) for n in names], 5, 7, host)
    assert [g.get("error", g.get("prg")) for g in got] == [ve.N_BY_HAND[n][1] for n in names]
    c, _ = pc.check_objects_vs_oracle(rt, [ve.N_BY_HAND[n][0] for n in names], 5, 7, host)
    assert (c["matched"], c["errors"]) == (2, 2)


# ---------------------------------------------------------------- KMeans fits across the LDS form's range (tests/test_kmeans_edges.py)
def test_lds_edges_through_the_lds_form(hip, monkeypatch):
    """Every fit of the fixture through mprg_kmeans_fit_lds by class (the fits without a class through mprg_kmeans_fit), bit-exact;
    the launches cover every class 0..5 — 4 and 5 with more than 64 KB of dynamic LDS, 512 / 1 024 threads per fit."""
    from tests.test_kmeans_edges import check_fits, load_fits
    fits = load_fits()["fits"]
    calls = _record_calls(hip, monkeypatch)
    assert check_fits(hip, fits, "lds") == len(fits)
    assert {a[4] for name, a in calls if name == "mprg_kmeans_fit_lds"} == set(range(6))


@pytest.mark.parametrize("path,n_slots", [("one-launch", 0), ("fit", 5), ("fit", 4096), ("wide", 0), ("wide-stats", 0)])
def test_lds_edges_through_the_other_forms(rt, path, n_slots):
    from tests.test_kmeans_edges import check_fits, load_fits
    fits = load_fits()["fits"]
    assert check_fits(rt, fits, path, n_slots) == len(fits)


def test_fits_with_many_samples(rt):
    from tests.kmeans_direct import run_kmeans_fits
    from tests.test_kmeans_relocation import MANY_SAMPLE_PATHS, many_sample_fits
    fits = many_sample_fits()
    for path, slots in MANY_SAMPLE_PATHS:
        got = run_kmeans_fits(rt, fits, path=path, n_slots=slots)
        for g, f in zip(got, fits):
            assert not g["status"] & 2
            assert g["labels"] == f["labels"] and g["inertia_hex"] == f["inertia"] and g["n_iter"] == f["n_iter"]


def test_relocation_with_wide_matrices(rt):
    from tests.test_kmeans_relocation import check, wide_relocation_fits
    fits = wide_relocation_fits()
    assert len(fits) >= 3
    check(rt, fits)
    check(rt, fits, path="one-launch")
    check(rt, fits, path="wave")
    check(rt, fits, path="small")
    check(rt, fits, path="lds")
    check(rt, fits, path="fit", n_slots=2)


def test_fits_outside_the_lds_count_form(rt):
    from tests.kmeans_direct import run_kmeans_fits
    from tests.test_kmeans_relocation import COUNT_FORM_PATHS, count_form_fits
    fits = count_form_fits()
    for path, slots in COUNT_FORM_PATHS:
        got = run_kmeans_fits(rt, fits, path=path, n_slots=slots)
        for g, f in zip(got, fits):
            assert not g["status"] & 2
            assert g["labels"] == f["labels"] and g["inertia_hex"] == f["inertia"] and g["n_iter"] == f["n_iter"]


# ---------------------------------------------------------------- the clustering loop at LDS classes 4 / 5 through the forest
@pytest.mark.parametrize("kloop", ["fused", "rounds"])
def test_loops_with_fits_of_the_largest_lds_classes(rt, monkeypatch, kloop):
    """Config-C alignments whose fits reach LDS classes 4 and 5 (tests/test_kmeans_edges.CLASS45_SEEDS) in one batch: the fused loop
    (k_cluster_loop_lds, whose staging keeps the counts — such fits are of class >= 4 or have none there, the general pass's) and the
    per-round launches (mprg_kmeans_fit_lds by class), against the oracle."""
    import make_prg_amd.forest as F
    from make_prg_amd.utils.synthetic import synth_config_fasta
    from tests.test_kmeans_edges import CLASS45_SEEDS
    monkeypatch.setattr(F, "KLOOP", kloop)
    monkeypatch.setattr(pc, "ENGINE", "forest")
    calls = _record_calls(rt, monkeypatch)
    eng = pc.check_vs_oracle(rt, [synth_config_fasta("C", s) for s in CLASS45_SEEDS], 5, 7)
    assert eng.kloop_fused == (kloop == "fused")
    if kloop == "rounds":
        assert {4, 5} <= {a[4] for name, a in calls if name == "mprg_kmeans_fit_lds"}
