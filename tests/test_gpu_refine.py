"""Leave-one-out refinement of `from_msa --unaligned --refine` on the MI355X, through both backends: refined MSAs and S byte-equal
to the spec's plain-Python statement (tests/refine_ref.py) on a few hundred small loci, `--band` against no band,
`--adjust-direction` with flipped records, the invariants and the S properties on config-C-shaped loci, the device entry points
one by one, their status codes for tables that point outside the buffers, and the command line end to end."""
import os
import random
import subprocess
import sys

import pytest

from make_prg_amd.from_msa import star_align as sa
from make_prg_amd.update import profile_align as pa
from tests import refine_common as rc
from tests import refine_ref as rr
from tests import star_ref as sr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", params=["runtime", "torch"])
def backend(request):
    import torch  # noqa: F401  (before the library: HipBackend needs torch's HIP runtime to be the one the library binds)
    from make_prg_amd import backend as b
    return b.HipRuntimeBackend(0) if request.param == "runtime" else b.HipBackend(0)


def small_loci():
    loci = sr.edge_loci() + rr.special_loci() + [rr.diverged_locus(s) for s in rr.DIVERGED_SEEDS]
    for seed in range(20, 26):
        loci += sr.random_loci(seed)
    return loci


@pytest.fixture(scope="module")
def small_spec():
    return [rr.refined_star_rows(l, 2) for l in small_loci()]


def test_small_loci_equal_the_spec_with_and_without_band(backend, small_spec):
    loci = small_loci()
    assert len(loci) >= 250
    recs = [rc.records(l) for l in loci]
    for kw in (dict(), dict(band=True), dict(band=True, budget_bytes=4 * pa.workspace_words(360, 420), chunk_bytes=1 << 14)):
        info, timings = [], {}
        msas = sa.star_msas(backend, recs, refine=2, refinement=info, timings=timings, **kw)
        for l, m, got, (rows, acc, trail) in zip(loci, msas, info, small_spec):
            assert m.rows_as_strings() == rows, (l, kw)
            assert got == (acc, trail[0], trail[-1]), (l, kw)
        assert sum(1 for a, _, _ in info if a == 2) >= 5 and sum(1 for a, _, _ in info if a == 0) >= 100
        assert timings["refine_s"] > 0


def test_six_diverged_loci_gain(backend):
    loci = [rr.diverged_locus(s) for s in rr.DIVERGED_SEEDS]
    info = []
    msas = sa.star_msas(backend, [rc.records(l) for l in loci], refine=3, refinement=info)
    for l, m, got in zip(loci, msas, info):
        rows, acc, trail = rr.refined_star_rows(l, 3)
        assert m.rows_as_strings() == rows and got == (acc, trail[0], trail[-1])
        assert acc >= 1 and got[2] == max(trail) > got[1]


def test_adjust_direction_with_flipped_records(backend):
    rng = random.Random(4)
    loci = [rr.diverged_locus(s, 8) for s in range(10, 22)] + sr.random_loci(31, 30)
    flipped = [[rc.revcomp(s) if i and rng.random() < 0.4 else s for i, s in enumerate(l)] for l in loci]
    recs = [rc.records(l) for l in flipped]
    star = sa.star_msas(backend, recs, adjust_direction=True)
    for band in (False, True):
        info = []
        msas = sa.star_msas(backend, recs, adjust_direction=True, refine=2, refinement=info, band=band)
        rc.check_invariants(flipped, msas, info, star)
        assert sum(t.startswith(sa.REVERSED_PREFIX) for m in msas for t in m.descriptions) >= 20
        assert sum(1 for a, _, _ in info if a) >= 8
        for m, got in zip(msas, info):                          # the spec on the sequences as the device oriented them
            rows, acc, trail = rr.refined_star_rows([r.replace("-", "") for r in m.rows_as_strings()], 2)
            assert m.rows_as_strings() == rows and got == (acc, trail[0], trail[-1])


def test_config_c_shaped_loci(backend):
    """Config-C-shaped loci (S ~ 100, C 1 000-3 000) with their gaps removed, in several chunks, pair launches and refinement
    groups: the invariants, S of the star MSA and of the result against the plain-Python objective, S(result) >= S(star), a
    locus with no accepted round equal to its star MSA, and the same MSAs with the band."""
    loci = [seqs for _, seqs in sr.synthetic_loci(range(12))]
    recs = [rc.records(l) for l in loci]
    budget = 4 * 600 * pa.workspace_words(3000, 3000)
    star = sa.star_msas(backend, recs, budget_bytes=budget, chunk_bytes=1 << 25)
    info = []
    msas = sa.star_msas(backend, recs, refine=2, refinement=info, budget_bytes=budget, chunk_bytes=1 << 25)
    rc.check_invariants(loci, msas, info, star)
    banded = sa.star_msas(backend, recs, refine=2, band=True, budget_bytes=1 << 24)
    assert [m.rows_as_strings() for m in banded] == [m.rows_as_strings() for m in msas]


def test_device_entries_one_by_one(backend):
    msas = [sr.star_rows(l)[1] for l in sr.edge_loci() + rr.special_loci() + sr.random_loci(8, 12) + [rr.diverged_locus(1)]]
    rng = random.Random(5)
    holed = []
    for m in msas:
        cuts = sorted(rng.randrange(len(m[0]) + 1) for _ in range(3))
        holed.append(["-" * (cuts[0] == 0) + "".join(ch + "-" * cuts.count(j + 1) for j, ch in enumerate(r)) for r in m])
    rc.check_counts_profiles_and_compaction(backend, msas + holed + [["--", "--"], ["-A-", "---", "-C-"]])


def test_abi_statuses(backend):
    rc.check_abi_statuses(backend)


def run_cli(args):
    env = dict(os.environ, PYTHONPATH=ROOT)
    res = subprocess.run([sys.executable, "-m", "make_prg_amd"] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-3000:]
    return res


def test_command_line_refine(tmp_path):
    src = tmp_path / "unaligned"
    src.mkdir()
    want, changed = {}, 0
    for k in range(6):
        recs = [(f"s{i} sample {i}", s) for i, s in enumerate(rr.diverged_locus(40 + k, 8))]
        (src / f"gene{k}.fa").write_text("".join(f">{t}\n{s}\n" for t, s in recs))
        rows, acc, _ = rr.refined_star_rows([s for _, s in recs], 2)
        changed += acc > 0
        want[f"gene{k}.fa"] = "".join(f">{t}\n{r}\n" for (t, _), r in zip(recs, rows))
    assert changed >= 3
    msa_dir, a, b = tmp_path / "msas", str(tmp_path / "A" / "a"), str(tmp_path / "B" / "b")
    res = run_cli(["from_msa", "--unaligned", "--refine", "--msa-dir", str(msa_dir), "-i", str(src), "-o", a])
    assert "--refine 2:" in res.stderr + res.stdout and "rounds accepted" in res.stderr + res.stdout
    run_cli(["from_msa", "-i", str(msa_dir), "-o", b])
    assert {p: (msa_dir / p).read_text() for p in os.listdir(msa_dir)} == want
    for suffix in (".prg.fa", ".prg.bin.zip", ".prg.gfa.zip", ".update_DS.zip"):
        assert open(a + suffix, "rb").read() == open(b + suffix, "rb").read(), suffix
    msa_dir2 = tmp_path / "msas2"
    run_cli(["from_msa", "--unaligned", "--refine", "2", "--band", "--adjust-direction", "--msa-dir", str(msa_dir2), "-i", str(src), "-o",
             str(tmp_path / "C" / "c")])
    assert {p: (msa_dir2 / p).read_text() for p in os.listdir(msa_dir2)} == want
    env = dict(os.environ, PYTHONPATH=ROOT)
    res = subprocess.run([sys.executable, "-m", "make_prg_amd", "from_msa", "--unaligned", "--refine", "17", "-i", str(src), "-o",
                          str(tmp_path / "D" / "d")], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert res.returncode == 2 and "--refine" in res.stderr
