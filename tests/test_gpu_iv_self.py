"""GPU twin of tests/test_iv_self_emulated.py: the same cases through the three partition kernels on the MI355X, 300 config-C alignments
through both forest hosts with the MPRG_IV_SELF hint used (this process) and ignored (a child: the switch is read once when the library
loads), and an alignment with N from tests/golden.  Run with `-m gpu`."""
import json
import os
import subprocess
import sys

import pytest

from tests import iv_self_cases as ic

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BACKEND = "from make_prg_amd.backend import HipRuntimeBackend as B; be = B(0)"


@pytest.fixture(scope="module")
def rt():
    import torch  # noqa: F401  (before the library: a later HipBackend needs torch's HIP runtime to be the one the library binds)
    from make_prg_amd.backend import HipRuntimeBackend
    return HipRuntimeBackend(0)


@pytest.fixture(scope="module")
def cases():
    return ic.all_cases()


def child(code: str, env: dict, timeout: int = 300):
    res = subprocess.run([sys.executable, "-c", "import json, sys; sys.path.insert(0, sys.argv[1]); from tests import iv_self_cases as ic; "
                          + BACKEND + "; " + code, ROOT], env=dict(os.environ, **env), capture_output=True, text=True, timeout=timeout)
    assert res.returncode == 0, res.stderr[-3000:]
    return json.loads(res.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("form", ["workgroup", "lists"])
def test_hint_is_the_scan(rt, cases, form):
    stats = ic.check_cases(rt, cases, form)
    print(form, stats)
    assert stats["yes"] > 1000 and stats["wave"] > 500 and stats["fused"] > 300


def test_hint_is_the_scan_fused_for_all(cases):
    stats = child("print(json.dumps(ic.check_cases(be, ic.all_cases(), 'lists')))", dict(MPRG_WAVE_VIEWS="0"))
    assert stats["yes"] > 1000


@pytest.mark.parametrize("form", ["workgroup", "lists"])
def test_no_hint_with_n_iupac_or_no_rows(rt, form):
    ic.check_no_hint(rt, form)


def test_no_hint_on_global_scratch(rt):
    ic.check_not_fast(rt)


@pytest.mark.parametrize("kloop", ["rounds", "fused"])
def test_forest_equal_with_the_switch_off(rt, kloop):
    on = ic.forest_digest(rt, kloop)
    off = child(f"print(json.dumps(ic.forest_digest(be, {kloop!r})))", dict(MPRG_IV_SELF="0"))
    assert [d["host"] for d in on] == (["per-step"] if kloop == "rounds" else ["per-step", "level"])
    ic.check_forest(on, off)


def test_alignment_with_n(rt):
    ic.check_golden_n(rt)
