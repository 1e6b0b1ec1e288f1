"""MPRG_IV_SELF / MPRG_NF_SELF on the emulation backend: the hint of the three partition kernels against the oracle's partition of
every non-match interval's own columns (tests/iv_self_cases.py), the views that must not carry it, and the forest with the hint used
and ignored (MPRG_IV_SELF=0 in a child process: the switch is read once when the library loads) — equal PRGs and trees, and no child of
a multi-interval node in a partition list."""
import json
import os
import subprocess
import sys

import pytest

from tests import iv_self_cases as ic
from tests.emu.backend import EmuBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BACKEND = "from tests.emu.backend import EmuBackend as B; be = B()"
N_FOREST = 6          # (alignments of the forest test: the emulation runs one workgroup at a time)


@pytest.fixture(scope="module")
def emu():
    return EmuBackend()


@pytest.fixture(scope="module")
def cases():
    return ic.all_cases()


def child(code: str, env: dict, timeout: int = 600):
    res = subprocess.run([sys.executable, "-c", "import json, sys; sys.path.insert(0, sys.argv[1]); from tests import iv_self_cases as ic; "
                          + BACKEND + "; " + code, ROOT], env=dict(os.environ, **env), capture_output=True, text=True, timeout=timeout)
    assert res.returncode == 0, res.stderr[-3000:]
    return json.loads(res.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("form", ["workgroup", "lists"])
def test_hint_is_the_scan(emu, cases, form):
    stats = ic.check_cases(emu, cases, form)
    print(form, stats)
    assert stats["yes"] > 1000 and stats["wave"] > 500 and stats["fused"] > 300


def test_hint_is_the_scan_fused_for_all(cases):
    stats = child("print(json.dumps(ic.check_cases(be, ic.all_cases(), 'lists')))", dict(MPRG_WAVE_VIEWS="0"))
    assert stats["yes"] > 1000


@pytest.mark.parametrize("form", ["workgroup", "lists"])
def test_no_hint_with_n_iupac_or_no_rows(emu, form):
    ic.check_no_hint(emu, form)


def test_no_hint_on_global_scratch(emu):
    ic.check_not_fast(emu)


@pytest.mark.parametrize("kloop", ["rounds", "fused"])
def test_forest_equal_with_the_switch_off(emu, kloop):
    on = ic.forest_digest(emu, kloop, N_FOREST)
    off = child(f"print(json.dumps(ic.forest_digest(be, {kloop!r}, {N_FOREST})))", dict(MPRG_IV_SELF="0"))
    assert [d["host"] for d in on] == (["per-step"] if kloop == "rounds" else ["per-step", "level"])
    ic.check_forest(on, off)


def test_alignment_with_n(emu):
    ic.check_golden_n(emu)
