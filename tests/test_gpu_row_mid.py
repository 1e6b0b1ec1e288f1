"""GPU twin of tests/test_row_mid_emulated.py: the mid-width views of mprg_ungap_dedupe (k_rows_mid) on the MI355X — the unaligned
16-byte loads, the staging rows in LDS between the wavefront-scope syncs, the barrier before the dedupe and many workgroups at once are
only seen here.  Every batch of tests/row_mid_cases.py: all output arrays against the same library with MPRG_ROW_MID=0 (a child
process) and against the restatement, two alignments against the oracle; 100 config-C alignments through the per-step host and
mprg_forest_level, the switch on and off, four against the oracle.  (The weak-hash build exists for the emulator alone.)
Run with `-m gpu`."""
import json
import os
import subprocess
import sys

import pytest

from tests import parity_common as pc
from tests import row_mid_cases as rm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH = 100


@pytest.fixture(scope="module")
def rt():
    import torch  # noqa: F401  (before the library: a later HipBackend needs torch's HIP runtime to be the one the library binds)
    from make_prg_amd.backend import HipRuntimeBackend
    return HipRuntimeBackend(0)


@pytest.fixture(autouse=True)
def forest_host(monkeypatch):
    monkeypatch.setattr(pc, "ENGINE", "forest")


def child(code, **env):
    run = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, sys.argv[1]); from tests import row_mid_cases as rm; "
                          "from make_prg_amd.backend import HipRuntimeBackend; be = HipRuntimeBackend(0); " + code, ROOT],
                         env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-3000:]
    return run.stdout


@pytest.fixture(scope="module")
def switch_off(tmp_path_factory):
    """Every batch's outputs with MPRG_ROW_MID=0, from ONE child process."""
    d = tmp_path_factory.mktemp("row_mid_off")
    paths = {b: str(d / f"{j}.npz") for j, b in enumerate(rm.BATCHES)}
    child("".join(f"rm.dump(be, {b!r}, {p!r}); " for b, p in paths.items()), MPRG_ROW_MID="0")
    return paths


@pytest.mark.parametrize("batch", rm.BATCHES)
def test_every_output_equals_the_switch_off(rt, switch_off, batch):
    assert rm.check_views(rt, batch, switch_off[batch]) >= 3


@pytest.mark.parametrize("batch", rm.BATCHES)
def test_two_alignments_vs_oracle(rt, batch):
    pc.check_vs_oracle(rt, *rm.oracle_texts(batch))


def test_forest_equal_with_the_switch_off(rt):
    on = rm.forest_digest(rt, range(BATCH))
    assert on["per_step"] == on["level"]
    off = json.loads(child(f"import json; print(json.dumps(rm.forest_digest(be, range({BATCH}))))", MPRG_ROW_MID="0").strip().splitlines()[-1])
    assert off == on


def test_four_alignments_vs_oracle(rt):
    from make_prg_amd.utils.synthetic import synth_config_fasta
    pc.check_vs_oracle(rt, [synth_config_fasta("C", s) for s in (1, 5, 17, 23)])
