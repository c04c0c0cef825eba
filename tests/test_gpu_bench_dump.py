"""bench.py --dump-outputs: the files hold what the last timed C2 step
computed.  One small run (2 x 2e6 rows, the pairs streamed through a buffer
smaller than the plan, so the dump reads the last two chunks and samples
them) against the same inputs run through the engine here."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, CHUNK = 2_000_000, 2_500_000  # ~6.5e6 pairs: three chunks, the last one partial


@pytest.fixture(scope="module")
def dumped(tmp_path_factory):
    d = tmp_path_factory.mktemp("dump")
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "2", "--warmup",
                          "1", "--rows", str(ROWS), "--chunk", str(CHUNK), "--dump-outputs",
                          str(d)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    line = json.loads([x for x in out.stdout.splitlines() if x.startswith("{")][-1])
    files = {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}
    return line, files


def test_plain_line_and_dump_files(dumped):
    line, files = dumped
    assert line["steps"] == 2 and line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(2 * ROWS / (line["ms_per_step"] * 1e-3))
    # a plain run measures nothing but its steps
    assert "operators" not in line and line["cpu_baseline"] is None
    assert set(files) == {"pairs", "pairs_index"} | {
        f"merge_{s}{t}" for s in "ab" for t in ("", "_index", "_run_of_row", "_run_of_row_index")}
    assert all(a.dtype == np.float64 for a in files.values())
    assert sum(a.nbytes for a in files.values()) <= 64e6


def test_dump_matches_engine(dumped, ctx):
    import torch

    import lime_amd
    from lime_amd import synth
    line, files = dumped
    sp = lime_amd.Space(list(synth.HG38.keys()), list(synth.HG38.values()))
    sets = []
    for seed in (0xA, 0xB):
        cols = [torch.empty(ROWS, dtype=torch.int32, device="cuda:0") for _ in range(3)]
        ctx.synth_uniform_rows(sp, 0, ROWS, seed, 50, 5000, *(c.data_ptr() for c in cols))
        torch.cuda.synchronize()
        sets.append(ctx.set_from_device(sp, ROWS, *(c.data_ptr() for c in cols)))
    plan = ctx.intersect(*sets)
    assert plan.n == line["config"]["pairs_per_step"] > 2 * CHUNK
    idx = files["pairs_index"].astype(np.int64)
    # sampled, from the last chunk and the one before it
    assert 0 < len(idx) < plan.n and idx.min() < (plan.n // CHUNK) * CHUNK <= idx.max()
    full = plan.fill_host()
    want = np.stack([full[k][idx] for k in ("start", "end", "a_row", "b_row")], 1)
    assert np.array_equal(files["pairs"], want.astype(np.float64))
    for s, X in zip("ab", sets):
        mg = ctx.merge(X)
        gs, ge = mg.copy_range(0, mg.n)
        pos = files[f"merge_{s}_index"].astype(np.int64)
        assert np.array_equal(files[f"merge_{s}"], np.stack([gs[pos], ge[pos]], 1))
        pos = files[f"merge_{s}_run_of_row_index"].astype(np.int64)
        assert len(pos) < ROWS
        assert np.array_equal(files[f"merge_{s}_run_of_row"], mg.run_of_row(ROWS)[pos])
        mg.close()
    plan.close()
    for X in sets:
        X.close()
