"""bench.py on the GPU: a plain run measures only its headline figure, --steps sets the number of
timed steps, and --dump-outputs writes what the last timed step returned."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu
FULL_ONLY = ("fft_block", "f32")  # legs a plain run does not measure


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    d = tmp_path_factory.mktemp("bench") / "dump"
    e = {k: v for k, v in os.environ.items()
         if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, f"{REPO}/bench.py", "--gpus", "1", "--steps", "3",
                        "--warmup", "1", "--batch", "4", "--src-len", "16", "--dump-outputs", str(d)],
                       capture_output=True, text=True, timeout=120, env=e)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0]), d


def test_plain_run_result_line(plain_run):
    out, _ = plain_run
    assert out["steps"] == 3 and out["warmup"] == 1 and out["n_gpus"] == 1
    assert out["unit"] == "mel-frames/s" and out["higher_is_better"] is True
    assert out["dtype"] == "bf16" and out["metric"].startswith("mel-frames/sec")
    assert out["ms_per_step"] > 0
    frames = out["config"]["valid_frames_per_rank_step"]
    assert out["value"] == pytest.approx(frames / (out["ms_per_step"] / 1e3), rel=1e-3)
    assert out["roofline"] is None and out["cpu_baseline"] is None
    assert not any(k in out for k in FULL_ONLY)


def test_plain_run_dumps_last_step(plain_run):
    out, d = plain_run
    got = {f[:-4]: np.load(d / f) for f in os.listdir(d)}
    assert {"loss_0", "gmm_loss", "grad_norm", "output_0", "output_1"} <= set(got)
    assert all(a.dtype == np.float32 for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 * 2 ** 20
    assert float(got["loss_0"]) == pytest.approx(out["final_loss"], rel=1e-6, abs=1e-5)
    assert np.isfinite(got["grad_norm"]) and got["grad_norm"] > 0
    T_m = out["config"]["seq_len"]
    assert got["output_0"].shape == (4, T_m, 80) and np.all(np.isfinite(got["output_0"]))
