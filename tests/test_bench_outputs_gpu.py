"""bench.py's plain run (one timed block of exactly --steps steps, nothing beyond the headline) and --dump-outputs: what
the timed loop hands back after its last step, as .npy files, identical from run to run.  GPU only."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu

SAMPLE = 1 << 21           # bench.DUMP_SAMPLE


def _bench(out_dir, edge, dtype, steps=7, warmup=2):
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--edge", str(edge), "--dtype", dtype,
           "--steps", str(steps), "--warmup", str(warmup), "--dump-outputs", str(out_dir)]
    p = subprocess.run(cmd, cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-3000:]
    return json.loads(lines[0])


@pytest.mark.parametrize("dtype,edge", [("f32", 48), ("f64", 132)])      # 132^3 > SAMPLE cells: the sampled form
def test_plain_run_times_the_steps_and_dumps_the_outputs(tmp_path, dtype, edge):
    out = _bench(tmp_path / "a", edge, dtype)
    assert out["unit"] == "Mcells/s" and out["higher_is_better"] is True and out["dtype"] == dtype
    assert out["steps"] == 7 and out["warmup"] == 2 and out["timed_blocks"]["blocks"] == 1
    assert out["ms_per_step"] > 0 and out["value"] == pytest.approx(edge ** 3 / out["ms_per_step"] / 1e3, rel=2e-2)
    assert not {"roofline", "parity_check", "f64_state", "viscosity", "cpu_baseline"} & set(out), sorted(out)

    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["d.npy", "history.npy", "r.npy", "x.npy"]
    ft = np.float32 if dtype == "f32" else np.float64
    for n in ("x", "r", "d"):
        a = np.load(tmp_path / "a" / f"{n}.npy")
        assert a.dtype == ft and a.shape == (min(edge ** 3, SAMPLE),) and np.isfinite(a).all()
    h = np.load(tmp_path / "a" / "history.npy")
    assert h.dtype == np.float64 and len(h) >= 2 * (2 + 7) + 1 and np.isfinite(h).all()
    assert np.abs(np.load(tmp_path / "a" / "x.npy")).max() > 0           # the solution moved off x = 0

    # same arguments -> same inputs -> the same outputs
    _bench(tmp_path / "b", edge, dtype)
    for n in names:
        np.testing.assert_array_equal(np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n))
