"""GPU: bench.py's plain run - the headline step only, exactly --steps timed steps - and what --dump-outputs writes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_plain_run_dumps_the_last_step(tmp_path):
    """A plain run prints one JSON line with the headline keys and none of the --full legs; --dump-outputs DIR holds the last
    timed step's SR batch, losses and parameters as float32 .npy files within 64 MB, and the generator losses it wrote are the
    ones the line reports."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "MASTER_ADDR")}
    out_dir = tmp_path / "out"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "4",
                        "--dump-outputs", str(out_dir)], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    out = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in out, k
    assert out["steps"] == 3 and out["unit"] == "HR images/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
    assert out["ms_per_step"] == pytest.approx(out["timed_region_s"] * 1e3 / 3, rel=1e-9)
    assert not {"srresnet_step", "srgan_shared_d_sr_step", "roofline", "cpu_baseline"} & set(out), "a --full leg ran in a plain run"

    names = sorted(os.listdir(out_dir))
    assert {"sr.npy", "d_loss.npy", "g_params.npy", "d_params.npy", "g_loss_Adversarial.npy", "g_loss_Pixel.npy",
            "g_loss_ST.npy"} <= set(names), names
    arrs = {n[:-4]: np.load(out_dir / n) for n in names}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrs.values())
    assert sum(os.path.getsize(out_dir / n) for n in names) <= 64 << 20
    assert arrs["sr"].shape == (16, 3, 96, 96)
    for k, v in out["config"]["losses_last_step"].items():
        assert float(arrs[f"g_loss_{k}"][0]) == pytest.approx(v, rel=1e-6), k
