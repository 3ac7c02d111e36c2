"""bench.py end to end on a small configuration: a plain run times exactly --steps steps,
prints only the headline line and, with --dump-outputs, writes the last timed step's results
as float32 / float64 .npy files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACTORS, BATCH, STEPS = 16, 32, 6
FULL_ONLY = ("roofline", "roofline_gather", "roofline_conv1", "roofline_conv2", "roofline_conv3", "roofline_hbm",
             "conv_iteration_alone", "probe_window", "decoupled_actors", "cpu_baseline")


def test_plain_run_line_and_dumped_outputs(dev, tmp_path):
    out_dir = tmp_path / "outputs"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
                        "--warmup", "2", "--actors", str(ACTORS), "--capacity", "4096", "--batch", str(BATCH),
                        "--settle", "8", "--dump-outputs", str(out_dir)],
                       capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == STEPS and d["full"] is False and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert not [k for k in FULL_ONLY if k in d]
    # the timed region is STEPS iterations: one update and ACTORS env steps each, ms_per_step its mean
    step_s = d["ms_per_step"] / 1e3
    assert step_s > 0
    assert d["learner_updates_per_sec"] * step_s == pytest.approx(1.0, rel=1e-2)
    assert d["value"] * step_s == pytest.approx(ACTORS, rel=1e-2)
    from reth_amd.model import DQNNetwork

    n_params = sum(v.numel() for v in DQNNetwork((4, 84, 84), 6).state_dict().values())
    want = {"q_network_params": [n_params], "learner_abs_td": [BATCH], "learner_batch_indices": [BATCH],
            "learner_is_weights": [BATCH], "actor_actions": [ACTORS], "actor_rewards": [ACTORS],
            "actor_dones": [ACTORS]}
    assert d["outputs_dumped"] == want
    assert sorted(os.listdir(out_dir)) == sorted(k + ".npy" for k in want)
    arrays = {k: np.load(out_dir / (k + ".npy"), allow_pickle=False) for k in want}
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    for k, a in arrays.items():
        assert a.dtype in (np.float32, np.float64) and list(a.shape) == want[k] and np.isfinite(a).all(), k
    assert (arrays["learner_abs_td"] >= 0).all() and arrays["learner_abs_td"].any()
    idx = arrays["learner_batch_indices"]
    assert ((idx >= 0) & (idx < 4096) & (idx == np.round(idx))).all()
    assert (arrays["learner_is_weights"] > 0).all() and arrays["learner_is_weights"].max() <= 1.0 + 1e-12
    assert set(np.unique(arrays["actor_actions"])) <= set(range(6))
    assert np.abs(arrays["q_network_params"]).max() > 0
