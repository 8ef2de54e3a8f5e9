"""bench.py's BASELINE legs end to end on the GPU (short runs): CASIA with DACP + ECDA forced on
at SNR 0 / 10 dB (configs[3]) and the mixed-corpus K-fold sweep (configs[4])."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the legs' runs keep what follows the timed steps (--full: per-kernel pass, parity block, BF16 and
# random-label legs) without the longest pieces
FULL = ("--full", "--no-cpu-baseline", "--no-data-path", "--fp32-steps", "0")
MOVED = ("parity", "fp32_mode", "bf16_mode", "random_labels", "data_path", "cpu_baseline")


def _bench(*args):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(args), cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=110)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.parametrize("snr", [0, 10])
def test_casia_forced_ecda_leg(snr):
    line = _bench(*FULL, "--flavor", "casia", "--force-ecda", "--snr", str(snr), "--steps", "6", "--warmup", "2")
    assert line["config"]["flavor"] == "casia" and line["config"]["snr_db"] == snr
    assert "configs[3]" in line["config"]["workload"]
    assert line["ecda_on_last_step"] == 1.0 and line["mask_sum_last_step"] > 1
    assert "scl_loss" in line["losses_last_step"] and line["losses_last_step"]["scl_loss"] == 0.0
    assert line["value"] > 0


def test_mixed_kfold_leg():
    line = _bench(*FULL, "--mixed", "--folds", "3", "--steps", "6", "--warmup", "3")
    assert line["config"]["flavor"] == "mixed"
    f = line["folds"]
    assert [x["fold"] for x in f] == [0, 1, 2]
    assert all(x["utterances"] == 6 * 64 and x["value"] > 0 for x in f)
    assert len({x["train_utterances"] for x in f}) > 1          # folds differ
    tot = sum(x["utterances"] for x in f) / sum(x["seconds"] for x in f)
    assert abs(line["value"] - tot) < 1e-6 * tot
    assert 2 * 64 * 100 <= f[0]["avg_valid_frames_per_step"] <= 2 * 64 * 300


def test_plain_run_is_lean_and_dumps_last_step_outputs(tmp_path):
    """Without --full the run ends with its timed steps (none of the side legs in the line), --steps
    sets their number (3 steps with events at every step: 3 timed launches of each long kernel), and
    --dump-outputs writes the last timed step's arrays as float32 .npy.  A second run with the same
    arguments writes the same bits: the inputs are seeded, the counter RNG depends on (seed, step)
    only, and the step repeats bit for bit (as tests/test_gpu_graph.py holds for replays)."""
    import numpy as np
    args = ("--gpus", "1", "--steps", "3", "--warmup", "1", "--settle-ms", "0", "--dump-outputs")
    out, again = tmp_path / "dump", tmp_path / "again"
    line = _bench(*args, str(out))
    assert line["steps"] == 3 and line["warmup"] == 1 and line["settle_steps"] == 0
    assert line["ms_per_step"] > 0 and abs(line["value"] - 64 / (line["ms_per_step"] * 1e-3)) < 1e-6 * line["value"]
    assert not [k for k in MOVED if k in line]
    for k in ("dad_encode_wp_f16", "dad_tail_ecda_w", "dad_wgrad_direct_f16_cp"):      # the timed region's own events
        assert line["kernels"][k]["timed_launches"] == 3, k
    assert "dad_optim" not in line["kernels"]                              # (the per-kernel pass did not run)
    assert "NaN" not in json.dumps(line)
    files = sorted(p.name for p in out.iterdir())
    assert files == sorted(k + ".npy" for k in line["dumped_outputs"])
    arrays = {f[:-4]: np.load(out / f) for f in files}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrays.values())
    assert all(list(arrays[k].shape) == v for k, v in line["dumped_outputs"].items())
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    for k, v in line["losses_last_step"].items():
        assert float(arrays[k][0]) == v, k
    assert arrays["z_clean"].shape == (64, 4) and arrays["z_strong"].shape == (64, 4)
    assert arrays["student_params"].shape == arrays["teacher_params"].shape == arrays["exp_avg"].shape
    assert float(arrays["msum"][0]) == line["mask_sum_last_step"]
    line2 = _bench(*args, str(again))
    assert line2["losses_last_step"] == line["losses_last_step"]
    assert sorted(p.name for p in again.iterdir()) == files
    for f in files:
        assert np.array_equal(np.load(again / f), arrays[f[:-4]]), f
