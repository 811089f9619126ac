"""GPU: bench.py end to end on a small shard.  A plain run measures the headline alone (set-up, warm-up, timed steps, the line);
`--full` adds the other legs after the timed steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import topk_oracle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOCS, STEPS = 2048, 3

# what only --full measures, as keys of the full report
FULL_ONLY = ("mfma_ceiling", "topk_parity", "parity_max_rel_err_vs_oracle_sample", "forced_collective_1rank", "cpu_baseline",
             "reference_on_this_gpu", "embed_head", "dropin_from_host_lists", "embed_and_score_1k_pages",
             "resident_colqwen2_page_geometry", "resident_short_documents", "resident_width_320", "loss_step_config5",
             "embed_and_score_1k_pages_vlm_in_the_loop", "embed_and_score_1k_pages_vlm_in_the_loop_colqwen2")


def _bench(*args, env_extra=None):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "BENCH_SHARE_GPU")}
    env.update(env_extra or {})
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--docs", str(DOCS), "--steps", str(STEPS), "--warmup", "1",
           *args]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = r.stdout.strip().split("\n")
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def _check_headline(d):
    assert d["metric"] == "MaxSim (query,doc) pairs scored/sec" and d["unit"] == "pairs/s" and d["higher_is_better"] is True
    assert d["dtype"] == "bf16" and d["steps"] == STEPS and d["warmup"] == 1
    assert d["value"] == pytest.approx(4 * DOCS / (d["ms_per_step"] * 1e-3), rel=1e-4)     # pairs of one step / time of one step
    assert d["roofline"]["kernel_ms"] > 0 and d["roofline"]["bound"] == "hbm"


def test_plain_run_measures_the_headline_alone(tmp_path):
    d = _bench("--dump-outputs", str(tmp_path))
    _check_headline(d)
    assert d["summary"] == {} and "cpu_baseline" not in d and "topk_parity" not in d
    assert "stream_ceiling_gbs" not in d["roofline"]
    detail = json.load(open(os.path.join(ROOT, d["detail"])))
    assert detail["value"] == pytest.approx(d["value"], rel=1e-5)
    assert [k for k in FULL_ONLY if k in detail] == [] and detail["regimes"] == [] and "power" not in detail["roofline"]
    # the dumped outputs are the last timed step's: the top-k is the (score desc, id asc) top-k of the dumped score matrix
    scores = np.load(tmp_path / "scores.npy")
    assert scores.shape == (4, DOCS) and scores.dtype == np.float32
    want_s, want_i = topk_oracle.topk(scores, 10)
    np.testing.assert_array_equal(np.load(tmp_path / "topk_ids.npy"), want_i.astype(np.float64))
    np.testing.assert_array_equal(np.load(tmp_path / "topk_scores.npy"), want_s)


def test_full_run_adds_the_other_legs():
    d = _bench("--full", "--no-cpu-baseline", "--regimes", "8,4x40", env_extra={"BENCH_POWER_SAMPLE": "0"})
    _check_headline(d)
    assert d["roofline"]["stream_ceiling_gbs"] > 0
    assert d["topk_parity"]["ids_equal"] is True and d["topk_parity"]["k100_ids_equal"] is True
    assert d["summary"]["forced_collective_equal"] is True and d["summary"]["nq8_frac"] > 0 and d["summary"]["frac_on_zeros"] > 0
    assert "cpu_baseline" not in d                                            # --no-cpu-baseline still narrows a full run
