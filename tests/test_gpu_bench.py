"""bench.py's two kinds of run on small tiles: a plain run prints the headline line and nothing it does not need; --full adds the legs
that take runs of their own (here without the CPU baseline and the live PMC passes, which only the full-size line times)."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--steps", "3", "--warmup", "2", "--width", "640", "--height", "360", "--focal", "500"]
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("two_steps_in_flight", "dropin", "cpu_baseline")


def _line(tmp_path, *extra):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    with socket.socket() as s:          # --force-dist's store (bench.py would otherwise take a fixed port)
        s.bind(("127.0.0.1", 0))
        env["MASTER_PORT"] = str(s.getsockname()[1])
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + list(extra), cwd=str(tmp_path), env=env,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-3000:]
    return json.loads(lines[0])


def test_plain_run_prints_the_headline_only(gpu, tmp_path):
    d = _line(tmp_path, "--dump-outputs", str(tmp_path / "dump"))
    assert all(k in d for k in HEADLINE), d.keys()
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["steps"] == 3 and d["warmup"] == 2 and d["higher_is_better"] is True
    assert d["unit"] == "Mpix/s" and d["dtype"] == "f32"
    # the figures of the warm-up's serialised step and of the timed region itself stay; the side legs do not run
    assert d["roofline"]["kernel"] and d["kernels_ms_one_step"]
    assert not any(k in d for k in FULL_ONLY), d.keys()
    assert "host_enqueue_ms_per_pair" not in d["config"] and d["preflight"]["after_idle_Mpix_s"] is None
    assert d["dump_outputs"]["files"] == 2 and sorted(os.listdir(tmp_path / "dump")) == ["pair0_mask.npy", "pair0_mosaic.npy"]


def test_full_run_adds_the_side_legs(gpu, tmp_path):
    d = _line(tmp_path, "--full", "--no-cpu-baseline", "--no-live-traffic")
    assert all(k in d for k in HEADLINE), d.keys()
    assert d["value"] > 0 and d["two_steps_in_flight"]["identical_mosaics"] is True
    assert d["dropin"]["literal_device_f32"]["equals_fused"] is True and d["dropin"]["literal_host_f32"]["equals_fused"] is True
    assert d["config"]["host_enqueue_ms_per_pair"] > 0 and d["preflight"]["after_idle_Mpix_s"] > 0
    assert "cpu_baseline" not in d


def test_plain_run_of_the_gather_path_keeps_what_ran(gpu, tmp_path):
    """--force-dist: the N > 1 path at world 1 over RCCL.  A plain run reports the gather it ran but times none of multi_gpu's legs."""
    d = _line(tmp_path, "--force-dist", "--pairs", "2")
    assert d["value"] > 0 and d["config"]["pairs_per_gpu"] == 2
    mg = d["multi_gpu"]
    assert mg["rccl_ranks"] == 1 and mg["gather"] == "chunk" and mg["gather_backend"] == "torch" and mg["send_bytes_per_rank"] > 0
    assert not any(k in mg for k in ("without_gather_Mpix_s", "gather_alone_ms", "root_gather_Mpix_s")), mg
