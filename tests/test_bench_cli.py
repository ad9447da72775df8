"""bench.py's command line: a plain run measures the headline alone, --full adds every other leg after the timed steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def parse(monkeypatch, *argv):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse_args()


def test_plain_run_leaves_out_every_leg_beside_the_headline(monkeypatch):
    a = parse(monkeypatch, "--gpus", "1", "--steps", "20", "--warmup", "5")
    assert not a.full and a.no_extras and a.no_cpu and not a.hc_only
    assert (a.steps, a.warmup, a.blocks, a.dist) == (20, 5, 1 << 20, 2)


def test_full_keeps_the_other_legs_and_their_switches(monkeypatch):
    a = parse(monkeypatch, "--full")
    assert a.full and not a.no_extras and not a.no_cpu and not a.hc_only
    a = parse(monkeypatch, "--full", "--no-cpu", "--hc-only")
    assert a.full and not a.no_extras and a.no_cpu and a.hc_only


def test_hc_only_without_full_is_refused(monkeypatch, capsys):
    with pytest.raises(SystemExit) as e:
        parse(monkeypatch, "--hc-only")
    assert e.value.code == 2 and "--full" in capsys.readouterr().err


@pytest.mark.gpu
def test_plain_run_prints_the_headline_alone(tmp_path):
    """A plain run on a small batch: one JSON line with the headline, verified, and nothing of --full in it; the dump is
    written all the same."""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--blocks", "16384", "--steps", "2",
                        "--warmup", "1", "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["full"] is False and d["verified"] is True and d["value"] > 0 and d["ms_per_step"] > 0
    assert d["steps"] == 2 and d["warmup"] == 1 and d["config"]["blocks_per_gpu"] == 16384
    assert d["cpu_baseline"] is None and d["roofline_hc"] is None
    assert d["roofline_encode"]["bit_exact_vs_cpu_reference"] is None
    assert list(d["extras"]) == ["D2-fuzzer(original/fuzzer.c)"]
    assert "decode_lane_GBps" not in d["extras"]["D2-fuzzer(original/fuzzer.c)"]
    used = np.load(tmp_path / "decode_result.npy")
    assert used.shape == (16384,) and (used > 0).all()
    assert np.load(tmp_path / "decoded_sample.npy").shape == (192, 65536)
