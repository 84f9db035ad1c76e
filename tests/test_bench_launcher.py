"""CPU: bench.py's multi-rank path.  `python bench.py --gpus 2` must start its two ranks itself (the driver invokes it
that way) and, started under torch.distributed.run, use the ranks it is given; both run the same launcher / barrier /
MAX-over-ranks / one-JSON-line code the GPU benchmark runs, with the step stubbed out (--stub-cpu, gloo backend)."""
import json
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]


def _line(stdout):
    lines = [ln for ln in stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, stdout
    return json.loads(lines[0])


def test_bench_self_launches_two_ranks():
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1",
                        "--repeats", "2", "--stub-cpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    j = _line(r.stdout)
    assert j["n_gpus"] == 2 and j["steps"] == 3 and j["warmup"] == 1 and j["valid"] is False
    assert j["scaling"] == "weak" and j["config"]["parallelism"] == "replicas x2" and len(j["repeats"]["ms_per_step_each"]) == 2
    # 2 ranks x 3 steps of >= 2 ms each
    assert j["ms_per_step"] >= 2.0 and abs(j["value"] - 2 * 3 / (j["ms_per_step"] * 3 / 1e3)) < 1e-2 * j["value"]


def test_bench_under_torch_distributed_run():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", str(port), str(ROOT / "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "0",
           "--repeats", "1", "--stub-cpu"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert _line(r.stdout)["n_gpus"] == 2


def test_single_rank_stub():
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--steps", "2", "--warmup", "0", "--repeats", "3",
                        "--stub-cpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    j = _line(r.stdout)
    assert j["n_gpus"] == 1 and "roofline" not in j and "cpu_baseline" not in j


def test_full_option_keeps_the_headline():
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--steps", "2", "--warmup", "1", "--full", "--stub-cpu"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    j = _line(r.stdout)
    assert j["steps"] == 2 and j["warmup"] == 1 and j["unit"] == "volumes/s" and j["higher_is_better"] is True


def test_dump_outputs_writes_the_last_step(tmp_path):
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--steps", "2", "--warmup", "0", "--stub-cpu",
                        "--dump-outputs", str(tmp_path / "out")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    j = _line(r.stdout)
    assert j["steps"] == 2 and j["repeats"]["n"] == 1 and len(j["repeats"]["ms_per_step_each"]) == 1
    import numpy as np
    a = np.load(tmp_path / "out" / "inputs_embeds.npy")
    assert a.dtype == np.float32 and a.shape == (8,)


def test_dump_outputs_samples_rows_within_the_budget(tmp_path):
    import numpy as np
    import torch
    sys.path.insert(0, str(ROOT))
    import bench
    out = torch.arange(4 * 1024 * 4096, dtype=torch.float32).reshape(4, 1024, 4096).to(torch.bfloat16)
    bench.dump_outputs(tmp_path, out, rank=1, world=2)
    a = np.load(tmp_path / "inputs_embeds_rank1.npy")
    rows = np.load(tmp_path / "inputs_embeds_rank1_rows.npy")
    assert a.dtype == np.float32 and rows.dtype == np.float64
    assert a.nbytes + rows.nbytes <= bench.DUMP_BYTES // 2 and a.shape[1] == 4096 and len(rows) == a.shape[0] > 1000
    assert np.all(np.diff(rows) > 0)
    np.testing.assert_array_equal(a, out.reshape(-1, 4096)[torch.from_numpy(rows).long()].float().numpy())
    bench.dump_outputs(tmp_path / "again", out, rank=1, world=2)  # the sample is fixed: the same rows every time
    assert np.array_equal(np.load(tmp_path / "again" / "inputs_embeds_rank1_rows.npy"), rows)
