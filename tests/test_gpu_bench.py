"""bench.py on the GPU box (`-m gpu`). A plain one-GPU run times the headline
only and `--dump-outputs` writes the last timed step's results. `--gpus 2` launches two
ranks itself (no torchrun); on a box with fewer GPUs than ranks they share
the device and reduce their timing / counter scalars over gloo. Each rank
simulates its own message shard (message sharding, no data-path collective),
so the line's deliveries are 2 x (messages per rank) x (peers - 1)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_plain_run_dumps_last_step(tmp_path):
    """A plain run measures the headline only (the --full entries stay null)
    and --dump-outputs writes the last timed step's results: equal to the same
    schedule on the CPU oracle bit for bit, every peer kept at this size."""
    import numpy as np
    import gossipsim
    import oracle
    N, B, K, W = 3001, 16, 2, 1
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--peers", str(N), "--batch", str(B),
           "--steps", str(K), "--warmup", str(W), "--dump-outputs", str(tmp_path / "dump")]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    line = json.loads([x for x in out.stdout.splitlines() if x.startswith("{")][-1])
    assert line["steps"] == K and line["deliveries"] == K * B * (N - 1) and line["ms_per_step"] > 0
    assert line["full"] is False
    for k in ("configs_1gpu", "cpu_baseline", "with_output", "at_second_size"):
        assert line[k] is None, k
    assert line["gossip"]["check"] is None
    lat, hops, peers = (np.load(str(tmp_path / "dump" / (n + ".npy"))) for n in ("latency_ns", "hops", "peers"))
    assert lat.dtype == np.float64 and hops.dtype == np.float32 and lat.shape == hops.shape == (B, N)
    assert (peers == np.arange(N)).all()
    t, pub, size = gossipsim.shard_messages(W + K - 1, 0, 1, B, N, 15000)
    ref = oracle.simulate(oracle.params(peers=N, seed=1), 5, (50, 150, 40, 130), sched=(t, pub, size))
    assert (ref["t_complete"] != gossipsim.UNDELIVERED).all()
    assert (lat == (ref["t_complete"] - t[:, None]).astype(np.float64)).all()
    assert (hops == ref["hops"]).all()


@pytest.mark.gpu
def test_bench_two_ranks_message_sharded():
    N, B, K = 20_000, 64, 2
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--peers", str(N), "--batch", str(B),
           "--steps", str(K), "--warmup", "1", "--configs", "0", "--cpu-seconds", "0", "--also-peers", "0",
           "--gossip-check", "0", "--output-steps", "0"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    line = json.loads([x for x in out.stdout.splitlines() if x.startswith("{")][-1])
    assert line["n_gpus"] == 2 and line["config"]["parallelism"] == "msg-shard2"
    assert line["dist"]["ranks"] == 2
    assert line["deliveries"] == 2 * K * B * (N - 1)
    assert line["value"] > 0 and line["gossip"]["fallback_batches"] == 0
