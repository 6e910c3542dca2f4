"""A/B of list-pass shapes on the bench workload (1M peers, 1024 messages per
round, one process, interleaved rounds): each config is `batch[:ENV=VAL,...]`,
e.g.  python scripts/ab_batch.py --configs 1024 512 512:GS_LPULL_SUM=0
Every config must give the same counters; prints ms per 1024 messages and the
window-pass time (HIP events) per config."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dst-libp2p-test-node_amd"))
import gossipsim  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--peers", type=int, default=1_000_000)
ap.add_argument("--rounds", type=int, default=4)
ap.add_argument("--msgs", type=int, default=1024)
ap.add_argument("--configs", nargs="+", default=["1024", "512", "512:GS_LPULL_SUM=0"])
args = ap.parse_args()
cfgs = []
sims = {}
for c in args.configs:
    b, _, env = c.partition(":")
    env = dict(kv.split("=") for kv in env.split(",")) if env else {}
    b = int(b)
    if b not in sims:
        s = gossipsim.Simulator(peers=args.peers, batch=b, fragments=1, seed=1)
        s.set_topogen_links(5, 50, 150, 40, 130)
        s.connect_gossipsub_peers()
        s.mesh_converge()
        s.run(gossipsim.shard_messages(0, 0, 1, b, args.peers, 15000), collect=False)  # warm-up
        sims[b] = s
    cfgs.append((c, b, env))
best = {c: (1e9, 0) for c, _, _ in cfgs}
allenv = set(k for _, _, e in cfgs for k in e)
for r in range(args.rounds):
    ref = None
    for c, b, env in cfgs:
        for k in allenv:
            os.environ.pop(k, None)
        os.environ.update(env)
        s = sims[b]
        s.reset_stats()
        s.set_timing(True)
        t0 = time.perf_counter()
        s.run(gossipsim.shard_messages(r + 1, 0, 1, args.msgs, args.peers, 15000), collect=False)
        dt = time.perf_counter() - t0
        s.set_timing(False)
        st = s.stats()
        key = (st["deliveries"], st["relaxations"], st["latency_sum_ms"], st["latency_max_ms"])
        if ref is None:
            ref = key
        assert key == ref, (c, key, ref)
        if dt < best[c][0]:
            best[c] = (dt, st["relax_ms"])
        print("round %d %-24s %.2f ms (passes %.2f ms, %d launches, list batches %d)" % (
            r, c, dt * 1e3, st["relax_ms"], st["relax_launches"], st["list_pull_batches"]), flush=True)
for c, _, _ in cfgs:
    print("BEST %-24s %.2f ms  passes %.2f ms" % (c, best[c][0] * 1e3, best[c][1]))
