"""Cost of the per-peer pubsub event counts (gs_set_pubsub_counts): step
time of run(collect=False) and of run(on_lat=no-op) with the switch on against both switches
off and against gs_set_traffic on, at 100k peers x 1024 messages and 1M peers x 128 messages
(rust preset, 5-stage links). The method of scripts/peer_delay_probe.py: one process; after
a warm-up run of each variant the variants alternate, --reps repetitions each, timed with a
host clock around calls that return synchronised; median (min-max) per variant. With either
switch on a batch keeps dense rows and its log, so against "off" the difference holds the
price of those as well as the passes' (attribute it from a kernel trace). Prints one JSON
line per shape (and appends it to --out).

  --switch       comma list of off,pubsub,traffic
  --sinks        comma list of none,noop
  --no-warmup    for a run under rocprofv3 --kernel-trace --stats"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pkg", default=os.path.join(ROOT, "dst-libp2p-test-node_amd"))
    ap.add_argument("--shapes", default="100000x1024,1000000x128")
    ap.add_argument("--switch", default="off,pubsub,traffic")
    ap.add_argument("--sinks", default="none,noop")
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--no-warmup", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    sys.path.insert(0, a.pkg)
    import gossipsim
    variants = [(k, sw) for k in a.sinks.split(",") for sw in a.switch.split(",")]

    for shape in a.shapes.split(","):
        N, M = (int(x) for x in shape.split("x"))
        B = min(M, 1024)
        t0 = time.perf_counter()
        sim = gossipsim.Simulator(peers=N, batch=B, seed=1)
        sim.set_topogen_links(5, 50, 150, 40, 130)
        sim.connect_gossipsub_peers()
        sim.mesh_converge(400)
        print("# %s: graph and mesh in %.1f s" % (shape, time.perf_counter() - t0), file=sys.stderr, flush=True)
        sched = gossipsim.shard_messages(0, 0, 1, M, N, 15000)
        warm = tuple(x[:min(M, 64)] for x in sched)

        def switch(sw):  # (outside the timed region: enabling allocates and zeroes)
            sim.set_pubsub_counts(sw == "pubsub")
            sim.set_traffic(sw == "traffic")

        def run(sink, s):
            if sink == "noop":
                sim.run(s, collect=False, block_msgs=16, on_lat=lambda first, v: None)
            else:
                sim.run(s, collect=False)

        if not a.no_warmup:
            for k, sw in variants:
                switch(sw)
                run(k, warm)
        secs = {"%s_%s" % v: [] for v in variants}
        sums = {}
        for rep in range(a.reps):
            for k, sw in variants:  # alternating
                sim.reset_stats()
                switch(sw)
                t0 = time.perf_counter()
                run(k, sched)
                secs["%s_%s" % (k, sw)].append(time.perf_counter() - t0)
                if sw == "pubsub":  # the totals are the run's own counters (frozen mesh)
                    c, st = sim.pubsub_counts().sum(axis=0), sim.stats()
                    assert int(c[0]) == int(c[1]) == st["relaxations"] and int(c[2]) == st["frag_deliveries"], (c, st)
                    sums = {n: int(v) for n, v in zip(gossipsim.PUBSUB_COLS, c)}
                print("# %s rep %d %s_%s: %.4f s" % (shape, rep, k, sw, secs["%s_%s" % (k, sw)][-1]), file=sys.stderr,
                      flush=True)
        rec = {"shape": shape, "peers": N, "messages": M, "batch": B, "seconds": secs, "totals": sums,
               "summary_s": {v: {"median": statistics.median(t), "min": min(t), "max": max(t)} for v, t in secs.items()}}
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
        sim.close()


if __name__ == "__main__":
    main()
