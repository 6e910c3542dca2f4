"""Cost of the per-peer delay accumulators (gs_set_peer_delay): step
time of run(on_lat=no-op) and of run(collect=False) with the switch on against the switch
off, at 100k peers x 1024 messages and 1M peers x 128 messages (rust preset, 5-stage
links). One process; after a warm-up run of each variant the variants alternate, --reps
repetitions each, timed with a host clock around calls that return synchronised; median
(min-max) per variant. For collect=False the off variant is the no-log twin, so the
difference there is the price of a logged completion plus the transpose, not of
k_peer_delay (attribute it from a kernel trace). Prints one JSON line per shape (and
appends it to --out).

  --pkg DIR      another build's gossipsim.py + libgossipsim.so (A/B of the switch-off
                 variants against a commit without the switch: use with --switch off)
  --switch       comma list of off,on
  --sinks        comma list of noop,none
  --no-warmup    for a run under rocprofv3 --kernel-trace --stats (the kernels' total
                 time then belongs to the one repetition this runs)"""
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
    ap.add_argument("--switch", default="off,on")
    ap.add_argument("--sinks", default="noop,none")
    ap.add_argument("--reps", type=int, default=3)
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
            if hasattr(sim, "set_peer_delay"):
                sim.set_peer_delay(sw == "on")
            elif sw == "on":
                raise SystemExit("this build has no gs_set_peer_delay: --switch off")

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
        completed = None
        for rep in range(a.reps):
            for k, sw in variants:  # alternating
                sim.reset_stats()
                switch(sw)
                t0 = time.perf_counter()
                run(k, sched)
                secs["%s_%s" % (k, sw)].append(time.perf_counter() - t0)
                if sw == "on":  # the accumulators hold the run's log lines
                    completed = int(sim.peer_delay()["completed"].sum())
                    assert completed == sim.stats()["deliveries"], (completed, sim.stats()["deliveries"])
                print("# %s rep %d %s_%s: %.4f s" % (shape, rep, k, sw, secs["%s_%s" % (k, sw)][-1]), file=sys.stderr,
                      flush=True)
        rec = {"shape": shape, "peers": N, "messages": M, "batch": B, "pkg": os.path.relpath(a.pkg, ROOT), "seconds": secs,
               "summary_s": {v: {"median": statistics.median(t), "min": min(t), "max": max(t)} for v, t in secs.items()}}
        if completed is not None:
            rec["completed"] = completed
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
        sim.close()


if __name__ == "__main__":
    main()
