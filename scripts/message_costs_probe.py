"""Cost of the per-message cost table (gs_set_message_costs) at 100k peers x 1024
messages and 1M peers x 128 messages (rust preset, 5-stage links), one batch per run, beside the
per-peer pubsub counts' passes over the same keys.

Both switches keep dense rows and their log, so the plan is the same with either or both on. The
message cost pass is taken as the step time of run(collect=False) with both switches on minus the
step with the pubsub counts alone, and the pubsub passes as both minus the message costs alone
("off" is timed as well, to show what the plan costs). The yardstick is not the code under test: a
device-to-device copy of the batch's N * L * 8 key bytes (hipMemcpyAsync, HIP events) in the same
process. The method of scripts/link_deliveries_probe.py: after a warm-up run of each variant the
variants alternate, --reps repetitions each, a host clock around calls that return synchronised;
median (min-max). Prints one JSON line per shape (and appends it to --out).

  --no-warmup    for a run under rocprofv3 --kernel-trace --stats (the kernels' own times)"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
VARIANTS = ("off", "pubsub", "costs", "pubsub_costs")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pkg", default=os.path.join(ROOT, "dst-libp2p-test-node_amd"))
    ap.add_argument("--shapes", default="100000x1024,1000000x128")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-warmup", action="store_true")
    ap.add_argument("--no-copy", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    sys.path.insert(0, a.pkg)
    import gossipsim
    from link_deliveries_probe import copy_ms

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

        def switch(v):  # (outside the timed region: enabling allocates and zeroes)
            sim.set_pubsub_counts(v in ("pubsub", "pubsub_costs"))
            sim.set_message_costs(v in ("costs", "pubsub_costs"))

        if not a.no_warmup:
            for v in VARIANTS:
                switch(v)
                sim.run(warm, collect=False)
        secs = {v: [] for v in VARIANTS}
        totals = {}
        for rep in range(a.reps):
            for v in VARIANTS:  # alternating
                sim.reset_stats()
                switch(v)
                t0 = time.perf_counter()
                sim.run(sched, collect=False)
                secs[v].append(time.perf_counter() - t0)
                if v == "pubsub_costs":  # the two reductions of the same events agree
                    mc = sim.message_costs().astype("int64").sum(axis=0)
                    ps = sim.pubsub_counts().astype("int64").sum(axis=0)
                    st = sim.stats()
                    assert mc[0] == ps[0] and mc[1] == ps[1] and mc[2] == ps[2] == st["frag_deliveries"], (mc, ps, st)
                    assert mc[4] == ps[4] and mc[5] == ps[5] and mc[6] == ps[6] == ps[7], (mc, ps)
                    totals = {n: int(x) for n, x in zip(gossipsim.MESSAGE_COST_COLS, mc)}
                print("# %s rep %d %s: %.4f s" % (shape, rep, v, secs[v][-1]), file=sys.stderr, flush=True)
        med = {v: statistics.median(t) for v, t in secs.items()}
        rec = {"shape": shape, "peers": N, "messages": M, "batch": B, "seconds": secs, "totals": totals,
               "summary_s": {v: {"median": med[v], "min": min(t), "max": max(t)} for v, t in secs.items()},
               "costs_pass_ms": 1e3 * (med["pubsub_costs"] - med["pubsub"]),
               "pubsub_pass_ms": 1e3 * (med["pubsub_costs"] - med["costs"]), "key_bytes": N * M * 8}
        sim.close()
        if not a.no_copy:
            c = copy_ms(N * M * 8, 20)
            rec["copy_ms"] = {"median": c[0], "min": c[1], "max": c[2]}
            rec["costs_pass_over_copy"] = rec["costs_pass_ms"] / c[0]
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
