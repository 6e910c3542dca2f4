"""Cost of the per-link first-delivery counts (gs_set_link_deliveries) at 100k
peers x 1024 messages and 1M peers x 128 messages (rust preset, 5-stage links), one batch per run.

The pass is one kernel per batch. Its price is taken as the step time of run(collect=False) with
the pubsub counts and the link deliveries on minus the step with the pubsub counts alone: both
keep dense rows and their log, so the difference is the pass and nothing of the plan ("off" is
timed as well, to show what the plan costs). The yardstick is not the code under test: a
device-to-device copy of the batch's N * L * 8 key bytes (hipMemcpyAsync, HIP events) in the same process,
whose time the pass is reported against. gs_get_peer_given, the read-out pass, is timed once per
repetition around the call (kernel, zeroing, N * 3 * 8 bytes to the host). The method of
scripts/pubsub_counts_probe.py: after a warm-up run of each variant the variants alternate,
--reps repetitions each, a host clock around calls that return synchronised; median (min-max).
Prints one JSON line per shape (and appends it to --out).

  --no-warmup    for a run under rocprofv3 --kernel-trace --stats (k_linkdel's own time)"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = ("off", "pubsub", "pubsub_links", "links")


def copy_ms(nbytes, reps):
    """Median (min, max) ms of a device-to-device hipMemcpyAsync of nbytes (that much read and as
    much written), timed with HIP events on the null stream, through the HIP runtime the library
    itself loaded."""
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so")
    vp, sz = ctypes.c_void_p, ctypes.c_size_t

    def ok(rc):
        if rc:
            raise RuntimeError("HIP error %d" % rc)
    a, b, e0, e1 = vp(), vp(), vp(), vp()
    ok(hip.hipMalloc(ctypes.byref(a), sz(nbytes)))
    ok(hip.hipMalloc(ctypes.byref(b), sz(nbytes)))
    ok(hip.hipMemset(a, 0, sz(nbytes)))
    ok(hip.hipEventCreate(ctypes.byref(e0)))
    ok(hip.hipEventCreate(ctypes.byref(e1)))
    out = []
    for i in range(reps + 2):
        ok(hip.hipEventRecord(e0, None))
        ok(hip.hipMemcpyAsync(b, a, sz(nbytes), 3, None))  # hipMemcpyDeviceToDevice
        ok(hip.hipEventRecord(e1, None))
        ok(hip.hipEventSynchronize(e1))
        ms = ctypes.c_float()
        ok(hip.hipEventElapsedTime(ctypes.byref(ms), e0, e1))
        if i >= 2:  # (two warm-up copies)
            out.append(ms.value)
    for e in (e0, e1):
        hip.hipEventDestroy(e)
    hip.hipFree(a)
    hip.hipFree(b)
    return statistics.median(out), min(out), max(out)


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
            sim.set_pubsub_counts(v in ("pubsub", "pubsub_links"))
            sim.set_link_deliveries(v in ("pubsub_links", "links"))

        if not a.no_warmup:
            for v in VARIANTS:
                switch(v)
                sim.run(warm, collect=False)
        secs = {v: [] for v in VARIANTS}
        given_s, totals = [], {}
        for rep in range(a.reps):
            for v in VARIANTS:  # alternating
                sim.reset_stats()
                switch(v)
                t0 = time.perf_counter()
                sim.run(sched, collect=False)
                secs[v].append(time.perf_counter() - t0)
                if v == "pubsub_links":  # per peer the row sums are the first receipts
                    t0 = time.perf_counter()
                    given = sim.peer_given()
                    given_s.append(time.perf_counter() - t0)
                    edge, st = sim.link_deliveries(), sim.stats()
                    first = int(sim.pubsub_counts()[:, gossipsim.PUBSUB_COLS.index("first")].sum())
                    assert int(edge.sum()) == int(given.sum()) == first == st["frag_deliveries"], (edge.sum(), first, st)
                    totals = {n: int(x) for n, x in zip(gossipsim.LINK_DELIVERY_COLS, edge.sum(axis=0))}
                print("# %s rep %d %s: %.4f s" % (shape, rep, v, secs[v][-1]), file=sys.stderr, flush=True)
        med = {v: statistics.median(t) for v, t in secs.items()}
        rec = {"shape": shape, "peers": N, "messages": M, "batch": B, "nnz": sim.graph_info()[1], "seconds": secs,
               "totals": totals, "peer_given_s": given_s,
               "summary_s": {v: {"median": med[v], "min": min(t), "max": max(t)} for v, t in secs.items()},
               "pass_ms": 1e3 * (med["pubsub_links"] - med["pubsub"]), "key_bytes": N * M * 8}
        sim.close()
        if not a.no_copy:
            c = copy_ms(N * M * 8, 20)
            rec["copy_ms"] = {"median": c[0], "min": c[1], "max": c[2]}
            rec["pass_over_copy"] = rec["pass_ms"] / c[0]
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
