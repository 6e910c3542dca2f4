"""Cost of the mesh event counts (gs_set_mesh_events): time of mesh_converge
with the switch on against off at three shapes (rust preset, 5-stage links): a config #3-shaped
churn converge (100k peers, 1 % churn, 400 epochs), a frozen converge at 100k peers and one at
1M. The method of scripts/pubsub_counts_probe.py: one process; after a warm-up converge of each
variant the variants alternate, --reps repetitions each, timed with a host clock around the
call, which returns synchronised; median (min-max) per variant. With the switch on every timed
repetition checks the identities between the per-peer columns and the series. Prints one JSON
line per shape (and appends it to --out).

  --pkg          the package directory to load (another build's, for switch-off comparisons:
                 a build without the switch runs with --switch off)
  --switch       comma list of off,on
  --no-warmup    for a run under rocprofv3 --kernel-trace --stats"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {
    "churn100k": (dict(peers=100000, churn_ppm=10000, churn_down=10, churn_horizon=16), 400),
    "frozen100k": (dict(peers=100000), 400),
    "frozen1m": (dict(peers=1000000), 400),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pkg", default=os.path.join(ROOT, "dst-libp2p-test-node_amd"))
    ap.add_argument("--shapes", default="churn100k,frozen100k,frozen1m")
    ap.add_argument("--switch", default="off,on")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-warmup", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    sys.path.insert(0, a.pkg)
    import gossipsim
    variants = a.switch.split(",")

    for shape in a.shapes.split(","):
        kw, max_hb = SHAPES[shape]
        t0 = time.perf_counter()
        sim = gossipsim.Simulator(batch=8, seed=1, **kw)
        sim.set_topogen_links(5, 50, 150, 40, 130)
        sim.connect_gossipsub_peers()
        print("# %s: graph in %.1f s" % (shape, time.perf_counter() - t0), file=sys.stderr, flush=True)

        def switch(sw):  # (outside the timed region: enabling allocates)
            if sw == "on" or "on" in variants:
                sim.set_mesh_events(sw == "on")

        if not a.no_warmup:
            for sw in variants:
                switch(sw)
                sim.mesh_converge(max_hb)
        secs = {sw: [] for sw in variants}
        sums, epochs = {}, 0
        for rep in range(a.reps):
            for sw in variants:  # alternating
                switch(sw)
                t0 = time.perf_counter()
                epochs = sim.mesh_converge(max_hb)
                secs[sw].append(time.perf_counter() - t0)
                if sw == "on":
                    ev, se = sim.mesh_events().sum(axis=0), sim.mesh_series()
                    st = se.sum(axis=0)
                    assert len(se) == epochs + 1, (len(se), epochs)
                    assert int(ev[0]) == int(ev[1]) == int(st[6]), (ev, st)
                    assert int(ev[2]) == int(ev[3]) == int(st[8] + st[7]), (ev, st)
                    assert [int(x) for x in ev[4:]] == [int(st[10]), int(st[11]), int(st[9])], (ev, st)
                    assert int(se[-1, 5]) == int(sim.mesh()[1].astype("uint64").sum())
                    sums = {n: int(v) for n, v in zip(gossipsim.MESH_SERIES_COLS[6:], st[6:])}
                print("# %s rep %d %s: %.4f s" % (shape, rep, sw, secs[sw][-1]), file=sys.stderr, flush=True)
        rec = {"shape": shape, "peers": kw["peers"], "max_heartbeats": max_hb, "epochs": epochs, "seconds": secs,
               "series_sums": sums, "pkg": os.path.relpath(a.pkg, ROOT),
               "summary_s": {v: {"median": statistics.median(t), "min": min(t), "max": max(t)}
                             for v, t in secs.items()}}
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
        sim.close()


if __name__ == "__main__":
    main()
