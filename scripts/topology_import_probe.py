"""Cost of importing a graph (gs_set_topology, gs_set_topology_dials) beside
building one. The project's usual method: one process; after a warm-up call of each variant the
variants alternate, --reps repetitions each, timed with a host clock around the call, which
returns synchronised; median (min-max) per variant. Every timed import is checked: its CSR is the
built graph's (shape built) or tests/topo_ref.py's (shape hub). One JSON line per shape (appended
to --out).

  built   PEERS peers (default 1M), the builder's own graph: build | csr | dials. The dials are
          the F_OUT entries of the built CSR, shuffled once.
  hub     100k peers on a lattice (v dials v+1..v+5) plus 64 peers of 256 connections each, dialed
          by them: dials with a wave per long row | dials-thread with GS_IMPORT_WAVE_ROWS=0 (a
          thread per row for those rows too).
  --no-warmup --reps 1   for a run under rocprofv3 --kernel-trace --stats"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "dst-libp2p-test-node_amd"), os.path.join(ROOT, "tests")]


def hub_graph():
    n, hubs = 100000, 64
    v = np.arange(n, dtype=np.int64)
    d = [np.repeat(v, 5)]
    t = [((v[:, None] + np.arange(1, 6)) % n).reshape(-1)]
    rng = np.random.default_rng(1)
    for h in range(hubs):
        d.append(np.full(256, n + h))
        t.append(rng.choice(n, 256, replace=False))
    return n + hubs, np.concatenate(d).astype(np.uint32), np.concatenate(t).astype(np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="built,hub")
    ap.add_argument("--peers", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-warmup", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import gossipsim
    import topo_ref

    for shape in a.shapes.split(","):
        if shape == "built":
            N = a.peers
            sim = gossipsim.Simulator(peers=N, seed=1, batch=8)
            sim.connect_gossipsub_peers()
            row, col, flags = sim.csr()
            d, t = topo_ref.csr_to_dials(row, col, flags)
            perm = np.random.default_rng(1).permutation(len(d))
            d, t = np.ascontiguousarray(d[perm]), np.ascontiguousarray(t[perm])
            calls = {"build": sim.connect_gossipsub_peers, "csr": lambda: sim.set_topology(row, col, flags),
                     "dials": lambda: sim.set_dials(d, t)}
        else:
            N, d, t = hub_graph()
            row, col, flags = topo_ref.dials_to_csr(N, d, t)
            sim = gossipsim.Simulator(peers=N, seed=1, batch=8)

            def dials(wave):
                os.environ["GS_IMPORT_WAVE_ROWS"] = "1" if wave else "0"
                sim.set_dials(d, t)
            calls = {"dials": lambda: dials(True), "dials-thread": lambda: dials(False)}
        if not a.no_warmup:
            for f in calls.values():
                f()
        secs = {k: [] for k in calls}
        for rep in range(a.reps):
            for k, f in calls.items():  # alternating
                t0 = time.perf_counter()
                f()
                secs[k].append(time.perf_counter() - t0)
                got = sim.csr()
                assert (got[0] == row).all() and (got[1] == col).all() and (got[2] == flags & 1).all(), k
                print("# %s rep %d %s: %.4f s" % (shape, rep, k, secs[k][-1]), file=sys.stderr, flush=True)
        rec = {"shape": shape, "peers": N, "dials": int(len(d)), "entries": int(len(col)),
               "max_degree": sim.graph_info()[2], "seconds": secs,
               "summary_s": {k: {"median": statistics.median(x), "min": min(x), "max": max(x)} for k, x in secs.items()}}
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
        sim.close()
        os.environ.pop("GS_IMPORT_WAVE_ROWS", None)


if __name__ == "__main__":
    main()
