"""Cost of importing a mesh (gs_set_mesh, gs_set_mesh_links; DESIGN.md §2.3 "A caller's mesh")
beside converging one. The project's usual method: one process; after a warm-up call of each
variant the variants alternate, --reps repetitions each, timed with a host clock around the call,
which returns synchronised; median (min-max) per variant. The mesh is the converged one read
back (rust preset, 5-stage links 50-150 Mbit / 40-130 ms); every timed call is checked: its mesh
rows, counts and CSR flags are the converged ones. One JSON line per size (appended to --out).

  converge   gs_mesh_converge on the same graph
  ell        gs_set_mesh of mesh() with its counts
  links      gs_set_mesh_links of the links, shuffled once with random orientations
  --no-warmup --reps 1   for a run under rocprofv3 --kernel-trace --stats"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "dst-libp2p-test-node_amd")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--peers", default="100000,1000000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-warmup", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import gossipsim

    for N in (int(x) for x in a.peers.split(",")):
        sim = gossipsim.Simulator(peers=N, seed=1, batch=8)
        sim.set_topogen_links(5, 50, 150, 40, 130)
        sim.connect_gossipsub_peers()
        epochs = sim.mesh_converge()
        mesh, cnt = sim.mesh()
        flags = sim.csr()[2]
        rows = np.repeat(np.arange(N, dtype=np.uint32), cnt)
        cols = mesh[mesh != 0xFFFFFFFF]  # (row-major: each row's ids in order)
        la, lb = rows[rows < cols], cols[rows < cols]
        rng = np.random.default_rng(1)
        perm, flip = rng.permutation(len(la)), rng.integers(0, 2, len(la)).astype(bool)
        la, lb = np.ascontiguousarray(np.where(flip, lb, la)[perm]), np.ascontiguousarray(np.where(flip, la, lb)[perm])
        calls = {"converge": sim.mesh_converge, "ell": lambda: sim.set_mesh(mesh, cnt),
                 "links": lambda: sim.set_mesh_links(la, lb)}
        if not a.no_warmup:
            for f in calls.values():
                f()
        secs = {k: [] for k in calls}
        for rep in range(a.reps):
            for k, f in calls.items():  # alternating
                t0 = time.perf_counter()
                f()
                secs[k].append(time.perf_counter() - t0)
                m2, c2 = sim.mesh()
                assert (m2 == mesh).all() and (c2 == cnt).all() and (sim.csr()[2] == flags).all(), k
                print("# %d rep %d %s: %.4f s" % (N, rep, k, secs[k][-1]), file=sys.stderr, flush=True)
        rec = {"peers": N, "links": int(len(la)), "entries": int(len(flags)), "converge_epochs": epochs,
               "widest_row": int(cnt.max()), "seconds": secs,
               "summary_s": {k: {"median": statistics.median(x), "min": min(x), "max": max(x)} for k, x in secs.items()}}
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
        sim.close()


if __name__ == "__main__":
    main()
