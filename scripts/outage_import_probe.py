"""Cost of a caller's outages (gs_set_outages, DESIGN.md §2.8 "A caller's outages") beside the churn
draw. The project's usual method: one process, the variants alternate, --reps repetitions each,
timed with a host clock around the call, which returns synchronised; median (min-max) per variant.
One JSON line per size (appended to --out).

  import     gs_set_outages of --intervals intervals (default peers / 10), one per sampled peer, shuffled
  lookup     gs_get_offline of epochs 1..--epochs from the imported rows (k_outage_range)
  draw       the same call from the draw of (churn_ppm 30000, churn_down 6) (k_offline_range), after
             gs_clear_outages

The host times of lookup and draw are mostly the copy of the bitsets to the host; the two kernels'
own times come from a run under rocprofv3 --kernel-trace --stats (a run of its own). Every lookup
is checked: its offline cells are the intervals' lengths inside the range."""
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
    ap.add_argument("--peers", default="1000000")
    ap.add_argument("--intervals", type=int, default=0)
    ap.add_argument("--epochs", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import gossipsim

    for N in (int(x) for x in a.peers.split(",")):
        n = a.intervals or N // 10
        E = a.epochs
        sim = gossipsim.Simulator(peers=N, seed=1, churn_ppm=30000, churn_down=6)
        rng = np.random.default_rng(1)
        peer = rng.choice(N, n, replace=False).astype(np.uint32)
        h_from = rng.integers(1, E, n).astype(np.uint32)
        h_to = (h_from + rng.integers(1, 9, n)).astype(np.uint32)
        cells = int((np.minimum(h_to, E + 1) - h_from).sum())
        secs = {"import": [], "lookup": [], "draw": []}
        draw_cells = None
        for rep in range(a.reps):
            t0 = time.perf_counter()
            sim.set_outages(peer, h_from, h_to)
            secs["import"].append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            tab = sim.offline(1, E)
            secs["lookup"].append(time.perf_counter() - t0)
            assert int(tab.sum()) == cells, (int(tab.sum()), cells)
            sim.clear_outages()
            t0 = time.perf_counter()
            tab = sim.offline(1, E)
            secs["draw"].append(time.perf_counter() - t0)
            assert draw_cells in (None, int(tab.sum()))
            draw_cells = int(tab.sum())
            print("# %d rep %d: import %.4f s lookup %.4f s draw %.4f s" % (
                N, rep, secs["import"][-1], secs["lookup"][-1], secs["draw"][-1]), file=sys.stderr, flush=True)
        rec = {"peers": N, "intervals": n, "epochs": E, "offline_cells_import": cells, "offline_cells_draw": draw_cells,
               "seconds": secs,
               "summary_s": {k: {"median": statistics.median(x), "min": min(x), "max": max(x)} for k, x in secs.items()}}
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
        sim.close()


if __name__ == "__main__":
    main()
