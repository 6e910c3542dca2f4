"""Go preset, fragmented IDONTWANT batches: the list pass against the push path.

Times the go preset with F = 8 and 15000-B messages (1875-B fragments, above
the 1000-B IDONTWANT threshold) in 128-message batches (rows of 1024 lanes),
collect=False, best of 3 after a warm-up run, at

  eager10k    10k peers, lazy gossip off
  eager100k   100k peers, lazy gossip off
  gossip100k  100k peers, lazy gossip on, a heartbeat 120 ms after each publish

once with GS_IDW_FRAG_LIST unset (the list pass, k_lpull<8, 16, true>) and
once with GS_IDW_FRAG_LIST=0 (the push path: k_scan / k_frontier / k_gossip).
Every (shape, leg) runs in a fresh child process under its own `timeout -k 10`
(the knob is read from a clean environment, and the parent never opens the
GPU); a child that fails or times out ends the probe. Prints one line per
child: ms per batch (best, and all three repeats: the run-to-run spread),
passes, us per pass, deliveries/s.

  python scripts/go_frag_probe.py [--out FILE] [--shapes eager10k,eager100k,gossip100k]
"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"eager10k": (10_000, 0, 240), "eager100k": (100_000, 0, 420), "gossip100k": (100_000, 1, 540)}
B, F, SIZE = 128, 8, 15000


def child(shape):
    sys.path.insert(0, os.path.join(ROOT, "dst-libp2p-test-node_amd"))
    import gossipsim

    N, gossip, _ = SHAPES[shape]
    kw = dict(node="go", peers=N, batch=B, fragments=F, seed=1, lazy_gossip=gossip)
    if gossip:
        # publishes are DELAY_NS apart, a whole number of heartbeats: the same offset for each
        kw["hb_phase_ns"] = (gossipsim.T0_NS + 120_000_000) % gossipsim.PeerConfig(node="go").heartbeat_ns
    sim = gossipsim.Simulator(**kw)
    sim.set_topogen_links(5, 50, 150, 40, 130)
    sim.connect_gossipsub_peers()
    sim.mesh_converge(400)
    # the first gossip-active batch of a context also pays the failed no-op proof: two warm-up batches
    for step in (0, 1):
        sim.run(gossipsim.shard_messages(step, 0, 1, B, N, SIZE), collect=False)
    runs = []
    for _ in range(3):
        sim.reset_stats()
        t0 = time.perf_counter()
        sim.run(gossipsim.shard_messages(2, 0, 1, B, N, SIZE), collect=False)
        runs.append(time.perf_counter() - t0)
    st = sim.stats()
    path = "list" if st["list_pull_batches"] and (not gossip or st["gossip_list_batches"]) else "push"
    deliv, iwant = st["deliveries"], st["gossip_iwant"]
    sim.reset_stats()
    sim.set_timing(True)
    sim.run(gossipsim.shard_messages(2, 0, 1, B, N, SIZE), collect=False)
    sim.set_timing(False)
    st = sim.stats()
    best = min(runs)
    leg = "GS_IDW_FRAG_LIST=" + os.environ.get("GS_IDW_FRAG_LIST", "unset")
    print("go_frag %-10s %-24s path %s: %.2f ms per batch (repeats %s), passes %d, %.1f us per pass, "
          "%.3g deliveries/s, iwant %d" %
          (shape, leg, path, best * 1e3, " ".join("%.2f" % (r * 1e3) for r in runs), st["relax_launches"],
           st["relax_ms"] * 1e3 / max(1, st["relax_launches"]), deliv / best, iwant), flush=True)
    sim.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child")
    ap.add_argument("--out")
    ap.add_argument("--shapes", default=",".join(SHAPES))
    a = ap.parse_args()
    if a.child:
        child(a.child)
        return 0
    lines = []
    for shape in a.shapes.split(","):
        for knob in (None, "0"):
            env = dict(os.environ)
            env.pop("GS_IDW_FRAG_LIST", None)
            if knob is not None:
                env["GS_IDW_FRAG_LIST"] = knob
            cmd = ["timeout", "-k", "10", str(SHAPES[shape][2]), sys.executable, os.path.abspath(__file__),
                   "--child", shape]
            r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
            sys.stdout.write(r.stdout)
            sys.stdout.flush()
            lines.append(r.stdout)
            if r.returncode:  # a fault, an abort or the time limit: nothing more is started
                print("go_frag %s: child exit status %d, stopping" % (shape, r.returncode), flush=True)
                return r.returncode
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.writelines(lines)
    return 0


if __name__ == "__main__":
    sys.exit(main())
