"""Diagnostic: where the shader clocks of k_lpull go, per pass (needs the
GS_PULL_PROF build: scripts/pull_prof.sh build). Slots: 0 skipped rows,
1 header + listed entries, 2 neighbour records -> LDS minima, 3 classify,
4 list appends, 5 sparse emit (targets, FIFO, records), 6 row state, 7 rows."""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dst-libp2p-test-node_amd"))
import gossipsim  # noqa: E402

# (GOSSIPSIM_LIB: another -DGS_PULL_PROF build, e.g. scripts/build_variant.sh's of a parent commit)
gossipsim.LIB_PATH = os.environ.get("GOSSIPSIM_LIB") or os.path.join(ROOT, "prof_build", "libgossipsim.so")
peers = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
L = gossipsim.lib()
L.gs_debug_pull_prof.argtypes = [ctypes.c_void_p]
sim = gossipsim.Simulator(peers=peers, batch=1024, fragments=1, seed=1, device=0, lazy_gossip=0)
sim.set_topogen_links(5, 50, 150, 40, 130)
sim.connect_gossipsub_peers()
sim.mesh_converge(400)
sim.run(gossipsim.shard_messages(0, 0, 1, 1024, peers, 15000), collect=False)
buf = np.zeros(32 * 8, dtype=np.uint64)
L.gs_debug_pull_prof(buf.ctypes.data)
sim.run(gossipsim.shard_messages(1, 0, 1, 1024, peers, 15000), collect=False)
L.gs_debug_pull_prof(buf.ctypes.data)
b = buf.reshape(32, 8).astype(np.float64)
names = ["skip", "entries", "records", "classify", "append", "sparse", "state"]
print("pass " + " ".join("%8s%%" % n for n in names) + "  active_rows   Gclk")
for p in range(32):
    t = b[p, :7].sum()
    if t == 0:
        continue
    print("%4d " % p + " ".join("%9.1f" % (100 * b[p, k] / t) for k in range(7)) + "  %11d %6.2f" % (int(b[p, 7]), t / 1e9))
tot = b[:, :7].sum(0)
print("all  " + " ".join("%9.1f" % x for x in 100 * tot / tot.sum()))
