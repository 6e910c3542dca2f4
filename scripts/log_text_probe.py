"""Arrival-log throughput probe: the host writer path
(run(on_lat=...) feeding LogStream.write_lat) against the device formatter
(gs_run_log with a callback that fwrites), both into /dev/null, at 100k peers x
1024 messages and 1M peers x 128 messages (rust preset, 5-stage links). One
process; after a warm-up run of each path the paths alternate, --reps
repetitions each, timed with a host clock around calls that return synchronised.
Also the latency stream alone (run(on_lat=no-op)), the rate the formatter must
leave unchanged. Prints one JSON line per shape (and appends it to --out).

  --pkg DIR     another build's gossipsim.py + libgossipsim.so (A/B against a
                commit without gs_run_log: use with --paths noop)
  --paths       comma list of host,text,noop,part
  --parts P     the path `part`: gs_run_partitioned_log over P loop-back parts on this
                GPU (P contexts, every part's text through the one host link), against
                `text` in the same process
  --no-warmup   for a run under rocprofv3 --kernel-trace --stats (the kernels'
                total time then belongs to the bytes this prints)"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINK_GBS = 63.0  # PCIe Gen5 x16, one direction


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pkg", default=os.path.join(ROOT, "dst-libp2p-test-node_amd"))
    ap.add_argument("--shapes", default="100000x1024,1000000x128")
    ap.add_argument("--paths", default="host,text,noop")
    ap.add_argument("--parts", type=int, default=0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--chunk-mb", type=int, default=0)
    ap.add_argument("--no-warmup", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    sys.path.insert(0, a.pkg)
    import gossipsim
    paths = a.paths.split(",")
    if a.parts and "part" not in paths:
        paths.append("part")
    libc = ctypes.CDLL(None)
    libc.fopen.restype = ctypes.c_void_p
    libc.fopen.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    libc.fwrite.restype = ctypes.c_size_t
    libc.fwrite.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p]
    libc.fclose.argtypes = [ctypes.c_void_p]
    null = libc.fopen(b"/dev/null", b"w")

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
        tot = {"bytes": 0, "lines": 0}

        def host(s):
            log = gossipsim.LogStream(sim.cfg, "/dev/null")
            r = sim._schedule(s)
            sim.run(s, collect=False, block_msgs=16,
                    on_lat=lambda first, v: log.write_lat(r[first:first + v.shape[0]], v))
            log.close()

        def text(s):
            def cb(user, first, n, txt, nbytes, lines):
                libc.fwrite(txt, 1, nbytes, null)
                tot["bytes"] += nbytes
                tot["lines"] += lines

            fn = gossipsim.TEXT_FN(cb)
            r = sim._schedule(s)
            sim.log_text_reset()
            sim._check(gossipsim.lib().gs_run_log(sim.ctx, r, len(r), fn, None, a.chunk_mb << 20))

        def noop(s):
            sim.run(s, collect=False, block_msgs=16, on_lat=lambda first, v: None)

        psims, comm = [], None
        if "part" in paths:
            t0 = time.perf_counter()
            for i in range(a.parts):
                ps = gossipsim.Simulator(peers=N, batch=B, seed=1)
                ps.set_topogen_links(5, 50, 150, 40, 130)
                ps.connect_gossipsub_peers()
                ps.mesh_converge(400)
                ps.set_partition(a.parts, i)
                psims.append(ps)
            comm = gossipsim.Comm(local_parts=a.parts)
            print("# %s: %d parts' graphs and meshes in %.1f s" % (shape, a.parts, time.perf_counter() - t0),
                  file=sys.stderr, flush=True)

        def part(s):
            def cb(user, first, n, txt, nbytes, lines):
                libc.fwrite(txt, 1, nbytes, null)
                tot["bytes"] += nbytes
                tot["lines"] += lines

            fn = gossipsim.TEXT_FN(cb)
            r = sim._schedule(s)
            arr = (ctypes.c_void_p * len(psims))(*[x.ctx for x in psims])
            for x in psims:
                x.log_text_reset()
            rc = gossipsim.lib().gs_run_partitioned_log(arr, len(psims), comm.h, r, len(r), fn, None, a.chunk_mb << 20)
            if rc:
                raise gossipsim.GossipSimError(rc, gossipsim.lib().gs_last_error(psims[0].ctx).decode())

        fns = {"host": host, "text": text, "noop": noop, "part": part}
        if not a.no_warmup:
            for p in paths:
                fns[p](warm)
        secs = {p: [] for p in paths}
        for rep in range(a.reps):
            for p in paths:  # alternating
                tot["bytes"] = tot["lines"] = 0
                sim.reset_stats()
                for x in psims:
                    x.reset_stats()
                t0 = time.perf_counter()
                fns[p](sched)
                secs[p].append(time.perf_counter() - t0)
                if p == "part":
                    part_tot = dict(tot)
                    assert sum(x.stats()["deliveries"] for x in psims) == part_tot["lines"]
                else:
                    lines = sim.stats()["deliveries"]
                if p == "text":
                    text_tot = dict(tot)
                print("# %s rep %d %s: %.3f s" % (shape, rep, p, secs[p][-1]), file=sys.stderr, flush=True)
        if paths == ["part"]:
            lines = part_tot["lines"]
        rec = {"shape": shape, "peers": N, "messages": M, "batch": B, "lines": int(lines), "seconds": secs}
        for p in paths:
            rec[p + "_lines_per_s"] = {"median": lines / statistics.median(secs[p]), "min": lines / max(secs[p]),
                                       "max": lines / min(secs[p])}
        if "text" in paths:
            rec["text_bytes"] = text_tot["bytes"]
            rec["text_lines"] = text_tot["lines"]
            gbs = text_tot["bytes"] / statistics.median(secs["text"]) / 1e9
            rec["text_GBps"] = gbs
            rec["text_link_fraction"] = gbs / LINK_GBS
        if "part" in paths:
            rec["parts"] = a.parts
            rec["part_bytes"] = part_tot["bytes"]
            rec["part_lines"] = part_tot["lines"]
            t = secs["part"]
            rec["part_GBps"] = {"median": part_tot["bytes"] / statistics.median(t) / 1e9,
                                "min": part_tot["bytes"] / max(t) / 1e9, "max": part_tot["bytes"] / min(t) / 1e9}
        if "text" in paths:
            t = secs["text"]
            rec["text_GBps_range"] = {"min": text_tot["bytes"] / max(t) / 1e9, "max": text_tot["bytes"] / min(t) / 1e9}
        if "text" in paths and "host" in paths:
            rec["speedup_median"] = statistics.median(secs["host"]) / statistics.median(secs["text"])
            rec["speedup_worst"] = min(secs["host"]) / max(secs["text"])
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
        if comm is not None:
            comm.close()
        for x in psims:
            x.close()
        sim.close()
    libc.fclose(null)


if __name__ == "__main__":
    main()
