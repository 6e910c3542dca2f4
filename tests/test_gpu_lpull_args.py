"""The list pass's scalar arguments at their ends (gs_lpull_kernel.h, DESIGN.md
§4.6): k_lpull carries its small row-loop scalars (K, the emitted window's
slot, lane bits, source bits, stage count, pass parity, flags) packed in one
word and derives others where they are used (tshift from sb, the latency /
serialisation tables from one base and S, the written halves of the record
and count double buffers from the read ones, window starts from one hi word).
A mis-decoded or mis-derived scalar gives wrong keys, so every case here is
bit-exact against the CPU oracle on a small graph: t_complete, hops and the
eight counters, the first differing (message, peer) reported."""
import functools

import numpy as np
import pytest

import gossipsim
import oracle
from test_gpu_gossip_list import _phase
from test_gpu_parity import T0, _sched, gpu_sim

pytestmark = pytest.mark.gpu
LINKS = (50, 150, 40, 130)  # the bench's link ranges (bench.py --links, with 5 stages)
COUNTERS = ("deliveries", "frag_deliveries", "relaxations", "bytes_alg", "latency_sum_ms", "latency_max_ms",
            "messages", "gossip_iwant")
LP_KMAX = 12      # gs_lpull_kernel.h: the longest ring of destination-window lists
MAX_STAGES = 16   # gs_common.h: the largest stage count the library accepts


def _first_diff(name, got, ref):
    if np.array_equal(got, ref):
        return
    m, u = np.argwhere(got != ref)[0]
    raise AssertionError("%s differs first at (message %d, peer %d): %d, oracle %d (%d cells differ)"
                         % (name, m, u, got[m, u], ref[m, u], int((got != ref).sum())))


def _exact(sim, res, ref):
    _first_diff("t_complete", res["t_complete"], ref["t_complete"])
    _first_diff("hops", res["hops"], ref["hops"])
    st = sim.stats()
    for k in COUNTERS:
        assert st[k] == ref["stats"][k], k
    return st


def _run(p, S, links, sched, batch, on_list=True):
    """One context, the whole schedule, against the oracle; on_list: every batch took the list pass."""
    sim, _ = gpu_sim(p, S, links, batch=batch)
    ref = oracle.simulate(p, S, links, sched=sched)
    st = _exact(sim, sim.run(sched), ref)
    if on_list:
        assert st["list_pull_batches"] == st["batches"] > 0
    return sim, st, ref


@pytest.mark.parametrize("peers,msgs", [(65, 24), (1000, 24), (4097, 24), (70_000, 8)])
def test_source_bits(monkeypatch, peers, msgs):
    """7, 10, 13 and 17 source bits (sb; tshift = sb + 6 follows from it)."""
    monkeypatch.setenv("GS_REQUIRE_LPULL", "1")
    assert (peers - 1).bit_length() in (7, 10, 13, 17)
    _run(oracle.params(peers=peers, seed=81, lazy_gossip=0), 5, LINKS, _sched(msgs, peers), batch=16)


@pytest.mark.parametrize("S,links", [(1, (50, 50, 50, 50)), (MAX_STAGES, LINKS), (5, LINKS)])
def test_stage_counts(monkeypatch, S, links):
    """One stage, the most the library accepts, and the bench's five: the
    serialisation tables sit at S * S and S * S + S of the latency table."""
    monkeypatch.setenv("GS_REQUIRE_LPULL", "1")
    _run(oracle.params(peers=1000, seed=82, lazy_gossip=0), S, links, _sched(24, 1000), batch=24)


@pytest.mark.parametrize("batch,frags", [(64, 1), (512, 1), (1024, 1), (16, 3), (256, 3)])
def test_chunk_counts_and_lane_bits(monkeypatch, batch, frags):
    """Rows of 64, 512 (8 chunks) and 1024 lanes (16 chunks), 6 to 10 lane
    bits; F = 3 is a padded fragment group (4 lanes) in rows of both widths."""
    monkeypatch.setenv("GS_REQUIRE_LPULL", "1")
    N = 300
    _run(oracle.params(peers=N, seed=83, lazy_gossip=0, fragments=frags), 5, LINKS, _sched(batch, N), batch=batch)


def _ring_k(p, S, links, dmax, size=15000):
    """lpull_ring's K (gs_relax.hip) for a frozen mesh of unfragmented messages without flood
    publish and gossip: span / Delta + 2, as a float (the host takes the floor)."""
    lat, bw = oracle.topogen_links(S, *links)
    lat = lat.astype(np.float64)
    ser = oracle.wire_bytes(size, p.muxer, p.signed_msgs) * 8e9 / bw.astype(np.float64)
    delta = lat.min() + ser.min()
    adj = max(lat[x, y] + max(0.0, ser[y] - ser[x]) for x in range(S) for y in range(S))
    return (delta + adj + dmax * ser.max()) / delta + 2


@pytest.mark.parametrize("S,links,k", [(10, (100, 150, 12, 130), LP_KMAX), (1, (50, 50, 50, 50), 4)])
def test_ring_lengths(monkeypatch, S, links, k):
    """A ring at its full length (ten stages, 12 to 111 ms: the latency spread
    makes K = LP_KMAX) and the shortest ring the host ever sets up (K = 4: one
    stage; span >= 2 Delta for any links, so no batch has K = 2 or 3)."""
    monkeypatch.setenv("GS_REQUIRE_LPULL", "1")
    N = 1000
    p = oracle.params(peers=N, seed=84, lazy_gossip=0, flood_publish=0)
    _, _, ref = _run(p, S, links, _sched(24, N), batch=24)
    kf = _ring_k(p, S, links, int(ref["cnt"].max()))  # (the widest mesh row)
    assert int(kf) == k and 0.05 < kf - int(kf) < 0.95, kf  # (away from a rounding of the host's integer times)


def test_go_preset_idontwant(monkeypatch):
    """k_lpull<.., IDW>: the go preset's IDONTWANT rows."""
    monkeypatch.setenv("GS_REQUIRE_LPULL", "1")
    N = 2000
    p = oracle.params_for("go", peers=N, seed=85, lazy_gossip=0)
    assert p.idontwant == 1000
    _run(p, 5, LINKS, _sched(24, N), batch=24)


def test_gossip_active_phase():
    """k_lpull<.., GOS>: a heartbeat at the publish instant, IHAVE / IWANT inside the passes."""
    N = 2000
    p = oracle.params(peers=N, seed=93, hb_phase_ns=_phase(0))
    _, st, _ = _run(p, 5, LINKS, _sched(24, N), batch=8, on_list=False)
    assert st["gossip_list_batches"] > 0 and st["gossip_iwant"] > 0


@pytest.mark.parametrize("gossip", [0, 1])
def test_churn_knobs_of_config_3(monkeypatch, gossip):
    """k_lpull<.., CHN> (and GOS + CHN): config #3's churn knobs, one publish per heartbeat."""
    monkeypatch.setenv("GS_REQUIRE_LPULL", "1")
    N, M, hb = 2000, 24, 1_000_000_000
    p = oracle.params(peers=N, seed=86, lazy_gossip=gossip, churn_ppm=10_000, churn_down=10, churn_horizon=16,
                      heartbeat_ns=hb, hb_phase_ns=T0 - 20 * hb + 370_000_000)
    sched = (T0 + np.arange(M, dtype=np.uint64) * np.uint64(hb), (6 + np.arange(M)) % N, np.full(M, 15000))
    _, st, _ = _run(p, 5, LINKS, sched, batch=M)
    assert 0 < st["deliveries"] < M * (N - 1)


@functools.lru_cache(maxsize=None)
def _part_ref():
    N = 2000
    p = oracle.params(peers=N, seed=87, lazy_gossip=0)
    sched = _sched(32, N)
    return p, sched, oracle.simulate(p, 5, LINKS, sched=sched)


def test_four_loopback_parts():
    """k_lpull<.., PART>: four loop-back parts of one graph (row offset u0,
    packed records read, this part's halves of the double buffers written)."""
    p, sched, ref = _part_ref()
    kw = {n: getattr(p, n) for n, _ in oracle.OrParams._fields_}
    kw["batch"] = 32
    sims = []
    for i in range(4):
        s = gossipsim.Simulator(**kw)
        s.set_topogen_links(5, *LINKS)
        s.connect_gossipsub_peers()
        s.mesh_converge()
        s.set_partition(4, i)
        sims.append(s)
    comm = gossipsim.Comm(local_parts=4)
    res = comm.run_partitioned(sims, sched)
    _first_diff("t_complete", np.concatenate([r["t_complete"] for r in res], axis=1), ref["t_complete"])
    _first_diff("hops", np.concatenate([r["hops"] for r in res], axis=1), ref["hops"])
    st = [s.stats() for s in sims]
    for k in COUNTERS:
        if k == "latency_max_ms":
            assert max(x[k] for x in st) == ref["stats"][k], k
        elif k == "messages":
            assert all(x[k] == ref["stats"][k] for x in st), k
        else:
            assert sum(x[k] for x in st) == ref["stats"][k], k
    assert all(x["list_pull_batches"] == x["batches"] > 0 for x in st)
    comm.close()


def test_forced_overflow_rerun(monkeypatch):
    """GS_LPULL_CAP: lists capped at 2 entries overflow (the capacity is read
    where entries are appended and where they are applied); the batch re-runs
    on the dense rows."""
    monkeypatch.setenv("GS_LPULL_CAP", "2")
    N = 2000
    _, st, _ = _run(oracle.params(peers=N, seed=88, lazy_gossip=0), 5, LINKS, _sched(64, N), batch=64, on_list=False)
    assert st["list_pull_batches"] == 0


def test_pass_parity_across_batches(monkeypatch):
    """Two consecutive batches on one context with different numbers of
    windows (24 messages, then 5 published half a second apart from each
    other). The passes of a batch alternate between the halves of the record
    and count buffers (the parity offset takes both values within every
    batch); the host numbers each batch's passes from 0, so a batch always
    starts on the same half, here on buffers the previous batch has used."""
    monkeypatch.setenv("GS_REQUIRE_LPULL", "1")
    N = 1000
    t, pub, size = _sched(29, N)
    t = t.copy()
    t[24:] = t[23] + np.uint64(1_000_000_000) + np.arange(5, dtype=np.uint64) * np.uint64(500_000_000)
    p = oracle.params(peers=N, seed=89, lazy_gossip=0)
    sim, _ = gpu_sim(p, 5, LINKS, batch=24)
    ref = oracle.simulate(p, 5, LINKS, sched=(t, pub, size))
    st = _exact(sim, sim.run((t, pub, size)), ref)
    assert st["batches"] == 2 and st["list_pull_batches"] == 2
    assert st["relax_launches"] > 0
