"""The list pass's row visit: the touched-chunk mask OR-reduced over the wave by
DPP row operations instead of six LDS shuffles (gs_lpull_kernel.h, wave_or32 of
gs_common.h). The cases also cover the row
addressing that round built and did not keep (32-bit offsets on scalar bases),
so that a later attempt finds its tests here.

That changes nothing the pass computes, so every case is bit-exact against the
CPU oracle: t_complete and hops of a logged run (collect=True), the counters
and the latency sum / max of a counters-only run (collect=False).

What can go wrong, and the shape that shows it:
 - a row offset computed from the wrong row or lane: peers that are no multiple
   of 64 or of the grid's stride (300, 3001), so the last scan group is partial
   and the last row is N - 1;
 - a DPP row or bank mask that loses a lane's contribution: the mask bit of a
   chunk that only one lane touched. A batch of 1 message has one record per
   neighbour (lane 0), one of 65 fills a neighbour's first 64 record lanes and
   lane 0 of the next turn (lanes >= 32 and lane 63 each alone in their chunk
   somewhere in the run), 1024 fills every chunk; rows of 512 lanes (batch=512)
   with 70 and 512 messages are the CH = 8 form;
 - the forms that share the code: logged and no-log, the go preset's dense keys
   (IDW), gossip windows (GOS), both, two loop-back parts (PART), and one run of
   fragment groups (F = 8), a family that keeps the shuffle form."""
import functools

import numpy as np
import pytest

import gossipsim
import oracle
from test_gpu_gossip_list import _phase
from test_gpu_parity import _knobs, gpu_sim
from test_gpu_record_stream import COUNTERS, LINKS, _exact, _first_diff
from test_gpu_row_insns import _both

T0 = gossipsim.T0_NS


def _sched_of(pub, size=15000):
    pub = np.asarray(pub)
    return T0 + np.arange(len(pub), dtype=np.uint64) * np.uint64(1_000_000_000), pub, np.full(len(pub), size)


def _publishers(B, peers, seed):
    return np.random.default_rng(seed).integers(0, peers, B)


@functools.lru_cache(maxsize=None)
def _case(peers, seed, B, node=None, **kw):
    """Parameters, schedule and the oracle's run (computed once, not changed)."""
    kw.setdefault("lazy_gossip", 0)
    p = oracle.params_for(node, peers=peers, seed=seed, **kw) if node else oracle.params(peers=peers, seed=seed, **kw)
    sched = _sched_of(_publishers(B, peers, seed + B))
    return p, sched, oracle.simulate(p, 5, LINKS, sched=sched)


def _counters_only(p, sched, batch, ref):
    sim, _ = gpu_sim(p, 5, LINKS, batch=batch)
    sim.run(sched, collect=False)
    st = sim.stats()
    for k in COUNTERS:
        assert st[k] == ref["stats"][k], "collect=False: " + k
    return st


# ---- row index and offsets ----
@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("peers,B", [(300, 1024), (3001, 600)], ids=["n300", "n3001"])
def test_rows_not_a_multiple_of_the_scan(monkeypatch, peers, B, seed):
    """Rows of 1024 lanes (600 messages still take them), logged and no-log."""
    monkeypatch.setenv("GS_REQUIRE_LPULL", "1")
    p, sched, ref = _case(peers, seed, B)
    _both(p, 5, LINKS, sched, B, ref)


# ---- the chunk mask ----
@pytest.mark.gpu
@pytest.mark.parametrize("batch,B", [(1024, 1), (1024, 65), (1024, 1024), (512, 70), (512, 512)])
def test_chunk_mask(monkeypatch, batch, B):
    monkeypatch.setenv("GS_REQUIRE_LPULL", "1")
    p, sched, ref = _case(300, 3, B)
    _both(p, 5, LINKS, sched, batch, ref)


# ---- the forms that share the code ----
@pytest.mark.gpu
@pytest.mark.parametrize("B", [600, 128], ids=["ch16", "ch8"])
def test_go_preset(monkeypatch, B):
    """k_lpull<1, CH, IDW>: dense final keys, no log."""
    monkeypatch.setenv("GS_REQUIRE_LPULL", "1")
    p, sched, ref = _case(300, 105, B, node="go")
    assert p.idontwant == 1000
    _both(p, 5, LINKS, sched, B, ref)


@functools.lru_cache(maxsize=None)
def _gossip(node):
    n, B = 4000, 128
    kw = dict(peers=n, seed=9, hb_phase_ns=_phase(370))
    p = oracle.params_for(node, **kw) if node else oracle.params(**kw)
    sched = _sched_of(_publishers(B, n, 7))
    return p, sched, oracle.simulate(p, 5, LINKS, sched=sched)


@pytest.mark.gpu
@pytest.mark.parametrize("node", [None, "go"], ids=["gos", "go_gos"])
def test_heartbeat_370_ms_after_the_publish(node):
    """k_lpull<1, 8, .., GOS> and <1, 8, IDW, .., GOS>: a heartbeat while the last peers are
    still waiting (4000 peers: a smaller graph is done by then), row-done words and IWANTs."""
    p, sched, ref = _gossip(node)
    assert ref["stats"]["gossip_iwant"] > 0
    sim, _ = gpu_sim(p, 5, LINKS, batch=len(sched[0]))
    st = _exact(sim, sim.run(sched), ref)
    assert st["gossip_list_batches"] == st["batches"] == 1
    _counters_only(p, sched, len(sched[0]), ref)


@pytest.mark.gpu
def test_two_loopback_parts():
    """k_lpull<1, 8, false, PART> at 3001 peers: local rows, global mesh rows (u0 + w)."""
    p, sched, ref = _case(3001, 4, 128)
    kw = _knobs(p)
    kw["batch"] = 128
    for collect in (True, False):
        sims = []
        for i in range(2):
            s = gossipsim.Simulator(**kw)
            s.set_topogen_links(5, *LINKS)
            s.connect_gossipsub_peers()
            s.mesh_converge()
            s.set_partition(2, i)
            sims.append(s)
        comm = gossipsim.Comm(local_parts=2)
        res = comm.run_partitioned(sims, sched, collect=collect)
        if collect:
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


@pytest.mark.gpu
def test_fragment_groups(monkeypatch):
    """k_lpull<8, ..>: 8 fragments per message at 300 peers (64 messages: rows of 512 lanes)."""
    monkeypatch.setenv("GS_REQUIRE_LPULL", "1")
    p, sched, ref = _case(300, 6, 64, fragments=8)
    _both(p, 5, LINKS, sched, 64, ref)
