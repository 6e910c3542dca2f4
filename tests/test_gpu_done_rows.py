"""The list pass books a row whose every lane is final without visiting it
(gs_lpull_kernel.h step 0, state word LP_LOG).

A row's state carries the count of its final lanes: the publisher's own lanes
(k_lpub) plus the finals of every visit. Step 0 takes a row whose count equals
the batch's lanes per row out of the pass: it is not visited whatever its
neighbours sent, it emits no records and its stale list entries drive no pass.
A count that runs ahead of the final lanes (a lane counted twice, a count kept
from the batch before, a comparison against less than the batch's lanes) ends a
row early and drops deliveries; a count that is never reached only costs the
visits it was meant to save. Either way the results must not move, so every
case is bit-exact against the CPU oracle, once with the final log
(collect=True: t_complete, hops, the eight counters) and once as the
counters-only twin (collect=False: the counters), every batch on the list pass.

What a shape is meant to exercise is asserted from the oracle's output alone by
a restatement of step 0's rule (_late_visits): every final in its window, a row
visited in window c when a mesh neighbour has finals in window c - 1, and the
visits after the row's own last final counted. On the CPU the oracle gives 477
such visits of 2118 at 300 peers x 1024 messages and 501 of 2076 at 300 x 128;
the margins below ask for a good part of that."""
import functools

import numpy as np
import pytest

import gossipsim
import oracle
import topo_ref as T
from test_gpu_gossip_list import _phase
from test_gpu_parity import UND, _knobs, gpu_sim
from test_gpu_record_stream import COUNTERS, LINKS, UNIFORM, _exact, _finals_per_window, _first_diff, _window_ns
from test_gpu_row_insns import LOCKSTEP, _both

pytestmark = pytest.mark.gpu

N = 300
E = 0xFFFFFFFF
T0 = gossipsim.T0_NS


def _sched_of(pub, size=15000):
    pub = np.asarray(pub)
    return T0 + np.arange(len(pub), dtype=np.uint64) * np.uint64(1_000_000_000), pub, np.full(len(pub), size)


def _random_publishers(B, peers, seed, among=None):
    rng = np.random.default_rng(seed)
    return rng.integers(0, peers, B) if among is None else rng.choice(among, B)


def _late_visits(tc, mesh, cnt, sched, delta):
    """One lockstep batch (tc [messages, peers], its schedule) -> the row visits of its
    PULL passes, those of them after the row's last lane became final, the most such
    visits of one row, and the rows whose every lane becomes final."""
    fw = _finals_per_window({"t_complete": tc}, sched, delta)  # [peers, windows]
    sent = fw > 0
    n, W = fw.shape
    visited = np.zeros((n, W + 1), bool)
    for w in range(n):
        nb = mesh[w, :cnt[w]].astype(np.int64) & 0xFFFFFF
        visited[w, 1:] = sent[nb].any(axis=0)
    finished = (tc != UND).all(axis=0)
    # (a row without a final of its own, every lane the publisher's: finished from the start)
    last = np.where(sent.any(axis=1), W - 1 - np.argmax(sent[:, ::-1], axis=1), -1)
    late = visited & (np.arange(W + 1)[None, :] > last[:, None]) & finished[:, None]
    return int(visited.sum()), int(late.sum()), int(late.sum(axis=1).max()), finished


@functools.lru_cache(maxsize=None)
def _converged(B):
    """Case 1's graph (300 peers, converged mesh, the bench's 5 link classes) with B
    random publishers: parameters, schedule, oracle run (computed once, not changed)."""
    p = oracle.params(peers=N, seed=1, lazy_gossip=0)
    sched = _sched_of(_random_publishers(B, N, B))
    return p, sched, oracle.simulate(p, 5, LINKS, sched=sched)


@pytest.mark.parametrize("B", [1024, 128, 70, 600], ids=["wide_rows", "narrow_rows", "70_of_512_lanes", "600_of_1024_lanes"])
def test_finished_rows_among_sending_neighbours(monkeypatch, B):
    """Rows of CH = 16 (1024 lanes) and CH = 8 (128), and rows that are partly
    filled: a batch of 70 runs in rows of 512 lanes, one of 600 in rows of 1024, and
    the full count is the batch's 70 or 600. A comparison against the row width would
    never skip; one against a smaller number would end rows with lanes still to come."""
    monkeypatch.setenv("GS_REQUIRE_LPULL", "1")
    p, sched, ref = _converged(B)
    visits, late, _, finished = _late_visits(ref["t_complete"], ref["mesh"], ref["cnt"], sched, _window_ns(p, 5, LINKS))
    print("B = %d: %d row visits, %d after the row finished" % (B, visits, late))
    assert finished.all() and late >= 100, (visits, late)
    _both(p, 5, LINKS, sched, B, ref)


def _both_on(make_sim, sched, ref):
    """_both for a context that make_sim() builds (an imported graph or mesh)."""
    sim = make_sim()
    st = _exact(sim, sim.run(sched), ref)
    sim2 = make_sim()
    sim2.run(sched, collect=False)
    st2 = sim2.stats()
    for k in COUNTERS:
        assert st2[k] == ref["stats"][k], "collect=False: " + k
    assert st["list_pull_batches"] == st["batches"] > 0
    assert st2["list_pull_batches"] == st2["batches"] > 0


@functools.lru_cache(maxsize=None)
def _ring():
    """140 peers on a ring with chords (steps 1, 2 and 5: six links each, all of them
    mesh links), one link class, 4 publishers inside an arc of 7 peers with 256 lanes
    each (LOCKSTEP: what one publisher's lanes may be)."""
    n, steps = 140, (1, 2, 5)
    p = oracle.params(peers=n, seed=7, lazy_gossip=0)
    dialer, target = T._dials(T.ring_dials(n, steps))
    row, col, _ = T.dials_to_csr(n, dialer, target)
    d = 2 * len(steps)
    mesh = np.full((n, gossipsim.MESH_W), E, np.uint32)
    mesh[:, :d] = col.reshape(n, d)
    cnt = np.full(n, d, np.uint8)
    lat, bw = oracle.topogen_links(1, *UNIFORM)
    sched = _sched_of(np.repeat(np.arange(4) * 2, LOCKSTEP))
    tc, hops, st = oracle.run(p, row, col, mesh, cnt, np.zeros(n, np.uint8), lat, bw, bw, *sched)
    return p, (dialer, target), mesh, cnt, sched, dict(t_complete=tc, hops=hops, stats=st)


def test_a_long_tail(monkeypatch):
    """The rows near the publishers' arc are finished for several windows while their
    neighbours on the far side still send, and the long way round delivers
    duplicates late: some row is visited in three windows after it finished."""
    monkeypatch.setenv("GS_REQUIRE_LPULL", "1")
    p, dials, mesh, cnt, sched, ref = _ring()
    visits, late, longest, finished = _late_visits(ref["t_complete"], mesh, cnt, sched, _window_ns(p, 1, UNIFORM))
    print("ring: %d row visits, %d after the row finished, %d of one row" % (visits, late, longest))
    assert finished.all() and ref["hops"].max() < 64 and longest >= 3, (visits, late, longest)
    rows = np.repeat(np.arange(p.peers), cnt)
    cols = mesh[:, :cnt[0]].reshape(-1)

    def make():
        sim = gossipsim.Simulator(batch=len(sched[0]), **_knobs(p))
        sim.set_topogen_links(1, *UNIFORM)
        sim.set_dials(*dials)
        sim.set_mesh_links(rows[rows < cols], cols[rows < cols])
        np.testing.assert_array_equal(sim.mesh()[0], mesh)
        return sim
    _both_on(make, sched, ref)


@functools.lru_cache(maxsize=None)
def _one_row_emptied():
    """Case 1's graph with the mesh row of one peer x emptied (its links taken out of
    its neighbours' rows as well). No publisher is x or connected to x (the publisher
    floods its connections), and the first 256 messages have one publisher."""
    p, _, conv = _converged(1024)
    row, col = conv["row_ptr"].astype(np.int64), conv["col"].astype(np.int64)
    x = 150
    apart = np.setdiff1d(np.arange(N), np.append(col[row[x]:row[x + 1]], x))
    pub = _random_publishers(1024, N, 5, among=apart)
    pub[:LOCKSTEP] = pub[0]
    mesh = np.full((N, gossipsim.MESH_W), E, np.uint32)
    cnt = np.zeros(N, np.uint8)
    for w in range(N):
        nb = np.sort(conv["mesh"][w, :conv["cnt"][w]].astype(np.int64) & 0xFFFFFF)
        nb = nb[nb != x] if w != x else nb[:0]
        mesh[w, :len(nb)] = nb
        cnt[w] = len(nb)
    sched = _sched_of(pub)
    tc, hops, st = oracle.run(p, conv["row_ptr"], conv["col"], mesh, cnt, conv["stage"], conv["lat"], conv["bw"],
                              conv["bw"], *sched)
    return p, x, mesh, cnt, sched, dict(t_complete=tc, hops=hops, stats=st)


def test_rows_that_never_finish(monkeypatch):
    """Every message misses peer x: its row's count stays 0 and the row keeps
    today's path, as the publishers' rows do until their last lane (one of them starts
    with 256 lanes counted by k_lpub); the other rows finish and are skipped."""
    monkeypatch.setenv("GS_REQUIRE_LPULL", "1")
    p, x, mesh, cnt, sched, ref = _one_row_emptied()
    B = len(sched[0])
    tc = ref["t_complete"]
    assert (tc[:, x] == UND).all() and int((tc == UND).sum()) == B
    assert ref["stats"]["deliveries"] == B * (N - 2) < B * (N - 1)
    assert (sched[1][:LOCKSTEP] == sched[1][0]).all()
    visits, late, _, finished = _late_visits(tc, mesh, cnt, sched, _window_ns(p, 5, LINKS))
    print("one row emptied: %d row visits, %d after the row finished" % (visits, late))
    assert not finished[x] and finished.sum() == N - 1 and late >= 100, (visits, late)

    def make():
        sim = gossipsim.Simulator(batch=B, **_knobs(p))
        sim.set_topogen_links(5, *LINKS)
        sim.connect_gossipsub_peers()
        sim.set_mesh(mesh, cnt)
        np.testing.assert_array_equal(sim.mesh()[0], mesh)
        return sim
    _both_on(make, sched, ref)


@pytest.mark.parametrize("B", [1024, 128])
def test_two_batches_in_one_run(monkeypatch, B):
    """Two batches on one context: the counts are cleared with the rest of the row
    state (lpull_begin); a count that survived would finish its rows at once in
    the second batch, which would then deliver nothing past the seeds."""
    monkeypatch.setenv("GS_REQUIRE_LPULL", "1")
    p = oracle.params(peers=N, seed=1, lazy_gossip=0)
    sched = _sched_of(_random_publishers(2 * B, N, 3 * B))
    ref = oracle.simulate(p, 5, LINKS, sched=sched)
    second = tuple(a[B:] for a in sched)
    _, late, _, finished = _late_visits(ref["t_complete"][B:], ref["mesh"], ref["cnt"], second, _window_ns(p, 5, LINKS))
    assert finished.all() and late >= 100, late
    sim, _ = gpu_sim(p, 5, LINKS, batch=B)
    st = _exact(sim, sim.run(sched), ref)
    assert st["batches"] == 2 == st["list_pull_batches"]
    sim2, _ = gpu_sim(p, 5, LINKS, batch=B)
    sim2.run(sched, collect=False)
    st2 = sim2.stats()
    for k in COUNTERS:
        assert st2[k] == ref["stats"][k], "collect=False: " + k
    assert st2["batches"] == 2 == st2["list_pull_batches"]


# ---- the further forms that took the test, 128 messages each ----
def test_go_preset(monkeypatch):
    """k_lpull<1, 8, IDW>: dense final keys and no log; the count is kept as in the no-log twin."""
    monkeypatch.setenv("GS_REQUIRE_LPULL", "1")
    n, B = 600, 128
    p = oracle.params_for("go", peers=n, seed=105, lazy_gossip=0)
    assert p.idontwant == 1000
    sched = _sched_of(_random_publishers(B, n, 11))
    ref = oracle.simulate(p, 5, LINKS, sched=sched)
    _, late, _, finished = _late_visits(ref["t_complete"], ref["mesh"], ref["cnt"], sched, _window_ns(p, 5, LINKS))
    assert finished.all() and late >= 100, late
    _both(p, 5, LINKS, sched, B, ref)


@functools.lru_cache(maxsize=None)
def _gossip_370():
    n, B = 4000, 128
    p = oracle.params(peers=n, seed=9, hb_phase_ns=_phase(370))
    sched = _sched_of(_random_publishers(B, n, 7))
    return p, sched, oracle.simulate(p, 5, LINKS, sched=sched)


def test_heartbeats_370_ms_after_the_publish():
    """k_lpull<1, 8, .., GOS>: a heartbeat while the last peers are still waiting (4000
    peers: a smaller graph is done by then and its gossip is a no-op). Most rows are
    finished in the gossip windows; the unfinished ones still send their IWANTs."""
    p, sched, ref = _gossip_370()
    assert ref["stats"]["gossip_iwant"] > 0
    sim, _ = gpu_sim(p, 5, LINKS, batch=len(sched[0]))
    st = _exact(sim, sim.run(sched), ref)
    assert st["gossip_list_batches"] == st["batches"] == 1
    sim2, _ = gpu_sim(p, 5, LINKS, batch=len(sched[0]))
    sim2.run(sched, collect=False)
    st2 = sim2.stats()
    for k in COUNTERS:
        assert st2[k] == ref["stats"][k], "collect=False: " + k


def test_two_loopback_parts():
    """k_lpull<1, 8, false, PART>: each part books its own finished rows."""
    p, sched, ref = _converged(128)
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
