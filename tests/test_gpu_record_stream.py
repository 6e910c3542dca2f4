"""The list pass's streamed record step (gs_lpull_kernel.h, STREAM;
DESIGN.md §4.3): a row's neighbours stream their 64-record chunks through four
contexts of two register slots each; a context whose neighbour is exhausted
takes the row's next candidate. A wrong cursor, a refill with stale constants
or a slot reused too early loses or invents a candidate key, so every case is
bit-exact against the CPU oracle: t_complete, hops and the eight counters.

The shapes: a neighbour's record count at the chunk edges (1, 63..65, 127..129,
257, 1024 lanes per row), neighbours of one row with very different counts,
rows with more and with fewer neighbours than contexts, and one small case per
instantiation family that shares the step (fragment groups, IDONTWANT, gossip,
partitioned). The coverage of the first two is asserted from the oracle's
completion times, not assumed."""
import functools

import numpy as np
import pytest

import gossipsim
import oracle
from test_gpu_gossip_list import _phase
from test_gpu_parity import UND, _sched, gpu_sim

pytestmark = pytest.mark.gpu
LINKS = (50, 150, 40, 130)  # the bench's link ranges (bench.py --links, with 5 stages)
UNIFORM = (50, 50, 50, 50)  # one link class (with S = 1)
COUNTERS = ("deliveries", "frag_deliveries", "relaxations", "bytes_alg", "latency_sum_ms", "latency_max_ms",
            "messages", "gossip_iwant")


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


def _window_ns(p, S, links, size=15000):
    """The window width Delta of an unfragmented batch: the smallest latency plus
    the smallest serialisation time (as _ring_k of test_gpu_lpull_args derives it)."""
    lat, bw = oracle.topogen_links(S, *links)
    ser = oracle.wire_bytes(size, p.muxer, p.signed_msgs) * 8e9 / bw.astype(np.float64)
    return int(lat.astype(np.float64).min() + ser.min())


def _finals_per_window(ref, sched, delta):
    """[peers, windows]: the messages of one lockstep batch that become final at a
    peer in each window of its own publish-relative time. A peer's finals of a
    window are the records its neighbours pull from it in the next pass."""
    tc = ref["t_complete"]
    rel = tc - np.asarray(sched[0], np.uint64)[:, None]
    ok = tc != UND
    ok[np.arange(tc.shape[0]), np.asarray(sched[1])] = False  # (the publisher's own lane is seeded, not pulled)
    win = np.where(ok, rel // np.uint64(delta), 0).astype(np.int64)
    out = np.zeros((tc.shape[1], int(win.max()) + 1), np.int64)
    m, u = np.nonzero(ok)
    np.add.at(out, (u, win[m, u]), 1)
    return out


def _one_publisher(B, N):
    """B publishes of one peer: every lane of the batch takes the same paths at
    the same publish-relative times, so a peer's B lanes are final in one window."""
    t, pub, size = _sched(B, N)
    return t, np.full(B, pub[0]), size


def _partly_lockstep(B, N, lock):
    """The first `lock` lanes from one publisher, the others from a publisher each:
    a peer's finals of a window are the lockstep lanes plus some of the others."""
    t, pub, size = _sched(B, N)
    pub = pub.copy()
    pub[:lock] = pub[0]
    return t, pub, size


@pytest.mark.parametrize("B", [1, 63, 64, 65, 127, 128, 129, 257, 1024])
def test_records_per_neighbour_at_chunk_edges(monkeypatch, B):
    """One link class and one publisher: a peer's lanes of a batch of B become
    final together, so a neighbour holds B records in a window: 1, one under /
    at / over a chunk (63..65), a slot pair (127..129), past two turns of a
    context (257) and 16 chunks (1024, rows of CH = 16)."""
    monkeypatch.setenv("GS_REQUIRE_LPULL", "1")
    N = 300
    p = oracle.params(peers=N, seed=101, lazy_gossip=0)
    sched = _one_publisher(B, N)
    _, _, ref = _run(p, 1, UNIFORM, sched, batch=B)
    fw = _finals_per_window(ref, sched, _window_ns(p, 1, UNIFORM))
    assert fw.max() >= max(B - 1, 1), fw.max()


@pytest.mark.parametrize("B", [192, 1024])
def test_uneven_streams(monkeypatch, B):
    """The bench's stages and links: in one window some peer holds more than a
    slot pair of records while another holds less than a chunk, so the contexts
    of a row drain and refill at different times."""
    monkeypatch.setenv("GS_REQUIRE_LPULL", "1")
    N = 1000
    p = oracle.params(peers=N, seed=102, lazy_gossip=0)
    # 1024 lanes of 1000 publishers are uneven as they are; 192 such lanes stay under a slot pair
    # per window (93 at most), so 100 of them are one publisher's (from about 110 lockstep lanes
    # on, these links put more than the 256 entries a list holds into one window of a row)
    sched = _sched(B, N) if B == 1024 else _partly_lockstep(B, N, 100)
    _, _, ref = _run(p, 5, LINKS, sched, batch=B)
    fw = _finals_per_window(ref, sched, _window_ns(p, 5, LINKS))
    # a mesh row whose neighbours are that uneven in one window
    mesh, cnt = ref["mesh"], ref["cnt"]
    found = False
    for w in range(N):
        nb = mesh[w, :cnt[w]].astype(np.int64) & 0xFFFFFF
        f = fw[nb]  # [neighbours, windows]
        big, small = (f > 128).any(axis=0), ((f > 0) & (f < 64)).any(axis=0)
        if (big & small).any():
            found = True
            break
    assert fw.max() > 128 and found, fw.max()


@pytest.mark.parametrize("d,d_lo,d_hi,d_out,connect_to", [(12, 10, 14, 4, 24), (3, 2, 4, 1, 10)])
def test_more_and_fewer_neighbours_than_contexts(monkeypatch, d, d_lo, d_hi, d_out, connect_to):
    """Mesh rows of 9-14 entries (three or more refills of the context set) and
    of 2-4 (contexts that never get a neighbour)."""
    monkeypatch.setenv("GS_REQUIRE_LPULL", "1")
    N, B = 600, 129
    p = oracle.params(peers=N, seed=103, lazy_gossip=0, d=d, d_lo=d_lo, d_hi=d_hi, d_lazy=d, d_out=d_out,
                      connect_to=connect_to)
    _, _, ref = _run(p, 5, LINKS, _sched(B, N), batch=B)
    cnt = ref["cnt"]
    if d == 12:
        assert cnt.max() >= 9, cnt.max()
    else:
        assert cnt.min() <= 3, cnt.min()


@pytest.mark.parametrize("B", [43, 171])
def test_fragment_groups(monkeypatch, B):
    """F = 3, a padded fragment group of 4 lanes: rows of 172 (CH = 8) and 684 lanes (CH = 16)."""
    monkeypatch.setenv("GS_REQUIRE_LPULL", "1")
    N = 300
    _run(oracle.params(peers=N, seed=104, lazy_gossip=0, fragments=3), 5, LINKS, _sched(B, N), batch=B)


def test_go_preset_idontwant(monkeypatch):
    """k_lpull<.., IDW>: the go preset's IDONTWANT rows, 129 lanes."""
    monkeypatch.setenv("GS_REQUIRE_LPULL", "1")
    N, B = 600, 129
    p = oracle.params_for("go", peers=N, seed=105, lazy_gossip=0)
    assert p.idontwant == 1000
    _run(p, 5, LINKS, _sched(B, N), batch=B)


def test_gossip_active_phase():
    """k_lpull<.., GOS>: a heartbeat at the publish instant, IHAVE / IWANT inside the passes, 65 lanes."""
    N, B = 1000, 65
    p = oracle.params(peers=N, seed=106, hb_phase_ns=_phase(0))
    _, st, _ = _run(p, 5, LINKS, _sched(B, N), batch=B, on_list=False)
    assert st["gossip_list_batches"] > 0 and st["gossip_iwant"] > 0


def test_two_batches_of_different_length(monkeypatch):
    """129 lanes, then 40 on the same context: the second batch starts on record
    and count halves, and in register slots, that the first one has used."""
    monkeypatch.setenv("GS_REQUIRE_LPULL", "1")
    N, B, B2 = 300, 129, 40
    t, pub, size = _sched(B + B2, N)
    p = oracle.params(peers=N, seed=107, lazy_gossip=0)
    sim, _ = gpu_sim(p, 5, LINKS, batch=B)
    ref = oracle.simulate(p, 5, LINKS, sched=(t, pub, size))
    st = _exact(sim, sim.run((t, pub, size)), ref)
    assert st["batches"] == 2 and st["list_pull_batches"] == 2


@functools.lru_cache(maxsize=None)
def _part_ref():
    N, B = 600, 129
    p = oracle.params(peers=N, seed=108, lazy_gossip=0)
    sched = _sched(B, N)
    return p, sched, oracle.simulate(p, 5, LINKS, sched=sched)


def test_two_loopback_parts():
    """k_lpull<.., PART>: two loop-back parts of one graph, 129 lanes (the
    neighbours' records are read from the packed exchange buffers)."""
    p, sched, ref = _part_ref()
    kw = {n: getattr(p, n) for n, _ in oracle.OrParams._fields_}
    kw["batch"] = 129
    sims = []
    for i in range(2):
        s = gossipsim.Simulator(**kw)
        s.set_topogen_links(5, *LINKS)
        s.connect_gossipsub_peers()
        s.mesh_converge()
        s.set_partition(2, i)
        sims.append(s)
    comm = gossipsim.Comm(local_parts=2)
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
