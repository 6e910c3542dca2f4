"""Reference of the per-link first-delivery counts (gs_set_link_deliveries).

A Python replay of DESIGN.md §2.5 for one message at a time with F = 1, no IDONTWANT and no IWANT:
a heap over keys (t, hops, src). The publisher holds key 0 and sends to its CSR row in ascending
id (to its mesh row without flood-publish); a first receipt at u forwards to mesh(u) \\ {src, p} in
ascending id, the copy at position pos (from 1) leaving at t + pos * ser_up(u) and arriving
lat + max(0, ser_dn(w) - ser_up(u)) later; ser = ceil(wire * 8e9 / bw) as in gs_oracle.c. Ties
are decided by the key order itself.

The replay proves itself against the oracle before it says anything: its arrival times and hops
must equal the oracle's t_complete and hops for every peer and message. Only then does it hand
out the src of every (peer, message), and from them the [nnz, 3] link counts and the [N, 3]
given. A case in which the oracle answered an IWANT (stats.gossip_iwant != 0) is not exact and is
refused."""
import heapq

import numpy as np

import oracle

PUBLISH, MESH, GOSSIP, COLS = 0, 1, 2, 3
UND = np.iinfo(np.uint64).max


def _ceil_div(a, b):
    return (a + b - 1) // b


def replay_message(p, g, t_pub, pub, size):
    """One message on graph g (row_ptr, col, mesh, cnt, stage, lat, bw): -> (t [N], hops [N], src [N]);
    t is absolute, UND where the message never arrives; src is -1 there and at the publisher."""
    N = p.peers
    row, col = g["row_ptr"].astype(np.int64), g["col"].astype(np.int64)
    stage, lat = g["stage"], g["lat"].reshape(len(g["bw"]), -1)
    wire = oracle.wire_bytes(int(size) // p.fragments, p.muxer, p.signed_msgs)
    ser = [_ceil_div(wire * 8_000_000_000, int(b)) for b in g["bw"]]  # up and down links are one table here
    mesh = [sorted(int(w) for w in g["mesh"][u, :g["cnt"][u]]) for u in range(N)]
    t = [None] * N
    hops, src = [0xFF] * N, [-1] * N
    t[pub], hops[pub] = 0, 0
    heap = []

    def send(u, at, hp, targets):
        su = int(stage[u])
        for pos, w in enumerate(targets, 1):
            sw = int(stage[w])
            arr = at + pos * ser[su] + int(lat[su, sw]) + max(0, ser[sw] - ser[su])
            heapq.heappush(heap, (arr, hp + 1, u, w))

    send(pub, 0, 0, [int(w) for w in col[row[pub]:row[pub + 1]]] if p.flood_publish else mesh[pub])
    while heap:
        at, hp, s, u = heapq.heappop(heap)
        if t[u] is not None:
            continue
        t[u], hops[u], src[u] = at, hp, s
        send(u, at, hp, [w for w in mesh[u] if w != s and w != pub])
    tabs = np.array([UND if x is None else int(t_pub) + x for x in t], np.uint64)
    return tabs, np.array(hops, np.uint8), np.array(src, np.int64)


def counts_of(g, pubs, src):
    """src [M, N] -> (edge [nnz, 3], given [N, 3]) over g's CSR."""
    row, col = g["row_ptr"].astype(np.int64), g["col"].astype(np.int64)
    N = len(row) - 1
    edge = np.zeros((len(col), COLS), np.uint64)
    given = np.zeros((N, COLS), np.uint64)
    for m, pub in enumerate(pubs):
        for u in np.nonzero(src[m] >= 0)[0]:
            s = int(src[m, u])
            e = row[u] + int(np.searchsorted(col[row[u]:row[u + 1]], s))
            assert e < row[u + 1] and col[e] == s, "the sender is a connection of the receiver"
            k = PUBLISH if s == int(pub) else MESH if s in g["mesh"][u, :g["cnt"][u]] else GOSSIP
            edge[e, k] += np.uint64(1)
            given[s, k] += np.uint64(1)
    return edge, given


def reference(p, g, sched):
    """The exact reference of a case: g is what oracle.simulate returns (row_ptr, col, mesh, cnt,
    stage, lat, bw, t_complete, hops, stats) for the schedule (t, publisher, size)."""
    assert p.fragments == 1 and not p.idontwant and not p.churn_ppm, "the replay covers F = 1 on a frozen mesh"
    assert g["stats"]["gossip_iwant"] == 0, "an IWANT was answered: not an exact case"
    t, pubs, sizes = sched[:3]
    src = np.zeros((len(t), p.peers), np.int64)
    for m in range(len(t)):
        tm, hm, src[m] = replay_message(p, g, t[m], int(pubs[m]), sizes[m])
        np.testing.assert_array_equal(tm, g["t_complete"][m], err_msg="replay t_complete, message %d" % m)
        np.testing.assert_array_equal(hm, g["hops"][m], err_msg="replay hops, message %d" % m)
    edge, given = counts_of(g, pubs, src)
    return dict(src=src, edge=edge, given=given)


def transpose_sum(col, edge, peers):
    """given[col[e]][k] += edge[e][k]: what gs_get_peer_given derives."""
    given = np.zeros((peers, COLS), np.uint64)
    np.add.at(given, np.asarray(col, np.int64), np.asarray(edge, np.uint64))
    return given


# ---- the cases of tests/test_link_deliveries_cpu.py and tests/test_gpu_link_deliveries.py ----
T0 = 946685300_003_000_000  # gossipsim.T0_NS: the benchmark's first publish instant
LINKS = (50, 150, 40, 130)
STAGES = 5
SIZE = 15000
PHASE = T0 % 1_000_000_000  # hb_phase_ns that puts a heartbeat on the publish instant

# name -> (oracle params, messages, batch); built graphs, all exact
BUILT = {
    "rust": (dict(peers=300, lazy_gossip=0), 4, 8),
    "quiet": (dict(peers=300), 4, 8),  # lazy gossip on, heartbeats off the publish instant: IHAVEs only
    "no_flood": (dict(peers=300, flood_publish=0, lazy_gossip=0), 4, 8),
    "n257_m1": (dict(peers=257, lazy_gossip=0), 1, 8),
    "n900_m12": (dict(peers=900, lazy_gossip=0), 12, 8),
}
_REF = {}


def sched_of(M, N, size=SIZE):
    t = np.uint64(T0) + np.arange(M, dtype=np.uint64) * np.uint64(1_000_000_000)
    return t, (37 * np.arange(M) + 4) % N, np.full(M, size)


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def built(name):
    """-> (p, sched, oracle.simulate's dict, reference) of a BUILT case, computed once, read-only."""
    if name not in _REF:
        kw, M, _ = BUILT[name]
        p = oracle.params(seed=71, **kw)
        sched = sched_of(M, p.peers)
        g = oracle.simulate(p, STAGES, LINKS, sched=sched)
        _REF[name] = (p, sched, _freeze(g), _freeze(reference(p, g, sched)))
    return _REF[name]


def on_graph(p, row, col, flags0, sched, mesh=None, cnt=None):
    """oracle.simulate's dict for a caller's CSR (and, with mesh / cnt, a caller's mesh in place of the
    converged one)."""
    lat, bw = oracle.topogen_links(STAGES, *LINKS)
    stage = (np.arange(p.peers) % STAGES).astype(np.uint8)
    if mesh is None:
        _, mesh, cnt, _ = oracle.mesh_converge(p, row, col, flags0, stage, lat)
    tc, hops, st = oracle.run(p, row, col, mesh, cnt, stage, lat, bw, bw, *sched)
    return _freeze(dict(row_ptr=row, col=col, flags0=flags0, mesh=mesh, cnt=cnt, stage=stage, lat=lat, bw=bw,
                        t_complete=tc, hops=hops, stats=st))


def hub():
    """The hub graph G2 of tests/topo_ref.py (degree 202) with its publishers: -> (p, sched, g, ref, dials)."""
    if "hub" not in _REF:
        import topo_ref
        N, d, t, pubs = topo_ref.graph("G2")
        p = oracle.params(peers=N, seed=7, lazy_gossip=0)
        M = len(pubs)
        sched = (np.uint64(T0) + np.arange(M, dtype=np.uint64) * np.uint64(1_000_000_000), np.asarray(pubs),
                 np.full(M, SIZE))
        g = on_graph(p, *topo_ref.dials_to_csr(N, d, t), sched)
        _REF["hub"] = (p, sched, g, _freeze(reference(p, g, sched)), (d, t))
    return _REF["hub"]


def empty_mesh():
    """The built graph of 300 peers under an empty mesh: the publisher's flood is all there is."""
    if "empty" not in _REF:
        p = oracle.params(peers=300, seed=71, lazy_gossip=0)
        sched = sched_of(3, 300)
        row, col, fl = oracle.build_topology(p)
        mesh = np.full((300, oracle.MESH_W), 0xFFFFFFFF, np.uint32)
        g = on_graph(p, row, col, fl, sched, mesh, np.zeros(300, np.uint8))
        _REF["empty"] = (p, sched, g, _freeze(reference(p, g, sched)))
    return _REF["empty"]


# invariant cases (the replay does not cover them): name -> (node, params, messages)
# "gossip": a heartbeat at every publish instant (hb_phase_ns = PHASE, as in
# tests/test_gpu_pubsub_counts.py) and one every 100 ms after it, so that peers who hold the
# message gossip it while the eager wave is still on its way (gossip_winners asserts from the
# oracle that an IWANT answer of a non-publisher wins somewhere)
INVARIANT = {
    "f3": (0, dict(peers=300, fragments=3, lazy_gossip=0), 4),
    "go": ("go", dict(peers=300, hb_phase_ns=PHASE), 4),
    "gossip": (0, dict(peers=300, hb_phase_ns=PHASE, heartbeat_ns=100_000_000), 4),
}


def invariant(name):
    """-> (p, sched, oracle.simulate's dict) of an INVARIANT case, computed once, read-only."""
    key = "inv-" + name
    if key not in _REF:
        node, kw, M = INVARIANT[name]
        p = oracle.params_for(node, seed=71, **kw)
        sched = sched_of(M, p.peers)
        _REF[key] = (p, sched, _freeze(oracle.simulate(p, STAGES, LINKS, sched=sched)))
    return _REF[key]


def gossip_winners():
    """The gossip case's reason to exist, from the oracle alone: -> (peers whose (t_complete, hops)
    differ from the same case with lazy_gossip = 0, messages with a proven GOSSIP delivery).

    Take, in one message, the differing peer u with the earliest arrival in either run. Up to
    that instant both runs are the same, so every eager copy on its way to u exists in both; had
    u's earliest copy been one of them, u would not differ. It is an IWANT answer, then, from a
    sender outside mesh(u); where u is no connection of the publisher the sender is not the
    publisher either, and the delivery is GOSSIP by definition (an answer of the publisher would
    count as PUBLISH)."""
    p, sched, g = invariant("gossip")
    kw = dict(INVARIANT["gossip"][1], lazy_gossip=0)
    g0 = oracle.simulate(oracle.params_for(0, seed=71, **kw), STAGES, LINKS, sched=sched)
    row, col = g["row_ptr"].astype(np.int64), g["col"]
    changed, proven = 0, 0
    for m, pub in enumerate(sched[1]):
        d = np.nonzero((g["t_complete"][m] != g0["t_complete"][m]) | (g["hops"][m] != g0["hops"][m]))[0]
        changed += len(d)
        if len(d):
            u = d[np.argmin(np.minimum(g["t_complete"][m][d], g0["t_complete"][m][d]))]
            proven += int(pub) not in col[row[u]:row[u + 1]]
    return changed, proven
