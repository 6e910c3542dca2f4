"""A caller's mesh on the device (gs_set_mesh, gs_set_mesh_links; DESIGN.md §2.3 "A caller's mesh"):
the imported arrays against what a converge leaves, and every frozen-mesh run path downstream of
them (the list pass, the push path, in-pass gossip, IDONTWANT, traffic, the pubsub counts,
loop-back parts, the checkpoint, the CLI) against the CPU oracle, which has always taken an
arbitrary mesh. Hand-made meshes push the gossip-active paths harder than a converged mesh does;
each case asserts from the oracle what makes it worth running."""
import os
import subprocess

import numpy as np
import pytest

import gossipsim
import oracle
import pubsub_ref as PS
import topo_ref as T

pytestmark = pytest.mark.gpu

T0 = gossipsim.T0_NS
UND = np.iinfo(np.uint64).max
E = 0xFFFFFFFF
W = gossipsim.MESH_W
LINKS = (5, (50, 150, 40, 130))
STATS = ("deliveries", "frag_deliveries", "relaxations", "bytes_alg", "latency_sum_ms", "latency_max_ms", "messages",
         "gossip_iwant")
_G, _REF = {}, {}


def _knobs(p):
    return {n: getattr(p, n) for n, _ in oracle.OrParams._fields_}


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


# ---- graphs: the oracle's builder (the device builds the same one) or a ring lattice (imported) ----
def graph(name, **kw):
    """-> dict(p, row, col, fl0, built, flags, mesh, cnt: the converged mesh, stage, lat, bw)."""
    key = (name, tuple(sorted(kw.items())))
    if key not in _G:
        if name == "A":
            p = oracle.params(peers=200, connect_to=10, seed=7, **kw)
        elif name == "Ago":
            p = oracle.params_for("go", peers=200, connect_to=10, seed=7, **kw)
        elif name == "B":
            p = oracle.params(peers=64, connect_to=4, seed=7, **kw)
        else:  # "R64", "R140": every peer connected to its two ring neighbours
            p = oracle.params(peers=int(name[1:]), seed=7, **kw)
        N = p.peers
        if name[0] == "R":
            row, col, fl0 = T.dials_to_csr(N, *T._dials(T.ring_dials(N, (1,))))
        else:
            row, col, fl0 = oracle.build_topology(p)
        lat, bw = oracle.topogen_links(LINKS[0], *LINKS[1])
        stage = (np.arange(N) % LINKS[0]).astype(np.uint8)
        flags, mesh, cnt, _ = oracle.mesh_converge(p, row, col, fl0, stage, lat)
        _G[key] = _freeze(dict(p=p, row=row, col=col, fl0=fl0, built=name[0] != "R", flags=flags, mesh=mesh, cnt=cnt,
                               stage=stage, lat=lat, bw=bw, rows=np.repeat(np.arange(N), np.diff(row.astype(np.int64)))))
    return _G[key]


def mask_of(g, which):
    """The mesh `which` as a mask over the CSR's entries (both ends of every link)."""
    u, w = g["rows"], g["col"].astype(np.int64)
    conv = (g["flags"] & 2) != 0
    return {"conv": conv, "mod2": conv & ((u + w) % 2 == 0), "empty": np.zeros(len(w), bool),
            "all": np.ones(len(w), bool), "nonmesh3": ~conv & ((u + w) % 3 != 0)}[which]


def links_of(g, mask):
    m = mask & (g["rows"] < g["col"])
    return g["rows"][m].astype(np.uint32), g["col"][m].astype(np.uint32)


def rows_of(g, mask):
    """Mesh rows [N, MESH_W] ascending, EMPTY padded, and counts."""
    N = g["p"].peers
    cnt = np.bincount(g["rows"][mask], minlength=N)
    assert cnt.max(initial=0) <= W
    mesh = np.full((N, W), E, np.uint32)
    slot = np.arange(int(mask.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    mesh[g["rows"][mask], slot] = g["col"][mask]
    return mesh, cnt.astype(np.uint8)


BIG = 240000  # pubsub_ref splits a peer's bytes into copies and RPCs: it needs a large message (its docstring)


def sched_of(N, M=4, size=15000):
    return (T0 + np.arange(M, dtype=np.uint64) * np.uint64(1_000_000_000), (7 * np.arange(M)) % N, np.full(M, size))


def ref_of(name, which, size=15000, **kw):
    """The oracle on graph `name` with mesh `which` (computed once, read-only): one frozen run with traffic."""
    key = (name, which, size, tuple(sorted(kw.items())))
    if key not in _REF:
        g = graph(name, **kw)
        p, N = g["p"], g["p"].peers
        mask = mask_of(g, which)
        mesh, cnt = rows_of(g, mask)
        sched = sched_of(N, size=size)
        tr = np.zeros((N, oracle.TR_COLS), np.uint64)
        tc, hops, st = oracle.run(p, g["row"], g["col"], mesh, cnt, g["stage"], g["lat"], g["bw"], g["bw"], *sched,
                                  traffic=tr)
        _REF[key] = _freeze(dict(g=g, p=p, mask=mask, mesh=mesh, cnt=cnt, links=links_of(g, mask), sched=sched,
                                 flags=(g["fl0"] & 1) | (mask.astype(np.uint8) << 1), t_complete=tc, hops=hops, stats=st,
                                 traffic=tr, und=int((tc == UND).sum())))
    return _REF[key]


def pubsub_of(r):
    """pubsub_ref.reference on the case's mesh: its whole-run step (oracle.simulate, which converges a
    mesh of its own) is stood in for by the case's run; the per-message splits are the helper's."""
    if "pubsub" not in r:
        g = r["g"]
        whole = dict(row_ptr=g["row"], col=g["col"], mesh=r["mesh"], cnt=r["cnt"], stage=g["stage"], lat=g["lat"],
                     bw=g["bw"], t_complete=r["t_complete"], traffic=r["traffic"])
        keep = oracle.simulate
        oracle.simulate = lambda *a, **k: whole
        try:
            ref = PS.reference(r["p"], LINKS[0], LINKS[1], r["sched"])
        finally:
            oracle.simulate = keep
        assert ref["exact"]
        ref["counts"].setflags(write=False)
        r.setdefault("pubsub", ref["counts"])
    return r["pubsub"]


def new_sim(g, batch=8):
    """A context with links and the graph, no mesh."""
    sim = gossipsim.Simulator(batch=batch, **_knobs(g["p"]))
    sim.set_topogen_links(LINKS[0], *LINKS[1])
    if g["built"]:
        sim.connect_gossipsub_peers()
    else:
        sim.set_topology(g["row"], g["col"], g["fl0"])
    return sim


def imported(r, how, batch=8):
    sim = new_sim(r["g"], batch)
    if how == "ell":
        sim.set_mesh(r["mesh"], r["cnt"])
    else:
        sim.set_mesh_links(*r["links"])
    return sim


def same_mesh(sim, r):
    mesh, cnt = sim.mesh()
    np.testing.assert_array_equal(cnt, r["cnt"], err_msg="mesh count")
    np.testing.assert_array_equal(mesh, r["mesh"], err_msg="mesh")
    row, col, fl = sim.csr()
    np.testing.assert_array_equal(row, r["g"]["row"], err_msg="row_ptr")
    np.testing.assert_array_equal(col, r["g"]["col"], err_msg="col")
    np.testing.assert_array_equal(fl, r["flags"], err_msg="flags (F_OUT | F_MESH)")


def same_run(sim, r):
    sim.reset_stats()
    res = sim.run(r["sched"])
    np.testing.assert_array_equal(res["t_complete"], r["t_complete"], err_msg="t_complete")
    np.testing.assert_array_equal(res["hops"], r["hops"], err_msg="hops")
    st = sim.stats()
    for k in STATS:
        assert st[k] == r["stats"][k], k
    return res


# ---- 1. round trip ----
def test_round_trip(tmp_path):
    r = ref_of("A", "conv")
    assert r["und"] == 0 and r["stats"]["gossip_iwant"] == 0 and 4 <= r["cnt"].min() and r["cnt"].max() <= 8
    a = new_sim(r["g"])
    a.mesh_converge()
    same_mesh(a, r)  # (the converged mesh is the oracle's)
    m, c = a.mesh()
    ra = same_run(a, r)
    fa = a.csr()[2]
    path = tmp_path / "mesh.txt"
    gossipsim.write_mesh_links(path, m, c)
    la, lb = gossipsim.read_dials(path)
    assert len(la) == int(c.sum()) // 2 and (la < lb).all()
    for how in ("ell", "ell-nocount", "links"):
        b = new_sim(r["g"])
        with pytest.raises(gossipsim.GossipSimError, match="GS_ESTATE"):
            b.mesh()
        if how == "links":
            b.set_mesh_links(la, lb)
        else:
            b.set_mesh(m, c if how == "ell" else None)
        for x, y in zip(a.mesh(), b.mesh()):
            np.testing.assert_array_equal(x, y, err_msg=how)
        np.testing.assert_array_equal(b.csr()[2], fa, err_msg=how)
        same_mesh(b, r)
        rb = same_run(b, r)
        for k in ("t_complete", "hops"):
            np.testing.assert_array_equal(ra[k], rb[k], err_msg=how)
        assert {k: a.stats()[k] for k in STATS} == {k: b.stats()[k] for k in STATS}


# ---- 2. hand-made meshes against oracle.run ----
CASES = [("A", "mod2", {}, "links"), ("A", "mod2", dict(fragments=3), "ell"), ("A", "mod2", dict(fragments=4), "links"),
         ("Ago", "mod2", {}, "ell"), ("A", "empty", {}, "links"), ("A", "empty", {}, "ell"), ("B", "all", {}, "ell"),
         ("B", "nonmesh3", {}, "links"), ("R64", "all", {}, "ell")]


def _worth_running(name, which, kw, r):
    g, st, N = r["g"], r["stats"], r["p"].peers
    if which == "mod2":  # about half the converged links: holes that only IHAVE / IWANT fill, longer paths
        conv = ref_of(name, "conv", **kw)
        assert 0 < len(r["links"][0]) < len(conv["links"][0]) and r["cnt"].max() <= 8
        assert st["gossip_iwant"] > 0 and r["und"] == 0 and r["hops"].max() > conv["hops"].max()
        if name == "Ago":
            assert r["p"].node == 1 and r["p"].idontwant == 1000
    if which == "empty":  # flood publishing plus gossip only: every non-publisher still completes
        assert r["cnt"].max() == 0 and len(r["links"][0]) == 0 and st["gossip_iwant"] > 0 and r["und"] == 0
        assert st["deliveries"] == len(r["sched"][0]) * (N - 1)
    if name == "B" and which == "all":  # wider than D_hi, yet legal
        assert 9 <= r["cnt"].max() <= W and r["cnt"].max() > r["p"].d_hi and r["und"] == 0
        assert (r["cnt"] == np.diff(g["row"].astype(np.int64))).all() and st["gossip_iwant"] == 0
    if which == "nonmesh3":  # a sparse mesh beside the converged one: peers without any mesh link
        assert (r["cnt"] == 0).any() and (r["cnt"] > 0).any() and st["gossip_iwant"] > 0 and r["und"] == 0
        assert not (r["mask"] & mask_of(g, "conv")).any()
    if name == "R64":  # the ring as graph and mesh: no connection outside the mesh, the far side N / 2 hops away
        assert (r["cnt"] == 2).all() and r["hops"].max() == 32 and st["gossip_iwant"] == 0 and r["und"] == 0


@pytest.mark.parametrize("name,which,kw,how", CASES,
                         ids=["%s-%s%s-%s" % (n, m, "-f%d" % k["fragments"] if k else "", h) for n, m, k, h in CASES])
def test_hand_made_meshes(name, which, kw, how):
    r = ref_of(name, which, **kw)
    _worth_running(name, which, kw, r)
    sim = imported(r, how)
    same_mesh(sim, r)
    sim.set_traffic(True)
    sim.set_pubsub_counts()
    same_run(sim, r)
    np.testing.assert_array_equal(sim.traffic(), r["traffic"], err_msg="traffic")
    assert int(sim.pubsub_counts()[:, PS.IWANT_TX].sum()) == r["stats"]["gossip_iwant"]
    # the per-peer pubsub counts: the same schedule with messages large enough for the helper's split
    big = ref_of(name, which, size=BIG, **kw)
    assert (big["stats"]["gossip_iwant"] > 0) == (r["stats"]["gossip_iwant"] > 0)
    sim.set_pubsub_counts()  # (zeroes them)
    same_run(sim, big)
    want, got = pubsub_of(big), sim.pubsub_counts()
    for col, cname in enumerate(gossipsim.PUBSUB_COLS):
        np.testing.assert_array_equal(got[:, col], want[:, col], err_msg=cname)


def test_a_mesh_longer_than_the_hop_field():
    """The ring at N = 140: the far side is 70 hops away, past the key's 6-bit hop field. That is the
    run's GS_ERANGE as on any such graph, not the import's. On this ring every
    message needs 70 hops, so no shorter schedule fits either; the context is shown to go on working
    by taking a mesh on a lattice with chords next and running the schedule there."""
    g = graph("R140")
    mesh, cnt = rows_of(g, mask_of(g, "all"))
    sim = new_sim(g)
    sim.set_mesh(mesh, cnt)
    with pytest.raises(gossipsim.GossipSimError, match="GS_ERANGE.*hop"):
        sim.run(sched_of(140))
    with pytest.raises(gossipsim.GossipSimError, match="GS_ERANGE.*hop"):
        sim.run(sched_of(140, 1))
    np.testing.assert_array_equal(sim.mesh()[0], mesh)  # the mesh stands
    N = 140
    row, col, fl0 = T.dials_to_csr(N, *T._dials(T.ring_dials(N, (1, 2, 5))))
    rows = np.repeat(np.arange(N), np.diff(row.astype(np.int64)))
    m2 = np.full((N, W), E, np.uint32)
    m2[:, :6] = col.reshape(N, 6)
    p = g["p"]
    tc, hops, st = oracle.run(p, row, col, m2, np.full(N, 6, np.uint8), g["stage"], g["lat"], g["bw"], g["bw"],
                              *sched_of(N))
    assert hops.max() < 64 and (tc != UND).all()
    sim.set_topology(row, col, fl0)
    sim.set_mesh_links(rows[rows < col], col[rows < col])
    sim.reset_stats()
    res = sim.run(sched_of(N))
    np.testing.assert_array_equal(res["t_complete"], tc)
    np.testing.assert_array_equal(res["hops"], hops)


# ---- 3. the mesh is a function of the set of links ----
def test_order_freeness():
    r = ref_of("A", "mod2")
    a, b = r["links"]
    rng = np.random.default_rng(11)
    for k in range(3):
        perm, flip = rng.permutation(len(a)), rng.integers(0, 2, len(a)).astype(bool)
        pa, pb = np.where(flip, b, a)[perm], np.where(flip, a, b)[perm]
        assert flip.any() and not flip.all() and (perm != np.arange(len(a))).any()
        sim = new_sim(r["g"])
        sim.set_mesh_links(pa, pb)
        same_mesh(sim, r)
        same_run(sim, r)
        mesh = r["mesh"].copy()
        for u in range(len(mesh)):  # rows shuffled in place, inside the counted part
            n = int(r["cnt"][u])
            mesh[u, :n] = rng.permutation(mesh[u, :n])
        assert (mesh != r["mesh"]).any()
        sim = new_sim(r["g"])
        sim.set_mesh(mesh, r["cnt"] if k else None)
        same_mesh(sim, r)
        same_run(sim, r)


# ---- 4. defects ----
def _entry(g, u, w):
    e = int(g["row"][u]) + int(np.searchsorted(g["col"][int(g["row"][u]):int(g["row"][u + 1])], w))
    assert g["col"][e] == w
    return e


def _not_connected(g, u):
    nb = set(g["col"][int(g["row"][u]):int(g["row"][u + 1])].tolist()) | {u}
    return next(w for w in range(g["p"].peers) if w not in nb)


def _ell_case(kind):
    """-> (mesh, count), the message. Every case carries its defect at two places; the smaller is named."""
    r = ref_of("A", "mod2")
    g, N = r["g"], r["p"].peers
    mesh, cnt = r["mesh"].copy(), r["cnt"].copy()
    full = np.flatnonzero(cnt >= 2)
    u1, u2 = int(full[5]), int(full[40])
    if kind == "count":
        cnt[[u2, u1]] = [200, 17]
        return (mesh, cnt), "count > GS_MESH_W at peer %d" % u1
    if kind == "range":
        mesh[u1, 1], mesh[u2, 0] = N, N + 7
        return (mesh, cnt), "id >= peers at slot %d" % (u1 * W + 1)
    if kind == "empty-inside":  # EMPTY inside the counted part is an id >= peers
        mesh[u1, 0], mesh[u2, 0] = E, E
        return (mesh, cnt), "id >= peers at slot %d" % (u1 * W)
    if kind == "self":
        mesh[u1, 1], mesh[u2, 1] = u1, u2
        return (mesh, cnt), "peer in its own row at slot %d" % (u1 * W + 1)
    if kind == "noconn":
        mesh[u1, 0], mesh[u2, 1] = _not_connected(g, u1), _not_connected(g, u2)
        return (mesh, cnt), "not a connection at slot %d" % (u1 * W)
    if kind == "repeat":  # the later slot of the two
        mesh[u1, 1], mesh[u2, 1] = mesh[u1, 0], mesh[u2, 0]
        return (mesh, cnt), "same peer twice in a row at slot %d" % (u1 * W + 1)
    if kind == "asym":  # u drops w: w's entry of u is marked, its reverse is not
        ents = []
        for u in (u1, u2):
            w = int(mesh[u, 0])
            mesh[u, :cnt[u] - 1] = mesh[u, 1:cnt[u]]
            mesh[u, cnt[u] - 1] = E
            cnt[u] -= 1
            ents.append(_entry(g, w, u))
        return (mesh, cnt), "without its reverse at entry %d" % min(ents)
    if kind == "two-kinds":  # the kinds' order decides before the index: id >= peers outranks the self-loop
        mesh[u1, 0], mesh[u2, 1] = u1, N
        return (mesh, cnt), "id >= peers at slot %d" % (u2 * W + 1)
    if kind == "two-stages":  # a slot's defect outranks the missing reverse, whatever the indices
        a0, b0 = int(r["links"][0][0]), int(r["links"][1][0])  # the first link: b0 drops a0, a0's entry keeps its mark
        keep = mesh[b0, :cnt[b0]][mesh[b0, :cnt[b0]] != a0]
        mesh[b0, :cnt[b0]] = np.append(keep, E)
        cnt[b0] -= 1
        assert b0 != u2 and _entry(g, a0, b0) < u2 * W
        mesh[u2, 1] = mesh[u2, 0]
        return (mesh, cnt), "same peer twice in a row at slot %d" % (u2 * W + 1)
    raise KeyError(kind)


def _link_case(kind):
    r = ref_of("A", "mod2")
    g, N = r["g"], r["p"].peers
    a, b = (x.copy() for x in r["links"])
    if kind == "range":
        a[200], b[90] = N, N + 1
        return (a, b), "id >= peers at link 90"
    if kind == "self":
        b[[33, 150]] = a[[33, 150]]
        return (a, b), "a == b at link 33"
    if kind == "noconn":
        b[120], b[60] = _not_connected(g, int(a[120])), _not_connected(g, int(a[60]))
        return (a, b), "not a connection at link 60"
    if kind == "repeat":  # links 7 and 100 again, the second in the other orientation: the later of each pair repeats
        a2 = np.concatenate([a[:150], b[100:101], a[150:], a[7:8]])
        b2 = np.concatenate([b[:150], a[100:101], b[150:], b[7:8]])
        return (a2, b2), "same link twice at link 150"
    if kind == "two-kinds":
        a[10], b[10], b[250] = 5, 5, N
        return (a, b), "id >= peers at link 250"
    if kind == "two-stages":  # a link's own defect outranks a repeat before it
        a2, b2 = np.concatenate([a[:5], a[3:4], a[5:]]), np.concatenate([b[:5], b[3:4], b[5:]])
        b2[300] = a2[300]
        return (a2, b2), "a == b at link 300"
    raise KeyError(kind)


DEFECTS = [("ell", k) for k in ("count", "range", "empty-inside", "self", "noconn", "repeat", "asym", "two-kinds",
                                "two-stages")] + \
    [("links", k) for k in ("range", "self", "noconn", "repeat", "two-kinds", "two-stages")]


@pytest.fixture(scope="module")
def standing():
    """The two contexts every refusal is tried on: one with a converged mesh, one with none."""
    r = ref_of("A", "conv")
    with_mesh, without = new_sim(r["g"]), new_sim(r["g"])
    with_mesh.mesh_converge()
    return r, with_mesh, without


@pytest.mark.parametrize("how,kind", DEFECTS, ids=["%s-%s" % x for x in DEFECTS])
def test_defects_leave_the_context_as_it_was(standing, how, kind):
    r, with_mesh, without = standing
    args, msg = (_ell_case if how == "ell" else _link_case)(kind)
    for sim in (with_mesh, without):
        with pytest.raises(gossipsim.GossipSimError, match="GS_EINVAL.*" + msg + "$"):
            (sim.set_mesh if how == "ell" else sim.set_mesh_links)(*args)
    same_mesh(with_mesh, r)
    same_run(with_mesh, r)
    for call in (without.mesh, lambda: without.run(r["sched"])):
        with pytest.raises(gossipsim.GossipSimError, match="GS_ESTATE"):
            call()
    np.testing.assert_array_equal(without.csr()[2], r["g"]["fl0"])


def test_a_row_wider_than_the_ell(standing):
    r, with_mesh, without = standing
    g = r["g"]
    deg = np.diff(g["row"].astype(np.int64))
    assert deg.max() > W  # every connection of the CONNECTTO 10 graph: rows of up to 30
    for sim in (with_mesh, without):
        with pytest.raises(gossipsim.GossipSimError, match="GS_ERANGE.*mesh row exceeds GS_MESH_W"):
            sim.set_mesh_links(*links_of(g, mask_of(g, "all")))
    same_mesh(with_mesh, r)
    same_run(with_mesh, r)
    with pytest.raises(gossipsim.GossipSimError, match="GS_ESTATE"):
        without.mesh()


# ---- 5. state rules ----
def test_state_rules():
    r, conv = ref_of("A", "mod2"), ref_of("A", "conv")
    g = r["g"]
    sim = gossipsim.Simulator(batch=8, **_knobs(g["p"]))
    for call in (lambda: sim.set_mesh(r["mesh"], r["cnt"]), lambda: sim.set_mesh_links(*r["links"])):
        with pytest.raises(gossipsim.GossipSimError, match="GS_ESTATE.*gs_build_topology first"):
            call()
    sim.connect_gossipsub_peers()
    for call in (lambda: sim.set_mesh(r["mesh"], r["cnt"]), lambda: sim.set_mesh_links(*r["links"])):
        with pytest.raises(gossipsim.GossipSimError, match="GS_ESTATE.*gs_set_links first"):
            call()
    sim.set_topogen_links(LINKS[0], *LINKS[1])
    sim.set_mesh_events()
    sim.set_mesh(r["mesh"], r["cnt"])
    same_mesh(sim, r)
    for getter in (sim.mesh_events, sim.mesh_series):  # they describe a converge
        with pytest.raises(gossipsim.GossipSimError, match="GS_ESTATE"):
            getter()
    same_run(sim, r)
    # whatever undoes a converged mesh undoes an imported one
    for undo in (lambda: sim.set_topogen_links(LINKS[0], *LINKS[1]), sim.connect_gossipsub_peers,
                 lambda: sim.set_topology(g["row"], g["col"], g["fl0"])):
        undo()
        for call in (sim.mesh, lambda: sim.run(r["sched"])):
            with pytest.raises(gossipsim.GossipSimError, match="GS_ESTATE"):
                call()
        sim.set_mesh_links(*r["links"])
        same_mesh(sim, r)
    # a converge after an import starts from the empty mesh: the converged mesh of a fresh context
    fresh = new_sim(g)
    fresh.set_mesh_events()
    assert sim.mesh_converge() == fresh.mesh_converge()
    same_mesh(sim, conv)
    np.testing.assert_array_equal(sim.mesh_events(), fresh.mesh_events())
    np.testing.assert_array_equal(sim.mesh_series(), fresh.mesh_series())
    same_run(sim, conv)
    sim.set_mesh_links(*r["links"])  # and back
    same_run(sim, r)
    # under churn every epoch's mesh comes from the chain
    churn = gossipsim.Simulator(batch=8, **_knobs(oracle.params(peers=200, connect_to=10, seed=7, churn_ppm=10000)))
    churn.set_topogen_links(LINKS[0], *LINKS[1])
    churn.connect_gossipsub_peers()
    for call in (lambda: churn.set_mesh(r["mesh"], r["cnt"]), lambda: churn.set_mesh_links(*r["links"])):
        with pytest.raises(gossipsim.GossipSimError, match="GS_EUNSUPPORTED.*churn"):
            call()


# ---- 6. partitioned ----
def _joined(res, key):
    return np.concatenate([x[key] for x in res], axis=1)


@pytest.mark.parametrize("parts", [2, 3])
def test_partitioned_on_a_hand_made_mesh(parts):
    r = ref_of("A", "mod2")
    sims = [imported(r, "links" if i % 2 else "ell") for i in range(parts)]
    comm = gossipsim.Comm(local_parts=parts)
    res = comm.run_partitioned(sims, r["sched"])
    np.testing.assert_array_equal(_joined(res, "t_complete"), r["t_complete"])
    np.testing.assert_array_equal(_joined(res, "hops"), r["hops"])
    st = [s.stats() for s in sims]
    assert all(x["ms_batches"] > 0 for x in st)  # gossip-active batches: the message-sharded protocol
    one = imported(r, "ell")  # and gs_run itself
    got = same_run(one, r)
    np.testing.assert_array_equal(_joined(res, "t_complete"), got["t_complete"])


def test_partitioned_round_trip_on_the_peer_protocols():
    r = ref_of("A", "conv")
    src = new_sim(r["g"])
    src.mesh_converge()
    sims = [new_sim(r["g"]) for _ in range(2)]
    sims[0].set_mesh(*src.mesh())
    sims[1].set_mesh_links(*r["links"])
    comm = gossipsim.Comm(local_parts=2)
    res = comm.run_partitioned(sims, r["sched"])
    np.testing.assert_array_equal(_joined(res, "t_complete"), r["t_complete"])
    np.testing.assert_array_equal(_joined(res, "hops"), r["hops"])
    assert all(s.stats()["ms_batches"] == 0 for s in sims)
    assert sum(s.stats()["deliveries"] for s in sims) == r["stats"]["deliveries"]


def test_one_rccl_rank_on_an_imported_mesh():
    """The ranks' configuration check with the mesh's fingerprint folded into its hashed word."""
    r = ref_of("A", "mod2")
    s = imported(r, "links")
    comm = gossipsim.Comm(nranks=1, rank=0, uid=gossipsim.Comm.get_id(), device=0)
    (res,) = comm.run_partitioned([s], r["sched"])
    np.testing.assert_array_equal(res["t_complete"], r["t_complete"])
    np.testing.assert_array_equal(res["hops"], r["hops"])
    comm.close()


def test_partitioned_refuses_two_meshes():
    """The parts compare a fingerprint of the imported mesh; a converged (or loaded) mesh has none, so
    an import beside a converge of the same mesh is refused as well."""
    r = ref_of("A", "conv")
    a, b = r["links"]
    sims = [imported(r, "ell"), new_sim(r["g"]), new_sim(r["g"])]
    sims[1].set_mesh_links(a[1:], b[1:])  # one link less
    sims[2].mesh_converge()               # the same mesh, converged
    np.testing.assert_array_equal(sims[2].mesh()[0], sims[0].mesh()[0])
    comm = gossipsim.Comm(local_parts=2)
    for other in (1, 2):
        for pair in ([sims[0], sims[other]], [sims[other], sims[0]]):
            with pytest.raises(gossipsim.GossipSimError, match="GS_EINVAL.*same mesh"):
                comm.run_partitioned(pair, r["sched"])
        assert all(s.stats()["messages"] == 0 for s in sims)  # before any batch
    sims[1].set_mesh_links(a, b)  # no context is left mid-batch: the setters and a run go on
    sims[2].set_mesh(r["mesh"])
    for other in (1, 2):
        res = comm.run_partitioned([sims[0], sims[other]], r["sched"])
        np.testing.assert_array_equal(_joined(res, "t_complete"), r["t_complete"])


# ---- 7. checkpoint and CLI ----
def test_checkpoint_of_an_imported_mesh(tmp_path):
    r = ref_of("B", "nonmesh3")
    sim = imported(r, "links")
    sim.save_state(tmp_path / "m.state")
    back = gossipsim.Simulator.load_state(tmp_path / "m.state")
    same_mesh(back, r)
    same_run(back, r)
    same_run(sim, r)


def test_cli_mesh_flags(tmp_path):
    exe = os.path.join(os.path.dirname(gossipsim.LIB_PATH), "gossipsim-node")
    r = ref_of("A", "mod2")
    gossipsim.write_mesh_links(tmp_path / "mesh.txt", r["mesh"], r["cnt"])
    env = dict(os.environ, PEERS="200", CONNECTTO="10", GS_SEED="7", GS_BATCH="8")
    args = [exe, "-st", "5", "-bl", "50", "-bh", "150", "-ll", "40", "-lh", "130", "-s", "15000", "-m", "4",
            "--publisher", "0", "--rotation", "7", "--delay-ms", "1000"]
    # the file in another order and orientation: the dump is the mesh's own text
    a, b = gossipsim.read_dials(tmp_path / "mesh.txt")
    perm = np.random.default_rng(5).permutation(len(a))
    with open(tmp_path / "shuffled.txt", "w") as f:
        f.write("# the mesh at the end of the run\n")
        f.writelines("%d %d\n" % ((a[i], b[i]) if i % 2 else (b[i], a[i])) for i in perm)
    subprocess.run(args + ["--mesh", str(tmp_path / "shuffled.txt"), "--latencies", str(tmp_path / "lat"),
                           "--dump-mesh", str(tmp_path / "dump")], env=env, check=True, timeout=60)
    assert open(tmp_path / "dump").read() == open(tmp_path / "mesh.txt").read()
    sched = gossipsim.schedule_runsh(4, 200, 0, 7, T0, gossipsim.DELAY_NS, 15000)
    sim = imported(r, "ell")
    res = sim.run(sched)
    np.testing.assert_array_equal(res["t_complete"], r["t_complete"])  # run.sh's schedule is the cases': the oracle's log
    sim.write_latency_log(str(tmp_path / "py_lat"), res)
    assert sorted(open(tmp_path / "lat").read().splitlines()) == sorted(open(tmp_path / "py_lat").read().splitlines())
    # --dump-mesh after a converge writes the converged mesh
    subprocess.run(args + ["--dump-mesh", str(tmp_path / "conv")], env=env, check=True, timeout=60)
    conv = ref_of("A", "conv")
    gossipsim.write_mesh_links(tmp_path / "py_conv", conv["mesh"], conv["cnt"])
    assert open(tmp_path / "conv").read() == open(tmp_path / "py_conv").read()
    for flag in ("--mesh-metrics", "--mesh-series"):
        out = subprocess.run(args + ["--mesh", str(tmp_path / "mesh.txt"), flag, str(tmp_path / "mm")], env=env,
                             timeout=60, capture_output=True, text=True)
        assert out.returncode == 2 and "--mesh" in out.stderr and flag in out.stderr
        assert not os.path.exists(tmp_path / "mm")
    bad = tmp_path / "bad.txt"
    bad.write_text("0 1\n3 3\n")
    out = subprocess.run(args + ["--mesh", str(bad)], env=env, timeout=60, capture_output=True, text=True)
    assert out.returncode == 1 and "a == b at link 1" in out.stderr
