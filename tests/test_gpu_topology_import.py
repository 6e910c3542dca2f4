"""A caller's peer graph on the device (gs_set_topology, gs_set_topology_dials):
the imported CSR against the numpy helper, and everything downstream of it (mesh, runs, churn,
traffic, the metrics switches, partitioned runs, the checkpoint, the CLI) against the CPU oracle,
which has always taken an arbitrary graph. Each case asserts from the oracle what makes it worth
running (a hub row, lost deliveries, IWANTs, ...)."""
import os
import subprocess

import numpy as np
import pytest

import gossipsim
import mesh_ref
import oracle
import pubsub_ref as PS
import topo_ref as T

pytestmark = pytest.mark.gpu

T0 = gossipsim.T0_NS
UND = np.iinfo(np.uint64).max
LINKS = (5, (50, 150, 40, 130))
STATS = ("deliveries", "frag_deliveries", "relaxations", "bytes_alg", "latency_sum_ms", "latency_max_ms", "messages",
         "gossip_iwant")
_REF = {}


def _knobs(p):
    return {n: getattr(p, n) for n, _ in oracle.OrParams._fields_}


def params(name, **kw):
    N = T.graph(name)[0]
    return oracle.params_for("go", peers=N, seed=7, **kw) if name == "G6" else oracle.params(peers=N, seed=7, **kw)


def sched_of(name, M=4):
    N, _, _, pubs = T.graph(name)
    return T0 + np.arange(M, dtype=np.uint64) * np.uint64(1_000_000_000), np.asarray(pubs[:M]), np.full(M, 15000)


def ref_of(name, **kw):
    """The oracle on graph `name` (computed once, read-only): CSR of the helper, mesh, one frozen run."""
    key = (name, tuple(sorted(kw.items())))
    if key not in _REF:
        N, d, t, _ = T.graph(name)
        p = params(name, **kw)
        row, col, fl = T.dials_to_csr(N, d, t)
        lat, bw = oracle.topogen_links(LINKS[0], *LINKS[1])
        stage = (np.arange(N) % LINKS[0]).astype(np.uint8)
        flags, mesh, cnt, ep = oracle.mesh_converge(p, row, col, fl, stage, lat)
        sched = sched_of(name)
        tr = np.zeros((N, oracle.TR_COLS), np.uint64)
        tc, hops, st = oracle.run(p, row, col, mesh, cnt, stage, lat, bw, bw, *sched, traffic=tr)
        _REF[key] = dict(p=p, row=row, col=col, flags0=fl, flags=flags, mesh=mesh, cnt=cnt, epochs=ep, lat=lat, bw=bw,
                         stage=stage, sched=sched, t_complete=tc, hops=hops, stats=st, traffic=tr, dials=(d, t))
        for v in _REF[key].values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return _REF[key]


def new_sim(p, batch=8):
    sim = gossipsim.Simulator(batch=batch, **_knobs(p))
    sim.set_topogen_links(LINKS[0], *LINKS[1])
    return sim


def imported(r, how="dials", batch=8):
    sim = new_sim(r["p"], batch)
    if how == "dials":
        sim.set_dials(*r["dials"])
    else:
        sim.set_topology(r["row"], r["col"], r["flags0"])
    return sim


def same_csr(sim, row, col, flags, mask=0xFF):
    r, c, f = sim.csr()
    np.testing.assert_array_equal(r, row, err_msg="row_ptr")
    np.testing.assert_array_equal(c, col, err_msg="col")
    np.testing.assert_array_equal(f & mask, flags & mask, err_msg="flags")
    deg = np.diff(row.astype(np.int64))
    assert sim.graph_info() == (len(row) - 1, len(col), int(deg.max()))


def same_run(sim, r):
    assert sim.mesh_converge() == r["epochs"]
    same_csr(sim, r["row"], r["col"], r["flags"])
    mesh, cnt = sim.mesh()
    np.testing.assert_array_equal(cnt, r["cnt"], err_msg="mesh count")
    np.testing.assert_array_equal(mesh, r["mesh"], err_msg="mesh")
    res = sim.run(r["sched"])
    np.testing.assert_array_equal(res["t_complete"], r["t_complete"], err_msg="t_complete")
    np.testing.assert_array_equal(res["hops"], r["hops"], err_msg="hops")
    st = sim.stats()
    for k in STATS:
        assert st[k] == r["stats"][k], k
    return res


# ---- 1. oracle parity ----
CASES = [("G1", "dials", {}), ("G1", "dials", dict(fragments=3)), ("G2", "dials", {}), ("G2", "csr", {}),
         ("G3", "dials", {}), ("G3", "csr", {}), ("G4", "dials", {}), ("G5", "csr", {}), ("G6", "dials", {})]


@pytest.mark.parametrize("name,how,kw", CASES, ids=["%s-%s%s" % (n, h, "-f3" if k else "") for n, h, k in CASES])
def test_oracle_parity(name, how, kw):
    r = ref_of(name, **kw)
    deg = np.diff(r["row"].astype(np.int64))
    und = int((r["t_complete"] == UND).sum())
    if name == "G1":
        assert len(r["col"]) == 2972 and (deg.min(), deg.max()) == (7, 15) and r["epochs"] > 7 and und == 0
    if name in ("G2", "G3"):  # a row past the 64-entry forms, a long convergence, IWANTs
        assert deg.max() == 202 and deg.min() == 4 and r["epochs"] > 100 and r["stats"]["gossip_iwant"] > 0 and und == 0
    if name == "G4":  # nothing crosses to the other component
        assert und == 400 and r["cnt"].min() >= 4
    if name == "G5":
        assert deg.max() == 2 and r["cnt"].max() < r["p"].d_lo and und == 0 and r["hops"].max() == 39
    if name == "G6":
        assert r["p"].node == 1 and r["p"].idontwant == 1000 and und == 0
    sim = imported(r, how)
    same_csr(sim, r["row"], r["col"], r["flags0"])
    same_run(sim, r)


# ---- 2. round trips ----
def test_round_trips(tmp_path):
    p = oracle.params(peers=257, seed=5)
    sched = (T0 + np.arange(4, dtype=np.uint64) * np.uint64(1_000_000_000), np.array([6, 7, 150, 256]), np.full(4, 15000))
    a = new_sim(p)
    a.connect_gossipsub_peers()
    ep = a.mesh_converge()
    row, col, flags = a.csr()
    assert (flags & 2).any()  # taken after the converge: the mesh bit is set, and is not read
    ra = a.run(sched)
    b = new_sim(p)
    b.set_topology(row, col, flags)
    same_csr(b, row, col, flags, mask=1)
    assert not (b.csr()[2] & 2).any()
    assert b.mesh_converge() == ep
    same_csr(b, row, col, flags)
    for x, y in zip(a.mesh(), b.mesh()):
        np.testing.assert_array_equal(x, y)
    rb = b.run(sched)
    for k in ("t_complete", "hops"):
        np.testing.assert_array_equal(ra[k], rb[k])
    # the dials the F_OUT bits name, in any order, give the same CSR
    d, t = T.csr_to_dials(row, col, flags)
    assert len(d) == int((flags & 1).sum()) > len(col) // 2  # (mutual dials: more dials than connections)
    perm = np.random.default_rng(1).permutation(len(d))
    c = new_sim(p)
    c.set_dials(d[perm], t[perm])
    same_csr(c, row, col, flags, mask=1)
    # and through the text file
    path = tmp_path / "dials.txt"
    gossipsim.write_dials(path, row, col, flags)
    d2, t2 = gossipsim.read_dials(path)
    np.testing.assert_array_equal(d2, d)
    np.testing.assert_array_equal(t2, t)
    c.set_dials(d2, t2)
    same_csr(c, row, col, flags, mask=1)


# ---- 3. churn and traffic on G1 ----
def test_churn_on_an_imported_graph():
    N, d, t, _ = T.graph("G1")
    r0 = ref_of("G1")
    p = params("G1", churn_ppm=10000, hb_phase_ns=gossipsim.SHADOW_START_NS)
    sched = r0["sched"]
    h_lo = min(oracle.epoch_at(p, x) for x in sched[0])
    h_hi = max(oracle.epoch_at(p, x) for x in sched[0]) + p.churn_horizon
    snaps = oracle.mesh_churn(p, r0["row"], r0["col"], r0["flags0"], r0["stage"], r0["lat"], h_lo, h_hi)
    tr = np.zeros((N, oracle.TR_COLS), np.uint64)
    tc, hops, st = oracle.run_churn(p, r0["row"], r0["col"], snaps, h_lo, r0["stage"], r0["lat"], r0["bw"], r0["bw"],
                                    *sched, traffic=tr)
    assert (tc == UND).sum() > 0 and st["gossip_iwant"] > 0
    sim = new_sim(p)
    sim.set_dials(d, t)
    sim.mesh_converge()
    sim.set_traffic(True)
    res = sim.run(sched)
    np.testing.assert_array_equal(res["t_complete"], tc)
    np.testing.assert_array_equal(res["hops"], hops)
    got = sim.stats()
    for k in STATS:
        assert got[k] == st[k], k
    np.testing.assert_array_equal(sim.traffic(), tr)


def test_frozen_traffic_on_an_imported_graph():
    r = ref_of("G1")
    sim = imported(r)
    sim.mesh_converge()
    sim.set_traffic(True)
    sim.run(r["sched"])
    np.testing.assert_array_equal(sim.traffic(), r["traffic"])


# ---- 4. row-length edges of the dial builder ----
def _star(ends):
    """Peer 0 with `ends` dial ends: it dials 1..k, and the first ends - k of them dial back."""
    k = min(ends, 256)
    pairs = [(0, v) for v in range(1, k + 1)] + [(v, 0) for v in range(1, ends - k + 1)]
    n = k + 1
    return n, pairs


@pytest.mark.parametrize("ends,wave", [(63, 1), (64, 1), (65, 1), (128, 1), (256, 1), (512, 1), (65, 0), (512, 0)])
def test_row_lengths(monkeypatch, ends, wave):
    """Rows up to 64 dial ends sort a thread per row, longer ones a wave per row; with
    GS_IMPORT_WAVE_ROWS=0 the thread-per-row kernel takes the long rows too."""
    if not wave:
        monkeypatch.setenv("GS_IMPORT_WAVE_ROWS", "0")
    n, pairs = _star(ends)
    N = n + 5
    pairs += [(v, v + 1) for v in range(n - 1, N - 1)]  # a tail, so other rows are short
    d, t = T._dials(pairs)
    perm = np.random.default_rng(ends).permutation(len(d))
    sim = new_sim(oracle.params(peers=N, seed=7))
    sim.set_dials(d[perm], t[perm])
    row, col, flags = T.dials_to_csr(N, d, t)
    assert row[1] == min(ends, 256) and int(flags[:int(row[1])].sum()) == min(ends, 256)
    same_csr(sim, row, col, flags)


def test_degree_limits_and_the_smallest_graph():
    sim = new_sim(oracle.params(peers=300, seed=7))
    d, t = T._dials([(v, 0) for v in range(1, 257)] + [(v, v + 1) for v in range(256, 299)])
    sim.set_dials(d, t)  # exactly 256 connections
    assert sim.graph_info()[2] == 256
    same_csr(sim, *T.dials_to_csr(300, d, t))
    row, col, flags = sim.csr()
    sim.set_topology(row, col, flags)
    d, t = T._dials([(v, 0) for v in range(1, 258)] + [(v, v + 1) for v in range(257, 299)])
    with pytest.raises(gossipsim.GossipSimError, match="GS_EUNSUPPORTED.*256"):
        sim.set_dials(d, t)
    with pytest.raises(gossipsim.GossipSimError, match="GS_EUNSUPPORTED.*256"):
        sim.set_topology(*T.dials_to_csr(300, d, t))
    d, t = T._dials([(v, 0) for v in range(1, 258)] + [(0, v) for v in range(1, 257)] + [(v, v + 1) for v in range(257, 299)])
    with pytest.raises(gossipsim.GossipSimError, match="GS_EUNSUPPORTED.*512 dial ends at peer 0"):
        sim.set_dials(d, t)  # 513 ends: refused from the count
    same_csr(sim, row, col, flags)
    two = new_sim(oracle.params(peers=2, connect_to=1, seed=7))
    two.set_dials([1], [0])
    same_csr(two, np.array([0, 1, 2], np.uint64), np.array([1, 0], np.uint32), np.array([0, 1], np.uint8))


# ---- 5. defects ----
def _csr_case(kind):
    N, d, t, _ = T.graph("G1")
    row, col, fl = (x.copy() for x in T.dials_to_csr(N, d, t))
    if kind == "row0":
        row[0] = 1
        return (row, col, fl), "row_ptr\\[0\\]"
    if kind == "monotone":
        row[10] = row[11] + 1
        return (row, col, fl), "not monotone at peer 10"
    if kind == "range":
        col[int(row[20]) + 1] = N
        return (row, col, fl), "id >= peers at entry %d" % (row[20] + 1)
    if kind == "self":
        e = int(row[20])
        col[e] = 20
        return (row, col, fl), "self-loop at entry %d" % e
    if kind == "order":
        e = int(row[30])
        col[e], col[e + 1] = col[e + 1], col[e]
        fl[e], fl[e + 1] = fl[e + 1], fl[e]
        return (row, col, fl), "not strictly ascending at entry %d" % (e + 1)
    if kind in ("reverse", "alone"):  # drop an entry (u, w): w's entry loses its reverse ...
        e = int(row[40])
        if kind == "alone":  # ... or every entry of peer 40, and theirs: a peer with no connection
            keep = np.ones(len(col), bool)
            keep[int(row[40]):int(row[41])] = False
            rows = np.repeat(np.arange(N), np.diff(row.astype(np.int64)))
            keep &= col != 40
            cnt = np.bincount(rows[keep], minlength=N)
            row2 = np.zeros(N + 1, np.uint64)
            row2[1:] = np.cumsum(cnt)
            return (row2, col[keep], fl[keep]), "no connection\\) at peer 40"
        w = int(col[e])
        keep = np.ones(len(col), bool)
        keep[e] = False
        row[41:] -= 1
        col, fl = col[keep], fl[keep]
        back = int(row[w]) + int(np.searchsorted(col[int(row[w]):int(row[w + 1])], 40))
        assert col[back] == 40
        return (row, col, fl), "without its reverse at entry %d" % back
    if kind == "dialer":
        e = int(row[50]) + 2
        w = int(col[e])
        back = int(row[w]) + int(np.searchsorted(col[int(row[w]):int(row[w + 1])], 50))
        fl[e] = fl[back] = 0
        return (row, col, fl), "without a dialer.* at entry %d" % min(e, back)
    raise KeyError(kind)


def _dial_case(kind):
    N, d, t, _ = T.graph("G1")
    d, t = d.copy(), t.copy()
    if kind == "range":
        t[[700, 900]] = N
        return (d, t), "id >= peers at dial 700"
    if kind == "self":
        t[[33, 800]] = d[[33, 800]]
        return (d, t), "dialer == target at dial 33"
    if kind == "repeat":  # the later dial of the pair is the repeat
        d = np.concatenate([d[:500], d[100:101], d[500:], d[7:8]])
        t = np.concatenate([t[:500], t[100:101], t[500:], t[7:8]])
        return (d, t), "same ordered pair twice at dial 500"
    if kind == "alone":
        keep = (d != 77) & (t != 77)
        return (d[keep], t[keep]), "in no dial\\) at peer 77"
    raise KeyError(kind)


DEFECTS = [("csr", k) for k in ("row0", "monotone", "range", "self", "order", "reverse", "dialer", "alone")] + \
    [("dials", k) for k in ("range", "self", "repeat", "alone")]


@pytest.mark.parametrize("how,kind", DEFECTS, ids=["%s-%s" % x for x in DEFECTS])
def test_defects_leave_the_context_as_it_was(how, kind):
    r = ref_of("G1")
    sim = imported(r)
    sim.mesh_converge()
    before = sim.run(r["sched"])
    args, msg = (_csr_case if how == "csr" else _dial_case)(kind)
    with pytest.raises(gossipsim.GossipSimError, match="GS_EINVAL.*" + msg):
        (sim.set_topology if how == "csr" else sim.set_dials)(*args)
    same_csr(sim, r["row"], r["col"], r["flags"])
    after = sim.run(r["sched"])  # no converge needed: the mesh is still there
    for k in ("t_complete", "hops"):
        np.testing.assert_array_equal(after[k], before[k])
        np.testing.assert_array_equal(after[k], r[k])


def test_python_checks_arrays_before_the_call():
    r = ref_of("G5")
    sim = new_sim(r["p"])
    with pytest.raises(ValueError):
        sim.set_topology(r["row"][:-1], r["col"], r["flags0"])
    with pytest.raises(ValueError):
        sim.set_topology(r["row"], r["col"][:-1], r["flags0"][:-1])
    with pytest.raises(TypeError):
        sim.set_topology(r["row"], r["col"].astype(np.float64), r["flags0"])
    with pytest.raises(ValueError):
        sim.set_dials([1, 2], [0])
    with pytest.raises(ValueError):
        sim.set_dials([-1], [0])
    with pytest.raises(TypeError):
        sim.set_dials([0.5], [1])
    with pytest.raises(gossipsim.GossipSimError, match="GS_ESTATE"):
        sim.csr()  # none of these reached the library


# ---- 6. lifecycle ----
def test_lifecycle(tmp_path):
    r = ref_of("G1")
    sim = imported(r)
    with pytest.raises(gossipsim.GossipSimError, match="GS_ESTATE"):
        sim.run(r["sched"])
    same_run(sim, r)
    sim.set_topology(r["row"], r["col"], r["flags"])  # an import after a converge: converge again first
    with pytest.raises(gossipsim.GossipSimError, match="GS_ESTATE"):
        sim.run(r["sched"])
    with pytest.raises(gossipsim.GossipSimError, match="GS_ESTATE"):
        sim.mesh()
    sim.reset_stats()
    same_run(sim, r)
    # checkpoint of the imported, converged graph
    sim.save_state(tmp_path / "g1.state")
    back = gossipsim.Simulator.load_state(tmp_path / "g1.state")
    same_csr(back, r["row"], r["col"], r["flags"])
    res = back.run(r["sched"])
    np.testing.assert_array_equal(res["t_complete"], r["t_complete"])
    np.testing.assert_array_equal(res["hops"], r["hops"])
    # the builder after an import gives the built graph again
    built = new_sim(r["p"])
    built.connect_gossipsub_peers()
    ep = built.mesh_converge()
    want = built.run(r["sched"])
    sim.connect_gossipsub_peers()
    with pytest.raises(gossipsim.GossipSimError, match="GS_ESTATE"):
        sim.run(r["sched"])
    assert sim.mesh_converge() == ep
    same_csr(sim, *built.csr())
    got = sim.run(r["sched"])
    np.testing.assert_array_equal(got["t_complete"], want["t_complete"])
    # a larger graph over a converged one, saved before its own converge (no stale per-entry arrays)
    N = r["p"].peers
    d, t = T._dials(T.ring_dials(N, range(1, 13)))
    wide = T.dials_to_csr(N, d, t)
    assert len(wide[1]) > sim.graph_info()[1] > len(r["col"])
    sim.set_dials(d, t)
    sim.save_state(tmp_path / "wide.state")
    back = gossipsim.Simulator.load_state(tmp_path / "wide.state")
    same_csr(back, *wide)
    assert back.mesh_converge() == sim.mesh_converge()
    for x, y in zip(back.mesh(), sim.mesh()):
        np.testing.assert_array_equal(x, y)


def test_import_over_a_churn_run_with_other_row_widths():
    """A context that ran churn on narrow rows (the mask ring) takes the hub graph, and back."""
    kw = dict(churn_ppm=10000, hb_phase_ns=gossipsim.SHADOW_START_NS)
    p = oracle.params(peers=260, seed=7, **kw)
    lat, bw = oracle.topogen_links(LINKS[0], *LINKS[1])
    stage = (np.arange(260) % LINKS[0]).astype(np.uint8)
    sched = sched_of("G2")
    h_lo = min(oracle.epoch_at(p, x) for x in sched[0])
    h_hi = max(oracle.epoch_at(p, x) for x in sched[0]) + p.churn_horizon
    sim = new_sim(p)
    narrow = T._dials(T.ring_dials(260, (1, 2, 5)))
    for d, t in (narrow, T.graph("G2")[1:3], narrow):
        row, col, fl = T.dials_to_csr(260, d, t)
        snaps = oracle.mesh_churn(p, row, col, fl, stage, lat, h_lo, h_hi)
        tc, hops, st = oracle.run_churn(p, row, col, snaps, h_lo, stage, lat, bw, bw, *sched)
        sim.set_dials(d, t)
        sim.mesh_converge()
        sim.reset_stats()
        res = sim.run(sched)
        np.testing.assert_array_equal(res["t_complete"], tc)
        np.testing.assert_array_equal(res["hops"], hops)
        assert sim.stats()["gossip_iwant"] == st["gossip_iwant"]


# ---- 7. the metrics switches on an imported graph ----
def test_switches_on_the_hub_graph():
    r = ref_of("G2")
    sim = imported(r, "csr")
    sim.set_mesh_events()
    sim.set_pubsub_counts()
    sim.set_peer_delay()
    assert sim.mesh_converge() == r["epochs"]
    mesh_ref.check_identities(sim.mesh_events(), sim.mesh_series())
    res = sim.run(r["sched"])
    np.testing.assert_array_equal(res["t_complete"], r["t_complete"])
    st, pc = sim.stats(), sim.pubsub_counts().astype(np.int64)
    assert pc[:, PS.MSG_TX].sum() == pc[:, PS.MSG_RX].sum() == st["relaxations"] == r["stats"]["relaxations"]
    assert pc[:, PS.FIRST].sum() == st["frag_deliveries"] == r["stats"]["frag_deliveries"]
    assert pc[:, PS.IWANT_TX].sum() == st["gossip_iwant"] == r["stats"]["gossip_iwant"] > 0
    assert int(sim.peer_delay()["completed"].sum()) == st["deliveries"] == r["stats"]["deliveries"]


# ---- 8. partitioned ----
@pytest.mark.parametrize("parts", [2, 3])
def test_partitioned_on_an_imported_graph(parts):
    r = ref_of("G1")
    sims = [imported(r, "dials" if i % 2 else "csr") for i in range(parts)]
    for s in sims:
        s.mesh_converge()
    comm = gossipsim.Comm(local_parts=parts)
    res = comm.run_partitioned(sims, r["sched"])
    np.testing.assert_array_equal(np.concatenate([x["t_complete"] for x in res], axis=1), r["t_complete"])
    np.testing.assert_array_equal(np.concatenate([x["hops"] for x in res], axis=1), r["hops"])
    assert sum(s.stats()["deliveries"] for s in sims) == r["stats"]["deliveries"]


def test_one_rccl_rank_on_an_imported_graph():
    """The ranks' configuration check with a fingerprint folded into its hashed word."""
    r = ref_of("G1")
    s = imported(r)
    s.mesh_converge()
    comm = gossipsim.Comm(nranks=1, rank=0, uid=gossipsim.Comm.get_id(), device=0)
    (res,) = comm.run_partitioned([s], r["sched"])
    np.testing.assert_array_equal(res["t_complete"], r["t_complete"])
    np.testing.assert_array_equal(res["hops"], r["hops"])
    comm.close()


def test_partitioned_refuses_two_graphs():
    r = ref_of("G1")
    d, t = r["dials"]
    chord = int(np.flatnonzero((t.astype(np.int64) - d.astype(np.int64)) % 300 > 3)[0])
    sims = [imported(r), new_sim(r["p"]), new_sim(r["p"])]
    sims[1].set_dials(np.delete(d, chord), np.delete(t, chord))
    sims[2].connect_gossipsub_peers()
    for s in sims:
        s.mesh_converge()
    comm = gossipsim.Comm(local_parts=2)
    for other in (1, 2):  # another import, and the built graph
        with pytest.raises(gossipsim.GossipSimError, match="GS_EINVAL.*same graph"):
            comm.run_partitioned([sims[0], sims[other]], r["sched"])
        assert sims[0].stats()["messages"] == 0  # before any batch


# ---- 9. the key's hop field ----
def test_a_path_longer_than_the_hop_field():
    N = 100
    p = oracle.params(peers=N, seed=7)
    sim = new_sim(p)
    sim.set_dials(np.arange(N - 1), np.arange(1, N))
    sim.mesh_converge()
    with pytest.raises(gossipsim.GossipSimError, match="GS_ERANGE"):
        sim.run((np.array([T0], np.uint64), np.array([0]), np.array([15000])))


# ---- 10. the CLI ----
def test_cli_topology_flags(tmp_path):
    exe = os.path.join(os.path.dirname(gossipsim.LIB_PATH), "gossipsim-node")
    r = ref_of("G1")
    gossipsim.write_dials(tmp_path / "g1.txt", r["row"], r["col"], r["flags0"])
    env = dict(os.environ, PEERS="300", CONNECTTO="10", GS_SEED="7", GS_BATCH="8")
    args = [exe, "-st", "5", "-bl", "50", "-bh", "150", "-ll", "40", "-lh", "130", "-s", "15000", "-m", "4",
            "--publisher", "6", "--rotation", "1", "--delay-ms", "1000"]
    subprocess.run(args + ["--topology", str(tmp_path / "g1.txt"), "--latencies", str(tmp_path / "lat"),
                           "--dump-topology", str(tmp_path / "dump")], env=env, check=True, timeout=60)
    assert open(tmp_path / "dump").read() == open(tmp_path / "g1.txt").read()
    sim = imported(r)
    sim.mesh_converge()
    sched = gossipsim.schedule_runsh(4, 300, 6, 1, T0, gossipsim.DELAY_NS, 15000)
    sim.write_latency_log(str(tmp_path / "py_lat"), sim.run(sched))
    assert sorted(open(tmp_path / "lat").read().splitlines()) == sorted(open(tmp_path / "py_lat").read().splitlines())
    # the dump of a built graph is write_dials of its CSR
    subprocess.run(args + ["--dump-topology", str(tmp_path / "built")], env=env, check=True, timeout=60)
    built = new_sim(r["p"])
    built.connect_gossipsub_peers()
    gossipsim.write_dials(tmp_path / "py_built", *built.csr())
    assert open(tmp_path / "built").read() == open(tmp_path / "py_built").read()
    bad = tmp_path / "bad.txt"
    bad.write_text("0 1\n1 1\n")
    out = subprocess.run(args + ["--topology", str(bad)], env=env, timeout=60, capture_output=True, text=True)
    assert out.returncode == 1 and "dialer == target at dial 1" in out.stderr
