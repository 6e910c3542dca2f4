"""Per-link first-delivery counts (gs_set_link_deliveries) on the device.

Exact cases compare all three columns of the link array and of peer_given with tests/link_ref.py,
a replay of DESIGN.md §2.5 that tests/test_link_deliveries_cpu.py proves against the oracle. The
cases the replay does not cover (fragments, IDONTWANT, IWANT answers) are checked by invariants
against the pubsub counts, the mesh and the oracle's rows."""
import numpy as np
import pytest

import gossipsim
import link_ref as R
import oracle

pytestmark = pytest.mark.gpu

FIRST = gossipsim.PUBSUB_COLS.index("first")
CHURN = dict(churn_ppm=20000, heartbeat_ns=200_000_000, hb_phase_ns=R.T0 - 2_000_000_000, churn_horizon=10)


def _knobs(p):
    return {n: getattr(p, n) for n, _ in oracle.OrParams._fields_}


def new_sim(p, batch=8):
    sim = gossipsim.Simulator(batch=batch, **_knobs(p))
    sim.set_topogen_links(R.STAGES, *R.LINKS)
    return sim


def gpu_sim(p, batch=8):
    sim = new_sim(p, batch)
    sim.connect_gossipsub_peers()
    sim.mesh_converge()
    return sim


def _part(sched, a, b):
    return tuple(x[a:b] for x in sched)


def _aligned(sim, g):
    """The counters are aligned with the CSR the reference counted over."""
    row, col, _ = sim.csr()
    np.testing.assert_array_equal(row, g["row_ptr"], err_msg="row_ptr")
    np.testing.assert_array_equal(col, g["col"], err_msg="col")


def _oracle_rows(res, g, m0=0, m1=None):
    np.testing.assert_array_equal(res["t_complete"], g["t_complete"][m0:m1], err_msg="t_complete")
    np.testing.assert_array_equal(res["hops"], g["hops"][m0:m1], err_msg="hops")


def _same(sim, r, what=""):
    edge, given = sim.link_deliveries(), sim.peer_given()
    assert edge.shape == r["edge"].shape and given.shape == r["given"].shape
    for k, name in enumerate(gossipsim.LINK_DELIVERY_COLS):
        np.testing.assert_array_equal(edge[:, k], r["edge"][:, k], err_msg="%s link %s" % (what, name))
        np.testing.assert_array_equal(given[:, k], r["given"][:, k], err_msg="%s given %s" % (what, name))


# ---- 1. exact cases ----
@pytest.mark.parametrize("name", sorted(R.BUILT))
def test_exact_on_built_graphs(name):
    """rust: the plain case; quiet: lazy gossip on, IHAVEs only; no_flood: the publisher's mesh sends
    are PUBLISH; n257_m1: a row count that is no multiple of the block's rows and L below a wave;
    n900_m12: two batches, so the counters carry."""
    p, sched, g, r = R.built(name)
    sim = gpu_sim(p, R.BUILT[name][2])
    sim.set_link_deliveries()
    assert not sim.link_deliveries().any() and not sim.peer_given().any()
    _oracle_rows(sim.run(sched), g)
    _aligned(sim, g)
    _same(sim, r, name)
    st = sim.stats()
    assert st["gossip_iwant"] == 0
    if name == "n900_m12":
        assert st["batches"] == 2
    if name == "quiet":
        assert p.lazy_gossip == 1


def test_exact_on_the_hub_graph():
    """Degree 202: a staged row and a histogram wider than a wave. The switch goes on before a graph
    exists; an import after a run zeroes the counters."""
    p, sched, g, r, dials = R.hub()
    sim = new_sim(p)
    sim.set_link_deliveries()  # no graph yet: the counters are allocated when first needed
    with pytest.raises(gossipsim.GossipSimError, match="GS_ESTATE"):
        sim.link_deliveries()
    with pytest.raises(gossipsim.GossipSimError, match="GS_ESTATE"):
        sim.peer_given()
    sim.set_dials(*dials)
    assert sim.graph_info()[2] == 202
    assert not sim.link_deliveries().any()
    sim.mesh_converge()
    _oracle_rows(sim.run(sched), g)
    _aligned(sim, g)
    _same(sim, r, "hub")
    sim.set_dials(*dials)  # the edge slots could mean other links now
    assert not sim.link_deliveries().any() and not sim.peer_given().any()
    sim.mesh_converge()
    sim.run(sched, collect=False)
    _same(sim, r, "hub again")
    sim.connect_gossipsub_peers()  # so does a built graph
    assert sim.link_deliveries().shape[0] == sim.graph_info()[1] and not sim.link_deliveries().any()


def test_exact_under_an_imported_empty_mesh():
    """Every delivery is PUBLISH, or nothing is delivered."""
    p, sched, g, r = R.empty_mesh()
    sim = new_sim(p)
    sim.connect_gossipsub_peers()
    sim.set_mesh(g["mesh"], g["cnt"])
    sim.set_link_deliveries()
    _oracle_rows(sim.run(sched), g)
    _aligned(sim, g)
    _same(sim, r, "empty mesh")
    edge = sim.link_deliveries()
    assert not edge[:, 1:].any() and int(edge[:, 0].sum()) == sim.stats()["frag_deliveries"] > 0


# ---- 2. invariants where the replay does not reach ----
def _rows_of(row):
    return np.repeat(np.arange(len(row) - 1), np.diff(row.astype(np.int64)))


def _in_mesh(sim, rows, col):
    mesh, cnt = sim.mesh()
    valid = np.arange(mesh.shape[1])[None, :] < cnt[:, None]
    return ((mesh[rows] == col[:, None]) & valid[rows]).any(axis=1)


def _column_invariants(sim, edge, pubs):
    row, col, _ = sim.csr()
    rows = _rows_of(row)
    inm = _in_mesh(sim, rows, col)
    assert inm[edge[:, R.MESH] > 0].all(), "a MESH entry is a mesh link of the receiver"
    assert not inm[edge[:, R.GOSSIP] > 0].any(), "a GOSSIP entry is no mesh link of the receiver"
    assert np.isin(col[edge[:, R.PUBLISH] > 0], pubs).all(), "a PUBLISH entry's sender is a publisher"
    return rows, col


@pytest.mark.parametrize("name", sorted(R.INVARIANT))
def test_invariants(name):
    """f3: groups of 4 lanes with a padding lane; go: IDONTWANT; gossip: IWANT answers that win."""
    p, sched, g = R.invariant(name)
    sim = gpu_sim(p)
    sim.set_link_deliveries()
    sim.set_pubsub_counts()
    _oracle_rows(sim.run(sched), g)
    edge = sim.link_deliveries()
    rows, col = _column_invariants(sim, edge, sched[1])
    per_peer = np.zeros(p.peers, np.uint64)
    np.add.at(per_peer, rows, edge.sum(axis=1))
    np.testing.assert_array_equal(per_peer, sim.pubsub_counts()[:, FIRST], err_msg="row sums == GS_PS_FIRST")
    np.testing.assert_array_equal(sim.peer_given(), R.transpose_sum(col, edge, p.peers))
    assert int(edge.sum()) == g["stats"]["frag_deliveries"] == sim.stats()["frag_deliveries"]
    if name == "gossip":
        assert min(R.gossip_winners()) > 0 and int(edge[:, R.GOSSIP].sum()) > 0
    if not p.lazy_gossip:
        assert int(edge[:, R.GOSSIP].sum()) == 0
    if name == "f3":
        assert p.fragments == 3 and int(edge.sum()) == 3 * g["stats"]["deliveries"]
    if name == "go":
        assert p.idontwant and R.SIZE >= p.idontwant


@pytest.mark.parametrize("name", ["go", "gossip"])
def test_one_parent_per_peer_and_message(name):
    """F = 1, one message per run() with a reset between: every peer the oracle completes has exactly
    one entry of count 1; its sender is one hop nearer and earlier in the oracle's rows, and the
    publisher's children are the peers at hop 1."""
    p, sched, g = R.invariant(name)
    assert p.fragments == 1
    sim = gpu_sim(p)
    sim.set_link_deliveries()
    row, col, _ = sim.csr()
    rows = _rows_of(row)
    for m in range(len(sched[0])):
        sim.reset_link_deliveries()
        _oracle_rows(sim.run(_part(sched, m, m + 1)), g, m, m + 1)
        edge = sim.link_deliveries()
        _column_invariants(sim, edge, sched[1][m:m + 1])
        pub, tc, hops = int(sched[1][m]), g["t_complete"][m], g["hops"][m].astype(np.int64)
        tot = edge.sum(axis=1)
        assert set(np.unique(tot)) <= {0, 1}
        hit = np.nonzero(tot)[0]
        done = np.nonzero((tc != R.UND) & (np.arange(p.peers) != pub))[0]
        np.testing.assert_array_equal(rows[hit], done)  # exactly one entry per completed peer, none elsewhere
        u, s = rows[hit], col[hit].astype(np.int64)
        assert (hops[s] + 1 == hops[u]).all() and (tc[s] < tc[u]).all()
        assert ((s == pub) == (hops[u] == 1)).all()
        assert ((s == pub) == (edge[hit, R.PUBLISH] == 1)).all()


# ---- 3. behaviour ----
def test_carry_resets_and_run_log():
    """2 + 2 messages: the counters carry across calls; both resets and enabling again zero them;
    run_log counts like run."""
    p, sched, g, r = R.built("rust")
    sim = gpu_sim(p)
    sim.set_link_deliveries()
    sim.run(_part(sched, 0, 2), collect=False)
    assert sim.link_deliveries().any()
    sim.run(_part(sched, 2, 4), collect=False)
    _same(sim, r, "2 + 2")
    sim.reset_link_deliveries()
    assert not sim.link_deliveries().any() and not sim.peer_given().any()
    sim.run(_part(sched, 0, 1), collect=False)
    assert sim.link_deliveries().any()
    sim.reset_stats()
    assert not sim.link_deliveries().any()
    sim.run_log(sched, on_text=lambda first, n, text, lines: None)
    _same(sim, r, "run_log")
    sim.set_link_deliveries()  # enabling zeroes
    assert not sim.link_deliveries().any()
    sim.run(sched, on_lat=lambda first, lat: None)
    _same(sim, r, "on_lat")
    sim.set_link_deliveries(False)
    with pytest.raises(gossipsim.GossipSimError, match="GS_ESTATE"):
        sim.link_deliveries()


def test_the_switch_changes_nothing_else():
    p, sched, _, _ = R.built("quiet")
    on, off = gpu_sim(p), gpu_sim(p)
    on.set_link_deliveries()
    a, b = on.run(sched), off.run(sched)
    np.testing.assert_array_equal(a["t_complete"], b["t_complete"])
    np.testing.assert_array_equal(a["hops"], b["hops"])
    assert on.stats() == off.stats()


def test_errors_and_state(tmp_path):
    p, sched, g, r = R.built("rust")
    sim = gpu_sim(p)
    with pytest.raises(gossipsim.GossipSimError, match="GS_ESTATE"):
        sim.link_deliveries()  # the switch is off
    with pytest.raises(gossipsim.GossipSimError, match="GS_ESTATE"):
        sim.peer_given()
    sim.set_link_deliveries()
    lib = gossipsim.lib()
    assert lib.gs_get_link_deliveries(sim.ctx, None) == gossipsim.GS_EINVAL
    assert lib.gs_get_peer_given(sim.ctx, None) == gossipsim.GS_EINVAL
    sim.run(sched, collect=False)
    sim.write_link_deliveries(tmp_path / "links")
    row, col, _ = sim.csr()
    rows = _rows_of(row)
    want = "".join("%d %d %d %d %d\n" % ((rows[e], col[e]) + tuple(int(x) for x in r["edge"][e]))
                   for e in np.nonzero(r["edge"].sum(axis=1))[0])
    assert (tmp_path / "links").read_text() == want
    sim.save_state(tmp_path / "state")
    loaded = gossipsim.Simulator.load_state(tmp_path / "state")
    with pytest.raises(gossipsim.GossipSimError, match="GS_ESTATE"):
        loaded.link_deliveries()  # a loaded context has the switch off
    churn = new_sim(oracle.params(peers=300, seed=71, **CHURN))
    with pytest.raises(gossipsim.GossipSimError, match="GS_EUNSUPPORTED.*gs_set_link_deliveries"):
        churn.set_link_deliveries()
    churn.set_link_deliveries(False)


def test_partitioned_mode_refuses_the_switch():
    """part_begin and run_partitioned name the switch; the contexts stay usable once it is off."""
    p, sched, g, _ = R.built("rust")
    sims = []
    for i in range(2):
        s = gpu_sim(p, batch=4)
        s.set_partition(2, i)
        s.set_link_deliveries()
        sims.append(s)
    with pytest.raises(gossipsim.GossipSimError, match="GS_EUNSUPPORTED.*gs_set_link_deliveries"):
        sims[0].part_begin(sched)
    comm = gossipsim.Comm(local_parts=2)
    with pytest.raises(gossipsim.GossipSimError, match="GS_EUNSUPPORTED.*gs_set_link_deliveries"):
        comm.run_partitioned(sims, sched)
    for s in sims:
        s.set_link_deliveries(False)
    out = comm.run_partitioned(sims, sched)
    np.testing.assert_array_equal(np.concatenate([o["t_complete"] for o in out], axis=1), g["t_complete"])
    comm.close()


def test_cli_link_deliveries(tmp_path):
    """gossipsim-node --link-deliveries: the file is write_link_deliveries() of the same run."""
    import os
    import subprocess
    exe = os.path.join(os.path.dirname(gossipsim.LIB_PATH), "gossipsim-node")
    N, M = 300, 4
    env = dict(os.environ, PEERS=str(N), CONNECTTO="10", GS_SEED="5", GS_BATCH="4")
    args = [exe, "-st", "5", "-bl", "50", "-bh", "150", "-ll", "40", "-lh", "130", "-m", str(M), "-s", str(R.SIZE)]
    subprocess.run(args + ["--link-deliveries", str(tmp_path / "a")], env=env, check=True, timeout=60)
    sim = gpu_sim(oracle.params(peers=N, seed=5), batch=4)
    sim.set_link_deliveries()
    sim.run(gossipsim.schedule_runsh(M, N, 6, 1, gossipsim.T0_NS, gossipsim.DELAY_NS, R.SIZE), collect=False)
    sim.write_link_deliveries(tmp_path / "py")
    text = (tmp_path / "a").read_text()
    assert text == (tmp_path / "py").read_text()
    rowsum = sum(sum(int(x) for x in line.split()[2:]) for line in text.splitlines())
    assert rowsum == sim.stats()["frag_deliveries"] == M * (N - 1)
