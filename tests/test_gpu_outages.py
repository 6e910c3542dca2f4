"""A caller's outages on the device (gs_set_outages, gs_clear_outages, gs_get_offline; DESIGN.md
§2.8 "A caller's outages"): who is offline when, in place of the churn draw.

The offline bitsets are all the epoch chain and the run read of churn, so three things pin the
import: the bitsets themselves through the getter (the draw's against oracle.offline, a
schedule's against outage_ref.table); the draw's own table imported as intervals, which must
give the draw's run and the oracle's bit for bit on every batch path; and a schedule no draw
can express, against oracle.run_churn on the device's own per-epoch meshes (run_churn reads the
snapshots and offline flags it is given, and converge(h) leaves snapshot h: both facts are
checked without a GPU in test_outages_cpu.py). Integer equality only."""
import os
import subprocess

import numpy as np
import pytest

import gossipsim
import oracle
import outage_ref

pytestmark = pytest.mark.gpu

T0 = gossipsim.T0_NS
UND = gossipsim.UNDELIVERED
FOREVER = gossipsim.OUTAGE_FOREVER
N, STAGES, LINKS = 300, 5, (50, 150, 40, 130)
HB = 400_000_000
PHASE = T0 - 30 * HB + 150_000_000  # a publish at T0 + i heartbeats falls into epoch 29 + i
M, BATCH, MAX_HB, H_TOP = 16, 8, 60, 60
COUNTERS = ("deliveries", "frag_deliveries", "relaxations", "bytes_alg", "latency_sum_ms", "latency_max_ms",
            "messages", "gossip_iwant")
ENV_KNOBS = ("GS_LPULL_CAP", "GS_LPULL_CAP_BATCHES", "GS_REQUIRE_LPULL", "GS_CHN_PIPE", "GS_CHURN_LIST")
SCHED = (T0 + np.arange(M, dtype=np.uint64) * np.uint64(HB), (6 + np.arange(M)) % N, np.full(M, 15000))


def _params(ppm, down, gossip=1, frags=1, peers=N, seed=59):
    return oracle.params(peers=peers, seed=seed, churn_ppm=ppm, churn_down=down, churn_horizon=10, heartbeat_ns=HB,
                         hb_phase_ns=PHASE, lazy_gossip=gossip, fragments=frags)


def _new(p, batch=BATCH, links=True):
    kw = {n: getattr(p, n) for n, _ in oracle.OrParams._fields_}
    kw["batch"] = batch
    sim = gossipsim.Simulator(**kw)
    if links:
        sim.set_topogen_links(STAGES, *LINKS)
        sim.connect_gossipsub_peers()
    return sim


def _oracle_table(p, h_hi, peers=N):
    return np.array([[oracle.offline(p, u, h) for u in range(peers)] for h in range(h_hi + 1)], bool)


def _arrays(intervals):
    if not intervals:
        return [], [], []
    return tuple(np.array(x, np.uint32) for x in zip(*intervals))


def _quiet(monkeypatch, **env):
    for k in ENV_KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


_CACHE = {}


def _cached(key, make):
    """Computed once per module, shared, never written."""
    if key not in _CACHE:
        v = make()
        for x in (v.values() if isinstance(v, dict) else v if isinstance(v, tuple) else ()):
            if isinstance(x, np.ndarray):
                x.setflags(write=False)
        _CACHE[key] = v
    return _CACHE[key]


def _draw_ref(gossip=1, frags=1):
    """oracle.simulate of the (30000, 6) draw with max_hb = 60."""
    return _cached(("draw", gossip, frags),
                   lambda: oracle.simulate(_params(30000, 6, gossip, frags), STAGES, LINKS, sched=SCHED, max_hb=MAX_HB))


def _draw_table():
    return _cached("table", lambda: (_oracle_table(_params(30000, 6), H_TOP),))[0]


def _draw_intervals():
    """The maximal intervals of the (30000, 6) table over epochs 1..60."""
    return outage_ref.maximal_intervals(_draw_table())


def _same_graph_and_mesh(sim, ref, ep):
    row, col, flags = sim.csr()
    np.testing.assert_array_equal(row, ref["row_ptr"], err_msg="row_ptr")
    np.testing.assert_array_equal(col, ref["col"], err_msg="col")
    mesh, cnt = sim.mesh()
    np.testing.assert_array_equal(cnt, ref["cnt"], err_msg="mesh count")
    np.testing.assert_array_equal(mesh, ref["mesh"], err_msg="mesh")
    np.testing.assert_array_equal(flags, ref["flags"], err_msg="flags")
    assert ep == ref["epochs"]


def _same_run(res, st, ref):
    np.testing.assert_array_equal(res["t_complete"], ref["t_complete"], err_msg="t_complete")
    np.testing.assert_array_equal(res["hops"], ref["hops"], err_msg="hops")
    for k in COUNTERS:
        assert st[k] == ref["stats"][k], k


# ---- 1. the draw through the getter ----
def test_the_draw_through_the_getter():
    p = _params(30000, 6, peers=130, seed=3)  # three words, the last with 2 live bits
    want = _oracle_table(p, 60, 130)
    assert want.sum() == 1259 and not want[0].any()
    sim = _new(p, links=False)
    got = sim.offline(0, 60)
    assert got.shape == (61, 130) and got.dtype == bool
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(sim.offline(23, 41), want[23:42])  # a range not starting at 0
    np.testing.assert_array_equal(sim.offline(37, 37), want[37:38])  # a single epoch
    # the raw words: bits at and past `peers` are 0
    bits = np.full(3 * 2, np.iinfo(np.uint64).max, np.uint64)
    sim._check(gossipsim.lib().gs_get_offline(sim.ctx, 36, 37, gossipsim._ptr(bits, gossipsim.u64)))
    assert (bits.reshape(2, 3)[:, 2] >> np.uint64(2) == 0).all()
    with pytest.raises(gossipsim.GossipSimError, match="GS_EINVAL"):
        sim.offline(5, 4)
    calm = _new(_params(0, 6, peers=130, seed=3), links=False)
    with pytest.raises(gossipsim.GossipSimError, match="GS_ESTATE"):
        calm.offline(0, 3)


# ---- 2. an imported schedule through the getter ----
HAND = [(0, 1, 2), (63, 3, 9), (64, 5, 6), (129, 7, FOREVER), (77, 10, 14), (77, 25, 30), (77, 14, 20)]


def test_a_schedule_through_the_getter():
    sim = _new(_params(30000, 6, peers=130, seed=3), links=False)
    tabs = {}
    for seed in (1, 2):
        order = np.random.default_rng(seed).permutation(len(HAND))
        sim.set_outages(*_arrays([HAND[i] for i in order]))
        for lo, hi in ((0, 0), (1, 40), (17, 17), (39, 200)):
            got = sim.offline(lo, hi)
            np.testing.assert_array_equal(got, outage_ref.table(130, HAND, lo, hi), err_msg="%d..%d" % (lo, hi))
            if seed == 2:  # a second shuffle gives the same tables
                np.testing.assert_array_equal(got, tabs[(lo, hi)])
            tabs[(lo, hi)] = got
    assert tabs[(1, 40)].sum() == 1 + 6 + 1 + 34 + 15 and tabs[(39, 200)][:, 129].all()
    # touching intervals given as their union are the same schedule
    merged = [x for x in HAND if x[0] != 77] + [(77, 10, 20), (77, 25, 30)]
    sim.set_outages(*_arrays(merged))
    np.testing.assert_array_equal(sim.offline(1, 40), tabs[(1, 40)])
    sim.clear_outages()  # and the draw is back
    assert sim.offline(1, 40).sum() != tabs[(1, 40)].sum()


# ---- 3. the draw, imported, is the draw and the oracle ----
def _imported(gossip=1, frags=1, events=False):
    """A (5, 2) context with the (30000, 6) draw's intervals imported, converged to epoch 60."""
    p = _params(5, 2, gossip, frags)
    sim = _new(p)
    if events:
        sim.set_mesh_events(True)
    assert not sim.offline(0, H_TOP).any()  # its own table is empty through epoch 60 ...
    assert not _cached("calm", lambda: (_oracle_table(p, H_TOP),))[0].any()  # ... as the oracle's
    iv = _draw_intervals()
    order = np.random.default_rng(7).permutation(len(iv))
    sim.set_outages(*_arrays([iv[i] for i in order]))
    np.testing.assert_array_equal(sim.offline(0, H_TOP), _draw_table())
    return sim, sim.mesh_converge(MAX_HB)


def test_the_case_is_not_empty():
    tab, iv = _draw_table(), _draw_intervals()
    assert tab.sum() == 2999 and len(iv) == 466
    per_peer = np.bincount([u for u, _, _ in iv], minlength=N)
    assert per_peer.max() == 4 and (per_peer > 1).sum() == 153  # peers that leave more than once
    off_at_pub = [bool(tab[29 + i, SCHED[1][i]]) for i in range(M)]
    assert sum(off_at_pub) == 4  # publishers that are offline at their t_pub
    ref = _draw_ref()
    for i in np.flatnonzero(off_at_pub):
        assert (ref["t_complete"][i] == UND).all()


@pytest.mark.parametrize("way", ["list", "push", "nogossip", "frags2"])
def test_the_draw_imported_against_the_oracle(monkeypatch, way):
    gossip, frags = (0 if way == "nogossip" else 1), (2 if way == "frags2" else 1)
    _quiet(monkeypatch, **({"GS_CHURN_LIST": "0"} if way == "push" else {"GS_REQUIRE_LPULL": "1"}))
    ref = _draw_ref(gossip, frags)
    sim, ep = _imported(gossip, frags)
    _same_graph_and_mesh(sim, ref, ep)
    res = sim.run(SCHED)
    st = sim.stats()
    print(way, {k: st[k] for k in ("batches", "list_pull_batches") + COUNTERS})
    _same_run(res, st, ref)
    assert st["batches"] == M // BATCH
    assert st["list_pull_batches"] == (0 if way == "push" else st["batches"])
    if gossip:
        assert st["gossip_iwant"] > 0
    sim.close()


def test_the_draw_imported_against_the_drawing_device(monkeypatch):
    """The same arrays, the mesh events of the converge and the pubsub counts from a context that
    draws (30000, 6) and from one that imports the draw's intervals."""
    _quiet(monkeypatch)
    out = []
    for imported in (False, True):
        if imported:
            sim, ep = _imported(events=True)
        else:
            sim = _new(_params(30000, 6))
            sim.set_mesh_events(True)
            ep = sim.mesh_converge(MAX_HB)
        sim.set_pubsub_counts(True)
        d = dict(ep=ep, csr=sim.csr(), mesh=sim.mesh(), events=sim.mesh_events(), series=sim.mesh_series(),
                 off=sim.offline(0, H_TOP))
        d["res"] = sim.run(SCHED)
        d["stats"] = sim.stats()
        d["pubsub"] = sim.pubsub_counts()
        out.append(d)
        sim.close()
    a, b = out
    assert a["ep"] == b["ep"]
    for x, y in zip(a["csr"] + a["mesh"], b["csr"] + b["mesh"]):
        np.testing.assert_array_equal(x, y)
    for k in ("events", "series", "off", "pubsub"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    assert a["series"].shape[0] == MAX_HB + 1 and a["events"].any() and a["pubsub"].any()
    _same_run(b["res"], b["stats"], dict(t_complete=a["res"]["t_complete"], hops=a["res"]["hops"], stats=a["stats"]))
    _same_run(a["res"], a["stats"], _draw_ref())


# ---- 4. the empty schedule ----
def test_the_empty_schedule(monkeypatch):
    """n = 0 on a (30000, 6) context: a churn context in which nobody leaves, the oracle at (5, 2),
    whose table is empty over the epochs used."""
    _quiet(monkeypatch)
    calm = _params(5, 2)
    assert not _cached("calm", lambda: (_oracle_table(calm, H_TOP),))[0].any()
    ref = _cached("calm_ref", lambda: oracle.simulate(calm, STAGES, LINKS, sched=SCHED, max_hb=MAX_HB))
    sim = _new(_params(30000, 6))
    assert sim.offline(0, H_TOP).any()
    sim.set_outages([], [], [])
    assert not sim.offline(0, H_TOP).any()
    _same_graph_and_mesh(sim, ref, sim.mesh_converge(MAX_HB))
    res = sim.run(SCHED)
    _same_run(res, sim.stats(), ref)
    assert not (res["t_complete"] == UND).any()
    sim.close()


# ---- 5. a what-if the draw cannot express ----
WHATIF = [(u, 33, 41) for u in range(40)] + [(u, 31, FOREVER) for u in range(100, 105)] + \
    [(200, 30, 32), (200, 32, 35), (200, 50, 52)]
H_LO, H_HI = 29, 54  # the epochs the schedule can use (t_pub's epoch .. the last one + churn_horizon)


def _whatif_table():
    return _cached("whatif_table", lambda: (outage_ref.table(N, WHATIF, 0, H_TOP),))[0]


def _whatif_sim(p=None):
    sim = _new(p if p is not None else _params(30000, 6))
    order = np.random.default_rng(3).permutation(len(WHATIF))
    sim.set_outages(*_arrays([WHATIF[i] for i in order]))
    return sim


def _whatif_ref():
    """oracle.run_churn over the device's own per-epoch meshes (converge(h) and mesh() for every epoch
    the run uses) and the reference table."""
    def make():
        p = _params(30000, 6)
        sim = _whatif_sim(p)
        tab = _whatif_table()
        np.testing.assert_array_equal(sim.offline(0, H_TOP), tab)
        row, col, _ = sim.csr()
        E = H_HI - H_LO + 1
        smesh = np.zeros((E, N, gossipsim.MESH_W), np.uint32)
        scnt = np.zeros((E, N), np.uint8)
        for h in range(H_LO, H_HI + 1):
            assert sim.mesh_converge(h) == h
            mesh, cnt = sim.mesh()
            off = tab[h]
            links = set()
            for u in range(N):
                assert (mesh[u, cnt[u]:] == 0xFFFFFFFF).all()
                links.update((u, int(w)) for w in mesh[u, :cnt[u]])
            assert cnt[off].sum() == 0, "epoch %d: an offline peer has mesh links" % h
            assert not any(off[w] for _, w in links), "epoch %d: a link to an offline peer" % h
            assert all((w, u) in links for u, w in links), "epoch %d: a link without its reverse" % h
            assert len(links) > N  # and the online peers do have a mesh
            smesh[h - H_LO], scnt[h - H_LO] = mesh, cnt
        sim.close()
        lat, bw = oracle.topogen_links(STAGES, *LINKS)
        stage = (np.arange(N) % STAGES).astype(np.uint8)
        soff = tab[H_LO:H_HI + 1].astype(np.uint8)
        tc, hops, stats = oracle.run_churn(p, row, col, (smesh, scnt, soff), H_LO, stage, lat, bw, bw, *SCHED)
        return dict(t_complete=tc, hops=hops, stats=stats)
    return _cached("whatif_ref", make)


@pytest.mark.parametrize("converge_to", [54, 20])
def test_a_whatif_against_the_oracle_on_the_devices_meshes(monkeypatch, converge_to):
    """After converge(54) the run replays the chain from epoch 0; after converge(20) the chain advances
    from the converged state."""
    _quiet(monkeypatch)
    ref = _whatif_ref()
    sim = _whatif_sim()
    assert sim.mesh_converge(converge_to) == converge_to
    res = sim.run(SCHED)
    st = sim.stats()
    _same_run(res, st, ref)
    assert st["gossip_iwant"] > 0
    # not vacuous: publishers 10..17 publish at epochs 33..40, inside the block's outage
    tab = _whatif_table()
    dead = [i for i in range(M) if tab[29 + i, SCHED[1][i]]]
    assert dead == list(range(4, 12))
    for i in dead:
        assert (res["t_complete"][i] == UND).all()
    alive = [i for i in range(M) if i not in dead]
    assert all((res["t_complete"][i] != UND).sum() > N // 2 for i in alive)
    calm = _cached("calm_ref", lambda: oracle.simulate(_params(5, 2), STAGES, LINKS, sched=SCHED, max_hb=MAX_HB))
    assert (res["t_complete"] == UND).sum() != (calm["t_complete"] == UND).sum()
    sim.close()


# ---- 6. refusals and state rules ----
def _big_row(peer, n):
    return [(peer, 1 + 2 * k, 2 + 2 * k) for k in range(n)]


REFUSALS = [
    ("range", [(1, 2, 3), (2, 2, 3), (N, 2, 3), (3, 2, 3), (N + 7, 1, 2)], "GS_EINVAL", "peer >= peers at interval 2"),
    ("zero", [(1, 2, 3), (4, 0, 3), (2, 0, 1)], "GS_EINVAL", "h_from == 0.*at interval 1"),
    ("empty", [(1, 2, 3), (1, 5, 5), (2, 9, 4)], "GS_EINVAL", "h_from >= h_to at interval 1"),
    ("overlap", [(5, 3, 8), (6, 1, 2), (5, 7, 9)], "GS_EINVAL", "share an epoch at interval 0"),
    ("overlap-late", [(6, 1, 2), (7, 3, 8), (5, 3, 8), (8, 1, 9), (5, 7, 9)], "GS_EINVAL",
     "share an epoch at interval 2"),
    ("overlap-twice", [(5, 3, 8), (5, 3, 8)], "GS_EINVAL", "share an epoch at interval 0"),
    # the interval that spans the others is neither first in the list nor next to the one it overlaps
    ("overlap-nested", [(9, 4, 5), (9, 2, 3), (1, 1, 2), (1, 2, 3), (9, 30, 31), (9, 1, 10)], "GS_EINVAL",
     "share an epoch at interval 0"),
    ("overlap-forever", [(9, 40, 41), (9, 4, FOREVER)], "GS_EINVAL", "share an epoch at interval 0"),
    ("kinds", [(5, 3, 8), (5, 7, 9), (4, 9, 9), (N, 1, 2)], "GS_EINVAL", "peer >= peers at interval 3"),
    ("row", _big_row(3, 256) + _big_row(9, 257) + _big_row(7, 257), "GS_EUNSUPPORTED",
     "more than 256 intervals at peer 7"),
]


def test_refusals_leave_the_context_as_it_was(monkeypatch):
    _quiet(monkeypatch)
    ref = _whatif_ref()
    sim = _whatif_sim()
    sim.mesh_converge(20)
    before = sim.run(SCHED)
    np.testing.assert_array_equal(before["t_complete"], ref["t_complete"])
    tab = sim.offline(0, H_TOP)
    for name, iv, status, text in REFUSALS:
        with pytest.raises(gossipsim.GossipSimError, match="%s.*outages: .*%s$" % (status, text)):
            sim.set_outages(*_arrays(iv))
        np.testing.assert_array_equal(sim.offline(0, H_TOP), tab, err_msg=name)
    with pytest.raises(gossipsim.GossipSimError, match="GS_EINVAL"):
        sim.set_outages([1, 2], [1], [2, 3])
    sim.reset_stats()
    after = sim.run(SCHED)  # no converge in between: the mesh, the chain and the ring still stand
    _same_run(after, sim.stats(), ref)
    np.testing.assert_array_equal(after["t_complete"], before["t_complete"])
    np.testing.assert_array_equal(after["hops"], before["hops"])
    sim.set_outages(*_arrays(_big_row(3, 256)))  # 256 intervals of one peer are accepted
    np.testing.assert_array_equal(sim.offline(0, 600), outage_ref.table(N, _big_row(3, 256), 0, 600))
    sim.close()


def test_state_rules(tmp_path, monkeypatch):
    _quiet(monkeypatch)
    calm = _new(_params(0, 6))
    with pytest.raises(gossipsim.GossipSimError, match="GS_ESTATE"):
        calm.set_outages([1], [2], [3])
    calm.clear_outages()  # nothing imported: a no-op
    calm.close()
    sim = _new(_params(30000, 6))
    sim.set_mesh_events(True)
    sim.clear_outages()
    sim.mesh_converge(MAX_HB)
    sim.mesh_events()
    sim.save_state(tmp_path / "draw.state")
    sim.set_outages([], [], [])
    with pytest.raises(gossipsim.GossipSimError, match="GS_ESTATE"):  # a converge must follow
        sim.run(SCHED)
    with pytest.raises(gossipsim.GossipSimError, match="GS_ESTATE"):
        sim.mesh_events()
    with pytest.raises(gossipsim.GossipSimError, match="GS_ESTATE"):
        sim.mesh_series()
    with pytest.raises(gossipsim.GossipSimError, match="GS_EUNSUPPORTED"):
        sim.save_state(tmp_path / "imported.state")
    sim.mesh_converge(MAX_HB)
    sim.mesh_events()
    with pytest.raises(gossipsim.GossipSimError, match="GS_EUNSUPPORTED"):
        sim.save_state(tmp_path / "imported.state")
    with pytest.raises(gossipsim.GossipSimError, match="GS_EUNSUPPORTED"):  # unchanged: no imported mesh under churn
        sim.set_mesh(*sim.mesh())
    with pytest.raises(gossipsim.GossipSimError, match="GS_EUNSUPPORTED"):
        sim.set_link_deliveries(True)
    # back to the draw: test 3's run again
    sim.clear_outages()
    with pytest.raises(gossipsim.GossipSimError, match="GS_ESTATE"):
        sim.run(SCHED)
    ref = _draw_ref()
    _same_graph_and_mesh(sim, ref, sim.mesh_converge(MAX_HB))
    sim.reset_stats()
    res = sim.run(SCHED)
    _same_run(res, sim.stats(), ref)
    sim.save_state(tmp_path / "draw2.state")
    sim.close()


# ---- 7. partitioned ----
def test_partitioned(monkeypatch):
    _quiet(monkeypatch)
    ref = _whatif_ref()
    sims = [_whatif_sim(), _whatif_sim()]
    for s in sims:
        s.mesh_converge(20)
    comm = gossipsim.Comm(local_parts=2)
    res = comm.run_partitioned(sims, SCHED)
    np.testing.assert_array_equal(np.concatenate([x["t_complete"] for x in res], axis=1), ref["t_complete"])
    np.testing.assert_array_equal(np.concatenate([x["hops"] for x in res], axis=1), ref["hops"])
    for s in sims:
        st = s.stats()
        assert st["batches"] == M // BATCH and st["ms_batches"] == st["batches"], st
    one = _whatif_sim()
    one.mesh_converge(20)
    got = one.run(SCHED)
    np.testing.assert_array_equal(np.concatenate([x["t_complete"] for x in res], axis=1), got["t_complete"])
    # the schedule in one part only
    plain = _new(_params(30000, 6))
    plain.mesh_converge(20)
    sims[1].reset_stats()
    for pair in ([sims[1], plain], [plain, sims[1]]):
        with pytest.raises(gossipsim.GossipSimError, match="GS_EINVAL.*same outages"):
            comm.run_partitioned(pair, SCHED)
    assert sims[1].stats()["messages"] == 0 and plain.stats()["messages"] == 0  # before any batch
    # another schedule in the other part is refused as well
    other = _new(_params(30000, 6))
    other.set_outages(*_arrays(WHATIF[1:]))
    other.mesh_converge(20)
    with pytest.raises(gossipsim.GossipSimError, match="GS_EINVAL.*same outages"):
        comm.run_partitioned([sims[1], other], SCHED)
    for s in sims + [one, plain, other]:
        s.close()


# ---- 8. CLI ----
def test_cli_outages(tmp_path, monkeypatch):
    _quiet(monkeypatch)
    exe = os.path.join(os.path.dirname(gossipsim.LIB_PATH), "gossipsim-node")
    at = lambda h: PHASE + h * HB
    f = tmp_path / "outages.txt"
    with open(f, "w") as out:
        out.write("# the what-if of test 5 as times: down just before heartbeat h_from, up just before h_to\n")
        for u, a, b in WHATIF:
            out.write("%d %d\n" % (u, at(a) - 7) if b == FOREVER else "%d %d %d\n" % (u, at(a) - 7, at(b) - 3))
    p, d, t = gossipsim.read_outages(f)
    got = gossipsim.outage_epochs(_params(30000, 6), p, d, t)
    assert list(zip(*(x.tolist() for x in got))) == WHATIF
    env = dict(os.environ, PEERS=str(N), CONNECTTO="10", GS_SEED="59", GS_BATCH=str(BATCH), GS_CHURN_PPM="30000",
               GS_CHURN_DOWN="6", GS_CHURN_HORIZON="10", GOSSIPSUB_HEARTBEAT_MS="400", GS_HB_PHASE_NS=str(PHASE))
    args = [exe, "-st", "5", "-bl", "50", "-bh", "150", "-ll", "40", "-lh", "130", "-s", "15000", "-m", str(M),
            "--publisher", "6", "--rotation", "1", "--delay-ms", "400", "--max-heartbeats", "20"]
    subprocess.run(args + ["--outages", str(f), "--latencies", str(tmp_path / "lat")], env=env, check=True, timeout=60)
    sched = gossipsim.schedule_runsh(M, N, 6, 1, T0, HB, 15000)
    sim = _whatif_sim()
    sim.mesh_converge(20)
    res = sim.run(sched)
    np.testing.assert_array_equal(res["t_complete"], _whatif_ref()["t_complete"])
    sim.write_latency_log(str(tmp_path / "py_lat"), res)
    lines = sorted(open(tmp_path / "lat").read().splitlines())
    assert lines and lines == sorted(open(tmp_path / "py_lat").read().splitlines())
    sim.close()
    # an error on a run without churn, and a bad file names its line
    out = subprocess.run(args + ["--outages", str(f)], env=dict(env, GS_CHURN_PPM="0"), timeout=60,
                         capture_output=True, text=True)
    assert out.returncode == 2 and "--outages" in out.stderr and "churn" in out.stderr
    bad = tmp_path / "bad.txt"
    bad.write_text("1 5 9\n\n2 x\n")
    out = subprocess.run(args + ["--outages", str(bad)], env=env, timeout=60, capture_output=True, text=True)
    assert out.returncode == 1 and "line 3" in out.stderr
    over = tmp_path / "over.txt"
    over.write_text("1 %d %d\n4 %d\n1 %d %d\n" % (at(3), at(9), at(2), at(8) - 1, at(12)))
    out = subprocess.run(args + ["--outages", str(over)], env=env, timeout=60, capture_output=True, text=True)
    assert out.returncode == 1 and "share an epoch at interval 0" in out.stderr
