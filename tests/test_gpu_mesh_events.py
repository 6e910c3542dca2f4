"""Mesh event counts and per-epoch mesh health on the device (gs_set_mesh_events, DESIGN.md
§2.15) against tests/mesh_ref.py, the pure-Python restatement of the heartbeat epoch that is
pinned to the oracle's mesh of every epoch. Every comparison is exact equality: all seven
columns for every peer and all twelve series columns for every row."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gossipsim
import oracle
import mesh_ref as R

pytestmark = pytest.mark.gpu

CASES, L5, ref_of = R.CASES, R.L5, R.ref_of

T0 = gossipsim.T0_NS
# a short churn run: heartbeats every 200 ms, epoch 10 at T0
RUN = dict(peers=300, seed=1, churn_ppm=20000, churn_down=5, heartbeat_ns=200_000_000, hb_phase_ns=T0 - 2_000_000_000,
           churn_horizon=10)
_EXTRA = {}


def extra_ref(key, kw, max_hb, links=L5):
    if key not in _EXTRA:
        _EXTRA[key] = R.reference(oracle.params(**kw), links[0], links[1], max_hb)
    return _EXTRA[key]


def gpu_sim(p, links=L5, events=True, batch=8):
    kw = {n: getattr(p, n) for n, _ in oracle.OrParams._fields_}
    sim = gossipsim.Simulator(batch=batch, **kw)
    sim.set_topogen_links(links[0], *links[1])
    sim.connect_gossipsub_peers()
    if events:
        sim.set_mesh_events()
    return sim


def _same(sim, r, what=""):
    ev, se = sim.mesh_events(), sim.mesh_series()
    assert ev.dtype == np.uint64 and se.dtype == np.uint64
    for col, cname in enumerate(gossipsim.MESH_EVENT_COLS):
        np.testing.assert_array_equal(ev[:, col], r["events"][:, col], err_msg="%s %s" % (what, cname))
    assert se.shape == r["series"].shape, what
    for col, cname in enumerate(gossipsim.MESH_SERIES_COLS):
        np.testing.assert_array_equal(se[:, col], r["series"][:, col], err_msg="%s series %s" % (what, cname))
    return ev, se


def _sched(M, N, t0=T0):
    t = t0 + np.arange(M, dtype=np.uint64) * np.uint64(400_000_000)
    return t, (37 * np.arange(M) + 4) % N, np.full(M, 15000)


@pytest.mark.parametrize("name", sorted(CASES))
def test_cases_against_the_reference(name):
    kw, links, max_hb = CASES[name][:3]
    r = ref_of(name)
    sim = gpu_sim(oracle.params(**kw), links)
    assert sim.graph_info()[2] == r["max_degree"]
    assert sim.mesh_converge(max_hb) == r["epochs"]
    ev, se = _same(sim, r, name)
    R.check_identities(ev, se)
    mesh, cnt = sim.mesh()
    np.testing.assert_array_equal(mesh, r["mesh"])
    np.testing.assert_array_equal(cnt, r["count"])
    np.testing.assert_array_equal(se[-1, R.LINKS], cnt.astype(np.uint64).sum())


def _run_both(kw, max_hb, sched):
    out = []
    for events in (False, True):
        sim = gpu_sim(oracle.params(**kw), events=events)
        ep = sim.mesh_converge(max_hb)
        mesh, cnt = sim.mesh()
        res = sim.run(sched)
        out.append((ep, mesh, cnt, res["t_complete"], res["hops"], sim.stats()))
    return out


@pytest.mark.parametrize("which", ["frozen", "churn"])
def test_the_switch_changes_nothing_else(which):
    """Mesh, out_epochs, gs_run's results and gs_stats with the switch on are those with it off."""
    if which == "frozen":
        kw, _, max_hb = CASES["A"][:3]
        off, on = _run_both(kw, max_hb, _sched(3, 300))
    else:
        off, on = _run_both(RUN, 20, _sched(4, 300, T0 + 3_000_000_000))
    assert off[0] == on[0]
    for a, b in zip(off[1:5], on[1:5]):
        np.testing.assert_array_equal(a, b)
    assert off[5] == on[5]
    assert off[5]["deliveries"] > 0


def test_a_second_converge_replaces_the_counts():
    kw, links, max_hb = CASES["D"][:3]
    sim = gpu_sim(oracle.params(**kw), links)
    sim.mesh_converge(max_hb)
    assert sim.mesh_converge(12) == 12
    _same(sim, extra_ref("D12", kw, 12), "D at 12")
    assert sim.mesh_series().shape[0] == 13
    sim.mesh_converge(max_hb)
    _same(sim, ref_of("D"), "D again")
    # frozen: a converge cut short at heartbeat 3, then the whole one
    kw, links, max_hb = CASES["A"][:3]
    sim = gpu_sim(oracle.params(**kw), links)
    assert sim.mesh_converge(3) == 3
    _same(sim, extra_ref("A3", kw, 3), "A at 3")
    sim.mesh_converge(max_hb)
    _same(sim, ref_of("A"), "A whole")


def test_gs_run_leaves_the_counts():
    """The epochs gs_run's chain steps after the converge, or replays from epoch 0, are not
    counted; a frozen run neither."""
    r = extra_ref("RUN20", RUN, 20)
    sim = gpu_sim(oracle.params(**RUN))
    assert sim.mesh_converge(20) == 20
    _same(sim, r, "before the runs")
    res = sim.run(_sched(4, 300, T0 + 3_000_000_000))  # epochs 25..: the chain continues from 20
    assert (res["hops"] > 0).any()
    _same(sim, r, "after a continuing run")
    sim.run(_sched(3, 300), collect=False)  # epoch 10 has left the ring: replay from epoch 0
    _same(sim, r, "after a replaying run")
    kw, links, max_hb = CASES["A"][:3]
    sim = gpu_sim(oracle.params(**kw), links)
    sim.mesh_converge(max_hb)
    sim.run(_sched(2, 300), collect=False)
    sim.reset_stats()
    _same(sim, ref_of("A"), "frozen")


def test_state_errors(tmp_path):
    kw, links, max_hb = CASES["G"][:3]
    L = gossipsim.lib()
    sim = gpu_sim(oracle.params(**kw), links, events=False)
    sim.mesh_converge(max_hb)
    getters = (sim.mesh_events, sim.mesh_series, lambda: sim.write_mesh_series(str(tmp_path / "s")))
    for get in getters:  # the switch is off
        with pytest.raises(gossipsim.GossipSimError, match="GS_ESTATE"):
            get()
    sim.set_mesh_events()
    for get in getters:  # on, but no converge since
        with pytest.raises(gossipsim.GossipSimError, match="GS_ESTATE.*gs_mesh_converge"):
            get()
    sim.mesh_converge(max_hb)
    _same(sim, ref_of("G"), "G")
    rows = sim.mesh_series().shape[0]
    se = np.zeros((rows + 1, R.SERIES_COLS), np.uint64)
    pu64 = ctypes.POINTER(ctypes.c_uint64)
    assert L.gs_get_mesh_series(sim.ctx, se.ctypes.data_as(pu64), rows + 1) == gossipsim.GS_EINVAL
    assert L.gs_get_mesh_series(sim.ctx, se.ctypes.data_as(pu64), rows - 1) == gossipsim.GS_EINVAL
    assert L.gs_get_mesh_series(sim.ctx, None, rows) == gossipsim.GS_EINVAL
    assert L.gs_get_mesh_events(sim.ctx, None) == gossipsim.GS_EINVAL
    assert L.gs_mesh_series_rows(sim.ctx, None) == gossipsim.GS_EINVAL
    sim.save_state(tmp_path / "state")
    loaded = gossipsim.Simulator.load_state(tmp_path / "state")
    with pytest.raises(gossipsim.GossipSimError, match="GS_ESTATE"):
        loaded.mesh_events()  # the switch is off in a loaded context
    sim.set_mesh_events(False)
    for get in getters:
        with pytest.raises(gossipsim.GossipSimError, match="GS_ESTATE"):
            get()
    sim.set_mesh_events()  # enabling again: nothing to read until the next converge
    with pytest.raises(gossipsim.GossipSimError, match="GS_ESTATE"):
        sim.mesh_events()
    sim.mesh_converge(max_hb)
    _same(sim, ref_of("G"), "G again")


def test_a_part_counts_all_peers():
    """A context holding one of two parts: the mesh is replicated, so are the counts."""
    kw, links, max_hb = CASES["A"][:3]
    for part in (0, 1):
        sim = gpu_sim(oracle.params(**kw), links)
        sim.set_partition(2, part)
        sim.mesh_converge(max_hb)
        _same(sim, ref_of("A"), "part %d" % part)


def test_cli_flags(tmp_path):
    """gossipsim-node --mesh-metrics / --mesh-series write what the Python writers write, and
    the values are the reference's."""
    exe = os.path.join(os.path.dirname(gossipsim.LIB_PATH), "gossipsim-node")
    kw, links, max_hb = CASES["A"][:3]
    N = kw["peers"]
    env = dict(os.environ, PEERS=str(N), CONNECTTO="10", GS_SEED=str(kw["seed"]), GS_BATCH="4")
    args = [exe, "-st", "5", "-bl", "50", "-bh", "150", "-ll", "40", "-lh", "130", "-m", "1", "-s", "1000",
            "--max-heartbeats", str(max_hb)]
    subprocess.run(args + ["--mesh-metrics", str(tmp_path / "m"), "--mesh-series", str(tmp_path / "s")], env=env,
                   check=True, timeout=60)
    sim = gpu_sim(oracle.params(**kw), links)
    sim.mesh_converge(max_hb)
    sim.write_mesh_metrics(str(tmp_path / "pm"))
    sim.write_mesh_series(str(tmp_path / "ps"))
    text = open(str(tmp_path / "m")).read()
    assert text == open(str(tmp_path / "pm")).read()
    assert open(str(tmp_path / "s")).read() == open(str(tmp_path / "ps")).read()
    r = ref_of("A")
    series = {}
    for line in text.splitlines():
        if line.startswith("#"):
            assert re.match(r"# (HELP|TYPE) [a-z0-9_]+ \S", line), line
            continue
        m = re.match(r'^([a-z0-9_]+)\{(?:[a-z_]+="[^"]*",)*peer_id="pod-(\d+)"\} (\d+)$', line)
        assert m, line
        series.setdefault(m.group(1), {})[int(m.group(2))] = int(m.group(3))
    cols = dict(libp2p_pubsub_broadcast_graft_total=R.ME_GRAFT_TX, libp2p_pubsub_received_graft_total=R.ME_GRAFT_RX,
                libp2p_pubsub_broadcast_prune_total=R.ME_PRUNE_TX, libp2p_pubsub_received_prune_total=R.ME_PRUNE_RX)
    for name, col in cols.items():
        assert [series[name][u] for u in range(N)] == r["events"][:, col].tolist(), name
    assert [series["libp2p_gossipsub_peers_per_topic_mesh"][u] for u in range(N)] == r["count"].tolist()
    deg = np.diff(sim.csr()[0].astype(np.int64)).tolist()
    assert [series["libp2p_pubsub_received_subscriptions_total"][u] for u in range(N)] == deg
    assert len(series) == 10
    lines = open(str(tmp_path / "s")).read().splitlines()
    assert len(lines) == r["epochs"] + 2
    assert [int(x) for x in lines[-1].split(",")] == [r["epochs"]] + r["series"][-1].tolist()
