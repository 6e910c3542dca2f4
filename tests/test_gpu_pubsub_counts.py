"""Per-peer pubsub event counts (gs_set_pubsub_counts) against the oracle.

The reference is tests/pubsub_ref.py: the oracle's per-peer traffic of one message at a time,
split into fragment copies, IHAVE and IWANT RPCs (large messages make the split unique; the
helper asserts it for every peer and message). All eight columns are compared exactly."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gossipsim
import oracle
import pubsub_ref as R

pytestmark = pytest.mark.gpu

T0 = gossipsim.T0_NS
LINKS = (50, 150, 40, 130)
SIZE = 240000
PHASE = T0 % 1_000_000_000  # a heartbeat at the publish instant: IHAVEs race the eager wave
CHURN = dict(churn_ppm=20000, heartbeat_ns=200_000_000, hb_phase_ns=T0 - 2_000_000_000, churn_horizon=10)
SIX = [R.MSG_TX, R.MSG_RX, R.IHAVE_TX, R.IHAVE_RX, R.IWANT_TX, R.IWANT_RX]

# name -> (node, oracle params, messages, batch)
CASES = {
    "rust": (0, dict(peers=300, hb_phase_ns=PHASE), 4, 8),
    "f3": (0, dict(peers=300, fragments=3, hb_phase_ns=PHASE), 4, 8),
    "go_f1": ("go", dict(peers=300, hb_phase_ns=PHASE), 4, 8),
    "go_f2": ("go", dict(peers=300, fragments=2, hb_phase_ns=PHASE), 4, 8),
    "nim": ("nim", dict(peers=300, hb_phase_ns=PHASE), 3, 8),
    "no_flood": (0, dict(peers=300, flood_publish=0, hb_phase_ns=PHASE), 3, 8),
    "no_gossip": (0, dict(peers=300, lazy_gossip=0), 3, 8),
    "quiet": (0, dict(peers=300), 3, 8),  # heartbeats off the publish instant: IHAVEs only
    "quic": (0, dict(peers=300, muxer=1, signed_msgs=0, hb_phase_ns=PHASE), 3, 8),
    "churn_f1": (0, dict(peers=600, **CHURN), 6, 8),
    "churn_f2": (0, dict(peers=600, fragments=2, **CHURN), 6, 8),
    "n257_m1": (0, dict(peers=257, hb_phase_ns=PHASE), 1, 8),
    "n300_m12": (0, dict(peers=300, hb_phase_ns=PHASE), 12, 8),
    "n900_m5": (0, dict(peers=900, hb_phase_ns=PHASE), 5, 8),
}
_REF = {}


def _sched(M, N, size=SIZE):
    t = T0 + np.arange(M, dtype=np.uint64) * np.uint64(1_000_000_000)
    return t, (37 * np.arange(M) + 4) % N, np.full(M, size)


def _params(name):
    node, kw, M, batch = CASES[name]
    return oracle.params_for(node, seed=71, **kw), M, batch


def _overrides():
    """F = 2 with per-message chunk counts and a size change mid-schedule (cuts a batch)."""
    p = oracle.params(peers=300, seed=71, fragments=2, hb_phase_ns=PHASE)
    t, pub, size = _sched(5, 300)
    size = size.copy()
    size[3:] = 300000
    return p, (t, pub, size, np.array([0, 3, 2, 1, 0], np.uint32))


def ref_of(name):
    """The case's reference, computed once and shared (never modified)."""
    if name not in _REF:
        if name == "overrides":
            p, sched = _overrides()
        else:
            p, M, _ = _params(name)
            sched = _sched(M, p.peers)
        r = R.reference(p, 5, LINKS, sched)
        r["counts"].setflags(write=False)
        _REF[name] = (p, sched, r)
    return _REF[name]


def gpu_sim(p, batch=8):
    kw = {n: getattr(p, n) for n, _ in oracle.OrParams._fields_}
    sim = gossipsim.Simulator(batch=batch, **kw)
    sim.set_topogen_links(5, *LINKS)
    sim.connect_gossipsub_peers()
    sim.mesh_converge()
    return sim


def _part(sched, a, b):
    return tuple(x[a:b] for x in sched)


def _run_case(name, batch=8):
    p, sched, r = ref_of(name)
    sim = gpu_sim(p, batch)
    sim.set_pubsub_counts()
    res = sim.run(sched)
    np.testing.assert_array_equal(res["t_complete"], r["whole"]["t_complete"])
    return sim, sim.pubsub_counts(), r


def _same(got, r, what=""):
    for col, cname in enumerate(gossipsim.PUBSUB_COLS):
        np.testing.assert_array_equal(got[:, col], r["counts"][:, col], err_msg="%s %s" % (what, cname))


def test_rust_carries_across_calls_and_resets():
    """2 + 2 messages: the counters carry across calls; both resets zero them."""
    p, sched, r = ref_of("rust")
    assert r["exact"] and int(r["counts"][:, R.IWANT_TX].sum()) > 0
    sim = gpu_sim(p)
    sim.set_pubsub_counts()
    assert not sim.pubsub_counts().any()
    sim.run(_part(sched, 0, 2))
    sim.run(_part(sched, 2, 4))
    _same(sim.pubsub_counts(), r)
    sim.reset_pubsub_counts()
    assert not sim.pubsub_counts().any()
    sim.run(_part(sched, 0, 1), collect=False)
    assert sim.pubsub_counts().any()
    sim.reset_stats()
    assert not sim.pubsub_counts().any()
    sim.run(sched, collect=False)  # after a reset the same counts again
    _same(sim.pubsub_counts(), r)
    sim.set_pubsub_counts()  # enabling zeroes
    assert not sim.pubsub_counts().any()


def test_fragment_groups_with_a_padding_lane():
    """F = 3 in groups of 4 lanes: the padding lane counts nothing, FIRST == 3 x received."""
    _, got, r = _run_case("f3")
    assert r["exact"]
    _same(got, r)
    np.testing.assert_array_equal(got[:, R.FIRST], 3 * r["whole"]["traffic"][:, R.TR_RECEIVED])


def test_per_message_chunks_and_a_size_change():
    sim, got, r = _run_case("overrides")
    assert r["exact"] and sim.stats()["batches"] >= 3
    _same(got, r)


@pytest.mark.parametrize("name", ["go_f1", "go_f2", "nim", "no_flood", "no_gossip", "quiet", "quic"])
def test_presets_and_knobs(name):
    sim, got, r = _run_case(name)
    assert r["exact"]
    _same(got, r, name)
    if name == "no_gossip":
        assert not got[:, [R.IHAVE_TX, R.IHAVE_RX, R.IWANT_TX, R.IWANT_RX]].any()
    else:
        assert got[:, R.IHAVE_TX].any()
    if name == "quiet":
        assert not got[:, R.IWANT_TX].any()
    if name.startswith("go"):  # IDONTWANT really skips sends: fewer than without it
        p0 = oracle.params_for("go", seed=71, idontwant=0, **CASES[name][1])
        ref0 = oracle.simulate(p0, 5, LINKS, sched=_sched(CASES[name][2], 300))
        assert int(got[:, R.MSG_TX].sum()) == r["whole"]["stats"]["relaxations"] < ref0["stats"]["relaxations"]


def test_churn_single_fragment():
    """Losses: a lost send counts at the sender only."""
    _, got, r = _run_case("churn_f1")
    assert r["exact"]
    _same(got, r)
    assert int(got[:, R.MSG_TX].sum()) > int(got[:, R.MSG_RX].sum())
    assert int(got[:, R.IHAVE_TX].sum()) >= int(got[:, R.IHAVE_RX].sum())


def test_churn_two_fragments():
    """Partial receipts exist: the six send / receive columns per peer, first receipts by their
    total and the per-peer lower bound F x received."""
    _, got, r = _run_case("churn_f2")
    assert not r["exact"]
    for col in SIX:
        np.testing.assert_array_equal(got[:, col], r["counts"][:, col], err_msg=gossipsim.PUBSUB_COLS[col])
    whole = r["whole"]
    assert int(got[:, R.FIRST].sum()) == whole["stats"]["frag_deliveries"]
    assert (2 * whole["traffic"][:, R.TR_RECEIVED] <= got[:, R.FIRST]).all()
    np.testing.assert_array_equal(got[:, R.DUP], got[:, R.MSG_RX] - got[:, R.FIRST])
    assert int(got[:, R.FIRST].sum()) > 2 * int(whole["traffic"][:, R.TR_RECEIVED].sum())


@pytest.mark.parametrize("name", ["n257_m1", "n300_m12", "n900_m5"])
def test_edges(name):
    """One message at 257 peers; two batches, the second short; more than one block of rows."""
    sim, got, r = _run_case(name)
    _same(got, r, name)
    if name == "n300_m12":
        assert sim.stats()["batches"] == 2


SINKS = ["array", "on_lat", "run_log", "null"]


def _run_sink(sim, sched, sink):
    if sink == "array":
        sim.run(sched)
    elif sink == "on_lat":
        sim.run(sched, on_lat=lambda first, lat: None)
    elif sink == "run_log":
        sim.run_log(sched, on_text=lambda first, n, text, lines: None)
    else:
        sim.run(sched, collect=False)


@pytest.mark.parametrize("sink", SINKS)
def test_one_result_whatever_the_sink(sink):
    """Every output path gives the same counts, and the switch changes nothing else: gs_stats of
    the same run with the switch off is the same dict."""
    p, sched, r = ref_of("rust")
    on = gpu_sim(p)
    on.set_pubsub_counts()
    _run_sink(on, sched, sink)
    _same(on.pubsub_counts(), r, sink)
    off = gpu_sim(p)
    _run_sink(off, sched, sink)
    assert on.stats() == off.stats()


def test_both_switches():
    """gs_set_traffic beside it: the traffic is still the oracle's, the counts still right, and
    on the frozen mesh the totals are the run's own counters."""
    p, sched, r = ref_of("rust")
    sim = gpu_sim(p)
    sim.set_traffic(True)
    sim.set_pubsub_counts()
    sim.run(sched)
    np.testing.assert_array_equal(sim.traffic(), r["whole"]["traffic"])
    got = sim.pubsub_counts()
    _same(got, r)
    st = sim.stats()
    assert int(got[:, R.MSG_TX].sum()) == st["relaxations"] == r["whole"]["stats"]["relaxations"]
    assert int(got[:, R.FIRST].sum()) == st["frag_deliveries"] == r["whole"]["stats"]["frag_deliveries"]


def test_errors_and_state(tmp_path):
    p, sched, _ = ref_of("rust")
    sim = gpu_sim(p)
    with pytest.raises(gossipsim.GossipSimError, match="GS_ESTATE"):
        sim.pubsub_counts()
    sim.set_pubsub_counts()
    assert gossipsim.lib().gs_get_pubsub_counts(sim.ctx, None) == gossipsim.GS_EINVAL
    sim.run(_part(sched, 0, 1), collect=False)
    sim.save_state(tmp_path / "state")
    loaded = gossipsim.Simulator.load_state(tmp_path / "state")
    with pytest.raises(gossipsim.GossipSimError, match="GS_ESTATE"):
        loaded.pubsub_counts()  # the switch is off in a loaded context
    loaded.set_pubsub_counts()
    assert not loaded.pubsub_counts().any()
    # partitioned mode refuses the switch, naming it (no heartbeat at the publish instant:
    # nothing else about the batch is unsupported there)
    sims = []
    for i in range(2):
        s = gpu_sim(oracle.params(peers=300, seed=71), batch=4)
        s.set_partition(2, i)
        s.set_pubsub_counts()
        sims.append(s)
    with pytest.raises(gossipsim.GossipSimError, match="GS_EUNSUPPORTED.*gs_set_pubsub_counts"):
        sims[0].part_begin(sched)
    comm = gossipsim.Comm(local_parts=2)
    with pytest.raises(gossipsim.GossipSimError, match="GS_EUNSUPPORTED.*gs_set_pubsub_counts"):
        comm.run_partitioned(sims, sched)
    comm.close()


def test_cli_pubsub_metrics(tmp_path):
    """gossipsim-node --pubsub-metrics: the file parses, and every peer's series are
    pubsub_counts() of the same run."""
    exe = os.path.join(os.path.dirname(gossipsim.LIB_PATH), "gossipsim-node")
    N, M = 300, 4
    env = dict(os.environ, PEERS=str(N), CONNECTTO="10", FRAGMENTS="2", GS_SEED="5", GS_BATCH="4")
    args = [exe, "-st", "5", "-bl", "50", "-bh", "150", "-ll", "40", "-lh", "130", "-m", str(M), "-s", str(SIZE)]
    subprocess.run(args + ["--pubsub-metrics", str(tmp_path / "a")], env=env, check=True, timeout=60)
    sim = gpu_sim(oracle.params(peers=N, seed=5, fragments=2), batch=4)
    sim.set_pubsub_counts()
    sim.run(gossipsim.schedule_runsh(M, N, 6, 1, gossipsim.T0_NS, gossipsim.DELAY_NS, SIZE), collect=False)
    got = sim.pubsub_counts()
    assert got[:, R.MSG_TX].any() and got[:, R.DUP].any()
    text = open(str(tmp_path / "a")).read()
    series = {}
    for line in text.splitlines():
        if line.startswith("#"):
            assert re.match(r"# (HELP|TYPE) [a-z0-9_]+ \S", line), line
            continue
        m = re.match(r'^([a-z0-9_]+)\{(?:[a-z_]+="[^"]*",)*peer_id="pod-(\d+)"\} (\d+)$', line)
        assert m, line
        series.setdefault(m.group(1), {})[int(m.group(2))] = int(m.group(3))
    cols = dict(libp2p_pubsub_broadcast_messages_total=R.MSG_TX, libp2p_pubsub_received_messages_total=R.MSG_RX,
                libp2p_pubsub_broadcast_ihave_total=R.IHAVE_TX, libp2p_pubsub_received_ihave_total=R.IHAVE_RX,
                libp2p_pubsub_broadcast_iwant_total=R.IWANT_TX, libp2p_pubsub_received_iwant_total=R.IWANT_RX,
                libp2p_gossipsub_received_total=R.FIRST, libp2p_gossipsub_duplicate_total=R.DUP,
                dst_testnode_received_chunks_total=R.FIRST)
    assert set(series) == set(cols)
    for name, col in cols.items():
        assert [series[name][u] for u in range(N)] == got[:, col].tolist(), name
    sim.write_pubsub_metrics(str(tmp_path / "py"))
    assert open(str(tmp_path / "py")).read() == text
