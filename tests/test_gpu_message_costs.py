"""Per-message cost table (gs_set_message_costs) against the oracle.

The reference is tests/msgcost_ref.py: the oracle run one message at a time with per-peer traffic,
split into fragment copies, IHAVE and IWANT RPCs and summed over the peers (the helper asserts every
split). All eight columns are compared exactly, and t_complete is asserted equal to the oracle's
before any count is looked at."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gossipsim
import msgcost_ref as R
import oracle
import pubsub_ref as PS
from test_gpu_pubsub_counts import _part, gpu_sim

pytestmark = pytest.mark.gpu


def _same(got, r, what=""):
    assert got.shape == r["costs"].shape, what
    for col, cname in enumerate(gossipsim.MESSAGE_COST_COLS):
        np.testing.assert_array_equal(got[:, col], r["costs"][:, col], err_msg="%s %s" % (what, cname))


def _run_case(name, batch=8):
    p, sched, r = R.case(name)
    sim = gpu_sim(p, batch)
    sim.set_message_costs()
    res = sim.run(sched)
    np.testing.assert_array_equal(res["t_complete"], r["whole"]["t_complete"])
    return sim, sim.message_costs(), r


def test_rust_with_a_heartbeat_at_the_publish_instant():
    _, _, r = R.case("rust")
    assert (r["costs"][:, R.IWANT] > 0).any()
    sim, got, r = _run_case("rust")
    _same(got, r)
    np.testing.assert_array_equal(got[:, R.DUP], got[:, R.DATA_RX] - got[:, R.FIRST])
    off = gpu_sim(R.case("rust")[0])  # the switch changes nothing else: gs_stats is the same dict
    off.run(R.case("rust")[1])
    assert sim.stats() == off.stats()


def test_fragment_groups_with_a_padding_lane():
    """F = 3 in groups of 4 lanes: the padding lane counts nothing, FIRST == 3 x DELIVERED."""
    _, got, r = _run_case("f3")
    _same(got, r)
    np.testing.assert_array_equal(got[:, R.FIRST], 3 * got[:, R.DELIVERED])


@pytest.mark.parametrize("name", ["go_f2", "no_flood", "quic"])
def test_presets_and_knobs(name):
    """go_f2: IDONTWANT skips sends; no_flood: the publisher sends to its mesh; quic."""
    _, got, r = _run_case(name)
    _same(got, r, name)
    if name == "go_f2":  # IDONTWANT really skips sends: fewer than without it
        from test_gpu_pubsub_counts import CASES, _sched
        p0 = oracle.params_for("go", seed=71, idontwant=0, **CASES[name][1])
        ref0 = oracle.simulate(p0, 5, R.LINKS, sched=_sched(CASES[name][2], 300))
        assert int(got[:, R.DATA_TX].sum()) == r["whole"]["stats"]["relaxations"] < ref0["stats"]["relaxations"]


@pytest.mark.parametrize("name", ["churn_f1", "churn_f2"])
def test_churn(name):
    """Losses: a lost copy counts as sent only. With two fragments partial receipts exist and FIRST is
    still exact per message (the one-message oracle run's own frag_deliveries)."""
    _, _, r = R.case(name)
    assert (r["costs"][:, R.DATA_TX] > r["costs"][:, R.DATA_RX]).any()
    _, got, r = _run_case(name)
    _same(got, r, name)


def test_per_message_chunks_and_a_size_change():
    """Rows from three batches land at their schedule indices."""
    sim, got, r = _run_case("overrides")
    assert sim.stats()["batches"] >= 3
    _same(got, r)


@pytest.mark.parametrize("batch", [8, 1])
def test_batch_size(batch):
    """12 messages in two batches (the second short) and in twelve."""
    sim, got, r = _run_case("n300_m12", batch)
    assert sim.stats()["batches"] == (2 if batch == 8 else 12)
    _same(got, r, "batch %d" % batch)


@pytest.mark.parametrize("name", ["n257_m1", "n257_m5"])
def test_lane_shapes(name):
    """peers = 257. M = 1: L = 1, the 64 rows of a wave hit one LDS row, and the last wave holds one
    valid lane. M = 5: a wave straddles rows and messages."""
    _, got, r = _run_case(name)
    _same(got, r, name)


def test_regrouped_classes_come_back_in_schedule_order():
    """A 1500 ms message delay with gossip: two offset classes, the run regroups the messages by
    class (class_plan) and the rows still come back in schedule order."""
    p, sched, r = R.case("delay")
    offs = {(int(t) - p.hb_phase_ns) % p.heartbeat_ns for t in sched[0]}
    assert len(offs) == 2
    c = r["costs"]
    assert len({tuple(int(x) for x in row) for row in c}) > 2  # the rows tell the messages apart
    sim, got, r = _run_case("delay")
    assert sim.stats()["batches"] == 2
    _same(got, r)


def test_log_path():
    """The same table through gs_run_log."""
    p, sched, r = R.case("rust")
    sim = gpu_sim(p)
    sim.set_message_costs()
    sim.run_log(sched, on_text=lambda first, n, text, lines: None)
    _same(sim.message_costs(), r, "run_log")


def test_direct_form_equals_the_lds_form(monkeypatch):
    """GS_MSGCOST_LDS_ROWS=2 at batch 8: more rows than the table may hold, so the lanes add to the
    global table directly (the library reads the knob at every launch)."""
    lds = _run_case("n300_m12")[1]
    monkeypatch.setenv("GS_MSGCOST_LDS_ROWS", "2")
    _, direct, r = _run_case("n300_m12")
    np.testing.assert_array_equal(direct, lds)
    _same(direct, r, "direct")
    monkeypatch.setenv("GS_MSGCOST_LDS_ROWS", "0")  # the publisher's block too
    _same(_run_case("n300_m12")[1], r, "direct, publishers too")


def test_life_cycle():
    p, sched, r = R.case("rust")
    sim = gpu_sim(p)
    with pytest.raises(gossipsim.GossipSimError, match="GS_ESTATE"):
        sim.message_costs()
    sim.set_message_costs()
    assert sim.message_costs().shape == (0, 8)  # rows is 0 before a run
    L = gossipsim.lib()
    one = np.zeros(8, np.uint64)
    ptr = one.ctypes.data_as(gossipsim.P(gossipsim.u64))
    assert L.gs_get_message_costs(sim.ctx, ptr, 1) == gossipsim.GS_EINVAL  # a wrong rows
    sim.run(_part(sched, 0, 2), collect=False)
    np.testing.assert_array_equal(sim.message_costs(), r["costs"][0:2])
    sim.run(_part(sched, 2, 4), collect=False)  # the second call's rows alone: not cumulative
    got = sim.message_costs()
    assert got.shape == (2, 8)
    np.testing.assert_array_equal(got, r["costs"][2:4])
    assert L.gs_get_message_costs(sim.ctx, ptr, 4) == gossipsim.GS_EINVAL
    assert L.gs_get_message_costs(sim.ctx, None, 2) == gossipsim.GS_EINVAL
    sim.reset_stats()  # leaves the table alone
    np.testing.assert_array_equal(sim.message_costs(), r["costs"][2:4])
    sim.set_message_costs()  # enabling empties it
    assert sim.message_costs().shape == (0, 8)
    sim.run(sched, collect=False)
    _same(sim.message_costs(), r)
    sim.set_message_costs(False)
    with pytest.raises(gossipsim.GossipSimError, match="GS_ESTATE"):
        sim.message_costs()
    rows = gossipsim.u64(0)
    assert gossipsim.STATUS[L.gs_message_costs_rows(sim.ctx, ctypes.byref(rows))] == "GS_ESTATE"


def test_partitioned_mode_refuses_the_switch():
    sched = R.case("rust")[1]
    sims = []
    for i in range(2):
        s = gpu_sim(oracle.params(peers=300, seed=71), batch=4)
        s.set_partition(2, i)
        s.set_message_costs()
        sims.append(s)
    with pytest.raises(gossipsim.GossipSimError, match="GS_EUNSUPPORTED.*gs_set_message_costs"):
        sims[0].part_begin(sched)
    comm = gossipsim.Comm(local_parts=2)
    with pytest.raises(gossipsim.GossipSimError, match="GS_EUNSUPPORTED.*gs_set_message_costs"):
        comm.run_partitioned(sims, sched)
    for s in sims:  # the contexts work again once it is off
        s.set_message_costs(False)
    ref = oracle.simulate(oracle.params(peers=300, seed=71), 5, R.LINKS, sched=sched)
    out = comm.run_partitioned(sims, sched)
    comm.close()
    tc = np.concatenate([o["t_complete"] for o in out], axis=1)
    np.testing.assert_array_equal(tc, ref["t_complete"])


@pytest.mark.parametrize("name", ["n900_m5", "churn_f2"])
def test_sums_equal_the_pubsub_counts_and_the_stats(name):
    """With the pubsub switch on in the same run: every column summed over the messages is the
    matching pubsub column summed over the peers. Frozen mesh: the sums are the run's own stats too
    (each identity asserted on the oracle's numbers first)."""
    p, sched, r = R.case(name)
    sim = gpu_sim(p)
    sim.set_message_costs()
    sim.set_pubsub_counts()
    res = sim.run(sched)
    np.testing.assert_array_equal(res["t_complete"], r["whole"]["t_complete"])
    mc = sim.message_costs().astype(np.int64).sum(axis=0)
    ps = sim.pubsub_counts().astype(np.int64).sum(axis=0)
    pairs = [(R.DATA_TX, PS.MSG_TX), (R.DATA_RX, PS.MSG_RX), (R.FIRST, PS.FIRST), (R.DUP, PS.DUP),
             (R.IHAVE_TX, PS.IHAVE_TX), (R.IHAVE_RX, PS.IHAVE_RX), (R.IWANT, PS.IWANT_TX), (R.IWANT, PS.IWANT_RX)]
    for a, b in pairs:
        assert mc[a] == ps[b], (gossipsim.MESSAGE_COST_COLS[a], gossipsim.PUBSUB_COLS[b])
    _same(sim.message_costs(), r, name)
    if name == "n900_m5":
        oc, ost, st = r["costs"].astype(np.int64).sum(axis=0), r["whole"]["stats"], sim.stats()
        for col, key in ((R.FIRST, "frag_deliveries"), (R.DELIVERED, "deliveries"), (R.IWANT, "gossip_iwant"),
                         (R.DATA_TX, "relaxations")):
            assert oc[col] == ost[key], "the oracle itself: %s" % key
            assert mc[col] == st[key], key


def test_more_than_one_grid_stride_round():
    """10 000 peers x 64 messages = 640 000 lanes, more than num_cus * 8 * 256: the kernels' loops
    take more than one round. No oracle here: this compares two device paths of different launch
    shape, one batch of 64 against 64 single-message calls (row m of the first is row 0 of call m)."""
    N, M = 10000, 64
    p = oracle.params(peers=N, seed=71, hb_phase_ns=gossipsim.T0_NS % 1_000_000_000)
    t = gossipsim.T0_NS + np.arange(M, dtype=np.uint64) * np.uint64(1_000_000_000)
    sched = (t, (37 * np.arange(M) + 4) % N, np.full(M, 240000))
    sim = gpu_sim(p, batch=64)
    sim.set_message_costs()
    sim.run(sched, collect=False)
    assert sim.stats()["batches"] == 1
    whole = sim.message_costs()
    assert whole.shape == (M, 8) and (whole[:, R.DELIVERED] == N - 1).all() and whole[:, R.IHAVE_TX].all()
    for m in range(M):
        sim.run(_part(sched, m, m + 1), collect=False)
        one = sim.message_costs()
        assert one.shape == (1, 8)
        np.testing.assert_array_equal(one[0], whole[m], err_msg="message %d" % m)


def test_cli_message_costs(tmp_path):
    """gossipsim-node --message-costs: the file is write_message_costs() of the same run, through
    the streamed log and through the device-formatted one."""
    import subprocess
    exe = os.path.join(os.path.dirname(gossipsim.LIB_PATH), "gossipsim-node")
    N, M, size = 300, 4, 240000
    env = dict(os.environ, PEERS=str(N), CONNECTTO="10", FRAGMENTS="2", GS_SEED="5", GS_BATCH="4")
    args = [exe, "-st", "5", "-bl", "50", "-bh", "150", "-ll", "40", "-lh", "130", "-m", str(M), "-s", str(size)]
    subprocess.run(args + ["--message-costs", str(tmp_path / "a")], env=env, check=True, timeout=60)
    subprocess.run(args + ["--message-costs", str(tmp_path / "b"), "--device-log", "--latencies", str(tmp_path / "l")],
                   env=env, check=True, timeout=60)
    sim = gpu_sim(oracle.params(peers=N, seed=5, fragments=2), batch=4)
    sim.set_message_costs()
    sched = gossipsim.schedule_runsh(M, N, 6, 1, gossipsim.T0_NS, gossipsim.DELAY_NS, size)
    sim.run(sched, collect=False)
    got = sim.message_costs()
    assert got.shape == (M, 8) and got[:, R.DATA_TX].all() and got[:, R.DUP].all()
    sim.write_message_costs(str(tmp_path / "py"), sched)
    text = open(str(tmp_path / "py")).read()
    assert text.count("\n") == M + 1 and text.startswith("#msg\tt_pub_ns\t")
    assert open(str(tmp_path / "a")).read() == text
    assert open(str(tmp_path / "b")).read() == text
