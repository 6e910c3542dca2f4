"""Per-peer delay accumulators on the device (gs_set_peer_delay, csrc/gs_peerdelay.h) and the
nim node's metrics written from them (gs_write_testnode_metrics).

The reference of every check is the numpy restatement `_restate` below, fed the oracle's
t_complete reduced to the logged ms (test_gpu_features._logged_ms) or a crafted array, never
a device result:
    ms     = (t_complete - t_pub) // 10^6 over delivered pairs (publisher row only with self_log)
    bucket = np.searchsorted(bounds, ms, side="left")
    last   = the observation with the largest (t_pub + ms * 10^6, t_pub)
"""
import os
import subprocess

import numpy as np
import pytest

import gossipsim
import oracle
from test_gpu_features import _logged_ms
from test_gpu_parity import T0, _sched, gpu_sim
from test_gpu_part_log import CASES, N_CASE, _ranges
from test_gpu_partition import _parts

pytestmark = pytest.mark.gpu
LINKS = (50, 150, 40, 130)
NONE = gossipsim.LAT_NONE
UND = gossipsim.UNDELIVERED
BOUNDS = np.array(gossipsim.DELAY_BOUNDS_MS, np.uint16)
DT = gossipsim.PEER_DELAY_DTYPE
MS_NS = np.uint64(1_000_000)
GS_ESTATE, GS_EUNSUPPORTED = -4, -6


def _restate(ms, t_pub, carry=None):
    """The accumulators after the observations ms[M, n] (uint16, LAT_NONE = none) of messages
    published at t_pub[M], on top of `carry` (an earlier result) or of zero."""
    ms = np.asarray(ms, np.uint16)
    M, n = ms.shape
    tp = np.broadcast_to(np.asarray(t_pub, np.uint64)[:, None], (M, n))
    out = np.zeros(n, DT) if carry is None else carry.copy()
    had = out["completed"] > 0
    ok = ms != NONE
    v = np.where(ok, ms, 0).astype(np.uint64)
    out["completed"] += ok.sum(axis=0).astype(np.uint64)
    out["delay_sum_ms"] += v.sum(axis=0)
    b = np.searchsorted(BOUNDS, ms, side="left")
    for i in range(len(BOUNDS) + 1):
        out["bucket"][:, i] += ((b == i) & ok).sum(axis=0).astype(np.uint64)
    rx = np.where(ok, tp + v * MS_NS, 0)
    tpk = np.where(ok, tp, 0)
    top = np.lexsort((tpk, rx, ok), axis=0)[-1]  # per column: the largest (observed, rx, t_pub)
    col = np.arange(n)
    any_ok = ok[top, col]
    n_rx, n_tp, n_ms = rx[top, col], tpk[top, col], v[top, col]
    o_rx = out["last_rx_ns"].copy()
    o_tp = o_rx - out["last_ms"].astype(np.uint64) * MS_NS
    take = any_ok & (~had | (n_rx > o_rx) | ((n_rx == o_rx) & (n_tp > o_tp)))
    out["last_rx_ns"] = np.where(take, n_rx, o_rx)
    out["last_ms"] = np.where(take, n_ms, out["last_ms"]).astype(np.uint32)
    return out


def _same(got, want):
    for f in DT.names:
        np.testing.assert_array_equal(got[f], want[f], err_msg=f)


def _oracle_delay(p, sched, ref):
    return _restate(_logged_ms(ref["t_complete"].copy(), sched, p.self_log), sched[0])


def test_every_edge_no_graph():
    """130 peers (groups of 64, 64 and 2), batch 8, 37 messages (5 pieces, the last partial):
    b - 1, b and b + 1 of every bound, 0, 65534, LAT_NONE, one peer with no observation, and
    two messages whose t_pub + ms * 10^6 tie with different t_pub."""
    N, M = 130, 37
    vals = np.array(sorted({int(b) + d for b in BOUNDS for d in (-1, 0, 1)} | {0, 65534}), np.uint16)
    lat = vals[np.arange(M * N) % len(vals)].reshape(M, N).copy()
    rng = np.random.default_rng(7)
    lat[rng.random((M, N)) < 0.15] = NONE
    lat[:, 77] = NONE
    t = T0 + np.arange(M, dtype=np.uint64) * np.uint64(1_000_000_000)
    t[35:] += np.uint64(1000_000_000_000)  # the last two messages: later than every other arrival
    t[36] = t[35] + np.uint64(5_000_000)
    lat[35, 3], lat[36, 3] = 30, 25        # one arrival instant at peer 3, from two publish times
    lat[35, 4], lat[36, 4] = 30, NONE
    sched = (t, (6 + np.arange(M)) % N, np.full(M, 15000))
    want = _restate(lat, t)
    assert want["last_ms"][3] == 25 and want["last_rx_ns"][3] == int(t[36]) + 25_000_000 == int(t[35]) + 30_000_000
    assert want["last_ms"][4] == 30 and want["completed"][77] == 0 and want["last_rx_ns"][77] == 0
    assert (want["bucket"].sum(axis=0) > 0).all()  # every bucket is hit
    sim = gossipsim.Simulator(peers=N, seed=3, batch=8)
    with pytest.raises(gossipsim.GossipSimError) as e:
        sim.peer_delay()
    assert e.value.status == GS_ESTATE
    sim.set_peer_delay()
    _same(sim.peer_delay(), np.zeros(N, DT))
    sim.peer_delay_add_lat(sched, lat)
    _same(sim.peer_delay(), want)
    # a second call adds on top: the first 20 messages again, 3 s later
    t2 = t[:20] + np.uint64(3_000_000_000)
    sim.peer_delay_add_lat((t2, sched[1][:20], sched[2][:20]), lat[:20])
    _same(sim.peer_delay(), _restate(lat[:20], t2, carry=want))
    sim.reset_peer_delay()
    _same(sim.peer_delay(), np.zeros(N, DT))
    sim.set_peer_delay(False)
    with pytest.raises(gossipsim.GossipSimError) as e:
        sim.peer_delay()
    assert e.value.status == GS_ESTATE


_SINK_REF = {}


def _sink_case():
    if not _SINK_REF:
        p = oracle.params(peers=300, seed=5)
        sched = _sched(12, 300)
        ref = oracle.simulate(p, 5, LINKS, sched=sched)
        _SINK_REF.update(p=p, sched=sched, ref=ref, want=_oracle_delay(p, sched, ref))
    return _SINK_REF


def _run_sink(sim, sched, sink):
    """One run through `sink` -> what the sink itself received."""
    if sink == "none":
        return sim.run(sched, collect=False).get("t_complete")
    if sink == "arrays":
        res = sim.run(sched)
        return res["t_complete"].copy(), res["hops"].copy()
    if sink == "on_lat":
        blocks = []
        sim.run(sched, collect=False, on_lat=lambda first, v: blocks.append((first, v.copy())), block_msgs=2)
        return blocks
    if sink == "on_block":
        blocks = []
        sim.run(sched, on_block=lambda first, a, h: blocks.append((first, a.copy(), h.copy())), block_msgs=2)
        return blocks
    chunks = []
    sim.run_log(sched, on_text=lambda first, n, text, lines: chunks.append((first, n, text, lines)))
    return chunks


def _eq(a, b):
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_eq(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return np.array_equal(a, b)
    return a == b


@pytest.mark.parametrize("sink", ["none", "arrays", "on_lat", "on_block", "run_log"])
def test_one_result_whatever_the_sink(sink):
    """300 peers (no multiple of 64), 12 messages in batches of 5 (three, the last partial):
    the accumulators equal the oracle's through every hook site and with a NULL sink, and the
    sink sees exactly what it sees with the switch off."""
    c = _sink_case()
    out, st = [], []
    for on in (False, True):
        sim, _ = gpu_sim(c["p"], 5, LINKS, batch=5)
        if on:
            sim.set_peer_delay()
        out.append(_run_sink(sim, c["sched"], sink))
        st.append(sim.stats())
        if on:
            _same(sim.peer_delay(), c["want"])
    assert _eq(out[0], out[1])
    for k in ("deliveries", "relaxations", "gossip_iwant", "batches"):
        assert st[0][k] == st[1][k], k
    assert st[1]["batches"] == 3


FLAVOURS = ["rust_f1", "rust_f3", "go", "nim", "gossip_iwant", "churn", "non_lockstep"]
_FL_REF = {}


def _flavour(case):
    """(params, schedule, batch, the oracle's run, the oracle's accumulators), once per case."""
    if case not in _FL_REF:
        if case == "non_lockstep":
            p = oracle.params(peers=N_CASE, seed=98, lazy_gossip=1, hb_phase_ns=int(T0) % 1_000_000_000)
            M, batch = 20, 8
            sched = (T0 + np.arange(M, dtype=np.uint64) * np.uint64(1_500_000_000), (6 + np.arange(M)) % N_CASE,
                     np.full(M, 15000))
        else:
            mk, M, batch, _ = CASES[case]
            p = mk(N_CASE)
            sched = _sched(M, N_CASE)
        ref = oracle.simulate(p, 5, LINKS, sched=sched)
        _FL_REF[case] = (p, sched, batch, ref, _oracle_delay(p, sched, ref))
    return _FL_REF[case]


@pytest.mark.parametrize("case", FLAVOURS)
def test_flavours_and_paths(case):
    """1001 peers, 20 messages, batches of 8: every node flavour and completion path against
    the oracle; the conditions on the oracle's result keep a case from degenerating."""
    p, sched, batch, ref, want = _flavour(case)
    M = len(sched[0])
    tc = ref["t_complete"]
    if case == "churn":
        assert int((tc == UND).sum()) == 2655
        assert [int(x) for x in want["bucket"][:, 9:].sum(axis=0)] == [616, 449, 911, 808]
        ms = _logged_ms(tc.copy(), sched, p.self_log)
        assert int(ms[ms != NONE].max()) == 16486
    if case == "go":
        assert p.self_log == 1 and int(want["bucket"][:, 0].sum()) == M
    if case == "rust_f1":
        assert (tc != UND).all() and (want["completed"] >= M - 1).all()
    sim, _ = gpu_sim(p, 5, LINKS, batch=batch)
    sim.set_peer_delay()
    if case == "non_lockstep":  # array sinks: the class order regroups the batches
        res = sim.run(sched)
        np.testing.assert_array_equal(res["t_complete"], tc)
        np.testing.assert_array_equal(res["hops"], ref["hops"])
        assert sim.stats()["batches"] > (M + batch - 1) // batch
    else:
        sim.run(sched, collect=False)
    _same(sim.peer_delay(), want)
    assert sim.stats()["deliveries"] == ref["stats"]["deliveries"]


def _cat(sims):
    return np.concatenate([s.peer_delay() for s in sims])


_WHOLE = {}


def _whole(case):
    """gs_run's accumulators of the unpartitioned graph, once per case."""
    if case not in _WHOLE:
        mk, M, batch, _ = CASES[case]
        p = mk(N_CASE)
        sim, _ = gpu_sim(p, 5, LINKS, batch=batch)
        sim.set_peer_delay()
        sim.run(_sched(M, N_CASE), collect=False)
        _WHOLE[case] = sim.peer_delay()
    return _WHOLE[case]


@pytest.mark.parametrize("P", [2, 3])
@pytest.mark.parametrize("case", ["rust_f1", "churn", "ms_batch2"])
def test_partitioned(case, P):
    """Loop-back parts at 1001 peers (ranges 333 / 334 / 334): the peer protocols (rust_f1) and
    the message-sharded batches (churn; batches of 2 over the parts), with NULL sinks and
    through the log's text: the parts' arrays side by side are gs_run's and the oracle's."""
    mk, M, batch, _ = CASES[case]
    p = mk(N_CASE)
    sched = _sched(M, N_CASE)
    want = _oracle_delay(p, sched, oracle.simulate(p, 5, LINKS, sched=sched)) if case == "ms_batch2" \
        else _flavour(case)[4]
    _same(_whole(case), want)
    sims = _parts(p, 5, LINKS, P, batch)
    for s in sims:
        s.set_peer_delay()
    comm = gossipsim.Comm(local_parts=P)
    assert comm.run_partitioned(sims, sched, collect=False) is None
    assert [len(s.peer_delay()) for s in sims] == [u1 - u0 for u0, u1 in _ranges(N_CASE, P)]
    _same(_cat(sims), want)
    ms_b = [s.stats()["ms_batches"] for s in sims]
    assert all(x == 0 for x in ms_b) if case == "rust_f1" else all(x > 0 for x in ms_b)
    for s in sims:
        s.reset_peer_delay()
    _same(_cat(sims), np.zeros(N_CASE, DT))
    comm.run_partitioned_log(sims, sched, on_text=lambda *a: None)
    _same(_cat(sims), want)
    comm.close()


def test_one_rccl_rank():
    """One RCCL rank on the churn shape of test_gpu_part_log.test_one_rccl_rank: the
    message-sharded pack / send / recv path, the switch in the ranks' configuration word."""
    N, M = 2000, 12
    p = oracle.params(peers=N, seed=59, churn_ppm=20000, hb_phase_ns=gossipsim.SHADOW_START_NS, lazy_gossip=1)
    sched = _sched(M, N)
    want = _oracle_delay(p, sched, oracle.simulate(p, 5, LINKS, sched=sched))
    (s,) = _parts(p, 5, LINKS, 1, M)
    s.set_peer_delay()
    comm = gossipsim.Comm(nranks=1, rank=0, uid=gossipsim.Comm.get_id(), device=0)
    comm.run_partitioned([s], sched, collect=False)
    _same(s.peer_delay(), want)
    assert s.stats()["ms_batches"] > 0
    comm.close()


def test_partitioned_rules():
    """Parts that disagree on the switch: GS_EINVAL; the caller-driven protocol with the
    switch on, and gs_run on a context that holds one of two parts: GS_EUNSUPPORTED."""
    N = 300
    p = oracle.params(peers=N, seed=5)
    sched = _sched(2, N)
    sims = _parts(p, 5, LINKS, 2, 4)
    sims[0].set_peer_delay()
    comm = gossipsim.Comm(local_parts=2)
    with pytest.raises(gossipsim.GossipSimError) as e:
        comm.run_partitioned(sims, sched, collect=False)
    assert e.value.status == gossipsim.GS_EINVAL
    comm.close()
    with pytest.raises(gossipsim.GossipSimError) as e:
        sims[0].part_begin(sched)
    assert e.value.status == GS_EUNSUPPORTED
    with pytest.raises(gossipsim.GossipSimError) as e:
        sims[0].run(sched, collect=False)
    assert e.value.status == GS_EUNSUPPORTED
    sims[1].run(sched, collect=False)  # (the switch off: as before)
    assert sims[1].part_begin(sched) != gossipsim.KEY_NONE


def test_erange():
    """A logged latency of 65535 ms or more (the 70 s heartbeat churn shape of
    test_gpu_log_text.test_errors) with the switch on and no sink: GS_ERANGE, whole and with
    2 parts; after reset_peer_delay a good run on the same contexts matches the oracle."""
    N = 300
    hb = 70_000_000_000
    t0 = (946684800 + 500) * 1_000_000_000
    phase = t0 - 10 * hb + 20_000_000_000
    p = oracle.params(peers=N, seed=5, churn_ppm=150000, churn_down=1, churn_horizon=4, heartbeat_ns=hb,
                      hb_phase_ns=phase, lazy_gossip=1)
    rows = gossipsim.schedule_runsh(6, N, 6, 1, t0 + gossipsim.HTTP_TRANSIT_NS, 1_000_000_000, 15000)
    cols = (np.array([r.t_pub_ns for r in rows], dtype=np.uint64), np.array([r.publisher for r in rows]),
            np.array([r.msg_size for r in rows]))
    ref = oracle.simulate(p, 5, LINKS, sched=cols)
    wide = (ref["t_complete"] - cols[0][:, None]) // MS_NS
    wide[ref["t_complete"] == UND] = 0
    assert int(wide.max()) >= 65535
    good = int(np.nonzero(wide.max(axis=1) < 65535)[0][0])  # a message whose latencies all fit
    one = tuple(c[good:good + 1] for c in cols)
    want = _oracle_delay(p, one, oracle.simulate(p, 5, LINKS, sched=one))
    sim, _ = gpu_sim(p, 5, LINKS)
    sim.set_peer_delay()
    with pytest.raises(gossipsim.GossipSimError) as e:
        sim.run(cols, collect=False)
    assert e.value.status == gossipsim.GS_ERANGE
    sim.reset_peer_delay()
    sim.run(one, collect=False)
    _same(sim.peer_delay(), want)
    sims = _parts(p, 5, LINKS, 2, 64)
    for s in sims:
        s.set_peer_delay()
    comm = gossipsim.Comm(local_parts=2)
    with pytest.raises(gossipsim.GossipSimError) as e:
        comm.run_partitioned(sims, cols, collect=False)
    assert e.value.status == gossipsim.GS_ERANGE
    for s in sims:
        s.reset_peer_delay()
    comm.run_partitioned(sims, one, collect=False)
    _same(_cat(sims), want)
    comm.close()


def test_cli_testnode_metrics(tmp_path):
    """gossipsim-node --testnode-metrics, with and without --device-log: the file is
    write_testnode_metrics over the Python run's array, which is the oracle's."""
    exe = os.path.join(os.path.dirname(gossipsim.LIB_PATH), "gossipsim-node")
    N, M = 300, 6
    env = dict(os.environ, PEERS=str(N), CONNECTTO="10", FRAGMENTS="1", GS_SEED="5", GS_BATCH="4")
    args = [exe, "-st", "5", "-bl", "50", "-bh", "150", "-ll", "40", "-lh", "130", "-m", str(M), "-s", "15000"]
    subprocess.run(args + ["--testnode-metrics", str(tmp_path / "a")], env=env, check=True, timeout=60)
    subprocess.run(args + ["--testnode-metrics", str(tmp_path / "b"), "--latencies", str(tmp_path / "lat"),
                           "--device-log"], env=env, check=True, timeout=60)
    p = oracle.params(peers=N, seed=5)
    sim, _ = gpu_sim(p, 5, LINKS, batch=4)
    sim.set_peer_delay()
    rows = gossipsim.schedule_runsh(M, N, 6, 1, gossipsim.T0_NS, gossipsim.DELAY_NS, 15000)
    sim.run(rows, collect=False)
    cols = (np.array([r.t_pub_ns for r in rows], dtype=np.uint64), np.array([r.publisher for r in rows]),
            np.array([r.msg_size for r in rows]))
    _same(sim.peer_delay(), _oracle_delay(p, cols, oracle.simulate(p, 5, LINKS, sched=cols)))
    sim.write_testnode_metrics(str(tmp_path / "py"), rows)
    want = open(str(tmp_path / "py"), "rb").read()
    assert want.count(b"dst_testnode_completed_messages_total{") == N
    assert open(str(tmp_path / "a"), "rb").read() == want
    assert open(str(tmp_path / "b"), "rb").read() == want
    assert open(str(tmp_path / "lat"), "rb").read().count(b"\n") == M * (N - 1)
