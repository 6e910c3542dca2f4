"""The arrival log of peer-partitioned runs (gs_run_partitioned_log, and on_lat
through gs_run_partitioned): each part formats, or streams, the lines of its own
peers. A part's text is gs_run_log's text of the unpartitioned run with only the
lines of the part's peers kept; for the cases marked "oracle" the reference is
the host writer over the oracle's logged ms (test_gpu_features._logged_ms),
filtered the same way. Loop-back parts on one GPU, and one RCCL rank."""
import numpy as np
import pytest

import gossipsim
import oracle
from test_gpu_features import _logged_ms
from test_gpu_log_text import _Chunks, _host_text
from test_gpu_partition import _parts, _sched

pytestmark = pytest.mark.gpu
T0 = gossipsim.T0_NS
LINKS = (50, 150, 40, 130)
NONE = gossipsim.LAT_NONE
SUMMED = ("deliveries", "frag_deliveries", "latency_sum_ms")


def _ranges(N, P):
    return [(i * N // P, (i + 1) * N // P) for i in range(P)]


def _filter(text, u0, u1):
    """The lines of peers [u0, u1), in their order."""
    keep = []
    for line in text.splitlines(keepends=True):
        assert line.startswith(b"shadow.data/hosts/peer")
        if u0 <= int(line[22:line.index(b"/", 22)]) < u1:
            keep.append(line)
    return b"".join(keep)


class _PartChunks:
    """on_text of Comm.run_partitioned_log: one _Chunks per part."""

    def __init__(self, P):
        self.parts = [_Chunks() for _ in range(P)]

    def __call__(self, part, first, n, text, lines):
        self.parts[part](first, n, text, lines)


def _whole_log(p, sched, batch):
    """gs_run_log on an unpartitioned simulator -> (text, its counters)."""
    (sim,) = _parts(p, 5, LINKS, 1, batch)
    got = _Chunks()
    sim.run_log(sched, on_text=got)
    return got.text(), sim.stats()


def _oracle_text(p, sched, tmp_path, name="oracle"):
    ref = oracle.simulate(p, 5, LINKS, sched=sched)
    ms = _logged_ms(ref["t_complete"].copy(), sched, p.self_log)
    sim = gossipsim.Simulator(**{n: getattr(p, n) for n, _ in oracle.OrParams._fields_})
    return _host_text(sim.cfg, tmp_path, sim._schedule(sched), [(0, ms)], name), ref, ms


def _check_parts(got, want, N, P, M):
    for (u0, u1), ch in zip(_ranges(N, P), got.parts):
        assert ch.text() == _filter(want, u0, u1), (u0, u1)
        assert ch.tiles(M)
    assert sum(ch.lines() for ch in got.parts) == want.count(b"\n")


@pytest.mark.parametrize("N,P", [(10050, 8), (130, 3), (130, 8)])
def test_formatter_over_ranges_digit_boundaries(tmp_path, N, P):
    """Peer-id digit boundaries inside parts (10050 / 8: part 7 owns 8793..10049 and crosses
    9999 / 10000, part 0 crosses 9 / 10, 99 / 100 and 999 / 1000; no first peer but 0 is a
    multiple of 64), and parts smaller than one wave (130 / 3: 43, 43, 44 peers; 130 / 8:
    16 or 17). (oracle)"""
    M = 3
    p = oracle.params(peers=N, seed=71)
    sched = _sched(M, N)
    want, ref, _ = _oracle_text(p, sched, tmp_path)
    sims = _parts(p, 5, LINKS, P, 4)
    comm = gossipsim.Comm(local_parts=P)
    got = _PartChunks(P)
    n = comm.run_partitioned_log(sims, sched, on_text=got)
    _check_parts(got, want, N, P, M)
    assert sum(n) == ref["stats"]["deliveries"] == sum(s.stats()["deliveries"] for s in sims)
    assert all(u0 % 64 for u0, _ in _ranges(N, P)[1:])
    comm.close()


CASES = {
    # name: (params, messages, batch, oracle reference?)
    "rust_f1": (lambda N: oracle.params(peers=N, seed=98), 20, 8, True),
    "rust_f3": (lambda N: oracle.params(peers=N, seed=98, fragments=3), 20, 8, False),
    "push": (lambda N: oracle.params(peers=N, seed=98), 20, 8, False),
    "nim": (lambda N: oracle.params_for("nim", peers=N, seed=98), 20, 8, False),
    "gossip_iwant": (lambda N: oracle.params(peers=N, seed=98, lazy_gossip=1, hb_phase_ns=T0 % 1_000_000_000), 20, 8,
                     False),
    "churn": (lambda N: oracle.params(peers=N, seed=98, churn_ppm=20000, hb_phase_ns=gossipsim.SHADOW_START_NS,
                                      lazy_gossip=1), 20, 8, True),
    "go": (lambda N: oracle.params_for("go", peers=N, seed=98), 20, 8, True),
    "ms_batch2": (lambda N: oracle.params(peers=N, seed=98, churn_ppm=20000, hb_phase_ns=gossipsim.SHADOW_START_NS,
                                          lazy_gossip=1), 6, 2, False),
}
N_CASE = 1001  # ranges 333 / 334 / 334 with P = 3
_REFS = {}


def _case(case, tmp_path):
    """(params, schedule, batch, reference text, gs_run's counters, the logged ms or None), once per case."""
    if case not in _REFS:
        mk, M, batch, ora = CASES[case]
        p = mk(N_CASE)
        sched = _sched(M, N_CASE)
        whole, st = _whole_log(p, sched, batch)
        want, ms = whole, None
        if ora:
            want, _, ms = _oracle_text(p, sched, tmp_path, "oracle_" + case)
        _REFS[case] = (p, sched, batch, want, st, ms)
    return _REFS[case]


@pytest.mark.parametrize("P", [2, 3, 8])
@pytest.mark.parametrize("case", [c for c in CASES if c != "ms_batch2"])
def test_every_batch_path(tmp_path, monkeypatch, case, P):
    """gs_run_partitioned_log on every partitioned batch path — the list pass (final logs,
    k_lcomplete; fragment groups, k_complete), the push protocol, the publishers' own lines,
    and the message-sharded batches (lazy gossip whose IWANTs count, churn, IDONTWANT:
    k_lat_rows): a part's text is the reference's lines of its peers, the counters summed
    over the parts are gs_run's."""
    p, sched, batch, want, rst, ms = _case(case, tmp_path)
    M = len(sched[0])
    if case == "push":
        monkeypatch.setenv("GS_PART_PUSH", "1")
    if case == "nim":
        assert p.self_log == 1
    if case == "churn":
        assert int((ms == NONE).sum()) > M  # undelivered pairs beside the publishers' rows
    sims = _parts(p, 5, LINKS, P, batch)
    comm = gossipsim.Comm(local_parts=P)
    got = _PartChunks(P)
    comm.run_partitioned_log(sims, sched, on_text=got)
    _check_parts(got, want, N_CASE, P, M)
    st = [s.stats() for s in sims]
    for k in SUMMED:
        assert sum(x[k] for x in st) == rst[k], k
    if case == "rust_f1":
        assert all(x["list_pull_batches"] > 0 for x in st)
    if case == "push":
        assert all(x["list_pull_batches"] == 0 and x["ms_batches"] == 0 for x in st)
    if case == "gossip_iwant":
        assert all(x["gossip_fallback_batches"] > 0 for x in st)
    if case in ("gossip_iwant", "churn", "go"):
        assert all(x["ms_batches"] > 0 for x in st)
    comm.close()


def test_message_sharded_batch_smaller_than_parts(tmp_path):
    """Batches of 2 messages over 3 parts: a part with no message of the batch still
    formats its own peers' lines of it."""
    p, sched, batch, want, rst, _ = _case("ms_batch2", tmp_path)
    M = len(sched[0])
    sims = _parts(p, 5, LINKS, 3, batch)
    comm = gossipsim.Comm(local_parts=3)
    got = _PartChunks(3)
    comm.run_partitioned_log(sims, sched, on_text=got)
    _check_parts(got, want, N_CASE, 3, M)
    st = [s.stats() for s in sims]
    assert all(x["ms_batches"] == M // batch for x in st)
    for k in SUMMED:
        assert sum(x[k] for x in st) == rst[k], k
    comm.close()


def test_chunks(tmp_path):
    """chunk_bytes of about 3 messages of a part's bound: chunks of 3, 3, 2 messages inside
    the batches of 8, each within the budget; chunk_bytes = 1: one message per call."""
    p, sched, batch, want, _, _ = _case("rust_f1", tmp_path)
    M, P = len(sched[0]), 3
    sims = _parts(p, 5, LINKS, P, batch)
    comm = gossipsim.Comm(local_parts=P)
    budget = 3 * 334 * gossipsim.log_line_max(sims[0].cfg)
    got = _PartChunks(P)
    comm.run_partitioned_log(sims, sched, on_text=got, chunk_bytes=budget)
    _check_parts(got, want, N_CASE, P, M)
    for ch in got.parts:
        assert [c[1] for c in ch.calls] == [3, 3, 2, 3, 3, 2, 3, 1]
        assert all(len(c[2]) <= budget for c in ch.calls)
    for s in sims:
        s.log_text_reset()
    one = _PartChunks(P)
    comm.run_partitioned_log(sims, sched, on_text=one, chunk_bytes=1)
    _check_parts(one, want, N_CASE, P, M)
    assert all([c[1] for c in ch.calls] == [1] * M for ch in one.parts)
    comm.close()


def test_counters_carried_and_reset(tmp_path):
    """Two calls (12 + 8 messages) give one whole reference; after log_text_reset on every
    simulator the first call's text repeats; after another split the numbering starts at 1."""
    p, sched, batch, want, _, _ = _case("rust_f1", tmp_path)
    M, P, M1 = len(sched[0]), 3, 12
    cut = lambda a, b: tuple(x[a:b] for x in sched)
    first, _ = _whole_log(p, cut(0, M1), batch)
    assert want.startswith(first)
    sims = _parts(p, 5, LINKS, P, batch)
    comm = gossipsim.Comm(local_parts=P)
    a, b = _PartChunks(P), _PartChunks(P)
    comm.run_partitioned_log(sims, cut(0, M1), on_text=a)
    comm.run_partitioned_log(sims, cut(M1, M), on_text=b)
    for (u0, u1), x, y in zip(_ranges(N_CASE, P), a.parts, b.parts):
        assert x.text() + y.text() == _filter(want, u0, u1)
        assert x.tiles(M1) and y.tiles(M - M1)
    for s in sims:
        s.log_text_reset()
    c = _PartChunks(P)
    comm.run_partitioned_log(sims, cut(0, M1), on_text=c)
    _check_parts(c, first, N_CASE, P, M1)
    comm.close()
    comm = gossipsim.Comm(local_parts=2)  # the first two simulators as the halves of another split
    d = _PartChunks(2)
    comm.run_partitioned_log(sims[:2], cut(0, M1), on_text=d)
    _check_parts(d, first, N_CASE, 2, M1)
    comm.close()


LAT_CASES = {
    "rust": lambda N: oracle.params(peers=N, seed=98),
    "nim": lambda N: oracle.params_for("nim", peers=N, seed=98),
    "churn": CASES["churn"][0],
    "gossip_iwant": CASES["gossip_iwant"][0],
}


class _Blocks:
    def __init__(self, P):
        self.parts = [dict() for _ in range(P)]

    def __call__(self, part, first, lat):
        assert first not in self.parts[part]
        self.parts[part][first] = lat.copy()

    def whole(self):
        return np.concatenate([np.concatenate([b[k] for k in sorted(b)]) for b in self.parts], axis=1)


@pytest.mark.parametrize("P", [2, 3])
@pytest.mark.parametrize("case", list(LAT_CASES))
def test_on_lat_stream(case, P):
    """on_lat through gs_run_partitioned, alone and beside the arrays: blocks of 6 inside
    the batches of 8, [n][own peers]; the parts side by side are the oracle's logged ms."""
    N, M = N_CASE, 20
    p = LAT_CASES[case](N)
    sched = _sched(M, N)
    ref = oracle.simulate(p, 5, LINKS, sched=sched)
    want = _logged_ms(ref["t_complete"].copy(), sched, p.self_log)
    sims = _parts(p, 5, LINKS, P, 8)
    comm = gossipsim.Comm(local_parts=P)
    got = _Blocks(P)
    assert comm.run_partitioned(sims, sched, collect=False, on_lat=got, block_msgs=6) is None
    for (u0, u1), b in zip(_ranges(N, P), got.parts):
        assert sorted(b) == [0, 6, 8, 14, 16]
        assert all(v.shape[1] == u1 - u0 for v in b.values())
    np.testing.assert_array_equal(got.whole(), want)
    both = _Blocks(P)
    res = comm.run_partitioned(sims, sched, on_lat=both, block_msgs=6)
    np.testing.assert_array_equal(both.whole(), want)
    np.testing.assert_array_equal(np.concatenate([r["t_complete"] for r in res], axis=1), ref["t_complete"])
    np.testing.assert_array_equal(np.concatenate([r["hops"] for r in res], axis=1), ref["hops"])
    comm.close()


def test_on_lat_beside_summary_and_sink_rules():
    """on_lat beside a summary on list-pass batches; on_lat without GS_WANT_LAT_MS, and the
    bit without on_lat, are GS_EINVAL for any part's sink."""
    N, M, P = N_CASE, 20, 3
    p = oracle.params(peers=N, seed=98)
    sched = _sched(M, N)
    ref = oracle.simulate(p, 5, LINKS, sched=sched)
    want = _logged_ms(ref["t_complete"].copy(), sched, p.self_log)
    sims = _parts(p, 5, LINKS, P, 8)
    comm = gossipsim.Comm(local_parts=P)
    got = _Blocks(P)
    res = comm.run_partitioned(sims, sched, collect=False, summary=True, on_lat=got, block_msgs=6)
    np.testing.assert_array_equal(got.whole(), want)
    delivered = sum(np.array([x.delivered for x in r["summary"]], np.uint64) for r in res)
    np.testing.assert_array_equal(delivered, (want != NONE).sum(axis=1).astype(np.uint64))
    assert all(s.stats()["list_pull_batches"] > 0 for s in sims)
    for kw in (dict(on_lat=_Blocks(P), want=0), dict(want=gossipsim.WANT_LAT_MS)):
        with pytest.raises(gossipsim.GossipSimError) as e:
            comm.run_partitioned(sims, sched, collect=False, **kw)
        assert e.value.status == gossipsim.GS_EINVAL
    comm.close()


def test_errors():
    """NULL on_text: GS_EINVAL. A logged latency of 65535 ms or more (the 70 s heartbeat
    churn shape of test_gpu_log_text.test_errors) with 2 parts: GS_ERANGE from the text
    and from on_lat, and no part hands out anything of the failing batch; after
    log_text_reset a good call on the same contexts gives the reference text. Traffic and
    gs_run_log on a partitioned context stay GS_EUNSUPPORTED."""
    N, P = 300, 2
    hb = 70_000_000_000
    t0 = (946684800 + 500) * 1_000_000_000
    phase = t0 - 10 * hb + 20_000_000_000
    p = oracle.params(peers=N, seed=5, churn_ppm=150000, churn_down=1, churn_horizon=4, heartbeat_ns=hb,
                      hb_phase_ns=phase, lazy_gossip=1)
    sched = gossipsim.schedule_runsh(6, N, 6, 1, t0 + gossipsim.HTTP_TRANSIT_NS, 1_000_000_000, 15000)
    sims = _parts(p, 5, LINKS, P, 64)
    comm = gossipsim.Comm(local_parts=P)
    with pytest.raises(gossipsim.GossipSimError) as e:
        comm.run_partitioned_log(sims, sched)
    assert e.value.status == gossipsim.GS_EINVAL
    got = _PartChunks(P)
    with pytest.raises(gossipsim.GossipSimError) as e:
        comm.run_partitioned_log(sims, sched, on_text=got)
    assert e.value.status == gossipsim.GS_ERANGE
    assert all(ch.calls == [] for ch in got.parts)
    blocks = _Blocks(P)
    with pytest.raises(gossipsim.GossipSimError) as e:
        comm.run_partitioned(sims, sched, collect=False, on_lat=blocks)
    assert e.value.status == gossipsim.GS_ERANGE
    assert all(b == {} for b in blocks.parts)
    # a message of the schedule whose latencies all fit, by the unpartitioned gs_run_log
    good = want = None
    for m in range(len(sched)):
        one = (gossipsim.GsPublish * 1)(sched[m])
        try:
            want, _ = _whole_log(p, one, 64)
        except gossipsim.GossipSimError as err:
            assert err.status == gossipsim.GS_ERANGE
            continue
        good = one
        break
    assert good is not None
    for s in sims:
        s.log_text_reset()
    ok = _PartChunks(P)
    comm.run_partitioned_log(sims, good, on_text=ok)
    _check_parts(ok, want, N, P, 1)
    with pytest.raises(gossipsim.GossipSimError) as e:
        sims[0].run_log(good, on_text=_Chunks())
    assert e.value.status == -6  # GS_EUNSUPPORTED
    for s in sims:
        s.set_traffic(True)
    with pytest.raises(gossipsim.GossipSimError) as e:
        comm.run_partitioned_log(sims, good, on_text=_PartChunks(P))
    assert e.value.status == -6  # GS_EUNSUPPORTED
    comm.close()


@pytest.mark.parametrize("case", ["frozen", "churn"])
def test_one_rccl_rank(case):
    """One RCCL rank (the part is all peers): the frozen mesh on the peer protocols, and
    churn on the message-sharded pack / send / recv path with the error word agreed through
    the rank collective; the text is gs_run_log's, byte for byte."""
    N, M = 2000, 12
    kw = dict(peers=N, seed=59)
    if case == "churn":
        kw.update(churn_ppm=20000, hb_phase_ns=gossipsim.SHADOW_START_NS, lazy_gossip=1)
    p = oracle.params(**kw)
    sched = _sched(M, N)
    want, rst = _whole_log(p, sched, M)
    (s,) = _parts(p, 5, LINKS, 1, M)
    comm = gossipsim.Comm(nranks=1, rank=0, uid=gossipsim.Comm.get_id(), device=0)
    got = _PartChunks(1)
    (n,) = comm.run_partitioned_log([s], sched, on_text=got)
    assert got.parts[0].text() == want and got.parts[0].tiles(M)
    assert n == want.count(b"\n")
    st = s.stats()
    assert st["deliveries"] == rst["deliveries"]
    assert (st["ms_batches"] > 0) == (case == "churn")
    comm.close()
