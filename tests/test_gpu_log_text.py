"""The arrival log formatted on the device (gs_run_log / gs_format_lat_log,
csrc/gs_logtext.h): the text handed out, chunk after chunk, is byte for byte
what the host writer (gs_log_write_lat through LogStream.write_lat) writes for
the same latencies — the line main.rs:93 prints in the grep form of
shadow/run.sh:61. Synthetic latencies go through the host writer directly;
simulated runs take the oracle's t_complete, reduced to the logged ms
(test_gpu_features._logged_ms), through the same host writer."""
import os
import subprocess

import numpy as np
import pytest

import gossipsim
import oracle
from test_gpu_features import _logged_ms
from test_gpu_parity import T0, _knobs, _sched, gpu_sim

pytestmark = pytest.mark.gpu
LINKS = (50, 150, 40, 130)
NONE = gossipsim.LAT_NONE


def _host_text(cfg, tmp_path, rows, blocks, name="host"):
    """One host LogStream fed the latency blocks [(first, lat[n, N])] in order -> its bytes."""
    path = str(tmp_path / name)
    log = gossipsim.LogStream(cfg, path)
    for first, lat in blocks:
        log.write_lat(rows[first:first + lat.shape[0]], lat)
    log.close()
    return open(path, "rb").read()


class _Chunks:
    def __init__(self):
        self.calls = []

    def __call__(self, first, n, text, lines):
        assert text.count(b"\n") == lines and (not text or text.endswith(b"\n"))
        self.calls.append((first, n, text, lines))

    def text(self):
        return b"".join(c[2] for c in self.calls)

    def lines(self):
        return sum(c[3] for c in self.calls)

    def tiles(self, M, first=0):
        """first_msg / n_msgs tile [first, first + M) in order."""
        at = first
        for f, n, _, _ in self.calls:
            assert f == at and n >= 1
            at += n
        return at == first + M


def _rows(sim, sched):
    return sim._schedule(sched)


def test_peer_id_digit_boundaries(tmp_path):
    """peers = 10 050 (ids of 1 to 5 digits), every digit count of the ms, LAT_NONE at
    random, a whole 64-peer group and a whole message empty, the publisher rows; the
    default chunk and one message per chunk."""
    N, M = 10050, 3
    rng = np.random.default_rng(11)
    vals = np.array([0, 9, 10, 99, 100, 999, 1000, 9999, 10000, 65534], np.uint16)
    lat = vals[(np.arange(M * N) % len(vals))].reshape(M, N).copy()
    lat[rng.random((M, N)) < 0.15] = NONE
    lat[0, 128:192] = NONE          # one whole group of 64 peers
    lat[1, :] = NONE                # one whole message
    sched = _sched(M, N)
    lat[np.arange(M), np.asarray(sched[1])] = NONE  # the publishers log nothing (rust)
    sim = gossipsim.Simulator(peers=N, seed=3)
    rows = _rows(sim, sched)
    want = _host_text(sim.cfg, tmp_path, rows, [(0, lat)])
    got = _Chunks()
    n = sim.format_lat_log(sched, lat, on_text=got)
    assert got.text() == want
    assert n == got.lines() == int((lat != NONE).sum()) and got.tiles(M)
    sim.log_text_reset()
    one = _Chunks()
    sim.format_lat_log(sched, lat, on_text=one, chunk_bytes=1)  # raised to one message's bound
    assert [(c[0], c[1]) for c in one.calls] == [(0, 1), (1, 1), (2, 1)]
    assert one.calls[1][2] == b"" and one.calls[1][3] == 0
    assert one.text() == want


def test_line_number_boundaries_and_carry(tmp_path):
    """peers = 130 (two full waves and a tail of 2), 1100 messages: peers that log every
    message, every third, or none, so neighbouring lines carry line numbers of different
    digit counts (9/10, 99/100, 999/1000); >= 5 chunks; a second call continues the
    numbering, log_text_reset restarts it."""
    N, M1, M2 = 130, 1100, 50
    M = M1 + M2
    rng = np.random.default_rng(12)
    lat = rng.integers(0, 3000, (M, N)).astype(np.uint16)
    m = np.arange(M)[:, None]
    u = np.arange(N)[None, :]
    lat[(u % 3 == 1) & (m % 3 != 0)] = NONE   # every third message
    lat[(u % 7 == 5) & (m % 10 != 9)] = NONE  # every tenth
    lat[:, 77] = NONE                         # one peer logs nothing
    sched = (T0 + np.arange(M, dtype=np.uint64) * np.uint64(250_000_000), (6 + np.arange(M)) % N, np.full(M, 15000))
    part = lambda a, b: tuple(x[a:b] for x in sched)
    sim = gossipsim.Simulator(peers=N, seed=4)
    rows = _rows(sim, sched)
    want = _host_text(sim.cfg, tmp_path, rows, [(0, lat[:M1]), (M1, lat[M1:])])
    first_len = len(_host_text(sim.cfg, tmp_path, rows, [(0, lat[:M1])], "first"))
    a, b = _Chunks(), _Chunks()
    chunk = first_len // 6
    sim.format_lat_log(part(0, M1), lat[:M1], on_text=a, chunk_bytes=chunk)
    assert len(a.calls) >= 5 and a.tiles(M1)
    assert all(len(c[2]) <= chunk for c in a.calls)
    sim.format_lat_log(part(M1, M), lat[M1:], on_text=b)
    assert b.tiles(M2)
    assert a.text() + b.text() == want
    assert a.text() == want[:first_len]
    assert a.lines() + b.lines() == int((lat != NONE).sum())
    sim.log_text_reset()
    c = _Chunks()
    sim.format_lat_log(part(0, M1), lat[:M1], on_text=c, chunk_bytes=chunk)
    assert c.text() == want[:first_len]


@pytest.mark.parametrize("node", ["nim", "go"])
def test_node_flavours(tmp_path, node):
    """nim: 63-bit msgIds of 18-19 digits; go: tx_time; both with the publishers' own lines."""
    N, M = 65, 40
    rng = np.random.default_rng(13)
    lat = rng.integers(0, 70, (M, N)).astype(np.uint16) ** 2
    lat[rng.random((M, N)) < 0.1] = NONE
    sched = _sched(M, N)
    lat[np.arange(M), np.asarray(sched[1])] = 0  # self log: the publisher's line, 0 ms
    sim = gossipsim.Simulator(**_knobs(oracle.params_for(node, peers=N, seed=14)))
    assert sim.cfg.self_log == 1
    want = _host_text(sim.cfg, tmp_path, _rows(sim, sched), [(0, lat)])
    if node == "nim":
        ids = {len(l.split(b":")[2].split(b" ")[0]) for l in want.splitlines()}
        assert ids <= {17, 18, 19} and 19 in ids
    got = _Chunks()
    sim.format_lat_log(sched, lat, on_text=got, chunk_bytes=3 * N * 100)
    assert len(got.calls) > 1 and got.text() == want


_REFS = {}


def _case(case):
    """(params, schedule, the oracle's run) of a test_latency_ms_stream shape, computed once."""
    if case not in _REFS:
        N, M = 1400, 20
        kw = dict(peers=N, seed=98)
        if case == "churn":
            kw.update(churn_ppm=30000, hb_phase_ns=gossipsim.SHADOW_START_NS)
        elif case == "frags3":
            kw.update(fragments=3)
        elif case == "gossip_370":
            kw.update(hb_phase_ns=(T0 + 370_000_000) % 1_000_000_000)
        if case == "nim_self_log":
            p = oracle.params_for("nim", **kw)
        elif case == "go_idontwant":
            p = oracle.params_for("go", **kw)
            assert p.idontwant == 1000
        else:
            p = oracle.params(**kw)
        sched = _sched(M, N)
        _REFS[case] = (p, sched, oracle.simulate(p, 5, LINKS, sched=sched))
    return _REFS[case]


@pytest.mark.parametrize("case", ["rust", "nim_self_log", "churn", "frags3", "gossip_370", "go_idontwant"])
def test_run_log_against_oracle(tmp_path, case):
    """gs_run_log on every completion path: the text equals the host writer's over the
    oracle's logged ms, with the default chunk and with chunks of about 3 messages
    (batches of 8: chunk sizes 3, 3, 2 across the run), and the counters are gs_run's."""
    p, sched, ref = _case(case)
    N, M = p.peers, len(sched[0])
    ms = _logged_ms(ref["t_complete"].copy(), sched, p.self_log)
    sim, _ = gpu_sim(p, 5, LINKS, batch=8)
    want = _host_text(sim.cfg, tmp_path, _rows(sim, sched), [(0, ms)])
    for chunk in (0, 3 * N * gossipsim.log_line_max(sim.cfg)):
        sim.reset_stats()
        sim.log_text_reset()
        got = _Chunks()
        n = sim.run_log(sched, on_text=got, chunk_bytes=chunk)
        assert got.text() == want, chunk
        assert got.tiles(M)
        assert [c[1] for c in got.calls] == ([8, 8, 4] if not chunk else [3, 3, 2, 3, 3, 2, 3, 1])
        st = sim.stats()
        assert st["deliveries"] == ref["stats"]["deliveries"]
        own = M if p.self_log else 0  # the publishers' own lines are no deliveries
        assert n == got.lines() == st["deliveries"] + own == int((ms != NONE).sum())


def test_run_log_batch_slices(tmp_path):
    """1500 peers, 128 messages in batches of 16 (the batch-slice shape): the text equals
    the on_lat stream of the same simulator class through the host writer; to a file."""
    N, M = 1500, 128
    p = oracle.params(peers=N, seed=301, fragments=1, lazy_gossip=0)
    sched = _sched(M, N)
    sim, _ = gpu_sim(p, 5, LINKS, batch=16)
    rows = _rows(sim, sched)
    blocks = []
    sim.run(sched, collect=False, on_lat=lambda first, v: blocks.append((first, v.copy())), block_msgs=16)
    want = _host_text(sim.cfg, tmp_path, rows, sorted(blocks, key=lambda b: b[0]))
    sim2, _ = gpu_sim(p, 5, LINKS, batch=16)
    out = str(tmp_path / "device")
    n = sim2.run_log(sched, path=out)
    assert open(out, "rb").read() == want
    assert n == want.count(b"\n") == sim2.stats()["deliveries"]
    assert sim2.stats()["batches"] == 8


def test_errors():
    """No callback: GS_EINVAL. A logged latency of 65535 ms or more (the 70 s heartbeat
    shape of test_gpu_parity.test_cli_latency_past_u16): GS_ERANGE, and nothing of the
    failing batch is handed out."""
    sim, _ = gpu_sim(oracle.params(peers=300, seed=5), 5, LINKS)
    with pytest.raises(gossipsim.GossipSimError) as e:
        sim.run_log(_sched(2, 300))
    assert e.value.status == gossipsim.GS_EINVAL
    with pytest.raises(gossipsim.GossipSimError) as e:
        sim.format_lat_log(_sched(2, 300), np.zeros((2, 300), np.uint16))
    assert e.value.status == gossipsim.GS_EINVAL
    hb = 70_000_000_000
    t0 = (946684800 + 500) * 1_000_000_000
    phase = t0 - 10 * hb + 20_000_000_000
    p = oracle.params(peers=300, seed=5, churn_ppm=150000, churn_down=1, churn_horizon=4, heartbeat_ns=hb,
                      hb_phase_ns=phase, lazy_gossip=1)
    sched = gossipsim.schedule_runsh(6, 300, 6, 1, t0 + gossipsim.HTTP_TRANSIT_NS, 1_000_000_000, 15000)
    sim, _ = gpu_sim(p, 5, LINKS)
    got = _Chunks()
    with pytest.raises(gossipsim.GossipSimError) as e:
        sim.run_log(sched, on_text=got)
    assert e.value.status == gossipsim.GS_ERANGE
    assert got.calls == []


def test_cli_device_log_past_u16(tmp_path):
    """A latency the u16 latencies cannot carry (the shape of
    test_gpu_parity.test_cli_latency_past_u16): --device-log falls back to the completion
    times like the default path, and both write the same whole log."""
    exe = os.path.join(os.path.dirname(gossipsim.LIB_PATH), "gossipsim-node")
    hb = 70_000_000_000
    t0 = (946684800 + 500) * 1_000_000_000
    phase = t0 - 10 * hb + 20_000_000_000
    env = dict(os.environ, PEERS="300", CONNECTTO="10", FRAGMENTS="1", GS_SEED="5", GS_CHURN_PPM="150000",
               GS_CHURN_DOWN="1", GS_CHURN_HORIZON="4", GOSSIPSUB_HEARTBEAT_MS=str(hb // 1_000_000),
               GS_HB_PHASE_NS=str(phase), GS_LAZY_GOSSIP="1")
    args = [exe, "-st", "5", "-bl", "50", "-bh", "150", "-ll", "40", "-lh", "130", "-m", "6", "-s", "15000"]
    subprocess.run(args + ["--latencies", str(tmp_path / "a")], env=env, check=True, timeout=120)
    subprocess.run(args + ["--latencies", str(tmp_path / "b"), "--device-log"], env=env, check=True, timeout=120)
    a = open(str(tmp_path / "a"), "rb").read()
    assert max(int(x.rsplit(b" ", 1)[1]) for x in a.splitlines()) >= 65535
    assert a == open(str(tmp_path / "b"), "rb").read()


def test_cli_device_log(tmp_path):
    """gossipsim-node --device-log writes the same --latencies file as the host writer path."""
    exe = os.path.join(os.path.dirname(gossipsim.LIB_PATH), "gossipsim-node")
    env = dict(os.environ, PEERS="900", CONNECTTO="10", FRAGMENTS="1", GS_SEED="99", GS_BATCH="8")
    args = [exe, "-st", "5", "-bl", "50", "-bh", "150", "-ll", "40", "-lh", "130", "-m", "10", "-s", "15000"]
    subprocess.run(args + ["--latencies", str(tmp_path / "a")], env=env, check=True, timeout=60)
    subprocess.run(args + ["--latencies", str(tmp_path / "b"), "--device-log"], env=env, check=True, timeout=60)
    a = open(str(tmp_path / "a"), "rb").read()
    assert a.count(b"\n") == 10 * 899
    assert a == open(str(tmp_path / "b"), "rb").read()
