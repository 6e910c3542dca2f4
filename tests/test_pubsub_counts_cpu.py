"""Host side of the per-peer pubsub event counts (no GPU): the reference decomposition of
tests/pubsub_ref.py on the oracle alone, gs_write_pubsub_metrics on a hand-made array against a
text built here, NULL arguments, the header's enum and the INTEGRATION.md / Rust entries."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gossipsim
import oracle
import pubsub_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T0 = gossipsim.T0_NS
LINKS = (50, 150, 40, 130)
PHASE = T0 % 1_000_000_000  # a heartbeat at the publish instant: IHAVEs race the eager wave

# (family, help of go-test-node/metrics.go:84-220, topic label, column)
FAMILIES = [
    ("libp2p_pubsub_broadcast_messages_total", "pubsub broadcast messages", True, R.MSG_TX),
    ("libp2p_pubsub_received_messages_total", "pubsub received messages", True, R.MSG_RX),
    ("libp2p_pubsub_broadcast_ihave_total", "pubsub broadcast ihave", True, R.IHAVE_TX),
    ("libp2p_pubsub_received_ihave_total", "pubsub received ihave", True, R.IHAVE_RX),
    ("libp2p_pubsub_broadcast_iwant_total", "pubsub broadcast iwant", False, R.IWANT_TX),
    ("libp2p_pubsub_received_iwant_total", "pubsub received iwant", False, R.IWANT_RX),
    ("libp2p_gossipsub_received_total", "number of messages received (deduplicated)", False, R.FIRST),
    ("libp2p_gossipsub_duplicate_total", "number of duplicates received", False, R.DUP),
]


def _sched(M, N, size=240000):
    t = T0 + np.arange(M, dtype=np.uint64) * np.uint64(1_000_000_000)
    return t, (37 * np.arange(M) + 4) % N, np.full(M, size)


@pytest.mark.parametrize("kw", [dict(), dict(fragments=3), dict(node="go", fragments=2)])
def test_reference_identities_on_the_oracle(kw):
    """Frozen mesh: nothing is lost, so every send arrives; the totals are the oracle's own
    counters (relaxations = fragment sends, frag_deliveries = first receipts, gossip_iwant)."""
    kw = dict(kw)
    p = oracle.params_for(kw.pop("node", 0), peers=300, seed=71, hb_phase_ns=PHASE, **kw)
    r = R.reference(p, 5, LINKS, _sched(4, 300))
    c, st = r["counts"].astype(np.int64), r["whole"]["stats"]
    assert r["exact"]
    tot = c.sum(axis=0)
    assert tot[R.MSG_TX] == tot[R.MSG_RX] == st["relaxations"]
    assert tot[R.FIRST] == st["frag_deliveries"] == p.fragments * st["deliveries"]
    assert tot[R.IHAVE_TX] == tot[R.IHAVE_RX] > 0
    assert tot[R.IWANT_TX] == tot[R.IWANT_RX] == st["gossip_iwant"] > 0
    np.testing.assert_array_equal(c[:, R.DUP], c[:, R.MSG_RX] - c[:, R.FIRST])
    assert (c[:, R.DUP] >= 2).all()  # every peer sees the message from several mesh neighbours


def test_reference_under_churn():
    """Losses: sends exceed arrivals. With fragments partial receipts exist, so F x received is
    no per-peer reference and the helper says so."""
    kw = dict(peers=600, seed=71, churn_ppm=20000, heartbeat_ns=200_000_000, hb_phase_ns=T0 - 2_000_000_000,
              churn_horizon=10)
    r = R.reference(oracle.params(**kw), 5, LINKS, _sched(6, 600))
    tot = r["counts"].astype(np.int64).sum(axis=0)
    assert r["exact"] and tot[R.MSG_TX] > tot[R.MSG_RX] and tot[R.FIRST] == r["whole"]["stats"]["frag_deliveries"]
    r2 = R.reference(oracle.params(fragments=2, **kw), 5, LINKS, _sched(6, 600))
    assert not r2["exact"]
    assert r2["whole"]["stats"]["frag_deliveries"] > 2 * int(r2["whole"]["traffic"][:, R.TR_RECEIVED].sum())


def test_reference_rejects_an_undecidable_input():
    """15000 bytes in 3 fragments: a peer's IHAVEs of one message exceed one fragment's wire
    bytes, the split is not unique and the helper fails instead of guessing."""
    p = oracle.params(peers=300, seed=71, fragments=3, hb_phase_ns=PHASE)
    with pytest.raises(AssertionError):
        R.reference(p, 5, LINKS, _sched(4, 300, size=15000))


def _crafted():
    c = np.zeros((3, R.COLS), np.uint64)
    c[0] = [70, 61, 12, 49, 300, 280, 2, 3]
    c[1] = [2 ** 40 + 5, 9, 9, 0, 0, 1, 0, 0]
    return c


def _expected(mux, c):
    out = []
    for name, text, topic, col in FAMILIES:
        out.append("# HELP %s %s\n# TYPE %s counter\n" % (name, text, name))
        for u in range(len(c)):
            out.append('%s{%speer_id="pod-%d"} %d\n' % (name, 'topic="test",' if topic else "", u, c[u, col]))
    name = "dst_testnode_received_chunks_total"
    out.append("# HELP %s number of application-level message chunks received\n# TYPE %s counter\n" % (name, name))
    for u in range(len(c)):
        out.append('%s{muxer="%s",peer_id="pod-%d"} %d\n' % (name, mux, u, c[u, R.FIRST]))
    return "".join(out)


@pytest.mark.parametrize("mux", ["yamux", "quic", "mplex"])
def test_writer_against_expected_text(tmp_path, mux):
    c = _crafted()
    cfg = gossipsim.PeerConfig(peers=3, connect_to=1, muxer=mux)
    path = str(tmp_path / "m")
    gossipsim.write_pubsub_metrics(cfg, path, c)
    got = open(path).read()
    assert got == _expected(mux, c)
    assert got.count('topic="test"') == 4 * 3 and got.count("# TYPE") == 9
    assert 'libp2p_pubsub_broadcast_messages_total{topic="test",peer_id="pod-1"} %d\n' % (2 ** 40 + 5) in got
    with pytest.raises(gossipsim.GossipSimError):
        gossipsim.write_pubsub_metrics(cfg, path, np.zeros((3, 7), np.uint64))


def test_null_arguments(tmp_path):
    L = gossipsim.lib()
    c = _crafted()
    cfg = gossipsim.PeerConfig(peers=3, connect_to=1)
    good = [ctypes.byref(cfg.c), str(tmp_path / "x").encode(), 3, c.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))]
    assert L.gs_write_pubsub_metrics(*good) == 0
    for k in (0, 1, 3):
        args = list(good)
        args[k] = None
        assert L.gs_write_pubsub_metrics(*args) == gossipsim.GS_EINVAL, k
    args = list(good)
    args[1] = str(tmp_path / "no_such_dir" / "x").encode()
    assert L.gs_write_pubsub_metrics(*args) == gossipsim.GS_EINVAL
    for fn, extra in (("gs_set_pubsub_counts", (1,)), ("gs_get_pubsub_counts", (None,)),
                      ("gs_reset_pubsub_counts", ())):
        assert getattr(L, fn)(None, *extra) == gossipsim.GS_EINVAL, fn


def test_header_enum_and_bindings():
    hdr = open(os.path.join(ROOT, "include", "gossipsim.h")).read()
    want = dict(GS_PS_MSG_TX=0, GS_PS_MSG_RX=1, GS_PS_FIRST=2, GS_PS_DUP=3, GS_PS_IHAVE_TX=4, GS_PS_IHAVE_RX=5,
                GS_PS_IWANT_TX=6, GS_PS_IWANT_RX=7, GS_PUBSUB_COLS=8)
    for name, val in want.items():
        m = re.search(r"\b%s = (\d+)" % name, hdr)
        assert m and int(m.group(1)) == val, name
    assert re.search(r"#define GS_ABI_VERSION 10u", hdr)
    assert len(gossipsim.PUBSUB_COLS) == R.COLS == 8
    assert gossipsim.PUBSUB_COLS.index("first") == R.FIRST and gossipsim.PUBSUB_COLS.index("iwant_rx") == R.IWANT_RX
    for fn in ("gs_set_pubsub_counts", "gs_get_pubsub_counts", "gs_reset_pubsub_counts", "gs_write_pubsub_metrics"):
        assert re.search(r"gs_status %s\(" % fn, hdr), fn


def test_integration_md_and_rust_name_the_entries():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    rs = open(os.path.join(ROOT, "rust", "gossipsim-sys", "src", "lib.rs")).read()
    for fn in ("gs_set_pubsub_counts", "gs_get_pubsub_counts", "gs_reset_pubsub_counts", "gs_write_pubsub_metrics"):
        assert "`%s`" % fn in text, fn
        assert re.search(r"pub fn %s\(" % fn, rs), fn
    assert "metrics.go:84-220" in text and "main.nim:37-41" in text
    assert re.search(r"pub const GS_PUBSUB_COLS: usize = 8;", rs)
