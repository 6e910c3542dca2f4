"""Host side of the per-peer delay metrics (no GPU): gs_write_testnode_metrics on a crafted
gs_peer_delay array against a text built here, the struct's layout, NULL arguments, and the
INTEGRATION.md entries."""
import ctypes
import os
import re

import numpy as np
import pytest

import gossipsim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LE = ["1.0", "5.0", "10.0", "25.0", "50.0", "100.0", "250.0", "500.0", "1000.0", "2500.0", "5000.0", "10000.0"]
HELP = {
    "dst_testnode_publish_requests_total": ("counter", "number of /publish requests accepted by the test node"),
    "dst_testnode_publish_failures_total": ("counter", "number of failed local publish attempts"),
    "dst_testnode_completed_messages_total": ("counter", "number of application-level messages fully received"),
    "dst_testnode_message_delay_ms_sum": ("counter", "sum of message delays in milliseconds (use with rate)"),
    "dst_testnode_message_delay_ms": ("histogram", "message delay histogram for percentile analysis"),
    "dst_testnode_last_message_delay_ms": ("gauge", "last observed message delay in milliseconds (real-time)"),
    "dst_testnode_mesh_size": ("gauge", "current GossipSub mesh size for the test topic"),
    "dst_testnode_topic_peers": ("gauge", "current number of GossipSub peers for the test topic"),
}


def _crafted():
    """3 peers: one with every bucket hit, one with a single slow message, one with nothing."""
    d = np.zeros(3, gossipsim.PEER_DELAY_DTYPE)
    d["bucket"][0] = np.arange(1, 14)
    d["bucket"][1, 12] = 1
    d["completed"] = d["bucket"].sum(axis=1)
    d["delay_sum_ms"] = [123456, 16486, 0]
    d["last_ms"] = [7, 16486, 0]
    d["last_rx_ns"] = [5_000_000_007_000_000, 5_000_016_486_000_000, 0]
    return d


def _expected(mux, d, published, mesh, deg):
    lab = lambda u: '{muxer="%s",peer_id="pod-%d"}' % (mux, u)
    out = []

    def family(name, values):
        typ, text = HELP[name]
        out.append("# HELP %s %s\n# TYPE %s %s\n" % (name, text, name, typ))
        for u, v in enumerate(values):
            out.append("%s%s %d\n" % (name, lab(u), v))

    family("dst_testnode_publish_requests_total", published)
    family("dst_testnode_publish_failures_total", [0] * len(d))
    family("dst_testnode_completed_messages_total", d["completed"])
    family("dst_testnode_message_delay_ms_sum", d["delay_sum_ms"])
    name = "dst_testnode_message_delay_ms"
    out.append("# HELP %s %s\n# TYPE %s histogram\n" % (name, HELP[name][1], name))
    for u in range(len(d)):
        cum = np.cumsum(d["bucket"][u])
        for le, c in zip(LE + ["+Inf"], cum):
            out.append('%s_bucket{muxer="%s",peer_id="pod-%d",le="%s"} %d\n' % (name, mux, u, le, c))
        out.append("%s_sum%s %d\n" % (name, lab(u), d["delay_sum_ms"][u]))
        out.append("%s_count%s %d\n" % (name, lab(u), cum[-1]))
    family("dst_testnode_last_message_delay_ms", d["last_ms"])
    family("dst_testnode_mesh_size", mesh)
    family("dst_testnode_topic_peers", deg)
    return "".join(out)


@pytest.mark.parametrize("mux", ["yamux", "quic", "mplex"])
def test_writer_against_expected_text(tmp_path, mux):
    d = _crafted()
    cfg = gossipsim.PeerConfig(peers=3, connect_to=1, muxer=mux)
    row = np.array([0, 2, 3, 5], np.uint64)
    mesh = np.array([2, 1, 0], np.uint8)
    sched = (gossipsim.GsPublish * 4)(*[gossipsim.GsPublish(1000 + i, pub, 15000) for i, pub in enumerate([2, 0, 2, 2])])
    path = str(tmp_path / "m")
    gossipsim.write_testnode_metrics(cfg, path, row, mesh, sched, d)
    got = open(path).read()
    assert got == _expected(mux, d, [1, 0, 3], mesh, [2, 1, 2])
    # cumulative buckets, +Inf = _count = completed
    for u in range(3):
        b = [int(x) for x in re.findall(r'_bucket\{muxer="%s",peer_id="pod-%d",le="[^"]+"\} (\d+)' % (mux, u), got)]
        assert len(b) == 13 and b == sorted(b) and b == list(np.cumsum(d["bucket"][u]))
        cnt = int(re.search(r'_ms_count\{muxer="%s",peer_id="pod-%d"\} (\d+)' % (mux, u), got).group(1))
        assert b[-1] == cnt == int(d["completed"][u])
    assert "received_chunks" not in got
    assert got.count('muxer="%s"' % mux) == 3 * (7 + 15)


def test_struct_layout():
    """gs_peer_delay is 136 bytes in the header, in ctypes and in the numpy dtype."""
    assert ctypes.sizeof(gossipsim.GsPeerDelay) == 136 == gossipsim.PEER_DELAY_DTYPE.itemsize
    for name, _ in gossipsim.GsPeerDelay._fields_:
        assert getattr(gossipsim.GsPeerDelay, name).offset == gossipsim.PEER_DELAY_DTYPE.fields[name][1], name
    hdr = open(os.path.join(ROOT, "include", "gossipsim.h")).read()
    assert re.search(r"#define GS_DELAY_BUCKETS 12u", hdr)
    body = re.search(r"typedef struct gs_peer_delay \{(.*?)\} gs_peer_delay;", hdr, re.S).group(1)
    fields = re.findall(r"^\s*(uint64_t|uint32_t)\s+(\w+)(\[GS_DELAY_BUCKETS \+ 1\])?;", body, re.M)
    size = sum((8 if t == "uint64_t" else 4) * (13 if arr else 1) for t, _, arr in fields)
    assert [f[1] for f in fields] == [n for n, _ in gossipsim.GsPeerDelay._fields_] and size == 136
    assert gossipsim.DELAY_BOUNDS_MS == (1, 5, 10, 25, 50, 100, 250, 500, 1000, 2500, 5000, 10000)
    assert re.search(r"#define GS_ABI_VERSION 10u", hdr)


def test_null_arguments(tmp_path):
    L = gossipsim.lib()
    d = _crafted()
    cfg = gossipsim.PeerConfig(peers=3, connect_to=1)
    row = np.array([0, 2, 3, 5], np.uint64)
    mesh = np.array([2, 1, 0], np.uint8)
    sched = (gossipsim.GsPublish * 1)(gossipsim.GsPublish(1000, 0, 15000))
    P, u64, u8 = ctypes.POINTER, ctypes.c_uint64, ctypes.c_uint8
    good = [ctypes.byref(cfg.c), str(tmp_path / "x").encode(), row.ctypes.data_as(P(u64)), mesh.ctypes.data_as(P(u8)),
            sched, 1, d.ctypes.data_as(P(gossipsim.GsPeerDelay))]
    assert L.gs_write_testnode_metrics(*good) == 0
    for k in (0, 1, 2, 3, 4, 6):
        args = list(good)
        args[k] = None
        assert L.gs_write_testnode_metrics(*args) == gossipsim.GS_EINVAL, k
    args = list(good)
    args[4], args[5] = None, 0  # no schedule at all is allowed
    assert L.gs_write_testnode_metrics(*args) == 0
    bad = (gossipsim.GsPublish * 1)(gossipsim.GsPublish(1000, 3, 15000))  # a publisher past the peers
    args = list(good)
    args[4] = bad
    assert L.gs_write_testnode_metrics(*args) == gossipsim.GS_EINVAL
    for fn, extra in (("gs_set_peer_delay", (1,)), ("gs_get_peer_delay", (None,)), ("gs_reset_peer_delay", ()),
                      ("gs_peer_delay_add_lat", (None, 0, None))):
        assert getattr(L, fn)(None, *extra) == gossipsim.GS_EINVAL, fn


def test_integration_md_names_the_entries():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for fn in ("gs_set_peer_delay", "gs_get_peer_delay", "gs_reset_peer_delay", "gs_peer_delay_add_lat",
               "gs_write_testnode_metrics"):
        assert "`%s`" % fn in text, fn
    assert "main.nim:25-78" in text and "main.nim:147-154" in text
