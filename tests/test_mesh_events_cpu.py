"""Host side of the mesh event counts (gs_set_mesh_events), no GPU: the
reference of tests/mesh_ref.py pinned to the oracle with its identities and the conditions that
make the cases worth running, both host writers on hand-made arrays against text built here,
NULL and bad-size arguments, the header's enums and the INTEGRATION.md / Rust entries."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gossipsim
import oracle
import mesh_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES, SUMS, ref_of = R.CASES, R.SUMS, R.ref_of


@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_pinned_identities_and_sums(name):
    r = ref_of(name)  # (asserts every epoch's mesh / the final mesh and epoch count against the oracle)
    epochs, sums = CASES[name][3:]
    assert r["epochs"] == epochs and r["series"].shape == (epochs + 1, R.SERIES_COLS)
    assert r["events"].shape == (CASES[name][0]["peers"], R.EVENT_COLS)
    R.check_identities(r["events"], r["series"])
    tot = r["series"].astype(np.int64).sum(axis=0)
    assert tuple(int(tot[k]) for k in SUMS) == sums
    # non-trivial: every kind of event occurs
    for k in (R.GRAFTS, R.REJECTS, R.PRUNES, R.ADDS, R.DELS):
        assert tot[k] > 0, k
    churn = CASES[name][0].get("churn_ppm", 0) > 0
    assert (tot[R.DROPS] > 0) == churn
    if not churn:
        assert not r["events"][:, R.ME_MESH_DROP].any()
        assert (r["series"][:, R.ONLINE] == CASES[name][0]["peers"]).all()
    else:
        assert (r["series"][1:, R.ONLINE] < CASES[name][0]["peers"]).any()


def test_case_shapes():
    """C jumps over quiescent epochs (PRUNEs still fall at epoch 62); F and H have rows wider
    than 64 entries; without the subscription exchange row 0 is the empty mesh."""
    c = ref_of("C")
    assert len(c["stepped"]) == 11 < c["epochs"] + 1 == 65
    assert c["series"][62, R.PRUNES] > 0 and 62 in c["stepped"] and 30 not in c["stepped"]
    np.testing.assert_array_equal(c["series"][30, :R.LINKS + 1], c["series"][29, :R.LINKS + 1])
    assert not c["series"][30, R.GRAFTS:].any()
    assert ref_of("F")["max_degree"] == ref_of("H")["max_degree"] == 87 > 64
    for name in ("A", "D"):
        assert ref_of(name)["max_degree"] <= 64
    b = ref_of("B")
    assert 0 not in b["stepped"]
    assert b["series"][0].tolist() == [257, 257] + [0] * 10
    assert ref_of("A")["series"][0, R.GRAFTS] > 0


# (family, type, help of go-test-node/metrics.go, topic label)
FAMILIES = [
    ("libp2p_pubsub_broadcast_graft_total", "counter", "pubsub broadcast graft", True),
    ("libp2p_pubsub_received_graft_total", "counter", "pubsub received graft", True),
    ("libp2p_pubsub_broadcast_prune_total", "counter", "pubsub broadcast prune", True),
    ("libp2p_pubsub_received_prune_total", "counter", "pubsub received prune", True),
    ("libp2p_pubsub_broadcast_subscriptions_total", "counter", "pubsub broadcast subscriptions", True),
    ("libp2p_pubsub_received_subscriptions_total", "counter", "pubsub received subscriptions", True),
    ("libp2p_gossipsub_peers_per_topic_mesh", "gauge", "gossipsub peers per topic in mesh", True),
    ("libp2p_gossipsub_low_peers_topics", "gauge", "number of topics in mesh with at least one but below dlow peers",
     False),
    ("libp2p_gossipsub_healthy_peers_topics", "gauge", "number of topics in mesh with at least dlow peers", False),
    ("libp2p_gossipsub_no_peers_topics", "gauge", "number of topics in mesh with no peers", False),
]


def _crafted():
    ev = np.zeros((4, R.EVENT_COLS), np.uint64)
    ev[0] = [7, 6, 5, 4, 3, 2, 1]
    ev[1] = [2 ** 40 + 5, 0, 9, 1, 0, 0, 12]
    ev[3] = [1, 2, 3, 4, 5, 6, 7]
    row = np.array([0, 3, 3, 10, 22], np.uint64)
    mc = np.array([3, 0, 4, 9], np.uint8)  # d_lo = 4: low, none, healthy, healthy
    return row, mc, ev


def _expected_metrics(row, mc, ev, d_lo):
    deg = np.diff(row.astype(np.int64))
    values = [ev[:, R.ME_GRAFT_TX], ev[:, R.ME_GRAFT_RX], ev[:, R.ME_PRUNE_TX], ev[:, R.ME_PRUNE_RX], deg, deg, mc,
              [int(0 < m < d_lo) for m in mc], [int(m >= d_lo and m > 0) for m in mc], [int(m == 0) for m in mc]]
    out = []
    for (name, typ, text, topic), val in zip(FAMILIES, values):
        out.append("# HELP %s %s\n# TYPE %s %s\n" % (name, text, name, typ))
        for u in range(len(mc)):
            out.append('%s{%speer_id="pod-%d"} %d\n' % (name, 'topic="test",' if topic else "", u, int(val[u])))
    return "".join(out)


@pytest.mark.parametrize("d_lo", [4, 5])
def test_metrics_writer_against_expected_text(tmp_path, d_lo):
    row, mc, ev = _crafted()
    cfg = gossipsim.PeerConfig(peers=4, connect_to=1, d_lo=d_lo)
    path = str(tmp_path / "m")
    gossipsim.write_mesh_metrics(cfg, path, row, mc, ev)
    got = open(path).read()
    assert got == _expected_metrics(row, mc, ev, d_lo)
    assert got.count('topic="test"') == 7 * 4 and got.count("# TYPE") == 10
    assert 'libp2p_pubsub_broadcast_graft_total{topic="test",peer_id="pod-1"} %d\n' % (2 ** 40 + 5) in got
    assert 'libp2p_gossipsub_low_peers_topics{peer_id="pod-0"} 1\n' in got
    assert 'libp2p_gossipsub_healthy_peers_topics{peer_id="pod-2"} %d\n' % (1 if d_lo == 4 else 0) in got
    with pytest.raises(gossipsim.GossipSimError):
        gossipsim.write_mesh_metrics(cfg, path, row, mc, np.zeros((4, 6), np.uint64))
    with pytest.raises(gossipsim.GossipSimError):
        gossipsim.write_mesh_metrics(cfg, path, row[:-1], mc, ev)


def test_series_writer_against_expected_text(tmp_path):
    se = np.arange(3 * R.SERIES_COLS, dtype=np.uint64).reshape(3, R.SERIES_COLS)
    se[1, R.LINKS] = 2 ** 40 + 5
    path = str(tmp_path / "s.csv")
    gossipsim.write_mesh_series(path, se)
    want = "epoch,online,no_peers,low,healthy,over,links,grafts,rejects,prunes,drops,adds,dels\n"
    for h in range(3):
        want += ",".join([str(h)] + [str(int(x)) for x in se[h]]) + "\n"
    assert open(path).read() == want
    assert ",%d," % (2 ** 40 + 5) in want
    assert want.splitlines()[0].split(",")[1:] == list(gossipsim.MESH_SERIES_COLS)
    with pytest.raises(gossipsim.GossipSimError):
        gossipsim.write_mesh_series(path, np.zeros((3, 11), np.uint64))
    gossipsim.write_mesh_series(path, np.zeros((0, R.SERIES_COLS), np.uint64))  # no rows: the header alone
    assert open(path).read() == want.splitlines()[0] + "\n"


def test_null_and_bad_arguments(tmp_path):
    L = gossipsim.lib()
    row, mc, ev = _crafted()
    cfg = gossipsim.PeerConfig(peers=4, connect_to=1)
    pu64, pu8 = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint8)
    good = [ctypes.byref(cfg.c), str(tmp_path / "x").encode(), 4, row.ctypes.data_as(pu64), mc.ctypes.data_as(pu8),
            ev.ctypes.data_as(pu64)]
    assert L.gs_write_mesh_metrics(*good) == 0
    for k in (0, 1, 3, 4, 5):
        args = list(good)
        args[k] = None
        assert L.gs_write_mesh_metrics(*args) == gossipsim.GS_EINVAL, k
    args = list(good)
    args[1] = str(tmp_path / "no_such_dir" / "x").encode()
    assert L.gs_write_mesh_metrics(*args) == gossipsim.GS_EINVAL
    se = np.zeros((2, R.SERIES_COLS), np.uint64)
    assert L.gs_write_mesh_series(str(tmp_path / "s").encode(), se.ctypes.data_as(pu64), 2) == 0
    assert L.gs_write_mesh_series(None, se.ctypes.data_as(pu64), 2) == gossipsim.GS_EINVAL
    assert L.gs_write_mesh_series(str(tmp_path / "s").encode(), None, 2) == gossipsim.GS_EINVAL
    assert L.gs_write_mesh_series(args[1], se.ctypes.data_as(pu64), 2) == gossipsim.GS_EINVAL
    rows = ctypes.c_uint32(0)
    for fn, extra in (("gs_set_mesh_events", (1,)), ("gs_get_mesh_events", (ev.ctypes.data_as(pu64),)),
                      ("gs_mesh_series_rows", (ctypes.byref(rows),)),
                      ("gs_get_mesh_series", (se.ctypes.data_as(pu64), 2))):
        assert getattr(L, fn)(None, *extra) == gossipsim.GS_EINVAL, fn


def test_header_enums_and_bindings():
    hdr = open(os.path.join(ROOT, "include", "gossipsim.h")).read()
    want = dict(GS_ME_GRAFT_TX=0, GS_ME_GRAFT_RX=1, GS_ME_PRUNE_TX=2, GS_ME_PRUNE_RX=3, GS_ME_MESH_ADD=4,
                GS_ME_MESH_DEL=5, GS_ME_MESH_DROP=6, GS_MESH_EVENT_COLS=7, GS_MS_ONLINE=0, GS_MS_NO_PEERS=1,
                GS_MS_LOW=2, GS_MS_HEALTHY=3, GS_MS_OVER=4, GS_MS_LINKS=5, GS_MS_GRAFTS=6, GS_MS_REJECTS=7,
                GS_MS_PRUNES=8, GS_MS_DROPS=9, GS_MS_ADDS=10, GS_MS_DELS=11, GS_MESH_SERIES_COLS=12)
    for name, val in want.items():
        m = re.search(r"\b%s = (\d+)" % name, hdr)
        assert m and int(m.group(1)) == val, name
    assert re.search(r"#define GS_ABI_VERSION 10u", hdr)
    assert len(gossipsim.MESH_EVENT_COLS) == R.EVENT_COLS == 7
    assert len(gossipsim.MESH_SERIES_COLS) == R.SERIES_COLS == 12
    for name, val in want.items():  # the Python name lists are the header's order
        if name.startswith("GS_ME_") and name[6:].endswith(("_TX", "_RX")):  # direction first, as TRAFFIC_COLS
            kind, way = name[6:].lower().split("_")
            assert gossipsim.MESH_EVENT_COLS[val] == "%s_%s" % (way, kind), name
        elif name.startswith("GS_ME_"):
            assert gossipsim.MESH_EVENT_COLS[val] == name[6:].lower(), name
        elif name.startswith("GS_MS_"):
            assert gossipsim.MESH_SERIES_COLS[val] == name[6:].lower(), name
    assert gossipsim.MESH_EVENT_COLS.index("tx_prune") == R.ME_PRUNE_TX
    assert gossipsim.MESH_EVENT_COLS.index("mesh_drop") == R.ME_MESH_DROP
    assert gossipsim.MESH_SERIES_COLS.index("rejects") == R.REJECTS
    assert gossipsim.MESH_SERIES_COLS.index("dels") == R.DELS
    for fn in FUNCTIONS:
        assert re.search(r"gs_status %s\(" % fn, hdr), fn
        assert fn in gossipsim.SIGNATURES, fn
    for method in ("set_mesh_events", "mesh_events", "mesh_series", "write_mesh_metrics", "write_mesh_series"):
        assert callable(getattr(gossipsim.Simulator, method)), method


FUNCTIONS = ("gs_set_mesh_events", "gs_get_mesh_events", "gs_mesh_series_rows", "gs_get_mesh_series",
             "gs_write_mesh_metrics", "gs_write_mesh_series")


def test_integration_md_and_rust_name_the_entries():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    rs = open(os.path.join(ROOT, "rust", "gossipsim-sys", "src", "lib.rs")).read()
    for fn in FUNCTIONS:
        assert "`%s`" % fn in text, fn
        assert re.search(r"pub fn %s\(" % fn, rs), fn
    assert "metrics.go:164-190" in text and "metrics.go:224-258" in text
    assert re.search(r"pub const GS_MESH_EVENT_COLS: usize = 7;", rs)
    assert re.search(r"pub const GS_MESH_SERIES_COLS: usize = 12;", rs)
