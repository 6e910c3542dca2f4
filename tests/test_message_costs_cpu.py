"""Host side of the per-message cost table (no GPU): the header's enum and
functions with the ABI still 10, the Rust and INTEGRATION.md entries, the reference of
tests/msgcost_ref.py on the oracle alone, and gs_write_message_costs fed the reference counts
against the oracle's byte and packet sums per message."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gossipsim
import msgcost_ref as R
import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FNS = ("gs_set_message_costs", "gs_message_costs_rows", "gs_get_message_costs", "gs_write_message_costs")
HEADER = ["#msg", "t_pub_ns", "publisher", "msg_size", "chunks"] + list(gossipsim.MESSAGE_COST_COLS) + list(R.BYTE_COLS)


def test_header_enum_and_functions():
    hdr = open(os.path.join(ROOT, "include", "gossipsim.h")).read()
    want = dict(GS_MC_DATA_TX=0, GS_MC_DATA_RX=1, GS_MC_FIRST=2, GS_MC_DUP=3, GS_MC_IHAVE_TX=4, GS_MC_IHAVE_RX=5,
                GS_MC_IWANT=6, GS_MC_DELIVERED=7, GS_MC_COLS=8)
    for name, val in want.items():
        m = re.search(r"\b%s = (\d+)" % name, hdr)
        assert m and int(m.group(1)) == val, name
    assert re.search(r"#define GS_ABI_VERSION 10u", hdr) and gossipsim.ABI_VERSION == 10
    for fn in FNS:
        assert re.search(r"gs_status %s\(" % fn, hdr), fn
    assert gossipsim.MESSAGE_COST_COLS == ("data_tx", "data_rx", "first", "dup", "ihave_tx", "ihave_rx", "iwant",
                                           "delivered")
    assert len(gossipsim.MESSAGE_COST_COLS) == R.COLS == 8
    assert gossipsim.MESSAGE_COST_COLS.index("iwant") == R.IWANT
    assert gossipsim.MESSAGE_COST_COLS.index("delivered") == R.DELIVERED


def test_rust_and_integration_name_the_entries():
    rs = open(os.path.join(ROOT, "rust", "gossipsim-sys", "src", "lib.rs")).read()
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for fn in FNS:
        assert re.search(r"pub fn %s\(" % fn, rs), fn
        assert "`%s`" % fn in text, fn
    assert re.search(r"pub const GS_MC_COLS: usize = 8;", rs)


def test_reference_identities_on_the_oracle():
    """Frozen mesh, one fragment: nothing is lost, a message's first receipts are its deliveries,
    and the rows sum to the whole run's own counters."""
    p, sched, r = R.case("rust")
    c, st = r["costs"].astype(np.int64), r["whole"]["stats"]
    np.testing.assert_array_equal(c[:, R.DATA_TX], c[:, R.DATA_RX])
    np.testing.assert_array_equal(c[:, R.IHAVE_TX], c[:, R.IHAVE_RX])
    np.testing.assert_array_equal(c[:, R.FIRST], c[:, R.DELIVERED])
    assert (c[:, R.DELIVERED] == p.peers - 1).all()
    tot = c.sum(axis=0)
    assert tot[R.DATA_TX] == st["relaxations"] and tot[R.FIRST] == st["frag_deliveries"]
    assert tot[R.IWANT] == st["gossip_iwant"] > 0 and tot[R.DELIVERED] == st["deliveries"]


def test_reference_under_churn_loses_copies():
    for name in ("churn_f1", "churn_f2"):
        _, _, r = R.case(name)
        c = r["costs"].astype(np.int64)
        assert (c[:, R.DATA_TX] > c[:, R.DATA_RX]).any(), name
    c2 = R.case("churn_f2")[2]["costs"].astype(np.int64)
    assert (c2[:, R.FIRST] > 2 * c2[:, R.DELIVERED]).any()  # partial receipts exist


def _cfg(p):
    return gossipsim.PeerConfig(**{n: getattr(p, n) for n, _ in oracle.OrParams._fields_})


def _parse(path):
    lines = open(str(path)).read().split("\n")
    assert lines[-1] == "" and lines[0].split("\t") == HEADER
    return np.array([[int(x) for x in ln.split("\t")] for ln in lines[1:-1]], dtype=object).reshape(-1, len(HEADER))


@pytest.mark.parametrize("name", ["rust", "go_f1", "go_f2", "nim", "quic", "overrides", "churn_f2"])
def test_writer_reproduces_the_oracle_s_bytes(tmp_path, name):
    """The rust, go and nim presets on yamux, quic (unsigned), per-message chunk counts with a size
    change, and lost copies: the wire cost derived from the counts is the sum over peers of the
    oracle's per-peer traffic of that message alone."""
    p, sched, r = R.case(name)
    path = tmp_path / "costs.tsv"
    gossipsim.write_message_costs(_cfg(p), path, sched, r["costs"])
    rows = _parse(path)
    M = len(sched[0])
    assert rows.shape[0] == M
    frags = sched[3] if len(sched) > 3 else np.zeros(M, np.uint32)
    for i in range(M):
        assert list(rows[i, :5]) == [i, int(sched[0][i]), int(sched[1][i]), int(sched[2][i]), int(frags[i]) or p.fragments]
        assert list(rows[i, 5:13]) == [int(x) for x in r["costs"][i]], "message %d counts" % i
        assert list(rows[i, 13:]) == [int(x) for x in r["bytes"][i]], "message %d bytes" % i
    if name == "quic":
        assert p.muxer == 1 and not p.signed_msgs
    if name == "overrides":
        assert len(set(rows[:, 4])) == 3 and len(set(rows[:, 3])) == 2


def test_writer_arguments(tmp_path):
    L = gossipsim.lib()
    p, sched, r = R.case("rust")
    cfg = _cfg(p)
    arr = gossipsim.Simulator._schedule(None, sched)
    costs = np.ascontiguousarray(r["costs"])
    good = [ctypes.byref(cfg.c), str(tmp_path / "x").encode(), arr, len(arr),
            costs.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))]
    assert L.gs_write_message_costs(*good) == 0
    for k in (0, 1, 2, 4):
        args = list(good)
        args[k] = None
        assert L.gs_write_message_costs(*args) == gossipsim.GS_EINVAL, k
    args = list(good)
    args[1] = str(tmp_path / "no_such_dir" / "x").encode()
    assert L.gs_write_message_costs(*args) == gossipsim.GS_EINVAL
    # no message at all: the header line alone, and no array is read
    assert L.gs_write_message_costs(good[0], good[1], None, 0, None) == 0
    assert open(str(tmp_path / "x")).read() == "\t".join(HEADER) + "\n"
    # a message no node can publish (the rust node needs 8 bytes per fragment)
    short = (sched[0][:1], sched[1][:1], np.array([7]))
    with pytest.raises(gossipsim.GossipSimError, match="GS_EINVAL"):
        gossipsim.write_message_costs(cfg, tmp_path / "y", short, r["costs"][:1])
    with pytest.raises(gossipsim.GossipSimError, match="GS_EINVAL"):
        gossipsim.write_message_costs(cfg, tmp_path / "y", sched, r["costs"][:, :7])
    with pytest.raises(gossipsim.GossipSimError, match="GS_EINVAL"):
        gossipsim.write_message_costs(cfg, tmp_path / "y", sched, r["costs"][:2])
    # the context functions: a null context, and the switch's states need no device
    assert L.gs_set_message_costs(None, 1) == gossipsim.GS_EINVAL
    assert L.gs_message_costs_rows(None, None) == gossipsim.GS_EINVAL
    assert L.gs_get_message_costs(None, None, 0) == gossipsim.GS_EINVAL
