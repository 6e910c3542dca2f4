"""Per-link first deliveries without a GPU: the reference of the GPU tests proven
against the oracle, the host-only writer byte for byte, and the transposed sum."""
import numpy as np
import pytest

import gossipsim
import link_ref as R


def test_case_constants_are_the_package_s():
    assert R.T0 == gossipsim.T0_NS
    assert gossipsim.LINK_DELIVERY_COLS == ("publish", "mesh", "gossip")
    assert (R.PUBLISH, R.MESH, R.GOSSIP, R.COLS) == (0, 1, 2, len(gossipsim.LINK_DELIVERY_COLS))


def _consistent(p, sched, g, r):
    """What a proven replay implies for its counts: one entry per completed (peer, message), none
    GOSSIP, and the given side the transposed sum."""
    M = len(sched[0])
    done = int((g["t_complete"] != R.UND).sum()) - M  # (the publishers complete without a receipt)
    assert int(r["edge"].sum()) == done == g["stats"]["frag_deliveries"]
    assert not r["edge"][:, R.GOSSIP].any()
    np.testing.assert_array_equal(r["given"], R.transpose_sum(g["col"], r["edge"], p.peers))


@pytest.mark.parametrize("name", sorted(R.BUILT))
def test_replay_equals_the_oracle_on_built_graphs(name):
    """R.reference asserts t_complete and hops of every peer and message against the oracle."""
    p, sched, g, r = R.built(name)
    _consistent(p, sched, g, r)
    if name == "no_flood":  # the publisher sends to its mesh only, and that still counts as PUBLISH
        pubs = sched[1]
        assert int(r["edge"][:, R.PUBLISH].sum()) == int(sum(g["cnt"][int(x)] for x in pubs))
    if name == "quiet":  # lazy gossip on, and it changed nothing
        np.testing.assert_array_equal(r["edge"], R.built("rust")[3]["edge"])


def test_replay_equals_the_oracle_on_the_hub_graph():
    p, sched, g, r, _ = R.hub()
    _consistent(p, sched, g, r)
    deg = np.diff(g["row_ptr"].astype(np.int64))
    assert deg.max() == deg[0] == 202 and sched[1][0] == 0  # the hub publishes the first message
    assert int(r["given"][0, R.PUBLISH]) > 64
    hub_row = r["edge"][:202].sum(axis=1)  # and receives the others: over an entry beyond a wave's 64 too
    assert hub_row[64:].any() and hub_row[:64].any()


def test_replay_equals_the_oracle_under_an_empty_mesh():
    p, sched, g, r = R.empty_mesh()
    _consistent(p, sched, g, r)
    assert not r["edge"][:, R.MESH].any() and r["edge"][:, R.PUBLISH].any()
    assert (g["t_complete"] == R.UND).any()  # nothing is forwarded


def test_replay_refuses_a_case_with_iwant_answers():
    p, sched, g = R.invariant("gossip")
    assert g["stats"]["gossip_iwant"] > 0
    with pytest.raises(AssertionError, match="not an exact case"):
        R.reference(p, g, sched)


def test_the_gossip_case_has_an_iwant_answer_that_wins():
    """Chosen here, on the CPU: lazy gossip changes some arrival, and in at least one message the
    first change is provably an answer of a non-publisher (GOSSIP, not PUBLISH)."""
    p, sched, g = R.invariant("gossip")
    assert all((int(t) - p.hb_phase_ns) % p.heartbeat_ns == 0 for t in sched[0])  # a heartbeat at every publish
    changed, proven = R.gossip_winners()
    assert changed > 0 and proven > 0 and g["stats"]["gossip_iwant"] > 0


# a hand-made graph of 5 peers: peer 1 has no connection, peer 2 all three kinds, peer 4 the last row
ROW = np.array([0, 2, 2, 5, 7, 9], np.uint64)
COL = np.array([2, 3, 0, 3, 4, 0, 2, 2, 3], np.uint32)
COUNTS = np.array([[0, 0, 0], [0, 7, 0],
                   [1, 2, 3], [0, 0, 0], [0, 0, 18446744073709551615],
                   [4, 0, 0], [0, 0, 0],
                   [0, 5, 0], [6, 0, 1]], np.uint64)
TEXT = "0 3 0 7 0\n2 0 1 2 3\n2 4 0 0 18446744073709551615\n3 0 4 0 0\n4 2 0 5 0\n4 3 6 0 1\n"


def test_writer_byte_for_byte(tmp_path):
    """One line per entry with a non-zero count, in CSR order, plain integers."""
    path = tmp_path / "links.txt"
    gossipsim.write_link_deliveries(path, ROW, COL, COUNTS)
    assert path.read_bytes() == TEXT.encode()
    gossipsim.write_link_deliveries(path, ROW, COL, np.zeros_like(COUNTS))
    assert path.read_bytes() == b""
    lib = gossipsim.lib()
    assert lib.gs_write_link_deliveries(None, 5, None, None, None) == gossipsim.GS_EINVAL
    with pytest.raises(gossipsim.GossipSimError, match="GS_EINVAL"):
        gossipsim.write_link_deliveries(path, ROW, COL, COUNTS[:, :2])
    with pytest.raises(gossipsim.GossipSimError, match="GS_EINVAL"):
        gossipsim.write_link_deliveries(tmp_path / "no" / "dir", ROW, COL, COUNTS)


def test_writer_of_a_graph_without_entries(tmp_path):
    path = tmp_path / "none.txt"
    gossipsim.write_link_deliveries(path, np.zeros(3, np.uint64), np.zeros(0, np.uint32), np.zeros((0, 3), np.uint64))
    assert path.read_bytes() == b""


def test_transposed_sum_of_a_hand_made_array():
    small = COUNTS.copy()
    small[4, 2] = 9
    # senders: peer 0 <- entries 2, 5; peer 2 <- 0, 6, 7; peer 3 <- 1, 3, 8; peer 4 <- 4
    got = R.transpose_sum(COL, small, 5)
    np.testing.assert_array_equal(got, [[5, 2, 3], [0, 0, 0], [0, 5, 0], [6, 7, 1], [0, 0, 9]])
    assert int(got.sum()) == int(small.sum())
