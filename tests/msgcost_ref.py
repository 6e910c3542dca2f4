"""Reference for the per-message cost table (gs_set_message_costs), from the
oracle alone. A helper, not a test.

Per message the oracle runs alone with per-peer traffic, as pubsub_ref.reference does; each
peer's (bytes, packets) of a direction is split into fragment copies, IHAVE and IWANT RPCs with
pubsub_ref._split (which asserts every split: integral, non-negative, control bytes below one
fragment's) and the splits are summed over the peers. Nothing is skipped: an input the split
cannot decide fails here.

FIRST is the one-message run's own stats["frag_deliveries"] (first receipts of a fragment at a
non-publisher: exact with fragments and under churn too), DELIVERED the sum of the peers'
GS_TR_RECEIVED, asserted equal to stats["deliveries"]. The byte sums are the plain sums over peers
of the traffic columns of that message alone.
"""
import numpy as np

import oracle
import pubsub_ref as P

DATA_TX, DATA_RX, FIRST, DUP, IHAVE_TX, IHAVE_RX, IWANT, DELIVERED = range(8)
COLS = 8
# the per-message byte sums, in the order gs_write_message_costs writes them
BYTE_COLS = ("tx_bytes", "rx_bytes", "tx_packets", "rx_packets", "ack_packets", "ack_bytes")
# oracle traffic columns (gossipsim.h GS_TR_*)
TX_CTRL_PKTS, RX_CTRL_PKTS, TX_CTRL_HDR, RX_CTRL_HDR = 8, 9, 10, 11


def reference(p, S, links, sched, mode=0):
    """-> dict(costs=[M, 8] uint64, bytes=[M, 6] uint64 (BYTE_COLS), whole=oracle.simulate's result
    with traffic, stats=[the one-message runs' stats]). sched: (t, pub, size[, frags])."""
    whole = oracle.simulate(p, S, links, mode=mode, sched=sched, traffic=True)
    t, pub, size = (np.asarray(x) for x in sched[:3])
    frags = np.asarray(sched[3]) if len(sched) > 3 else np.zeros(len(t), np.uint32)
    N, M = p.peers, len(t)
    ih = oracle.ctrl_packets(0, p.node, p.muxer)[:2]
    iw = oracle.ctrl_packets(1, p.node, p.muxer)[:2]
    costs = np.zeros((M, COLS), np.int64)
    nbytes = np.zeros((M, len(BYTE_COLS)), np.uint64)
    total = np.zeros((N, oracle.TR_COLS), np.uint64)
    stats = []
    for i in range(M):
        F = int(frags[i]) or p.fragments
        payload = P.frag_payload(p, size[i], F)
        W = oracle.wire_bytes(payload, p.muxer, p.signed_msgs)
        pk = oracle.wire_packets(payload, p.muxer, p.signed_msgs)[0]
        tr = np.zeros((N, oracle.TR_COLS), np.uint64)
        one = (t[i:i + 1], pub[i:i + 1], size[i:i + 1], frags[i:i + 1])
        if p.churn_ppm:
            tc, _, st = oracle.run_churn(p, whole["row_ptr"], whole["col"], whole["snaps"], whole["h_lo"],
                                         whole["stage"], whole["lat"], whole["bw"], whole["bw"], *one, traffic=tr)
        else:
            tc, _, st = oracle.run(p, whole["row_ptr"], whole["col"], whole["mesh"], whole["cnt"], whole["stage"],
                                   whole["lat"], whole["bw"], whole["bw"], *one, traffic=tr)
        np.testing.assert_array_equal(tc[0], whole["t_complete"][i], err_msg="message %d alone differs" % i)
        total += tr
        stats.append(st)
        n, a, x = P._split(tr[:, P.TX_BYTES], tr[:, P.TX_PKTS], W, pk, ih, iw, "message %d tx" % i)
        costs[i, DATA_TX], costs[i, IHAVE_TX], costs[i, IWANT] = n.sum(), a.sum(), x.sum()
        n, a, x = P._split(tr[:, P.RX_BYTES], tr[:, P.RX_PKTS], W, pk, ih, iw, "message %d rx" % i)
        costs[i, DATA_RX], costs[i, IHAVE_RX] = n.sum(), a.sum()
        assert int(x.sum()) == costs[i, IWANT], "message %d: an IWANT was lost" % i
        costs[i, FIRST] = st["frag_deliveries"]
        costs[i, DELIVERED] = int(tr[:, P.TR_RECEIVED].sum())
        assert costs[i, DELIVERED] == st["deliveries"], "message %d: received != deliveries" % i
        costs[i, DUP] = costs[i, DATA_RX] - costs[i, FIRST]
        assert costs[i, DUP] >= 0 and costs[i, DATA_TX] >= costs[i, DATA_RX] and costs[i, IHAVE_TX] >= costs[i, IHAVE_RX]
        s = tr.sum(axis=0)
        assert s[TX_CTRL_PKTS] == s[RX_CTRL_PKTS] and s[TX_CTRL_HDR] == s[RX_CTRL_HDR], "message %d: an ACK was lost" % i
        nbytes[i] = [s[P.TX_BYTES], s[P.RX_BYTES], s[P.TX_PKTS], s[P.RX_PKTS], s[TX_CTRL_PKTS], s[TX_CTRL_HDR]]
    # the messages are independent: their traffic sums to the run's
    np.testing.assert_array_equal(total, whole["traffic"], err_msg="per-message traffic does not sum to the run's")
    return dict(costs=costs.astype(np.uint64), bytes=nbytes, whole=whole, stats=stats)


LINKS = (50, 150, 40, 130)
_REF = {}


def _delay_case():
    """Lazy gossip with a 1500 ms message delay over a 1 s heartbeat: the messages alternate
    between two offset classes, so the run regroups them (class_plan) and the first one has a
    heartbeat at its publish instant."""
    import test_gpu_pubsub_counts as G
    p = oracle.params(peers=300, seed=71, hb_phase_ns=G.PHASE)
    t, pub, size = G._sched(6, 300)
    t = t[0] + np.arange(6, dtype=np.uint64) * np.uint64(1_500_000_000)
    return p, (t, pub, size)


def case(name):
    """-> (params, schedule, reference) of a named case, computed once and shared (never
    modified). The names and parameter sets are tests/test_gpu_pubsub_counts.py's CASES (240000-byte
    messages, five topogen stages, seed 71) and its `overrides`; `n257_m5` and `delay` are the same
    family at another shape."""
    if name not in _REF:
        import test_gpu_pubsub_counts as G
        if name == "overrides":
            p, sched = G._overrides()
        elif name == "delay":
            p, sched = _delay_case()
        elif name == "n257_m5":
            p = oracle.params_for(0, seed=71, peers=257, hb_phase_ns=G.PHASE)
            sched = G._sched(5, 257)
        else:
            p, M, _ = G._params(name)
            sched = G._sched(M, p.peers)
        r = reference(p, 5, LINKS, sched)
        r["costs"].setflags(write=False)
        r["bytes"].setflags(write=False)
        _REF[name] = (p, sched, r)
    return _REF[name]
