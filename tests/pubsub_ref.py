"""Reference for the per-peer pubsub event counts (gs_set_pubsub_counts), from the oracle's
per-peer traffic alone. A helper, not a test.

The oracle accounts bytes and packets per peer (traffic=True), not events. Run on ONE message
with a large message, a peer's (bytes, packets) pair of one direction splits uniquely:
    n_data = bytes // W                                    (control bytes stay below W)
    ihw * a + iww * x  = bytes   - W  * n_data
    ihpk * a + iwpk * x = packets - pk * n_data            (a IHAVE RPCs, x IWANT RPCs)
with W, pk one fragment copy on the wire and (ihw, ihpk), (iww, iwpk) one IHAVE / IWANT RPC.
Messages are independent given the mesh of each epoch, so the per-message
splits sum to the run's counts. Every split is asserted integral, non-negative and with its
control bytes below W: an input the method cannot decide fails here and is never skipped.

First receipts: with one fragment a peer's first receipts are its delivered messages
(GS_TR_RECEIVED). With F fragments on a frozen mesh where every peer completes they are F
per delivered message. Otherwise (churn with fragments: partial receipts exist) only the
total, stats["frag_deliveries"], is a reference: `exact` says which holds.
"""
import numpy as np

import oracle

MSG_TX, MSG_RX, FIRST, DUP, IHAVE_TX, IHAVE_RX, IWANT_TX, IWANT_RX = range(8)
COLS = 8
# oracle traffic columns (gossipsim.h GS_TR_*)
TX_BYTES, RX_BYTES, TX_PKTS, RX_PKTS, TR_RECEIVED = 0, 1, 2, 3, 6
UND = np.iinfo(np.uint64).max


def frag_payload(p, msg_size, F):
    """The data field of one fragment: msg_size / F, the go node 8 bytes more."""
    return int(msg_size) // int(F) + (8 if p.node == 1 else 0)


def _split(nbytes, npkts, W, pk, ih, iw, what):
    """[N] bytes and packets -> (data copies, IHAVE RPCs, IWANT RPCs), each [N] int64."""
    b = nbytes.astype(np.int64)
    q = npkts.astype(np.int64)
    n = b // W
    rb, rp = b - W * n, q - pk * n
    det = ih[0] * iw[1] - iw[0] * ih[1]
    assert det != 0, "%s: IHAVE and IWANT RPCs are not told apart by (bytes, packets)" % what
    a_num, x_num = rb * iw[1] - iw[0] * rp, ih[0] * rp - rb * ih[1]
    assert not (a_num % det).any() and not (x_num % det).any(), "%s: the split is not integral" % what
    a, x = a_num // det, x_num // det
    assert (a >= 0).all() and (x >= 0).all() and (rp >= 0).all(), "%s: a negative count" % what
    assert (ih[0] * a + iw[0] * x < W).all(), "%s: control bytes reach one fragment's %d wire bytes" % (what, W)
    assert (W * n + ih[0] * a + iw[0] * x == b).all() and (pk * n + ih[1] * a + iw[1] * x == q).all()
    return n, a, x


def reference(p, S, links, sched, mode=0):
    """-> dict(counts=[N, 8] uint64, exact=bool, whole=oracle.simulate's result with traffic).
    sched: (t, pub, size[, frags]). FIRST and DUP are per-peer exact only where `exact`."""
    whole = oracle.simulate(p, S, links, mode=mode, sched=sched, traffic=True)
    t, pub, size = (np.asarray(x) for x in sched[:3])
    frags = np.asarray(sched[3]) if len(sched) > 3 else np.zeros(len(t), np.uint32)
    N, M = p.peers, len(t)
    ih = oracle.ctrl_packets(0, p.node, p.muxer)[:2]
    iw = oracle.ctrl_packets(1, p.node, p.muxer)[:2]
    counts = np.zeros((N, COLS), np.int64)
    total = np.zeros((N, oracle.TR_COLS), np.uint64)
    exact = True
    for i in range(M):
        F = int(frags[i]) or p.fragments
        payload = frag_payload(p, size[i], F)
        W = oracle.wire_bytes(payload, p.muxer, p.signed_msgs)
        pk = oracle.wire_packets(payload, p.muxer, p.signed_msgs)[0]
        tr = np.zeros((N, oracle.TR_COLS), np.uint64)
        one = (t[i:i + 1], pub[i:i + 1], size[i:i + 1], frags[i:i + 1])
        if p.churn_ppm:
            tc, _, _ = oracle.run_churn(p, whole["row_ptr"], whole["col"], whole["snaps"], whole["h_lo"],
                                        whole["stage"], whole["lat"], whole["bw"], whole["bw"], *one, traffic=tr)
        else:
            tc, _, _ = oracle.run(p, whole["row_ptr"], whole["col"], whole["mesh"], whole["cnt"], whole["stage"],
                                  whole["lat"], whole["bw"], whole["bw"], *one, traffic=tr)
        np.testing.assert_array_equal(tc[0], whole["t_complete"][i], err_msg="message %d alone differs" % i)
        total += tr
        n, a, x = _split(tr[:, TX_BYTES], tr[:, TX_PKTS], W, pk, ih, iw, "message %d tx" % i)
        counts[:, MSG_TX] += n
        counts[:, IHAVE_TX] += a
        counts[:, IWANT_TX] += x
        n, a, x = _split(tr[:, RX_BYTES], tr[:, RX_PKTS], W, pk, ih, iw, "message %d rx" % i)
        counts[:, MSG_RX] += n
        counts[:, IHAVE_RX] += a
        counts[:, IWANT_RX] += x
        counts[:, FIRST] += F * tr[:, TR_RECEIVED].astype(np.int64)
        if F > 1 and p.churn_ppm:  # partial receipts exist: F per delivered message is a lower bound
            exact = False
        elif F > 1:  # frozen mesh: nobody holds only a part of the message
            assert (tc[0][np.arange(N) != pub[i]] != UND).all(), "message %d: a peer did not complete" % i
    # the messages are independent: their traffic sums to the run's
    np.testing.assert_array_equal(total, whole["traffic"], err_msg="per-message traffic does not sum to the run's")
    if exact:
        counts[:, DUP] = counts[:, MSG_RX] - counts[:, FIRST]
        assert (counts[:, DUP] >= 0).all()
    else:  # (no per-peer reference: the columns are left zero)
        counts[:, FIRST] = 0
    return dict(counts=counts.astype(np.uint64), exact=exact, whole=whole)
