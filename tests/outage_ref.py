"""Reference of a caller's outages (gs_set_outages, DESIGN.md §2.8 "A caller's outages"), in
numpy and plain Python: the offline table of a list of intervals, the maximal intervals of a
table, and a restatement of the time-to-epoch rule of gs_outage_epochs."""
import numpy as np

FOREVER = 0xFFFFFFFF  # GS_OUTAGE_FOREVER
T_NEVER = 0xFFFFFFFFFFFFFFFF


def table(peers, intervals, h_lo, h_hi):
    """bool [h_hi - h_lo + 1, peers]: peer u is offline in epoch h iff an interval (u, a, b) has
    a <= h < b (b == FOREVER: a <= h); epoch 0 has nobody offline."""
    t = np.zeros((h_hi - h_lo + 1, peers), bool)
    for u, a, b in intervals:
        a, b = int(a), int(b)
        lo = max(a, h_lo, 1)
        hi = h_hi + 1 if b == FOREVER else min(b, h_hi + 1)
        if lo < hi:
            t[lo - h_lo:hi - h_lo, int(u)] = True
    return t


def maximal_intervals(tab, h_lo=0):
    """The maximal runs of True per peer of a table whose row k is epoch h_lo + k, as a list of
    (peer, h_from, h_to) in peer order; a run that reaches the last row ends there (h_to = last + 1)."""
    out = []
    E, N = tab.shape
    for u in range(N):
        col = np.concatenate(([False], tab[:, u], [False]))
        d = np.diff(col.astype(np.int8))
        for a, b in zip(np.flatnonzero(d == 1), np.flatnonzero(d == -1)):
            out.append((u, h_lo + int(a), h_lo + int(b)))
    return out


def epochs_of(heartbeat_ns, hb_phase_ns, t_down, t_up):
    """The epochs h >= 1 with t_down <= hb_phase + h * heartbeat < t_up as (h_from, h_to), or None
    when there is none; t_up == T_NEVER: h_to = FOREVER. Found by counting heartbeats one by one
    from a lower bound (no ceiling division: another route than the library's)."""
    hb, ph = int(heartbeat_ns), int(hb_phase_ns)
    t_down, t_up = int(t_down), int(t_up)
    h = max(1, (t_down - ph) // hb - 1) if t_down > ph else 1
    while ph + h * hb < t_down:
        h += 1
    if t_up != T_NEVER and ph + h * hb >= t_up:
        return None
    if t_up == T_NEVER:
        return h, FOREVER
    e = max(h, (t_up - ph) // hb - 1)
    while ph + e * hb < t_up:
        e += 1
    return h, e
