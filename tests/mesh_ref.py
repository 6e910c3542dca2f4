"""Reference of the mesh event counts and the per-epoch mesh health (gs_set_mesh_events,
DESIGN.md §2.15): a pure-Python restatement of the heartbeat epoch of DESIGN.md §2.3 with the
disconnect of §2.8 (oracle/gs_oracle.c mesh_epoch and the converge loop with its wake jump)
that also counts what the oracle throws away.

It is a reference only after it reproduced the oracle, and reference() asserts that itself:
under churn the mesh, its size and the offline set of every epoch and peer against
oracle.mesh_churn(..., 0, H); on a frozen mesh the final mesh and the epoch count against
oracle.mesh_converge. The random keys are the oracle's (oracle.rng, purposes 3, 4, 5), the
offline draws oracle.offline, the graph oracle.build_topology, the links oracle.topogen_links;
the stage of a peer is u mod S.

Columns (gossipsim.h GS_ME_* / GS_MS_*). An entry e = (u -> w) is a CSR entry of row u."""
import numpy as np

import oracle

ME_GRAFT_TX, ME_GRAFT_RX, ME_PRUNE_TX, ME_PRUNE_RX, ME_MESH_ADD, ME_MESH_DEL, ME_MESH_DROP = range(7)
EVENT_COLS = 7
ONLINE, NO_PEERS, LOW, HEALTHY, OVER, LINKS, GRAFTS, REJECTS, PRUNES, DROPS, ADDS, DELS = range(12)
SERIES_COLS = 12
P_GRAFT, P_PRUNE, P_OUT_GRAFT = 3, 4, 5
BIT_OUT = 1
HS_RTTS_DEFAULT = 3


class _Mesh:
    def __init__(self, p, stages, links):
        self.p = p
        N = self.N = p.peers
        lat, _ = oracle.topogen_links(stages, *links)
        self.lat_np = lat
        self.lat = [[int(x) for x in r] for r in lat]
        self.stage_np = (np.arange(N) % stages).astype(np.uint8)
        self.stage = [int(s) for s in self.stage_np]
        self.row_ptr, self.col_np, self.flags0 = oracle.build_topology(p)
        self.row = [int(x) for x in self.row_ptr]
        self.col = [int(x) for x in self.col_np]
        self.out = [bool(f & BIT_OUT) for f in self.flags0]
        nnz = len(self.col)
        pos = {}
        for u in range(N):
            for e in range(self.row[u], self.row[u + 1]):
                pos[(u, self.col[e])] = e
        self.src = [0] * nnz
        for u in range(N):
            for e in range(self.row[u], self.row[u + 1]):
                self.src[e] = u
        self.rev = [pos[(self.col[e], self.src[e])] for e in range(nnz)]
        self.mesh = [False] * nnz
        self.until = [0] * nnz
        self.bo = (p.backoff_ns + p.heartbeat_ns - 1) // p.heartbeat_ns
        self.events = np.zeros((N, EVENT_COLS), np.int64)
        self.max_degree = max(self.row[u + 1] - self.row[u] for u in range(N))

    def _pick(self, cand, purpose, u, epoch):
        """Candidates in ascending (rng key, entry) order."""
        seed = self.p.seed
        return [e for _, e in sorted((oracle.rng(seed, purpose, u, epoch, self.col[e]), e) for e in cand)]

    def gauges(self, off):
        p, N, row, mesh = self.p, self.N, self.row, self.mesh
        g = [0] * SERIES_COLS
        for u in range(N):
            m = sum(mesh[row[u]:row[u + 1]])
            g[LINKS] += m
            if off is not None and off[u]:
                continue
            g[ONLINE] += 1
            if m == 0:
                g[NO_PEERS] += 1
            elif m < p.d_lo:
                g[LOW] += 1
            else:
                g[HEALTHY] += 1
            if m > p.d_hi:
                g[OVER] += 1
        return g

    def epoch(self, epoch, off, sub):
        """One epoch; returns (changes as mesh_epoch counts them, the epoch's series row)."""
        p, N, row, col, rev = self.p, self.N, self.row, self.col, self.rev
        mesh, until, out = self.mesh, self.until, self.out
        ev = self.events
        s = [0] * SERIES_COLS
        nnz = len(col)
        prop = [0] * nnz  # 1 graft, 2 prune
        acc = [False] * nnz
        # 0: links to offline peers leave the mesh (no PRUNE, no back-off); each end counts its entry
        if off is not None:
            for u in range(N):
                for e in range(row[u], row[u + 1]):
                    if mesh[e] and (off[u] or off[col[e]]):
                        mesh[e] = False
                        ev[u, ME_MESH_DROP] += 1
                        s[DROPS] += 1
        before = list(mesh)  # the mesh after the disconnect
        if sub:  # A0: the first D_lo connections in subscription-arrival order
            hs = p.hs_rtts if p.hs_rtts else HS_RTTS_DEFAULT
            for u in range(N):
                su = self.stage[u]
                cand = []
                for e in range(row[u], row[u + 1]):
                    if not mesh[e]:
                        sw = self.stage[col[e]]
                        cand.append((hs * (self.lat[su][sw] + self.lat[sw][su]) + self.lat[sw][su], e))
                for _, e in sorted(cand)[:p.d_lo]:
                    prop[e] |= 1
        else:  # A: heartbeat decisions
            for u in range(N):
                if off is not None and off[u]:
                    continue
                ents = range(row[u], row[u + 1])
                m = sum(1 for e in ents if mesh[e])
                o = sum(1 for e in ents if mesh[e] and out[e])
                mm, oo = m, o

                def elig(e):
                    return not mesh[e] and epoch > until[e] and not (off is not None and off[col[e]])

                if m < p.d_lo:
                    for e in self._pick([e for e in ents if elig(e)], P_GRAFT, u, epoch)[:p.d - m]:
                        prop[e] |= 1
                        mm += 1
                        oo += out[e]
                if mm > p.d_hi:
                    excess, removed = mm - p.d, 0
                    for e in self._pick([e for e in ents if mesh[e]], P_PRUNE, u, epoch):
                        if removed >= excess:
                            break
                        if out[e]:
                            if oo <= p.d_out:
                                continue
                            oo -= 1
                        prop[e] |= 2
                        removed += 1
                        mm -= 1
                if mm >= p.d_lo and oo < p.d_out:
                    cand = [e for e in ents if out[e] and elig(e) and not (prop[e] & 1)]
                    for e in self._pick(cand, P_OUT_GRAFT, u, epoch)[:p.d_out - oo]:
                        prop[e] |= 1
                        mm += 1
        for e in range(nnz):
            u, w = self.src[e], col[e]
            if prop[e] & 1:
                ev[u, ME_GRAFT_TX] += 1
                ev[w, ME_GRAFT_RX] += 1
                s[GRAFTS] += 1
            if prop[e] & 2:
                ev[u, ME_PRUNE_TX] += 1
                ev[w, ME_PRUNE_RX] += 1
                s[PRUNES] += 1
        # B: receivers handle GRAFTs in (arrival, id) order
        for w in range(N):
            sw = self.stage[w]
            ents = range(row[w], row[w + 1])
            c = sum(1 for e in ents if (mesh[e] and not (prop[e] & 2)) or (prop[e] & 1))
            inbox = []
            for e in ents:
                if prop[rev[e]] & 1:
                    su = self.stage[col[e]]
                    if sub:
                        hs = p.hs_rtts if p.hs_rtts else HS_RTTS_DEFAULT
                        key = (hs + 1) * (self.lat[su][sw] + self.lat[sw][su])
                    else:
                        key = self.lat[su][sw]
                    inbox.append((key, e))
            for _, e in sorted(inbox):  # (arrival, entry): entries ascend with the sender's id
                in_mesh = (mesh[e] and not (prop[e] & 2)) or (prop[e] & 1)
                if in_mesh:
                    acc[rev[e]] = True
                    continue
                if epoch < until[e] or (c >= p.d_hi and not out[e]):
                    until[e] = epoch + self.bo  # the PRUNE reply
                    ev[w, ME_PRUNE_TX] += 1
                    ev[col[e], ME_PRUNE_RX] += 1
                    s[REJECTS] += 1
                    continue
                acc[rev[e]] = True
                mesh[e] = True
                c += 1
        # C: PRUNEs and rejections applied, both ends back off
        changes = 0
        for e in range(nnz):
            pr = prop[e]
            if pr & 1:
                changes += 1
                if acc[e]:
                    mesh[e] = True
                else:
                    mesh[e] = False
                    until[e] = epoch + self.bo
            if pr & 2:
                changes += 1
                mesh[e] = False
                until[e] = epoch + self.bo
            if prop[rev[e]] & 2:
                mesh[e] = False
                until[e] = epoch + self.bo
        for e in range(nnz):
            if mesh[e] and not before[e]:
                ev[self.src[e], ME_MESH_ADD] += 1
                s[ADDS] += 1
            elif before[e] and not mesh[e]:
                ev[self.src[e], ME_MESH_DEL] += 1
                s[DELS] += 1
        g = self.gauges(off)
        for k in (ONLINE, NO_PEERS, LOW, HEALTHY, OVER, LINKS):
            s[k] = g[k]
        return changes, s

    def wake(self, epoch):
        """The converge loop's jump: the earliest back-off expiry that can wake a hungry peer."""
        p, row, mesh, out, until = self.p, self.row, self.mesh, self.out, self.until
        wake = None
        for u in range(self.N):
            ents = range(row[u], row[u + 1])
            m = sum(1 for e in ents if mesh[e])
            o = sum(1 for e in ents if mesh[e] and out[e])
            need_any = m < p.d_lo
            need_out = not need_any and m <= p.d_hi and o < p.d_out
            if not need_any and not need_out:
                continue
            for e in ents:
                if mesh[e] or (need_out and not out[e]):
                    continue
                if until[e] >= epoch + 1 and (wake is None or until[e] + 1 < wake):
                    wake = until[e] + 1
        return wake

    def ell(self):
        """(mesh [N, 16] ascending ids padded with 2^32 - 1, count [N]) as the oracle extracts them."""
        N = self.N
        mesh = np.full((N, oracle.MESH_W), 0xFFFFFFFF, np.uint32)
        cnt = np.zeros(N, np.uint8)
        for u in range(N):
            ids = [self.col[e] for e in range(self.row[u], self.row[u + 1]) if self.mesh[e]]
            assert len(ids) <= oracle.MESH_W
            mesh[u, :len(ids)] = ids
            cnt[u] = len(ids)
        return mesh, cnt


def reference(p, stages, links, max_hb):
    """-> dict(events uint64 [N, 7], series uint64 [epochs + 1, 12], epochs, stepped (the epochs
    that ran), max_degree, mesh, count (the final mesh)). Asserts the pinning to the oracle."""
    M = _Mesh(p, stages, links)
    N = p.peers
    rows = {}  # epoch -> series row
    last = 0
    if p.churn_ppm:
        snaps = oracle.mesh_churn(p, M.row_ptr, M.col_np, M.flags0, M.stage_np, M.lat_np, 0, max_hb)
        for h in range(max_hb + 1):
            off = None
            if h == 0:
                if p.sub_graft:
                    rows[0] = M.epoch(0, None, True)[1]
            else:
                off = [oracle.offline(p, u, h) for u in range(N)]
                rows[h] = M.epoch(h, off, False)[1]
            mesh, cnt = M.ell()
            np.testing.assert_array_equal(mesh, snaps[0][h], err_msg="mesh of epoch %d" % h)
            np.testing.assert_array_equal(cnt, snaps[1][h], err_msg="mesh size of epoch %d" % h)
            np.testing.assert_array_equal(np.array(off if off else [0] * N, np.uint8), snaps[2][h],
                                          err_msg="offline set of epoch %d" % h)
        last = max_hb
    else:
        if p.sub_graft:
            rows[0] = M.epoch(0, None, True)[1]
        epoch = 1
        while epoch <= max_hb:
            changes, rows[epoch] = M.epoch(epoch, None, False)
            last = epoch
            if changes:
                epoch += 1
                continue
            wake = M.wake(epoch)
            if wake is None or wake > max_hb:
                break
            epoch = wake
        _, omesh, ocnt, oep = oracle.mesh_converge(p, M.row_ptr, M.col_np, M.flags0, M.stage_np, M.lat_np, max_hb)
        mesh, cnt = M.ell()
        np.testing.assert_array_equal(mesh, omesh, err_msg="final mesh")
        np.testing.assert_array_equal(cnt, ocnt, err_msg="final mesh size")
        assert last == oep, (last, oep)
    # an epoch the jump skipped changes nothing: no events, the previous row's gauges
    series = np.zeros((last + 1, SERIES_COLS), np.uint64)
    prev = [0] * SERIES_COLS
    prev[ONLINE] = prev[NO_PEERS] = N  # before epoch 0: the empty mesh, everyone online
    for h in range(last + 1):
        if h in rows:
            prev = rows[h]
        else:
            prev = [prev[k] if k <= LINKS else 0 for k in range(SERIES_COLS)]
        series[h] = prev
    mesh, cnt = M.ell()
    out = dict(events=M.events.astype(np.uint64), series=series, epochs=last, stepped=sorted(rows),
               max_degree=M.max_degree, mesh=mesh, count=cnt)
    out["events"].setflags(write=False)
    out["series"].setflags(write=False)
    return out


def check_identities(events, series):
    """The identities of DESIGN.md §2.15 between the per-peer columns and the series."""
    ev = np.asarray(events).astype(np.int64)
    se = np.asarray(series).astype(np.int64)
    tot, st = ev.sum(axis=0), se.sum(axis=0)
    assert tot[ME_GRAFT_TX] == tot[ME_GRAFT_RX] == st[GRAFTS]
    assert tot[ME_PRUNE_TX] == tot[ME_PRUNE_RX] == st[PRUNES] + st[REJECTS]
    assert tot[ME_MESH_ADD] == st[ADDS] and tot[ME_MESH_DEL] == st[DELS] and tot[ME_MESH_DROP] == st[DROPS]
    links = 0
    for h in range(len(se)):
        links = links - se[h, DROPS] + se[h, ADDS] - se[h, DELS]
        assert se[h, LINKS] == links, h
        assert se[h, ONLINE] == se[h, NO_PEERS] + se[h, LOW] + se[h, HEALTHY], h
        assert se[h, OVER] <= se[h, HEALTHY], h


L5 = (5, (50, 150, 40, 130))
WIDE = dict(peers=200, connect_to=40, seed=1, sub_graft=0, d_out=2)  # max degree 87: 64-lane rows

# The cases of tests/test_mesh_events_cpu.py and tests/test_gpu_mesh_events.py.
# name -> (oracle params over the rust preset, (stages, links), max_heartbeats, epochs,
#          series sums GRAFTS, REJECTS, PRUNES, DROPS, ADDS, DELS)
CASES = {
    "A": (dict(peers=300, seed=1), L5, 400, 7, (1872, 293, 310, 0, 2606, 580)),
    "B": (dict(peers=257, seed=2, sub_graft=0, d_out=2), L5, 400, 6, (1615, 335, 307, 0, 2106, 572)),
    "C": (dict(peers=100, seed=2), (1, (50, 50, 50, 50)), 400, 64, (720, 177, 186, 0, 972, 326)),
    "D": (dict(peers=300, seed=1, churn_ppm=10000, churn_down=10), L5, 40, 40, (2845, 461, 467, 1502, 4192, 896)),
    "E": (dict(peers=300, seed=3, churn_ppm=30000, churn_down=4, backoff_ns=3_000_000_000), L5, 40, 40,
          (5021, 880, 735, 4298, 7586, 1450)),
    "F": (dict(WIDE, churn_ppm=20000, churn_down=5), L5, 24, 24, (1820, 358, 392, 974, 2834, 716)),
    "G": (dict(peers=64, seed=1, churn_ppm=20000, churn_down=5), L5, 30, 30, (600, 67, 97, 382, 938, 184)),
    "H": (WIDE, L5, 400, 5, (1286, 333, 400, 0, 1818, 718)),
}
SUMS = [GRAFTS, REJECTS, PRUNES, DROPS, ADDS, DELS]
_REF = {}


def ref_of(name):
    """The case's reference, computed once and shared (read-only arrays); reference() asserts
    the pinning to the oracle itself."""
    if name not in _REF:
        kw, (stages, links), max_hb = CASES[name][:3]
        _REF[name] = reference(oracle.params(**kw), stages, links, max_hb)
    return _REF[name]
