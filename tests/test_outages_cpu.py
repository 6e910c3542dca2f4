"""The host side of a caller's outages (DESIGN.md §2.8 "A caller's outages"), no GPU: the text
file's reader, the time-to-epoch conversion against outage_ref's restatement, the declarations,
and the two facts about the oracle the GPU tests of test_gpu_outages.py rest on."""
import os
import re

import numpy as np
import pytest

import gossipsim
import oracle
import outage_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HB = 400_000_000
PHASE = 1_000_000_123
NEVER = gossipsim.T_NEVER
FOREVER = gossipsim.OUTAGE_FOREVER


class _Cfg:
    heartbeat_ns, hb_phase_ns = HB, PHASE


def _raw_read(path, cap):
    """gs_read_outages with room for `cap` rows -> (status, n, rows)."""
    L = gossipsim.lib()
    n = gossipsim.u64()
    p, d, t = np.zeros(max(cap, 1), np.uint32), np.zeros(max(cap, 1), np.uint64), np.zeros(max(cap, 1), np.uint64)
    rc = L.gs_read_outages(str(path).encode(), gossipsim._ptr(p, gossipsim.u32), gossipsim._ptr(d, gossipsim.u64),
                           gossipsim._ptr(t, gossipsim.u64), cap, gossipsim.ctypes.byref(n))
    return rc, n.value, list(zip(p[:cap].tolist(), d[:cap].tolist(), t[:cap].tolist()))


def test_reader_columns_comments_and_cap(tmp_path):
    f = tmp_path / "o.txt"
    f.write_text("# pod restarts of run 7\n\n3 100 200\n  4\t150   # never came back\n\n"
                 "4294967295 0 18446744073709551614\n")
    p, d, t = gossipsim.read_outages(f)
    assert p.dtype == np.uint32 and d.dtype == np.uint64 and t.dtype == np.uint64
    assert p.tolist() == [3, 4, 4294967295]
    assert d.tolist() == [100, 150, 0]
    assert t.tolist() == [200, NEVER, 18446744073709551614]
    # the cap contract: GS_ERANGE with *n = rows, the rows that fit are written; NULL arrays count only
    rc, n, rows = _raw_read(f, 2)
    assert rc == gossipsim.GS_ERANGE and n == 3 and rows == [(3, 100, 200), (4, 150, NEVER)]
    rc, n, rows = _raw_read(f, 3)
    assert rc == 0 and n == 3 and rows[2] == (4294967295, 0, 18446744073709551614)
    n = gossipsim.u64()
    assert gossipsim.lib().gs_read_outages(str(f).encode(), None, None, None, 0, gossipsim.ctypes.byref(n)) == \
        gossipsim.GS_ERANGE and n.value == 3
    f.write_text("# nothing\n\n")
    assert [len(x) for x in gossipsim.read_outages(f)] == [0, 0, 0]


@pytest.mark.parametrize("bad", ["7", "1 2 3 4", "x 1 2", "1 -5 9", "4294967296 1 2", "1 2 18446744073709551616",
                                 "1 2x 3", "+1 2 3"])
def test_reader_names_the_bad_line(tmp_path, bad):
    f = tmp_path / "o.txt"
    f.write_text("# c\n0 1 2\n\n%s\n5 6 7\n" % bad)
    rc, n, _ = _raw_read(f, 8)
    assert rc == gossipsim.GS_EINVAL and n == 4  # the fourth line of the file
    with pytest.raises(gossipsim.GossipSimError, match=r"GS_EINVAL.*line 4"):
        gossipsim.read_outages(f)
    with pytest.raises(gossipsim.GossipSimError, match="GS_EINVAL"):
        gossipsim.read_outages(tmp_path / "missing.txt")


def _conv(rows):
    p, d, t = (np.array(x, dt) for x, dt in zip(zip(*rows), (np.uint32, np.uint64, np.uint64)))
    po, a, b = gossipsim.outage_epochs(_Cfg, p, d, t)
    return list(zip(po.tolist(), a.tolist(), b.tolist()))


def _ref(rows):
    out = []
    for u, d, t in rows:
        e = outage_ref.epochs_of(HB, PHASE, d, t)
        if e is not None:
            out.append((u, e[0], e[1]))
    return out


def test_conversion_named_cases():
    at = lambda h: PHASE + h * HB
    cases = [
        ([(1, at(5), at(9) + 1)], [(1, 5, 10)]),      # t_down on a heartbeat: that epoch is included
        ([(1, at(5) + 1, at(9))], [(1, 6, 9)]),       # t_up on a heartbeat: that epoch is excluded
        ([(1, at(5) + 1, at(6) - 1)], []),            # between two heartbeats: left out
        ([(1, at(5) + 1, at(6))], []),                # up exactly at the next heartbeat: still none
        ([(1, at(5), at(5) + 1)], [(1, 5, 6)]),       # one heartbeat
        ([(1, 17, at(3) + 5)], [(1, 1, 4)]),          # down before the phase: clamped to 1
        ([(1, PHASE, at(1))], []),                    # the phase itself is epoch 0's heartbeat: nobody offline there
        ([(1, 0, PHASE)], []),
        ([(1, at(7) - 3, NEVER)], [(1, 7, FOREVER)]),  # forever
        ([(1, 0, NEVER)], [(1, 1, FOREVER)]),
        # two outages disjoint in time that touch in epochs: [5, 7) and [7, 9)
        ([(2, at(5) - 9, at(6) + 10), (2, at(6) + 20, at(8) + 1)], [(2, 5, 7), (2, 7, 9)]),
        # input order kept, the dropped one leaves no hole
        ([(9, at(4), at(5)), (3, at(2) + 1, at(2) + 2), (0, at(1), NEVER)], [(9, 4, 5), (0, 1, FOREVER)]),
    ]
    for rows, want in cases:
        assert _conv(rows) == want, rows
        assert _ref(rows) == want, rows
    po, a, b = gossipsim.outage_epochs(_Cfg, [], [], [])
    assert len(po) == len(a) == len(b) == 0
    with pytest.raises(gossipsim.GossipSimError, match="GS_EINVAL"):
        gossipsim.outage_epochs(_Cfg, [1], [100], [99])
    with pytest.raises(gossipsim.GossipSimError, match="GS_ERANGE"):
        gossipsim.outage_epochs(_Cfg, [1], [PHASE + (2 ** 32) * HB], [NEVER])


def test_conversion_random_against_the_restatement():
    rng = np.random.default_rng(11)
    rows = []
    for _ in range(600):
        d = int(rng.integers(0, PHASE + 50 * HB))
        if rng.random() < 0.3:  # on or right beside a heartbeat
            d = PHASE + int(rng.integers(0, 50)) * HB + int(rng.integers(-1, 2))
        t = d + int(rng.integers(0, 6 * HB))
        if rng.random() < 0.3:
            t = max(d, PHASE + int(rng.integers(0, 56)) * HB + int(rng.integers(-1, 2)))
        if rng.random() < 0.05:
            t = NEVER
        rows.append((int(rng.integers(0, 1000)), d, t))
    got, want = _conv(rows), _ref(rows)
    assert got == want
    assert 0 < len(want) < len(rows)  # some outages cover no heartbeat, most do
    # the table of the kept intervals is the definition applied cell by cell
    sel = rows[:40]
    tab = outage_ref.table(1000, _conv(sel), 0, 60)
    for u, d, t in sel:
        for h in range(1, 61):
            if d <= PHASE + h * HB < t:
                assert tab[h, u]
    assert not tab[0].any()


def test_reference_table_and_maximal_intervals():
    iv = [(0, 1, 2), (3, 2, 5), (3, 5, 7), (3, 9, FOREVER), (4, 6, 8)]
    tab = outage_ref.table(5, iv, 0, 12)
    assert tab[:, 0].nonzero()[0].tolist() == [1]
    assert tab[:, 3].nonzero()[0].tolist() == [2, 3, 4, 5, 6, 9, 10, 11, 12]
    assert not tab[0].any() and not tab[:, 1].any()
    # touching intervals are their union; a run that reaches the last row ends there
    assert outage_ref.maximal_intervals(tab) == [(0, 1, 2), (3, 2, 7), (3, 9, 13), (4, 6, 8)]
    assert (outage_ref.table(5, iv, 4, 6) == tab[4:7]).all()
    assert (outage_ref.table(5, outage_ref.maximal_intervals(tab), 0, 12) == tab).all()
    assert outage_ref.maximal_intervals(tab[4:7], 4) == [(3, 4, 7), (4, 6, 7)]


def test_declarations():
    src = open(os.path.join(ROOT, "rust", "gossipsim-sys", "src", "lib.rs")).read()
    hdr = open(os.path.join(ROOT, "include", "gossipsim.h")).read()
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name, args in (("gs_set_outages", 5), ("gs_clear_outages", 1), ("gs_get_offline", 4), ("gs_outage_epochs", 9),
                       ("gs_read_outages", 6)):
        decl = re.search(r"pub fn %s\(([^)]*)\)\s*->\s*gs_status;" % name, src)
        assert decl and len(decl.group(1).split(",")) == args, name
        cdecl = re.search(r"gs_status %s\(([^)]*)\);" % name, hdr)
        assert cdecl and len(cdecl.group(1).split(",")) == args, name
        assert len(gossipsim.SIGNATURES[name][1]) == args
        assert name in integ, name
    assert "#define GS_ABI_VERSION 10u" in hdr
    assert "#define GS_OUTAGE_FOREVER 0xFFFFFFFFu" in hdr and "#define GS_OUTAGE_ROW_MAX 256u" in hdr
    assert gossipsim.OUTAGE_FOREVER == outage_ref.FOREVER and gossipsim.T_NEVER == outage_ref.T_NEVER


# ---- the oracle facts the GPU tests rest on ----
N, STAGES, LINKS = 300, 5, (50, 150, 40, 130)
T0 = gossipsim.T0_NS


def _params(ppm=30000, down=6):
    return oracle.params(peers=N, seed=59, churn_ppm=ppm, churn_down=down, churn_horizon=10, heartbeat_ns=HB,
                         hb_phase_ns=T0 - 30 * HB + 150_000_000)


def test_oracle_converge_is_the_snapshot_under_churn():
    """oracle.mesh_converge(max_hb=h) under churn leaves exactly slot h of oracle.mesh_churn."""
    p = _params()
    lat, _ = oracle.topogen_links(STAGES, *LINKS)
    stage = (np.arange(N) % STAGES).astype(np.uint8)
    row, col, flags0 = oracle.build_topology(p)
    hs = (29, 30, 41, 54)
    snaps = oracle.mesh_churn_ranges(p, row, col, flags0, stage, lat, [(h, h) for h in hs])
    for h in hs:
        _, mesh, cnt, ep = oracle.mesh_converge(p, row, col, flags0, stage, lat, max_hb=h)
        smesh, scnt, soff = snaps[(h, h)]
        assert ep == h
        np.testing.assert_array_equal(mesh, smesh[0])
        np.testing.assert_array_equal(cnt, scnt[0])
        assert soff[0].any()  # somebody is offline: the snapshot is of a churn epoch


def test_oracle_run_churn_reads_no_churn_knob():
    """or_run_churn takes the snapshots and offline flags as arguments: the same snapshots under
    (30000, 6) and under (5, 2) give the same run."""
    p, q = _params(), _params(5, 2)
    lat, bw = oracle.topogen_links(STAGES, *LINKS)
    stage = (np.arange(N) % STAGES).astype(np.uint8)
    row, col, flags0 = oracle.build_topology(p)
    M = 16
    t = T0 + np.arange(M, dtype=np.uint64) * np.uint64(HB)
    pub, size = (6 + np.arange(M)) % N, np.full(M, 15000)
    h_lo = oracle.epoch_at(p, t[0])
    h_hi = oracle.epoch_at(p, t[-1]) + p.churn_horizon
    assert (h_lo, h_hi) == (29, 54)
    snaps = oracle.mesh_churn(p, row, col, flags0, stage, lat, h_lo, h_hi)
    a = oracle.run_churn(p, row, col, snaps, h_lo, stage, lat, bw, bw, t, pub, size)
    b = oracle.run_churn(q, row, col, snaps, h_lo, stage, lat, bw, bw, t, pub, size)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    assert a[2] == b[2]
    assert (a[0] == gossipsim.UNDELIVERED).any() and (a[0] != gossipsim.UNDELIVERED).any()
    # and the (5, 2) draw itself has nobody offline through epoch 60
    assert not any(oracle.offline(q, u, h) for u in range(N) for h in range(61))
