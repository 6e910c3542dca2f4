"""The host side of the graph import: the dial list's text file, the numpy
helper tests/topo_ref.py against the oracle's builder, shadow_parity's --dials. No GPU."""
import numpy as np
import pytest

import gossipsim
import oracle
import shadow_parity
import topo_ref as T

u32, u64 = gossipsim.u32, gossipsim.u64


def _read(path, cap):
    d, t, n = np.full(max(cap, 1), 77, np.uint32), np.full(max(cap, 1), 77, np.uint32), u64()
    rc = gossipsim.lib().gs_read_dials(str(path).encode(), gossipsim._ptr(d, u32), gossipsim._ptr(t, u32), cap,
                                       gossipsim.ctypes.byref(n))
    return rc, n.value, d, t


def test_read_dials_comments_blanks_and_cap(tmp_path):
    f = tmp_path / "d.txt"
    f.write_text("# dials of run 3\n\n0 1\n  2\t0   # peer 2 dialed 0\n\n   \n16777215 4294967295\n#1 2\n")
    d, t = gossipsim.read_dials(f)
    assert d.dtype == t.dtype == np.uint32
    assert d.tolist() == [0, 2, 16777215] and t.tolist() == [1, 0, 4294967295]
    n = u64()
    assert gossipsim.lib().gs_read_dials(str(f).encode(), None, None, 0, gossipsim.ctypes.byref(n)) == gossipsim.GS_ERANGE
    assert n.value == 3
    rc, rows, dd, tt = _read(f, 2)  # too small: the rows that fit, the count, GS_ERANGE
    assert (rc, rows) == (gossipsim.GS_ERANGE, 3) and dd.tolist() == [0, 2] and tt.tolist() == [1, 0]
    rc, rows, dd, tt = _read(f, 3)
    assert (rc, rows) == (0, 3) and dd.tolist() == d.tolist()
    empty = tmp_path / "e.txt"
    empty.write_text("# nothing\n")
    assert [len(x) for x in gossipsim.read_dials(empty)] == [0, 0]


@pytest.mark.parametrize("text", ["0 1\nx 2\n", "0 1\n5\n", "0 1 2\n", "0 -1\n", "0 4294967296\n", "0 1x\n", "0.5 1\n"])
def test_read_dials_malformed(tmp_path, text):
    f = tmp_path / "bad.txt"
    f.write_text(text)
    rc, _, _, _ = _read(f, 8)
    assert rc == gossipsim.GS_EINVAL
    with pytest.raises(gossipsim.GossipSimError, match="GS_EINVAL"):
        gossipsim.read_dials(f)
    with pytest.raises(gossipsim.GossipSimError, match="GS_EINVAL"):
        gossipsim.read_dials(tmp_path / "missing.txt")


def test_write_dials_hand_arrays(tmp_path):
    big = (1 << 24) - 1
    # peer 0 -- 2 (0 dialed), 1 -- 2 (mutual), 2 -- big (big dialed); bit 1 (mesh) is not read
    row = np.zeros(big + 2, np.uint64)
    row[1:] = 1
    row[2:] = 2
    row[3:] = 5
    row[big + 1] = 6
    col = np.array([2, 2, 0, 1, big, 2], np.uint32)
    flags = np.array([1, 3, 2, 1, 0, 1], np.uint8)
    f = tmp_path / "w.txt"
    gossipsim.write_dials(f, row, col, flags)
    assert f.read_text() == "0 2\n1 2\n2 1\n%d 2\n" % big
    d, t = gossipsim.read_dials(f)
    assert d.tolist() == [0, 1, 2, big] and t.tolist() == [2, 2, 1, 2]
    with pytest.raises(ValueError):
        gossipsim.write_dials(f, row, col[:-1], flags[:-1])
    with pytest.raises(TypeError):
        gossipsim.write_dials(f, row, col.astype(np.float32), flags)
    with pytest.raises(gossipsim.GossipSimError, match="GS_EINVAL"):
        gossipsim.write_dials(tmp_path / "no" / "dir.txt", row[:4], col[:5], flags[:5])


def test_helper_round_trip_on_the_built_graph():
    """The dials read off a built CSR's F_OUT bits give back the same CSR (the builder's graph is
    the union of its accepted dials), in any order."""
    p = oracle.params(peers=257, seed=5)
    row, col, flags = oracle.build_topology(p)
    d, t = T.csr_to_dials(row, col, flags)
    assert (len(d), len(col)) == (2827, 5524) and len(d) - len(col) // 2 == 65  # 130 entries of mutual pairs
    perm = np.random.default_rng(2).permutation(len(d))
    for dd, tt in ((d, t), (d[perm], t[perm])):
        r2, c2, f2 = T.dials_to_csr(257, dd, tt)
        np.testing.assert_array_equal(r2, row)
        np.testing.assert_array_equal(c2, col)
        np.testing.assert_array_equal(f2, flags & 1)


def test_test_graphs_are_what_the_cases_say():
    for name, dials, nnz, dmin, dmax in (("G1", 1494, 2972, 7, 15), ("G2", 720, 1436, 4, 202), ("G3", 718, 1436, 4, 202),
                                         ("G4", 800, 1600, 8, 8), ("G5", 39, 78, 1, 2), ("G6", 1500, 3000, 10, 10)):
        N, d, t, pubs = T.graph(name)
        row, col, flags = T.dials_to_csr(N, d, t)
        deg = np.diff(row.astype(np.int64))
        assert (len(d), len(col), deg.min(), deg.max()) == (dials, nnz, dmin, dmax), name
        assert len(np.unique(d.astype(np.int64) * N + t)) == len(d) and (d != t).all() and max(pubs) < N
        rows = np.repeat(np.arange(N), deg)
        assert (np.diff(col.astype(np.int64))[np.diff(rows) == 0] > 0).all()  # rows strictly ascending


class _Sim:
    def __init__(self):
        self.calls = []

    def connect_gossipsub_peers(self):
        self.calls.append("built")

    def set_dials(self, d, t):
        self.calls.append((d.tolist(), t.tolist()))


def test_shadow_parity_dials_argument(tmp_path, monkeypatch):
    f = tmp_path / "dials.txt"
    f.write_text("1 0\n2 0 # late joiner\n")
    a, b = _Sim(), _Sim()
    shadow_parity.connect(a)
    shadow_parity.connect(b, str(f))
    assert a.calls == ["built"] and b.calls == [([1, 2], [0, 0])]
    seen = {}
    monkeypatch.setattr(shadow_parity, "run", lambda args: seen.update(vars(args)) or {"pass": True, "per_message": []})
    assert shadow_parity.main(["--latencies", "l", "--peers", "3"]) == 0 and seen["dials"] is None
    assert shadow_parity.main(["--latencies", "l", "--peers", "3", "--dials", str(f)]) == 0 and seen["dials"] == str(f)
