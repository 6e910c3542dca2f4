"""The host side of the mesh import (DESIGN.md §2.3 "A caller's mesh"): the link file's writer against
the dial list's reader, the Python wrappers' array checks, the rust declarations, shadow_parity's
--mesh. No GPU."""
import os
import re

import numpy as np
import pytest

import gossipsim
import shadow_parity

E = 0xFFFFFFFF
W = gossipsim.MESH_W


def rows(n, links):
    """Mesh rows [n, MESH_W] (ascending, EMPTY padded) and counts of the undirected links."""
    m, c = np.full((n, W), E, np.uint32), np.zeros(n, np.uint8)
    for a, b in sorted(set((min(x), max(x)) for x in links)):
        for u, w in ((a, b), (b, a)):
            m[u, c[u]] = w
            c[u] += 1
    return np.sort(m, axis=1), c


def test_writer_and_reader_round_trip(tmp_path):
    f = tmp_path / "m.txt"
    links = [(0, 2), (1, 2), (3, 2), (0, 4)]
    m, c = rows(5, links)
    gossipsim.write_mesh_links(f, m, c)
    assert f.read_text() == "0 2\n0 4\n1 2\n2 3\n"  # a < b, in row order
    a, b = gossipsim.read_dials(f)
    assert sorted(zip(a.tolist(), b.tolist())) == sorted((min(x), max(x)) for x in links)
    gossipsim.write_mesh_links(f, m)  # without counts a row ends at its first EMPTY
    assert f.read_text() == "0 2\n0 4\n1 2\n2 3\n"
    gossipsim.write_mesh_links(f, m.reshape(-1), c)  # flat, as the C ABI takes it
    assert f.read_text() == "0 2\n0 4\n1 2\n2 3\n"
    # the counts decide, not what stands behind them; rows in any order inside
    m2 = m.copy()
    m2[2, :3] = [3, 0, 1]
    m2[4, 1:] = 1
    gossipsim.write_mesh_links(f, m2, c)
    assert f.read_text() == "0 2\n0 4\n1 2\n2 3\n"
    # comments and blank lines go through the reader
    f.write_text("# the mesh at the end of run 3\n\n2 0\n  1\t2   # either orientation\n\n")
    a, b = gossipsim.read_dials(f)
    assert a.tolist() == [2, 1] and b.tolist() == [0, 2]


def test_the_empty_mesh_and_a_large_id(tmp_path):
    f = tmp_path / "e.txt"
    m, c = rows(6, [])
    gossipsim.write_mesh_links(f, m, c)
    assert f.read_text() == ""
    assert [len(x) for x in gossipsim.read_dials(f)] == [0, 0]
    gossipsim.write_mesh_links(f, m)
    assert f.read_text() == ""
    big = (1 << 24) - 1  # the widest id a packed mesh entry holds; the writer reads the rows it is given
    m = np.full((3, W), E, np.uint32)
    m[0, :2], m[1, 0], m[2, 0] = [2, big], big, 0
    gossipsim.write_mesh_links(f, m, np.array([2, 1, 1], np.uint8))
    assert f.read_text() == "0 2\n0 %d\n1 %d\n" % (big, big)
    a, b = gossipsim.read_dials(f)
    assert a.tolist() == [0, 0, 1] and b.tolist() == [2, big, big]
    m, c = rows(6, [(0, 1)])
    with pytest.raises(gossipsim.GossipSimError, match="GS_EINVAL"):
        gossipsim.write_mesh_links(tmp_path / "no" / "dir.txt", m[:4], c[:4])


def test_wrappers_check_arrays_before_the_call(tmp_path):
    sim = gossipsim.Simulator.__new__(gossipsim.Simulator)  # no context: a check that passes would fail on it
    sim.peers, sim.ctx = 5, None
    m, c = rows(5, [(0, 1)])
    for bad, exc in ((m[:4], ValueError), (m[:, :8], ValueError), (m.astype(np.float64), TypeError),
                     (m.astype(np.int64) - 2, ValueError), (m.reshape(5, 4, 4), ValueError)):
        with pytest.raises(exc):
            sim.set_mesh(bad, c if bad.shape[0] == 5 else None)
        if bad.shape != (4, W):  # (four rows are a mesh of four peers to the writer)
            with pytest.raises(exc):
                gossipsim.write_mesh_links(tmp_path / "x", bad)
    for bad, exc in ((c[:4], ValueError), (c.astype(np.float32), TypeError), (c.astype(np.int32) + 256, ValueError),
                     (c.reshape(5, 1), ValueError)):
        with pytest.raises(exc):
            sim.set_mesh(m, bad)
    for a, b, exc in (([0, 1], [1], ValueError), ([-1], [0], ValueError), ([0.5], [1], TypeError),
                      ([[0]], [[1]], ValueError), ([1 << 32], [0], ValueError)):
        with pytest.raises(exc, match="a |b "):
            sim.set_mesh_links(a, b)
    assert not os.path.exists(tmp_path / "x")


def test_rust_crate_declares_the_entries():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "rust", "gossipsim-sys", "src", "lib.rs")).read()
    hdr = open(os.path.join(root, "include", "gossipsim.h")).read()
    for name, args in (("gs_set_mesh", 3), ("gs_set_mesh_links", 4), ("gs_write_mesh_links", 4)):
        decl = re.search(r"pub fn %s\(([^)]*)\)\s*->\s*gs_status;" % name, src)
        assert decl and len(decl.group(1).split(",")) == args, name
        cdecl = re.search(r"gs_status %s\(([^)]*)\);" % name, hdr)
        assert cdecl and len(cdecl.group(1).split(",")) == args, name
    assert gossipsim.SIGNATURES["gs_set_mesh_links"][1][1] is gossipsim.u64
    assert "#define GS_ABI_VERSION 10u" in hdr


class _Sim:
    def __init__(self):
        self.calls = []

    def mesh_converge(self):
        self.calls.append("converged")
        return 7

    def set_mesh_links(self, a, b):
        self.calls.append((a.tolist(), b.tolist()))


def test_shadow_parity_mesh_argument(tmp_path, monkeypatch):
    f = tmp_path / "mesh.txt"
    f.write_text("1 0\n0 2 # grafted late\n")
    a, b = _Sim(), _Sim()
    assert shadow_parity.form_mesh(a) == 7
    shadow_parity.form_mesh(b, str(f))
    assert a.calls == ["converged"] and b.calls == [([1, 0], [0, 2])]
    seen = {}
    monkeypatch.setattr(shadow_parity, "run", lambda args: seen.update(vars(args)) or {"pass": True, "per_message": []})
    assert shadow_parity.main(["--latencies", "l", "--peers", "3"]) == 0 and seen["mesh"] is None
    assert shadow_parity.main(["--latencies", "l", "--peers", "3", "--dials", "d", "--mesh", str(f)]) == 0
    assert seen["mesh"] == str(f) and seen["dials"] == "d"
