"""numpy reference of the dial-list import: dials -> the CSR gs_set_topology_dials must give."""
import numpy as np


def dials_to_csr(peers, dialer, target):
    """The undirected union of dialer[i] -> target[i]: (row_ptr u64, col u32, flags u8), rows
    ascending, flags bit 0 where the row's peer dialed col."""
    d, t = np.asarray(dialer, np.int64), np.asarray(target, np.int64)
    key = np.concatenate([d * peers + t, t * peers + d])          # (row, col) of both ends
    out = np.concatenate([np.ones(len(d), np.uint8), np.zeros(len(d), np.uint8)])
    uniq, inv = np.unique(key, return_inverse=True)
    flags = np.zeros(len(uniq), np.uint8)
    np.maximum.at(flags, inv, out)
    row_ptr = np.zeros(peers + 1, np.uint64)
    row_ptr[1:] = np.cumsum(np.bincount(uniq // peers, minlength=peers))
    return row_ptr, (uniq % peers).astype(np.uint32), flags


def _dials(pairs):
    """Distinct (dialer, target) pairs, sorted -> two uint32 arrays."""
    a = np.unique(np.asarray(pairs, np.int64).reshape(-1, 2), axis=0)
    return a[:, 0].astype(np.uint32), a[:, 1].astype(np.uint32)


def ring_dials(n, steps, base=0):
    return [(base + v, base + (v + s) % n) for v in range(n) for s in steps]


def graph(name):
    """The test graphs of tests/test_gpu_topology_import.py: -> (peers, dialer, target, publishers)."""
    if name == "G1":  # lattice + two random chords per peer
        rng, pairs = np.random.default_rng(3), ring_dials(300, (1, 2, 3))
        for v in range(300):
            pairs += [(v, int(x)) for x in rng.choice(300, 2, replace=False) if x != v]
        return (300,) + _dials(pairs) + ((6, 7, 150, 299),)
    if name in ("G2", "G3"):  # a hub of degree 202: dialed by 200 peers (G2), dialing them (G3)
        hub = [(v, 0) if name == "G2" else (0, v) for v in range(1, 201)]
        return (260,) + _dials(hub + ring_dials(260, (1, 2))) + ((0, 5, 230, 259),)
    if name == "G4":  # two components
        return (200,) + _dials(ring_dials(100, (1, 2, 3, 7)) + ring_dials(100, (1, 2, 3, 7), 100)) + ((6, 7, 150, 199),)
    if name == "G5":  # a path
        return (40,) + _dials([(v, v + 1) for v in range(39)]) + ((0, 13, 20, 39),)
    if name == "G6":  # a wider lattice, for the go preset
        return (300,) + _dials(ring_dials(300, (1, 2, 3, 11, 50))) + ((6, 7, 150, 299),)
    raise KeyError(name)


def csr_to_dials(row_ptr, col, flags):
    """The dials of a CSR: one (row's peer, col) per entry with bit 0, in row order."""
    rows = np.repeat(np.arange(len(row_ptr) - 1, dtype=np.uint32), np.diff(row_ptr.astype(np.int64)))
    m = (flags & 1) != 0
    return rows[m], col[m].astype(np.uint32)
