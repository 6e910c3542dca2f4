"""The list pass's per-row code with fewer instructions (gs_lpull_kernel.h,
gs_lpull_emit.h).

The emit step builds the mask of a lane's excluded mesh entries (its source
and the message's publisher) from the row's entries by constant lane index: one
block for entries 0-7 and, in rows with more than 8 entries, one for 8-15. A
block that reads the wrong lanes, a mask bit in the wrong place or padding
that matches a source sends a message back where it came from or drops a
receiver; the classification step decides which lanes are final, pending or
dead from the chunks' minima, and a lane in the wrong class is emitted twice,
never, or in the wrong window. Either changes completion times, hops or
counters, so every case is bit-exact against the CPU oracle, once with the
final log (collect=True: t_complete, hops, the eight counters) and once as the
counters-only twin (collect=False: the counters).

The shapes: meshes whose every row has more than 8 entries, up to 15 (the
library takes D_hi < MESH_W = 16: gs_create refuses D_hi = 16, so no converged
row is 16 wide), and meshes with rows on both sides of 8, each in rows of CH = 8 and CH = 16,
with random publishers and with one publisher of the largest degree for up to
256 lanes of the batch (the body that excludes source and publisher in the
widest rows); chunks that hold only
finals and then only dead lanes, chunks that hold finals and pendings at once,
and rows whose upper chunks are never touched. What a shape is meant to produce
is asserted from the oracle's mesh and completion times."""
import functools

import numpy as np
import pytest

import oracle
from test_gpu_parity import UND, _sched, gpu_sim
from test_gpu_record_stream import (COUNTERS, LINKS, UNIFORM, _exact, _finals_per_window, _one_publisher, _window_ns)

pytestmark = pytest.mark.gpu

N = 300
# mesh degrees 9..15 (every value present; 15 = MESH_W - 1 is the widest row a context takes) and 8..12
WIDE = dict(d=12, d_lo=9, d_hi=15, connect_to=20)
BOTH_SIDES = dict(d=9, d_lo=8, d_hi=12, connect_to=16)
# One publisher's lanes take the same paths at the same times, and on five link classes
# each of them is listed for the same later windows: in these meshes 384 such lanes outgrow
# a row's list of 1024 entries (ERR_LIST: the batch leaves the list pass; so it does at the
# parent commit, profiles/r15_insn/lockstep_list_overflow.txt), 256 do not. A batch of 128
# is one publisher's throughout; of 1024 lanes the first 256 are, the others have a
# publisher each.
LOCKSTEP = 256


def _both(p, S, links, sched, batch, ref):
    """The schedule on a fresh context with its log and on another as a
    counters-only run, both against one oracle run, every batch on the list pass."""
    sim, _ = gpu_sim(p, S, links, batch=batch)
    st = _exact(sim, sim.run(sched), ref)
    sim2, _ = gpu_sim(p, S, links, batch=batch)
    sim2.run(sched, collect=False)
    st2 = sim2.stats()
    for k in COUNTERS:
        assert st2[k] == ref["stats"][k], "collect=False: " + k
    assert st["list_pull_batches"] == st["batches"] > 0
    assert st2["list_pull_batches"] == st2["batches"] > 0


def _window_of(ref, sched, delta):
    """[messages, peers]: the window of its own publish-relative time in which a
    message becomes final at a peer (as _finals_per_window counts them); -1 for
    the publisher's own lane and for a message that never arrives."""
    tc = ref["t_complete"]
    ok = tc != UND
    ok[np.arange(tc.shape[0]), np.asarray(sched[1])] = False
    rel = tc - np.asarray(sched[0], np.uint64)[:, None]
    return np.where(ok, rel // np.uint64(delta), 0).astype(np.int64) - (~ok).astype(np.int64)


@functools.lru_cache(maxsize=None)
def _mesh_case(wide, B, one):
    """Parameters, schedule and oracle run of one mesh case (computed once, not changed)."""
    p = oracle.params(peers=N, seed=131, lazy_gossip=0, **(WIDE if wide else BOTH_SIDES))
    t, pub, size = _sched(B, N)
    if one:  # from the peer with the most mesh entries (the mesh does not depend on the schedule)
        cnt = oracle.simulate(p, 5, LINKS, sched=_sched(1, N))["cnt"]
        pub = pub.copy()
        pub[:LOCKSTEP] = int(np.argmax(cnt))
    sched = (t, pub, size)
    return p, sched, oracle.simulate(p, 5, LINKS, sched=sched)


@pytest.mark.parametrize("one", [False, True], ids=["random_publishers", "one_publisher"])
@pytest.mark.parametrize("B", [128, 1024])
def test_mesh_rows_wider_than_8(monkeypatch, B, one):
    """Every row has 9 to 15 mesh entries, 24 rows the 15 that D_hi < MESH_W
    allows: each emit iteration runs both blocks of the excluded-entry mask, in
    rows of CH = 8 (B = 128) and CH = 16 (B = 1024). One publisher of the
    largest degree (LOCKSTEP): its 15 neighbours' rows exclude source and publisher."""
    monkeypatch.setenv("GS_REQUIRE_LPULL", "1")
    p, sched, ref = _mesh_case(True, B, one)
    cnt = ref["cnt"]
    assert cnt.min() > 8 and cnt.max() == 15, (cnt.min(), cnt.max())
    assert set(range(9, 16)) <= set(int(c) for c in cnt)
    if one:
        assert cnt[sched[1][0]] == 15 and (sched[1][:min(B, LOCKSTEP)] == sched[1][0]).all()
    _both(p, 5, LINKS, sched, B, ref)


@pytest.mark.parametrize("one", [False, True], ids=["random_publishers", "one_publisher"])
@pytest.mark.parametrize("B", [128, 1024])
def test_mesh_rows_on_both_sides_of_8(monkeypatch, B, one):
    """Degrees 8 to 12 in one mesh: rows that skip the second block next to rows that run it."""
    monkeypatch.setenv("GS_REQUIRE_LPULL", "1")
    p, sched, ref = _mesh_case(False, B, one)
    cnt = ref["cnt"]
    assert cnt.min() == 8 < cnt.max(), (cnt.min(), cnt.max())
    _both(p, 5, LINKS, sched, B, ref)


def test_chunks_of_finals_only_then_dead_only(monkeypatch):
    """B = 1024 lanes of one publisher on one link class: a row's lanes are final
    in one window, so each of its 16 chunks holds only finals; the records that
    its other neighbours send afterwards meet chunks whose every lane is dead."""
    monkeypatch.setenv("GS_REQUIRE_LPULL", "1")
    B = 1024
    p = oracle.params(peers=N, seed=131, lazy_gossip=0)
    sched = _one_publisher(B, N)
    ref = oracle.simulate(p, 1, UNIFORM, sched=sched)
    fw = _finals_per_window(ref, sched, _window_ns(p, 1, UNIFORM))
    # every row but the publisher's takes all its B finals in one window ...
    rows = np.setdiff1d(np.arange(N), sched[1][:1])
    assert (fw[rows].max(axis=1) == B).all()
    # ... and in some row a neighbour is final in a later window than the row itself: its
    # records reach lanes that are final already
    mesh, cnt = ref["mesh"], ref["cnt"]
    first = fw.argmax(axis=1)
    assert any((first[mesh[w, :cnt[w]].astype(np.int64) & 0xFFFFFF] > first[w]).any() for w in rows)
    _both(p, 1, UNIFORM, sched, B, ref)


@pytest.mark.parametrize("B", [65, 513, 1024])
def test_chunks_of_finals_and_pendings(monkeypatch, B):
    """Random publishers on the bench's links: a row's lanes spread over the
    windows, so a chunk holds finals, pendings and dead lanes at once. B = 1024:
    all 16 chunks. B = 513: rows of CH = 16 whose chunk 8 holds one lane and
    whose chunks 9-15 are never touched. B = 65: the same edge at chunk 1 (rows
    of 65 lanes run at CH = 8: chunks 2-7 are never touched)."""
    monkeypatch.setenv("GS_REQUIRE_LPULL", "1")
    p = oracle.params(peers=N, seed=131, lazy_gossip=0)
    sched = _sched(B, N)
    ref = oracle.simulate(p, 5, LINKS, sched=sched)
    # every row has a chunk in which some lanes are final in one window and others in a
    # later one: its neighbours (final a window or more before it, each forwarding every
    # lane) have sent candidates for the later lanes by then, so they stand as pendings
    win = _window_of(ref, sched, _window_ns(p, 5, LINKS))  # [messages, peers], -1: the publisher's own lane
    mixed = np.zeros(N, bool)
    for q in range(0, B, 64):
        w = win[q:q + 64]
        lo = np.where(w >= 0, w, np.iinfo(np.int64).max).min(axis=0)
        mixed |= (w.max(axis=0) > lo) & (lo != np.iinfo(np.int64).max)
    assert mixed.all(), int(mixed.sum())
    if B % 64 == 1:  # the last chunk holds one lane
        assert (B - 1) // 64 < (8 if B <= 512 else 16) - 1
    _both(p, 5, LINKS, sched, B, ref)

