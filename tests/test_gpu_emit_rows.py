"""The list pass's emit step in two bodies and its row loop without a wait at
the header (gs_lpull_kernel.h, gs_lpull_emit.h).

Single-fragment rows run step 4 in one of two loop bodies, chosen per row: with
the message's publisher (rows marked LP_PUB: a publisher of the batch and its
mesh neighbours) or without any load. The row loop gathers the next row's
record counts inside the record step, so that nothing but stores is pending
when the next row begins. A wrong body (a publisher that forwards to itself, a
receiver mask that keeps the publisher), a stale mark from an earlier batch or
a header value read before it landed changes completion times, hops or
counters, so every case is bit-exact against the CPU oracle, once with the
final log (collect=True: t_complete, hops, the eight counters) and once as the
counters-only twin (collect=False: the counters).

The shapes: emit loops of 1, 63..65, 129 and 1024 finals in rows of both
bodies, batches in which every row needs the publisher, marks that change from
batch to batch, waves with 0 to 3 active rows (plain, with in-pass gossip and
in two loop-back parts) and rows of CH = 8 and CH = 16. What a shape is meant
to cover is asserted from the mesh and the oracle's completion times."""
import numpy as np
import pytest
import torch

import gossipsim
import oracle
from test_gpu_gossip_list import _phase
from test_gpu_parity import _knobs, _sched, gpu_sim
from test_gpu_record_stream import (COUNTERS, LINKS, UNIFORM, _exact, _finals_per_window, _first_diff, _one_publisher,
                                    _window_ns)

pytestmark = pytest.mark.gpu


def _both(p, S, links, sched, batch, on_list=True):
    """The schedule on a fresh context with its log and on another as a
    counters-only run, both against one oracle run."""
    ref = oracle.simulate(p, S, links, sched=sched)
    sim, _ = gpu_sim(p, S, links, batch=batch)
    st = _exact(sim, sim.run(sched), ref)
    sim2, _ = gpu_sim(p, S, links, batch=batch)
    sim2.run(sched, collect=False)
    st2 = sim2.stats()
    for k in COUNTERS:
        assert st2[k] == ref["stats"][k], "collect=False: " + k
    if on_list:
        assert st["list_pull_batches"] == st["batches"] > 0
        assert st2["list_pull_batches"] == st2["batches"] > 0
    return ref, st, st2


def _marked_rows(ref, pubs):
    """The rows of LP_PUB: the batch's publishers and their mesh neighbours."""
    mesh, cnt = ref["mesh"], ref["cnt"]
    rows = set()
    for x in np.unique(np.asarray(pubs)):
        rows.add(int(x))
        rows.update(int(y) & 0xFFFFFF for y in mesh[x, :cnt[x]])
    return np.array(sorted(rows))


@pytest.mark.parametrize("B", [1, 63, 64, 65, 129, 1024])
def test_emit_iterations_at_64_final_edges(monkeypatch, B):
    """One link class and one publisher: a row's B lanes are final in one window,
    so its emit loop runs ceil(B / 64) iterations with a full or a partly filled
    last one, in the publisher's neighbours (the body with the publisher) and in
    the other rows (the body without)."""
    monkeypatch.setenv("GS_REQUIRE_LPULL", "1")
    N = 300
    p = oracle.params(peers=N, seed=131, lazy_gossip=0)
    sched = _one_publisher(B, N)
    ref, _, _ = _both(p, 1, UNIFORM, sched, batch=B)
    marked = _marked_rows(ref, sched[1])
    plain = np.setdiff1d(np.arange(N), marked)
    assert len(marked) > 1 and len(plain) > 0
    fw = _finals_per_window(ref, sched, _window_ns(p, 1, UNIFORM))
    need = max(B - 1, 1)
    assert fw[marked].max() >= need and fw[plain].max() >= need, (fw[marked].max(), fw[plain].max())


def test_every_row_publishes(monkeypatch):
    """N = B = 128 and message m published by peer m: every row is marked, and
    every row is the publisher of one of its own lanes."""
    monkeypatch.setenv("GS_REQUIRE_LPULL", "1")
    N = B = 128
    p = oracle.params(peers=N, seed=132, lazy_gossip=0)
    t, _, size = _sched(B, N)
    sched = (t, np.arange(N), size)
    ref, _, _ = _both(p, 5, LINKS, sched, batch=B)
    assert len(_marked_rows(ref, sched[1])) == N


def test_one_publisher_of_the_largest_degree(monkeypatch):
    """All B messages from the peer with the most mesh neighbours: the most
    rows that exclude the same publisher from every lane's receivers."""
    monkeypatch.setenv("GS_REQUIRE_LPULL", "1")
    N, B = 300, 128
    p = oracle.params(peers=N, seed=133, lazy_gossip=0)
    sim, _ = gpu_sim(p, 5, LINKS, batch=B)
    _, cnt = sim.mesh()
    t, _, size = _sched(B, N)
    sched = (t, np.full(B, int(np.argmax(cnt))), size)
    ref, _, _ = _both(p, 5, LINKS, sched, batch=B)
    assert len(_marked_rows(ref, sched[1])) == 1 + int(cnt.max())


def test_marks_follow_the_batch(monkeypatch):
    """Three batches of 64 in one run, each with publishers of its own: some row
    is a publisher's neighbour in the first batch only and runs the body without
    the publisher afterwards (a mark left standing would be harmless, a mark
    missing in batch 2 or 3 would not: both directions exist)."""
    monkeypatch.setenv("GS_REQUIRE_LPULL", "1")
    N, B = 2000, 64
    p = oracle.params(peers=N, seed=134, lazy_gossip=0)
    t, _, size = _sched(3 * B, N)
    sched = (t, np.arange(3 * B) * 7 % N, size)  # 192 publishers, each once
    assert len(np.unique(sched[1])) == 3 * B
    ref, st, st2 = _both(p, 5, LINKS, sched, batch=B)
    assert st["batches"] == st2["batches"] == 3
    m = [_marked_rows(ref, sched[1][k * B:(k + 1) * B]) for k in range(3)]
    assert len(np.setdiff1d(m[0], np.union1d(m[1], m[2]))) > 0  # marked in batch 1 only
    assert len(np.setdiff1d(m[2], np.union1d(m[0], m[1]))) > 0  # marked in batch 3 only


def _rows_2_to_3_per_wave(parts=1):
    """N for which a wave of the list pass's grid owns 2 or 3 rows (four blocks of
    four waves per CU at this size, a row per wave and stride), N no multiple of
    the wave count: the first and last passes then have waves with 0 to 3 active
    rows. A part's grid is sized by the rows the part owns: N / parts of them."""
    waves = torch.cuda.get_device_properties(0).multi_processor_count * 16
    n = waves * 244 // 100
    if n % waves == 0:
        n += 1
    assert 2 * waves < n < 3 * waves
    return n * parts  # (10 000 on 256 CUs, less six, per part)


def test_row_pipeline_edges(monkeypatch):
    monkeypatch.setenv("GS_REQUIRE_LPULL", "1")
    N, B = _rows_2_to_3_per_wave(), 8
    _both(oracle.params(peers=N, seed=135, lazy_gossip=0), 5, LINKS, _sched(B, N), batch=B)


def test_row_pipeline_edges_with_gossip(monkeypatch):
    """The same rows with a heartbeat 370 ms after every publish: IHAVE / IWANT inside the passes."""
    monkeypatch.setenv("GS_REQUIRE_LPULL", "1")
    N, B = _rows_2_to_3_per_wave(), 8
    p = oracle.params(peers=N, seed=135, hb_phase_ns=_phase(370))
    _, st, st2 = _both(p, 5, LINKS, _sched(B, N), batch=B, on_list=False)
    # every batch took its gossip inside the list pass. A batch whose eager run is found to need
    # gossip runs the list pass twice (gossip_fallback_batches counts the discarded eager run, not a
    # run off the list pass: GS_REQUIRE_LPULL fails any such run)
    for x in (st, st2):
        assert x["gossip_list_batches"] == x["batches"] > 0, x
        assert x["list_pull_batches"] >= x["batches"], x


def test_row_pipeline_edges_in_two_parts(monkeypatch):
    """Two loop-back parts of that many rows each: the next row's record offsets are gathered with its counts."""
    monkeypatch.setenv("GS_REQUIRE_LPULL", "1")
    N, B = _rows_2_to_3_per_wave(parts=2), 8
    p = oracle.params(peers=N, seed=135, lazy_gossip=0)
    sched = _sched(B, N)
    ref = oracle.simulate(p, 5, LINKS, sched=sched)
    for collect in (True, False):
        sims = []
        for i in range(2):
            s = gossipsim.Simulator(batch=B, **_knobs(p))
            s.set_topogen_links(5, *LINKS)
            s.connect_gossipsub_peers()
            s.mesh_converge()
            s.set_partition(2, i)
            sims.append(s)
        comm = gossipsim.Comm(local_parts=2)
        res = comm.run_partitioned(sims, sched, collect=collect)
        if collect:
            _first_diff("t_complete", np.concatenate([r["t_complete"] for r in res], axis=1), ref["t_complete"])
            _first_diff("hops", np.concatenate([r["hops"] for r in res], axis=1), ref["hops"])
        st = [s.stats() for s in sims]
        for k in COUNTERS:
            if k == "latency_max_ms":
                assert max(x[k] for x in st) == ref["stats"][k], k
            elif k == "messages":
                assert all(x[k] == ref["stats"][k] for x in st), k
            else:
                assert sum(x[k] for x in st) == ref["stats"][k], k
        assert all(x["list_pull_batches"] == x["batches"] > 0 for x in st)
        comm.close()


@pytest.mark.parametrize("B", [512, 1024])
def test_rows_of_8_and_16_chunks(monkeypatch, B):
    """Rows of 512 lanes (CH = 8, six waves per SIMD) and of 1024 (CH = 16, four)."""
    monkeypatch.setenv("GS_REQUIRE_LPULL", "1")
    N = 300
    _both(oracle.params(peers=N, seed=136, lazy_gossip=0), 5, LINKS, _sched(B, N), batch=B)
