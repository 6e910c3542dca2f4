"""Counters-only runs (gs_run without a sink, gossipsim.h: "device-resident
run, counters only") on the frozen-mesh eager list pass, the mode bench.py's
headline times: the counters and the lazy gossip no-op proof come from the
final logs, never from dense rows: from a stream over the logged keys alone
(k_lsum: batch-wide sums, and the proof of a lockstep batch from the batch's
deliveries and latest final time), or per message through k_lcomplete where
the batch is not lockstep.

Every test compares such a run (sim.run(sched, collect=False)) with references
that take another way: the same run with GS_LPULL_DENSE=1 (dense rows,
k_complete) and values derived from the rows of a collect=True run, checked
against the CPU oracle where compare() is used. All compared values are
integers and must be equal. The cases are those at which a batch-wide
completion could go wrong: both instantiations
of the pass, window starts that are no multiples of 1 ms, the proof on both
sides of its threshold, schedules that are not lockstep, the overflow re-run,
counters carried over batches and runs.

GS_SLICES=0 throughout: at these sizes several batches would otherwise run as
one sliced pass."""
import contextlib
import os

import numpy as np
import pytest

import oracle
from test_gpu_parity import T0, UND, _sched, compare, gpu_sim

pytestmark = pytest.mark.gpu
HETERO = (5, (50, 150, 40, 130))  # window starts and widths that are no multiples of 1 ms
UNIFORM = (1, (50, 50, 50, 50))
HB = 1_000_000_000
KEYS = ("deliveries", "frag_deliveries", "relaxations", "bytes_alg", "latency_sum_ms", "latency_max_ms",
        "gossip_noop_msgs", "gossip_fallback_batches", "gossip_list_batches", "list_pull_batches", "gossip_iwant")


@contextlib.contextmanager
def _env(**kv):
    """Environment for one run: value None removes the variable."""
    kv.setdefault("GS_SLICES", "0")
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _counters(p, links, scheds, batch, dense, **env):
    """Stats after counters-only runs of `scheds`, one after the other on one context."""
    with _env(GS_LPULL_DENSE="1" if dense else None, **env):
        sim, _ = gpu_sim(p, links[0], links[1], batch=batch)
        for sched in scheds:
            sim.run(sched, collect=False)
        st = sim.stats()
        sim.close()
    return st


def _from_rows(t_complete, sched):
    """(deliveries, latency sum, latency max) in whole ms from [M, N] completion times."""
    t_pub, pub, _ = sched
    lat = t_complete - np.asarray(t_pub, dtype=np.uint64)[:, None]
    ok = t_complete != UND
    ok[np.arange(len(pub)), np.asarray(pub)] = False  # the publisher's own key is no delivery
    ms = lat[ok] // np.uint64(1_000_000)
    return int(ok.sum()), int(ms.sum()), int(ms.max())


@pytest.mark.parametrize("links", [HETERO, UNIFORM], ids=["hetero", "uniform"])
@pytest.mark.parametrize("gossip", [0, 1])
@pytest.mark.parametrize("N,M,B", [(1300, 64, 16), (700, 640, 640)], ids=["ch8", "ch16"])
def test_counters_only_equals_dense_and_rows(N, M, B, gossip, links):
    """Both instantiations of the pass (rows of <= 512 lanes: 8 chunks; 640
    lanes: 16), with and without lazy gossip, on both link sets."""
    p = oracle.params(peers=N, seed=410 + gossip, lazy_gossip=gossip)
    sched = _sched(M, N)
    new = _counters(p, links, [sched], B, False)
    ref = _counters(p, links, [sched], B, True)
    for k in KEYS:
        print(k, new[k], ref[k])
    for k in KEYS:
        assert new[k] == ref[k], k
    with _env():
        sim, _ = gpu_sim(p, links[0], links[1], batch=B)
        res = sim.run(sched)
        sim.close()
    d, s, mx = _from_rows(res["t_complete"], sched)
    print("rows", d, s, mx)
    assert (new["deliveries"], new["latency_sum_ms"], new["latency_max_ms"]) == (d, s, mx)
    assert d == M * (N - 1)


PHASES = (None, 30, 55, 120, 370)  # heartbeats this many ms after every publish (None: hb_phase_ns 0)


def _phase_params(ms):
    kw = {} if ms is None else {"hb_phase_ns": (T0 + ms * 1_000_000) % HB}
    return oracle.params(peers=1200, seed=420, **kw)


@pytest.fixture(scope="module")
def phase_reference():
    """The dense-path run of every phase, once."""
    sched = _sched(32, 1200)
    return {ms: _counters(_phase_params(ms), HETERO, [sched], 8, True) for ms in PHASES}


def test_proof_reference_has_both_outcomes(phase_reference):
    """The phases below lie on both sides of the no-op proof's threshold."""
    noop = [ms for ms in PHASES if phase_reference[ms]["gossip_noop_msgs"] == 32]
    fail = [ms for ms in PHASES if phase_reference[ms]["gossip_fallback_batches"] > 0]
    print("proof holds at", noop, "fails at", fail)
    assert noop and fail


@pytest.mark.parametrize("ms", PHASES)
def test_proof_decides_as_dense_path(phase_reference, ms):
    """The no-op proof of a counters-only batch decides as the dense path's at
    every phase; the rows of the same configuration equal the oracle's."""
    p = _phase_params(ms)
    sched = _sched(32, 1200)
    new = _counters(p, HETERO, [sched], 8, False)
    ref = phase_reference[ms]
    for k in KEYS:
        print(k, new[k], ref[k])
    for k in KEYS:
        assert new[k] == ref[k], k
    with _env():
        compare(p, HETERO[0], HETERO[1], sched, batch=8)


@pytest.mark.parametrize("split", [None, "0"], ids=["classes", "one_batch"])
def test_nonlockstep_schedule(split):
    """Publishes 1.5 heartbeats apart (two offsets into the heartbeat): regrouped
    into one lockstep batch per offset class, or with GS_CLASS_SPLIT=0 one batch
    that is not lockstep (the per-message proof)."""
    N, M = 1500, 48
    p = oracle.params(peers=N, seed=81, hb_phase_ns=(T0 + 120_000_000) % HB)
    t = T0 + np.arange(M, dtype=np.uint64) * np.uint64(1_500_000_000)
    sched = (t, (6 + np.arange(M)) % N, np.full(M, 15000))
    new = _counters(p, HETERO, [sched], 64, False, GS_CLASS_SPLIT=split)
    ref = _counters(p, HETERO, [sched], 64, True, GS_CLASS_SPLIT=split)
    for k in KEYS:
        print(k, new[k], ref[k])
    for k in KEYS:
        assert new[k] == ref[k], k


@pytest.mark.parametrize("gossip", [0, 1])
def test_list_overflow_restores_counters(gossip):
    """Lists capped at 3 entries: the pass overflows, the counters are restored
    and the batch re-runs on k_pull; the stats are the uncapped run's."""
    N, M = 1200, 64
    p = oracle.params(peers=N, seed=430, lazy_gossip=gossip)
    sched = _sched(M, N)
    cap = _counters(p, HETERO, [sched], M, False, GS_LPULL_CAP="3")
    new = _counters(p, HETERO, [sched], M, False)
    for k in KEYS:
        print(k, cap[k], new[k])
    assert cap["list_pull_batches"] == 0 and new["list_pull_batches"] >= 1  # the capped batch went to k_pull
    for k in KEYS:
        if k != "list_pull_batches":
            assert cap[k] == new[k], k


def test_counters_accumulate_over_batches_and_runs():
    """4 batches in one run, then a second run on the same context without
    reset_stats: sums and maximum equal the dense path's."""
    N = 1000
    p = oracle.params(peers=N, seed=440)
    a = _sched(32, N)
    b = (a[0] + np.uint64(40 * HB), (a[1] + 500) % N, a[2])
    new = _counters(p, HETERO, [a, b], 8, False)
    ref = _counters(p, HETERO, [a, b], 8, True)
    for k in KEYS + ("messages", "batches"):
        print(k, new[k], ref[k])
    for k in KEYS + ("messages", "batches"):
        assert new[k] == ref[k], k
    assert new["batches"] == 8 and new["deliveries"] == 64 * (N - 1)
