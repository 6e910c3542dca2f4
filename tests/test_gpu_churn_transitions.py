"""Churn batch path transitions against the CPU oracle.

A churn run carries the epoch ring, the table-set parity, the saved counters
and the chain ahead (gs_run.h Ahead) from one batch to the next, and a
batch takes one of three paths:

  L  the churn list pass;
  F  the list pass starts, a candidate list overflows and the batch re-runs on
     the push path (forced for single batches: GS_LPULL_CAP=3 with
     GS_LPULL_CAP_BATCHES);
  P  the list pass refuses the batch from the start (2 MB messages, whose
     uplink serialisation outlasts a heartbeat): the push path.

Every sequence here is bit-exact against the oracle (CSR, mesh, epochs,
t_complete, hops, the eight counters; integer equality only) and asserts the
exact number of batches and of list-pass batches, so a forced fallback that
did not happen, or an L batch that fell back, fails. The oracle's result
depends on the schedule alone: one oracle run per (params, schedule), shared
by the path variants. Shape: 900 peers, batches of 40 one-per-heartbeat
publishes, the smallest at which the ring wraps between back-to-back batches
(R = batch + horizon + 1 = 51 slots)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import gossipsim
import oracle

pytestmark = pytest.mark.gpu

T0 = gossipsim.T0_NS
N, STAGES, LINKS, BATCH = 900, 5, (50, 150, 40, 130), 40
HB = 400_000_000
BIG = 2_000_000  # bytes: a P batch
COUNTERS = ("deliveries", "frag_deliveries", "relaxations", "bytes_alg", "latency_sum_ms", "latency_max_ms",
            "messages", "gossip_iwant")
ENV_KNOBS = ("GS_LPULL_CAP", "GS_LPULL_CAP_BATCHES", "GS_REQUIRE_LPULL", "GS_CHN_PIPE")


def _params(gossip=1, frags=1, seed=59):
    return oracle.params(peers=N, seed=seed, churn_ppm=30000, lazy_gossip=gossip, fragments=frags, heartbeat_ns=HB,
                         churn_down=6, churn_horizon=10, hb_phase_ns=T0 - 30 * HB + 150_000_000)


def _lockstep(seq):
    """One publish per heartbeat, 40 per letter of seq; a P batch's messages are 2 MB
    (batches are cut at a size change)."""
    M = BATCH * len(seq)
    t = T0 + np.arange(M, dtype=np.uint64) * np.uint64(HB)
    size = np.repeat([BIG if x == "P" else 15000 for x in seq], BATCH)
    sched = (t, (6 + np.arange(M)) % N, size)
    return sched, [np.arange(k * BATCH, (k + 1) * BATCH) for k in range(len(seq))]


def _nonlockstep():
    """test_nonlockstep_churn_delay_on_list_pass's schedule: publishes 1.5 heartbeats
    apart, regrouped into two offset-class batches (run order: ascending offset)."""
    M = 40
    t = T0 + np.arange(M, dtype=np.uint64) * np.uint64(600_000_000)
    sched = (t, (6 + np.arange(M)) % N, np.full(M, 15000))
    off = (t - np.uint64(_params().hb_phase_ns)) % np.uint64(HB)
    return sched, [np.flatnonzero(off == o) for o in np.unique(off)]


_REF = {}


def _ref(key, p, sched):
    """The oracle's result of (params, schedule): computed once, shared, never written."""
    if key not in _REF:
        ref = oracle.simulate(p, STAGES, LINKS, sched=sched)
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REF[key] = ref
    return _REF[key]


def _sim(p, batch, ref=None):
    kw = {n: getattr(p, n) for n, _ in oracle.OrParams._fields_}
    kw["batch"] = batch
    sim = gossipsim.Simulator(**kw)
    sim.set_topogen_links(STAGES, *LINKS)
    sim.connect_gossipsub_peers()
    ep = sim.mesh_converge(400)
    if ref is not None:  # as test_gpu_parity.compare
        row, col, flags = sim.csr()
        np.testing.assert_array_equal(row, ref["row_ptr"], err_msg="row_ptr")
        np.testing.assert_array_equal(col, ref["col"], err_msg="col")
        mesh, cnt = sim.mesh()
        np.testing.assert_array_equal(cnt, ref["cnt"], err_msg="mesh count")
        np.testing.assert_array_equal(mesh, ref["mesh"], err_msg="mesh")
        np.testing.assert_array_equal(flags, ref["flags"], err_msg="flags")
        assert ep == ref["epochs"]
    return sim


def _first_bad_batch(res, ref, batches):
    """(index of the first batch whose t_complete or hops differ, a description), or None."""
    for k, idx in enumerate(batches):
        for name in ("t_complete", "hops"):
            a, b = np.asarray(res[name])[idx], ref[name][idx]
            if not np.array_equal(a, b):
                bad = np.argwhere(a != b)
                return k, "%s differs first in batch %d (messages %d..%d): %d of %d entries, first at message %d peer %d" % (
                    name, k, idx[0], idx[-1], len(bad), a.size, idx[bad[0][0]], bad[0][1])
    return None


def _check(res, st, ref, batches, n_list, gossip):
    bad = _first_bad_batch(res, ref, batches)
    print("stats:", {k: st[k] for k in ("batches", "list_pull_batches") + COUNTERS}, "first bad batch:", bad)
    assert st["batches"] == len(batches), st
    assert st["list_pull_batches"] == n_list, st
    assert bad is None, bad[1]
    np.testing.assert_array_equal(res["t_complete"], ref["t_complete"], err_msg="t_complete")
    np.testing.assert_array_equal(res["hops"], ref["hops"], err_msg="hops")
    for k in COUNTERS:
        assert st[k] == ref["stats"][k], k
    if gossip:
        assert st["gossip_iwant"] > 0


def _force(monkeypatch, forced, pipe=None):
    """GS_LPULL_CAP=3 on the batches of `forced` (run order), every other test knob unset."""
    for k in ENV_KNOBS:
        monkeypatch.delenv(k, raising=False)
    if forced:
        monkeypatch.setenv("GS_LPULL_CAP", "3")
        monkeypatch.setenv("GS_LPULL_CAP_BATCHES", ",".join(str(k) for k in forced))
    if pipe is not None:
        monkeypatch.setenv("GS_CHN_PIPE", pipe)


def _forced_of(seq):
    return [k for k, x in enumerate(seq) if x == "F"]


def _ref_key(seq, gossip, frags):
    return ("lockstep", gossip, frags, tuple(x == "P" for x in seq))


@pytest.mark.parametrize("seq,gossip,frags,pipe", [
    ("FLL", 1, 1, None), ("FLL", 0, 1, None),  # a list-pass batch prepared ahead, after a fallback
    ("LFL", 1, 1, None), ("LFL", 0, 1, None),  # the batch that falls back was itself prepared ahead
    ("LLF", 1, 1, None),  # the fallback on the last batch: no chain ahead to join
    ("FFL", 1, 1, None),
    ("FLFL", 1, 1, None),
    ("LPL", 1, 1, None),  # no chain ahead for the P batch; the third prepares in line after a push batch
    ("PLL", 1, 1, None),
    ("FPL", 1, 1, None),  # the push batch after a replay finds its ELL snapshots and in-lists rebuilt
    ("LFP", 1, 1, None),
    ("FLL", 1, 1, "0"),  # control: without the chain ahead the replay precedes batch 1's own churn_ring
    ("FL", 1, 2, None),  # fragment groups on the churn list pass
])
def test_churn_path_sequence(monkeypatch, seq, gossip, frags, pipe):
    """Back-to-back churn batches on the paths of `seq`, bit-exact against the
    oracle with exactly len(seq) batches, the L ones (only) on the list pass.

    Before the prepared batch was dropped on a replaying fallback, FLL, LFL
    (gossip on and off), FLFL and FL with 2 fragments differed from the oracle
    at batch index 1, 2, 1 and 1: the first list-pass batch after a fallback,
    whose seeds read ring slots the replay had overwritten."""
    p = _params(gossip, frags)
    sched, batches = _lockstep(seq)
    ref = _ref(_ref_key(seq, gossip, frags), p, sched)
    _force(monkeypatch, _forced_of(seq), pipe)
    sim = _sim(p, BATCH, ref)
    res = sim.run(sched)
    _check(res, sim.stats(), ref, batches, seq.count("L"), gossip)
    sim.close()


@pytest.mark.parametrize("gossip", [1, 0])
def test_nonlockstep_churn_fallback_then_list_pass(monkeypatch, gossip):
    """Two offset-class batches over the same epochs: class batch 0 falls back
    to the push path, class batch 1 stays on the list pass and builds its tables
    from a ring the fallback left current."""
    p = _params(gossip, seed=83)
    sched, batches = _nonlockstep()
    ref = _ref(("nonlockstep", gossip), p, sched)
    _force(monkeypatch, [0])
    sim = _sim(p, 64, ref)
    res = sim.run(sched)
    _check(res, sim.stats(), ref, batches, 1, gossip)
    sim.close()


@pytest.mark.parametrize("order", ["forced_first", "clean_first"])
def test_two_runs_on_one_simulator(monkeypatch, order):
    """A run whose last batch fell back and a run on the list pass alone, one
    after the other on one Simulator in either order: the second run starts
    from the ring, mesh state and table parity the first one left, and both
    equal the oracle's result of the schedule."""
    p = _params()
    sched, batches = _lockstep("LF")
    ref = _ref(_ref_key("LF", 1, 1), p, sched)
    for k in ENV_KNOBS:
        monkeypatch.delenv(k, raising=False)
    sim = _sim(p, BATCH, ref)
    for forced in ([1], []) if order == "forced_first" else ([], [1]):
        _force(monkeypatch, forced)
        sim.reset_stats()
        res = sim.run(sched)
        _check(res, sim.stats(), ref, batches, 2 - len(forced), 1)
    sim.close()


def _child(out):
    """FLL in a process of its own (test_fallback_after_chain_ahead_is_reached)."""
    sched, _ = _lockstep("FLL")
    sim = _sim(_params(), BATCH)
    res = sim.run(sched)
    st = sim.stats()
    np.savez(out, t_complete=res["t_complete"], hops=res["hops"], keys=np.array(sorted(st)),
             vals=np.array([st[k] for k in sorted(st)], np.uint64))


def test_fallback_after_chain_ahead_is_reached(tmp_path):
    """The FLL case in a fresh process with GS_DEBUG_AHEAD (read once per
    process): batch 40..80's chain started and was enqueued beside batch 0's
    passes before batch 0 fell back, the fallback dropped the prepared batch
    (its ring slots were replayed over), and the run equals the oracle."""
    out = str(tmp_path / "fll.npz")
    env = {k: v for k, v in os.environ.items() if k not in ENV_KNOBS}
    env.update(GS_DEBUG_AHEAD="1", GS_LPULL_CAP="3", GS_LPULL_CAP_BATCHES="0")
    code = ("import sys; sys.path[:0] = %r; import test_gpu_churn_transitions as T; T._child(sys.argv[1])"
            % [os.path.dirname(os.path.abspath(__file__)), os.path.dirname(oracle.__file__),
               os.path.dirname(gossipsim.__file__)])
    r = subprocess.run([sys.executable, "-c", code, out], env=env, timeout=120, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True)
    print(r.stderr)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stderr.splitlines()
    started = [i for i, x in enumerate(lines) if re.match(r"\[ah\] batch 40\.\.80: chain to epoch \d+", x)]
    enqueued = [i for i, x in enumerate(lines) if re.match(r"\[ah\] batch 40: chain enqueued \(\d+ epochs\)", x)]
    dropped = [i for i, x in enumerate(lines) if re.match(r"\[ah\] batch 40: dropped", x)]
    assert len(started) == 1 and len(enqueued) == 1 and len(dropped) == 1, lines
    assert started[0] < enqueued[0] < dropped[0]
    sched, batches = _lockstep("FLL")
    ref = _ref(_ref_key("FLL", 1, 1), _params(), sched)
    z = np.load(out)
    st = dict(zip((str(k) for k in z["keys"]), (int(v) for v in z["vals"])))
    _check(dict(t_complete=z["t_complete"], hops=z["hops"]), st, ref, batches, 2, 1)
