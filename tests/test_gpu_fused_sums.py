"""Counters-only batches on the no-log list pass (k_lpull<1, CH, .., NOLOG>,
DESIGN.md §4.6 round 9): the passes write no final log and add the deliveries,
the latency sum and maximum themselves; the lazy gossip no-op proof of a
lockstep batch reads the batch's deliveries and latest final time from two
words kept beside the pass control slots.

A default counters-only run (sim.run(sched, collect=False)) is compared with
three references that take other ways: the same run with GS_LPULL_SUM=0 (the
final log and k_lsum), the same run with GS_LPULL_DENSE=1 (dense rows,
k_complete), and values derived from the rows of a collect=True run, which
compare() checks against the CPU oracle. All compared values are integers and
must be equal. GS_SLICES=0 except where stated (test_gpu_counters_only's
helpers set it).

The 2^38 ns bound (a final time at which the passes' 32-bit ms would differ
from k_lsum's: the batch is run again with its log) has no test: no public
knob reaches it on the list pass at a small shape. A window must stay below
2^32 ns (latency + serialisation of the fastest link), so a hop costs at most
a few seconds, and the sparsest meshes that still deliver (d = 2, 1200 to 2500
peers, 4.2 s links, 4.2 s serialisation, which the list pass refuses anyway)
end at 245 to 274.5 s in the oracle, under 2^38 ns = 274.88 s."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import gossipsim
import oracle
from test_gpu_counters_only import HB, HETERO, KEYS, PHASES, UNIFORM, _counters, _env, _from_rows, _phase_params
from test_gpu_parity import T0, _sched, compare, gpu_sim

pytestmark = pytest.mark.gpu
NOLOG_LINE = re.compile(r"\[lp\] batch (\d+): completion in-pass \(no log\)")
ANY_LINE = re.compile(r"\[lp\] batch (\d+): completion (.*)")


def _three(p, links, scheds, batch, **env):
    """Stats of the default run and of its two references (log + k_lsum, dense rows)."""
    new = _counters(p, links, scheds, batch, False, **env)
    log = _counters(p, links, scheds, batch, False, GS_LPULL_SUM="0", **env)
    dense = _counters(p, links, scheds, batch, True, **env)
    return new, log, dense


def _assert_equal(new, refs, keys=KEYS):
    for k in keys:
        print(k, new[k], [r[k] for r in refs])
    for k in keys:
        for r in refs:
            assert new[k] == r[k], k


@pytest.mark.parametrize("links", [HETERO, UNIFORM], ids=["hetero", "uniform"])
@pytest.mark.parametrize("gossip", [0, 1])
@pytest.mark.parametrize("N,M,B", [(1300, 64, 16), (700, 640, 640)], ids=["ch8", "ch16"])
def test_nolog_equals_log_dense_and_rows(N, M, B, gossip, links):
    """Both instantiations of the no-log pass (rows of <= 512 lanes: 8 chunks;
    640 lanes: 16), with and without lazy gossip, on both link sets."""
    p = oracle.params(peers=N, seed=410 + gossip, lazy_gossip=gossip)
    sched = _sched(M, N)
    new, log, dense = _three(p, links, [sched], B)
    _assert_equal(new, (log, dense))
    with _env():
        sim, res = compare(p, links[0], links[1], sched, batch=B)
        sim.close()
    d, s, mx = _from_rows(res["t_complete"], sched)
    print("rows", d, s, mx)
    assert (new["deliveries"], new["latency_sum_ms"], new["latency_max_ms"]) == (d, s, mx)
    assert new["deliveries"] == M * (N - 1)


@pytest.fixture(scope="module")
def phase_reference():
    """The logged run (GS_LPULL_SUM=0) and the dense-path run of every phase, once."""
    sched = _sched(32, 1200)
    return {ms: (_counters(_phase_params(ms), HETERO, [sched], 8, False, GS_LPULL_SUM="0"),
                 _counters(_phase_params(ms), HETERO, [sched], 8, True)) for ms in PHASES}


def test_proof_reference_has_both_outcomes(phase_reference):
    """The phases lie on both sides of the no-op proof's threshold, in both references."""
    for which in (0, 1):
        noop = [ms for ms in PHASES if phase_reference[ms][which]["gossip_noop_msgs"] == 32]
        fail = [ms for ms in PHASES if phase_reference[ms][which]["gossip_fallback_batches"] > 0]
        print("proof holds at", noop, "fails at", fail)
        assert noop and fail


@pytest.mark.parametrize("ms", PHASES)
def test_proof_decides_as_references(phase_reference, ms):
    """The proof from the two batch words decides as k_lsum's and the dense
    path's at every phase; after a failed proof (counters restored, the batch
    run again with the gossip) the counters are equal too."""
    new = _counters(_phase_params(ms), HETERO, [_sched(32, 1200)], 8, False)
    _assert_equal(new, phase_reference[ms])


@pytest.mark.parametrize("gossip", [0, 1])
def test_list_overflow_restores_counters(gossip):
    """Lists capped at 3 entries: the no-log pass has added to the delivery and
    latency counters by the time it overflows; they are restored and the batch
    re-runs on k_pull with the uncapped run's stats."""
    N, M = 1200, 64
    p = oracle.params(peers=N, seed=430, lazy_gossip=gossip)
    sched = _sched(M, N)
    cap = _counters(p, HETERO, [sched], M, False, GS_LPULL_CAP="3")
    new = _counters(p, HETERO, [sched], M, False)
    for k in KEYS:
        print(k, cap[k], new[k])
    assert cap["list_pull_batches"] == 0 and new["list_pull_batches"] >= 1
    for k in KEYS:
        if k != "list_pull_batches":
            assert cap[k] == new[k], k
    assert new["deliveries"] == M * (N - 1)


def test_state_between_runs_on_one_context():
    """Counters-only, rows, counters-only, and one more counters-only run on one
    context without reset_stats: the rows equal the oracle's (no stale "no log"
    state), sums and maximum the dense path's (no stale batch words)."""
    N, M, B = 1000, 16, 8
    p = oracle.params(peers=N, seed=450)
    a = _sched(M, N)
    b = (a[0] + np.uint64(40 * HB), (a[1] + 500) % N, a[2])
    ref = oracle.simulate(p, HETERO[0], HETERO[1], sched=a)
    stats = {}
    for dense in (False, True):
        with _env(GS_LPULL_DENSE="1" if dense else None):
            sim, _ = gpu_sim(p, HETERO[0], HETERO[1], batch=B)
            sim.run(a, collect=False)
            res = sim.run(a)
            np.testing.assert_array_equal(res["t_complete"], ref["t_complete"], err_msg="t_complete")
            np.testing.assert_array_equal(res["hops"], ref["hops"], err_msg="hops")
            sim.run(a, collect=False)
            sim.run(b, collect=False)
            stats[dense] = sim.stats()
            sim.close()
    _assert_equal(stats[False], (stats[True],), KEYS + ("messages", "batches"))
    assert stats[False]["deliveries"] == 4 * M * (N - 1)
    d, s, mx = _from_rows(ref["t_complete"], a)
    assert stats[False]["latency_max_ms"] >= mx and d == M * (N - 1)


def test_several_batches_per_run():
    """Four batches in one run: the batch words start from zero in every batch
    (each proof holds or fails on its own batch), the counters accumulate."""
    N = 1000
    p = oracle.params(peers=N, seed=440)
    sched = _sched(32, N)
    new, log, dense = _three(p, HETERO, [sched], 8)
    _assert_equal(new, (log, dense), KEYS + ("messages", "batches"))
    assert new["batches"] == 4 and new["deliveries"] == 32 * (N - 1)
    assert new["gossip_noop_msgs"] + 8 * new["gossip_fallback_batches"] == 32


# ---- the host rule, seen through GS_DEBUG_COMPLETION in a fresh process ----
RULE_N, RULE_M, RULE_B = 1000, 16, 8


def _rule_cases():
    """name -> (params, links, schedule, run kwargs, env, takes the no-log form)."""
    N, M = RULE_N, RULE_M
    s = _sched(M, N)
    late = (T0 + np.arange(M, dtype=np.uint64) * np.uint64(1_500_000_000), (6 + np.arange(M)) % N, np.full(M, 15000))
    base = oracle.params(peers=N, seed=460)
    return {
        "default": (base, HETERO, s, {}, {}, True),
        "default_no_gossip": (oracle.params(peers=N, seed=460, lazy_gossip=0), HETERO, s, {}, {}, True),
        "knob_off": (base, HETERO, s, {}, {"GS_LPULL_SUM": "0"}, False),
        "sink": (base, HETERO, s, {"collect": True}, {}, False),
        "on_lat": (base, HETERO, s, {"on_lat": True}, {}, False),
        "fragments8": (oracle.params(peers=N, seed=460, fragments=8), HETERO, s, {}, {}, False),
        "go_preset": (oracle.params_for("go", peers=N, seed=460), HETERO, s, {}, {}, False),
        "churn": (oracle.params(peers=N, seed=460, churn_ppm=30000, churn_down=6, churn_horizon=10,
                                hb_phase_ns=T0 - 30 * HB + 150_000_000), HETERO, s, {}, {}, False),
        "slices": (base, HETERO, s, {}, {"GS_SLICES": None}, False),
        "nonlockstep": (oracle.params(peers=N, seed=460, hb_phase_ns=(T0 + 120_000_000) % HB), HETERO, late, {},
                        {"GS_CLASS_SPLIT": "0"}, False),
    }


def _run_case(case, dense):
    p, links, sched, kw, env, _ = case
    kw = dict(kw)
    if kw.pop("on_lat", False):
        kw["on_lat"] = lambda first, lat: None
    kw.setdefault("collect", False)
    with _env(GS_LPULL_DENSE="1" if dense else None, **env):
        sim, _ = gpu_sim(p, links[0], links[1], batch=RULE_B)
        sim.run(sched, **kw)
        st = sim.stats()
        sim.close()
    return st


def _child(out):
    """Every case of the host rule, one after the other, with a marker line on stderr."""
    res = {}
    for name, case in _rule_cases().items():
        sys.stderr.write("[case] %s\n" % name)
        sys.stderr.flush()
        st = _run_case(case, False)
        res[name] = np.array([st[k] for k in KEYS], np.uint64)
    np.savez(out, **res)


@pytest.fixture(scope="module")
def rule_child(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("rule") / "rule.npz")
    env = {k: v for k, v in os.environ.items() if not k.startswith("GS_")}
    env["GS_DEBUG_COMPLETION"] = "1"
    code = ("import sys; sys.path[:0] = %r; import test_gpu_fused_sums as T; T._child(sys.argv[1])"
            % [os.path.dirname(os.path.abspath(__file__)), os.path.dirname(oracle.__file__),
               os.path.dirname(gossipsim.__file__)])
    r = subprocess.run([sys.executable, "-c", code, out], env=env, timeout=300, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True)
    print(r.stderr)
    assert r.returncode == 0, r.stderr[-2000:]
    lines, cur = {}, None
    for x in r.stderr.splitlines():
        if x.startswith("[case] "):
            cur = x[7:]
            lines[cur] = []
        elif cur is not None and ANY_LINE.match(x):
            lines[cur].append(x)
    z = np.load(out)
    return lines, {k: dict(zip(KEYS, (int(v) for v in z[k]))) for k in z.files}


@pytest.mark.parametrize("name", list(_rule_cases()))
def test_host_rule(rule_child, name):
    """The no-log form is taken exactly where nothing reads a per-message value
    and the batch is one the plain FP = 1 pass runs; every case equals the
    dense path's counters."""
    lines, stats = rule_child
    case = _rule_cases()[name]
    took = [x for x in lines[name] if NOLOG_LINE.match(x)]
    print(name, lines[name])
    if case[5] and case[0].lazy_gossip:
        # the first batch at least: after a failed proof the context's later batches go
        # straight to the gossip inside the passes, which keeps its log
        assert took and NOLOG_LINE.match(lines[name][0])
    elif case[5]:
        assert len(took) == len(lines[name]) == RULE_M // RULE_B
    else:
        assert not took
    ref = _run_case(case, True)
    _assert_equal(stats[name], (ref,))
