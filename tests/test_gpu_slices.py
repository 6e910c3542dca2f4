"""Batch slices (gs_run.h Run::try_slices / run_lpull_batch's Slices): several
full batches of one shape on a small graph run as ONE list pass over copies of
the graph (slice j's rows are j * N + peer). The results must be those of the
same batches run one at a time (GS_SLICES=0) and of the CPU oracle, for every
way a run hands results out (rows, streamed blocks, latency stream, summaries,
device-resident counters), with single- and multi-fragment rows and with lazy
gossip (the eager pass's no-op proof per slice, and a phase where the proof
fails and the group is re-run with the gossip inside its passes).

Reference: config #2 (BASELINE.json, shadow/README.md:57: 10k peers,
FRAGMENTS=8, 1000 messages); main.rs:101-143 / 228-235 for the rules the
oracle restates."""
import numpy as np
import pytest

import gossipsim
import oracle
from test_gpu_parity import T0, _sched, compare, gpu_sim

pytestmark = pytest.mark.gpu
LINKS = (50, 150, 40, 130)
HB = 1_000_000_000


def _run(monkeypatch, slices, p, sched, batch, how):
    monkeypatch.setenv("GS_SLICES", slices)
    sim, _ = gpu_sim(p, 5, LINKS, batch=batch)
    out = {}
    if how == "rows":
        res = sim.run(sched)
        out["t"], out["h"] = res["t_complete"], res["hops"]
    elif how == "summary":
        res = sim.run(sched, summary=True)
        out["t"] = res["t_complete"]
        out.update({"summary_" + k: v for k, v in res["summary"].items()})
    elif how == "lat":
        got = []
        sim.run(sched, collect=False, on_lat=lambda first, lat: got.append((first, lat.copy())), block_msgs=7)
        out["lat"] = np.concatenate([x for _, x in sorted(got, key=lambda y: y[0])])
    else:
        sim.run(sched, collect=False)
    st = sim.stats()
    sim.close()
    return out, st


KEYS = ("deliveries", "frag_deliveries", "relaxations", "latency_sum_ms", "latency_max_ms", "messages", "batches",
        "gossip_iwant", "list_pull_batches")


@pytest.mark.parametrize("frags,gossip,how", [
    (1, 0, "rows"), (1, 1, "rows"), (8, 1, "rows"), (1, 1, "none"), (4, 0, "lat"), (1, 1, "lat"),
    (2, 1, "summary")])
def test_slices_equal_single_batches(monkeypatch, frags, gossip, how):
    """8 batches of 16 messages at 1500 peers: one sliced pass (8 copies of the
    graph) equals the 8 single batches bit for bit, with fewer window passes."""
    p = oracle.params(peers=1500, seed=300 + frags, fragments=frags, lazy_gossip=gossip)
    sched = _sched(128, 1500)
    a, sa = _run(monkeypatch, "", p, sched, 16, how)
    b, sb = _run(monkeypatch, "0", p, sched, 16, how)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    for k in KEYS:
        assert sa[k] == sb[k], k
    assert sa["batches"] == 8 and sa["list_pull_batches"] == 8


def test_slices_fewer_passes_with_timing(monkeypatch):
    """The sliced group runs its passes once for all its batches."""
    p = oracle.params(peers=1200, seed=310, fragments=1)
    sched = _sched(64, 1200)
    launches = {}
    for env in ("", "0"):
        monkeypatch.setenv("GS_SLICES", env)
        sim, _ = gpu_sim(p, 5, LINKS, batch=16)
        sim.set_timing(True)
        sim.run(sched, collect=False)
        launches[env] = sim.stats()["relax_launches"]
        sim.close()
    assert launches[""] * 2 < launches["0"]


@pytest.mark.parametrize("frags", [1, 8])
def test_slices_against_oracle(monkeypatch, frags):
    """A sliced run (3 slices of 10 + a single batch of the rest) equals the oracle."""
    monkeypatch.setenv("GS_SLICES", "")
    p = oracle.params(peers=900, seed=320 + frags, fragments=frags)
    compare(p, 5, LINKS, _sched(37, 900), batch=10)


def test_slices_gossip_phase_falls_back_exactly(monkeypatch):
    """Heartbeats 120 ms after every publish: IWANTs change the result, the
    group's no-op proof fails and the group runs again with the IHAVE / IWANT
    inside its passes — still the oracle's result; the discarded eager run
    counts once as a fallback."""
    monkeypatch.setenv("GS_SLICES", "")
    p = oracle.params(peers=1200, seed=330, hb_phase_ns=(T0 + 120_000_000) % HB)
    sim, _ = compare(p, 5, LINKS, _sched(32, 1200), batch=8)
    st = sim.stats()
    # the group's eager pass fails its proof (one fallback), then the group runs its gossip
    # inside its passes
    assert st["gossip_iwant"] > 0 and st["batches"] == 4
    assert st["gossip_fallback_batches"] == 1 and st["gossip_list_batches"] == 4


def test_slices_c2_shape_bench_path(monkeypatch):
    """bench.py's config #2 shape (10k peers, F = 8, 128-message batches) on a
    quarter of its messages: device-resident counters equal the single-batch run."""
    p = oracle.params(peers=10_000, seed=1, fragments=8)
    sched = gossipsim.shard_messages(1, 0, 1, 256, 10_000, 15000)
    _, sa = _run(monkeypatch, "", p, sched, 128, "none")
    _, sb = _run(monkeypatch, "0", p, sched, 128, "none")
    for k in KEYS:
        assert sa[k] == sb[k], k
    assert sa["gossip_noop_msgs"] == 256


@pytest.mark.parametrize("frags,slices", [(2, "0"), (8, "0"), (8, ""), (3, "")])
def test_fragment_groups_complete_from_logs(monkeypatch, frags, slices):
    """Fragmented batches complete from the final logs (k_lcomplete reduces each
    message's F fragment lanes: reassembly) unless a sink takes rows: the
    counters, the gossip no-op proof and the u16 latency stream equal the dense
    rows' k_complete (GS_LPULL_DENSE=1)."""
    p = oracle.params(peers=1300, seed=340 + frags, fragments=frags)
    sched = _sched(64, 1300)
    out = {}
    for dense in ("", "1"):
        monkeypatch.setenv("GS_LPULL_DENSE", dense)
        o, st = _run(monkeypatch, slices, p, sched, 16, "lat")
        _, st2 = _run(monkeypatch, slices, p, sched, 16, "none")
        out[dense] = (o["lat"], st, st2)
    np.testing.assert_array_equal(out[""][0], out["1"][0])
    for k in KEYS + ("gossip_noop_msgs",):
        assert out[""][1][k] == out["1"][1][k], k
        assert out[""][2][k] == out["1"][2][k], k
    assert out[""][2]["gossip_noop_msgs"] == 64


@pytest.mark.parametrize("frags,phase_ms", [(1, 55), (1, 30), (4, 120)])
def test_slices_gossip_active_equal_single_batches(monkeypatch, frags, phase_ms):
    """Gossip-active groups (the in-pass IHAVE / IWANT over slice rows: CSR and
    rng by the peer, planes and row-done bits by the slice row, each slice's
    heartbeat indices) equal the same batches run one at a time."""
    p = oracle.params(peers=1400, seed=350 + phase_ms, fragments=frags, hb_phase_ns=(T0 + phase_ms * 1_000_000) % HB)
    sched = _sched(96, 1400)
    a, sa = _run(monkeypatch, "", p, sched, 16, "rows")
    b, sb = _run(monkeypatch, "0", p, sched, 16, "rows")
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    # (which batches take the in-pass gossip may differ: a single batch can prove its gossip a no-op)
    for k in ("deliveries", "frag_deliveries", "relaxations", "latency_sum_ms", "latency_max_ms", "messages",
              "batches", "gossip_iwant"):
        assert sa[k] == sb[k], k
    assert sa["gossip_iwant"] > 0 and sa["gossip_list_batches"] >= 5


def test_slices_gossip_active_against_oracle(monkeypatch):
    monkeypatch.setenv("GS_SLICES", "")
    p = oracle.params(peers=1100, seed=360, fragments=2, hb_phase_ns=(T0 + 90_000_000) % HB)
    sim, _ = compare(p, 5, LINKS, _sched(40, 1100), batch=8)
    st = sim.stats()
    assert st["gossip_iwant"] > 0 and st["gossip_list_batches"] == 5


def test_slices_failed_proof_reruns_the_group_in_pass(monkeypatch):
    """The group whose eager no-op proof fails runs again as a group, with the
    gossip inside its passes, not as single batches: against the oracle both
    ways, the same fallback and in-pass counts, and fewer than half the window
    passes. (Passes of one batch: P1 eager, P2 >= P1 with the in-pass gossip's
    narrower windows; a group's pass count is a batch's. Sliced P1 + P2, single
    batches P1 + 4 * P2 > 2 * (P1 + P2).)"""
    p = oracle.params(peers=1200, seed=330, hb_phase_ns=(T0 + 120_000_000) % HB)
    sched = _sched(32, 1200)
    ref = oracle.simulate(p, 5, LINKS, sched=sched)
    launches = {}
    for env in ("", "0"):
        monkeypatch.setenv("GS_SLICES", env)
        sim, _ = compare(p, 5, LINKS, sched, batch=8, ref=ref)
        st = sim.stats()
        print(repr(env), {k: st[k] for k in ("batches", "gossip_fallback_batches", "gossip_list_batches",
                                             "list_pull_batches", "relax_launches")})
        assert st["batches"] == 4 and st["gossip_fallback_batches"] == 1 and st["gossip_list_batches"] == 4
        launches[env] = st["relax_launches"]
        sim.close()
    assert launches[""] * 2 < launches["0"]


def test_class_cuts_split_what_would_be_a_slice_group(monkeypatch):
    """Publishes 1.5 heartbeats apart with batches of 8: the class regrouping
    cuts every 8 messages into two lockstep batches of 4 (heartbeats 950 and
    450 ms after the publishes), and a slice group must not reach across a cut.
    On links of 10-50 ms every message is complete long before its first
    heartbeat, so every no-op proof holds and a group that ignored the cuts
    would succeed: the same schedule without the regrouping (GS_CLASS_SPLIT=0)
    does run as one group of 4 mixed slices, 4 batches. With the cuts: 8
    batches of 4, no full batch for a group. Both equal the oracle."""
    monkeypatch.setenv("GS_SLICES", "")
    monkeypatch.setenv("GS_REQUIRE_LPULL", "1")
    N, M, links = 1200, 32, (50, 150, 10, 50)
    p = oracle.params(peers=N, seed=370, hb_phase_ns=(T0 + 950_000_000) % HB)
    t = T0 + np.arange(M, dtype=np.uint64) * np.uint64(1_500_000_000)
    sched = (t, (6 + np.arange(M)) % N, np.full(M, 15000))
    ref = oracle.simulate(p, 5, links, sched=sched)
    for split, batches in (("", 8), ("0", 4)):
        monkeypatch.setenv("GS_CLASS_SPLIT", split)
        sim, _ = compare(p, 5, links, sched, batch=8, ref=ref)
        st = sim.stats()
        print(repr(split), {k: st[k] for k in ("batches", "messages", "gossip_noop_msgs", "gossip_fallback_batches",
                                               "list_pull_batches", "relax_launches", "latency_max_ms")})
        sim.close()
        assert st["gossip_noop_msgs"] == M and st["gossip_fallback_batches"] == 0
        assert st["batches"] == st["list_pull_batches"] == batches and st["messages"] == M
