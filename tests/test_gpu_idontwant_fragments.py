"""Fragmented IDONTWANT batches (the go preset: FRAGMENTS > 1 and IDONTWANT
for fragments >= 1000 B, go-test-node/env.go:29, main.go:70-73,165) on the
list pass: rows of fragment groups with dense final keys, every fragment lane
tested against the same lane of each mesh neighbour (k_lpull<FP, CH, true>,
gs_lpull_kernel.h). Bit-exact against the CPU oracle, whose
rule is per fragment (gs_oracle.c: best[w][f] + lat(w -> u) <= t), at every
fragment width, both chunk counts, with lazy gossip inside the passes, after a
list overflow, between batches without IDONTWANT, with per-peer traffic and
through the latency stream. GS_IDW_FRAG_LIST=0 keeps such batches on the push
path (the behaviour before this path existed)."""
import functools

import numpy as np
import pytest

import gossipsim
import oracle
from test_gpu_features import _logged_ms
from test_gpu_gossip_list import _phase
from test_gpu_parity import _sched, compare, gpu_sim

pytestmark = pytest.mark.gpu
LINKS = (50, 150, 40, 130)

# F -> (message size, batch, messages, peers): L = batch * FP covers one 64-lane
# chunk, rows of <= 512 lanes (8 chunks) and of 1024 lanes (16 chunks). 16
# fragments of 15000 B fall below the 1000-B threshold, hence 32000 B.
EAGER = {2: (15000, 8, 20, 1500), 3: (15000, 16, 16, 1500), 4: (15000, 64, 64, 1500),
         8: (15000, 128, 128, 2000), 16: (32000, 64, 64, 2000)}


def _go(frags, peers, **kw):
    kw.setdefault("seed", 62)
    return oracle.params_for("go", peers=peers, fragments=frags, **kw)


@functools.lru_cache(maxsize=None)
def _eager_ref(frags, idontwant=None):
    """The oracle's run of an EAGER shape (shared by the tests, never modified)."""
    size, _, M, N = EAGER[frags]
    kw = dict(lazy_gossip=0)
    if idontwant is not None:
        kw["idontwant"] = idontwant
    return oracle.simulate(_go(frags, N, **kw), 5, LINKS, sched=_sched(M, N, size=size))


def _eager(frags):
    size, B, M, N = EAGER[frags]
    sim, res = compare(_go(frags, N, lazy_gossip=0), 5, LINKS, _sched(M, N, size=size), batch=B, ref=_eager_ref(frags))
    return sim, res


@pytest.mark.parametrize("frags", [2, 3, 4, 8, 16])
def test_fragmented_idontwant_on_list_pass(monkeypatch, frags):
    """Every fragment width (FP = 2, 4 with and without a padding lane, 8, 16)
    with rows of 16, 64, 256 and 1024 lanes: each batch runs on the list pass
    (GS_REQUIRE_LPULL: no other path may take it), bit-exact, and IDONTWANT
    really suppresses sends there (fewer relaxations than the oracle's run of
    the same schedule without IDONTWANT)."""
    monkeypatch.setenv("GS_REQUIRE_LPULL", "1")
    sim, _ = _eager(frags)
    st = sim.stats()
    assert st["list_pull_batches"] == st["batches"] > 0
    assert st["relaxations"] < _eager_ref(frags, idontwant=0)["stats"]["relaxations"]


@pytest.mark.parametrize("frags", [8, 3])
@pytest.mark.parametrize("path", ["list", "push"])
def test_fragmented_idontwant_list_equals_push(monkeypatch, path, frags):
    """The same batches on the list pass and, with GS_IDW_FRAG_LIST=0, on the
    push path: both equal the oracle (and so each other)."""
    if path == "push":
        monkeypatch.setenv("GS_IDW_FRAG_LIST", "0")
    sim, _ = _eager(frags)
    st = sim.stats()
    if path == "list":
        assert st["list_pull_batches"] >= 1
    else:
        assert st["list_pull_batches"] == 0


@pytest.mark.parametrize("frags,phase_ms", [(2, 120), (8, 120), (4, 250), (8, 370)])
def test_fragmented_idontwant_gossip_in_list_pass(frags, phase_ms):
    """Lazy gossip on (the go preset's default) with a heartbeat landing
    mid-dissemination (120, 250 ms) or late in it (370 ms): after the first
    batch's failed no-op proof the batches' IHAVE / IWANT run inside the
    IDONTWANT list pass of fragment-group rows, the sender planes built from
    the dense rows (the oracle counts 9,943, 41,933, 81,592 and 143 IWANTs)."""
    p = _go(frags, 2400, seed=260 + phase_ms, hb_phase_ns=_phase(phase_ms))
    sim, _ = compare(p, 5, LINKS, _sched(32, 2400), batch=8)
    st = sim.stats()
    assert st["gossip_iwant"] > 0
    assert st["gossip_fallback_batches"] <= 1
    assert st["gossip_list_batches"] >= 3


def test_fragmented_idontwant_list_overflow_reruns_on_push_path(monkeypatch):
    """Candidate lists capped at 2 entries overflow: the batch, its dense keys
    partly written by the passes, re-runs on the push path from fresh keys."""
    monkeypatch.setenv("GS_LPULL_CAP", "2")
    p = _go(4, 1500, seed=63, lazy_gossip=0)
    sim, _ = compare(p, 5, LINKS, _sched(64, 1500), batch=64)
    assert sim.stats()["list_pull_batches"] == 0


def test_idontwant_and_plain_batches_alternate(monkeypatch):
    """One run whose fragments are above the IDONTWANT threshold (15000 B / 8),
    then below it (3000 B / 8), then above it again: IDONTWANT batches (dense
    INF-initialised keys) and plain ones (the final log) alternate in the same
    buffers of one context, all of them on the list pass."""
    monkeypatch.setenv("GS_REQUIRE_LPULL", "1")
    N = 1500
    t, pub, size = _sched(24, N)
    size = size.copy()
    size[8:16] = 3000
    p = _go(8, N, seed=65, lazy_gossip=0)
    assert p.idontwant == 1000
    sim, _ = compare(p, 5, LINKS, (t, pub, size), batch=8)
    st = sim.stats()
    assert st["batches"] == 3 and st["list_pull_batches"] == 3


def test_fragmented_idontwant_peer_traffic():
    """gs_set_traffic after the IDONTWANT list pass of F = 3 rows (a padding
    lane per group): the traffic pass reads the dense final keys; per-peer
    counters bit-exact against the oracle, accumulated over two runs."""
    p = _go(3, 900, seed=71)
    sched = _sched(12, 900)
    ref = oracle.simulate(p, 5, LINKS, sched=sched, traffic=True)
    sim, _ = gpu_sim(p, 5, LINKS, batch=8)
    sim.set_traffic(True)
    sim.run((sched[0][:5], sched[1][:5], sched[2][:5]))
    sim.run((sched[0][5:], sched[1][5:], sched[2][5:]))
    np.testing.assert_array_equal(sim.traffic(), ref["traffic"])
    assert sim.stats()["list_pull_batches"] >= 1


def test_colliding_fragments_with_idontwant():
    """Defect D8 (rust layout, msg_size / F <= 10: every fragment carries chunk
    id 0, so one fragment lane spreads and no message completes) with an
    IDONTWANT threshold below the fragment size: bit-exact on whichever path
    takes the batch."""
    p = oracle.params(peers=500, seed=6, fragments=4, idontwant=1)
    compare(p, 5, LINKS, _sched(9, 500, size=40), batch=4)


def test_fragmented_idontwant_latency_stream():
    """The u16 latency stream the CLI logs from (gs_result_sink.on_lat) after
    the IDONTWANT list pass of F = 8 rows: the ms of the oracle's t_complete."""
    N, M = 1500, 16
    p = _go(8, N, lazy_gossip=0)
    sched = _sched(M, N)
    ref = oracle.simulate(p, 5, LINKS, sched=sched)
    sim, _ = gpu_sim(p, 5, LINKS, batch=8)
    lat = {}
    sim.run(sched, on_lat=lambda first, v: lat.__setitem__(first, v.copy()), block_msgs=4)
    got = np.concatenate([lat[k] for k in sorted(lat)])
    np.testing.assert_array_equal(got, _logged_ms(ref["t_complete"], sched, p.self_log))
    st = sim.stats()
    assert st["list_pull_batches"] == 2 and st["deliveries"] == ref["stats"]["deliveries"]
