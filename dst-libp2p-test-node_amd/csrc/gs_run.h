// The driver of one gs_run call: which path a batch takes (PathPlan and the
// functions that fill it: the only place those conditions are written), one batch
// on the push path (run_push_batch, beside run_pull_batch and run_lpull_batch),
// the chain ahead of churn runs (Ahead) and the batch loop (Run).
// Included by gs_relax.hip inside its namespaces, as gs_part.h is: the kernels
// live in that unit's anonymous namespace.
#pragma once

// ---- schedule facts ----

// A publish time against the heartbeats hb_phase + h * hb: its epoch and offset
// into it (t >= hb_phase: churn and the class regrouping check that first), and
// the first heartbeat at or after it, h0, rel0 after the publish. Messages with
// one rel0 are lockstep: their heartbeats and epoch boundaries are one relative
// time for all lanes (for t > hb_phase: rel0 equal exactly when off is).
struct HbPos {
  uint64_t ep, off, h0, rel0;
};
static HbPos hb_pos(const Ctx& c, uint64_t t) {
  const uint64_t hb = c.cfg.heartbeat_ns, ph = c.cfg.hb_phase_ns;
  if (t <= ph) return {0, 0, 0, ph - t};
  const uint64_t ep = (t - ph) / hb, off = (t - ph) % hb;
  return {ep, off, ep + (off ? 1 : 0), off ? hb - off : 0};
}

// Messages a pull-path batch holds at the most: the pull path holds a row in
// registers, PULL_LMAX lanes of FP per message.
static uint32_t pull_batch_cap(uint32_t Bmax, uint32_t F0) {
  return std::max<uint32_t>(1, std::min<uint32_t>(Bmax, PULL_LMAX / pow2_at_least(F0)));
}

// The end of the same-shape run from a0: consecutive messages of a0's size and
// chunk count (serialisation tables and the lane layout are per batch), `cap` at
// the most, not across a cut of the class regrouping; ring (churn): their publish
// epochs [h_lo, h_hi] plus the lifetime fit the snapshot ring.
static uint64_t same_shape_end(const Ctx& c, const gs_publish* sched, uint64_t n, uint64_t a0, uint64_t cap,
                               const std::vector<uint8_t>* cut, bool ring, uint64_t& h_lo, uint64_t& h_hi) {
  const uint32_t F0 = frags_of(c, sched[a0]);
  h_lo = h_hi = ring ? hb_pos(c, sched[a0].t_pub_ns).ep : 0;
  uint64_t a1 = a0 + 1;
  while (a1 < n && a1 - a0 < cap && !(cut && (*cut)[a1]) && sched[a1].msg_size == sched[a0].msg_size &&
         frags_of(c, sched[a1]) == F0) {
    if (ring) {
      const uint64_t ep = hb_pos(c, sched[a1].t_pub_ns).ep, lo2 = std::min(h_lo, ep), hi2 = std::max(h_hi, ep);
      if (hi2 + c.cfg.churn_horizon - lo2 + 1 > c.ring_R) break;
      h_lo = lo2;
      h_hi = hi2;
    }
    a1++;
  }
  return a1;
}

// ---- the plan of a batch ----

// Decided once per batch (or slice group) before anything is enqueued for it:
// the paths it is offered to. Run::run_batch tries them in this order, each
// falling through to the next when it cannot take the batch or loses it:
//   chn   the churn list pass                      -> the push path
//   glp   (when the context prefers it) the list pass with the gossip inside
//   lp    the eager list pass, no-log when `nolog` -> k_pull, or the push path under IDONTWANT
//   pull  k_pull alone (list pass off or no ring)
//   else  the eager push path; then with lazy gossip the no-op proof, and when it
//         fails glp (unless tried), then the push path with gossip.
struct PathPlan {
  bool idw = false;       // IDONTWANT active in this batch
  bool lockstep = false;  // lazy gossip: one rel0 for every message (hb_pos)
  // The list pass's window width: the batch's Delta, but no wider than the smallest
  // latency when IDONTWANT is active (a neighbour's key final in the same window as
  // the sender's can then never pass the test t_y + lat(y -> u) <= t_u: the sender
  // cannot see it yet; keys of earlier windows are final and stored before the pass
  // starts) or lazy gossip runs inside the pass (an IHAVE never shares a window with
  // its heartbeat): win for the eager pass, win_gos with the gossip inside, win_chn
  // for the churn list pass (which carries the gossip whenever it is configured).
  uint64_t win = 0, win_gos = 0, win_chn = 0;
  bool pull = false;   // the pull path at all (k_pull behind the list pass)
  bool lp = false;     // the list pass
  bool glp = false;    // lazy gossip inside the list pass
  bool chn = false;    // the churn list pass
  bool dense = false;  // the batch's reader needs dense [N][L] rows (k_lfinal)
  bool nolog = false;  // the no-log form, once a ring fits
  // run_lpull_batch's options as far as the plan decides them; a path adds what it carries
  LpOpts opts() const {
    LpOpts o;
    o.dense = dense;
    o.idw = idw;
    return o;
  }
};

static bool idw_active(const Ctx& c, const Batch& b) { return c.cfg.idontwant && b.payload >= c.cfg.idontwant; }
static uint64_t lp_window(const Batch& b, bool narrow) { return narrow ? std::min(b.delta, b.lat_min) : b.delta; }
static Batch with_window(const Batch& b, uint64_t w) {
  Batch x = b;
  x.delta = w;
  return x;
}

// Dense rows: a sink's rows or summaries, a pass over the final keys (Ctx::keys_pass:
// per-peer traffic, pubsub counts, per-link first deliveries or message costs), GS_LPULL_DENSE (diagnostic:
// dense rows + k_complete, whose known key stream calibrates the PMC read factor,
// scripts/pmc_summary.py). IDONTWANT batches keep their final keys dense all along
// and ask for no conversion: run_lpull_batch never looks at `dense` under IDONTWANT, so
// the in-pass gossip, which used to pass it regardless, shares the rule. (Slice groups
// refuse such a pass up front: the keys_pass term is false there.)
static bool dense_rows(const Ctx& c, const SinkWants& sw, bool idw) {
  return !idw && (sw.rows() || sw.summary || c.keys_pass() || getenv("GS_LPULL_DENSE"));
}

// Lazy gossip inside the list pass (GOS, gs_lpull_kernel.h), on top of the list
// pass taking the batch: rows with or without IDONTWANT (fragment groups too: every
// fragment is gossiped on its own at its message's heartbeats, as the oracle's
// sched_gossip) on the frozen mesh, lockstep, CSR rows narrow enough for a 58-bit
// target mask, windows of at least a grain and heartbeats farther apart than an
// IHAVE travels. GS_GOSSIP_LIST=0 keeps such batches on the eager pass + no-op
// proof, with the push path behind it. (The old loop spelled this twice: `glp`
// of a single batch named the list pass's conditions again, `glp_ok` of a slice
// group left them out, having checked them before the group formed. One rule:
// PathPlan::glp = lp && lazy gossip && this.)
static bool gossip_list_admit(const Ctx& c, const Batch& b, const PathPlan& p) {
  return p.lockstep && !env_off("GS_GOSSIP_LIST") && c.max_degree <= GSE_HOPS && p.win_gos >= pull_grain(b.tshift) &&
         c.cfg.heartbeat_ns > b.lat_max + p.win_gos;
}

// After n batches ran with the gossip inside their passes (iwant0: C_GOSSIP before
// them). GLP_QUIET batches in a row whose gossip sent no IWANT: the next one tries
// the eager pass and its no-op proof first again (glp_prefer was never
// cleared). Not after one: batches alternating with and without IWANTs (a
// heartbeat late in the dissemination) would pay a failed proof every other batch.
static void glp_account(Ctx& c, uint64_t iwant0, uint32_t n) {
  if (read_counter(c, C_GOSSIP) != iwant0) c.glp_quiet = 0;
  else if ((c.glp_quiet += n) >= GLP_QUIET) c.glp_prefer = false;
}

// GS_RELAX_VARIANT: the paths a run may take, a bit mask (default 237, every path
// on): owner-computes pull (32) over candidate lists (64), fragmented batches too
// (128; config #2 7.2e8 against 6.7e8/s on k_pull's dense rows, round 4); k_pull's
// dense rows without 64; without 32 the push path, split into scan + frontier (8).
// Bits 1, 2 and 4 selected forms of the push path that are gone and are not read.
struct PathKnob {
  bool pull, list, frag_list, split;
};
static PathKnob path_knob() {
  const long e = env_int("GS_RELAX_VARIANT", -1), v = e < 0 ? 237 : e;  // unset or negative: the default
  return {(v & 32) != 0, (v & 64) != 0, (v & 128) != 0, (v & 8) != 0};
}

// Fresh keys and uplink FIFO state for a batch on any path (the list pull path
// needs no dense keys).
static void reset_keys(Ctx& c, const Batch& b, bool dense_keys) {
  hipStream_t s = c.stream;
  const uint32_t N = c.cfg.peers;
  c.keys_log = c.keys_none = false;
  if (dense_keys) GS_HIP(hipMemsetAsync(c.d_keys.p, 0xFF, (uint64_t)N * b.L * 8, s));
  if (b.FP > 1) GS_HIP(hipMemsetAsync(c.d_busy.p, 0, (size_t)N * b.B * 8, s));
}

// ---- one batch on the push path ----

// Fresh bucket state for the push path in form f.
static void reset_push(Ctx& c, const Batch& b, PushForm f, bool with_gossip, size_t max_tiles) {
  hipStream_t s = c.stream;
  const uint64_t total = (uint64_t)c.cfg.peers * b.L;
  GS_HIP(hipMemsetAsync(c.d_fbits.p, 0, (total + 63) / 64 * 8, s));
  if (f.skip) {  // tmin 0 forces every tile's first scan
    c.d_tmin.alloc(max_tiles);
    c.d_touched.alloc(max_tiles);
    GS_HIP(hipMemsetAsync(c.d_tmin.p, 0, (total + 63) / 64 * 8, s));
    GS_HIP(hipMemsetAsync(c.d_touched.p, 0, (total + 63) / 64, s));
    if (with_gossip) {
      c.d_tgmin.alloc(max_tiles);
      c.d_tnf.alloc(max_tiles);
      c.d_tstamp.alloc(max_tiles);
      GS_HIP(hipMemsetAsync(c.d_tstamp.p, 0, (total + 63) / 64 * 4, s));
    }
  }
  GS_HIP(hipMemsetAsync(c.d_ctrl.p, 0xFF, 4 * 8, s));
  // with gossip the first bucket is [0, Delta): the publisher's own IHAVEs
  // can land before the first eager arrival
  if (with_gossip) GS_HIP(hipMemsetAsync(c.d_ctrl.p, 0, 8, s));
}

// The split path's frontier segments (one per scan wave) and, with gossip, its
// gossip and holder lists.
static void push_lists(Ctx& c, const Batch& b, PushForm f, bool with_gossip, unsigned grid, RelaxArgs& ra) {
  hipStream_t s = c.stream;
  const uint32_t FP = b.FP;
  const uint64_t total = (uint64_t)c.cfg.peers * b.L;
  const uint64_t nwaves = (uint64_t)grid * (TB / 64), ntiles = (total + 63) / 64;
  // tiles one scan wave can visit: groups of 64 with tile skip (k_scan), single tiles without
  const uint64_t gt = f.skip ? 64 : 1;
  const uint64_t wave_tiles = ((ntiles + gt - 1) / gt + nwaves - 1) / nwaves * gt;
  ra.seg_cap = (uint32_t)(wave_tiles * (64 / FP));
  c.d_fr_idx.alloc(nwaves * ra.seg_cap);
  if (FP == 1) c.d_fr_key.alloc(nwaves * ra.seg_cap);
  c.d_fr_cnt.alloc(nwaves);
  ra.fr_idx = c.d_fr_idx.p;
  ra.fr_key = c.d_fr_key.p;
  ra.fr_cnt = c.d_fr_cnt.p;
  if (!with_gossip) return;
  // gossip list: per-lane entries, one segment per scan wave
  ra.gl_cap = (uint32_t)(wave_tiles * 64);
  c.d_gl_idx.alloc(nwaves * ra.gl_cap);
  c.d_gl_cnt.alloc(nwaves);
  c.d_nonfinal.alloc(3);
  GS_HIP(hipMemsetAsync(c.d_nonfinal.p, 0, 3 * 8, s));
  ra.gl_idx = c.d_gl_idx.p;
  ra.gl_cnt = c.d_gl_cnt.p;
  if (ra.ring_in) {
    c.d_gl_key.alloc(nwaves * ra.gl_cap);
    ra.gl_key = c.d_gl_key.p;
    // holder list (a lane is finalised once) and per-launch marks
    c.d_hl_idx.alloc(total);
    c.d_hl_key.alloc(total);
    c.d_hl_cnt.alloc(1);
    c.d_hl_mark.alloc(2 * (size_t)HL_LAUNCHES);
    c.d_hwin.alloc(total);
    GS_HIP(hipMemsetAsync(c.d_hwin.p, 0xFF, total, s));
    ra.hwin = c.d_hwin.p;
    c.d_hs_idx.alloc(nwaves * ra.gl_cap);
    c.d_hs_key.alloc(nwaves * ra.gl_cap);
    c.d_hl_min.alloc(3);
    GS_HIP(hipMemsetAsync(c.d_hl_cnt.p, 0, 8, s));
    GS_HIP(hipMemsetAsync(c.d_hl_min.p, 0xFF, 3 * 8, s));
    ra.hs_idx = c.d_hs_idx.p;
    ra.hs_key = c.d_hs_key.p;
    ra.hl_min = c.d_hl_min.p;
    ra.hl_idx = c.d_hl_idx.p;
    ra.hl_key = c.d_hl_key.p;
    ra.hl_cnt = (unsigned long long*)c.d_hl_cnt.p;
    ra.hl_lo = c.d_hl_mark.p;
    ra.hl_end = c.d_hl_mark.p + HL_LAUNCHES;
  }
  ra.nonfinal = c.d_nonfinal.p;
  if (f.skip) {
    ra.tgmin = c.d_tgmin.p;
    ra.tnf = c.d_tnf.p;
    ra.tstamp = c.d_tstamp.p;
  }
}

// One batch on the push path in form f: k_seed, then bucket launches in chunks of
// 8 until the ctrl word of the next bucket is empty. g0 (churn + lazy gossip): the
// earliest time an IHAVE of the batch can arrive.
static void run_push_batch(Ctx& c, const Batch& b, PushForm f, bool with_gossip, uint64_t g0, size_t max_tiles) {
  hipStream_t s = c.stream;
  const uint32_t N = c.cfg.peers, FP = b.FP;
  const uint64_t total = (uint64_t)N * b.L;
  reset_keys(c, b, true);
  reset_push(c, b, f, with_gossip, max_tiles);
  launch_seed(c, b, 0, N);
  RelaxArgs ra = relax_args(c, b, with_gossip);
  if (ra.ring_in) {
    ra.malive = c.d_malive.p;
    ra.g0 = g0;
  }
  ra.busy = c.d_busy.p;
  ra.fbits = c.d_fbits.p;
  ra.tmin = c.d_tmin.p;
  ra.touched = c.d_touched.p;
  ra.ctrl = c.d_ctrl.p;
  ra.counters = c.d_counters.p; ra.delta = b.delta;
  const uint64_t need = (total + TB - 1) / TB;
  const unsigned grid = (unsigned)std::min<uint64_t>(need, (uint64_t)c.num_cus * SPLIT_BLOCKS_PER_CU);
  if (f.split) push_lists(c, b, f, with_gossip, grid, ra);
  uint32_t launch = 0;
  const uint32_t chunk = 8;
  for (;;) {
    if (ra.hl_idx && launch + chunk > HL_LAUNCHES)
      c.fail(GS_EUNSUPPORTED, "churn + lazy gossip batch needs more than 65536 buckets");
    for (uint32_t q = 0; q < chunk; q++) {
      ra.launch = launch++;
      if (c.timing) {  // (start, scan end, end) per bucket
        GS_HIP(hipEventRecord(run_ev(c, c.ev_n), s));
        const hipEvent_t mid = run_ev(c, c.ev_n + 1);
        relax_dispatch(FP, f, ra, grid, s, mid);
        if (!f.split) GS_HIP(hipEventRecord(mid, s));  // the fused kernel: all of it counts as scan
        GS_HIP(hipEventRecord(run_ev(c, c.ev_n + 2), s));
        c.ev_n += 3;
      } else {
        relax_dispatch(FP, f, ra, grid, s);
      }
    }
    GS_HIP(hipGetLastError());
    GS_HIP(hipMemcpyAsync(c.h_pinned, c.d_ctrl.p, 3 * 8, hipMemcpyDeviceToHost, s));
    GS_HIP(hipStreamSynchronize(s));
    if (c.h_pinned[launch % 3] == INF64) break;
  }
  c.stats.relax_launches += launch;
}

// ---- per-run and per-batch context state, as guards ----

// The run's latency lines are handed out asynchronously (c.lat_async) until it ends.
struct AsyncOff {
  Ctx& c;
  int unwinding0 = std::uncaught_exceptions();
  explicit AsyncOff(Ctx& cc) : c(cc) {
    if (c.lat_pend.on) {  // left by a run that failed: its lines are not handed out
      GS_HIP(hipStreamSynchronize(c.copy));
      c.lat_pend.on = false;
    }
    c.lat_async = true;
  }
  ~AsyncOff() {
    c.lat_async = false;
    //  a run that fails after a batch completed still hands out that
    // batch's pending latency lines, as the synchronous sink did before; nothing
    // here may throw while the error unwinds
    Ctx::LatPending& p = c.lat_pend;
    if (std::uncaught_exceptions() <= unwinding0 || !p.on) return;
    p.on = false;
    if (hipEventSynchronize(c.lat_done[p.par]) != hipSuccess || (c.h_laterr[p.par] & ERR_LAT16)) return;
    for (uint32_t q0 = 0; q0 < p.B; q0 += p.bm) {
      const uint32_t n = std::min(p.bm, p.B - q0);
      p.sink->on_lat(p.sink->user, p.row0 + q0, n, p.un, c.h_lat[p.par] + (size_t)q0 * p.un);
    }
  }
};

// Churn runs (config #3): the epoch chain is latency-bound and runs as fast on
// one XCD's 32 CUs as on all 256 (one L2 holds its per-peer state; bits 0..31
// of the CU mask, 4 CUs on each XCD, take twice as long), and the list pass at
// 100k peers as fast on 7 XCDs (or 4) as on 8 (profiles/r06_chain). So the
// chain gets its own XCD (c.chain_pipe, GS_CHAIN_XCDS, default XCD 0) and the
// rest of the run the others (c.pass_ms, GS_PASS_XCDS, default 1-7): the next
// batch's chain then runs beside this batch's passes (Ahead below).
// GS_CHN_PIPE=0 keeps one stream (GS_PASS_XCDS alone then still moves the passes).
static bool chain_pipe_wanted(Ctx& c) {
  ensure_cus(c);
  return c.cfg.churn_ppm && !env_off("GS_CHN_PIPE") && c.num_cus == 256 && c.cfg.flood_publish && !c.keys_pass() &&
         !c.sink_dev && !getenv("GS_DEBUG_CHN");
}
// c.stream is the passes' stream for the run; the caller's stream waits for it at the end.
struct PassStream {
  Ctx& c;
  hipStream_t orig = nullptr;
  PassStream(Ctx& cc, bool pipe) : c(cc) {
    uint32_t px = xcd_env("GS_PASS_XCDS");
    if (pipe) {
      if (!c.chain_pipe) {
        const uint32_t cx = xcd_env("GS_CHAIN_XCDS");
        c.chain_pipe = xcd_stream(c, cx ? cx : 0x01u);
      }
      if (!px) px = 0xFEu & ~xcd_env("GS_CHAIN_XCDS");
    }
    if (!px) return;
    if (!c.pass_ms) {  // created once per context (a CU-masked stream costs ~10 ms)
      c.pass_ms = xcd_stream(c, px);
      for (auto& ev : c.pass_ev) GS_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    }
    orig = c.stream;
    GS_HIP(hipEventRecord(c.pass_ev[0], orig));
    GS_HIP(hipStreamWaitEvent(c.pass_ms, c.pass_ev[0], 0));
    c.stream = c.pass_ms;
  }
  ~PassStream() {
    if (!orig) return;
    (void)hipEventRecord(c.pass_ev[1], c.pass_ms);
    (void)hipStreamWaitEvent(orig, c.pass_ev[1], 0);
    (void)hipStreamSynchronize(orig);
    c.stream = orig;
  }
};

// While churn_ring runs the epochs of a batch the churn list pass takes (defer):
// no inverse IHAVE lists (the push path's) and no ELL snapshots (the pass reads
// the mask ring) beside the epochs; the caller may set c.epoch_hook, cleared here too.
struct ChurnDefer {
  Ctx& c;
  ChurnDefer(Ctx& cc, bool defer) : c(cc) {
    c.ring_in_defer = defer;
    c.ring_ell_defer = defer;
  }
  ~ChurnDefer() {
    c.epoch_hook = nullptr;
    c.ring_in_defer = false;
    c.ring_ell_defer = false;
  }
};

// The list pass calls `poll` between groups of passes.
struct PassPoll {
  Ctx& c;
  PassPoll(Ctx& cc, std::function<void()> poll) : c(cc) { c.pass_poll = std::move(poll); }
  ~PassPoll() { c.pass_poll = nullptr; }
};

// ---- the chain ahead ----

// The next churn list-pass batch's epoch chain and tables, enqueued on the
// chain's XCD (c.chain_pipe) while this batch's passes run on the others (the
// host enqueues the chain in slices between pass groups, at most AH_LEAD epochs
// ahead of what the GPU finished). The list pass reads only the batch tables,
// so the chain may overwrite ring slots of the batch whose passes run; a batch
// that falls back to the push path joins the chain first and has churn_ring
// replay its ring slots. A replay (from epoch 0 up to the falling-back batch's
// last epoch) takes the ring and the mesh state back below the prepared batch's
// last epoch h1: the prepared batch is then dropped and prepares in line after
// the push path's run, as a batch without a chain ahead does (the seeds and the
// push path read the ring's offline bits, so a prepared batch is only good
// while the ring holds its epochs).
struct Ahead {
  static constexpr uint64_t AH_MARK = 16, AH_LEAD = 192, AH_SLICE = 64;
  Ctx& c;
  bool on = false, joined = false;
  uint64_t i0 = 0, i1 = 0, h1 = 0;  // the prepared batch's messages and last epoch
  ChnPrep cp;
  EvRun* run = nullptr;
  hipEvent_t ready = nullptr;
  std::vector<hipEvent_t> marks;  // ring of events every AH_MARK epochs on the chain stream
  uint64_t mark_n = 0, done_h = 0, enq_h = 0;

  explicit Ahead(Ctx& cc) : c(cc) {}
  Ahead(const Ahead&) = delete;
  ~Ahead() {
    if (run) chain_free(run);
    if (ready) (void)hipEventDestroy(ready);
    for (auto e : marks) (void)hipEventDestroy(e);
  }
  static bool debug() {
    static const bool dbg = getenv("GS_DEBUG_AHEAD") != nullptr;
    return dbg;
  }

  // Messages [n0, n1), publish epochs from hl, lifetime to h1 (epochs q0 per message):
  // the chain and tables of that batch from here on, if the ring can simply go on.
  void start(uint64_t n0, uint64_t n1, uint64_t hl, uint64_t h1_, const uint64_t* q0, const gs_publish* pubs,
             uint32_t B, uint32_t FP) {
    const uint32_t par = c.ct_par ^ 1u;
    // the chain overwrites ring slots: after every reader of this batch's slots on the main stream
    if (!ready) GS_HIP(hipEventCreateWithFlags(&ready, hipEventDisableTiming));
    GS_HIP(hipEventRecord(ready, c.stream));
    GS_HIP(hipStreamWaitEvent(c.chain_pipe, ready, 0));
    chn_begin(c, cp, par, c.chain_pipe, hl, (uint32_t)(h1_ - hl + 1), q0, pubs, B, FP);
    run = chain_begin(c, h1_, c.chain_pipe, [this](uint64_t h) { chn_chunks(c, cp, h, false); });
    if (!run) return;  // (not a plain continuation of the ring: the batch prepares in line)
    c.ct_par = par;
    on = true;
    joined = false;
    i0 = n0;
    i1 = n1;
    h1 = h1_;
    mark_n = done_h = enq_h = 0;
    if (debug())
      fprintf(stderr, "[ah] batch %llu..%llu: chain to epoch %llu (state %llu), tables %u\n", (unsigned long long)n0,
              (unsigned long long)n1, (unsigned long long)h1, (unsigned long long)c.churn_state, par);
    pump(false);
  }

  // More of the chain, keeping at most AH_LEAD epochs in flight (all: the rest of it).
  void pump(bool all) {
    if (!on || !run) return;
    while (run) {
      if (!all) {
        while (mark_n && done_h + AH_MARK <= enq_h) {  // the oldest outstanding mark
          const uint64_t k = done_h / AH_MARK + 1;  // mark k: after epoch k * AH_MARK of the run
          if (k > mark_n) break;
          if (hipEventQuery(marks[(k - 1) % marks.size()]) != hipSuccess) break;
          done_h = k * AH_MARK;
        }
        if (enq_h >= done_h + AH_LEAD) return;
      }
      const uint64_t n = all ? ~0ull : std::min<uint64_t>(AH_SLICE, done_h + AH_LEAD - enq_h);
      for (uint64_t k = 0; k < n && run; k++) {
        const bool fin = chain_advance(c, *run, 1);
        enq_h++;
        if (enq_h % AH_MARK == 0) {
          if (marks.size() < 2 * AH_LEAD / AH_MARK + 2) {
            hipEvent_t e;
            GS_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            marks.push_back(e);
          }
          mark_n = enq_h / AH_MARK;
          GS_HIP(hipEventRecord(marks[(mark_n - 1) % marks.size()], c.chain_pipe));
        }
        if (fin) enqueue_end();
      }
      if (!all) return;
    }
  }

  // The prepared batch's tables before the main stream's next work.
  void join() {
    if (!on || joined) return;
    pump(true);
    GS_HIP(hipStreamWaitEvent(c.stream, ready, 0));
    joined = true;
    if (debug()) fprintf(stderr, "[ah] batch %llu: joined\n", (unsigned long long)i0);
  }

  // The prepared batch is taken (its ChnPrep copied out) or given up.
  void drop() { on = false; }

 private:
  void enqueue_end() {  // every epoch is enqueued: the rest of the tables, then `ready`
    if (debug())
      fprintf(stderr, "[ah] batch %llu: chain enqueued (%llu epochs)\n", (unsigned long long)i0,
              (unsigned long long)enq_h);
    chain_free(run);
    run = nullptr;
    chn_end(c, cp, c.chain_pipe);
    if (!ready) GS_HIP(hipEventCreateWithFlags(&ready, hipEventDisableTiming));
    GS_HIP(hipEventRecord(ready, c.chain_pipe));
  }
};

// ---- the run ----

// One batch of the loop: its messages, geometry, plan and what its paths hand on.
struct BatchRun {
  uint64_t i0 = 0, i1 = 0;
  uint64_t h_lo = 0, h_hi = 0;  // churn: publish epochs of the batch
  Batch b;
  PathPlan p;
  ChnPrep cp;             // churn list pass: the batch's tables
  uint64_t g0 = INF64;    // churn + lazy gossip: the earliest IHAVE arrival
  bool glp_tried = false;
  NoLog nl;               // the eager batch ran the no-log list pass
};

// A slice group (Run::try_slices): S consecutive full batches of Bc messages of
// one shape from i0, run as one list pass over S copies of the graph.
struct SliceGroup {
  uint64_t i0 = 0;
  uint32_t S = 0, Bc = 0;
  std::vector<Batch> bs;             // the slices
  Batch g;                           // the group's pass: slice 0's shape, keys over S x N rows
  std::vector<uint32_t> spub, lpub;  // publishers as slice rows and as peers
  std::vector<uint64_t> stp, rel, hab;  // publish times; lazy gossip: rel0 and h0 of every message
  PathPlan p;
  bool wants = false;  // the sink takes something per message
  Slices sl{};
};

struct Run {
  Ctx& c;
  const gs_publish* sched;
  const uint64_t n_msgs;
  const gs_result_sink* sink;
  const std::vector<uint8_t>* cut;  // the class regrouping's batch cuts (class_plan), or null
  const uint32_t N, Bmax;
  const SinkWants sw;
  AsyncOff async_off;
  const bool pipe_on;
  PassStream pass_stream;
  const bool gossip, churn;
  const PathKnob knob;
  bool lanes32 = false, pull_any = false, chn_any = false;
  size_t max_tiles = 0;
  uint32_t sl_max = 0;      // GS_SLICES
  uint64_t slice_skip = 0;  // messages before it run as single batches
  std::vector<uint64_t> q0v, r0v, rel0, habs0, q0a, r0a;
  std::vector<uint8_t> malive;
  Ahead ah;

  // rows per pass a slice group aims at (memory: ~S x N x L x 40 B)
  static constexpr uint64_t SL_ROWS = 1ull << 19;

  Run(Ctx& cc, const gs_publish* sched_, uint64_t n, const gs_result_sink* sink_, const std::vector<uint8_t>* cut_)
      : c(cc), sched(sched_), n_msgs(n), sink(sink_), cut(cut_), N(cc.cfg.peers), Bmax(cc.cfg.batch),
        sw(sink_wants(cc, sink_)), async_off(cc), pipe_on(chain_pipe_wanted(cc)), pass_stream(cc, pipe_on),
        gossip(cc.cfg.lazy_gossip != 0), churn(cc.cfg.churn_ppm != 0), knob(path_knob()), q0v(Bmax), r0v(Bmax),
        rel0(Bmax), habs0(Bmax), q0a(Bmax), r0a(Bmax), malive(Bmax), ah(cc) {
    hipStream_t s = c.stream;
    GS_HIP(hipMemsetAsync(c.d_counters.p + C_ERR, 0, 8, s));
    check_schedule(c, sched, n_msgs);
    uint32_t Fmax = 1;
    for (uint64_t i = 0; i < n_msgs; i++) Fmax = std::max(Fmax, frags_of(c, sched[i]));
    const uint32_t FPmax = pow2_at_least(Fmax);
    lanes32 = (uint64_t)N * Bmax * FPmax < (1ull << 32);  // frontier and gossip list indices are u32
    // the pull path needs rows in LDS and one mesh per batch (churn uses one per
    // epoch: the push path, or the churn list pass)
    pull_any = knob.pull && !churn;
    // churn on the list pass (gs_cpull.h): CSR rows of <= 64 entries (<= 58 with lazy gossip:
    // the IHAVE entry's target mask); GS_CHURN_LIST=0 keeps churn batches on the push path
    chn_any = churn && knob.pull && knob.list && !env_off("GS_CHURN_LIST") &&
              c.max_degree <= (gossip ? GSE_HOPS : CELL_W) && N < (1u << 21);
    if (churn && !lanes32) c.fail(GS_EUNSUPPORTED, "churn needs peers*batch*FP < 2^32");
    if (churn) {  // epoch of every publish; the snapshot ring
      for (uint64_t i = 0; i < n_msgs; i++)
        if (sched[i].t_pub_ns < c.cfg.hb_phase_ns || hb_pos(c, sched[i].t_pub_ns).ep >= (1ull << 20))
          c.fail(GS_EINVAL, "churn needs every publish within 2^20 heartbeats after hb_phase_ns");
      ensure_ring(c);
    }
    max_tiles = ((size_t)N * Bmax * FPmax + 63) / 64;
    c.d_keys.alloc((size_t)N * Bmax * FPmax);
    c.d_fbits.alloc(max_tiles);
    if (FPmax > 1) c.d_busy.alloc((size_t)N * Bmax);
    c.d_tc.alloc((size_t)N * Bmax);
    c.d_hops.alloc((size_t)N * Bmax);
    c.d_cnt_save.alloc(C_COUNT);
    c.ev_n = 0;
    if (c.timing) {
      GS_HIP(hipEventRecord(run_ev(c, 0), s));
      run_ev(c, 1);
      c.ev_n = 2;
    }
    sl_max = (uint32_t)std::max(0l, env_int("GS_SLICES", 64));
  }

  // The whole schedule, batch by batch; then the run's statistics.
  void run() {
    uint64_t i0 = 0;
    for (c.run_batch = 0; i0 < n_msgs; c.run_batch++) {
      uint64_t ie = 0;
      if (i0 >= slice_skip && try_slices(i0, ie)) {
        i0 = ie;
        continue;
      }
      i0 = run_batch(i0);
    }
    lat_flush(c);  // the last batch's latencies
    if (c.timing) GS_HIP(hipEventRecord(run_ev(c, 1), c.stream));
    collect_stats(c);
    if (!c.timing) return;
    double scan = 0, front = 0;
    for (size_t q = 2; q + 2 < c.ev_n; q += 3) {
      float x = 0, y = 0;
      GS_HIP(hipEventElapsedTime(&x, c.ev_pool[q], c.ev_pool[q + 1]));
      GS_HIP(hipEventElapsedTime(&y, c.ev_pool[q + 1], c.ev_pool[q + 2]));
      scan += x;
      front += y;
    }
    c.stats.relax_ms += scan + front;
    c.stats.scan_ms += scan;
    c.stats.frontier_ms += front;
    float rm = 0;
    GS_HIP(hipEventElapsedTime(&rm, c.ev_pool[0], c.ev_pool[1]));
    c.stats.run_ms += rm;
  }

  // ---- planning ----

  // The list pass can take batches of FP lanes per message at all: bit 64; rows of
  // fragment groups with bit 128 (the default).
  bool list_pass_any(uint32_t FP) const { return knob.list && (FP == 1 || knob.frag_list); }

  // The push path's form for a batch; gc: it runs with lazy gossip or churn. Those
  // run split + tile skip (their long tail of IHAVE and churn buckets touches few
  // tiles; gossip and churn exist on the split path only: run_batch and the
  // constructor refuse what its 32-bit indices cannot hold). Else split wherever its
  // indices fit, unless the knob asks for the fused kernel.
  PushForm push_form(bool gc) const {
    const bool split = gc || (lanes32 && knob.split);
    return {split, split && gc};
  }

  // The plan of batch b but for its churn list pass (chn_admit). rel: rel0 of its n messages
  // (lazy gossip); sliced: a slice group's pass (frozen mesh, no per-peer traffic, never no-log).
  PathPlan plan(const Batch& b, const uint64_t* rel, size_t n, bool sliced) const {
    PathPlan p;
    p.idw = idw_active(c, b);
    p.lockstep = gossip && n > 0;
    for (size_t q = 1; q < n && p.lockstep; q++) p.lockstep = rel[q] == rel[0];
    p.win = lp_window(b, p.idw);
    p.win_gos = lp_window(b, true);
    p.win_chn = gossip ? p.win_gos : p.win;
    // fragmented IDONTWANT batches (rows of fragment groups, each lane tested on its
    // own) wherever fragmented rows run at all (bit 128); GS_IDW_FRAG_LIST=0 keeps
    // them on the push path (A/B, per batch). With colliding fragments (defect D8)
    // only lane 0 of a group is ever final, as without IDONTWANT. k_pull has no
    // IDONTWANT: such a batch needs the list pass (bit 64).
    const bool idw_frag = knob.frag_list && !env_off("GS_IDW_FRAG_LIST");
    p.pull = pull_any && p.win >= pull_grain(b.tshift) && (!p.idw || (knob.list && (b.FP == 1 || idw_frag)));
    p.lp = p.pull && list_pass_any(b.FP);
    p.glp = p.lp && gossip && gossip_list_admit(c, b, p);
    p.dense = dense_rows(c, sw, p.idw);
    // No log (the passes complete the batch) exactly when nothing will read a per-message
    // value: no sink wants, no traffic pass, rows of single-fragment lanes on the frozen
    // mesh without IDONTWANT, and with lazy gossip a lockstep batch, whose no-op proof
    // needs the batch's deliveries and latest final time only (batch_sums). The passes'
    // 32-bit ms need every final time below 2^38 ns: checked on the batch's latest final
    // time after its passes (NoLog::inexact). GS_LPULL_SUM=0 (A/B, per batch): the log and k_lsum.
    p.nolog = !sliced && !p.dense && !sw.lat && !p.idw && !churn && b.FP == 1 && (!gossip || p.lockstep) &&
              !env_off("GS_LPULL_SUM");
    return p;
  }

  // churn: the batch runs on the churn list pass (gs_cpull.h) — lockstep batches (its
  // publishes at one offset r0 into their epochs; fragment groups included) without
  // IDONTWANT whose windows fit the rules
  bool chn_admit(const Batch& bb, const PathPlan& p, const uint64_t* r0, uint64_t h_lo, uint64_t h_hi) const {
    if (!chn_any || bb.collide || !c.d_ring_mm.p) return false;
    const uint64_t hb = c.cfg.heartbeat_ns;
    bool lock = true;
    for (uint32_t q = 1; q < bb.B && lock; q++) lock = r0[q] == r0[0];
    const uint64_t dl = p.win_chn;
    const uint64_t cE = h_hi + c.cfg.churn_horizon - h_lo + 1;
    return !p.idw && lock && cE <= 4096 && dl >= pull_grain(bb.tshift) && hb > lpull_rmax(bb) + 2 * dl &&
           (!gossip || hb > bb.lat_max + dl);
  }

  // a batch: up to B messages of one shape; a pull-path batch is capped (pull_batch_cap).
  // Returns the end; churn: the batch's publish epochs [h_lo, h_hi].
  uint64_t form(uint64_t a0, uint64_t& h_lo, uint64_t& h_hi) const {
    const uint32_t F0 = frags_of(c, sched[a0]);
    const uint64_t cap = pull_any || (chn_any && F0 == 1) ? pull_batch_cap(Bmax, F0) : Bmax;
    return same_shape_end(c, sched, n_msgs, a0, cap, cut, churn, h_lo, h_hi);
  }

  // ---- batch slices ----
  // Consecutive full batches of one shape on a small graph run as one list pass
  // over S copies of the graph (run_lpull_batch's Slices), so that a launch has
  // S x N rows instead of N: a pass of a few rows per resident wave is mostly
  // latency (config #2's 10k-peer F = 8 rows: 98 us per pass at 10k rows, 340 us
  // at 80k; scripts/c2_probe.py). Frozen mesh, no IDONTWANT, no per-peer traffic;
  // lazy gossip through the eager pass's no-op proof, per slice, and when that
  // fails (or failed before: glp_prefer) inside the group's passes as run_glp
  // does, if the whole group is lockstep (else single batches take it).
  // GS_SLICES=0 turns them off, GS_SLICES=n caps a group at n slices.

  // The group from i0, if there is one: at least two full batches of i0's shape.
  bool form_slices(uint64_t i0, SliceGroup& G) {
    if (sl_max < 2 || !pull_any || c.keys_pass() || (uint64_t)N * 2 >= (1u << 21)) return false;
    const uint32_t F0 = frags_of(c, sched[i0]);
    if (!list_pass_any(pow2_at_least(F0))) return false;
    const uint32_t Bc = pull_batch_cap(Bmax, F0);
    const uint64_t s_cap = std::min<uint64_t>({(uint64_t)sl_max, std::max<uint64_t>(1, SL_ROWS / N), ((1ull << 21) - 1) / N});
    uint64_t lo = 0, hi = 0;
    const uint64_t n_same = same_shape_end(c, sched, n_msgs, i0, s_cap * Bc, cut, false, lo, hi) - i0;
    const uint32_t S = (uint32_t)std::min<uint64_t>(n_same / Bc, s_cap);
    if (S < 2) return false;
    slice_skip = i0 + (uint64_t)S * Bc;  // unless the group completes
    G.i0 = i0;
    G.S = S;
    G.Bc = Bc;
    G.bs.resize(S);
    G.spub.resize((size_t)S * Bc);
    G.lpub.resize((size_t)S * Bc);
    G.stp.resize((size_t)S * Bc);
    for (uint32_t j = 0; j < S; j++) {
      const uint64_t q0 = i0 + (uint64_t)j * Bc;
      G.bs[j] = setup_batch(c, sched, q0, q0 + Bc, j == 0);
      for (uint32_t q = 0; q < Bc; q++) {
        G.lpub[(size_t)j * Bc + q] = sched[q0 + q].publisher;
        G.spub[(size_t)j * Bc + q] = sched[q0 + q].publisher + j * N;
      }
      std::copy(G.bs[j].tpub.begin(), G.bs[j].tpub.end(), G.stp.begin() + (size_t)j * Bc);
    }
    G.g = G.bs[0];  // the slices' keys: the source field holds slice rows (S x N ids)
    G.g.sb = bits_for(S * N);
    G.g.tshift = G.g.sb + HOP_BITS;
    G.g.tmax = G.g.tshift >= 64 ? 0 : (INF64 >> G.g.tshift);
    for (Batch& bj : G.bs) {
      bj.sb = G.g.sb;
      bj.tshift = G.g.tshift;
      bj.tmax = G.g.tmax;
    }
    // lazy gossip: every message's first heartbeat (the group's IHAVE / IWANT inside the
    // passes need them all the same time after their publishes)
    G.rel.resize(G.stp.size());
    G.hab.resize(G.stp.size());
    if (gossip)
      for (size_t q = 0; q < G.stp.size(); q++) {
        const HbPos hp = hb_pos(c, G.stp[q]);
        G.rel[q] = hp.rel0;
        G.hab[q] = hp.h0;
      }
    G.wants = sw.rows() || sw.lat || sw.summary;
    return true;
  }

  // The group from i0 as one pass, if one forms and its plan lets it run; else
  // (false) single batches take the messages before slice_skip.
  bool try_slices(uint64_t i0, uint64_t& i_end) {
    SliceGroup G;
    if (!form_slices(i0, G)) return false;
    G.p = plan(G.g, G.rel.data(), G.rel.size(), true);
    if (G.p.idw || !G.p.lp) return false;  // (IDONTWANT; a window below the grain)
    if (gossip && c.glp_prefer && !G.p.glp) return false;  // single batches (the push path)
    hipStream_t s = c.stream;
    const size_t NR = (size_t)G.S * N;
    c.d_spub.alloc(G.spub.size());
    c.d_lpub.alloc(G.lpub.size());
    c.d_stpub.alloc(G.stp.size());
    GS_HIP(hipMemcpyAsync(c.d_spub.p, G.spub.data(), G.spub.size() * 4, hipMemcpyHostToDevice, s));
    GS_HIP(hipMemcpyAsync(c.d_lpub.p, G.lpub.data(), G.lpub.size() * 4, hipMemcpyHostToDevice, s));
    GS_HIP(hipMemcpyAsync(c.d_stpub.p, G.stp.data(), G.stp.size() * 8, hipMemcpyHostToDevice, s));
    c.d_keys.alloc(NR * G.g.L);
    if (G.g.FP > 1) c.d_busy.alloc(NR * G.Bc);
    G.sl = Slices{G.S, N, c.d_spub.p, c.d_lpub.p};
    if (!(gossip && c.glp_prefer ? slices_glp(G) : slices_eager(G))) return false;
    GS_HIP(hipStreamSynchronize(s));  // (lpub / tpub / habs0 host copies die here)
    c.stats.messages += (uint64_t)G.S * G.Bc;
    c.stats.batches += G.S;
    i_end = i0 + (uint64_t)G.S * G.Bc;
    return true;
  }

  void slices_fresh(const SliceGroup& G) {  // per-run state of the group's pass
    c.keys_log = c.keys_none = false;
    if (G.g.FP > 1) GS_HIP(hipMemsetAsync(c.d_busy.p, 0, (size_t)G.S * N * G.Bc * 8, c.stream));
  }
  // every slice's completion for the sink: its publishers and publish times where completion reads them
  void slices_deliver(const SliceGroup& G) {
    hipStream_t s = c.stream;
    for (uint32_t j = 0; j < G.S; j++) {
      GS_HIP(hipMemcpyAsync(c.d_pub.p, G.lpub.data() + (size_t)j * G.Bc, G.Bc * 4, hipMemcpyHostToDevice, s));
      GS_HIP(hipMemcpyAsync(c.d_tpub.p, G.bs[j].tpub.data(), G.Bc * 8, hipMemcpyHostToDevice, s));
      launch_complete(c, G.bs[j], 0, N, sink, G.i0 + (uint64_t)j * G.Bc, (size_t)j * N);
    }
  }
  // The slices' counters (mstat: and their per-message reductions, every slice's into
  // c.h_slms): one launch over the final log, else one per slice.
  void slices_count(const SliceGroup& G, bool mstat) {
    hipStream_t s = c.stream;
    const uint32_t S = G.S, Bc = G.Bc;
    if (c.keys_log) {
      run_complete(c, G.bs[0], 0, N, mstat, false, false, false, 0, c.d_lpub.p, c.d_stpub.p, S);
      if (mstat) GS_HIP(hipMemcpyAsync(c.h_slms, c.d_mstat.p, (size_t)S * Bc * MS_COLS * 8, hipMemcpyDeviceToHost, s));
      return;
    }
    for (uint32_t j = 0; j < S; j++) {
      run_complete(c, G.bs[j], 0, N, mstat, false, false, false, (size_t)j * N, c.d_lpub.p + (size_t)j * Bc,
                   c.d_stpub.p + (size_t)j * Bc);
      if (mstat)
        GS_HIP(hipMemcpyAsync(c.h_slms + (size_t)j * Bc * MS_COLS, c.d_mstat.p, (size_t)Bc * MS_COLS * 8,
                              hipMemcpyDeviceToHost, s));
    }
  }
  void slices_finish(const SliceGroup& G) {  // completion of a group whose keys stand
    if (!G.wants) slices_count(G, false);    // device-resident results: the counters only
    else slices_deliver(G);
  }

  // The group with the gossip inside its passes.
  bool slices_glp(const SliceGroup& G) {
    hipStream_t s = c.stream;
    const uint64_t grain = pull_grain(G.g.tshift);
    const Batch gg = with_window(G.g, G.p.win_gos);
    uint32_t lb = 0;
    const uint32_t K = lpull_ring(c, gg, gg.delta / grain * grain, &lb, true, false, G.S * N);
    if (!K) return false;
    slices_fresh(G);
    c.d_habs0.alloc(std::max<size_t>(Bmax, G.hab.size()));
    GS_HIP(hipMemcpyAsync(c.d_habs0.p, G.hab.data(), G.hab.size() * 8, hipMemcpyHostToDevice, s));
    const GosRun gr{G.rel[0], c.cfg.heartbeat_ns};
    const uint64_t iw0 = read_counter(c, C_GOSSIP);
    LpOpts o = G.p.opts();
    o.gos = &gr;
    o.sl = &G.sl;
    if (!run_lpull_batch(c, gg, K, lb, o)) return false;
    c.stats.list_pull_batches += G.S - 1;
    c.stats.gossip_list_batches += G.S;
    glp_account(c, iw0, G.S);
    slices_finish(G);
    return true;
  }

  // The group on the eager pass; with lazy gossip its result stands only if gossip is a
  // no-op in every slice, else the gossip inside the passes takes the group (when admitted).
  bool slices_eager(const SliceGroup& G) {
    hipStream_t s = c.stream;
    const uint32_t S = G.S, Bc = G.Bc;
    const uint64_t grain = pull_grain(G.g.tshift);
    uint32_t lb = 0;
    const uint32_t K = lpull_ring(c, G.g, G.p.win / grain * grain, &lb, false, false, S * N);
    if (!K) return false;
    slices_fresh(G);
    if (gossip) GS_HIP(hipMemcpyAsync(c.d_cnt_save.p, c.d_counters.p, C_COUNT * 8, hipMemcpyDeviceToDevice, s));
    LpOpts o = G.p.opts();
    o.sl = &G.sl;
    if (!run_lpull_batch(c, G.g, K, lb, o)) return false;  // (a list overflowed: counters restored)
    c.stats.list_pull_batches += S - 1;
    if (!gossip) {
      slices_finish(G);
      return true;
    }
    // every slice's reductions into one pinned buffer, one wait
    const size_t msb = (size_t)S * Bc * MS_COLS * 8;
    if (c.h_slms_bytes < msb) {
      if (c.h_slms) GS_HIP(hipHostFree(c.h_slms));
      c.h_slms = nullptr;
      c.h_slms_bytes = 0;
      GS_HIP(hipHostMalloc((void**)&c.h_slms, msb, hipHostMallocDefault));
      c.h_slms_bytes = msb;
    }
    slices_count(G, true);
    GS_HIP(hipStreamSynchronize(s));
    bool noop = true;
    for (uint32_t j = 0; j < S && noop; j++) {
      const std::vector<uint64_t> r0(G.rel.begin() + (size_t)j * Bc, G.rel.begin() + (size_t)(j + 1) * Bc);
      noop = gossip_noop(G.bs[j], c.h_slms + (size_t)j * Bc * MS_COLS, r0);
    }
    if (noop) {
      c.stats.gossip_noop_msgs += (uint64_t)S * Bc;
      if (G.wants) {  // the sink's results: completion again per slice, its counters not counted twice
        c.d_cnt_save2.alloc(C_COUNT);
        GS_HIP(hipMemcpyAsync(c.d_cnt_save2.p, c.d_counters.p, C_COUNT * 8, hipMemcpyDeviceToDevice, s));
        slices_deliver(G);
        GS_HIP(hipMemcpyAsync(c.d_counters.p, c.d_cnt_save2.p, C_COUNT * 8, hipMemcpyDeviceToDevice, s));
      }
      return true;
    }
    // gossip changes the group: discard the eager run
    GS_HIP(hipMemcpyAsync(c.d_counters.p, c.d_cnt_save.p, C_COUNT * 8, hipMemcpyDeviceToDevice, s));
    c.stats.list_pull_batches -= S;
    if (!G.p.glp) return false;  // (the single batches take it: they count their own fallbacks)
    c.stats.gossip_fallback_batches++;
    c.glp_prefer = true;
    c.glp_quiet = 0;
    return slices_glp(G);
  }

  // ---- one batch ----

  // The batch from i0: form it, prepare its churn and gossip inputs, plan, run the
  // planned paths in PathPlan's order, count. Returns its end.
  uint64_t run_batch(uint64_t i0) {
    BatchRun r;
    r.i0 = i0;
    r.i1 = form(i0, r.h_lo, r.h_hi);
    r.b = setup_batch(c, sched, r.i0, r.i1);
    const uint32_t B = r.b.B;
    for (uint32_t q = 0; q < B && (churn || gossip); q++) {
      const HbPos hp = hb_pos(c, r.b.tpub[q]);
      if (churn) q0v[q] = hp.ep, r0v[q] = hp.off;
      if (gossip) rel0[q] = hp.rel0, habs0[q] = hp.h0;
    }
    r.p = plan(r.b, rel0.data(), B, false);
    r.p.chn = churn && chn_admit(r.b, r.p, r0v.data(), r.h_lo, r.h_hi);
    if (churn) prepare_churn(r);
    if (gossip) prepare_gossip(r);
    bool done = false;
    if (r.p.chn) done = run_churn_list(r);  // (a list overflow falls back to the push path)
    if (r.p.glp && c.glp_prefer) done = run_glp(r);
    // Lazy gossip on a frozen mesh: run eager forwarding first (the pull pass,
    // or the push path without gossip when IDONTWANT needs it) and keep it if
    // the batch proves gossip a no-op; otherwise discard its counters and run
    // the gossip inside the list pass, or the push path with gossip (DESIGN.md
    // §2.7). Under churn some peers never complete, so the proof cannot hold
    // and gossip runs directly.
    if (!done && (r.p.pull || (gossip && !churn))) {
      if (gossip) GS_HIP(hipMemcpyAsync(c.d_cnt_save.p, c.d_counters.p, C_COUNT * 8, hipMemcpyDeviceToDevice, c.stream));
      run_eager(r);
      done = !gossip ? finish_eager(r) : gossip_proof(r);
    }
    if (!done) {
      if (getenv("GS_REQUIRE_LPULL")) c.fail(GS_EUNSUPPORTED, "the push path would take this batch (GS_REQUIRE_LPULL)");
      if (gossip && !lanes32)
        c.fail(GS_EUNSUPPORTED, "lazy gossip changes this batch and the push path needs "
                                "peers*batch*FP < 2^32: use a smaller batch");
      run_push_batch(c, r.b, push_form(gossip || churn), gossip, r.g0, max_tiles);
      complete(r);
    }
    c.stats.messages += B;
    c.stats.batches++;
    return r.i1;
  }

  void complete(const BatchRun& r) {
    if (c.keys_pass()) launch_key_passes(c, r.b, r.i0);
    launch_complete(c, r.b, 0, N, sink, r.i0);
  }

  // churn: the ring holds the batch's epochs; a churn list-pass batch's tables (r.cp), from
  // the chain ahead when it prepared this batch, else built beside the epochs here.
  void prepare_churn(BatchRun& r) {
    hipStream_t s = c.stream;
    const bool chn = r.p.chn;
    const uint64_t h_lo = r.h_lo, h_end = r.h_hi + c.cfg.churn_horizon;
    if (ah.on && !(chn && ah.i0 == r.i0 && ah.i1 == r.i1)) {  // (not expected: batches form the same way)
      ah.join();
      ah.drop();
    }
    if (ah.on) {  // this batch's chain and tables ran ahead beside the last batch's passes
      ah.join();
      r.cp = ah.cp;
      ah.drop();
    } else {
      {
        ChurnDefer defer(c, chn);
        if (chn) {
          c.ct_par ^= 1u;
          chn_begin(c, r.cp, c.ct_par, s, h_lo, (uint32_t)(h_end - h_lo + 1), q0v.data(), sched + r.i0, r.b.B, r.b.FP);
          r.cp.s = nullptr;  // (the chunk events go where churn_ring runs the chain)
          c.epoch_hook = [&](uint64_t h) { chn_chunks(c, r.cp, h, false); };
        }
        churn_ring(c, h_lo, h_end);
      }
      // readers of the ELL snapshots beside the list pass: seeds to the mesh (no flood
      // publish), the per-peer traffic pass, the GS_DEBUG_CHN check
      if (chn && (!c.cfg.flood_publish || c.keys_pass() || getenv("GS_DEBUG_CHN"))) ensure_ring_ell(c, h_lo, h_end);
      //  a batch for the push path may overlap the last epochs of an
      // earlier churn list-pass batch, which skipped their ELL snapshots and
      // inverse IHAVE lists: rebuild those slots (tag-checked: free when current)
      if (!chn) {
        ensure_ring_ell(c, h_lo, h_end);
        if (gossip) ensure_in_lists(c, h_lo, h_end);
      }
      if (chn) chn_end(c, r.cp);
    }
    c.d_q0.alloc(Bmax);
    c.d_r0.alloc(Bmax);
    GS_HIP(hipMemcpyAsync(c.d_q0.p, q0v.data(), r.b.B * 8, hipMemcpyHostToDevice, s));
    GS_HIP(hipMemcpyAsync(c.d_r0.p, r0v.data(), r.b.B * 8, hipMemcpyHostToDevice, s));
    GS_HIP(hipStreamSynchronize(s));
  }

  // lazy gossip: the first heartbeat at or after each t_pub, on the device; churn: which
  // messages gossip can spread at all, and the earliest IHAVE arrival g0
  void prepare_gossip(BatchRun& r) {
    hipStream_t s = c.stream;
    const uint32_t B = r.b.B;
    c.d_rel0.alloc(Bmax);
    c.d_habs0.alloc(Bmax);
    GS_HIP(hipMemcpyAsync(c.d_rel0.p, rel0.data(), B * 8, hipMemcpyHostToDevice, s));
    GS_HIP(hipMemcpyAsync(c.d_habs0.p, habs0.data(), B * 8, hipMemcpyHostToDevice, s));
    if (churn) {  // per message: gossip can spread it (publisher online at t_pub, a heartbeat in its lifetime)
      for (uint32_t q = 0; q < B; q++) {
        malive[q] = habs0[q] <= q0v[q] + c.cfg.churn_horizon &&
                    !c.offline(sched[r.i0 + q].publisher, q0v[q]);
        r.g0 = std::min(r.g0, rel0[q]);
      }
      uint64_t lmin = INF64;
      for (uint64_t l : c.lat_ns) lmin = std::min(lmin, l);
      r.g0 += lmin;
      c.d_malive.alloc(Bmax);
      GS_HIP(hipMemcpyAsync(c.d_malive.p, malive.data(), B, hipMemcpyHostToDevice, s));
    }
    GS_HIP(hipStreamSynchronize(s));  // rel0 / habs0 host vectors are rewritten by the next batch
  }

  // The chain ahead for the batch from n0, if it is a churn list-pass batch past the ring's state.
  void ahead_start(uint64_t n0) {
    if (!pipe_on || ah.on || n0 >= n_msgs) return;
    uint64_t hl = 0, hh = 0;
    const uint64_t n1 = form(n0, hl, hh);
    const Batch b2 = setup_batch(c, sched, n0, n1, false);
    for (uint32_t q = 0; q < b2.B; q++) {
      const HbPos hp = hb_pos(c, b2.tpub[q]);
      q0a[q] = hp.ep;
      r0a[q] = hp.off;
    }
    const uint64_t h1 = hh + c.cfg.churn_horizon;
    if (!chn_admit(b2, plan(b2, nullptr, 0, false), r0a.data(), hl, hh) || h1 <= c.churn_state) return;
    ah.start(n0, n1, hl, h1, q0a.data(), sched + n0, b2.B, b2.FP);
  }

  // Churn on the list pass. When it cannot take the batch or loses it (false): the ring
  // as the push path reads it.
  bool run_churn_list(BatchRun& r) {
    const Batch& b = r.b;
    const uint64_t h_lo = r.h_lo, h_end = r.h_hi + c.cfg.churn_horizon;
    bool done = false;
    uint32_t lb = 0;
    const Batch bc = with_window(b, r.p.win_chn);
    const uint64_t grain = pull_grain(b.tshift);
    const uint32_t K = lpull_ring(c, bc, bc.delta / grain * grain, &lb, gossip, true);
    if (K) {
      reset_keys(c, b, false);
      const GosRun gr{rel0[0], c.cfg.heartbeat_ns};
      const ChnRun cr{h_lo, r0v[0], (uint32_t)(h_end - h_lo + 1), gossip ? (uint32_t)(habs0[0] - q0v[0]) : 0u, r.cp.par};
      // the next batch's chain beside these passes, from the first pass group on:
      // the seeds (k_seed reads this batch's offline bits in the ring) are
      // enqueued by then, and the chain's stream waits for them
      bool ah_tried = false;
      std::function<void()> between;
      if (pipe_on) between = [&] {
        if (!ah_tried) {
          ah_tried = true;
          ahead_start(r.i1);
        } else {
          ah.pump(false);
        }
      };
      PassPoll poll(c, std::move(between));
      LpOpts o = r.p.opts();
      o.gos = gossip ? &gr : nullptr;
      o.chn = &cr;
      if (run_lpull_batch(c, bc, K, lb, o)) {
        if (gossip) c.stats.gossip_list_batches++;
        complete(r);
        done = true;
      }
    }
    if (done) return true;
    if (getenv("GS_REQUIRE_LPULL")) c.fail(GS_EUNSUPPORTED, "churn list pass cannot take this batch (GS_REQUIRE_LPULL)");
    // the push path reads the ring: a chain ahead (of this batch or for the next one)
    // may have run past or overwritten this batch's slots, or a replay moved the ring
    ah.join();
    churn_ring(c, h_lo, h_end);  // (no epochs when current; else runs / replays them)
    // a replay ended at this batch's last epoch: the ring slots of the prepared batch's later
    // epochs (its seeds read their offline bits) hold older epochs again and the mesh state is
    // behind its tables. The prepared batch is dropped and prepares in line (chn_begin into the
    // other table set, which this batch's list pass has left; churn_ring runs the epochs again).
    // The join above enqueued the whole chain and churn_ring waited for its stream.
    if (ah.on && c.churn_state < ah.h1) {
      if (Ahead::debug())
        fprintf(stderr, "[ah] batch %llu: dropped (the fallback's replay left the ring at epoch %llu of %llu)\n",
                (unsigned long long)ah.i0, (unsigned long long)c.churn_state, (unsigned long long)ah.h1);
      ah.drop();
    }
    ensure_ring_ell(c, h_lo, h_end);  // the push path reads the ELL ring
    if (gossip) ensure_in_lists(c, h_lo, h_end);
    return false;
  }

  // The batch with the gossip inside the list pass (false: no ring fits, or a list overflowed).
  bool run_glp(BatchRun& r) {
    const Batch& b = r.b;
    r.glp_tried = true;
    const Batch bg = with_window(b, r.p.win_gos);
    const uint64_t grain = pull_grain(b.tshift);
    uint32_t lb = 0;
    const uint32_t K = lpull_ring(c, bg, bg.delta / grain * grain, &lb, true);
    if (!K) return false;
    reset_keys(c, b, r.p.idw);  // IDONTWANT: dense INF keys (the finals stay dense rows)
    const GosRun gr{rel0[0], c.cfg.heartbeat_ns};
    const uint64_t iw0 = read_counter(c, C_GOSSIP);
    LpOpts o = r.p.opts();
    o.gos = &gr;
    if (!run_lpull_batch(c, bg, K, lb, o)) return false;
    c.stats.gossip_list_batches++;
    glp_account(c, iw0, 1);
    complete(r);
    return true;
  }

  // Eager forwarding: the list pass (no-log when the plan allows and a ring fits), behind
  // it k_pull, or the push path where IDONTWANT needs it; without the pull path the push path.
  void run_eager(BatchRun& r) {
    const Batch& b = r.b;
    const PathPlan& p = r.p;
    if (!p.pull) return run_push_batch(c, b, push_form(false), false, r.g0, max_tiles);
    const uint64_t grain = pull_grain(b.tshift);
    uint32_t lb = 0;
    const Batch bw = with_window(b, p.win);
    const uint32_t K = p.lp ? lpull_ring(c, bw, bw.delta / grain * grain, &lb) : 0u;
    reset_keys(c, b, K == 0 || p.idw);  // IDONTWANT: dense INF keys
    if (p.lp && !K && getenv("GS_REQUIRE_LPULL"))  // test knob: no silent k_pull fallback
      c.fail(GS_EUNSUPPORTED, "list pull path cannot take this batch (GS_REQUIRE_LPULL)");
    r.nl.on = K && p.nolog;
    LpOpts o = p.opts();
    o.nl = &r.nl;
    bool lp_ok = K && run_lpull_batch(c, bw, K, lb, o);
    if (!lp_ok && r.nl.inexact) {  // the same pass again with its log (k_lsum's 64-bit ms)
      r.nl = NoLog{};
      lp_ok = run_lpull_batch(c, bw, K, lb, o);
    }
    if (lp_ok) return;
    r.nl.on = false;
    if (K && getenv("GS_REQUIRE_LPULL")) c.fail(GS_EUNSUPPORTED, "list pull overflow (GS_REQUIRE_LPULL)");
    if (p.idw) {  // k_pull has no IDONTWANT: the push path takes the batch
      run_push_batch(c, b, push_form(false), false, r.g0, max_tiles);
    } else {  // a candidate list overflowed (or no ring fits): this batch runs on k_pull
      if (K) reset_keys(c, b, true);
      run_pull_batch(c, b);
    }
  }

  // Without lazy gossip the eager result is the batch's.
  bool finish_eager(const BatchRun& r) {
    if (c.keys_pass()) launch_key_passes(c, r.b, r.i0);
    if (!r.nl.on) launch_complete(c, r.b, 0, N, sink, r.i0);  // (a no-log batch: the passes completed it)
    return true;
  }

  // Lazy gossip: keep the eager result only if gossip provably changes nothing (true);
  // else its counters are discarded and, when the plan admits it and it was not tried
  // yet, the batch runs again with the gossip inside the list pass.
  bool gossip_proof(BatchRun& r) {
    hipStream_t s = c.stream;
    const Batch& b = r.b;
    const uint32_t B = b.B;
    const bool lockstep = r.p.lockstep;
    // a lockstep batch (one rel0): a message has at most N - 1 deliveries, so the batch's
    // total is reached only when none is undelivered, and the largest of the messages'
    // latest times is the batch's; the per-message test is then a test of these two
    bool noop;
    if (r.nl.on) {  // the two values came with the last pass group's control words
      noop = r.nl.deliv == (uint64_t)B * (N - 1) && r.nl.tmax < rel0[0] + b.lat_min;
    } else {
      const bool bsum = batch_sums(c, b, true, sw.lat, 1, lockstep);
      run_complete(c, b, 0, N, true, sw.summary, sw.rows() || sw.summary, sw.lat, 0, nullptr, nullptr, 1, lockstep);
      std::vector<uint64_t> ms(bsum ? 2 : (size_t)B * MS_COLS);
      GS_HIP(hipMemcpyAsync(ms.data(), c.d_mstat.p, ms.size() * 8, hipMemcpyDeviceToHost, s));
      GS_HIP(hipStreamSynchronize(s));
      noop = bsum ? ms[0] == (uint64_t)B * (N - 1) && ms[1] < rel0[0] + b.lat_min : gossip_noop(b, ms.data(), rel0);
    }
    if (noop) {
      if (c.keys_pass()) launch_key_passes(c, b, r.i0);
      deliver(c, b, 0, N, sink, r.i0);
      c.stats.gossip_noop_msgs += B;
      return true;
    }
    // gossip can change this batch: discard the eager run's counters
    GS_HIP(hipMemcpyAsync(c.d_counters.p, c.d_cnt_save.p, C_COUNT * 8, hipMemcpyDeviceToDevice, s));
    c.stats.gossip_fallback_batches++;
    if (!r.p.glp || r.glp_tried) return false;
    c.glp_prefer = true;  // the context's later batches go there directly (no eager run first)
    c.glp_quiet = 0;
    return run_glp(r);
  }
};
