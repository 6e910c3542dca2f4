// gs_prun.h — the driver of gs_run_partitioned(_log): one PRun per call, one
// short function per step, one function per exchange with its loop-back body
// (device copies between this process's parts) next to its rank body (grouped
// send / recv through the coll_* wrappers). Included by gs_comm.hip after the
// wrappers, as gs_relax.hip includes gs_run.h. DESIGN.md §5.4 says which path
// a batch takes and which exchange it uses.
#pragma once

namespace {

// Bytes per ncclSend / ncclRecv piece of the record exchange: 2^30 by default
// (DESIGN.md §5); GS_RCCL_PIECE_BYTES lowers it (tests force many pieces).
uint64_t rccl_piece_bytes() {  // read per batch: tests change it between runs
  const long x = env_int("GS_RCCL_PIECE_BYTES", 0);
  return x > 0 ? std::min<uint64_t>((uint64_t)x, 1ull << 30) : (1ull << 30);
}

// A part's share of a message-sharded batch runs through gs_run's engine with
// four context fields overridden; they come back however the share ends.
struct MsShare {
  Ctx& c;
  const uint32_t batch;
  const Ctx::TextRun text;
  const bool pdelay;
  MsShare(Ctx& ctx, uint32_t share) : c(ctx), batch(ctx.cfg.batch), text(ctx.text), pdelay(ctx.pdelay) {
    c.cfg.batch = share;  // buffers for this part's share, not the whole batch
    c.sink_dev = true;
    c.text = Ctx::TextRun{};  // (the log's text is of the own peers' rows, after the exchange)
    c.pdelay = false;         // (and so are the delay accumulators' observations: part_lat_stage)
  }
  ~MsShare() {
    c.cfg.batch = batch;
    c.sink_dev = false;
    c.text = text;
    c.pdelay = pdelay;
  }
};

struct PRun;

// The record exchange of a list-pass batch, decided once per batch: routed per
// destination part (at most PART_ROUTE_PMAX parts), or every part's records
// to every part (gathered). Loop-back parts on one device route by default,
// each part's pack storing straight into the destination contexts (direct: no
// copies); ranks gather by default. GS_PART_ROUTE = 1 / 0 forces routed /
// gathered (loop-back routed then goes through send segments and copies, as
// ranks do, when GS_PART_DIRECT=0). dev_ctl: loop-back parts on one device
// also combine their pass control on the device (part_lp_combine).
struct LpExchange {
  bool one_dev, routed, direct, dev_ctl;
  explicit LpExchange(const PRun& r);
};

// One gs_run_partitioned call over this process's parts (the counterpart of
// Run, gs_run.h): nctx contexts of a loop-back communicator, or this rank's one.
struct PRun {
  gs_comm* cm;
  Ctx** cx;
  uint32_t nctx;
  const gs_publish* sched;
  const gs_result_sink* sinks;
  // the batch in progress: messages [i0, i0 + B) over P parts of N peers
  uint64_t i0 = 0;
  uint32_t B = 0, P = 0, N = 0;
  PartLayout lay{};
  uint64_t pb = 0;            // rccl_piece_bytes() of the batch
  std::vector<uint64_t> ctl;  // push: every part's bucket key as the host read it

  // ---- helpers ----
  uint32_t me(uint32_t i) const { return cm->local ? i : cm->rank; }  // the part context i holds
  const gs_result_sink* sink(uint32_t i) const { return sinks ? &sinks[i] : nullptr; }
  // A part stages its latencies for its sink's on_lat (or the text), or for its delay accumulators.
  bool wants_lat(uint32_t i) const { return cx[i]->pdelay || (sinks && sinks[i].on_lat); }

  // f(i, context i) on every part with its device current. "Enqueue on every
  // part, then wait on every part" is two calls.
  template <class F>
  void each(F&& f) {
    for (uint32_t i = 0; i < nctx; i++) {
      GS_HIP(hipSetDevice(cx[i]->cfg.device));
      f(i, *cx[i]);
    }
  }

  // Ranks agree on one word, MIN or MAX (an all-reduce through the scratch's
  // flag word on context 0's stream); loop-back parts hold it already.
  uint64_t agree(uint64_t word, ncclRedOp_t op) {
    if (cm->local) return word;
    Ctx& c = *cx[0];
    uint64_t* w = cm->scratch_flag();
    c.h_pinned[0] = word;
    GS_HIP(hipMemcpyAsync(w, c.h_pinned, 8, hipMemcpyHostToDevice, c.stream));
    coll_AllReduce(cm, w, w, 1, ncclUint64, op, c.stream);
    GS_HIP(hipMemcpyAsync(c.h_pinned, w, 8, hipMemcpyDeviceToHost, c.stream));
    GS_HIP(hipStreamSynchronize(c.stream));
    return c.h_pinned[0];
  }

  // The rank guard: a rank that fails f makes every rank fail the call (a
  // status word, MAX) instead of leaving the others waiting in a collective;
  // the error text names the reason only on the failing rank. Loop-back parts
  // share one thread: f's error just leaves.
  template <class F>
  void guarded(F&& f) {
    if (cm->local) return f();
    std::string why;
    gs_status code = GS_OK;
    try {
      f();
    } catch (const Error& e) {
      code = e.code;
      why = e.msg;
    }
    const uint64_t any = agree(code != GS_OK, ncclMax);
    if (code != GS_OK) throw Error(code, why);
    if (any) throw Error(GS_EINVAL, "another rank failed this partitioned call");
  }

  // Every rank's n words (n <= HP_GATHER_WORDS) -> out[rank * n + k] on the host, through the
  // scratch's control rows; loop-back: the one row is the caller's. Returns the rows.
  uint32_t gather(const uint64_t* mine, uint32_t n, uint64_t* out) {
    if (cm->local) {
      memcpy(out, mine, n * 8);
      return 1;
    }
    Ctx& c = *cx[0];
    uint64_t* w = cm->scratch_ctl();
    memcpy(c.h_pinned + HP_GATHER, mine, n * 8);
    GS_HIP(hipMemcpyAsync(w + (size_t)cm->rank * n, c.h_pinned + HP_GATHER, n * 8, hipMemcpyHostToDevice, c.stream));
    coll_AllGather(cm, w + (size_t)cm->rank * n, w, n, ncclUint64, c.stream);
    std::vector<uint64_t> h((size_t)cm->nranks * n);
    GS_HIP(hipMemcpyAsync(h.data(), w, h.size() * 8, hipMemcpyDeviceToHost, c.stream));
    GS_HIP(hipStreamSynchronize(c.stream));
    memcpy(out, h.data(), h.size() * 8);
    return cm->nranks;
  }

  // Timing (gs_set_timing): events from the context's pool (run_ev) under its
  // cursor ev_n, which each peer path starts at 0. The list pass records a pair
  // around every pass; push a triple per bucket on the part's stream — bucket
  // start, scan + counts done (scan_ms), relax done (frontier_ms: the routed
  // export, the exchange and the receive-side relaxation).
  void timing_reset() {
    for (uint32_t i = 0; i < nctx; i++) cx[i]->ev_n = 0;
  }
  void mark(Ctx& c) {
    if (c.timing) GS_HIP(hipEventRecord(run_ev(c, c.ev_n++), c.stream));
  }
  // The path's events into the stats: per group of `stride` events the last
  // two bound frontier time, and of a triple the first two scan time.
  void total_times(size_t stride) {
    each([&](uint32_t, Ctx& c) {
      if (!c.timing) return;
      GS_HIP(hipStreamSynchronize(c.stream));
      auto between = [&](size_t a) {
        float x = 0;
        GS_HIP(hipEventElapsedTime(&x, c.ev_pool[a], c.ev_pool[a + 1]));
        return x;
      };
      double scan = 0, front = 0;
      for (size_t q = 0; q + stride - 1 < c.ev_n; q += stride) {
        if (stride == 3) scan += between(q);
        front += between(q + stride - 2);
      }
      if (stride == 3 && c.ev_n % 3 == 2) scan += between(c.ev_n - 2);  // the last scan, which found no bucket left
      c.stats.scan_ms += scan;
      c.stats.frontier_ms += front;
      c.stats.relax_ms += scan + front;
    });
  }

  // One transfer of n elements in pieces of at most pb bytes, cut at whole
  // elements; both ends cut the same count the same way. 8-byte elements
  // travel as ncclUint64, every other size as its bytes.
  template <class T, class Fn>
  void pieces(T* p, uint64_t n, Fn&& xfer) {
    constexpr bool word = sizeof(T) == 8;
    const uint64_t piece = std::max<uint64_t>(1, pb / sizeof(T));
    for (uint64_t k = 0; k < n; k += piece)
      xfer(p + k, std::min(piece, n - k) * (word ? 1 : sizeof(T)), word ? ncclUint64 : ncclUint8);
  }
  template <class T>
  void send_pieces(const T* p, uint64_t n, uint32_t peer) {
    pieces(p, n, [&](const T* q, size_t k, ncclDataType_t t) { coll_Send(cm, q, k, t, (int)peer, cx[0]->stream); });
  }
  template <class T>
  void recv_pieces(T* p, uint64_t n, uint32_t peer) {
    pieces(p, n, [&](T* q, size_t k, ncclDataType_t t) { coll_Recv(cm, q, k, t, (int)peer, cx[0]->stream); });
  }

  // Every rank must run the same protocol: the knobs that decide the batches
  // and the collectives they enter are compared across ranks (MIN and MAX of
  // each word agree) before the first batch.
  void check_same_config(uint64_t n_msgs, uint64_t lat) {
    if (cm->local) return;
    Ctx& c = *cx[0];
    // FNV-1a over the schedule, and whether the sink takes the u16 latencies (bit 0) or the delay
    // accumulators do (bit 1: gs_set_peer_delay) — lat_gate's collective
    uint64_t h = (1469598103934665603ull ^ lat) * 1099511628211ull;
    for (uint64_t i = 0; i < n_msgs; i++) {
      const uint64_t v[4] = {sched[i].t_pub_ns, sched[i].publisher, sched[i].msg_size, sched[i].frags};
      for (uint64_t x : v) h = (h ^ x) * 1099511628211ull;
    }
    if (c.topo_fp) h = (h ^ c.topo_fp) * 1099511628211ull;  // an imported graph's fingerprint (0: the built one)
    if (c.mesh_fp) h = (h ^ c.mesh_fp) * 1099511628211ull;  // an imported mesh's (0: a converged one)
    if (c.outage_fp) h = (h ^ c.outage_fp) * 1099511628211ull;  // an imported outage schedule's (0: the draw)
    const uint64_t sig[8] = {c.cfg.peers, c.cfg.batch, c.cfg.lazy_gossip, c.cfg.idontwant,
                             c.cfg.churn_ppm, c.cfg.fragments, c.cfg.seed, h ^ n_msgs};
    static_assert(2 * sizeof sig <= HP_SCRATCH * 8, "the MIN and MAX rows in the mirror's scratch words");
    DevBuf<uint64_t> d;
    d.alloc(16);
    memcpy(c.h_pinned, sig, sizeof sig);
    GS_HIP(hipMemcpyAsync(d.p, c.h_pinned, sizeof sig, hipMemcpyHostToDevice, c.stream));
    GS_HIP(hipMemcpyAsync(d.p + 8, c.h_pinned, sizeof sig, hipMemcpyHostToDevice, c.stream));
    coll_AllReduce(cm, d.p, d.p, 8, ncclUint64, ncclMin, c.stream);
    coll_AllReduce(cm, d.p + 8, d.p + 8, 8, ncclUint64, ncclMax, c.stream);
    GS_HIP(hipMemcpyAsync(c.h_pinned, d.p, 16 * 8, hipMemcpyDeviceToHost, c.stream));
    GS_HIP(hipStreamSynchronize(c.stream));
    for (int k = 0; k < 8; k++)
      if (c.h_pinned[k] != c.h_pinned[8 + k])
        throw Error(GS_EINVAL, "RCCL ranks disagree on the partitioned run (peers, batch, lazy_gossip, idontwant, "
                               "churn, fragments, seed, schedule, the imported graph, the latency stream or gs_set_peer_delay, "
                               "the imported mesh, the imported outages)");
  }

  // ---- the u16 latencies of a batch ----
  // They leave (a sink's on_lat, or the log's text) only when no part and no
  // rank failed the batch: the staged parts' error words (part_lat_stage),
  // combined over the ranks with the pass control's all-gather, before the
  // first hand-over. Every rank then fails the call alike, and none is left
  // waiting in the next batch's collectives.
  void lat_gate() {
    uint64_t err = 0, all[64];
    each([&](uint32_t, Ctx& c) {
      if (c.lat_staged) err |= part_lat_err(c);
    });
    const uint32_t rows = gather(&err, 1, all);
    for (uint32_t k = 0; k < rows; k++) err |= all[k];
    if (err & ERR_LAT16)
      throw Error(GS_ERANGE, "a logged latency of 65535 ms or more does not fit the u16 latencies (GS_WANT_LAT_MS, "
                             "the arrival log's text)");
    if (err) throw Error(GS_ERANGE, "arrival log: a peer's line counter would pass 2^32 - 1");
  }
  // Every part that hands out latencies stages the finished batch (ms_sched:
  // the schedule rows of a message-sharded one), then the gate. Returns whether any did.
  bool lat_stage_all(const gs_publish* ms_sched) {
    bool any = false;
    each([&](uint32_t i, Ctx& c) {
      if (!wants_lat(i)) return;
      part_lat_stage(c, B, ms_sched);
      any = true;
    });
    if (any) lat_gate();
    return any;
  }

  // ---- message-sharded batch ----
  // The batches the peer protocols cannot take — churn (a mesh per heartbeat
  // epoch), IDONTWANT, and lazy gossip that is not a no-op (receiver-centric
  // IWANTs read other parts' keys) — run over the replicated graph instead.
  // Part p simulates messages [B*p/P, B*(p+1)/P) of the batch over all N peers
  // with gs_run's engine, then one all-to-all transposes the results: part r
  // receives, from every part, the rows of its own peers, so each sink still
  // gets [B][own peers]. The per-part memory is the same N*B/P lanes as the
  // peer protocols'; the data crossing GPUs is the results (9 B per lane),
  // once per batch.
  void run_ms() {
    each([&](uint32_t i, Ctx& c) {
      guarded([&] { ms_share(i, c); });
    });
    exchange_ms();
    ms_deliver();
  }

  // 1. a part's share of the messages over all N peers (device-resident rows [mp][N])
  void ms_share(uint32_t i, Ctx& c) {
    const uint32_t m0 = lay.m0(me(i)), mp = lay.mn(me(i));
    if (c.traffic) c.fail(GS_EUNSUPPORTED, "per-peer traffic is not supported in partitioned mode");
    if (c.pubsub) c.fail(GS_EUNSUPPORTED, "per-peer pubsub counts (gs_set_pubsub_counts) are not supported in partitioned mode");
    if (c.linkdel) c.fail(GS_EUNSUPPORTED, "per-link first deliveries (gs_set_link_deliveries) are not supported in partitioned mode");
    if (c.msgcost) c.fail(GS_EUNSUPPORTED, "per-message costs (gs_set_message_costs) are not supported in partitioned mode");
    if (sinks && sinks[i].summary)
      c.fail(GS_EUNSUPPORTED, "per-message summaries of a message-sharded partitioned batch (churn, IDONTWANT or "
                              "lazy gossip IWANTs): use gs_run");
    c.d_ms_tc.alloc(std::max<size_t>(1, (size_t)mp * N));
    c.d_ms_hops.alloc(std::max<size_t>(1, (size_t)mp * N));
    const uint64_t batches = c.stats.batches;
    if (mp) {
      gs_result_sink ds{};
      ds.t_complete_ns = c.d_ms_tc.p;
      ds.hops = c.d_ms_hops.p;
      MsShare share(c, lay.mmax());
      run_messages(c, sched + i0 + m0, mp, &ds);
    }
    c.stats.messages += B - mp;  // every part counts the batch, as in the peer protocols
    c.stats.batches = batches + 1;
    c.stats.ms_batches++;
  }

  // 2. the transposition: part r's peers of every part's messages into r's d_tc_t / d_hops_t [B][un_r]
  void exchange_ms() {
    if (cm->local) {
      each([&](uint32_t, Ctx& c) { GS_HIP(hipStreamSynchronize(c.stream)); });
      each([&](uint32_t r, Ctx& d) {
        const uint32_t u0 = lay.u0(r), un = lay.un(r);
        d.d_tc_t.alloc((size_t)un * B);
        d.d_hops_t.alloc((size_t)un * B);
        for (uint32_t p = 0; p < nctx; p++) {  // part p's block of r's peers, straight from p's rows
          const uint32_t mp = lay.mn(p);
          if (!mp) continue;
          GS_HIP(hipMemcpy2DAsync(d.d_tc_t.p + lay.ms_recv_off(p, r), (size_t)un * 8, cx[p]->d_ms_tc.p + u0,
                                  (size_t)N * 8, (size_t)un * 8, mp, hipMemcpyDeviceToDevice, d.stream));
          GS_HIP(hipMemcpy2DAsync(d.d_hops_t.p + lay.ms_recv_off(p, r), un, cx[p]->d_ms_hops.p + u0, N, un, mp,
                                  hipMemcpyDeviceToDevice, d.stream));
        }
      });
      each([&](uint32_t, Ctx& c) { GS_HIP(hipStreamSynchronize(c.stream)); });
      return;
    }
    Ctx& c = *cx[0];
    const uint32_t r0 = cm->rank, mme = lay.mn(r0), unme = lay.un(r0);
    GS_HIP(hipSetDevice(c.cfg.device));
    // pack: destination r's block [mme][un_r] at lay.ms_send_off(r0, r)
    c.d_ms_send.alloc(std::max<size_t>(1, (size_t)mme * N));
    c.d_ms_sendh.alloc(std::max<size_t>(1, (size_t)mme * N));
    if (mme)
      for (uint32_t r = 0; r < P; r++) {
        const uint32_t u0 = lay.u0(r), un = lay.un(r);
        GS_HIP(hipMemcpy2DAsync(c.d_ms_send.p + lay.ms_send_off(r0, r), (size_t)un * 8, c.d_ms_tc.p + u0,
                                (size_t)N * 8, (size_t)un * 8, mme, hipMemcpyDeviceToDevice, c.stream));
        GS_HIP(hipMemcpy2DAsync(c.d_ms_sendh.p + lay.ms_send_off(r0, r), un, c.d_ms_hops.p + u0, N, un, mme,
                                hipMemcpyDeviceToDevice, c.stream));
      }
    c.d_tc_t.alloc((size_t)unme * B);
    c.d_hops_t.alloc((size_t)unme * B);
    coll_group_start(cm);
    for (uint32_t r = 0; r < P; r++) {
      const uint64_t n = lay.ms_count(r0, r), off = lay.ms_send_off(r0, r);
      send_pieces(c.d_ms_send.p + off, n, r);
      send_pieces(c.d_ms_sendh.p + off, n, r);
    }
    for (uint32_t p = 0; p < P; p++) {
      const uint64_t n = lay.ms_count(p, r0), off = lay.ms_recv_off(p, r0);
      recv_pieces(c.d_tc_t.p + off, n, p);
      recv_pieces(c.d_hops_t.p + off, n, p);
    }
    coll_group_end(cm);
    GS_HIP(hipStreamSynchronize(c.stream));
  }

  // 3. own peers' rows into the sinks; the logged latencies of them from the exchanged
  // completion times (k_lat_rows), every part's before the gate and the first hand-over
  void ms_deliver() {
    const bool any = lat_stage_all(sched + i0);
    if (!sinks && !any) return;
    each([&](uint32_t i, Ctx& c) {
      if (wants_lat(i)) part_lat_deliver_ms(c, B, sink(i), i0);
      else if (sinks) deliver_rows(c, B, lay.un(me(i)), &sinks[i], i0);
      GS_HIP(hipStreamSynchronize(c.stream));
    });
  }

  // ---- what the two peer protocols share ----
  // Counters of every part before a batch; restored when the peer protocols'
  // eager result is discarded (lazy gossip can change the batch).
  void save_counters() {
    each([&](uint32_t, Ctx& c) {
      c.d_cnt_save.alloc(C_COUNT);
      GS_HIP(hipMemcpyAsync(c.d_cnt_save.p, c.d_counters.p, C_COUNT * 8, hipMemcpyDeviceToDevice, c.stream));
    });
  }
  // The batch's tail once every part's completion ran and the parts (and
  // ranks) agreed on ok, the lazy-gossip no-op proof: the eager result stands
  // and leaves, or (an IHAVE can land before the last delivery) the batch runs
  // again message-sharded, with gossip, from the saved counters.
  void finish_or_gossip(bool ok) {
    if (ok) {
      lat_stage_all(nullptr);
      each([&](uint32_t i, Ctx& c) { part_dev_finish(c, sink(i), i0); });
      return;
    }
    each([&](uint32_t, Ctx& c) {
      part_abort(c);
      GS_HIP(hipMemcpyAsync(c.d_counters.p, c.d_cnt_save.p, C_COUNT * 8, hipMemcpyDeviceToDevice, c.stream));
      GS_HIP(hipStreamSynchronize(c.stream));
      c.stats.gossip_fallback_batches++;
    });
    run_ms();
  }

  // ---- the list pass over partitioned rows ----
  // Every part runs the window passes of gs_run over its own rows; between
  // passes the parts agree on the pass control (records emitted, min pending
  // key, error word) and exchange the pass's records, packed, with every
  // peer's count and offset. Returns false, with every part's state and
  // counters as before, when the list pass cannot take the batch (ring bound,
  // memory, a knob) or a candidate list overflowed: push takes the batch.
  bool run_lp() {
    uint64_t key = INF64;
    if (!lp_begin(key)) return lp_abort();
    each([&](uint32_t, Ctx& c) { part_lp_set(c, 0, key); });  // slot 2 as pass 0 reads it: no records, the min seeded key
    timing_reset();
    const LpExchange x(*this);
    std::vector<uint64_t> st((size_t)P * 4), cnt(P);  // per part: mode, records, min pending, error word
    for (;;) {
      each([&](uint32_t, Ctx& c) {
        mark(c);
        part_lp_pass(c);
        mark(c);
      });
      lp_control(x, st.data());
      uint64_t recs = 0, minp = INF64, err = 0;
      for (uint32_t p = 0; p < P; p++) {
        recs += cnt[p] = st[(size_t)p * 4 + 1];
        minp = std::min(minp, st[(size_t)p * 4 + 2]);
        err |= st[(size_t)p * 4 + 3];
      }
      if (err & (ERR_LIST | ERR_RING)) return lp_abort();  // lost entries somewhere: the push protocol takes the batch
      if (st[0] == PM_DONE) break;  // the pass mode: grid- and part-uniform
      if (!x.dev_ctl) each([&](uint32_t, Ctx& c) { part_lp_set(c, recs, minp); });
      if (!recs) continue;  // the next pass emits a window: it reads no records
      if (x.direct) exchange_lp_direct(cnt.data(), recs);
      else if (x.routed) exchange_lp_routed(cnt.data(), recs);
      else exchange_lp_gathered(cnt.data(), recs);
    }
    total_times(2);
    lp_end();
    return true;
  }

  // Every part's set-up enqueued, then each one's seeds waited for; the ranks
  // then share whether some part cannot take the batch, and the min seeded key.
  bool lp_begin(uint64_t& key) {
    std::vector<uint64_t> smin(nctx, INF64);
    uint64_t bad = 0;  // some part cannot take the batch on the list pass
    guarded([&] {
      each([&](uint32_t, Ctx& c) { bad |= part_lp_begin(c, sched + i0, B) ? 0u : 1u; });
      if (!bad) each([&](uint32_t i, Ctx& c) { smin[i] = part_lp_seed_min(c); });
    });
    key = *std::min_element(smin.begin(), smin.end());
    const uint64_t mine[2] = {bad, ~key};
    uint64_t all[2 * 64];
    const uint32_t rows = gather(mine, 2, all);
    for (uint32_t k = 0; k < rows; k++) {
      bad |= all[2 * k];
      key = std::min(key, ~all[2 * k + 1]);
    }
    return !bad;
  }
  bool lp_abort() {
    each([&](uint32_t, Ctx& c) { part_lp_abort(c); });
    return false;
  }

  // The control read: st[p * 4 ..] = part p's {mode, records, min pending, error word} of the last pass.
  void lp_control(const LpExchange& x, uint64_t* st) {
    if (x.dev_ctl) {
      part_lp_combine(cx, P, st);  // (and every part's slot holds the combined values: no part_lp_set)
    } else if (cm->local) {  // every part's control read in flight, then each one waited for
      each([&](uint32_t, Ctx& c) { part_lp_read_enqueue(c); });
      each([&](uint32_t i, Ctx& c) { part_lp_read_wait(c, st + (size_t)i * 4); });
    } else {
      uint64_t mine[4];
      part_lp_read(*cx[0], mine);
      gather(mine, 4, st);
    }
  }

  // Direct (loop-back parts on one device): every part stores its routed
  // records into the destinations, at the gathered bases (holes allowed).
  void exchange_lp_direct(const uint64_t* cnt, uint64_t recs) {
    std::vector<uint64_t> base(P + 1);
    lp_bases(cnt, P, base.data());
    for (uint32_t i = 0; i < nctx; i++) cx[i]->d_rpk.alloc(recs);  // (before any pack stores into it)
    for (uint32_t i = 0; i < nctx; i++) {
      part_lp_pack_route_direct(cx, P, i, base[i]);
      if (!cx[i]->part_xev) GS_HIP(hipEventCreateWithFlags(&cx[i]->part_xev, hipEventDisableTiming));
      GS_HIP(hipEventRecord(cx[i]->part_xev, cx[i]->stream));
    }
    for (uint32_t q = 0; q < nctx; q++)  // the next pass of q reads what every part stored into it
      for (uint32_t i = 0; i < nctx; i++)
        if (i != q) GS_HIP(hipStreamWaitEvent(cx[q]->stream, cx[i]->part_xev, 0));
  }

  // Routed: each part receives only the records with a receiver it owns
  // (gs_layout.h lp_route_bases), from the senders' segments d_rsend.
  void exchange_lp_routed(const uint64_t* cnt, uint64_t recs) {
    std::vector<uint64_t> route((size_t)P * P), bq(P);
    each([&](uint32_t i, Ctx& c) {
      c.d_rpk.alloc(recs);
      part_lp_pack_route(c, P, me(i), cnt[me(i)]);
    });
    if (cm->local) {
      each([&](uint32_t i, Ctx& c) { part_lp_route_read(c, P, &route[(size_t)i * P]); });  // (every pack done)
      each([&](uint32_t q, Ctx& d) {
        lp_route_bases(route.data(), P, q, bq.data());
        for (uint32_t p = 0; p < nctx; p++) {
          if (p == q) continue;
          Ctx& src = *cx[p];
          const uint64_t n = route[(size_t)p * P + q], cap = std::max<uint64_t>(cnt[p], 1);
          const uint32_t u0 = lay.u0(p), un = lay.un(p);
          if (n) GS_HIP(hipMemcpyAsync(d.d_rpk.p + bq[p], src.d_rsend.p + (size_t)q * cap, n * 8,
                                       hipMemcpyDeviceToDevice, d.stream));
          GS_HIP(hipMemcpyAsync(d.d_rcg.p + u0, src.d_rrcg.p + (size_t)q * un, un * 4, hipMemcpyDeviceToDevice,
                                d.stream));
          GS_HIP(hipMemcpyAsync(d.d_roffg.p + u0, src.d_rroff.p + (size_t)q * un, un * 8, hipMemcpyDeviceToDevice,
                                d.stream));
        }
        part_lp_route_fix(d, P, q, bq.data());
      });
      for (uint32_t q = 0; q < nctx; q++) GS_HIP(hipStreamSynchronize(cx[q]->stream));  // sources reused next pass
      return;
    }
    Ctx& c = *cx[0];
    const uint32_t r0 = cm->rank, myun = lay.un(r0);
    coll_AllGather(cm, c.d_pkcur.p, cm->scratch_mat(), P, ncclUint64, c.stream);  // row p: p's counts
    GS_HIP(hipMemcpyAsync(route.data(), cm->scratch_mat(), (size_t)P * P * 8, hipMemcpyDeviceToHost, c.stream));
    GS_HIP(hipStreamSynchronize(c.stream));
    lp_route_bases(route.data(), P, r0, bq.data());
    const uint64_t mycap = std::max<uint64_t>(cnt[r0], 1);
    coll_group_start(cm);
    for (uint32_t d = 0; d < P; d++) {
      if (d == r0) continue;
      send_pieces(c.d_rsend.p + (size_t)d * mycap, route[(size_t)r0 * P + d], d);
      coll_Send(cm, c.d_rrcg.p + (size_t)d * myun, myun, ncclUint32, (int)d, c.stream);
      coll_Send(cm, c.d_rroff.p + (size_t)d * myun, myun, ncclUint64, (int)d, c.stream);
    }
    for (uint32_t sr = 0; sr < P; sr++) {
      if (sr == r0) continue;
      const uint32_t u0 = lay.u0(sr), un = lay.un(sr);
      recv_pieces(c.d_rpk.p + bq[sr], route[(size_t)sr * P + r0], sr);
      coll_Recv(cm, c.d_rcg.p + u0, un, ncclUint32, (int)sr, c.stream);
      coll_Recv(cm, c.d_roffg.p + u0, un, ncclUint64, (int)sr, c.stream);
    }
    coll_group_end(cm);
    part_lp_route_fix(c, P, r0, bq.data());
  }

  // Gathered: every part's whole record range to every part, each packed in
  // place at its gathered base (part_lp_pack) with its tables at its peers.
  void exchange_lp_gathered(const uint64_t* cnt, uint64_t recs) {
    std::vector<uint64_t> base(P + 1);
    lp_bases(cnt, P, base.data());
    each([&](uint32_t i, Ctx& c) {
      c.d_rpk.alloc(recs);
      part_lp_pack(c, base[me(i)], cnt[me(i)]);
    });
    if (cm->local) {
      for (uint32_t i = 0; i < nctx; i++) GS_HIP(hipStreamSynchronize(cx[i]->stream));  // every pack done
      each([&](uint32_t q, Ctx& d) {  // every other part's range (each packed its own in place)
        for (uint32_t p = 0; p < nctx; p++) {
          if (p == q) continue;
          Ctx& src = *cx[p];
          const uint64_t n = cnt[p], u0 = lay.u0(p), un = lay.un(p);
          if (n) GS_HIP(hipMemcpyAsync(d.d_rpk.p + base[p], src.d_rpk.p + base[p], n * 8, hipMemcpyDeviceToDevice,
                                       d.stream));
          GS_HIP(hipMemcpyAsync(d.d_rcg.p + u0, src.d_rcg.p + u0, un * 4, hipMemcpyDeviceToDevice, d.stream));
          GS_HIP(hipMemcpyAsync(d.d_roffg.p + u0, src.d_roffg.p + u0, un * 8, hipMemcpyDeviceToDevice, d.stream));
        }
      });
      for (uint32_t q = 0; q < nctx; q++) GS_HIP(hipStreamSynchronize(cx[q]->stream));  // sources reused next pass
      return;
    }
    Ctx& c = *cx[0];
    const uint32_t r0 = cm->rank;
    const uint64_t myu0 = lay.u0(r0), myun = lay.un(r0);
    coll_group_start(cm);
    for (uint32_t d = 0; d < P; d++) {
      if (d == r0) continue;
      send_pieces(c.d_rpk.p + base[r0], cnt[r0], d);  // (the own range stays where it was packed)
      coll_Send(cm, c.d_rcg.p + myu0, myun, ncclUint32, (int)d, c.stream);
      coll_Send(cm, c.d_roffg.p + myu0, myun, ncclUint64, (int)d, c.stream);
    }
    for (uint32_t sr = 0; sr < P; sr++) {
      if (sr == r0) continue;
      const uint64_t u0 = lay.u0(sr), un = lay.un(sr);
      recv_pieces(c.d_rpk.p + base[sr], cnt[sr], sr);
      coll_Recv(cm, c.d_rcg.p + u0, un, ncclUint32, (int)sr, c.stream);
      coll_Recv(cm, c.d_roffg.p + u0, un, ncclUint64, (int)sr, c.stream);
    }
    coll_group_end(cm);
  }

  // Completion of every part enqueued, then each one waited for with its
  // lazy-gossip no-op proof; the ranks share the verdicts in an all-gather.
  void lp_end() {
    bool ok = true;
    each([&](uint32_t i, Ctx& c) { part_lp_end_enqueue(c, sink(i)); });
    each([&](uint32_t, Ctx& c) { ok = part_lp_end_check(c) && ok; });
    if (cx[0]->cfg.lazy_gossip) {
      const uint64_t mine = ok ? 0 : 1;
      uint64_t all[64];
      const uint32_t rows = gather(&mine, 1, all);
      for (uint32_t k = 0; k < rows; k++) ok = ok && !all[k];
    }
    finish_or_gossip(ok);
  }

  // ---- the push protocol: scan / routed export / receive per bucket ----
  void run_push() {
    push_begin();
    timing_reset();
    std::vector<uint64_t> mat((size_t)P * P), nrecv(nctx);  // mat[s * P + d] = records part s sends to part d (this bucket)
    for (;;) {
      each([&](uint32_t, Ctx& c) {  // 1. scan + per-destination counts
        mark(c);
        part_dev_bucket(c, P);
        part_dev_scan_count(c, P);
        mark(c);
      });
      if (push_read(mat.data()) == INF64) break;  // every part agrees: the MIN all-reduce made it the same everywhere
      push_export(mat.data(), nrecv.data());
      exchange_push(mat.data());
      each([&](uint32_t i, Ctx& c) {  // 4. relax into own peers
        part_dev_relax_next(c, c.d_pin.p, nrecv[i]);
        mark(c);
      });
      ctrl_min(false);  // next bucket = MIN over parts
    }
    total_times(3);
    bool ok = true;  // lazy gossip: the eager result stands only where every part proves it a no-op
    each([&](uint32_t i, Ctx& c) {
      ok = part_dev_complete(c, sinks && sinks[i].summary, true, wants_lat(i)) && ok;
    });
    if (cx[0]->cfg.lazy_gossip) ok = agree(ok ? 1 : 0, ncclMin) != 0;
    finish_or_gossip(ok);
  }

  // Every part's batch set-up (a rank whose set-up fails takes the others out
  // with it); the seeded min is left in ctrl[0], then the MIN over the parts.
  void push_begin() {
    ctl.assign(nctx, INF64);
    guarded([&] {
      each([&](uint32_t i, Ctx& c) { ctl[i] = part_begin(c, sched + i0, B); });
    });
    ctrl_min(true);
  }

  // The MIN of every part's ctrl[0] into every part's ctrl[0]: over the ranks
  // on the device; loop-back through the host, from `ctl` when the host holds
  // the parts' words already, else read first.
  void ctrl_min(bool have) {
    if (!cm->local) {
      coll_AllReduce(cm, cx[0]->d_ctrl.p, cx[0]->d_ctrl.p, 1, ncclUint64, ncclMin, cx[0]->stream);
      return;
    }
    if (!have) {
      each([&](uint32_t i, Ctx& c) {
        GS_HIP(hipMemcpyAsync(&ctl[i], c.d_ctrl.p, 8, hipMemcpyDeviceToHost, c.stream));
      });
      for (uint32_t i = 0; i < nctx; i++) GS_HIP(hipStreamSynchronize(cx[i]->stream));
    }
    const uint64_t k = *std::min_element(ctl.begin(), ctl.end());
    each([&](uint32_t, Ctx& c) {
      c.h_pinned[0] = k;
      GS_HIP(hipMemcpyAsync(c.d_ctrl.p, c.h_pinned, 8, hipMemcpyHostToDevice, c.stream));
      GS_HIP(hipStreamSynchronize(c.stream));
    });
  }

  // 2. the count matrix and the bucket key on the host (the one read per bucket); returns the key
  uint64_t push_read(uint64_t* mat) {
    if (cm->local) {
      each([&](uint32_t i, Ctx& c) {
        GS_HIP(hipMemcpyAsync(&mat[(size_t)i * P], c.d_dcnt.p, P * 8, hipMemcpyDeviceToHost, c.stream));
        GS_HIP(hipMemcpyAsync(&ctl[i], c.d_ctrl.p, 8, hipMemcpyDeviceToHost, c.stream));
      });
      for (uint32_t i = 0; i < nctx; i++) GS_HIP(hipStreamSynchronize(cx[i]->stream));
    } else {
      Ctx& c = *cx[0];
      coll_AllGather(cm, c.d_dcnt.p, cm->scratch_mat(), P, ncclUint64, c.stream);
      GS_HIP(hipMemcpyAsync(mat, cm->scratch_mat(), (size_t)P * P * 8, hipMemcpyDeviceToHost, c.stream));
      GS_HIP(hipMemcpyAsync(&ctl[0], c.d_ctrl.p, 8, hipMemcpyDeviceToHost, c.stream));
      GS_HIP(hipStreamSynchronize(c.stream));
    }
    return ctl[0];
  }

  // 3. every part's records grouped by destination into d_pout, d_pin sized for what it receives
  void push_export(const uint64_t* mat, uint64_t* nrecv) {
    each([&](uint32_t i, Ctx& c) {
      uint64_t ns = 0, nr = 0;
      for (uint32_t d = 0; d < P; d++) ns += mat[(size_t)me(i) * P + d];
      for (uint32_t s = 0; s < P; s++) nr += mat[(size_t)s * P + me(i)];
      nrecv[i] = nr;
      c.d_pout.alloc(std::max<uint64_t>(ns, 1));
      c.d_pin.alloc(std::max<uint64_t>(nr, 1));
      part_dev_export(c, P, c.d_pout.p);
    });
  }

  // The bucket's all-to-all-v: part i receives from every s, in source order.
  // Peak buckets at 1M peers move GBs per pair, so the ranks' point-to-point
  // transfers go in pieces: cut in records, sent as bytes.
  void exchange_push(const uint64_t* mat) {
    if (cm->local) {
      for (uint32_t i = 0; i < nctx; i++) GS_HIP(hipStreamSynchronize(cx[i]->stream));  // every export done
      each([&](uint32_t i, Ctx& c) {
        uint64_t roff = 0;
        for (uint32_t s = 0; s < nctx; s++) {
          uint64_t soff = 0;
          for (uint32_t d = 0; d < i; d++) soff += mat[(size_t)s * P + d];
          const uint64_t n = mat[(size_t)s * P + i];
          if (n)
            GS_HIP(hipMemcpyAsync(c.d_pin.p + roff, cx[s]->d_pout.p + soff, n * sizeof(gs_part_record),
                                  hipMemcpyDeviceToDevice, c.stream));
          roff += n;
        }
      });
      return;
    }
    Ctx& c = *cx[0];
    const uint32_t r0 = cm->rank;
    coll_group_start(cm);
    uint64_t soff = 0, roff = 0;
    for (uint32_t d = 0; d < P; d++) {
      send_pieces(c.d_pout.p + soff, mat[(size_t)r0 * P + d], d);
      soff += mat[(size_t)r0 * P + d];
    }
    for (uint32_t s = 0; s < P; s++) {
      recv_pieces(c.d_pin.p + roff, mat[(size_t)s * P + r0], s);
      roff += mat[(size_t)s * P + r0];
    }
    coll_group_end(cm);
  }

  // One batch: message-sharded where the peer protocols cannot take it (churn,
  // IDONTWANT: the same decision on every rank), else the list pass when it
  // can take the batch, else the push protocol.
  void run_batch(uint64_t first, uint32_t n) {
    i0 = first;
    B = n;
    P = cm->nranks;
    N = cx[0]->cfg.peers;
    lay = PartLayout{P, N, B};
    pb = rccl_piece_bytes();
    if (part_needs_ms(*cx[0], sched + i0, B)) return run_ms();
    if (cx[0]->cfg.lazy_gossip) save_counters();
    if (!run_lp()) run_push();
  }
};

LpExchange::LpExchange(const PRun& r) {
  one_dev = r.cm->local != 0;
  for (uint32_t i = 1; i < r.nctx; i++) one_dev = one_dev && r.cx[i]->cfg.device == r.cx[0]->cfg.device;
  dev_ctl = one_dev && r.P <= PART_ROUTE_PMAX;
  const bool direct_ok = dev_ctl && !env_off("GS_PART_DIRECT");
  routed = r.P <= PART_ROUTE_PMAX && env_int("GS_PART_ROUTE", direct_ok) != 0;
  direct = routed && direct_ok;
}

// gs_run_partitioned's body; gs_run_partitioned_log calls it with latency-only sinks while
// every context's text callback is set (Ctx::text, as gs_run_log).
gs_status run_partitioned(gs_ctx* const* ctxs, uint32_t nctx, gs_comm* comm, const gs_publish* sched, uint64_t n_msgs,
                          const gs_result_sink* sinks) {
  Ctx* c0 = ctxs[0];
  try {
    if (comm->local ? nctx != comm->nranks : nctx != 1)
      c0->fail(GS_EINVAL, "gs_run_partitioned: pass one context per part (local) or this rank's context (RCCL)");
    for (uint32_t i = 0; sinks && i < nctx; i++) check_sink(*c0, &sinks[i]);  // gs_run's rules, for every part's sink
    std::vector<Ctx*> cx(ctxs, ctxs + nctx);
    PRun r{comm, cx.data(), nctx, sched, sinks};
    r.each([&](uint32_t i, Ctx& c) {
      if (!c.mesh_built) c.fail(GS_ESTATE, "gs_mesh_converge first");
      if (c.cfg.peers != c0->cfg.peers || c.cfg.batch != c0->cfg.batch)
        c0->fail(GS_EINVAL, "every part needs the same peers and batch");
      if (c.pdelay != c0->pdelay) c0->fail(GS_EINVAL, "every part needs the same gs_set_peer_delay switch");
      if (c.topo_fp != c0->topo_fp)  // (0: gs_build_topology's graph, a function of the configuration)
        c0->fail(GS_EINVAL, "every part needs the same graph (gs_set_topology / gs_set_topology_dials)");
      if (c.mesh_fp != c0->mesh_fp)  // (0: a converged or loaded mesh; an import of the same mesh is not 0)
        c0->fail(GS_EINVAL, "every part needs the same mesh (gs_set_mesh / gs_set_mesh_links in every part, or in none)");
      if (c.outage_fp != c0->outage_fp)  // (0: the draw; churn batches run message-sharded over one offline table)
        c0->fail(GS_EINVAL, "every part needs the same outages (gs_set_outages in every part, or in none)");
      part_set(c, comm->nranks, r.me(i));
    });
    if (!comm->local && c0->cfg.device != comm->device)
      c0->fail(GS_EINVAL, "the context and the communicator must use the same device");
    r.check_same_config(n_msgs, ((sinks && sinks[0].on_lat) ? 1 : 0) | (c0->pdelay ? 2 : 0));
    uint64_t i0 = 0;
    while (i0 < n_msgs) {  // batches of equal size and chunk count, at most cfg.batch messages
      uint64_t i1 = i0 + 1;
      while (i1 < n_msgs && i1 - i0 < c0->cfg.batch && sched[i1].msg_size == sched[i0].msg_size &&
             sched[i1].frags == sched[i0].frags)
        i1++;
      r.run_batch(i0, (uint32_t)(i1 - i0));
      i0 = i1;
    }
  } catch (const Error& e) {
    for (uint32_t i = 0; i < nctx; i++) part_abort(*ctxs[i]);  // no context is left mid-batch
    c0->last_error = e.msg;
    return e.code;
  } catch (const std::exception& e) {
    for (uint32_t i = 0; i < nctx; i++) part_abort(*ctxs[i]);
    c0->last_error = e.what();
    return GS_ENOMEM;
  }
  return GS_OK;
}

}  // namespace
