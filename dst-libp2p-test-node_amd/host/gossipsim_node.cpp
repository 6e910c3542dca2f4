// gossipsim-node — C++ host CLI standing in for the reference experiment:
// the env surface of rust-test-node (src/env.rs:27-87), topogen.py's link
// graph parameters (shadow/topogen.py:13-36), run.sh's publish schedule
// (shadow/run.sh:23-36) in place of the HTTP injector, and the arrival log
// that shadow/summary_latency*.awk parse (main.rs:93, run.sh:61).
//
//   PEERS=1000 CONNECTTO=10 FRAGMENTS=1 MUXER=yamux \
//   ./gossipsim-node -bl 50 -bh 150 -ll 40 -lh 130 -st 5 -s 15000 -m 10 \
//       --publisher 6 --rotation 1 --delay-ms 1000 --latencies latencies1
//   awk -f summary_latency_large.awk latencies1
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/gossipsim.h"

namespace {

void usage() {
  fprintf(stderr,
          "usage: gossipsim-node [-bl MBIT] [-bh MBIT] [-ll MS] [-lh MS] [-st STAGES] [--shortest]\n"
          "         [-s MSG_BYTES] [-m MESSAGES] [--publisher ID] [--rotation 0|1]\n"
          "         [--delay-ms MS] [--t0-s SECONDS] [--http-us US] [--max-heartbeats H] [--latencies PATH]\n"
          "         [--device-log]\n"
          "         [--gml network_topology.gml --yaml shadow.yaml] [--schedule FILE] [--shadowlog PATH] [--metrics PATH]\n"
          "         [--testnode-metrics PATH] [--pubsub-metrics PATH] [--mesh-metrics PATH] [--mesh-series PATH]\n"
          "         [--topology DIALS] [--dump-topology PATH] [--mesh LINKS] [--dump-mesh PATH] [--link-deliveries PATH]\n"
          "         [--message-costs PATH] [--outages FILE]\n"
          "  --topology imports a dial list (one \"dialer target\" per line) in place of the random dialing;\n"
          "    --dump-topology writes the dial list of the graph the run used\n"
          "  --mesh imports a mesh (one \"a b\" link per line) in place of the heartbeats' converge (not with\n"
          "    --mesh-metrics / --mesh-series, which describe a converge); --dump-mesh writes the links of the mesh\n"
          "    the run used\n"
          "  --outages imports who is offline when (one \"peer t_down_ns [t_up_ns]\" per line, absolute ns; no third\n"
          "    column: the peer never returns) in place of the churn draw, converted to heartbeat epochs with the run's\n"
          "    heartbeat and phase; an error on a run without churn (GS_CHURN_PPM = 0)\n"
          "  --yaml also supplies the injector's -s/-m/-d and start_time unless given on the command line\n"
          "  --device-log writes --latencies from the device-formatted text (gs_run_log), one fwrite per chunk\n"
          "  --testnode-metrics writes the nim node's per-peer delay metrics (dst_testnode_*, gs_set_peer_delay);\n"
          "    a run with a latency of 65535 ms or more then fails\n"
          "  --pubsub-metrics writes the go node's per-peer pubsub counters (libp2p_pubsub_*, gs_set_pubsub_counts)\n"
          "  --mesh-metrics writes the go node's per-peer GRAFT / PRUNE counters and mesh gauges, --mesh-series the\n"
          "    per-epoch mesh health as CSV, both of the mesh convergence (gs_set_mesh_events)\n"
          "  --link-deliveries writes \"receiver sender publish mesh gossip\" per connection that delivered a fragment\n"
          "    first: who delivered to whom, by the publisher, over the mesh, by IWANT answers (gs_set_link_deliveries)\n"
          "  --message-costs writes one TSV line per message: copies sent and arrived, first receipts, duplicates,\n"
          "    IHAVEs, IWANTs, completions and the wire bytes they cost (gs_set_message_costs)\n"
          "env: PEERS CONNECTTO FRAGMENTS MUXER MAXCONNECTIONS GOSSIPSUB_* SELFTRIGGER GS_NODE GS_SEED GS_BATCH\n"
          "     GS_DEVICE\n");
}

// Results arrive as the logged latency, message-major blocks of u16 ms
// (gs_result_sink.on_lat, GS_WANT_LAT_MS: 2 bytes per (peer, message), the
// value main.rs:93 prints): the log is streamed through gs_log_write_lat and
// the latencies folded into a 1 ms histogram, so no [messages][peers] host
// array is held. A run with a latency of 65535 ms or more (which the u16
// stream cannot carry: gs_run fails with GS_ERANGE) is delivered again as
// completion times (on_block, gs_log_write), the log rewritten from the start.
struct Stream {
  gs_log* log = nullptr;
  const gs_publish* sched = nullptr;
  gs_status st = GS_OK;
  std::vector<uint64_t> hist_ms;
  bool self_log = false;
};

void on_lat(void* user, uint64_t first, uint32_t n, uint32_t peers, const uint16_t* lat) {
  Stream* S = (Stream*)user;
  if (S->log && S->st == GS_OK) S->st = gs_log_write_lat(S->log, S->sched + first, n, lat);
  for (size_t i = 0; i < (size_t)n * peers; i++) {
    const uint16_t ms = lat[i];
    if (ms == GS_LAT_NONE) continue;  // undelivered, or the publisher without SELFTRIGGER
    if (ms >= S->hist_ms.size()) S->hist_ms.resize((size_t)ms + 1, 0);
    S->hist_ms[ms]++;
  }
}

// The same from completion times (the u64 fallback): the lines main.rs:93
// prints, (t_complete - tx_time) / 1e6 truncated; the publisher logs only with
// SELFTRIGGER (cfg.self_log).
void on_block(void* user, uint64_t first, uint32_t n, uint32_t peers, const uint64_t* tc, const uint8_t*) {
  Stream* S = (Stream*)user;
  if (S->log && S->st == GS_OK) S->st = gs_log_write(S->log, S->sched + first, n, tc);
  for (uint32_t q = 0; q < n; q++) {
    const gs_publish& p = S->sched[first + q];
    for (uint32_t u = 0; u < peers; u++) {
      const uint64_t t = tc[(size_t)q * peers + u];
      if (t == GS_UNDELIVERED || (u == p.publisher && !S->self_log)) continue;
      const uint64_t ms = (t - p.t_pub_ns) / 1000000ull;
      if (ms >= S->hist_ms.size()) S->hist_ms.resize((size_t)ms + 1, 0);
      S->hist_ms[ms]++;
    }
  }
}

// --device-log: the log's text arrives formatted (gs_run_log), one fwrite per chunk.
struct TextOut {
  FILE* f = nullptr;
  bool ok = true;
  uint64_t lines = 0;
};

void on_text(void* user, uint64_t, uint32_t, const char* text, uint64_t bytes, uint64_t lines) {
  TextOut* T = (TextOut*)user;
  if (bytes && fwrite(text, 1, (size_t)bytes, T->f) != bytes) T->ok = false;
  T->lines += lines;
}

// nearest-rank percentile (rank ceil(q*n)) of the 1 ms histogram
uint64_t pct(const std::vector<uint64_t>& h, uint64_t n, uint32_t q100) {
  const uint64_t rank = (n * q100 + 99) / 100;
  uint64_t acc = 0;
  for (size_t i = 0; i < h.size(); i++)
    if ((acc += h[i]) >= rank && rank) return i;
  return 0;
}

int die(gs_ctx* ctx, gs_status st, const char* what) {
  fprintf(stderr, "%s failed (%d): %s\n", what, st, ctx ? gs_last_error(ctx) : "");
  if (ctx) gs_destroy(ctx);
  return 1;
}

}  // namespace

int main(int argc, char** argv) {
  // topogen.py defaults (topogen.py:15-26) and run.sh's fixed publisher knobs
  uint32_t bl = 50, bh = 50, ll = 100, lh = 100, stages = 1, mode = GS_LINKS_DIRECT;
  uint32_t msg_size = 1500, n_msgs = 10, publisher = 6, rotation = 1, max_hb = 400;
  uint64_t delay_ms = 1000, t0_s = 946684800ull + 500ull;  // Shadow epoch + injector start (topogen.py:130)
  // the POST reaches the node 1.5 round trips over the 1 ms injector-hub links
  // after the injector sends it (topogen.py:64-69); tx_time is stamped then
  uint64_t http_us = 3000;
  std::string latencies, gml, yaml, shadowlog, metrics, schedule, testnode, pubsub, mesh_metrics, mesh_series;
  std::string topology, dump_topology, mesh_file, dump_mesh, link_deliveries, message_costs, outages;
  bool set_size = false, set_msgs = false, set_delay = false, set_t0 = false, device_log = false;
  for (int i = 1; i < argc; i++) {
    std::string a = argv[i];
    auto next = [&](void) -> const char* {
      if (i + 1 >= argc) { usage(); exit(2); }
      return argv[++i];
    };
    if (a == "-bl") bl = (uint32_t)atoi(next());
    else if (a == "-bh") bh = (uint32_t)atoi(next());
    else if (a == "-ll") ll = (uint32_t)atoi(next());
    else if (a == "-lh") lh = (uint32_t)atoi(next());
    else if (a == "-st") stages = (uint32_t)atoi(next());
    else if (a == "--shortest") mode = GS_LINKS_SHORTEST;
    else if (a == "-s") { msg_size = (uint32_t)atoi(next()); set_size = true; }
    else if (a == "-m") { n_msgs = (uint32_t)atoi(next()); set_msgs = true; }
    else if (a == "--publisher") publisher = (uint32_t)atoi(next());
    else if (a == "--rotation") rotation = (uint32_t)atoi(next());
    else if (a == "--delay-ms") { delay_ms = strtoull(next(), nullptr, 10); set_delay = true; }
    else if (a == "--t0-s") { t0_s = strtoull(next(), nullptr, 10); set_t0 = true; }
    else if (a == "--http-us") http_us = strtoull(next(), nullptr, 10);
    else if (a == "--max-heartbeats") max_hb = (uint32_t)atoi(next());
    else if (a == "--latencies") latencies = next();
    else if (a == "--device-log") device_log = true;  // --latencies from gs_run_log's text
    else if (a == "--gml") gml = next();            // a Shadow experiment's network graph ...
    else if (a == "--yaml") yaml = next();          // ... and its host placement (topogen.py output)
    else if (a == "--shadowlog") shadowlog = next(); // tracker counters for summary_shadowlog.awk
    else if (a == "--metrics") metrics = next();    // the node metrics (rust-test-node/src/metrics.rs)
    else if (a == "--testnode-metrics") testnode = next();  // the nim node's metrics (gossipsub-queues/main.nim:25-78)
    else if (a == "--pubsub-metrics") pubsub = next();  // the go node's pubsub counters (go-test-node/metrics.go:84-220)
    else if (a == "--mesh-metrics") mesh_metrics = next();  // the go node's GRAFT / PRUNE counters (metrics.go:164-190)
    else if (a == "--mesh-series") mesh_series = next();    // per-epoch mesh health (its tracer, metrics.go:224-258)
    else if (a == "--topology") topology = next();  // a dial list ("dialer target" per line) in place of the built graph
    else if (a == "--dump-topology") dump_topology = next();  // the dial list of the graph the run used
    else if (a == "--mesh") mesh_file = next();  // a link list ("a b" per line) in place of the converge
    else if (a == "--dump-mesh") dump_mesh = next();  // the links of the mesh the run used
    else if (a == "--link-deliveries") link_deliveries = next();  // per-link first deliveries (P2, main.rs:252-258)
    else if (a == "--message-costs") message_costs = next();  // what each message cost
    else if (a == "--outages") outages = next();  // who is offline when, in place of the churn draw
    else if (a == "--schedule") schedule = next();  // rows: t_pub_ns publisher msg_size [frags]
    else { usage(); return 2; }
  }
  if (!mesh_file.empty() && (!mesh_metrics.empty() || !mesh_series.empty())) {  // (their getters: GS_ESTATE after an import)
    fprintf(stderr, "--mesh cannot be combined with %s: the mesh events describe a converge\n",
            mesh_metrics.empty() ? "--mesh-series" : "--mesh-metrics");
    return 2;
  }
  gs_config cfg;
  gs_config_default(&cfg);
  char err[256] = {0};
  gs_status st = gs_config_from_env(&cfg, err, sizeof(err));
  if (st != GS_OK) { fprintf(stderr, "Error reading peer settings: %s\n", err); return 1; }

  std::vector<uint64_t> lat((size_t)stages * stages), bw(stages), bw_dn;
  std::vector<uint8_t> stage_of_peer;
  if (!gml.empty()) {  // links straight from the Shadow experiment files
    if (yaml.empty()) { fprintf(stderr, "--gml needs --yaml (host placement)\n"); return 2; }
    uint32_t V = 0;
    gs_links_from_gml(gml.c_str(), mode, 0, &V, nullptr, nullptr, nullptr);
    lat.assign((size_t)V * V, 0);
    bw.assign(V, 0);
    bw_dn.assign(V, 0);
    if ((st = gs_links_from_gml(gml.c_str(), mode, V, &V, lat.data(), bw.data(), bw_dn.data())) != GS_OK) {
      fprintf(stderr, "cannot read %s (%d)\n", gml.c_str(), st);
      return 1;
    }
    stages = V;
    stage_of_peer.assign(cfg.peers, 0);
    if ((st = gs_shadow_hosts(yaml.c_str(), cfg.peers, stage_of_peer.data())) != GS_OK) {
      fprintf(stderr, "cannot place the %u peers with %s (%d)\n", cfg.peers, yaml.c_str(), st);
      return 1;
    }
  } else {
    st = gs_topogen_links(stages, bl, bh, ll, lh, mode, lat.data(), bw.data());
    if (st != GS_OK) { fprintf(stderr, "invalid topogen parameters\n"); return 1; }
    bw_dn = bw;
  }

  if (!outages.empty() && !cfg.churn_ppm) {
    fprintf(stderr, "--outages needs a run with churn (GS_CHURN_PPM != 0; its value is not read with --outages)\n");
    return 2;
  }
  gs_ctx* ctx = nullptr;
  if ((st = gs_create(&cfg, &ctx)) != GS_OK) return die(nullptr, st, "gs_create");
  if ((st = gs_set_links(ctx, stages, lat.data(), bw.data(), bw_dn.data(),
                         stage_of_peer.empty() ? nullptr : stage_of_peer.data())) != GS_OK)
    return die(ctx, st, "gs_set_links");
  const bool counters = !shadowlog.empty() || !metrics.empty();
  if (counters && (st = gs_set_traffic(ctx, 1)) != GS_OK) return die(ctx, st, "gs_set_traffic");
  if (!testnode.empty() && (st = gs_set_peer_delay(ctx, 1)) != GS_OK) return die(ctx, st, "gs_set_peer_delay");
  if (!pubsub.empty() && (st = gs_set_pubsub_counts(ctx, 1)) != GS_OK) return die(ctx, st, "gs_set_pubsub_counts");
  if (!link_deliveries.empty() && (st = gs_set_link_deliveries(ctx, 1)) != GS_OK)
    return die(ctx, st, "gs_set_link_deliveries");
  if (!message_costs.empty() && (st = gs_set_message_costs(ctx, 1)) != GS_OK) return die(ctx, st, "gs_set_message_costs");
  const bool mesh_events = !mesh_metrics.empty() || !mesh_series.empty();
  if (mesh_events && (st = gs_set_mesh_events(ctx, 1)) != GS_OK) return die(ctx, st, "gs_set_mesh_events");
  if (topology.empty()) {
    if ((st = gs_build_topology(ctx)) != GS_OK) return die(ctx, st, "gs_build_topology");
  } else {  // the connections a real run made (its dial log lines, main.rs:340-348)
    uint64_t rows = 0;
    st = gs_read_dials(topology.c_str(), nullptr, nullptr, 0, &rows);
    if (st != GS_OK && st != GS_ERANGE) { fprintf(stderr, "malformed dial list %s\n", topology.c_str()); return die(ctx, st, "gs_read_dials"); }
    std::vector<uint32_t> dialer(rows + 1), target(rows + 1);
    if ((st = gs_read_dials(topology.c_str(), dialer.data(), target.data(), rows, &rows)) != GS_OK) return die(ctx, st, "gs_read_dials");
    if ((st = gs_set_topology_dials(ctx, rows, dialer.data(), target.data())) != GS_OK) return die(ctx, st, "gs_set_topology_dials");
  }
  if (!dump_topology.empty()) {
    uint64_t nnz = 0;
    if ((st = gs_graph_info(ctx, nullptr, &nnz, nullptr)) != GS_OK) return die(ctx, st, "gs_graph_info");
    std::vector<uint64_t> row((size_t)cfg.peers + 1);
    std::vector<uint32_t> col(nnz + 1);
    std::vector<uint8_t> fl(nnz + 1);
    if ((st = gs_get_csr(ctx, row.data(), col.data(), fl.data())) != GS_OK) return die(ctx, st, "gs_get_csr");
    if ((st = gs_write_dials(dump_topology.c_str(), cfg.peers, row.data(), col.data(), fl.data())) != GS_OK)
      return die(ctx, st, "gs_write_dials");
  }
  if (!outages.empty()) {  // the outages of a real run (its pods' restarts), or a what-if; before the converge
    uint64_t rows = 0, kept = 0;
    st = gs_read_outages(outages.c_str(), nullptr, nullptr, nullptr, 0, &rows);
    if (st != GS_OK && st != GS_ERANGE) {
      fprintf(stderr, "malformed outage list %s: line %llu\n", outages.c_str(), (unsigned long long)rows);
      return die(ctx, st, "gs_read_outages");
    }
    std::vector<uint32_t> op(rows + 1), hf(rows + 1), ht(rows + 1);
    std::vector<uint64_t> td(rows + 1), tu(rows + 1);
    if ((st = gs_read_outages(outages.c_str(), op.data(), td.data(), tu.data(), rows, &rows)) != GS_OK)
      return die(ctx, st, "gs_read_outages");
    if ((st = gs_outage_epochs(&cfg, rows, op.data(), td.data(), tu.data(), op.data(), hf.data(), ht.data(), &kept)) != GS_OK) {
      fprintf(stderr, "outage list %s: an outage ends before it starts, or lies past epoch 2^32 - 2\n", outages.c_str());
      return die(ctx, st, "gs_outage_epochs");
    }
    if ((st = gs_set_outages(ctx, kept, op.data(), hf.data(), ht.data())) != GS_OK) return die(ctx, st, "gs_set_outages");
  }
  uint32_t epochs = 0;
  if (mesh_file.empty()) {
    if ((st = gs_mesh_converge(ctx, max_hb, &epochs)) != GS_OK) return die(ctx, st, "gs_mesh_converge");
  } else {  // the mesh a real run ended up with (a tracer's Graft / Prune events, go metrics.go:328-340), or a what-if one
    uint64_t rows = 0;
    st = gs_read_dials(mesh_file.c_str(), nullptr, nullptr, 0, &rows);
    if (st != GS_OK && st != GS_ERANGE) { fprintf(stderr, "malformed link list %s\n", mesh_file.c_str()); return die(ctx, st, "gs_read_dials"); }
    std::vector<uint32_t> la(rows + 1), lb(rows + 1);
    if ((st = gs_read_dials(mesh_file.c_str(), la.data(), lb.data(), rows, &rows)) != GS_OK) return die(ctx, st, "gs_read_dials");
    if ((st = gs_set_mesh_links(ctx, rows, la.data(), lb.data())) != GS_OK) return die(ctx, st, "gs_set_mesh_links");
  }
  if (!dump_mesh.empty()) {
    std::vector<uint32_t> m((size_t)cfg.peers * GS_MESH_W);
    std::vector<uint8_t> mc(cfg.peers);
    if ((st = gs_get_mesh(ctx, m.data(), mc.data())) != GS_OK) return die(ctx, st, "gs_get_mesh");
    if ((st = gs_write_mesh_links(dump_mesh.c_str(), cfg.peers, m.data(), mc.data())) != GS_OK)
      return die(ctx, st, "gs_write_mesh_links");
  }
  if (!mesh_metrics.empty()) {  // the events of the convergence, the mesh it ended with
    std::vector<uint64_t> row((size_t)cfg.peers + 1), ev((size_t)cfg.peers * GS_MESH_EVENT_COLS);
    std::vector<uint8_t> mc(cfg.peers);
    if ((st = gs_get_csr(ctx, row.data(), nullptr, nullptr)) != GS_OK) return die(ctx, st, "gs_get_csr");
    if ((st = gs_get_mesh(ctx, nullptr, mc.data())) != GS_OK) return die(ctx, st, "gs_get_mesh");
    if ((st = gs_get_mesh_events(ctx, ev.data())) != GS_OK) return die(ctx, st, "gs_get_mesh_events");
    st = gs_write_mesh_metrics(&cfg, mesh_metrics.c_str(), cfg.peers, row.data(), mc.data(), ev.data());
    if (st != GS_OK) return die(ctx, st, "gs_write_mesh_metrics");
  }
  if (!mesh_series.empty()) {
    uint32_t rows = 0;
    if ((st = gs_mesh_series_rows(ctx, &rows)) != GS_OK) return die(ctx, st, "gs_mesh_series_rows");
    std::vector<uint64_t> se((size_t)rows * GS_MESH_SERIES_COLS);
    if ((st = gs_get_mesh_series(ctx, se.data(), rows)) != GS_OK) return die(ctx, st, "gs_get_mesh_series");
    if ((st = gs_write_mesh_series(mesh_series.c_str(), se.data(), rows)) != GS_OK)
      return die(ctx, st, "gs_write_mesh_series");
  }

  std::vector<gs_publish> sched;
  if (!schedule.empty()) {  // an explicit publish schedule stands in for the HTTP injector
    uint64_t rows = 0;
    st = gs_read_schedule(schedule.c_str(), nullptr, 0, &rows);
    if (st != GS_OK && st != GS_ERANGE) { fprintf(stderr, "malformed schedule %s\n", schedule.c_str()); return die(ctx, st, "gs_read_schedule"); }
    sched.resize(rows);
    if ((st = gs_read_schedule(schedule.c_str(), sched.data(), rows, &rows)) != GS_OK) return die(ctx, st, "gs_read_schedule");
    n_msgs = (uint32_t)rows;
  } else {
    uint64_t t0_ns = t0_s * 1000000000ull;
    gs_injector inj;
    if (!yaml.empty() && gs_shadow_injector(yaml.c_str(), &inj) == GS_OK) {  // traffic_sync.py args (topogen.py:125-136)
      if (!set_size) msg_size = inj.msg_size;
      if (!set_msgs) n_msgs = inj.messages;
      if (!set_delay && inj.delay_ns) delay_ms = inj.delay_ns / 1000000ull;
      if (!set_t0) t0_ns = 946684800000000000ull + inj.start_ns;  // Shadow epoch + the controller's start_time
    }
    sched.resize(n_msgs);
    gs_schedule_runsh(n_msgs, cfg.peers, publisher, rotation, t0_ns + http_us * 1000ull, delay_ms * 1000000ull,
                      msg_size, sched.data());
  }
  Stream strm;
  strm.sched = sched.data();
  strm.self_log = cfg.self_log != 0;
  bool text_done = false, wide_only = false;
  if (device_log && !latencies.empty()) {  // the log formatted on the device, written as it arrives
    TextOut out;
    if (!(out.f = fopen(latencies.c_str(), "w"))) return die(ctx, GS_EINVAL, "fopen --latencies");
    st = gs_run_log(ctx, sched.data(), n_msgs, on_text, &out, 0);
    if (fclose(out.f) || !out.ok) return die(ctx, GS_EINVAL, "fwrite --latencies");
    if (st == GS_OK) {
      text_done = true;
    } else if (st == GS_ERANGE && testnode.empty()) {  // as below: the run again through the completion times
      wide_only = true;
      gs_log_text_reset(ctx);
    } else {
      return die(ctx, st, "gs_run_log");
    }
  }
  if (!text_done && !latencies.empty() && (st = gs_log_open(&cfg, latencies.c_str(), &strm.log)) != GS_OK)
    return die(ctx, st, "gs_log_open");
  gs_result_sink sink{};
  sink.want = GS_WANT_LAT_MS;  // the logged latency, streamed through on_lat
  sink.on_lat = on_lat;
  sink.user = &strm;
  sink.block_msgs = 16;
  if (!text_done && !wide_only) st = gs_run(ctx, sched.data(), n_msgs, &sink);
  // (with --testnode-metrics the delay accumulators take the u16 latencies too: the error stands)
  if (wide_only || (st == GS_ERANGE && testnode.empty() && strstr(gs_last_error(ctx), "GS_WANT_LAT_MS"))) {
    // a latency the u16 stream cannot carry: the same run again (it is
    // deterministic) through the u64 completion times, the log from the start
    if (strm.log) gs_log_close(strm.log);
    strm.log = nullptr;
    strm.st = GS_OK;
    strm.hist_ms.clear();
    if (!latencies.empty() && (st = gs_log_open(&cfg, latencies.c_str(), &strm.log)) != GS_OK)
      return die(ctx, st, "gs_log_open");
    gs_reset_stats(ctx);  // (also restarts the per-peer traffic and pubsub counters and the link deliveries)
    gs_result_sink wide{};
    wide.want = GS_WANT_T_COMPLETE;
    wide.on_block = on_block;
    wide.user = &strm;
    wide.block_msgs = 16;
    st = gs_run(ctx, sched.data(), n_msgs, &wide);
  }
  if (st != GS_OK) return die(ctx, st, "gs_run");
  if (strm.log && ((st = gs_log_close(strm.log)) != GS_OK || (st = strm.st) != GS_OK))
    return die(ctx, st, "gs_log_write");
  gs_stats s;
  gs_get_stats(ctx, &s);
  uint64_t n = 0;
  for (uint64_t c : strm.hist_ms) n += c;
  if (text_done)  // no latency reached the host: the counters' mean and max
    fprintf(stderr,
            "peers=%u mesh_epochs=%u messages=%llu deliveries=%llu frag_deliveries=%llu "
            "relaxations=%llu gossip_iwant=%llu latency_ms mean=%llu max=%llu\n",
            cfg.peers, epochs, (unsigned long long)s.messages, (unsigned long long)s.deliveries,
            (unsigned long long)s.frag_deliveries, (unsigned long long)s.relaxations,
            (unsigned long long)s.gossip_iwant,
            (unsigned long long)(s.deliveries ? s.latency_sum_ms / s.deliveries : 0),
            (unsigned long long)s.latency_max_ms);
  else
    fprintf(stderr,
            "peers=%u mesh_epochs=%u messages=%llu deliveries=%llu frag_deliveries=%llu "
            "relaxations=%llu gossip_iwant=%llu latency_ms p50=%llu p95=%llu max=%llu\n",
            cfg.peers, epochs, (unsigned long long)s.messages, (unsigned long long)s.deliveries,
            (unsigned long long)s.frag_deliveries, (unsigned long long)s.relaxations,
            (unsigned long long)s.gossip_iwant, (unsigned long long)pct(strm.hist_ms, n, 50),
            (unsigned long long)pct(strm.hist_ms, n, 95), (unsigned long long)pct(strm.hist_ms, n, 100));
  if (counters) {
    std::vector<uint64_t> tr((size_t)cfg.peers * GS_TRAFFIC_COLS), row((size_t)cfg.peers + 1);
    std::vector<uint8_t> mc(cfg.peers);
    if ((st = gs_get_traffic(ctx, tr.data())) != GS_OK) return die(ctx, st, "gs_get_traffic");
    if ((st = gs_get_csr(ctx, row.data(), nullptr, nullptr)) != GS_OK) return die(ctx, st, "gs_get_csr");
    if ((st = gs_get_mesh(ctx, nullptr, mc.data())) != GS_OK) return die(ctx, st, "gs_get_mesh");
    const uint64_t end_s = sched.empty() ? 0 : (sched.back().t_pub_ns / 1000000000ull) - 946684800ull + 1;
    if (!shadowlog.empty() && (st = gs_write_shadow_heartbeat(shadowlog.c_str(), cfg.peers, tr.data(), end_s)) != GS_OK)
      return die(ctx, st, "gs_write_shadow_heartbeat");
    if (!metrics.empty() && (st = gs_write_node_metrics(&cfg, metrics.c_str(), row.data(), mc.data(), tr.data())) != GS_OK)
      return die(ctx, st, "gs_write_node_metrics");
  }
  if (!testnode.empty()) {
    std::vector<gs_peer_delay> pd(cfg.peers);
    std::vector<uint64_t> row((size_t)cfg.peers + 1);
    std::vector<uint8_t> mc(cfg.peers);
    if ((st = gs_get_peer_delay(ctx, pd.data())) != GS_OK) return die(ctx, st, "gs_get_peer_delay");
    if ((st = gs_get_csr(ctx, row.data(), nullptr, nullptr)) != GS_OK) return die(ctx, st, "gs_get_csr");
    if ((st = gs_get_mesh(ctx, nullptr, mc.data())) != GS_OK) return die(ctx, st, "gs_get_mesh");
    if ((st = gs_write_testnode_metrics(&cfg, testnode.c_str(), row.data(), mc.data(), sched.data(), n_msgs,
                                        pd.data())) != GS_OK)
      return die(ctx, st, "gs_write_testnode_metrics");
  }
  if (!pubsub.empty()) {
    std::vector<uint64_t> pc((size_t)cfg.peers * GS_PUBSUB_COLS);
    if ((st = gs_get_pubsub_counts(ctx, pc.data())) != GS_OK) return die(ctx, st, "gs_get_pubsub_counts");
    if ((st = gs_write_pubsub_metrics(&cfg, pubsub.c_str(), cfg.peers, pc.data())) != GS_OK)
      return die(ctx, st, "gs_write_pubsub_metrics");
  }
  if (!link_deliveries.empty()) {
    uint64_t nnz = 0;
    if ((st = gs_graph_info(ctx, nullptr, &nnz, nullptr)) != GS_OK) return die(ctx, st, "gs_graph_info");
    std::vector<uint64_t> row((size_t)cfg.peers + 1), ld((nnz + 1) * GS_LD_COLS);
    std::vector<uint32_t> col(nnz + 1);
    if ((st = gs_get_csr(ctx, row.data(), col.data(), nullptr)) != GS_OK) return die(ctx, st, "gs_get_csr");
    if ((st = gs_get_link_deliveries(ctx, ld.data())) != GS_OK) return die(ctx, st, "gs_get_link_deliveries");
    if ((st = gs_write_link_deliveries(link_deliveries.c_str(), cfg.peers, row.data(), col.data(), ld.data())) != GS_OK)
      return die(ctx, st, "gs_write_link_deliveries");
  }
  if (!message_costs.empty()) {  // (the table is the last gs_run / gs_run_log call's: the whole schedule)
    uint64_t rows = 0;
    if ((st = gs_message_costs_rows(ctx, &rows)) != GS_OK) return die(ctx, st, "gs_message_costs_rows");
    std::vector<uint64_t> mc((size_t)rows * GS_MC_COLS + 1);
    if ((st = gs_get_message_costs(ctx, mc.data(), rows)) != GS_OK) return die(ctx, st, "gs_get_message_costs");
    if (rows != sched.size()) return die(ctx, GS_ESTATE, "gs_message_costs_rows");
    if ((st = gs_write_message_costs(&cfg, message_costs.c_str(), sched.data(), rows, mc.data())) != GS_OK)
      return die(ctx, st, "gs_write_message_costs");
  }
  gs_destroy(ctx);
  return 0;
}
