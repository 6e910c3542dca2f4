// gs_internal.h — context layout and kernel-launch entry points shared by the
// translation units of libgossipsim (not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdlib.h>

#include <functional>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/gossipsim.h"
#include "gs_common.h"

#define GS_HIP(call)                                                                   \
  do {                                                                                 \
    hipError_t e_ = (call);                                                            \
    if (e_ != hipSuccess) throw gs::Error(GS_EDEVICE, std::string(#call) + ": " +      \
                                                          hipGetErrorString(e_));      \
  } while (0)

namespace gs {

struct Error {
  gs_status code;
  std::string msg;
  Error(gs_status c, std::string m) : code(c), msg(std::move(m)) {}
};

// One dispatch on a batch's lanes per message: f(std::integral_constant<int, FP>{}) for
// FP in {1, 2, 4, 8, 16}. FP = pow2_at_least(F) with F <= MAX_FRAGS, so the throw cannot fire.
template <class Fn>
void with_fp(uint32_t FP, Fn&& f) {
  switch (FP) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 8: return f(std::integral_constant<int, 8>{});
    case 16: return f(std::integral_constant<int, 16>{});
  }
  throw Error(GS_EINVAL, "internal: " + std::to_string(FP) + " lanes per message (not 1, 2, 4, 8 or 16)");
}

// Environment knobs (DESIGN.md §6.1 lists every one the library reads). Both
// call getenv every time: tests set os.environ between runs of one process. A
// knob read once per process is cached by its caller in a static.
// env_off: set, non-empty and 0 (the switches that are on unless turned off).
inline bool env_off(const char* name) {
  const char* e = getenv(name);
  return e && *e && atoi(e) == 0;
}
// env_int: the value, or dflt when unset or empty.
inline long env_int(const char* name, long dflt) {
  const char* e = getenv(name);
  return e && *e ? atol(e) : dflt;
}

// Device-side error word bits (set by kernels, checked by the host).
// ERR_LIST: a list pull candidate list overflowed; ERR_RING: a list pull candidate
// fell outside the K-window ring the host bound promised. Both re-run the batch on k_pull.
// ERR_LAT16: a logged latency of 65535 ms or more for the u16 stream (GS_WANT_LAT_MS).
// ERR_LINES: a peer's line counter of the arrival log's text would pass 2^32 - 1 in the batch (k_lt_room).
// ERR_LINK: a final key's src is not in the receiver's CSR row (k_linkdel, gs_linkdel.h).
enum : uint32_t {
  ERR_TIME = 1, ERR_HOPS = 2, ERR_MESH = 4, ERR_DEG = 8, ERR_LIST = 16, ERR_RING = 32, ERR_LAT16 = 64, ERR_LINES = 128,
  ERR_LINK = 256
};

// Device buffer owned by a context.
template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  void alloc(size_t count) {
    if (count <= n && p) return;
    release();
    if (count == 0) return;
    GS_HIP(hipMalloc((void**)&p, count * sizeof(T)));
    n = count;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
  ~DevBuf() { release(); }
};

// Counters written by kernels: index constants into Ctx::d_counters.
constexpr uint32_t H_PINNED_WORDS = 32;
constexpr uint32_t GLP_QUIET = 8;  // see glp_account (gs_run.h)

enum : uint32_t {
  C_FD = 0, C_R = 1, C_DELIV = 2, C_LAT_SUM = 3, C_LAT_MAX = 4, C_BUCKETS = 5,
  C_R_FWD = 6, C_MESH_CHANGES = 7, C_MESH_WAKE = 8, C_ERR = 9, C_PUSH = 10, C_GOSSIP = 11, C_PASSES = 12,
  C_GLISTED = 13, C_TSCANNED = 14, C_TSCANNED_G = 15,  // diagnostics (GS_DEBUG_COUNTS): gossip-listed
                                                       // lanes, tiles scanned, of them only for gossip
  C_COUNT = 16
};

// The pull and list passes' control, Ctx::d_pctrl (gs_pull_kernel.h): PS_SLOTS slots of
// {lo, mode, records emitted, min pending key}. Pass k writes slot k % 3 and decides from
// slot (k + 2) % 3; k_seed leaves the seeds' min key in the slot pass 0 decides from.
enum : uint64_t { PM_DONE = 0, PM_EMIT = 1, PM_PULL = 2 };
enum : uint32_t {
  PS_LO = 0, PS_MODE = 1, PS_RECORDS = 2, PS_MIN = 3, PS_WORDS = 4, PS_SLOTS = 3,
  PS_SEED_MIN = (PS_SLOTS - 1) * PS_WORDS + PS_MIN
};

// Ctx::h_pinned, the pinned host mirror. Words [0, HP_SCRATCH) are any call's read-back,
// valid from its copy to its next use of the mirror and no longer (collect_stats: C_COUNT
// words; part_lp_route_read: LP_PMAX; PRun::check_same_config: 16; the passes' PS_SLOTS
// slots). The words above are written by one function and read by another later on:
enum : uint32_t {
  HP_SCRATCH = 16,
  HP_GATHER = 16,    // [HP_GATHER_WORDS] PRun::gather's own row on its way to the device (gs_prun.h)
  HP_LP_ERR = 20,    // lpull_passes -> run_lpull_batch: the error word as of the last pass read ...
  HP_LP_BATCH = 21,  // [2] ... and a no-log batch's words LP_CT_TMAX, LP_CT_DELIV
  HP_LP_SET = 24,    // [2] part_lp_set's records and min pending key on their way to the device
  HP_SEED_MIN = 28,  // part_lp_begin -> part_lp_seed_min
  HP_LAT_ERR = 30,   // part_lat_stage -> part_lat_err
  HP_GATHER_WORDS = 4
};
static_assert(C_COUNT <= HP_SCRATCH && PS_SLOTS * PS_WORDS <= HP_SCRATCH, "a call's read-back stays in the scratch");
static_assert(HP_GATHER + HP_GATHER_WORDS <= HP_LP_ERR && HP_LP_ERR < HP_LP_BATCH && HP_LP_BATCH + 2 <= HP_LP_SET &&
                  HP_LP_SET + 2 <= HP_SEED_MIN && HP_SEED_MIN < HP_LAT_ERR && HP_LAT_ERR < H_PINNED_WORDS,
              "the named words of h_pinned are apart and inside it");

// Per-batch geometry (gs_relax.hip setup_batch).
struct Batch {
  uint32_t B = 0, L = 0, F = 0, FP = 1, sb = 0, tshift = 0, Fe = 1;
  uint64_t lat_min = 0;  // smallest latency between used link classes (lazy-gossip no-op proof)
  uint64_t lat_max = 0;  // largest latency between used link classes (IHAVE travel bound)
  uint64_t ans_max = 0;  // largest IHAVE-arrival -> IWANT-answer-arrival time (lat + ser + lat + dn)
  uint64_t ser_max = 0;      // largest uplink serialisation of a used link class
  uint64_t lat_adj_max = 0;  // largest lat(x->y) + max(0, ser_dn(y) - ser_up(x)) over used classes
  bool collide = false;
  uint64_t payload = 0, tmax = 0, delta = 1;
  std::vector<uint64_t> tpub;
};

struct Ctx {
  gs_config cfg{};
  std::string last_error;
  hipStream_t stream = nullptr;
  hipStream_t side = nullptr;           // second stream: churn IHAVE lists beside the epoch steps
  std::vector<hipEvent_t> side_ev;      // its chunk events
  hipStream_t chain_pipe = nullptr;  // churn runs: the chain's stream on its own XCD (GS_CHAIN_XCDS, default 0)
  hipEvent_t chain_ev[2] = {nullptr, nullptr};  // its join events with the context's stream (churn_ring)
  bool timing = false;
  bool traffic = false;        // gs_set_traffic: per-peer send/receive counters
  DevBuf<uint64_t> d_traffic;  // [N][GS_TRAFFIC_COLS]
  bool pubsub = false;         // gs_set_pubsub_counts (gs_pubsub.h): per-peer event counters
  DevBuf<uint64_t> d_pubsub;   // [N][GS_PUBSUB_COLS]
  // gs_set_link_deliveries (gs_linkdel.h): per-link first-delivery counters, aligned with the CSR
  bool linkdel = false;
  bool ld_ready = false;        // d_linkdel is allocated for the current graph and zeroed since the last reset
  DevBuf<uint64_t> d_linkdel;   // [nnz][GS_LD_COLS]
  // A pass over the finished batch's dense final keys follows (any of the switches): the run plan
  // keeps dense rows and the churn ring's ELL snapshots, and takes no path without them.
  bool keys_pass() const { return traffic || pubsub || linkdel || msgcost; }
  // gs_set_message_costs (gs_msgcost.h): the per-message cost table of the last gs_run / gs_run_log call
  bool msgcost = false;
  uint64_t mc_rows = 0;            // the call's messages (0 before a run and after enabling)
  DevBuf<uint64_t> d_msgcost;      // [mc_rows][GS_MC_COLS], rows in the order the run driver took the messages
  std::vector<uint64_t> mc_perm;   // row i is the schedule's message mc_perm[i] (class_plan); empty: row i is message i
  // gs_set_peer_delay (gs_peerdelay.h): per-peer delay accumulators of the context's own rows
  bool pdelay = false;
  DevBuf<uint64_t> d_pdelay;   // [PD_COLS][own rows]
  uint32_t pdelay_n = 0;       // the rows d_pdelay covers (0: zeroed at the next use, part_set after a new split)
  // gs_set_mesh_events (gs_meshev.h): the mesh events of the last gs_mesh_converge, all N peers
  bool meshev = false;
  bool meshev_valid = false;          // a converge finished since the switch went on
  DevBuf<uint64_t> d_me;              // [GS_MESH_EVENT_COLS][N] per-peer counts
  DevBuf<uint32_t> d_me_size;         // [N] mesh size after the last counted epoch
  DevBuf<uint64_t> d_ms;              // [me_cap][GS_MESH_SERIES_COLS] series rows of stepped epochs, in stepping order
  uint32_t me_cap = 0, me_used = 0;   // its rows, and those written since the last read-back
  std::vector<uint32_t> me_epochs;    // the epoch of every stepped row
  std::vector<uint64_t> me_stepped;   // the stepped rows read back so far
  std::vector<uint64_t> me_series;    // [out_epochs + 1][GS_MESH_SERIES_COLS]: every epoch's row (me_finish)

  // links
  uint32_t S = 0;
  std::vector<uint64_t> lat_ns, bw_up, bw_dn;
  std::vector<uint8_t> stage_host;
  std::vector<uint8_t> stage_used;  // [S] 1 if some peer sits on that link class
  bool links_set = false;

  // graph (device resident)
  bool topo_built = false, mesh_built = false;
  uint32_t k = 0;            // dials per peer
  uint64_t nnz = 0;
  uint32_t max_degree = 0;
  uint64_t topo_fp = 0;      // fingerprint of an imported graph (gs_set_topology*); 0: gs_build_topology's
  uint64_t mesh_fp = 0;      // fingerprint of an imported mesh (gs_set_mesh*); 0: a converged or loaded one
  DevBuf<uint8_t> d_stage;
  DevBuf<uint32_t> d_dial;   // [N*k]
  DevBuf<uint8_t> d_acc;     // [N*k] dial accepted
  DevBuf<uint64_t> d_row;    // [N+1]
  DevBuf<uint32_t> d_col;    // [nnz]
  DevBuf<uint8_t> d_flags;   // [nnz] F_OUT | F_MESH
  DevBuf<uint32_t> d_rev;    // [nnz] index of the reverse entry
  DevBuf<uint32_t> d_until;  // [nnz] back-off: graft refused while epoch < until
  DevBuf<uint8_t> d_prop;    // [nnz] per-epoch GRAFT/PRUNE/ACCEPT bits
  DevBuf<uint8_t> d_iprop;   // [nnz] event-driven epochs: the GRAFT/PRUNE bits a neighbour proposed, at the receiver's entry
  DevBuf<uint32_t> d_mesh;   // [N*MESH_W] packed stage<<24|peer, EMPTY padded
  DevBuf<uint32_t> d_lat32;  // [S*S] u32 latency for the mesh kernels
  bool lat32_ok = false;     // d_lat32 holds the current links
  // churn: ring of per-epoch snapshots, slot = epoch % ring_R
  DevBuf<uint32_t> d_ring_mesh; // [R][N][MESH_W]
  DevBuf<uint64_t> d_ring_off;  // [R][(N+63)/64]
  DevBuf<uint32_t> d_ring_in;     // lazy gossip: [R][N][GT_IN] senders of the IHAVEs reaching a peer per epoch
  DevBuf<uint64_t> d_gout;        // scratch of ring_in_lists: IHAVE target masks over CSR rows, per (epoch, sender)
  DevBuf<uint8_t> d_csrpos;       // [nnz] position of the row's peer in its neighbour's row (ring_in_lists, GOS)
  bool csrpos_valid = false;      // d_csrpos is of the current CSR
  DevBuf<uint64_t> d_ring_mm;     // [R][N] mesh of each epoch as a mask over the CSR row (max_degree <= 64)
  std::vector<uint64_t> ring_in_tag;  // [R] epoch whose inverse IHAVE lists a slot holds (~0: none)
  bool ring_in_defer = false;         // the churn list pass takes the batch: no inverse lists beside the epochs
  // the ELL snapshots too: a churn list-pass batch reads only the mask ring, so the
  // epochs skip the ELL copy and ensure_ring_ell rebuilds a slot from its mask when
  // another reader needs it (push-path fallback, non-flood seeds, traffic)
  std::vector<uint64_t> ring_ell_tag;  // [R] epoch whose ELL snapshot a slot holds (~0: none)
  bool ring_ell_defer = false;
  // called by the epoch chain after it enqueued epoch h on the context's stream (and once with
  // h0 - 1 when the run's offline bits are written): the churn list pass's tables of the epochs
  // done so far go to the side stream (gs_relax.hip chn_chunks)
  std::function<void(uint64_t)> epoch_hook;
  std::vector<hipEvent_t> cp_ev[2];   // their events, per table set
  DevBuf<uint64_t> d_q0, d_r0;  // [B] epoch of t_pub, t_pub - start of that epoch
  uint32_t ring_R = 0;
  uint64_t churn_state = 0, ring_lo = 1, ring_hi = 0;  // mesh state epoch; valid ring epochs
  DevBuf<uint8_t> d_mcnt;    // [N]
  DevBuf<uint8_t> d_pst;     // event-driven churn epochs: [PS_PLANES][N] per-peer flags and counts
  DevBuf<uint64_t> d_offlin; // offline bitsets of a run of churn epochs, [epochs + 1][(N+63)/64]
  // a caller's outages in place of the draw (gs_set_outages, gs_outages.h): each peer's sorted, disjoint
  // intervals as a CSR of h_to << 32 | h_from words, on the device and on the host
  bool outages_on = false;
  uint64_t outage_fp = 0;       // fingerprint of the imported schedule; 0: the draw
  DevBuf<uint32_t> d_og_ptr;    // [N+1]
  DevBuf<uint64_t> d_og_iv;
  std::vector<uint32_t> og_ptr;
  std::vector<uint64_t> og_iv;
  // Is peer u offline in heartbeat epoch h, from whichever source is active (the host's
  // publisher-online checks; the device's bitsets come from k_offline_range / k_outage_range).
  bool offline(uint32_t u, uint64_t h) const {
    if (!outages_on) return offline_draw(cfg.seed, cfg.churn_ppm, cfg.churn_down, u, h);
    if (h == 0) return false;
    uint32_t lo = og_ptr[u], hi = og_ptr[u + 1];
    const uint32_t b = lo;
    while (lo < hi) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if ((uint32_t)og_iv[mid] <= h) lo = mid + 1; else hi = mid;
    }
    if (lo == b) return false;
    const uint32_t to = (uint32_t)(og_iv[lo - 1] >> 32);
    return to == 0xFFFFFFFFu || h < to;
  }

  // dissemination (per batch)
  DevBuf<uint64_t> d_keys;   // [N * B * FP] peer-major (u, m, f)
  DevBuf<uint64_t> d_busy;   // [N * B] uplink FIFO end per (u, m) (F > 1)
  DevBuf<uint64_t> d_fbits;  // final bitset, one u64 per 64-lane tile
  DevBuf<uint32_t> d_fr_idx; // bucket frontier (per-scan-wave segments)
  DevBuf<uint64_t> d_fr_key;
  DevBuf<uint32_t> d_fr_cnt;
  DevBuf<uint64_t> d_tmin;   // split tile skip: min pending key per tile
  DevBuf<uint8_t> d_touched; // split tile skip: pushed since last scan
  DevBuf<uint64_t> d_tgmin;  // split tile skip + gossip: next IHAVE arrival per tile
  DevBuf<uint32_t> d_tnf;    // split tile skip + gossip: non-final lanes per tile
  DevBuf<uint32_t> d_tstamp; // split tile skip + gossip: launch + 1 of the last scan
  DevBuf<uint32_t> d_gl_idx; // lazy gossip: lanes with an IHAVE arrival in the bucket
  DevBuf<uint32_t> d_gl_cnt;
  DevBuf<uint64_t> d_gl_key; // receiver-centric gossip: the listed lane's key (saves its re-read)
  DevBuf<uint32_t> d_hl_idx;  // churn + gossip: holder list (RelaxArgs::hl_*): lane, key, count, launch marks
  DevBuf<uint64_t> d_hl_key;
  DevBuf<uint64_t> d_hl_cnt;
  DevBuf<uint64_t> d_hl_mark;
  DevBuf<uint32_t> d_hs_idx;  // per scan wave scratch of the holders found (copied to the list)
  DevBuf<uint64_t> d_hs_key;
  DevBuf<uint64_t> d_hl_min;
  DevBuf<uint8_t> d_hwin;     // [N][L] first gossip heartbeat of each final lane (RelaxArgs::hwin)
  DevBuf<uint64_t> d_nonfinal;  // [3]
  DevBuf<uint64_t> d_rel0;   // [B] first heartbeat >= t_pub (relative ns)
  DevBuf<uint64_t> d_habs0;  // [B] its absolute heartbeat index
  DevBuf<uint8_t> d_malive;  // [B] churn + gossip: the message can spread (publisher online at t_pub)
  DevBuf<uint32_t> d_pub;    // [B]
  DevBuf<uint64_t> d_tpub;   // [B]
  DevBuf<uint64_t> d_tc;     // [N * B] peer-major completion times (device result)
  DevBuf<uint8_t> d_hops;    // [N * B]
  DevBuf<uint64_t> d_tc_t;   // [B * N] message-major staging for the caller's sink
  DevBuf<uint8_t> d_hops_t;
  DevBuf<uint16_t> d_lat;    // [N * B] peer-major logged latency in ms (GS_WANT_LAT_MS)
  DevBuf<uint16_t> d_lat_t;  // [B * N] message-major staging of it
  hipEvent_t blk_ev[2] = {nullptr, nullptr};  // double-buffered streaming: D2H of block k done
  // latency-only sinks inside gs_run (gs_relax.hip deliver_lat_async): a finished
  // batch's u16 latencies leave on the copy stream into a whole-batch pinned
  // buffer while the next batch's passes run; its callbacks run at the next
  // batch's delivery or at the end of the run (message order kept)
  bool lat_async = false;
  hipStream_t copy = nullptr;
  DevBuf<uint16_t> d_lat_t2;                  // the other parity's message-major staging
  uint16_t* h_lat[2] = {nullptr, nullptr};    // pinned [B][un] per parity
  size_t h_lat_bytes[2] = {0, 0};
  uint64_t* h_laterr = nullptr;               // pinned: the error word after each parity's batch
  hipEvent_t lat_src[2] = {nullptr, nullptr}, lat_done[2] = {nullptr, nullptr};
  struct LatPending {
    bool on = false;
    uint32_t par = 0, B = 0, un = 0, bm = 64;
    uint64_t row0 = 0;
    const gs_result_sink* sink = nullptr;
  } lat_pend;
  uint32_t lat_par = 0;
  // the arrival log as text (gs_logtext.h; gs_run_log, gs_format_lat_log): the callback of the
  // call in progress (fn set = deliver hands a batch's latencies to the formatter), the
  // per-peer line counters, a chunk's line numbers / group sums / group offsets / ids, and
  // the two device and pinned text buffers with their events
  struct TextRun {
    gs_text_fn fn = nullptr;
    void* user = nullptr;
    uint64_t chunk = 0;
    const gs_publish* sched = nullptr;
  } text;
  // (N below: the context's own peers, all of them or a part's range [part_u0, part_u0 + part_un))
  DevBuf<uint32_t> d_tcnt;   // [N]
  uint32_t tcnt_n = 0;       // the rows d_tcnt counts (0: zeroed at the next use, part_set after a new split)
  DevBuf<uint32_t> d_tln;    // [chunk msgs][N]
  DevBuf<uint32_t> d_tgsum;  // [chunk msgs][(N + 63) / 64]
  DevBuf<uint64_t> d_tgoff;
  DevBuf<uint8_t> d_tids;    // [B][24]
  DevBuf<uint64_t> d_tmeta;  // [4] bytes, lines, counter overflow
  DevBuf<char> d_text[2];
  char* h_text[2] = {nullptr, nullptr};
  size_t h_text_bytes[2] = {0, 0};
  uint64_t* h_tmeta = nullptr;  // pinned [2][4]
  hipEvent_t text_meta_ev[2] = {nullptr, nullptr}, text_fmt_ev[2] = {nullptr, nullptr},
             text_done_ev[2] = {nullptr, nullptr};
  uint32_t text_par = 0;
  bool text_busy = false;
  // gs_run_partitioned's latencies (part_lat_stage): d_lat_t holds the batch's message-major
  // latencies and the error word is on its way to h_pinned[HP_LAT_ERR] (deliver skips both steps)
  bool lat_staged = false;
  DevBuf<uint64_t> d_lr_tpub;  // [B] a message-sharded batch's publish times and publishers (k_lat_rows)
  DevBuf<uint32_t> d_lr_pub;
  DevBuf<uint32_t> d_tables; // lat[S*S] | ser_up[S] | ser_dn[S] (u32 ns)
  DevBuf<uint64_t> d_ctrl;   // [4] triple-buffered next-min keys + spare
  // owner-computes pull path (gs_pull_kernel.h)
  DevBuf<uint32_t> d_chunkmin; // [N][16] per 64-lane chunk: hi word of the min key beyond the last emitted window
  DevBuf<uint64_t> d_lrec;   // [2][N][L] per-row arrival records (gs_pull_kernel.h)
  DevBuf<uint32_t> d_lcnt;   // [2][N]
  DevBuf<uint8_t> d_rpos;    // [N][MESH_W] index of w in mesh(mesh[w][j])
  // batch slices (gs_relax.hip run_slices): S copies of the graph's mesh rows, reverse
  // positions and stages; the slices' publishers as slice rows and as peers
  DevBuf<uint32_t> d_smesh;  // [S * N][MESH_W]
  DevBuf<uint8_t> d_srpos;
  DevBuf<uint8_t> d_sstage;  // [S * N]
  DevBuf<uint32_t> d_spub;   // [S][B]
  DevBuf<uint32_t> d_lpub;
  DevBuf<uint64_t> d_cnt_save2;  // [C_COUNT] counters around a slice group's repeated completions
  DevBuf<uint64_t> d_stpub;  // [S][B] the slices' publish times
  uint64_t* h_slms = nullptr;  // pinned [S][B][MS_COLS]: every slice's reductions for the gossip no-op proof
  size_t h_slms_bytes = 0;
  bool rpos_valid = false;
  bool keys_log = false;       // keys hold the list pull path's final logs (not dense rows): k_lcomplete
  bool keys_none = false;      // the last batch ran the no-log list pass: keys hold neither rows nor logs
  uint32_t mesh_dmax = 0;      // widest frozen-mesh row (list pull ring bound); 0 = not known
  DevBuf<uint64_t> d_pctrl;  // [PS_SLOTS][PS_WORDS] pass control slots, then the no-log pass's batch words (LP_CT_WORDS)
  // list pull path (gs_lpull_kernel.h)
  DevBuf<uint64_t> d_lblk;   // [K][N][L] candidate lists per destination-window slot
  DevBuf<uint32_t> d_lst;    // [N][16] list lengths per destination window, final-log length
  DevBuf<uint64_t> d_skey;   // list pull path: the publishes' first sends (k_seed -> k_lseed)
  DevBuf<uint32_t> d_slane;  // (row << 11) | lane
  DevBuf<uint32_t> d_scnt;
  DevBuf<uint64_t> d_lp_save;  // [C_COUNT] counters before a list pull batch (overflow re-run)
  DevBuf<uint32_t> d_lfin;   // [N][32] final bits
  DevBuf<uint16_t> d_flane;  // [N][L] lanes of the final log
  DevBuf<uint64_t> d_counters;  // [C_COUNT]
  DevBuf<uint64_t> d_cnt_save;  // [C_COUNT] counters before a batch (gossip fallback restores them)
  uint64_t* h_pinned = nullptr; // pinned host mirror of ctrl + counters (H_PINNED_WORDS; the HP_ words above)
  // per-message reductions of k_complete / k_pct (gs_relax.hip)
  DevBuf<uint64_t> d_mstat;     // [B][MS_COLS]
  DevBuf<uint32_t> d_hist;      // [B][GS_HIST_BINS]
  DevBuf<uint32_t> d_pbin;      // [B][2]
  DevBuf<uint32_t> d_fine;      // [B][2][GS_HIST_MS]
  void* h_block = nullptr;      // pinned staging of streamed result blocks (gs_result_sink.on_block)
  bool sink_dev = false;        // the sink's arrays are device memory (message-sharded partitioned batches)
  DevBuf<uint64_t> d_ms_tc;     // message-sharded partitioned batch: this part's messages [mp][N] ...
  DevBuf<uint8_t> d_ms_hops;
  DevBuf<uint64_t> d_ms_send;   // ... packed per destination part (RCCL)
  DevBuf<uint8_t> d_ms_sendh;
  size_t h_block_bytes = 0;

  // peer-partitioned mode (gs_part.h): this context holds keys of peers [u0, u0 + un)
  uint32_t part_parts = 1, part_idx = 0, part_u0 = 0, part_un = 0;
  bool part_open = false;       // between gs_part_begin and gs_part_finish
  Batch part_b;
  unsigned part_grid = 0;
  uint32_t part_seg_cap = 0;
  DevBuf<uint64_t> d_pcnt;      // [4] frontier groups, records, relax min key, spare
  DevBuf<uint64_t> d_dcnt, d_dpos;  // [64] records per destination part / their write cursors
  DevBuf<gs_part_record> d_pout, d_pin;  // gs_run_partitioned: records sent / received this bucket
  // gs_run_partitioned on the list pass (gs_part.h part_lp_*): this part's rows in the list
  // buffers above (local row indexing); every peer's records of the last pass, packed
  bool part_lp = false;
  uint32_t part_lpK = 0, part_lplb = 0, part_lppass = 0;
  unsigned part_lpgrid = 0;
  DevBuf<uint32_t> d_rcg;    // [N] records per peer (global ids)
  DevBuf<uint64_t> d_roffg;  // [N] their offsets in d_rpk
  DevBuf<uint64_t> d_rpk;    // every part's records of the last pass
  hipEvent_t part_xev = nullptr;  // loop-back routed stores of the last pass done (other parts wait on it)
  hipEvent_t part_pev = nullptr;  // loop-back: this part's pass done (part 0's combine waits on it)
  DevBuf<uint64_t> d_pstat;       // loop-back, part 0: every part's pass control (k_part_combine)
  uint64_t* h_pstat = nullptr;    // its pinned read-back (LP_PMAX x 4 words)
  DevBuf<uint64_t> d_pkcur;  // pack cursor (routed: one per destination part)
  // routed exchange (k_lpack_route): the records for each other part [P][cap] and
  // this part's per-peer offsets / counts for each destination [P][un]
  DevBuf<uint64_t> d_rsend;
  DevBuf<uint64_t> d_rroff;
  DevBuf<uint32_t> d_rrcg;
  // lazy gossip inside the list pass (gs_lpull_kernel.h, GOS batches)
  DevBuf<uint32_t> d_gpl;      // [N][32] sender planes of the built heartbeat
  DevBuf<uint64_t> d_gse;      // [N][L] their entries
  DevBuf<uint32_t> d_rowdone;  // [(N + 31) / 32]
  DevBuf<uint64_t> d_gctl;     // [GC_WORDS]
  bool glp_prefer = false;     // the last eager no-op proof failed: run gossip batches on the list pass first
  uint32_t glp_quiet = 0;      // list-pass gossip batches in a row without an IWANT (GLP_QUIET clears glp_prefer)
  // churn on the list pass (gs_cpull.h, k_lpull<.., CHN>): the CSR rows as 64-wide ELL rows (once
  // per topology), per batch the per-epoch mesh / IHAVE-eligible masks of every row over the
  // batch's epochs, each peer's offline epochs, and the offline lanes per relative epoch
  DevBuf<uint32_t> d_ccol;     // [N][64] stage << 24 | peer, ascending, EMPTY padded
  DevBuf<uint8_t> d_cpos;      // [N][64] position of the row's peer in that neighbour's row
  bool cell_valid = false;
  // the churn list pass's per-batch tables, two sets: the next batch's are built
  // (its epoch chain beside this batch's passes) while this batch's are read
  struct ChnTables {
    DevBuf<uint64_t> cmm, cgt;  // [N][cE] mesh / IHAVE targets of each epoch as masks over the CSR row
    DevBuf<uint64_t> offe;      // [N][cW] offline bit per epoch of the batch range
    DevBuf<uint32_t> coff;      // [H + 2][N][32] offline lanes per relative epoch (transposed like the final bits)
    DevBuf<uint32_t> cq;        // [B] epoch of t_pub - first epoch of the range
    DevBuf<uint8_t> pubok;      // [B] the publisher was online at t_pub
    DevBuf<uint32_t> calive;    // [32] published lanes in the final bits' transposed layout
  } ct[2];
  uint32_t ct_par = 0;          // the table set the next batch prepared in line uses
  std::function<void()> pass_poll;  // called by the list pass between groups of passes (the chain ahead)
  uint64_t run_batch = 0;           // the batch loop's iteration in this gs_run call (Run::run, GS_LPULL_CAP_BATCHES)
  hipStream_t pass_ms = nullptr;    // churn runs: the passes' stream off the chain's XCDs (GS_PASS_XCDS)
  hipEvent_t pass_ev[2] = {nullptr, nullptr};
  DevBuf<uint8_t> d_gnz;       // [N] the row's IHAVE plane of the built heartbeat is not empty
  DevBuf<uint16_t> d_gtag;     // [N] the built heartbeat (GC_BK) whose IHAVEs the row takes by scanning planes
  DevBuf<uint32_t> d_gpc;      // [N] IHAVE entries pushed to the row per heartbeat (bk << 16 | count)
  DevBuf<uint64_t> d_luni;     // [2][N] per pass: OR of the receiver masks of a row's records

  // stats
  gs_stats stats{};
  std::vector<hipEvent_t> ev_pool;
  size_t ev_n = 0;  // timing: the cursor of the run in progress into ev_pool (run_ev below)
  int num_cus = 0;
  std::string gossip_why;  // the message that broke the last partitioned gossip no-op proof

  ~Ctx();
  void fail(gs_status c, const std::string& m) { throw Error(c, m); }
};

// Timing events come from a per-context pool: [0] run start, [1] run end, then
// one (start, scan end, end) triple around every relaxation launch; c.ev_n is
// the cursor of the run in progress (Run, gs_run.h; PRun, gs_prun.h).
inline hipEvent_t run_ev(Ctx& c, size_t i) {
  while (c.ev_pool.size() <= i) {
    hipEvent_t e;
    GS_HIP(hipEventCreate(&e));
    c.ev_pool.push_back(e);
  }
  return c.ev_pool[i];
}

// The arrival log as text: Ctx::text holds the callback for the length of one call
// (gs_run_log, gs_format_lat_log, gs_run_partitioned_log), whose latency-only sink's
// on_lat is never called.
inline void text_sink_unused(void*, uint64_t, uint32_t, uint32_t, const uint16_t*) {}
struct TextCall {
  Ctx* c;
  TextCall(Ctx* ctx, const gs_publish* sched, gs_text_fn fn, void* user, uint64_t chunk) : c(ctx) {
    c->text.fn = fn;
    c->text.user = user;
    c->text.chunk = chunk;
    c->text.sched = sched;
  }
  TextCall(const TextCall&) = delete;
  ~TextCall() { c->text = Ctx::TextRun{}; }
};
void check_sink(Ctx& c, const gs_result_sink* sink);  // gs_ctx.hip: gs_run's rules for a sink

// ---- launchers (gs_topology.hip / gs_mesh.hip / gs_relax.hip) ----
void launch_topology(Ctx& c);
void import_csr(Ctx& c, const uint64_t* row_ptr, const uint32_t* col, const uint8_t* flags);  // gs_set_topology
void import_dials(Ctx& c, uint64_t n, const uint32_t* dialer, const uint32_t* target);        // gs_set_topology_dials
void graph_replaced(Ctx& c);  // the context holds another graph than before (an import, a build after one)
uint32_t run_mesh(Ctx& c, uint32_t max_heartbeats);
void import_mesh_ell(Ctx& c, const uint32_t* mesh, const uint8_t* count);                  // gs_set_mesh
void import_mesh_links(Ctx& c, uint64_t n, const uint32_t* a, const uint32_t* b);         // gs_set_mesh_links
// a caller's outages in place of the churn draw (gs_outages.h)
void import_outages(Ctx& c, uint64_t n, const uint32_t* peer, const uint32_t* h_from, const uint32_t* h_to);  // gs_set_outages
void clear_outages(Ctx& c);                                                                                  // gs_clear_outages
void get_offline(Ctx& c, uint64_t h_lo, uint64_t h_hi, uint64_t* bits);                                        // gs_get_offline
inline void ensure_cus(Ctx& c) {
  if (c.num_cus == 0) {
    hipDeviceProp_t prop;
    c.num_cus = hipGetDeviceProperties(&prop, c.cfg.device) == hipSuccess ? prop.multiProcessorCount : 256;
  }
}
hipStream_t xcd_stream(Ctx& c, uint32_t xcds);
uint32_t xcd_env(const char* name);
void churn_ring(Ctx& c, uint64_t h_lo, uint64_t h_hi);
// the epoch chain in slices (gs_mesh.hip): nullptr when [churn_state + 1, h1] is
// no plain continuation inside the ring (the caller runs churn_ring instead)
struct EvRun;
EvRun* chain_begin(Ctx& c, uint64_t h1, hipStream_t s, std::function<void(uint64_t)> hook);
bool chain_advance(Ctx& c, EvRun& r, uint64_t max_epochs);  // true once every epoch is enqueued
void chain_free(EvRun* r);
void ensure_csrpos(Ctx& c);
void ensure_in_lists(Ctx& c, uint64_t h0, uint64_t h1);
void ensure_ring_ell(Ctx& c, uint64_t h0, uint64_t h1);
hipStream_t side_stream(Ctx& c);
void run_messages(Ctx& c, const gs_publish* sched, uint64_t n_msgs, const gs_result_sink* sink);
void deliver_rows(Ctx& c, uint32_t B, uint32_t un, const gs_result_sink* sink, uint64_t sink_row0);
// the arrival log as text (gs_logtext.h): c.text holds the callback
void format_lat_log(Ctx& c, const gs_publish* sched, uint64_t n_msgs, const uint16_t* lat_ms);
void log_text_reset(Ctx& c);
// per-peer delay accumulators (gs_peerdelay.h)
void pubsub_set(Ctx& c, bool on);
void pubsub_reset(Ctx& c);
void pubsub_get(Ctx& c, uint64_t* out);
// per-link first-delivery counters (gs_linkdel.h)
void linkdel_set(Ctx& c, bool on);
void linkdel_reset(Ctx& c);
void linkdel_get(Ctx& c, uint64_t* out);
void linkdel_given(Ctx& c, uint64_t* out);
// per-message cost table (gs_msgcost.h)
void msgcost_set(Ctx& c, bool on);
void msgcost_begin(Ctx& c, uint64_t n);
void msgcost_get(Ctx& c, uint64_t* out);
// mesh event counts of the last converge (gs_meshev.h, gs_mesh.hip)
void mesh_events_set(Ctx& c, bool on);
void mesh_events_get(Ctx& c, uint64_t* out);
void peer_delay_set(Ctx& c, bool on);
void peer_delay_reset(Ctx& c);
void peer_delay_get(Ctx& c, gs_peer_delay* out);
void peer_delay_add_lat(Ctx& c, const gs_publish* sched, uint64_t n_msgs, const uint16_t* lat_ms);
void part_set(Ctx& c, uint32_t parts, uint32_t part);
uint64_t part_begin(Ctx& c, const gs_publish* sched, uint64_t n_msgs);
bool part_scan(Ctx& c, uint64_t bucket_key, gs_part_record* rec, uint64_t cap, uint64_t* n, uint64_t* m1);
uint64_t part_relax(Ctx& c, uint64_t bucket_key, const gs_part_record* rec, uint64_t n);
void part_finish(Ctx& c, const gs_result_sink* sink);
// device-driven partitioned protocol (gs_prun.h)
void part_dev_bucket(Ctx& c, uint32_t parts);
void part_dev_scan_count(Ctx& c, uint32_t parts);
void part_dev_export(Ctx& c, uint32_t parts, gs_part_record* out);
void part_dev_relax_next(Ctx& c, const gs_part_record* in, uint64_t n);
bool part_dev_complete(Ctx& c, bool hist, bool store = true, bool lat = false);
void part_dev_finish(Ctx& c, const gs_result_sink* sink, uint64_t row0);
// the u16 latencies of a partitioned batch (gs_relax.hip): message-major into d_lat_t with the
// error word on its way to the host (enqueued), the word once it is there, the hand-over
void part_lat_stage(Ctx& c, uint32_t B, const gs_publish* ms_sched);
uint64_t part_lat_err(Ctx& c);
void part_lat_deliver_ms(Ctx& c, uint32_t B, const gs_result_sink* sink, uint64_t row0);
void part_abort(Ctx& c);
bool part_needs_ms(Ctx& c, const gs_publish* sched, uint64_t n_msgs);
// the list pass over partitioned rows (gs_part.h)
bool part_lp_begin(Ctx& c, const gs_publish* sched, uint64_t n_msgs);  // enqueued: then part_lp_seed_min
uint64_t part_lp_seed_min(Ctx& c);  // wait for the part's seeds: their min key
void part_lp_pass(Ctx& c);
void part_lp_read(Ctx& c, uint64_t out[4]);  // last pass: mode, records, min pending, error word
void part_lp_read_enqueue(Ctx& c);                   // part_lp_read in two steps
void part_lp_read_wait(Ctx& c, uint64_t out[4]);
void part_lp_combine(Ctx** cx, uint32_t P, uint64_t* st);  // loop-back on one device: read + set of all parts
void part_lp_set(Ctx& c, uint64_t records, uint64_t minp);  // the combined values into the last pass's slot
void part_lp_pack(Ctx& c, uint64_t base, uint64_t mine);
void part_lp_pack_route(Ctx& c, uint32_t P, uint32_t me, uint64_t mine);
void part_lp_pack_route_direct(Ctx** cx, uint32_t P, uint32_t me, uint64_t base);
void part_lp_route_read(Ctx& c, uint32_t P, uint64_t* counts);
void part_lp_route_fix(Ctx& c, uint32_t P, uint32_t me, const uint64_t* base);
void part_lp_end_enqueue(Ctx& c, const gs_result_sink* sink);  // completion (final logs or dense rows)
bool part_lp_end_check(Ctx& c);  // wait, then the gossip proof
void part_lp_abort(Ctx& c);

// small device helpers
void device_exclusive_scan(Ctx& c, const uint64_t* in, uint64_t* out, uint32_t n);
uint64_t read_counter(Ctx& c, uint32_t idx);

}  // namespace gs
