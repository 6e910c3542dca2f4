/*
 * gossipsim.h — C ABI of the MI355X-native GossipSub dissemination simulator.
 *
 * This is the drop-in boundary for the reference's hot path: message
 * dissemination across the GossipSub peer mesh of vacp2p/dst-libp2p-test-node.
 * In the reference that path sits behind rust-libp2p's NetworkBehaviour
 * (libp2p-gossipsub 0.49.2, not vendored; pinned at
 * rust-test-node/Cargo.lock:1640) and is driven by rust-test-node/src/main.rs.
 * Every entry point below names the reference interface it replaces.
 *
 * Conventions
 *  - Plain C: fixed-width integers, plain pointers and sizes, no C++ types.
 *  - Every call returns gs_status (0 = OK, negative = error); the message of the
 *    last failure is available from gs_last_error(ctx). No exception crosses
 *    the ABI.
 *  - The caller owns every host array it passes in; the library owns the
 *    device buffers of a context.
 *  - A context is bound to ONE HIP device and is not thread-safe: use one host
 *    thread per context. Multi-GPU = one context per GPU, each simulating its
 *    own message shard (message batches are independent).
 *  - All simulated times are integer nanoseconds.
 */
#ifndef GOSSIPSIM_H
#define GOSSIPSIM_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GS_ABI_VERSION 10u

/* Sentinel for "never delivered" in t_complete_ns. */
#define GS_UNDELIVERED UINT64_MAX

typedef int32_t gs_status;
enum {
    GS_OK = 0,
    GS_EINVAL = -1,       /* bad argument / knob combination               */
    GS_ENOMEM = -2,       /* host or device allocation failed              */
    GS_EDEVICE = -3,      /* HIP runtime error or no usable device         */
    GS_ESTATE = -4,       /* call out of order (e.g. run before topology)  */
    GS_ERANGE = -5,       /* a packed field overflowed (time, hops, mesh)  */
    GS_EUNSUPPORTED = -6  /* knob recognised but not implemented yet       */
};

/* MUXER (rust-test-node/src/env.rs:48-50,69-71; nim adds mplex,
 * nim-test-node/gossipsub-queues/main.nim:433-441). */
enum { GS_MUX_YAMUX = 0, GS_MUX_QUIC = 1, GS_MUX_MPLEX = 2 };

/* Node flavour whose gossipsub settings, payload layout and log line the
 * simulator reproduces (gs_config_preset): rust-test-node (the north star),
 * go-test-node, nim-test-node/gossipsub-queues. */
enum { GS_NODE_RUST = 0, GS_NODE_GO = 1, GS_NODE_NIM = 2 };

/* Link-table mode for gs_topogen_links. */
enum {
    GS_LINKS_DIRECT = 0,   /* latency of the direct GML edge (topogen intent)       */
    GS_LINKS_SHORTEST = 1  /* shortest path over the GML graph incl. injector hub  */
};

/* Simulator configuration. Field meaning follows the reference's knobs:
 * rust-test-node/src/env.rs:27-87 (PEERS, CONNECTTO, FRAGMENTS, MUXER) and
 * rust-test-node/src/main.rs:223-241 (gossipsub ConfigBuilder). */
typedef struct gs_config {
    uint32_t abi_version;        /* must be GS_ABI_VERSION                         */
    uint32_t peers;              /* PEERS (env.rs:38-41)                           */
    uint32_t connect_to;         /* CONNECTTO (env.rs:43-46)                       */
    uint32_t dial_extra;         /* 1: rust/go dial CONNECTTO+1 (main.rs:337); 0: nim */
    uint32_t max_connections;    /* MAXCONNECTIONS inbound cap (nim main.nim:429); 0 = none */
    uint32_t fragments;          /* FRAGMENTS (env.rs:64-67)                       */
    uint32_t muxer;              /* GS_MUX_*                                       */
    uint32_t signed_msgs;        /* 1: MessageAuthenticity::Signed (main.rs:397)   */
    uint32_t d;                  /* mesh_n      (main.rs:231)                       */
    uint32_t d_lo;               /* mesh_n_low  (main.rs:232)                       */
    uint32_t d_hi;               /* mesh_n_high (main.rs:233)                       */
    uint32_t d_lazy;             /* gossip_lazy (main.rs:235)                       */
    uint32_t d_out;              /* mesh_outbound_min (main.rs:234)                 */
    uint32_t gossip_factor_milli;/* gossip_factor x 1000 (main.rs:230)              */
    uint64_t heartbeat_ns;       /* heartbeat_interval (main.rs:228)                */
    uint64_t backoff_ns;         /* prune_backoff (main.rs:229)                     */
    uint32_t flood_publish;      /* flood_publish (main.rs:227)                     */
    uint32_t idontwant;          /* IDONTWANT suppression (go main.go:165); 0 = off */
    uint32_t lazy_gossip;        /* IHAVE/IWANT gossip relaxations; 0 = off         */
    uint32_t self_log;           /* publisher logs its own message (nim SELFTRIGGER)*/
    uint64_t seed;               /* counter-RNG key (reference RNG is unseeded, main.rs:308) */
    int32_t  device;             /* HIP device ordinal                              */
    uint32_t batch;              /* messages simulated together per device batch    */
    uint32_t history_gossip;     /* mcache windows gossiped (upstream default 3)    */
    uint64_t hb_phase_ns;        /* heartbeats at hb_phase + h*heartbeat (absolute) */
    /* churn (BASELINE config #3; build-defined): each heartbeat
     * epoch every peer starts a churn_down-epoch outage with probability
     * churn_ppm / 1e6; the mesh evolves epoch by epoch and every send uses the
     * mesh of its epoch. 0 = frozen converged mesh. Needs hb_phase_ns within
     * 2^20 heartbeats of every publish. */
    uint32_t churn_ppm;
    uint32_t churn_down;         /* outage length in heartbeats (default 10)        */
    uint32_t churn_horizon;      /* message lifetime in heartbeats under churn: no  */
                                 /* event past epoch(t_pub) + horizon (default 16)  */
    uint32_t node;               /* GS_NODE_*: fragment layout + log line */
    /* subscription-time grafting (libp2p-gossipsub handle_received_subscriptions,
     * reached through the 20 s connection pump of main.rs:357-379): before
     * heartbeat 1 every peer grafts its first D_lo connections in handshake
     * order. 1 in the rust preset. */
    uint32_t sub_graft;
    /* round trips from the common dial instant until a connection carries its
     * first subscription (TCP + multistream + Noise XX + yamux; a model
     * constant of the subscription epoch); 0 = 3 (default) */
    uint32_t hs_rtts;
} gs_config;

/* One publish injection (replaces POST /publish, main.rs:50-56,152-168; the
 * PublishCommand of main.rs:65-71 carries msg_size and chunks). */
typedef struct gs_publish {
    uint64_t t_pub_ns;    /* absolute publish time = tx_time stamped at main.rs:105-111 */
    uint32_t publisher;   /* peer id that publishes                                     */
    uint32_t msg_size;    /* msgSize of the request; fragment payload = msg_size/F      */
    uint32_t frags;       /* F of this message (chunks, main.rs:163-168); 0 = cfg.fragments */
    uint32_t reserved;    /* 0                                                          */
} gs_publish;

/* Latency histogram bins of gs_msg_summary: 100 ms each (hop_lat of
 * shadow/summary_latency.awk:8), the last one open-ended. */
#define GS_HIST_BINS 64u
#define GS_HIST_MS 100u

/* Per-message reduction of one run, computed on the device:
 * latency = (t_complete - tx_time) / 1e6 truncated, as logged (main.rs:91-93),
 * over the peers that log the message (the publisher only with self_log). */
typedef struct gs_msg_summary {
    uint64_t delivered;            /* log lines of this message                          */
    uint64_t lat_sum_ms;
    uint32_t p50_ms, p95_ms;       /* nearest-rank percentiles: value at rank ceil(q*n)  */
    uint32_t max_ms;
    uint32_t reserved;
    uint32_t hist[GS_HIST_BINS];   /* hist[min(ms / 100, 63)]                            */
} gs_msg_summary;

/* Streaming receiver of results: called from gs_run on the caller's thread
 * with message-major blocks of at most `block_msgs` messages; the arrays are
 * library-owned and valid only during the call ([n_msgs][peers], either may
 * be NULL when gs_result_sink.want does not select it). */
typedef void (*gs_block_fn)(void* user, uint64_t first_msg, uint32_t n_msgs, uint32_t peers,
                            const uint64_t* t_complete_ns, const uint8_t* hops);

/* Streaming receiver of the logged latency (GS_WANT_LAT_MS, ABI 9): the
 * value each peer's log line carries, (t_complete - tx_time) / 1e6 truncated
 * (rust-test-node/src/main.rs:91-93), message-major [n_msgs][peers] u16;
 * GS_LAT_NONE where the peer logs nothing (undelivered; the publisher unless
 * cfg.self_log). 2 bytes per (peer, message) instead of the 9 of
 * t_complete + hops. A latency of 65535 ms or more fails the run (GS_ERANGE). */
typedef void (*gs_lat_fn)(void* user, uint64_t first_msg, uint32_t n_msgs, uint32_t peers, const uint16_t* lat_ms);
#define GS_LAT_NONE 0xFFFFu

/* Outputs a streaming sink delivers (gs_result_sink.want): t_complete and
 * hops through on_block, the logged latency through on_lat. */
enum { GS_WANT_T_COMPLETE = 1u, GS_WANT_HOPS = 2u, GS_WANT_LAT_MS = 4u };

/* Where gs_run puts results. Every member may be NULL / 0.
 *  - t_complete_ns / hops: caller arrays, message-major [n_msgs][peers];
 *    without on_block only; they must be NULL when on_block is set
 *    (GS_EINVAL otherwise: nothing is ever written through them then);
 *  - on_block: streaming delivery instead of the arrays (no [n_msgs][peers]
 *    host array is needed for large N); `want` selects what it receives
 *    (GS_WANT_* bits, 0 = both); ABI 7 (ABI 6 used non-NULL array pointers
 *    as the selection flags);
 *  - summary: [n_msgs] per-message latency reductions;
 *  - on_lat: the logged latency in ms, u16, streamed in the same blocks; set
 *    iff want has GS_WANT_LAT_MS (ABI 9). gs_run_partitioned streams each
 *    part's own peers: blocks of [n_msgs][own peers]. */
typedef struct gs_result_sink {
    uint64_t* t_complete_ns;  /* completion time of message m at peer u (GS_UNDELIVERED if never) */
    uint8_t*  hops;           /* hop count of the completing fragment (0 at the publisher)        */
    gs_block_fn on_block;
    void*     user;
    uint32_t  block_msgs;     /* messages per on_block call; 0 = 64                               */
    uint32_t  want;           /* GS_WANT_T_COMPLETE | GS_WANT_HOPS (on_block; neither = both)     */
                              /* | GS_WANT_LAT_MS (on_lat)                                        */
    gs_msg_summary* summary;
    gs_lat_fn on_lat;         /* ABI 9: the logged latency stream (GS_WANT_LAT_MS)                */
} gs_result_sink;

/* Counters accumulated since gs_create / gs_reset_stats. */
typedef struct gs_stats {
    uint64_t messages;          /* messages simulated                                  */
    uint64_t deliveries;        /* (peer,msg) completions at non-publishers = log lines */
    uint64_t frag_deliveries;   /* FD: fragment first arrivals at non-publishers       */
    uint64_t relaxations;       /* R: flood-publish sends + forward sends (dups incl.) */
    uint64_t bytes_alg;         /* 16*FD + 12*R + 8*deliveries           */
    uint64_t latency_sum_ms;    /* sum of per-delivery latency in ms (truncated)       */
    uint64_t latency_max_ms;    /* max per-delivery latency in ms                      */
    uint64_t relax_launches;    /* bucket-relaxation kernel launches                   */
    uint64_t buckets;           /* non-empty Delta-buckets processed                   */
    double   relax_ms;          /* device time of relaxation launches (timing on)      */
    double   run_ms;            /* device time of whole gs_run calls (timing on)       */
    uint64_t relax_bytes_alg;   /* 16*FD + 12*R_forward: algorithmic bytes of relax    */
    uint64_t pushes;            /* atomicMin pushes issued (forward sends not dropped  */
                                /* because the target was already final)              */
    double   scan_ms;           /* relax_ms split: bucket scan + compaction kernel     */
    double   frontier_ms;       /* relax_ms split: frontier forwarding kernel          */
    uint64_t gossip_iwant;      /* IWANT responses sent (counted in relaxations too)   */
    uint64_t gossip_noop_msgs;  /* lazy gossip on the pull path: messages proven to      */
                                /* finish everywhere before their first IHAVE can land    */
                                /* (no IWANT possible)                   */
    uint64_t gossip_fallback_batches; /* batches re-run on the push path with gossip    */
    uint64_t batches;           /* device batches run (gs_run splits at cfg.batch, size /  */
                                /* chunk changes and the churn snapshot ring)             */
    uint64_t list_pull_batches; /* batches whose eager passes ran on candidate lists      */
                                /* (k_lpull) rather than dense rows       */
    uint64_t ms_batches;        /* gs_run_partitioned batches run message-sharded (ABI 8) */
    uint64_t gossip_list_batches; /* batches whose lazy gossip ran inside the list pass    */
                                /* (IHAVE / IWANT decided per window, ABI 9; §2.7)        */
} gs_stats;

/* ---- host-only helpers (no device work) ---------------------------------- */

/* Defaults of the rust preset (main.rs:36-38,223-241; env.rs:38-67). */
void gs_config_default(gs_config* cfg);

/* Overwrite cfg with the defaults of one node flavour (gs_config_default +
 * the node's own settings):
 *  GS_NODE_RUST  rust-test-node/src/main.rs:223-241 (= gs_config_default);
 *  GS_NODE_GO    go-test-node/main.go:153-175,374-385: Dout 2, IDONTWANT
 *                threshold 1000 B, StrictNoSign (unsigned), local delivery of
 *                own messages (self log), 8-byte stamp + msg_size/F payload;
 *  GS_NODE_NIM   nim-test-node/gossipsub-queues/main.nim:242-332,396,429:
 *                CONNECTTO dials (no +1), MAXCONNECTIONS 250, Dout = D/2,
 *                anonymize (unsigned), SELFTRIGGER, 16-byte header, log line
 *                keyed by msgId.
 * Returns GS_EINVAL for an unknown node. */
gs_status gs_config_preset(gs_config* cfg, uint32_t node);

/* Read the reference's env surface into cfg: PEERS, CONNECTTO, FRAGMENTS,
 * MUXER (env.rs:38-67), MAXCONNECTIONS (nim main.nim:429), GOSSIPSUB_D,
 * _D_LOW, _D_HIGH, _D_LAZY, _D_OUT, _HEARTBEAT_MS, _PRUNE_BACKOFF_SEC,
 * _GOSSIP_FACTOR, _FLOOD_PUBLISH (nim main.nim:252-284), SELFTRIGGER, plus
 * GS_SEED / GS_BATCH / GS_DEVICE. GS_NODE=rust|go|nim first applies that
 * node's preset (gs_config_preset). Validation mirrors env.rs:69-75:
 * unknown muxer and CONNECTTO >= PEERS are errors (message in err). */
gs_status gs_config_from_env(gs_config* cfg, char* err, size_t err_len);

/* Wire bytes of one fragment of `payload` bytes on one hop. */
uint64_t gs_wire_bytes(uint64_t payload, uint32_t muxer, uint32_t signed_msgs);

/* Stage link tables from topogen.py's parameters (shadow/topogen.py:39-71):
 * lat_ns[S*S] (row = sender stage), bw_bps[S] (up == down). */
gs_status gs_topogen_links(uint32_t stages, uint32_t min_bw_mbit, uint32_t max_bw_mbit,
                           uint32_t min_lat_ms, uint32_t max_lat_ms, uint32_t mode,
                           uint64_t* lat_ns, uint64_t* bw_bps);

/* Link tables from a Shadow network graph file (network_topology.gml as
 * shadow/topogen.py:39-71 writes it: node host_bandwidth_up/down, edge latency;
 * units bit/Kbit/Mbit/Gbit, ns/us/ms/s). Every GML node becomes one link class,
 * so V = *nodes classes: lat_ns[V*V], bw_up_bps[V], bw_down_bps[V]. mode as
 * gs_topogen_links (GS_LINKS_DIRECT needs an edge for every pair). Returns
 * GS_ERANGE with *nodes = V when V > max_nodes (call again with room), and
 * GS_EUNSUPPORTED for a non-zero packet_loss (not modelled). */
gs_status gs_links_from_gml(const char* gml_path, uint32_t mode, uint32_t max_nodes, uint32_t* nodes,
                            uint64_t* lat_ns, uint64_t* bw_up_bps, uint64_t* bw_down_bps);

/* Peer -> link class from a Shadow config (shadow.yaml as topogen.py:73-139
 * writes it): host "pod-<id>" (the id parse of rust env.rs:34-36) ->
 * network_node_id, incl. YAML anchors/aliases; hosts with id >= peers (the
 * injector) are skipped; a peer without a host is GS_EINVAL. */
gs_status gs_shadow_hosts(const char* yaml_path, uint32_t peers, uint8_t* stage_of_peer);

/* The publish injector of a Shadow config (shadow.yaml as topogen.py:125-136
 * writes it): the controller host's process `args`
 * "traffic_sync.py -s <msg_size> -m <messages> -d <delay> -n <peers> ..." and
 * its start_time. The delay is read in milliseconds, the unit shadow/run.sh:36
 * passes (topogen.py:26's help text says seconds). */
typedef struct gs_injector {
    uint64_t start_ns;    /* process start_time (500s in topogen.py:133)          */
    uint64_t delay_ns;    /* -d: inter-message delay                              */
    uint32_t msg_size;    /* -s                                                   */
    uint32_t messages;    /* -m                                                   */
    uint32_t peers;       /* -n                                                   */
    uint32_t reserved;
} gs_injector;
gs_status gs_shadow_injector(const char* yaml_path, gs_injector* out);

/* A publish schedule file: one row per message, "t_pub_ns publisher msg_size
 * [frags]" (whitespace separated, '#' comments). Returns GS_ERANGE with
 * *n = rows when cap is too small (call again with room), GS_EINVAL on a
 * malformed row. */
gs_status gs_read_schedule(const char* path, gs_publish* out, uint64_t cap, uint64_t* n);

/* Publish schedule of shadow/run.sh:34-36 (publisher_id, publisher_rotation,
 * inter_message_delay): row i = {t0 + i*delay, (pub0 + i*rotation) mod N, size}. */
gs_status gs_schedule_runsh(uint32_t n_msgs, uint32_t peers, uint32_t publisher_id,
                            uint32_t rotation, uint64_t t0_ns, uint64_t delay_ns,
                            uint32_t msg_size, gs_publish* out);

/* Write arrival lines exactly as `grep -rne 'milliseconds\|BW' shadow.data/`
 * would print them for rust nodes (main.rs:93; shadow/run.sh:61):
 *   shadow.data/hosts/peer<u>/main.1000.stdout:<line>:<tx_time> milliseconds: <ms>
 * grouped by peer in ascending id, line numbers counted per peer. */
gs_status gs_write_latency_log(const char* path, const gs_publish* sched, uint64_t n_msgs,
                               uint32_t peers, const uint64_t* t_complete_ns,
                               uint32_t self_log);

/* The same arrival log for the node flavour of cfg (peers, self_log, node,
 * seed): rust and go print "<tx_time> milliseconds: <ms>" (main.rs:93,
 * go-test-node/main.go:49); nim prints "<msgId> milliseconds: <ms>"
 * (nim gossipsub-queues/main.nim:150) with msgId a 63-bit id drawn from
 * (seed, publisher, t_pub) in place of the node's rand(high(int64)). */
gs_status gs_write_node_log(const gs_config* cfg, const char* path, const gs_publish* sched,
                            uint64_t n_msgs, const uint64_t* t_complete_ns);

/* Streaming arrival log (the same lines as gs_write_node_log) for runs too
 * large for a [n_msgs][peers] host array: feed it the message-major blocks of
 * gs_result_sink.on_block. Lines come out block by block (message-major within
 * a block) instead of grouped by peer; the per-peer line numbers count across
 * blocks exactly as the grouped writer counts them, so every line is
 * identical and the awk summaries are unchanged. */
typedef struct gs_log gs_log;
gs_status gs_log_open(const gs_config* cfg, const char* path, gs_log** out);
/* sched = the block's n_msgs schedule rows, t_complete_ns = [n_msgs][peers]. */
gs_status gs_log_write(gs_log* log, const gs_publish* sched, uint32_t n_msgs, const uint64_t* t_complete_ns);
/* The same from the u16 latency stream (gs_result_sink.on_lat, ABI 9):
 * lat_ms = [n_msgs][peers], GS_LAT_NONE where no line is written. */
gs_status gs_log_write_lat(gs_log* log, const gs_publish* sched, uint32_t n_msgs, const uint16_t* lat_ms);
gs_status gs_log_close(gs_log* log);

/* Packets and header bytes of one fragment send in the same model as
 * gs_wire_bytes: TCP/IPv4 segments of <= 1460 B carrying 40 B of headers each,
 * or QUIC packets of <= 1415 B carrying 65 B each. */
void gs_wire_packets(uint64_t payload, uint32_t muxer, uint32_t signed_msgs, uint64_t* packets,
                     uint64_t* header_bytes);

/* Wire size of one lazy-gossip control RPC carrying one message id (IHAVE:
 * RPC{control{ihave{topic "test", id}}}, IWANT: RPC{control{iwant{id}}}; the
 * id is 20 bytes for the rust / nim nodes' decimal hashes, 32 for go's sha256)
 * through the muxer stack, or one pure ACK packet (header only). */
enum { GS_CTRL_IHAVE = 0, GS_CTRL_IWANT = 1, GS_CTRL_ACK = 2 };
void gs_control_packets(uint32_t kind, uint32_t node, uint32_t muxer, uint64_t* bytes, uint64_t* packets,
                        uint64_t* header_bytes);

/* Columns of a per-peer traffic row (gs_get_traffic). Data columns count every
 * packet that carries bytes of a gossipsub RPC (message sends, IWANT answers,
 * IHAVE and IWANT control RPCs); the ctrl columns count the pure TCP/QUIC ACKs
 * (one per <= 2 data packets received, sent back to the sender). */
enum { GS_TR_TX_BYTES = 0, GS_TR_RX_BYTES = 1, GS_TR_TX_PKTS = 2, GS_TR_RX_PKTS = 3,
       GS_TR_TX_HDR = 4, GS_TR_RX_HDR = 5,
       GS_TR_RECEIVED = 6,   /* completed messages (main.rs:94 inc_received_message)   */
       GS_TR_PUBLISHED = 7,  /* messages published (main.rs:515 inc_messages_published) */
       GS_TR_TX_CTRL_PKTS = 8, GS_TR_RX_CTRL_PKTS = 9,  /* pure ACK packets            */
       GS_TR_TX_CTRL_HDR = 10, GS_TR_RX_CTRL_HDR = 11,  /* their (header-only) bytes    */
       GS_TRAFFIC_COLS = 12 };

/* Shadow's per-host heartbeat counters for the same runs, one "[node]" line
 * per peer as Shadow's tracker logs them (recv/send bytes, then inbound and
 * outbound localhost / remote packet, header and payload counters), so that
 * shadow/summary_shadowlog.awk:12-143 summarises them unchanged. traffic is
 * [peers][GS_TRAFFIC_COLS]. Host names are pod-<id> (topogen.py:118). */
gs_status gs_write_shadow_heartbeat(const char* path, uint32_t peers, const uint64_t* traffic,
                                    uint64_t sim_seconds);

/* The test node's Prometheus metrics (rust-test-node/src/metrics.rs:13-199,
 * names shared with the go and nim nodes) for every peer, in the OpenMetrics
 * text format prometheus-client encodes (counters with _total, "# EOF"), one
 * series per peer labelled peer="pod-<id>": connected / pubsub peers and
 * subscriptions = CSR degree, topics = 1, mesh peers = mesh_count, topic
 * health buckets against cfg->d_lo (metrics.rs:158-176), received / validated
 * and published messages from the traffic columns. Arrays are host copies:
 * row_ptr[peers+1] (gs_get_csr), mesh_count[peers] (gs_get_mesh),
 * traffic[peers][GS_TRAFFIC_COLS] (gs_get_traffic). */
gs_status gs_write_node_metrics(const gs_config* cfg, const char* path, const uint64_t* row_ptr,
                                const uint8_t* mesh_count, const uint64_t* traffic);

/* ---- context lifecycle (replaces SwarmBuilder + build_behaviour, main.rs:391-440) ---- */

gs_status gs_create(const gs_config* cfg, struct gs_ctx** out);
gs_status gs_destroy(struct gs_ctx* ctx);

/* Checkpoint / resume (no counterpart in the reference, whose
 * runs are single Shadow executions): gs_save_state writes the configuration,
 * link tables, CSR + mesh flags + PRUNE back-offs, the mesh ELL, the churn
 * mesh state's epoch, the counters and the per-peer traffic of a context to
 * `path`; gs_load_state makes a new context on `device` from such a file. A
 * schedule continued on the loaded context gives exactly the results and
 * counters the saved context would have given (every random draw is a pure
 * function of the seed: there is no generator state). GS_EINVAL for a file of
 * another ABI version or a damaged one. */
gs_status gs_save_state(struct gs_ctx* ctx, const char* path);
gs_status gs_load_state(const char* path, int32_t device, struct gs_ctx** out);
/* The configuration a context was created (or loaded) with. */
gs_status gs_get_config(const struct gs_ctx* ctx, gs_config* out);
const char* gs_last_error(const struct gs_ctx* ctx);

/* Per-stage link model. lat_ns is S x S (sender stage row), bw arrays have S
 * entries in bit/s; stage_of_peer has `peers` entries or is NULL (= u % S,
 * topogen.py:121-122). */
gs_status gs_set_links(struct gs_ctx* ctx, uint32_t stages, const uint64_t* lat_ns,
                       const uint64_t* bw_up_bps, const uint64_t* bw_down_bps,
                       const uint8_t* stage_of_peer);

/* Random ID dialing -> symmetric CSR peer graph, on the device
 * (replaces connect_gossipsub_peers, main.rs:303-389). */
gs_status gs_build_topology(struct gs_ctx* ctx);

/* A caller's graph in place of the built one: either call stands
 * where gs_build_topology stands and may be repeated at any time; a converge must
 * follow before the next run. connect_to, dial_extra and max_connections play no
 * part. A refused graph (GS_EINVAL for a defect, GS_EUNSUPPORTED for a peer with
 * more than 256 connections or >= 2^32 entries) leaves the context as it was;
 * gs_last_error names the kind of defect and the smallest entry, dial or peer index
 * that has it.
 * gs_set_topology: the graph in gs_get_csr's layout, rows ascending by id; of flags
 * only bit 0 ("the row's peer dialed col") is read. Every entry needs its reverse,
 * every connection bit 0 on at least one end, every peer a connection. */
gs_status gs_set_topology(struct gs_ctx* ctx, const uint64_t* row_ptr /*[peers+1]*/,
                          const uint32_t* col, const uint8_t* flags);
/* gs_set_topology_dials: the undirected union of the accepted dials dialer[i] ->
 * target[i] (the "dialing" log lines, main.rs:340-348), in any order: the graph is a
 * function of the set. u -> w and w -> u together are a mutual dial; the same
 * ordered pair twice, dialer == target and a peer in no dial are defects. */
gs_status gs_set_topology_dials(struct gs_ctx* ctx, uint64_t n_dials,
                                const uint32_t* dialer, const uint32_t* target);
/* Host only. A dial list as text: one "dialer target" pair per line, '#' comments
 * and blank lines as gs_read_schedule, and its cap contract (GS_ERANGE with
 * *n = rows when cap is too small; dialer and target may then be NULL). */
gs_status gs_read_dials(const char* path, uint32_t* dialer, uint32_t* target, uint64_t cap, uint64_t* n);
/* One line per entry with bit 0 set, in row order. */
gs_status gs_write_dials(const char* path, uint32_t peers, const uint64_t* row_ptr,
                         const uint32_t* col, const uint8_t* flags);

/* Graph size after gs_build_topology or an import. */
gs_status gs_graph_info(const struct gs_ctx* ctx, uint32_t* peers, uint64_t* nnz,
                        uint32_t* max_degree);

/* Copy the CSR out: row_ptr[peers+1], col[nnz], flags[nnz] (bit0 = outbound,
 * bit1 = in mesh). Any pointer may be NULL. */
gs_status gs_get_csr(struct gs_ctx* ctx, uint64_t* row_ptr, uint32_t* col, uint8_t* flags);

/* Heartbeat GRAFT/PRUNE to a fixed point or max_heartbeats epochs
 * (libp2p-gossipsub heartbeat, configured at main.rs:228-236). With churn
 * there is no fixed point: exactly max_heartbeats epochs run, and gs_run then
 * advances the mesh to the epochs its schedule needs. */
gs_status gs_mesh_converge(struct gs_ctx* ctx, uint32_t max_heartbeats, uint32_t* out_epochs);

/* Mesh width of gs_get_mesh rows. */
#define GS_MESH_W 16u
/* Copy the mesh out: mesh[peers*GS_MESH_W] (ascending ids, UINT32_MAX padding),
 * count[peers]. Either pointer may be NULL. */
gs_status gs_get_mesh(struct gs_ctx* ctx, uint32_t* mesh, uint8_t* count);

/* A caller's mesh in place of the converged one (DESIGN.md §2.3 "A caller's mesh"):
 * the mesh a real run ended up with (a tracer's Graft / Prune events,
 * go-test-node/metrics.go:328-340), or any what-if mesh, the empty one included. Either
 * call stands where gs_mesh_converge stands: it needs the topology and the links
 * (GS_ESTATE), leaves what a converge would leave (the mesh bit of gs_get_csr's flags
 * on exactly these links, rows ascending, no back-offs), and is undone by whatever
 * undoes a converged mesh; a later gs_mesh_converge starts from the empty mesh as
 * always. The mesh is a function of the set of links: no order of rows' slots or of the
 * list shows in it. GS_EUNSUPPORTED when churn_ppm != 0 (every epoch's mesh then
 * comes from the chain, which starts at epoch 0). A refused mesh (GS_EINVAL for a
 * defect, GS_ERANGE for a row wider than GS_MESH_W) leaves the context as it was;
 * gs_last_error names the kind of defect and the smallest slot, link, peer or CSR
 * entry that has it. The mesh events of gs_set_mesh_events describe a converge:
 * their getters return GS_ESTATE until the next one. Partitioned runs need the
 * import in every context or in none (GS_EINVAL before any batch otherwise).
 * gs_set_mesh: gs_get_mesh's layout, mesh[peers*GS_MESH_W] of plain ids in any order
 * inside a row; a row is its first count[u] slots, or with count == NULL ends at its
 * first UINT32_MAX. Every link needs its reverse in the other peer's row. */
gs_status gs_set_mesh(struct gs_ctx* ctx, const uint32_t* mesh, const uint8_t* count);
/* gs_set_mesh_links: the undirected links {a[i], b[i]}, in any order and either
 * orientation, each once. n_links == 0 is the empty mesh (flood publishing plus
 * gossip only). */
gs_status gs_set_mesh_links(struct gs_ctx* ctx, uint64_t n_links, const uint32_t* a, const uint32_t* b);
/* Host only. One "a b" line per link with a < b, in row order: the text form of
 * gs_write_dials, read back by gs_read_dials. count may be NULL as for gs_set_mesh. */
gs_status gs_write_mesh_links(const char* path, uint32_t peers, const uint32_t* mesh, const uint8_t* count);

/* A caller's outages in place of the churn draw (DESIGN.md §2.8 "A caller's outages"): who
 * is offline when, as intervals (peer[i], h_from[i], h_to[i]) in heartbeat epochs. The peer
 * is offline during the epochs h_from <= h < h_to; h_to == GS_OUTAGE_FOREVER: it never
 * returns. Epoch 0 has nobody offline (h_from >= 1). The schedule is a function of the set
 * of intervals: the list's order shows in nothing. Intervals of one peer may touch (their
 * union) but not share an epoch. n == 0 is the empty schedule: a churn context in which
 * nobody ever leaves. churn_ppm != 0 remains what makes a context a churn context
 * (GS_ESTATE otherwise); while a schedule is imported, its value and churn_down are not
 * read, churn_horizon applies as before.
 * gs_set_outages stands before gs_mesh_converge and may be repeated at any time: an accepted
 * schedule un-builds the mesh (a converge must follow; a run before it returns GS_ESTATE),
 * restarts the epoch chain and the ring, and leaves the mesh-event getters at GS_ESTATE until
 * that converge. A refused one (GS_EINVAL for peer >= peers, h_from == 0, h_from >= h_to or
 * two intervals of one peer that share an epoch; GS_EUNSUPPORTED for n >= 2^32 or more than
 * GS_OUTAGE_ROW_MAX intervals of one peer) leaves the context as it was; gs_last_error names
 * the kind of defect and the smallest interval (or peer) index that has it.
 * gs_clear_outages returns to the draw, with the same invalidation; without an import it
 * does nothing and returns GS_OK.
 * gs_save_state returns GS_EUNSUPPORTED while a schedule is imported (the file does not
 * carry it). Partitioned runs need the same schedule in every context, or none (GS_EINVAL
 * before any batch otherwise). */
#define GS_OUTAGE_FOREVER 0xFFFFFFFFu
#define GS_OUTAGE_ROW_MAX 256u
gs_status gs_set_outages(struct gs_ctx* ctx, uint64_t n, const uint32_t* peer,
                         const uint32_t* h_from, const uint32_t* h_to);
gs_status gs_clear_outages(struct gs_ctx* ctx);
/* The offline bitsets of epochs [h_lo, h_hi] from whichever source is active, the draw or
 * the imported schedule, written by the kernel that feeds the epoch chain:
 * bits[(h_hi - h_lo + 1)][(peers + 63) / 64], bit u % 64 of word u / 64 = peer u is offline.
 * Bits at and past `peers` are 0, and epoch 0 is all 0. GS_ESTATE when churn_ppm == 0,
 * GS_EINVAL when h_hi < h_lo. */
gs_status gs_get_offline(struct gs_ctx* ctx, uint32_t h_lo, uint32_t h_hi, uint64_t* bits);
/* Host only. The times of a trace as epochs: a peer is offline in epoch h >= 1 iff it is
 * down at the heartbeat that starts the epoch, t_down <= hb_phase + h * heartbeat < t_up
 * (cfg's heartbeat_ns and hb_phase_ns; the rule is build-defined, as churn is). So
 * h_from = max(1, ceil((t_down - hb_phase) / heartbeat)), 1 when t_down <= hb_phase, and
 * h_to = ceil((t_up - hb_phase) / heartbeat), GS_OUTAGE_FOREVER when t_up == UINT64_MAX.
 * An outage that covers no heartbeat is left out; *n_out counts the ones kept, in input
 * order (the output arrays hold n entries and may be the input's). Outages of one peer that
 * are disjoint in time can touch in epochs but never overlap. GS_EINVAL for t_up < t_down,
 * GS_ERANGE for an epoch past 2^32 - 2. */
gs_status gs_outage_epochs(const gs_config* cfg, uint64_t n, const uint32_t* peer,
                           const uint64_t* t_down_ns, const uint64_t* t_up_ns,
                           uint32_t* peer_out, uint32_t* h_from, uint32_t* h_to, uint64_t* n_out);
/* Host only. An outage list as text: one "peer t_down_ns [t_up_ns]" line per outage, a
 * missing third column meaning the peer never returns (t_up = UINT64_MAX); '#' comments,
 * blank lines and the cap contract as gs_read_dials. A malformed line is GS_EINVAL with
 * *n = the number of that line, counted from 1 (0: the file cannot be opened). */
gs_status gs_read_outages(const char* path, uint32_t* peer, uint64_t* t_down_ns,
                          uint64_t* t_up_ns, uint64_t cap, uint64_t* n);

/* Simulate n_msgs publishes (replaces publish_new_message + the receive /
 * forward / reassembly loop, main.rs:79-143,519-528). Results go to `sink`
 * (may be NULL: device-resident run, counters only). */
gs_status gs_run(struct gs_ctx* ctx, const gs_publish* sched, uint64_t n_msgs,
                 const gs_result_sink* sink);

/* Device-formatted arrival log: `text` holds `bytes` bytes = `lines` whole lines of the
 * messages [first_msg, first_msg + n_msgs), valid only during the call. The concatenation
 * of all calls of a run, in call order, is byte for byte what gs_log_write_lat writes for
 * the same run's on_lat stream (gs_log_open on a context-fresh counter state). */
typedef void (*gs_text_fn)(void* user, uint64_t first_msg, uint32_t n_msgs,
                           const char* text, uint64_t bytes, uint64_t lines);

/* gs_run whose only output is the log text (replaces the println! of main.rs:93 and the
 * grep of shadow/run.sh:61 at once). chunk_bytes: text bytes per callback at most
 * (0 = default, 256 MB; raised to one message's bound, peers x the longest line). The
 * callback of one chunk runs while the next is formatted and copied. Counters in
 * gs_stats as gs_run. GS_ERANGE: a latency of 65535 ms or more (before any text of that
 * batch is handed out), or a peer's line counter passing 2^32 - 1. */
gs_status gs_run_log(struct gs_ctx*, const gs_publish* sched, uint64_t n_msgs,
                     gs_text_fn on_text, void* user, uint64_t chunk_bytes);

/* The same formatter over a caller's u16 array lat_ms[n_msgs][peers] (an archived on_lat
 * stream): needs only gs_create, no graph. */
gs_status gs_format_lat_log(struct gs_ctx*, const gs_publish* sched, uint64_t n_msgs,
                            const uint16_t* lat_ms, gs_text_fn on_text, void* user,
                            uint64_t chunk_bytes);

/* Per-peer line counters: zero at gs_create, carried across gs_run_log / gs_format_lat_log /
 * gs_run_partitioned_log calls (as one gs_log carries them across gs_log_write_lat calls);
 * this zeroes them. They are per context and cover the context's own peers — all of them, or
 * the range of its partition — and are also zeroed when the context's partition
 * (parts, part) changes (gs_set_partition, gs_run_partitioned with another communicator
 * size). After a failed call they are unspecified until this call. */
gs_status gs_log_text_reset(struct gs_ctx*);

/* Host-only: the longest line cfg can produce, in bytes (sizes the buffers). */
uint32_t gs_log_line_max(const gs_config* cfg);

gs_status gs_get_stats(const struct gs_ctx* ctx, gs_stats* out);
gs_status gs_reset_stats(struct gs_ctx* ctx);

/* 1: record HIP events around every relaxation launch and around gs_run. */
gs_status gs_set_timing(struct gs_ctx* ctx, uint32_t enable);

/* 1: account every send of gs_run per peer (the counters Shadow's tracker
 * keeps per host, summary_shadowlog.awk): flood-publish and forward sends of a
 * fragment, lazy gossip's IHAVE and IWANT RPCs and IWANT answers, each to the
 * sender's tx and — unless lost to churn (receiver offline or the message's
 * lifetime over at the arrival) — the receiver's rx columns, plus the ACKs the
 * receiver returns. Counted after each batch from the final keys (extra passes
 * over them), so it is off by default. Enabling zeroes the counters, as does
 * gs_reset_stats. */
gs_status gs_set_traffic(struct gs_ctx* ctx, uint32_t enable);
/* Copy the per-peer counters out: traffic[peers][GS_TRAFFIC_COLS]. */
gs_status gs_get_traffic(struct gs_ctx* ctx, uint64_t* traffic);

/* ---- per-peer pubsub event counts --------------------------
 * What go-test-node/metrics.go:84-220 counts per node, and the nim node's
 * dst_testnode_received_chunks_total (main.nim:37-41). The events are exactly
 * the sends, arrivals and losses gs_set_traffic accounts;
 * here each is counted, not weighed in bytes. A "message" is one fragment copy. */
enum { GS_PS_MSG_TX = 0,    /* fragment copies sent: flood-publish, forwards (after IDONTWANT  */
                            /* skips), IWANT answers; sends lost to churn included             */
       GS_PS_MSG_RX = 1,    /* copies that arrived (a lost send is not counted, as for rx traffic) */
       GS_PS_FIRST = 2,     /* first receipts of a fragment at a non-publisher                 */
       GS_PS_DUP = 3,       /* duplicates: MSG_RX - FIRST                                      */
       GS_PS_IHAVE_TX = 4, GS_PS_IHAVE_RX = 5,  /* IHAVE RPCs sent / arrived                   */
       GS_PS_IWANT_TX = 6, GS_PS_IWANT_RX = 7,  /* IWANT RPCs sent / arrived                   */
       GS_PUBSUB_COLS = 8 };
/* 1: every batch of gs_run and gs_run_log adds its events to per-peer counters
 * on the device (extra passes over the final keys, as gs_set_traffic: off by
 * default, diagnostic). Enabling allocates and zeroes the counters; they carry
 * across batches and calls and are zeroed by gs_reset_pubsub_counts and
 * gs_reset_stats. IDONTWANT, GRAFT, PRUNE and subscription RPCs are not
 * counted. Partitioned mode (gs_part_begin, gs_run_partitioned*) returns
 * GS_EUNSUPPORTED while the switch is on. gs_save_state does not carry the
 * counters: a loaded context has the switch off. */
gs_status gs_set_pubsub_counts(struct gs_ctx* ctx, uint32_t enable);
/* out[peers][GS_PUBSUB_COLS]. GS_ESTATE while the switch is off. */
gs_status gs_get_pubsub_counts(struct gs_ctx* ctx, uint64_t* out);
gs_status gs_reset_pubsub_counts(struct gs_ctx* ctx);

/* The go node's pubsub counters (go-test-node/metrics.go:84-220, help strings
 * verbatim) and the nim node's chunk counter for every peer, in the Prometheus
 * text exposition format ("# HELP" / "# TYPE" per family), one series per peer
 * labelled peer_id="pod-<id>", with topic="test" first where metrics.go has a
 * topic label: libp2p_pubsub_broadcast_messages_total (MSG_TX),
 * libp2p_pubsub_received_messages_total (MSG_RX),
 * libp2p_pubsub_broadcast_ihave_total, libp2p_pubsub_received_ihave_total,
 * libp2p_pubsub_broadcast_iwant_total, libp2p_pubsub_received_iwant_total,
 * libp2p_gossipsub_received_total (FIRST), libp2p_gossipsub_duplicate_total
 * (DUP) and dst_testnode_received_chunks_total (FIRST; labels muxer, peer_id as
 * main.nim:40). counts[peers][GS_PUBSUB_COLS] is a host copy
 * (gs_get_pubsub_counts). Host only. */
gs_status gs_write_pubsub_metrics(const gs_config* cfg, const char* path, uint32_t peers, const uint64_t* counts);

/* ---- per-link first-delivery counts -------------------------
 * Of the fragments a peer received first, how many came over each of its
 * connections: the per-link question of the one scoring term all three nodes
 * configure, first-message-deliveries P2 (rust-test-node/src/main.rs:252-258,
 * go-test-node/main.go:186-193, nim-test-node/gossipsub-queues/main.nim:335-340).
 * The sender is the src field of the final key. A first receipt
 * is GS_PS_FIRST's: a fragment's first arrival at a non-publisher. */
enum { GS_LD_PUBLISH = 0,   /* the sender is the message's publisher (with or without flood-publish) */
       GS_LD_MESH = 1,      /* the sender is in the receiver's row of the frozen mesh               */
       GS_LD_GOSSIP = 2,    /* neither: an IWANT answer                            */
       GS_LD_COLS = 3 };
/* 1: every finished batch of gs_run and gs_run_log adds its first receipts to
 * per-link counters on the device, [nnz][GS_LD_COLS] aligned with gs_get_csr's
 * arrays: entry e in the row of peer u counts the fragments u received first
 * from col[e]; a peer's row over the three columns sums to its GS_PS_FIRST. One
 * extra pass over the final keys (off by default, diagnostic). Enabling zeroes
 * the counters; it may come before a graph exists (they are allocated when first
 * needed). They carry across batches and calls and are zeroed by
 * gs_reset_link_deliveries, gs_reset_stats, and a graph built or imported
 * (gs_build_topology, gs_set_topology, gs_set_topology_dials: the entries then
 * mean other links). GS_EUNSUPPORTED on a context with churn_ppm > 0 (the mesh
 * of a send and of its arrival can differ). Partitioned mode (gs_part_begin,
 * gs_run_partitioned*) returns GS_EUNSUPPORTED while the switch is on.
 * gs_save_state does not carry the counters: a loaded context has the switch
 * off. */
gs_status gs_set_link_deliveries(struct gs_ctx* ctx, uint32_t enable);
/* out[nnz][GS_LD_COLS]. GS_ESTATE while the switch is off or no graph exists. */
gs_status gs_get_link_deliveries(struct gs_ctx* ctx, uint64_t* out);
/* out[peers][GS_LD_COLS]: the first deliveries each peer made as the sender, the
 * transposed sum of the link counters (what P2 rewards), derived on the device
 * at read-out. GS_ESTATE as gs_get_link_deliveries. */
gs_status gs_get_peer_given(struct gs_ctx* ctx, uint64_t* out);
gs_status gs_reset_link_deliveries(struct gs_ctx* ctx);
/* Host only. One line "receiver sender publish mesh gossip" (plain integers) per
 * CSR entry with a non-zero count, in CSR order; row_ptr[peers+1], col[nnz] and
 * counts[nnz][GS_LD_COLS] are host copies (gs_get_csr, gs_get_link_deliveries). */
gs_status gs_write_link_deliveries(const char* path, uint32_t peers, const uint64_t* row_ptr, const uint32_t* col,
                                   const uint64_t* counts);

/* ---- per-message cost table --------------------------------
 * What each message of one gs_run / gs_run_log call cost: the sends, arrivals
 * and losses the per-peer traffic and pubsub counts enumerate, reduced by
 * message instead of by peer. A schedule that sweeps message size or chunk count
 * (gs_publish.frags) gets every message's cost from one call. */
enum { GS_MC_DATA_TX = 0,   /* fragment copies sent: the publisher's sends, forwards and IWANT    */
                            /* answers; duplicates and lost copies included                       */
       GS_MC_DATA_RX = 1,   /* copies that arrived                                                */
       GS_MC_FIRST = 2,     /* first receipts of a fragment at a non-publisher                    */
       GS_MC_DUP = 3,       /* duplicates: DATA_RX - FIRST                                        */
       GS_MC_IHAVE_TX = 4, GS_MC_IHAVE_RX = 5,  /* IHAVE RPCs sent / arrived                      */
       GS_MC_IWANT = 6,     /* IWANT RPCs (always delivered: sent equals arrived)                 */
       GS_MC_DELIVERED = 7, /* completions at non-publishers (every fragment received)            */
       GS_MC_COLS = 8 };
/* 1: every gs_run and gs_run_log call fills a table on the device with one row
 * per message of its schedule, in schedule order (whatever batches the run cuts
 * or regroups). The table belongs to the most recent call: it is zeroed at the
 * call's start, does not accumulate, and gs_reset_stats leaves it alone. One
 * extra pass over each batch's final keys (off by default, diagnostic). Enabling
 * (again) empties the table. Partitioned mode (gs_part_begin,
 * gs_run_partitioned*) returns GS_EUNSUPPORTED while the switch is on.
 * gs_save_state does not carry the table: a loaded context has the switch off. */
gs_status gs_set_message_costs(struct gs_ctx* ctx, uint32_t enable);
/* The table's rows: the messages of the last call; 0 before any run and after
 * the switch is enabled. GS_ESTATE while the switch is off. */
gs_status gs_message_costs_rows(struct gs_ctx* ctx, uint64_t* rows);
/* out[rows][GS_MC_COLS]. GS_ESTATE while the switch is off; GS_EINVAL when rows
 * is not gs_message_costs_rows' count. */
gs_status gs_get_message_costs(struct gs_ctx* ctx, uint64_t* out, uint64_t rows);
/* Host only. One TSV line per message under a '#' header line: its index, the
 * schedule fields (t_pub_ns, publisher, msg_size, chunks), the GS_MC_COLS counts,
 * and the wire cost derived from them with gs_wire_bytes, gs_wire_packets and
 * gs_control_packets: tx and rx bytes and packets (fragment copies, IHAVEs and
 * IWANTs), the pure ACK packets (ceil(packets / 2) per arrival) and their bytes.
 * costs[n_msgs][GS_MC_COLS] is a host copy (gs_get_message_costs). GS_EINVAL: a
 * null argument, a message no node can publish (its fragment too short), a path
 * that cannot be written. */
gs_status gs_write_message_costs(const gs_config* cfg, const char* path, const gs_publish* sched, uint64_t n_msgs,
                                 const uint64_t* costs);

/* ---- mesh events and per-epoch mesh health -----------------
 * What go-test-node/metrics.go:164-190 counts per node (GRAFT and PRUNE RPCs
 * sent and received) and what its tracer follows (metrics.go:224-258 mesh size,
 * Graft / Prune; 328-362 topic health), for the epochs one gs_mesh_converge call
 * steps. The rules are those of DESIGN.md §2.3 (steps A, B, C) and the
 * disconnect of §2.8. An entry e = (u -> w) is a CSR entry of row u. */
enum { GS_ME_GRAFT_TX = 0,  /* entries of u that carry a GRAFT after step A (subscription grafts, */
                            /* the D - m grafts, the outbound grafts)                            */
       GS_ME_GRAFT_RX = 1,  /* neighbours' GRAFTs that target u (the ones step B handles)        */
       GS_ME_PRUNE_TX = 2,  /* u's step-A PRUNEs + the GRAFTs u rejects in B (the PRUNE reply:   */
                            /* back-off not over, or at D_hi and the grafter not dialed by u)    */
       GS_ME_PRUNE_RX = 3,  /* neighbours' step-A PRUNEs of u + u's own GRAFTs that were rejected */
       GS_ME_MESH_ADD = 4,  /* entries of u outside the mesh after the epoch's disconnect and in */
                            /* it after C (both ends of a new link count their own entry)        */
       GS_ME_MESH_DEL = 5,  /* entries of u in the mesh after the disconnect and out of it after */
                            /* C: a PRUNE sent or received (entries, not RPCs)                   */
       GS_ME_MESH_DROP = 6, /* entries of u in the mesh at the start of the epoch whose either   */
                            /* end is offline in it (§2.8: no PRUNE, no back-off; an offline     */
                            /* peer counts its own entries too)                                  */
       GS_MESH_EVENT_COLS = 7 };
/* One series row per epoch h = 0..out_epochs, the state after step C. */
enum { GS_MS_ONLINE = 0,    /* peers online in epoch h                                           */
       GS_MS_NO_PEERS = 1,  /* online peers with mesh size 0                                     */
       GS_MS_LOW = 2,       /* online peers with 0 < m < D_lo                                    */
       GS_MS_HEALTHY = 3,   /* online peers with m >= D_lo (the three classes: metrics.go:348-362) */
       GS_MS_OVER = 4,      /* online peers with m > D_hi (a subset of HEALTHY)                  */
       GS_MS_LINKS = 5,     /* sum of m over all peers                                           */
       GS_MS_GRAFTS = 6,    /* GRAFT proposals in the epoch                                      */
       GS_MS_REJECTS = 7,   /* GRAFTs rejected in B                                              */
       GS_MS_PRUNES = 8,    /* step-A PRUNEs                                                     */
       GS_MS_DROPS = 9,     /* entries dropped by the disconnect                                 */
       GS_MS_ADDS = 10,     /* entries that entered the mesh                                     */
       GS_MS_DELS = 11,     /* entries that left it by PRUNE                                     */
       GS_MESH_SERIES_COLS = 12 };
/* 1: gs_mesh_converge records both results for the epochs it steps from the
 * empty mesh: epoch 0 (the subscription exchange; empty when sub_graft is 0)
 * and heartbeats 1..out_epochs (frozen mesh: up to the fixed point, with its
 * exact jumps over quiescent epochs; churn: exactly max_heartbeats). One more
 * row kernel per stepped epoch; off by default, diagnostic. Every converge call
 * zeroes and refills both, so they describe the last call, for all peers
 * whatever partition the context holds (the mesh is replicated). The epochs
 * gs_run's churn chain steps or replays later are NOT counted (it replays from
 * epoch 0 and may drop a run it stepped ahead): converge to the horizon you
 * want to read. Enabling allocates. gs_save_state does not carry the results:
 * a loaded context has the switch off. */
gs_status gs_set_mesh_events(struct gs_ctx* ctx, uint32_t enable);
/* out[peers][GS_MESH_EVENT_COLS]. GS_ESTATE while the switch is off or before a
 * converge ran since it went on (the two calls below as well). */
gs_status gs_get_mesh_events(struct gs_ctx* ctx, uint64_t* out);
/* *rows = out_epochs + 1 of the last converge. */
gs_status gs_mesh_series_rows(struct gs_ctx* ctx, uint32_t* rows);
/* out[rows][GS_MESH_SERIES_COLS]; GS_EINVAL unless rows is gs_mesh_series_rows'.
 * An epoch the frozen-mesh jump skipped has no events and the previous row's
 * gauges; with sub_graft = 0 row 0 is the empty mesh (ONLINE = NO_PEERS = peers). */
gs_status gs_get_mesh_series(struct gs_ctx* ctx, uint64_t* out, uint32_t rows);

/* The go node's GRAFT / PRUNE / subscription counters and mesh gauges
 * (go-test-node/metrics.go:164-190 and 224-258, 328-362; help strings verbatim)
 * for every peer in the Prometheus text exposition format, as
 * gs_write_pubsub_metrics: libp2p_pubsub_broadcast_graft_total (GS_ME_GRAFT_TX),
 * libp2p_pubsub_received_graft_total, libp2p_pubsub_broadcast_prune_total,
 * libp2p_pubsub_received_prune_total, libp2p_pubsub_broadcast_subscriptions_total
 * and libp2p_pubsub_received_subscriptions_total (both the CSR degree),
 * libp2p_gossipsub_peers_per_topic_mesh (gauge, mesh_count),
 * libp2p_gossipsub_low_peers_topics, libp2p_gossipsub_healthy_peers_topics and
 * libp2p_gossipsub_no_peers_topics (gauges, 0 or 1 per peer against cfg->d_lo).
 * row_ptr[peers + 1] (gs_get_csr), mesh_count[peers] (gs_get_mesh) and
 * events[peers][GS_MESH_EVENT_COLS] (gs_get_mesh_events) are host copies. Host only. */
gs_status gs_write_mesh_metrics(const gs_config* cfg, const char* path, uint32_t peers, const uint64_t* row_ptr,
                                const uint8_t* mesh_count, const uint64_t* events);
/* series[rows][GS_MESH_SERIES_COLS] (gs_get_mesh_series) as CSV: the header line
 * epoch,online,no_peers,low,healthy,over,links,grafts,rejects,prunes,drops,adds,dels
 * and one line per row. Host only. */
gs_status gs_write_mesh_series(const char* path, const uint64_t* series, uint32_t rows);

/* ---- what each node shows about delay ---------------------
 * The per-peer application metrics of nim-test-node/gossipsub-queues
 * (main.nim:25-78,147-154), reduced on the device from the logged latencies
 * every completion path produces. An observation is exactly an arrival-log
 * line: a (peer, message) pair that is delivered, the publisher's own row only
 * with cfg.self_log (then at delay 0). The delay is the logged ms
 * ((t_complete - tx_time) / 1e6 truncated). */
#define GS_DELAY_BUCKETS 12u   /* le = 1,5,10,25,50,100,250,500,1000,2500,5000,10000 ms (main.nim:59) */
typedef struct gs_peer_delay {
    uint64_t completed;      /* observations = log lines of this peer (main.nim:151)              */
    uint64_t delay_sum_ms;   /* main.nim:152                                                      */
    uint64_t last_rx_ns;     /* t_pub_ns + last_ms * 1e6 of the last observation; 0 if none       */
    uint32_t last_ms;        /* main.nim:154                                                      */
    uint32_t reserved;       /* 0                                                                 */
    uint64_t bucket[GS_DELAY_BUCKETS + 1]; /* NOT cumulative: bucket[i] counts bound[i-1] < ms <= bound[i], */
                                           /* bucket[0] ms <= 1 (0 included), bucket[12] ms > 10000         */
} gs_peer_delay;

/* 1: every batch of gs_run, gs_run_log, gs_run_partitioned and
 * gs_run_partitioned_log adds its observations to per-peer accumulators on the
 * device, whatever the sink asks for and with a NULL sink (the completion then
 * writes the logged latencies, so no batch runs without its log). Off by
 * default; enabling allocates and zeroes the accumulators. They cover the
 * context's own rows — all peers, or the range of its partition — carry across
 * batches and calls, and are zeroed by gs_reset_peer_delay, by enabling, and
 * when the context's partition (parts, part) changes. After a failed run call
 * they are unspecified until gs_reset_peer_delay.
 * "Last" is the observation that maximises (t_pub_ns + ms * 1e6, t_pub_ns): it
 * depends on no processing order, and orders completions at ms grain (the node
 * orders them by wall clock: two completions at one peer less than 1 ms apart
 * may swap).
 * While the switch is on, a logged latency of 65535 ms or more fails the run
 * call with GS_ERANGE, as for every consumer of the u16 latencies.
 * Partitioned mode: gs_part_begin (the caller-driven protocol) returns
 * GS_EUNSUPPORTED while the switch is on, and so does gs_run on a context that
 * holds one of several parts (as gs_run_log); all contexts (and ranks) of a
 * gs_run_partitioned* call must agree on it (GS_EINVAL).
 * gs_save_state does not carry the accumulators: a loaded context has the
 * switch off. */
gs_status gs_set_peer_delay(struct gs_ctx*, uint32_t enable);
/* out[own rows]. GS_ESTATE while the switch is off. */
gs_status gs_get_peer_delay(struct gs_ctx*, gs_peer_delay* out);
gs_status gs_reset_peer_delay(struct gs_ctx*);
/* Add a caller's archived on_lat stream lat_ms[n_msgs][own rows] (GS_LAT_NONE
 * where no line is logged): needs only gs_create and the switch, no graph. The
 * stream is uploaded in pieces of at most cfg.batch messages. */
gs_status gs_peer_delay_add_lat(struct gs_ctx*, const gs_publish* sched, uint64_t n_msgs, const uint16_t* lat_ms);

/* The nim node's Prometheus metrics (nim-test-node/gossipsub-queues
 * main.nim:25-78, help strings verbatim) for every peer, in the text exposition
 * format ("# HELP" / "# TYPE" per family), one series per peer labelled
 * muxer="yamux|quic|mplex", peer_id="pod-<id>" (the node prints its libp2p
 * PeerId, which cannot be derived; pod-<id> matches gs_write_node_metrics):
 * dst_testnode_publish_requests_total (counted from sched),
 * dst_testnode_publish_failures_total (0), dst_testnode_completed_messages_total,
 * dst_testnode_message_delay_ms_sum, the histogram dst_testnode_message_delay_ms
 * (cumulative _bucket{le=...}, _sum, _count), dst_testnode_last_message_delay_ms,
 * dst_testnode_mesh_size (mesh_count) and dst_testnode_topic_peers (CSR degree).
 * dst_testnode_received_chunks_total is not written here: it counts fragment
 * first arrivals, which completion does not keep per peer
 * (gs_write_pubsub_metrics writes it from the event counters). Arrays are host copies:
 * row_ptr[peers+1], mesh_count[peers], delay[peers] (gs_get_peer_delay; the
 * parts' arrays side by side). Host only. */
gs_status gs_write_testnode_metrics(const gs_config* cfg, const char* path, const uint64_t* row_ptr,
                                    const uint8_t* mesh_count, const gs_publish* sched, uint64_t n_msgs,
                                    const gs_peer_delay* delay);

/* ---- peer-partitioned mode -------------------------
 * Context `part` of `parts` owns the keys of peers [part*N/parts,
 * (part+1)*N/parts); topology and mesh are built identically (replicated) in
 * every partition. One batch (<= cfg.batch messages of equal size) is driven
 * bucket by bucket by the caller, who performs the exchange:
 *   k = min over parts of gs_part_begin(...)
 *   while k != UINT64_MAX:
 *     gs_part_scan(ctx, k, recs, cap, &n, &m1)        -- own arrivals of k's bucket
 *     all-gather the n records of every part           -- RCCL / loop-back
 *     gs_part_relax(ctx, k, all_recs, n_all, &m2)      -- edges into own peers
 *     k = min over parts of min(m1, m2)
 *   gs_part_finish(ctx, sink)                         -- sink rows hold own peers
 * Record pointers are DEVICE pointers on the context's device; the records
 * passed to gs_part_relax must be complete when it is called (synchronise the
 * stream that gathered them). A scan whose records exceed `capacity` returns
 * GS_ERANGE with *out_n = the capacity needed and changes no state: call it
 * again with a larger buffer. IDONTWANT, churn and per-peer traffic are not
 * supported in this mode, lazy gossip only as the proven no-op
 * (GS_EUNSUPPORTED). Results are bit-identical to gs_run. */
typedef struct gs_part_record {
    uint64_t key;      /* packed first-arrival key (t_rel | hops | src)          */
    uint64_t start;    /* uplink start of its forward (FIFO fold by the owner)   */
    uint32_t peer;     /* global id of the forwarding peer                        */
    uint32_t slot;     /* message * FP + fragment within the batch               */
} gs_part_record;

gs_status gs_set_partition(struct gs_ctx* ctx, uint32_t parts, uint32_t part);
gs_status gs_part_begin(struct gs_ctx* ctx, const gs_publish* sched, uint64_t n_msgs,
                        uint64_t* out_min_key);
gs_status gs_part_scan(struct gs_ctx* ctx, uint64_t bucket_key, gs_part_record* dev_records,
                       uint64_t capacity, uint64_t* out_n, uint64_t* out_min_key);
gs_status gs_part_relax(struct gs_ctx* ctx, uint64_t bucket_key, const gs_part_record* dev_records,
                        uint64_t n, uint64_t* out_min_key);
/* sink arrays are [n_msgs][own peers] (message-major over this part's peers) */
gs_status gs_part_finish(struct gs_ctx* ctx, const gs_result_sink* sink);

/* ---- multi-GPU communicator and the library-driven partitioned run ---------
 * (SURVEY §8b gs_comm_init, §8e; the reference's process boundary is one swarm
 * task per process, rust-test-node/src/main.rs:466-477.) One rank per process
 * and GPU over RCCL (xGMI), or several parts in one process (loopback device
 * copies: tests, several parts on one GPU). */
typedef struct gs_comm gs_comm;
#define GS_COMM_ID_BYTES 128
typedef struct gs_comm_id { char internal[GS_COMM_ID_BYTES]; } gs_comm_id;
/* An RCCL unique id: rank 0 creates it and hands it to the other ranks out of
 * band (as ncclGetUniqueId). GS_EUNSUPPORTED when RCCL cannot be loaded. */
gs_status gs_comm_get_id(gs_comm_id* out);
/* This process's rank of an nranks-rank RCCL communicator on HIP device
 * `device` (collective: every rank calls it). */
gs_status gs_comm_init(uint32_t nranks, uint32_t rank, const gs_comm_id* id, int32_t device, gs_comm** out);
/* nparts parts driven by this process (one context each, any devices). */
gs_status gs_comm_init_local(uint32_t nparts, gs_comm** out);
/* ABI 10: a rank whose collectives are the caller's own transport (any
 * process launcher: torch.distributed gloo, MPI, sockets). The library stages
 * every collective of the partitioned protocols through host memory and calls
 *  - allgather(user, mine, n, out): every rank's n u64 words into
 *    out[rank * n + k] (the MIN / MAX all-reduces are reduced from it);
 *  - exchange(user, send, send_bytes, recv, recv_bytes): an all-to-all-v of
 *    host bytes — send[p] (send_bytes[p] bytes) to rank p, recv[p]
 *    (recv_bytes[p] bytes, sizes known to both ends) from rank p, for every
 *    p < nranks (the own entry is 0 bytes).
 * A callback returns 0 on success; anything else fails the call on this rank
 * (the others then fail in their next collective or in the transport).
 * Collective order and sizes are the RCCL backend's, so every rank of a run
 * makes the same calls in the same order. `device` is the rank's HIP device. */
typedef struct gs_comm_ops {
    void* user;
    int (*allgather)(void* user, const uint64_t* mine, uint64_t n, uint64_t* out);
    int (*exchange)(void* user, const void* const* send, const uint64_t* send_bytes, void* const* recv,
                    const uint64_t* recv_bytes);
} gs_comm_ops;
gs_status gs_comm_init_ops(uint32_t nranks, uint32_t rank, const gs_comm_ops* ops, int32_t device, gs_comm** out);
/* Transport check (ABI 10, host memory only, no device work): one allgather of
 * (rank, nranks) words and one exchange of position-hashed buffers of
 * 1 + 977 * (sender + 3 * receiver) bytes, each checked; GS_EDEVICE names the
 * first mismatch. For gs_comm_init_ops communicators (others: GS_OK). */
gs_status gs_comm_check(gs_comm* comm);
gs_status gs_comm_destroy(gs_comm* comm);
/* gs_run with the peers partitioned over the communicator's parts: ctxs are
 * this process's contexts (RCCL: nctx = 1, the rank's; local: nctx = nparts,
 * part i = ctxs[i]), all built with the same config, topology and mesh. The
 * library sets each context's partition, runs every batch on the list pass
 * over own rows (records exchanged between window passes: loop-back parts on
 * one device store each record straight into the parts owning a receiver and
 * combine the pass control on the device; ranks exchange every part's records,
 * or with GS_PART_ROUTE=1 only the routed ones) or the bucket
 * protocol (per bucket: own scan, records routed only to the parts owning a
 * target with grouped send/recv, relax into own peers, MIN all-reduce of the
 * next bucket key) and writes part i's peers to sinks[i] ([n_msgs][own peers];
 * sinks may be NULL). Batches the peer protocols cannot take — churn,
 * IDONTWANT, lazy gossip whose IWANTs can change the result — run
 * message-sharded over the replicated graph (part p simulates its share of
 * the batch's messages for all peers, one all-to-all hands every part its own
 * peers' rows; gs_stats.ms_batches counts them). Collective over the
 * communicator. Results are bit-identical to gs_run. GS_EUNSUPPORTED: per-peer
 * traffic (gs_set_traffic), per-peer pubsub counts (gs_set_pubsub_counts),
 * per-link first deliveries (gs_set_link_deliveries), per-message costs
 * (gs_set_message_costs), and sink summaries of a
 * message-sharded batch.
 * Every sinks[i] follows gs_result_sink's rules (GS_EINVAL otherwise); on_lat
 * receives [n][own peers] u16, and the parts' blocks side by side are gs_run's
 * on_lat stream. GS_ERANGE (a logged latency of 65535 ms or more): no part, and
 * no rank, hands out a block of the failing batch, and every rank returns it. */
gs_status gs_run_partitioned(struct gs_ctx* const* ctxs, uint32_t nctx, gs_comm* comm, const gs_publish* sched,
                             uint64_t n_msgs, const gs_result_sink* sinks);

/* gs_run_partitioned whose only output is the arrival log's text, each part formatting
 * the lines of its own peers on its own device. on_text is called with users[i] for
 * ctxs[i] (users may be NULL: user = NULL for every part).
 * For the part that owns peers [u0, u1), its calls' text in call order is gs_run_log's text
 * of an unpartitioned context (same config and schedule, fresh line counters) with only the
 * lines of peers in [u0, u1) kept, in their order there: message-major, ascending peer id
 * inside a message. So the parts' lines together are gs_run_log's lines, and a peer's line
 * numbers do not depend on the split. Per part, first_msg / n_msgs tile the schedule in
 * order; chunks hold whole messages and never span batches; chunk_bytes is per part (0 =
 * the default, a smaller value is raised to one message's bound over the part's peers).
 * All callbacks run on the calling thread; the order of calls between parts is unspecified.
 * Line counters: see gs_log_text_reset. GS_ERANGE (a latency of 65535 ms or more, a line
 * counter passing 2^32 - 1): no part, and no rank, hands out text of the failing batch, and
 * every rank returns it. GS_EINVAL: on_text is NULL. */
gs_status gs_run_partitioned_log(struct gs_ctx* const* ctxs, uint32_t nctx, gs_comm* comm,
                                 const gs_publish* sched, uint64_t n_msgs,
                                 gs_text_fn on_text, void* const* users, uint64_t chunk_bytes);

#ifdef __cplusplus
}
#endif
#endif /* GOSSIPSIM_H */
