"""Python host mirror of the reference's test-node interface over libgossipsim.so.

The reference node (rust-test-node/src/main.rs) reads its knobs from the env
(env.rs:27-87), dials random peers (main.rs:303-389), accepts
`POST /publish {"topic","msgSize","version"}` (main.rs:50-56,146-221) and
prints `<tx_time> milliseconds: <latency>` per completed message (main.rs:93).
This module keeps those names and error behaviour on top of the C ABI in
include/gossipsim.h:

    cfg = PeerConfig.from_env()          # env.rs get_peer_details
    sim = Simulator(cfg)                 # SwarmBuilder + build_behaviour
    sim.set_topogen_links(...)           # shadow/topogen.py link graph
    sim.connect_gossipsub_peers()        # main.rs:303-389 -> CSR on the GPU
    sim.mesh_converge()                  # heartbeat GRAFT/PRUNE fixed point
    sim.publish(publisher, msg_size, t)  # POST /publish
    res = sim.run()                      # receive/forward/reassemble on the GPU
    sim.write_latency_log(path, res)     # awk-parseable arrival lines

Everything here is plumbing; all simulation work runs in the HIP library. The
library must be present: there is no CPU fallback (a missing .so raises).
"""
import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GOSSIPSIM_LIB", os.path.join(HERE, "libgossipsim.so"))
ABI_VERSION = 10
MESH_W = 16
UNDELIVERED = np.uint64(0xFFFFFFFFFFFFFFFF)
MUXERS = {"yamux": 0, "quic": 1, "mplex": 2}
NODES = {"rust": 0, "go": 1, "nim": 2}  # GS_NODE_*: rust-test-node, go-test-node, nim gossipsub-queues
STATUS = {0: "GS_OK", -1: "GS_EINVAL", -2: "GS_ENOMEM", -3: "GS_EDEVICE", -4: "GS_ESTATE",
          -5: "GS_ERANGE", -6: "GS_EUNSUPPORTED"}

u32, u64, i32, u8 = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int32, ctypes.c_uint8
P = ctypes.POINTER


class GsConfig(ctypes.Structure):
    _fields_ = [(n, u32) for n in (
        "abi_version", "peers", "connect_to", "dial_extra", "max_connections", "fragments",
        "muxer", "signed_msgs", "d", "d_lo", "d_hi", "d_lazy", "d_out", "gossip_factor_milli")] + [
        ("heartbeat_ns", u64), ("backoff_ns", u64)] + [
        (n, u32) for n in ("flood_publish", "idontwant", "lazy_gossip", "self_log")] + [
        ("seed", u64), ("device", i32), ("batch", u32), ("history_gossip", u32), ("hb_phase_ns", u64)] + [
        (n, u32) for n in ("churn_ppm", "churn_down", "churn_horizon", "node", "sub_graft", "hs_rtts")]


class GsPublish(ctypes.Structure):
    _fields_ = [("t_pub_ns", u64), ("publisher", u32), ("msg_size", u32), ("frags", u32), ("reserved", u32)]


HIST_BINS, HIST_MS = 64, 100  # GS_HIST_BINS / GS_HIST_MS


class GsMsgSummary(ctypes.Structure):
    _fields_ = [("delivered", u64), ("lat_sum_ms", u64), ("p50_ms", u32), ("p95_ms", u32), ("max_ms", u32),
                ("reserved", u32), ("hist", u32 * HIST_BINS)]


BLOCK_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p, u64, u32, u32, P(u64), P(u8))
LAT_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p, u64, u32, u32, P(ctypes.c_uint16))
TEXT_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p, u64, u32, ctypes.c_void_p, u64, u64)  # gs_text_fn


class GsResultSink(ctypes.Structure):
    _fields_ = [("t_complete_ns", P(u64)), ("hops", P(u8)), ("on_block", BLOCK_FN), ("user", ctypes.c_void_p),
                ("block_msgs", u32), ("want", u32), ("summary", P(GsMsgSummary)), ("on_lat", LAT_FN)]


WANT_T_COMPLETE, WANT_HOPS, WANT_LAT_MS = 1, 2, 4  # gs_result_sink.want (GS_WANT_*)
LAT_NONE = 0xFFFF  # GS_LAT_NONE: the peer logs nothing for the message


class GsStats(ctypes.Structure):
    _fields_ = [(n, u64) for n in (
        "messages", "deliveries", "frag_deliveries", "relaxations", "bytes_alg",
        "latency_sum_ms", "latency_max_ms", "relax_launches", "buckets")] + [
        ("relax_ms", ctypes.c_double), ("run_ms", ctypes.c_double), ("relax_bytes_alg", u64),
        ("pushes", u64), ("scan_ms", ctypes.c_double), ("frontier_ms", ctypes.c_double),
        ("gossip_iwant", u64), ("gossip_noop_msgs", u64), ("gossip_fallback_batches", u64), ("batches", u64),
        ("list_pull_batches", u64), ("ms_batches", u64), ("gossip_list_batches", u64)]


class GsInjector(ctypes.Structure):
    _fields_ = [("start_ns", u64), ("delay_ns", u64), ("msg_size", u32), ("messages", u32), ("peers", u32),
                ("reserved", u32)]


ALLGATHER_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, P(u64), u64, P(u64))
EXCHANGE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, P(ctypes.c_void_p), P(u64), P(ctypes.c_void_p), P(u64))


class GsCommOps(ctypes.Structure):  # gs_comm_ops (ABI 10)
    _fields_ = [("user", ctypes.c_void_p), ("allgather", ALLGATHER_FN), ("exchange", EXCHANGE_FN)]


DELAY_BOUNDS_MS = (1, 5, 10, 25, 50, 100, 250, 500, 1000, 2500, 5000, 10000)  # main.nim:59; GS_DELAY_BUCKETS


class GsPeerDelay(ctypes.Structure):  # gs_peer_delay
    _fields_ = [("completed", u64), ("delay_sum_ms", u64), ("last_rx_ns", u64), ("last_ms", u32), ("reserved", u32),
                ("bucket", u64 * (len(DELAY_BOUNDS_MS) + 1))]


# the same layout as a numpy structured dtype (Simulator.peer_delay)
PEER_DELAY_DTYPE = np.dtype([("completed", "<u8"), ("delay_sum_ms", "<u8"), ("last_rx_ns", "<u8"), ("last_ms", "<u4"),
                             ("reserved", "<u4"), ("bucket", "<u8", (len(DELAY_BOUNDS_MS) + 1,))])


class GsPartRecord(ctypes.Structure):
    _fields_ = [("key", u64), ("start", u64), ("peer", u32), ("slot", u32)]


# Every symbol include/gossipsim.h declares, with its ctypes signature.
SIGNATURES = {
    "gs_config_default": (None, [P(GsConfig)]),
    "gs_config_preset": (i32, [P(GsConfig), u32]),
    "gs_write_node_log": (i32, [P(GsConfig), ctypes.c_char_p, P(GsPublish), u64, P(u64)]),
    "gs_log_open": (i32, [P(GsConfig), ctypes.c_char_p, P(ctypes.c_void_p)]),
    "gs_log_write": (i32, [ctypes.c_void_p, P(GsPublish), u32, P(u64)]),
    "gs_log_write_lat": (i32, [ctypes.c_void_p, P(GsPublish), u32, P(ctypes.c_uint16)]),
    "gs_log_close": (i32, [ctypes.c_void_p]),
    "gs_config_from_env": (i32, [P(GsConfig), ctypes.c_char_p, ctypes.c_size_t]),
    "gs_wire_bytes": (u64, [u64, u32, u32]),
    "gs_wire_packets": (None, [u64, u32, u32, P(u64), P(u64)]),
    "gs_control_packets": (None, [u32, u32, u32, P(u64), P(u64), P(u64)]),
    "gs_write_shadow_heartbeat": (i32, [ctypes.c_char_p, u32, P(u64), u64]),
    "gs_links_from_gml": (i32, [ctypes.c_char_p, u32, u32, P(u32), P(u64), P(u64), P(u64)]),
    "gs_shadow_hosts": (i32, [ctypes.c_char_p, u32, P(u8)]),
    "gs_write_node_metrics": (i32, [P(GsConfig), ctypes.c_char_p, P(u64), P(u8), P(u64)]),
    "gs_set_traffic": (i32, [ctypes.c_void_p, u32]),
    "gs_get_traffic": (i32, [ctypes.c_void_p, P(u64)]),
    "gs_set_pubsub_counts": (i32, [ctypes.c_void_p, u32]),
    "gs_get_pubsub_counts": (i32, [ctypes.c_void_p, P(u64)]),
    "gs_reset_pubsub_counts": (i32, [ctypes.c_void_p]),
    "gs_write_pubsub_metrics": (i32, [P(GsConfig), ctypes.c_char_p, u32, P(u64)]),
    "gs_set_link_deliveries": (i32, [ctypes.c_void_p, u32]),
    "gs_get_link_deliveries": (i32, [ctypes.c_void_p, P(u64)]),
    "gs_get_peer_given": (i32, [ctypes.c_void_p, P(u64)]),
    "gs_reset_link_deliveries": (i32, [ctypes.c_void_p]),
    "gs_write_link_deliveries": (i32, [ctypes.c_char_p, u32, P(u64), P(u32), P(u64)]),
    "gs_set_message_costs": (i32, [ctypes.c_void_p, u32]),
    "gs_message_costs_rows": (i32, [ctypes.c_void_p, P(u64)]),
    "gs_get_message_costs": (i32, [ctypes.c_void_p, P(u64), u64]),
    "gs_write_message_costs": (i32, [P(GsConfig), ctypes.c_char_p, P(GsPublish), u64, P(u64)]),
    "gs_set_mesh_events": (i32, [ctypes.c_void_p, u32]),
    "gs_get_mesh_events": (i32, [ctypes.c_void_p, P(u64)]),
    "gs_mesh_series_rows": (i32, [ctypes.c_void_p, P(u32)]),
    "gs_get_mesh_series": (i32, [ctypes.c_void_p, P(u64), u32]),
    "gs_write_mesh_metrics": (i32, [P(GsConfig), ctypes.c_char_p, u32, P(u64), P(u8), P(u64)]),
    "gs_write_mesh_series": (i32, [ctypes.c_char_p, P(u64), u32]),
    "gs_set_peer_delay": (i32, [ctypes.c_void_p, u32]),
    "gs_get_peer_delay": (i32, [ctypes.c_void_p, P(GsPeerDelay)]),
    "gs_reset_peer_delay": (i32, [ctypes.c_void_p]),
    "gs_peer_delay_add_lat": (i32, [ctypes.c_void_p, P(GsPublish), u64, P(ctypes.c_uint16)]),
    "gs_write_testnode_metrics": (i32, [P(GsConfig), ctypes.c_char_p, P(u64), P(u8), P(GsPublish), u64,
                                        P(GsPeerDelay)]),
    "gs_topogen_links": (i32, [u32, u32, u32, u32, u32, u32, P(u64), P(u64)]),
    "gs_schedule_runsh": (i32, [u32, u32, u32, u32, u64, u64, u32, P(GsPublish)]),
    "gs_shadow_injector": (i32, [ctypes.c_char_p, P(GsInjector)]),
    "gs_read_schedule": (i32, [ctypes.c_char_p, P(GsPublish), u64, P(u64)]),
    "gs_write_latency_log": (i32, [ctypes.c_char_p, P(GsPublish), u64, u32, P(u64), u32]),
    "gs_create": (i32, [P(GsConfig), P(ctypes.c_void_p)]),
    "gs_destroy": (i32, [ctypes.c_void_p]),
    "gs_last_error": (ctypes.c_char_p, [ctypes.c_void_p]),
    "gs_set_links": (i32, [ctypes.c_void_p, u32, P(u64), P(u64), P(u64), P(u8)]),
    "gs_build_topology": (i32, [ctypes.c_void_p]),
    "gs_set_topology": (i32, [ctypes.c_void_p, P(u64), P(u32), P(u8)]),
    "gs_set_topology_dials": (i32, [ctypes.c_void_p, u64, P(u32), P(u32)]),
    "gs_read_dials": (i32, [ctypes.c_char_p, P(u32), P(u32), u64, P(u64)]),
    "gs_write_dials": (i32, [ctypes.c_char_p, u32, P(u64), P(u32), P(u8)]),
    "gs_graph_info": (i32, [ctypes.c_void_p, P(u32), P(u64), P(u32)]),
    "gs_get_csr": (i32, [ctypes.c_void_p, P(u64), P(u32), P(u8)]),
    "gs_mesh_converge": (i32, [ctypes.c_void_p, u32, P(u32)]),
    "gs_get_mesh": (i32, [ctypes.c_void_p, P(u32), P(u8)]),
    "gs_set_mesh": (i32, [ctypes.c_void_p, P(u32), P(u8)]),
    "gs_set_mesh_links": (i32, [ctypes.c_void_p, u64, P(u32), P(u32)]),
    "gs_write_mesh_links": (i32, [ctypes.c_char_p, u32, P(u32), P(u8)]),
    "gs_set_outages": (i32, [ctypes.c_void_p, u64, P(u32), P(u32), P(u32)]),
    "gs_clear_outages": (i32, [ctypes.c_void_p]),
    "gs_get_offline": (i32, [ctypes.c_void_p, u32, u32, P(u64)]),
    "gs_outage_epochs": (i32, [P(GsConfig), u64, P(u32), P(u64), P(u64), P(u32), P(u32), P(u32), P(u64)]),
    "gs_read_outages": (i32, [ctypes.c_char_p, P(u32), P(u64), P(u64), u64, P(u64)]),
    "gs_run": (i32, [ctypes.c_void_p, P(GsPublish), u64, P(GsResultSink)]),
    "gs_run_log": (i32, [ctypes.c_void_p, P(GsPublish), u64, TEXT_FN, ctypes.c_void_p, u64]),
    "gs_format_lat_log": (i32, [ctypes.c_void_p, P(GsPublish), u64, P(ctypes.c_uint16), TEXT_FN, ctypes.c_void_p,
                                u64]),
    "gs_log_text_reset": (i32, [ctypes.c_void_p]),
    "gs_log_line_max": (u32, [P(GsConfig)]),
    "gs_get_stats": (i32, [ctypes.c_void_p, P(GsStats)]),
    "gs_get_config": (i32, [ctypes.c_void_p, P(GsConfig)]),
    "gs_save_state": (i32, [ctypes.c_void_p, ctypes.c_char_p]),
    "gs_load_state": (i32, [ctypes.c_char_p, i32, P(ctypes.c_void_p)]),
    "gs_reset_stats": (i32, [ctypes.c_void_p]),
    "gs_set_timing": (i32, [ctypes.c_void_p, u32]),
    "gs_set_partition": (i32, [ctypes.c_void_p, u32, u32]),
    "gs_part_begin": (i32, [ctypes.c_void_p, P(GsPublish), u64, P(u64)]),
    "gs_part_scan": (i32, [ctypes.c_void_p, u64, ctypes.c_void_p, u64, P(u64), P(u64)]),
    "gs_part_relax": (i32, [ctypes.c_void_p, u64, ctypes.c_void_p, u64, P(u64)]),
    "gs_part_finish": (i32, [ctypes.c_void_p, P(GsResultSink)]),
    "gs_comm_get_id": (i32, [ctypes.c_char_p]),
    "gs_comm_init": (i32, [u32, u32, ctypes.c_char_p, i32, P(ctypes.c_void_p)]),
    "gs_comm_init_local": (i32, [u32, P(ctypes.c_void_p)]),
    "gs_comm_init_ops": (i32, [u32, u32, ctypes.c_void_p, i32, P(ctypes.c_void_p)]),
    "gs_comm_check": (i32, [ctypes.c_void_p]),
    "gs_comm_destroy": (i32, [ctypes.c_void_p]),
    "gs_run_partitioned": (i32, [P(ctypes.c_void_p), u32, ctypes.c_void_p, P(GsPublish), u64, P(GsResultSink)]),
    "gs_run_partitioned_log": (i32, [P(ctypes.c_void_p), u32, ctypes.c_void_p, P(GsPublish), u64, TEXT_FN,
                                     P(ctypes.c_void_p), u64]),
}
COMM_ID_BYTES = 128
GS_EINVAL = -1
GS_ERANGE = -5
KEY_NONE = (1 << 64) - 1  # empty-bucket marker of the partitioned protocol

_lib = None


def lib():
    """Load libgossipsim.so; raise if it is missing (no fallback path exists)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libgossipsim.so not built at %s: run __graft_entry__.build() "
                               "(make -C dst-libp2p-test-node_amd)" % LIB_PATH)
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


class GossipSimError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__("%s (%d): %s" % (STATUS.get(status, "?"), status, msg))
        self.status = status


def _ptr(a, ct):
    return a.ctypes.data_as(P(ct))


def log_line_max(cfg):
    """The longest arrival-log line `cfg` (a PeerConfig) can produce, in bytes (gs_log_line_max)."""
    return int(lib().gs_log_line_max(ctypes.byref(cfg.c)))


def wire_bytes(payload, muxer="yamux", signed=True):
    return int(lib().gs_wire_bytes(payload, MUXERS[muxer] if isinstance(muxer, str) else muxer,
                                   1 if signed else 0))


def wire_packets(payload, muxer="yamux", signed=True):
    """-> (packets, header bytes) of one fragment send (the model of wire_bytes)."""
    pk, hd = u64(), u64()
    lib().gs_wire_packets(payload, MUXERS[muxer] if isinstance(muxer, str) else muxer, 1 if signed else 0,
                          ctypes.byref(pk), ctypes.byref(hd))
    return pk.value, hd.value


CTRL_KINDS = {"ihave": 0, "iwant": 1, "ack": 2}


def control_packets(kind, node="rust", muxer="yamux"):
    """-> (wire bytes, packets, header bytes) of one IHAVE / IWANT RPC (one
    message id) or one pure ACK packet (gs_control_packets)."""
    b, pk, hd = u64(), u64(), u64()
    lib().gs_control_packets(CTRL_KINDS.get(kind, kind), NODES.get(node, node) if isinstance(node, str) else node,
                             MUXERS[muxer] if isinstance(muxer, str) else muxer,
                             ctypes.byref(b), ctypes.byref(pk), ctypes.byref(hd))
    return b.value, pk.value, hd.value


TRAFFIC_COLS = ("tx_bytes", "rx_bytes", "tx_packets", "rx_packets", "tx_header_bytes", "rx_header_bytes",
                "received", "published", "tx_ctrl_packets", "rx_ctrl_packets", "tx_ctrl_header_bytes",
                "rx_ctrl_header_bytes")


def write_shadow_heartbeat(path, traffic, sim_seconds=900):
    """Per-peer traffic [N, len(TRAFFIC_COLS)] as Shadow tracker "[node]" lines (shadow/summary_shadowlog.awk);
    sim_seconds defaults to topogen's 15-minute stop time (shadow/topogen.py:82)."""
    tr = np.ascontiguousarray(traffic, np.uint64)
    rc = lib().gs_write_shadow_heartbeat(path.encode(), tr.shape[0], _ptr(tr, u64), sim_seconds)
    if rc:
        raise GossipSimError(rc, "gs_write_shadow_heartbeat failed")


def write_node_metrics(cfg, path, row_ptr, mesh_count, traffic):
    """OpenMetrics text of the test node's metrics for every peer (gs_write_node_metrics)."""
    row = np.ascontiguousarray(row_ptr, np.uint64)
    mc = np.ascontiguousarray(mesh_count, np.uint8)
    tr = np.ascontiguousarray(traffic, np.uint64)
    rc = lib().gs_write_node_metrics(ctypes.byref(cfg.c), path.encode(), _ptr(row, u64), _ptr(mc, u8), _ptr(tr, u64))
    if rc:
        raise GossipSimError(rc, "gs_write_node_metrics failed")


# gs_get_pubsub_counts columns (GS_PS_*)
PUBSUB_COLS = ("msg_tx", "msg_rx", "first", "dup", "ihave_tx", "ihave_rx", "iwant_tx", "iwant_rx")


def write_pubsub_metrics(cfg, path, counts):
    """Prometheus text of the go node's pubsub counters (libp2p_pubsub_*, libp2p_gossipsub_received /
    duplicate, go-test-node/metrics.go:84-220) and the nim node's dst_testnode_received_chunks_total
    for every peer (gs_write_pubsub_metrics). counts: uint64 [peers, len(PUBSUB_COLS)]
    (Simulator.pubsub_counts)."""
    pc = np.ascontiguousarray(counts, np.uint64)
    if pc.ndim != 2 or pc.shape[1] != len(PUBSUB_COLS):
        raise GossipSimError(GS_EINVAL, "counts [peers, %d] are needed" % len(PUBSUB_COLS))
    rc = lib().gs_write_pubsub_metrics(ctypes.byref(cfg.c), path.encode(), pc.shape[0], _ptr(pc, u64))
    if rc:
        raise GossipSimError(rc, "gs_write_pubsub_metrics failed")


# gs_get_mesh_events columns (GS_ME_*) and gs_get_mesh_series columns (GS_MS_*)
MESH_EVENT_COLS = ("tx_graft", "rx_graft", "tx_prune", "rx_prune", "mesh_add", "mesh_del", "mesh_drop")
MESH_SERIES_COLS = ("online", "no_peers", "low", "healthy", "over", "links", "grafts", "rejects", "prunes", "drops",
                    "adds", "dels")


def write_mesh_metrics(cfg, path, row_ptr, mesh_count, events):
    """Prometheus text of the go node's GRAFT / PRUNE / subscription counters and mesh gauges
    (go-test-node/metrics.go:164-190, 224-258, 328-362) for every peer (gs_write_mesh_metrics).
    events: uint64 [peers, len(MESH_EVENT_COLS)] (Simulator.mesh_events)."""
    ev = np.ascontiguousarray(events, np.uint64)
    if ev.ndim != 2 or ev.shape[1] != len(MESH_EVENT_COLS):
        raise GossipSimError(GS_EINVAL, "events [peers, %d] are needed" % len(MESH_EVENT_COLS))
    row = np.ascontiguousarray(row_ptr, np.uint64)
    mc = np.ascontiguousarray(mesh_count, np.uint8)
    if row.shape != (ev.shape[0] + 1,) or mc.shape != (ev.shape[0],):
        raise GossipSimError(GS_EINVAL, "row_ptr [peers + 1] and mesh_count [peers] are needed")
    rc = lib().gs_write_mesh_metrics(ctypes.byref(cfg.c), path.encode(), ev.shape[0], _ptr(row, u64), _ptr(mc, u8),
                                     _ptr(ev, u64))
    if rc:
        raise GossipSimError(rc, "gs_write_mesh_metrics failed")


def write_mesh_series(path, series):
    """The per-epoch mesh health as CSV (gs_write_mesh_series). series: uint64
    [rows, len(MESH_SERIES_COLS)] (Simulator.mesh_series)."""
    se = np.ascontiguousarray(series, np.uint64)
    if se.ndim != 2 or se.shape[1] != len(MESH_SERIES_COLS):
        raise GossipSimError(GS_EINVAL, "series [rows, %d] are needed" % len(MESH_SERIES_COLS))
    rc = lib().gs_write_mesh_series(path.encode(), _ptr(se, u64), se.shape[0])
    if rc:
        raise GossipSimError(rc, "gs_write_mesh_series failed")


# gs_get_link_deliveries / gs_get_peer_given columns (GS_LD_*)
LINK_DELIVERY_COLS = ("publish", "mesh", "gossip")


def write_link_deliveries(path, row_ptr, col, counts):
    """One "receiver sender publish mesh gossip" line per CSR entry with a non-zero count, in CSR
    order (gs_write_link_deliveries). row_ptr, col: Simulator.csr()'s; counts: uint64
    [nnz, len(LINK_DELIVERY_COLS)] (Simulator.link_deliveries)."""
    row = np.ascontiguousarray(row_ptr, np.uint64)
    c = np.ascontiguousarray(col, np.uint32)
    ld = np.ascontiguousarray(counts, np.uint64)
    if row.ndim != 1 or row.size < 2 or c.ndim != 1 or c.size != int(row[-1]):
        raise GossipSimError(GS_EINVAL, "row_ptr [peers + 1] and col [row_ptr[-1]] are needed")
    if ld.ndim != 2 or ld.shape != (c.size, len(LINK_DELIVERY_COLS)):
        raise GossipSimError(GS_EINVAL, "counts [nnz, %d] are needed" % len(LINK_DELIVERY_COLS))
    pad = 1 if c.size == 0 else 0  # (a pointer to take)
    rc = lib().gs_write_link_deliveries(str(path).encode(), row.size - 1, _ptr(row, u64),
                                        _ptr(np.resize(c, c.size + pad), u32),
                                        _ptr(np.resize(ld.reshape(-1), ld.size + pad), u64))
    if rc:
        raise GossipSimError(rc, "cannot write the link deliveries %s" % path)


# gs_get_message_costs columns (GS_MC_*)
MESSAGE_COST_COLS = ("data_tx", "data_rx", "first", "dup", "ihave_tx", "ihave_rx", "iwant", "delivered")


def write_message_costs(cfg, path, schedule, costs):
    """One TSV line per message: the schedule fields, the MESSAGE_COST_COLS counts and the wire
    bytes, packets and ACKs they cost (gs_write_message_costs). schedule: a GsPublish array
    or the (t, publisher, msg_size[, frags]) arrays of the run's messages; costs: uint64
    [messages, len(MESSAGE_COST_COLS)] (Simulator.message_costs)."""
    sched = schedule if isinstance(schedule, ctypes.Array) else Simulator._schedule(None, schedule)
    M = len(sched)
    mc = np.ascontiguousarray(costs, np.uint64)
    if mc.ndim != 2 or mc.shape != (M, len(MESSAGE_COST_COLS)):
        raise GossipSimError(GS_EINVAL, "costs [messages, %d] are needed" % len(MESSAGE_COST_COLS))
    pad = 1 if M == 0 else 0  # (a pointer to take)
    rc = lib().gs_write_message_costs(ctypes.byref(cfg.c), str(path).encode(), sched, M,
                                      _ptr(np.resize(mc.reshape(-1), mc.size + pad), u64))
    if rc:
        raise GossipSimError(rc, "cannot write the message costs %s" % path)


def write_testnode_metrics(cfg, path, row_ptr, mesh_count, schedule, delay):
    """Prometheus text of the nim node's application metrics (dst_testnode_*, nim gossipsub-queues
    main.nim:25-78) for every peer (gs_write_testnode_metrics). schedule: a GsPublish array
    (publish requests per peer); delay: a PEER_DELAY_DTYPE array [peers] (Simulator.peer_delay,
    the parts' arrays concatenated)."""
    row = np.ascontiguousarray(row_ptr, np.uint64)
    mc = np.ascontiguousarray(mesh_count, np.uint8)
    pd = np.ascontiguousarray(delay, PEER_DELAY_DTYPE)
    if pd.shape != (cfg.peers,) or row.shape != (cfg.peers + 1,) or mc.shape != (cfg.peers,):
        raise GossipSimError(GS_EINVAL, "row_ptr [peers + 1], mesh_count [peers] and delay [peers] are needed")
    rc = lib().gs_write_testnode_metrics(ctypes.byref(cfg.c), path.encode(), _ptr(row, u64), _ptr(mc, u8), schedule,
                                         len(schedule), _ptr(pd, GsPeerDelay))
    if rc:
        raise GossipSimError(rc, "gs_write_testnode_metrics failed")


def links_from_gml(path, shortest=False):
    """Shadow network graph (network_topology.gml) -> (lat_ns[V,V], bw_up[V], bw_down[V])."""
    V = u32()
    cap = 16
    while True:
        lat, up, dn = np.zeros(cap * cap, np.uint64), np.zeros(cap, np.uint64), np.zeros(cap, np.uint64)
        rc = lib().gs_links_from_gml(path.encode(), 1 if shortest else 0, cap, ctypes.byref(V), _ptr(lat, u64),
                                     _ptr(up, u64), _ptr(dn, u64))
        if rc == GS_ERANGE and V.value > cap:
            cap = V.value
            continue
        if rc:
            raise GossipSimError(rc, "cannot ingest %s" % path)
        n = V.value
        return lat[:n * n].reshape(n, n), up[:n], dn[:n]


def shadow_hosts(path, peers):
    """shadow.yaml hosts pod-<i> -> network_node_id, as the stage_of_peer array of set_links."""
    st = np.zeros(peers, np.uint8)
    rc = lib().gs_shadow_hosts(path.encode(), peers, _ptr(st, u8))
    if rc:
        raise GossipSimError(rc, "cannot map the %d peers of %s" % (peers, path))
    return st


def topogen_links(stages=1, min_bw=50, max_bw=50, min_lat=100, max_lat=100, shortest=False):
    """shadow/topogen.py:39-71 -> (lat_ns[S,S], bw_bps[S]); defaults = topogen.py:15-20."""
    lat = np.zeros(stages * stages, np.uint64)
    bw = np.zeros(stages, np.uint64)
    rc = lib().gs_topogen_links(stages, min_bw, max_bw, min_lat, max_lat, 1 if shortest else 0,
                                _ptr(lat, u64), _ptr(bw, u64))
    if rc:
        raise GossipSimError(rc, "invalid topogen parameters")
    return lat.reshape(stages, stages), bw


def schedule_runsh(n_msgs, peers, publisher_id, rotation, t0_ns, delay_ns, msg_size):
    """shadow/run.sh:34-36 publisher/rotation/delay -> structured schedule array."""
    out = (GsPublish * n_msgs)()
    rc = lib().gs_schedule_runsh(n_msgs, peers, publisher_id, rotation, t0_ns, delay_ns, msg_size,
                                 out)
    if rc:
        raise GossipSimError(rc, "invalid schedule")
    return out


def shadow_injector(path):
    """The injector process of a Shadow config (traffic_sync.py args + start_time, topogen.py:125-136)."""
    inj = GsInjector()
    rc = lib().gs_shadow_injector(path.encode(), ctypes.byref(inj))
    if rc:
        raise GossipSimError(rc, "no injector host in %s" % path)
    return {n: getattr(inj, n) for n, _ in GsInjector._fields_ if n != "reserved"}


def read_schedule(path):
    """Schedule file rows "t_pub_ns publisher msg_size [frags]" -> GsPublish array."""
    n = u64()
    rc = lib().gs_read_schedule(path.encode(), None, 0, ctypes.byref(n))
    if rc not in (0, GS_ERANGE):
        raise GossipSimError(rc, "malformed schedule %s" % path)
    out = (GsPublish * n.value)()
    rc = lib().gs_read_schedule(path.encode(), out, n.value, ctypes.byref(n))
    if rc:
        raise GossipSimError(rc, "malformed schedule %s" % path)
    return out


def _fits(a, nbytes):
    """An integer (or bool) array's values fit `nbytes` unsigned bytes (no pass over unsigned arrays that narrow)."""
    if a.size == 0 or a.dtype.kind == "b" or (a.dtype.kind == "u" and a.dtype.itemsize <= nbytes):
        return True
    return int(a.min()) >= 0 and int(a.max()) < (1 << (8 * nbytes))


def _csr_arrays(row_ptr, col, flags, peers=None):
    """A CSR's three arrays as gs_set_topology / gs_write_dials take them; dtype and shape errors raise here."""
    row, col, flags = np.asarray(row_ptr), np.asarray(col), np.asarray(flags)
    for name, a, kinds in (("row_ptr", row, "ui"), ("col", col, "ui"), ("flags", flags, "uib")):
        if a.ndim != 1:
            raise ValueError("%s must be one-dimensional" % name)
        if a.dtype.kind not in kinds and a.size:
            raise TypeError("%s must hold integers, not %s" % (name, a.dtype))
    if row.size < 2 or (peers is not None and row.size != peers + 1):
        raise ValueError("row_ptr must have peers + 1 entries")
    if row.size and row.dtype.kind == "i" and (row < 0).any():
        raise ValueError("row_ptr must not be negative")
    if not _fits(col, 4):
        raise ValueError("col must fit 32 unsigned bits")
    if not _fits(flags, 1):
        raise ValueError("flags must fit 8 unsigned bits")
    row = np.ascontiguousarray(row, np.uint64)
    if col.shape != flags.shape or col.size != int(row[-1]):
        raise ValueError("col and flags must have row_ptr[-1] entries each")
    pad = 1 if col.size == 0 else 0  # (a pointer to take)
    return (row, np.ascontiguousarray(np.resize(col, col.size + pad), np.uint32),
            np.ascontiguousarray(np.resize(flags, flags.size + pad), np.uint8))


def _dial_arrays(dialer, target, names=("dialer", "target")):
    d, t = np.asarray(dialer), np.asarray(target)
    for name, a in zip(names, (d, t)):
        if a.ndim != 1:
            raise ValueError("%s must be one-dimensional" % name)
        if a.size and a.dtype.kind not in "ui":
            raise TypeError("%s must hold integers, not %s" % (name, a.dtype))
        if not _fits(a, 4):
            raise ValueError("%s must fit 32 unsigned bits" % name)
    if d.shape != t.shape:
        raise ValueError("%s and %s must have the same length" % names)
    return np.ascontiguousarray(d, np.uint32), np.ascontiguousarray(t, np.uint32)


def _mesh_arrays(mesh, count, peers=None):
    """Mesh rows in Simulator.mesh()'s layout as gs_set_mesh / gs_write_mesh_links take them: [peers, MESH_W]
    (or flat) ids, count[peers] or None; dtype and shape errors raise here."""
    m = np.asarray(mesh)
    if m.ndim not in (1, 2) or (m.ndim == 2 and m.shape[1] != MESH_W) or m.size % MESH_W:
        raise ValueError("mesh must be [peers, %d] (or that many ids flat)" % MESH_W)
    if m.size and m.dtype.kind not in "ui":
        raise TypeError("mesh must hold integers, not %s" % m.dtype)
    if not _fits(m, 4):
        raise ValueError("mesh must fit 32 unsigned bits")
    n = m.size // MESH_W
    if n == 0 or (peers is not None and n != peers):
        raise ValueError("mesh must have peers rows")
    c = None
    if count is not None:
        c = np.asarray(count)
        if c.ndim != 1 or c.size != n:
            raise ValueError("count must have peers entries")
        if c.dtype.kind not in "uib":
            raise TypeError("count must hold integers, not %s" % c.dtype)
        if not _fits(c, 1):
            raise ValueError("count must fit 8 unsigned bits")
        c = np.ascontiguousarray(c, np.uint8)
    return np.ascontiguousarray(m.reshape(-1), np.uint32), c


def write_mesh_links(path, mesh, count=None):
    """One "a b" line per mesh link with a < b, in row order (gs_write_mesh_links); read_dials reads it back."""
    m, c = _mesh_arrays(mesh, count)
    rc = lib().gs_write_mesh_links(str(path).encode(), m.size // MESH_W, _ptr(m, u32), None if c is None else _ptr(c, u8))
    if rc:
        raise GossipSimError(rc, "cannot write the mesh links %s" % path)


def read_dials(path):
    """Dial list file, one "dialer target" pair per line -> (dialer, target) uint32 arrays (gs_read_dials)."""
    n = u64()
    rc = lib().gs_read_dials(str(path).encode(), None, None, 0, ctypes.byref(n))
    if rc not in (0, GS_ERANGE):
        raise GossipSimError(rc, "malformed dial list %s" % path)
    d, t = np.zeros(max(n.value, 1), np.uint32), np.zeros(max(n.value, 1), np.uint32)
    rc = lib().gs_read_dials(str(path).encode(), _ptr(d, u32), _ptr(t, u32), n.value, ctypes.byref(n))
    if rc:
        raise GossipSimError(rc, "malformed dial list %s" % path)
    return d[:n.value], t[:n.value]


OUTAGE_FOREVER = 0xFFFFFFFF  # GS_OUTAGE_FOREVER: h_to of a peer that never returns
OUTAGE_ROW_MAX = 256  # GS_OUTAGE_ROW_MAX
T_NEVER = 0xFFFFFFFFFFFFFFFF  # t_up_ns of a peer that never returns


def read_outages(path):
    """Outage file, one "peer t_down_ns [t_up_ns]" line per outage -> (peer uint32, t_down_ns, t_up_ns uint64)
    arrays (gs_read_outages); without a third column t_up_ns is T_NEVER."""
    n = u64()
    rc = lib().gs_read_outages(str(path).encode(), None, None, None, 0, ctypes.byref(n))
    if rc not in (0, GS_ERANGE):
        raise GossipSimError(rc, "malformed outage list %s: line %d" % (path, n.value))
    k = max(n.value, 1)
    p, d, t = np.zeros(k, np.uint32), np.zeros(k, np.uint64), np.zeros(k, np.uint64)
    rc = lib().gs_read_outages(str(path).encode(), _ptr(p, u32), _ptr(d, u64), _ptr(t, u64), n.value, ctypes.byref(n))
    if rc:
        raise GossipSimError(rc, "malformed outage list %s: line %d" % (path, n.value))
    return p[:n.value], d[:n.value], t[:n.value]


def outage_epochs(cfg, peer, t_down_ns, t_up_ns):
    """Outages in ns as intervals of heartbeat epochs under cfg's heartbeat_ns and hb_phase_ns (a PeerConfig, or
    anything with these two attributes) -> (peer, h_from, h_to) uint32 arrays (gs_outage_epochs): a peer is
    offline in epoch h >= 1 iff it is down at the heartbeat that starts it; an outage that covers no heartbeat
    is left out, t_up_ns == T_NEVER gives h_to == OUTAGE_FOREVER."""
    if isinstance(cfg, PeerConfig):
        c = cfg.c
    else:
        c = GsConfig()
        lib().gs_config_default(ctypes.byref(c))
        c.heartbeat_ns, c.hb_phase_ns = int(cfg.heartbeat_ns), int(cfg.hb_phase_ns)
    p = np.ascontiguousarray(peer, np.uint32).reshape(-1)
    d = np.ascontiguousarray(t_down_ns, np.uint64).reshape(-1)
    t = np.ascontiguousarray(t_up_ns, np.uint64).reshape(-1)
    if not (p.size == d.size == t.size):
        raise GossipSimError(GS_EINVAL, "peer, t_down_ns and t_up_ns differ in length")
    k = max(p.size, 1)
    po, hf, ht = np.zeros(k, np.uint32), np.zeros(k, np.uint32), np.zeros(k, np.uint32)
    n = u64()
    rc = lib().gs_outage_epochs(ctypes.byref(c), p.size, _ptr(np.resize(p, k), u32), _ptr(np.resize(d, k), u64),
                                _ptr(np.resize(t, k), u64), _ptr(po, u32), _ptr(hf, u32), _ptr(ht, u32), ctypes.byref(n))
    if rc:
        raise GossipSimError(rc, "outage_epochs: t_up_ns < t_down_ns, or an epoch past 2^32 - 2")
    return po[:n.value], hf[:n.value], ht[:n.value]


def write_dials(path, row_ptr, col, flags):
    """One "dialer target" line per entry whose flags bit 0 is set, in row order (gs_write_dials)."""
    row, col, flags = _csr_arrays(row_ptr, col, flags)
    rc = lib().gs_write_dials(str(path).encode(), len(row) - 1, _ptr(row, u64), _ptr(col, u32), _ptr(flags, u8))
    if rc:
        raise GossipSimError(rc, "cannot write the dial list %s" % path)


# Schedule constants of the benchmark workload: Shadow epoch 2000-01-01 plus the
# injector start (shadow/topogen.py:130), 1000 ms spacing and publisher
# (6 + i) mod N with rotation (shadow/README.md:57, run.sh:34-36). The injector
# POSTs over a fresh TCP connection across the 1 ms injector-hub links
# (topogen.py:64-69): the request reaches the node 1.5 round trips = 3 ms after
# the injector's send, and the node stamps tx_time then (main.rs:105-111).
# Heartbeats tick on whole seconds (process start 5 s, topogen.py:106, plus
# libp2p-gossipsub's 5 s heartbeat_initial_delay; hb_phase_ns = 0 is the same
# phase), so a publish lands 3 ms after a heartbeat.
INJECTOR_START_NS = 946684800_000_000_000 + 500_000_000_000
HTTP_TRANSIT_NS = 3_000_000
T0_NS = INJECTOR_START_NS + HTTP_TRANSIT_NS
# Heartbeat 0 when every node starts (Shadow starts processes at 5 s,
# shadow/topogen.py:106): the phase churn runs need.
SHADOW_START_NS = 946684800_000_000_000 + 5_000_000_000
DELAY_NS = 1_000_000_000
PUBLISHER0 = 6


def shard_messages(step, rank, world, batch, peers, msg_size):
    """Message-batch sharding across ranks: global message index
    (step*world + rank)*batch + q; messages are independent given the frozen mesh,
    so ranks share nothing on the data path."""
    idx = (np.uint64(step) * np.uint64(world) + np.uint64(rank)) * np.uint64(batch) + \
        np.arange(batch, dtype=np.uint64)
    t = np.uint64(T0_NS) + idx * np.uint64(DELAY_NS)
    pub = ((np.uint64(PUBLISHER0) + idx) % np.uint64(peers)).astype(np.uint32)
    return t, pub, np.full(batch, msg_size, np.uint32)


class PeerConfig:
    """Knobs of env.rs:14-25 + gossipsub ConfigBuilder (main.rs:223-241)."""

    def __init__(self, **kw):
        """Knobs over the defaults of `node` (rust | go | nim, gs_config_preset; default rust)."""
        self.c = GsConfig()
        node = kw.pop("node", 0)
        node = NODES[node] if isinstance(node, str) else int(node)
        rc = lib().gs_config_preset(ctypes.byref(self.c), node)
        if rc:
            raise GossipSimError(rc, "unknown node flavour %r" % node)
        for k, v in kw.items():
            if k == "muxer" and isinstance(v, str):
                v = MUXERS[v]
            if not hasattr(self.c, k):
                raise AttributeError("unknown knob %s" % k)
            setattr(self.c, k, v)

    @classmethod
    def from_env(cls):
        """get_peer_details (env.rs:27-87): same env names and validation errors."""
        self = cls()
        err = ctypes.create_string_buffer(256)
        rc = lib().gs_config_from_env(ctypes.byref(self.c), err, 256)
        if rc:
            raise GossipSimError(rc, err.value.decode())
        return self

    def __getattr__(self, k):
        if k == "c":
            raise AttributeError(k)
        return getattr(self.c, k)


class Simulator:
    """One context = one HIP device (include/gossipsim.h threading rules)."""

    def __init__(self, cfg=None, **kw):
        self.cfg = cfg if cfg is not None else PeerConfig(**kw)
        self.ctx = ctypes.c_void_p()
        rc = lib().gs_create(ctypes.byref(self.cfg.c), ctypes.byref(self.ctx))
        if rc:
            raise GossipSimError(rc, "gs_create failed")
        self.peers = self.cfg.c.peers
        self._sched = []

    # ---- checkpoint / resume (gs_save_state / gs_load_state) ----
    def save_state(self, path):
        """Links, CSR, mesh, churn mesh state, counters and traffic into `path`."""
        self._check(lib().gs_save_state(self.ctx, str(path).encode()))

    @classmethod
    def load_state(cls, path, device=0):
        """A new simulator on `device` that continues where the saved one stopped."""
        self = cls.__new__(cls)
        self.ctx = ctypes.c_void_p()
        rc = lib().gs_load_state(str(path).encode(), device, ctypes.byref(self.ctx))
        if rc:
            raise GossipSimError(rc, "gs_load_state(%s) failed" % path)
        self.cfg = PeerConfig()
        lib().gs_get_config(self.ctx, ctypes.byref(self.cfg.c))
        self.peers = self.cfg.c.peers
        self._sched = []
        return self

    def _check(self, rc):
        if rc:
            raise GossipSimError(rc, lib().gs_last_error(self.ctx).decode())

    def close(self):
        if self.ctx:
            lib().gs_destroy(self.ctx)
            self.ctx = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- links / topology / mesh ----
    def set_links(self, lat_ns, bw_up, bw_down=None, stage_of_peer=None):
        lat = np.ascontiguousarray(np.asarray(lat_ns, np.uint64).reshape(-1))
        S = int(round(len(lat) ** 0.5))
        up = np.ascontiguousarray(bw_up, np.uint64)
        dn = np.ascontiguousarray(bw_up if bw_down is None else bw_down, np.uint64)
        st = None if stage_of_peer is None else np.ascontiguousarray(stage_of_peer, np.uint8)
        self._check(lib().gs_set_links(self.ctx, S, _ptr(lat, u64), _ptr(up, u64), _ptr(dn, u64),
                                       None if st is None else _ptr(st, u8)))
        self._links = (lat, up, dn, st)

    def set_topogen_links(self, stages=1, min_bw=50, max_bw=50, min_lat=100, max_lat=100,
                          shortest=False):
        lat, bw = topogen_links(stages, min_bw, max_bw, min_lat, max_lat, shortest)
        self.set_links(lat, bw, bw)
        return lat, bw

    def set_shadow_links(self, gml_path, yaml_path, shortest=False):
        """Links straight from a Shadow experiment: the GML graph + shadow.yaml's host placement."""
        lat, up, dn = links_from_gml(gml_path, shortest)
        self.set_links(lat, up, dn, shadow_hosts(yaml_path, self.peers))
        return lat, up, dn

    def connect_gossipsub_peers(self):
        """main.rs:303-389: random ID dialing -> CSR (device resident)."""
        self._check(lib().gs_build_topology(self.ctx))

    build_topology = connect_gossipsub_peers

    def set_topology(self, row_ptr, col, flags):
        """A caller's graph in csr()'s layout in place of the built one (gs_set_topology); of flags
        only bit 0 is read. A refused graph leaves the simulator as it was."""
        row, col, flags = _csr_arrays(row_ptr, col, flags, self.peers)
        self._check(lib().gs_set_topology(self.ctx, _ptr(row, u64), _ptr(col, u32), _ptr(flags, u8)))

    def set_dials(self, dialer, target):
        """The undirected union of the dials dialer[i] -> target[i], in any order (gs_set_topology_dials)."""
        d, t = _dial_arrays(dialer, target)
        pad = 1 if d.size == 0 else 0
        self._check(lib().gs_set_topology_dials(self.ctx, d.size, _ptr(np.resize(d, d.size + pad), u32),
                                                _ptr(np.resize(t, t.size + pad), u32)))

    def graph_info(self):
        n, nnz, md = u32(), u64(), u32()
        self._check(lib().gs_graph_info(self.ctx, ctypes.byref(n), ctypes.byref(nnz),
                                        ctypes.byref(md)))
        return n.value, nnz.value, md.value

    def csr(self):
        _, nnz, _ = self.graph_info()
        row = np.zeros(self.peers + 1, np.uint64)
        col = np.zeros(max(nnz, 1), np.uint32)
        flags = np.zeros(max(nnz, 1), np.uint8)
        self._check(lib().gs_get_csr(self.ctx, _ptr(row, u64), _ptr(col, u32), _ptr(flags, u8)))
        return row, col[:nnz], flags[:nnz]

    def mesh_converge(self, max_heartbeats=400):
        ep = u32()
        self._check(lib().gs_mesh_converge(self.ctx, max_heartbeats, ctypes.byref(ep)))
        return ep.value

    def mesh(self):
        m = np.zeros(self.peers * MESH_W, np.uint32)
        c = np.zeros(self.peers, np.uint8)
        self._check(lib().gs_get_mesh(self.ctx, _ptr(m, u32), _ptr(c, u8)))
        return m.reshape(self.peers, MESH_W), c

    def set_mesh(self, mesh, count=None):
        """A caller's mesh in mesh()'s layout in place of the converged one (gs_set_mesh): ids in any order
        inside a row; without count a row ends at its first 0xFFFFFFFF. A refused mesh leaves the simulator
        as it was."""
        m, c = _mesh_arrays(mesh, count, self.peers)
        self._check(lib().gs_set_mesh(self.ctx, _ptr(m, u32), None if c is None else _ptr(c, u8)))

    def set_mesh_links(self, a, b):
        """The mesh as the set of undirected links {a[i], b[i]}, in any order and either orientation
        (gs_set_mesh_links); no link is the empty mesh."""
        a, b = _dial_arrays(a, b, ("a", "b"))
        pad = 1 if a.size == 0 else 0
        self._check(lib().gs_set_mesh_links(self.ctx, a.size, _ptr(np.resize(a, a.size + pad), u32),
                                            _ptr(np.resize(b, b.size + pad), u32)))

    # ---- a caller's outages in place of the churn draw (gs_set_outages) ----
    def set_outages(self, peer, h_from, h_to):
        """Who is offline when: peer[i] is offline during the heartbeat epochs h_from[i] <= h < h_to[i]
        (OUTAGE_FOREVER: it never returns), in any order; no interval is a churn context in which nobody
        leaves (gs_set_outages). A converge must follow. A refused schedule leaves the simulator as it was."""
        p = np.ascontiguousarray(peer, np.uint32).reshape(-1)
        a = np.ascontiguousarray(h_from, np.uint32).reshape(-1)
        b = np.ascontiguousarray(h_to, np.uint32).reshape(-1)
        if not (p.size == a.size == b.size):
            raise GossipSimError(GS_EINVAL, "peer, h_from and h_to differ in length")
        k = max(p.size, 1)
        self._check(lib().gs_set_outages(self.ctx, p.size, _ptr(np.resize(p, k), u32), _ptr(np.resize(a, k), u32),
                                         _ptr(np.resize(b, k), u32)))

    def clear_outages(self):
        """Back to the churn draw (gs_clear_outages); a converge must follow if a schedule was imported."""
        self._check(lib().gs_clear_outages(self.ctx))

    def offline(self, h_lo, h_hi):
        """bool [h_hi - h_lo + 1, peers]: who is offline in each heartbeat epoch of [h_lo, h_hi], from the draw
        or the imported schedule, as the device's own kernel writes it (gs_get_offline)."""
        E, W = int(h_hi) - int(h_lo) + 1, (self.peers + 63) // 64
        bits = np.zeros(max(E, 1) * W, np.uint64)
        self._check(lib().gs_get_offline(self.ctx, int(h_lo), int(h_hi), _ptr(bits, u64)))
        b = np.unpackbits(bits.reshape(E, W).view(np.uint8), axis=1, bitorder="little")
        return b[:, :self.peers].astype(bool)

    # ---- publish / run ----
    def publish(self, publisher, msg_size, t_pub_ns):
        """POST /publish (main.rs:152-168): queue one injection."""
        if not 0 <= publisher < self.peers:
            raise GossipSimError(-1, "publisher out of range")
        self._sched.append((int(t_pub_ns), int(publisher), int(msg_size)))

    def _schedule(self, schedule):
        """(t, publisher, msg_size[, frags]) arrays or a GsPublish array -> GsPublish array."""
        if schedule is None:
            schedule = (GsPublish * len(self._sched))(*[GsPublish(*r) for r in self._sched])
            self._sched = []
        elif not isinstance(schedule, ctypes.Array):
            t, p, s = schedule[:3]
            fr = schedule[3] if len(schedule) > 3 else 0
            # one vectorised fill of the gs_publish layout (a per-element struct loop cost
            # ~0.7 ms per 1024 messages, most of a config #1 run)
            rec = np.zeros(len(t), np.dtype([("t_pub_ns", "<u8"), ("publisher", "<u4"), ("msg_size", "<u4"),
                                             ("frags", "<u4"), ("reserved", "<u4")]))
            assert rec.dtype.itemsize == ctypes.sizeof(GsPublish)
            rec["t_pub_ns"] = np.asarray(t, np.uint64)
            rec["publisher"] = np.asarray(p, np.uint32)
            rec["msg_size"] = np.asarray(s, np.uint32)
            rec["frags"] = np.asarray(fr, np.uint32)
            schedule = (GsPublish * len(t)).from_buffer_copy(rec.tobytes())
        return schedule

    def run(self, schedule=None, collect=True, summary=False, on_block=None, block_msgs=0,
            want=WANT_T_COMPLETE | WANT_HOPS, on_lat=None):
        """Simulate the queued publishes (or `schedule`); returns t_complete/hops [M, N].

        summary: also return the device's per-message latency reductions
        (gs_msg_summary: delivered, lat_sum_ms, p50/p95/max ms, 100 ms histogram).
        on_block(first_msg, t_complete[n, N], hops[n, N]): stream the results in
        blocks of `block_msgs` messages instead of returning [M, N] arrays;
        `want` (WANT_* bits) selects which of the two it receives (None if not).
        on_lat(first_msg, lat_ms[n, N] uint16): the logged latency stream
        (GS_WANT_LAT_MS: (t_complete - tx_time) // 1e6 as main.rs:93 logs it,
        LAT_NONE where nothing is logged), in the same blocks; it may be used
        alone or beside on_block."""
        schedule = self._schedule(schedule)
        M = len(schedule)
        res = {"schedule": schedule}
        sink = GsResultSink()
        keep = []
        if on_lat is not None:
            def _lcb(user, first, n, peers, lat):
                on_lat(int(first), np.ctypeslib.as_array(lat, (n, peers)))

            lcb = LAT_FN(_lcb)
            keep.append(lcb)
            sink.on_lat = lcb
            sink.block_msgs = block_msgs
            sink.want = WANT_LAT_MS | (want & (WANT_T_COMPLETE | WANT_HOPS) if on_block is not None else 0)
        if on_block is not None:
            N = self.peers

            def _cb(user, first, n, peers, tc, hp):
                a = np.ctypeslib.as_array(tc, (n, peers)) if tc else None
                h = np.ctypeslib.as_array(hp, (n, peers)) if hp else None
                on_block(int(first), a, h)

            cb = BLOCK_FN(_cb)
            keep.append(cb)
            sink.want = want | (WANT_LAT_MS if on_lat is not None else 0)
            sink.on_block = cb
            sink.block_msgs = block_msgs
        elif collect and on_lat is None:
            tc = np.zeros(M * self.peers, np.uint64)
            hops = np.zeros(M * self.peers, np.uint8)
            sink.t_complete_ns = _ptr(tc, u64)
            sink.hops = _ptr(hops, u8)
            res["t_complete"] = tc.reshape(M, self.peers)
            res["hops"] = hops.reshape(M, self.peers)
        if summary:
            sm = (GsMsgSummary * M)()
            sink.summary = ctypes.cast(sm, P(GsMsgSummary))
            keep.append(sm)
        use_sink = on_block is not None or on_lat is not None or collect or summary
        self._check(lib().gs_run(self.ctx, schedule, M, ctypes.byref(sink) if use_sink else None))
        if summary:
            res["summary"] = {
                "delivered": np.array([x.delivered for x in sm], np.uint64),
                "lat_sum_ms": np.array([x.lat_sum_ms for x in sm], np.uint64),
                "p50_ms": np.array([x.p50_ms for x in sm], np.uint32),
                "p95_ms": np.array([x.p95_ms for x in sm], np.uint32),
                "max_ms": np.array([x.max_ms for x in sm], np.uint32),
                "hist": np.array([list(x.hist) for x in sm], np.uint32).reshape(M, HIST_BINS)}
        return res

    def _text_call(self, call, on_text, path):
        """One gs_run_log / gs_format_lat_log call: `call(cb)` with the gs_text_fn for on_text
        or the file at `path` (neither: NULL, which the library refuses). -> lines handed out."""
        total = [0]
        f = open(path, "wb", buffering=0) if path is not None else None
        err = []

        def _tcb(user, first, n, text, nbytes, lines):
            total[0] += lines
            try:
                buf = (ctypes.c_char * nbytes).from_address(text) if nbytes else b""
                if f is not None:
                    f.write(buf)
                if on_text is not None:
                    on_text(int(first), int(n), bytes(buf), int(lines))
            except BaseException as e:  # (no exception crosses the C frames)
                err.append(e)

        cb = TEXT_FN(_tcb) if (on_text is not None or f is not None) else TEXT_FN()
        try:
            self._check(call(cb))
        finally:
            if f is not None:
                f.close()
        if err:
            raise err[0]
        return total[0]

    def run_log(self, schedule=None, on_text=None, path=None, chunk_bytes=0):
        """gs_run_log: simulate like run(), the only output being the arrival log's text,
        formatted on the device: written to `path`, and / or handed to
        on_text(first_msg, n_msgs, text_bytes, lines) chunk by chunk (whole messages,
        at most chunk_bytes each; 0 = the default). The chunks in order are byte for
        byte what LogStream.write_lat writes for run(on_lat=...). -> lines written."""
        schedule = self._schedule(schedule)
        return self._text_call(
            lambda cb: lib().gs_run_log(self.ctx, schedule, len(schedule), cb, None, chunk_bytes), on_text, path)

    def format_lat_log(self, schedule, lat_ms, on_text=None, path=None, chunk_bytes=0):
        """gs_format_lat_log: the same text from a stored latency stream lat_ms[M, N]
        uint16 (LAT_NONE = no line); needs no topology. -> lines written."""
        schedule = self._schedule(schedule)
        lat = np.ascontiguousarray(lat_ms, np.uint16)
        if lat.shape != (len(schedule), self.peers):
            raise GossipSimError(GS_EINVAL, "lat_ms must be [len(schedule), peers]")
        return self._text_call(
            lambda cb: lib().gs_format_lat_log(self.ctx, schedule, len(schedule), _ptr(lat, ctypes.c_uint16), cb, None,
                                               chunk_bytes), on_text, path)

    def log_text_reset(self):
        """Zero the per-peer line counters run_log / format_lat_log carry across calls."""
        self._check(lib().gs_log_text_reset(self.ctx))

    def stats(self):
        st = GsStats()
        self._check(lib().gs_get_stats(self.ctx, ctypes.byref(st)))
        return {n: getattr(st, n) for n, _ in GsStats._fields_}

    def reset_stats(self):
        self._check(lib().gs_reset_stats(self.ctx))

    def set_timing(self, on=True):
        self._check(lib().gs_set_timing(self.ctx, 1 if on else 0))

    def set_traffic(self, on=True):
        """Per-peer send/receive counters of later runs (zeroed now)."""
        self._check(lib().gs_set_traffic(self.ctx, 1 if on else 0))

    def traffic(self):
        """-> uint64 [N, len(TRAFFIC_COLS)] in TRAFFIC_COLS order."""
        tr = np.zeros((self.peers, len(TRAFFIC_COLS)), np.uint64)
        self._check(lib().gs_get_traffic(self.ctx, _ptr(tr, u64)))
        return tr

    def write_node_metrics(self, path):
        """Every peer's Prometheus metrics (rust-test-node/src/metrics.rs names) after traffic runs."""
        write_node_metrics(self.cfg, path, self.csr()[0], self.mesh()[1], self.traffic())

    # ---- mesh events and per-epoch mesh health (gs_set_mesh_events) ----
    def set_mesh_events(self, on=True):
        """While on, every mesh_converge records the per-peer GRAFT / PRUNE / mesh event counts and
        one row of network-wide mesh health per epoch it steps (the later epochs of run's churn
        chain are not counted)."""
        self._check(lib().gs_set_mesh_events(self.ctx, 1 if on else 0))

    def mesh_events(self):
        """-> uint64 [N, len(MESH_EVENT_COLS)] of the last mesh_converge, in MESH_EVENT_COLS order."""
        ev = np.zeros((self.peers, len(MESH_EVENT_COLS)), np.uint64)
        self._check(lib().gs_get_mesh_events(self.ctx, _ptr(ev, u64)))
        return ev

    def mesh_series(self):
        """-> uint64 [epochs + 1, len(MESH_SERIES_COLS)]: row h is the mesh after epoch h."""
        rows = u32()
        self._check(lib().gs_mesh_series_rows(self.ctx, ctypes.byref(rows)))
        se = np.zeros((rows.value, len(MESH_SERIES_COLS)), np.uint64)
        self._check(lib().gs_get_mesh_series(self.ctx, _ptr(se, u64), rows.value))
        return se

    def write_mesh_metrics(self, path):
        """Every peer's go-node GRAFT / PRUNE counters and mesh gauges after a mesh_converge with
        set_mesh_events."""
        write_mesh_metrics(self.cfg, path, self.csr()[0], self.mesh()[1], self.mesh_events())

    def write_mesh_series(self, path):
        write_mesh_series(path, self.mesh_series())

    # ---- per-message cost table (gs_set_message_costs) ----
    def set_message_costs(self, on=True):
        """Every run / run_log call fills a table with one row per message of its schedule (off by
        default; one extra pass per batch). Enabling empties the table."""
        self._check(lib().gs_set_message_costs(self.ctx, 1 if on else 0))

    def message_costs(self):
        """-> uint64 [messages of the last run / run_log call, len(MESSAGE_COST_COLS)], in schedule
        order; no rows before a run."""
        rows = u64(0)
        self._check(lib().gs_message_costs_rows(self.ctx, ctypes.byref(rows)))
        mc = np.zeros((rows.value, len(MESSAGE_COST_COLS)), np.uint64)
        buf = mc if rows.value else np.zeros(1, np.uint64)
        self._check(lib().gs_get_message_costs(self.ctx, _ptr(buf, u64), rows.value))
        return mc

    def write_message_costs(self, path, schedule):
        """The table of the last run / run_log call of `schedule` as TSV, with the wire cost."""
        write_message_costs(self.cfg, path, schedule, self.message_costs())

    # ---- per-peer pubsub event counts (gs_set_pubsub_counts) ----
    def set_pubsub_counts(self, on=True):
        """Per-peer event counters of later runs: fragment copies, IHAVEs and IWANTs sent and
        received, first receipts and duplicates (zeroed now)."""
        self._check(lib().gs_set_pubsub_counts(self.ctx, 1 if on else 0))

    def pubsub_counts(self):
        """-> uint64 [N, len(PUBSUB_COLS)] in PUBSUB_COLS order."""
        pc = np.zeros((self.peers, len(PUBSUB_COLS)), np.uint64)
        self._check(lib().gs_get_pubsub_counts(self.ctx, _ptr(pc, u64)))
        return pc

    def reset_pubsub_counts(self):
        self._check(lib().gs_reset_pubsub_counts(self.ctx))

    def write_pubsub_metrics(self, path):
        """Every peer's go-node pubsub counters and the nim node's chunk counter after runs with
        set_pubsub_counts."""
        write_pubsub_metrics(self.cfg, path, self.pubsub_counts())

    # ---- per-link first deliveries (gs_set_link_deliveries) ----
    def set_link_deliveries(self, on=True):
        """Per-link counters of later runs: the fragments each peer received first over each of its
        connections, split by publisher / mesh neighbour / IWANT answer (zeroed now)."""
        self._check(lib().gs_set_link_deliveries(self.ctx, 1 if on else 0))

    def link_deliveries(self):
        """-> uint64 [nnz, len(LINK_DELIVERY_COLS)] aligned with csr(): entry e of peer u's row counts
        what u received first from col[e]."""
        _, nnz, _ = self.graph_info()
        ld = np.zeros((max(nnz, 1), len(LINK_DELIVERY_COLS)), np.uint64)
        self._check(lib().gs_get_link_deliveries(self.ctx, _ptr(ld, u64)))
        return ld[:nnz]

    def peer_given(self):
        """-> uint64 [N, len(LINK_DELIVERY_COLS)]: the first deliveries each peer made as the sender."""
        pg = np.zeros((self.peers, len(LINK_DELIVERY_COLS)), np.uint64)
        self._check(lib().gs_get_peer_given(self.ctx, _ptr(pg, u64)))
        return pg

    def reset_link_deliveries(self):
        self._check(lib().gs_reset_link_deliveries(self.ctx))

    def write_link_deliveries(self, path):
        """The non-zero link counters after runs with set_link_deliveries, one line per link."""
        row, col, _ = self.csr()
        write_link_deliveries(path, row, col, self.link_deliveries())

    # ---- what each node shows about delay (gs_set_peer_delay) ----
    def _own_rows(self):
        u0, u1 = getattr(self, "part_range", (0, self.peers))
        return u1 - u0

    def set_peer_delay(self, on=True):
        """Per-peer delay accumulators (completed, delay sum, histogram, last delay) of later
        runs, kept on the device whatever the runs' sinks take (zeroed now)."""
        self._check(lib().gs_set_peer_delay(self.ctx, 1 if on else 0))

    def peer_delay(self):
        """-> PEER_DELAY_DTYPE array [own peers]: completed, delay_sum_ms, last_rx_ns, last_ms,
        bucket[13] (not cumulative; bounds DELAY_BOUNDS_MS, the last one above 10000 ms)."""
        out = np.zeros(self._own_rows(), PEER_DELAY_DTYPE)
        self._check(lib().gs_get_peer_delay(self.ctx, _ptr(out, GsPeerDelay)))
        return out

    def reset_peer_delay(self):
        self._check(lib().gs_reset_peer_delay(self.ctx))

    def peer_delay_add_lat(self, schedule, lat_ms):
        """Add a stored latency stream lat_ms[M, own peers] uint16 (LAT_NONE = no observation)
        to the accumulators; needs no topology."""
        schedule = self._schedule(schedule)
        lat = np.ascontiguousarray(lat_ms, np.uint16)
        if lat.shape != (len(schedule), self._own_rows()):
            raise GossipSimError(GS_EINVAL, "lat_ms must be [len(schedule), own peers]")
        self._check(lib().gs_peer_delay_add_lat(self.ctx, schedule, len(schedule), _ptr(lat, ctypes.c_uint16)))

    def write_testnode_metrics(self, path, schedule):
        """Every peer's nim-node metrics (dst_testnode_*) after runs of `schedule` with set_peer_delay."""
        write_testnode_metrics(self.cfg, path, self.csr()[0], self.mesh()[1], self._schedule(schedule),
                               self.peer_delay())

    def open_log(self, path):
        """Streaming arrival log (gs_log_open); feed it with LogStream.write(schedule_rows, t_complete)."""
        return LogStream(self.cfg, path)

    def write_latency_log(self, path, res):
        """Arrival lines as `grep -rne 'milliseconds\\|BW' shadow.data/` prints them."""
        sched = res["schedule"]
        tc = np.ascontiguousarray(res["t_complete"], np.uint64)
        rc = lib().gs_write_node_log(ctypes.byref(self.cfg.c), path.encode(), sched, len(sched), _ptr(tc, u64))
        if rc:
            raise GossipSimError(rc, "gs_write_latency_log failed")

    # ---- peer-partitioned mode (include/gossipsim.h gs_part_*; driver in partition.py) ----
    def set_partition(self, parts, part):
        self._check(lib().gs_set_partition(self.ctx, parts, part))
        self.part_range = (part * self.peers // parts, (part + 1) * self.peers // parts)

    def part_begin(self, schedule):
        schedule = self._schedule(schedule)
        if not hasattr(self, "part_range"):
            self.part_range = (0, self.peers)
        k = u64()
        self._check(lib().gs_part_begin(self.ctx, schedule, len(schedule), ctypes.byref(k)))
        self._part_sched = schedule
        return k.value

    def part_scan(self, bucket_key, dev_ptr, capacity):
        """-> (ok, n, next_key): ok False means `capacity` < n records (state unchanged)."""
        n, m = u64(), u64()
        rc = lib().gs_part_scan(self.ctx, bucket_key, dev_ptr, capacity, ctypes.byref(n), ctypes.byref(m))
        if rc == GS_ERANGE and n.value > capacity:
            return False, n.value, m.value
        self._check(rc)
        return True, n.value, m.value

    def part_relax(self, bucket_key, dev_ptr, n):
        m = u64()
        self._check(lib().gs_part_relax(self.ctx, bucket_key, dev_ptr, n, ctypes.byref(m)))
        return m.value

    def part_finish(self, collect=True):
        """-> {"t_complete", "hops"} [M, own peers] (message-major over this part's peers)."""
        M = len(self._part_sched)
        u0, u1 = self.part_range
        res = {"schedule": self._part_sched, "peer_range": (u0, u1)}
        if collect:
            tc = np.zeros(M * (u1 - u0), np.uint64)
            hops = np.zeros(M * (u1 - u0), np.uint8)
            sink = GsResultSink(_ptr(tc, u64), _ptr(hops, u8))
            self._check(lib().gs_part_finish(self.ctx, ctypes.byref(sink)))
            res["t_complete"] = tc.reshape(M, u1 - u0)
            res["hops"] = hops.reshape(M, u1 - u0)
        else:
            self._check(lib().gs_part_finish(self.ctx, None))
        return res


class LogStream:
    """gs_log_*: the arrival log written block by block (message-major blocks
    from Simulator.run(on_block=...)), identical lines to write_latency_log."""

    def __init__(self, cfg, path):
        self.h = ctypes.c_void_p()
        rc = lib().gs_log_open(ctypes.byref(cfg.c), path.encode(), ctypes.byref(self.h))
        if rc:
            raise GossipSimError(rc, "gs_log_open %s" % path)

    def write(self, sched_rows, t_complete):
        """sched_rows: GsPublish array (or slice) of the block; t_complete [n, N] uint64."""
        tc = np.ascontiguousarray(t_complete, np.uint64)
        n = tc.shape[0]
        rows = (GsPublish * n)(*sched_rows[:n]) if not isinstance(sched_rows, ctypes.Array) else sched_rows
        rc = lib().gs_log_write(self.h, rows, n, _ptr(tc, u64))
        if rc:
            raise GossipSimError(rc, "gs_log_write failed")

    def write_lat(self, sched_rows, lat_ms):
        """The same lines from a block of the u16 latency stream (run(on_lat=...))."""
        lat = np.ascontiguousarray(lat_ms, np.uint16)
        n = lat.shape[0]
        rows = (GsPublish * n)(*sched_rows[:n]) if not isinstance(sched_rows, ctypes.Array) else sched_rows
        rc = lib().gs_log_write_lat(self.h, rows, n, _ptr(lat, ctypes.c_uint16))
        if rc:
            raise GossipSimError(rc, "gs_log_write_lat failed")

    def close(self):
        if self.h:
            rc = lib().gs_log_close(self.h)
            self.h = ctypes.c_void_p()
            if rc:
                raise GossipSimError(rc, "gs_log_close failed")


class Comm:
    """gs_comm: the parts of a peer-partitioned run (include/gossipsim.h).

    Comm(local_parts=P)                     P parts driven by this process
    Comm(nranks, rank, uid, device)         one rank of an RCCL communicator;
                                            uid = Comm.get_id() on rank 0,
                                            handed to the others out of band"""

    def __init__(self, nranks=1, rank=0, uid=None, device=0, local_parts=None, transport=None):
        self.h = ctypes.c_void_p()
        if transport is not None:  # the caller's collectives (gs_comm_init_ops)
            self._ops = _ops_of(transport, nranks)
            rc = lib().gs_comm_init_ops(nranks, rank, ctypes.byref(self._ops), device, ctypes.byref(self.h))
            self.parts, self.local, self.rank = nranks, False, rank
        elif local_parts is not None:
            rc = lib().gs_comm_init_local(local_parts, ctypes.byref(self.h))
            self.parts, self.local = local_parts, True
        else:
            if uid is None:
                uid = Comm.get_id()
            rc = lib().gs_comm_init(nranks, rank, uid, device, ctypes.byref(self.h))
            self.parts, self.local, self.rank = nranks, False, rank
        if rc:
            raise GossipSimError(rc, "gs_comm_init failed")

    def check(self):
        """gs_comm_check: one all-gather and one exchange of known bytes through the transport."""
        rc = lib().gs_comm_check(self.h)
        if rc:
            raise GossipSimError(rc, "gs_comm_check: the transport delivered wrong data")

    @staticmethod
    def get_id():
        buf = ctypes.create_string_buffer(COMM_ID_BYTES)
        rc = lib().gs_comm_get_id(buf)
        if rc:
            raise GossipSimError(rc, "gs_comm_get_id failed (RCCL not loadable?)")
        return buf.raw

    def run_partitioned(self, sims, schedule, collect=True, summary=False, on_lat=None, block_msgs=0, want=None):
        """gs_run_partitioned over this process's Simulators (local: one per part,
        in part order; RCCL: this rank's). -> per part {"t_complete", "hops",
        "peer_range"} [M, own peers] (collect) or None.
        on_lat(part, first_msg, lat_ms[n, own peers] uint16): every part's logged
        latency stream (GS_WANT_LAT_MS) in blocks of block_msgs messages, alone
        (collect=False) or beside the arrays; the parts' blocks side by side are
        Simulator.run's on_lat stream. summary: also "summary" per part (the
        gs_msg_summary rows as a ctypes array). want: the sinks' want word, when
        it is not to follow from on_lat (tests of the sink rules)."""
        schedule = sims[0]._schedule(schedule)
        M = len(schedule)
        arr = (ctypes.c_void_p * len(sims))(*[s.ctx for s in sims])
        sinks, keep, out = (GsResultSink * len(sims))(), [], []
        err = []
        for i, sim in enumerate(sims):
            part = i if self.local else self.rank
            u0, u1 = part * sim.peers // self.parts, (part + 1) * sim.peers // self.parts
            sim.part_range = (u0, u1)
            if on_lat is not None:
                def _lcb(user, first, n, peers, lat, part=part):
                    try:
                        on_lat(part, int(first), np.ctypeslib.as_array(lat, (n, peers)))
                    except BaseException as e:  # (no exception crosses the C frames)
                        err.append(e)

                lcb = LAT_FN(_lcb)
                keep.append(lcb)
                sinks[i].on_lat = lcb
                sinks[i].block_msgs = block_msgs
                sinks[i].want = WANT_LAT_MS
            if want is not None:
                sinks[i].want = want
            res = {"peer_range": (u0, u1)}
            out.append(res)
            if summary:
                sm = (GsMsgSummary * M)()
                sinks[i].summary = ctypes.cast(sm, P(GsMsgSummary))
                res["summary"] = sm
            if collect:
                tc = np.zeros(M * (u1 - u0), np.uint64)
                hp = np.zeros(M * (u1 - u0), np.uint8)
                keep += [tc, hp]
                sinks[i].t_complete_ns = _ptr(tc, u64)
                sinks[i].hops = _ptr(hp, u8)
                res.update(t_complete=tc.reshape(M, u1 - u0), hops=hp.reshape(M, u1 - u0))
        use_sinks = collect or summary or on_lat is not None or want is not None
        rc = lib().gs_run_partitioned(arr, len(sims), self.h, schedule, M, sinks if use_sinks else None)
        if rc:
            raise GossipSimError(rc, lib().gs_last_error(sims[0].ctx).decode())
        if err:
            raise err[0]
        return out if collect or summary else None

    def run_partitioned_log(self, sims, schedule, on_text=None, paths=None, chunk_bytes=0):
        """gs_run_partitioned_log: run_partitioned whose only output is the arrival log's
        text, each part formatting its own peers' lines on its device: written to
        paths[i] (one file per part), and / or handed to
        on_text(part, first_msg, n_msgs, text_bytes, lines) chunk by chunk. A part's
        chunks in order are Simulator.run_log's text with only that part's peers' lines
        kept. With neither, the library gets NULL and refuses. -> lines per part."""
        schedule = sims[0]._schedule(schedule)
        arr = (ctypes.c_void_p * len(sims))(*[s.ctx for s in sims])
        parts = [i if self.local else self.rank for i in range(len(sims))]
        for sim, part in zip(sims, parts):
            sim.part_range = (part * sim.peers // self.parts, (part + 1) * sim.peers // self.parts)
        users = (ctypes.c_void_p * len(sims))(*range(len(sims)))  # user = the context's index
        files = [open(p, "wb", buffering=0) for p in paths] if paths is not None else None
        total, err = [0] * len(sims), []

        def _tcb(user, first, n, text, nbytes, lines):
            i = int(user or 0)
            total[i] += lines
            try:
                buf = (ctypes.c_char * nbytes).from_address(text) if nbytes else b""
                if files is not None:
                    files[i].write(buf)
                if on_text is not None:
                    on_text(parts[i], int(first), int(n), bytes(buf), int(lines))
            except BaseException as e:  # (no exception crosses the C frames)
                err.append(e)

        cb = TEXT_FN(_tcb) if (on_text is not None or files is not None) else TEXT_FN()
        try:
            rc = lib().gs_run_partitioned_log(arr, len(sims), self.h, schedule, len(schedule), cb, users, chunk_bytes)
        finally:
            for f in files or []:
                f.close()
        if rc:
            raise GossipSimError(rc, lib().gs_last_error(sims[0].ctx).decode())
        if err:
            raise err[0]
        return total

    def close(self):
        if self.h:
            lib().gs_comm_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _ops_of(transport, nranks):
    """gs_comm_ops over a transport object with allgather(np.uint64[n]) -> [nranks, n]
    and exchange(list of send bytes, list of recv sizes) -> list of recv bytes.
    An exception in the transport becomes a non-zero return (the call fails)."""
    def allgather(_user, mine, n, out):
        try:
            a = np.ctypeslib.as_array(mine, (n,)).copy() if n else np.zeros(0, np.uint64)
            got = np.ascontiguousarray(transport.allgather(a), np.uint64).reshape(-1)
            if got.size != nranks * n:
                return 2
            ctypes.memmove(out, got.ctypes.data, got.nbytes)
            return 0
        except Exception:  # noqa: BLE001  (reported as the call's failure)
            import traceback
            traceback.print_exc()
            return 1

    def exchange(_user, send, send_bytes, recv, recv_bytes):
        try:
            sends = [ctypes.string_at(send[p], send_bytes[p]) if send_bytes[p] else b"" for p in range(nranks)]
            sizes = [int(recv_bytes[p]) for p in range(nranks)]
            got = transport.exchange(sends, sizes)
            for p in range(nranks):
                if len(got[p]) != sizes[p]:
                    return 2
                if sizes[p]:
                    ctypes.memmove(recv[p], bytes(got[p]), sizes[p])
            return 0
        except Exception:  # noqa: BLE001
            import traceback
            traceback.print_exc()
            return 1

    ops = GsCommOps()
    ops._cb = (ALLGATHER_FN(allgather), EXCHANGE_FN(exchange))  # kept alive with the struct
    ops.allgather, ops.exchange = ops._cb
    return ops


class TorchDistTransport:
    """gs_comm_ops over torch.distributed (any backend with all_gather and
    point-to-point send / recv, e.g. gloo on CPU tensors): one rank per process,
    launched by torchrun or multiprocessing, the rendezvous the caller's."""

    def __init__(self, group=None):
        import torch
        import torch.distributed as dist
        self.torch, self.dist, self.group = torch, dist, group
        self.rank = dist.get_rank(group)
        self.size = dist.get_world_size(group)

    def allgather(self, mine):
        t = self.torch.from_numpy(mine.view(np.int64).copy())
        out = [self.torch.empty_like(t) for _ in range(self.size)]
        self.dist.all_gather(out, t, group=self.group)
        return np.stack([o.numpy().view(np.uint64) for o in out])

    def exchange(self, sends, sizes):
        torch, dist = self.torch, self.dist
        reqs, recvs = [], [b""] * self.size
        bufs = {}
        for p in range(self.size):
            if p == self.rank:
                continue
            if sizes[p]:
                bufs[p] = torch.empty(sizes[p], dtype=torch.uint8)
                reqs.append(dist.irecv(bufs[p], src=p, group=self.group))
            if len(sends[p]):
                reqs.append(dist.isend(torch.frombuffer(bytearray(sends[p]), dtype=torch.uint8), dst=p,
                                       group=self.group))
        for r in reqs:
            r.wait()
        for p, b in bufs.items():
            recvs[p] = b.numpy().tobytes()
        return recvs
