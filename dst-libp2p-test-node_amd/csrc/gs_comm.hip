// gs_comm.hip — the multi-GPU communicator (include/gossipsim.h gs_comm_*) and
// the entry points of the library-driven peer-partitioned run
// (gs_run_partitioned, gs_run_partitioned_log), whose driver is
// gs_prun.h. One process drives one GPU (RCCL over xGMI, or the caller's
// gs_comm_ops transport), or one thread drives several loop-back parts
// (device copies; the tests run P parts on one GPU). A batch takes one of
// three paths:
//   list pass — every part runs gs_run's window passes over its own rows; per
//     pass the parts agree on the pass control and exchange the records (§5);
//   push — per bucket: scan and count per destination part, the count matrix,
//     an all-to-all-v of the records, relax, MIN of the next bucket key (§5);
//   message-sharded — part p simulates its share of the batch's messages over
//     all peers, then one all-to-all transposes the results (§5.3).
#include <dlfcn.h>
#include <string.h>
#include <rccl/rccl.h>  // types and enums only: the functions are resolved with dlsym

#include <algorithm>
#include <new>
#include <optional>
#include <vector>

#include "gs_internal.h"
#include "gs_layout.h"

struct gs_ctx : gs::Ctx {};

namespace gs {
namespace {

// RCCL entry points, loaded on first use so that libgossipsim loads (and
// single-GPU runs work) where no RCCL is installed.
struct Rccl {
  void* h = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*GroupStart)() = nullptr;
  ncclResult_t (*GroupEnd)() = nullptr;
  const char* (*ErrorString)(ncclResult_t) = nullptr;
};

Rccl* rccl() {
  static Rccl r;
  static bool tried = false;
  if (!tried) {
    tried = true;
    const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    for (const char* n : names)
      if ((r.h = dlopen(n, RTLD_NOW | RTLD_LOCAL))) break;
    if (r.h) {
#define GS_SYM(f, name) r.f = (decltype(r.f))dlsym(r.h, name)
      GS_SYM(GetUniqueId, "ncclGetUniqueId");
      GS_SYM(CommInitRank, "ncclCommInitRank");
      GS_SYM(CommDestroy, "ncclCommDestroy");
      GS_SYM(AllReduce, "ncclAllReduce");
      GS_SYM(AllGather, "ncclAllGather");
      GS_SYM(Send, "ncclSend");
      GS_SYM(Recv, "ncclRecv");
      GS_SYM(GroupStart, "ncclGroupStart");
      GS_SYM(GroupEnd, "ncclGroupEnd");
      GS_SYM(ErrorString, "ncclGetErrorString");
#undef GS_SYM
      if (!r.GetUniqueId || !r.CommInitRank || !r.CommDestroy || !r.AllReduce || !r.AllGather || !r.Send ||
          !r.Recv || !r.GroupStart || !r.GroupEnd || !r.ErrorString) {
        dlclose(r.h);
        r.h = nullptr;
      }
    }
  }
  return r.h ? &r : nullptr;
}

#define GS_NCCL(call)                                                                               \
  do {                                                                                              \
    ncclResult_t r_ = (call);                                                                       \
    if (r_ != ncclSuccess) throw gs::Error(GS_EDEVICE, std::string(#call) + ": " + rccl()->ErrorString(r_)); \
  } while (0)

}  // namespace
}  // namespace gs

using namespace gs;

struct gs_comm {
  uint32_t local = 0;    // 1: in-process parts, 0: RCCL or the caller's transport (ops)
  uint32_t nranks = 1, rank = 0;
  int32_t device = 0;
  ncclComm_t nc = nullptr;
  bool has_ops = false;  // gs_comm_init_ops: collectives staged through host memory into ops
  gs_comm_ops ops{};
  // ranks: [parts][parts] count matrix, 1 flag word (PRun::agree), [parts][4] gathered control (PRun::gather)
  uint64_t* d_scratch = nullptr;
  static size_t scratch_bytes(uint32_t P) { return ((size_t)P * P + 1 + 4 * (size_t)P) * 8; }
  uint64_t* scratch_mat() const { return d_scratch; }
  uint64_t* scratch_flag() const { return d_scratch + (size_t)nranks * nranks; }
  uint64_t* scratch_ctl() const { return scratch_flag() + 1; }
  // ops backend: the send / recv calls of the open group, exchanged at its end
  struct Xfer {
    const void* src;
    void* dst;
    uint64_t bytes;
    int peer;
  };
  std::vector<Xfer> xs, xr;
  hipStream_t xstream = nullptr;
};

namespace gs {
namespace {

// The rank collectives of the partitioned protocols (RCCL's names and
// arguments, less the communicator): RCCL over xGMI, or through the caller's
// gs_comm_ops on host copies — a D2H copy, the callback, an H2D copy — in the
// same order and sizes on every rank.
size_t type_bytes(ncclDataType_t t) {
  switch (t) {
    case ncclInt8: case ncclUint8: return 1;
    case ncclInt32: case ncclUint32: case ncclFloat32: return 4;
    default: return 8;  // ncclUint64 (the only wide type used)
  }
}
void ops_fail(int rc, const char* what) {
  if (rc) throw Error(GS_EDEVICE, std::string("gs_comm_ops.") + what + " returned " + std::to_string(rc));
}
// every rank's n u64 words of the device buffer send -> recv[rank * n + k]
void coll_AllGather(gs_comm* cm, const void* send, void* recv, size_t n, ncclDataType_t t, hipStream_t s) {
  if (!cm->has_ops) {
    GS_NCCL(rccl()->AllGather(send, recv, n, t, cm->nc, s));
    return;
  }
  if (t != ncclUint64) throw Error(GS_EINVAL, "internal: ops all-gather of u64 words only");
  std::vector<uint64_t> mine(n), all((size_t)cm->nranks * n);
  GS_HIP(hipMemcpyAsync(mine.data(), send, n * 8, hipMemcpyDeviceToHost, s));
  GS_HIP(hipStreamSynchronize(s));
  ops_fail(cm->ops.allgather(cm->ops.user, mine.data(), n, all.data()), "allgather");
  GS_HIP(hipMemcpyAsync(recv, all.data(), all.size() * 8, hipMemcpyHostToDevice, s));
  GS_HIP(hipStreamSynchronize(s));
}
// in-place MIN / MAX of n u64 words over the ranks (ops: reduced from an all-gather)
void coll_AllReduce(gs_comm* cm, const void* send, void* recv, size_t n, ncclDataType_t t, ncclRedOp_t op,
                    hipStream_t s) {
  if (!cm->has_ops) {
    GS_NCCL(rccl()->AllReduce(send, recv, n, t, op, cm->nc, s));
    return;
  }
  if (t != ncclUint64 || (op != ncclMin && op != ncclMax)) throw Error(GS_EINVAL, "internal: ops all-reduce");
  std::vector<uint64_t> mine(n), all((size_t)cm->nranks * n);
  GS_HIP(hipMemcpyAsync(mine.data(), send, n * 8, hipMemcpyDeviceToHost, s));
  GS_HIP(hipStreamSynchronize(s));
  ops_fail(cm->ops.allgather(cm->ops.user, mine.data(), n, all.data()), "allgather");
  for (size_t k = 0; k < n; k++) {
    uint64_t v = all[k];
    for (uint32_t p = 1; p < cm->nranks; p++)
      v = op == ncclMin ? std::min(v, all[(size_t)p * n + k]) : std::max(v, all[(size_t)p * n + k]);
    mine[k] = v;
  }
  GS_HIP(hipMemcpyAsync(recv, mine.data(), n * 8, hipMemcpyHostToDevice, s));
  GS_HIP(hipStreamSynchronize(s));
}
void coll_group_start(gs_comm* cm) {
  if (!cm->has_ops) {
    GS_NCCL(rccl()->GroupStart());
    return;
  }
  cm->xs.clear();
  cm->xr.clear();
  cm->xstream = nullptr;
}
void coll_Send(gs_comm* cm, const void* buf, size_t count, ncclDataType_t t, int peer, hipStream_t s) {
  if (!cm->has_ops) {
    GS_NCCL(rccl()->Send(buf, count, t, peer, cm->nc, s));
    return;
  }
  cm->xs.push_back({buf, nullptr, (uint64_t)count * type_bytes(t), peer});
  cm->xstream = s;
}
void coll_Recv(gs_comm* cm, void* buf, size_t count, ncclDataType_t t, int peer, hipStream_t s) {
  if (!cm->has_ops) {
    GS_NCCL(rccl()->Recv(buf, count, t, peer, cm->nc, s));
    return;
  }
  cm->xr.push_back({nullptr, buf, (uint64_t)count * type_bytes(t), peer});
  cm->xstream = s;
}
// ops: the group's sends concatenated per peer in call order (the receiver's
// recvs from that peer split the bytes in its own call order, as RCCL matches
// a group's point-to-point calls per peer), one exchange, the recvs scattered
void coll_group_end(gs_comm* cm) {
  if (!cm->has_ops) {
    GS_NCCL(rccl()->GroupEnd());
    return;
  }
  const uint32_t P = cm->nranks;
  std::vector<std::vector<uint8_t>> sb(P), rb(P);
  std::vector<uint64_t> sn(P, 0), rn(P, 0);
  for (const auto& x : cm->xs) sn[x.peer] += x.bytes;
  for (const auto& x : cm->xr) rn[x.peer] += x.bytes;
  hipStream_t s = cm->xstream;
  for (uint32_t p = 0; p < P; p++) {
    sb[p].resize(sn[p]);
    rb[p].resize(rn[p]);
  }
  std::vector<uint64_t> at(P, 0);
  for (const auto& x : cm->xs) {
    if (x.bytes) GS_HIP(hipMemcpyAsync(sb[x.peer].data() + at[x.peer], x.src, x.bytes, hipMemcpyDeviceToHost, s));
    at[x.peer] += x.bytes;
  }
  if (s) GS_HIP(hipStreamSynchronize(s));
  // a rank's own transfers (the push protocol sends a part's records to itself)
  // stay here: the transport sees 0 bytes for the own entry
  const uint32_t me = cm->rank;
  if (sn[me] != rn[me]) throw Error(GS_EINVAL, "internal: own send and receive differ in the ops exchange");
  if (rn[me]) memcpy(rb[me].data(), sb[me].data(), rn[me]);
  std::vector<uint64_t> sx = sn, rx = rn;
  sx[me] = rx[me] = 0;
  std::vector<const void*> sp(P);
  std::vector<void*> rp(P);
  for (uint32_t p = 0; p < P; p++) {
    sp[p] = sb[p].data();
    rp[p] = rb[p].data();
  }
  ops_fail(cm->ops.exchange(cm->ops.user, sp.data(), sx.data(), rp.data(), rx.data()), "exchange");
  std::fill(at.begin(), at.end(), 0);
  for (const auto& x : cm->xr) {
    if (x.bytes) GS_HIP(hipMemcpyAsync(x.dst, rb[x.peer].data() + at[x.peer], x.bytes, hipMemcpyHostToDevice, s));
    at[x.peer] += x.bytes;
  }
  if (s) GS_HIP(hipStreamSynchronize(s));
  cm->xs.clear();
  cm->xr.clear();
}

}  // namespace
}  // namespace gs

extern "C" gs_status gs_comm_get_id(gs_comm_id* out) {
  static_assert(sizeof(gs_comm_id) == sizeof(ncclUniqueId), "gs_comm_id must hold an ncclUniqueId");
  if (!out) return GS_EINVAL;
  Rccl* r = rccl();
  if (!r) return GS_EUNSUPPORTED;
  ncclUniqueId id;
  if (r->GetUniqueId(&id) != ncclSuccess) return GS_EDEVICE;
  memcpy(out, &id, sizeof id);
  return GS_OK;
}

extern "C" gs_status gs_comm_init(uint32_t nranks, uint32_t rank, const gs_comm_id* id, int32_t device,
                                  gs_comm** out) {
  if (!out || !id || nranks < 1 || nranks > 64 || rank >= nranks) return GS_EINVAL;
  *out = nullptr;
  Rccl* r = rccl();
  if (!r) return GS_EUNSUPPORTED;
  if (hipSetDevice(device) != hipSuccess) return GS_EDEVICE;
  gs_comm* c = new (std::nothrow) gs_comm();
  if (!c) return GS_ENOMEM;
  c->nranks = nranks;
  c->rank = rank;
  c->device = device;
  ncclUniqueId nid;
  memcpy(&nid, id, sizeof nid);
  if (r->CommInitRank(&c->nc, (int)nranks, nid, (int)rank) != ncclSuccess ||
      hipMalloc((void**)&c->d_scratch, gs_comm::scratch_bytes(nranks)) != hipSuccess) {
    if (c->nc) r->CommDestroy(c->nc);
    delete c;
    return GS_EDEVICE;
  }
  *out = c;
  return GS_OK;
}

extern "C" gs_status gs_comm_init_local(uint32_t nparts, gs_comm** out) {
  if (!out || nparts < 1 || nparts > 64) return GS_EINVAL;
  gs_comm* c = new (std::nothrow) gs_comm();
  if (!c) return GS_ENOMEM;
  c->local = 1;
  c->nranks = nparts;
  *out = c;
  return GS_OK;
}

extern "C" gs_status gs_comm_init_ops(uint32_t nranks, uint32_t rank, const gs_comm_ops* ops, int32_t device,
                                      gs_comm** out) {
  if (!out || !ops || !ops->allgather || !ops->exchange || nranks < 1 || nranks > 64 || rank >= nranks)
    return GS_EINVAL;
  *out = nullptr;
  gs_comm* c = new (std::nothrow) gs_comm();
  if (!c) return GS_ENOMEM;
  c->has_ops = true;
  c->ops = *ops;
  c->nranks = nranks;
  c->rank = rank;
  c->device = device;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) == hipSuccess && device >= 0 && device < ndev) {  // (gs_comm_check needs none)
    if (hipSetDevice(device) != hipSuccess ||
        hipMalloc((void**)&c->d_scratch, gs_comm::scratch_bytes(nranks)) != hipSuccess) {
      delete c;
      return GS_EDEVICE;
    }
  }
  *out = c;
  return GS_OK;
}

// Host-only check of the caller's transport: the words and bytes every rank
// must see, from a position hash (sender, receiver, byte index).
extern "C" gs_status gs_comm_check(gs_comm* c) {
  if (!c) return GS_EINVAL;
  if (!c->has_ops) return GS_OK;
  const uint32_t P = c->nranks, me = c->rank;
  const uint64_t mine[2] = {me, P};
  std::vector<uint64_t> all(2 * (size_t)P);
  if (c->ops.allgather(c->ops.user, mine, 2, all.data())) return GS_EDEVICE;
  for (uint32_t p = 0; p < P; p++)
    if (all[2 * p] != p || all[2 * p + 1] != P) return GS_EDEVICE;
  auto len = [](uint32_t s, uint32_t d) { return s == d ? 0ull : 1ull + 977ull * (s + 3ull * d); };
  auto byte = [](uint32_t s, uint32_t d, uint64_t i) {
    return (uint8_t)(((i + 1) * 0x9E3779B97F4A7C15ull ^ ((uint64_t)s << 40) ^ ((uint64_t)d << 20)) >> 56);
  };
  std::vector<std::vector<uint8_t>> sb(P), rb(P);
  std::vector<uint64_t> sn(P), rn(P);
  std::vector<const void*> sp(P);
  std::vector<void*> rp(P);
  for (uint32_t p = 0; p < P; p++) {
    sn[p] = len(me, p);
    rn[p] = len(p, me);
    sb[p].resize(sn[p]);
    for (uint64_t i = 0; i < sn[p]; i++) sb[p][i] = byte(me, p, i);
    rb[p].assign(rn[p], 0);
    sp[p] = sb[p].data();
    rp[p] = rb[p].data();
  }
  if (c->ops.exchange(c->ops.user, sp.data(), sn.data(), rp.data(), rn.data())) return GS_EDEVICE;
  for (uint32_t p = 0; p < P; p++)
    for (uint64_t i = 0; i < rn[p]; i++)
      if (rb[p][i] != byte(p, me, i)) return GS_EDEVICE;
  return GS_OK;
}

extern "C" gs_status gs_comm_destroy(gs_comm* c) {
  if (!c) return GS_EINVAL;
  if (c->nc) {
    (void)hipSetDevice(c->device);
    rccl()->CommDestroy(c->nc);
  }
  if (c->d_scratch) (void)hipFree(c->d_scratch);
  delete c;
  return GS_OK;
}

#include "gs_prun.h"

extern "C" gs_status gs_run_partitioned(gs_ctx* const* ctxs, uint32_t nctx, gs_comm* comm, const gs_publish* sched,
                                        uint64_t n_msgs, const gs_result_sink* sinks) {
  if (!ctxs || !nctx || !comm || (!sched && n_msgs)) return GS_EINVAL;
  for (uint32_t i = 0; i < nctx; i++)
    if (!ctxs[i]) return GS_EINVAL;
  return run_partitioned(ctxs, nctx, comm, sched, n_msgs, sinks);
}

// The arrival log's text of a partitioned run (gs_logtext.h): gs_run_partitioned with a
// latency-only sink per part, whose on_lat is never called: while a context's text callback
// is set, its batches' latencies go to the formatter over the part's own peer range.
extern "C" gs_status gs_run_partitioned_log(gs_ctx* const* ctxs, uint32_t nctx, gs_comm* comm, const gs_publish* sched,
                                            uint64_t n_msgs, gs_text_fn on_text, void* const* users,
                                            uint64_t chunk_bytes) {
  if (!ctxs || !nctx || !comm || (!sched && n_msgs)) return GS_EINVAL;
  for (uint32_t i = 0; i < nctx; i++)
    if (!ctxs[i]) return GS_EINVAL;
  if (!on_text) {
    ctxs[0]->last_error = "gs_run_partitioned_log: on_text is NULL";
    return GS_EINVAL;
  }
  if (nctx > 64) return GS_EINVAL;  // (a communicator has at most 64 parts)
  gs_result_sink sinks[64] = {};
  std::optional<TextCall> calls[64];
  for (uint32_t i = 0; i < nctx; i++) {
    sinks[i].want = GS_WANT_LAT_MS;
    sinks[i].on_lat = text_sink_unused;
    calls[i].emplace(ctxs[i], sched, on_text, users ? users[i] : nullptr, chunk_bytes);
  }
  return run_partitioned(ctxs, nctx, comm, sched, n_msgs, sinks);
}
