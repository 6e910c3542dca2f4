// gs_msgcost.h — per-message cost table of a gs_run / gs_run_log call (gs_set_message_costs,
// DESIGN.md §2.17): for every message of the call's schedule the fragment copies sent and
// arrived, first receipts, duplicates, IHAVE and IWANT RPCs and completions.
// Included by gs_relax.hip beside gs_pubsub.h.
//
// The events are the sends, arrivals and losses gs_traffic.h enumerates from the final keys;
// this header adds no send rule. MsgAcc is that enumeration's third accumulation policy,
// k_msgcost_pub / k_msgcost_fwd<FP> / k_msgcost_gossip<FP> its kernels. Every lane of the
// bodies works for exactly one message m (sends_pub: the block's; sends_fwd, sends_gossip:
// its key's), so:
//  * a lane keeps its counts in registers, the arrivals of its own sends included:
//    data_acked, ihave_acked and iwant_rx are called exactly where a send of the lane (or the
//    IWANT it answers) arrived, so no receiver's row is touched and data_arrive / ihave_arrive
//    are empty (data_rx names the same arrival as the data_acked beside it and stays empty);
//  * a block reduces by message in an LDS table [rows][MC_DEV] of u32 (ds_add, no return),
//    and at its end adds every non-zero cell to the global table with one atomic;
//  * above the rows that fit MC_LDS_BYTES (GS_MSGCOST_LDS_ROWS), or where a
//    block's lanes could overflow a u32 cell, the lanes add to the global table directly;
//  * first receipts: the lanes of a wave that work for the same message are consecutive (a
//    fragment group, or the whole wave when L == FP); each such run is counted with one
//    ballot and popcount and its first lane adds the sum (MsgAcc::first);
//  * duplicates are DATA_RX - FIRST, derived at read-out and never counted.
// Integer adds commute, so the counts depend on no processing order.
#pragma once

// The device's columns of one row (GS_MC_DUP is derived) and where each lands in the table.
enum : uint32_t { MC_TX = 0, MC_RX, MC_FIRST, MC_IHTX, MC_IHRX, MC_IW, MC_DELIV, MC_DEV };
static_assert(GS_MC_DATA_TX == MC_TX && GS_MC_DATA_RX == MC_RX && GS_MC_FIRST == MC_FIRST && GS_MC_DUP == 3 &&
                  GS_MC_IHAVE_TX == MC_IHTX + 1 && GS_MC_IHAVE_RX == MC_IHRX + 1 && GS_MC_IWANT == MC_IW + 1 &&
                  GS_MC_DELIVERED == MC_DELIV + 1 && GS_MC_COLS == MC_DEV + 1,
              "the device's columns are the table's without GS_MC_DUP");
__host__ __device__ constexpr uint32_t mc_col(uint32_t d) { return d + (d >= GS_MC_DUP ? 1u : 0u); }
constexpr uint32_t MC_LDS_BYTES = 48u << 10;
constexpr uint32_t MC_LDS_ROWS = MC_LDS_BYTES / (MC_DEV * 4);  // 1755

struct MsgArgs {
  uint64_t* costs;  // the batch's rows of the table, [B][GS_MC_COLS] (GS_MC_DUP stays 0 on the device)
  uint32_t Fe, flood, collide;
  uint32_t rows;    // rows of the block's LDS table; 0: the lanes add to `costs` directly
};

__device__ __forceinline__ uint32_t* mc_tab() {
  extern __shared__ uint32_t mc_lds[];
  return mc_lds;
}

// ONE: the block works for one message (sends_pub), row 0 of its table is that message's.
template <bool ONE>
__device__ __forceinline__ void mc_add(const MsgArgs& t, uint32_t m, uint32_t d, uint32_t n) {
  if (t.rows) atomicAdd(&mc_tab()[(ONE ? 0u : m) * MC_DEV + d], n);
  else atomicAdd((unsigned long long*)&t.costs[(size_t)m * GS_MC_COLS + mc_col(d)], (unsigned long long)n);
}

__device__ __forceinline__ void mc_begin(const MsgArgs& t) {
  if (!t.rows) return;
  uint32_t* tab = mc_tab();
  for (uint32_t i = threadIdx.x; i < t.rows * MC_DEV; i += TB) tab[i] = 0;
  __syncthreads();
}

// The block's table to the global one; m0: the message of row 0.
__device__ __forceinline__ void mc_end(const MsgArgs& t, uint32_t m0) {
  if (!t.rows) return;
  __syncthreads();
  const uint32_t* tab = mc_tab();
  for (uint32_t i = threadIdx.x; i < t.rows * MC_DEV; i += TB) {
    const uint32_t v = tab[i];
    if (v) atomicAdd((unsigned long long*)&t.costs[(size_t)(m0 + i / MC_DEV) * GS_MC_COLS + mc_col(i % MC_DEV)],
                     (unsigned long long)v);
  }
}

// One lane's counts of its message in registers. (A lane sends at most MESH_W copies as a
// forwarder, Fe * degree / TB + 1 as a publisher's thread, and history_gossip * degree IHAVEs
// with as many answers: far inside u32.)
template <bool ONE>
struct MsgLane {
  uint32_t tx = 0, rx = 0, ihtx = 0, ihrx = 0, iw = 0;
  __device__ void data_tx(const MsgArgs&, uint64_t n) { tx += (uint32_t)n; }
  __device__ void data_acked(const MsgArgs&, uint64_t n) { rx += (uint32_t)n; }
  __device__ void data_rx(const MsgArgs&) {}
  __device__ void ihave_tx(const MsgArgs&) { ihtx++; }
  __device__ void ihave_acked(const MsgArgs&) { ihrx++; }
  __device__ void iwant_tx(const MsgArgs&) {}
  __device__ void iwant_rx(const MsgArgs&) { iw++; }
  __device__ void iwant_acked(const MsgArgs&) {}
  __device__ void flush(const MsgArgs& t, uint32_t, uint32_t m) const {
    if (tx) mc_add<ONE>(t, m, MC_TX, tx);
    if (rx) mc_add<ONE>(t, m, MC_RX, rx);
    if (ihtx) mc_add<ONE>(t, m, MC_IHTX, ihtx);
    if (ihrx) mc_add<ONE>(t, m, MC_IHRX, ihrx);
    if (iw) mc_add<ONE>(t, m, MC_IW, iw);
  }
};

template <bool ONE>
struct MsgAccT {
  using Args = MsgArgs;
  using Peer = MsgLane<ONE>;
  static constexpr bool completions = true;
  static __device__ __forceinline__ void data_arrive(const Args&, uint32_t) {}
  static __device__ __forceinline__ void ihave_arrive(const Args&, uint32_t) {}
  static __device__ __forceinline__ void published(const Args&, uint32_t) {}
  static __device__ __forceinline__ void completed(const Args& t, uint32_t, uint32_t m) { mc_add<ONE>(t, m, MC_DELIV, 1); }
  // f: this lane's key is a first receipt. Called by every lane of the wave. A lane whose
  // left neighbour works for another message (or lane 0) leads a run of lanes of one
  // message, up to the next leader; it adds the run's first receipts. (An invalid lane's m
  // is past the batch's and its f is false: its run adds nothing.)
  static __device__ __forceinline__ void first(const Args& t, bool f, bool, uint32_t, uint64_t, uint32_t, int lane,
                                               uint32_t m) {
    const uint64_t got = __ballot(f);
    const uint32_t left = __shfl_up(m, 1);
    const bool lead = lane == 0 || left != m;
    const uint64_t leads = __ballot(lead);
    if (!lead) return;
    const uint64_t above = lane == 63 ? 0ull : leads & (~0ull << (lane + 1));
    const uint32_t hi = above ? (uint32_t)__ffsll((unsigned long long)above) - 1 : 64;
    const uint64_t below_hi = hi == 64 ? ~0ull : (1ull << hi) - 1;
    const uint32_t n = (uint32_t)__popcll(got & below_hi & ~((1ull << lane) - 1));
    if (n) mc_add<ONE>(t, m, MC_FIRST, n);
  }
};
using MsgAcc = MsgAccT<false>;

__global__ __launch_bounds__(TB) void k_msgcost_pub(RelaxArgs a, MsgArgs t) {
  mc_begin(t);
  sends_pub<MsgAccT<true>>(a, t);
  mc_end(t, blockIdx.x);
}
template <int FP>
__global__ __launch_bounds__(TB) void k_msgcost_fwd(RelaxArgs a, MsgArgs t) {
  mc_begin(t);
  sends_fwd<MsgAcc, FP>(a, t);
  mc_end(t, 0);
}
template <int FP>
__global__ __launch_bounds__(TB) void k_msgcost_gossip(RelaxArgs a, MsgArgs t) {
  mc_begin(t);
  sends_gossip<MsgAcc, FP>(a, t);
  mc_end(t, 0);
}

// The costs of the batch just finished (keys final, before the next reset); its messages are
// rows [i0, i0 + B) of the call's table, in the order the run driver takes them (mc_perm).
static void launch_msgcost(Ctx& c, const Batch& b, uint64_t i0) {
  if (c.keys_none) c.fail(GS_EINVAL, "internal: the message cost pass after a no-log list pass");
  if (i0 + b.B > c.mc_rows) c.fail(GS_EINVAL, "internal: a batch past the message cost table");
  const bool gossip = c.cfg.lazy_gossip != 0;
  const RelaxArgs ra = relax_args(c, b, gossip);
  MsgArgs ma{};
  ma.costs = c.d_msgcost.p + i0 * GS_MC_COLS;
  ma.Fe = b.Fe;
  ma.flood = c.cfg.flood_publish;
  ma.collide = b.collide ? 1 : 0;
  hipStream_t s = c.stream;
  const unsigned grid = keys_pass_grid(c, ra.total);
  // An LDS cell is a u32. A block runs ceil(total / (grid * TB)) rounds of TB lanes, and one
  // lane adds at most `per_lane` to a column of its message (MESH_W forwards and their
  // arrivals; history_gossip heartbeats times at most max_degree targets, each one IHAVE, one
  // IWANT and one answer; 1 first receipt; 1 completion). Their product bounds every cell of
  // the block's table; where it does not fit 32 bits the direct form runs.
  const uint64_t rounds = (ra.total + (uint64_t)grid * TB - 1) / ((uint64_t)grid * TB);
  const uint64_t per_lane = std::max<uint64_t>(MESH_W, (uint64_t)c.cfg.history_gossip * std::max<uint32_t>(1, c.max_degree));
  const uint32_t cap = (uint32_t)std::min<long>(MC_LDS_ROWS, std::max<long>(0, env_int("GS_MSGCOST_LDS_ROWS", MC_LDS_ROWS)));
  const bool lds = b.B <= cap && rounds * TB * per_lane < (1ull << 32);
  // the publisher's block: Fe * degree sends in all (degree <= MAX_DEG), one row
  MsgArgs mp = ma;
  mp.rows = cap ? 1 : 0;
  ma.rows = lds ? b.B : 0;
  k_msgcost_pub<<<b.B, TB, mp.rows * MC_DEV * 4, s>>>(ra, mp);
  const size_t shm = (size_t)ma.rows * MC_DEV * 4;
  with_fp(b.FP, [&](auto fp) {
    k_msgcost_fwd<fp.value><<<grid, TB, shm, s>>>(ra, ma);
    if (gossip && c.cfg.history_gossip) k_msgcost_gossip<fp.value><<<grid, TB, shm, s>>>(ra, ma);
  });
  GS_HIP(hipGetLastError());
}

void msgcost_set(Ctx& c, bool on) {
  c.msgcost = on;
  c.mc_rows = 0;
  c.mc_perm.clear();
}

// A gs_run / gs_run_log call of n messages begins: its table, zeroed.
void msgcost_begin(Ctx& c, uint64_t n) {
  if (!c.msgcost) return;
  c.mc_perm.clear();
  c.mc_rows = n;
  if (!n) return;
  c.d_msgcost.alloc((size_t)n * GS_MC_COLS);
  GS_HIP(hipMemsetAsync(c.d_msgcost.p, 0, (size_t)n * GS_MC_COLS * 8, c.stream));
}

// gs_get_message_costs: the rows back in schedule order (row i of the device table is the
// schedule's message mc_perm[i] where class_plan regrouped the call), duplicates derived.
void msgcost_get(Ctx& c, uint64_t* out) {
  const size_t n = c.mc_rows;
  if (!n) return;
  std::vector<uint64_t> tmp(c.mc_perm.empty() ? 0 : n * GS_MC_COLS);
  uint64_t* dst = c.mc_perm.empty() ? out : tmp.data();
  GS_HIP(hipMemcpyAsync(dst, c.d_msgcost.p, n * GS_MC_COLS * 8, hipMemcpyDeviceToHost, c.stream));
  GS_HIP(hipStreamSynchronize(c.stream));
  for (size_t i = 0; i < n && !c.mc_perm.empty(); i++)
    memcpy(out + (size_t)c.mc_perm[i] * GS_MC_COLS, tmp.data() + i * GS_MC_COLS, GS_MC_COLS * 8);
  for (size_t i = 0; i < n; i++) {
    uint64_t* r = out + i * GS_MC_COLS;
    r[GS_MC_DUP] = r[GS_MC_DATA_RX] - r[GS_MC_FIRST];
  }
}
