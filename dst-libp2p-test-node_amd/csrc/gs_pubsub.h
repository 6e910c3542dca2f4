// gs_pubsub.h — per-peer pubsub event counts of a finished batch (gs_set_pubsub_counts,
// DESIGN.md §2.14): what go-test-node/metrics.go:84-220 counts per node — messages,
// IHAVEs and IWANTs sent and received, first receipts and duplicates — and the nim node's
// dst_testnode_received_chunks_total (main.nim:37-41).
// Included by gs_relax.hip after launch_traffic.
//
// The events are exactly the sends, arrivals and losses gs_traffic.h enumerates from the
// final keys; this header adds no send rule. PubsubAcc is that enumeration's second
// accumulation policy, k_pubsub_pub / k_pubsub_fwd<FP> / k_pubsub_gossip<FP> its kernels:
//  * a sender's counts stay in registers and are flushed once per lane, one atomic per
//    non-zero column (PeerEvents::flush);
//  * an arrival at another peer is one atomic on that peer's rx column;
//  * a first receipt is the lane's own finite key at a non-publisher: the lanes of a wave
//    that share a row (L consecutive lanes) are counted with one ballot and popcount, and
//    the row's first lane in the wave adds the sum (PubsubAcc::first);
//  * duplicates are MSG_RX - FIRST, derived at read-out and never counted.
// Integer adds commute, so the counts depend on no processing order.
#pragma once

struct PubsubArgs {
  uint64_t* counts;  // [N][GS_PUBSUB_COLS] (the GS_PS_DUP column stays 0 on the device)
  uint32_t Fe, flood, collide;
};

// Event counts of one peer in registers.
struct PeerEvents {
  uint32_t mtx = 0, mrx = 0, ihtx = 0, ihrx = 0, iwtx = 0, iwrx = 0;
  __device__ void data_tx(const PubsubArgs&, uint64_t n) { mtx += (uint32_t)n; }
  __device__ void data_acked(const PubsubArgs&, uint64_t) {}
  __device__ void data_rx(const PubsubArgs&) { mrx++; }
  __device__ void ihave_tx(const PubsubArgs&) { ihtx++; }
  __device__ void ihave_acked(const PubsubArgs&) {}
  __device__ void iwant_tx(const PubsubArgs&) { iwtx++; }
  __device__ void iwant_rx(const PubsubArgs&) { iwrx++; }
  __device__ void iwant_acked(const PubsubArgs&) {}
  __device__ void flush(const PubsubArgs& t, uint32_t x, uint32_t) const {
    unsigned long long* r = (unsigned long long*)(t.counts + (size_t)x * GS_PUBSUB_COLS);
    if (mtx) atomicAdd(&r[GS_PS_MSG_TX], (unsigned long long)mtx);
    if (mrx) atomicAdd(&r[GS_PS_MSG_RX], (unsigned long long)mrx);
    if (ihtx) atomicAdd(&r[GS_PS_IHAVE_TX], (unsigned long long)ihtx);
    if (ihrx) atomicAdd(&r[GS_PS_IHAVE_RX], (unsigned long long)ihrx);
    if (iwtx) atomicAdd(&r[GS_PS_IWANT_TX], (unsigned long long)iwtx);
    if (iwrx) atomicAdd(&r[GS_PS_IWANT_RX], (unsigned long long)iwrx);
  }
};

struct PubsubAcc {
  using Args = PubsubArgs;
  using Peer = PeerEvents;
  static constexpr bool completions = false;
  static __device__ __forceinline__ void add(const Args& t, uint32_t x, int col, uint32_t n) {
    atomicAdd((unsigned long long*)&t.counts[(size_t)x * GS_PUBSUB_COLS + col], (unsigned long long)n);
  }
  static __device__ __forceinline__ void data_arrive(const Args& t, uint32_t x) { add(t, x, GS_PS_MSG_RX, 1); }
  static __device__ __forceinline__ void ihave_arrive(const Args& t, uint32_t x) { add(t, x, GS_PS_IHAVE_RX, 1); }
  static __device__ __forceinline__ void published(const Args&, uint32_t) {}
  static __device__ __forceinline__ void completed(const Args&, uint32_t, uint32_t) {}
  // f: this lane's key is a first receipt (finite, not the publisher's, fl < Fe). Called by
  // every lane of the wave. Row u's lanes of the wave at `base` are [lo, hi); lane lo adds
  // the row's count.
  static __device__ __forceinline__ void first(const Args& t, bool f, bool valid, uint32_t u, uint64_t base,
                                               uint32_t L, int lane, uint32_t) {
    const uint64_t got = __ballot(f);
    if (!valid) return;
    const uint64_t r0 = (uint64_t)u * L, r1 = r0 + L;  // (r1 > base: the lane's gid is in [r0, r1))
    const uint32_t lo = r0 > base ? (uint32_t)(r0 - base) : 0;
    const uint32_t hi = r1 - base < 64 ? (uint32_t)(r1 - base) : 64;
    if ((uint32_t)lane != lo) return;
    const uint64_t below_hi = hi == 64 ? ~0ull : (1ull << hi) - 1;
    const uint32_t n = (uint32_t)__popcll(got & below_hi & ~((1ull << lo) - 1));
    if (n) add(t, u, GS_PS_FIRST, n);
  }
};

__global__ __launch_bounds__(TB) void k_pubsub_pub(RelaxArgs a, PubsubArgs t) { sends_pub<PubsubAcc>(a, t); }
template <int FP>
__global__ __launch_bounds__(TB) void k_pubsub_fwd(RelaxArgs a, PubsubArgs t) { sends_fwd<PubsubAcc, FP>(a, t); }
template <int FP>
__global__ __launch_bounds__(TB) void k_pubsub_gossip(RelaxArgs a, PubsubArgs t) { sends_gossip<PubsubAcc, FP>(a, t); }

// The event counts of the batch just finished (keys final, before the next reset).
static void launch_pubsub(Ctx& c, const Batch& b) {
  if (c.keys_none) c.fail(GS_EINVAL, "internal: the pubsub count pass after a no-log list pass");
  const bool gossip = c.cfg.lazy_gossip != 0;
  const RelaxArgs ra = relax_args(c, b, gossip);
  PubsubArgs pa{};
  pa.counts = c.d_pubsub.p;
  pa.Fe = b.Fe;
  pa.flood = c.cfg.flood_publish;
  pa.collide = b.collide ? 1 : 0;
  hipStream_t s = c.stream;
  const unsigned grid = keys_pass_grid(c, ra.total);
  k_pubsub_pub<<<b.B, TB, 0, s>>>(ra, pa);
  with_fp(b.FP, [&](auto fp) {
    k_pubsub_fwd<fp.value><<<grid, TB, 0, s>>>(ra, pa);
    if (gossip && c.cfg.history_gossip) k_pubsub_gossip<fp.value><<<grid, TB, 0, s>>>(ra, pa);
  });
  GS_HIP(hipGetLastError());
}

static void pubsub_zero(Ctx& c) {
  GS_HIP(hipMemsetAsync(c.d_pubsub.p, 0, (size_t)c.cfg.peers * GS_PUBSUB_COLS * 8, c.stream));
}

void pubsub_set(Ctx& c, bool on) {
  c.pubsub = on;
  if (!on) return;
  c.d_pubsub.alloc((size_t)c.cfg.peers * GS_PUBSUB_COLS);
  pubsub_zero(c);
  GS_HIP(hipStreamSynchronize(c.stream));
}

// (enqueued: gs_reset_stats synchronises once for all its counters)
void pubsub_reset(Ctx& c) {
  if (c.pubsub) pubsub_zero(c);
}

// gs_get_pubsub_counts: the counters out, duplicates derived.
void pubsub_get(Ctx& c, uint64_t* out) {
  const size_t N = c.cfg.peers;
  GS_HIP(hipMemcpyAsync(out, c.d_pubsub.p, N * GS_PUBSUB_COLS * 8, hipMemcpyDeviceToHost, c.stream));
  GS_HIP(hipStreamSynchronize(c.stream));
  for (size_t u = 0; u < N; u++) {
    uint64_t* r = out + u * GS_PUBSUB_COLS;
    r[GS_PS_DUP] = r[GS_PS_MSG_RX] - r[GS_PS_FIRST];
  }
}
