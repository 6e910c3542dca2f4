// gs_peerdelay.h — what each node shows about delay: the per-peer series
// of nim-test-node/gossipsub-queues (main.nim:25-78,147-154) — completed messages, the delay
// sum, the delay histogram and the last delay — reduced on the device from the
// message-major logged latencies lat_t[B][un] that every completion path ends with.
// Included by gs_relax.hip.
//
// The context's rows are the peers [u0, u0 + un): all of them, or a part's range. Only the
// row index matters here. An observation is an arrival-log line: a (row, message) whose
// latency is not GS_LAT_NONE.
//
// Accumulators: PD_COLS u64 columns [col][un] (structure of arrays, lane = row, so the
// read-modify-write is coalesced), carried across batches and calls:
//   PD_SUM      sum of the delays in ms
//   PD_LAST_RX  t_pub_ns + ms * 10^6 of the last observation (0: none)
//   PD_LAST_MS  its ms
//   PD_BUCKET+i observations of bucket i (not cumulative); the count is their sum
// "Last" is the observation with the largest (t_pub + ms * 10^6, t_pub): two observations
// with the same pair have the same ms, so the result depends on no processing order
// (class order, message shards, calls). The carried pair is (PD_LAST_RX, PD_LAST_RX -
// PD_LAST_MS * 10^6), and (0, 0) where there is none: an observation equal to it changes nothing.
//   k_peer_delay  lane = row: the columns read once, a loop over the batch's messages
//                 (PD_AHEAD loads issued before the first use, t_pub wave-uniform), the
//                 columns stored once. No atomic: a pure function of the input.
#pragma once

constexpr uint32_t PD_SUM = 0, PD_LAST_RX = 1, PD_LAST_MS = 2, PD_BUCKET = 3;
constexpr uint32_t PD_COLS = PD_BUCKET + GS_DELAY_BUCKETS + 1;
constexpr uint32_t PD_AHEAD = 8;   // messages whose loads are in flight together
constexpr uint32_t PD_WAVES = 4;
static_assert(PD_COLS == 16, "the accumulators are 128 bytes per row");
static_assert(GS_DELAY_BUCKETS == 12, "k_peer_delay's bounds are the 12 of main.nim:59");

// cum += ms <= bound, one register per bound (no array indexed by the bucket)
#define PD_BOUNDS(X) X(0, 1u) X(1, 5u) X(2, 10u) X(3, 25u) X(4, 50u) X(5, 100u) X(6, 250u) X(7, 500u) \
                     X(8, 1000u) X(9, 2500u) X(10, 5000u) X(11, 10000u)

__global__ __launch_bounds__(PD_WAVES * 64) void k_peer_delay(const uint16_t* __restrict__ lat_t,
                                                              const uint64_t* __restrict__ tpub,
                                                              uint64_t* __restrict__ acc, uint32_t un, uint32_t B) {
  const uint32_t u = blockIdx.x * (PD_WAVES * 64) + threadIdx.x;
  if (u >= un) return;
  uint64_t sum = acc[(size_t)PD_SUM * un + u];
  uint64_t brx = acc[(size_t)PD_LAST_RX * un + u];
  uint32_t bms = (uint32_t)acc[(size_t)PD_LAST_MS * un + u];
  uint64_t btp = brx - (uint64_t)bms * 1000000ull;
  uint32_t n = 0;
#define PD_DECL(i, b) uint32_t c##i = 0;
  PD_BOUNDS(PD_DECL)
#undef PD_DECL
  const uint16_t* p = lat_t + u;
  for (uint32_t m0 = 0; m0 < B; m0 += PD_AHEAD) {
    uint32_t v[PD_AHEAD];
#pragma unroll
    for (uint32_t k = 0; k < PD_AHEAD; k++) v[k] = m0 + k < B ? p[(size_t)(m0 + k) * un] : GS_LAT_NONE;
#pragma unroll
    for (uint32_t k = 0; k < PD_AHEAD; k++) {
      const uint32_t ms = v[k];
      if (ms == GS_LAT_NONE) continue;
      const uint64_t tp = tpub[m0 + k];  // (m0 + k < B: the tail's values are GS_LAT_NONE)
      const uint64_t rx = tp + (uint64_t)ms * 1000000ull;
      n++;
      sum += ms;
#define PD_CMP(i, b) c##i += ms <= b;
      PD_BOUNDS(PD_CMP)
#undef PD_CMP
      if (rx > brx || (rx == brx && tp > btp)) {
        brx = rx;
        btp = tp;
        bms = ms;
      }
    }
  }
  acc[(size_t)PD_SUM * un + u] = sum;
  acc[(size_t)PD_LAST_RX * un + u] = brx;
  acc[(size_t)PD_LAST_MS * un + u] = bms;
  uint32_t prev = 0;
#define PD_OUT(i, b)                                     \
  acc[(size_t)(PD_BUCKET + i) * un + u] += c##i - prev;  \
  prev = c##i;
  PD_BOUNDS(PD_OUT)
#undef PD_OUT
  acc[(size_t)(PD_BUCKET + GS_DELAY_BUCKETS) * un + u] += n - prev;
}

// The rows the context's accumulators cover: all peers, or its partition's range.
static uint32_t pd_rows(const Ctx& c) { return c.part_un ? c.part_un : c.cfg.peers; }

// The accumulators of the context's un rows: zeroed when the switch goes on, and again when
// the rows are another range than they were kept for (part_set forgets them when the
// partition changes, as the line counters).
static void pd_ensure(Ctx& c, uint32_t un) {
  if (c.d_pdelay.p && c.pdelay_n == un) return;
  c.d_pdelay.alloc((size_t)PD_COLS * un);
  GS_HIP(hipMemsetAsync(c.d_pdelay.p, 0, (size_t)PD_COLS * un * 8, c.stream));
  c.pdelay_n = un;
}

// A finished batch's observations, enqueued: lat_t[B][un] message-major and the B publish
// times on the device, both ready on the context's stream. Once per batch, before
// anything of it is handed out.
static void pd_accumulate(Ctx& c, const uint16_t* lat_t, const uint64_t* d_tpub, uint32_t B, uint32_t un) {
  if (!c.pdelay || !B || !un) return;
  pd_ensure(c, un);
  k_peer_delay<<<(un + PD_WAVES * 64 - 1) / (PD_WAVES * 64), PD_WAVES * 64, 0, c.stream>>>(lat_t, d_tpub, c.d_pdelay.p,
                                                                                             un, B);
  GS_HIP(hipGetLastError());
}

void peer_delay_set(Ctx& c, bool on) {
  c.pdelay = on;
  if (!on) return;
  c.pdelay_n = 0;
  pd_ensure(c, pd_rows(c));
  GS_HIP(hipStreamSynchronize(c.stream));
}

void peer_delay_reset(Ctx& c) {
  if (!c.pdelay) return;
  c.pdelay_n = 0;
  pd_ensure(c, pd_rows(c));
  GS_HIP(hipStreamSynchronize(c.stream));
}

// gs_get_peer_delay: the columns out, the array of structs assembled on the host.
void peer_delay_get(Ctx& c, gs_peer_delay* out) {
  const uint32_t un = pd_rows(c);
  pd_ensure(c, un);
  std::vector<uint64_t> h((size_t)PD_COLS * un);
  GS_HIP(hipMemcpyAsync(h.data(), c.d_pdelay.p, h.size() * 8, hipMemcpyDeviceToHost, c.stream));
  GS_HIP(hipStreamSynchronize(c.stream));
  for (uint32_t u = 0; u < un; u++) {
    gs_peer_delay& o = out[u];
    o.completed = 0;
    for (uint32_t i = 0; i <= GS_DELAY_BUCKETS; i++) {
      o.bucket[i] = h[(size_t)(PD_BUCKET + i) * un + u];
      o.completed += o.bucket[i];
    }
    o.delay_sum_ms = h[(size_t)PD_SUM * un + u];
    o.last_rx_ns = h[(size_t)PD_LAST_RX * un + u];
    o.last_ms = (uint32_t)h[(size_t)PD_LAST_MS * un + u];
    o.reserved = 0;
  }
}

// gs_peer_delay_add_lat: a caller's message-major lat_ms[n_msgs][own rows], in pieces of at
// most cfg.batch messages.
void peer_delay_add_lat(Ctx& c, const gs_publish* sched, uint64_t n_msgs, const uint16_t* lat_ms) {
  const uint32_t un = pd_rows(c);
  const uint64_t piece = c.cfg.batch;
  c.d_lat_t.alloc((size_t)piece * un);
  c.d_lr_tpub.alloc(piece);
  std::vector<uint64_t> tp(piece);
  for (uint64_t m0 = 0; m0 < n_msgs; m0 += piece) {
    const uint32_t B = (uint32_t)std::min<uint64_t>(piece, n_msgs - m0);
    for (uint32_t m = 0; m < B; m++) tp[m] = sched[m0 + m].t_pub_ns;
    GS_HIP(hipMemcpyAsync(c.d_lr_tpub.p, tp.data(), (size_t)B * 8, hipMemcpyHostToDevice, c.stream));
    GS_HIP(hipMemcpyAsync(c.d_lat_t.p, lat_ms + m0 * un, (size_t)B * un * 2, hipMemcpyHostToDevice, c.stream));
    pd_accumulate(c, c.d_lat_t.p, c.d_lr_tpub.p, B, un);
    GS_HIP(hipStreamSynchronize(c.stream));  // (tp is written again)
  }
}
