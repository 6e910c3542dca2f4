// gs_relax.hip — eager forwarding + seen-cache + uplink FIFO + reassembly as
// Delta-stepping frontier relaxation over a batch of concurrent messages.
//
// Reference behaviour replaced: publish_new_message
// (rust-test-node/src/main.rs:101-143) flood-publishes F fragments; each peer's
// first receipt of a fragment is forwarded to mesh \ {src, publisher}
// (libp2p-gossipsub forward_msg, upstream) through the peer's uplink FIFO;
// create_message_handler (main.rs:79-99) completes on the F-th fragment.
//
// Layout (HBM): keys[u][m][f] (u64, peer-major, f padded to FP = 2^k) holds
// key = t_rel_ns << (6+sb) | hops << sb | src; min key wins, so the seen-cache
// IS the key array and ties break on (time, hops, src) deterministically.
// Every relaxation adds >= Delta = min latency + min serialisation, so all
// keys inside the current bucket [lo, lo+Delta) are final: one launch per
// non-empty bucket scans the keys (coalesced), forwards the bucket's arrivals
// with 64-bit atomicMin pushes into the same (m,f) slot of the targets, and
// reduces the next pending key to pick the next bucket on the device
// (triple-buffered ctrl words; no host round trip per bucket).
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <exception>

#include "gs_internal.h"
#include "gs_layout.h"

namespace gs {
namespace {

constexpr int TB = 256;

#include "gs_relax_kernel.h"
#include "gs_pull_kernel.h"
#include "gs_traffic.h"


struct SeedArgs {
  uint64_t* keys;
  const uint64_t* row;
  const uint32_t* col;
  const uint32_t* mesh;
  const uint32_t* pub;
  const uint8_t* stage;
  const uint32_t* tables;
  uint64_t* ctrl;      // min seeded key (push: the first bucket; pull: slot 2's min)
  uint32_t* chunkmin;  // pull path: [N][16] min pending key hi-word per 64-lane chunk (push path: nullptr)
  // list pull path: seeds appended to a list instead of the dense keys (k_lseed
  // files them into the candidate lists); the publishers' own lanes go to k_lpub
  uint64_t* skey;
  uint32_t* slane;     // (row << 11) | lane
  uint32_t* scnt;
  uint64_t* counters;
  uint64_t tmax;
  uint32_t L, FP, Fe, S, sb, tshift, flood;
  uint32_t u0, un;  // keys held for peers [u0, u0 + un) (the whole graph unless partitioned)
  uint32_t soff;    // batch slice (run_slices): its rows are soff + peer (list seeds and key sources)
  // churn: see RelaxArgs
  const uint32_t* ring_mesh;
  const uint64_t* ring_off;
  const uint64_t* q0;
  const uint64_t* r0;
  uint64_t hb_ns;
  uint32_t churn, ring_R, w64, horizon, N;
};

// publish_new_message (main.rs:101-143): self key at the publisher and the
// flood (or mesh) sends of every fragment through its uplink FIFO. Only
// targets inside [u0, u0 + un) are written; the publisher's owner counts R.
__global__ __launch_bounds__(TB) void k_seed(SeedArgs a) {
  __shared__ uint32_t live[MAX_DEG];  // churn: the connections online at t_pub, ascending
  __shared__ uint32_t wcnt[TB / 64];
  const uint32_t m = blockIdx.x, p = a.pub[m], sp = a.stage[p], S = a.S;
  const uint64_t ser = a.tables[S * S + sp];
  // churn: an offline publisher publishes nothing (the injector's POST finds no node)
  if (a.churn && ep_off(a, a.q0[m], p)) return;
  const bool own_pub = p - a.u0 < a.un;
  if (own_pub && threadIdx.x < a.Fe && !a.skey) a.keys[(size_t)(p - a.u0) * a.L + (size_t)m * a.FP + threadIdx.x] = (uint64_t)p;
  uint32_t deg;
  const uint32_t* tg;
  bool packed;
  if (a.flood) { deg = (uint32_t)(a.row[p + 1] - a.row[p]); tg = a.col + a.row[p]; packed = false; }
  else {
    tg = a.churn ? ep_mesh(a, a.q0[m], p) : a.mesh + (size_t)p * MESH_W;
    deg = 0;
    while (deg < MESH_W && tg[deg] != EMPTY) deg++;
    packed = true;
  }
  if (a.churn && a.flood) {  // compact the online connections in id order (deg <= MAX_DEG = TB)
    const uint32_t j = threadIdx.x;
    const bool on = j < deg && !ep_off(a, a.q0[m], tg[j]);
    const uint64_t bm = __ballot(on);
    if ((threadIdx.x & 63) == 0) wcnt[threadIdx.x >> 6] = (uint32_t)__popcll(bm);
    __syncthreads();
    uint32_t base = 0;
    for (uint32_t q = 0; q < (threadIdx.x >> 6); q++) base += wcnt[q];
    if (on) live[base + (uint32_t)__popcll(bm & ((1ull << (threadIdx.x & 63)) - 1))] = tg[j];
    uint32_t tot = 0;
    for (uint32_t q = 0; q < TB / 64; q++) tot += wcnt[q];
    __syncthreads();
    deg = tot;
    tg = live;
  }
  uint64_t nmin = INF64;
  uint32_t err = 0;
  const uint32_t total = a.Fe * deg;
  for (uint32_t i = threadIdx.x; i < total; i += TB) {
    const uint32_t f = i / deg, j = i % deg;
    const uint32_t w = packed ? (tg[j] & 0xFFFFFFu) : tg[j];
    const uint32_t sw = a.stage[w];
    const uint64_t sd = a.tables[S * S + S + sw];
    const uint64_t arr = ((uint64_t)f * deg + j + 1) * ser + a.tables[sp * S + sw] + (sd > ser ? sd - ser : 0);
    if (arr > a.tmax) err |= ERR_TIME;
    const uint64_t nk = (arr << a.tshift) | (1ull << a.sb) | (p + a.soff);
    if (w - a.u0 >= a.un) continue;
    if (a.churn && ev_lost(a, m, arr, w)) continue;
    if (a.skey) {  // one send per (target, fragment): no duplicates to reduce
      const uint32_t q = atomicAdd(a.scnt, 1u);
      a.skey[q] = nk;
      a.slane[q] = ((w - a.u0 + a.soff) << 11) | (m * a.FP + f);
      nmin = nk < nmin ? nk : nmin;
      continue;
    }
    atomicMin((unsigned long long*)&a.keys[(size_t)(w - a.u0) * a.L + (size_t)m * a.FP + f], (unsigned long long)nk);
    if (a.chunkmin)
      atomicMin(&a.chunkmin[(size_t)(w - a.u0) * PULL_CH + ((m * a.FP + f) >> 6)], (uint32_t)(nk >> 32));
    nmin = nk < nmin ? nk : nmin;
  }
  nmin = wave_min(nmin);
  for (int off = 32; off > 0; off >>= 1) err |= __shfl_xor(err, off);
  if ((threadIdx.x & 63) == 0) {
    if (nmin != INF64) atomicMin((unsigned long long*)a.ctrl, (unsigned long long)nmin);
    if (err) atomicOr((unsigned*)&a.counters[C_ERR], err);
  }
  if (threadIdx.x == 0 && own_pub) atomicAdd((unsigned long long*)&a.counters[C_R], (unsigned long long)total);
}

struct CompArgs {
  const uint64_t* keys;
  const uint32_t* pub;
  const uint64_t* tpub;
  uint64_t* tc;     // [N][B] peer-major, like the keys
  uint8_t* hops;    // [N][B]
  uint16_t* lat;    // [N][B] logged latency in ms (GS_WANT_LAT_MS), else nullptr
  uint64_t* counters;
  uint64_t* mstat;  // [B][MS_COLS] per-message reductions (k_complete / k_pct)
  uint32_t* hist;   // [B][GS_HIST_BINS] 100 ms latency bins (summary requested), else nullptr
  const uint32_t* pbin;  // k_pct: [B][2] the 100 ms bins holding p50 / p95
  uint32_t* fine;   // k_pct: [B][2][GS_HIST_MS] 1 ms counts inside those bins
  uint32_t N, B, F, FP, L, sb, tshift, collide, self_log, MT;
  uint32_t u0;  // global id of keys row 0
};

// per-message columns of mstat
enum : uint32_t { MS_TMAX = 0, MS_UNDEL = 1, MS_LOGGED = 2, MS_LSUM = 3, MS_LMAX = 4, MS_COLS = 8 };

// Lane -> (message, row offset) of the message-tiled completion kernels: a
// wave covers MT consecutive messages of 64/MT consecutive rows (MT = 64 for
// batches of >= 64 messages), so every load is a contiguous piece of a row
// and every lane keeps one message for the whole kernel (per-message
// reductions stay in registers). grid = (row chunks, message tiles).
struct MsgTile {
  uint32_t m, uoff, rstep;
  bool mv;
  __device__ MsgTile(uint32_t MT, uint32_t B) {
    const uint32_t lane = threadIdx.x & 63;
    m = blockIdx.y * MT + lane % MT;
    uoff = (threadIdx.x >> 6) * (64 / MT) + lane / MT;
    rstep = gridDim.x * (TB / 64) * (64 / MT);
    mv = m < B;
  }
};

// Sum per-lane values of the block's lanes that hold the same message and add
// them to the message's global counter (LDS staging, one atomic per message).
template <bool MAX>
__device__ __forceinline__ void msg_flush(uint64_t v, uint64_t* lds, uint32_t MT, uint32_t m0, uint32_t B,
                                          uint64_t* dst, uint32_t col) {
  __syncthreads();
  lds[threadIdx.x] = v;
  __syncthreads();
  if (threadIdx.x < MT && m0 + threadIdx.x < B) {
    uint64_t t = 0;
    for (uint32_t i = threadIdx.x; i < TB; i += MT) t = MAX ? (lds[i] > t ? lds[i] : t) : t + lds[i];
    if (t) {
      unsigned long long* p = (unsigned long long*)&dst[(size_t)(m0 + threadIdx.x) * MS_COLS + col];
      if (MAX) atomicMax(p, (unsigned long long)t); else atomicAdd(p, (unsigned long long)t);
    }
  }
}

// Reassembly (main.rs:79-99): completion = max over fragments of the first
// arrival. keys[(u*B + m)*FP + f] -> tc[u*B + m] (peer-major; the transpose to
// the caller's message-major sink runs only when results are copied out).
// Per message it also reduces: the latest relative completion and the number
// of non-publishers that never complete (the lazy-gossip no-op proof of
// DESIGN.md §2.7), and with HIST the log lines, their latency sum / max and a
// 100 ms histogram (gs_msg_summary).
template <int FP, bool HIST>
__global__ __launch_bounds__(TB) void k_complete(CompArgs a) {
  __shared__ uint64_t red[TB];
  __shared__ uint32_t sh[HIST ? 64 * GS_HIST_BINS : 1];
  const MsgTile mt(a.MT, a.B);
  if (HIST)
    for (uint32_t i = threadIdx.x; i < 64 * GS_HIST_BINS; i += TB) sh[i] = 0;
  if (HIST) __syncthreads();
  uint64_t deliv = 0, lsum = 0, lmax = 0, tmax = 0, undel = 0, logged = 0, lgsum = 0, lgmax = 0;
  const uint32_t pm = mt.mv ? a.pub[mt.m] : EMPTY;
  const uint64_t tp = mt.mv ? a.tpub[mt.m] : 0;
  for (uint32_t u = blockIdx.x * (TB / 64) * (64 / a.MT) + mt.uoff; mt.mv && u < a.N; u += mt.rstep) {
    const size_t i = (size_t)u * a.B + mt.m;
    const uint64_t* kp = a.keys + i * FP;
    uint64_t mk = 0;
    bool ok = true;
#pragma unroll
    for (int f = 0; f < FP; f++) {  // padded fragments are INF: only f < F count
      const uint64_t x = f < (int)a.F ? kp[f] : 0;
      ok &= x != INF64;
      mk = x > mk ? x : mk;
    }
    uint64_t tc = INF64;
    uint8_t h = 0xFF;
    int64_t lms = -1;  // logged latency in ms
    if (u + a.u0 == pm) {  // its own key is set unless it published nothing (churn)
      if (kp[0] != INF64) {
        tc = tp;
        h = 0;
        if (a.self_log) lms = 0;
      }
    } else if (!a.collide && ok) {
      const uint64_t trel = mk >> a.tshift;
      tc = tp + trel;
      h = (uint8_t)((mk >> a.sb) & ((1u << HOP_BITS) - 1));
      const uint64_t ms = trel / 1000000ull;
      deliv++;
      lsum += ms;
      lmax = ms > lmax ? ms : lmax;
      tmax = trel > tmax ? trel : tmax;
      lms = (int64_t)ms;
    } else {
      undel++;
    }
    if (HIST && lms >= 0) {
      logged++;
      lgsum += (uint64_t)lms;
      lgmax = (uint64_t)lms > lgmax ? (uint64_t)lms : lgmax;
      const uint32_t bin = (uint64_t)lms / GS_HIST_MS < GS_HIST_BINS ? (uint32_t)((uint64_t)lms / GS_HIST_MS)
                                                                       : GS_HIST_BINS - 1;
      atomicAdd(&sh[((threadIdx.x & 63) % a.MT) * GS_HIST_BINS + bin], 1u);
    }
    if (a.tc) {  // results kept only when a sink will read them
      a.tc[i] = tc;
      a.hops[i] = h;
    }
    if (a.lat) {  // the log line's value (main.rs:93), GS_LAT_NONE where nothing is logged
      if (lms >= 0xFFFF) atomicOr((unsigned*)&a.counters[C_ERR], ERR_LAT16);
      a.lat[i] = lms < 0 ? (uint16_t)GS_LAT_NONE : (uint16_t)(lms < 0xFFFF ? lms : 0xFFFE);
    }
  }
  {
    const uint64_t d = wave_sum(deliv), s = wave_sum(lsum);
    uint64_t mx = lmax;
    for (int off = 32; off > 0; off >>= 1) {
      const uint64_t x = __shfl_xor(mx, off);
      mx = x > mx ? x : mx;
    }
    if ((threadIdx.x & 63) == 0 && d) {
      atomicAdd((unsigned long long*)&a.counters[C_DELIV], (unsigned long long)d);
      atomicAdd((unsigned long long*)&a.counters[C_LAT_SUM], (unsigned long long)s);
      atomicMax((unsigned long long*)&a.counters[C_LAT_MAX], (unsigned long long)mx);
    }
  }
  if (!a.mstat) return;  // block-uniform
  const uint32_t m0 = blockIdx.y * a.MT;
  msg_flush<true>(tmax, red, a.MT, m0, a.B, a.mstat, MS_TMAX);
  msg_flush<false>(undel, red, a.MT, m0, a.B, a.mstat, MS_UNDEL);
  if constexpr (HIST) {
    msg_flush<false>(logged, red, a.MT, m0, a.B, a.mstat, MS_LOGGED);
    msg_flush<false>(lgsum, red, a.MT, m0, a.B, a.mstat, MS_LSUM);
    msg_flush<true>(lgmax, red, a.MT, m0, a.B, a.mstat, MS_LMAX);
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < a.MT * GS_HIST_BINS; i += TB) {
      const uint32_t mm = m0 + i / GS_HIST_BINS;
      if (sh[i] && mm < a.B) atomicAdd(&a.hist[(size_t)mm * GS_HIST_BINS + i % GS_HIST_BINS], sh[i]);
    }
  }
}

// Exact percentiles, second pass: 1 ms counts inside the two 100 ms bins that
// hold each message's p50 / p95 rank (the host picked them from the histogram).
__global__ __launch_bounds__(TB) void k_pct(CompArgs a) {
  __shared__ uint32_t sf[64 * 2 * GS_HIST_MS];
  const MsgTile mt(a.MT, a.B);
  for (uint32_t i = threadIdx.x; i < 64 * 2 * GS_HIST_MS; i += TB) sf[i] = 0;
  __syncthreads();
  const uint32_t pm = mt.mv ? a.pub[mt.m] : EMPTY;
  const uint64_t tp = mt.mv ? a.tpub[mt.m] : 0;
  const uint32_t b50 = mt.mv ? a.pbin[mt.m * 2] : ~0u, b95 = mt.mv ? a.pbin[mt.m * 2 + 1] : ~0u;
  const uint32_t ml = (threadIdx.x & 63) % a.MT;
  for (uint32_t u = blockIdx.x * (TB / 64) * (64 / a.MT) + mt.uoff; mt.mv && u < a.N; u += mt.rstep) {
    const uint64_t t = a.tc[(size_t)u * a.B + mt.m];
    if (t == INF64 || (u + a.u0 == pm && !a.self_log)) continue;
    const uint64_t ms = (t - tp) / 1000000ull;
    const uint32_t bin = ms / GS_HIST_MS < GS_HIST_BINS ? (uint32_t)(ms / GS_HIST_MS) : GS_HIST_BINS - 1;
    const uint32_t r = bin == GS_HIST_BINS - 1 ? GS_HIST_MS - 1 : (uint32_t)(ms % GS_HIST_MS);
    if (bin == b50) atomicAdd(&sf[(ml * 2) * GS_HIST_MS + r], 1u);
    if (bin == b95) atomicAdd(&sf[(ml * 2 + 1) * GS_HIST_MS + r], 1u);
  }
  __syncthreads();
  const uint32_t m0 = blockIdx.y * a.MT;
  for (uint32_t i = threadIdx.x; i < a.MT * 2 * GS_HIST_MS; i += TB) {
    const uint32_t mm = m0 + i / (2 * GS_HIST_MS);
    if (sf[i] && mm < a.B) atomicAdd(&a.fine[(size_t)mm * 2 * GS_HIST_MS + i % (2 * GS_HIST_MS)], sf[i]);
  }
}

// The logged latency [N][B] u16 -> [B][N] through a 64x64 LDS tile (the
// message-major GS_WANT_LAT_MS stream).
__global__ __launch_bounds__(TB) void k_transpose16(const uint16_t* __restrict__ lat, uint16_t* __restrict__ lat_t,
                                                    uint32_t N, uint32_t B) {
  __shared__ uint16_t s[64][66];
  const uint32_t u0 = blockIdx.x * 64, m0 = blockIdx.y * 64;
  const uint32_t nu = min(64u, N - u0), nm = min(64u, B - m0);
  for (uint32_t i = threadIdx.x; i < 64 * 64; i += TB) {
    const uint32_t pu = i >> 6, qm = i & 63;
    if (pu < nu && qm < nm) s[qm][pu] = lat[(size_t)(u0 + pu) * B + m0 + qm];
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < 64 * 64; i += TB) {
    const uint32_t qm = i >> 6, pu = i & 63;
    if (pu < nu && qm < nm) lat_t[(size_t)(m0 + qm) * N + u0 + pu] = s[qm][pu];
  }
}

// [N][B] -> [B][N] through a 64x64 LDS tile, for the caller's message-major
// sink (include/gossipsim.h); not on the device-resident path.
__global__ __launch_bounds__(TB) void k_transpose(const uint64_t* __restrict__ tc, const uint8_t* __restrict__ hp,
                                                  uint64_t* __restrict__ tc_t, uint8_t* __restrict__ hp_t,
                                                  uint32_t N, uint32_t B) {
  __shared__ uint64_t s_tc[64][65];
  __shared__ uint8_t s_h[64][68];
  const uint32_t u0 = blockIdx.x * 64, m0 = blockIdx.y * 64;
  const uint32_t nu = min(64u, N - u0), nm = min(64u, B - m0);
  for (uint32_t i = threadIdx.x; i < 64 * 64; i += TB) {
    const uint32_t pu = i >> 6, qm = i & 63;
    if (pu < nu && qm < nm) {
      const size_t src = (size_t)(u0 + pu) * B + m0 + qm;
      s_tc[qm][pu] = tc[src];
      s_h[qm][pu] = hp[src];
    }
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < 64 * 64; i += TB) {
    const uint32_t qm = i >> 6, pu = i & 63;
    if (pu < nu && qm < nm) {
      const size_t dst = (size_t)(m0 + qm) * N + u0 + pu;
      tc_t[dst] = s_tc[qm][pu];
      hp_t[dst] = s_h[qm][pu];
    }
  }
}

#include "gs_lpull_kernel.h"
#include "gs_cpull.h"

uint32_t pow2_at_least(uint32_t x) { uint32_t p = 1; while (p < x) p <<= 1; return p; }

}  // namespace

// Chunks of one publish (PublishCommand.chunks, main.rs:65-71,163-168): the
// row's own count, 0 = FRAGMENTS of the node (env.rs:64-67).
static uint32_t frags_of(const Ctx& c, const gs_publish& p) { return p.frags ? p.frags : c.cfg.fragments; }

static void check_schedule(Ctx& c, const gs_publish* sched, uint64_t n_msgs) {
  for (uint64_t i = 0; i < n_msgs; i++) {
    if (sched[i].publisher >= c.cfg.peers) c.fail(GS_EINVAL, "publisher id out of range");
    if (sched[i].frags > MAX_FRAGS) c.fail(GS_EINVAL, "frags must be in 0..16 (0 = cfg.fragments)");
    if (frag_invalid(c.cfg.node, sched[i].msg_size, frags_of(c, sched[i])))  // the node's publish fails
      c.fail(GS_EINVAL, c.cfg.node == NODE_RUST ? "fragment payload shorter than the 8-byte tx_time stamp"
                        : c.cfg.node == NODE_GO ? "fragment too short for its chunk byte (payload[10])"
                                                : "fragment shorter than the 16-byte nim header + chunk byte");
  }
}

// Upload pub/tpub/link tables for messages [i0, i1) (equal msg_size) and
// compute the bucket width Delta = min latency + min serialisation.
// upload = false: only the host fields (a batch slice after the first: same shape and tables)
static Batch setup_batch(Ctx& c, const gs_publish* sched, uint64_t i0, uint64_t i1, bool upload = true) {
  Batch b;
  const uint32_t N = c.cfg.peers, S = c.S;
  b.F = frags_of(c, sched[i0]);
  b.FP = pow2_at_least(b.F);
  b.B = (uint32_t)(i1 - i0);
  b.L = b.B * b.FP;
  b.sb = bits_for(N);
  b.tshift = b.sb + HOP_BITS;
  b.tmax = b.tshift >= 64 ? 0 : (INF64 >> b.tshift);
  b.payload = frag_payload(c.cfg.node, sched[i0].msg_size, b.F);
  b.collide = frag_collide(c.cfg.node, sched[i0].msg_size, b.F);  // defect D8 (rust layout)
  b.Fe = b.collide ? 1 : b.F;
  hipStream_t s = c.stream;
  const uint64_t wire = gs_wire_bytes(b.payload, c.cfg.muxer, c.cfg.signed_msgs);
  std::vector<uint32_t> tab((size_t)S * S + 2 * S), pub(b.B);
  uint64_t min_lat = INF64, min_ser = INF64;
  // Delta from the link classes peers actually sit on (a Shadow graph may
  // carry nodes no peer uses, e.g. topogen's 1 ms injector hub)
  for (uint32_t x = 0; x < S; x++)
    for (uint32_t y = 0; y < S; y++) {
      if (c.lat_ns[(size_t)x * S + y] >= (1ull << 32)) c.fail(GS_ERANGE, "latency >= 2^32 ns");
      tab[(size_t)x * S + y] = (uint32_t)c.lat_ns[(size_t)x * S + y];
      if (c.stage_used[x] && c.stage_used[y]) min_lat = std::min<uint64_t>(min_lat, c.lat_ns[(size_t)x * S + y]);
    }
  for (uint32_t x = 0; x < S; x++) {
    const uint64_t up = ser_ns(wire, c.bw_up[x]), dn = ser_ns(wire, c.bw_dn[x]);
    if (up >= (1ull << 32) || dn >= (1ull << 32)) c.fail(GS_ERANGE, "serialisation >= 2^32 ns");
    tab[(size_t)S * S + x] = (uint32_t)up;
    tab[(size_t)S * S + S + x] = (uint32_t)dn;
    if (c.stage_used[x]) min_ser = std::min(min_ser, up);
  }
  b.delta = std::max<uint64_t>(1, min_lat + min_ser);
  for (uint32_t x = 0; x < S; x++) {
    if (!c.stage_used[x]) continue;
    b.ser_max = std::max<uint64_t>(b.ser_max, tab[(size_t)S * S + x]);
    for (uint32_t y = 0; y < S; y++) {
      if (!c.stage_used[y]) continue;
      const uint64_t up = tab[(size_t)S * S + x], dn = tab[(size_t)S * S + S + y];
      b.lat_adj_max = std::max<uint64_t>(b.lat_adj_max, tab[(size_t)x * S + y] + (dn > up ? dn - up : 0));
    }
  }
  b.lat_min = min_lat;
  for (uint32_t x = 0; x < S; x++)  // IHAVE x -> y, IWANT y -> x, answer x -> y (uplink of x, downlink of y)
    for (uint32_t y = 0; y < S; y++) {
      if (!c.stage_used[x] || !c.stage_used[y]) continue;
      const uint64_t up = tab[(size_t)S * S + x], dn = tab[(size_t)S * S + S + y];
      b.lat_max = std::max<uint64_t>(b.lat_max, tab[(size_t)x * S + y]);
      b.ans_max = std::max<uint64_t>(b.ans_max, (uint64_t)tab[(size_t)y * S + x] + up + tab[(size_t)x * S + y] +
                                                    (dn > up ? dn - up : 0));
    }
  b.tpub.resize(b.B);
  for (uint32_t q = 0; q < b.B; q++) { pub[q] = sched[i0 + q].publisher; b.tpub[q] = sched[i0 + q].t_pub_ns; }
  if (!upload) return b;
  c.d_pub.alloc(c.cfg.batch);
  c.d_tpub.alloc(c.cfg.batch);
  c.d_tables.alloc((size_t)S * S + 2 * S);
  GS_HIP(hipMemcpyAsync(c.d_pub.p, pub.data(), b.B * 4, hipMemcpyHostToDevice, s));
  GS_HIP(hipMemcpyAsync(c.d_tpub.p, b.tpub.data(), b.B * 8, hipMemcpyHostToDevice, s));
  GS_HIP(hipMemcpyAsync(c.d_tables.p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, s));
  // the host vectors die here: make the copies complete first
  GS_HIP(hipStreamSynchronize(s));
  return b;
}

// churn fields shared by SeedArgs and RelaxArgs (the ring and per-message epochs of gs_run)
template <class A>
static void set_churn_args(Ctx& c, A& a) {
  if (!c.cfg.churn_ppm) return;
  a.churn = 1;
  a.ring_mesh = c.d_ring_mesh.p;
  a.ring_off = c.d_ring_off.p;
  a.q0 = c.d_q0.p;
  a.r0 = c.d_r0.p;
  a.hb_ns = c.cfg.heartbeat_ns;
  a.ring_R = c.ring_R;
  a.w64 = (c.cfg.peers + 63) / 64;
  a.horizon = c.cfg.churn_horizon;
  a.N = c.cfg.peers;
}

static void launch_seed(Ctx& c, const Batch& b, uint32_t u0, uint32_t un, uint64_t* seed_min = nullptr,
                        uint32_t* chunkmin = nullptr, bool to_list = false, const uint32_t* pub = nullptr,
                        uint32_t soff = 0) {
  SeedArgs sa{};
  if (to_list) {
    sa.skey = c.d_skey.p;
    sa.slane = c.d_slane.p;
    sa.scnt = c.d_scnt.p;
  }
  set_churn_args(c, sa);
  sa.keys = c.d_keys.p; sa.row = c.d_row.p; sa.col = c.d_col.p; sa.mesh = c.d_mesh.p;
  sa.pub = pub ? pub : c.d_pub.p; sa.stage = c.d_stage.p; sa.tables = c.d_tables.p;
  sa.soff = soff;
  sa.ctrl = seed_min ? seed_min : c.d_ctrl.p; sa.chunkmin = chunkmin;
  sa.counters = c.d_counters.p; sa.tmax = b.tmax; sa.L = b.L; sa.FP = b.FP; sa.Fe = b.Fe;
  sa.S = c.S; sa.sb = b.sb; sa.tshift = b.tshift; sa.flood = c.cfg.flood_publish;
  sa.u0 = u0; sa.un = un;
  k_seed<<<b.B, TB, 0, c.stream>>>(sa);
  GS_HIP(hipGetLastError());
}

// k_complete over the keys rows [0, un) (global ids u0 + row) into d_tc /
// d_hops; with `mstat` also the per-message reductions, with `hist` the
// 100 ms histograms of gs_msg_summary.
// store: write d_tc / d_hops (results go to a sink); without it only the
// counters and reductions are produced (a device-resident run).
// lat: also the logged latencies [un][B] u16 into d_lat (GS_WANT_LAT_MS).
// r0: the batch's rows start at row r0 of the key / log buffers (a batch slice, run_slices)
// pub / tpub: the batch's publishers and publish times (default d_pub / d_tpub)
// batch_wide: of the reductions the caller reads only the batch's deliveries and latest
// final time, d_mstat[0] and [1] (batch_sums tells whether they are written that way)
static bool batch_sums(const Ctx& c, const Batch& b, bool mstat, bool lat, uint32_t nsl, bool batch_wide) {
  return c.keys_log && b.FP == 1 && !lat && nsl == 1 && (!mstat || batch_wide);
}
static void run_complete(Ctx& c, const Batch& b, uint32_t u0, uint32_t un, bool mstat, bool hist,
                         bool store = true, bool lat = false, size_t r0 = 0, const uint32_t* pub = nullptr,
                         const uint64_t* tpub = nullptr, uint32_t nsl = 1, bool batch_wide = false) {
  if (!pub) pub = c.d_pub.p;
  if (!tpub) tpub = c.d_tpub.p;
  hipStream_t s = c.stream;
  if (c.keys_none) c.fail(GS_EINVAL, "internal: completion after a no-log list pass (the passes completed the batch)");
  if (lat) c.d_lat.alloc((size_t)un * c.cfg.batch);
  if (c.keys_log) {  // list pull path, results on the device: reduce the final logs
    // (nsl batch slices of un rows each, one launch: block row y = slice y, run_slices)
    if (hist || store || (lat && nsl > 1)) c.fail(GS_EINVAL, "internal: final logs need k_lfinal");
    LPullArgs la{};
    la.u0 = u0;  // rows [0, un) are global peers u0 + row (a part of gs_run_partitioned)
    la.keys = c.d_keys.p + r0 * b.L; la.flane = c.d_flane.p + r0 * b.L; la.st = c.d_lst.p + r0 * LP_SW;
    la.pub = pub;
    la.counters = c.d_counters.p; la.N = un; la.B = b.B; la.L = b.L; la.tshift = b.tshift;
    la.F = b.F; la.collide = b.collide ? 1u : 0u;
    la.self_log = c.cfg.self_log;
    if (mstat) {
      c.d_mstat.alloc((size_t)std::max(c.cfg.batch, nsl * b.B) * MS_COLS);
      GS_HIP(hipMemsetAsync(c.d_mstat.p, 0, (size_t)nsl * b.B * MS_COLS * 8, s));
    }
    if (batch_sums(c, b, mstat, lat, nsl, batch_wide)) {  // the logged keys alone (k_lsum)
      const unsigned grid = (unsigned)std::max<uint64_t>(
          1, std::min<uint64_t>(((uint64_t)un + PULL_WAVES - 1) / PULL_WAVES, (uint64_t)std::max(1, c.num_cus) * 8));
      k_lsum<<<grid, TB, 0, s>>>(la, mstat ? c.d_mstat.p : nullptr);
      GS_HIP(hipGetLastError());
      return;
    }
    const unsigned grid = (unsigned)std::max<uint64_t>(
        1, std::min<uint64_t>(((uint64_t)un + LC_WAVES - 1) / LC_WAVES,
                              std::max<uint64_t>(1, (uint64_t)std::max(1, c.num_cus) / nsl)));
    k_lcomplete<<<dim3(grid, nsl), LC_WAVES * 64, 0, s>>>(la, mstat ? c.d_mstat.p : nullptr, lat ? c.d_lat.p : nullptr);
    GS_HIP(hipGetLastError());
    return;
  }
  CompArgs ca{};
  ca.keys = c.d_keys.p + r0 * b.L; ca.pub = pub; ca.tpub = tpub; ca.tc = store ? c.d_tc.p : nullptr;
  ca.hops = c.d_hops.p; ca.counters = c.d_counters.p; ca.N = un; ca.B = b.B; ca.F = b.F;
  ca.lat = lat ? c.d_lat.p : nullptr;
  ca.FP = b.FP; ca.L = b.L; ca.sb = b.sb; ca.tshift = b.tshift; ca.collide = b.collide ? 1 : 0;
  ca.u0 = u0;
  ca.self_log = c.cfg.self_log;
  ca.MT = std::min<uint32_t>(64, pow2_at_least(b.B));
  if (mstat || hist) {
    c.d_mstat.alloc((size_t)c.cfg.batch * MS_COLS);
    GS_HIP(hipMemsetAsync(c.d_mstat.p, 0, (size_t)b.B * MS_COLS * 8, s));
    ca.mstat = c.d_mstat.p;
  }
  if (hist) {
    c.d_hist.alloc((size_t)c.cfg.batch * GS_HIST_BINS);
    GS_HIP(hipMemsetAsync(c.d_hist.p, 0, (size_t)b.B * GS_HIST_BINS * 4, s));
    ca.hist = c.d_hist.p;
  }
  const uint32_t tiles = (b.B + ca.MT - 1) / ca.MT;
  const uint64_t rows_per_block = (TB / 64) * (64 / ca.MT);
  const uint64_t want = std::max<uint64_t>(1, (uint64_t)c.num_cus * 16 / tiles);
  // >= 16 rows per lane: every block ends in one atomic per message and column,
  // and a grid of thin blocks serialises on them (config #2, 10k rows x 2 message
  // tiles: 2048 blocks per tile, 595 us per batch, profiles/r04_v3)
  const uint64_t thick = (un + rows_per_block * 16 - 1) / (rows_per_block * 16);
  dim3 grid((unsigned)std::max<uint64_t>(1, std::min<uint64_t>(thick, want)), tiles);
  with_fp(b.FP, [&](auto fp) {
    if (hist) k_complete<fp.value, true><<<grid, TB, 0, s>>>(ca);
    else k_complete<fp.value, false><<<grid, TB, 0, s>>>(ca);
  });
  GS_HIP(hipGetLastError());
}

// Nearest-rank percentile (rank ceil(q*n)) resolved from the 100 ms histogram:
// the bin holding the rank, and the rank left inside that bin.
static void pct_bin(const uint32_t* h, uint64_t n, uint32_t q100, uint32_t* bin, uint64_t* rest) {
  const uint64_t rank = (n * q100 + 99) / 100;
  uint64_t acc = 0;
  for (uint32_t k = 0; k < GS_HIST_BINS; k++) {
    if (acc + h[k] >= rank) { *bin = k; *rest = rank - acc; return; }
    acc += h[k];
  }
  *bin = GS_HIST_BINS - 1;
  *rest = 0;
}

// gs_msg_summary of the batch's messages (rows [0, un) of d_tc): counts and
// histograms from k_complete, exact p50 / p95 from k_pct's 1 ms counts inside
// the two bins (a rank in the open last bin is read from the message's column).
static void fill_summary(Ctx& c, const Batch& b, uint32_t u0, uint32_t un, gs_msg_summary* out) {
  hipStream_t s = c.stream;
  const uint32_t B = b.B;
  std::vector<uint64_t> ms((size_t)B * MS_COLS);
  std::vector<uint32_t> hist((size_t)B * GS_HIST_BINS), pbin((size_t)B * 2, ~0u), rest((size_t)B * 2, 0);
  GS_HIP(hipMemcpyAsync(ms.data(), c.d_mstat.p, ms.size() * 8, hipMemcpyDeviceToHost, s));
  GS_HIP(hipMemcpyAsync(hist.data(), c.d_hist.p, hist.size() * 4, hipMemcpyDeviceToHost, s));
  GS_HIP(hipStreamSynchronize(s));
  std::vector<uint32_t> slow;  // messages whose p50 or p95 lies in the open last bin
  for (uint32_t q = 0; q < B; q++) {
    gs_msg_summary& r = out[q];
    memset(&r, 0, sizeof r);
    r.delivered = ms[(size_t)q * MS_COLS + MS_LOGGED];
    r.lat_sum_ms = ms[(size_t)q * MS_COLS + MS_LSUM];
    r.max_ms = (uint32_t)ms[(size_t)q * MS_COLS + MS_LMAX];
    memcpy(r.hist, &hist[(size_t)q * GS_HIST_BINS], sizeof r.hist);
    if (!r.delivered) continue;
    uint64_t rs[2];
    uint32_t bn[2];
    pct_bin(r.hist, r.delivered, 50, &bn[0], &rs[0]);
    pct_bin(r.hist, r.delivered, 95, &bn[1], &rs[1]);
    if (bn[0] == GS_HIST_BINS - 1 || bn[1] == GS_HIST_BINS - 1) { slow.push_back(q); continue; }
    for (int k = 0; k < 2; k++) { pbin[q * 2 + k] = bn[k]; rest[q * 2 + k] = (uint32_t)rs[k]; }
  }
  c.d_pbin.alloc((size_t)c.cfg.batch * 2);
  c.d_fine.alloc((size_t)c.cfg.batch * 2 * GS_HIST_MS);
  GS_HIP(hipMemcpyAsync(c.d_pbin.p, pbin.data(), pbin.size() * 4, hipMemcpyHostToDevice, s));
  GS_HIP(hipMemsetAsync(c.d_fine.p, 0, (size_t)B * 2 * GS_HIST_MS * 4, s));
  CompArgs ca{};
  ca.pub = c.d_pub.p; ca.tpub = c.d_tpub.p; ca.tc = c.d_tc.p; ca.N = un; ca.B = B; ca.u0 = u0;
  ca.self_log = c.cfg.self_log; ca.pbin = c.d_pbin.p; ca.fine = c.d_fine.p;
  ca.MT = std::min<uint32_t>(64, pow2_at_least(B));
  const uint32_t tiles = (B + ca.MT - 1) / ca.MT;
  const uint64_t rows_per_block = (TB / 64) * (64 / ca.MT);
  dim3 grid((unsigned)std::max<uint64_t>(1, std::min<uint64_t>((un + rows_per_block - 1) / rows_per_block,
                                                               std::max<uint64_t>(1, (uint64_t)c.num_cus * 8 / tiles))),
            tiles);
  k_pct<<<grid, TB, 0, s>>>(ca);
  GS_HIP(hipGetLastError());
  std::vector<uint32_t> fine((size_t)B * 2 * GS_HIST_MS);
  GS_HIP(hipMemcpyAsync(fine.data(), c.d_fine.p, fine.size() * 4, hipMemcpyDeviceToHost, s));
  GS_HIP(hipStreamSynchronize(s));
  for (uint32_t q = 0; q < B; q++) {
    if (pbin[q * 2] == ~0u) continue;
    for (int k = 0; k < 2; k++) {
      const uint32_t* f = &fine[((size_t)q * 2 + k) * GS_HIST_MS];
      uint64_t acc = 0;
      uint32_t r = 0;
      while (r < GS_HIST_MS - 1 && acc + f[r] < rest[q * 2 + k]) acc += f[r++];
      (k ? out[q].p95_ms : out[q].p50_ms) = pbin[q * 2 + k] * GS_HIST_MS + r;
    }
  }
  for (uint32_t q : slow) {  // rare (heavy churn tails): the column, sorted on the host
    std::vector<uint64_t> col(un);
    GS_HIP(hipMemcpy2DAsync(col.data(), 8, c.d_tc.p + q, (size_t)B * 8, 8, un, hipMemcpyDeviceToHost, s));
    std::vector<uint32_t> pub(1);
    GS_HIP(hipMemcpyAsync(pub.data(), c.d_pub.p + q, 4, hipMemcpyDeviceToHost, s));
    GS_HIP(hipStreamSynchronize(s));
    std::vector<uint64_t> v;
    for (uint32_t u = 0; u < un; u++)
      if (col[u] != INF64 && (u + u0 != pub[0] || c.cfg.self_log)) v.push_back((col[u] - b.tpub[q]) / 1000000ull);
    std::sort(v.begin(), v.end());
    const uint64_t n = v.size();
    out[q].p50_ms = (uint32_t)v[(n * 50 + 99) / 100 - 1];
    out[q].p95_ms = (uint32_t)v[(n * 95 + 99) / 100 - 1];
  }
}

#include "gs_peerdelay.h"

// What a sink takes from a batch (include/gossipsim.h gs_result_sink): with
// on_block the want bits select t_complete / hops (neither = both), without
// it the non-NULL arrays do; on_lat takes the logged latency (GS_WANT_LAT_MS).
// lat: the batch's logged latencies are needed — by the sink's on_lat, or by the
// context's delay accumulators (gs_set_peer_delay; the one place that switch
// becomes a want: the completion then writes d_lat and no batch runs without its log).
struct SinkWants {
  bool tc = false, h = false, lat = false, on_lat = false, summary = false;
  bool rows() const { return tc || h; }
};
static SinkWants sink_wants(const Ctx& c, const gs_result_sink* sink) {
  SinkWants w;
  w.lat = c.pdelay;
  if (!sink) return w;
  if (sink->on_block) {
    uint32_t th = sink->want & (GS_WANT_T_COMPLETE | GS_WANT_HOPS);
    if (!th) th = GS_WANT_T_COMPLETE | GS_WANT_HOPS;
    w.tc = (th & GS_WANT_T_COMPLETE) != 0;
    w.h = (th & GS_WANT_HOPS) != 0;
  } else {
    w.tc = sink->t_complete_ns != nullptr;
    w.h = sink->hops != nullptr;
  }
  w.on_lat = sink->on_lat != nullptr;
  w.lat = w.lat || w.on_lat;
  w.summary = sink->summary != nullptr;
  return w;
}

// Message-major rows of the batch — [B][un] in d_tc_t / d_hops_t, and the
// latency in d_lat_t — into a sink's rows [row0, row0 + B): its arrays (host
// memory; device memory when c.sink_dev, the message-sharded partitioned
// batches of gs_comm.hip), and the on_block / on_lat streams in blocks of
// block_msgs messages through two pinned staging halves (the copy of block k
// runs while the caller's callbacks consume block k - 1).
void deliver_rows(Ctx& c, uint32_t B, uint32_t un, const gs_result_sink* sink, uint64_t sink_row0) {
  hipStream_t s = c.stream;
  const SinkWants w = sink_wants(c, sink);
  if (!sink->on_block && w.rows()) {
    const hipMemcpyKind kind = c.sink_dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (w.tc) GS_HIP(hipMemcpyAsync(sink->t_complete_ns + sink_row0 * un, c.d_tc_t.p, (size_t)B * un * 8, kind, s));
    if (w.h) GS_HIP(hipMemcpyAsync(sink->hops + sink_row0 * un, c.d_hops_t.p, (size_t)B * un, kind, s));
  }
  const bool st_rows = sink->on_block != nullptr, st_lat = w.on_lat;
  if (!st_rows && !st_lat) return;
  const uint32_t bm = std::max<uint32_t>(1, std::min<uint32_t>(sink->block_msgs ? sink->block_msgs : 64, B));
  const size_t cell = (st_rows && w.tc ? 8 : 0) + (st_lat ? 2 : 0) + (st_rows && w.h ? 1 : 0);
  const size_t half = ((size_t)bm * un * cell + 255) & ~(size_t)255;
  if (c.h_block_bytes < 2 * half) {
    if (c.h_block) GS_HIP(hipHostFree(c.h_block));
    c.h_block = nullptr;
    c.h_block_bytes = 0;
    GS_HIP(hipHostMalloc(&c.h_block, 2 * half, hipHostMallocDefault));
    c.h_block_bytes = 2 * half;
  }
  for (int k = 0; k < 2; k++)
    if (!c.blk_ev[k]) GS_HIP(hipEventCreateWithFlags(&c.blk_ev[k], hipEventDisableTiming));
  struct Part { uint64_t* tc; uint16_t* lat; uint8_t* h; };
  auto part = [&](int k) {  // [t_complete u64][latency u16][hops u8] of one half
    uint8_t* p = (uint8_t*)c.h_block + (size_t)k * half;
    Part q{nullptr, nullptr, nullptr};
    if (st_rows && w.tc) { q.tc = (uint64_t*)p; p += (size_t)bm * un * 8; }
    if (st_lat) { q.lat = (uint16_t*)p; p += (size_t)bm * un * 2; }
    if (st_rows && w.h) q.h = p;
    return q;
  };
  auto hand_over = [&](int k, uint32_t q0, uint32_t n) {
    GS_HIP(hipEventSynchronize(c.blk_ev[k]));
    const Part q = part(k);
    if (st_rows) sink->on_block(sink->user, sink_row0 + q0, n, un, q.tc, q.h);
    if (st_lat) sink->on_lat(sink->user, sink_row0 + q0, n, un, q.lat);
  };
  int prev = -1;
  uint32_t pq0 = 0, pn = 0;
  for (uint32_t q0 = 0, k = 0; q0 < B; q0 += bm, k ^= 1) {
    const uint32_t n = std::min(bm, B - q0);
    const Part q = part((int)k);
    if (q.tc) GS_HIP(hipMemcpyAsync(q.tc, c.d_tc_t.p + (size_t)q0 * un, (size_t)n * un * 8, hipMemcpyDeviceToHost, s));
    if (q.lat)
      GS_HIP(hipMemcpyAsync(q.lat, c.d_lat_t.p + (size_t)q0 * un, (size_t)n * un * 2, hipMemcpyDeviceToHost, s));
    if (q.h) GS_HIP(hipMemcpyAsync(q.h, c.d_hops_t.p + (size_t)q0 * un, (size_t)n * un, hipMemcpyDeviceToHost, s));
    GS_HIP(hipEventRecord(c.blk_ev[k], s));
    if (prev >= 0) hand_over(prev, pq0, pn);  // block k - 1 while block k is copied
    prev = (int)k;
    pq0 = q0;
    pn = n;
  }
  hand_over(prev, pq0, pn);
}

// The pending latency-only delivery of the previous batch (deliver_lat_async):
// wait for its copy, check the error word it carried (a latency the u16 stream
// cannot hold fails the run before any of that batch's lines are handed out),
// then its callbacks block by block.
static void lat_flush(Ctx& c) {
  Ctx::LatPending& p = c.lat_pend;
  if (!p.on) return;
  p.on = false;
  GS_HIP(hipEventSynchronize(c.lat_done[p.par]));
  if (c.h_laterr[p.par] & ERR_LAT16)
    c.fail(GS_ERANGE, "a logged latency of 65535 ms or more does not fit the u16 stream (GS_WANT_LAT_MS)");
  for (uint32_t q0 = 0; q0 < p.B; q0 += p.bm) {
    const uint32_t n = std::min(p.bm, p.B - q0);
    p.sink->on_lat(p.sink->user, p.row0 + q0, n, p.un, c.h_lat[p.par] + (size_t)q0 * p.un);
  }
}

// A latency-only sink inside gs_run (on_lat, no rows, no summary): the batch's
// transposed u16 latencies leave on the copy stream into a whole-batch pinned
// buffer of this batch's parity while the next batch's passes run; the
// previous batch's callbacks run now (its copy had this batch's passes to
// finish), this batch's at the next delivery or at the end of the run.
static void deliver_lat_async(Ctx& c, const Batch& b, uint32_t un, const gs_result_sink* sink, uint64_t sink_row0) {
  hipStream_t s = c.stream;
  const uint32_t par = c.lat_par;
  c.lat_par ^= 1u;
  DevBuf<uint16_t>& lt = par ? c.d_lat_t2 : c.d_lat_t;
  lt.alloc((size_t)un * c.cfg.batch);
  dim3 tg((un + 63) / 64, (b.B + 63) / 64);
  k_transpose16<<<tg, TB, 0, s>>>(c.d_lat.p, lt.p, un, b.B);
  GS_HIP(hipGetLastError());
  pd_accumulate(c, lt.p, c.d_tpub.p, b.B, un);
  const size_t bytes = (size_t)b.B * un * 2;
  if (c.h_lat_bytes[par] < bytes) {
    if (c.h_lat[par]) GS_HIP(hipHostFree(c.h_lat[par]));
    c.h_lat[par] = nullptr;
    c.h_lat_bytes[par] = 0;
    GS_HIP(hipHostMalloc((void**)&c.h_lat[par], bytes, hipHostMallocDefault));
    c.h_lat_bytes[par] = bytes;
  }
  if (!c.h_laterr) GS_HIP(hipHostMalloc((void**)&c.h_laterr, 2 * 8, hipHostMallocDefault));
  if (!c.copy) GS_HIP(hipStreamCreateWithFlags(&c.copy, hipStreamNonBlocking));
  for (int k = 0; k < 2; k++) {
    if (!c.lat_src[k]) GS_HIP(hipEventCreateWithFlags(&c.lat_src[k], hipEventDisableTiming));
    if (!c.lat_done[k]) GS_HIP(hipEventCreateWithFlags(&c.lat_done[k], hipEventDisableTiming));
  }
  GS_HIP(hipEventRecord(c.lat_src[par], s));
  GS_HIP(hipStreamWaitEvent(c.copy, c.lat_src[par], 0));
  GS_HIP(hipMemcpyAsync(c.h_lat[par], lt.p, bytes, hipMemcpyDeviceToHost, c.copy));
  GS_HIP(hipMemcpyAsync(c.h_laterr + par, c.d_counters.p + C_ERR, 8, hipMemcpyDeviceToHost, c.copy));
  GS_HIP(hipEventRecord(c.lat_done[par], c.copy));
  lat_flush(c);  // the previous batch, in message order
  Ctx::LatPending& p = c.lat_pend;
  p.on = true;
  p.par = par;
  p.B = b.B;
  p.un = un;
  p.bm = std::max<uint32_t>(1, std::min<uint32_t>(sink->block_msgs ? sink->block_msgs : 64, b.B));
  p.row0 = sink_row0;
  p.sink = sink;
}

#include "gs_logtext.h"

// Results of a completed batch (peer-major d_tc / d_hops / d_lat of peers
// [u0, u0 + un)) into the sink: transposed to message-major, copied out,
// summaries.
static void deliver(Ctx& c, const Batch& b, uint32_t u0, uint32_t un, const gs_result_sink* sink,
                    uint64_t sink_row0) {
  const SinkWants w = sink_wants(c, sink);
  if (!sink && !w.lat) return;  // (no sink: the delay accumulators still take the batch)
  hipStream_t s = c.stream;
  if (c.keys_none && (w.rows() || w.lat || w.summary))
    c.fail(GS_EINVAL, "internal: a sink's results after a no-log list pass");
  if (c.text.fn) {  // gs_run_log: the latencies leave as text (its sink asks for nothing else)
    deliver_text(c, b, u0, un, sink_row0);
    return;
  }
  if (c.lat_async && w.on_lat && !w.rows() && !w.summary) {
    deliver_lat_async(c, b, un, sink, sink_row0);
    return;
  }
  lat_flush(c);  // (a pending batch is delivered before this one)
  if (w.rows()) {
    c.d_tc_t.alloc((size_t)un * c.cfg.batch);
    c.d_hops_t.alloc((size_t)un * c.cfg.batch);
    dim3 tg((un + 63) / 64, (b.B + 63) / 64);
    k_transpose<<<tg, TB, 0, s>>>(c.d_tc.p, c.d_hops.p, c.d_tc_t.p, c.d_hops_t.p, un, b.B);
    GS_HIP(hipGetLastError());
  }
  if (w.lat && c.lat_staged) {  // a partitioned batch: transposed and checked over every part already
    c.lat_staged = false;
  } else if (w.lat) {
    c.d_lat_t.alloc((size_t)un * c.cfg.batch);
    dim3 tg((un + 63) / 64, (b.B + 63) / 64);
    k_transpose16<<<tg, TB, 0, s>>>(c.d_lat.p, c.d_lat_t.p, un, b.B);
    GS_HIP(hipGetLastError());
    pd_accumulate(c, c.d_lat_t.p, c.d_tpub.p, b.B, un);
    GS_HIP(hipMemcpyAsync(c.h_pinned, c.d_counters.p + C_ERR, 8, hipMemcpyDeviceToHost, s));
    GS_HIP(hipStreamSynchronize(s));
    if (c.h_pinned[0] & ERR_LAT16) c.fail(GS_ERANGE, "a logged latency of 65535 ms or more does not fit the u16 "
                                                     "stream (GS_WANT_LAT_MS, gs_set_peer_delay)");
  }
  if (w.rows() || w.on_lat) deliver_rows(c, b.B, un, sink, sink_row0);
  if (w.summary) fill_summary(c, b, u0, un, sink->summary + sink_row0);
}

// Completion + delivery of a finished batch.
static void launch_complete(Ctx& c, const Batch& b, uint32_t u0, uint32_t un, const gs_result_sink* sink,
                            uint64_t sink_row0, size_t r0 = 0) {
  const bool hist = sink && sink->summary;
  const SinkWants w = sink_wants(c, sink);
  run_complete(c, b, u0, un, hist, hist, w.rows() || w.summary, w.lat, r0);  // k_pct reads d_tc
  deliver(c, b, u0, un, sink, sink_row0);
}

// The batch's fields of RelaxArgs shared by the bucket launches and the
// traffic passes: keys, graph, link tables, churn ring, and with `gossip` the
// lazy-gossip inputs (heartbeats per message, CSR, IHAVE target ring).
// Bucket launches one churn + gossip batch may take (the holder list's
// per-launch marks, RelaxArgs::hl_lo / hl_end).
constexpr uint32_t HL_LAUNCHES = 1u << 16;

static RelaxArgs relax_args(Ctx& c, const Batch& b, bool gossip) {
  RelaxArgs ra{};
  set_churn_args(c, ra);
  ra.keys = c.d_keys.p; ra.mesh = c.d_mesh.p; ra.pub = c.d_pub.p;
  ra.stage = c.d_stage.p; ra.tables = c.d_tables.p;
  ra.total = (uint64_t)c.cfg.peers * b.L; ra.tmax = b.tmax;
  ra.N = c.cfg.peers; ra.B = b.B; ra.F = b.F; ra.L = b.L; ra.S = c.S; ra.sb = b.sb; ra.tshift = b.tshift;
  ra.idw = (c.cfg.idontwant && b.payload >= c.cfg.idontwant) ? 1 : 0;
  ra.row = c.d_row.p;
  ra.col = c.d_col.p;
  if (gossip) {
    ra.rel0 = c.d_rel0.p;
    ra.habs0 = c.d_habs0.p;
    ra.hb_ns = c.cfg.heartbeat_ns;
    ra.seed = c.cfg.seed;
    ra.gossip = 1;
    if (c.cfg.churn_ppm) {
      ra.ring_in = c.d_ring_in.p;
      // heartbeats of a message from index gs_switch on are decided
      // sender-centric (exact for any value; GS_GOSSIP_SWITCH for tests / A/B)
      ra.gs_switch = (uint32_t)env_int("GS_GOSSIP_SWITCH", 4);
      // the per-lane first gossip heartbeat (RelaxArgs::hwin) saturates at 254:
      // the receiver-centric test k < j0 needs gs_switch <= 254 to stay exact
      // (a larger switch puts every heartbeat of a 16-epoch lifetime on that side anyway)
      if (ra.gs_switch > 254) ra.gs_switch = 254;
    }
    ra.hist = c.cfg.history_gossip;
    ra.d_lazy = c.cfg.d_lazy;
    ra.gf_milli = c.cfg.gossip_factor_milli;
  }
  return ra;
}

// The grid of a grid-stride pass over a finished batch's `total` dense keys.
static unsigned keys_pass_grid(const Ctx& c, uint64_t total) {
  return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((total + TB - 1) / TB, (uint64_t)c.num_cus * 8));
}

// Per-peer traffic of the batch just finished (keys final, before the next
// reset; gs_traffic.h).
static void launch_traffic(Ctx& c, const Batch& b) {
  if (c.keys_none) c.fail(GS_EINVAL, "internal: the traffic pass after a no-log list pass");
  const bool gossip = c.cfg.lazy_gossip != 0;
  const RelaxArgs ra = relax_args(c, b, gossip);
  TrafficArgs ta{};
  ta.traffic = c.d_traffic.p;
  ta.W = gs_wire_bytes(b.payload, c.cfg.muxer, c.cfg.signed_msgs);
  gs_wire_packets(b.payload, c.cfg.muxer, c.cfg.signed_msgs, &ta.pk, &ta.hdr);
  gs_control_packets(GS_CTRL_IHAVE, c.cfg.node, c.cfg.muxer, &ta.ihw, &ta.ihpk, &ta.ihhd);
  gs_control_packets(GS_CTRL_IWANT, c.cfg.node, c.cfg.muxer, &ta.iww, &ta.iwpk, &ta.iwhd);
  gs_control_packets(GS_CTRL_ACK, c.cfg.node, c.cfg.muxer, &ta.ack, nullptr, nullptr);
  ta.Fe = b.Fe;
  ta.flood = c.cfg.flood_publish;
  ta.collide = b.collide ? 1 : 0;
  hipStream_t s = c.stream;
  const unsigned grid = keys_pass_grid(c, ra.total);
  k_traffic_pub<<<b.B, TB, 0, s>>>(ra, ta);
  with_fp(b.FP, [&](auto fp) {
    k_traffic_fwd<fp.value><<<grid, TB, 0, s>>>(ra, ta);
    if (gossip && c.cfg.history_gossip) k_traffic_gossip<fp.value><<<grid, TB, 0, s>>>(ra, ta);
  });
  GS_HIP(hipGetLastError());
}

#include "gs_pubsub.h"
#include "gs_linkdel.h"
#include "gs_msgcost.h"

// The passes over a finished batch's dense final keys (Ctx::keys_pass): each switch's own.
// i0: the batch's first message in the run driver's schedule.
static void launch_key_passes(Ctx& c, const Batch& b, uint64_t i0) {
  if (c.traffic) launch_traffic(c, b);
  if (c.pubsub) launch_pubsub(c, b);
  if (c.linkdel) launch_linkdel(c, b);
  if (c.msgcost) launch_msgcost(c, b, i0);
}

// Read the device counters into ctx->stats (and raise the device error word).
static void collect_stats(Ctx& c) {
  hipStream_t s = c.stream;
  GS_HIP(hipMemcpyAsync(c.h_pinned, c.d_counters.p, C_COUNT * 8, hipMemcpyDeviceToHost, s));
  GS_HIP(hipStreamSynchronize(s));
  const uint64_t* h = c.h_pinned;
  if (h[C_ERR] & ERR_TIME) c.fail(GS_ERANGE, "relative arrival time overflowed the key's time field");
  if (h[C_ERR] & ERR_HOPS) c.fail(GS_ERANGE, "hop count overflowed the key's 6-bit hop field");
  if (h[C_ERR] & ERR_LINK) c.fail(GS_ERANGE, "a final key names a sender outside the receiver's CSR row (link deliveries)");
  c.stats.frag_deliveries = h[C_FD];
  c.stats.relaxations = h[C_R] + h[C_R_FWD] + h[C_GOSSIP];
  c.stats.gossip_iwant = h[C_GOSSIP];
  c.stats.deliveries = h[C_DELIV];
  c.stats.latency_sum_ms = h[C_LAT_SUM];
  c.stats.latency_max_ms = h[C_LAT_MAX];
  c.stats.buckets = h[C_BUCKETS];
  c.stats.bytes_alg = 16 * h[C_FD] + 12 * c.stats.relaxations + 8 * h[C_DELIV];
  c.stats.relax_bytes_alg = 16 * h[C_FD] + 12 * h[C_R_FWD];
  c.stats.pushes = h[C_PUSH];
  static const bool dbg = getenv("GS_DEBUG_COUNTS") != nullptr;
  if (dbg)
    fprintf(stderr, "[gs] buckets %llu gossip-listed lanes %llu tiles scanned %llu (for gossip only %llu) iwant %llu\n",
            (unsigned long long)h[C_BUCKETS], (unsigned long long)h[C_GLISTED], (unsigned long long)h[C_TSCANNED],
            (unsigned long long)h[C_TSCANNED_G], (unsigned long long)h[C_GOSSIP]);
}


// One pass of the pull or list path, under timing as (start, mid, end): the whole pass is frontier time.
template <class Fn>
static void timed_pass(Ctx& c, hipStream_t s, Fn&& launch) {
  if (!c.timing) return launch();
  GS_HIP(hipEventRecord(run_ev(c, c.ev_n), s));
  GS_HIP(hipEventRecord(run_ev(c, c.ev_n + 1), s));
  launch();
  GS_HIP(hipEventRecord(run_ev(c, c.ev_n + 2), s));
  c.ev_n += 3;
}

// The reverse positions of the mesh (k_rpos), once per mesh: every pull and list pass reads them.
static void ensure_rpos(Ctx& c) {
  if (c.rpos_valid) return;
  const uint32_t N = c.cfg.peers;
  hipStream_t s = c.stream;
  c.d_rpos.alloc((size_t)N * MESH_W);
  GS_HIP(hipMemsetAsync(c.d_counters.p + C_ERR, 0, 8, s));
  k_rpos<<<(unsigned)(((uint64_t)N * MESH_W + TB - 1) / TB), TB, 0, s>>>(c.d_mesh.p, c.d_rpos.p, N, c.d_counters.p);
  GS_HIP(hipGetLastError());
  if (read_counter(c, C_ERR) & ERR_MESH) c.fail(GS_ERANGE, "mesh is not symmetric");
  c.rpos_valid = true;
}

// The pass control before a batch's seeds: every slot {lo 0, DONE, 0 records, min INF}; the
// batch words behind the slots (a no-log list pass's latest final time and deliveries) 0.
static void pctrl_reset(Ctx& c) {
  static_assert(LP_CT_TMAX == PS_SLOTS * PS_WORDS && PM_DONE == 0, "the batch words follow the slots; zero is DONE");
  hipStream_t s = c.stream;
  c.d_pctrl.alloc(LP_CT_WORDS);
  GS_HIP(hipMemsetAsync(c.d_pctrl.p, 0, LP_CT_WORDS * 8, s));
  for (uint32_t q = 0; q < PS_SLOTS; q++) GS_HIP(hipMemsetAsync(c.d_pctrl.p + q * PS_WORDS + PS_MIN, 0xFF, 8, s));
}

// In the host's last read of the control slots (h_pinned[0 ..]): the slot the last of `pass` passes wrote.
static const uint64_t* last_slot(const Ctx& c, uint32_t pass) {
  return c.h_pinned + ((pass - 1) % PS_SLOTS) * PS_WORDS;
}

// One batch on the owner-computes path (gs_pull_kernel.h): seed, then passes in
// chunks of 8 until a pass decides DONE (one host read of the ctrl slots per chunk).
static void run_pull_batch(Ctx& c, const Batch& b) {
  const uint32_t N = c.cfg.peers, L = b.L;
  hipStream_t s = c.stream;
  const size_t NL = (size_t)N * L;
  c.d_chunkmin.alloc((size_t)N * PULL_CH);
  c.d_lrec.alloc(2 * NL);
  c.d_lcnt.alloc(2 * (size_t)N);
  ensure_rpos(c);
  GS_HIP(hipMemsetAsync(c.d_chunkmin.p, 0xFF, (size_t)N * PULL_CH * 4, s));
  pctrl_reset(c);
  launch_seed(c, b, 0, N, c.d_pctrl.p + PS_SEED_MIN, c.d_chunkmin.p);
  PullArgs pa{};
  pa.keys = c.d_keys.p; pa.busy = c.d_busy.p; pa.chunkmin = c.d_chunkmin.p;
  pa.lrec = c.d_lrec.p; pa.lcnt = c.d_lcnt.p; pa.rpos = c.d_rpos.p;
  pa.mesh = c.d_mesh.p; pa.pub = c.d_pub.p; pa.stage = c.d_stage.p; pa.tables = c.d_tables.p;
  // windows on the key's high-word grain (gs_pull_kernel.h); the caller checked delta >= grain
  const uint64_t grain = pull_grain(b.tshift);
  pa.ctrl = c.d_pctrl.p; pa.counters = c.d_counters.p; pa.delta = b.delta / grain * grain;
  pa.tmax = b.tmax - grain;
  pa.N = N; pa.B = b.B; pa.L = L; pa.S = c.S; pa.sb = b.sb; pa.tshift = b.tshift;
  // 33 KB of LDS per block: 4 blocks (16 waves, 16 rows in flight) per CU
  const unsigned grid = (unsigned)std::max<uint64_t>(
      1, std::min<uint64_t>(((uint64_t)N + PULL_WAVES - 1) / PULL_WAVES, (uint64_t)c.num_cus * 4));
  uint32_t pass = 0;
  for (;;) {
    for (uint32_t q = 0; q < 8; q++) {
      pa.pass = pass++;
      timed_pass(c, s, [&] { pull_dispatch(b.FP, pa, grid, s); });
    }
    GS_HIP(hipGetLastError());
    GS_HIP(hipMemcpyAsync(c.h_pinned, c.d_pctrl.p, PS_SLOTS * PS_WORDS * 8, hipMemcpyDeviceToHost, s));
    GS_HIP(hipStreamSynchronize(s));
    if (last_slot(c, pass)[PS_MODE] == PM_DONE) break;
  }
  c.stats.relax_launches += pass;
}

// Largest arrival offset of a forward relative to its uplink start: latency +
// downlink excess + MESH_W serialisations (the receiver's FIFO position).
// Largest arrival after a lane's final time: the uplink FIFO behind the other
// FP - 1 fragments' sends, then MESH_W serialisations, the adjusted latency.
static uint64_t lpull_rmax(const Batch& b) {
  return b.lat_adj_max + (uint64_t)MESH_W * b.ser_max * b.FP;
}

// Entries per candidate list: at least 256, so that rows of few lanes (small
// batches) still hold several passes' appends of the same lanes.
static uint32_t lpull_stride(const Batch& b) { return std::max<uint32_t>(b.L, 256); }

// Ring size K of the list pull path (gs_lpull_kernel.h) for this batch, or 0
// when it cannot take the batch (then k_pull runs). A candidate made from a
// record of window b arrives before b*D + D (start inside the window) + the
// fragment FIFO + the largest link latency + MESH_W serialisations, so its
// destination is at most K - 1 windows after the emitted one; the entry
// packs (t - window start) | hops | src | lane into 64 bits; the seed list
// packs row << 11 | lane (N < 2^21); the lists must fit the device memory left.
// rows: the pass's rows (batch slices: slices x peers)
static uint32_t lpull_ring(Ctx& c, const Batch& b, uint64_t delta, uint32_t* lb, bool gos = false, bool chn = false,
                           uint32_t rows = 0) {
  if (!c.mesh_dmax) {  // widest mesh row, once per mesh
    std::vector<uint32_t> m((size_t)c.cfg.peers * MESH_W);
    GS_HIP(hipMemcpyAsync(m.data(), c.d_mesh.p, m.size() * 4, hipMemcpyDeviceToHost, c.stream));
    GS_HIP(hipStreamSynchronize(c.stream));
    uint32_t dmax = 1;
    for (size_t u = 0; u < c.cfg.peers; u++) {
      uint32_t d = 0;
      while (d < MESH_W && m[u * MESH_W + d] != EMPTY) d++;
      dmax = std::max(dmax, d);
    }
    c.mesh_dmax = dmax;
  }
  const uint32_t N = rows ? rows : c.cfg.peers;
  if (b.tshift >= 32 || b.L > PULL_LMAX || delta < 2 || N >= (1u << 21)) return 0;  // seed list: row << 11
  // a fragment waits behind at most the other FP - 1 fragments' sends to the
  // row's mesh peers (c.mesh_dmax, the widest mesh row)
  // (churn: each epoch has its own mesh, bounded by the ELL width)
  const uint64_t dm = chn ? MESH_W : c.mesh_dmax ? c.mesh_dmax : MESH_W;
  const uint64_t fifo = (uint64_t)(b.FP - 1) * dm * b.ser_max;
  const uint64_t span = delta + fifo + b.lat_adj_max + dm * b.ser_max;
  // k_seed's first sends (every fragment to every mesh peer, or to every
  // connection with flood publish) land in windows 1 .. K of source window 0
  const uint64_t sdeg = c.cfg.flood_publish ? std::max<uint64_t>(c.max_degree, 1) : dm;
  const uint64_t seed_span = (uint64_t)b.FP * sdeg * b.ser_max + b.lat_adj_max;
  uint64_t K = std::max(span / delta + 2, seed_span / delta + 1);
  // GOS: an IWANT answer is appended from the window of its IHAVE's arrival
  if (gos) K = std::max<uint64_t>(K, (delta + b.ans_max) / delta + 2);
  if (K > LP_KMAX) return 0;
  // test knob: a ring smaller than the bound forces ERR_RING and the k_pull re-run
  // (per batch: tests set it between runs)
  K = std::min<uint64_t>(K, (uint64_t)std::max(2l, env_int("GS_LPULL_K", LP_KMAX)));
  uint32_t tb = 0;
  while ((1ull << tb) < delta) tb++;
  *lb = bits_for(b.L);
  if (tb + b.tshift + *lb > 63) return 0;  // bit 63 of an entry marks a pushed IHAVE (gs_lpull_kernel.h)
  uint64_t need = (uint64_t)K * N * lpull_stride(b) * 8 + (uint64_t)N * b.L * 2 + (uint64_t)N * (LP_SW + LP_FW) * 4;
  uint64_t have = (uint64_t)c.d_lblk.n * 8 + (uint64_t)c.d_flane.n * 2 + (uint64_t)(c.d_lst.n + c.d_lfin.n) * 4;
  if (gos) {  // sender planes and entries
    need += (uint64_t)N * b.L * 8 + (uint64_t)N * LP_FW * 4;
    have += (uint64_t)c.d_gse.n * 8 + (uint64_t)c.d_gpl.n * 4;
  }
  if (need > have) {
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) != hipSuccess || need - have + (4ull << 30) > fr) return 0;
  }
  return (uint32_t)K;
}

// What a batch on the list pull path (run_lpull_batch) can carry.
// Lazy gossip inside the passes (GOS): the batch's heartbeats relative to
// every t_pub (lockstep) and the IHAVE travel bounds.
struct GosRun {
  uint64_t rel0, hb;
};
// Churn on the list pass (gs_cpull.h): the batch's first epoch and epoch count,
// the common offset of its publishes into their epochs, heartbeat 0's relative epoch.
struct ChnRun {
  uint64_t E0, r0;
  uint32_t cE, ghoff;
  uint32_t par;  // the table set (Ctx::ct) chn_begin filled for the batch
};

// Batch slices (Run::try_slices, gs_run.h): S batches of the same shape as one pass over S
// copies of the graph, slice j's rows j * N1 + peer; the copies' mesh rows,
// reverse positions and stages (d_smesh, d_srpos, d_sstage), the publishers
// as slice rows (spub, k_lpull / k_lpub) and as peers (lpub, k_seed).
struct Slices {
  uint32_t S, N1;
  const uint32_t* spub;
  const uint32_t* lpub;
};

// No-log batch (k_lpull<1, CH, .., NOLOG>): the caller reads only
// counters, so the passes write no final log and complete the batch themselves.
// on: asked for by the caller (PathPlan::nolog's rule, gs_run.h). After the batch: inexact = a final
// time reached 2^38 ns, where the passes' 32-bit ms are not k_lsum's (the counters are restored
// and the caller runs the batch again with its log); else tmax / deliv, the batch's latest
// final time after t_pub and its deliveries, for the no-op proof of a lockstep batch.
struct NoLog {
  bool on = false, inexact = false;
  uint64_t tmax = 0, deliv = 0;
};
constexpr uint64_t NOLOG_TLIM = 1ull << 38;  // (t >> 6) / 15625 in 32 bits

// What one list-pass batch runs with: dense rows for its reader (k_lfinal), IDONTWANT
// (dense final keys all along), lazy gossip and churn inside the passes, batch slices,
// the no-log form. part: the rows are a part's (gs_part.h), row r is peer u0 + r and the pass
// reads its neighbours' records from the packed exchange buffers (d_rpk, d_roffg, d_rcg).
struct LpOpts {
  bool dense = false, idw = false, part = false;
  uint32_t u0 = 0;
  const GosRun* gos = nullptr;
  const ChnRun* chn = nullptr;
  const Slices* sl = nullptr;
  NoLog* nl = nullptr;
};

// The list pass's grid for `rows` rows (a part passes the rows it owns).
// 40 KB of LDS per block: 4 blocks (16 waves, 16 rows in flight) resident per
// CU. Large graphs launch up to 16 blocks per CU so that a pass's tail is
// made of short blocks, keeping >= 32 rows per wave (1M peers: 54.3 ms per
// step at 4 blocks per CU, 53.1 at 16; 100k peers: 7.8 ms at 16, 6.8 at 4;
// profiles/r02_v7/lpull_grid_sweep.txt)
// a power of two: 15 per CU measured 56.4 ms against 53.1 at 16 on one box
static unsigned lpull_grid(uint64_t rows, int cus) {
  uint64_t bpc = 4;  // whole blocks per CU
  while (bpc < 16 && rows >= (uint64_t)cus * PULL_WAVES * 32 * bpc * 2) bpc *= 2;
  return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((rows + PULL_WAVES - 1) / PULL_WAVES, (uint64_t)cus * bpc));
}

// Test knobs, read per batch: GS_LPULL_CAP's small lists force the overflow re-run;
// GS_LPULL_CAP_BATCHES (comma-separated 0-based indices of the run's batch loop, in run
// order: after the class regrouping) keeps the cap to the listed batches (by_batch: not for a
// part, c.run_batch is gs_run's)
static uint32_t lpull_cap(const Ctx& c, uint32_t ls, bool by_batch) {
  long cap = env_int("GS_LPULL_CAP", (long)ls);
  const char* capb = by_batch ? getenv("GS_LPULL_CAP_BATCHES") : nullptr;
  if (capb && *capb) {
    bool listed = false;
    for (const char* q = capb; *q && !listed;) {
      char* end = nullptr;
      const unsigned long long v = strtoull(q, &end, 10);
      listed = end != q && v == c.run_batch;
      q = end != q ? end : q + 1;
      while (*q == ',' || *q == ' ') q++;
    }
    if (!listed) cap = (long)ls;
  }
  return (uint32_t)std::min<long>(std::max(1l, cap), (long)ls);
}

// The seed list's entries at the most: one per (target, fragment) of every publish (flood: every connection).
static uint64_t lpull_scap(const Ctx& c, const Batch& b, const LpOpts& o) {
  return (uint64_t)(o.sl ? o.sl->S : 1) * b.B * b.Fe * std::max<uint64_t>(c.max_degree, MESH_W);
}

// The batch's buffers for the pass's N rows, cleared state and saved counters, then its seeds.
// Both drivers' set-up: run_lpull_batch's for the whole graph (or its slices), part_lp_begin's
// (gs_part.h) for a part's rows.
static void lpull_begin(Ctx& c, const Batch& b, uint32_t K, const LpOpts& o, uint32_t N) {
  const uint32_t N0 = c.cfg.peers;
  const Slices* sl = o.sl;
  hipStream_t s = c.stream;
  const size_t NL = (size_t)N * b.L;
  const uint64_t scap = lpull_scap(c, b, o);
  c.d_lrec.alloc((o.chn ? 4 : 2) * NL);  // churn records are 16 B
  c.d_lcnt.alloc(2 * (size_t)N);
  c.d_lblk.alloc((size_t)K * N * lpull_stride(b));
  c.d_lst.alloc((size_t)N * LP_SW);
  c.d_lfin.alloc((size_t)N * LP_FW);
  if (!(o.nl && o.nl->on)) c.d_flane.alloc(NL);
  ensure_rpos(c);
  if (sl) {  // the graph copies of the slices (rebuilt per group: a few MB)
    c.d_smesh.alloc((size_t)N * MESH_W);
    c.d_srpos.alloc((size_t)N * MESH_W);
    c.d_sstage.alloc(N);
    k_srep<<<(unsigned)(((uint64_t)N * MESH_W + TB - 1) / TB), TB, 0, s>>>(
        N0, sl->S, c.d_mesh.p, c.d_rpos.p, c.d_stage.p, c.d_smesh.p, c.d_srpos.p, c.d_sstage.p);
    GS_HIP(hipGetLastError());
  }
  GS_HIP(hipMemsetAsync(c.d_lst.p, 0, (size_t)N * LP_SW * 4, s));
  GS_HIP(hipMemsetAsync(c.d_lfin.p, 0, (size_t)N * LP_FW * 4, s));
  pctrl_reset(c);
  c.d_lp_save.alloc(C_COUNT);
  GS_HIP(hipMemcpyAsync(c.d_lp_save.p, c.d_counters.p, C_COUNT * 8, hipMemcpyDeviceToDevice, s));
  c.d_skey.alloc(scap);
  c.d_slane.alloc(scap);
  c.d_scnt.alloc(1);
  GS_HIP(hipMemsetAsync(c.d_scnt.p, 0, 4, s));
  if (sl)
    for (uint32_t j = 0; j < sl->S; j++)
      launch_seed(c, b, 0, N0, c.d_pctrl.p + PS_SEED_MIN, nullptr, true, sl->lpub + (size_t)j * b.B, j * N0);
  else
    launch_seed(c, b, o.u0, N, c.d_pctrl.p + PS_SEED_MIN, nullptr, true);
}

// The passes' arguments but for lazy gossip's (lpull_gos_args); churn: its per-row state, cleared.
static LPullArgs lpull_args(Ctx& c, const Batch& b, uint32_t K, uint32_t lb, const LpOpts& o, uint32_t N) {
  const Slices* sl = o.sl;
  const ChnRun* chn = o.chn;
  hipStream_t s = c.stream;
  LPullArgs la{};
  la.keys = c.d_keys.p; la.flane = c.d_flane.p; la.busy = c.d_busy.p; la.blk = c.d_lblk.p;
  if (o.nl && o.nl->on) la.keys = nullptr, la.flane = nullptr;  // (k_lpub's sign that no log is kept)
  la.st = c.d_lst.p; la.fin = c.d_lfin.p;
  la.lrec = c.d_lrec.p; la.lcnt = c.d_lcnt.p; la.rpos = c.d_rpos.p;
  la.mesh = c.d_mesh.p; la.pub = c.d_pub.p; la.stage = c.d_stage.p; la.tables = c.d_tables.p;
  if (sl) {
    la.mesh = c.d_smesh.p;
    la.rpos = c.d_srpos.p;
    la.stage = c.d_sstage.p;
    la.pub = sl->spub;
    la.rN = c.cfg.peers;
  }
  const uint64_t grain = pull_grain(b.tshift);
  la.ctrl = c.d_pctrl.p; la.counters = c.d_counters.p; la.delta = b.delta / grain * grain;
  la.tmax = b.tmax - grain;
  la.N = N; la.B = b.B; la.L = b.L; la.S = c.S; la.sb = b.sb; la.tshift = b.tshift;
  la.K = K; la.lb = lb; la.dG = (uint32_t)(la.delta / grain);
  la.idw = o.idw ? 1u : 0u;
  la.rmax = lpull_rmax(b);
  la.u0 = o.u0;
  if (o.part) la.rpk = c.d_rpk.p, la.roff = c.d_roffg.p, la.rcg = c.d_rcg.p;
  la.ghk = ~0u;
  la.gsw = ~0u;  // (frozen mesh: every heartbeat's IHAVEs are decided by the receivers)
  if (chn) {  // churn (gs_cpull.h): the tables k_cprep built for this batch
    la.ccol = c.d_ccol.p;
    la.cpos = c.d_cpos.p;
    const Ctx::ChnTables& t = c.ct[chn->par & 1];
    la.cmm = t.cmm.p;
    la.cgt = t.cgt.p;
    la.coff = t.coff.p;
    la.cq = t.cq.p;
    la.pubok = t.pubok.p;
    la.calive = t.calive.p;
    c.d_luni.alloc(2 * (size_t)N);
    la.luni = c.d_luni.p;
    c.d_gnz.alloc(N);
    la.gnz = c.d_gnz.p;
    c.d_gtag.alloc(N);
    GS_HIP(hipMemsetAsync(c.d_gtag.p, 0, (size_t)N * 2, s));  // GC_BK counts from 1 per batch
    la.gtag = c.d_gtag.p;
    c.d_gpc.alloc(N);
    GS_HIP(hipMemsetAsync(c.d_gpc.p, 0, (size_t)N * 4, s));
    la.gpc = c.d_gpc.p;
    la.cr0 = chn->r0;
    la.chb = c.cfg.heartbeat_ns;
    la.cE = chn->cE;
    la.chz = c.cfg.churn_horizon;
    la.ghoff = chn->ghoff;
    la.ghk = c.cfg.churn_horizon - chn->ghoff;
    // heartbeats from gsw on push their IHAVEs to the targets that may still need
    // them (GS_GOSSIP_SWITCH, any value is exact). Off by default: at config #3's
    // shape the pushes cost more in k_gsend than the plane scans they replace
    // (121 ms per batch without, 129 ms from heartbeat 4 on, 193 ms from 1 on)
    la.gsw = (uint32_t)env_int("GS_GOSSIP_SWITCH", ~0u);
  }
  la.ls = lpull_stride(b);
  la.lcap = lpull_cap(c, la.ls, !o.part);
  return la;
}

// The seeds into the candidate lists (k_lseed), the rows whose emit step needs the publishers
// (k_lpubnb sets LP_PUB; not for a part, whose rows that kernel would index by global peer id:
// it runs with pubw = 0) and the publishers' own lanes into the logs (k_lpub).
static void lpull_seed(Ctx& c, const Batch& b, const LpOpts& o, LPullArgs& la) {
  const Slices* sl = o.sl;
  hipStream_t s = c.stream;
  const uint64_t scap = lpull_scap(c, b, o);
  k_lseed<<<(unsigned)std::max<uint64_t>(1, std::min<uint64_t>((scap + TB - 1) / TB, (uint64_t)c.num_cus * 4)), TB, 0, s>>>(
      la, c.d_skey.p, c.d_slane.p, c.d_scnt.p);
  if (!o.part) {
    la.pubw = 1;
    const uint64_t nm = (uint64_t)(sl ? sl->S : 1u) * b.B, width = (o.chn ? CELL_W : MESH_W) + 1;
    k_lpubnb<<<(unsigned)((nm * width + TB - 1) / TB), TB, 0, s>>>(la, (uint32_t)nm);
  }
  for (uint32_t j = 0; j < (sl ? sl->S : 1u); j++) {  // (a slice's publishers are its rows)
    LPullArgs lj = la;
    if (sl) lj.pub = sl->spub + (size_t)j * b.B;
    k_lpub<<<(b.B * b.Fe + 255) / 256, 256, 0, s>>>(lj, b.Fe);
  }
  GS_HIP(hipGetLastError());
}

// GOS: sender planes, row-done bits, heartbeat control (gs_lpull_kernel.h)
static void lpull_gos_args(Ctx& c, const Batch& b, const LpOpts& o, LPullArgs& la) {
  const uint32_t N = la.N;
  hipStream_t s = c.stream;
  ensure_csrpos(c);
  c.d_gpl.alloc((size_t)N * LP_FW);
  c.d_gse.alloc((size_t)N * b.L);
  c.d_rowdone.alloc(((size_t)N + 31) / 32);
  c.d_gctl.alloc(GC_WORDS);
  GS_HIP(hipMemsetAsync(c.d_rowdone.p, 0, ((size_t)N + 31) / 32 * 4, s));
  GS_HIP(hipMemsetAsync(c.d_gctl.p, 0, GC_WORDS * 8, s));
  GS_HIP(hipMemcpyAsync(c.d_gctl.p + GC_FD0, c.d_counters.p + C_FD, 8, hipMemcpyDeviceToDevice, s));
  GS_HIP(hipMemcpyAsync(c.d_gctl.p + GC_FDP, c.d_counters.p + C_FD, 8, hipMemcpyDeviceToDevice, s));
  la.grel0 = o.gos->rel0;
  la.ghb = o.gos->hb;
  la.glat_min = b.lat_min;
  la.glat_max = b.lat_max;
  // lanes that can be final, less the publishers'
  la.gnf = (uint64_t)(o.sl ? o.sl->S : 1u) * b.B * b.Fe * (c.cfg.peers - 1);
  la.F = b.F;
  la.collide = b.collide ? 1u : 0u;
  la.gseed = c.cfg.seed;
  la.ghist = c.cfg.history_gossip;
  la.gd_lazy = c.cfg.d_lazy;
  la.ggf = c.cfg.gossip_factor_milli;
  la.gctl = c.d_gctl.p;
  la.gpl = c.d_gpl.p;
  la.gse = c.d_gse.p;
  la.rowdone = c.d_rowdone.p;
  la.row = c.d_row.p;
  la.col = c.d_col.p;
  la.flags = c.d_flags.p;
  la.csrpos = c.d_csrpos.p;
  la.habs0 = c.d_habs0.p;
}

// Passes in groups of 8 until one decides DONE (one host read of the control slots, the
// error word and, no-log, the batch words per group) or a list is lost. Returns the
// passes run; c.h_pinned[HP_LP_ERR] and [HP_LP_BATCH ..] hold the last read of those.
static uint32_t lpull_passes(Ctx& c, uint32_t FP, LPullArgs& la, unsigned grid, bool gos, bool nolog) {
  hipStream_t s = c.stream;
  uint32_t pass = 0;
  for (;;) {
    for (uint32_t q = 0; q < 8; q++) {
      la.pass = pass++;
      timed_pass(c, s, [&] { lpull_dispatch(FP, la, grid, s, gos, nolog); });
    }
    GS_HIP(hipGetLastError());
    GS_HIP(hipMemcpyAsync(c.h_pinned, c.d_pctrl.p, PS_SLOTS * PS_WORDS * 8, hipMemcpyDeviceToHost, s));
    GS_HIP(hipMemcpyAsync(c.h_pinned + HP_LP_ERR, c.d_counters.p + C_ERR, 8, hipMemcpyDeviceToHost, s));  // same sync
    if (nolog)  // (and the batch words: final once DONE is read)
      GS_HIP(hipMemcpyAsync(c.h_pinned + HP_LP_BATCH, c.d_pctrl.p + LP_CT_TMAX, 16, hipMemcpyDeviceToHost, s));
    if (c.pass_poll) c.pass_poll();  // (while these passes run: the next batch's epoch chain is enqueued)
    GS_HIP(hipStreamSynchronize(s));
    const uint64_t* sl = last_slot(c, pass);
    static const bool dbg_pass = getenv("GS_DEBUG_PASSES") != nullptr;
    if (dbg_pass && pass % 256 == 0)
      fprintf(stderr, "[gs] pass %u: mode %llu lo %llu records %llu min %llx err %llx\n", pass,
              (unsigned long long)sl[PS_MODE], (unsigned long long)sl[PS_LO], (unsigned long long)sl[PS_RECORDS],
              (unsigned long long)sl[PS_MIN], (unsigned long long)c.h_pinned[HP_LP_ERR]);
    // a batch's passes end (every window of its lifetime emitted); a count far
    // past that is a bug, reported instead of looping
    if (pass > (1u << 20)) c.fail(GS_ERANGE, "internal: the list pass did not finish in 2^20 passes");
    if (sl[PS_MODE] == PM_DONE) break;
    if (c.h_pinned[HP_LP_ERR] & (ERR_LIST | ERR_RING)) break;  // lost already: stop early, re-run on k_pull
  }
  return pass;
}

// One batch on the list pull path: k_seed appends the first sends to a seed
// list (no dense key table to reset), k_lseed files them into the candidate
// lists, k_lpub logs the publishers' own lanes, then passes in chunks of 8 as
// on the k_pull path; completion reads the final logs (k_lcomplete) unless a
// caller needs dense rows (k_lfinal).
// Returns false (counters restored) when a list overflowed: the caller re-runs
// the batch on k_pull.
static bool run_lpull_batch(Ctx& c, const Batch& b, uint32_t K, uint32_t lb, const LpOpts& o) {
  const Slices* sl = o.sl;
  NoLog* nl = o.nl;
  const uint32_t N = sl ? sl->S * c.cfg.peers : c.cfg.peers;  // the pass's rows
  hipStream_t s = c.stream;
  const bool nolog = nl && nl->on;
  if (nolog && (o.dense || o.idw || o.gos || o.chn || sl || b.FP != 1))
    c.fail(GS_EINVAL, "internal: no-log list pass asked for a batch it cannot take");
  lpull_begin(c, b, K, o, N);
  LPullArgs la = lpull_args(c, b, K, lb, o, N);
  const unsigned grid = lpull_grid(N, c.num_cus);
  lpull_seed(c, b, o, la);
  if (o.gos) lpull_gos_args(c, b, o, la);
  c.stats.relax_launches += lpull_passes(c, b.FP, la, grid, o.gos != nullptr, nolog);
  if (c.h_pinned[HP_LP_ERR] & (ERR_LIST | ERR_RING)) {  // the error word as of the last pass read
    GS_HIP(hipMemcpyAsync(c.d_counters.p, c.d_lp_save.p, C_COUNT * 8, hipMemcpyDeviceToDevice, s));
    return false;
  }
  static_assert(LP_CT_DELIV == LP_CT_TMAX + 1, "the batch words' host copy");
  const uint64_t* bw = c.h_pinned + HP_LP_BATCH;  // LP_CT_TMAX, LP_CT_DELIV as of the last pass read
  static const bool dbg_comp = getenv("GS_DEBUG_COMPLETION") != nullptr;
  if (nolog && bw[0] >= NOLOG_TLIM) {  // the in-pass ms were not exact: restored as after an overflow
    GS_HIP(hipMemcpyAsync(c.d_counters.p, c.d_lp_save.p, C_COUNT * 8, hipMemcpyDeviceToDevice, s));
    nl->inexact = true;
    if (dbg_comp)
      fprintf(stderr, "[lp] batch %llu: no-log pass discarded (a final time >= 2^38 ns)\n",
              (unsigned long long)c.run_batch);
    return false;
  }
  c.stats.list_pull_batches++;
  if (dbg_comp)
    fprintf(stderr, "[lp] batch %llu: completion %s\n", (unsigned long long)c.run_batch,
            nolog ? "in-pass (no log)" : o.idw ? "dense keys (idontwant)" : o.dense ? "dense rows (k_lfinal)" : "final log");
  if (nolog) {  // nothing to complete: no log was written, the counters are added
    nl->tmax = bw[0];
    nl->deliv = bw[1];
    c.keys_none = true;
    return true;
  }
  if (o.idw) return true;  // the final keys are dense rows already
  if (o.dense) {  // a sink, the traffic pass or a fragment group needs [N][L] rows
    k_lfinal<<<grid, TB, 0, s>>>(la);
    GS_HIP(hipGetLastError());
  } else {
    c.keys_log = true;
  }
  return true;
}

#ifdef GS_PULL_PROF
extern "C" int gs_debug_pull_prof(uint64_t* out) {  // 32 passes x 8 slots; read and clear
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_pull_prof), sizeof(g_pull_prof)) != hipSuccess) return -1;
  static const uint64_t zero[32 * 8] = {};
  return hipMemcpyToSymbol(HIP_SYMBOL(g_pull_prof), zero, sizeof(g_pull_prof)) == hipSuccess ? 0 : -1;
}
#endif

// Blocks per CU of the split (push) path's scan / frontier / gossip grid: 4
// measured best on config #3 (k_scan 177 -> 136 us, k_frontier 65 -> 38 us per
// bucket vs 16; 1-2 and 32-64 slower, profiles/r01_v10/c3_grid_sweep.txt).
constexpr uint32_t SPLIT_BLOCKS_PER_CU = 4;

// Lazy gossip is a no-op for message q when every non-publisher completed and
// the last completion lies before the first IHAVE can arrive: the earliest
// gossip heartbeat is rel0 (the first one at or after t_pub; every gossiping
// peer holds the message by then at the latest) and an IHAVE travels at least
// the smallest link latency. Then every IHAVE target has seen the message, no
// IWANT is sent and no key changes.
static bool gossip_noop(const Batch& b, const uint64_t* ms, const std::vector<uint64_t>& rel0) {
  for (uint32_t q = 0; q < b.B; q++)
    if (ms[(size_t)q * MS_COLS + MS_UNDEL] || ms[(size_t)q * MS_COLS + MS_TMAX] >= rel0[q] + b.lat_min) return false;
  return true;
}

// The churn list pass's per-batch tables (gs_cpull.h) for epochs [E0, E0 + cE)
// and the batch's publish epochs q0 (lanes). chn_begin before the epoch chain
// runs; chn_chunks then puts k_cprep of every chunk of 64 epochs whose epochs
// the chain has enqueued on the side stream (the chain is latency-bound, the
// target selection compute-bound: they overlap), chn_end the rest, the
// offline lanes per relative epoch (k_coff) and the join.
struct ChnPrep {
  uint64_t E0 = 0;
  uint32_t cE = 0, cW = 0, next = 0, par = 0;  // par: the table set (Ctx::ct) this batch fills
  bool offe = false;
  size_t nev = 0;
  hipStream_t s = nullptr;  // the stream the epoch chain runs on (chunk events are recorded there)
  CPrepArgs pa{};
  unsigned grid = 1;
};
static hipEvent_t cp_event(Ctx& c, uint32_t par, size_t i) {
  std::vector<hipEvent_t>& v = c.cp_ev[par & 1];
  while (v.size() <= i) {
    hipEvent_t e;
    GS_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    v.push_back(e);
  }
  return v[i];
}
static void chn_begin(Ctx& c, ChnPrep& cp, uint32_t par, hipStream_t s, uint64_t E0, uint32_t cE, const uint64_t* q0,
                      const gs_publish* sched, uint32_t B, uint32_t FP) {
  const uint32_t N = c.cfg.peers, H = c.cfg.churn_horizon, R = c.ring_R;
  const uint32_t cW = (cE + 63) / 64;
  Ctx::ChnTables& t = c.ct[par & 1];
  if (!c.cell_valid) {
    c.d_ccol.alloc((size_t)N * CELL_W);
    c.d_cpos.alloc((size_t)N * CELL_W);
    k_cell<<<(unsigned)(((uint64_t)N * CELL_W + TB - 1) / TB), TB, 0, s>>>(N, c.d_row.p, c.d_col.p, c.d_rev.p,
                                                                          c.d_stage.p, c.d_ccol.p, c.d_cpos.p);
    GS_HIP(hipGetLastError());
    c.cell_valid = true;
  }
  std::vector<uint32_t> cq(B);
  std::vector<uint8_t> ok(B);
  for (uint32_t q = 0; q < B; q++) {
    cq[q] = (uint32_t)(q0[q] - E0);
    ok[q] = !c.offline(sched[q].publisher, q0[q]);
  }
  std::vector<uint16_t> alive(64, 0);  // lane j: bit q = lane q*64 + j published (lane l: message l / FP)
  for (uint32_t l = 0; l < B * FP; l++)
    if (ok[l / FP]) alive[l & 63] |= (uint16_t)(1u << (l >> 6));
  t.cq.alloc(c.cfg.batch);
  t.pubok.alloc(c.cfg.batch);
  t.calive.alloc(LP_FW);
  GS_HIP(hipMemcpyAsync(t.cq.p, cq.data(), B * 4, hipMemcpyHostToDevice, s));
  GS_HIP(hipMemcpyAsync(t.pubok.p, ok.data(), B, hipMemcpyHostToDevice, s));
  GS_HIP(hipMemcpyAsync(t.calive.p, alive.data(), 128, hipMemcpyHostToDevice, s));
  t.offe.alloc((size_t)N * cW);
  t.cmm.alloc((size_t)N * cE);
  t.cgt.alloc((size_t)N * cE);
  t.coff.alloc((size_t)(H + 2) * N * LP_FW);
  GS_HIP(hipStreamSynchronize(s));  // cq / ok / alive die here
  cp.E0 = E0;
  cp.cE = cE;
  cp.cW = cW;
  cp.next = 0;
  cp.par = par & 1;
  cp.offe = false;
  cp.nev = 0;
  cp.s = s;
  CPrepArgs& pa = cp.pa;
  pa = CPrepArgs{};
  pa.ccol = c.d_ccol.p; pa.ring_mm = c.d_ring_mm.p; pa.offe = t.offe.p; pa.cq = t.cq.p;
  pa.cmm = t.cmm.p; pa.cgt = c.cfg.lazy_gossip ? t.cgt.p : nullptr; pa.coff = t.coff.p;
  pa.E0 = E0; pa.N = N; pa.R = R; pa.cE = cE; pa.cW = cW; pa.B = B; pa.H = H; pa.FP = FP;
  pa.seed = c.cfg.seed; pa.d_lazy = c.cfg.d_lazy; pa.gf_milli = c.cfg.gossip_factor_milli;
  ensure_cus(c);
  cp.grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((N + 3) / 4, (uint64_t)std::max(c.num_cus, 1) * 8));
}
// The chunks whose epochs are all <= h_done (every remaining one with `all`).
static void chn_chunks(Ctx& c, ChnPrep& cp, uint64_t h_done, bool all) {
  uint32_t c1 = cp.next;
  while (c1 < cp.cW && (all || cp.E0 + std::min<uint64_t>(64ull * (c1 + 1), cp.cE) - 1 <= h_done)) c1++;
  if (c1 == cp.next) return;
  const uint32_t N = c.cfg.peers, w64 = (N + 63) / 64;
  hipStream_t side = side_stream(c);
  const hipEvent_t e = cp_event(c, cp.par, cp.nev++);
  GS_HIP(hipEventRecord(e, cp.s ? cp.s : c.stream));  // (in line: the stream churn_ring runs the chain on)
  GS_HIP(hipStreamWaitEvent(side, e, 0));
  if (!cp.offe) {  // every epoch's offline bits are in the ring once the chain's run started
    k_offe<<<dim3(w64, cp.cW), 64, 0, side>>>(N, c.d_ring_off.p, w64, c.ring_R, cp.E0, cp.cE, cp.cW,
                                              c.ct[cp.par].offe.p);
    k_coff<<<cp.grid, TB, 0, side>>>(cp.pa);  // the offline lanes need no mesh: beside the chain too
    cp.offe = true;
  }
  cp.pa.c0 = cp.next;
  cp.pa.c1 = c1;
  k_cprep<<<cp.grid, TB, 0, side>>>(cp.pa);
  GS_HIP(hipGetLastError());
  cp.next = c1;
}
// The rest of the tables, then `to` waits for them (nullptr: cp.s, and the host too).
static void chn_end(Ctx& c, ChnPrep& cp, hipStream_t to = nullptr) {
  chn_chunks(c, cp, 0, true);
  const hipEvent_t e = cp_event(c, cp.par, cp.nev++);
  GS_HIP(hipEventRecord(e, side_stream(c)));
  GS_HIP(hipStreamWaitEvent(to ? to : c.stream, e, 0));
  GS_HIP(hipGetLastError());
  if (to) return;
  const uint32_t N = c.cfg.peers, R = c.ring_R, cE = cp.cE;
  const uint64_t E0 = cp.E0;
  const Ctx::ChnTables& t = c.ct[cp.par];
  hipStream_t s = c.stream;
  GS_HIP(hipStreamSynchronize(s));
  if (getenv("GS_DEBUG_CHN")) {  // diagnostic: the tables against the ELL ring and offline_draw
    std::vector<uint64_t> row(N + 1), cmm((size_t)N * cE), cge((size_t)N * cE);
    std::vector<uint32_t> col(c.nnz), ell((size_t)R * N * MESH_W);
    GS_HIP(hipMemcpy(row.data(), c.d_row.p, (N + 1) * 8, hipMemcpyDeviceToHost));
    GS_HIP(hipMemcpy(col.data(), c.d_col.p, c.nnz * 4, hipMemcpyDeviceToHost));
    GS_HIP(hipMemcpy(cmm.data(), t.cmm.p, cmm.size() * 8, hipMemcpyDeviceToHost));
    GS_HIP(hipMemcpy(cge.data(), t.cgt.p, cge.size() * 8, hipMemcpyDeviceToHost));
    GS_HIP(hipMemcpy(ell.data(), c.d_ring_mesh.p, ell.size() * 4, hipMemcpyDeviceToHost));
    uint64_t bad_mm = 0, bad_ge = 0;
    for (uint32_t w = 0; w < N; w++)
      for (uint32_t e = 0; e < cE; e++) {
        const uint64_t E = E0 + e;
        const uint32_t* er = &ell[((size_t)(E % R) * N + w) * MESH_W];
        uint64_t mm = 0, ge = 0;
        const bool woff = c.offline(w, E);
        std::vector<std::pair<uint64_t, uint32_t>> cand;
        for (uint64_t x = row[w]; x < row[w + 1]; x++) {
          bool in = false;
          for (uint32_t j = 0; j < MESH_W; j++) in |= er[j] != EMPTY && (er[j] & 0xFFFFFFu) == col[x];
          if (in) mm |= 1ull << (x - row[w]);
          else if (!woff && !c.offline(col[x], E))
            cand.push_back({rng(c.cfg.seed, P_GOSSIP, w, (uint32_t)E, col[x]), (uint32_t)(x - row[w])});
        }
        std::sort(cand.begin(), cand.end(), [&](const std::pair<uint64_t, uint32_t>& p1, const std::pair<uint64_t, uint32_t>& p2) {
          return p1.first < p2.first || (p1.first == p2.first && col[row[w] + p1.second] < col[row[w] + p2.second]);
        });
        uint32_t r = (uint32_t)(((uint64_t)cand.size() * c.cfg.gossip_factor_milli) / 1000);
        if (r < c.cfg.d_lazy) r = c.cfg.d_lazy;
        if (r > cand.size()) r = (uint32_t)cand.size();
        for (uint32_t q = 0; q < r; q++) ge |= 1ull << cand[q].second;
        if (!c.cfg.lazy_gossip) ge = 0;
        if (mm != cmm[(size_t)w * cE + e] && bad_mm++ < 5)
          fprintf(stderr, "[chn] mm w %u E %llu dev %llx host %llx\n", w, (unsigned long long)E,
                  (unsigned long long)cmm[(size_t)w * cE + e], (unsigned long long)mm);
        if (ge != cge[(size_t)w * cE + e] && bad_ge++ < 5)
          fprintf(stderr, "[chn] ge w %u E %llu dev %llx host %llx\n", w, (unsigned long long)E,
                  (unsigned long long)cge[(size_t)w * cE + e], (unsigned long long)ge);
      }
    fprintf(stderr, "[chn] E0 %llu cE %u: mm mismatches %llu, ge mismatches %llu\n", (unsigned long long)E0, cE,
            (unsigned long long)bad_mm, (unsigned long long)bad_ge);
  }
}

// The churn snapshot ring: R slots of per-epoch meshes, offline
// bitsets and (lazy gossip) inverse IHAVE lists, sized once per context.
static void ensure_ring(Ctx& c) {
  if (c.ring_R) return;
  const uint32_t N = c.cfg.peers, Bmax = c.cfg.batch;
  const bool gossip = c.cfg.lazy_gossip != 0;
  const uint64_t w64 = ((uint64_t)N + 63) / 64;
  const uint64_t per_slot = (uint64_t)N * MESH_W * 4 + w64 * 8 + (gossip ? (uint64_t)N * (GT_IN * 4 + 4) : 0) +
                            (uint64_t)N * 8;
  // test knob: a small budget forces batch cuts at the ring size
  const uint64_t budget = (uint64_t)env_int("GS_RING_BUDGET_MB", 16 << 10) << 20;
  const uint64_t want = (uint64_t)Bmax + c.cfg.churn_horizon + 1;
  c.ring_R = (uint32_t)std::min<uint64_t>(want, std::max<uint64_t>(c.cfg.churn_horizon + 2, budget / per_slot));
  c.d_ring_mesh.alloc((size_t)c.ring_R * N * MESH_W);
  c.d_ring_off.alloc((size_t)c.ring_R * w64);
  if (c.max_degree <= CELL_W) c.d_ring_mm.alloc((size_t)c.ring_R * N);  // the churn list pass's meshes
  if (gossip) c.d_ring_in.alloc((size_t)c.ring_R * N * GT_IN);  // inverse IHAVE lists (ring_in_lists)
}

#include "gs_run.h"

// Schedules that are not lockstep: the churn list pass and the
// gossip inside the list pass need every message of a batch at the same
// offset r = (t_pub - hb_phase) mod heartbeat (its heartbeats and epoch
// boundaries are then one relative time for all lanes). run.sh's free
// message_delay (run.sh:36; 1500 ms gives two offsets) and arbitrary POST
// /publish sequences (main.rs:146-221) are not. Messages are independent
// given the mesh of each epoch, so the run takes each group of consecutive
// messages a batch could hold (same size and chunk count, <= the batch size,
// churn: its epochs in the ring) in offset-class order — a batch per class,
// each lockstep — and hands the results back in schedule order. Classes per
// group are capped (at 64; a group with more keeps its
// order); streaming sinks (on_block, on_lat) and device sinks keep the order
// too. GS_CLASS_SPLIT=0 turns the regrouping off.
static bool class_plan(Ctx& c, const gs_publish* sched, uint64_t n, const gs_result_sink* sink,
                       std::vector<uint64_t>& perm, std::vector<uint8_t>& cut) {
  const bool churn = c.cfg.churn_ppm != 0, gossip = c.cfg.lazy_gossip != 0;
  if ((!churn && !gossip) || n < 2 || c.sink_dev) return false;
  if (sink && (sink->on_block || sink->on_lat)) return false;
  if (env_off("GS_CLASS_SPLIT")) return false;
  constexpr uint64_t cmax = 64;
  for (uint64_t i = 0; i < n; i++)
    if (sched[i].t_pub_ns < c.cfg.hb_phase_ns) return false;  // (Run reports what it must)
  if (churn) ensure_ring(c);
  perm.resize(n);
  cut.assign(n, 0);
  bool any = false;
  for (uint64_t g0 = 0; g0 < n;) {  // a group: what one batch could hold
    const uint32_t F0 = frags_of(c, sched[g0]);
    uint64_t lo = 0, hi = 0;
    const uint64_t g1 = same_shape_end(c, sched, n, g0, pull_batch_cap(c.cfg.batch, F0), nullptr, churn, lo, hi);
    std::vector<std::pair<uint64_t, uint64_t>> key(g1 - g0);  // (offset class, message)
    for (uint64_t i = g0; i < g1; i++) key[i - g0] = {hb_pos(c, sched[i].t_pub_ns).off, i};
    std::stable_sort(key.begin(), key.end(), [](const std::pair<uint64_t, uint64_t>& x,
                                                 const std::pair<uint64_t, uint64_t>& y) { return x.first < y.first; });
    uint64_t ncls = 1;
    for (size_t k = 1; k < key.size(); k++) ncls += key[k].first != key[k - 1].first;
    const bool split = ncls > 1 && ncls <= cmax && !(churn && F0 > 1);  // (fragmented churn: the push path)
    cut[g0] = 1;
    for (uint64_t i = g0; i < g1; i++) {
      perm[i] = split ? key[i - g0].second : i;
      if (split && i > g0 && key[i - g0].first != key[i - g0 - 1].first) cut[i] = 1;
    }
    any = any || split;
    g0 = g1;
  }
  return any;
}

void run_messages(Ctx& c, const gs_publish* sched, uint64_t n_msgs, const gs_result_sink* sink) {
  std::vector<uint64_t> perm;
  std::vector<uint8_t> cut;
  if (!class_plan(c, sched, n_msgs, sink, perm, cut)) return Run(c, sched, n_msgs, sink, nullptr).run();
  if (c.msgcost) c.mc_perm = perm;  // the cost table's rows come in class order (msgcost_get)
  std::vector<gs_publish> ps(n_msgs);
  for (uint64_t i = 0; i < n_msgs; i++) ps[i] = sched[perm[i]];
  if (!sink) return Run(c, ps.data(), n_msgs, nullptr, &cut).run();
  // the results in class order, then every row back to its message
  const uint32_t N = c.cfg.peers;
  gs_result_sink ts = *sink;
  std::vector<uint64_t> tc(sink->t_complete_ns ? (size_t)n_msgs * N : 0);
  std::vector<uint8_t> hp(sink->hops ? (size_t)n_msgs * N : 0);
  std::vector<gs_msg_summary> sm(sink->summary ? n_msgs : 0);
  ts.t_complete_ns = sink->t_complete_ns ? tc.data() : nullptr;
  ts.hops = sink->hops ? hp.data() : nullptr;
  ts.summary = sink->summary ? sm.data() : nullptr;
  Run(c, ps.data(), n_msgs, &ts, &cut).run();
  for (uint64_t i = 0; i < n_msgs; i++) {
    const uint64_t m = perm[i];
    if (sink->t_complete_ns) memcpy(sink->t_complete_ns + m * N, tc.data() + i * N, (size_t)N * 8);
    if (sink->hops) memcpy(sink->hops + m * N, hp.data() + i * N, N);
    if (sink->summary) sink->summary[m] = sm[i];
  }
}


#include "gs_part.h"

}  // namespace gs
