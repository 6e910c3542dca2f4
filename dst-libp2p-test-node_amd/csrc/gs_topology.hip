// gs_topology.hip — random ID dialing -> symmetric CSR peer graph on gfx950.
//
// Replaces connect_gossipsub_peers (rust-test-node/src/main.rs:303-389): each
// peer takes a random subset of the other ids and dials min(CONNECTTO+1,
// 2*CONNECTTO, N-1) of them (defect D4); the undirected union of accepted dials
// is the peer graph, with bit F_OUT on (u,w) when u dialed w. Optional
// MAXCONNECTIONS inbound cap (nim gossipsub-queues/main.nim:429).
//
// Kernels are one thread per peer / per dial: this runs once per simulation
// and is HBM-trivial (N*k*~40 B); determinism comes from per-row sorting, not
// from atomic order.
//
// The second half imports a caller's graph instead (gs_set_topology: a CSR;
// gs_set_topology_dials: a dial list): validated on the device,
// built beside the context's graph and swapped in only when it is accepted.
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "gs_import.h"
#include "gs_internal.h"

namespace gs {
namespace {

constexpr int TB = 256;

// Floyd's k-subset of the N-1 other ids, then ordered by a per-(v,id) key.
__global__ __launch_bounds__(TB) void k_dials(uint32_t N, uint32_t k, uint64_t seed,
                                              uint32_t* __restrict__ dial) {
  const uint32_t v = blockIdx.x * TB + threadIdx.x;
  if (v >= N) return;
  uint32_t out[MAX_DIALS];
  uint64_t key[MAX_DIALS];
  const uint64_t n = N - 1;
  for (uint32_t i = 0; i < k; i++) {
    const uint64_t j = n - k + i;
    const uint32_t r = (uint32_t)rand_below(rng(seed, P_DIAL, v, i, 0), j + 1);
    bool dup = false;
    for (uint32_t q = 0; q < i; q++) dup |= (out[q] == r);
    out[i] = dup ? (uint32_t)j : r;
  }
  for (uint32_t i = 0; i < k; i++) {
    const uint32_t id = out[i] < v ? out[i] : out[i] + 1;
    const uint64_t kx = rng(seed, P_DIAL_ORDER, v, id, 0);
    int32_t j = (int32_t)i - 1;
    while (j >= 0 && (key[j] > kx || (key[j] == kx && out[j] > id))) {
      out[j + 1] = out[j];
      key[j + 1] = key[j];
      j--;
    }
    out[j + 1] = id;
    key[j + 1] = kx;
  }
  for (uint32_t i = 0; i < k; i++) dial[(size_t)v * k + i] = out[i];
}

__global__ __launch_bounds__(TB) void k_inbound_count(uint64_t total, uint32_t k,
                                                      const uint32_t* __restrict__ dial,
                                                      uint64_t* __restrict__ cnt) {
  const uint64_t e = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (e >= total) return;
  atomicAdd((unsigned long long*)&cnt[dial[e]], 1ull);
}

__global__ __launch_bounds__(TB) void k_inbound_scatter(uint32_t N, uint32_t k,
                                                        const uint32_t* __restrict__ dial,
                                                        const uint64_t* __restrict__ off,
                                                        uint64_t* __restrict__ fill,
                                                        uint64_t* __restrict__ in) {
  const uint64_t e = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (e >= (uint64_t)N * k) return;
  const uint32_t v = (uint32_t)(e / k), j = (uint32_t)(e % k), t = dial[e];
  const uint64_t pos = atomicAdd((unsigned long long*)&fill[t], 1ull);
  in[off[t] + pos] = ((uint64_t)j << 32) | v;
}

// Acceptor t takes non-mutual inbound dials in (dial index, dialer) order up
// to max(0, cap - k).
__global__ __launch_bounds__(TB) void k_inbound_accept(uint32_t N, uint32_t k, uint32_t quota,
                                                       const uint32_t* __restrict__ dial,
                                                       const uint64_t* __restrict__ off,
                                                       uint64_t* __restrict__ in,
                                                       uint8_t* __restrict__ acc) {
  const uint32_t t = blockIdx.x * TB + threadIdx.x;
  if (t >= N) return;
  const uint64_t b = off[t], e = off[t + 1];
  for (uint64_t i = b + 1; i < e; i++) {  // insertion sort (rows ~ k long)
    const uint64_t x = in[i];
    uint64_t j = i;
    while (j > b && in[j - 1] > x) { in[j] = in[j - 1]; j--; }
    in[j] = x;
  }
  uint32_t taken = 0;
  for (uint64_t i = b; i < e; i++) {
    const uint32_t v = (uint32_t)in[i], j = (uint32_t)(in[i] >> 32);
    bool mutual = false;
    for (uint32_t q = 0; q < k; q++) mutual |= (dial[(size_t)t * k + q] == v);
    if (mutual) continue;
    if (taken < quota) taken++;
    else acc[(size_t)v * k + j] = 0;
  }
}

__global__ __launch_bounds__(TB) void k_deg(uint32_t N, uint32_t k, const uint32_t* __restrict__ dial,
                                            const uint8_t* __restrict__ acc,
                                            uint64_t* __restrict__ deg) {
  const uint64_t e = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (e >= (uint64_t)N * k || !acc[e]) return;
  atomicAdd((unsigned long long*)&deg[e / k], 1ull);
  atomicAdd((unsigned long long*)&deg[dial[e]], 1ull);
}

__global__ __launch_bounds__(TB) void k_half_edges(uint32_t N, uint32_t k,
                                                   const uint32_t* __restrict__ dial,
                                                   const uint8_t* __restrict__ acc,
                                                   const uint64_t* __restrict__ off,
                                                   uint64_t* __restrict__ fill,
                                                   uint64_t* __restrict__ he) {
  const uint64_t e = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (e >= (uint64_t)N * k || !acc[e]) return;
  const uint32_t v = (uint32_t)(e / k), t = dial[e];
  uint64_t p = atomicAdd((unsigned long long*)&fill[v], 1ull);
  he[off[v] + p] = ((uint64_t)t << 1) | 1ull;
  p = atomicAdd((unsigned long long*)&fill[t], 1ull);
  he[off[t] + p] = ((uint64_t)v << 1);
}

// Per-row sort + dedupe (OR of the outbound bits); ndeg[v] = distinct peers.
__global__ __launch_bounds__(TB) void k_sort_dedupe(uint32_t N, const uint64_t* __restrict__ off,
                                                    uint64_t* __restrict__ he,
                                                    uint64_t* __restrict__ ndeg) {
  const uint32_t v = blockIdx.x * TB + threadIdx.x;
  if (v >= N) return;
  const uint64_t b = off[v], e = off[v + 1];
  for (uint64_t i = b + 1; i < e; i++) {
    const uint64_t x = he[i];
    uint64_t j = i;
    while (j > b && he[j - 1] > x) { he[j] = he[j - 1]; j--; }
    he[j] = x;
  }
  uint64_t w = b;
  for (uint64_t i = b; i < e; i++) {
    if (w > b && (he[w - 1] >> 1) == (he[i] >> 1)) { he[w - 1] |= he[i] & 1ull; continue; }
    he[w++] = he[i];
  }
  ndeg[v] = w - b;
}

__global__ __launch_bounds__(TB) void k_compact(uint32_t N, const uint64_t* __restrict__ off,
                                                const uint64_t* __restrict__ he,
                                                const uint64_t* __restrict__ row,
                                                uint32_t* __restrict__ col,
                                                uint8_t* __restrict__ flags,
                                                unsigned* __restrict__ maxdeg) {
  const uint32_t v = blockIdx.x * TB + threadIdx.x;
  if (v >= N) return;
  const uint64_t b = off[v], r = row[v], n = row[v + 1] - r;
  for (uint64_t i = 0; i < n; i++) {
    col[r + i] = (uint32_t)(he[b + i] >> 1);
    flags[r + i] = (uint8_t)(he[b + i] & 1ull);
  }
  atomicMax(maxdeg, (unsigned)n);
}

// rev[e] = index of (w -> u) for e = (u -> w).
__global__ __launch_bounds__(TB) void k_reverse(uint32_t N, const uint64_t* __restrict__ row,
                                                const uint32_t* __restrict__ col,
                                                uint32_t* __restrict__ rev) {
  const uint32_t u = blockIdx.x * TB + threadIdx.x;
  if (u >= N) return;
  for (uint64_t e = row[u]; e < row[u + 1]; e++) {
    const uint32_t w = col[e];
    uint64_t lo = row[w], hi = row[w + 1];
    while (lo < hi) {
      const uint64_t mid = (lo + hi) >> 1;
      if (col[mid] < u) lo = mid + 1; else hi = mid;
    }
    rev[e] = (uint32_t)lo;
  }
}

inline unsigned blocks(uint64_t n) { return (unsigned)((n + TB - 1) / TB); }

// ---- import of a caller's graph (gs_set_topology, gs_set_topology_dials) ----
// (the defect word and the fingerprint's mix: gs_import.h)
enum : uint64_t {  // CSR defects, in reporting order (index: entry; CK_ALONE: peer)
  CK_RANGE = 1, CK_SELF = 2, CK_ORDER = 3, CK_NOREV = 4, CK_NODIALER = 5, CK_ALONE = 6
};
enum : uint64_t {  // dial-list defects, in reporting order (index: dial; DK_ALONE, DK_ENDS: peer)
  DK_RANGE = 1, DK_SELF = 2, DK_ALONE = 3, DK_ENDS = 4, DK_REPEAT = 5
};
constexpr uint32_t IMP_ENDS = 2 * MAX_DEG;  // dial ends of a valid row (every connection a mutual dial)
constexpr uint32_t IMP_THREAD_ENDS = 64;    // rows up to here sort one thread per row

// Thread t checks entry t (t < nnz) and peer t (t < N): the defects of DESIGN.md §2.1, rev as
// k_reverse finds it, the flags cut to F_OUT, the widest row. A row that is not ascending
// reports CK_ORDER, which outranks whatever the search in it then reports.
__global__ __launch_bounds__(TB) void k_import_csr(uint32_t N, uint64_t nnz, const uint64_t* __restrict__ row,
                                                   const uint32_t* __restrict__ col,
                                                   const uint8_t* __restrict__ fin, uint8_t* __restrict__ fout,
                                                   uint32_t* __restrict__ rev, unsigned long long* err,
                                                   unsigned* __restrict__ maxdeg) {
  const uint64_t t = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (t < N) {
    const uint64_t n = row[t + 1] - row[t];
    if (n == 0) imp_defect(err, CK_ALONE, t);
    atomicMax(maxdeg, (unsigned)(n > 0xFFFFFFFFull ? 0xFFFFFFFFull : n));
  }
  if (t >= nnz) return;
  uint32_t lo_u = 0, hi_u = N;  // the row of entry t: row[u] <= t < row[u + 1]
  while (lo_u < hi_u) {
    const uint32_t mid = lo_u + ((hi_u - lo_u) >> 1);
    if (row[mid + 1] <= t) lo_u = mid + 1; else hi_u = mid;
  }
  const uint32_t u = lo_u, w = col[t];
  const uint8_t f = fin[t] & F_OUT;
  fout[t] = f;
  if (w >= N) { imp_defect(err, CK_RANGE, t); return; }
  if (w == u) { imp_defect(err, CK_SELF, t); return; }
  if (t > row[u] && col[t - 1] >= w) imp_defect(err, CK_ORDER, t);
  uint64_t lo = row[w], hi = row[w + 1];
  const uint64_t end = hi;
  while (lo < hi) {
    const uint64_t mid = (lo + hi) >> 1;
    if (col[mid] < u) lo = mid + 1; else hi = mid;
  }
  if (lo >= end || col[lo] != u) { imp_defect(err, CK_NOREV, t); return; }
  rev[t] = (uint32_t)lo;
  if (!f && !(fin[lo] & F_OUT)) imp_defect(err, CK_NODIALER, t);
}

// 64-bit fingerprint of (row_ptr, col, flags & F_OUT): a sum of mixed words, so no order decides
// it. A fixed grid strides over the words and adds one partial sum per wave.
constexpr unsigned FP_BLOCKS = 1024;
__global__ __launch_bounds__(TB) void k_import_fingerprint(uint32_t N, uint64_t nnz, const uint64_t* __restrict__ row,
                                                           const uint32_t* __restrict__ col,
                                                           const uint8_t* __restrict__ flags,
                                                           unsigned long long* fp) {
  const uint64_t n = nnz > (uint64_t)N + 1 ? nnz : (uint64_t)N + 1;
  uint64_t x = 0;
  for (uint64_t t = (uint64_t)blockIdx.x * TB + threadIdx.x; t < n; t += (uint64_t)gridDim.x * TB) {
    if (t <= N) x += imp_mix((t << 1) ^ imp_mix(row[t]));
    if (t < nnz) x += imp_mix(((t << 1) | 1ull) ^ imp_mix(((uint64_t)col[t] << 1) | (flags[t] & F_OUT)));
  }
  for (int d = 32; d; d >>= 1) x += (uint64_t)__shfl_xor((unsigned long long)x, d, 64);
  if ((threadIdx.x & 63) == 0 && x) atomicAdd(fp, (unsigned long long)x);
}

// Dial i: its ids, then one dial end at each of its two peers.
__global__ __launch_bounds__(TB) void k_dial_count(uint32_t N, uint64_t n, const uint32_t* __restrict__ dialer,
                                                   const uint32_t* __restrict__ target, uint64_t* __restrict__ cnt,
                                                   unsigned long long* err) {
  const uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (i >= n) return;
  const uint32_t u = dialer[i], w = target[i];
  if (u >= N || w >= N) { imp_defect(err, DK_RANGE, i); return; }
  if (u == w) { imp_defect(err, DK_SELF, i); return; }
  atomicAdd((unsigned long long*)&cnt[u], 1ull);
  atomicAdd((unsigned long long*)&cnt[w], 1ull);
}

// Peer v from its count alone: in no dial, or more ends than a valid row has; rows past
// `thread_ends` ends go on the list of the wave-per-row sort (in any order).
__global__ __launch_bounds__(TB) void k_dial_rows(uint32_t N, uint32_t thread_ends, const uint64_t* __restrict__ cnt,
                                                  uint32_t* __restrict__ big, unsigned* __restrict__ nbig,
                                                  unsigned long long* err) {
  const uint32_t v = blockIdx.x * TB + threadIdx.x;
  if (v >= N) return;
  const uint64_t n = cnt[v];
  if (n == 0) imp_defect(err, DK_ALONE, v);
  else if (n > IMP_ENDS) imp_defect(err, DK_ENDS, v);
  else if (n > thread_ends) big[atomicAdd(nbig, 1u)] = v;
}

// A dial end in its peer's row: (other peer << 1 | F_OUT) << 32 | dial index, so a sorted row
// holds each connection's ends side by side, the inbound one first, repeats in dial order.
__global__ __launch_bounds__(TB) void k_dial_scatter(uint64_t n, const uint32_t* __restrict__ dialer,
                                                     const uint32_t* __restrict__ target,
                                                     const uint64_t* __restrict__ off, uint64_t* __restrict__ fill,
                                                     uint64_t* __restrict__ he) {
  const uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (i >= n) return;
  const uint32_t u = dialer[i], w = target[i];
  uint64_t p = atomicAdd((unsigned long long*)&fill[u], 1ull);
  he[off[u] + p] = ((((uint64_t)w << 1) | 1ull) << 32) | i;
  p = atomicAdd((unsigned long long*)&fill[w], 1ull);
  he[off[w] + p] = (((uint64_t)u << 1) << 32) | i;
}

// Rows of at most thread_ends ends, a thread each (k_sort_dedupe's pattern): sort, merge the two
// ends of a mutual dial, report the later dial of a repeated pair. The row is left in
// k_compact's form (peer << 1 | F_OUT), ndeg[v] connections long.
__global__ __launch_bounds__(TB) void k_dial_sort_thread(uint32_t N, uint32_t thread_ends,
                                                         const uint64_t* __restrict__ off, uint64_t* __restrict__ he,
                                                         uint64_t* __restrict__ ndeg, unsigned long long* err) {
  const uint32_t v = blockIdx.x * TB + threadIdx.x;
  if (v >= N) return;
  const uint64_t b = off[v], e = off[v + 1];
  if (e - b > thread_ends) return;
  for (uint64_t i = b + 1; i < e; i++) {
    const uint64_t x = he[i];
    uint64_t j = i;
    while (j > b && he[j - 1] > x) { he[j] = he[j - 1]; j--; }
    he[j] = x;
  }
  uint64_t w = b, prev = ~0ull;  // prev: the last end's peer << 1 | F_OUT
  for (uint64_t i = b; i < e; i++) {
    const uint64_t x = he[i], key = x >> 32;
    if (key == prev) imp_defect(err, DK_REPEAT, x & 0xFFFFFFFFull);
    if ((key >> 1) == (prev >> 1)) he[w - 1] |= key & 1ull;
    else he[w++] = key;
    prev = key;
  }
  ndeg[v] = w - b;
}

// Rows of thread_ends + 1 .. IMP_ENDS ends, a wave each with the row in LDS (4 KB): every lane
// ranks its ends against the whole row (the keys are distinct: the dial index is part of them),
// then the wave merges and compacts 64 sorted ends at a time.
__global__ __launch_bounds__(TB) void k_dial_sort_wave(uint32_t nbig, const uint32_t* __restrict__ big,
                                                       const uint64_t* __restrict__ off, uint64_t* __restrict__ he,
                                                       uint64_t* __restrict__ ndeg, unsigned long long* err) {
  __shared__ uint64_t s_in[TB / 64][IMP_ENDS], s_out[TB / 64][IMP_ENDS];
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = blockIdx.x * (TB / 64) + wv;
  const bool on = r < nbig;
  const uint32_t v = on ? big[r] : 0;
  const uint64_t b = on ? off[v] : 0;
  uint32_t n = on ? (uint32_t)(off[v + 1] - b) : 0;
  if (n > IMP_ENDS) n = IMP_ENDS;  // (k_dial_rows lists no longer row)
  uint64_t* in = s_in[wv];
  uint64_t* out = s_out[wv];
  for (uint32_t i = lane; i < n; i += 64) in[i] = he[b + i];
  __syncthreads();
  for (uint32_t i = lane; i < n; i += 64) {
    const uint64_t x = in[i];
    uint32_t rank = 0;
    for (uint32_t j = 0; j < n; j++) rank += in[j] < x;
    out[rank] = x;
  }
  __syncthreads();
  uint32_t base = 0;
  for (uint32_t i0 = 0; i0 < n; i0 += 64) {
    const uint32_t i = i0 + lane;
    const bool have = i < n;
    const uint64_t key = have ? out[i] >> 32 : 0;
    const uint64_t before = have && i > 0 ? out[i - 1] >> 32 : ~0ull;
    const uint64_t after = have && i + 1 < n ? out[i + 1] >> 32 : ~0ull;
    if (have && key == before) imp_defect(err, DK_REPEAT, out[i] & 0xFFFFFFFFull);
    const bool head = have && (key >> 1) != (before >> 1);
    const uint64_t merged = key | ((after >> 1) == (key >> 1) ? after & 1ull : 0ull);
    const uint64_t bm = __ballot(head);
    if (head) he[b + base + (uint32_t)__popcll(bm & ((1ull << lane) - 1))] = merged;
    base += (uint32_t)__popcll(bm);
  }
  if (on && lane == 0) ndeg[v] = base;
}

}  // namespace

void device_exclusive_scan(Ctx& c, const uint64_t* in, uint64_t* out, uint32_t n) {
  size_t tmp = 0;
  GS_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp, in, out, n, c.stream));
  DevBuf<uint8_t> t;
  t.alloc(tmp ? tmp : 1);
  GS_HIP(hipcub::DeviceScan::ExclusiveSum(t.p, tmp, in, out, n, c.stream));
  GS_HIP(hipStreamSynchronize(c.stream));
}

void launch_topology(Ctx& c) {
  const uint32_t N = c.cfg.peers, k = c.k;
  const uint64_t Nk = (uint64_t)N * k;
  hipStream_t s = c.stream;
  c.d_dial.alloc(Nk);
  c.d_acc.alloc(Nk);
  GS_HIP(hipMemsetAsync(c.d_acc.p, 1, Nk, s));
  k_dials<<<blocks(N), TB, 0, s>>>(N, k, c.cfg.seed, c.d_dial.p);
  GS_HIP(hipGetLastError());

  DevBuf<uint64_t> cnt, off, fill, tmp;
  cnt.alloc((size_t)N + 1);
  off.alloc((size_t)N + 1);
  fill.alloc(N);
  if (c.cfg.max_connections) {
    const uint32_t quota = c.cfg.max_connections > k ? c.cfg.max_connections - k : 0;
    GS_HIP(hipMemsetAsync(cnt.p, 0, ((size_t)N + 1) * 8, s));
    GS_HIP(hipMemsetAsync(fill.p, 0, (size_t)N * 8, s));
    k_inbound_count<<<blocks(Nk), TB, 0, s>>>(Nk, k, c.d_dial.p, cnt.p);
    device_exclusive_scan(c, cnt.p, off.p, N + 1);
    tmp.alloc(Nk);
    k_inbound_scatter<<<blocks(Nk), TB, 0, s>>>(N, k, c.d_dial.p, off.p, fill.p, tmp.p);
    k_inbound_accept<<<blocks(N), TB, 0, s>>>(N, k, quota, c.d_dial.p, off.p, tmp.p, c.d_acc.p);
    GS_HIP(hipGetLastError());
  }
  // half-edge buckets
  GS_HIP(hipMemsetAsync(cnt.p, 0, ((size_t)N + 1) * 8, s));
  GS_HIP(hipMemsetAsync(fill.p, 0, (size_t)N * 8, s));
  k_deg<<<blocks(Nk), TB, 0, s>>>(N, k, c.d_dial.p, c.d_acc.p, cnt.p);
  device_exclusive_scan(c, cnt.p, off.p, N + 1);
  uint64_t he_n = 0;
  GS_HIP(hipMemcpy(&he_n, off.p + N, 8, hipMemcpyDeviceToHost));
  DevBuf<uint64_t> he, ndeg;
  he.alloc(he_n ? he_n : 1);
  ndeg.alloc((size_t)N + 1);
  k_half_edges<<<blocks(Nk), TB, 0, s>>>(N, k, c.d_dial.p, c.d_acc.p, off.p, fill.p, he.p);
  GS_HIP(hipMemsetAsync(ndeg.p, 0, ((size_t)N + 1) * 8, s));
  k_sort_dedupe<<<blocks(N), TB, 0, s>>>(N, off.p, he.p, ndeg.p);
  c.d_row.alloc((size_t)N + 1);
  device_exclusive_scan(c, ndeg.p, c.d_row.p, N + 1);
  GS_HIP(hipMemcpy(&c.nnz, c.d_row.p + N, 8, hipMemcpyDeviceToHost));
  if (c.nnz >= (1ull << 32)) c.fail(GS_EUNSUPPORTED, "graph has >= 2^32 entries");
  c.d_col.alloc(c.nnz ? c.nnz : 1);
  c.d_flags.alloc(c.nnz ? c.nnz : 1);
  c.d_rev.alloc(c.nnz ? c.nnz : 1);
  DevBuf<unsigned> md;
  md.alloc(1);
  GS_HIP(hipMemsetAsync(md.p, 0, 4, s));
  k_compact<<<blocks(N), TB, 0, s>>>(N, off.p, he.p, c.d_row.p, c.d_col.p, c.d_flags.p, md.p);
  k_reverse<<<blocks(N), TB, 0, s>>>(N, c.d_row.p, c.d_col.p, c.d_rev.p);
  GS_HIP(hipGetLastError());
  unsigned maxdeg = 0;
  GS_HIP(hipMemcpyAsync(&maxdeg, md.p, 4, hipMemcpyDeviceToHost, s));
  GS_HIP(hipStreamSynchronize(s));
  c.max_degree = maxdeg;
}

// Another graph than the one before stands in the context: what gs_build_topology invalidates,
// and what else hangs on the old CSR — the per-entry arrays (a saved state writes nnz
// back-offs), the churn ring (sized once per context, with the mask ring only for rows of at
// most 64 entries) and the chain's state, the mesh events of the last converge.
void graph_replaced(Ctx& c) {
  c.csrpos_valid = false;
  c.cell_valid = false;
  c.mesh_built = false;
  c.glp_prefer = false;
  c.glp_quiet = 0;
  c.rpos_valid = false;
  c.mesh_dmax = 0;
  c.d_until.release();
  c.d_prop.release();
  c.d_iprop.release();
  c.d_csrpos.release();
  c.ring_R = 0;  // ensure_ring sizes the ring again for this graph's rows
  c.d_ring_mm.release();
  c.ring_in_tag.clear();
  c.ring_ell_tag.clear();
  c.churn_state = 0;
  c.ring_lo = 1;
  c.ring_hi = 0;
  c.meshev_valid = false;
  c.ld_ready = false;  // the edge slots mean other links
}

// ---- import: everything is built in buffers of the call's own and swapped
// into the context at the end, so a refused graph leaves the context as it was ----
namespace {

struct Staged {
  DevBuf<uint64_t> row;
  DevBuf<uint32_t> col, rev;
  DevBuf<uint8_t> flags;
  uint64_t nnz = 0;
  uint32_t max_degree = 0;
};

template <class T>
void swap_buf(DevBuf<T>& a, DevBuf<T>& b) {
  std::swap(a.p, b.p);
  std::swap(a.n, b.n);
}

// The staged graph becomes the context's (graph_replaced: what hangs on the old one goes).
void adopt(Ctx& c, Staged& g) {
  hipStream_t s = c.stream;
  DevBuf<unsigned long long> fp;
  fp.alloc(1);
  GS_HIP(hipMemsetAsync(fp.p, 0, 8, s));
  k_import_fingerprint<<<std::min(FP_BLOCKS, blocks(std::max<uint64_t>(g.nnz, (uint64_t)c.cfg.peers + 1))), TB, 0, s>>>(
      c.cfg.peers, g.nnz, g.row.p, g.col.p, g.flags.p, fp.p);
  GS_HIP(hipGetLastError());
  unsigned long long h = 0;
  GS_HIP(hipMemcpyAsync(&h, fp.p, 8, hipMemcpyDeviceToHost, s));
  for (hipStream_t st : {c.side, c.chain_pipe, c.pass_ms, c.copy, s})  // nothing still reads the old graph
    if (st) GS_HIP(hipStreamSynchronize(st));
  swap_buf(c.d_row, g.row);
  swap_buf(c.d_col, g.col);
  swap_buf(c.d_flags, g.flags);
  swap_buf(c.d_rev, g.rev);
  c.nnz = g.nnz;
  c.max_degree = g.max_degree;
  c.topo_fp = h ? h : 1;  // 0 is the built graph
  c.topo_built = true;
  graph_replaced(c);
}

std::string at(const char* what, const char* unit, uint64_t idx) {
  return std::string(what) + " at " + unit + " " + std::to_string(idx);
}

}  // namespace

void import_csr(Ctx& c, const uint64_t* row_ptr, const uint32_t* col, const uint8_t* flags) {
  const uint32_t N = c.cfg.peers;
  hipStream_t s = c.stream;
  // row_ptr on the host: its last word sizes the copies of col and flags
  if (row_ptr[0] != 0) c.fail(GS_EINVAL, "CSR: row_ptr[0] is not 0");
  for (uint32_t v = 0; v < N; v++)
    if (row_ptr[v + 1] < row_ptr[v]) c.fail(GS_EINVAL, at("CSR: row_ptr not monotone", "peer", v));
  Staged g;
  g.nnz = row_ptr[N];
  if (g.nnz >= (1ull << 32)) c.fail(GS_EUNSUPPORTED, "graph has >= 2^32 entries");
  if (g.nnz && (!col || !flags)) c.fail(GS_EINVAL, "null col or flags");
  const size_t nz = g.nnz ? g.nnz : 1;
  DevBuf<uint8_t> fin;
  DevBuf<unsigned long long> err;
  DevBuf<unsigned> md;
  g.row.alloc((size_t)N + 1);
  g.col.alloc(nz);
  g.flags.alloc(nz);
  g.rev.alloc(nz);
  fin.alloc(nz);
  err.alloc(1);
  md.alloc(1);
  GS_HIP(hipMemcpyAsync(g.row.p, row_ptr, ((size_t)N + 1) * 8, hipMemcpyHostToDevice, s));
  if (g.nnz) {
    GS_HIP(hipMemcpyAsync(g.col.p, col, g.nnz * 4, hipMemcpyHostToDevice, s));
    GS_HIP(hipMemcpyAsync(fin.p, flags, g.nnz, hipMemcpyHostToDevice, s));
  }
  GS_HIP(hipMemsetAsync(err.p, 0xFF, 8, s));
  GS_HIP(hipMemsetAsync(md.p, 0, 4, s));
  k_import_csr<<<blocks(std::max<uint64_t>(g.nnz, N)), TB, 0, s>>>(N, g.nnz, g.row.p, g.col.p, fin.p, g.flags.p,
                                                                 g.rev.p, err.p, md.p);
  GS_HIP(hipGetLastError());
  unsigned long long e = 0;
  unsigned maxdeg = 0;
  GS_HIP(hipMemcpyAsync(&e, err.p, 8, hipMemcpyDeviceToHost, s));
  GS_HIP(hipMemcpyAsync(&maxdeg, md.p, 4, hipMemcpyDeviceToHost, s));
  GS_HIP(hipStreamSynchronize(s));
  if (e != IMP_NONE) {
    const uint64_t idx = e & ((1ull << IMP_KIND_SHIFT) - 1);
    switch (e >> IMP_KIND_SHIFT) {
      case CK_RANGE: c.fail(GS_EINVAL, at("CSR: id >= peers", "entry", idx));
      case CK_SELF: c.fail(GS_EINVAL, at("CSR: self-loop", "entry", idx));
      case CK_ORDER: c.fail(GS_EINVAL, at("CSR: row not strictly ascending", "entry", idx));
      case CK_NOREV: c.fail(GS_EINVAL, at("CSR: entry without its reverse", "entry", idx));
      case CK_NODIALER: c.fail(GS_EINVAL, at("CSR: connection without a dialer (F_OUT on neither end)", "entry", idx));
      default: c.fail(GS_EINVAL, at("CSR: Failed to connect any peers (no connection)", "peer", idx));
    }
  }
  if (maxdeg > MAX_DEG) c.fail(GS_EUNSUPPORTED, "peer degree exceeds 256");
  g.max_degree = maxdeg;
  adopt(c, g);
}

void import_dials(Ctx& c, uint64_t n, const uint32_t* dialer, const uint32_t* target) {
  const uint32_t N = c.cfg.peers;
  hipStream_t s = c.stream;
  if (n == 0) c.fail(GS_EINVAL, at("dial list: Failed to connect any peers (in no dial)", "peer", 0));
  if (n >= (1ull << 32)) c.fail(GS_EUNSUPPORTED, "graph has >= 2^32 entries");  // (a valid list gives >= n entries)
  // GS_IMPORT_WAVE_ROWS=0: every row sorts a thread per row (the measurement of DESIGN.md §4.9)
  const uint32_t thread_ends = env_off("GS_IMPORT_WAVE_ROWS") ? IMP_ENDS : IMP_THREAD_ENDS;
  DevBuf<uint32_t> dd, dt, big;
  DevBuf<uint64_t> cnt, off, fill, he, ndeg;
  DevBuf<unsigned long long> err;
  DevBuf<unsigned> word;  // [0] rows on the wave list, [1] widest row
  dd.alloc(n);
  dt.alloc(n);
  big.alloc(N);
  cnt.alloc((size_t)N + 1);
  off.alloc((size_t)N + 1);
  fill.alloc(N);
  ndeg.alloc((size_t)N + 1);
  err.alloc(1);
  word.alloc(2);
  GS_HIP(hipMemcpyAsync(dd.p, dialer, n * 4, hipMemcpyHostToDevice, s));
  GS_HIP(hipMemcpyAsync(dt.p, target, n * 4, hipMemcpyHostToDevice, s));
  GS_HIP(hipMemsetAsync(cnt.p, 0, ((size_t)N + 1) * 8, s));
  GS_HIP(hipMemsetAsync(fill.p, 0, (size_t)N * 8, s));
  GS_HIP(hipMemsetAsync(ndeg.p, 0, ((size_t)N + 1) * 8, s));
  GS_HIP(hipMemsetAsync(err.p, 0xFF, 8, s));
  GS_HIP(hipMemsetAsync(word.p, 0, 8, s));
  k_dial_count<<<blocks(n), TB, 0, s>>>(N, n, dd.p, dt.p, cnt.p, err.p);
  k_dial_rows<<<blocks(N), TB, 0, s>>>(N, thread_ends, cnt.p, big.p, word.p, err.p);
  GS_HIP(hipGetLastError());
  unsigned long long e = 0;
  unsigned nbig = 0;
  auto refuse = [&]() {
    if (e == IMP_NONE) return;
    const uint64_t idx = e & ((1ull << IMP_KIND_SHIFT) - 1);
    switch (e >> IMP_KIND_SHIFT) {
      case DK_RANGE: c.fail(GS_EINVAL, at("dial list: id >= peers", "dial", idx));
      case DK_SELF: c.fail(GS_EINVAL, at("dial list: dialer == target", "dial", idx));
      case DK_ALONE: c.fail(GS_EINVAL, at("dial list: Failed to connect any peers (in no dial)", "peer", idx));
      case DK_ENDS: c.fail(GS_EUNSUPPORTED, at("dial list: more than 512 dial ends", "peer", idx));
      default: c.fail(GS_EINVAL, at("dial list: the same ordered pair twice", "dial", idx));
    }
  };
  GS_HIP(hipMemcpyAsync(&e, err.p, 8, hipMemcpyDeviceToHost, s));
  GS_HIP(hipMemcpyAsync(&nbig, word.p, 4, hipMemcpyDeviceToHost, s));
  GS_HIP(hipStreamSynchronize(s));
  refuse();
  device_exclusive_scan(c, cnt.p, off.p, N + 1);  // (every id is in range from here on, every row <= IMP_ENDS)
  he.alloc(2 * n);
  k_dial_scatter<<<blocks(n), TB, 0, s>>>(n, dd.p, dt.p, off.p, fill.p, he.p);
  k_dial_sort_thread<<<blocks(N), TB, 0, s>>>(N, thread_ends, off.p, he.p, ndeg.p, err.p);
  if (nbig) k_dial_sort_wave<<<(nbig + TB / 64 - 1) / (TB / 64), TB, 0, s>>>(nbig, big.p, off.p, he.p, ndeg.p, err.p);
  GS_HIP(hipGetLastError());
  Staged g;
  g.row.alloc((size_t)N + 1);
  device_exclusive_scan(c, ndeg.p, g.row.p, N + 1);
  GS_HIP(hipMemcpyAsync(&e, err.p, 8, hipMemcpyDeviceToHost, s));
  GS_HIP(hipMemcpyAsync(&g.nnz, g.row.p + N, 8, hipMemcpyDeviceToHost, s));
  GS_HIP(hipStreamSynchronize(s));
  refuse();
  if (g.nnz >= (1ull << 32)) c.fail(GS_EUNSUPPORTED, "graph has >= 2^32 entries");
  g.col.alloc(g.nnz);
  g.flags.alloc(g.nnz);
  g.rev.alloc(g.nnz);
  k_compact<<<blocks(N), TB, 0, s>>>(N, off.p, he.p, g.row.p, g.col.p, g.flags.p, word.p + 1);
  k_reverse<<<blocks(N), TB, 0, s>>>(N, g.row.p, g.col.p, g.rev.p);
  GS_HIP(hipGetLastError());
  GS_HIP(hipMemcpyAsync(&g.max_degree, word.p + 1, 4, hipMemcpyDeviceToHost, s));
  GS_HIP(hipStreamSynchronize(s));
  if (g.max_degree > MAX_DEG) c.fail(GS_EUNSUPPORTED, "peer degree exceeds 256");
  adopt(c, g);
}

}  // namespace gs
