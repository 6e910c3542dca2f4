// gs_outages.h — a caller's outages in place of the churn draw (gs_set_outages,
// gs_clear_outages, gs_get_offline; DESIGN.md §2.8 "A caller's outages"). Included by
// gs_mesh.hip right after k_offline_range, at namespace gs scope: k_outage_range is that
// kernel's twin, and the two launch sites of the epoch chain pick one of them.
//
// A schedule is a set of intervals (peer, h_from, h_to): the peer is offline during the
// heartbeat epochs h_from <= h < h_to, h_to == GS_OUTAGE_FOREVER meaning every epoch from
// h_from on. The offline bitsets are all the epoch chain, the ring, the list pass, the push
// kernels and the counting passes read of churn, so the import swaps one predicate.
//
// The build is the dial import's (gs_topology.hip): a thread per interval validates and
// counts it into its peer's row, a scan gives the row pointers, a scatter places the
// intervals, a thread per peer sorts its row by h_from (insertion sort, rows of at most
// GS_OUTAGE_ROW_MAX intervals), finds the intervals that share an epoch with another one and
// merges the touching ones; a second scan and a copy leave the rows as a CSR of (h_from,
// h_to) pairs. Everything is built in buffers of the call's own and swapped into the
// context only when the schedule is accepted. Defects are one word reduced with atomicMin
// (gs_import.h), so the reported kind and index depend on no order of threads.
#pragma once

namespace {

enum : uint64_t {  // defects in reporting order (index: interval; OG_ROW: peer)
  OG_RANGE = 1, OG_ZERO = 2, OG_EMPTY = 3, OG_ROW = 4, OG_OVERLAP = 5
};
constexpr uint32_t OG_FOREVER = 0xFFFFFFFFu;  // GS_OUTAGE_FOREVER

inline unsigned og_blocks(uint64_t n) { return (unsigned)((n + TB - 1) / TB); }

// Is u offline in epoch h >= 1: the last interval of its sorted, disjoint row that starts
// at or before h covers h. Most rows are empty: the two row pointers decide them.
__device__ __forceinline__ bool og_offline(const uint32_t* __restrict__ ptr, const uint2* __restrict__ iv, uint32_t u,
                                           uint64_t h) {
  const uint32_t b = ptr[u], e = ptr[u + 1];
  if (b == e) return false;
  uint32_t lo = b, hi = e;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (iv[mid].x <= h) lo = mid + 1; else hi = mid;
  }
  if (lo == b) return false;
  const uint32_t to = iv[lo - 1].y;
  return to == OG_FOREVER || h < to;
}

// k_offline_range's twin: the offline bitsets of epochs h0 + y, y < gridDim.y, into lin[y]
// (w64 words each) and, for epochs >= ring_h0 and a ring, into ring slot h % R. One ballot
// per wave is the bitset word; lanes at and past N and epoch 0 give 0.
__global__ __launch_bounds__(TB) void k_outage_range(uint32_t N, const uint32_t* __restrict__ ptr,
                                                     const uint2* __restrict__ iv, uint64_t h0, uint64_t* lin,
                                                     uint32_t w64, uint64_t* ring, uint32_t R, uint64_t ring_h0) {
  const uint32_t u = blockIdx.x * TB + threadIdx.x;
  const uint64_t h = h0 + blockIdx.y;
  const uint64_t m = __ballot(u < N && h != 0 && og_offline(ptr, iv, u, h));
  if ((threadIdx.x & 63) == 0 && u < N) {
    lin[(size_t)blockIdx.y * w64 + (u >> 6)] = m;
    if (ring && h >= ring_h0) ring[(size_t)(h % R) * w64 + (u >> 6)] = m;
  }
}

// Interval i: its own defects, then one count in its peer's row.
__global__ __launch_bounds__(TB) void k_og_count(uint32_t N, uint64_t n, const uint32_t* __restrict__ peer,
                                                 const uint32_t* __restrict__ from, const uint32_t* __restrict__ to,
                                                 uint64_t* __restrict__ cnt, unsigned long long* err) {
  const uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (i >= n) return;
  const uint32_t u = peer[i];
  if (u >= N) { imp_defect(err, OG_RANGE, i); return; }
  if (from[i] == 0) { imp_defect(err, OG_ZERO, i); return; }
  if (from[i] >= to[i]) { imp_defect(err, OG_EMPTY, i); return; }
  atomicAdd((unsigned long long*)&cnt[u], 1ull);
}

// Peer v from its count alone: more intervals than a thread sorts.
__global__ __launch_bounds__(TB) void k_og_rows(uint32_t N, const uint64_t* __restrict__ cnt,
                                                unsigned long long* err) {
  const uint32_t v = blockIdx.x * TB + threadIdx.x;
  if (v < N && cnt[v] > GS_OUTAGE_ROW_MAX) imp_defect(err, OG_ROW, v);
}

// Interval i into its peer's row: key = h_from << 32 | h_to, and its index beside it.
__global__ __launch_bounds__(TB) void k_og_scatter(uint64_t n, const uint32_t* __restrict__ peer,
                                                   const uint32_t* __restrict__ from, const uint32_t* __restrict__ to,
                                                   const uint64_t* __restrict__ off, uint64_t* __restrict__ fill,
                                                   uint64_t* __restrict__ key, uint32_t* __restrict__ idx) {
  const uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (i >= n) return;
  const uint32_t u = peer[i];
  const uint64_t p = off[u] + atomicAdd((unsigned long long*)&fill[u], 1ull);
  key[p] = ((uint64_t)from[i] << 32) | to[i];
  idx[p] = (uint32_t)i;
}

// Row v, a thread each: sort by (h_from, h_to), then one walk with the largest h_to so far.
// An interval that starts before that end shares an epoch with the interval that holds it:
// both are reported, which reports every interval that overlaps any other (an interval no
// earlier one overlaps holds the largest end until a later one that overlaps it takes over).
// Touching neighbours merge; the row is left ndeg[v] intervals long.
__global__ __launch_bounds__(TB) void k_og_sort(uint32_t N, const uint64_t* __restrict__ off,
                                                uint64_t* __restrict__ key, uint32_t* __restrict__ idx,
                                                uint64_t* __restrict__ ndeg, unsigned long long* err) {
  const uint32_t v = blockIdx.x * TB + threadIdx.x;
  if (v >= N) return;
  const uint64_t b = off[v], e = off[v + 1];
  for (uint64_t i = b + 1; i < e; i++) {
    const uint64_t x = key[i];
    const uint32_t xi = idx[i];
    uint64_t j = i;
    while (j > b && key[j - 1] > x) { key[j] = key[j - 1]; idx[j] = idx[j - 1]; j--; }
    key[j] = x;
    idx[j] = xi;
  }
  uint64_t w = b;
  uint32_t end = 0, end_idx = 0;  // the largest h_to so far (every h_from is >= 1) and the interval that holds it
  for (uint64_t i = b; i < e; i++) {
    const uint64_t x = key[i];
    const uint32_t f = (uint32_t)(x >> 32), t = (uint32_t)x;
    if (f < end) {
      imp_defect(err, OG_OVERLAP, idx[i]);
      imp_defect(err, OG_OVERLAP, end_idx);
    }
    if (w > b && f == end) key[w - 1] = (key[w - 1] & 0xFFFFFFFF00000000ull) | t;  // touching: their union
    else key[w++] = x;
    if (t > end) { end = t; end_idx = idx[i]; }
  }
  ndeg[v] = w - b;
}

// The merged rows as the CSR the lookups read, and the schedule's fingerprint: a sum of mixed
// words over (peer, interval), so neither the list's order nor the threads' decides it.
__global__ __launch_bounds__(TB) void k_og_compact(uint32_t N, const uint64_t* __restrict__ off,
                                                   const uint64_t* __restrict__ key, const uint64_t* __restrict__ row,
                                                   uint32_t* __restrict__ ptr, uint2* __restrict__ iv,
                                                   unsigned long long* fp) {
  const uint32_t v = blockIdx.x * TB + threadIdx.x;
  uint64_t x = 0;
  if (v <= N) ptr[v] = (uint32_t)row[v];
  if (v < N) {
    const uint64_t b = off[v], r = row[v], n = row[v + 1] - r;
    for (uint64_t i = 0; i < n; i++) {
      const uint64_t k = key[b + i];
      iv[r + i] = make_uint2((uint32_t)(k >> 32), (uint32_t)k);
      x += imp_mix((((uint64_t)v << 1) | 1ull) ^ imp_mix(k));
    }
  }
  for (int d = 32; d; d >>= 1) x += (uint64_t)__shfl_xor((unsigned long long)x, d, 64);
  if ((threadIdx.x & 63) == 0 && x) atomicAdd(fp, (unsigned long long)x);
}

template <class T>
void og_swap(DevBuf<T>& a, DevBuf<T>& b) {
  std::swap(a.p, b.p);
  std::swap(a.n, b.n);
}

// The offline source changed: what a converge leaves is of the old one, and so are the chain's
// state, the ring and the mesh events (graph_replaced's part for the epochs).
void og_invalidate(Ctx& c) {
  c.mesh_built = false;
  c.glp_prefer = false;
  c.glp_quiet = 0;
  c.rpos_valid = false;
  c.mesh_dmax = 0;
  c.ring_in_tag.assign(c.ring_in_tag.size(), ~0ull);
  c.ring_ell_tag.assign(c.ring_ell_tag.size(), ~0ull);
  c.churn_state = 0;
  c.ring_lo = 1;
  c.ring_hi = 0;
  c.meshev_valid = false;
}

void og_quiesce(Ctx& c) {  // nothing still reads the old rows
  for (hipStream_t st : {c.side, c.chain_pipe, c.pass_ms, c.copy, c.stream})
    if (st) GS_HIP(hipStreamSynchronize(st));
}

std::string og_at(const char* what, const char* unit, uint64_t idx) {
  return std::string(what) + " at " + unit + " " + std::to_string(idx);
}

}  // namespace

// The offline bitsets of epochs [h_first, h_first + E) from the context's source, on stream s:
// the draw (k_offline_range) or the imported rows (k_outage_range), the same outputs.
void offline_range(Ctx& c, hipStream_t s, uint64_t h_first, uint64_t E, uint64_t* lin, uint32_t w64, uint64_t* ring,
                   uint64_t ring_h0) {
  const uint32_t N = c.cfg.peers;
  for (uint64_t y0 = 0; y0 < E; y0 += 32768) {  // grid.y limit
    const uint32_t ny = (uint32_t)std::min<uint64_t>(32768, E - y0);
    const dim3 grid(og_blocks(N), ny);
    if (c.outages_on)
      k_outage_range<<<grid, TB, 0, s>>>(N, c.d_og_ptr.p, (const uint2*)c.d_og_iv.p, h_first + y0, lin + y0 * w64, w64,
                                         ring, c.ring_R, ring_h0);
    else
      k_offline_range<<<grid, TB, 0, s>>>(N, c.cfg.seed, c.cfg.churn_ppm, c.cfg.churn_down, h_first + y0,
                                          lin + y0 * w64, w64, ring, c.ring_R, ring_h0);
  }
}

void import_outages(Ctx& c, uint64_t n, const uint32_t* peer, const uint32_t* h_from, const uint32_t* h_to) {
  const uint32_t N = c.cfg.peers;
  hipStream_t s = c.stream;
  if (n >= (1ull << 32)) c.fail(GS_EUNSUPPORTED, "outages: 2^32 or more intervals");
  DevBuf<uint32_t> dp, df, dt, idx, ptr;
  DevBuf<uint64_t> cnt, off, fill, key, ndeg, row, iv;
  DevBuf<unsigned long long> word;  // [0] the defect, [1] the fingerprint
  const size_t nz = n ? n : 1;
  cnt.alloc((size_t)N + 1);
  off.alloc((size_t)N + 1);
  fill.alloc(N);
  ndeg.alloc((size_t)N + 1);
  row.alloc((size_t)N + 1);
  ptr.alloc((size_t)N + 1);
  key.alloc(nz);
  idx.alloc(nz);
  iv.alloc(nz);
  word.alloc(2);
  GS_HIP(hipMemsetAsync(cnt.p, 0, ((size_t)N + 1) * 8, s));
  GS_HIP(hipMemsetAsync(fill.p, 0, (size_t)N * 8, s));
  GS_HIP(hipMemsetAsync(ndeg.p, 0, ((size_t)N + 1) * 8, s));
  GS_HIP(hipMemsetAsync(word.p, 0xFF, 8, s));
  GS_HIP(hipMemsetAsync(word.p + 1, 0, 8, s));
  unsigned long long e = 0, fp = 0;
  auto refuse = [&]() {
    if (e == IMP_NONE) return;
    const uint64_t i = e & ((1ull << IMP_KIND_SHIFT) - 1);
    switch (e >> IMP_KIND_SHIFT) {
      case OG_RANGE: c.fail(GS_EINVAL, og_at("outages: peer >= peers", "interval", i));
      case OG_ZERO: c.fail(GS_EINVAL, og_at("outages: h_from == 0 (epoch 0 has nobody offline)", "interval", i));
      case OG_EMPTY: c.fail(GS_EINVAL, og_at("outages: h_from >= h_to", "interval", i));
      case OG_ROW: c.fail(GS_EUNSUPPORTED, og_at("outages: more than 256 intervals", "peer", i));
      default: c.fail(GS_EINVAL, og_at("outages: two intervals of one peer share an epoch", "interval", i));
    }
  };
  if (n) {
    dp.alloc(n);
    df.alloc(n);
    dt.alloc(n);
    GS_HIP(hipMemcpyAsync(dp.p, peer, n * 4, hipMemcpyHostToDevice, s));
    GS_HIP(hipMemcpyAsync(df.p, h_from, n * 4, hipMemcpyHostToDevice, s));
    GS_HIP(hipMemcpyAsync(dt.p, h_to, n * 4, hipMemcpyHostToDevice, s));
    k_og_count<<<og_blocks(n), TB, 0, s>>>(N, n, dp.p, df.p, dt.p, cnt.p, word.p);
    k_og_rows<<<og_blocks(N), TB, 0, s>>>(N, cnt.p, word.p);
    GS_HIP(hipGetLastError());
    GS_HIP(hipMemcpyAsync(&e, word.p, 8, hipMemcpyDeviceToHost, s));
    GS_HIP(hipStreamSynchronize(s));
    refuse();
  }
  device_exclusive_scan(c, cnt.p, off.p, N + 1);  // (every peer is in range from here on, every row <= GS_OUTAGE_ROW_MAX)
  if (n) {
    k_og_scatter<<<og_blocks(n), TB, 0, s>>>(n, dp.p, df.p, dt.p, off.p, fill.p, key.p, idx.p);
    k_og_sort<<<og_blocks(N), TB, 0, s>>>(N, off.p, key.p, idx.p, ndeg.p, word.p);
    GS_HIP(hipGetLastError());
  }
  device_exclusive_scan(c, ndeg.p, row.p, N + 1);
  k_og_compact<<<og_blocks((uint64_t)N + 1), TB, 0, s>>>(N, off.p, key.p, row.p, ptr.p, (uint2*)iv.p, word.p + 1);
  GS_HIP(hipGetLastError());
  std::vector<uint32_t> hptr((size_t)N + 1);
  GS_HIP(hipMemcpyAsync(&e, word.p, 8, hipMemcpyDeviceToHost, s));
  GS_HIP(hipMemcpyAsync(&fp, word.p + 1, 8, hipMemcpyDeviceToHost, s));
  GS_HIP(hipMemcpyAsync(hptr.data(), ptr.p, ((size_t)N + 1) * 4, hipMemcpyDeviceToHost, s));
  GS_HIP(hipStreamSynchronize(s));
  refuse();
  std::vector<uint64_t> hiv(hptr[N]);  // the host's copy, for the publisher-online checks (Ctx::offline)
  if (hptr[N]) GS_HIP(hipMemcpyAsync(hiv.data(), iv.p, (size_t)hptr[N] * 8, hipMemcpyDeviceToHost, s));
  og_quiesce(c);
  og_swap(c.d_og_ptr, ptr);
  og_swap(c.d_og_iv, iv);
  c.og_ptr.swap(hptr);
  c.og_iv.swap(hiv);
  c.outages_on = true;
  c.outage_fp = fp ? fp : 1;  // 0 is the draw
  og_invalidate(c);
}

void clear_outages(Ctx& c) {
  if (!c.outages_on) return;
  og_quiesce(c);
  c.outages_on = false;
  c.outage_fp = 0;
  c.d_og_ptr.release();
  c.d_og_iv.release();
  c.og_ptr = std::vector<uint32_t>();
  c.og_iv = std::vector<uint64_t>();
  og_invalidate(c);
}

// gs_get_offline: the bitsets of epochs [h_lo, h_hi], [(h_hi - h_lo + 1)][(peers + 63) / 64].
void get_offline(Ctx& c, uint64_t h_lo, uint64_t h_hi, uint64_t* bits) {
  const uint32_t w64 = (c.cfg.peers + 63) / 64;
  const uint64_t E = h_hi - h_lo + 1;
  DevBuf<uint64_t> d;
  d.alloc((size_t)E * w64);
  offline_range(c, c.stream, h_lo, E, d.p, w64, nullptr, 0);
  GS_HIP(hipGetLastError());
  GS_HIP(hipMemcpyAsync(bits, d.p, (size_t)E * w64 * 8, hipMemcpyDeviceToHost, c.stream));
  GS_HIP(hipStreamSynchronize(c.stream));
}
