// gs_meshimport.h — a caller's mesh in place of the converged one (gs_set_mesh: ELL rows in
// gs_get_mesh's layout; gs_set_mesh_links: a list of undirected links; DESIGN.md §2.3 "A
// caller's mesh"). Included by gs_mesh.hip at its end, inside namespace gs: it reuses
// MeshArgs and k_extract, so the imported arrays are what a converge would leave.
//
// Every frozen-mesh run is a function of (CSR, links, mesh) alone, so nothing below the ABI
// changes but the mesh's three arrays: F_MESH in the CSR flags (lazy gossip picks its targets
// among the connections without it), the packed ELL and the counts. They are built in
// buffers of the call's own and swapped in only when the mesh is accepted.
//
// One thread per ELL slot / per link finds its connection in the CSR row (rows ascend: a
// binary search of at most 8 steps) and sets a byte mark on the entry; one thread per entry
// then checks the reverse mark and writes the staged flags, one per peer counts its row.
// The marks make the mesh a function of the set of links: no order of slots, links or
// threads shows in the result. Defects are one word reduced with atomicMin (gs_import.h,
// which gs_mesh.hip includes at its top).
#pragma once

namespace {

enum : uint64_t {  // ELL defects, in reporting order (index: slot u * MESH_W + j; MK_COUNT: peer; MK_ASYM: CSR entry)
  MK_COUNT = 1, MK_RANGE = 2, MK_SELF = 3, MK_NOCONN = 4, MK_REPEAT = 5, MK_ASYM = 6
};
enum : uint64_t {  // link-list defects, in reporting order (index: link)
  LK_RANGE = 1, LK_SELF = 2, LK_NOCONN = 3, LK_REPEAT = 4
};

// Entry of w in u's CSR row, or EMPTY (u < N; fewer than 2^32 entries).
__device__ __forceinline__ uint32_t mi_find(const uint64_t* __restrict__ row, const uint32_t* __restrict__ col,
                                            uint32_t u, uint32_t w) {
  uint64_t lo = row[u], hi = row[u + 1];
  const uint64_t end = hi;
  while (lo < hi) {
    const uint64_t mid = (lo + hi) >> 1;
    if (col[mid] < w) lo = mid + 1; else hi = mid;
  }
  return lo < end && col[lo] == w ? (uint32_t)lo : EMPTY;
}

// Slot t = u * MESH_W + j of the caller's rows. With counts the row is its first count[u]
// slots, without it ends at its first EMPTY; the slots behind are not read as ids.
__global__ __launch_bounds__(TB) void k_mesh_mark_ell(uint32_t N, const uint64_t* __restrict__ row,
                                                      const uint32_t* __restrict__ col,
                                                      const uint32_t* __restrict__ mesh,
                                                      const uint8_t* __restrict__ count, uint8_t* __restrict__ mark,
                                                      unsigned long long* err) {
  const uint64_t t = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (t >= (uint64_t)N * MESH_W) return;
  const uint32_t u = (uint32_t)(t / MESH_W), j = (uint32_t)(t % MESH_W);
  const uint32_t* r = mesh + (size_t)u * MESH_W;
  if (count) {
    const uint32_t n = count[u];
    if (n > MESH_W) {
      if (j == 0) imp_defect(err, MK_COUNT, u);
      return;
    }
    if (j >= n) return;
  }
  const uint32_t w = r[j];
  bool twice = false;
  for (uint32_t i = 0; i < j; i++) {
    const uint32_t x = r[i];
    if (!count && x == EMPTY) return;  // the row ended before this slot
    twice |= x == w;
  }
  if (!count && w == EMPTY) return;
  if (w >= N) { imp_defect(err, MK_RANGE, t); return; }
  if (w == u) { imp_defect(err, MK_SELF, t); return; }
  const uint32_t e = mi_find(row, col, u, w);
  if (e == EMPTY) { imp_defect(err, MK_NOCONN, t); return; }
  if (twice) { imp_defect(err, MK_REPEAT, t); return; }
  mark[e] = 1;
}

// Link i: its connection's entry at the smaller end (one name per unordered pair) and the
// smallest link index that names it.
__global__ __launch_bounds__(TB) void k_mesh_first_links(uint32_t N, uint64_t n, const uint64_t* __restrict__ row,
                                                         const uint32_t* __restrict__ col,
                                                         const uint32_t* __restrict__ rev,
                                                         const uint32_t* __restrict__ la,
                                                         const uint32_t* __restrict__ lb, uint32_t* __restrict__ ent,
                                                         unsigned* first, unsigned long long* err) {
  const uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (i >= n) return;
  const uint32_t u = la[i], w = lb[i];
  ent[i] = EMPTY;
  if (u >= N || w >= N) { imp_defect(err, LK_RANGE, i); return; }
  if (u == w) { imp_defect(err, LK_SELF, i); return; }
  uint32_t e = mi_find(row, col, u, w);
  if (e == EMPTY) { imp_defect(err, LK_NOCONN, i); return; }
  if (u > w) e = rev[e];
  ent[i] = e;
  atomicMin(&first[e], (unsigned)i);
}

// Link i marks both ends of its connection, or is the repeat of an earlier link.
__global__ __launch_bounds__(TB) void k_mesh_mark_links(uint64_t n, const uint32_t* __restrict__ rev,
                                                        const uint32_t* __restrict__ ent,
                                                        const unsigned* __restrict__ first,
                                                        uint8_t* __restrict__ mark, unsigned long long* err) {
  const uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (i >= n) return;
  const uint32_t e = ent[i];
  if (e == EMPTY) return;
  if (first[e] != (unsigned)i) { imp_defect(err, LK_REPEAT, i); return; }
  mark[e] = 1;
  mark[rev[e]] = 1;
}

// Thread t takes entry t (t < nnz): a mark without its reverse, the staged flags; and peer t
// (t < N): the row's mesh size for the widest row.
__global__ __launch_bounds__(TB) void k_mesh_sym(uint32_t N, uint64_t nnz, const uint64_t* __restrict__ row,
                                                 const uint32_t* __restrict__ rev,
                                                 const uint8_t* __restrict__ flags, const uint8_t* __restrict__ mark,
                                                 uint8_t* __restrict__ fout, unsigned long long* err,
                                                 unsigned* __restrict__ widest) {
  const uint64_t t = (uint64_t)blockIdx.x * TB + threadIdx.x;
  unsigned n = 0;
  if (t < N)
    for (uint64_t e = row[t]; e < row[t + 1]; e++) n += mark[e];
  for (int d = 32; d; d >>= 1) n = max(n, (unsigned)__shfl_xor((int)n, d, 64));
  if ((threadIdx.x & 63) == 0 && n) atomicMax(widest, n);
  if (t >= nnz) return;
  const uint8_t m = mark[t];
  fout[t] = (uint8_t)((flags[t] & F_OUT) | (m ? F_MESH : 0));
  if (m && !mark[rev[t]]) imp_defect(err, MK_ASYM, t);
}

// 64-bit fingerprint of (F_MESH per entry): k_import_fingerprint's sum of mixed words.
constexpr unsigned MFP_BLOCKS = 1024;
__global__ __launch_bounds__(TB) void k_mesh_fingerprint(uint64_t nnz, const uint8_t* __restrict__ flags,
                                                         unsigned long long* fp) {
  uint64_t x = 0;
  for (uint64_t t = (uint64_t)blockIdx.x * TB + threadIdx.x; t < nnz; t += (uint64_t)gridDim.x * TB)
    x += imp_mix((t << 1) ^ imp_mix((flags[t] & F_MESH) ? 1 : 0));
  for (int d = 32; d; d >>= 1) x += (uint64_t)__shfl_xor((unsigned long long)x, d, 64);
  if ((threadIdx.x & 63) == 0 && x) atomicAdd(fp, (unsigned long long)x);
}

struct MeshStaged {
  DevBuf<uint8_t> mark, flags, mcnt;
  DevBuf<uint32_t> mesh;
  DevBuf<unsigned long long> word;  // [0] the defect, [1] the fingerprint
  DevBuf<unsigned> widest;
};

void mesh_stage(Ctx& c, MeshStaged& g) {
  const size_t nz = c.nnz ? c.nnz : 1;
  g.mark.alloc(nz);
  g.flags.alloc(nz);
  g.mcnt.alloc(c.cfg.peers);
  g.mesh.alloc((size_t)c.cfg.peers * MESH_W);
  g.word.alloc(2);
  g.widest.alloc(1);
  GS_HIP(hipMemsetAsync(g.mark.p, 0, nz, c.stream));
  GS_HIP(hipMemsetAsync(g.word.p, 0xFF, 8, c.stream));
  GS_HIP(hipMemsetAsync(g.word.p + 1, 0, 8, c.stream));
  GS_HIP(hipMemsetAsync(g.widest.p, 0, 4, c.stream));
}

template <class T>
void mesh_swap(DevBuf<T>& a, DevBuf<T>& b) {
  std::swap(a.p, b.p);
  std::swap(a.n, b.n);
}

// The marks are set: symmetry and row widths, then the staged arrays as k_extract leaves
// them, and only then the swap. `refuse(kind, index)` throws the defect's message.
template <class Refuse>
void mesh_adopt(Ctx& c, MeshStaged& g, Refuse&& refuse) {
  const uint32_t N = c.cfg.peers;
  hipStream_t s = c.stream;
  k_mesh_sym<<<blocks(std::max<uint64_t>(c.nnz, N)), TB, 0, s>>>(N, c.nnz, c.d_row.p, c.d_rev.p, c.d_flags.p, g.mark.p,
                                                               g.flags.p, g.word.p, g.widest.p);
  GS_HIP(hipGetLastError());
  unsigned long long e = 0, h = 0;
  unsigned widest = 0;
  GS_HIP(hipMemcpyAsync(&e, g.word.p, 8, hipMemcpyDeviceToHost, s));
  GS_HIP(hipMemcpyAsync(&widest, g.widest.p, 4, hipMemcpyDeviceToHost, s));
  GS_HIP(hipStreamSynchronize(s));
  if (e != IMP_NONE) refuse(e >> IMP_KIND_SHIFT, e & ((1ull << IMP_KIND_SHIFT) - 1));
  if (widest > MESH_W) c.fail(GS_ERANGE, "mesh row exceeds GS_MESH_W entries");
  MeshArgs a{};  // what k_extract reads (no row is wider than the ELL: its error word stays untouched)
  a.row = c.d_row.p; a.col = c.d_col.p; a.flags = g.flags.p; a.stage = c.d_stage.p;
  a.counters = c.d_counters.p; a.N = N;
  k_extract<<<blocks(N), TB, 0, s>>>(a, g.mesh.p, g.mcnt.p);
  k_mesh_fingerprint<<<std::min(MFP_BLOCKS, blocks(std::max<uint64_t>(c.nnz, 1))), TB, 0, s>>>(c.nnz, g.flags.p,
                                                                                             g.word.p + 1);
  GS_HIP(hipGetLastError());
  GS_HIP(hipMemcpyAsync(&h, g.word.p + 1, 8, hipMemcpyDeviceToHost, s));
  if (c.d_until.p) GS_HIP(hipMemsetAsync(c.d_until.p, 0, c.d_until.n * 4, s));  // no back-offs come with a mesh
  for (hipStream_t st : {c.side, c.chain_pipe, c.pass_ms, c.copy, s})  // nothing still reads the old mesh
    if (st) GS_HIP(hipStreamSynchronize(st));
  mesh_swap(c.d_flags, g.flags);
  mesh_swap(c.d_mesh, g.mesh);
  mesh_swap(c.d_mcnt, g.mcnt);
  c.mesh_fp = h ? h : 1;  // 0 is a converged mesh
  c.mesh_built = true;
  c.rpos_valid = false;  // what run_mesh invalidates
  c.mesh_dmax = 0;
  c.glp_prefer = false;
  c.ring_in_tag.assign(c.ring_in_tag.size(), ~0ull);
  c.ring_ell_tag.assign(c.ring_ell_tag.size(), ~0ull);
  c.meshev_valid = false;  // the mesh events describe a converge
}

std::string mesh_at(const char* what, const char* unit, uint64_t idx) {
  return std::string(what) + " at " + unit + " " + std::to_string(idx);
}

}  // namespace

void import_mesh_ell(Ctx& c, const uint32_t* mesh, const uint8_t* count) {
  const uint32_t N = c.cfg.peers;
  const size_t slots = (size_t)N * MESH_W;
  hipStream_t s = c.stream;
  MeshStaged g;
  DevBuf<uint32_t> in;
  DevBuf<uint8_t> cnt;
  mesh_stage(c, g);
  in.alloc(slots);
  GS_HIP(hipMemcpyAsync(in.p, mesh, slots * 4, hipMemcpyHostToDevice, s));
  if (count) {
    cnt.alloc(N);
    GS_HIP(hipMemcpyAsync(cnt.p, count, N, hipMemcpyHostToDevice, s));
  }
  k_mesh_mark_ell<<<blocks(slots), TB, 0, s>>>(N, c.d_row.p, c.d_col.p, in.p, cnt.p, g.mark.p, g.word.p);
  GS_HIP(hipGetLastError());
  mesh_adopt(c, g, [&](uint64_t kind, uint64_t idx) {
    switch (kind) {
      case MK_COUNT: c.fail(GS_EINVAL, mesh_at("mesh: count > GS_MESH_W", "peer", idx));
      case MK_RANGE: c.fail(GS_EINVAL, mesh_at("mesh: id >= peers", "slot", idx));
      case MK_SELF: c.fail(GS_EINVAL, mesh_at("mesh: a peer in its own row", "slot", idx));
      case MK_NOCONN: c.fail(GS_EINVAL, mesh_at("mesh: not a connection", "slot", idx));
      case MK_REPEAT: c.fail(GS_EINVAL, mesh_at("mesh: the same peer twice in a row", "slot", idx));
      default: c.fail(GS_EINVAL, mesh_at("mesh: link without its reverse", "entry", idx));
    }
  });
}

void import_mesh_links(Ctx& c, uint64_t n, const uint32_t* la, const uint32_t* lb) {
  const uint32_t N = c.cfg.peers;
  hipStream_t s = c.stream;
  if (n >= (1ull << 32)) c.fail(GS_EINVAL, "link list: 2^32 or more links");  // (no graph has as many connections)
  MeshStaged g;
  DevBuf<uint32_t> da, db, ent;
  DevBuf<unsigned> first;
  mesh_stage(c, g);
  if (n) {
    da.alloc(n);
    db.alloc(n);
    ent.alloc(n);
    first.alloc(c.nnz ? c.nnz : 1);
    GS_HIP(hipMemcpyAsync(da.p, la, n * 4, hipMemcpyHostToDevice, s));
    GS_HIP(hipMemcpyAsync(db.p, lb, n * 4, hipMemcpyHostToDevice, s));
    GS_HIP(hipMemsetAsync(first.p, 0xFF, first.n * 4, s));
    k_mesh_first_links<<<blocks(n), TB, 0, s>>>(N, n, c.d_row.p, c.d_col.p, c.d_rev.p, da.p, db.p, ent.p, first.p,
                                                g.word.p);
    k_mesh_mark_links<<<blocks(n), TB, 0, s>>>(n, c.d_rev.p, ent.p, first.p, g.mark.p, g.word.p);
    GS_HIP(hipGetLastError());
  }
  mesh_adopt(c, g, [&](uint64_t kind, uint64_t idx) {
    switch (kind) {
      case LK_RANGE: c.fail(GS_EINVAL, mesh_at("link list: id >= peers", "link", idx));
      case LK_SELF: c.fail(GS_EINVAL, mesh_at("link list: a == b", "link", idx));
      case LK_NOCONN: c.fail(GS_EINVAL, mesh_at("link list: not a connection", "link", idx));
      case LK_REPEAT: c.fail(GS_EINVAL, mesh_at("link list: the same link twice", "link", idx));
      default: c.fail(GS_EINVAL, mesh_at("link list: internal defect kind", "entry", idx));
    }
  });
}
