// gs_linkdel.h — per-link first-delivery counts of a finished batch (gs_set_link_deliveries,
// DESIGN.md §2.16): of the fragments a peer received first, how many came over each of its
// connections — what the first-message-deliveries term P2 asks per link
// (rust-test-node/src/main.rs:252-258, go-test-node/main.go:186-193,
// nim-test-node/gossipsub-queues/main.nim:335-340).
// Included by gs_relax.hip after gs_pubsub.h.
//
// The final key of (u, m, f) is t_rel | hops | src and src is the neighbour
// whose copy won. k_linkdel<FP> reads the batch's dense final keys once, owner-computes by
// receiver row, and adds every first receipt (PubsubAcc::first's: a finite key at a
// non-publisher in a lane fl < Fe) to the counter of u's CSR entry for src, in the column
//   GS_LD_PUBLISH  src is the message's publisher (with or without flood-publish),
//   GS_LD_MESH     src is in u's row of the frozen mesh the batch ran on,
//   GS_LD_GOSSIP   neither: an IWANT answer.
// A wave owns row u: it stages the row's neighbour ids (ascending, at most MAX_DEG) in LDS with
// the mesh membership of each in bit 31, walks the row's L keys 64 at a time, finds src by
// binary search in the staged row and adds 1 to an LDS histogram [deg][GS_LD_COLS]; then lanes
// j < deg add their non-zero bins to the global counters with plain loads and stores: within a
// launch no other wave touches that row's entries, and launches are stream-ordered. No global
// atomics; integer adds commute, so the counts depend on no processing order.
// A src outside u's CSR row cannot happen under §2.5's rules: it raises ERR_LINK, counts
// nothing, and the run call fails (collect_stats).
#pragma once

struct LinkDelArgs {
  uint64_t* counts;    // [nnz][GS_LD_COLS], aligned with the CSR
  uint64_t* counters;  // the device error word (C_ERR)
  uint32_t Fe;
};

constexpr uint32_t LD_ROWS = TB / 64;  // rows per block and round, one per wave
constexpr uint32_t LD_MESH_BIT = 1u << 31;
static_assert(STAGE_SHIFT < 31, "a staged neighbour id leaves bit 31 free");

template <int FP>
__global__ __launch_bounds__(TB) void k_linkdel(RelaxArgs a, LinkDelArgs t) {
  __shared__ uint32_t ids[LD_ROWS][MAX_DEG];                // neighbour id | LD_MESH_BIT
  __shared__ uint32_t bins[LD_ROWS][MAX_DEG * GS_LD_COLS];  // the row's histogram
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint64_t smask = (1ull << a.sb) - 1;
  uint32_t* const id = ids[wv];
  uint32_t* const bin = bins[wv];
  // (block-uniform loop: every thread reaches both barriers of a round)
  for (uint32_t r0 = blockIdx.x * LD_ROWS; r0 < a.N; r0 += gridDim.x * LD_ROWS) {
    const uint32_t u = r0 + wv;
    const bool valid = u < a.N;
    uint64_t e0 = 0;
    uint32_t deg = 0, err = 0;
    if (valid) {
      e0 = a.row[u];
      deg = (uint32_t)(a.row[u + 1] - e0);
      if (deg > MAX_DEG) { err = ERR_LINK; deg = 0; }  // (no graph has such a row: gs_build_topology, the imports)
    }
    const bool work = valid && !err;
    if (work) {
      uint32_t mrow[MESH_W];
      load_mesh_row(a.mesh, u, mrow);
      for (uint32_t j = lane; j < deg; j += 64) {
        const uint32_t w = a.col[e0 + j];
        bool inm = false;
#pragma unroll
        for (int q = 0; q < (int)MESH_W; q++) inm |= mrow[q] != EMPTY && (mrow[q] & 0xFFFFFFu) == w;
        id[j] = w | (inm ? LD_MESH_BIT : 0u);
#pragma unroll
        for (int k = 0; k < GS_LD_COLS; k++) bin[j * GS_LD_COLS + k] = 0;
      }
    }
    __syncthreads();
    if (work) {
      const uint64_t* keys = a.keys + (size_t)u * a.L;
      for (uint32_t i = lane; i < a.L; i += 64) {
        const uint64_t key = keys[i];
        const uint32_t m = i / FP, fl = i & (FP - 1);
        if (key == INF64 || fl >= t.Fe) continue;
        const uint32_t pm = a.pub[m];
        if (u == pm) continue;
        const uint32_t src = (uint32_t)(key & smask);
        uint32_t lo = 0, hi = deg;  // the first staged id >= src
        while (lo < hi) {
          const uint32_t mid = (lo + hi) >> 1;
          if ((id[mid] & ~LD_MESH_BIT) < src) lo = mid + 1; else hi = mid;
        }
        const uint32_t e = lo < deg ? id[lo] : EMPTY;
        if (lo >= deg || (e & ~LD_MESH_BIT) != src) { err = ERR_LINK; continue; }
        const int k = src == pm ? GS_LD_PUBLISH : (e & LD_MESH_BIT) ? GS_LD_MESH : GS_LD_GOSSIP;
        atomicAdd(&bin[lo * GS_LD_COLS + k], 1u);
      }
    }
    __syncthreads();
    if (work) {
      for (uint32_t j = lane; j < deg; j += 64) {
        uint64_t* o = t.counts + (e0 + j) * GS_LD_COLS;
#pragma unroll
        for (int k = 0; k < GS_LD_COLS; k++) {
          const uint32_t v = bin[j * GS_LD_COLS + k];
          if (v) o[k] += v;
        }
      }
    }
    if (err) atomicOr((unsigned*)&t.counters[C_ERR], err);
    // (the next round's staging writes only what this lane itself read above)
  }
}

// gs_get_peer_given: given[col[e]][k] += edge[e][k], one thread per entry (a read-out pass).
__global__ __launch_bounds__(TB) void k_linkdel_given(const uint32_t* col, const uint64_t* edge, uint64_t nnz,
                                                      unsigned long long* given) {
  const uint64_t e = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (e >= nnz) return;
  const uint32_t w = col[e];
#pragma unroll
  for (int k = 0; k < GS_LD_COLS; k++) {
    const uint64_t v = edge[e * GS_LD_COLS + k];
    if (v) atomicAdd(&given[(size_t)w * GS_LD_COLS + k], (unsigned long long)v);
  }
}

// The counters of the context's current graph, allocated and zeroed when first needed
// (ld_ready is false after enabling, a reset, and a graph built or imported).
static void linkdel_ensure(Ctx& c) {
  if (c.ld_ready) return;
  const size_t n = std::max<size_t>(1, (size_t)c.nnz * GS_LD_COLS);
  c.d_linkdel.alloc(n);
  GS_HIP(hipMemsetAsync(c.d_linkdel.p, 0, n * 8, c.stream));
  c.ld_ready = true;
}

// The first deliveries of the batch just finished (keys final, before the next reset).
static void launch_linkdel(Ctx& c, const Batch& b) {
  if (c.keys_none) c.fail(GS_EINVAL, "internal: the link delivery pass after a no-log list pass");
  linkdel_ensure(c);
  ensure_cus(c);
  const RelaxArgs ra = relax_args(c, b, false);
  LinkDelArgs la{};
  la.counts = c.d_linkdel.p;
  la.counters = c.d_counters.p;
  la.Fe = b.Fe;
  const unsigned grid = (unsigned)std::max<uint64_t>(
      1, std::min<uint64_t>(((uint64_t)ra.N + LD_ROWS - 1) / LD_ROWS, (uint64_t)c.num_cus * 8));
  with_fp(b.FP, [&](auto fp) { k_linkdel<fp.value><<<grid, TB, 0, c.stream>>>(ra, la); });
  GS_HIP(hipGetLastError());
}


void linkdel_set(Ctx& c, bool on) {
  if (on && c.cfg.churn_ppm)
    c.fail(GS_EUNSUPPORTED, "per-link first deliveries (gs_set_link_deliveries) under churn: the mesh of a send and "
                            "of its arrival can differ, so the publish / mesh / gossip split has no single answer");
  c.linkdel = on;
  c.ld_ready = false;
  if (!on || !c.topo_built) return;
  linkdel_ensure(c);
  GS_HIP(hipStreamSynchronize(c.stream));
}

// (zeroed at the next use: a run's pass or a read-out, both on the context's stream)
void linkdel_reset(Ctx& c) { c.ld_ready = false; }

void linkdel_get(Ctx& c, uint64_t* out) {
  linkdel_ensure(c);
  if (c.nnz)
    GS_HIP(hipMemcpyAsync(out, c.d_linkdel.p, (size_t)c.nnz * GS_LD_COLS * 8, hipMemcpyDeviceToHost, c.stream));
  GS_HIP(hipStreamSynchronize(c.stream));
}

void linkdel_given(Ctx& c, uint64_t* out) {
  linkdel_ensure(c);
  const size_t n = (size_t)c.cfg.peers * GS_LD_COLS;
  DevBuf<uint64_t> given;
  given.alloc(n);
  hipStream_t s = c.stream;
  GS_HIP(hipMemsetAsync(given.p, 0, n * 8, s));
  if (c.nnz) {
    k_linkdel_given<<<(unsigned)((c.nnz + TB - 1) / TB), TB, 0, s>>>(c.d_col.p, c.d_linkdel.p, c.nnz,
                                                                    (unsigned long long*)given.p);
    GS_HIP(hipGetLastError());
  }
  GS_HIP(hipMemcpyAsync(out, given.p, n * 8, hipMemcpyDeviceToHost, s));
  GS_HIP(hipStreamSynchronize(s));
}
