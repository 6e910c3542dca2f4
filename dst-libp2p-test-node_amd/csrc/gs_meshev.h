// gs_meshev.h — mesh event counts and per-epoch mesh health of a gs_mesh_converge call
// (gs_set_mesh_events): what go-test-node/metrics.go:164-190 counts per
// node (GRAFT and PRUNE RPCs sent and received) and what its tracer follows
// (metrics.go:224-258 mesh size and Graft / Prune events, 328-362 topic health).
// Included by gs_mesh.hip, inside its unnamed namespace, after the epoch kernels.
//
// This header adds no mesh rule. Between GRAFT handling (B) and apply (C) every event of an
// epoch is a function of a row's own entries e and of prop[rev[e]] (p = prop[e], q =
// prop[rev[e]], f = flags[e]; the mesh is symmetric after every apply step):
//   GRAFT sent / received       p & PR_GRAFT / q & PR_GRAFT
//   step-A PRUNE sent / received p & PR_PRUNE / q & PR_PRUNE
//   rejected GRAFT (the PRUNE reply)  a GRAFT without PR_ACCEPT after B: sent by the row that
//                               holds q, received by the row that holds p
//   entry leaves the mesh       f & F_MESH with a PRUNE on p or q
//   entry enters the mesh       p == GRAFT|ACCEPT (the grafter's entry, set by C), or
//                               q == GRAFT|ACCEPT without an own GRAFT (the receiver's entry,
//                               which B has set already)
//   mesh size after C           entries with F_MESH and no PRUNE, plus the grafter's accepted
//   mesh size after the disconnect  entries with F_MESH less the receiver's entries B set;
//                               the row's size after the previous counted epoch (msize) minus
//                               it is what the disconnect dropped (§2.8; 0 on a frozen mesh)
// k_mesh_events runs once per counted epoch between B and C over every row (a receiver that
// only rejected carries no flag of the event-driven epochs): one row per group of G lanes as
// the row kernels, grid-stride. A row adds its seven counts to its own entries of the
// columns [col][N] (no atomic: one group per row), and the block's twelve series values go
// to the epoch's row with one atomic per block and non-zero column. Integer adds commute,
// so both results are a pure function of the input.
#pragma once

struct MeshEvArgs {
  uint64_t* ev;      // [GS_MESH_EVENT_COLS][N]
  uint32_t* msize;   // [N] mesh size after the last counted epoch
  uint64_t* series;  // [GS_MESH_SERIES_COLS] the epoch's row
};

template <int K>
__device__ __forceinline__ uint32_t me_pick(const uint32_t (&v)[K], int l) {
  uint32_t x = 0;
#pragma unroll
  for (int k = 0; k < K; k++)
    if (l == k) x = v[k];
  return x;
}

template <int G>
__global__ __launch_bounds__(TB) void k_mesh_events(MeshArgs a, MeshEvArgs m) {
  constexpr uint32_t R = TB / G;  // rows per block and round
  static_assert(G >= (int)GS_MESH_SERIES_COLS, "one lane per column");
  __shared__ uint32_t ssum[GS_MESH_SERIES_COLS];
  if (threadIdx.x < GS_MESH_SERIES_COLS) ssum[threadIdx.x] = 0;
  __syncthreads();
  const int lane = threadIdx.x & (G - 1);
  uint32_t acc[GS_MESH_SERIES_COLS] = {};  // this group's rows (group-uniform)
  for (uint32_t u = blockIdx.x * R + threadIdx.x / G; u < a.N; u += gridDim.x * R) {  // group-uniform
    const uint64_t b = a.row[u];
    const uint32_t deg = (uint32_t)(a.row[u + 1] - b);
    const uint32_t mprev = m.msize[u];
    uint32_t f[HB_PER_LANE], p[HB_PER_LANE], r[HB_PER_LANE], q[HB_PER_LANE];
#pragma unroll
    for (int k = 0; k < HB_PER_LANE; k++) {  // the row's entries, then the neighbours' proposals together
      const uint32_t i = (uint32_t)(k * G + lane);
      const bool v = i < deg;
      f[k] = v ? a.flags[b + i] : 0u;
      p[k] = v ? a.prop[b + i] : 0u;
      r[k] = v ? a.rev[b + i] : 0u;
    }
#pragma unroll
    for (int k = 0; k < HB_PER_LANE; k++) q[k] = (uint32_t)(k * G + lane) < deg ? a.prop[r[k]] : 0u;
    uint32_t gtx = 0, grx = 0, prn = 0, nprn = 0, rej = 0, nrej = 0, add = 0, del = 0, mdisc = 0, mafter = 0;
#pragma unroll
    for (int k = 0; k < HB_PER_LANE; k++) {
      if (k * G >= (int)deg) continue;  // group-uniform
      const bool mesh = (f[k] & F_MESH) != 0;
      const bool og = (p[k] & PR_GRAFT) != 0, ng = (q[k] & PR_GRAFT) != 0;
      const bool oacc = p[k] == (PR_GRAFT | PR_ACCEPT), nacc = q[k] == (PR_GRAFT | PR_ACCEPT);
      const bool pruned = ((p[k] | q[k]) & PR_PRUNE) != 0;
      const bool radd = nacc && !og;  // the receiver's side of an accepted GRAFT
      auto cnt = [&](bool x) { return (uint32_t)__popcll(gballot<G>(x)); };
      gtx += cnt(og);
      grx += cnt(ng);
      prn += cnt((p[k] & PR_PRUNE) != 0);
      nprn += cnt((q[k] & PR_PRUNE) != 0);
      rej += cnt(og && !oacc);
      nrej += cnt(ng && !nacc);
      add += cnt(oacc || radd);
      del += cnt(mesh && pruned);
      mdisc += cnt(mesh && !radd);
      mafter += cnt((mesh && !pruned) || oacc);
    }
    const uint32_t drop = mprev - mdisc;
    const uint32_t ev[GS_MESH_EVENT_COLS] = {gtx, grx, prn + nrej, nprn + rej, add, del, drop};
    static_assert(GS_ME_GRAFT_TX == 0 && GS_ME_GRAFT_RX == 1 && GS_ME_PRUNE_TX == 2 && GS_ME_PRUNE_RX == 3 &&
                      GS_ME_MESH_ADD == 4 && GS_ME_MESH_DEL == 5 && GS_ME_MESH_DROP == 6,
                  "k_mesh_events: the order of ev[]");
    const uint32_t mine = me_pick(ev, lane);
    if (lane < (int)GS_MESH_EVENT_COLS && mine) m.ev[(size_t)lane * a.N + u] += mine;
    if (lane == 0 && mafter != mprev) m.msize[u] = mafter;
    const bool on = !is_off(a.off, u);
    acc[GS_MS_ONLINE] += on;
    acc[GS_MS_NO_PEERS] += on && mafter == 0;
    acc[GS_MS_LOW] += on && mafter > 0 && mafter < a.d_lo;
    acc[GS_MS_HEALTHY] += on && mafter >= a.d_lo;
    acc[GS_MS_OVER] += on && mafter > a.d_hi;
    acc[GS_MS_LINKS] += mafter;
    acc[GS_MS_GRAFTS] += gtx;
    acc[GS_MS_REJECTS] += rej;
    acc[GS_MS_PRUNES] += prn;
    acc[GS_MS_DROPS] += drop;
    acc[GS_MS_ADDS] += add;
    acc[GS_MS_DELS] += del;
  }
  const uint32_t mine = me_pick(acc, lane);
  if (lane < (int)GS_MESH_SERIES_COLS && mine) atomicAdd(&ssum[lane], mine);
  __syncthreads();
  if (threadIdx.x < GS_MESH_SERIES_COLS && ssum[threadIdx.x])
    atomicAdd((unsigned long long*)&m.series[threadIdx.x], (unsigned long long)ssum[threadIdx.x]);
}

// Series rows the device holds between two read-backs: every epoch of a churn converge
// (nothing synchronises between its epochs), a small chunk of the stepped epochs of a frozen
// one, whose loop reads a word back after every epoch anyway and whose max_heartbeats bounds
// nothing (a fixed point is reached after some tens of stepped epochs).
constexpr uint32_t ME_CHUNK = 8;

// Rows [0, c.me_used) of the device chunk to the host list of stepped rows; the chunk is clear again.
static void me_flush(Ctx& c) {
  if (!c.me_used) return;
  const size_t words = (size_t)c.me_used * GS_MESH_SERIES_COLS, at = c.me_stepped.size();
  c.me_stepped.resize(at + words);
  GS_HIP(hipMemcpyAsync(c.me_stepped.data() + at, c.d_ms.p, words * 8, hipMemcpyDeviceToHost, c.stream));
  GS_HIP(hipMemsetAsync(c.d_ms.p, 0, words * 8, c.stream));
  GS_HIP(hipStreamSynchronize(c.stream));
  c.me_used = 0;
}

// Start of a counted converge: both results zeroed. `rows`: the series rows the device must
// hold at once.
static void me_begin(Ctx& c, uint64_t rows) {
  const size_t N = c.cfg.peers;
  hipStream_t s = c.stream;
  ensure_cus(c);
  c.meshev_valid = false;
  c.me_epochs.clear();
  c.me_stepped.clear();
  c.me_series.clear();
  c.me_used = 0;
  c.me_cap = (uint32_t)std::max<uint64_t>(rows, 1);
  c.d_ms.alloc((size_t)c.me_cap * GS_MESH_SERIES_COLS);
  GS_HIP(hipMemsetAsync(c.d_ms.p, 0, (size_t)c.me_cap * GS_MESH_SERIES_COLS * 8, s));
  GS_HIP(hipMemsetAsync(c.d_me.p, 0, N * GS_MESH_EVENT_COLS * 8, s));
  GS_HIP(hipMemsetAsync(c.d_me_size.p, 0, N * 4, s));
}

// The events of epoch a.epoch, enqueued on s between its GRAFT handling and its apply step.
// (frozen converge: s is the context's stream, which a full chunk's read-back waits for)
static void me_epoch(Ctx& c, const MeshArgs& a, uint32_t G, hipStream_t s) {
  if (c.me_used == c.me_cap) me_flush(c);
  MeshEvArgs m{};
  m.ev = c.d_me.p;
  m.msize = c.d_me_size.p;
  m.series = c.d_ms.p + (size_t)c.me_used * GS_MESH_SERIES_COLS;
  const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(row_blocks(a.N, G), (uint64_t)c.num_cus * 8));
  if (G == 16) k_mesh_events<16><<<grid, TB, 0, s>>>(a, m);
  else k_mesh_events<64><<<grid, TB, 0, s>>>(a, m);
  c.me_epochs.push_back(a.epoch);
  c.me_used++;
}

// End of a counted converge that stepped up to epoch `last`: the series rows 0..last on the
// host. An epoch the frozen-mesh jump skipped (or epoch 0 without the subscription exchange)
// changed nothing: no events, the previous row's gauges; before epoch 0 the mesh is empty
// and everyone online.
static void me_finish(Ctx& c, uint32_t last) {
  me_flush(c);
  const size_t W = GS_MESH_SERIES_COLS;
  c.me_series.assign(((size_t)last + 1) * W, 0);
  uint64_t prev[GS_MESH_SERIES_COLS] = {};
  prev[GS_MS_ONLINE] = prev[GS_MS_NO_PEERS] = c.cfg.peers;
  size_t k = 0;
  for (uint32_t h = 0; h <= last; h++) {
    uint64_t* row = c.me_series.data() + (size_t)h * W;
    if (k < c.me_epochs.size() && c.me_epochs[k] == h) {
      std::copy_n(c.me_stepped.data() + k * W, W, row);
      k++;
    } else {
      for (uint32_t j = 0; j <= GS_MS_LINKS; j++) row[j] = prev[j];
    }
    std::copy_n(row, W, prev);
  }
  if (k != c.me_epochs.size()) c.fail(GS_EINVAL, "internal: mesh event rows out of epoch order");
  c.me_stepped.clear();
  c.me_stepped.shrink_to_fit();
}
