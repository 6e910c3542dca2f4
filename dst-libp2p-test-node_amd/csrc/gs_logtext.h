// gs_logtext.h — the arrival log formatted on the device: the
// bytes gs_log_write_lat (gs_host.cpp) would write for a batch's u16 latencies,
// built in message-major order from the message-major latencies [B][N], handed
// out chunk by chunk (whole messages under a byte budget) through two device
// text buffers and two pinned host buffers, the copy of chunk k on the copy
// stream beside the formatting of chunk k + 1. Included by gs_relax.hip.
//
// The context's rows are the peers [u0, u0 + N): all of them (gs_run_log, gs_format_lat_log:
// u0 = 0), or the range a part of gs_run_partitioned_log owns. Latencies, line numbers and
// counters are indexed by row; the line carries the global id u0 + row.
//
// A line: shadow.data/hosts/peer<u>/main.1000.stdout:<line>:<id> milliseconds: <ms>\n
//   <id> = the message's preformatted id string (t_pub_ns as %lld; nim: msgId),
//   <line> = the peer's line counter (u32 [N], carried across batches and calls).
// Per chunk of nm messages, G = ceil(N / 64) groups of 64 consecutive rows each (a part's
// first group starts at its first peer, at no multiple of 64 of the global id):
//   k_lt_count  lane = row, loop over the chunk's messages: line numbers (the counter
//               carried in a register, stored back once), line lengths, and per
//               (message, group) the bytes and lines of its 64 peers;
//   k_lt_scan   one block: exclusive prefix sum of those in (message, group) order
//               = every group's byte offset; the chunk's bytes and lines;
//   k_lt_emit   wave = one (message, group): its 64 lines are one contiguous run of
//               the text, built in LDS at the run's offset mod 16 and copied out in
//               aligned 16-byte stores (byte stores for the < 16-byte head and tail).
// No atomic decides a byte position: the text is a pure function of the input.
#pragma once

constexpr uint32_t LT_ID_MAX = 20;      // "%lld" of an int64, a 19-digit nim msgId
constexpr uint32_t LT_ID_STRIDE = 24;   // per message: the id's chars, its length in byte 23
constexpr uint32_t LT_FIXED = 22 + 18 + 1 + 15 + 1;  // the line's constant text
constexpr uint32_t LT_LINE_MAX = LT_FIXED + 8 + 10 + LT_ID_MAX + 5;  // peers < 2^24, line u32, ms u16
constexpr uint32_t LT_WAVES = 4;
constexpr uint32_t LT_RUN = 64 * LT_LINE_MAX + 16;  // a wave's run + its offset mod 16
constexpr uint32_t LT_SCAN_T = 1024;
constexpr uint64_t LT_CHUNK_DEFAULT = 256ull << 20;
static_assert(LT_RUN % 16 == 0, "runs are read back as 16-byte slots");
static_assert(LT_LINE_MAX == 100, "gs_log_line_max (gs_host.cpp) counts the same line");

struct LtArgs {
  const uint16_t* lat_t;  // [nm][N] the chunk's latencies, message-major
  const uint8_t* ids;     // [nm][LT_ID_STRIDE]
  uint32_t* cnt;          // [N] line counters
  uint32_t* ln;           // [nm][N] line numbers (0 = no line)
  uint32_t* gsum;         // [nm][G] bytes | lines << 16 of a group
  uint64_t* goff;         // [nm][G] byte offset of a group's run
  uint64_t* meta;         // [0] bytes, [1] lines, [2] a line counter passed 2^32 - 1
  char* text;
  uint32_t N, nm, G;      // N: own rows
  uint32_t u0;            // the peer of row 0
};

__device__ __forceinline__ uint32_t lt_div10(uint32_t v) { return __umulhi(v, 0xCCCCCCCDu) >> 3; }
__device__ __forceinline__ uint32_t lt_digits(uint32_t v) {
  return 1u + (v >= 10u) + (v >= 100u) + (v >= 1000u) + (v >= 10000u) + (v >= 100000u) + (v >= 1000000u) +
         (v >= 10000000u) + (v >= 100000000u) + (v >= 1000000000u);
}
__device__ __forceinline__ uint32_t lt_len(uint32_t u, uint32_t line, uint32_t idlen, uint32_t ms) {
  return LT_FIXED + lt_digits(u) + lt_digits(line) + idlen + lt_digits(ms);
}
// v in decimal at p[0 .. nd)
__device__ __forceinline__ unsigned char* lt_put(unsigned char* p, uint32_t v, uint32_t nd) {
  for (uint32_t k = nd; k-- > 0;) {
    const uint32_t q = lt_div10(v);
    p[k] = (unsigned char)('0' + (v - q * 10u));
    v = q;
  }
  return p + nd;
}

__global__ __launch_bounds__(LT_WAVES * 64) void k_lt_count(LtArgs a) {
  const uint32_t lane = threadIdx.x & 63, g = blockIdx.x * LT_WAVES + (threadIdx.x >> 6);
  if (g >= a.G) return;  // (whole waves)
  const uint32_t u = g * 64 + lane;
  const bool in = u < a.N;
  uint32_t c = in ? a.cnt[u] : 0u;
  bool over = false;
  for (uint32_t m = 0; m < a.nm; m++) {
    const uint32_t idlen = a.ids[(size_t)m * LT_ID_STRIDE + LT_ID_STRIDE - 1];
    const uint32_t v = in ? a.lat_t[(size_t)m * a.N + u] : GS_LAT_NONE;
    const bool lg = v != GS_LAT_NONE;
    if (lg) {
      over = over || c == 0xFFFFFFFFu;
      c++;
    }
    if (in) a.ln[(size_t)m * a.N + u] = lg ? c : 0u;
    uint32_t s = lg ? (lt_len(a.u0 + u, c, idlen, v) | 1u << 16) : 0u;  // <= 64 * 100 bytes, 64 lines
    for (int d = 32; d; d >>= 1) s += __shfl_xor(s, d);
    if (lane == 0) a.gsum[(size_t)m * a.G + g] = s;
  }
  if (in) a.cnt[u] = c;
  if (over) a.meta[2] = 1;
}

// A whole batch before any of its text leaves (gs_run_partitioned_log: no part hands out a
// chunk of a batch that fails in any part): would a row's counter pass 2^32 - 1 over the
// batch's B messages? lane = row; ERR_LINES into the counters' error word.
__global__ __launch_bounds__(LT_WAVES * 64) void k_lt_room(const uint16_t* __restrict__ lat_t,
                                                           const uint32_t* __restrict__ cnt, uint32_t N, uint32_t B,
                                                           uint64_t* counters) {
  const uint32_t u = blockIdx.x * (LT_WAVES * 64) + threadIdx.x;
  if (u >= N) return;
  uint64_t c = cnt[u];
  for (uint32_t m = 0; m < B; m++) c += lat_t[(size_t)m * N + u] != GS_LAT_NONE;
  if (c > 0xFFFFFFFFull) atomicOr((unsigned*)&counters[C_ERR], ERR_LINES);
}

__global__ __launch_bounds__(LT_SCAN_T) void k_lt_scan(LtArgs a) {
  __shared__ uint64_t sb[LT_SCAN_T], sl[LT_SCAN_T];
  const uint64_t n = (uint64_t)a.nm * a.G, per = (n + LT_SCAN_T - 1) / LT_SCAN_T;
  const uint32_t t = threadIdx.x;
  const uint64_t i0 = min(n, t * per), i1 = min(n, i0 + per);
  uint64_t b = 0, l = 0;
  for (uint64_t i = i0; i < i1; i++) {
    const uint32_t s = a.gsum[i];
    b += s & 0xFFFFu;
    l += s >> 16;
  }
  sb[t] = b;
  sl[t] = l;
  __syncthreads();
  for (uint32_t d = 1; d < LT_SCAN_T; d <<= 1) {  // inclusive scan of the threads' sums
    const uint64_t xb = t >= d ? sb[t - d] : 0, xl = t >= d ? sl[t - d] : 0;
    __syncthreads();
    sb[t] += xb;
    sl[t] += xl;
    __syncthreads();
  }
  uint64_t off = sb[t] - b;
  for (uint64_t i = i0; i < i1; i++) {
    a.goff[i] = off;
    off += a.gsum[i] & 0xFFFFu;
  }
  if (t == LT_SCAN_T - 1) {
    a.meta[0] = sb[t];
    a.meta[1] = sl[t];
  }
}

__global__ __launch_bounds__(LT_WAVES * 64) void k_lt_emit(LtArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned char sm[LT_WAVES][LT_RUN];
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint64_t w = (uint64_t)blockIdx.x * LT_WAVES + wv, nw = (uint64_t)a.nm * a.G;
  const bool wave_in = w < nw;  // (no early return: the block's barrier below)
  const uint32_t m = wave_in ? (uint32_t)(w / a.G) : 0u, g = wave_in ? (uint32_t)(w % a.G) : 0u;
  const uint32_t u = g * 64 + lane;
  const bool in = wave_in && u < a.N;
  const uint8_t* id = a.ids + (size_t)m * LT_ID_STRIDE;
  const uint32_t idlen = id[LT_ID_STRIDE - 1];
  const uint32_t v = in ? a.lat_t[(size_t)m * a.N + u] : GS_LAT_NONE;
  const bool lg = v != GS_LAT_NONE;
  const uint32_t line = lg ? a.ln[(size_t)m * a.N + u] : 0u;
  const uint32_t id_u = a.u0 + u;  // the peer the line names
  const uint32_t du = lt_digits(id_u), dl = lt_digits(line), dv = lt_digits(v);
  const uint32_t len = lg ? LT_FIXED + du + dl + idlen + dv : 0u;
  uint32_t inc = len;  // inclusive prefix sum over the lanes
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t x = __shfl_up(inc, d);
    if ((int)lane >= d) inc += x;
  }
  const uint32_t T = __shfl(inc, 63);
  const uint64_t base = wave_in ? a.goff[w] : 0;
  const uint32_t shift = (uint32_t)(base & 15u);
  unsigned char* run = sm[wv];
  if (lg) {
    unsigned char* p = run + shift + (inc - len);
    constexpr char PFX[] = "shadow.data/hosts/peer", MID[] = "/main.1000.stdout:", MSW[] = " milliseconds: ";
#pragma unroll
    for (int i = 0; i < 22; i++) p[i] = (unsigned char)PFX[i];
    p = lt_put(p + 22, id_u, du);
#pragma unroll
    for (int i = 0; i < 18; i++) p[i] = (unsigned char)MID[i];
    p = lt_put(p + 18, line, dl);
    *p++ = ':';
    for (uint32_t i = 0; i < idlen; i++) p[i] = id[i];
    p += idlen;
#pragma unroll
    for (int i = 0; i < 15; i++) p[i] = (unsigned char)MSW[i];
    p = lt_put(p + 15, v, dv);
    *p = '\n';
  }
  __syncthreads();
  if (!wave_in || T == 0) return;
  // LDS byte i of the run <-> text byte base - shift + i: 16-byte slots line up
  unsigned char* dst = (unsigned char*)a.text + (base - shift);
  const uint32_t end = shift + T;
  const uint32_t j0 = (shift + 15u) >> 4, j1 = end >> 4;  // whole slots [j0, j1)
  const uint32_t head_end = min(j0 * 16u, end);
  if (shift + lane < head_end) dst[shift + lane] = run[shift + lane];
  for (uint32_t j = j0 + lane; j < j1; j += 64)
    *(uint4*)(dst + (size_t)j * 16) = *(const uint4*)(run + (size_t)j * 16);
  const uint32_t tail = max(j1 * 16u, head_end);
  if (tail + lane < end) dst[tail + lane] = run[tail + lane];
}

// The id string a message's lines carry (gs_host.cpp log_line_ms).
static uint32_t lt_msg_id(const gs_config& cfg, const gs_publish& p, uint8_t* out) {
  char buf[32];
  int n;
  if (cfg.node == GS_NODE_NIM) n = snprintf(buf, sizeof buf, "%llu", (unsigned long long)nim_msg_id(cfg.seed, p.publisher, p.t_pub_ns));
  else n = snprintf(buf, sizeof buf, "%lld", (long long)p.t_pub_ns);
  if (n < 1 || n > (int)LT_ID_MAX) throw Error(GS_ERANGE, "arrival log: a message id longer than 20 characters");
  memset(out, 0, LT_ID_STRIDE);
  memcpy(out, buf, (size_t)n);
  out[LT_ID_STRIDE - 1] = (uint8_t)n;
  return (uint32_t)n;
}

// The line counters of the context's un rows: zero at gs_create (allocated at the first use),
// and again when the rows are another range than the counters were kept for (part_set
// forgets them when the partition changes).
static void lt_counters(Ctx& c, uint32_t un) {
  if (c.d_tcnt.p && c.tcnt_n == un) return;
  c.d_tcnt.alloc(un);
  GS_HIP(hipMemsetAsync(c.d_tcnt.p, 0, (size_t)un * 4, c.stream));
  c.tcnt_n = un;
}

// The text of messages [0, B) (schedule rows sched[0 .. B), message-major latencies
// lat_t[B][un] of the peers [u0, u0 + un) on the device, ready on the context's stream)
// to c.text's callback, first_msg counted from row0.
static void text_emit(Ctx& c, const uint16_t* lat_t, uint32_t B, const gs_publish* sched, uint64_t row0, uint32_t u0,
                      uint32_t un) {
  hipStream_t s = c.stream;
  const uint32_t N = un, G = (N + 63) / 64;
  if (!c.copy) GS_HIP(hipStreamCreateWithFlags(&c.copy, hipStreamNonBlocking));
  if (c.text_busy) {  // a call that failed half way: nothing of it is in flight any more
    GS_HIP(hipStreamSynchronize(c.copy));
    GS_HIP(hipStreamSynchronize(s));
  }
  c.text_busy = true;
  for (int k = 0; k < 2; k++) {
    if (!c.text_meta_ev[k]) GS_HIP(hipEventCreateWithFlags(&c.text_meta_ev[k], hipEventDisableTiming));
    if (!c.text_fmt_ev[k]) GS_HIP(hipEventCreateWithFlags(&c.text_fmt_ev[k], hipEventDisableTiming));
    if (!c.text_done_ev[k]) GS_HIP(hipEventCreateWithFlags(&c.text_done_ev[k], hipEventDisableTiming));
  }
  if (!c.h_tmeta) GS_HIP(hipHostMalloc((void**)&c.h_tmeta, 2 * 4 * 8, hipHostMallocDefault));
  lt_counters(c, un);
  // ids, and every message's bound: N lines of the longest it can have
  std::vector<uint8_t> ids((size_t)B * LT_ID_STRIDE);
  std::vector<uint64_t> bound(B);
  const uint32_t dpeer = (uint32_t)std::to_string(u0 + un - 1).size();
  uint64_t bmax = 0, btot = 0;
  for (uint32_t m = 0; m < B; m++) {
    const uint32_t idlen = lt_msg_id(c.cfg, sched[m], &ids[(size_t)m * LT_ID_STRIDE]);
    bound[m] = (uint64_t)N * (LT_FIXED + dpeer + 10 + idlen + 5);
    bmax = std::max(bmax, bound[m]);
    btot += bound[m];
  }
  const uint64_t cap = std::min(btot, std::max(c.text.chunk ? c.text.chunk : LT_CHUNK_DEFAULT, bmax));
  const uint64_t nm_max = std::max<uint64_t>(1, cap / ((uint64_t)N * (LT_FIXED + dpeer + 10 + 1 + 5)));
  const size_t cells = (size_t)std::min<uint64_t>(B, nm_max);
  c.d_tids.alloc(std::max<size_t>(ids.size(), (size_t)c.cfg.batch * LT_ID_STRIDE));
  GS_HIP(hipMemcpyAsync(c.d_tids.p, ids.data(), ids.size(), hipMemcpyHostToDevice, s));
  c.d_tln.alloc(cells * N);
  c.d_tgsum.alloc(cells * G);
  c.d_tgoff.alloc(cells * G);
  c.d_tmeta.alloc(4);
  for (int k = 0; k < 2; k++) {
    c.d_text[k].alloc((size_t)cap + 16);
    if (c.h_text_bytes[k] < cap) {
      if (c.h_text[k]) GS_HIP(hipHostFree(c.h_text[k]));
      c.h_text[k] = nullptr;
      c.h_text_bytes[k] = 0;
      GS_HIP(hipHostMalloc((void**)&c.h_text[k], (size_t)cap, hipHostMallocDefault));
      c.h_text_bytes[k] = (size_t)cap;
    }
  }
  struct Pend {
    bool on = false;
    uint32_t par = 0, n = 0;
    uint64_t first = 0, bytes = 0, lines = 0;
  } pend;
  auto hand_over = [&] {
    if (!pend.on) return;
    pend.on = false;
    GS_HIP(hipEventSynchronize(c.text_done_ev[pend.par]));
    c.text.fn(c.text.user, pend.first, pend.n, c.h_text[pend.par], pend.bytes, pend.lines);
  };
  for (uint32_t m0 = 0; m0 < B;) {
    uint32_t nm = 1;  // whole messages under the budget (a message's bound always fits)
    for (uint64_t sum = bound[m0]; m0 + nm < B && nm < cells && sum + bound[m0 + nm] <= cap; nm++) sum += bound[m0 + nm];
    const uint32_t par = c.text_par;
    c.text_par ^= 1u;
    // (buffer `par` is free: its last chunk was handed over before the other parity's was enqueued)
    LtArgs a{};
    a.lat_t = lat_t + (size_t)m0 * N; a.ids = c.d_tids.p + (size_t)m0 * LT_ID_STRIDE; a.cnt = c.d_tcnt.p;
    a.ln = c.d_tln.p; a.gsum = c.d_tgsum.p; a.goff = c.d_tgoff.p; a.meta = c.d_tmeta.p; a.text = c.d_text[par].p;
    a.N = N; a.nm = nm; a.G = G; a.u0 = u0;
    GS_HIP(hipMemsetAsync(c.d_tmeta.p, 0, 4 * 8, s));
    k_lt_count<<<(G + LT_WAVES - 1) / LT_WAVES, LT_WAVES * 64, 0, s>>>(a);
    k_lt_scan<<<1, LT_SCAN_T, 0, s>>>(a);
    GS_HIP(hipMemcpyAsync(c.h_tmeta + par * 4, c.d_tmeta.p, 4 * 8, hipMemcpyDeviceToHost, s));
    GS_HIP(hipEventRecord(c.text_meta_ev[par], s));
    const uint64_t nw = (uint64_t)nm * G;
    k_lt_emit<<<(unsigned)((nw + LT_WAVES - 1) / LT_WAVES), LT_WAVES * 64, 0, s>>>(a);
    GS_HIP(hipGetLastError());
    GS_HIP(hipEventRecord(c.text_fmt_ev[par], s));
    GS_HIP(hipEventSynchronize(c.text_meta_ev[par]));
    const uint64_t bytes = c.h_tmeta[par * 4], lines = c.h_tmeta[par * 4 + 1];
    if (c.h_tmeta[par * 4 + 2]) {
      hand_over();  // (the chunk before it is whole)
      c.fail(GS_ERANGE, "arrival log: a peer's line counter would pass 2^32 - 1");
    }
    if (bytes > cap) c.fail(GS_EDEVICE, "internal: arrival log chunk larger than its bound");
    GS_HIP(hipStreamWaitEvent(c.copy, c.text_fmt_ev[par], 0));
    if (bytes) GS_HIP(hipMemcpyAsync(c.h_text[par], c.d_text[par].p, (size_t)bytes, hipMemcpyDeviceToHost, c.copy));
    GS_HIP(hipEventRecord(c.text_done_ev[par], c.copy));
    hand_over();  // chunk k - 1, while chunk k is formatted and copied
    pend.on = true;
    pend.par = par;
    pend.n = nm;
    pend.first = row0 + m0;
    pend.bytes = bytes;
    pend.lines = lines;
    m0 += nm;
  }
  hand_over();
  c.text_busy = false;
}

// gs_run_log's and gs_run_partitioned_log's sink (deliver): the finished batch's peer-major
// d_lat of the peers [u0, u0 + un) as text. A partitioned batch comes staged (part_lat_stage:
// message-major already, every part's error word checked by the caller).
static void deliver_text(Ctx& c, const Batch& b, uint32_t u0, uint32_t un, uint64_t sink_row0) {
  hipStream_t s = c.stream;
  if (c.lat_staged) {
    c.lat_staged = false;
    text_emit(c, c.d_lat_t.p, b.B, c.text.sched + sink_row0, sink_row0, u0, un);
    return;
  }
  c.d_lat_t.alloc((size_t)un * c.cfg.batch);
  dim3 tg((un + 63) / 64, (b.B + 63) / 64);
  k_transpose16<<<tg, TB, 0, s>>>(c.d_lat.p, c.d_lat_t.p, un, b.B);
  GS_HIP(hipGetLastError());
  pd_accumulate(c, c.d_lat_t.p, c.d_tpub.p, b.B, un);  // (a staged batch: part_lat_stage did)
  GS_HIP(hipMemcpyAsync(c.h_pinned, c.d_counters.p + C_ERR, 8, hipMemcpyDeviceToHost, s));
  GS_HIP(hipStreamSynchronize(s));
  if (c.h_pinned[0] & ERR_LAT16)  // before any text of the batch is handed out
    c.fail(GS_ERANGE, "a logged latency of 65535 ms or more does not fit the arrival log's u16 latencies");
  text_emit(c, c.d_lat_t.p, b.B, c.text.sched + sink_row0, sink_row0, u0, un);
}

// gs_format_lat_log: the same over a caller's message-major lat_ms[n_msgs][N].
void format_lat_log(Ctx& c, const gs_publish* sched, uint64_t n_msgs, const uint16_t* lat_ms) {
  const uint32_t N = c.cfg.peers;
  const uint64_t piece = std::max<uint64_t>(1, std::min<uint64_t>(n_msgs, (64ull << 20) / N));  // <= 128 MB staged
  c.d_lat_t.alloc((size_t)piece * N);
  for (uint64_t m0 = 0; m0 < n_msgs; m0 += piece) {
    const uint32_t B = (uint32_t)std::min<uint64_t>(piece, n_msgs - m0);
    GS_HIP(hipMemcpyAsync(c.d_lat_t.p, lat_ms + m0 * N, (size_t)B * N * 2, hipMemcpyHostToDevice, c.stream));
    text_emit(c, c.d_lat_t.p, B, sched + m0, m0, 0, N);
  }
}

void log_text_reset(Ctx& c) {
  if (!c.d_tcnt.p || !c.tcnt_n) return;
  GS_HIP(hipMemsetAsync(c.d_tcnt.p, 0, (size_t)c.tcnt_n * 4, c.stream));
  GS_HIP(hipStreamSynchronize(c.stream));
}
