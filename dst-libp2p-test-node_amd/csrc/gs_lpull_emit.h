// k_lpull's step 4, the emit loop of one row: included in the kernel's body
// (gs_lpull_kernel.h) once per form, with LP_EMIT_PUB set by the includer.
//   LP_EMIT_PUB 1: the message's publisher is loaded where the row needs it
//                  (needp) and excluded from the receivers.
//   LP_EMIT_PUB 0: a row that is no publisher nor a publisher's neighbour, of an
//                  instantiation whose loop then has no load at all (FP == 1, no
//                  IDONTWANT, no churn): pm is the constant EMPTY, which no peer
//                  id is, so neither the receivers nor the final mask test it.
// gfx950 counts loads and stores in one in-order vmcnt and the compiler cannot
// count the record stores of this loop (variable trip count), so the wait for
// the publisher load is a vmcnt(0): with the load in the body, every iteration
// of every row drained the previous iteration's record stores, although only
// the rows of LP_PUB issue it.
#ifndef LP_EMIT_PUB
#error "gs_lpull_emit.h: set LP_EMIT_PUB"
#endif
      for (uint32_t g0 = 0; g0 < cnt; g0 += GPW) {
        const uint32_t gi = g0 + (uint32_t)lane / FP;
        const bool gv = gi < cnt;
        const uint32_t grp = gv ? LST[gi] : 0;
        const uint32_t i = grp * FP + (lane & (FP - 1));
        const uint64_t x = gv ? CW[i] : INF64;  // final lanes were set to INF in step 3
        // the message's publisher (excluded from the receivers); a row that is
        // no publisher nor a publisher's neighbour needs none (no load)
        uint32_t pm = EMPTY;
#if LP_EMIT_PUB
        if (needp) pm = gv ? a.pub[psl + grp] : EMPTY;
#endif
        // FP == 1: LST holds only lanes final in window c; a fragment group's
        // other lanes are re-checked
        const bool act = gv && (FP == 1 || (x != INF64 && ((uint32_t)(x >> 32) - hlo) < hspan))
#if LP_EMIT_PUB
                         && u0 + w != pm
#endif
            ;
        const uint32_t src = (uint32_t)x & ((1u << sbe) - 1u);  // sb < 32
        uint32_t xm = 0;  // excluded mesh indices: source, publisher (IDW: and IDONTWANT)
        uint64_t im64 = 0;  // churn: the receivers as a mask over the CSR row
        if constexpr (CHN) {  // the mesh of the epoch the lane was received in, less source and publisher
          const uint32_t kk = kc + ((x >> tse) >= eBc ? 1u : 0u);
          const uint64_t mmv = act ? a.cmm[(size_t)w * a.cE + a.cq[grp] + kk] : 0ull;
          uint64_t xm64 = 0;
          for (uint32_t k = 0; k < deg; k++) {  // wave-uniform: entry k from lane k
            const uint32_t y = __builtin_amdgcn_readlane(ej, k) & 0xFFFFFFu;
            xm64 |= (y == src || y == pm) ? 1ull << k : 0ull;
          }
          im64 = mmv & ~xm64;
        } else if constexpr (IDW) {
          // IDONTWANT from y already here: ky + lat(y -> w) <= t_w. The keys of
          // IB mesh entries are loaded before any is tested (one round trip per
          // IB entries instead of one per entry; CH = 8 rows run at 80 VGPRs).
          // Fragment groups: lane i is one fragment, so a group's lanes read
          // consecutive keys of y's row (one segment per group); a lane not
          // final in this window (act false: final earlier, pending or
          // padding) loads nothing and counts no receiver
          constexpr uint32_t IB = CH == 8 ? 2 : 8;
          const uint64_t tw = x >> tse;
          for (uint32_t k0 = 0; k0 < deg; k0 += IB) {  // wave-uniform: entry k from lane k
            uint64_t ky[IB];
#pragma unroll
            for (uint32_t u = 0; u < IB; u++) {
              const uint32_t k = k0 + u;
              const uint32_t y = k < deg ? (uint32_t)__builtin_amdgcn_readlane(ej, k) & 0xFFFFFFu : src;
              ky[u] = act && y != src && y != pm ? a.keys[(size_t)y * LL + i] : INF64;
            }
#pragma unroll
            for (uint32_t u = 0; u < IB; u++) {
              const uint32_t k = k0 + u;
              if (k >= deg) break;  // (wave-uniform)
              const uint32_t e = __builtin_amdgcn_readlane(ej, k);
              const uint32_t y = e & 0xFFFFFFu;
              const bool sk = y == src || y == pm ||
                              (ky[u] != INF64 && (ky[u] >> tse) + lat[(e >> STAGE_SHIFT) * Se + sw] <= tw);
              xm |= sk ? 1u << k : 0u;
            }
          }
        } else if constexpr (XMV) {
          // rows of 1024 single-fragment lanes (XMV, set by the includer with ejm,
          // the entries' peer ids): entry k from lane k by constant lane index, a
          // block for entries 15-8 in the rows that have them (wave-uniform) and
          // one for 7-0, not a loop of deg trips (a lane read by a scalar index,
          // its shift and mask, the counter and the branch were 10 instructions
          // per entry). The lanes past deg hold EMPTY's low 24 bits, no peer's id
          // (no src) and not EMPTY (no pm), and im keeps only the bits below deg.
          auto xblock = [&](const int k0) {
#pragma unroll
            for (int k = k0 + 7; k >= k0; k--) {
              const uint32_t y = __builtin_amdgcn_readlane(ejm, k);
              // (from the top entry down, the mask doubled and the compare added:
              // the compiler reads each lane once and needs no shift per bit)
#if LP_EMIT_PUB
              xm = xm + xm + (uint32_t)(y == src || y == pm);
#else
              xm = xm + xm + (uint32_t)(y == src);
#endif
            }
          };
          static_assert(MESH_W == 16, "the excluded-entry mask: two blocks of 8 mesh entries");
          if (deg > 8) xblock(8);
          xblock(0);
        } else {
          // (rows of 512 lanes and fragment groups sit at their VGPR limits: the
          // unrolled form costs every one of them scratch)
          for (uint32_t k = 0; k < deg; k++) {  // wave-uniform: entry k from lane k
            const uint32_t y = __builtin_amdgcn_readlane(ej, k) & 0xFFFFFFu;
#if LP_EMIT_PUB
            xm |= (y == src || y == pm) ? 1u << k : 0u;
#else
            xm |= y == src ? 1u << k : 0u;
#endif
          }
        }
        const uint32_t im = CHN ? 0u : ((1u << deg) - 1u) & ~xm;  // the receivers (deg <= MESH_W = 16)
        const uint32_t n = act ? (CHN ? (uint32_t)__popcll(im64) : (uint32_t)__popc(im)) : 0u;
        const uint64_t start = uplink_start<FP>(a.busy, (size_t)w * a.B + grp, act, x, n, serw, tse);
        const uint32_t hp = (uint32_t)(x >> sbe) & hmask;
        if (act) {
          fd++;
          nr += n;
          if constexpr (NOLOG) {  // k_lsum's ms: floor(t / 1e6) = floor(floor(t / 64) / 15625), t < 2^38
            s_ls += (uint32_t)((x >> tse) >> 6) / 15625u;
            s_max = x > s_max ? x : s_max;  // the key orders by time first
          }
          if (n && hp + 1 >= (1u << HOP_BITS)) err |= ERR_HOPS;
          if (start - wlo >= (1ull << 32) || (n && start >= tlim)) err |= ERR_TIME;
        }
        // act as lane masks: listed (gi < cnt) and not the message's publisher
#if LP_EMIT_PUB
        const uint64_t fm = FP == 1 ? (__builtin_amdgcn_uicmp(gi, cnt, 36) & __builtin_amdgcn_uicmp(pm, u0 + w, 33))
                                    : __ballot(act);  // final log: 64 entries per store
#else
        const uint64_t fm = __builtin_amdgcn_uicmp(gi, cnt, 36);
#endif
        if constexpr (IDW) {
          if (act) a.keys[(size_t)w * LL + i] = x;  // dense: the neighbours' IDONTWANT tests read it
        } else if constexpr (!NOLOG) {
          if (act) {
            const uint32_t p =
                logc + __builtin_amdgcn_mbcnt_hi((uint32_t)(fm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)fm, 0u));
            // the final log is read after the passes (completion): stream it past the caches
            __builtin_nontemporal_store(x, &a.keys[(size_t)w * LL + p]);
            __builtin_nontemporal_store((uint16_t)i, &a.flane[(size_t)w * LL + p]);
          }
          logc += (uint32_t)__popcll(fm);
        }
        const bool want = act && n != 0;
        const uint64_t wm = fm & __builtin_amdgcn_uicmp(n, 0u, 33);
        if (want) {
          const size_t ri = (size_t)w * LL + ecnt +
                            __builtin_amdgcn_mbcnt_hi((uint32_t)(wm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)wm, 0u));
          if constexpr (CHN) {
            uni |= im64;
            const uint64_t r0 = ((start - wlo) << 32) | ((uint64_t)hp << LP_HOP_SHIFT) | i;
            *reinterpret_cast<uint4*>(wrec + ri * 2) =
                make_uint4((uint32_t)r0, (uint32_t)(r0 >> 32), (uint32_t)im64, (uint32_t)(im64 >> 32));
          } else {
            const uint64_t rv = ((start - wlo) << 32) | ((uint64_t)hp << LP_HOP_SHIFT) | ((uint64_t)im << LP_IM_SHIFT) | i;
            wrec[ri] = rv;
          }
        }
        ecnt += (uint32_t)__popcll(wm);
      }
#undef LP_EMIT_PUB
