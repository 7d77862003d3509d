// Key-value radix scatter (mpx_sort_pairs_ws; the dispatcher is in sort.hip).
// A sibling of radix_scatter_lean_kernel (sort_radix.hpp) that carries one
// opaque 32-bit payload word per key: the same four 8-bit LSD passes, the same
// count and scan kernels (digit counts do not depend on the payload), the same
// ranking forms — returning LDS adds with two hot-digit slots (RANK 4,
// variants 20 / 21 / 22) and the peer-mask table (RANK 0, variants 7 / 8) —
// and the same slice-major, lane-minor rank order, so every pass is stable.
// A key ranked to tile-local position p is staged with its payload
// (s_keys[p], s_vals[p]); the write-out reads both at i and stores both at
// gbase[digit] + i. The keys-only kernel is left as it is (its register and
// LDS figures are the tuned ones); this one has its own budget:
//   * LDS: two staging arrays. 4096 / 8192 / 16384-key tiles with the
//     returning-add ranking hold 37 / 73 / 145 KiB per block (4 / 2 / 1
//     blocks per CU, as keys-only). The peer-mask fallback adds 2 KiB of
//     tables per wave: 45 / 89 KiB, so 3 / 1 blocks per CU.
//   * registers: the keys-only kernel keeps three 16-key sets in flight under
//     128 VGPRs; a payload set beside them spills (12 - 44 B per lane in the
//     compiler's report). Here the keys prefetch ONE tile ahead (two key sets)
//     and the payload has one set: a tile's payload loads are issued when its
//     ranking starts, before the prefetch of the next tile's keys, so waiting
//     for them does not wait for that prefetch; they are first needed at the
//     staging step, behind the ranking and the digit scan. The per-wave
//     offsets are read again after the scan instead of held across it. Zero
//     scratch in every instantiation (profiles/lab5_sort.md has the table).
//     In iota mode (argsort) pass 0 has no payload loads at all: the value
//     is the key's index, computed at the staging step.
//   * descending order: pass 0 complements the order-preserving key, pass 3
//     complements it back before the inverse transform. The count kernel
//     counts the digits of the uncomplemented key, and the complement maps
//     digit d to 255 - d in every pass, so pass 0 reads the count rows
//     mirrored (offs / tot row 255 - d) instead of counting again.
#pragma once

#include "sort_radix.hpp"

namespace mpx {
namespace {

// waves per SIMD the LDS leaves room for: 4 with the returning-add ranking at
// every tile size; the peer-mask tables leave 3 blocks of 4 waves (4096-key
// tiles) or 1 block of 8 (8192-key tiles) per CU
constexpr int pairs_wpe(int tpb, int rank) { return rank != 0 ? 4 : tpb == 256 ? 3 : 2; }

template <int IN_MODE, int OUT_MODE, bool IOTA, int TPB, int RANK>
__global__ __launch_bounds__(TPB) __attribute__((amdgpu_waves_per_eu(pairs_wpe(TPB, RANK)))) void radix_scatter_pairs_kernel(
    const uint32_t *__restrict__ kin, uint32_t *__restrict__ kout, const uint32_t *__restrict__ vin,
    uint32_t *__restrict__ vout, int64_t n, int shift, uint32_t flip, const uint32_t *__restrict__ tot,
    const uint32_t *__restrict__ offs, int ntiles) {
    static_assert(RANK == 0 || RANK == 4, "pairs: the peer-mask and the hot-digit returning-add rankings");
    static_assert(!IOTA || IN_MODE != kRawKeys, "the payload is generated in pass 0 only");
    constexpr int NW = TPB / 64, TILE = TPB * kRPer;  // kRWaveKeys keys per wave
    __shared__ uint32_t s_keys[TILE];  // staging
    __shared__ uint32_t s_vals[TILE];
    // per-wave peer-mask tables (RANK 0): every slice clears the words it set
    __shared__ uint32_t s_tbl[RANK == 0 ? NW * 512 : 1];
    __shared__ uint32_t s_cnt[NW][256];  // digit counters, one row per wave
    __shared__ uint32_t s_gbase[256];
    __shared__ uint32_t s_wsum[4];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    if constexpr (RANK == 0)
        for (int i = t; i < NW * 512; i += TPB) s_tbl[i] = 0;
    for (int i = t; i < NW * 256; i += TPB) (&s_cnt[0][0])[i] = 0;
    const int xcd = blockIdx.x % kNumXCDs, per = gridDim.x / kNumXCDs;  // gridDim.x: a multiple of 8
    const int t1 = (int)((int64_t)ntiles * (xcd + 1) / kNumXCDs);
    const int t0 = (int)((int64_t)ntiles * xcd / kNumXCDs);
    int tile = t0 + (int)blockIdx.x / kNumXCDs;
    if (tile >= t1) return;  // block-uniform
    const uint32_t n32 = (uint32_t)n;   // n < 2^30
    const int nbytes = (int)(n32 * 4u);  // the byte bound fits the descriptor's 32 bits
    const __amdgpu_buffer_rsrc_t rkin = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t *>(kin), 0, nbytes,
                                                                          0x00020000);
    const __amdgpu_buffer_rsrc_t rvin = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t *>(IOTA ? kin : vin), 0,
                                                                          nbytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rkout = __builtin_amdgcn_make_buffer_rsrc(kout, 0, nbytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rvout = __builtin_amdgcn_make_buffer_rsrc(vout, 0, nbytes, 0x00020000);
    const int wlane = w * kRWaveKeys + lane;  // slice e of this lane is tile key wlane + 64 e
    uint32_t *tbl = s_tbl + (RANK == 0 ? w * 512 : 0);
    uint32_t *const myword = tbl + (lane >> 5);
    const uint32_t mybit = 1u << (lane & 31);
    // descending pass 0: the complemented key's digit d was counted as 255 - d
    const bool mirror = IN_MODE != kRawKeys && flip != 0u;  // grid-uniform
    const int row = mirror ? 255 - t : t;
    const uint32_t mytot = t < 256 ? tot[row] : 0u;
    const uint32_t dbase = scan256_excl_lds(mytot, s_wsum);  // + the barrier after the zeroing
    // the pass's hot digits: as in radix_scatter_lean_kernel (RANK 4)
    constexpr bool HOT = RANK == 4;
    constexpr int HN = 2;
    int nh = 0;
    uint32_t hd[HN] = {};
    if constexpr (HOT) {
        __shared__ uint32_t s_hotc[4], s_cd[kHotShare], s_cc[kHotShare], s_hd[HN];
        const bool hot = t < 256 && (uint64_t)mytot * kHotShare >= (uint64_t)n;
        const uint64_t hm = __builtin_amdgcn_ballot_w64(hot);
        if (t < 256 && lane == 0) s_hotc[w] = (uint32_t)__popcll(hm);
        lds_barrier();
        uint32_t pos = lanes_below(hm), all = 0;
#pragma unroll
        for (int ww = 0; ww < 4; ++ww) {
            const uint32_t c = s_hotc[ww];
            pos += ww < w ? c : 0u;
            all += c;
        }
        if (hot) {  // pos < kHotShare: the candidates hold more than all keys otherwise
            s_cd[pos] = (uint32_t)t;
            s_cc[pos] = mytot;
        }
        lds_barrier();
        if (hot) {
            uint32_t order = 0;
            for (uint32_t c = 0; c < all; ++c)
                order += s_cc[c] > mytot || (s_cc[c] == mytot && s_cd[c] < (uint32_t)t);
            if (order < (uint32_t)HN) s_hd[order] = (uint32_t)t;
        }
        lds_barrier();
        nh = (int)__builtin_amdgcn_readfirstlane(all < (uint32_t)HN ? all : (uint32_t)HN);
#pragma unroll
        for (int j = 0; j < HN; ++j) hd[j] = j < nh ? __builtin_amdgcn_readfirstlane(s_hd[j]) : 256u;
    }

    // whole tiles: one offset register, slices in the immediate field; the
    // partial last tile (block-uniform) loads and stores under explicit index
    // checks, so correctness never rests on the descriptor's range check
    auto load_words = [&](const __amdgpu_buffer_rsrc_t &rs, uint32_t (&dst)[kRPer], int tl) {
        const int64_t tile0 = (int64_t)tl * TILE;
        if (tile0 + TILE <= n) {
            const uint32_t voff = ((uint32_t)tile0 + (uint32_t)wlane) * 4u;  // < n * 4 < 2^32
#pragma unroll
            for (int e = 0; e < kRPer; ++e)  // non-temporal: read once
                dst[e] = __builtin_amdgcn_raw_buffer_load_b32(rs, (int)(voff + e * 256u), 0, 2);
        } else {
            const uint32_t i0 = (uint32_t)tile0 + (uint32_t)wlane;
#pragma unroll
            for (int e = 0; e < kRPer; ++e) {
                const uint32_t i = i0 + e * 64u;
                dst[e] = i < n32 ? __builtin_amdgcn_raw_buffer_load_b32(rs, (int)(i * 4u), 0, 0) : 0u;
            }
        }
    };
    auto load_tile = [&](uint32_t (&dst)[kRPer], int tl) { load_words(rkin, dst, tl); };
    auto load_vals = [&](uint32_t (&dst)[kRPer], int tl) {
        if constexpr (!IOTA) load_words(rvin, dst, tl);
    };
    // HOTP: a separate instance of the tile loop for a pass with hot digits
    auto do_tile = [&](uint32_t (&key)[kRPer], uint32_t (&val)[kRPer], int ptile, auto hotp) {
        constexpr bool HOTP = decltype(hotp)::value;
        // s_cnt and the tables are zero here (kernel start / previous write-out)
        const uint32_t excl = t < 256 ? offs[(size_t)row * ntiles + ptile] : 0u;
        const int64_t tile0 = (int64_t)ptile * TILE;
        const bool full = tile0 + TILE <= n;  // block-uniform
#pragma unroll
        for (int e = 0; e < kRPer; ++e) {
            key[e] = to_key_t<IN_MODE>(key[e]);
            if constexpr (IN_MODE != kRawKeys) key[e] ^= flip;
        }
        if (!full) {  // pads rank last (digit 255 in every pass) and are never stored
            const uint32_t i0 = (uint32_t)tile0 + (uint32_t)wlane;
#pragma unroll
            for (int e = 0; e < kRPer; ++e)
                if (i0 + e * 64u >= n32) key[e] = 0xffffffffu;
        }
        uint32_t rank[kRPer];
        if constexpr (HOTP) {
            uint32_t hc[HN] = {};  // wave-uniform counts of the hot digits
#pragma unroll
            for (int e = 0; e < kRPer; ++e) {
                const uint32_t d = (key[e] >> shift) & 255u;
                uint32_t r = 0;
                bool hit = false;
#pragma unroll
                for (int j = 0; j < HN; ++j) {
                    const bool is = d == hd[j];
                    const uint64_t m = __builtin_amdgcn_uicmp(d, hd[j], 32);  // ICMP_EQ: the compare's lane mask
                    const uint32_t rj =
                        __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, hc[j]));
                    r = is ? rj : r;
                    hc[j] += (uint32_t)__popcll(m);
                    hit = hit || is;
                }
                if (!hit) r = atomicAdd(&s_cnt[w][d], 1u);
                rank[e] = r;
            }
            // no returning add touched a hot digit's counter
            if (lane == 0) {
                const int wrow = __builtin_amdgcn_readfirstlane(w);
#pragma unroll
                for (int j = 0; j < HN; ++j)
                    if (j < nh) s_cnt[wrow][hd[j]] = hc[j];
            }
        } else if constexpr (RANK == 4) {
#pragma unroll
            for (int e = 0; e < kRPer; ++e) rank[e] = atomicAdd(&s_cnt[w][(key[e] >> shift) & 255u], 1u);
        } else {
#pragma unroll
            for (int g = 0; g < kRPer; g += 4) {  // 4 slices in flight: bounds the live LDS results
                uint32_t lo[4], hi[4], before[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const uint32_t d = (key[g + e] >> shift) & 255u;
                    atomicOr(myword + 2 * d, mybit);
                    lo[e] = tbl[2 * d];
                    hi[e] = tbl[2 * d + 1];
                    myword[2 * d] = 0;
                    before[e] = s_cnt[w][d];
                    // one add per distinct digit (its lowest lane)
                    const uint64_t m = ((uint64_t)hi[e] << 32) | lo[e];
                    if (lanes_below(m) == 0) atomicAdd(&s_cnt[w][d], (uint32_t)__popcll(m));
                }
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    rank[g + e] = before[e] + __builtin_amdgcn_mbcnt_hi(hi[e], __builtin_amdgcn_mbcnt_lo(lo[e], 0u));
            }
        }
        lds_barrier();
        uint32_t cnt = 0;
        if (t < 256) {
#pragma unroll
            for (int ww = 0; ww < NW; ++ww) cnt += s_cnt[ww][t];
        }
        const uint32_t dstart = scan256_excl_dpp(cnt, s_wsum);
        if (t < 256) {
            // the rows are read again instead of kept across the scan: NW
            // registers less where the keys, ranks, payload and prefetch are live
            uint32_t run = dstart;
#pragma unroll
            for (int ww = 0; ww < NW; ++ww) {
                const uint32_t c = s_cnt[ww][t];
                s_cnt[ww][t] = run;
                run += c;
            }
            s_gbase[t] = excl + dbase - dstart;
        }
        lds_barrier();
#pragma unroll
        for (int e = 0; e < kRPer; ++e) {
            const uint32_t p = s_cnt[w][(key[e] >> shift) & 255u] + rank[e];  // < TILE
            s_keys[p] = key[e];
            // iota: the key's index in the caller's array (< n < 2^30; a pad's is never stored)
            s_vals[p] = IOTA ? (uint32_t)tile0 + (uint32_t)wlane + e * 64u : val[e];
        }
        lds_barrier();
        // this wave's staging reads of its own row are done (program order)
#pragma unroll
        for (int i = lane; i < 256; i += 64) s_cnt[w][i] = 0;
        if (full) {
#pragma unroll
            for (int j = 0; j < TILE / TPB; ++j) {
                const int i = t + j * TPB;
                uint32_t k = s_keys[i];
                const uint32_t v = s_vals[i];
                const int off = (int)((s_gbase[(k >> shift) & 255u] + (uint32_t)i) * 4u);
                if constexpr (OUT_MODE != kRawKeys) k ^= flip;
                __builtin_amdgcn_raw_buffer_store_b32(from_key_t<OUT_MODE>(k), rkout, off, 0, 0);
                __builtin_amdgcn_raw_buffer_store_b32(v, rvout, off, 0, 0);
            }
        } else {
            for (int j = 0; j < TILE / TPB; ++j) {
                const int i = t + j * TPB;
                uint32_t k = s_keys[i];
                const uint32_t v = s_vals[i];
                const uint32_t pos = s_gbase[(k >> shift) & 255u] + (uint32_t)i;  // < n + TILE < 2^31
                if constexpr (OUT_MODE != kRawKeys) k ^= flip;
                if (pos < n32) {
                    __builtin_amdgcn_raw_buffer_store_b32(from_key_t<OUT_MODE>(k), rkout, (int)(pos * 4u), 0, 0);
                    __builtin_amdgcn_raw_buffer_store_b32(v, rvout, (int)(pos * 4u), 0, 0);
                }
            }
        }
    };

    auto run_tiles = [&](auto hotp) {
        uint32_t v[kRPer] = {};  // the one payload set: the tile being ranked
        uint32_t a[kRPer], b[kRPer];
        load_tile(a, tile);
        for (; tile < t1; tile += per) {
            load_vals(v, tile);
            if (tile + per < t1) load_tile(b, tile + per);  // in flight under this tile's work
            do_tile(a, v, tile, hotp);
#pragma unroll
            for (int e = 0; e < kRPer; ++e) a[e] = b[e];
        }
    };
    if constexpr (HOT) {
        if (nh > 0)  // block-uniform
            run_tiles(std::true_type{});
        else
            run_tiles(std::false_type{});
    } else {
        run_tiles(std::false_type{});
    }
}

// pass p of the pairs scatter: the first pass reads raw int32 / float32 keys
// (and the caller's payload, or generates the index), the last writes raw
// keys back, the middle passes move (key, payload) words
template <int TPB, int RANK>
void launch_pairs(int p, int mode, bool iota, uint32_t flip, int blocks, hipStream_t s, const uint32_t *ksrc,
                  uint32_t *kdst, const uint32_t *vsrc, uint32_t *vdst, int64_t n, const uint32_t *tot,
                  const uint32_t *offs, int ntiles) {
    const dim3 g((unsigned)blocks), b(TPB);
    const int sh = 8 * p;
    const bool f = mode == kRawF32;
#define MPX_PAIRS(I, O, IO)                                                                                          \
    hipLaunchKernelGGL((radix_scatter_pairs_kernel<I, O, IO, TPB, RANK>), g, b, 0, s, ksrc, kdst, vsrc, vdst, n,     \
                       sh, flip, tot, offs, ntiles)
    if (p == 0 && f && iota)
        MPX_PAIRS(kRawF32, kRawKeys, true);
    else if (p == 0 && f)
        MPX_PAIRS(kRawF32, kRawKeys, false);
    else if (p == 0 && iota)
        MPX_PAIRS(kRawI32, kRawKeys, true);
    else if (p == 0)
        MPX_PAIRS(kRawI32, kRawKeys, false);
    else if (p == 3 && f)
        MPX_PAIRS(kRawKeys, kRawF32, false);
    else if (p == 3)
        MPX_PAIRS(kRawKeys, kRawI32, false);
    else
        MPX_PAIRS(kRawKeys, kRawKeys, false);
#undef MPX_PAIRS
}

size_t radix_pairs_ws_bytes(int64_t n) { return radix_ws_bytes(n) + ((size_t)n * 4 + 255) / 256 * 256; }

}  // namespace
}  // namespace mpx
