// lab3 classifier, the f16 distance GEMM (MFMA16): the looped kernel, the
// one-shot production kernel, and the fix-up kernel of its device deferral list.
#pragma once

#include "classify_rank.hpp"

namespace mpx {
namespace {

// ---------------------------------------------------------------------------
// MFMA16 (round 6, VERDICT r5 Next #1): the distance GEMM on
// v_mfma_f32_32x32x16_f16 with ONE pixel per lane and all of its classes in
// that lane's accumulator registers.
//
// Why f16 and not int8: an int8 GEMM needs the 16-bit weights in two limbs at
// two fixed-point scales, so every (pixel, class) key costs two shift-adds
// (D_a << 13, D_b << 5 and the tag) before the top-2 — and its common scale
// leaves small weights few bits, so 1.2 % of the pixels fell inside the
// margin at 32 classes. In f16 each limb carries its own exponent: the weight
// is hi + lo (two f16, ~22 bits), the products with the exact integer
// features are exact in the fp32 accumulator, and the accumulator IS the
// distance: one v_and_or per key puts the class tag in its low mantissa bits
// (the FAST32 key), and the top-2 takes 2.5 VALU per PAIR of keys:
//     t = med3(B, k0, k1); B = min3(B, k0, k1); S = min(S, t)
// (second-smallest of {B, S, k0, k1} = min(S, med3(B, k0, k1)), and the S
// updates of two pairs fuse into one v_min3).
//
// One pixel per lane on a 32x32 tile: the D rows of lane half h are rows
// (r & 3) + 8 (r >> 2) + 4 h, i.e. register r of either half is class r of
// the 16-class set. Lane l supplies B[k = 8 h + j][col = l & 31] = feature j
// of ITS OWN pixel, and the A rows of half h are non-zero only in k-block h
// (A[i][8 kb + j] = w[class(i)][j] when (i >> 2) & 1 == kb, else 0), so the
// rows a lane reads sum its own pixel's features only: 64 pixels x 16 classes
// per MFMA triple, no cross-lane merge, no duplicated feature bytes.
//
// Features (all exact in f16; q = channel - 128 from the byte via the 0x64xx
// magic: f16 0x64nn = 1024 + nn, minus 1152): the six products P = q_i q_j
// as h = f16(P) (|h| <= 16384) and l = P - h (|l| <= 4, one v_pk_fma), and
// the three channels. 24 slots in three K = 8 fragments:
//     B1 = [h(rr gg bb rb rg bg), r, g]  x hi limbs, then the same B1 x lo limbs
//     B3 = [l(rr gg bb rb rg bg), b, b]  x hi limbs (hi and lo of b)
// The class constant (+ a positivity bias) is the fp32 accumulator input.
// build_half bounds |computed - reference chain| per class (limb rounding,
// fp32 accumulation as any 25-term sum, the reference chain's own error), and
// a pixel is decided by the FAST32 test against T2 = 2 max_c tol_c; the rest
// take the fp32 then the fp64 stage (per-wave lists, as MFMA8S).
// ---------------------------------------------------------------------------
typedef _Float16 h2_t __attribute__((ext_vector_type(2)));
typedef _Float16 h8_t __attribute__((ext_vector_type(8)));

template <int NSET>
struct Mfma16Lane {
    h8_t a[NSET][kHalfMfmas];  // A fragments (zero where the row's half is not the lane's k-block)
    f32x16 cinit[NSET];
};

template <int NSET>
__device__ __forceinline__ Mfma16Lane<NSET> mfma16_lane(const HalfParams &hp, int lane) {
    Mfma16Lane<NSET> L;
    const int i = lane & 31;                                 // this lane's A row
    const bool mine = ((i >> 2) & 1) == (lane >> 5);         // row i is read by lane half (lane >> 5)
    const int cls = (i & 3) + 4 * (i >> 3);                  // class (within the set) of D row i
#pragma unroll
    for (int s = 0; s < NSET; ++s) {
#pragma unroll
        for (int j = 0; j < kHalfMfmas; ++j) {
            const uint4 u = mine ? make_uint4(hp.w[s][j][cls][0], hp.w[s][j][cls][1], hp.w[s][j][cls][2],
                                              hp.w[s][j][cls][3])
                                 : make_uint4(0, 0, 0, 0);
            L.a[s][j] = __builtin_bit_cast(h8_t, u);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) L.cinit[s][r] = hp.c[16 * s + r];
    }
    return L;
}

__device__ __forceinline__ uint32_t h2_bits(h2_t v) { return __builtin_bit_cast(uint32_t, v); }

// the three K = 8 feature fragments of pixel p (layout in the header above)
__device__ __forceinline__ void mfma16_features(uint32_t p, h8_t &B1, h8_t &B3) {
    const h2_t off = {(_Float16)-1152.0f, (_Float16)-1152.0f};
    const h2_t R1 = __builtin_bit_cast(h2_t, __builtin_amdgcn_perm(0x64646464u, p, 0x04010400u)) + off;  // {r, g}
    const h2_t R2 = __builtin_bit_cast(h2_t, __builtin_amdgcn_perm(0x64646464u, p, 0x04000402u)) + off;  // {b, r}
    const uint32_t R3 = __builtin_amdgcn_perm(0u, h2_bits(R2), 0x01000100u);                                // {b, b}
    const h2_t R2x = {R2.x, R2.x}, R2s = {R2.y, R2.x}, R1y = {R1.y, R1.y};
    const h2_t H0 = R1 * R1;    // {rr, gg}
    const h2_t H1 = R2 * R2x;   // {bb, rb}
    const h2_t H2 = R2s * R1y;  // {rg, bg}
    const h2_t L0 = __builtin_elementwise_fma(R1, R1, -H0);
    const h2_t L1 = __builtin_elementwise_fma(R2, R2x, -H1);
    const h2_t L2 = __builtin_elementwise_fma(R2s, R1y, -H2);
    B1 = __builtin_bit_cast(h8_t, make_uint4(h2_bits(H0), h2_bits(H1), h2_bits(H2), h2_bits(R1)));
    B3 = __builtin_bit_cast(h8_t, make_uint4(h2_bits(L0), h2_bits(L1), h2_bits(L2), R3));
}

// min3 of keys (VALU results, never MFMA registers: no hazard hidden from the
// compiler). Written in C the backend CSEs min(k0, k1) with the med3 below and
// emits two v_min instead of one v_min3.
__device__ __forceinline__ uint32_t umin3(uint32_t a, uint32_t b, uint32_t c) {
    uint32_t r;
    asm("v_min3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

// rank one pixel: provisional output and whether its top-2 margin is within T2
template <int NSET, int NR>
__device__ __forceinline__ uint32_t mfma16_pixel(uint32_t p, const Mfma16Lane<NSET> &L, float T2, bool &undecided) {
    h8_t B1, B3;
    mfma16_features(p, B1, B3);
    f32x16 acc[NSET];
#pragma unroll
    for (int s = 0; s < NSET; ++s) {
        acc[s] = __builtin_amdgcn_mfma_f32_32x32x16_f16(L.a[s][0], B1, L.cinit[s], 0, 0, 0);
        acc[s] = __builtin_amdgcn_mfma_f32_32x32x16_f16(L.a[s][1], B1, acc[s], 0, 0, 0);
        acc[s] = __builtin_amdgcn_mfma_f32_32x32x16_f16(L.a[s][2], B3, acc[s], 0, 0, 0);
    }
    uint32_t B = 0, S = 0;
#pragma unroll
    for (int s = 0; s < NSET; ++s) {
        constexpr int kLast = NR;
        const int nr = s == NSET - 1 ? kLast : 16;
        uint32_t k[16];
#pragma unroll
        for (int r = 0; r < 16; ++r)
            if (r < nr) k[r] = (__float_as_uint(acc[s][r]) & ~31u) | (uint32_t)(16 * s + r);
        int r0 = 0;
        if (s == 0) {
            B = min(k[0], k[1]);
            S = max(k[0], k[1]);
            r0 = 2;
        }
#pragma unroll
        for (int r = r0; r < 16; r += 2) {
            if (r < nr) {
                const uint32_t a = k[r], b = k[r + 1];
                const uint32_t t = max(min(a, b), min(max(a, b), B));  // v_med3_u32
                B = umin3(B, a, b);
                S = min(S, t);
            }
        }
    }
    undecided = !decided(B, S, T2);
    return __builtin_amdgcn_perm(B & 31u, p, 0x04020100u);
}

// Undecided pixels of a whole one-shot launch: each wave appends its LDS list
// of (vector << 4 | pixel mask) entries to one device list (one atomic per
// wave) and classify_fixup_kernel re-ranks them all afterwards, every lane
// busy. At 0.05-0.1 % undecided a wave holds ~1-4 entries, and re-ranking
// them inside the wave ran the fp32 stage (~15 VALU x nc per pixel slot) once
// per wave for a handful of lanes: ~25 % of the kernel's VALU at 32 classes
// (round-6 counters, profiles/lab3_classify.md).
// The list is split into kDeferSubs sub-lists (sub-list = workgroup id mod
// kDeferSubs, each with its own counter): one counter for the whole launch
// serialised ~16K same-address atomics in the L2 (+30-50 µs at 4-16
// classes, round 6). Fix-up block b owns sub-list b: it reads its count,
// re-ranks the entries and zeroes the count for the next launch.
constexpr uint32_t kDeferSubs = 256;
struct DeferList {
    uint64_t *ent;  // kDeferSubs x cap entries; nullptr: no device list (the looped kernel takes the whole image)
    uint32_t *ctr;  // 2 x kDeferSubs counters, used by calls of alternating parity
    uint32_t cap;   // entries per sub-list
    uint32_t par;   // this call's parity: the fix-up zeroes the other parity's counters for the next call
};

// grid = kDeferSubs blocks: block b re-ranks sub-list b in chunks of
// kFixChunk entries, each in three block-wide phases with every lane busy:
// expand the entries' undecided pixels into an LDS list, rank them with the
// fp32 proven margin, and run the exact fp64 chain on the compacted rest.
// (One thread per entry ran the fp32 and fp64 chains with a third of the
// lanes active and the fp64 chain in nearly every wave: 25-47 µs for ~50K
// entries, round 6.) The block also zeroes the other parity's counter, which
// the next call appends to.
constexpr int kFixChunk = 1024;

// the exact chain alone (the one-shot kernel's rare list-overflow path: the
// fp32 stage's registers would raise the whole kernel's VGPR count)
__device__ __forceinline__ uint32_t fix_entry_direct(uint32_t *img, uint64_t e, int nc, const ClassParams &cp) {
    const int64_t vi = (int64_t)(e >> 4);
    const uint32_t mask = (uint32_t)e & 15u;
    for (int m = 0; m < 4; ++m)
        if ((mask >> m) & 1u) img[vi * 4 + m] = classify_direct(img[vi * 4 + m], nc, cp);
    return (uint32_t)__popc(mask);
}

__global__ __launch_bounds__(256) void classify_fixup_kernel(uint32_t *__restrict__ img, DeferList dl, int nc,
                                                             ClassParams cp, FastParams fp, uint32_t *amb) {
    __shared__ int64_t s_px[4 * kFixChunk];   // pixel indices of one chunk's undecided pixels
    __shared__ int64_t s_px2[4 * kFixChunk];  // those the fp32 stage leaves to the fp64 chain
    __shared__ uint32_t s_n, s_n2, s_tot;
    const uint32_t sub = blockIdx.x;
    const uint32_t n = min(dl.ctr[dl.par * kDeferSubs + sub], dl.cap);
    const uint64_t *ent = dl.ent + (size_t)sub * dl.cap;
    if (threadIdx.x == 0) s_tot = 0;
    for (uint32_t c0 = 0; c0 < n; c0 += kFixChunk) {
        const uint32_t cn = min(n - c0, (uint32_t)kFixChunk);
        if (threadIdx.x == 0) s_n = s_n2 = 0;
        __syncthreads();
        for (uint32_t j = threadIdx.x; j < 4 * cn; j += 256) {  // expand
            const uint64_t e = ent[c0 + (j >> 2)];
            const uint32_t m = j & 3;
            if ((e >> m) & 1u) s_px[atomicAdd(&s_n, 1u)] = (int64_t)(e >> 4) * 4 + m;
        }
        __syncthreads();
        const uint32_t np = s_n;
        for (uint32_t k = threadIdx.x; k < np; k += 256) {  // fp32 stage
            const int64_t idx = s_px[k];
            uint32_t o;
            if (classify_fp32_one(img[idx], nc, fp, o))
                img[idx] = o;
            else
                s_px2[atomicAdd(&s_n2, 1u)] = idx;
        }
        __syncthreads();
        const uint32_t n2 = s_n2;
        for (uint32_t k = threadIdx.x; k < n2; k += 256) {  // the exact chain, compacted
            const int64_t idx = s_px2[k];
            img[idx] = classify_direct(img[idx], nc, cp);
        }
        if (threadIdx.x == 0) s_tot += np;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (amb && s_tot) atomicAdd(amb, s_tot);
        dl.ctr[(dl.par ^ 1u) * kDeferSubs + sub] = 0;
    }
}

// The MFMA8S loop skeleton (one pixel per lane, four per 16-B vector, one
// trip of loads ahead, per-wave deferral lists without block barriers): the
// remainder of an image past classify_mfma16t_kernel's whole blocks, and the
// whole image under a caller grid or when no device list could be allocated.
template <int NSET, int NR>
__global__ __launch_bounds__(256) void classify_mfma16_kernel(uint32_t *__restrict__ img, int64_t nvec, int nc,
                                                              ClassParams cp, HalfParams hp, FastParams fp,
                                                              uint32_t *amb) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const Mfma16Lane<NSET> L = mfma16_lane<NSET>(hp, lane);
    const float T2 = hp.T2;
    __shared__ int64_t s_amb[4][kAmb8sCapW];  // vector index << 4 | undecided-pixel mask
    __shared__ uint32_t s_namb[4], s_npx[4];
    __shared__ int64_t s_amb2[4][kAmb8sCap2W];
    __shared__ uint32_t s_ambpx2[4][kAmb8sCap2W];
    __shared__ uint32_t s_namb2[4];
    if (lane == 0) s_namb[w] = s_npx[w] = s_namb2[w] = 0;
    __builtin_amdgcn_wave_barrier();
    uint4 *v = reinterpret_cast<uint4 *>(img);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint4 qn = i < nvec ? v[i] : uint4{};
    // A wave walks the loop with all of its lanes (i - lane is the wave's first
    // vector): the MFMA reads the B fragments of all 64 lanes, and although a
    // lane's rows carry zero weights for the other half's k-block, 0 x a stale
    // f16 NaN / Inf pattern in a lane that left the loop is NaN, which made
    // every pixel of a partial last wave undecided (exact, but through the
    // fallback). Lanes past the end rank a finite pixel and store nothing.
    for (; i - lane < nvec; i += stride) {
        const bool in = i < nvec;
        const uint4 q = qn;
        if (i + stride < nvec) qn = v[i + stride];
        const uint32_t px[4] = {q.x, q.y, q.z, q.w};
        uint32_t o[4];
        bool u[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) o[m] = mfma16_pixel<NSET, NR>(px[m], L, T2, u[m]);
        if (__builtin_expect(in & (u[0] | u[1] | u[2] | u[3]), 0)) {
            const uint32_t mask = (uint32_t)u[0] | ((uint32_t)u[1] << 1) | ((uint32_t)u[2] << 2) | ((uint32_t)u[3] << 3);
            const uint32_t slot = atomicAdd(&s_namb[w], 1u);
            if (slot < (uint32_t)kAmb8sCapW) {
                s_amb[w][slot] = (i << 4) | mask;
            } else {  // list full: the exact chain inline
#pragma unroll
                for (int m = 0; m < 4; ++m)
                    if ((mask >> m) & 1u) o[m] = classify_direct(px[m], nc, cp);
            }
        }
        if (in) v[i] = make_uint4(o[0], o[1], o[2], o[3]);
    }
    // the empty asm keeps the re-ranking's LDS row addresses and lane-0 mask
    // from being computed before the loop and held in registers across it
    // (NSET 1, NR 4: 81 instead of 79 VGPRs, 5 instead of 6 waves per SIMD)
    int we = w, le = lane;
    asm volatile("" : "+v"(we), "+v"(le));
    rerank_wave_list(img, le, we, s_amb, s_namb, s_npx, s_amb2, s_ambpx2, s_namb2, nc, cp, fp, amb);
}

// The production form: every thread takes exactly T 16-B vectors (T x 256
// per block, no loop, no bounds checks: the launch covers whole blocks and
// the host sends the remainder to the looped kernel above), all T loads
// issued before the first pixel is ranked. Straight-line code is the one
// shape for which the compiler's s_waitcnt placement is exact: in a loop it
// waited vmcnt(0) at the loop head (the previous trip's store) and before
// every store (its own prefetch), whatever the buffering (round 6 probes).
// A wave's undecided pixels (<= 64 T entries: its LDS list never fills) go
// to the launch's device list and classify_fixup_kernel.
constexpr int kM16Trips = 4;

template <int NSET, int NR>
__global__ __launch_bounds__(256) void classify_mfma16t_kernel(
    uint32_t *__restrict__ img, int nc, ClassParams cp, HalfParams hp, FastParams fp, DeferList dl, uint32_t *amb) {
    constexpr int T = kM16Trips;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __shared__ int64_t s_amb[4][64 * T];  // vector index << 4 | undecided-pixel mask
    __shared__ uint32_t s_namb[4];
    if (lane == 0) s_namb[w] = 0;
    const Mfma16Lane<NSET> L = mfma16_lane<NSET>(hp, lane);  // its loads first: trip 0 waits for them alone
    const float T2 = hp.T2;
    uint4 *v = reinterpret_cast<uint4 *>(img);
    const int64_t base = (int64_t)blockIdx.x * (256 * T) + threadIdx.x;
    uint4 q[T];
#pragma unroll
    for (int t = 0; t < T; ++t) q[t] = v[base + 256 * t];
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int t = 0; t < T; ++t) {
        const int64_t vi = base + 256 * t;
        const uint32_t px[4] = {q[t].x, q[t].y, q[t].z, q[t].w};
        uint32_t o[4];
        bool u[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) o[m] = mfma16_pixel<NSET, NR>(px[m], L, T2, u[m]);
        if (__builtin_expect(u[0] | u[1] | u[2] | u[3], 0)) {
            const uint32_t mask = (uint32_t)u[0] | ((uint32_t)u[1] << 1) | ((uint32_t)u[2] << 2) | ((uint32_t)u[3] << 3);
            s_amb[w][atomicAdd(&s_namb[w], 1u)] = (vi << 4) | mask;  // at most one entry per lane and trip
        }
        v[vi] = make_uint4(o[0], o[1], o[2], o[3]);
        __builtin_amdgcn_sched_barrier(0);  // one trip's registers at a time
    }
    __builtin_amdgcn_wave_barrier();
    const uint32_t nd = s_namb[w];
    if (nd == 0) return;
    const uint32_t sub = blockIdx.x % kDeferSubs;
    uint32_t b0 = 0;
    if (lane == 0) b0 = atomicAdd(&dl.ctr[dl.par * kDeferSubs + sub], nd);
    b0 = __shfl(b0, 0);
    uint64_t *ent = dl.ent + (size_t)sub * dl.cap;
    uint32_t over = 0;
    for (uint32_t j = lane; j < nd; j += 64) {
        const uint64_t e = (uint64_t)s_amb[w][j];
        if (b0 + j < dl.cap)
            ent[b0 + j] = e;
        else
            over += fix_entry_direct(img, e, nc, cp);  // list full: this lane re-ranks it (never at benchmark rates)
    }
    if (amb && over) atomicAdd(amb, over);
}

}  // namespace
}  // namespace mpx
