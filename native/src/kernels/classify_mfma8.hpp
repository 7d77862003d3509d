// lab3 classifier, the exact int8 distance GEMMs: MFMA8 (32x32x16, any class
// count) and MFMA8S (4x4x4, one pixel per lane, up to kMfma8sMaxClasses).
#pragma once

#include <utility>

#include "classify_rank.hpp"

namespace mpx {
namespace {

// ---------------------------------------------------------------------------
// MFMA8: the distance GEMM in exact int8 x int8 -> int32 on
// v_mfma_i32_32x32x16_i8 (BASELINE config 4 "MFMA
// distance-GEMM").
//   Features (K = 16, every one an exact int8): the six centred products
//   P = q_i q_j (|P| <= 2^14) split as P = 256 h + l with h = (P + 128) >> 8 in
//   [-64, 64] (byte 1 of P + 128) and l in [-128, 127] (byte 0 of P), the three
//   centred channels q in [-128, 127], one zero slot; the constant term rides
//   in the MFMA's accumulator input.
//     half-wave 0 (k 0..7):  h(rr gg bb rg rb gb), r, g
//     half-wave 1 (k 8..15): l(rr gg bb rg rb gb), b, 0
//   Weights: the slot weights V (256 w for h slots, w for l and linear slots)
//   as integers v = round(V / u) in 16 bits, split v = 256 a + b over two
//   int8 GEMMs; the class constant round(w9 / u) is the accumulator input of
//   the b GEMM. The int32 key of (pixel, class) is
//       ((D_a << 8) + D_b) << 5 | class     (|.| < 2^31, checked on the host)
//   — exact integer arithmetic, so the only error is the weight rounding,
//   u/2 per unit of |feature|: the host bounds it (plus the reference chain's
//   own error) and a pixel is decided only when its second-best key exceeds
//   the best by more than 2 max_c tol_c / u; every other pixel is deferred to
//   the exact fp64 chain at the end of the block (all lanes busy).
//   A (weights): lane l holds A[class l & 31][k = 8 (l >> 5) .. +7] (loaded once)
//   B (features): lane l holds B[k = 8 (l >> 5) .. +7][pixel l & 31]
//   D: lane l, reg r holds class (r & 3) + 8 (r >> 2) + 4 (l >> 5), pixel l & 31
// Per (pixel, class) the VALU spends 4 instructions (shift-add, shift-or tag,
// med3, min) against fast32's ~9.
// ---------------------------------------------------------------------------
typedef int i32x16 __attribute__((ext_vector_type(16)));

constexpr int kAmb8Cap = 2048;

// The MFMA results are read by compiler-visible instructions only: the
// hazard recognizer does not see inline-asm reads of an MFMA destination and
// would not pad them (a read right after the MFMA sees stale registers). The
// empty asm between the two v_lshl_add_u32 only stops the compiler from
// re-associating them into a shift + or + add chain (5 instead of 4 VALU).
template <int NREG, int RR>
__device__ __forceinline__ void rank_reg(const i32x16 &da, const i32x16 &db, int32_t &B, int32_t &S) {
    if constexpr (RR < NREG) {
        uint32_t x = ((uint32_t)da[RR] << 13) + (uint32_t)((RR & 3) + 8 * (RR >> 2));
        asm volatile("" : "+v"(x));
        const int32_t key = (int32_t)(((uint32_t)db[RR] << 5) + x);
        // med3(B, key, S) in the form the backend selects as v_med3_i32 (an
        // inline-asm med3 may not be ordered after an in-flight MFMA's
        // writeback to a reused dead accumulator register)
        S = max(min(B, key), min(max(B, key), S));
        B = min(B, key);
    }
}

template <int NREG, int... R>
__device__ __forceinline__ void rank_regs(const i32x16 &da, const i32x16 &db, int32_t &B, int32_t &S,
                                          std::integer_sequence<int, R...>) {
    (rank_reg<NREG, R>(da, db, B, S), ...);
}

// Per-wave constants of the mfma8 GEMM (weights, accumulator init, byte
// selectors of the feature packing).
// packed 16-bit channel products (the int8 feature builders)
typedef short s16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t s16x2_bits(s16x2 v) { return __builtin_bit_cast(uint32_t, v); }

struct Mfma8Lane {
    long wa, wb;
    i32x16 cinit;
    int add, h;
    uint32_t sel0, sel1;  // feature dwords from the packed products (mfma8_chunk)
};

__device__ __forceinline__ Mfma8Lane mfma8_lane(const I8Params &ip, int lane) {
    Mfma8Lane L;
    L.h = lane >> 5;
    const int col = lane & 31;
    L.wa = (long)ip.a[col][L.h];
    L.wb = (long)ip.b[col][L.h];
#pragma unroll
    for (int r = 0; r < 16; ++r) L.cinit[r] = ip.c[(r & 3) + 8 * (r >> 2) + 4 * L.h];
    // half 0 packs byte 1 of P + 128 (the h limbs), half 1 byte 0 of P (the l limbs)
    L.add = L.h ? 0 : 128;
    const uint32_t sel = L.h ? 0u : 1u;
    // d0 = byte s of each 16-bit product [rr gg | bb rg]: perm(PB, PA)
    L.sel0 = sel | ((2u + sel) << 8) | ((4u + sel) << 16) | ((6u + sel) << 24);
    // d1 = [rb.s, gb.s, b or r, 0 or g]: perm(PC, centred pixel)
    L.sel1 = (4u + sel) | ((6u + sel) << 8) | ((L.h ? 2u : 0u) << 16) | ((L.h ? 0x0Cu : 1u) << 24);
    return L;
}

// One 128-pixel chunk (the 16 B of pixels 4 col .. +3 in every lane): the
// provisional output (class of the best int32 key in the alpha byte) and a
// mask of the pixels whose top-2 margin is within T2 (valid in half-wave 0).
template <int NREG>
__device__ __forceinline__ uint32_t mfma8_chunk(const uint4 &q, const Mfma8Lane &L, int32_t T2, uint4 &o) {
    const uint32_t px[4] = {q.x, q.y, q.z, q.w};
    int32_t rb[4], rs[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        // the six products as three packed 16-bit multiply-adds of sign-extended
        // channel pairs (mfma8s_features: one v_perm per pair), then one v_perm
        // per feature dword
        const uint32_t x = px[m] ^ 0x80808080u;  // bytes - 128
        const uint32_t y = x << 8;
        auto pair = [&](uint32_t sl) { return __builtin_bit_cast(s16x2, __builtin_amdgcn_perm(y, x, sl)); };
        const s16x2 U = pair(0x08010A00u), V = pair(0x0A000B02u), W = pair(0x08010B02u);  // {r,g} {b,r} {b,g}
        const s16x2 Z = {V.x, V.x};
        const s16x2 ad = {(short)L.add, (short)L.add};
        const uint32_t PA = s16x2_bits(U * U + ad), PB = s16x2_bits(V * W + ad), PC = s16x2_bits(U * Z + ad);
        const uint32_t d0 = __builtin_amdgcn_perm(PB, PA, L.sel0);
        const uint32_t d1 = __builtin_amdgcn_perm(PC, x, L.sel1);
        const long feat = (long)(((uint64_t)d1 << 32) | d0);
        const i32x16 da = __builtin_amdgcn_mfma_i32_32x32x16_i8(L.wa, feat, i32x16{}, 0, 0, 0);
        const i32x16 db = __builtin_amdgcn_mfma_i32_32x32x16_i8(L.wb, feat, L.cinit, 0, 0, 0);
        int32_t B = INT32_MAX, S = INT32_MAX;
        // key = ((da << 8) + db) << 5 | tag as two v_lshl_add_u32:
        // (da << 13) + tag first, then (db << 5) + that
        rank_regs<NREG>(da, db, B, S, std::make_integer_sequence<int, 16>{});
        B |= 4 * L.h;  // row tags (r & 3) + 8 (r >> 2) never set bit 2
        S |= 4 * L.h;
        const auto sb = __builtin_amdgcn_permlane32_swap((uint32_t)B, (uint32_t)B, false, false);
        const auto ss = __builtin_amdgcn_permlane32_swap((uint32_t)S, (uint32_t)S, false, false);
        const int32_t B0 = (int32_t)sb[0], B1 = (int32_t)sb[1], S0 = (int32_t)ss[0], S1 = (int32_t)ss[1];
        rb[m] = min(B0, B1);
        rs[m] = min(max(B0, B1), min(S0, S1));
    }
    uint32_t *op = &o.x;
    uint32_t undecided = 0;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        op[m] = (px[m] & 0x00ffffffu) | (((uint32_t)rb[m] & 31u) << 24);
        // exact integers: the tag bits are below the shift
        if ((rs[m] >> 5) - (rb[m] >> 5) <= T2) undecided |= 1u << m;
    }
    return undecided;
}

// Each chunk is stored as soon as it is ranked and the undecided pixels are
// re-stored one by one after the block's grid-stride loop (partial-line HBM
// writes: 56-71 MiB per 8192^2 image, kernels_r3.md). Ranking a window of
// chunks into LDS and resolving its undecided pixels before one whole store
// wrote every byte once (1.03x the image against 1.22x) but ran 434-444 ->
// 523 µs at nc = 32 (three barriers per window): retired (round 6).
constexpr int kAmb8Cap2 = 256;  // pixels the fp32 stage leaves to the fp64 chain, per block

template <int NREG>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5))) void classify_mfma8_kernel(uint32_t *__restrict__ img, int64_t nchunks, int nc,
                                                             ClassParams cp, I8Params ip, FastParams fp, uint32_t *amb) {
    const int lane = threadIdx.x & 63;
    const int h = lane >> 5;
    const int col = lane & 31;
    const Mfma8Lane L = mfma8_lane(ip, lane);
    uint4 *v = reinterpret_cast<uint4 *>(img);
    const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x >> 6);
    __shared__ int64_t s_amb[kAmb8Cap];
    __shared__ uint32_t s_ambpx[kAmb8Cap];
    __shared__ uint32_t s_namb;
    if (threadIdx.x == 0) s_namb = 0;
    __syncthreads();
    const int64_t wave = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    int64_t ch = wave;
    uint4 qn = ch < nchunks ? v[ch * 32 + col] : uint4{};
    for (; ch < nchunks; ch += nwaves) {
        const uint4 q = qn;
        if (ch + nwaves < nchunks) qn = v[(ch + nwaves) * 32 + col];
        uint4 o;
        const uint32_t und = mfma8_chunk<NREG>(q, L, ip.T2, o);
        if (h == 0) {
            const uint32_t px[4] = {q.x, q.y, q.z, q.w};
            uint32_t *op = &o.x;
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                if (__builtin_expect((und >> m) & 1u, 0)) {
                    const uint32_t slot = atomicAdd(&s_namb, 1u);  // also the block's count
                    if (slot < (uint32_t)kAmb8Cap) {
                        s_amb[slot] = (ch * 32 + col) * 4 + m;
                        s_ambpx[slot] = px[m];
                    } else {
                        op[m] = classify_direct(px[m], nc, cp);
                    }
                }
            }
            v[ch * 32 + col] = o;
        }
    }
    __shared__ int64_t s_amb2[kAmb8Cap2];
    __shared__ uint32_t s_ambpx2[kAmb8Cap2];
    __shared__ uint32_t s_namb2;
    if (threadIdx.x == 0) s_namb2 = 0;
    __syncthreads();
    const uint32_t nd = min(s_namb, (uint32_t)kAmb8Cap);
    if (amb && threadIdx.x == 0 && s_namb) atomicAdd(amb, s_namb);  // one global add per block
    // two stages, every lane busy in each: the fp32 proven-margin ranking
    // settles all but ~1% of the int8 path's undecided pixels (its bound is
    // ~2^-16 of the weights' against the int8 keys' 2^-8 .. 2^-16); the
    // rest take the exact fp64 chain together
    for (uint32_t j = threadIdx.x; j < nd; j += blockDim.x) {
        const uint32_t px = s_ambpx[j];
        uint32_t o;
        if (classify_fp32_one(px, nc, fp, o)) {
            img[s_amb[j]] = o;
        } else {
            const uint32_t slot = atomicAdd(&s_namb2, 1u);
            if (slot < (uint32_t)kAmb8Cap2) {
                s_amb2[slot] = s_amb[j];
                s_ambpx2[slot] = px;
            } else {
                img[s_amb[j]] = classify_direct(px, nc, cp);
            }
        }
    }
    __syncthreads();
    const uint32_t nd2 = min(s_namb2, (uint32_t)kAmb8Cap2);
    for (uint32_t j = threadIdx.x; j < nd2; j += blockDim.x) img[s_amb2[j]] = classify_direct(s_ambpx2[j], nc, cp);
}

// ---------------------------------------------------------------------------
// MFMA8S: the same exact int8 distance GEMM for nc <= 8 classes on
// v_mfma_i32_4x4x4_16b_i8 (16 blocks of 4 x 4 x 4; VERDICT r4 Next #4), one
// pixel per lane.
//   The 32x32 form above gives every pixel to two lanes (the two K halves)
//   and spends 75% of its rows on absent classes below 9 classes: the
//   per-pixel feature bytes are built twice and the ranking merges half-waves.
//   Here the 16-byte feature vector of a pixel is four dwords (K = 4 per
//   instruction, four chained instructions per row set) that ONE lane builds,
//   and every result of the pixel lands in that lane:
//     A (weights): lane l supplies row l & 3 of every block (the blocks share
//                  the weights): row r of row set s = limb r & 1 (0: a, 1: b)
//                  of class 2 s + (r >> 1), slots 4 t .. 4 t + 3 for step t;
//     B (features): lane l supplies column l & 3 of block l >> 2 — its pixel;
//     D: lane l, register r = row r of its own pixel's column.
//   (Layout measured on gfx950 with tools/experiments/mfma4_layout.hip.)
//   Features (build_i8's slots): F0 = h(rr gg bb rg), F1 = h(rb gb) r g,
//   F2 = l(rr gg bb rg), F3 = l(rb gb) b 0, from three v_pk_mad-style 16-bit
//   products P + 128 of the centred channels: h = byte 1 of P + 128, l = byte 0
//   of P = byte 0 of (P + 128) ^ 0x80.
//   Keys as in MFMA8: ((D_a << 8) + D_b) << 5 | class — two v_lshl_add per
//   class — then the running top-2 in the lane; no cross-lane merge.
//   NS = row sets (2 classes each) with real classes: 1 .. 7 up to
//   kMfma8sMaxClasses = 13 classes.
// ---------------------------------------------------------------------------
constexpr int kMfma8sMaxClasses = 13;
typedef int i32x4 __attribute__((ext_vector_type(4)));

template <int NS>
struct Mfma8sLane {
    int w[NS][4];     // [row set][step]: 4 int8 weights of this lane's row
    i32x4 cinit[NS];  // [row set]: {0, c(2s), 0, c(2s + 1)}
};

template <int NS>
__device__ __forceinline__ Mfma8sLane<NS> mfma8s_lane(const I8Params &ip, int lane) {
    Mfma8sLane<NS> L;
    const int r = lane & 3;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int c = 2 * s + (r >> 1);
        const uint64_t *limb = (r & 1) ? ip.b[c] : ip.a[c];
#pragma unroll
        for (int t = 0; t < 4; ++t) L.w[s][t] = (int)(uint32_t)(limb[t >> 1] >> (32 * (t & 1)));
        L.cinit[s] = i32x4{0, ip.c[2 * s], 0, ip.c[2 * s + 1]};
    }
    return L;
}

// the four feature dwords of pixel p (build_i8's slot order)
__device__ __forceinline__ void mfma8s_features(uint32_t p, int (&F)[4]) {
    const uint32_t x = p ^ 0x80808080u;  // centred channels as signed bytes
    // sign-extended 16-bit pairs in one v_perm each: with {x << 8 : x} as the
    // perm's 64-bit source, selectors 8 / 10 / 11 replicate the top bits of
    // bytes 1 / 5 / 7 = the signs of g / r / b (one shift instead of three
    // bit-field extracts)
    const uint32_t y = x << 8;
    auto pair = [&](uint32_t sel) { return __builtin_bit_cast(s16x2, __builtin_amdgcn_perm(y, x, sel)); };
    const s16x2 c128 = {128, 128};
    const s16x2 U = pair(0x08010A00u), V = pair(0x0A000B02u), W = pair(0x08010B02u);
    const s16x2 Z = {V.x, V.x};  // op_sel of V's low half in the packed multiply, no instruction
    // U = {r, g}, V = {b, r}, W = {b, g}, Z = {b, b}
    const uint32_t P01 = s16x2_bits(U * U + c128);  // [rr | gg] + 128
    const uint32_t P23 = s16x2_bits(V * W + c128);  // [bb | rg] + 128
    const uint32_t P45 = s16x2_bits(U * Z + c128);  // [rb | gb] + 128
    F[0] = (int)__builtin_amdgcn_perm(P23, P01, 0x07050301u);                  // h(rr gg bb rg)
    F[1] = (int)__builtin_amdgcn_perm(x, P45, 0x05040301u);                    // h(rb gb), r, g
    F[2] = (int)(__builtin_amdgcn_perm(P23, P01, 0x06040200u) ^ 0x80808080u);  // l(rr gg bb rg)
    F[3] = (int)(__builtin_amdgcn_perm(x, P45, 0x0C060200u) ^ 0x00008080u);    // l(rb gb), b, 0
}

// rank one pixel: provisional output and whether its top-2 margin is within T2
template <int NS>
__device__ __forceinline__ uint32_t mfma8s_pixel(uint32_t p, const Mfma8sLane<NS> &L, int32_t T2k, bool &undecided) {
    int F[4];
    mfma8s_features(p, F);
    i32x4 D[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) D[s] = L.cinit[s];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int s = 0; s < NS; ++s) D[s] = __builtin_amdgcn_mfma_i32_4x4x4i8(L.w[s][t], F[t], D[s], 0, 0, 0);
    int32_t B = INT32_MAX, S = INT32_MAX;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            // v_lshl_or_b32 + v_lshl_add_u32 per class (the empty asm keeps the
            // compiler from re-associating them into shift, shift-add and or;
            // it costs an s_nop 0, a cycle of this wave, not a VALU slot)
            uint32_t x = ((uint32_t)D[s][2 * h + 1] << 5) | (uint32_t)(2 * s + h);
            asm volatile("" : "+v"(x));
            const int32_t key = (int32_t)(((uint32_t)D[s][2 * h] << 13) + x);
            S = max(min(B, key), min(max(B, key), S));
            B = min(B, key);
        }
    }
    // (S >> 5) - (B >> 5) <= T2, tested conservatively on the tagged keys:
    // S - B <= 32 T2 + 31 (T2k) holds whenever the exact test does
    undecided = (uint32_t)(S - B) <= (uint32_t)T2k;
    return __builtin_amdgcn_perm((uint32_t)B & 31u, p, 0x04020100u);
}

// One trip of loads in flight (two measured level, non-temporal loads /
// stores measured neutral or slower: profiles/lab3_classify.md, round 5).
template <int NS>
__global__ __launch_bounds__(256) void classify_mfma8s_kernel(uint32_t *__restrict__ img, int64_t nvec, int nc,
                                                              ClassParams cp, I8Params ip, FastParams fp,
                                                              uint32_t *amb) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const Mfma8sLane<NS> L = mfma8s_lane<NS>(ip, lane);
    const int32_t T2k = ip.T2 * 32 + 31;
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
    auto trip = [&](const uint4 q, int64_t vi) {
        const uint32_t px[4] = {q.x, q.y, q.z, q.w};
        uint32_t o[4];
        bool u[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) o[m] = mfma8s_pixel<NS>(px[m], L, T2k, u[m]);
        // the test on the four compare masks (scalar ORs); the entry's bit mask
        // is built only inside the rare branch
        if (__builtin_expect(u[0] | u[1] | u[2] | u[3], 0)) {
            const uint32_t mask = (uint32_t)u[0] | ((uint32_t)u[1] << 1) | ((uint32_t)u[2] << 2) | ((uint32_t)u[3] << 3);
            const uint32_t slot = atomicAdd(&s_namb[w], 1u);
            if (slot < (uint32_t)kAmb8sCapW) {
                s_amb[w][slot] = (vi << 4) | mask;
            } else {  // list full: the exact chain inline (never at the benchmark's rates)
#pragma unroll
                for (int m = 0; m < 4; ++m)
                    if ((mask >> m) & 1u) o[m] = classify_direct(px[m], nc, cp);
            }
        }
        v[vi] = make_uint4(o[0], o[1], o[2], o[3]);
    };
    uint4 qn = i < nvec ? v[i] : uint4{};
    // a per-lane loop is fine here (unlike classify_mfma16_kernel's): lanes
    // past the end leave stale integer features, and 0 x stale is 0 in int8
    for (; i < nvec; i += stride) {
        const uint4 q = qn;
        if (i + stride < nvec) qn = v[i + stride];
        trip(q, i);
    }
    rerank_wave_list(img, lane, w, s_amb, s_namb, s_npx, s_amb2, s_ambpx2, s_namb2, nc, cp, fp, amb);
}

}  // namespace
}  // namespace mpx
