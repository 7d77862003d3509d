// lab3: per-pixel Mahalanobis maximum-likelihood classification.
//
// Reference: lab3/src/main.cu:40-76 — for every pixel p, argmin over classes of
// (p - mu_c)^T A_c (p - mu_c) in fp64 with class statistics in __constant__
// memory; strict '<' keeps the lowest class on ties, an all-NaN pixel keeps
// class -1 (stored as 255); alpha is written in place.
//
// MI355X design
//   * class parameters travel as kernel arguments: the class loop index is
//     wave-uniform, so every parameter load is a scalar s_load into SGPRs — the
//     CDNA equivalent of a constant-cache broadcast, with no hipMemcpyToSymbol
//     in the launch path;
//   * each lane moves 4 pixels with one 16-B load and one 16-B store (the
//     reference does a 4-B load and a 1-B store per pixel);
//   * DIRECT: the fp64 FMA chain the reference GPU kernel compiles to, so the
//     classes are bit-identical to mpx_cpu_classify. fp64 VALU runs at half the
//     fp32 rate, so this path is VALU-bound at ~19 fp64 ops per (pixel, class).
//   * FAST32 and MFMA32 decide in fp32 and prove the decision:
//       Q_c(p) = sum_k w_ck phi_k(q),  phi = [r^2 g^2 b^2 rg rb gb r g b 1](q)
//     with q = p - 128 per channel (the expanded quadratic form of the
//     symmetrised A_c around the cube centre: |q| <= 128 keeps every term,
//     and so the rounding bound, ~4x smaller than around 0). The host bounds
//     |fp32 evaluation - reference fp64 chain| by tol_c for every pixel in
//     [0,255]^3 (rounding of the weights, of the 10-term fmaf chain and of the
//     reference chain itself). A pixel is classified in fp32 only if the
//     second-best value exceeds the best by more than 2 max_c tol_c; every
//     other pixel (near ties) is recomputed with the DIRECT chain, so all
//     paths produce identical classes.
//       - FAST32: VALU, two pixels per v_pk_fma_f32, 9 packed FMAs per class
//         and pixel pair;
//       - MFMA32: one v_mfma_f32_32x32x2f32 chain of K = 10 per 32 pixels x
//         32 classes (the distance GEMM; gfx950 f32 MFMA is a k-ordered fmaf
//         chain, so the same bound applies), the VALU only ranks the results.
//     The argmin works on 32-bit keys (value bits with the low 5 mantissa bits
//     replaced by the class index): best = min(best, key), second =
//     med3(best, key, second). A bias folded into the constant weight makes
//     every computed value positive, so unsigned key order is value order.
#include <algorithm>
#include <memory>
#include <mutex>
#include <tuple>
#include <utility>
#include <vector>
#include <cstdlib>
#include <cstring>

#include "internal.hpp"

#include <cmath>

namespace mpx {
namespace {

struct ClassParams {
    double mu[MPX_MAX_CLASSES * 3];
    double A[MPX_MAX_CLASSES * 9];
};

constexpr int kFeat = 10;

struct FastParams {
    float w[MPX_MAX_CLASSES][kFeat];  // expanded weights incl. bias; padded classes: 0 ... 0, 3e38
    float T2;                         // decision margin 2 * max_c tol_c
};

// one class of the reference chain
#define MPX_DIRECT_CLASS(c)                                                                               \
    do {                                                                                                  \
        const double d0 = pr - cp.mu[3 * (c) + 0];                                                        \
        const double d1 = pg - cp.mu[3 * (c) + 1];                                                        \
        const double d2 = pb - cp.mu[3 * (c) + 2];                                                        \
        const double *A = cp.A + 9 * (c);                                                                 \
        double t0 = fma(d0, A[0], 0.0), t1 = fma(d0, A[1], 0.0), t2 = fma(d0, A[2], 0.0);                \
        t0 = fma(d1, A[3], t0);                                                                           \
        t1 = fma(d1, A[4], t1);                                                                           \
        t2 = fma(d1, A[5], t2);                                                                           \
        t0 = fma(d2, A[6], t0);                                                                           \
        t1 = fma(d2, A[7], t1);                                                                           \
        t2 = fma(d2, A[8], t2);                                                                           \
        double dist = fma(t0, d0, 0.0);                                                                   \
        dist = fma(t1, d1, dist);                                                                         \
        dist = fma(t2, d2, dist);                                                                         \
        if (dist < best) {                                                                                \
            best = dist;                                                                                  \
            cls = (c);                                                                                    \
        }                                                                                                 \
    } while (0)

__device__ __forceinline__ uint32_t classify_direct(uint32_t p, int nc, const ClassParams &cp) {
    const double pr = (double)mpx_px_r(p), pg = (double)mpx_px_g(p), pb = (double)mpx_px_b(p);
    double best = 1.7976931348623157e308;  // DBL_MAX
    int cls = -1;
    // a plain loop: unrolled, the dynamic class index into the by-value kernel
    // argument made the compiler copy all of ClassParams to scratch (3080 B
    // per lane) in every kernel that inlines this chain (round 6)
    for (int c = 0; c < nc; ++c) MPX_DIRECT_CLASS(c);
    return (p & 0x00ffffffu) | ((uint32_t)(uint8_t)cls << 24);
}
#undef MPX_DIRECT_CLASS

__global__ void classify_direct_kernel(uint32_t *__restrict__ img, int64_t npix, int nc, ClassParams cp,
                                       int vec) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t done = 0;
    if (vec) {
        const int64_t nvec = npix / 4;
        uint4 *v = reinterpret_cast<uint4 *>(img);
        for (int64_t i = tid; i < nvec; i += stride) {
            uint4 q = v[i];
            q.x = classify_direct(q.x, nc, cp);
            q.y = classify_direct(q.y, nc, cp);
            q.z = classify_direct(q.z, nc, cp);
            q.w = classify_direct(q.w, nc, cp);
            v[i] = q;
        }
        done = nvec * 4;
    }
    for (int64_t i = done + tid; i < npix; i += stride) img[i] = classify_direct(img[i], nc, cp);
}

// ---------------------------------------------------------------------------
// fp32 decision helpers
// ---------------------------------------------------------------------------
typedef float f2_t __attribute__((ext_vector_type(2)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr uint32_t kKeyInit = 0x7f7fffe0u | 31u;  // ~FLT_MAX: "no class yet"

__device__ __forceinline__ uint32_t umed3(uint32_t a, uint32_t b, uint32_t c) {
    uint32_t r;
    asm("v_med3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

__device__ __forceinline__ uint32_t make_key(float d, uint32_t cls) {
    return (__float_as_uint(d) & ~31u) | cls;
}

// same, class index wave-uniform: one v_bfi_b32 (inline 31 + one SGPR), where
// the plain form needs v_and + v_or (gfx9 VOP3 takes no literal next to an SGPR)
__device__ __forceinline__ uint32_t make_key_s(float d, uint32_t cls) {
    uint32_t r;
    asm("v_bfi_b32 %0, 31, %1, %2" : "=v"(r) : "s"(cls), "v"(__float_as_uint(d)));
    return r;
}

// running top-2 over keys (B <= S invariant)
__device__ __forceinline__ void rank_key(uint32_t k, uint32_t &B, uint32_t &S) {
    S = umed3(B, k, S);
    B = min(B, k);
}

// merge another lane's (B2, S2) into (B, S)
__device__ __forceinline__ void merge_top2(uint32_t &B, uint32_t &S, uint32_t B2, uint32_t S2) {
    const uint32_t hi = max(B, B2);
    S = min(hi, min(S, S2));
    B = min(B, B2);
}

// true when the fp32 ranking provably equals the reference's. Keys lose at
// most 2^-18 of their value to the class tag, so it suffices that
// vs - vb > T2 + vb 2^-17 exactly; evaluating the test in fp32 costs at most
// 2^-23 relative on each side, covered by the 1.125 factor on vs >= vb and
// the host's (1 + 2^-20) inflation of T2.
__device__ __forceinline__ bool decided(uint32_t B, uint32_t S, float T2) {
    const float vb = __uint_as_float(B & ~31u), vs = __uint_as_float(S & ~31u);
    return (vs - vb) > fmaf(vs, 0x1.2p-17f, T2);
}

__device__ __forceinline__ uint32_t finish_pixel(uint32_t p, uint32_t B, uint32_t S, float T2, int nc,
                                                 const ClassParams &cp, uint32_t *amb) {
    if (__builtin_expect(decided(B, S, T2), 1)) return (p & 0x00ffffffu) | ((B & 31u) << 24);
    if (amb) atomicAdd(amb, 1u);
    return classify_direct(p, nc, cp);
}

// One pixel through the proven-margin fp32 ranking (the FAST32 arithmetic,
// unpacked): true with the class in `out` when the margin decides it.
__device__ __forceinline__ bool classify_fp32_one(uint32_t p, int nc, const FastParams &fp, uint32_t &out) {
    const float r = (float)(p & 0xffu) - 128.0f, g = (float)((p >> 8) & 0xffu) - 128.0f,
                b = (float)((p >> 16) & 0xffu) - 128.0f;
    const float f[9] = {r * r, g * g, b * b, r * g, r * b, g * b, r, g, b};
    uint32_t B = kKeyInit, S = kKeyInit;
    int c = 0;
    for (; c + 4 <= nc; c += 4) {  // one batch of scalar loads per four classes
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float *w = fp.w[c + j];
            float d = w[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) d = fmaf(w[k], f[k], d);
            rank_key(make_key(d, (uint32_t)(c + j)), B, S);
        }
    }
    for (; c < nc; ++c) {
        const float *w = fp.w[c];
        float d = w[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) d = fmaf(w[k], f[k], d);
        rank_key(make_key(d, (uint32_t)c), B, S);
    }
    out = (p & 0x00ffffffu) | ((B & 31u) << 24);
    return decided(B, S, fp.T2);
}

// ---------------------------------------------------------------------------
// FAST32: VALU, 4 pixels per lane as two packed pairs.
//
// Undecided pixels (top-2 margin within the fp32 bound, ~0.02%) are not
// re-ranked in fp64 inside the loop, where one such lane stalls its whole wave
// for a full fp64 chain: their indices go to a per-block LDS list and the
// block re-ranks them together after its grid-stride loop (all lanes busy)
// and overwrites the provisional fp32 result. A full list falls back to the
// inline fp64 chain.
// ---------------------------------------------------------------------------
constexpr int kAmbCap = 512;

// NQ = 2 16-B vectors (8 pixels) per thread and loop trip (nvec counts pairs
// of vectors): 8192^2, nc 4 / 16 / 32: 126 / 357-359 / 616-626 µs against 127
// / 361-365 / 638-641 with one (round 3). The pairs' FMA chains are issued
// interleaved (each FMA's result is needed NP / 2 instructions later, not by
// the next one) and the top-2 step is plain C (v_med3_u32 by pattern, no
// inline asm): nc = 16 / 32 307.6 -> 302.3 / 526.8 -> 521.7 µs (round 4).
// Non-temporal loads / stores, wave-contiguous vectors and two trips of loads
// in flight measured neutral (profiles/lab3_classify.md) and were removed.
constexpr int kFastNQ = 2;

__global__ __launch_bounds__(256) void classify_fast32_kernel(uint32_t *__restrict__ img, int64_t nvec, int nc,
                                                              ClassParams cp, FastParams fp, uint32_t *amb) {
    constexpr int NQ = kFastNQ;
    constexpr int NP = 4 * NQ;  // pixels per thread and trip
    __shared__ int64_t s_amb[kAmbCap];
    __shared__ uint32_t s_ambpx[kAmbCap];
    __shared__ uint32_t s_namb;
    if (threadIdx.x == 0) s_namb = 0;
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    uint4 *v = reinterpret_cast<uint4 *>(img);
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    // software-pipelined grid-stride loop: the next 16-B vectors are in flight
    // while these are ranked (a thread walks ~32 vectors at 8192^2; without
    // the prefetch each step exposes a full HBM round trip)
    auto load_q = [&](uint4 (&q)[NQ], int64_t it) {
#pragma unroll
        for (int qq = 0; qq < NQ; ++qq) q[qq] = it < nvec ? v[it * NQ + qq] : uint4{};
    };
    auto unpack = [&](const uint4 (&q)[NQ], uint32_t (&px)[NP]) {
#pragma unroll
        for (int qq = 0; qq < NQ; ++qq) {
            px[4 * qq + 0] = q[qq].x;
            px[4 * qq + 1] = q[qq].y;
            px[4 * qq + 2] = q[qq].z;
            px[4 * qq + 3] = q[qq].w;
        }
    };
    // rank the NP pixels of trip i and store them
    auto rank_store = [&](const uint32_t (&px)[NP], int64_t i) {
        f2_t f[NP / 2][9];
#pragma unroll
        for (int h = 0; h < NP / 2; ++h) {
            // channel - 128, exact in fp32 (v_cvt_f32_ubyteN + one packed add).
            // NB: (float)__builtin_amdgcn_sbfe(x, o, 8) is miscompiled by hipcc
            // 7.2 into v_cvt_f32_u32_sdwa sext(x) (negative values convert as
            // unsigned), so signed bytes are never converted directly.
            const uint32_t a = px[2 * h], b = px[2 * h + 1];
            const f2_t c128 = {-128.0f, -128.0f};
            const f2_t r = f2_t{(float)(a & 0xffu), (float)(b & 0xffu)} + c128;
            const f2_t g = f2_t{(float)((a >> 8) & 0xffu), (float)((b >> 8) & 0xffu)} + c128;
            const f2_t bl = f2_t{(float)((a >> 16) & 0xffu), (float)((b >> 16) & 0xffu)} + c128;
            f[h][0] = r * r;
            f[h][1] = g * g;
            f[h][2] = bl * bl;
            f[h][3] = r * g;
            f[h][4] = r * bl;
            f[h][5] = g * bl;
            f[h][6] = r;
            f[h][7] = g;
            f[h][8] = bl;
        }
        uint32_t B[NP], S[NP];
#pragma unroll
        for (int q = 0; q < NP; ++q) B[q] = S[q] = kKeyInit;
        auto one_class = [&](int c) {
            const float *w = fp.w[c];
            f2_t d[NP / 2];
#pragma unroll
            for (int h = 0; h < NP / 2; ++h) d[h] = f2_t{w[9], w[9]};
#pragma unroll
            for (int k = 0; k < 9; ++k)
#pragma unroll
                for (int h = 0; h < NP / 2; ++h) d[h] = __builtin_elementwise_fma(f2_t{w[k], w[k]}, f[h][k], d[h]);
#pragma unroll
            for (int h = 0; h < NP / 2; ++h) {
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    const uint32_t k = make_key_s(q ? d[h].y : d[h].x, (uint32_t)c);
                    uint32_t &Bq = B[2 * h + q], &Sq = S[2 * h + q];
                    Sq = max(min(Bq, k), min(max(Bq, k), Sq));
                    Bq = min(Bq, k);
                }
            }
        };
        // four classes per iteration: their weights' scalar loads issue
        // together (one s_waitcnt per four classes instead of per class)
        int c = 0;
        for (; c + 4 <= nc; c += 4) {
            one_class(c);
            one_class(c + 1);
            one_class(c + 2);
            one_class(c + 3);
        }
        for (; c < nc; ++c) one_class(c);
        uint32_t o[NP];
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            o[k] = (px[k] & 0x00ffffffu) | ((B[k] & 31u) << 24);
            if (__builtin_expect(!decided(B[k], S[k], fp.T2), 0)) {
                const uint32_t slot = atomicAdd(&s_namb, 1u);  // also the block's count (one global add at the end)
                if (slot < (uint32_t)kAmbCap) {  // deferred
                    s_amb[slot] = (i * NQ + (k >> 2)) * 4 + (k & 3);
                    s_ambpx[slot] = px[k];
                } else {
                    o[k] = classify_direct(px[k], nc, cp);
                }
            }
        }
#pragma unroll
        for (int qq = 0; qq < NQ; ++qq) v[i * NQ + qq] = make_uint4(o[4 * qq], o[4 * qq + 1], o[4 * qq + 2], o[4 * qq + 3]);
    };
    uint4 qn[NQ];
    load_q(qn, i);
    for (; i < nvec; i += stride) {
        uint32_t px[NP];
        unpack(qn, px);
        if (i + stride < nvec) load_q(qn, i + stride);
        rank_store(px, i);
    }
    __syncthreads();
    const uint32_t nd = min(s_namb, (uint32_t)kAmbCap);
    // the ambiguity count: one global add per block, not one per pixel
    if (amb && threadIdx.x == 0 && s_namb) atomicAdd(amb, s_namb);
    for (uint32_t j = threadIdx.x; j < nd; j += blockDim.x) {
        img[s_amb[j]] = classify_direct(s_ambpx[j], nc, cp);
    }
}

// ---------------------------------------------------------------------------
// MFMA32: distance GEMM on v_mfma_f32_32x32x2f32.
//   D[class][pixel] = sum_k W[class][k] * PHI[k][pixel], K = 10 = 5 MFMAs.
//   A (W):   lane l holds W[class = l & 31][k = 2t + (l >> 5)]  (loaded once)
//   B (PHI): lane l holds phi_{2t + (l >> 5)}(pixel l & 31)
//   D:       lane l, reg r holds class (r & 3) + 8 (r >> 2) + 4 (l >> 5), pixel l & 31
// A wave takes 128-pixel chunks: lane l loads the 16 B at pixel 4 (l & 31)
// (both half-waves load the same bytes), and group m = 0..3 uses pixel
// 4 (l & 31) + m as column l & 31, so every result lands in the lane that
// owns the pixel's uint4. The two half-waves' top-2 keys are merged with
// v_permlane32_swap. NREG = accumulator registers with real classes (4 for
// nc <= 8, 8 for nc <= 16, 12 for nc <= 24, 16 for nc <= 32).
// ---------------------------------------------------------------------------
template <int NREG>
__global__ __launch_bounds__(256) void classify_mfma32_kernel(uint32_t *__restrict__ img, int64_t nchunks, int nc,
                                                              ClassParams cp, FastParams fp, uint32_t *amb) {
    const int lane = threadIdx.x & 63;
    const int h = lane >> 5;
    const int col = lane & 31;
    const int64_t wave = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x >> 6);
    float a[5];
#pragma unroll
    for (int t = 0; t < 5; ++t) a[t] = fp.w[col][2 * t + h];
    // feature byte offsets for k = 2t + h (see the table in the header)
    const uint32_t sx0 = 8u * h, sy0 = 8u * h;   // rr | gg
    const uint32_t sx1 = h ? 0u : 16u;            // bb | rg
    const uint32_t sy1 = h ? 8u : 16u;
    const uint32_t sx2 = 8u * h, sy2 = 16u;       // rb | gb
    const uint32_t sx3 = 8u * h;                  // r  | g
    const uint32_t tag = 4u * h;                  // class offset of this half-wave's rows
    uint4 *v = reinterpret_cast<uint4 *>(img);
    for (int64_t ch = wave; ch < nchunks; ch += nwaves) {
        const uint4 q = v[ch * 32 + col];
        const uint32_t px[4] = {q.x, q.y, q.z, q.w};
        f32x16 acc[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            // signed bytes (channel - 128) feed the exact integer products; the
            // single-channel features convert the unsigned byte and subtract 128
            // (see the sbfe miscompile note in the FAST32 kernel)
            const int p = (int)(px[m] ^ 0x80808080u);
            const float phi0 = (float)(__mul24(__builtin_amdgcn_sbfe(p, sx0, 8), __builtin_amdgcn_sbfe(p, sy0, 8)));
            const float phi1 = (float)(__mul24(__builtin_amdgcn_sbfe(p, sx1, 8), __builtin_amdgcn_sbfe(p, sy1, 8)));
            const float phi2 = (float)(__mul24(__builtin_amdgcn_sbfe(p, sx2, 8), __builtin_amdgcn_sbfe(p, sy2, 8)));
            const float phi3 = (float)__builtin_amdgcn_ubfe(px[m], sx3, 8) - 128.0f;
            const float phi4 = h ? 1.0f : (float)((px[m] >> 16) & 0xffu) - 128.0f;
            f32x16 c = {};
            c = __builtin_amdgcn_mfma_f32_32x32x2f32(a[0], phi0, c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_32x32x2f32(a[1], phi1, c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_32x32x2f32(a[2], phi2, c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_32x32x2f32(a[3], phi3, c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4], phi4, c, 0, 0, 0);
            acc[m] = c;
        }
        uint32_t rb[4], rs[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            uint32_t B = make_key(acc[m][0], 0u), S = kKeyInit;
#pragma unroll
            for (int r = 1; r < NREG; ++r) rank_key(make_key(acc[m][r], (uint32_t)((r & 3) + 8 * (r >> 2))), B, S);
            B |= tag;  // row tags (r & 3) + 8 (r >> 2) never set bit 2
            S |= tag;
            const auto sb = __builtin_amdgcn_permlane32_swap(B, B, false, false);
            const auto ss = __builtin_amdgcn_permlane32_swap(S, S, false, false);
            // (sb[0], sb[1]) = (own, partner) in either order: the merge is symmetric
            B = sb[0];
            S = ss[0];
            merge_top2(B, S, sb[1], ss[1]);
            rb[m] = B;
            rs[m] = S;
        }
        if (h == 0) {
            uint4 o;
            o.x = finish_pixel(q.x, rb[0], rs[0], fp.T2, nc, cp, amb);
            o.y = finish_pixel(q.y, rb[1], rs[1], fp.T2, nc, cp, amb);
            o.z = finish_pixel(q.z, rb[2], rs[2], fp.T2, nc, cp, amb);
            o.w = finish_pixel(q.w, rb[3], rs[3], fp.T2, nc, cp, amb);
            v[ch * 32 + col] = o;
        }
    }
}

// ---------------------------------------------------------------------------
// MFMA64: the distance GEMM in fp64 on v_mfma_f64_16x16x4_f64.
//   D[class][pixel] = sum_k W[class][k] * PHI[k][pixel], K = 12 (10 features,
//   k = 10, 11 carry zero weights) = 3 MFMAs per 16 classes x 16 pixels.
//   A (W):   lane l holds W[class = 16 T + (l & 15)][k = 4t + (l >> 4)]
//   B (PHI): lane l holds phi_{4t + (l >> 4)}(pixel l & 15)
//   D:       lane l, reg r holds class 16 T + (l >> 4) + 4 r, pixel l & 15
//            (the f64 C/D map, not the f32 one)
// Every feature is one integer product x_a x_b of the centred bytes
// {r, g, b, 1}: lane group g = l >> 4 picks the byte pair of its k once
// (kPair), so the feature build is branch-free and exact. A wave takes 64-pixel
// chunks: lane l loads the 16 B at pixel 4 (l & 15) (all four lane groups load
// the same bytes) and group m = 0..3 uses pixel 4 (l & 15) + m as column
// l & 15. The four lane groups' top-2 lists are merged with two xor shuffles.
// fp64 keeps the bound ~2^29 x tighter than fp32, so the exact fallback is
// taken only on genuine near-ties; NT = 16-class tiles (1 for nc <= 16, else 2).
// ---------------------------------------------------------------------------
typedef double f64x4 __attribute__((ext_vector_type(4)));

struct Fast64Params {
    double w[MPX_MAX_CLASSES][kFeat];  // padded classes: 0 ... 0, 1e300
    double T2;                         // decision margin 2 * max_c tol_c
};

// byte pair (a, b) of feature k: phi_k = (byte_a - 128) (byte_b - 128), byte 3 = 129 (the constant 1)
__constant__ const uint8_t kPair[12][2] = {{0, 0}, {1, 1}, {2, 2}, {0, 1}, {0, 2}, {1, 2},
                                           {0, 3}, {1, 3}, {2, 3}, {3, 3}, {3, 3}, {3, 3}};

// fp64 keys: the low 5 mantissa bits carry the class (a relative change of at
// most 2^-47, inside the decision slack), so the running top-2 is three f64
// min/max per entry and the class comes back with the winning value.
__device__ __forceinline__ double tag_f64(double d, uint32_t cls) {
    const uint64_t u = (uint64_t)__double_as_longlong(d);
    return __longlong_as_double((long long)((u & ~31ull) | cls));
}

__device__ __forceinline__ void rank_f64(double k, double &B, double &S) {
    S = fmin(S, fmax(B, k));
    B = fmin(B, k);
}

// (B, S) of this lane and of its partner lane across a permlane swap: the
// swap returns {own, partner} in an order that differs between the two
// lanes, and the merge is symmetric, so both end with the merged pair
template <bool X32>
__device__ __forceinline__ void merge_lanes_f64(double &B, double &S) {
    const uint64_t ub = (uint64_t)__double_as_longlong(B), us = (uint64_t)__double_as_longlong(S);
    const uint32_t w[4] = {(uint32_t)ub, (uint32_t)(ub >> 32), (uint32_t)us, (uint32_t)(us >> 32)};
    uint32_t x[4], y[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const auto r = X32 ? __builtin_amdgcn_permlane32_swap(w[i], w[i], false, false)
                           : __builtin_amdgcn_permlane16_swap(w[i], w[i], false, false);
        x[i] = r[0];
        y[i] = r[1];
    }
    auto dbl = [](uint32_t lo, uint32_t hi) { return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo)); };
    const double B0 = dbl(x[0], x[1]), S0 = dbl(x[2], x[3]), B1 = dbl(y[0], y[1]), S1 = dbl(y[2], y[3]);
    S = fmin(fmax(B0, B1), fmin(S0, S1));
    B = fmin(B0, B1);
}

template <int NT>
__global__ __launch_bounds__(256) void classify_mfma64_kernel(uint32_t *__restrict__ img, int64_t nchunks, int nc,
                                                              ClassParams cp, Fast64Params fp, uint32_t *amb) {
    const int lane = threadIdx.x & 63;
    const int g = lane >> 4;
    const int col = lane & 15;
    const int64_t wave = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x >> 6);
    double a[NT][3];
    uint32_t sa[3], sb[3];
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const int k = 4 * t + g;
#pragma unroll
        for (int T = 0; T < NT; ++T) a[T][t] = k < kFeat ? fp.w[16 * T + col][k] : 0.0;
        sa[t] = 8u * kPair[k][0];
        sb[t] = 8u * kPair[k][1];
    }
    uint4 *v = reinterpret_cast<uint4 *>(img);
    int64_t ch = wave;
    uint4 qn = ch < nchunks ? v[ch * 16 + col] : uint4{};
    for (; ch < nchunks; ch += nwaves) {
        const uint4 q = qn;
        if (ch + nwaves < nchunks) qn = v[(ch + nwaves) * 16 + col];
        const uint32_t px[4] = {q.x, q.y, q.z, q.w};
        double vb[4], vs[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const uint32_t p = (px[m] & 0x00ffffffu) | (129u << 24);
            double phi[3];
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                const int x = (int)__builtin_amdgcn_ubfe(p, sa[t], 8) - 128;
                const int y = (int)__builtin_amdgcn_ubfe(p, sb[t], 8) - 128;
                phi[t] = (double)__mul24(x, y);
            }
            vb[m] = 1.7976931348623157e308;  // DBL_MAX: low 5 bits already 31
            vs[m] = 1.7976931348623157e308;
#pragma unroll
            for (int T = 0; T < NT; ++T) {
                f64x4 c = {};
                c = __builtin_amdgcn_mfma_f64_16x16x4f64(a[T][0], phi[0], c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f64_16x16x4f64(a[T][1], phi[1], c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f64_16x16x4f64(a[T][2], phi[2], c, 0, 0, 0);
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (16 * T + 4 * r < nc)  // wave-uniform: skip rows holding only padded classes
                        rank_f64(tag_f64(c[r], (uint32_t)(16 * T + g + 4 * r)), vb[m], vs[m]);
            }
            merge_lanes_f64<false>(vb[m], vs[m]);
            merge_lanes_f64<true>(vb[m], vs[m]);
        }
        if (g == 0) {
            uint4 o;
            uint32_t *op = &o.x;
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                // proven: the reference chain ranks the same class first (see
                // build_fast64); 2^-46 covers both keys' tags and the subtraction
                if (__builtin_expect((vs[m] - vb[m]) > fma(fabs(vs[m]) + fabs(vb[m]), 0x1p-46, fp.T2), 1)) {
                    const uint32_t cls = (uint32_t)__double_as_longlong(vb[m]) & 31u;
                    op[m] = (px[m] & 0x00ffffffu) | (cls << 24);
                } else {
                    if (amb) atomicAdd(amb, 1u);
                    op[m] = classify_direct(px[m], nc, cp);
                }
            }
            v[ch * 16 + col] = o;
        }
    }
}


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

struct I8Params {
    uint64_t a[MPX_MAX_CLASSES][2];  // hi limbs: [class][half] = 8 int8 weights of k = 8 half .. +7
    uint64_t b[MPX_MAX_CLASSES][2];  // lo limbs
    int32_t c[MPX_MAX_CLASSES];      // round(w9 / u); padded classes: 2^26 - 64 (never the argmin)
    int32_t T2;                      // decision margin in key units (key >> 5)
};

constexpr int kAmb8Cap = 2048;

__device__ __forceinline__ int32_t imed3(int32_t a, int32_t b, int32_t c) {
    int32_t r;
    asm("v_med3_i32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

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
//   kMfma8sMaxClasses = 13 classes (8 for MPX_CLS_MFMA8S_MAX=16, A/B).
// ---------------------------------------------------------------------------
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

// The deferred list holds one entry per (lane, trip) with any undecided
// pixel: the 16-B vector index and a 4-bit mask of its undecided pixels —
// one append per trip instead of one per pixel (with ~0.4% of the pixels
// undecided at nc = 4, a quarter of the trips have one). The pixels are
// re-read from the image after the loop: their RGB bytes are untouched.
// Every list is private to one wave (its own LDS rows and counters): a wave
// appends, then ranks its own deferred pixels, in program order — LDS
// operations of one wave execute in order — so the kernel has no block
// barrier, and short-lived workgroups cost no more than long ones.
constexpr int kAmb8sCapW = 256;   // deferred (vector, mask) entries per wave
constexpr int kAmb8sCap2W = 64;   // pixels the fp32 stage leaves to the fp64 chain, per wave

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
    // this wave's deferred pixels: the fp32 proven-margin ranking first, the
    // exact fp64 chain for what it leaves (every lane of the wave busy in each
    // stage); the wave's appends above precede these reads in program order
    __builtin_amdgcn_wave_barrier();
    const uint32_t nd = min(s_namb[w], (uint32_t)kAmb8sCapW);
    for (uint32_t j = lane; j < nd; j += 64) {
        const int64_t e = s_amb[w][j];
        const int64_t vi = e >> 4;
        const uint32_t mask = (uint32_t)e & 15u;
        atomicAdd(&s_npx[w], (uint32_t)__popc(mask));
        const uint4 q = v[vi];  // a vector this wave wrote above, in program order
        const uint32_t px[4] = {q.x, q.y, q.z, q.w};
        for (int m = 0; m < 4; ++m) {
            if (!((mask >> m) & 1u)) continue;
            uint32_t o;
            if (classify_fp32_one(px[m], nc, fp, o)) {
                img[vi * 4 + m] = o;
            } else {
                const uint32_t slot = atomicAdd(&s_namb2[w], 1u);
                if (slot < (uint32_t)kAmb8sCap2W) {
                    s_amb2[w][slot] = vi * 4 + m;
                    s_ambpx2[w][slot] = px[m];
                } else {
                    img[vi * 4 + m] = classify_direct(px[m], nc, cp);
                }
            }
        }
    }
    __builtin_amdgcn_wave_barrier();
    if (amb && lane == 0 && s_npx[w]) atomicAdd(amb, s_npx[w]);  // one global add per wave with any
    const uint32_t nd2 = min(s_namb2[w], (uint32_t)kAmb8sCap2W);
    for (uint32_t j = lane; j < nd2; j += 64) img[s_amb2[w][j]] = classify_direct(s_ambpx2[w][j], nc, cp);
}

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

constexpr int kHalfMfmas = 3;  // MFMAs per 16-class set

struct HalfParams {
    uint32_t w[2][kHalfMfmas][16][4];  // [set][mfma][class in set]: 8 f16 slot weights (the A row)
    float c[MPX_MAX_CLASSES];          // accumulator init: scaled constant + bias; padded classes 3e38
    float T2;                          // decision margin (scaled units; the FAST32 test)
};

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

// Undecided pixels of a whole launch: each wave appends its LDS list of
// (vector << 4 | pixel mask) entries to one device list (one atomic per wave)
// and classify_fixup_kernel re-ranks them all afterwards, every lane busy. At
// 0.05-0.1 % undecided a wave holds ~1-4 entries, and re-ranking them inside
// the wave ran the fp32 stage (~15 VALU x nc per pixel slot) once per wave for
// a handful of lanes: ~25 % of the kernel's VALU at 32 classes (round-6
// counters, profiles/lab3_classify.md).
// The list is split into kDeferSubs sub-lists (sub-list = workgroup id mod
// kDeferSubs, each with its own counter): one counter for the whole launch
// serialised ~16K same-address atomics in the L2 (+30-50 µs at 4-16
// classes, round 6). Fix-up block b owns sub-list b: it reads its count,
// re-ranks the entries and zeroes the count for the next launch.
constexpr uint32_t kDeferSubs = 256;
struct DeferList {
    uint64_t *ent;  // kDeferSubs x cap entries; nullptr: re-rank inside each wave (no device list)
    uint32_t *ctr;  // 2 x kDeferSubs counters, used by calls of alternating parity
    uint32_t cap;   // entries per sub-list
    uint32_t par;   // this call's parity: the fix-up zeroes the other parity's counters for the next call
};

// re-rank the undecided pixels of one entry: fp32 proven margin, else fp64
__device__ __forceinline__ uint32_t fix_entry(uint32_t *img, uint64_t e, int nc, const ClassParams &cp,
                                              const FastParams &fp) {
    const int64_t vi = (int64_t)(e >> 4);
    const uint32_t mask = (uint32_t)e & 15u;
    const uint4 q = reinterpret_cast<const uint4 *>(img)[vi];
    const uint32_t px[4] = {q.x, q.y, q.z, q.w};
    for (int m = 0; m < 4; ++m) {
        if (!((mask >> m) & 1u)) continue;
        uint32_t o;
        if (!classify_fp32_one(px[m], nc, fp, o)) o = classify_direct(px[m], nc, cp);
        img[vi * 4 + m] = o;
    }
    return (uint32_t)__popc(mask);
}

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
// whole image when no device deferral list could be allocated.
template <int NSET, int NR>
__global__ __launch_bounds__(256) void classify_mfma16_kernel(uint32_t *__restrict__ img, int64_t nvec, int nc,
                                                              ClassParams cp, HalfParams hp, FastParams fp,
                                                              DeferList dl, uint32_t *amb) {
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
    __builtin_amdgcn_wave_barrier();
    const uint32_t nd = min(s_namb[w], (uint32_t)kAmb8sCapW);
    if (dl.ent != nullptr) {  // to the launch's device list (classify_fixup_kernel)
        if (nd == 0) return;
        const uint32_t sub = blockIdx.x % kDeferSubs;
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(&dl.ctr[dl.par * kDeferSubs + sub], nd);
        base = __shfl(base, 0);
        uint64_t *ent = dl.ent + (size_t)sub * dl.cap;
        uint32_t over = 0;
        for (uint32_t j = lane; j < nd; j += 64) {
            const uint64_t e = (uint64_t)s_amb[w][j];
            if (base + j < dl.cap)
                ent[base + j] = e;
            else
                over += fix_entry(img, e, nc, cp, fp);  // list full: this lane re-ranks it (never at benchmark rates)
        }
        if (amb && over) atomicAdd(amb, over);
        return;
    }
    // this wave's deferred pixels: the fp32 proven-margin ranking first, the
    // exact fp64 chain for what it leaves (every lane of the wave busy in each)
    for (uint32_t j = lane; j < nd; j += 64) {
        const int64_t e = s_amb[w][j];
        const int64_t vi = e >> 4;
        const uint32_t mask = (uint32_t)e & 15u;
        atomicAdd(&s_npx[w], (uint32_t)__popc(mask));
        const uint4 q = v[vi];  // written by this wave above, in program order
        const uint32_t px[4] = {q.x, q.y, q.z, q.w};
        for (int m = 0; m < 4; ++m) {
            if (!((mask >> m) & 1u)) continue;
            uint32_t o;
            if (classify_fp32_one(px[m], nc, fp, o)) {
                img[vi * 4 + m] = o;
            } else {
                const uint32_t slot = atomicAdd(&s_namb2[w], 1u);
                if (slot < (uint32_t)kAmb8sCap2W) {
                    s_amb2[w][slot] = vi * 4 + m;
                    s_ambpx2[w][slot] = px[m];
                } else {
                    img[vi * 4 + m] = classify_direct(px[m], nc, cp);
                }
            }
        }
    }
    __builtin_amdgcn_wave_barrier();
    if (amb && lane == 0 && s_npx[w]) atomicAdd(amb, s_npx[w]);
    const uint32_t nd2 = min(s_namb2[w], (uint32_t)kAmb8sCap2W);
    for (uint32_t j = lane; j < nd2; j += 64) img[s_amb2[w][j]] = classify_direct(s_ambpx2[w][j], nc, cp);
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

// ---------------------------------------------------------------------------
// Host: expanded fp32 weights and the rigorous decision margin.
// ---------------------------------------------------------------------------
typedef long double ld;

// |q_i q_j| <= 128^2, |q_i| <= 128 for q = p - 128, p in [0, 255]^3
constexpr ld kPhiMax[kFeat] = {16384, 16384, 16384, 16384, 16384, 16384, 128, 128, 128, 1};

// Expanded weights w[c][k] of the centred quadratic form, the reference
// chain's own error bound refb[c] and the indefiniteness slack psd[c]. False
// for non-finite statistics or a symmetrised A that is not positive definite.
bool expand_classes(int nc, const double *mu, const double *inv, ld (*w)[kFeat], ld *refb, ld *psd) {
    const ld u64 = std::ldexp((ld)1, -53);
    for (int c = 0; c < nc; ++c) {
        const double *A = inv + 9 * c;
        const double *mraw = mu + 3 * c;
        for (int i = 0; i < 3; ++i)
            if (!std::isfinite(mraw[i])) return false;
        const ld m[3] = {(ld)mraw[0] - 128, (ld)mraw[1] - 128, (ld)mraw[2] - 128};  // centred mean (exact)
        for (int i = 0; i < 9; ++i)
            if (!std::isfinite(A[i])) return false;
        ld S[3][3];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) S[i][j] = ((ld)A[3 * i + j] + (ld)A[3 * j + i]) / 2;
        // positive definiteness (Cholesky pivots): Q_c >= 0 keeps biased values positive
        const ld p0 = S[0][0];
        if (!(p0 > 0)) return false;
        const ld l10 = S[1][0] / p0, l20 = S[2][0] / p0;
        const ld p1 = S[1][1] - l10 * S[1][0];
        if (!(p1 > 0)) return false;
        const ld l21 = (S[2][1] - l20 * S[1][0]) / p1;
        const ld p2 = S[2][2] - l20 * S[2][0] - l21 * (S[2][1] - l20 * S[1][0]);
        if (!(p2 > 0)) return false;
        ld Sm[3], sabs = 0, dmax[3];
        for (int i = 0; i < 3; ++i) {
            Sm[i] = S[i][0] * m[0] + S[i][1] * m[1] + S[i][2] * m[2];
            dmax[i] = std::fmax(std::fabs((ld)mraw[i]), std::fabs(255 - (ld)mraw[i])) * (1 + 4 * u64);
        }
        w[c][0] = S[0][0];
        w[c][1] = S[1][1];
        w[c][2] = S[2][2];
        w[c][3] = 2 * S[0][1];
        w[c][4] = 2 * S[0][2];
        w[c][5] = 2 * S[1][2];
        w[c][6] = -2 * Sm[0];
        w[c][7] = -2 * Sm[1];
        w[c][8] = -2 * Sm[2];
        w[c][9] = m[0] * Sm[0] + m[1] * Sm[1] + m[2] * Sm[2];
        // reference fp64 chain: |computed - exact| <= ~8 u sum |A_ij| |d_i| |d_j|; 16 u for margin
        ld aq = 0;
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                aq += std::fabs((ld)A[3 * i + j]) * dmax[i] * dmax[j];
                sabs += std::fabs(S[i][j]);
            }
        refb[c] = 16 * u64 * aq;
        // a slightly indefinite S hidden by long-double rounding: Q >= -1e-15 |S| |d|^2
        psd[c] = 1e-15L * sabs * (dmax[0] * dmax[0] + dmax[1] * dmax[1] + dmax[2] * dmax[2]);
    }
    return true;
}

// false when the fp32 decision cannot be proven (non-finite statistics, a
// symmetrised A that is not positive definite, or magnitudes near fp32 range)
bool build_fast(int nc, const double *mu, const double *inv, FastParams &fp) {
    const ld u32 = std::ldexp((ld)1, -24);
    const ld g10 = 10 * u32 / (1 - 10 * u32);
    const ld *phimax = kPhiMax;
    ld w[MPX_MAX_CLASSES][kFeat], refb[MPX_MAX_CLASSES], psd[MPX_MAX_CLASSES];
    if (!expand_classes(nc, mu, inv, w, refb, psd)) return false;
    auto tol = [&](int c, ld bias, float *out) -> ld {
        ld mag = 0, rep = 0, ev = 0;
        for (int k = 0; k < kFeat; ++k) {
            const ld wk = w[c][k] + (k == 9 ? bias : 0);
            const float f = (float)wk;
            if (out) out[k] = f;
            rep += std::fabs((ld)f - wk) * phimax[k];
            ev += std::fabs((ld)f) * phimax[k];
            mag += std::fabs(wk) * phimax[k];
        }
        // fp32 chain + weight rounding + long-double arithmetic slack + reference chain
        return (g10 * ev + rep + 1e-15L * mag + refb[c] + psd[c]) * 1.001L + 1e-30L;
    };
    ld tmax0 = 0, mag = 0;
    for (int c = 0; c < nc; ++c) {
        tmax0 = std::fmax(tmax0, tol(c, 0, nullptr));
        for (int k = 0; k < kFeat; ++k) mag = std::fmax(mag, std::fabs(w[c][k]) * phimax[k]);
    }
    if (!(mag < 1e30L)) return false;
    const ld bias = 4 * tmax0;
    ld tmax = 0;
    for (int c = 0; c < nc; ++c) tmax = std::fmax(tmax, tol(c, bias, fp.w[c]));
    if (!(bias > 2 * tmax)) return false;
    for (int c = nc; c < MPX_MAX_CLASSES; ++c)
        for (int k = 0; k < kFeat; ++k) fp.w[c][k] = (k == 9) ? 3.0e38f : 0.0f;
    const ld t2x = 2 * tmax * (1 + std::ldexp((ld)1, -20));  // see decided()
    float t2 = (float)t2x;
    if ((ld)t2 < t2x) t2 = std::nextafter(t2, INFINITY);
    fp.T2 = t2;
    return true;
}

// fp64 weights for MFMA64. The f64 MFMA's summation order and internal
// rounding are not specified, so its error is bounded as any 12-term sum with
// unit roundoff 2^-52 (twice RNE's, covering a truncating adder):
// gamma_12 sum_k |w_k| phimax_k, plus the weight rounding and the reference
// chain's error; a pixel is decided in fp64 only beyond 2 max_c tol_c.
bool build_fast64(int nc, const double *mu, const double *inv, Fast64Params &fp) {
    const ld u = std::ldexp((ld)1, -52);
    const ld g12 = 12 * u / (1 - 12 * u);
    ld w[MPX_MAX_CLASSES][kFeat], refb[MPX_MAX_CLASSES], psd[MPX_MAX_CLASSES];
    if (!expand_classes(nc, mu, inv, w, refb, psd)) return false;
    ld tmax = 0;
    for (int c = 0; c < nc; ++c) {
        ld ev = 0, rep = 0, mag = 0;
        for (int k = 0; k < kFeat; ++k) {
            const double f = (double)w[c][k];
            fp.w[c][k] = f;
            ev += std::fabs((ld)f) * kPhiMax[k];
            rep += std::fabs((ld)f - w[c][k]) * kPhiMax[k];
            mag += std::fabs(w[c][k]) * kPhiMax[k];
        }
        if (!(mag < 1e300L)) return false;
        // long-double expansion slack: ~20 operations at 2^-64 each
        const ld t = (g12 * ev + rep + 1e-17L * mag + refb[c]) * 1.001L + 1e-300L;
        tmax = std::fmax(tmax, t);
    }
    for (int c = nc; c < MPX_MAX_CLASSES; ++c)
        for (int k = 0; k < kFeat; ++k) fp.w[c][k] = (k == 9) ? 1e300 : 0.0;
    const ld t2x = 2 * tmax * (1 + std::ldexp((ld)1, -40));
    double t2 = (double)t2x;
    if ((ld)t2 < t2x) t2 = std::nextafter(t2, INFINITY);
    fp.T2 = t2;
    return true;
}


// Integer weights for MFMA8 (see the kernel): slot weights V_s as
// v_s = round(V_s / u) with |v_s| <= 32639 (two int8 limbs), the constant as
// c = round(w9 / u) in the accumulator; u is doubled until every key fits
// int32 after the 5-bit class tag (|sum_s Fmax_s |v_s|| + |c| < 2^26). The
// decision bound per class: u/2 per unit of feature magnitude (weight
// rounding; the int32 arithmetic is exact) + u/2 (constant) + the reference
// chain's error; T2 = ceil(2 max_c tol_c / u) + 1 in key units.
constexpr int kSlots = 16;
// slot -> (expanded weight index, scale, max |feature|)
constexpr int kSlotW[kSlots] = {0, 1, 2, 3, 4, 5, 6, 7, 0, 1, 2, 3, 4, 5, 8, -1};
constexpr ld kSlotScale[kSlots] = {256, 256, 256, 256, 256, 256, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0};
constexpr ld kSlotFmax[kSlots] = {64, 64, 64, 64, 64, 64, 128, 128, 128, 128, 128, 128, 128, 128, 128, 0};

bool build_i8(int nc, const double *mu, const double *inv, I8Params &ip) {
    ld w[MPX_MAX_CLASSES][kFeat], refb[MPX_MAX_CLASSES], psd[MPX_MAX_CLASSES];
    if (!expand_classes(nc, mu, inv, w, refb, psd)) return false;
    ld vmax = 0, mag = 0;
    for (int c = 0; c < nc; ++c)
        for (int s = 0; s < kSlots; ++s)
            if (kSlotW[s] >= 0) {
                vmax = std::fmax(vmax, std::fabs(w[c][kSlotW[s]] * kSlotScale[s]));
                mag = std::fmax(mag, std::fabs(w[c][kSlotW[s]]) * kPhiMax[kSlotW[s]]);
            }
    if (!(vmax > 0) || !(mag < 1e30L)) return false;
    // The decision bound uses the weights' ACTUAL rounding errors (round 5):
    // per class, u (sum_s |delta_cs| Fmax_s + |delta_c|) with delta = the
    // integer minus the exact scaled weight, instead of the worst case u / 2
    // per unit — and the scale u is chosen among 64 candidates (up to +25 %) above the
    // smallest that fits for the smallest margin in value units (T2 u), so
    // fewer pixels fall inside it and take the exact fallback.
    long long v[MPX_MAX_CLASSES][kSlots], cc[MPX_MAX_CLASSES];
    auto fits_at = [&](ld u, long long (*vv)[kSlots], long long *cv) -> bool {
        for (int c = 0; c < nc; ++c) {
            ld tot = 0;
            for (int s = 0; s < kSlots; ++s) {
                vv[c][s] = kSlotW[s] >= 0 ? std::llround(w[c][kSlotW[s]] * kSlotScale[s] / u) : 0;
                if (std::llabs(vv[c][s]) > 32639) return false;
                tot += kSlotFmax[s] * (ld)std::llabs(vv[c][s]);
            }
            const ld cw = w[c][9] / u;
            if (!(std::fabs(cw) < (ld)(1 << 26))) return false;
            cv[c] = std::llround(cw);
            tot += (ld)std::llabs(cv[c]);
            if (!(tot < (ld)(1 << 26) - 64)) return false;  // key = ((D_a << 8) + D_b) << 5 | tag
        }
        return true;
    };
    // margin in key units at scale u (the integers already in vv / cv)
    auto t2_at = [&](ld u, long long (*vv)[kSlots], const long long *cv) -> ld {
        ld tmax = 0;
        for (int c = 0; c < nc; ++c) {
            ld q = std::fabs((ld)cv[c] - w[c][9] / u);  // constant rounding, <= 1/2
            for (int s = 0; s < kSlots; ++s)
                if (kSlotW[s] >= 0) q += kSlotFmax[s] * std::fabs((ld)vv[c][s] - w[c][kSlotW[s]] * kSlotScale[s] / u);
            // weight + constant rounding (exact integer arithmetic otherwise) + reference chain + long-double slack
            const ld t = (u * q + refb[c] + psd[c] + 1e-15L * mag * 16) * 1.001L + u * 1e-6L;
            tmax = std::fmax(tmax, t);
        }
        return std::ceil(2 * tmax / u) + 1;
    };
    ld u0 = vmax / 32639;
    for (int attempt = 0;; ++attempt) {
        if (attempt > 60) return false;
        if (fits_at(u0, v, cc)) break;
        u0 *= 2;
    }
    ld best_u = u0, t2 = t2_at(u0, v, cc);
    {
        long long vv[MPX_MAX_CLASSES][kSlots], cv[MPX_MAX_CLASSES];
        for (int k = 1; k < 64; ++k) {
            const ld u = u0 * (1 + (ld)k / 256);
            if (!fits_at(u, vv, cv)) continue;
            const ld t = t2_at(u, vv, cv);
            if (t * u < t2 * best_u) {
                best_u = u;
                t2 = t;
                std::memcpy(v, vv, sizeof(v));
                std::memcpy(cc, cv, sizeof(cc));
            }
        }
    }
    if (!(t2 < (ld)(1 << 24))) return false;  // nothing would ever be decided
    ip.T2 = (int32_t)t2;
    for (int c = 0; c < MPX_MAX_CLASSES; ++c) {
        for (int hf = 0; hf < 2; ++hf) {
            uint64_t pa = 0, pb = 0;
            for (int j = 0; j < 8; ++j) {
                const int s = 8 * hf + j;
                long long a8 = 0, b8 = 0;
                if (c < nc) {
                    const long long x = v[c][s];
                    a8 = (x + 128) >> 8;  // floor: x = 256 a + b with b in [-128, 127]
                    b8 = x - 256 * a8;
                }
                pa |= (uint64_t)(uint8_t)(int8_t)a8 << (8 * j);
                pb |= (uint64_t)(uint8_t)(int8_t)b8 << (8 * j);
            }
            ip.a[c][hf] = pa;
            ip.b[c][hf] = pb;
        }
        ip.c[c] = c < nc ? (int32_t)cc[c] : (1 << 26) - 64;  // above every real key: never the argmin
    }
    return true;
}

// x rounded to the nearest f16 (ties to even); 0 below the normal range (the
// kernel sees no f16 subnormals) and false on overflow
bool f16_round(ld x, ld &r, uint16_t &bits) {
    r = 0;
    bits = 0;
    if (x == 0) return true;
    const ld a = std::fabs(x);
    int ex;
    std::frexp(a, &ex);  // a = f 2^ex, f in [0.5, 1): normal f16 exponent E = ex - 1
    if (ex - 1 < -14) return true;
    const ld quantum = std::ldexp((ld)1, ex - 11);
    ld m = std::nearbyint(a / quantum) * quantum;
    std::frexp(m, &ex);
    if (!(m <= (ld)65504)) return false;
    const int E = ex - 1;
    const uint32_t mant = (uint32_t)std::llround((m / std::ldexp((ld)1, E) - 1) * 1024);
    bits = (uint16_t)(((x < 0) ? 0x8000u : 0u) | ((uint32_t)(E + 15) << 10) | mant);
    r = x < 0 ? -m : m;
    return true;
}

// f16 limbs for MFMA16 (see the kernel): every expanded weight times a common
// power of two 2^e (the largest in [2^13, 2^14)) as hi + lo f16. The bound per
// class, in scaled units: the limb rounding against the exact weight (per
// unit of feature: 16384 for the h slots, 4 for the l slots, which take hi
// only, 128 for the channels), the fp32 accumulator's rounding as any sum of
// 25 terms (24 exact products + the constant) with unit roundoff 2^-23 (twice
// RNE's: covers any internal order and a truncating adder), the constant's
// own fp32 rounding, and the reference fp64 chain's error.
bool build_half(int nc, const double *mu, const double *inv, HalfParams &hp) {
    ld w[MPX_MAX_CLASSES][kFeat], refb[MPX_MAX_CLASSES], psd[MPX_MAX_CLASSES];
    if (!expand_classes(nc, mu, inv, w, refb, psd)) return false;
    ld wmax = 0, mag = 0;
    for (int c = 0; c < nc; ++c)
        for (int k = 0; k < kFeat; ++k) {
            if (k < 9) wmax = std::fmax(wmax, std::fabs(w[c][k]));
            mag = std::fmax(mag, std::fabs(w[c][k]) * kPhiMax[k]);
        }
    if (!(wmax > 0) || !(mag < 1e30L)) return false;
    int ex;
    std::frexp(wmax, &ex);
    const ld scale = std::ldexp((ld)1, 14 - ex);  // wmax * scale in [2^13, 2^14)
    // expanded weight of each quadratic slot j (rr gg bb rb rg bg) and its feature bound
    constexpr int kQuad[6] = {0, 1, 2, 4, 3, 5};
    const ld u = std::ldexp((ld)1, -23);
    const ld g25 = 25 * u / (1 - 25 * u);
    ld hi[MPX_MAX_CLASSES][9], lo[MPX_MAX_CLASSES][9];
    uint16_t hb[MPX_MAX_CLASSES][9], lb[MPX_MAX_CLASSES][9];
    ld base_tol[MPX_MAX_CLASSES], base_abs[MPX_MAX_CLASSES];
    for (int c = 0; c < nc; ++c) {
        ld rep = 0, abs_terms = 0;
        for (int k = 0; k < 9; ++k) {
            const ld x = w[c][k] * scale;
            if (!f16_round(x, hi[c][k], hb[c][k])) return false;
            if (!f16_round(x - hi[c][k], lo[c][k], lb[c][k])) return false;
            const ld dev = std::fabs(hi[c][k] + lo[c][k] - x);
            if (k < 6) {
                rep += dev * 16384 + std::fabs(lo[c][k]) * 4;
                abs_terms += (std::fabs(hi[c][k]) + std::fabs(lo[c][k])) * 16384 + std::fabs(hi[c][k]) * 4;
            } else {
                rep += dev * 128;
                abs_terms += (std::fabs(hi[c][k]) + std::fabs(lo[c][k])) * 128;
            }
        }
        base_tol[c] = rep + (refb[c] + psd[c] + 1e-15L * mag) * scale;
        base_abs[c] = abs_terms;
    }
    // the accumulator input of class c with a positivity bias, and its bound
    auto tol = [&](int c, ld bias, float *cout) -> ld {
        const ld cx = w[c][9] * scale + bias;
        const float cf = (float)cx;
        if (cout) *cout = cf;
        const ld acc = g25 * (base_abs[c] + std::fabs((ld)cf));
        return (base_tol[c] + acc + std::fabs((ld)cf - cx)) * 1.001L + 1e-30L;
    };
    ld tmax0 = 0;
    for (int c = 0; c < nc; ++c) tmax0 = std::fmax(tmax0, tol(c, 0, nullptr));
    const ld bias = 4 * tmax0;
    ld tmax = 0;
    for (int c = 0; c < nc; ++c) tmax = std::fmax(tmax, tol(c, bias, &hp.c[c]));
    if (!(bias > 2 * tmax)) return false;
    if (!(mag * scale + bias < 1e37L)) return false;
    for (int c = nc; c < MPX_MAX_CLASSES; ++c) hp.c[c] = 3.0e38f;
    std::memset(hp.w, 0, sizeof(hp.w));
    for (int c = 0; c < nc; ++c) {
        uint16_t e[kHalfMfmas][8];
        for (int j = 0; j < 6; ++j) {
            e[0][j] = hb[c][kQuad[j]];  // B1: h slots x hi
            e[1][j] = lb[c][kQuad[j]];  // B1: h slots x lo
            e[2][j] = hb[c][kQuad[j]];  // B3: l slots x hi
        }
        e[0][6] = hb[c][6];  // B1: r, g (hi)
        e[0][7] = hb[c][7];
        e[1][6] = lb[c][6];  // B1: r, g (lo)
        e[1][7] = lb[c][7];
        e[2][6] = hb[c][8];  // B3: b, b (hi, lo)
        e[2][7] = lb[c][8];
        for (int j = 0; j < kHalfMfmas; ++j)
            for (int d = 0; d < 4; ++d)
                hp.w[c / 16][j][c % 16][d] = (uint32_t)e[j][2 * d] | ((uint32_t)e[j][2 * d + 1] << 16);
    }
    const ld t2x = 2 * tmax * (1 + std::ldexp((ld)1, -20));  // see decided()
    float t2 = (float)t2x;
    if ((ld)t2 < t2x) t2 = std::nextafter(t2, INFINITY);
    hp.T2 = t2;
    return true;
}
}  // namespace

// Paths other than MFMA8 under AUTO: FAST32, or DIRECT when no decision bound
// can be proven for these statistics. The fp32 MFMA form (MFMA) never wins:
// the f32 MFMA and the f32 VALU share one datapath on gfx950 —
// SQ_VALU_MFMA_BUSY_CYCLES and the VALU issue cycles ADD UP to the kernel time
// (nc = 4: 132 vs 546 us, nc = 32: 677 vs 689 us at 8192^2;
// profiles/lab3_classify.md).
int classify_choose(int nc, int path, bool fast_ok) {
    (void)nc;
    if (path == MPX_CLS_DIRECT || !fast_ok) return MPX_CLS_DIRECT;
    if (path == MPX_CLS_AUTO) return MPX_CLS_FAST;
    return path;
}

// AUTO: MFMA16 from 4 classes, FAST32 below, each where its statistics
// permit a bound (else FAST32, then DIRECT). Round 6, 8192^2, three rotated
// images, host marshalling included, median µs of three alternated rounds on
// one box (profiles/raw/r6/lab3/, profiles/lab3_classify.md):
//   nc        1    2    3    4    5    8    12   16   24   32
//   mfma16   118  113  122  121  125  141  158  174  251  286
//   mfma8    110  112  116  120  146  176  232  277  322  392
//   fast      97  106  117  127  146  187  237  297  415  531
// A second box (profiles/raw/r6/inwave/) ordered fast32 / mfma16 the same
// way at 1-4 classes (99 / 131, 104 / 117, 116 / 121, 125 / 120). Below 4
// classes FAST32 needs no fix-up launch and no MFMA; from 4 MFMA16 wins, by
// 14-46 % from 5. MFMA8 never wins by more than the spread of its
// neighbours, so AUTO does not take it (explicit "mfma8" still runs it).
constexpr int kAutoMfma16MinClasses = 4;
constexpr int kMfma8sMaxClasses = 13;

// The path AUTO (or an explicit path) resolves to for these statistics, with
// the parameters it needs built; DIRECT when no fp32 / int bound exists.
int classify_resolve_uncached(int nc, const double *mu, const double *inv, int path, bool aligned, FastParams &fp,
                              Fast64Params &fp64, I8Params &ip8, HalfParams &hp);

// Resolved parameters of recent (statistics, path) pairs: a classifier is
// typically run many times with one set of class statistics (the benchmark
// loops, the slab models), and proving the int8 bound (a search over 256
// weight scales) costs ~1 ms of host time at 32 classes — more than the
// kernel. A small most-recently-used list keyed by the exact bytes.
struct ResolvedEntry {
    int nc = 0, path = 0, chosen = 0;
    bool aligned = false;
    double mu[MPX_MAX_CLASSES * 3], inv[MPX_MAX_CLASSES * 9];
    FastParams fp;
    Fast64Params fp64;
    I8Params ip8;
    HalfParams hp;
};

int classify_resolve(int nc, const double *mu, const double *inv, int path, bool aligned, FastParams &fp,
                     Fast64Params &fp64, I8Params &ip8, HalfParams &hp) {
    static std::mutex mtx;
    static std::vector<std::unique_ptr<ResolvedEntry>> cache;  // most recent first
    constexpr size_t kCap = 16;
    {
        std::lock_guard<std::mutex> lk(mtx);
        for (size_t i = 0; i < cache.size(); ++i) {
            const ResolvedEntry &e = *cache[i];
            if (e.nc == nc && e.path == path && e.aligned == aligned &&
                std::memcmp(e.mu, mu, sizeof(double) * 3 * nc) == 0 &&
                std::memcmp(e.inv, inv, sizeof(double) * 9 * nc) == 0) {
                fp = e.fp;
                fp64 = e.fp64;
                ip8 = e.ip8;
                hp = e.hp;
                const int chosen = e.chosen;
                std::rotate(cache.begin(), cache.begin() + (std::ptrdiff_t)i, cache.begin() + (std::ptrdiff_t)i + 1);
                return chosen;
            }
        }
    }
    auto e = std::make_unique<ResolvedEntry>();
    const int chosen = classify_resolve_uncached(nc, mu, inv, path, aligned, e->fp, e->fp64, e->ip8, e->hp);
    e->nc = nc;
    e->path = path;
    e->aligned = aligned;
    e->chosen = chosen;
    std::memcpy(e->mu, mu, sizeof(double) * 3 * nc);
    std::memcpy(e->inv, inv, sizeof(double) * 9 * nc);
    fp = e->fp;
    fp64 = e->fp64;
    ip8 = e->ip8;
    hp = e->hp;
    std::lock_guard<std::mutex> lk(mtx);
    cache.insert(cache.begin(), std::move(e));
    if (cache.size() > kCap) cache.pop_back();
    return chosen;
}

int classify_resolve_uncached(int nc, const double *mu, const double *inv, int path, bool aligned, FastParams &fp,
                              Fast64Params &fp64, I8Params &ip8, HalfParams &hp) {
    if (path == MPX_CLS_DIRECT || !aligned) return MPX_CLS_DIRECT;
    // mfma8 re-ranks its undecided pixels in fp32 first: its FastParams too
    // (T2 = +inf when the fp32 bound cannot be proven: the fp64 chain then
    // takes every undecided pixel)
    auto fp_for_i8 = [&] {
        if (!build_fast(nc, mu, inv, fp)) fp.T2 = INFINITY;
    };
    if (path == MPX_CLS_AUTO && nc >= kAutoMfma16MinClasses && build_half(nc, mu, inv, hp)) {
        fp_for_i8();
        return MPX_CLS_MFMA16;
    }
    const bool ok = path == MPX_CLS_MFMA64   ? build_fast64(nc, mu, inv, fp64)
                    : path == MPX_CLS_MFMA8  ? build_i8(nc, mu, inv, ip8)
                    : path == MPX_CLS_MFMA16 ? build_half(nc, mu, inv, hp)
                                             : build_fast(nc, mu, inv, fp);
    if ((path == MPX_CLS_MFMA8 || path == MPX_CLS_MFMA16) && ok) fp_for_i8();
    return classify_choose(nc, path, ok);
}

// One device deferral list per (device, stream), allocated on first use and
// reset by the fix-up kernel itself (no memset launch per call). nullptr
// lists (allocation failed) fall back to the in-wave re-ranking.
DeferList defer_list(hipStream_t s, bool take) {
    static std::mutex mtx;
    static std::vector<std::tuple<int, hipStream_t, DeferList>> lists;
    constexpr uint32_t kCap = 4096;  // entries per sub-list (8 MiB in all); 4 pixels each
    int dev = 0;  // the stream's device (the image's), not necessarily the current one
    if (hipStreamGetDevice(s, &dev) != hipSuccess) {
        (void)hipGetLastError();
        return DeferList{nullptr, nullptr, 0, 0};
    }
    std::lock_guard<std::mutex> lk(mtx);
    for (auto &t : lists)
        if (std::get<0>(t) == dev && std::get<1>(t) == s) {
            DeferList &d = std::get<2>(t);
            // launches that use the list alternate counter sets: the fix-up of
            // one zeroes the set of the next (launches of one stream run in order)
            if (take) d.par ^= 1u;
            return d;
        }
    DeferList d{nullptr, nullptr, kCap, 0};
    int cur = 0;
    (void)hipGetDevice(&cur);
    if (cur != dev) (void)hipSetDevice(dev);
    struct Restore {
        int cur, dev;
        ~Restore() {
            if (cur != dev) (void)hipSetDevice(cur);
        }
    } restore{cur, dev};
    if (hipMalloc(&d.ent, sizeof(uint64_t) * kCap * kDeferSubs) != hipSuccess) {
        (void)hipGetLastError();
        return DeferList{nullptr, nullptr, 0, 0};
    }
    if (hipMalloc(&d.ctr, 2 * kDeferSubs * sizeof(uint32_t)) != hipSuccess ||
        hipMemsetAsync(d.ctr, 0, 2 * kDeferSubs * sizeof(uint32_t), s) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipFree(d.ent);
        return DeferList{nullptr, nullptr, 0, 0};
    }
    lists.emplace_back(dev, s, d);
    return d;
}

int classify_impl(uint32_t *img, int64_t npix, int nc, const double *mu, const double *inv, int grid, int block,
                  int path, uint32_t *amb, void *stream) {
    MPX_CHECK_ARG(npix >= 0, "npix must be >= 0");
    MPX_CHECK_ARG(nc >= 1 && nc <= MPX_MAX_CLASSES, "need 1 <= nc <= 32");
    MPX_CHECK_ARG(mu && inv, "null class parameters");
    MPX_CHECK_ARG(grid >= 0 && block >= 0 && block <= 1024, "bad launch geometry");
    MPX_CHECK_ARG(path >= MPX_CLS_DIRECT && path <= MPX_CLS_MFMA16, "bad path");
    if (npix == 0) return MPX_OK;
    MPX_CHECK_ARG(img, "null image");
    ClassParams cp{};
    for (int i = 0; i < 3 * nc; ++i) cp.mu[i] = mu[i];
    for (int i = 0; i < 9 * nc; ++i) cp.A[i] = inv[i];
    hipStream_t s = as_stream(stream);
    FastParams fp;
    Fast64Params fp64;
    I8Params ip8;
    HalfParams hp;
    const int chosen = classify_resolve(nc, mu, inv, path, aligned16(img), fp, fp64, ip8, hp);
    int64_t done = 0;  // pixels handled by a fast path; the rest go DIRECT
    // MFMA8 up to kMfma8sMaxClasses: the one-pixel-per-lane 4x4x4 form (MFMA8S)
    if (chosen == MPX_CLS_MFMA8 && nc <= kMfma8sMaxClasses) {
        const int64_t nvec = npix / 4;
        if (nvec > 0) {
            const int64_t blocks = (nvec + 255) / 256;
            // at most 16 blocks per CU (two resident rounds at 8 waves per SIMD,
            // 16 trips per thread at 8192^2): more, shorter-lived workgroups
            // balance the load across CUs, and fewer trips per thread keep less
            // store latency on each wave's critical path (gfx950 stores count
            // in vmcnt with the loads). 8192^2, µs, 8 -> 16 blocks per CU:
            // nc = 2 126-129 -> 118, nc = 4 133-135 -> 128-130, nc = 8 same
            // (profiles/lab3_classify.md)
            const int g = grid > 0 ? (int)useful_grid(grid, nvec, 256)
                                   : (int)std::min<int64_t>(blocks, (int64_t)kNumCUs * 16);
            const int ns = (nc + 1) / 2;
#define MPX_MFMA8S(NS) \
    hipLaunchKernelGGL((classify_mfma8s_kernel<NS>), dim3(g), dim3(256), 0, s, img, nvec, nc, cp, ip8, fp, amb)
            if (ns == 1)
                MPX_MFMA8S(1);
            else if (ns == 2)
                MPX_MFMA8S(2);
            else if (ns == 3)
                MPX_MFMA8S(3);
            else if (ns == 4)
                MPX_MFMA8S(4);
            else if (ns == 5)
                MPX_MFMA8S(5);
            else if (ns == 6)
                MPX_MFMA8S(6);
            else
                MPX_MFMA8S(7);
#undef MPX_MFMA8S
            MPX_RETURN_IF_HIP_ERROR(hipGetLastError());
            done = nvec * 4;
        }
    } else if (chosen == MPX_CLS_MFMA16) {
        const int64_t nvec = npix / 4;
        if (nvec > 0) {
            const int64_t blocks = (nvec + 255) / 256;
            const int g = grid > 0 ? (int)useful_grid(grid, nvec, 256) : (int)std::min<int64_t>(blocks, (int64_t)kNumCUs * 16);
            // registers ranked in the last 16-class set: an even count (padded classes never win)
            const int last = nc > 16 ? nc - 16 : nc;
            // a caller geometry (the harness's launch sweeps) drives the looped
            // kernel over the whole image; by default whole blocks go one-shot
            const int64_t want = grid > 0 ? 0 : nvec / (256 * kM16Trips);
            const DeferList dl = want > 0 ? defer_list(s, true) : DeferList{nullptr, nullptr, 0, 0};
            const int64_t nblk = dl.ent != nullptr ? want : 0;
            const int64_t vdone = nblk * 256 * kM16Trips;
            uint32_t *rimg = img + 4 * vdone;
            const int64_t rvec = nvec - vdone;
            const int gr = (int)std::min<int64_t>((rvec + 255) / 256, g);
            const DeferList none{nullptr, nullptr, 0, 0};
#define MPX_MFMA16(NSET, NR)                                                                                          \
    do {                                                                                                              \
        if (nblk > 0)                                                                                                 \
            hipLaunchKernelGGL((classify_mfma16t_kernel<NSET, NR>), dim3((unsigned)nblk), dim3(256), 0, s, img, nc, cp, \
                               hp, fp, dl, amb);                                                                      \
        if (rvec > 0)                                                                                                 \
            hipLaunchKernelGGL((classify_mfma16_kernel<NSET, NR>), dim3(gr), dim3(256), 0, s, rimg, rvec, nc, cp, hp, \
                               fp, none, amb);                                                                        \
    } while (0)
            if (nc <= 16) {
                switch ((last + 1) / 2) {
                    case 1: MPX_MFMA16(1, 2); break;
                    case 2: MPX_MFMA16(1, 4); break;
                    case 3: MPX_MFMA16(1, 6); break;
                    case 4: MPX_MFMA16(1, 8); break;
                    case 5: MPX_MFMA16(1, 10); break;
                    case 6: MPX_MFMA16(1, 12); break;
                    case 7: MPX_MFMA16(1, 14); break;
                    default: MPX_MFMA16(1, 16); break;
                }
            } else if (last <= 4) {
                MPX_MFMA16(2, 4);
            } else if (last <= 8) {
                MPX_MFMA16(2, 8);
            } else if (last <= 12) {
                MPX_MFMA16(2, 12);
            } else {
                MPX_MFMA16(2, 16);
            }
#undef MPX_MFMA16
            MPX_RETURN_IF_HIP_ERROR(hipGetLastError());
            if (nblk > 0) {
                hipLaunchKernelGGL(classify_fixup_kernel, dim3(kDeferSubs), dim3(256), 0, s, img, dl, nc, cp, fp, amb);
                MPX_RETURN_IF_HIP_ERROR(hipGetLastError());
            }
            done = nvec * 4;
        }
    } else if (chosen == MPX_CLS_MFMA8) {
        const int64_t nchunks = npix / 128;
        if (nchunks > 0) {
            const int64_t blocks = (nchunks + 3) / 4;
            // 16 blocks per CU (round-5 sweep at 8192^2, 2048 -> 4096 blocks:
            // nc = 12 269.5 -> 261.1 µs, 16 269.7 -> 262.7, 32 391.1 -> 375.2;
            // 8192 and 16384 slower again; profiles/lab3_classify.md)
            const int g = grid > 0 ? grid : (int)std::min<int64_t>(blocks, (int64_t)kNumCUs * 16);
#define MPX_MFMA8_LAUNCH(NREG) \
    hipLaunchKernelGGL((classify_mfma8_kernel<NREG>), dim3(g), dim3(256), 0, s, img, nchunks, nc, cp, ip8, fp, amb)
            if (nc <= 8)
                MPX_MFMA8_LAUNCH(4);
            else if (nc <= 16)
                MPX_MFMA8_LAUNCH(8);
            else if (nc <= 24)  // registers 0-11 hold classes 0-23
                MPX_MFMA8_LAUNCH(12);
            else
                MPX_MFMA8_LAUNCH(16);
#undef MPX_MFMA8_LAUNCH
            MPX_RETURN_IF_HIP_ERROR(hipGetLastError());
            done = nchunks * 128;
        }
    } else if (chosen == MPX_CLS_MFMA64) {
        const int64_t nchunks = npix / 64;
        if (nchunks > 0) {
            const int64_t blocks = (nchunks + 3) / 4;
            const int g = grid > 0 ? grid : (int)std::min<int64_t>(blocks, (int64_t)kNumCUs * 8);
            if (nc <= 16)
                hipLaunchKernelGGL(classify_mfma64_kernel<1>, dim3(g), dim3(256), 0, s, img, nchunks, nc, cp, fp64,
                                   amb);
            else
                hipLaunchKernelGGL(classify_mfma64_kernel<2>, dim3(g), dim3(256), 0, s, img, nchunks, nc, cp, fp64,
                                   amb);
            MPX_RETURN_IF_HIP_ERROR(hipGetLastError());
            done = nchunks * 64;
        }
    } else if (chosen == MPX_CLS_MFMA) {
        const int64_t nchunks = npix / 128;
        if (nchunks > 0) {
            const int64_t blocks = (nchunks + 3) / 4;
            const int g = grid > 0 ? grid : (int)std::min<int64_t>(blocks, (int64_t)kNumCUs * 8);
            if (nc <= 16)
                hipLaunchKernelGGL(classify_mfma32_kernel<8>, dim3(g), dim3(256), 0, s, img, nchunks, nc, cp, fp, amb);
            else
                hipLaunchKernelGGL(classify_mfma32_kernel<16>, dim3(g), dim3(256), 0, s, img, nchunks, nc, cp, fp,
                                   amb);
            MPX_RETURN_IF_HIP_ERROR(hipGetLastError());
            done = nchunks * 128;
        }
    } else if (chosen == MPX_CLS_FAST) {
        const int64_t nvec = npix / (4 * kFastNQ);
        if (nvec > 0) {
            // the kernel is compiled for 256-thread workgroups
            // (__launch_bounds__(256)): a larger caller block would not launch
            // ("unspecified launch failure"), so it is capped
            const int blk = block > 0 ? std::min(block, 256) : 256;
            const int64_t blocks = (nvec + blk - 1) / blk;
            // 32 blocks per CU (round-5 sweep at 8192^2, 2048 -> 8192 blocks:
            // nc = 12 285.6 -> 247.4 µs, 16 297.9 -> 288.2, 32 524.4 -> 504.9;
            // profiles/lab3_classify.md)
            const int g = grid > 0 ? (int)useful_grid(grid, nvec, blk) : (int)std::min<int64_t>(blocks, (int64_t)kNumCUs * 32);
            hipLaunchKernelGGL(classify_fast32_kernel, dim3(g), dim3(blk), 0, s, img, nvec, nc, cp, fp, amb);
            MPX_RETURN_IF_HIP_ERROR(hipGetLastError());
            done = nvec * 4 * kFastNQ;
        }
    }
    if (done < npix) {
        uint32_t *rest = img + done;
        const int64_t n = npix - done;
        const int vec = aligned16(rest) ? 1 : 0;
        int blk = block > 0 ? block : 256;
        int g = grid;
        if (g == 0 || chosen != MPX_CLS_DIRECT) {
            int64_t want = (n / 4 + blk - 1) / blk;
            g = (int)std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)kNumCUs * 8));
        } else {
            // caller geometry: thread t handles vector t (or pixel t) and tail pixel t
            g = (int)useful_grid(g, vec ? std::max<int64_t>(n / 4, 4) : n, blk);
        }
        hipLaunchKernelGGL(classify_direct_kernel, dim3(g), dim3(blk), 0, s, rest, n, nc, cp, vec);
        MPX_RETURN_IF_HIP_ERROR(hipGetLastError());
    }
    return MPX_OK;
}

int classify_plan_impl(int nc, const double *mu, const double *inv, int path, float *margin) {
    MPX_CHECK_ARG(nc >= 1 && nc <= MPX_MAX_CLASSES, "need 1 <= nc <= 32");
    MPX_CHECK_ARG(mu && inv, "null class parameters");
    MPX_CHECK_ARG(path >= MPX_CLS_DIRECT && path <= MPX_CLS_MFMA16, "bad path");
    FastParams fp;
    Fast64Params fp64;
    I8Params ip8;
    HalfParams hp;
    const int chosen = classify_resolve(nc, mu, inv, path, true, fp, fp64, ip8, hp);
    if (margin)
        *margin = chosen == MPX_CLS_MFMA8    ? (float)ip8.T2  // in key units
                  : chosen == MPX_CLS_MFMA16 ? hp.T2
                  : chosen == MPX_CLS_MFMA64 ? (float)fp64.T2
                  : chosen == MPX_CLS_DIRECT ? 0.0f
                                             : fp.T2;
    return chosen;
}

MPX_MODULE_ANCHOR(classify)

}  // namespace mpx

extern "C" int mpx_classify(uint32_t *img, int64_t npix, int nc, const double *mu, const double *inv, int grid,
                            int block, int path, void *stream) {
    return mpx::classify_impl(img, npix, nc, mu, inv, grid, block, path, nullptr, stream);
}

extern "C" int mpx_classify_ex(uint32_t *img, int64_t npix, int nc, const double *mu, const double *inv, int grid,
                               int block, int path, uint32_t *ambiguous, void *stream) {
    return mpx::classify_impl(img, npix, nc, mu, inv, grid, block, path, ambiguous, stream);
}

// Host-side export of the MFMA8 integer weights (tests emulate the kernel's
// exact integer arithmetic on the CPU): a, b = [32][16] int8 limbs by slot,
// c = [32] accumulator constants, *t2 = decision margin in key units.
extern "C" int mpx_classify_i8_params(int nc, const double *mu, const double *inv, int8_t *a, int8_t *b, int32_t *c,
                                      int32_t *t2) {
    MPX_CHECK_ARG(nc >= 1 && nc <= MPX_MAX_CLASSES && mu && inv && a && b && c && t2, "bad arguments");
    mpx::I8Params ip;
    if (!mpx::build_i8(nc, mu, inv, ip)) return MPX_ERR_UNSUPPORTED;
    for (int k = 0; k < MPX_MAX_CLASSES; ++k) {
        for (int s = 0; s < 16; ++s) {
            a[16 * k + s] = (int8_t)(uint8_t)(ip.a[k][s / 8] >> (8 * (s % 8)));
            b[16 * k + s] = (int8_t)(uint8_t)(ip.b[k][s / 8] >> (8 * (s % 8)));
        }
        c[k] = ip.c[k];
    }
    *t2 = ip.T2;
    return MPX_OK;
}

extern "C" int mpx_classify_plan(int nc, const double *mu, const double *inv, int path, float *margin) {
    return mpx::classify_plan_impl(nc, mu, inv, path, margin);
}

// Host-side export of the MFMA16 f16 weights (tests emulate the kernel on the
// CPU): w = [32 classes][3 MFMAs][8 slots] f16 bit patterns, c = [32] fp32
// accumulator inputs, *t2 = decision margin (the FAST32 test, scaled units).
extern "C" int mpx_classify_f16_params(int nc, const double *mu, const double *inv, uint16_t *w, float *c,
                                       float *t2) {
    MPX_CHECK_ARG(nc >= 1 && nc <= MPX_MAX_CLASSES && mu && inv && w && c && t2, "bad arguments");
    mpx::HalfParams hp;
    if (!mpx::build_half(nc, mu, inv, hp)) return MPX_ERR_UNSUPPORTED;
    for (int k = 0; k < MPX_MAX_CLASSES; ++k) {
        for (int j = 0; j < mpx::kHalfMfmas; ++j)
            for (int s = 0; s < 8; ++s) w[(k * mpx::kHalfMfmas + j) * 8 + s] = (uint16_t)(hp.w[k / 16][j][k % 16][s / 2] >> (16 * (s % 2)));
        c[k] = hp.c[k];
    }
    *t2 = hp.T2;
    return MPX_OK;
}
