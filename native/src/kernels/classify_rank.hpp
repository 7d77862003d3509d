// lab3 classifier, device ranking primitives shared by the kernel families:
// the reference fp64 chain, 32-bit keys and their running top-2, the proven
// fp32 decision test, and the per-wave re-ranking of deferred pixels.
#pragma once

#include "classify_params.hpp"
#include "internal.hpp"

namespace mpx {
namespace {

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

// The deferred list of the one-pixel-per-lane kernels (MFMA8S, looped MFMA16)
// holds one entry per (lane, trip) with any undecided pixel: the 16-B vector
// index and a 4-bit mask of its undecided pixels — one append per trip
// instead of one per pixel (with ~0.4% of the pixels undecided at nc = 4, a
// quarter of the trips have one). The pixels are re-read from the image after
// the loop: their RGB bytes are untouched.
// Every list is private to one wave (its own LDS rows and counters): a wave
// appends, then ranks its own deferred pixels, in program order — LDS
// operations of one wave execute in order — so the kernel has no block
// barrier, and short-lived workgroups cost no more than long ones.
constexpr int kAmb8sCapW = 256;   // deferred (vector, mask) entries per wave
constexpr int kAmb8sCap2W = 64;   // pixels the fp32 stage leaves to the fp64 chain, per wave

// Wave w's deferred pixels (its rows of the kernel's LDS lists): the fp32
// proven-margin ranking first, the exact fp64 chain for what it leaves
// (every lane of the wave busy in each stage); the wave's appends in its loop
// precede these reads in program order. (The per-trip append stays a copy in
// each kernel: through a helper it changed classify_mfma8s_kernel's registers.)
__device__ __forceinline__ void rerank_wave_list(uint32_t *__restrict__ img, int lane, int w,
                                                 int64_t (&s_amb)[4][kAmb8sCapW], uint32_t (&s_namb)[4],
                                                 uint32_t (&s_npx)[4], int64_t (&s_amb2)[4][kAmb8sCap2W],
                                                 uint32_t (&s_ambpx2)[4][kAmb8sCap2W], uint32_t (&s_namb2)[4], int nc,
                                                 const ClassParams &cp, const FastParams &fp, uint32_t *amb) {
    uint4 *v = reinterpret_cast<uint4 *>(img);
    __builtin_amdgcn_wave_barrier();
    const uint32_t nd = min(s_namb[w], (uint32_t)kAmb8sCapW);
    for (uint32_t j = lane; j < nd; j += 64) {
        const int64_t e = s_amb[w][j];
        const int64_t vi = e >> 4;
        const uint32_t mask = (uint32_t)e & 15u;
        atomicAdd(&s_npx[w], (uint32_t)__popc(mask));
        const uint4 q = v[vi];  // a vector this wave wrote in its loop, in program order
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

}  // namespace
}  // namespace mpx
