// lab3 classifier, the floating-point distance GEMMs with several pixels per
// lane group: MFMA32 (fp32) and MFMA64 (fp64). Explicit paths only.
#pragma once

#include "classify_rank.hpp"

namespace mpx {
namespace {

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

}  // namespace
}  // namespace mpx
