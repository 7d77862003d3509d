// lab3 classifier, the VALU kernels: DIRECT (the reference fp64 chain) and
// FAST32 (packed fp32 with the proven margin).
#pragma once

#include "classify_rank.hpp"

namespace mpx {
namespace {

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

}  // namespace
}  // namespace mpx
