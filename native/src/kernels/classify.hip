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
//
// This file: launch code and C entry points. Kernels: classify_fast32.hpp
// (DIRECT, FAST32), _mfma32.hpp (MFMA32, MFMA64), _mfma8.hpp (MFMA8, MFMA8S),
// _mfma16.hpp (MFMA16, fix-up) over classify_rank.hpp's device primitives;
// the margins are proven on the host in native/src/core/classify_bounds.cpp.
#include <algorithm>
#include <mutex>
#include <tuple>
#include <vector>

#include "classify_bounds.hpp"
#include "classify_fast32.hpp"
#include "classify_mfma16.hpp"
#include "classify_mfma32.hpp"
#include "classify_mfma8.hpp"

namespace mpx {

// One device deferral list per (device, stream), allocated on first use and
// reset by the fix-up kernel itself (no memset launch per call). Every call
// takes the next counter parity. nullptr lists (allocation failed) send the
// whole image through the looped kernel's in-wave re-ranking.
DeferList defer_list(hipStream_t s) {
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
            d.par ^= 1u;
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
    const Resolved rs = classify_resolve(nc, mu, inv, path, aligned16(img));
    const int chosen = rs.chosen;
    const FastParams &fp = rs.fp;
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
            // <NS>: row sets of two classes
            static const decltype(&classify_mfma8s_kernel<1>) kern[7] = {
                classify_mfma8s_kernel<1>, classify_mfma8s_kernel<2>, classify_mfma8s_kernel<3>, classify_mfma8s_kernel<4>,
                classify_mfma8s_kernel<5>, classify_mfma8s_kernel<6>, classify_mfma8s_kernel<7>};
            hipLaunchKernelGGL(kern[(nc + 1) / 2 - 1], dim3(g), dim3(256), 0, s, img, nvec, nc, cp, rs.ip8, fp, amb);
            MPX_RETURN_IF_HIP_ERROR(hipGetLastError());
            done = nvec * 4;
        }
    } else if (chosen == MPX_CLS_MFMA16) {
        const int64_t nvec = npix / 4;
        if (nvec > 0) {
            const int64_t blocks = (nvec + 255) / 256;
            const int g = grid > 0 ? (int)useful_grid(grid, nvec, 256) : (int)std::min<int64_t>(blocks, (int64_t)kNumCUs * 16);
            // <NSET, NR>: NR registers ranked in the last 16-class set (even; from 17 classes a multiple of 4: padding never wins)
#define MPX_M16_KERNELS(K) \
    {K<1, 2>, K<1, 4>, K<1, 6>, K<1, 8>, K<1, 10>, K<1, 12>, K<1, 14>, K<1, 16>, K<2, 4>, K<2, 8>, K<2, 12>, K<2, 16>}
            static const decltype(&classify_mfma16t_kernel<1, 2>) oneshot[12] = MPX_M16_KERNELS(classify_mfma16t_kernel);
            static const decltype(&classify_mfma16_kernel<1, 2>) looped[12] = MPX_M16_KERNELS(classify_mfma16_kernel);
#undef MPX_M16_KERNELS
            const int ki = nc <= 16 ? (nc + 1) / 2 - 1 : 8 + (nc - 16 + 3) / 4 - 1;
            // a caller geometry (the harness's launch sweeps) drives the looped
            // kernel over the whole image; by default whole blocks go one-shot
            const int64_t want = grid > 0 ? 0 : nvec / (256 * kM16Trips);
            const DeferList dl = want > 0 ? defer_list(s) : DeferList{nullptr, nullptr, 0, 0};
            const int64_t nblk = dl.ent != nullptr ? want : 0;
            const int64_t vdone = nblk * 256 * kM16Trips;
            uint32_t *rimg = img + 4 * vdone;
            const int64_t rvec = nvec - vdone;
            const int gr = (int)std::min<int64_t>((rvec + 255) / 256, g);
            if (nblk > 0)
                hipLaunchKernelGGL(oneshot[ki], dim3((unsigned)nblk), dim3(256), 0, s, img, nc, cp, rs.hp, fp, dl, amb);
            if (rvec > 0) hipLaunchKernelGGL(looped[ki], dim3(gr), dim3(256), 0, s, rimg, rvec, nc, cp, rs.hp, fp, amb);
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
            // 16 blocks per CU (round-5 sweep at 8192^2, 2048 -> 4096 blocks:
            // nc = 12 269.5 -> 261.1 µs, 16 269.7 -> 262.7, 32 391.1 -> 375.2;
            // 8192 and 16384 slower again; profiles/lab3_classify.md)
            const int g = grid > 0 ? grid : (int)std::min<int64_t>((nchunks + 3) / 4, (int64_t)kNumCUs * 16);
            // <NREG>: accumulator registers with real classes, 4 per 8 classes (registers 0-11 hold classes 0-23)
            static const decltype(&classify_mfma8_kernel<4>) kern[4] = {
                classify_mfma8_kernel<4>, classify_mfma8_kernel<8>, classify_mfma8_kernel<12>, classify_mfma8_kernel<16>};
            hipLaunchKernelGGL(kern[(nc - 1) / 8], dim3(g), dim3(256), 0, s, img, nchunks, nc, cp, rs.ip8, fp, amb);
            MPX_RETURN_IF_HIP_ERROR(hipGetLastError());
            done = nchunks * 128;
        }
    } else if (chosen == MPX_CLS_MFMA64) {
        const int64_t nchunks = npix / 64;
        if (nchunks > 0) {
            const int g = grid > 0 ? grid : (int)std::min<int64_t>((nchunks + 3) / 4, (int64_t)kNumCUs * 8);
            const auto kern = nc <= 16 ? classify_mfma64_kernel<1> : classify_mfma64_kernel<2>;  // 16-class tiles
            hipLaunchKernelGGL(kern, dim3(g), dim3(256), 0, s, img, nchunks, nc, cp, rs.fp64, amb);
            MPX_RETURN_IF_HIP_ERROR(hipGetLastError());
            done = nchunks * 64;
        }
    } else if (chosen == MPX_CLS_MFMA) {
        const int64_t nchunks = npix / 128;
        if (nchunks > 0) {
            const int g = grid > 0 ? grid : (int)std::min<int64_t>((nchunks + 3) / 4, (int64_t)kNumCUs * 8);
            const auto kern = nc <= 16 ? classify_mfma32_kernel<8> : classify_mfma32_kernel<16>;
            hipLaunchKernelGGL(kern, dim3(g), dim3(256), 0, s, img, nchunks, nc, cp, fp, amb);
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
    const Resolved rs = classify_resolve(nc, mu, inv, path, true);
    if (margin) *margin = classify_margin(rs);
    return rs.chosen;
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
