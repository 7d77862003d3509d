// 3-D Jacobi sweep kernels (7-point stencil) shared by jacobi3d.hip (production
// launches) and native/tune/jacobi_variants.hip (mpx_jacobi3d_variant,
// libmpx_tune.so). The design notes are at the top of jacobi3d.hip; the wave
// helpers (DPP shifts, wave max, residual_max, kStripVec, kDrop) are those of
// the 2-D kernels in jacobi_wave.hpp.
#pragma once
#include "jacobi_wave.hpp"

#include <climits>
#include <limits>

namespace mpx {
namespace {

// launches with fewer waves than this shrink their tile (rows per wave of the
// rows form, planes per wave of the march form), as launch_jacobi does: four
// waves for each of the 1024 SIMDs, one round at the occupancy of the fattest
// instantiations. A 3-D wave lives for a whole tile, not 8 rows, so the 2-D
// launcher's 16384 is not needed to even out the tail.
constexpr int kJ3MinWaves = 4096;
constexpr int kJ3Rows = 16;  // rows per block of the per-lane kernel

// s of the contract: ((((zm + zp) + (ym + yp)) + (xm + xp)) [+ b]) * (T)(1.0 / 6.0),
// each operation rounded (the tree builds with -ffp-contract=off)
template <typename T, bool RHS>
__device__ __forceinline__ T j3_value(T zm, T zp, T ym, T yp, T xm, T xp, T b) {
    const T n = ((zm + zp) + (ym + yp)) + (xm + xp);
    if constexpr (RHS) return (n + b) * (T)(1.0 / 6.0);
    else return n * (T)(1.0 / 6.0);
}

// REMAP: workgroups that are neighbours in the launch order (adjacent strips,
// row tiles, planes: the ones that re-read each other's rows) run on one XCD
// and meet in its L2, instead of round-robin over the eight (internal.hpp)
template <bool REMAP>
__device__ __forceinline__ int j3_block() {
    if constexpr (REMAP) return xcd_remap((int)blockIdx.x, (int)gridDim.x);
    else return (int)blockIdx.x;
}

// block-uniform tail of the wave kernels: one conditional atomic per workgroup
template <typename T, int WPB>
__device__ __forceinline__ void j3_fold_residual(T rmax, T *resid) {
    using B = typename JVec<T>::bits;
    __shared__ T s_m[WPB];
    const T m = wave_max_dpp(rmax);
    if ((threadIdx.x & 63) == 0) s_m[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        T mm = s_m[0];
#pragma unroll
        for (int q = 1; q < WPB; ++q) mm = s_m[q] > mm ? s_m[q] : mm;
        if (mm > (T)0) residual_max(reinterpret_cast<B *>(resid), __builtin_bit_cast(B, mm));
    }
}

// ---------------------------------------------------------------------------
// per-lane kernel: any width and alignment. One element per lane, kJ3Rows rows
// of one plane per block; the seven loads go through the caches.
// ---------------------------------------------------------------------------
template <typename T, bool RHS, bool ACCEL>
__global__ __launch_bounds__(256) void jacobi3d_kernel(const T *__restrict__ u, const T *__restrict__ b,
                                                       T *__restrict__ un, int nx, int ny, int k0, int nxb, int nyb,
                                                       T omega, T *__restrict__ resid) {
    const unsigned bid = blockIdx.x;
    const int xb = (int)(bid % (unsigned)nxb);
    const unsigned t = bid / (unsigned)nxb;
    const int yb = (int)(t % (unsigned)nyb);
    const int64_t k = k0 + (int64_t)(t / (unsigned)nyb);
    const int x = xb * 256 + (int)threadIdx.x;
    const int64_t plane = (int64_t)ny * nx;
    const T *uc = u + k * plane;
    T *o = un + k * plane;
    T rmax = (T)0;
    if (x < nx) {
        const int y0 = yb * kJ3Rows, y1 = min(y0 + kJ3Rows, ny);
        const bool xin = x > 0 && x < nx - 1;
        for (int y = y0; y < y1; ++y) {
            const int64_t i = (int64_t)y * nx + x;
            const T c = uc[i];
            T out = c;
            if (xin && y > 0 && y < ny - 1) {
                T src = (T)0;
                if constexpr (RHS) src = b[k * plane + i];
                const T s = j3_value<T, RHS>(uc[i - plane], uc[i + plane], uc[i - nx], uc[i + nx], uc[i - 1], uc[i + 1],
                                             src);
                const T d = s > c ? s - c : c - s;
                rmax = d > rmax ? d : rmax;
                if constexpr (ACCEL) {
                    const T p = o[i];
                    const T df = s - p;
                    const T w = omega * df;
                    out = p + w;
                } else {
                    out = s;
                }
            }
            o[i] = out;
        }
    }
    if (resid) {
        using B = typename JVec<T>::bits;
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const T v = __shfl_xor(rmax, m);
            rmax = v > rmax ? v : rmax;
        }
        if ((threadIdx.x & 63) == 0 && rmax > (T)0)
            residual_max(reinterpret_cast<B *>(resid), __builtin_bit_cast(B, rmax));
    }
}

// ---------------------------------------------------------------------------
// wave form 0, "rows": the 2-D strip walk inside one plane. A wave owns a strip
// of 62 vectors and R rows [i0, i1) of plane k; the plane's rows ride in the
// 5-slot ring of the 2-D kernel (unconditional clamped prefetch three rows
// ahead, slots compile-time through the unroll by 5), and the rows of planes
// k - 1 and k + 1 at the same (y, x) come in as two more streams in rings
// indexed like the centre row. Three loads of u per point: the two re-reads
// are left to L2 / Infinity Cache (consecutive waves are adjacent strips, then
// row blocks, then planes, so neighbouring planes are in flight together).
// b and p (= un on entry) are read once, non-temporal, at centre rows only, p
// by the lanes that store it and before their store (jacobi_wave.hpp gives the
// in-place argument; it carries over row for row). Rows 0 and ny - 1 are walked
// too and copied through.
// ---------------------------------------------------------------------------
template <typename T, bool RHS, bool ACCEL, bool REMAP = false, int WPB = 4>
__global__ __launch_bounds__(64 * WPB) void jacobi3d_rows_kernel(const T *__restrict__ u, const T *__restrict__ b,
                                                                T *__restrict__ un, int nx, int ny, int k0, int strips,
                                                                int nrb, int R, int nwaves, T omega,
                                                                T *__restrict__ resid) {
    using V = typename JWide<T>::type;
    constexpr int NV = JVec<T>::n;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(j3_block<REMAP>() * WPB + (threadIdx.x >> 6));
    T rmax = (T)0;
    if (wave < nwaves) {
        const int strip = wave % strips;  // consecutive waves: adjacent strips of the same rows
        const int t = wave / strips;
        const int rb = t % nrb;
        const int64_t plane = (int64_t)ny * nx;
        const int64_t poff = (k0 + (int64_t)(t / nrb)) * plane;
        const int nvec = nx / NV;
        const int cv = strip * kStripVec - 1 + lane;  // this lane's column vector
        const bool out_lane = lane >= 1 && lane <= kStripVec && cv < nvec;
        const int cvc = min(max(cv, 0), nvec - 1);
        const int i0 = rb * R;
        const int i1 = min(i0 + R, ny);
        const int lo = max(i0 - 1, 0), hi = min(i1, ny - 1);  // rows of the plane the u ring may touch
        const T *base = u + poff + (int64_t)cvc * NV;
        auto ld = [&](int i) { return *reinterpret_cast<const V *>(base + (int64_t)i * nx); };
        auto ldm = [&](int i) { return *reinterpret_cast<const V *>(base - plane + (int64_t)i * nx); };
        auto ldq = [&](int i) { return *reinterpret_cast<const V *>(base + plane + (int64_t)i * nx); };
        auto ldb = [&](int i) {
            return __builtin_nontemporal_load(
                reinterpret_cast<const V *>(b + poff + (int64_t)cvc * NV + (int64_t)i * nx));
        };
        auto ldp = [&](int i) {
            return __builtin_nontemporal_load(
                reinterpret_cast<const V *>(un + poff + (int64_t)cvc * NV + (int64_t)i * nx));
        };
        const uint32_t soff = out_lane ? (uint32_t)(cv * NV * sizeof(T)) : kDrop;
        const int j0 = cv * NV;
        // ring: row i0 - 1 + t lives in slot t % 5; only rows of the block are
        // centres, so the centre-indexed rings clamp to [i0, i1 - 1]
        V S[5], ZM[5], ZP[5];
        S[0] = ld(lo);
        S[1] = ld(i0);
        S[2] = ld(min(i0 + 1, hi));
        S[3] = ld(min(i0 + 2, hi));
        S[4] = V{};
        ZM[0] = V{}, ZP[0] = V{}, ZM[4] = V{}, ZP[4] = V{};
        ZM[1] = ldm(i0), ZP[1] = ldq(i0);
        ZM[2] = ldm(min(i0 + 1, i1 - 1)), ZP[2] = ldq(min(i0 + 1, i1 - 1));
        ZM[3] = ldm(min(i0 + 2, i1 - 1)), ZP[3] = ldq(min(i0 + 2, i1 - 1));
        V B[RHS ? 5 : 1];
        if constexpr (RHS) {
            B[0] = V{}, B[4] = V{};
            B[1] = ldb(i0);
            B[2] = ldb(min(i0 + 1, i1 - 1));
            B[3] = ldb(min(i0 + 2, i1 - 1));
        }
        V P[ACCEL ? 5 : 1];
        if constexpr (ACCEL) {
            P[0] = V{}, P[4] = V{};
            P[1] = ldp(i0);
            P[2] = ldp(min(i0 + 1, i1 - 1));
            P[3] = ldp(min(i0 + 2, i1 - 1));
        }
        __builtin_amdgcn_sched_barrier(0);
        auto step = [&](auto kc, int i) {
            constexpr int k = decltype(kc)::value;
            const int r = i + k;  // row computed in this step, < i1
            S[(k + 4) % 5] = ld(min(r + 3, hi));
            const int rc = min(r + 3, i1 - 1);
            ZM[(k + 4) % 5] = ldm(rc);
            ZP[(k + 4) % 5] = ldq(rc);
            if constexpr (RHS) B[(k + 4) % 5] = ldb(rc);
            if constexpr (ACCEL) P[(k + 4) % 5] = ldp(rc);
            const V up = S[k % 5], cen = S[(k + 1) % 5], dn = S[(k + 2) % 5];
            const V zm = ZM[(k + 1) % 5], zp = ZP[(k + 1) % 5];
            const T left = dpp_shift<T>(cen[NV - 1], 0x138);  // lane - 1's last element
            const T right = dpp_shift<T>(cen[0], 0x130);      // lane + 1's first element
            const bool rowin = r > 0 && r < ny - 1;           // wave-uniform
            V res;
#pragma unroll
            for (int e = 0; e < NV; ++e) {
                const int j = j0 + e;
                const T l = e == 0 ? left : cen[e - 1];
                const T rr = e == NV - 1 ? right : cen[e + 1];
                T src = (T)0;
                if constexpr (RHS) src = B[(k + 1) % 5][e];
                const T sm = j3_value<T, RHS>(zm[e], zp[e], up[e], dn[e], l, rr, src);
                const bool interior = rowin && j > 0 && j < nx - 1;
                if constexpr (ACCEL) {
                    const T pv = P[(k + 1) % 5][e];
                    const T df = sm - pv;
                    const T w = omega * df;
                    res[e] = interior ? pv + w : cen[e];
                } else {
                    res[e] = interior ? sm : cen[e];
                }
                const T d = sm > cen[e] ? sm - cen[e] : cen[e] - sm;
                rmax = fmax(rmax, (interior && out_lane) ? d : (T)0);  // select + v_max: no exec branch
            }
            // one descriptor per output row: descriptor ranges are 32-bit
            const __amdgpu_buffer_rsrc_t orow = __builtin_amdgcn_make_buffer_rsrc(
                un + poff + (int64_t)r * nx, 0, nx * (int)sizeof(T), 0x00020000);
            typedef uint32_t u4 __attribute__((ext_vector_type(4)));
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4, res), orow, soff, 0, 2);  // non-temporal
            __builtin_amdgcn_sched_barrier(0);
        };
        using I0 = std::integral_constant<int, 0>;
        using I1 = std::integral_constant<int, 1>;
        using I2 = std::integral_constant<int, 2>;
        using I3 = std::integral_constant<int, 3>;
        using I4 = std::integral_constant<int, 4>;
        const int nrow = i1 - i0;
        const int ngrp = nrow / 5;
        int i = i0;
        for (int g = 0; g < ngrp; ++g, i += 5) {
            step(I0{}, i);
            step(I1{}, i);
            step(I2{}, i);
            step(I3{}, i);
            step(I4{}, i);
        }
        const int rem = nrow - ngrp * 5;
        if (rem > 0) {
            step(I0{}, i);
            if (rem > 1) {
                step(I1{}, i);
                if (rem > 2) {
                    step(I2{}, i);
                    if (rem > 3) step(I3{}, i);
                }
            }
        }
    }
    if (resid) j3_fold_residual<T, WPB>(rmax, resid);  // block-uniform; no wave returned early
}

// ---------------------------------------------------------------------------
// wave form 1, "march" (2.5-D): a wave owns a strip of 62 vectors x TY rows
// [i0, i0 + TY) and marches the planes [z0, z1) of its z block. Three planes of
// TY + 2 row vectors stay in registers (roles rotate through an unroll by 3, so
// no register moves): z and y neighbours come from registers, x neighbours
// from the adjacent lanes (DPP). Each plane of u is fetched once per wave,
// (TY + 2) / TY rows per output row; the overlap rows are shared with the row
// tile above and below, whose waves run at the same time. A step issues every
// load of plane z + 1 (and of b and p at plane z) at once and then computes
// plane z; other waves of the SIMD cover the wait. Rows past ny - 1 (the last
// row tile) compute on clamped rows and are dropped at the store.
// ---------------------------------------------------------------------------
template <typename T, int TY, bool RHS, bool ACCEL, bool REMAP = false, int WPB = 4>
__global__ __launch_bounds__(64 * WPB) void jacobi3d_march_kernel(const T *__restrict__ u, const T *__restrict__ b,
                                                                 T *__restrict__ un, int nx, int ny, int k0, int k1,
                                                                 int strips, int nrb, int KZ, int nwaves, T omega,
                                                                 T *__restrict__ resid) {
    using V = typename JWide<T>::type;
    constexpr int NV = JVec<T>::n;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(j3_block<REMAP>() * WPB + (threadIdx.x >> 6));
    T rmax = (T)0;
    if (wave < nwaves) {
        const int strip = wave % strips;  // consecutive waves: adjacent strips, then row tiles, then z blocks
        const int t = wave / strips;
        const int i0 = (t % nrb) * TY;
        const int z0 = k0 + (t / nrb) * KZ;  // < k1: the launch has ceil((k1 - k0) / KZ) z blocks
        const int z1 = min(z0 + KZ, k1);
        const int64_t plane = (int64_t)ny * nx;
        const int nvec = nx / NV;
        const int cv = strip * kStripVec - 1 + lane;
        const bool out_lane = lane >= 1 && lane <= kStripVec && cv < nvec;
        const int cvc = min(max(cv, 0), nvec - 1);
        int roff[TY + 2];  // element offset of row i0 - 1 + m, clamped into the plane (ny * nx < 2^31)
#pragma unroll
        for (int m = 0; m < TY + 2; ++m) roff[m] = min(max(i0 - 1 + m, 0), ny - 1) * nx;
        const T *ucol = u + (int64_t)cvc * NV;
        auto ld = [&](int z, int m) { return *reinterpret_cast<const V *>(ucol + (int64_t)z * plane + roff[m]); };
        auto ldb = [&](int z, int m) {
            return __builtin_nontemporal_load(
                reinterpret_cast<const V *>(b + (int64_t)cvc * NV + (int64_t)z * plane + roff[m]));
        };
        auto ldp = [&](int z, int m) {
            return __builtin_nontemporal_load(
                reinterpret_cast<const V *>(un + (int64_t)cvc * NV + (int64_t)z * plane + roff[m]));
        };
        const uint32_t soff = out_lane ? (uint32_t)(cv * NV * sizeof(T)) : kDrop;
        const int j0 = cv * NV;
        V Q0[TY + 2], Q1[TY + 2], Q2[TY + 2];
#pragma unroll
        for (int m = 0; m < TY + 2; ++m) {
            Q0[m] = ld(z0 - 1, m);
            Q1[m] = ld(z0, m);
            Q2[m] = V{};
        }
        // M, C, N: planes z - 1, z, z + 1
        auto step = [&](auto &M, auto &C, auto &N, int z) {
#pragma unroll
            for (int m = 0; m < TY + 2; ++m) N[m] = ld(z + 1, m);
            V B[RHS ? TY : 1], P[ACCEL ? TY : 1];
            if constexpr (RHS) {
#pragma unroll
                for (int m = 0; m < TY; ++m) B[m] = ldb(z, m + 1);
            }
            if constexpr (ACCEL) {  // this lane's own elements of un, before they are stored
#pragma unroll
                for (int m = 0; m < TY; ++m) P[m] = ldp(z, m + 1);
            }
#pragma unroll
            for (int m = 1; m <= TY; ++m) {
                const int r = i0 - 1 + m;  // >= 0
                const bool rok = r < ny;
                const bool rowin = r > 0 && r < ny - 1;  // wave-uniform
                const V cen = C[m];
                const T left = dpp_shift<T>(cen[NV - 1], 0x138);
                const T right = dpp_shift<T>(cen[0], 0x130);
                V res;
#pragma unroll
                for (int e = 0; e < NV; ++e) {
                    const int j = j0 + e;
                    const T l = e == 0 ? left : cen[e - 1];
                    const T rr = e == NV - 1 ? right : cen[e + 1];
                    T src = (T)0;
                    if constexpr (RHS) src = B[m - 1][e];
                    const T sm = j3_value<T, RHS>(M[m][e], N[m][e], C[m - 1][e], C[m + 1][e], l, rr, src);
                    const bool interior = rowin && j > 0 && j < nx - 1;
                    if constexpr (ACCEL) {
                        const T pv = P[m - 1][e];
                        const T df = sm - pv;
                        const T w = omega * df;
                        res[e] = interior ? pv + w : cen[e];
                    } else {
                        res[e] = interior ? sm : cen[e];
                    }
                    const T d = sm > cen[e] ? sm - cen[e] : cen[e] - sm;
                    rmax = fmax(rmax, (interior && out_lane) ? d : (T)0);
                }
                const __amdgpu_buffer_rsrc_t orow = __builtin_amdgcn_make_buffer_rsrc(
                    un + (int64_t)z * plane + roff[m], 0, nx * (int)sizeof(T), 0x00020000);
                typedef uint32_t u4 __attribute__((ext_vector_type(4)));
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4, res), orow, rok ? soff : kDrop, 0, 2);
            }
        };
        int z = z0;
        while (true) {
            step(Q0, Q1, Q2, z);
            if (++z >= z1) break;
            step(Q1, Q2, Q0, z);
            if (++z >= z1) break;
            step(Q2, Q0, Q1, z);
            if (++z >= z1) break;
        }
    }
    if (resid) j3_fold_residual<T, WPB>(rmax, resid);
}

// ---------------------------------------------------------------------------
// host side: argument checks and launches shared by the production entries and
// the tuning entry
// ---------------------------------------------------------------------------
// omega: in T's range before the conversion (NaN fails the first comparison),
// positive after it
template <typename T>
inline int j3_check(const void *u, const void *un, int nx, int ny, int k0, int k1, bool accel, double omega_d,
                    T *omega) {
    MPX_CHECK_ARG(u && un, "null pointer");
    MPX_CHECK_ARG(nx >= 3 && ny >= 3 && (int64_t)ny * nx < ((int64_t)1 << 31) && k0 >= 1 && k1 >= k0,
                  "bad volume geometry (nx, ny >= 3, ny * nx < 2^31, 1 <= k0 <= k1)");
    const bool w_ok = omega_d > 0.0 && omega_d <= (double)std::numeric_limits<T>::max();
    *omega = w_ok ? (T)omega_d : (T)0;
    MPX_CHECK_ARG(!accel || *omega > (T)0, "omega must be finite and positive");
    return MPX_OK;
}

template <typename T>
inline bool j3_vector_layout(const T *u, const T *b, const T *un, int nx) {
    return nx % JVec<T>::n == 0 && aligned16(u) && aligned16(un) && (!b || aligned16(b)) &&
           (int64_t)nx * (int64_t)sizeof(T) < (int64_t)kDrop;
}

inline int64_t j3_waves(int strips, int ny, int ty, int planes, int kz) {
    return (int64_t)strips * ((ny + ty - 1) / ty) * ((planes + kz - 1) / kz);
}

template <typename T, bool RHS, bool ACCEL, bool REMAP>
int launch_j3_rows(const T *u, const T *b, T *un, int nx, int ny, int k0, int k1, int R, T omega, T *resid,
                   hipStream_t s) {
    const int strips = (nx / JVec<T>::n + kStripVec - 1) / kStripVec;
    const int nrb = (ny + R - 1) / R;
    const int64_t nw = j3_waves(strips, ny, R, k1 - k0, 1);
    MPX_CHECK_ARG(nw <= INT_MAX, "volume too large for one launch");
    hipLaunchKernelGGL((jacobi3d_rows_kernel<T, RHS, ACCEL, REMAP>), dim3((unsigned)((nw + 3) / 4)), dim3(256), 0, s, u, b, un,
                       nx, ny, k0, strips, nrb, R, (int)nw, omega, resid);
    MPX_RETURN_IF_HIP_ERROR(hipGetLastError());
    return MPX_OK;
}

template <typename T, int TY, bool RHS, bool ACCEL, bool REMAP>
int launch_j3_march(const T *u, const T *b, T *un, int nx, int ny, int k0, int k1, int KZ, T omega, T *resid,
                    hipStream_t s) {
    const int strips = (nx / JVec<T>::n + kStripVec - 1) / kStripVec;
    const int nrb = (ny + TY - 1) / TY;
    const int64_t nw = j3_waves(strips, ny, TY, k1 - k0, KZ);
    MPX_CHECK_ARG(nw <= INT_MAX, "volume too large for one launch");
    hipLaunchKernelGGL((jacobi3d_march_kernel<T, TY, RHS, ACCEL, REMAP>), dim3((unsigned)((nw + 3) / 4)), dim3(256), 0, s, u, b,
                       un, nx, ny, k0, k1, strips, nrb, KZ, (int)nw, omega, resid);
    MPX_RETURN_IF_HIP_ERROR(hipGetLastError());
    return MPX_OK;
}

}  // namespace
}  // namespace mpx
