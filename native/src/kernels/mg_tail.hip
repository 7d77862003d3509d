// The coarse levels of a multigrid V-cycle in one kernel (models.PoissonMultigrid
// and PoissonMultigrid3D, tail_points): from descriptor 0 down to the coarsest
// level and back up, exactly the sequence of launches the models make for a
// level k >= 1 (sweeps, residual, restriction, zero fill, the recursion,
// prolongation, post-sweeps), with a workgroup barrier where the launched cycle
// has a kernel boundary.
//
// MI355X design: below a few thousand points a level is launch-bound (65 of the
// 81 launches of a 2049^2 cycle have a few microseconds of work at most,
// profiles/multigrid.md), so
//   * one workgroup of up to 1024 threads runs the whole sub-cycle; the only
//     synchronisation is __syncthreads(), always in control flow that depends on
//     kernel arguments alone (level count, sweep counts), so it is uniform;
//   * a phase hands its points to the threads by a strided walk over the level
//     (point t, t + T, t + 2T, ...; row and column advance by the quotient and
//     remainder of T, no division per point), so a row wider than the workgroup
//     and a level smaller than a wave are the same code;
//   * what one phase writes the next reads through plain global loads and
//     stores of one CU (the levels of a tail fit the L2 many times over): the
//     barrier's workgroup-scope release / acquire makes them visible. The
//     pointers carry no __restrict__ and no const-cache hint;
//   * the restriction into level k + 1's b and the zero fill of its u write
//     disjoint buffers and share a phase;
//   * every point's expression is the launched operator's, operation for
//     operation (jacobi_wave.hpp, multigrid.hip, multigrid3d.hip; the order is
//     in capi.h), each + - * rounded once (-ffp-contract=off), so the tail is
//     bit-identical to the launches it replaces.
//
// Sweeps ping-pong between a level's u and un: after the kernel a level's
// iterate lies in un when the level ran an odd number of sweeps (nu1 + nu2, on
// the last level coarse_sweeps or 1), in u otherwise. Rows 0 and H - 1 (3-D:
// planes 0 and D - 1 too) of un are never written; padding is never touched.
#include "internal.hpp"

#include <limits>

namespace mpx {
namespace {

constexpr int kTailThreads = 1024;

struct Tail2 {
    mpx_mg_level lv[MPX_MG_TAIL_MAX_LEVELS];
};
struct Tail3 {
    mpx_mg3_level lv[MPX_MG_TAIL_MAX_LEVELS];
};

// The strided walk of one thread over the points of a (rows, cols) box: point
// index t = threadIdx.x, then t + T, ...; f(i, j) with i in [0, rows), j in
// [0, cols). One division per phase (uniform), none per point.
template <typename F>
__device__ __forceinline__ void walk2(int rows, int cols, F f) {
    const int T = (int)blockDim.x, t = (int)threadIdx.x;
    const int qi = T / cols, qj = T - qi * cols;
    int i = t / cols, j = t - i * cols;
    while (i < rows) {
        f(i, j);
        j += qj;
        i += qi;
        if (j >= cols) {
            j -= cols;
            ++i;
        }
    }
}

// the same over a (planes, rows, cols) box: f(k, i, j)
template <typename F>
__device__ __forceinline__ void walk3(int planes, int rows, int cols, F f) {
    const int T = (int)blockDim.x, t = (int)threadIdx.x;
    const int tr = T / cols, qj = T - tr * cols;  // T = (qk * rows + qi) * cols + qj
    const int qk = tr / rows, qi = tr - qk * rows;
    const int r0 = t / cols;
    int j = t - r0 * cols;
    int k = r0 / rows, i = r0 - k * rows;
    while (k < planes) {
        f(k, i, j);
        j += qj;
        i += qi;
        k += qk;
        if (j >= cols) {
            j -= cols;
            ++i;
        }
        if (i >= rows) {
            i -= rows;
            ++k;
        }
    }
}

// ------------------------------------------------------------------ 2-D phases
// damped sweep over rows [1, h - 1): un = c + omega * (s - c) at the interior
// columns, s = (((up + dn) + (l + r)) + b) * 0.25; columns 0 / w - 1 copy through
template <typename T>
__device__ __forceinline__ void tail_relax(const T *u, const T *b, T *un, int h, int w, int pitch, T omega) {
    walk2(h - 2, w, [&](int ii, int j) {
        const int64_t o = (int64_t)(ii + 1) * pitch + j;
        const T *c = u + o;
        const T cv = c[0];
        T out = cv;
        if (j > 0 && j < w - 1) {
            const T n4 = (c[-pitch] + c[pitch]) + (c[-1] + c[1]);
            const T s = (n4 + b[o]) * (T)0.25;
            const T d = s - cv;
            const T t = omega * d;
            out = cv + t;
        }
        un[o] = out;
    });
}

// r = ((((up + dn) + (l + rt)) + b) - 4 c) at the interior points
template <typename T>
__device__ __forceinline__ void tail_residual(const T *u, const T *b, T *r, int h, int w, int pitch) {
    walk2(h - 2, w - 2, [&](int ii, int jj) {
        const int64_t o = (int64_t)(ii + 1) * pitch + (jj + 1);
        const T *c = u + o;
        T n = (c[-pitch] + c[pitch]) + (c[-1] + c[1]);
        n = n + b[o];
        const T c4 = (T)4 * c[0];
        r[o] = n - c4;
    });
}

// P[J] of the full weighting in one fine plane: m points at the fine row 2I
template <typename T>
__device__ __forceinline__ T tail_weight(const T *m, int j, int pitch) {
    const T *t = m - pitch, *d = m + pitch;
    const T e = (t[j] + d[j]) + (m[j - 1] + m[j + 1]);
    const T x = (t[j - 1] + t[j + 1]) + (d[j - 1] + d[j + 1]);
    const T eh = e * (T)0.5;
    const T xq = x * (T)0.25;
    return (m[j] + eh) + xq;
}

// full weighting of the fine r into the interior of the coarse bc, and the
// coarse u <- 0 on all of its (hc, wc) points
template <typename T>
__device__ __forceinline__ void tail_restrict_zero(const T *r, int pr, T *bc, T *uc, int hc, int wc, int pc) {
    walk2(hc, wc, [&](int I, int J) {
        const int64_t o = (int64_t)I * pc + J;
        uc[o] = (T)0;
        if (I > 0 && I < hc - 1 && J > 0 && J < wc - 1) bc[o] = tail_weight<T>(r + (int64_t)(2 * I) * pr, 2 * J, pr);
    });
}

// bilinear interpolation of the coarse e added to the fine interior of u
template <typename T>
__device__ __forceinline__ void tail_prolong(const T *e, int pe, T *u, int h, int w, int pu) {
    walk2(h - 2, w - 2, [&](int ii, int jj) {
        const int i = ii + 1, j = jj + 1, J = j >> 1;
        const T *c0 = e + (int64_t)(i >> 1) * pe;
        const T *c1 = c0 + pe;  // read on odd rows only
        T v;
        if (!(i & 1)) {
            v = (j & 1) ? (c0[J] + c0[J + 1]) * (T)0.5 : c0[J];
        } else if (!(j & 1)) {
            v = (c0[J] + c1[J]) * (T)0.5;
        } else {
            v = ((c0[J] + c1[J]) + (c0[J + 1] + c1[J + 1])) * (T)0.25;
        }
        T *o = u + (int64_t)i * pu + j;
        *o = *o + v;
    });
}

template <typename T>
__global__ __launch_bounds__(kTailThreads) void mg_tail_kernel(Tail2 a, int n, int nu1, int nu2, int coarse, T omega) {
    // down: level k's iterate is in u before its sweeps (given, or zeroed here)
    for (int k = 0; k + 1 < n; ++k) {
        const mpx_mg_level &f = a.lv[k], &c = a.lv[k + 1];
        T *cur = (T *)f.u, *oth = (T *)f.un;
        for (int s = 0; s < nu1; ++s) {
            tail_relax<T>(cur, (const T *)f.b, oth, f.h, f.w, f.pitch, omega);
            __syncthreads();
            T *t = cur;
            cur = oth;
            oth = t;
        }
        tail_residual<T>(cur, (const T *)f.b, (T *)f.r, f.h, f.w, f.pitch);
        __syncthreads();
        tail_restrict_zero<T>((const T *)f.r, f.pitch, (T *)c.b, (T *)c.u, c.h, c.w, c.pitch);
        __syncthreads();
    }
    {
        const mpx_mg_level &f = a.lv[n - 1];
        const bool exact = f.h == 3 && f.w == 3;
        const int sweeps = exact ? 1 : coarse;
        const T om = exact ? (T)1 : omega;
        T *cur = (T *)f.u, *oth = (T *)f.un;
        for (int s = 0; s < sweeps; ++s) {
            tail_relax<T>(cur, (const T *)f.b, oth, f.h, f.w, f.pitch, om);
            __syncthreads();
            T *t = cur;
            cur = oth;
            oth = t;
        }
    }
    // up: the coarse iterate's buffer follows from its sweep count
    for (int k = n - 2; k >= 0; --k) {
        const mpx_mg_level &f = a.lv[k], &c = a.lv[k + 1];
        const int csweeps = k + 2 < n ? nu1 + nu2 : (c.h == 3 && c.w == 3 ? 1 : coarse);
        const T *e = (const T *)((csweeps & 1) ? c.un : c.u);
        T *cur = (T *)((nu1 & 1) ? f.un : f.u), *oth = (T *)((nu1 & 1) ? f.u : f.un);
        tail_prolong<T>(e, c.pitch, cur, f.h, f.w, f.pitch);
        __syncthreads();
        for (int s = 0; s < nu2; ++s) {
            tail_relax<T>(cur, (const T *)f.b, oth, f.h, f.w, f.pitch, omega);
            __syncthreads();
            T *t = cur;
            cur = oth;
            oth = t;
        }
    }
}

// ------------------------------------------------------------------ 3-D phases
// n = ((zm + zp) + (ym + yp)) + (xm + xp) around c
template <typename T>
__device__ __forceinline__ T tail3_neighbours(const T *c, int pitch, int64_t plane) {
    return ((c[-plane] + c[plane]) + (c[-pitch] + c[pitch])) + (c[-1] + c[1]);
}

// damped sweep over planes [1, d - 1): un = c + omega * (s - c) at the interior
// points, s = (n + b) * (1/6); boundary rows and columns copy through
template <typename T>
__device__ __forceinline__ void tail3_relax(const T *u, const T *b, T *un, int d, int h, int w, int pitch,
                                            int64_t plane, T omega) {
    walk3(d - 2, h, w, [&](int kk, int i, int j) {
        const int64_t o = (int64_t)(kk + 1) * plane + (int64_t)i * pitch + j;
        const T *c = u + o;
        const T cv = c[0];
        T out = cv;
        if (i > 0 && i < h - 1 && j > 0 && j < w - 1) {
            const T nb = tail3_neighbours<T>(c, pitch, plane) + b[o];
            const T s = nb * (T)(1.0 / 6.0);
            const T df = s - cv;
            const T t = omega * df;
            out = cv + t;
        }
        un[o] = out;
    });
}

template <typename T>
__device__ __forceinline__ void tail3_residual(const T *u, const T *b, T *r, int d, int h, int w, int pitch,
                                               int64_t plane) {
    walk3(d - 2, h - 2, w - 2, [&](int kk, int ii, int jj) {
        const int64_t o = (int64_t)(kk + 1) * plane + (int64_t)(ii + 1) * pitch + (jj + 1);
        const T *c = u + o;
        const T nb = tail3_neighbours<T>(c, pitch, plane) + b[o];
        const T c6 = (T)6 * c[0];
        r[o] = nb - c6;
    });
}

// 27-point full weighting (separable: the 2-D rule per fine plane, then
// (P_2K + (P_2K-1 + P_2K+1) * 0.5) * 0.5) and the coarse u <- 0
template <typename T>
__device__ __forceinline__ void tail3_restrict_zero(const T *r, int pr, int64_t sr, T *bc, T *uc, int dc, int hc, int wc,
                                                    int pc, int64_t sc) {
    walk3(dc, hc, wc, [&](int K, int J, int I) {
        const int64_t o = (int64_t)K * sc + (int64_t)J * pc + I;
        uc[o] = (T)0;
        if (K > 0 && K < dc - 1 && J > 0 && J < hc - 1 && I > 0 && I < wc - 1) {
            const T *m = r + (int64_t)(2 * K) * sr + (int64_t)(2 * J) * pr;
            const T lo = tail_weight<T>(m - sr, 2 * I, pr);
            const T mid = tail_weight<T>(m, 2 * I, pr);
            const T hi = tail_weight<T>(m + sr, 2 * I, pr);
            const T z = lo + hi;
            const T zh = z * (T)0.5;
            const T v = mid + zh;
            bc[o] = v * (T)0.5;
        }
    });
}

// trilinear interpolation added to the fine interior: pair sums in z, then y,
// then x, one exact scale 0.5^(odd coordinates), no multiply when it is 1
template <typename T>
__device__ __forceinline__ void tail3_prolong(const T *e, int pe, int64_t se, T *u, int d, int h, int w, int pu,
                                              int64_t su) {
    walk3(d - 2, h - 2, w - 2, [&](int kk, int ii, int jj) {
        const int k = kk + 1, i = ii + 1, j = jj + 1, I = j >> 1;
        const int64_t dz = (k & 1) ? se : 0;  // the +1 neighbours are read on odd coordinates only
        const int64_t dy = (i & 1) ? pe : 0;
        const T *c = e + (int64_t)(k >> 1) * se + (int64_t)(i >> 1) * pe;
        const int odd = (k & 1) + (i & 1) + (j & 1);
        T z00 = c[I], z10 = c[I + dy], x;
        if (k & 1) {
            z00 = z00 + c[I + dz];
            z10 = z10 + c[I + dy + dz];
        }
        const T y0 = (i & 1) ? z00 + z10 : z00;
        if (j & 1) {
            T z01 = c[I + 1], z11 = c[I + 1 + dy];
            if (k & 1) {
                z01 = z01 + c[I + 1 + dz];
                z11 = z11 + c[I + 1 + dy + dz];
            }
            const T y1 = (i & 1) ? z01 + z11 : z01;
            x = y0 + y1;
        } else {
            x = y0;
        }
        const T scale = odd == 1 ? (T)0.5 : odd == 2 ? (T)0.25 : (T)0.125;
        T *o = u + (int64_t)k * su + (int64_t)i * pu + j;
        *o = odd ? *o + x * scale : *o + x;
    });
}

template <typename T>
__global__ __launch_bounds__(kTailThreads) void mg3_tail_kernel(Tail3 a, int n, int nu1, int nu2, int coarse, T omega) {
    for (int k = 0; k + 1 < n; ++k) {
        const mpx_mg3_level &f = a.lv[k], &c = a.lv[k + 1];
        T *cur = (T *)f.u, *oth = (T *)f.un;
        for (int s = 0; s < nu1; ++s) {
            tail3_relax<T>(cur, (const T *)f.b, oth, f.d, f.h, f.w, f.pitch, f.plane, omega);
            __syncthreads();
            T *t = cur;
            cur = oth;
            oth = t;
        }
        tail3_residual<T>(cur, (const T *)f.b, (T *)f.r, f.d, f.h, f.w, f.pitch, f.plane);
        __syncthreads();
        tail3_restrict_zero<T>((const T *)f.r, f.pitch, f.plane, (T *)c.b, (T *)c.u, c.d, c.h, c.w, c.pitch, c.plane);
        __syncthreads();
    }
    {
        const mpx_mg3_level &f = a.lv[n - 1];
        const bool exact = f.d == 3 && f.h == 3 && f.w == 3;
        const int sweeps = exact ? 1 : coarse;
        const T om = exact ? (T)1 : omega;
        T *cur = (T *)f.u, *oth = (T *)f.un;
        for (int s = 0; s < sweeps; ++s) {
            tail3_relax<T>(cur, (const T *)f.b, oth, f.d, f.h, f.w, f.pitch, f.plane, om);
            __syncthreads();
            T *t = cur;
            cur = oth;
            oth = t;
        }
    }
    for (int k = n - 2; k >= 0; --k) {
        const mpx_mg3_level &f = a.lv[k], &c = a.lv[k + 1];
        const int csweeps = k + 2 < n ? nu1 + nu2 : (c.d == 3 && c.h == 3 && c.w == 3 ? 1 : coarse);
        const T *e = (const T *)((csweeps & 1) ? c.un : c.u);
        T *cur = (T *)((nu1 & 1) ? f.un : f.u), *oth = (T *)((nu1 & 1) ? f.u : f.un);
        tail3_prolong<T>(e, c.pitch, c.plane, cur, f.d, f.h, f.w, f.pitch, f.plane);
        __syncthreads();
        for (int s = 0; s < nu2; ++s) {
            tail3_relax<T>(cur, (const T *)f.b, oth, f.d, f.h, f.w, f.pitch, f.plane, omega);
            __syncthreads();
            T *t = cur;
            cur = oth;
            oth = t;
        }
    }
}

// ------------------------------------------------------------------ launchers
// omega rounded once to T, finite and positive before and after (launch_jacobi)
template <typename T>
bool tail_omega(double omega_d, T *omega) {
    const bool ok = omega_d > 0.0 && omega_d <= (double)std::numeric_limits<T>::max();
    *omega = ok ? (T)omega_d : (T)0;
    return *omega > (T)0;
}

// a workgroup of whole waves, no larger than the largest level needs
inline int tail_threads(int64_t points) {
    const int64_t t = (points + kWave - 1) / kWave * kWave;
    return (int)(t < kWave ? kWave : t > kTailThreads ? kTailThreads : t);
}

template <typename T>
int launch_mg_tail(const mpx_mg_level *lv, int n, int nu1, int nu2, int coarse, double omega_d, void *stream) {
    MPX_CHECK_ARG(lv, "null pointer");
    MPX_CHECK_ARG(n >= 1 && n <= MPX_MG_TAIL_MAX_LEVELS, "need 1..16 levels");
    MPX_CHECK_ARG(nu1 >= 0 && nu2 >= 1 && coarse >= 1, "need nu1 >= 0, nu2 >= 1 and coarse_sweeps >= 1");
    T omega;
    MPX_CHECK_ARG(tail_omega<T>(omega_d, &omega), "omega must be finite and positive");
    Tail2 a{};
    for (int k = 0; k < n; ++k) {
        const mpx_mg_level &l = lv[k];
        MPX_CHECK_ARG(l.u && l.un && l.b && (l.r || k + 1 == n), "null pointer");
        MPX_CHECK_ARG(l.h >= 3 && l.w >= 3 && l.pitch >= l.w, "bad grid geometry");
        MPX_CHECK_ARG(k == 0 || (lv[k - 1].h == 2 * l.h - 1 && lv[k - 1].w == 2 * l.w - 1),
                      "a level is not the coarse grid of the level before it");
        a.lv[k] = l;
    }
    const int threads = tail_threads((int64_t)lv[0].h * lv[0].w);
    hipLaunchKernelGGL((mg_tail_kernel<T>), dim3(1), dim3(threads), 0, as_stream(stream), a, n, nu1, nu2, coarse, omega);
    MPX_RETURN_IF_HIP_ERROR(hipGetLastError());
    return MPX_OK;
}

template <typename T>
int launch_mg3_tail(const mpx_mg3_level *lv, int n, int nu1, int nu2, int coarse, double omega_d, void *stream) {
    MPX_CHECK_ARG(lv, "null pointer");
    MPX_CHECK_ARG(n >= 1 && n <= MPX_MG_TAIL_MAX_LEVELS, "need 1..16 levels");
    MPX_CHECK_ARG(nu1 >= 0 && nu2 >= 1 && coarse >= 1, "need nu1 >= 0, nu2 >= 1 and coarse_sweeps >= 1");
    T omega;
    MPX_CHECK_ARG(tail_omega<T>(omega_d, &omega), "omega must be finite and positive");
    Tail3 a{};
    for (int k = 0; k < n; ++k) {
        const mpx_mg3_level &l = lv[k];
        MPX_CHECK_ARG(l.u && l.un && l.b && (l.r || k + 1 == n), "null pointer");
        MPX_CHECK_ARG(l.d >= 3 && l.h >= 3 && l.w >= 3 && l.pitch >= l.w && l.plane >= (int64_t)l.h * l.pitch,
                      "bad grid geometry");
        MPX_CHECK_ARG(k == 0 || (lv[k - 1].d == 2 * l.d - 1 && lv[k - 1].h == 2 * l.h - 1 && lv[k - 1].w == 2 * l.w - 1),
                      "a level is not the coarse grid of the level before it");
        a.lv[k] = l;
    }
    const int threads = tail_threads((int64_t)lv[0].d * lv[0].h * lv[0].w);
    hipLaunchKernelGGL((mg3_tail_kernel<T>), dim3(1), dim3(threads), 0, as_stream(stream), a, n, nu1, nu2, coarse, omega);
    MPX_RETURN_IF_HIP_ERROR(hipGetLastError());
    return MPX_OK;
}

}  // namespace
MPX_MODULE_ANCHOR(mg_tail)

}  // namespace mpx

extern "C" int mpx_mg_tail_f64(const mpx_mg_level *lv, int n, int nu1, int nu2, int coarse_sweeps, double omega,
                               void *stream) {
    return mpx::launch_mg_tail<double>(lv, n, nu1, nu2, coarse_sweeps, omega, stream);
}

extern "C" int mpx_mg_tail_f32(const mpx_mg_level *lv, int n, int nu1, int nu2, int coarse_sweeps, double omega,
                               void *stream) {
    return mpx::launch_mg_tail<float>(lv, n, nu1, nu2, coarse_sweeps, omega, stream);
}

extern "C" int mpx_mg3_tail_f64(const mpx_mg3_level *lv, int n, int nu1, int nu2, int coarse_sweeps, double omega,
                                void *stream) {
    return mpx::launch_mg3_tail<double>(lv, n, nu1, nu2, coarse_sweeps, omega, stream);
}

extern "C" int mpx_mg3_tail_f32(const mpx_mg3_level *lv, int n, int nu1, int nu2, int coarse_sweeps, double omega,
                                void *stream) {
    return mpx::launch_mg3_tail<float>(lv, n, nu1, nu2, coarse_sweeps, omega, stream);
}
