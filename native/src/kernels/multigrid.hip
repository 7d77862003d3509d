// Grid-transfer and residual kernels of the geometric multigrid V-cycle for the
// 2-D Poisson solver (models.PoissonMultigrid). The smoother is the damped
// Jacobi sweep of jacobi.hip (mpx_jacobi_relax_*).
//
// Layout: an (H, W) grid with Dirichlet values in rows 0 / H-1 and columns
// 0 / W-1; its coarse grid is (Hc, Wc) with H = 2 Hc - 1, W = 2 Wc - 1 and
// coarse point (I, J) on fine point (2I, 2J). Every tensor has its own row
// pitch (elements); padding is never read and never written.
//
// MI355X design: all three kernels are HBM-bound (3 / 1.25 / 2.25 words per
// fine point), so
//   * a lane owns one 16-B vector of the narrower grid per row (residual: of
//     u; restrict and prolong: of the coarse grid, and with it the two fine
//     vectors below it) and walks a block of rows down, so every input row is
//     fetched once and the rows shared by two output rows stay in registers
//     (a launch too small to fill the device that way shortens its walks:
//     mg_rows_per_lane, profiles/multigrid.md);
//   * the even/odd column interleave of the transfers happens inside the lane
//     (coarse vector k <-> fine elements 2k, 2k+1 of the lane's vector pair);
//     the one element a lane needs from its neighbour comes through a DPP wave
//     shift, and only lanes 0 / 63 of a wave load it themselves — no strided
//     global access;
//   * the VEC = false form (one element per lane, scalar loads) serves bases
//     and pitches that are not 16-byte multiples, as jacobi_kernel<T, false>;
//   * every + - * is one rounded operation (-ffp-contract=off), in the order
//     written in capi.h; the factors 4, 0.5 and 0.25 are exact.
#include "mg_lane.hpp"

namespace mpx {
namespace {

constexpr int kMgRows = 16;       // rows of the residual walked per lane
constexpr int kMgCoarseRows = 8;  // coarse rows walked per lane by the transfers
// a launch halves its rows per lane until it has this many waves (or one row):
// the coarser levels have too few columns to fill the device with long walks
constexpr int kMgMinWaves = 8192;

inline int mg_rows_per_lane(int lanes, int rows, int most) {
    const int64_t waves_x = (int64_t)((lanes + 255) / 256) * 4;
    int r = most;
    while (r > 1 && waves_x * ((rows + r - 1) / r) < kMgMinWaves) r >>= 1;
    return r;
}

// r = ((((up + dn) + (l + rt)) [+ b]) - 4 c) at the interior points of an
// (rows, cols) grid; max|r| folded into resid as the sweeps fold theirs
template <typename T, bool VEC, bool RHS>
__global__ __launch_bounds__(256) void mg_residual_kernel(const T *__restrict__ u, const T *__restrict__ b,
                                                          T *__restrict__ r, int rows, int cols, int pu, int pb,
                                                          int pr, int rpl, T *__restrict__ resid) {
    constexpr int NV = VEC ? JVec<T>::n : 1;
    const int j0 = NV * (blockIdx.x * blockDim.x + threadIdx.x);
    const int i0 = 1 + blockIdx.y * rpl;  // block-uniform: the whole wave walks the rows
    const int i1 = min(i0 + rpl, rows - 1);
    T rmax = (T)0;
    T up[NV], cen[NV], dn[NV];
    load_n<T, VEC, NV>(u + (int64_t)(i0 - 1) * pu, j0, cols, up);
    load_n<T, VEC, NV>(u + (int64_t)i0 * pu, j0, cols, cen);
    for (int i = i0; i < i1; ++i) {
        load_n<T, VEC, NV>(u + (int64_t)(i + 1) * pu, j0, cols, dn);
        const T *crow = u + (int64_t)i * pu;
        const T left = from_left<T>(cen[NV - 1], crow, j0, cols);
        const T right = from_right<T>(cen[0], crow, j0 + NV, cols);
        T src[NV];
        if constexpr (RHS) load_n<T, VEC, NV>(b + (int64_t)i * pb, j0, cols, src);
        T res[NV];
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const int j = j0 + k;
            const T l = k == 0 ? left : cen[k - 1];
            const T rt = k == NV - 1 ? right : cen[k + 1];
            T n = (up[k] + dn[k]) + (l + rt);
            if constexpr (RHS) n = n + src[k];
            const T c4 = (T)4 * cen[k];
            res[k] = n - c4;
            const T a = res[k] < (T)0 ? -res[k] : res[k];
            if (j > 0 && j < cols - 1) rmax = a > rmax ? a : rmax;
        }
        store_n<T, VEC, NV>(r + (int64_t)i * pr, j0, 1, cols - 2, res);
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            up[k] = cen[k];
            cen[k] = dn[k];
        }
    }
    if (resid) {
        using B = typename JVec<T>::bits;
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const T o = __shfl_xor(rmax, m);
            rmax = o > rmax ? o : rmax;
        }
        if ((threadIdx.x & 63) == 0 && rmax > (T)0) residual_max(reinterpret_cast<B *>(resid), __builtin_bit_cast(B, rmax));
    }
}

// full weighting, scaled for the h^2-scaled right-hand side of the coarse grid.
// A lane owns the coarse columns [J0, J0 + NV) and the fine columns
// [2 J0, 2 J0 + 2 NV) below them; of a fine row it keeps, per coarse column,
// the centre r[., 2J] and the rounded side sum r[., 2J-1] + r[., 2J+1]
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void mg_restrict_kernel(const T *__restrict__ r, T *__restrict__ bc, int hc, int wc,
                                                          int pr, int pc, int rpl) {
    constexpr int NV = VEC ? JVec<T>::n : 1;
    const int J0 = NV * (blockIdx.x * blockDim.x + threadIdx.x);
    const int f0 = 2 * J0;
    const int w = 2 * wc - 1;
    const int I0 = 1 + blockIdx.y * rpl;
    const int I1 = min(I0 + rpl, hc - 1);
    auto fetch = [&](int i, T (&c)[NV], T (&s)[NV]) {
        const T *row = r + (int64_t)i * pr;
        T a[2][NV];
        load_n<T, VEC, NV>(row, f0, w, a[0]);
        load_n<T, VEC, NV>(row, f0 + NV, w, a[1]);
        const T left = from_left<T>(a[1][NV - 1], row, f0, w);
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            c[k] = a[(2 * k) / NV][(2 * k) % NV];
            const T lft = k == 0 ? left : a[(2 * k - 1) / NV][(2 * k - 1) % NV];
            s[k] = lft + a[(2 * k + 1) / NV][(2 * k + 1) % NV];
        }
    };
    T tc[NV], ts[NV];
    fetch(2 * I0 - 1, tc, ts);
    for (int I = I0; I < I1; ++I) {
        T mc[NV], ms[NV], bn[NV], bs[NV];
        fetch(2 * I, mc, ms);
        fetch(2 * I + 1, bn, bs);
        T out[NV];
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const T e = (tc[k] + bn[k]) + ms[k];
            const T d = ts[k] + bs[k];
            const T eh = e * (T)0.5;
            const T dq = d * (T)0.25;
            out[k] = (mc[k] + eh) + dq;
            tc[k] = bn[k];
            ts[k] = bs[k];
        }
        store_n<T, VEC, NV>(bc + (int64_t)I * pc, J0, 1, wc - 2, out);
    }
}

// bilinear interpolation of the coarse e, added to the fine interior of u in
// place. A lane owns the coarse columns [J0, J0 + NV) (plus e[., J0 + NV] from
// its right neighbour) and reads and writes only its own fine columns
// [2 J0, 2 J0 + 2 NV) of u; coarse row I feeds the fine rows 2I and 2I + 1
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void mg_prolong_kernel(const T *__restrict__ e, T *__restrict__ u, int hc, int wc,
                                                         int pe, int pu, int rpl) {
    constexpr int NV = VEC ? JVec<T>::n : 1;
    const int J0 = NV * (blockIdx.x * blockDim.x + threadIdx.x);
    const int f0 = 2 * J0;
    const int w = 2 * wc - 1;
    const int I0 = blockIdx.y * rpl;
    const int I1 = min(I0 + rpl, hc - 1);
    auto fetch = [&](int I, T (&c)[NV + 1]) {
        const T *row = e + (int64_t)I * pe;
        T own[NV];
        load_n<T, VEC, NV>(row, J0, wc, own);
#pragma unroll
        for (int k = 0; k < NV; ++k) c[k] = own[k];
        c[NV] = from_right<T>(own[0], row, J0 + NV, wc);
    };
    // fine row i: columns 2J get ev, columns 2J + 1 get od
    auto add_row = [&](int i, const T (&ev)[NV], const T (&od)[NV]) {
        T *row = u + (int64_t)i * pu;
        T a[2][NV];
        load_n<T, VEC, NV>(row, f0, w, a[0]);
        load_n<T, VEC, NV>(row, f0 + NV, w, a[1]);
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            a[(2 * k) / NV][(2 * k) % NV] = a[(2 * k) / NV][(2 * k) % NV] + ev[k];
            a[(2 * k + 1) / NV][(2 * k + 1) % NV] = a[(2 * k + 1) / NV][(2 * k + 1) % NV] + od[k];
        }
        store_n<T, VEC, NV>(row, f0, 1, w - 2, a[0]);
        store_n<T, VEC, NV>(row, f0 + NV, 1, w - 2, a[1]);
    };
    T cur[NV + 1], nxt[NV + 1];
    fetch(I0, cur);
    for (int I = I0; I < I1; ++I) {
        fetch(I + 1, nxt);
        T ev[NV], od[NV];
        if (I >= 1) {  // block-uniform; fine row 0 is boundary
#pragma unroll
            for (int k = 0; k < NV; ++k) {
                const T h = cur[k] + cur[k + 1];
                ev[k] = cur[k];
                od[k] = h * (T)0.5;
            }
            add_row(2 * I, ev, od);
        }
        T v[NV + 1];
#pragma unroll
        for (int k = 0; k <= NV; ++k) v[k] = cur[k] + nxt[k];
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const T q = v[k] + v[k + 1];
            ev[k] = v[k] * (T)0.5;
            od[k] = q * (T)0.25;
        }
        add_row(2 * I + 1, ev, od);
#pragma unroll
        for (int k = 0; k <= NV; ++k) cur[k] = nxt[k];
    }
}

template <typename T>
int launch_mg_residual(const T *u, const T *b, T *r, int rows, int cols, int pu, int pb, int pr, T *resid,
                       void *stream) {
    MPX_CHECK_ARG(u && r, "null pointer");
    MPX_CHECK_ARG(rows >= 3 && cols >= 3 && pu >= cols && pr >= cols && (!b || pb >= cols), "bad grid geometry");
    const bool vec = mg_vec<T>({u, b, r}, {pu, b ? pb : 0, pr});
    const int lanes = vec ? (cols + JVec<T>::n - 1) / JVec<T>::n : cols;
    const int rpl = mg_rows_per_lane(lanes, rows - 2, kMgRows);
    const dim3 blk(256), grd((lanes + 255) / 256, (rows - 2 + rpl - 1) / rpl);
    auto go = [&](auto vc, auto rc) {
        hipLaunchKernelGGL((mg_residual_kernel<T, decltype(vc)::value, decltype(rc)::value>), grd, blk, 0,
                           as_stream(stream), u, b, r, rows, cols, pu, pb, pr, rpl, resid);
    };
    if (vec) {
        if (b) go(std::true_type{}, std::true_type{});
        else go(std::true_type{}, std::false_type{});
    } else {
        if (b) go(std::false_type{}, std::true_type{});
        else go(std::false_type{}, std::false_type{});
    }
    MPX_RETURN_IF_HIP_ERROR(hipGetLastError());
    return MPX_OK;
}

template <typename T>
int launch_mg_restrict(const T *r, T *bc, int hc, int wc, int pr, int pc, void *stream) {
    MPX_CHECK_ARG(r && bc, "null pointer");
    MPX_CHECK_ARG(hc >= 2 && wc >= 2 && wc < (1 << 29) && hc < (1 << 29) && pr >= 2 * wc - 1 && pc >= wc,
                  "bad grid geometry");
    if (hc < 3 || wc < 3) return MPX_OK;  // no coarse interior
    const bool vec = mg_vec<T>({r, bc}, {pr, pc});
    const int lanes = vec ? (wc + JVec<T>::n - 1) / JVec<T>::n : wc;
    const int rpl = mg_rows_per_lane(lanes, hc - 2, kMgCoarseRows);
    const dim3 blk(256), grd((lanes + 255) / 256, (hc - 2 + rpl - 1) / rpl);
    if (vec) hipLaunchKernelGGL((mg_restrict_kernel<T, true>), grd, blk, 0, as_stream(stream), r, bc, hc, wc, pr, pc, rpl);
    else hipLaunchKernelGGL((mg_restrict_kernel<T, false>), grd, blk, 0, as_stream(stream), r, bc, hc, wc, pr, pc, rpl);
    MPX_RETURN_IF_HIP_ERROR(hipGetLastError());
    return MPX_OK;
}

template <typename T>
int launch_mg_prolong(const T *e, T *u, int hc, int wc, int pe, int pu, void *stream) {
    MPX_CHECK_ARG(e && u, "null pointer");
    MPX_CHECK_ARG(hc >= 2 && wc >= 2 && wc < (1 << 29) && hc < (1 << 29) && pe >= wc && pu >= 2 * wc - 1,
                  "bad grid geometry");
    const bool vec = mg_vec<T>({e, u}, {pe, pu});
    const int lanes = vec ? (wc + JVec<T>::n - 1) / JVec<T>::n : wc;
    const int rpl = mg_rows_per_lane(lanes, hc - 1, kMgCoarseRows);
    const dim3 blk(256), grd((lanes + 255) / 256, (hc - 1 + rpl - 1) / rpl);
    if (vec) hipLaunchKernelGGL((mg_prolong_kernel<T, true>), grd, blk, 0, as_stream(stream), e, u, hc, wc, pe, pu, rpl);
    else hipLaunchKernelGGL((mg_prolong_kernel<T, false>), grd, blk, 0, as_stream(stream), e, u, hc, wc, pe, pu, rpl);
    MPX_RETURN_IF_HIP_ERROR(hipGetLastError());
    return MPX_OK;
}

}  // namespace
MPX_MODULE_ANCHOR(multigrid)

}  // namespace mpx

extern "C" int mpx_mg_residual_f64(const double *u, const double *b, double *r, int rows, int cols, int pitch_u,
                                   int pitch_b, int pitch_r, double *resid, void *stream) {
    return mpx::launch_mg_residual<double>(u, b, r, rows, cols, pitch_u, pitch_b, pitch_r, resid, stream);
}

extern "C" int mpx_mg_residual_f32(const float *u, const float *b, float *r, int rows, int cols, int pitch_u,
                                   int pitch_b, int pitch_r, float *resid, void *stream) {
    return mpx::launch_mg_residual<float>(u, b, r, rows, cols, pitch_u, pitch_b, pitch_r, resid, stream);
}

extern "C" int mpx_mg_restrict_f64(const double *r, double *bc, int hc, int wc, int pitch_r, int pitch_bc,
                                   void *stream) {
    return mpx::launch_mg_restrict<double>(r, bc, hc, wc, pitch_r, pitch_bc, stream);
}

extern "C" int mpx_mg_restrict_f32(const float *r, float *bc, int hc, int wc, int pitch_r, int pitch_bc, void *stream) {
    return mpx::launch_mg_restrict<float>(r, bc, hc, wc, pitch_r, pitch_bc, stream);
}

extern "C" int mpx_mg_prolong_add_f64(const double *e, double *u, int hc, int wc, int pitch_e, int pitch_u,
                                      void *stream) {
    return mpx::launch_mg_prolong<double>(e, u, hc, wc, pitch_e, pitch_u, stream);
}

extern "C" int mpx_mg_prolong_add_f32(const float *e, float *u, int hc, int wc, int pitch_e, int pitch_u, void *stream) {
    return mpx::launch_mg_prolong<float>(e, u, hc, wc, pitch_e, pitch_u, stream);
}
