// Grid-transfer and residual kernels of the geometric multigrid V-cycle for the
// 2-D Poisson solver (models.PoissonMultigrid). The smoother is the damped
// Jacobi sweep of jacobi.hip (mpx_jacobi_relax_*).
//
// Layout: an (H, W) grid with Dirichlet values in rows 0 / H-1 and columns
// 0 / W-1; its coarse grid is (Hc, Wc) with H = 2 Hc - 1, W = 2 Wc - 1 and
// coarse point (I, J) on fine point (2I, 2J). Every tensor has its own row
// pitch (elements); padding is never read and never written.
//
// MI355X design: the kernels are HBM-bound (residual 3, restrict 1.25,
// prolong-add 2.25, cubic prolong 1.25 words per fine point), so
//   * a lane owns one 16-B vector of the narrower grid per row (residual: of
//     u; restrict and prolong: of the coarse grid, and with it the two fine
//     vectors below it) and walks a block of rows down, so every input row is
//     fetched once and the rows shared by two output rows stay in registers
//     (a launch too small to fill the device that way shortens its walks:
//     mg_rows_per_lane, profiles/multigrid.md);
//   * the even/odd column interleave of the transfers happens inside the lane
//     (coarse vector k <-> fine elements 2k, 2k+1 of the lane's vector pair);
//     the one element a lane needs from its neighbour (the cubic prolongation:
//     one from the left, two from the right) comes through a DPP wave shift,
//     and only lanes 0 / 63 of a wave load it themselves — no strided global
//     access;
//   * the VEC = false form (one element per lane, scalar loads) serves bases
//     and pitches that are not 16-byte multiples, as jacobi_kernel<T, false>;
//   * every + - * is one rounded operation (-ffp-contract=off), in the order
//     written in capi.h; the factors 4, 0.5, 0.25 and 0.125 are exact.
#include "mg_lane.hpp"

namespace mpx {
namespace {

constexpr int kMgRows = 16;       // rows of the residual walked per lane
constexpr int kMgCoarseRows = 8;  // coarse rows walked per lane by the transfers
// and by the cubic prolongation: 8193^2 measured fastest at 2 in both dtypes (fp64
// 223 us against 262 / 234 / 253 / 270 at 1 / 4 / 8 / 16: profiles/multigrid.md)
constexpr int kMgCubicRows = 2;
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

// cubic interpolation of the coarse c written to the fine interior of u (the
// FMG interpolant). A lane owns the coarse columns [J0, J0 + NV) and the fine
// columns [2 J0, 2 J0 + 2 NV) below them. A coarse row is interpolated along
// the row as it is fetched (ev: the fine columns 2J, od: 2J + 1); the lane
// lacks c[J0 - 1], c[J0 + NV] and c[J0 + NV + 1], which come from its
// neighbours by wave shifts. A block walks R coarse rows: it fetches the rows
// I0 - 1 .. I0 + R + 1 in one group of loads, each once, and keeps them
// interpolated in registers; fine row 2I is row I, fine row 2I + 1 the cubic
// midpoint of the rows I - 1 .. I + 2. The ghost columns c[-1] and c[wc] are
// computed by every lane from the ends of the row (uniform addresses) and
// selected by column; the ghost rows -1 and hc are formed from the
// interpolated rows under block-uniform conditions
template <typename T, bool VEC, int R>
__global__ __launch_bounds__(256) void mg_prolong_cubic_kernel(const T *__restrict__ c, T *__restrict__ u, int hc,
                                                               int wc, int pc, int pu) {
    constexpr int NV = VEC ? JVec<T>::n : 1;
    constexpr int M = R + 3;
    const int J0 = NV * (blockIdx.x * blockDim.x + threadIdx.x);
    const int f0 = 2 * J0;
    const int w = 2 * wc - 1;
    const int I0 = blockIdx.y * R;
    const bool wcubic = wc >= 4, hcubic = hc >= 4;
    // slot q holds row I0 - 1 + q. Where that is a ghost row the slot fetches the
    // fourth row the ghost is made of: row 3 for row -1, row hc - 4 for row hc
    // (three rows: any row, it is not used); rows past hc belong to no step
    const T *rows[M];
    int cols[M];
#pragma unroll
    for (int q = 0; q < M; ++q) {
        const int r = I0 - 1 + q;
        const int src = r < 0 ? min(3, hc - 1) : (r == hc ? max(hc - 4, 0) : min(r, hc - 1));
        rows[q] = c + (int64_t)src * pc;
        cols[q] = wc;
    }
    T own[M][NV];
    load_rows<T, VEC, NV, M>(rows, J0, cols, own);
    T le[M], e1[M], e2[M], hd[M][4], tl[M][4];
#pragma unroll
    for (int q = 0; q < M; ++q) {
        le[q] = left_edge<T>(rows[q], J0, wc);
        e1[q] = right_edge<T>(rows[q], J0 + NV, wc);
        e2[q] = right_edge<T>(rows[q], J0 + NV + 1, wc);
        // both ends of the row, from the end inwards (wc == 3: the fourth is not used)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            hd[q][t] = rows[q][min(t, wc - 1)];
            tl[q][t] = rows[q][max(wc - 1 - t, 0)];
        }
    }
    T ev[M][NV], od[M][NV];
#pragma unroll
    for (int q = 0; q < M; ++q) {
        const T gl = cubic_ghost<T>(wcubic, hd[q][0], hd[q][1], hd[q][2], hd[q][3]);
        const T gr = cubic_ghost<T>(wcubic, tl[q][0], tl[q][1], tl[q][2], tl[q][3]);
        // x[t] = c[J0 - 1 + t], t = 0 .. NV + 2, the ghosts at columns -1 and wc
        T x[NV + 3];
        x[0] = shift_from_left<T>(own[q][NV - 1], le[q]);
#pragma unroll
        for (int k = 0; k < NV; ++k) x[k + 1] = own[q][k];
        x[NV + 1] = shift_from_right<T>(own[q][0], e1[q]);
        // two columns on: the right lane's second element, or (one element per lane) its x[NV + 1]
        if constexpr (NV >= 2) x[NV + 2] = shift_from_right<T>(own[q][1], e2[q]);
        else x[NV + 2] = shift_from_right<T>(x[NV + 1], e2[q]);
#pragma unroll
        for (int t = 0; t < NV + 3; ++t) {
            const int J = J0 - 1 + t;
            x[t] = J == -1 ? gl : (J == wc ? gr : x[t]);
        }
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            ev[q][k] = x[k + 1];
            od[q][k] = cubic_mid<T>(x[k], x[k + 1], x[k + 2], x[k + 3]);
        }
    }
    if (I0 == 0) {  // row -1 from the rows 0, 1, 2 and 3
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            ev[0][k] = cubic_ghost<T>(hcubic, ev[1][k], ev[2][k], ev[3][k], ev[0][k]);
            od[0][k] = cubic_ghost<T>(hcubic, od[1][k], od[2][k], od[3][k], od[0][k]);
        }
    }
#pragma unroll
    for (int q = 3; q < M; ++q) {
        if (I0 - 1 + q == hc) {  // row hc from the rows hc - 1, hc - 2, hc - 3 and hc - 4
#pragma unroll
            for (int k = 0; k < NV; ++k) {
                ev[q][k] = cubic_ghost<T>(hcubic, ev[q - 1][k], ev[q - 2][k], ev[q - 3][k], ev[q][k]);
                od[q][k] = cubic_ghost<T>(hcubic, od[q - 1][k], od[q - 2][k], od[q - 3][k], od[q][k]);
            }
        }
    }
    // fine row i: columns 2J get ev, columns 2J + 1 get od; interior only
    auto put_row = [&](int i, const T(&pe)[NV], const T(&po)[NV]) {
        T *row = u + (int64_t)i * pu;
        T a[2][NV];
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            a[(2 * k) / NV][(2 * k) % NV] = pe[k];
            a[(2 * k + 1) / NV][(2 * k + 1) % NV] = po[k];
        }
        store_n<T, VEC, NV>(row, f0, 1, w - 2, a[0]);
        store_n<T, VEC, NV>(row, f0 + NV, 1, w - 2, a[1]);
    };
#pragma unroll
    for (int s = 0; s < R; ++s) {
        const int I = I0 + s;  // block-uniform
        if (I >= hc - 1) break;
        if (I >= 1) put_row(2 * I, ev[s + 1], od[s + 1]);  // fine row 0 is boundary
        T mv[NV], md[NV];
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            mv[k] = cubic_mid<T>(ev[s][k], ev[s + 1][k], ev[s + 2][k], ev[s + 3][k]);
            md[k] = cubic_mid<T>(od[s][k], od[s + 1][k], od[s + 2][k], od[s + 3][k]);
        }
        put_row(2 * I + 1, mv, md);
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

template <typename T>
int launch_mg_prolong_cubic(const T *c, T *u, int hc, int wc, int pc, int pu, void *stream) {
    MPX_CHECK_ARG(c && u, "null pointer");
    MPX_CHECK_ARG(hc >= 3 && wc >= 3 && wc < (1 << 29) && hc < (1 << 29) && pc >= wc && pu >= 2 * wc - 1,
                  "bad grid geometry");
    const bool vec = mg_vec<T>({c, u}, {pc, pu});
    const int lanes = vec ? (wc + JVec<T>::n - 1) / JVec<T>::n : wc;
    const int rpl = mg_rows_per_lane(lanes, hc - 1, kMgCubicRows);
    const dim3 blk(256), grd((lanes + 255) / 256, (hc - 1 + rpl - 1) / rpl);
    auto go = [&](auto vc, auto rc) {
        hipLaunchKernelGGL((mg_prolong_cubic_kernel<T, decltype(vc)::value, decltype(rc)::value>), grd, blk, 0,
                           as_stream(stream), c, u, hc, wc, pc, pu);
    };
    using R1 = std::integral_constant<int, 1>;
    using R2 = std::integral_constant<int, kMgCubicRows>;
    if (vec) {
        if (rpl == 1) go(std::true_type{}, R1{});
        else go(std::true_type{}, R2{});
    } else {
        if (rpl == 1) go(std::false_type{}, R1{});
        else go(std::false_type{}, R2{});
    }
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

extern "C" int mpx_mg_prolong_cubic_f64(const double *c, double *u, int hc, int wc, int pitch_c, int pitch_u,
                                        void *stream) {
    return mpx::launch_mg_prolong_cubic<double>(c, u, hc, wc, pitch_c, pitch_u, stream);
}

extern "C" int mpx_mg_prolong_cubic_f32(const float *c, float *u, int hc, int wc, int pitch_c, int pitch_u,
                                        void *stream) {
    return mpx::launch_mg_prolong_cubic<float>(c, u, hc, wc, pitch_c, pitch_u, stream);
}
