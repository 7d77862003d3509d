// Smoother, residual and grid-transfer kernels of the geometric multigrid
// V-cycle for the 3-D Poisson solver (models.PoissonMultigrid3D). The contracts
// (association order, what is read and written) are in capi.h.
//
// Layout: a (D, H, W) grid, x fastest, Dirichlet values on all six faces; its
// coarse grid is (Dc, Hc, Wc) with D = 2 Dc - 1, H = 2 Hc - 1, W = 2 Wc - 1 and
// coarse point (K, J, I) on fine point (2K, 2J, 2I). Every tensor has its own
// row pitch and plane stride (elements; plane offsets are 64-bit); padding is
// never read and never written.
//
// MI355X design: all five kernels are HBM-bound (relax 3, residual 3, restrict
// 1.125, prolong-add 2.125, cubic prolong 1.125 words per fine point), the shape
// is multigrid.hip's one dimension up:
//   * a workgroup is 4 waves of 64 lanes in x; a lane owns one 16-B vector of
//     the narrower grid per row (relax, residual: of u; restrict and prolong: of
//     the coarse grid, and with it the two fine vectors below it), so the
//     even/odd interleave of the transfers stays inside the lane and the one
//     element a lane lacks in x comes through a DPP wave shift (mg_lane.hpp);
//   * relax and residual are one kernel with two epilogues. A wave walks a block
//     of rows of one plane with the plane's three rows in registers; the rows
//     of planes k - 1 and k + 1 are two more load streams (the "rows" form of
//     profiles/jacobi3d.md). The four waves of a workgroup own consecutive row
//     blocks; workgroups run along x, then y, then z, so the re-reads of the
//     neighbouring planes meet in L2 / Infinity Cache;
//   * the transfers walk down z: a wave owns one coarse row J and a block of
//     coarse planes. Restriction keeps the in-plane result of fine plane 2K + 1
//     for coarse plane K + 1; prolongation keeps the two coarse rows of plane
//     K + 1. The rows shared between neighbouring J are re-read by the next wave
//     of the same workgroup. The cubic prolongation (full multigrid) keeps the
//     in-plane interpolated fine rows 2J and 2J + 1 of the four coarse planes
//     K - 1 .. K + 2 (fp64: 16 vectors), fetches the coarse rows J - 1 .. J + 2
//     of one new plane per step and stores every fine point once. That state
//     costs registers (fp64: 158 VGPRs, three waves per SIMD), and the kernel
//     runs at half of prolong-add's rate for half its bytes
//     (profiles/multigrid3d.md);
//   * all loads of a step (relax: the four streams of a row; restrict: the six
//     vectors of a fine plane; prolong: the coarse rows, then the fine rows of a
//     plane; cubic prolong: the four coarse rows of a plane) go through one
//     load_rows group, issued back to back and waited for once; load_n row by
//     row costs a full memory latency per load;
//   * a launch too small to fill the device shortens its walks (mg3_walk). The
//     walks are short anyway: longer ones measured slower (profiles/multigrid3d.md);
//   * known cost: a row of 2^n + 1 elements ends in a wave with one active lane
//     (relax at 513^3 fp64: 761 us against 661 us at width 512);
//   * the VEC = false form (one element per lane) serves bases and strides that
//     are not 16-byte multiples;
//   * every + - * is one rounded operation (-ffp-contract=off), in the order
//     written in capi.h; the factors 6, 0.5, 0.25 and 0.125 are exact.
#include "mg_lane.hpp"

#include <climits>
#include <cstdio>
#include <cstdlib>
#include <limits>

namespace mpx {
namespace {

constexpr int kMg3Waves = 4;  // waves (rows of the stencil walk, coarse rows of the transfers) per workgroup

// rows walked per lane by relax / residual, coarse planes walked per lane by the
// restriction and by the prolongation, and the wave count below which a launch
// halves its walk (profiles/multigrid3d.md).
// MPX_MG3_WALK="rows,restrict_planes,prolong_planes,min_waves" replaces them for
// A/B measurements; read once per process.
struct Mg3Walk {
    int rows = 4, restrict_planes = 4, prolong_planes = 2, min_waves = 8192;
};

// coarse planes walked per lane by the cubic prolongation: a block of R planes
// fetches R + 3, so the walk is longer than the other transfers'.
// MPX_MG3_CUBIC_WALK="planes" replaces it for A/B measurements; min_waves is
// Mg3Walk's.
inline int mg3_cubic_planes() {
    static const int planes = [] {
        int v = 8;
        if (const char *s = std::getenv("MPX_MG3_CUBIC_WALK")) {
            int a = 0;
            if (std::sscanf(s, "%d", &a) == 1 && a >= 1 && a <= 64) v = a;
        }
        return v;
    }();
    return planes;
}

inline const Mg3Walk &mg3_walk_config() {
    static const Mg3Walk w = [] {
        Mg3Walk v;
        if (const char *s = std::getenv("MPX_MG3_WALK")) {
            int a = 0, b = 0, c = 0, d = 0;
            const auto ok = [](int x) { return x >= 1 && x <= 64; };
            if (std::sscanf(s, "%d,%d,%d,%d", &a, &b, &c, &d) == 4 && ok(a) && ok(b) && ok(c) && d >= 1) {
                v.rows = a;
                v.restrict_planes = b;
                v.prolong_planes = c;
                v.min_waves = d;
            }
        }
        return v;
    }();
    return w;
}

// the walk of a launch with `across` waves per walked block and `along` steps to walk
inline int mg3_walk(int64_t across, int along, int most) {
    const int64_t min_waves = mg3_walk_config().min_waves;
    int r = most;
    while (r > 1 && across * ((along + r - 1) / r) < min_waves) r >>= 1;
    return r;
}

// relax (RELAX): out = c + omega * (s - c) with s = (n [+ b]) * (1/6) at the
// interior points of plane k0 + ..., boundary rows and columns copied through,
// max|s - c| folded into resid. residual (!RELAX): out = (n [+ b]) - 6 c at the
// interior points only, max|out| folded. n = ((zm + zp) + (ym + yp)) + (xm + xp).
template <typename T, bool VEC, bool RHS, bool RELAX>
__global__ __launch_bounds__(64 * kMg3Waves) void mg3_stencil_kernel(
    const T *__restrict__ u, const T *__restrict__ b, T *__restrict__ out, int ny, int nx, int pu, int64_t su, int pb,
    int64_t sb, int po, int64_t so, int k0, int nxb, int nyb, int rpl, T omega, T *__restrict__ resid) {
    constexpr int NV = VEC ? JVec<T>::n : 1;
    const unsigned bid = blockIdx.x;
    const int xb = (int)(bid % (unsigned)nxb);
    const unsigned t = bid / (unsigned)nxb;
    const int yb = (int)(t % (unsigned)nyb);
    const int64_t k = k0 + (int64_t)(t / (unsigned)nyb);
    const int j0 = NV * (xb * 64 + (int)threadIdx.x);
    const int i0 = 1 + (yb * kMg3Waves + (int)threadIdx.y) * rpl;  // wave-uniform: the whole wave walks the rows
    if (i0 >= ny - 1) return;
    const int i1 = min(i0 + rpl, ny - 1);
    const T *uk = u + k * su;
    const T *bk = RHS ? b + k * sb : nullptr;
    T *ok = out + k * so;
    T rmax = (T)0;
    T up[NV], cen[NV];
    load_n<T, VEC, NV>(uk + (int64_t)(i0 - 1) * pu, j0, nx, up);
    load_n<T, VEC, NV>(uk + (int64_t)i0 * pu, j0, nx, cen);
    if constexpr (RELAX) {
        if (i0 == 1) store_n<T, VEC, NV>(ok, j0, 0, nx - 1, up);  // row 0 copies through
    }
    constexpr int M = RHS ? 4 : 3;  // the load streams of a row: row i + 1, planes k - 1 and k + 1, b
    int cols[M];
#pragma unroll
    for (int m = 0; m < M; ++m) cols[m] = nx;
    for (int i = i0; i < i1; ++i) {
        const T *crow = uk + (int64_t)i * pu;
        const T *rows[M];
        rows[0] = crow + pu;
        rows[1] = crow - su;
        rows[2] = crow + su;
        if constexpr (RHS) rows[3] = bk + (int64_t)i * pb;
        T g[M][NV];
        load_rows<T, VEC, NV, M>(rows, j0, cols, g);
        const T le = left_edge<T>(crow, j0, nx);
        const T re = right_edge<T>(crow, j0 + NV, nx);
        const T left = shift_from_left<T>(cen[NV - 1], le);
        const T right = shift_from_right<T>(cen[0], re);
        T(&dn)[NV] = g[0];
        T(&zm)[NV] = g[1];
        T(&zp)[NV] = g[2];
        T(&src)[NV] = g[M - 1];  // b with RHS
        T res[NV];
#pragma unroll
        for (int e = 0; e < NV; ++e) {
            const int j = j0 + e;
            const T l = e == 0 ? left : cen[e - 1];
            const T rt = e == NV - 1 ? right : cen[e + 1];
            T n = ((zm[e] + zp[e]) + (up[e] + dn[e])) + (l + rt);
            if constexpr (RHS) n = n + src[e];
            const bool interior = j > 0 && j < nx - 1;
            T a;
            if constexpr (RELAX) {
                const T s = n * (T)(1.0 / 6.0);
                const T d = s - cen[e];
                const T w = omega * d;
                res[e] = interior ? cen[e] + w : cen[e];
                a = d < (T)0 ? -d : d;
            } else {
                const T c6 = (T)6 * cen[e];
                res[e] = n - c6;
                a = res[e] < (T)0 ? -res[e] : res[e];
            }
            if (interior) rmax = a > rmax ? a : rmax;
        }
        if constexpr (RELAX) store_n<T, VEC, NV>(ok + (int64_t)i * po, j0, 0, nx - 1, res);
        else store_n<T, VEC, NV>(ok + (int64_t)i * po, j0, 1, nx - 2, res);
#pragma unroll
        for (int e = 0; e < NV; ++e) {
            up[e] = cen[e];
            cen[e] = dn[e];
        }
    }
    if constexpr (RELAX) {
        if (i1 == ny - 1) store_n<T, VEC, NV>(ok + (int64_t)(ny - 1) * po, j0, 0, nx - 1, cen);  // row ny - 1
    }
    if (resid) {
        using B = typename JVec<T>::bits;
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const T o = __shfl_xor(rmax, m);
            rmax = o > rmax ? o : rmax;
        }
        if (threadIdx.x == 0 && rmax > (T)0) residual_max(reinterpret_cast<B *>(resid), __builtin_bit_cast(B, rmax));
    }
}

// 27-point full weighting, separable: the 2-D rule of mg_restrict_kernel in each
// fine plane (P), then (P_2K + (P_2K-1 + P_2K+1) * 0.5) * 0.5 down z. A lane
// owns the coarse columns [I0, I0 + NV) of coarse row J and the fine columns
// [2 I0, 2 I0 + 2 NV) below them.
template <typename T, bool VEC>
__global__ __launch_bounds__(64 * kMg3Waves) void mg3_restrict_kernel(const T *__restrict__ r, T *__restrict__ bc,
                                                                       int dc, int hc, int wc, int pr, int64_t sr,
                                                                       int pc, int64_t sc, int nxb, int njb, int kpl) {
    constexpr int NV = VEC ? JVec<T>::n : 1;
    const unsigned bid = blockIdx.x;
    const int xb = (int)(bid % (unsigned)nxb);
    const unsigned t = bid / (unsigned)nxb;
    const int jb = (int)(t % (unsigned)njb);
    const int kb = (int)(t / (unsigned)njb);
    const int I0 = NV * (xb * 64 + (int)threadIdx.x);
    const int f0 = 2 * I0;
    const int w = 2 * wc - 1;
    const int J = 1 + jb * kMg3Waves + (int)threadIdx.y;  // wave-uniform
    if (J >= hc - 1) return;
    const int K0 = 1 + kb * kpl;
    const int K1 = min(K0 + kpl, dc - 1);
    // P_k[J, I0 ...]: the 2-D full weighting of fine plane k around fine row 2J.
    // Of each of the three fine rows a lane keeps, per coarse column, the centre
    // r[., 2I] and the rounded side sum r[., 2I-1] + r[., 2I+1]; the six vectors
    // are one group of loads
    auto plane = [&](int k, T (&P)[NV]) {
        const T *mid = r + (int64_t)k * sr + (int64_t)(2 * J) * pr;
        const T *rows[6] = {mid - pr, mid - pr + NV, mid, mid + NV, mid + pr, mid + pr + NV};
        const int cols[6] = {w, w - NV, w, w - NV, w, w - NV};
        T a[6][NV];
        load_rows<T, VEC, NV, 6>(rows, f0, cols, a);
        const T le[3] = {left_edge<T>(mid - pr, f0, w), left_edge<T>(mid, f0, w), left_edge<T>(mid + pr, f0, w)};
        T c[3][NV], sd[3][NV];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const T left = shift_from_left<T>(a[2 * q + 1][NV - 1], le[q]);
#pragma unroll
            for (int e = 0; e < NV; ++e) {
                c[q][e] = a[2 * q + (2 * e) / NV][(2 * e) % NV];
                const T lft = e == 0 ? left : a[2 * q + (2 * e - 1) / NV][(2 * e - 1) % NV];
                sd[q][e] = lft + a[2 * q + (2 * e + 1) / NV][(2 * e + 1) % NV];
            }
        }
#pragma unroll
        for (int e = 0; e < NV; ++e) {
            const T ee = (c[0][e] + c[2][e]) + sd[1][e];
            const T d = sd[0][e] + sd[2][e];
            const T eh = ee * (T)0.5;
            const T dq = d * (T)0.25;
            P[e] = (c[1][e] + eh) + dq;
        }
    };
    T lo[NV];
    plane(2 * K0 - 1, lo);
    for (int K = K0; K < K1; ++K) {
        T mid[NV], hi[NV], res[NV];
        plane(2 * K, mid);
        plane(2 * K + 1, hi);
#pragma unroll
        for (int e = 0; e < NV; ++e) {
            const T z = lo[e] + hi[e];
            const T zh = z * (T)0.5;
            const T v = mid[e] + zh;
            res[e] = v * (T)0.5;
            lo[e] = hi[e];
        }
        store_n<T, VEC, NV>(bc + (int64_t)K * sc + (int64_t)J * pc, I0, 1, wc - 2, res);
    }
}

// trilinear interpolation of the coarse e, added to the fine interior of u in
// place: unscaled pair sums in z, then y, then x, one exact scale at the end. A
// lane owns the coarse columns [I0, I0 + NV] (the last from its right
// neighbour) of the coarse rows J and J + 1 and reads and writes only its own
// fine columns [2 I0, 2 I0 + 2 NV) of the fine rows 2J, 2J + 1.
template <typename T, bool VEC>
__global__ __launch_bounds__(64 * kMg3Waves) void mg3_prolong_kernel(const T *__restrict__ e, T *__restrict__ u, int dc,
                                                                      int hc, int wc, int pe, int64_t se, int pu,
                                                                      int64_t su, int nxb, int njb, int kpl) {
    constexpr int NV = VEC ? JVec<T>::n : 1;
    const unsigned bid = blockIdx.x;
    const int xb = (int)(bid % (unsigned)nxb);
    const unsigned t = bid / (unsigned)nxb;
    const int jb = (int)(t % (unsigned)njb);
    const int kb = (int)(t / (unsigned)njb);
    const int I0 = NV * (xb * 64 + (int)threadIdx.x);
    const int f0 = 2 * I0;
    const int w = 2 * wc - 1;
    const int J = jb * kMg3Waves + (int)threadIdx.y;  // wave-uniform
    if (J >= hc - 1) return;
    const int K0 = kb * kpl;
    const int K1 = min(K0 + kpl, dc - 1);
    // coarse rows J and J + 1 of coarse plane K, columns [I0, I0 + NV]: one group of loads
    auto fetch = [&](int K, T (&c0)[NV + 1], T (&c1)[NV + 1]) {
        const T *r0 = e + (int64_t)K * se + (int64_t)J * pe;
        const T *rows[2] = {r0, r0 + pe};
        const int cols[2] = {wc, wc};
        T own[2][NV];
        load_rows<T, VEC, NV, 2>(rows, I0, cols, own);
        const T e0 = right_edge<T>(rows[0], I0 + NV, wc);
        const T e1 = right_edge<T>(rows[1], I0 + NV, wc);
#pragma unroll
        for (int q = 0; q < NV; ++q) {
            c0[q] = own[0][q];
            c1[q] = own[1][q];
        }
        c0[NV] = shift_from_right<T>(own[0][0], e0);
        c1[NV] = shift_from_right<T>(own[1][0], e1);
    };
    // a fine row held in a[base], a[base + 1]: columns 2I get Y[I], columns
    // 2I + 1 get Y[I] + Y[I + 1], scaled by 0.5 per odd coordinate (ODD: of the
    // row's plane and row index)
    auto add_row = [&](auto &a, int base, const T (&Y)[NV + 1], auto odd) {
        constexpr int ODD = decltype(odd)::value;
        constexpr T fe = ODD == 0 ? (T)1 : (ODD == 1 ? (T)0.5 : (T)0.25);
        constexpr T fo = fe * (T)0.5;
#pragma unroll
        for (int q = 0; q < NV; ++q) {
            T ev = Y[q];
            if constexpr (ODD != 0) ev = ev * fe;
            const T x = Y[q] + Y[q + 1];
            const T od = x * fo;
            a[base + (2 * q) / NV][(2 * q) % NV] = a[base + (2 * q) / NV][(2 * q) % NV] + ev;
            a[base + (2 * q + 1) / NV][(2 * q + 1) % NV] = a[base + (2 * q + 1) / NV][(2 * q + 1) % NV] + od;
        }
    };
    // fine plane k from its z sums Z0 (coarse row J) and Z1 (coarse row J + 1):
    // fine rows 2J (Y = Z0; row 0 is boundary) and 2J + 1 (Y = Z0 + Z1), their
    // vectors of u loaded as one group
    auto add_plane = [&](int k, const T (&Z0)[NV + 1], const T (&Z1)[NV + 1], auto zodd) {
        constexpr int ZODD = decltype(zodd)::value;
        T *row1 = u + (int64_t)k * su + (int64_t)(2 * J + 1) * pu;
        T Y[NV + 1];
#pragma unroll
        for (int q = 0; q <= NV; ++q) Y[q] = Z0[q] + Z1[q];
        if (J >= 1) {
            T *row0 = row1 - pu;
            const T *rows[4] = {row0, row0 + NV, row1, row1 + NV};
            const int cols[4] = {w, w - NV, w, w - NV};
            T a[4][NV];
            load_rows<T, VEC, NV, 4>(rows, f0, cols, a);
            add_row(a, 0, Z0, std::integral_constant<int, ZODD>{});
            add_row(a, 2, Y, std::integral_constant<int, ZODD + 1>{});
            store_n<T, VEC, NV>(row0, f0, 1, w - 2, a[0]);
            store_n<T, VEC, NV>(row0, f0 + NV, 1, w - 2, a[1]);
            store_n<T, VEC, NV>(row1, f0, 1, w - 2, a[2]);
            store_n<T, VEC, NV>(row1, f0 + NV, 1, w - 2, a[3]);
        } else {
            const T *rows[2] = {row1, row1 + NV};
            const int cols[2] = {w, w - NV};
            T a[2][NV];
            load_rows<T, VEC, NV, 2>(rows, f0, cols, a);
            add_row(a, 0, Y, std::integral_constant<int, ZODD + 1>{});
            store_n<T, VEC, NV>(row1, f0, 1, w - 2, a[0]);
            store_n<T, VEC, NV>(row1, f0 + NV, 1, w - 2, a[1]);
        }
    };
    T a0[NV + 1], a1[NV + 1];
    fetch(K0, a0, a1);
    for (int K = K0; K < K1; ++K) {
        T n0[NV + 1], n1[NV + 1];
        fetch(K + 1, n0, n1);
        if (K >= 1) add_plane(2 * K, a0, a1, std::integral_constant<int, 0>{});  // fine plane 0 is boundary
        T z0[NV + 1], z1[NV + 1];
#pragma unroll
        for (int q = 0; q <= NV; ++q) {
            z0[q] = a0[q] + n0[q];
            z1[q] = a1[q] + n1[q];
            a0[q] = n0[q];
            a1[q] = n1[q];
        }
        add_plane(2 * K + 1, z0, z1, std::integral_constant<int, 1>{});
    }
}

// tricubic interpolation of the coarse c written to the fine interior of u (the
// FMG interpolant): mg_prolong_cubic_kernel's rule in every coarse plane, then
// the same 1-D rule down z through the interpolated planes. A lane owns the
// coarse columns [I0, I0 + NV) and the fine columns [2 I0, 2 I0 + 2 NV) below
// them, a wave the coarse rows J - 1 .. J + 2 and with them the fine rows 2J and
// 2J + 1. plane() fetches those four rows of one coarse plane in one group of
// loads, interpolates each along x (c[I0 - 1], c[I0 + NV] and c[I0 + NV + 1]
// come from the neighbouring lanes by wave shifts, the ghost columns -1 and wc
// from the ends of the row in the workgroups that hold them), forms the ghost
// row -1 or hc from the interpolated rows and leaves the two fine rows of the
// plane: q[0] = fine row 2J, q[1] = fine row 2J + 1, each as the lane's two fine
// vectors. The march keeps them for the coarse planes K - 1 .. K + 2: fine plane
// 2K is plane K's rows, fine plane 2K + 1 the midpoints of the four. The ghost
// planes -1 and dc are formed element by element from the interpolated planes;
// their slot first fetches the fourth plane the ghost is made of. All row,
// plane and ghost conditions are wave-uniform.
template <typename T, bool VEC>
__global__ __launch_bounds__(64 * kMg3Waves) void mg3_prolong_cubic_kernel(const T *__restrict__ c, T *__restrict__ u,
                                                                            int dc, int hc, int wc, int pc, int64_t sc,
                                                                            int pu, int64_t su, int nxb, int njb,
                                                                            int kpl) {
    constexpr int NV = VEC ? JVec<T>::n : 1;
    const unsigned bid = blockIdx.x;
    const int xb = (int)(bid % (unsigned)nxb);
    const unsigned t = bid / (unsigned)nxb;
    const int jb = (int)(t % (unsigned)njb);
    const int kb = (int)(t / (unsigned)njb);
    const int I0 = NV * (xb * 64 + (int)threadIdx.x);
    const int f0 = 2 * I0;
    const int w = 2 * wc - 1;
    const int J = jb * kMg3Waves + (int)threadIdx.y;  // wave-uniform
    if (J >= hc - 1) return;
    const int K0 = kb * kpl;
    const int K1 = min(K0 + kpl, dc - 1);
    const bool wcubic = wc >= 4, hcubic = hc >= 4, dcubic = dc >= 4;
    // the waves whose lanes see column -1 / column wc (block-uniform)
    const bool at_left = xb == 0, at_right = NV * (xb * 64 + 64) + 1 >= wc;
    // slot s holds coarse row J - 1 + s. Where that is a ghost row the slot fetches
    // the fourth row the ghost is made of: row 3 for row -1, row hc - 4 for row hc
    // (three rows: any row, it is not used)
    int64_t roff[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int r = J - 1 + s;
        const int src = r < 0 ? min(3, hc - 1) : (r == hc ? max(hc - 4, 0) : r);
        roff[s] = (int64_t)src * pc;
    }
    auto plane = [&](int P, T (&q)[2][2][NV]) {
        const T *base = c + (int64_t)P * sc;
        const T *rows[4];
        int cols[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            rows[s] = base + roff[s];
            cols[s] = wc;
        }
        T own[4][NV];
        load_rows<T, VEC, NV, 4>(rows, I0, cols, own);
        T le[4], e1[4], e2[4], gl[4], gr[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            le[s] = left_edge<T>(rows[s], I0, wc);
            e1[s] = right_edge<T>(rows[s], I0 + NV, wc);
            e2[s] = right_edge<T>(rows[s], I0 + NV + 1, wc);
            gl[s] = gr[s] = (T)0;
        }
        // the ghost columns, from the ends of the row inwards (wc == 3: the fourth is not used)
        if (at_left) {
#pragma unroll
            for (int s = 0; s < 4; ++s)
                gl[s] = cubic_ghost<T>(wcubic, rows[s][0], rows[s][1], rows[s][2], rows[s][min(3, wc - 1)]);
        }
        if (at_right) {
#pragma unroll
            for (int s = 0; s < 4; ++s)
                gr[s] = cubic_ghost<T>(wcubic, rows[s][wc - 1], rows[s][wc - 2], rows[s][wc - 3], rows[s][max(wc - 4, 0)]);
        }
        // f[s]: row J - 1 + s interpolated along x, the lane's 2 NV fine columns
        T f[4][2 * NV];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            // x[m] = c[I0 - 1 + m], m = 0 .. NV + 2, the ghosts at columns -1 and wc
            T x[NV + 3];
            x[0] = shift_from_left<T>(own[s][NV - 1], le[s]);
#pragma unroll
            for (int k = 0; k < NV; ++k) x[k + 1] = own[s][k];
            x[NV + 1] = shift_from_right<T>(own[s][0], e1[s]);
            // two columns on: the right lane's second element, or (one element per lane) its x[NV + 1]
            if constexpr (NV >= 2) x[NV + 2] = shift_from_right<T>(own[s][1], e2[s]);
            else x[NV + 2] = shift_from_right<T>(x[NV + 1], e2[s]);
#pragma unroll
            for (int m = 0; m < NV + 3; ++m) {
                const int I = I0 - 1 + m;
                x[m] = I == -1 ? gl[s] : (I == wc ? gr[s] : x[m]);
            }
#pragma unroll
            for (int k = 0; k < NV; ++k) {
                f[s][2 * k] = x[k + 1];
                f[s][2 * k + 1] = cubic_mid<T>(x[k], x[k + 1], x[k + 2], x[k + 3]);
            }
        }
        if (J == 0) {  // row -1 from the rows 0, 1, 2 and 3
#pragma unroll
            for (int e = 0; e < 2 * NV; ++e) f[0][e] = cubic_ghost<T>(hcubic, f[1][e], f[2][e], f[3][e], f[0][e]);
        }
        if (J + 2 == hc) {  // row hc from the rows hc - 1, hc - 2, hc - 3 and hc - 4
#pragma unroll
            for (int e = 0; e < 2 * NV; ++e) f[3][e] = cubic_ghost<T>(hcubic, f[2][e], f[1][e], f[0][e], f[3][e]);
        }
#pragma unroll
        for (int e = 0; e < 2 * NV; ++e) {
            q[0][e / NV][e % NV] = f[1][e];
            q[1][e / NV][e % NV] = cubic_mid<T>(f[0][e], f[1][e], f[2][e], f[3][e]);
        }
    };
    // fine plane k, rows 2J (row 0 is boundary) and 2J + 1; interior only
    auto put = [&](int k, const T (&q)[2][2][NV]) {
        T *row0 = u + (int64_t)k * su + (int64_t)(2 * J) * pu;
        if (J >= 1) {
            store_n<T, VEC, NV>(row0, f0, 1, w - 2, q[0][0]);
            store_n<T, VEC, NV>(row0, f0 + NV, 1, w - 2, q[0][1]);
        }
        store_n<T, VEC, NV>(row0 + pu, f0, 1, w - 2, q[1][0]);
        store_n<T, VEC, NV>(row0 + pu, f0 + NV, 1, w - 2, q[1][1]);
    };
    // one step of the march: a, b, c hold the coarse planes K - 1 (plane -1: the
    // slot starts as plane 3), K and K + 1; d receives plane K + 2 (plane dc: the
    // slot starts as plane dc - 4). The four sets rotate by name, not by copies
    auto step = [&](int K, T (&a)[2][2][NV], const T (&b)[2][2][NV], const T (&cc)[2][2][NV], T (&d)[2][2][NV]) {
        T mid[2][2][NV];
        plane(K + 2 == dc ? max(dc - 4, 0) : K + 2, d);
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int v = 0; v < 2; ++v)
#pragma unroll
                for (int e = 0; e < NV; ++e) {
                    if (K == 0) a[r][v][e] = cubic_ghost<T>(dcubic, b[r][v][e], cc[r][v][e], d[r][v][e], a[r][v][e]);
                    if (K + 2 == dc) d[r][v][e] = cubic_ghost<T>(dcubic, cc[r][v][e], b[r][v][e], a[r][v][e], d[r][v][e]);
                    mid[r][v][e] = cubic_mid<T>(a[r][v][e], b[r][v][e], cc[r][v][e], d[r][v][e]);
                }
        if (K >= 1) put(2 * K, b);  // fine plane 0 is boundary
        put(2 * K + 1, mid);
    };
    T q0[2][2][NV], q1[2][2][NV], q2[2][2][NV], q3[2][2][NV];
    plane(K0 == 0 ? min(3, dc - 1) : K0 - 1, q0);
    plane(K0, q1);
    plane(K0 + 1, q2);
    for (int K = K0; K < K1; K += 4) {
        step(K, q0, q1, q2, q3);
        if (K + 1 >= K1) break;
        step(K + 1, q1, q2, q3, q0);
        if (K + 2 >= K1) break;
        step(K + 2, q2, q3, q0, q1);
        if (K + 3 >= K1) break;
        step(K + 3, q3, q0, q1, q2);
    }
}

inline bool mg3_strides_ok(int h, int w, int pitch, int64_t plane) {
    return pitch >= w && plane >= (int64_t)h * pitch;
}

template <typename T>
bool mg3_vec(std::initializer_list<const void *> ptrs, std::initializer_list<int> pitches,
             std::initializer_list<int64_t> planes) {
    if (!mg_vec<T>(ptrs, pitches)) return false;
    for (int64_t s : planes)
        if (s % JVec<T>::n) return false;
    return true;
}

template <typename T, bool RELAX>
int launch_mg3_stencil(const T *u, const T *b, T *out, int d, int ny, int nx, int pu, int64_t su, int pb, int64_t sb,
                       int po, int64_t so, int k0, int k1, double omega_d, T *resid, void *stream) {
    MPX_CHECK_ARG(u && out, "null pointer");
    MPX_CHECK_ARG(nx >= 3 && ny >= 3 && d >= 3 && k0 >= 1 && k1 >= k0 && k1 <= d - 1, "bad grid geometry");
    MPX_CHECK_ARG(mg3_strides_ok(ny, nx, pu, su) && mg3_strides_ok(ny, nx, po, so) && (!b || mg3_strides_ok(ny, nx, pb, sb)),
                  "bad strides (pitch >= W, plane stride >= H * pitch)");
    T omega = (T)1;
    if constexpr (RELAX) {
        const bool w_ok = omega_d > 0.0 && omega_d <= (double)std::numeric_limits<T>::max();
        omega = w_ok ? (T)omega_d : (T)0;
        MPX_CHECK_ARG(omega > (T)0, "omega must be finite and positive");
    }
    if (k1 == k0) return MPX_OK;
    const bool vec = mg3_vec<T>({u, b, out}, {pu, b ? pb : 0, po}, {su, b ? sb : 0, so});
    const int lanes = vec ? (nx + JVec<T>::n - 1) / JVec<T>::n : nx;
    const int nxb = (lanes + 63) / 64;
    const int rpl = mg3_walk((int64_t)nxb * (k1 - k0), ny - 2, mg3_walk_config().rows);
    const int nyb = ((ny - 2 + rpl - 1) / rpl + kMg3Waves - 1) / kMg3Waves;
    const int64_t nblk = (int64_t)nxb * nyb * (k1 - k0);
    MPX_CHECK_ARG(nblk <= INT_MAX, "grid too large for one launch");
    const dim3 blk(64, kMg3Waves), grd((unsigned)nblk);
    auto go = [&](auto vc, auto rc) {
        hipLaunchKernelGGL((mg3_stencil_kernel<T, decltype(vc)::value, decltype(rc)::value, RELAX>), grd, blk, 0,
                           as_stream(stream), u, b, out, ny, nx, pu, su, pb, sb, po, so, k0, nxb, nyb, rpl, omega, resid);
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

inline bool mg3_coarse_ok(int dc, int hc, int wc) {
    return dc >= 2 && hc >= 2 && wc >= 2 && dc < (1 << 29) && hc < (1 << 29) && wc < (1 << 29);
}

// the transfers: one wave per coarse row (restrict: the interior rows; prolong: rows 0 .. hc - 2)
// and block of coarse planes (restrict: of planes 1 .. dc - 2; prolong: of planes 0 .. dc - 2)
template <typename T, bool RESTRICT>
int launch_mg3_transfer(const T *coarse_or_r, T *out, int dc, int hc, int wc, int p_fine, int64_t s_fine, int p_coarse,
                        int64_t s_coarse, void *stream) {
    MPX_CHECK_ARG(coarse_or_r && out, "null pointer");
    MPX_CHECK_ARG(mg3_coarse_ok(dc, hc, wc), "bad grid geometry");
    MPX_CHECK_ARG(mg3_strides_ok(2 * hc - 1, 2 * wc - 1, p_fine, s_fine) && mg3_strides_ok(hc, wc, p_coarse, s_coarse),
                  "bad strides (pitch >= W, plane stride >= H * pitch)");
    if (RESTRICT && (dc < 3 || hc < 3 || wc < 3)) return MPX_OK;  // no coarse interior
    const bool vec = mg3_vec<T>({coarse_or_r, out}, {p_fine, p_coarse}, {s_fine, s_coarse});
    const int lanes = vec ? (wc + JVec<T>::n - 1) / JVec<T>::n : wc;
    const int nxb = (lanes + 63) / 64;
    const int rows = RESTRICT ? hc - 2 : hc - 1;
    const int planes = RESTRICT ? dc - 2 : dc - 1;
    const int kpl = mg3_walk((int64_t)nxb * rows, planes,
                             RESTRICT ? mg3_walk_config().restrict_planes : mg3_walk_config().prolong_planes);
    const int njb = (rows + kMg3Waves - 1) / kMg3Waves;
    const int64_t nblk = (int64_t)nxb * njb * ((planes + kpl - 1) / kpl);
    MPX_CHECK_ARG(nblk <= INT_MAX, "grid too large for one launch");
    const dim3 blk(64, kMg3Waves), grd((unsigned)nblk);
    hipStream_t s = as_stream(stream);
    if constexpr (RESTRICT) {
        if (vec) hipLaunchKernelGGL((mg3_restrict_kernel<T, true>), grd, blk, 0, s, coarse_or_r, out, dc, hc, wc, p_fine,
                                    s_fine, p_coarse, s_coarse, nxb, njb, kpl);
        else hipLaunchKernelGGL((mg3_restrict_kernel<T, false>), grd, blk, 0, s, coarse_or_r, out, dc, hc, wc, p_fine,
                                s_fine, p_coarse, s_coarse, nxb, njb, kpl);
    } else {
        if (vec) hipLaunchKernelGGL((mg3_prolong_kernel<T, true>), grd, blk, 0, s, coarse_or_r, out, dc, hc, wc, p_coarse,
                                    s_coarse, p_fine, s_fine, nxb, njb, kpl);
        else hipLaunchKernelGGL((mg3_prolong_kernel<T, false>), grd, blk, 0, s, coarse_or_r, out, dc, hc, wc, p_coarse,
                                s_coarse, p_fine, s_fine, nxb, njb, kpl);
    }
    MPX_RETURN_IF_HIP_ERROR(hipGetLastError());
    return MPX_OK;
}

// the cubic prolongation: one wave per coarse row 0 .. hc - 2 and block of the coarse planes 0 .. dc - 2
template <typename T>
int launch_mg3_prolong_cubic(const T *c, T *u, int dc, int hc, int wc, int pc, int64_t sc, int pu, int64_t su,
                             void *stream) {
    MPX_CHECK_ARG(c && u, "null pointer");
    MPX_CHECK_ARG(mg3_coarse_ok(dc, hc, wc) && dc >= 3 && hc >= 3 && wc >= 3, "bad grid geometry");
    MPX_CHECK_ARG(mg3_strides_ok(2 * hc - 1, 2 * wc - 1, pu, su) && mg3_strides_ok(hc, wc, pc, sc),
                  "bad strides (pitch >= W, plane stride >= H * pitch)");
    const bool vec = mg3_vec<T>({c, u}, {pc, pu}, {sc, su});
    const int lanes = vec ? (wc + JVec<T>::n - 1) / JVec<T>::n : wc;
    const int nxb = (lanes + 63) / 64;
    const int kpl = mg3_walk((int64_t)nxb * (hc - 1), dc - 1, mg3_cubic_planes());
    const int njb = (hc - 1 + kMg3Waves - 1) / kMg3Waves;
    const int64_t nblk = (int64_t)nxb * njb * ((dc - 1 + kpl - 1) / kpl);
    MPX_CHECK_ARG(nblk <= INT_MAX, "grid too large for one launch");
    const dim3 blk(64, kMg3Waves), grd((unsigned)nblk);
    hipStream_t s = as_stream(stream);
    if (vec) hipLaunchKernelGGL((mg3_prolong_cubic_kernel<T, true>), grd, blk, 0, s, c, u, dc, hc, wc, pc, sc, pu, su, nxb,
                                njb, kpl);
    else hipLaunchKernelGGL((mg3_prolong_cubic_kernel<T, false>), grd, blk, 0, s, c, u, dc, hc, wc, pc, sc, pu, su, nxb,
                            njb, kpl);
    MPX_RETURN_IF_HIP_ERROR(hipGetLastError());
    return MPX_OK;
}

}  // namespace
MPX_MODULE_ANCHOR(multigrid3d)

}  // namespace mpx

extern "C" int mpx_jacobi3d_relax_f64(const double *u, const double *b, double *un, int d, int ny, int nx, int pitch,
                                      int64_t plane, int k0, int k1, double omega, double *resid, void *stream) {
    return mpx::launch_mg3_stencil<double, true>(u, b, un, d, ny, nx, pitch, plane, pitch, plane, pitch, plane, k0, k1,
                                                 omega, resid, stream);
}

extern "C" int mpx_jacobi3d_relax_f32(const float *u, const float *b, float *un, int d, int ny, int nx, int pitch,
                                      int64_t plane, int k0, int k1, double omega, float *resid, void *stream) {
    return mpx::launch_mg3_stencil<float, true>(u, b, un, d, ny, nx, pitch, plane, pitch, plane, pitch, plane, k0, k1,
                                                omega, resid, stream);
}

extern "C" int mpx_mg3_residual_f64(const double *u, const double *b, double *r, int d, int ny, int nx, int pitch_u,
                                    int64_t plane_u, int pitch_b, int64_t plane_b, int pitch_r, int64_t plane_r,
                                    double *resid, void *stream) {
    return mpx::launch_mg3_stencil<double, false>(u, b, r, d, ny, nx, pitch_u, plane_u, pitch_b, plane_b, pitch_r,
                                                  plane_r, 1, d - 1, 1.0, resid, stream);
}

extern "C" int mpx_mg3_residual_f32(const float *u, const float *b, float *r, int d, int ny, int nx, int pitch_u,
                                    int64_t plane_u, int pitch_b, int64_t plane_b, int pitch_r, int64_t plane_r,
                                    float *resid, void *stream) {
    return mpx::launch_mg3_stencil<float, false>(u, b, r, d, ny, nx, pitch_u, plane_u, pitch_b, plane_b, pitch_r, plane_r,
                                                 1, d - 1, 1.0, resid, stream);
}

extern "C" int mpx_mg3_restrict_f64(const double *r, double *bc, int dc, int hc, int wc, int pitch_r, int64_t plane_r,
                                    int pitch_bc, int64_t plane_bc, void *stream) {
    return mpx::launch_mg3_transfer<double, true>(r, bc, dc, hc, wc, pitch_r, plane_r, pitch_bc, plane_bc, stream);
}

extern "C" int mpx_mg3_restrict_f32(const float *r, float *bc, int dc, int hc, int wc, int pitch_r, int64_t plane_r,
                                    int pitch_bc, int64_t plane_bc, void *stream) {
    return mpx::launch_mg3_transfer<float, true>(r, bc, dc, hc, wc, pitch_r, plane_r, pitch_bc, plane_bc, stream);
}

extern "C" int mpx_mg3_prolong_add_f64(const double *e, double *u, int dc, int hc, int wc, int pitch_e, int64_t plane_e,
                                       int pitch_u, int64_t plane_u, void *stream) {
    return mpx::launch_mg3_transfer<double, false>(e, u, dc, hc, wc, pitch_u, plane_u, pitch_e, plane_e, stream);
}

extern "C" int mpx_mg3_prolong_add_f32(const float *e, float *u, int dc, int hc, int wc, int pitch_e, int64_t plane_e,
                                       int pitch_u, int64_t plane_u, void *stream) {
    return mpx::launch_mg3_transfer<float, false>(e, u, dc, hc, wc, pitch_u, plane_u, pitch_e, plane_e, stream);
}

extern "C" int mpx_mg3_prolong_cubic_f64(const double *c, double *u, int dc, int hc, int wc, int pitch_c, int64_t plane_c,
                                         int pitch_u, int64_t plane_u, void *stream) {
    return mpx::launch_mg3_prolong_cubic<double>(c, u, dc, hc, wc, pitch_c, plane_c, pitch_u, plane_u, stream);
}

extern "C" int mpx_mg3_prolong_cubic_f32(const float *c, float *u, int dc, int hc, int wc, int pitch_c, int64_t plane_c,
                                         int pitch_u, int64_t plane_u, void *stream) {
    return mpx::launch_mg3_prolong_cubic<float>(c, u, dc, hc, wc, pitch_c, plane_c, pitch_u, plane_u, stream);
}

extern "C" int mpx_mg3_walk(int *out) {
    MPX_CHECK_ARG(out, "null out");
    const mpx::Mg3Walk &w = mpx::mg3_walk_config();
    out[0] = w.rows;
    out[1] = w.restrict_planes;
    out[2] = w.prolong_planes;
    out[3] = w.min_waves;
    out[4] = mpx::kMg3Waves;
    return MPX_OK;
}

extern "C" int mpx_mg3_cubic_walk(int *out) {
    MPX_CHECK_ARG(out, "null out");
    out[0] = mpx::mg3_cubic_planes();
    out[1] = mpx::mg3_walk_config().min_waves;
    out[2] = mpx::kMg3Waves;
    return MPX_OK;
}
