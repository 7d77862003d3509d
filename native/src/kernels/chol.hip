// lab4: dense Cholesky A = L L^T of a symmetric positive definite matrix in fp64,
// lower storage, and the solve with its factor (the contract is in capi.h).
// Right-looking, panels of NB = 64 columns, three kernels:
//
//   diag      chol_diag_kernel: one workgroup factors the jb x jb diagonal block
//             in LDS, column by column in the reference's operation order, and
//             keeps the info word (the whole factorisation for n <= 64);
//   panel     chol_panel_kernel: L21 = A21 L11^-T, one lane per row, the rows
//             staged through LDS with coalesced loads and stores, L11 in LDS
//             read as broadcasts, k ascending as in the reference;
//   update    chol_syrk_kernel: A22 -= L21 L21^T on v_mfma_f64_16x16x4_f64
//             (dense_tile.hpp's tile, shared with lu.hip and qr.hip), the
//             T (T + 1) / 2 lower tiles only.
//
// The factorisation launches diag once, for the first block. Every later
// diagonal block is factored by the workgroup that has just updated it, tile
// (0, 0) of the update before (AHEAD), while the other tiles are still in
// flight: two launches per panel, and the block's 64 serial columns are off the
// critical path wherever the update has other work. mpx_chol_phase_f64 runs the
// three kernels separately.
//
// No pivot search, so nothing is launched per column, nobody waits on another
// workgroup and there is no workspace. The strict upper triangle and the pitch
// padding are never read or written.
//
// The solve is blocked forward (L y = b) and back (L^T x = y) substitution:
// chol_trsm_kernel on the diagonal blocks, dense_tile.hpp's
// dense_update_kernel<kRows> / <kKMajor> between them.
#include "dense_tile.hpp"

namespace mpx {
MPX_MODULE_ANCHOR(chol)

namespace {

constexpr int NB = 64;  // panel width = K of the update

// The jb x jb block at (j0, j0), jb <= NB, by one workgroup, right-looking in
// LDS: column j takes its square root and its divisions, then every element
// right of it takes its k = j term, which is the reference's order element by
// element (t = a_ij, t -= l_ik l_jk for k ascending, every operation rounded
// once). Thread 0 keeps info: the first column whose reduced diagonal is not
// > 0, unless an earlier panel already reported one.
__device__ __forceinline__ void diag_block(double (*s)[NB + 1], double *ajj, int64_t pitch, int j0, int jb,
                                           int32_t *info) {
    const int tid = threadIdx.x, cq0 = tid >> 6;
    {  // clamped addresses (always inside the lower triangle) make the loads unconditional: all in flight together
        double v[16];
        const int c = tid & 63;
#pragma unroll
        for (int it = 0; it < 16; ++it) {
            const int i = it * 4 + cq0, ii = i < jb ? i : jb - 1;
            v[it] = ajj[(int64_t)ii * pitch + (c < ii ? c : ii)];
        }
#pragma unroll
        for (int it = 0; it < 16; ++it) {
            const int i = it * 4 + cq0;
            if (i < jb && c <= i) s[i][c] = v[it];
        }
    }
    const int row = tid & 63, cq = tid >> 6;
    const int mine = tid < jb ? tid : 0;  // the row whose column entry this thread divides
    int bad = 0;
    for (int j = 0; j < jb; ++j) {
        __syncthreads();
        const double t = s[j][j], lij = s[mine][j];
        const double d = sqrt(t);
        if (!(t > 0.0) && bad == 0) bad = j0 + j + 1;
        if (tid > j && tid < jb) s[tid][j] = lij / d;
        __syncthreads();
        if (tid == 0) s[j][j] = d;  // nobody reads it again before the write-back
        if (row < jb && row > j) {
            // columns c = j + 1 + cq + 4 m <= row: every load before the first store, no
            // divergent branch (a column past the row loads the diagonal and stores
            // into the pad column), and a uniform exit once the block's edge is passed
            const double li = s[row][j];
            double v[16];
#pragma unroll
            for (int m = 0; m < 16; ++m) {
                if (j + 1 + 4 * m >= jb) break;
                const int c = j + 1 + cq + 4 * m, cc = c < row ? c : row;
                v[m] = s[row][cc] - li * s[cc][j];
            }
#pragma unroll
            for (int m = 0; m < 16; ++m) {
                if (j + 1 + 4 * m >= jb) break;
                const int c = j + 1 + cq + 4 * m;
                s[row][c <= row ? c : NB] = v[m];
            }
        }
    }
    __syncthreads();
    for (int e = tid; e < NB * NB; e += 256) {
        const int i = e >> 6, c = e & 63;
        if (i < jb && c <= i) ajj[(int64_t)i * pitch + c] = s[i][c];
    }
    if (tid == 0) {
        if (j0 == 0)
            *info = bad;
        else if (bad && *info == 0)
            *info = bad;
    }
}

__global__ __launch_bounds__(256) void chol_diag_kernel(double *a, int64_t pitch, int j0, int jb, int32_t *info) {
    __shared__ double s[NB][NB + 1];
    diag_block(s, a + (int64_t)j0 * pitch + j0, pitch, j0, jb, info);
}

// The substitutions below keep a lane's vector in LDS at xs[i][lane ^ i] (the
// swizzle lets a workgroup fill it by rows or by columns without bank
// conflicts) and the triangle at s[i][k], read as broadcasts. They work in 8 x 8
// register blocks, which changes no element's operation order, only how many
// LDS reads are in flight: a dependent chain of single reads costs an LDS round
// trip per term. Rows past a ragged triangle hold the identity and +0.0, so
// they add acc - (+0.0) = acc to the real rows and nothing else.
__device__ __forceinline__ int xs_at(int i, int lane) { return i * 64 + (lane ^ i); }

// x_i = (x_i - sum_{k < i} s[i][k] x_k) / s[i][i] for i ascending, k ascending
__device__ __forceinline__ void subst_lower(const double *__restrict__ s, double *__restrict__ xs, int lane,
                                            int nblk) {
#pragma unroll 1
    for (int ib = 0; ib < nblk; ++ib) {
        double x[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) x[u] = xs[xs_at(ib * 8 + u, lane)];
#pragma unroll 1
        for (int kb = 0; kb < ib; ++kb) {
            double y[8];
#pragma unroll
            for (int v = 0; v < 8; ++v) y[v] = xs[xs_at(kb * 8 + v, lane)];
#pragma unroll
            for (int v = 0; v < 8; ++v)
#pragma unroll
                for (int u = 0; u < 8; ++u) x[u] -= s[(ib * 8 + u) * 64 + kb * 8 + v] * y[v];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = ib * 8 + u;
#pragma unroll
            for (int v = 0; v < u; ++v) x[u] -= s[i * 64 + ib * 8 + v] * x[v];
            x[u] = x[u] / s[i * 65];
            xs[xs_at(i, lane)] = x[u];
        }
    }
}

// x_i = (x_i - sum_{k > i} s[k][i] x_k) / s[i][i] for i descending, k ascending:
// one chain after the other (x_i's first term needs the finished x_{i+1}), eight
// terms of a chain loaded at a time
__device__ __forceinline__ void subst_lower_trans(const double *__restrict__ s, double *__restrict__ xs, int lane,
                                                  int nblk) {
#pragma unroll 1
    for (int ib = nblk - 1; ib >= 0; --ib) {
        double x[8];
#pragma unroll
        for (int u = 7; u >= 0; --u) {
            const int i = ib * 8 + u;
            double acc = xs[xs_at(i, lane)];
#pragma unroll
            for (int v = u + 1; v < 8; ++v) acc -= s[(ib * 8 + v) * 64 + i] * x[v];
#pragma unroll 1
            for (int kb = ib + 1; kb < nblk; ++kb) {
#pragma unroll
                for (int v = 0; v < 8; ++v) acc -= s[(kb * 8 + v) * 64 + i] * xs[xs_at(kb * 8 + v, lane)];
            }
            x[u] = acc / s[i * 65];
            xs[xs_at(i, lane)] = x[u];
        }
    }
}

// the lower jb x jb triangle at t into s, the identity past it; the strict
// upper triangle of t is never read
__device__ __forceinline__ void load_triangle(double *__restrict__ s, const double *__restrict__ t, int64_t ldt,
                                              int jb, int tid) {
    // lane = column; clamped addresses (always inside the triangle) make the loads
    // unconditional, so that sixteen rows' loads are in flight together
#pragma unroll 1
    for (int i0 = 0; i0 < NB; i0 += 16) {
        double v[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int ii = i0 + q < jb ? i0 + q : jb - 1;
            v[q] = t[(int64_t)ii * ldt + (tid < ii ? tid : ii)];
        }
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int i = i0 + q;
            s[i * 64 + tid] = (i < jb && tid <= i) ? v[q] : (i == tid ? 1.0 : 0.0);
        }
    }
}

// L21 = A21 L11^-T for the rows below the full-width block at t: row r of A21
// becomes x with x_c = (a_rc - sum_{k < c} x_k l_ck) / l_cc, k ascending. A
// workgroup (one wave) takes 64 rows, staged with coalesced row loads and
// stores (lane = column); in the substitution a lane owns a row.
__global__ __launch_bounds__(64) void chol_panel_kernel(const double *__restrict__ t, int64_t ldt,
                                                        double *__restrict__ x, int64_t ldx, int rows) {
    __shared__ __attribute__((aligned(16))) double s[NB * NB];
    __shared__ double xs[NB * 64];
    const int tid = threadIdx.x;
    load_triangle(s, t, ldt, NB, tid);
    const int r0 = blockIdx.x * 64;
    const int nr = rows - r0 < 64 ? rows - r0 : 64;
#pragma unroll 1
    for (int q0 = 0; q0 < 64; q0 += 16) {  // rows past the last are copies of it that nobody uses
        double v[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) v[q] = x[(int64_t)(r0 + (q0 + q < nr ? q0 + q : nr - 1)) * ldx + tid];
#pragma unroll
        for (int q = 0; q < 16; ++q) xs[xs_at(tid, q0 + q)] = v[q];
    }
    __syncthreads();
    if (tid < nr) subst_lower(s, xs, tid, 8);
    __syncthreads();
    for (int r = 0; r < nr; ++r) x[(int64_t)(r0 + r) * ldx + tid] = xs[xs_at(tid, r)];
}

// B (jb x ncols) <- T^-1 B (TRANS = false) or T^-T B (TRANS = true), T the
// lower jb x jb (jb <= NB) block at t with its diagonal; a lane owns a column
// of B.
template <bool TRANS>
__global__ __launch_bounds__(64) void chol_trsm_kernel(const double *__restrict__ t, int64_t ldt, int jb,
                                                       double *__restrict__ b, int64_t ldb, int ncols) {
    __shared__ __attribute__((aligned(16))) double s[NB * NB];
    __shared__ double xs[NB * 64];
    const int tid = threadIdx.x;
    load_triangle(s, t, ldt, jb, tid);
    const int col = blockIdx.x * 64 + tid;
    const bool ok = col < ncols;
    const int nblk = (jb + 7) >> 3;
    const int cc = ok ? col : ncols - 1;
#pragma unroll 1
    for (int i0 = 0; i0 < NB; i0 += 16) {
        double v[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) v[q] = b[(int64_t)(i0 + q < jb ? i0 + q : jb - 1) * ldb + cc];
#pragma unroll
        for (int q = 0; q < 16; ++q) xs[xs_at(i0 + q, tid)] = (ok && i0 + q < jb) ? v[q] : 0.0;
    }
    __syncthreads();
    if (!ok) return;
    if (TRANS)
        subst_lower_trans(s, xs, tid, nblk);
    else
        subst_lower(s, xs, tid, nblk);
    for (int i = 0; i < jb; ++i) b[(int64_t)i * ldb + col] = xs[xs_at(i, tid)];
}

// A22 (M x M, col <= row only) -= A A^T, A = L21 stored M x K, K <= NB, on
// dense_tile.hpp's tile: both operands are row blocks of A in the `rows` layout.
// blockIdx.x counts the lower tiles row by row, (bi, bj) with bj <= bi;
// diagonal tiles touch C only where col <= row, and their upper-right wave has
// nothing to do.
// V2: 16-byte global loads (a 16-byte aligned A with an even pitch).
// AHEAD: the workgroup of tile (0, 0) goes on to factor that tile, the next
// panel's diagonal block at column jn (diag_block, the same code and so the same
// bits as chol_diag_kernel), while the other tiles are still being updated: the
// block's serial 64 columns leave the critical path and the next panel needs no
// launch for them. Nobody waits on anybody: the tile is this workgroup's own.
template <bool V2, bool AHEAD>
__global__ __launch_bounds__(256) void chol_syrk_kernel(const double *__restrict__ A, int64_t lda, double *C,
                                                        int64_t ldc, int M, int K, int jn, int32_t *info) {
    __shared__ __attribute__((aligned(16))) double lds[2 * NB * 64];
    static_assert(sizeof(double) * (NB + 1) * NB <= sizeof(lds), "diag_block's tile fits the operands' LDS");
    double *As = lds, *Bs = lds + NB * 64;
    const int tid = threadIdx.x, wave = tid >> 6;
    const int b = blockIdx.x;
    int bi = (int)((sqrtf(8.0f * (float)b + 1.0f) - 1.0f) * 0.5f);
    while ((bi + 1) * (bi + 2) / 2 <= b) ++bi;
    while (bi * (bi + 1) / 2 > b) --bi;
    const int bj = b - bi * (bi + 1) / 2;
    const int m0 = bi * 64, n0 = bj * 64;
    stage_rows<V2, true>(As, A + (int64_t)m0 * lda, lda, M - m0, K, tid);
    stage_rows<V2, false>(Bs, A + (int64_t)n0 * lda, lda, M - n0, K, tid);
    const bool idle = bi == bj && (wave & 1) > (wave >> 1);  // wave-uniform: the quarter above the diagonal
    tile_update<true, kRows, kRows>(C, ldc, m0, n0, M, M, As, Bs, K, idle);
    if (AHEAD && blockIdx.x == 0) {
        __threadfence_block();
        __syncthreads();  // the tile is in memory for this workgroup, and the operands' LDS is free
        diag_block(reinterpret_cast<double(*)[NB + 1]>(lds), C, ldc, jn, M < NB ? M : NB, info);
    }
}

template <bool AHEAD = false>
int launch_syrk(const double *A, int64_t lda, double *C, int64_t ldc, int M, int K, hipStream_t s, int jn = 0,
                int32_t *info = nullptr) {
    if (M <= 0 || K <= 0) return MPX_OK;
    const int tm = (M + 63) / 64;
    const dim3 grid(tm * (tm + 1) / 2);
    if (aligned16(A) && lda % 2 == 0)
        hipLaunchKernelGGL((chol_syrk_kernel<true, AHEAD>), grid, dim3(256), 0, s, A, lda, C, ldc, M, K, jn, info);
    else
        hipLaunchKernelGGL((chol_syrk_kernel<false, AHEAD>), grid, dim3(256), 0, s, A, lda, C, ldc, M, K, jn, info);
    MPX_RETURN_IF_HIP_ERROR(hipGetLastError());
    return MPX_OK;
}

template <bool TRANS>
int launch_trsm(const double *t, int64_t ldt, int jb, double *b, int64_t ldb, int ncols, hipStream_t s) {
    if (ncols <= 0 || jb <= 0) return MPX_OK;
    hipLaunchKernelGGL(chol_trsm_kernel<TRANS>, dim3((ncols + 63) / 64), dim3(64), 0, s, t, ldt, jb, b, ldb, ncols);
    MPX_RETURN_IF_HIP_ERROR(hipGetLastError());
    return MPX_OK;
}

// The phases of the panel step at j0; mask bit = phase. ahead: the update also
// factors the next diagonal block (the factorisation's form: its panels after
// the first then start at phase 1).
int panel_step(double *a, int n, int64_t pitch, int32_t *info, int j0, int mask, bool ahead, hipStream_t s) {
    const int jb = n - j0 < NB ? n - j0 : NB;
    const int rest = n - j0 - jb;
    double *ajj = a + (int64_t)j0 * pitch + j0;
    double *a21 = ajj + (int64_t)jb * pitch;
    if (mask & 1) {
        hipLaunchKernelGGL(chol_diag_kernel, dim3(1), dim3(256), 0, s, a, pitch, j0, jb, info);
        MPX_RETURN_IF_HIP_ERROR(hipGetLastError());
    }
    if (rest <= 0) return MPX_OK;  // below a ragged block there is nothing: jb == NB from here on
    if (mask & 2) {
        hipLaunchKernelGGL(chol_panel_kernel, dim3((rest + 63) / 64), dim3(64), 0, s, ajj, pitch, a21, pitch, rest);
        MPX_RETURN_IF_HIP_ERROR(hipGetLastError());
    }
    if (mask & 4) {
        if (ahead) return launch_syrk<true>(a21, pitch, a21 + jb, pitch, rest, jb, s, j0 + jb, info);
        return launch_syrk(a21, pitch, a21 + jb, pitch, rest, jb, s);
    }
    return MPX_OK;
}

int check_factor_args(const double *a, int n, int64_t pitch, const int32_t *info) {
    MPX_CHECK_ARG(n >= 0, "chol: n < 0");
    MPX_CHECK_ARG(pitch >= n, "chol: pitch < n");
    if (n == 0) return MPX_OK;
    MPX_CHECK_ARG(a && info, "chol: null pointer");
    return MPX_OK;
}

}  // namespace
}  // namespace mpx

using namespace mpx;

extern "C" int mpx_chol_factor_f64(double *a, int n, int64_t pitch, int32_t *info, void *stream) {
    if (int rc = check_factor_args(a, n, pitch, info)) return rc;
    if (n == 0) return MPX_OK;
    for (int j0 = 0; j0 < n; j0 += NB)
        if (int rc = panel_step(a, n, pitch, info, j0, j0 == 0 ? 7 : 6, true, as_stream(stream))) return rc;
    return MPX_OK;
}

extern "C" int mpx_chol_phase_f64(double *a, int n, int64_t pitch, int32_t *info, int j0, int phase, void *stream) {
    if (int rc = check_factor_args(a, n, pitch, info)) return rc;
    MPX_CHECK_ARG(j0 >= 0 && j0 % NB == 0 && j0 < n, "chol: not a panel column");
    MPX_CHECK_ARG(phase >= 0 && phase < 3, "chol: phase outside 0..2");
    return panel_step(a, n, pitch, info, j0, 1 << phase, false, as_stream(stream));
}

extern "C" int mpx_chol_solve_f64(const double *l, int n, int64_t pitch, double *b, int nrhs, int64_t pitch_b,
                                  void *stream) {
    MPX_CHECK_ARG(n >= 0 && nrhs >= 0, "chol solve: n < 0 or nrhs < 0");
    MPX_CHECK_ARG(pitch >= n && pitch_b >= nrhs, "chol solve: pitch < n or pitch_b < nrhs");
    if (n == 0 || nrhs == 0) return MPX_OK;
    MPX_CHECK_ARG(l && b, "chol solve: null pointer");
    hipStream_t s = as_stream(stream);
    for (int k0 = 0; k0 < n; k0 += NB) {  // L y = b
        const int jb = n - k0 < NB ? n - k0 : NB;
        const double *t = l + (int64_t)k0 * pitch + k0;
        double *bk = b + (int64_t)k0 * pitch_b;
        if (int rc = launch_trsm<false>(t, pitch, jb, bk, pitch_b, nrhs, s)) return rc;
        if (int rc = launch_dense_update<kRows>(t + (int64_t)jb * pitch, pitch, bk, pitch_b,
                                                bk + (int64_t)jb * pitch_b, pitch_b, n - k0 - jb, nrhs, jb, s))
            return rc;
    }
    for (int k0 = (n - 1) / NB * NB; k0 >= 0; k0 -= NB) {  // L^T x = y
        const int jb = n - k0 < NB ? n - k0 : NB;
        const double *lk = l + (int64_t)k0 * pitch;
        double *bk = b + (int64_t)k0 * pitch_b;
        if (int rc = launch_trsm<true>(lk + k0, pitch, jb, bk, pitch_b, nrhs, s)) return rc;
        if (int rc = launch_dense_update<kKMajor>(lk, pitch, bk, pitch_b, b, pitch_b, k0, nrhs, jb, s)) return rc;
    }
    return MPX_OK;
}
