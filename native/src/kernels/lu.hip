// lab4: dense LU with partial pivoting in fp64 and the solve with its factors
// (the contract is in capi.h). Right-looking, panels of NB = 64 columns:
//
//   panel     lu_panel_col_kernel, one launch per panel column: scale and
//             rank-1 update of the rest of the panel, every wave records the
//             partial argmax of the next column, and the last workgroup to
//             finish (a counter after __threadfence(), nobody ever waits) folds
//             the partials, swaps the two rows' panel segments and writes the
//             pivot for the next launch;
//   tail      lu_tail_kernel: once at most kTailRows rows remain one workgroup
//             factors the whole remaining square in one launch (a system of
//             that size is one launch plus the init);
//   laswp     lu_laswp_kernel: the panel's interchanges left and right of it,
//             in order (they do not commute), one lane per column;
//   U12       dense_trsm_kernel<false>: one lane per column, the unit triangle in
//             LDS read as broadcasts, substitution down the column in registers;
//   update    dense_update_kernel<kRows>: C -= A B for K <= 64 on
//             v_mfma_f64_16x16x4_f64, both operands staged once in LDS.
//
// The solve permutes B, then runs blocked forward / back substitution with
// dense_trsm_kernel on the diagonal blocks and dense_update_kernel between
// them. Both kernels, the tile they are built from, the init kernel and the
// panel-column kernel's handshake are dense_tile.hpp's, shared with chol.hip and
// qr.hip.
#include <climits>

#include "dense_tile.hpp"

namespace mpx {
MPX_MODULE_ANCHOR(lu)

namespace {

constexpr int NB = 64;          // panel width = K of the update
constexpr int kTailRows = 256;  // remaining rows one workgroup factors alone
constexpr int kColRows = 64;    // rows per workgroup of the panel-column kernel (4 waves x 16)
constexpr int kWsHeader = 256;  // bytes in front of the partials: word 0 = the finished-workgroup counter

struct PivPart {  // a partial pivot search: largest |a_ik| and its lowest row
    double v;
    int idx;
    int pad;
};

// the pivot rule: larger magnitude, the lower row among equal ones (NaN never wins)
__device__ __forceinline__ void take_better(double &bv, int &bi, double v, int i) {
    if (v > bv || (v == bv && i < bi)) {
        bv = v;
        bi = i;
    }
}

__device__ __forceinline__ void wave_best(double &v, int &i) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const double ov = __shfl_xor(v, s);
        const int oi = __shfl_xor(i, s);
        take_better(v, i, ov, oi);
    }
}

// Panel [j0, j0 + jb) at step j (-1: only the pivot search of column j0). With
// c = j0 + j the pivot row c is in place: rows i > c get l = a_ic / a_cc and
// a_i,col -= l a_c,col for the panel columns right of c; lane = panel column.
__global__ __launch_bounds__(256) void lu_panel_col_kernel(double *__restrict__ a, int n, int64_t pitch, int j0,
                                                           int jb, int j, int32_t *__restrict__ piv,
                                                           int32_t *__restrict__ info, unsigned *counter,
                                                           PivPart *part) {
    __shared__ double s_v[4];
    __shared__ int s_i[4];
    __shared__ int s_flag;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = j0 + j, cn = c + 1;
    const bool search = cn < j0 + jb;  // the next column is still this panel's
    const int col = j0 + lane;
    const bool incol = lane < jb;
    const int r0 = cn + (int)blockIdx.x * kColRows + wave * 16;
    double u = 0.0, d = 0.0;
    if (j >= 0) {
        d = a[(int64_t)c * pitch + c];
        if (incol) u = a[(int64_t)c * pitch + col];
    }
    double x[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        const int i = r0 + t;
        x[t] = (i < n && incol) ? a[(int64_t)i * pitch + col] : 0.0;
    }
    double bv = -1.0;
    int bi = INT_MAX;
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        const int i = r0 + t;
        if (i >= n) break;  // wave-uniform
        double v = x[t];
        if (j >= 0 && d != 0.0) {  // a zero pivot leaves its column and the rows below as they are
            const double l = __shfl(v, j) / d;
            if (incol && col >= c) {
                v = col == c ? l : v - l * u;
                a[(int64_t)i * pitch + col] = v;
            }
        }
        if (search && col == cn) take_better(bv, bi, fabs(v), i);
    }
    if (!search) return;
    // one partial per wave, written by the lane that owns column cn, so that a
    // single fence covers the rows and the partial
    if (lane == cn - j0) part[blockIdx.x * 4 + wave] = PivPart{bv, bi, 0};
    if (!last_workgroup(counter, &s_flag)) return;
    // the last workgroup to finish: every other one's rows and partials are visible
    double *rc = a + (int64_t)cn * pitch + col;
    const double t0 = threadIdx.x < jb ? *rc : 0.0;  // in flight while the partials are folded
    bv = -1.0;
    bi = INT_MAX;
    for (int k = threadIdx.x; k < 4 * (int)gridDim.x; k += 256) take_better(bv, bi, part[k].v, part[k].idx);
    wave_best(bv, bi);
    if (lane == 0) {
        s_v[wave] = bv;
        s_i[wave] = bi;
    }
    __syncthreads();
    bv = s_v[0];
    bi = s_i[0];
    for (int w = 1; w < 4; ++w) take_better(bv, bi, s_v[w], s_i[w]);
    const int p = (bv == 0.0 || bi < cn || bi >= n) ? cn : bi;
    if (threadIdx.x == 0) {
        piv[cn] = p;
        if (bv == 0.0 && *info == 0) *info = cn + 1;
        *counter = 0;
    }
    if (p != cn && threadIdx.x < jb) {
        double *rp = a + (int64_t)p * pitch + col;
        *rc = *rp;
        *rp = t0;
    }
}

// The remaining square [c0, n) x [c0, n), n - c0 <= kTailRows, by one workgroup:
// unblocked, in global memory (it stays in L2), four barriers per column.
__global__ __launch_bounds__(1024) void lu_tail_kernel(double *__restrict__ a, int n, int64_t pitch, int c0,
                                                       int32_t *__restrict__ piv, int32_t *__restrict__ info) {
    __shared__ double s_v[16];
    __shared__ int s_i[16];
    __shared__ double s_l[kTailRows], s_u[kTailRows];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int c = c0; c < n; ++c) {
        double bv = -1.0;
        int bi = INT_MAX;
        if (c + tid < n) {
            bv = fabs(a[(int64_t)(c + tid) * pitch + c]);
            bi = c + tid;
        }
        wave_best(bv, bi);
        if (lane == 0) {
            s_v[wave] = bv;
            s_i[wave] = bi;
        }
        __syncthreads();
        bv = s_v[0];
        bi = s_i[0];
        for (int w = 1; w < 4; ++w) take_better(bv, bi, s_v[w], s_i[w]);  // rows c + [0, 256): waves 0..3
        const bool zero = bv == 0.0;
        const int p = (zero || bi < c || bi >= n) ? c : bi;
        if (tid == 0) {
            piv[c] = p;
            if (zero && *info == 0) *info = c + 1;
        }
        if (p != c && c0 + tid < n) {
            double *rc = a + (int64_t)c * pitch + c0 + tid, *rp = a + (int64_t)p * pitch + c0 + tid;
            const double t0 = *rc, t1 = *rp;
            *rc = t1;
            *rp = t0;
        }
        __syncthreads();
        const int mm = n - c - 1;
        if (zero || mm == 0) continue;  // uniform
        if (tid < mm) {
            const double l = a[(int64_t)(c + 1 + tid) * pitch + c] / a[(int64_t)c * pitch + c];
            a[(int64_t)(c + 1 + tid) * pitch + c] = l;
            s_l[tid] = l;
            s_u[tid] = a[(int64_t)c * pitch + c + 1 + tid];
        }
        __syncthreads();
        for (int e = tid; e < mm * mm; e += 1024) {
            const int r = e / mm, q = e - r * mm;
            double *px = a + (int64_t)(c + 1 + r) * pitch + c + 1 + q;
            *px = *px - s_l[r] * s_u[q];
        }
        __syncthreads();
    }
}

// Interchanges k in [k0, k1) applied in order to the columns [0, cl) and [cr, n).
__global__ __launch_bounds__(256) void lu_laswp_kernel(double *__restrict__ a, int n, int64_t pitch, int k0, int k1,
                                                       const int32_t *__restrict__ piv, int cl, int cr) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    const int col = idx < cl ? idx : idx - cl + cr;
    if (col >= n) return;
    for (int k = k0; k < k1; ++k) {
        const int p = piv[k];
        if (p == k) continue;  // uniform
        double *rk = a + (int64_t)k * pitch + col, *rp = a + (int64_t)p * pitch + col;
        const double t0 = *rk, t1 = *rp;
        *rk = t1;
        *rp = t0;
    }
}

// Interchanges of the solve: one lane per right-hand side.
__global__ __launch_bounds__(64) void lu_permute_kernel(double *__restrict__ b, int64_t ldb, int nrhs, int n,
                                                        const int32_t *__restrict__ piv) {
    const int col = blockIdx.x * 64 + threadIdx.x;
    if (col >= nrhs) return;
    for (int k = 0; k < n; ++k) {
        const int p = piv[k];
        if (p == k || p < 0 || p >= n) continue;
        double *rk = b + (int64_t)k * ldb + col, *rp = b + (int64_t)p * ldb + col;
        const double t0 = *rk, t1 = *rp;
        *rk = t1;
        *rp = t0;
    }
}

int launch_laswp(double *a, int n, int64_t pitch, int k0, int k1, const int32_t *piv, int cl, int cr, hipStream_t s) {
    const int cols = cl + (n - cr);
    if (cols <= 0) return MPX_OK;
    hipLaunchKernelGGL(lu_laswp_kernel, dim3((cols + 255) / 256), dim3(256), 0, s, a, n, pitch, k0, k1, piv, cl, cr);
    MPX_RETURN_IF_HIP_ERROR(hipGetLastError());
    return MPX_OK;
}

struct Ws {
    unsigned *counter;
    PivPart *part;
};

// four partials (one per wave) for every workgroup of the tallest panel-column launch
int64_t ws_bytes(int n) {
    return n <= 0 ? 0 : kWsHeader + (int64_t)sizeof(PivPart) * 4 * ((n + kColRows - 1) / kColRows + 1);
}

// Panel width of the factorisation: NB, or MPX_LU_NB = 16 / 32 (tools/bench_lu.py's
// sweep; read once per process). The kernels take any width up to NB.
int panel_nb() {
    static const int v = [] {
        const char *e = std::getenv("MPX_LU_NB");
        const int x = e ? std::atoi(e) : NB;
        return (x == 16 || x == 32) ? x : NB;
    }();
    return v;
}

// the four phases of the panel step at j0 (n - j0 > kTailRows, so the panel is full width); mask bit = phase
int panel_step(double *a, int n, int64_t pitch, int32_t *piv, int32_t *info, int j0, int mask, Ws ws,
               hipStream_t s) {
    const int NB = panel_nb();
    const int rest = n - j0 - NB;
    double *ajj = a + (int64_t)j0 * pitch + j0;
    if (mask & 1) {
        for (int j = -1; j < NB; ++j) {
            const int rows = n - (j0 + j) - 1;
            hipLaunchKernelGGL(lu_panel_col_kernel, dim3((rows + kColRows - 1) / kColRows), dim3(256), 0, s, a, n,
                               pitch, j0, NB, j, piv, info, ws.counter, ws.part);
        }
        MPX_RETURN_IF_HIP_ERROR(hipGetLastError());
    }
    if (mask & 2)
        if (int rc = launch_laswp(a, n, pitch, j0, j0 + NB, piv, j0, j0 + NB, s)) return rc;
    if (mask & 4)
        if (int rc = launch_dense_trsm<false>(ajj, pitch, NB, ajj + NB, pitch, rest, s)) return rc;
    if (mask & 8)
        if (int rc = launch_dense_update<kRows>(ajj + (int64_t)NB * pitch, pitch, ajj + NB, pitch,
                                                ajj + (int64_t)NB * pitch + NB, pitch, rest, rest, NB, s))
            return rc;
    return MPX_OK;
}

int check_factor_args(const double *a, int n, int64_t pitch, const int32_t *piv, const int32_t *info,
                      const void *workspace, int64_t workspace_bytes) {
    MPX_CHECK_ARG(n >= 0, "lu: n < 0");
    MPX_CHECK_ARG(pitch >= n, "lu: pitch < n");
    if (n == 0) return MPX_OK;
    MPX_CHECK_ARG(a && piv && info, "lu: null pointer");
    MPX_CHECK_ARG(workspace && workspace_bytes >= ws_bytes(n), "lu: workspace shorter than mpx_lu_workspace_bytes(n)");
    MPX_CHECK_ARG(aligned16(workspace), "lu: workspace not 16-byte aligned");
    return MPX_OK;
}

Ws ws_of(void *workspace) {
    return Ws{static_cast<unsigned *>(workspace),
              reinterpret_cast<PivPart *>(static_cast<char *>(workspace) + kWsHeader)};
}

}  // namespace
}  // namespace mpx

using namespace mpx;

extern "C" int64_t mpx_lu_workspace_bytes(int n) { return ws_bytes(n); }

extern "C" int mpx_lu_panel_width(void) { return panel_nb(); }

extern "C" int mpx_lu_factor_f64(double *a, int n, int64_t pitch, int32_t *piv, int32_t *info, void *workspace,
                                 int64_t workspace_bytes, void *stream) {
    if (int rc = check_factor_args(a, n, pitch, piv, info, workspace, workspace_bytes)) return rc;
    if (n == 0) return MPX_OK;
    hipStream_t s = as_stream(stream);
    const Ws ws = ws_of(workspace);
    hipLaunchKernelGGL(dense_init_kernel<>, dim3(1), dim3(1), 0, s, info, ws.counter);
    MPX_RETURN_IF_HIP_ERROR(hipGetLastError());
    int j0 = 0;
    for (; n - j0 > kTailRows; j0 += panel_nb())
        if (int rc = panel_step(a, n, pitch, piv, info, j0, 15, ws, s)) return rc;
    hipLaunchKernelGGL(lu_tail_kernel, dim3(1), dim3(1024), 0, s, a, n, pitch, j0, piv, info);
    MPX_RETURN_IF_HIP_ERROR(hipGetLastError());
    return launch_laswp(a, n, pitch, j0, n, piv, j0, n, s);
}

extern "C" int mpx_lu_phase_f64(double *a, int n, int64_t pitch, int32_t *piv, int32_t *info, int j0, int phase,
                                void *workspace, int64_t workspace_bytes, void *stream) {
    if (int rc = check_factor_args(a, n, pitch, piv, info, workspace, workspace_bytes)) return rc;
    MPX_CHECK_ARG(j0 >= 0 && j0 % panel_nb() == 0 && n - j0 > kTailRows, "lu: not a panel column");
    MPX_CHECK_ARG(phase >= 0 && phase < 4, "lu: phase outside 0..3");
    const Ws ws = ws_of(workspace);
    if (phase == 0) {
        hipLaunchKernelGGL(dense_init_kernel<>, dim3(1), dim3(1), 0, as_stream(stream), info, ws.counter);
        MPX_RETURN_IF_HIP_ERROR(hipGetLastError());
    }
    return panel_step(a, n, pitch, piv, info, j0, 1 << phase, ws, as_stream(stream));
}

extern "C" int mpx_lu_solve_f64(const double *lu, int n, int64_t pitch, const int32_t *piv, double *b, int nrhs,
                                int64_t pitch_b, void *workspace, int64_t workspace_bytes, void *stream) {
    (void)workspace;
    (void)workspace_bytes;
    MPX_CHECK_ARG(n >= 0 && nrhs >= 0, "lu solve: n < 0 or nrhs < 0");
    MPX_CHECK_ARG(pitch >= n && pitch_b >= nrhs, "lu solve: pitch < n or pitch_b < nrhs");
    if (n == 0 || nrhs == 0) return MPX_OK;
    MPX_CHECK_ARG(lu && piv && b, "lu solve: null pointer");
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(lu_permute_kernel, dim3((nrhs + 63) / 64), dim3(64), 0, s, b, pitch_b, nrhs, n, piv);
    MPX_RETURN_IF_HIP_ERROR(hipGetLastError());
    for (int k0 = 0; k0 < n; k0 += NB) {  // L y = P b
        const int jb = n - k0 < NB ? n - k0 : NB;
        const double *t = lu + (int64_t)k0 * pitch + k0;
        double *bk = b + (int64_t)k0 * pitch_b;
        if (int rc = launch_dense_trsm<false>(t, pitch, jb, bk, pitch_b, nrhs, s)) return rc;
        if (int rc = launch_dense_update<kRows>(t + (int64_t)jb * pitch, pitch, bk, pitch_b,
                                                bk + (int64_t)jb * pitch_b, pitch_b, n - k0 - jb, nrhs, jb, s))
            return rc;
    }
    for (int k0 = (n - 1) / NB * NB; k0 >= 0; k0 -= NB) {  // U x = y
        const int jb = n - k0 < NB ? n - k0 : NB;
        double *bk = b + (int64_t)k0 * pitch_b;
        if (int rc = launch_dense_trsm<true>(lu + (int64_t)k0 * pitch + k0, pitch, jb, bk, pitch_b, nrhs, s)) return rc;
        if (int rc = launch_dense_update<kRows>(lu + k0, pitch, bk, pitch_b, b, pitch_b, k0, nrhs, jb, s)) return rc;
    }
    return MPX_OK;
}
