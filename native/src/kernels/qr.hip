// lab4: dense Householder QR A = Q R of a tall or square matrix (m >= n) in
// fp64, LAPACK geqrf storage, the application of Q and Q^T from the stored
// reflectors and the solve with R (the contract is in capi.h). Right-looking,
// panels of NB = 64 columns:
//
//   panel     qr_panel_col_kernel, one launch per panel column and one more to
//             finish the panel: launch j scales column c - 1 into v and applies
//             reflector c - 1 to the panel columns right of it (rank-1, VALU,
//             lane = panel column), and every workgroup leaves its partial of
//             the Gram row g_col = sum_{i > c} a_ic a_i,col. The last workgroup
//             to finish (a counter after __threadfence(), nobody ever waits)
//             folds the partials in index order, forms beta, tau_c and the row
//             w of the next rank-1 update, and updates row c itself;
//   W         qr_vtc_kernel: W = V^T C on v_mfma_f64_16x16x4_f64 with a K loop
//             over the rows. The rows are cut into chunks of kChunkRows whose
//             partial products go to the workspace; one more column tile holds
//             V^T V. V is read in place: the panel's diagonal block is masked to
//             unit lower on the way into LDS;
//   T         qr_t_kernel: the chunks of V^T V summed in order, then the
//             64 x 64 upper-triangular T of H_0 .. H_63 = I - V T V^T (larft,
//             forward, columnwise), one workgroup;
//   Z         qr_z_kernel: the chunks of W summed in order, Z = T^T W (or T W
//             for Q), lane = column;
//   apply     dense_update_kernel<kRows, ., true>: C -= V Z, K = 64, both
//             operands staged once, V's diagonal block masked the same way.
//
// A factorisation is n + ceil(n / 64) panel launches, four more per panel that
// has columns to its right, and one init: n + O(n / 64). An application of Q or
// Q^T to a block is four launches per panel. Nothing depends on the matrix's
// width but which columns exist: the row chunks and the rows per panel
// workgroup follow from m and the column's index alone, so column j of the
// result is a function of columns 0 .. j.
//
// rsolve is blocked back substitution with R: dense_trsm_kernel<true> on the
// diagonal blocks, dense_update_kernel between them. The MFMA tile with its LDS
// layouts, these two kernels, the init kernel and the panel kernel's handshake
// are dense_tile.hpp's, shared with lu.hip and chol.hip.
#include "dense_tile.hpp"

namespace mpx {
MPX_MODULE_ANCHOR(qr)

namespace {

constexpr int NB = 64;             // panel width = K of the apply
constexpr int kChunkRows = 1024;   // rows of one partial W (16 K steps of 64)
constexpr int kWsHeader = 256;     // bytes in front: word 0 = the finished-workgroup counter
constexpr int kStateDoubles = 128; // w[64] of the pending rank-1 update, [64] = alpha - beta (0: none)

// rows per workgroup of the panel kernel: 64, more for very tall matrices so
// that the fold stays within 256 partials; a function of m alone
int panel_rows(int m) { return 64 * (m > 16384 ? (m + 16383) / 16384 : 1); }

// Panel [j0, j0 + jb), launch j in 0 .. jb, c = j0 + j; lane = panel column.
// Rows i >= c: with the pending reflector c - 1 (state: w, d = alpha - beta,
// d == 0 when tau = 0) v_i = a_i,c-1 / d is stored and a_i,col -= v_i w_col for
// col >= c. For j < jb the rows i > c then add a_ic a_i,col to the Gram row, in
// ascending row order within a wave, the four waves in order, and the last
// workgroup folds the workgroups' partials in index order and builds reflector
// c from sigma = g_c.
__global__ __launch_bounds__(256) void qr_panel_col_kernel(double *a, int m, int64_t pitch, int j0, int jb, int j,
                                                           int rpw, double *__restrict__ tau,
                                                           int32_t *__restrict__ info, unsigned *counter,
                                                           double *state, double *part) {
    __shared__ double s_g[4][64];
    __shared__ int s_flag;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = j0 + j, col = j0 + lane;
    const bool incol = lane < jb;
    const bool gram = j < jb, apply = j > 0;
    double d = 0.0, w = 0.0;
    if (apply) {
        d = state[64];
        w = state[lane];
    }
    const int wrows = rpw >> 2;
    const int rbase = c + (int)blockIdx.x * rpw + wave * wrows;
    double g = 0.0;
    for (int t0 = 0; t0 < wrows; t0 += 16) {
        const int r0 = rbase + t0;
        if (r0 >= m) break;  // wave-uniform
        double x[16];
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const int i = r0 + t;
            x[t] = (i < m && incol) ? a[(int64_t)i * pitch + col] : 0.0;
        }
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const int i = r0 + t;
            double v = x[t];
            if (i < m && apply && d != 0.0) {  // wave-uniform; tau = 0 leaves everything as it is
                const double vi = __shfl(v, j - 1) / d;
                if (incol && lane >= j - 1) {
                    v = lane == j - 1 ? vi : v - vi * w;
                    a[(int64_t)i * pitch + col] = v;
                }
            }
            if (i < m && gram && i > c) g += __shfl(v, j) * v;  // wave-uniform
        }
    }
    if (!gram) return;
    s_g[wave][lane] = g;
    __syncthreads();
    if (wave == 0) part[(int64_t)blockIdx.x * 64 + lane] = ((s_g[0][lane] + s_g[1][lane]) + s_g[2][lane]) + s_g[3][lane];
    if (!last_workgroup(counter, &s_flag)) return;
    // the last workgroup to finish: every other one's rows and partials are visible
    double acc = 0.0;
    for (int b = wave; b < (int)gridDim.x; b += 4) acc += part[(int64_t)b * 64 + lane];
    s_g[wave][lane] = acc;
    __syncthreads();
    if (wave != 0) return;
    const double gc = ((s_g[0][lane] + s_g[1][lane]) + s_g[2][lane]) + s_g[3][lane];
    const double sigma = __shfl(gc, j);
    double *rc = a + (int64_t)c * pitch;
    const double alpha = rc[c];
    const bool mine = incol && lane >= j;
    const double x = mine ? rc[col] : 0.0;
    double tc = 0.0, dn = 0.0, wn = 0.0, rcc = alpha;
    if (sigma != 0.0) {  // a NaN goes this way too
        const double norm = sqrt(alpha * alpha + sigma);
        const double beta = -copysign(norm, alpha);
        tc = (beta - alpha) / beta;
        dn = alpha - beta;
        wn = tc * (x + gc / dn);
        rcc = beta;
        if (mine) rc[col] = lane == j ? beta : x - wn;
    }
    state[lane] = wn;
    if (lane == 0) {
        state[64] = dn;
        tau[c] = tc;
        if (rcc == 0.0 && *info == 0) *info = c + 1;
        *counter = 0;
    }
}

// W_chunk (64 x 64 tile) = V^T C over the rows of one chunk. V: rows x jb at V
// (the panel, its first 64 rows the diagonal block), C: rows x N. blockIdx.x is
// the column tile, tile ntiles is V itself (V^T V for T), blockIdx.y the chunk.
// Both operands are k-major as they lie in memory (k = the row), so nothing is
// transposed on the way into LDS (dense_tile.hpp); the rows of V's diagonal
// block are masked to unit lower on the way. Every K step of 64 rows is staged
// and consumed between two barriers. The tile is stored whole: past jb and past
// N it holds the zeros of the padding.
template <bool V2>
__global__ __launch_bounds__(256) void qr_vtc_kernel(const double *__restrict__ V, int64_t ldv, int jb,
                                                     const double *__restrict__ C, int64_t ldc, int N, int rows,
                                                     double *__restrict__ W, int64_t ldw, int ntiles) {
    __shared__ __attribute__((aligned(16))) double As[NB * 64];
    __shared__ __attribute__((aligned(16))) double Bs[NB * 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tile = blockIdx.x, chunk = blockIdx.y;
    const int n0 = tile * 64;
    const int g = lane >> 4, l15 = lane & 15;
    const int wr = (wave >> 1) * 32, wc = (wave & 1) * 32;
    const int kb = chunk * kChunkRows;
    const int ke = rows < kb + kChunkRows ? rows : kb + kChunkRows;
    f64x4 acc[2][2];
#pragma unroll
    for (int im = 0; im < 2; ++im)
#pragma unroll
        for (int in = 0; in < 2; ++in) acc[im][in] = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
    for (int k0 = kb; k0 < ke; k0 += 64) {
        __syncthreads();  // the step before has been read
        const double *vk = V + (int64_t)k0 * ldv;
        stage_kmajor<V2, false>(As, vk, ldv, rows - k0, jb, tid, k0);
        if (tile < ntiles)
            stage_kmajor<V2, false>(Bs, C + (int64_t)k0 * ldc + n0, ldc, rows - k0, N - n0, tid);
        else
            stage_kmajor<V2, false>(Bs, vk, ldv, rows - k0, jb, tid, k0);
        __syncthreads();
        tile_mma<kKMajor, kKMajor>(acc, As, Bs, 0, 64);
    }
    double *wt = W + (int64_t)chunk * 64 * ldw + n0;
#pragma unroll
    for (int im = 0; im < 2; ++im)
#pragma unroll
        for (int in = 0; in < 2; ++in)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                wt[(int64_t)(wr + im * 16 + g + 4 * r) * ldw + wc + in * 16 + l15] = acc[im][in][r];
}

// T (64 x 64, row-major, zero below the diagonal) from G = V^T V, whose chunks
// sit in the last column tile of W and are summed in ascending order:
//   T_jj = tau_j,  T[0:j, j] = -tau_j T[0:j, 0:j] G[0:j, j],  k ascending.
// Thread i of the first wave owns row i of T and keeps it in registers (the
// loops are unrolled, so the row is indexed statically); G is read from LDS as
// broadcasts, which do not wait for the row's chain of additions. The zeros left
// of the diagonal are summed along: they add +0. Columns past jb take tau = 0.
__global__ __launch_bounds__(256) void qr_t_kernel(const double *__restrict__ G, int64_t ldw, int chunks,
                                                   const double *__restrict__ tau, int jb, double *__restrict__ T) {
    __shared__ double Gs[NB][NB + 1];
    __shared__ double s_tau[NB];
    const int tid = threadIdx.x, lane = tid & 63;
    for (int p = tid >> 6; p < NB; p += 4) {
        double s = 0.0;
#pragma unroll 8
        for (int ch = 0; ch < chunks; ++ch) s += G[((int64_t)ch * 64 + p) * ldw + lane];
        Gs[p][lane] = s;
    }
    if (tid < NB) s_tau[tid] = tid < jb ? tau[tid] : 0.0;
    __syncthreads();
    if (tid >= NB) return;
    double t[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < j; ++k) s += t[k] * Gs[k][j];
        t[j] = tid == j ? s_tau[j] : (tid < j ? -s_tau[j] * s : 0.0);
    }
#pragma unroll
    for (int j = 0; j < NB; ++j) T[tid * 64 + j] = t[j];
}

// Z (64 x ncols, pitch ldz) = T^T W (TRANS: the step of Q^T and of the
// factorisation) or T W (the step of Q), W the sum of its chunks in ascending
// order. A workgroup takes 64 columns, a lane a column; the four waves share
// the rows of W on the way in and the rows of Z on the way out (interleaved:
// the triangle's long and short rows spread evenly). T sits in LDS and is read
// as broadcasts, k ascending.
template <bool TRANS>
__global__ __launch_bounds__(256) void qr_z_kernel(const double *__restrict__ W, int64_t ldw, int chunks,
                                                   const double *__restrict__ T, double *__restrict__ Z, int64_t ldz) {
    __shared__ double Ts[NB * NB];
    __shared__ double xs[NB][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = blockIdx.x * 64 + lane;
    for (int e = tid; e < NB * NB; e += 256) Ts[e] = T[e];
    for (int k = wave; k < NB; k += 4) {
        double s = 0.0;
#pragma unroll 8
        for (int ch = 0; ch < chunks; ++ch) s += W[((int64_t)ch * 64 + k) * ldw + col];
        xs[k][lane] = s;
    }
    __syncthreads();
    for (int i = wave; i < NB; i += 4) {
        double acc = 0.0;
        if (TRANS) {
#pragma unroll 8
            for (int k = 0; k <= i; ++k) acc += Ts[k * 64 + i] * xs[k][lane];
        } else {
#pragma unroll 8
            for (int k = i; k < NB; ++k) acc += Ts[i * 64 + k] * xs[k][lane];
        }
        Z[(int64_t)i * ldz + col] = acc;
    }
}

int64_t round64(int64_t x) { return (x + 63) / 64 * 64; }
int chunks_of(int rows) { return (rows + kChunkRows - 1) / kChunkRows; }

// header | state | panel partials | T | Z (64 x npad) | W (chunks x 64 x (npad + 64))
struct Ws {
    unsigned *counter;
    double *state, *part, *T, *Z, *W;
};

int64_t part_doubles(int m) { return 64 * (int64_t)((m + panel_rows(m) - 1) / panel_rows(m) + 1); }

int64_t ws_bytes(int m, int n, int nrhs) {
    if (m <= 0 || n <= 0) return 0;
    const int64_t npad = round64(n > nrhs ? n : nrhs);
    return kWsHeader + 8 * (kStateDoubles + part_doubles(m) + NB * NB + 64 * npad +
                            (int64_t)chunks_of(m) * 64 * (npad + 64));
}

Ws ws_of(void *workspace, int m, int ncols) {
    Ws w;
    w.counter = static_cast<unsigned *>(workspace);
    w.state = reinterpret_cast<double *>(static_cast<char *>(workspace) + kWsHeader);
    w.part = w.state + kStateDoubles;
    w.T = w.part + part_doubles(m);
    w.Z = w.T + NB * NB;
    w.W = w.Z + 64 * round64(ncols);
    return w;
}

// One block reflector applied to C (rows x N): C <- (I - V T^T V^T) C (trans)
// or (I - V T V^T) C. V is the panel at `v` (rows x jb, its diagonal block on
// top), tau the panel's. mask bit 1: W and V^T V, bit 2: T and Z, bit 3: apply.
int block_apply(const double *v, int64_t ldv, int rows, int jb, const double *tau, double *c, int64_t ldc, int N,
                bool trans, const Ws &ws, int mask, hipStream_t s) {
    if (rows <= 0 || N <= 0 || jb <= 0) return MPX_OK;
    const int ntiles = (N + 63) / 64, chunks = chunks_of(rows);
    const int64_t ldz = 64 * (int64_t)ntiles, ldw = ldz + 64;
    if (mask & 2) {
        const dim3 grid(ntiles + 1, chunks);
        if (aligned16(v) && aligned16(c) && ldv % 2 == 0 && ldc % 2 == 0)
            hipLaunchKernelGGL(qr_vtc_kernel<true>, grid, dim3(256), 0, s, v, ldv, jb, c, ldc, N, rows, ws.W, ldw,
                               ntiles);
        else
            hipLaunchKernelGGL(qr_vtc_kernel<false>, grid, dim3(256), 0, s, v, ldv, jb, c, ldc, N, rows, ws.W, ldw,
                               ntiles);
        MPX_RETURN_IF_HIP_ERROR(hipGetLastError());
    }
    if (mask & 4) {
        hipLaunchKernelGGL(qr_t_kernel, dim3(1), dim3(256), 0, s, ws.W + ldz, ldw, chunks, tau, jb, ws.T);
        if (trans)
            hipLaunchKernelGGL(qr_z_kernel<true>, dim3(ntiles), dim3(256), 0, s, ws.W, ldw, chunks, ws.T, ws.Z, ldz);
        else
            hipLaunchKernelGGL(qr_z_kernel<false>, dim3(ntiles), dim3(256), 0, s, ws.W, ldw, chunks, ws.T, ws.Z, ldz);
        MPX_RETURN_IF_HIP_ERROR(hipGetLastError());
    }
    if (mask & 8) return launch_dense_update<kRows, true>(v, ldv, ws.Z, ldz, c, ldc, rows, N, jb, s);
    return MPX_OK;
}

// the panel step at j0; mask bit 0: the panel's columns, bits 1..3: block_apply's
int panel_step(double *a, int m, int n, int64_t pitch, double *tau, int32_t *info, int j0, int mask, const Ws &ws,
               hipStream_t s) {
    const int jb = n - j0 < NB ? n - j0 : NB;
    if (mask & 1) {
        const int rpw = panel_rows(m);
        for (int j = 0; j <= jb; ++j) {
            const int rows = m - (j0 + j);
            if (rows <= 0) break;  // a square matrix's last panel: nothing below the last row
            hipLaunchKernelGGL(qr_panel_col_kernel, dim3((rows + rpw - 1) / rpw), dim3(256), 0, s, a, m, pitch, j0,
                               jb, j, rpw, tau, info, ws.counter, ws.state, ws.part);
        }
        MPX_RETURN_IF_HIP_ERROR(hipGetLastError());
    }
    double *v = a + (int64_t)j0 * pitch + j0;
    return block_apply(v, pitch, m - j0, jb, tau + j0, v + jb, pitch, n - j0 - jb, true, ws, mask, s);
}

int check_factor_args(const double *a, int m, int n, int64_t pitch, const double *tau, const int32_t *info,
                      const void *workspace, int64_t workspace_bytes) {
    MPX_CHECK_ARG(m >= 0 && n >= 0, "qr: m < 0 or n < 0");
    MPX_CHECK_ARG(m >= n, "qr: m < n");
    MPX_CHECK_ARG(pitch >= n, "qr: pitch < n");
    if (m == 0 || n == 0) return MPX_OK;
    MPX_CHECK_ARG(a && tau && info, "qr: null pointer");
    MPX_CHECK_ARG(workspace && workspace_bytes >= ws_bytes(m, n, 0),
                  "qr: workspace shorter than mpx_qr_workspace_bytes(m, n, 0)");
    MPX_CHECK_ARG(aligned16(workspace), "qr: workspace not 16-byte aligned");
    return MPX_OK;
}

}  // namespace
}  // namespace mpx

using namespace mpx;

extern "C" int64_t mpx_qr_workspace_bytes(int m, int n, int nrhs) {
    if (m < 0 || n < 0 || nrhs < 0 || m < n) return 0;
    return ws_bytes(m, n, nrhs);
}

extern "C" int mpx_qr_plan(int m, int n, int32_t out[4]) {
    MPX_CHECK_ARG(m >= 0 && n >= 0 && m >= n, "qr plan: m < n or a negative size");
    MPX_CHECK_ARG(out, "qr plan: null pointer");
    out[0] = panel_rows(m);
    out[1] = kChunkRows;
    out[2] = chunks_of(m);
    out[3] = NB;
    return MPX_OK;
}

extern "C" int mpx_qr_factor_f64(double *a, int m, int n, int64_t pitch, double *tau, int32_t *info, void *workspace,
                                 int64_t workspace_bytes, void *stream) {
    if (int rc = check_factor_args(a, m, n, pitch, tau, info, workspace, workspace_bytes)) return rc;
    if (m == 0 || n == 0) return MPX_OK;
    hipStream_t s = as_stream(stream);
    const Ws ws = ws_of(workspace, m, n);
    hipLaunchKernelGGL(dense_init_kernel<>, dim3(1), dim3(1), 0, s, info, ws.counter);
    MPX_RETURN_IF_HIP_ERROR(hipGetLastError());
    for (int j0 = 0; j0 < n; j0 += NB)
        if (int rc = panel_step(a, m, n, pitch, tau, info, j0, 15, ws, s)) return rc;
    return MPX_OK;
}

extern "C" int mpx_qr_phase_f64(double *a, int m, int n, int64_t pitch, double *tau, int32_t *info, int j0, int phase,
                                void *workspace, int64_t workspace_bytes, void *stream) {
    if (int rc = check_factor_args(a, m, n, pitch, tau, info, workspace, workspace_bytes)) return rc;
    MPX_CHECK_ARG(j0 >= 0 && j0 % NB == 0 && j0 < n, "qr: not a panel column");
    MPX_CHECK_ARG(phase >= 0 && phase < 4, "qr: phase outside 0..3");
    const Ws ws = ws_of(workspace, m, n);
    if (phase == 0 && j0 == 0) {
        hipLaunchKernelGGL(dense_init_kernel<>, dim3(1), dim3(1), 0, as_stream(stream), info, ws.counter);
        MPX_RETURN_IF_HIP_ERROR(hipGetLastError());
    }
    return panel_step(a, m, n, pitch, tau, info, j0, 1 << phase, ws, as_stream(stream));
}

extern "C" int mpx_qr_apply_f64(const double *qr, int m, int n, int64_t pitch, const double *tau, double *b, int nrhs,
                                int64_t pitch_b, int transpose, void *workspace, int64_t workspace_bytes,
                                void *stream) {
    MPX_CHECK_ARG(m >= 0 && n >= 0 && nrhs >= 0, "qr apply: a negative size");
    MPX_CHECK_ARG(m >= n, "qr apply: m < n");
    MPX_CHECK_ARG(pitch >= n && pitch_b >= nrhs, "qr apply: pitch < n or pitch_b < nrhs");
    if (m == 0 || n == 0 || nrhs == 0) return MPX_OK;
    MPX_CHECK_ARG(qr && tau && b, "qr apply: null pointer");
    MPX_CHECK_ARG(workspace && workspace_bytes >= ws_bytes(m, n, nrhs),
                  "qr apply: workspace shorter than mpx_qr_workspace_bytes(m, n, nrhs)");
    MPX_CHECK_ARG(aligned16(workspace), "qr apply: workspace not 16-byte aligned");
    hipStream_t s = as_stream(stream);
    const Ws ws = ws_of(workspace, m, nrhs);
    const int last = (n - 1) / NB * NB;
    for (int q = 0; q <= last; q += NB) {  // Q^T = H_{n-1} .. H_0: the panels in order; Q: in reverse
        const int j0 = transpose ? q : last - q;
        const int jb = n - j0 < NB ? n - j0 : NB;
        if (int rc = block_apply(qr + (int64_t)j0 * pitch + j0, pitch, m - j0, jb, tau + j0, b + (int64_t)j0 * pitch_b,
                                 pitch_b, nrhs, transpose != 0, ws, 14, s))
            return rc;
    }
    return MPX_OK;
}

extern "C" int mpx_qr_rsolve_f64(const double *qr, int n, int64_t pitch, double *b, int nrhs, int64_t pitch_b,
                                 void *stream) {
    MPX_CHECK_ARG(n >= 0 && nrhs >= 0, "qr rsolve: n < 0 or nrhs < 0");
    MPX_CHECK_ARG(pitch >= n && pitch_b >= nrhs, "qr rsolve: pitch < n or pitch_b < nrhs");
    if (n == 0 || nrhs == 0) return MPX_OK;
    MPX_CHECK_ARG(qr && b, "qr rsolve: null pointer");
    hipStream_t s = as_stream(stream);
    for (int k0 = (n - 1) / NB * NB; k0 >= 0; k0 -= NB) {  // R x = y
        const int jb = n - k0 < NB ? n - k0 : NB;
        double *bk = b + (int64_t)k0 * pitch_b;
        if (int rc = launch_dense_trsm<true>(qr + (int64_t)k0 * pitch + k0, pitch, jb, bk, pitch_b, nrhs, s)) return rc;
        if (int rc = launch_dense_update<kRows>(qr + k0, pitch, bk, pitch_b, b, pitch_b, k0, nrhs, jb, s)) return rc;
    }
    return MPX_OK;
}
