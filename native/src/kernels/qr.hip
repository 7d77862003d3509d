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
//   apply     qr_update_kernel: C -= V Z, K = 64, both operands staged once.
//
// A factorisation is n + ceil(n / 64) panel launches, four more per panel that
// has columns to its right, and one init: n + O(n / 64). An application of Q or
// Q^T to a block is four launches per panel. Nothing depends on the matrix's
// width but which columns exist: the row chunks and the rows per panel
// workgroup follow from m and the column's index alone, so column j of the
// result is a function of columns 0 .. j.
//
// rsolve is blocked back substitution with R: qr_trsm_kernel on the diagonal
// blocks, qr_update_kernel between them.
#include "internal.hpp"

namespace mpx {
MPX_MODULE_ANCHOR(qr)

namespace {

constexpr int NB = 64;             // panel width = K of the apply
constexpr int kChunkRows = 1024;   // rows of one partial W (16 K steps of 64)
constexpr int kWsHeader = 256;     // bytes in front: word 0 = the finished-workgroup counter
constexpr int kStateDoubles = 128; // w[64] of the pending rank-1 update, [64] = alpha - beta (0: none)
constexpr int kNoUnit = 1 << 30;   // "this block is not the panel's diagonal block"

typedef double f64x4 __attribute__((ext_vector_type(4)));

// rows per workgroup of the panel kernel: 64, more for very tall matrices so
// that the fold stays within 256 partials; a function of m alone
int panel_rows(int m) { return 64 * (m > 16384 ? (m + 16383) / 16384 : 1); }

__global__ void qr_init_kernel(int32_t *info, unsigned *counter) {
    *info = 0;
    *counter = 0;
}

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
    __threadfence();  // this thread's stores before the counter below
    __syncthreads();
    if (threadIdx.x == 0) s_flag = atomicAdd(counter, 1u) == gridDim.x - 1;
    __syncthreads();
    if (!s_flag) return;
    // the last workgroup to finish: every other one's rows and partials are visible
    __threadfence();
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

// The two LDS layouts of a 64 x 64 MFMA operand block (chol.hip's, with its
// swizzles), zero-filled outside [0, rmax) x [0, kmax) resp. [0, kmax) x [0, cmax).
// `unit` is the index of the block's first row within the panel's V, or
// kNoUnit: rows below 64 of V are the panel's diagonal block, which holds R on
// and above its diagonal and stands for a unit lower triangle.
__device__ __forceinline__ double unit_lower(double v, int row, int col) {
    return row >= NB || row > col ? v : (row == col ? 1.0 : 0.0);
}

template <bool V2, bool NEG>
__device__ __forceinline__ void stage_rows(double *__restrict__ dst, const double *__restrict__ src, int64_t ld,
                                           int rmax, int kmax, int tid, int unit) {
    if (V2) {
#pragma unroll
        for (int it = 0; it < 8; ++it) {
            const int e = tid + it * 256;
            const int r = e >> 5, k = (e & 31) * 2;
            double2 v = {0.0, 0.0};
            if (r < rmax) {
                const double *p = src + (int64_t)r * ld + k;
                if (k + 1 < kmax)
                    v = *reinterpret_cast<const double2 *>(p);
                else if (k < kmax)
                    v.x = *p;
                if (unit != kNoUnit) {
                    if (k < kmax) v.x = unit_lower(v.x, unit + r, k);
                    if (k + 1 < kmax) v.y = unit_lower(v.y, unit + r, k + 1);
                }
            }
            if (NEG) v = double2{-v.x, -v.y};
            *reinterpret_cast<double2 *>(&dst[r * 64 + (k ^ ((r & 15) << 1))]) = v;
        }
    } else {
#pragma unroll
        for (int it = 0; it < 16; ++it) {
            const int e = tid + it * 256;
            const int r = e >> 6, k = e & 63;
            double v = (r < rmax && k < kmax) ? src[(int64_t)r * ld + k] : 0.0;
            if (unit != kNoUnit && r < rmax && k < kmax) v = unit_lower(v, unit + r, k);
            dst[r * 64 + (k ^ ((r & 15) << 1))] = NEG ? -v : v;
        }
    }
}

template <bool V2>
__device__ __forceinline__ void stage_kmajor(double *__restrict__ dst, const double *__restrict__ src, int64_t ld,
                                             int kmax, int cmax, int tid, int unit) {
    if (V2) {
#pragma unroll
        for (int it = 0; it < 8; ++it) {
            const int e = tid + it * 256;
            const int k = e >> 5, c = (e & 31) * 2;
            double2 v = {0.0, 0.0};
            if (k < kmax) {
                const double *p = src + (int64_t)k * ld + c;
                if (c + 1 < cmax)
                    v = *reinterpret_cast<const double2 *>(p);
                else if (c < cmax)
                    v.x = *p;
                if (unit != kNoUnit) {
                    if (c < cmax) v.x = unit_lower(v.x, unit + k, c);
                    if (c + 1 < cmax) v.y = unit_lower(v.y, unit + k, c + 1);
                }
            }
            *reinterpret_cast<double2 *>(&dst[k * 64 + (c ^ ((k & 3) << 4))]) = v;
        }
    } else {
#pragma unroll
        for (int it = 0; it < 16; ++it) {
            const int e = tid + it * 256;
            const int k = e >> 6, c = e & 63;
            double v = (k < kmax && c < cmax) ? src[(int64_t)k * ld + c] : 0.0;
            if (unit != kNoUnit && k < kmax && c < cmax) v = unit_lower(v, unit + k, c);
            dst[k * 64 + (c ^ ((k & 3) << 4))] = v;
        }
    }
}

// W_chunk (64 x 64 tile) = V^T C over the rows of one chunk. V: rows x jb at V
// (the panel, its first 64 rows the diagonal block), C: rows x N. blockIdx.x is
// the column tile, tile ntiles is V itself (V^T V for T), blockIdx.y the chunk.
// Both operands are k-major as they lie in memory (k = the row), so nothing is
// transposed on the way into LDS:
//   A operand: lane l holds V[4 t + (l >> 4)][l & 15], B: C[4 t + (l >> 4)][l & 15],
//   D: lane l, reg r holds W row (l >> 4) + 4 r, column l & 15 (the f64 map).
// Every K step of 64 rows is staged and consumed between two barriers. The
// tile is stored whole: past jb and past N it holds the zeros of the padding.
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
        stage_kmajor<V2>(As, vk, ldv, rows - k0, jb, tid, k0);
        if (tile < ntiles)
            stage_kmajor<V2>(Bs, C + (int64_t)k0 * ldc + n0, ldc, rows - k0, N - n0, tid, kNoUnit);
        else
            stage_kmajor<V2>(Bs, vk, ldv, rows - k0, jb, tid, k0);
        __syncthreads();
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const int k = 4 * t + g;
            const double a0 = As[k * 64 + ((wr + l15) ^ (g << 4))];
            const double a1 = As[k * 64 + ((wr + 16 + l15) ^ (g << 4))];
            const double b0 = Bs[k * 64 + ((wc + l15) ^ (g << 4))];
            const double b1 = Bs[k * 64 + ((wc + 16 + l15) ^ (g << 4))];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        }
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

// C (M x N) -= A (M x K) B (K x N), K <= NB: lu_update_kernel's shape with
// chol.hip's swizzle. A workgroup owns a 64 x 64 tile of C, stages -A (rows
// layout) and B (k-major) once, each of its four waves takes a 32 x 32 quarter
// as 2 x 2 MFMA tiles with C loaded into the accumulators.
//   A operand: lane l holds A[l & 15][4 t + (l >> 4)], B: B[4 t + (l >> 4)][l & 15],
//   C/D: lane l, reg r holds row (l >> 4) + 4 r, column l & 15.
// UNIT: A is a panel's V, whose first block is masked to unit lower.
template <bool V2, bool UNIT>
__global__ __launch_bounds__(256) void qr_update_kernel(const double *__restrict__ A, int64_t lda,
                                                        const double *__restrict__ B, int64_t ldb, double *C,
                                                        int64_t ldc, int M, int N, int K) {
    __shared__ __attribute__((aligned(16))) double As[NB * 64];
    __shared__ __attribute__((aligned(16))) double Bs[NB * 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
    stage_rows<V2, true>(As, A + (int64_t)m0 * lda, lda, M - m0, K, tid, UNIT ? m0 : kNoUnit);
    stage_kmajor<V2>(Bs, B + n0, ldb, K, N - n0, tid, kNoUnit);
    const int g = lane >> 4, l15 = lane & 15;
    const int wr = (wave >> 1) * 32, wc = (wave & 1) * 32;
    f64x4 acc[2][2];
#pragma unroll
    for (int im = 0; im < 2; ++im)
#pragma unroll
        for (int in = 0; in < 2; ++in)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = m0 + wr + im * 16 + g + 4 * r, col = n0 + wc + in * 16 + l15;
                acc[im][in][r] = (row < M && col < N) ? C[(int64_t)row * ldc + col] : 0.0;
            }
    __syncthreads();
    for (int k0 = 0; k0 < K; k0 += 16) {  // uniform: a ragged block stops early
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int k = k0 + 4 * t + g;
            const int kr = k ^ (l15 << 1);
            const double a0 = As[(wr + l15) * 64 + kr], a1 = As[(wr + 16 + l15) * 64 + kr];
            const double b0 = Bs[k * 64 + ((wc + l15) ^ (g << 4))], b1 = Bs[k * 64 + ((wc + 16 + l15) ^ (g << 4))];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        }
    }
#pragma unroll
    for (int im = 0; im < 2; ++im)
#pragma unroll
        for (int in = 0; in < 2; ++in)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = m0 + wr + im * 16 + g + 4 * r, col = n0 + wc + in * 16 + l15;
                if (row < M && col < N) C[(int64_t)row * ldc + col] = acc[im][in][r];
            }
}

// B (jb x ncols) <- R^-1 B by back substitution, R the upper jb x jb (jb <= NB)
// block at t: a lane owns a column of B, R sits in LDS and is read as
// broadcasts, k ascending, one division by the diagonal.
__global__ __launch_bounds__(64) void qr_trsm_kernel(const double *__restrict__ t, int64_t ldt, int jb,
                                                     double *__restrict__ b, int64_t ldb, int ncols) {
    __shared__ double s[NB][NB];
    __shared__ double xs[NB][64];
    const int tid = threadIdx.x;
    for (int e = tid; e < NB * NB; e += 64) {
        const int i = e >> 6, k = e & 63;
        if (i < jb && k < jb && k >= i) s[i][k] = t[(int64_t)i * ldt + k];
    }
    const int col = blockIdx.x * 64 + tid;
    const bool ok = col < ncols;
#pragma unroll 8
    for (int i = 0; i < jb; ++i) xs[i][tid] = ok ? b[(int64_t)i * ldb + col] : 0.0;
    __syncthreads();
    for (int i = jb - 1; i >= 0; --i) {
        double acc = xs[i][tid];
#pragma unroll 4
        for (int k = i + 1; k < jb; ++k) acc -= s[i][k] * xs[k][tid];
        xs[i][tid] = acc / s[i][i];
    }
    if (!ok) return;
#pragma unroll 8
    for (int i = 0; i < jb; ++i) b[(int64_t)i * ldb + col] = xs[i][tid];
}

template <bool UNIT>
int launch_update(const double *A, int64_t lda, const double *B, int64_t ldb, double *C, int64_t ldc, int M, int N,
                  int K, hipStream_t s) {
    if (M <= 0 || N <= 0 || K <= 0) return MPX_OK;
    const dim3 grid((N + 63) / 64, (M + 63) / 64);
    if (aligned16(A) && aligned16(B) && lda % 2 == 0 && ldb % 2 == 0)
        hipLaunchKernelGGL((qr_update_kernel<true, UNIT>), grid, dim3(256), 0, s, A, lda, B, ldb, C, ldc, M, N, K);
    else
        hipLaunchKernelGGL((qr_update_kernel<false, UNIT>), grid, dim3(256), 0, s, A, lda, B, ldb, C, ldc, M, N, K);
    MPX_RETURN_IF_HIP_ERROR(hipGetLastError());
    return MPX_OK;
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
    if (mask & 8) return launch_update<true>(v, ldv, ws.Z, ldz, c, ldc, rows, N, jb, s);
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
    hipLaunchKernelGGL(qr_init_kernel, dim3(1), dim3(1), 0, s, info, ws.counter);
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
        hipLaunchKernelGGL(qr_init_kernel, dim3(1), dim3(1), 0, as_stream(stream), info, ws.counter);
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
        hipLaunchKernelGGL(qr_trsm_kernel, dim3((nrhs + 63) / 64), dim3(64), 0, s, qr + (int64_t)k0 * pitch + k0,
                           pitch, jb, bk, pitch_b, nrhs);
        MPX_RETURN_IF_HIP_ERROR(hipGetLastError());
        if (int rc = launch_update<false>(qr + k0, pitch, bk, pitch_b, b, pitch_b, k0, nrhs, jb, s)) return rc;
    }
    return MPX_OK;
}
