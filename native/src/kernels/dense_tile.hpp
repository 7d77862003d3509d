// lab4: what the dense fp64 factorisations (lu.hip, chol.hip, qr.hip) share: the
// 64 x 64 tile on v_mfma_f64_16x16x4_f64 with its two LDS operand layouts, the
// update kernel built from it, the lane-per-column triangular solve, the init
// kernel and the finished-workgroup handshake of the panel-column kernels.
// Header only, internal linkage: every translation unit that includes it keeps
// its own code object.
#pragma once

#include "internal.hpp"

namespace mpx {
namespace {

constexpr int kTile = 64;         // edge of a workgroup's tile of C = the largest K of an operand block
constexpr int kNoUnit = 1 << 30;  // "this block is not a panel's diagonal block"

typedef double f64x4 __attribute__((ext_vector_type(4)));

// A workgroup of four waves owns a 64 x 64 tile of C; wave w takes the 32 x 32
// quarter at (32 (w >> 1), 32 (w & 1)) as 2 x 2 MFMA tiles:
//   A operand: lane l holds A[l & 15][4 t + (l >> 4)], B: B[4 t + (l >> 4)][l & 15],
//   C/D: lane l, reg r holds row (l >> 4) + 4 r, column l & 15 (the f64 map).
// The two LDS layouts of a 64 x 64 operand block, both filled with coalesced
// global reads and vector LDS stores, both read without conflicts:
//   rows    X[r][k ^ ((r & 15) << 1)] from a matrix whose rows hold k contiguously;
//           an operand read X[base + (l & 15)][4 t + (l >> 4)] then takes 32 distinct
//           bank pairs per half-wave: bit 0 from l >> 4, bits 1..4 from l & 15
//           (a shift of << 2, the LU update's first form, left rows r and r + 8 on
//           the same pairs: 8 conflict cycles per LDS instruction on the counters,
//           0 with << 1);
//   kmajor  X[k][c ^ ((k & 3) << 4)] from a matrix whose rows hold c contiguously;
//           the four k rows of an operand read take distinct segments.
// An operand uses the layout its global storage has, so nothing is transposed on
// the way into LDS: the Cholesky update reads L21 twice as `rows` (its B operand
// B[k][c] = L21[n0 + c][k] is the A read of other rows), a backward update reads
// L^T's block as `kmajor`, V^T C reads both operands as `kmajor` (k = the row).
enum TileLayout { kRows, kKMajor };

// `unit` is the index of a block's first row within a QR panel's V, or kNoUnit:
// rows below 64 of V are the panel's diagonal block, which holds R on and above
// its diagonal and stands for a unit lower triangle.
__device__ __forceinline__ double unit_lower(double v, int row, int col) {
    return row >= kTile || row > col ? v : (row == col ? 1.0 : 0.0);
}

// Zero-filled outside [0, rmax) x [0, kmax) resp. [0, kmax) x [0, cmax); NEG
// stages the negative. V2: 16-byte global loads (a 16-byte aligned src with an
// even ld).
template <bool V2, bool NEG>
__device__ __forceinline__ void stage_rows(double *__restrict__ dst, const double *__restrict__ src, int64_t ld,
                                           int rmax, int kmax, int tid, int unit = kNoUnit) {
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

template <bool V2, bool NEG>
__device__ __forceinline__ void stage_kmajor(double *__restrict__ dst, const double *__restrict__ src, int64_t ld,
                                             int kmax, int cmax, int tid, int unit = kNoUnit) {
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
            if (NEG) v = double2{-v.x, -v.y};
            *reinterpret_cast<double2 *>(&dst[k * 64 + (c ^ ((k & 3) << 4))]) = v;
        }
    } else {
#pragma unroll
        for (int it = 0; it < 16; ++it) {
            const int e = tid + it * 256;
            const int k = e >> 6, c = e & 63;
            double v = (k < kmax && c < cmax) ? src[(int64_t)k * ld + c] : 0.0;
            if (unit != kNoUnit && k < kmax && c < cmax) v = unit_lower(v, unit + k, c);
            dst[k * 64 + (c ^ ((k & 3) << 4))] = NEG ? -v : v;
        }
    }
}

// A wave's place in the tile, from threadIdx.x (a workgroup of 256 threads).
// The functions below work it out themselves and take no wave or lane argument:
// the compiler simplifies each of them on its own before it inlines them, and
// only from the thread index does it know the ranges that let it pair the two
// LDS reads of an operand into one instruction.
struct TileLane {
    int g, l15, wr, wc;
};
__device__ __forceinline__ TileLane tile_lane() {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    return TileLane{lane >> 4, lane & 15, (wave >> 1) * 32, (wave & 1) * 32};
}

// acc += A B over k in [k_begin, k_end) of the staged blocks, 16 at a time
// (uniform: a narrower K stops early). The four MFMAs of a step go in the order
// [0][0], [0][1], [1][0], [1][1]; every accumulator sees k ascending.
template <TileLayout A_LAYOUT, TileLayout B_LAYOUT>
__device__ __forceinline__ void tile_mma(f64x4 (&acc)[2][2], const double *As, const double *Bs, int k_begin,
                                         int k_end) {
    const TileLane w = tile_lane();
    const int g = w.g, l15 = w.l15, wr = w.wr, wc = w.wc;
    for (int k0 = k_begin; k0 < k_end; k0 += 16) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int k = k0 + 4 * t + g;
            const int kr = k ^ (l15 << 1);
            double a0, a1, b0, b1;
            if (A_LAYOUT == kKMajor) {
                a0 = As[k * 64 + ((wr + l15) ^ (g << 4))];
                a1 = As[k * 64 + ((wr + 16 + l15) ^ (g << 4))];
            } else {
                a0 = As[(wr + l15) * 64 + kr];
                a1 = As[(wr + 16 + l15) * 64 + kr];
            }
            if (B_LAYOUT == kKMajor) {
                b0 = Bs[k * 64 + ((wc + l15) ^ (g << 4))];
                b1 = Bs[k * 64 + ((wc + 16 + l15) ^ (g << 4))];
            } else {
                b0 = Bs[(wc + l15) * 64 + kr];
                b1 = Bs[(wc + 16 + l15) * 64 + kr];
            }
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        }
    }
}

// The tile at (m0, n0) of C (M x N) -= A B over k in [0, K) of the staged
// blocks: the wave's quarter of C into the accumulators (+0.0 outside C), the
// barrier that completes the staging, the MFMAs, the predicated store. LOWER: C
// is the lower triangle of a square matrix, only col <= row is touched. A wave
// with `idle` set (wave-uniform) takes part in the barrier and nothing else.
// The load and the store are one function with the K loop between them, not
// helpers of their own that share the accumulators by reference: built that way
// the accumulators travel between AGPRs and VGPRs in every pass of the K loop.
template <bool LOWER, TileLayout A_LAYOUT, TileLayout B_LAYOUT>
__device__ __forceinline__ void tile_update(double *C, int64_t ldc, int m0, int n0, int M, int N, const double *As,
                                            const double *Bs, int K, bool idle = false) {
    const TileLane w = tile_lane();
    f64x4 acc[2][2];
#pragma unroll
    for (int im = 0; im < 2; ++im)
#pragma unroll
        for (int in = 0; in < 2; ++in)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = m0 + w.wr + im * 16 + w.g + 4 * r, col = n0 + w.wc + in * 16 + w.l15;
                const bool in_c = LOWER ? (row < M && col <= row) : (row < M && col < N);
                acc[im][in][r] = in_c ? C[(int64_t)row * ldc + col] : 0.0;
            }
    __syncthreads();
    if (idle) return;
    tile_mma<A_LAYOUT, B_LAYOUT>(acc, As, Bs, 0, K);
#pragma unroll
    for (int im = 0; im < 2; ++im)
#pragma unroll
        for (int in = 0; in < 2; ++in)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = m0 + w.wr + im * 16 + w.g + 4 * r, col = n0 + w.wc + in * 16 + w.l15;
                const bool in_c = LOWER ? (row < M && col <= row) : (row < M && col < N);
                if (in_c) C[(int64_t)row * ldc + col] = acc[im][in][r];
            }
}

// C (M x N) -= A B, K <= kTile, B stored K x N. A_LAYOUT kRows: A stored M x K;
// kKMajor: C -= A^T B with A stored K x M. A workgroup stages -A and B in LDS
// once (no K loop to pipeline) and updates its tile. UNIT (kRows): A is a QR
// panel's V, whose first block is masked to unit lower.
template <TileLayout A_LAYOUT, bool V2, bool UNIT>
__global__ __launch_bounds__(256) void dense_update_kernel(const double *__restrict__ A, int64_t lda,
                                                           const double *__restrict__ B, int64_t ldb, double *C,
                                                           int64_t ldc, int M, int N, int K) {
    static_assert(!UNIT || A_LAYOUT == kRows, "the unit-lower mask is the rows layout's");
    __shared__ __attribute__((aligned(16))) double As[kTile * 64];
    __shared__ __attribute__((aligned(16))) double Bs[kTile * 64];
    const int tid = threadIdx.x;
    const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
    if (A_LAYOUT == kKMajor)
        stage_kmajor<V2, true>(As, A + m0, lda, K, M - m0, tid);
    else
        stage_rows<V2, true>(As, A + (int64_t)m0 * lda, lda, M - m0, K, tid, UNIT ? m0 : kNoUnit);
    stage_kmajor<V2, false>(Bs, B + n0, ldb, K, N - n0, tid);
    tile_update<false, A_LAYOUT, kKMajor>(C, ldc, m0, n0, M, N, As, Bs, K);
}

template <TileLayout A_LAYOUT, bool UNIT = false>
int launch_dense_update(const double *A, int64_t lda, const double *B, int64_t ldb, double *C, int64_t ldc, int M,
                        int N, int K, hipStream_t s) {
    if (M <= 0 || N <= 0 || K <= 0) return MPX_OK;
    const dim3 grid((N + 63) / 64, (M + 63) / 64);
    if (aligned16(A) && aligned16(B) && lda % 2 == 0 && ldb % 2 == 0)
        hipLaunchKernelGGL((dense_update_kernel<A_LAYOUT, true, UNIT>), grid, dim3(256), 0, s, A, lda, B, ldb, C, ldc,
                           M, N, K);
    else
        hipLaunchKernelGGL((dense_update_kernel<A_LAYOUT, false, UNIT>), grid, dim3(256), 0, s, A, lda, B, ldb, C,
                           ldc, M, N, K);
    MPX_RETURN_IF_HIP_ERROR(hipGetLastError());
    return MPX_OK;
}

// B (jb x ncols) <- T^-1 B by substitution, T the jb x jb (jb <= kTile) block at
// t: its strict lower part with a unit diagonal, or (UPPER) its upper part with
// one division by the diagonal, k ascending. T sits in LDS and is read as
// broadcasts; a lane owns a column of B, which it keeps in its own LDS column
// (64 doubles in registers with the loops unrolled spilled).
template <bool UPPER>
__global__ __launch_bounds__(64) void dense_trsm_kernel(const double *__restrict__ t, int64_t ldt, int jb,
                                                        double *__restrict__ b, int64_t ldb, int ncols) {
    __shared__ double s[kTile][kTile];
    __shared__ double xs[kTile][64];
    const int tid = threadIdx.x;
    for (int e = tid; e < kTile * kTile; e += 64) {
        const int i = e >> 6, k = e & 63;
        if (i < jb && k < jb) s[i][k] = t[(int64_t)i * ldt + k];
    }
    const int col = blockIdx.x * 64 + tid;
    const bool ok = col < ncols;
#pragma unroll 8
    for (int i = 0; i < jb; ++i) xs[i][tid] = ok ? b[(int64_t)i * ldb + col] : 0.0;
    __syncthreads();
    if (!UPPER) {
        for (int i = 1; i < jb; ++i) {
            double acc = xs[i][tid];
#pragma unroll 4
            for (int k = 0; k < i; ++k) acc -= s[i][k] * xs[k][tid];
            xs[i][tid] = acc;
        }
    } else {
        for (int i = jb - 1; i >= 0; --i) {
            double acc = xs[i][tid];
#pragma unroll 4
            for (int k = i + 1; k < jb; ++k) acc -= s[i][k] * xs[k][tid];
            xs[i][tid] = acc / s[i][i];
        }
    }
    if (!ok) return;
#pragma unroll 8
    for (int i = 0; i < jb; ++i) b[(int64_t)i * ldb + col] = xs[i][tid];
}

template <bool UPPER>
int launch_dense_trsm(const double *t, int64_t ldt, int jb, double *b, int64_t ldb, int ncols, hipStream_t s) {
    if (ncols <= 0 || jb <= 0) return MPX_OK;
    hipLaunchKernelGGL(dense_trsm_kernel<UPPER>, dim3((ncols + 63) / 64), dim3(64), 0, s, t, ldt, jb, b, ldb, ncols);
    MPX_RETURN_IF_HIP_ERROR(hipGetLastError());
    return MPX_OK;
}

// (a template only so that the translation units that do not launch it do not carry it)
template <int = 0>
__global__ void dense_init_kernel(int32_t *info, unsigned *counter) {
    *info = 0;
    *counter = 0;
}

// The handshake that ends a panel-column kernel: every workgroup counts itself
// in after its stores, and the one that finds all the others counted (nobody
// ever waits) sees their stores and goes on alone. True in that workgroup, in
// all of its threads; it resets *counter when it is done.
__device__ __forceinline__ bool last_workgroup(unsigned *counter, int *s_flag) {
    __threadfence();  // this thread's stores before the counter below
    __syncthreads();
    if (threadIdx.x == 0) *s_flag = atomicAdd(counter, 1u) == gridDim.x - 1;
    __syncthreads();
    if (!*s_flag) return false;
    __threadfence();  // every other workgroup's stores are visible
    return true;
}

}  // namespace
}  // namespace mpx
