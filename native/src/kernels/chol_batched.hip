// lab4, batched: Cholesky A = L L^T of many small symmetric positive definite
// fp64 matrices, lower storage, and the solve with the factors (the contract is
// in capi.h). Plain VALU arithmetic in the operation order of the unblocked CPU
// reference, every operation rounded once, so for n <= 64 every member agrees
// with it bit for bit.
//
//   factor   chol_batched_factor_kernel<NP>, NP = 8 / 16 / 32 / 64 >= n: a lane
//            owns one row in NP registers (every loop unrolled, static register
//            indices), 64 / NP members share a wave. Right-looking, the order of
//            chol.hip's diag_block: at step j the reduced diagonal is broadcast
//            within the member's NP lanes, every lane forms the same square root
//            and the same failure flag, the rows below j divide and publish
//            column j of L through one LDS row per member slot, and a lane
//            subtracts the k = j term from its elements j + 1 .. row. One launch,
//            one global read and one global write of the lower triangles; info
//            is written by the kernel.
//   solve    chol_batched_solve_kernel<NP>: a lane is one (member, right-hand
//            side) pair, 64 / min(nrhs, 64) members per wave; the lane's column
//            of B lives in its own LDS column, L is read directly (the lanes of
//            one member read the same address), its lower triangle only.
//   n > 64   a loop over the single-matrix entries of chol.hip on the same stream.
#include <climits>

#include "internal.hpp"

namespace mpx {
MPX_MODULE_ANCHOR(chol_batched)

namespace {

constexpr int kSmall = 64;  // largest n of the one-launch kernels

// Columns K .. NP-1, unrolled by recursion so that every register index is a
// constant. n is uniform over the workgroup; sl is the member slot's pair of
// LDS rows (column K goes through row K & 1, so one barrier per column is
// enough: the row written at step K + 2 was last read before the barrier of
// step K + 1).
template <int NP, int K>
__device__ __forceinline__ void factor_steps(double (&r)[NP], int &bad, const int n, const int row,
                                             double (*sl)[64]) {
    if constexpr (K < NP) {
        if (K >= n) return;  // uniform over the workgroup
        const double t = __shfl(r[K], K, NP);  // the reduced diagonal, from the lane of row K
        const double d = sqrt(t);
        if (!(t > 0.0) && bad == 0) bad = K + 1;  // zero, negative and NaN; go on regardless
        const double l = r[K] / d;                // what the rows below K keep
        r[K] = row == K ? d : l;                  // rows above K hold nothing of column K
        if constexpr (K + 1 < NP) {
            if (K + 1 < n) {
                sl[K & 1][row] = l;
                __syncthreads();
                // elements K + 1 .. row take their k = K term; the registers past
                // the row take one too, and nobody looks at them: they are never
                // stored, and what they publish sits at LDS slots nobody reads
#pragma unroll
                for (int c = K + 1; c < NP; ++c) r[c] = r[c] - l * sl[K & 1][c];
            }
        }
        factor_steps<NP, K + 1>(r, bad, n, row, sl);
    }
}

// One wave per workgroup; lane = (member slot g, row) with NP lanes per member.
template <int NP>
__global__ __launch_bounds__(64) void chol_batched_factor_kernel(double *__restrict__ a, int batch, int n,
                                                                 int64_t pitch, int64_t stride,
                                                                 int32_t *__restrict__ info) {
    __shared__ double s_l[2][64];  // column j of L per member slot, two steps deep
    const int lane = threadIdx.x;
    const int g = lane / NP, row = lane % NP;
    const int64_t m = (int64_t)blockIdx.x * (64 / NP) + g;
    const bool live = m < batch && row < n;  // padded rows and members past the end touch no memory
    double *arow = a + (live ? m * stride + (int64_t)row * pitch : 0);
    double r[NP];
#pragma unroll
    for (int c = 0; c < NP; ++c) r[c] = 0.0;
    if (live) {
        // clamped addresses (always inside the row's part of the lower triangle)
        // make the loads unconditional: all in flight together
#pragma unroll
        for (int c = 0; c < NP; ++c) {
            const double v = arow[c < row ? c : row];
            r[c] = c <= row ? v : 0.0;
        }
    }
    int bad = 0;
    factor_steps<NP, 0>(r, bad, n, row, reinterpret_cast<double(*)[64]>(&s_l[0][g * NP]));
    if (!live) return;
    if (row == 0) info[m] = bad;
#pragma unroll
    for (int c = 0; c < NP; ++c)
        if (c <= row) arow[c] = r[c];
}

// One wave per workgroup, `mats` = 64 / min(nrhs, 64) members in it; lane =
// (member slot, column). The lane's column of B sits in its own LDS column.
template <int NP>
__global__ __launch_bounds__(64) void chol_batched_solve_kernel(const double *__restrict__ l, int batch, int n,
                                                                int64_t pitch, int64_t stride,
                                                                double *__restrict__ b, int nrhs, int64_t pitch_b,
                                                                int64_t stride_b, int width, int chunks) {
    __shared__ double xs[NP][64];
    const int lane = threadIdx.x;
    const int mats = 64 / width;
    const int64_t blk = blockIdx.x / chunks;
    const int chunk = blockIdx.x % chunks;
    const int g = lane / width;
    const int64_t m = blk * mats + g;
    const int col = chunk * 64 + lane % width;
    if (g >= mats || m >= batch || col >= nrhs) return;  // no barrier below: a lane works alone
    const double *t = l + m * stride;
    double *bc = b + m * stride_b + col;
    for (int i = 0; i < n; ++i) xs[i][lane] = bc[(int64_t)i * pitch_b];
    for (int i = 0; i < n; ++i) {  // L y = b
        const double *ti = t + (int64_t)i * pitch;
        double acc = xs[i][lane];
#pragma unroll 4
        for (int k = 0; k < i; ++k) acc -= ti[k] * xs[k][lane];
        xs[i][lane] = acc / ti[i];
    }
    for (int i = n - 1; i >= 0; --i) {  // L^T x = y: column i of L below the diagonal
        const double *ci = t + i;
        double acc = xs[i][lane];
#pragma unroll 4
        for (int k = i + 1; k < n; ++k) acc -= ci[(int64_t)k * pitch] * xs[k][lane];
        xs[i][lane] = acc / ci[(int64_t)i * pitch];
    }
    for (int i = 0; i < n; ++i) bc[(int64_t)i * pitch_b] = xs[i][lane];
}

template <int NP>
int launch_factor(double *a, int batch, int n, int64_t pitch, int64_t stride, int32_t *info, hipStream_t s) {
    const int per = 64 / NP;
    hipLaunchKernelGGL(chol_batched_factor_kernel<NP>, dim3((unsigned)(((int64_t)batch + per - 1) / per)), dim3(64), 0,
                       s, a, batch, n, pitch, stride, info);
    MPX_RETURN_IF_HIP_ERROR(hipGetLastError());
    return MPX_OK;
}

template <int NP>
int launch_solve(const double *l, int batch, int n, int64_t pitch, int64_t stride, double *b, int nrhs,
                 int64_t pitch_b, int64_t stride_b, int width, int64_t chunks, int64_t blocks, hipStream_t s) {
    hipLaunchKernelGGL(chol_batched_solve_kernel<NP>, dim3((unsigned)blocks), dim3(64), 0, s, l, batch, n, pitch,
                       stride, b, nrhs, pitch_b, stride_b, width, (int)chunks);
    MPX_RETURN_IF_HIP_ERROR(hipGetLastError());
    return MPX_OK;
}

// stride >= (n - 1) * pitch + width without overflow (pitch >= width >= 1, n >= 1 here)
bool stride_covers(int64_t stride, int n, int64_t pitch, int width) {
    if (pitch > (INT64_MAX - width) / (n > 1 ? n - 1 : 1)) return false;
    return stride >= (int64_t)(n - 1) * pitch + width;
}

}  // namespace
}  // namespace mpx

using namespace mpx;

extern "C" int mpx_chol_factor_batched_f64(double *a, int batch, int n, int64_t pitch, int64_t stride, int32_t *info,
                                           void *stream) {
    MPX_CHECK_ARG(batch >= 0 && n >= 0, "chol batched: batch < 0 or n < 0");
    MPX_CHECK_ARG(pitch >= n, "chol batched: pitch < n");
    if (batch == 0 || n == 0) return MPX_OK;
    MPX_CHECK_ARG(batch == 1 || stride_covers(stride, n, pitch, n), "chol batched: stride < (n - 1) * pitch + n");
    MPX_CHECK_ARG(a && info, "chol batched: null pointer");
    hipStream_t s = as_stream(stream);
    if (n <= 8) return launch_factor<8>(a, batch, n, pitch, stride, info, s);
    if (n <= 16) return launch_factor<16>(a, batch, n, pitch, stride, info, s);
    if (n <= 32) return launch_factor<32>(a, batch, n, pitch, stride, info, s);
    if (n <= kSmall) return launch_factor<64>(a, batch, n, pitch, stride, info, s);
    for (int m = 0; m < batch; ++m)  // stream-ordered; every member has its own info word
        if (int rc = mpx_chol_factor_f64(a + (int64_t)m * stride, n, pitch, info + m, stream)) return rc;
    return MPX_OK;
}

extern "C" int mpx_chol_solve_batched_f64(const double *l, int batch, int n, int64_t pitch, int64_t stride, double *b,
                                          int nrhs, int64_t pitch_b, int64_t stride_b, void *stream) {
    MPX_CHECK_ARG(batch >= 0 && n >= 0 && nrhs >= 0, "chol batched solve: batch < 0, n < 0 or nrhs < 0");
    MPX_CHECK_ARG(pitch >= n && pitch_b >= nrhs, "chol batched solve: pitch < n or pitch_b < nrhs");
    if (batch == 0 || n == 0 || nrhs == 0) return MPX_OK;
    MPX_CHECK_ARG(batch == 1 || (stride_covers(stride, n, pitch, n) && stride_covers(stride_b, n, pitch_b, nrhs)),
                  "chol batched solve: stride < (n - 1) * pitch + n or stride_b < (n - 1) * pitch_b + nrhs");
    MPX_CHECK_ARG(l && b, "chol batched solve: null pointer");
    if (n > kSmall) {
        for (int m = 0; m < batch; ++m)
            if (int rc = mpx_chol_solve_f64(l + (int64_t)m * stride, n, pitch, b + (int64_t)m * stride_b, nrhs,
                                            pitch_b, stream))
                return rc;
        return MPX_OK;
    }
    const int width = nrhs < 64 ? nrhs : 64;
    const int mats = 64 / width;
    const int64_t chunks = ((int64_t)nrhs + 63) / 64;
    const int64_t blocks = (((int64_t)batch + mats - 1) / mats) * chunks;
    MPX_CHECK_ARG(blocks <= INT_MAX, "chol batched solve: batch x nrhs too large for one launch");
    hipStream_t s = as_stream(stream);
    if (n <= 8) return launch_solve<8>(l, batch, n, pitch, stride, b, nrhs, pitch_b, stride_b, width, chunks, blocks, s);
    if (n <= 16) return launch_solve<16>(l, batch, n, pitch, stride, b, nrhs, pitch_b, stride_b, width, chunks, blocks, s);
    if (n <= 32) return launch_solve<32>(l, batch, n, pitch, stride, b, nrhs, pitch_b, stride_b, width, chunks, blocks, s);
    return launch_solve<64>(l, batch, n, pitch, stride, b, nrhs, pitch_b, stride_b, width, chunks, blocks, s);
}
