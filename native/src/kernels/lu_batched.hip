// lab4, batched: LU with partial pivoting of many small fp64 matrices and the
// solve with the factors (the contract is in capi.h). Plain VALU arithmetic in
// the operation order of the unblocked CPU reference, every operation rounded
// once, so for n <= 64 the results agree with it bit for bit.
//
//   factor   lu_batched_factor_kernel<NP>, NP = 8 / 16 / 32 / 64 >= n: a lane
//            owns one row in NP registers (every loop unrolled, static register
//            indices), 64 / NP matrices share a wave. Rows never move: a lane
//            tracks its row's current position, the pivot search is an argmax
//            over (|a|, position) within the NP lanes of a matrix, and the
//            pivot row reaches the other lanes through one LDS row per matrix,
//            read as a broadcast. One launch, one global read and one global
//            write of the matrix; piv and info are written by the kernel.
//   solve    lu_batched_solve_kernel<NP>: a lane is one (matrix, right-hand
//            side) pair, 64 / min(nrhs, 64) matrices per wave; the lane's
//            column of B lives in its own LDS column, the factors are read
//            directly (the lanes of one matrix read the same address).
//   n > 64   a loop over the single-matrix entries of lu.hip on the same stream.
#include <climits>

#include "internal.hpp"

namespace mpx {
MPX_MODULE_ANCHOR(lu_batched)

namespace {

constexpr int kSmall = 64;  // largest n of the one-launch kernels

// the pivot rule of lu.hip: larger magnitude, the lower position among equal ones
__device__ __forceinline__ void take_better(double &bv, int &bi, double v, int i) {
    if (v > bv || (v == bv && i < bi)) {
        bv = v;
        bi = i;
    }
}

// Steps K .. NP-1 of the elimination, unrolled by recursion so that every
// register index is a constant. live, n, m and su are uniform over the NP lanes
// of a matrix; pos is the position the lane's row holds after the interchanges
// so far.
template <int NP, int K>
__device__ __forceinline__ void factor_steps(double (&r)[NP], int &pos, int &first_zero, const bool live, const int n,
                                             const int lane, const int64_t m, double *su,
                                             int32_t *__restrict__ piv) {
    if constexpr (K < NP) {
        if (K >= n) return;  // uniform over the workgroup
        // candidates: positions K..n-1. The reference starts from row K and
        // replaces it on a strictly larger magnitude only, so a NaN at position
        // K stays the pivot and a NaN below it never becomes one.
        const double mag = fabs(r[K]);
        double bv = -1.0;
        int bi = INT_MAX;
        if (live && pos >= K) {
            bv = mag != mag ? (pos == K ? __builtin_inf() : -1.0) : mag;
            bi = (pos << 6) | lane;
        }
#pragma unroll
        for (int s = NP / 2; s >= 1; s >>= 1) {  // stays inside the matrix's NP lanes
            const double ov = __shfl_xor(bv, s);
            const int oi = __shfl_xor(bi, s);
            take_better(bv, bi, ov, oi);
        }
        const bool zero = bv == 0.0;
        const int p = zero ? K : (bi >> 6);
        const int src = bi & 63;  // the lane that holds the pivot row
        if (zero && first_zero == 0) first_zero = K + 1;
        if (live && pos == K) piv[m * n + K] = p;  // the lane at position K before the interchange
        if (!zero) {
            if (pos == K)
                pos = p;
            else if (lane == src)
                pos = K;
        }
        __syncthreads();  // the previous step's reads of su
        if (live && lane == src && !zero) {
#pragma unroll
            for (int j = K; j < NP; ++j) su[j] = r[j];
        }
        __syncthreads();
        if (live && !zero && pos > K) {
            const double l = r[K] / su[K];
            r[K] = l;
#pragma unroll
            for (int j = K + 1; j < NP; ++j) r[j] = r[j] - l * su[j];
        }
        factor_steps<NP, K + 1>(r, pos, first_zero, live, n, lane, m, su, piv);
    }
}

// One wave per workgroup; lane = (matrix slot g, row) with NP lanes per matrix.
// Rows stay in their lanes; a row is stored at the position it ended at.
template <int NP>
__global__ __launch_bounds__(64) void lu_batched_factor_kernel(double *__restrict__ a, int batch, int n,
                                                               int64_t pitch, int64_t stride,
                                                               int32_t *__restrict__ piv,
                                                               int32_t *__restrict__ info) {
    __shared__ double s_u[64];  // one pivot row per matrix slot
    const int lane = threadIdx.x;
    const int g = lane / NP, row = lane % NP;
    const int64_t m = (int64_t)blockIdx.x * (64 / NP) + g;
    const bool live = m < batch && row < n;  // padded rows and matrices past the end touch no memory
    const double *arow = a + (live ? m * stride + (int64_t)row * pitch : 0);
    double r[NP];
#pragma unroll
    for (int j = 0; j < NP; ++j) r[j] = (live && j < n) ? arow[j] : 0.0;
    int pos = row;
    int first_zero = 0;
    factor_steps<NP, 0>(r, pos, first_zero, live, n, lane, m, s_u + g * NP, piv);
    if (!live) return;
    if (row == 0) info[m] = first_zero;
    double *out = a + m * stride + (int64_t)pos * pitch;
#pragma unroll
    for (int j = 0; j < NP; ++j)
        if (j < n) out[j] = r[j];
}

// One wave per workgroup, `mats` = 64 / min(nrhs, 64) matrices in it; lane =
// (matrix slot, column). The lane's column of B sits in its own LDS column.
template <int NP>
__global__ __launch_bounds__(64) void lu_batched_solve_kernel(const double *__restrict__ lu, int batch, int n,
                                                              int64_t pitch, int64_t stride,
                                                              const int32_t *__restrict__ piv, double *__restrict__ b,
                                                              int nrhs, int64_t pitch_b, int64_t stride_b, int width,
                                                              int chunks) {
    __shared__ double xs[NP][64];
    const int lane = threadIdx.x;
    const int mats = 64 / width;
    const int64_t blk = blockIdx.x / chunks;
    const int chunk = blockIdx.x % chunks;
    const int g = lane / width;
    const int64_t m = blk * mats + g;
    const int col = chunk * 64 + lane % width;
    if (g >= mats || m >= batch || col >= nrhs) return;  // no barrier below: a lane works alone
    const double *t = lu + m * stride;
    const int32_t *pv = piv + m * n;
    double *bc = b + m * stride_b + col;
    for (int i = 0; i < n; ++i) xs[i][lane] = bc[(int64_t)i * pitch_b];
    for (int k = 0; k < n; ++k) {
        const int p = pv[k];
        if (p == k || p < 0 || p >= n) continue;
        const double t0 = xs[k][lane];
        xs[k][lane] = xs[p][lane];
        xs[p][lane] = t0;
    }
    for (int i = 1; i < n; ++i) {
        const double *ti = t + (int64_t)i * pitch;
        double acc = xs[i][lane];
#pragma unroll 4
        for (int k = 0; k < i; ++k) acc -= ti[k] * xs[k][lane];
        xs[i][lane] = acc;
    }
    for (int i = n - 1; i >= 0; --i) {
        const double *ti = t + (int64_t)i * pitch;
        double acc = xs[i][lane];
#pragma unroll 4
        for (int k = i + 1; k < n; ++k) acc -= ti[k] * xs[k][lane];
        xs[i][lane] = acc / ti[i];
    }
    for (int i = 0; i < n; ++i) bc[(int64_t)i * pitch_b] = xs[i][lane];
}

template <int NP>
int launch_factor(double *a, int batch, int n, int64_t pitch, int64_t stride, int32_t *piv, int32_t *info,
                  hipStream_t s) {
    const int per = 64 / NP;
    hipLaunchKernelGGL(lu_batched_factor_kernel<NP>, dim3((unsigned)(((int64_t)batch + per - 1) / per)), dim3(64), 0, s, a, batch, n,
                       pitch, stride, piv, info);
    MPX_RETURN_IF_HIP_ERROR(hipGetLastError());
    return MPX_OK;
}

template <int NP>
int launch_solve(const double *lu, int batch, int n, int64_t pitch, int64_t stride, const int32_t *piv, double *b,
                 int nrhs, int64_t pitch_b, int64_t stride_b, hipStream_t s) {
    const int width = nrhs < 64 ? nrhs : 64;
    const int mats = 64 / width;
    const int64_t chunks = ((int64_t)nrhs + 63) / 64;
    const int64_t blocks = (((int64_t)batch + mats - 1) / mats) * chunks;
    MPX_CHECK_ARG(blocks <= INT_MAX, "lu batched solve: batch x nrhs too large for one launch");
    hipLaunchKernelGGL(lu_batched_solve_kernel<NP>, dim3((unsigned)blocks), dim3(64), 0, s, lu, batch, n, pitch,
                       stride, piv, b, nrhs, pitch_b, stride_b, width, (int)chunks);
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

extern "C" int64_t mpx_lu_batched_workspace_bytes(int batch, int n) {
    return (batch <= 0 || n <= kSmall) ? 0 : mpx_lu_workspace_bytes(n);
}

extern "C" int mpx_lu_factor_batched_f64(double *a, int batch, int n, int64_t pitch, int64_t stride, int32_t *piv,
                                         int32_t *info, void *workspace, int64_t workspace_bytes, void *stream) {
    MPX_CHECK_ARG(batch >= 0 && n >= 0, "lu batched: batch < 0 or n < 0");
    MPX_CHECK_ARG(pitch >= n, "lu batched: pitch < n");
    if (batch == 0 || n == 0) return MPX_OK;
    MPX_CHECK_ARG(batch == 1 || stride_covers(stride, n, pitch, n), "lu batched: stride < (n - 1) * pitch + n");
    MPX_CHECK_ARG(a && piv && info, "lu batched: null pointer");
    const int64_t need = mpx_lu_batched_workspace_bytes(batch, n);
    MPX_CHECK_ARG(need == 0 || (workspace && workspace_bytes >= need),
                  "lu batched: workspace shorter than mpx_lu_batched_workspace_bytes(batch, n)");
    MPX_CHECK_ARG(need == 0 || aligned16(workspace), "lu batched: workspace not 16-byte aligned");
    hipStream_t s = as_stream(stream);
    if (n <= 8) return launch_factor<8>(a, batch, n, pitch, stride, piv, info, s);
    if (n <= 16) return launch_factor<16>(a, batch, n, pitch, stride, piv, info, s);
    if (n <= 32) return launch_factor<32>(a, batch, n, pitch, stride, piv, info, s);
    if (n <= kSmall) return launch_factor<64>(a, batch, n, pitch, stride, piv, info, s);
    for (int m = 0; m < batch; ++m)  // stream-ordered, so one workspace serves every matrix
        if (int rc = mpx_lu_factor_f64(a + (int64_t)m * stride, n, pitch, piv + (int64_t)m * n, info + m, workspace,
                                       workspace_bytes, stream))
            return rc;
    return MPX_OK;
}

extern "C" int mpx_lu_solve_batched_f64(const double *lu, int batch, int n, int64_t pitch, int64_t stride,
                                        const int32_t *piv, double *b, int nrhs, int64_t pitch_b, int64_t stride_b,
                                        void *stream) {
    MPX_CHECK_ARG(batch >= 0 && n >= 0 && nrhs >= 0, "lu batched solve: batch < 0, n < 0 or nrhs < 0");
    MPX_CHECK_ARG(pitch >= n && pitch_b >= nrhs, "lu batched solve: pitch < n or pitch_b < nrhs");
    if (batch == 0 || n == 0 || nrhs == 0) return MPX_OK;
    MPX_CHECK_ARG(batch == 1 || (stride_covers(stride, n, pitch, n) && stride_covers(stride_b, n, pitch_b, nrhs)),
                  "lu batched solve: stride < (n - 1) * pitch + n or stride_b < (n - 1) * pitch_b + nrhs");
    MPX_CHECK_ARG(lu && piv && b, "lu batched solve: null pointer");
    hipStream_t s = as_stream(stream);
    if (n <= 8) return launch_solve<8>(lu, batch, n, pitch, stride, piv, b, nrhs, pitch_b, stride_b, s);
    if (n <= 16) return launch_solve<16>(lu, batch, n, pitch, stride, piv, b, nrhs, pitch_b, stride_b, s);
    if (n <= 32) return launch_solve<32>(lu, batch, n, pitch, stride, piv, b, nrhs, pitch_b, stride_b, s);
    if (n <= kSmall) return launch_solve<64>(lu, batch, n, pitch, stride, piv, b, nrhs, pitch_b, stride_b, s);
    for (int m = 0; m < batch; ++m)
        if (int rc = mpx_lu_solve_f64(lu + (int64_t)m * stride, n, pitch, piv + (int64_t)m * n,
                                      b + (int64_t)m * stride_b, nrhs, pitch_b, nullptr, 0, stream))
            return rc;
    return MPX_OK;
}
