// Lane helpers shared by the multigrid kernels (multigrid.hip, 2-D;
// multigrid3d.hip, 3-D): a lane owns 16-byte vectors of a row, loads and stores
// them whole where they lie inside the row and element by element at its end,
// and gets the one element it lacks on either side from the neighbouring lane
// through a DPP wave shift.
#pragma once
#include "jacobi_wave.hpp"

#include <initializer_list>

namespace mpx {
namespace {

// elements [j0, j0 + N) of a row of `cols` elements, 0 past its end: one 16-B
// load when the whole vector lies inside the row (VEC: row + j0 is 16-B aligned)
template <typename T, bool VEC, int N>
__device__ __forceinline__ void load_n(const T *row, int j0, int cols, T (&dst)[N]) {
    if constexpr (VEC) {
        static_assert(N == JVec<T>::n, "one 16-byte vector");
        if (j0 + N <= cols) {
            const typename JVec<T>::type q = *reinterpret_cast<const typename JVec<T>::type *>(row + j0);
#pragma unroll
            for (int k = 0; k < N; ++k) dst[k] = lane_of<T>(q, k);
            return;
        }
    }
#pragma unroll
    for (int k = 0; k < N; ++k) dst[k] = (j0 + k < cols) ? row[j0 + k] : (T)0;
}

// stores the elements of [j0, j0 + N) that lie in the columns [lo, hi]; one
// 16-B store when all do
template <typename T, bool VEC, int N>
__device__ __forceinline__ void store_n(T *row, int j0, int lo, int hi, const T (&v)[N]) {
    if constexpr (VEC) {
        if (j0 >= lo && j0 + N - 1 <= hi) {
            if constexpr (JVec<T>::n == 2)
                *reinterpret_cast<double2 *>(row + j0) = make_double2(v[0], v[1]);
            else
                *reinterpret_cast<float4 *>(row + j0) = make_float4(v[0], v[1], v[2], v[3]);
            return;
        }
    }
#pragma unroll
    for (int k = 0; k < N; ++k)
        if (j0 + k >= lo && j0 + k <= hi) row[j0 + k] = v[k];
}

// row[j0 - 1], the last element of the lane to the left (`last` is this
// lane's): a DPP wave shift; lane 0 of a wave loads it. Called by whole waves.
template <typename T>
__device__ __forceinline__ T from_left(T last, const T *row, int j0, int cols) {
    T v = dpp_shift<T>(last, 0x138);
    if ((threadIdx.x & 63) == 0) v = (j0 > 0 && j0 - 1 < cols) ? row[j0 - 1] : (T)0;
    return v;
}

// row[jn], the first element of the lane to the right (`first` is this lane's,
// jn the column after this lane's last); lane 63 of a wave loads it
template <typename T>
__device__ __forceinline__ T from_right(T first, const T *row, int jn, int cols) {
    T v = dpp_shift<T>(first, 0x130);
    if ((threadIdx.x & 63) == 63) v = jn < cols ? row[jn] : (T)0;
    return v;
}

// load_n for M rows at once, row m holding cols[m] elements: one branch for the
// whole group (a lane takes the 16-B loads when every one of its vectors lies
// inside its row), so the M loads are issued back to back and waited for once.
// load_n row by row makes every load wait for the one before it: the two arms
// of its branch write the same registers.
template <typename T, bool VEC, int N, int M>
__device__ __forceinline__ void load_rows(const T *const (&rows)[M], int j0, const int (&cols)[M], T (&dst)[M][N]) {
    if constexpr (VEC) {
        static_assert(N == JVec<T>::n, "one 16-byte vector");
        bool full = true;
#pragma unroll
        for (int m = 0; m < M; ++m) full = full && j0 + N <= cols[m];
        if (full) {
            typename JVec<T>::type q[M];
#pragma unroll
            for (int m = 0; m < M; ++m) q[m] = *reinterpret_cast<const typename JVec<T>::type *>(rows[m] + j0);
#pragma unroll
            for (int m = 0; m < M; ++m)
#pragma unroll
                for (int k = 0; k < N; ++k) dst[m][k] = lane_of<T>(q[m], k);
            return;
        }
    }
#pragma unroll
    for (int m = 0; m < M; ++m)
#pragma unroll
        for (int k = 0; k < N; ++k) dst[m][k] = (j0 + k < cols[m]) ? rows[m][j0 + k] : (T)0;
}

// from_left / from_right in two steps, so that the one load of lanes 0 / 63 can
// be issued with a group of loads and merged after the wave shift:
// left_edge is row[j0 - 1] in lane 0 of a wave (0 in the other lanes and outside
// the row), right_edge row[jn] in lane 63
template <typename T>
__device__ __forceinline__ T left_edge(const T *row, int j0, int cols) {
    return ((threadIdx.x & 63) == 0 && j0 > 0 && j0 - 1 < cols) ? row[j0 - 1] : (T)0;
}

template <typename T>
__device__ __forceinline__ T right_edge(const T *row, int jn, int cols) {
    return ((threadIdx.x & 63) == 63 && jn < cols) ? row[jn] : (T)0;
}

// the element left of this lane's vector: the last element of the lane to the
// left, or lane 0's left_edge. Called by whole waves.
template <typename T>
__device__ __forceinline__ T shift_from_left(T last, T edge) {
    const T v = dpp_shift<T>(last, 0x138);
    return (threadIdx.x & 63) == 0 ? edge : v;
}

template <typename T>
__device__ __forceinline__ T shift_from_right(T first, T edge) {
    const T v = dpp_shift<T>(first, 0x130);
    return (threadIdx.x & 63) == 63 ? edge : v;
}

// the midpoint of the cubic through four equidistant values (weights
// (-1, 9, 9, -1) / 16, the scale factors exact) and the value one step before
// c0 on the cubic through c0..c3 (CUBIC) or the parabola through c0..c2
template <typename T>
__device__ __forceinline__ T cubic_mid(T cm, T c0, T c1, T c2) {
    const T a = c0 + c1;
    const T o = cm + c2;
    const T d = a - o;
    const T t = a + d * (T)0.125;
    return t * (T)0.5;
}

template <typename T>
__device__ __forceinline__ T cubic_ghost(bool cubic, T c0, T c1, T c2, T c3) {
    const T s = c0 + c2;
    const T q = s * (T)4 - c3;
    const T g4 = q - c1 * (T)6;
    const T d = c0 - c1;
    const T g3 = d * (T)3 + c2;
    return cubic ? g4 : g3;
}

// the vector kernels need 16-byte aligned bases and strides that are multiples
// of the 16-byte vector
template <typename T>
bool mg_vec(std::initializer_list<const void *> ptrs, std::initializer_list<int> pitches) {
    for (const void *p : ptrs)
        if (p && !aligned16(p)) return false;
    for (int p : pitches)
        if (p % JVec<T>::n) return false;
    return true;
}

}  // namespace
}  // namespace mpx
