// 3-D Jacobi sweep (7-point stencil) for the distributed stencil tier: plane
// slabs with one halo plane below and above, Dirichlet rows 0 / ny - 1 and
// columns 0 / nx - 1, fused L-infinity residual. The contract (association
// order, copy-through, Chebyshev step) is in capi.h.
//
// MI355X design: HBM-bound, 2 words per point at the floor (3 with b or p, 4
// with both). x reuse is the 2-D kernel's: 62-vector wave strips whose left /
// right neighbours come from the adjacent lanes through DPP. For y and z two
// forms exist (jacobi3d.hpp):
//   * rows:  the 2-D row ring inside a plane, planes k - 1 and k + 1 as two
//            more load streams served by L2 / Infinity Cache;
//   * march: a wave keeps three planes of TY + 2 row vectors in registers and
//            marches KZ planes, so every plane is fetched once per wave.
// j3_tile() below names the form and tile of each production instantiation;
// the measurements behind it are in profiles/jacobi3d.md. Every other
// combination is instantiated only by the tuning entry
// (native/tune/jacobi_variants.hip).
// Widths that are not a multiple of the 16-byte vector, or unaligned pointers,
// take the per-lane kernel.
#include "jacobi3d.hpp"

namespace mpx {
namespace {

// form 0: rows (ty = rows per wave, kz = 1); form 1: march (ty x kz per wave);
// + 2: workgroups remapped so that launch-order neighbours share an XCD.
// Chosen per sweep kind from the 512^3 tables of profiles/jacobi3d.md, the same
// form for both dtypes: the plain sweep marches (z reuse costs no second fetch, and
// the remap keeps the row overlap of neighbouring tiles in one L2); with b or
// the previous iterate as further streams the march form's registers cost it
// occupancy and the rows form is as fast (b alone) or faster. Rows per wave of
// the rows form: 4 beat 8 and 16 in every kind.
struct J3Choice {
    int form, ty, kz;
};
template <typename T, bool RHS, bool ACCEL>
constexpr J3Choice j3_tile() {
    if (RHS || ACCEL) return {0, 4, 1};
    return {3, 4, sizeof(T) == 8 ? 16 : 8};  // KZ: 16 beat 8 in fp64, 8 beat 16 in fp32, in every session
}

template <typename T, bool RHS, bool ACCEL>
int launch_jacobi3d(const T *u, const T *b, T *un, int nx, int ny, int k0, int k1, double omega_d, T *resid,
                    void *stream) {
    T omega;
    if (const int rc = j3_check<T>(u, un, nx, ny, k0, k1, ACCEL, omega_d, &omega)) return rc;
    if (k1 == k0) return MPX_OK;
    hipStream_t s = as_stream(stream);
    if (j3_vector_layout(u, b, un, nx)) {
        constexpr J3Choice tile = j3_tile<T, RHS, ACCEL>();
        const int strips = (nx / JVec<T>::n + kStripVec - 1) / kStripVec;
        // small volumes: smaller tiles, more waves (as launch_jacobi does)
        constexpr bool REMAP = (tile.form & 2) != 0;
        if constexpr ((tile.form & 1) == 0) {
            int R = tile.ty;
            while (R > 1 && j3_waves(strips, ny, R, k1 - k0, 1) < kJ3MinWaves) R >>= 1;
            return launch_j3_rows<T, RHS, ACCEL, REMAP>(u, b, un, nx, ny, k0, k1, R, omega, resid, s);
        } else {
            int KZ = tile.kz;
            while (KZ > 1 && j3_waves(strips, ny, tile.ty, k1 - k0, KZ) < kJ3MinWaves) KZ >>= 1;
            return launch_j3_march<T, tile.ty, RHS, ACCEL, REMAP>(u, b, un, nx, ny, k0, k1, KZ, omega, resid, s);
        }
    }
    const int nxb = (nx + 255) / 256, nyb = (ny + kJ3Rows - 1) / kJ3Rows;
    const int64_t nblk = (int64_t)nxb * nyb * (k1 - k0);
    MPX_CHECK_ARG(nblk <= INT_MAX, "volume too large for one launch");
    hipLaunchKernelGGL((jacobi3d_kernel<T, RHS, ACCEL>), dim3((unsigned)nblk), dim3(256), 0, s, u, b, un, nx, ny, k0, nxb,
                       nyb, omega, resid);
    MPX_RETURN_IF_HIP_ERROR(hipGetLastError());
    return MPX_OK;
}

template <typename T>
int jacobi3d_entry(const T *u, const T *b, T *un, int nx, int ny, int k0, int k1, bool accel, double omega, T *resid,
                   void *stream) {
    if (accel) {
        if (b) return launch_jacobi3d<T, true, true>(u, b, un, nx, ny, k0, k1, omega, resid, stream);
        return launch_jacobi3d<T, false, true>(u, nullptr, un, nx, ny, k0, k1, omega, resid, stream);
    }
    if (b) return launch_jacobi3d<T, true, false>(u, b, un, nx, ny, k0, k1, 1.0, resid, stream);
    return launch_jacobi3d<T, false, false>(u, nullptr, un, nx, ny, k0, k1, 1.0, resid, stream);
}

}  // namespace
MPX_MODULE_ANCHOR(jacobi3d)

}  // namespace mpx

extern "C" int mpx_jacobi3d_f64(const double *u, const double *b, double *un, int nx, int ny, int k0, int k1,
                                double *resid, void *stream) {
    return mpx::jacobi3d_entry<double>(u, b, un, nx, ny, k0, k1, false, 1.0, resid, stream);
}

extern "C" int mpx_jacobi3d_f32(const float *u, const float *b, float *un, int nx, int ny, int k0, int k1, float *resid,
                                void *stream) {
    return mpx::jacobi3d_entry<float>(u, b, un, nx, ny, k0, k1, false, 1.0, resid, stream);
}

extern "C" int mpx_jacobi3d_accel_f64(const double *u, const double *b, double *un, int nx, int ny, int k0, int k1,
                                      double omega, double *resid, void *stream) {
    return mpx::jacobi3d_entry<double>(u, b, un, nx, ny, k0, k1, true, omega, resid, stream);
}

extern "C" int mpx_jacobi3d_accel_f32(const float *u, const float *b, float *un, int nx, int ny, int k0, int k1,
                                      double omega, float *resid, void *stream) {
    return mpx::jacobi3d_entry<float>(u, b, un, nx, ny, k0, k1, true, omega, resid, stream);
}

extern "C" int mpx_jacobi3d_tile(int fp64, int rhs, int accel, int *out) {
    using namespace mpx;
    MPX_CHECK_ARG(out, "null pointer");
    J3Choice c;
    if (fp64)
        c = accel ? (rhs ? j3_tile<double, true, true>() : j3_tile<double, false, true>())
                  : (rhs ? j3_tile<double, true, false>() : j3_tile<double, false, false>());
    else
        c = accel ? (rhs ? j3_tile<float, true, true>() : j3_tile<float, false, true>())
                  : (rhs ? j3_tile<float, true, false>() : j3_tile<float, false, false>());
    out[0] = c.form;
    out[1] = c.ty;
    out[2] = c.kz;
    out[3] = kJ3MinWaves;
    return MPX_OK;
}
