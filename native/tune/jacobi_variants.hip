// Tuning entry point of the Jacobi wave kernel (tools/experiments/jbench.py):
// explicit rows per wave R and the A/B forms of round 2-3 (buffer-store cache
// policy, non-temporal loads, no tail exit, alternating walks, 16-wave
// workgroups). Built into libmpx_tune.so only; production launches are in
// native/src/kernels/jacobi.hip. The 3-D entry (explicit wave form and tile of
// the kernels in jacobi3d.hpp, production launches in jacobi3d.hip) is at the end.
#include "../src/kernels/jacobi_wave.hpp"
#include "../src/kernels/jacobi3d.hpp"

// Tuning entry point (tools/jbench.py): wave kernel with an explicit rows-per-
// wave R and buffer-store cache policy aux (0 default, 2 = nontemporal).
extern "C" int mpx_jacobi_variant(void *u, void *un, int cols, int pitch, int r0, int r1, void *resid, int fp64,
                                  int R, int aux, void *stream) {
    using namespace mpx;
    MPX_CHECK_ARG(u && un && cols >= 1 && pitch >= cols && r0 >= 1 && r1 >= r0 && R >= 1, "bad arguments");
    MPX_CHECK_ARG(aux == 0 || aux == 2 || aux == 6 || aux == 10 || aux == 18 || aux == 22 || aux == 50,
                  "aux must be 0, 2, 6 (2 + non-temporal loads), 10 (2 without the tail exit) or 18 (2 + "
                  "alternating walk directions), 22 (18 + non-temporal interior row loads), 50 (18 with 16-wave "
                  "workgroups)");
    const int NV = fp64 ? 2 : 4;
    MPX_CHECK_ARG(pitch % NV == 0 && cols % NV == 0 && aligned16(u) && aligned16(un), "needs the vector layout");
    const int strips = (cols / NV + kStripVec - 1) / kStripVec;
    const int nwaves = strips * ((r1 - r0 + R - 1) / R);
    const dim3 g((nwaves + 3) / 4), b(256);
    hipStream_t s = as_stream(stream);
#define MPX_JV(T, A)                                                                                          \
    hipLaunchKernelGGL((jacobi_wave_kernel<T, A>), g, b, 0, s, (const T *)u, (T *)un, cols, pitch, r0, r1, strips, \
                       R, nwaves, (T *)resid, mpx_jacobi_peer{}, (const T *)nullptr, (T)0)
#define MPX_JVN(T)                                                                                             \
    hipLaunchKernelGGL((jacobi_wave_kernel<T, 2, 1>), g, b, 0, s, (const T *)u, (T *)un, cols, pitch, r0, r1,    \
                       strips, R, nwaves, (T *)resid, mpx_jacobi_peer{}, (const T *)nullptr, (T)0)
#define MPX_JVA(T)                                                                                             \
    hipLaunchKernelGGL((jacobi_wave_kernel<T, 2, 0, true, false, true>), g, b, 0, s, (const T *)u, (T *)un, cols,  \
                       pitch, r0, r1, strips, R, nwaves, (T *)resid, mpx_jacobi_peer{}, (const T *)nullptr, (T)0)
#define MPX_JVW(T)                                                                                             \
    hipLaunchKernelGGL((jacobi_wave_kernel<T, 2, 0, true, false, true, 16>), dim3((nwaves + 15) / 16), dim3(1024),  \
                       0, s, (const T *)u, (T *)un, cols, pitch, r0, r1, strips, R, nwaves, (T *)resid,               \
                       mpx_jacobi_peer{}, (const T *)nullptr, (T)0)
#define MPX_JVI(T)                                                                                             \
    hipLaunchKernelGGL((jacobi_wave_kernel<T, 2, 2, true, false, true>), g, b, 0, s, (const T *)u, (T *)un, cols,  \
                       pitch, r0, r1, strips, R, nwaves, (T *)resid, mpx_jacobi_peer{}, (const T *)nullptr, (T)0)
#define MPX_JVX(T)                                                                                             \
    hipLaunchKernelGGL((jacobi_wave_kernel<T, 2, 0, false>), g, b, 0, s, (const T *)u, (T *)un, cols, pitch, r0, \
                       r1, strips, R, nwaves, (T *)resid, mpx_jacobi_peer{}, (const T *)nullptr, (T)0)
    if (fp64) {
        if (aux == 22) MPX_JVI(double); else if (aux == 50) MPX_JVW(double); else if (aux == 18) MPX_JVA(double); else if (aux == 10) MPX_JVX(double); else if (aux == 6) MPX_JVN(double); else if (aux) MPX_JV(double, 2); else MPX_JV(double, 0);
    } else {
        if (aux == 22) MPX_JVI(float); else if (aux == 50) MPX_JVW(float); else if (aux == 18) MPX_JVA(float); else if (aux == 10) MPX_JVX(float); else if (aux == 6) MPX_JVN(float); else if (aux) MPX_JV(float, 2); else MPX_JV(float, 0);
    }
#undef MPX_JV
#undef MPX_JVN
#undef MPX_JVX
#undef MPX_JVI
#undef MPX_JVA
#undef MPX_JVW
    MPX_RETURN_IF_HIP_ERROR(hipGetLastError());
    return MPX_OK;
}

// The production template with a source term, <T, 2, 0, true, false, true, 4,
// RHS = true>, at an explicit rows-per-wave R (row-block tests) and with plain
// (nt = 0) or non-temporal (nt = 1) loads of b (the A/B of profiles/jacobi.md).
extern "C" int mpx_jacobi_rhs_variant(void *u, const void *b, void *un, int cols, int pitch, int r0, int r1,
                                      void *resid, int fp64, int R, int nt, void *stream) {
    using namespace mpx;
    MPX_CHECK_ARG(u && b && un && cols >= 1 && pitch >= cols && r0 >= 1 && r1 >= r0 && R >= 1, "bad arguments");
    MPX_CHECK_ARG(nt == 0 || nt == 1, "nt must be 0 (plain loads of b) or 1 (non-temporal)");
    const int NV = fp64 ? 2 : 4;
    MPX_CHECK_ARG(pitch % NV == 0 && cols % NV == 0 && aligned16(u) && aligned16(b) && aligned16(un),
                  "needs the vector layout");
    if (r1 == r0) return MPX_OK;
    const int strips = (cols / NV + kStripVec - 1) / kStripVec;
    const int nwaves = strips * ((r1 - r0 + R - 1) / R);
    const dim3 g((nwaves + 3) / 4), blk(256);
    hipStream_t s = as_stream(stream);
#define MPX_JR(T, NT)                                                                                            \
    hipLaunchKernelGGL((jacobi_wave_kernel<T, 2, 0, true, false, true, 4, true, NT>), g, blk, 0, s, (const T *)u, \
                       (T *)un, cols, pitch, r0, r1, strips, R, nwaves, (T *)resid, mpx_jacobi_peer{}, (const T *)b, (T)0)
    if (fp64) {
        if (nt) MPX_JR(double, true); else MPX_JR(double, false);
    } else {
        if (nt) MPX_JR(float, true); else MPX_JR(float, false);
    }
#undef MPX_JR
    MPX_RETURN_IF_HIP_ERROR(hipGetLastError());
    return MPX_OK;
}

// The production templates of the Chebyshev step, <T, 2, 0, true, false, true,
// 4, RHS, RHS, ACCEL = true> (b null: the Laplace form), at an explicit rows-
// per-wave R (row-block tests). un is in-out.
extern "C" int mpx_jacobi_accel_variant(void *u, const void *b, void *un, int cols, int pitch, int r0, int r1,
                                        double omega, void *resid, int fp64, int R, void *stream) {
    using namespace mpx;
    MPX_CHECK_ARG(u && un && cols >= 1 && pitch >= cols && r0 >= 1 && r1 >= r0 && R >= 1, "bad arguments");
    MPX_CHECK_ARG(omega > 0.0 && omega <= (fp64 ? 1.7976931348623157e308 : 3.402823466e38) &&
                      (fp64 || (float)omega > 0.0f),
                  "omega must be finite and positive");
    const int NV = fp64 ? 2 : 4;
    MPX_CHECK_ARG(pitch % NV == 0 && cols % NV == 0 && aligned16(u) && (!b || aligned16(b)) && aligned16(un),
                  "needs the vector layout");
    if (r1 == r0) return MPX_OK;
    const int strips = (cols / NV + kStripVec - 1) / kStripVec;
    const int nwaves = strips * ((r1 - r0 + R - 1) / R);
    const dim3 g((nwaves + 3) / 4), blk(256);
    hipStream_t s = as_stream(stream);
#define MPX_JA(T, RHS)                                                                                          \
    hipLaunchKernelGGL((jacobi_wave_kernel<T, 2, 0, true, false, true, 4, RHS, RHS && kRhsNT, true>), g, blk, 0, s, \
                       (const T *)u, (T *)un, cols, pitch, r0, r1, strips, R, nwaves, (T *)resid, mpx_jacobi_peer{},  \
                       (const T *)b, (T)omega)
    if (fp64) {
        if (b) MPX_JA(double, true); else MPX_JA(double, false);
    } else {
        if (b) MPX_JA(float, true); else MPX_JA(float, false);
    }
#undef MPX_JA
    MPX_RETURN_IF_HIP_ERROR(hipGetLastError());
    return MPX_OK;
}

// 3-D sweeps (native/src/kernels/jacobi3d.hpp) with an explicit wave form and
// tile, so tests run production tile shapes at tiny sizes and the bench tool
// measures both forms: form 0 = rows (ty rows per wave, kz must be 1), form 1 =
// march (ty in {2, 4, 8} rows x kz planes per wave), forms 2 and 3 = the same
// with the workgroups remapped per XCD. b null: the Laplace form; accel != 0:
// the Chebyshev step with omega, un in-out.
extern "C" int mpx_jacobi3d_variant(int fp64, const void *u, const void *b, void *un, int nx, int ny, int k0, int k1,
                                    int accel, double omega, void *resid, int form, int ty, int kz, void *stream) {
    using namespace mpx;
    MPX_CHECK_ARG(form >= 0 && form <= 3, "form must be 0 (rows), 1 (march), 2 or 3 (the same, XCD-remapped)");
    MPX_CHECK_ARG((form & 1) == 0 ? (ty >= 1 && kz == 1) : ((ty == 2 || ty == 4 || ty == 8) && kz >= 1),
                  "tile: rows takes ty >= 1 and kz == 1, march ty in {2, 4, 8} and kz >= 1");
    hipStream_t s = as_stream(stream);
#define MPX_J3A(T, RHS, ACCEL, REMAP)                                                                                \
    do {                                                                                                             \
        if ((form & 1) == 0)                                                                                         \
            return launch_j3_rows<T, RHS, ACCEL, REMAP>((const T *)u, (const T *)b, (T *)un, nx, ny, k0, k1, ty, w,  \
                                                        (T *)resid, s);                                              \
        if (ty == 2)                                                                                                 \
            return launch_j3_march<T, 2, RHS, ACCEL, REMAP>((const T *)u, (const T *)b, (T *)un, nx, ny, k0, k1, kz, \
                                                            w, (T *)resid, s);                                       \
        if (ty == 4)                                                                                                 \
            return launch_j3_march<T, 4, RHS, ACCEL, REMAP>((const T *)u, (const T *)b, (T *)un, nx, ny, k0, k1, kz, \
                                                            w, (T *)resid, s);                                       \
        return launch_j3_march<T, 8, RHS, ACCEL, REMAP>((const T *)u, (const T *)b, (T *)un, nx, ny, k0, k1, kz, w,  \
                                                        (T *)resid, s);                                              \
    } while (0)
#define MPX_J3(T, RHS, ACCEL)                                                                                        \
    do {                                                                                                             \
        T w;                                                                                                         \
        if (const int rc = j3_check<T>(u, un, nx, ny, k0, k1, ACCEL, omega, &w)) return rc;                          \
        MPX_CHECK_ARG(j3_vector_layout((const T *)u, (const T *)b, (const T *)un, nx), "needs the vector layout");   \
        if (k1 == k0) return MPX_OK;                                                                                 \
        if (form & 2) MPX_J3A(T, RHS, ACCEL, true);                                                                  \
        MPX_J3A(T, RHS, ACCEL, false);                                                                               \
    } while (0)
#define MPX_J3K(T)                                                                                                   \
    do {                                                                                                             \
        if (accel) {                                                                                                 \
            if (b) MPX_J3(T, true, true);                                                                            \
            MPX_J3(T, false, true);                                                                                  \
        }                                                                                                            \
        if (b) MPX_J3(T, true, false);                                                                               \
        MPX_J3(T, false, false);                                                                                     \
    } while (0)
    if (fp64) MPX_J3K(double);
    MPX_J3K(float);
#undef MPX_J3K
#undef MPX_J3
#undef MPX_J3A
}
