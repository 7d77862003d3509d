/*
 * Host (CPU) implementations of every mpx operator. They define the numerics
 * the HIP kernels are tested against bit for bit:
 *   - luminance without FMA (mpx_luma), Roberts/conv gradient without FMA,
 *     conv taps accumulated with one fmaf per tap in (dy, dx) row-major order;
 *   - lab3 quadratic form with the FMA chain the reference GPU kernel compiles to
 *     (nvcc contracts `temp += d*A`; reference lab3/src/main.cu:57-67).
 * The same file is built twice: serial -O0 (reproduces the reference CPU
 * methodology, README.md:11) and OpenMP -O3 (honest multi-core baseline).
 */
#ifndef MPX_CPU_KERNELS_H
#define MPX_CPU_KERNELS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int mpx_cpu_threads(void);
void mpx_cpu_vsub_f64(const double *a, const double *b, double *c, int64_t n);
void mpx_cpu_vsub_f32(const float *a, const float *b, float *c, int64_t n);
void mpx_cpu_roberts(const uint32_t *in, uint32_t *out, int w, int h);
void mpx_cpu_roberts_rgb(const uint32_t *in, uint32_t *out, int w, int h);
void mpx_cpu_conv(const uint32_t *in, uint32_t *out, int w, int pitch, int oy0, int oy1, int y_lo,
                  int y_hi, int k, int anchor, int mode, const float *wx, const float *wy);
void mpx_cpu_classify(uint32_t *img, int64_t npix, int nc, const double *mu, const double *inv);
double mpx_cpu_jacobi_f64(const double *u, double *un, int cols, int pitch, int r0, int r1);
double mpx_cpu_jacobi_rhs_f64(const double *u, const double *b, double *un, int cols, int pitch, int r0, int r1);
double mpx_cpu_jacobi_accel_f64(const double *u, const double *b, double *un, int cols, int pitch, int r0, int r1,
                                double omega);
double mpx_cpu_jacobi3d_f64(const double *u, const double *b, double *un, int nx, int ny, int k0, int k1);
double mpx_cpu_jacobi3d_accel_f64(const double *u, const double *b, double *un, int nx, int ny, int k0, int k1,
                                  double omega);
/* lab5: ascending sort in place, same order as mpx_sort (dtype: enum mpx_sort_dtype). */
void mpx_cpu_sort(void *data, int64_t n, int dtype);
/* Stable key-value sort, same order and flags as mpx_sort_pairs_ws (capi.h:
 * 1 = MPX_SORT_IOTA, 2 = MPX_SORT_DESCENDING); int32 / float32 keys, n < 2^32. */
void mpx_cpu_sort_pairs(void *keys, uint32_t *vals, int64_t n, int dtype, int flags);
/* lab4: unblocked LU with partial pivoting and the solve with its factors, the
 * contract of mpx_lu_factor_f64 / mpx_lu_solve_f64 (capi.h); bad arguments
 * write nothing but *info = 0. */
void mpx_cpu_lu_factor_f64(double *a, int n, int64_t pitch, int32_t *piv, int32_t *info);
void mpx_cpu_lu_solve_f64(const double *lu, int n, int64_t pitch, const int32_t *piv, double *b, int nrhs,
                          int64_t pitch_b);
/* The same for `batch` matrices (matrix m at a + m * stride, piv (batch, n), one
 * info word each; B's matrices stride_b apart): an OpenMP loop over the matrices
 * that calls the two functions above, so every matrix gets exactly their result. */
void mpx_cpu_lu_factor_batched_f64(double *a, int batch, int n, int64_t pitch, int64_t stride, int32_t *piv,
                                   int32_t *info);
void mpx_cpu_lu_solve_batched_f64(const double *lu, int batch, int n, int64_t pitch, int64_t stride,
                                  const int32_t *piv, double *b, int nrhs, int64_t pitch_b, int64_t stride_b);
/* lab4: unblocked Cholesky A = L L^T in lower storage and the solve with L, the
 * contract of mpx_chol_factor_f64 / mpx_chol_solve_f64 (capi.h); bad arguments
 * write nothing but *info = 0. */
void mpx_cpu_chol_factor_f64(double *a, int n, int64_t pitch, int32_t *info);
void mpx_cpu_chol_solve_f64(const double *l, int n, int64_t pitch, double *b, int nrhs, int64_t pitch_b);
/* The same for `batch` matrices (member m at a + m * stride, one info word each;
 * B's members stride_b apart): an OpenMP loop over the members that calls the
 * two functions above, so every member gets exactly their result. Bad arguments
 * write nothing. */
void mpx_cpu_chol_factor_batched_f64(double *a, int batch, int n, int64_t pitch, int64_t stride, int32_t *info);
void mpx_cpu_chol_solve_batched_f64(const double *l, int batch, int n, int64_t pitch, int64_t stride, double *b,
                                    int nrhs, int64_t pitch_b, int64_t stride_b);
/* lab4: unblocked Householder QR (m >= n, geqrf storage), the application of
 * Q (transpose = 0) or Q^T from the stored reflectors and the solve with R,
 * the contract of mpx_qr_factor_f64 / mpx_qr_apply_f64 / mpx_qr_rsolve_f64
 * (capi.h): rows summed in ascending order, OpenMP over the columns of the
 * update; bad arguments write nothing but *info = 0. */
void mpx_cpu_qr_factor_f64(double *a, int m, int n, int64_t pitch, double *tau, int32_t *info);
void mpx_cpu_qr_apply_f64(const double *qr, int m, int n, int64_t pitch, const double *tau, double *b, int nrhs,
                          int64_t pitch_b, int transpose);
void mpx_cpu_qr_rsolve_f64(const double *qr, int n, int64_t pitch, double *b, int nrhs, int64_t pitch_b);

/* lab1 host text I/O (reference lab1/src/main.cu:46-52 scanf per value,
 * :82-84 printf per value), parallel over OpenMP threads in the -fopenmp builds
 * and serial otherwise; byte-identical to the serial strtod / "%.10e " path.
 * mpx_parse_doubles: the next `count` whitespace-separated numbers of
 * buf[pos, len) (buf NUL-terminated at len) into out[]; returns how many were
 * parsed (< count: missing or malformed token at that index) and sets *end to
 * the offset just past the last parsed token.
 * mpx_format_e10: "%.10e " for each of n values, as one malloc'd buffer of
 * *len bytes (caller frees). */
int64_t mpx_parse_doubles(const char *buf, size_t len, size_t pos, int64_t count, double *out, size_t *end);
char *mpx_format_e10(const double *v, int64_t n, size_t *len);

/* lab3 host statistics H1 (reference lab3/src/main.cu:102-152). Returns 0, or
 * -1 when a coordinate lies outside the image. */
int mpx_cpu_class_stats(const uint32_t *img, int w, int h, int nc, const int *np,
                        const int *coords, double *mu, double *inv);

#ifdef __cplusplus
}
#endif

#endif
