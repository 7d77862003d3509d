/*
 * CPU reference operators (see cpu_kernels.h). OpenMP pragmas are inert in the
 * serial -O0 build (no -fopenmp), which reproduces the reference's single-thread
 * methodology; the library build uses -O3 -fopenmp.
 */
#include "cpu_kernels.h"

#include <float.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fastfloat.h"
#include "mpx/common.h"

#ifdef _OPENMP
#include <omp.h>
#endif

/* On x86-64 gcc only emits a hardware FMA for fmaf() inside an "fma" target
 * clone; the default clone calls libm's correctly rounded fmaf. Both give the
 * same bits, the clone is just faster. */
#if defined(__GNUC__) && !defined(__clang__) && defined(__x86_64__) && !defined(MPX_NO_CLONES)
#define MPX_FMA_CLONES __attribute__((target_clones("fma", "default")))
#else
#define MPX_FMA_CLONES
#endif

int mpx_cpu_threads(void) {
#ifdef _OPENMP
    return omp_get_max_threads();
#else
    return 1;
#endif
}

/* ---- lab1 text I/O ---- */
static int is_ws(char c) { return c == ' ' || c == '\n' || c == '\t' || c == '\r' || c == '\f' || c == '\v'; }

int64_t mpx_parse_doubles(const char *buf, size_t len, size_t pos, int64_t count, double *out, size_t *end) {
    *end = pos;
    if (count <= 0) return 0;
    while (pos < len && is_ws(buf[pos])) ++pos;
    int T = 1;
#ifdef _OPENMP
    T = omp_get_max_threads();
    if ((int64_t)(len - pos) < ((int64_t)1 << 16)) T = 1;
#endif
    /* chunk k starts at a token start (or len): cut evenly, then move each cut
     * past the token it lands in and the whitespace after it */
    size_t *start = (size_t *)malloc(sizeof(size_t) * (size_t)(T + 1));
    int64_t *ntok = (int64_t *)calloc((size_t)T + 1, sizeof(int64_t));
    if (!start || !ntok) {
        free(start);
        free(ntok);
        return 0;
    }
    start[0] = pos;
    start[T] = len;
    for (int k = 1; k < T; ++k) {
        size_t c = pos + (len - pos) / (size_t)T * (size_t)k;
        if (c < start[k - 1]) c = start[k - 1];
        if (c > pos && !is_ws(buf[c - 1]))
            while (c < len && !is_ws(buf[c])) ++c;
        while (c < len && is_ws(buf[c])) ++c;
        start[k] = c;
    }
    /* pass 1: tokens per chunk */
#ifdef _OPENMP
#pragma omp parallel for schedule(static, 1) num_threads(T)
#endif
    for (int k = 0; k < T; ++k) {
        int64_t c = 0;
        int in_tok = 0;
        for (size_t i = start[k]; i < start[k + 1]; ++i) {
            const int w = is_ws(buf[i]);
            if (!w && !in_tok) ++c;
            in_tok = !w;
        }
        ntok[k + 1] = c;
    }
    for (int k = 0; k < T; ++k) ntok[k + 1] += ntok[k];
    /* pass 2: strtod each token whose index is < count */
    int64_t bad = count;  /* first malformed token index */
    size_t last_end = pos;
#ifdef _OPENMP
#pragma omp parallel for schedule(static, 1) num_threads(T) reduction(min : bad)
#endif
    for (int k = 0; k < T; ++k) {
        int64_t idx = ntok[k];
        size_t i = start[k];
        while (idx < count && i < start[k + 1]) {
            while (i < start[k + 1] && is_ws(buf[i])) ++i;
            if (i >= start[k + 1]) break;
            const char *fe = NULL;
            size_t j;
            if (mpx_fast_strtod(buf + i, buf + start[k + 1], &out[idx], &fe)) {  /* exact fast path */
                j = (size_t)(fe - buf);
            } else {  /* anything the fast path does not decide: the C library */
                char *e = NULL;
                out[idx] = strtod(buf + i, &e);
                if (e == buf + i) {  /* not a number */
                    if (idx < bad) bad = idx;
                    break;
                }
                j = i;
                while (j < start[k + 1] && !is_ws(buf[j])) ++j;
                if ((size_t)(e - buf) != j) {  /* trailing junk in the token */
                    if (idx < bad) bad = idx;
                    break;
                }
            }
            if (idx == count - 1) last_end = j;
            i = j;
            ++idx;
        }
    }
    const int64_t got = ntok[T] < count ? ntok[T] : count;
    free(start);
    free(ntok);
    const int64_t n = bad < got ? bad : got;
    if (n == count) *end = last_end;
    return n;
}

char *mpx_format_e10(const double *v, int64_t n, size_t *len) {
    int T = 1;
#ifdef _OPENMP
    T = omp_get_max_threads();
    if (n < 4096) T = 1;
#endif
    char **part = (char **)calloc((size_t)T, sizeof(char *));
    size_t *plen = (size_t *)calloc((size_t)T + 1, sizeof(size_t));
    int fail = 0;
    char *outb = NULL;
    size_t total = 0;
    if (!part || !plen) goto out;
    /* pass 1: each thread formats its slice (exact fast path, snprintf when
     * the fast path cannot decide) */
#ifdef _OPENMP
#pragma omp parallel for schedule(static, 1) num_threads(T) reduction(| : fail)
#endif
    for (int k = 0; k < T; ++k) {
        const int64_t a = n * k / T, b = n * (k + 1) / T;
        char *buf = (char *)malloc((size_t)(b - a) * 32 + 1);
        if (!buf) {
            fail |= 1;
            continue;
        }
        size_t o = 0;
        for (int64_t i = a; i < b; ++i) {
            const int l = mpx_fast_e10(v[i], buf + o);
            o += l ? (size_t)l : (size_t)snprintf(buf + o, 32, "%.10e", v[i]);
            buf[o++] = ' ';
        }
        part[k] = buf;
        plen[k + 1] = o;
    }
    for (int k = 0; k < T; ++k) plen[k + 1] += plen[k];
    total = plen[T];
    outb = fail ? NULL : (char *)malloc(total + 1);
    /* pass 2: the slices land at their prefix offsets in parallel */
    if (outb) {
#ifdef _OPENMP
#pragma omp parallel for schedule(static, 1) num_threads(T)
#endif
        for (int k = 0; k < T; ++k) memcpy(outb + plen[k], part[k], plen[k + 1] - plen[k]);
        outb[total] = 0;
    }
out:
    if (part)
        for (int k = 0; k < T; ++k) free(part[k]);
    free(part);
    free(plen);
    *len = outb ? total : 0;
    return outb;
}

void mpx_cpu_vsub_f64(const double *a, const double *b, double *c, int64_t n) {
    int64_t i;
#pragma omp parallel for schedule(static)
    for (i = 0; i < n; ++i) c[i] = a[i] - b[i];
}

void mpx_cpu_vsub_f32(const float *a, const float *b, float *c, int64_t n) {
    int64_t i;
#pragma omp parallel for schedule(static)
    for (i = 0; i < n; ++i) c[i] = a[i] - b[i];
}

/* Roberts cross exactly as the reference CPU program evaluates it, including
 * recomputing luminance four times per pixel (reference lab2/src/main.c:23-59). */
void mpx_cpu_roberts(const uint32_t *in, uint32_t *out, int w, int h) {
    int y;
#pragma omp parallel for schedule(static)
    for (y = 0; y < h; ++y) {
        const int y1 = y + 1 < h ? y + 1 : h - 1;
        for (int x = 0; x < w; ++x) {
            const int x1 = x + 1 < w ? x + 1 : w - 1;
            const uint32_t p00 = in[(int64_t)y * w + x];
            const float y00 = mpx_luma(p00);
            const float y10 = mpx_luma(in[(int64_t)y * w + x1]);
            const float y01 = mpx_luma(in[(int64_t)y1 * w + x]);
            const float y11 = mpx_luma(in[(int64_t)y1 * w + x1]);
            const float gx = y11 - y00;
            const float gy = y10 - y01;
            const float g2 = gx * gx + gy * gy;
            const float g = sqrtf(g2);
            out[(int64_t)y * w + x] = mpx_px_gray(mpx_sat_u8(g), mpx_px_a(p00));
        }
    }
}

/* Per-channel Roberts cross, L1 magnitude: every colour channel c of
 * pixel (x, y) becomes min(255, |c(x,y) - c(x+1,y+1)| + |c(x+1,y) - c(x,y+1)|)
 * with clamp-to-edge neighbours, alpha kept. The operator behind the
 * reference's lab2/test_data/lenna_out.data (byte-exact on all 512 x 512
 * pixels; no reference program computes it). Integer arithmetic. */
void mpx_cpu_roberts_rgb(const uint32_t *in, uint32_t *out, int w, int h) {
    int y;
#pragma omp parallel for schedule(static)
    for (y = 0; y < h; ++y) {
        const int y1 = y + 1 < h ? y + 1 : h - 1;
        for (int x = 0; x < w; ++x) {
            const int x1 = x + 1 < w ? x + 1 : w - 1;
            const uint32_t a = in[(int64_t)y * w + x], b = in[(int64_t)y * w + x1];
            const uint32_t c = in[(int64_t)y1 * w + x], d = in[(int64_t)y1 * w + x1];
            uint32_t o = a & 0xff000000u;
            for (int ch = 0; ch < 24; ch += 8) {
                const int va = (int)((a >> ch) & 255u), vb = (int)((b >> ch) & 255u);
                const int vc = (int)((c >> ch) & 255u), vd = (int)((d >> ch) & 255u);
                int g = abs(va - vd) + abs(vb - vc);
                g = g > 255 ? 255 : g;
                o |= (uint32_t)g << ch;
            }
            out[(int64_t)y * w + x] = o;
        }
    }
}

static inline float conv_finish(int mode, float gx, float gy) {
    if (mode == MPX_CONV_MAG2) {
        const float a = gx * gx;
        const float b = gy * gy;
        return sqrtf(a + b);
    }
    if (mode == MPX_CONV_ABS1) return fabsf(gx);
    return gx;
}

MPX_FMA_CLONES
static void conv_rows(const float *lum, int lum_y0, const uint32_t *in, uint32_t *out, int w,
                      int pitch, int oy0, int oy1, int y_lo, int y_hi, int k, int anchor, int mode,
                      const float *wx, const float *wy) {
    int y;
#pragma omp parallel for schedule(static)
    for (y = oy0; y < oy1; ++y) {
        for (int x = 0; x < w; ++x) {
            float ax = 0.0f, ay = 0.0f;
            for (int dy = 0; dy < k; ++dy) {
                const int yy = mpx_clampi(y + dy - anchor, y_lo, y_hi);
                const float *row = lum + (int64_t)(yy - lum_y0) * w;
                for (int dx = 0; dx < k; ++dx) {
                    const int xx = mpx_clampi(x + dx - anchor, 0, w - 1);
                    ax = fmaf(wx[dy * k + dx], row[xx], ax);
                    if (mode == MPX_CONV_MAG2) ay = fmaf(wy[dy * k + dx], row[xx], ay);
                }
            }
            const float g = conv_finish(mode, ax, ay);
            out[(int64_t)y * pitch + x] = mpx_px_gray(mpx_sat_u8(g), mpx_px_a(in[(int64_t)y * pitch + x]));
        }
    }
}

/* Separable form (MPX_CONV_SEP, common.h): per input row the horizontal
 * factor sums, then per output the vertical sum of those, then the scale.
 * Every sum is a sequential fmaf chain from 0 in index order. */
MPX_FMA_CLONES
static void conv_rows_sep(const float *lum, int lum_y0, int nrows, const uint32_t *in, uint32_t *out,
                          int w, int pitch, int oy0, int oy1, int y_lo, int y_hi, int k, int anchor,
                          int mode, const float *wx, const float *wy) {
    const int two = mode == MPX_CONV_MAG2;
    /* horizontal pass: hs[0] (gx factor) and hs[1] (gy factor) of every row */
    float *hs = (float *)malloc(sizeof(float) * (size_t)nrows * (size_t)w * (two ? 2 : 1));
    if (!hs) return;
    float *hsy = two ? hs + (size_t)nrows * (size_t)w : 0;
    int r;
#pragma omp parallel for schedule(static)
    for (r = 0; r < nrows; ++r) {
        const float *row = lum + (int64_t)r * w;
        for (int x = 0; x < w; ++x) {
            float ax = 0.0f, ay = 0.0f;
            for (int dx = 0; dx < k; ++dx) {
                const float l = row[mpx_clampi(x + dx - anchor, 0, w - 1)];
                ax = fmaf(wx[dx], l, ax);
                if (two) ay = fmaf(wy[dx], l, ay);
            }
            hs[(int64_t)r * w + x] = ax;
            if (two) hsy[(int64_t)r * w + x] = ay;
        }
    }
    int y;
#pragma omp parallel for schedule(static)
    for (y = oy0; y < oy1; ++y) {
        for (int x = 0; x < w; ++x) {
            float ax = 0.0f, ay = 0.0f;
            for (int dy = 0; dy < k; ++dy) {
                const int64_t rr = (int64_t)(mpx_clampi(y + dy - anchor, y_lo, y_hi) - lum_y0) * w + x;
                ax = fmaf(wx[k + dy], hs[rr], ax);
                if (two) ay = fmaf(wy[k + dy], hsy[rr], ay);
            }
            const float gx = ax * wx[2 * k];
            const float gy = two ? ay * wy[2 * k] : 0.0f;
            const float g = conv_finish(mode, gx, gy);
            out[(int64_t)y * pitch + x] = mpx_px_gray(mpx_sat_u8(g), mpx_px_a(in[(int64_t)y * pitch + x]));
        }
    }
    free(hs);
}

void mpx_cpu_conv(const uint32_t *in, uint32_t *out, int w, int pitch, int oy0, int oy1, int y_lo,
                  int y_hi, int k, int anchor, int mode, const float *wx, const float *wy) {
    if (oy1 <= oy0 || w <= 0) return;
    /* luminance plane for every input row the requested outputs touch */
    const int r0 = mpx_clampi(oy0 - anchor, y_lo, y_hi);
    const int r1 = mpx_clampi(oy1 - 1 + (k - 1 - anchor), y_lo, y_hi);
    const int nrows = r1 - r0 + 1;
    float *lum = (float *)malloc(sizeof(float) * (size_t)nrows * (size_t)w);
    if (!lum) return;
    int r;
#pragma omp parallel for schedule(static)
    for (r = 0; r < nrows; ++r) {
        const uint32_t *src = in + (int64_t)(r0 + r) * pitch;
        float *dst = lum + (int64_t)r * w;
        for (int x = 0; x < w; ++x) dst[x] = mpx_luma(src[x]);
    }
    if (mode & MPX_CONV_SEP)
        conv_rows_sep(lum, r0, nrows, in, out, w, pitch, oy0, oy1, y_lo, y_hi, k, anchor, MPX_CONV_BASE(mode), wx, wy);
    else
        conv_rows(lum, r0, in, out, w, pitch, oy0, oy1, y_lo, y_hi, k, anchor, mode, wx, wy);
    free(lum);
}

/* lab3 per-pixel quadratic form, FMA chain of the reference GPU kernel
 * (reference lab3/src/main.cu:49-72): strict '<' keeps the lowest class on
 * ties, an all-NaN pixel keeps class -1 which is stored as 255. */
MPX_FMA_CLONES
void mpx_cpu_classify(uint32_t *img, int64_t npix, int nc, const double *mu, const double *inv) {
    int64_t i;
#pragma omp parallel for schedule(static)
    for (i = 0; i < npix; ++i) {
        const uint32_t p = img[i];
        const double pr = (double)mpx_px_r(p), pg = (double)mpx_px_g(p), pb = (double)mpx_px_b(p);
        double best = DBL_MAX;
        int cls = -1;
        for (int c = 0; c < nc; ++c) {
            const double d0 = pr - mu[3 * c + 0];
            const double d1 = pg - mu[3 * c + 1];
            const double d2 = pb - mu[3 * c + 2];
            const double *A = inv + 9 * c;
            double t0 = fma(d0, A[0], 0.0), t1 = fma(d0, A[1], 0.0), t2 = fma(d0, A[2], 0.0);
            t0 = fma(d1, A[3], t0);
            t1 = fma(d1, A[4], t1);
            t2 = fma(d1, A[5], t2);
            t0 = fma(d2, A[6], t0);
            t1 = fma(d2, A[7], t1);
            t2 = fma(d2, A[8], t2);
            double dist = fma(t0, d0, 0.0);
            dist = fma(t1, d1, dist);
            dist = fma(t2, d2, dist);
            if (dist < best) {
                best = dist;
                cls = c;
            }
        }
        img[i] = (p & 0x00ffffffu) | ((uint32_t)(uint8_t)cls << 24);
    }
}

double mpx_cpu_jacobi_f64(const double *u, double *un, int cols, int pitch, int r0, int r1) {
    double res = 0.0;
    int i;
#pragma omp parallel for schedule(static) reduction(max : res)
    for (i = r0; i < r1; ++i) {
        const double *up = u + (int64_t)(i - 1) * pitch;
        const double *uc = u + (int64_t)i * pitch;
        const double *ud = u + (int64_t)(i + 1) * pitch;
        double *o = un + (int64_t)i * pitch;
        o[0] = uc[0];
        o[cols - 1] = uc[cols - 1];
        for (int j = 1; j < cols - 1; ++j) {
            const double s = ((up[j] + ud[j]) + (uc[j - 1] + uc[j + 1])) * 0.25;
            const double d = fabs(s - uc[j]);
            res = d > res ? d : res;
            o[j] = s;
        }
    }
    return res;
}

/* Poisson sweep: the source term b (u's layout, scaled by h^2) joins after the
 * four neighbours, in the GPU kernels' association. */
double mpx_cpu_jacobi_rhs_f64(const double *u, const double *b, double *un, int cols, int pitch, int r0, int r1) {
    double res = 0.0;
    int i;
    if (!b) return NAN;
#pragma omp parallel for schedule(static) reduction(max : res)
    for (i = r0; i < r1; ++i) {
        const double *up = u + (int64_t)(i - 1) * pitch;
        const double *uc = u + (int64_t)i * pitch;
        const double *ud = u + (int64_t)(i + 1) * pitch;
        const double *bc = b + (int64_t)i * pitch;
        double *o = un + (int64_t)i * pitch;
        o[0] = uc[0];
        o[cols - 1] = uc[cols - 1];
        for (int j = 1; j < cols - 1; ++j) {
            const double s = (((up[j] + ud[j]) + (uc[j - 1] + uc[j + 1])) + bc[j]) * 0.25;
            const double d = fabs(s - uc[j]);
            res = d > res ? d : res;
            o[j] = s;
        }
    }
    return res;
}

/* Chebyshev step: un = un + omega * (s - un) with s the plain (b == NULL) or
 * Poisson value above; a subtract, a multiply and an add, each rounded
 * (-ffp-contract=off), as in the GPU kernels. un is in-out; the residual stays
 * max|s - u|. NaN, with nothing written, on a null u / un, bad geometry or an
 * omega that is not finite and positive. */
double mpx_cpu_jacobi_accel_f64(const double *u, const double *b, double *un, int cols, int pitch, int r0, int r1,
                                double omega) {
    double res = 0.0;
    int i;
    if (!u || !un || cols < 1 || pitch < cols || r0 < 1 || r1 < r0 || !(omega > 0.0) || !isfinite(omega)) return NAN;
#pragma omp parallel for schedule(static) reduction(max : res)
    for (i = r0; i < r1; ++i) {
        const double *up = u + (int64_t)(i - 1) * pitch;
        const double *uc = u + (int64_t)i * pitch;
        const double *ud = u + (int64_t)(i + 1) * pitch;
        const double *bc = b ? b + (int64_t)i * pitch : NULL;
        double *o = un + (int64_t)i * pitch;
        o[0] = uc[0];
        o[cols - 1] = uc[cols - 1];
        for (int j = 1; j < cols - 1; ++j) {
            const double n4 = (up[j] + ud[j]) + (uc[j - 1] + uc[j + 1]);
            const double s = bc ? (n4 + bc[j]) * 0.25 : n4 * 0.25;
            const double d = fabs(s - uc[j]);
            res = d > res ? d : res;
            const double p = o[j];
            const double t = omega * (s - p);
            o[j] = p + t;
        }
    }
    return res;
}

/* Damped Jacobi sweep (the multigrid smoother): un = c + omega * (s - c) with c
 * the centre value of u and s the plain (b == NULL) or Poisson value; a
 * subtract, a multiply and an add, each rounded. un is output only; the
 * residual is max|s - c|. NaN, with nothing written, on a null u / un, bad
 * geometry or an omega that is not finite and positive. */
double mpx_cpu_jacobi_relax_f64(const double *u, const double *b, double *un, int cols, int pitch, int r0, int r1,
                                double omega) {
    double res = 0.0;
    int i;
    if (!u || !un || cols < 1 || pitch < cols || r0 < 1 || r1 < r0 || !(omega > 0.0) || !isfinite(omega)) return NAN;
#pragma omp parallel for schedule(static) reduction(max : res)
    for (i = r0; i < r1; ++i) {
        const double *up = u + (int64_t)(i - 1) * pitch;
        const double *uc = u + (int64_t)i * pitch;
        const double *ud = u + (int64_t)(i + 1) * pitch;
        const double *bc = b ? b + (int64_t)i * pitch : NULL;
        double *o = un + (int64_t)i * pitch;
        o[0] = uc[0];
        o[cols - 1] = uc[cols - 1];
        for (int j = 1; j < cols - 1; ++j) {
            const double n4 = (up[j] + ud[j]) + (uc[j - 1] + uc[j + 1]);
            const double s = bc ? (n4 + bc[j]) * 0.25 : n4 * 0.25;
            const double c = uc[j];
            const double d = fabs(s - c);
            res = d > res ? d : res;
            const double t = omega * (s - c);
            o[j] = c + t;
        }
    }
    return res;
}

/* Multigrid operators on an (H, W) grid with Dirichlet rows 0 / H-1 and columns
 * 0 / W-1 and its coarse grid (hc, wc), H = 2 hc - 1, W = 2 wc - 1 (capi.h);
 * every operation rounded (-ffp-contract=off), in the GPU kernels' order. */
double mpx_cpu_mg_residual_f64(const double *u, const double *b, double *r, int rows, int cols, int pitch_u,
                               int pitch_b, int pitch_r) {
    double res = 0.0;
    int i;
    if (!u || !r || rows < 3 || cols < 3 || pitch_u < cols || pitch_r < cols || (b && pitch_b < cols)) return NAN;
#pragma omp parallel for schedule(static) reduction(max : res)
    for (i = 1; i < rows - 1; ++i) {
        const double *up = u + (int64_t)(i - 1) * pitch_u;
        const double *uc = u + (int64_t)i * pitch_u;
        const double *ud = u + (int64_t)(i + 1) * pitch_u;
        const double *bc = b ? b + (int64_t)i * pitch_b : NULL;
        double *o = r + (int64_t)i * pitch_r;
        for (int j = 1; j < cols - 1; ++j) {
            double n = (up[j] + ud[j]) + (uc[j - 1] + uc[j + 1]);
            if (bc) n = n + bc[j];
            const double c4 = 4.0 * uc[j];
            const double v = n - c4;
            const double a = fabs(v);
            res = a > res ? a : res;
            o[j] = v;
        }
    }
    return res;
}

int mpx_cpu_mg_restrict_f64(const double *r, double *bc, int hc, int wc, int pitch_r, int pitch_bc) {
    int I;
    if (!r || !bc || hc < 2 || wc < 2 || hc >= (1 << 29) || wc >= (1 << 29) || pitch_r < 2 * wc - 1 || pitch_bc < wc)
        return -1;
#pragma omp parallel for schedule(static)
    for (I = 1; I < hc - 1; ++I) {
        const double *t = r + (int64_t)(2 * I - 1) * pitch_r;
        const double *m = r + (int64_t)(2 * I) * pitch_r;
        const double *d = r + (int64_t)(2 * I + 1) * pitch_r;
        double *o = bc + (int64_t)I * pitch_bc;
        for (int J = 1; J < wc - 1; ++J) {
            const int j = 2 * J;
            const double e = (t[j] + d[j]) + (m[j - 1] + m[j + 1]);
            const double x = (t[j - 1] + t[j + 1]) + (d[j - 1] + d[j + 1]);
            const double eh = e * 0.5;
            const double xq = x * 0.25;
            o[J] = (m[j] + eh) + xq;
        }
    }
    return 0;
}

int mpx_cpu_mg_prolong_add_f64(const double *e, double *u, int hc, int wc, int pitch_e, int pitch_u) {
    int i;
    if (!e || !u || hc < 2 || wc < 2 || hc >= (1 << 29) || wc >= (1 << 29) || pitch_e < wc || pitch_u < 2 * wc - 1)
        return -1;
    const int h = 2 * hc - 1, w = 2 * wc - 1;
#pragma omp parallel for schedule(static)
    for (i = 1; i < h - 1; ++i) {
        const double *c0 = e + (int64_t)(i / 2) * pitch_e;
        const double *c1 = c0 + pitch_e; /* read on odd rows only: i / 2 + 1 <= hc - 1 there */
        double *o = u + (int64_t)i * pitch_u;
        for (int j = 1; j < w - 1; ++j) {
            const int J = j / 2;
            double v;
            if (!(i & 1)) {
                v = (j & 1) ? (c0[J] + c0[J + 1]) * 0.5 : c0[J];
            } else if (!(j & 1)) {
                v = (c0[J] + c1[J]) * 0.5;
            } else {
                v = ((c0[J] + c1[J]) + (c0[J + 1] + c1[J + 1])) * 0.25;
            }
            o[j] = o[j] + v;
        }
    }
    return 0;
}

/* prolong_cubic (capi.h): the midpoint of four values, the ghost before c0, and
 * element j of a row of n values interpolated to 2n - 1 */
static inline double cubic_mid(double cm, double c0, double c1, double c2) {
    const double a = c0 + c1;
    const double o = cm + c2;
    const double d = a - o;
    const double t = a + d * 0.125;
    return t * 0.5;
}

static inline double cubic_ghost(int n, double c0, double c1, double c2, double c3) {
    if (n >= 4) {
        const double s = c0 + c2;
        const double q = s * 4.0 - c3;
        return q - c1 * 6.0;
    }
    const double d = c0 - c1;
    return d * 3.0 + c2;
}

static inline double cubic_row(const double *c, int n, int j) {
    const int K = j / 2;
    if (!(j & 1)) return c[K];
    const double cm = K >= 1 ? c[K - 1] : cubic_ghost(n, c[0], c[1], c[2], c[n >= 4 ? 3 : 2]);
    const double cp = K + 2 < n ? c[K + 2] : cubic_ghost(n, c[n - 1], c[n - 2], c[n - 3], c[n >= 4 ? n - 4 : 0]);
    return cubic_mid(cm, c[K], c[K + 1], cp);
}

/* element (i, j) of the 2-D rule applied to an hc x wc grid: cubic_row along the
 * coarse rows, then the 1-D rule down column j of the interpolated rows, the
 * ghost rows from the first / last four of them */
static inline double cubic_plane(const double *c, int hc, int wc, int pitch_c, int i, int j) {
    const int K = i / 2;
    if (!(i & 1)) return cubic_row(c + (int64_t)K * pitch_c, wc, j);
    double v[4];
    for (int q = 0; q < 4; ++q) {
        const int I = K - 1 + q;
        if (I >= 0 && I < hc) {
            v[q] = cubic_row(c + (int64_t)I * pitch_c, wc, j);
        } else {
            double g[4];
            for (int t = 0; t < 4; ++t) {
                const int R = t < 3 || hc >= 4 ? t : 0; /* hc == 3: the fourth is not used */
                g[t] = cubic_row(c + (int64_t)(I < 0 ? R : hc - 1 - R) * pitch_c, wc, j);
            }
            v[q] = cubic_ghost(hc, g[0], g[1], g[2], g[3]);
        }
    }
    return cubic_mid(v[0], v[1], v[2], v[3]);
}

int mpx_cpu_mg_prolong_cubic_f64(const double *c, double *u, int hc, int wc, int pitch_c, int pitch_u) {
    int i;
    if (!c || !u || hc < 3 || wc < 3 || hc >= (1 << 29) || wc >= (1 << 29) || pitch_c < wc || pitch_u < 2 * wc - 1)
        return -1;
    const int h = 2 * hc - 1, w = 2 * wc - 1;
#pragma omp parallel for schedule(static)
    for (i = 1; i < h - 1; ++i) {
        double *o = u + (int64_t)i * pitch_u;
        for (int j = 1; j < w - 1; ++j) o[j] = cubic_plane(c, hc, wc, pitch_c, i, j);
    }
    return 0;
}

/* 3-D sweep over planes [k0, k1) of a (planes + 2, ny, nx) buffer, x fastest:
 * s = ((((zm + zp) + (ym + yp)) + (xm + xp)) [+ b]) * (1/6), every operation
 * rounded (-ffp-contract=off), in the GPU kernels' association. Boundary rows
 * and columns of a swept plane are copied through. omega == NULL: un = s;
 * otherwise the Chebyshev step un = un + omega * (s - un), un in-out. */
static double jacobi3d_planes(const double *u, const double *b, double *un, int nx, int ny, int k0, int k1,
                              const double *omega) {
    const int64_t plane = (int64_t)ny * nx;
    const double c = 1.0 / 6.0;
    double res = 0.0;
    int k;
#pragma omp parallel for schedule(static) reduction(max : res)
    for (k = k0; k < k1; ++k) {
        const double *uc = u + (int64_t)k * plane;
        const double *bc = b ? b + (int64_t)k * plane : NULL;
        double *o = un + (int64_t)k * plane;
        for (int y = 0; y < ny; ++y) {
            const int64_t r = (int64_t)y * nx;
            if (y == 0 || y == ny - 1) {
                for (int x = 0; x < nx; ++x) o[r + x] = uc[r + x];
                continue;
            }
            o[r] = uc[r];
            o[r + nx - 1] = uc[r + nx - 1];
            for (int x = 1; x < nx - 1; ++x) {
                const int64_t i = r + x;
                const double n6 = ((uc[i - plane] + uc[i + plane]) + (uc[i - nx] + uc[i + nx])) + (uc[i - 1] + uc[i + 1]);
                const double s = bc ? (n6 + bc[i]) * c : n6 * c;
                const double d = fabs(s - uc[i]);
                res = d > res ? d : res;
                if (omega) {
                    const double p = o[i];
                    const double t = *omega * (s - p);
                    o[i] = p + t;
                } else {
                    o[i] = s;
                }
            }
        }
    }
    return res;
}

static int jacobi3d_geometry_ok(const void *u, const void *un, int nx, int ny, int k0, int k1) {
    return u && un && nx >= 3 && ny >= 3 && (int64_t)ny * nx < ((int64_t)1 << 31) && k0 >= 1 && k1 >= k0;
}

double mpx_cpu_jacobi3d_f64(const double *u, const double *b, double *un, int nx, int ny, int k0, int k1) {
    if (!jacobi3d_geometry_ok(u, un, nx, ny, k0, k1)) return NAN;
    return jacobi3d_planes(u, b, un, nx, ny, k0, k1, NULL);
}

double mpx_cpu_jacobi3d_accel_f64(const double *u, const double *b, double *un, int nx, int ny, int k0, int k1,
                                  double omega) {
    if (!jacobi3d_geometry_ok(u, un, nx, ny, k0, k1) || !(omega > 0.0) || !isfinite(omega)) return NAN;
    return jacobi3d_planes(u, b, un, nx, ny, k0, k1, &omega);
}

/* 3-D multigrid operators on a pitched (D, H, W) grid (row pitch and 64-bit
 * plane stride in elements) with Dirichlet values on all six faces, and its
 * coarse grid (dc, hc, wc), D = 2 dc - 1, H = 2 hc - 1, W = 2 wc - 1 (capi.h);
 * every operation rounded (-ffp-contract=off), in the GPU kernels' order. */
static int mg3_strides_ok(int h, int w, int pitch, int64_t plane) {
    return pitch >= w && plane >= (int64_t)h * pitch;
}

static int mg3_coarse_ok(int dc, int hc, int wc) {
    return dc >= 2 && hc >= 2 && wc >= 2 && dc < (1 << 29) && hc < (1 << 29) && wc < (1 << 29);
}

/* n = ((zm + zp) + (ym + yp)) + (xm + xp) around row pointer c, column x */
static inline double mg3_neighbours(const double *c, int x, int pitch, int64_t plane) {
    return ((c[x - plane] + c[x + plane]) + (c[x - pitch] + c[x + pitch])) + (c[x - 1] + c[x + 1]);
}

/* Damped 3-D sweep over planes [k0, k1): un = c + omega * (s - c) at the
 * interior points, boundary rows and columns of a swept plane copied through,
 * un output only; returns max|s - c|. u, b and un share pitch and plane stride. */
double mpx_cpu_jacobi3d_relax_f64(const double *u, const double *b, double *un, int d, int ny, int nx, int pitch,
                                  int64_t plane, int k0, int k1, double omega) {
    const double sixth = 1.0 / 6.0;
    double res = 0.0;
    int k;
    if (!u || !un || nx < 3 || ny < 3 || d < 3 || k0 < 1 || k1 < k0 || k1 > d - 1 || !mg3_strides_ok(ny, nx, pitch, plane) ||
        !(omega > 0.0) || !isfinite(omega))
        return NAN;
#pragma omp parallel for schedule(static) reduction(max : res)
    for (k = k0; k < k1; ++k) {
        for (int y = 0; y < ny; ++y) {
            const int64_t off = (int64_t)k * plane + (int64_t)y * pitch;
            const double *c = u + off;
            double *o = un + off;
            if (y == 0 || y == ny - 1) {
                for (int x = 0; x < nx; ++x) o[x] = c[x];
                continue;
            }
            o[0] = c[0];
            o[nx - 1] = c[nx - 1];
            for (int x = 1; x < nx - 1; ++x) {
                const double n = mg3_neighbours(c, x, pitch, plane);
                const double s = b ? (n + b[off + x]) * sixth : n * sixth;
                const double df = s - c[x];
                const double a = fabs(df);
                res = a > res ? a : res;
                const double t = omega * df;
                o[x] = c[x] + t;
            }
        }
    }
    return res;
}

double mpx_cpu_mg3_residual_f64(const double *u, const double *b, double *r, int d, int ny, int nx, int pitch_u,
                                int64_t plane_u, int pitch_b, int64_t plane_b, int pitch_r, int64_t plane_r) {
    double res = 0.0;
    int k;
    if (!u || !r || nx < 3 || ny < 3 || d < 3 || !mg3_strides_ok(ny, nx, pitch_u, plane_u) ||
        !mg3_strides_ok(ny, nx, pitch_r, plane_r) || (b && !mg3_strides_ok(ny, nx, pitch_b, plane_b)))
        return NAN;
#pragma omp parallel for schedule(static) reduction(max : res)
    for (k = 1; k < d - 1; ++k) {
        for (int y = 1; y < ny - 1; ++y) {
            const double *c = u + (int64_t)k * plane_u + (int64_t)y * pitch_u;
            const double *bb = b ? b + (int64_t)k * plane_b + (int64_t)y * pitch_b : NULL;
            double *o = r + (int64_t)k * plane_r + (int64_t)y * pitch_r;
            for (int x = 1; x < nx - 1; ++x) {
                double n = mg3_neighbours(c, x, pitch_u, plane_u);
                if (bb) n = n + bb[x];
                const double c6 = 6.0 * c[x];
                const double v = n - c6;
                const double a = fabs(v);
                res = a > res ? a : res;
                o[x] = v;
            }
        }
    }
    return res;
}

/* P_k[J][I]: the 2-D full weighting of fine plane k (pointer to its row 2J) */
static inline double mg3_plane_weight(const double *m, int j, int pitch) {
    const double *t = m - pitch, *dn = m + pitch;
    const double e = (t[j] + dn[j]) + (m[j - 1] + m[j + 1]);
    const double x = (t[j - 1] + t[j + 1]) + (dn[j - 1] + dn[j + 1]);
    const double eh = e * 0.5;
    const double xq = x * 0.25;
    return (m[j] + eh) + xq;
}

int mpx_cpu_mg3_restrict_f64(const double *r, double *bc, int dc, int hc, int wc, int pitch_r, int64_t plane_r,
                             int pitch_bc, int64_t plane_bc) {
    int K;
    if (!r || !bc || !mg3_coarse_ok(dc, hc, wc) || !mg3_strides_ok(2 * hc - 1, 2 * wc - 1, pitch_r, plane_r) ||
        !mg3_strides_ok(hc, wc, pitch_bc, plane_bc))
        return -1;
    if (dc < 3 || hc < 3 || wc < 3) return 0; /* no coarse interior */
#pragma omp parallel for schedule(static)
    for (K = 1; K < dc - 1; ++K) {
        for (int J = 1; J < hc - 1; ++J) {
            const double *m = r + (int64_t)(2 * K) * plane_r + (int64_t)(2 * J) * pitch_r;
            double *o = bc + (int64_t)K * plane_bc + (int64_t)J * pitch_bc;
            for (int I = 1; I < wc - 1; ++I) {
                const double lo = mg3_plane_weight(m - plane_r, 2 * I, pitch_r);
                const double mid = mg3_plane_weight(m, 2 * I, pitch_r);
                const double hi = mg3_plane_weight(m + plane_r, 2 * I, pitch_r);
                const double z = lo + hi;
                const double zh = z * 0.5;
                const double v = mid + zh;
                o[I] = v * 0.5;
            }
        }
    }
    return 0;
}

int mpx_cpu_mg3_prolong_add_f64(const double *e, double *u, int dc, int hc, int wc, int pitch_e, int64_t plane_e,
                                int pitch_u, int64_t plane_u) {
    int k;
    if (!e || !u || !mg3_coarse_ok(dc, hc, wc) || !mg3_strides_ok(hc, wc, pitch_e, plane_e) ||
        !mg3_strides_ok(2 * hc - 1, 2 * wc - 1, pitch_u, plane_u))
        return -1;
    const int d = 2 * dc - 1, h = 2 * hc - 1, w = 2 * wc - 1;
    static const double scale[4] = {1.0, 0.5, 0.25, 0.125};
#pragma omp parallel for schedule(static)
    for (k = 1; k < d - 1; ++k) {
        const int64_t dz = (k & 1) ? plane_e : 0; /* the +1 neighbours are read on odd coordinates only */
        for (int i = 1; i < h - 1; ++i) {
            const int64_t dy = (i & 1) ? pitch_e : 0;
            const double *c = e + (int64_t)(k / 2) * plane_e + (int64_t)(i / 2) * pitch_e;
            double *o = u + (int64_t)k * plane_u + (int64_t)i * pitch_u;
            for (int j = 1; j < w - 1; ++j) {
                const int I = j / 2;
                const int odd = (k & 1) + (i & 1) + (j & 1);
                /* z pair sums at the (up to) four coarse (row, column) corners, then y, then x */
                double z00 = c[I], z10 = c[I + dy], y0, y1 = 0.0, x;
                if (k & 1) {
                    z00 = z00 + c[I + dz];
                    z10 = z10 + c[I + dy + dz];
                }
                y0 = (i & 1) ? z00 + z10 : z00;
                if (j & 1) {
                    double z01 = c[I + 1], z11 = c[I + 1 + dy];
                    if (k & 1) {
                        z01 = z01 + c[I + 1 + dz];
                        z11 = z11 + c[I + 1 + dy + dz];
                    }
                    y1 = (i & 1) ? z01 + z11 : z01;
                    x = y0 + y1;
                } else {
                    x = y0;
                }
                o[j] = odd ? o[j] + x * scale[odd] : o[j] + x;
            }
        }
    }
    return 0;
}

/* mg3_prolong_cubic (capi.h): cubic_plane in every coarse plane, then the 1-D
 * rule down z through the interpolated planes, the ghost planes element by
 * element from the first / last four of them */
int mpx_cpu_mg3_prolong_cubic_f64(const double *c, double *u, int dc, int hc, int wc, int pitch_c, int64_t plane_c,
                                  int pitch_u, int64_t plane_u) {
    int k;
    if (!c || !u || !mg3_coarse_ok(dc, hc, wc) || dc < 3 || hc < 3 || wc < 3 ||
        !mg3_strides_ok(hc, wc, pitch_c, plane_c) || !mg3_strides_ok(2 * hc - 1, 2 * wc - 1, pitch_u, plane_u))
        return -1;
    const int d = 2 * dc - 1, h = 2 * hc - 1, w = 2 * wc - 1;
#pragma omp parallel for schedule(static)
    for (k = 1; k < d - 1; ++k) {
        const int K = k / 2;
        for (int i = 1; i < h - 1; ++i) {
            double *o = u + (int64_t)k * plane_u + (int64_t)i * pitch_u;
            for (int j = 1; j < w - 1; ++j) {
                if (!(k & 1)) {
                    o[j] = cubic_plane(c + (int64_t)K * plane_c, hc, wc, pitch_c, i, j);
                    continue;
                }
                double v[4];
                for (int q = 0; q < 4; ++q) {
                    const int P = K - 1 + q;
                    if (P >= 0 && P < dc) {
                        v[q] = cubic_plane(c + (int64_t)P * plane_c, hc, wc, pitch_c, i, j);
                    } else {
                        double g[4];
                        for (int t = 0; t < 4; ++t) {
                            const int R = t < 3 || dc >= 4 ? t : 0; /* dc == 3: the fourth is not used */
                            g[t] = cubic_plane(c + (int64_t)(P < 0 ? R : dc - 1 - R) * plane_c, hc, wc, pitch_c, i, j);
                        }
                        v[q] = cubic_ghost(dc, g[0], g[1], g[2], g[3]);
                    }
                }
                o[j] = cubic_mid(v[0], v[1], v[2], v[3]);
            }
        }
    }
    return 0;
}

/* Host statistics with the reference's exact operation order
 * (reference lab3/src/main.cu:102-152): mean, unbiased covariance, cofactor
 * determinant and the modular-index adjugate inverse. */
int mpx_cpu_class_stats(const uint32_t *img, int w, int h, int nc, const int *np,
                        const int *coords, double *mu, double *inv) {
    const int *pts = coords;
    for (int c = 0; c < nc; ++c) {
        const int n = np[c];
        double sum[3] = {0.0, 0.0, 0.0};
        for (int i = 0; i < n; ++i) {
            const int x = pts[2 * i], y = pts[2 * i + 1];
            if (x < 0 || y < 0 || x >= w || y >= h) return -1;
            const uint32_t px = img[(int64_t)y * w + x];
            sum[0] += (double)mpx_px_r(px);
            sum[1] += (double)mpx_px_g(px);
            sum[2] += (double)mpx_px_b(px);
        }
        double avg[3] = {sum[0] / n, sum[1] / n, sum[2] / n};
        double cov[3][3];
        memset(cov, 0, sizeof(cov));
        for (int i = 0; i < n; ++i) {
            const uint32_t px = img[(int64_t)pts[2 * i + 1] * w + pts[2 * i]];
            const double d[3] = {(double)mpx_px_r(px) - avg[0], (double)mpx_px_g(px) - avg[1],
                                 (double)mpx_px_b(px) - avg[2]};
            for (int a = 0; a < 3; ++a)
                for (int b = 0; b < 3; ++b) {
                    const double prod = d[a] * d[b];
                    cov[a][b] += prod;
                }
        }
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) cov[a][b] /= (n - 1);
        const double m0 = cov[1][1] * cov[2][2] - cov[2][1] * cov[1][2];
        const double m1 = cov[1][0] * cov[2][2] - cov[1][2] * cov[2][0];
        const double m2 = cov[1][0] * cov[2][1] - cov[1][1] * cov[2][0];
        const double det = cov[0][0] * m0 - cov[0][1] * m1 + cov[0][2] * m2;
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) {
                const double p1 = cov[(b + 1) % 3][(a + 1) % 3] * cov[(b + 2) % 3][(a + 2) % 3];
                const double p2 = cov[(b + 1) % 3][(a + 2) % 3] * cov[(b + 2) % 3][(a + 1) % 3];
                inv[9 * c + 3 * a + b] = (p1 - p2) / det;
            }
        mu[3 * c + 0] = avg[0];
        mu[3 * c + 1] = avg[1];
        mu[3 * c + 2] = avg[2];
        pts += 2 * n;
    }
    return 0;
}

/* ---- lab5 sort: order-preserving uint32 keys (floats: IEEE total order of
 * the bit patterns), the same key map as native/src/kernels/sort.hip ---- */
static int cmp_u32(const void *a, const void *b) {
    const uint32_t x = *(const uint32_t *)a, y = *(const uint32_t *)b;
    return (x > y) - (x < y);
}

#ifdef _OPENMP
/* OpenMP build: T sorted runs (qsort per thread), then log2(T) rounds of
 * pairwise merges, each round's merges in parallel. */
static void merge_u32(const uint32_t *a, int64_t na, const uint32_t *b, int64_t nb, uint32_t *out) {
    int64_t i = 0, j = 0, o = 0;
    while (i < na && j < nb) out[o++] = b[j] < a[i] ? b[j++] : a[i++];
    while (i < na) out[o++] = a[i++];
    while (j < nb) out[o++] = b[j++];
}

static int sort_u32_parallel(uint32_t *x, int64_t n) {
    int runs = omp_get_max_threads();
    if (runs < 2 || n < (1 << 16)) return 0;
    uint32_t *tmp = (uint32_t *)malloc((size_t)n * sizeof(uint32_t));
    int64_t *bound = (int64_t *)malloc((size_t)(runs + 1) * sizeof(int64_t));
    if (!tmp || !bound) {
        free(tmp);
        free(bound);
        return 0;
    }
    for (int r = 0; r <= runs; ++r) bound[r] = n * r / runs;
#pragma omp parallel for schedule(static)
    for (int r = 0; r < runs; ++r) qsort(x + bound[r], (size_t)(bound[r + 1] - bound[r]), sizeof(uint32_t), cmp_u32);
    uint32_t *src = x, *dst = tmp;
    for (int width = 1; width < runs; width *= 2) {
#pragma omp parallel for schedule(dynamic, 1)
        for (int r = 0; r < runs; r += 2 * width) {
            const int mid = r + width < runs ? r + width : runs;
            const int end = r + 2 * width < runs ? r + 2 * width : runs;
            merge_u32(src + bound[r], bound[mid] - bound[r], src + bound[mid], bound[end] - bound[mid], dst + bound[r]);
        }
        uint32_t *t = src;
        src = dst;
        dst = t;
    }
    if (src != x) memcpy(x, src, (size_t)n * sizeof(uint32_t));
    free(tmp);
    free(bound);
    return 1;
}
#endif

void mpx_cpu_sort(void *data, int64_t n, int dtype) {
    if (n < 2) return;
    if (dtype == MPX_SORT_U8) { /* counting sort (per-thread histograms in the OpenMP build) */
        uint8_t *x = (uint8_t *)data;
        int64_t cnt[256] = {0};
#ifdef _OPENMP
#pragma omp parallel
        {
            int64_t local[256] = {0};
#pragma omp for schedule(static) nowait
            for (int64_t i = 0; i < n; ++i) local[x[i]]++;
#pragma omp critical
            for (int v = 0; v < 256; ++v) cnt[v] += local[v];
        }
        int64_t start[257];
        start[0] = 0;
        for (int v = 0; v < 256; ++v) start[v + 1] = start[v] + cnt[v];
#pragma omp parallel for schedule(dynamic, 8)
        for (int v = 0; v < 256; ++v) memset(x + start[v], v, (size_t)cnt[v]);
#else
        for (int64_t i = 0; i < n; ++i) cnt[x[i]]++;
        int64_t o = 0;
        for (int v = 0; v < 256; ++v)
            for (int64_t c = 0; c < cnt[v]; ++c) x[o++] = (uint8_t)v;
#endif
        return;
    }
    uint32_t *x = (uint32_t *)data;
    const int is_float = dtype == MPX_SORT_F32;
#ifdef _OPENMP
#pragma omp parallel for schedule(static)
#endif
    for (int64_t i = 0; i < n; ++i) {
        const uint32_t v = x[i];
        x[i] = is_float ? (v ^ ((uint32_t)((int32_t)v >> 31) | 0x80000000u)) : (v ^ 0x80000000u);
    }
#ifdef _OPENMP
    if (!sort_u32_parallel(x, n))
#endif
        qsort(x, (size_t)n, sizeof(uint32_t), cmp_u32);
#ifdef _OPENMP
#pragma omp parallel for schedule(static)
#endif
    for (int64_t i = 0; i < n; ++i) {
        const uint32_t k = x[i];
        x[i] = is_float ? (k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu)) : (k ^ 0x80000000u);
    }
}

/* ---- stable key-value sort: 64-bit composites (order-preserving key << 32 |
 * input index). The index makes every composite distinct, so any sort of the
 * composites is the stable sort of the keys (qsort alone is not stable);
 * descending complements the key, which keeps equal keys in input order. ---- */
static int cmp_u64(const void *a, const void *b) {
    const uint64_t x = *(const uint64_t *)a, y = *(const uint64_t *)b;
    return (x > y) - (x < y);
}

#ifdef _OPENMP
static void merge_u64(const uint64_t *a, int64_t na, const uint64_t *b, int64_t nb, uint64_t *out) {
    int64_t i = 0, j = 0, o = 0;
    while (i < na && j < nb) out[o++] = b[j] < a[i] ? b[j++] : a[i++];
    while (i < na) out[o++] = a[i++];
    while (j < nb) out[o++] = b[j++];
}

/* sort_u32_parallel on composites: sorted runs, then rounds of pairwise
 * merges; the result is in x or tmp (returned), NULL = not taken */
static uint64_t *sort_u64_parallel(uint64_t *x, uint64_t *tmp, int64_t n) {
    int runs = omp_get_max_threads();
    if (runs < 2 || n < (1 << 16)) return NULL;
    int64_t *bound = (int64_t *)malloc((size_t)(runs + 1) * sizeof(int64_t));
    if (!bound) return NULL;
    for (int r = 0; r <= runs; ++r) bound[r] = n * r / runs;
#pragma omp parallel for schedule(static)
    for (int r = 0; r < runs; ++r) qsort(x + bound[r], (size_t)(bound[r + 1] - bound[r]), sizeof(uint64_t), cmp_u64);
    uint64_t *src = x, *dst = tmp;
    for (int width = 1; width < runs; width *= 2) {
#pragma omp parallel for schedule(dynamic, 1)
        for (int r = 0; r < runs; r += 2 * width) {
            const int mid = r + width < runs ? r + width : runs;
            const int end = r + 2 * width < runs ? r + 2 * width : runs;
            merge_u64(src + bound[r], bound[mid] - bound[r], src + bound[mid], bound[end] - bound[mid], dst + bound[r]);
        }
        uint64_t *t = src;
        src = dst;
        dst = t;
    }
    free(bound);
    return src;
}
#endif

void mpx_cpu_sort_pairs(void *keys, uint32_t *vals, int64_t n, int dtype, int flags) {
    const int iota = flags & 1, desc = flags & 2; /* MPX_SORT_IOTA, MPX_SORT_DESCENDING */
    if (n < 1 || n > (int64_t)0xffffffff || (dtype != MPX_SORT_I32 && dtype != MPX_SORT_F32)) return;
    if (n == 1) {
        if (iota) vals[0] = 0;
        return;
    }
    uint32_t *x = (uint32_t *)keys;
    const int is_float = dtype == MPX_SORT_F32;
    const uint32_t flip = desc ? 0xffffffffu : 0u;
    /* composites, a merge buffer, and the caller's payload (gathered from) */
    uint64_t *c = (uint64_t *)malloc((size_t)n * sizeof(uint64_t));
    uint64_t *tmp = (uint64_t *)malloc((size_t)n * sizeof(uint64_t));
    uint32_t *pay = iota ? NULL : (uint32_t *)malloc((size_t)n * sizeof(uint32_t));
    if (!c || !tmp || (!iota && !pay)) {
        fprintf(stderr, "mpx_cpu_sort_pairs: out of memory for %lld pairs\n", (long long)n);
        abort();
    }
    if (pay) memcpy(pay, vals, (size_t)n * sizeof(uint32_t));
#ifdef _OPENMP
#pragma omp parallel for schedule(static)
#endif
    for (int64_t i = 0; i < n; ++i) {
        const uint32_t v = x[i];
        const uint32_t k = is_float ? (v ^ ((uint32_t)((int32_t)v >> 31) | 0x80000000u)) : (v ^ 0x80000000u);
        c[i] = ((uint64_t)(k ^ flip) << 32) | (uint64_t)i;
    }
    uint64_t *sorted = NULL;
#ifdef _OPENMP
    sorted = sort_u64_parallel(c, tmp, n);
#endif
    if (!sorted) {
        qsort(c, (size_t)n, sizeof(uint64_t), cmp_u64);
        sorted = c;
    }
#ifdef _OPENMP
#pragma omp parallel for schedule(static)
#endif
    for (int64_t i = 0; i < n; ++i) {
        const uint32_t k = (uint32_t)(sorted[i] >> 32) ^ flip, idx = (uint32_t)sorted[i];
        x[i] = is_float ? (k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu)) : (k ^ 0x80000000u);
        vals[i] = iota ? idx : pay[idx];
    }
    free(c);
    free(tmp);
    free(pay);
}

/* ---- lab4: dense LU with partial pivoting (the contract is in capi.h) ---- */
void mpx_cpu_lu_factor_f64(double *a, int n, int64_t pitch, int32_t *piv, int32_t *info) {
    if (info) *info = 0;
    if (!a || !piv || n <= 0 || pitch < n) return;
    for (int k = 0; k < n; ++k) {
        int p = k;
        double best = fabs(a[k * pitch + k]);
        for (int i = k + 1; i < n; ++i) {
            const double v = fabs(a[i * pitch + k]);
            if (v > best) { /* strict: the lowest row wins among equal magnitudes */
                best = v;
                p = i;
            }
        }
        if (best == 0.0) {
            piv[k] = k;
            if (info && *info == 0) *info = k + 1;
            continue;
        }
        piv[k] = p;
        double *rk = a + k * pitch;
        if (p != k) {
            double *rp = a + p * pitch;
            for (int j = 0; j < n; ++j) {
                const double t = rk[j];
                rk[j] = rp[j];
                rp[j] = t;
            }
        }
        const double d = rk[k];
#ifdef _OPENMP
#pragma omp parallel for schedule(static) if ((int64_t)(n - k) * (n - k) > 16384)
#endif
        for (int i = k + 1; i < n; ++i) {
            double *ri = a + i * pitch;
            const double l = ri[k] / d;
            ri[k] = l;
            for (int j = k + 1; j < n; ++j) ri[j] -= l * rk[j];
        }
    }
}

void mpx_cpu_lu_solve_f64(const double *lu, int n, int64_t pitch, const int32_t *piv, double *b, int nrhs,
                          int64_t pitch_b) {
    if (!lu || !piv || !b || n <= 0 || nrhs <= 0 || pitch < n || pitch_b < nrhs) return;
    for (int k = 0; k < n; ++k) {
        const int p = piv[k];
        if (p == k) continue;
        for (int j = 0; j < nrhs; ++j) {
            const double t = b[k * pitch_b + j];
            b[k * pitch_b + j] = b[p * pitch_b + j];
            b[p * pitch_b + j] = t;
        }
    }
    /* forward with unit L, then back with U: row i takes the finished rows k */
    for (int i = 1; i < n; ++i) {
        double *bi = b + i * pitch_b;
#ifdef _OPENMP
#pragma omp parallel for schedule(static) if ((int64_t)i * nrhs > 16384)
#endif
        for (int j = 0; j < nrhs; ++j) {
            double s = bi[j];
            for (int k = 0; k < i; ++k) s -= lu[i * pitch + k] * b[k * pitch_b + j];
            bi[j] = s;
        }
    }
    for (int i = n - 1; i >= 0; --i) {
        double *bi = b + i * pitch_b;
        const double d = lu[i * pitch + i];
#ifdef _OPENMP
#pragma omp parallel for schedule(static) if ((int64_t)(n - i) * nrhs > 16384)
#endif
        for (int j = 0; j < nrhs; ++j) {
            double s = bi[j];
            for (int k = i + 1; k < n; ++k) s -= lu[i * pitch + k] * b[k * pitch_b + j];
            bi[j] = s / d;
        }
    }
}

/* batched: every matrix on its own through the single-matrix functions above
 * (their inner OpenMP regions run serially inside this one) */
void mpx_cpu_lu_factor_batched_f64(double *a, int batch, int n, int64_t pitch, int64_t stride, int32_t *piv,
                                   int32_t *info) {
    if (!a || !piv || !info || batch <= 0 || n < 0 || pitch < n) return;
#ifdef _OPENMP
#pragma omp parallel for schedule(static)
#endif
    for (int m = 0; m < batch; ++m) mpx_cpu_lu_factor_f64(a + m * stride, n, pitch, piv + (int64_t)m * n, info + m);
}

void mpx_cpu_lu_solve_batched_f64(const double *lu, int batch, int n, int64_t pitch, int64_t stride,
                                  const int32_t *piv, double *b, int nrhs, int64_t pitch_b, int64_t stride_b) {
    if (!lu || !piv || !b || batch <= 0) return;
#ifdef _OPENMP
#pragma omp parallel for schedule(static)
#endif
    for (int m = 0; m < batch; ++m)
        mpx_cpu_lu_solve_f64(lu + m * stride, n, pitch, piv + (int64_t)m * n, b + m * stride_b, nrhs, pitch_b);
}

/* ---- lab4: dense Cholesky A = L L^T, lower storage (the contract is in capi.h) ---- */
void mpx_cpu_chol_factor_f64(double *a, int n, int64_t pitch, int32_t *info) {
    if (info) *info = 0;
    if (!a || n <= 0 || pitch < n) return;
    for (int j = 0; j < n; ++j) {
        double *rj = a + j * pitch;
        double t = rj[j];
        for (int k = 0; k < j; ++k) t -= rj[k] * rj[k];
        if (!(t > 0.0) && info && *info == 0) *info = j + 1; /* zero, negative and NaN; go on regardless */
        const double d = sqrt(t);
        rj[j] = d;
#ifdef _OPENMP
#pragma omp parallel for schedule(static) if ((int64_t)(n - j) * j > 16384)
#endif
        for (int i = j + 1; i < n; ++i) {
            double *ri = a + i * pitch;
            double s = ri[j];
            for (int k = 0; k < j; ++k) s -= ri[k] * rj[k];
            ri[j] = s / d;
        }
    }
}

void mpx_cpu_chol_solve_f64(const double *l, int n, int64_t pitch, double *b, int nrhs, int64_t pitch_b) {
    if (!l || !b || n <= 0 || nrhs <= 0 || pitch < n || pitch_b < nrhs) return;
    /* L y = b, then L^T x = y: row i takes the finished rows k, k ascending */
    for (int i = 0; i < n; ++i) {
        double *bi = b + i * pitch_b;
        const double d = l[i * pitch + i];
#ifdef _OPENMP
#pragma omp parallel for schedule(static) if ((int64_t)i * nrhs > 16384)
#endif
        for (int j = 0; j < nrhs; ++j) {
            double s = bi[j];
            for (int k = 0; k < i; ++k) s -= l[i * pitch + k] * b[k * pitch_b + j];
            bi[j] = s / d;
        }
    }
    for (int i = n - 1; i >= 0; --i) {
        double *bi = b + i * pitch_b;
        const double d = l[i * pitch + i];
#ifdef _OPENMP
#pragma omp parallel for schedule(static) if ((int64_t)(n - i) * nrhs > 16384)
#endif
        for (int j = 0; j < nrhs; ++j) {
            double s = bi[j];
            for (int k = i + 1; k < n; ++k) s -= l[k * pitch + i] * b[k * pitch_b + j];
            bi[j] = s / d;
        }
    }
}

/* batched: every member on its own through the two functions above (their
 * inner OpenMP regions run serially inside this one) */
void mpx_cpu_chol_factor_batched_f64(double *a, int batch, int n, int64_t pitch, int64_t stride, int32_t *info) {
    if (!a || !info || batch <= 0 || n < 0 || pitch < n) return;
#ifdef _OPENMP
#pragma omp parallel for schedule(static)
#endif
    for (int m = 0; m < batch; ++m) mpx_cpu_chol_factor_f64(a + m * stride, n, pitch, info + m);
}

void mpx_cpu_chol_solve_batched_f64(const double *l, int batch, int n, int64_t pitch, int64_t stride, double *b,
                                    int nrhs, int64_t pitch_b, int64_t stride_b) {
    if (!l || !b || batch <= 0) return;
#ifdef _OPENMP
#pragma omp parallel for schedule(static)
#endif
    for (int m = 0; m < batch; ++m)
        mpx_cpu_chol_solve_f64(l + m * stride, n, pitch, b + m * stride_b, nrhs, pitch_b);
}

/* ---- lab4: dense Householder QR, geqrf storage (the contract is in capi.h) ---- */
void mpx_cpu_qr_factor_f64(double *a, int m, int n, int64_t pitch, double *tau, int32_t *info) {
    if (info) *info = 0;
    if (!a || !tau || m <= 0 || n <= 0 || m < n || pitch < n) return;
    for (int j = 0; j < n; ++j) {
        double *rj = a + j * pitch;
        const double alpha = rj[j];
        double sigma = 0.0;
        for (int i = j + 1; i < m; ++i) sigma += a[i * pitch + j] * a[i * pitch + j];
        if (sigma == 0.0) { /* the column is left as it is: R_jj = alpha with its sign */
            tau[j] = 0.0;
            if (alpha == 0.0 && info && *info == 0) *info = j + 1;
            continue;
        }
        const double norm = sqrt(alpha * alpha + sigma);
        const double beta = -copysign(norm, alpha);
        const double t = (beta - alpha) / beta, d = alpha - beta;
        tau[j] = t;
        if (beta == 0.0 && info && *info == 0) *info = j + 1;
        /* the columns right of j first: they read column j unscaled, rows ascending */
#ifdef _OPENMP
#pragma omp parallel for schedule(static) if ((int64_t)(m - j) * (n - j) > 16384)
#endif
        for (int col = j + 1; col < n; ++col) {
            double g = 0.0;
            for (int i = j + 1; i < m; ++i) g += a[i * pitch + j] * a[i * pitch + col];
            const double w = t * (rj[col] + g / d);
            rj[col] -= w;
            for (int i = j + 1; i < m; ++i) a[i * pitch + col] -= (a[i * pitch + j] / d) * w;
        }
        for (int i = j + 1; i < m; ++i) a[i * pitch + j] = a[i * pitch + j] / d;
        rj[j] = beta;
    }
}

void mpx_cpu_qr_apply_f64(const double *qr, int m, int n, int64_t pitch, const double *tau, double *b, int nrhs,
                          int64_t pitch_b, int transpose) {
    if (!qr || !tau || !b || m <= 0 || n <= 0 || nrhs <= 0 || m < n || pitch < n || pitch_b < nrhs) return;
    for (int q = 0; q < n; ++q) { /* Q^T = H_{n-1} .. H_0 takes H_0 first, Q = H_0 .. H_{n-1} takes it last */
        const int j = transpose ? q : n - 1 - q;
        const double t = tau[j];
        if (t == 0.0) continue;
#ifdef _OPENMP
#pragma omp parallel for schedule(static) if ((int64_t)(m - j) * nrhs > 16384)
#endif
        for (int col = 0; col < nrhs; ++col) {
            double s = b[j * pitch_b + col];
            for (int i = j + 1; i < m; ++i) s += qr[i * pitch + j] * b[i * pitch_b + col];
            s = t * s;
            b[j * pitch_b + col] -= s;
            for (int i = j + 1; i < m; ++i) b[i * pitch_b + col] -= qr[i * pitch + j] * s;
        }
    }
}

void mpx_cpu_qr_rsolve_f64(const double *qr, int n, int64_t pitch, double *b, int nrhs, int64_t pitch_b) {
    if (!qr || !b || n <= 0 || nrhs <= 0 || pitch < n || pitch_b < nrhs) return;
    for (int i = n - 1; i >= 0; --i) {
        double *bi = b + i * pitch_b;
        const double d = qr[i * pitch + i];
#ifdef _OPENMP
#pragma omp parallel for schedule(static) if ((int64_t)(n - i) * nrhs > 16384)
#endif
        for (int j = 0; j < nrhs; ++j) {
            double s = bi[j];
            for (int k = i + 1; k < n; ++k) s -= qr[i * pitch + k] * b[k * pitch_b + j];
            bi[j] = s / d;
        }
    }
}
