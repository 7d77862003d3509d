/*
 * C ABI of libmpx.so — the one native library behind every lab CLI, the
 * multi-GPU tools and the Python package (loaded with ctypes).
 *
 * Conventions
 *   - every function returns 0 on success, a non-zero mpx error code otherwise;
 *     mpx_last_error() returns a thread-local human readable message;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream), so a
 *     PyTorch caller passes torch.cuda.current_stream().cuda_stream;
 *   - GPU entry points never allocate, free or synchronise (graph-capturable);
 *   - grid/block arguments of 0 mean "choose for MI355X" (256 CUs, wave64).
 *
 * The reference has no library at all (its library.cu is an empty kernel,
 * reference library.cu:3-4); every lab re-declared its own macros.
 */
#ifndef MPX_CAPI_H
#define MPX_CAPI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum mpx_status {
    MPX_OK = 0,
    MPX_ERR_ARG = 1,
    MPX_ERR_HIP = 2,
    MPX_ERR_UNSUPPORTED = 3,
    MPX_ERR_IO = 4
};

const char *mpx_last_error(void);
const char *mpx_version(void);
/* Loads every libmpx code object on the current device now instead of at the
 * first launch of one of its kernels (HIP loads them lazily, ~0.25 ms each). */
int mpx_preload_modules(void);

/* ---------------- device queries ---------------- */
int mpx_device_count(int *count);
/* Writes a multi-line report like the reference gpu_info (gpu_info/src/main.cu:9-16). */
int mpx_device_report(int device, char *buf, size_t len);
int mpx_stream_sync(void *stream);

/* ---------------- lab1: element-wise vector subtraction ---------------- */
/* c[i] = a[i] - b[i]; reference lab1/src/main.cu:22-29 */
int mpx_vsub_f64(const double *a, const double *b, double *c, int64_t n, int grid, int block,
                 void *stream);
int mpx_vsub_f32(const float *a, const float *b, float *c, int64_t n, int grid, int block,
                 void *stream);

/* ---------------- lab2: Roberts cross (launch-geometry faithful) ---------------- */
/* block (bx,by) and grid (gx,gy) exactly as the harness passes them
 * (reference lab2/src/to_plot.cu:57-64,106). Each thread owns 4 pixels of a row. */
int mpx_roberts(const uint32_t *in, uint32_t *out, int w, int h, int bx, int by, int gx, int gy,
                void *stream);
/* Per-channel Roberts cross, L1 magnitude, saturated to 255, alpha kept (the
 * operator of the reference's lab2/test_data samples; mpx_cpu_roberts_rgb). */
int mpx_roberts_rgb(const uint32_t *in, uint32_t *out, int w, int h, void *stream);

/* ---------------- lab2 generalisation: KxK convolution on luminance ---------------- */
/*
 * Output rows [oy0, oy1) of a (possibly slab-local) image.
 *   in/out   point at row 0 of the local slab, `pitch` pixels per row;
 *   y_lo/y_hi are the rows (relative to row 0, may be negative / >= rows when
 *            halo rows are resident) that input reads are clamped into;
 *   k, anchor  window size (2..7) and its anchor (taps at y+dy-anchor);
 *   wx, wy   k*k row-major taps (wy ignored unless mode == MPX_CONV_MAG2).
 * Accumulation order is fixed: dy ascending, dx ascending, one fmaf per tap.
 */
int mpx_conv(const uint32_t *in, uint32_t *out, int w, int pitch, int oy0, int oy1, int y_lo,
             int y_hi, int k, int anchor, int mode, const float *wx, const float *wy,
             void *stream);

/* mpx_conv with peer-sourced halo rows (one-sided xGMI loads): input rows with
 * logical index < 0 are read at in_up + row*pitch, rows >= own_rows at
 * in_dn + row*pitch (pointers into IPC-mapped neighbour slabs, biased so the
 * logical row index applies unchanged), rows [0, own_rows) from `in`. */
int mpx_conv_peer(const uint32_t *in, const uint32_t *in_up, const uint32_t *in_dn, int own_rows,
                  uint32_t *out, int w, int pitch, int oy0, int oy1, int y_lo, int y_hi, int k, int anchor,
                  int mode, const float *wx, const float *wy, void *stream);

/* Generic direct (untiled, one pixel per thread) variant of mpx_conv: any
 * anchor, naive global loads; the baseline the tiled kernel is measured against. */
int mpx_conv_direct(const uint32_t *in, uint32_t *out, int w, int pitch, int oy0, int oy1, int y_lo,
                    int y_hi, int k, int anchor, int mode, const float *wx, const float *wy,
                    void *stream);

/* Minimum image size in pixels for the band kernel (smaller aligned images take
 * the wave kernel); returns the previous value, n < 0 only queries. */
long long mpx_conv_set_band_min(long long n);
/* band kernel mode (as MPX_CONV_BAND: 0 wave kernel, 1 plain stores, 2 NT stores,
 * 3 NT stores + NT interior loads (default), 4 vertical halo sharing through LDS
 * for 5-row windows); returns the previous mode, m < 0 queries */
int mpx_conv_set_band_mode(int m);
/* Which kernel an mpx_conv / mpx_conv_peer launch of `rows` output rows
 * (oy1 - oy0) of a w-wide image with a k x k window takes, given 16-byte
 * aligned rows, a tap class with a band instantiation (every dense class;
 * separable MAG2 / LIN1) and the current band mode and band minimum:
 * 0 wave kernel, 1 conv_band4_kernel, 2 conv_band16v_kernel. *seg receives the
 * rows per wave segment and *opt the kernel's OPT value (0, 2, 34, 2|2048,
 * 34|2048: bit 11 = batched aprons, walks of at most 32 rows; 2|64 for the
 * 16v kernel); both 0 for the wave kernel. resident: the MPX_CONV_RESIDENT
 * hint; remote_rows: mpx_conv_peer with halo rows outside `in`. The launcher
 * decides by the same function; host arithmetic only, no GPU needed. */
int mpx_conv_band_plan(int w, int rows, int k, int anchor, int resident, int remote_rows,
                       int *seg, int *opt);

/* Tuning-harness entry (tools/kbench.py): kernel variants for k in {2, 5}, MAG2,
 * whole image. kind 0 = LDS streaming kernel (p1 = rows per wave 4/8/16,
 * p2 = tiles per workgroup, 0 = auto); kind 1 = wave-streaming kernel
 * (p1 = rows per wave segment). fast selects the fast magnitude path. */
int mpx_conv_variant(const uint32_t *in, uint32_t *out, int w, int h, int k, int kind, int p1, int p2, int fast,
                     const float *wx, const float *wy, void *stream);
/* Exhaustive check of the fast magnitude path over every float in [0, 65025];
 * adds the number of disagreements with correctly rounded sqrtf to *bad_device. */
int mpx_selftest_fast_sqrt(unsigned long long *bad_device, int raw, void *stream);

/* Named filter table (native/include/mpx/filters.h). Returns MPX_ERR_ARG for an
 * unknown name; wx/wy receive k*k taps (wy zero-filled for one-filter modes).
 * mpx_filter_name(i) enumerates the table (NULL past the end). */
int mpx_filter_lookup(const char *name, int *k, int *anchor, int *mode, float *wx, float *wy);
const char *mpx_filter_name(int i);

/* ---------------- lab3: Mahalanobis maximum-likelihood classifier ---------------- */
/*
 * Per-class statistics from training points (reference lab3/src/main.cu:102-152).
 * coords holds (x, y) pairs for every class back to back; np[c] points per class.
 * mu: nc*3, inv: nc*9 (row-major inverse covariance), computed in fp64 on the host.
 */
int mpx_class_stats(const uint32_t *img, int w, int h, int nc, const int *np, const int *coords,
                    double *mu, double *inv);
/* img[i].a = argmin_c (p - mu_c)^T inv_c (p - mu_c), in place (alpha = 255 if all NaN). */
int mpx_classify(uint32_t *img, int64_t npix, int nc, const double *mu, const double *inv,
                 int grid, int block, int path, void *stream);
/* Same; when `ambiguous` (device uint32) is non-NULL it is incremented once per
 * pixel whose fp32 margin was too small and that took the exact fp64 chain. */
int mpx_classify_ex(uint32_t *img, int64_t npix, int nc, const double *mu, const double *inv,
                    int grid, int block, int path, uint32_t *ambiguous, void *stream);
/* Host-side plan: the path `path` resolves to for these statistics (DIRECT when
 * the fp32 decision cannot be proven) and the fp32 decision margin. <0 = error. */
int mpx_classify_plan(int nc, const double *mu, const double *inv, int path, float *margin);
/* MFMA8 integer weights as the kernel uses them (CPU emulation in the tests):
 * a, b: 32 x 16 int8 limbs per class and slot; c: 32 accumulator constants;
 * *t2: decision margin in key units. MPX_ERR_UNSUPPORTED when no bound exists. */
int mpx_classify_i8_params(int nc, const double *mu, const double *inv, int8_t *a, int8_t *b, int32_t *c,
                           int32_t *t2);

/* ---------------- native RCCL tier (inter-GPU transport) ---------------- */
/*
 * The ncclXxx entry points are bound with dlsym from `path` (the librccl torch
 * loaded; RTLD_NOLOAD first so one RCCL serves the whole process).
 * A communicator owns a non-blocking comm stream and two events:
 * p2p_start orders a grouped send/recv list after the work queued on `stream`
 * and runs it on the comm stream; p2p_wait makes `stream` wait for it.
 */
int mpx_comm_load(const char *path);
int mpx_comm_version(void);
int mpx_comm_unique_id(void *out, int nbytes); /* returns the id size */
int mpx_comm_init(void **comm, int nranks, int rank, const void *id, int nbytes, int device);
int mpx_comm_destroy(void *comm);
int mpx_comm_rank(void *comm);
int mpx_comm_size(void *comm);
int mpx_comm_p2p_start(void *comm, int n, const int *kind, void *const *ptr, const int64_t *bytes,
                       const int *peer, void *stream); /* kind 0 send, 1 recv */
int mpx_comm_p2p_wait(void *comm, void *stream);
/* the same op list in order on `stream` itself (no comm stream, no events) */
int mpx_comm_p2p(void *comm, int n, const int *kind, void *const *ptr, const int64_t *bytes, const int *peer,
                 void *stream);
/* dtype 0 f64, 1 f32, 2 i32, 3 u64; op 0 sum, 1 max, 2 min; on `stream` */
int mpx_comm_allreduce(void *comm, const void *send, void *recv, int64_t count, int dtype, int op,
                       void *stream);
int mpx_comm_check(void *comm);
/* ncclCommAbort: release a communicator whose peers hung or died (watchdog) */
int mpx_comm_abort(void *comm);
/* the communicator's comm stream (for caller-managed cross-step pipelining) */
void *mpx_comm_stream(void *comm);

/* ---------------- device memory shared between the processes of a node ---------------- */
int mpx_ipc_handle_size(void);
/* handle: mpx_ipc_handle_size() bytes; *offset = ptr - base of ptr's allocation */
int mpx_ipc_get_handle(const void *ptr, void *handle, int64_t *offset);
/* maps a peer's allocation on the current device (peer access enabled lazily) */
int mpx_ipc_open(const void *handle, void **base);
/* the same with hipSetDevice(device) first (mapping from a helper thread) */
int mpx_ipc_open_dev(int device, const void *handle, void **base);
int mpx_ipc_close(void *base);
/* stream-ordered device-to-device copy (either side may be IPC-mapped) */
int mpx_memcpy_d2d(void *dst, const void *src, int64_t bytes, void *stream);

/* ---------------- one-sided transports: probes, streaming halo fetch (peer.hip) ---------------- */
/* *out += position-sensitive checksum of nrows rows read with the kernels' 16-byte
 * buffer loads (sys != 0: system-scope cache policy); zero *out first. */
int mpx_rows_checksum(const void *rows, int64_t row_bytes, int nrows, int64_t pitch_bytes, int sys,
                      unsigned long long *out, void *stream);
/* Signalled start-up probe (one workgroup): write a (rank, buffer)-pattern into
 * own_rows[0..3] (buffer = index / 2; NULL = skip) with system-scope stores,
 * publish sync[0] = magic (release), then for each side s with flag[s]: wait
 * flag[s] >= magic (bounded; sync[64] = 1 on give-up) and compare
 * nb_rows[s][0..1] with the neighbour's pattern; mismatching words are added
 * to sync[96]. row_bytes: a multiple of 4 (16-byte accesses when every row is
 * 16-byte aligned and row_bytes a multiple of 16, 4-byte ones otherwise). */
typedef struct mpx_peer_probe {
    void *own_rows[4];
    const void *nb_rows[2][2];
    const unsigned int *flag[2];
    unsigned int *sync;
    int64_t row_bytes;
    int rank;
    unsigned int magic;
    unsigned int spin_limit;
} mpx_peer_probe;
int mpx_peer_probe_run(const mpx_peer_probe *p, void *stream);
/* Streaming halo fetch (filters the fused band kernel does not cover): block s
 * first copies this rank's own boundary rows own_src[s] into its mailbox rows
 * mb_dst[s] (mb_bytes[s], system-scope write-through stores); once BOTH blocks'
 * copies are acknowledged the later one publishes sync[0] = step (release).
 * Then per side s with a neighbour (flag[s] != NULL): wait flag[s] >= step
 * (bounded), and when src[s] is set copy bytes[s] from it (the neighbour's
 * mailbox rows, system-scope loads) to dst[s] (this rank's halo rows). A side
 * without rows to copy still waits: the neighbour reads this rank's mailbox
 * (write-after-read order). */
typedef struct mpx_halo_fetch {
    const void *src[2];
    void *dst[2];
    int64_t bytes[2];
    const unsigned int *flag[2];
    unsigned int *sync;
    unsigned int step;
    unsigned int spin_limit;
    const void *own_src[2];
    void *mb_dst[2];
    int64_t mb_bytes[2];
} mpx_halo_fetch;
int mpx_halo_fetch_run(const mpx_halo_fetch *f, void *stream);
/* Streaming convolution with the halo exchange fused into the band kernel (one
 * launch per step, no fetch kernel): the waves whose rows touch the slab edges
 * read their halo rows straight from the neighbours' mailboxes (system-scope
 * loads) after a bounded wait on the neighbour's step word, write their first
 * n_first / last n_last output rows into this rank's mailbox as well
 * (write-through), and the last of the n_edge edge waves publishes the step;
 * interior waves never wait. The step index c = this rank's sync[0] (completed
 * steps, read on the device): the halo rows come from slot c & 1 of the
 * neighbours' mailboxes, the output rows go to slot (c + 1) & 1 of this one.
 * up_src[p] / dn_src[p]: biased row-source pointers (logical row g < 0 at
 * up_src[p] + g * w, g >= own_rows at dn_src[p] + g * w); NULL flag = global
 * edge (the clamp rows then come from `in` itself). Requires the band kernel:
 * k <= 5 with at most two columns of reach per side, w % 4 == 0, pitch == w,
 * 16-byte aligned rows. */
typedef struct mpx_conv_stream_peer {
    const uint32_t *up_src[2];
    const uint32_t *dn_src[2];
    const unsigned int *up_flag;
    const unsigned int *dn_flag;
    uint32_t *mb_first[2];
    uint32_t *mb_last[2];
    unsigned int *sync;
    int n_first;
    int n_last;
    int n_edge; /* filled in by the launcher */
    unsigned int spin_limit;
} mpx_conv_stream_peer;
int mpx_conv_stream_peer_run(const uint32_t *in, uint32_t *out, int w, int pitch, int own_rows, int y_lo, int y_hi,
                         int k, int anchor, int mode, const float *wx, const float *wy,
                         const mpx_conv_stream_peer *sp, void *stream);
/* 1 when mpx_conv_stream_peer can run this launch shape, else 0 */
int mpx_conv_stream_peer_ok(int w, int pitch, int own_rows, int k, int anchor, int mode);
/* IPC-exportable sync block: uncached (kind 2), fine-grained (1) or coarse (0) memory, zeroed */
int mpx_sync_alloc(int64_t bytes, void **ptr, int *kind);
int mpx_sync_free(void *ptr);
/* synchronous host access to word `word` (0..127) of a sync block */
int mpx_sync_write(unsigned int *sync, int word, unsigned int value);
int mpx_sync_read(const unsigned int *sync, int word, unsigned int *value);
int mpx_sync_clear(unsigned int *sync, int64_t bytes);

/* ---------------- 2-D Jacobi (distributed stencil tier) ---------------- */
/*
 * One sweep over rows [r0, r1) of a slab stored with one halo row above and
 * below: `u`/`un` point at the first halo row, rows 1..rows are owned, the row
 * pitch is `pitch` elements, columns 0 and cols-1 are Dirichlet boundary.
 *   un[i][j] = 0.25*(u[i-1][j] + u[i+1][j] + u[i][j-1] + u[i][j+1])  (j in 1..cols-2)
 * Rows listed in [r0, r1) are 1-based owned rows. When `resid` is non-NULL the
 * kernel folds max|un-u| over the swept points into *resid (atomic max, bit
 * pattern of a non-negative double), so callers zero it first.
 */
/* One-sided, device-signalled halo sweep of a whole slab (rows 1..rows of a
 * (rows + 2) x pitch buffer): the halo rows are read from the neighbours'
 * IPC-mapped buffers, ordered by completed-iteration counters (see jacobi.hip).
 * up_row[k] / dn_row[k]: the neighbour's last / first owned row of u at even
 * (k = 0) / odd (k = 1) iterations — rows of its MAILBOX (a small exported
 * allocation, so slabs of any size keep the one-sided transport), or of its
 * slab buffers when mb_first / mb_last are NULL; NULL (with a NULL flag) at
 * the global boundary, where the local halo row is the boundary row.
 * sync: this rank's mpx_jacobi_sync_bytes() block; word 0 = completed
 * iterations (the neighbours' *_flag points at theirs), word 64 != 0 after a
 * bounded wait gave up. */
typedef struct mpx_jacobi_peer {
    const void *up_row[2];
    const void *dn_row[2];
    const unsigned int *up_flag;
    const unsigned int *dn_flag;
    unsigned int *sync;
    unsigned int spin_limit; /* polls before a wait gives up (0 = default, ~seconds) */
    /* this rank's mailbox rows (one row each; slot p receives the edge row of
     * u^(t) for t % 2 == p, written during sweep t - 1 with write-through
     * stores): mb_first = its first owned row (read by the upper neighbour),
     * mb_last = its last (read by the lower one); NULL at a global edge */
    void *mb_first[2];
    void *mb_last[2];
} mpx_jacobi_peer;
int mpx_jacobi_sync_bytes(void);
int mpx_jacobi_peer_sweep(int fp64, void *u, void *un, int cols, int pitch, int rows, void *resid,
                          const mpx_jacobi_peer *p, void *stream);
int mpx_jacobi_f64(const double *u, double *un, int cols, int pitch, int r0, int r1,
                   double *resid, void *stream);
int mpx_jacobi_f32(const float *u, float *un, int cols, int pitch, int r0, int r1, float *resid,
                   void *stream);
/* Poisson sweeps (-Laplace(u) = f): the same sweeps with a right-hand side `b`
 * laid out like u (same shape and pitch), b = h^2 * f already scaled by the
 * mesh width:
 *   un[i][j] = (((u[i-1][j] + u[i+1][j]) + (u[i][j-1] + u[i][j+1])) + b[i][j]) * 0.25
 * in exactly this association (four correctly rounded adds, an exact scale),
 * so fp32, fp64 and the CPU reference agree bit for bit with a plain
 * expression. b is read at the interior points of the swept rows only: its
 * halo rows and boundary columns are don't-care. A NULL b is an argument
 * error; a b that is not 16-byte aligned takes the scalar kernel (the peer
 * sweep refuses it). The residual stays max|un - u|. */
int mpx_jacobi_rhs_f64(const double *u, const double *b, double *un, int cols, int pitch, int r0, int r1,
                       double *resid, void *stream);
int mpx_jacobi_rhs_f32(const float *u, const float *b, float *un, int cols, int pitch, int r0, int r1,
                       float *resid, void *stream);
int mpx_jacobi_peer_sweep_rhs(int fp64, void *u, const void *b, void *un, int cols, int pitch, int rows,
                              void *resid, const mpx_jacobi_peer *p, void *stream);
/* Chebyshev (semi-iterative) step. With s the value of the plain sweep (b NULL)
 * or of the Poisson sweep (b given) and p = un[i][j] as found on entry, the
 * iterate before last:
 *   un[i][j] = p + omega * (s - p)
 * a subtract, a multiply and an add, each rounded separately (never an FMA), so
 * fp32, fp64, the CPU reference and a plain expression agree bit for bit. un is
 * in-out: only rows [r0, r1) are read and written. omega is rounded once to the
 * sweep's type; it must be finite and positive (also after that rounding).
 * The residual word keeps its meaning, max|s - u|, a quarter of the defect's
 * max norm, independent of omega. Path selection, the alignment rules and the
 * peer descriptor are those of the sweeps above. The first step of a sequence
 * is the plain sweep itself (mpx_jacobi_f64 / mpx_jacobi_rhs_f64), not
 * omega = 1: (s - p) + p is not s in floating point. */
int mpx_jacobi_accel_f64(const double *u, const double *b, double *un, int cols, int pitch, int r0, int r1,
                         double omega, double *resid, void *stream);
int mpx_jacobi_accel_f32(const float *u, const float *b, float *un, int cols, int pitch, int r0, int r1,
                         double omega, float *resid, void *stream);
int mpx_jacobi_peer_sweep_accel(int fp64, void *u, const void *b, void *un, int cols, int pitch, int rows,
                                double omega, void *resid, const mpx_jacobi_peer *p, void *stream);
/* Damped Jacobi sweep (the multigrid smoother). With s the value of the plain
 * sweep (b NULL) or of the Poisson sweep (b given) and c = u[i][j], the
 * interior points of rows [r0, r1) get
 *     un[i][j] = c + omega * (s - c)
 * as three rounded operations, omega rounded once to the buffer type (finite
 * and positive, before and after that rounding: otherwise MPX_ERR_ARG and
 * nothing is written). un is output only; boundary columns copy through; the
 * residual is max|s - c|. Path selection and alignment rules are those of the
 * sweeps above; pitch >= cols, padding is never read or written. */
int mpx_jacobi_relax_f64(const double *u, const double *b, double *un, int cols, int pitch, int r0, int r1,
                         double omega, double *resid, void *stream);
int mpx_jacobi_relax_f32(const float *u, const float *b, float *un, int cols, int pitch, int r0, int r1,
                         double omega, float *resid, void *stream);

/* Geometric multigrid on an (H, W) grid with Dirichlet values in rows 0 / H-1
 * and columns 0 / W-1 (native/src/kernels/multigrid.hip). The coarse grid of
 * (H, W) is (hc, wc) with H = 2 hc - 1, W = 2 wc - 1; coarse (I, J) sits on
 * fine (2I, 2J). Every buffer has its own row pitch in elements (>= its
 * width); padding is never read for a result and never written; row offsets
 * are 64-bit. Every + - * is one rounded operation, never an FMA. 16-byte
 * aligned bases with pitches that are multiples of the 16-byte vector take the
 * vector kernels, everything else the per-element kernels.
 *
 * residual: r = ((((up + dn) + (l + rt)) + b) - 4 c) at the interior points
 *   (without b: no "+ b"); r's boundary is not written; resid (nullable, zeroed
 *   by the caller) receives max|r|. rows, cols >= 3.
 * restrict (full weighting, scaled for the h^2-scaled coarse right-hand side):
 *   for coarse interior (I, J), i = 2I, j = 2J,
 *     e = (r[i-1][j] + r[i+1][j]) + (r[i][j-1] + r[i][j+1])
 *     d = (r[i-1][j-1] + r[i-1][j+1]) + (r[i+1][j-1] + r[i+1][j+1])
 *     bc[I][J] = (r[i][j] + e * 0.5) + d * 0.25
 *   bc's boundary is not written; r's boundary is not read for a result.
 * prolong_add (bilinear interpolation added to u's interior, in place):
 *     u[2I][2J]     += e[I][J]
 *     u[2I+1][2J]   += (e[I][J] + e[I+1][J]) * 0.5
 *     u[2I][2J+1]   += (e[I][J] + e[I][J+1]) * 0.5
 *     u[2I+1][2J+1] += ((e[I][J] + e[I+1][J]) + (e[I][J+1] + e[I+1][J+1])) * 0.25
 *   e's boundary is read; u's boundary is not written. hc, wc >= 2.
 * prolong_cubic (cubic interpolation of the coarse c written over u's interior;
 *   the interpolant of full multigrid). The 1-D rule takes n >= 3 values
 *   c[0..n-1] to 2n - 1 values: the even ones copy c, and the midpoint between
 *   K and K + 1 is, with a = c[K] + c[K+1] and o = c[K-1] + c[K+2],
 *     m = (a + (a - o) * 0.125) * 0.5
 *   (the weights (-1, 9, 9, -1) / 16). c[-1] and c[n] are ghosts extrapolated
 *   from the same values:
 *     n >= 4: c[-1] = ((c[0] + c[2]) * 4 - c[3]) - c[1] * 6
 *             c[n]  = ((c[n-1] + c[n-3]) * 4 - c[n-4]) - c[n-2] * 6
 *     n == 3: c[-1] = (c[0] - c[1]) * 3 + c[2],  c[3] = (c[2] - c[1]) * 3 + c[0]
 *   (with the midpoint rule: the one-sided cubic (5, 15, -5, 1) / 16 and the
 *   parabola (3, 6, -1) / 8). The 2-D rule applies the 1-D rule along every
 *   coarse row, which gives hc rows of width W, and then down the columns of
 *   those rows; the ghost rows are formed element by element from the
 *   interpolated rows. c's boundary is read (the coarse Dirichlet values); only
 *   u's interior is written. hc, wc >= 3. */
int mpx_mg_residual_f64(const double *u, const double *b, double *r, int rows, int cols, int pitch_u, int pitch_b,
                        int pitch_r, double *resid, void *stream);
int mpx_mg_residual_f32(const float *u, const float *b, float *r, int rows, int cols, int pitch_u, int pitch_b,
                        int pitch_r, float *resid, void *stream);
int mpx_mg_restrict_f64(const double *r, double *bc, int hc, int wc, int pitch_r, int pitch_bc, void *stream);
int mpx_mg_restrict_f32(const float *r, float *bc, int hc, int wc, int pitch_r, int pitch_bc, void *stream);
int mpx_mg_prolong_add_f64(const double *e, double *u, int hc, int wc, int pitch_e, int pitch_u, void *stream);
int mpx_mg_prolong_add_f32(const float *e, float *u, int hc, int wc, int pitch_e, int pitch_u, void *stream);
int mpx_mg_prolong_cubic_f64(const double *c, double *u, int hc, int wc, int pitch_c, int pitch_u, void *stream);
int mpx_mg_prolong_cubic_f32(const float *c, float *u, int hc, int wc, int pitch_c, int pitch_u, void *stream);

/* 3-D sweeps (the 7-point Laplace / Poisson stencil). u, un and the optional b
 * are contiguous (planes + 2) x ny x nx buffers, x fastest; planes 0 and
 * planes + 1 are halo planes, rows 0 / ny - 1 and columns 0 / nx - 1 are
 * Dirichlet. A sweep covers planes [k0, k1), 1 <= k0 <= k1 (empty: no-op):
 *     s = ((((zm + zp) + (ym + yp)) + (xm + xp)) [+ b]) * c,  c = (T)(1.0 / 6.0)
 * at the interior points, every operation rounded, never fused; boundary
 * elements of a swept plane receive u's value, other planes are not written.
 * b == NULL is the Laplace form. The accel entries write p + omega * (s - p)
 * with p = un's value on entry (three rounded operations, omega rounded once
 * to T and finite and positive before and after). resid (may be NULL): a
 * one-element device word zeroed by the caller that receives max|s - u| over
 * the swept interior points. Needs nx >= 3, ny >= 3, ny * nx < 2^31; plane
 * offsets are 64-bit. Widths that are a multiple of the 16-byte vector with
 * 16-byte aligned pointers take the wave-strip kernel, everything else the
 * per-lane kernel (native/src/kernels/jacobi3d.hip). */
int mpx_jacobi3d_f64(const double *u, const double *b, double *un, int nx, int ny, int k0, int k1, double *resid,
                     void *stream);
int mpx_jacobi3d_f32(const float *u, const float *b, float *un, int nx, int ny, int k0, int k1, float *resid,
                     void *stream);
int mpx_jacobi3d_accel_f64(const double *u, const double *b, double *un, int nx, int ny, int k0, int k1, double omega,
                           double *resid, void *stream);
int mpx_jacobi3d_accel_f32(const float *u, const float *b, float *un, int nx, int ny, int k0, int k1, double omega,
                           float *resid, void *stream);
/* The wave-strip form and tile of the production launches for a dtype (fp64 != 0:
 * double) and sweep kind (rhs: with b; accel: the Chebyshev entries): out[0] =
 * form (0: rows-in-plane walk, 1: z-march; + 2: workgroups remapped so that
 * launch-order neighbours share an XCD), out[1] = TY (rows per wave), out[2] =
 * KZ (planes marched per wave), out[3] = the wave count below which a launch
 * halves its tile (rows: TY, march: KZ) until it has that many waves or the
 * tile is 1. out: 4 ints. */
int mpx_jacobi3d_tile(int fp64, int rhs, int accel, int *out);

/* 3-D geometric multigrid on a (D, H, W) grid, x fastest, with Dirichlet values
 * on all six faces (native/src/kernels/multigrid3d.hip). Every buffer is
 * pitched: unit element stride in x, a row pitch >= W and a plane stride >=
 * H * pitch, both in elements; plane offsets are 64-bit; padding is never read
 * for a result and never written. The coarse grid of (D, H, W) is (dc, hc, wc)
 * with D = 2 dc - 1, H = 2 hc - 1, W = 2 wc - 1; coarse (K, J, I) sits on fine
 * (2K, 2J, 2I). The discrete equation is 6 u - (sum of the six neighbours) = b,
 * b = h^2 f. Every + - * is one rounded operation in the buffer type, never an
 * FMA, so fp32, fp64, the CPU references and a dtype-preserving expression
 * agree bit for bit. 16-byte aligned bases with pitches and plane strides that
 * are multiples of the 16-byte vector take the vector kernels, everything else
 * the per-element kernels. Null pointers and bad geometry: MPX_ERR_ARG, nothing
 * written. With n = ((zm + zp) + (ym + yp)) + (xm + xp) [+ b] (b NULL: no "+ b")
 * and c the centre value:
 *
 * jacobi3d_relax (the damped sweep over planes [k0, k1), 1 <= k0 <= k1 <= d - 1;
 *   empty: no-op): s = n * (T)(1.0 / 6.0), exactly mpx_jacobi3d_*'s s; interior
 *   points get un = c + omega * (s - c), three rounded operations, omega rounded
 *   once to T (finite and positive before and after that rounding: otherwise
 *   MPX_ERR_ARG and nothing is written). Boundary rows and columns of a swept
 *   plane copy through; other planes are not written; un is output only. resid
 *   (nullable, zeroed by the caller) receives max|s - c| as the sweeps fold
 *   theirs. u, b and un share one pitch and one plane stride.
 * mg3_residual: r = n - (T)6 * c at the interior points; r's boundary is not
 *   written; resid (nullable, zeroed by the caller) receives max|r|. d, ny,
 *   nx >= 3.
 * mg3_restrict (27-point full weighting, scaled for the h^2-scaled coarse
 *   right-hand side, defined separably): for each fine plane k, P_k[J][I] is the
 *   2-D rule of mg_restrict above applied in the plane, with i = 2J, j = 2I:
 *     e = (r[k][i-1][j] + r[k][i+1][j]) + (r[k][i][j-1] + r[k][i][j+1])
 *     d = (r[k][i-1][j-1] + r[k][i-1][j+1]) + (r[k][i+1][j-1] + r[k][i+1][j+1])
 *     P_k[J][I] = (r[k][i][j] + e * 0.5) + d * 0.25
 *   then bc[K][J][I] = (P_2K + (P_2K-1 + P_2K+1) * 0.5) * 0.5 at the coarse
 *   interior (weights: centre 0.5, face 0.25, edge 0.125, corner 0.0625). bc's
 *   boundary is not written; r's boundary is not read for a result; without a
 *   coarse interior (dc, hc or wc < 3) the call is a no-op. dc, hc, wc >= 2.
 * mg3_prolong_add (trilinear interpolation added to u's interior, in place):
 *   unscaled pair sums in z, then y, then x, and one exact scale:
 *     Z[k]       = e[K] for k = 2K,        e[K] + e[K+1] for k = 2K + 1
 *     Y[k][i]    = Z[k][J] for i = 2J,     Z[k][J] + Z[k][J+1] for i = 2J + 1
 *     X[k][i][j] = Y[k][i][I] for j = 2I,  Y[k][i][I] + Y[k][i][I+1] for j = 2I + 1
 *     u[k][i][j] += X[k][i][j] * 0.5^(number of odd coordinates among k, i, j)
 *   with no multiply when that factor is 1. e's boundary is read; u's boundary
 *   is not written. dc, hc, wc >= 2.
 * mg3_prolong_cubic (tricubic interpolation of the coarse c written over u's
 *   interior; the interpolant of full multigrid), separable, built from the 1-D
 *   rule of prolong_cubic above, unchanged (midpoint (a + (a - o) * 0.125) * 0.5,
 *   cubic ghosts for n >= 4, parabola ghosts for n == 3): the rule runs along x
 *   in every coarse row, which gives dc x hc rows of width W; then along y down
 *   the columns of those rows, the ghost rows formed element by element from
 *   the interpolated rows, which gives dc planes of H x W; then along z through
 *   those planes, the ghost planes formed element by element from them. So the
 *   interior of fine plane 2K, 1 <= K <= dc - 2, is mg_prolong_cubic of coarse
 *   plane K bit for bit. c's boundary is read (the coarse Dirichlet values);
 *   only u's interior is written. dc, hc, wc >= 3. */
int mpx_jacobi3d_relax_f64(const double *u, const double *b, double *un, int d, int ny, int nx, int pitch,
                           int64_t plane, int k0, int k1, double omega, double *resid, void *stream);
int mpx_jacobi3d_relax_f32(const float *u, const float *b, float *un, int d, int ny, int nx, int pitch, int64_t plane,
                           int k0, int k1, double omega, float *resid, void *stream);
int mpx_mg3_residual_f64(const double *u, const double *b, double *r, int d, int ny, int nx, int pitch_u,
                         int64_t plane_u, int pitch_b, int64_t plane_b, int pitch_r, int64_t plane_r, double *resid,
                         void *stream);
int mpx_mg3_residual_f32(const float *u, const float *b, float *r, int d, int ny, int nx, int pitch_u, int64_t plane_u,
                         int pitch_b, int64_t plane_b, int pitch_r, int64_t plane_r, float *resid, void *stream);
int mpx_mg3_restrict_f64(const double *r, double *bc, int dc, int hc, int wc, int pitch_r, int64_t plane_r,
                         int pitch_bc, int64_t plane_bc, void *stream);
int mpx_mg3_restrict_f32(const float *r, float *bc, int dc, int hc, int wc, int pitch_r, int64_t plane_r, int pitch_bc,
                         int64_t plane_bc, void *stream);
int mpx_mg3_prolong_add_f64(const double *e, double *u, int dc, int hc, int wc, int pitch_e, int64_t plane_e,
                            int pitch_u, int64_t plane_u, void *stream);
int mpx_mg3_prolong_add_f32(const float *e, float *u, int dc, int hc, int wc, int pitch_e, int64_t plane_e, int pitch_u,
                            int64_t plane_u, void *stream);
int mpx_mg3_prolong_cubic_f64(const double *c, double *u, int dc, int hc, int wc, int pitch_c, int64_t plane_c,
                              int pitch_u, int64_t plane_u, void *stream);
int mpx_mg3_prolong_cubic_f32(const float *c, float *u, int dc, int hc, int wc, int pitch_c, int64_t plane_c,
                              int pitch_u, int64_t plane_u, void *stream);
/* The walks of the 3-D multigrid launches: out[0] = rows of a plane walked per
 * lane by relax / residual, out[1] / out[2] = coarse planes walked per lane by
 * the restriction / the prolongation, out[3] = the wave count below which a
 * launch halves its walk until it has that many waves or the walk is 1,
 * out[4] = waves per workgroup (row blocks of the stencil walk, coarse rows of
 * the transfers). out: 5 ints. */
int mpx_mg3_walk(int *out);
/* The walk of mg3_prolong_cubic: out[0] = coarse planes walked per lane,
 * out[1] = the wave count below which a launch halves that walk (mpx_mg3_walk's
 * out[3]), out[2] = waves (coarse rows) per workgroup. out: 3 ints. */
int mpx_mg3_cubic_walk(int *out);

/* The coarse levels of a V-cycle in one kernel (native/src/kernels/mg_tail.hip):
 * one workgroup runs, from lv[0] down to lv[n - 1] and back up, what the launched
 * cycle runs for a level k >= 1. For every level but the last: nu1 damped sweeps
 * (mpx_jacobi_relax / mpx_jacobi3d_relax over all interior rows / planes, with
 * the level's b), the residual into r, full weighting of r into the next level's
 * b, the next level's u <- 0 on its H x W (D x H x W) elements, the next level,
 * prolongation added in place, nu2 damped sweeps. The last level: coarse_sweeps
 * damped sweeps, or one sweep with omega = 1 when it is 3 x 3 (3 x 3 x 3). Every
 * point's expression is that of the launched operator above, operation for
 * operation, so the result is bit-identical to the launches.
 *
 * Sweeps ping-pong between a level's u and un, starting from u: afterwards a
 * level's iterate lies in un when the level ran an odd number of sweeps
 * (nu1 + nu2; the last level coarse_sweeps or 1), in u otherwise; the other of
 * the two and r are scratch. Rows 0 and H - 1 (3-D: planes 0 and D - 1 too) of
 * un are never written and are read by every second sweep: as for the launched
 * sweeps they are input and hold the boundary values of the level (lv[0]: those
 * of its u; below lv[0]: zeros). u, un, b and r of a level share its
 * pitch (and plane stride); padding is never read for a result and never
 * written; r of the last level may be NULL. One launch of one workgroup on
 * `stream`; no allocation, no synchronisation, no residual maximum.
 * MPX_ERR_ARG, nothing written: null pointers, n < 1 or n > 16, a level that is
 * not the coarse grid of the one before it (H = 2 Hc - 1, ...), a dimension
 * below 3, pitch < w, plane < h * pitch, nu1 < 0, nu2 < 1, coarse_sweeps < 1, an
 * omega that is not finite and positive before and after its rounding to T. */
#define MPX_MG_TAIL_MAX_LEVELS 16
typedef struct mpx_mg_level {
    void *u, *un, *b, *r;
    int h, w, pitch;
} mpx_mg_level;
typedef struct mpx_mg3_level {
    void *u, *un, *b, *r;
    int d, h, w, pitch;
    int64_t plane;
} mpx_mg3_level;
int mpx_mg_tail_f64(const mpx_mg_level *lv, int n, int nu1, int nu2, int coarse_sweeps, double omega, void *stream);
int mpx_mg_tail_f32(const mpx_mg_level *lv, int n, int nu1, int nu2, int coarse_sweeps, double omega, void *stream);
int mpx_mg3_tail_f64(const mpx_mg3_level *lv, int n, int nu1, int nu2, int coarse_sweeps, double omega, void *stream);
int mpx_mg3_tail_f32(const mpx_mg3_level *lv, int n, int nu1, int nu2, int coarse_sweeps, double omega, void *stream);

/* ---------------- lab5: ascending sort (no reference program) ---------------- */
/* In place on the device; dtype is an mpx_sort_dtype. int32/float32: LSD radix sort
 * (onesweep, 8-bit digits) on order-preserving uint32 keys, bitonic network for
 * n <= 4096 or n >= 2^30; uint8: counting sort.
 * mpx_sort_ws takes the scratch from the caller (>= mpx_sort_workspace_bytes(n, dtype)
 * bytes, 16-byte aligned, stream-ordered with `stream`; may be NULL when that size is 0).
 * mpx_sort allocates and frees its own scratch and synchronises the stream. */
int64_t mpx_sort_workspace_bytes(int64_t n, int dtype);
int mpx_sort_ws(void *data, int64_t n, int dtype, void *workspace, int64_t workspace_bytes, void *stream);
/* After the sort's stream drained: non-zero if a bounded look-back wait of the
 * sort that last used `workspace` gave up (hardware-fault detector). */
int mpx_sort_ws_status(const void *workspace, int64_t n, int dtype);
int mpx_sort(void *data, int64_t n, int dtype, void *stream);
/* 1 when the current device applies same-address returning LDS adds in
 * ascending lane order (the stability premise of the production radix
 * ranking; probed once per device, synchronising the stream), 0 when not,
 * negative when the probe could not run. AUTO falls back to the peer-mask
 * ranking unless 1. */
int mpx_sort_lane_order_ok(void *stream);

/* Stable key-value sort, in place on the device: `keys` (int32 or float32,
 * dtype MPX_SORT_I32 / MPX_SORT_F32, floats in the IEEE total order above) and
 * one opaque 32-bit word per key in `vals`, moved with its key and never
 * interpreted. Equal keys keep their input order, ascending and descending
 * (as torch.sort(stable=True, descending=True)). Four 8-bit LSD radix passes
 * for every n >= 2; n < 2^30 (MPX_ERR_UNSUPPORTED beyond, before any pointer
 * is touched), MPX_SORT_U8 and unknown flag bits are MPX_ERR_UNSUPPORTED.
 * flags: MPX_SORT_IOTA — `vals` is output only and receives the permutation
 * (vals[i] = input index of the key now at i; the argsort), generated in the
 * first pass instead of loaded; MPX_SORT_DESCENDING — descending keys.
 * The workspace follows mpx_sort_ws: caller-provided,
 * >= mpx_sort_pairs_workspace_bytes(n, dtype) bytes (a second n x 4 byte array
 * beside the keys-only layout; 0 for n < 2), 16-byte aligned, stream-ordered.
 * mpx_cpu_sort_pairs is the stable CPU reference (n < 2^32). */
enum { MPX_SORT_IOTA = 1, MPX_SORT_DESCENDING = 2 };
int64_t mpx_sort_pairs_workspace_bytes(int64_t n, int dtype);
int mpx_sort_pairs_ws(void *keys, uint32_t *vals, int64_t n, int dtype, int flags, void *workspace,
                      int64_t workspace_bytes, void *stream);

/* ---------------- lab4: dense LU with partial pivoting, fp64 (no reference program) ---------------- */
/* Right-looking LU of a square row-major n x n matrix, in place
 * (native/src/kernels/lu.hip): unit-lower L (multipliers a_ik / pivot below the
 * diagonal) and U (on and above it) in one array, as LAPACK getrf stores them.
 * Column k's pivot is the row i >= k of largest |a_ik| in the updated column,
 * the lowest row index among equal magnitudes; piv[k] is that row (0-based: the
 * row interchanged with row k, LAPACK's ipiv minus one), and the interchange
 * moves the whole row. A column whose remaining part is exactly zero takes
 * piv[k] = k, is left as it is, and elimination goes on; *info (a device word)
 * receives k + 1 for the first such k and 0 otherwise. NaN / inf propagate and
 * the pivots chosen among them are unspecified.
 * Panels of 64 columns: one launch per panel column while more than 256 rows
 * remain (partial pivot searches folded by the last workgroup to finish, found
 * with a counter, never by waiting), one workgroup for the rest; row
 * interchanges outside the panel, U12 by substitution with the panel's unit
 * triangle, and the trailing update on v_mfma_f64_16x16x4_f64. The MFMA's
 * accumulation order is unspecified, so the GPU and the CPU reference do not
 * agree bit for bit on general input; both satisfy the componentwise backward
 * error bounds of LU (tests/test_lu.py) and agree exactly wherever every
 * intermediate is exactly representable.
 * solve: B (n x nrhs, row-major, pitch_b) <- A^-1 B with the factors: rows
 * interchanged by piv, then forward substitution with unit L and back
 * substitution with U in blocks of 64 rows, the diagonal blocks by substitution
 * (never an inverse), the blocks between them by the MFMA update.
 * pitch >= n and pitch_b >= nrhs are row pitches in elements; padding is never
 * read or written; 16-byte aligned bases with even pitches load the update's
 * operands 16 bytes at a time, everything else 8. The workspace is the
 * caller's, >= mpx_lu_workspace_bytes(n) bytes, 16-byte aligned and
 * stream-ordered (mpx_sort_ws's rule); the solve needs none and ignores it.
 * MPX_ERR_ARG before any pointer is touched: n < 0, nrhs < 0, pitch < n,
 * pitch_b < nrhs, a null pointer, a short workspace. n = 0 and nrhs = 0 are
 * no-ops. No allocation, no synchronisation. */
int64_t mpx_lu_workspace_bytes(int n);
int mpx_lu_factor_f64(double *a, int n, int64_t pitch, int32_t *piv, int32_t *info, void *workspace,
                      int64_t workspace_bytes, void *stream);
int mpx_lu_solve_f64(const double *lu, int n, int64_t pitch, const int32_t *piv, double *b, int nrhs,
                     int64_t pitch_b, void *workspace, int64_t workspace_bytes, void *stream);
/* Tuning-harness entries (tools/bench_lu.py): the phases of one panel step at
 * column j0 (a multiple of the panel width with more than 256 rows left) on their own. phase 0: the panel
 * (needs the workspace), 1: the interchanges outside it, 2: U12, 3: the
 * trailing update. mpx_lu_panel_width: the panel width in use, 64, or
 * MPX_LU_NB = 16 / 32 from the environment (the sweep; read once per process). */
int mpx_lu_panel_width(void);
int mpx_lu_phase_f64(double *a, int n, int64_t pitch, int32_t *piv, int32_t *info, int j0, int phase,
                     void *workspace, int64_t workspace_bytes, void *stream);

/* Batched: `batch` square n x n matrices of one size (native/src/kernels/lu_batched.hip).
 * Matrix m starts at a + m * stride, its rows are pitch >= n elements apart,
 * and stride >= (n - 1) * pitch + n for batch > 1 (64-bit arithmetic); the
 * padding between rows and between matrices is never read or written. piv is
 * (batch, n) contiguous int32, 0-based; info is batch int32 device words, each
 * 0 or k + 1 for that matrix's first exactly zero pivot. B's matrix m starts at
 * b + m * stride_b, rows pitch_b >= nrhs apart, stride_b >= (n - 1) * pitch_b + nrhs.
 * n <= 64: per matrix the result is exactly what mpx_cpu_lu_factor_f64 /
 * mpx_cpu_lu_solve_f64 produce for that matrix alone, bit for bit: the same
 * pivot rule (largest magnitude, the lowest current row among equals, piv[k] = k
 * and the column left as it is on an exactly zero column; a NaN at row k stays
 * the pivot, a NaN below it never becomes one), l = a_ik / d by IEEE division,
 * a_ij = a_ij - l u_kj for k ascending with every operation rounded once (no
 * FMA), forward substitution s -= lu_ik b_kj for k ascending, back substitution
 * the same for k = i + 1 .. n - 1 ascending and then one division by the
 * diagonal. The factorisation is one launch: a lane holds one row in registers
 * (padded to 8 / 16 / 32 / 64 columns, 64 / padded width matrices per wave), the
 * matrix is read and written once, piv and info are written by the kernel. The
 * solve is one launch: a lane is one (matrix, right-hand side) pair,
 * 64 / min(nrhs, 64) matrices per wave; out-of-range pivot entries are skipped.
 * Neither needs a workspace: mpx_lu_batched_workspace_bytes is 0 for n <= 64.
 * n > 64: correct, not fast. A loop over the matrices through
 * mpx_lu_factor_f64 / mpx_lu_solve_f64 on the same stream, with one workspace
 * of mpx_lu_workspace_bytes(n) bytes (16-byte aligned) reused across the
 * stream-ordered matrices; the yardstick there is the single-matrix one (exact
 * recovery and the backward-error bounds), not bits.
 * MPX_ERR_ARG before any pointer is touched: batch < 0, n < 0, nrhs < 0,
 * pitch < n, pitch_b < nrhs, a short stride, a null pointer, a short or
 * misaligned workspace. batch = 0, n = 0 and nrhs = 0 are no-ops. No
 * allocation, no host synchronisation, everything on the given stream. */
int64_t mpx_lu_batched_workspace_bytes(int batch, int n);
int mpx_lu_factor_batched_f64(double *a, int batch, int n, int64_t pitch, int64_t stride, int32_t *piv,
                              int32_t *info, void *workspace, int64_t workspace_bytes, void *stream);
int mpx_lu_solve_batched_f64(const double *lu, int batch, int n, int64_t pitch, int64_t stride, const int32_t *piv,
                             double *b, int nrhs, int64_t pitch_b, int64_t stride_b, void *stream);

/* lab4: Cholesky factorisation A = L L^T of a symmetric positive definite
 * n x n fp64 matrix, row-major, lower storage, in place
 * (native/src/kernels/chol.hip). Only the lower triangle (diagonal included) is
 * read, and on exit it holds L; the strict upper triangle and the pitch padding
 * are never read and never written. Per element, every operation rounded once
 * (no FMA):
 *   t = a_ij;  for k = 0 .. j-1 ascending:  t = t - (l_ik * l_jk)
 *   j == i:  l_jj = sqrt(t)  (correctly rounded);   j < i:  l_ij = t / l_jj  (IEEE division)
 * *info (a device word) is 0, or j + 1 for the first column whose reduced
 * diagonal t is not > 0 (zero, negative and NaN alike). Columns 0 .. j-1 of L
 * are then valid in every row, the rest of the lower triangle is unspecified;
 * the kernels run on with whatever values result, and the first failure stays.
 * Panels of 64 columns and nothing per column: one workgroup factors the
 * diagonal block in LDS, L21 = A21 L11^-T by substitution with one lane per row,
 * and A22 -= L21 L21^T on v_mfma_f64_16x16x4_f64 over the lower tiles only. The
 * workgroup that updates the next diagonal block factors it on the spot, so a
 * factorisation is 1 + 2 (ceil(n / 64) - 1) launches. The diagonal block and the
 * panel solve are plain VALU in the order above, so columns 0 .. 63 of L (the
 * whole factor for n <= 64) equal mpx_cpu_chol_factor_f64's bit for bit; from
 * column 64 on the MFMA's unspecified accumulation order is in every element,
 * and the yardsticks are exact recovery and the backward-error bounds
 * (tests/test_cholesky.py). What holds bit for bit at any n: an element of L
 * depends on the leading rows and columns only (chol(A[:m, :m]) is the leading
 * block of chol(A), a block-diagonal matrix factors block by block), and the
 * columns of B are independent systems, NaN and infinite ones included
 * (tests/test_cholesky_invariants.py).
 * solve: B (n x nrhs, row-major, pitch_b) <- A^-1 B with L:
 *   acc = b_i;  for k = 0 .. i-1 ascending:    acc -= l_ik y_k;   y_i = acc / l_ii
 *   acc = y_i;  for k = i+1 .. n-1 ascending:  acc -= l_ki x_k;   x_i = acc / l_ii
 * in blocks of 64 rows, the diagonal blocks by substitution (never an inverse),
 * the blocks between them by the MFMA update (bit for bit the CPU reference's
 * result for n <= 64). 16-byte aligned bases with even pitches load the
 * updates' operands 16 bytes at a time, everything else 8.
 * MPX_ERR_ARG before any pointer is touched: n < 0, nrhs < 0, pitch < n,
 * pitch_b < nrhs, a null pointer. n = 0 and nrhs = 0 are no-ops. No workspace,
 * no allocation, no synchronisation; everything runs on the given stream. */
int mpx_chol_factor_f64(double *a, int n, int64_t pitch, int32_t *info, void *stream);
int mpx_chol_solve_f64(const double *l, int n, int64_t pitch, double *b, int nrhs, int64_t pitch_b, void *stream);
/* Tuning-harness entry (tools/bench_cholesky.py): one phase of the panel step at
 * column j0 (a multiple of 64 below n). phase 0: the diagonal block (it zeroes
 * *info first when j0 == 0), 1: the panel solve, 2: the symmetric update alone
 * (it leaves the next diagonal block updated, not factored). The three in order
 * over every panel give the factorisation's bits. */
int mpx_chol_phase_f64(double *a, int n, int64_t pitch, int32_t *info, int j0, int phase, void *stream);

/* Batched: `batch` symmetric positive definite n x n matrices of one size
 * (native/src/kernels/chol_batched.hip). Member m starts at a + m * stride, its
 * rows are pitch >= n elements apart, and stride >= (n - 1) * pitch + n for
 * batch > 1 (64-bit arithmetic, the product must not wrap). Per member the
 * contract is exactly mpx_chol_factor_f64 / mpx_chol_solve_f64 above: lower
 * storage, in place; only the lower triangle, diagonal included, is read or
 * written, and the strict upper triangle, the pitch padding and the gap between
 * members are never read and never written. info is batch int32 device words,
 * every one written by the call and nothing outside info[0 .. batch): 0, or
 * j + 1 for that member's first column whose reduced diagonal is not > 0 (zero,
 * negative and NaN alike); columns before it are valid in every row, the rest
 * of that member's triangle is unspecified, and no other member is affected.
 * B's member m starts at b + m * stride_b, rows pitch_b >= nrhs apart,
 * stride_b >= (n - 1) * pitch_b + nrhs.
 * n <= 64: per member the result is exactly what mpx_cpu_chol_factor_f64 /
 * mpx_cpu_chol_solve_f64 produce for that member alone, bit for bit:
 * t = a_ij, t = t - (l_ik * l_jk) for k ascending with every operation rounded
 * once (no FMA), l_jj = sqrt(t) correctly rounded, l_ij = t / l_jj by IEEE
 * division; forward substitution acc -= l_ik y_k for k ascending, then / l_ii,
 * back substitution acc -= l_ki x_k for k = i + 1 .. n - 1 ascending, then
 * / l_ii. The factorisation is one launch: a lane holds one row in registers
 * (padded to 8 / 16 / 32 / 64 columns, 64 / padded width members per wave),
 * right-looking: at column j the reduced diagonal is broadcast within the
 * member's lanes, the rows below divide and publish column j through LDS, and
 * every lane subtracts the k = j term from its elements j + 1 .. row. The lower
 * triangles are read and written once; info is written by the kernel. The solve
 * is one launch: a lane is one (member, right-hand side) pair,
 * 64 / min(nrhs, 64) members per wave, ceil(nrhs / 64) chunks.
 * n > 64: correct, not fast. A loop over the members through
 * mpx_chol_factor_f64 / mpx_chol_solve_f64 on the same stream; the yardstick
 * there is the single-matrix one (exact recovery and the backward-error
 * bounds), not bits.
 * MPX_ERR_ARG before any pointer is touched: batch < 0, n < 0, nrhs < 0,
 * pitch < n, pitch_b < nrhs, a short stride, a null pointer, batch x nrhs
 * beyond the blocks of one launch. batch = 0, n = 0 and nrhs = 0 are no-ops. No
 * workspace, no allocation, no host synchronisation, everything on the given
 * stream. */
int mpx_chol_factor_batched_f64(double *a, int batch, int n, int64_t pitch, int64_t stride, int32_t *info,
                                void *stream);
int mpx_chol_solve_batched_f64(const double *l, int batch, int n, int64_t pitch, int64_t stride, double *b, int nrhs,
                               int64_t pitch_b, int64_t stride_b, void *stream);

/* lab4: Householder QR A = Q R of a tall or square m x n fp64 matrix (m >= n >= 0),
 * row-major with a row pitch, in place, in LAPACK geqrf storage
 * (native/src/kernels/qr.hip). On return the upper triangle of A[0:n, 0:n]
 * holds R, column j below the diagonal holds v_j[j+1:m] (v_j[j] = 1 implied),
 * tau is n doubles, H_j = I - tau_j v_j v_j^T and Q = H_0 H_1 .. H_{n-1}. The
 * pitch padding is never read or written.
 * Reflector j (LAPACK dlarfg's rule without its rescaling): alpha = a_jj,
 * sigma = sum_{i > j} a_ij^2. sigma == 0 exactly: tau_j = 0 and the column is
 * left as it is, so R_jj = alpha with its sign. Otherwise
 *   norm = sqrt(alpha^2 + sigma)  (sqrt correctly rounded),
 *   beta = -copysign(norm, alpha),  tau_j = (beta - alpha) / beta,
 *   v_i = a_ij / (alpha - beta)  (an IEEE division, not a reciprocal),  R_jj = beta,
 * and every column right of j takes w = tau_j (a_j,col + g_col / (alpha - beta))
 * with g_col = sum_{i > j} a_ij a_i,col: a_j,col -= w, a_i,col -= v_i w. The
 * diagonal of R may be negative; the last column of a square matrix has
 * tau = 0. The sums of squares are plain fp64: a_ij^2 must neither overflow
 * nor underflow to zero (no scaled norms).
 * *info (a device word) is 0, or j + 1 for the first column with R_jj == 0
 * exactly. The factorisation runs on regardless (nothing is singular for QR
 * itself; only the triangular solve needs info). A NaN is not a zero: it
 * propagates to its own column and the columns right of it, nowhere else.
 * Panels of 64 columns, right-looking. One launch per panel column (and one
 * more per panel): a rank-1 VALU update of the panel, per-workgroup partials of
 * the next column's Gram row, folded in index order by the last workgroup to
 * finish (a counter after __threadfence(), nobody ever waits). Then four
 * launches per panel with columns to its right: W = V^T C and V^T V on
 * v_mfma_f64_16x16x4_f64 with a K loop over the rows, cut into chunks of 1024
 * rows whose partials are summed in ascending order; T (larft, forward,
 * columnwise) by one workgroup; Z = T^T W; C -= V Z on the MFMA. A
 * factorisation is n + 5 ceil(n / 64) + 1 launches at most. No floating-point
 * atomics; every reduction over rows has a fixed order that depends on m, the
 * pitch alignment class and the column's index alone: two runs give the same
 * bits, and column j of the result depends only on columns 0 .. j of the input
 * (the factorisation of A[:, :k] is the first k columns of that of A, bit for
 * bit). The MFMA's accumulation order is unspecified and the reduction orders
 * differ, so the GPU and the CPU reference agree to Householder QR's
 * backward-error bounds, not bit for bit (tests/test_qr.py), and exactly
 * wherever every intermediate is exactly representable.
 * apply: B (m x nrhs, row-major, pitch_b) <- Q^T B (transpose != 0) or Q B from
 * the stored reflectors, one block reflector I - V T V^T per panel, four
 * launches each; T is rebuilt per panel and never stored across calls.
 * rsolve: B (n x nrhs) <- R^-1 B with the upper triangle of qr[0:n, 0:n], blocked
 * back substitution: substitution on the 64 x 64 diagonal blocks (never an
 * inverse), the MFMA update between them.
 * The workspace is the caller's, >= mpx_qr_workspace_bytes(m, n, nrhs) bytes
 * (nrhs = 0 for the factorisation), 16-byte aligned and stream-ordered
 * (mpx_sort_ws's rule); rsolve needs none.
 * MPX_ERR_ARG before any pointer is touched: a negative size, m < n, pitch < n,
 * pitch_b < nrhs, a null pointer, a short or misaligned workspace. m = 0, n = 0
 * and nrhs = 0 are no-ops. No allocation, no host synchronisation. */
int64_t mpx_qr_workspace_bytes(int m, int n, int nrhs);
int mpx_qr_factor_f64(double *a, int m, int n, int64_t pitch, double *tau, int32_t *info, void *workspace,
                      int64_t workspace_bytes, void *stream);
int mpx_qr_apply_f64(const double *qr, int m, int n, int64_t pitch, const double *tau, double *b, int nrhs,
                     int64_t pitch_b, int transpose, void *workspace, int64_t workspace_bytes, void *stream);
int mpx_qr_rsolve_f64(const double *qr, int n, int64_t pitch, double *b, int nrhs, int64_t pitch_b, void *stream);
/* The launcher's geometry for an m x n matrix, so that tests aim at the real
 * chunking: out = {rows per workgroup of the panel kernel, rows of one W chunk,
 * W chunks of the first panel, panel width}. */
int mpx_qr_plan(int m, int n, int32_t out[4]);
/* Tuning-harness entry (tools/bench_qr.py): one phase of the panel step at
 * column j0 (a multiple of 64 below n). phase 0: the panel's columns (it zeroes
 * *info first when j0 == 0), 1: W = V^T C and V^T V, 2: T and Z, 3: C -= V Z.
 * Phases 1..3 do nothing for the last panel. The four in order over every panel
 * give the factorisation's bits. */
int mpx_qr_phase_f64(double *a, int m, int n, int64_t pitch, double *tau, int32_t *info, int j0, int phase,
                     void *workspace, int64_t workspace_bytes, void *stream);

/* ---------------- CPU references (OpenMP, -O3, same numerics) ---------------- */
int mpx_cpu_threads(void);
void mpx_cpu_vsub_f64(const double *a, const double *b, double *c, int64_t n);
void mpx_cpu_vsub_f32(const float *a, const float *b, float *c, int64_t n);
void mpx_cpu_roberts(const uint32_t *in, uint32_t *out, int w, int h);
void mpx_cpu_roberts_rgb(const uint32_t *in, uint32_t *out, int w, int h);
void mpx_cpu_conv(const uint32_t *in, uint32_t *out, int w, int pitch, int oy0, int oy1, int y_lo,
                  int y_hi, int k, int anchor, int mode, const float *wx, const float *wy);
void mpx_cpu_classify(uint32_t *img, int64_t npix, int nc, const double *mu, const double *inv);
double mpx_cpu_jacobi_f64(const double *u, double *un, int cols, int pitch, int r0, int r1);
/* with the right-hand side of mpx_jacobi_rhs_f64; NaN when b is NULL */
double mpx_cpu_jacobi_rhs_f64(const double *u, const double *b, double *un, int cols, int pitch, int r0, int r1);
/* the Chebyshev step of mpx_jacobi_accel_f64 (b may be NULL, un is in-out);
 * NaN, with nothing written, on a null u / un, bad geometry or a bad omega */
double mpx_cpu_jacobi_accel_f64(const double *u, const double *b, double *un, int cols, int pitch, int r0, int r1,
                                double omega);
/* the damped sweep of mpx_jacobi_relax_f64 (b may be NULL, un output only);
 * NaN, with nothing written, on a null u / un, bad geometry or a bad omega */
double mpx_cpu_jacobi_relax_f64(const double *u, const double *b, double *un, int cols, int pitch, int r0, int r1,
                                double omega);
/* the multigrid operators of mpx_mg_*_f64. residual returns max|r| (NaN, with
 * nothing written, on bad arguments); restrict and prolong_add return 0, or
 * -1, with nothing written, on bad arguments */
double mpx_cpu_mg_residual_f64(const double *u, const double *b, double *r, int rows, int cols, int pitch_u,
                               int pitch_b, int pitch_r);
int mpx_cpu_mg_restrict_f64(const double *r, double *bc, int hc, int wc, int pitch_r, int pitch_bc);
int mpx_cpu_mg_prolong_add_f64(const double *e, double *u, int hc, int wc, int pitch_e, int pitch_u);
int mpx_cpu_mg_prolong_cubic_f64(const double *c, double *u, int hc, int wc, int pitch_c, int pitch_u);
/* the 3-D sweeps of mpx_jacobi3d_f64 / mpx_jacobi3d_accel_f64 (b may be NULL);
 * both return the residual, or NaN, with nothing written, on a null u / un,
 * bad geometry or a bad omega */
double mpx_cpu_jacobi3d_f64(const double *u, const double *b, double *un, int nx, int ny, int k0, int k1);
double mpx_cpu_jacobi3d_accel_f64(const double *u, const double *b, double *un, int nx, int ny, int k0, int k1,
                                  double omega);
/* the 3-D multigrid operators of mpx_jacobi3d_relax_f64 / mpx_mg3_*_f64. relax
 * and residual return the residual (NaN, with nothing written, on a null
 * pointer, bad geometry or a bad omega); restrict and prolong_add return 0, or
 * -1, with nothing written, on bad arguments */
double mpx_cpu_jacobi3d_relax_f64(const double *u, const double *b, double *un, int d, int ny, int nx, int pitch,
                                  int64_t plane, int k0, int k1, double omega);
double mpx_cpu_mg3_residual_f64(const double *u, const double *b, double *r, int d, int ny, int nx, int pitch_u,
                                int64_t plane_u, int pitch_b, int64_t plane_b, int pitch_r, int64_t plane_r);
int mpx_cpu_mg3_restrict_f64(const double *r, double *bc, int dc, int hc, int wc, int pitch_r, int64_t plane_r,
                             int pitch_bc, int64_t plane_bc);
int mpx_cpu_mg3_prolong_cubic_f64(const double *c, double *u, int dc, int hc, int wc, int pitch_c, int64_t plane_c,
                                  int pitch_u, int64_t plane_u);
int mpx_cpu_mg3_prolong_add_f64(const double *e, double *u, int dc, int hc, int wc, int pitch_e, int64_t plane_e,
                                int pitch_u, int64_t plane_u);
void mpx_cpu_sort(void *data, int64_t n, int dtype);
void mpx_cpu_sort_pairs(void *keys, uint32_t *vals, int64_t n, int dtype, int flags);
/* the unblocked algorithm of mpx_lu_factor_f64 / mpx_lu_solve_f64 (info: a host
 * word); bad arguments write nothing but *info = 0 */
void mpx_cpu_lu_factor_f64(double *a, int n, int64_t pitch, int32_t *piv, int32_t *info);
void mpx_cpu_lu_solve_f64(const double *lu, int n, int64_t pitch, const int32_t *piv, double *b, int nrhs,
                          int64_t pitch_b);
/* the batched entries' reference and what CPU tensors run: an OpenMP loop over
 * the matrices that calls the two functions above (info: batch host words) */
void mpx_cpu_lu_factor_batched_f64(double *a, int batch, int n, int64_t pitch, int64_t stride, int32_t *piv,
                                   int32_t *info);
void mpx_cpu_lu_solve_batched_f64(const double *lu, int batch, int n, int64_t pitch, int64_t stride,
                                  const int32_t *piv, double *b, int nrhs, int64_t pitch_b, int64_t stride_b);
/* the unblocked algorithm of mpx_chol_factor_f64 / mpx_chol_solve_f64 (info: a
 * host word), OpenMP over the rows of a column; bad arguments write nothing but
 * *info = 0 */
void mpx_cpu_chol_factor_f64(double *a, int n, int64_t pitch, int32_t *info);
void mpx_cpu_chol_solve_f64(const double *l, int n, int64_t pitch, double *b, int nrhs, int64_t pitch_b);
/* the batched Cholesky entries' reference and what CPU tensors run: an OpenMP
 * loop over the members that calls the two functions above (info: batch host
 * words); bad arguments write nothing */
void mpx_cpu_chol_factor_batched_f64(double *a, int batch, int n, int64_t pitch, int64_t stride, int32_t *info);
void mpx_cpu_chol_solve_batched_f64(const double *l, int batch, int n, int64_t pitch, int64_t stride, double *b,
                                    int nrhs, int64_t pitch_b, int64_t stride_b);
/* the unblocked algorithm of mpx_qr_factor_f64 / mpx_qr_apply_f64 /
 * mpx_qr_rsolve_f64 (info: a host word), rows summed in ascending order, OpenMP
 * over the columns of the update; bad arguments write nothing but *info = 0 */
void mpx_cpu_qr_factor_f64(double *a, int m, int n, int64_t pitch, double *tau, int32_t *info);
void mpx_cpu_qr_apply_f64(const double *qr, int m, int n, int64_t pitch, const double *tau, double *b, int nrhs,
                          int64_t pitch_b, int transpose);
void mpx_cpu_qr_rsolve_f64(const double *qr, int n, int64_t pitch, double *b, int nrhs, int64_t pitch_b);

#ifdef __cplusplus
}
#endif

#endif /* MPX_CAPI_H */
