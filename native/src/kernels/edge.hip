// lab2: Roberts cross and its KxK generalisation (gradient-magnitude / linear
// convolution on fp32 luminance of RGBA8 images).
//
// Reference behaviour: lab2/src/main.cu:15-52 — per pixel, four tex2D fetches
// (clamp addressing), luminance recomputed for each of them, Gx = Y11 - Y00,
// Gy = Y10 - Y01, G = sqrtf(Gx^2 + Gy^2) clamped and truncated, alpha of p00
// preserved. The reference reads through a texture cache; CDNA has no reason
// to: this file stages each tile's luminance ONCE per input pixel in LDS
// (160 KiB per CU), moves 16 B per lane from HBM, and writes 8-16 B per lane.
//
// Numerics are defined by native/src/cpu/cpu_kernels.c and reproduced bit for
// bit: luminance and the gradient magnitude without FMA contraction (this TU
// is compiled with -ffp-contract=off), correctly rounded sqrtf (hipcc default),
// taps accumulated with one explicit fmaf each in (dy, dx) row-major order.
#include <algorithm>

#include "edge_launch.hpp"

namespace mpx {
using edge::Taps;
using edgel::launch_tiled;
using edgel::make_taps;
namespace {

// ---------------------------------------------------------------------------
// Generic direct kernel: any K <= MPX_MAX_K and any anchor, one output pixel
// per thread straight from global memory. Used for (K, anchor) pairs without a
// tiled instantiation and as the naive baseline in profiles.
// ---------------------------------------------------------------------------
template <int MODE, bool SEP>
__global__ void conv_direct_kernel(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, int w,
                                   int pitch, int oy0, int oy1, int y_lo, int y_hi, int k, int anchor,
                                   Taps taps, edge::RowSrc rs) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = oy0 + blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= w || y >= oy1) return;
    float ax = 0.0f, ay = 0.0f;
    for (int dy = 0; dy < k; ++dy) {
        const int gy = mpx_clampi(y + dy - anchor, y_lo, y_hi);
        const uint32_t *row = (gy < 0 ? rs.up : (gy >= rs.own_rows ? rs.dn : in)) + (int64_t)gy * pitch;
        float hx = 0.0f, hy = 0.0f;  // SEP: horizontal factor sums of this row
        for (int dx = 0; dx < k; ++dx) {
            const float l = mpx_luma(row[mpx_clampi(x + dx - anchor, 0, w - 1)]);
            if constexpr (SEP) {
                hx = fmaf(taps.wx[dx], l, hx);
                if (MODE == MPX_CONV_MAG2) hy = fmaf(taps.wy[dx], l, hy);
            } else {
                ax = fmaf(taps.wx[dy * k + dx], l, ax);
                if (MODE == MPX_CONV_MAG2) ay = fmaf(taps.wy[dy * k + dx], l, ay);
            }
        }
        if constexpr (SEP) {
            ax = fmaf(taps.wx[k + dy], hx, ax);
            if (MODE == MPX_CONV_MAG2) ay = fmaf(taps.wy[k + dy], hy, ay);
        }
    }
    if constexpr (SEP) {
        ax = ax * taps.wx[2 * k];
        if (MODE == MPX_CONV_MAG2) ay = ay * taps.wy[2 * k];
    }
    out[(int64_t)y * pitch + x] = edge::gray_px<MODE, false>(ax, ay, mpx_px_a(in[(int64_t)y * pitch + x]));
}

template <int MODE, bool SEP>
void launch_direct(const uint32_t *in, uint32_t *out, int w, int pitch, int oy0, int oy1, int y_lo, int y_hi, int k,
                   int anchor, const Taps &taps, hipStream_t s, const edge::RowSrc &rs) {
    const dim3 blk(64, 4);
    const dim3 grd((w + 63) / 64, (oy1 - oy0 + 3) / 4);
    hipLaunchKernelGGL((conv_direct_kernel<MODE, SEP>), grd, blk, 0, s, in, out, w, pitch, oy0, oy1, y_lo, y_hi, k,
                       anchor, taps, rs);
}

// separable filters: wave kernel for the centred odd windows, direct otherwise
// (ABS1 separable filters always take the direct kernel: no named filter uses it)
template <int MODE>
int dispatch_sep(const uint32_t *in, uint32_t *out, int w, int pitch, int oy0, int oy1, int y_lo, int y_hi,
                 int k, int anchor, const Taps &taps, bool vec, hipStream_t s, const edge::RowSrc &rs) {
    if constexpr (MODE != MPX_CONV_ABS1) {
        if (k == 3 && anchor == 1) return edgel::launch_sep<3, 1, MODE>(in, out, w, pitch, oy0, oy1, y_lo, y_hi, taps, vec, s, rs);
        if (k == 5 && anchor == 2) return edgel::launch_sep<5, 2, MODE>(in, out, w, pitch, oy0, oy1, y_lo, y_hi, taps, vec, s, rs);
        if (k == 7 && anchor == 3) return edgel::launch_sep<7, 3, MODE>(in, out, w, pitch, oy0, oy1, y_lo, y_hi, taps, vec, s, rs);
    }
    launch_direct<MODE, true>(in, out, w, pitch, oy0, oy1, y_lo, y_hi, k, anchor, taps, s, rs);
    return MPX_OK;
}

template <int MODE>
int dispatch_mode(const uint32_t *in, uint32_t *out, int w, int pitch, int oy0, int oy1, int y_lo, int y_hi,
                  int k, int anchor, const Taps &taps, bool vec, hipStream_t s, const edge::RowSrc &rs) {
    if (k == 2 && anchor == 0) return launch_tiled<2, 0, MODE>(in, out, w, pitch, oy0, oy1, y_lo, y_hi, taps, vec, s, rs);
    if (k == 3 && anchor == 1) return launch_tiled<3, 1, MODE>(in, out, w, pitch, oy0, oy1, y_lo, y_hi, taps, vec, s, rs);
    if (k == 5 && anchor == 2) return launch_tiled<5, 2, MODE>(in, out, w, pitch, oy0, oy1, y_lo, y_hi, taps, vec, s, rs);
    if (k == 7 && anchor == 3) return launch_tiled<7, 3, MODE>(in, out, w, pitch, oy0, oy1, y_lo, y_hi, taps, vec, s, rs);
    launch_direct<MODE, false>(in, out, w, pitch, oy0, oy1, y_lo, y_hi, k, anchor, taps, s, rs);
    return MPX_OK;
}

template <int MODE>
void launch_direct_any(bool sep, const uint32_t *in, uint32_t *out, int w, int pitch, int oy0, int oy1, int y_lo,
                       int y_hi, int k, int anchor, const Taps &taps, hipStream_t s, const edge::RowSrc &rs) {
    if (sep) launch_direct<MODE, true>(in, out, w, pitch, oy0, oy1, y_lo, y_hi, k, anchor, taps, s, rs);
    else launch_direct<MODE, false>(in, out, w, pitch, oy0, oy1, y_lo, y_hi, k, anchor, taps, s, rs);
}

}  // namespace

int conv_impl(const uint32_t *in, uint32_t *out, int w, int pitch, int oy0, int oy1, int y_lo, int y_hi, int k,
              int anchor, int mode, const float *wx, const float *wy, void *stream, bool force_direct,
              edge::RowSrc rs = edge::RowSrc{}) {
    MPX_CHECK_ARG(in && out && wx, "null pointer");
    if (!rs.up) rs.up = in;
    if (!rs.dn) rs.dn = in;
    MPX_CHECK_ARG(rs.own_rows >= 1, "own_rows must be positive");
    MPX_CHECK_ARG(w > 0 && pitch >= w, "bad width/pitch");
    MPX_CHECK_ARG(k >= 1 && k <= MPX_MAX_K && anchor >= 0 && anchor < k, "bad window");
    const bool sep = (mode & MPX_CONV_SEP) != 0;
    // the load-policy hint travels to launch_band through a thread-local (the
    // launch is synchronous in this thread); restored on every return
    const edgel::ResidentHint hint((mode & MPX_CONV_RESIDENT) != 0);
    mode = MPX_CONV_BASE(mode) | (mode & ~(MPX_CONV_SEP | MPX_CONV_RESIDENT | 3));  // any unknown flag fails the range check
    MPX_CHECK_ARG(mode >= MPX_CONV_MAG2 && mode <= MPX_CONV_LIN1, "bad mode");
    MPX_CHECK_ARG(mode != MPX_CONV_MAG2 || wy, "MAG2 needs wy");
    MPX_CHECK_ARG(y_lo <= y_hi && oy0 >= 0, "bad row range");
    if (oy1 <= oy0) return MPX_OK;
    const Taps taps = make_taps(k, wx, wy, mode == MPX_CONV_MAG2, sep);
    // 8-B pair loads/stores of the wave kernel: even width and pitch, 8-B aligned rows
    const bool vec = (w % 2 == 0) && (pitch % 2 == 0) &&
                     ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out) |
                       reinterpret_cast<uintptr_t>(rs.up) | reinterpret_cast<uintptr_t>(rs.dn)) & 7u) == 0;
    hipStream_t s = as_stream(stream);
    int rc;
    if (force_direct) {
        switch (mode) {
            case MPX_CONV_MAG2:
                launch_direct_any<MPX_CONV_MAG2>(sep, in, out, w, pitch, oy0, oy1, y_lo, y_hi, k, anchor, taps, s, rs);
                break;
            case MPX_CONV_ABS1:
                launch_direct_any<MPX_CONV_ABS1>(sep, in, out, w, pitch, oy0, oy1, y_lo, y_hi, k, anchor, taps, s, rs);
                break;
            default:
                launch_direct_any<MPX_CONV_LIN1>(sep, in, out, w, pitch, oy0, oy1, y_lo, y_hi, k, anchor, taps, s, rs);
        }
        rc = MPX_OK;
    } else if (sep) {
        if (mode == MPX_CONV_MAG2)
            rc = dispatch_sep<MPX_CONV_MAG2>(in, out, w, pitch, oy0, oy1, y_lo, y_hi, k, anchor, taps, vec, s, rs);
        else if (mode == MPX_CONV_ABS1)
            rc = dispatch_sep<MPX_CONV_ABS1>(in, out, w, pitch, oy0, oy1, y_lo, y_hi, k, anchor, taps, vec, s, rs);
        else
            rc = dispatch_sep<MPX_CONV_LIN1>(in, out, w, pitch, oy0, oy1, y_lo, y_hi, k, anchor, taps, vec, s, rs);
    } else if (mode == MPX_CONV_MAG2) {
        rc = dispatch_mode<MPX_CONV_MAG2>(in, out, w, pitch, oy0, oy1, y_lo, y_hi, k, anchor, taps, vec, s, rs);
    } else if (mode == MPX_CONV_ABS1) {
        rc = dispatch_mode<MPX_CONV_ABS1>(in, out, w, pitch, oy0, oy1, y_lo, y_hi, k, anchor, taps, vec, s, rs);
    } else {
        rc = dispatch_mode<MPX_CONV_LIN1>(in, out, w, pitch, oy0, oy1, y_lo, y_hi, k, anchor, taps, vec, s, rs);
    }
    if (rc != MPX_OK) return rc;
    MPX_RETURN_IF_HIP_ERROR(hipGetLastError());
    return MPX_OK;
}

MPX_MODULE_ANCHOR(edge)

}  // namespace mpx

extern "C" int mpx_conv(const uint32_t *in, uint32_t *out, int w, int pitch, int oy0, int oy1, int y_lo, int y_hi,
                        int k, int anchor, int mode, const float *wx, const float *wy, void *stream) {
    return mpx::conv_impl(in, out, w, pitch, oy0, oy1, y_lo, y_hi, k, anchor, mode, wx, wy, stream, false);
}

extern "C" int mpx_conv_peer(const uint32_t *in, const uint32_t *in_up, const uint32_t *in_dn, int own_rows,
                             uint32_t *out, int w, int pitch, int oy0, int oy1, int y_lo, int y_hi, int k, int anchor,
                             int mode, const float *wx, const float *wy, void *stream) {
    mpx::edge::RowSrc rs;
    rs.up = in_up;
    rs.dn = in_dn;
    rs.own_rows = own_rows;
    return mpx::conv_impl(in, out, w, pitch, oy0, oy1, y_lo, y_hi, k, anchor, mode, wx, wy, stream, false, rs);
}

extern "C" int mpx_conv_direct(const uint32_t *in, uint32_t *out, int w, int pitch, int oy0, int oy1, int y_lo,
                               int y_hi, int k, int anchor, int mode, const float *wx, const float *wy,
                               void *stream) {
    return mpx::conv_impl(in, out, w, pitch, oy0, oy1, y_lo, y_hi, k, anchor, mode, wx, wy, stream, true);
}


// Minimum image size (pixels) for the band kernel; returns the previous value.
// n < 0 only queries. Tests set 0 to run the band kernel on small images.
// Band kernel mode (MPX_CONV_BAND semantics, 0..4); returns the previous mode.
// m < 0 only queries.
extern "C" int mpx_conv_set_band_mode(int m) {
    if (m < 0 || m > 4) return mpx::edgel::g_band_mode.load();
    return mpx::edgel::g_band_mode.exchange(m);
}

extern "C" long long mpx_conv_set_band_min(long long n) {
    if (n < 0) return mpx::edgel::g_band_min_pixels.load();
    return mpx::edgel::g_band_min_pixels.exchange(n);
}

// The plan launch_band itself follows (edgel::band_plan): host arithmetic only.
extern "C" int mpx_conv_band_plan(int w, int rows, int k, int anchor, int resident, int remote_rows, int *seg,
                                  int *opt) {
    const mpx::edgel::BandPlan p = mpx::edgel::band_plan(w, rows, k, anchor, resident != 0, remote_rows != 0);
    if (seg) *seg = p.seg;
    if (opt) *opt = p.opt;
    return p.kernel;
}
