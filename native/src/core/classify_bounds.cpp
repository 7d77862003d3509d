// lab3 classifier, host only: expanded weights and the rigorous decision
// margins of every proven path, the path choice and the cache of resolved
// parameters (see the header of native/src/kernels/classify.hip).
#include "../kernels/classify_bounds.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <vector>

namespace mpx {
namespace {

typedef long double ld;

// |q_i q_j| <= 128^2, |q_i| <= 128 for q = p - 128, p in [0, 255]^3
constexpr ld kPhiMax[kFeat] = {16384, 16384, 16384, 16384, 16384, 16384, 128, 128, 128, 1};

// Expanded weights w[c][k] of the centred quadratic form, the reference
// chain's own error bound refb[c] and the indefiniteness slack psd[c].
struct Expanded {
    ld w[MPX_MAX_CLASSES][kFeat], refb[MPX_MAX_CLASSES], psd[MPX_MAX_CLASSES];
};

// False for non-finite statistics or a symmetrised A that is not positive definite.
bool expand_classes(int nc, const double *mu, const double *inv, Expanded &e) {
    const ld u64 = std::ldexp((ld)1, -53);
    for (int c = 0; c < nc; ++c) {
        const double *A = inv + 9 * c;
        const double *mraw = mu + 3 * c;
        for (int i = 0; i < 3; ++i)
            if (!std::isfinite(mraw[i])) return false;
        const ld m[3] = {(ld)mraw[0] - 128, (ld)mraw[1] - 128, (ld)mraw[2] - 128};  // centred mean (exact)
        for (int i = 0; i < 9; ++i)
            if (!std::isfinite(A[i])) return false;
        ld S[3][3];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) S[i][j] = ((ld)A[3 * i + j] + (ld)A[3 * j + i]) / 2;
        // positive definiteness (Cholesky pivots): Q_c >= 0 keeps biased values positive
        const ld p0 = S[0][0];
        if (!(p0 > 0)) return false;
        const ld l10 = S[1][0] / p0, l20 = S[2][0] / p0;
        const ld p1 = S[1][1] - l10 * S[1][0];
        if (!(p1 > 0)) return false;
        const ld l21 = (S[2][1] - l20 * S[1][0]) / p1;
        const ld p2 = S[2][2] - l20 * S[2][0] - l21 * (S[2][1] - l20 * S[1][0]);
        if (!(p2 > 0)) return false;
        ld Sm[3], sabs = 0, dmax[3];
        for (int i = 0; i < 3; ++i) {
            Sm[i] = S[i][0] * m[0] + S[i][1] * m[1] + S[i][2] * m[2];
            dmax[i] = std::fmax(std::fabs((ld)mraw[i]), std::fabs(255 - (ld)mraw[i])) * (1 + 4 * u64);
        }
        ld *w = e.w[c];
        w[0] = S[0][0];
        w[1] = S[1][1];
        w[2] = S[2][2];
        w[3] = 2 * S[0][1];
        w[4] = 2 * S[0][2];
        w[5] = 2 * S[1][2];
        w[6] = -2 * Sm[0];
        w[7] = -2 * Sm[1];
        w[8] = -2 * Sm[2];
        w[9] = m[0] * Sm[0] + m[1] * Sm[1] + m[2] * Sm[2];
        // reference fp64 chain: |computed - exact| <= ~8 u sum |A_ij| |d_i| |d_j|; 16 u for margin
        ld aq = 0;
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                aq += std::fabs((ld)A[3 * i + j]) * dmax[i] * dmax[j];
                sabs += std::fabs(S[i][j]);
            }
        e.refb[c] = 16 * u64 * aq;
        // a slightly indefinite S hidden by long-double rounding: Q >= -1e-15 |S| |d|^2
        e.psd[c] = 1e-15L * sabs * (dmax[0] * dmax[0] + dmax[1] * dmax[1] + dmax[2] * dmax[2]);
    }
    return true;
}

// The margin a kernel tests against: 2 tmax (1 + 2^-slack) (see decided()),
// rounded up to the kernel's type.
template <typename T>
T margin_up(ld tmax, int slack) {
    const ld t2x = 2 * tmax * (1 + std::ldexp((ld)1, -slack));
    T t2 = (T)t2x;
    if ((ld)t2 < t2x) t2 = std::nextafter(t2, (T)INFINITY);
    return t2;
}

// The positivity bias and the bound with it, in two passes: tol(c, bias,
// store) is class c's bound with `bias` added to its constant term (and
// stores that class's parameters when asked). The bias is 4 x the largest
// unbiased bound; false when it does not stay above 2 x the biased one.
template <typename Tol>
bool biased_bound(int nc, Tol tol, ld &bias, ld &tmax) {
    ld tmax0 = 0;
    for (int c = 0; c < nc; ++c) tmax0 = std::fmax(tmax0, tol(c, 0, false));
    bias = 4 * tmax0;
    tmax = 0;
    for (int c = 0; c < nc; ++c) tmax = std::fmax(tmax, tol(c, bias, true));
    return bias > 2 * tmax;
}

}  // namespace

// false when the fp32 decision cannot be proven (non-finite statistics, a
// symmetrised A that is not positive definite, or magnitudes near fp32 range)
bool build_fast(int nc, const double *mu, const double *inv, FastParams &fp) {
    const ld u32 = std::ldexp((ld)1, -24);
    const ld g10 = 10 * u32 / (1 - 10 * u32);
    const ld *phimax = kPhiMax;
    Expanded e;
    if (!expand_classes(nc, mu, inv, e)) return false;
    auto tol = [&](int c, ld bias, bool store) -> ld {
        ld mag = 0, rep = 0, ev = 0;
        for (int k = 0; k < kFeat; ++k) {
            const ld wk = e.w[c][k] + (k == 9 ? bias : 0);
            const float f = (float)wk;
            if (store) fp.w[c][k] = f;
            rep += std::fabs((ld)f - wk) * phimax[k];
            ev += std::fabs((ld)f) * phimax[k];
            mag += std::fabs(wk) * phimax[k];
        }
        // fp32 chain + weight rounding + long-double arithmetic slack + reference chain
        return (g10 * ev + rep + 1e-15L * mag + e.refb[c] + e.psd[c]) * 1.001L + 1e-30L;
    };
    ld mag = 0;
    for (int c = 0; c < nc; ++c)
        for (int k = 0; k < kFeat; ++k) mag = std::fmax(mag, std::fabs(e.w[c][k]) * phimax[k]);
    if (!(mag < 1e30L)) return false;
    ld bias, tmax;
    if (!biased_bound(nc, tol, bias, tmax)) return false;
    for (int c = nc; c < MPX_MAX_CLASSES; ++c)
        for (int k = 0; k < kFeat; ++k) fp.w[c][k] = (k == 9) ? 3.0e38f : 0.0f;
    fp.T2 = margin_up<float>(tmax, 20);
    return true;
}

// fp64 weights for MFMA64. The f64 MFMA's summation order and internal
// rounding are not specified, so its error is bounded as any 12-term sum with
// unit roundoff 2^-52 (twice RNE's, covering a truncating adder):
// gamma_12 sum_k |w_k| phimax_k, plus the weight rounding and the reference
// chain's error; a pixel is decided in fp64 only beyond 2 max_c tol_c.
bool build_fast64(int nc, const double *mu, const double *inv, Fast64Params &fp) {
    const ld u = std::ldexp((ld)1, -52);
    const ld g12 = 12 * u / (1 - 12 * u);
    Expanded e;
    if (!expand_classes(nc, mu, inv, e)) return false;
    ld tmax = 0;
    for (int c = 0; c < nc; ++c) {
        ld ev = 0, rep = 0, mag = 0;
        for (int k = 0; k < kFeat; ++k) {
            const double f = (double)e.w[c][k];
            fp.w[c][k] = f;
            ev += std::fabs((ld)f) * kPhiMax[k];
            rep += std::fabs((ld)f - e.w[c][k]) * kPhiMax[k];
            mag += std::fabs(e.w[c][k]) * kPhiMax[k];
        }
        if (!(mag < 1e300L)) return false;
        // long-double expansion slack: ~20 operations at 2^-64 each
        const ld t = (g12 * ev + rep + 1e-17L * mag + e.refb[c]) * 1.001L + 1e-300L;
        tmax = std::fmax(tmax, t);
    }
    for (int c = nc; c < MPX_MAX_CLASSES; ++c)
        for (int k = 0; k < kFeat; ++k) fp.w[c][k] = (k == 9) ? 1e300 : 0.0;
    fp.T2 = margin_up<double>(tmax, 40);
    return true;
}

// Integer weights for MFMA8 (see the kernel): slot weights V_s as
// v_s = round(V_s / u) with |v_s| <= 32639 (two int8 limbs), the constant as
// c = round(w9 / u) in the accumulator; u is doubled until every key fits
// int32 after the 5-bit class tag (|sum_s Fmax_s |v_s|| + |c| < 2^26). The
// decision bound per class: u/2 per unit of feature magnitude (weight
// rounding; the int32 arithmetic is exact) + u/2 (constant) + the reference
// chain's error; T2 = ceil(2 max_c tol_c / u) + 1 in key units.
constexpr int kSlots = 16;
// slot -> (expanded weight index, scale, max |feature|)
constexpr int kSlotW[kSlots] = {0, 1, 2, 3, 4, 5, 6, 7, 0, 1, 2, 3, 4, 5, 8, -1};
constexpr ld kSlotScale[kSlots] = {256, 256, 256, 256, 256, 256, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0};
constexpr ld kSlotFmax[kSlots] = {64, 64, 64, 64, 64, 64, 128, 128, 128, 128, 128, 128, 128, 128, 128, 0};

bool build_i8(int nc, const double *mu, const double *inv, I8Params &ip) {
    Expanded e;
    if (!expand_classes(nc, mu, inv, e)) return false;
    const auto &w = e.w;
    ld vmax = 0, mag = 0;
    for (int c = 0; c < nc; ++c)
        for (int s = 0; s < kSlots; ++s)
            if (kSlotW[s] >= 0) {
                vmax = std::fmax(vmax, std::fabs(w[c][kSlotW[s]] * kSlotScale[s]));
                mag = std::fmax(mag, std::fabs(w[c][kSlotW[s]]) * kPhiMax[kSlotW[s]]);
            }
    if (!(vmax > 0) || !(mag < 1e30L)) return false;
    // The decision bound uses the weights' ACTUAL rounding errors (round 5):
    // per class, u (sum_s |delta_cs| Fmax_s + |delta_c|) with delta = the
    // integer minus the exact scaled weight, instead of the worst case u / 2
    // per unit — and the scale u is chosen among 64 candidates (up to +25 %) above the
    // smallest that fits for the smallest margin in value units (T2 u), so
    // fewer pixels fall inside it and take the exact fallback.
    long long v[MPX_MAX_CLASSES][kSlots], cc[MPX_MAX_CLASSES];
    auto fits_at = [&](ld u, long long (*vv)[kSlots], long long *cv) -> bool {
        for (int c = 0; c < nc; ++c) {
            ld tot = 0;
            for (int s = 0; s < kSlots; ++s) {
                vv[c][s] = kSlotW[s] >= 0 ? std::llround(w[c][kSlotW[s]] * kSlotScale[s] / u) : 0;
                if (std::llabs(vv[c][s]) > 32639) return false;
                tot += kSlotFmax[s] * (ld)std::llabs(vv[c][s]);
            }
            const ld cw = w[c][9] / u;
            if (!(std::fabs(cw) < (ld)(1 << 26))) return false;
            cv[c] = std::llround(cw);
            tot += (ld)std::llabs(cv[c]);
            if (!(tot < (ld)(1 << 26) - 64)) return false;  // key = ((D_a << 8) + D_b) << 5 | tag
        }
        return true;
    };
    // margin in key units at scale u (the integers already in vv / cv)
    auto t2_at = [&](ld u, long long (*vv)[kSlots], const long long *cv) -> ld {
        ld tmax = 0;
        for (int c = 0; c < nc; ++c) {
            ld q = std::fabs((ld)cv[c] - w[c][9] / u);  // constant rounding, <= 1/2
            for (int s = 0; s < kSlots; ++s)
                if (kSlotW[s] >= 0) q += kSlotFmax[s] * std::fabs((ld)vv[c][s] - w[c][kSlotW[s]] * kSlotScale[s] / u);
            // weight + constant rounding (exact integer arithmetic otherwise) + reference chain + long-double slack
            const ld t = (u * q + e.refb[c] + e.psd[c] + 1e-15L * mag * 16) * 1.001L + u * 1e-6L;
            tmax = std::fmax(tmax, t);
        }
        return std::ceil(2 * tmax / u) + 1;
    };
    ld u0 = vmax / 32639;
    for (int attempt = 0;; ++attempt) {
        if (attempt > 60) return false;
        if (fits_at(u0, v, cc)) break;
        u0 *= 2;
    }
    ld best_u = u0, t2 = t2_at(u0, v, cc);
    {
        long long vv[MPX_MAX_CLASSES][kSlots], cv[MPX_MAX_CLASSES];
        for (int k = 1; k < 64; ++k) {
            const ld u = u0 * (1 + (ld)k / 256);
            if (!fits_at(u, vv, cv)) continue;
            const ld t = t2_at(u, vv, cv);
            if (t * u < t2 * best_u) {
                best_u = u;
                t2 = t;
                std::memcpy(v, vv, sizeof(v));
                std::memcpy(cc, cv, sizeof(cc));
            }
        }
    }
    if (!(t2 < (ld)(1 << 24))) return false;  // nothing would ever be decided
    ip.T2 = (int32_t)t2;
    for (int c = 0; c < MPX_MAX_CLASSES; ++c) {
        for (int hf = 0; hf < 2; ++hf) {
            uint64_t pa = 0, pb = 0;
            for (int j = 0; j < 8; ++j) {
                const int s = 8 * hf + j;
                long long a8 = 0, b8 = 0;
                if (c < nc) {
                    const long long x = v[c][s];
                    a8 = (x + 128) >> 8;  // floor: x = 256 a + b with b in [-128, 127]
                    b8 = x - 256 * a8;
                }
                pa |= (uint64_t)(uint8_t)(int8_t)a8 << (8 * j);
                pb |= (uint64_t)(uint8_t)(int8_t)b8 << (8 * j);
            }
            ip.a[c][hf] = pa;
            ip.b[c][hf] = pb;
        }
        ip.c[c] = c < nc ? (int32_t)cc[c] : (1 << 26) - 64;  // above every real key: never the argmin
    }
    return true;
}

// x rounded to the nearest f16 (ties to even); 0 below the normal range (the
// kernel sees no f16 subnormals) and false on overflow
static bool f16_round(ld x, ld &r, uint16_t &bits) {
    r = 0;
    bits = 0;
    if (x == 0) return true;
    const ld a = std::fabs(x);
    int ex;
    std::frexp(a, &ex);  // a = f 2^ex, f in [0.5, 1): normal f16 exponent E = ex - 1
    if (ex - 1 < -14) return true;
    const ld quantum = std::ldexp((ld)1, ex - 11);
    ld m = std::nearbyint(a / quantum) * quantum;
    std::frexp(m, &ex);
    if (!(m <= (ld)65504)) return false;
    const int E = ex - 1;
    const uint32_t mant = (uint32_t)std::llround((m / std::ldexp((ld)1, E) - 1) * 1024);
    bits = (uint16_t)(((x < 0) ? 0x8000u : 0u) | ((uint32_t)(E + 15) << 10) | mant);
    r = x < 0 ? -m : m;
    return true;
}

// f16 limbs for MFMA16 (see the kernel): every expanded weight times a common
// power of two 2^e (the largest in [2^13, 2^14)) as hi + lo f16. The bound per
// class, in scaled units: the limb rounding against the exact weight (per
// unit of feature: 16384 for the h slots, 4 for the l slots, which take hi
// only, 128 for the channels), the fp32 accumulator's rounding as any sum of
// 25 terms (24 exact products + the constant) with unit roundoff 2^-23 (twice
// RNE's: covers any internal order and a truncating adder), the constant's
// own fp32 rounding, and the reference fp64 chain's error.
bool build_half(int nc, const double *mu, const double *inv, HalfParams &hp) {
    Expanded e;
    if (!expand_classes(nc, mu, inv, e)) return false;
    const auto &w = e.w;
    ld wmax = 0, mag = 0;
    for (int c = 0; c < nc; ++c)
        for (int k = 0; k < kFeat; ++k) {
            if (k < 9) wmax = std::fmax(wmax, std::fabs(w[c][k]));
            mag = std::fmax(mag, std::fabs(w[c][k]) * kPhiMax[k]);
        }
    if (!(wmax > 0) || !(mag < 1e30L)) return false;
    int ex;
    std::frexp(wmax, &ex);
    const ld scale = std::ldexp((ld)1, 14 - ex);  // wmax * scale in [2^13, 2^14)
    // expanded weight of each quadratic slot j (rr gg bb rb rg bg) and its feature bound
    constexpr int kQuad[6] = {0, 1, 2, 4, 3, 5};
    const ld u = std::ldexp((ld)1, -23);
    const ld g25 = 25 * u / (1 - 25 * u);
    ld hi[MPX_MAX_CLASSES][9], lo[MPX_MAX_CLASSES][9];
    uint16_t hb[MPX_MAX_CLASSES][9], lb[MPX_MAX_CLASSES][9];
    ld base_tol[MPX_MAX_CLASSES], base_abs[MPX_MAX_CLASSES];
    for (int c = 0; c < nc; ++c) {
        ld rep = 0, abs_terms = 0;
        for (int k = 0; k < 9; ++k) {
            const ld x = w[c][k] * scale;
            if (!f16_round(x, hi[c][k], hb[c][k])) return false;
            if (!f16_round(x - hi[c][k], lo[c][k], lb[c][k])) return false;
            const ld dev = std::fabs(hi[c][k] + lo[c][k] - x);
            if (k < 6) {
                rep += dev * 16384 + std::fabs(lo[c][k]) * 4;
                abs_terms += (std::fabs(hi[c][k]) + std::fabs(lo[c][k])) * 16384 + std::fabs(hi[c][k]) * 4;
            } else {
                rep += dev * 128;
                abs_terms += (std::fabs(hi[c][k]) + std::fabs(lo[c][k])) * 128;
            }
        }
        base_tol[c] = rep + (e.refb[c] + e.psd[c] + 1e-15L * mag) * scale;
        base_abs[c] = abs_terms;
    }
    // the accumulator input of class c with a positivity bias, and its bound
    auto tol = [&](int c, ld bias, bool store) -> ld {
        const ld cx = w[c][9] * scale + bias;
        const float cf = (float)cx;
        if (store) hp.c[c] = cf;
        const ld acc = g25 * (base_abs[c] + std::fabs((ld)cf));
        return (base_tol[c] + acc + std::fabs((ld)cf - cx)) * 1.001L + 1e-30L;
    };
    ld bias, tmax;
    if (!biased_bound(nc, tol, bias, tmax)) return false;
    if (!(mag * scale + bias < 1e37L)) return false;
    for (int c = nc; c < MPX_MAX_CLASSES; ++c) hp.c[c] = 3.0e38f;
    std::memset(hp.w, 0, sizeof(hp.w));
    for (int c = 0; c < nc; ++c) {
        uint16_t h[kHalfMfmas][8];
        for (int j = 0; j < 6; ++j) {
            h[0][j] = hb[c][kQuad[j]];  // B1: h slots x hi
            h[1][j] = lb[c][kQuad[j]];  // B1: h slots x lo
            h[2][j] = hb[c][kQuad[j]];  // B3: l slots x hi
        }
        h[0][6] = hb[c][6];  // B1: r, g (hi)
        h[0][7] = hb[c][7];
        h[1][6] = lb[c][6];  // B1: r, g (lo)
        h[1][7] = lb[c][7];
        h[2][6] = hb[c][8];  // B3: b, b (hi, lo)
        h[2][7] = lb[c][8];
        for (int j = 0; j < kHalfMfmas; ++j)
            for (int d = 0; d < 4; ++d)
                hp.w[c / 16][j][c % 16][d] = (uint32_t)h[j][2 * d] | ((uint32_t)h[j][2 * d + 1] << 16);
    }
    hp.T2 = margin_up<float>(tmax, 20);
    return true;
}

// Explicit paths and AUTO below kAutoMfma16MinClasses: FAST32 under AUTO, or
// DIRECT when no decision bound can be proven for these statistics. The fp32
// MFMA form (MFMA) never wins: the f32 MFMA and the f32 VALU share one
// datapath on gfx950 — SQ_VALU_MFMA_BUSY_CYCLES and the VALU issue cycles ADD
// UP to the kernel time (nc = 4: 132 vs 546 us, nc = 32: 677 vs 689 us at
// 8192^2; profiles/lab3_classify.md).
static int classify_choose(int path, bool fast_ok) {
    if (path == MPX_CLS_DIRECT || !fast_ok) return MPX_CLS_DIRECT;
    if (path == MPX_CLS_AUTO) return MPX_CLS_FAST;
    return path;
}

// AUTO: MFMA16 from 4 classes, FAST32 below, each where its statistics
// permit a bound (else FAST32, then DIRECT). Round 6, 8192^2, three rotated
// images, host marshalling included, median µs of three alternated rounds on
// one box (profiles/raw/r6/lab3/, profiles/lab3_classify.md):
//   nc        1    2    3    4    5    8    12   16   24   32
//   mfma16   118  113  122  121  125  141  158  174  251  286
//   mfma8    110  112  116  120  146  176  232  277  322  392
//   fast      97  106  117  127  146  187  237  297  415  531
// A second box (profiles/raw/r6/inwave/) ordered fast32 / mfma16 the same
// way at 1-4 classes (99 / 131, 104 / 117, 116 / 121, 125 / 120). Below 4
// classes FAST32 needs no fix-up launch and no MFMA; from 4 MFMA16 wins, by
// 14-46 % from 5. MFMA8 never wins by more than the spread of its
// neighbours, so AUTO does not take it (explicit "mfma8" still runs it).
constexpr int kAutoMfma16MinClasses = 4;

static void resolve_uncached(int nc, const double *mu, const double *inv, int path, bool aligned, Resolved &r) {
    r.chosen = MPX_CLS_DIRECT;
    if (path == MPX_CLS_DIRECT || !aligned) return;
    // mfma8 re-ranks its undecided pixels in fp32 first: its FastParams too
    // (T2 = +inf when the fp32 bound cannot be proven: the fp64 chain then
    // takes every undecided pixel)
    auto fp_for_i8 = [&] {
        if (!build_fast(nc, mu, inv, r.fp)) r.fp.T2 = INFINITY;
    };
    if (path == MPX_CLS_AUTO && nc >= kAutoMfma16MinClasses && build_half(nc, mu, inv, r.hp)) {
        fp_for_i8();
        r.chosen = MPX_CLS_MFMA16;
        return;
    }
    const bool ok = path == MPX_CLS_MFMA64   ? build_fast64(nc, mu, inv, r.fp64)
                    : path == MPX_CLS_MFMA8  ? build_i8(nc, mu, inv, r.ip8)
                    : path == MPX_CLS_MFMA16 ? build_half(nc, mu, inv, r.hp)
                                             : build_fast(nc, mu, inv, r.fp);
    if ((path == MPX_CLS_MFMA8 || path == MPX_CLS_MFMA16) && ok) fp_for_i8();
    r.chosen = classify_choose(path, ok);
}

// Resolved parameters of recent (statistics, path) pairs: a classifier is
// typically run many times with one set of class statistics (the benchmark
// loops, the slab models), and proving the int8 bound (a search over 256
// weight scales) costs ~1 ms of host time at 32 classes — more than the
// kernel. A small most-recently-used list keyed by the exact bytes.
Resolved classify_resolve(int nc, const double *mu, const double *inv, int path, bool aligned) {
    struct ResolvedEntry {
        int nc, path;
        bool aligned;
        double mu[MPX_MAX_CLASSES * 3], inv[MPX_MAX_CLASSES * 9];
        Resolved r;
    };
    static std::mutex mtx;
    static std::vector<std::unique_ptr<ResolvedEntry>> cache;  // most recent first
    constexpr size_t kCap = 16;
    {
        std::lock_guard<std::mutex> lk(mtx);
        for (size_t i = 0; i < cache.size(); ++i) {
            const ResolvedEntry &e = *cache[i];
            if (e.nc == nc && e.path == path && e.aligned == aligned &&
                std::memcmp(e.mu, mu, sizeof(double) * 3 * nc) == 0 &&
                std::memcmp(e.inv, inv, sizeof(double) * 9 * nc) == 0) {
                std::rotate(cache.begin(), cache.begin() + (std::ptrdiff_t)i, cache.begin() + (std::ptrdiff_t)i + 1);
                return cache[0]->r;
            }
        }
    }
    auto e = std::make_unique<ResolvedEntry>();  // zeroed: a path's unused parameter sets stay defined
    resolve_uncached(nc, mu, inv, path, aligned, e->r);
    e->nc = nc;
    e->path = path;
    e->aligned = aligned;
    std::memcpy(e->mu, mu, sizeof(double) * 3 * nc);
    std::memcpy(e->inv, inv, sizeof(double) * 9 * nc);
    const Resolved r = e->r;
    std::lock_guard<std::mutex> lk(mtx);
    cache.insert(cache.begin(), std::move(e));
    if (cache.size() > kCap) cache.pop_back();
    return r;
}

float classify_margin(const Resolved &r) {
    return r.chosen == MPX_CLS_MFMA8    ? (float)r.ip8.T2  // in key units
           : r.chosen == MPX_CLS_MFMA16 ? r.hp.T2
           : r.chosen == MPX_CLS_MFMA64 ? (float)r.fp64.T2
           : r.chosen == MPX_CLS_DIRECT ? 0.0f
                                        : r.fp.T2;
}

}  // namespace mpx
