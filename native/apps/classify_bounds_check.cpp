// Stand-alone check of the classifier's host bounds (classify_bounds.cpp, no
// HIP): resolves a handful of fixed class statistics on every path and prints
// which builders succeed, the path taken and its margin. Provable statistics
// must build on every path; degenerate ones (a non-finite mean, an indefinite
// matrix, magnitudes near the fp32 range) must be refused and resolve to
// DIRECT. The fp64 builder (explicit "mfma64" only) legitimately holds at
// magnitudes that are out of range for fp32 alone; that case is printed and
// not counted as a refusal. Built with ASan/UBSan under MPX_HOST_SANITIZE.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../src/kernels/classify_bounds.hpp"

namespace {

struct Case {
    const char *name;
    int nc;
    std::vector<double> mu, inv;
    bool provable;
};

Case make_case(const char *name, int nc, bool provable) {
    Case c{name, nc, std::vector<double>(3 * nc), std::vector<double>(9 * nc, 0.0), provable};
    for (int k = 0; k < nc; ++k) {
        const double t = nc > 1 ? (double)k / (nc - 1) : 0.5;
        c.mu[3 * k + 0] = 20.0 + 215.0 * t;
        c.mu[3 * k + 1] = 235.0 - 200.0 * t;
        c.mu[3 * k + 2] = 40.0 + 7.0 * (k % 5) + 100.0 * t;
        double *A = &c.inv[9 * k];
        A[0] = 0.020 + 0.001 * k;
        A[4] = 0.030 - 0.0005 * k;
        A[8] = 0.025;
        A[1] = A[3] = 0.004;   // symmetric part
        A[2] = 0.003;          // and an asymmetric pair: the bounds symmetrise
        A[6] = 0.001;
    }
    return c;
}

const char *kPathName[7] = {"direct", "mfma", "auto", "fast", "mfma64", "mfma8", "mfma16"};

}  // namespace

int main() {
    std::vector<Case> cases;
    cases.push_back(make_case("two separated classes", 2, true));
    cases.push_back(make_case("32 classes", 32, true));
    cases.push_back(make_case("non-finite mean", 3, false));
    cases.back().mu[4] = NAN;
    cases.push_back(make_case("indefinite matrix", 3, false));
    cases.back().inv[9 + 4] = -0.03;
    cases.push_back(make_case("near fp32 range", 3, false));
    for (double &a : cases.back().inv) a *= 1e35;

    int built = 0, refused = 0, nprov = 0, ndeg = 0;
    for (const Case &c : cases) {
        const double *mu = c.mu.data(), *inv = c.inv.data();
        mpx::FastParams fp;
        mpx::Fast64Params fp64;
        mpx::I8Params ip;
        mpx::HalfParams hp;
        const bool ok32 = mpx::build_fast(c.nc, mu, inv, fp), ok64 = mpx::build_fast64(c.nc, mu, inv, fp64),
                   ok8 = mpx::build_i8(c.nc, mu, inv, ip), ok16 = mpx::build_half(c.nc, mu, inv, hp);
        std::printf("%s (nc = %d): builders fast %d fast64 %d i8 %d half %d\n", c.name, c.nc, ok32, ok64, ok8, ok16);
        bool good = c.provable ? ok32 && ok64 && ok8 && ok16 : !ok32 && !ok8 && !ok16;
        for (int path = MPX_CLS_DIRECT; path <= MPX_CLS_MFMA16; ++path) {
            const mpx::Resolved r = mpx::classify_resolve(c.nc, mu, inv, path, true);
            const mpx::Resolved again = mpx::classify_resolve(c.nc, mu, inv, path, true);  // from the cache
            const bool same = std::memcmp(&r, &again, sizeof(r)) == 0;
            std::printf("  %-6s -> %-6s margin %.9g%s\n", kPathName[path], kPathName[r.chosen],
                        (double)mpx::classify_margin(r), same ? "" : "  CACHE MISMATCH");
            int want = MPX_CLS_DIRECT;
            if (c.provable)
                want = path != MPX_CLS_AUTO ? path : c.nc >= 4 ? MPX_CLS_MFMA16 : MPX_CLS_FAST;
            else if (path == MPX_CLS_MFMA64 && ok64)
                want = MPX_CLS_MFMA64;
            good = good && same && r.chosen == want;
            if (r.chosen != MPX_CLS_DIRECT && !(mpx::classify_margin(r) > 0)) good = false;
        }
        // an unaligned image takes DIRECT whatever the statistics
        good = good && mpx::classify_resolve(c.nc, mu, inv, MPX_CLS_AUTO, false).chosen == MPX_CLS_DIRECT;
        (c.provable ? nprov : ndeg) += 1;
        (c.provable ? built : refused) += good ? 1 : 0;
    }
    std::printf("summary: provable built %d/%d, degenerate refused to direct %d/%d\n", built, nprov, refused, ndeg);
    return built == nprov && refused == ndeg ? 0 : 1;
}
