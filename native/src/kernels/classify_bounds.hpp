// lab3 classifier, host only (native/src/core/classify_bounds.cpp, no HIP):
// the proven decision margins of the fp32 / fp64 / int8 / f16 paths and the
// path choice, so that they compile, run and sanitize on any host.
#pragma once

#include "classify_params.hpp"

namespace mpx {

// Parameters of one path with a bound on |computed - reference fp64 chain|
// proven for every pixel in [0, 255]^3; false when no bound can be proven.
bool build_fast(int nc, const double *mu, const double *inv, FastParams &fp);
bool build_fast64(int nc, const double *mu, const double *inv, Fast64Params &fp);
bool build_i8(int nc, const double *mu, const double *inv, I8Params &ip);
bool build_half(int nc, const double *mu, const double *inv, HalfParams &hp);

// The path AUTO (or an explicit path) resolves to for these statistics, with
// the parameters that path needs built; DIRECT when no fp32 / int bound exists.
struct Resolved {
    int chosen;
    FastParams fp;
    Fast64Params fp64;
    I8Params ip8;
    HalfParams hp;
};
Resolved classify_resolve(int nc, const double *mu, const double *inv, int path, bool aligned);
float classify_margin(const Resolved &r);  // of the chosen path, as mpx_classify_plan reports it

}  // namespace mpx
