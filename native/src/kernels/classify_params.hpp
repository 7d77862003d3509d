// lab3 classifier: the parameter structs the host builds (classify_bounds.cpp)
// and the kernels take by value. No HIP; the fields are the kernel-argument layout.
#pragma once

#include <cstdint>

#include "mpx/common.h"

namespace mpx {

struct ClassParams {
    double mu[MPX_MAX_CLASSES * 3];
    double A[MPX_MAX_CLASSES * 9];
};

constexpr int kFeat = 10;

struct FastParams {
    float w[MPX_MAX_CLASSES][kFeat];  // expanded weights incl. bias; padded classes: 0 ... 0, 3e38
    float T2;                         // decision margin 2 * max_c tol_c
};

struct Fast64Params {
    double w[MPX_MAX_CLASSES][kFeat];  // padded classes: 0 ... 0, 1e300
    double T2;                         // decision margin 2 * max_c tol_c
};

struct I8Params {
    uint64_t a[MPX_MAX_CLASSES][2];  // hi limbs: [class][half] = 8 int8 weights of k = 8 half .. +7
    uint64_t b[MPX_MAX_CLASSES][2];  // lo limbs
    int32_t c[MPX_MAX_CLASSES];      // round(w9 / u); padded classes: 2^26 - 64 (never the argmin)
    int32_t T2;                      // decision margin in key units (key >> 5)
};

constexpr int kHalfMfmas = 3;  // MFMAs per 16-class set

struct HalfParams {
    uint32_t w[2][kHalfMfmas][16][4];  // [set][mfma][class in set]: 8 f16 slot weights (the A row)
    float c[MPX_MAX_CLASSES];          // accumulator init: scaled constant + bias; padded classes 3e38
    float T2;                          // decision margin (scaled units; the FAST32 test)
};

}  // namespace mpx
