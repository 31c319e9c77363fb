// The decimal rounding of label text, shared by every kernel that writes KITTI fields (result2kitti.hip, recombine.hip).
// Files that include it are built with -ffp-contract=off: the one fused operation is the explicit fma below.
#pragma once
#include <math.h>

#include <hip/hip_runtime.h>

namespace sgv3d {

// CPython's round(v, 4), bit for bit: the double nearest to the decimal that v rounds to, decimal ties (which need an
// exactly representable v * 1e4 = k + 0.5) to even.  p = v * 1e4 is rounded, so a p that lands on k + 0.5 may come from
// a v on either side of the tie: e = fma(v, 1e4, -p) is the exact residual v * 1e4 - p and its sign says which.  Only
// e == 0 is a true tie, which rint resolves to even as Python does.  n / 1e4 is correctly rounded and n, 1e4 are exact,
// so the quotient is the double nearest to the decimal n * 1e-4, which is what Python's dtoa-based round returns.  rint
// keeps the sign of zero (round(-1e-5, 4) = -0.0).
__host__ __device__ inline double round4(double v) {
    const double p = v * 1e4;
    const double e = fma(v, 1e4, -p);
    double n = rint(p);
    if (fabs(p - n) == 0.5 && e != 0.0) n = floor(p) + (e > 0.0 ? 1.0 : 0.0);
    return n / 1e4;
}

}  // namespace sgv3d
