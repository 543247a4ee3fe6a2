// One step of the S13 fold, shared by the folds that promise its bits: the fused forms (as_fused.hip) and
// late-interaction search (as_maxsim.hip).  Device code only.
#pragma once

namespace as {

// One step of S13 for one position: every product and every sum rounded once, never contracted into an FMA.  (The pragma holds
// from here to the end of the including file: whatever floating-point arithmetic follows it there is not contracted either.)
#pragma clang fp contract(off)
template <int MODE>
__device__ __forceinline__ double fused_step(double f, double wj, double s, bool have) {
    const double t = wj * s;
    if (!have) return t;
    if (MODE == 0) return f + t;
    return (t > f || f != f) ? t : f;   // the first largest term wins; a NaN never displaces a number
}

}  // namespace as
