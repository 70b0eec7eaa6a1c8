// pgmg_vort_dev.h — what the transport passes share (k_vort_step, pgmg_vorticity.hip;
// k_bouss_step, pgmg_boussinesq.hip): a lane's share of one row and the wave maximum of the
// velocity bound.  Device only.
#pragma once
#include "pgmg_grad_dev.h"
#include "pgmg_real.h"

namespace pgmg {

using VD2 = V2<double>;

// a lane's share of one row: its pair, and the one value an edge lane loads beside it (lane 0
// the column left of its pair -- column 0 for the first lane --, lane 63 the column right of it)
struct VRow {
    VD2 o;
    double e;
};

// the maximum of one non-negative double over the 64 lanes of a wave (wave_sum's moves; a lane
// without a source reads 0).  All 64 lanes must be active
__device__ __forceinline__ double wave_max(double v)
{
    v = fmax(v, dpp64<0x111>(v));
    v = fmax(v, dpp64<0x112>(v));
    v = fmax(v, dpp64<0x114>(v));
    v = fmax(v, dpp64<0x118>(v));
    return fmax(fmax(readlane64(v, 15), readlane64(v, 31)), fmax(readlane64(v, 47), readlane64(v, 63)));
}

}  // namespace pgmg
