// Signed depth of one bead below the lamina of one volumetric map: the report's reading of
// the voxel record that exp_map_key.h reads for the A-step (include/igm_hip.h,
// igm_report_map_levels).  The translation unit is built with -ffp-contract=off: the value
// is the header's expression operation by operation.
//   voxel  = rint((x - origin) / grid)   f32 coordinate, float64 map geometry, half to even;
//            clamped to [0, n - 1] per axis, and a clamped bead counts as outside
//   L      = e * grid + origin           centre of the record's nearest lamina voxel e
//   dist   = sqrt_rn((t0^2 + t2^2) + t1^2), t = x - L: exp_map_key's summation order
//   depth  = +dist in the grid on a voxel with w != 0, else -dist
// The clamp is made on the double, so no coordinate (NaN and inf included: both land on
// voxel 0 or n - 1 and count as outside) reads a voxel outside the map.
#pragma once
#include "exact_math.h"
#include "mstep_common.h"

namespace igm {

__device__ __forceinline__ double exp_map_depth(const float (&p)[3], const ms::VolMapDev& m,
                                                const int4* __restrict__ vox) {
    long long v[3];
    bool in = true;
    for (int d = 0; d < 3; ++d) {
        const double u = rint(((double)p[d] - (double)m.origin[d]) / (double)m.grid[d]);
        const double top = (double)(m.n[d] - 1);
        in = in && u >= 0.0 && u <= top;
        v[d] = (long long)(u >= 0.0 ? (u <= top ? u : top) : 0.0);  // NaN: voxel 0
    }
    const int4 r = vox[m.off + (v[0] * m.n[1] + v[1]) * m.n[2] + v[2]];
    const int e[3] = {r.x, r.y, r.z};
    double t[3];
    for (int d = 0; d < 3; ++d) t[d] = (double)p[d] - ((double)e[d] * (double)m.grid[d] + (double)m.origin[d]);
    const double dist = sqrt_rn((t[0] * t[0] + t[2] * t[2]) + t[1] * t[1]);
    return in && r.w != 0 ? dist : -dist;
}

}  // namespace igm
