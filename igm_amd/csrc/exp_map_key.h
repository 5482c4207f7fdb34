// snormsq_exp of the reference on one bead and one volumetric map, shared by the DamID
// A-steps (asteps.hip) and the GenDamid membership test (restraints.hip).  Both
// translation units are built with -ffp-contract=off: the value is bit-exact.
//   voxel = np.round((x - origin) / grid)   f32 coordinate, float64 map geometry, half to even
//   outside the grid (both forms):  |(voxel - center) * grid|^2, the reference's mixed units
//   inside, NUCL = false:  |x - (edt * grid + origin)|^2   bead to its voxel's nearest lamina
//       voxel centre (DamidActivationDistanceStep.py:79-115, gendamid.py:17-47)
//   inside, NUCL = true:   |(voxel - edt) * grid|^2        voxel to voxel
//       (NuclDamidActivationDistanceStep.py:78-110)
// np.dot sums (t0^2 + t2^2) + t1^2 like the reference BLAS.
#pragma once
#include "mstep_common.h"

namespace igm {

template <bool NUCL>
__device__ __forceinline__ double exp_map_key(const float (&p)[3], const ms::VolMapDev& m,
                                              const int4* __restrict__ vox) {
    long long v[3];
    bool in = true;
    for (int d = 0; d < 3; ++d) {
        v[d] = (long long)rint(((double)p[d] - (double)m.origin[d]) / (double)m.grid[d]);
        in = in && v[d] >= 0 && v[d] < m.n[d];
    }
    double t[3];
    if (in) {
        const int4 r = vox[m.off + (v[0] * m.n[1] + v[1]) * m.n[2] + v[2]];
        const int e[3] = {r.x, r.y, r.z};
        for (int d = 0; d < 3; ++d) {
            if (NUCL)
                t[d] = (double)(v[d] - (long long)e[d]) * (double)m.grid[d];
            else
                t[d] = (double)p[d] - ((double)e[d] * (double)m.grid[d] + (double)m.origin[d]);
        }
    } else {
        for (int d = 0; d < 3; ++d) t[d] = ((double)v[d] - (double)m.center[d]) * (double)m.grid[d];
    }
    return (t[0] * t[0] + t[2] * t[2]) + t[1] * t[1];
}

}  // namespace igm
