// Per-structure restraint selection for configuration D: the DamID lamina envelope
// membership of Damid._apply_envelope (igm/restraints/damid.py:112-143) for every
// (structure, DamID row) at once.  A bead joins the structure's lamina envelope when
//     snormsq_ellipsoid(x_i, abc * (1 - cr), r_i) >= d_i^2          (damid.py:119-126)
// with the NumPy 1.x scalar arithmetic of snormsq_ellipsoid (damid.py:43-61): the
// float32 squares divided by float64 (abc*cutoff - r)^2 and summed in float64, compared
// with float64(d)^2.  Built with -ffp-contract=off, so membership is bit-exact.
//
// The same for the volumetric laminas of GenDamid._apply_envelope
// (igm/restraints/gendamid.py:17-47,101-107): a bead joins when
//     snormsq_exp(x_i, map of the structure) < d_i^2
// where d is a NumPy float32 scalar and d**2, a scalar-scalar operation of NumPy 1.x, is
// float64(d)^2 as in damid.py (the golden holds beads at exactly d from their lamina
// voxel, which a float32 square that rounds up would select).
#include <hip/hip_runtime.h>

#include "exp_map_key.h"
#include "igm_ctx.h"

namespace {
using namespace igm;

__global__ void base_flags_kernel(const uint32_t* __restrict__ base, int64_t natom, int64_t total,
                                  uint32_t* __restrict__ out) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < total) out[k] = base[k % natom];
}

struct SelArgs {
    int nstruct, natom;
    const float* xyz;  // (S, natom, 3) struct-major (the M-step layout)
    const float* radii;
    const igm_damid_row* rows;
    int64_t nrows;
    double abc[3];  // semiaxes * (1 - contact_range), float64 (damid.py:122-123)
    uint32_t bit;
    uint32_t* out;       // (S, natom)
    int* nsel;           // (S) selected rows
};

// grid (ceil(nrows / 256), S): consecutive rows across the wave, one structure per y
__global__ void __launch_bounds__(256) damid_select_kernel(SelArgs A) {
    const int s = blockIdx.y;
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int hit = 0;
    if (q < A.nrows) {
        const igm_damid_row w = A.rows[q];
        const int i = w.loc;
        if (i >= 0 && i < A.natom) {
            const float* x = A.xyz + ((size_t)s * A.natom + i) * 3;
            const double r = (double)A.radii[i];
            const double a = A.abc[0] - r, b = A.abc[1] - r, c = A.abc[2] - r;
            const double v = ((double)__fmul_rn(x[0], x[0]) / (a * a) + (double)__fmul_rn(x[1], x[1]) / (b * b)) +
                             (double)__fmul_rn(x[2], x[2]) / (c * c);
            const double d = (double)w.dist;
            if (v >= d * d) {
                atomicOr(&A.out[(size_t)s * A.natom + i], A.bit);
                hit = 1;
            }
        }
    }
    if (A.nsel) {
        for (int o = 32; o > 0; o >>= 1) hit += __shfl_xor(hit, o, 64);
        if ((threadIdx.x & 63) == 0 && hit) atomicAdd(&A.nsel[s], hit);
    }
}

struct VolSelArgs {
    int nstruct, natom;
    const float* xyz;  // (S, natom, 3) struct-major
    const igm_damid_row* rows;
    int64_t nrows;
    const ms::VolMapDev* maps;
    const int4* vox;
    const int* smap;  // (S) pool index of each structure, or NULL: map 0
    uint32_t bit;
    uint32_t* out;  // (S, natom)
    int* nsel;      // (S) selected rows
};

// grid (ceil(nrows / 256), S): consecutive rows across the wave, one structure per y;
// every lane gathers the one 16-byte voxel of its bead
__global__ void __launch_bounds__(256) volume_select_kernel(VolSelArgs A) {
    const int s = blockIdx.y;
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int hit = 0;
    if (q < A.nrows) {
        const igm_damid_row w = A.rows[q];
        const int i = w.loc;
        if (i >= 0 && i < A.natom) {
            const float* x = A.xyz + ((size_t)s * A.natom + i) * 3;
            const float p[3] = {x[0], x[1], x[2]};
            const ms::VolMapDev m = A.maps[A.smap ? A.smap[s] : 0];
            const double v = exp_map_key<false>(p, m, A.vox);
            const double d = (double)w.dist;
            if (v < d * d) {
                atomicOr(&A.out[(size_t)s * A.natom + i], A.bit);
                hit = 1;
            }
        }
    }
    if (A.nsel) {
        for (int o = 32; o > 0; o >>= 1) hit += __shfl_xor(hit, o, 64);
        if ((threadIdx.x & 63) == 0 && hit) atomicAdd(&A.nsel[s], hit);
    }
}

__global__ void check_map_index_kernel(const int* __restrict__ smap, int n, int nmap, int* __restrict__ bad) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q < n && (smap[q] < 0 || smap[q] >= nmap)) atomicOr(bad, 1);
}

}  // namespace

extern "C" int igm_volume_select(igm_ctx* c, uint32_t flags, int32_t nstruct, int32_t natom, const float* xyz,
                                 const igm_damid_row* rows, int64_t nrows, const int32_t* struct_map,
                                 uint32_t env_bit, const uint32_t* base_flags, int32_t base_per_struct,
                                 uint32_t* out_flags, int32_t* n_selected) {
    if (!c) return IGM_E_INVALID;
    if (nstruct <= 0 || natom <= 0 || nrows < 0 || !xyz || (nrows > 0 && !rows) || !base_flags || !out_flags ||
        env_bit == 0u)
        return fail(c, IGM_E_INVALID, "igm_volume_select: invalid arguments");
    if (nrows > (int64_t)0x7fffffff * 256 || nstruct > 65535)
        return fail(c, IGM_E_UNSUPPORTED, "igm_volume_select: grid too large");
    if (c->vol_nmap <= 0) return fail(c, IGM_E_INVALID, "igm_volume_select: no map staged (igm_mstep_set_volumes)");
    if (!struct_map && c->vol_nsmap > 0 && c->vol_nsmap < nstruct)
        return fail(c, IGM_E_INVALID, "igm_volume_select: volume map index staged for %d structures, batch has %d",
                    c->vol_nsmap, nstruct);
    IGM_HIP_CHECK(c, hipSetDevice(c->device));
    const float* d_xyz;
    const igm_damid_row* d_rows;
    const uint32_t* d_base;
    const int32_t* d_smap = nullptr;
    const size_t nf = (size_t)nstruct * natom;
    IGM_TRY(to_device(c, flags, "vs_xyz", xyz, nf * 3, &d_xyz));
    IGM_TRY(to_device(c, flags, "vs_rows", rows, (size_t)nrows, &d_rows));
    IGM_TRY(to_device(c, flags, "vs_base", base_flags, base_per_struct ? nf : (size_t)natom, &d_base));
    if (struct_map) {
        // the kernel indexes the map pool with these: reject any index outside it
        IGM_TRY(to_device(c, flags, "vs_smap", struct_map, (size_t)nstruct, &d_smap));
        void* p_bad;
        IGM_TRY(workspace(c, "vs_bad", sizeof(int), &p_bad));
        IGM_HIP_CHECK(c, hipMemsetAsync(p_bad, 0, sizeof(int), c->stream));
        hipLaunchKernelGGL(check_map_index_kernel, dim3((unsigned)ceil_div(nstruct, 256)), dim3(256), 0, c->stream,
                           d_smap, nstruct, c->vol_nmap, (int*)p_bad);
        IGM_HIP_CHECK(c, hipGetLastError());
        int bad = 0;
        IGM_HIP_CHECK(c, hipMemcpyAsync(&bad, p_bad, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        IGM_HIP_CHECK(c, hipStreamSynchronize(c->stream));
        if (bad) return fail(c, IGM_E_INVALID, "igm_volume_select: map index outside [0, %d)", c->vol_nmap);
    } else if (c->vol_nsmap > 0) {
        void* ps;
        IGM_TRY(workspace(c, "vol_smap", 1, &ps));
        d_smap = (const int32_t*)ps;
    }
    uint32_t* d_out;
    int32_t* d_nsel = nullptr;
    IGM_TRY(out_device(c, flags, "vs_out", out_flags, nf, &d_out));
    if (n_selected) {
        IGM_TRY(out_device(c, flags, "vs_nsel", n_selected, (size_t)nstruct, &d_nsel));
        IGM_HIP_CHECK(c, hipMemsetAsync(d_nsel, 0, sizeof(int32_t) * nstruct, c->stream));
    }
    // base_per_struct: natom == nf makes the broadcast kernel a plain copy
    hipLaunchKernelGGL(base_flags_kernel, dim3((unsigned)ceil_div((int64_t)nf, 256)), dim3(256), 0, c->stream, d_base,
                       base_per_struct ? (int64_t)nf : (int64_t)natom, (int64_t)nf, d_out);
    IGM_HIP_CHECK(c, hipGetLastError());
    if (nrows > 0) {
        VolSelArgs A;
        A.nstruct = nstruct;
        A.natom = natom;
        A.xyz = d_xyz;
        A.rows = d_rows;
        A.nrows = nrows;
        void *pm, *pv;
        IGM_TRY(workspace(c, "vol_maps", 1, &pm));
        IGM_TRY(workspace(c, "vol_vox", 1, &pv));
        A.maps = (const ms::VolMapDev*)pm;
        A.vox = (const int4*)pv;
        A.smap = d_smap;
        A.bit = env_bit;
        A.out = d_out;
        A.nsel = d_nsel;
        Timed tm(c, "volume_select");
        hipLaunchKernelGGL(volume_select_kernel, dim3((unsigned)ceil_div(nrows, 256), (unsigned)nstruct), dim3(256), 0,
                           c->stream, A);
        IGM_HIP_CHECK(c, hipGetLastError());
    }
    IGM_TRY(to_host(c, flags, out_flags, d_out, nf));
    if (n_selected) IGM_TRY(to_host(c, flags, n_selected, d_nsel, (size_t)nstruct));
    return finish(c, flags);
}

extern "C" int igm_damid_select(igm_ctx* c, uint32_t flags, int32_t nstruct, int32_t natom, const float* xyz,
                                const float* radii, const igm_damid_row* rows, int64_t nrows,
                                const double* semiaxes, double contact_range, uint32_t env_bit,
                                const uint32_t* base_flags, uint32_t* out_flags, int32_t* n_selected) {
    if (!c) return IGM_E_INVALID;
    if (nstruct <= 0 || natom <= 0 || nrows < 0 || !xyz || !radii || (nrows > 0 && !rows) || !semiaxes ||
        !base_flags || !out_flags || env_bit == 0u)
        return fail(c, IGM_E_INVALID, "igm_damid_select: invalid arguments");
    if (nrows > (int64_t)0x7fffffff * 256 || nstruct > 65535)
        return fail(c, IGM_E_UNSUPPORTED, "igm_damid_select: grid too large");
    IGM_HIP_CHECK(c, hipSetDevice(c->device));
    const float *d_xyz, *d_radii;
    const igm_damid_row* d_rows;
    const uint32_t* d_base;
    const size_t nf = (size_t)nstruct * natom;
    IGM_TRY(to_device(c, flags, "ds_xyz", xyz, nf * 3, &d_xyz));
    IGM_TRY(to_device(c, flags, "ds_radii", radii, (size_t)natom, &d_radii));
    IGM_TRY(to_device(c, flags, "ds_rows", rows, (size_t)nrows, &d_rows));
    IGM_TRY(to_device(c, flags, "ds_base", base_flags, (size_t)natom, &d_base));
    uint32_t* d_out;
    int32_t* d_nsel = nullptr;
    IGM_TRY(out_device(c, flags, "ds_out", out_flags, nf, &d_out));
    if (n_selected) {
        IGM_TRY(out_device(c, flags, "ds_nsel", n_selected, (size_t)nstruct, &d_nsel));
        IGM_HIP_CHECK(c, hipMemsetAsync(d_nsel, 0, sizeof(int32_t) * nstruct, c->stream));
    }
    hipLaunchKernelGGL(base_flags_kernel, dim3((unsigned)ceil_div((int64_t)nf, 256)), dim3(256), 0, c->stream, d_base,
                       natom, (int64_t)nf, d_out);
    IGM_HIP_CHECK(c, hipGetLastError());
    SelArgs A;
    A.nstruct = nstruct;
    A.natom = natom;
    A.xyz = d_xyz;
    A.radii = d_radii;
    A.rows = d_rows;
    A.nrows = nrows;
    const double cutoff = 1.0 - contact_range;
    for (int k = 0; k < 3; ++k) A.abc[k] = semiaxes[k] * cutoff;
    A.bit = env_bit;
    A.out = d_out;
    A.nsel = d_nsel;
    if (nrows > 0) {
        Timed tm(c, "damid_select");
        hipLaunchKernelGGL(damid_select_kernel, dim3((unsigned)ceil_div(nrows, 256), (unsigned)nstruct), dim3(256), 0,
                           c->stream, A);
        IGM_HIP_CHECK(c, hipGetLastError());
    }
    IGM_TRY(to_host(c, flags, out_flags, d_out, nf));
    if (n_selected) IGM_TRY(to_host(c, flags, n_selected, d_nsel, (size_t)nstruct));
    return finish(c, flags);
}
