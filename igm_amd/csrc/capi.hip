// Context management of libigmhip.so (include/igm_hip.h).
#include <cmath>

#include "igm_ctx.h"

extern "C" {

const char* igm_version(void) { return "igm_amd 0.1 gfx950"; }

int igm_ctx_create(int device, igm_ctx** out) {
    if (!out) return IGM_E_INVALID;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return IGM_E_HIP;
    if (device < 0 || device >= ndev) return IGM_E_INVALID;
    if (hipSetDevice(device) != hipSuccess) return IGM_E_HIP;
    igm_ctx* c = new igm_ctx();
    c->device = device;
    if (hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return IGM_E_HIP;
    }
    c->stream = c->own_stream;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) {
        c->num_cus = prop.multiProcessorCount;
        c->lds_per_block = prop.sharedMemPerBlock;
    }
    *out = c;
    return IGM_OK;
}

void igm_ctx_destroy(igm_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    for (auto& kv : c->ws)
        if (kv.second.first) (void)hipFree(kv.second.first);
    for (auto& kv : c->kev) {
        if (kv.second.first) (void)hipEventDestroy(kv.second.first);
        if (kv.second.second) (void)hipEventDestroy(kv.second.second);
    }
    for (size_t g = 0; g < c->aux.size(); ++g) {
        (void)hipStreamSynchronize(c->aux[g]);
        (void)hipStreamDestroy(c->aux[g]);
        (void)hipEventDestroy(c->aux_ev[g]);
    }
    if (c->fork_ev) (void)hipEventDestroy(c->fork_ev);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;
}

const char* igm_last_error(const igm_ctx* c) { return c ? c->err.c_str() : "null context"; }

int igm_ctx_set_stream(igm_ctx* c, void* s) {
    if (!c) return IGM_E_INVALID;
    c->stream = s ? static_cast<hipStream_t>(s) : c->own_stream;
    return IGM_OK;
}

int igm_ctx_synchronize(igm_ctx* c) {
    if (!c) return IGM_E_INVALID;
    IGM_HIP_CHECK(c, hipStreamSynchronize(c->stream));
    return IGM_OK;
}

// Position anchors of the igm_mstep_* calls that follow: validated and kept on the host;
// every call builds the device form for its own batch (mstep.hip: stage_anchors).
int igm_mstep_set_anchors(igm_ctx* c, int32_t nstruct, const int64_t* anchor_ptr, const igm_anchor* anchors) {
    using igm::fail;
    if (!c) return IGM_E_INVALID;
    if (nstruct < 0 || (nstruct > 0 && !anchor_ptr))
        return fail(c, IGM_E_INVALID, "igm_mstep_set_anchors: invalid arguments");
    c->anch_ptr_h.clear();
    c->anch_h.clear();
    if (nstruct == 0) return IGM_OK;
    if (anchor_ptr[0] != 0) return fail(c, IGM_E_INVALID, "igm_mstep_set_anchors: anchor_ptr[0] = %lld, not 0",
                                        (long long)anchor_ptr[0]);
    for (int s = 0; s < nstruct; ++s)
        if (anchor_ptr[s + 1] < anchor_ptr[s])
            return fail(c, IGM_E_INVALID, "igm_mstep_set_anchors: anchor_ptr is not monotone at structure %d", s);
    const int64_t n = anchor_ptr[nstruct];
    if (n > 0 && !anchors) return fail(c, IGM_E_INVALID, "igm_mstep_set_anchors: anchors is NULL");
    if (n + nstruct > 0x7fffffff) return fail(c, IGM_E_UNSUPPORTED, "igm_mstep_set_anchors: %lld anchors", (long long)n);
    for (int64_t q = 0; q < n; ++q) {
        const igm_anchor& a = anchors[q];
        if (!std::isfinite(a.x) || !std::isfinite(a.y) || !std::isfinite(a.z))
            return fail(c, IGM_E_INVALID, "igm_mstep_set_anchors: anchor %lld has a non-finite target", (long long)q);
        if (!std::isfinite(a.r0) || !std::isfinite(a.k))
            return fail(c, IGM_E_INVALID, "igm_mstep_set_anchors: anchor %lld has a non-finite r0 or k", (long long)q);
        if (a.r0 < 0.0f) return fail(c, IGM_E_INVALID, "igm_mstep_set_anchors: anchor %lld has r0 < 0", (long long)q);
    }
    c->anch_ptr_h.assign(anchor_ptr, anchor_ptr + nstruct + 1);
    c->anch_h.assign(anchors, anchors + n);
    return IGM_OK;
}

double igm_last_kernel_ms(const igm_ctx* c, const char* name) {
    if (!c || !name) return -1.0;
    auto sum = c->kms.find(name);
    if (sum != c->kms.end()) return sum->second;
    auto it = c->kev.find(name);
    if (it == c->kev.end()) return -1.0;
    if (hipEventSynchronize(it->second.second) != hipSuccess) return -1.0;
    float ms = -1.f;
    if (hipEventElapsedTime(&ms, it->second.first, it->second.second) != hipSuccess) return -1.0;
    return ms;
}

}  // extern "C"
