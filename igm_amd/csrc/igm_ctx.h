// Internal context / workspace / error plumbing shared by the HIP translation units.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/igm_hip.h"

struct igm_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    std::string err;
    // named device workspaces, grown on demand (never shrunk until destroy)
    std::map<std::string, std::pair<void*, size_t>> ws;
    // per kernel family: (start, stop) events of its last launch on `stream`
    std::map<std::string, std::pair<hipEvent_t, hipEvent_t>> kev;
    // per kernel family launched once per batch of one call: the event times of its launches
    // summed by that call (igm_last_kernel_ms reads these before kev)
    std::map<std::string, double> kms;
    // volumetric maps staged by igm_mstep_set_volumes (device copies live in ws slots
    // "vol_maps", "vol_vox", "vol_smap")
    int vol_nmap = 0, vol_nsmap = 0;
    // host copies of the default table and of the per-envelope tables of
    // igm_mstep_set_envelope_maps (empty: envelope e reads the default table)
    std::vector<int> vol_smap_h;
    std::vector<int> vol_emap_h[IGM_MAX_ENVELOPES];
    // position anchors staged by igm_mstep_set_anchors (host copies; the igm_mstep_* calls
    // build their device form, ws slots "ms_anch" / "ms_aidx" / "ms_nanch")
    std::vector<int64_t> anch_ptr_h;  // (nstruct + 1), empty: nothing staged
    std::vector<igm_anchor> anch_h;
    int num_cus = 256;
    // last HBM-size anneal: {K, slots, builds, re-cuts, largest resident set, largest
    // owned set, abort (0: the domain-decomposed engine ran; -1 / > 0: the population
    // engine ran, by choice / after an abort)}
    size_t lds_per_block = 65536;
    // auxiliary streams (+ one event each) for independent work inside one call,
    // created on first use: the population engine runs its structure groups on them
    std::vector<hipStream_t> aux;
    std::vector<hipEvent_t> aux_ev;
    hipEvent_t fork_ev = nullptr;
};

namespace igm {

inline int fail(igm_ctx* c, int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (c) c->err = buf;
    return code;
}

#define IGM_HIP_CHECK(ctx, expr)                                                           \
    do {                                                                                  \
        hipError_t _e = (expr);                                                           \
        if (_e != hipSuccess)                                                             \
            return ::igm::fail((ctx), IGM_E_HIP, "%s:%d %s -> %s", __FILE__, __LINE__,    \
                               #expr, hipGetErrorString(_e));                              \
    } while (0)

#define IGM_TRY(expr)               \
    do {                            \
        int _r = (expr);            \
        if (_r != IGM_OK) return _r; \
    } while (0)

// Device workspace slot `name` of at least `bytes` (contents undefined).
inline int workspace(igm_ctx* c, const char* name, size_t bytes, void** out) {
    auto& slot = c->ws[name];
    if (slot.second < bytes) {
        if (slot.first) {
            (void)hipStreamSynchronize(c->stream);
            (void)hipFree(slot.first);
            slot.first = nullptr;
            slot.second = 0;
        }
        size_t sz = bytes < 256 ? 256 : bytes;
        if (hipMalloc(&slot.first, sz) != hipSuccess) {
            (void)hipGetLastError();
            return fail(c, IGM_E_NOMEM, "hipMalloc(%zu) failed for workspace '%s'", sz, name);
        }
        slot.second = sz;
    }
    *out = slot.first;
    return IGM_OK;
}

// Get a device view of a caller array: either the pointer itself (device mode)
// or a staged copy in workspace `name`.
template <typename T>
inline int to_device(igm_ctx* c, uint32_t flags, const char* name, const T* p, size_t n, const T** out) {
    if (flags & IGM_DEVICE_PTRS || p == nullptr || n == 0) {
        *out = p;
        return IGM_OK;
    }
    void* d;
    IGM_TRY(workspace(c, name, n * sizeof(T), &d));
    IGM_HIP_CHECK(c, hipMemcpyAsync(d, p, n * sizeof(T), hipMemcpyHostToDevice, c->stream));
    *out = static_cast<const T*>(d);
    return IGM_OK;
}

template <typename T>
inline int out_device(igm_ctx* c, uint32_t flags, const char* name, T* p, size_t n, T** out) {
    if (flags & IGM_DEVICE_PTRS || p == nullptr || n == 0) {
        *out = p;
        return IGM_OK;
    }
    void* d;
    IGM_TRY(workspace(c, name, n * sizeof(T), &d));
    *out = static_cast<T*>(d);
    return IGM_OK;
}

template <typename T>
inline int to_host(igm_ctx* c, uint32_t flags, T* host, const T* dev, size_t n) {
    if (flags & IGM_DEVICE_PTRS || host == nullptr || n == 0 || host == dev) return IGM_OK;
    IGM_HIP_CHECK(c, hipMemcpyAsync(host, dev, n * sizeof(T), hipMemcpyDeviceToHost, c->stream));
    return IGM_OK;
}

inline int finish(igm_ctx* c, uint32_t flags) {
    if (!(flags & IGM_ASYNC) || !(flags & IGM_DEVICE_PTRS)) IGM_HIP_CHECK(c, hipStreamSynchronize(c->stream));
    IGM_HIP_CHECK(c, hipGetLastError());
    return IGM_OK;
}

// Event-bracketed region on the context stream (elapsed time is read lazily by
// igm_last_kernel_ms, so timing never adds a host synchronisation).
struct Timed {
    igm_ctx* c;
    std::pair<hipEvent_t, hipEvent_t>* ev;
    Timed(igm_ctx* c_, const char* name) : c(c_) {
        auto& e = c->kev[name];
        if (!e.first) {
            (void)hipEventCreate(&e.first);
            (void)hipEventCreate(&e.second);
        }
        ev = &e;
        (void)hipEventRecord(e.first, c->stream);
    }
    ~Timed() { (void)hipEventRecord(ev->second, c->stream); }
};

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// Device table of the map index that volume envelope e reads for structure s of a call
// over nstruct structures: table[e * stride + s] (table NULL: map 0).  Without a table of
// igm_mstep_set_envelope_maps this is the default struct_map of igm_mstep_set_volumes with
// stride 0 -- the lookup of a library without per-envelope tables; otherwise one row per
// envelope (its own table, else the default one, else zeros), staged in "vol_etab".
// A staged table must cover the structures of the call.
inline int envelope_map_tables(igm_ctx* c, int nstruct, const int** table, int* stride) {
    *table = nullptr;
    *stride = 0;
    bool own = false;
    for (int e = 0; e < IGM_MAX_ENVELOPES; ++e) {
        const int n = (int)c->vol_emap_h[e].size();
        if (n > 0 && n < nstruct)
            return fail(c, IGM_E_INVALID, "volume map index of envelope %d staged for %d structures, batch has %d", e,
                        n, nstruct);
        own = own || n > 0;
    }
    if (c->vol_nsmap > 0 && c->vol_nsmap < nstruct)
        return fail(c, IGM_E_INVALID, "volume map index staged for %d structures, batch has %d", c->vol_nsmap, nstruct);
    void* ps;
    if (!own) {
        if (c->vol_nsmap > 0) {
            IGM_TRY(workspace(c, "vol_smap", 1, &ps));
            *table = (const int*)ps;
        }
        return IGM_OK;
    }
    std::vector<int> tab((size_t)IGM_MAX_ENVELOPES * nstruct, 0);
    for (int e = 0; e < IGM_MAX_ENVELOPES; ++e) {
        const std::vector<int>& src = c->vol_emap_h[e].empty() ? c->vol_smap_h : c->vol_emap_h[e];
        for (int s = 0; s < nstruct && s < (int)src.size(); ++s) tab[(size_t)e * nstruct + s] = src[s];
    }
    IGM_TRY(workspace(c, "vol_etab", sizeof(int) * tab.size(), &ps));
    IGM_HIP_CHECK(c, hipMemcpyAsync(ps, tab.data(), sizeof(int) * tab.size(), hipMemcpyHostToDevice, c->stream));
    IGM_HIP_CHECK(c, hipStreamSynchronize(c->stream));  // tab dies here
    *table = (const int*)ps;
    *stride = nstruct;
    return IGM_OK;
}

// Device form of the anchors staged by igm_mstep_set_anchors for a call over nstruct
// structures of natom atoms (all NULL: nothing staged, the kernels without the term run):
//   anch   every structure's anchors sorted by atom -- a stable sort, so the anchors of one
//          atom keep the order given -- each structure closed by a sentinel (atom = ~0u)
//   aidx   (nstruct, natom): index in anch of the atom's first anchor, -1 = none; an atom's
//          anchors are the entries from there on that carry its id
//   nanch  (nstruct) anchors of the structure (thermo temp of group all)
struct AnchorsDev {
    const igm_anchor* anch;
    const int* aidx;
    const int* nanch;
};

inline int stage_anchors(igm_ctx* c, int nstruct, int natom, AnchorsDev* out) {
    *out = AnchorsDev{nullptr, nullptr, nullptr};
    if (c->anch_ptr_h.empty()) return IGM_OK;
    if ((int)c->anch_ptr_h.size() != nstruct + 1)
        return fail(c, IGM_E_INVALID, "anchors staged for %d structures, batch has %d (igm_mstep_set_anchors)",
                    (int)c->anch_ptr_h.size() - 1, nstruct);
    const int64_t n = c->anch_ptr_h[nstruct];
    if (n == 0) return IGM_OK;  // every row empty: the code path of nothing staged
    std::vector<igm_anchor> dev((size_t)n + nstruct);
    std::vector<int> idx((size_t)nstruct * natom, -1), cnt(nstruct);
    std::vector<int> first(natom + 1);
    for (int s = 0; s < nstruct; ++s) {
        const int64_t b0 = c->anch_ptr_h[s], b1 = c->anch_ptr_h[s + 1];
        const igm_anchor* src = c->anch_h.data() + b0;
        const int m = (int)(b1 - b0);
        cnt[s] = m;
        std::fill(first.begin(), first.end(), 0);
        for (int q = 0; q < m; ++q) {
            if (src[q].atom >= (uint32_t)natom)
                return fail(c, IGM_E_INVALID, "anchor %d of structure %d: atom %u >= natom %d", q, s, src[q].atom,
                            natom);
            ++first[src[q].atom + 1];
        }
        const size_t base = (size_t)b0 + s;  // one sentinel per earlier structure
        int* ix = idx.data() + (size_t)s * natom;
        for (int a = 0; a < natom; ++a) {
            if (first[a + 1] > 0) ix[a] = (int)(base + first[a]);
            first[a + 1] += first[a];
        }
        for (int q = 0; q < m; ++q) dev[base + first[src[q].atom]++] = src[q];  // counting sort: stable
        dev[base + m] = igm_anchor{~0u, 0.f, 0.f, 0.f, 0.f, 0.f};
    }
    void *pa, *pi, *pn;
    IGM_TRY(workspace(c, "ms_anch", sizeof(igm_anchor) * dev.size(), &pa));
    IGM_TRY(workspace(c, "ms_aidx", sizeof(int) * idx.size(), &pi));
    IGM_TRY(workspace(c, "ms_nanch", sizeof(int) * cnt.size(), &pn));
    IGM_HIP_CHECK(c, hipMemcpyAsync(pa, dev.data(), sizeof(igm_anchor) * dev.size(), hipMemcpyHostToDevice, c->stream));
    IGM_HIP_CHECK(c, hipMemcpyAsync(pi, idx.data(), sizeof(int) * idx.size(), hipMemcpyHostToDevice, c->stream));
    IGM_HIP_CHECK(c, hipMemcpyAsync(pn, cnt.data(), sizeof(int) * cnt.size(), hipMemcpyHostToDevice, c->stream));
    IGM_HIP_CHECK(c, hipStreamSynchronize(c->stream));  // the host vectors die here
    *out = AnchorsDev{(const igm_anchor*)pa, (const int*)pi, (const int*)pn};
    return IGM_OK;
}

// at least n auxiliary streams; the work on them is forked from and joined into c->stream
inline int aux_streams(igm_ctx* c, int n) {
    if (!c->fork_ev) IGM_HIP_CHECK(c, hipEventCreateWithFlags(&c->fork_ev, hipEventDisableTiming));
    while ((int)c->aux.size() < n) {
        hipStream_t st;
        hipEvent_t ev;
        IGM_HIP_CHECK(c, hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        IGM_HIP_CHECK(c, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        c->aux.push_back(st);
        c->aux_ev.push_back(ev);
    }
    return IGM_OK;
}

// the first n auxiliary streams wait for the work queued so far on c->stream
inline int aux_fork(igm_ctx* c, int n) {
    IGM_HIP_CHECK(c, hipEventRecord(c->fork_ev, c->stream));
    for (int g = 0; g < n; ++g) IGM_HIP_CHECK(c, hipStreamWaitEvent(c->aux[g], c->fork_ev, 0));
    return IGM_OK;
}

// c->stream waits for the work queued on the first n auxiliary streams
inline int aux_join(igm_ctx* c, int n) {
    for (int g = 0; g < n; ++g) {
        IGM_HIP_CHECK(c, hipEventRecord(c->aux_ev[g], c->aux[g]));
        IGM_HIP_CHECK(c, hipStreamWaitEvent(c->stream, c->aux_ev[g], 0));
    }
    return IGM_OK;
}

}  // namespace igm
