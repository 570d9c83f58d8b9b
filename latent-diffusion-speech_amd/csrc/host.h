// The host toolkit every C-ABI entry of liblds is written on: error macros, a handle's device allocations, the name -> tensor map of a
// create call, the workspace allocators and the argument checks that several components state in the same words.  Host code only; include
// it after kernels.h.  Nothing here launches on its own account (upload_clip_ints goes through launch_set_list).
#pragma once
#include "../../include/lds.h"
#include "kernels.h"

#include <stdint.h>
#include <string.h>

#include <map>
#include <string>
#include <vector>

// lds::set_error (model.hip, next to lds_last_error) records the thread's message and returns the code
#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) return lds::set_error(LDS_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)
#define LDS_TRY(expr)                    \
    do {                                 \
        int r_ = (expr);                 \
        if (r_ != LDS_OK) return r_;     \
    } while (0)

// the end of an entry that launched without checking each launch: did the last one succeed
static int launched(const char* fn) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? LDS_OK : lds::set_error(LDS_EHIP, "%s: %s", fn, hipGetErrorString(e));
}

// ------------------------------------------------------------------------------------------------
// device allocations owned by a handle
// ------------------------------------------------------------------------------------------------
struct Owner {
    std::vector<void*> ptrs;
    ~Owner() {
        for (void* p : ptrs) (void)hipFree(p);
    }
    float* upload(const std::vector<float>& h) {
        void* d = nullptr;
        if (hipMalloc(&d, h.size() * sizeof(float)) != hipSuccess) return nullptr;
        if (hipMemcpy(d, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipFree(d);
            return nullptr;
        }
        ptrs.push_back(d);
        return (float*)d;
    }
    void* upload_bytes(const void* h, size_t n) {
        void* d = nullptr;
        if (hipMalloc(&d, n) != hipSuccess) return nullptr;
        if (hipMemcpy(d, h, n, hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipFree(d);
            return nullptr;
        }
        ptrs.push_back(d);
        return d;
    }
};

struct Tensors {
    std::map<std::string, std::pair<const float*, int64_t>> m;
    std::string missing;
    // numel < 0: any positive size, reported through *got (a tensor whose length the checkpoint decides, such as a classifier's bias)
    const float* get(const std::string& k, int64_t numel, int64_t* got = nullptr) {
        auto it = m.find(k);
        if (it == m.end() || (numel >= 0 ? it->second.second != numel : it->second.second < 1)) {
            if (missing.empty()) missing = k + (it == m.end() ? " (absent)" : " (wrong size)");
            return nullptr;
        }
        if (got) *got = it->second.second;
        return it->second.first;
    }
    bool has(const std::string& k) const { return m.count(k) != 0; }
};

// The weights of a create call: the caller's name -> tensor map (entries with a null name or pointer count as absent) and the new
// handle's device allocations.
struct WeightLoader {
    Tensors T;
    Owner& o;
    WeightLoader(Owner& own, int n, const char* const* names, const float* const* ptrs, const int64_t* numel) : o(own) {
        for (int i = 0; i < n; ++i)
            if (names[i] && ptrs[i]) T.m[names[i]] = {ptrs[i], numel[i]};
    }
    const float* get(const std::string& k, int64_t cnt) { return T.get(k, cnt); }
    const float* opt(const std::string& k, int64_t cnt) {      // a tensor the checkpoint may leave out: absent or of another size is no error
        auto it = T.m.find(k);
        return it != T.m.end() && it->second.second == cnt ? it->second.first : nullptr;
    }
    float* vec(const std::string& k, int64_t cnt, int64_t* got = nullptr) {      // a tensor uploaded as it is (cnt < 0, got: Tensors::get)
        int64_t n = cnt;
        const float* p = T.get(k, cnt, &n);
        if (p && got) *got = n;
        return p ? o.upload(std::vector<float>(p, p + n)) : nullptr;
    }
    // the end of a create: hands the handle out, or deletes it and names the first tensor that was absent or of the wrong size
    // ("<tag>: <tensor>", or "<miss_tag> <tensor>" where the create's message has always read that way)
    template <class H>
    int finish(bool ok, const char* tag, H* h, H** out, const char* miss_tag = nullptr) {
        if (ok) { *out = h; return LDS_OK; }
        delete h;
        if (!T.missing.empty()) return miss_tag ? lds::set_error(LDS_EMISSING, "%s %s", miss_tag, T.missing.c_str()) : lds::set_error(LDS_EMISSING, "%s: %s", tag, T.missing.c_str());
        return lds::set_error(LDS_ENOMEM, "%s weight upload failed", tag);
    }
};

// ------------------------------------------------------------------------------------------------
// workspaces (caller-owned memory): every slot starts on a 256-byte boundary
// ------------------------------------------------------------------------------------------------
// byte offsets of a plan that stores offsets, not pointers (its *_workspace_bytes entry takes no memory)
struct Slots {
    size_t o = 0;
    static size_t round(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
    size_t take(size_t bytes) { const size_t at = o; o += round(bytes); return at; }
};
// bump allocator of a plan that stores pointers; a null base sizes the plan
struct Arena {
    char* base; size_t cap; size_t used = 0; bool ok = true;
    std::vector<std::pair<std::string, std::pair<size_t, size_t>>>* log = nullptr;      // (name, (offset, bytes)) of every slot: lds_debug_unet_plan
    Arena(void* p, size_t n) : base((char*)p), cap(n) {}
    float* f(size_t n_floats, const char* name = nullptr) {
        size_t bytes = (n_floats * sizeof(float) + 255) & ~(size_t)255;
        if (base && used + bytes > cap) ok = false;
        char* p = base ? base + used : nullptr;
        if (log) log->push_back({name ? name : "slot" + std::to_string(log->size()), {used, bytes}});
        used += bytes;
        return (float*)p;
    }
};
// A *_workspace_bytes entry: the call's limits (check), then its plan (plan) run on an arena without memory
template <class Check, class Plan>
static int plan_bytes(size_t* out, Check check, Plan plan) {
    if (!out) return lds::set_error(LDS_EINVAL, "null argument");
    LDS_TRY(check());
    Arena A(nullptr, 0);
    plan(A);
    *out = A.used;
    return LDS_OK;
}

// ------------------------------------------------------------------------------------------------
// per-clip counts given by the caller: no more than 64 of them
// ------------------------------------------------------------------------------------------------
// every value in lo .. hi
static int clip_lens_check(const char* name, const int32_t* v, int B, int64_t lo, int64_t hi) {
    if (B > 64) return lds::set_error(LDS_EINVAL, "per-clip lengths: at most 64 clips per call (got %d)", B);
    for (int b = 0; b < B; ++b)
        if (v[b] < lo || v[b] > hi) return lds::set_error(LDS_EINVAL, "%s[%d] = %d outside %lld .. %lld", name, b, v[b], (long long)lo, (long long)hi);
    return LDS_OK;
}
// ... into the 64 slots of a by-value kernel argument (XvLens, CtcLens, CtcLabs, KnLens): v[b] = src[b] in 0 .. T, zeros behind them.
// `fn` is the entry's name and `name` the argument's in the messages; the caller has refused B > 64 and sets the struct's other fields.
static int clip_lens_fill(const char* fn, const char* name, int B, int T, const int32_t* src, int (&v)[64]) {
    if (!src) return lds::set_error(LDS_EINVAL, "%s: null %s", fn, name);
    for (int i = 0; i < 64; ++i) v[i] = 0;
    for (int b = 0; b < B; ++b) {
        if (src[b] < 0 || src[b] > T) return lds::set_error(LDS_EINVAL, "%s: %s[%d] = %d outside 0 .. %d", fn, name, b, src[b], T);
        v[b] = src[b];
    }
    return LDS_OK;
}
// ... to a device slot, carried in a kernel's arguments (launch_set_list): stream-ordered, `host` is read during the call only
static int upload_clip_ints(const int32_t* host, int B, int* dev, hipStream_t st) {
    float tmp[64];
    for (int b = 0; b < B; ++b) memcpy(&tmp[b], &host[b], sizeof(int));
    HIP_TRY(lds::launch_set_list((float*)dev, tmp, B, st));
    return LDS_OK;
}

// ------------------------------------------------------------------------------------------------
// dimension rules; `tag` is the component's or the entry's name in the messages
// ------------------------------------------------------------------------------------------------
static int range_check(const char* tag, const char* name, int v, int lo, int hi) {
    return v < lo || v > hi ? lds::set_error(LDS_EINVAL, "%s: %s %d outside %d .. %d", tag, name, v, lo, hi) : LDS_OK;
}
static int width_check(const char* tag, const char* name, int v, bool capped) {      // a GEMM's channel count; capped: at most 1024
    if (capped && (v < 64 || v % 64 || v > 1024)) return lds::set_error(LDS_EINVAL, "%s: %s %d must be a multiple of 64 in 64 .. 1024", tag, name, v);
    if (v < 64 || v % 64) return lds::set_error(LDS_EINVAL, "%s: %s %d must be a positive multiple of 64", tag, name, v);
    return LDS_OK;
}
static int heads_check(const char* tag, int n_state, int n_head) {
    return n_head < 1 || n_state != n_head * 64 ? lds::set_error(LDS_EINVAL, "%s: n_state / n_head must be 64 (got %d / %d)", tag, n_state, n_head) : LDS_OK;
}
