// Stand-alone check of host.h (make host_selftest; tests/test_cpu_host_toolkit.py): host only, AddressSanitizer + UBSan, linked against
// host_stub_hip.cpp, so "device" memory is malloc'd and the sanitizer's leak check at exit witnesses that a failed create frees its uploads.
#include "host.h"

#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>

static char g_msg[512];
int lds::set_error(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_msg, sizeof(g_msg), fmt, ap);
    va_end(ap);
    return code;
}
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "host_selftest: line %d: %s (last message: %s)\n", __LINE__, #c, g_msg); exit(1); } } while (0)
static bool said(const char* text) { return strcmp(g_msg, text) == 0; }

static int g_deleted = 0;
struct Handle { Owner own; float *a = nullptr, *b = nullptr; ~Handle() { ++g_deleted; } };
static int create(int n, const char* const* names, const float* const* ptrs, const int64_t* numel, Handle** out) {
    Handle* h = new Handle();
    WeightLoader W(h->own, n, names, ptrs, numel);
    h->a = W.vec("a", 3);
    h->b = W.vec("b", 2);
    return W.finish(h->a && h->b, "selftest", h, out);
}

int main() {
    // Arena and Slots: a sizing pass and a real pass agree, slots are 256-byte aligned, a zero-size slot takes nothing, capacity is exact
    const size_t floats[4] = {1, 0, 64, 65};
    size_t off[2][4], total[2];
    static char mem[4096];
    for (int pass = 0; pass < 2; ++pass) {
        Arena A(pass ? mem : nullptr, pass ? total[0] : 0);
        for (int i = 0; i < 4; ++i) { off[pass][i] = A.used; const float* p = A.f(floats[i]); CHECK(pass ? (const char*)p == mem + off[1][i] : p == nullptr); }
        total[pass] = A.used;
        CHECK(A.ok);
    }
    Slots S;
    for (int i = 0; i < 4; ++i) {
        CHECK(off[0][i] == off[1][i] && off[0][i] % 256 == 0 && S.take(floats[i] * 4) == off[0][i]);
    }
    CHECK(total[0] == total[1] && total[0] == S.o && total[0] == 256 + 0 + 256 + 512 && off[0][1] == off[0][2] && Slots::round(257) == 512);
    Arena tight(mem, total[0] - 1);
    for (int i = 0; i < 4; ++i) tight.f(floats[i]);
    CHECK(!tight.ok);

    // Tensors: absent / wrong size, only the first failure is kept, the any-size lookup
    const float data[4] = {1, 2, 3, 4};
    Tensors T;
    T.m["a"] = {data, 3};
    T.m["empty"] = {data, 0};
    int64_t got = -1;
    CHECK(T.get("a", 3) == data && T.missing.empty() && T.get("a", -1, &got) == data && got == 3);
    CHECK(!T.get("empty", -1, &got) && got == 3 && T.missing == "empty (wrong size)");
    T.missing.clear();
    CHECK(!T.get("nope", 3) && T.missing == "nope (absent)" && !T.get("a", 4) && T.missing == "nope (absent)");
    T.missing.clear();
    CHECK(!T.get("a", 4) && T.missing == "a (wrong size)" && T.has("a") && !T.has("nope"));

    // Owner + WeightLoader::finish: a good create hands the handle out; a failed one deletes it, and its upload of "a" with it (leak check)
    const char* names[2] = {"a", "b"};
    const float* ptrs[2] = {data, data};
    int64_t numel[2] = {3, 2};
    Handle* h = nullptr;
    CHECK(create(2, names, ptrs, numel, &h) == LDS_OK && h && h->own.ptrs.size() == 2 && memcmp(h->a, data, 12) == 0 && g_deleted == 0);
    delete h;
    h = nullptr;
    numel[1] = 5;
    CHECK(create(2, names, ptrs, numel, &h) == LDS_EMISSING && !h && g_deleted == 2 && said("selftest: b (wrong size)"));
    CHECK(create(1, names, ptrs, numel, &h) == LDS_EMISSING && !h && g_deleted == 3 && said("selftest: b (absent)"));
    {      // the any-size upload reports the count it took
        Owner own;
        WeightLoader W(own, 2, names, ptrs, numel);
        CHECK(W.vec("a", -1, &got) && got == 3 && own.ptrs.size() == 1 && !W.vec("nope", -1, &got) && got == 3);
    }

    // the per-clip length filler
    int v[64];
    int32_t src[64];
    for (int i = 0; i < 64; ++i) { v[i] = -7; src[i] = i % 2 ? 9 : 0; }
    CHECK(clip_lens_fill("fn", "n_frames", 64, 9, src, v) == LDS_OK && v[0] == 0 && v[1] == 9 && v[62] == 0 && v[63] == 9);
    CHECK(clip_lens_fill("fn", "lengths", 3, 9, src, v) == LDS_OK && v[1] == 9);
    for (int i = 3; i < 64; ++i) CHECK(v[i] == 0);
    src[2] = -1;
    CHECK(clip_lens_fill("fn", "n_frames", 3, 9, src, v) == LDS_EINVAL && said("fn: n_frames[2] = -1 outside 0 .. 9"));
    src[2] = 10;
    CHECK(clip_lens_fill("fn", "lengths", 3, 9, src, v) == LDS_EINVAL && said("fn: lengths[2] = 10 outside 0 .. 9"));
    CHECK(clip_lens_fill("fn", "n_frames", 3, 9, nullptr, v) == LDS_EINVAL && said("fn: null n_frames"));

    // range_check: both bounds inclusive; the texts lds_xvector_embed has always given for B = 65 and T = 0
    CHECK(range_check("t", "B", 1, 1, 64) == LDS_OK && range_check("t", "B", 64, 1, 64) == LDS_OK);
    CHECK(range_check("lds_xvector_embed", "B", 65, 1, 64) == LDS_EINVAL && said("lds_xvector_embed: B 65 outside 1 .. 64"));
    CHECK(range_check("lds_xvector_embed", "T", 0, 1, 32768) == LDS_EINVAL && said("lds_xvector_embed: T 0 outside 1 .. 32768"));
    puts("host_selftest ok");
    return 0;
}
