// Host side of liblds: weight packing, the UNet1D forward plan, the sampler loops, the front end
// and the vocoder, exported through the C ABI in include/lds.h.  Everything here only enqueues
// kernels on the caller's stream; no allocation or synchronisation happens after *_create.
#include "../../include/lds.h"
#include "../../include/lds_test.h"
#include "k4p.h"
#include "k8b3.h"
#include "kernels.h"
#include "host.h"

#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <map>
#include <mutex>
#include <string>
#include <vector>

using namespace lds;

// ------------------------------------------------------------------------------------------------
// errors
// ------------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";
int lds::set_error(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
extern "C" const char* lds_last_error(void) { return g_err; }
extern "C" int lds_version(void) { return 1; }

// ------------------------------------------------------------------------------------------------
// event profiler (off by default; bench.py turns it on for one instrumented pass)
// ------------------------------------------------------------------------------------------------
// One event marks each launch boundary.  Inside lds_sampler_run every launch is wrapped, so consecutive scopes share the
// boundary event (a kernel's stop is the next kernel's start): an interval is that kernel's execution plus its own dispatch,
// not two event packets per kernel.
struct ProfRec { std::string name; double flops, bytes; int ia, ib; };
// level 0 = off, 1 = one record per kernel family / tile configuration, 2 = names also carry the operand shapes.
// The records are process-global and guarded by g_prof_mu; with the profiler off (the product path) a launch only reads
// the atomic level, so forward calls on different streams / threads share no mutable state (include/lds.h conventions).
static std::atomic<int> g_prof_level{0};
static std::mutex g_prof_mu;
static bool g_prof_chain = false;
static std::vector<ProfRec> g_prof;
static std::vector<hipEvent_t> g_prof_ev;
static hipStream_t g_prof_last_stream = nullptr;
static int g_prof_last_stop = -1;

static int prof_mark(hipStream_t st) {      // g_prof_mu held
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) return -1;
    (void)hipEventRecord(e, st);
    g_prof_ev.push_back(e);
    return (int)g_prof_ev.size() - 1;
}
static thread_local lds::ProfScope* tl_prof_open = nullptr;
bool lds::prof_attach_events(hipEvent_t* start, hipEvent_t* stop) {
    lds::ProfScope* ps = tl_prof_open;
    if (!ps || !ps->on || ps->attached) return false;
    std::lock_guard<std::mutex> lk(g_prof_mu);
    if (ps->idx < 0 || ps->idx >= (int)g_prof.size()) return false;
    hipEvent_t e0, e1;
    if (hipEventCreate(&e0) != hipSuccess) return false;
    if (hipEventCreate(&e1) != hipSuccess) { (void)hipEventDestroy(e0); return false; }
    g_prof_ev.push_back(e0);
    g_prof[ps->idx].ia = (int)g_prof_ev.size() - 1;      // (the event marked at the scope's start is simply not read)
    g_prof_ev.push_back(e1);
    g_prof[ps->idx].ib = (int)g_prof_ev.size() - 1;
    ps->attached = true;
    g_prof_last_stop = -1;                               // a chained neighbour must not reuse a bound event as its start mark
    *start = e0; *stop = e1;
    return true;
}
lds::ProfScope::ProfScope(hipStream_t st, const char* name, double flops, double bytes, bool attachable) : on(g_prof_level.load(std::memory_order_relaxed) != 0), s(st) {
    if (!on) return;
    tl_prof_open = this;
    std::lock_guard<std::mutex> lk(g_prof_mu);
    ProfRec r;
    r.name = name; r.flops = flops; r.bytes = bytes; r.ib = -1;
    r.ia = attachable ? -1 : ((g_prof_chain && g_prof_last_stop >= 0 && g_prof_last_stream == st) ? g_prof_last_stop : prof_mark(st));
    if (r.ia < 0 && !attachable) { on = false; return; }
    if (attachable) g_prof_last_stop = -1;      // no stream event here: a chained neighbour records its own start
    g_prof.push_back(r);
    idx = (int)g_prof.size() - 1;
}
lds::ProfScope::~ProfScope() {
    if (tl_prof_open == this) tl_prof_open = nullptr;
    if (!on || attached) return;
    std::lock_guard<std::mutex> lk(g_prof_mu);
    if (idx < 0 || idx >= (int)g_prof.size()) return;      // the profiler was reset while this scope was open
    if (g_prof[idx].ia < 0) return;                         // attachable scope whose launcher took no events: the record stays empty
    g_prof[idx].ib = prof_mark(s);
    g_prof_last_stop = g_prof[idx].ib;
    g_prof_last_stream = s;
}
void lds::ProfScope::rename(const std::string& n) {
    if (!on) return;
    std::lock_guard<std::mutex> lk(g_prof_mu);
    if (idx >= 0 && idx < (int)g_prof.size()) g_prof[idx].name = n;
}
struct ProfChain {      // RAII: boundary events are shared while alive
    bool prev = false, act;
    ProfChain() : act(g_prof_level.load(std::memory_order_relaxed) != 0) {
        if (!act) return;
        std::lock_guard<std::mutex> lk(g_prof_mu);
        prev = g_prof_chain; g_prof_chain = true; g_prof_last_stop = -1;
    }
    ~ProfChain() {
        if (!act) return;
        std::lock_guard<std::mutex> lk(g_prof_mu);
        g_prof_chain = prev; g_prof_last_stop = -1;
    }
};

extern "C" int lds_prof_enable(int on) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    for (hipEvent_t e : g_prof_ev) (void)hipEventDestroy(e);
    g_prof_ev.clear();
    g_prof.clear();
    g_prof_last_stop = -1;
    g_prof_level.store(on < 0 ? 0 : (on > 2 ? 2 : on));
    return LDS_OK;
}

// JSON: [{"name":..., "count":n, "ms":total, "flops":total, "bytes":total}, ...]; synchronises the recorded events.
extern "C" int lds_prof_summary(char* buf, size_t cap) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    struct Agg { long long n = 0; double ms = 0, fl = 0, by = 0; };
    std::map<std::string, Agg> agg;
    for (auto& r : g_prof) {
        float ms = 0.f;
        if (r.ia < 0 && r.ib < 0) continue;      // an attachable scope whose launcher did not take the events (nothing was launched)
        if (r.ib < 0 || hipEventSynchronize(g_prof_ev[r.ib]) != hipSuccess || hipEventElapsedTime(&ms, g_prof_ev[r.ia], g_prof_ev[r.ib]) != hipSuccess)
            return set_error(LDS_EHIP, "profiler event read failed");
        Agg& a = agg[r.name];
        a.n++; a.ms += ms; a.fl += r.flops; a.by += r.bytes;
    }
    std::string out = "[";
    bool first = true;
    for (auto& kv : agg) {
        char line[512];
        snprintf(line, sizeof(line), "%s{\"name\":\"%s\",\"count\":%lld,\"ms\":%.6f,\"flops\":%.6e,\"bytes\":%.6e}", first ? "" : ",",
                 kv.first.c_str(), kv.second.n, kv.second.ms, kv.second.fl, kv.second.by);
        out += line;
        first = false;
    }
    out += "]";
    if (out.size() + 1 > cap) return set_error(LDS_ENOMEM, "profile summary needs %zu bytes", out.size() + 1);
    memcpy(buf, out.c_str(), out.size() + 1);
    return LDS_OK;
}

// ------------------------------------------------------------------------------------------------
// weight packing (Owner, Tensors: host.h)
// ------------------------------------------------------------------------------------------------
// packed conv / linear weights: [KT][Ci][Mp] + bias[Mp]
struct ConvW {
    float* w = nullptr;
    float* bias = nullptr;
    int Co = 0, Ci = 0, K = 1, Mp = 0;
    void* w3 = nullptr;      // the same weights as three bf16 planes [KT][Ci/8][3][Mp][8] (split-bf16 path, conv_bf3.hip)
    void* wh = nullptr;      // ... as two fp16 planes [KT][Ci/8][2][Mp][8] of (w * 2^k); wh_inv = 2^-k undoes the scale in the epilogue
    float wh_inv = 1.0f;
    float* wu = nullptr;     // a k 3 convolution's Winograd F(2,3) taps U0..U3, packed [4][Ci][Mp] like w (pack_wino; conv_wino.hip)
};

static int round_mp(int Co) { return Co <= 32 ? 32 : (Co + 63) / 64 * 64; }

// packed weight index (see conv_gemm.hip, "k-interleaved tiles"): [tap][k/8][k%2][Mp][(k%8)/2]
static inline size_t widx(int tap, int k, int m, int Ci, int Mp) {
    return ((((size_t)tap * (Ci / 8) + k / 8) * 2 + (k & 1)) * Mp + m) * 4 + ((k & 7) >> 1);
}

// Split twins of a packed fp32 weight set (k8b3.h): three bf16 planes [tap][Ci/8][3][Mp][8], or two fp16 planes [tap][Ci/8][2][Mp][8] of
// the weights times a power of two that puts the largest one in [2^13, 2^14) (fp16's exponent range; `scale_override` != 0 forces the
// factor: a resnet's conv2 and shortcut share one because they accumulate into the same registers).  `p` = the fp32 packed host copy (widx).
static float f16_weight_scale(const std::vector<float>& p) {
    float mx = 0.f;
    for (float v : p) mx = std::max(mx, fabsf(v));
    if (!(mx > 0.f) || !std::isfinite(mx)) return 1.0f;
    return ldexpf(1.0f, 13 - (int)floorf(log2f(mx)));
}
static bool pack_split_from_packed(Owner& o, const std::vector<float>& p, int K, int Ci, int Mp, int fmt, float scale_override, ConvW& out) {
    const int npl = fmt_planes(fmt);
    const float sc = (fmt == FMT_F16X2) ? (scale_override != 0.f ? scale_override : f16_weight_scale(p)) : 1.0f;
    std::vector<uint16_t> q((size_t)K * Ci * Mp * npl, 0);
    for (int tap = 0; tap < K; ++tap)
        for (int ci = 0; ci < Ci; ++ci)
            for (int m = 0; m < Mp; ++m) {
                uint16_t t3[3] = {0, 0, 0};
                const float v = p[widx(tap, ci, m, Ci, Mp)];
                if (fmt == FMT_F16X2) split2h_host(v * sc, t3);
                else split3_host(v, t3);
                for (int pl = 0; pl < npl; ++pl) q[((((size_t)tap * (Ci / 8) + ci / 8) * npl + pl) * Mp + m) * 8 + (ci & 7)] = t3[pl];
            }
    void* d = o.upload_bytes(q.data(), q.size() * sizeof(uint16_t));
    if (!d) return false;
    if (fmt == FMT_F16X2) { out.wh = d; out.wh_inv = 1.0f / sc; }
    else out.w3 = d;
    return true;
}
static bool read_back(const ConvW& W, std::vector<float>& p) {      // (the packers keep no host copy)
    p.resize((size_t)W.K * W.Ci * W.Mp);
    return W.w && hipMemcpy(p.data(), W.w, p.size() * sizeof(float), hipMemcpyDeviceToHost) == hipSuccess;
}
static bool make_split_twin(Owner& o, ConvW& W, int fmt, float scale_override = 0.f) {
    if (fmt == FMT_F16X2 ? W.wh != nullptr : W.w3 != nullptr) return true;
    std::vector<float> p;
    return read_back(W, p) && pack_split_from_packed(o, p, W.K, W.Ci, W.Mp, fmt, scale_override, W);
}
static bool make_bf3_twin(Owner& o, ConvW& W) { return make_split_twin(o, W, FMT_BF16X3); }
// conv2 + shortcut of a resnet: one common fp16 weight scale (they share accumulators in the fused launch)
static bool make_split_twin_pair(Owner& o, ConvW& A, ConvW& Bw, int fmt) {
    if (fmt != FMT_F16X2) return make_split_twin(o, A, fmt) && make_split_twin(o, Bw, fmt);
    std::vector<float> pa, pb;
    if (!read_back(A, pa) || !read_back(Bw, pb)) return false;
    const float sc = std::min(f16_weight_scale(pa), f16_weight_scale(pb));
    return pack_split_from_packed(o, pa, A.K, A.Ci, A.Mp, fmt, sc, A) && pack_split_from_packed(o, pb, Bw.K, Bw.Ci, Bw.Mp, fmt, sc, Bw);
}

// reference layout w[Co][Ci][K] (or [Co][Ci] for Linear) -> packed
static bool pack_conv(Owner& o, const float* w, const float* b, int Co, int Ci, int K, ConvW& out) {
    const int Mp = round_mp(Co);
    std::vector<float> p((size_t)K * Ci * Mp, 0.f), pb(Mp, 0.f);
    for (int co = 0; co < Co; ++co)
        for (int ci = 0; ci < Ci; ++ci)
            for (int k = 0; k < K; ++k) p[widx(k, ci, co, Ci, Mp)] = w[((size_t)co * Ci + ci) * K + k];
    if (b)
        for (int co = 0; co < Co; ++co) pb[co] = b[co];
    out.w = o.upload(p);
    out.bias = b ? o.upload(pb) : nullptr;
    out.Co = Co; out.Ci = Ci; out.K = K; out.Mp = Mp;
    return out.w && (!b || out.bias);
}

// Winograd F(2,3) taps of a k 3 convolution (conv_wino.hip), reference layout g[Co][Ci][3] -> U[4][Co][Ci]:
// U0 = g0, U1 = (g0 + g1 + g2) / 2, U2 = (g0 - g1 + g2) / 2, U3 = g2, computed in double and rounded once to fp32
static void wino_taps(const float* g, int Co, int Ci, std::vector<float>& U) {
    const size_t n = (size_t)Co * Ci;
    U.assign(4 * n, 0.f);
    for (size_t i = 0; i < n; ++i) {
        const double g0 = g[3 * i], g1 = g[3 * i + 1], g2 = g[3 * i + 2];
        U[i] = (float)g0;
        U[n + i] = (float)((g0 + g1 + g2) * 0.5);
        U[2 * n + i] = (float)((g0 - g1 + g2) * 0.5);
        U[3 * n + i] = (float)g2;
    }
}
// ... packed next to the direct weights of `out` (which stay: latency mode, the split modes and the shapes that are not routed use them)
static bool pack_wino(Owner& o, const float* w, int Co, int Ci, ConvW& out) {
    std::vector<float> U;
    wino_taps(w, Co, Ci, U);
    const int Mp = out.Mp;
    std::vector<float> p((size_t)4 * Ci * Mp, 0.f);
    for (int j = 0; j < 4; ++j)
        for (int co = 0; co < Co; ++co)
            for (int ci = 0; ci < Ci; ++ci) p[widx(j, ci, co, Ci, Mp)] = U[((size_t)j * Co + co) * Ci + ci];
    out.wu = o.upload(p);
    return out.wu != nullptr;
}
// conv2 + the 1x1 shortcut of a resnet as ONE Winograd reduction over Cm + Cin / 2 channels.  conv_wino joins Y[2i] = M0 + M1 + M2
// and Y[2i+1] = M1 - M2 - M3, so an addend on M0 reaches the even frame, one on M3 (negated) the odd frame, and a pair (A on M1, B on M2)
// puts A + B into the even and A - B into the odd frame.  With x_e[i] = x[2i], x_o[i] = x[2i+1] of the raw block input and its channels
// split into a first half A and a second half B, the shortcut S rides as
//   tap 0: S_A . x_e(A)     tap 1: S_B / 2 . (x_e(B) + x_o(B))     tap 2: S_B / 2 . (x_e(B) - x_o(B))     tap 3: -S_A . x_o(A)
// two products per output pair like the direct form, but Cin / 2 deep on every one of the four waves.
// g [Co][Cm][3], S [Co][Cin] -> U [4][Co][Cm + Cin/2]: wino_taps(g), then the extension; S_B halved in double and rounded once (exact)
static void wino_pair_taps(const float* g, const float* S, int Co, int Cm, int Cin, std::vector<float>& U) {
    std::vector<float> U3;
    wino_taps(g, Co, Cm, U3);
    const int half = Cin / 2, Ck = Cm + half;
    U.assign((size_t)4 * Co * Ck, 0.f);
    for (int j = 0; j < 4; ++j)
        for (int co = 0; co < Co; ++co) {
            float* row = &U[((size_t)j * Co + co) * Ck];
            memcpy(row, &U3[((size_t)j * Co + co) * Cm], sizeof(float) * Cm);
            for (int e = 0; e < half; ++e) {
                const double sa = S[(size_t)co * Cin + e], sb = S[(size_t)co * Cin + half + e];
                row[Cm + e] = (float)(j == 0 ? sa : j == 3 ? -sa : sb * 0.5);
            }
        }
}
static float* pack_wino_pair(Owner& o, const float* w2, const float* ws, int Co, int Cm, int Cin, int Mp) {
    std::vector<float> U;
    wino_pair_taps(w2, ws, Co, Cm, Cin, U);
    const int Ck = Cm + Cin / 2;
    std::vector<float> p((size_t)4 * Ck * Mp, 0.f);
    for (int j = 0; j < 4; ++j)
        for (int co = 0; co < Co; ++co)
            for (int ci = 0; ci < Ck; ++ci) p[widx(j, ci, co, Ck, Mp)] = U[((size_t)j * Co + co) * Ck + ci];
    return o.upload(p);
}

// GEGLU projection (reference attention.py:280-301): rows [0,4C) are the value half, [4C,8C) the gate.
// Interleave them in 32-row groups so one wave's two MFMA row tiles hold value and gate of the same channels.
static bool pack_geglu(Owner& o, const float* w, const float* b, int C8, int Ci, ConvW& out) {
    const int half = C8 / 2;
    std::vector<float> p((size_t)Ci * C8, 0.f), pb(C8, 0.f);
    for (int m = 0; m < C8; ++m) {
        const int q = m / 64, s = (m % 64) / 32, r = m % 32;
        const int src = (s == 0 ? 0 : half) + 32 * q + r;
        for (int ci = 0; ci < Ci; ++ci) p[widx(0, ci, m, Ci, C8)] = w[(size_t)src * Ci + ci];
        pb[m] = b[src];
    }
    out.w = o.upload(p);
    out.bias = o.upload(pb);
    out.Co = C8; out.Ci = Ci; out.K = 1; out.Mp = C8;
    return out.w && out.bias;
}

// LayerNorm folded into a following linear layer: weights pre-multiplied by gamma, plus the two per-row constants of
// DmaConvArgs (c1 = sum_c W*gamma, c2 = sum_c W*beta + bias).  `perm[m]` = source row of packed row m.
static bool pack_ln_fold(Owner& o, const float* w, const float* b, const float* gamma, const float* beta, int Co, int Ci,
                         const std::vector<int>& perm, ConvW& out, float*& c1_out, float*& c2_out) {
    const int Mp = round_mp(Co);
    std::vector<float> p((size_t)Ci * Mp, 0.f), c1(Mp, 0.f), c2(Mp, 0.f);
    for (int m = 0; m < Co; ++m) {
        const int src = perm.empty() ? m : perm[m];
        double s1 = 0, s2 = b ? (double)b[src] : 0.0;
        for (int ci = 0; ci < Ci; ++ci) {
            const float wg = w[(size_t)src * Ci + ci] * gamma[ci];
            p[widx(0, ci, m, Ci, Mp)] = wg;
            s1 += (double)wg;
            s2 += (double)w[(size_t)src * Ci + ci] * (double)beta[ci];
        }
        c1[m] = (float)s1; c2[m] = (float)s2;
    }
    out.w = o.upload(p);
    out.bias = nullptr;
    out.Co = Co; out.Ci = Ci; out.K = 1; out.Mp = Mp;
    c1_out = o.upload(c1);
    c2_out = o.upload(c2);
    return out.w && c1_out && c2_out;
}

// GroupNorm (affine, no activation) folded into a following 1x1 convolution (DmaConvArgs::gnf_part): weights pre-multiplied by gamma,
// cg[g][m] = sum_{c in group g} W[m,c] gamma_c (what the group's mean multiplies) and c2[m] = sum_c W[m,c] beta_c + bias[m]
static bool pack_gn_fold(Owner& o, const float* w, const float* b, const float* gamma, const float* beta, int Co, int Ci, int groups, ConvW& out,
                         float*& cg_out, float*& c2_out) {
    const int Mp = round_mp(Co), gsz = Ci / groups;
    std::vector<float> p((size_t)Ci * Mp, 0.f), cg((size_t)groups * Mp, 0.f), c2(Mp, 0.f);
    for (int m = 0; m < Co; ++m) {
        double s2 = b ? (double)b[m] : 0.0;
        for (int g = 0; g < groups; ++g) {
            double s1 = 0;
            for (int ci = g * gsz; ci < (g + 1) * gsz; ++ci) {
                const float wg = w[(size_t)m * Ci + ci] * gamma[ci];
                p[widx(0, ci, m, Ci, Mp)] = wg;
                s1 += (double)wg;
                s2 += (double)w[(size_t)m * Ci + ci] * (double)beta[ci];
            }
            cg[(size_t)g * Mp + m] = (float)s1;
        }
        c2[m] = (float)s2;
    }
    out.w = o.upload(p);
    out.bias = nullptr;
    out.Co = Co; out.Ci = Ci; out.K = 1; out.Mp = Mp;
    cg_out = o.upload(cg);
    c2_out = o.upload(c2);
    return out.w && cg_out && c2_out;
}

// ConvTranspose1d (reference models.py:233-236) as `stride` interleaved phase filters of K/stride taps:
// packed[tap][ci][co*stride + phi] = w[ci][co][phi + stride*(KT-1-tap)]
static bool pack_convT(Owner& o, const float* w, const float* b, int Ci, int Co, int K, int stride, ConvW& out) {
    const int KT = K / stride, M = Co * stride, Mp = round_mp(M);
    std::vector<float> p((size_t)KT * Ci * Mp, 0.f), pb(Mp, 0.f);
    for (int tap = 0; tap < KT; ++tap)
        for (int ci = 0; ci < Ci; ++ci)
            for (int co = 0; co < Co; ++co)
                for (int phi = 0; phi < stride; ++phi)
                    p[widx(tap, ci, co * stride + phi, Ci, Mp)] = w[((size_t)ci * Co + co) * K + phi + stride * (KT - 1 - tap)];
    for (int co = 0; co < Co; ++co)
        for (int phi = 0; phi < stride; ++phi) pb[co * stride + phi] = b ? b[co] : 0.f;
    out.w = o.upload(p);
    out.bias = o.upload(pb);
    out.Co = M; out.Ci = Ci; out.K = KT; out.Mp = Mp;
    return out.w && out.bias;
}

// ------------------------------------------------------------------------------------------------
// conv helper
// ------------------------------------------------------------------------------------------------
struct Src {
    const float* x1; int C1; const float* x2; int C2; int Tsrc;
};
struct ConvOpt {
    int stride = 1, pad = 0, dil = 1, ups = 0;
    int act_in = ACT_NONE; float slope = 0.f;
    const float* bias_bc = nullptr; const float* res = nullptr;
    int epi = EPI_NONE; int accum = 0; float out_div = 1.f;
    int phases = 1, tpad = 0; int To = -1; int Tout = -1; int tile = 0;
    int Cout = -1;
    const int* vlen = nullptr; const int* vlen_in = nullptr;      // ragged batches: valid output / input frames per batch element (kernels.h ConvArgs)
};

static int run_conv(const ConvW& W, const Src& s, const ConvOpt& o, float* out, int B, hipStream_t st) {
    ConvArgs a;
    memset(&a, 0, sizeof(a));
    a.x1 = s.x1; a.x2 = s.x2 ? s.x2 : s.x1; a.C1 = s.C1; a.C2 = s.C2; a.Tsrc = s.Tsrc;
    a.Tin = o.ups ? 2 * s.Tsrc : s.Tsrc;
    a.xb1 = (long long)s.C1 * s.Tsrc; a.xb2 = (long long)s.C2 * s.Tsrc;
    a.w = W.w; a.Mp = W.Mp; a.Co = W.Co; a.Ci = W.Ci; a.KT = W.K;
    a.stride = o.stride; a.dil = o.dil; a.pad = o.pad; a.ups = o.ups;
    a.act_in = o.act_in; a.slope = o.slope;
    a.bias = W.bias; a.bias_bc = o.bias_bc; a.res = o.res; a.epi = o.epi; a.accum = o.accum; a.out_div = o.out_div;
    a.out = out;
    if (s.C1 + s.C2 != W.Ci) return set_error(LDS_EINVAL, "conv: input channels %d+%d != %d", s.C1, s.C2, W.Ci);
    const int To_nat = (a.Tin + 2 * o.pad - o.dil * (W.K - 1) - 1) / o.stride + 1;
    a.To = o.To > 0 ? o.To : To_nat;
    a.Tout = o.Tout > 0 ? o.Tout : a.To;
    a.phases = o.phases; a.tpad = o.tpad;
    a.Cout = o.Cout > 0 ? o.Cout : W.Co / o.phases;
    a.B = B;
    a.vlen = o.vlen; a.vlen_in = o.vlen_in;
    const double real_rows = (o.phases > 1) ? (double)W.Co : (double)(a.Cout);
    const double flops = 2.0 * B * (double)a.To * real_rows * (double)W.Ci * (double)W.K;
    const double bytes = 4.0 * ((double)B * W.Ci * s.Tsrc + (double)W.K * W.Ci * W.Co + (double)B * a.Cout * a.Tout * (o.res ? 2.0 : 1.0));
    hipError_t e;
    {
        const bool mono = o.tile == 0 && conv_mono_applies(a);        // conv_post: one output channel, a stream
        const bool small = mono || (o.tile == 0 && conv_small_applies(a));      // narrow vocoder stages: register-resident weights, 16x16x4 MFMA
        ProfScope ps(st, mono ? "conv_mono" : small ? "conv_small" : "conv_gemm", flops, bytes);
        e = mono ? launch_conv_mono(a, st) : small ? launch_conv_small(a, st) : launch_conv_gemm(a, o.tile, st);
        if (ps.on) {
            std::string cfgs(small ? conv_small_last_config() : conv_gemm_last_config());   // "BM.. BN.. KT.. S.. U.. grid ..."
            std::string nm = std::string(mono ? "conv_mono<" : small ? "conv_small<" : "conv_gemm<") + cfgs.substr(0, cfgs.find(" grid")) + ">";
            if (g_prof_level.load(std::memory_order_relaxed) >= 2) {      // per-shape breakdown (bench.py's vocoder leg, tuning sessions)
                char sh[96];
                snprintf(sh, sizeof(sh), " Ci%d Co%d K%d d%d To%d%s%s", W.Ci, W.Co, W.K, o.dil, a.To, o.phases > 1 ? " convT" : "", o.res ? " +res" : "");
                nm += sh;
            }
            ps.rename(nm);
        }
    }
    if (e != hipSuccess)
        return set_error(LDS_EHIP, "conv_gemm launch failed (%s): Co %d Ci %d K %d stride %d dil %d ups %d To %d", hipGetErrorString(e), W.Co,
                    W.Ci, W.K, o.stride, o.dil, o.ups, a.To);
    return LDS_OK;
}

// DMA-fed K4P convolution (conv_dma.hip)
struct DOpt {
    int stride = 1, pad = 0, ups = 0;
    const float* res = nullptr;
    int epi = EPI_NONE, out_plain = 0, plain_from = -1;
    float* out2 = nullptr;
    int vt_D = 0;
    float2* lnpart_out = nullptr;
    float2* gnpart_out = nullptr;
    int voc = 0, dil = 1, xpad = 1, opad = 1;
    float act_slope = 0.f; float* out_act = nullptr; const float* acc_in = nullptr; float out_div = 1.f;
    int ph_log2 = 0, ph_tpad = 0, ph_Tout = 0;      // polyphase ConvTranspose output (kernels.h)
    const float2* ln_part = nullptr; int ln_np = 0; float ln_eps = 1e-5f; const float* ln_c1 = nullptr; const float* ln_c2 = nullptr;
    const float2* gnf_part = nullptr; int gnf_groups = 0; float gnf_eps = 1e-5f; const float* gnf_cg = nullptr; const float* gnf_c2 = nullptr;   // GroupNorm fold
    int cfg = 0;
    int lvl_in = 0, lvl_out = 0;      // ragged batches: UNet levels of the input / output tensors (k4p.h ragged_len)
    const int* vlen = nullptr;        // ... vocoder: valid output frames per batch element, given outright
    int out_f32 = 0;      // split-bf16 path: the K4P-range output channels stay fp32 K4P (q / k for the attention kernel)
};
// Batch size the launchers judge their tile / split choices at while a UNet call of this thread is running: 0 = the nominal batch (the
// default: results do not depend on the batch split), the actual batch in latency mode (lds_unet_set_latency_mode).
static std::atomic<int> g_touch_w{0};       // lds_debug_set_touch_weights: experiment, off in the product path
static std::atomic<int> g_voc_pair{1};     // lds_debug_set_voc_pair: 0 = the narrow vocoder stages' residual steps as two launches (A/B measurements, tests)
static std::atomic<int> g_gn_fold{1};      // lds_debug_set_gn_fold: 0 = the transformer's GroupNorm as its own pass (A/B measurements, tests)
// per-utterance lengths of the ragged batch a UNet call of this thread is running on (device int32 [B]; null = none): k4p.h ragged_len
static thread_local const int* tl_lens = nullptr;
struct LensScope {
    const int* prev;
    explicit LensScope(const int* l) : prev(tl_lens) { tl_lens = l; }
    ~LensScope() { tl_lens = prev; }
};
static thread_local int tl_tile_batch = 0;
// ... and the scratch of the latency mode's cluster split-K (kernels.h DmaConvArgs::ksplit): partial tiles + arrival counters
constexpr long long kClusterPartFloats = 4ll << 20;      // 16 MB: 320 workgroups x 4 waves x 1024 floats = 1.3 M floats are ever in use
constexpr int kClusterCounters = 4096;
static thread_local float* tl_kpart = nullptr;
static thread_local unsigned* tl_kcount = nullptr;
struct TileBatchScope {
    int prev; float* pp; unsigned* pc;
    explicit TileBatchScope(int tb, float* kpart = nullptr, unsigned* kcount = nullptr) : prev(tl_tile_batch), pp(tl_kpart), pc(tl_kcount) {
        tl_tile_batch = tb; tl_kpart = tb ? kpart : nullptr; tl_kcount = tb ? kcount : nullptr;
    }
    ~TileBatchScope() { tl_tile_batch = prev; tl_kpart = pp; tl_kcount = pc; }
};

// Debug trace (include/lds_test.h lds_debug_trace): while on, a UNet forward synchronises after every stage and keeps a host copy of the
// stage's output tensor, so that two runs (two modes, two workspace fill patterns) can be compared stage by stage.  Off in the product path:
// a forward then only reads the atomic flag.
static std::atomic<int> g_trace_on{0};
struct TraceRec { std::string name; std::vector<char> bytes; };
static std::mutex g_trace_mu;
static std::vector<TraceRec> g_trace;
static thread_local std::string tl_trace_stage;
static int trace_out(hipStream_t st, const char* what, const void* dev, size_t bytes) {
    if (!g_trace_on.load(std::memory_order_relaxed)) return LDS_OK;
    HIP_TRY(hipStreamSynchronize(st));
    TraceRec r;
    r.name = tl_trace_stage + "." + what;
    r.bytes.resize(bytes);
    HIP_TRY(hipMemcpy(r.bytes.data(), dev, bytes, hipMemcpyDeviceToHost));
    std::lock_guard<std::mutex> lk(g_trace_mu);
    g_trace.push_back(std::move(r));
    return LDS_OK;
}
extern "C" int lds_debug_trace(int on) {
    std::lock_guard<std::mutex> lk(g_trace_mu);
    if (on) g_trace.clear();
    g_trace_on.store(on ? 1 : 0);
    return LDS_OK;
}
extern "C" int lds_debug_trace_count(void) {
    std::lock_guard<std::mutex> lk(g_trace_mu);
    return (int)g_trace.size();
}
extern "C" int lds_debug_trace_get(int i, char* name, size_t name_cap, const void** data, size_t* bytes) {
    std::lock_guard<std::mutex> lk(g_trace_mu);
    if (i < 0 || i >= (int)g_trace.size() || !name || !data || !bytes || name_cap == 0) return set_error(LDS_EINVAL, "bad argument");
    snprintf(name, name_cap, "%s", g_trace[i].name.c_str());
    *data = g_trace[i].bytes.data();
    *bytes = g_trace[i].bytes.size();
    return LDS_OK;
}
// every 32-bit word of a device buffer = pattern (tests poison a workspace with NaN patterns: a kernel that reads what no kernel of the call wrote shows)
extern "C" int lds_debug_fill_u32(void* dev, size_t n_words, uint32_t pattern, void* stream) {
    if (!dev) return set_error(LDS_EINVAL, "bad argument");
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)dev, (int)pattern, n_words, (hipStream_t)stream));
    return LDS_OK;
}

static int fill_dconv(const ConvW& W, const float* x1, int C1, const float* x2, int C2, int Tsrc, const DOpt& o, float* out, int B, DmaConvArgs& a) {
    memset(&a, 0, sizeof(a));
    a.tile_batch = tl_tile_batch;
    a.lens = tl_lens; a.lvl_in = o.lvl_in; a.lvl_out = o.lvl_out;
    a.vlen = o.vlen;
    a.kpart = tl_kpart; a.kcount = tl_kcount; a.kpart_cap = kClusterPartFloats; a.kcount_cap = kClusterCounters;
    if (C1 + C2 != W.Ci) return set_error(LDS_EINVAL, "dconv: input channels %d+%d != %d", C1, C2, W.Ci);
    a.x1 = x1; a.x2 = x2 ? x2 : x1; a.C1 = C1; a.C2 = C2; a.Tsrc = Tsrc;
    a.w = W.w; a.bias = W.bias; a.Mp = W.Mp; a.Co = W.Co; a.Ci = W.Ci; a.KT = W.K;
    a.stride = o.stride; a.pad = o.pad; a.ups = o.ups;
    a.res = o.res; a.epi = o.epi; a.out = out; a.out_plain = o.out_plain;
    a.Cout = (o.epi == EPI_GEGLU || o.epi == EPI_GLU) ? W.Co / 2 : W.Co;
    a.plain_from = (o.plain_from >= 0) ? o.plain_from : a.Cout;
    a.out2 = o.out2; a.vt_D = o.vt_D; a.lnpart_out = o.lnpart_out; a.gnpart_out = o.gnpart_out;
    a.voc = o.voc; a.dil = o.dil; a.xpad = o.xpad; a.opad = o.opad; a.act_slope = o.act_slope; a.out_act = o.out_act; a.acc_in = o.acc_in; a.out_div = o.out_div;
    a.ln_part = o.ln_part; a.ln_np = o.ln_np; a.ln_eps = o.ln_eps; a.ln_c1 = o.ln_c1; a.ln_c2 = o.ln_c2;
    a.gnf_part = o.gnf_part; a.gnf_groups = o.gnf_groups; a.gnf_eps = o.gnf_eps; a.gnf_cg = o.gnf_cg; a.gnf_c2 = o.gnf_c2;
    a.ph_log2 = o.ph_log2; a.ph_tpad = o.ph_tpad; a.ph_Tout = o.ph_Tout; a.ph_Cout = o.ph_Tout ? (W.Co >> o.ph_log2) : 0;
    const int Tin = o.ups ? 2 * Tsrc : Tsrc;
    a.To = (Tin + 2 * o.pad - o.dil * (W.K - 1) - 1) / o.stride + 1;
    a.B = B;
    return LDS_OK;
}
static int run_dconv(const ConvW& W, const float* x1, int C1, const float* x2, int C2, int Tsrc, const DOpt& o, float* out, int B,
                     hipStream_t st) {
    DmaConvArgs a;
    int rc = fill_dconv(W, x1, C1, x2, C2, Tsrc, o, out, B, a);
    if (rc != LDS_OK) return rc;
    const double flops = 2.0 * B * (double)a.To * (double)W.Co * (double)W.Ci * (double)W.K;
    const double bytes = 4.0 * ((double)B * W.Ci * Tsrc + (double)W.K * W.Ci * W.Co + (double)B * a.Cout * a.To * (o.res ? 2.0 : 1.0));
    hipError_t e;
    if (g_touch_w.load(std::memory_order_relaxed)) HIP_TRY(launch_touch_lines(W.w, 4ll * W.K * W.Ci * W.Mp, st));
    {
        ProfScope ps(st, "conv_dma", flops, bytes, true);
        e = launch_conv_dma(a, o.cfg, st);
        if (ps.on) {
            std::string cfgs(conv_dma_last_config());
            std::string nm = "conv_dma<" + cfgs.substr(0, cfgs.find(" grid")) + ">";
            if (g_prof_level.load(std::memory_order_relaxed) >= 2) {
                char sh[96];
                snprintf(sh, sizeof(sh), " Ci%d Co%d K%d To%d%s%s%s", W.Ci, W.Co, W.K, a.To, o.res ? " +res" : "", o.acc_in ? " +acc" : "", o.ph_Tout ? " convT" : "");
                nm += sh;
            }
            ps.rename(nm);
        }
    }
    if (e != hipSuccess)
        return set_error(LDS_EHIP, "conv_dma launch failed (%s): Co %d Ci %d K %d stride %d ups %d To %d", hipGetErrorString(e), W.Co, W.Ci, W.K,
                    o.stride, o.ups, a.To);
    return LDS_OK;
}
// the same operator on the split-bf16 path (conv_bf3.hip): K8B3 activations, W.w3 weights
static int run_dconv_bf3(const ConvW& W, const void* x1, int C1, const void* x2, int C2, int Tsrc, const DOpt& o, void* out, int B, hipStream_t st,
                         int nprod = 0, int fmt = FMT_BF16X3) {
    DmaConvArgs a;
    int rc = fill_dconv(W, (const float*)x1, C1, (const float*)x2, C2, Tsrc, o, (float*)out, B, a);
    if (rc != LDS_OK) return rc;
    const void* wsp = (fmt == FMT_F16X2) ? W.wh : W.w3;
    if (!wsp) return set_error(LDS_EINVAL, "split weights were not packed for this layer");
    a.w = (const float*)wsp;
    a.x2 = (const float*)x2;      // null = one source (fill_dconv aliases x1 for the fp32 kernel)
    a.out_f32 = o.out_f32;
    a.acc_scale = (fmt == FMT_F16X2) ? W.wh_inv : 0.f;
    const double flops = 2.0 * B * (double)a.To * (double)W.Co * (double)W.Ci * (double)W.K;
    const double bytes = 2.0 * fmt_planes(fmt) * ((double)B * W.Ci * Tsrc + (double)W.K * W.Ci * W.Co + (double)B * a.Cout * a.To * (o.res ? 2.0 : 1.0));
    hipError_t e;
    {
        ProfScope ps(st, "conv_bf3", flops, bytes, true);
        e = launch_conv_bf3(a, o.cfg, nprod, fmt, st);
        if (ps.on) {
            std::string cfgs(conv_bf3_last_config());
            std::string nm = "conv_bf3<" + cfgs.substr(0, cfgs.find(" grid")) + ">";
            if (g_prof_level.load(std::memory_order_relaxed) >= 2) {
                char sh[96];
                snprintf(sh, sizeof(sh), " Ci%d Co%d K%d To%d%s", W.Ci, W.Co, W.K, a.To, o.res ? " +res" : "");
                nm += sh;
            }
            ps.rename(nm);
        }
    }
    if (e != hipSuccess)
        return set_error(LDS_EHIP, "conv_bf3 launch failed (%s): Co %d Ci %d K %d stride %d ups %d To %d cfg %d", hipGetErrorString(e), W.Co, W.Ci, W.K, o.stride,
                    o.ups, a.To, o.cfg);
    return LDS_OK;
}
// conv2 (k 3 over h) and the 1x1 shortcut (over the block input x1 ; x2) of a resnet in one launch: out = W2 * h + Ws * [x1 ; x2] + bias.
// Returns 1 when there is no fused variant for these shapes (the caller then runs the two convolutions separately).
static int run_dconv_pair(const ConvW& W3, const float* h, const ConvW& W1, const float* x1, int C1, const float* x2, int C2, int T, const float* bias_pair,
                          float2* gnpart_out, float* out, int B, hipStream_t st, int lvl = 0) {
    DmaConvArgs a3, a1;
    DOpt o3;
    o3.lvl_in = o3.lvl_out = lvl;
    o3.pad = 1;
    int rc = fill_dconv(W3, h, W3.Ci, nullptr, 0, T, o3, out, B, a3);
    if (rc != LDS_OK) return rc;
    DOpt o1;
    o1.lvl_in = o1.lvl_out = lvl;
    o1.gnpart_out = gnpart_out;
    rc = fill_dconv(W1, x1, C1, x2, C2, T, o1, out, B, a1);
    if (rc != LDS_OK) return rc;
    a3.bias = nullptr;
    a1.bias = bias_pair;
    const double flops = 2.0 * B * (double)a1.To * (double)W3.Co * ((double)W3.Ci * 3.0 + (double)W1.Ci);
    const double bytes = 4.0 * ((double)B * (W3.Ci + W1.Ci) * T + (double)W3.Co * (3.0 * W3.Ci + W1.Ci) + (double)B * a1.Cout * a1.To);
    if (!conv_dma_pair_applies(a3, a1)) return 1;
    hipError_t e;
    if (g_touch_w.load(std::memory_order_relaxed)) {
        HIP_TRY(launch_touch_lines(W3.w, 4ll * W3.K * W3.Ci * W3.Mp, st));
        HIP_TRY(launch_touch_lines(W1.w, 4ll * W1.K * W1.Ci * W1.Mp, st));
    }
    {
        ProfScope ps(st, "conv_dma", flops, bytes, true);
        e = launch_conv_dma_pair(a3, a1, st);
        if (ps.on) {
            std::string cfgs(conv_dma_last_config());
            std::string nm = "conv_dma<" + cfgs.substr(0, cfgs.find(" grid")) + ">";
            if (g_prof_level.load(std::memory_order_relaxed) >= 2) {
                char sh[96];
                snprintf(sh, sizeof(sh), " Ci%d+%d Co%d K3+1 To%d", W3.Ci, W1.Ci, W3.Co, a1.To);
                nm += sh;
            }
            ps.rename(nm);
        }
    }
    if (e != hipSuccess) return set_error(LDS_EHIP, "conv_dma pair launch failed (%s): Co %d Ci %d+%d To %d", hipGetErrorString(e), W3.Co, W3.Ci, W1.Ci, a1.To);
    return LDS_OK;
}

static int run_dconv_pair_bf3(const ConvW& W3, const void* h, const ConvW& W1, const void* x1, int C1, const void* x2, int C2, int T, const float* bias_pair,
                              float2* gnpart_out, void* out, int B, hipStream_t st, int fmt, int lvl = 0) {
    DmaConvArgs a3, a1;
    DOpt o3;
    o3.lvl_in = o3.lvl_out = lvl;
    o3.pad = 1;
    int rc = fill_dconv(W3, (const float*)h, W3.Ci, nullptr, 0, T, o3, (float*)out, B, a3);
    if (rc != LDS_OK) return rc;
    DOpt o1;
    o1.lvl_in = o1.lvl_out = lvl;
    o1.gnpart_out = gnpart_out;
    rc = fill_dconv(W1, (const float*)x1, C1, (const float*)x2, C2, T, o1, (float*)out, B, a1);
    if (rc != LDS_OK) return rc;
    const void *w3p = (fmt == FMT_F16X2) ? W3.wh : W3.w3, *w1p = (fmt == FMT_F16X2) ? W1.wh : W1.w3;
    if (!w3p || !w1p) return set_error(LDS_EINVAL, "split weights were not packed for this layer");
    if (fmt == FMT_F16X2 && W3.wh_inv != W1.wh_inv) return set_error(LDS_EINVAL, "internal: the pair's fp16 weight scales differ");
    a3.w = (const float*)w3p; a1.w = (const float*)w1p;
    a3.acc_scale = a1.acc_scale = (fmt == FMT_F16X2) ? W1.wh_inv : 0.f;
    a3.x2 = nullptr; a1.x2 = (const float*)x2;
    a3.bias = nullptr;
    a1.bias = bias_pair;
    const double flops = 2.0 * B * (double)a1.To * (double)W3.Co * ((double)W3.Ci * 3.0 + (double)W1.Ci);
    const double bytes = 2.0 * fmt_planes(fmt) * ((double)B * (W3.Ci + W1.Ci) * T + (double)W3.Co * (3.0 * W3.Ci + W1.Ci) + (double)B * a1.Cout * a1.To);
    if (!conv_bf3_pair_applies(a3, a1)) return 1;
    hipError_t e;
    {
        ProfScope ps(st, "conv_bf3", flops, bytes, true);
        e = launch_conv_bf3_pair(a3, a1, fmt, st);
        if (ps.on) {
            std::string cfgs(conv_bf3_last_config());
            std::string nm = "conv_bf3<" + cfgs.substr(0, cfgs.find(" grid")) + ">";
            if (g_prof_level.load(std::memory_order_relaxed) >= 2) {
                char sh[96];
                snprintf(sh, sizeof(sh), " Ci%d+%d Co%d K3+1 To%d", W3.Ci, W1.Ci, W3.Co, a1.To);
                nm += sh;
            }
            ps.rename(nm);
        }
    }
    if (e != hipSuccess) return set_error(LDS_EHIP, "conv_bf3 pair launch failed (%s): Co %d Ci %d+%d To %d", hipGetErrorString(e), W3.Co, W3.Ci, W1.Ci, a1.To);
    return LDS_OK;
}

// Which resnet k 3 convolutions run in the Winograd form (conv_wino.hip) in exact-fp32 mode.  The choice depends on the shape (Ci, Co, T at
// this level) alone -- never on the actual batch, so an utterance's result stays bit-identical for any batch split.  The table names the
// (Ci, Co) of the UNet's resnets with the shortest T at which tools/bench_wino.py measured the Winograd pair (gn_wino + conv_wino) faster
// than the direct pair (gn_stream + conv_dma) at the nominal batch of 16 by more than the larger of the two spreads; every longer T that
// was measured won by more (profiles/r26_wino_shapes.json).  Shapes that were not measured keep the direct path.
static int wino_min_T(int Ci, int Co) {
    static const int kTable[][3] = {
        {256, 256, 64},  {512, 256, 64},  {640, 256, 130}, {256, 384, 256}, {384, 384, 256}, {640, 384, 256},
        {768, 384, 256}, {896, 384, 256}, {384, 512, 128}, {512, 512, 64},  {896, 512, 128}, {1024, 512, 64},
    };
    for (const auto& s : kTable)
        if (s[0] == Ci && s[1] == Co) return s[2];
    return 0;
}
static bool wino_routed(int Ci, int Co, int T) {
    const int Tmin = wino_min_T(Ci, Co);
    return Tmin > 0 && T >= Tmin;
}
static bool wino_routed_any_T(int Ci, int Co) { return wino_min_T(Ci, Co) > 0; }      // (load time: T is not known yet)
// A resnet's k 3 convolution over the planes `v` that launch_gn_wino wrote (W.wu: its packed taps).  The profiler's record carries the
// algorithmic FLOP of the convolution it replaces, 2 B T Co Ci 3 -- the figure every other family reports -- not the two thirds it executes.
// (`family`: the record's name; `Ci_name`: the input channels of the operator it stands for; a.Ci is the depth the kernel reduces over)
static int run_wconv_args(WinoConvArgs& a, const char* family, int Ci_name, double flops, double bytes, hipStream_t st, int cfg) {
    hipError_t e;
    {
        ProfScope ps(st, family, flops, bytes, true);
        e = launch_conv_wino(a, cfg, st);
        if (ps.on) {
            std::string cfgs(conv_wino_last_config());
            std::string nm = std::string(family) + "<" + cfgs.substr(0, cfgs.find(" grid")) + ">";
            if (g_prof_level.load(std::memory_order_relaxed) >= 2) {
                char sh[96];
                snprintf(sh, sizeof(sh), " Ci%d Co%d K3 To%d%s", Ci_name, a.Co, a.T, a.res ? " +res" : "");
                nm += sh;
            }
            ps.rename(nm);
        }
    }
    if (e != hipSuccess) return set_error(LDS_EHIP, "%s launch failed (%s): Co %d Ci %d T %d cfg %d", family, hipGetErrorString(e), a.Co, a.Ci, a.T, cfg);
    return LDS_OK;
}
static int run_wconv(const ConvW& W, const float* v, int T, const float* res, float2* gnpart_out, float* out, int B, hipStream_t st, int lvl, int cfg = 0) {
    if (!W.wu || W.K != 3) return set_error(LDS_EINVAL, "wconv: the Winograd taps were not packed for this layer");
    WinoConvArgs a{};
    a.v = v; a.u = W.wu; a.bias = W.bias; a.res = res; a.out = out; a.gnpart_out = gnpart_out;
    a.lens = tl_lens; a.lvl = lvl;
    a.B = B; a.Ci = W.Ci; a.Mp = W.Mp; a.Co = W.Co; a.T = T;
    const double flops = 2.0 * B * (double)T * (double)W.Co * (double)W.Ci * 3.0;
    const double bytes = 4.0 * ((double)B * W.Ci * 4.0 * ((T + 1) / 2) + 4.0 * W.Ci * W.Co + (double)B * W.Co * T * (res ? 2.0 : 1.0));
    return run_wconv_args(a, "conv_wino", W.Ci, flops, bytes, st, cfg);
}
// Which conv2 + shortcut pairs run as one conv_wino launch over Cm + Cin / 2 channels (pack_wino_pair) in exact-fp32 mode: (Cin, Cm) of the
// UNet's resnets with a shortcut and the shortest T at which tools/bench_wino.py --pair measured the new form (conv1's pass with the side
// output + gn_wpair + conv_wino_pair) faster than the direct one (conv1's pass + gn_stream + conv_dma_pair) at the nominal batch of 16 by
// more than the larger of the two spreads (profiles/r30_wino_pair_shapes.json).  Like wino_min_T it never sees the batch or
// the lengths; a pair is routed only where conv1 is (its pass writes the shortcut's planes).
static int wino_pair_min_T(int Cin, int Cm) {
    static const int kTable[][3] = {
        {256, 384, 256}, {384, 512, 128}, {1024, 512, 64}, {896, 512, 128}, {896, 384, 256}, {768, 384, 256}, {640, 384, 256}, {512, 256, 512},
    };      // (640 -> 256 at 512 frames measured 0.69 us faster with a spread of 0.85 us: it stays direct)
    for (const auto& s : kTable)
        if (s[0] == Cin && s[1] == Cm) return s[2];
    return 0;
}
static bool wino_pair_routed(int Cin, int Cm, int T) {
    const int Tmin = wino_pair_min_T(Cin, Cm);
    return Tmin > 0 && T >= Tmin && wino_routed(Cin, Cm, T);
}
static size_t wino_pair_plane_floats(int Cin, int Cm, int T) { return (size_t)(Cm + Cin / 2) * 4 * (size_t)((T + 1) / 2); }      // per utterance
// conv2 + shortcut over the pair planes `v` ([B][(Cm + Cin/2)/8][2][4][P][4]: launch_gn_wino_pair's two passes) with the taps of pack_wino_pair.
// The record carries the algorithmic FLOP of the pair it replaces, 2 B T Co (3 Cm + Cin), and Ci = Cin in its name.
static int run_wconv_pair(const float* wu_pair, int Cin, int Cm, int Mp, const float* v, int T, const float* bias_pair, float2* gnpart_out, float* out, int B,
                          hipStream_t st, int lvl, int cfg = 0) {
    if (!wu_pair) return set_error(LDS_EINVAL, "wconv pair: the pair's Winograd taps were not packed for this resnet");
    WinoConvArgs a{};
    a.v = v; a.u = wu_pair; a.bias = bias_pair; a.res = nullptr; a.out = out; a.gnpart_out = gnpart_out;
    a.lens = tl_lens; a.lvl = lvl;
    a.B = B; a.Ci = Cm + Cin / 2; a.Mp = Mp; a.Co = Cm; a.T = T;
    const double flops = 2.0 * B * (double)T * (double)Cm * (3.0 * Cm + (double)Cin);
    const double bytes = 4.0 * ((double)B * a.Ci * 4.0 * ((T + 1) / 2) + 4.0 * a.Ci * Cm + (double)B * Cm * T);
    return run_wconv_args(a, "conv_wino_pair", Cin, flops, bytes, st, cfg);
}

// The UNet's plan is the same in both GEMM modes; these pick the kernel family.  In LDS_GEMM_SPLIT_BF16 mode every activation buffer
// holds a K8B3 tensor (k8b3.h) instead of a K4P one -- except q / k / v, which stay fp32 for the attention kernel.
// mode = lds_unet::gemm_mode: 0 exact fp32 (K4P tensors); 1 / 2 split planes, format mode - 1 (k8b3.h)
static int dconv_any(int mode, const ConvW& W, const float* x1, int C1, const float* x2, int C2, int Tsrc, const DOpt& o, float* out, int B, hipStream_t st) {
    return mode ? run_dconv_bf3(W, x1, C1, x2, C2, Tsrc, o, out, B, st, 0, mode - 1) : run_dconv(W, x1, C1, x2, C2, Tsrc, o, out, B, st);
}
static hipError_t gn_any(int mode, const float* x1, const float* x2, int C1, int C2, int T, int groups, float eps, const float* gamma, const float* beta,
                         const float* ss, int ss_stride, int ss_off, int silu, const float2* gp1, const float2* gp2, float* y, int B, hipStream_t s, int lvl = 0) {
    return mode ? launch_gn_stream_bf3(x1, x2, C1, C2, T, groups, eps, gamma, beta, ss, ss_stride, ss_off, silu, gp1, gp2, y, B, s, mode - 1, tl_lens, lvl)
                : launch_gn_stream(x1, x2, C1, C2, T, groups, eps, gamma, beta, ss, ss_stride, ss_off, silu, gp1, gp2, y, B, s, tl_lens, lvl);
}
static hipError_t to_act_any(int mode, const float* in, float* out, int B, int C, int T, int Ctot, int c_off, hipStream_t s) {
    return mode ? launch_to_k8b3(in, out, B, C, T, Ctot, c_off, s, mode - 1, tl_lens) : launch_to_k4p(in, out, B, C, T, Ctot, c_off, s, tl_lens);
}

// ================================================================================================
// UNet
// ================================================================================================
struct ResnetW {
    int cin = 0, cout = 0;
    float *g1 = nullptr, *b1 = nullptr, *g2 = nullptr, *b2 = nullptr;
    ConvW conv1, conv2, sc;
    float* bias_pair = nullptr;      // conv2.bias + conv_shortcut.bias per packed row (the fused conv2 + shortcut launch)
    float* wu_pair = nullptr;        // conv2 + shortcut as one Winograd reduction, [4][cout + cin/2][Mp] packed (pack_wino_pair), where the pair is routed
    bool has_sc = false;
    int temb_off = 0;
};
struct TfmW {
    int C = 0;
    float *gn_g = nullptr, *gn_b = nullptr;
    float *qkv_c1[2] = {nullptr, nullptr}, *qkv_c2[2] = {nullptr, nullptr}, *ff1_c1 = nullptr, *ff1_c2 = nullptr;   // folded LayerNorm constants
    ConvW proj_in, qkv[2], o[2], ff1, ff2_out;      // ff2_out = ff.net.2 and proj_out composed (load_tfm)
    // `norm` (GroupNorm, no activation) folded into proj_in (pack_gn_fold): one launch and one activation round trip fewer per block
    ConvW proj_in_g; float *pi_cg = nullptr, *pi_c2 = nullptr; bool fold = false;
};
struct DownBlk { std::vector<ResnetW> res; std::vector<TfmW> att; bool has_down = false; ConvW down; int ch = 0; };
struct UpBlk { std::vector<ResnetW> res; std::vector<TfmW> att; std::vector<int> skip_ch; bool has_up = false; ConvW up; int ch = 0; };

struct lds_unet {
    lds_unet_cfg cfg;
    Owner own;
    int M = 0, H = 0, G = 8, heads = 8, temb = 0, tproj_dim = 0;
    ConvW conv_in, conv_out;
    ConvW conv_in_x, conv_in_c;      // conv_in split over its input channels: the sample's rows / the condition's rows (+ bias), see unet_stage_cond
    float *gno_g = nullptr, *gno_b = nullptr;
    float* freqs = nullptr;
    float *t_w1 = nullptr, *t_b1 = nullptr, *t_w2 = nullptr, *t_b2 = nullptr;
    float *tp_w = nullptr, *tp_b = nullptr;
    int tp_M = 0;
    std::vector<DownBlk> down;
    ResnetW mid_r0, mid_r1;
    TfmW mid_t;
    std::vector<UpBlk> up;
    int max_ci = 0;
    int gemm_mode = LDS_GEMM_F32;      // LDS_GEMM_SPLIT_BF16 / LDS_GEMM_SPLIT_F16: every conv / linear through conv_bf3 (lds_unet_set_gemm_mode)
    bool split_packed[2] = {false, false};
    int latency_mode = 0;              // 1: tile / split choices from the actual batch (lds_unet_set_latency_mode)
    std::atomic<int> in_calls{0};      // forward / sampler calls of any thread currently enqueueing on this handle (the mode switches refuse meanwhile)
};
struct UnetCallScope {      // RAII: one call in progress
    lds_unet* u;
    explicit UnetCallScope(lds_unet* u_) : u(u_) { u->in_calls.fetch_add(1, std::memory_order_acq_rel); }
    ~UnetCallScope() { u->in_calls.fetch_sub(1, std::memory_order_acq_rel); }
};

static float* up_vec(Owner& o, const float* p, int64_t n) {
    if (!p) return nullptr;
    return o.upload(std::vector<float>(p, p + n));
}

static bool load_resnet(lds_unet* u, Tensors& T, const std::string& p, int cin, int cout, std::vector<float>& tpw,
                        std::vector<float>& tpb, ResnetW& r) {
    Owner& o = u->own;
    r.cin = cin; r.cout = cout;
    r.g1 = up_vec(o, T.get(p + "norm1.weight", cin), cin);
    r.b1 = up_vec(o, T.get(p + "norm1.bias", cin), cin);
    r.g2 = up_vec(o, T.get(p + "norm2.weight", cout), cout);
    r.b2 = up_vec(o, T.get(p + "norm2.bias", cout), cout);
    const float* w1 = T.get(p + "conv1.weight", (int64_t)cout * cin * 3);
    const float* c1b = T.get(p + "conv1.bias", cout);
    const float* w2 = T.get(p + "conv2.weight", (int64_t)cout * cout * 3);
    const float* c2b = T.get(p + "conv2.bias", cout);
    const float* tw = T.get(p + "time_emb_proj.weight", (int64_t)2 * cout * u->temb);
    const float* tb = T.get(p + "time_emb_proj.bias", 2 * cout);
    if (!r.g1 || !r.b1 || !r.g2 || !r.b2 || !w1 || !c1b || !w2 || !c2b || !tw || !tb) return false;
    if (!pack_conv(o, w1, c1b, cout, cin, 3, r.conv1)) return false;
    if (!pack_conv(o, w2, c2b, cout, cout, 3, r.conv2)) return false;
    r.has_sc = cin != cout;
    // the Winograd taps of conv1 and of a conv2 without shortcut, where some level routes the shape to conv_wino (the direct pack stays)
    if (wino_routed_any_T(cin, cout) && !pack_wino(o, w1, cout, cin, r.conv1)) return false;
    if (!r.has_sc && wino_routed_any_T(cout, cout) && !pack_wino(o, w2, cout, cout, r.conv2)) return false;
    if (r.has_sc) {
        const float* ws = T.get(p + "conv_shortcut.weight", (int64_t)cout * cin);
        const float* bs = T.get(p + "conv_shortcut.bias", cout);
        if (!ws || !bs || !pack_conv(o, ws, bs, cout, cin, 1, r.sc)) return false;
        std::vector<float> bp(r.conv2.Mp, 0.f);
        for (int co = 0; co < cout; ++co) bp[co] = c2b[co] + bs[co];
        r.bias_pair = o.upload(bp);
        if (!r.bias_pair) return false;
        if (wino_pair_min_T(cin, cout) > 0 && wino_routed_any_T(cin, cout)) {
            r.wu_pair = pack_wino_pair(o, w2, ws, cout, cout, cin, r.conv2.Mp);
            if (!r.wu_pair) return false;
        }
    }
    r.temb_off = (int)tpb.size();
    tpw.insert(tpw.end(), tw, tw + (size_t)2 * cout * u->temb);
    tpb.insert(tpb.end(), tb, tb + 2 * cout);
    if (cin > u->max_ci) u->max_ci = cin;
    return true;
}

static bool load_tfm(lds_unet* u, Tensors& T, const std::string& p, int C, TfmW& t) {
    Owner& o = u->own;
    t.C = C;
    t.gn_g = up_vec(o, T.get(p + "norm.weight", C), C);
    t.gn_b = up_vec(o, T.get(p + "norm.bias", C), C);
    const float* piw = T.get(p + "proj_in.weight", (int64_t)C * C);
    const float* pib = T.get(p + "proj_in.bias", C);
    const float* pow_ = T.get(p + "proj_out.weight", (int64_t)C * C);
    const float* pob = T.get(p + "proj_out.bias", C);
    if (!t.gn_g || !t.gn_b || !piw || !pib || !pow_ || !pob) return false;
    if (!pack_conv(o, piw, pib, C, C, 1, t.proj_in)) return false;
    t.fold = u->G <= 8 && C % u->G == 0 && (C / u->G) % 16 == 0;
    if (t.fold && !pack_gn_fold(o, piw, pib, T.get(p + "norm.weight", C), T.get(p + "norm.bias", C), C, C, u->G, t.proj_in_g, t.pi_cg, t.pi_c2)) return false;
    const std::string b = p + "transformer_blocks.0.";
    const float *lg[3], *lb[3];
    for (int i = 0; i < 3; ++i) {
        const std::string n = b + "norm" + std::to_string(i + 1);
        lg[i] = T.get(n + ".weight", C);
        lb[i] = T.get(n + ".bias", C);
        if (!lg[i] || !lb[i]) return false;
    }
    for (int i = 0; i < 2; ++i) {
        const std::string a = b + "attn" + std::to_string(i + 1) + ".";
        const float* q = T.get(a + "to_q.weight", (int64_t)C * C);
        const float* k = T.get(a + "to_k.weight", (int64_t)C * C);
        const float* v = T.get(a + "to_v.weight", (int64_t)C * C);
        const float* ow = T.get(a + "to_out.0.weight", (int64_t)C * C);
        const float* ob = T.get(a + "to_out.0.bias", C);
        if (!q || !k || !v || !ow || !ob) return false;
        std::vector<float> cat((size_t)3 * C * C);
        memcpy(cat.data(), q, sizeof(float) * C * C);
        memcpy(cat.data() + (size_t)C * C, k, sizeof(float) * C * C);
        memcpy(cat.data() + (size_t)2 * C * C, v, sizeof(float) * C * C);
        // norm{1,2} (LayerNorm) is folded into the bias-free q/k/v projection
        if (!pack_ln_fold(o, cat.data(), nullptr, lg[i], lb[i], 3 * C, C, {}, t.qkv[i], t.qkv_c1[i], t.qkv_c2[i])) return false;
        if (!pack_conv(o, ow, ob, C, C, 1, t.o[i])) return false;
    }
    const float* f1 = T.get(b + "ff.net.0.proj.weight", (int64_t)8 * C * C);
    const float* f1b = T.get(b + "ff.net.0.proj.bias", 8 * C);
    const float* f2 = T.get(b + "ff.net.2.weight", (int64_t)C * 4 * C);
    const float* f2b = T.get(b + "ff.net.2.bias", C);
    if (!f1 || !f1b || !f2 || !f2b) return false;
    {
        // norm3 folded into the GEGLU projection; rows interleaved value/gate in 32-row groups as in pack_geglu
        std::vector<int> perm(8 * C);
        for (int mm = 0; mm < 8 * C; ++mm) perm[mm] = ((mm % 64) / 32 == 0 ? 0 : 4 * C) + 32 * (mm / 64) + mm % 32;
        if (!pack_ln_fold(o, f1, f1b, lg[2], lb[2], 8 * C, C, perm, t.ff1, t.ff1_c1, t.ff1_c2)) return false;
    }
    {
        // ff.net.2 (4C -> C, + residual h) and proj_out (C -> C, + residual x) are two linear maps with nothing between them
        // (reference attention.py:197-203, transformer_1d.py:289-295):
        //   out = Wp (W2 ff + b2 + h) + bp + x = [Wp W2 | Wp] [ff ; h] + (Wp b2 + bp) + x
        // so they run as ONE convolution over the virtual concat [ff ; h] (5C input channels) with host-composed weights
        // (products accumulated in double, rounded to fp32 once): same FLOPs, one launch and one activation round trip fewer.
        const int C4 = 4 * C, C5 = 5 * C;
        std::vector<float> wcat((size_t)C * C5), bcat(C);
        std::vector<double> acc(C4);
        for (int m = 0; m < C; ++m) {
            std::fill(acc.begin(), acc.end(), 0.0);
            double bs = (double)pob[m];
            for (int k = 0; k < C; ++k) {
                const double a = (double)pow_[(size_t)m * C + k];
                const float* w2r = f2 + (size_t)k * C4;
                for (int n = 0; n < C4; ++n) acc[n] += a * (double)w2r[n];
                bs += a * (double)f2b[k];
                wcat[(size_t)m * C5 + C4 + k] = pow_[(size_t)m * C + k];
            }
            for (int n = 0; n < C4; ++n) wcat[(size_t)m * C5 + n] = (float)acc[n];
            bcat[m] = (float)bs;
        }
        if (!pack_conv(o, wcat.data(), bcat.data(), C, C5, 1, t.ff2_out)) return false;
    }
    return true;
}

extern "C" int lds_unet_create(const lds_unet_cfg* cfg, int n, const char* const* names, const float* const* ptrs,
                               const int64_t* numel, lds_unet** out) {
    if (!cfg || !names || !ptrs || !numel || !out) return set_error(LDS_EINVAL, "null argument");
    if (cfg->n_blocks < 2 || cfg->n_blocks > 8) return set_error(LDS_EINVAL, "n_blocks %d unsupported", cfg->n_blocks);
    Tensors T;
    for (int i = 0; i < n; ++i) T.m[names[i]] = {ptrs[i], numel[i]};
    lds_unet* u = new lds_unet();
    u->cfg = *cfg;
    u->M = cfg->out_dims; u->H = cfg->n_hidden; u->G = cfg->norm_groups; u->heads = cfg->n_heads;
    const int* boc = cfg->block_out_channels;
    const int nb = cfg->n_blocks, L = cfg->n_layers;
    u->tproj_dim = boc[0];
    u->temb = boc[0] * 4;
    for (int i = 0; i < nb; ++i) {
        const int hd = boc[i] / cfg->n_heads;
        // 16 * groups: GroupNorm statistics travel as 16-channel partials, and a skip-concat's groups must be made of whole ones
        if (boc[i] % 64 != 0 || cfg->norm_groups <= 0 || boc[i] % (16 * cfg->norm_groups) != 0 || (hd != 32 && hd != 48 && hd != 64)) {
            delete u;
            return set_error(LDS_EINVAL, "block_out_channels[%d]=%d unsupported (need a multiple of 64 and of 16*norm_groups, head dim 32/48/64)", i, boc[i]);
        }
    }
    if ((u->M % 16) || (u->H % 16)) { delete u; return set_error(LDS_EINVAL, "out_dims and n_hidden must be multiples of 16"); }
    Owner& o = u->own;
    bool ok = true;
    std::vector<float> tpw, tpb;
    const int cin0 = u->M + u->H;
    {
        const float* w = T.get("conv_in.weight", (int64_t)boc[0] * cin0 * 3);
        const float* b = T.get("conv_in.bias", boc[0]);
        ok = ok && w && b && pack_conv(o, w, b, boc[0], cin0, 3, u->conv_in);
        if (ok) {
            std::vector<float> wx((size_t)boc[0] * u->M * 3), wc((size_t)boc[0] * u->H * 3);
            for (int co = 0; co < boc[0]; ++co)
                for (int ci = 0; ci < cin0; ++ci)
                    for (int k = 0; k < 3; ++k) {
                        const float v = w[((size_t)co * cin0 + ci) * 3 + k];
                        if (ci < u->M) wx[((size_t)co * u->M + ci) * 3 + k] = v;
                        else wc[((size_t)co * u->H + (ci - u->M)) * 3 + k] = v;
                    }
            ok = pack_conv(o, wx.data(), nullptr, boc[0], u->M, 3, u->conv_in_x) && pack_conv(o, wc.data(), b, boc[0], u->H, 3, u->conv_in_c);
        }
        u->t_w1 = up_vec(o, T.get("time_embedding.linear_1.weight", (int64_t)u->temb * u->tproj_dim), (int64_t)u->temb * u->tproj_dim);
        u->t_b1 = up_vec(o, T.get("time_embedding.linear_1.bias", u->temb), u->temb);
        u->t_w2 = up_vec(o, T.get("time_embedding.linear_2.weight", (int64_t)u->temb * u->temb), (int64_t)u->temb * u->temb);
        u->t_b2 = up_vec(o, T.get("time_embedding.linear_2.bias", u->temb), u->temb);
        ok = ok && u->t_w1 && u->t_b1 && u->t_w2 && u->t_b2;
        // Timesteps(flip_sin_to_cos=True, freq_shift=0): f_i = exp(-ln(1e4) * i / half), fp32 like the reference
        const int half = u->tproj_dim / 2;
        std::vector<float> fr(half);
        for (int i = 0; i < half; ++i) fr[i] = expf(((float)(-log(10000.0)) * (float)i) / (float)half);
        u->freqs = o.upload(fr);
    }
    // down blocks
    std::vector<int> skip_ch{boc[0]};
    int cprev = boc[0];
    for (int i = 0; i < nb && ok; ++i) {
        DownBlk d;
        d.ch = boc[i];
        const bool last = i == nb - 1;
        const std::string p = "down_blocks." + std::to_string(i) + ".";
        for (int j = 0; j < L && ok; ++j) {
            ResnetW r;
            ok = load_resnet(u, T, p + "resnets." + std::to_string(j) + ".", j == 0 ? cprev : boc[i], boc[i], tpw, tpb, r);
            d.res.push_back(r);
            if (!last && ok) {
                TfmW t;
                ok = load_tfm(u, T, p + "attentions." + std::to_string(j) + ".", boc[i], t);
                d.att.push_back(t);
            }
            skip_ch.push_back(boc[i]);
        }
        if (!last && ok) {
            d.has_down = true;
            const float* w = T.get(p + "downsamplers.0.conv.weight", (int64_t)boc[i] * boc[i] * 3);
            const float* b = T.get(p + "downsamplers.0.conv.bias", boc[i]);
            ok = w && b && pack_conv(o, w, b, boc[i], boc[i], 3, d.down);
            skip_ch.push_back(boc[i]);
        }
        cprev = boc[i];
        u->down.push_back(d);
    }
    // mid
    if (ok) {
        const int c = boc[nb - 1];
        ok = load_resnet(u, T, "mid_block.resnets.0.", c, c, tpw, tpb, u->mid_r0) &&
             load_tfm(u, T, "mid_block.attentions.0.", c, u->mid_t) && load_resnet(u, T, "mid_block.resnets.1.", c, c, tpw, tpb, u->mid_r1);
    }
    // up blocks
    int cout = boc[nb - 1];
    for (int i = 0; i < nb && ok; ++i) {
        UpBlk b;
        const int prev = cout;
        cout = boc[nb - 1 - i];
        b.ch = cout;
        const bool last = i == nb - 1;
        const std::string p = "up_blocks." + std::to_string(i) + ".";
        for (int j = 0; j < L + 1 && ok; ++j) {
            const int sk = skip_ch.back();
            skip_ch.pop_back();
            const int hin = j == 0 ? prev : cout;
            b.skip_ch.push_back(sk);
            ResnetW r;
            ok = load_resnet(u, T, p + "resnets." + std::to_string(j) + ".", hin + sk, cout, tpw, tpb, r);
            b.res.push_back(r);
            if (i != 0 && ok) {
                TfmW t;
                ok = load_tfm(u, T, p + "attentions." + std::to_string(j) + ".", cout, t);
                b.att.push_back(t);
            }
        }
        if (!last && ok) {
            b.has_up = true;
            const float* w = T.get(p + "upsamplers.0.conv.weight", (int64_t)cout * cout * 3);
            const float* bb = T.get(p + "upsamplers.0.conv.bias", cout);
            ok = w && bb && pack_conv(o, w, bb, cout, cout, 3, b.up);
        }
        u->up.push_back(b);
    }
    if (ok) {
        u->gno_g = up_vec(o, T.get("conv_norm_out.weight", boc[0]), boc[0]);
        u->gno_b = up_vec(o, T.get("conv_norm_out.bias", boc[0]), boc[0]);
        const float* w = T.get("conv_out.weight", (int64_t)u->M * boc[0] * 3);
        const float* b = T.get("conv_out.bias", u->M);
        ok = u->gno_g && u->gno_b && w && b && pack_conv(o, w, b, u->M, boc[0], 3, u->conv_out);
    }
    if (ok) {
        u->tp_M = (int)tpb.size();
        u->tp_w = o.upload(tpw);
        u->tp_b = o.upload(tpb);
        ok = u->tp_w && u->tp_b;
    }
    if (cin0 > u->max_ci) u->max_ci = cin0;
    if (!ok) {
        std::string miss = T.missing;
        delete u;
        if (!miss.empty()) return set_error(LDS_EMISSING, "weight tensor %s", miss.c_str());
        return set_error(LDS_ENOMEM, "device allocation / upload failed while packing weights");
    }
    *out = u;
    return LDS_OK;
}

extern "C" void lds_unet_destroy(lds_unet* u) { delete u; }

// split twins (format fmt) of every weight set the forward pass uses (first switch to that mode only)
static bool unet_pack_split(lds_unet* u, int fmt) {
    Owner& o = u->own;
    bool ok = true;
    auto T1 = [&](ConvW& W) { ok = ok && make_split_twin(o, W, fmt); };
    auto res = [&](ResnetW& r) {
        T1(r.conv1);
        if (r.has_sc) ok = ok && make_split_twin_pair(o, r.conv2, r.sc, fmt);
        else T1(r.conv2);
    };
    auto tfm = [&](TfmW& t) { T1(t.proj_in); if (t.fold) T1(t.proj_in_g); T1(t.qkv[0]); T1(t.qkv[1]); T1(t.o[0]); T1(t.o[1]); T1(t.ff1); T1(t.ff2_out); };
    T1(u->conv_in); T1(u->conv_in_x); T1(u->conv_in_c); T1(u->conv_out);
    for (auto& d : u->down) {
        for (auto& r : d.res) res(r);
        for (auto& t : d.att) tfm(t);
        if (d.has_down) T1(d.down);
    }
    res(u->mid_r0); tfm(u->mid_t); res(u->mid_r1);
    for (auto& b : u->up) {
        for (auto& r : b.res) res(r);
        for (auto& t : b.att) tfm(t);
        if (b.has_up) T1(b.up);
    }
    return ok;
}
extern "C" int lds_unet_set_gemm_mode(lds_unet* u, int mode) {
    if (u && mode == LDS_GEMM_SPLIT_BF16)
        return set_error(LDS_EINVAL, "the split-bf16 UNet mode was removed in round 4: lossless but no faster than exact fp32 (DESIGN 10.1); the kernel format remains (lds_test_dconv_split)");
    if (!u || (mode != LDS_GEMM_F32 && mode != LDS_GEMM_SPLIT_F16)) return set_error(LDS_EINVAL, "bad argument");
    if (u->in_calls.load(std::memory_order_acquire) > 0) return set_error(LDS_EBUSY, "a forward / sampler call of this handle is in progress on another thread");
    if (mode != LDS_GEMM_F32 && !u->split_packed[mode - 1]) {
        if (u->M % 16 || u->H % 16) return set_error(LDS_EINVAL, "split GEMM modes need out_dims and n_hidden to be multiples of 16");
        if (!unet_pack_split(u, mode - 1)) return set_error(LDS_ENOMEM, "packing the split weights failed");
        u->split_packed[mode - 1] = true;
    }
    u->gemm_mode = mode;
    return LDS_OK;
}
extern "C" int lds_unet_get_gemm_mode(const lds_unet* u) { return u ? u->gemm_mode : LDS_EINVAL; }
extern "C" int lds_unet_set_latency_mode(lds_unet* u, int on) {
    if (!u || (on != 0 && on != 1)) return set_error(LDS_EINVAL, "bad argument");
    if (u->in_calls.load(std::memory_order_acquire) > 0) return set_error(LDS_EBUSY, "a forward / sampler call of this handle is in progress on another thread");
    u->latency_mode = on;
    return LDS_OK;
}
extern "C" int lds_unet_get_latency_mode(const lds_unet* u) { return u ? u->latency_mode : LDS_EINVAL; }

static int down_len(int T) { return (T - 1) / 2 + 1; }  // Conv1d k3 s2 p1

// All UNet activations between kernels are K4P tensors (k4p.h): floats(C, T) = C * (T + 2) per batch element.
struct UnetWs {
    float *e1, *emb, *tproj;
    float2* lnp;
    float* kpart; unsigned* kcount;      // latency mode: cluster split-K scratch (partial tiles, arrival counters)
    int* lens_dev;                       // ragged batches: the per-utterance lengths (<= 64 utterances)
    float* xin;
    float *xk, *ck, *cinc;      // sampler runs: the sample alone in K4P, the condition alone, conv_in's condition half (+ bias), computed once per run
    std::vector<float*> skips;
    float *cur[2], *r, *h1, *sc, *ta, *tb, *upt, *gno, *wpl, *qk, *v, *att, *ff;
    int ss_stride = 0;
    // GroupNorm partial statistics of an activation buffer (written by its producer's epilogue, read by gn_stream)
    std::map<const float*, float2*> gpart;
    float2* gp(const float* act) const {
        auto it = gpart.find(act);
        return it == gpart.end() ? nullptr : it->second;
    }
};

static size_t k4(int C, int T) { return (size_t)C * (T + 2); }

static void plan_ws(const lds_unet* u, Arena& A, int B, int T, UnetWs& w) {
    // floats of one activation tensor: K4P = C * (T + 2); K8B3 (split-bf16 mode) = 1.5x that
    const int bf3 = u->gemm_mode;      // 0 = fp32; else split planes, format bf3 - 1
    auto k4 = [bf3](int C, int Tl) -> size_t { return bf3 ? split_floats(bf3 - 1, C, Tl) : (size_t)C * (Tl + 2); };
    const int nb = u->cfg.n_blocks, L = u->cfg.n_layers;
    const int* boc = u->cfg.block_out_channels;
    w.e1 = A.f((size_t)B * u->temb, "e1");
    w.emb = A.f((size_t)B * u->temb, "emb");
    w.tproj = A.f((size_t)B * u->tp_M, "tproj");
    w.xin = A.f(B * k4(u->M + u->H, T), "xin");
    w.xk = A.f(B * k4(u->M, T), "xk"); w.ck = A.f(B * k4(u->H, T), "ck"); w.cinc = A.f(B * k4(u->conv_in.Co, T), "cinc");
    std::vector<int> Ts{T};
    for (int i = 0; i < nb - 1; ++i) Ts.push_back(down_len(Ts.back()));
    size_t maxct = 0, maxgn = k4(boc[0], T), maxatt = 0;      // k4(C, T) = C * (T + 2) also covers the VT layout's C * ceil4(T) up to C floats
    size_t maxgp = 0;                                          // GroupNorm partials of one activation: (C/16) * ceil(T/32) float2 per utterance
    auto gpn = [](int C, int Tl) { return (size_t)(C / 16) * ((Tl + 31) / 32) * 2; };
    w.gpart.clear();
    auto act = [&](int C, int Tl) {                            // an exactly-sized activation buffer + its partials
        const std::string nm = "skip" + std::to_string(w.gpart.size());
        float* p = A.f(B * k4(C, Tl), nm.c_str());
        w.gpart[p] = (float2*)A.f(B * gpn(C, Tl), (nm + ".gnpart").c_str());
        return p;
    };
    w.skips.clear();
    w.skips.push_back(act(boc[0], T));
    for (int i = 0; i < nb; ++i) {
        const int Tl = Ts[i];
        maxct = std::max(maxct, k4(boc[i], Tl));
        maxgp = std::max(maxgp, gpn(boc[i], Tl));
        maxgn = std::max(maxgn, k4(boc[i], Tl));
        if (i > 0) maxgn = std::max(maxgn, k4(boc[i - 1], Tl));
        if (i != nb - 1) maxatt = std::max(maxatt, k4(boc[i], Tl));
        for (int j = 0; j < L; ++j) w.skips.push_back(act(boc[i], Tl));
        if (i != nb - 1) w.skips.push_back(act(boc[i], Ts[i + 1]));
    }
    maxatt = std::max(maxatt, k4(boc[nb - 1], Ts[nb - 1]));
    // up path: block i works at resolution nb-1-i with out channels boc[nb-1-i]; resnet inputs are (hidden + skip) channels
    {
        int prev = boc[nb - 1];
        for (int i = 0; i < nb; ++i) {
            const int lvl = nb - 1 - i, co = boc[lvl], Tl = Ts[lvl];
            maxct = std::max(maxct, k4(co, Tl));
            maxgp = std::max(maxgp, gpn(co, Tl));
            if (lvl > 0) { maxct = std::max(maxct, k4(co, Ts[lvl - 1])); maxgp = std::max(maxgp, gpn(co, Ts[lvl - 1])); }
            if (i != 0) maxatt = std::max(maxatt, k4(co, Tl));
            maxgn = std::max(maxgn, k4(prev + boc[nb - 1], Tl));   // upper bound: hidden + widest skip
            maxgn = std::max(maxgn, k4(2 * std::max(prev, co), Tl));
            prev = co;
        }
    }
    // a resnet convolution routed to conv_wino reads the four Winograd planes from `gno`, 4 C ceil(T / 2) floats per utterance (twice the
    // direct K4P tensor).  Only the exact-fp32 default mode routes, but the slot is sized alike in every mode: a handle's workspace then
    // never shrinks when it is switched to a split mode or to latency mode.
    // `wpl`: the planes of a routed conv2 + shortcut pair (run_wconv_pair).  Not `gno`: conv1's pass writes the shortcut's planes while
    // conv1's own planes live there.  Sized alike in every mode, as `gno` is.
    size_t maxwpl = 0;
    {
        auto planes = [&](const ResnetW& r, int Tl) {
            const size_t P = (size_t)(Tl + 1) / 2;
            if (r.conv1.wu && wino_routed(r.cin, r.cout, Tl)) maxgn = std::max(maxgn, 4 * (size_t)r.cin * P);
            if (r.conv2.wu && wino_routed(r.cout, r.cout, Tl)) maxgn = std::max(maxgn, 4 * (size_t)r.cout * P);
            if (r.wu_pair && wino_pair_routed(r.cin, r.cout, Tl)) maxwpl = std::max(maxwpl, wino_pair_plane_floats(r.cin, r.cout, Tl));
        };
        for (int i = 0; i < nb; ++i) {
            for (const ResnetW& r : u->down[i].res) planes(r, Ts[i]);
            for (const ResnetW& r : u->up[i].res) planes(r, Ts[nb - 1 - i]);
        }
        planes(u->mid_r0, Ts[nb - 1]);
        planes(u->mid_r1, Ts[nb - 1]);
    }
    auto scratch = [&](const char* nm) {                       // a maximum-sized activation buffer + its partials
        float* p = A.f(B * maxct, nm);
        w.gpart[p] = (float2*)A.f(B * maxgp, (std::string(nm) + ".gnpart").c_str());
        return p;
    };
    w.cur[0] = scratch("cur0"); w.cur[1] = scratch("cur1");
    w.r = scratch("r"); w.h1 = scratch("h1"); w.sc = A.f(B * maxct, "sc");
    w.ta = A.f(B * maxct, "ta"); w.tb = A.f(B * maxct, "tb"); w.upt = A.f(B * maxct, "upt");
    w.gno = A.f(B * maxgn, "gno");
    w.wpl = maxwpl ? A.f(B * maxwpl, "wpl") : nullptr;
    w.qk = A.f(B * maxatt * 2, "qk"); w.v = A.f(B * (maxatt + 2048), "v"); w.att = A.f(B * maxatt, "att"); w.ff = A.f(B * maxatt * 4, "ff");
    w.lnp = (float2*)A.f(B * (maxatt / 32 + 64) * 2, "lnp");
    w.lens_dev = (int*)A.f(64, "lens");
    w.kpart = u->latency_mode ? A.f(kClusterPartFloats, "kpart") : nullptr;
    w.kcount = u->latency_mode ? (unsigned*)A.f(kClusterCounters, "kcount") : nullptr;
    A.f(16384, "tail_slack");   // tail slack: ragged last tiles read (masked) entries past a tensor's end
}

// the workspace plan of a forward as text, one slot per line: "name offset bytes" (tools/diag_poison.py fills one slot at a time)
extern "C" int lds_debug_unet_plan(const lds_unet* u, int B, int T, char* buf, size_t cap) {
    if (!u || !buf || B <= 0 || T <= 0) return set_error(LDS_EINVAL, "bad argument");
    std::vector<std::pair<std::string, std::pair<size_t, size_t>>> log;
    Arena A(nullptr, 0);
    A.log = &log;
    UnetWs w;
    plan_ws(u, A, B, T, w);
    std::string out;
    for (auto& e : log) out += e.first + " " + std::to_string(e.second.first) + " " + std::to_string(e.second.second) + "\n";
    if (out.size() + 1 > cap) return set_error(LDS_ENOMEM, "plan needs %zu bytes", out.size() + 1);
    memcpy(buf, out.c_str(), out.size() + 1);
    return LDS_OK;
}

extern "C" int lds_unet_workspace_bytes(const lds_unet* u, int B, int T, size_t* out) {
    if (!u || !out || B <= 0 || T <= 0) return set_error(LDS_EINVAL, "bad argument");
    Arena A(nullptr, 0);
    UnetWs w;
    plan_ws(u, A, B, T, w);
    *out = A.used;
    return LDS_OK;
}

// bytes of one activation tensor [B][C][T] between kernels in the handle's GEMM mode (K4P fp32 or split planes): the debug trace's copies
static size_t act_bytes(const lds_unet* u, int B, int C, int T) {
    return sizeof(float) * (size_t)B * (u->gemm_mode ? split_floats(u->gemm_mode - 1, C, T) : (size_t)C * (T + 2));
}
#define TRACE(what, ptr, bytes) LDS_TRY(trace_out(st, what, ptr, bytes))
// an activation tensor in the handle's layout; the record's name carries what a reader needs to decode it: "stage.what|C|T|mode"
#define TRACE_ACT(what, ptr, C_, T_)                                                                                  \
    do {                                                                                                              \
        if (g_trace_on.load(std::memory_order_relaxed)) {                                                             \
            char nm_[64];                                                                                             \
            snprintf(nm_, sizeof(nm_), "%s|%d|%d|%d", what, (int)(C_), (int)(T_), u->gemm_mode);                      \
            LDS_TRY(trace_out(st, nm_, ptr, act_bytes(u, B, C_, T_)));                                                \
        }                                                                                                             \
    } while (0)

static int run_resnet(const lds_unet* u, const ResnetW& r, const UnetWs& w, const float* x1, int C1, const float* x2, int C2, int T,
                      float* out, int B, hipStream_t st, int lvl = 0) {
    // reference resnet.py:591-641 (scale_shift): GN -> SiLU -> conv1 -> GN -> *(1+scale)+shift -> SiLU -> conv2 -> + shortcut.
    // GroupNorm(+scale/shift)+SiLU is materialised once per tensor by a streaming pass (gn_stream) so the convolutions stay
    // VALU-free; its statistics come from the partials the producers of x1 / x2 / h1 wrote in their epilogues.
    const int bf3 = u->gemm_mode;      // 0 = fp32; else split planes, format bf3 - 1
    // exact-fp32 mode, shapes of wino_routed's table: the GroupNorm pass writes the Winograd planes instead of the K4P tensor and conv_wino
    // reads them (the debug trace records K4P tensors: a traced run keeps the direct path)
    const bool wino_ok = !bf3 && !u->latency_mode && !g_trace_on.load(std::memory_order_relaxed);
    // ... and a routed conv2 + shortcut pair reads `wpl`: conv1's pass writes the shortcut's planes into its last cin / 16 blocks on the way
    const bool wino1 = wino_ok && r.conv1.wu && wino_routed(C1 + C2, r.cout, T);
    const bool wpair = wino1 && r.has_sc && r.wu_pair && w.wpl && wino_pair_routed(C1 + C2, r.cout, T);
    const long long wpl_stride = (long long)wino_pair_plane_floats(C1 + C2, r.cout, T);
    if (wpair) {
        const int Pn = (T + 1) / 2;
        HIP_TRY(launch_gn_wino_pair(x1, x2, C1, C2, T, u->G, 1e-5f, r.g1, r.b1, nullptr, 0, 0, 1, w.gp(x1), x2 ? w.gp(x2) : nullptr, w.gno, (long long)(C1 + C2) * 4 * Pn,
                                    w.wpl + (size_t)r.cout * 4 * Pn, wpl_stride, B, st, tl_lens, lvl));
        LDS_TRY(run_wconv(r.conv1, w.gno, T, nullptr, w.gp(w.h1), w.h1, B, st, lvl));
    } else if (wino1) {
        HIP_TRY(launch_gn_wino(x1, x2, C1, C2, T, u->G, 1e-5f, r.g1, r.b1, nullptr, 0, 0, 1, w.gp(x1), x2 ? w.gp(x2) : nullptr, w.gno, B, st, tl_lens, lvl));
        LDS_TRY(run_wconv(r.conv1, w.gno, T, nullptr, w.gp(w.h1), w.h1, B, st, lvl));
    } else {
        HIP_TRY(gn_any(bf3, x1, x2, C1, C2, T, u->G, 1e-5f, r.g1, r.b1, nullptr, 0, 0, 1, w.gp(x1), x2 ? w.gp(x2) : nullptr, w.gno, B, st, lvl));
        DOpt o1;
        o1.lvl_in = o1.lvl_out = lvl;
        o1.pad = 1; o1.gnpart_out = w.gp(w.h1);
        TRACE_ACT("gn1", w.gno, C1 + C2, T);
        LDS_TRY(dconv_any(bf3, r.conv1, w.gno, C1 + C2, nullptr, 0, T, o1, w.h1, B, st));
    }
    TRACE_ACT("conv1", w.h1, r.cout, T);
    if (wino_ok && !r.has_sc && C2 == 0 && r.conv2.wu && wino_routed(r.cout, r.cout, T)) {
        HIP_TRY(launch_gn_wino(w.h1, nullptr, r.cout, 0, T, u->G, 1e-5f, r.g2, r.b2, w.tproj, w.ss_stride, r.temb_off, 1, w.gp(w.h1), nullptr, w.gno, B, st, tl_lens, lvl));
        return run_wconv(r.conv2, w.gno, T, x1, w.gp(out), out, B, st, lvl);
    }
    if (wpair) {
        HIP_TRY(launch_gn_wino_pair(w.h1, nullptr, r.cout, 0, T, u->G, 1e-5f, r.g2, r.b2, w.tproj, w.ss_stride, r.temb_off, 1, w.gp(w.h1), nullptr, w.wpl, wpl_stride,
                                    nullptr, 0, B, st, tl_lens, lvl));
        return run_wconv_pair(r.wu_pair, C1 + C2, r.cout, r.conv2.Mp, w.wpl, T, r.bias_pair, w.gp(out), out, B, st, lvl);
    }
    HIP_TRY(gn_any(bf3, w.h1, nullptr, r.cout, 0, T, u->G, 1e-5f, r.g2, r.b2, w.tproj, w.ss_stride, r.temb_off, 1, w.gp(w.h1), nullptr, w.gno, B, st, lvl));
    TRACE_ACT("gn2", w.gno, r.cout, T);
    const float* res = x1;
    if (r.has_sc) {
        // the shortcut rides in conv2's launch (second reduction into the same accumulators; skip-concat on read: two source pointers)
        const int rc = bf3 ? run_dconv_pair_bf3(r.conv2, w.gno, r.sc, x1, C1, x2, C2, T, r.bias_pair, w.gp(out), out, B, st, bf3 - 1, lvl)
                           : run_dconv_pair(r.conv2, w.gno, r.sc, x1, C1, x2, C2, T, r.bias_pair, w.gp(out), out, B, st, lvl);
        if (rc == LDS_OK) TRACE_ACT("conv2sc", out, r.cout, T);
        if (rc != 1) return rc;
        DOpt os;      // no fused variant for these shapes: two launches
        os.lvl_in = os.lvl_out = lvl;
        LDS_TRY(dconv_any(bf3, r.sc, x1, C1, x2, C2, T, os, w.sc, B, st));
        res = w.sc;
    }
    DOpt o2;
    o2.lvl_in = o2.lvl_out = lvl;
    o2.pad = 1; o2.res = res; o2.gnpart_out = w.gp(out);
    LDS_TRY(dconv_any(bf3, r.conv2, w.gno, r.cout, nullptr, 0, T, o2, out, B, st));
    TRACE_ACT("conv2", out, r.cout, T);
    return LDS_OK;
}

static int run_tfm(const lds_unet* u, const TfmW& t, const UnetWs& w, const float* x, int T, float* out, int B, hipStream_t st, int lvl = 0) {
    // reference transformer_1d.py:256-295 + attention.py:130-203, kept channel-major (K4P).  Every conv that feeds a
    // LayerNorm also emits per-32-channel (mean, M2) partials per frame; the consumer (QKV / FF1) combines them per column and
    // applies the LayerNorm in its epilogue (weights pre-multiplied by gamma, pack_ln_fold).
    const int bf3 = u->gemm_mode;      // 0 = fp32; else split planes, format bf3 - 1
    const int C = t.C;
    DOpt op;
    op.lvl_in = op.lvl_out = lvl;
    op.lnpart_out = w.lnp;
    if (t.fold && g_gn_fold.load(std::memory_order_relaxed)) {
        // proj_in(GroupNorm(x)) in one launch: the statistics come from the partials x's producer wrote, the normalisation is a rescaling
        // of the accumulators between groups and a per-row constant (kernels.h DmaConvArgs::gnf_part)
        op.gnf_part = w.gp(x); op.gnf_groups = u->G; op.gnf_eps = 1e-6f; op.gnf_cg = t.pi_cg; op.gnf_c2 = t.pi_c2;
        LDS_TRY(dconv_any(bf3, t.proj_in_g, x, C, nullptr, 0, T, op, w.ta, B, st));
    } else {
        HIP_TRY(gn_any(bf3, x, nullptr, C, 0, T, u->G, 1e-6f, t.gn_g, t.gn_b, nullptr, 0, 0, 0, w.gp(x), nullptr, w.gno, B, st, lvl));
        LDS_TRY(dconv_any(bf3, t.proj_in, w.gno, C, nullptr, 0, T, op, w.ta, B, st));
    }
    TRACE_ACT("proj_in", w.ta, C, T);
    float* h = w.ta;
    float* hn = w.tb;
    for (int a = 0; a < 2; ++a) {
        DOpt oq;
        oq.lvl_in = oq.lvl_out = lvl;
        oq.plain_from = 2 * C; oq.out2 = w.v; oq.vt_D = C / u->heads;      // q, k in K4P; v in attention's VT layout
        oq.ln_part = w.lnp; oq.ln_np = C / 32; oq.ln_c1 = t.qkv_c1[a]; oq.ln_c2 = t.qkv_c2[a];   // LayerNorm folded into the epilogue
        oq.out_f32 = bf3 ? 1 : 0;                                          // (split-bf16 mode: q / k / v stay fp32 for the attention kernel)
        LDS_TRY(dconv_any(bf3, t.qkv[a], h, C, nullptr, 0, T, oq, w.qk, B, st));
        TRACE(a ? "qk2" : "qk1", w.qk, sizeof(float) * (size_t)B * 2 * C * (T + 2));
        TRACE(a ? "v2" : "v1", w.v, sizeof(float) * (size_t)B * C * ((T + 3) & ~3));
        if (bf3) HIP_TRY(launch_attention_k4p_out_bf3(w.qk, w.v, w.att, B, C, T, u->heads, st, bf3 - 1, tl_tile_batch, tl_lens, lvl));
        else HIP_TRY(launch_attention_k4p(w.qk, w.v, w.att, B, C, T, u->heads, st, tl_tile_batch, tl_lens, lvl));
        DOpt oo;
        oo.lvl_in = oo.lvl_out = lvl;
        oo.res = h; oo.lnpart_out = w.lnp;
        TRACE_ACT(a ? "att2" : "att1", w.att, C, T);
        LDS_TRY(dconv_any(bf3, t.o[a], w.att, C, nullptr, 0, T, oo, hn, B, st));
        TRACE_ACT(a ? "o2" : "o1", hn, C, T);
        float* tmp = h; h = hn; hn = tmp;
    }
    DOpt of;
    of.lvl_in = of.lvl_out = lvl;
    of.epi = EPI_GEGLU;
    of.ln_part = w.lnp; of.ln_np = C / 32; of.ln_c1 = t.ff1_c1; of.ln_c2 = t.ff1_c2;
    LDS_TRY(dconv_any(bf3, t.ff1, h, C, nullptr, 0, T, of, w.ff, B, st));
    TRACE_ACT("ff1", w.ff, 4 * C, T);
    DOpt o2;      // ff.net.2 + residual + proj_out + residual in one launch (load_tfm: ff2_out)
    o2.lvl_in = o2.lvl_out = lvl;
    o2.res = x; o2.gnpart_out = w.gp(out);
    LDS_TRY(dconv_any(bf3, t.ff2_out, w.ff, 4 * C, h, C, T, o2, out, B, st));
    TRACE_ACT("ff2_out", out, C, T);
    return LDS_OK;
}

// Ragged batches: per-utterance lengths (host int32 [B], 1 <= len <= T; null = none) -> the workspace's device copy, carried in a launch's
// kernel arguments (<= 64 utterances).
static int ragged_len_host(int n, int lvl) { for (int i = 0; i < lvl; ++i) n = (n - 1) / 2 + 1; return n; }
static int upload_lens(const lds_unet* u, const int* lens_host, int B, int T, int* dev, hipStream_t st) {
    if (B > 64) return set_error(LDS_EINVAL, "per-utterance lengths: at most 64 utterances per call (got %d)", B);
    float tmp[64];
    for (int b = 0; b < B; ++b) {
        if (lens_host[b] < 1 || lens_host[b] > T) return set_error(LDS_EINVAL, "length[%d] = %d outside 1 .. %d", b, lens_host[b], T);
        memcpy(&tmp[b], &lens_host[b], sizeof(int));
    }
    HIP_TRY(launch_set_list((float*)dev, tmp, B, st));
    return LDS_OK;
}

// uniform_t: every batch element shares t[0] (the samplers' case) -> the time-embedding path runs for one column and
// the resnets read it with batch stride 0
// time embedding for n timesteps t[0..n): e1 / emb are [n][temb] scratch, tproj [n][tp_M] receives every resnet's projection
static int time_embedding(const lds_unet* u, const float* t, float* e1, float* emb, float* tproj, int n, hipStream_t st) {
    HIP_TRY(launch_small_linear(u->t_w1, u->t_b1, t, 1, IN_SINUSOID, u->freqs, e1, u->temb, 1, u->temb, u->tproj_dim, n, st));
    HIP_TRY(launch_small_linear(u->t_w2, u->t_b2, e1, u->temb, IN_PLAIN, nullptr, emb, u->temb, 1, u->temb, u->temb, n, st));
    HIP_TRY(launch_small_linear(u->tp_w, u->tp_b, emb, u->temb, IN_PLAIN, nullptr, tproj, u->tp_M, 0, u->tp_M, u->temb, n, st));
    return LDS_OK;
}

// the condition is the same for every evaluation of a sampler run: its channels of the K4P input tensor are written once
static int unet_stage_cond(lds_unet* u, const float* cond, void* ws, size_t ws_bytes, int B, int T, hipStream_t st, const int* lens_host = nullptr) {
    Arena A(ws, ws_bytes);
    UnetWs w;
    plan_ws(u, A, B, T, w);
    if (!A.ok) return set_error(LDS_ENOMEM, "unet workspace too small: need %zu bytes, got %zu", A.used, ws_bytes);
    if (lens_host) LDS_TRY(upload_lens(u, lens_host, B, T, w.lens_dev, st));
    LensScope lsc(lens_host ? w.lens_dev : nullptr);
    TileBatchScope tbs(u->latency_mode ? B : 0, w.kpart, w.kcount);
    if (u->latency_mode) HIP_TRY(launch_fill((float*)w.kcount, 0.f, kClusterCounters, st));      // (bit pattern 0 = counter 0)
    // conv_in is linear in its input channels: the condition's contribution (and the bias) is the same for every evaluation of the run.
    // It is computed here once; an evaluation convolves the 80 sample channels only and adds it as the residual (1008 -> 240 reduction
    // terms per output of conv_in, every NFE).
    const int bf3 = u->gemm_mode;      // 0 = fp32; else split planes, format bf3 - 1
    HIP_TRY(to_act_any(bf3, cond, w.ck, B, u->H, T, u->H, 0, st));
    DOpt o;
    o.pad = 1;
    return dconv_any(bf3, u->conv_in_c, w.ck, u->H, nullptr, 0, T, o, w.cinc, B, st);
}

// tproj_pre: this timestep's column of all resnets' time_emb_proj outputs, computed ahead by the sampler (implies uniform_t);
// cond_staged: the condition channels of the input tensor were already converted by unet_stage_cond
static int unet_forward_impl(lds_unet* u, const float* x, const float* cond, const float* t, float* eps, void* ws, size_t ws_bytes,
                             int B, int T, hipStream_t st, bool uniform_t = false, const float* tproj_pre = nullptr,
                             bool cond_staged = false, const int* lens_host = nullptr) {
    UnetCallScope in_call(u);
    Arena A(ws, ws_bytes);
    UnetWs w;
    plan_ws(u, A, B, T, w);
    if (!A.ok) return set_error(LDS_ENOMEM, "unet workspace too small: need %zu bytes, got %zu", A.used, ws_bytes);
    // ragged batch: the lengths reach the device once per call (per run when the sampler staged them with the condition)
    if (lens_host && !cond_staged) LDS_TRY(upload_lens(u, lens_host, B, T, w.lens_dev, st));
    LensScope lsc(lens_host ? w.lens_dev : nullptr);
    TileBatchScope tbs(u->latency_mode ? B : 0, w.kpart, w.kcount);
    // the counters are left at zero by every launch that uses them; a forward starts from zeroed ones whatever the workspace held before
    if (u->latency_mode && !cond_staged) HIP_TRY(launch_fill((float*)w.kcount, 0.f, kClusterCounters, st));
    const int nb = u->cfg.n_blocks;
    const int bf3 = u->gemm_mode;      // 0 = fp32; else split planes, format bf3 - 1
    // time embedding (reference embeddings.py:24-64,157-201) and all resnets' time_emb_proj in one launch.
    // e1 = SiLU(linear_1(sinusoid(t))); emb = SiLU(linear_2(e1)) -- every consumer of emb applies SiLU first
    // (resnet.py:610), so only the activated embedding is stored
    const int Bt = uniform_t ? 1 : B;
    w.ss_stride = (uniform_t || tproj_pre) ? 0 : u->tp_M;
    if (tproj_pre) {
        w.tproj = const_cast<float*>(tproj_pre);
    } else {
        LDS_TRY(time_embedding(u, t, w.e1, w.emb, w.tproj, Bt, st));
    }
    // the virtual concat [x ; cond] (reference diffusion.py:105) becomes one K4P tensor
    const int cin = u->M + u->H;
    size_t si = 0;
    if (cond_staged) {      // sampler run: conv_in over the sample's channels + the condition half staged by unet_stage_cond
        HIP_TRY(to_act_any(bf3, x, w.xk, B, u->M, T, u->M, 0, st));
        DOpt o;
        o.pad = 1; o.res = w.cinc; o.gnpart_out = w.gp(w.skips[si]);
        LDS_TRY(dconv_any(bf3, u->conv_in_x, w.xk, u->M, nullptr, 0, T, o, w.skips[si], B, st));
    } else {
        HIP_TRY(to_act_any(bf3, x, w.xin, B, u->M, T, cin, 0, st));
        HIP_TRY(to_act_any(bf3, cond, w.xin, B, u->H, T, cin, u->M, st));
        DOpt o;
        o.pad = 1; o.gnpart_out = w.gp(w.skips[si]);
        LDS_TRY(dconv_any(bf3, u->conv_in, w.xin, cin, nullptr, 0, T, o, w.skips[si], B, st));
    }
    const bool tr = g_trace_on.load(std::memory_order_relaxed) != 0;
    auto stage = [&](const char* fmt, int i, int j) { if (tr) { char nm[48]; snprintf(nm, sizeof(nm), fmt, i, j); tl_trace_stage = nm; } };
    stage("conv_in", 0, 0);
    TRACE_ACT("out", w.skips[si], u->conv_in.Co, T);
    const float* cur = w.skips[si++];
    int Tl = T, lvl = 0;      // lvl: how many stride-2 convolutions lie between the input and this resolution (ragged batches, k4p.h)
    std::vector<int> skipT{T};
    for (int i = 0; i < nb; ++i) {
        const DownBlk& d = u->down[i];
        for (size_t j = 0; j < d.res.size(); ++j) {
            float* dst = w.skips[si];
            const bool att = !d.att.empty();
            stage("down%d.res%d", i, (int)j);
            LDS_TRY(run_resnet(u, d.res[j], w, cur, d.res[j].cin, nullptr, 0, Tl, att ? w.r : dst, B, st, lvl));
            stage("down%d.tfm%d", i, (int)j);
            if (att) LDS_TRY(run_tfm(u, d.att[j], w, w.r, Tl, dst, B, st, lvl));
            cur = dst;
            ++si;
            skipT.push_back(Tl);
        }
        if (d.has_down) {
            DOpt o;
            o.lvl_in = lvl; o.lvl_out = lvl + 1;
            o.pad = 1; o.stride = 2; o.gnpart_out = w.gp(w.skips[si]);
            LDS_TRY(dconv_any(bf3, d.down, cur, d.ch, nullptr, 0, Tl, o, w.skips[si], B, st));
            Tl = down_len(Tl);
            stage("down%d.downsample", i, 0);
            TRACE_ACT("out", w.skips[si], d.ch, Tl);
            ++lvl;
            cur = w.skips[si++];
            skipT.push_back(Tl);
        }
    }
    stage("mid.res0", 0, 0);
    LDS_TRY(run_resnet(u, u->mid_r0, w, cur, u->mid_r0.cin, nullptr, 0, Tl, w.cur[0], B, st, lvl));
    stage("mid.tfm", 0, 0);
    LDS_TRY(run_tfm(u, u->mid_t, w, w.cur[0], Tl, w.cur[1], B, st, lvl));
    stage("mid.res1", 0, 0);
    LDS_TRY(run_resnet(u, u->mid_r1, w, w.cur[1], u->mid_r1.cin, nullptr, 0, Tl, w.cur[0], B, st, lvl));
    cur = w.cur[0];
    int ci = 0;  // index of the buffer `cur` lives in
    for (int i = 0; i < nb; ++i) {
        const UpBlk& b = u->up[i];
        for (size_t j = 0; j < b.res.size(); ++j) {
            --si;
            const float* skip = w.skips[si];
            if (skipT[si] != Tl) return set_error(LDS_EINVAL, "internal: skip length mismatch");
            const int hin = b.res[j].cin - b.skip_ch[j];
            const bool att = !b.att.empty();
            float* dst = w.cur[ci ^ 1];
            stage("up%d.res%d", i, (int)j);
            LDS_TRY(run_resnet(u, b.res[j], w, cur, hin, skip, b.skip_ch[j], Tl, att ? w.r : dst, B, st, lvl));
            stage("up%d.tfm%d", i, (int)j);
            if (att) LDS_TRY(run_tfm(u, b.att[j], w, w.r, Tl, dst, B, st, lvl));
            cur = dst;
            ci ^= 1;
        }
        if (b.has_up) {
            // reference resnet.py:137-173: nearest x2 (or size= of the next skip when T % 2^n != 0) then conv k3
            const int Tn = skipT[si - 1];
            float* dst = w.cur[ci ^ 1];
            DOpt o;
            o.pad = 1; o.gnpart_out = w.gp(dst);
            o.lvl_in = o.lvl_out = lvl - 1;
            // ragged batch: the on-read doubling needs EVERY utterance's target length to be twice its own length at this level
            bool doubles = Tn == 2 * Tl;
            if (lens_host)
                for (int ub = 0; ub < B; ++ub) doubles = doubles && ragged_len_host(lens_host[ub], lvl - 1) == 2 * ragged_len_host(lens_host[ub], lvl);
            if (doubles) {
                o.lvl_in = lvl;
                o.ups = 1;
                LDS_TRY(dconv_any(bf3, b.up, cur, b.ch, nullptr, 0, Tl, o, dst, B, st));
            } else {
                HIP_TRY(bf3 ? launch_resample_k8b3(cur, w.upt, B, b.ch, Tl, Tn, st, bf3 - 1, tl_lens, lvl, lvl - 1) : launch_resample_k4p(cur, w.upt, B, b.ch, Tl, Tn, st, tl_lens, lvl, lvl - 1));
                LDS_TRY(dconv_any(bf3, b.up, w.upt, b.ch, nullptr, 0, Tn, o, dst, B, st));
            }
            Tl = Tn;
            --lvl;
            stage("up%d.upsample", i, 0);
            TRACE_ACT("out", dst, b.ch, Tl);
            cur = dst;
            ci ^= 1;
        }
    }
    // out: GN -> SiLU -> conv k3 (reference unet_1d_condition.py:1028-1031); eps leaves in the caller's frame-major layout
    const int c0 = u->cfg.block_out_channels[0];
    HIP_TRY(gn_any(bf3, cur, nullptr, c0, 0, Tl, u->G, 1e-5f, u->gno_g, u->gno_b, nullptr, 0, 0, 1, w.gp(cur), nullptr, w.gno, B, st, 0));
    stage("out", 0, 0);
    TRACE_ACT("gn", w.gno, c0, Tl);
    DOpt o;
    o.pad = 1; o.out_plain = 1;
    LDS_TRY(dconv_any(bf3, u->conv_out, w.gno, c0, nullptr, 0, Tl, o, eps, B, st));
    TRACE("eps", eps, sizeof(float) * (size_t)B * u->M * Tl);
    return LDS_OK;
}

extern "C" int lds_unet_forward(lds_unet* u, const float* x, const float* cond, const float* t, float* eps, void* ws, size_t ws_bytes,
                                int B, int T, void* stream) {
    if (!u || !x || !cond || !t || !eps || !ws || B <= 0 || T <= 0) return set_error(LDS_EINVAL, "bad argument");
    return unet_forward_impl(u, x, cond, t, eps, ws, ws_bytes, B, T, (hipStream_t)stream);
}
extern "C" int lds_unet_forward_ragged(lds_unet* u, const float* x, const float* cond, const float* t, const int32_t* lengths, float* eps, void* ws,
                                       size_t ws_bytes, int B, int T, void* stream) {
    if (!u || !x || !cond || !t || !lengths || !eps || !ws || B <= 0 || T <= 0) return set_error(LDS_EINVAL, "bad argument");
    return unet_forward_impl(u, x, cond, t, eps, ws, ws_bytes, B, T, (hipStream_t)stream, false, nullptr, false, lengths);
}

// ================================================================================================
// Sampler loops
// ================================================================================================
constexpr int kTimePre = 64;      // timesteps whose embeddings are computed ahead per sampler call (a DDPM chunk is 64 rows)
struct SampWs { float *tvec, *eps, *m0, *m1, *m2, *xt, *xp, *tp_t, *tp_e1, *tp_emb, *tp_proj; size_t unet_off; };

static void plan_samp(const lds_unet* u, Arena& A, int B, int T, SampWs& s) {
    const size_t n = (size_t)B * u->M * T;
    s.tvec = A.f(B);
    s.eps = A.f(n); s.m0 = A.f(n); s.m1 = A.f(n); s.m2 = A.f(n); s.xt = A.f(n); s.xp = A.f(n);
    s.tp_t = A.f(kTimePre); s.tp_e1 = A.f((size_t)kTimePre * u->temb); s.tp_emb = A.f((size_t)kTimePre * u->temb);
    s.tp_proj = A.f((size_t)kTimePre * u->tp_M);
    s.unet_off = A.used;
}

extern "C" int lds_sampler_workspace_bytes(const lds_unet* u, int B, int T, size_t* out) {
    if (!u || !out || B <= 0 || T <= 0) return set_error(LDS_EINVAL, "bad argument");
    Arena A(nullptr, 0);
    SampWs s;
    plan_samp(u, A, B, T, s);
    size_t un = 0;
    LDS_TRY(lds_unet_workspace_bytes(u, B, T, &un));
    *out = A.used + un;
    return LDS_OK;
}

static int sampler_run_impl(lds_unet* u, int method, int n_rows, const float* table, const float* cond, float* x, const float* noise, void* ws, size_t ws_bytes,
                            int B, int T, void* stream, const int* lens);
extern "C" int lds_sampler_run(lds_unet* u, int method, int n_rows, const float* table, const float* cond, float* x,
                               const float* noise, void* ws, size_t ws_bytes, int B, int T, void* stream) {
    return sampler_run_impl(u, method, n_rows, table, cond, x, noise, ws, ws_bytes, B, T, stream, nullptr);
}
extern "C" int lds_sampler_run_ragged(lds_unet* u, int method, int n_rows, const float* table, const float* cond, float* x, const float* noise,
                                      const int32_t* lengths, void* ws, size_t ws_bytes, int B, int T, void* stream) {
    if (!lengths) return set_error(LDS_EINVAL, "bad argument");
    return sampler_run_impl(u, method, n_rows, table, cond, x, noise, ws, ws_bytes, B, T, stream, lengths);
}
static int sampler_run_impl(lds_unet* u, int method, int n_rows, const float* table, const float* cond, float* x, const float* noise, void* ws, size_t ws_bytes,
                            int B, int T, void* stream, const int* lens) {
    if (!u || !table || !cond || !x || !ws || n_rows <= 0 || B <= 0 || T <= 0) return set_error(LDS_EINVAL, "bad argument");
    UnetCallScope in_call(u);
    hipStream_t st = (hipStream_t)stream;
    ProfChain chain;
    Arena A(ws, ws_bytes);
    SampWs s;
    plan_samp(u, A, B, T, s);
    if (!A.ok || A.used > ws_bytes) return set_error(LDS_ENOMEM, "sampler workspace too small");
    void* uws = (char*)ws + s.unet_off;
    const size_t uws_bytes = ws_bytes - s.unet_off;
    const long long n = (long long)B * u->M * T;
    const int S = LDS_TABLE_STRIDE;
    // Every evaluation of a run shares the condition and uses a timestep known from the table: the condition channels are
    // converted once, and the time embeddings (time MLP + all 22 time_emb_proj, 75 MB of weights) of all steps are computed
    // in one batched pass instead of once per evaluation.  Per-column results do not depend on the batching.
    std::vector<float> tlist;
    for (int i = 0; i < n_rows; ++i) tlist.push_back(table[(size_t)i * S]);
    if (method == LDS_METHOD_PLMS) tlist.push_back(table[1]);
    const bool pre = (int)tlist.size() <= kTimePre;
    if (pre) {
        HIP_TRY(launch_set_list(s.tp_t, tlist.data(), (int)tlist.size(), st));      // in the launch's arguments: no pageable async copy
        LDS_TRY(time_embedding(u, s.tp_t, s.tp_e1, s.tp_emb, s.tp_proj, (int)tlist.size(), st));
    }
    LDS_TRY(unet_stage_cond(u, cond, uws, uws_bytes, B, T, st, lens));
    auto model = [&](const float* xin, float t_in) -> int {
        if (pre) {
            for (size_t i = 0; i < tlist.size(); ++i)
                if (tlist[i] == t_in)
                    return unet_forward_impl(u, xin, cond, nullptr, s.eps, uws, uws_bytes, B, T, st, true, s.tp_proj + i * u->tp_M, true, lens);
        }
        HIP_TRY(launch_fill(s.tvec, t_in, B, st));
        return unet_forward_impl(u, xin, cond, s.tvec, s.eps, uws, uws_bytes, B, T, st, true, nullptr, true, lens);
    };
    float *m0 = s.m0, *m1 = s.m1, *m2 = s.m2;
    if (method == LDS_METHOD_DPM_SOLVER_PP) {
        // row i: {t_in, sigma_i, alpha_i, order, sigma_{i+1}/sigma_i, alpha_{i+1}*phi, 0.5*that, 1/r0}
        for (int i = 0; i < n_rows; ++i) {
            const float* r = table + (size_t)i * S;
            LDS_TRY(model(x, r[0]));
            float* tmp = m1; m1 = m0; m0 = tmp;
            HIP_TRY(launch_dpm_step(x, s.eps, m0, m1, r[1], r[2], r[3] < 1.5f ? 0 : 1, r[4], r[5], r[6], r[7], n, st));      // (x0 and the update: one launch)
        }
    } else if (method == LDS_METHOD_UNIPC) {
        // row 0: {t_in, sigma, alpha}; rows s>=1: {t_in, sigma_s, alpha_s, order, sigma_s/sigma_{s-1}, alpha_s*h_phi_1,
        //                                         alpha_s*B_h, r_k, rho_p, rho_c0, rho_c1, use_corrector}
        LDS_TRY(model(x, table[0]));
        HIP_TRY(launch_ew(EW_X0, m0, x, s.eps, nullptr, nullptr, table[1], table[2], 0, 0, 0, n, st));
        for (int i = 1; i < n_rows; ++i) {
            const float* r = table + (size_t)i * S;
            const bool o2 = r[3] > 1.5f, corr = r[11] > 0.5f;
            HIP_TRY(launch_ew(EW_AXPBY, s.xt, x, m0, nullptr, nullptr, r[4], r[5], 0, 0, 0, n, st));
            const float* xpred = s.xt;
            if (o2) {
                HIP_TRY(launch_ew(EW_UNIPC_PRED, s.xp, s.xt, m0, m1, nullptr, r[6], r[8], r[7], 0, 0, n, st));
                xpred = s.xp;
            }
            if (corr) {
                LDS_TRY(model(xpred, r[0]));
                HIP_TRY(launch_ew(EW_X0, m2, xpred, s.eps, nullptr, nullptr, r[1], r[2], 0, 0, 0, n, st));
                if (o2) HIP_TRY(launch_ew(EW_UNIPC_CORR, x, s.xt, m0, m2, m1, r[6], r[9], r[7], r[10], 0, n, st));
                else HIP_TRY(launch_ew(EW_UNIPC_CORR1, x, s.xt, m0, m2, nullptr, r[6], 0, 0, r[10], 0, n, st));
                float* tmp = m1; m1 = m0; m0 = m2; m2 = tmp;
            } else {
                HIP_TRY(launch_ew(EW_COPY, x, xpred, nullptr, nullptr, nullptr, 0, 0, 0, 0, 0, n, st));
            }
        }
    } else if (method == LDS_METHOD_DDPM) {
        // row n: {t, sqrt_recip_ac, sqrt_recipm1_ac, coef1, coef2, mask*exp(0.5*logvar)}
        if (!noise) return set_error(LDS_EINVAL, "DDPM needs per-step noise");
        for (int i = 0; i < n_rows; ++i) {
            const float* r = table + (size_t)i * S;
            LDS_TRY(model(x, r[0]));
            HIP_TRY(launch_ew(EW_DDPM, x, x, s.eps, noise + (size_t)i * n, nullptr, r[1], r[2], r[3], r[4], r[5], n, st));
        }
    } else if (method == LDS_METHOD_DDIM) {
        // row n: {t, sqrt(a_prev), sqrt(a_t), sqrt((1-a_prev)/a_prev) - sqrt((1-a_t)/a_t)}
        for (int i = 0; i < n_rows; ++i) {
            const float* r = table + (size_t)i * S;
            LDS_TRY(model(x, r[0]));
            HIP_TRY(launch_ew(EW_DDIM, x, x, s.eps, nullptr, nullptr, r[1], r[2], r[3], 0, 0, n, st));
        }
    } else if (method == LDS_METHOD_PLMS) {
        // row n: {t, t_prev, a_prev - a_t, c1, c2}; eps history in m0 (latest) .. m2, working copy in xt
        int nh = 0;
        for (int i = 0; i < n_rows; ++i) {
            const float* r = table + (size_t)i * S;
            LDS_TRY(model(x, r[0]));
            float* e = s.xt;   // keep eps_t
            HIP_TRY(launch_ew(EW_COPY, e, s.eps, nullptr, nullptr, nullptr, 0, 0, 0, 0, 0, n, st));
            float* ep = s.xp;
            if (nh == 0) {
                HIP_TRY(launch_ew(EW_PLMS_PRED, ep, x, e, nullptr, nullptr, r[2], r[3], r[4], 0, 0, n, st));
                LDS_TRY(model(ep, r[1]));
                HIP_TRY(launch_ew(EW_LIN4, ep, e, s.eps, nullptr, nullptr, 1.f, 1.f, 0, 0, 2.f, n, st));
            } else if (nh == 1) {
                HIP_TRY(launch_ew(EW_LIN4, ep, e, m0, nullptr, nullptr, 3.f, -1.f, 0, 0, 2.f, n, st));
            } else if (nh == 2) {
                HIP_TRY(launch_ew(EW_LIN4, ep, e, m0, m1, nullptr, 23.f, -16.f, 5.f, 0, 12.f, n, st));
            } else {
                HIP_TRY(launch_ew(EW_LIN4, ep, e, m0, m1, m2, 55.f, -59.f, 37.f, -9.f, 24.f, n, st));
            }
            HIP_TRY(launch_ew(EW_PLMS_PRED, x, x, ep, nullptr, nullptr, r[2], r[3], r[4], 0, 0, n, st));
            float* tmp = m2; m2 = m1; m1 = m0; m0 = tmp;
            HIP_TRY(launch_ew(EW_COPY, m0, e, nullptr, nullptr, nullptr, 0, 0, 0, 0, 0, n, st));
            if (nh < 3) ++nh;
        }
    } else {
        return set_error(LDS_EINVAL, "unknown sampler method %d", method);
    }
    return LDS_OK;
}

// ================================================================================================
// Front end
// ================================================================================================
struct lds_embed {
    Owner own;
    int Cin = 0, H = 0, n_spk = 0;
    ConvW lin;
    float* spk = nullptr;
};

extern "C" int lds_embed_create(int input_channel, int n_hidden, int n_spk, const float* unit_w, const float* unit_b,
                                const float* spk_w, lds_embed** out) {
    if (!unit_w || !unit_b || !out || input_channel % 16 || n_hidden <= 0) return set_error(LDS_EINVAL, "bad argument");
    lds_embed* e = new lds_embed();
    e->Cin = input_channel; e->H = n_hidden; e->n_spk = (spk_w && n_spk > 1) ? n_spk : 0;
    bool ok = pack_conv(e->own, unit_w, unit_b, n_hidden, input_channel, 1, e->lin);
    if (ok && e->n_spk) { e->spk = up_vec(e->own, spk_w, (int64_t)n_spk * n_hidden); ok = e->spk != nullptr; }
    if (!ok) { delete e; return set_error(LDS_ENOMEM, "embed upload failed"); }
    *out = e;
    return LDS_OK;
}
extern "C" void lds_embed_destroy(lds_embed* e) { delete e; }
extern "C" int lds_embed_workspace_bytes(const lds_embed* e, int B, int T, size_t* out) {
    if (!e || !out) return set_error(LDS_EINVAL, "bad argument");
    Arena A(nullptr, 0);
    A.f((size_t)B * e->Cin * T);
    A.f((size_t)B * e->H);
    *out = A.used;
    return LDS_OK;
}
extern "C" int lds_embed_forward(lds_embed* e, const float* units, const int64_t* spk_id, float* cond, void* ws, size_t ws_bytes,
                                 int B, int T, void* stream) {
    if (!e || !units || !cond || !ws) return set_error(LDS_EINVAL, "bad argument");
    hipStream_t st = (hipStream_t)stream;
    Arena A(ws, ws_bytes);
    float* ut = A.f((size_t)B * e->Cin * T);
    float* sb = A.f((size_t)B * e->H);
    if (!A.ok) return set_error(LDS_ENOMEM, "embed workspace too small");
    HIP_TRY(launch_transpose(units, ut, B, T, e->Cin, 1.0f, st));          // [B,T,K] -> [B,K,T]
    ConvOpt o;
    if (e->n_spk) {
        if (!spk_id) return set_error(LDS_EINVAL, "spk_id required");
        HIP_TRY(launch_gather_rows(e->spk, spk_id, -1, sb, B, e->H, e->n_spk, st));
        o.bias_bc = sb;
    }
    Src s{ut, e->Cin, nullptr, 0, T};
    return run_conv(e->lin, s, o, cond, B, st);
}

extern "C" int lds_transpose(const float* in, float* out, int B, int R, int C, float scale, void* stream) {
    if (!in || !out) return set_error(LDS_EINVAL, "bad argument");
    HIP_TRY(launch_transpose(in, out, B, R, C, scale, (hipStream_t)stream));
    return LDS_OK;
}

extern "C" int lds_gather_rows(const float* table, const int64_t* idx, float* out, int n_idx, int C, int n_rows, void* stream) {
    if (!table || !idx || !out || n_idx <= 0 || C <= 0 || n_rows <= 0) return set_error(LDS_EINVAL, "bad argument");
    HIP_TRY(launch_gather_rows(table, idx, 0, out, n_idx, C, n_rows, (hipStream_t)stream));
    return LDS_OK;
}

extern "C" int lds_resample_frames(const float* in, float* out, int B, int Tin, int Tout, int C, float step, void* stream) {
    if (!in || !out) return set_error(LDS_EINVAL, "bad argument");
    HIP_TRY(launch_resample_frames(in, out, B, Tin, Tout, C, step, (hipStream_t)stream));
    return LDS_OK;
}

extern "C" int lds_axpby(float* out, const float* a, const float* b, float c0, float c1, int64_t n, void* stream) {
    if (!out || !a || !b || n <= 0) return set_error(LDS_EINVAL, "bad argument");
    HIP_TRY(launch_ew(EW_AXPBY, out, a, b, nullptr, nullptr, c0, -c1, 0, 0, 0, n, (hipStream_t)stream));
    return LDS_OK;
}

// ================================================================================================
// Vocoder
// ================================================================================================
struct VocRes { std::vector<ConvW> c1, c2; int k = 3; std::vector<int> dil; };
// What the generator (lds_vocoder) and the encoder (lds_vae_encoder) share: the config and the MRF weight sets, stage s owning
// rbs[s * n_kernels + j] (the reference's resblocks order in both directions)
struct VocNet {
    lds_vocoder_cfg cfg;
    Owner own;
    std::vector<VocRes> rbs;
};
struct lds_vocoder : VocNet {
    ConvW pre, post;
    std::vector<ConvW> ups;
};

// fold weight norm: w = g * v / ||v|| (norm over all dims but 0), reference hifi_vaegan.py:61
static bool get_folded(Tensors& T, const std::string& p, int64_t d0, int64_t rest, std::vector<float>& out) {
    if (T.has(p + "weight")) {
        const float* w = T.get(p + "weight", d0 * rest);
        if (!w) return false;
        out.assign(w, w + d0 * rest);
        return true;
    }
    const float* g = T.get(p + "weight_g", d0);
    const float* v = T.get(p + "weight_v", d0 * rest);
    if (!g || !v) return false;
    out.resize(d0 * rest);
    for (int64_t i = 0; i < d0; ++i) {
        double ss = 0;
        for (int64_t j = 0; j < rest; ++j) ss += (double)v[i * rest + j] * v[i * rest + j];
        const float sc = g[i] / (float)sqrt(ss);
        for (int64_t j = 0; j < rest; ++j) out[i * rest + j] = v[i * rest + j] * sc;
    }
    return true;
}

// The MRF weight sets of one stage (reference models.py:161-222): n_kernels resblocks at `ch` channels, appended to net.rbs
static bool load_mrf_stage(Tensors& T, VocNet& net, int stage, int ch) {
    const lds_vocoder_cfg* cfg = &net.cfg;
    Owner& o = net.own;
    std::vector<float> w;
    bool ok = true;
    for (int j = 0; j < cfg->n_kernels && ok; ++j) {
        VocRes rb;
        rb.k = cfg->resblock_kernel_sizes[j];
        if (rb.k != 3 && rb.k != 7 && rb.k != 11) { T.missing = "resblock kernel size must be 3, 7 or 11"; return false; }
        const std::string rp = "resblocks." + std::to_string(stage * cfg->n_kernels + j) + ".";
        for (int m = 0; m < cfg->n_dil && ok; ++m) {
            rb.dil.push_back(cfg->resblock_dilation_sizes[j][m]);
            if (rb.dil.back() < 1 || rb.dil.back() > 5) { T.missing = "dilation must be 1..5"; return false; }
            ConvW a, b;
            if (cfg->resblock == 1) {
                const std::string p1 = rp + "convs1." + std::to_string(m) + ".", p2 = rp + "convs2." + std::to_string(m) + ".";
                ok = get_folded(T, p1, ch, (int64_t)ch * rb.k, w) && pack_conv(o, w.data(), T.get(p1 + "bias", ch), ch, ch, rb.k, a);
                ok = ok && get_folded(T, p2, ch, (int64_t)ch * rb.k, w) && pack_conv(o, w.data(), T.get(p2 + "bias", ch), ch, ch, rb.k, b);
                rb.c1.push_back(a);
                rb.c2.push_back(b);
            } else {
                const std::string p1 = rp + "convs." + std::to_string(m) + ".";
                ok = get_folded(T, p1, ch, (int64_t)ch * rb.k, w) && pack_conv(o, w.data(), T.get(p1 + "bias", ch), ch, ch, rb.k, a);
                rb.c1.push_back(a);
            }
        }
        net.rbs.push_back(rb);
    }
    return ok;
}

extern "C" int lds_vocoder_create(const lds_vocoder_cfg* cfg, int n, const char* const* names, const float* const* ptrs,
                                  const int64_t* numel, lds_vocoder** out) {
    if (!cfg || !names || !ptrs || !numel || !out) return set_error(LDS_EINVAL, "null argument");
    if (cfg->n_ups < 1 || cfg->n_ups > 8 || cfg->n_kernels < 1 || cfg->n_kernels > 4 || cfg->n_dil < 1 || cfg->n_dil > 4)
        return set_error(LDS_EINVAL, "vocoder config out of range");
    Tensors T;
    for (int i = 0; i < n; ++i) T.m[names[i]] = {ptrs[i], numel[i]};
    lds_vocoder* v = new lds_vocoder();
    v->cfg = *cfg;
    Owner& o = v->own;
    bool ok = true;
    std::vector<float> w;
    const int c0 = cfg->upsample_initial_channel, ci = cfg->inter_channels;
    if (ci % 16) { delete v; return set_error(LDS_EINVAL, "inter_channels must be a multiple of 16"); }
    ok = get_folded(T, "conv_pre.", c0, (int64_t)ci * 7, w) && pack_conv(o, w.data(), T.get("conv_pre.bias", c0), c0, ci, 7, v->pre);
    int ch = c0;
    for (int i = 0; i < cfg->n_ups && ok; ++i) {
        const int cin = c0 >> i, cout = c0 >> (i + 1), k = cfg->upsample_kernel_sizes[i], s = cfg->upsample_rates[i];
        if (cout < 16 || (cout % 16) || k % s != 0 || ((k - s) % 2) != 0) { ok = false; T.missing = "unsupported upsample geometry"; break; }
        const std::string p = "ups." + std::to_string(i) + ".";
        ConvW cw;
        ok = get_folded(T, p, cin, (int64_t)cout * k, w) && pack_convT(o, w.data(), T.get(p + "bias", cout), cin, cout, k, s, cw);
        v->ups.push_back(cw);
        ch = cout;
        ok = ok && load_mrf_stage(T, *v, i, ch);
    }
    ok = ok && get_folded(T, "conv_post.", 1, (int64_t)ch * 7, w) && pack_conv(o, w.data(), T.get("conv_post.bias", 1), 1, ch, 7, v->post);
    if (!ok) {
        std::string miss = T.missing;
        delete v;
        if (!miss.empty()) return set_error(LDS_EMISSING, "vocoder: %s", miss.c_str());
        return set_error(LDS_ENOMEM, "vocoder weight upload failed");
    }
    *out = v;
    return LDS_OK;
}
extern "C" void lds_vocoder_destroy(lds_vocoder* v) { delete v; }

// Stages whose width is a multiple of 64 run on the DMA-fed K4P kernel (conv_dma): the tensors between the resblock convolutions
// live in K4P with kVocPad zero frames per side (the dilated k 7 / 11 taps reach 25 frames out), LeakyReLU is applied once per
// tensor by the producer's epilogue, and the MRF's running sum is accumulated in K4P.  Narrower stages (the 32 / 16-channel
// tail) and their upsamplers stay on the register-staged conv_gemm / conv_small over plain tensors.
constexpr int kVocPad = 32;
struct VocWs { float *x, *xs, *ta, *ra, *rb; float *kx_raw, *kx_act, *kt_act, *ka_raw, *ka_act, *kb_raw, *kb_act, *ks, *kin; int* vlens; };
static bool voc_dma_stage(const VocNet* v, int ch) {
    if (ch % 64) return false;
    for (const VocRes& rb : v->rbs)
        for (int d : rb.dil)
            if ((rb.k * d - d) / 2 > kVocPad || (d != 1 && d != 3 && d != 5)) return false;
    return true;
}
// the upsampler in front of a DMA stage runs on conv_dma too (polyphase rows, 2 taps per phase, power-of-two rate) and writes the
// stage's K4P tensors directly; its input is the previous stage's MRF output kept in K4P with LeakyReLU applied (VocWs::kin)
static bool voc_dma_ups(const lds_vocoder* v, int i) {
    const int s = v->cfg.upsample_rates[i], ch = v->cfg.upsample_initial_channel >> (i + 1);
    return voc_dma_stage(v, ch) && v->ups[i].K == 2 && (s & (s - 1)) == 0 && s <= 16 && v->ups[i].Mp == v->ups[i].Co && (2 * ch) % 16 == 0;
}
static void plan_voc(const lds_vocoder* v, Arena& A, int B, int T, VocWs& w) {
    size_t mx = (size_t)v->cfg.upsample_initial_channel * T, mk = 0;
    int Tl = T;
    for (int i = 0; i < v->cfg.n_ups; ++i) {
        if (voc_dma_ups(v, i)) mk = std::max(mk, (size_t)(v->cfg.upsample_initial_channel >> i) * (Tl + 2 * kVocPad));      // kin
        Tl *= v->cfg.upsample_rates[i];
        const int ch = v->cfg.upsample_initial_channel >> (i + 1);
        const size_t ct = (size_t)ch * Tl;
        if (ct > mx) mx = ct;
        if (voc_dma_stage(v, ch)) mk = std::max(mk, (size_t)ch * (Tl + 2 * kVocPad));
    }
    w.x = A.f(B * mx); w.xs = A.f(B * mx); w.ta = A.f(B * mx); w.ra = A.f(B * mx); w.rb = A.f(B * mx);
    float** kb[9] = {&w.kx_raw, &w.kx_act, &w.kt_act, &w.ka_raw, &w.ka_act, &w.kb_raw, &w.kb_act, &w.ks, &w.kin};
    for (float** pp : kb) *pp = mk ? A.f(B * mk + 4096) : nullptr;
    w.vlens = (int*)A.f(9 * 64);      // ragged batches: per-stage valid lengths of <= 64 utterances
}
extern "C" int lds_vocoder_workspace_bytes(const lds_vocoder* v, int B, int T, size_t* out) {
    if (!v || !out || B <= 0 || T <= 0) return set_error(LDS_EINVAL, "bad argument");
    Arena A(nullptr, 0);
    VocWs w;
    plan_voc(v, A, B, T, w);
    *out = A.used;
    return LDS_OK;
}

// MRF of one stage on the K4P / LDS-DMA path (reference models.py:161-222,250-259): x plain [B][ch][Tl] (null: the upsampler has
// already written kx_raw / kx_act) -> mean_j resblock_j(x), to xs plain, or (xs null) as LeakyReLU(0.1)(.) to the K4P tensor kin,
// the next upsampler's input
static int voc_mrf_dma(const VocNet* v, const VocWs& w, int stage, const float* x, float* xs, int ch, int Tl, int B, hipStream_t st, const int* vlen = nullptr) {
    const lds_vocoder_cfg& c = v->cfg;
    const int P = kVocPad;
    if (x) HIP_TRY(launch_to_k4p_act(x, w.kx_raw, w.kx_act, 0.1f, B, ch, Tl, P, st, vlen));
    float* acts[4] = {w.kx_act, w.kt_act, w.ka_act, w.kb_act};
    for (float* a : acts) HIP_TRY(launch_k4p_zero_pads(a, B, ch, Tl, P, st));      // the epilogues below store real frames only
    if (!xs) HIP_TRY(launch_k4p_zero_pads(w.kin, B, ch, Tl, P, st));
    for (int j = 0; j < c.n_kernels; ++j) {
        const VocRes& rb = v->rbs[stage * c.n_kernels + j];
        const float* cur_raw = w.kx_raw;
        const float* cur_act = w.kx_act;
        float* nraw[2] = {w.ka_raw, w.kb_raw};
        float* nact[2] = {w.ka_act, w.kb_act};
        const int nd = (int)rb.dil.size();
        for (int m = 0; m < nd; ++m) {
            const bool last = m == nd - 1;
            const int d = rb.dil[m];
            const float* in2 = cur_act;
            DOpt o2;                                   // the convolution that closes the residual step: x = conv(...) + x
            o2.voc = 1; o2.xpad = P; o2.opad = P; o2.res = cur_raw; o2.vlen = vlen;
            const ConvW* W2 = &rb.c1[m];
            if (c.resblock == 1) {
                DOpt o1;                               // xt = c1(lrelu(x)), stored as lrelu(xt)
                o1.voc = 1; o1.xpad = P; o1.opad = P; o1.dil = d; o1.pad = (rb.k * d - d) / 2; o1.act_slope = 0.1f; o1.vlen = vlen;
                LDS_TRY(run_dconv(rb.c1[m], cur_act, ch, nullptr, 0, Tl, o1, w.kt_act, B, st));
                in2 = w.kt_act; W2 = &rb.c2[m];
                o2.pad = (rb.k - 1) / 2;
            } else {
                o2.dil = d; o2.pad = (rb.k * d - d) / 2;
            }
            float* dst;
            if (!last) {                               // raw value (next residual) + LeakyReLU'd value (next convolution's input)
                dst = nraw[m & 1]; o2.out_act = nact[m & 1]; o2.act_slope = 0.1f;
            } else if (j < c.n_kernels - 1) {          // xs (+)= resblock_j(x), kept in K4P
                dst = w.ks; o2.acc_in = (j > 0) ? w.ks : nullptr;
            } else if (xs) {                           // xs = (xs + resblock_j(x)) / n_kernels, back in the plain layout
                dst = xs; o2.out_plain = 1; o2.acc_in = (j > 0) ? w.ks : nullptr; o2.out_div = (float)c.n_kernels;
            } else {                                   // ... or LeakyReLU'd in K4P for the next upsampler
                dst = w.kin; o2.acc_in = (j > 0) ? w.ks : nullptr; o2.out_div = (float)c.n_kernels; o2.act_slope = 0.1f;
            }
            LDS_TRY(run_dconv(*W2, in2, ch, nullptr, 0, Tl, o2, dst, B, st));
            cur_raw = nraw[m & 1]; cur_act = nact[m & 1];
        }
    }
    return LDS_OK;
}

// One residual step of ResBlock1 on a narrow stage as one launch (voc_pair.hip): out = (accum ? out : 0) + c2(lrelu(c1(lrelu(x)))) + x, / div
static int run_voc_pair(const ConvW& W1, const ConvW& W2, const float* x, float* out, int ch, int Tl, int dil, bool accum, float div, const int* vlen, int B,
                        hipStream_t st) {
    VocPairArgs a;
    memset(&a, 0, sizeof(a));
    a.x = x; a.out = out; a.w1 = W1.w; a.b1 = W1.bias; a.Mp1 = W1.Mp; a.w2 = W2.w; a.b2 = W2.bias; a.Mp2 = W2.Mp;
    a.C = ch; a.KT = W1.K; a.dil = dil; a.B = B; a.T = Tl; a.accum = accum ? 1 : 0; a.out_div = div; a.slope = 0.1f; a.vlen = vlen;
    const double flops = 2.0 * 2.0 * B * (double)Tl * ch * ch * W1.K;
    const double bytes = 4.0 * B * (double)ch * Tl * (accum ? 3.0 : 2.0);
    hipError_t e;
    {
        ProfScope ps(st, "voc_pair", flops, bytes);
        e = launch_voc_pair(a, st);
        if (ps.on) {
            std::string cfgs(voc_pair_last_config());
            std::string nm = "voc_pair<" + cfgs.substr(0, cfgs.find(" grid")) + ">";
            if (g_prof_level.load(std::memory_order_relaxed) >= 2) {
                char sh[96];
                snprintf(sh, sizeof(sh), " Ci%d Co%d K%d+%d d%d To%d +res%s", ch, ch, W1.K, W2.K, dil, Tl, accum ? " +acc" : "");
                nm += sh;
            }
            ps.rename(nm);
        }
    }
    if (e != hipSuccess) return set_error(LDS_EHIP, "voc_pair launch failed (%s): C %d K %d dil %d T %d", hipGetErrorString(e), ch, W1.K, dil, Tl);
    return LDS_OK;
}
static bool voc_pair_ok(const lds_vocoder_cfg& c, const VocRes& rb, int m, int ch) {
    return c.resblock == 1 && g_voc_pair.load(std::memory_order_relaxed) && voc_pair_applies(ch, rb.k, rb.dil[m]) && rb.c1[m].Mp == 32 && rb.c2[m].Mp == 32;
}

// MRF of one narrow stage on the register-staged kernels over plain tensors (voc_pair / conv_small / conv_gemm): x [B][ch][Tl] ->
// xs = mean_j resblock_j(x), through the scratch tensors w.ra / w.rb / w.ta
static int voc_mrf_plain(const VocNet* v, const VocWs& w, int stage, const float* x, float* xs, int ch, int Tl, int B, hipStream_t st,
                         const int* vlen) {
    const lds_vocoder_cfg& c = v->cfg;
    for (int j = 0; j < c.n_kernels; ++j) {
        const VocRes& rb = v->rbs[stage * c.n_kernels + j];
        const float* cur = x;
        float* pp[2] = {w.ra, w.rb};
        const int nd = (int)rb.dil.size();
        for (int m = 0; m < nd; ++m) {
            const bool last = m == nd - 1;
            const int d = rb.dil[m];
            Src s1{cur, ch, nullptr, 0, Tl};
            ConvOpt o1;
            o1.dil = d; o1.pad = (rb.k * d - d) / 2; o1.act_in = ACT_LRELU; o1.slope = 0.1f; o1.vlen = vlen;
            ConvOpt o2;
            o2.res = cur; o2.vlen = vlen;
            if (last) { o2.accum = j > 0; o2.out_div = (j == c.n_kernels - 1) ? (float)c.n_kernels : 1.0f; }
            float* dst = last ? xs : pp[m & 1];
            if (voc_pair_ok(c, rb, m, ch)) {
                LDS_TRY(run_voc_pair(rb.c1[m], rb.c2[m], cur, dst, ch, Tl, d, o2.accum != 0, o2.out_div, vlen, B, st));
            } else if (c.resblock == 1) {
                LDS_TRY(run_conv(rb.c1[m], s1, o1, w.ta, B, st));
                Src s2{w.ta, ch, nullptr, 0, Tl};
                o2.pad = (rb.k - 1) / 2; o2.act_in = ACT_LRELU; o2.slope = 0.1f;
                LDS_TRY(run_conv(rb.c2[m], s2, o2, dst, B, st));
            } else {
                o2.dil = d; o2.pad = o1.pad; o2.act_in = ACT_LRELU; o2.slope = 0.1f;
                LDS_TRY(run_conv(rb.c1[m], s1, o2, dst, B, st));
            }
            cur = dst;
        }
    }
    return LDS_OK;
}

static int vocoder_forward_impl(lds_vocoder* v, const float* z, float* wav, void* ws, size_t ws_bytes, int B, int T, void* stream, const int* lens_host);
extern "C" int lds_vocoder_forward(lds_vocoder* v, const float* z, float* wav, void* ws, size_t ws_bytes, int B, int T, void* stream) {
    return vocoder_forward_impl(v, z, wav, ws, ws_bytes, B, T, stream, nullptr);
}
extern "C" int lds_vocoder_forward_ragged(lds_vocoder* v, const float* z, const int32_t* lengths, float* wav, void* ws, size_t ws_bytes, int B, int T, void* stream) {
    if (!lengths) return set_error(LDS_EINVAL, "bad argument");
    return vocoder_forward_impl(v, z, wav, ws, ws_bytes, B, T, stream, lengths);
}
static int vocoder_forward_impl(lds_vocoder* v, const float* z, float* wav, void* ws, size_t ws_bytes, int B, int T, void* stream, const int* lens_host) {
    if (!v || !z || !wav || !ws || B <= 0 || T <= 0) return set_error(LDS_EINVAL, "bad argument");
    hipStream_t st = (hipStream_t)stream;
    ProfChain chain;
    Arena A(ws, ws_bytes);
    VocWs w;
    plan_voc(v, A, B, T, w);
    if (!A.ok) return set_error(LDS_ENOMEM, "vocoder workspace too small: need %zu", A.used);
    const lds_vocoder_cfg& c = v->cfg;
    // Ragged batch: stage s of utterance b has vl[s][b] valid frames (the transposed convolutions' own length formula applied to the
    // utterance's length); every stage writes zeros beyond them, which is the zero padding the utterance's convolutions see when it runs
    // alone.  The lists travel in kernel arguments (<= 64 utterances).
    std::vector<const int*> vl(c.n_ups + 1, nullptr);
    if (lens_host) {
        if (B > 64) return set_error(LDS_EINVAL, "per-utterance lengths: at most 64 utterances per call (got %d)", B);
        std::vector<int> cur(lens_host, lens_host + B);
        for (int i = 0; i <= c.n_ups; ++i) {
            float tmp[64];
            for (int b = 0; b < B; ++b) {
                if (i == 0 && (cur[b] < 1 || cur[b] > T)) return set_error(LDS_EINVAL, "length[%d] = %d outside 1 .. %d", b, cur[b], T);
                memcpy(&tmp[b], &cur[b], sizeof(int));
            }
            HIP_TRY(launch_set_list((float*)(w.vlens + 64 * i), tmp, B, st));
            vl[i] = w.vlens + 64 * i;
            if (i < c.n_ups) {
                const int s_ = c.upsample_rates[i], k = c.upsample_kernel_sizes[i];
                for (int b = 0; b < B; ++b) cur[b] = (cur[b] - 1) * s_ - 2 * ((k - s_ + 1) / 2) + k;
            }
        }
    }
    // reference models.py:248-262
    {
        Src s{z, c.inter_channels, nullptr, 0, T};
        ConvOpt o;
        o.pad = 3; o.vlen = vl[0]; o.vlen_in = vl[0];
        LDS_TRY(run_conv(v->pre, s, o, w.x, B, st));
    }
    int ch = c.upsample_initial_channel, Tl = T;
    float* x = w.x;
    float* xs = w.xs;
    bool k4p_in = false;      // the current tensor lives in w.kin (K4P, LeakyReLU applied) instead of x
    for (int i = 0; i < c.n_ups; ++i) {
        const int s_ = c.upsample_rates[i], k = c.upsample_kernel_sizes[i], cout = ch / 2;
        const int Tn = (Tl - 1) * s_ - 2 * ((k - s_ + 1) / 2) + k;
        const bool k4p_next = i + 1 < c.n_ups && voc_dma_ups(v, i + 1);      // this stage's output feeds a DMA upsampler
        if (voc_dma_ups(v, i)) {
            // x = ups[i](leaky_relu(x, 0.1)) on conv_dma: K4P in (kin), the stage's kx_raw / kx_act out
            if (!k4p_in) {
                HIP_TRY(launch_to_k4p_act(x, w.kx_raw, w.kin, 0.1f, B, ch, Tl, kVocPad, st, vl[i]));      // (kx_raw: scratch for the unused raw copy)
                HIP_TRY(launch_k4p_zero_pads(w.kin, B, ch, Tl, kVocPad, st));
            }
            int lg = 0;
            while ((1 << lg) < s_) ++lg;
            DOpt o;
            o.voc = 1; o.xpad = kVocPad; o.opad = kVocPad; o.pad = 1; o.act_slope = 0.1f; o.out_act = w.kx_act;
            o.ph_log2 = lg; o.ph_tpad = (k - s_ + 1) / 2; o.ph_Tout = Tn; o.vlen = vl[i + 1];
            LDS_TRY(run_dconv(v->ups[i], w.kin, ch, nullptr, 0, Tl, o, w.kx_raw, B, st));
            ch = cout; Tl = Tn;
            LDS_TRY(voc_mrf_dma(v, w, i, nullptr, k4p_next ? nullptr : xs, ch, Tl, B, st, vl[i + 1]));
            if (!k4p_next) { float* t = x; x = xs; xs = t; }
            k4p_in = k4p_next;
            continue;
        }
        {
            // x = ups[i](leaky_relu(x, 0.1)) as a polyphase conv
            Src s{x, ch, nullptr, 0, Tl};
            ConvOpt o;
            o.pad = v->ups[i].K - 1; o.act_in = ACT_LRELU; o.slope = 0.1f;
            o.phases = s_; o.tpad = (k - s_ + 1) / 2; o.To = Tl + 1; o.Tout = Tn; o.Cout = cout; o.vlen = vl[i + 1]; o.vlen_in = vl[i];
            LDS_TRY(run_conv(v->ups[i], s, o, xs, B, st));
        }
        { float* t = x; x = xs; xs = t; }
        ch = cout; Tl = Tn;
        if (voc_dma_stage(v, ch)) {
            LDS_TRY(voc_mrf_dma(v, w, i, x, xs, ch, Tl, B, st, vl[i + 1]));
            { float* t = x; x = xs; xs = t; }
            continue;
        }
        LDS_TRY(voc_mrf_plain(v, w, i, x, xs, ch, Tl, B, st, vl[i + 1]));
        { float* t = x; x = xs; xs = t; }
    }
    Src s{x, ch, nullptr, 0, Tl};
    ConvOpt o;
    o.pad = 3; o.act_in = ACT_LRELU; o.slope = 0.01f; o.epi = EPI_TANH; o.vlen = vl[c.n_ups];
    return run_conv(v->post, s, o, wav, B, st);
}

// ================================================================================================
// VAE encoder (audio -> latent): the generator run backwards (reference models.py:14-67, hifi_vaegan.py:32-50)
// ================================================================================================
// conv_pre, the downsamplers and conv_post keep the reference's unpacked [Co][Ci][K] weights: conv_down (conv_down.hip) reads them as
// the A operand of its implicit GEMM as they are
struct DownW { float* w = nullptr; float* bias = nullptr; int Co = 0, Ci = 0, K = 0, stride = 1, pad = 0; };
struct lds_vae_encoder : VocNet {
    DownW pre, post;
    std::vector<DownW> downs;      // downs[i]: stage i, stride rates[n_ups - 1 - i]
    int hop = 1;
};

static bool load_down(Tensors& T, Owner& o, const std::string& p, int Co, int Ci, int K, int stride, int pad, DownW& d) {
    std::vector<float> w;
    if (!get_folded(T, p, Co, (int64_t)Ci * K, w)) return false;      // Conv1d weight norm: over dims 1, 2 of [Co][Ci][K]
    const float* b = T.get(p + "bias", Co);
    if (!b) return false;
    d.w = o.upload(w);
    d.bias = o.upload(std::vector<float>(b, b + Co));
    d.Co = Co; d.Ci = Ci; d.K = K; d.stride = stride; d.pad = pad;
    return d.w && d.bias;
}

// the geometry the downsamplers support: k = 2u, u a power of two in 2 .. 16 (padding (k - u + 1) / 2 = u / 2, L -> L / u)
static bool down_geometry_ok(int u, int k) { return u >= 2 && u <= 16 && (u & (u - 1)) == 0 && k == 2 * u; }

extern "C" int lds_vae_encoder_create(const lds_vocoder_cfg* cfg, int n, const char* const* names, const float* const* ptrs,
                                      const int64_t* numel, lds_vae_encoder** out) {
    if (!cfg || !names || !ptrs || !numel || !out || n < 0) return set_error(LDS_EINVAL, "null argument");
    if (cfg->n_ups < 1 || cfg->n_ups > 8 || cfg->n_kernels < 1 || cfg->n_kernels > 4 || cfg->n_dil < 1 || cfg->n_dil > 4 || cfg->inter_channels < 1 ||
        cfg->upsample_initial_channel < 1)
        return set_error(LDS_EINVAL, "encoder config out of range");
    const int nu = cfg->n_ups, c0 = cfg->upsample_initial_channel;
    if ((c0 >> nu) < 1 || (c0 >> nu) << nu != c0) return set_error(LDS_EINVAL, "encoder: upsample_initial_channel must be divisible by 2^n_ups");
    int hop = 1;
    for (int i = 0; i < nu; ++i) {
        const int u = cfg->upsample_rates[nu - 1 - i], k = cfg->upsample_kernel_sizes[nu - 1 - i], cout = c0 >> (nu - 1 - i);
        if (!down_geometry_ok(u, k)) return set_error(LDS_EINVAL, "encoder: unsupported downsample geometry (stride %d, kernel %d; needs k = 2u, u a power of two <= 16)", u, k);
        if (cout < 16 || cout % 16) return set_error(LDS_EINVAL, "encoder: unsupported stage width %d (a multiple of 16 is needed)", cout);
        hop *= u;
    }
    Tensors T;
    for (int i = 0; i < n; ++i) T.m[names[i]] = {ptrs[i], numel[i]};
    lds_vae_encoder* e = new lds_vae_encoder();
    e->cfg = *cfg;
    e->hop = hop;
    bool ok = load_down(T, e->own, "conv_pre.", c0 >> nu, 1, 7, 1, 3, e->pre);
    for (int i = 0; i < nu && ok; ++i) {
        const int u = cfg->upsample_rates[nu - 1 - i], k = cfg->upsample_kernel_sizes[nu - 1 - i];
        const int cin = c0 >> (nu - i), cout = c0 >> (nu - 1 - i);
        DownW d;
        ok = load_down(T, e->own, "ups." + std::to_string(i) + ".", cout, cin, k, u, (k - u + 1) / 2, d);
        e->downs.push_back(d);
        ok = ok && load_mrf_stage(T, *e, i, cout);
    }
    ok = ok && load_down(T, e->own, "conv_post.", 2 * cfg->inter_channels, c0, 7, 1, 3, e->post);
    if (!ok) {
        std::string miss = T.missing;
        delete e;
        if (!miss.empty()) return set_error(LDS_EMISSING, "encoder: %s", miss.c_str());
        return set_error(LDS_ENOMEM, "encoder weight upload failed");
    }
    *out = e;
    return LDS_OK;
}
extern "C" void lds_vae_encoder_destroy(lds_vae_encoder* e) { delete e; }

struct EncWs { VocWs v; float* y; };
static bool enc_args_ok(const lds_vae_encoder* e, int B, int64_t L) {
    return e && B > 0 && B <= 65535 && L > 0 && L % e->hop == 0 && L <= (int64_t)1 << 30;
}
// Stage tensors ping-pong through v.x / v.xs ([B][16][L] after conv_pre is the widest: every stage halves the width at least as often
// as it doubles the channels); y = conv_post's [B][2C][T].  The plain MRF stages' scratch (ta, ra, rb) and the DMA-fed stages' K4P
// tensors (sized as in plan_voc) share one region: every stage writes the scratch it reads before reading it, and the stages run one
// after the other on the stream, so a narrow stage and a DMA stage never hold it at the same time.
static void plan_enc(const lds_vae_encoder* e, Arena& A, int B, int64_t L, EncWs& w) {
    size_t mx = (size_t)e->pre.Co * L, mk = 0, mp = 0;
    int64_t Tl = L;
    for (const DownW& d : e->downs) {
        Tl /= d.stride;
        mx = std::max(mx, (size_t)d.Co * Tl);
        if (voc_dma_stage(e, d.Co)) mk = std::max(mk, (size_t)d.Co * (Tl + 2 * kVocPad));
        else mp = std::max(mp, (size_t)d.Co * Tl);
    }
    VocWs& v = w.v;
    v.x = A.f(B * mx); v.xs = A.f(B * mx);
    auto rnd = [](size_t n) { return (n * sizeof(float) + 255) / 256 * 256 / sizeof(float); };      // Arena's slot rounding
    const size_t plain = mp ? rnd(B * mp) : 0, k4 = mk ? rnd(B * mk + 4096) : 0;
    float* shared = A.f(std::max(3 * plain, 8 * k4));
    v.ta = v.ra = v.rb = nullptr;      // (planning without a buffer: every pointer stays null)
    if (mp && shared) { v.ta = shared; v.ra = shared + plain; v.rb = shared + 2 * plain; }
    float** kb[8] = {&v.kx_raw, &v.kx_act, &v.kt_act, &v.ka_raw, &v.ka_act, &v.kb_raw, &v.kb_act, &v.ks};
    for (int i = 0; i < 8; ++i) *kb[i] = (mk && shared) ? shared + i * k4 : nullptr;
    v.kin = nullptr;      // (the encoder's MRF stages always return a plain tensor)
    w.y = A.f((size_t)B * e->post.Co * (L / e->hop));
    v.vlens = (int*)A.f((e->downs.size() + 2) * 64);      // ragged batches: the sample lengths and every stage's lengths, <= 64 clips
}
extern "C" int lds_vae_encoder_workspace_bytes(const lds_vae_encoder* e, int B, int64_t L, size_t* out) {
    if (!out || !enc_args_ok(e, B, L)) return set_error(LDS_EINVAL, "bad argument (B %d, L %lld: B >= 1 and L a positive multiple of the hop)", B, (long long)L);
    Arena A(nullptr, 0);
    EncWs w;
    plan_enc(e, A, B, L, w);
    *out = A.used;
    return LDS_OK;
}

static int run_down(const DownW& d, const float* x, int64_t L, float slope, float* out, int B, hipStream_t st, int tile = 0, const int* vlen_in = nullptr,
                    const int* vlen = nullptr) {
    ConvDownArgs a;
    memset(&a, 0, sizeof(a));
    a.x = x; a.w = d.w; a.bias = d.bias; a.out = out; a.vlen_in = vlen_in; a.vlen = vlen;
    a.Ci = d.Ci; a.Co = d.Co; a.K = d.K; a.stride = d.stride; a.pad = d.pad; a.L = (int)L; a.B = B; a.slope = slope; a.tile = tile;
    a.To = (int)((L + 2 * d.pad - d.K) / d.stride + 1);
    const double flops = 2.0 * B * (double)a.To * d.Co * (double)d.Ci * d.K;
    const double bytes = 4.0 * ((double)B * d.Ci * L + (double)d.Co * d.Ci * d.K + (double)B * d.Co * a.To);
    hipError_t e;
    {
        ProfScope ps(st, "conv_down", flops, bytes);
        e = launch_conv_down(a, st);
        if (ps.on) {
            std::string cfgs(conv_down_last_config());
            std::string nm = "conv_down<" + cfgs.substr(0, cfgs.find(" grid")) + ">";
            if (g_prof_level.load(std::memory_order_relaxed) >= 2) {
                char sh[96];
                snprintf(sh, sizeof(sh), " Ci%d Co%d K%d s%d To%d", d.Ci, d.Co, d.K, d.stride, a.To);
                nm += sh;
            }
            ps.rename(nm);
        }
    }
    if (e != hipSuccess)
        return set_error(LDS_EHIP, "conv_down launch failed (%s): Co %d Ci %d K %d stride %d L %lld", hipGetErrorString(e), d.Co, d.Ci, d.K, d.stride, (long long)L);
    return LDS_OK;
}

static int vae_encoder_forward_impl(lds_vae_encoder* e, const float* audio, const int32_t* lens_host, const float* noise, float* out, float* z,
                                    int only_mean, void* ws, size_t ws_bytes, int B, int64_t L, void* stream);
extern "C" int lds_vae_encoder_forward(lds_vae_encoder* e, const float* audio, const float* noise, float* out, float* z, int only_mean, void* ws,
                                       size_t ws_bytes, int B, int64_t L, void* stream) {
    return vae_encoder_forward_impl(e, audio, nullptr, noise, out, z, only_mean, ws, ws_bytes, B, L, stream);
}
extern "C" int lds_vae_encoder_forward_ragged(lds_vae_encoder* e, const float* audio, const int32_t* lengths, const float* noise, float* out, float* z,
                                              int only_mean, void* ws, size_t ws_bytes, int B, int64_t L, void* stream) {
    if (!lengths) return set_error(LDS_EINVAL, "bad argument: lengths is null");
    // more than 64 clips is refused before the other arguments are judged (clip_lens_check says so), the values after them
    if (B <= 64 && !enc_args_ok(e, B, L)) return set_error(LDS_EINVAL, "bad argument (B %d, L %lld: B >= 1 and L a positive multiple of the hop)", B, (long long)L);
    LDS_TRY(clip_lens_check("length", lengths, B, 1, L));
    return vae_encoder_forward_impl(e, audio, lengths, noise, out, z, only_mean, ws, ws_bytes, B, L, stream);
}
static int vae_encoder_forward_impl(lds_vae_encoder* e, const float* audio, const int32_t* lens_host, const float* noise, float* out, float* z,
                                    int only_mean, void* ws, size_t ws_bytes, int B, int64_t L, void* stream) {
    if (!audio || !out || !ws || (z && !noise) || !enc_args_ok(e, B, L)) return set_error(LDS_EINVAL, "bad argument");
    hipStream_t st = (hipStream_t)stream;
    ProfChain chain;
    Arena A(ws, ws_bytes);
    EncWs w;
    plan_enc(e, A, B, L, w);
    if (!A.ok) return set_error(LDS_ENOMEM, "encoder workspace too small: need %zu", A.used);
    // Ragged batch: clip b is audio[b, :len_b] encoded alone, i.e. zero-padded to Lp_b = ceil(len_b / hop) * hop samples.  vl[0] = len_b
    // (conv_pre reads the audio as zeros from there on), vl[1] = Lp_b (conv_pre's output), vl[2 + i] = Lp_b / (u_0 ... u_i) after
    // downsampler i (k = 2u, pad u / 2: a multiple of u maps to L / u exactly); the last is the clip's frame count T_b.  Every stage
    // stores zeros beyond its length, which is the zero padding the clip's convolutions see when it runs alone.
    const size_t nd = e->downs.size();
    std::vector<const int*> vl(nd + 2, nullptr);
    if (lens_host) {
        std::vector<int64_t> cur(B);
        for (int b = 0; b < B; ++b) cur[b] = lens_host[b];
        for (size_t i = 0; i < nd + 2; ++i) {
            float tmp[64];
            for (int b = 0; b < B; ++b) {
                const int v = (int)cur[b];
                memcpy(&tmp[b], &v, sizeof(int));
            }
            HIP_TRY(launch_set_list((float*)(w.v.vlens + 64 * i), tmp, B, st));
            vl[i] = w.v.vlens + 64 * i;
            for (int b = 0; b < B; ++b) {
                if (i == 0) cur[b] = (cur[b] + e->hop - 1) / e->hop * e->hop;
                else if (i <= nd) cur[b] /= e->downs[i - 1].stride;
            }
        }
    }
    // reference models.py:39-54
    LDS_TRY(run_down(e->pre, audio, L, 1.0f, w.v.x, B, st, 0, vl[0], vl[1]));
    float* x = w.v.x;
    float* xs = w.v.xs;
    int64_t Tl = L;
    for (size_t i = 0; i < nd; ++i) {
        const DownW& d = e->downs[i];
        const int* vlen = vl[i + 2];
        LDS_TRY(run_down(d, x, Tl, 0.1f, xs, B, st, 0, vl[i + 1], vlen));      // x = ups[i](leaky_relu(x, 0.1))
        { float* t = x; x = xs; xs = t; }
        Tl /= d.stride;
        if (voc_dma_stage(e, d.Co)) LDS_TRY(voc_mrf_dma(e, w.v, (int)i, x, xs, d.Co, (int)Tl, B, st, vlen));
        else LDS_TRY(voc_mrf_plain(e, w.v, (int)i, x, xs, d.Co, (int)Tl, B, st, vlen));
        { float* t = x; x = xs; xs = t; }
    }
    LDS_TRY(run_down(e->post, x, Tl, 0.01f, w.y, B, st, 0, vl[nd + 1], vl[nd + 1]));      // conv_post(leaky_relu(x)) -> [B][2C][T]
    HIP_TRY(launch_vae_head(w.y, noise, out, z, B, e->cfg.inter_channels, (int)Tl, only_mean, st, vl[nd + 1]));
    return LDS_OK;
}

// ================================================================================================
// Units encoders: what Whisper, HuBERT, wav2vec 2.0 and w2v-BERT 2.0 below state in common on top of host.h (WeightLoader, plan_bytes,
// upload_clip_ints, the dimension rules).  Nothing here launches on its own account: the four *_run functions stay the sequences of launches.
// ================================================================================================
// q | k | v as one [3C][C] weight and one [3C] bias; kb may be null (Whisper's key has no bias): zeros
struct QkvCat { std::vector<float> w, b; };
static QkvCat cat_qkv(const float* qw, const float* kw, const float* vw, const float* qb, const float* kb, const float* vb, int C) {
    const size_t CC = (size_t)C * C;
    QkvCat q{std::vector<float>(3 * CC), std::vector<float>((size_t)3 * C, 0.f)};
    memcpy(q.w.data(), qw, sizeof(float) * CC);
    memcpy(q.w.data() + CC, kw, sizeof(float) * CC);
    memcpy(q.w.data() + 2 * CC, vw, sizeof(float) * CC);
    memcpy(q.b.data(), qb, sizeof(float) * C);
    if (kb) memcpy(q.b.data() + C, kb, sizeof(float) * C);
    memcpy(q.b.data() + 2 * C, vb, sizeof(float) * C);
    return q;
}
// The q | k | v convolution's options: q and k stay K4P, the value third goes to `v` in attention's VT layout.  With ln_part the
// LayerNorm in front is folded in (pack_ln_fold's c1 / c2, the partials of the C input channels).
static DOpt qkv_opt(int C, float* v, const float2* ln_part = nullptr, const float* c1 = nullptr, const float* c2 = nullptr, float ln_eps = 1e-5f) {
    DOpt o;
    o.plain_from = 2 * C; o.out2 = v; o.vt_D = 64;
    if (ln_part) { o.ln_part = ln_part; o.ln_np = C / 32; o.ln_eps = ln_eps; o.ln_c1 = c1; o.ln_c2 = c2; }
    return o;
}

// The transformer's tensors of one call, T frames of C channels per clip: the LayerNorm partials of lnw channels, the residual stream's
// two, q | k, v (VT layout), attention's output and the feed-forward's hidden tensor (`big` floats per clip).  Returns a slot of `more`
// floats per clip behind them (an encoder's own last tensor); the tail slack ends the workspace.
struct TfWs {
    float2* lnp;
    float *xa, *xb, *qk, *v, *att, *big;
};
static float* plan_tf(Arena& A, size_t B, size_t C, size_t T, size_t big, size_t lnw, TfWs& w, size_t more = 0) {
    w.lnp = (float2*)A.f(B * (lnw / 32) * T * 2);
    w.xa = A.f(B * C * (T + 2)); w.xb = A.f(B * C * (T + 2));
    w.qk = A.f(B * 2 * C * (T + 2));
    w.v = A.f(B * (C * ((T + 3) & ~(size_t)3) + 2048));
    w.att = A.f(B * C * (T + 2));
    w.big = A.f(B * big);
    float* last = A.f(B * more);
    A.f(16384);      // tail slack: ragged last tiles read (masked) entries past a tensor's end
    return last;
}

// A pre-LN transformer block (Whisper's, wav2vec 2.0's): both LayerNorms folded into the GEMM that reads them.
struct PreLnBlockW {
    ConvW qkv, out, fc1, fc2;
    float *qkv_c1 = nullptr, *qkv_c2 = nullptr, *fc1_c1 = nullptr, *fc1_c2 = nullptr;
};
// the tensors of one block as the checkpoint holds them (weight, bias); kb may be null
struct PreLnBlockSrc {
    const float *ag, *ab, *qw, *qb, *kw, *kb, *vw, *vb, *ow, *ob, *mg, *mb, *f1, *f1b, *f2, *f2b;
};
static bool pack_preln_block(Owner& o, const PreLnBlockSrc& s, int C, int n_ffn, PreLnBlockW& bw) {
    if (!s.ag || !s.ab || !s.qw || !s.qb || !s.kw || !s.vw || !s.vb || !s.ow || !s.ob || !s.mg || !s.mb || !s.f1 || !s.f1b || !s.f2 || !s.f2b) return false;
    const QkvCat q = cat_qkv(s.qw, s.kw, s.vw, s.qb, s.kb, s.vb, C);
    return pack_ln_fold(o, q.w.data(), q.b.data(), s.ag, s.ab, 3 * C, C, {}, bw.qkv, bw.qkv_c1, bw.qkv_c2) && pack_conv(o, s.ow, s.ob, C, C, 1, bw.out) &&
           pack_ln_fold(o, s.f1, s.f1b, s.mg, s.mb, n_ffn, C, {}, bw.fc1, bw.fc1_c1, bw.fc1_c2) && pack_conv(o, s.f2, s.f2b, C, n_ffn, 1, bw.fc2);
}
// One block in five launches: x -> x (through xn).  w.lnp holds the partials of x on entry and on return; lvl: the ragged level of the
// frames under `lens` (k4p.h ragged_len; 1: Whisper, whose lens count mel frames; 0: lens are the clips' own frame counts).
static int run_preln_block(const PreLnBlockW& bw, float* x, float* xn, const TfWs& w, int C, int T, int n_ffn, int n_head, int lvl, const int* lens, int B,
                           hipStream_t st) {
    DOpt oq = qkv_opt(C, w.v, w.lnp, bw.qkv_c1, bw.qkv_c2);      // q | k | v of ln1(x)
    oq.lvl_in = oq.lvl_out = lvl;
    LDS_TRY(run_dconv(bw.qkv, x, C, nullptr, 0, T, oq, w.qk, B, st));
    HIP_TRY(launch_attention_k4p(w.qk, w.v, w.att, B, C, T, n_head, st, 0, lens, lvl));
    DOpt oo;      // x + out(.), partials for ln2
    oo.lvl_in = oo.lvl_out = lvl;
    oo.res = x; oo.lnpart_out = w.lnp;
    LDS_TRY(run_dconv(bw.out, w.att, C, nullptr, 0, T, oo, xn, B, st));
    DOpt o1;      // gelu(fc1(ln2(.)))
    o1.lvl_in = o1.lvl_out = lvl;
    o1.epi = EPI_GELU;
    o1.ln_part = w.lnp; o1.ln_np = C / 32; o1.ln_c1 = bw.fc1_c1; o1.ln_c2 = bw.fc1_c2;
    LDS_TRY(run_dconv(bw.fc1, xn, C, nullptr, 0, T, o1, w.big, B, st));
    DOpt o2;      // + fc2(.), partials for the next block's ln1 / the final LayerNorm
    o2.lvl_in = o2.lvl_out = lvl;
    o2.res = xn; o2.lnpart_out = w.lnp;
    return run_dconv(bw.fc2, w.big, n_ffn, nullptr, 0, T, o2, x, B, st);
}

// ---- the waveform convolution stack of HuBERT and wav2vec 2.0 ----
// what HuBERT and wav2vec 2.0 hold alike: the strided convolutions behind conv0, the feature projection and the positional convolution
struct ConvStackW {
    ConvW conv[6];                                                // conv1 .. conv6
    ConvW fproj;                                                  // the projection with the LayerNorm in front of it folded in
    float *fproj_c1 = nullptr, *fproj_c2 = nullptr;
    float *pos_w = nullptr, *pos_b = nullptr;                     // weight norm folded, packed for hubert_posconv
};
constexpr int kHubertLevels = 7;      // conv0 .. conv6
// frames after every layer of the feature extractor for a clip of n samples padded by `pad` zeros per side (model.py:99-106)
static void hubert_levels(int64_t n, int pad, int32_t* lv) {
    int64_t f = (n + 2 * pad - 10) / 5 + 1;
    lv[0] = (int32_t)f;
    for (int i = 1; i < kHubertLevels; ++i) {
        f = (i <= 4) ? (f - 3) / 2 + 1 : (f - 2) / 2 + 1;
        lv[i] = (int32_t)f;
    }
}

// The stack's part of a workspace: the clips' sample counts and their frame counts after conv0 .. conv6 on the device, and the two
// tensors the levels alternate between (conv0's output is the largest tensor of the call).  slen / nlen are what the launches take:
// null for a dense batch, the device copies once `upload` has run.
struct ConvStackWs {
    int* d_slen;
    int* d_nlen[kHubertLevels];
    float *ca, *cb;
    const int* slen = nullptr;
    const int* nlen[kHubertLevels] = {};
    void plan(Arena& A, size_t B, size_t D, const int32_t* nb) {
        d_slen = (int*)A.f(64);
        for (int i = 0; i < kHubertLevels; ++i) d_nlen[i] = (int*)A.f(64);
        ca = A.f(B * D * ((size_t)nb[0] + 2));
        cb = A.f(B * D * ((size_t)nb[1] + 2));
    }
    int upload(const int32_t* lens_host, int pad, int B, hipStream_t st) {
        int32_t lv[kHubertLevels][64];
        for (int b = 0; b < B; ++b) {
            int32_t one[kHubertLevels];
            hubert_levels(lens_host[b], pad, one);
            for (int i = 0; i < kHubertLevels; ++i) lv[i][b] = one[i];
        }
        LDS_TRY(upload_clip_ints(lens_host, B, d_slen, st));
        slen = d_slen;
        for (int i = 0; i < kHubertLevels; ++i) {
            LDS_TRY(upload_clip_ints(lv[i], B, d_nlen[i], st));
            nlen[i] = d_nlen[i];
        }
        return LDS_OK;
    }
};

// the dimension rules of HuBERT and wav2vec 2.0; n_proj < 0: the encoder has no proj
static int conv_stack_dims_check(const char* tag, int conv_dim, int n_state, int n_head, int n_layer, int n_ffn, int n_proj, int pos_kernel, int pos_groups,
                                 int n_ctx) {
    LDS_TRY(width_check(tag, "conv_dim", conv_dim, true));
    LDS_TRY(width_check(tag, "n_state", n_state, true));
    LDS_TRY(heads_check(tag, n_state, n_head));
    LDS_TRY(range_check(tag, "n_layer", n_layer, 1, 64));
    LDS_TRY(width_check(tag, "n_ffn", n_ffn, false));
    if (n_proj >= 0) LDS_TRY(width_check(tag, "n_proj", n_proj, false));
    if (pos_kernel < 2 || pos_kernel > 128 || (pos_kernel & 1)) return set_error(LDS_EINVAL, "%s: pos_kernel %d must be even in 2 .. 128", tag, pos_kernel);
    if (pos_groups < 1 || n_state % pos_groups || (n_state / pos_groups) % 16 || n_state / pos_groups > 64)
        return set_error(LDS_EINVAL, "%s: n_state / pos_groups must be 16, 32, 48 or 64 (got %d / %d)", tag, n_state, pos_groups);
    return range_check(tag, "n_ctx", n_ctx, 1, 1500);
}
// the limits of one call on audio: B clips in buffers of L samples, `pad` zeros (at most max_pad) added on each side of every clip;
// nb = the buffers' frame counts
static int conv_stack_shape_check(const char* tag, int n_ctx, int B, int64_t L, int pad, int max_pad, int32_t* nb) {
    LDS_TRY(range_check(tag, "B", B, 1, 65535));
    LDS_TRY(range_check(tag, "pad", pad, 0, max_pad));
    if (L + 2 * pad < 400 || L > ((int64_t)1 << 30)) return set_error(LDS_EINVAL, "%s: L %lld outside %d .. 2^30 samples", tag, (long long)L, 400 - 2 * pad);
    hubert_levels(L, pad, nb);
    if (nb[6] > n_ctx) return set_error(LDS_EINVAL, "%s: %d frames exceed n_ctx %d", tag, nb[6], n_ctx);
    return LDS_OK;
}

// ================================================================================================
// Whisper units encoder: log-mel front end + AudioEncoder (reference encoder/whisper/audio.py:62-82, model.py:112-131,
// tools/tools.py:105-126).  Channel-major K4P like the UNet's transformer, and built from the same launches: every LayerNorm is
// folded into the 1x1 convolution that reads it (pack_ln_fold), q | k | v is one convolution whose value third is stored in
// attention's VT layout, `out` and `mlp.2` add the residual and emit the next LayerNorm's partials.  Five launches per block.
// ================================================================================================
struct lds_whisper {
    lds_whisper_cfg cfg;
    Owner own;
    ConvW conv1, conv2;
    std::vector<PreLnBlockW> blocks;
    float *post_g = nullptr, *post_b = nullptr;
    float* posk = nullptr;        // the sinusoid table as one K4P element [n_state][n_ctx]
    double* basis = nullptr;      // [400][201] (cos, sin) times the periodic Hann window
    float* filtT = nullptr;       // [201][n_mels]
};

constexpr int kWhisperHop = 160, kWhisperNfft = 400, kWhisperBins = 201;

static int whisper_cfg_check(const lds_whisper_cfg* c) {
    if (!c) return set_error(LDS_EINVAL, "null argument");
    if (c->n_mels != 80 && c->n_mels != 128) return set_error(LDS_EINVAL, "whisper: n_mels %d (80 or 128)", c->n_mels);
    LDS_TRY(width_check("whisper", "n_state", c->n_state, false));
    LDS_TRY(heads_check("whisper", c->n_state, c->n_head));
    LDS_TRY(range_check("whisper", "n_layer", c->n_layer, 1, 64));
    LDS_TRY(range_check("whisper", "n_ctx", c->n_ctx, 1, 65536));
    return LDS_OK;
}

extern "C" int lds_whisper_create(const lds_whisper_cfg* cfg, int n, const char* const* names, const float* const* ptrs, const int64_t* numel,
                                  const float* mel_filters, lds_whisper** out) {
    if (!cfg || !names || !ptrs || !numel || !mel_filters || !out || n < 0) return set_error(LDS_EINVAL, "null argument");
    LDS_TRY(whisper_cfg_check(cfg));
    const int C = cfg->n_state, M = cfg->n_mels, NC = cfg->n_ctx;
    lds_whisper* h = new lds_whisper();
    h->cfg = *cfg;
    WeightLoader T(h->own, n, names, ptrs, numel);
    Owner& o = h->own;
    bool ok = true;
    {
        const float* w1 = T.get("encoder.conv1.weight", (int64_t)C * M * 3);
        const float* b1 = T.get("encoder.conv1.bias", C);
        const float* w2 = T.get("encoder.conv2.weight", (int64_t)C * C * 3);
        const float* b2 = T.get("encoder.conv2.bias", C);
        ok = w1 && b1 && w2 && b2 && pack_conv(o, w1, b1, C, M, 3, h->conv1) && pack_conv(o, w2, b2, C, C, 3, h->conv2);
    }
    h->blocks.resize(cfg->n_layer);
    for (int l = 0; l < cfg->n_layer && ok; ++l) {
        const std::string p = "encoder.blocks." + std::to_string(l) + ".";
        const int64_t CC = (int64_t)C * C;
        const PreLnBlockSrc s = {T.get(p + "attn_ln.weight", C),    T.get(p + "attn_ln.bias", C),
                                 T.get(p + "attn.query.weight", CC), T.get(p + "attn.query.bias", C),
                                 T.get(p + "attn.key.weight", CC),   nullptr,      // (no bias: model.py:47)
                                 T.get(p + "attn.value.weight", CC), T.get(p + "attn.value.bias", C),
                                 T.get(p + "attn.out.weight", CC),   T.get(p + "attn.out.bias", C),
                                 T.get(p + "mlp_ln.weight", C),      T.get(p + "mlp_ln.bias", C),
                                 T.get(p + "mlp.0.weight", 4 * CC),  T.get(p + "mlp.0.bias", 4 * C),
                                 T.get(p + "mlp.2.weight", 4 * CC),  T.get(p + "mlp.2.bias", C)};
        ok = pack_preln_block(o, s, C, 4 * C, h->blocks[l]);
    }
    if (ok) {
        h->post_g = T.vec("encoder.ln_post.weight", C);
        h->post_b = T.vec("encoder.ln_post.bias", C);
        ok = h->post_g && h->post_b;
    }
    if (ok) {
        // sinusoids(n_ctx, n_state) (model.py:35-40) with the reference's operation order in fp32: the increment is a double that torch
        // rounds to fp32 when it multiplies the integer range; the two products (increment x index, frame x inverse timescale) are fp32
        // products.  exp / sin / cos of those fp32 arguments are evaluated in double and rounded once, i.e. correctly rounded fp32
        // functions: an fp32 exp that is off by one ulp moves the table by 1500 ulp at frame 1500 (1e-4), and fp32 exp implementations
        // differ by that (torch's CPU exp is not correctly rounded for 6 of large-v3's 640 timescales), so the table is pinned to the
        // one definition that every platform reproduces (tests/whisper_numpy.py sinusoids is the same).
        const int half = C / 2;
        const float ninc = (float)(-(log(10000.0) / (double)(half - 1)));
        std::vector<float> inv(half), pk((size_t)C * (NC + 2), 0.f);
        for (int j = 0; j < half; ++j) inv[j] = (float)exp((double)(ninc * (float)j));
        for (int t = 0; t < NC; ++t)
            for (int j = 0; j < half; ++j) {
                const float st = (float)t * inv[j];
                pk[k4p_index(C, NC, 0, j, t)] = (float)sin((double)st);
                pk[k4p_index(C, NC, 0, half + j, t)] = (float)cos((double)st);
            }
        h->posk = o.upload(pk);
        // windowed DFT basis in double (logmel.hip): bin k of sample i of a frame; the angle is reduced exactly (k * i mod 400)
        std::vector<double> bs((size_t)kWhisperNfft * kWhisperBins * 2);
        const double two_pi = 6.283185307179586476925286766559;
        for (int i = 0; i < kWhisperNfft; ++i) {
            const double win = 0.5 - 0.5 * cos(two_pi * (double)i / kWhisperNfft);      // torch.hann_window(400): periodic
            for (int k = 0; k < kWhisperBins; ++k) {
                const double ang = two_pi * (double)((k * i) % kWhisperNfft) / kWhisperNfft;
                bs[((size_t)i * kWhisperBins + k) * 2] = win * cos(ang);
                bs[((size_t)i * kWhisperBins + k) * 2 + 1] = -win * sin(ang);
            }
        }
        h->basis = (double*)o.upload_bytes(bs.data(), bs.size() * sizeof(double));
        std::vector<float> ft((size_t)kWhisperBins * M);
        for (int m = 0; m < M; ++m)
            for (int k = 0; k < kWhisperBins; ++k) ft[(size_t)k * M + m] = mel_filters[(size_t)m * kWhisperBins + k];
        h->filtT = o.upload(ft);
        ok = h->posk && h->basis && h->filtT;
    }
    return T.finish(ok, "whisper", h, out);
}
extern "C" void lds_whisper_destroy(lds_whisper* h) { delete h; }

struct WhisperWs : TfWs {                  // big: conv1's output [C][F], later mlp.0's [4C][T]
    int *slen, *flen;                      // device copies of the clips' sample / mel-frame counts (<= 64 clips)
    float *logspec, *pmax, *melk;          // front end scratch; conv1's K4P input
};
// F = mel frames per clip buffer, T = (F - 1) / 2 + 1 encoder frames
static void plan_whisper(const lds_whisper* h, Arena& A, int B, int F, WhisperWs& w) {
    const size_t C = h->cfg.n_state, M = h->cfg.n_mels, T = (size_t)(F - 1) / 2 + 1, Bz = B;
    w.slen = (int*)A.f(64); w.flen = (int*)A.f(64);
    w.logspec = A.f(Bz * M * F);
    w.pmax = A.f(Bz * ((F + 15) / 16));
    w.melk = A.f(Bz * M * (F + 2));
    plan_tf(A, Bz, C, T, std::max(C * (F + 2), 4 * C * (T + 2)), C, w);
}
// the limits of one call: B clips in buffers of F mel frames
static int whisper_shape_check(const lds_whisper* h, int B, int64_t F) {
    if (!h) return set_error(LDS_EINVAL, "null handle");
    LDS_TRY(range_check("whisper", "B", B, 1, 65535));
    if (F < 1) return set_error(LDS_EINVAL, "whisper: no mel frame (a clip needs at least 400 samples)");
    if ((F - 1) / 2 + 1 > h->cfg.n_ctx) return set_error(LDS_EINVAL, "whisper: %lld frames exceed n_ctx %d", (long long)((F - 1) / 2 + 1), h->cfg.n_ctx);
    return LDS_OK;
}
extern "C" int lds_whisper_workspace_bytes(const lds_whisper* h, int B, int64_t L, size_t* out) {
    return plan_bytes(
        out,
        [&] {
            if (L < kWhisperNfft) return set_error(LDS_EINVAL, "whisper: L %lld below 400 samples", (long long)L);
            return whisper_shape_check(h, B, L / kWhisperHop);
        },
        [&](Arena& A) { WhisperWs w; plan_whisper(h, A, B, (int)(L / kWhisperHop), w); });
}

// audio -> (mel_plain and / or units); or mel_in (plain [B][n_mels][F]) -> units.  lens_host: samples per clip (audio) or mel frames per
// clip (mel_in); null = the buffer's length.  Every argument has been checked by the callers.
static int whisper_run(lds_whisper* h, const float* audio, int64_t L, const float* mel_in, int F, const int32_t* lens_host, float* mel_plain,
                       float* units, void* ws, size_t ws_bytes, int B, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    ProfChain chain;
    Arena A(ws, ws_bytes);
    WhisperWs w;
    plan_whisper(h, A, B, F, w);
    if (!A.ok) return set_error(LDS_ENOMEM, "whisper workspace too small: need %zu", A.used);
    const int C = h->cfg.n_state, M = h->cfg.n_mels, T = (F - 1) / 2 + 1;
    const int* slen = nullptr;
    const int* flen = nullptr;      // mel frames per clip: "level 0" of ragged_len; the encoder's frames are its level 1
    if (lens_host) {
        int32_t fl[64];
        for (int b = 0; b < B; ++b) fl[b] = audio ? lens_host[b] / kWhisperHop : lens_host[b];
        if (audio) { LDS_TRY(upload_clip_ints(lens_host, B, w.slen, st)); slen = w.slen; }
        LDS_TRY(upload_clip_ints(fl, B, w.flen, st));
        flen = w.flen;
    }
    if (audio) {
        if (mel_plain) HIP_TRY(launch_logmel(audio, slen, L, F, h->basis, h->filtT, M, w.logspec, w.pmax, mel_plain, 0, B, st));
        if (units) HIP_TRY(launch_logmel(audio, slen, L, F, h->basis, h->filtT, M, w.logspec, w.pmax, w.melk, 1, B, st));
    } else {
        HIP_TRY(launch_to_k4p(mel_in, w.melk, B, M, F, M, 0, st, flen));
    }
    if (!units) return LDS_OK;
    LensScope ls(flen);
    TileBatchScope tb(0);      // tile rules judged at the nominal batch (16 clips): a clip's units do not depend on the batch it is in
    {
        DOpt o;      // gelu(conv1(mel))
        o.pad = 1; o.epi = EPI_GELU; o.lvl_in = 0; o.lvl_out = 0;
        LDS_TRY(run_dconv(h->conv1, w.melk, M, nullptr, 0, F, o, w.big, B, st));
    }
    {
        DOpt o;      // gelu(conv2(.)), stride 2: F -> T frames, a clip's F_b -> (F_b - 1) / 2 + 1
        o.pad = 1; o.stride = 2; o.epi = EPI_GELU; o.lvl_in = 0; o.lvl_out = 1;
        LDS_TRY(run_dconv(h->conv2, w.big, C, nullptr, 0, F, o, w.xa, B, st));
    }
    HIP_TRY(launch_whisper_pos(w.xa, h->posk, h->cfg.n_ctx, w.lnp, flen, B, C, T, st));
    float* x = w.xa;
    float* xn = w.xb;
    for (const PreLnBlockW& bw : h->blocks) LDS_TRY(run_preln_block(bw, x, xn, w, C, T, 4 * C, h->cfg.n_head, 1, flen, B, st));
    HIP_TRY(launch_whisper_ln_post(x, w.lnp, h->post_g, h->post_b, 1e-5f, units, flen, B, C, T, st));
    return LDS_OK;
}

// argument checks shared by the audio entries; *F_out = mel frames of the buffers
static int whisper_audio_check(const lds_whisper* h, const float* audio, const int32_t* lengths, const void* ws, int B, int64_t L, int* F_out) {
    if (!h || !audio || !ws) return set_error(LDS_EINVAL, "null argument");
    if (L < kWhisperNfft || L > ((int64_t)1 << 30)) return set_error(LDS_EINVAL, "whisper: L %lld outside 400 .. 2^30 samples", (long long)L);
    LDS_TRY(whisper_shape_check(h, B, L / kWhisperHop));
    if (lengths) LDS_TRY(clip_lens_check("length", lengths, B, kWhisperNfft, L));
    *F_out = (int)(L / kWhisperHop);
    return LDS_OK;
}
extern "C" int lds_whisper_logmel(lds_whisper* h, const float* audio, const int32_t* lengths, float* mel, void* ws, size_t ws_bytes, int B, int64_t L,
                                  void* stream) {
    int F = 0;
    if (!mel) return set_error(LDS_EINVAL, "null argument");
    LDS_TRY(whisper_audio_check(h, audio, lengths, ws, B, L, &F));
    return whisper_run(h, audio, L, nullptr, F, lengths, mel, nullptr, ws, ws_bytes, B, stream);
}
extern "C" int lds_whisper_encode(lds_whisper* h, const float* audio, const int32_t* lengths, float* units, void* ws, size_t ws_bytes, int B, int64_t L,
                                  void* stream) {
    int F = 0;
    if (!units) return set_error(LDS_EINVAL, "null argument");
    LDS_TRY(whisper_audio_check(h, audio, lengths, ws, B, L, &F));
    return whisper_run(h, audio, L, nullptr, F, lengths, nullptr, units, ws, ws_bytes, B, stream);
}
extern "C" int lds_whisper_encode_mel(lds_whisper* h, const float* mel, const int32_t* n_frames, float* units, void* ws, size_t ws_bytes, int B, int F,
                                      void* stream) {
    if (!h || !mel || !units || !ws) return set_error(LDS_EINVAL, "null argument");
    LDS_TRY(whisper_shape_check(h, B, F));
    if (n_frames) LDS_TRY(clip_lens_check("n_frames", n_frames, B, 1, F));
    return whisper_run(h, nullptr, 0, mel, F, n_frames, nullptr, units, ws, ws_bytes, B, stream);
}

// ================================================================================================
// HuBERT units encoder (reference encoder/hubert/model.py:19-148: Hubert.encode / HubertSoft.units): a 7-layer waveform convolution
// stack, a LayerNorm + Linear projection, a grouped positional convolution and post-LayerNorm transformer blocks.  K4P throughout like the
// Whisper encoder above and built from the same launches; its own kernels are in hubert.hip.  Post-LN: a block's LayerNorm output is the
// next residual, so it is materialised (launch_hubert_ln) and the GEMMs read it with plain weights.  Seven launches per block.
// The frame counts do not follow ragged_len's halving rule (k 3 / k 2 convolutions without padding), so every level's per-clip counts
// are computed on the host and the launches of a level run with that level's array as their `lens` at level 0.
// ================================================================================================
struct HubertBlockW {
    ConvW qkv, out, fc1, fc2;
    float *n1_g = nullptr, *n1_b = nullptr, *n2_g = nullptr, *n2_b = nullptr;
};
struct lds_hubert : ConvStackW {
    lds_hubert_cfg cfg;
    Owner own;
    float *w0 = nullptr, *gn_g = nullptr, *gn_b = nullptr;      // conv0 [conv_dim][10], norm0
    float *norm_g = nullptr, *norm_b = nullptr;
    std::vector<HubertBlockW> blocks;
    ConvW proj;
};

static int hubert_cfg_check(const lds_hubert_cfg* c) {
    if (!c) return set_error(LDS_EINVAL, "null argument");
    return conv_stack_dims_check("hubert", c->conv_dim, c->n_state, c->n_head, c->n_layer, c->n_ffn, c->n_proj, c->pos_kernel, c->pos_groups, c->n_ctx);
}

// weight norm of the positional convolution folded in double (parametrizations.weight_norm(dim=2): one norm per tap, over the other two
// axes): w[:, :, k] = g[k] v[:, :, k] / |v[:, :, k]|; then the A-operand order of hubert_posconv: [group][k][ci / 4][row tile][lane]
static float* pack_posconv(Owner& o, const float* g, const float* v, int C, int groups, int K) {
    const int gw = C / groups, MT = gw / 16;
    std::vector<double> sc(K);
    for (int k = 0; k < K; ++k) {
        double s = 0;
        for (int64_t i = 0; i < (int64_t)C * gw; ++i) s += (double)v[i * K + k] * (double)v[i * K + k];
        sc[k] = (double)g[k] / sqrt(s);
    }
    std::vector<float> p((size_t)C * gw * K);
    for (int gi = 0; gi < groups; ++gi)
        for (int k = 0; k < K; ++k)
            for (int c4 = 0; c4 < gw / 4; ++c4)
                for (int m = 0; m < MT; ++m)
                    for (int l = 0; l < 64; ++l) {
                        const int co = gi * gw + m * 16 + (l & 15), ci = c4 * 4 + (l >> 4);
                        p[((((size_t)gi * K + k) * (gw / 4) + c4) * MT + m) * 64 + l] = (float)((double)v[((size_t)co * gw + ci) * K + k] * sc[k]);
                    }
    return o.upload(p);
}

extern "C" int lds_hubert_create(const lds_hubert_cfg* cfg, int n, const char* const* names, const float* const* ptrs, const int64_t* numel, lds_hubert** out) {
    if (!cfg || !names || !ptrs || !numel || !out || n < 0) return set_error(LDS_EINVAL, "null argument");
    LDS_TRY(hubert_cfg_check(cfg));
    const int D = cfg->conv_dim, C = cfg->n_state, F = cfg->n_ffn, K = cfg->pos_kernel, gw = C / cfg->pos_groups;
    lds_hubert* h = new lds_hubert();
    h->cfg = *cfg;
    WeightLoader T(h->own, n, names, ptrs, numel);
    Owner& o = h->own;
    h->w0 = T.vec("feature_extractor.conv0.weight", (int64_t)D * 10);
    h->gn_g = T.vec("feature_extractor.norm0.weight", D);
    h->gn_b = T.vec("feature_extractor.norm0.bias", D);
    bool ok = h->w0 && h->gn_g && h->gn_b;
    for (int i = 1; i <= 6 && ok; ++i) {
        const int k = i <= 4 ? 3 : 2;
        const float* w = T.get("feature_extractor.conv" + std::to_string(i) + ".weight", (int64_t)D * D * k);
        ok = w && pack_conv(o, w, nullptr, D, D, k, h->conv[i - 1]);
    }
    if (ok) {
        const float *g = T.get("feature_projection.norm.weight", D), *b = T.get("feature_projection.norm.bias", D);
        const float *w = T.get("feature_projection.projection.weight", (int64_t)C * D), *wb = T.get("feature_projection.projection.bias", C);
        ok = g && b && w && wb && pack_ln_fold(o, w, wb, g, b, C, D, {}, h->fproj, h->fproj_c1, h->fproj_c2);
    }
    if (ok) {
        const float* g = T.get("positional_embedding.conv.parametrizations.weight.original0", K);
        const float* v = T.get("positional_embedding.conv.parametrizations.weight.original1", (int64_t)C * gw * K);
        h->pos_b = T.vec("positional_embedding.conv.bias", C);
        if (g && v) h->pos_w = pack_posconv(o, g, v, C, cfg->pos_groups, K);
        h->norm_g = T.vec("norm.weight", C);
        h->norm_b = T.vec("norm.bias", C);
        ok = h->pos_w && h->pos_b && h->norm_g && h->norm_b;
    }
    h->blocks.resize(cfg->n_layer);
    for (int l = 0; l < cfg->n_layer && ok; ++l) {
        const std::string p = "encoder.layers." + std::to_string(l) + ".";
        HubertBlockW& bw = h->blocks[l];
        const int64_t CC = (int64_t)C * C;
        const float *iw = T.get(p + "self_attn.in_proj_weight", 3 * CC), *ib = T.get(p + "self_attn.in_proj_bias", 3 * C);
        const float *ow = T.get(p + "self_attn.out_proj.weight", CC), *ob = T.get(p + "self_attn.out_proj.bias", C);
        const float *f1 = T.get(p + "linear1.weight", (int64_t)F * C), *f1b = T.get(p + "linear1.bias", F);
        const float *f2 = T.get(p + "linear2.weight", (int64_t)F * C), *f2b = T.get(p + "linear2.bias", C);
        if (!iw || !ib || !ow || !ob || !f1 || !f1b || !f2 || !f2b) { ok = false; break; }
        bw.n1_g = T.vec(p + "norm1.weight", C); bw.n1_b = T.vec(p + "norm1.bias", C);
        bw.n2_g = T.vec(p + "norm2.weight", C); bw.n2_b = T.vec(p + "norm2.bias", C);
        ok = bw.n1_g && bw.n1_b && bw.n2_g && bw.n2_b && pack_conv(o, iw, ib, 3 * C, C, 1, bw.qkv) && pack_conv(o, ow, ob, C, C, 1, bw.out) &&
             pack_conv(o, f1, f1b, F, C, 1, bw.fc1) && pack_conv(o, f2, f2b, C, F, 1, bw.fc2);
    }
    if (ok) {
        const float *w = T.get("proj.weight", (int64_t)cfg->n_proj * C), *b = T.get("proj.bias", cfg->n_proj);
        ok = w && b && pack_conv(o, w, b, cfg->n_proj, C, 1, h->proj);
    }
    return T.finish(ok, "hubert", h, out);
}
extern "C" void lds_hubert_destroy(lds_hubert* h) { delete h; }

struct HubertWs : ConvStackWs, TfWs {      // lnp: conv6's LayerNorm partials for the folded feature projection
    float2 *part, *stat;                   // norm0's statistics
    float* pj;
};
static void plan_hubert(const lds_hubert* h, Arena& A, int B, const int32_t* nb, HubertWs& w) {
    const size_t D = h->cfg.conv_dim, C = h->cfg.n_state, F = h->cfg.n_ffn, P = h->cfg.n_proj, T = nb[6], Bz = B;
    w.plan(A, Bz, D, nb);
    w.part = (float2*)A.f(Bz * (((size_t)nb[0] + 255) / 256) * D * 2);
    w.stat = (float2*)A.f(Bz * D * 2);
    w.pj = plan_tf(A, Bz, C, T, F * (T + 2), D, w, P * (T + 2));
}
static int hubert_shape_check(const lds_hubert* h, int B, int64_t L, int pad, int32_t* nb) {
    if (!h) return set_error(LDS_EINVAL, "null handle");
    return conv_stack_shape_check("hubert", h->cfg.n_ctx, B, L, pad, 40, nb);
}
extern "C" int lds_hubert_workspace_bytes(const lds_hubert* h, int B, int64_t L, int pad, size_t* out) {
    int32_t nb[kHubertLevels];
    return plan_bytes(out, [&] { return hubert_shape_check(h, B, L, pad, nb); }, [&](Arena& A) { HubertWs w; plan_hubert(h, A, B, nb, w); });
}

// audio -> feat ([B][T][conv_dim]) and / or enc ([B][T][n_state], or [B][T][n_proj] with want_proj).  Every argument has been checked.
static int hubert_run(lds_hubert* h, const float* audio, int64_t L, int pad, const int32_t* lens_host, const int32_t* nb, float* feat, float* enc,
                      int n_layers_run, int want_proj, void* ws, size_t ws_bytes, int B, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    ProfChain chain;
    Arena A(ws, ws_bytes);
    HubertWs w;
    plan_hubert(h, A, B, nb, w);
    if (!A.ok) return set_error(LDS_ENOMEM, "hubert workspace too small: need %zu", A.used);
    const int D = h->cfg.conv_dim, C = h->cfg.n_state, T = nb[6];
    if (lens_host) LDS_TRY(w.upload(lens_host, pad, B, st));
    TileBatchScope tb(0);      // tile rules judged at the nominal batch: a clip's units do not depend on the batch it is in
    HIP_TRY(launch_hubert_conv0(audio, w.slen, L, pad, h->w0, h->gn_g, h->gn_b, 1e-5f, w.nlen[0], nb[0], D, w.part, w.stat, w.ca, B, st));
    float* x = w.ca;
    float* xn = w.cb;
    for (int i = 1; i < kHubertLevels; ++i) {      // gelu(conv_i(.)): stride 2, no padding; frames beyond a clip's count at level i are zeros
        LensScope ls(w.nlen[i]);
        DOpt o;
        o.stride = 2; o.pad = 0; o.epi = EPI_GELU;
        if (i == kHubertLevels - 1) o.lnpart_out = w.lnp;      // partials for feature_projection.norm
        LDS_TRY(run_dconv(h->conv[i - 1], x, D, nullptr, 0, nb[i - 1], o, xn, B, st));
        { float* t = x; x = xn; xn = t; }
    }
    const int* flen = w.nlen[kHubertLevels - 1];
    if (feat) HIP_TRY(launch_hubert_store_frames(x, feat, flen, B, D, T, st));
    if (!enc) return LDS_OK;
    LensScope ls(flen);
    {
        DOpt o;      // projection(norm(.))
        o.ln_part = w.lnp; o.ln_np = D / 32; o.ln_c1 = h->fproj_c1; o.ln_c2 = h->fproj_c2;
        LDS_TRY(run_dconv(h->fproj, x, D, nullptr, 0, T, o, w.xa, B, st));
    }
    HIP_TRY(launch_hubert_posconv(w.xa, h->pos_w, h->pos_b, w.xb, flen, B, C, T, h->cfg.pos_kernel, h->cfg.pos_groups, st));
    HIP_TRY(launch_hubert_ln(w.xb, h->norm_g, h->norm_b, 1e-5f, w.xa, flen, B, C, T, st));
    for (int l = 0; l < n_layers_run; ++l) {
        const HubertBlockW& bw = h->blocks[l];
        const DOpt oq = qkv_opt(C, w.v);      // q | k | v
        LDS_TRY(run_dconv(bw.qkv, w.xa, C, nullptr, 0, T, oq, w.qk, B, st));
        HIP_TRY(launch_attention_k4p(w.qk, w.v, w.att, B, C, T, h->cfg.n_head, st, 0, flen, 0));
        DOpt oo;      // x + out_proj(.), then norm1
        oo.res = w.xa;
        LDS_TRY(run_dconv(bw.out, w.att, C, nullptr, 0, T, oo, w.xb, B, st));
        HIP_TRY(launch_hubert_ln(w.xb, bw.n1_g, bw.n1_b, 1e-5f, w.xa, flen, B, C, T, st));
        DOpt o1;      // gelu(linear1(.))
        o1.epi = EPI_GELU;
        LDS_TRY(run_dconv(bw.fc1, w.xa, C, nullptr, 0, T, o1, w.big, B, st));
        DOpt o2;      // + linear2(.), then norm2
        o2.res = w.xa;
        LDS_TRY(run_dconv(bw.fc2, w.big, h->cfg.n_ffn, nullptr, 0, T, o2, w.xb, B, st));
        HIP_TRY(launch_hubert_ln(w.xb, bw.n2_g, bw.n2_b, 1e-5f, w.xa, flen, B, C, T, st));
    }
    if (want_proj) {
        DOpt o;
        LDS_TRY(run_dconv(h->proj, w.xa, C, nullptr, 0, T, o, w.pj, B, st));
        HIP_TRY(launch_hubert_store_frames(w.pj, enc, flen, B, h->cfg.n_proj, T, st));
    } else {
        HIP_TRY(launch_hubert_store_frames(w.xa, enc, flen, B, C, T, st));
    }
    return LDS_OK;
}

static int hubert_audio_check(const lds_hubert* h, const float* audio, const int32_t* lengths, const void* out, const void* ws, int B, int64_t L, int pad,
                              int32_t* nb) {
    if (!h || !audio || !out || !ws) return set_error(LDS_EINVAL, "null argument");
    LDS_TRY(hubert_shape_check(h, B, L, pad, nb));
    if (lengths) LDS_TRY(clip_lens_check("length", lengths, B, 400 - 2 * pad, L));
    return LDS_OK;
}
extern "C" int lds_hubert_features(lds_hubert* h, const float* audio, const int32_t* lengths, float* out, void* ws, size_t ws_bytes, int B, int64_t L, int pad,
                                   void* stream) {
    int32_t nb[kHubertLevels];
    LDS_TRY(hubert_audio_check(h, audio, lengths, out, ws, B, L, pad, nb));
    return hubert_run(h, audio, L, pad, lengths, nb, out, nullptr, 0, 0, ws, ws_bytes, B, stream);
}
extern "C" int lds_hubert_encode(lds_hubert* h, const float* audio, const int32_t* lengths, float* out, int n_layers_run, int want_proj, void* ws,
                                 size_t ws_bytes, int B, int64_t L, int pad, void* stream) {
    int32_t nb[kHubertLevels];
    LDS_TRY(hubert_audio_check(h, audio, lengths, out, ws, B, L, pad, nb));
    if (n_layers_run < 0 || n_layers_run > h->cfg.n_layer) return set_error(LDS_EINVAL, "hubert: n_layers_run %d outside 0 .. %d", n_layers_run, h->cfg.n_layer);
    if (want_proj && n_layers_run != h->cfg.n_layer) return set_error(LDS_EINVAL, "hubert: proj follows the last layer (n_layers_run %d of %d)", n_layers_run, h->cfg.n_layer);
    return hubert_run(h, audio, L, pad, lengths, nb, nullptr, out, n_layers_run, want_proj, ws, ws_bytes, B, stream);
}

// ================================================================================================
// wav2vec 2.0 units encoder in its layer-norm flavour (XLSR-53; reference tools/tools.py Audio2xlsr_53_56k: fairseq's
// extract_features(source, padding_mask = all False)["x"]).  HuBERT's convolution strides and frame rule (no padding of the clip), but
// every convolution has a bias and a LayerNorm over the channels of each frame in front of its GELU (w2v.hip), the positional convolution
// is followed by no LayerNorm, and the blocks are pre-LN: Whisper's five launches with every LayerNorm folded into the GEMM that reads it,
// then `encoder.layer_norm` through whisper_ln_post.  Tensor names are fairseq's (what pretrain/xlsr_53_56k.pt holds).
// ================================================================================================
struct lds_w2v : ConvStackW {                                      // (conv1 .. conv6 are biased here)
    lds_w2v_cfg cfg;
    Owner own;
    float *w0 = nullptr, *b0 = nullptr;                            // conv0 [conv_dim][10] and its bias
    float *ln_g[kHubertLevels] = {}, *ln_b[kHubertLevels] = {};    // the LayerNorm behind conv0 .. conv6
    std::vector<PreLnBlockW> blocks;
    float *post_g = nullptr, *post_b = nullptr;                    // encoder.layer_norm
};

static int w2v_cfg_check(const lds_w2v_cfg* c) {
    if (!c) return set_error(LDS_EINVAL, "null argument");
    return conv_stack_dims_check("w2v", c->conv_dim, c->n_state, c->n_head, c->n_layer, c->n_ffn, -1, c->pos_kernel, c->pos_groups, c->n_ctx);
}

extern "C" int lds_w2v_create(const lds_w2v_cfg* cfg, int n, const char* const* names, const float* const* ptrs, const int64_t* numel, lds_w2v** out) {
    if (!cfg || !names || !ptrs || !numel || !out || n < 0) return set_error(LDS_EINVAL, "null argument");
    LDS_TRY(w2v_cfg_check(cfg));
    const int D = cfg->conv_dim, C = cfg->n_state, F = cfg->n_ffn, K = cfg->pos_kernel, gw = C / cfg->pos_groups;
    lds_w2v* h = new lds_w2v();
    h->cfg = *cfg;
    WeightLoader T(h->own, n, names, ptrs, numel);
    Owner& o = h->own;
    bool ok = true;
    for (int i = 0; i < kHubertLevels && ok; ++i) {
        const std::string p = "feature_extractor.conv_layers." + std::to_string(i) + ".";
        h->ln_g[i] = T.vec(p + "2.1.weight", D);
        h->ln_b[i] = T.vec(p + "2.1.bias", D);
        ok = h->ln_g[i] && h->ln_b[i];
        if (!ok) break;
        if (i == 0) {
            h->w0 = T.vec(p + "0.weight", (int64_t)D * 10);
            h->b0 = T.vec(p + "0.bias", D);
            ok = h->w0 && h->b0;
        } else {
            const int k = i <= 4 ? 3 : 2;
            const float *w = T.get(p + "0.weight", (int64_t)D * D * k), *b = T.get(p + "0.bias", D);
            ok = w && b && pack_conv(o, w, b, D, D, k, h->conv[i - 1]);
        }
    }
    if (ok) {
        const float *g = T.get("layer_norm.weight", D), *b = T.get("layer_norm.bias", D);
        const float *w = T.get("post_extract_proj.weight", (int64_t)C * D), *wb = T.get("post_extract_proj.bias", C);
        ok = g && b && w && wb && pack_ln_fold(o, w, wb, g, b, C, D, {}, h->fproj, h->fproj_c1, h->fproj_c2);
    }
    if (ok) {
        const float* g = T.get("encoder.pos_conv.0.weight_g", K);
        const float* v = T.get("encoder.pos_conv.0.weight_v", (int64_t)C * gw * K);
        h->pos_b = T.vec("encoder.pos_conv.0.bias", C);
        if (g && v) h->pos_w = pack_posconv(o, g, v, C, cfg->pos_groups, K);
        ok = h->pos_w && h->pos_b;
    }
    h->blocks.resize(cfg->n_layer);
    for (int l = 0; l < cfg->n_layer && ok; ++l) {
        const std::string p = "encoder.layers." + std::to_string(l) + ".";
        const int64_t CC = (int64_t)C * C, FC = (int64_t)F * C;
        const PreLnBlockSrc s = {T.get(p + "self_attn_layer_norm.weight", C), T.get(p + "self_attn_layer_norm.bias", C),
                                 T.get(p + "self_attn.q_proj.weight", CC),    T.get(p + "self_attn.q_proj.bias", C),
                                 T.get(p + "self_attn.k_proj.weight", CC),    T.get(p + "self_attn.k_proj.bias", C),
                                 T.get(p + "self_attn.v_proj.weight", CC),    T.get(p + "self_attn.v_proj.bias", C),
                                 T.get(p + "self_attn.out_proj.weight", CC),  T.get(p + "self_attn.out_proj.bias", C),
                                 T.get(p + "final_layer_norm.weight", C),     T.get(p + "final_layer_norm.bias", C),
                                 T.get(p + "fc1.weight", FC),                 T.get(p + "fc1.bias", F),
                                 T.get(p + "fc2.weight", FC),                 T.get(p + "fc2.bias", C)};
        ok = s.kb && pack_preln_block(o, s, C, F, h->blocks[l]);
    }
    if (ok) {
        h->post_g = T.vec("encoder.layer_norm.weight", C);
        h->post_b = T.vec("encoder.layer_norm.bias", C);
        ok = h->post_g && h->post_b;
    }
    return T.finish(ok, "w2v", h, out);
}
extern "C" void lds_w2v_destroy(lds_w2v* h) { delete h; }

// ca / cb: a level's LayerNorm output / its raw convolution; lnp: LayerNorm partials of the extractor's output, then of the residual stream
struct W2vWs : ConvStackWs, TfWs {};
static void plan_w2v(const lds_w2v* h, Arena& A, int B, const int32_t* nb, W2vWs& w) {
    const size_t D = h->cfg.conv_dim, C = h->cfg.n_state, F = h->cfg.n_ffn, T = nb[6], Bz = B;
    w.plan(A, Bz, D, nb);
    plan_tf(A, Bz, C, T, F * (T + 2), std::max(D, C), w);
}
static int w2v_shape_check(const lds_w2v* h, int B, int64_t L, int32_t* nb) {
    if (!h) return set_error(LDS_EINVAL, "null handle");
    return conv_stack_shape_check("w2v", h->cfg.n_ctx, B, L, 0, 0, nb);
}
extern "C" int lds_w2v_workspace_bytes(const lds_w2v* h, int B, int64_t L, size_t* out) {
    int32_t nb[kHubertLevels];
    return plan_bytes(out, [&] { return w2v_shape_check(h, B, L, nb); }, [&](Arena& A) { W2vWs w; plan_w2v(h, A, B, nb, w); });
}

// audio -> feat ([B][T][conv_dim]) or enc ([B][T][n_state]).  Every argument has been checked.
static int w2v_run(lds_w2v* h, const float* audio, int64_t L, const int32_t* lens_host, const int32_t* nb, float* feat, float* enc, void* ws, size_t ws_bytes,
                   int B, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    ProfChain chain;
    Arena A(ws, ws_bytes);
    W2vWs w;
    plan_w2v(h, A, B, nb, w);
    if (!A.ok) return set_error(LDS_ENOMEM, "w2v workspace too small: need %zu", A.used);
    const int D = h->cfg.conv_dim, C = h->cfg.n_state, T = nb[6];
    if (lens_host) LDS_TRY(w.upload(lens_host, 0, B, st));
    TileBatchScope tb(0);      // tile rules judged at the nominal batch: a clip's units do not depend on the batch it is in
    HIP_TRY(launch_w2v_conv0(audio, w.slen, L, h->w0, h->b0, h->ln_g[0], h->ln_b[0], 1e-5f, w.nlen[0], nb[0], D, w.ca, B, st));
    for (int i = 1; i < kHubertLevels; ++i) {      // conv_i + bias (stride 2, no padding) into cb, GELU(LayerNorm(.)) back into ca
        LensScope ls(w.nlen[i]);
        DOpt o;
        o.stride = 2; o.pad = 0;
        LDS_TRY(run_dconv(h->conv[i - 1], w.ca, D, nullptr, 0, nb[i - 1], o, w.cb, B, st));
        // the last level's partials serve the feature projection's folded layer_norm
        HIP_TRY(launch_w2v_ln_act(w.cb, h->ln_g[i], h->ln_b[i], 1e-5f, w.ca, (i == kHubertLevels - 1 && enc) ? w.lnp : nullptr, w.nlen[i], B, D, nb[i], st));
    }
    const int* flen = w.nlen[kHubertLevels - 1];
    if (feat) HIP_TRY(launch_hubert_store_frames(w.ca, feat, flen, B, D, T, st));
    if (!enc) return LDS_OK;
    LensScope ls(flen);
    {
        DOpt o;      // post_extract_proj(layer_norm(.))
        o.ln_part = w.lnp; o.ln_np = D / 32; o.ln_c1 = h->fproj_c1; o.ln_c2 = h->fproj_c2;
        LDS_TRY(run_dconv(h->fproj, w.ca, D, nullptr, 0, T, o, w.xa, B, st));
    }
    HIP_TRY(launch_hubert_posconv(w.xa, h->pos_w, h->pos_b, w.xb, flen, B, C, T, h->cfg.pos_kernel, h->cfg.pos_groups, st));
    HIP_TRY(launch_w2v_lnpart(w.xb, w.lnp, flen, B, C, T, st));      // partials for the first block's self_attn_layer_norm
    float* x = w.xb;
    float* xn = w.xa;
    for (const PreLnBlockW& bw : h->blocks) LDS_TRY(run_preln_block(bw, x, xn, w, C, T, h->cfg.n_ffn, h->cfg.n_head, 0, flen, B, st));
    HIP_TRY(launch_whisper_ln_post(x, w.lnp, h->post_g, h->post_b, 1e-5f, enc, flen, B, C, T, st, 0));
    return LDS_OK;
}

static int w2v_audio_check(const lds_w2v* h, const float* audio, const int32_t* lengths, const void* out, const void* ws, int B, int64_t L, int32_t* nb) {
    if (!h || !audio || !out || !ws) return set_error(LDS_EINVAL, "null argument");
    LDS_TRY(w2v_shape_check(h, B, L, nb));
    if (lengths) LDS_TRY(clip_lens_check("length", lengths, B, 400, L));
    return LDS_OK;
}
extern "C" int lds_w2v_features(lds_w2v* h, const float* audio, const int32_t* lengths, float* out, void* ws, size_t ws_bytes, int B, int64_t L, void* stream) {
    int32_t nb[kHubertLevels];
    LDS_TRY(w2v_audio_check(h, audio, lengths, out, ws, B, L, nb));
    return w2v_run(h, audio, L, lengths, nb, out, nullptr, ws, ws_bytes, B, stream);
}
extern "C" int lds_w2v_encode(lds_w2v* h, const float* audio, const int32_t* lengths, float* out, void* ws, size_t ws_bytes, int B, int64_t L, void* stream) {
    int32_t nb[kHubertLevels];
    LDS_TRY(w2v_audio_check(h, audio, lengths, out, ws, B, L, nb));
    return w2v_run(h, audio, L, lengths, nb, nullptr, out, ws, ws_bytes, B, stream);
}

// ================================================================================================
// WavLM units encoder (transformers' WavLMModel; so-vits-svc's wavlmbase+, kNN-VC's WavLM-Large).  Two flavours of one network:
//   stable_layer_norm 0 (Base / Base+): HuBERT's skeleton above with pad 0 -- bias-free convolutions, a GroupNorm behind conv0, post-LN blocks;
//   stable_layer_norm 1 (Large): wav2vec 2.0's skeleton above with zero convolution biases -- a LayerNorm behind every convolution, pre-LN
//   blocks, a final encoder.layer_norm.
// What neither has: every block's self-attention adds gate[h][i] * bias[h][j - i] to its scores.  The bias is layer 0's rel_attn_embed
// looked up at the bucket of j - i, a Toeplitz table [heads][2 n_ctx - 1] built once at create; the gate [B][heads][T] comes from the
// block's attention input in one small launch (wavlm.hip) that runs beside the q | k | v convolution's, and attention_k4p_bias applies both.
// In the stable flavour the attention's LayerNorm is therefore materialised (launch_hubert_ln: the gate reads it too) instead of folded
// into the q | k | v convolution; the feed-forward's stays folded.  Tensor names are WavLMModel.state_dict()'s.
// ================================================================================================
struct WavlmBlockW {
    ConvW qkv, out, fc1, fc2;
    float *n1_g = nullptr, *n1_b = nullptr, *n2_g = nullptr, *n2_b = nullptr;      // layer_norm, final_layer_norm (n2: post-LN flavour only)
    float *fc1_c1 = nullptr, *fc1_c2 = nullptr;                                    // stable flavour: final_layer_norm folded into fc1
    float *gate_w = nullptr, *gate_b = nullptr, *gate_c = nullptr;                 // gru_rel_pos_linear [8][64], [8]; gru_rel_pos_const [heads]
};
struct lds_wavlm : ConvStackW {
    lds_wavlm_cfg cfg;
    Owner own;
    float *w0 = nullptr, *b0 = nullptr;                            // conv0 [conv_dim][10]; zeros (the stable flavour's conv0 kernel takes a bias)
    float *ln_g[kHubertLevels] = {}, *ln_b[kHubertLevels] = {};    // the norm behind conv0 (both flavours) .. conv6 (stable flavour)
    float *norm_g = nullptr, *norm_b = nullptr;                    // encoder.layer_norm
    float* toep = nullptr;                                         // [n_head][2 n_ctx - 1]
    std::vector<WavlmBlockW> blocks;
};

// WavLMAttention._relative_positions_bucket for one distance d = key - query, its large branch in float32 as torch runs it
static int wavlm_bucket(int d, int num_buckets, int max_distance) {
    const int nb = num_buckets / 2, me = nb / 2, a = d < 0 ? -d : d;
    int v = a;
    if (a >= me) {
        float x = logf((float)a / (float)me);
        x = x / (float)log((double)max_distance / (double)me);
        x = x * (float)(nb - me);
        const long long big = (long long)((float)me + x);
        v = big < nb - 1 ? (int)big : nb - 1;
    }
    return (d > 0 ? nb : 0) + v;
}
static int wavlm_bucket_check(int num_buckets, int max_distance) {
    if (num_buckets < 4 || num_buckets % 4 || num_buckets > 4096) return set_error(LDS_EINVAL, "wavlm: num_buckets %d must be a multiple of 4 in 4 .. 4096", num_buckets);
    if (max_distance <= num_buckets / 4 || max_distance > (1 << 20))
        return set_error(LDS_EINVAL, "wavlm: max_distance %d outside num_buckets / 4 + 1 = %d .. 2^20", max_distance, num_buckets / 4 + 1);
    return LDS_OK;
}
static int wavlm_cfg_check(const lds_wavlm_cfg* c) {
    if (!c) return set_error(LDS_EINVAL, "null argument");
    LDS_TRY(conv_stack_dims_check("wavlm", c->conv_dim, c->n_state, c->n_head, c->n_layer, c->n_ffn, -1, c->pos_kernel, c->pos_groups, c->n_ctx));
    LDS_TRY(wavlm_bucket_check(c->num_buckets, c->max_distance));
    if (c->stable_layer_norm != 0 && c->stable_layer_norm != 1) return set_error(LDS_EINVAL, "wavlm: stable_layer_norm %d (0 or 1)", c->stable_layer_norm);
    return LDS_OK;
}

extern "C" int lds_wavlm_create(const lds_wavlm_cfg* cfg, int n, const char* const* names, const float* const* ptrs, const int64_t* numel, lds_wavlm** out) {
    if (!cfg || !names || !ptrs || !numel || !out || n < 0) return set_error(LDS_EINVAL, "null argument");
    LDS_TRY(wavlm_cfg_check(cfg));
    const int D = cfg->conv_dim, C = cfg->n_state, F = cfg->n_ffn, K = cfg->pos_kernel, gw = C / cfg->pos_groups, H = cfg->n_head;
    const bool stable = cfg->stable_layer_norm != 0;
    lds_wavlm* h = new lds_wavlm();
    h->cfg = *cfg;
    WeightLoader T(h->own, n, names, ptrs, numel);
    Owner& o = h->own;
    bool ok = true;
    for (int i = 0; i < kHubertLevels && ok; ++i) {
        const std::string p = "feature_extractor.conv_layers." + std::to_string(i) + ".";
        if (i == 0 || stable) {      // GroupNorm(C, C) behind conv0 (Base) / a LayerNorm behind every convolution (Large)
            h->ln_g[i] = T.vec(p + "layer_norm.weight", D);
            h->ln_b[i] = T.vec(p + "layer_norm.bias", D);
            ok = h->ln_g[i] && h->ln_b[i];
            if (!ok) break;
        }
        if (i == 0) {
            h->w0 = T.vec(p + "conv.weight", (int64_t)D * 10);
            h->b0 = o.upload(std::vector<float>(D, 0.f));
            ok = h->w0 && h->b0;
        } else {
            const int k = i <= 4 ? 3 : 2;
            const float* w = T.get(p + "conv.weight", (int64_t)D * D * k);
            ok = w && pack_conv(o, w, nullptr, D, D, k, h->conv[i - 1]);
        }
    }
    if (ok) {
        const float *g = T.get("feature_projection.layer_norm.weight", D), *b = T.get("feature_projection.layer_norm.bias", D);
        const float *w = T.get("feature_projection.projection.weight", (int64_t)C * D), *wb = T.get("feature_projection.projection.bias", C);
        ok = g && b && w && wb && pack_ln_fold(o, w, wb, g, b, C, D, {}, h->fproj, h->fproj_c1, h->fproj_c2);
    }
    if (ok) {
        const float* g = T.get("encoder.pos_conv_embed.conv.parametrizations.weight.original0", K);
        const float* v = T.get("encoder.pos_conv_embed.conv.parametrizations.weight.original1", (int64_t)C * gw * K);
        h->pos_b = T.vec("encoder.pos_conv_embed.conv.bias", C);
        if (g && v) h->pos_w = pack_posconv(o, g, v, C, cfg->pos_groups, K);
        h->norm_g = T.vec("encoder.layer_norm.weight", C);
        h->norm_b = T.vec("encoder.layer_norm.bias", C);
        ok = h->pos_w && h->pos_b && h->norm_g && h->norm_b;
    }
    if (ok) {      // the bias of every layer: layer 0's embedding at the bucket of every distance
        const int NB = cfg->num_buckets, W = 2 * cfg->n_ctx - 1;
        const float* e = T.get("encoder.layers.0.attention.rel_attn_embed.weight", (int64_t)NB * H);
        if (e) {
            std::vector<float> tp((size_t)H * W);
            for (int d = -(cfg->n_ctx - 1); d < cfg->n_ctx; ++d) {
                const int bk = wavlm_bucket(d, NB, cfg->max_distance);
                for (int hd = 0; hd < H; ++hd) tp[(size_t)hd * W + d + cfg->n_ctx - 1] = e[(size_t)bk * H + hd];
            }
            h->toep = o.upload(tp);
        }
        ok = h->toep != nullptr;
    }
    h->blocks.resize(cfg->n_layer);
    for (int l = 0; l < cfg->n_layer && ok; ++l) {
        const std::string p = "encoder.layers." + std::to_string(l) + ".";
        WavlmBlockW& bw = h->blocks[l];
        const int64_t CC = (int64_t)C * C, FC = (int64_t)F * C;
        const float *qw = T.get(p + "attention.q_proj.weight", CC), *qb = T.get(p + "attention.q_proj.bias", C);
        const float *kw = T.get(p + "attention.k_proj.weight", CC), *kb = T.get(p + "attention.k_proj.bias", C);
        const float *vw = T.get(p + "attention.v_proj.weight", CC), *vb = T.get(p + "attention.v_proj.bias", C);
        const float *ow = T.get(p + "attention.out_proj.weight", CC), *ob = T.get(p + "attention.out_proj.bias", C);
        const float *g2 = T.get(p + "final_layer_norm.weight", C), *b2 = T.get(p + "final_layer_norm.bias", C);
        const float *f1 = T.get(p + "feed_forward.intermediate_dense.weight", FC), *f1b = T.get(p + "feed_forward.intermediate_dense.bias", F);
        const float *f2 = T.get(p + "feed_forward.output_dense.weight", FC), *f2b = T.get(p + "feed_forward.output_dense.bias", C);
        if (!qw || !qb || !kw || !kb || !vw || !vb || !ow || !ob || !g2 || !b2 || !f1 || !f1b || !f2 || !f2b) { ok = false; break; }
        bw.n1_g = T.vec(p + "layer_norm.weight", C); bw.n1_b = T.vec(p + "layer_norm.bias", C);
        bw.gate_w = T.vec(p + "attention.gru_rel_pos_linear.weight", 8 * 64);
        bw.gate_b = T.vec(p + "attention.gru_rel_pos_linear.bias", 8);
        bw.gate_c = T.vec(p + "attention.gru_rel_pos_const", H);
        const QkvCat q = cat_qkv(qw, kw, vw, qb, kb, vb, C);
        ok = bw.n1_g && bw.n1_b && bw.gate_w && bw.gate_b && bw.gate_c && pack_conv(o, q.w.data(), q.b.data(), 3 * C, C, 1, bw.qkv) &&
             pack_conv(o, ow, ob, C, C, 1, bw.out) && pack_conv(o, f2, f2b, C, F, 1, bw.fc2);
        if (!ok) break;
        if (stable) {
            ok = pack_ln_fold(o, f1, f1b, g2, b2, F, C, {}, bw.fc1, bw.fc1_c1, bw.fc1_c2);
        } else {
            bw.n2_g = o.upload(std::vector<float>(g2, g2 + C)); bw.n2_b = o.upload(std::vector<float>(b2, b2 + C));
            ok = bw.n2_g && bw.n2_b && pack_conv(o, f1, f1b, F, C, 1, bw.fc1);
        }
    }
    return T.finish(ok, "wavlm", h, out);
}
extern "C" void lds_wavlm_destroy(lds_wavlm* h) { delete h; }

struct WavlmWs : ConvStackWs, TfWs {
    float2 *part, *stat;      // Base: norm0's statistics
    double2* wstat;           // the clips' waveform statistics
    float *wave, *gate;       // the normalised waveform [B][L]; the block's gate [B][n_head][T]
};
static void plan_wavlm(const lds_wavlm* h, Arena& A, int B, int64_t L, const int32_t* nb, WavlmWs& w) {
    const size_t D = h->cfg.conv_dim, C = h->cfg.n_state, F = h->cfg.n_ffn, T = nb[6], Bz = B;
    w.plan(A, Bz, D, nb);
    w.part = (float2*)A.f(Bz * (((size_t)nb[0] + 255) / 256) * D * 2);
    w.stat = (float2*)A.f(Bz * D * 2);
    w.wstat = (double2*)A.f(Bz * 4);
    w.wave = A.f(Bz * (size_t)L);
    w.gate = plan_tf(A, Bz, C, T, F * (T + 2), std::max(D, C), w, (size_t)h->cfg.n_head * T);
}
static int wavlm_shape_check(const lds_wavlm* h, int B, int64_t L, int32_t* nb) {
    if (!h) return set_error(LDS_EINVAL, "null handle");
    LDS_TRY(range_check("wavlm", "B", B, 1, 64));
    return conv_stack_shape_check("wavlm", h->cfg.n_ctx, B, L, 0, 0, nb);
}
extern "C" int lds_wavlm_workspace_bytes(const lds_wavlm* h, int B, int64_t L, size_t* out) {
    int32_t nb[kHubertLevels];
    return plan_bytes(out, [&] { return wavlm_shape_check(h, B, L, nb); }, [&](Arena& A) { WavlmWs w; plan_wavlm(h, A, B, L, nb, w); });
}

// audio -> feat ([B][T][conv_dim]) or enc ([B][T][n_state] = hidden_states[n_layers_run]).  Every argument has been checked.
// layer_w (host float[n_layer + 1], with n_layers_run = n_layer) or NULL: enc = sum_l layer_w[l] hidden_states[l] instead, each hidden state added
// where it exists, l ascending (launch_hubert_store_frames_acc); with NULL the launches are the plain encode's.
static int wavlm_run(lds_wavlm* h, const float* audio, int64_t L, const int32_t* lens_host, const int32_t* nb, float* feat, float* enc, int n_layers_run,
                     int normalize, void* ws, size_t ws_bytes, int B, void* stream, const float* layer_w = nullptr) {
    hipStream_t st = (hipStream_t)stream;
    ProfChain chain;
    Arena A(ws, ws_bytes);
    WavlmWs w;
    plan_wavlm(h, A, B, L, nb, w);
    if (!A.ok) return set_error(LDS_ENOMEM, "wavlm workspace too small: need %zu", A.used);
    const int D = h->cfg.conv_dim, C = h->cfg.n_state, T = nb[6], H = h->cfg.n_head, F = h->cfg.n_ffn;
    const bool stable = h->cfg.stable_layer_norm != 0;
    if (lens_host) LDS_TRY(w.upload(lens_host, 0, B, st));
    TileBatchScope tb(0);      // tile rules judged at the nominal batch: a clip's units do not depend on the batch it is in
    if (normalize) {
        HIP_TRY(launch_wavlm_wave_norm(audio, w.slen, L, w.wstat, w.wave, B, st));
        audio = w.wave;
    }
    float* x = w.ca;
    if (stable) {      // w2v_run's stack: conv_i into cb, GELU(LayerNorm(.)) back into ca
        HIP_TRY(launch_w2v_conv0(audio, w.slen, L, h->w0, h->b0, h->ln_g[0], h->ln_b[0], 1e-5f, w.nlen[0], nb[0], D, w.ca, B, st));
        for (int i = 1; i < kHubertLevels; ++i) {
            LensScope ls(w.nlen[i]);
            DOpt o;
            o.stride = 2; o.pad = 0;
            LDS_TRY(run_dconv(h->conv[i - 1], w.ca, D, nullptr, 0, nb[i - 1], o, w.cb, B, st));
            HIP_TRY(launch_w2v_ln_act(w.cb, h->ln_g[i], h->ln_b[i], 1e-5f, w.ca, (i == kHubertLevels - 1 && enc) ? w.lnp : nullptr, w.nlen[i], B, D, nb[i], st));
        }
    } else {           // hubert_run's stack with pad 0: gelu(conv_i(.)), the levels alternating between ca and cb
        HIP_TRY(launch_hubert_conv0(audio, w.slen, L, 0, h->w0, h->ln_g[0], h->ln_b[0], 1e-5f, w.nlen[0], nb[0], D, w.part, w.stat, w.ca, B, st));
        float* xn = w.cb;
        for (int i = 1; i < kHubertLevels; ++i) {
            LensScope ls(w.nlen[i]);
            DOpt o;
            o.stride = 2; o.pad = 0; o.epi = EPI_GELU;
            if (i == kHubertLevels - 1) o.lnpart_out = w.lnp;
            LDS_TRY(run_dconv(h->conv[i - 1], x, D, nullptr, 0, nb[i - 1], o, xn, B, st));
            { float* t = x; x = xn; xn = t; }
        }
    }
    const int* flen = w.nlen[kHubertLevels - 1];
    if (feat) HIP_TRY(launch_hubert_store_frames(x, feat, flen, B, D, T, st));
    if (!enc) return LDS_OK;
    LensScope ls(flen);
    {
        DOpt o;      // projection(layer_norm(.))
        o.ln_part = w.lnp; o.ln_np = D / 32; o.ln_c1 = h->fproj_c1; o.ln_c2 = h->fproj_c2;
        LDS_TRY(run_dconv(h->fproj, x, D, nullptr, 0, T, o, w.xa, B, st));
    }
    HIP_TRY(launch_hubert_posconv(w.xa, h->pos_w, h->pos_b, w.xb, flen, B, C, T, h->cfg.pos_kernel, h->cfg.pos_groups, st));
    // the residual stream is w.xb in the stable flavour (w.xa holds a block's layer_norm output), w.xa in the post-LN flavour
    if (!stable) HIP_TRY(launch_hubert_ln(w.xb, h->norm_g, h->norm_b, 1e-5f, w.xa, flen, B, C, T, st));
    for (int l = 0; l < n_layers_run; ++l) {
        const WavlmBlockW& bw = h->blocks[l];
        if (layer_w) HIP_TRY(launch_hubert_store_frames_acc(stable ? w.xb : w.xa, enc, flen, layer_w[l], l == 0, B, C, T, st));
        if (stable) HIP_TRY(launch_hubert_ln(w.xb, bw.n1_g, bw.n1_b, 1e-5f, w.xa, flen, B, C, T, st));
        const DOpt oq = qkv_opt(C, w.v);      // q | k | v and the gate of the attention input w.xa
        LDS_TRY(run_dconv(bw.qkv, w.xa, C, nullptr, 0, T, oq, w.qk, B, st));
        HIP_TRY(launch_wavlm_gate(w.xa, bw.gate_w, bw.gate_b, bw.gate_c, w.gate, flen, B, C, T, H, st));
        HIP_TRY(launch_attention_k4p_bias(w.qk, w.v, w.gate, h->toep, w.att, B, C, T, H, flen, h->cfg.n_ctx, st));
        if (stable) {
            DOpt oo;      // x + out_proj(.), partials for final_layer_norm
            oo.res = w.xb; oo.lnpart_out = w.lnp;
            LDS_TRY(run_dconv(bw.out, w.att, C, nullptr, 0, T, oo, w.xa, B, st));
            DOpt o1;      // gelu(intermediate_dense(final_layer_norm(.)))
            o1.epi = EPI_GELU;
            o1.ln_part = w.lnp; o1.ln_np = C / 32; o1.ln_c1 = bw.fc1_c1; o1.ln_c2 = bw.fc1_c2;
            LDS_TRY(run_dconv(bw.fc1, w.xa, C, nullptr, 0, T, o1, w.big, B, st));
            DOpt o2;      // + output_dense(.)
            o2.res = w.xa;
            LDS_TRY(run_dconv(bw.fc2, w.big, F, nullptr, 0, T, o2, w.xb, B, st));
        } else {
            DOpt oo;      // x + out_proj(.), then layer_norm
            oo.res = w.xa;
            LDS_TRY(run_dconv(bw.out, w.att, C, nullptr, 0, T, oo, w.xb, B, st));
            HIP_TRY(launch_hubert_ln(w.xb, bw.n1_g, bw.n1_b, 1e-5f, w.xa, flen, B, C, T, st));
            DOpt o1;      // gelu(intermediate_dense(.))
            o1.epi = EPI_GELU;
            LDS_TRY(run_dconv(bw.fc1, w.xa, C, nullptr, 0, T, o1, w.big, B, st));
            DOpt o2;      // + output_dense(.), then final_layer_norm
            o2.res = w.xa;
            LDS_TRY(run_dconv(bw.fc2, w.big, F, nullptr, 0, T, o2, w.xb, B, st));
            HIP_TRY(launch_hubert_ln(w.xb, bw.n2_g, bw.n2_b, 1e-5f, w.xa, flen, B, C, T, st));
        }
    }
    if (stable && n_layers_run == h->cfg.n_layer) {      // hidden_states[n_layer] is behind encoder.layer_norm, the earlier ones are not
        HIP_TRY(launch_hubert_ln(w.xb, h->norm_g, h->norm_b, 1e-5f, w.xa, flen, B, C, T, st));
        if (layer_w) HIP_TRY(launch_hubert_store_frames_acc(w.xa, enc, flen, layer_w[n_layers_run], 0, B, C, T, st));
        else HIP_TRY(launch_hubert_store_frames(w.xa, enc, flen, B, C, T, st));
    } else if (layer_w) {
        HIP_TRY(launch_hubert_store_frames_acc(w.xa, enc, flen, layer_w[n_layers_run], 0, B, C, T, st));
    } else {
        HIP_TRY(launch_hubert_store_frames(stable ? w.xb : w.xa, enc, flen, B, C, T, st));
    }
    return LDS_OK;
}

static int wavlm_audio_check(const lds_wavlm* h, const float* audio, const int32_t* lengths, const void* out, const void* ws, int B, int64_t L, int normalize,
                             int32_t* nb) {
    if (!h || !audio || !out || !ws) return set_error(LDS_EINVAL, "null argument");
    LDS_TRY(wavlm_shape_check(h, B, L, nb));
    if (normalize != 0 && normalize != 1) return set_error(LDS_EINVAL, "wavlm: normalize %d (0 or 1)", normalize);
    if (lengths) LDS_TRY(clip_lens_check("length", lengths, B, 400, L));
    return LDS_OK;
}
extern "C" int lds_wavlm_features(lds_wavlm* h, const float* audio, const int32_t* lengths, float* out, int normalize, void* ws, size_t ws_bytes, int B,
                                  int64_t L, void* stream) {
    int32_t nb[kHubertLevels];
    LDS_TRY(wavlm_audio_check(h, audio, lengths, out, ws, B, L, normalize, nb));
    return wavlm_run(h, audio, L, lengths, nb, out, nullptr, 0, normalize, ws, ws_bytes, B, stream);
}
extern "C" int lds_wavlm_encode(lds_wavlm* h, const float* audio, const int32_t* lengths, float* out, int n_layers_run, int normalize, void* ws,
                                size_t ws_bytes, int B, int64_t L, void* stream) {
    int32_t nb[kHubertLevels];
    LDS_TRY(wavlm_audio_check(h, audio, lengths, out, ws, B, L, normalize, nb));
    if (n_layers_run < 0 || n_layers_run > h->cfg.n_layer) return set_error(LDS_EINVAL, "wavlm: n_layers_run %d outside 0 .. %d", n_layers_run, h->cfg.n_layer);
    return wavlm_run(h, audio, L, lengths, nb, nullptr, out, n_layers_run, normalize, ws, ws_bytes, B, stream);
}
extern "C" int lds_wavlm_encode_layersum(lds_wavlm* h, const float* audio, const int32_t* lengths, const float* layer_w, float* out, int normalize, void* ws,
                                         size_t ws_bytes, int B, int64_t L, void* stream) {
    int32_t nb[kHubertLevels];
    LDS_TRY(wavlm_audio_check(h, audio, lengths, out, ws, B, L, normalize, nb));
    if (!layer_w) return set_error(LDS_EINVAL, "wavlm: null layer_w");
    for (int l = 0; l <= h->cfg.n_layer; ++l)
        if (!std::isfinite(layer_w[l])) return set_error(LDS_EINVAL, "wavlm: layer_w[%d] is not finite", l);
    return wavlm_run(h, audio, L, lengths, nb, nullptr, out, h->cfg.n_layer, normalize, ws, ws_bytes, B, stream, layer_w);
}

// ================================================================================================
// w2v-BERT 2.0 units encoder (reference tools/tools.py Wav2Vec2Bert: transformers' Wav2Vec2BertModel on SeamlessM4TFeatureExtractor's
// input_features, with its attention mask).  A Kaldi-style filter bank (w2vbert.hip), LayerNorm + Linear, then n_layer Conformer blocks:
// half-step feed-forward, self-attention with a relative-key bias, convolution module, half-step feed-forward, LayerNorm.  The four
// pre-LayerNorms of a block are folded into the GEMMs that read them (pack_ln_fold), the 0.5 of the half steps into output_dense, swish
// and GLU are conv_dma epilogues, final_layer_norm is materialised because it is the next block's residual stream.
// A clip of n frames gives rows = (n + 1) / 2 rows of which valid = n / 2 are unmasked: with n odd the last row is a query and a residual
// row like any other, but no attention key, zero behind the feature projection and zero as the convolution module's input.
// Launches per encode: 2 or 3 small uploads (rows, unmasked rows; the sample counts when lengths are given: launch_set_list) + 3 (filter bank)
// + 1 (K4P + partials) + 1 (projection) + 13 per block, 12 in the last (no partials behind the last final_layer_norm) + 1 (frame-major
// store): 319 at 24 layers without lengths, 320 with.
// ================================================================================================
struct W2vbertBlockW {
    ConvW f1a, f1b, qkv, out, pw1, pw2, f2a, f2b;
    float *f1_c1 = nullptr, *f1_c2 = nullptr, *qkv_c1 = nullptr, *qkv_c2 = nullptr, *pw1_c1 = nullptr, *pw1_c2 = nullptr, *f2_c1 = nullptr, *f2_c2 = nullptr;
    float *E = nullptr, *dw = nullptr, *dw_g = nullptr, *dw_b = nullptr, *fin_g = nullptr, *fin_b = nullptr;
};
struct lds_w2vbert {
    lds_w2vbert_cfg cfg;
    Owner own;
    double* basis = nullptr;      // [400][257] (cos, sin): 2^15, mean removal, pre-emphasis and the Povey window folded in
    float* filtT = nullptr;       // [257][n_mels] Kaldi mel triangles
    ConvW fproj;                  // feature_projection.layer_norm folded into feature_projection.projection
    float *fproj_c1 = nullptr, *fproj_c2 = nullptr;
    std::vector<W2vbertBlockW> blocks;
};
constexpr int kFbFrame = 400, kFbHop = 160, kFbFft = 512, kFbBins = 257;
constexpr float kFbMelFloor = 1.192092955078125e-07f;
constexpr int kW2vbertMinSamples = kFbFrame + kFbHop;      // two frames: one frame makes the ddof = 1 variance 0 / 0 in the reference

// The frame's whole linear front end as one [400][257] complex matrix (audio_utils.spectrogram's order): x * 2^15, minus the frame's mean,
// y[0] = 0.03 u[0], y[j] = u[j] - 0.97 u[j - 1], times hanning(400) ^ 0.85, zero-padded DFT of 512.
static std::vector<double> w2vbert_basis() {
    const double PI = 3.14159265358979323846;
    std::vector<double> win(kFbFrame), g((size_t)kFbFrame * kFbBins * 2), out((size_t)kFbFrame * kFbBins * 2);
    for (int i = 0; i < kFbFrame; ++i) win[i] = pow(0.5 - 0.5 * cos(2.0 * PI * i / (kFbFrame - 1)), 0.85);
    auto e = [&](int i, int k, int part) {
        const double a = 2.0 * PI * (double)((i * k) % kFbFft) / kFbFft;
        return win[i] * (part ? -sin(a) : cos(a));
    };
    for (int k = 0; k < kFbBins; ++k)
        for (int part = 0; part < 2; ++part) {
            double G = 0.0;
            for (int i = 0; i < kFbFrame; ++i) {
                double v = e(i, k, part);
                if (i + 1 < kFbFrame) v -= 0.97 * e(i + 1, k, part);
                if (i == 0) v -= 0.97 * e(0, k, part);
                g[((size_t)i * kFbBins + k) * 2 + part] = v;
                G += v;
            }
            for (int i = 0; i < kFbFrame; ++i) out[((size_t)i * kFbBins + k) * 2 + part] = (g[((size_t)i * kFbBins + k) * 2 + part] - G / kFbFrame) * 32768.0;
        }
    return out;
}
// Kaldi-scale mel triangles, built in mel space (audio_utils.mel_filter_bank with mel_scale "kaldi", triangularize_in_mel_space, no norm):
// n_mels filters between 20 Hz and 8 kHz over the 257 bins of a 512-point DFT at 16 kHz; [257][n_mels]
static std::vector<float> w2vbert_mel_filters(int n_mels) {
    auto mel = [](double f) { return 1127.0 * log(1.0 + f / 700.0); };
    const double lo = mel(20.0), hi = mel(8000.0);
    std::vector<double> c(n_mels + 2);
    for (int i = 0; i < n_mels + 2; ++i) c[i] = lo + (hi - lo) * i / (n_mels + 1);
    std::vector<float> f((size_t)kFbBins * n_mels);
    for (int k = 0; k < kFbBins; ++k) {
        const double fm = mel(16000.0 / kFbFft * k);
        for (int m = 0; m < n_mels; ++m) {
            const double down = (fm - c[m]) / (c[m + 1] - c[m]), up = (c[m + 2] - fm) / (c[m + 2] - c[m + 1]);
            f[(size_t)k * n_mels + m] = (float)std::max(0.0, std::min(down, up));
        }
    }
    return f;
}

static int w2vbert_cfg_check(const lds_w2vbert_cfg* c) {
    if (!c) return set_error(LDS_EINVAL, "null argument");
    if (c->n_mels < 8 || c->n_mels > 128 || c->stride < 1 || c->stride > 8 || (c->n_mels * c->stride) % 32 || c->n_mels * c->stride > 1024)
        return set_error(LDS_EINVAL, "w2vbert: n_mels %d x stride %d must be a multiple of 32 up to 1024 (n_mels 8 .. 128, stride 1 .. 8)", c->n_mels, c->stride);
    LDS_TRY(width_check("w2vbert", "n_state", c->n_state, true));
    LDS_TRY(heads_check("w2vbert", c->n_state, c->n_head));
    LDS_TRY(width_check("w2vbert", "n_ffn", c->n_ffn, false));
    LDS_TRY(range_check("w2vbert", "n_layer", c->n_layer, 1, 64));
    if (c->left_max < 0 || c->right_max < 0 || c->left_max + c->right_max + 1 > kW2vbertRelStride)
        return set_error(LDS_EINVAL, "w2vbert: left_max %d + right_max %d + 1 distances exceed %d", c->left_max, c->right_max, kW2vbertRelStride);
    if (c->dw_kernel < 1 || c->dw_kernel > 31 || !(c->dw_kernel & 1)) return set_error(LDS_EINVAL, "w2vbert: dw_kernel %d must be odd in 1 .. 31", c->dw_kernel);
    LDS_TRY(range_check("w2vbert", "n_ctx", c->n_ctx, 1, 1500));
    if (!(c->eps > 0.f) || !(c->eps < 1.f)) return set_error(LDS_EINVAL, "w2vbert: eps %g outside (0, 1)", (double)c->eps);
    return LDS_OK;
}

extern "C" int lds_w2vbert_create(const lds_w2vbert_cfg* cfg, int n, const char* const* names, const float* const* ptrs, const int64_t* numel, lds_w2vbert** out) {
    if (!cfg || !names || !ptrs || !numel || !out || n < 0) return set_error(LDS_EINVAL, "null argument");
    LDS_TRY(w2vbert_cfg_check(cfg));
    const int Fd = cfg->n_mels * cfg->stride, C = cfg->n_state, F = cfg->n_ffn, K = cfg->dw_kernel, NR = cfg->left_max + cfg->right_max + 1;
    lds_w2vbert* h = new lds_w2vbert();
    h->cfg = *cfg;
    WeightLoader T(h->own, n, names, ptrs, numel);
    Owner& o = h->own;
    bool ok = true;
    {
        const std::vector<double> bs = w2vbert_basis();
        h->basis = (double*)o.upload_bytes(bs.data(), bs.size() * sizeof(double));
        h->filtT = o.upload(w2vbert_mel_filters(cfg->n_mels));
        ok = h->basis && h->filtT;
    }
    if (ok) {
        const float *g = T.get("feature_projection.layer_norm.weight", Fd), *b = T.get("feature_projection.layer_norm.bias", Fd);
        const float *w = T.get("feature_projection.projection.weight", (int64_t)C * Fd), *wb = T.get("feature_projection.projection.bias", C);
        ok = g && b && w && wb && pack_ln_fold(o, w, wb, g, b, C, Fd, {}, h->fproj, h->fproj_c1, h->fproj_c2);
    }
    // GLU's rows: value and gate of the same channels in one wave's two MFMA row tiles (pack_geglu's interleave)
    std::vector<int> glu_perm((size_t)2 * C);
    for (int m = 0; m < 2 * C; ++m) glu_perm[m] = ((m % 64) / 32 ? C : 0) + 32 * (m / 64) + m % 32;
    h->blocks.resize(cfg->n_layer);
    for (int l = 0; l < cfg->n_layer && ok; ++l) {
        const std::string p = "encoder.layers." + std::to_string(l) + ".";
        W2vbertBlockW& bw = h->blocks[l];
        const int64_t CC = (int64_t)C * C, FC = (int64_t)F * C;
        // a half-step feed-forward: LayerNorm folded into intermediate_dense, the 0.5 into output_dense
        auto ffn = [&](const std::string& ln, const std::string& ff, ConvW& a, float*& c1, float*& c2, ConvW& bq) -> bool {
            const float *g = T.get(p + ln + ".weight", C), *b = T.get(p + ln + ".bias", C);
            const float *w1 = T.get(p + ff + ".intermediate_dense.weight", FC), *b1 = T.get(p + ff + ".intermediate_dense.bias", F);
            const float *w2 = T.get(p + ff + ".output_dense.weight", FC), *b2 = T.get(p + ff + ".output_dense.bias", C);
            if (!g || !b || !w1 || !b1 || !w2 || !b2) return false;
            std::vector<float> hw(w2, w2 + FC), hb(b2, b2 + C);
            for (float& v : hw) v *= 0.5f;
            for (float& v : hb) v *= 0.5f;
            return pack_ln_fold(o, w1, b1, g, b, F, C, {}, a, c1, c2) && pack_conv(o, hw.data(), hb.data(), C, F, 1, bq);
        };
        ok = ffn("ffn1_layer_norm", "ffn1", bw.f1a, bw.f1_c1, bw.f1_c2, bw.f1b) && ffn("ffn2_layer_norm", "ffn2", bw.f2a, bw.f2_c1, bw.f2_c2, bw.f2b);
        if (!ok) break;
        const float *ag = T.get(p + "self_attn_layer_norm.weight", C), *ab = T.get(p + "self_attn_layer_norm.bias", C);
        const float *qw = T.get(p + "self_attn.linear_q.weight", CC), *qb = T.get(p + "self_attn.linear_q.bias", C);
        const float *kw = T.get(p + "self_attn.linear_k.weight", CC), *kb = T.get(p + "self_attn.linear_k.bias", C);
        const float *vw = T.get(p + "self_attn.linear_v.weight", CC), *vb = T.get(p + "self_attn.linear_v.bias", C);
        const float *ow = T.get(p + "self_attn.linear_out.weight", CC), *ob = T.get(p + "self_attn.linear_out.bias", C);
        const float *cg = T.get(p + "conv_module.layer_norm.weight", C), *cbt = T.get(p + "conv_module.layer_norm.bias", C);
        const float *p1 = T.get(p + "conv_module.pointwise_conv1.weight", 2 * CC), *p2 = T.get(p + "conv_module.pointwise_conv2.weight", CC);
        const float* dw = T.get(p + "conv_module.depthwise_conv.weight", (int64_t)C * K);
        if (!ag || !ab || !qw || !qb || !kw || !kb || !vw || !vb || !ow || !ob || !cg || !cbt || !p1 || !p2 || !dw) { ok = false; break; }
        const QkvCat qkv = cat_qkv(qw, kw, vw, qb, kb, vb, C);
        std::vector<float> dwp((size_t)C * K);      // [K4P row][k][4]: row = (c / 8) * 2 + (c & 1), element (c & 7) / 2
        for (int c = 0; c < C; ++c)
            for (int k = 0; k < K; ++k) dwp[((size_t)((c >> 3) * 2 + (c & 1)) * K + k) * 4 + ((c & 7) >> 1)] = dw[(size_t)c * K + k];
        bw.dw = o.upload(dwp);
        bw.E = T.vec(p + "self_attn.distance_embedding.weight", (int64_t)NR * 64);
        bw.dw_g = T.vec(p + "conv_module.depthwise_layer_norm.weight", C);
        bw.dw_b = T.vec(p + "conv_module.depthwise_layer_norm.bias", C);
        bw.fin_g = T.vec(p + "final_layer_norm.weight", C);
        bw.fin_b = T.vec(p + "final_layer_norm.bias", C);
        ok = bw.dw && bw.E && bw.dw_g && bw.dw_b && bw.fin_g && bw.fin_b &&
             pack_ln_fold(o, qkv.w.data(), qkv.b.data(), ag, ab, 3 * C, C, {}, bw.qkv, bw.qkv_c1, bw.qkv_c2) && pack_conv(o, ow, ob, C, C, 1, bw.out) &&
             pack_ln_fold(o, p1, nullptr, cg, cbt, 2 * C, C, glu_perm, bw.pw1, bw.pw1_c1, bw.pw1_c2) && pack_conv(o, p2, nullptr, C, C, 1, bw.pw2);
    }
    return T.finish(ok, "w2vbert", h, out);
}
extern "C" void lds_w2vbert_destroy(lds_w2vbert* h) { delete h; }

static int w2vbert_frames(int64_t n) { return n < kFbFrame ? 0 : (int)((n - kFbFrame) / kFbHop) + 1; }

struct W2vbertWs : TfWs {          // lnp: LayerNorm partials of the residual stream
    int *slen, *rows, *valid;      // device copies: the clips' sample counts, rows and unmasked rows
    float* logspec; double2* stat;
    float* feats;                  // input_features when the caller does not receive them
    float* fk; float2* lnf;        // ... as K4P, and their LayerNorm partials
    float* relp;
};
static void plan_w2vbert(const lds_w2vbert* h, Arena& A, int B, int N, int R, W2vbertWs& w) {
    const size_t M = h->cfg.n_mels, Fd = (size_t)h->cfg.n_mels * h->cfg.stride, C = h->cfg.n_state, F = h->cfg.n_ffn, T = R, Bz = B;
    w.slen = (int*)A.f(64); w.rows = (int*)A.f(64); w.valid = (int*)A.f(64);
    w.logspec = A.f(Bz * M * (size_t)N);
    w.stat = (double2*)A.f(Bz * M * 4);
    w.feats = A.f(Bz * T * Fd);
    w.fk = A.f(Bz * Fd * (T + 2));
    w.lnf = (float2*)A.f(Bz * (Fd / 32) * T * 2);
    w.relp = plan_tf(A, Bz, C, T, F * (T + 2), C, w, h->cfg.n_head * T * kW2vbertRelStride);
}
// the limits of one call: B clips in buffers of L samples -> N frames, R rows
static int w2vbert_shape_check(const lds_w2vbert* h, int B, int64_t L, int& N, int& R) {
    if (!h) return set_error(LDS_EINVAL, "null handle");
    LDS_TRY(range_check("w2vbert", "B", B, 1, 64));
    if (L < kW2vbertMinSamples || L > ((int64_t)1 << 30)) return set_error(LDS_EINVAL, "w2vbert: L %lld outside %d .. 2^30 samples", (long long)L, kW2vbertMinSamples);
    N = w2vbert_frames(L);
    R = (N + h->cfg.stride - 1) / h->cfg.stride;
    if (R > h->cfg.n_ctx) return set_error(LDS_EINVAL, "w2vbert: %d rows exceed n_ctx %d", R, h->cfg.n_ctx);
    return LDS_OK;
}
extern "C" int lds_w2vbert_workspace_bytes(const lds_w2vbert* h, int B, int64_t L, size_t* out) {
    int N, R;
    return plan_bytes(out, [&] { return w2vbert_shape_check(h, B, L, N, R); }, [&](Arena& A) { W2vbertWs w; plan_w2vbert(h, A, B, N, R, w); });
}

// audio -> feats_out ([B][R][n_mels * stride]) and / or enc ([B][R][n_state]); or feats_in -> enc.  nfr: every clip's frame count (host, [B]),
// N / R: the buffers' frames / rows.  Every argument has been checked.
static int w2vbert_run(lds_w2vbert* h, const float* audio, int64_t L, const int32_t* slen_host, const float* feats_in, const int32_t* nfr, int N, int R,
                       float* feats_out, float* enc, void* ws, size_t ws_bytes, int B, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    ProfChain chain;
    Arena A(ws, ws_bytes);
    W2vbertWs w;
    plan_w2vbert(h, A, B, N, R, w);
    if (!A.ok) return set_error(LDS_ENOMEM, "w2vbert workspace too small: need %zu", A.used);
    const lds_w2vbert_cfg& c = h->cfg;
    const int Fd = c.n_mels * c.stride, C = c.n_state, T = R;
    int32_t rows[64], valid[64];
    for (int b = 0; b < B; ++b) { rows[b] = (nfr[b] + c.stride - 1) / c.stride; valid[b] = nfr[b] / c.stride; }
    LDS_TRY(upload_clip_ints(rows, B, w.rows, st));
    LDS_TRY(upload_clip_ints(valid, B, w.valid, st));
    const float* feats = feats_in;
    if (audio) {
        const int* slen = nullptr;
        if (slen_host) {
            LDS_TRY(upload_clip_ints(slen_host, B, w.slen, st));
            slen = w.slen;
        }
        float* fo = feats_out ? feats_out : w.feats;
        HIP_TRY(launch_w2vbert_fbank(audio, slen, L, N, R, h->basis, h->filtT, c.n_mels, c.stride, kFbMelFloor, w.logspec, w.stat, fo, B, st));
        feats = fo;
    }
    if (!enc) return LDS_OK;
    TileBatchScope tb(0);      // tile rules judged at the nominal batch: a clip's units do not depend on the batch it is in
    HIP_TRY(launch_w2vbert_feats_k4p(feats, w.fk, w.lnf, w.valid, B, Fd, T, st));
    float* x = w.xa;
    float* xn = w.xb;
    {
        LensScope lv(w.valid);      // rows at and beyond `valid` are zeros behind the projection (Wav2Vec2BertEncoder.forward's masked_fill)
        DOpt o;
        o.ln_part = w.lnf; o.ln_np = Fd / 32; o.ln_eps = c.eps; o.ln_c1 = h->fproj_c1; o.ln_c2 = h->fproj_c2;
        o.lnpart_out = w.lnp;
        LDS_TRY(run_dconv(h->fproj, w.fk, Fd, nullptr, 0, T, o, x, B, st));
    }
    LensScope ls(w.rows);
    float* glu = w.att;      // the convolution module's two tensors reuse attention's (both are consumed before the module starts)
    float* dwo = w.qk;
    for (const W2vbertBlockW& bw : h->blocks) {
        auto ffn = [&](const ConvW& a, const float* c1, const float* c2, const ConvW& bq, float* xin, float* xout, float2* part_out) -> int {
            DOpt o1;      // swish(intermediate_dense(layer_norm(.)))
            o1.epi = EPI_SWISH;
            o1.ln_part = w.lnp; o1.ln_np = C / 32; o1.ln_eps = c.eps; o1.ln_c1 = c1; o1.ln_c2 = c2;
            LDS_TRY(run_dconv(a, xin, C, nullptr, 0, T, o1, w.big, B, st));
            DOpt o2;      // + 0.5 output_dense(.)
            o2.res = xin; o2.lnpart_out = part_out;
            return run_dconv(bq, w.big, c.n_ffn, nullptr, 0, T, o2, xout, B, st);
        };
        LDS_TRY(ffn(bw.f1a, bw.f1_c1, bw.f1_c2, bw.f1b, x, xn, w.lnp));      // partials for self_attn_layer_norm
        std::swap(x, xn);
        const DOpt oq = qkv_opt(C, w.v, w.lnp, bw.qkv_c1, bw.qkv_c2, c.eps);      // q | k | v of self_attn_layer_norm(x)
        LDS_TRY(run_dconv(bw.qkv, x, C, nullptr, 0, T, oq, w.qk, B, st));
        HIP_TRY(launch_w2vbert_relpos(w.qk, bw.E, w.relp, w.rows, B, C, T, c.n_head, c.left_max + c.right_max + 1, st));
        HIP_TRY(launch_attention_k4p_rel(w.qk, w.v, w.relp, w.att, B, C, T, c.n_head, w.rows, w.valid, c.left_max, c.right_max, st));
        DOpt oo;      // x + linear_out(.), partials for conv_module.layer_norm
        oo.res = x; oo.lnpart_out = w.lnp;
        LDS_TRY(run_dconv(bw.out, w.att, C, nullptr, 0, T, oo, xn, B, st));
        std::swap(x, xn);
        {
            LensScope lv(w.valid);      // the module's input is zero on the masked row: GLU(pointwise_conv1(0)) = 0, written as zeros
            DOpt og;
            og.epi = EPI_GLU;
            og.ln_part = w.lnp; og.ln_np = C / 32; og.ln_eps = c.eps; og.ln_c1 = bw.pw1_c1; og.ln_c2 = bw.pw1_c2;
            LDS_TRY(run_dconv(bw.pw1, x, C, nullptr, 0, T, og, glu, B, st));
        }
        HIP_TRY(launch_w2vbert_dwconv(glu, bw.dw, bw.dw_g, bw.dw_b, c.eps, dwo, w.valid, w.rows, B, C, T, c.dw_kernel, st));
        DOpt op;      // x + pointwise_conv2(.), partials for ffn2_layer_norm
        op.res = x; op.lnpart_out = w.lnp;
        LDS_TRY(run_dconv(bw.pw2, dwo, C, nullptr, 0, T, op, xn, B, st));
        std::swap(x, xn);
        LDS_TRY(ffn(bw.f2a, bw.f2_c1, bw.f2_c2, bw.f2b, x, xn, nullptr));
        std::swap(x, xn);
        // final_layer_norm, materialised: it is the next block's residual stream; its partials serve the next ffn1_layer_norm
        HIP_TRY(launch_hubert_ln(x, bw.fin_g, bw.fin_b, c.eps, xn, w.rows, B, C, T, st));
        std::swap(x, xn);
        if (&bw != &h->blocks.back()) { HIP_TRY(launch_w2v_lnpart(x, w.lnp, w.rows, B, C, T, st)); }
    }
    HIP_TRY(launch_hubert_store_frames(x, enc, w.rows, B, C, T, st));
    return LDS_OK;
}

static int w2vbert_audio_check(const lds_w2vbert* h, const float* audio, const int32_t* lengths, const void* out, const void* ws, int B, int64_t L, int& N,
                               int& R, int32_t* nfr) {
    if (!h || !audio || !out || !ws) return set_error(LDS_EINVAL, "null argument");
    LDS_TRY(w2vbert_shape_check(h, B, L, N, R));
    if (lengths) LDS_TRY(clip_lens_check("length", lengths, B, kW2vbertMinSamples, L));
    for (int b = 0; b < B; ++b) nfr[b] = lengths ? w2vbert_frames(lengths[b]) : N;
    return LDS_OK;
}
extern "C" int lds_w2vbert_fbank(lds_w2vbert* h, const float* audio, const int32_t* lengths, float* out, void* ws, size_t ws_bytes, int B, int64_t L, void* stream) {
    int N, R;
    int32_t nfr[64];
    LDS_TRY(w2vbert_audio_check(h, audio, lengths, out, ws, B, L, N, R, nfr));
    return w2vbert_run(h, audio, L, lengths, nullptr, nfr, N, R, out, nullptr, ws, ws_bytes, B, stream);
}
extern "C" int lds_w2vbert_encode(lds_w2vbert* h, const float* audio, const int32_t* lengths, float* out, void* ws, size_t ws_bytes, int B, int64_t L, void* stream) {
    int N, R;
    int32_t nfr[64];
    LDS_TRY(w2vbert_audio_check(h, audio, lengths, out, ws, B, L, N, R, nfr));
    return w2vbert_run(h, audio, L, lengths, nullptr, nfr, N, R, nullptr, out, ws, ws_bytes, B, stream);
}
extern "C" int lds_w2vbert_encode_features(lds_w2vbert* h, const float* feats, const int32_t* n_frames, float* out, void* ws, size_t ws_bytes, int B, int R,
                                           void* stream) {
    if (!h || !feats || !out || !ws) return set_error(LDS_EINVAL, "null argument");
    LDS_TRY(range_check("w2vbert", "B", B, 1, 64));
    if (R < 1 || R > h->cfg.n_ctx) return set_error(LDS_EINVAL, "w2vbert: %d rows outside 1 .. n_ctx %d", R, h->cfg.n_ctx);
    const int st = h->cfg.stride;
    int32_t nfr[64];
    for (int b = 0; b < B; ++b) {
        nfr[b] = n_frames ? n_frames[b] : R * st;
        if (nfr[b] < 2 || nfr[b] < st || (nfr[b] + st - 1) / st > R) return set_error(LDS_EINVAL, "n_frames[%d] = %d outside %d .. %d", b, nfr[b], st > 2 ? st : 2, R * st);
    }
    return w2vbert_run(h, nullptr, 0, nullptr, feats, nfr, R * st, R, nullptr, out, ws, ws_bytes, B, stream);
}

// ================================================================================================
// Single-op test entry points
// ================================================================================================
extern "C" int lds_test_conv(const lds_conv_test* a, float* out, int B, void* stream) {
    if (!a || !out) return set_error(LDS_EINVAL, "bad argument");
    hipStream_t st = (hipStream_t)stream;
    Owner own;
    ConvW W;
    const int Ci = a->C1 + a->C2;
    if (!pack_conv(own, a->w, a->bias, a->Co, Ci, a->K, W)) return set_error(LDS_ENOMEM, "test conv: upload failed");
    ConvOpt o;
    o.pad = a->pad; o.dil = a->dil;
    o.act_in = a->act_in; o.slope = a->slope; o.res = a->res; o.epi = a->epilogue; o.tile = a->tile;
    Src s{a->x1, a->C1, a->x2, a->C2, a->Tsrc};
    const int r = run_conv(W, s, o, out, B, st);
    HIP_TRY(hipStreamSynchronize(st));   // test-only entry point: temporaries are freed on return
    return r;
}

// ---- K4P path test entry points: plain tensors in / out, converted on the device ----
struct TmpDev {
    std::vector<void*> p;
    ~TmpDev() { for (void* q : p) (void)hipFree(q); }
    float* f(size_t n) { void* d = nullptr; if (hipMalloc(&d, n * sizeof(float) + 65536) != hipSuccess) return nullptr; p.push_back(d); return (float*)d; }
};

// lds_test_tap_k4p (include/lds_test.h): the raw K4P output of the next K4P test entry, pad frames included.  An armed tap makes the entry
// fill that buffer with NaN before its launch (tap_fill) and copy it out, as it is, before converting it (tap_take).
static thread_local float* g_tap_dst = nullptr;
static thread_local size_t g_tap_floats = 0;
extern "C" int lds_test_tap_k4p(float* dst, size_t floats) {
    if ((dst != nullptr) != (floats > 0)) return set_error(LDS_EINVAL, "bad argument");
    g_tap_dst = dst; g_tap_floats = floats;
    return LDS_OK;
}
static hipError_t tap_fill(float* k, size_t floats, hipStream_t st) {
    return g_tap_dst ? hipMemsetAsync(k, 0xff, floats * sizeof(float), st) : hipSuccess;
}
static hipError_t tap_take(const float* k, size_t floats, hipStream_t st) {
    if (!g_tap_dst) return hipSuccess;
    float* dst = g_tap_dst;
    g_tap_dst = nullptr;
    if (floats != g_tap_floats) return hipErrorInvalidValue;      // the caller sized the buffer for another tensor
    return hipMemcpyAsync(dst, k, floats * sizeof(float), hipMemcpyDeviceToDevice, st);
}

// bf3 = 1: the same operator through the split-bf16 kernel (K8B3 tensors, conv_bf3.hip) with `nprod` bf16 products per fp32 product
static int dconv_test_impl(const lds_dconv_test* a, float* out, float* lnpart, int B, int iters, float* ms_out, void* stream, int bf3 = 0, int nprod = 0, int fmt = 0,
                           const int* alt_cfgs = nullptr, int n_alt = 0) {
    hipStream_t st = (hipStream_t)stream;
    Owner own;
    TmpDev tmp;
    ConvW W;
    const int Ci = a->C1 + a->C2, T = a->T;
    bool ok = (a->epilogue == EPI_GEGLU) ? pack_geglu(own, a->w, a->bias, a->Co, Ci, W) : pack_conv(own, a->w, a->bias, a->Co, Ci, a->K, W);
    if (ok && bf3) ok = make_split_twin(own, W, fmt);
    if (!ok) return set_error(LDS_ENOMEM, "test dconv: upload failed");
    auto act_floats = [&](int C, int Tl) { return bf3 ? (size_t)B * split_floats(fmt, C, Tl) : (size_t)B * C * (Tl + 2); };
    auto to_act = [&](const float* src, float* dst, int C, int Tl) { return bf3 ? launch_to_k8b3(src, dst, B, C, Tl, C, 0, st, fmt) : launch_to_k4p(src, dst, B, C, Tl, C, 0, st); };
    auto from_act = [&](const float* src, float* dst, int C, int Tl) { return bf3 ? launch_from_k8b3(src, dst, B, C, Tl, st, fmt) : launch_from_k4p(src, dst, B, C, Tl, st); };
    float* k1 = tmp.f(act_floats(a->C1, T));
    float* k2 = a->C2 ? tmp.f(act_floats(a->C2, T)) : nullptr;
    if (!k1 || (a->C2 && !k2)) return set_error(LDS_ENOMEM, "test dconv: alloc failed");
    HIP_TRY(to_act(a->x1, k1, a->C1, T));
    if (a->C2) HIP_TRY(to_act(a->x2, k2, a->C2, T));
    const int Cout = (a->epilogue == EPI_GEGLU) ? a->Co / 2 : a->Co;
    const int Tin = a->ups ? 2 * T : T;
    const int To = (Tin + 2 * a->pad - (a->K - 1) - 1) / a->stride + 1;
    const int Ck = a->v_split ? (Cout / 3) * 2 : Cout;
    DOpt o;
    o.stride = a->stride; o.pad = a->pad; o.ups = a->ups; o.epi = a->epilogue; o.cfg = a->cfg; o.out_plain = a->plain_out;
    const bool qk_f32 = bf3 && a->v_split;      // the QKV projection of the split-bf16 path keeps q / k in fp32 K4P for the attention kernel
    o.out_f32 = qk_f32 ? 1 : 0;
    float* kres = nullptr;
    if (a->res) {
        kres = tmp.f(act_floats(Ck, To));
        if (!kres) return set_error(LDS_ENOMEM, "alloc");
        HIP_TRY(to_act(a->res, kres, Ck, To));
        o.res = kres;
    }
    float* kout = a->plain_out ? out : tmp.f(qk_f32 ? (size_t)B * Ck * (To + 2) : act_floats(Ck, To));
    float* vout = nullptr;
    if (!kout) return set_error(LDS_ENOMEM, "alloc");
    const int To4 = (To + 3) & ~3;
    if (a->v_split) {
        vout = tmp.f((size_t)B * (Cout - Ck) * To4);
        if (!vout) return set_error(LDS_ENOMEM, "alloc");
        HIP_TRY(hipMemsetAsync(vout, 0xff, sizeof(float) * B * (Cout - Ck) * To4, st));      // NaN fill: the zero tail must be written
        o.plain_from = Ck; o.out2 = vout;
        if (a->v_split > 1) o.vt_D = a->v_split;      // value third in attention's VT layout with this head dim
    }
    o.lnpart_out = (float2*)lnpart;
    const bool tap = !bf3 && !a->plain_out;
    if (tap) HIP_TRY(tap_fill(kout, (size_t)B * Ck * (To + 2), st));
    auto run = [&]() { return bf3 ? run_dconv_bf3(W, k1, a->C1, k2, a->C2, T, o, kout, B, st, nprod, fmt) : run_dconv(W, k1, a->C1, k2, a->C2, T, o, kout, B, st); };
    int r = run();
    if (r == LDS_OK && iters > 0 && ms_out) {
        hipEvent_t e0, e1;
        HIP_TRY(hipEventCreate(&e0));
        HIP_TRY(hipEventCreate(&e1));
        HIP_TRY(hipEventRecord(e0, st));
        for (int i = 0; i < iters && r == LDS_OK; ++i) {
            if (n_alt > 0) o.cfg = alt_cfgs[i % n_alt];      // lds_bench_dconv_alt: consecutive launches rotate through kernel instantiations
            r = run();
        }
        HIP_TRY(hipEventRecord(e1, st));
        HIP_TRY(hipEventSynchronize(e1));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
        *ms_out = ms / iters;
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
    }
    auto from_out = [&](const float* src, float* dst, int C, int Tl) { return qk_f32 ? launch_from_k4p(src, dst, B, C, Tl, st) : from_act(src, dst, C, Tl); };
    if (r == LDS_OK && tap) HIP_TRY(tap_take(kout, (size_t)B * Ck * (To + 2), st));
    if (r == LDS_OK && !a->plain_out) {
        if (a->v_split > 1) {
            // out = [B][Ck][To] plain q;k, then the raw VT buffer [B][(Cout-Ck)/D][ceil4(To)/4][D][4]
            HIP_TRY(from_out(kout, out, Ck, To));
            HIP_TRY(hipMemcpyAsync(out + (size_t)B * Ck * To, vout, sizeof(float) * B * (Cout - Ck) * To4, hipMemcpyDeviceToDevice, st));
        } else if (a->v_split) {
            // out = [q;k] back to plain (first 2/3 of the channels) followed by the already-plain v third
            float* tmpo = tmp.f((size_t)B * Ck * To);
            if (!tmpo) return set_error(LDS_ENOMEM, "alloc");
            HIP_TRY(from_out(kout, tmpo, Ck, To));
            for (int b = 0; b < B; ++b) {
                HIP_TRY(hipMemcpyAsync(out + (size_t)b * Cout * To, tmpo + (size_t)b * Ck * To, sizeof(float) * Ck * To, hipMemcpyDeviceToDevice, st));
                HIP_TRY(hipMemcpyAsync(out + (size_t)b * Cout * To + (size_t)Ck * To, vout + (size_t)b * (Cout - Ck) * To,
                                       sizeof(float) * (Cout - Ck) * To, hipMemcpyDeviceToDevice, st));
            }
        } else {
            HIP_TRY(from_out(kout, out, Ck, To));
        }
    }
    HIP_TRY(hipStreamSynchronize(st));
    return r;
}
extern "C" int lds_test_dconv(const lds_dconv_test* a, float* out, float* lnpart, int B, void* stream) {
    if (!a || !out) return set_error(LDS_EINVAL, "bad argument");
    return dconv_test_impl(a, out, lnpart, B, 0, nullptr, stream);
}
extern "C" int lds_bench_dconv(const lds_dconv_test* a, float* out, int B, int iters, float* ms_out, char* cfg_out, size_t cfg_cap, void* stream) {
    if (!a || !out || !ms_out || iters <= 0) return set_error(LDS_EINVAL, "bad argument");
    int r = dconv_test_impl(a, out, nullptr, B, iters, ms_out, stream);
    if (cfg_out && cfg_cap) snprintf(cfg_out, cfg_cap, "%s", conv_dma_last_config());
    return r;
}
// the same launch `iters` times, rotating through the tile configurations cfgs[0 .. n) (instantiations of the same operator): what does a
// launch cost when the previous launch ran other code?  (tools/bench_icache.py)
extern "C" int lds_bench_dconv_alt(const lds_dconv_test* a, float* out, int B, int iters, const int* cfgs, int n, float* ms_out, void* stream) {
    if (!a || !out || !cfgs || n < 1 || !ms_out) return set_error(LDS_EINVAL, "bad argument");
    return dconv_test_impl(a, out, nullptr, B, iters, ms_out, stream, 0, 0, 0, cfgs, n);
}
extern "C" int lds_test_dconv_split(const lds_dconv_test* a, float* out, float* lnpart, int B, int nprod, int fmt, void* stream) {
    if (!a || !out || (fmt != FMT_BF16X3 && fmt != FMT_F16X2)) return set_error(LDS_EINVAL, "bad argument");
    return dconv_test_impl(a, out, lnpart, B, 0, nullptr, stream, 1, nprod, fmt);
}
extern "C" int lds_test_dconv_bf3(const lds_dconv_test* a, float* out, float* lnpart, int B, int nprod, void* stream) {
    return lds_test_dconv_split(a, out, lnpart, B, nprod, FMT_BF16X3, stream);
}
extern "C" int lds_bench_dconv_split(const lds_dconv_test* a, float* out, int B, int iters, int nprod, int fmt, float* ms_out, char* cfg_out, size_t cfg_cap,
                                     void* stream) {
    if (!a || !out || !ms_out || iters <= 0 || (fmt != FMT_BF16X3 && fmt != FMT_F16X2)) return set_error(LDS_EINVAL, "bad argument");
    int r = dconv_test_impl(a, out, nullptr, B, iters, ms_out, stream, 1, nprod, fmt);
    if (cfg_out && cfg_cap) snprintf(cfg_out, cfg_cap, "%s", conv_bf3_last_config());
    return r;
}
extern "C" int lds_bench_dconv_bf3(const lds_dconv_test* a, float* out, int B, int iters, int nprod, float* ms_out, char* cfg_out, size_t cfg_cap, void* stream) {
    if (!a || !out || !ms_out || iters <= 0) return set_error(LDS_EINVAL, "bad argument");
    int r = dconv_test_impl(a, out, nullptr, B, iters, ms_out, stream, 1, nprod, FMT_BF16X3);
    if (cfg_out && cfg_cap) snprintf(cfg_out, cfg_cap, "%s", conv_bf3_last_config());
    return r;
}

extern "C" int lds_test_gn_apply(const float* x1, const float* x2, int C1, int C2, int T, int groups, float eps, const float* gamma,
                                 const float* beta, const float* scale_shift, int silu, float* out, int B, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    Owner own;
    TmpDev tmp;
    const int C = C1 + C2, nT = (T + 31) / 32;
    float* g = up_vec(own, gamma, C);
    float* be = up_vec(own, beta, C);
    float* k1 = tmp.f((size_t)B * C1 * (T + 2));
    float* k2 = C2 ? tmp.f((size_t)B * C2 * (T + 2)) : nullptr;
    float* ky = tmp.f((size_t)B * C * (T + 2));
    float* p1 = tmp.f((size_t)B * (C1 / 16) * nT * 2);
    float* p2 = C2 ? tmp.f((size_t)B * (C2 / 16) * nT * 2) : nullptr;
    if (!g || !be || !k1 || (C2 && (!k2 || !p2)) || !ky || !p1) return set_error(LDS_ENOMEM, "alloc");
    HIP_TRY(launch_to_k4p(x1, k1, B, C1, T, C1, 0, st));
    HIP_TRY(launch_gn_partials(k1, C1, T, (float2*)p1, B, st));
    if (C2) {
        HIP_TRY(launch_to_k4p(x2, k2, B, C2, T, C2, 0, st));
        HIP_TRY(launch_gn_partials(k2, C2, T, (float2*)p2, B, st));
    }
    HIP_TRY(launch_gn_stream(k1, k2, C1, C2, T, groups, eps, g, be, scale_shift, 2 * C, 0, silu, (const float2*)p1, (const float2*)p2, ky, B, st));
    HIP_TRY(launch_from_k4p(ky, out, B, C, T, st));
    HIP_TRY(hipStreamSynchronize(st));
    return LDS_OK;
}

// timing of the streaming GroupNorm alone on zero-filled tensors (tools/bench_gn.py)
extern "C" int lds_bench_gn_stream(int C1, int C2, int T, int B, int iters, float* ms_out, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    TmpDev tmp;
    const int C = C1 + C2, nT = (T + 31) / 32;
    float* k1 = tmp.f((size_t)B * C1 * (T + 2));
    float* k2 = C2 ? tmp.f((size_t)B * C2 * (T + 2)) : nullptr;
    float* ky = tmp.f((size_t)B * C * (T + 2));
    float* p1 = tmp.f((size_t)B * (C1 / 16) * nT * 2);
    float* p2 = C2 ? tmp.f((size_t)B * (C2 / 16) * nT * 2) : nullptr;
    float* gb = tmp.f(2 * C);
    if (!k1 || (C2 && (!k2 || !p2)) || !ky || !p1 || !gb || iters <= 0 || !ms_out) return set_error(LDS_ENOMEM, "alloc");
    HIP_TRY(hipMemsetAsync(k1, 0, sizeof(float) * B * C1 * (T + 2), st));
    if (C2) HIP_TRY(hipMemsetAsync(k2, 0, sizeof(float) * B * C2 * (T + 2), st));
    HIP_TRY(hipMemsetAsync(gb, 0, sizeof(float) * 2 * C, st));
    HIP_TRY(launch_gn_partials(k1, C1, T, (float2*)p1, B, st));
    if (C2) HIP_TRY(launch_gn_partials(k2, C2, T, (float2*)p2, B, st));
    hipEvent_t e0, e1;
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    for (int w = 0; w < 3; ++w)
        HIP_TRY(launch_gn_stream(k1, k2, C1, C2, T, 8, 1e-5f, gb, gb + C, nullptr, 0, 0, 1, (const float2*)p1, (const float2*)p2, ky, B, st));
    HIP_TRY(hipEventRecord(e0, st));
    for (int i = 0; i < iters; ++i)
        HIP_TRY(launch_gn_stream(k1, k2, C1, C2, T, 8, 1e-5f, gb, gb + C, nullptr, 0, 0, 1, (const float2*)p1, (const float2*)p2, ky, B, st));
    HIP_TRY(hipEventRecord(e1, st));
    HIP_TRY(hipEventSynchronize(e1));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
    *ms_out = ms / iters;
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return LDS_OK;
}

// mid = conv1x1(x) written with the epilogue's GroupNorm partials; out = GroupNorm(mid) by the streaming pass that combines
// those partials (the statistics path the UNet uses)
extern "C" int lds_test_gn_chain_k4p(const float* x, const float* w1, const float* bias1, const float* gamma, const float* beta, float eps,
                                     int groups, int silu, float* mid, float* out, int B, int C, int Co, int T, int cfg, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    Owner own;
    TmpDev tmp;
    ConvW W1;
    if (!pack_conv(own, w1, bias1, Co, C, 1, W1)) return set_error(LDS_ENOMEM, "upload failed");
    float* g = up_vec(own, gamma, Co);
    float* be = up_vec(own, beta, Co);
    const int nT = (T + 31) / 32;
    float* kx = tmp.f((size_t)B * C * (T + 2));
    float* km = tmp.f((size_t)B * Co * (T + 2));
    float* ko = tmp.f((size_t)B * Co * (T + 2));
    float* gp = tmp.f((size_t)B * (Co / 16) * nT * 2);
    if (!g || !be || !kx || !km || !ko || !gp) return set_error(LDS_ENOMEM, "alloc");
    HIP_TRY(hipMemsetAsync(gp, 0xff, sizeof(float) * B * (Co / 16) * nT * 2, st));      // NaN fill: every partial must be written
    HIP_TRY(launch_to_k4p(x, kx, B, C, T, C, 0, st));
    DOpt o1;
    o1.gnpart_out = (float2*)gp; o1.cfg = cfg;
    LDS_TRY(run_dconv(W1, kx, C, nullptr, 0, T, o1, km, B, st));
    HIP_TRY(launch_gn_stream(km, nullptr, Co, 0, T, groups, eps, g, be, nullptr, 0, 0, silu, (const float2*)gp, nullptr, ko, B, st));
    HIP_TRY(launch_from_k4p(km, mid, B, Co, T, st));
    HIP_TRY(launch_from_k4p(ko, out, B, Co, T, st));
    HIP_TRY(hipStreamSynchronize(st));
    return LDS_OK;
}

// mid = w1 * x (1x1, emits LayerNorm partials); out = w2 * LayerNorm_C(mid) with the LayerNorm folded into conv2's epilogue
// conv (1x1, GroupNorm partials from its epilogue) -> proj(GroupNorm(mid)) as ONE launch with the normalisation folded (DmaConvArgs::gnf_part)
extern "C" int lds_test_gn_fold_k4p(const float* x, const float* w1, const float* bias1, const float* gamma, const float* beta, float eps, int groups,
                                    const float* w2, const float* bias2, float* mid, float* out, int B, int C, int Cm, int Co, int T, int cfg, int tile_batch,
                                    void* stream) {
    hipStream_t st = (hipStream_t)stream;
    Owner own;
    TmpDev tmp;
    ConvW W1, W2;
    float *cg = nullptr, *c2 = nullptr;
    if (!pack_conv(own, w1, bias1, Cm, C, 1, W1) || !pack_gn_fold(own, w2, bias2, gamma, beta, Co, Cm, groups, W2, cg, c2)) return set_error(LDS_ENOMEM, "upload failed");
    const int nT = (T + 31) / 32;
    float* kx = tmp.f((size_t)B * C * (T + 2));
    float* km = tmp.f((size_t)B * Cm * (T + 2));
    float* ko = tmp.f((size_t)B * Co * (T + 2));
    float* gp = tmp.f((size_t)B * (Cm / 16) * nT * 2);
    float* kpart = tmp.f((size_t)kClusterPartFloats);
    unsigned* kcount = (unsigned*)tmp.f(kClusterCounters);
    if (!kx || !km || !ko || !gp || !kpart || !kcount) return set_error(LDS_ENOMEM, "alloc");
    HIP_TRY(hipMemsetAsync(kcount, 0, sizeof(unsigned) * kClusterCounters, st));
    HIP_TRY(launch_to_k4p(x, kx, B, C, T, C, 0, st));
    DOpt o1;
    o1.gnpart_out = (float2*)gp;
    LDS_TRY(run_dconv(W1, kx, C, nullptr, 0, T, o1, km, B, st));
    {
        TileBatchScope tbs(tile_batch, kpart, kcount);      // tile_batch > 0: the latency mode's choices (cluster split-K through the fold)
        DOpt o2;
        o2.cfg = cfg;
        o2.gnf_part = (const float2*)gp; o2.gnf_groups = groups; o2.gnf_eps = eps; o2.gnf_cg = cg; o2.gnf_c2 = c2;
        LDS_TRY(run_dconv(W2, km, Cm, nullptr, 0, T, o2, ko, B, st));
    }
    HIP_TRY(launch_from_k4p(km, mid, B, Cm, T, st));
    HIP_TRY(launch_from_k4p(ko, out, B, Co, T, st));
    HIP_TRY(hipStreamSynchronize(st));
    return LDS_OK;
}

// the same through either kernel family (fmt -1 = exact fp32 / K4P, conv_dma.hip; 0 = three bf16 planes, 1 = two fp16 planes, conv_bf3.hip).  reps >= 1:
// the folded launch runs `reps` times on the same inputs into out[rep][B][Co][T] -- a determinism check: every repetition must equal the first
// bit for bit, also when several workgroups share a CU.
extern "C" int lds_test_gn_fold_split(const float* x, const float* w1, const float* bias1, const float* gamma, const float* beta, float eps, int groups,
                                      const float* w2, const float* bias2, float* mid, float* out, int B, int C, int Cm, int Co, int T, int cfg, int tile_batch,
                                      int fmt, int reps, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!x || !w1 || !w2 || !mid || !out || (fmt != -1 && fmt != FMT_BF16X3 && fmt != FMT_F16X2) || reps < 1) return set_error(LDS_EINVAL, "bad argument");
    const bool f32 = fmt < 0;
    Owner own;
    TmpDev tmp;
    ConvW W1, W2;
    float *cg = nullptr, *c2 = nullptr;
    if (!pack_conv(own, w1, bias1, Cm, C, 1, W1) || !pack_gn_fold(own, w2, bias2, gamma, beta, Co, Cm, groups, W2, cg, c2)) return set_error(LDS_ENOMEM, "upload failed");
    if (!f32 && (!make_split_twin(own, W1, fmt) || !make_split_twin(own, W2, fmt))) return set_error(LDS_ENOMEM, "upload failed");
    const int nT = (T + 31) / 32;
    auto act = [&](int Cc) { return f32 ? (size_t)Cc * (T + 2) : split_floats(fmt, Cc, T); };
    float* kx = tmp.f((size_t)B * act(C));
    float* km = tmp.f((size_t)B * act(Cm));
    float* ko = tmp.f((size_t)B * act(Co));
    float* gp = tmp.f((size_t)B * (Cm / 16) * nT * 2);
    float* kpart = tmp.f((size_t)kClusterPartFloats);
    unsigned* kcount = (unsigned*)tmp.f(kClusterCounters);
    if (!kx || !km || !ko || !gp || !kpart || !kcount) return set_error(LDS_ENOMEM, "alloc");
    HIP_TRY(hipMemsetAsync(kcount, 0, sizeof(unsigned) * kClusterCounters, st));
    HIP_TRY(to_act_any(f32 ? 0 : fmt + 1, x, kx, B, C, T, C, 0, st));
    DOpt o1;
    o1.gnpart_out = (float2*)gp;
    LDS_TRY(dconv_any(f32 ? 0 : fmt + 1, W1, kx, C, nullptr, 0, T, o1, km, B, st));
    if (f32) HIP_TRY(launch_from_k4p(km, mid, B, Cm, T, st));
    else HIP_TRY(launch_from_k8b3(km, mid, B, Cm, T, st, fmt));
    for (int rep = 0; rep < reps; ++rep) {
        {
            TileBatchScope tbs(tile_batch, kpart, kcount);
            DOpt o2;
            o2.cfg = cfg;
            o2.gnf_part = (const float2*)gp; o2.gnf_groups = groups; o2.gnf_eps = eps; o2.gnf_cg = cg; o2.gnf_c2 = c2;
            LDS_TRY(dconv_any(f32 ? 0 : fmt + 1, W2, km, Cm, nullptr, 0, T, o2, ko, B, st));
        }
        float* dst = out + (size_t)rep * B * Co * T;
        if (f32) HIP_TRY(launch_from_k4p(ko, dst, B, Co, T, st));
        else HIP_TRY(launch_from_k8b3(ko, dst, B, Co, T, st, fmt));
    }
    HIP_TRY(hipStreamSynchronize(st));
    return LDS_OK;
}

// The cluster split-K hand-off under test (conv_dma.hip / conv_bf3.hip cluster_join): a K-tap convolution Ci -> Co over [B, Ci, T] with the latency
// mode's tile and cluster choices at tile_batch = B, launched `reps` times back to back ALTERNATING between the inputs xa and xb -- the partial
// tiles of consecutive launches share their scratch slots, so a partial read stale (from this CU's L1, from the XCD's L2) is the other input's and
// shows as an O(1) error -- into out[rep][B][Co][T]; ref_a / ref_b: the same tile shapes with one workgroup per tile (no cluster).  fmt -1 = exact
// fp32 (conv_dma), 0 / 1 = split planes (conv_bf3).  cfg_out: the cluster launch's configuration string ("... KS<S> ...").
extern "C" int lds_test_cluster_join(const float* xa, const float* xb, const float* w, const float* bias, int Ci, int Co, int K, int T, int B, int fmt, int reps,
                                     float* out, float* ref_a, float* ref_b, char* cfg_out, size_t cfg_cap, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!xa || !xb || !w || !out || !ref_a || !ref_b || reps < 1 || (K != 1 && K != 3) || (fmt != -1 && fmt != FMT_BF16X3 && fmt != FMT_F16X2)) return set_error(LDS_EINVAL, "bad argument");
    const bool f32 = fmt < 0;
    const int mode = f32 ? 0 : fmt + 1;
    Owner own;
    TmpDev tmp;
    ConvW W;
    if (!pack_conv(own, w, bias, Co, Ci, K, W) || (!f32 && !make_split_twin(own, W, fmt))) return set_error(LDS_ENOMEM, "upload failed");
    auto act = [&](int Cc) { return f32 ? (size_t)Cc * (T + 2) : split_floats(fmt, Cc, T); };
    float* ka = tmp.f((size_t)B * act(Ci));
    float* kb = tmp.f((size_t)B * act(Ci));
    float* ko = tmp.f((size_t)B * act(Co));
    float* kpart = tmp.f((size_t)kClusterPartFloats);
    unsigned* kcount = (unsigned*)tmp.f(kClusterCounters);
    if (!ka || !kb || !ko || !kpart || !kcount) return set_error(LDS_ENOMEM, "alloc");
    HIP_TRY(hipMemsetAsync(kcount, 0, sizeof(unsigned) * kClusterCounters, st));
    HIP_TRY(to_act_any(mode, xa, ka, B, Ci, T, Ci, 0, st));
    HIP_TRY(to_act_any(mode, xb, kb, B, Ci, T, Ci, 0, st));
    DOpt o;
    o.pad = K / 2;
    auto back = [&](float* dst) { return f32 ? launch_from_k4p(ko, dst, B, Co, T, st) : launch_from_k8b3(ko, dst, B, Co, T, st, fmt); };
    {
        TileBatchScope tbs(B, nullptr, nullptr);      // the same tile choices, no scratch: one workgroup per tile
        LDS_TRY(dconv_any(mode, W, ka, Ci, nullptr, 0, T, o, ko, B, st));
        HIP_TRY(back(ref_a));
        LDS_TRY(dconv_any(mode, W, kb, Ci, nullptr, 0, T, o, ko, B, st));
        HIP_TRY(back(ref_b));
    }
    for (int rep = 0; rep < reps; ++rep) {
        {
            TileBatchScope tbs(B, kpart, kcount);
            LDS_TRY(dconv_any(mode, W, (rep & 1) ? kb : ka, Ci, nullptr, 0, T, o, ko, B, st));
        }
        if (rep == 0 && cfg_out && cfg_cap) snprintf(cfg_out, cfg_cap, "%s", f32 ? conv_dma_last_config() : conv_bf3_last_config());
        HIP_TRY(back(out + (size_t)rep * B * Co * T));
    }
    HIP_TRY(hipStreamSynchronize(st));
    return LDS_OK;
}

extern "C" int lds_test_ln_chain_k4p(const float* x, const float* w1, const float* w2, const float* gamma, const float* beta, float eps,
                                     float* mid, float* out, int B, int C, int Co, int T, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    Owner own;
    TmpDev tmp;
    ConvW W1, W2;
    float *c1 = nullptr, *c2 = nullptr;
    if (!pack_conv(own, w1, nullptr, C, C, 1, W1) || !pack_ln_fold(own, w2, nullptr, gamma, beta, Co, C, {}, W2, c1, c2)) return set_error(LDS_ENOMEM, "upload failed");
    float* kx = tmp.f((size_t)B * C * (T + 2));
    float* km = tmp.f((size_t)B * C * (T + 2));
    float* ko = tmp.f((size_t)B * Co * (T + 2));
    float* part = tmp.f((size_t)B * (C / 32) * T * 2);
    if (!kx || !km || !ko || !part) return set_error(LDS_ENOMEM, "alloc");
    HIP_TRY(launch_to_k4p(x, kx, B, C, T, C, 0, st));
    HIP_TRY(tap_fill(ko, (size_t)B * Co * (T + 2), st));
    DOpt o1;
    o1.lnpart_out = (float2*)part;
    LDS_TRY(run_dconv(W1, kx, C, nullptr, 0, T, o1, km, B, st));
    DOpt o2;
    o2.ln_part = (const float2*)part; o2.ln_np = C / 32; o2.ln_eps = eps; o2.ln_c1 = c1; o2.ln_c2 = c2;
    LDS_TRY(run_dconv(W2, km, C, nullptr, 0, T, o2, ko, B, st));
    HIP_TRY(tap_take(ko, (size_t)B * Co * (T + 2), st));
    HIP_TRY(launch_from_k4p(km, mid, B, C, T, st));
    HIP_TRY(launch_from_k4p(ko, out, B, Co, T, st));
    HIP_TRY(hipStreamSynchronize(st));
    return LDS_OK;
}

// One residual step of a vocoder ResBlock1 on the K4P / LDS-DMA path (reference models.py:186-192):
//   out = c2(lrelu(c1(lrelu(x)))) + x,  c1: k taps with dilation d, c2: k taps with dilation 1, slope 0.1;
// x plain [B,C,T] -> K4P raw + LeakyReLU'd copies (32 pad frames) -> c1 (activated output) -> c2 (+ residual).  mode 0: plain
// output; 1: raw K4P output and its LeakyReLU'd twin (returned as out / out_act, converted back); 2: running-sum epilogue
// out = (acc + y) / div with `acc` = a plain tensor converted to K4P.
extern "C" int lds_test_voc_step(const float* x, const float* w1, const float* b1, const float* w2, const float* b2, int C, int T, int K, int dil, int mode,
                                 const float* acc, float div, float* out, float* out_act, int B, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!x || !w1 || !w2 || !out || C % 64 || (K != 3 && K != 7 && K != 11)) return set_error(LDS_EINVAL, "bad argument");
    Owner own;
    TmpDev tmp;
    ConvW W1, W2;
    if (!pack_conv(own, w1, b1, C, C, K, W1) || !pack_conv(own, w2, b2, C, C, K, W2)) return set_error(LDS_ENOMEM, "upload failed");
    const int P = kVocPad;
    const size_t n = (size_t)B * C * (T + 2 * P) + 4096;
    float *raw = tmp.f(n), *act = tmp.f(n), *mid = tmp.f(n), *o_raw = tmp.f(n), *o_act = tmp.f(n), *kacc = tmp.f(n);
    if (!raw || !act || !mid || !o_raw || !o_act || !kacc) return set_error(LDS_ENOMEM, "alloc");
    HIP_TRY(hipMemsetAsync(mid, 0xff, n * sizeof(float), st));      // NaN fill: pads must be zeroed explicitly, real frames written
    HIP_TRY(hipMemsetAsync(act, 0xff, n * sizeof(float), st));
    HIP_TRY(launch_to_k4p_act(x, raw, act, 0.1f, B, C, T, P, st));
    HIP_TRY(launch_k4p_zero_pads(act, B, C, T, P, st));
    HIP_TRY(launch_k4p_zero_pads(mid, B, C, T, P, st));
    DOpt o1;
    o1.voc = 1; o1.xpad = P; o1.opad = P; o1.dil = dil; o1.pad = (K * dil - dil) / 2; o1.act_slope = 0.1f;
    LDS_TRY(run_dconv(W1, act, C, nullptr, 0, T, o1, mid, B, st));
    DOpt o2;
    o2.voc = 1; o2.xpad = P; o2.opad = P; o2.pad = (K - 1) / 2; o2.res = raw;
    if (mode == 0) {
        o2.out_plain = 1;
        LDS_TRY(run_dconv(W2, mid, C, nullptr, 0, T, o2, out, B, st));
    } else if (mode == 1) {
        o2.out_act = o_act; o2.act_slope = 0.1f;
        LDS_TRY(run_dconv(W2, mid, C, nullptr, 0, T, o2, o_raw, B, st));
        // K4P (pad 32) -> plain: reuse to_k4p's inverse through a pad-aware copy
        HIP_TRY(launch_from_k4p_pad(o_raw, out, B, C, T, P, st));
        if (out_act) HIP_TRY(launch_from_k4p_pad(o_act, out_act, B, C, T, P, st));
    } else {
        if (!acc) return set_error(LDS_EINVAL, "mode 2 needs acc");
        HIP_TRY(launch_to_k4p_act(acc, kacc, nullptr, 0.f, B, C, T, P, st));
        o2.acc_in = kacc; o2.out_div = div; o2.out_plain = 1;
        LDS_TRY(run_dconv(W2, mid, C, nullptr, 0, T, o2, out, B, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    return LDS_OK;
}

static int attention_test_impl(const float* qkv, float* out, int B, int C, int T, int heads, int f16math, void* stream, int tile_batch = 0, const int* lens_host = nullptr);
extern "C" int lds_test_attention_k4p(const float* qkv, float* out, int B, int C, int T, int heads, void* stream) {
    return attention_test_impl(qkv, out, B, C, T, heads, 0, stream);
}
extern "C" int lds_test_attention_f16math(const float* qkv, float* out, int B, int C, int T, int heads, void* stream) {
    return attention_test_impl(qkv, out, B, C, T, heads, 1, stream);
}
extern "C" int lds_test_attention_latency(const float* qkv, float* out, int B, int C, int T, int heads, int f16math, void* stream) {
    return attention_test_impl(qkv, out, B, C, T, heads, f16math, stream, B);      // the latency mode's choice (tile_batch = the actual batch)
}
// ragged batch (include/lds_test.h): lens = host int32 [B], the clips' lengths at the buffer's resolution
extern "C" int lds_test_attention_ragged(const float* qkv, const int* lens, float* out, int B, int C, int T, int heads, int f16math, int latency, void* stream) {
    if (!lens) return set_error(LDS_EINVAL, "lens is null");
    for (int b = 0; b < B; ++b)
        if (lens[b] < 1 || lens[b] > T) return set_error(LDS_EINVAL, "length out of range");
    return attention_test_impl(qkv, out, B, C, T, heads, f16math, stream, latency ? B : 0, lens);
}
static int attention_test_impl(const float* qkv, float* out, int B, int C, int T, int heads, int f16math, void* stream, int tile_batch, const int* lens_host) {
    hipStream_t st = (hipStream_t)stream;
    TmpDev tmp;
    int* dlens = nullptr;
    if (lens_host) {
        dlens = (int*)tmp.f((size_t)B);
        if (!dlens) return set_error(LDS_ENOMEM, "alloc");
        HIP_TRY(hipMemcpyAsync(dlens, lens_host, sizeof(int) * B, hipMemcpyHostToDevice, st));
    }
    float* qkp = tmp.f((size_t)B * 2 * C * T);       // plain [B][2C][T]
    float* vpl = tmp.f((size_t)B * C * T);
    float* vt = tmp.f((size_t)B * C * (T + 3));
    float* kqk = tmp.f((size_t)B * 2 * C * (T + 2));
    float* ko = tmp.f((size_t)B * C * (T + 2));
    if (!qkp || !vpl || !vt || !kqk || !ko) return set_error(LDS_ENOMEM, "alloc");
    for (int b = 0; b < B; ++b) {
        HIP_TRY(hipMemcpyAsync(qkp + (size_t)b * 2 * C * T, qkv + (size_t)b * 3 * C * T, sizeof(float) * 2 * C * T, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemcpyAsync(vpl + (size_t)b * C * T, qkv + (size_t)b * 3 * C * T + (size_t)2 * C * T, sizeof(float) * C * T, hipMemcpyDeviceToDevice, st));
    }
    // ragged: q and k keep whatever the caller put beyond a clip's length; the value rows are zeros there, as the QKV convolution's epilogue
    // writes them (attention_k4p.hip: a masked key's probability is 0, and 0 * V must be 0); the output buffer starts as NaN
    if (lens_host) {
        for (int b = 0; b < B; ++b)
            if (lens_host[b] < T)
                HIP_TRY(hipMemset2DAsync(vpl + (size_t)b * C * T + lens_host[b], sizeof(float) * T, 0, sizeof(float) * (T - lens_host[b]), C, st));
        HIP_TRY(hipMemsetAsync(ko, 0xff, (size_t)B * C * (T + 2) * sizeof(float), st));
    }
    HIP_TRY(launch_to_k4p(qkp, kqk, B, 2 * C, T, 2 * C, 0, st));
    HIP_TRY(launch_plain_to_vt(vpl, vt, B, C, T, C / heads, st));
    HIP_TRY(tap_fill(ko, (size_t)B * C * (T + 2), st));
    if (lens_host && f16math) HIP_TRY(launch_attention_k4p_f16math(kqk, vt, ko, B, C, T, heads, st, tile_batch, dlens));
    else if (f16math) HIP_TRY(launch_attention_k4p_f16math(kqk, vt, ko, B, C, T, heads, st, tile_batch));
    else HIP_TRY(launch_attention_k4p(kqk, vt, ko, B, C, T, heads, st, tile_batch, dlens, 0));
    HIP_TRY(tap_take(ko, (size_t)B * C * (T + 2), st));
    HIP_TRY(launch_from_k4p(ko, out, B, C, T, st));
    HIP_TRY(hipStreamSynchronize(st));
    return LDS_OK;
}

extern "C" int lds_test_conv_transpose(const float* x, const float* w, const float* bias, float* out, int B, int Ci, int Co, int T, int K,
                                       int stride, int pad, float in_slope, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (K % stride || pad != (K - stride + 1) / 2) return set_error(LDS_EINVAL, "unsupported transposed-conv geometry");
    Owner own;
    ConvW W;
    if (!pack_convT(own, w, bias, Ci, Co, K, stride, W)) return set_error(LDS_ENOMEM, "upload failed");
    Src s{x, Ci, nullptr, 0, T};
    ConvOpt o;
    o.pad = W.K - 1; o.phases = stride; o.tpad = pad; o.To = T + 1; o.Tout = (T - 1) * stride - 2 * pad + K; o.Cout = Co;
    if (in_slope != 1.0f) { o.act_in = ACT_LRELU; o.slope = in_slope; }
    int r = run_conv(W, s, o, out, B, st);
    HIP_TRY(hipStreamSynchronize(st));
    return r;
}

extern "C" int lds_test_split_roundtrip(const float* x, float* out, int B, int C, int T, int fmt, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!x || !out || (C & 7) || (fmt != FMT_BF16X3 && fmt != FMT_F16X2)) return set_error(LDS_EINVAL, "bad argument");
    TmpDev tmp;
    float* k = tmp.f((size_t)B * split_floats(fmt, C, T));
    if (!k) return set_error(LDS_ENOMEM, "alloc");
    HIP_TRY(launch_to_k8b3(x, k, B, C, T, C, 0, st, fmt));
    HIP_TRY(launch_from_k8b3(k, out, B, C, T, st, fmt));
    HIP_TRY(hipStreamSynchronize(st));
    return LDS_OK;
}
extern "C" int lds_test_k8b3_roundtrip(const float* x, float* out, int B, int C, int T, void* stream) { return lds_test_split_roundtrip(x, out, B, C, T, FMT_BF16X3, stream); }

extern "C" int lds_test_gn_apply_bf3(const float* x1, const float* x2, int C1, int C2, int T, int groups, float eps, const float* gamma,
                                     const float* beta, const float* scale_shift, int silu, float* out, int B, void* stream) {
    return lds_test_gn_apply_split(x1, x2, C1, C2, T, groups, eps, gamma, beta, scale_shift, silu, out, B, FMT_BF16X3, stream);
}
extern "C" int lds_test_gn_apply_split(const float* x1, const float* x2, int C1, int C2, int T, int groups, float eps, const float* gamma,
                                       const float* beta, const float* scale_shift, int silu, float* out, int B, int fmt, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (fmt != FMT_BF16X3 && fmt != FMT_F16X2) return set_error(LDS_EINVAL, "bad argument");
    Owner own;
    TmpDev tmp;
    const int C = C1 + C2, nT = (T + 31) / 32;
    float* g = up_vec(own, gamma, C);
    float* be = up_vec(own, beta, C);
    float* k1 = tmp.f((size_t)B * split_floats(fmt, C1, T));
    float* k2 = C2 ? tmp.f((size_t)B * split_floats(fmt, C2, T)) : nullptr;
    float* ky = tmp.f((size_t)B * split_floats(fmt, C, T));
    float* p1 = tmp.f((size_t)B * (C1 / 16) * nT * 2);
    float* p2 = C2 ? tmp.f((size_t)B * (C2 / 16) * nT * 2) : nullptr;
    if (!g || !be || !k1 || (C2 && (!k2 || !p2)) || !ky || !p1) return set_error(LDS_ENOMEM, "alloc");
    HIP_TRY(launch_to_k8b3(x1, k1, B, C1, T, C1, 0, st, fmt));
    HIP_TRY(launch_gn_partials_bf3(k1, C1, T, (float2*)p1, B, st, fmt));
    if (C2) {
        HIP_TRY(launch_to_k8b3(x2, k2, B, C2, T, C2, 0, st, fmt));
        HIP_TRY(launch_gn_partials_bf3(k2, C2, T, (float2*)p2, B, st, fmt));
    }
    HIP_TRY(launch_gn_stream_bf3(k1, k2, C1, C2, T, groups, eps, g, be, scale_shift, 2 * C, 0, silu, (const float2*)p1, (const float2*)p2, ky, B, st, fmt));
    HIP_TRY(launch_from_k8b3(ky, out, B, C, T, st, fmt));
    HIP_TRY(hipStreamSynchronize(st));
    return LDS_OK;
}

extern "C" int lds_debug_set_touch_weights(int on) {
    g_touch_w.store(on ? 1 : 0);
    return LDS_OK;
}
extern "C" int lds_debug_set_voc_pair(int on) {
    g_voc_pair.store(on ? 1 : 0);
    return LDS_OK;
}
// One residual step of a narrow-stage ResBlock1 through the fused kernel: x dev [B][C][T], weights host [C][C][K] / [C]; acc dev or null (then
// out = step(x)), lengths host int32 [B] or null; out dev [B][C][T] (must not alias x).
extern "C" int lds_test_voc_pair(const float* x, const float* w1, const float* b1, const float* w2, const float* b2, int C, int T, int K, int dil,
                                 const float* acc, float div, const int32_t* lengths, float* out, int B, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!x || !w1 || !w2 || !out || !voc_pair_applies(C, K, dil) || B < 1 || B > 64) return set_error(LDS_EINVAL, "bad argument");
    Owner own;
    TmpDev tmp;
    ConvW W1, W2;
    if (!pack_conv(own, w1, b1, C, C, K, W1) || !pack_conv(own, w2, b2, C, C, K, W2)) return set_error(LDS_ENOMEM, "upload failed");
    int* vl = nullptr;
    if (lengths) {
        vl = (int*)tmp.f(64);
        if (!vl) return set_error(LDS_ENOMEM, "alloc");
        float t4[64];
        memcpy(t4, lengths, sizeof(int) * B);
        HIP_TRY(launch_set_list((float*)vl, t4, B, st));
    }
    if (acc) HIP_TRY(hipMemcpyAsync(out, acc, sizeof(float) * (size_t)B * C * T, hipMemcpyDeviceToDevice, st));
    LDS_TRY(run_voc_pair(W1, W2, x, out, C, T, dil, acc != nullptr, div, vl, B, st));
    HIP_TRY(hipStreamSynchronize(st));
    return LDS_OK;
}
// The encoder's convolution alone: x dev [B][Ci][T], w host [Co][Ci][K], b host [Co] or null; out dev [B][Co][To], To = (T + 2 pad - K) / stride + 1
// with pad = (K - stride + 1) / 2 (the reference's downsampler padding; 3 for k 7, stride 1), LeakyReLU(slope) on the input (1 = none);
// tile 0 = the product path's choice, else forced (kernels.h ConvDownArgs::tile); cfg_out (or null) = the configuration that ran
static int conv_down_test_impl(const float* x, const float* w, const float* b, int Ci, int Co, int K, int stride, int T, int B, float slope,
                               const int32_t* lengths_in, const int32_t* lengths_out, int tile, float* out, char* cfg_out, size_t cfg_cap, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!x || !w || !out || Ci < 1 || Co < 1 || K < stride || stride < 1 || T < 1 || B < 1 || B > 65535 || T % stride) return set_error(LDS_EINVAL, "bad argument");
    const int pad = (K - stride + 1) / 2, To = (T + 2 * pad - K) / stride + 1;
    const int32_t* src[2] = {lengths_in, lengths_out};
    const int lim[2] = {T, To};
    for (int i = 0; i < 2 && lengths_in; ++i)
        for (int e = 0; e < B; ++e)
            if (src[i][e] < 0 || src[i][e] > lim[i]) return set_error(LDS_EINVAL, "lengths_%s[%d] = %d outside 0 .. %d", i ? "out" : "in", e, src[i][e], lim[i]);
    Owner own;
    TmpDev tmp;
    DownW d;
    d.w = own.upload(std::vector<float>(w, w + (size_t)Co * Ci * K));
    if (b) d.bias = own.upload(std::vector<float>(b, b + Co));
    if (!d.w || (b && !d.bias)) return set_error(LDS_ENOMEM, "upload failed");
    d.Co = Co; d.Ci = Ci; d.K = K; d.stride = stride; d.pad = pad;
    int* vl[2] = {nullptr, nullptr};
    for (int i = 0; i < 2 && lengths_in; ++i) {
        float t4[64];
        memcpy(t4, src[i], sizeof(int) * B);
        vl[i] = (int*)tmp.f(64);
        if (!vl[i]) return set_error(LDS_ENOMEM, "alloc");
        HIP_TRY(launch_set_list((float*)vl[i], t4, B, st));
    }
    LDS_TRY(run_down(d, x, T, slope, out, B, st, tile, vl[0], vl[1]));
    if (cfg_out && cfg_cap) snprintf(cfg_out, cfg_cap, "%s", conv_down_last_config());
    HIP_TRY(hipStreamSynchronize(st));
    return LDS_OK;
}
extern "C" int lds_test_conv_down(const float* x, const float* w, const float* b, int Ci, int Co, int K, int stride, int T, int B, float slope,
                                  int tile, float* out, char* cfg_out, size_t cfg_cap, void* stream) {
    return conv_down_test_impl(x, w, b, Ci, Co, K, stride, T, B, slope, nullptr, nullptr, tile, out, cfg_out, cfg_cap, stream);
}
// ... in a ragged batch: lengths_in / lengths_out host int32 [B] (B <= 64) = every element's valid input frames (0 .. T) and output frames
// (0 .. To) (kernels.h ConvDownArgs::vlen_in / vlen)
extern "C" int lds_test_conv_down_ragged(const float* x, const float* w, const float* b, int Ci, int Co, int K, int stride, int T, int B, float slope,
                                         const int32_t* lengths_in, const int32_t* lengths_out, int tile, float* out, char* cfg_out, size_t cfg_cap,
                                         void* stream) {
    if (!lengths_in || !lengths_out || B < 1 || B > 64) return set_error(LDS_EINVAL, "bad argument: lengths_in / lengths_out null or B %d outside 1 .. 64", B);
    return conv_down_test_impl(x, w, b, Ci, Co, K, stride, T, B, slope, lengths_in, lengths_out, tile, out, cfg_out, cfg_cap, stream);
}
extern "C" int lds_debug_set_gn_fold(int on) {
    g_gn_fold.store(on ? 1 : 0);
    return LDS_OK;
}
extern "C" int lds_debug_set_split_rule(int rule) {
    conv_bf3_set_debug_rule(rule);
    return LDS_OK;
}

// ---- conv_dma / conv_bf3 modes that only whole-model runs reach otherwise (tests/test_gpu_conv_modes.py) ----
// host int32 lengths [B] -> a device copy (B <= 64), as the ragged drivers carry them
static int test_upload_lens(TmpDev& tmp, const int32_t* host, int B, int*& dev, hipStream_t st) {
    dev = nullptr;
    if (!host) return LDS_OK;
    if (B < 1 || B > 64) return set_error(LDS_EINVAL, "per-utterance lengths: 1 .. 64 batch elements (got %d)", B);
    dev = (int*)tmp.f(64);
    if (!dev) return set_error(LDS_ENOMEM, "alloc");
    float t4[64];
    memcpy(t4, host, sizeof(int) * B);
    HIP_TRY(launch_set_list((float*)dev, t4, B, st));
    return LDS_OK;
}
struct TestActs {      // plain <-> the activation layout of a kernel family (fmt -1: K4P; 0 / 1: split planes)
    int fmt, B; hipStream_t st;
    size_t floats(int C, int T) const { return fmt < 0 ? (size_t)B * C * (T + 2) : (size_t)B * split_floats(fmt, C, T); }
    hipError_t to(const float* src, float* dst, int C, int T) const { return fmt < 0 ? launch_to_k4p(src, dst, B, C, T, C, 0, st) : launch_to_k8b3(src, dst, B, C, T, C, 0, st, fmt); }
    hipError_t from(const float* src, float* dst, int C, int T) const { return fmt < 0 ? launch_from_k4p(src, dst, B, C, T, st) : launch_from_k8b3(src, dst, B, C, T, st, fmt); }
};

// The fused resnet tail alone (run_resnet -> run_dconv_pair[_bf3]): out = conv_k3(h; w3) + conv_1x1([x1 ; x2]; w1) + b3 + b1 with the epilogue's
// GroupNorm partials.  No fused variant for the shapes is an error: the two-launch fallback is never run here.
extern "C" int lds_test_dconv_pair(const float* h, const float* x1, const float* x2, const float* w3, const float* b3, const float* w1, const float* b1, int B,
                                   int Cm, int C1, int C2, int Co, int T, const int32_t* lengths, int lvl, int tile_batch, int fmt, float* out, float* gnpart,
                                   char* cfg_out, size_t cfg_cap, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!h || !x1 || (C2 > 0) != (x2 != nullptr) || !w3 || !b3 || !w1 || !b1 || !out || !gnpart || B < 1 || T < 1 || Cm < 8 || C1 < 8 || C2 < 0 || (Cm & 7) || (C1 & 7) ||
        (C2 & 7) || Co < 32 || Co % 32 || lvl < 0 || tile_batch < 0 || (fmt != -1 && fmt != FMT_BF16X3 && fmt != FMT_F16X2))
        return set_error(LDS_EINVAL, "bad argument");
    const bool f32 = fmt < 0;
    Owner own;
    TmpDev tmp;
    ConvW W3, W1;
    if (!pack_conv(own, w3, nullptr, Co, Cm, 3, W3) || !pack_conv(own, w1, nullptr, Co, C1 + C2, 1, W1)) return set_error(LDS_ENOMEM, "upload failed");
    if (!f32 && !make_split_twin_pair(own, W3, W1, fmt)) return set_error(LDS_ENOMEM, "upload failed");
    std::vector<float> bp(W3.Mp, 0.f);
    for (int co = 0; co < Co; ++co) bp[co] = b3[co] + b1[co];
    float* bias_pair = own.upload(bp);
    if (!bias_pair) return set_error(LDS_ENOMEM, "upload failed");
    int* lens = nullptr;
    LDS_TRY(test_upload_lens(tmp, lengths, B, lens, st));
    const TestActs act{fmt, B, st};
    const int nT = (T + 31) / 32;
    float* kh = tmp.f(act.floats(Cm, T));
    float* k1 = tmp.f(act.floats(C1, T));
    float* k2 = C2 ? tmp.f(act.floats(C2, T)) : nullptr;
    float* ko = tmp.f(act.floats(Co, T));
    float* kpart = tile_batch ? tmp.f((size_t)kClusterPartFloats) : nullptr;
    unsigned* kcount = tile_batch ? (unsigned*)tmp.f(kClusterCounters) : nullptr;
    if (!kh || !k1 || (C2 && !k2) || !ko || (tile_batch && (!kpart || !kcount))) return set_error(LDS_ENOMEM, "alloc");
    if (kcount) HIP_TRY(hipMemsetAsync(kcount, 0, sizeof(unsigned) * kClusterCounters, st));
    HIP_TRY(hipMemsetAsync(ko, 0xff, sizeof(float) * act.floats(Co, T), st));                        // NaN fill: every frame and every partial must be written
    HIP_TRY(hipMemsetAsync(gnpart, 0xff, sizeof(float) * (size_t)B * (Co / 16) * nT * 2, st));
    HIP_TRY(act.to(h, kh, Cm, T));
    HIP_TRY(act.to(x1, k1, C1, T));
    if (C2) HIP_TRY(act.to(x2, k2, C2, T));
    int rc;
    {
        LensScope ls(lens);
        TileBatchScope tbs(tile_batch, kpart, kcount);
        rc = f32 ? run_dconv_pair(W3, kh, W1, k1, C1, k2, C2, T, bias_pair, (float2*)gnpart, ko, B, st, lvl)
                 : run_dconv_pair_bf3(W3, kh, W1, k1, C1, k2, C2, T, bias_pair, (float2*)gnpart, ko, B, st, fmt, lvl);
    }
    if (rc == 1) rc = set_error(LDS_EINVAL, "dconv pair: no fused variant for Cm %d C1 %d C2 %d Co %d T %d (fmt %d, tile_batch %d)", Cm, C1, C2, Co, T, fmt, tile_batch);
    if (rc == LDS_OK) {
        if (cfg_out && cfg_cap) snprintf(cfg_out, cfg_cap, "%s", f32 ? conv_dma_last_config() : conv_bf3_last_config());
        if (f32) HIP_TRY(tap_take(ko, act.floats(Co, T), st));
        HIP_TRY(act.from(ko, out, Co, T));
    }
    HIP_TRY(hipStreamSynchronize(st));
    return rc;
}

// lds_test_dconv with the modes of the encoders and the ragged drivers (include/lds_test.h lds_dconv_ex_test)
extern "C" int lds_test_dconv_ex(const lds_dconv_ex_test* a, float* out, float* gnpart, int B, char* cfg_out, size_t cfg_cap, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!a || !a->x1 || !a->w || !out || B < 1 || a->T < 1 || (a->C2 > 0) != (a->x2 != nullptr) || a->C1 < 8 || (a->C1 & 7) || a->C2 < 0 || (a->C2 & 7) || a->Co < 32 ||
        a->Co % 32 || a->K < 1 || a->stride < 1 || a->pad < 0 || (a->epilogue != EPI_NONE && a->epilogue != EPI_GELU && a->epilogue != EPI_GEGLU) || a->lvl_in < 0 ||
        a->lvl_out < 0 || a->tile_batch < 0 || (a->fmt != -1 && a->fmt != FMT_BF16X3 && a->fmt != FMT_F16X2) || (a->ln_gamma != nullptr) != (a->ln_beta != nullptr) ||
        a->v_split < 0 || a->v_split == 1 || a->cfg < 0)
        return set_error(LDS_EINVAL, "bad argument");
    const bool f32 = a->fmt < 0, ln = a->ln_gamma != nullptr, geglu = a->epilogue == EPI_GEGLU;
    // the transformer's two folded projections as the UNet runs them: FF1 (GEGLU rows interleaved as pack_geglu does) and QKV (value third in VT layout)
    if (geglu && (!ln || !f32 || a->Co % 128 || a->res || gnpart || a->v_split)) return set_error(LDS_EINVAL, "GEGLU here is the folded FF1: fp32, LayerNorm fold, Co a multiple of 128");
    if (a->v_split && (!f32 || a->Co % 3 || (a->Co / 3) % a->v_split || ((a->Co / 3) * 2) % 8 || a->res || gnpart || a->K != 1 || a->stride != 1))
        return set_error(LDS_EINVAL, "v_split is the fp32 QKV projection: 1x1, Co = 3 C, C a multiple of the head dim");
    const int mode = f32 ? 0 : a->fmt + 1;
    const int Ci = a->C1 + a->C2, T = a->T;
    const int To = (T + 2 * a->pad - (a->K - 1) - 1) / a->stride + 1;
    if (To < 1) return set_error(LDS_EINVAL, "bad argument: no output frame");
    if (ln && (a->K != 1 || a->C2 || Ci % 32)) return set_error(LDS_EINVAL, "the LayerNorm fold takes a 1x1 convolution over one source of a multiple of 32 channels");
    Owner own;
    TmpDev tmp;
    ConvW W, Wid;
    float *c1 = nullptr, *c2 = nullptr;
    std::vector<int> perm;
    if (geglu) {
        perm.resize(a->Co);
        for (int mm = 0; mm < a->Co; ++mm) perm[mm] = ((mm % 64) / 32 == 0 ? 0 : a->Co / 2) + 32 * (mm / 64) + mm % 32;
    }
    bool ok = ln ? pack_ln_fold(own, a->w, a->bias, a->ln_gamma, a->ln_beta, a->Co, Ci, perm, W, c1, c2) : pack_conv(own, a->w, a->bias, a->Co, Ci, a->K, W);
    if (ok && ln) {      // the partials' producer: an identity 1x1 convolution, whose epilogue writes the per-frame LayerNorm partials of x itself
        std::vector<float> eye((size_t)Ci * Ci, 0.f);
        for (int c = 0; c < Ci; ++c) eye[(size_t)c * Ci + c] = 1.0f;
        ok = pack_conv(own, eye.data(), nullptr, Ci, Ci, 1, Wid);
    }
    if (ok && !f32) ok = make_split_twin(own, W, a->fmt) && (!ln || make_split_twin(own, Wid, a->fmt));
    if (!ok) return set_error(LDS_ENOMEM, "test dconv: upload failed");
    int* lens = nullptr;
    LDS_TRY(test_upload_lens(tmp, a->lengths, B, lens, st));
    const TestActs act{a->fmt, B, st};
    float* k1 = tmp.f(act.floats(a->C1, T));
    float* k2 = a->C2 ? tmp.f(act.floats(a->C2, T)) : nullptr;
    float* kx = ln ? tmp.f(act.floats(Ci, T)) : nullptr;
    float* part = ln ? tmp.f((size_t)B * (Ci / 32) * T * 2) : nullptr;
    float* kres = a->res ? tmp.f(act.floats(a->Co, To)) : nullptr;
    const int Cout = geglu ? a->Co / 2 : a->Co, Ck = a->v_split ? (Cout / 3) * 2 : Cout, To4 = (To + 3) & ~3;      // (K4P channels; the rest is the VT third)
    float* ko = tmp.f(act.floats(Ck, To));
    float* vout = a->v_split ? tmp.f((size_t)B * (Cout - Ck) * To4) : nullptr;
    float* kpart = a->tile_batch ? tmp.f((size_t)kClusterPartFloats) : nullptr;
    unsigned* kcount = a->tile_batch ? (unsigned*)tmp.f(kClusterCounters) : nullptr;
    if (!k1 || (a->C2 && !k2) || (ln && (!kx || !part)) || (a->res && !kres) || !ko || (a->v_split && !vout) || (a->tile_batch && (!kpart || !kcount))) return set_error(LDS_ENOMEM, "alloc");
    if (kcount) HIP_TRY(hipMemsetAsync(kcount, 0, sizeof(unsigned) * kClusterCounters, st));
    HIP_TRY(hipMemsetAsync(ko, 0xff, sizeof(float) * act.floats(Ck, To), st));      // NaN fill: every frame and every partial must be written
    if (vout) HIP_TRY(hipMemsetAsync(vout, 0xff, sizeof(float) * (size_t)B * (Cout - Ck) * To4, st));      // (the VT tail too)
    if (gnpart) HIP_TRY(hipMemsetAsync(gnpart, 0xff, sizeof(float) * (size_t)B * (a->Co / 16) * ((To + 31) / 32) * 2, st));
    HIP_TRY(act.to(a->x1, k1, a->C1, T));
    if (a->C2) HIP_TRY(act.to(a->x2, k2, a->C2, T));
    if (a->res) HIP_TRY(act.to(a->res, kres, a->Co, To));
    int rc = LDS_OK;
    {
        LensScope ls(lens);
        const float* xin = k1;
        if (ln) {
            DOpt oi;
            oi.lvl_in = oi.lvl_out = a->lvl_in;
            oi.lnpart_out = (float2*)part;
            rc = dconv_any(mode, Wid, k1, Ci, nullptr, 0, T, oi, kx, B, st);
            xin = kx;
        }
        if (rc == LDS_OK) {
            TileBatchScope tbs(a->tile_batch, kpart, kcount);
            DOpt o;
            o.stride = a->stride; o.pad = a->pad; o.epi = a->epilogue; o.res = kres; o.cfg = a->cfg;
            o.lvl_in = a->lvl_in; o.lvl_out = a->lvl_out;
            if (a->v_split) { o.plain_from = Ck; o.out2 = vout; o.vt_D = a->v_split; }
            o.gnpart_out = (float2*)gnpart;
            if (ln) { o.ln_part = (const float2*)part; o.ln_np = Ci / 32; o.ln_eps = a->ln_eps; o.ln_c1 = c1; o.ln_c2 = c2; }
            rc = dconv_any(mode, W, xin, a->C1, k2, a->C2, T, o, ko, B, st);
        }
    }
    if (rc == LDS_OK) {
        if (cfg_out && cfg_cap) snprintf(cfg_out, cfg_cap, "%s", f32 ? conv_dma_last_config() : conv_bf3_last_config());
        if (f32) HIP_TRY(tap_take(ko, act.floats(Ck, To), st));
        HIP_TRY(act.from(ko, out, Ck, To));      // out = [B][Ck][To], then (v_split) the raw VT buffer [B][(Cout - Ck) / D][ceil4(To) / 4][D][4]
        if (vout) HIP_TRY(hipMemcpyAsync(out + (size_t)B * Ck * To, vout, sizeof(float) * (size_t)B * (Cout - Ck) * To4, hipMemcpyDeviceToDevice, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    return rc;
}

// ---- conv_wino (include/lds_test.h) ----
extern "C" int lds_test_wino_pack(const float* g, int Co, int Ci, float* U) {
    if (!g || !U || Co < 1 || Ci < 1) return set_error(LDS_EINVAL, "bad argument");
    std::vector<float> u;
    wino_taps(g, Co, Ci, u);
    memcpy(U, u.data(), u.size() * sizeof(float));
    return LDS_OK;
}
struct lds_wino_test {      // (the entries' arguments, gathered)
    const float *x1, *x2; int C1, C2, T;
    const float *gamma, *beta, *scale_shift; int groups, silu;
    const float *w, *bias; int Co;
    const float* res; const int32_t* lengths; int poison, cfg;
    int lvl;      // `lengths` are level-0 lengths and T is the tensor's length at this level (run_resnet's lvl)
};
// the device state both entries share: packed weights, K4P sources with their partials, residual, the planes / K4P scratch, the output
struct WinoTestState {
    Owner own; TmpDev tmp; ConvW W;
    float *gamma = nullptr, *beta = nullptr, *k1 = nullptr, *k2 = nullptr, *kres = nullptr, *planes = nullptr, *ko = nullptr;
    float2 *gp1 = nullptr, *gp2 = nullptr;
    int *lens = nullptr, *lens_lvl = nullptr;      // the level-0 lengths the kernels receive; the same reduced to the level, for the staging
    int Ci = 0, P = 0;
    size_t plane_floats = 0, out_floats = 0;
};
static int wino_test_setup(const lds_wino_test* a, int B, hipStream_t st, WinoTestState& s) {
    if (!a || !a->x1 || !a->w || !a->gamma || !a->beta || B < 1 || a->T < 1 || (a->C2 > 0) != (a->x2 != nullptr) || a->C1 < 16 || (a->C1 & 15) || a->C2 < 0 || (a->C2 & 15) ||
        a->Co < 16 || (a->Co & 15) || a->groups < 1 || (a->C1 + a->C2) % a->groups || ((a->C1 + a->C2) / a->groups) % 16 || a->cfg < 0 || a->lvl < 0 || a->lvl > 30)
        return set_error(LDS_EINVAL, "bad argument");
    const int Ci = a->C1 + a->C2, T = a->T, nT = (T + 31) / 32;
    s.Ci = Ci; s.P = (T + 1) / 2;
    int32_t reduced[64];      // the lengths at level lvl, as the kernels reduce them: (n - 1) / 2 + 1 per level
    for (int b = 0; b < B && b < 64 && a->lengths; ++b) {
        int n = a->lengths[b];
        for (int i = 0; i < a->lvl && n >= 1; ++i) n = (n - 1) / 2 + 1;
        if (n < 1 || n > T) return set_error(LDS_EINVAL, "lengths[%d] = %d (%d at level %d) outside 1 .. %d", b, a->lengths[b], n, a->lvl, T);
        reduced[b] = n;
    }
    if (!pack_conv(s.own, a->w, a->bias, a->Co, Ci, 3, s.W) || !pack_wino(s.own, a->w, a->Co, Ci, s.W)) return set_error(LDS_ENOMEM, "upload failed");
    s.gamma = up_vec(s.own, a->gamma, Ci); s.beta = up_vec(s.own, a->beta, Ci);
    LDS_TRY(test_upload_lens(s.tmp, a->lengths, B, s.lens, st));
    LDS_TRY(test_upload_lens(s.tmp, a->lengths ? reduced : nullptr, B, s.lens_lvl, st));
    s.plane_floats = (size_t)B * Ci * 4 * s.P; s.out_floats = (size_t)B * a->Co * (T + 2);
    s.k1 = s.tmp.f((size_t)B * a->C1 * (T + 2));
    s.k2 = a->C2 ? s.tmp.f((size_t)B * a->C2 * (T + 2)) : nullptr;
    s.gp1 = (float2*)s.tmp.f((size_t)B * (a->C1 / 16) * nT * 2);
    s.gp2 = a->C2 ? (float2*)s.tmp.f((size_t)B * (a->C2 / 16) * nT * 2) : nullptr;
    s.kres = a->res ? s.tmp.f(s.out_floats) : nullptr;
    s.planes = s.tmp.f(std::max(s.plane_floats, (size_t)B * Ci * (T + 2)));      // (the direct path's K4P tensor in lds_bench_wino)
    s.ko = s.tmp.f(s.out_floats);
    if (!s.gamma || !s.beta || !s.k1 || (a->C2 && (!s.k2 || !s.gp2)) || !s.gp1 || (a->res && !s.kres) || !s.planes || !s.ko) return set_error(LDS_ENOMEM, "alloc");
    HIP_TRY(hipMemsetAsync(s.gp1, 0xff, sizeof(float2) * (size_t)B * (a->C1 / 16) * nT, st));      // (NaN: a partial beyond a length is never read)
    if (a->C2) HIP_TRY(hipMemsetAsync(s.gp2, 0xff, sizeof(float2) * (size_t)B * (a->C2 / 16) * nT, st));
    HIP_TRY(launch_to_k4p(a->x1, s.k1, B, a->C1, T, a->C1, 0, st, s.lens_lvl));
    if (a->C2) HIP_TRY(launch_to_k4p(a->x2, s.k2, B, a->C2, T, a->C2, 0, st, s.lens_lvl));
    if (a->res) HIP_TRY(launch_to_k4p(a->res, s.kres, B, a->Co, T, a->Co, 0, st, s.lens_lvl));
    if (a->poison) {      // NaN / Inf in the sources' pad frames and beyond the lengths: nothing of it may reach a plane
        HIP_TRY(launch_k4p_poison(s.k1, B, a->C1, T, s.lens_lvl, st));
        if (a->C2) HIP_TRY(launch_k4p_poison(s.k2, B, a->C2, T, s.lens_lvl, st));
    }
    HIP_TRY(launch_gn_partials(s.k1, a->C1, T, s.gp1, B, st, s.lens_lvl, 0));
    if (a->C2) HIP_TRY(launch_gn_partials(s.k2, a->C2, T, s.gp2, B, st, s.lens_lvl, 0));
    return LDS_OK;
}
static int wino_test_run(const lds_wino_test* a, WinoTestState& s, float2* gnpart, int B, hipStream_t st) {
    HIP_TRY(launch_gn_wino(s.k1, s.k2, a->C1, a->C2, a->T, a->groups, 1e-5f, s.gamma, s.beta, a->scale_shift, 2 * s.Ci, 0, a->silu, s.gp1, s.gp2, s.planes, B, st, s.lens, a->lvl));
    return run_wconv(s.W, s.planes, a->T, s.kres, gnpart, s.ko, B, st, a->lvl, a->cfg);
}
static int wino_conv_test(const lds_wino_test* a, float* out, float* vplanes, float* gnpart, int B, hipStream_t st) {
    if (!out) return set_error(LDS_EINVAL, "bad argument");
    WinoTestState s;
    LDS_TRY(wino_test_setup(a, B, st, s));
    // NaN fill: every plane entry, every output frame (pads included) and every partial of a block inside a length must be written
    HIP_TRY(hipMemsetAsync(s.planes, 0xff, sizeof(float) * s.plane_floats, st));
    HIP_TRY(hipMemsetAsync(s.ko, 0xff, sizeof(float) * s.out_floats, st));
    if (gnpart) HIP_TRY(hipMemsetAsync(gnpart, 0xff, sizeof(float) * (size_t)B * (a->Co / 16) * ((a->T + 31) / 32) * 2, st));
    int rc;
    {
        LensScope ls(s.lens);
        rc = wino_test_run(a, s, (float2*)gnpart, B, st);
    }
    if (rc == LDS_OK) {
        HIP_TRY(tap_take(s.ko, s.out_floats, st));
        HIP_TRY(launch_from_k4p(s.ko, out, B, a->Co, a->T, st));
        if (vplanes) HIP_TRY(hipMemcpyAsync(vplanes, s.planes, sizeof(float) * s.plane_floats, hipMemcpyDeviceToDevice, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    return rc;
}
extern "C" int lds_test_wino_conv(const float* x1, const float* x2, int C1, int C2, int T, const float* gamma, const float* beta, const float* scale_shift,
                                  int groups, int silu, const float* w, const float* bias, int Co, const float* res, const int32_t* lengths, int poison, int cfg,
                                  float* out, float* vplanes, float* gnpart, int B, void* stream) {
    const lds_wino_test args{x1, x2, C1, C2, T, gamma, beta, scale_shift, groups, silu, w, bias, Co, res, lengths, poison, cfg, 0};
    return wino_conv_test(&args, out, vplanes, gnpart, B, (hipStream_t)stream);
}
extern "C" int lds_test_wino_conv_lvl(const float* x1, const float* x2, int C1, int C2, int T, const float* gamma, const float* beta, const float* scale_shift,
                                      int groups, int silu, const float* w, const float* bias, int Co, const float* res, const int32_t* lengths, int poison, int cfg,
                                      int lvl, float* out, float* vplanes, float* gnpart, int B, void* stream) {
    const lds_wino_test args{x1, x2, C1, C2, T, gamma, beta, scale_shift, groups, silu, w, bias, Co, res, lengths, poison, cfg, lvl};
    return wino_conv_test(&args, out, vplanes, gnpart, B, (hipStream_t)stream);
}
extern "C" int lds_test_wino_min_T(int Ci, int Co) { return wino_min_T(Ci, Co); }
// direct (gn_stream + conv_dma) against Winograd (gn_wino + conv_wino) on one shape, alternating: `reps` times a block of `iters` direct
// passes, then a block of `iters` Winograd passes, each block between two events on the stream; ms_direct / ms_wino [reps] = a block's time per pass
extern "C" int lds_bench_wino(const float* x1, const float* x2, int C1, int C2, int T, const float* gamma, const float* beta, const float* scale_shift,
                              int groups, int silu, const float* w, const float* bias, int Co, const float* res, int cfg, int B, int iters, int reps,
                              float* ms_direct, float* ms_wino, char* cfg_out, size_t cfg_cap, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!ms_direct || !ms_wino || iters < 1 || reps < 1) return set_error(LDS_EINVAL, "bad argument");
    const lds_wino_test args{x1, x2, C1, C2, T, gamma, beta, scale_shift, groups, silu, w, bias, Co, res, nullptr, 0, cfg, 0};
    const lds_wino_test* a = &args;
    WinoTestState s;
    LDS_TRY(wino_test_setup(a, B, st, s));
    float2* gnpart = (float2*)s.tmp.f((size_t)B * (a->Co / 16) * ((a->T + 31) / 32) * 2);
    if (!gnpart) return set_error(LDS_ENOMEM, "alloc");
    DOpt o;
    o.pad = 1; o.res = s.kres; o.gnpart_out = gnpart;
    auto direct = [&]() -> int {
        HIP_TRY(launch_gn_stream(s.k1, s.k2, a->C1, a->C2, a->T, a->groups, 1e-5f, s.gamma, s.beta, a->scale_shift, 2 * s.Ci, 0, a->silu, s.gp1, s.gp2, s.planes, B, st));
        return run_dconv(s.W, s.planes, s.Ci, nullptr, 0, a->T, o, s.ko, B, st);
    };
    LDS_TRY(direct());
    std::string cfgs = std::string("direct ") + conv_dma_last_config();
    LDS_TRY(wino_test_run(a, s, gnpart, B, st));
    cfgs += std::string(" | wino ") + conv_wino_last_config();
    if (cfg_out && cfg_cap) snprintf(cfg_out, cfg_cap, "%s", cfgs.c_str());
    hipEvent_t ev[3];
    for (auto& e : ev) HIP_TRY(hipEventCreate(&e));
    int rc = LDS_OK;
    for (int r = 0; r < reps && rc == LDS_OK; ++r) {
        HIP_TRY(hipEventRecord(ev[0], st));
        for (int i = 0; i < iters && rc == LDS_OK; ++i) rc = direct();
        HIP_TRY(hipEventRecord(ev[1], st));
        for (int i = 0; i < iters && rc == LDS_OK; ++i) rc = wino_test_run(a, s, gnpart, B, st);
        HIP_TRY(hipEventRecord(ev[2], st));
        HIP_TRY(hipEventSynchronize(ev[2]));
        float d = 0.f, w = 0.f;
        HIP_TRY(hipEventElapsedTime(&d, ev[0], ev[1]));
        HIP_TRY(hipEventElapsedTime(&w, ev[1], ev[2]));
        ms_direct[r] = d / iters; ms_wino[r] = w / iters;
    }
    for (auto& e : ev) (void)hipEventDestroy(e);
    HIP_TRY(hipStreamSynchronize(st));
    return rc;
}

// ---- conv2 + shortcut as one conv_wino launch (include/lds_test.h) ----
extern "C" int lds_test_wino_pair_pack(const float* g, const float* S, int Co, int Cm, int Cin, float* U) {
    if (!g || !S || !U || Co < 1 || Cm < 1 || Cin < 2 || (Cin & 1)) return set_error(LDS_EINVAL, "bad argument");
    std::vector<float> u;
    wino_pair_taps(g, S, Co, Cm, Cin, u);
    memcpy(U, u.data(), u.size() * sizeof(float));
    return LDS_OK;
}
extern "C" int lds_test_wino_pair_min_T(int Cin, int Cm) { return wino_pair_min_T(Cin, Cm); }
struct lds_wino_pair_test {      // (the entries' arguments, gathered)
    const float *h, *x1, *x2; int Cm, C1, C2, T;
    const float *gamma1, *beta1, *gamma2, *beta2, *scale_shift; int groups;
    const float *w2, *b2, *ws, *bs;
    const int32_t* lengths; int poison, cfg, lvl;
};
// the tail of a resnet with a shortcut from conv1's GroupNorm pass on (run_resnet): K4P sources with their partials, both weight forms
struct WinoPairTestState {
    Owner own; TmpDev tmp; ConvW W2, Ws;
    float *wu_pair = nullptr, *bias_pair = nullptr, *gamma1 = nullptr, *beta1 = nullptr, *gamma2 = nullptr, *beta2 = nullptr;
    float *kh = nullptr, *k1 = nullptr, *k2 = nullptr, *v1 = nullptr, *wpl = nullptr, *gno = nullptr, *ko = nullptr;
    float2 *gph = nullptr, *gp1 = nullptr, *gp2 = nullptr;
    int *lens = nullptr, *lens_lvl = nullptr;
    int Cin = 0, P = 0;
    size_t v1_floats = 0, wpl_floats = 0, out_floats = 0;
};
static int wino_pair_test_setup(const lds_wino_pair_test* a, int B, hipStream_t st, WinoPairTestState& s) {
    if (!a || !a->h || !a->x1 || !a->w2 || !a->b2 || !a->ws || !a->bs || !a->gamma1 || !a->beta1 || !a->gamma2 || !a->beta2 || B < 1 || B > 64 || a->T < 1 ||
        (a->C2 > 0) != (a->x2 != nullptr) || a->C1 < 16 || (a->C1 & 15) || a->C2 < 0 || (a->C2 & 15) || a->Cm < 16 || (a->Cm & 15) || a->groups < 1 ||
        (a->C1 + a->C2) % a->groups || ((a->C1 + a->C2) / a->groups) % 16 || a->Cm % a->groups || (a->Cm / a->groups) % 16 || a->cfg < 0 || a->lvl < 0 || a->lvl > 30)
        return set_error(LDS_EINVAL, "bad argument");
    const int Cin = a->C1 + a->C2, Cm = a->Cm, T = a->T, nT = (T + 31) / 32;
    s.Cin = Cin; s.P = (T + 1) / 2;
    int32_t reduced[64];
    for (int b = 0; b < B && a->lengths; ++b) {
        int n = a->lengths[b];
        for (int i = 0; i < a->lvl && n >= 1; ++i) n = (n - 1) / 2 + 1;
        if (n < 1 || n > T) return set_error(LDS_EINVAL, "lengths[%d] = %d (%d at level %d) outside 1 .. %d", b, a->lengths[b], n, a->lvl, T);
        reduced[b] = n;
    }
    if (!pack_conv(s.own, a->w2, nullptr, Cm, Cm, 3, s.W2) || !pack_conv(s.own, a->ws, nullptr, Cm, Cin, 1, s.Ws)) return set_error(LDS_ENOMEM, "upload failed");
    s.wu_pair = pack_wino_pair(s.own, a->w2, a->ws, Cm, Cm, Cin, s.W2.Mp);
    std::vector<float> bp(s.W2.Mp, 0.f);
    for (int co = 0; co < Cm; ++co) bp[co] = a->b2[co] + a->bs[co];
    s.bias_pair = s.own.upload(bp);
    s.gamma1 = up_vec(s.own, a->gamma1, Cin); s.beta1 = up_vec(s.own, a->beta1, Cin);
    s.gamma2 = up_vec(s.own, a->gamma2, Cm); s.beta2 = up_vec(s.own, a->beta2, Cm);
    LDS_TRY(test_upload_lens(s.tmp, a->lengths, B, s.lens, st));
    LDS_TRY(test_upload_lens(s.tmp, a->lengths ? reduced : nullptr, B, s.lens_lvl, st));
    s.v1_floats = (size_t)B * Cin * 4 * s.P; s.wpl_floats = (size_t)B * wino_pair_plane_floats(Cin, Cm, T); s.out_floats = (size_t)B * Cm * (T + 2);
    s.kh = s.tmp.f(s.out_floats);
    s.k1 = s.tmp.f((size_t)B * a->C1 * (T + 2));
    s.k2 = a->C2 ? s.tmp.f((size_t)B * a->C2 * (T + 2)) : nullptr;
    s.gph = (float2*)s.tmp.f((size_t)B * (Cm / 16) * nT * 2);
    s.gp1 = (float2*)s.tmp.f((size_t)B * (a->C1 / 16) * nT * 2);
    s.gp2 = a->C2 ? (float2*)s.tmp.f((size_t)B * (a->C2 / 16) * nT * 2) : nullptr;
    s.v1 = s.tmp.f(s.v1_floats);
    s.wpl = s.tmp.f(s.wpl_floats);
    s.gno = s.tmp.f(s.out_floats);      // (the direct path's K4P tensor in lds_bench_wino_pair)
    s.ko = s.tmp.f(s.out_floats);
    if (!s.wu_pair || !s.bias_pair || !s.gamma1 || !s.beta1 || !s.gamma2 || !s.beta2 || !s.kh || !s.k1 || (a->C2 && (!s.k2 || !s.gp2)) || !s.gph || !s.gp1 || !s.v1 ||
        !s.wpl || !s.gno || !s.ko)
        return set_error(LDS_ENOMEM, "alloc");
    HIP_TRY(hipMemsetAsync(s.gph, 0xff, sizeof(float2) * (size_t)B * (Cm / 16) * nT, st));      // (NaN: a partial beyond a length is never read)
    HIP_TRY(hipMemsetAsync(s.gp1, 0xff, sizeof(float2) * (size_t)B * (a->C1 / 16) * nT, st));
    if (a->C2) HIP_TRY(hipMemsetAsync(s.gp2, 0xff, sizeof(float2) * (size_t)B * (a->C2 / 16) * nT, st));
    HIP_TRY(launch_to_k4p(a->h, s.kh, B, Cm, T, Cm, 0, st, s.lens_lvl));
    HIP_TRY(launch_to_k4p(a->x1, s.k1, B, a->C1, T, a->C1, 0, st, s.lens_lvl));
    if (a->C2) HIP_TRY(launch_to_k4p(a->x2, s.k2, B, a->C2, T, a->C2, 0, st, s.lens_lvl));
    if (a->poison) {      // NaN / Inf in the sources' pad frames and beyond the lengths: nothing of it may reach a plane
        HIP_TRY(launch_k4p_poison(s.kh, B, Cm, T, s.lens_lvl, st));
        HIP_TRY(launch_k4p_poison(s.k1, B, a->C1, T, s.lens_lvl, st));
        if (a->C2) HIP_TRY(launch_k4p_poison(s.k2, B, a->C2, T, s.lens_lvl, st));
    }
    HIP_TRY(launch_gn_partials(s.kh, Cm, T, s.gph, B, st, s.lens_lvl, 0));
    HIP_TRY(launch_gn_partials(s.k1, a->C1, T, s.gp1, B, st, s.lens_lvl, 0));
    if (a->C2) HIP_TRY(launch_gn_partials(s.k2, a->C2, T, s.gp2, B, st, s.lens_lvl, 0));
    return LDS_OK;
}
// conv1's pass with the side output, conv2's pass, the pair launch: run_resnet's three launches around conv1
static int wino_pair_test_run(const lds_wino_pair_test* a, WinoPairTestState& s, float2* gnpart, int B, hipStream_t st) {
    const long long stride = (long long)wino_pair_plane_floats(s.Cin, a->Cm, a->T);
    HIP_TRY(launch_gn_wino_pair(s.k1, s.k2, a->C1, a->C2, a->T, a->groups, 1e-5f, s.gamma1, s.beta1, nullptr, 0, 0, 1, s.gp1, s.gp2, s.v1, (long long)s.Cin * 4 * s.P,
                                s.wpl + (size_t)a->Cm * 4 * s.P, stride, B, st, s.lens, a->lvl));
    HIP_TRY(launch_gn_wino_pair(s.kh, nullptr, a->Cm, 0, a->T, a->groups, 1e-5f, s.gamma2, s.beta2, a->scale_shift, 2 * a->Cm, 0, 1, s.gph, nullptr, s.wpl, stride,
                                nullptr, 0, B, st, s.lens, a->lvl));
    return run_wconv_pair(s.wu_pair, s.Cin, a->Cm, s.W2.Mp, s.wpl, a->T, s.bias_pair, gnpart, s.ko, B, st, a->lvl, a->cfg);
}
extern "C" int lds_test_wino_pair(const float* h, const float* x1, const float* x2, int Cm, int C1, int C2, int T, const float* gamma1, const float* beta1,
                                  const float* gamma2, const float* beta2, const float* scale_shift, int groups, const float* w2, const float* b2, const float* ws,
                                  const float* bs, const int32_t* lengths, int poison, int cfg, int lvl, float* out, float* vplanes, float* pplanes, float* gnpart,
                                  int B, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!out) return set_error(LDS_EINVAL, "bad argument");
    const lds_wino_pair_test args{h, x1, x2, Cm, C1, C2, T, gamma1, beta1, gamma2, beta2, scale_shift, groups, w2, b2, ws, bs, lengths, poison, cfg, lvl};
    WinoPairTestState s;
    LDS_TRY(wino_pair_test_setup(&args, B, st, s));
    // NaN fill: every plane entry, every output frame (pads included) and every partial of a block inside a length must be written
    HIP_TRY(hipMemsetAsync(s.v1, 0xff, sizeof(float) * s.v1_floats, st));
    HIP_TRY(hipMemsetAsync(s.wpl, 0xff, sizeof(float) * s.wpl_floats, st));
    HIP_TRY(hipMemsetAsync(s.ko, 0xff, sizeof(float) * s.out_floats, st));
    if (gnpart) HIP_TRY(hipMemsetAsync(gnpart, 0xff, sizeof(float) * (size_t)B * (Cm / 16) * ((T + 31) / 32) * 2, st));
    int rc;
    {
        LensScope ls(s.lens);
        rc = wino_pair_test_run(&args, s, (float2*)gnpart, B, st);
    }
    if (rc == LDS_OK) {
        HIP_TRY(tap_take(s.ko, s.out_floats, st));
        HIP_TRY(launch_from_k4p(s.ko, out, B, Cm, T, st));
        if (vplanes) HIP_TRY(hipMemcpyAsync(vplanes, s.v1, sizeof(float) * s.v1_floats, hipMemcpyDeviceToDevice, st));
        if (pplanes) HIP_TRY(hipMemcpyAsync(pplanes, s.wpl, sizeof(float) * s.wpl_floats, hipMemcpyDeviceToDevice, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    return rc;
}
// the direct tail (gn_wino on the block input, gn_stream, conv_dma_pair) against the new one (wino_pair_test_run) on one shape, alternating as
// lds_bench_wino does: conv1's pass is in both blocks, so the side output's cost is in the comparison
extern "C" int lds_bench_wino_pair(const float* h, const float* x1, const float* x2, int Cm, int C1, int C2, int T, const float* gamma1, const float* beta1,
                                   const float* gamma2, const float* beta2, const float* scale_shift, int groups, const float* w2, const float* b2, const float* ws,
                                   const float* bs, int cfg, int B, int iters, int reps, float* ms_direct, float* ms_wino, char* cfg_out, size_t cfg_cap,
                                   void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!ms_direct || !ms_wino || iters < 1 || reps < 1) return set_error(LDS_EINVAL, "bad argument");
    const lds_wino_pair_test args{h, x1, x2, Cm, C1, C2, T, gamma1, beta1, gamma2, beta2, scale_shift, groups, w2, b2, ws, bs, nullptr, 0, cfg, 0};
    const lds_wino_pair_test* a = &args;
    WinoPairTestState s;
    LDS_TRY(wino_pair_test_setup(a, B, st, s));
    float2* gnpart = (float2*)s.tmp.f((size_t)B * (Cm / 16) * ((T + 31) / 32) * 2);
    if (!gnpart) return set_error(LDS_ENOMEM, "alloc");
    auto direct = [&]() -> int {
        HIP_TRY(launch_gn_wino(s.k1, s.k2, C1, C2, T, groups, 1e-5f, s.gamma1, s.beta1, nullptr, 0, 0, 1, s.gp1, s.gp2, s.v1, B, st));
        HIP_TRY(launch_gn_stream(s.kh, nullptr, Cm, 0, T, groups, 1e-5f, s.gamma2, s.beta2, scale_shift, 2 * Cm, 0, 1, s.gph, nullptr, s.gno, B, st));
        const int rc = run_dconv_pair(s.W2, s.gno, s.Ws, s.k1, C1, s.k2, C2, T, s.bias_pair, gnpart, s.ko, B, st);
        return rc == 1 ? set_error(LDS_EINVAL, "bench wino pair: no fused direct variant for these shapes") : rc;
    };
    LDS_TRY(direct());
    std::string cfgs = std::string("direct ") + conv_dma_last_config();
    LDS_TRY(wino_pair_test_run(a, s, gnpart, B, st));
    cfgs += std::string(" | wino ") + conv_wino_last_config();
    if (cfg_out && cfg_cap) snprintf(cfg_out, cfg_cap, "%s", cfgs.c_str());
    hipEvent_t ev[3];
    for (auto& e : ev) HIP_TRY(hipEventCreate(&e));
    int rc = LDS_OK;
    for (int r = -1; r < reps && rc == LDS_OK; ++r) {      // (r = -1: one alternation that is not reported -- the first block of a shape runs into the clock's ramp)
        HIP_TRY(hipEventRecord(ev[0], st));
        for (int i = 0; i < iters && rc == LDS_OK; ++i) rc = direct();
        HIP_TRY(hipEventRecord(ev[1], st));
        for (int i = 0; i < iters && rc == LDS_OK; ++i) rc = wino_pair_test_run(a, s, gnpart, B, st);
        HIP_TRY(hipEventRecord(ev[2], st));
        HIP_TRY(hipEventSynchronize(ev[2]));
        float d = 0.f, w = 0.f;
        HIP_TRY(hipEventElapsedTime(&d, ev[0], ev[1]));
        HIP_TRY(hipEventElapsedTime(&w, ev[1], ev[2]));
        if (r >= 0) { ms_direct[r] = d / iters; ms_wino[r] = w / iters; }
    }
    for (auto& e : ev) (void)hipEventDestroy(e);
    HIP_TRY(hipStreamSynchronize(st));
    return rc;
}

// One vocoder upsampler on conv_dma, as vocoder_forward_impl runs the stages voc_dma_ups admits: plain x -> LeakyReLU(0.1) K4P copy with kVocPad
// zero frames per side -> polyphase ConvTranspose1d(K, stride, padding (K - stride + 1) / 2) -> the raw output and its LeakyReLU(0.1)
extern "C" int lds_test_voc_ups(const float* x, const float* w, const float* bias, int B, int Ci, int Co, int T, int K, int stride, const int32_t* lengths_in,
                                const int32_t* lengths_out, float* out, float* out_act, char* cfg_out, size_t cfg_cap, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    int lg = 0;
    while ((1 << lg) < stride) ++lg;
    if (!x || !w || !out || !out_act || B < 1 || T < 1 || Ci < 16 || Ci % 16 || Co < 64 || Co % 64 || stride < 2 || stride > 16 || (1 << lg) != stride || K != 2 * stride ||
        (lengths_in != nullptr) != (lengths_out != nullptr))
        return set_error(LDS_EINVAL, "bad argument");
    const int P = kVocPad, tpad = (K - stride + 1) / 2, Tn = (T - 1) * stride - 2 * tpad + K;
    for (int b = 0; b < B && lengths_in; ++b)
        if (lengths_in[b] < 0 || lengths_in[b] > T || lengths_out[b] < 0 || lengths_out[b] > Tn)
            return set_error(LDS_EINVAL, "lengths_in[%d] = %d / lengths_out[%d] = %d outside 0 .. %d / 0 .. %d", b, lengths_in[b], b, lengths_out[b], T, Tn);
    Owner own;
    TmpDev tmp;
    ConvW W;
    if (!pack_convT(own, w, bias, Ci, Co, K, stride, W)) return set_error(LDS_ENOMEM, "upload failed");
    int *vin = nullptr, *vout = nullptr;
    LDS_TRY(test_upload_lens(tmp, lengths_in, B, vin, st));
    LDS_TRY(test_upload_lens(tmp, lengths_out, B, vout, st));
    const size_t n_in = (size_t)B * Ci * (T + 2 * P), n_out = (size_t)B * Co * (Tn + 2 * P);
    float *scratch = tmp.f(n_in), *kin = tmp.f(n_in), *o_raw = tmp.f(n_out), *o_act = tmp.f(n_out);
    if (!scratch || !kin || !o_raw || !o_act) return set_error(LDS_ENOMEM, "alloc");
    HIP_TRY(hipMemsetAsync(kin, 0xff, n_in * sizeof(float), st));        // NaN fill: pads must be zeroed explicitly, real frames written
    HIP_TRY(hipMemsetAsync(o_raw, 0xff, n_out * sizeof(float), st));
    HIP_TRY(hipMemsetAsync(o_act, 0xff, n_out * sizeof(float), st));
    HIP_TRY(launch_to_k4p_act(x, scratch, kin, 0.1f, B, Ci, T, P, st, vin));
    HIP_TRY(launch_k4p_zero_pads(kin, B, Ci, T, P, st));
    DOpt o;
    o.voc = 1; o.xpad = P; o.opad = P; o.pad = 1; o.act_slope = 0.1f; o.out_act = o_act;
    o.ph_log2 = lg; o.ph_tpad = tpad; o.ph_Tout = Tn; o.vlen = vout;
    const int rc = run_dconv(W, kin, Ci, nullptr, 0, T, o, o_raw, B, st);
    if (rc == LDS_OK) {
        if (cfg_out && cfg_cap) snprintf(cfg_out, cfg_cap, "%s", conv_dma_last_config());
        HIP_TRY(launch_from_k4p_pad(o_raw, out, B, Co, Tn, P, st));
        HIP_TRY(launch_from_k4p_pad(o_act, out_act, B, Co, Tn, P, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    return rc;
}

// The wav2vec 2.0 encoder's own kernels alone (w2v.hip), plain tensors in and out; every pointer but the lengths is a device pointer.
extern "C" int lds_test_w2v_conv0(const float* audio, const int32_t* lengths, const float* w, const float* bias, const float* gamma, const float* beta,
                                  float eps, float* out, int B, int C, int64_t L, void* stream) {
    if (!audio || !w || !bias || !gamma || !beta || !out || B < 1 || B > 64 || L < 10 || L > ((int64_t)1 << 30)) return set_error(LDS_EINVAL, "bad argument");
    hipStream_t st = (hipStream_t)stream;
    TmpDev tmp;
    const int N0 = (int)((L - 10) / 5 + 1);
    float* ko = tmp.f((size_t)B * C * (N0 + 2));
    int* dl = (int*)tmp.f(128);
    if (!ko || !dl) return set_error(LDS_ENOMEM, "alloc");
    const int *slen = nullptr, *nlen = nullptr;
    if (lengths) {
        int32_t n0[64];
        for (int b = 0; b < B; ++b) {
            if (lengths[b] < 10 || lengths[b] > L) return set_error(LDS_EINVAL, "length[%d] = %d outside 10 .. %lld", b, lengths[b], (long long)L);
            n0[b] = (lengths[b] - 10) / 5 + 1;
        }
        LDS_TRY(upload_clip_ints(lengths, B, dl, st));
        LDS_TRY(upload_clip_ints(n0, B, dl + 64, st));
        slen = dl; nlen = dl + 64;
    }
    HIP_TRY(launch_w2v_conv0(audio, slen, L, w, bias, gamma, beta, eps, nlen, N0, C, ko, B, st));
    HIP_TRY(launch_from_k4p(ko, out, B, C, N0, st));
    HIP_TRY(hipStreamSynchronize(st));
    return LDS_OK;
}
extern "C" int lds_test_w2v_ln_act(const float* x, const int32_t* n_frames, const float* gamma, const float* beta, float eps, float* out, float* part, int B,
                                   int C, int T, void* stream) {
    if (!x || !gamma || !beta || !out || B < 1 || B > 64 || T < 1 || C < 64 || C % 64) return set_error(LDS_EINVAL, "bad argument");
    hipStream_t st = (hipStream_t)stream;
    TmpDev tmp;
    float* kx = tmp.f((size_t)B * C * (T + 2));
    float* ko = tmp.f((size_t)B * C * (T + 2));
    int* dl = (int*)tmp.f(64);
    if (!kx || !ko || !dl) return set_error(LDS_ENOMEM, "alloc");
    const int* nlen = nullptr;
    if (n_frames) {
        for (int b = 0; b < B; ++b)
            if (n_frames[b] < 1 || n_frames[b] > T) return set_error(LDS_EINVAL, "n_frames[%d] = %d outside 1 .. %d", b, n_frames[b], T);
        LDS_TRY(upload_clip_ints(n_frames, B, dl, st));
        nlen = dl;
    }
    HIP_TRY(launch_to_k4p(x, kx, B, C, T, C, 0, st));
    HIP_TRY(launch_w2v_ln_act(kx, gamma, beta, eps, ko, (float2*)part, nlen, B, C, T, st));
    HIP_TRY(launch_from_k4p(ko, out, B, C, T, st));
    HIP_TRY(hipStreamSynchronize(st));
    return LDS_OK;
}

// The w2v-BERT 2.0 encoder's own kernels alone (w2vbert.hip, attention_k4p.hip), plain tensors in and out; every pointer but the lengths is a
// device pointer.
extern "C" int lds_test_w2vbert_fbank(const float* audio, const int32_t* lengths, float* out, int B, int64_t L, void* stream) {
    if (!audio || !out || B < 1 || B > 64 || L < kW2vbertMinSamples || L > ((int64_t)1 << 30)) return set_error(LDS_EINVAL, "bad argument");
    hipStream_t st = (hipStream_t)stream;
    const int n_mels = 80, stride = 2, N = w2vbert_frames(L), R = (N + 1) / 2;
    Owner own;
    const std::vector<double> bs = w2vbert_basis();
    double* basis = (double*)own.upload_bytes(bs.data(), bs.size() * sizeof(double));
    float* filtT = own.upload(w2vbert_mel_filters(n_mels));
    TmpDev tmp;
    float* logspec = tmp.f((size_t)B * n_mels * N);
    double2* stat = (double2*)tmp.f((size_t)B * n_mels * 4);
    int* dl = (int*)tmp.f(64);
    if (!basis || !filtT || !logspec || !stat || !dl) return set_error(LDS_ENOMEM, "alloc");
    const int* slen = nullptr;
    if (lengths) {
        for (int b = 0; b < B; ++b)
            if (lengths[b] < kW2vbertMinSamples || lengths[b] > L) return set_error(LDS_EINVAL, "length[%d] = %d outside %d .. %lld", b, lengths[b], kW2vbertMinSamples, (long long)L);
        LDS_TRY(upload_clip_ints(lengths, B, dl, st));
        slen = dl;
    }
    HIP_TRY(launch_w2vbert_fbank(audio, slen, L, N, R, basis, filtT, n_mels, stride, kFbMelFloor, logspec, stat, out, B, st));
    HIP_TRY(hipStreamSynchronize(st));
    return LDS_OK;
}
extern "C" int lds_test_w2vbert_attention(const float* qkv, const float* E, const int32_t* q_rows, const int32_t* k_rows, float* out, int B, int C, int T,
                                          int heads, int left, int right, void* stream) {
    if (!qkv || !E || !out || B < 1 || B > 64 || T < 1 || heads < 1 || C != heads * 64 || left < 0 || right < 0 || left + right + 1 > kW2vbertRelStride)
        return set_error(LDS_EINVAL, "bad argument");
    hipStream_t st = (hipStream_t)stream;
    TmpDev tmp;
    float* qkp = tmp.f((size_t)B * 2 * C * T);       // plain [B][2C][T]
    float* vpl = tmp.f((size_t)B * C * T);
    float* vt = tmp.f((size_t)B * C * (T + 3) + 2048);
    float* kqk = tmp.f((size_t)B * 2 * C * (T + 2));
    float* ko = tmp.f((size_t)B * C * (T + 2));
    float* relp = tmp.f((size_t)B * heads * T * kW2vbertRelStride);
    int* dl = (int*)tmp.f(128);
    if (!qkp || !vpl || !vt || !kqk || !ko || !relp || !dl) return set_error(LDS_ENOMEM, "alloc");
    const int *ql = nullptr, *kl = nullptr;
    if (q_rows || k_rows) {
        if (!q_rows || !k_rows) return set_error(LDS_EINVAL, "q_rows and k_rows come together");
        for (int b = 0; b < B; ++b)
            if (q_rows[b] < 1 || q_rows[b] > T || k_rows[b] < 1 || k_rows[b] > q_rows[b]) return set_error(LDS_EINVAL, "rows[%d] = (%d, %d) outside 1 .. %d", b, q_rows[b], k_rows[b], T);
        LDS_TRY(upload_clip_ints(q_rows, B, dl, st));
        LDS_TRY(upload_clip_ints(k_rows, B, dl + 64, st));
        ql = dl; kl = dl + 64;
    }
    for (int b = 0; b < B; ++b) {
        HIP_TRY(hipMemcpyAsync(qkp + (size_t)b * 2 * C * T, qkv + (size_t)b * 3 * C * T, sizeof(float) * 2 * C * T, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemcpyAsync(vpl + (size_t)b * C * T, qkv + (size_t)b * 3 * C * T + (size_t)2 * C * T, sizeof(float) * C * T, hipMemcpyDeviceToDevice, st));
    }
    HIP_TRY(launch_to_k4p(qkp, kqk, B, 2 * C, T, 2 * C, 0, st));
    HIP_TRY(launch_plain_to_vt(vpl, vt, B, C, T, 64, st));
    HIP_TRY(launch_w2vbert_relpos(kqk, E, relp, ql, B, C, T, heads, left + right + 1, st));
    HIP_TRY(launch_attention_k4p_rel(kqk, vt, relp, ko, B, C, T, heads, ql, kl, left, right, st));
    HIP_TRY(launch_from_k4p(ko, out, B, C, T, st));
    HIP_TRY(hipStreamSynchronize(st));
    return LDS_OK;
}
extern "C" int lds_test_w2vbert_dwconv(const float* x, const float* w, const float* gamma, const float* beta, float eps, const int32_t* in_rows,
                                       const int32_t* out_rows, float* out, int B, int C, int T, int K, void* stream) {
    if (!x || !w || !gamma || !beta || !out || B < 1 || B > 64 || T < 1 || C < 64 || C % 64 || C > 1024 || K < 1 || K > 31) return set_error(LDS_EINVAL, "bad argument");
    hipStream_t st = (hipStream_t)stream;
    TmpDev tmp;
    float* kx = tmp.f((size_t)B * C * (T + 2));
    float* ko = tmp.f((size_t)B * C * (T + 2));
    float* wp = tmp.f((size_t)C * K);
    int* dl = (int*)tmp.f(128);
    if (!kx || !ko || !wp || !dl) return set_error(LDS_ENOMEM, "alloc");
    std::vector<float> hw((size_t)C * K), hp((size_t)C * K);
    HIP_TRY(hipMemcpy(hw.data(), w, hw.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (int c = 0; c < C; ++c)
        for (int k = 0; k < K; ++k) hp[((size_t)((c >> 3) * 2 + (c & 1)) * K + k) * 4 + ((c & 7) >> 1)] = hw[(size_t)c * K + k];
    HIP_TRY(hipMemcpy(wp, hp.data(), hp.size() * sizeof(float), hipMemcpyHostToDevice));
    const int *vl = nullptr, *nl = nullptr;
    if (in_rows || out_rows) {
        if (!in_rows || !out_rows) return set_error(LDS_EINVAL, "in_rows and out_rows come together");
        for (int b = 0; b < B; ++b)
            if (out_rows[b] < 1 || out_rows[b] > T || in_rows[b] < 1 || in_rows[b] > out_rows[b]) return set_error(LDS_EINVAL, "rows[%d] = (%d, %d) outside 1 .. %d", b, in_rows[b], out_rows[b], T);
        LDS_TRY(upload_clip_ints(in_rows, B, dl, st));
        LDS_TRY(upload_clip_ints(out_rows, B, dl + 64, st));
        vl = dl; nl = dl + 64;
    }
    HIP_TRY(launch_to_k4p(x, kx, B, C, T, C, 0, st));
    HIP_TRY(launch_w2vbert_dwconv(kx, wp, gamma, beta, eps, ko, vl, nl, B, C, T, K, st));
    HIP_TRY(launch_from_k4p(ko, out, B, C, T, st));
    HIP_TRY(hipStreamSynchronize(st));
    return LDS_OK;
}

// The WavLM encoder's gated-bias attention alone (attention_k4p.hip), plain tensors in and out; every pointer but the lengths is a device
// pointer.  wavlm_buckets touches no device.
extern "C" int lds_test_wavlm_attention(const float* qkv, const float* gate, const float* toep, const int32_t* lengths, float* out, int B, int C, int T,
                                        int heads, int n_ctx, void* stream) {
    if (!qkv || !gate || !toep || !out || B < 1 || B > 64 || T < 1 || heads < 1 || C != heads * 64 || n_ctx < T || n_ctx > 1500) return set_error(LDS_EINVAL, "bad argument");
    hipStream_t st = (hipStream_t)stream;
    TmpDev tmp;
    float* qkp = tmp.f((size_t)B * 2 * C * T);       // plain [B][2C][T]
    float* vpl = tmp.f((size_t)B * C * T);
    float* vt = tmp.f((size_t)B * C * (T + 3) + 2048);
    float* kqk = tmp.f((size_t)B * 2 * C * (T + 2));
    float* ko = tmp.f((size_t)B * C * (T + 2));
    int* dl = (int*)tmp.f(64);
    if (!qkp || !vpl || !vt || !kqk || !ko || !dl) return set_error(LDS_ENOMEM, "alloc");
    const int* ln = nullptr;
    if (lengths) {
        for (int b = 0; b < B; ++b)
            if (lengths[b] < 1 || lengths[b] > T) return set_error(LDS_EINVAL, "lengths[%d] = %d outside 1 .. %d", b, lengths[b], T);
        LDS_TRY(upload_clip_ints(lengths, B, dl, st));
        ln = dl;
    }
    for (int b = 0; b < B; ++b) {
        HIP_TRY(hipMemcpyAsync(qkp + (size_t)b * 2 * C * T, qkv + (size_t)b * 3 * C * T, sizeof(float) * 2 * C * T, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemcpyAsync(vpl + (size_t)b * C * T, qkv + (size_t)b * 3 * C * T + (size_t)2 * C * T, sizeof(float) * C * T, hipMemcpyDeviceToDevice, st));
        if (lengths && lengths[b] < T)
            HIP_TRY(hipMemset2DAsync(vpl + (size_t)b * C * T + lengths[b], sizeof(float) * T, 0, sizeof(float) * (T - lengths[b]), C, st));
    }
    HIP_TRY(hipMemsetAsync(ko, 0xff, (size_t)B * C * (T + 2) * sizeof(float), st));
    HIP_TRY(launch_to_k4p(qkp, kqk, B, 2 * C, T, 2 * C, 0, st));
    HIP_TRY(launch_plain_to_vt(vpl, vt, B, C, T, 64, st));
    HIP_TRY(launch_attention_k4p_bias(kqk, vt, gate, toep, ko, B, C, T, heads, ln, n_ctx, st));
    HIP_TRY(launch_from_k4p(ko, out, B, C, T, st));
    HIP_TRY(hipStreamSynchronize(st));
    return LDS_OK;
}
extern "C" int lds_test_wavlm_buckets(int num_buckets, int max_distance, int n, int32_t* out) {
    if (!out || n < 1 || n > (1 << 20)) return set_error(LDS_EINVAL, "bad argument");
    LDS_TRY(wavlm_bucket_check(num_buckets, max_distance));
    for (int d = -(n - 1); d < n; ++d) out[d + n - 1] = wavlm_bucket(d, num_buckets, max_distance);
    return LDS_OK;
}
