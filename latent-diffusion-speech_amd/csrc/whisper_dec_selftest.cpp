// The Whisper decoder's host side on its own under AddressSanitizer + UBSan (tests/test_cpu_whisper_decoder.py): an ordinary executable
// with the host-only objects of the library linked in (build_asan/*.o + host_stub_hip.cpp), where hipMalloc is malloc and a launch fails.  So a create
// packs and "uploads" its weights for real, and every refusal below has to come before anything is enqueued: a call that reached a
// launch would answer LDS_EHIP, not the code it is held to.
#include "../../include/lds.h"

#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

static int fails = 0;
static void expect(const char* what, int rc, int want, const char* needle = nullptr) {
    const char* msg = lds_last_error();
    const bool ok = rc == want && (!needle || (msg && strstr(msg, needle)));
    printf("%s %s: rc %d%s%s\n", ok ? "ok  " : "FAIL", what, rc, rc ? " -- " : "", rc ? (msg ? msg : "") : "");
    if (!ok) ++fails;
}

int main() {
    const lds_whisper_decoder_cfg cfg{97, 16, 64, 1, 2, 40};
    const int C = cfg.n_state;
    std::vector<std::string> names;
    std::vector<std::vector<float>> data;
    auto add = [&](const std::string& n, size_t cnt) { names.push_back(n); data.emplace_back(cnt, 0.01f); };
    add("decoder.token_embedding.weight", (size_t)cfg.n_vocab * C);
    add("decoder.positional_embedding", (size_t)cfg.n_text_ctx * C);
    for (int i = 0; i < cfg.n_layer; ++i) {
        const std::string p = "decoder.blocks." + std::to_string(i) + ".";
        for (const char* a : {"attn", "cross_attn"}) {
            for (const char* m : {"query", "value", "out"}) { add(p + a + "." + m + ".weight", (size_t)C * C); add(p + a + "." + m + ".bias", C); }
            add(p + a + ".key.weight", (size_t)C * C);
            add(p + std::string(a) + "_ln.weight", C); add(p + std::string(a) + "_ln.bias", C);
        }
        add(p + "mlp_ln.weight", C); add(p + "mlp_ln.bias", C);
        add(p + "mlp.0.weight", (size_t)4 * C * C); add(p + "mlp.0.bias", 4 * C);
        add(p + "mlp.2.weight", (size_t)4 * C * C); add(p + "mlp.2.bias", C);
    }
    add("decoder.ln.weight", C); add("decoder.ln.bias", C);
    std::vector<const char*> np;
    std::vector<const float*> pp;
    std::vector<int64_t> ne;
    for (size_t i = 0; i < names.size(); ++i) { np.push_back(names[i].c_str()); pp.push_back(data[i].data()); ne.push_back((int64_t)data[i].size()); }
    const int n = (int)names.size();

    lds_whisper_decoder* h = nullptr;
    lds_whisper_decoder_cfg bad = cfg;
    bad.n_head = 2;
    expect("create: n_state / n_head != 64", lds_whisper_decoder_create(&bad, n, np.data(), pp.data(), ne.data(), &h), LDS_EINVAL, "n_state / n_head");
    bad = cfg; bad.n_text_ctx = 449;
    expect("create: n_text_ctx 449", lds_whisper_decoder_create(&bad, n, np.data(), pp.data(), ne.data(), &h), LDS_EINVAL, "n_text_ctx");
    bad = cfg; bad.n_audio_ctx = 1501;
    expect("create: n_audio_ctx 1501", lds_whisper_decoder_create(&bad, n, np.data(), pp.data(), ne.data(), &h), LDS_EINVAL, "n_audio_ctx");
    {
        std::vector<const char*> np2 = np;
        for (int i = 0; i < n; ++i)
            if (names[i] == "decoder.blocks.1.cross_attn.key.weight") np2[i] = nullptr;
        expect("create: a missing tensor", lds_whisper_decoder_create(&cfg, n, np2.data(), pp.data(), ne.data(), &h), LDS_EMISSING,
               "decoder.blocks.1.cross_attn.key.weight (absent)");
        std::vector<int64_t> ne2 = ne;
        ne2[0] -= 1;
        expect("create: a tensor of the wrong size", lds_whisper_decoder_create(&cfg, n, np.data(), pp.data(), ne2.data(), &h), LDS_EMISSING,
               "decoder.token_embedding.weight (wrong size)");
    }
    expect("create", lds_whisper_decoder_create(&cfg, n, np.data(), pp.data(), ne.data(), &h), LDS_OK);
    if (!h) return 1;

    size_t need = 0, need2 = 0;
    expect("workspace_bytes", lds_whisper_decoder_workspace_bytes(h, 3, 40, 16, &need), LDS_OK);
    expect("workspace_bytes: S = 2", lds_whisper_decoder_workspace_bytes(h, 3, 40, 2, &need2), LDS_OK);
    // the cross part: 2 * n_layer * B * T * n_state floats (each slot a multiple of 256 bytes here) lie inside either size
    if (!(need > need2 && need2 > (size_t)2 * cfg.n_layer * 3 * 40 * C * 4)) { printf("FAIL sizes %zu %zu\n", need, need2); ++fails; }
    expect("workspace_bytes: S > n_text_ctx", lds_whisper_decoder_workspace_bytes(h, 3, 40, 17, &need2), LDS_EINVAL, "n_text_ctx");
    expect("workspace_bytes: T > n_audio_ctx", lds_whisper_decoder_workspace_bytes(h, 3, 41, 16, &need2), LDS_EINVAL, "T 41");
    expect("workspace_bytes: B = 65", lds_whisper_decoder_workspace_bytes(h, 65, 40, 16, &need2), LDS_EINVAL, "B 65");

    std::vector<char> ws(need);
    std::vector<float> units((size_t)3 * 40 * C, 0.f), out((size_t)3 * 16 * cfg.n_vocab);
    std::vector<int64_t> toks((size_t)3 * 16, 1);
    const int32_t nf_bad[3] = {1, 41, 7}, nf_zero[3] = {1, 0, 7}, plen[3] = {1, 2, 4}, plen_bad[3] = {1, 5, 4};
    expect("cross: n_frames > T", lds_whisper_decoder_cross(h, units.data(), nf_bad, 3, 40, ws.data(), need, nullptr), LDS_EINVAL, "n_frames[1] = 41");
    expect("cross: n_frames = 0", lds_whisper_decoder_cross(h, units.data(), nf_zero, 3, 40, ws.data(), need, nullptr), LDS_EINVAL, "n_frames[1] = 0");
    expect("cross: a small workspace", lds_whisper_decoder_cross(h, units.data(), nullptr, 3, 40, ws.data(), 4096, nullptr), LDS_ENOMEM, "need ");
    expect("logits: S > n_text_ctx", lds_whisper_decoder_logits(h, toks.data(), nullptr, nullptr, 3, 17, 40, out.data(), nullptr, nullptr, nullptr, nullptr, ws.data(), need, nullptr),
           LDS_EINVAL, "n_text_ctx");
    expect("logits: S = 1", lds_whisper_decoder_logits(h, toks.data(), nullptr, nullptr, 3, 1, 40, out.data(), nullptr, nullptr, nullptr, nullptr, ws.data(), need, nullptr),
           LDS_EINVAL);
    expect("logits: nothing asked for", lds_whisper_decoder_logits(h, toks.data(), nullptr, nullptr, 3, 9, 40, nullptr, nullptr, nullptr, nullptr, nullptr, ws.data(), need, nullptr),
           LDS_EINVAL, "nothing to compute");
    expect("logits: half a scoring request", lds_whisper_decoder_logits(h, toks.data(), nullptr, nullptr, 3, 9, 40, nullptr, out.data(), nullptr, nullptr, nullptr, ws.data(), need, nullptr),
           LDS_EINVAL, "together");
    expect("logits: a small workspace", lds_whisper_decoder_logits(h, toks.data(), nullptr, nullptr, 3, 16, 40, out.data(), nullptr, nullptr, nullptr, nullptr, ws.data(), need - 256, nullptr),
           LDS_ENOMEM, "need ");

    lds_whisper_decode_opts o{};
    o.max_new_tokens = 4; o.eos = 95; o.pad = 95; o.num_beams = 1;
    std::vector<float> tlp(3 * 4), slp(3);
    int n_tok = 0;
    auto gen = [&](const lds_whisper_decode_opts& oo, const int32_t* pl, int P, int cap, size_t bytes) {
        return lds_whisper_decoder_generate(h, toks.data(), pl, 3, P, 40, cap, &oo, toks.data(), tlp.data(), slp.data(), nullptr, &n_tok, ws.data(), bytes, nullptr);
    };
    lds_whisper_decode_opts b1 = o; b1.no_repeat_ngram_size = 2;
    expect("generate: an n-gram ban", gen(b1, plen, 4, 16, need), LDS_EINVAL, "no_repeat_ngram_size");
    b1 = o; b1.num_beams = 5;
    expect("generate: beams", gen(b1, plen, 4, 16, need), LDS_EINVAL, "beam search");
    b1 = o; b1.temperature = 0.2f;
    expect("generate: a temperature", gen(b1, plen, 4, 16, need), LDS_EINVAL, "temperature");
    b1 = o; b1.eos = 97;
    expect("generate: eos outside the vocabulary", gen(b1, plen, 4, 16, need), LDS_EINVAL, "eos 97");
    b1 = o; b1.n_suppress = 3;
    expect("generate: a suppress count without ids", gen(b1, plen, 4, 16, need), LDS_EINVAL, "suppress");
    b1 = o; b1.max_new_tokens = 0;
    expect("generate: max_new_tokens 0", gen(b1, plen, 4, 16, need), LDS_EINVAL, "max_new_tokens");
    expect("generate: cap > n_text_ctx", gen(o, plen, 4, 17, need), LDS_EINVAL, "n_text_ctx");
    expect("generate: no room behind the prompt", gen(o, plen, 16, 16, need), LDS_EINVAL, "no room");
    expect("generate: prompt_len > P", gen(o, plen_bad, 4, 16, need), LDS_EINVAL, "prompt_len[1] = 5");
    expect("generate: a small workspace", gen(o, plen, 4, 16, need - 256), LDS_ENOMEM, "need ");
    expect("generate: null options", lds_whisper_decoder_generate(h, toks.data(), plen, 3, 4, 40, 16, nullptr, toks.data(), tlp.data(), slp.data(), nullptr, &n_tok, ws.data(), need, nullptr),
           LDS_EINVAL, "null options");
    lds_whisper_decoder_destroy(h);
    printf("%s\n", fails ? "whisper decoder selftest FAILED" : "whisper decoder selftest passed");
    return fails ? 1 : 0;
}
