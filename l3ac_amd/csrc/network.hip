// Network construction (weight lookup, layout transforms, upload) and the encode / decode pipelines.
#include "network.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>

namespace {

constexpr int HEADS = 6;  // LocalTrans.builder (reference l3ac/local_trans.py:51)

struct Builder {
    l3ac_ctx* ctx = nullptr;
    std::unordered_map<std::string, const l3ac_tensor*> map;
    std::vector<float> host;  // staging image of the device arena
    float* dev = nullptr;
    size_t cap = 0;
    std::string err;
    // every weight image (bf16x3 split images of the GEMM weights, the fused kernels' streams) in the order of the walk: `write` puts it
    // into the staging copy of the one device allocation they share, *target is bound to its place there
    struct Image { size_t bytes; std::function<void(unsigned char*)> write; const unsigned char** target; };
    std::vector<Image> images;
    bool trans_stacks = false;  // some LocalTrans stack has its trans_stack_kernel image
    const float* host_of(const float* d) const { return host.data() + (d - dev); }

    void image(std::vector<unsigned char> img, const unsigned char** target) {
        const size_t bytes = img.size();
        images.push_back({bytes, [img = std::move(img)](unsigned char* out) { std::memcpy(out, img.data(), img.size()); }, target});
    }
    // an [n][k] weight of the arena (its final layout) as a GEMM operand: queues its split image, bound to the weight's slot in split_img
    // (the largest images: built straight into the staging copy)
    const float* gemm(const float* d, int n, int k) {
        if (d && err.empty() && gemm_split_eligible(n, k))
            images.push_back({(size_t)gemm_split_image_bytes(n, k), [=](unsigned char* out) { gemm_split_image_host(host_of(d), k, n, k, out); },
                              &ctx->split_img[d]});
        return d;
    }
    const float* find(const std::string& name, int64_t numel) {
        auto it = map.find(name);
        if (it == map.end()) {
            if (err.empty()) err = "missing weight tensor '" + name + "'";
            return nullptr;
        }
        if (it->second->numel != numel) {
            if (err.empty())
                err = "weight tensor '" + name + "' has " + std::to_string(it->second->numel) + " elements, expected " +
                      std::to_string(numel);
            return nullptr;
        }
        return it->second->data;
    }
    // reserve n floats in the arena (256-byte aligned), return {host pointer, device pointer}: both null when the arena is full
    float* alloc(size_t n, const float** dptr) {
        const size_t off = (host.size() + 63) / 64 * 64;
        if (off + n > cap) {
            if (err.empty()) err = "internal: weight arena overflow";
            *dptr = nullptr;
            return nullptr;
        }
        host.resize(off + n, 0.f);
        *dptr = dev + off;
        return host.data() + off;
    }
    const float* copy(const std::string& name, int64_t numel) {
        const float* src = find(name, numel);
        const float* d = nullptr;
        float* h = alloc((size_t)numel, &d);
        if (src && d) std::memcpy(h, src, (size_t)numel * sizeof(float));
        return d;
    }
    // Conv1d weight [co][ci][k] -> [co][k][ci]  (k-contiguous rows for the implicit-conv GEMM)
    const float* conv(const std::string& name, int co, int ci, int k) {
        const float* src = find(name, (int64_t)co * ci * k);
        const float* d = nullptr;
        float* h = alloc((size_t)co * ci * k, &d);
        if (src && d)
            for (int o = 0; o < co; ++o)
                for (int c = 0; c < ci; ++c)
                    for (int j = 0; j < k; ++j) h[((size_t)o * k + j) * ci + c] = src[((size_t)o * ci + c) * k + j];
        return d;
    }
    // depth-wise Conv1d weight [c][1][7] -> [7][c]
    const float* dwconv(const std::string& name, int c) {
        const float* src = find(name, (int64_t)c * 7);
        const float* d = nullptr;
        float* h = alloc((size_t)c * 7, &d);
        if (src && d)
            for (int ch = 0; ch < c; ++ch)
                for (int j = 0; j < 7; ++j) h[(size_t)j * c + ch] = src[(size_t)ch * 7 + j];
        return d;
    }
    // weight [n][k] -> [k][n]
    const float* transposed(const std::string& name, int n, int k) {
        const float* src = find(name, (int64_t)n * k);
        const float* d = nullptr;
        float* h = alloc((size_t)k * n, &d);
        if (src && d)
            for (int o = 0; o < n; ++o)
                for (int i = 0; i < k; ++i) h[(size_t)i * n + o] = src[(size_t)o * k + i];
        return d;
    }
    // FeedForward's first weight [2 * ffi][dim] -> (value, gate) 32-row tiles interleaved, zero padded: [ff_n][dim]
    const float* ff_value_gate(const std::string& name, int ffi, int dim, int ff_n) {
        const float* src = find(name, (int64_t)2 * ffi * dim);
        const float* d = nullptr;
        float* h = alloc((size_t)ff_n * dim, &d);
        if (src && d)
            for (int j = 0; j < ffi; ++j) {
                const int jb = j / 32, r = j % 32;
                std::memcpy(h + (size_t)(64 * jb + r) * dim, src + (size_t)j * dim, dim * sizeof(float));
                std::memcpy(h + (size_t)(64 * jb + 32 + r) * dim, src + (size_t)(ffi + j) * dim, dim * sizeof(float));
            }
        return d;
    }
    // FeedForward's second weight [dim][ffi] -> [dim][ff_pad] zero padded along k
    const float* ff_padded(const std::string& name, int dim, int ffi, int ff_pad) {
        const float* src = find(name, (int64_t)dim * ffi);
        const float* d = nullptr;
        float* h = alloc((size_t)dim * ff_pad, &d);
        if (src && d)
            for (int o = 0; o < dim; ++o) std::memcpy(h + (size_t)o * ff_pad, src + (size_t)o * ffi, ffi * sizeof(float));
        return d;
    }
    // the trend convs of n branches, p.blocks.<i>.1 = Conv1d weight [co][1][7] and bias [co], packed as [n][co][7] and [n][co]
    void trend(const std::string& p, int n, int co, const float** tw, const float** tb) {
        float* hw = alloc((size_t)n * co * 7, tw);
        float* hb = alloc((size_t)n * co, tb);
        for (int i = 0; i < n; ++i) {
            const float* w = find(p + ".blocks." + std::to_string(i) + ".1.weight", co * 7);
            const float* bb = find(p + ".blocks." + std::to_string(i) + ".1.bias", co);
            if (w && bb && hw && hb) {
                std::memcpy(hw + (size_t)i * co * 7, w, (size_t)co * 7 * sizeof(float));
                std::memcpy(hb + (size_t)i * co, bb, co * sizeof(float));
            }
        }
    }
    // snake: 1 / (alpha + 1e-8) evaluated in fp32 exactly as layers.py:32 does
    const float* inv_alpha(const std::string& name, int n) {
        const float* src = find(name, n);
        const float* d = nullptr;
        float* h = alloc((size_t)n, &d);
        if (src && d)
            for (int i = 0; i < n; ++i) h[i] = 1.0f / (src[i] + 1e-8f);
        return d;
    }
};

static float silu(float x) { return x / (1.0f + std::exp(-x)); }

// DynamicPositionBias MLP over the integer distances 0 .. 2W-1 (local_attention.transformer), [heads][2W]
const float* build_bias_table(Builder& b, const std::string& prefix, int dim, int window) {
    const int hdim = dim / 2;
    const float* w0 = b.find(prefix + ".mlp.0.weight", hdim);
    const float* b0 = b.find(prefix + ".mlp.0.bias", hdim);
    const float* w2 = b.find(prefix + ".mlp.2.weight", (int64_t)hdim * hdim);
    const float* b2 = b.find(prefix + ".mlp.2.bias", hdim);
    const float* w4 = b.find(prefix + ".mlp.4.weight", (int64_t)HEADS * hdim);
    const float* b4 = b.find(prefix + ".mlp.4.bias", HEADS);
    const float* d = nullptr;
    float* h = b.alloc((size_t)HEADS * 2 * window, &d);
    if (!(w0 && b0 && w2 && b2 && w4 && b4 && d)) return d;
    std::vector<float> h1(hdim), h2(hdim);
    for (int dist = 0; dist < 2 * window; ++dist) {
        for (int i = 0; i < hdim; ++i) h1[i] = silu(w0[i] * (float)dist + b0[i]);
        for (int i = 0; i < hdim; ++i) {
            float s = b2[i];
            for (int j = 0; j < hdim; ++j) s += w2[(size_t)i * hdim + j] * h1[j];
            h2[i] = silu(s);
        }
        for (int hd = 0; hd < HEADS; ++hd) {
            float s = b4[hd];
            for (int j = 0; j < hdim; ++j) s += w4[(size_t)hd * hdim + j] * h2[j];
            h[(size_t)hd * 2 * window + dist] = s;
        }
    }
    return d;
}

// One builder per block kind: it reads the block `p` of the reference's module list into the block it is given, queues the block's weight
// images — only when every tensor of the network so far was found: the images are made from the arena's staging copy — and enters the
// block into the name index of the l3ac_op_* entry points.  The images' targets point into the block: it must not move afterwards.

void build_first_block(Builder& b, FirstBlockW& f, const std::string& p, int d0) {  // modules.py:71-93
    b.trend(p, 5, 4, &f.tw, &f.tb);
    f.d0 = d0;
    f.w1 = b.copy(p + ".conv_1.weight", 80 * 20);
    f.b1 = b.copy(p + ".conv_1.bias", 80);
    f.w2 = b.transposed(p + ".conv_2.weight", d0, 81);  // [81][d0]
    f.b2 = b.copy(p + ".conv_2.bias", d0);
}

void build_conv_unit(Builder& b, ConvUnitW& u, const std::string& p, int c) {
    u.c = c;
    u.dw_w = b.dwconv(p + ".dw_conv.weight", c);
    u.dw_b = b.copy(p + ".dw_conv.bias", c);
    u.ln_w = b.copy(p + ".norm.weight", c);
    u.ln_b = b.copy(p + ".norm.bias", c);
    u.w1 = b.gemm(b.copy(p + ".pw_conv1.weight", (int64_t)4 * c * c), 4 * c, c);
    u.b1 = b.copy(p + ".pw_conv1.bias", 4 * c);
    u.alpha = b.copy(p + ".act.alpha", 4 * c);
    u.inv_alpha = b.inv_alpha(p + ".act.alpha", 4 * c);
    u.gamma = b.copy(p + ".grn.gamma", 4 * c);
    u.beta = b.copy(p + ".grn.beta", 4 * c);
    u.w2 = b.gemm(b.copy(p + ".pw_conv2.weight", (int64_t)4 * c * c), c, 4 * c);
    u.b2 = b.copy(p + ".pw_conv2.bias", c);
    if (b.err.empty()) {
        if (conv_unit_wide_supported(c)) {  // (C = 96 .. 256; on the exact route C = 96 takes conv_unit_fused_kernel: fp32 weights)
            b.image(conv_unit_wide_image(b.host_of(u.w1), b.host_of(u.w2), c), &u.wide_img);
        } else if (conv_unit_fused_supported(c)) {
            b.image(conv_unit_w1_image(b.host_of(u.w1), c), &u.w1_img);
            b.image(conv_unit_w2_image(b.host_of(u.w2), c), &u.w2_img);
            if (conv_unit_ring_supported(c)) b.image(conv_unit_ring_image(b.host_of(u.w1), b.host_of(u.w2), c), &u.ring_img);
        }
    }
    b.ctx->by_unit[p] = &u;
}

// Conv1d(k = stride): with `norm` the layer p.0 of a Sequential whose p.1 is the ChannelNorm (encoder), else p itself (DownTrans)
void build_down(Builder& b, DownW& d, const std::string& p, int cin, int cout, int stride, bool norm) {
    d.cin = cin;
    d.cout = cout;
    d.stride = stride;
    const std::string conv = norm ? p + ".0" : p;
    d.w = b.gemm(b.conv(conv + ".weight", cout, cin, stride), cout, stride * cin);
    d.b = b.copy(conv + ".bias", cout);
    if (norm) {
        d.nw = b.copy(p + ".1.weight", cout);
        d.nb = b.copy(p + ".1.bias", cout);
        if (b.err.empty() && down_exact_supported(cin, stride, cout)) b.image(down_exact_image(b.host_of(d.w), cin * stride, cout), &d.exact_img);
    }
    b.ctx->by_down[p] = &d;
}

// `split`: the conv runs as a GEMM that may take the bf16x3 route (the decoder's; the encoder's output conv stays on fp32)
void build_conv_k3(Builder& b, ConvK3W& k, const std::string& p, int cin, int cout, bool split) {
    k.cin = cin;
    k.cout = cout;
    k.w = b.conv(p + ".weight", cout, cin, 3);
    if (split) b.gemm(k.w, cout, 3 * cin);
    k.b = b.copy(p + ".bias", cout);
    b.ctx->by_k3[p] = &k;
}

void build_enhance(Builder& b, EnhW& e, const std::string& p, int c) {
    e.c = c;
    b.trend(p, 4, 1, &e.t.tw, &e.t.tb);
    e.in_w = b.copy(p + ".merge_layer.0.weight", 4);
    e.in_b = b.copy(p + ".merge_layer.0.bias", 4);
    e.gate_w = b.copy(p + ".merge_layer.1.weight", (int64_t)c * 4);
    e.gate_b = b.copy(p + ".merge_layer.1.bias", c);
    b.ctx->by_enh[p] = &e;
}

void build_up(Builder& b, UpW& u, const std::string& p, int cin, int cout, int scale) {
    u.cin = cin;
    u.cout = cout;
    u.scale = scale;
    u.w = b.gemm(b.copy(p + ".0.weight", (int64_t)cout * cin), cout, cin);
    u.b = b.copy(p + ".0.bias", cout);
    u.nw = b.copy(p + ".2.weight", cout);
    u.nb = b.copy(p + ".2.bias", cout);
    if (b.err.empty() && up_fused_supported(cin, cout)) b.image(up_fused_image(b.host_of(u.w), cin, cout), &u.fused_img);
    b.ctx->by_up[p] = &u;
}

void build_legacy_unit(Builder& b, LegacyW& l, const std::string& p, int c, int dil) {
    l.c = c;
    l.dil = dil;
    l.a0 = b.copy(p + ".0.alpha", c);
    l.ia0 = b.inv_alpha(p + ".0.alpha", c);
    l.w1 = b.conv(p + ".1.weight", c, c, 7);
    l.b1 = b.copy(p + ".1.bias", c);
    l.a1 = b.copy(p + ".2.alpha", c);
    l.ia1 = b.inv_alpha(p + ".2.alpha", c);
    l.w2 = b.copy(p + ".3.weight", (int64_t)c * c);
    l.b2 = b.copy(p + ".3.bias", c);
    if (b.err.empty() && last_block_fused_supported(c, 9)) {  // (9: the largest dilation of the last block's three units)
        b.image(legacy_w1_image(b.host_of(l.w1), c), &l.w1_img);
        b.image(legacy_w2_image(b.host_of(l.w2), c), &l.w2_img);
    }
}

void build_head(Builder& b, HeadW& h, const std::string& p, int c) {
    h.c = c;
    h.alpha = b.copy(p + ".1.alpha", c);
    h.inv_alpha = b.inv_alpha(p + ".1.alpha", c);
    h.w = b.conv(p + ".2.weight", 1, c, 7);  // [1][7][c]
    h.b = b.copy(p + ".2.bias", 1);
}

void build_local_trans(Builder& b, LocalTransW& t, const std::string& p, int window, int depth) {
    const l3ac_ctx* ctx = b.ctx;
    t.window = window;
    const int dim = ctx->cfg.feature_dim;
    const int inner = ctx->inner, ffi = ctx->ff_inner;
    for (int l = 0; l < depth; ++l) {
        const std::string a = p + ".layers." + std::to_string(l) + ".0";
        const std::string f = p + ".layers." + std::to_string(l) + ".1";
        TransLayerW w{};
        w.ln1w = b.copy(a + ".norm.weight", dim);
        w.ln1b = b.copy(a + ".norm.bias", dim);
        w.wqkv = b.gemm(b.copy(a + ".to_qkv.weight", (int64_t)3 * inner * dim), 3 * inner, dim);
        w.wout = b.gemm(b.copy(a + ".to_out.weight", (int64_t)dim * inner), dim, inner);
        w.ln2w = b.copy(f + ".0.weight", dim);
        w.ln2b = b.copy(f + ".0.bias", dim);
        w.wff1 = b.gemm(b.ff_value_gate(f + ".1.weight", ffi, dim, ctx->ff_n), ctx->ff_n, dim);
        w.wff2 = b.gemm(b.ff_padded(f + ".4.weight", dim, ffi, ctx->ff_pad), dim, ctx->ff_pad);
        t.layers.push_back(w);
    }
    t.bias_table = build_bias_table(b, p + ".dynamic_pos_bias", dim, window);
    // the stack as trans_stack_kernel takes it
    if (b.err.empty() && trans_stack_supported(dim, ctx->dim_head, HEADS, ffi, 1, window, depth)) {
        const float* d = nullptr;
        float* ln = b.alloc((size_t)depth * 4 * dim, &d);
        if (d) {
            t.stack_ln = d;
            std::vector<unsigned char> img;
            img.reserve((size_t)depth * (size_t)trans_stack_layer_image_bytes());
            for (int l = 0; l < depth; ++l) {
                const TransLayerW& w = t.layers[l];
                const float* srcs[4] = {w.ln1w, w.ln1b, w.ln2w, w.ln2b};
                for (int q = 0; q < 4; ++q) std::memcpy(ln + ((size_t)l * 4 + q) * dim, b.host_of(srcs[q]), dim * sizeof(float));
                trans_stack_layer_image(img, b.host_of(w.wqkv), b.host_of(w.wout), b.host_of(w.wff1), ctx->ff_n, b.host_of(w.wff2), ctx->ff_pad);
            }
            b.image(std::move(img), &t.stack_img);
            b.trans_stacks = true;
        }
    }
    b.ctx->by_trans[p] = &t;
}

int free_buf(float*& p) {
    if (p) {
        L3AC_HIP_CHECK(hipFree(p));
        p = nullptr;
    }
    return L3AC_OK;
}

}  // namespace

int network_build(l3ac_ctx* ctx, const l3ac_tensor* tensors, int n_tensors) {
    const l3ac_config& c = ctx->cfg;
    L3AC_REQUIRE(c.abi_version == L3AC_ABI_VERSION, "config abi_version %d != %d", c.abi_version, L3AC_ABI_VERSION);
    L3AC_REQUIRE(c.n_enc >= 2 && c.n_enc <= L3AC_MAX_STAGES && c.n_dec >= 2 && c.n_dec <= L3AC_MAX_STAGES,
                 "bad stage counts (n_enc=%d n_dec=%d)", c.n_enc, c.n_dec);
    L3AC_REQUIRE(c.n_levels >= 1 && c.n_levels <= L3AC_MAX_LEVELS, "bad n_levels=%d", c.n_levels);
    L3AC_REQUIRE(c.feature_dim >= 8 && c.feature_dim % 8 == 0, "feature_dim=%d must be a multiple of 8", c.feature_dim);
    L3AC_REQUIRE(c.en_coder_compress_rate >= 1 && c.en_coder_window_size >= 1, "bad en_coder geometry");
    for (int i = 0; i < c.n_enc; ++i) L3AC_REQUIRE(c.enc_dims[i] % 4 == 0, "encoder_dims must be multiples of 4");
    for (int i = 0; i < c.n_dec; ++i) L3AC_REQUIRE(c.dec_dims[i] % 4 == 0, "decoder_dims must be multiples of 4");
    ctx->enc_rate = 1;
    for (int i = 0; i + 1 < c.n_enc; ++i) ctx->enc_rate *= c.compress_rates[i];
    int dec_rate = 1;
    for (int i = 0; i + 1 < c.n_dec; ++i) dec_rate *= c.decode_rates[i];
    L3AC_REQUIRE(dec_rate == ctx->enc_rate, "prod(decode_rates)=%d != prod(compress_rates)=%d", dec_rate, ctx->enc_rate);
    ctx->hop = ctx->enc_rate * c.en_coder_compress_rate;
    ctx->dim_head = c.feature_dim / 4;  // LocalTrans.builder: dim_head = feature_dim // 4
    ctx->inner = HEADS * ctx->dim_head;
    ctx->ff_inner = (int)((double)c.feature_dim * 4 * 2 / 3);  // FeedForward: int(dim * mult * 2 / 3)
    ctx->ff_pad = (int)round_up64(ctx->ff_inner, 4);
    ctx->ff_n = 64 * (int)ceil_div64(ctx->ff_inner, 32);
    const bool compressed = c.en_coder_compress_rate != 1;
    if (compressed) L3AC_REQUIRE(c.en_coder_depth >= 2, "compressed en_decoder needs en_coder_depth >= 2");

    // Every container of blocks gets its final size here, from the config alone: the walk below fills the blocks in place and none of them
    // moves again — the queued images' targets and the name index point into them.
    ctx->enc_units.resize(c.n_enc);
    for (int i = 0; i < c.n_enc; ++i) ctx->enc_units[i].resize(std::max(c.enc_depths[i], 0));
    ctx->enc_down.resize(c.n_enc - 1);
    ctx->en_enc.resize(compressed ? 2 : 1);
    ctx->en_dec.resize(compressed ? 2 : 1);
    ctx->dec_units.resize(c.n_dec - 1);
    for (int i = 0; i + 1 < c.n_dec; ++i) ctx->dec_units[i].resize(std::max(c.dec_depths[i], 0));
    ctx->dec_enh.resize(c.n_dec - 1);
    ctx->dec_up.resize(c.n_dec - 1);
    ctx->legacy.resize(3);

    Builder b;
    b.ctx = ctx;
    int64_t total = 0;
    for (int i = 0; i < n_tensors; ++i) {
        L3AC_REQUIRE(tensors[i].name && tensors[i].data && tensors[i].numel > 0, "tensor %d is malformed", i);
        b.map[tensors[i].name] = &tensors[i];
        total += tensors[i].numel;
    }
    b.cap = (size_t)total * 2 + (size_t)n_tensors * 128 + (size_t)HEADS * 2 * 8 * (c.en_coder_window_size * c.en_coder_compress_rate + 64) + (1 << 16);
    L3AC_HIP_CHECK(hipMalloc((void**)&ctx->arena, b.cap * sizeof(float)));
    b.dev = ctx->arena;
    b.host.reserve(b.cap);
    ctx->arena_floats = b.cap;

    // ---- encoder (modules.py:71-116): first block, per stage its ConvUnits [and the down layer to the next], output conv ----------------
    // the coders' module lists: each call names the next entry
    int blk = 0;
    auto enc = [&blk] { return "encoder.blocks." + std::to_string(blk++); };
    auto dec = [&blk] { return "decoder.blocks." + std::to_string(blk++); };
    build_first_block(b, ctx->first, enc(), c.enc_dims[0]);
    for (int i = 0; i < c.n_enc; ++i) {
        const std::string stage = enc();
        for (size_t j = 0; j < ctx->enc_units[i].size(); ++j)
            build_conv_unit(b, ctx->enc_units[i][j], stage + "." + std::to_string(j) + ".module", c.enc_dims[i]);
        if (i + 1 == c.n_enc) break;
        L3AC_REQUIRE(c.compress_rates[i] >= 1, "bad compress rate");
        build_down(b, ctx->enc_down[i], enc(), c.enc_dims[i], c.enc_dims[i + 1], c.compress_rates[i], true);
    }
    build_conv_k3(b, ctx->enc_out, enc(), c.enc_dims[c.n_enc - 1], c.feature_dim, false);

    // ---- local-attention stacks in execution order (local_trans.py:56-94, :129-186; en_codec.py:25-44) ------------------------------
    const int win = c.en_coder_window_size;
    if (compressed) {
        const int r = c.en_coder_compress_rate;
        build_local_trans(b, ctx->en_enc[0], "en_encoder.down_trans.trans", win * r, 3 / 2);
        build_local_trans(b, ctx->en_enc[1], "en_encoder.local_trans", win, 3 - 3 / 2);
        build_down(b, ctx->en_down, "en_encoder.down_trans.down_layer", c.feature_dim, c.feature_dim, r, false);
        build_local_trans(b, ctx->en_dec[0], "en_decoder.local_trans", win, c.en_coder_depth - 2);
        build_local_trans(b, ctx->en_dec[1], "en_decoder.up_trans.trans", win * r, 2);
    } else {
        build_local_trans(b, ctx->en_enc[0], "en_encoder.local_trans", win, 1);
        build_local_trans(b, ctx->en_dec[0], "en_decoder.local_trans", win, c.en_coder_depth);
    }

    // ---- quantiser (vq/__init__.py:13-14) -------------------------------------------------------------
    ctx->q_win = b.copy("quantizer.project_in.weight", (int64_t)c.n_levels * c.feature_dim);
    ctx->q_bin = b.copy("quantizer.project_in.bias", c.n_levels);
    ctx->q_wout = b.copy("quantizer.project_out.weight", (int64_t)c.feature_dim * c.n_levels);
    ctx->q_bout = b.copy("quantizer.project_out.bias", c.feature_dim);

    // ---- decoder (modules.py:135-201): input conv, per stage its ConvUnits, EnhanceBlock and up layer, last block ----------------------
    blk = 0;
    build_conv_k3(b, ctx->dec_in, dec(), c.feature_dim, c.dec_dims[0], true);
    for (int i = 0; i + 1 < c.n_dec; ++i) {
        const std::string stage = dec();
        for (size_t j = 0; j < ctx->dec_units[i].size(); ++j)
            build_conv_unit(b, ctx->dec_units[i][j], stage + "." + std::to_string(j) + ".module", c.dec_dims[i]);
        build_enhance(b, ctx->dec_enh[i], dec(), c.dec_dims[i]);
        build_up(b, ctx->dec_up[i], dec(), c.dec_dims[i], c.dec_dims[i + 1], c.decode_rates[i]);
    }
    {
        const std::string last = dec() + ".block";
        const int cl = c.dec_dims[c.n_dec - 1];
        const int dils[3] = {1, 3, 9};
        for (int u = 0; u < 3; ++u) build_legacy_unit(b, ctx->legacy[u], last + ".0." + std::to_string(u) + ".module.block", cl, dils[u]);
        build_head(b, ctx->head, last, cl);
    }
    if (!b.err.empty()) {
        l3ac_set_error("%s", b.err.c_str());
        return L3AC_EWEIGHT;
    }
    L3AC_HIP_CHECK(hipMemcpy(ctx->arena, b.host.data(), b.host.size() * sizeof(float), hipMemcpyHostToDevice));

    // ---- the weight images, each padded to 256 bytes, in one device allocation ---------------------------------------------------------
    {
        auto pad = [](size_t n) { return (n + 255) / 256 * 256; };
        size_t total_img = 0;
        for (const auto& e : b.images) total_img += pad(e.bytes);
        if (total_img) {
            std::vector<unsigned char> himg(total_img, 0);
            L3AC_HIP_CHECK(hipMalloc((void**)&ctx->img_arena, total_img));
            ctx->img_bytes = total_img;
            size_t off = 0;
            for (const auto& e : b.images) {
                e.write(himg.data() + off);
                *e.target = ctx->img_arena + off;
                off += pad(e.bytes);
            }
            L3AC_HIP_CHECK(hipMemcpy(ctx->img_arena, himg.data(), total_img, hipMemcpyHostToDevice));
        }
    }

    L3AC_HIP_CHECK(hipMalloc((void**)&ctx->bad_index_count, sizeof(int)));
    L3AC_HIP_CHECK(hipMemset(ctx->bad_index_count, 0, sizeof(int)));
    L3AC_HIP_CHECK(hipMalloc((void**)&ctx->wide_counters, 64));
    L3AC_HIP_CHECK(hipMemset(ctx->wide_counters, 0, 64));
    if (b.trans_stacks) {  // cooperative form of the transformer stacks (few clips: the streaming chunk): its scratch, counters zeroed ONCE
                           // here — every launch leaves them zeroed again
        L3AC_HIP_CHECK(hipMalloc(&ctx->coop.scratch, trans_stack_coop_bytes()));
        L3AC_HIP_CHECK(hipMemset(ctx->coop.scratch, 0, trans_stack_coop_bytes()));
        // the failure word lives in pinned host memory the device can add to: the host reads it without a device call
        L3AC_HIP_CHECK(hipHostMalloc((void**)&ctx->coop.fail_host, 64, hipHostMallocMapped | hipHostMallocCoherent));
        *ctx->coop.fail_host = 0;
        L3AC_HIP_CHECK(hipHostGetDevicePointer((void**)&ctx->coop.fail_dev, ctx->coop.fail_host, 0));
    }
    {  // GRN guard: starts at +inf
        const float inf = INFINITY;
        L3AC_HIP_CHECK(hipMalloc((void**)&ctx->grn_min_sumsq, sizeof(float)));
        L3AC_HIP_CHECK(hipMemcpy(ctx->grn_min_sumsq, &inf, sizeof(float), hipMemcpyHostToDevice));
    }
    return L3AC_OK;
}

void network_free(l3ac_ctx* ctx) {
    if (ctx->bad_index_count) (void)hipFree(ctx->bad_index_count);
    ctx->bad_index_count = nullptr;
    if (ctx->wide_counters) (void)hipFree(ctx->wide_counters);
    ctx->wide_counters = nullptr;
    trans_coop_release(ctx->coop);
    if (ctx->coop.scratch) (void)hipFree(ctx->coop.scratch);
    ctx->coop.scratch = nullptr;
    if (ctx->coop.fail_host) (void)hipHostFree(ctx->coop.fail_host);
    ctx->coop.fail_host = ctx->coop.fail_dev = nullptr;
    if (ctx->grn_min_sumsq) (void)hipFree(ctx->grn_min_sumsq);
    ctx->grn_min_sumsq = nullptr;
    if (ctx->arena) (void)hipFree(ctx->arena);
    ctx->arena = nullptr;
    if (ctx->img_arena) (void)hipFree(ctx->img_arena);
    ctx->img_arena = nullptr;
    ctx->split_img.clear();
    Workspace& w = ctx->ws;
    for (float** p : {&w.x0, &w.x1, &w.a, &w.h, &w.yi, &w.stats, &w.sumsq}) {
        if (*p) (void)hipFree(*p);
        *p = nullptr;
    }
    if (w.plan) (void)hipFree(w.plan);
    w.plan = nullptr;
}

// ---------------------------------------------------------------------------------------------------------
// workspace
// ---------------------------------------------------------------------------------------------------------
int workspace_ensure(l3ac_ctx* ctx, size_t x_floats, size_t a_floats, size_t h_floats, size_t yi_floats, size_t batch,
                     hipStream_t s) {
    Workspace& w = ctx->ws;
    if (x_floats <= w.x_cap && a_floats <= w.a_cap && h_floats <= w.h_cap && yi_floats <= w.yi_cap && batch <= w.b_cap)
        return L3AC_OK;
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (s) (void)hipStreamIsCapturing(s, &st);
    if (st != hipStreamCaptureStatusNone) {
        l3ac_set_error("workspace too small while the stream is capturing: call l3ac_reserve() first");
        return L3AC_ENOMEM;
    }
    L3AC_HIP_CHECK(hipDeviceSynchronize());  // buffers may still be in use by earlier launches
    auto grow = [&](float*& p, size_t& cap, size_t want, size_t mult) -> int {
        if (want <= cap) return L3AC_OK;
        L3AC_TRY(free_buf(p));
        cap = 0;
        L3AC_HIP_CHECK(hipMalloc((void**)&p, (want * mult + 64) * sizeof(float)));
        cap = want;
        return L3AC_OK;
    };
    const size_t x_want = x_floats > w.x_cap ? x_floats : w.x_cap;
    if (x_want > w.x_cap) {
        L3AC_TRY(free_buf(w.x0));
        L3AC_TRY(free_buf(w.x1));
        w.x_cap = 0;
        L3AC_HIP_CHECK(hipMalloc((void**)&w.x0, (x_want + 64) * sizeof(float)));
        L3AC_HIP_CHECK(hipMalloc((void**)&w.x1, (x_want + 64) * sizeof(float)));
        w.x_cap = x_want;
    }
    L3AC_TRY(grow(w.a, w.a_cap, a_floats, 1));
    L3AC_TRY(grow(w.h, w.h_cap, h_floats, 1));
    L3AC_TRY(grow(w.yi, w.yi_cap, yi_floats, 1));
    if (batch > w.b_cap) {
        L3AC_TRY(free_buf(w.stats));
        L3AC_TRY(free_buf(w.sumsq));
        if (w.plan) L3AC_HIP_CHECK(hipFree(w.plan));
        w.plan = nullptr;
        w.b_cap = 0;
        L3AC_HIP_CHECK(hipMalloc((void**)&w.stats, (batch * 8 + 64) * sizeof(float)));
        L3AC_HIP_CHECK(hipMalloc((void**)&w.sumsq, (batch + 64) * sizeof(float)));
        L3AC_HIP_CHECK(hipMalloc((void**)&w.plan, (batch * RaggedPlan::plan_ints() + 64) * sizeof(int)));
        w.b_cap = batch;
    }
    return L3AC_OK;
}

// h as the scratch of the wide ConvUnit's front end, in floats: bf16x3 planes of whole 32-frame tiles of ALL the call's rows
// (conv_unit_wide_scratch_bytes) — larger than 4C floats per row when there are few rows
static size_t wide_scratch_floats(int c, int64_t rows) { return (conv_unit_wide_scratch_bytes(c, rows) + 3) / 4; }

int workspace_ensure_clip(l3ac_ctx* ctx, int batch, int samples, hipStream_t s) {
    const l3ac_config& c = ctx->cfg;
    size_t x = 0, a = 0, h = 0, yi = 0;
    auto upd = [](size_t& m, int64_t v) { if ((size_t)v > m) m = (size_t)v; };
    int64_t f = round_up64(samples, ctx->hop);
    size_t wide_floats = 0;
    auto wide = [&](int cdim, int64_t fr) {
        if (conv_unit_wide_supported(cdim)) wide_floats = std::max(wide_floats, wide_scratch_floats(cdim, (int64_t)batch * fr));
    };
    for (int i = 0; i < c.n_enc; ++i) {
        upd(x, f * c.enc_dims[i]);
        upd(h, f * 4 * c.enc_dims[i]);
        wide(c.enc_dims[i], f);
        if (i + 1 < c.n_enc) f /= c.compress_rates[i];
    }
    upd(x, f * c.feature_dim);
    const int64_t tr_cols = std::max<int64_t>(std::max<int64_t>(3 * ctx->inner, ctx->ff_n), 4 * c.feature_dim);
    upd(h, f * tr_cols);
    upd(a, f * std::max<int64_t>(ctx->inner, c.feature_dim));
    for (int i = 0; i < c.n_dec; ++i) {
        upd(x, f * c.dec_dims[i]);
        upd(h, f * 4 * c.dec_dims[i]);
        wide(c.dec_dims[i], f);
        upd(yi, f * 4);
        if (i + 1 < c.n_dec) {
            upd(x, f * c.dec_dims[i + 1]);
            f *= c.decode_rates[i];
        }
    }
    upd(a, (int64_t)x);
    return workspace_ensure(ctx, x * batch, a * batch, std::max(h * batch, wide_floats), yi * batch, (size_t)batch, s);
}

// The size limits every block entry shares, asked before the workspace is sized for the call: frame numbers inside a clip are ints with a
// tile and a halo added (dwconv_ln_kernel, the enhance kernels, the LegacyUnit and head kernels, the stem), and 2^34 rows keep every
// kernel's tile count -- tiles of 14 frames and more, plus one per clip -- below 2^31 - 65536
static int op_shape_ok(int batch, int frames) {
    L3AC_REQUIRE(frames <= L3AC_MAX_CLIP_FRAMES, "block entry: %d frames per clip, the limit is 2^31 - 65536 (32-bit frame numbers)", frames);
    L3AC_REQUIRE((int64_t)batch * frames < L3AC_MAX_ROWS, "block entry: batch * frames = %lld, the limit is 2^34 rows (32-bit tile numbers)",
                 (long long)batch * frames);
    return L3AC_OK;
}

// the workspace of one block of at most c_max channels (the l3ac_op_* entries); h: 4C floats per row, or the wide front end's scratch
int workspace_ensure_op(l3ac_ctx* ctx, int batch, int frames, int c_max, hipStream_t s) {
    L3AC_TRY(op_shape_ok(batch, frames));
    const size_t rows = (size_t)batch * frames;
    return workspace_ensure(ctx, rows * c_max, rows * c_max, std::max(rows * 4 * c_max, wide_scratch_floats(c_max, (int64_t)rows)), rows * 4,
                            (size_t)batch, s);
}

// ---------------------------------------------------------------------------------------------------------
// blocks
// ---------------------------------------------------------------------------------------------------------
static inline void swap_bufs(float** a, float** b) {
    float* t = *a;
    *a = *b;
    *b = t;
}

// The form of one ConvUnit call: the wide fused kernel, a narrow fused kernel, or row kernel + GEMMs.  Only the last can run in place
// and only it evaluates the exact GRN; the wide kernel computes on the bf16 matrix cores only (bf16x3), so it belongs to the split route
enum class UnitForm { Wide, Fused, Rows };
static UnitForm conv_unit_form(const l3ac_ctx* ctx, const ConvUnitW& w, bool in_place) {
    if (in_place || ctx->cfg.grn_exact) return UnitForm::Rows;
    if (w.wide_img && ctx->gemm_split && conv_unit_wide_supported(w.c)) return UnitForm::Wide;
    return conv_unit_fused_supported(w.c) ? UnitForm::Fused : UnitForm::Rows;
}

// option "unit_counter": 1 both kernel families hand their units out by the context's counters, 2 the wide ConvUnit only, 3 the
// LegacyUnit only, 0 neither (null = equal static shares)
static int* wide_unit_counters(const l3ac_ctx* ctx) { return ctx->unit_counter == 1 || ctx->unit_counter == 2 ? ctx->wide_counters : nullptr; }
static int* legacy_unit_counters(const l3ac_ctx* ctx) { return ctx->unit_counter == 1 || ctx->unit_counter == 3 ? ctx->wide_counters + 4 : nullptr; }

int conv_unit_step(l3ac_ctx* ctx, hipStream_t s, const ConvUnitW& w, float** cur, float** alt, int batch, int frames) {
    if (conv_unit_form(ctx, w, false) == UnitForm::Rows) return run_conv_unit(ctx, s, w, *cur, *cur, batch, frames);
    L3AC_TRY(run_conv_unit(ctx, s, w, *cur, *alt, batch, frames));
    swap_bufs(cur, alt);
    return L3AC_OK;
}

// a product with one of the context's weights (g.w) on the context's route: its split image — null on the exact route, which then takes
// the fp32 MFMA kernel — and its choice of batch products for gemm_split_kernel_w256
static int gemm_on_route(const l3ac_ctx* ctx, hipStream_t s, GemmArgs g) {
    g.w_img = ctx->img(g.w);
    g.w256 = ctx->gemm_w256;
    return launch_gemm(s, g);
}

// A ragged call (ctx->rag): zero `width` rows after each clip's last frame of x [batch][frames][c] — the zero
// padding the next op, which reads up to `width` frames ahead, sees in the clip alone; duplicate each clip's last frame into the row
// after it ahead of a linear upsampling.  Neither launches anything on the plain path.
static int rag_mask(const l3ac_ctx* ctx, hipStream_t s, float* x, int batch, int frames, int c, int width) {
    const RaggedPlan* r = ctx->rag;
    return r ? launch_ragged_mask(s, x, batch, frames, c, r->n_dev, frames / r->max_tok, width) : L3AC_OK;
}
static int rag_dup(const l3ac_ctx* ctx, hipStream_t s, float* x, int batch, int frames, int c) {
    const RaggedPlan* r = ctx->rag;
    return r ? launch_ragged_dup(s, x, batch, frames, c, r->n_dev, frames / r->max_tok) : L3AC_OK;
}

static int run_conv_unit_rows(l3ac_ctx* ctx, hipStream_t s, const ConvUnitW& w, const float* x, float* y, int batch, int frames) {
    const int64_t rows = (int64_t)batch * frames;
    Workspace& ws = ctx->ws;
    RowArgs r{};  // dw_conv + LayerNorm (modules.py:33-35)
    r.x = x; r.y = ws.a; r.batch = batch; r.frames_in = frames; r.frames_out = frames; r.c = w.c;
    r.src = SRC_DWCONV7; r.norm = NORM_LN; r.dw_w = w.dw_w; r.dw_b = w.dw_b; r.nw = w.ln_w; r.nb = w.ln_b; r.eps = 1e-8f;
    L3AC_TRY(launch_rows(s, r));
    GemmArgs g{};  // pw_conv1 -> snake -> GRN (modules.py:36-38)
    g.a = ws.a; g.lda = w.c; g.w = w.w1; g.ldw = w.c; g.c = ws.h; g.ldc = 4 * w.c; g.m = rows; g.n = 4 * w.c; g.k = w.c;
    g.bias = w.b1; g.alpha = w.alpha; g.inv_alpha = w.inv_alpha; g.gamma = w.gamma; g.beta = w.beta;
    g.epi = ctx->cfg.grn_exact ? EPI_SNAKE : EPI_SNAKE_GRN;
    L3AC_TRY(gemm_on_route(ctx, s, g));
    if (ctx->cfg.grn_exact) {
        L3AC_TRY(launch_grn_sumsq(s, ws.h, batch, (int64_t)frames * 4 * w.c, ws.sumsq));
        L3AC_TRY(launch_grn_apply(s, ws.h, batch, frames, 4 * w.c, ws.sumsq, w.gamma, w.beta, ctx->grn_min_sumsq));
    }
    GemmArgs g2{};  // pw_conv2 + residual (modules.py:39, xtract/nn/layers.py:59-62)
    g2.a = ws.h; g2.lda = 4 * w.c; g2.w = w.w2; g2.ldw = 4 * w.c; g2.c = y; g2.ldc = w.c; g2.m = rows; g2.n = w.c; g2.k = 4 * w.c;
    g2.bias = w.b2; g2.epi = EPI_BIAS_RES; g2.res = x; g2.ldres = w.c;
    return gemm_on_route(ctx, s, g2);
}

static int conv_unit_group(const l3ac_ctx* ctx, const ConvUnitW& w, int batch, int frames);

// All ConvUnits of one stage.  Wide (unfused) units run in place, so the clip-group loop can sit OUTSIDE the units: a
// group's activations then stay in the Infinity Cache from one unit to the next as well.
int run_conv_units(l3ac_ctx* ctx, hipStream_t s, const std::vector<ConvUnitW>& units, float** cur, float** alt, int batch,
                   int frames) {
    if (units.empty()) return L3AC_OK;
    if (conv_unit_form(ctx, units[0], false) != UnitForm::Rows || units.size() == 1 || ctx->rag) {
        for (const ConvUnitW& u : units) {
            L3AC_TRY(rag_mask(ctx, s, *cur, batch, frames, u.c, 3));  // dw_conv k7
            L3AC_TRY(conv_unit_step(ctx, s, u, cur, alt, batch, frames));
        }
        return L3AC_OK;
    }
    const int group = conv_unit_group(ctx, units[0], batch, frames);
    for (int b0 = 0; b0 < batch; b0 += group) {
        const int nb = std::min(group, batch - b0);
        float* xg = *cur + (int64_t)b0 * frames * units[0].c;
        for (const ConvUnitW& u : units) L3AC_TRY(run_conv_unit_rows(ctx, s, u, xg, xg, nb, frames));
    }
    return L3AC_OK;
}

int run_conv_unit(l3ac_ctx* ctx, hipStream_t s, const ConvUnitW& w, const float* x, float* y, int batch, int frames) {
    switch (conv_unit_form(ctx, w, x == y)) {
        case UnitForm::Wide:  // (planes and hidden image in the hidden tensor's buffer: workspace_ensure_clip, workspace_ensure_op)
            return launch_conv_unit_wide(s, w, x, y, reinterpret_cast<unsigned char*>(ctx->ws.h), ctx->ws.h_cap * sizeof(float), batch, frames,
                                         ctx->wide_sliced, wide_unit_counters(ctx));
        case UnitForm::Fused: return launch_conv_unit_fused(s, w, x, y, batch, frames, ctx->gemm_split, ctx->narrow_ring);
        case UnitForm::Rows: break;
    }
    const int group = conv_unit_group(ctx, w, batch, frames);
    for (int b0 = 0; b0 < batch; b0 += group) {
        const int nb = std::min(group, batch - b0);
        const int64_t off = (int64_t)b0 * frames * w.c;
        L3AC_TRY(run_conv_unit_rows(ctx, s, w, x + off, y + off, nb, frames));
    }
    return L3AC_OK;
}

static int conv_unit_group(const l3ac_ctx* ctx, const ConvUnitW& w, int batch, int frames) {
    // Clips are independent, so the unit can run over groups of clips whose hidden tensor (4C floats per frame) stays in the
    // 256 MB Infinity Cache between the two products instead of making an HBM round trip (measured, 1kbps x 256: 19.15 ->
    // 18.65 ms per step at 192 MB; 96 MB and below lose more to the smaller launches than they save).  Option "unit_chunk_mb"
    // sets the target size of that tensor per group (0 = whole batch in one go).
    const int64_t chunk_mb = ctx->unit_chunk_mb;
    const int64_t per_clip = (int64_t)frames * 4 * w.c * sizeof(float);
    int group = batch;
    if (chunk_mb > 0 && !ctx->cfg.grn_exact) group = (int)std::max<int64_t>(1, std::min<int64_t>(batch, (chunk_mb << 20) / per_clip));
    return group;
}

// the one-kernel form of a down layer (down_exact_kernel): the bits of the GEMM + row kernel it replaces, on either route
static bool use_down_exact(const l3ac_ctx* ctx, const DownW& w) { return ctx->down_fused == 2 && w.exact_img && w.nw; }

int run_down(l3ac_ctx* ctx, hipStream_t s, const DownW& w, const float* x, float* y, int batch, int frames) {
    L3AC_REQUIRE(frames % w.stride == 0, "down layer: frames=%d not a multiple of stride %d", frames, w.stride);
    if (use_down_exact(ctx, w) && x != y) return launch_down_exact(s, w, x, y, batch, frames / w.stride);
    const int64_t rows_out = (int64_t)batch * (frames / w.stride);
    GemmArgs g{};  // Conv1d(k = stride): non-overlapping patches are contiguous in the frame-major layout
    g.a = x; g.lda = (int64_t)w.stride * w.cin; g.w = w.w; g.ldw = (int64_t)w.stride * w.cin; g.c = y; g.ldc = w.cout;
    g.m = rows_out; g.n = w.cout; g.k = w.stride * w.cin; g.bias = w.b; g.epi = EPI_BIAS;
    L3AC_TRY(gemm_on_route(ctx, s, g));
    if (w.nw) {  // ChannelNorm channels_first (modules.py:98), in place
        RowArgs r{};
        r.x = y; r.y = y; r.batch = batch; r.frames_in = frames / w.stride; r.frames_out = frames / w.stride; r.c = w.cout;
        r.src = SRC_PLAIN; r.norm = NORM_CN; r.nw = w.nw; r.nb = w.nb; r.eps = 1e-8f;
        L3AC_TRY(launch_rows(s, r));
    }
    return L3AC_OK;
}

int run_conv_k3(l3ac_ctx* ctx, hipStream_t s, const ConvK3W& w, const float* x, float* y, int batch, int frames) {
    GemmArgs g{};
    g.a = x; g.lda = w.cin; g.taps = 3; g.dil = 1; g.cin = w.cin; g.frames = frames;
    g.w = w.w; g.ldw = 3 * w.cin; g.c = y; g.ldc = w.cout; g.m = (int64_t)batch * frames; g.n = w.cout; g.k = 3 * w.cin;
    g.bias = w.b; g.epi = EPI_BIAS;
    return gemm_on_route(ctx, s, g);
}

// the EnhanceBlock's four branch signals of x into ws.yi and their InstanceNorm statistics into ws.stats, each clip over its own frames
static int enhance_branches_stats(l3ac_ctx* ctx, hipStream_t s, const EnhW& w, const float* x, int batch, int frames) {
    Workspace& ws = ctx->ws;
    const RaggedClips rc = ctx->rag ? ctx->rag->clips(frames) : RaggedClips{};
    L3AC_TRY(launch_enhance_branches(s, w.t, x, batch, frames, w.c, ws.yi, ctx->rag ? &rc : nullptr));
    return launch_enhance_stats(s, ws.yi, batch, frames, ws.stats, ctx->rag ? &rc : nullptr);
}

int run_enhance(l3ac_ctx* ctx, hipStream_t s, const EnhW& w, const float* x, float* y, int batch, int frames) {
    Workspace& ws = ctx->ws;
    L3AC_TRY(enhance_branches_stats(ctx, s, w, x, batch, frames));
    RowArgs r{};
    r.x = x; r.y = y; r.batch = batch; r.frames_in = frames; r.frames_out = frames; r.c = w.c;
    r.src = SRC_GATE; r.norm = NORM_NONE; r.yi = ws.yi; r.stats = ws.stats; r.in_w = w.in_w; r.in_b = w.in_b;
    r.gate_w = w.gate_w; r.gate_b = w.gate_b;
    return launch_rows(s, r);
}

// The limit of an up layer in either form (launch_rows SRC_LERP, launch_up_fused): both take the source position of the linear upsampling
// in fp32.  Asked before the layer's first launch, and by the l3ac_op_* entries before they size the workspace.
int up_layer_frames_ok(int frames, int scale) {
    L3AC_REQUIRE((int64_t)frames * scale <= L3AC_MAX_LERP_FRAMES_OUT,
                 "up layer: %d frames x %d: more than 2^23 output frames per clip (fp32 source positions of the linear upsampling)", frames, scale);
    return L3AC_OK;
}

// The limits of a ConvUnit call that depend on the form it takes (run_conv_unit's choice): conv_unit_ring_kernel's clip length
int conv_unit_shape_ok(const l3ac_ctx* ctx, const ConvUnitW& w, bool in_place, int frames) {
    if (conv_unit_form(ctx, w, in_place) == UnitForm::Fused && conv_unit_fused_takes_ring(w, ctx->gemm_split, ctx->narrow_ring))
        return conv_unit_ring_clip_ok(frames, w.c);
    return L3AC_OK;
}

// Upsample(linear) of x [batch][frames][c] by `scale` into y, and the ChannelNorm (nw, nb) of the result where nw is given.  A ragged call
// writes x first: the linear upsampling reads each clip's last frame again from the row after it
static int upsample_rows(l3ac_ctx* ctx, hipStream_t s, float* x, float* y, int batch, int frames, int c, int scale, const float* nw, const float* nb) {
    L3AC_TRY(rag_dup(ctx, s, x, batch, frames, c));
    RowArgs r{};
    r.x = x; r.y = y; r.batch = batch; r.frames_in = frames; r.frames_out = (int64_t)frames * scale; r.c = c;
    r.src = SRC_LERP; r.scale = scale;
    if (nw) { r.norm = NORM_CN; r.nw = nw; r.nb = nb; r.eps = 1e-8f; }
    return launch_rows(s, r);
}

int run_up(l3ac_ctx* ctx, hipStream_t s, const UpW& w, const float* x, float* tmp, float* y, int batch, int frames) {
    L3AC_TRY(up_layer_frames_ok(frames, w.scale));
    GemmArgs g{};  // 1x1 conv (modules.py:161)
    g.a = x; g.lda = w.cin; g.w = w.w; g.ldw = w.cin; g.c = tmp; g.ldc = w.cout; g.m = (int64_t)batch * frames; g.n = w.cout; g.k = w.cin;
    g.bias = w.b; g.epi = EPI_BIAS;
    L3AC_TRY(gemm_on_route(ctx, s, g));
    return upsample_rows(ctx, s, tmp, y, batch, frames, w.cout, w.scale, w.nw, w.nb);  // Upsample(linear) + ChannelNorm (modules.py:162-163)
}

// the one-kernel form of EnhanceBlock gate + up layer (kernels/up_fused.hip): bf16x3 route, the narrow stages' widths
static bool use_up_fused(const l3ac_ctx* ctx, const UpW& w) { return ctx->gemm_split && w.fused_img != nullptr; }

// EnhanceBlock + UpLayer of one decoder stage: the gate is applied inside the up conv's A staging (no pass of its own).
// x is left untouched; tmp holds the conv output at the input rate.
int run_enhance_up(l3ac_ctx* ctx, hipStream_t s, const EnhW& e, const UpW& w, float* x, float* tmp, float* y, int batch, int frames) {
    // separate passes (gate as a row kernel, in place; then the up layer) where the gated GEMM does not cover the geometry — and where
    // the 1x1 conv is wide enough for the bf16x3 route (512 -> 256: the gated fp32-MFMA GEMM ran it at 81 TFLOP/s, 0.173 ms per step
    // and 41 us for a single clip; a memory-bound gate pass + the split GEMM take 0.10 ms / 16 us).  The choice depends on the
    // weight's shape and the context's route only, never on the batch.
    const bool wide_up = ctx->img(w.w) != nullptr && gemm_split_eligible(w.cout, w.cin);
    if (w.cin % 16 != 0 || e.c != w.cin || wide_up) {
        L3AC_REQUIRE(tmp != nullptr, "enhance_up: scratch missing");
        L3AC_TRY(up_layer_frames_ok(frames, w.scale));
        // the pipeline calls this in place (x == y: the gate may overwrite x); any other caller's x is only read, so the gated
        // rows go to the hidden-tensor scratch (free here: the up layer's GEMM writes tmp)
        float* gated = x;
        if (x != y) {
            L3AC_REQUIRE((size_t)batch * frames * e.c <= ctx->ws.h_cap, "enhance_up: workspace too small for the gated rows");
            gated = ctx->ws.h;
        }
        L3AC_TRY(run_enhance(ctx, s, e, x, gated, batch, frames));
        return run_up(ctx, s, w, gated, tmp, y, batch, frames);
    }
    Workspace& ws = ctx->ws;
    L3AC_TRY(up_layer_frames_ok(frames, w.scale));
    L3AC_TRY(enhance_branches_stats(ctx, s, e, x, batch, frames));
    if (use_up_fused(ctx, w) && x != y) {  // gate, conv, upsample and ChannelNorm in one kernel; it reads x while it writes y
        // ragged: the kernel's upsampling clamps at the batch's last frame; with the frame after each clip's last a copy of it (x and yi:
        // the gate and the 1x1 conv are per frame) its lerp gives the clamped form's l0 * x[n - 1] + l1 * x[n - 1]
        L3AC_TRY(rag_dup(ctx, s, x, batch, frames, e.c));
        L3AC_TRY(rag_dup(ctx, s, ws.yi, batch, frames, 4));
        return launch_up_fused(s, e, w, x, ws.yi, ws.stats, y, batch, frames);
    }
    L3AC_REQUIRE(tmp != nullptr, "enhance_up: scratch missing");
    GemmArgs g{};  // gate (tconv/__init__.py:35-44) + 1x1 conv (modules.py:161)
    g.a = x; g.lda = w.cin; g.w = w.w; g.ldw = w.cin; g.c = tmp; g.ldc = w.cout; g.m = (int64_t)batch * frames; g.n = w.cout; g.k = w.cin;
    g.bias = w.b; g.epi = EPI_BIAS;
    g.gate_yi = ws.yi; g.gate_stats = ws.stats; g.gate_in_w = e.in_w; g.gate_in_b = e.in_b; g.gate_w = e.gate_w; g.gate_b = e.gate_b;
    g.gate_frames = frames;
    L3AC_TRY(launch_gemm(s, g));  // (not gemm_on_route: the gated A operand exists in the fp32 kernel only)
    return upsample_rows(ctx, s, tmp, y, batch, frames, w.cout, w.scale, w.nw, w.nb);  // Upsample(linear) + ChannelNorm (modules.py:162-163)
}

// The output stage's form depends on the head's width and the largest dilation only: fused kernels (bf16x3 or exact fp32 by the
// context's route) for every unit and the head, or snake + implicit GEMM + GEMM and snake + head kernel.
static bool last_block_fused(const l3ac_ctx* ctx) {
    int max_dil = 1;
    for (const LegacyW& l : ctx->legacy) max_dil = l.dil > max_dil ? l.dil : max_dil;
    return last_block_fused_supported(ctx->head.c, max_dil);
}

// One LegacyUnit (modules.py:47-64), x -> y.  The fused kernel reads x while it writes y (x != y); the unfused form may run in
// place; only the unfused form uses ws.a / ws.h.
int run_legacy_unit(l3ac_ctx* ctx, hipStream_t s, const LegacyW& l, const float* x, float* y, int batch, int frames) {
    if (last_block_fused(ctx))
        return launch_legacy_unit_fused(s, l, x, y, batch, frames, ctx->gemm_split, legacy_unit_counters(ctx));
    Workspace& ws = ctx->ws;
    const int64_t rows = (int64_t)batch * frames;
    L3AC_TRY(launch_snake(s, x, ws.a, rows, l.c, l.a0, l.ia0));
    GemmArgs g{};
    g.a = ws.a; g.lda = l.c; g.taps = 7; g.dil = l.dil; g.cin = l.c; g.frames = frames;
    g.w = l.w1; g.ldw = 7 * l.c; g.c = ws.h; g.ldc = l.c; g.m = rows; g.n = l.c; g.k = 7 * l.c;
    g.bias = l.b1; g.epi = EPI_SNAKE; g.alpha = l.a1; g.inv_alpha = l.ia1;
    L3AC_TRY(gemm_on_route(ctx, s, g));
    GemmArgs g2{};
    g2.a = ws.h; g2.lda = l.c; g2.w = l.w2; g2.ldw = l.c; g2.c = y; g2.ldc = l.c; g2.m = rows; g2.n = l.c; g2.k = l.c;
    g2.bias = l.b2; g2.epi = EPI_BIAS_RES; g2.res = x; g2.ldres = l.c;
    return gemm_on_route(ctx, s, g2);
}

// Snake1d -> Conv1d(c -> 1, k7) -> Tanh (modules.py:192-194); tanh is left out while the context's head_pretanh switch is on.
// x is only read; the unfused form uses ws.a.
int run_head(l3ac_ctx* ctx, hipStream_t s, const float* x, float* audio, int batch, int frames) {
    const HeadW& hd = ctx->head;
    if (last_block_fused(ctx)) return launch_head_fused(s, hd, x, batch, frames, audio, ctx->head_pretanh);
    L3AC_TRY(launch_snake(s, x, ctx->ws.a, (int64_t)batch * frames, hd.c, hd.alpha, hd.inv_alpha));
    return launch_head(s, ctx->ws.a, batch, frames, hd.c, hd.w, hd.b, audio, ctx->head_pretanh);
}

int run_last_block(l3ac_ctx* ctx, hipStream_t s, float* x, float* audio, int batch, int frames) {
    // fused units ping-pong between x and the scratch buffer; unfused ones run in place (they use the scratch buffer themselves)
    float* cur = x;
    float* alt = last_block_fused(ctx) ? ctx->ws.a : x;
    for (const LegacyW& l : ctx->legacy) {
        L3AC_TRY(rag_mask(ctx, s, cur, batch, frames, l.c, 3 * l.dil));  // k7 at dilation dil
        L3AC_TRY(run_legacy_unit(ctx, s, l, cur, alt, batch, frames));
        swap_bufs(&cur, &alt);
    }
    L3AC_TRY(rag_mask(ctx, s, cur, batch, frames, ctx->head.c, 3));  // head k7
    L3AC_TRY(run_head(ctx, s, cur, audio, batch, frames));
    return rag_mask(ctx, s, audio, batch, frames, 1, frames);  // a clip's samples end with its tokens
}

// the fused stack kernel computes on the bf16 matrix cores only (bf16x3): it belongs to the split route
static bool use_trans_stack(const l3ac_ctx* ctx, const LocalTransW& w, int frames) {
    return ctx->gemm_split && w.stack_img && w.stack_ln &&
           trans_stack_supported(ctx->cfg.feature_dim, ctx->dim_head, HEADS, ctx->ff_inner, frames, w.window, (int)w.layers.size());
}

static int run_local_trans_layers(l3ac_ctx* ctx, hipStream_t s, const LocalTransW& w, float* x, int batch, int frames);

// the whole stack in one launch, one workgroup per clip (six in the cooperative form), at the attention's scale dim_head^-0.5
static int trans_stack(l3ac_ctx* ctx, hipStream_t s, const LocalTransW& w, float* x, int batch, int frames) {
    return launch_trans_stack(s, w, x, batch, frames, (float)std::pow((double)ctx->dim_head, -0.5), &ctx->coop);
}

int run_local_trans(l3ac_ctx* ctx, hipStream_t s, const LocalTransW& w, float* x, int batch, int frames) {
    if (use_trans_stack(ctx, w, frames))
        return trans_stack(ctx, s, w, x, batch, frames);
    return run_local_trans_layers(ctx, s, w, x, batch, frames);
}

// A ragged batch's LocalTrans stack (ctx->rag), x in place, `spare` a free activation buffer.  The stack kernel and the layered route
// do not give the same bits, and which one a clip gets alone depends on its own frame count: so do the clips that would take the stack
// alone (a prefix of RaggedPlan::order: the count is monotone in n_tok) in that kernel, over the largest of their frame counts, and the
// others on the layered route.  Attention is causal, so a clip's rows after its own frames — zero here — never reach its frames.
static int run_local_trans_ragged(l3ac_ctx* ctx, hipStream_t s, const LocalTransW& w, float* x, float* spare, int batch, int frames) {
    const RaggedPlan& r = *ctx->rag;
    const int mult = frames / r.max_tok, dim = ctx->cfg.feature_dim;
    L3AC_TRY(launch_ragged_mask(s, x, batch, frames, dim, r.n_dev, mult, frames));
    int nq = 0;
    while (nq < batch && use_trans_stack(ctx, w, r.n_tok[r.order[nq]] * mult)) ++nq;
    const int fq = nq ? r.n_tok[r.order[nq - 1]] * mult : 0;          // rows of the stack's clips
    const int fl = nq < batch ? r.n_tok[r.order[batch - 1]] * mult : 0;  // rows of the layered route's clips
    if (nq == batch && fq == frames) return run_local_trans(ctx, s, w, x, batch, frames);
    if (nq == 0 && fl == frames) return run_local_trans_layers(ctx, s, w, x, batch, frames);
    // compact copies in `spare`: the stack's clips [nq][fq][dim], then the layered route's [batch - nq][fl][dim]
    const int64_t clip = (int64_t)frames * dim;
    float* q = spare;
    float* l = spare + (int64_t)nq * fq * dim;
    if (nq) L3AC_TRY(launch_ragged_gather(s, x, q, r.order_dev, 0, nq, fq, dim, clip, (int64_t)fq * dim, false));
    if (nq < batch) L3AC_TRY(launch_ragged_gather(s, x, l, r.order_dev, nq, batch - nq, fl, dim, clip, (int64_t)fl * dim, false));
    if (nq) L3AC_TRY(trans_stack(ctx, s, w, q, nq, fq));
    if (nq < batch) L3AC_TRY(run_local_trans_layers(ctx, s, w, l, batch - nq, fl));
    if (nq) L3AC_TRY(launch_ragged_gather(s, q, x, r.order_dev, 0, nq, fq, dim, clip, (int64_t)fq * dim, true));
    if (nq < batch) L3AC_TRY(launch_ragged_gather(s, l, x, r.order_dev, nq, batch - nq, fl, dim, clip, (int64_t)fl * dim, true));
    return L3AC_OK;
}

// one LocalTrans stack of the pipeline, x = *cur in place (*alt is free)
static int local_trans_step(l3ac_ctx* ctx, hipStream_t s, const LocalTransW& w, float** cur, float** alt, int batch, int frames) {
    if (ctx->rag) return run_local_trans_ragged(ctx, s, w, *cur, *alt, batch, frames);
    return run_local_trans(ctx, s, w, *cur, batch, frames);
}

static int run_local_trans_layers(l3ac_ctx* ctx, hipStream_t s, const LocalTransW& w, float* x, int batch, int frames) {
    Workspace& ws = ctx->ws;
    const int dim = ctx->cfg.feature_dim;
    const int64_t rows = (int64_t)batch * frames;
    for (const TransLayerW& l : w.layers) {
        RowArgs r{};  // LocalMHA prenorm
        r.x = x; r.y = ws.a; r.batch = batch; r.frames_in = frames; r.frames_out = frames; r.c = dim;
        r.src = SRC_PLAIN; r.norm = NORM_LN; r.nw = l.ln1w; r.nb = l.ln1b; r.eps = 1e-5f;
        L3AC_TRY(launch_rows(s, r));
        GemmArgs g{};  // to_qkv (no bias)
        g.a = ws.a; g.lda = dim; g.w = l.wqkv; g.ldw = dim; g.c = ws.h; g.ldc = 3 * ctx->inner; g.m = rows; g.n = 3 * ctx->inner; g.k = dim;
        g.epi = EPI_BIAS;
        L3AC_TRY(gemm_on_route(ctx, s, g));
        L3AC_TRY(launch_attention(s, ws.h, ws.a, w.bias_table, batch, frames, HEADS, ctx->dim_head, w.window));
        GemmArgs go{};  // to_out + residual (local_trans.py:45)
        go.a = ws.a; go.lda = ctx->inner; go.w = l.wout; go.ldw = ctx->inner; go.c = x; go.ldc = dim; go.m = rows; go.n = dim; go.k = ctx->inner;
        go.epi = EPI_BIAS_RES; go.res = x; go.ldres = dim;
        L3AC_TRY(gemm_on_route(ctx, s, go));
        r.nw = l.ln2w; r.nb = l.ln2b;  // FeedForward LayerNorm
        L3AC_TRY(launch_rows(s, r));
        GemmArgs f1{};  // Linear(dim, 2*inner) + GEGLU, value/gate tiles interleaved at upload
        f1.a = ws.a; f1.lda = dim; f1.w = l.wff1; f1.ldw = dim; f1.c = ws.h; f1.ldc = ctx->ff_pad; f1.m = rows; f1.n = ctx->ff_n; f1.k = dim;
        f1.epi = EPI_GEGLU; f1.n_out = ctx->ff_inner;
        L3AC_TRY(gemm_on_route(ctx, s, f1));
        GemmArgs f2{};  // Linear(inner, dim) + residual (local_trans.py:46)
        f2.a = ws.h; f2.lda = ctx->ff_pad; f2.w = l.wff2; f2.ldw = ctx->ff_pad; f2.c = x; f2.ldc = dim; f2.m = rows; f2.n = dim; f2.k = ctx->ff_pad;
        f2.epi = EPI_BIAS_RES; f2.res = x; f2.ldres = dim;
        L3AC_TRY(gemm_on_route(ctx, s, f2));
    }
    return L3AC_OK;
}

// ---------------------------------------------------------------------------------------------------------
// sub-modules
// ---------------------------------------------------------------------------------------------------------
int run_encoder(l3ac_ctx* ctx, hipStream_t s, const float* audio, int64_t audio_stride, int batch, int samples,
                int frames, float** cur, float** alt) {
    const l3ac_config& c = ctx->cfg;
    const RaggedClips rc = ctx->rag ? ctx->rag->clips(frames) : RaggedClips{};
    L3AC_TRY(launch_first_block(s, ctx->first, audio, audio_stride, batch, samples, frames, *cur, ctx->rag ? &rc : nullptr));
    int f = frames;
    for (int i = 0; i < c.n_enc; ++i) {
        L3AC_TRY(run_conv_units(ctx, s, ctx->enc_units[i], cur, alt, batch, f));
        if (i + 1 < c.n_enc) {
            L3AC_TRY(run_down(ctx, s, ctx->enc_down[i], *cur, *alt, batch, f));
            swap_bufs(cur, alt);
            f /= c.compress_rates[i];
        }
    }
    L3AC_TRY(rag_mask(ctx, s, *cur, batch, f, c.enc_dims[c.n_enc - 1], 1));  // k3
    L3AC_TRY(run_conv_k3(ctx, s, ctx->enc_out, *cur, *alt, batch, f));
    swap_bufs(cur, alt);
    return L3AC_OK;
}

int run_en_encoder(l3ac_ctx* ctx, hipStream_t s, int batch, int frames, float** cur, float** alt, int* n_tok) {
    // input (B, C, T) permuted to (B, T, C) by the reference (local_trans.py:162): already frame-major here
    L3AC_TRY(local_trans_step(ctx, s, ctx->en_enc[0], cur, alt, batch, frames));
    if (ctx->en_enc.size() == 2) {
        L3AC_TRY(run_down(ctx, s, ctx->en_down, *cur, *alt, batch, frames));
        swap_bufs(cur, alt);
        frames /= ctx->en_down.stride;
        L3AC_TRY(local_trans_step(ctx, s, ctx->en_enc[1], cur, alt, batch, frames));
    }
    *n_tok = frames;
    return L3AC_OK;
}

int run_en_decoder(l3ac_ctx* ctx, hipStream_t s, int batch, int n_tok, float** cur, float** alt, int* frames) {
    L3AC_TRY(local_trans_step(ctx, s, ctx->en_dec[0], cur, alt, batch, n_tok));
    int f = n_tok;
    if (ctx->en_dec.size() == 2) {
        const int r = ctx->cfg.en_coder_compress_rate;
        L3AC_TRY(upsample_rows(ctx, s, *cur, *alt, batch, f, ctx->cfg.feature_dim, r, nullptr, nullptr));  // UpTransV2.up_layer (local_trans.py:121-124)
        swap_bufs(cur, alt);
        f *= r;
        L3AC_TRY(local_trans_step(ctx, s, ctx->en_dec[1], cur, alt, batch, f));
    }
    *frames = f;
    return L3AC_OK;
}

int run_decoder(l3ac_ctx* ctx, hipStream_t s, int batch, int frames, float** cur, float** alt, float* audio) {
    const l3ac_config& c = ctx->cfg;
    L3AC_TRY(rag_mask(ctx, s, *cur, batch, frames, ctx->dec_in.cin, 1));  // k3
    L3AC_TRY(run_conv_k3(ctx, s, ctx->dec_in, *cur, *alt, batch, frames));
    swap_bufs(cur, alt);
    int f = frames;
    for (int i = 0; i + 1 < c.n_dec; ++i) {
        L3AC_TRY(run_conv_units(ctx, s, ctx->dec_units[i], cur, alt, batch, f));
        if (use_up_fused(ctx, ctx->dec_up[i])) {  // the one-kernel form cannot work in place: result in the other buffer
            L3AC_TRY(run_enhance_up(ctx, s, ctx->dec_enh[i], ctx->dec_up[i], *cur, nullptr, *alt, batch, f));
            swap_bufs(cur, alt);
        } else {
            L3AC_TRY(run_enhance_up(ctx, s, ctx->dec_enh[i], ctx->dec_up[i], *cur, *alt, *cur, batch, f));
        }
        f *= c.decode_rates[i];
    }
    return run_last_block(ctx, s, *cur, audio, batch, f);
}
