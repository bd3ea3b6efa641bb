// The life of a handle and its parameters: iodine_create (configuration check, device buffers of every weight pack), iodine_destroy, the
// parameter table's readers and iodine_set_params, which refreshes the packs the selected kernels read (iodine_dispatch.cpp).
#include "iodine_internal.h"

std::string g_create_error;

namespace {

template <typename T>
hipError_t dev_alloc(iodine_handle* h, T** p, size_t n)
{
    void* q = nullptr;
    hipError_t e = hipMalloc(&q, std::max<size_t>(n, 1) * sizeof(T));
    if (e == hipSuccess) { *p = (T*)q; h->owned.push_back(q); }
    return e;
}

std::string validate(const iodine_config& c)
{
    char m[384];
    if (c.encoding & ~IODINE_ENC_FULL) return "ARCH.ENCODING has unknown entries";
    if ((c.encoding & (IODINE_ENC_POSTERIOR | IODINE_ENC_GRAD_POST)) != (IODINE_ENC_POSTERIOR | IODINE_ENC_GRAD_POST))
        return "ARCH.ENCODING must contain 'posterior' and 'grad_post' (the LSTM input of the refinement head is built for both; every "
               "shipped config and lib/config/defaults.py:57-80 have them); any subset of the image-shaped entries is accepted";
    if (!(c.encoding & (IODINE_ENC_FULL & ~(IODINE_ENC_POSTERIOR | IODINE_ENC_GRAD_POST))))
        return "ARCH.ENCODING has no image-shaped entry: the refinement conv stack would have no input";
    if (c.img_channels != 3) return "ARCH.IMG_CHANNELS must be 3";
    // KERNEL_SIZE 3 with 32 / 64 channels runs on the tuned kernels; other odd kernel sizes and channel counts on the generic
    // fallback path (kernels_generic.hip)
    for (int k : {c.dec_kernel_size, c.ref_kernel_size})
        if (k != 3 && k != 5 && k != 7) return "KERNEL_SIZE must be 3, 5 or 7 (odd: the reference pads with KERNEL_SIZE // 2, iodine.py:419,580)";
    if (c.ref_stride < 1 || c.ref_stride > 8) return "REF.STRIDE must be in 1..8 (2: tuned kernels; other strides: generic path)";
    if (c.img_size < 8 || c.img_size > 1024) return "ARCH.IMG_SIZE must be in 8..1024 (multiples of 16 run on the tuned kernels, other sizes on the generic path)";
    if (c.dec_conv_chan < 8 || c.dec_conv_chan > 256 || c.dec_conv_chan % 4 != 0) return "DEC.CONV_CHAN must be a multiple of 4 in 8..256";
    if (c.ref_conv_chan < 4 || c.ref_conv_chan > 256 || 256 % c.ref_conv_chan != 0) return "REF.CONV_CHAN must divide 256 (4 ... 256)";
    if (9 * c.dec_conv_chan < c.dim_latent) return "DIM_LATENT must not exceed 9 * DEC.CONV_CHAN";
    if (c.dec_conv_layers < 1 || c.dec_conv_layers > 32) return "DEC.CONV_LAYERS must be in 1..32";
    if (c.ref_conv_layers < 1 || c.ref_conv_layers > 16 || (c.ref_stride == 2 && (c.img_size >> c.ref_conv_layers) < 1)) return "REF.CONV_LAYERS out of range for IMG_SIZE";
    if (c.slots < 1 || c.slots > 16) return "ARCH.SLOTS must be in 1..16 (the per-pixel kernels keep every slot of a pixel in registers: instantiated for K <= 16)";
    if (c.iters < 1) return "ARCH.ITERS must be >= 1";
    // (the refinement head reads its weight rows as 16-byte vectors: widths that are not multiples of 4 run on a zero-padded inner handle,
    // PadShim - round 6)
    if (c.dim_latent < 2 || c.dim_latent > 256) return "ARCH.DIM_LATENT must be in 2..256";
    if (c.ref_mlp_units < 1 || c.ref_mlp_units > 1024) return "REF.MLP_UNITS must be in 1..1024";
    {
        // the head's LDS budget, on the widths it runs at (rounded up to multiples of 4): its single-launch form keeps 16 slices of the 4H gate
        // partial sums on chip; beyond that only the three-launch form (gate GEMM on fp32 MFMA: 4H a multiple of 32) can run
        const int Hp = (c.ref_mlp_units + 3) / 4 * 4, Lp = (c.dim_latent + 3) / 4 * 4;
        if (refine_head_form(c.ref_conv_chan, Hp, Lp, 1) < 0) {
            snprintf(m, sizeof m, "REF.MLP_UNITS = %d (run at %d) must be a multiple of 8 after rounding up to a multiple of 4, or small enough for the "
                     "refinement head's single-launch form: it needs %zu bytes of LDS, the limit is 98304 (MLP_UNITS up to about 356)",
                     c.ref_mlp_units, Hp, refine_head_lds_bytes(c.ref_conv_chan, Hp, Lp, 0));
            return m;
        }
    }
    if (!(c.sigma > 0)) { snprintf(m, sizeof m, "ARCH.SIGMA must be > 0 (got %g)", c.sigma); return m; }
    return "";
}

// ---- iodine_set_params: what it queues, and its five groups of packs

// Plain copies (biases, raw weights of the head backward) are collected and issued as one launch; (round 5) the head's transposes
// [R][Cc] -> [Cc][R] and the bias sum ride in the same launch.  The split-fp16 packs (power-of-two scale + layout per tensor and direction)
// are collected too and issued as one batched launch at the end.
struct ParamPacker {
    hipStream_t st;
    MultiCopy mc;
    std::vector<PackJob> pj;
    explicit ParamPacker(hipStream_t s) : st(s) { mc.count = 0; }
    hipError_t flush() { const hipError_t e = launch_multi_copy(st, mc); mc.count = 0; return e; }
    hipError_t copy(float* dst, const float* src, size_t count) {
        if (mc.count == MCOPY_MAX) {
            const hipError_t e = flush();
            if (e != hipSuccess) return e;
        }
        mc.src[mc.count] = src; mc.src2[mc.count] = nullptr; mc.dst[mc.count] = dst; mc.n[mc.count] = (int)count; mc.op[mc.count] = 0;
        mc.cols[mc.count] = 0; ++mc.count;
        return hipSuccess;
    }
    hipError_t transpose(float* dst, const float* src, int R, int Cc) {
        const hipError_t e = copy(dst, src, (size_t)R * Cc);
        if (e == hipSuccess) { mc.op[mc.count - 1] = 1; mc.cols[mc.count - 1] = Cc; }
        return e;
    }
    hipError_t add2(float* dst, const float* a, const float* b2, int count) {
        const hipError_t e = copy(dst, a, (size_t)count);
        if (e == hipSuccess) { mc.op[mc.count - 1] = 2; mc.src2[mc.count - 1] = b2; }
        return e;
    }
    hipError_t ws(const float* src, int C, int tflip, float* meta, void* dst) {
        pj.push_back(PackJob{src, dst, meta, 0, {C, tflip, 0, 0, 0}});
        return hipSuccess;
    }
    hipError_t f16(const float* src, int O, int I, int cin, int cout, int tflip, float* meta, void* dst) {
        pj.push_back(PackJob{src, dst, meta, 1, {O, I, cin, cout, tflip}});
        return hipSuccess;
    }
};

// fallback path: [tap][ci][co] packs of every conv, plain bias copies
int pack_decoder_generic(iodine_handle* h, ParamPacker& pk, const float* const* dev)
{
    hipStream_t st = pk.st;
    const ParamSlots& ps = h->slot;
    const int L = h->L, Cd = h->Cd;
    for (int l = 0; l < h->Dd; ++l) {
        HIPCHK(h, launch_gen_pack_weights(st, dev[ps.dec_w[l]], Cd, l == 0 ? L + 2 : Cd, h->kd, h->gen_wdec[l]));
        if (l > 0) HIPCHK(h, pk.copy(h->dec_b[l], dev[ps.dec_b[l]], Cd));
    }
    // bias + the conv of the two coordinate channels of the broadcast layer: the same map for every slot-image
    HIPCHK(h, launch_gen_l0_coord(st, h->gen_wdec[0], dev[ps.dec_b[0]], h->lin, L, h->S, Cd, h->kd, h->gen_cterm));
    HIPCHK(h, launch_gen_pack_weights(st, dev[ps.out_w], 4, Cd, h->kd, h->gen_wout));
    HIPCHK(h, pk.copy(h->dec_out_b, dev[ps.out_b], 4));
    HIPCHK(h, launch_gen_identity(st, h->gen_ident, 9 * Cd, L));
    // gen_conv_precision 1: hi / lo slice images of the C -> C layers, both directions (from the packs above; stream order)
    h->gen_split = h->gen_precision == 1 && gen_split_cch(h->kd, Cd) != 0 && h->Dd > 1;
    if (h->gen_split) {
        if (h->gs_wf.empty()) {
            h->gs_wf.assign(h->Dd, nullptr); h->gs_wb.assign(h->Dd, nullptr); h->gs_mf.assign(h->Dd, nullptr); h->gs_mb.assign(h->Dd, nullptr);
            const size_t pb = gen_split_pack_bytes(h->kd, Cd), mb = sizeof(float) * (size_t)(Cd / 16);
            for (int l = 1; l < h->Dd; ++l)
                for (void** q : {&h->gs_wf[l], &h->gs_wb[l], (void**)&h->gs_mf[l], (void**)&h->gs_mb[l]}) {
                    const hipError_t e_ = hipMalloc(q, q == &h->gs_wf[l] || q == &h->gs_wb[l] ? pb : mb);
                    if (e_ != hipSuccess) {                            // (what was allocated stays in `owned`; the next call starts over)
                        h->gs_wf.clear(); h->gs_wb.clear(); h->gs_mf.clear(); h->gs_mb.clear();
                        return h->fail(IODINE_ERR_HIP, std::string("hipMalloc of the split weight packs: ") + hipGetErrorString(e_));
                    }
                    h->owned.push_back(*q);
                }
        }
        for (int l = 1; l < h->Dd; ++l) {
            HIPCHK(h, launch_gen_split_pack(st, h->gen_wdec[l], h->kd, Cd, 0, h->gs_wf[l], h->gs_mf[l]));
            HIPCHK(h, launch_gen_split_pack(st, h->gen_wdec[l], h->kd, Cd, 1, h->gs_wb[l], h->gs_mb[l]));
        }
    }
    return IODINE_OK;
}

// the generic refinement stack: the same packs, the first layer from its 17 internal channels
int pack_refine_generic(iodine_handle* h, ParamPacker& pk, const float* const* dev)
{
    hipStream_t st = pk.st;
    const ParamSlots& ps = h->slot;
    const int Cr = h->Cr;
    for (int l = 0; l < h->Dr; ++l) {
        const float* w = dev[ps.ref_w[l]];
        if (l == 0 && h->n_in < 17) { HIPCHK(h, launch_enc_expand_weights(st, w, Cr, h->n_in, h->enc_map, h->ref_w17, h->kr * h->kr)); w = h->ref_w17; }
        HIPCHK(h, launch_gen_pack_weights(st, w, Cr, l == 0 ? 17 : Cr, h->kr, h->gen_wref[l]));
        HIPCHK(h, pk.copy(h->ref_b[l], dev[ps.ref_b[l]], Cr));
    }
    return IODINE_OK;
}

// the tuned decoder: only the selected path's packs - the ones dec_conv_fwd / dec_conv_dgrad read - are maintained (a change of
// conv_variant / conv_precision invalidates the parameters)
int pack_decoder_tuned(iodine_handle* h, ParamPacker& pk, const float* const* dev, DecPath path)
{
    hipStream_t st = pk.st;
    const ParamSlots& ps = h->slot;
    const int L = h->L, Cd = h->Cd;
    HIPCHK(h, launch_dec_l0_prepare(st, dev[ps.dec_w[0]], dev[ps.dec_b[0]], h->lin, Cd, L, h->S, h->wcls, h->wclsT, h->cmap));
    for (int l = 1; l < h->Dd; ++l) {
        const float* w = dev[ps.dec_w[l]];
        switch (path) {
        case DEC_WS_F16:                                       // weight-stationary register layout
            HIPCHK(h, pk.ws(w, Cd, 0, h->dec_wmeta[l], h->dec_wsf[l]));
            HIPCHK(h, pk.ws(w, Cd, 1, h->dec_wmeta[l] + 2, h->dec_wsb[l]));
            break;
        case DEC_TILE_F16:
            HIPCHK(h, pk.f16(w, Cd, Cd, Cd, Cd, 0, h->dec_wmeta[l], h->dec_wf16[l]));
            HIPCHK(h, pk.f16(w, Cd, Cd, Cd, Cd, 1, h->dec_wmeta[l] + 2, h->dec_wb16[l]));
            break;
        case DEC_WS_F32:                                       // the same register layout, fp32
            HIPCHK(h, launch_pack_conv_weights_ws32(st, w, Cd, 0, h->dec_wsf[l]));
            HIPCHK(h, launch_pack_conv_weights_ws32(st, w, Cd, 1, h->dec_wsb[l]));
            break;
        case DEC_TILE_F32:
            HIPCHK(h, launch_pack_conv_weights(st, w, Cd, Cd, Cd, Cd, 0, h->dec_wf[l]));
            HIPCHK(h, launch_pack_conv_weights(st, w, Cd, Cd, Cd, Cd, 1, h->dec_wb[l]));
            break;
        case DEC_GENERIC: break;
        }
        HIPCHK(h, pk.copy(h->dec_b[l], dev[ps.dec_b[l]], Cd));
    }
    HIPCHK(h, pk.copy(h->dec_out_b, dev[ps.out_b], 4));
    if (dec_f16(path)) {
        // split-fp16 GEMM-form packs of the output conv, forward and data gradient (one scale): two more jobs of the batched pack
        pk.pj.push_back(PackJob{dev[ps.out_w], h->dec_out_w16, h->dec_out_meta, 3, {Cd, 0, 0, 0, 0}});
        pk.pj.push_back(PackJob{dev[ps.out_w], h->dec_out_wb16, h->dec_out_meta, 4, {Cd, 1, 0, 0, 0}});
    } else {                                                   // exact-fp32 forms of the output conv
        HIPCHK(h, launch_pack_dec_out(st, dev[ps.out_w], h->dec_out_w, Cd));
        HIPCHK(h, launch_pack_conv_weights(st, dev[ps.out_w], 4, Cd, 4, Cd, 1, h->dec_out_wb));
        if (h->dec_out_w32) HIPCHK(h, launch_pack_dec_out_rows32(st, dev[ps.out_w], Cd, h->dec_out_w32));
    }
    return IODINE_OK;
}

// the tuned refinement conv stack: every pack of the family, whatever the per-form options say (they do not invalidate the parameters)
int pack_refine_tuned(iodine_handle* h, ParamPacker& pk, const float* const* dev, RefFamily fam)
{
    hipStream_t st = pk.st;
    const ParamSlots& ps = h->slot;
    const int Cr = h->Cr;
    // first layer: the reference weight has n_in input channels (ARCH.ENCODING subset); the kernels see 17
    const float* w0 = dev[ps.ref_w[0]];
    if (h->n_in < 17) { HIPCHK(h, launch_enc_expand_weights(st, w0, Cr, h->n_in, h->enc_map, h->ref_w17)); w0 = h->ref_w17; }
    for (int l = 0; l < h->Dr; ++l) {
        if (fam == REF_GATHER) HIPCHK(h, launch_pack_conv_weights(st, l == 0 ? w0 : dev[ps.ref_w[l]], Cr, l == 0 ? 17 : Cr, l == 0 ? 20 : Cr, Cr, 0, h->ref_w[l]));
        HIPCHK(h, pk.copy(h->ref_b[l], dev[ps.ref_b[l]], Cr));
    }
    switch (fam) {
    case REF_GATHER: for (int l = 1; l < h->Dr; ++l) HIPCHK(h, launch_pack_conv_weights(st, dev[ps.ref_w[l]], Cr, Cr, Cr, Cr, 2, h->ref_wb[l])); break;
    case REF_S2_F16: case REF_S2_F32: {
        // split fp16: jobs of the batched pack; exact fp32: fp32 weights in the same LDS-tile / register layouts, in the same buffers
        const bool f16 = fam == REF_S2_F16;
        auto tile = [&](const float* w, int I, int cin, int tflip, float* meta, void* dst) {
            return f16 ? pk.f16(w, Cr, I, cin, Cr, tflip, meta, dst) : launch_pack_conv_weights_s2f32(st, w, Cr, I, cin, Cr, tflip, dst);
        };
        for (int l = 0; l < h->Dr; ++l) {
            const float* w = l == 0 ? w0 : dev[ps.ref_w[l]];
            HIPCHK(h, tile(w, l == 0 ? 17 : Cr, l == 0 ? 32 : Cr, 0, h->ref_wmeta[l], h->ref_wf16[l]));
            if (l > 0) HIPCHK(h, tile(w, Cr, Cr, 2, h->ref_wmeta[l] + 2, h->ref_wb16[l]));
        }
        // split first layer (refine_split): the same weights in the internal channel order, packed as two 16-channel convs
        HIPCHK(h, launch_ref_split_weights(st, w0, Cr, h->ref_wk, h->ref_wsh));
        HIPCHK(h, tile(h->ref_wk, 12, 16, 0, h->ref_wkmeta, h->ref_wk16));
        HIPCHK(h, tile(h->ref_wsh, 8, 16, 0, h->ref_wshmeta, h->ref_wsh16));
        if (f16 && ref_pack_l0f(h)) {                          // fused encoding + layer 0: both parts as K = 16 MFMA operands
            pk.pj.push_back(PackJob{h->ref_wk, h->ref_l0k, h->ref_l0kmeta, 2, {Cr, 12, 0, 0, 0}});
            pk.pj.push_back(PackJob{h->ref_wsh, h->ref_l0s, h->ref_l0smeta, 2, {Cr, 8, 0, 0, 0}});
        }
        for (int l = 1; l < h->Dr && ref_pack_ws(h); ++l)       // weight-stationary forward of layers 1 ..
            HIPCHK(h, f16 ? pk.ws(dev[ps.ref_w[l]], Cr, 0, h->ref_wsf_meta[l], h->ref_wsf[l]) : launch_pack_conv_weights_ws32(st, dev[ps.ref_w[l]], Cr, 0, h->ref_wsf[l]));
        if (f16 && ref_pack_bwd01(h))                          // fused layer-1 / layer-0 backward: W1 as the transposed conv's A operand
            HIPCHK(h, pk.ws(dev[ps.ref_w[1]], Cr, 1, h->ref_w1ws_meta, h->ref_w1ws));
        break;
    }
    case REF_GENERIC: break;                                   // (pack_refine_generic)
    }
    return IODINE_OK;
}

// raw copies of the head's weights for its backward GEMMs, then the head as the forward reads it - the same on every path
int pack_head(iodine_handle* h, ParamPacker& pk, const float* const* dev)
{
    const ParamSlots& ps = h->slot;
    const int L = h->L, Cr = h->Cr, H = h->H;
    auto copy_raw = [&](float* dst, int slot) { return pk.copy(dst, dev[slot], h->params[slot].numel()); };
    HIPCHK(h, copy_raw(h->raw_mlp_w, ps.mlp_w));
    HIPCHK(h, copy_raw(h->raw_wih, ps.wih));
    HIPCHK(h, copy_raw(h->raw_whh, ps.whh));
    HIPCHK(h, copy_raw(h->raw_wm, ps.wm));
    HIPCHK(h, copy_raw(h->raw_wv, ps.wv));
    // head
    HIPCHK(h, pk.transpose(h->mlp_wT, dev[ps.mlp_w], H, Cr));
    HIPCHK(h, pk.copy(h->mlp_b, dev[ps.mlp_b], H));
    HIPCHK(h, pk.transpose(h->wihT, dev[ps.wih], 4 * H, H + 4 * L));
    HIPCHK(h, pk.transpose(h->whhT, dev[ps.whh], 4 * H, H));
    HIPCHK(h, pk.add2(h->lstm_b, dev[ps.bih], dev[ps.bhh], 4 * H));
    HIPCHK(h, pk.transpose(h->wmT, dev[ps.wm], L, H));
    HIPCHK(h, pk.transpose(h->wvT, dev[ps.wv], L, H));
    HIPCHK(h, pk.copy(h->bm, dev[ps.bm], L));
    HIPCHK(h, pk.copy(h->bv, dev[ps.bv], L));
    HIPCHK(h, pk.copy(h->init_mean, dev[ps.init_mean], L));
    HIPCHK(h, pk.copy(h->init_logvar, dev[ps.init_logvar], L));
    return IODINE_OK;
}

}  // namespace

extern "C" {

int iodine_create(const iodine_config* cfg, iodine_handle** out)
{
    if (out) *out = nullptr;
    if (!cfg || !out) { g_create_error = "null argument"; return IODINE_ERR_INVALID; }
    const std::string why = validate(*cfg);
    if (!why.empty()) { g_create_error = why; return IODINE_ERR_INVALID; }
    iodine_handle* h = new iodine_handle();
    h->cfg = *cfg;
    h->obj.sigma = cfg->sigma;
    if (cfg->dim_latent % 4 != 0 || cfg->ref_mlp_units % 4 != 0) {
        // boundary handle of a zero-padded inner handle (iodine_pad.cpp): owns the reference-shaped parameter table and the maps only
        h->n_in = 0;
        for (unsigned bit = 0; bit < 12; ++bit) {
            static const int cnt[12] = {0, 0, 3, 3, 1, 1, 1, 3, 1, 1, 1, 2};      // channels per ENCODING entry, order of the IODINE_ENC_* bits
            if (cfg->encoding & (1u << bit)) h->n_in += cnt[bit];
        }
        build_param_table(h);
        const int rc = pad_create(h);
        if (rc) { iodine_destroy(h); return rc; }
        *out = h;
        return IODINE_OK;
    }
    h->L = cfg->dim_latent; h->T = cfg->iters; h->K = cfg->slots; h->S = cfg->img_size; h->P = h->S * h->S;
    h->Cd = cfg->dec_conv_chan; h->Dd = cfg->dec_conv_layers; h->Cr = cfg->ref_conv_chan; h->Dr = cfg->ref_conv_layers;
    h->H = cfg->ref_mlp_units;
    h->kd = cfg->dec_kernel_size; h->kr = cfg->ref_kernel_size; h->rs = cfg->ref_stride;
    h->generic = h->kd != 3 || (h->Cd != 32 && h->Cd != 64) || h->S % 16 != 0;
    h->gen_ref = h->kr != 3 || (h->Cr != 32 && h->Cr != 64) || h->S % 16 != 0 || h->rs != 2;
    {
        // image-shaped entries in CODE order (iodine.py:277-340) with their channel counts
        static const struct { unsigned bit; int first, count; } ent[10] = {
            {IODINE_ENC_IMAGE, 0, 3}, {IODINE_ENC_MEANS, 3, 3}, {IODINE_ENC_MASK, 6, 1}, {IODINE_ENC_MASK_LOGITS, 7, 1},
            {IODINE_ENC_MASK_POSTERIOR, 8, 1}, {IODINE_ENC_GRAD_MEANS, 9, 3}, {IODINE_ENC_GRAD_MASK, 12, 1},
            {IODINE_ENC_LIKELIHOOD, 13, 1}, {IODINE_ENC_LEAVE_ONE_OUT, 14, 1}, {IODINE_ENC_COORDINATE, 15, 2}};
        h->n_in = 0;
        for (const auto& e : ent)
            if (cfg->encoding & e.bit) for (int q = 0; q < e.count; ++q) h->enc_map[h->n_in++] = e.first + q;
        for (int j = h->n_in; j < 17; ++j) h->enc_map[j] = -1;
        h->enc_chmask = 0;
        for (int j = 0; j < h->n_in; ++j) h->enc_chmask |= 1u << h->enc_map[j];
    }
    build_param_table(h);

    auto bail = [&](hipError_t e, const char* what) {
        g_create_error = std::string(what) + ": " + hipGetErrorString(e);
        iodine_destroy(h);
        return IODINE_ERR_HIP;
    };
#define ALLOC(ptr, n) do { hipError_t e_ = dev_alloc(h, &(ptr), (n)); if (e_ != hipSuccess) return bail(e_, "hipMalloc " #ptr); } while (0)
    const int L = h->L, Cd = h->Cd, Cr = h->Cr, H = h->H;
    ALLOC(h->lin, (size_t)h->S);
    ALLOC(h->wcls, (size_t)9 * L * Cd);
    ALLOC(h->wclsT, (size_t)9 * L * Cd);
    ALLOC(h->cmap, (size_t)h->P * Cd);
    h->dec_wf.assign(h->Dd, nullptr); h->dec_wb.assign(h->Dd, nullptr); h->dec_b.assign(h->Dd, nullptr);
    h->dec_wf16.assign(h->Dd, nullptr); h->dec_wb16.assign(h->Dd, nullptr); h->dec_wmeta.assign(h->Dd, nullptr);
    h->dec_wsf.assign(h->Dd, nullptr); h->dec_wsb.assign(h->Dd, nullptr);
    for (int l = 1; l < h->Dd; ++l) {
        ALLOC(h->dec_wsf[l], conv_ws_wpk_bytes(Cd) / 4);
        ALLOC(h->dec_wsb[l], conv_ws_wpk_bytes(Cd) / 4);
        ALLOC(h->dec_wf[l], conv_wpk_elems(Cd, Cd) * 4);
        ALLOC(h->dec_wb[l], conv_wpk_elems(Cd, Cd) * 4);
        ALLOC(h->dec_b[l], (size_t)Cd);
        ALLOC(h->dec_wf16[l], (size_t)(Cd / 16) * 9 * 2 * 2 * Cd * 4);      // fp16 x 8 per uint4 = 4 floats
        ALLOC(h->dec_wb16[l], (size_t)(Cd / 16) * 9 * 2 * 2 * Cd * 4);
        ALLOC(h->dec_wmeta[l], (size_t)4);
    }
    ALLOC(h->dec_out_w, (size_t)9 * Cd * 4);
    if (Cd == 64 || Cd == 32) ALLOC(h->dec_out_w32, (size_t)2 * (Cd / 2) * 64);
    ALLOC(h->dec_out_b, (size_t)4);
    ALLOC(h->dec_out_wb, conv_wpk_elems(4, Cd) * 4);
    ALLOC(h->dec_out_w16, (size_t)(Cd / 16) * 2 * 2 * 64 * 4);            // GEMM-form pack: [chunk][hi/lo][kh][64][8 fp16]
    ALLOC(h->dec_out_meta, (size_t)4);
    ALLOC(h->dec_out_wb16, (size_t)3 * 2 * 2 * Cd * 4);
    // refinement conv stack: the packs of every tuned family (ref_family() changes with conv_precision), the optional ones by ref_pack_*()
    for (auto* v : {&h->ref_w, &h->ref_b, &h->ref_wb, &h->ref_wf16, &h->ref_wb16, &h->ref_wmeta, &h->ref_wsf, &h->ref_wsf_meta}) v->assign(h->Dr, nullptr);
    for (int l = 0; l < h->Dr; ++l) {
        ALLOC(h->ref_w[l], conv_wpk_elems(l == 0 ? 20 : Cr, Cr) * 4); ALLOC(h->ref_b[l], (size_t)Cr);
        ALLOC(h->ref_wf16[l], (size_t)((l == 0 ? 32 : Cr) / 16) * 9 * 2 * 2 * Cr * 4); ALLOC(h->ref_wmeta[l], (size_t)4);
        if (l == 0) continue;
        ALLOC(h->ref_wb[l], conv_wpk_elems(Cr, Cr) * 4); ALLOC(h->ref_wb16[l], (size_t)(Cr / 16) * 9 * 2 * 2 * Cr * 4);
        if (ref_pack_ws(h)) { ALLOC(h->ref_wsf[l], conv_ws_wpk_bytes(Cr) / 4); ALLOC(h->ref_wsf_meta[l], (size_t)4); }
    }
    ALLOC(h->mlp_wT, (size_t)Cr * H); ALLOC(h->mlp_b, (size_t)H);
    ALLOC(h->wihT, (size_t)(H + 4 * L + H) * 4 * H);         // [W_ih^T ; W_hh^T] contiguous: one K-major operand for the gate GEMM (head_mfma)
    h->whhT = h->wihT + (size_t)(H + 4 * L) * 4 * H;
    ALLOC(h->lstm_b, (size_t)4 * H);
    ALLOC(h->wmT, (size_t)H * L); ALLOC(h->bm, (size_t)L); ALLOC(h->wvT, (size_t)H * L); ALLOC(h->bv, (size_t)L);
    ALLOC(h->init_mean, (size_t)L); ALLOC(h->init_logvar, (size_t)L);
    ALLOC(h->raw_mlp_w, (size_t)H * Cr); ALLOC(h->raw_wih, (size_t)4 * H * (H + 4 * L)); ALLOC(h->raw_whh, (size_t)4 * H * H);
    ALLOC(h->raw_wm, (size_t)L * H); ALLOC(h->raw_wv, (size_t)L * H);
    // split first layer: one 16-channel chunk each for the per-slot (12 real) and the per-image (8 real) channels
    ALLOC(h->ref_wk, (size_t)Cr * 12 * 9); ALLOC(h->ref_wsh, (size_t)Cr * 8 * 9); ALLOC(h->ref_g20, (size_t)Cr * 20 * 9);
    if (ref_pack_bwd01(h)) { ALLOC(h->ref_w1ws, conv_ws_wpk_bytes(Cr) / 4); ALLOC(h->ref_w1ws_meta, (size_t)4); }
    ALLOC(h->ref_w17, (size_t)Cr * 17 * h->kr * h->kr); ALLOC(h->ref_g17, (size_t)Cr * 17 * h->kr * h->kr);
    if (dec_path(h) == DEC_GENERIC) {
        const int kkd = h->kd * h->kd;
        h->gen_wdec.assign(h->Dd, nullptr);
        for (int l = 0; l < h->Dd; ++l) ALLOC(h->gen_wdec[l], (size_t)kkd * (l == 0 ? L + 2 : Cd) * Cd);
        ALLOC(h->gen_wout, (size_t)kkd * Cd * 4); ALLOC(h->gen_cterm, (size_t)h->P * Cd); ALLOC(h->gen_ident, (size_t)9 * Cd * L);
    }
    if (ref_family(h) == REF_GENERIC) {
        const int kkr = h->kr * h->kr;
        h->gen_wref.assign(h->Dr, nullptr);
        for (int l = 0; l < h->Dr; ++l) ALLOC(h->gen_wref[l], (size_t)kkr * (l == 0 ? 17 : Cr) * Cr);
    }
    ALLOC(h->ref_wk16, (size_t)9 * 2 * 2 * Cr * 4); ALLOC(h->ref_wsh16, (size_t)9 * 2 * 2 * Cr * 4);
    ALLOC(h->ref_wkmeta, (size_t)4); ALLOC(h->ref_wshmeta, (size_t)4);
    {
        float* c_ = nullptr;
        ALLOC(c_, (size_t)4);
        h->elbo_counter = reinterpret_cast<unsigned*>(c_);
        if (hipError_t e_ = hipMemset(c_, 0, 16); e_ != hipSuccess) return bail(e_, "hipMemset elbo_counter");
    }
    if (Cr % 16 == 0) {
        float *pk = nullptr, *ps = nullptr;
        ALLOC(pk, refine_l0_wpk_bytes(Cr) / 4); ALLOC(ps, refine_l0_wpk_bytes(Cr) / 4); ALLOC(h->ref_l0kmeta, (size_t)4); ALLOC(h->ref_l0smeta, (size_t)4);
        h->ref_l0k = pk; h->ref_l0s = ps;
    }
    // gradient accumulators: ONE buffer, parameters back to back in named_parameters() order (the layout the wrapper's
    // flat gradient buffer has too), so that zeroing and the final scale-and-add are one launch each
    h->gacc.assign(h->params.size(), nullptr);
    h->gacc_total = 0;
    for (size_t i = 0; i < h->params.size(); ++i) h->gacc_total += h->params[i].numel();
    ALLOC(h->gacc_arena, h->gacc_total);
    {
        size_t off = 0;
        for (size_t i = 0; i < h->params.size(); ++i) { h->gacc[i] = h->gacc_arena + off; off += h->params[i].numel(); }
    }
#undef ALLOC
    std::vector<float> lin(h->S);
    iodine_linspace_host(h->S, lin.data());
    hipError_t e = hipMemcpy(h->lin, lin.data(), sizeof(float) * h->S, hipMemcpyHostToDevice);
    if (e != hipSuccess) return bail(e, "hipMemcpy linspace");
    *out = h;
    return IODINE_OK;
}

void iodine_destroy(iodine_handle* h)
{
    if (!h) return;
    if (h->shim) pad_destroy(h);
    for (void* p : h->owned) (void)hipFree(p);
    for (auto& t : h->wtabs) if (t.dev) (void)hipFree(t.dev);
    for (auto& c : h->prof) for (auto& e : c.ev) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
    if (h->ws_own) (void)hipFree(h->ws_own);
    drop_graphs(h);
    delete h;
}

int iodine_num_params(const iodine_handle* h) { return h ? (int)h->params.size() : 0; }

int iodine_param_info(const iodine_handle* h, int index, const char** name, int* ndim, long long dims[4])
{
    if (!h || index < 0 || index >= (int)h->params.size()) return IODINE_ERR_INVALID;
    const ParamInfo& p = h->params[index];
    if (name) *name = p.name.c_str();
    if (ndim) *ndim = p.ndim;
    if (dims) for (int i = 0; i < 4; ++i) dims[i] = p.dims[i];
    return IODINE_OK;
}

int iodine_set_params(iodine_handle* h, void* stream, const float* const* dev, int n)
{
    if (!h) return IODINE_ERR_INVALID;
    if (h->shim) return pad_set_params(h, stream, dev, n);
    if (int rc = set_params_check(h, dev, n)) return rc;
    ParamPacker pk((hipStream_t)stream);
    // The order is the stream order the packs depend on: the generic stack's packs in front of the tuned decoder's, the other families'
    // behind; the batched pack last, behind the ref_split / enc_expand launches whose outputs it reads.
    const DecPath path = dec_path(h);
    const RefFamily fam = ref_family(h);
    if (path == DEC_GENERIC) { if (int r = pack_decoder_generic(h, pk, dev)) return r; }
    if (fam == REF_GENERIC) { if (int r = pack_refine_generic(h, pk, dev)) return r; }
    if (path != DEC_GENERIC) { if (int r = pack_decoder_tuned(h, pk, dev, path)) return r; }
    if (fam != REF_GENERIC) { if (int r = pack_refine_tuned(h, pk, dev, fam)) return r; }
    if (int r = pack_head(h, pk, dev)) return r;
    HIPCHK(h, pk.flush());
    if (!pk.pj.empty()) HIPCHK(h, launch_pack_batch(pk.st, pk.pj.data(), (int)pk.pj.size()));
    h->params_set = true;
    h->calls.saved_passes_gone();
    return IODINE_OK;
}

}  // extern "C"
