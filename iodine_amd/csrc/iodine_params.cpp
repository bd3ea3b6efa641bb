// The life of a handle and its parameters: iodine_create (configuration check, device buffers of every weight pack), iodine_destroy, the
// parameter table's readers and iodine_set_params, which refreshes the packs the selected kernels read (iodine_dispatch.cpp).
#include "iodine_internal.h"

thread_local std::string g_create_error;

namespace {

// The device buffers of iodine_create: one hipMalloc each, owned by the handle (iodine_destroy frees h->owned).  The first failure is kept
// and turns every later request into a no-op, so the alloc_* functions below read as plain lists; iodine_create looks at `err` once.
struct DevAlloc {
    iodine_handle* h;
    const char* group = "";                     // what was being allocated when `err` was set, for the message
    hipError_t err = hipSuccess;
    void in(const char* g) { if (err == hipSuccess) group = g; }
    void* bytes(size_t n) {
        void* q = nullptr;
        if (err == hipSuccess && (err = hipMalloc(&q, std::max(n, sizeof(float)))) == hipSuccess) h->owned.push_back(q);
        return err == hipSuccess ? q : nullptr;
    }
    float* f32(size_t bytes_) { return (float*)bytes(bytes_); }
    float* floats(size_t n) { return f32(n * sizeof(float)); }
    // a pack of `n` bytes (pack_geom.h) with the meta block it is given (second: its data-gradient half), or one of its own
    Pack pack(size_t n) { void* d = bytes(n); return Pack{d, floats(WPK_META_FLOATS)}; }
    Pack pack(size_t n, float* meta, bool second = false) { return Pack{bytes(n), meta && second ? meta + 2 : meta}; }
};

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

// Plain copies (biases, raw weights of the head backward), the head's transposes and the bias sum ride in one launch (CopyBatch).  The
// split-fp16 packs (power-of-two scale + layout per tensor and direction) are collected too and issued as one batched launch at the end.
struct ParamPacker : CopyBatch {
    std::vector<PackJob> pj;
    using CopyBatch::CopyBatch;
    // jobs of the batched pack (kernels_pack.hip): the scale goes to p.meta, the pack to p.data
    hipError_t job(int kind, const float* src, const Pack& p, int p0, int p1 = 0, int p2 = 0, int p3 = 0, int p4 = 0) {
        pj.push_back(PackJob{src, p.data, p.meta, kind, {p0, p1, p2, p3, p4}});
        return hipSuccess;
    }
    hipError_t ws(const float* src, int C, int tflip, const Pack& p) { return job(0, src, p, C, tflip); }
    hipError_t f16(const float* src, int O, int I, int cin, int cout, int tflip, const Pack& p) { return job(1, src, p, O, I, cin, cout, tflip); }
};

// ---- DEC_GENERIC.  Allocated here (iodine_create, on that path only), filled below, read by decoder_forward / decoder_backward_generic
void alloc_decoder_generic(iodine_handle* h, DevAlloc& da)
{
    GenPacks& g = h->gen;
    const int L = h->L, Cd = h->Cd, k = h->kd;
    da.in("generic decoder packs");
    g.wdec.assign(h->Dd, nullptr);
    for (int l = 0; l < h->Dd; ++l) g.wdec[l] = da.f32(wpk_gen_bytes(k, l == 0 ? L + 2 : Cd, Cd));
    g.wout = da.f32(wpk_gen_bytes(k, Cd, 4)); g.cterm = da.floats((size_t)h->P * Cd); g.ident = da.floats((size_t)9 * Cd * L);
}

// gen_conv_precision 1: the slice images of layers 1 .., both directions - by the first iodine_set_params that needs them
int alloc_gen_split(iodine_handle* h)
{
    GenPacks& g = h->gen;
    if (!g.split_f.empty()) return IODINE_OK;
    DevAlloc da{h};
    g.split_f.assign(h->Dd, Pack()); g.split_b.assign(h->Dd, Pack());
    const size_t pb = gen_split_pack_bytes(h->kd, h->Cd), mb = sizeof(float) * wpk_gen_split_meta_floats(h->Cd);
    for (int l = 1; l < h->Dd; ++l)
        for (Pack* p : {&g.split_f[l], &g.split_b[l]}) { p->data = da.bytes(pb); p->meta = da.f32(mb); }
    if (da.err == hipSuccess) return IODINE_OK;
    g.split_f.clear(); g.split_b.clear();                          // (what was allocated stays in `owned`; the next call starts over)
    return h->fail(IODINE_ERR_HIP, std::string("hipMalloc of the split weight packs: ") + hipGetErrorString(da.err));
}

// fallback path: [tap][ci][co] packs of every conv, plain bias copies
int pack_decoder_generic(iodine_handle* h, ParamPacker& pk, const float* const* dev)
{
    hipStream_t st = pk.st;
    const ParamSlots& ps = h->slot;
    GenPacks& g = h->gen;
    const int L = h->L, Cd = h->Cd;
    for (int l = 0; l < h->Dd; ++l) {
        HIPCHK(h, launch_gen_pack_weights(st, dev[ps.dec_w[l]], Cd, l == 0 ? L + 2 : Cd, h->kd, g.wdec[l]));
        if (l > 0) HIPCHK(h, pk.copy(h->dec.bias[l], dev[ps.dec_b[l]], Cd));
    }
    // bias + the conv of the two coordinate channels of the broadcast layer: the same map for every slot-image
    HIPCHK(h, launch_gen_l0_coord(st, g.wdec[0], dev[ps.dec_b[0]], h->lin, L, h->S, Cd, h->kd, g.cterm));
    HIPCHK(h, launch_gen_pack_weights(st, dev[ps.out_w], 4, Cd, h->kd, g.wout));
    HIPCHK(h, pk.copy(h->dec.out.bias, dev[ps.out_b], 4));
    HIPCHK(h, launch_gen_identity(st, g.ident, 9 * Cd, L));
    // gen_conv_precision 1: hi / lo slice images of the C -> C layers, both directions (from the packs above; stream order)
    g.split_on = h->opt.gen_precision == 1 && gen_split_cch(h->kd, Cd) != 0 && h->Dd > 1;
    if (g.split_on) {
        if (int rc = alloc_gen_split(h)) return rc;
        for (int l = 1; l < h->Dd; ++l) {
            HIPCHK(h, launch_gen_split_pack(st, g.wdec[l], h->kd, Cd, 0, g.split_f[l].data, g.split_f[l].meta));
            HIPCHK(h, launch_gen_split_pack(st, g.wdec[l], h->kd, Cd, 1, g.split_b[l].data, g.split_b[l].meta));
        }
    }
    return IODINE_OK;
}

// ---- REF_GENERIC.  Allocated on that family only; read by ref_conv_fwd / ref_conv_dgrad (biases, w17: alloc_refine_tuned)
void alloc_refine_generic(iodine_handle* h, DevAlloc& da)
{
    da.in("generic refinement packs");
    h->gen.wref.assign(h->Dr, nullptr);
    for (int l = 0; l < h->Dr; ++l) h->gen.wref[l] = da.f32(wpk_gen_bytes(h->kr, l == 0 ? 17 : h->Cr, h->Cr));
}

// the generic refinement stack: the same packs, the first layer from its 17 internal channels
int pack_refine_generic(iodine_handle* h, ParamPacker& pk, const float* const* dev)
{
    hipStream_t st = pk.st;
    const ParamSlots& ps = h->slot;
    const int Cr = h->Cr;
    for (int l = 0; l < h->Dr; ++l) {
        const float* w = dev[ps.ref_w[l]];
        if (l == 0 && h->n_in < 17) { HIPCHK(h, launch_enc_expand_weights(st, w, Cr, h->n_in, h->enc_map, h->ref.w17, h->kr * h->kr)); w = h->ref.w17; }
        HIPCHK(h, launch_gen_pack_weights(st, w, Cr, l == 0 ? 17 : Cr, h->kr, h->gen.wref[l]));
        HIPCHK(h, pk.copy(h->ref.bias[l], dev[ps.ref_b[l]], Cr));
    }
    return IODINE_OK;
}

// ---- the tuned decoder.  Every path's packs are allocated for every handle (conv_precision / conv_variant change the path; the bias
// copies serve the generic path too); read by dec_conv_fwd / dec_conv_dgrad / dec_out_dgrad / decoder_forward on the path named in DecPacks
void alloc_decoder_tuned(iodine_handle* h, DevAlloc& da)
{
    DecPacks& d = h->dec;
    const int L = h->L, Cd = h->Cd, Dd = h->Dd;
    da.in("decoder packs");
    d.wcls = da.floats((size_t)9 * L * Cd); d.wclsT = da.floats((size_t)9 * L * Cd); d.cmap = da.floats((size_t)h->P * Cd);
    d.bias.assign(Dd, nullptr); d.tile32_f.assign(Dd, nullptr); d.tile32_b.assign(Dd, nullptr);
    for (auto* v : {&d.ws_f, &d.ws_b, &d.tile_f, &d.tile_b}) v->assign(Dd, Pack());
    for (int l = 1; l < Dd; ++l) {
        float* meta = da.floats(WPK_META_FLOATS);                   // one block per layer: the forward pair, then the data gradient's
        d.ws_f[l] = da.pack(wpk_ws_bytes(Cd), meta); d.ws_b[l] = da.pack(wpk_ws_bytes(Cd), meta, true);
        d.tile32_f[l] = da.f32(wpk_tile_f32_bytes(Cd, Cd)); d.tile32_b[l] = da.f32(wpk_tile_f32_bytes(Cd, Cd));
        d.bias[l] = da.floats((size_t)Cd);
        d.tile_f[l] = da.pack(wpk_tile_f16_bytes(Cd, Cd), meta); d.tile_b[l] = da.pack(wpk_tile_f16_bytes(Cd, Cd), meta, true);
    }
    d.out.taps = da.f32(wpk_out_taps_bytes(Cd));
    if (Cd == 64 || Cd == 32) d.out.rows32 = da.f32(wpk_out_rows32_bytes(Cd));
    d.out.bias = da.floats((size_t)4);
    d.out.dgrad32 = da.f32(wpk_tile_f32_bytes(4, Cd));
    d.out.gemm = da.pack(wpk_out_gemm_bytes(Cd));
    d.out.dgrad = da.pack(wpk_out_dgrad_bytes(Cd), d.out.gemm.meta);      // (one scale for both forms)
}

// only the selected path's packs - the ones dec_conv_fwd / dec_conv_dgrad read - are maintained (a change of
// conv_variant / conv_precision invalidates the parameters)
int pack_decoder_tuned(iodine_handle* h, ParamPacker& pk, const float* const* dev, DecPath path)
{
    hipStream_t st = pk.st;
    const ParamSlots& ps = h->slot;
    DecPacks& d = h->dec;
    const int L = h->L, Cd = h->Cd;
    HIPCHK(h, launch_dec_l0_prepare(st, dev[ps.dec_w[0]], dev[ps.dec_b[0]], h->lin, Cd, L, h->S, d.wcls, d.wclsT, d.cmap));
    for (int l = 1; l < h->Dd; ++l) {
        const float* w = dev[ps.dec_w[l]];
        switch (path) {                                        // (forward, then the data gradient: the transposed conv)
        case DEC_WS_F16: HIPCHK(h, pk.ws(w, Cd, 0, d.ws_f[l])); HIPCHK(h, pk.ws(w, Cd, 1, d.ws_b[l])); break;       // weight-stationary register layout
        case DEC_TILE_F16: HIPCHK(h, pk.f16(w, Cd, Cd, Cd, Cd, 0, d.tile_f[l])); HIPCHK(h, pk.f16(w, Cd, Cd, Cd, Cd, 1, d.tile_b[l])); break;
        case DEC_WS_F32:                                       // the same register layout, fp32
            HIPCHK(h, launch_pack_conv_weights_ws32(st, w, Cd, 0, d.ws_f[l].data)); HIPCHK(h, launch_pack_conv_weights_ws32(st, w, Cd, 1, d.ws_b[l].data));
            break;
        case DEC_TILE_F32:
            HIPCHK(h, launch_pack_conv_weights(st, w, Cd, Cd, Cd, Cd, 0, d.tile32_f[l])); HIPCHK(h, launch_pack_conv_weights(st, w, Cd, Cd, Cd, Cd, 1, d.tile32_b[l]));
            break;
        case DEC_GENERIC: break;
        }
        HIPCHK(h, pk.copy(d.bias[l], dev[ps.dec_b[l]], Cd));
    }
    HIPCHK(h, pk.copy(d.out.bias, dev[ps.out_b], 4));
    if (dec_f16(path)) {
        // split-fp16 GEMM-form packs of the output conv, forward and data gradient (one scale): two more jobs of the batched pack
        HIPCHK(h, pk.job(3, dev[ps.out_w], d.out.gemm, Cd, 0));
        HIPCHK(h, pk.job(4, dev[ps.out_w], d.out.dgrad, Cd, 1));
    } else {                                                   // exact-fp32 forms of the output conv
        HIPCHK(h, launch_pack_dec_out(st, dev[ps.out_w], d.out.taps, Cd));
        HIPCHK(h, launch_pack_conv_weights(st, dev[ps.out_w], 4, Cd, 4, Cd, 1, d.out.dgrad32));
        if (d.out.rows32) HIPCHK(h, launch_pack_dec_out_rows32(st, dev[ps.out_w], Cd, d.out.rows32));
    }
    return IODINE_OK;
}

// ---- the tuned refinement conv stack.  The packs of every tuned family are allocated for every handle (ref_family() changes with
// conv_precision; biases and w17 / g17 serve the generic family too), the optional ones by ref_pack_*(); read by ref_conv_fwd / ref_conv_wgrad /
// ref_conv_dgrad behind the family and the same predicates
void alloc_refine_tuned(iodine_handle* h, DevAlloc& da)
{
    RefPacks& r = h->ref;
    const int Cr = h->Cr, Dr = h->Dr;
    da.in("refinement packs");
    for (auto* v : {&r.bias, &r.gather_f, &r.gather_b}) v->assign(Dr, nullptr);
    for (auto* v : {&r.s2_f, &r.s2_b, &r.ws}) v->assign(Dr, Pack());
    for (int l = 0; l < Dr; ++l) {
        r.gather_f[l] = da.f32(wpk_tile_f32_bytes(l == 0 ? 20 : Cr, Cr)); r.bias[l] = da.floats((size_t)Cr);
        r.s2_f[l] = da.pack(wpk_s2_tile_bytes(l == 0 ? 32 : Cr, Cr));   // (its meta: the forward pair, then the data gradient's)
        if (l == 0) continue;
        r.gather_b[l] = da.f32(wpk_tile_f32_bytes(Cr, Cr)); r.s2_b[l] = da.pack(wpk_s2_tile_bytes(Cr, Cr), r.s2_f[l].meta, true);
        if (ref_pack_ws(h)) r.ws[l] = da.pack(wpk_ws_bytes(Cr));
    }
    // split first layer: one 16-channel chunk each for the per-slot (12 real) and the per-image (8 real) channels
    r.wk = da.floats((size_t)Cr * 12 * 9); r.wsh = da.floats((size_t)Cr * 8 * 9); r.g20 = da.floats((size_t)Cr * 20 * 9);
    if (ref_pack_bwd01(h)) r.bwd01 = da.pack(wpk_ws_bytes(Cr));
    r.w17 = da.floats((size_t)Cr * 17 * h->kr * h->kr); r.g17 = da.floats((size_t)Cr * 17 * h->kr * h->kr);
    r.split_k = da.pack(wpk_s2_tile_bytes(16, Cr)); r.split_sh = da.pack(wpk_s2_tile_bytes(16, Cr));
    if (Cr % 16 == 0) { r.l0k = da.pack(wpk_l0_bytes(Cr)); r.l0s = da.pack(wpk_l0_bytes(Cr)); }      // (ref_pack_l0f is "these exist")
}

// the tuned refinement conv stack: every pack of the family, whatever the per-form options say (they do not invalidate the parameters)
int pack_refine_tuned(iodine_handle* h, ParamPacker& pk, const float* const* dev, RefFamily fam)
{
    hipStream_t st = pk.st;
    const ParamSlots& ps = h->slot;
    RefPacks& r = h->ref;
    const int Cr = h->Cr;
    // first layer: the reference weight has n_in input channels (ARCH.ENCODING subset); the kernels see 17
    const float* w0 = dev[ps.ref_w[0]];
    if (h->n_in < 17) { HIPCHK(h, launch_enc_expand_weights(st, w0, Cr, h->n_in, h->enc_map, r.w17)); w0 = r.w17; }
    for (int l = 0; l < h->Dr; ++l) {
        if (fam == REF_GATHER) HIPCHK(h, launch_pack_conv_weights(st, l == 0 ? w0 : dev[ps.ref_w[l]], Cr, l == 0 ? 17 : Cr, l == 0 ? 20 : Cr, Cr, 0, r.gather_f[l]));
        HIPCHK(h, pk.copy(r.bias[l], dev[ps.ref_b[l]], Cr));
    }
    switch (fam) {
    case REF_GATHER: for (int l = 1; l < h->Dr; ++l) HIPCHK(h, launch_pack_conv_weights(st, dev[ps.ref_w[l]], Cr, Cr, Cr, Cr, 2, r.gather_b[l])); break;
    case REF_S2_F16: case REF_S2_F32: {
        // split fp16: jobs of the batched pack; exact fp32: fp32 weights in the same LDS-tile / register layouts, in the same buffers
        const bool f16 = fam == REF_S2_F16;
        auto tile = [&](const float* w, int I, int cin, int tflip, const Pack& p) {
            return f16 ? pk.f16(w, Cr, I, cin, Cr, tflip, p) : launch_pack_conv_weights_s2f32(st, w, Cr, I, cin, Cr, tflip, p.data);
        };
        for (int l = 0; l < h->Dr; ++l) {
            const float* w = l == 0 ? w0 : dev[ps.ref_w[l]];
            HIPCHK(h, tile(w, l == 0 ? 17 : Cr, l == 0 ? 32 : Cr, 0, r.s2_f[l]));
            if (l > 0) HIPCHK(h, tile(w, Cr, Cr, 2, r.s2_b[l]));
        }
        // split first layer (refine_split): the same weights in the internal channel order, packed as two 16-channel convs
        HIPCHK(h, launch_ref_split_weights(st, w0, Cr, r.wk, r.wsh));
        HIPCHK(h, tile(r.wk, 12, 16, 0, r.split_k));
        HIPCHK(h, tile(r.wsh, 8, 16, 0, r.split_sh));
        if (f16 && ref_pack_l0f(h)) {                          // fused encoding + layer 0: both parts as K = 16 MFMA operands
            HIPCHK(h, pk.job(2, r.wk, r.l0k, Cr, 12));
            HIPCHK(h, pk.job(2, r.wsh, r.l0s, Cr, 8));
        }
        for (int l = 1; l < h->Dr && ref_pack_ws(h); ++l)       // weight-stationary forward of layers 1 ..
            HIPCHK(h, f16 ? pk.ws(dev[ps.ref_w[l]], Cr, 0, r.ws[l]) : launch_pack_conv_weights_ws32(st, dev[ps.ref_w[l]], Cr, 0, r.ws[l].data));
        if (f16 && ref_pack_bwd01(h))                          // fused layer-1 / layer-0 backward: W1 as the transposed conv's A operand
            HIPCHK(h, pk.ws(dev[ps.ref_w[1]], Cr, 1, r.bwd01));
        break;
    }
    case REF_GENERIC: break;                                   // (pack_refine_generic)
    }
    return IODINE_OK;
}

// ---- the refinement head: allocated for every handle, read by refine_step and the head's backward (iodine_train.cpp)
void alloc_head(iodine_handle* h, DevAlloc& da)
{
    HeadPacks& d = h->head;
    const size_t L = h->L, Cr = h->Cr, H = h->H;
    da.in("refinement head");
    d.mlp_wT = da.floats(Cr * H); d.mlp_b = da.floats(H);
    d.wihT = da.floats((H + 4 * L + H) * 4 * H);             // [W_ih^T ; W_hh^T] contiguous: one K-major operand for the gate GEMM (head_mfma)
    d.whhT = d.wihT ? d.wihT + (H + 4 * L) * 4 * H : nullptr;
    d.lstm_b = da.floats(4 * H);
    d.wmT = da.floats(H * L); d.bm = da.floats(L); d.wvT = da.floats(H * L); d.bv = da.floats(L);
    d.init_mean = da.floats(L); d.init_logvar = da.floats(L);
    d.raw_mlp_w = da.floats(H * Cr); d.raw_wih = da.floats(4 * H * (H + 4 * L)); d.raw_whh = da.floats(4 * H * H);
    d.raw_wm = da.floats(L * H); d.raw_wv = da.floats(L * H);
}

// raw copies of the head's weights for its backward GEMMs, then the head as the forward reads it - the same on every path
int pack_head(iodine_handle* h, ParamPacker& pk, const float* const* dev)
{
    const ParamSlots& ps = h->slot;
    const int L = h->L, Cr = h->Cr, H = h->H;
    auto copy_raw = [&](float* dst, int slot) { return pk.copy(dst, dev[slot], h->params[slot].numel()); };
    HIPCHK(h, copy_raw(h->head.raw_mlp_w, ps.mlp_w));
    HIPCHK(h, copy_raw(h->head.raw_wih, ps.wih));
    HIPCHK(h, copy_raw(h->head.raw_whh, ps.whh));
    HIPCHK(h, copy_raw(h->head.raw_wm, ps.wm));
    HIPCHK(h, copy_raw(h->head.raw_wv, ps.wv));
    // head
    HIPCHK(h, pk.transpose(h->head.mlp_wT, dev[ps.mlp_w], H, Cr));
    HIPCHK(h, pk.copy(h->head.mlp_b, dev[ps.mlp_b], H));
    HIPCHK(h, pk.transpose(h->head.wihT, dev[ps.wih], 4 * H, H + 4 * L));
    HIPCHK(h, pk.transpose(h->head.whhT, dev[ps.whh], 4 * H, H));
    HIPCHK(h, pk.add2(h->head.lstm_b, dev[ps.bih], dev[ps.bhh], 4 * H));
    HIPCHK(h, pk.transpose(h->head.wmT, dev[ps.wm], L, H));
    HIPCHK(h, pk.transpose(h->head.wvT, dev[ps.wv], L, H));
    HIPCHK(h, pk.copy(h->head.bm, dev[ps.bm], L));
    HIPCHK(h, pk.copy(h->head.bv, dev[ps.bv], L));
    HIPCHK(h, pk.copy(h->head.init_mean, dev[ps.init_mean], L));
    HIPCHK(h, pk.copy(h->head.init_logvar, dev[ps.init_logvar], L));
    return IODINE_OK;
}

}  // namespace

extern "C" {

int iodine_create(const iodine_config* cfg, iodine_handle** out)
{
    if (out) *out = nullptr;
    if (!cfg || !out) return free_fail(IODINE_ERR_INVALID, "null argument");
    const std::string why = validate(*cfg);
    if (!why.empty()) return free_fail(IODINE_ERR_INVALID, why);
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
        iodine_destroy(h);
        return free_hip(what, e);
    };
    DevAlloc da{h, "lin, elbo_counter"};
    h->lin = da.floats((size_t)h->S);
    h->elbo_counter = (unsigned*)da.floats(4);
    alloc_decoder_tuned(h, da);
    alloc_refine_tuned(h, da);
    alloc_head(h, da);
    if (dec_path(h) == DEC_GENERIC) alloc_decoder_generic(h, da);
    if (ref_family(h) == REF_GENERIC) alloc_refine_generic(h, da);
    // gradient accumulators: ONE buffer, parameters back to back in named_parameters() order (the layout the wrapper's
    // flat gradient buffer has too), so that zeroing and the final scale-and-add are one launch each
    h->gacc.assign(h->params.size(), nullptr);
    h->gacc_total = 0;
    for (size_t i = 0; i < h->params.size(); ++i) h->gacc_total += h->params[i].numel();
    da.in("gradient accumulators");
    h->gacc_arena = da.floats(h->gacc_total);
    if (da.err != hipSuccess) return bail(da.err, (std::string("hipMalloc, ") + da.group).c_str());
    {
        size_t off = 0;
        for (size_t i = 0; i < h->params.size(); ++i) { h->gacc[i] = h->gacc_arena + off; off += h->params[i].numel(); }
    }
    if (hipError_t e_ = hipMemset(h->elbo_counter, 0, 16); e_ != hipSuccess) return bail(e_, "hipMemset elbo_counter");
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
    if (h->adapt.dev) (void)hipFree(h->adapt.dev);
    if (h->adapt.counts_host) (void)hipHostFree(h->adapt.counts_host);
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
