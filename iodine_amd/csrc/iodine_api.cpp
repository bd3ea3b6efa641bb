// The compute handle of libiodine_hip.so: parameter repacking, workspace planning, kernel dispatch and the T-step refinement loop
// (kernel launch sequence), settings.  See include/iodine_hip.h for the ABI and the reference call sites each entry point replaces;
// iodine_pad.cpp for handles at a padded width, iodine_ops.cpp for the entry points that take no handle.
#include "iodine_internal.h"

std::string g_create_error;

namespace {

// bump allocator over a (possibly NULL = size query) base pointer
struct Arena {
    char* base;
    size_t off = 0;
    explicit Arena(void* b) : base((char*)b) {}
    template <typename T> T* take(size_t n) {
        off = (off + 255) & ~(size_t)255;
        T* p = base ? (T*)(base + off) : nullptr;
        off += n * sizeof(T);
        return p;
    }
};

}  // namespace

#ifdef IODINE_XSKIP_HOOK
int g_iod_xskip = 0;
#endif

namespace {

// bracket one launch expression with profiler events (no-op unless profiling is on)
#define PROF(h, st, cat, expr)                                                       \
    do {                                                                             \
        hipEvent_t e0_ = nullptr, e1_ = nullptr;                                     \
        ProfCat* pc_ = nullptr;                                                      \
        if ((h)->profile > 1) { pc_ = (h)->prof_cat(cat); pc_->seen_win++; }         \
        else if ((h)->profile == 1 && !strncmp(cat, "conv_tile_", 10)) {             \
            pc_ = (h)->prof_cat(cat);                                                \
            pc_->seen_win++;                                                         \
            if (pc_->seen++ % (unsigned long long)(h)->profile_stride) pc_ = nullptr;    \
        }                                                                            \
        if (pc_) {                                                                   \
            if (pc_->used == pc_->ev.size()) {                                       \
                hipEvent_t a_, b_;                                                   \
                HIPCHK(h, hipEventCreate(&a_)); HIPCHK(h, hipEventCreate(&b_));      \
                pc_->ev.push_back({a_, b_});                                         \
            }                                                                        \
            e0_ = pc_->ev[pc_->used].first; e1_ = pc_->ev[pc_->used].second;         \
            pc_->used++;                                                             \
            HIPCHK(h, hipEventRecord(e0_, st));                                      \
        }                                                                            \
        HIPCHK(h, expr);                                                             \
        if (e1_) HIPCHK(h, hipEventRecord(e1_, st));                                 \
    } while (0)

// Which kernels the decoder runs on.  Decided here and nowhere else: the launch sites below, the packs iodine_set_params refreshes and the
// workspace plan all switch on it, so a weight pack that is read is a pack that was written.  A function, not a cached field: the options
// may change between calls (conv_precision / conv_variant invalidate the parameters, and the graph key holds both).
enum DecPath {
    DEC_GENERIC,      // kernels_generic.hip: KERNEL_SIZE other than 3, CONV_CHAN other than 32 / 64, sizes that are no multiple of 16
    DEC_WS_F16,       // split-fp16, weight-stationary persistent kernel (conv_variant 6, power-of-two image sizes >= 16)
    DEC_TILE_F16,     // split-fp16, LDS-tiled 16 x 16 tiles
    DEC_WS_F32,       // exact fp32 (conv_precision 0): the weight-stationary kernel's fp32 form (v_mfma_f32_16x16x4_f32, no tile scales / side buffers)
    DEC_TILE_F32,     // exact fp32, the round-1 LDS-tiled kernels
};

DecPath dec_path(const iodine_handle* h)
{
    if (h->generic) return DEC_GENERIC;
    const bool ws = h->variant == 6 && h->S >= 16 && (h->S & (h->S - 1)) == 0;
    if (h->precision != 0) return ws ? DEC_WS_F16 : DEC_TILE_F16;
    return ws && (h->Cd == 64 || h->Cd == 32) ? DEC_WS_F32 : DEC_TILE_F32;
}

bool dec_f16(DecPath p) { return p == DEC_WS_F16 || p == DEC_TILE_F16; }
// fp16 MFMAs per product on DEC_WS_F16: the split's three, or hi.hi alone (conv_precision 2, the only kernel that option changes)
int dec_ws_products(const iodine_handle* h) { return h->precision == 2 ? 1 : 3; }

// Which kernels the refinement conv stack runs on, decided the same way.  The family depends on the configuration and conv_precision only:
// iodine_set_params switches on it alone and keeps every pack of the family current - the per-form options do not invalidate the parameters.
enum RefFamily {
    REF_GENERIC,      // kernels_generic.hip: KERNEL_SIZE other than 3, CONV_CHAN other than 32 / 64, sizes that are no multiple of 16, stride != 2
    REF_S2_F16,       // the tuned stride-2 kernels, split fp16
    REF_S2_F32,       // the same kernels in their fp32-MFMA form (conv_precision 0): same buffers, fp32 weights in the same layouts
    REF_GATHER,       // the gather kernels: some layer has an odd input size, which the tuned kernels do not take
};
RefFamily ref_family(const iodine_handle* h)
{
    if (h->gen_ref) return REF_GENERIC;
    for (int l = 0, s = h->S; l < h->Dr; ++l, s /= 2) if (s % 2 != 0) return REF_GATHER;
    return h->precision != 0 ? REF_S2_F16 : REF_S2_F32;
}
bool ref_s2(RefFamily f) { return f == REF_S2_F16 || f == REF_S2_F32; }
// Which optional packs exist at these shapes: iodine_set_params writes a pack where its predicate holds, a launch site reads it only behind it.
bool ref_pack_ws(const iodine_handle* h) { return h->Cr == 64; }                                               // ref_wsf[1 ..]
bool ref_pack_bwd01(const iodine_handle* h) { return h->Dr >= 2 && refine_bwd01_ok(h->S, h->Cr); }             // ref_w1ws
bool ref_pack_l0f(const iodine_handle* h) { return h->ref_l0k != nullptr; }                                    // ref_l0k / ref_l0s
// The form of a forward pass: the family with the options and the kernels' own shape limits.  A pure function of the handle: it is evaluated
// inside graphed bodies, which a replay does not execute - what a later call needs of it (CallState) is stored outside of them.
// split: the channels every slot of an image shares are written and convolved once per image (split first layer); l0f: ... and encoding +
// layer 0 are one kernel, the encoding stays on chip unless a reader asks for it
struct RefForm { RefFamily fam; bool split, l0f; };
RefForm ref_form(const iodine_handle* h)
{
    const RefFamily fam = ref_family(h);
    const bool split = h->refine_split && ref_s2(fam);
    return {fam, split, split && fam == REF_S2_F16 && h->refine_l0_fused && ref_pack_l0f(h) && refine_l0_fused_ok(h->S, h->Cr, h->K)};
}
// layer l (input size s) on the weight-stationary kernel?
bool ref_layer_ws(const iodine_handle* h, const RefForm& f, int l, int s) { return l > 0 && h->refine_ws && ref_s2(f.fam) && ref_pack_ws(h) && conv3x3_s2ws_ok(s, h->Cr); }
// layer 1's data gradient + layer 0's weight gradient in one launch?  fwd_split: what the saved forward left (CallState), not the current option
bool ref_bwd01(const iodine_handle* h, bool fwd_split) { return h->refine_bwd_fused && fwd_split && ref_family(h) == REF_S2_F16 && ref_pack_bwd01(h); }

// The per-layer launches of the tuned decoder (layers 1 .. Dd-1 are 3x3 convs Cd -> Cd, then the output conv Cd -> 4), one switch each.
// zig-zag (`l & 1`): odd decoder layers walk the slot-images backwards (forward pass: l0 writes forwards, layer 1 reads
// backwards, layer 2 forwards, ...; backward pass the same by layer), so a launch starts on the part of its input
// that the previous launch wrote last - still in the 256 MiB Infinity Cache - instead of the part written first.
// Tiles are independent: results do not depend on the order.  Measured -0.3 % on the cfg3 step (same-box A/B).
// The per-cell maxima (tmax_*) exist on the weight-stationary split-fp16 path only.
int dec_conv_fwd(iodine_handle* h, hipStream_t st, int N, int l)
{
    Buffers& b = h->buf;
    const int S = h->S, Cd = h->Cd;
    switch (dec_path(h)) {
    case DEC_WS_F16:
        PROF(h, st, "conv_tile_fwd", launch_conv3x3_ws_f16x3(st, b.act[l - 1], h->dec_wsf[l], h->dec_wmeta[l], h->dec_b[l], nullptr, b.act[l],
                                                             b.tmax_act[l - 1], b.tmax_act[l], N, S, Cd, EPI_BIAS_ELU, l & 1, dec_ws_products(h)));
        break;
    case DEC_TILE_F16:
        PROF(h, st, "conv_tile_fwd", launch_conv3x3_tile_f16x3(st, b.act[l - 1], h->dec_wf16[l], h->dec_wmeta[l], h->dec_b[l], nullptr, b.act[l],
                                                               N, S, Cd, Cd, EPI_BIAS_ELU, l & 1));
        break;
    case DEC_WS_F32:
        PROF(h, st, "conv_tile_fwd", launch_conv3x3_ws_f32(st, b.act[l - 1], h->dec_wsf[l], h->dec_b[l], nullptr, b.act[l], N, S, Cd, EPI_BIAS_ELU, l & 1));
        break;
    case DEC_TILE_F32:
        PROF(h, st, "conv_tile_fwd", launch_conv3x3_tile(st, b.act[l - 1], h->dec_wf[l], h->dec_b[l], nullptr, b.act[l], N, S, Cd, Cd, EPI_BIAS_ELU));
        break;
    case DEC_GENERIC: break;                               // (decoder_forward branches off before)
    }
    return IODINE_OK;
}

// data gradient of layer l: b.dpre[cur] -> out with epilogue epi (EPI_MUL_ELUGRAD into b.dpre[cur ^ 1], or the broadcast layer's row sums)
int dec_conv_dgrad(iodine_handle* h, hipStream_t st, int N, int l, int cur, float* out, int epi)
{
    Buffers& b = h->buf;
    const int S = h->S, Cd = h->Cd;
    switch (dec_path(h)) {
    case DEC_WS_F16:
        PROF(h, st, "conv_tile_dgrad", launch_conv3x3_ws_f16x3(st, b.dpre[cur], h->dec_wsb[l], h->dec_wmeta[l] + 2, nullptr, b.act[l - 1], out,
                                                               b.tmax_dpre[cur], b.tmax_dpre[cur ^ 1], N, S, Cd, epi, l & 1, dec_ws_products(h)));
        break;
    case DEC_TILE_F16:
        PROF(h, st, "conv_tile_dgrad", launch_conv3x3_tile_f16x3(st, b.dpre[cur], h->dec_wb16[l], h->dec_wmeta[l] + 2, nullptr, b.act[l - 1], out,
                                                                 N, S, Cd, Cd, epi, l & 1));
        break;
    case DEC_WS_F32:
        PROF(h, st, "conv_tile_dgrad", launch_conv3x3_ws_f32(st, b.dpre[cur], h->dec_wsb[l], nullptr, b.act[l - 1], out, N, S, Cd, epi, l & 1));
        break;
    case DEC_TILE_F32:                                     // (never asked for the row-sum epilogues: fused_l0 in decoder_backward_data)
        PROF(h, st, "conv_tile_dgrad", launch_conv3x3_tile(st, b.dpre[cur], h->dec_wb[l], nullptr, b.act[l - 1], out, N, S, Cd, Cd, epi));
        break;
    case DEC_GENERIC: break;
    }
    return IODINE_OK;
}

// weight / bias gradient of layer l as partial tiles: part / part_b = (accum ? part : 0) + alpha x this launch
int dec_conv_wgrad(iodine_handle* h, hipStream_t st, int N, int l, int cur, float* part, float* part_b, float alpha, int accum,
                   int* nparts, int* ncop, int* nb)
{
    Buffers& b = h->buf;
    const int S = h->S, Cd = h->Cd;
    switch (dec_path(h)) {
    case DEC_WS_F16:
    case DEC_TILE_F16:
        PROF(h, st, "conv_tile_wgrad", launch_conv3x3_wgrad_f16x3_ws(st, b.act[l - 1], b.dpre[cur], part, part_b, N, S, Cd, Cd, nparts, ncop, nb,
                                                                      alpha, accum));
        break;
    case DEC_WS_F32:
        PROF(h, st, "conv_tile_wgrad", launch_conv3x3_wgrad_f32_ws(st, b.act[l - 1], b.dpre[cur], part, part_b, N, S, Cd, nparts, ncop, nb, alpha, accum));
        break;
    case DEC_TILE_F32:                                     // takes no pass factor: alpha = 1, accum = 0 only (decoder_backward_data)
        PROF(h, st, "conv_tile_wgrad", launch_conv3x3_wgrad_tile(st, b.act[l - 1], b.dpre[cur], part, part_b, N, S, Cd, Cd, nparts, ncop, nb));
        break;
    case DEC_GENERIC: break;
    }
    return IODINE_OK;
}

// the output conv's data gradient b.g -> b.dpre[cur] on its own (inference, option out_bwd_fused 0, the exact-fp32 paths)
int dec_out_dgrad(iodine_handle* h, hipStream_t st, int N, int cur)
{
    Buffers& b = h->buf;
    const DecPath path = dec_path(h);
    if (dec_f16(path))
        PROF(h, st, "dec_out_dgrad", launch_dec_out_dgrad_f16x3(st, b.g, h->dec_out_wb16, h->dec_out_meta, b.act[h->Dd - 1], b.dpre[cur], N, h->S,
                                                                 h->Cd, path == DEC_WS_F16 ? b.tmax_dpre[cur] : nullptr));
    else
        PROF(h, st, "dec_out_dgrad", launch_conv3x3_tile(st, b.g, h->dec_out_wb, nullptr, b.act[h->Dd - 1], b.dpre[cur], N, h->S, 4, h->Cd,
                                                         EPI_MUL_ELUGRAD));
    return IODINE_OK;
}

// ... and its weight / bias gradient as partial tiles (none of these kernels takes a pass factor); *ncop: padded output channels of a tile
int dec_out_wgrad(iodine_handle* h, hipStream_t st, int N, float* part, float* part_b, int* nparts, int* ncop, int* nb)
{
    Buffers& b = h->buf;
    const float* a = b.act[h->Dd - 1];
    *ncop = 4;
    switch (dec_path(h)) {
    case DEC_WS_F16:
    case DEC_TILE_F16:                                     // GEMM form: rows (tap, co), no N = 4 -> 32 padding
        PROF(h, st, "dec_out_wgrad", launch_dec_out_wgrad_gemm_f16x3(st, a, b.g, part, part_b, N, h->S, h->Cd, nparts, nb));
        break;
    case DEC_WS_F32:                                       // exact fp32, GEMM form (kernels_wgrad32.hip)
        PROF(h, st, "dec_out_wgrad", launch_dec_out_wgrad_f32(st, a, b.g, part, part_b, N, h->S, h->Cd, nparts, nb));
        break;
    case DEC_TILE_F32:
        PROF(h, st, "dec_out_wgrad", launch_conv3x3_wgrad_tile(st, a, b.g, part, part_b, N, h->S, h->Cd, 4, nparts, ncop, nb));
        break;
    case DEC_GENERIC: break;
    }
    return IODINE_OK;
}

template <typename T>
hipError_t dev_alloc(iodine_handle* h, T** p, size_t n)
{
    void* q = nullptr;
    hipError_t e = hipMalloc(&q, std::max<size_t>(n, 1) * sizeof(T));
    if (e == hipSuccess) { *p = (T*)q; h->owned.push_back(q); }
    return e;
}

void build_param_table(iodine_handle* h)
{
    // names / shapes of the reference module tree in named_parameters() order
    // (iodine.py:26-33, 412-423, 446-464, 543-557, 570-584, 596-604)
    // (returns the parameter's index: h->slot keeps it, so nothing downstream looks a parameter up by name)
    auto add = [&](const std::string& n, std::initializer_list<long long> d) {
        ParamInfo p; p.name = n; p.ndim = (int)d.size(); int i = 0;
        for (long long v : d) p.dims[i++] = v;
        for (; i < 4; ++i) p.dims[i] = 1;
        h->params.push_back(p);
        return (int)h->params.size() - 1;
    };
    const iodine_config& c = h->cfg;
    ParamSlots& s = h->slot;
    int cin = h->n_in;
    for (int i = 0; i < c.ref_conv_layers; ++i) {
        s.ref_w.push_back(add("refine.mlc.layers." + std::to_string(i) + ".weight", {c.ref_conv_chan, cin, c.ref_kernel_size, c.ref_kernel_size}));
        s.ref_b.push_back(add("refine.mlc.layers." + std::to_string(i) + ".bias", {c.ref_conv_chan}));
        cin = c.ref_conv_chan;
    }
    const long long H = c.ref_mlp_units, L = c.dim_latent;
    s.mlp_w = add("refine.mlp.layers.0.weight", {H, c.ref_conv_chan});
    s.mlp_b = add("refine.mlp.layers.0.bias", {H});
    s.wih = add("refine.lstm.weight_ih", {4 * H, H + 4 * L});
    s.whh = add("refine.lstm.weight_hh", {4 * H, H});
    s.bih = add("refine.lstm.bias_ih", {4 * H});
    s.bhh = add("refine.lstm.bias_hh", {4 * H});
    s.wm = add("refine.mean_update.weight", {L, H});
    s.bm = add("refine.mean_update.bias", {L});
    s.wv = add("refine.logvar_update.weight", {L, H});
    s.bv = add("refine.logvar_update.bias", {L});
    cin = c.dim_latent + 2;
    for (int i = 0; i < c.dec_conv_layers; ++i) {
        s.dec_w.push_back(add("decoder.mlc.layers." + std::to_string(i) + ".weight", {c.dec_conv_chan, cin, c.dec_kernel_size, c.dec_kernel_size}));
        s.dec_b.push_back(add("decoder.mlc.layers." + std::to_string(i) + ".bias", {c.dec_conv_chan}));
        cin = c.dec_conv_chan;
    }
    s.out_w = add("decoder.conv.weight", {4, c.dec_conv_chan, c.dec_kernel_size, c.dec_kernel_size});
    s.out_b = add("decoder.conv.bias", {4});
    s.init_mean = add("posterior.init_mean", {L});
    s.init_logvar = add("posterior.init_logvar", {L});
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

// spatial size of refinement layer l's OUTPUT
// (k x k, pad k // 2, stride rs: floor((s + 2 (k // 2) - k) / rs) + 1 = (s - 1) / rs + 1 for odd k)
int ref_out_size(const iodine_handle* h, int s) { return (s - 1) / h->rs + 1; }

void plan(const iodine_handle* h, int B, int mode, Arena& a, Buffers& b)
{
    const int N = B * h->K, P = h->P, L = h->L, Cd = h->Cd, Cr = h->Cr, H = h->H, T = h->T;
    const bool gen_dec = dec_path(h) == DEC_GENERIC, gen_ref = ref_family(h) == REF_GENERIC;
    b.B = B; b.mode = mode; b.K = h->K; b.T = h->T;
    b.F = h->frames > 0 ? h->frames : 1;
    b.x4 = a.take<float>((size_t)b.F * B * P * 4);           // [F][B][P][4]: evaluation i reads frame i (x4_frame)
    b.V = a.take<float>((size_t)N * 9 * Cd);
    b.dec_out = a.take<float>((size_t)N * P * 4);
    b.g = a.take<float>((size_t)N * P * 4);
    b.part = a.take<double>((size_t)B * pixel_blocks_per_image(P) * (6 * h->K + 3));
    b.lnstat = a.take<float>((size_t)N * 8);
    b.ll_img = a.take<float>((size_t)B);
    b.img_terms = a.take<float>((size_t)(T + 1) * B * 2);
    b.scal = a.take<float>((size_t)(T + 1) * 3 + 4);
    b.rows = a.take<float>((size_t)N * h->S * 3 * Cd);
    b.rows_p = a.take<float>((size_t)N * h->S * (h->S / 16 > 0 ? h->S / 16 : 1) * (mode != 0 ? 4 : 3) * Cd);   // per-tile row sums (EPI_L0ROWS / EPI_L0ROWSX)
    b.l0scr = a.take<float>(l0_rows_scratch_floats(N, Cd));
    b.Rc = a.take<float>((size_t)N * 9 * Cd);
    b.pm = a.take<float>((size_t)N * L);
    b.plv = a.take<float>((size_t)N * L);
    b.act.resize(h->Dd);
    for (int l = 0; l < h->Dd; ++l) b.act[l] = a.take<float>((size_t)N * P * Cd);
    b.dpre[0] = a.take<float>((size_t)N * P * Cd);
    b.dpre[1] = a.take<float>((size_t)N * P * Cd);
    b.tmax_act.resize(h->Dd);
    for (int l = 0; l < h->Dd; ++l) b.tmax_act[l] = a.take<float>(conv_ws_tmax_floats(N, h->S));
    b.tmax_dpre[0] = a.take<float>(conv_ws_tmax_floats(N, h->S));
    b.tmax_dpre[1] = a.take<float>(conv_ws_tmax_floats(N, h->S));
    const int ncopy = mode == 1 ? T + 1 : 1;
    auto per_iter = [&](std::vector<float*>& v, size_t n, int copies) {      // `copies` instances back to back, the rest alias [0]
        v.resize(T + 1);
        float* base = a.take<float>(n * (size_t)copies);
        for (int i = 0; i <= T; ++i) v[i] = (i < copies && base) ? base + (size_t)i * n : base;
    };
    per_iter(b.z, (size_t)N * L, ncopy);
    if (mode != 1) b.z[T] = a.take<float>((size_t)N * L);   // the final sample must not overwrite the last elbo()'s z (self.z)
    per_iter(b.g_pm, (size_t)N * L, ncopy);
    per_iter(b.g_plv, (size_t)N * L, ncopy);
    per_iter(b.latent, (size_t)N * 4 * L, ncopy);
    {
        // training keeps the refinement inputs of all T iterations, back to back: the conv stack of the refinement network is
        // back-propagated for all iterations in ONE batch of T * N slot-images (iodine_train_backward)
        const size_t n_enc = (size_t)N * P * 20;
        float* base = a.take<float>(n_enc * (mode == 1 ? T : 1));
        b.enc.resize(T + 1);
        for (int i = 0; i <= T; ++i) b.enc[i] = (mode == 1 && i < T) ? (base ? base + (size_t)i * n_enc : nullptr) : base;
        // split form (refine_split): the same memory as per-slot tensors [N][P][12] of all kept iterations back to back,
        // followed by the per-image tensors [B][P][8]
        const size_t n_k = (size_t)N * P * 12, n_s = (size_t)B * P * 8;
        const int keep = mode == 1 ? T : 1;
        b.enck.resize(T + 1); b.encs.resize(T + 1);
        for (int i = 0; i <= T; ++i) {
            const int j = (mode == 1 && i < T) ? i : 0;
            b.enck[i] = base ? base + (size_t)j * n_k : nullptr;
            b.encs[i] = base ? base + (size_t)keep * n_k + (size_t)j * n_s : nullptr;
        }
        b.rmap = a.take<float>((size_t)B * (h->S / 2) * (h->S / 2) * Cr);
    }
    per_iter(b.pooled, (size_t)N * Cr, ncopy);
    per_iter(b.u, (size_t)N * H, ncopy);
    per_iter(b.gates, (size_t)N * 4 * H, ncopy);
    per_iter(b.xin, (size_t)N * (H + 4 * L), ncopy);
    {   // gate GEMM of the refinement head (head_mfma): its input rows [u | latent | h_prev] and its output, rows padded to a multiple of 32
        const size_t Np = ((size_t)N + 31) / 32 * 32;
        b.head_xh = a.take<float>(Np * (size_t)(H + 4 * L + H));
        b.head_gp = a.take<float>(Np * (size_t)4 * H);
    }
    // LSTM state: h[i], c[i] = state BEFORE iteration i; inference ping-pongs two copies
    b.h.resize(T + 2); b.c.resize(T + 2);
    if (mode == 1) {
        // (each array contiguous over the iterations: the head's weight gradients are one GEMM over all T * N rows)
        float* hb = a.take<float>((size_t)(T + 2) * N * H);
        float* cb = a.take<float>((size_t)(T + 2) * N * H);
        for (int i = 0; i <= T + 1; ++i) { b.h[i] = hb ? hb + (size_t)i * N * H : nullptr; b.c[i] = cb ? cb + (size_t)i * N * H : nullptr; }
    } else {
        float* hh[2] = {a.take<float>((size_t)N * H), a.take<float>((size_t)N * H)};
        float* cc[2] = {a.take<float>((size_t)N * H), a.take<float>((size_t)N * H)};
        for (int i = 0; i <= T + 1; ++i) { b.h[i] = hh[i & 1]; b.c[i] = cc[i & 1]; }
    }
    b.ract.assign(T + 1, std::vector<float*>(h->Dr));
    {
        int s = h->S;
        for (int l = 0; l < h->Dr; ++l) {
            s = ref_out_size(h, s);
            const size_t n_l = (size_t)N * s * s * Cr;
            float* base = a.take<float>(n_l * (mode == 1 ? T : 1));         // [T][N][s][s][Cr] in training (see enc)
            for (int i = 0; i <= T; ++i) b.ract[i][l] = (mode == 1 && i < T) ? (base ? base + (size_t)i * n_l : nullptr) : base;
        }
    }
    if (mode != 0) {
        // what one weight-gradient pass of the decoder needs: training, and mode 2 = "decoder backward" (a single decode / elbo kept for
        // iodine_decode_backward / iodine_elbo_backward): the inference carve-up plus this block
        const int Cmax = Cd > Cr ? Cd : Cr;
        const size_t part_elems = (size_t)512 * 4 * 9 * 32 * 32 > (size_t)512 * 9 * Cmax * Cmax
                                      ? (size_t)512 * 4 * 9 * 32 * 32 : (size_t)512 * 9 * Cmax * Cmax;
        b.wg_part = a.take<float>(part_elems);
        b.wg_part_b = a.take<float>((size_t)512 * 64);
        b.wg_acc.assign(h->Dd, nullptr); b.wg_acc_b.assign(h->Dd, nullptr);
        if (h->wgrad_accum && !gen_dec && mode == 1) {      // (a single pass has nothing to accumulate over: shared scratch)
            b.wg_acc[0] = a.take<float>((size_t)1024 * 2 * 9 * Cd * 4);       // dec_out_bwd_fused: <= 1024 blocks x KS <= 2 tiles of [9][Cd][4]
            b.wg_acc_b[0] = a.take<float>((size_t)1024 * 4);
            for (int l = 1; l < h->Dd; ++l) {
                b.wg_acc[l] = a.take<float>((size_t)512 * 4 * 9 * 32 * 32 > (size_t)512 * 9 * Cd * Cd ? (size_t)512 * 4 * 9 * 32 * 32 : (size_t)512 * 9 * Cd * Cd);
                b.wg_acc_b[l] = a.take<float>((size_t)512 * 64);
            }
        }
        b.wg_fold = a.take<float>((size_t)WGRAD_FOLD * 9 * Cmax * Cmax);
        b.Dsum = a.take<float>((size_t)P * Cd);
        b.Dpart = a.take<float>((size_t)l0_dgroups(N) * P * Cd);
        b.rown = a.take<float>((size_t)N * h->S * 4 * Cd);
        b.Rsum = a.take<float>((size_t)h->S * 4 * Cd);
        b.RT = a.take<float>((size_t)N * 9 * Cd);
        b.tmp_lz = a.take<float>((size_t)L * 9 * Cd);
    }
    if (mode == 1) {
        // ddm / ddv / dgates / ds: one instance per iteration (weight gradients of the head in one pass over all of them)
        b.ddm = a.take<float>((size_t)T * N * L); b.ddv = a.take<float>((size_t)T * N * L);
        b.dc1 = a.take<float>((size_t)N * H); b.dgates = a.take<float>((size_t)T * N * 4 * H);
        b.dxin = a.take<float>((size_t)N * H); b.ds = a.take<float>((size_t)T * N * H);
        b.dpooled = a.take<float>((size_t)T * N * Cr);                     // all iterations (batched conv-stack backward)
        for (int j = 0; j < 2; ++j) { b.carry_h[j] = a.take<float>((size_t)N * H); b.carry_c[j] = a.take<float>((size_t)N * H); }
        b.rdpre.resize(h->Dr);
        int s = h->S;
        for (int l = 0; l < h->Dr; ++l) { s = ref_out_size(h, s); b.rdpre[l] = a.take<float>((size_t)T * N * s * s * Cr); }
        b.aux_seed = a.take<float>((size_t)2 * (T + 1) * N * L);
    }
    if (gen_dec) {
        b.gen_l0 = a.take<float>(gen_l0_scratch_floats(N, h->S, Cd, h->kd));   // row / tap sums, prefix table of the broadcast layer
    }
    if ((gen_dec || gen_ref) && mode != 0) {
        size_t scr = 0;
        if (gen_dec) scr = std::max(gen_wgrad_scratch_floats(Cd, 4, h->kd), gen_wgrad_scratch_floats(Cd, Cd, h->kd));
        if (gen_ref && mode == 1) scr = std::max(scr, std::max(gen_wgrad_scratch_floats(17, Cr, h->kr), gen_wgrad_scratch_floats(Cr, Cr, h->kr)));
        b.gen_scr = a.take<float>(scr);
    }
    // option sigma_grad (at the end: the carve-up in front of it is the same with or without a reader of these two)
    b.sg_part = a.take<double>((size_t)B * pixel_blocks_per_image(P));
    b.sgrad = a.take<float>((size_t)T + 1);
    // option input_grad: carved only while a bit is set, behind everything else - with the option off the plan is what it was
    b.ig = h->input_grad;
    b.ig_x = (b.ig & 1) ? a.take<float>((size_t)b.F * B * 3 * P) : nullptr;
    b.ig_w = (b.ig & 2) ? a.take<float>((size_t)b.F * B * P) : nullptr;
    b.bytes = (a.off + 255) & ~(size_t)255;
}

void drop_graphs(iodine_handle* h)
{
    for (auto& g : h->graphs) {
        if (g.exec) (void)hipGraphExecDestroy(g.exec);
        if (g.graph) (void)hipGraphDestroy(g.graph);
    }
    h->graphs.clear();
    h->seen_keys.clear();
}

int ensure_workspace(iodine_handle* h, int B, int mode)
{
    if (h->buf.B == B && h->buf.mode == mode && h->buf.K == h->K && h->buf.T == h->T && h->buf.F == (h->frames > 0 ? h->frames : 1) &&
        h->buf.ig == h->input_grad && h->buf.bytes > 0)
        return IODINE_OK;
    Arena q(nullptr); Buffers tmp; plan(h, B, mode, q, tmp);
    void* base = nullptr;
    if (h->ws_user) {
        if (h->ws_user_bytes < tmp.bytes) {
            char m[200];
            snprintf(m, sizeof m, "workspace too small: need %zu bytes for batch %d mode %d at %d slots / %d iterations / %d frame(s), have %zu",
                     tmp.bytes, B, mode, h->K, h->T, tmp.F, h->ws_user_bytes);
            return h->fail(IODINE_ERR_WORKSPACE, m);
        }
        base = h->ws_user;
    } else {
        if (h->ws_own_bytes < tmp.bytes) {
            if (h->ws_own) { HIPCHK(h, hipFree(h->ws_own)); h->ws_own = nullptr; h->ws_own_bytes = 0; }
            HIPCHK(h, hipMalloc(&h->ws_own, tmp.bytes));
            h->ws_own_bytes = tmp.bytes;
        }
        base = h->ws_own;
    }
    Arena a(base);
    plan(h, B, mode, a, h->buf);
    h->calls.arena_gone();                                 // a re-planned arena no longer holds the saved forward / the last elbo() outputs
    // captured graphs stay: their key holds the arena's base address, the batch, the run shape and (through the entry point) the mode,
    // and the carve-up is a pure function of those - a step that alternates training and reconstruct calls keeps replaying both
    return IODINE_OK;
}

// one decoder forward pass from z (already in buf.V via dec_v) -> dec_out
int decoder_forward(iodine_handle* h, hipStream_t st, int N, const float* z, float* out = nullptr)
{
    Buffers& b = h->buf;
    if (!out) out = b.dec_out;
    const DecPath path = dec_path(h);
    if (path == DEC_GENERIC) {
        // fallback: the broadcast layer from the prefix table of its per-tap latent products (kernels_genl0.hip: the broadcast tensor is
        // never built), every other layer a generic fp32 conv (kernels_generic.hip)
        PROF(h, st, "gen_l0", launch_gen_l0_fwd(st, z, h->gen_wdec[0], h->gen_cterm, b.gen_l0, b.act[0], N, h->L, h->S, h->Cd, h->kd));
        const float* in = b.act[0];
        for (int l = 1; l < h->Dd; ++l) {
            if (h->gen_split)
                PROF(h, st, "gen_conv_f16x3", launch_gen_split_conv(st, in, h->gs_wf[l], h->gs_mf[l], h->dec_b[l], nullptr, b.act[l], N, h->S, h->Cd, h->kd, 1));
            else
                PROF(h, st, "gen_conv", launch_gen_conv_fwd(st, in, h->gen_wdec[l], h->dec_b[l], b.act[l], N, h->S, h->Cd, h->Cd, h->Cd, h->kd, 1, 1));
            in = b.act[l];
        }
        PROF(h, st, "gen_conv", launch_gen_conv_fwd(st, in, h->gen_wout, h->dec_out_b, out, N, h->S, h->Cd, h->Cd, 4, h->kd, 1, 0));
        return IODINE_OK;
    }
    const float* last = b.act[h->Dd - 1];
    const float* tmax = path == DEC_WS_F16 ? b.tmax_act[h->Dd - 1] : nullptr;
    PROF(h, st, "dec_l0", launch_dec_l0(st, b.V, h->cmap, b.act[0], N, h->S, h->Cd, path == DEC_WS_F16 ? b.tmax_act[0] : nullptr));
    for (int l = 1; l < h->Dd; ++l)
        if (int rc = dec_conv_fwd(h, st, N, l)) return rc;
    if (path == DEC_WS_F16 && h->dec_out_rows && dec_out_rows_ok(h->S, h->Cd, tmax))
        PROF(h, st, "dec_out", launch_dec_out_rows_f16x3(st, last, h->dec_out_w16, h->dec_out_meta, h->dec_out_b, out, N, h->S, h->Cd, tmax));
    else if (dec_f16(path))
        PROF(h, st, "dec_out", launch_dec_out_stream_f16x3(st, last, h->dec_out_w16, h->dec_out_meta, h->dec_out_b, out, N, h->S, h->Cd, tmax));
    else if (h->dec_out_rows && dec_out_rows_ok(h->S, h->Cd, last) && h->dec_out_w32)      // exact fp32 MFMA, row-streaming
        PROF(h, st, "dec_out", launch_dec_out_rows_f16x3(st, last, h->dec_out_w32, nullptr, h->dec_out_b, out, N, h->S, h->Cd, nullptr, 1));
    else
        PROF(h, st, "dec_out", launch_dec_out(st, last, h->dec_out_w, h->dec_out_b, out, N, h->S, h->Cd));
    return IODINE_OK;
}

// gradient of B*ELBO wrt the decoder input z through the whole decoder (replaces the autograd traversal of
// (B*elbo).backward(), iodine.py:90,137).  Leaves d(pre-activation) of layer 0 in the returned buffer.
// With train the decoder weight gradients of this pass are accumulated on the way with the factor train_alpha
// (= -w_i / B): they are what the outer loss.backward() (train.py:63) would compute for this decoder pass.  The flag is separate from
// the factor: a pass with loss weight 0 (iter_weights 'last', an explicit 0) is still a training pass - it takes part in the first-pass
// overwrite of the maps accumulated over the passes (Dsum, Rsum, the kept partial tiles of wgrad_accum) and in the last pass's reduction /
// coordinate and bias gradients; only launches that purely ADD alpha x (this pass) to an accumulator are skipped for it.
// the same on the generic fallback path: plain chain of data gradients (and, in training, weight gradients with the pass factor);
// the broadcast layer's weight gradient and the gradient wrt z come from the tap-window sums of its pre-activation gradient
// (kernels_genl0.hip); dz is left in the first L entries of every row of buf.Rc (dz_latent multiplies that by the identity in h->gen_ident)
int decoder_backward_generic(iodine_handle* h, hipStream_t st, int N, float train_alpha, int it)   // it: only b.z[it], the decoded z
{
    // (every weight gradient here is an accumulation gacc += alpha x ..., without first / last bookkeeping: a zero-weight pass skips them)
    Buffers& b = h->buf;
    const ParamSlots& ps = h->slot;
    const int Cd = h->Cd, Dd = h->Dd, L = h->L, S = h->S, k = h->kd;
    int cur = 0;
    PROF(h, st, "gen_conv", launch_gen_conv_dgrad(st, b.g, h->gen_wout, b.act[Dd - 1], b.dpre[cur], N, S, Cd, Cd, 4, k, 1));
    if (train_alpha != 0.f)
        PROF(h, st, "gen_conv", launch_gen_conv_wgrad(st, b.act[Dd - 1], b.g, b.gen_scr, N, S, Cd, Cd, Cd, 4, k, 1, train_alpha,
                                                      h->gacc[ps.out_w], h->gacc[ps.out_b]));
    for (int l = Dd - 1; l > 0; --l) {
        float *gw = h->gacc[ps.dec_w[l]], *gb = h->gacc[ps.dec_b[l]];
        if (train_alpha != 0.f && h->gen_split && gen_split_wgrad_ok(k, Cd))
            PROF(h, st, "gen_conv_f16x3", launch_gen_split_wgrad(st, b.act[l - 1], b.dpre[cur], b.gen_scr, N, S, Cd, k, train_alpha, gw, gb));
        else if (train_alpha != 0.f)
            PROF(h, st, "gen_conv", launch_gen_conv_wgrad(st, b.act[l - 1], b.dpre[cur], b.gen_scr, N, S, Cd, Cd, Cd, Cd, k, 1, train_alpha, gw, gb));
        if (h->gen_split)
            PROF(h, st, "gen_conv_f16x3", launch_gen_split_conv(st, b.dpre[cur], h->gs_wb[l], h->gs_mb[l], nullptr, b.act[l - 1], b.dpre[cur ^ 1], N, S, Cd, k, 0));
        else
            PROF(h, st, "gen_conv", launch_gen_conv_dgrad(st, b.dpre[cur], h->gen_wdec[l], b.act[l - 1], b.dpre[cur ^ 1], N, S, Cd, Cd, Cd, k, 1));
        cur ^= 1;
    }
    HIPCHK(h, launch_zero_fill(st, b.Rc, (size_t)N * 9 * Cd));
    PROF(h, st, "gen_l0", launch_gen_l0_bwd(st, b.dpre[cur], b.z[it], h->gen_wdec[0], h->lin, b.gen_l0, N, L, S, Cd, k, train_alpha,
                                            h->gacc[ps.dec_w[0]], h->gacc[ps.dec_b[0]], b.Rc, 9 * Cd));
    return IODINE_OK;
}

// where one weight-gradient launch of a decoder pass leaves its partial tiles and when they are reduced.  Option wgrad_accum (round 5): a
// block's partial tile accumulates alpha_i x (pass i) in a per-layer buffer and is reduced once, after the last pass (it == T); otherwise
// the shared scratch, reduced with the pass factor straight away
struct WgradPass { float *part, *part_b; float alpha; int accum; float reduce_alpha; bool reduce; };

// single: the pass is the only one of its backward (iodine_decode_backward / iodine_elbo_backward) - first (overwrite the maps accumulated
// over the passes) and last (emit the coordinate / bias gradients, reduce the kept partial tiles) at once; `it` then only names the z buffer
int decoder_backward_data(iodine_handle* h, hipStream_t st, int N, float** dpre0, bool train, float train_alpha, int it, bool single = false)
{
    const bool first = single || it == 0, last = single || it == h->T;
    Buffers& b = h->buf;
    const ParamSlots& ps = h->slot;
    const int Cd = h->Cd, Dd = h->Dd;
    const DecPath path = dec_path(h);
    if (path == DEC_GENERIC) { *dpre0 = nullptr; return decoder_backward_generic(h, st, N, train ? train_alpha : 0.f, it); }
    if (!train) train_alpha = 0.f;                         // (what the launches below were handed for an inference pass)
    const bool zero_w = train && train_alpha == 0.f;       // a training pass whose loss weight is 0
    int cur = 0, nparts = 0, ncop = 4, nb = 0, rc;
    // training: one pass over the last hidden activation gives the data gradient AND the weight / bias gradient
    const bool out_fused = train && dec_f16(path) && h->out_bwd_fused;
    const bool acc_w = train && h->wgrad_accum && !b.wg_acc.empty() && b.wg_acc[0];
    auto wgrad_pass = [&](bool acc, int l) {
        return acc ? WgradPass{b.wg_acc[l], b.wg_acc_b[l], train_alpha, !first, 1.f, last}
                   : WgradPass{b.wg_part, b.wg_part_b, 1.f, 0, train_alpha, true};
    };
    // output conv: only the fused kernel takes a pass factor, so the separate weight-gradient kernels reduce per pass
    WgradPass wp = wgrad_pass(acc_w && out_fused, 0);
#ifdef IODINE_XSKIP_HOOK
    if (!(g_iod_xskip & 256))
#endif
    if (out_fused)
        PROF(h, st, "dec_out_bwd", launch_dec_out_bwd_fused_f16x3(st, b.act[Dd - 1], b.g, h->dec_out_wb16, h->dec_out_meta, b.dpre[cur],
                                                                   path == DEC_WS_F16 ? b.tmax_dpre[cur] : nullptr, wp.part, wp.part_b,
                                                                   N, h->S, Cd, &nparts, &nb, wp.alpha, wp.accum));
    else if ((rc = dec_out_dgrad(h, st, N, cur)))
        return rc;
    if (train && !out_fused && (rc = dec_out_wgrad(h, st, N, wp.part, wp.part_b, &nparts, &ncop, &nb))) return rc;
    if (train && wp.reduce)
        HIPCHK(h, launch_wgrad_reduce(st, wp.part, nparts, Cd, ncop, 4, Cd, Cd, wp.reduce_alpha, h->gacc[ps.out_w], b.wg_fold, wp.part_b, nb,
                                      h->gacc[ps.out_b]));
    bool fused_l0 = false;
    for (int l = Dd - 1; l >= 1; --l) {
        // (a zero-weight pass without kept partial tiles would reduce 0 x its tiles into the accumulator: skipped)
        if (train && !(zero_w && !(acc_w && path != DEC_TILE_F32))) {
            wp = wgrad_pass(acc_w && path != DEC_TILE_F32, l);      // (the LDS-tiled fp32 kernel takes no pass factor)
            if ((rc = dec_conv_wgrad(h, st, N, l, cur, wp.part, wp.part_b, wp.alpha, wp.accum, &nparts, &ncop, &nb))) return rc;
            if (wp.reduce)
                HIPCHK(h, launch_wgrad_reduce(st, wp.part, nparts, Cd, ncop, Cd, Cd, Cd, wp.reduce_alpha, h->gacc[ps.dec_w[l]], b.wg_fold,
                                              wp.part_b, nb, h->gacc[ps.dec_b[l]]));
        }
        // Inference: nothing but the broadcast layer's row / class sums needs d(pre-activation 0), so the last data gradient
        // reduces its tile to per-row sums in its epilogue (EPI_L0ROWS) and the 0.94 GB tensor is neither written nor re-read.
        // Training: the same with one more sum per row (EPI_L0ROWSX, weight-stationary kernel only): class sums for dz and the
        // latent-channel weights, slot-summed row sums for the coordinate-channel weights and the bias.
        fused_l0 = l == 1 && h->fuse_l0 && (dec_f16(path) ? (!train || path == DEC_WS_F16) : path == DEC_WS_F32);
        if ((rc = dec_conv_dgrad(h, st, N, l, cur, fused_l0 ? b.rows_p : b.dpre[cur ^ 1],
                                 fused_l0 ? (train ? EPI_L0ROWSX : EPI_L0ROWS) : EPI_MUL_ELUGRAD)))
            return rc;
        cur ^= 1;
    }
    *dpre0 = b.dpre[cur];
    if (fused_l0 && !train) {
        PROF(h, st, "l0_reduce", launch_l0_reduce_cls_tiles(st, b.rows_p, b.Rc, N, h->S, Cd, b.l0scr));
        return IODINE_OK;
    }
    if (fused_l0) {
        PROF(h, st, "l0_reduce", launch_l0_reduce_cls_tiles_x(st, b.rows_p, b.Rc, b.rown, N, h->S, Cd, b.l0scr));
        HIPCHK(h, launch_l0_rowsum_acc(st, b.rown, N, h->S, Cd, train_alpha, first, b.Rsum));
    } else
    // row / class sums of dpre0 for dz; in training the same read also feeds the slot-summed gradient map, which is
    // accumulated (with this pass's factor) over the T+1 passes and consumed once after the last one
    PROF(h, st, "l0_reduce", launch_l0_reduce(st, *dpre0, b.rows, b.Rc, N, h->S, Cd, train ? b.Dpart : nullptr,
                                              b.Dsum, train_alpha, first));
    if (train) {
        // layer 0 (spatial broadcast): latent-channel weights from z and the per-tap sums, coordinate channels
        // and bias from the slot-summed gradient map
        float *gw = h->gacc[ps.dec_w[0]], *gb = h->gacc[ps.dec_b[0]];
        if (zero_w) {                                       // gw += 0 x (this pass)
        } else if (sgemm_tn_mfma_ok(h->L, 9 * Cd, N)) {     // z^T . RT on fp32 MFMA, accumulated straight into gw[co][ci][tap]
            HIPCHK(h, launch_l0_tap_sums(st, b.Rc, b.RT, N, Cd));
            HIPCHK(h, launch_sgemm_tn_mfma(st, h->L, 9 * Cd, N, train_alpha, b.z[it], h->L, b.RT, 9 * Cd, 1.f, gw, h->L + 2, 1, Cd));
        } else                                              // (round 6) tap sums + product + scatter in one launch
            HIPCHK(h, launch_l0_latent_wgrad(st, b.Rc, b.z[it], N, h->L, Cd, train_alpha, gw));
        if (last) {
            if (fused_l0) HIPCHK(h, launch_l0_coord_grads_rows(st, b.Rsum, h->lin, h->S, Cd, h->L, 1.f, gw, gb));
            else HIPCHK(h, launch_l0_coord_grads(st, b.Dsum, h->lin, h->S, Cd, h->L, 1.f, gw, gb, b.wg_part));
        }
    }
    return IODINE_OK;
}

// the image ELBO evaluation i scores, differentiates and encodes: frame i of a clip (iodine_set_frames), else the one image
const float* x4_frame(const iodine_handle* h, int i)
{
    return h->buf.x4 + (h->frames > 0 ? (size_t)i * h->buf.B * h->P * 4 : 0);
}

// elbo() + inner backward + get_input_encoding for iteration i (iodine.py:85-93 / 133-142)
// sgrad: also leave d LL_i / d sigma in buf.sgrad[i] (option sigma_grad; the callers that offer it: training forward, saved elbo)
int elbo_and_gradients(iodine_handle* h, hipStream_t st, int B, const float* eps_i, int i, bool need_grads,
                       bool train = false, float train_alpha = 0.f, bool sgrad = false, int igrad = 0, float ig_coef = 0.f)
{
    const float sigma = (float)h->obj.sigma, beta = (float)h->obj.beta;     // the handle's current objective (iodine_set_objective)
    Buffers& b = h->buf;
    const int N = B * h->K;
    HIPCHK(h, launch_dec_v(st, b.pm, b.plv, eps_i, nullptr, h->wcls, b.z[i], b.V, N, h->L, h->Cd));
    int rc = decoder_forward(h, st, N, b.z[i]);
    if (rc) return rc;
    PROF(h, st, "pixel_pass1", launch_pixel_pass1(st, x4_frame(h, i), b.dec_out, b.g, b.part, B, h->K, h->P, sigma, h->precision == 0));
    // the ticket of pixel_finalize_elbo_kernel is reset by the last block of every launch; the first launch of an entry point also
    // starts from a fresh 0 (a memset node under graph capture), whatever a failed call or a misuse of the handle from a second
    // stream left in it - once per call, not per launch (a memset is a launch of its own)
    if (i == 0) HIPCHK(h, hipMemsetAsync(h->elbo_counter, 0, sizeof(unsigned), st));
    HIPCHK(h, launch_pixel_finalize_elbo(st, b.part, B, h->K, h->P, h->cfg.layernorm, b.lnstat, b.ll_img, b.pm, b.plv, h->L,
                                         b.img_terms + (size_t)i * B * 2, b.scal + 3 * i, h->elbo_counter, beta));
    if (sgrad)
        PROF(h, st, "pixel_sigma_grad", launch_pixel_sigma_grad(st, x4_frame(h, i), b.dec_out, b.sg_part, b.sgrad + i, B, h->K, h->P, h->obj.sigma,
                                                                h->precision == 0));
    if (igrad) {
        // igrad: the bits of option input_grad; buf.ig_x / ig_w += ig_coef x d (B LL_i) / d (x, w).  A still image (and a weight map shared
        // by the frames of a clip) is met by every evaluation: the first one writes, the others add, in evaluation order.  Frame i of a clip
        // (per-frame weights alike) is met by evaluation i alone, and is written in the caller's batch-first layout
        const size_t P = (size_t)h->P, F = train && h->frames > 0 ? (size_t)h->frames : 0;       // (a single elbo takes one image)
        const bool wpf = F && h->ig_call_wpf;
        PROF(h, st, "pixel_input_grad", launch_pixel_input_grad(st, x4_frame(h, i), b.dec_out, (igrad & 1) ? b.ig_x + (F ? i * 3 * P : 0) : nullptr,
                                                                F ? F * 3 * P : 3 * P, (igrad & 2) ? b.ig_w + (wpf ? i * P : 0) : nullptr,
                                                                wpf ? F * P : P, B, h->K, h->P, sigma, h->precision == 0, ig_coef,
                                                                F || i == 0, wpf || i == 0));
    }
    if (!need_grads) return IODINE_OK;
    float* dpre0 = nullptr;
    rc = decoder_backward_data(h, st, N, &dpre0, train, train_alpha, i);
    if (rc) return rc;
    HIPCHK(h, launch_dz_latent(st, b.Rc, dec_path(h) == DEC_GENERIC ? h->gen_ident : h->wclsT, b.pm, b.plv, eps_i, N, h->L, h->Cd, h->cfg.layernorm,
                               b.g_pm[i], b.g_plv[i], b.latent[i], h->Lreal, beta));
    return IODINE_OK;
}

// The per-layer launches of the refinement conv stack, one switch each like the decoder's; none of them writes host state.
// Layer l of iteration i: b.ract[i][l] from an input of size s.  Layer 0 starts from the decoder output and writes the encoding on the way;
// its fused form keeps the encoding on chip unless keep_enc (the backward / iodine_debug_copy("enc") read it).
int ref_conv_fwd(iodine_handle* h, hipStream_t st, const RefForm& f, int i, int l, int s, int B, bool keep_enc)
{
    Buffers& b = h->buf;
    const int N = B * h->K, Cr = h->Cr, cip = l == 0 ? 20 : Cr, f32 = f.fam == REF_S2_F32;
    const float* in = l == 0 ? b.enc[i] : b.ract[i][l - 1];
    const char* cat = l == 0 ? "refine_l0" : "refine_conv";
    if (l == 0 && f.l0f) {
        PROF(h, st, "refine_l0f", launch_refine_l0_fused(st, x4_frame(h, i), b.dec_out, b.lnstat, h->lin, h->ref_l0k, h->ref_l0kmeta, h->ref_l0s, h->ref_l0smeta,
                                                         h->ref_b[0], b.ract[i][0], keep_enc ? b.enck[i] : nullptr, keep_enc ? b.encs[i] : nullptr, B, h->K,
                                                         h->S, Cr, (float)h->obj.sigma, h->enc_chmask, h->stable_enc));
        return IODINE_OK;
    }
    if (l == 0)
        PROF(h, st, "pixel_pass2", launch_pixel_pass2(st, x4_frame(h, i), b.dec_out, b.lnstat, h->lin, f.split ? b.enck[i] : b.enc[i], B, h->K, h->S,
                                                      (float)h->obj.sigma, f.split ? b.encs[i] : nullptr, h->enc_chmask, h->precision == 0, h->stable_enc));
    switch (f.fam) {
    case REF_GENERIC:
        PROF(h, st, "gen_conv", launch_gen_conv_fwd(st, in, h->gen_wref[l], h->ref_b[l], b.ract[i][l], N, s, l == 0 ? 17 : Cr, cip, Cr, h->kr, h->rs, 1,
                                                    l == 0 ? h->enc_chmask : 0xffffffffu));
        break;
    case REF_S2_F16: case REF_S2_F32:
        if (l == 0 && f.split) {                           // the per-image channels once per image, then the per-slot ones on top
            PROF(h, st, cat, launch_conv3x3_s2_f16x3(st, b.encs[i], h->ref_wsh16, h->ref_wshmeta, nullptr, b.rmap, B, s, 8, Cr, nullptr, 0, f32));
            PROF(h, st, cat, launch_conv3x3_s2_f16x3(st, b.enck[i], h->ref_wk16, h->ref_wkmeta, h->ref_b[0], b.ract[i][0], N, s, 12, Cr, b.rmap, h->K, f32));
        } else if (ref_layer_ws(h, f, l, s))
            PROF(h, st, cat, launch_conv3x3_s2ws_f16x3(st, in, h->ref_wsf[l], h->ref_wsf_meta[l], h->ref_b[l], b.ract[i][l], N, s, Cr, f32));
        else
            PROF(h, st, cat, launch_conv3x3_s2_f16x3(st, in, h->ref_wf16[l], h->ref_wmeta[l], h->ref_b[l], b.ract[i][l], N, s, cip, Cr, nullptr, 0, f32));
        break;
    case REF_GATHER: PROF(h, st, cat, launch_conv3x3_gather(st, in, h->ref_w[l], h->ref_b[l], b.ract[i][l], N, s, s, cip, Cr, 2)); break;
    }
    return IODINE_OK;
}

// weight / bias gradient of layer l (input size s) over all NT slot-images into the accumulators.  split: the saved forward left layer 0's
// input in the split layout; fuse01: layer 1's data gradient rides in layer 0's launch (ref_bwd01)
int ref_conv_wgrad(iodine_handle* h, hipStream_t st, int NT, int l, int s, bool split, bool fuse01)
{
    Buffers& b = h->buf;
    const int Cr = h->Cr, cip = l == 0 ? 20 : Cr, ireal = l == 0 ? 17 : Cr, so = ref_out_size(h, s), f32 = h->precision == 0;
    const float* in = l == 0 ? b.enc[0] : b.ract[0][l - 1];
    int nparts = 0, cipad = 0, nb = 0;
    float *gb = h->gacc[h->slot.ref_b[l]], *gw = h->gacc[h->slot.ref_w[l]];
    // the destination: the accumulator itself, or (first layer of an ARCH.ENCODING subset) a 17-channel scratch gathered into it afterwards
    const bool gather0 = l == 0 && h->n_in < 17;
    float* gw_dst = gather0 ? h->ref_g17 : gw;
    if (gather0) HIPCHK(h, launch_zero_fill(st, h->ref_g17, (size_t)Cr * 17 * h->kr * h->kr));
    switch (ref_family(h)) {
    case REF_GENERIC:
        PROF(h, st, "gen_conv", launch_gen_conv_wgrad(st, in, b.rdpre[l], b.gen_scr, NT, s, ireal, cip, ireal, Cr, h->kr, h->rs, 1.f, gw_dst, gb,
                                                      l == 0 ? h->enc_chmask : 0xffffffffu));
        break;
    case REF_S2_F16: case REF_S2_F32: {
        // split first layer: 12 per-slot + 8 per-image channels from two tensors, gradient in the internal channel order, then unsplit
        const bool split0 = l == 0 && split;
        if (split0 && fuse01)
            PROF(h, st, "refine_bwd01", launch_refine_bwd01(st, b.rdpre[1], h->ref_w1ws, h->ref_w1ws_meta, b.ract[0][0], b.enck[0], b.encs[0], b.wg_part,
                                                            b.wg_part_b, NT, s, Cr, h->K, &nparts, &cipad, &nb));
        else
            PROF(h, st, "refine_wgrad", launch_conv3x3_s2_wgrad_f16x3(st, split0 ? b.enck[0] : in, b.rdpre[l], b.wg_part, b.wg_part_b, NT, s, cip, Cr, &nparts,
                                                                      &cipad, &nb, split0 ? b.encs[0] : nullptr, split0 ? h->K : 0, f32));
        const int ir = split0 ? 20 : ireal;
        if (split0) HIPCHK(h, launch_zero_fill(st, h->ref_g20, (size_t)Cr * 20 * 9));
        HIPCHK(h, launch_wgrad_reduce(st, b.wg_part, nparts, cipad, Cr, Cr, ir, ir, 1.f, split0 ? h->ref_g20 : gw_dst, b.wg_fold, b.wg_part_b, nb, gb));
        if (split0) HIPCHK(h, launch_ref_unsplit_grad(st, h->ref_g20, Cr, gw_dst));
        break;
    }
    case REF_GATHER:
        PROF(h, st, "refine_wgrad", launch_conv3x3_wgrad_gather(st, in, b.rdpre[l], b.wg_part, NT, s, s, cip, Cr, 2, &nparts, &cipad));
        HIPCHK(h, launch_wgrad_reduce(st, b.wg_part, nparts, cipad, Cr, Cr, ireal, ireal, 1.f, gw_dst, b.wg_fold));
        PROF(h, st, "refine_bias_grad", launch_colsum_tall(st, b.rdpre[l], NT * so * so, Cr, 1.f, gb, b.wg_part_b, (size_t)512 * 64));
        break;
    }
    if (gather0) HIPCHK(h, launch_enc_gather_grad(st, h->ref_g17, Cr, h->n_in, h->enc_map, gw, h->kr * h->kr));
    return IODINE_OK;
}

// data gradient of layer l >= 1 (input size s): b.rdpre[l] -> b.rdpre[l - 1]
int ref_conv_dgrad(iodine_handle* h, hipStream_t st, int NT, int l, int s)
{
    Buffers& b = h->buf;
    float *d = b.rdpre[l], *out = b.rdpre[l - 1], *act = b.ract[0][l - 1];
    switch (ref_family(h)) {
    case REF_GENERIC: PROF(h, st, "gen_conv", launch_gen_conv_dgrad(st, d, h->gen_wref[l], act, out, NT, s, h->Cr, h->Cr, h->Cr, h->kr, h->rs)); break;
    case REF_S2_F16: case REF_S2_F32:
        PROF(h, st, "refine_dgrad", launch_conv3x3_s2_dgrad_f16x3(st, d, h->ref_wb16[l], h->ref_wmeta[l] + 2, act, out, NT, s, h->Cr, h->precision == 0));
        break;
    case REF_GATHER: PROF(h, st, "refine_dgrad", launch_conv3x3_gather_dgrad(st, d, h->ref_wb[l], act, out, NT, s, s, h->Cr, 2)); break;
    }
    return IODINE_OK;
}

// Backward of the conv stack, last layer first, for ALL iterations at once: its inputs are detached (iodine.py:343), so the T passes only meet
// in the weight gradients - one batch of NT = T * N slot-images per layer (the saved inputs / activations lie back to back, plan()) instead
// of T launches over N each.  fwd_split: the layout the saved forward left its inputs in (CallState::fwd_split).
int refine_stack_backward(iodine_handle* h, hipStream_t st, int NT, bool fwd_split)
{
    Buffers& b = h->buf;
    std::vector<int> sz(h->Dr + 1, h->S);
    for (int l = 0; l < h->Dr; ++l) sz[l + 1] = ref_out_size(h, sz[l]);
    HIPCHK(h, launch_pool_bwd(st, b.dpooled, b.ract[0][h->Dr - 1], b.rdpre[h->Dr - 1], NT, sz[h->Dr] * sz[h->Dr], h->Cr));
    const bool fuse01 = ref_bwd01(h, fwd_split);           // d(pre-activation 0), the largest tensor of this backward, never leaves the chip
    for (int l = h->Dr - 1; l >= 0; --l) {
        if (int r = ref_conv_wgrad(h, st, NT, l, sz[l], fwd_split, fuse01)) return r;
        if (l > 1 || (l == 1 && !fuse01))
            if (int r = ref_conv_dgrad(h, st, NT, l, sz[l])) return r;
    }
    return IODINE_OK;
}

// refine() + posterior.update() for iteration i (iodine.py:95-100 / 144-145)
int refine_step(iodine_handle* h, hipStream_t st, int B, int i, bool save)
{
    Buffers& b = h->buf;
    const int N = B * h->K;
    const RefForm f = ref_form(h);
    int s = h->S;
    for (int l = 0; l < h->Dr; ++l, s = ref_out_size(h, s))
        if (int r = ref_conv_fwd(h, st, f, i, l, s, B, save || h->stop_after >= 0)) return r;
    PROF(h, st, "refine_head", launch_refine_head(st, b.ract[i][h->Dr - 1], N, s * s, h->Cr, h->H, h->L, h->mlp_wT, h->mlp_b, h->wihT, h->whhT, h->lstm_b,
                                 h->wmT, h->bm, h->wvT, h->bv, b.latent[i], b.h[i], b.c[i], b.h[i + 1], b.c[i + 1], b.pm, b.plv,
                                 save ? b.pooled[i] : nullptr, save ? b.u[i] : nullptr, save ? b.gates[i] : nullptr, save ? b.xin[i] : nullptr,
                                 nullptr, nullptr, b.head_xh, b.head_gp, h->head_mfma));   // (the form: refine_head_form; head_mfma where both fit)
    return IODINE_OK;
}

int check_ready(iodine_handle* h, int batch)
{
    if (!h) return IODINE_ERR_INVALID;
    if (!h->params_set) return h->fail(IODINE_ERR_STATE, "iodine_set_params has not been called");
    if (batch < 1) return h->fail(IODINE_ERR_INVALID, "batch must be >= 1");
    // several kernels index one activation tensor [N][P][C] with 32-bit element offsets
    const size_t cmax = (size_t)std::max(std::max(h->Cd, h->Cr), 20);
    if ((size_t)batch * h->K * h->P * cmax >= ((size_t)1 << 31))
        return h->fail(IODINE_ERR_INVALID, "batch too large for one device: batch * slots * pixels * channels must stay below 2^31 "
                                           "(shard the images over ranks, iodine_amd.parallel)");
    return IODINE_OK;
}

// Run `body` (a fixed-shape sequence of launches on `st`) eagerly, or - with option "graph" - through a hipGraph keyed by
// the full argument tuple: the first call with a tuple runs eagerly (it also performs the one-time hipFuncSetAttribute
// calls of the launchers), the second is captured + instantiated, later ones are a single hipGraphLaunch.  Host-side state
// changes must NOT live in `body` (a replay does not execute it).
template <typename F>
int run_graphed(iodine_handle* h, hipStream_t st, const std::vector<uintptr_t>& key, F&& body)
{
    if (!h->graph || h->profile) return body();
    if (!st) return h->fail(IODINE_ERR_INVALID, "option graph=1 needs a non-default stream (the legacy null stream cannot be captured)");
    for (auto& g : h->graphs)
        if (g.key == key) {
            g.used = ++h->graph_clock;
            HIPCHK(h, hipGraphLaunch(g.exec, st));
            ++h->graph_replays;
            return IODINE_OK;
        }
    bool seen = false;
    for (auto& k : h->seen_keys) if (k == key) { seen = true; break; }
    if (!seen) {
        if (h->seen_keys.size() >= 64) h->seen_keys.clear();
        h->seen_keys.push_back(key);
        return body();
    }
    HIPCHK(h, hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
    const int rc = body();
    hipGraph_t graph = nullptr;
    const hipError_t e = hipStreamEndCapture(st, &graph);
    if (rc) { if (graph) (void)hipGraphDestroy(graph); return rc; }
    if (e != hipSuccess) return h->fail(IODINE_ERR_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(e));
    GraphEntry ge;
    ge.key = key; ge.graph = graph;
    const hipError_t e2 = hipGraphInstantiate(&ge.exec, graph, nullptr, nullptr, 0);
    if (e2 != hipSuccess) { (void)hipGraphDestroy(graph); return h->fail(IODINE_ERR_HIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(e2)); }
    if (h->graphs.size() >= 8) {                           // least recently used out
        size_t lru = 0;
        for (size_t i = 1; i < h->graphs.size(); ++i) if (h->graphs[i].used < h->graphs[lru].used) lru = i;
        (void)hipGraphExecDestroy(h->graphs[lru].exec); (void)hipGraphDestroy(h->graphs[lru].graph);
        h->graphs.erase(h->graphs.begin() + lru);
    }
    ge.used = ++h->graph_clock;
    h->graphs.push_back(ge);
    ++h->graph_captures;
    HIPCHK(h, hipGraphLaunch(ge.exec, st));
    return IODINE_OK;
}

// first element of a graph key: the entry point (1, 4, 5: reconstruct, train forward, train backward)
enum { GK_DECODE = 2, GK_ELBO = 3, GK_DECODE_SAVED = 6, GK_ELBO_SAVED = 7, GK_DECODE_BWD = 8, GK_ELBO_BWD = 9 };

// o: the objective the body runs with - host scalars are baked into the captured nodes, so the key carries the bit patterns of sigma and
// beta and the generation of the weight table (the handle's current objective; a backward passes the one its forward saved)
// pw: the pixel weights of a call that packs x - the captured pack kernel bakes the pointer and the flag like every other address
std::vector<uintptr_t> graph_key(const iodine_handle* h, int entry, int batch, std::initializer_list<const void*> ptrs, const Objective* o = nullptr,
                                 const PixelWeights* pw = nullptr)
{
    if (!o) o = &h->obj;
    uint64_t sb, bb;
    memcpy(&sb, &o->sigma, 8); memcpy(&bb, &o->beta, 8);
    std::vector<uintptr_t> k = {(uintptr_t)entry, (uintptr_t)batch, (uintptr_t)h->K, (uintptr_t)h->T, (uintptr_t)h->stop_after, (uintptr_t)h->precision,
                                (uintptr_t)h->variant, (uintptr_t)h->fuse_l0, (uintptr_t)h->out_bwd_fused, (uintptr_t)h->refine_split, (uintptr_t)(h->head_fused | (h->refine_bwd_fused << 1) | (h->refine_ws << 2) | (h->refine_l0_fused << 3) | (h->head_mfma << 4) | (h->wgrad_accum << 5) | (h->dec_out_rows << 6) | (h->gen_precision << 7) | (h->sigma_grad << 8) | (h->stable_enc << 9) | (h->input_grad << 10)),
                                (uintptr_t)(h->ws_user ? h->ws_user : h->ws_own), (uintptr_t)h->frames};
    k.push_back((uintptr_t)sb); k.push_back((uintptr_t)bb); k.push_back((uintptr_t)o->wgen);
    k.push_back((uintptr_t)(pw ? pw->w : nullptr)); k.push_back((uintptr_t)(pw ? pw->per_frame : 0));
    for (const void* p : ptrs) k.push_back((uintptr_t)p);
    return k;
}

}  // namespace

// ---- the host-only refusals of the entry points (see iodine_internal.h): nothing below launches, allocates or changes state

int set_params_check(iodine_handle* h, const float* const* dev, int n)
{
    if (n != (int)h->params.size() || !dev) return h->fail(IODINE_ERR_INVALID, "iodine_set_params: wrong parameter count");
    for (int i = 0; i < n; ++i)
        if (!dev[i]) return h->fail(IODINE_ERR_INVALID, "iodine_set_params: null pointer for " + h->params[i].name);
    return IODINE_OK;
}

int reconstruct_check(iodine_handle* h, int batch, const float* x, const float* eps, const float* const* state_in, float* const* traj)
{
    if (state_in && !(state_in[0] && state_in[1] && state_in[2] && state_in[3]))
        return h->fail(IODINE_ERR_INVALID, "iodine_reconstruct_seq: an initial state needs all four tensors - post_mean, post_logvar (B,K,L) and "
                                           "the LSTM state h, c (B,K,MLP_UNITS)");
    if (traj && !(traj[0] && traj[1] && traj[2] && traj[3] && traj[4]))
        return h->fail(IODINE_ERR_INVALID, "iodine_reconstruct_seq: a trajectory needs all five buffers - pred, mask, mean (T+1,B,..) and kl, ll (T,B)");
    if (h->frames > 0 && h->frames != h->T) {
        char m[256];
        snprintf(m, sizeof m, "iodine_reconstruct: the frames setting is %d, but a call of %d iterations makes %d ELBO evaluations: it takes "
                              "x of shape (B, %d, 3, %d, %d), one frame per evaluation (or frames 0: one image (B, 3, %d, %d))",
                 h->frames, h->T, h->T, h->T, h->S, h->S, h->S, h->S);
        return h->fail(IODINE_ERR_INVALID, m);
    }
    if (traj && h->stop_after >= 0 && h->stop_after <= h->T)
        return h->fail(IODINE_ERR_INVALID, "iodine_reconstruct_seq: a trajectory has T + 1 entries, the last one the final decode - not "
                                           "available with option stop_after_iters (which skips it)");
    if (int rc = check_ready(h, batch)) return rc;
    if (!x || !eps) return h->fail(IODINE_ERR_INVALID, "iodine_reconstruct: x and eps are required");
    return IODINE_OK;
}

int decode_check(iodine_handle* h, int batch, const float* z)
{
    if (int rc = check_ready(h, batch)) return rc;
    if (!z) return h->fail(IODINE_ERR_INVALID, "iodine_decode: z is required");
    return IODINE_OK;
}

// every index of the host arrays is checked here, before anything is launched: none reaches a kernel unchecked
int scene_edit_check(iodine_handle* h, int batch, const float* z, int n_edits, const int* image, const int* slot, const int* kind,
                     const float* z_new, int chunk_images)
{
    if (int rc = check_ready(h, batch)) return rc;
    char m[256];
    if (!z) return h->fail(IODINE_ERR_INVALID, "iodine_scene_edit: z is required");
    if (n_edits < 1 || !image || !slot || !kind)
        return h->fail(IODINE_ERR_INVALID, "iodine_scene_edit: n_edits must be >= 1, with the host arrays image, slot and kind of n_edits entries each");
    if (chunk_images != 0 && chunk_images < batch) {
        snprintf(m, sizeof m, "iodine_scene_edit: chunk_images = %d is smaller than the batch of %d images (the arena holds the base decode; "
                              "0 = the batch)", chunk_images, batch);
        return h->fail(IODINE_ERR_INVALID, m);
    }
    for (int e = 0; e < n_edits; ++e) {
        const char* bad = nullptr;
        if (image[e] < 0 || image[e] >= batch) { snprintf(m, sizeof m, "iodine_scene_edit: edit %d: image %d is outside 0..%d", e, image[e], batch - 1); bad = m; }
        else if (slot[e] < 0 || slot[e] >= h->K) { snprintf(m, sizeof m, "iodine_scene_edit: edit %d: slot %d is outside 0..%d (the run shape has %d slots)", e, slot[e], h->K - 1, h->K); bad = m; }
        else if (kind[e] != 0 && kind[e] != 1) { snprintf(m, sizeof m, "iodine_scene_edit: edit %d: kind %d is neither 0 (replace) nor 1 (remove)", e, kind[e]); bad = m; }
        else if (kind[e] == 1 && h->K == 1) { snprintf(m, sizeof m, "iodine_scene_edit: edit %d: removes the only slot of image %d (K = 1 leaves nothing to render)", e, image[e]); bad = m; }
        else if (kind[e] == 0 && !z_new) { snprintf(m, sizeof m, "iodine_scene_edit: edit %d: replaces slot %d of image %d, but z_new is NULL", e, slot[e], image[e]); bad = m; }
        if (bad) return h->fail(IODINE_ERR_INVALID, bad);
    }
    if (chunk_images > batch) return check_ready(h, chunk_images);      // the arena (and the edit decodes) run at chunk_images
    return IODINE_OK;
}

int predictive_check(iodine_handle* h, int batch, int n_samples, const float* post_mean, const float* post_logvar, const float* eps,
                     const float* x, int chunk_images, const float* ll)
{
    if (int rc = check_ready(h, batch)) return rc;
    char m[256];
    if (n_samples < 1) {
        snprintf(m, sizeof m, "iodine_predictive: n_samples must be >= 1 (got %d)", n_samples);
        return h->fail(IODINE_ERR_INVALID, m);
    }
    if (n_samples > PREDICTIVE_MAX_SAMPLES) {
        snprintf(m, sizeof m, "iodine_predictive: n_samples = %d is above %d: the running moments divide by the sample index as an fp32 number, "
                              "exact up to 2^24 - far below the count at which the int32 votes could wrap", n_samples, PREDICTIVE_MAX_SAMPLES);
        return h->fail(IODINE_ERR_INVALID, m);
    }
    if (!eps) return h->fail(IODINE_ERR_INVALID, "iodine_predictive: eps (n_samples, B, K, L) is required");
    if ((post_mean == nullptr) != (post_logvar == nullptr))
        return h->fail(IODINE_ERR_INVALID, "iodine_predictive: pass both post_mean and post_logvar, or neither");
    if (chunk_images != 0 && chunk_images < batch) {
        snprintf(m, sizeof m, "iodine_predictive: chunk_images = %d is smaller than the batch of %d images (a chunk holds every image of at "
                              "least one sample; 0 = the batch)", chunk_images, batch);
        return h->fail(IODINE_ERR_INVALID, m);
    }
    if (ll && !x) return h->fail(IODINE_ERR_INVALID, "iodine_predictive: ll is the likelihood of x under every sample, but x is NULL");
    if (batch > 65535) return h->fail(IODINE_ERR_INVALID, "iodine_predictive: batch above 65535 images (one grid row per image): run the images in groups");
    if (chunk_images > batch) return check_ready(h, chunk_images);      // the arena (and the chunk decodes) run at chunk_images
    return IODINE_OK;
}

int elbo_check(iodine_handle* h, int batch, const float* x, const float* eps, const float* post_mean, const float* post_logvar)
{
    if (int rc = check_ready(h, batch)) return rc;
    if (!x || !eps) return h->fail(IODINE_ERR_INVALID, "iodine_elbo: x and eps are required");
    if ((post_mean == nullptr) != (post_logvar == nullptr))
        return h->fail(IODINE_ERR_INVALID, "iodine_elbo: pass both post_mean and post_logvar, or neither");
    return IODINE_OK;
}

// the list of chosen evaluations of iodine_train_forward_frames / iodine_train_backward_frames (n == 0: nothing to check)
int train_frames_check(iodine_handle* h, const char* who, const int* idx, int n, const void* ptrs)
{
    if (n < 0) return h->fail(IODINE_ERR_INVALID, std::string(who) + ": n_frames must be >= 0");
    if (n == 0) return IODINE_OK;
    if (!idx || !ptrs) return h->fail(IODINE_ERR_INVALID, std::string(who) + ": frame_idx and the array of six pointers are required with n_frames > 0");
    for (int j = 0; j < n; ++j)
        if (idx[j] < 0 || idx[j] > h->T || (j > 0 && idx[j] <= idx[j - 1])) {
            char m[256];
            snprintf(m, sizeof m, ": frame_idx must be ascending and unique with values in 0..%d (a forward of %d iterations makes %d ELBO "
                                  "evaluations); entry %d is %d", h->T, h->T, h->T + 1, j, idx[j]);
            return h->fail(IODINE_ERR_INVALID, std::string(who) + m);
        }
    return IODINE_OK;
}

int train_forward_check(iodine_handle* h, int batch, const float* x, const float* eps, const float* loss, const float* const* state_in,
                        const FrameSet* fr)
{
    char m[256];
    if (fr) if (int rc = train_frames_check(h, "iodine_train_forward_frames", fr->idx, fr->n, fr->out)) return rc;
    if (state_in && !(state_in[0] && state_in[1] && state_in[2] && state_in[3]))
        return h->fail(IODINE_ERR_INVALID, "iodine_train_forward_seq: an initial state needs all four tensors - post_mean, post_logvar (B,K,L) and "
                                           "the LSTM state h, c (B,K,MLP_UNITS)");
    if (h->frames > 0 && h->frames != h->T + 1) {
        snprintf(m, sizeof m, "iodine_train_forward: the frames setting is %d, but a forward of %d iterations makes %d ELBO evaluations: it takes "
                              "x of shape (B, %d, 3, %d, %d), one frame per evaluation (or frames 0: one image (B, 3, %d, %d))",
                 h->frames, h->T, h->T + 1, h->T + 1, h->S, h->S, h->S, h->S);
        return h->fail(IODINE_ERR_INVALID, m);
    }
    if (h->obj.nw != 0 && h->obj.nw != h->T + 1) {
        snprintf(m, sizeof m, "iodine_train_forward: the objective has %d iteration weights, but a forward of %d iterations makes %d ELBO "
                              "evaluations: it takes %d weights (iodine_set_objective; 0 weights = the default (i + 1) / (T + 1))",
                 h->obj.nw, h->T, h->T + 1, h->T + 1);
        return h->fail(IODINE_ERR_INVALID, m);
    }
    if (int rc = check_ready(h, batch)) return rc;
    if (!x || !eps || !loss) return h->fail(IODINE_ERR_INVALID, "iodine_train_forward: x, eps and loss are required");
    // the backward pass runs the refinement conv stack over all T iterations as one batch of T * N slot-images
    if ((size_t)batch * h->K * h->T * h->P * 20 >= ((size_t)1 << 31) || (size_t)batch * h->K * h->T * (size_t)ref_out_size(h, h->S) * ref_out_size(h, h->S) * h->Cr >= ((size_t)1 << 31))
        return h->fail(IODINE_ERR_INVALID, "batch too large for one device in training: batch * slots * iters * pixels * 20 must stay below "
                                           "2^31 (shard the images over ranks, iodine_amd.parallel)");
    return IODINE_OK;
}

int train_backward_check(iodine_handle* h, float* const* param_grads, int n, const AuxCot* aux)
{
    if (!h->calls.fwd_done) return h->fail(IODINE_ERR_STATE, "iodine_train_backward: no iodine_train_forward to differentiate");
    if (n != (int)h->params.size() || !param_grads) return h->fail(IODINE_ERR_INVALID, "iodine_train_backward: wrong parameter count");
    if (h->buf.mode != 1 || h->buf.B != h->calls.fwd_batch || h->buf.K != h->K || h->buf.T != h->T)
        return h->fail(IODINE_ERR_STATE, "iodine_train_backward: the training workspace of the forward pass was re-planned");
    if (aux && aux->frames)
        if (int rc = train_frames_check(h, "iodine_train_backward_frames", aux->frames->idx, aux->frames->n, aux->frames->g)) return rc;
    if (aux && aux->frames && aux->frames->n > 0 && h->Cd < 4)
        return h->fail(IODINE_ERR_INVALID, "iodine_train_backward_frames: needs DEC.CONV_CHAN >= 4");
    if (aux && aux->g_state && !h->calls.fwd_from_state)
        return h->fail(IODINE_ERR_STATE, "iodine_train_backward_seq: g_state asks for the gradient of an initial state, but the saved forward ran "
                                         "without one (iodine_train_forward / iodine_train_forward_seq with state_in = NULL start from "
                                         "posterior.init_mean / init_logvar, which receive that gradient as parameters)");
    return IODINE_OK;
}

// the state a single-pass backward needs: a decode / elbo that ran with option save_for_backward and nothing since
int diff_ready(iodine_handle* h, int kind, const char* who)
{
    if (!h->params_set) return h->fail(IODINE_ERR_STATE, std::string(who) + ": iodine_set_params has not been called");
    if (h->calls.diff_kind != kind)
        return h->fail(IODINE_ERR_STATE, std::string(who) + (kind == 1 ? ": no iodine_decode" : ": no iodine_elbo") +
                                             " with option save_for_backward to differentiate (none has run, another compute call has re-used "
                                             "the workspace since, or it was differentiated already)");
    if (h->buf.mode != 2 || h->buf.B != h->calls.diff_batch || h->buf.K != h->K)
        return h->fail(IODINE_ERR_STATE, std::string(who) + ": the workspace of the forward pass was re-planned");
    return IODINE_OK;
}

int decode_backward_check(iodine_handle* h, int batch)
{
    if (int rc = diff_ready(h, 1, "iodine_decode_backward")) return rc;
    if (batch != h->calls.diff_batch) return h->fail(IODINE_ERR_INVALID, "iodine_decode_backward: batch differs from the decode it differentiates");
    return IODINE_OK;
}

// the iodine_last_* readers: is what they read still in the arena, and is count within the batch that left it
static int last_check(iodine_handle* h, bool stale, const char* who, const char* why, int count)
{
    if (stale || h->buf.bytes == 0) return h->fail(IODINE_ERR_STATE, std::string(who) + why);
    if (count < 1 || count > h->calls.last_elbo_batch) return h->fail(IODINE_ERR_INVALID, std::string(who) + ": count must be in 1..batch of the last call");
    return IODINE_OK;
}
int last_elbo_outputs_check(iodine_handle* h, int count)
{
    if (h->calls.redecoded && h->calls.last_elbo_iter >= 0 && h->buf.bytes != 0)
        return h->fail(IODINE_ERR_STATE, "iodine_last_elbo_outputs: iodine_train_backward_frames has decoded an earlier evaluation again since, "
                                         "the decoder output of the forward's final elbo() is gone (read it before the backward)");
    return last_check(h, h->calls.last_elbo_iter < 0, "iodine_last_elbo_outputs", ": no elbo() has run on the current workspace", count);
}
int last_posterior_check(iodine_handle* h, int count)
{
    return last_check(h, h->calls.last_elbo_iter < 0, "iodine_last_posterior", ": no refinement has run on the current workspace", count);
}
int last_refine_state_check(iodine_handle* h, int count)
{
    return last_check(h, h->calls.state_iter < 0 || h->buf.mode != 0, "iodine_last_refine_state",
                      ": no iodine_reconstruct has run on the current workspace, or another compute call has re-used it since", count);
}
int last_train_state_check(iodine_handle* h, int count)
{
    return last_check(h, h->calls.state_iter < 0 || h->buf.mode != 1, "iodine_last_train_state",
                      ": no iodine_train_forward has run on the current workspace, or another compute call has re-used it since", count);
}

extern "C" {

int iodine_abi_version(void) { return IODINE_ABI_VERSION; }

const char* iodine_last_error(const iodine_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

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
    hipStream_t st = (hipStream_t)stream;
    const ParamSlots& ps = h->slot;
    // plain copies (biases, raw weights of the head backward) are collected and issued as one launch
    MultiCopy mc;
    mc.count = 0;
    auto queue_copy = [&](float* dst, const float* src, size_t count) -> hipError_t {
        if (mc.count == MCOPY_MAX) {
            const hipError_t e = launch_multi_copy(st, mc);
            if (e != hipSuccess) return e;
            mc.count = 0;
        }
        mc.src[mc.count] = src; mc.src2[mc.count] = nullptr; mc.dst[mc.count] = dst; mc.n[mc.count] = (int)count; mc.op[mc.count] = 0;
        mc.cols[mc.count] = 0; ++mc.count;
        return hipSuccess;
    };
    // (round 5) the head's transposes [R][Cc] -> [Cc][R] and the bias sum ride in the same launch as the plain copies
    auto queue_transpose = [&](float* dst, const float* src, int R, int Cc) -> hipError_t {
        const hipError_t e = queue_copy(dst, src, (size_t)R * Cc);
        if (e == hipSuccess) { mc.op[mc.count - 1] = 1; mc.cols[mc.count - 1] = Cc; }
        return e;
    };
    auto queue_add2 = [&](float* dst, const float* a, const float* b2, int count) -> hipError_t {
        const hipError_t e = queue_copy(dst, a, (size_t)count);
        if (e == hipSuccess) { mc.op[mc.count - 1] = 2; mc.src2[mc.count - 1] = b2; }
        return e;
    };
    const int L = h->L, Cd = h->Cd, Cr = h->Cr, H = h->H;
    // split-fp16 packs (power-of-two scale + layout per tensor and direction) are collected and issued as two launches at the end
    std::vector<PackJob> pj;
    auto pack_ws = [&](const float* src, int C, int tflip, float* meta, void* dst) {
        pj.push_back(PackJob{src, dst, meta, 0, {C, tflip, 0, 0, 0}});
        return hipSuccess;
    };
    auto pack_f16 = [&](const float* src, int O, int I, int cin, int cout, int tflip, float* meta, void* dst) {
        pj.push_back(PackJob{src, dst, meta, 1, {O, I, cin, cout, tflip}});
        return hipSuccess;
    };
    const DecPath path = dec_path(h);
    if (path == DEC_GENERIC) {
        // fallback path: [tap][ci][co] packs of every conv, plain bias copies, the head below as on the tuned path
        for (int l = 0; l < h->Dd; ++l) {
            HIPCHK(h, launch_gen_pack_weights(st, dev[ps.dec_w[l]], Cd, l == 0 ? L + 2 : Cd, h->kd, h->gen_wdec[l]));
            if (l > 0) HIPCHK(h, queue_copy(h->dec_b[l], dev[ps.dec_b[l]], Cd));
        }
        // bias + the conv of the two coordinate channels of the broadcast layer: the same map for every slot-image
        HIPCHK(h, launch_gen_l0_coord(st, h->gen_wdec[0], dev[ps.dec_b[0]], h->lin, L, h->S, Cd, h->kd, h->gen_cterm));
        HIPCHK(h, launch_gen_pack_weights(st, dev[ps.out_w], 4, Cd, h->kd, h->gen_wout));
        HIPCHK(h, queue_copy(h->dec_out_b, dev[ps.out_b], 4));
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
    }
    const RefFamily fam = ref_family(h);
    for (int l = 0; l < h->Dr && fam == REF_GENERIC; ++l) {   // (the generic stack's packs in front of the decoder's, the other families' behind)
        const float* w = dev[ps.ref_w[l]];
        if (l == 0 && h->n_in < 17) { HIPCHK(h, launch_enc_expand_weights(st, w, Cr, h->n_in, h->enc_map, h->ref_w17, h->kr * h->kr)); w = h->ref_w17; }
        HIPCHK(h, launch_gen_pack_weights(st, w, Cr, l == 0 ? 17 : Cr, h->kr, h->gen_wref[l]));
        HIPCHK(h, queue_copy(h->ref_b[l], dev[ps.ref_b[l]], Cr));
    }
    if (path != DEC_GENERIC) {
    // decoder
    HIPCHK(h, launch_dec_l0_prepare(st, dev[ps.dec_w[0]], dev[ps.dec_b[0]], h->lin, Cd, L, h->S, h->wcls, h->wclsT, h->cmap));
    for (int l = 1; l < h->Dd; ++l) {
        // only the selected path's packs - the ones dec_conv_fwd / dec_conv_dgrad read - are maintained (a change of conv_variant /
        // conv_precision invalidates the parameters)
        const float* w = dev[ps.dec_w[l]];
        switch (path) {
        case DEC_WS_F16:                                       // weight-stationary register layout
            HIPCHK(h, pack_ws(w, Cd, 0, h->dec_wmeta[l], h->dec_wsf[l]));
            HIPCHK(h, pack_ws(w, Cd, 1, h->dec_wmeta[l] + 2, h->dec_wsb[l]));
            break;
        case DEC_TILE_F16:
            HIPCHK(h, pack_f16(w, Cd, Cd, Cd, Cd, 0, h->dec_wmeta[l], h->dec_wf16[l]));
            HIPCHK(h, pack_f16(w, Cd, Cd, Cd, Cd, 1, h->dec_wmeta[l] + 2, h->dec_wb16[l]));
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
        HIPCHK(h, queue_copy(h->dec_b[l], dev[ps.dec_b[l]], Cd));
    }
    HIPCHK(h, queue_copy(h->dec_out_b, dev[ps.out_b], 4));
    if (dec_f16(path)) {
        // split-fp16 GEMM-form packs of the output conv, forward and data gradient (one scale): two more jobs of the batched pack
        pj.push_back(PackJob{dev[ps.out_w], h->dec_out_w16, h->dec_out_meta, 3, {Cd, 0, 0, 0, 0}});
        pj.push_back(PackJob{dev[ps.out_w], h->dec_out_wb16, h->dec_out_meta, 4, {Cd, 1, 0, 0, 0}});
    } else {                                                   // exact-fp32 forms of the output conv
        HIPCHK(h, launch_pack_dec_out(st, dev[ps.out_w], h->dec_out_w, Cd));
        HIPCHK(h, launch_pack_conv_weights(st, dev[ps.out_w], 4, Cd, 4, Cd, 1, h->dec_out_wb));
        if (h->dec_out_w32) HIPCHK(h, launch_pack_dec_out_rows32(st, dev[ps.out_w], Cd, h->dec_out_w32));
    }
    }   // tuned decoder
    if (fam != REF_GENERIC) {
    // refinement conv stack: every pack of the family, whatever the per-form options say (they do not invalidate the parameters)
    // first layer: the reference weight has n_in input channels (ARCH.ENCODING subset); the kernels see 17
    const float* w0 = dev[ps.ref_w[0]];
    if (h->n_in < 17) { HIPCHK(h, launch_enc_expand_weights(st, w0, Cr, h->n_in, h->enc_map, h->ref_w17)); w0 = h->ref_w17; }
    for (int l = 0; l < h->Dr; ++l) {
        if (fam == REF_GATHER) HIPCHK(h, launch_pack_conv_weights(st, l == 0 ? w0 : dev[ps.ref_w[l]], Cr, l == 0 ? 17 : Cr, l == 0 ? 20 : Cr, Cr, 0, h->ref_w[l]));
        HIPCHK(h, queue_copy(h->ref_b[l], dev[ps.ref_b[l]], Cr));
    }
    switch (fam) {
    case REF_GATHER: for (int l = 1; l < h->Dr; ++l) HIPCHK(h, launch_pack_conv_weights(st, dev[ps.ref_w[l]], Cr, Cr, Cr, Cr, 2, h->ref_wb[l])); break;
    case REF_S2_F16: case REF_S2_F32: {
        // split fp16: jobs of the batched pack; exact fp32: fp32 weights in the same LDS-tile / register layouts, in the same buffers
        const bool f16 = fam == REF_S2_F16;
        auto tile = [&](const float* w, int I, int cin, int tflip, float* meta, void* dst) {
            return f16 ? pack_f16(w, Cr, I, cin, Cr, tflip, meta, dst) : launch_pack_conv_weights_s2f32(st, w, Cr, I, cin, Cr, tflip, dst);
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
            pj.push_back(PackJob{h->ref_wk, h->ref_l0k, h->ref_l0kmeta, 2, {Cr, 12, 0, 0, 0}});
            pj.push_back(PackJob{h->ref_wsh, h->ref_l0s, h->ref_l0smeta, 2, {Cr, 8, 0, 0, 0}});
        }
        for (int l = 1; l < h->Dr && ref_pack_ws(h); ++l)       // weight-stationary forward of layers 1 ..
            HIPCHK(h, f16 ? pack_ws(dev[ps.ref_w[l]], Cr, 0, h->ref_wsf_meta[l], h->ref_wsf[l]) : launch_pack_conv_weights_ws32(st, dev[ps.ref_w[l]], Cr, 0, h->ref_wsf[l]));
        if (f16 && ref_pack_bwd01(h))                          // fused layer-1 / layer-0 backward: W1 as the transposed conv's A operand
            HIPCHK(h, pack_ws(dev[ps.ref_w[1]], Cr, 1, h->ref_w1ws_meta, h->ref_w1ws));
        break;
    }
    case REF_GENERIC: break;                                   // (packed above, in front of the decoder)
    }
    }
    auto copy_raw = [&](float* dst, int slot) { return queue_copy(dst, dev[slot], h->params[slot].numel()); };
    HIPCHK(h, copy_raw(h->raw_mlp_w, ps.mlp_w));
    HIPCHK(h, copy_raw(h->raw_wih, ps.wih));
    HIPCHK(h, copy_raw(h->raw_whh, ps.whh));
    HIPCHK(h, copy_raw(h->raw_wm, ps.wm));
    HIPCHK(h, copy_raw(h->raw_wv, ps.wv));
    // head
    HIPCHK(h, queue_transpose(h->mlp_wT, dev[ps.mlp_w], H, Cr));
    HIPCHK(h, queue_copy(h->mlp_b, dev[ps.mlp_b], H));
    HIPCHK(h, queue_transpose(h->wihT, dev[ps.wih], 4 * H, H + 4 * L));
    HIPCHK(h, queue_transpose(h->whhT, dev[ps.whh], 4 * H, H));
    HIPCHK(h, queue_add2(h->lstm_b, dev[ps.bih], dev[ps.bhh], 4 * H));
    HIPCHK(h, queue_transpose(h->wmT, dev[ps.wm], L, H));
    HIPCHK(h, queue_transpose(h->wvT, dev[ps.wv], L, H));
    HIPCHK(h, queue_copy(h->bm, dev[ps.bm], L));
    HIPCHK(h, queue_copy(h->bv, dev[ps.bv], L));
    HIPCHK(h, queue_copy(h->init_mean, dev[ps.init_mean], L));
    HIPCHK(h, queue_copy(h->init_logvar, dev[ps.init_logvar], L));
    HIPCHK(h, launch_multi_copy(st, mc));
    if (!pj.empty()) HIPCHK(h, launch_pack_batch(st, pj.data(), (int)pj.size()));      // (behind ref_split / enc_expand: stream order)
    h->params_set = true;
    h->calls.saved_passes_gone();
    return IODINE_OK;
}

size_t iodine_workspace_bytes(const iodine_handle* h, int batch, int mode)
{
    if (!h || batch < 1) return 0;
    if (h->shim) return pad_workspace_bytes(h, batch, mode);
    Arena q(nullptr); Buffers tmp; plan(h, batch, mode, q, tmp);
    return tmp.bytes;
}

int iodine_set_workspace(iodine_handle* h, void* dev_ptr, size_t bytes)
{
    if (!h) return IODINE_ERR_INVALID;
    if (h->shim) return pad_set_workspace(h, dev_ptr, bytes);
    if (((uintptr_t)dev_ptr & 255) != 0) return h->fail(IODINE_ERR_INVALID, "workspace must be 256-byte aligned");
    h->ws_user = dev_ptr; h->ws_user_bytes = dev_ptr ? bytes : 0;
    h->buf = Buffers();
    h->calls.arena_gone();
    return IODINE_OK;                    // graphs are keyed by the arena address (see ensure_workspace)
}

int iodine_set_run_shape(iodine_handle* h, int slots, int iters)
{
    if (!h) return IODINE_ERR_INVALID;
    if (h->shim) return pad_set_run_shape(h, slots, iters);
    if (slots < 1 || slots > 16)
        return h->fail(IODINE_ERR_INVALID, "slots must be in 1..16 (the per-pixel kernels keep every slot of a pixel in registers: "
                                           "instantiated for K <= 16)");
    if (iters < 1) return h->fail(IODINE_ERR_INVALID, "iters must be >= 1");
    if (slots != h->K || iters != h->T) h->calls.saved_passes_gone();   // a pending forward ran at the old shape: its backward is refused (IODINE_ERR_STATE)
    // the workspace is re-planned by the next compute call (ensure_workspace keys on the run shape); the state of the last call
    // stays readable at the shape it was produced with (buf.K / buf.T)
    h->K = slots; h->T = iters;
    return IODINE_OK;
}

int iodine_set_frames(iodine_handle* h, int frames)
{
    if (!h) return IODINE_ERR_INVALID;
    if (h->shim) return pad_set_frames(h, frames);
    if (frames < 0) return h->fail(IODINE_ERR_INVALID, "frames must be >= 0 (0: one image per batch entry)");
    if (frames != h->frames) h->calls.saved_passes_gone();   // the workspace is re-planned by the next compute call (ensure_workspace keys on it)
    h->frames = frames;
    return IODINE_OK;
}

int iodine_set_pixel_weights(iodine_handle* h, const float* w_dev, int per_frame)
{
    if (!h) return IODINE_ERR_INVALID;
    if (h->shim) return pad_set_pixel_weights(h, w_dev, per_frame);
    if (w_dev && per_frame && h->frames == 0)
        return h->fail(IODINE_ERR_INVALID, "iodine_set_pixel_weights: per_frame = 1 is one weight image per frame of a clip (B, E, S, S), but the "
                                           "frames setting is 0: x is one image per batch entry (iodine_set_frames; per_frame = 0: weights (B, S, S))");
    h->pix_w = w_dev;
    h->pix_w_per_frame = w_dev && per_frame ? 1 : 0;
    return IODINE_OK;
}

int iodine_set_objective(iodine_handle* h, double sigma, double beta, const double* iter_weights, int n_weights)
{
    if (!h) return IODINE_ERR_INVALID;
    if (h->shim) return pad_set_objective(h, sigma, beta, iter_weights, n_weights);   // (the inner handle holds the objective)
    char m[256];
    if (!(sigma > 0) || !std::isfinite(sigma)) {
        snprintf(m, sizeof m, "iodine_set_objective: sigma must be a finite number > 0 (got %g)", sigma);
        return h->fail(IODINE_ERR_INVALID, m);
    }
    if (!(beta >= 0) || !std::isfinite(beta)) {
        snprintf(m, sizeof m, "iodine_set_objective: beta must be a finite number >= 0 (got %g)", beta);
        return h->fail(IODINE_ERR_INVALID, m);
    }
    if (n_weights < 0 || (n_weights > 0 && !iter_weights))
        return h->fail(IODINE_ERR_INVALID, "iodine_set_objective: n_weights must be >= 0 (0 = the default weighting) and the weights given");
    std::vector<float> w((size_t)n_weights);
    bool any = false;
    for (int i = 0; i < n_weights; ++i) {
        if (!(iter_weights[i] >= 0) || !std::isfinite(iter_weights[i])) {
            snprintf(m, sizeof m, "iodine_set_objective: iteration weight %d must be a finite number >= 0 (got %g)", i, iter_weights[i]);
            return h->fail(IODINE_ERR_INVALID, m);
        }
        w[i] = (float)iter_weights[i];
        any = any || w[i] > 0.f;
    }
    if (n_weights > 0 && !any) return h->fail(IODINE_ERR_INVALID, "iodine_set_objective: the iteration weights are all zero (in fp32): no loss");
    Objective o;
    o.sigma = sigma; o.beta = beta;
    if (n_weights > 0) {
        // content-addressed, immutable tables: work already queued (or a captured graph, or a saved forward's backward) that reads an
        // earlier table keeps reading what it was given; a weighting that comes back finds its table - and its graphs - again
        WeightTable* t = nullptr;
        for (auto& c : h->wtabs) if (c.w == w) { t = &c; break; }
        if (!t) {
            if (h->wtabs.size() >= 64) {
                // a long schedule of distinct weightings: let the queued work finish, then drop the graphs (they hold table addresses) and
                // every table that neither the current objective nor a saved pass refers to
                HIPCHK(h, hipDeviceSynchronize());
                drop_graphs(h);
                for (auto it = h->wtabs.begin(); it != h->wtabs.end();) {
                    const float* d = it->dev;
                    if (d == h->obj.wtab || d == h->calls.fwd_obj.wtab || d == h->calls.diff_obj.wtab) { ++it; continue; }
                    (void)hipFree(it->dev);
                    it = h->wtabs.erase(it);
                }
            }
            void* d = nullptr;
            HIPCHK(h, hipMalloc(&d, sizeof(float) * (size_t)n_weights));
            const hipError_t e = hipMemcpy(d, w.data(), sizeof(float) * (size_t)n_weights, hipMemcpyHostToDevice);
            if (e != hipSuccess) { (void)hipFree(d); return h->fail(IODINE_ERR_HIP, std::string("hipMemcpy (iteration weights): ") + hipGetErrorString(e)); }
            h->wtabs.push_back(WeightTable());
            t = &h->wtabs.back();
            t->w = w; t->dev = (float*)d; t->gen = h->wgen_next++;
        }
        o.wtab = t->dev; o.whost = t->w.data(); o.nw = n_weights; o.wgen = t->gen;
    }
    h->obj = o;                                            // a pending forward keeps its own copy (fwd_obj / diff_obj): nothing is discarded
    return IODINE_OK;
}

int iodine_set_option(iodine_handle* h, const char* key, double value)
{
    if (!h || !key) return IODINE_ERR_INVALID;
    if (h->shim) return pad_set_option(h, key, value);
    if (!strcmp(key, "stop_after_iters")) { h->stop_after = (int)value; return IODINE_OK; }
    if (!strcmp(key, "profile")) { h->profile = (int)value; return IODINE_OK; }
    if (!strcmp(key, "graph")) { h->graph = value != 0; if (!h->graph) drop_graphs(h); return IODINE_OK; }
#ifdef IODINE_XSKIP_HOOK
    if (!strcmp(key, "xskip")) { g_iod_xskip = (int)value; return IODINE_OK; }       // timing-only ablation builds (common.h)
#endif
    if (!strcmp(key, "out_bwd_fused")) { h->out_bwd_fused = value != 0; return IODINE_OK; }
    if (!strcmp(key, "save_for_backward")) { h->save_bwd = value != 0; return IODINE_OK; }
    if (!strcmp(key, "fuse_l0")) { h->fuse_l0 = value != 0; return IODINE_OK; }
    if (!strcmp(key, "sigma_grad")) { h->sigma_grad = value != 0; return IODINE_OK; }
    if (!strcmp(key, "input_grad")) {
        if (value != 0 && value != 1 && value != 2 && value != 3) return h->fail(IODINE_ERR_INVALID, "option input_grad: 0, 1 (image), 2 (pixel weights) or 3 (both)");
        h->input_grad = (int)value;                    // (the next compute call re-plans the workspace: ensure_workspace keys on it)
        return IODINE_OK;
    }
    if (!strcmp(key, "stable_encoding")) { h->stable_enc = value != 0; return IODINE_OK; }
    if (!strcmp(key, "refine_split")) { h->refine_split = value != 0; return IODINE_OK; }
    if (!strcmp(key, "head_fused")) { h->head_fused = value != 0; return IODINE_OK; }
    if (!strcmp(key, "refine_bwd_fused")) { h->refine_bwd_fused = value != 0; return IODINE_OK; }
    if (!strcmp(key, "profile_stride")) {
        if (value < 1) return h->fail(IODINE_ERR_INVALID, "profile_stride must be >= 1");
        h->profile_stride = (int)value; return IODINE_OK;
    }
    if (!strcmp(key, "head_mfma")) { h->head_mfma = value != 0; return IODINE_OK; }
    if (!strcmp(key, "refine_l0_fused")) { h->refine_l0_fused = value != 0; return IODINE_OK; }
    if (!strcmp(key, "refine_ws")) { h->refine_ws = value != 0; return IODINE_OK; }
    if (!strcmp(key, "dec_out_rows")) { h->dec_out_rows = value != 0; return IODINE_OK; }
    if (!strcmp(key, "wgrad_accum")) {
        if (h->wgrad_accum != (value != 0)) { h->buf = Buffers(); h->calls.arena_gone(); }   // the arena is re-planned
        h->wgrad_accum = value != 0; return IODINE_OK;
    }
    if (!strcmp(key, "conv_variant")) {
        if (value != 1 && value != 6) return h->fail(IODINE_ERR_INVALID, "conv_variant must be 1 (LDS-tiled) or 6 (weight-stationary)");
        if (((int)value == 6) != (h->variant == 6)) h->params_set = false;   // the other kernel's weight packs are not kept up to date
        h->variant = (int)value;
        return IODINE_OK;
    }
    if (!strcmp(key, "conv_precision")) {
        if (value != 0 && value != 1 && value != 2)
            return h->fail(IODINE_ERR_INVALID, "conv_precision must be 0 (f32), 1 (f16x3) or 2 (f16x3 with single-product fp16 weight-stationary decoder convs)");
        // the other path's weight packs are not kept up to date (1 and 2 read the same packs; a switch between them invalidates the parameters
        // all the same, so that a saved forward pass is never finished at another precision)
        if (h->precision != (int)value) h->params_set = false;
        h->precision = (int)value;
        return IODINE_OK;
    }
    if (!strcmp(key, "gen_conv_precision")) {
        if (value != 0 && value != 1) return h->fail(IODINE_ERR_INVALID, "gen_conv_precision must be 0 (f32) or 1 (f16x3)");
        if (h->gen_precision != (int)value) h->params_set = false;    // the split packs are built by iodine_set_params
        h->gen_precision = (int)value;
        return IODINE_OK;
    }
    return h->fail(IODINE_ERR_INVALID, std::string("unknown option ") + key);
}

int iodine_reconstruct(iodine_handle* h, void* stream, int batch, const float* x, const float* eps, float* pred,
                       float* mask, float* mean, float* z, float* post_mean, float* post_logvar, float* elbo_iter)
{
    return iodine_reconstruct_seq(h, stream, batch, x, eps, pred, mask, mean, z, post_mean, post_logvar, elbo_iter, nullptr, nullptr);
}

int iodine_reconstruct_seq(iodine_handle* h, void* stream, int batch, const float* x, const float* eps, float* pred,
                           float* mask, float* mean, float* z, float* post_mean, float* post_logvar, float* elbo_iter,
                           const float* const* state_in, float* const* traj)
{
    if (!h) return IODINE_ERR_INVALID;
    if (h->shim) return pad_reconstruct_seq(h, stream, batch, x, eps, pred, mask, mean, z, post_mean, post_logvar, elbo_iter, state_in, traj);
    const PixelWeights pw(h);                              // one-shot: taken before the first refusal
    int rc = reconstruct_check(h, batch, x, eps, state_in, traj);
    if (rc) return rc;
    rc = ensure_workspace(h, batch, 0);
    if (rc) return rc;
    h->calls.compute_begins();                             // the arena is re-used: a saved training forward is gone
    hipStream_t st = (hipStream_t)stream;
    const int B = batch, N = B * h->K, T = h->T;
    const bool partial = h->stop_after >= 0 && h->stop_after <= T;     // debug: stop before the final sample/decode
    const int n_it = partial ? h->stop_after : T;
    auto body = [&]() -> int {
        Buffers& b = h->buf;
        const size_t eps_stride = (size_t)N * h->L;
        PROF(h, st, "frames_in", launch_x_to_nhwc4(st, x, b.x4, B, h->P, h->frames > 0 ? h->frames : 1, pw.w, pw.per_frame && h->frames > 0));
        if (state_in) {
            // continue from (lambda, h, c) of an earlier call instead of Gaussian.init_unit + zero LSTM state (iodine.py:81-83)
            HIPCHK(h, hipMemcpyAsync(b.pm, state_in[0], sizeof(float) * eps_stride, hipMemcpyDeviceToDevice, st));
            HIPCHK(h, hipMemcpyAsync(b.plv, state_in[1], sizeof(float) * eps_stride, hipMemcpyDeviceToDevice, st));
            HIPCHK(h, hipMemcpyAsync(b.h[0], state_in[2], sizeof(float) * (size_t)N * h->H, hipMemcpyDeviceToDevice, st));
            HIPCHK(h, hipMemcpyAsync(b.c[0], state_in[3], sizeof(float) * (size_t)N * h->H, hipMemcpyDeviceToDevice, st));
        } else
            HIPCHK(h, launch_posterior_init(st, h->init_mean, h->init_logvar, b.pm, b.plv, b.h[0], b.c[0], N, h->L, h->H));
        const size_t P = (size_t)h->P;
        for (int i = 0; i < n_it; ++i) {
            int r = elbo_and_gradients(h, st, B, eps + (size_t)i * eps_stride, i, true);
            if (r) return r;
            // trajectory entry i: the decode ELBO evaluation i made (the sample from lambda_i), through the final decode's kernel
            if (traj)
                PROF(h, st, "traj_out", launch_final_out(st, b.dec_out, traj[0] + (size_t)i * B * 3 * P, traj[1] + (size_t)i * N * P,
                                                         traj[2] + (size_t)i * N * 3 * P, nullptr, B, h->K, h->P));
            r = refine_step(h, st, B, i, false);
            if (r) return r;
        }
        if (!partial) {
            // z = posterior.sample(); decode(z)   (iodine.py:103,110).  The decoder writes into the (now free) gradient
            // buffer so that buf.dec_out keeps the outputs of the LAST elbo() call: the reference's self.mean / self.mask
            // and its logger entries are those (iodine.py:226-239), not the final decode.
            HIPCHK(h, launch_dec_v(st, b.pm, b.plv, eps + (size_t)T * eps_stride, nullptr, h->wcls, b.z[T], b.V, N, h->L, h->Cd));
            const int r = decoder_forward(h, st, N, b.z[T], b.g);
            if (r) return r;
            HIPCHK(h, launch_final_out(st, b.g, pred, mask, mean, nullptr, B, h->K, h->P));
            if (traj) {
                PROF(h, st, "traj_out", launch_final_out(st, b.g, traj[0] + (size_t)T * B * 3 * P, traj[1] + (size_t)T * N * P,
                                                         traj[2] + (size_t)T * N * 3 * P, nullptr, B, h->K, h->P));
                HIPCHK(h, launch_img_terms_split(st, b.img_terms, traj[3], traj[4], T * B));
            }
            if (z) HIPCHK(h, hipMemcpyAsync(z, b.z[T], sizeof(float) * eps_stride, hipMemcpyDeviceToDevice, st));
        }
        if (post_mean) HIPCHK(h, hipMemcpyAsync(post_mean, b.pm, sizeof(float) * eps_stride, hipMemcpyDeviceToDevice, st));
        if (post_logvar) HIPCHK(h, hipMemcpyAsync(post_logvar, b.plv, sizeof(float) * eps_stride, hipMemcpyDeviceToDevice, st));
        if (elbo_iter && n_it > 0) HIPCHK(h, hipMemcpyAsync(elbo_iter, b.scal, sizeof(float) * 3 * n_it, hipMemcpyDeviceToDevice, st));
        return IODINE_OK;
    };
    std::vector<uintptr_t> key = graph_key(h, 1, B, {x, eps, pred, mask, mean, z, post_mean, post_logvar, elbo_iter}, nullptr, &pw);
    for (int j = 0; j < 4; ++j) key.push_back((uintptr_t)(state_in ? state_in[j] : nullptr));
    for (int j = 0; j < 5; ++j) key.push_back((uintptr_t)(traj ? traj[j] : nullptr));
    rc = run_graphed(h, st, key, body);
    if (rc) return rc;
    h->calls.last_elbo_iter = n_it > 0 ? n_it - 1 : -1;
    h->calls.last_elbo_batch = B;
    h->calls.state_iter = n_it;                                  // buf.h / buf.c [n_it]: the LSTM state after the last update (iodine_last_refine_state)
    // (host state, outside the graphed body) did this call leave the encoding in the workspace?  ref_conv_fwd: l0f && !keep_enc skips it
    h->calls.enc_valid = n_it > 0 && (h->stop_after >= 0 || !ref_form(h).l0f);
    return IODINE_OK;
}

int iodine_last_refine_state(iodine_handle* h, void* stream, int count, float* lstm_h, float* lstm_c)
{
    if (!h) return IODINE_ERR_INVALID;
    if (h->shim) return pad_last_refine_state(h, stream, count, lstm_h, lstm_c);
    if (int rc = last_refine_state_check(h, count)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const size_t n = sizeof(float) * (size_t)count * h->buf.K * h->H;   // the slots of the call that produced the state, not the run shape
    if (lstm_h) HIPCHK(h, hipMemcpyAsync(lstm_h, h->buf.h[h->calls.state_iter], n, hipMemcpyDeviceToDevice, st));
    if (lstm_c) HIPCHK(h, hipMemcpyAsync(lstm_c, h->buf.c[h->calls.state_iter], n, hipMemcpyDeviceToDevice, st));
    return IODINE_OK;
}

int iodine_last_train_state(iodine_handle* h, void* stream, int count, float* lstm_h, float* lstm_c)
{
    if (!h) return IODINE_ERR_INVALID;
    if (h->shim) return pad_last_refine_state(h, stream, count, lstm_h, lstm_c, true);
    if (int rc = last_train_state_check(h, count)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const size_t n = sizeof(float) * (size_t)count * h->buf.K * h->H;
    if (lstm_h) HIPCHK(h, hipMemcpyAsync(lstm_h, h->buf.h[h->calls.state_iter], n, hipMemcpyDeviceToDevice, st));
    if (lstm_c) HIPCHK(h, hipMemcpyAsync(lstm_c, h->buf.c[h->calls.state_iter], n, hipMemcpyDeviceToDevice, st));
    return IODINE_OK;
}

int iodine_decode(iodine_handle* h, void* stream, int batch, const float* z, float* pred, float* mask, float* mean)
{
    if (h && h->shim) return pad_decode(h, stream, batch, z, pred, mask, mean);
    int rc = decode_check(h, batch, z);
    if (rc) return rc;
    const bool save = h->save_bwd != 0;                    // option save_for_backward: keep what iodine_decode_backward reads (workspace mode 2)
    rc = ensure_workspace(h, batch, save ? 2 : 0);
    if (rc) return rc;
    h->calls.compute_begins(true);                         // (a decode touches neither buf.h / buf.c nor the posterior)
    hipStream_t st = (hipStream_t)stream;
    const int N = batch * h->K;
    auto body = [&]() -> int {
        Buffers& b = h->buf;
        // plain: into the (free) gradient buffer - buf.dec_out belongs to the last elbo() call; saved: buf.dec_out (buf.g is the backward's)
        // and z kept in buf.z[0].  The launches are the same.
        float* out = save ? b.dec_out : b.g;
        if (save) HIPCHK(h, hipMemcpyAsync(b.z[0], z, sizeof(float) * (size_t)N * h->L, hipMemcpyDeviceToDevice, st));
        HIPCHK(h, launch_dec_v(st, nullptr, nullptr, nullptr, z, h->wcls, nullptr, b.V, N, h->L, h->Cd));
        const int r = decoder_forward(h, st, N, z, out);
        if (r) return r;
        HIPCHK(h, launch_final_out(st, out, pred, mask, mean, nullptr, batch, h->K, h->P));
        return IODINE_OK;
    };
    if (save) h->calls.last_elbo_iter = -1;                      // buf.dec_out no longer belongs to an elbo() call
    rc = run_graphed(h, st, graph_key(h, save ? GK_DECODE_SAVED : GK_DECODE, batch, {z, pred, mask, mean}), body);
    if (rc) return rc;
    if (save) { h->calls.diff_kind = 1; h->calls.diff_batch = batch; }
    return IODINE_OK;
}

int iodine_scene_edit(iodine_handle* h, void* stream, int batch, const float* z, int n_edits, const int* image, const int* slot, const int* kind,
                      const float* z_new, int chunk_images, float* pred, float* mask, float* mean, float* base_pred, float* base_mask,
                      float* base_mean)
{
    if (h && h->shim)
        return pad_scene_edit(h, stream, batch, z, n_edits, image, slot, kind, z_new, chunk_images, pred, mask, mean, base_pred, base_mask, base_mean);
    int rc = scene_edit_check(h, batch, z, n_edits, image, slot, kind, z_new, chunk_images);
    if (rc) return rc;
    const int W = chunk_images > batch ? chunk_images : batch;
    rc = ensure_workspace(h, W, 0);
    if (rc) return rc;
    // an iodine_decode at batch W as far as the arena goes, except that the base takes buf.dec_out (the chunk decodes write buf.g): the
    // last elbo()'s outputs are gone, as after a saved decode.  Not captured under option graph: the launch sequence depends on the list
    h->calls.compute_begins(true);
    h->calls.last_elbo_iter = -1;
    hipStream_t st = (hipStream_t)stream;
    Buffers& b = h->buf;
    const int K = h->K, L = h->L;
    const size_t P = (size_t)h->P;
    HIPCHK(h, launch_dec_v(st, nullptr, nullptr, nullptr, z, h->wcls, nullptr, b.V, batch * K, L, h->Cd));
    if (int r = decoder_forward(h, st, batch * K, z, b.dec_out)) return r;
    if (base_pred || base_mask || base_mean) HIPCHK(h, launch_final_out(st, b.dec_out, base_pred, base_mask, base_mean, nullptr, batch, K, h->P));
    // chunks of consecutive edits with at most W * K replacements each (removals ride along: they need no decode)
    const int cap = W * K;
    SceneEditList list;
    for (int e0 = 0; e0 < n_edits;) {
        int e1 = e0, rows = 0;
        for (; e1 < n_edits && (kind[e1] == 1 || rows < cap); ++e1) rows += kind[e1] == 0;
        if (rows > 0) {
            // gather the chunk's z_new rows into buf.z[0] (rows of removals are not read): one copy per run of consecutive replacements
            for (int e = e0, r = 0; e < e1;) {
                if (kind[e] == 1) { ++e; continue; }
                int f = e;
                while (f < e1 && kind[f] == 0) ++f;
                HIPCHK(h, hipMemcpyAsync(b.z[0] + (size_t)r * L, z_new + (size_t)e * L, sizeof(float) * (size_t)(f - e) * L, hipMemcpyDeviceToDevice, st));
                r += f - e; e = f;
            }
            HIPCHK(h, launch_dec_v(st, nullptr, nullptr, nullptr, b.z[0], h->wcls, nullptr, b.V, rows, L, h->Cd));
            if (int r = decoder_forward(h, st, rows, b.z[0], b.g)) return r;
        }
        for (int f0 = e0, r = 0; f0 < e1; f0 += SCENE_EDIT_MAX) {
            list.n = std::min(SCENE_EDIT_MAX, e1 - f0);
            for (int j = 0; j < list.n; ++j) {
                list.bs[j] = image[f0 + j] * 16 + slot[f0 + j];
                list.src[j] = kind[f0 + j] == 0 ? r++ : -1;
            }
            PROF(h, st, "scene_edit", launch_scene_edit_out(st, b.dec_out, b.g, list, pred ? pred + (size_t)f0 * 3 * P : nullptr,
                                                           mask ? mask + (size_t)f0 * K * P : nullptr, mean ? mean + (size_t)f0 * 3 * P : nullptr, K, h->P));
        }
        e0 = e1;
    }
    return IODINE_OK;
}

int iodine_predictive(iodine_handle* h, void* stream, int batch, int n_samples, const float* post_mean, const float* post_logvar,
                      const float* eps, const float* x, int chunk_images, float* z, float* pred_mean, float* pred_m2, float* mask_mean,
                      float* mask_m2, int* votes, float* ll)
{
    if (h && h->shim)
        return pad_predictive(h, stream, batch, n_samples, post_mean, post_logvar, eps, x, chunk_images, z, pred_mean, pred_m2, mask_mean, mask_m2,
                              votes, ll);
    if (!h) return IODINE_ERR_INVALID;
    const PixelWeights pw(h);                              // one-shot, like every call that takes x: gone whether the call succeeds or not
    int rc = predictive_check(h, batch, n_samples, post_mean, post_logvar, eps, x, chunk_images, ll);
    if (rc) return rc;
    const int W = chunk_images > batch ? chunk_images : batch;
    rc = ensure_workspace(h, W, 0);
    if (rc) return rc;
    // an iodine_decode at batch W as far as the arena goes (the chunk decodes write buf.g), except that the samples take buf.z[0] and the
    // packed image buf.x4: the last elbo()'s outputs are gone, as after iodine_scene_edit.  Not captured under option graph: the launch
    // sequence depends on the sample count
    h->calls.compute_begins(true);
    h->calls.last_elbo_iter = -1;
    hipStream_t st = (hipStream_t)stream;
    Buffers& b = h->buf;
    const int B = batch, K = h->K, L = h->L, N = B * K;
    const size_t P = (size_t)h->P;
    // running state of an output the caller did not ask for: carved from the (free) refinement input, [W K][P][20] floats >= (3 K + 6) B P
    float* spare = b.enc[0];
    bool used_spare = false;
    auto state = [&](float* out, size_t n) { if (out) return out; float* q = spare; spare += n; used_spare = true; return q; };
    float* s_pm = state(pred_mean, (size_t)B * 3 * P);
    float* s_p2 = state(pred_m2, (size_t)B * 3 * P);
    float* s_mm = state(mask_mean, (size_t)N * P);
    float* s_m2 = state(mask_m2, (size_t)N * P);
    int* s_vt = votes ? votes : (int*)state(nullptr, (size_t)N * P);
    if (used_spare) h->calls.enc_valid = false;
    const bool like = x && ll;                             // (x without ll: nothing to score)
    if (like) HIPCHK(h, launch_x_to_nhwc4(st, x, b.x4, B, h->P, 1, pw.w, 0));
    const float *pm = post_mean ? post_mean : h->init_mean, *plv = post_mean ? post_logvar : h->init_logvar;
    const int per_chunk = W / B;                           // >= 1 whole samples per chunk
    for (int s0 = 0; s0 < n_samples; s0 += per_chunk) {
        const int n_s = std::min(per_chunk, n_samples - s0);
        float* zc = z ? z + (size_t)s0 * N * L : b.z[0];  // (buf.z[0] holds W K rows)
        HIPCHK(h, launch_predictive_sample(st, pm, plv, eps + (size_t)s0 * N * L, zc, n_s, N, L, post_mean ? L : 0));
        HIPCHK(h, launch_dec_v(st, nullptr, nullptr, nullptr, zc, h->wcls, nullptr, b.V, n_s * N, L, h->Cd));
        if (int r = decoder_forward(h, st, n_s * N, zc, b.g)) return r;
        PROF(h, st, "predictive", launch_predictive_accum(st, b.g, like ? b.x4 : nullptr, B, K, h->P, s0, n_s, s_pm, s_p2, s_mm, s_m2, s_vt, b.part,
                                                         like ? ll + (size_t)s0 * B : nullptr, (float)h->obj.sigma, h->precision == 0));
    }
    return IODINE_OK;
}

int iodine_elbo(iodine_handle* h, void* stream, int batch, const float* x, const float* post_mean, const float* post_logvar,
                const float* eps, float* terms)
{
    if (h && h->shim) return pad_elbo(h, stream, batch, x, post_mean, post_logvar, eps, terms);
    if (!h) return IODINE_ERR_INVALID;
    const PixelWeights pw(h);                              // (one image per batch entry: weights (B, P) either way)
    int rc = elbo_check(h, batch, x, eps, post_mean, post_logvar);
    if (rc) return rc;
    const bool save = h->save_bwd != 0;                    // option save_for_backward: keep what iodine_elbo_backward reads (workspace mode 2)
    rc = ensure_workspace(h, batch, save ? 2 : 0);
    if (rc) return rc;
    h->calls.compute_begins();                             // (the initial posterior below zeroes buf.h[0] / c[0])
    h->ig_call_wpf = 0;
    hipStream_t st = (hipStream_t)stream;
    const int B = batch, N = B * h->K;
    auto body = [&]() -> int {
        Buffers& b = h->buf;
        HIPCHK(h, launch_x_to_nhwc4(st, x, b.x4, B, h->P, 1, pw.w, 0));
        if (post_mean) {
            HIPCHK(h, hipMemcpyAsync(b.pm, post_mean, sizeof(float) * (size_t)N * h->L, hipMemcpyDeviceToDevice, st));
            HIPCHK(h, hipMemcpyAsync(b.plv, post_logvar, sizeof(float) * (size_t)N * h->L, hipMemcpyDeviceToDevice, st));
        } else {
            HIPCHK(h, launch_posterior_init(st, h->init_mean, h->init_logvar, b.pm, b.plv, b.h[0], b.c[0], N, h->L, h->H));
        }
        const int r = elbo_and_gradients(h, st, B, eps, 0, false, false, 0.f, save && h->sigma_grad, save ? h->input_grad : 0, 1.f / (float)B);
        if (r) return r;
        if (terms) HIPCHK(h, hipMemcpyAsync(terms, b.scal, sizeof(float) * 3, hipMemcpyDeviceToDevice, st));
        // kept for iodine_elbo_backward: z (buf.z[0]), the activations, dec_out, d(B * ELBO) / d dec_out (buf.g), the posterior (buf.pm / plv)
        // and the noise - the caller's tensor may be gone by then; buf.latent[0] has no other use in a single elbo
        if (save) HIPCHK(h, hipMemcpyAsync(b.latent[0], eps, sizeof(float) * (size_t)N * h->L, hipMemcpyDeviceToDevice, st));
        return IODINE_OK;
    };
    rc = run_graphed(h, st, graph_key(h, save ? GK_ELBO_SAVED : GK_ELBO, B, {x, post_mean, post_logvar, eps, terms}, nullptr, &pw), body);
    if (rc) return rc;
    CallState& cs = h->calls;
    cs.last_elbo_iter = 0;
    cs.last_elbo_batch = B;
    if (save) { cs.diff_kind = 2; cs.diff_batch = B; cs.diff_init = post_mean == nullptr; cs.diff_obj = h->obj; }
    cs.sgrad_n = save && h->sigma_grad ? 1 : 0;
    cs.ig_bits = save ? h->input_grad : 0; cs.ig_frames = 0; cs.ig_wpf = 0;
    return IODINE_OK;
}

namespace {

// caller's flat gradient buffer <- the accumulators.  Only the decoder and the initial posterior (the tail of the parameter table) can
// have received anything: when accumulating, the refinement network's gradients are not touched at all; otherwise they are written as 0
int diff_flat_out(iodine_handle* h, hipStream_t st, const float* scale_dev, float* flat, int accumulate)
{
    const size_t first = accumulate ? (size_t)(h->gacc[h->slot.dec_w[0]] - h->gacc_arena) : 0;
    HIPCHK(h, launch_axpy_dev(st, h->gacc_arena + first, 1.f, scale_dev, flat + first, (int)(h->gacc_total - first), accumulate));
    return IODINE_OK;
}

}  // namespace

int iodine_decode_backward(iodine_handle* h, void* stream, int batch, const float* g_pred, const float* g_mask, const float* g_mean,
                           float* dz, float* flat_grads, int accumulate)
{
    if (!h) return IODINE_ERR_INVALID;
    if (h->shim) return pad_decode_backward(h, stream, batch, g_pred, g_mask, g_mean, dz, flat_grads, accumulate);
    int rc = decode_backward_check(h, batch);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int B = batch, N = B * h->K;
    std::vector<uintptr_t> key = graph_key(h, GK_DECODE_BWD, B, {g_pred, g_mask, g_mean, dz, flat_grads});
    key.push_back((uintptr_t)accumulate);
    auto body = [&]() -> int {
        Buffers& b = h->buf;
        if (flat_grads) HIPCHK(h, launch_zero_fill(st, h->gacc_arena, h->gacc_total));
        PROF(h, st, "render_bwd", launch_render_bwd(st, b.dec_out, g_pred, g_mask, g_mean, b.g, B, h->K, h->P, h->precision == 0));
        float* dpre0 = nullptr;
        // ONE decoder pass with factor 1: data gradient down to the class sums of the broadcast layer, every decoder weight gradient on the way
        const int r = decoder_backward_data(h, st, N, &dpre0, flat_grads != nullptr, 1.f, 0, true);
        if (r) return r;
        if (dz)
            HIPCHK(h, launch_dz_plain(st, b.Rc, dec_path(h) == DEC_GENERIC ? h->gen_ident : h->wclsT, N, h->L, h->Cd, dz, nullptr, nullptr, nullptr,
                                      1.f, nullptr, nullptr, 1.f));
        return flat_grads ? diff_flat_out(h, st, nullptr, flat_grads, accumulate) : IODINE_OK;
    };
    rc = run_graphed(h, st, key, body);
    h->calls.saved_passes_gone();                          // consumed, like autograd without retain_graph (buf.g and the accumulators were overwritten)
    return rc;
}

int iodine_elbo_backward(iodine_handle* h, void* stream, const float* grad_out_dev, float* g_post_mean, float* g_post_logvar,
                         float* flat_grads, int accumulate)
{
    if (!h) return IODINE_ERR_INVALID;
    if (h->shim) return pad_elbo_backward(h, stream, grad_out_dev, g_post_mean, g_post_logvar, flat_grads, accumulate);
    int rc = diff_ready(h, 2, "iodine_elbo_backward");
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int B = h->calls.diff_batch, N = B * h->K;
    const Objective obj = h->calls.diff_obj;                     // the objective the saved elbo ran with (beta: the KL part of the posterior gradients)
    std::vector<uintptr_t> key = graph_key(h, GK_ELBO_BWD, B, {grad_out_dev, g_post_mean, g_post_logvar, flat_grads}, &obj);
    key.push_back((uintptr_t)accumulate);
    key.push_back((uintptr_t)h->calls.diff_init);
    auto body = [&]() -> int {
        Buffers& b = h->buf;
        const ParamSlots& ps = h->slot;
        if (flat_grads) HIPCHK(h, launch_zero_fill(st, h->gacc_arena, h->gacc_total));
        // buf.g = d(B * ELBO) / d dec_out from pixel_pass1: ONE decoder pass, weight gradients with the factor 1 / B of the batch mean
        float* dpre0 = nullptr;
        const int r = decoder_backward_data(h, st, N, &dpre0, flat_grads != nullptr, 1.f / (float)B, 0, true);
        if (r) return r;
        // d ELBO / d lambda (iodine.py:193,220: batch means) into the slots the refinement loop uses for them
        HIPCHK(h, launch_dz_plain(st, b.Rc, dec_path(h) == DEC_GENERIC ? h->gen_ident : h->wclsT, N, h->L, h->Cd, nullptr, b.pm, b.plv, b.latent[0],
                                  1.f / (float)B, b.g_pm[0], b.g_plv[0], (float)obj.beta));
        if (flat_grads && h->calls.diff_init) {                  // lambda = init_mean / init_logvar repeated over (B, K): iodine.py:615-616
            HIPCHK(h, launch_colsum(st, b.g_pm[0], N, h->L, h->L, 1.f, h->gacc[ps.init_mean]));
            HIPCHK(h, launch_colsum(st, b.g_plv[0], N, h->L, h->L, 1.f, h->gacc[ps.init_logvar]));
        }
        if (g_post_mean) HIPCHK(h, launch_axpy_dev(st, b.g_pm[0], 1.f, grad_out_dev, g_post_mean, N * h->L, 0));
        if (g_post_logvar) HIPCHK(h, launch_axpy_dev(st, b.g_plv[0], 1.f, grad_out_dev, g_post_logvar, N * h->L, 0));
        return flat_grads ? diff_flat_out(h, st, grad_out_dev, flat_grads, accumulate) : IODINE_OK;
    };
    rc = run_graphed(h, st, key, body);
    h->calls.saved_passes_gone();
    return rc;
}

int iodine_last_elbo_outputs(iodine_handle* h, void* stream, int count, float* z, float* mean, float* mask,
                             float* mask_logits, float* pred)
{
    if (!h) return IODINE_ERR_INVALID;
    if (h->shim) return pad_last_elbo_outputs(h, stream, count, z, mean, mask, mask_logits, pred);
    if (int rc = last_elbo_outputs_check(h, count)) return rc;
    const int K = h->buf.K;                                         // the slots of the call that produced the state, not the run shape
    hipStream_t st = (hipStream_t)stream;
    Buffers& b = h->buf;
    if (mean || mask || mask_logits || pred)
        HIPCHK(h, launch_final_out(st, b.dec_out, pred, mask, mean, mask_logits, count, K, h->P));
    if (z)
        HIPCHK(h, hipMemcpyAsync(z, b.z[h->calls.last_elbo_iter], sizeof(float) * (size_t)count * K * h->L,
                                 hipMemcpyDeviceToDevice, st));
    return IODINE_OK;
}

int iodine_last_posterior(iodine_handle* h, void* stream, int count, float* post_mean, float* post_logvar)
{
    if (!h) return IODINE_ERR_INVALID;
    if (h->shim) return pad_last_posterior(h, stream, count, post_mean, post_logvar);
    if (int rc = last_posterior_check(h, count)) return rc;
    const int K = h->buf.K;                                         // the slots of the call that produced the state, not the run shape
    hipStream_t st = (hipStream_t)stream;
    const size_t n = sizeof(float) * (size_t)count * K * h->L;
    if (post_mean) HIPCHK(h, hipMemcpyAsync(post_mean, h->buf.pm, n, hipMemcpyDeviceToDevice, st));
    if (post_logvar) HIPCHK(h, hipMemcpyAsync(post_logvar, h->buf.plv, n, hipMemcpyDeviceToDevice, st));
    return IODINE_OK;
}

int iodine_last_sigma_grad(iodine_handle* h, void* stream, float* out, int n)
{
    if (!h) return IODINE_ERR_INVALID;
    if (h->shim) return pad_last_sigma_grad(h, stream, out, n);
    if (h->calls.sgrad_n == 0 || h->buf.bytes == 0)
        return h->fail(IODINE_ERR_STATE, "iodine_last_sigma_grad: the last compute call left no d LL / d sigma - it needs option sigma_grad and an "
                                         "iodine_train_forward* or an iodine_elbo with option save_for_backward, with no compute call since");
    if (!out || n != h->calls.sgrad_n) {
        char m[200];
        snprintf(m, sizeof m, "iodine_last_sigma_grad: the last call left %d value(s) (one per ELBO evaluation); out must hold n = %d floats",
                 h->calls.sgrad_n, h->calls.sgrad_n);
        return h->fail(IODINE_ERR_INVALID, m);
    }
    HIPCHK(h, hipMemcpyAsync(out, h->buf.sgrad, sizeof(float) * (size_t)n, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return IODINE_OK;
}

int iodine_last_input_grad(iodine_handle* h, void* stream, float* g_x, float* g_w)
{
    if (!h) return IODINE_ERR_INVALID;
    if (h->shim) return pad_last_input_grad(h, stream, g_x, g_w);
    const CallState& cs = h->calls;
    if (cs.ig_bits == 0 || h->buf.bytes == 0)
        return h->fail(IODINE_ERR_STATE, "iodine_last_input_grad: the last compute call left no d LL / d x or d LL / d w - it needs option input_grad and an "
                                         "iodine_train_forward* or an iodine_elbo with option save_for_backward, with no compute call since");
    if ((g_x && !(cs.ig_bits & 1)) || (g_w && !(cs.ig_bits & 2)))
        return h->fail(IODINE_ERR_STATE, "iodine_last_input_grad: the last call ran without the bit of option input_grad that this output needs "
                                         "(1: g_x, the image; 2: g_w, the pixel weights)");
    hipStream_t st = (hipStream_t)stream;
    const size_t BP = (size_t)cs.last_elbo_batch * h->P, F = cs.ig_frames > 0 ? (size_t)cs.ig_frames : 1;
    if (g_x) HIPCHK(h, hipMemcpyAsync(g_x, h->buf.ig_x, sizeof(float) * 3 * BP * F, hipMemcpyDeviceToDevice, st));
    if (g_w) HIPCHK(h, hipMemcpyAsync(g_w, h->buf.ig_w, sizeof(float) * BP * (cs.ig_wpf ? F : 1), hipMemcpyDeviceToDevice, st));
    return IODINE_OK;
}

int iodine_last_likelihood(iodine_handle* h, void* stream, int count, float* log_likelihood, float* k_log_likelihood)
{
    if (!h) return IODINE_ERR_INVALID;
    if (h->shim) return pad_last_likelihood(h, stream, count, log_likelihood, k_log_likelihood);
    if (int rc = last_elbo_outputs_check(h, count)) return rc;
    const int K = h->buf.K;                                         // the slots of the call that produced the state, not the run shape
    const Buffers& b = h->buf;
    // the image that evaluation scored: frame last_elbo_iter of a clip (x4 is frame-major), else the one image
    const float* x4 = b.x4 + (b.F > 1 ? (size_t)h->calls.last_elbo_iter * b.B * h->P * 4 : 0);
    HIPCHK(h, launch_pixel_like_maps((hipStream_t)stream, x4, b.dec_out, log_likelihood, k_log_likelihood, count, K, h->P, (float)h->obj.sigma,
                                     h->precision == 0));
    return IODINE_OK;
}

int iodine_train_forward(iodine_handle* h, void* stream, int batch, const float* x, const float* eps, float* loss,
                         float* elbo_iter)
{
    return iodine_train_forward_seq(h, stream, batch, x, eps, nullptr, loss, elbo_iter);
}

int iodine_train_forward_seq(iodine_handle* h, void* stream, int batch, const float* x, const float* eps, const float* const* state_in,
                             float* loss, float* elbo_iter)
{
    return train_forward_impl(h, stream, batch, x, eps, state_in, loss, elbo_iter, nullptr);
}

int iodine_train_forward_frames(iodine_handle* h, void* stream, int batch, const float* x, const float* eps, const float* const* state_in,
                                float* loss, float* elbo_iter, const int* frame_idx, int n_frames, float* const* frames_out)
{
    if (!h) return IODINE_ERR_INVALID;
    if (n_frames == 0) return train_forward_impl(h, stream, batch, x, eps, state_in, loss, elbo_iter, nullptr);
    FrameSet fr; fr.idx = frame_idx; fr.n = n_frames; fr.out = frames_out;
    return train_forward_impl(h, stream, batch, x, eps, state_in, loss, elbo_iter, &fr);
}

}  // extern "C"

// fr == NULL: iodine_train_forward_seq, every launch as before; otherwise the listed evaluations are also written out
int train_forward_impl(iodine_handle* h, void* stream, int batch, const float* x, const float* eps, const float* const* state_in, float* loss,
                       float* elbo_iter, const FrameSet* fr)
{
    if (!h) return IODINE_ERR_INVALID;
    if (h->shim) return pad_train_forward(h, stream, batch, x, eps, state_in, loss, elbo_iter, fr);
    const PixelWeights pw(h);
    int rc = train_forward_check(h, batch, x, eps, loss, state_in, fr);
    if (rc) return rc;
    rc = ensure_workspace(h, batch, 1);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int B = batch, N = B * h->K, T = h->T, L = h->L;
    h->calls.compute_begins();
    h->ig_call_wpf = pw.per_frame && h->frames > 0;
    auto body = [&]() -> int {
        Buffers& b = h->buf;
        const size_t eps_stride = (size_t)N * L;
        HIPCHK(h, launch_zero_fill(st, h->gacc_arena, h->gacc_total));
        PROF(h, st, "frames_in", launch_x_to_nhwc4(st, x, b.x4, B, h->P, h->frames > 0 ? h->frames : 1, pw.w, pw.per_frame && h->frames > 0));
        if (state_in) {
            // continue from (lambda, h, c) of an earlier call (truncated / exact BPTT over a clip): evaluation 0 samples from the given lambda
            HIPCHK(h, hipMemcpyAsync(b.pm, state_in[0], sizeof(float) * eps_stride, hipMemcpyDeviceToDevice, st));
            HIPCHK(h, hipMemcpyAsync(b.plv, state_in[1], sizeof(float) * eps_stride, hipMemcpyDeviceToDevice, st));
            HIPCHK(h, hipMemcpyAsync(b.h[0], state_in[2], sizeof(float) * (size_t)N * h->H, hipMemcpyDeviceToDevice, st));
            HIPCHK(h, hipMemcpyAsync(b.c[0], state_in[3], sizeof(float) * (size_t)N * h->H, hipMemcpyDeviceToDevice, st));
        } else
            HIPCHK(h, launch_posterior_init(st, h->init_mean, h->init_logvar, b.pm, b.plv, b.h[0], b.c[0], N, L, h->H));
        int fj = 0;                                        // next entry of the list of chosen evaluations
        for (int i = 0; i <= T; ++i) {
            // d loss / d (B * ELBO_i) = -w_i / B; the default weighting keeps its closed form
            const float alpha = h->obj.whost ? -h->obj.whost[i] / (float)B : -((float)(i + 1) / (float)(T + 1)) / (float)B;
            int r = elbo_and_gradients(h, st, B, eps + (size_t)i * eps_stride, i, true, true, alpha, h->sigma_grad != 0, h->input_grad, -alpha);
            if (r) return r;
            if (fr && fj < fr->n && fr->idx[fj] == i) {
                // what this evaluation decoded and the lambda it sampled from (buf.pm / plv: the refinement step below moves them on);
                // its decoder backward above only read dec_out
                float* const* o = fr->out;
                const size_t NP = (size_t)N * h->P;
                if (o[1] || o[2] || o[3])
                    HIPCHK(h, launch_final_out(st, b.dec_out, nullptr, o[2] ? o[2] + fj * NP : nullptr, o[1] ? o[1] + fj * NP * 3 : nullptr,
                                               o[3] ? o[3] + fj * NP : nullptr, B, h->K, h->P));
                float* const dst[3] = {o[0], o[4], o[5]};
                const float* const src[3] = {b.z[i], b.pm, b.plv};
                for (int q = 0; q < 3; ++q)
                    if (dst[q]) HIPCHK(h, hipMemcpyAsync(dst[q] + fj * eps_stride, src[q], sizeof(float) * eps_stride, hipMemcpyDeviceToDevice, st));
                ++fj;
            }
            if (i == 0 && !state_in) {
                // lambda_0 = init_mean / init_logvar repeated over (B, K) (iodine.py:615-616): their gradient is the
                // column sum of d loss / d lambda_0; later lambdas are detached from it (iodine.py:642-643).  From a caller's state the two
                // parameters are not part of the graph: d loss / d lambda_0 goes to the state instead (iodine_train_backward_seq, g_state)
                HIPCHK(h, launch_colsum(st, b.g_pm[0], N, L, L, alpha, h->gacc[h->slot.init_mean]));
                HIPCHK(h, launch_colsum(st, b.g_plv[0], N, L, L, alpha, h->gacc[h->slot.init_logvar]));
            }
            if (i < T) {
                r = refine_step(h, st, B, i, true);
                if (r) return r;
            }
        }
        HIPCHK(h, launch_loss(st, b.scal, T + 1, loss, h->obj.wtab));
        if (elbo_iter) HIPCHK(h, hipMemcpyAsync(elbo_iter, b.scal, sizeof(float) * 3 * (T + 1), hipMemcpyDeviceToDevice, st));
        return IODINE_OK;
    };
    std::vector<uintptr_t> key = graph_key(h, 4, B, {x, eps, loss, elbo_iter}, nullptr, &pw);
    for (int j = 0; j < 4; ++j) key.push_back((uintptr_t)(state_in ? state_in[j] : nullptr));     // (all four NULL: no state)
    if (fr) {                                              // the list is baked into the captured launches like every address
        key.push_back((uintptr_t)fr->n);
        for (int j = 0; j < fr->n; ++j) key.push_back((uintptr_t)fr->idx[j]);
        for (int j = 0; j < 6; ++j) key.push_back((uintptr_t)fr->out[j]);
    }
    rc = run_graphed(h, st, key, body);
    if (rc) return rc;
    CallState& cs = h->calls;
    cs.fwd_done = true;
    cs.fwd_from_state = state_in != nullptr;
    cs.state_iter = T;                                     // buf.h / buf.c [T]: the LSTM state after the last update (iodine_last_train_state)
    cs.fwd_obj = h->obj;                                   // the backward differentiates the forward as it ran (a replay ran the same objective: graph key)
    cs.enc_valid = true;                                   // training keeps the encoding of every iteration (the backward reads it)
    cs.fwd_batch = B;
    cs.fwd_split = ref_form(h).split;      // layout of the saved refinement inputs (refine_split is part of the graph key)
    cs.last_elbo_iter = T;
    cs.last_elbo_batch = B;
    cs.sgrad_n = h->sigma_grad ? T + 1 : 0;
    cs.ig_bits = h->input_grad; cs.ig_frames = h->frames > 0 ? h->frames : 0; cs.ig_wpf = h->ig_call_wpf;
    return IODINE_OK;
}

// aux != NULL: the backward with auxiliary cotangents (iodine_train_backward_aux) - grad_scale / grad_scale_dev are then not used, aux->gl
// takes their place; aux == NULL: the plain backward, every launch as before
int train_backward_impl(iodine_handle* h, void* stream, float grad_scale, const float* grad_scale_dev, float* const* param_grads, int n,
                        int accumulate, const AuxCot* aux)
{
    if (!h) return IODINE_ERR_INVALID;
    if (h->shim) return pad_train_backward(h, stream, grad_scale, grad_scale_dev, param_grads, n, accumulate, aux);
    if (int rc = train_backward_check(h, param_grads, n, aux)) return rc;
    hipStream_t st = (hipStream_t)stream;
    std::vector<const void*> kp;
    for (int i = 0; i < n; ++i) kp.push_back(param_grads[i]);
    const Objective obj = h->calls.fwd_obj;                      // the objective of the saved forward, whatever the handle holds by now
    std::vector<uintptr_t> key = graph_key(h, 5, h->calls.fwd_batch, {}, &obj);
    for (const void* q : kp) key.push_back((uintptr_t)q);
    uint32_t gs_bits; memcpy(&gs_bits, &grad_scale, 4);
    key.push_back(gs_bits);
    key.push_back((uintptr_t)grad_scale_dev);
    key.push_back((uintptr_t)accumulate);
    key.push_back((uintptr_t)h->calls.fwd_split);                // the backward body reads the saved inputs in the forward's layout
    if (aux) {
        key.push_back(1);
        for (const void* q : {aux->gl, aux->mean, aux->mask, aux->logits, aux->z, aux->pm, aux->plv, aux->lstm_h, aux->lstm_c}) key.push_back((uintptr_t)q);
        for (int j = 0; j < 4; ++j) key.push_back((uintptr_t)(aux->g_state ? aux->g_state[j] : nullptr));
    }
    // iodine_train_backward_frames: cotangents on chosen evaluations (kinds in the order of FrameSet)
    const FrameSet* fr = aux && aux->frames && aux->frames->n > 0 ? aux->frames : nullptr;
    bool redecode = false;                                       // does an evaluation i < T take a decoder pass?
    if (fr) {
        key.push_back(2); key.push_back((uintptr_t)fr->n);
        for (int j = 0; j < fr->n; ++j) key.push_back((uintptr_t)fr->idx[j]);
        for (int j = 0; j < 6; ++j) key.push_back((uintptr_t)fr->g[j]);
        for (int j = 0; j < fr->n; ++j) redecode = redecode || (fr->idx[j] < h->T && (fr->g[1] || fr->g[2] || fr->g[3]));
    }
    auto body = [&]() -> int {
    Buffers& b = h->buf;
    const int B = h->calls.fwd_batch, N = B * h->K, T = h->T, L = h->L, H = h->H, Cr = h->Cr, IN = H + 4 * L;
    const ParamSlots& ps = h->slot;
    float *seed_m = nullptr, *seed_v = nullptr;
    size_t seed_stride = 0;
    const float *seed0_m = nullptr, *seed0_v = nullptr;           // seeds of evaluation 0: d / d lambda_0
    const size_t NL = (size_t)N * L, NP = (size_t)N * h->P;
    // cotangent of kind q on entry j of the list
    auto fg = [&](int q, int j, size_t per) -> const float* { return fr->g[q] ? fr->g[q] + (size_t)j * per : nullptr; };
    // iodine_train_backward_seq: cotangents on (h_T, c_T) start the carries of iteration T - 1, the carries left after iteration 0 are
    // d / d (h_0, c_0) of the state the forward started from
    const float *cot_h = aux ? aux->lstm_h : nullptr, *cot_c = aux ? aux->lstm_c : nullptr;
    float *gs_h = aux && aux->g_state ? aux->g_state[2] : nullptr, *gs_c = aux && aux->g_state ? aux->g_state[3] : nullptr;
    if (aux) {
        // Auxiliary cotangents on the final evaluation (iodine.py:171-187,642-651).  Order of the scaling: what the forward accumulated
        // carries the ELBO weights and takes d(out) / d(loss) now, in place (the refinement part is still 0); the auxiliary terms join with
        // factor 1; the ELBO seeds of the BPTT are multiplied on the device; the hand-over at the end runs with scale 1.
        HIPCHK(h, launch_scale_dev_add(st, h->gacc_arena, aux->gl, nullptr, (int)h->gacc_total));
        const bool dec = aux->mean || aux->mask || aux->logits;
        const float* const wl = dec_path(h) == DEC_GENERIC ? h->gen_ident : h->wclsT;
        if (fr) {
            // Cotangents on chosen evaluations.  Evaluation T (last in the list) first, on the kept activations like the final state's
            // cotangents above - and added to them where both are given: the rendering backward is linear in the cotangents, so the second
            // set is rendered into the (free) ping-pong buffer and added before the ONE decoder pass.
            const int jT = fr->idx[fr->n - 1] == T ? fr->n - 1 : -1;
            const float *t_mean = jT >= 0 ? fg(1, jT, NP * 3) : nullptr, *t_mask = jT >= 0 ? fg(2, jT, NP) : nullptr,
                        *t_logits = jT >= 0 ? fg(3, jT, NP) : nullptr;
            const bool decf = t_mean || t_mask || t_logits;
            if (dec)
                PROF(h, st, "render_bwd", launch_render_bwd_logits(st, b.dec_out, nullptr, aux->mask, aux->mean, aux->logits, b.g, B, h->K, h->P,
                                                                   h->precision == 0));
            if (decf)
                PROF(h, st, "render_bwd", launch_render_bwd_logits(st, b.dec_out, nullptr, t_mask, t_mean, t_logits, dec ? b.dpre[0] : b.g, B, h->K,
                                                                   h->P, h->precision == 0));
            if (dec && decf) HIPCHK(h, launch_axpy_dev(st, b.dpre[0], 1.f, nullptr, b.g, (int)(NP * 4), 1));
            float* dpre0 = nullptr;
            if (dec || decf)
                if (int r = decoder_backward_data(h, st, N, &dpre0, true, 1.f, T, true)) return r;
            // seeds of every evaluation: slice e of [T + 1][N][L]; slices 1 .. T are what the head's BPTT adds at iteration e - 1
            float *m_all = b.aux_seed, *v_all = b.aux_seed + (size_t)(T + 1) * NL;
            HIPCHK(h, launch_zero_fill(st, b.aux_seed, (size_t)2 * (T + 1) * NL));
            HIPCHK(h, launch_latent_seed(st, dec || decf ? b.Rc : nullptr, wl, N, L, h->Cd, aux->z, aux->pm, aux->plv, b.z[T], b.pm,
                                         m_all + (size_t)T * NL, v_all + (size_t)T * NL, L, jT >= 0 ? fg(0, jT, NL) : nullptr,
                                         jT >= 0 ? fg(4, jT, NL) : nullptr, jT >= 0 ? fg(5, jT, NL) : nullptr));
            // every other listed evaluation: decoded again from the saved z_i with the launches the forward ran (they overwrite V, the
            // activations, dec_out and g), rendering backward, ONE decoder pass with factor 1, seeds from (z_i, mu_i); mu_i is the first L
            // of every row of the saved refinement input latent[i], written from buf.pm before the head moved it on
            for (int j = 0; j < fr->n; ++j) {
                const int i = fr->idx[j];
                if (i == T) continue;
                const float *c_mean = fg(1, j, NP * 3), *c_mask = fg(2, j, NP), *c_logits = fg(3, j, NP), *c_z = fg(0, j, NL),
                            *c_pm = fg(4, j, NL), *c_plv = fg(5, j, NL);
                const bool deci = c_mean || c_mask || c_logits;
                if (!deci && !c_z && !c_pm && !c_plv) continue;
                if (deci) {
                    HIPCHK(h, launch_dec_v(st, nullptr, nullptr, nullptr, b.z[i], h->wcls, nullptr, b.V, N, L, h->Cd));
                    if (int r = decoder_forward(h, st, N, b.z[i])) return r;
                    PROF(h, st, "render_bwd", launch_render_bwd_logits(st, b.dec_out, nullptr, c_mask, c_mean, c_logits, b.g, B, h->K, h->P,
                                                                       h->precision == 0));
                    if (int r = decoder_backward_data(h, st, N, &dpre0, true, 1.f, i, true)) return r;
                }
                HIPCHK(h, launch_latent_seed(st, deci ? b.Rc : nullptr, wl, N, L, h->Cd, c_z, c_pm, c_plv, b.z[i], b.latent[i],
                                             m_all + (size_t)i * NL, v_all + (size_t)i * NL, 4 * L));
                if (i == 0) { seed0_m = m_all; seed0_v = v_all; }
            }
            seed_m = m_all + NL; seed_v = v_all + NL; seed_stride = NL;
            if (seed0_m && !h->calls.fwd_from_state) {
                // lambda_0 = init_mean / init_logvar repeated over (B, K): column sums, factor 1 (from a state: g_state, below)
                HIPCHK(h, launch_colsum(st, seed0_m, N, L, L, 1.f, h->gacc[ps.init_mean]));
                HIPCHK(h, launch_colsum(st, seed0_v, N, L, L, 1.f, h->gacc[ps.init_logvar]));
            }
        } else {
        if (dec) {
            // evaluation T's decoder activations and dec_out are still in the arena: the forward's last launches were that evaluation's own
            // decoder backward, which only reads them, and any compute call since would have cleared fwd_done.  ONE decoder pass with
            // factor 1: every decoder weight gradient, and the class sums of the broadcast layer for dz
            PROF(h, st, "render_bwd", launch_render_bwd_logits(st, b.dec_out, nullptr, aux->mask, aux->mean, aux->logits, b.g, B, h->K, h->P,
                                                               h->precision == 0));
            float* dpre0 = nullptr;
            if (int r = decoder_backward_data(h, st, N, &dpre0, true, 1.f, T, true)) return r;
        }
        seed_m = b.aux_seed; seed_v = b.aux_seed + (size_t)N * L;
        HIPCHK(h, launch_latent_seed(st, dec ? b.Rc : nullptr, wl, N, L, h->Cd, aux->z, aux->pm, aux->plv, b.z[T], b.pm, seed_m, seed_v));
        }
    }
    if (h->head_fused && head_bptt_fits(L, H, Cr)) {
        // the whole BPTT recurrence of the head in one launch (rows are independent: a block walks i = T-1 .. 0 for its rows)
        PROF(h, st, "head_bwd", launch_head_bptt(st, b.g_pm[0], b.g_plv[0], b.gates[0], b.c[0], b.u[0], h->raw_wm, h->raw_wv, h->raw_whh,
                                                 h->raw_wih, h->raw_mlp_w, b.ddm, b.ddv, b.dgates, b.ds, b.dpooled, T, N, B, L, H, Cr,
                                                 seed_m, seed_v, aux ? aux->gl : nullptr, obj.wtab, cot_h, cot_c, gs_h, gs_c,
                                                 seed_stride));
    } else {
        // the same recurrence as a launch sequence (9 launches per iteration)
        float* const ch[2] = {b.carry_h[0], b.carry_h[1]};
        float* const cc[2] = {b.carry_c[0], b.carry_c[1]};
        HIPCHK(h, launch_head_bptt_unfused(st, b.g_pm[0], b.g_plv[0], b.gates[0], b.c[0], b.u[0], h->raw_wm, h->raw_wv, h->raw_whh, h->raw_wih,
                                           h->raw_mlp_w, b.ddm, b.ddv, b.dgates, b.ds, b.dpooled, T, N, B, L, H, Cr, aux != nullptr, seed_m, seed_v,
                                           aux ? aux->gl : nullptr, obj.whost, cot_h, cot_c, gs_h, gs_c, seed_stride, b.dc1, b.dxin, ch, cc));
    }
    if (aux && aux->g_state) {
        // d loss / d lambda_0 of the state: d(out) / d(loss) x (-w_0 / B) x d(B ELBO_0) / d lambda_0 - the term the forward hands to init_mean /
        // init_logvar as a column sum when it starts from them.  Nothing else reaches lambda_0: lambda_1 = detach(lambda_0) + delta_0, and the
        // refinement inputs are detached (iodine.py:343,642-643)
        const float alpha0 = obj.whost ? -obj.whost[0] / (float)B : -(1.f / (float)(T + 1)) / (float)B;
        float* const dst[2] = {aux->g_state[0], aux->g_state[1]};
        const float* const src[2] = {b.g_pm[0], b.g_plv[0]};
        const float* const add0[2] = {seed0_m, seed0_v};         // cotangents on evaluation 0 (iodine_train_backward_frames), unscaled
        for (int j = 0; j < 2; ++j) {
            if (!dst[j]) continue;
            HIPCHK(h, launch_scale(st, src[j], alpha0, dst[j], N * L));
            HIPCHK(h, launch_scale_dev_add(st, dst[j], aux->gl, add0[j], N * L));
        }
    }
    {
        // Weight gradients of the head: sums over the iterations of X_i^T D_i = ONE GEMM per parameter over all T * N rows
        // (the per-iteration operands lie back to back: c[1..T], xin[0..T-1], h[0..T-1], pooled[0..T-1] and ddm / ddv / dgates / ds)
        const int R = T * N;
        HIPCHK(h, launch_sgemm(st, 1, 0, L, H, R, 1.f, b.ddm, L, b.c[1], H, 1.f, h->gacc[ps.wm], H));
        HIPCHK(h, launch_sgemm(st, 1, 0, L, H, R, 1.f, b.ddv, L, b.c[1], H, 1.f, h->gacc[ps.wv], H));
        HIPCHK(h, launch_colsum(st, b.ddm, R, L, L, 1.f, h->gacc[ps.bm]));
        HIPCHK(h, launch_colsum(st, b.ddv, R, L, L, 1.f, h->gacc[ps.bv]));
        HIPCHK(h, launch_sgemm(st, 1, 0, 4 * H, IN, R, 1.f, b.dgates, 4 * H, b.xin[0], IN, 1.f, h->gacc[ps.wih], IN));
        HIPCHK(h, launch_sgemm(st, 1, 0, 4 * H, H, R, 1.f, b.dgates, 4 * H, b.h[0], H, 1.f, h->gacc[ps.whh], H));
        HIPCHK(h, launch_colsum(st, b.dgates, R, 4 * H, 4 * H, 1.f, h->gacc[ps.bih]));
        HIPCHK(h, launch_colsum(st, b.dgates, R, 4 * H, 4 * H, 1.f, h->gacc[ps.bhh]));
        HIPCHK(h, launch_sgemm(st, 1, 0, H, Cr, R, 1.f, b.ds, H, b.pooled[0], Cr, 1.f, h->gacc[ps.mlp_w], Cr));
        HIPCHK(h, launch_colsum(st, b.ds, R, H, H, 1.f, h->gacc[ps.mlp_b]));
    }
    if (int r = refine_stack_backward(h, st, T * N, h->calls.fwd_split)) return r;
    bool flat = true;                                          // caller's gradients back to back in the same order?
    for (size_t p = 0; p < h->params.size() && flat; ++p)
        flat = param_grads[p] && param_grads[p] == param_grads[0] + (h->gacc[p] - h->gacc_arena);
    const float out_scale = aux ? 1.f : grad_scale;            // (aux: d(out) / d(loss) was applied above)
    const float* out_scale_dev = aux ? nullptr : grad_scale_dev;
    if (flat) {
        HIPCHK(h, launch_axpy_dev(st, h->gacc_arena, out_scale, out_scale_dev, param_grads[0], (int)h->gacc_total, accumulate));
        return IODINE_OK;
    }
    for (size_t p = 0; p < h->params.size(); ++p) {
        if (!param_grads[p]) continue;
        HIPCHK(h, launch_axpy_dev(st, h->gacc[p], out_scale, out_scale_dev, param_grads[p], (int)h->params[p].numel(), accumulate));
    }
    return IODINE_OK;
    };
    const int rc = run_graphed(h, st, key, body);
    // like autograd without retain_graph: the saved forward is consumed (a second backward would add the BPTT terms to the
    // accumulators twice); iodine_train_forward must run again first
    h->calls.saved_passes_gone();
    if (redecode) h->calls.redecoded = true;                   // buf.dec_out is no longer the final elbo()'s (iodine_last_elbo_outputs refuses)
    return rc;
}

// The entries that write one flat gradient buffer.  ``entry``: 0 iodine_train_backward_flat, 1 _aux, 2 _seq, 3 _frames - the arguments it
// does not have are NULL in ``aux``.  NULL / 0 arguments narrow a call frames -> seq -> aux -> flat, to the narrower entry itself, launch for
// launch: no chosen evaluation or no cotangent on any of them; nothing that crosses the ends of the saved forward; no auxiliary cotangent.
static int train_backward_flat(iodine_handle* h, void* stream, int entry, AuxCot aux, float* flat_grads, int accumulate)
{
    static const char* const who[4] = {"iodine_train_backward_flat", "iodine_train_backward_aux", "iodine_train_backward_seq", "iodine_train_backward_frames"};
    if (!h) return IODINE_ERR_INVALID;
    if (entry == 3) {
        const float* const* g = aux.frames->g;
        if (aux.frames->n == 0 || !(g[0] || g[1] || g[2] || g[3] || g[4] || g[5])) { entry = 2; aux.frames = nullptr; }
    }
    if (entry == 2 && !aux.lstm_h && !aux.lstm_c && !aux.g_state) entry = 1;
    if (entry == 1 && flat_grads && aux.gl && !aux.mean && !aux.mask && !aux.logits && !aux.z && !aux.pm && !aux.plv) entry = 0;
    if (!flat_grads) return h->fail(IODINE_ERR_INVALID, std::string(who[entry]) + ": flat_grads is required");
    std::vector<float*> ptrs(h->params.size());
    size_t off = 0;                                            // parameters back to back in named_parameters() order (= the gacc layout)
    for (size_t p = 0; p < h->params.size(); ++p) { ptrs[p] = flat_grads + off; off += h->params[p].numel(); }
    // (the loss cotangent: the plain backward scales its output by grad_scale_dev, with auxiliary cotangents it is aux.gl)
    return train_backward_impl(h, stream, 1.f, entry == 0 ? aux.gl : nullptr, ptrs.data(), (int)ptrs.size(), accumulate ? 1 : 0, entry == 0 ? nullptr : &aux);
}

extern "C" {

int iodine_train_backward(iodine_handle* h, void* stream, float grad_scale, float* const* param_grads, int n)
{
    return train_backward_impl(h, stream, grad_scale, nullptr, param_grads, n, 1);
}

int iodine_train_backward_flat(iodine_handle* h, void* stream, const float* grad_loss_dev, float* flat_grads, int accumulate)
{
    return train_backward_flat(h, stream, 0, AuxCot{grad_loss_dev}, flat_grads, accumulate);
}

int iodine_train_backward_aux(iodine_handle* h, void* stream, const float* grad_loss_dev, const float* g_mean, const float* g_mask,
                              const float* g_logits, const float* g_z, const float* g_post_mean, const float* g_post_logvar,
                              float* flat_grads, int accumulate)
{
    return train_backward_flat(h, stream, 1, AuxCot{grad_loss_dev, g_mean, g_mask, g_logits, g_z, g_post_mean, g_post_logvar}, flat_grads, accumulate);
}

int iodine_train_backward_seq(iodine_handle* h, void* stream, const float* grad_loss_dev, const float* g_mean, const float* g_mask,
                              const float* g_logits, const float* g_z, const float* g_post_mean, const float* g_post_logvar,
                              const float* g_lstm_h, const float* g_lstm_c, float* flat_grads, int accumulate, float* const* g_state)
{
    return train_backward_flat(h, stream, 2, AuxCot{grad_loss_dev, g_mean, g_mask, g_logits, g_z, g_post_mean, g_post_logvar, g_lstm_h, g_lstm_c, g_state},
                               flat_grads, accumulate);
}

int iodine_train_backward_frames(iodine_handle* h, void* stream, const float* grad_loss_dev, const float* g_mean, const float* g_mask,
                                 const float* g_logits, const float* g_z, const float* g_post_mean, const float* g_post_logvar,
                                 const float* g_lstm_h, const float* g_lstm_c, float* flat_grads, int accumulate, float* const* g_state,
                                 const int* frame_idx, int n_frames, const float* const* g_frames)
{
    if (!h) return IODINE_ERR_INVALID;
    iodine_handle* const shaped = h->shim ? pad_inner(h) : h;  // (the handle that holds the run shape)
    if (int rc = train_frames_check(shaped, "iodine_train_backward_frames", frame_idx, n_frames, g_frames)) {
        if (shaped != h) h->err = shaped->err;
        return rc;
    }
    FrameSet fr; fr.idx = frame_idx; fr.n = n_frames; fr.g = g_frames;
    return train_backward_flat(h, stream, 3, AuxCot{grad_loss_dev, g_mean, g_mask, g_logits, g_z, g_post_mean, g_post_logvar, g_lstm_h, g_lstm_c, g_state, &fr},
                               flat_grads, accumulate);
}

int iodine_logger_scalars(iodine_handle* h, void* stream, float* out2)
{
    if (!h || !out2) return IODINE_ERR_INVALID;
    if (h->shim) return pad_logger_scalars(h, stream, out2);
    if (!h->params_set) return h->fail(IODINE_ERR_STATE, "iodine_set_params has not been called");
    HIPCHK(h, launch_mean2((hipStream_t)stream, h->init_mean, h->init_logvar, h->Lreal > 0 ? h->Lreal : h->L, out2));
    return IODINE_OK;
}

int iodine_debug_copy(iodine_handle* h, void* stream, const char* name, int iter, float* dst, size_t max_floats,
                      size_t* n_floats)
{
    if (!h || !name) return IODINE_ERR_INVALID;
    if (h->shim) return pad_debug_copy(h, stream, name, iter, dst, max_floats, n_floats);
    if (h->buf.bytes == 0) return h->fail(IODINE_ERR_STATE, "iodine_debug_copy: no workspace yet");
    Buffers& b = h->buf;
    const size_t N = (size_t)b.B * b.K, P = h->P, L = h->L;        // the shape of the call that left the buffers, not the run shape
    if (iter < 0 || iter > b.T) return h->fail(IODINE_ERR_INVALID, "iodine_debug_copy: bad iteration index");
    const std::string s(name);
    const float* src = nullptr; size_t n = 0; bool join = false;      // join: enc in the split layout, back into the reference's 17 (+3 pad) channel order
    if (s == "z") { src = b.z[iter]; n = N * L; }
    else if (s == "dec_out") { src = b.dec_out; n = N * P * 4; }
    else if (s == "g") { src = b.g; n = N * P * 4; }
    else if (s == "enc") {
        n = N * P * 20;
        // with refine_l0_fused the inference loop never writes the encoding (kernels_refl0.hip keeps it on chip) unless stop_after_iters asks
        if (!h->calls.enc_valid)
            return h->fail(IODINE_ERR_STATE, "iodine_debug_copy: enc was not materialised by the last call (set stop_after_iters >= 0 or refine_l0_fused=0)");
        src = b.enc[iter]; join = ref_form(h).split;
    }
    else if (s == "latent") { src = b.latent[iter]; n = N * 4 * L; }
    else if (s == "g_pm") { src = b.g_pm[iter]; n = N * L; }
    else if (s == "g_plv") { src = b.g_plv[iter]; n = N * L; }
    else if (s == "lnstat") { src = b.lnstat; n = N * 8; }
    else if (s == "Rc") { src = b.Rc; n = N * 9 * h->Cd; }
    else if (s == "V") { src = b.V; n = N * 9 * h->Cd; }
    else if (s == "h") { src = b.h[iter + 1]; n = N * h->H; }
    else if (s == "c") { src = b.c[iter + 1]; n = N * h->H; }
    else if (s == "pm") { src = b.pm; n = N * L; }
    else if (s == "plv") { src = b.plv; n = N * L; }
    else if (s == "scal") { src = b.scal; n = (size_t)(b.T + 1) * 3; }
    else if (s == "img_terms") { src = b.img_terms; n = (size_t)(b.T + 1) * b.B * 2; }
    else if (s.rfind("act", 0) == 0) {
        const int l = atoi(s.c_str() + 3);
        if (l < 0 || l >= h->Dd) return h->fail(IODINE_ERR_INVALID, "bad decoder layer");
        src = b.act[l]; n = N * P * h->Cd;
    } else if (s.rfind("ract", 0) == 0) {
        const int l = atoi(s.c_str() + 4);
        if (l < 0 || l >= h->Dr) return h->fail(IODINE_ERR_INVALID, "bad refinement layer");
        int sz = h->S; for (int j = 0; j <= l; ++j) sz = ref_out_size(h, sz);
        src = b.ract[iter][l]; n = N * sz * sz * h->Cr;
    } else return h->fail(IODINE_ERR_INVALID, "iodine_debug_copy: unknown buffer " + s);
    if (n_floats) *n_floats = n;
    if (dst) {
        if (n > max_floats) return h->fail(IODINE_ERR_INVALID, "iodine_debug_copy: destination too small");
        if (join) HIPCHK(h, launch_enc_join((hipStream_t)stream, b.enck[iter], b.encs[iter], dst, (int)N, b.K, (int)P));
        else HIPCHK(h, hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    }
    return IODINE_OK;
}

int iodine_profile_read(iodine_handle* h, const char* category, double* total_ms, long long* launches, int reset)
{
    if (!h || !category) return IODINE_ERR_INVALID;
    if (h->shim) return pad_profile_read(h, category, total_ms, launches, reset);
    double tot = 0.0; long long cnt = 0;
    if (!strcmp(category, "graph_captures") || !strcmp(category, "graph_replays")) {    // hipGraph bookkeeping (option "graph")
        if (total_ms) *total_ms = 0.0;
        if (launches) *launches = category[6] == 'c' ? h->graph_captures : h->graph_replays;
        if (reset) { if (category[6] == 'c') h->graph_captures = 0; else h->graph_replays = 0; }
        return IODINE_OK;
    }
    if (!strncmp(category, "seen:", 5)) {               // launches of the category since the last reset, bracketed or not (profile_stride)
        for (auto& c : h->prof)
            if (c.name == category + 5) { cnt = (long long)c.seen_win; if (reset) c.seen_win = 0; }
        if (total_ms) *total_ms = 0.0;
        if (launches) *launches = cnt;
        return IODINE_OK;
    }
    for (auto& c : h->prof) {
        if (c.name != category) continue;
        for (size_t i = 0; i < c.used; ++i) {
            HIPCHK(h, hipEventSynchronize(c.ev[i].second));
            float ms = 0.f;
            HIPCHK(h, hipEventElapsedTime(&ms, c.ev[i].first, c.ev[i].second));
            tot += ms; ++cnt;
        }
        if (reset) c.used = 0;
    }
    if (total_ms) *total_ms = tot;
    if (launches) *launches = cnt;
    return IODINE_OK;
}

}  // extern "C"
