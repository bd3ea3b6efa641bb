// Which kernels run and in what order: the path selectors of the decoder and the refinement conv stack, their per-layer launchers and the
// launch sequences the entry points are made of (decoder forward / backward, one ELBO evaluation, one refinement step, the batched backward
// of the refinement stack).  Nothing but selectors and launches: a kernel change lands here.  Declarations: iodine_host.h.
#include "iodine_internal.h"

#ifdef IODINE_XSKIP_HOOK
int g_iod_xskip = 0;
#endif

// (DecPath, RefFamily and RefForm with their comments: iodine_host.h)
DecPath dec_path(const iodine_handle* h)
{
    if (h->generic) return DEC_GENERIC;
    const bool ws = h->opt.variant == 6 && h->S >= 16 && (h->S & (h->S - 1)) == 0;
    if (h->opt.precision != 0) return ws ? DEC_WS_F16 : DEC_TILE_F16;
    return ws && (h->Cd == 64 || h->Cd == 32) ? DEC_WS_F32 : DEC_TILE_F32;
}

bool dec_f16(DecPath p) { return p == DEC_WS_F16 || p == DEC_TILE_F16; }
// fp16 MFMAs per product on DEC_WS_F16: the split's three, or hi.hi alone (conv_precision 2, the only kernel that option changes)
int dec_ws_products(const iodine_handle* h) { return h->opt.precision == 2 ? 1 : 3; }

RefFamily ref_family(const iodine_handle* h)
{
    if (h->gen_ref) return REF_GENERIC;
    for (int l = 0, s = h->S; l < h->Dr; ++l, s /= 2) if (s % 2 != 0) return REF_GATHER;
    return h->opt.precision != 0 ? REF_S2_F16 : REF_S2_F32;
}
bool ref_s2(RefFamily f) { return f == REF_S2_F16 || f == REF_S2_F32; }
// Which optional packs exist at these shapes: iodine_set_params writes a pack where its predicate holds, a launch site reads it only behind it.
bool ref_pack_ws(const iodine_handle* h) { return h->Cr == 64; }                                               // ref.ws[1 ..]
bool ref_pack_bwd01(const iodine_handle* h) { return h->Dr >= 2 && refine_bwd01_ok(h->S, h->Cr); }             // ref.bwd01
bool ref_pack_l0f(const iodine_handle* h) { return h->ref.l0k.data != nullptr; }                               // ref.l0k / ref.l0s
RefForm ref_form(const iodine_handle* h)
{
    const RefFamily fam = ref_family(h);
    const bool split = h->opt.refine_split && ref_s2(fam);
    return {fam, split, split && fam == REF_S2_F16 && h->opt.refine_l0_fused && ref_pack_l0f(h) && refine_l0_fused_ok(h->S, h->Cr, h->K)};
}
// layer l (input size s) on the weight-stationary kernel?
bool ref_layer_ws(const iodine_handle* h, const RefForm& f, int l, int s) { return l > 0 && h->opt.refine_ws && ref_s2(f.fam) && ref_pack_ws(h) && conv3x3_s2ws_ok(s, h->Cr); }
// layer 1's data gradient + layer 0's weight gradient in one launch?  fwd_split: what the saved forward left (CallState), not the current option
bool ref_bwd01(const iodine_handle* h, bool fwd_split) { return h->opt.refine_bwd_fused && fwd_split && ref_family(h) == REF_S2_F16 && ref_pack_bwd01(h); }

namespace {

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
        PROF(h, st, "conv_tile_fwd", launch_conv3x3_ws_f16x3(st, b.act[l - 1], h->dec.ws_f[l].data, h->dec.ws_f[l].meta, h->dec.bias[l], nullptr, b.act[l],
                                                             b.tmax_act[l - 1], b.tmax_act[l], N, S, Cd, EPI_BIAS_ELU, l & 1, dec_ws_products(h)));
        break;
    case DEC_TILE_F16:
        PROF(h, st, "conv_tile_fwd", launch_conv3x3_tile_f16x3(st, b.act[l - 1], h->dec.tile_f[l].data, h->dec.tile_f[l].meta, h->dec.bias[l], nullptr, b.act[l],
                                                               N, S, Cd, Cd, EPI_BIAS_ELU, l & 1));
        break;
    case DEC_WS_F32:
        PROF(h, st, "conv_tile_fwd", launch_conv3x3_ws_f32(st, b.act[l - 1], h->dec.ws_f[l].data, h->dec.bias[l], nullptr, b.act[l], N, S, Cd, EPI_BIAS_ELU, l & 1));
        break;
    case DEC_TILE_F32:
        PROF(h, st, "conv_tile_fwd", launch_conv3x3_tile(st, b.act[l - 1], h->dec.tile32_f[l], h->dec.bias[l], nullptr, b.act[l], N, S, Cd, Cd, EPI_BIAS_ELU));
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
        PROF(h, st, "conv_tile_dgrad", launch_conv3x3_ws_f16x3(st, b.dpre[cur], h->dec.ws_b[l].data, h->dec.ws_b[l].meta, nullptr, b.act[l - 1], out,
                                                               b.tmax_dpre[cur], b.tmax_dpre[cur ^ 1], N, S, Cd, epi, l & 1, dec_ws_products(h)));
        break;
    case DEC_TILE_F16:
        PROF(h, st, "conv_tile_dgrad", launch_conv3x3_tile_f16x3(st, b.dpre[cur], h->dec.tile_b[l].data, h->dec.tile_b[l].meta, nullptr, b.act[l - 1], out,
                                                                 N, S, Cd, Cd, epi, l & 1));
        break;
    case DEC_WS_F32:
        PROF(h, st, "conv_tile_dgrad", launch_conv3x3_ws_f32(st, b.dpre[cur], h->dec.ws_b[l].data, nullptr, b.act[l - 1], out, N, S, Cd, epi, l & 1));
        break;
    case DEC_TILE_F32:                                     // (never asked for the row-sum epilogues: fused_l0 in decoder_backward_data)
        PROF(h, st, "conv_tile_dgrad", launch_conv3x3_tile(st, b.dpre[cur], h->dec.tile32_b[l], nullptr, b.act[l - 1], out, N, S, Cd, Cd, epi));
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
        PROF(h, st, "dec_out_dgrad", launch_dec_out_dgrad_f16x3(st, b.g, h->dec.out.dgrad.data, h->dec.out.dgrad.meta, b.act[h->Dd - 1], b.dpre[cur], N, h->S,
                                                                 h->Cd, path == DEC_WS_F16 ? b.tmax_dpre[cur] : nullptr));
    else
        PROF(h, st, "dec_out_dgrad", launch_conv3x3_tile(st, b.g, h->dec.out.dgrad32, nullptr, b.act[h->Dd - 1], b.dpre[cur], N, h->S, 4, h->Cd,
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

}  // namespace

// one decoder forward pass from z (already in buf.V via dec_v) -> dec_out
int decoder_forward(iodine_handle* h, hipStream_t st, int N, const float* z, float* out)
{
    Buffers& b = h->buf;
    if (!out) out = b.dec_out;
    const DecPath path = dec_path(h);
    if (path == DEC_GENERIC) {
        // fallback: the broadcast layer from the prefix table of its per-tap latent products (kernels_genl0.hip: the broadcast tensor is
        // never built), every other layer a generic fp32 conv (kernels_generic.hip)
        PROF(h, st, "gen_l0", launch_gen_l0_fwd(st, z, h->gen.wdec[0], h->gen.cterm, b.gen_l0, b.act[0], N, h->L, h->S, h->Cd, h->kd));
        const float* in = b.act[0];
        for (int l = 1; l < h->Dd; ++l) {
            if (h->gen.split_on)
                PROF(h, st, "gen_conv_f16x3", launch_gen_split_conv(st, in, h->gen.split_f[l].data, h->gen.split_f[l].meta, h->dec.bias[l], nullptr, b.act[l], N, h->S, h->Cd, h->kd, 1));
            else
                PROF(h, st, "gen_conv", launch_gen_conv_fwd(st, in, h->gen.wdec[l], h->dec.bias[l], b.act[l], N, h->S, h->Cd, h->Cd, h->Cd, h->kd, 1, 1));
            in = b.act[l];
        }
        PROF(h, st, "gen_conv", launch_gen_conv_fwd(st, in, h->gen.wout, h->dec.out.bias, out, N, h->S, h->Cd, h->Cd, 4, h->kd, 1, 0));
        return IODINE_OK;
    }
    const float* last = b.act[h->Dd - 1];
    const float* tmax = path == DEC_WS_F16 ? b.tmax_act[h->Dd - 1] : nullptr;
    PROF(h, st, "dec_l0", launch_dec_l0(st, b.V, h->dec.cmap, b.act[0], N, h->S, h->Cd, path == DEC_WS_F16 ? b.tmax_act[0] : nullptr));
    for (int l = 1; l < h->Dd; ++l)
        if (int rc = dec_conv_fwd(h, st, N, l)) return rc;
    if (path == DEC_WS_F16 && h->opt.dec_out_rows && dec_out_rows_ok(h->S, h->Cd, tmax))
        PROF(h, st, "dec_out", launch_dec_out_rows_f16x3(st, last, h->dec.out.gemm.data, h->dec.out.gemm.meta, h->dec.out.bias, out, N, h->S, h->Cd, tmax));
    else if (dec_f16(path))
        PROF(h, st, "dec_out", launch_dec_out_stream_f16x3(st, last, h->dec.out.gemm.data, h->dec.out.gemm.meta, h->dec.out.bias, out, N, h->S, h->Cd, tmax));
    else if (h->opt.dec_out_rows && dec_out_rows_ok(h->S, h->Cd, last) && h->dec.out.rows32)      // exact fp32 MFMA, row-streaming
        PROF(h, st, "dec_out", launch_dec_out_rows_f16x3(st, last, h->dec.out.rows32, nullptr, h->dec.out.bias, out, N, h->S, h->Cd, nullptr, 1));
    else
        PROF(h, st, "dec_out", launch_dec_out(st, last, h->dec.out.taps, h->dec.out.bias, out, N, h->S, h->Cd));
    return IODINE_OK;
}

namespace {

// gradient of B*ELBO wrt the decoder input z through the whole decoder (replaces the autograd traversal of
// (B*elbo).backward(), iodine.py:90,137).  Leaves d(pre-activation) of layer 0 in the returned buffer.
// With train the decoder weight gradients of this pass are accumulated on the way with the factor train_alpha
// (= -w_i / B): they are what the outer loss.backward() (train.py:63) would compute for this decoder pass.  The flag is separate from
// the factor: a pass with loss weight 0 (iter_weights 'last', an explicit 0) is still a training pass - it takes part in the first-pass
// overwrite of the maps accumulated over the passes (Dsum, Rsum, the kept partial tiles of wgrad_accum) and in the last pass's reduction /
// coordinate and bias gradients; only launches that purely ADD alpha x (this pass) to an accumulator are skipped for it.
// the same on the generic fallback path: plain chain of data gradients (and, in training, weight gradients with the pass factor);
// the broadcast layer's weight gradient and the gradient wrt z come from the tap-window sums of its pre-activation gradient
// (kernels_genl0.hip); dz is left in the first L entries of every row of buf.Rc (dz_latent multiplies that by the identity in h->gen.ident)
int decoder_backward_generic(iodine_handle* h, hipStream_t st, int N, float train_alpha, int it)   // it: only b.z[it], the decoded z
{
    // (every weight gradient here is an accumulation gacc += alpha x ..., without first / last bookkeeping: a zero-weight pass skips them)
    Buffers& b = h->buf;
    const ParamSlots& ps = h->slot;
    const int Cd = h->Cd, Dd = h->Dd, L = h->L, S = h->S, k = h->kd;
    int cur = 0;
    PROF(h, st, "gen_conv", launch_gen_conv_dgrad(st, b.g, h->gen.wout, b.act[Dd - 1], b.dpre[cur], N, S, Cd, Cd, 4, k, 1));
    if (train_alpha != 0.f)
        PROF(h, st, "gen_conv", launch_gen_conv_wgrad(st, b.act[Dd - 1], b.g, b.gen_scr, N, S, Cd, Cd, Cd, 4, k, 1, train_alpha,
                                                      h->gacc[ps.out_w], h->gacc[ps.out_b]));
    for (int l = Dd - 1; l > 0; --l) {
        float *gw = h->gacc[ps.dec_w[l]], *gb = h->gacc[ps.dec_b[l]];
        if (train_alpha != 0.f && h->gen.split_on && gen_split_wgrad_ok(k, Cd))
            PROF(h, st, "gen_conv_f16x3", launch_gen_split_wgrad(st, b.act[l - 1], b.dpre[cur], b.gen_scr, N, S, Cd, k, train_alpha, gw, gb));
        else if (train_alpha != 0.f)
            PROF(h, st, "gen_conv", launch_gen_conv_wgrad(st, b.act[l - 1], b.dpre[cur], b.gen_scr, N, S, Cd, Cd, Cd, Cd, k, 1, train_alpha, gw, gb));
        if (h->gen.split_on)
            PROF(h, st, "gen_conv_f16x3", launch_gen_split_conv(st, b.dpre[cur], h->gen.split_b[l].data, h->gen.split_b[l].meta, nullptr, b.act[l - 1], b.dpre[cur ^ 1], N, S, Cd, k, 0));
        else
            PROF(h, st, "gen_conv", launch_gen_conv_dgrad(st, b.dpre[cur], h->gen.wdec[l], b.act[l - 1], b.dpre[cur ^ 1], N, S, Cd, Cd, Cd, k, 1));
        cur ^= 1;
    }
    HIPCHK(h, launch_zero_fill(st, b.Rc, (size_t)N * 9 * Cd));
    PROF(h, st, "gen_l0", launch_gen_l0_bwd(st, b.dpre[cur], b.z[it], h->gen.wdec[0], h->lin, b.gen_l0, N, L, S, Cd, k, train_alpha,
                                            h->gacc[ps.dec_w[0]], h->gacc[ps.dec_b[0]], b.Rc, 9 * Cd));
    return IODINE_OK;
}

}  // namespace

// single: the pass is the only one of its backward (iodine_decode_backward / iodine_elbo_backward) - first (overwrite the maps accumulated
// over the passes) and last (emit the coordinate / bias gradients, reduce the kept partial tiles) at once; `it` then only names the z buffer
int decoder_backward_data(iodine_handle* h, hipStream_t st, int N, float** dpre0, bool train, float train_alpha, int it, bool single)
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
    const bool out_fused = train && dec_f16(path) && h->opt.out_bwd_fused;
    const bool acc_w = train && h->opt.wgrad_accum && !b.wg_acc.empty() && b.wg_acc[0];
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
        PROF(h, st, "dec_out_bwd", launch_dec_out_bwd_fused_f16x3(st, b.act[Dd - 1], b.g, h->dec.out.dgrad.data, h->dec.out.dgrad.meta, b.dpre[cur],
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
        fused_l0 = l == 1 && h->opt.fuse_l0 && (dec_f16(path) ? (!train || path == DEC_WS_F16) : path == DEC_WS_F32);
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
                       bool train, float train_alpha, bool sgrad, int igrad, float ig_coef)
{
    const float sigma = (float)h->obj.sigma, beta = (float)h->obj.beta;     // the handle's current objective (iodine_set_objective)
    Buffers& b = h->buf;
    const int N = B * h->K;
    HIPCHK(h, launch_dec_v(st, b.pm, b.plv, eps_i, nullptr, h->dec.wcls, b.z[i], b.V, N, h->L, h->Cd));
    int rc = decoder_forward(h, st, N, b.z[i]);
    if (rc) return rc;
    PROF(h, st, "pixel_pass1", launch_pixel_pass1(st, x4_frame(h, i), b.dec_out, b.g, b.part, B, h->K, h->P, sigma, h->opt.precision == 0, h->opt.joint_ll));
    // the ticket of pixel_finalize_elbo_kernel is reset by the last block of every launch; the first launch of an entry point also
    // starts from a fresh 0 (a memset node under graph capture), whatever a failed call or a misuse of the handle from a second
    // stream left in it - once per call, not per launch (a memset is a launch of its own)
    if (i == 0) HIPCHK(h, hipMemsetAsync(h->elbo_counter, 0, sizeof(unsigned), st));
    HIPCHK(h, launch_pixel_finalize_elbo(st, b.part, B, h->K, h->P, h->cfg.layernorm, b.lnstat, b.ll_img, b.pm, b.plv, h->L,
                                         b.img_terms + (size_t)i * B * 2, b.scal + 3 * i, h->elbo_counter, beta));
    if (sgrad)
        PROF(h, st, "pixel_sigma_grad", launch_pixel_sigma_grad(st, x4_frame(h, i), b.dec_out, b.sg_part, b.sgrad + i, B, h->K, h->P, h->obj.sigma,
                                                                h->opt.precision == 0, h->opt.joint_ll));
    if (igrad) {
        // igrad: the bits of option input_grad; buf.ig_x / ig_w += ig_coef x d (B LL_i) / d (x, w).  A still image (and a weight map shared
        // by the frames of a clip) is met by every evaluation: the first one writes, the others add, in evaluation order.  Frame i of a clip
        // (per-frame weights alike) is met by evaluation i alone, and is written in the caller's batch-first layout
        const size_t P = (size_t)h->P, F = train && h->frames > 0 ? (size_t)h->frames : 0;       // (a single elbo takes one image)
        const bool wpf = F && h->ig_call_wpf;
        PROF(h, st, "pixel_input_grad", launch_pixel_input_grad(st, x4_frame(h, i), b.dec_out, (igrad & 1) ? b.ig_x + (F ? i * 3 * P : 0) : nullptr,
                                                                F ? F * 3 * P : 3 * P, (igrad & 2) ? b.ig_w + (wpf ? i * P : 0) : nullptr,
                                                                wpf ? F * P : P, B, h->K, h->P, sigma, h->opt.precision == 0, ig_coef,
                                                                F || i == 0, wpf || i == 0, h->opt.joint_ll));
    }
    if (!need_grads) return IODINE_OK;
    float* dpre0 = nullptr;
    rc = decoder_backward_data(h, st, N, &dpre0, train, train_alpha, i);
    if (rc) return rc;
    HIPCHK(h, launch_dz_latent(st, b.Rc, dec_path(h) == DEC_GENERIC ? h->gen.ident : h->dec.wclsT, b.pm, b.plv, eps_i, N, h->L, h->Cd, h->cfg.layernorm,
                               b.g_pm[i], b.g_plv[i], b.latent[i], h->Lreal, beta));
    return IODINE_OK;
}

namespace {

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
        PROF(h, st, "refine_l0f", launch_refine_l0_fused(st, x4_frame(h, i), b.dec_out, b.lnstat, h->lin, h->ref.l0k.data, h->ref.l0k.meta, h->ref.l0s.data, h->ref.l0s.meta,
                                                         h->ref.bias[0], b.ract[i][0], keep_enc ? b.enck[i] : nullptr, keep_enc ? b.encs[i] : nullptr, B, h->K,
                                                         h->S, Cr, (float)h->obj.sigma, h->enc_chmask, h->opt.stable_enc, h->opt.joint_ll));
        return IODINE_OK;
    }
    if (l == 0)
        PROF(h, st, "pixel_pass2", launch_pixel_pass2(st, x4_frame(h, i), b.dec_out, b.lnstat, h->lin, f.split ? b.enck[i] : b.enc[i], B, h->K, h->S,
                                                      (float)h->obj.sigma, f.split ? b.encs[i] : nullptr, h->enc_chmask, h->opt.precision == 0, h->opt.stable_enc, h->opt.joint_ll));
    switch (f.fam) {
    case REF_GENERIC:
        PROF(h, st, "gen_conv", launch_gen_conv_fwd(st, in, h->gen.wref[l], h->ref.bias[l], b.ract[i][l], N, s, l == 0 ? 17 : Cr, cip, Cr, h->kr, h->rs, 1,
                                                    l == 0 ? h->enc_chmask : 0xffffffffu));
        break;
    case REF_S2_F16: case REF_S2_F32:
        if (l == 0 && f.split) {                           // the per-image channels once per image, then the per-slot ones on top
            PROF(h, st, cat, launch_conv3x3_s2_f16x3(st, b.encs[i], h->ref.split_sh.data, h->ref.split_sh.meta, nullptr, b.rmap, B, s, 8, Cr, nullptr, 0, f32));
            PROF(h, st, cat, launch_conv3x3_s2_f16x3(st, b.enck[i], h->ref.split_k.data, h->ref.split_k.meta, h->ref.bias[0], b.ract[i][0], N, s, 12, Cr, b.rmap, h->K, f32));
        } else if (ref_layer_ws(h, f, l, s))
            PROF(h, st, cat, launch_conv3x3_s2ws_f16x3(st, in, h->ref.ws[l].data, h->ref.ws[l].meta, h->ref.bias[l], b.ract[i][l], N, s, Cr, f32));
        else
            PROF(h, st, cat, launch_conv3x3_s2_f16x3(st, in, h->ref.s2_f[l].data, h->ref.s2_f[l].meta, h->ref.bias[l], b.ract[i][l], N, s, cip, Cr, nullptr, 0, f32));
        break;
    case REF_GATHER: PROF(h, st, cat, launch_conv3x3_gather(st, in, h->ref.gather_f[l], h->ref.bias[l], b.ract[i][l], N, s, s, cip, Cr, 2)); break;
    }
    return IODINE_OK;
}

// weight / bias gradient of layer l (input size s) over all NT slot-images into the accumulators.  split: the saved forward left layer 0's
// input in the split layout; fuse01: layer 1's data gradient rides in layer 0's launch (ref_bwd01)
int ref_conv_wgrad(iodine_handle* h, hipStream_t st, int NT, int l, int s, bool split, bool fuse01)
{
    Buffers& b = h->buf;
    const int Cr = h->Cr, cip = l == 0 ? 20 : Cr, ireal = l == 0 ? 17 : Cr, so = ref_out_size(h, s), f32 = h->opt.precision == 0;
    const float* in = l == 0 ? b.enc[0] : b.ract[0][l - 1];
    int nparts = 0, cipad = 0, nb = 0;
    float *gb = h->gacc[h->slot.ref_b[l]], *gw = h->gacc[h->slot.ref_w[l]];
    // the destination: the accumulator itself, or (first layer of an ARCH.ENCODING subset) a 17-channel scratch gathered into it afterwards
    const bool gather0 = l == 0 && h->n_in < 17;
    float* gw_dst = gather0 ? h->ref.g17 : gw;
    if (gather0) HIPCHK(h, launch_zero_fill(st, h->ref.g17, (size_t)Cr * 17 * h->kr * h->kr));
    switch (ref_family(h)) {
    case REF_GENERIC:
        PROF(h, st, "gen_conv", launch_gen_conv_wgrad(st, in, b.rdpre[l], b.gen_scr, NT, s, ireal, cip, ireal, Cr, h->kr, h->rs, 1.f, gw_dst, gb,
                                                      l == 0 ? h->enc_chmask : 0xffffffffu));
        break;
    case REF_S2_F16: case REF_S2_F32: {
        // split first layer: 12 per-slot + 8 per-image channels from two tensors, gradient in the internal channel order, then unsplit
        const bool split0 = l == 0 && split;
        if (split0 && fuse01)
            PROF(h, st, "refine_bwd01", launch_refine_bwd01(st, b.rdpre[1], h->ref.bwd01.data, h->ref.bwd01.meta, b.ract[0][0], b.enck[0], b.encs[0], b.wg_part,
                                                            b.wg_part_b, NT, s, Cr, h->K, &nparts, &cipad, &nb));
        else
            PROF(h, st, "refine_wgrad", launch_conv3x3_s2_wgrad_f16x3(st, split0 ? b.enck[0] : in, b.rdpre[l], b.wg_part, b.wg_part_b, NT, s, cip, Cr, &nparts,
                                                                      &cipad, &nb, split0 ? b.encs[0] : nullptr, split0 ? h->K : 0, f32));
        const int ir = split0 ? 20 : ireal;
        if (split0) HIPCHK(h, launch_zero_fill(st, h->ref.g20, (size_t)Cr * 20 * 9));
        HIPCHK(h, launch_wgrad_reduce(st, b.wg_part, nparts, cipad, Cr, Cr, ir, ir, 1.f, split0 ? h->ref.g20 : gw_dst, b.wg_fold, b.wg_part_b, nb, gb));
        if (split0) HIPCHK(h, launch_ref_unsplit_grad(st, h->ref.g20, Cr, gw_dst));
        break;
    }
    case REF_GATHER:
        PROF(h, st, "refine_wgrad", launch_conv3x3_wgrad_gather(st, in, b.rdpre[l], b.wg_part, NT, s, s, cip, Cr, 2, &nparts, &cipad));
        HIPCHK(h, launch_wgrad_reduce(st, b.wg_part, nparts, cipad, Cr, Cr, ireal, ireal, 1.f, gw_dst, b.wg_fold));
        PROF(h, st, "refine_bias_grad", launch_colsum_tall(st, b.rdpre[l], NT * so * so, Cr, 1.f, gb, b.wg_part_b, (size_t)512 * 64));
        break;
    }
    if (gather0) HIPCHK(h, launch_enc_gather_grad(st, h->ref.g17, Cr, h->n_in, h->enc_map, gw, h->kr * h->kr));
    return IODINE_OK;
}

// data gradient of layer l >= 1 (input size s): b.rdpre[l] -> b.rdpre[l - 1]
int ref_conv_dgrad(iodine_handle* h, hipStream_t st, int NT, int l, int s)
{
    Buffers& b = h->buf;
    float *d = b.rdpre[l], *out = b.rdpre[l - 1], *act = b.ract[0][l - 1];
    switch (ref_family(h)) {
    case REF_GENERIC: PROF(h, st, "gen_conv", launch_gen_conv_dgrad(st, d, h->gen.wref[l], act, out, NT, s, h->Cr, h->Cr, h->Cr, h->kr, h->rs)); break;
    case REF_S2_F16: case REF_S2_F32:
        PROF(h, st, "refine_dgrad", launch_conv3x3_s2_dgrad_f16x3(st, d, h->ref.s2_b[l].data, h->ref.s2_b[l].meta, act, out, NT, s, h->Cr, h->opt.precision == 0));
        break;
    case REF_GATHER: PROF(h, st, "refine_dgrad", launch_conv3x3_gather_dgrad(st, d, h->ref.gather_b[l], act, out, NT, s, s, h->Cr, 2)); break;
    }
    return IODINE_OK;
}

}  // namespace

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
        if (int r = ref_conv_fwd(h, st, f, i, l, s, B, save || h->opt.stop_after >= 0)) return r;
    PROF(h, st, "refine_head", launch_refine_head(st, b.ract[i][h->Dr - 1], N, s * s, h->Cr, h->H, h->L, h->head.mlp_wT, h->head.mlp_b, h->head.wihT, h->head.whhT, h->head.lstm_b,
                                 h->head.wmT, h->head.bm, h->head.wvT, h->head.bv, b.latent[i], b.h[i], b.c[i], b.h[i + 1], b.c[i + 1], b.pm, b.plv,
                                 save ? b.pooled[i] : nullptr, save ? b.u[i] : nullptr, save ? b.gates[i] : nullptr, save ? b.xin[i] : nullptr,
                                 nullptr, nullptr, b.head_xh, b.head_gp, h->opt.head_mfma));   // (the form: refine_head_form; head_mfma where both fit)
    return IODINE_OK;
}
