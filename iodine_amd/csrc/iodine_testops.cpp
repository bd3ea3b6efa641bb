// The kernel-test entry points of libiodine_hip.so (iodine_op_*), handle-free.  Kernel-level tests only: each allocates its scratch, runs
// the production launchers, synchronises and frees - not entry points to time.  Messages go where iodine_last_error(NULL) finds them
// (free_fail / free_hip, iodine_internal.h).  See include/iodine_hip.h.
#include "iodine_internal.h"

namespace {

// Device scratch of one entry: ONE hipMalloc cut into the regions asked for, each starting on 16 bytes (as in the library's workspace: the
// kernels read packs and tables with 16-byte loads), freed when the entry returns.  A failed allocation leaves the message.
class OpScratch {
    char* base_ = nullptr;
    std::vector<size_t> off_;
public:
    OpScratch(const char* who, std::initializer_list<size_t> region_bytes)
    {
        size_t total = 0;
        for (size_t b : region_bytes) { off_.push_back(total); total += (b + 15) & ~(size_t)15; }
        const hipError_t e = hipMalloc((void**)&base_, std::max<size_t>(total, 16));
        if (e != hipSuccess) { base_ = nullptr; free_fail(IODINE_ERR_HIP, std::string(who) + ": hipMalloc of " + std::to_string(total) + " bytes of scratch: " + hipGetErrorString(e)); }
    }
    ~OpScratch() { if (base_) (void)hipFree(base_); }
    OpScratch(const OpScratch&) = delete;
    OpScratch& operator=(const OpScratch&) = delete;
    bool ok() const { return base_ != nullptr; }
    template <typename T = float> T* at(int region) const { return reinterpret_cast<T*>(base_ + off_[region]); }
    Pack pack(int region) const { return Pack{at<char>(region), at(region + 1)}; }     // a pack and, on the next region, its meta block
};

// the end of every entry: wait for the launches, leave the message of the first error
int op_done(const char* who, hipStream_t st, hipError_t e) { return free_hip(who, e == hipSuccess ? hipStreamSynchronize(st) : e); }

constexpr size_t META_BYTES = 64;                       // the meta block of a pack, on a region of its own

}  // namespace

extern "C" {

int iodine_op_conv3x3(void* stream, int mode, const float* in, const float* w, const float* bias, const float* aux,
                      float* out, int n, int ih, int iw, int w_o, int w_i, int cin_pad, int cout, int stride, int epi,
                      int tflip)
{
    hipStream_t st = (hipStream_t)stream;
    const bool square_cc = cin_pad == cout && w_o == cout && w_i == cout && ih == iw;      // what the weight-stationary kernels take
    switch (mode) {
    case IODINE_CONV_S2_FWD: case IODINE_CONV_S2_DGRAD: case IODINE_CONV_S2_FWD_F32: case IODINE_CONV_S2_DGRAD_F32: {   // stride-2 tile kernels; ih = fine size
        const bool fwd = mode == IODINE_CONV_S2_FWD || mode == IODINE_CONV_S2_FWD_F32;
        const int f32 = mode == IODINE_CONV_S2_FWD_F32 || mode == IODINE_CONV_S2_DGRAD_F32;
        const int cp = fwd ? (cin_pad == 20 ? 32 : (cin_pad == 12 || cin_pad == 8 ? 16 : cin_pad)) : cin_pad;   // floats per pixel -> packed chunks
        OpScratch scr("iodine_op_conv3x3(s2 f16x3)", {wpk_s2_tile_bytes(cp, cout), META_BYTES});
        if (!scr.ok()) return IODINE_ERR_HIP;
        const Pack p = scr.pack(0);
        hipError_t e = f32 ? launch_pack_conv_weights_s2f32(st, w, w_o, w_i, cp, cout, fwd ? 0 : 2, p.data)
                           : launch_pack_conv_weights_f16(st, w, w_o, w_i, cp, cout, fwd ? 0 : 2, p.meta, p.data);
        if (e == hipSuccess)
            e = fwd ? launch_conv3x3_s2_f16x3(st, in, p.data, p.meta, bias, out, n, ih, cin_pad, cout, nullptr, 0, f32)
                    : launch_conv3x3_s2_dgrad_f16x3(st, in, p.data, p.meta, aux, out, n, ih, cout, f32);
        return op_done("iodine_op_conv3x3(s2 f16x3)", st, e);
    }
    case IODINE_CONV_WS: case IODINE_CONV_WS_B: case IODINE_CONV_WS_1P: {   // weight-stationary split-fp16 kernel (per-cell max side buffer from launch_cell_max)
        if (!square_cc || ih % 16 != 0) return free_fail(IODINE_ERR_INVALID, "iodine_op_conv3x3(ws): shape");
        const size_t tf = conv_ws_tmax_floats(n, ih);
        OpScratch scr("iodine_op_conv3x3(ws)", {wpk_ws_bytes(cout), META_BYTES, tf * sizeof(float), tf * sizeof(float)});
        if (!scr.ok()) return IODINE_ERR_HIP;
        const Pack p = scr.pack(0);
        float *tin = scr.at(2), *tout = scr.at(3);
        hipError_t e = launch_pack_conv_weights_ws(st, w, cout, tflip, p.meta, p.data);
        if (e == hipSuccess) e = launch_cell_max(st, in, tin, n, ih, cout);
        if (e == hipSuccess) e = launch_conv3x3_ws_f16x3(st, in, p.data, p.meta, bias, aux, out, tin, tout, n, ih, cout, epi, 0, mode == IODINE_CONV_WS_1P ? 1 : 3);
        return op_done("iodine_op_conv3x3(ws)", st, e);
    }
    case IODINE_CONV_S2WS: case IODINE_CONV_S2WS_F32: {   // weight-stationary STRIDE-2 conv c -> c + bias + ELU (kernels_refws.hip); ih = fine size
        if (!square_cc || !conv3x3_s2ws_ok(ih, cout)) return free_fail(IODINE_ERR_INVALID, "iodine_op_conv3x3(s2ws): shape");
        const bool f32 = mode == IODINE_CONV_S2WS_F32;
        OpScratch scr("iodine_op_conv3x3(s2ws)", {wpk_ws_bytes(cout), META_BYTES});
        if (!scr.ok()) return IODINE_ERR_HIP;
        const Pack p = scr.pack(0);
        hipError_t e = f32 ? launch_pack_conv_weights_ws32(st, w, cout, 0, p.data) : launch_pack_conv_weights_ws(st, w, cout, 0, p.meta, p.data);
        if (e == hipSuccess) e = launch_conv3x3_s2ws_f16x3(st, in, p.data, p.meta, bias, out, n, ih, cout, f32);
        return op_done("iodine_op_conv3x3(s2ws)", st, e);
    }
    case IODINE_CONV_WS_F32: {      // exact-fp32 form of the weight-stationary kernel (v_mfma_f32_16x16x4_f32)
        if (!square_cc || ih % 16 != 0) return free_fail(IODINE_ERR_INVALID, "iodine_op_conv3x3(ws f32): shape");
        OpScratch scr("iodine_op_conv3x3(ws f32)", {wpk_ws_bytes(cout)});
        if (!scr.ok()) return IODINE_ERR_HIP;
        hipError_t e = launch_pack_conv_weights_ws32(st, w, cout, tflip, scr.at<char>(0));
        if (e == hipSuccess) e = launch_conv3x3_ws_f32(st, in, scr.at<char>(0), bias, aux, out, n, ih, cout, epi, 0);
        return op_done("iodine_op_conv3x3(ws f32)", st, e);
    }
#ifdef IODINE_WITH_WINO
    case IODINE_CONV_WINO: {        // Winograd F(2x2, 3x3) split-fp16 kernel (C = 64): experiment libraries only (tools/wino_variants.sh)
        if (!square_cc || ih % 16 != 0) return free_fail(IODINE_ERR_INVALID, "iodine_op_conv3x3(wino): shape");
        const size_t tf = conv_ws_tmax_floats(n, ih);
        OpScratch scr("iodine_op_conv3x3(wino)", {conv_wino_wpk_bytes(cout), META_BYTES, tf * sizeof(float), tf * sizeof(float), conv_wino_scratch_floats(cout) * sizeof(float)});
        if (!scr.ok()) return IODINE_ERR_HIP;
        const Pack p = scr.pack(0);
        float *tin = scr.at(2), *tout = scr.at(3);
        hipError_t e = launch_pack_conv_weights_wino(st, w, cout, tflip, p.meta, p.data, scr.at(4));
        if (e == hipSuccess) e = launch_cell_max(st, in, tin, n, ih, cout);
        if (e == hipSuccess) e = launch_conv3x3_wino_f16x3(st, in, p.data, p.meta, bias, aux, out, tin, tout, n, ih, cout, epi, 0);
        return op_done("iodine_op_conv3x3(wino)", st, e);
    }
#endif
    case IODINE_CONV_TILE_F16: {    // split-fp16 LDS-tiled kernel
        OpScratch scr("iodine_op_conv3x3(f16x3)", {wpk_tile_f16_bytes(cin_pad, cout), META_BYTES});
        if (!scr.ok()) return IODINE_ERR_HIP;
        const Pack p = scr.pack(0);
        hipError_t e = launch_pack_conv_weights_f16(st, w, w_o, w_i, cin_pad, cout, tflip, p.meta, p.data);
        if (e == hipSuccess) e = launch_conv3x3_tile_f16x3(st, in, p.data, p.meta, bias, aux, out, n, ih, cin_pad, cout, epi, 0);
        return op_done("iodine_op_conv3x3(f16x3)", st, e);
    }
    default: break;
    }
    // the fp32 LDS-tile pack: IODINE_CONV_TILE_F32 on the stride-1 tile kernel, every other mode on the gather kernel
    OpScratch scr("iodine_op_conv3x3", {wpk_tile_f32_bytes(cin_pad, cout)});
    if (!scr.ok()) return IODINE_ERR_HIP;
    float* wpk = scr.at(0);
    hipError_t e = launch_pack_conv_weights(st, w, w_o, w_i, cin_pad, cout, tflip, wpk);
    if (e == hipSuccess && mode == IODINE_CONV_TILE_F32)
        e = (ih == iw && stride == 1) ? launch_conv3x3_tile(st, in, wpk, bias, aux, out, n, ih, cin_pad, cout, epi) : hipErrorInvalidValue;
    else if (e == hipSuccess)
        e = launch_conv3x3_gather(st, in, wpk, bias, out, n, ih, iw, cin_pad, cout, stride);
    return op_done("iodine_op_conv3x3", st, e);
}

int iodine_op_dec_out(void* stream, const float* in, const float* w, const float* bias, float* out, int n, int s, int c)
{
    hipStream_t st = (hipStream_t)stream;
    OpScratch scr("iodine_op_dec_out", {wpk_out_taps_bytes(c)});
    if (!scr.ok()) return IODINE_ERR_HIP;
    hipError_t e = launch_pack_dec_out(st, w, scr.at(0), c);
    if (e == hipSuccess) e = launch_dec_out(st, in, scr.at(0), bias, out, n, s, c);
    return op_done("iodine_op_dec_out", st, e);
}

int iodine_op_dec_out_f16x3(void* stream, const float* in, const float* w, const float* bias, float* out, int n, int s, int c, int variant)
{
    hipStream_t st = (hipStream_t)stream;
    if (s % 16 != 0 || (c != 64 && c != 32)) return free_fail(IODINE_ERR_INVALID, "iodine_op_dec_out_f16x3: shape");
    // IODINE_DEC_OUT_ROWS_F32 puts its rows32 operand where the GEMM-form pack was (pack_geom.h asserts that it fits at c = 32 / 64)
    OpScratch scr("iodine_op_dec_out_f16x3", {std::max(wpk_out_gemm_bytes(c), wpk_out_rows32_bytes(c)), META_BYTES, conv_ws_tmax_floats(n, s) * sizeof(float)});
    if (!scr.ok()) return IODINE_ERR_HIP;
    const Pack p = scr.pack(0);
    float* tin = scr.at(2);
    hipError_t e = launch_pack_dec_out_gemm(st, w, c, p.meta, p.data);
    if (e == hipSuccess) e = launch_cell_max(st, in, tin, n, s, c);
    if (e == hipSuccess && variant == IODINE_DEC_OUT_ROWS_F32) {          // exact-fp32 row-streaming form: its own weight operand
        e = launch_pack_dec_out_rows32(st, w, c, (float*)p.data);
        if (e == hipSuccess) e = launch_dec_out_rows_f16x3(st, in, p.data, nullptr, bias, out, n, s, c, nullptr, 1);
    } else if (e == hipSuccess)
        e = variant == IODINE_DEC_OUT_ROWS ? launch_dec_out_rows_f16x3(st, in, p.data, p.meta, bias, out, n, s, c, tin)
                                           : launch_dec_out_stream_f16x3(st, in, p.data, p.meta, bias, out, n, s, c, variant == IODINE_DEC_OUT_TILES_NOMAX ? nullptr : tin);
    return op_done("iodine_op_dec_out_f16x3", st, e);
}

int iodine_op_conv3x3_wgrad(void* stream, const float* in, const float* d, float* gw, float* gb, int n, int s, int ci_pad,
                            int ci_real, int co, int stride)
{
    hipStream_t st = (hipStream_t)stream;
    const int cmax = std::max(std::max(ci_pad, co), 32);
    // partial tiles, their fold stage and the partial bias rows, sized as the library's workspace sizes them
    OpScratch scr("iodine_op_conv3x3_wgrad", {sizeof(float) * 512 * 4 * 9 * cmax * cmax, sizeof(float) * WGRAD_FOLD * 9 * cmax * cmax, sizeof(float) * 512 * 64});
    if (!scr.ok()) return IODINE_ERR_HIP;
    float *part = scr.at(0), *fold = scr.at(1), *part_b = scr.at(2);
    int nparts = 0, cip = 0, nb = 0;
    hipError_t e;
    if (stride == 1 && co == 4) {
        e = launch_dec_out_wgrad_gemm_f16x3(st, in, d, part, part_b, n, s, ci_pad, &nparts, &nb);
        if (e == hipSuccess) e = launch_wgrad_reduce(st, part, nparts, ci_pad, 4, 4, ci_real, ci_real, 1.f, gw, fold);
    } else if (stride == 1) {
        e = launch_conv3x3_wgrad_f16x3_ws(st, in, d, part, part_b, n, s, ci_pad, co, &nparts, &cip, &nb);
        // stride-1 partial tiles are [9][ci][co padded to 32]
        if (e == hipSuccess) e = launch_wgrad_reduce(st, part, nparts, ci_pad, cip, co, ci_real, ci_real, 1.f, gw, fold);
    } else {                                           // stride 2; IODINE_WGRAD_STRIDE2_F32: the exact-fp32 form of the same kernel
        e = launch_conv3x3_s2_wgrad_f16x3(st, in, d, part, part_b, n, s, ci_pad, co, &nparts, &cip, &nb, nullptr, 0, stride == IODINE_WGRAD_STRIDE2_F32);
        if (e == hipSuccess) e = launch_wgrad_reduce(st, part, nparts, cip, co, co, ci_real, ci_real, 1.f, gw, fold);
    }
    if (e == hipSuccess) e = launch_colsum(st, part_b, nb, co, co, 1.f, gb);
    return op_done("iodine_op_conv3x3_wgrad", st, e);
}

int iodine_op_gen_conv(void* stream, int mode, const float* in, const float* w, const float* bias, const float* aux, float* out, float* gb,
                       int n, int si, int ci, int ldc, int co, int k, int s, int elu)
{
    hipStream_t st = (hipStream_t)stream;
    if (mode < IODINE_GEN_FWD || mode > IODINE_GEN_WGRAD || s < 1 || s > 8 || (k != 3 && k != 5 && k != 7) || ldc < ci) return free_fail(IODINE_ERR_INVALID, "iodine_op_gen_conv: argument");
    // tests only: elu bit 8 set = bits 9.. carry a per-channel mask of the input channels that can be non-zero (what the library hands
    // the stride-2 kernels for an ARCH.ENCODING subset: all-zero 4- / 16-channel groups are skipped) - the masked form must equal the plain one
    const unsigned chmask = (elu & 0x100) ? ((unsigned)elu >> 9) : 0xffffffffu;
    elu &= 1;
    // weights [tap][ci][co]: the forward pack has ci rows, the data-gradient pack ldc rows (the packed input-channel count is din's stride)
    OpScratch scr("iodine_op_gen_conv", {wpk_gen_bytes(k, ldc, co), mode == IODINE_GEN_WGRAD ? gen_wgrad_scratch_floats(ci, co, k) * sizeof(float) : 0});
    if (!scr.ok()) return IODINE_ERR_HIP;
    float* wt = scr.at(0);
    hipError_t e = hipSuccess;
    if (mode == IODINE_GEN_FWD) {
        e = launch_gen_pack_weights(st, w, co, ci, k, wt);
        if (e == hipSuccess) e = launch_gen_conv_fwd(st, in, wt, bias, out, n, si, ci, ldc, co, k, s, elu, chmask);
    } else if (mode == IODINE_GEN_DGRAD) {
        e = launch_gen_pack_weights(st, w, co, ldc, k, wt);     // (w has ldc input channels here: ci of them are computed)
        if (e == hipSuccess) e = launch_gen_conv_dgrad(st, in, wt, aux, out, n, si, ci, ldc, co, k, s);
    } else {
        e = launch_gen_conv_wgrad(st, in, aux, scr.at(1), n, si, ci, ldc, ci, co, k, s, 1.f, out, gb, chmask);
    }
    return op_done("iodine_op_gen_conv", st, e);
}

int iodine_op_gen_conv_tier(int mode, int si, int ci, int ldc, int co, int k, int s)
{
    // (host arithmetic only: runs without a GPU)
    if (mode < IODINE_GEN_FWD || mode > IODINE_GEN_WGRAD || si < 1 || ci < 1 || co < 1 || s < 1 || s > 8 || (k != 3 && k != 5 && k != 7) || ldc < ci) return -1;
    const GenTierSel sel = gen_conv_tier(mode, si, ci, ldc, co, k, s);
    return (int)sel.tier | (sel.np << 8) | (sel.seg << 16);
}

int iodine_op_gen_l0(void* stream, int mode, const float* z, const float* w, const float* bias, const float* dpre, float* out, float* gw,
                     float* gb, float* dz, int n, int L, int s, int co, int k, int ld, float alpha)
{
    hipStream_t st = (hipStream_t)stream;
    if (mode < IODINE_GEN_FWD || mode > IODINE_GEN_DGRAD || n < 1 || L < 1 || s < 1 || co < 1 || k < 1 || k > GEN_L0_KMAX || k % 2 == 0 || !z || !w
        || (mode == IODINE_GEN_FWD && (!bias || !out)) || (mode == IODINE_GEN_DGRAD && (!dpre || !dz || ld < L || (alpha != 0.f && (!gw || !gb)))))
        return free_fail(IODINE_ERR_INVALID, "iodine_op_gen_l0: argument");
    // (the forward reads cterm and the prefix table with 16-byte loads)
    OpScratch scr("iodine_op_gen_l0", {wpk_gen_bytes(k, L + 2, co), (size_t)s * sizeof(float), mode == IODINE_GEN_FWD ? (size_t)s * s * co * sizeof(float) : 0,
                                       gen_l0_scratch_floats(n, s, co, k) * sizeof(float)});
    if (!scr.ok()) return IODINE_ERR_HIP;
    float *wt = scr.at(0), *lin = scr.at(1), *cterm = scr.at(2), *tmp = scr.at(3);
    std::vector<float> hlin((size_t)s);
    iodine_linspace_host(s, hlin.data());
    hipError_t e = hipMemcpyAsync(lin, hlin.data(), (size_t)s * sizeof(float), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);         // (hlin is pageable host memory)
    if (e == hipSuccess) e = launch_gen_pack_weights(st, w, co, L + 2, k, wt);
    if (e == hipSuccess && mode == IODINE_GEN_FWD) {
        e = launch_gen_l0_coord(st, wt, bias, lin, L, s, co, k, cterm);
        if (e == hipSuccess) e = launch_gen_l0_fwd(st, z, wt, cterm, tmp, out, n, L, s, co, k);
    } else if (e == hipSuccess) {
        e = launch_gen_l0_bwd(st, dpre, z, wt, lin, tmp, n, L, s, co, k, alpha, gw, gb, dz, ld);
    }
    return op_done("iodine_op_gen_l0", st, e);
}

int iodine_op_gen_conv_f16x3(void* stream, int mode, const float* in, const float* w, const float* bias, const float* aux, float* out, float* gb,
                             int n, int si, int ci, int ldc, int co, int k, int s, int elu)
{
    hipStream_t st = (hipStream_t)stream;
    if (mode < IODINE_GEN_FWD || mode > IODINE_GEN_WGRAD || n < 1 || si < 1) return free_fail(IODINE_ERR_INVALID, "iodine_op_gen_conv_f16x3: argument");
    if (s != 1 || ci != co || ldc != ci || !gen_split_cch(k, ci))
        return free_fail(IODINE_ERR_INVALID, "iodine_op_gen_conv_f16x3: shape not covered by the split kernels (stride 1, ci = co = ldc a multiple of 16, k in {3, 5, 7}, slice fits LDS)");
    if (mode == IODINE_GEN_WGRAD) {
        if (!gen_split_wgrad_ok(k, ci) || !aux || !out || !gb)
            return free_fail(IODINE_ERR_INVALID, "iodine_op_gen_conv_f16x3: mode 2 needs aux (gradient), out (gw), gb and a shape the split weight gradient covers");
        OpScratch scr("iodine_op_gen_conv_f16x3", {gen_wgrad_scratch_floats(ci, co, k) * sizeof(float)});
        if (!scr.ok()) return IODINE_ERR_HIP;
        return op_done("iodine_op_gen_conv_f16x3", st, launch_gen_split_wgrad(st, in, aux, scr.at(0), n, si, ci, k, 1.f, out, gb));
    }
    OpScratch scr("iodine_op_gen_conv_f16x3", {wpk_gen_bytes(k, ci, co), wpk_gen_split_meta_floats(ci) * sizeof(float), gen_split_pack_bytes(k, ci)});
    if (!scr.ok()) return IODINE_ERR_HIP;
    float *wt = scr.at(0), *meta = scr.at(1);
    void* pk = scr.at<char>(2);
    hipError_t e = launch_gen_pack_weights(st, w, co, ci, k, wt);
    if (e == hipSuccess) e = launch_gen_split_pack(st, wt, k, ci, mode, pk, meta);
    if (e == hipSuccess)
        e = launch_gen_split_conv(st, in, pk, meta, mode == IODINE_GEN_FWD ? bias : nullptr, mode == IODINE_GEN_DGRAD ? aux : nullptr, out, n, si, ci, k,
                                  mode == IODINE_GEN_FWD ? (elu & 1) : 0);
    return op_done("iodine_op_gen_conv_f16x3", st, e);
}

int iodine_op_render_bwd(void* stream, const float* dec_out, const float* g_pred, const float* g_mask, const float* g_mean, float* g_out,
                         int batch, int slots, int pixels, int strict)
{
    hipStream_t st = (hipStream_t)stream;
    if (!dec_out || !g_out || batch < 1 || slots < 1 || slots > 16 || pixels < 1) return free_fail(IODINE_ERR_INVALID, "iodine_op_render_bwd: argument");
    return op_done("iodine_op_render_bwd", st, launch_render_bwd(st, dec_out, g_pred, g_mask, g_mean, g_out, batch, slots, pixels, strict ? 1 : 0));
}

int iodine_op_render_bwd_logits(void* stream, const float* dec_out, const float* g_pred, const float* g_mask, const float* g_mean,
                                const float* g_logits, float* g_out, int batch, int slots, int pixels, int strict)
{
    hipStream_t st = (hipStream_t)stream;
    if (!dec_out || !g_out || batch < 1 || slots < 1 || slots > 16 || pixels < 1) return free_fail(IODINE_ERR_INVALID, "iodine_op_render_bwd_logits: argument");
    return op_done("iodine_op_render_bwd_logits", st,
                   launch_render_bwd_logits(st, dec_out, g_pred, g_mask, g_mean, g_logits, g_out, batch, slots, pixels, strict ? 1 : 0));
}

int iodine_op_pixel_maps(void* stream, const float* x_nchw, const float* w_or_null, const float* dec_out_nhwc4, int batch, int slots,
                         int pixels, float sigma, int strict, float coef, float* ll, float* kll, float* gx, float* gw, int first)
{
    hipStream_t st = (hipStream_t)stream;
    if (!x_nchw || !dec_out_nhwc4 || batch < 1 || slots < 1 || slots > 16 || pixels < 1 || !(sigma > 0.f) ||
        (size_t)batch * slots * pixels >= ((size_t)1 << 31))
        return free_fail(IODINE_ERR_INVALID, "iodine_op_pixel_maps: argument");
    OpScratch scr("iodine_op_pixel_maps", {(size_t)batch * pixels * 4 * sizeof(float)});
    if (!scr.ok()) return IODINE_ERR_HIP;
    float* x4 = scr.at(0);
    hipError_t e = launch_x_to_nhwc4(st, x_nchw, x4, batch, pixels, 1, w_or_null, 0);
    const int st_ = strict & 1, joint = (strict >> 1) & 1;                 // the flag word: bit 0 strict, bit 1 joint_likelihood
    if (e == hipSuccess) e = launch_pixel_like_maps(st, x4, dec_out_nhwc4, ll, kll, batch, slots, pixels, sigma, st_, joint);
    if (e == hipSuccess)
        e = launch_pixel_input_grad(st, x4, dec_out_nhwc4, gx, (size_t)3 * pixels, gw, (size_t)pixels, batch, slots, pixels, sigma, st_,
                                    coef, first ? 1 : 0, first ? 1 : 0, joint);
    return op_done("iodine_op_pixel_maps", st, e);
}

// the per-pixel mixture kernels of one ELBO evaluation, kernel-level (tests/test_gpu_pixel.py): the production launchers in the order
// elbo_and_gradients / refine_step / iodine_reconstruct run them
int iodine_op_pixel_encode(void* stream, const float* x_nchw, const float* w_or_null, const float* dec_out_nhwc4, const float* pm, const float* plv,
                           const float* lin, int batch, int slots, int size, int latent, float sigma, float beta, int flags, unsigned chmask,
                           int repeat, float* const* out)
{
    hipStream_t st = (hipStream_t)stream;
    const size_t B = (size_t)(batch > 0 ? batch : 0), K = (size_t)(slots > 0 ? slots : 0), S = (size_t)(size > 0 ? size : 0), P = S * S;
    bool ok = x_nchw && dec_out_nhwc4 && pm && plv && lin && out && batch >= 1 && slots >= 1 && slots <= 16 && size >= 1 && size <= 46340 &&
              latent >= 1 && sigma > 0.f && repeat >= 1 && B * K * P * 20 < ((size_t)1 << 31) && B * K * (size_t)latent < ((size_t)1 << 31);
    for (int j = 0; ok && j < 5; ++j) ok = out[j] != nullptr;              // (g, lnstat, ll_img, img_terms, scal: pass 1 and the finalize write them all)
    if (ok && out[7] && !out[6]) ok = false;                               // (enc_sh belongs to the split form of enc)
    if (!ok)
        return free_fail(IODINE_ERR_INVALID, "iodine_op_pixel_encode: argument (x, dec_out, pm, plv, lin and out[0..4] required; batch, size, latent, repeat >= 1; slots "
                          "in 1..16; sigma > 0; enc_sh only with enc; batch * slots * size^2 * 20 and batch * slots * latent below 2^31)");
    float *g = out[0], *lnstat = out[1], *ll_img = out[2], *img_terms = out[3], *scal = out[4], *sgrad = out[5], *enc = out[6], *enc_sh = out[7];
    const int Pi = (int)P, strict = flags & 1, use_ln = (flags >> 1) & 1, stable = (flags >> 2) & 1, joint = (flags >> 3) & 1;
    const size_t nblk = (size_t)pixel_blocks_per_image(Pi);
    // [x4: B P float4][part: B nblk (6 K + 3) doubles][sg_part: B nblk doubles][counter: one word]
    OpScratch scr("iodine_op_pixel_encode", {B * P * 4 * sizeof(float), B * nblk * (6 * K + 3) * sizeof(double), B * nblk * sizeof(double), 16});
    if (!scr.ok()) return IODINE_ERR_HIP;
    float* x4 = scr.at(0);
    double *part = scr.at<double>(1), *sg_part = scr.at<double>(2);
    unsigned* counter = scr.at<unsigned>(3);
    hipError_t e = hipMemsetAsync(counter, 0, 16, st);
    if (e == hipSuccess) e = launch_x_to_nhwc4(st, x_nchw, x4, batch, Pi, 1, w_or_null, 0);
    for (int r = 0; e == hipSuccess && r < repeat; ++r) {                  // (repeat > 1: the finalize finds the counter its last launch left)
        // ... and scal as NaN: a launch whose ticket elects no last block would otherwise leave the previous launch's (equal) values
        if (r > 0 && (e = hipMemsetAsync(scal, 0xff, 3 * sizeof(float), st)) != hipSuccess) break;
        e = launch_pixel_pass1(st, x4, dec_out_nhwc4, g, part, batch, slots, Pi, sigma, strict, joint);
        if (e == hipSuccess)
            e = launch_pixel_finalize_elbo(st, part, batch, slots, Pi, use_ln, lnstat, ll_img, pm, plv, latent, img_terms, scal, counter, beta);
    }
    if (e == hipSuccess && sgrad) e = launch_pixel_sigma_grad(st, x4, dec_out_nhwc4, sg_part, sgrad, batch, slots, Pi, (double)sigma, strict, joint);
    if (e == hipSuccess && enc) e = launch_pixel_pass2(st, x4, dec_out_nhwc4, lnstat, lin, enc, batch, slots, size, sigma, enc_sh, chmask, strict, stable, joint);
    if (e == hipSuccess) e = launch_final_out(st, dec_out_nhwc4, out[8], out[9], out[10], out[11], batch, slots, Pi);
    return op_done("iodine_op_pixel_encode", st, e);
}

int iodine_op_conv3x3_wgrad_f32(void* stream, const float* in, const float* d, float* gw, float* gb, int n, int s, int c)
{
    hipStream_t st = (hipStream_t)stream;
    OpScratch scr("iodine_op_conv3x3_wgrad_f32", {sizeof(float) * 512 * 4 * 9 * 32 * 32, sizeof(float) * WGRAD_FOLD * 9 * 64 * 64, sizeof(float) * 512 * 64});
    if (!scr.ok()) return IODINE_ERR_HIP;
    float *part = scr.at(0), *fold = scr.at(1), *part_b = scr.at(2);
    const bool out_conv = c < 0;                    // the output conv |c| -> 4 in GEMM form (d has 4 channels; gw [4][|c|][3][3], gb [4])
    const int ci = out_conv ? -c : c, co = out_conv ? 4 : c;
    int nparts = 0, cop = 4, nb = 0;
    hipError_t e = out_conv ? launch_dec_out_wgrad_f32(st, in, d, part, part_b, n, s, ci, &nparts, &nb)
                            : launch_conv3x3_wgrad_f32_ws(st, in, d, part, part_b, n, s, ci, &nparts, &cop, &nb);
    if (e == hipSuccess) e = launch_wgrad_reduce(st, part, nparts, ci, cop, co, ci, ci, 1.f, gw, fold);
    if (e == hipSuccess) e = launch_colsum(st, part_b, nb, co, co, 1.f, gb);
    return op_done("iodine_op_conv3x3_wgrad_f32", st, e);
}

// ---- the refinement head and its backward, kernel-level (tests/test_gpu_head.py, tests/test_gpu_sgemm.py) --------------------------------

int iodine_op_sgemm(void* stream, int form, int ta, int tb, int M, int N, int K, float alpha, const float* A, int lda, const float* B, int ldb,
                    float beta, float* Cm, int ldc, int mode_c)
{
    hipStream_t st = (hipStream_t)stream;
    if (form < IODINE_SGEMM_DISPATCH || form > IODINE_SGEMM_MFMA_L0MAP || M < 1 || N < 1 || K < 1 || !A || !B || !Cm || lda < 1 || ldb < 1 || ldc < 1)
        return free_fail(IODINE_ERR_INVALID, "iodine_op_sgemm: argument");
    if (form == IODINE_SGEMM_DISPATCH) {
        if (lda < (ta ? M : K) || ldb < (tb ? K : N) || ldc < N) return free_fail(IODINE_ERR_INVALID, "iodine_op_sgemm: leading dimension");
        return op_done("iodine_op_sgemm", st, launch_sgemm(st, ta, tb, M, N, K, alpha, A, lda, B, ldb, beta, Cm, ldc));
    }
    // A [K][M] (IODINE_SGEMM_MFMA_ROWMAJOR: [M][K] row-major), B [K][N]; IODINE_SGEMM_MFMA_L0MAP writes through the broadcast layer's map:
    // N = 9 mode_c, ldc = L + 2 >= M
    const bool rowmajor = form == IODINE_SGEMM_MFMA_ROWMAJOR, l0map = form == IODINE_SGEMM_MFMA_L0MAP;
    if (!sgemm_tn_mfma_ok(M, N, K) || lda < (rowmajor ? K : M) || ldb < N || (l0map ? (mode_c < 1 || N != 9 * mode_c || ldc < M) : ldc < N))
        return free_fail(IODINE_ERR_INVALID, "iodine_op_sgemm: shape not covered by the MFMA form (M, N multiples of 32; form 3: N = 9 mode_c, ldc >= M)");
    return op_done("iodine_op_sgemm", st, launch_sgemm_tn_mfma(st, M, N, K, alpha, A, lda, B, ldb, beta, Cm, ldc, l0map ? 1 : 0, l0map ? mode_c : 0, rowmajor ? 1 : 0));
}

int iodine_op_colsum(void* stream, int form, const float* src, int rows, int cols, int ld, float alpha, float* dst)
{
    hipStream_t st = (hipStream_t)stream;
    if (form < IODINE_COLSUM_BLOCK || form > IODINE_COLSUM_TALL || !src || !dst || rows < 1 || cols < 1 || ld < cols) return free_fail(IODINE_ERR_INVALID, "iodine_op_colsum: argument");
    if (form == IODINE_COLSUM_BLOCK) return op_done("iodine_op_colsum", st, launch_colsum(st, src, rows, cols, ld, alpha, dst));
    // the streaming form, only where launch_colsum_tall itself takes it (elsewhere it forwards to launch_colsum = the block form)
    if (ld != cols || cols % 4 != 0 || cols > 256 || 256 % (cols / 4) != 0 || rows < 8192)
        return free_fail(IODINE_ERR_INVALID, "iodine_op_colsum: the tall form takes contiguous rows >= 8192, cols a multiple of 4 with 256 % (cols / 4) == 0");
    const size_t tmp_elems = (size_t)512 * 64;                           // (the library's partial-bias scratch)
    OpScratch scr("iodine_op_colsum", {tmp_elems * sizeof(float)});
    if (!scr.ok()) return IODINE_ERR_HIP;
    return op_done("iodine_op_colsum", st, launch_colsum_tall(st, src, rows, cols, alpha, dst, scr.at(0), tmp_elems));
}

int iodine_op_refine_head(void* stream, int form, const float* const* in, float* const* out, int N, int PL, int C, int H, int L)
{
    hipStream_t st = (hipStream_t)stream;
    const bool split = form == IODINE_HEAD_THREE_LAUNCHES;
    bool ok = in && out && (form == IODINE_HEAD_ONE_LAUNCH || split) && N >= 1 && PL >= 1 && C >= 4 && C <= 256 && 256 % C == 0 && H >= 4 && H <= 1024 &&
              H % 4 == 0 && L >= 4 && L <= 256 && L % 4 == 0;
    for (int j = 0; ok && j < 14; ++j) ok = in[j] != nullptr;
    for (int j = 0; ok && j < 4; ++j) ok = out[j] != nullptr;              // (h, c, pm, plv; the rest optional)
    if (!ok) return free_fail(IODINE_ERR_INVALID, "iodine_op_refine_head: argument");
    if (!split ? refine_head_lds_bytes(C, H, L, 0) > 96 * 1024 : refine_head_form(C, H, L, 1) != 1)
        return free_fail(IODINE_ERR_INVALID, !split ? "iodine_op_refine_head: the single-launch form does not fit the LDS at these widths"
                                 : "iodine_op_refine_head: the three-launch form needs 4 * MLP_UNITS to be a multiple of 32");
    const float *mlp_w = in[0], *mlp_b = in[1], *wih = in[2], *whh = in[3], *bih = in[4], *bhh = in[5], *wm = in[6], *bm = in[7], *wv = in[8],
                *bv = in[9], *feat = in[10], *latent = in[11], *h_prev = in[12], *c_prev = in[13];
    const size_t IN = (size_t)H + 4 * L, Kg = IN + H, Np = ((size_t)N + 31) / 32 * 32;
    const size_t n_mlp = (size_t)C * H, n_w = Kg * 4 * H, n_b = (size_t)4 * H, n_u = (size_t)H * L, n_xh = split ? Np * Kg : 0, n_gp = split ? Np * 4 * H : 0;
    // ([W_ih^T ; W_hh^T] are one region, xh and gp another: the gate GEMM reads the first, one zero fill covers the second)
    OpScratch scr("iodine_op_refine_head", {n_mlp * sizeof(float), n_w * sizeof(float), n_b * sizeof(float), n_u * sizeof(float), n_u * sizeof(float),
                                            (n_xh + n_gp) * sizeof(float)});
    if (!scr.ok()) return IODINE_ERR_HIP;
    float *mlp_wT = scr.at(0), *wihT = scr.at(1), *whhT = wihT + IN * 4 * H, *lstm_b = scr.at(2), *wmT = scr.at(3), *wvT = scr.at(4), *xh = scr.at(5),
          *gp = xh + n_xh;
    // the operands as iodine_set_params builds them: transposes to [in][out], [W_ih^T ; W_hh^T] back to back, b_ih + b_hh (six entries: no flush)
    CopyBatch cb(st);
    (void)cb.transpose(mlp_wT, mlp_w, H, C); (void)cb.transpose(wihT, wih, 4 * H, (int)IN); (void)cb.transpose(whhT, whh, 4 * H, H);
    (void)cb.add2(lstm_b, bih, bhh, 4 * H); (void)cb.transpose(wmT, wm, L, H); (void)cb.transpose(wvT, wv, L, H);
    hipError_t e = cb.flush();
    if (e == hipSuccess && split) e = launch_zero_fill(st, xh, n_xh + n_gp);      // (rows N .. Np of the gate GEMM: the workspace's are finite too)
    if (e == hipSuccess)
        e = launch_refine_head(st, feat, N, PL, C, H, L, mlp_wT, mlp_b, wihT, whhT, lstm_b, wmT, bm, wvT, bv, latent, h_prev, c_prev, out[0], out[1],
                               out[2], out[3], out[6], out[7], out[8], out[9], out[4], out[5], split ? xh : nullptr, split ? gp : nullptr, 1);
    return op_done("iodine_op_refine_head", st, e);
}

int iodine_op_head_bptt(void* stream, int form, const float* const* in, float* const* out, int T, int N, int B, int L, int H, int Cr,
                        long long seed_stride)
{
    hipStream_t st = (hipStream_t)stream;
    bool ok = in && out && (form == IODINE_BPTT_FUSED || form == IODINE_BPTT_SEQUENCE) && T >= 1 && N >= 1 && B >= 1 && L >= 1 && H >= 1 && Cr >= 1 && seed_stride >= 0;
    for (int j = 0; ok && j < 10; ++j) ok = in[j] != nullptr;
    for (int j = 0; ok && j < 5; ++j) ok = out[j] != nullptr;
    if (!ok) return free_fail(IODINE_ERR_INVALID, "iodine_op_head_bptt: argument");
    const float *seed_m = in[10], *seed_v = in[11], *gl = in[12], *wtab = in[13], *dh_in = in[14], *dc_in = in[15];
    if ((seed_m == nullptr) != (seed_v == nullptr) || (!seed_m && (gl || dh_in || dc_in || out[5] || out[6] || seed_stride)))
        return free_fail(IODINE_ERR_INVALID, "iodine_op_head_bptt: gl, the carries and seed_stride belong to the seeded form (seed_m and seed_v given)");
    if (form == IODINE_BPTT_FUSED) {
        if (!head_bptt_fits(L, H, Cr)) return free_fail(IODINE_ERR_INVALID, "iodine_op_head_bptt: the fused kernel takes Cr <= H, and L, H, Cr multiples of 4");
        return op_done("iodine_op_head_bptt", st,
                       launch_head_bptt(st, in[0], in[1], in[2], in[3], in[4], in[5], in[6], in[7], in[8], in[9], out[0], out[1], out[2], out[3], out[4],
                                        T, N, B, L, H, Cr, seed_m, seed_v, gl, wtab, dh_in, dc_in, out[5], out[6], (size_t)seed_stride));
    }
    std::vector<float> whost;
    if (wtab) {                                                          // the launch sequence takes the loss weights from the host
        whost.resize((size_t)T + 1);
        const hipError_t e = hipMemcpyAsync(whost.data(), wtab, sizeof(float) * ((size_t)T + 1), hipMemcpyDeviceToHost, st);
        if (int rc = op_done("iodine_op_head_bptt", st, e)) return rc;
    }
    const size_t NH = (size_t)N * H * sizeof(float);                     // dc1, dxin, carry_h[2], carry_c[2]
    OpScratch scr("iodine_op_head_bptt", {NH, NH, NH, NH, NH, NH});
    if (!scr.ok()) return IODINE_ERR_HIP;
    float* const ch[2] = {scr.at(2), scr.at(3)};
    float* const cc[2] = {scr.at(4), scr.at(5)};
    return op_done("iodine_op_head_bptt", st,
                   launch_head_bptt_unfused(st, in[0], in[1], in[2], in[3], in[4], in[5], in[6], in[7], in[8], in[9], out[0], out[1], out[2], out[3], out[4],
                                            T, N, B, L, H, Cr, seed_m != nullptr, seed_m, seed_v, gl, wtab ? whost.data() : nullptr, dh_in, dc_in, out[5],
                                            out[6], (size_t)seed_stride, scr.at(0), scr.at(1), ch, cc));
}

int iodine_op_pool_bwd(void* stream, const float* dpooled, const float* act, float* dpre, int N, int PL, int C)
{
    hipStream_t st = (hipStream_t)stream;
    if (!dpooled || !act || !dpre || N < 1 || PL < 1 || C < 1) return free_fail(IODINE_ERR_INVALID, "iodine_op_pool_bwd: argument");
    return op_done("iodine_op_pool_bwd", st, launch_pool_bwd(st, dpooled, act, dpre, N, PL, C));
}

int iodine_op_refine_head_form(int C, int H, int L, int prefer_split) { return refine_head_form(C, H, L, prefer_split); }

}  // extern "C"
