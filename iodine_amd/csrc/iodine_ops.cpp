// Handle-free entry points of libiodine_hip.so: the optimizer and metric launches, the Philox sampler, the host linspace and the
// operator-level test entry points (iodine_op_*).  See include/iodine_hip.h.
#include "iodine_internal.h"
#include "assign.h"

extern "C" {

int iodine_adam_step(void* stream, const long long* ptrs_dev, const long long* offsets_dev, int n_tensors, long long total,
                     double lr, double beta1, double beta2, double eps, double weight_decay, int step)
{
    if (!ptrs_dev || !offsets_dev || n_tensors < 1 || total < 1 || step < 1) { g_create_error = "iodine_adam_step: bad argument"; return IODINE_ERR_INVALID; }
    const hipError_t e = launch_adam_multi((hipStream_t)stream, ptrs_dev, offsets_dev, n_tensors, total, lr, beta1, beta2, eps,
                                           weight_decay, step);
    if (e != hipSuccess) { g_create_error = std::string("iodine_adam_step: ") + hipGetErrorString(e); return IODINE_ERR_HIP; }
    return IODINE_OK;
}

size_t iodine_grad_norm_scratch_bytes(long long total)
{
    return total < 1 ? 0 : grad_norm_scratch_bytes(total);
}

int iodine_grad_norm(void* stream, const long long* ptrs_dev, const long long* offsets_dev, int n_tensors, long long total,
                     double max_norm, void* scratch_dev, size_t scratch_bytes, float* out4_dev)
{
    if (!ptrs_dev || !offsets_dev || n_tensors < 1 || total < 1 || !scratch_dev || !out4_dev || !(max_norm > 0.0) ||
        scratch_bytes < grad_norm_scratch_bytes(total) || ((uintptr_t)scratch_dev & 7)) {
        g_create_error = "iodine_grad_norm: bad argument (max_norm must be > 0; scratch of iodine_grad_norm_scratch_bytes, 8-byte aligned)";
        return IODINE_ERR_INVALID;
    }
    const hipError_t e = launch_grad_norm((hipStream_t)stream, ptrs_dev, offsets_dev, n_tensors, total, max_norm,
                                          (double*)scratch_dev, out4_dev);
    if (e != hipSuccess) { g_create_error = std::string("iodine_grad_norm: ") + hipGetErrorString(e); return IODINE_ERR_HIP; }
    return IODINE_OK;
}

int iodine_grad_scale(void* stream, const long long* ptrs_dev, const long long* offsets_dev, int n_tensors, long long total,
                      const float* coef_dev)
{
    if (!ptrs_dev || !offsets_dev || n_tensors < 1 || total < 1 || !coef_dev) { g_create_error = "iodine_grad_scale: bad argument"; return IODINE_ERR_INVALID; }
    const hipError_t e = launch_grad_scale((hipStream_t)stream, ptrs_dev, offsets_dev, n_tensors, total, coef_dev);
    if (e != hipSuccess) { g_create_error = std::string("iodine_grad_scale: ") + hipGetErrorString(e); return IODINE_ERR_HIP; }
    return IODINE_OK;
}

int iodine_adam_step_clipped(void* stream, const long long* ptrs_dev, const long long* offsets_dev, int n_tensors, long long total,
                             double lr, double beta1, double beta2, double eps, double weight_decay, int step,
                             const float* out4_dev, int skip_nonfinite)
{
    if (!ptrs_dev || !offsets_dev || n_tensors < 1 || total < 1 || step < 1 || !out4_dev) { g_create_error = "iodine_adam_step_clipped: bad argument"; return IODINE_ERR_INVALID; }
    const hipError_t e = launch_adam_multi((hipStream_t)stream, ptrs_dev, offsets_dev, n_tensors, total, lr, beta1, beta2, eps,
                                           weight_decay, step, out4_dev, skip_nonfinite ? 1 : 0);
    if (e != hipSuccess) { g_create_error = std::string("iodine_adam_step_clipped: ") + hipGetErrorString(e); return IODINE_ERR_HIP; }
    return IODINE_OK;
}

int iodine_ari_table(void* stream, const float* mask, const unsigned char* gt, int batch, int slots, int n_gt, int pixels,
                     int* table)
{
    if (!mask || !gt || !table || batch < 1 || slots < 1 || n_gt < 1 || pixels < 1 || (size_t)n_gt * slots > 8192) {
        g_create_error = "iodine_ari_table: bad argument";
        return IODINE_ERR_INVALID;
    }
    const hipError_t e = launch_ari_table((hipStream_t)stream, mask, gt, batch, slots, n_gt, pixels, table);
    if (e != hipSuccess) { g_create_error = std::string("iodine_ari_table: ") + hipGetErrorString(e); return IODINE_ERR_HIP; }
    return IODINE_OK;
}

int iodine_slot_table(void* stream, const float* mask, const float* mean_or_null, int batch, int slots, int size,
                      float* table, unsigned char* seg_or_null)
{
    if (!mask || !table || batch < 1 || slots < 1 || slots > 16 || size < 1 || size > 1024) {
        g_create_error = "iodine_slot_table: bad argument (mask and table required, batch >= 1, slots in 1..16, size in 1..1024)";
        return IODINE_ERR_INVALID;
    }
    const hipError_t e = launch_slot_table((hipStream_t)stream, mask, mean_or_null, batch, slots, size, table, seg_or_null);
    if (e != hipSuccess) { g_create_error = std::string("iodine_slot_table: ") + hipGetErrorString(e); return IODINE_ERR_HIP; }
    return IODINE_OK;
}

int iodine_seg_overlap(void* stream, const unsigned char* seg_a, const unsigned char* seg_b, int batch, int slots_a, int slots_b,
                       int pixels, int* table)
{
    if (!seg_a || !seg_b || !table || batch < 1 || slots_a < 1 || slots_a > 16 || slots_b < 1 || slots_b > 16 || pixels < 1 ||
        pixels > 1024 * 1024) {
        g_create_error = "iodine_seg_overlap: bad argument (three pointers required, batch >= 1, slots_a / slots_b in 1..16, pixels in 1..1024^2)";
        return IODINE_ERR_INVALID;
    }
    const hipError_t e = launch_seg_overlap((hipStream_t)stream, seg_a, seg_b, batch, slots_a, slots_b, pixels, table);
    if (e != hipSuccess) { g_create_error = std::string("iodine_seg_overlap: ") + hipGetErrorString(e); return IODINE_ERR_HIP; }
    return IODINE_OK;
}

int iodine_mask_overlap(void* stream, const float* mask, const unsigned char* gt, int batch, int slots, int n_gt, int size, float eps,
                        float* inter, float* nll_or_null, float* mask_area, int* gt_area)
{
    if (!mask || !gt || !inter || !mask_area || !gt_area || batch < 1 || slots < 1 || slots > 16 || n_gt < 1 || n_gt > 16 || size < 1 ||
        size > 1024 || !(eps > 0.f)) {
        g_create_error = "iodine_mask_overlap: bad argument (mask, gt, inter, mask_area, gt_area required, batch >= 1, slots and n_gt in 1..16, "
                         "size in 1..1024, eps > 0)";
        return IODINE_ERR_INVALID;
    }
    const hipError_t e = launch_mask_overlap((hipStream_t)stream, mask, gt, batch, slots, n_gt, size, eps, inter, nll_or_null, mask_area,
                                             gt_area);
    if (e != hipSuccess) { g_create_error = std::string("iodine_mask_overlap: ") + hipGetErrorString(e); return IODINE_ERR_HIP; }
    return IODINE_OK;
}

int iodine_assign(void* stream, const float* cost, const unsigned char* row_valid_or_null, int batch, int n_rows, int n_cols,
                  int* assign, float* total)
{
    if (!cost || !assign || !total || batch < 1 || n_rows < 1 || n_rows > 16 || n_cols < 1 || n_cols > 16) {
        g_create_error = "iodine_assign: bad argument (cost, assign, total required, batch >= 1, n_rows and n_cols in 1..16)";
        return IODINE_ERR_INVALID;
    }
    const hipError_t e = launch_assign((hipStream_t)stream, cost, row_valid_or_null, batch, n_rows, n_cols, assign, total);
    if (e != hipSuccess) { g_create_error = std::string("iodine_assign: ") + hipGetErrorString(e); return IODINE_ERR_HIP; }
    return IODINE_OK;
}

int iodine_assign_host(const float* cost, const unsigned char* row_valid_or_null, int n_rows, int n_cols, int* assign, float* total)
{
    if (!cost || !assign || !total || n_rows < 1 || n_rows > 16 || n_cols < 1 || n_cols > 16) {
        g_create_error = "iodine_assign_host: bad argument (cost, assign, total required, n_rows and n_cols in 1..16)";
        return IODINE_ERR_INVALID;
    }
    IodAssignWork work;
    iod_assign_solve(cost, row_valid_or_null, n_rows, n_cols, assign, total, &work);
    return IODINE_OK;
}

int iodine_mask_match(void* stream, const float* inter, const float* nll_or_null, const float* mask_area, const int* gt_area, int batch,
                      int slots, int n_gt, int match_kind, int loss_kind, int* assign, float* loss, float* coef, float* cost_or_null,
                      float* iou_or_null)
{
    const bool kinds = (match_kind == 0 || match_kind == 1) && (loss_kind == 0 || loss_kind == 1);
    if (!inter || !mask_area || !gt_area || !assign || !loss || !coef || batch < 1 || slots < 1 || slots > 16 || n_gt < 1 || n_gt > 16 ||
        !kinds || ((match_kind == 1 || loss_kind == 1) && !nll_or_null)) {
        g_create_error = "iodine_mask_match: bad argument (inter, mask_area, gt_area, assign, loss, coef required, batch >= 1, slots and n_gt in "
                         "1..16, kinds 0 = iou / 1 = ce, and nll with either kind 1)";
        return IODINE_ERR_INVALID;
    }
    const hipError_t e = launch_mask_match((hipStream_t)stream, inter, nll_or_null, mask_area, gt_area, batch, slots, n_gt, match_kind,
                                           loss_kind, assign, loss, coef, cost_or_null, iou_or_null);
    if (e != hipSuccess) { g_create_error = std::string("iodine_mask_match: ") + hipGetErrorString(e); return IODINE_ERR_HIP; }
    return IODINE_OK;
}

int iodine_mask_match_backward(void* stream, const float* mask, const unsigned char* gt, const int* assign, const float* coef,
                               const float* grad_loss, int batch, int slots, int n_gt, int size, int loss_kind, float eps,
                               float* grad_mask)
{
    if (!mask || !gt || !assign || !coef || !grad_loss || !grad_mask || batch < 1 || slots < 1 || slots > 16 || n_gt < 1 || n_gt > 16 ||
        size < 1 || size > 1024 || (loss_kind != 0 && loss_kind != 1) || !(eps > 0.f)) {
        g_create_error = "iodine_mask_match_backward: bad argument (six pointers required, batch >= 1, slots and n_gt in 1..16, size in 1..1024, "
                         "loss_kind 0 = iou / 1 = ce, eps > 0)";
        return IODINE_ERR_INVALID;
    }
    const hipError_t e = launch_mask_match_bwd((hipStream_t)stream, mask, gt, assign, coef, grad_loss, batch, slots, n_gt, size, loss_kind,
                                               eps, grad_mask);
    if (e != hipSuccess) { g_create_error = std::string("iodine_mask_match_backward: ") + hipGetErrorString(e); return IODINE_ERR_HIP; }
    return IODINE_OK;
}

int iodine_batch_gather(void* stream, const long long* index, int count, const void* images, int image_kind,
                        const unsigned short* masks_or_null, int size, int planes, float* x, unsigned char* gt_or_null)
{
    if (!index || !images || !x || count < 1 || size < 1 || size > 4096 || planes < 1 || planes > 16 || (image_kind != 0 && image_kind != 1)) {
        g_create_error = "iodine_batch_gather: bad argument (index, images, x required, count >= 1, size in 1..4096, planes in 1..16, "
                         "image_kind 0 = uint8 HWC / 1 = float32 CHW)";
        return IODINE_ERR_INVALID;
    }
    const hipError_t e = launch_batch_gather((hipStream_t)stream, index, count, images, image_kind, masks_or_null, size, planes, x, gt_or_null);
    if (e != hipSuccess) { g_create_error = std::string("iodine_batch_gather: ") + hipGetErrorString(e); return IODINE_ERR_HIP; }
    return IODINE_OK;
}

int iodine_synth_scenes(void* stream, int n, int size, unsigned long long seed, unsigned long long seed_step, unsigned long long stream_id,
                        unsigned long long stream_step, int kind, int max_objects, int frames, float* images,
                        unsigned short* masks_or_null, unsigned char* n_gt_or_null)
{
    if (!images || n < 1 || size < 1 || size > 1024 || (kind != 0 && kind != 1) || max_objects < 1 || max_objects > 16 || frames < 0 ||
        (long long)n * (frames > 0 ? frames : 1) > 0x7FFFFFFFll) {
        g_create_error = "iodine_synth_scenes: bad argument (images required, n >= 1, size in 1..1024, kind 0 = uniform / 1 = blobs, "
                         "max_objects in 1..16, frames >= 0, n * frames < 2^31)";
        return IODINE_ERR_INVALID;
    }
    const hipError_t e = launch_synth_scenes((hipStream_t)stream, n, size, seed, seed_step, stream_id, stream_step, kind, max_objects, frames,
                                             images, masks_or_null, n_gt_or_null);
    if (e != hipSuccess) { g_create_error = std::string("iodine_synth_scenes: ") + hipGetErrorString(e); return IODINE_ERR_HIP; }
    return IODINE_OK;
}

int iodine_randn(void* stream, float* out, long long n, unsigned long long seed, unsigned long long stream_id)
{
    if (!out || n < 1) { g_create_error = "iodine_randn: bad argument"; return IODINE_ERR_INVALID; }
    const hipError_t e = launch_randn_philox((hipStream_t)stream, out, n, seed, stream_id);
    if (e != hipSuccess) { g_create_error = std::string("iodine_randn: ") + hipGetErrorString(e); return IODINE_ERR_HIP; }
    return IODINE_OK;
}

void iodine_linspace_host(int n, float* out)
{
    // ATen's CPU linspace for float: step = (end - start) / (n - 1); first half counts up from start,
    // second half counts down from end (symmetric), all in fp32.
    const float start = -1.f, end = 1.f;
    if (n == 1) { out[0] = start; return; }
    const float step = (end - start) / (float)(n - 1);
    const int halfway = n / 2;
    for (int i = 0; i < n; ++i)
        out[i] = i < halfway ? start + step * (float)i : end - step * (float)(n - i - 1);
}

// ---- operator-level test entry points ---------------------------------------------------------
static std::string g_op_error;

int iodine_op_conv3x3(void* stream, int mode, const float* in, const float* w, const float* bias, const float* aux,
                      float* out, int n, int ih, int iw, int w_o, int w_i, int cin_pad, int cout, int stride, int epi,
                      int tflip)
{
    hipStream_t st = (hipStream_t)stream;
    float* wpk = nullptr;
    if (mode == 5 || mode == 6 || mode == 13 || mode == 14) {   // stride-2 forward (5) / data gradient (6), split-fp16; 13 / 14: their exact-fp32 forms; ih = fine size
        float* meta = nullptr;
        const bool fwd = mode == 5 || mode == 13;
        const int f32 = mode >= 13;
        const int cp = fwd ? (cin_pad == 20 ? 32 : (cin_pad == 12 || cin_pad == 8 ? 16 : cin_pad)) : cin_pad;   // floats per pixel -> packed chunks
        const size_t bytes = (size_t)(cp / 16) * 9 * 2 * 2 * cout * 16;
        if (hipMalloc((void**)&wpk, bytes + 64) != hipSuccess) return IODINE_ERR_HIP;
        meta = (float*)((char*)wpk + bytes);
        hipError_t e2 = f32 ? launch_pack_conv_weights_s2f32(st, w, w_o, w_i, cp, cout, fwd ? 0 : 2, wpk)
                            : launch_pack_conv_weights_f16(st, w, w_o, w_i, cp, cout, fwd ? 0 : 2, meta, wpk);
        if (e2 == hipSuccess)
            e2 = fwd ? launch_conv3x3_s2_f16x3(st, in, wpk, meta, bias, out, n, ih, cin_pad, cout, nullptr, 0, f32)
                     : launch_conv3x3_s2_dgrad_f16x3(st, in, wpk, meta, aux, out, n, ih, cout, f32);
        if (e2 == hipSuccess) e2 = hipStreamSynchronize(st);
        (void)hipFree(wpk);
        if (e2 != hipSuccess) { g_create_error = std::string("iodine_op_conv3x3(s2 f16x3): ") + hipGetErrorString(e2); return IODINE_ERR_HIP; }
        return IODINE_OK;
    }
    if (mode == 9 || mode == 10 || mode == 17) {  // weight-stationary split-fp16 kernel (per-cell max side buffer from launch_cell_max); 17: its one-product form (conv_precision 2)
        if (cin_pad != cout || w_o != cout || w_i != cout || ih != iw || ih % 16 != 0) { g_create_error = "iodine_op_conv3x3(ws): shape"; return IODINE_ERR_INVALID; }
        const size_t wb = conv_ws_wpk_bytes(cout), tf = conv_ws_tmax_floats(n, ih);
        char* buf = nullptr;
        if (hipMalloc((void**)&buf, wb + 64 + 2 * tf * sizeof(float)) != hipSuccess) return IODINE_ERR_HIP;
        float* meta = (float*)(buf + wb);
        float *tin = (float*)(buf + wb + 64), *tout = tin + tf;
        hipError_t e2 = launch_pack_conv_weights_ws(st, w, cout, tflip, meta, buf);
        if (e2 == hipSuccess) e2 = launch_cell_max(st, in, tin, n, ih, cout);
        if (e2 == hipSuccess) e2 = launch_conv3x3_ws_f16x3(st, in, buf, meta, bias, aux, out, tin, tout, n, ih, cout, epi, 0, mode == 17 ? 1 : 3);
        if (e2 == hipSuccess) e2 = hipStreamSynchronize(st);
        (void)hipFree(buf);
        if (e2 != hipSuccess) { g_create_error = std::string("iodine_op_conv3x3(ws): ") + hipGetErrorString(e2); return IODINE_ERR_HIP; }
        return IODINE_OK;
    }
    if (mode == 15 || mode == 16) { // weight-stationary STRIDE-2 conv c -> c + bias + ELU (kernels_refws.hip): split-fp16 (15) / exact fp32 (16); ih = fine size
        if (cin_pad != cout || w_o != cout || w_i != cout || ih != iw || !conv3x3_s2ws_ok(ih, cout)) { g_create_error = "iodine_op_conv3x3(s2ws): shape"; return IODINE_ERR_INVALID; }
        char* buf = nullptr;
        const size_t wb = conv_ws_wpk_bytes(cout);
        if (hipMalloc((void**)&buf, wb + 64) != hipSuccess) return IODINE_ERR_HIP;
        float* meta = (float*)(buf + wb);
        hipError_t e2 = mode == 16 ? launch_pack_conv_weights_ws32(st, w, cout, 0, buf) : launch_pack_conv_weights_ws(st, w, cout, 0, meta, buf);
        if (e2 == hipSuccess) e2 = launch_conv3x3_s2ws_f16x3(st, in, buf, meta, bias, out, n, ih, cout, mode == 16);
        if (e2 == hipSuccess) e2 = hipStreamSynchronize(st);
        (void)hipFree(buf);
        if (e2 != hipSuccess) { g_create_error = std::string("iodine_op_conv3x3(s2ws): ") + hipGetErrorString(e2); return IODINE_ERR_HIP; }
        return IODINE_OK;
    }
    if (mode == 12) {               // exact-fp32 form of the weight-stationary kernel (v_mfma_f32_16x16x4_f32)
        if (cin_pad != cout || w_o != cout || w_i != cout || ih != iw || ih % 16 != 0) { g_create_error = "iodine_op_conv3x3(ws f32): shape"; return IODINE_ERR_INVALID; }
        char* buf = nullptr;
        if (hipMalloc((void**)&buf, conv_ws_wpk_bytes(cout)) != hipSuccess) return IODINE_ERR_HIP;
        hipError_t e2 = launch_pack_conv_weights_ws32(st, w, cout, tflip, buf);
        if (e2 == hipSuccess) e2 = launch_conv3x3_ws_f32(st, in, buf, bias, aux, out, n, ih, cout, epi, 0);
        if (e2 == hipSuccess) e2 = hipStreamSynchronize(st);
        (void)hipFree(buf);
        if (e2 != hipSuccess) { g_create_error = std::string("iodine_op_conv3x3(ws f32): ") + hipGetErrorString(e2); return IODINE_ERR_HIP; }
        return IODINE_OK;
    }
#ifdef IODINE_WITH_WINO
    if (mode == 11) {               // Winograd F(2x2, 3x3) split-fp16 kernel (C = 64): experiment libraries only (tools/wino_variants.sh)
        if (cin_pad != cout || w_o != cout || w_i != cout || ih != iw || ih % 16 != 0) { g_create_error = "iodine_op_conv3x3(wino): shape"; return IODINE_ERR_INVALID; }
        const size_t wb = conv_wino_wpk_bytes(cout), tf = conv_ws_tmax_floats(n, ih), sf = conv_wino_scratch_floats(cout);
        char* buf = nullptr;
        if (hipMalloc((void**)&buf, wb + 64 + (2 * tf + sf) * sizeof(float)) != hipSuccess) return IODINE_ERR_HIP;
        float* meta = (float*)(buf + wb);
        float *tin = (float*)(buf + wb + 64), *tout = tin + tf, *scr = tout + tf;
        hipError_t e2 = launch_pack_conv_weights_wino(st, w, cout, tflip, meta, buf, scr);
        if (e2 == hipSuccess) e2 = launch_cell_max(st, in, tin, n, ih, cout);
        if (e2 == hipSuccess) e2 = launch_conv3x3_wino_f16x3(st, in, buf, meta, bias, aux, out, tin, tout, n, ih, cout, epi, 0);
        if (e2 == hipSuccess) e2 = hipStreamSynchronize(st);
        (void)hipFree(buf);
        if (e2 != hipSuccess) { g_create_error = std::string("iodine_op_conv3x3(wino): ") + hipGetErrorString(e2); return IODINE_ERR_HIP; }
        return IODINE_OK;
    }
#endif
    if (mode == 2) {                // split-fp16 LDS-tiled kernel
        float* meta = nullptr;
        const size_t bytes = (size_t)(cin_pad / 16) * 9 * 2 * 2 * cout * 16;
        if (hipMalloc((void**)&wpk, bytes + 64) != hipSuccess) return IODINE_ERR_HIP;
        meta = (float*)((char*)wpk + bytes);
        hipError_t e2 = launch_pack_conv_weights_f16(st, w, w_o, w_i, cin_pad, cout, tflip, meta, wpk);
        if (e2 == hipSuccess)
            e2 = launch_conv3x3_tile_f16x3(st, in, wpk, meta, bias, aux, out, n, ih, cin_pad, cout, epi, 0);
        if (e2 == hipSuccess) e2 = hipStreamSynchronize(st);
        (void)hipFree(wpk);
        if (e2 != hipSuccess) { g_create_error = std::string("iodine_op_conv3x3(f16x3): ") + hipGetErrorString(e2); return IODINE_ERR_HIP; }
        return IODINE_OK;
    }
    if (hipMalloc((void**)&wpk, conv_wpk_elems(cin_pad, cout) * 16) != hipSuccess) return IODINE_ERR_HIP;
    hipError_t e = launch_pack_conv_weights(st, w, w_o, w_i, cin_pad, cout, tflip, wpk);
    if (e == hipSuccess) {
        if (mode == 0) e = (ih == iw && stride == 1) ? launch_conv3x3_tile(st, in, wpk, bias, aux, out, n, ih, cin_pad, cout, epi)
                                                     : hipErrorInvalidValue;
        else e = launch_conv3x3_gather(st, in, wpk, bias, out, n, ih, iw, cin_pad, cout, stride);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    (void)hipFree(wpk);
    if (e != hipSuccess) { g_create_error = std::string("iodine_op_conv3x3: ") + hipGetErrorString(e); return IODINE_ERR_HIP; }
    return IODINE_OK;
}

int iodine_op_dec_out(void* stream, const float* in, const float* w, const float* bias, float* out, int n, int s, int c)
{
    hipStream_t st = (hipStream_t)stream;
    float* wk = nullptr;
    if (hipMalloc((void**)&wk, (size_t)9 * c * 4 * sizeof(float)) != hipSuccess) return IODINE_ERR_HIP;
    hipError_t e = launch_pack_dec_out(st, w, wk, c);
    if (e == hipSuccess) e = launch_dec_out(st, in, wk, bias, out, n, s, c);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    (void)hipFree(wk);
    if (e != hipSuccess) { g_create_error = std::string("iodine_op_dec_out: ") + hipGetErrorString(e); return IODINE_ERR_HIP; }
    return IODINE_OK;
}

int iodine_op_dec_out_f16x3(void* stream, const float* in, const float* w, const float* bias, float* out, int n, int s, int c, int variant)
{
    hipStream_t st = (hipStream_t)stream;
    const size_t wb = (size_t)(c / 16) * 2 * 2 * 64 * 16, tf = conv_ws_tmax_floats(n, s);
    char* buf = nullptr;
    if (s % 16 != 0 || (c != 64 && c != 32)) { g_create_error = "iodine_op_dec_out_f16x3: shape"; return IODINE_ERR_INVALID; }
    if (hipMalloc((void**)&buf, wb + 64 + tf * sizeof(float)) != hipSuccess) return IODINE_ERR_HIP;
    float* meta = (float*)(buf + wb);
    float* tin = (float*)(buf + wb + 64);
    hipError_t e = launch_pack_dec_out_gemm(st, w, c, meta, buf);
    if (e == hipSuccess) e = launch_cell_max(st, in, tin, n, s, c);
    if (e == hipSuccess && variant == 3) {          // exact-fp32 row-streaming form: its own weight operand (the buffer is large enough)
        e = launch_pack_dec_out_rows32(st, w, c, (float*)buf);
        if (e == hipSuccess) e = launch_dec_out_rows_f16x3(st, in, buf, nullptr, bias, out, n, s, c, nullptr, 1);
    } else if (e == hipSuccess)
        e = variant == 1 ? launch_dec_out_rows_f16x3(st, in, buf, meta, bias, out, n, s, c, tin)
                         : launch_dec_out_stream_f16x3(st, in, buf, meta, bias, out, n, s, c, variant == 2 ? nullptr : tin);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    (void)hipFree(buf);
    if (e != hipSuccess) { g_create_error = std::string("iodine_op_dec_out_f16x3: ") + hipGetErrorString(e); return IODINE_ERR_HIP; }
    return IODINE_OK;
}

int iodine_op_conv3x3_wgrad(void* stream, const float* in, const float* d, float* gw, float* gb, int n, int s, int ci_pad,
                            int ci_real, int co, int stride)
{
    hipStream_t st = (hipStream_t)stream;
    const int cmax = std::max(std::max(ci_pad, co), 32);
    const size_t part_elems = (size_t)512 * 4 * 9 * cmax * cmax, fold_elems = (size_t)WGRAD_FOLD * 9 * cmax * cmax;
    float* buf = nullptr;
    if (hipMalloc((void**)&buf, (part_elems + fold_elems + (size_t)512 * 64) * sizeof(float)) != hipSuccess) return IODINE_ERR_HIP;
    float *part = buf, *fold = buf + part_elems, *part_b = fold + fold_elems;
    int nparts = 0, cip = 0, nb = 0;
    hipError_t e;
    if (stride == 1 && co == 4) {
        e = launch_dec_out_wgrad_gemm_f16x3(st, in, d, part, part_b, n, s, ci_pad, &nparts, &nb);
        if (e == hipSuccess) e = launch_wgrad_reduce(st, part, nparts, ci_pad, 4, 4, ci_real, ci_real, 1.f, gw, fold);
    } else if (stride == 1) {
        e = launch_conv3x3_wgrad_f16x3_ws(st, in, d, part, part_b, n, s, ci_pad, co, &nparts, &cip, &nb);
        // stride-1 partial tiles are [9][ci][co padded to 32]
        if (e == hipSuccess) e = launch_wgrad_reduce(st, part, nparts, ci_pad, cip, co, ci_real, ci_real, 1.f, gw, fold);
    } else {                                           // stride 2; stride -2: the exact-fp32 form of the same kernel
        e = launch_conv3x3_s2_wgrad_f16x3(st, in, d, part, part_b, n, s, ci_pad, co, &nparts, &cip, &nb, nullptr, 0, stride == -2);
        if (e == hipSuccess) e = launch_wgrad_reduce(st, part, nparts, cip, co, co, ci_real, ci_real, 1.f, gw, fold);
    }
    if (e == hipSuccess) e = launch_colsum(st, part_b, nb, co, co, 1.f, gb);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    (void)hipFree(buf);
    if (e != hipSuccess) { g_create_error = std::string("iodine_op_conv3x3_wgrad: ") + hipGetErrorString(e); return IODINE_ERR_HIP; }
    return IODINE_OK;
}

int iodine_op_gen_conv(void* stream, int mode, const float* in, const float* w, const float* bias, const float* aux, float* out, float* gb,
                       int n, int si, int ci, int ldc, int co, int k, int s, int elu)
{
    hipStream_t st = (hipStream_t)stream;
    if (mode < 0 || mode > 2 || s < 1 || s > 8 || (k != 3 && k != 5 && k != 7) || ldc < ci) { g_create_error = "iodine_op_gen_conv: argument"; return IODINE_ERR_INVALID; }
    // tests only: elu bit 8 set = bits 9.. carry a per-channel mask of the input channels that can be non-zero (what the library hands
    // the stride-2 kernels for an ARCH.ENCODING subset: all-zero 4- / 16-channel groups are skipped) - the masked form must equal the plain one
    const unsigned chmask = (elu & 0x100) ? ((unsigned)elu >> 9) : 0xffffffffu;
    elu &= 1;
    float* buf = nullptr;
    // weights [tap][ci][co]: the forward pack has ci rows, the data-gradient pack ldc rows (the packed input-channel count is din's stride)
    const size_t wfl = (size_t)k * k * ldc * co, scr = mode == 2 ? gen_wgrad_scratch_floats(ci, co, k) : 0;
    if (hipMalloc((void**)&buf, (wfl + scr) * sizeof(float)) != hipSuccess) return IODINE_ERR_HIP;
    hipError_t e = hipSuccess;
    if (mode == 0) {
        e = launch_gen_pack_weights(st, w, co, ci, k, buf);
        if (e == hipSuccess) e = launch_gen_conv_fwd(st, in, buf, bias, out, n, si, ci, ldc, co, k, s, elu, chmask);
    } else if (mode == 1) {
        e = launch_gen_pack_weights(st, w, co, ldc, k, buf);    // (w has ldc input channels here: ci of them are computed)
        if (e == hipSuccess) e = launch_gen_conv_dgrad(st, in, buf, aux, out, n, si, ci, ldc, co, k, s);
    } else {
        e = launch_gen_conv_wgrad(st, in, aux, buf + wfl, n, si, ci, ldc, ci, co, k, s, 1.f, out, gb, chmask);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    (void)hipFree(buf);
    if (e != hipSuccess) { g_create_error = std::string("iodine_op_gen_conv: ") + hipGetErrorString(e); return IODINE_ERR_HIP; }
    return IODINE_OK;
}

int iodine_op_gen_conv_tier(int mode, int si, int ci, int ldc, int co, int k, int s)
{
    // (host arithmetic only: runs without a GPU)
    if (mode < 0 || mode > 2 || si < 1 || ci < 1 || co < 1 || s < 1 || s > 8 || (k != 3 && k != 5 && k != 7) || ldc < ci) return -1;
    const GenTierSel sel = gen_conv_tier(mode, si, ci, ldc, co, k, s);
    return (int)sel.tier | (sel.np << 8) | (sel.seg << 16);
}

int iodine_op_gen_l0(void* stream, int mode, const float* z, const float* w, const float* bias, const float* dpre, float* out, float* gw,
                     float* gb, float* dz, int n, int L, int s, int co, int k, int ld, float alpha)
{
    hipStream_t st = (hipStream_t)stream;
    // (kernel-level tests only: allocates and frees its scratch around the launches and synchronises - not an entry point to time)
    if (mode < 0 || mode > 1 || n < 1 || L < 1 || s < 1 || co < 1 || k < 1 || k > GEN_L0_KMAX || k % 2 == 0 || !z || !w
        || (mode == 0 && (!bias || !out)) || (mode == 1 && (!dpre || !dz || ld < L || (alpha != 0.f && (!gw || !gb))))) {
        g_create_error = "iodine_op_gen_l0: argument";
        return IODINE_ERR_INVALID;
    }
    // (every region starts on 16 bytes, as in the library's workspace: the forward reads cterm and the prefix table with 16-byte loads)
    const auto r4 = [](size_t v) { return (v + 3) & ~(size_t)3; };
    const size_t wfl = r4((size_t)k * k * (L + 2) * co), lfl = r4((size_t)s), cfl = mode == 0 ? r4((size_t)s * s * co) : 0,
                 sfl = gen_l0_scratch_floats(n, s, co, k);
    float* buf = nullptr;
    if (hipMalloc((void**)&buf, (wfl + lfl + cfl + sfl) * sizeof(float)) != hipSuccess) return IODINE_ERR_HIP;
    float *wt = buf, *lin = wt + wfl, *cterm = lin + lfl, *scr = cterm + cfl;
    std::vector<float> hlin((size_t)s);
    iodine_linspace_host(s, hlin.data());
    hipError_t e = hipMemcpyAsync(lin, hlin.data(), (size_t)s * sizeof(float), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);         // (hlin is pageable host memory)
    if (e == hipSuccess) e = launch_gen_pack_weights(st, w, co, L + 2, k, wt);
    if (e == hipSuccess && mode == 0) {
        e = launch_gen_l0_coord(st, wt, bias, lin, L, s, co, k, cterm);
        if (e == hipSuccess) e = launch_gen_l0_fwd(st, z, wt, cterm, scr, out, n, L, s, co, k);
    } else if (e == hipSuccess) {
        e = launch_gen_l0_bwd(st, dpre, z, wt, lin, scr, n, L, s, co, k, alpha, gw, gb, dz, ld);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    (void)hipFree(buf);
    if (e != hipSuccess) { g_create_error = std::string("iodine_op_gen_l0: ") + hipGetErrorString(e); return IODINE_ERR_HIP; }
    return IODINE_OK;
}

int iodine_op_gen_conv_f16x3(void* stream, int mode, const float* in, const float* w, const float* bias, const float* aux, float* out, float* gb,
                             int n, int si, int ci, int ldc, int co, int k, int s, int elu)
{
    hipStream_t st = (hipStream_t)stream;
    // (kernel-level tests only: allocates and frees its scratch around the launches and synchronises - not an entry point to time)
    if (mode < 0 || mode > 2 || n < 1 || si < 1) { g_create_error = "iodine_op_gen_conv_f16x3: argument"; return IODINE_ERR_INVALID; }
    if (s != 1 || ci != co || ldc != ci || !gen_split_cch(k, ci)) {
        g_create_error = "iodine_op_gen_conv_f16x3: shape not covered by the split kernels (stride 1, ci = co = ldc a multiple of 16, k in {3, 5, 7}, slice fits LDS)";
        return IODINE_ERR_INVALID;
    }
    if (mode == 2) {
        if (!gen_split_wgrad_ok(k, ci) || !aux || !out || !gb) {
            g_create_error = "iodine_op_gen_conv_f16x3: mode 2 needs aux (gradient), out (gw), gb and a shape the split weight gradient covers";
            return IODINE_ERR_INVALID;
        }
        float* scr = nullptr;
        if (hipMalloc((void**)&scr, gen_wgrad_scratch_floats(ci, co, k) * sizeof(float)) != hipSuccess) return IODINE_ERR_HIP;
        hipError_t e2 = launch_gen_split_wgrad(st, in, aux, scr, n, si, ci, k, 1.f, out, gb);
        if (e2 == hipSuccess) e2 = hipStreamSynchronize(st);
        (void)hipFree(scr);
        if (e2 != hipSuccess) { g_create_error = std::string("iodine_op_gen_conv_f16x3: ") + hipGetErrorString(e2); return IODINE_ERR_HIP; }
        return IODINE_OK;
    }
    if (ci / 16 > 64) { g_create_error = "iodine_op_gen_conv_f16x3: channel count"; return IODINE_ERR_INVALID; }   // (the 64-float scale slot below)
    const size_t wfl = (size_t)k * k * ci * co, pbytes = gen_split_pack_bytes(k, ci);
    float* buf = nullptr;
    if (hipMalloc((void**)&buf, (wfl + 64) * sizeof(float) + pbytes) != hipSuccess) return IODINE_ERR_HIP;
    float* meta = buf + wfl;
    void* pk = buf + wfl + 64;
    hipError_t e = launch_gen_pack_weights(st, w, co, ci, k, buf);
    if (e == hipSuccess) e = launch_gen_split_pack(st, buf, k, ci, mode, pk, meta);
    if (e == hipSuccess) e = launch_gen_split_conv(st, in, pk, meta, mode == 0 ? bias : nullptr, mode == 1 ? aux : nullptr, out, n, si, ci, k, mode == 0 ? (elu & 1) : 0);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    (void)hipFree(buf);
    if (e != hipSuccess) { g_create_error = std::string("iodine_op_gen_conv_f16x3: ") + hipGetErrorString(e); return IODINE_ERR_HIP; }
    return IODINE_OK;
}

int iodine_op_render_bwd(void* stream, const float* dec_out, const float* g_pred, const float* g_mask, const float* g_mean, float* g_out,
                         int batch, int slots, int pixels, int strict)
{
    hipStream_t st = (hipStream_t)stream;
    if (!dec_out || !g_out || batch < 1 || slots < 1 || slots > 16 || pixels < 1) { g_create_error = "iodine_op_render_bwd: argument"; return IODINE_ERR_INVALID; }
    hipError_t e = launch_render_bwd(st, dec_out, g_pred, g_mask, g_mean, g_out, batch, slots, pixels, strict ? 1 : 0);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { g_create_error = std::string("iodine_op_render_bwd: ") + hipGetErrorString(e); return IODINE_ERR_HIP; }
    return IODINE_OK;
}

int iodine_op_render_bwd_logits(void* stream, const float* dec_out, const float* g_pred, const float* g_mask, const float* g_mean,
                                const float* g_logits, float* g_out, int batch, int slots, int pixels, int strict)
{
    hipStream_t st = (hipStream_t)stream;
    if (!dec_out || !g_out || batch < 1 || slots < 1 || slots > 16 || pixels < 1) { g_create_error = "iodine_op_render_bwd_logits: argument"; return IODINE_ERR_INVALID; }
    hipError_t e = launch_render_bwd_logits(st, dec_out, g_pred, g_mask, g_mean, g_logits, g_out, batch, slots, pixels, strict ? 1 : 0);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { g_create_error = std::string("iodine_op_render_bwd_logits: ") + hipGetErrorString(e); return IODINE_ERR_HIP; }
    return IODINE_OK;
}

int iodine_op_pixel_maps(void* stream, const float* x_nchw, const float* w_or_null, const float* dec_out_nhwc4, int batch, int slots,
                         int pixels, float sigma, int strict, float coef, float* ll, float* kll, float* gx, float* gw, int first)
{
    hipStream_t st = (hipStream_t)stream;
    if (!x_nchw || !dec_out_nhwc4 || batch < 1 || slots < 1 || slots > 16 || pixels < 1 || !(sigma > 0.f) ||
        (size_t)batch * slots * pixels >= ((size_t)1 << 31)) {
        g_create_error = "iodine_op_pixel_maps: argument";
        return IODINE_ERR_INVALID;
    }
    float* x4 = nullptr;
    if (hipMalloc((void**)&x4, (size_t)batch * pixels * 4 * sizeof(float)) != hipSuccess) return IODINE_ERR_HIP;
    hipError_t e = launch_x_to_nhwc4(st, x_nchw, x4, batch, pixels, 1, w_or_null, 0);
    const int st_ = strict & 1, joint = (strict >> 1) & 1;                 // the flag word: bit 0 strict, bit 1 joint_likelihood
    if (e == hipSuccess) e = launch_pixel_like_maps(st, x4, dec_out_nhwc4, ll, kll, batch, slots, pixels, sigma, st_, joint);
    if (e == hipSuccess)
        e = launch_pixel_input_grad(st, x4, dec_out_nhwc4, gx, (size_t)3 * pixels, gw, (size_t)pixels, batch, slots, pixels, sigma, st_,
                                    coef, first ? 1 : 0, first ? 1 : 0, joint);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    (void)hipFree(x4);
    if (e != hipSuccess) { g_create_error = std::string("iodine_op_pixel_maps: ") + hipGetErrorString(e); return IODINE_ERR_HIP; }
    return IODINE_OK;
}

// the per-pixel mixture kernels of one ELBO evaluation, kernel-level (tests/test_gpu_pixel.py): the production launchers in the order
// elbo_and_gradients / refine_step / iodine_reconstruct run them.  (kernel-level tests only: allocates, synchronises and frees per call)
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
    if (!ok) {
        g_create_error = "iodine_op_pixel_encode: argument (x, dec_out, pm, plv, lin and out[0..4] required; batch, size, latent, repeat >= 1; slots "
                         "in 1..16; sigma > 0; enc_sh only with enc; batch * slots * size^2 * 20 and batch * slots * latent below 2^31)";
        return IODINE_ERR_INVALID;
    }
    float *g = out[0], *lnstat = out[1], *ll_img = out[2], *img_terms = out[3], *scal = out[4], *sgrad = out[5], *enc = out[6], *enc_sh = out[7];
    const int Pi = (int)P, strict = flags & 1, use_ln = (flags >> 1) & 1, stable = (flags >> 2) & 1, joint = (flags >> 3) & 1;
    const size_t nblk = (size_t)pixel_blocks_per_image(Pi);
    // [x4: B P float4][part: B nblk (6 K + 3) doubles][sg_part: B nblk doubles][counter: one word, 16 bytes]
    const size_t x4_bytes = B * P * 4 * sizeof(float), part_bytes = B * nblk * (6 * K + 3) * sizeof(double), sg_bytes = B * nblk * sizeof(double);
    char* buf = nullptr;
    if (hipMalloc((void**)&buf, x4_bytes + part_bytes + sg_bytes + 16) != hipSuccess) return IODINE_ERR_HIP;
    float* x4 = (float*)buf;
    double *part = (double*)(buf + x4_bytes), *sg_part = (double*)(buf + x4_bytes + part_bytes);
    unsigned* counter = (unsigned*)(buf + x4_bytes + part_bytes + sg_bytes);
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
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    (void)hipFree(buf);
    if (e != hipSuccess) { g_create_error = std::string("iodine_op_pixel_encode: ") + hipGetErrorString(e); return IODINE_ERR_HIP; }
    return IODINE_OK;
}

int iodine_op_conv3x3_wgrad_f32(void* stream, const float* in, const float* d, float* gw, float* gb, int n, int s, int c)
{
    hipStream_t st = (hipStream_t)stream;
    const size_t part_elems = (size_t)512 * 4 * 9 * 32 * 32, fold_elems = (size_t)WGRAD_FOLD * 9 * 64 * 64;
    float* buf = nullptr;
    if (hipMalloc((void**)&buf, (part_elems + fold_elems + (size_t)512 * 64) * sizeof(float)) != hipSuccess) return IODINE_ERR_HIP;
    float *part = buf, *fold = buf + part_elems, *part_b = fold + fold_elems;
    int nparts = 0, cop = 0, nb = 0;
    hipError_t e;
    if (c < 0) {                                    // the output conv |c| -> 4 in GEMM form (d has 4 channels; gw [4][|c|][3][3], gb [4])
        c = -c;
        e = launch_dec_out_wgrad_f32(st, in, d, part, part_b, n, s, c, &nparts, &nb);
        if (e == hipSuccess) e = launch_wgrad_reduce(st, part, nparts, c, 4, 4, c, c, 1.f, gw, fold);
        if (e == hipSuccess) e = launch_colsum(st, part_b, nb, 4, 4, 1.f, gb);
    } else {
    e = launch_conv3x3_wgrad_f32_ws(st, in, d, part, part_b, n, s, c, &nparts, &cop, &nb);
    if (e == hipSuccess) e = launch_wgrad_reduce(st, part, nparts, c, cop, c, c, c, 1.f, gw, fold);
    if (e == hipSuccess) e = launch_colsum(st, part_b, nb, c, c, 1.f, gb);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    (void)hipFree(buf);
    if (e != hipSuccess) { g_create_error = std::string("iodine_op_conv3x3_wgrad_f32: ") + hipGetErrorString(e); return IODINE_ERR_HIP; }
    return IODINE_OK;
}

// ---- the refinement head and its backward, kernel-level (tests/test_gpu_head.py, tests/test_gpu_sgemm.py) --------------------------------
// (kernel-level tests only: these allocate and free their scratch around the launches and synchronise - not entry points to time)
static int op_fail(const char* who, hipError_t e)
{
    g_create_error = std::string(who) + ": " + hipGetErrorString(e);
    return IODINE_ERR_HIP;
}

int iodine_op_sgemm(void* stream, int form, int ta, int tb, int M, int N, int K, float alpha, const float* A, int lda, const float* B, int ldb,
                    float beta, float* Cm, int ldc, int mode_c)
{
    hipStream_t st = (hipStream_t)stream;
    if (form < 0 || form > 3 || M < 1 || N < 1 || K < 1 || !A || !B || !Cm || lda < 1 || ldb < 1 || ldc < 1) {
        g_create_error = "iodine_op_sgemm: argument";
        return IODINE_ERR_INVALID;
    }
    hipError_t e;
    if (form == 0) {
        if (lda < (ta ? M : K) || ldb < (tb ? K : N) || ldc < N) { g_create_error = "iodine_op_sgemm: leading dimension"; return IODINE_ERR_INVALID; }
        e = launch_sgemm(st, ta, tb, M, N, K, alpha, A, lda, B, ldb, beta, Cm, ldc);
    } else {
        // A [K][M] (form 2: [M][K] row-major), B [K][N]; form 3 writes through the broadcast layer's map: N = 9 mode_c, ldc = L + 2 >= M
        const bool bad = !sgemm_tn_mfma_ok(M, N, K) || lda < (form == 2 ? K : M) || ldb < N ||
                         (form == 3 ? (mode_c < 1 || N != 9 * mode_c || ldc < M) : ldc < N);
        if (bad) { g_create_error = "iodine_op_sgemm: shape not covered by the MFMA form (M, N multiples of 32; form 3: N = 9 mode_c, ldc >= M)"; return IODINE_ERR_INVALID; }
        e = launch_sgemm_tn_mfma(st, M, N, K, alpha, A, lda, B, ldb, beta, Cm, ldc, form == 3 ? 1 : 0, form == 3 ? mode_c : 0, form == 2 ? 1 : 0);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return op_fail("iodine_op_sgemm", e);
    return IODINE_OK;
}

int iodine_op_colsum(void* stream, int form, const float* src, int rows, int cols, int ld, float alpha, float* dst)
{
    hipStream_t st = (hipStream_t)stream;
    if (form < 0 || form > 1 || !src || !dst || rows < 1 || cols < 1 || ld < cols) { g_create_error = "iodine_op_colsum: argument"; return IODINE_ERR_INVALID; }
    hipError_t e;
    if (form == 0) {
        e = launch_colsum(st, src, rows, cols, ld, alpha, dst);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
    } else {
        // the streaming form, only where launch_colsum_tall itself takes it (elsewhere it forwards to launch_colsum = form 0)
        if (ld != cols || cols % 4 != 0 || cols > 256 || 256 % (cols / 4) != 0 || rows < 8192) {
            g_create_error = "iodine_op_colsum: the tall form takes contiguous rows >= 8192, cols a multiple of 4 with 256 % (cols / 4) == 0";
            return IODINE_ERR_INVALID;
        }
        const size_t tmp_elems = (size_t)512 * 64;                       // (the library's partial-bias scratch)
        float* tmp = nullptr;
        if (hipMalloc((void**)&tmp, tmp_elems * sizeof(float)) != hipSuccess) return IODINE_ERR_HIP;
        e = launch_colsum_tall(st, src, rows, cols, alpha, dst, tmp, tmp_elems);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        (void)hipFree(tmp);
    }
    if (e != hipSuccess) return op_fail("iodine_op_colsum", e);
    return IODINE_OK;
}

int iodine_op_refine_head(void* stream, int form, const float* const* in, float* const* out, int N, int PL, int C, int H, int L)
{
    hipStream_t st = (hipStream_t)stream;
    bool ok = in && out && (form == 0 || form == 1) && N >= 1 && PL >= 1 && C >= 4 && C <= 256 && 256 % C == 0 && H >= 4 && H <= 1024 && H % 4 == 0 &&
              L >= 4 && L <= 256 && L % 4 == 0;
    for (int j = 0; ok && j < 14; ++j) ok = in[j] != nullptr;
    for (int j = 0; ok && j < 4; ++j) ok = out[j] != nullptr;              // (h, c, pm, plv; the rest optional)
    if (!ok) { g_create_error = "iodine_op_refine_head: argument"; return IODINE_ERR_INVALID; }
    if (form == 0 ? refine_head_lds_bytes(C, H, L, 0) > 96 * 1024 : refine_head_form(C, H, L, 1) != 1) {
        g_create_error = form == 0 ? "iodine_op_refine_head: the single-launch form does not fit the LDS at these widths"
                                   : "iodine_op_refine_head: the three-launch form needs 4 * MLP_UNITS to be a multiple of 32";
        return IODINE_ERR_INVALID;
    }
    const float *mlp_w = in[0], *mlp_b = in[1], *wih = in[2], *whh = in[3], *bih = in[4], *bhh = in[5], *wm = in[6], *bm = in[7], *wv = in[8],
                *bv = in[9], *feat = in[10], *latent = in[11], *h_prev = in[12], *c_prev = in[13];
    const size_t IN = (size_t)H + 4 * L, Kg = IN + H, Np = ((size_t)N + 31) / 32 * 32;
    const size_t n_mlp = (size_t)C * H, n_w = Kg * 4 * H, n_b = (size_t)4 * H, n_u = (size_t)H * L, n_xh = form == 1 ? Np * Kg : 0,
                 n_gp = form == 1 ? Np * 4 * H : 0;
    float* buf = nullptr;
    if (hipMalloc((void**)&buf, (n_mlp + n_w + n_b + 2 * n_u + n_xh + n_gp) * sizeof(float)) != hipSuccess) return IODINE_ERR_HIP;
    float *mlp_wT = buf, *wihT = mlp_wT + n_mlp, *whhT = wihT + IN * 4 * H, *lstm_b = wihT + n_w, *wmT = lstm_b + n_b, *wvT = wmT + n_u,
          *xh = wvT + n_u, *gp = xh + n_xh;
    // the operands as iodine_set_params builds them: transposes to [in][out], [W_ih^T ; W_hh^T] back to back, b_ih + b_hh
    MultiCopy mc;
    mc.count = 0;
    auto queue = [&](float* dst, const float* src, const float* src2, size_t n, int op, int cols) {
        mc.src[mc.count] = src; mc.src2[mc.count] = src2; mc.dst[mc.count] = dst; mc.n[mc.count] = (int)n; mc.op[mc.count] = op;
        mc.cols[mc.count] = cols; ++mc.count;
    };
    queue(mlp_wT, mlp_w, nullptr, n_mlp, 1, C);
    queue(wihT, wih, nullptr, IN * 4 * H, 1, (int)IN);
    queue(whhT, whh, nullptr, (size_t)H * 4 * H, 1, H);
    queue(lstm_b, bih, bhh, n_b, 2, 0);
    queue(wmT, wm, nullptr, n_u, 1, H);
    queue(wvT, wv, nullptr, n_u, 1, H);
    hipError_t e = launch_multi_copy(st, mc);
    if (e == hipSuccess && form == 1) e = launch_zero_fill(st, xh, n_xh + n_gp);      // (rows N .. Np of the gate GEMM: the workspace's are finite too)
    if (e == hipSuccess)
        e = launch_refine_head(st, feat, N, PL, C, H, L, mlp_wT, mlp_b, wihT, whhT, lstm_b, wmT, bm, wvT, bv, latent, h_prev, c_prev, out[0], out[1],
                               out[2], out[3], out[6], out[7], out[8], out[9], out[4], out[5], form == 1 ? xh : nullptr, form == 1 ? gp : nullptr, 1);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    (void)hipFree(buf);
    if (e != hipSuccess) return op_fail("iodine_op_refine_head", e);
    return IODINE_OK;
}

int iodine_op_head_bptt(void* stream, int form, const float* const* in, float* const* out, int T, int N, int B, int L, int H, int Cr,
                        long long seed_stride)
{
    hipStream_t st = (hipStream_t)stream;
    bool ok = in && out && (form == 0 || form == 1) && T >= 1 && N >= 1 && B >= 1 && L >= 1 && H >= 1 && Cr >= 1 && seed_stride >= 0;
    for (int j = 0; ok && j < 10; ++j) ok = in[j] != nullptr;
    for (int j = 0; ok && j < 5; ++j) ok = out[j] != nullptr;
    if (!ok) { g_create_error = "iodine_op_head_bptt: argument"; return IODINE_ERR_INVALID; }
    const float *seed_m = in[10], *seed_v = in[11], *gl = in[12], *wtab = in[13], *dh_in = in[14], *dc_in = in[15];
    if ((seed_m == nullptr) != (seed_v == nullptr) || (!seed_m && (gl || dh_in || dc_in || out[5] || out[6] || seed_stride))) {
        g_create_error = "iodine_op_head_bptt: gl, the carries and seed_stride belong to the seeded form (seed_m and seed_v given)";
        return IODINE_ERR_INVALID;
    }
    hipError_t e;
    if (form == 0) {
        if (!head_bptt_fits(L, H, Cr)) {
            g_create_error = "iodine_op_head_bptt: the fused kernel takes Cr <= H, and L, H, Cr multiples of 4";
            return IODINE_ERR_INVALID;
        }
        e = launch_head_bptt(st, in[0], in[1], in[2], in[3], in[4], in[5], in[6], in[7], in[8], in[9], out[0], out[1], out[2], out[3], out[4],
                             T, N, B, L, H, Cr, seed_m, seed_v, gl, wtab, dh_in, dc_in, out[5], out[6], (size_t)seed_stride);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
    } else {
        std::vector<float> whost;
        if (wtab) {                                                      // the launch sequence takes the loss weights from the host
            whost.resize((size_t)T + 1);
            e = hipMemcpyAsync(whost.data(), wtab, sizeof(float) * ((size_t)T + 1), hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            if (e != hipSuccess) return op_fail("iodine_op_head_bptt", e);
        }
        const size_t NH = (size_t)N * H;
        float* buf = nullptr;
        if (hipMalloc((void**)&buf, 6 * NH * sizeof(float)) != hipSuccess) return IODINE_ERR_HIP;
        float* const ch[2] = {buf + 2 * NH, buf + 3 * NH};
        float* const cc[2] = {buf + 4 * NH, buf + 5 * NH};
        e = launch_head_bptt_unfused(st, in[0], in[1], in[2], in[3], in[4], in[5], in[6], in[7], in[8], in[9], out[0], out[1], out[2], out[3], out[4],
                                     T, N, B, L, H, Cr, seed_m != nullptr, seed_m, seed_v, gl, wtab ? whost.data() : nullptr, dh_in, dc_in, out[5],
                                     out[6], (size_t)seed_stride, buf, buf + NH, ch, cc);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        (void)hipFree(buf);
    }
    if (e != hipSuccess) return op_fail("iodine_op_head_bptt", e);
    return IODINE_OK;
}

int iodine_op_pool_bwd(void* stream, const float* dpooled, const float* act, float* dpre, int N, int PL, int C)
{
    hipStream_t st = (hipStream_t)stream;
    if (!dpooled || !act || !dpre || N < 1 || PL < 1 || C < 1) { g_create_error = "iodine_op_pool_bwd: argument"; return IODINE_ERR_INVALID; }
    hipError_t e = launch_pool_bwd(st, dpooled, act, dpre, N, PL, C);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return op_fail("iodine_op_pool_bwd", e);
    return IODINE_OK;
}

int iodine_op_refine_head_form(int C, int H, int L, int prefer_split) { return refine_head_form(C, H, L, prefer_split); }

}  // extern "C"
