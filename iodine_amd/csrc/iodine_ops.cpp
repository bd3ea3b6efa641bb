// The product's handle-free entry points of libiodine_hip.so: the optimizer and metric launches, object tables, restarts, matching,
// resident data, the Philox sampler and the host linspace.  Each refuses with free_fail and ends its launch with free_hip
// (iodine_internal.h).  The kernel-test entries (iodine_op_*) are in iodine_testops.cpp.  See include/iodine_hip.h.
#include "iodine_internal.h"
#include "assign.h"
#include "components_host.h"

extern "C" {

int iodine_adam_step(void* stream, const long long* ptrs_dev, const long long* offsets_dev, int n_tensors, long long total,
                     double lr, double beta1, double beta2, double eps, double weight_decay, int step)
{
    if (!ptrs_dev || !offsets_dev || n_tensors < 1 || total < 1 || step < 1) return free_fail(IODINE_ERR_INVALID, "iodine_adam_step: bad argument");
    return free_hip("iodine_adam_step", launch_adam_multi((hipStream_t)stream, ptrs_dev, offsets_dev, n_tensors, total, lr, beta1, beta2, eps,
                                           weight_decay, step));
}

size_t iodine_grad_norm_scratch_bytes(long long total) { return total < 1 ? 0 : grad_norm_scratch_bytes(total); }

int iodine_grad_norm(void* stream, const long long* ptrs_dev, const long long* offsets_dev, int n_tensors, long long total,
                     double max_norm, void* scratch_dev, size_t scratch_bytes, float* out4_dev)
{
    if (!ptrs_dev || !offsets_dev || n_tensors < 1 || total < 1 || !scratch_dev || !out4_dev || !(max_norm > 0.0) ||
        scratch_bytes < grad_norm_scratch_bytes(total) || ((uintptr_t)scratch_dev & 7))
        return free_fail(IODINE_ERR_INVALID, "iodine_grad_norm: bad argument (max_norm must be > 0; scratch of iodine_grad_norm_scratch_bytes, 8-byte aligned)");
    return free_hip("iodine_grad_norm", launch_grad_norm((hipStream_t)stream, ptrs_dev, offsets_dev, n_tensors, total, max_norm,
                                          (double*)scratch_dev, out4_dev));
}

int iodine_grad_scale(void* stream, const long long* ptrs_dev, const long long* offsets_dev, int n_tensors, long long total,
                      const float* coef_dev)
{
    if (!ptrs_dev || !offsets_dev || n_tensors < 1 || total < 1 || !coef_dev) return free_fail(IODINE_ERR_INVALID, "iodine_grad_scale: bad argument");
    return free_hip("iodine_grad_scale", launch_grad_scale((hipStream_t)stream, ptrs_dev, offsets_dev, n_tensors, total, coef_dev));
}

int iodine_adam_step_clipped(void* stream, const long long* ptrs_dev, const long long* offsets_dev, int n_tensors, long long total,
                             double lr, double beta1, double beta2, double eps, double weight_decay, int step,
                             const float* out4_dev, int skip_nonfinite)
{
    if (!ptrs_dev || !offsets_dev || n_tensors < 1 || total < 1 || step < 1 || !out4_dev) return free_fail(IODINE_ERR_INVALID, "iodine_adam_step_clipped: bad argument");
    return free_hip("iodine_adam_step_clipped", launch_adam_multi((hipStream_t)stream, ptrs_dev, offsets_dev, n_tensors, total, lr, beta1, beta2, eps,
                                           weight_decay, step, out4_dev, skip_nonfinite ? 1 : 0));
}

int iodine_ari_table(void* stream, const float* mask, const unsigned char* gt, int batch, int slots, int n_gt, int pixels,
                     int* table)
{
    if (!mask || !gt || !table || batch < 1 || slots < 1 || n_gt < 1 || pixels < 1 || (size_t)n_gt * slots > 8192) return free_fail(IODINE_ERR_INVALID, "iodine_ari_table: bad argument");
    return free_hip("iodine_ari_table", launch_ari_table((hipStream_t)stream, mask, gt, batch, slots, n_gt, pixels, table));
}

int iodine_slot_table(void* stream, const float* mask, const float* mean_or_null, int batch, int slots, int size,
                      float* table, unsigned char* seg_or_null)
{
    if (!mask || !table || batch < 1 || slots < 1 || slots > 16 || size < 1 || size > 1024)
        return free_fail(IODINE_ERR_INVALID, "iodine_slot_table: bad argument (mask and table required, batch >= 1, slots in 1..16, size in 1..1024)");
    return free_hip("iodine_slot_table", launch_slot_table((hipStream_t)stream, mask, mean_or_null, batch, slots, size, table, seg_or_null));
}

int iodine_seg_overlap(void* stream, const unsigned char* seg_a, const unsigned char* seg_b, int batch, int slots_a, int slots_b,
                       int pixels, int* table)
{
    if (!seg_a || !seg_b || !table || batch < 1 || slots_a < 1 || slots_a > 16 || slots_b < 1 || slots_b > 16 || pixels < 1 ||
        pixels > 1024 * 1024)
        return free_fail(IODINE_ERR_INVALID, "iodine_seg_overlap: bad argument (three pointers required, batch >= 1, slots_a / slots_b in 1..16, pixels in 1..1024^2)");
    return free_hip("iodine_seg_overlap", launch_seg_overlap((hipStream_t)stream, seg_a, seg_b, batch, slots_a, slots_b, pixels, table));
}

size_t iodine_seg_components_scratch_bytes(int batch, int size)
{
    return batch < 1 || size < 1 || size > 1024 ? 0 : seg_components_scratch_bytes(batch, size);
}

// what both component entries refuse (batch and scratch are the device entry's own)
static const char* seg_components_bad(const unsigned char* seg, int slots, int size, int connectivity, int min_area, int max_components,
                                      const int* labels, const int* count, const int* table)
{
    return !seg ? "seg is NULL" : !labels ? "labels is NULL" : !count ? "count is NULL"
        : (slots < 1 || slots > 16) ? "slots must be in 1..16" : (size < 1 || size > 1024) ? "size must be in 1..1024"
        : (connectivity != 4 && connectivity != 8) ? "connectivity must be 4 or 8" : min_area < 1 ? "min_area must be >= 1"
        : (table && max_components < 1) ? "max_components must be >= 1 with a table" : max_components < 0 ? "max_components must be >= 0"
        : nullptr;
}

int iodine_seg_components(void* stream, const unsigned char* seg, int batch, int slots, int size, int connectivity, int min_area,
                          int max_components, int* labels, int* area_map_or_null, int* count, int* per_slot_or_null,
                          int* table_or_null, unsigned char* clean_or_null, void* scratch, size_t scratch_bytes)
{
    const char* bad = seg_components_bad(seg, slots, size, connectivity, min_area, max_components, labels, count, table_or_null);
    if (!bad)
        bad = (batch < 1 || batch > 65535) ? "batch must be in 1..65535" : !scratch ? "scratch is NULL"
            : scratch_bytes < seg_components_scratch_bytes(batch, size) ? "scratch is smaller than iodine_seg_components_scratch_bytes" : nullptr;
    if (bad) return free_fail(IODINE_ERR_INVALID, std::string("iodine_seg_components: ") + bad);
    return free_hip("iodine_seg_components", launch_seg_components((hipStream_t)stream, seg, batch, slots, size, connectivity, min_area,
                                                                   max_components, labels, area_map_or_null, count, per_slot_or_null,
                                                                   table_or_null, clean_or_null, scratch));
}

int iodine_seg_components_host(const unsigned char* seg, int slots, int size, int connectivity, int min_area, int max_components,
                               int* labels, int* area_map_or_null, int* count, int* per_slot_or_null, int* table_or_null,
                               unsigned char* clean_or_null)
{
    if (const char* bad = seg_components_bad(seg, slots, size, connectivity, min_area, max_components, labels, count, table_or_null))
        return free_fail(IODINE_ERR_INVALID, std::string("iodine_seg_components_host: ") + bad);
    iod_components_host(seg, slots, size, connectivity, min_area, max_components, labels, area_map_or_null, count, per_slot_or_null,
                        table_or_null, clean_or_null);
    return IODINE_OK;
}

int iodine_chain_score(void* stream, const float* x, const float* w_or_null, const float* mask, const float* mean, int chains, int batch,
                       int slots, int size, double sigma, int joint, float* ll_or_null, unsigned char* seg_or_null)
{
    const char* bad = !x ? "x is NULL" : !mask ? "mask is NULL" : !mean ? "mean is NULL"
        : (chains < 1 || chains > 1024) ? "chains must be in 1..1024" : batch < 1 ? "batch must be >= 1"
        : (long long)chains * batch > 0x7fffffffLL ? "chains * batch must be below 2^31"
        : (slots < 1 || slots > 16) ? "slots must be in 1..16" : (size < 1 || size > 1024) ? "size must be in 1..1024"
        : !(sigma > 0.0) ? "sigma must be > 0" : (joint != 0 && joint != 1) ? "joint must be 0 (per channel) or 1 (joint over RGB)"
        : (!ll_or_null && !seg_or_null) ? "ll_or_null and seg_or_null are both NULL: nothing to compute" : nullptr;
    if (bad) return free_fail(IODINE_ERR_INVALID, std::string("iodine_chain_score: ") + bad);
    return free_hip("iodine_chain_score", launch_chain_score((hipStream_t)stream, x, w_or_null, mask, mean, chains, batch, slots, size, sigma,
                                                             joint, ll_or_null, seg_or_null));
}

int iodine_chain_consensus(void* stream, const unsigned char* seg, const int* perm, const int* ref_or_null, const float* mask_or_null,
                           int chains, int batch, int slots, int size, int* votes_or_null, unsigned char* consensus_or_null,
                           float* agreement_or_null, float* match_or_null, float* mask_mean_or_null)
{
    const char* bad = !seg ? "seg is NULL" : !perm ? "perm is NULL"
        : (chains < 1 || chains > 1024) ? "chains must be in 1..1024" : batch < 1 ? "batch must be >= 1"
        : (long long)chains * batch > 0x7fffffffLL ? "chains * batch must be below 2^31"
        : (slots < 1 || slots > 16) ? "slots must be in 1..16" : (size < 1 || size > 1024) ? "size must be in 1..1024"
        : (match_or_null && !ref_or_null) ? "match needs ref, which is NULL"
        : (mask_mean_or_null && !mask_or_null) ? "mask_mean needs mask, which is NULL"
        : (!votes_or_null && !consensus_or_null && !agreement_or_null && !match_or_null && !mask_mean_or_null)
              ? "votes, consensus, agreement, match and mask_mean are all NULL: nothing to compute" : nullptr;
    if (bad) return free_fail(IODINE_ERR_INVALID, std::string("iodine_chain_consensus: ") + bad);
    return free_hip("iodine_chain_consensus", launch_chain_consensus((hipStream_t)stream, seg, perm, ref_or_null, mask_or_null, chains, batch, slots,
                                                                     size, votes_or_null, consensus_or_null, agreement_or_null, match_or_null,
                                                                     mask_mean_or_null));
}

int iodine_mask_overlap(void* stream, const float* mask, const unsigned char* gt, int batch, int slots, int n_gt, int size, float eps,
                        float* inter, float* nll_or_null, float* mask_area, int* gt_area)
{
    if (!mask || !gt || !inter || !mask_area || !gt_area || batch < 1 || slots < 1 || slots > 16 || n_gt < 1 || n_gt > 16 || size < 1 ||
        size > 1024 || !(eps > 0.f))
        return free_fail(IODINE_ERR_INVALID, "iodine_mask_overlap: bad argument (mask, gt, inter, mask_area, gt_area required, batch >= 1, slots and n_gt in 1..16, "
                         "size in 1..1024, eps > 0)");
    return free_hip("iodine_mask_overlap", launch_mask_overlap((hipStream_t)stream, mask, gt, batch, slots, n_gt, size, eps, inter, nll_or_null, mask_area,
                                             gt_area));
}

int iodine_assign(void* stream, const float* cost, const unsigned char* row_valid_or_null, int batch, int n_rows, int n_cols,
                  int* assign, float* total)
{
    if (!cost || !assign || !total || batch < 1 || n_rows < 1 || n_rows > 16 || n_cols < 1 || n_cols > 16)
        return free_fail(IODINE_ERR_INVALID, "iodine_assign: bad argument (cost, assign, total required, batch >= 1, n_rows and n_cols in 1..16)");
    return free_hip("iodine_assign", launch_assign((hipStream_t)stream, cost, row_valid_or_null, batch, n_rows, n_cols, assign, total));
}

int iodine_assign_host(const float* cost, const unsigned char* row_valid_or_null, int n_rows, int n_cols, int* assign, float* total)
{
    if (!cost || !assign || !total || n_rows < 1 || n_rows > 16 || n_cols < 1 || n_cols > 16)
        return free_fail(IODINE_ERR_INVALID, "iodine_assign_host: bad argument (cost, assign, total required, n_rows and n_cols in 1..16)");
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
        !kinds || ((match_kind == 1 || loss_kind == 1) && !nll_or_null))
        return free_fail(IODINE_ERR_INVALID, "iodine_mask_match: bad argument (inter, mask_area, gt_area, assign, loss, coef required, batch >= 1, slots and n_gt in "
                         "1..16, kinds 0 = iou / 1 = ce, and nll with either kind 1)");
    return free_hip("iodine_mask_match", launch_mask_match((hipStream_t)stream, inter, nll_or_null, mask_area, gt_area, batch, slots, n_gt, match_kind,
                                           loss_kind, assign, loss, coef, cost_or_null, iou_or_null));
}

int iodine_mask_match_backward(void* stream, const float* mask, const unsigned char* gt, const int* assign, const float* coef,
                               const float* grad_loss, int batch, int slots, int n_gt, int size, int loss_kind, float eps,
                               float* grad_mask)
{
    if (!mask || !gt || !assign || !coef || !grad_loss || !grad_mask || batch < 1 || slots < 1 || slots > 16 || n_gt < 1 || n_gt > 16 ||
        size < 1 || size > 1024 || (loss_kind != 0 && loss_kind != 1) || !(eps > 0.f))
        return free_fail(IODINE_ERR_INVALID, "iodine_mask_match_backward: bad argument (six pointers required, batch >= 1, slots and n_gt in 1..16, size in 1..1024, "
                         "loss_kind 0 = iou / 1 = ce, eps > 0)");
    return free_hip("iodine_mask_match_backward", launch_mask_match_bwd((hipStream_t)stream, mask, gt, assign, coef, grad_loss, batch, slots, n_gt, size, loss_kind,
                                               eps, grad_mask));
}

int iodine_batch_gather(void* stream, const long long* index, int count, const void* images, int image_kind,
                        const unsigned short* masks_or_null, int size, int planes, float* x, unsigned char* gt_or_null)
{
    if (!index || !images || !x || count < 1 || size < 1 || size > 4096 || planes < 1 || planes > 16 || (image_kind != 0 && image_kind != 1))
        return free_fail(IODINE_ERR_INVALID, "iodine_batch_gather: bad argument (index, images, x required, count >= 1, size in 1..4096, planes in 1..16, "
                         "image_kind 0 = uint8 HWC / 1 = float32 CHW)");
    return free_hip("iodine_batch_gather", launch_batch_gather((hipStream_t)stream, index, count, images, image_kind, masks_or_null, size, planes, x, gt_or_null));
}

int iodine_batch_window(void* stream, const long long* index, int count, const void* images, int image_kind,
                        const unsigned short* masks_or_null, int src_h, int src_w, const float* windows, int size, int planes, float* x,
                        unsigned char* gt_or_null)
{
    if (!index || !images || !windows || !x || count < 1 || src_h < 1 || src_h > 4096 || src_w < 1 || src_w > 4096 || size < 1 || size > 512 ||
        planes < 1 || planes > 16 || (image_kind != 0 && image_kind != 1))
        return free_fail(IODINE_ERR_INVALID, "iodine_batch_window: bad argument (index, images, windows, x required, count >= 1, src_h and src_w in "
                         "1..4096, size in 1..512, planes in 1..16, image_kind 0 = uint8 HWC / 1 = float32 CHW)");
    return free_hip("iodine_batch_window", launch_batch_window((hipStream_t)stream, index, count, images, image_kind, masks_or_null, src_h, src_w,
                                                               windows, size, planes, x, gt_or_null));
}

int iodine_synth_scenes(void* stream, int n, int size, unsigned long long seed, unsigned long long seed_step, unsigned long long stream_id,
                        unsigned long long stream_step, int kind, int max_objects, int frames, float* images,
                        unsigned short* masks_or_null, unsigned char* n_gt_or_null)
{
    if (!images || n < 1 || size < 1 || size > 1024 || (kind != 0 && kind != 1) || max_objects < 1 || max_objects > 16 || frames < 0 ||
        (long long)n * (frames > 0 ? frames : 1) > 0x7FFFFFFFll)
        return free_fail(IODINE_ERR_INVALID, "iodine_synth_scenes: bad argument (images required, n >= 1, size in 1..1024, kind 0 = uniform / 1 = blobs, "
                         "max_objects in 1..16, frames >= 0, n * frames < 2^31)");
    return free_hip("iodine_synth_scenes", launch_synth_scenes((hipStream_t)stream, n, size, seed, seed_step, stream_id, stream_step, kind, max_objects, frames,
                                             images, masks_or_null, n_gt_or_null));
}

int iodine_randn(void* stream, float* out, long long n, unsigned long long seed, unsigned long long stream_id)
{
    if (!out || n < 1) return free_fail(IODINE_ERR_INVALID, "iodine_randn: bad argument");
    return free_hip("iodine_randn", launch_randn_philox((hipStream_t)stream, out, n, seed, stream_id));
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

}  // extern "C"
