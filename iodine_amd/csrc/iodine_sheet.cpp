// Decomposition sheets: the argument checks and the launch of iodine_render_sheet, the size and form queries.  See include/iodine_hip.h.
#include "iodine_internal.h"

namespace {

// H and W of the sheet in 64 bits; the caller has checked the ranges of the terms
void sheet_dims(const iodine_sheet_spec& sp, long long& H, long long& W)
{
    const long long cw = (long long)sp.size * sp.scale + sp.pad;
    H = sp.pad + sp.rows * cw;
    W = sp.pad + sp.n_panels * cw;
}

// why the sizes and the panel list cannot be drawn ("" = they can); no pointer is looked at
std::string sheet_spec_error(const iodine_sheet_spec* sp)
{
    if (!sp) return "spec is NULL";
    if (sp->rows < 1) return "rows must be >= 1";
    if (sp->slots < 1 || sp->slots > 16) return "slots must be in 1..16";
    if (sp->n_gt < 0 || sp->n_gt > 16) return "n_gt must be in 0..16";
    if (sp->size < 1 || sp->size > 1024) return "size must be in 1..1024";
    if (sp->scale < 1 || sp->scale > 8) return "scale must be in 1..8";
    if (sp->pad < 0 || sp->pad > 16) return "pad must be in 0..16";
    if (sp->n_panels < 1 || sp->n_panels > IODINE_SHEET_MAX_PANELS) return "n_panels must be in 1..64";
    for (int c = 0; c < sp->n_panels; ++c) {
        const int kind = sp->panel_kind[c];
        if (kind > IODINE_SHEET_SLOT_MASK) return "panel " + std::to_string(c) + ": unknown kind " + std::to_string(kind);
        if (kind >= IODINE_SHEET_SLOT_MASKED && sp->panel_slot[c] >= sp->slots)
            return "panel " + std::to_string(c) + ": slot " + std::to_string((int)sp->panel_slot[c]) + " outside 0.." + std::to_string(sp->slots - 1);
    }
    long long H, W;
    sheet_dims(*sp, H, W);
    if (H * W * 3 >= (1ll << 31)) return "the sheet has 2^31 bytes or more (the kernel indexes it in 32 bits)";
    return "";
}

// spec_error plus the pointers: mask and sheet always, the inputs of every panel in the list
std::string sheet_call_error(const iodine_sheet_spec* sp, const float* x, const float* pred, const float* mask, const float* mean,
                             const unsigned char* gt, const unsigned char* sheet)
{
    std::string why = sheet_spec_error(sp);
    if (!why.empty()) return why;
    if (!mask) return "mask is NULL";
    if (!sheet) return "sheet is NULL";
    for (int c = 0; c < sp->n_panels; ++c) {
        const int kind = sp->panel_kind[c];
        const bool need_x = kind == IODINE_SHEET_IMAGE || kind == IODINE_SHEET_OVERLAY || kind == IODINE_SHEET_ERROR;
        const bool need_pred = kind == IODINE_SHEET_PRED || kind == IODINE_SHEET_ERROR;
        const bool need_mean = kind == IODINE_SHEET_SLOT_MASKED || kind == IODINE_SHEET_SLOT_MEAN;
        const char* missing = need_x && !x ? "x" : need_pred && !pred ? "pred" : need_mean && !mean ? "mean"
                            : kind == IODINE_SHEET_GT && (!gt || sp->n_gt < 1) ? "gt (with n_gt >= 1)" : nullptr;
        if (missing) return "panel " + std::to_string(c) + " (kind " + std::to_string(kind) + ") needs " + missing;
    }
    return "";
}

}  // namespace

extern "C" {

int iodine_sheet_size(const iodine_sheet_spec* spec, int* height, int* width)
{
    std::string why = !height || !width ? "height or width is NULL" : sheet_spec_error(spec);
    if (!why.empty()) return free_fail(IODINE_ERR_INVALID, "iodine_sheet_size: " + why);
    long long H, W;
    sheet_dims(*spec, H, W);
    *height = (int)H;
    *width = (int)W;
    return IODINE_OK;
}

int iodine_sheet_form(const iodine_sheet_spec* spec, const float* x, const float* pred, const float* mask, const float* mean,
                      const unsigned char* gt, const unsigned char* sheet)
{
    const std::string why = sheet_call_error(spec, x, pred, mask, mean, gt, sheet);
    if (!why.empty()) return free_fail(-1, "iodine_sheet_form: " + why);
    long long H, W;
    sheet_dims(*spec, H, W);
    return sheet_form(*spec, x, pred, mask, mean, gt, sheet, (int)W);
}

int iodine_render_sheet(void* stream, const iodine_sheet_spec* spec, const float* x, const float* pred, const float* mask,
                        const float* mean, const unsigned char* gt, const unsigned char* slot_color, const unsigned char* gt_color,
                        unsigned char* sheet)
{
    const std::string why = sheet_call_error(spec, x, pred, mask, mean, gt, sheet);
    if (!why.empty()) return free_fail(IODINE_ERR_INVALID, "iodine_render_sheet: " + why);
    long long H, W;
    sheet_dims(*spec, H, W);
    return free_hip("iodine_render_sheet", launch_render_sheet((hipStream_t)stream, *spec, x, pred, mask, mean, gt, slot_color, gt_color, sheet, (int)W));
}

}  // extern "C"
