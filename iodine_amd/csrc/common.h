// Host-side declarations of libiodine_hip.so (gfx950 only): the kernel launchers, the packed-weight geometry and the small
// per-device caches.  Device-side helpers are in device.h.
#pragma once
#include "device.h"
#include "launch.h"
#include <algorithm>
#include <atomic>

// compute units of the CURRENT device (persistent grids are sized from it), cached per device
inline hipError_t iod_cu_count(int* n_cu)
{
    static std::atomic<int> cache[32];
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    int v = cache[dev & 31].load(std::memory_order_acquire);
    if (!v) {
        e = hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev);
        if (e != hipSuccess) return e;
        cache[dev & 31].store(v, std::memory_order_release);
    }
    *n_cu = v;
    return hipSuccess;
}

// Timing-only ablation hook for tools/helper_cost.py: a library built with -DIODINE_XSKIP_HOOK lets
// iodine_set_option("xskip", mask) turn the tagged launchers into no-ops (results are then WRONG; the product build has no
// such option).  Bits: 1 partial-tile reductions, 2 head-backward GEMMs, 4 refine head, 8 pixel passes, 16 broadcast layer
// forward, 32 broadcast layer backward, 64 pointwise/axpy, 128 output conv forward, 256 output conv data gradient,
// 512 refinement convs forward, 1024 refinement conv gradients, 2048 output conv weight gradient.
#ifdef IODINE_XSKIP_HOOK
extern int g_iod_xskip;
#define IOD_XSKIP(bit) do { if (g_iod_xskip & (bit)) return hipSuccess; } while (0)
#else
#define IOD_XSKIP(bit) do { } while (0)
#endif

// ---- packed-weight geometry: the extent and index order of every weight pack (shared by host packers and kernels)
#include "pack_geom.h"

// EPI_L0ROWS: data-gradient form whose result is not stored but reduced to per-row left / interior / right sums
// (rows_p[n][y][tile x][3][C]): the input of the broadcast layer's backward when nothing else needs d(pre-activation 0)
// EPI_L0ROWSX (training): the same plus a fourth sum per row and tile, sum_x lin[x] * value over ALL the tile's columns
// (rows_p[n][y][tile x][4][C]): with it the coordinate-channel gradients of the broadcast layer follow from row sums too
enum ConvEpilogue { EPI_BIAS_ELU = 0, EPI_MUL_ELUGRAD = 1, EPI_NONE = 2, EPI_OUT4 = 3, EPI_L0ROWS = 4, EPI_L0ROWSX = 5 };

// ---- launchers (each returns hipError_t from the launch) -------------------------------
hipError_t launch_pack_conv_weights(hipStream_t st, const float* src_oihw, int O, int I, int cin_pad,
                                    int cout, int transpose_flip, float* dst);
hipError_t launch_conv3x3_tile(hipStream_t st, const float* in, const float* wpk, const float* bias,
                               const float* aux, float* out, int N, int S, int cin, int cout, int epi);
hipError_t launch_conv3x3_gather(hipStream_t st, const float* in, const float* wpk, const float* bias,
                                 float* out, int N, int IH, int IW, int cin, int cout, int stride);
hipError_t launch_dec_out(hipStream_t st, const float* in, const float* wk, const float* bias, float* out,
                          int N, int S, int C);

// kernels_pixel.hip
int pixel_blocks_per_image(int P);
// strict = 1 (conv_precision 0): libm expf + IEEE division in the per-pixel mixture terms (pixel_terms.h), 0: v_exp_f32 / v_rcp_f32 where bounded
// joint = 1 (option joint_likelihood): one mixture per pixel over the RGB vector, 0: the reference's mixture per colour channel - the same
// argument of every launcher below that evaluates the terms (pixel_terms_core, pixel_terms.h); never defaulted: a launch site that forgot it
// would silently evaluate the per-channel form in joint mode
hipError_t launch_pixel_pass1(hipStream_t st, const float* x4, const float* dec, float* g, double* part, int B,
                              int K, int P, float sigma, int strict, int joint);
// finalize + KL + batch means in one launch; counter: one zero-initialised device word per handle
hipError_t launch_pixel_finalize_elbo(hipStream_t st, const double* part, int B, int K, int P, int use_ln, float* lnstat, float* ll_img,
                                      const float* pm, const float* plv, int L, float* img_terms, float* scal, unsigned* counter, float beta);
hipError_t launch_pixel_pass2(hipStream_t st, const float* x4, const float* dec, const float* lnstat,
                              const float* lin, float* enc, int B, int K, int S, float sigma, float* enc_sh, unsigned chmask,
                              int strict, int stable, int joint);               // stable: option stable_encoding (mask_post, pixel_terms.h)
// option sigma_grad: out[0] = d LL / d sigma of the evaluation whose decoder output is dec (kernels_pixel.hip); part: B x blocks doubles
hipError_t launch_pixel_sigma_grad(hipStream_t st, const float* x4, const float* dec, double* part, float* out, int B, int K, int P,
                                   double sigma, int strict, int joint);
// kernels_pixmap.hip (iodine.py:210-220).  The raw per-pixel maps of the evaluation whose decoder output is dec: ll (B,3,P) = log_likelihood
// (joint: (B,1,P), one plane per image), kll (B,K,3,P) = K_log_likelihood, NCHW, either may be NULL; the pixel weight in lane 3 of x4 is not read
hipError_t launch_pixel_like_maps(hipStream_t st, const float* x4, const float* dec, float* ll, float* kll, int B, int K, int P, float sigma,
                                  int strict, int joint);
// option input_grad: gx[b * gx_bs + c * P + p] (=, first_x, or +=) coef * -sum_k g1_kc; gw[b * gw_bs + p] (=, first_w, or +=) coef * sum_c ll_c;
// either pointer may be NULL.  g1 / ll_sum come from pixel_terms_core: the pixel weight is inside g1, gw is raw
hipError_t launch_pixel_input_grad(hipStream_t st, const float* x4, const float* dec, float* gx, size_t gx_bs, float* gw, size_t gw_bs, int B,
                                   int K, int P, float sigma, int strict, float coef, int first_x, int first_w, int joint);
hipError_t launch_final_out(hipStream_t st, const float* dec, float* pred, float* mask, float* mean, float* logits,
                            int B, int K, int P);
// kernels_edit.hip: final_out for edits that each replace (src = row of `edit` [rows][P][4]) or remove (src < 0) ONE slot of an image of
// `base` [B K][P][4]; the per-edit host indices travel by value in the kernel arguments.  bs = image * 16 + slot
constexpr int SCENE_EDIT_MAX = 256;             // edits of one launch (2 KB of kernel arguments)
struct SceneEditList { int n; int bs[SCENE_EDIT_MAX]; int src[SCENE_EDIT_MAX]; };
hipError_t launch_scene_edit_out(hipStream_t st, const float* base, const float* edit, const SceneEditList& list, float* pred, float* mask,
                                 float* mean, int K, int P);
// kernels_predictive.hip (iodine_predictive): z [n_s][rows][L] = mean + exp(logvar / 2) eps for the samples of a chunk (post_stride L: a
// posterior (rows, L); 0: one row for all), and the per-pixel accumulation over those samples' decoder output dec [n_s B K][P][4] -
// Welford moments of pred (B,3,P) / mask (B,K,P), int votes (B,K,P), all five required (read when s0 > 0, written always); x4 != NULL:
// also ll [n_s][B] through part = n_s * B * predictive_blocks_per_image(P) doubles.  s0 = global index of the chunk's first sample
int predictive_blocks_per_image(int P);
hipError_t launch_predictive_sample(hipStream_t st, const float* pm, const float* plv, const float* eps, float* z, int n_s, int rows, int L,
                                    int post_stride);
hipError_t launch_predictive_accum(hipStream_t st, const float* dec, const float* x4, int B, int K, int P, int s0, int n_s, float* pred_mean,
                                   float* pred_m2, float* mask_mean, float* mask_m2, int* votes, double* part, float* ll, float sigma,
                                   int strict, int joint);
// kernels_render.hip: backward of the rendering (sigmoid, slot softmax, sum_k mask * mean) for the caller's gradients wrt pred (B,3,S,S),
// mask (B,K,1,S,S), mean (B,K,3,S,S) - NCHW, any of them NULL = zero - into g [N][P][4]; strict as for launch_pixel_pass1
hipError_t launch_render_bwd(hipStream_t st, const float* dec, const float* g_pred, const float* g_mask, const float* g_mean, float* g,
                             int B, int K, int P, int strict);
// the same with a gradient wrt the mask logits (B,K,1,S,S) added behind the softmax backward; g_logits == NULL: launch_render_bwd, bit for bit
hipError_t launch_render_bwd_logits(hipStream_t st, const float* dec, const float* g_pred, const float* g_mask, const float* g_mean,
                                    const float* g_logits, float* g, int B, int K, int P, int strict);
// seeds [N][L] of the head BPTT's first step from cotangents on the final evaluation of a training forward: dz = Rc . wclsT (Rc NULL: 0) + c_z,
// seed_m = dz + c_pm, seed_v = dz * (z - pm) / 2 + c_plv (z - pm = exp(logvar / 2) eps; no KL term); c_* may be NULL
hipError_t launch_latent_seed(hipStream_t st, const float* Rc, const float* wclsT, int N, int L, int C, const float* c_z, const float* c_pm,
                              const float* c_plv, const float* z, const float* pm, float* seed_m, float* seed_v,
                              int ldpm = 0,             // row stride of pm (0 = L): mu_i inside the saved refinement input [N][4 L]
                              const float* c_z2 = nullptr, const float* c_pm2 = nullptr, const float* c_plv2 = nullptr);   // a second set, added
// dz = Rc . wclsT without the KL / layer-norm terms of launch_dz_latent; pm != NULL: the posterior gradients of one ELBO instead (scale = 1 / B)
hipError_t launch_dz_plain(hipStream_t st, const float* Rc, const float* wclsT, int N, int L, int C, float* dz_out, const float* pm,
                           const float* plv, const float* eps, float scale, float* g_pm, float* g_plv, float beta);
// kernels_misc.hip
// F > 1: x is a clip (B,F,3,P), batch first; x4 [F][B][P][4], frame-major
// lane 3 of x4: the pixel weight w[b][f][p] (w_per_frame) / w[b][p] (every frame), 1.f where w is NULL
hipError_t launch_x_to_nhwc4(hipStream_t st, const float* x, float* x4, int B, int P, int F = 1, const float* w = nullptr, int w_per_frame = 0);
hipError_t launch_img_terms_split(hipStream_t st, const float* terms, float* kl, float* ll, int n);
hipError_t launch_posterior_init(hipStream_t st, const float* im, const float* ilv, float* pm, float* plv, float* h,
                                 float* c, int N, int L, int H);
hipError_t launch_dec_l0_prepare(hipStream_t st, const float* w, const float* bias, const float* lin, int C, int L,
                                 int S, float* wcls, float* wclsT, float* cmap);
hipError_t launch_dec_v(hipStream_t st, const float* pm, const float* plv, const float* eps, const float* z_in,
                        const float* wcls, float* z_out, float* V, int N, int L, int C);
hipError_t launch_dec_l0(hipStream_t st, const float* V, const float* cmap, float* out, int N, int S, int C, float* tmax = nullptr);
// slot groups of the fused layer-0 reduction (each at most 32 slots); Dpart holds l0_dgroups(N) * P * C floats
inline int l0_dgroups(int N) { const int g = (N + 31) / 32; return g < 8 ? 8 : g; }
// several small device-to-device copies in ONE launch (iodine_set_params: biases and raw weight copies)
// (round 5: also the transposes [R][Cc] -> [Cc][R] (op 1, n = R * Cc, cols = Cc) and the sum of two vectors (op 2, src + src2) of the same
// parameter update - one launch instead of seven)
constexpr int MCOPY_MAX = 40;
struct MultiCopy { const float* src[MCOPY_MAX]; const float* src2[MCOPY_MAX]; float* dst[MCOPY_MAX]; int n[MCOPY_MAX]; int op[MCOPY_MAX]; int cols[MCOPY_MAX]; int count; };
hipError_t launch_multi_copy(hipStream_t st, const MultiCopy& mc);
size_t l0_rows_scratch_floats(int N, int C);
hipError_t launch_l0_reduce_cls_tiles(hipStream_t st, const float* rows_p, float* Rc, int N, int S, int C, float* scratch);
hipError_t launch_l0_reduce_cls_tiles_x(hipStream_t st, const float* rows_p, float* Rc, float* rown, int N, int S, int C, float* scratch);
hipError_t launch_l0_rowsum_acc(hipStream_t st, const float* rown, int N, int S, int C, float alpha, int first, float* Rsum);
hipError_t launch_l0_coord_grads_rows(hipStream_t st, const float* Rsum, const float* lin, int S, int C, int L, float alpha,
                                      float* gw, float* gb);
hipError_t launch_l0_reduce(hipStream_t st, const float* dpre, float* rows, float* Rc, int N, int S, int C, float* Dpart,
                            float* Dacc, float alpha, int first);
hipError_t launch_dz_latent(hipStream_t st, const float* Rc, const float* wclsT, const float* pm, const float* plv,
                            const float* eps, int N, int L, int C, int use_ln, float* g_pm, float* g_plv, float* latent, int Lreal, float beta);
hipError_t launch_refine_head(hipStream_t st, const float* feat, int N, int PL, int C, int H, int L,
                              const float* mlp_wT, const float* mlp_b, const float* wihT, const float* whhT,
                              const float* lstm_b, const float* wmT, const float* bm, const float* wvT, const float* bv,
                              const float* latent, const float* h_prev, const float* c_prev, float* h_out, float* c_out,
                              float* pm, float* plv, float* sv_pooled, float* sv_s, float* sv_gates, float* sv_xin,
                              float* d_mean, float* d_logvar, float* xh = nullptr, float* gp = nullptr, int prefer_split = 1);
// which form launch_refine_head runs for these widths (multiples of 4) when it is given the xh / gp scratch: 0 = single launch, 1 = three
// launches (pre, gate GEMM, post), -1 = neither fits.  prefer_split picks between the two only where both can run.  Host arithmetic only.
int refine_head_form(int C, int H, int L, int prefer_split);
size_t refine_head_lds_bytes(int C, int H, int L, int split);
hipError_t launch_pack_dec_out(hipStream_t st, const float* w, float* wk, int C);
hipError_t launch_conv3x3_gather_dgrad(hipStream_t st, const float* d, const float* wpk, const float* aux, float* out,
                                       int N, int big_h, int big_w, int c, int stride);
// kernels_wgrad.hip
int wgrad_tile_blocks(int N, int S);
hipError_t launch_conv3x3_wgrad_tile(hipStream_t st, const float* a, const float* d, float* part, float* part_b, int N,
                                     int S, int ci, int nco, int* nparts, int* ncop, int* nbias_parts);
hipError_t launch_conv3x3_wgrad_gather(hipStream_t st, const float* in, const float* d, float* part, int N, int IH,
                                       int IW, int cip, int co, int stride, int* nparts, int* cipad);
constexpr int WGRAD_FOLD = 32;    // tiles left after the first reduction stage; `fold` holds WGRAD_FOLD * 9 * ci_pad * co_pad floats
hipError_t launch_wgrad_reduce(hipStream_t st, const float* part, int nparts, int ci_pad, int co_pad, int O_real,
                               int I_real, int I_dst, float alpha, float* dst, float* fold = nullptr,
                               const float* part_b = nullptr, int nb = 0, float* dst_b = nullptr);
// kernels_gemm.hip
hipError_t launch_colsum(hipStream_t st, const float* src, int rows, int cols, int ld, float alpha, float* dst);
hipError_t launch_colsum_tall(hipStream_t st, const float* src, int rows, int cols, float alpha, float* dst, float* tmp,
                              size_t tmp_elems);
hipError_t launch_sgemm(hipStream_t st, int ta, int tb, int M, int N, int K, float alpha, const float* A, int lda,
                        const float* B, int ldb, float beta, float* C, int ldc);
// C = alpha * A^T . B + beta * C, A [K][M], B [K][N], on fp32 MFMA (M, N multiples of 32); mode 1: C through the broadcast layer's weight map
bool sgemm_tn_mfma_ok(int M, int N, int K);
hipError_t launch_sgemm_tn_mfma(hipStream_t st, int M, int N, int K, float alpha, const float* A, int lda, const float* B, int ldb,
                                float beta, float* C, int ldc, int mode, int mode_c, int a_rowmajor = 0);
// kernels_train.hip
hipError_t launch_l0_tap_sums(hipStream_t st, const float* Rc, float* RT, int N, int C);
hipError_t launch_l0_latent_wgrad(hipStream_t st, const float* Rc, const float* z, int N, int L, int C, float alpha, float* gw);
hipError_t launch_l0_coord_grads(hipStream_t st, const float* D, const float* lin, int S, int C, int L, float alpha,
                                 float* gw, float* gb, float* scratch);
// wtab: device table of n loss weights (iodine_set_objective), NULL = the default (i + 1) / n
hipError_t launch_loss(hipStream_t st, const float* scal, int n, float* loss, const float* wtab);
hipError_t launch_scale(hipStream_t st, const float* a, float alpha, float* o, int n);
hipError_t launch_zero_fill(hipStream_t st, float* p, size_t n);       // p[0 .. n) = 0 as a kernel (not a memset node: see kernels_train.hip)
hipError_t launch_axpy_dev(hipStream_t st, const float* x, float alpha, const float* alpha_dev, float* y, int n, int accumulate);
// y = *s_dev * y + add in place (s_dev NULL: factor 0; add NULL: nothing added)
hipError_t launch_scale_dev_add(hipStream_t st, float* y, const float* s_dev, const float* add, int n);
hipError_t launch_mean2(hipStream_t st, const float* a, const float* b, int n, float* out);
// kernels_headbwd.hip
hipError_t launch_lstm_bwd_pointwise(hipStream_t st, const float* gates, const float* c0, const float* c1,
                                     const float* dc1_read, const float* dh1, const float* dc1_carry, float* dgates,
                                     float* dc0, int N, int H);
hipError_t launch_mlp_bwd_pointwise(hipStream_t st, const float* du, int ldu, const float* s, float* ds, int N, int H);
hipError_t launch_pool_bwd(hipStream_t st, const float* dpooled, const float* act, float* dpre, int N, int PL, int C);
bool head_bptt_fits(int L, int H, int Cr);
hipError_t launch_head_bptt(hipStream_t st, const float* g_pm, const float* g_plv, const float* gates, const float* cst, const float* u,
                            const float* Wm, const float* Wv, const float* Whh, const float* Wih, const float* Wmlp, float* ddm,
                            float* ddv, float* dgates, float* ds, float* dpooled, int T, int N, int B, int L, int H, int Cr,
                            const float* seed_m, const float* seed_v, const float* gl_dev,
                            const float* wtab,        // wtab: T + 1 loss weights, NULL = the default (i + 2) / (T + 1)
                            const float* dh_in = nullptr, const float* dc_in = nullptr,    // [N][H] cotangents on (h_T, c_T): initial carries
                            float* dh_out = nullptr, float* dc_out = nullptr,              // [N][H] d / d (h_0, c_0): the carries left (seeded instance only)
                            size_t seed_stride = 0);  // != 0: seed_m / seed_v are [T][N][L] (stride in floats), slice i joins step i; 0: step T - 1 alone
// the same recurrence as a launch sequence; whost: HOST table of T + 1 loss weights or NULL; scratch dc1, dxin, carry_h[2], carry_c[2]: [N][H] each
hipError_t launch_head_bptt_unfused(hipStream_t st, const float* g_pm, const float* g_plv, const float* gates, const float* cst, const float* u,
                                    const float* Wm, const float* Wv, const float* Whh, const float* Wih, const float* Wmlp, float* ddm,
                                    float* ddv, float* dgates, float* ds, float* dpooled, int T, int N, int B, int L, int H, int Cr,
                                    int seeded, const float* seed_m, const float* seed_v, const float* gl_dev, const float* whost,
                                    const float* dh_in, const float* dc_in, float* dh_out, float* dc_out, size_t seed_stride,
                                    float* dc1, float* dxin, float* const carry_h[2], float* const carry_c[2]);
// split-precision (3 x fp16 MFMA) variant of the stride-1 tile conv
hipError_t launch_pack_conv_weights_f16(hipStream_t st, const float* src, int O, int I, int cin, int cout, int tflip,
                                        float* meta, void* dst);
hipError_t launch_conv3x3_tile_f16x3(hipStream_t st, const float* in, const void* wpk, const float* wmeta,
                                     const float* bias, const float* aux, float* out, int N, int S, int cin, int cout,
                                     int epi, int rev = 0);
hipError_t launch_adam_multi(hipStream_t st, const long long* ptrs, const long long* offs, int n_tensors, long long total,
                             double lr, double beta1, double beta2, double eps, double wd, int step,
                             const float* out4 = nullptr, int skip_nonfinite = 0);   // out4: clipped step, see kernels_clip.hip
// kernels_clip.hip: global gradient norm + clip coefficient over the same tables (lib/engine/train.py:64)
size_t grad_norm_scratch_bytes(long long total);
hipError_t launch_grad_norm(hipStream_t st, const long long* ptrs, const long long* offs, int n_tensors, long long total,
                            double max_norm, double* partials, float* out4);
hipError_t launch_grad_scale(hipStream_t st, const long long* ptrs, const long long* offs, int n_tensors, long long total,
                             const float* coef_dev);
hipError_t launch_randn_philox(hipStream_t st, float* out, long long n, unsigned long long seed, unsigned long long stream_id);
hipError_t launch_ari_table(hipStream_t st, const float* mask, const unsigned char* gt, int B, int K, int G, int P,
                            int* table);
// kernels_objects.hip: per-slot object table + segmentation map, contingency table of two segmentations (stateless, like launch_ari_table)
hipError_t launch_slot_table(hipStream_t st, const float* mask, const float* mean, int B, int K, int S, float* table,
                             unsigned char* seg);
hipError_t launch_seg_overlap(hipStream_t st, const unsigned char* seg_a, const unsigned char* seg_b, int B, int Ka, int Kb, int P,
                              int* table);
// kernels_components.hip: connected components of segmentation maps (stateless; scratch of seg_components_scratch_bytes, host-only query)
size_t seg_components_scratch_bytes(int B, int S);
hipError_t launch_seg_components(hipStream_t st, const unsigned char* seg, int B, int slots, int S, int conn, int min_area, int M,
                                 int* labels, int* area_map, int* count, int* per_slot, int* table, unsigned char* clean, void* scratch);
// kernels_chains.hip: refinement restarts - C decodes of the same images scored and labelled, C labellings folded into one (stateless)
hipError_t launch_chain_score(hipStream_t st, const float* x, const float* w, const float* mask, const float* mean, int C, int B, int K,
                              int S, double sigma, int joint, float* ll, unsigned char* seg);
hipError_t launch_chain_consensus(hipStream_t st, const unsigned char* seg, const int* perm, const int* ref, const float* mask, int C,
                                  int B, int K, int S, int* votes, unsigned char* consensus, float* agreement, float* match,
                                  float* mask_mean);
// kernels_adaptive.hip: adaptive refinement - which of the n active images stop after t updates (one block, stable compaction), and the
// row gather / scatter that follows them (stateless).  AdaptiveRule: the controls of tests/adaptive_reference.py with the objective's beta.
// MoveEntry: row r of `rows` goes from src row src_index[r] to dst row dst_index[r] (NULL: r); src_rows / dst_rows = the arrays' extents in
// rows, an index outside them moves nothing; vec is the launcher's (float4 where the row size and both pointers allow it)
struct AdaptiveRule { int max_iters, min_iters, check_every; double tol, rtol, beta; };
struct MoveEntry { const float* src; float* dst; long long row_floats; const int* src_index; const int* dst_index; int rows, src_rows, dst_rows, vec; };
constexpr int ADAPTIVE_MOVE_MAX = 16;
hipError_t launch_adaptive_select(hipStream_t st, const float* terms, const int* idx_in, int n, int R, int t, int B, const AdaptiveRule& rule,
                                  const int* budget, int* idx_out, int* pos_out, int* stop_idx, int* stop_pos, int* counts, int* iters,
                                  float* ll, float* kl);
hipError_t launch_adaptive_move(hipStream_t st, const MoveEntry* entries, int count);
// kernels_sheet.hip: decomposition sheets - panels of a few scenes as one uint8 HWC picture (stateless).  W = the sheet's width;
// sheet_form: bit 0 = 16-byte loads, bit 1 = word stores, what the launcher will take for these pointers.
struct iodine_sheet_spec;
int sheet_form(const iodine_sheet_spec& sp, const float* x, const float* pred, const float* mask, const float* mean,
               const unsigned char* gt, const unsigned char* sheet, int W);
hipError_t launch_render_sheet(hipStream_t st, const iodine_sheet_spec& sp, const float* x, const float* pred, const float* mask,
                               const float* mean, const unsigned char* gt, const unsigned char* slot_color, const unsigned char* gt_color,
                               unsigned char* sheet, int W);
// kernels_match.hip: slots matched to ground-truth masks - statistics, assignment (assign.h), loss and its gradient (stateless)
hipError_t launch_mask_overlap(hipStream_t st, const float* mask, const unsigned char* gt, int B, int K, int G, int S, float eps,
                               float* inter, float* nll, float* mask_area, int* gt_area);
// kernels_batch.hip: device-resident datasets - a batch gathered from the store, synth.make_images on the device (stateless)
hipError_t launch_batch_gather(hipStream_t st, const long long* index, int count, const void* images, int kind, const unsigned short* masks,
                               int S, int planes, float* x, unsigned char* gt);
hipError_t launch_synth_scenes(hipStream_t st, int n, int S, unsigned long long seed, unsigned long long seed_step, unsigned long long stream,
                               unsigned long long stream_step, int kind, int max_objects, int frames, float* images, unsigned short* masks,
                               unsigned char* n_gt);
// kernels_window.hip: a batch cut out of native-size frames - crop, antialiased resize, flip and colour gain per item (stateless)
hipError_t launch_batch_window(hipStream_t st, const long long* index, int count, const void* images, int kind, const unsigned short* masks,
                               int H, int W, const float* windows, int S, int planes, float* x, unsigned char* gt);
hipError_t launch_assign(hipStream_t st, const float* cost, const unsigned char* row_valid, int B, int G, int K, int* assign,
                         float* total);
hipError_t launch_mask_match(hipStream_t st, const float* inter, const float* nll, const float* mask_area, const int* gt_area, int B,
                             int K, int G, int match_kind, int loss_kind, int* assign, float* loss, float* coef, float* cost_out,
                             float* iou_out);
hipError_t launch_mask_match_bwd(hipStream_t st, const float* mask, const unsigned char* gt, const int* assign, const float* coef,
                                 const float* grad_loss, int B, int K, int G, int S, int loss_kind, float eps, float* grad);
hipError_t launch_pack_dec_out_gemm(hipStream_t st, const float* w, int C, float* meta, void* dst);
hipError_t launch_pack_dec_out_dgrad(hipStream_t st, const float* w, int C, const float* meta, void* dst);
hipError_t launch_dec_out_dgrad_f16x3(hipStream_t st, const float* g, const void* wpk, const float* wmeta, const float* aux,
                                      float* out, int N, int S, int C, float* tmax = nullptr);
hipError_t launch_dec_out_stream_f16x3(hipStream_t st, const float* in, const void* wpk, const float* wmeta,
                                       const float* bias, float* out, int N, int S, int C, const float* tmax = nullptr);

// row-streaming form of the same output conv (round 5: no halo recompute; S in {32, 64, 128}, needs the producer's cell maxima)
bool dec_out_rows_ok(int S, int C, const float* tmax);
// f32 = 1: exact fp32 MFMA form (wpk = launch_pack_dec_out_rows32, wmeta / tmax unused)
hipError_t launch_dec_out_rows_f16x3(hipStream_t st, const float* in, const void* wpk, const float* wmeta, const float* bias, float* out,
                                     int N, int S, int C, const float* tmax, int f32 = 0);
hipError_t launch_pack_dec_out_rows32(hipStream_t st, const float* w, int C, float* dst);

// kernels_convws.hip: weight-stationary split-fp16 3x3 conv C -> C (weights in registers, persistent blocks)
hipError_t launch_pack_conv_weights_ws(hipStream_t st, const float* src, int C, int tflip, float* meta, void* dst);
// kernels_pack.hip: the packs above for many tensors in two launches.  kind 0 = launch_pack_conv_weights_ws(src, C = p[0], tflip = p[1]),
// kind 1 = launch_pack_conv_weights_f16(src, O = p[0], I = p[1], cin = p[2], cout = p[3], tflip = p[4]); meta / dst as there
// round 5: kind 2 = the two operands of kernels_refl0.hip (src [O][cinw][9], O = p[0], cinw = p[1]; scale of its own), kind 3 = launch_pack_dec_out_gemm(src, C = p[0]),
// kind 4 = launch_pack_dec_out_dgrad(src, C = p[0]) with the scale kind 3 of the same batch leaves in the shared meta (p[1] = 1: no scale of its own)
constexpr int PACK_BATCH_MAX = 48;
struct PackJob { const float* src; void* dst; float* meta; int kind; int p[5]; };
hipError_t launch_pack_batch(hipStream_t st, const PackJob* jobs, int n);
// round 6: tensors between the reference's shapes and the padded shapes of the inner handle (DIM_LATENT / MLP_UNITS not multiples of 4)
hipError_t launch_pad_gather(hipStream_t st, const float* src, const int* map, float* dst, int n);
hipError_t launch_pad_scatter(hipStream_t st, const float* src, const int* map, float* dst, int n, int accumulate);
hipError_t launch_resize_rows(hipStream_t st, const float* src, float* dst, long long rows, int w_src, int w_dst);
hipError_t launch_cell_max(hipStream_t st, const float* x, float* tmax, int N, int S, int C);
hipError_t launch_conv3x3_ws_f16x3(hipStream_t st, const float* in, const void* wpk, const float* wmeta, const float* bias,
                                   const float* aux, float* out, const float* tmax_in, float* tmax_out, int N, int S, int c,
                                   int epi, int rev, int products = 3);
// (products: fp16 MFMAs per product - 3 = the split, fp32-class; 1 = hi.hi alone with the activations rounded to nearest even, fp16-class:
// option conv_precision 2.  Same pack, same side buffers.)
// exact-fp32 form of the same kernel (conv_precision 0): fp32 weights in the register layout (same byte count), v_mfma_f32_16x16x4_f32
hipError_t launch_pack_conv_weights_ws32(hipStream_t st, const float* src, int C, int tflip, void* dst);
hipError_t launch_conv3x3_ws_f32(hipStream_t st, const float* in, const void* wpk, const float* bias, const float* aux, float* out,
                                 int N, int S, int c, int epi, int rev);
// kernels_wgrad32.hip: exact-fp32 weight gradient, persistent + prefetched (part: [nparts][9][c][c], part_b: [nbias_parts][c])
hipError_t launch_conv3x3_wgrad_f32_ws(hipStream_t st, const float* a, const float* d, float* part, float* part_b, int N, int S, int c,
                                       int* nparts, int* ncop, int* nbias_parts, float alpha = 1.f, int accum = 0);
// exact-fp32 weight gradient of the output conv c -> 4 in GEMM form (part: [nparts][9][c][4], part_b: [nbias_parts][4])
hipError_t launch_dec_out_wgrad_f32(hipStream_t st, const float* a, const float* g, float* part, float* part_b, int N, int S, int c,
                                    int* nparts, int* nbias_parts);
inline size_t conv_ws_tmax_floats(int N, int S) { return (size_t)N * (S / 16) * (S / 8) * 4; }

// tools/experiments/kernels_wino.hip (experiment, only in libraries built by tools/wino_variants.sh): Winograd F(2x2, 3x3) form
size_t conv_wino_wpk_bytes(int C);
size_t conv_wino_scratch_floats(int C);
hipError_t launch_pack_conv_weights_wino(hipStream_t st, const float* src, int C, int tflip, float* meta, void* dst, float* scratch);
hipError_t launch_conv3x3_wino_f16x3(hipStream_t st, const float* in, const void* wpk, const float* wmeta, const float* bias,
                                     const float* aux, float* out, const float* tmax_in, float* tmax_out, int N, int S, int c,
                                     int epi, int rev);

// kernels_refine.hip: split-fp16 stride-2 convs of the refinement network
hipError_t launch_conv3x3_s2_f16x3(hipStream_t st, const float* in, const void* wpk, const float* wmeta, const float* bias,
                                   float* out, int N, int S, int cin_real, int cout, const float* addmap = nullptr, int kdiv = 0,
                                   int f32 = 0);
// exact-fp32 forms of the three stride-2 kernels (conv_precision 0, round 5: v_mfma_f32_32x32x2_f32; f32 = 1 on the launchers):
// fp32 weights in the same LDS-tile layout / byte count as launch_pack_conv_weights_f16
hipError_t launch_pack_conv_weights_s2f32(hipStream_t st, const float* src, int O, int I, int cin, int cout, int tflip, void* dst);
hipError_t launch_ref_split_weights(hipStream_t st, const float* w, int O, float* w_slot, float* w_sh);
hipError_t launch_enc_expand_weights(hipStream_t st, const float* w, int O, int n_in, const int* map17, float* w17, int kk = 9);
hipError_t launch_enc_gather_grad(hipStream_t st, const float* g17, int O, int n_in, const int* map17, float* gw, int kk = 9);

// kernels_generic.hip: fallback fp32 convs for any odd kernel size / channel count (correctness path, see the file header)
constexpr int GEN_WGRAD_SLICES = 64;
constexpr int GEN_WGRAD_OUT_SLICES_MAX = 512;   // row slices of the 4-output-channel GEMM form (one per resident block)
constexpr int GEN_WGRAD_SLICES_MAX = 128;  // the row-staged form sizes its slices to the chip (two blocks per CU): scratch is sized for this many
hipError_t launch_gen_pack_weights(hipStream_t st, const float* w, int Co, int Ci, int k, float* wt);
// the kernel a generic conv runs on (gen_conv_tier: the launchers switch on it, iodine_op_gen_conv_tier reports it to the tests).  Forward and
// data gradient: MFMA_CCH16 / 8 / 4 (stride-1 MFMA kernel by chunk width), S2_MFMA, SCALAR; weight gradient: WGRAD_OUT (np = its NP
// instantiation 1 / 2 / 4 / 8), WGRAD_ROWS, WGRAD_MFMA, S2_MFMA, SCALAR.  The values are part of the C ABI (include/iodine_hip.h).
enum GenTier { GEN_TIER_MFMA_CCH16 = 0, GEN_TIER_MFMA_CCH8 = 1, GEN_TIER_MFMA_CCH4 = 2, GEN_TIER_S2_MFMA = 3, GEN_TIER_SCALAR = 4,
               GEN_TIER_WGRAD_OUT = 5, GEN_TIER_WGRAD_ROWS = 6, GEN_TIER_WGRAD_MFMA = 7 };
// seg: an output of the forward / data gradient is ONE fp32 fmaf chain over its Ck k^2 products, whose rounding grows with the chain; chains
// of more than GEN_CHAIN_MAX products (the default decoder's 5 x 5 x 64 stays one chain: its results do not change) are summed in nseg =
// ceil(products / GEN_CHAIN_SEG) segments that are added at the end.  seg = the segment length - staged chunks (MFMA kernel) or products
// (scalar kernels) -, 0 = one chain.
constexpr int GEN_CHAIN_MAX = 1600, GEN_CHAIN_SEG = 800;
struct GenTierSel { GenTier tier; int np; size_t lds; int seg; };  // lds: dynamic LDS bytes of the chosen kernel (0: none)
GenTierSel gen_conv_tier(int mode, int Si, int Ci, int ldc, int Co, int k, int s);
// chmask (stride-2 MFMA forms only): bit c = input channel c can be non-zero - groups of channels whose weights AND inputs are zero (an
// ARCH.ENCODING subset: absent encoding channels) are skipped; all ones = every channel
hipError_t launch_gen_conv_fwd(hipStream_t st, const float* in, const float* wt, const float* bias, float* out, int N, int Si, int Ci,
                               int ldc, int Co, int k, int s, int elu, unsigned chmask = 0xffffffffu);
hipError_t launch_gen_conv_dgrad(hipStream_t st, const float* dout, const float* wt, const float* aux, float* din, int N, int Si, int Ci,
                                 int ldi, int Co, int k, int s);
size_t gen_wgrad_scratch_floats(int Ci, int Co, int k);
hipError_t launch_gen_conv_wgrad(hipStream_t st, const float* in, const float* dout, float* scratch, int N, int Si, int Ci, int ldc,
                                 int Ci_dst, int Co, int k, int s, float alpha, float* gw, float* gb, unsigned chmask = 0xffffffffu);
// kernels_gensplit.hip: split-fp16 (3 x v_mfma_f32_16x16x32_f16) form of the stride-1 conv C -> C, forward and data gradient (option
// gen_conv_precision 1).  gen_split_cch: 32 / 16 = covered (k in {3, 5, 7}, C a multiple of 16, slice + halo fit the LDS), 0 = stays on fp32
int gen_split_cch(int k, int C);
size_t gen_split_pack_bytes(int k, int C);                  // wpk_gen_split_bytes at the chunk width gen_split_cch chooses (0: not covered)
hipError_t launch_gen_split_pack(hipStream_t st, const float* wt, int k, int C, int dgrad, void* dst, float* meta);
hipError_t launch_gen_split_conv(hipStream_t st, const float* in, const void* wpk, const float* wmeta, const float* bias, const float* aux,
                                 float* out, int N, int S, int C, int k, int elu);
bool gen_split_wgrad_ok(int k, int C);
hipError_t launch_gen_split_wgrad(hipStream_t st, const float* in, const float* dout, float* scratch, int N, int S, int C, int k, float alpha,
                                  float* gw, float* gb);
hipError_t launch_gen_wgrad_reduce(hipStream_t st, const float* part, int nslice, int Ci, int Ci_dst, int Co, int kk, float alpha, float* gw,
                                   float* gb);
// kernels_genl0.hip: the spatial-broadcast layer of the generic decoder without the broadcast tensor (prefix table of per-tap latent products
// forward, tap-window sums of the gradient backward); any odd k <= GEN_L0_KMAX
constexpr int GEN_L0_KMAX = 7;
size_t gen_l0_scratch_floats(int N, int S, int Co, int k);
hipError_t launch_gen_l0_coord(hipStream_t st, const float* wt0, const float* bias, const float* lin, int L, int S, int Co, int k, float* cterm);
hipError_t launch_gen_l0_fwd(hipStream_t st, const float* z, const float* wt0, const float* cterm, float* scratch, float* out, int N, int L, int S,
                             int Co, int k);
hipError_t launch_gen_l0_bwd(hipStream_t st, const float* dpre, const float* z, const float* wt0, const float* lin, float* scratch, int N, int L,
                             int S, int Co, int k, float alpha, float* gw, float* gb, float* dz, int ld);
// kernels_gens2.hip: the stride-2 convs of the generic path on v_mfma_f32_16x16x4_f32 (round 5)
bool gen_s2_fwd_ok(int k, int Ci, int ldc, int Co);
bool gen_s2_dgrad_ok(int k, int Ci, int ldi, int Co);
bool gen_s2_wgrad_ok(int k, int Ci, int ldc, int Co);
hipError_t launch_gen_s2_fwd(hipStream_t st, const float* in, const float* wt, const float* bias, float* out, int N, int Si, int Ci, int ldc,
                             int Co, int k, int elu, unsigned chmask = 0xffffffffu);
hipError_t launch_gen_s2_dgrad(hipStream_t st, const float* dout, const float* wt, const float* aux, float* din, int N, int Si, int Ci, int ldi,
                               int Co, int k);
hipError_t launch_gen_s2_wgrad(hipStream_t st, const float* in, const float* dout, float* part, int N, int Si, int Ci, int ldc, int Co, int k,
                               int nsl_max, int* nsl_out, unsigned chmask = 0xffffffffu);
hipError_t launch_gen_identity(hipStream_t st, float* m, int rows, int L);
hipError_t launch_ref_unsplit_grad(hipStream_t st, const float* g20, int O, float* gw);
hipError_t launch_enc_join(hipStream_t st, const float* enck, const float* encs, float* enc, int N, int K, int P);
hipError_t launch_conv3x3_s2_dgrad_f16x3(hipStream_t st, const float* d, const void* wpk, const float* wmeta, const float* aux,
                                         float* out, int N, int S, int c, int f32 = 0);
hipError_t launch_conv3x3_s2_wgrad_f16x3(hipStream_t st, const float* a, const float* d, float* part, float* part_b, int N,
                                         int S, int ci_real, int nco, int* nparts, int* cipad, int* nbias_parts,
                                         const float* a2 = nullptr, int kdiv = 0, int f32 = 0);
// kernels_refl0.hip: encoding (pixel_pass2's channels) + first refinement layer (conv k3 s2 17 -> 64, ELU) for all slots of an image
bool refine_l0_fused_ok(int S, int c, int K);
hipError_t launch_refine_l0_fused(hipStream_t st, const float* x4, const float* dec, const float* lnstat, const float* lin, const void* wk,
                                  const float* wkmeta, const void* ws, const float* wsmeta, const float* bias, float* out, float* enck,
                                  float* encs, int B, int K, int S, int c, float sigma, unsigned chmask, int stable, int joint);
// kernels_refws.hip: weight-stationary stride-2 conv C -> C + bias + ELU (refinement layers 1 ..), wpk = launch_pack_conv_weights_ws(w, C, 0)
bool conv3x3_s2ws_ok(int S, int c);
hipError_t launch_conv3x3_s2ws_f16x3(hipStream_t st, const float* in, const void* wpk, const float* wmeta, const float* bias, float* out,
                                     int N, int S, int c, int f32 = 0);       // f32 = 1: exact fp32 form, wpk = launch_pack_conv_weights_ws32(w, c, 0)
// kernels_refbwd.hip: data gradient of refinement layer 1 + weight / bias gradient of layer 0 in one pass (dpre0 never stored)
bool refine_bwd01_ok(int S, int c);
hipError_t launch_refine_bwd01(hipStream_t st, const float* rd1, const void* wpk, const float* wmeta, const float* act0, const float* enck,
                               const float* encs, float* part, float* part_b, int NT, int S, int c, int kdiv, int* nparts, int* cipad,
                               int* nbias_parts);
// kernels_outbwd.hip
hipError_t launch_dec_out_wgrad_gemm_f16x3(hipStream_t st, const float* a, const float* g, float* part, float* part_b, int N,
                                           int S, int c, int* nparts, int* nbias_parts);
hipError_t launch_dec_out_bwd_fused_f16x3(hipStream_t st, const float* a, const float* g, const void* wpk, const float* wmeta,
                                          float* out, float* tmax, float* part, float* part_b, int N, int S, int c,
                                          int* nparts, int* nbias_parts, float alpha = 1.f, int accum = 0);
// alpha / accum (round 5): part / part_b = (accum ? part : 0) + alpha x this launch - a block's partial tile kept over the decoder passes
// kernels_wgradws.hip
hipError_t launch_conv3x3_wgrad_f16x3_ws(hipStream_t st, const float* a, const float* d, float* part, float* part_b, int N,
                                         int S, int ci, int nco, int* nparts, int* ncop, int* nbias_parts, float alpha = 1.f, int accum = 0);
