// The training step: the forward that keeps every iteration (train_forward_impl), the backward through the refinement head and conv
// stack (train_backward_impl) and the eight entry points in front of them.
#include "iodine_internal.h"

extern "C" {

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
            HIPCHK(h, launch_posterior_init(st, h->head.init_mean, h->head.init_logvar, b.pm, b.plv, b.h[0], b.c[0], N, L, h->H));
        int fj = 0;                                        // next entry of the list of chosen evaluations
        for (int i = 0; i <= T; ++i) {
            // d loss / d (B * ELBO_i) = -w_i / B; the default weighting keeps its closed form
            const float alpha = h->obj.whost ? -h->obj.whost[i] / (float)B : -((float)(i + 1) / (float)(T + 1)) / (float)B;
            int r = elbo_and_gradients(h, st, B, eps + (size_t)i * eps_stride, i, true, true, alpha, h->opt.sigma_grad != 0, h->opt.input_grad, -alpha);
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
    cs.sgrad_n = h->opt.sigma_grad ? T + 1 : 0;
    cs.ig_bits = h->opt.input_grad; cs.ig_frames = h->frames > 0 ? h->frames : 0; cs.ig_wpf = h->ig_call_wpf;
    return IODINE_OK;
}

// ---- the phases of train_backward_impl, in the order it runs them

namespace {

// What aux_seeds leaves for the phases behind it: the seeds of the head's BPTT from auxiliary / per-frame cotangents (all NULL / 0: the plain
// backward).  seed_m / seed_v with seed_stride 0: the seeds of the final evaluation alone; with a stride: slice e - 1 is what the recurrence
// adds at iteration e - 1.  seed0_m / seed0_v: the seeds of evaluation 0 = d / d lambda_0, which no iteration of the recurrence reaches
struct BpttSeeds {
    float *seed_m = nullptr, *seed_v = nullptr;
    size_t seed_stride = 0;
    const float *seed0_m = nullptr, *seed0_v = nullptr;
};

// cotangent of kind q (order of FrameSet) on entry j of the list of chosen evaluations; per: the elements of one entry
const float* frame_cot(const FrameSet* fr, int q, int j, size_t per) { return fr->g[q] ? fr->g[q] + (size_t)j * per : nullptr; }

// auxiliary cotangents on the final evaluation only (iodine_train_backward_aux / _seq)
int aux_seeds_final(iodine_handle* h, hipStream_t st, const AuxCot* aux, BpttSeeds& s)
{
    Buffers& b = h->buf;
    const int B = h->calls.fwd_batch, N = B * h->K, T = h->T, L = h->L;
    const bool dec = aux->mean || aux->mask || aux->logits;
    const float* const wl = dec_path(h) == DEC_GENERIC ? h->gen.ident : h->dec.wclsT;
    if (dec) {
        // evaluation T's decoder activations and dec_out are still in the arena: the forward's last launches were that evaluation's own
        // decoder backward, which only reads them, and any compute call since would have cleared fwd_done.  ONE decoder pass with
        // factor 1: every decoder weight gradient, and the class sums of the broadcast layer for dz
        PROF(h, st, "render_bwd", launch_render_bwd_logits(st, b.dec_out, nullptr, aux->mask, aux->mean, aux->logits, b.g, B, h->K, h->P,
                                                           h->opt.precision == 0));
        float* dpre0 = nullptr;
        if (int r = decoder_backward_data(h, st, N, &dpre0, true, 1.f, T, true)) return r;
    }
    s.seed_m = b.aux_seed; s.seed_v = b.aux_seed + (size_t)N * L;
    HIPCHK(h, launch_latent_seed(st, dec ? b.Rc : nullptr, wl, N, L, h->Cd, aux->z, aux->pm, aux->plv, b.z[T], b.pm, s.seed_m, s.seed_v));
    return IODINE_OK;
}

// ... and cotangents on chosen evaluations on top (iodine_train_backward_frames)
int aux_seeds_frames(iodine_handle* h, hipStream_t st, const AuxCot* aux, const FrameSet* fr, BpttSeeds& s)
{
    Buffers& b = h->buf;
    const int B = h->calls.fwd_batch, N = B * h->K, T = h->T, L = h->L;
    const ParamSlots& ps = h->slot;
    const size_t NL = (size_t)N * L, NP = (size_t)N * h->P;
    const bool dec = aux->mean || aux->mask || aux->logits;
    const float* const wl = dec_path(h) == DEC_GENERIC ? h->gen.ident : h->dec.wclsT;
    // Cotangents on chosen evaluations.  Evaluation T (last in the list) first, on the kept activations like the final state's
    // cotangents (aux_seeds_final) - and added to them where both are given: the rendering backward is linear in the cotangents, so the
    // second set is rendered into the (free) ping-pong buffer and added before the ONE decoder pass.
    const int jT = fr->idx[fr->n - 1] == T ? fr->n - 1 : -1;
    const float *t_mean = jT >= 0 ? frame_cot(fr, 1, jT, NP * 3) : nullptr, *t_mask = jT >= 0 ? frame_cot(fr, 2, jT, NP) : nullptr,
                *t_logits = jT >= 0 ? frame_cot(fr, 3, jT, NP) : nullptr;
    const bool decf = t_mean || t_mask || t_logits;
    if (dec)
        PROF(h, st, "render_bwd", launch_render_bwd_logits(st, b.dec_out, nullptr, aux->mask, aux->mean, aux->logits, b.g, B, h->K, h->P,
                                                           h->opt.precision == 0));
    if (decf)
        PROF(h, st, "render_bwd", launch_render_bwd_logits(st, b.dec_out, nullptr, t_mask, t_mean, t_logits, dec ? b.dpre[0] : b.g, B, h->K,
                                                           h->P, h->opt.precision == 0));
    if (dec && decf) HIPCHK(h, launch_axpy_dev(st, b.dpre[0], 1.f, nullptr, b.g, (int)(NP * 4), 1));
    float* dpre0 = nullptr;
    if (dec || decf)
        if (int r = decoder_backward_data(h, st, N, &dpre0, true, 1.f, T, true)) return r;
    // seeds of every evaluation: slice e of [T + 1][N][L]; slices 1 .. T are what the head's BPTT adds at iteration e - 1
    float *m_all = b.aux_seed, *v_all = b.aux_seed + (size_t)(T + 1) * NL;
    HIPCHK(h, launch_zero_fill(st, b.aux_seed, (size_t)2 * (T + 1) * NL));
    HIPCHK(h, launch_latent_seed(st, dec || decf ? b.Rc : nullptr, wl, N, L, h->Cd, aux->z, aux->pm, aux->plv, b.z[T], b.pm,
                                 m_all + (size_t)T * NL, v_all + (size_t)T * NL, L, jT >= 0 ? frame_cot(fr, 0, jT, NL) : nullptr,
                                 jT >= 0 ? frame_cot(fr, 4, jT, NL) : nullptr, jT >= 0 ? frame_cot(fr, 5, jT, NL) : nullptr));
    // every other listed evaluation: decoded again from the saved z_i with the launches the forward ran (they overwrite V, the
    // activations, dec_out and g), rendering backward, ONE decoder pass with factor 1, seeds from (z_i, mu_i); mu_i is the first L
    // of every row of the saved refinement input latent[i], written from buf.pm before the head moved it on
    for (int j = 0; j < fr->n; ++j) {
        const int i = fr->idx[j];
        if (i == T) continue;
        const float *c_mean = frame_cot(fr, 1, j, NP * 3), *c_mask = frame_cot(fr, 2, j, NP), *c_logits = frame_cot(fr, 3, j, NP),
                    *c_z = frame_cot(fr, 0, j, NL), *c_pm = frame_cot(fr, 4, j, NL), *c_plv = frame_cot(fr, 5, j, NL);
        const bool deci = c_mean || c_mask || c_logits;
        if (!deci && !c_z && !c_pm && !c_plv) continue;
        if (deci) {
            HIPCHK(h, launch_dec_v(st, nullptr, nullptr, nullptr, b.z[i], h->dec.wcls, nullptr, b.V, N, L, h->Cd));
            if (int r = decoder_forward(h, st, N, b.z[i])) return r;
            PROF(h, st, "render_bwd", launch_render_bwd_logits(st, b.dec_out, nullptr, c_mask, c_mean, c_logits, b.g, B, h->K, h->P,
                                                               h->opt.precision == 0));
            if (int r = decoder_backward_data(h, st, N, &dpre0, true, 1.f, i, true)) return r;
        }
        HIPCHK(h, launch_latent_seed(st, deci ? b.Rc : nullptr, wl, N, L, h->Cd, c_z, c_pm, c_plv, b.z[i], b.latent[i],
                                     m_all + (size_t)i * NL, v_all + (size_t)i * NL, 4 * L));
        if (i == 0) { s.seed0_m = m_all; s.seed0_v = v_all; }
    }
    s.seed_m = m_all + NL; s.seed_v = v_all + NL; s.seed_stride = NL;
    if (s.seed0_m && !h->calls.fwd_from_state) {
        // lambda_0 = init_mean / init_logvar repeated over (B, K): column sums, factor 1 (from a state: state_grads)
        HIPCHK(h, launch_colsum(st, s.seed0_m, N, L, L, 1.f, h->gacc[ps.init_mean]));
        HIPCHK(h, launch_colsum(st, s.seed0_v, N, L, L, 1.f, h->gacc[ps.init_logvar]));
    }
    return IODINE_OK;
}

// 1. Auxiliary cotangents (iodine.py:171-187,642-651); aux == NULL: the plain backward, nothing to do.  Order of the scaling: what the
// forward accumulated carries the ELBO weights and takes d(out) / d(loss) now, in place (the refinement part is still 0); the auxiliary
// terms join with factor 1; the ELBO seeds of the BPTT are multiplied on the device; the hand-over at the end runs with scale 1.
int aux_seeds(iodine_handle* h, hipStream_t st, const AuxCot* aux, const FrameSet* fr, BpttSeeds& s)
{
    if (!aux) return IODINE_OK;
    HIPCHK(h, launch_scale_dev_add(st, h->gacc_arena, aux->gl, nullptr, (int)h->gacc_total));
    return fr ? aux_seeds_frames(h, st, aux, fr, s) : aux_seeds_final(h, st, aux, s);
}

// 2. The BPTT recurrence of the refinement head over the T iterations.  iodine_train_backward_seq: cotangents on (h_T, c_T) start the
// carries of iteration T - 1, the carries left after iteration 0 are d / d (h_0, c_0) of the state the forward started from
int head_bptt(iodine_handle* h, hipStream_t st, const AuxCot* aux, const Objective& obj, const BpttSeeds& s)
{
    Buffers& b = h->buf;
    const int B = h->calls.fwd_batch, N = B * h->K, T = h->T, L = h->L, H = h->H, Cr = h->Cr;
    const float *cot_h = aux ? aux->lstm_h : nullptr, *cot_c = aux ? aux->lstm_c : nullptr;
    float *gs_h = aux && aux->g_state ? aux->g_state[2] : nullptr, *gs_c = aux && aux->g_state ? aux->g_state[3] : nullptr;
    if (h->opt.head_fused && head_bptt_fits(L, H, Cr)) {
        // the whole BPTT recurrence of the head in one launch (rows are independent: a block walks i = T-1 .. 0 for its rows)
        PROF(h, st, "head_bwd", launch_head_bptt(st, b.g_pm[0], b.g_plv[0], b.gates[0], b.c[0], b.u[0], h->head.raw_wm, h->head.raw_wv, h->head.raw_whh,
                                                 h->head.raw_wih, h->head.raw_mlp_w, b.ddm, b.ddv, b.dgates, b.ds, b.dpooled, T, N, B, L, H, Cr,
                                                 s.seed_m, s.seed_v, aux ? aux->gl : nullptr, obj.wtab, cot_h, cot_c, gs_h, gs_c,
                                                 s.seed_stride));
    } else {
        // the same recurrence as a launch sequence (9 launches per iteration)
        float* const ch[2] = {b.carry_h[0], b.carry_h[1]};
        float* const cc[2] = {b.carry_c[0], b.carry_c[1]};
        HIPCHK(h, launch_head_bptt_unfused(st, b.g_pm[0], b.g_plv[0], b.gates[0], b.c[0], b.u[0], h->head.raw_wm, h->head.raw_wv, h->head.raw_whh, h->head.raw_wih,
                                           h->head.raw_mlp_w, b.ddm, b.ddv, b.dgates, b.ds, b.dpooled, T, N, B, L, H, Cr, aux != nullptr, s.seed_m, s.seed_v,
                                           aux ? aux->gl : nullptr, obj.whost, cot_h, cot_c, gs_h, gs_c, s.seed_stride, b.dc1, b.dxin, ch, cc));
    }
    return IODINE_OK;
}

// 3. d loss / d lambda_0 of the state a forward started from (g_state): d(out) / d(loss) x (-w_0 / B) x d(B ELBO_0) / d lambda_0 - the term
// the forward hands to init_mean / init_logvar as a column sum when it starts from them.  Nothing else reaches lambda_0: lambda_1 =
// detach(lambda_0) + delta_0, and the refinement inputs are detached (iodine.py:343,642-643)
int state_grads(iodine_handle* h, hipStream_t st, const AuxCot* aux, const Objective& obj, const BpttSeeds& s)
{
    if (!(aux && aux->g_state)) return IODINE_OK;
    Buffers& b = h->buf;
    const int B = h->calls.fwd_batch, N = B * h->K, T = h->T, L = h->L;
    const float alpha0 = obj.whost ? -obj.whost[0] / (float)B : -(1.f / (float)(T + 1)) / (float)B;
    float* const dst[2] = {aux->g_state[0], aux->g_state[1]};
    const float* const src[2] = {b.g_pm[0], b.g_plv[0]};
    const float* const add0[2] = {s.seed0_m, s.seed0_v};         // cotangents on evaluation 0 (iodine_train_backward_frames), unscaled
    for (int j = 0; j < 2; ++j) {
        if (!dst[j]) continue;
        HIPCHK(h, launch_scale(st, src[j], alpha0, dst[j], N * L));
        HIPCHK(h, launch_scale_dev_add(st, dst[j], aux->gl, add0[j], N * L));
    }
    return IODINE_OK;
}

// 4. Weight gradients of the head: sums over the iterations of X_i^T D_i = ONE GEMM per parameter over all T * N rows
// (the per-iteration operands lie back to back: c[1..T], xin[0..T-1], h[0..T-1], pooled[0..T-1] and ddm / ddv / dgates / ds)
int head_weight_grads(iodine_handle* h, hipStream_t st)
{
    Buffers& b = h->buf;
    const ParamSlots& ps = h->slot;
    const int L = h->L, H = h->H, Cr = h->Cr, IN = H + 4 * L, R = h->T * h->calls.fwd_batch * h->K;
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
    return IODINE_OK;
}

// 6. (5: refine_stack_backward, iodine_dispatch.cpp)  The accumulators to the caller's buffers: one launch where they lie back to back in the
// same order, else one per parameter asked for
int emit_param_grads(iodine_handle* h, hipStream_t st, float out_scale, const float* out_scale_dev, float* const* param_grads, int accumulate)
{
    bool flat = true;                                          // caller's gradients back to back in the same order?
    for (size_t p = 0; p < h->params.size() && flat; ++p)
        flat = param_grads[p] && param_grads[p] == param_grads[0] + (h->gacc[p] - h->gacc_arena);
    if (flat) {
        HIPCHK(h, launch_axpy_dev(st, h->gacc_arena, out_scale, out_scale_dev, param_grads[0], (int)h->gacc_total, accumulate));
        return IODINE_OK;
    }
    for (size_t p = 0; p < h->params.size(); ++p) {
        if (!param_grads[p]) continue;
        HIPCHK(h, launch_axpy_dev(st, h->gacc[p], out_scale, out_scale_dev, param_grads[p], (int)h->params[p].numel(), accumulate));
    }
    return IODINE_OK;
}

}  // namespace

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
        BpttSeeds s;
        if (int r = aux_seeds(h, st, aux, fr, s)) return r;
        if (int r = head_bptt(h, st, aux, obj, s)) return r;
        if (int r = state_grads(h, st, aux, obj, s)) return r;
        if (int r = head_weight_grads(h, st)) return r;
        if (int r = refine_stack_backward(h, st, h->T * h->calls.fwd_batch * h->K, h->calls.fwd_split)) return r;
        return emit_param_grads(h, st, aux ? 1.f : grad_scale, aux ? nullptr : grad_scale_dev, param_grads, accumulate);   // (aux: d(out) / d(loss) was applied in aux_seeds)
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

}  // extern "C"
