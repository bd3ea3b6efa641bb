// The entry points of the compute handle of libiodine_hip.so that are neither its life cycle nor the training step: settings and options,
// the inference calls (reconstruct, decode, scene edit, predictive, elbo), the backward of a saved decode / elbo, the iodine_last_* readers,
// logger scalars, debug copy and profile read.  See include/iodine_hip.h for the ABI and the reference call sites each entry point replaces.
// The rest of the host layer: iodine_dispatch.cpp - path selectors and launch sequences; iodine_plan.cpp - parameter table, workspace plan,
// graph key; iodine_checks.cpp - the host-only refusals; iodine_params.cpp - create / destroy / set_params; iodine_train.cpp - the training
// forward and backward; iodine_pad.cpp - handles at a padded width; iodine_ops.cpp - the product entry points that
// take no handle; iodine_testops.cpp - the kernel-test entries (iodine_op_*); iodine_sheet.cpp - decomposition sheets.
#include "iodine_internal.h"

extern "C" {

int iodine_abi_version(void) { return IODINE_ABI_VERSION; }

const char* iodine_last_error(const iodine_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

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
    if (!strcmp(key, "stop_after_iters")) { h->opt.stop_after = (int)value; return IODINE_OK; }
    if (!strcmp(key, "profile")) { h->opt.profile = (int)value; return IODINE_OK; }
    if (!strcmp(key, "graph")) { h->opt.graph = value != 0; if (!h->opt.graph) drop_graphs(h); return IODINE_OK; }
#ifdef IODINE_XSKIP_HOOK
    if (!strcmp(key, "xskip")) { g_iod_xskip = (int)value; return IODINE_OK; }       // timing-only ablation builds (common.h)
#endif
    if (!strcmp(key, "out_bwd_fused")) { h->opt.out_bwd_fused = value != 0; return IODINE_OK; }
    if (!strcmp(key, "save_for_backward")) { h->opt.save_bwd = value != 0; return IODINE_OK; }
    if (!strcmp(key, "fuse_l0")) { h->opt.fuse_l0 = value != 0; return IODINE_OK; }
    if (!strcmp(key, "sigma_grad")) { h->opt.sigma_grad = value != 0; return IODINE_OK; }
    if (!strcmp(key, "input_grad")) {
        if (value != 0 && value != 1 && value != 2 && value != 3) return h->fail(IODINE_ERR_INVALID, "option input_grad: 0, 1 (image), 2 (pixel weights) or 3 (both)");
        h->opt.input_grad = (int)value;                    // (the next compute call re-plans the workspace: ensure_workspace keys on it)
        return IODINE_OK;
    }
    if (!strcmp(key, "stable_encoding")) { h->opt.stable_enc = value != 0; return IODINE_OK; }
    if (!strcmp(key, "joint_likelihood")) {
        if (value != 0 && value != 1) return h->fail(IODINE_ERR_INVALID, "option joint_likelihood: 0 (a mixture per colour channel, the reference) or 1 (one mixture per pixel over RGB)");
        // a saved pass ran in the other form and iodine_train_backward_frames decodes earlier evaluations again: it is discarded, not mixed
        if (h->opt.joint_ll != (int)value && (h->calls.fwd_done || h->calls.diff_kind)) { h->calls.saved_passes_gone(); h->calls.form_changed = true; }
        h->opt.joint_ll = (int)value;
        return IODINE_OK;
    }
    if (!strcmp(key, "refine_split")) { h->opt.refine_split = value != 0; return IODINE_OK; }
    if (!strcmp(key, "head_fused")) { h->opt.head_fused = value != 0; return IODINE_OK; }
    if (!strcmp(key, "refine_bwd_fused")) { h->opt.refine_bwd_fused = value != 0; return IODINE_OK; }
    if (!strcmp(key, "profile_stride")) {
        if (value < 1) return h->fail(IODINE_ERR_INVALID, "profile_stride must be >= 1");
        h->opt.profile_stride = (int)value; return IODINE_OK;
    }
    if (!strcmp(key, "head_mfma")) { h->opt.head_mfma = value != 0; return IODINE_OK; }
    if (!strcmp(key, "refine_l0_fused")) { h->opt.refine_l0_fused = value != 0; return IODINE_OK; }
    if (!strcmp(key, "refine_ws")) { h->opt.refine_ws = value != 0; return IODINE_OK; }
    if (!strcmp(key, "dec_out_rows")) { h->opt.dec_out_rows = value != 0; return IODINE_OK; }
    if (!strcmp(key, "wgrad_accum")) {
        if (h->opt.wgrad_accum != (value != 0)) { h->buf = Buffers(); h->calls.arena_gone(); }   // the arena is re-planned
        h->opt.wgrad_accum = value != 0; return IODINE_OK;
    }
    if (!strcmp(key, "conv_variant")) {
        if (value != 1 && value != 6) return h->fail(IODINE_ERR_INVALID, "conv_variant must be 1 (LDS-tiled) or 6 (weight-stationary)");
        if (((int)value == 6) != (h->opt.variant == 6)) h->params_set = false;   // the other kernel's weight packs are not kept up to date
        h->opt.variant = (int)value;
        return IODINE_OK;
    }
    if (!strcmp(key, "conv_precision")) {
        if (value != 0 && value != 1 && value != 2)
            return h->fail(IODINE_ERR_INVALID, "conv_precision must be 0 (f32), 1 (f16x3) or 2 (f16x3 with single-product fp16 weight-stationary decoder convs)");
        // the other path's weight packs are not kept up to date (1 and 2 read the same packs; a switch between them invalidates the parameters
        // all the same, so that a saved forward pass is never finished at another precision)
        if (h->opt.precision != (int)value) h->params_set = false;
        h->opt.precision = (int)value;
        return IODINE_OK;
    }
    if (!strcmp(key, "gen_conv_precision")) {
        if (value != 0 && value != 1) return h->fail(IODINE_ERR_INVALID, "gen_conv_precision must be 0 (f32) or 1 (f16x3)");
        if (h->opt.gen_precision != (int)value) h->params_set = false;    // the split packs are built by iodine_set_params
        h->opt.gen_precision = (int)value;
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
    const bool partial = h->opt.stop_after >= 0 && h->opt.stop_after <= T;     // debug: stop before the final sample/decode
    const int n_it = partial ? h->opt.stop_after : T;
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
            HIPCHK(h, launch_posterior_init(st, h->head.init_mean, h->head.init_logvar, b.pm, b.plv, b.h[0], b.c[0], N, h->L, h->H));
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
            HIPCHK(h, launch_dec_v(st, b.pm, b.plv, eps + (size_t)T * eps_stride, nullptr, h->dec.wcls, b.z[T], b.V, N, h->L, h->Cd));
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
    h->calls.enc_valid = n_it > 0 && (h->opt.stop_after >= 0 || !ref_form(h).l0f);
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
    const bool save = h->opt.save_bwd != 0;                    // option save_for_backward: keep what iodine_decode_backward reads (workspace mode 2)
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
        HIPCHK(h, launch_dec_v(st, nullptr, nullptr, nullptr, z, h->dec.wcls, nullptr, b.V, N, h->L, h->Cd));
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
    HIPCHK(h, launch_dec_v(st, nullptr, nullptr, nullptr, z, h->dec.wcls, nullptr, b.V, batch * K, L, h->Cd));
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
            HIPCHK(h, launch_dec_v(st, nullptr, nullptr, nullptr, b.z[0], h->dec.wcls, nullptr, b.V, rows, L, h->Cd));
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
    const float *pm = post_mean ? post_mean : h->head.init_mean, *plv = post_mean ? post_logvar : h->head.init_logvar;
    const int per_chunk = W / B;                           // >= 1 whole samples per chunk
    for (int s0 = 0; s0 < n_samples; s0 += per_chunk) {
        const int n_s = std::min(per_chunk, n_samples - s0);
        float* zc = z ? z + (size_t)s0 * N * L : b.z[0];  // (buf.z[0] holds W K rows)
        HIPCHK(h, launch_predictive_sample(st, pm, plv, eps + (size_t)s0 * N * L, zc, n_s, N, L, post_mean ? L : 0));
        HIPCHK(h, launch_dec_v(st, nullptr, nullptr, nullptr, zc, h->dec.wcls, nullptr, b.V, n_s * N, L, h->Cd));
        if (int r = decoder_forward(h, st, n_s * N, zc, b.g)) return r;
        PROF(h, st, "predictive", launch_predictive_accum(st, b.g, like ? b.x4 : nullptr, B, K, h->P, s0, n_s, s_pm, s_p2, s_mm, s_m2, s_vt, b.part,
                                                         like ? ll + (size_t)s0 * B : nullptr, (float)h->obj.sigma, h->opt.precision == 0, h->opt.joint_ll));
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
    const bool save = h->opt.save_bwd != 0;                    // option save_for_backward: keep what iodine_elbo_backward reads (workspace mode 2)
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
            HIPCHK(h, launch_posterior_init(st, h->head.init_mean, h->head.init_logvar, b.pm, b.plv, b.h[0], b.c[0], N, h->L, h->H));
        }
        const int r = elbo_and_gradients(h, st, B, eps, 0, false, false, 0.f, save && h->opt.sigma_grad, save ? h->opt.input_grad : 0, 1.f / (float)B);
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
    cs.sgrad_n = save && h->opt.sigma_grad ? 1 : 0;
    cs.ig_bits = save ? h->opt.input_grad : 0; cs.ig_frames = 0; cs.ig_wpf = 0;
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
        PROF(h, st, "render_bwd", launch_render_bwd(st, b.dec_out, g_pred, g_mask, g_mean, b.g, B, h->K, h->P, h->opt.precision == 0));
        float* dpre0 = nullptr;
        // ONE decoder pass with factor 1: data gradient down to the class sums of the broadcast layer, every decoder weight gradient on the way
        const int r = decoder_backward_data(h, st, N, &dpre0, flat_grads != nullptr, 1.f, 0, true);
        if (r) return r;
        if (dz)
            HIPCHK(h, launch_dz_plain(st, b.Rc, dec_path(h) == DEC_GENERIC ? h->gen.ident : h->dec.wclsT, N, h->L, h->Cd, dz, nullptr, nullptr, nullptr,
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
        HIPCHK(h, launch_dz_plain(st, b.Rc, dec_path(h) == DEC_GENERIC ? h->gen.ident : h->dec.wclsT, N, h->L, h->Cd, nullptr, b.pm, b.plv, b.latent[0],
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
                                     h->opt.precision == 0, h->opt.joint_ll));
    return IODINE_OK;
}

int iodine_logger_scalars(iodine_handle* h, void* stream, float* out2)
{
    if (!h || !out2) return IODINE_ERR_INVALID;
    if (h->shim) return pad_logger_scalars(h, stream, out2);
    if (!h->params_set) return h->fail(IODINE_ERR_STATE, "iodine_set_params has not been called");
    HIPCHK(h, launch_mean2((hipStream_t)stream, h->head.init_mean, h->head.init_logvar, h->Lreal > 0 ? h->Lreal : h->L, out2));
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
