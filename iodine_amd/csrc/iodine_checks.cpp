// The host-only refusals of the entry points, shared by the compute handle and the padded boundary (iodine_pad.cpp): nothing here launches,
// allocates or changes state.  Declarations and the contract: iodine_internal.h.
#include "iodine_internal.h"

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
    if (traj && h->opt.stop_after >= 0 && h->opt.stop_after <= h->T)
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
    if (!h->calls.fwd_done && h->calls.form_changed)
        return h->fail(IODINE_ERR_STATE, "iodine_train_backward: option joint_likelihood changed after the forward pass, which discarded it - "
                                         "run the forward again in the form its backward is wanted in");
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
    if (h->calls.diff_kind != kind && h->calls.form_changed)
        return h->fail(IODINE_ERR_STATE, std::string(who) + ": option joint_likelihood changed after the forward pass, which discarded it - run "
                                             "the forward again in the form its backward is wanted in");
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
