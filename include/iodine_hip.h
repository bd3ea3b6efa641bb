/* libiodine_hip.so -- C ABI of the MI355X-native (gfx950) IODINE refinement step.
 *
 * The reference (zhixuan-lin/IODINE) has no FFI: its boundary for this path is the
 * nn.Module protocol of lib/modeling/iodine.py as used by lib/engine/train.py:58-65,
 * lib/engine/eval.py:14-28 and lib/eval/ari_eval.py:22.  Each entry point below names the
 * reference interface it replaces.  All pointers named *_dev / x / eps / outputs are DEVICE
 * pointers owned by the caller (torch); `stream` is a hipStream_t (pass
 * torch.cuda.current_stream().cuda_stream).  Nothing throws across this ABI: every call
 * returns an int status and iodine_last_error() gives the message.
 *
 * Layouts at the boundary are the reference's: images (B,3,S,S) NCHW fp32 in [0,1] (or, with iodine_set_frames, clips (B,E,3,S,S));
 * eps (T+1,B,K,L) standard normals, one slice per Gaussian.sample call
 * (iodine.py:620-634); parameters in state_dict order with state_dict shapes (OIHW convs).
 * A handle is bound to one device and is NOT re-entrant (neither is the reference module,
 * iodine.py:36-52); use one handle per (device, stream).
 */
#ifndef IODINE_HIP_H
#define IODINE_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IODINE_OK 0
#define IODINE_ERR_INVALID 1       /* bad argument / unsupported configuration */
#define IODINE_ERR_HIP 2           /* a HIP runtime call or kernel launch failed */
#define IODINE_ERR_STATE 3         /* call order violated (params not set, no forward before backward ...) */
#define IODINE_ERR_WORKSPACE 4     /* caller-provided workspace too small */

#define IODINE_ABI_VERSION 3

/* bit i set <=> the i-th entry of ARCH.ENCODING is enabled; order = code order of
 * IODINE.get_input_encoding (iodine.py:253-340).  Accepted: IODINE_ENC_FULL (every shipped IODINE config) and any list that keeps
 * 'posterior' and 'grad_post' and at least one image-shaped entry - in particular the reference's DEFAULT list
 * (lib/config/defaults.py:57-80: everything but 'coordinate', 15 input channels).  The first refinement layer's weight then has
 * that many input channels; absent channels are zero weights inside the library.  Lists without both latent entries are
 * rejected with a message, never approximated. */
#define IODINE_ENC_POSTERIOR      (1u << 0)
#define IODINE_ENC_GRAD_POST      (1u << 1)
#define IODINE_ENC_IMAGE          (1u << 2)
#define IODINE_ENC_MEANS          (1u << 3)
#define IODINE_ENC_MASK           (1u << 4)
#define IODINE_ENC_MASK_LOGITS    (1u << 5)
#define IODINE_ENC_MASK_POSTERIOR (1u << 6)
#define IODINE_ENC_GRAD_MEANS     (1u << 7)
#define IODINE_ENC_GRAD_MASK      (1u << 8)
#define IODINE_ENC_LIKELIHOOD     (1u << 9)
#define IODINE_ENC_LEAVE_ONE_OUT  (1u << 10)
#define IODINE_ENC_COORDINATE     (1u << 11)
#define IODINE_ENC_FULL           0xFFFu

/* Mirror of the ARCH.* node read by IODINE.__init__ (iodine.py:8-32; defaults lib/config/defaults.py:35-100). */
typedef struct iodine_config {
    int dim_latent;        /* ARCH.DIM_LATENT  (2..256; widths that are not multiples of 4 run zero-padded inside, same shapes at this boundary) */
    int iters;             /* ARCH.ITERS       */
    int slots;             /* ARCH.SLOTS       (1..16) */
    int img_size;          /* ARCH.IMG_SIZE    (multiples of 16: tuned kernels; other sizes >= 8: generic fallback path) */
    int img_channels;      /* ARCH.IMG_CHANNELS (3) */
    double sigma;          /* ARCH.SIGMA       */
    int layernorm;         /* ARCH.LAYERNORM   */
    int stop_gradient;     /* ARCH.STOP_GRADIENT (stored, unused: iodine.py:21 has no caller) */
    unsigned encoding;     /* ARCH.ENCODING as IODINE_ENC_* bits (see above for what is accepted) */
    int ref_conv_chan;     /* ARCH.REF.CONV_CHAN   (32 or 64: tuned kernels; other divisors of 256: generic fallback path) */
    int ref_conv_layers;   /* ARCH.REF.CONV_LAYERS */
    int ref_mlp_units;     /* ARCH.REF.MLP_UNITS   (1..1024, above about 356 only widths that are a multiple of 8 once rounded up to a multiple of 4: iodine_create names the bound; not a multiple of 4: zero-padded inside, iodine_debug_copy then shows the padded widths) */
    int ref_kernel_size;   /* ARCH.REF.KERNEL_SIZE (3: tuned kernels; 5, 7: generic fallback path, kernels_generic.hip) */
    int ref_stride;        /* ARCH.REF.STRIDE      (2: tuned kernels; 1, 3 .. 8: the refinement stack on the generic path) */
    int dec_conv_chan;     /* ARCH.DEC.CONV_CHAN   (32 or 64: tuned kernels; other multiples of 4 in 8..256: generic path) */
    int dec_conv_layers;   /* ARCH.DEC.CONV_LAYERS (>= 1) */
    int dec_kernel_size;   /* ARCH.DEC.KERNEL_SIZE (3: tuned kernels; 5 - the reference's default - and 7: generic path) */
} iodine_config;

typedef struct iodine_handle iodine_handle;

int iodine_abi_version(void);

/* IODINE(ARCH) -- iodine.py:8-52.  Builds the parameter table and the packed-weight buffers on the
 * current HIP device.  On failure *out is NULL and iodine_last_error(NULL) holds the reason.
 * iodine_last_error(NULL) returns the message of the CALLING THREAD's last failed iodine_create or handle-free call (valid until that
 * thread's next such failure); with a handle, the message of the handle's last failure (a handle is used from one thread at a time). */
int iodine_create(const iodine_config* cfg, iodine_handle** out);
void iodine_destroy(iodine_handle* h);
const char* iodine_last_error(const iodine_handle* h);

/* model.named_parameters() / state_dict() surface (lib/solver/build.py:10-14, lib/utils/checkpoint.py:43,68). */
int iodine_num_params(const iodine_handle* h);
int iodine_param_info(const iodine_handle* h, int index, const char** name, int* ndim, long long dims[4]);

/* load_state_dict / "parameters changed" notification: repacks every weight into the kernels' layouts
 * (NHWC/MFMA quads, border-class sums and coordinate map of the broadcast layer, transposed head weights).
 * dev_ptrs[i] is the i-th parameter (state_dict order, reference shapes, contiguous fp32). */
int iodine_set_params(iodine_handle* h, void* stream, const float* const* dev_ptrs, int n);

/* Workspace: mode 0 = inference (reconstruct/decode/elbo), 1 = training, 2 = decoder backward: what a decode / elbo that runs with
 * option "save_for_backward" and its iodine_decode_backward / iodine_elbo_backward need - the inference carve-up plus the scratch of
 * ONE weight-gradient pass of the decoder (partial tiles, fold scratch, the broadcast layer's slot-summed maps); at the same shape
 * bytes(0) <= bytes(2) <= bytes(1).  If no workspace is installed the library allocates one itself on first use (never inside the
 * refinement loop). */
size_t iodine_workspace_bytes(const iodine_handle* h, int batch, int mode);
int iodine_set_workspace(iodine_handle* h, void* dev_ptr, size_t bytes);

/* model.K = slots; model.n_iters = iters -- the reference reads both attributes on every call (Gaussian.init_unit(B, self.K),
 * get_input_encoding's repeat over K, the loops of encode / forward: iodine.py:81-83,123-126,279,312); no parameter depends on
 * them.  Sets the RUN shape of every following compute call (reconstruct, decode, elbo, train_forward); the constructor's
 * SLOTS / ITERS are the initial one.  slots in 1..16, iters >= 1.  iodine_workspace_bytes, the workspace plan, the per-call
 * 32-bit size checks, "stop_after_iters" and the kernel selection follow it; a compute call whose installed workspace is too
 * small for it returns IODINE_ERR_WORKSPACE.  A change while a training forward is pending discards it (the backward then
 * returns IODINE_ERR_STATE).  iodine_last_elbo_outputs / iodine_last_posterior / iodine_debug_copy keep reading the state of the
 * last call at the shape that call ran with.  Buffers with a slot or iteration axis (eps, outputs, z, the posterior) are sized by
 * the run shape of the call they are passed to. */
int iodine_set_run_shape(iodine_handle* h, int slots, int iters);

/* Video input: one frame per ELBO evaluation (the reference closes encode / forward over ONE x, iodine.py:73-105,115-158; nothing in the
 * math needs that).  frames = 0 - default: x of iodine_reconstruct / iodine_train_forward is (B,3,S,S).  frames = E > 0: x is a clip
 * (B,E,3,S,S), batch first as a loader of clips yields it, and ELBO evaluation i of the call uses x[:, i] for the likelihood, the
 * closed-form inner gradients and the image-shaped channels of the refinement input.  E must equal the evaluations the call makes - T for
 * iodine_reconstruct (its final sample + decode involves no image), T + 1 for iodine_train_forward (the loss stays
 * -sum_i (i+1)/(T+1) ELBO_i, ELBO_i against frame i; the backward never reads x); any other count is IODINE_ERR_INVALID with a message
 * naming the expected shape, before any launch - never clamped or repeated.  A setting like the run shape: it holds until changed,
 * iodine_workspace_bytes, the workspace plan (the converted frames, [E][B][P][4], +16 bytes per pixel and frame) and the hipGraph key
 * follow it, and a change while a training forward is pending discards it.  iodine_elbo takes one image (B,3,S,S) at any setting.
 * E identical frames give the bits of the single-image call. */
int iodine_set_frames(iodine_handle* h, int frames);

/* model.sigma, and the two weights the reference hard-codes -- the objective of every following compute call (reconstruct, elbo,
 * train_forward; decode does not depend on it).  The reference reads self.sigma on every elbo() call (iodine.py:210); beta is the KL weight
 * as if iodine.py:223 read `elbo = log_likelihood - beta * kl`; iter_weights are the per-evaluation loss weights as if iodine.py:152-153
 * used them instead of (i + 1) / (T + 1).  The constructor's ARCH.SIGMA, beta = 1 and the default weighting are the initial objective.
 *   sigma > 0: the likelihood, the closed-form pixel gradients and the likelihood-shaped channels of the refinement input.
 *   beta >= 0: the ELBO a call returns (elbo_iter[:, 0], terms[0], the loss), the -dKL / dlambda part of the inner gradient
 *     d(B * ELBO) / d lambda -- a refinement input, through the latent layer-norm, so the inference trajectory follows it -- and every
 *     outer gradient.  elbo_iter[:, 1:3], terms[1:3] and a trajectory's kl / ll stay the raw KL and log-likelihood.
 *   iter_weights: n_weights finite numbers >= 0, not all zero (after rounding to fp32), copied by the call; n_weights = 0 (iter_weights may
 *     be NULL) = the default (i + 1) / (T + 1), which keeps its closed form -- the launches and the arithmetic of a handle that never called
 *     this entry.  A table is read by iodine_train_forward only, where n_weights must equal T + 1 of the run shape: otherwise that call
 *     returns IODINE_ERR_INVALID naming both numbers (checked there, not here: the run shape may still change).  A weight of 0 is allowed
 *     anywhere: the evaluation still runs -- later iterations depend on it -- and adds nothing to the loss or the gradients.
 * A setting like the run shape: it holds until changed; invalid arguments are IODINE_ERR_INVALID and leave it as it was.  Unlike the run
 * shape a change does NOT discard a pending forward: iodine_train_backward* / iodine_train_backward_aux / iodine_elbo_backward differentiate
 * the saved pass with the objective IT ran with.  Call with the handle's device current (a new weight table is a small device allocation
 * of the handle, uploaded synchronously; tables are never rewritten, so queued work keeps reading the one it was given).  The hipGraph key
 * of option "graph" carries the bit patterns of sigma and beta and the identity of the weight table. */
int iodine_set_objective(iodine_handle* h, double sigma, double beta, const double* iter_weights, int n_weights);

/* Per-pixel observation weights w >= 0 of the likelihood, for the NEXT compute call that takes x:
 *     LL = mean_b sum_p w_p sum_c logsumexp_k(log(m_k + 1e-12) + l_kc),   ELBO = LL - beta * KL
 * (iodine.py:213-220 with w in front of the pixel sum; NOT normalised by sum(w) or mean(w)).  w_dev: device pointer, fp32, (B,S,S) with
 * per_frame = 0 -- with a clip (iodine_set_frames) the same weights for every frame -- or (B,E,S,S) with per_frame = 1, frame i weighting
 * ELBO evaluation i.  NULL = no weights.  per_frame = 1 while the frames setting is 0 is IODINE_ERR_INVALID (host only, nothing is set).
 *   weighted:      the LL / ELBO a call reports (elbo_iter[:, 0] and [:, 2], terms[0] and terms[2], the loss, iodine_logger_scalars'
 *                  likelihood, a trajectory's per-image ll); the closed-form gradients d(B * ELBO) / d mean and / d mask and with them
 *                  everything downstream, as autograd gives for the weighted objective: grad_post, the layer-normed gradient channels
 *                  9 - 12 of the refinement input (normalised from the weighted gradients), every outer gradient.
 *   not weighted:  the channels that describe the scene -- 8 mask_posterior, 13 likelihood, 14 leave_one_out_likelihood --, the image
 *                  channels, and the KL.
 * ONE-SHOT: the pointer is consumed by the next iodine_reconstruct[_seq] / iodine_elbo / iodine_train_forward[_seq] and cleared by it,
 * whether that call succeeds or is refused, so a stale pointer is never read; the call after it runs unweighted unless this entry is
 * called again.  iodine_decode takes no x and neither reads nor clears it.  The memory is the caller's: it is read on the compute call's
 * stream (packed next to the image, no extra buffer) and must stay valid until that work has run -- with option "graph" for as long as
 * the call is replayed: the pointer and the flag are part of the hipGraph key.  The backward passes need nothing: they differentiate
 * what the forward saved.  Values are the caller's contract -- finite, >= 0, not checked on the device; zeros are allowed, an image of
 * all zeros included (its gradients are exactly 0).  Weights are data: they receive no gradient.  A call without weights, and a call
 * whose weights are all 1, compute the bits of a library that never had this entry (the multiply is by an exact 1). */
int iodine_set_pixel_weights(iodine_handle* h, const float* w_dev, int per_frame);

/* pred, mask, mean = model.reconstruct(x) -- iodine.py:107-112 (encode :73-105 + decode :59-71).
 * Outputs (any may be NULL): pred (B,3,S,S), mask (B,K,1,S,S), mean (B,K,3,S,S) NCHW; z (B,K,L) = the final
 * sample; post_mean / post_logvar (B,K,L) = lambda after T updates; elbo_iter (T,3) = {ELBO, KL, LL} of each
 * elbo() call, batch means exactly as iodine.py:193,220,223. */
int iodine_reconstruct(iodine_handle* h, void* stream, int batch, const float* x, const float* eps,
                       float* pred, float* mask, float* mean, float* z, float* post_mean, float* post_logvar,
                       float* elbo_iter);

/* iodine_reconstruct with two optional additions (both NULL: the same call, launch for launch).
 *
 * state_in: {post_mean, post_logvar (B,K,L), h, c (B,K,MLP_UNITS)} - the refinement starts from this (lambda, LSTM state) instead of
 * Gaussian.init_unit + zeros (iodine.py:81-83) and runs T further iterations: T = 4 equals T = 2 followed by T = 2 from the state the
 * first call left (post_mean / post_logvar outputs + iodine_last_refine_state), bit for bit, given the matching slices of x and eps.
 * All four pointers are required.  The tensors are sized by (batch, run shape) of THIS call; nothing checks where they came from.
 *
 * traj: {pred (T+1,B,3,S,S), mask (T+1,B,K,1,S,S), mean (T+1,B,K,3,S,S), kl (T,B), ll (T,B)}, iteration first like eps and elbo_iter.
 * Entry j < T = the decode ELBO evaluation j made (the sample from lambda_j, scored against frame j), written by one launch of the final
 * decode's output kernel per iteration; entry T = the final decode = the pred / mask / mean outputs.  kl / ll: the per-image terms whose
 * batch means are elbo_iter[:, 1:3].  All five pointers are required; not available with option stop_after_iters (no final decode). */
int iodine_reconstruct_seq(iodine_handle* h, void* stream, int batch, const float* x, const float* eps,
                           float* pred, float* mask, float* mean, float* z, float* post_mean, float* post_logvar,
                           float* elbo_iter, const float* const* state_in, float* const* traj);

/* The LSTM state (h, c) after the last update of the last iodine_reconstruct / iodine_reconstruct_seq, in torch order as
 * RefinementNetwork.forward returns it (iodine.py:503): lstm_h / lstm_c (count,K,MLP_UNITS) of the first `count` images; either may be
 * NULL.  With iodine_last_posterior this is the state_in of a continuing call.  Any other compute call (decode excepted: it touches
 * neither), a re-planned workspace or iodine_set_workspace discards it: IODINE_ERR_STATE. */
int iodine_last_refine_state(iodine_handle* h, void* stream, int count, float* lstm_h, float* lstm_c);

/* pred, mask, mean = model.decode(z) -- iodine.py:59-71. */
int iodine_decode(iodine_handle* h, void* stream, int batch, const float* z, float* pred, float* mask, float* mean);

/* Scene edits: n_edits renderings of the scene decode(z), each with ONE slot of one image replaced by the decode of another latent or
 * removed -- latent traversals, object removal, slots moved between scenes.  The decoder treats slot-images independently and only the last
 * per-pixel step (softmax over the K slots, pred = sum_k mask x mean) couples the slots of an image, so the call decodes the base once
 * (B x K slot-images), then one slot-image per replace edit and none per removal, and renders every edit with one per-pixel pass over
 * the base and the edit decodes: B K + E slot-image decodes where E calls of iodine_decode on the edited scenes take E K.
 *   z (B,K,L) device, K = the run shape's slot count; image / slot / kind: HOST arrays of n_edits ints -- edit e acts on slot slot[e] of
 *   image image[e]; kind 0 = replace it by decode(z_new[e]), kind 1 = remove it (its logit becomes -inf: the other K - 1 slots are
 *   re-normalised, the removed slot's mask is exactly 0); z_new (n_edits,L) device, row e belongs to edit e, rows of removals are not
 *   read, NULL is allowed when every edit is a removal.
 *   Per edit, each may be NULL: pred (n_edits,3,S,S), mask (n_edits,K,1,S,S), mean (n_edits,3,S,S) = the sigmoid rgb of the slot-image put
 *   into slot slot[e] (of a removal: of the slot that was removed).  base_pred / base_mask / base_mean = the outputs of iodine_decode(z),
 *   each may be NULL.  A replace edit returns the bits iodine_decode returns for the edited z: same decoder kernels, same per-pixel
 *   operation order.
 * chunk_images: the size of the arena in images, >= batch; 0 = batch.  The workspace is planned for inference (mode 0) at
 * W = max(batch, chunk_images) images -- iodine_workspace_bytes(h, W, 0) -- and the edits run in chunks of consecutive edits with at most
 * W K replacements each: per chunk the z_new rows are gathered, decoded in one decoder pass and rendered by launches of at most 256 edits,
 * whose indices travel in the kernel arguments.  No host synchronisation, no allocation, everything on `stream`.
 * IODINE_ERR_INVALID, before anything is launched, with a message that names the offending edit: n_edits < 1, an image outside
 * 0..batch-1, a slot outside 0..K-1, a kind other than 0 / 1, a removal at K = 1, a replacement while z_new is NULL, chunk_images < batch
 * (and non-zero), batch or chunk_images beyond the 2^31 limit of iodine_decode.  The indices are host memory and never reach a kernel unchecked.
 * Call state: the call counts as an iodine_decode at batch W -- a saved training forward or saved decode / elbo is discarded, the LSTM
 * state of the last reconstruct stays -- and, because the base decode is kept in the buffer the last elbo() wrote, iodine_last_elbo_outputs
 * has nothing to read afterwards (IODINE_ERR_STATE), as after a decode under "save_for_backward".  Not differentiable.  The entry is NOT
 * captured under option "graph": its launch sequence depends on the edit list, so it always runs eagerly.  Profile category: "scene_edit"
 * (the per-pixel launches; the decoder passes are booked under the decoder's categories). */
int iodine_scene_edit(iodine_handle* h, void* stream, int batch, const float* z, int n_edits, const int* image, const int* slot, const int* kind,
                      const float* z_new, int chunk_images, float* pred, float* mask, float* mean, float* base_pred, float* base_mask,
                      float* base_mean);

/* Multi-sample evaluation: n_samples draws z_s = mu + exp(logvar/2) * eps[s] from ONE posterior (post_mean / post_logvar (B,K,L); both
 * NULL = the initial posterior, as in iodine_elbo), each decoded, and reduced per pixel WITHOUT writing any sample's planes: running mean
 * and sum of squared deviations (Welford, fp32, in sample order) of the rendered image and of the masks, the number of samples in which
 * each slot wins a pixel, and -- with x -- the per-image weighted log-likelihood of every sample (what the importance-weighted bound and
 * the Monte-Carlo ELBO are built from).  The decoder treats slot-images independently, so the S B K slot-images run on the decoder
 * kernels the path selector picks, unchanged; everything new is one per-pixel kernel that keeps one pixel of one image per thread for all
 * samples of a launch.
 *   eps (n_samples,B,K,L) device; x (B,3,S,S) or NULL.  Outputs, each may be NULL: z (n_samples,B,K,L) -- z[s] is bit for bit what
 *   iodine_elbo(x, post_mean, post_logvar, eps[s]) samples; pred_mean, pred_m2 (B,3,S,S) and mask_mean, mask_m2 (B,K,1,S,S): mean and M2 =
 *   sum_s (v_s - mean)^2 (population variance = M2 / n_samples; exactly 0 for one sample) of the per-sample pred / mask, which are the bits
 *   iodine_decode(z[s]) returns; votes (B,K,S,S) int32: samples whose mask arg-max at the pixel is slot k (the lowest index wins a tie, as in
 *   iodine_slot_table's segmentation map; sums to n_samples over k); ll (n_samples,B) = sum_p w_p sum_c logsumexp_k(..) of sample s and
 *   image b, needs x.  sigma is the objective's (iodine_set_objective), beta plays no part; a pending iodine_set_pixel_weights is
 *   consumed by this call like by any call that reads x.
 * chunk_images: the size of the arena in images, >= batch; 0 = batch.  The workspace is planned for inference (mode 0) at
 * W = max(batch, chunk_images) images -- iodine_workspace_bytes(h, W, 0) -- and the samples run in chunks of floor(W / batch) >= 1 whole
 * samples: per chunk one sampling launch, one decoder pass over n_s B K slot-images and one accumulate launch, which reads the running
 * state from the output buffers and writes it back.  The update is strictly sequential in the sample index, so every output is bitwise
 * independent of chunk_images.  No host synchronisation, no allocation, everything on `stream`; the likelihood is reduced through fp64
 * block partials in a fixed order (no float atomics).
 * IODINE_ERR_INVALID, before anything is launched, with a message that names the argument: n_samples < 1 or above 2^24 (the sample index
 * enters the moments as an fp32 number; int32 votes could wrap only far beyond), eps NULL, one of post_mean / post_logvar without the
 * other, chunk_images < batch (and non-zero), ll without x, batch above 65535, batch or chunk_images beyond the 2^31 limit of iodine_decode.
 * Call state: the call counts as an iodine_decode at batch W -- a saved training forward or saved decode / elbo is discarded, the LSTM
 * state of the last reconstruct stays -- and, because the chunk's samples and the packed image take buffers the last elbo() wrote,
 * iodine_last_elbo_outputs has nothing to read afterwards (IODINE_ERR_STATE), as after iodine_scene_edit.  Not differentiable.  The entry
 * is NOT captured under option "graph": its launch sequence depends on the sample count, so it always runs eagerly.  Profile category:
 * "predictive" (the accumulate launches; the decoder passes are booked under the decoder's categories). */
int iodine_predictive(iodine_handle* h, void* stream, int batch, int n_samples, const float* post_mean, const float* post_logvar,
                      const float* eps, const float* x, int chunk_images, float* z, float* pred_mean, float* pred_m2, float* mask_mean,
                      float* mask_m2, int* votes, float* ll);

/* elbo = model.elbo(x) -- IODINE.elbo, iodine.py:161-241: ONE sample z = mu + exp(logvar/2) * eps from the given posterior
 * (post_mean / post_logvar (B,K,L); both NULL = the initial posterior of Gaussian.init_unit, iodine.py:607-618), decode,
 * mixture log-likelihood and KL.  eps (B,K,L); terms (3) = {ELBO, KL, LL} (device, may be NULL).  The tensors the reference
 * leaves on `self` (z, mean, mask, mask_logits) and the `pred` it hands to the logger are read with
 * iodine_last_elbo_outputs. */
int iodine_elbo(iodine_handle* h, void* stream, int batch, const float* x, const float* post_mean, const float* post_logvar,
                const float* eps, float* terms);

/* Autograd through ONE decode / elbo (in the reference both are plain autograd code: model.decode(z) back-propagates into z and the
 * decoder weights, model.elbo(x).backward() fills the decoder weight gradients and posterior.mean.grad / .logvar.grad,
 * iodine.py:59-71,161-241).  Call order, as for the training pair: set option "save_for_backward" to 1, run iodine_decode /
 * iodine_elbo (same launches and outputs, bit for bit; the workspace is planned in mode 2 and z, the decoder activations and the
 * decoder output stay in it - after such a decode iodine_last_elbo_outputs has nothing to read), then call the matching backward
 * ONCE.  Any compute call in between (reconstruct, decode, elbo, train_forward, a backward), iodine_set_params, a re-planned workspace
 * or a changed run shape discards the saved pass: the backward then returns IODINE_ERR_STATE, as does a second backward or one with
 * nothing to differentiate.
 *
 * iodine_decode_backward: g_pred (B,3,S,S), g_mask (B,K,1,S,S), g_mean (B,K,3,S,S) = the caller's gradients wrt the three outputs of
 * the saved decode, NCHW, any of them NULL = zero.  Rendering backward, ONE decoder pass (data + every weight gradient), then
 * dz (B,K,L) = d / dz (may be NULL) and flat_grads (may be NULL; the layout of iodine_train_backward_flat: all parameters back to
 * back) = (accumulate ? flat_grads : 0) + d / d params.  Only decoder.* can be non-zero: the other parameters receive 0 when not
 * accumulating and are not touched when accumulating. */
int iodine_decode_backward(iodine_handle* h, void* stream, int batch, const float* g_pred, const float* g_mask, const float* g_mean,
                           float* dz, float* flat_grads, int accumulate);

/* model.elbo(x).backward() for the saved iodine_elbo.  grad_out_dev: autograd's incoming d(out) / d(ELBO), one float in DEVICE memory
 * (NULL = 1; read by the final writes, no host round trip).  g_post_mean / g_post_logvar (B,K,L; either may be NULL) = grad_out x
 * d ELBO / d (post_mean, post_logvar) with the batch-mean convention of iodine.py:193,220: (dz - mu) / B and
 * (dz * 1/2 exp(logvar / 2) eps - 1/2 (exp(logvar) - 1)) / B, dz = d(B * ELBO) / dz.  flat_grads (may be NULL) as above, times
 * grad_out; when the ELBO sampled from the initial posterior (post_mean = post_logvar = NULL) posterior.init_mean / init_logvar
 * receive the sums of the two posterior gradients over (B, K). */
int iodine_elbo_backward(iodine_handle* h, void* stream, const float* grad_out_dev, float* g_post_mean, float* g_post_logvar,
                         float* flat_grads, int accumulate);

/* self.z / self.mean / self.mask / self.mask_logits and pred of the LAST elbo() call (iodine.py:171-187,225) -- the one made by
 * iodine_elbo, the last refinement iteration of iodine_reconstruct (NOT its final decode: the reference's logger shows the
 * last elbo() call, iodine.py:226-239) or the final elbo of iodine_train_forward -- for the first `count` images of that
 * call's batch: z (count,K,L), mean (count,K,3,S,S), mask and mask_logits (count,K,1,S,S), pred (count,3,S,S); any may be
 * NULL.  count = 1 is what the logger side channel needs. */
int iodine_last_elbo_outputs(iodine_handle* h, void* stream, int count, float* z, float* mean, float* mask,
                             float* mask_logits, float* pred);

/* self.posterior.mean / self.posterior.logvar as the reference's module holds them after the last call (Gaussian.update,
 * iodine.py:636-645, leaves lambda_T on the module after forward / encode; a following model.elbo(x) samples from it,
 * iodine.py:170): post_mean / post_logvar (count,K,L) of the first `count` images of the last refinement call; either may be
 * NULL. */
int iodine_last_posterior(iodine_handle* h, void* stream, int count, float* post_mean, float* post_logvar);

/* loss = model(x) -- IODINE.forward, iodine.py:115-158.  loss (1) and elbo_iter (T+1,3) are device outputs.
 * Keeps what iodine_train_backward needs in the workspace (the autograd graph of the reference). */
int iodine_train_forward(iodine_handle* h, void* stream, int batch, const float* x, const float* eps,
                         float* loss, float* elbo_iter);

/* loss.backward() -- lib/engine/train.py:63.  Accumulates grad_scale * d loss / d param INTO param_grads[i]
 * (+=, like autograd's .grad accumulation; zero_grad is the caller's job, train.py:62).  Consumes the saved forward (autograd
 * without retain_graph): a second call, or a call after any other compute entry point re-used the workspace, returns
 * IODINE_ERR_STATE. */
int iodine_train_backward(iodine_handle* h, void* stream, float grad_scale, float* const* param_grads, int n);

/* The same with the caller's gradients as ONE buffer (parameters back to back in iodine_param_info order -- the layout
 * iodine_amd.IODINE hands to autograd and all-reduces in place) and autograd's incoming d(out)/d(loss) read from DEVICE memory
 * (grad_loss_dev, one float; NULL = 1): flat = (accumulate ? flat : 0) + *grad_loss_dev * d loss / d params.  One launch at the
 * end; no host round trip, no separate zero-fill. */
int iodine_train_backward_flat(iodine_handle* h, void* stream, const float* grad_loss_dev, float* flat_grads, int accumulate);

/* (loss + aux).backward() -- the backward of the saved iodine_train_forward with auxiliary cotangents on what the forward's FINAL elbo()
 * leaves on the reference's module, still attached to the graph (iodine.py:137,171-187,642-651): g_mean (B,K,3,S,S), g_mask and g_logits
 * (B,K,1,S,S), g_z (B,K,L) on self.mean / self.mask / self.mask_logits / self.z, g_post_mean / g_post_logvar (B,K,L) on
 * posterior.mean / posterior.logvar = lambda_T -- the shapes of iodine_last_elbo_outputs / iodine_last_posterior, NCHW, device memory.
 * Every one of them may be NULL (= zero), and so may grad_loss_dev (one float in device memory, autograd's d(out) / d(loss); NULL = 0:
 * only the auxiliary terms).  flat_grads (required; the layout of iodine_train_backward_flat)
 *   = (accumulate ? flat_grads : 0) + *grad_loss_dev * d loss / d params + sum_t <g_t, d t / d params>
 * with the reference's detach points: mean / mask / mask_logits go through the final rendering (mask = softmax(mask_logits): g_mask and
 * g_logits add at the logits) and ONE decoder pass -- the decoder.* gradients -- to z_T = mu_T + exp(logvar_T / 2) eps_T; from there
 * d mu_T = dz + g_post_mean, d logvar_T = dz * 1/2 exp(logvar_T / 2) eps_T + g_post_logvar (no KL term: the final ELBO's KL is part of
 * the loss) seed delta_{T-1} of the back-propagation through the T refinement iterations (lambda_T = detach(lambda_{T-1}) + delta_{T-1},
 * iodine.py:642-643) -- the refine.* gradients; nothing reaches posterior.init_mean / init_logvar on this way (the refinement inputs are
 * detached, iodine.py:343).  The auxiliary terms are NOT multiplied by *grad_loss_dev.  With every g_* NULL and grad_loss_dev given this is
 * iodine_train_backward_flat itself, launch for launch and bit for bit.  The decoder activations of the final evaluation are read where
 * the forward left them (no re-decode).  Consumes the saved forward and is refused with IODINE_ERR_STATE like the two entries above: no
 * forward, a re-planned workspace, a changed run shape, a second backward. */
int iodine_train_backward_aux(iodine_handle* h, void* stream, const float* grad_loss_dev, const float* g_mean, const float* g_mask,
                              const float* g_logits, const float* g_z, const float* g_post_mean, const float* g_post_logvar,
                              float* flat_grads, int accumulate);

/* Training from a carried state: truncated and exact back-propagation through time over a clip that is longer than one call.
 *
 * iodine_train_forward_seq: iodine_train_forward with an optional initial state (state_in NULL: the same call, launch for launch).
 * state_in = {post_mean, post_logvar (B,K,L), h, c (B,K,MLP_UNITS)}, torch order, as iodine_reconstruct_seq takes it; all four pointers are
 * required.  ELBO evaluation 0 samples from the given lambda and the LSTM starts from (h, c) instead of posterior.init_mean / init_logvar and
 * zeros (iodine.py:123-126); the call still makes T + 1 evaluations with the same objective and frames.  T = 4 equals T = 2 followed by
 * T = 2 from the state the first call left (iodine_last_posterior + iodine_last_train_state), evaluation by evaluation and bit for bit, given
 * the matching slices of x and eps; the boundary evaluation is made by both calls (the last of the first, evaluation 0 of the second), so the
 * second call usually runs with iter_weights[0] = 0.  posterior.init_mean / init_logvar are not part of such a forward: its backward hands
 * them nothing (zeros when not accumulating, untouched when accumulating). */
int iodine_train_forward_seq(iodine_handle* h, void* stream, int batch, const float* x, const float* eps, const float* const* state_in,
                             float* loss, float* elbo_iter);

/* The LSTM state (h, c) after the last update of the last iodine_train_forward / iodine_train_forward_seq (the reference keeps it on the
 * module as self.lstm_hidden, iodine.py:37,124,144): lstm_h / lstm_c (count,K,MLP_UNITS) of the first `count` images, torch order; either may
 * be NULL.  With iodine_last_posterior this is the state_in of the call that continues the clip.  It stays readable after the backward of
 * that forward; any other compute call, a re-planned workspace or iodine_set_workspace discards it: IODINE_ERR_STATE.  (A separate entry:
 * iodine_last_refine_state keeps answering for iodine_reconstruct alone, as it always has.) */
int iodine_last_train_state(iodine_handle* h, void* stream, int count, float* lstm_h, float* lstm_c);

/* iodine_train_backward_aux with what crosses the two ends of the saved forward (g_lstm_h, g_lstm_c and g_state all NULL: that entry, bit for
 * bit).
 *   g_lstm_h / g_lstm_c (B,K,MLP_UNITS; either may be NULL = zero): cotangents on the LSTM state after the last update - what
 *     iodine_last_train_state reads, torch order (h = o tanh(c), the read-out layers act on c).  They start the carries of iteration T - 1
 *     of the back-propagation through the head and, like the other auxiliary terms, are NOT multiplied by *grad_loss_dev.
 *   g_state: NULL, or four output pointers {g_post_mean, g_post_logvar (B,K,L), g_h, g_c (B,K,MLP_UNITS)}, each of which may be NULL - the
 *     gradient wrt the state_in the saved iodine_train_forward_seq started from.  The first two are *grad_loss_dev x (-w_0 / B) x
 *     d(B ELBO_0) / d lambda_0 (w_0 = the loss weight of evaluation 0; nothing else reaches lambda_0: lambda_1 = detach(lambda_0) + delta_0
 *     and the refinement inputs are detached, iodine.py:343,642-643), the last two the carries left after iteration 0.  Overwritten, never
 *     accumulated into.  After a forward that ran without a state: IODINE_ERR_STATE with a message, and the saved forward stays.
 * Exact BPTT over chunks: run the chunks' forwards once to collect each chunk's entry state, then walk them in reverse - forward again from
 * the entry state, backward with the cotangents on (lambda_T via g_post_mean / g_post_logvar, h_T, c_T) that the following chunk's g_state
 * returned, accumulate = 1.  Consumes the saved forward and is refused like the entries above. */
int iodine_train_backward_seq(iodine_handle* h, void* stream, const float* grad_loss_dev, const float* g_mean, const float* g_mask,
                              const float* g_logits, const float* g_z, const float* g_post_mean, const float* g_post_logvar,
                              const float* g_lstm_h, const float* g_lstm_c, float* flat_grads, int accumulate, float* const* g_state);

/* Per-frame auxiliary losses: chosen ELBO evaluations of the training forward, attached (the reference leaves self.z / mean / mask /
 * mask_logits and posterior.mean / logvar of EVERY elbo() call of IODINE.forward on the graph; a tracker trained one frame per evaluation
 * puts a loss on each of them).
 *
 * iodine_train_forward_frames: iodine_train_forward_seq (state_in NULL or given) that also writes out what the listed evaluations decoded.
 *   frame_idx: n_frames evaluation indices in HOST memory, ascending, unique, each in 0..T (T = the final evaluation).
 *   frames_out: six device pointers {z (n_frames,B,K,L), mean (n_frames,B,K,3,S,S), mask, mask_logits (n_frames,B,K,1,S,S), post_mean,
 *     post_logvar (n_frames,B,K,L)}, evaluation first, NCHW, like the traj buffers of iodine_reconstruct_seq; each may be NULL.  Entry j is
 *     what evaluation frame_idx[j] decoded and the lambda it sampled z from.
 * n_frames = 0: iodine_train_forward_seq, launch for launch.  Loss, ELBO terms and everything the forward saves are the same bits for any
 * list; per listed evaluation the call adds one rendering launch and three small copies.
 *
 * iodine_train_backward_frames: iodine_train_backward_seq plus cotangents on chosen evaluations (n_frames = 0, or every g_frames pointer
 * NULL: that entry, bit for bit).
 *   frame_idx / n_frames: as above; the list is independent of the forward's (every z_i is kept by a training forward).
 *   g_frames: six device pointers in the order {g_z, g_mean, g_mask, g_logits, g_post_mean, g_post_logvar}, each (n_frames, B, ..) as above
 *     or NULL (= zero).
 * For a listed evaluation i < T the decoder runs again from the saved z_i with the launches the forward ran; the rendering backward of
 * (g_mean, g_mask, g_logits) and ONE decoder pass with factor 1 give the decoder.* gradients and dz_i; d mu_i = dz_i + g_z + g_post_mean,
 * d logvar_i = (dz_i + g_z) * 1/2 exp(logvar_i / 2) eps_i + g_post_logvar (no KL term).  For i >= 1 the two join d loss / d delta_{i-1}
 * (lambda_i = detach(lambda_{i-1}) + delta_{i-1}) and follow the head, the LSTM carries and the refinement convs back to iteration 0; for
 * i = 0 they go to posterior.init_mean / init_logvar as column sums, or - after a forward from a state - are added to g_state[0] / [1], and
 * nothing of them reaches refine.*.  An evaluation whose three image-shaped cotangents are all NULL takes no decoder pass.  Evaluation T
 * takes the path of the final state's cotangents (kept activations, no re-decode); given both ways, the two sets add.  Like them, none of
 * these terms is multiplied by *grad_loss_dev.  Cost: one decoder forward (i < T) and one decoder backward pass per listed evaluation with an
 * image-shaped cotangent.  The re-decode overwrites the decoder output of the final elbo(): iodine_last_elbo_outputs then answers
 * IODINE_ERR_STATE until the next compute call; iodine_last_posterior and iodine_last_train_state stay valid.  Refused before any launch
 * with IODINE_ERR_INVALID: indices out of range, unsorted or repeated, n_frames < 0, a NULL array with n_frames > 0. */
int iodine_train_forward_frames(iodine_handle* h, void* stream, int batch, const float* x, const float* eps, const float* const* state_in,
                                float* loss, float* elbo_iter, const int* frame_idx, int n_frames, float* const* frames_out);
int iodine_train_backward_frames(iodine_handle* h, void* stream, const float* grad_loss_dev, const float* g_mean, const float* g_mask,
                                 const float* g_logits, const float* g_z, const float* g_post_mean, const float* g_post_logvar,
                                 const float* g_lstm_h, const float* g_lstm_c, float* flat_grads, int accumulate, float* const* g_state,
                                 const int* frame_idx, int n_frames, const float* const* g_frames);

/* A learned observation scale: d LL_e / d sigma of every ELBO evaluation e of the last call that ran with option "sigma_grad" 1 -- the
 * batch mean over the images of  sum_p ( sum_{k,c} g1_kc (x_c - mu_kc) - 3 w_p ) / sigma  with g1_kc = w_p r_kc (x_c - mu_kc) / sigma^2 the
 * closed-form d(B * ELBO) / d mean of the per-pixel terms (r: responsibilities, w_p: the pixel weight of iodine_set_pixel_weights, 1
 * without), i.e. the derivative of the LL the call reports (elbo_iter[e][2] / terms[2]), weighted exactly like it, summed like it (fp64
 * partial sums in a fixed order).  Sigma reaches the loss only through this direct term: the refinement inputs are detached
 * (iodine.py:343).  The values are RAW, like elbo_iter: not multiplied by the iteration weights, beta or a sign -- d loss / d sigma of a
 * training forward is  -sum_e w_e out[e]  with the weights it ran with, d ELBO / d sigma of an elbo is out[0].
 *   n = T + 1 after iodine_train_forward / _seq / _frames (from a state and over a clip alike), n = 1 after an iodine_elbo that ran with
 *   option "save_for_backward"; out: n floats of device memory, written on `stream`.  Another n: IODINE_ERR_INVALID.
 * IODINE_ERR_STATE when the last compute call did not produce the values: the option was off, the call was of another kind
 * (reconstruct, decode, a plain elbo), or the workspace was re-planned since.  The values survive the backward of that forward. */
int iodine_last_sigma_grad(iodine_handle* h, void* stream, float* out, int n);

/* Gradients into the image and the pixel weights (kernels_pixmap.hip): what the last compute call that ran with option "input_grad"
 * accumulated.  With log_likelihood = logsumexp_k(log(mask + 1e-12) + K_log_likelihood) and LL = log_likelihood.mean(0).sum()
 * (iodine.py:210-220), weighted per pixel by w_p (iodine_set_pixel_weights, 1 without):
 *   d LL / d x[b,c,p] = -(1 / B) sum_k g1_kc,  g1_kc = w_p r_kc (x_c - mu_kc) / sigma^2  (r: responsibilities; the weight is inside)
 *   d LL / d w[b,p]   =  (1 / B) sum_c log_likelihood[b,c,p]                             (raw: NOT multiplied by w)
 * Option "joint_likelihood": log_likelihood = logsumexp_k(log(mask + 1e-12) + sum_c K_log_likelihood), one plane per image, and
 *   d LL / d x[b,c,p] = -(1 / B) sum_k g1_kc,  g1_kc = w_p r_k (x_c - mu_kc) / sigma^2   (ONE responsibility r_k per slot and pixel,
 *                                                                                         r_k = softmax_k(log(mask_k + 1e-12) + sum_c l_kc))
 *   d LL / d w[b,p]   =  (1 / B) log_likelihood[b,0,p]
 * The refinement inputs are detached (iodine.py:343) and the KL term does not see the image: these direct terms are all of d ELBO / d x.
 * The reference treats weights it does not have as data; here they are differentiable on request.
 *   after iodine_train_forward / _seq / _frames:  sum_e a_e d LL_e / d (x, w)  with a_e the iteration weights the call ran with
 *   (iodine_set_objective; beta does not enter; a_e = 0 adds an exact 0), added in evaluation order in fp32 -- d loss / d x is MINUS g_x.
 *   A clip: frame e belongs to evaluation e alone, g_x (B, T + 1, 3, S, S) holds a_e d LL_e / d x_e, in the batch-first layout the entry
 *   point took the clip in; g_w likewise (B, T + 1, S, S) when the call's weights were per frame, else (B, S, S) summed over the frames.
 *   after an iodine_elbo that ran with option "save_for_backward":  d LL / d (x, w), g_x (B, 3, S, S), g_w (B, S, S).
 * Either pointer may be NULL; device memory, written on `stream`.  IODINE_ERR_STATE when the last compute call left nothing: the option
 * was off (or lacked the bit an output needs: 1 image, 2 weights), the call was of another kind (reconstruct, decode, a plain elbo), or the
 * workspace was re-planned since.  The values survive the backward of that forward. */
int iodine_last_input_grad(iodine_handle* h, void* stream, float* g_x, float* g_w);

/* The per-pixel likelihood maps the reference leaves on the module after every elbo() (iodine.py:210-216), of the evaluation
 * iodine_last_elbo_outputs reads -- computed on request from its decoder output and its image (its frame of a clip):
 *   k_log_likelihood (count, K, 3, S, S) = gaussian_log_likelihood(x[:, None], mean, sigma),
 *   log_likelihood   (count, 3, S, S)    = logsumexp_k(log(mask + 1e-12) + k_log_likelihood);     either may be NULL.
 * With option "joint_likelihood" log_likelihood is (count,1,S,S) = logsumexp_k(log(mask + 1e-12) + k_log_likelihood.sum(2)), one plane
 * per image (a third of the floats: size the buffer by the option); k_log_likelihood is unchanged.
 * K = the slots of that call; sigma = the handle's current objective.  RAW: pixel weights do not enter (the weighted LL the call reported is
 * sum_p w_p sum_c log_likelihood).  The kernel is apart from the one that sums the reported LL: sum_c of the map agrees with
 * elbo_iter[..][2] to fp32 rounding, not bitwise.  Plain outputs: nothing is attached to a graph (the reference's attributes are).
 * Same count rule and refusals as iodine_last_elbo_outputs (IODINE_ERR_STATE when no elbo() has run on the current workspace). */
int iodine_last_likelihood(iodine_handle* h, void* stream, int count, float* log_likelihood, float* k_log_likelihood);

/* logger.update(init_mean=posterior.init_mean.mean(), init_logvar=posterior.init_logvar.mean()) -- iodine.py:156-157:
 * out2 (2, device) = the two means of the parameters last handed to iodine_set_params. */
int iodine_logger_scalars(iodine_handle* h, void* stream, float* out2);

/* torch.randn_like of Gaussian.sample (iodine.py:632) without ATen: n standard normals from Philox4x32-10 + Box-Muller,
 * counter-based (element e depends only on (seed, stream_id, e)); the wrapper passes one stream_id per call. */
int iodine_randn(void* stream, float* out, long long n, unsigned long long seed, unsigned long long stream_id);

/* optimizer.step() -- lib/engine/train.py:65 with the Adam built by lib/solver/build.py:5-16.  One fused launch over all
 * tensors.  ptrs_dev[4*t + {0,1,2,3}] = device addresses of {param, grad, exp_avg, exp_avg_sq} of tensor t (as int64),
 * offsets_dev[t] = first flat element index of tensor t, total = sum of the element counts; step counts from 1.
 * Semantics of torch.optim.Adam (amsgrad=False, maximize=False, coupled weight decay). */
int iodine_adam_step(void* stream, const long long* ptrs_dev, const long long* offsets_dev, int n_tensors, long long total,
                     double lr, double beta1, double beta2, double eps, double weight_decay, int step);

/* Global-norm gradient clipping -- the line the reference carries commented out at lib/engine/train.py:64,
 * `clip_grad_norm_(model.parameters(), 5.0)`, with the semantics of torch.nn.utils.clip_grad_norm_ at norm_type = 2.
 * All four entries take the tables of the Adam step above (the norm and the scale read only ptrs_dev[4*t + 1], the
 * gradient), enqueue on `stream` and return: no call synchronises, no value comes back to the host.
 *
 * Bytes of scratch the norm over `total` elements needs (lib/engine/train.py:64; the caller allocates and owns it: device
 * memory, 8-byte aligned; a function of `total` alone). */
size_t iodine_grad_norm_scratch_bytes(long long total);

/* total_norm and clip coefficient of lib/engine/train.py:64: out4_dev[0] = total_norm = 2-norm of all gradients taken together,
 * out4_dev[1] = clip_coef = min(1, max_norm / (total_norm + 1e-6)) as torch computes it, out4_dev[2] = 1 if total_norm is
 * inf / NaN else 0, out4_dev[3] += out4_dev[2] (a running count: the caller zeroes it once).  Sums run in fp64 in a fixed
 * order without atomics: the same gradients give the same bits on every call.  The caller owns scratch_dev (at least the
 * bytes the entry above reports) and out4_dev (4 floats); the library keeps neither.
 * max_norm <= 0 or NaN is IODINE_ERR_INVALID; +inf is allowed and gives clip_coef = 1.  Does not synchronise. */
int iodine_grad_norm(void* stream, const long long* ptrs_dev, const long long* offsets_dev, int n_tensors, long long total,
                     double max_norm, void* scratch_dev, size_t scratch_bytes, float* out4_dev);

/* The in-place half of lib/engine/train.py:64, `g.mul_(clip_coef)` of torch.nn.utils.clip_grad_norm_: every gradient of the
 * table is multiplied by *coef_dev (one float in device memory the caller owns, e.g. out4_dev + 1).  Does not synchronise. */
int iodine_grad_scale(void* stream, const long long* ptrs_dev, const long long* offsets_dev, int n_tensors, long long total,
                      const float* coef_dev);

/* lib/engine/train.py:64-65 in one launch: the Adam step above on gradients multiplied by out4_dev[1] (the clip comes
 * before the weight-decay term, as torch clips .grad and Adam then adds weight_decay * param; the gradients themselves are NOT
 * rewritten).  skip_nonfinite != 0: when out4_dev[2] != 0 (non-finite norm) parameters and both moments are left untouched;
 * 0 is torch's behaviour (NaN / inf flow into the parameters).  out4_dev is the caller's, as the norm entry wrote it
 * earlier on the same stream.  Does not synchronise. */
int iodine_adam_step_clipped(void* stream, const long long* ptrs_dev, const long long* offsets_dev, int n_tensors, long long total,
                             double lr, double beta1, double beta2, double eps, double weight_decay, int step,
                             const float* out4_dev, int skip_nonfinite);

/* ARI evaluation epilogue -- lib/eval/ari_eval.py:25-39 + lib/utils/ari.py:36-52: per-pixel argmax over the K slot masks and
 * the integer contingency table[b][i][k] = |gt_i AND (argmax == k)|.  mask (B,K,1,S,S) fp32 (device, as returned by
 * iodine_reconstruct), gt (B,G,S,S) uint8 0/1 (device, padded with empty masks), table (B,G,K) int32 (device, overwritten).
 * The ARI formula itself (lib/utils/ari.py:6-33, a handful of scalars per image) stays on the host. */
int iodine_ari_table(void* stream, const float* mask, const unsigned char* gt, int batch, int slots, int n_gt, int pixels,
                     int* table);

/* Per-slot object table and segmentation map of one decode: what a user of the masks computes first (count, crop, follow the slots).
 * Stateless like the ARI entry above: no handle, no workspace, one launch, no synchronise.
 *   mask (B,K,1,S,S) fp32 (device, as iodine_reconstruct / iodine_decode / a trajectory entry returns it), mean_or_null (B,K,3,S,S) fp32,
 *   table (B,K,14) fp32 (device, overwritten), seg_or_null (B,S,S) uint8 (device, overwritten): seg[b][p] = argmax_k mask[b][k][p].
 * The argmax compares `v > best` from slot 0 upwards: on a tie the LOWEST index wins, as in iodine_ari_table, and a NaN never wins.
 * Pixel p has col = p % S, row = p / S; "hard" pixels of slot k are those whose seg equals k.  Columns of table[b][k]:
 *    0      soft_area          sum_p m
 *    1      hard_area          number of hard pixels
 *    2, 3   soft_cx, soft_cy   sum m col / soft_area, sum m row / soft_area            (0 where soft_area == 0)
 *    4, 5   hard_cx, hard_cy   mean col, mean row of the hard pixels                    (-1 where there are none)
 *    6..9   x0, y0, x1, y1     inclusive bounding box of the hard pixels                (all -1 where there are none)
 *   10..12  r, g, b            sum m mean_c / soft_area                                 (0 where soft_area == 0 or mean_or_null is NULL)
 *   13      peak               max_p m
 * An empty slot therefore reads hard_area 0 and -1 in columns 4..9; a slot whose mask is identically 0 also has 0 in columns 0, 2, 3 and
 * 10..12.  Counts, coordinate sums and the box are integer arithmetic, converted once ((float)((double)sum / (double)count)); the soft sums
 * run in fp64 over fixed-order fp32 groups of four and use no atomics, so the same input gives the same bits on every call.
 * IODINE_ERR_INVALID, before anything touches the device: mask or table NULL, batch < 1, slots outside 1..16, size outside 1..1024. */
int iodine_slot_table(void* stream, const float* mask, const float* mean_or_null, int batch, int slots, int size,
                      float* table, unsigned char* seg_or_null);

/* Contingency table of two segmentations (two runs of a multi-stable model, two frames of a clip): seg_a, seg_b (B,P) uint8 (device, e.g.
 * the seg of iodine_slot_table), table (B,Ka,Kb) int32 (device, overwritten), table[b][i][j] = #{p : seg_a[b][p] == i and seg_b[b][p] == j}.
 * It is the table the ARI formula takes; IoU of slot i with slot j is table[i][j] / (rowsum_i + colsum_j - table[i][j]).  A pixel whose
 * label is >= slots_a in seg_a or >= slots_b in seg_b is left out of every count (the labels are the caller's and are never used as an
 * index unchecked).  Integer atomics only: exact and reproducible.  IODINE_ERR_INVALID, before anything touches the device: a NULL
 * pointer, batch < 1, slots_a or slots_b outside 1..16, pixels outside 1..1024 * 1024.  Does not synchronise. */
int iodine_seg_overlap(void* stream, const unsigned char* seg_a, const unsigned char* seg_b, int batch, int slots_a, int slots_b,
                       int pixels, int* table);

/* Connected components of segmentation maps: the OBJECTS of a map, where the entries above read one slot as one object (a slot that
 * grabbed two objects, a background cut into pieces and the speckle of an argmax map along object borders are all "one slot").  Integers
 * only: every output is exact and the same input gives the same bits on every call and every stream.
 *   seg (B,S,S) uint8 (the seg of iodine_slot_table), pixel p = row * S + col.  A pixel is VALID if seg[p] < slots; an invalid pixel
 *   belongs to no component and separates its neighbours.  Two valid pixels are joined if they hold the same value and are 4-neighbours
 *   (connectivity 4) or 8-neighbours (connectivity 8); the components are the classes of that relation.  first(c) is the smallest p of
 *   component c, area(c) its pixel count, slot(c) its value.  c is KEPT if area(c) >= min_area and SMALL otherwise; the kept components
 *   of an image are numbered 0, 1, .. in increasing first(c) - the raster order in which scipy.ndimage.label numbers.
 * Outputs, all overwritten (device memory for iodine_seg_components, host memory for iodine_seg_components_host):
 *   labels (B,S,S) int32            id of the pixel's kept component; -1 in small components and at invalid pixels
 *   area_map_or_null (B,S,S) int32  area of the pixel's component, small ones included; 0 at invalid pixels
 *   count (B,4) int32               kept components, small components, pixels in small components, invalid pixels
 *   per_slot_or_null (B,slots,4) int32   per slot: kept components, small components, area of its largest component (0 if none), its
 *                                   pixels in small components
 *   table_or_null (B,M,8) int32, M = max_components: row i < M describes kept component i: slot, area, sum_col, sum_row, x0, y0, x1, y1
 *                                   (inclusive box; centroid = sum / area on the caller's side; the sums fit int32 up to S = 1024).  Rows
 *                                   from the number of kept components upwards are all -1; ids >= M appear in labels and count only.
 *   clean_or_null (B,S,S) uint8     kept and invalid pixels keep seg.  A small component c takes slot(d) of one kept component d: the
 *                                   candidates are the kept components that contain a 4-neighbour of a pixel of c (the 4-neighbourhood
 *                                   whatever connectivity is); d has the largest area, and the smaller first(d) on a tie.  A small
 *                                   component without a kept 4-neighbour is left as it is.  ONE pass over the components of seg, not
 *                                   iterated: clean may still hold components below min_area (specks enclosed by specks, or specks that
 *                                   took different slots), and two kept regions of one slot may have grown together.
 * iodine_seg_components: no handle, no allocation, no synchronise, everything on `stream`.  Union-find with atomic-minimum merges (every
 *   retry strictly lowers a root; no loop waits for "nothing changed", so every launch ends for any input).  Images up to
 *   IODINE_COMPONENTS_LDS_MAX_SIZE run one block per image with the parent array in LDS; larger ones merge 64 x 64 tiles in LDS and then
 *   across the tile borders in `labels`.  scratch: device memory of iodine_seg_components_scratch_bytes(batch, size) bytes (host-only query,
 *   0 for batch < 1 or size outside 1..1024), any alignment, contents irrelevant before and after.
 * iodine_seg_components_host: one image on host pointers, a plain serial flood fill of the same rule (csrc/components_host.h).
 * IODINE_ERR_INVALID, before anything touches the device, with the entry's name in iodine_last_error(NULL): seg, labels or count NULL,
 *   batch outside 1..65535, slots outside 1..16, size outside 1..1024, connectivity other than 4 / 8, min_area < 1, max_components < 1 with
 *   a table or < 0 without, scratch NULL or scratch_bytes below the query. */
#define IODINE_COMPONENTS_LDS_MAX_SIZE 128
size_t iodine_seg_components_scratch_bytes(int batch, int size);
int iodine_seg_components(void* stream, const unsigned char* seg, int batch, int slots, int size, int connectivity, int min_area,
                          int max_components, int* labels, int* area_map_or_null, int* count, int* per_slot_or_null,
                          int* table_or_null, unsigned char* clean_or_null, void* scratch, size_t scratch_bytes);
int iodine_seg_components_host(const unsigned char* seg, int slots, int size, int connectivity, int min_area, int max_components,
                               int* labels, int* area_map_or_null, int* count, int* per_slot_or_null, int* table_or_null,
                               unsigned char* clean_or_null);

/* Refinement restarts (IODINE.restarts): inference is stochastic and multi-stable, so the same images are refined C times - C chains - and
 * the chains are scored, labelled and folded into one labelling.  Two stateless entries in the contract of the two above: no handle, no
 * workspace, no allocation, no synchronise, everything on `stream`, no float atomics.  P = size * size; row c B + b of a (C,B,..) tensor is
 * chain c of image b, as iodine_reconstruct returns the decodes of x repeated chain-major.
 *
 * iodine_chain_score: x (B,3,S,S) fp32, w_or_null (B,S,S) fp32 observation weights (NULL = 1), mask (C,B,K,1,S,S), mean (C,B,K,3,S,S) fp32
 *   (device) -> ll_or_null (C,B) fp32, seg_or_null (C,B,S,S) uint8 (device, overwritten; either may be NULL, not both).
 *     ll[c][b] = sum_p w_p LL_p,  l_kc = -(x_c - mu_kc)^2 / (2 sigma^2) - ln sigma - ln(2 pi) / 2          (iodine.py:213-216, 661-666)
 *     joint = 0:  LL_p = sum_c logsumexp_k(log(m_k + 1e-12) + l_kc)       joint = 1:  LL_p = logsumexp_k(log(m_k + 1e-12) + sum_c l_kc)
 *   the likelihood of the state a reconstruct RETURNS, which its elbo terms (lambda_0 .. lambda_{T-1}) never score.  fp32 per pixel; each
 *   logsumexp runs over the slots in index order with the maximum so far subtracted from every exponent (the sum is rescaled when the
 *   maximum rises), w_p LL_p is formed and added in fp64 - per thread in pixel order, per wave in a fixed butterfly, across waves in index
 *   order - and rounded to fp32 once: the same input gives the same bits on every call.
 *     seg[c][b][p] = argmax_k m_k, comparing `v > best` from slot 0 upwards: the LOWEST index wins a tie and a NaN never wins - the rules,
 *   and for the same masks the bits, of iodine_slot_table's map.
 *   One thread owns a pixel of an image and loops over the chains of its block, so every mask and mean plane is read once and x / w once
 *   per block of chains; 16-byte loads where P % 4 == 0 and x, w, mask, mean are 16-byte and seg 4-byte aligned, scalar loads otherwise.
 *   IODINE_ERR_INVALID, before anything touches the device, the argument named in iodine_last_error(NULL): x, mask or mean NULL, chains
 *   outside 1..1024, batch < 1 (or chains * batch >= 2^31), slots outside 1..16, size outside 1..1024, sigma <= 0 or NaN, joint other
 *   than 0 / 1, ll_or_null and seg_or_null both NULL.
 *
 * iodine_chain_consensus: seg (C,B,P) uint8 (e.g. the seg above), perm (C,B,K) int32 - slot i of chain c is slot perm[c][b][i] of the
 *   common labelling (iodine_seg_overlap of every chain against one of them, 1 - IoU into iodine_assign) -, ref_or_null (B) int32 - each
 *   image's reference chain -, mask_or_null (C,B,K,1,S,S) fp32.  The relabelled label of chain c at pixel p is t = perm[c][b][seg[c][b][p]].
 *   Outputs, device, overwritten, each may be NULL (not all):
 *     votes (B,K,P) int32      votes[b][j][p] = #{c : t_c(p) = j}
 *     consensus (B,P) uint8    argmax_j votes, `v > best` from 0 upwards from a best of 0: the lowest index on a tie
 *     agreement (B,P) fp32     (float)votes[winner] / (float)C
 *     match (C,B) fp32         (float)((double)#{p : t_c(p) = t_ref[b](p)} / (double)P); needs ref
 *     mask_mean (B,K,1,P) fp32 mask_mean[b][j][p] = (sum_c sum_{i : perm[c][b][i] = j} mask[c][b][i][p]) / (float)C, added in fp32 from 0 in
 *                              chain order (i ascending within a chain) and divided once; needs mask
 *   Index safety: a label >= K, or a perm entry outside 0..K-1, leaves that pixel of that chain out of every count (and such a slot out of
 *   mask_mean); a ref[b] outside 0..C-1 leaves match[.][b] = 0; device data is never used as an index unchecked.  WITH SUCH A PIXEL THE
 *   VOTES SUM TO LESS THAN C, and a pixel no chain votes on reads consensus 0, agreement 0.  Counts are integers and exact; perm is not
 *   required to be a permutation.  16-byte accesses where P % 4 == 0 and the pointers are aligned for them (seg, consensus 4 bytes; mask,
 *   votes, agreement, mask_mean 16), element-wise otherwise.
 *   IODINE_ERR_INVALID, before anything touches the device, the argument named in iodine_last_error(NULL): seg or perm NULL, chains
 *   outside 1..1024, batch < 1 (or chains * batch >= 2^31), slots outside 1..16, size outside 1..1024, match without ref, mask_mean
 *   without mask, every output NULL. */
int iodine_chain_score(void* stream, const float* x, const float* w_or_null, const float* mask, const float* mean, int chains, int batch,
                       int slots, int size, double sigma, int joint, float* ll_or_null, unsigned char* seg_or_null);
int iodine_chain_consensus(void* stream, const unsigned char* seg, const int* perm, const int* ref_or_null, const float* mask_or_null,
                           int chains, int batch, int slots, int size, int* votes_or_null, unsigned char* consensus_or_null,
                           float* agreement_or_null, float* match_or_null, float* mask_mean_or_null);

/* Adaptive refinement (IODINE.reconstruct_adaptive): refine every image until ITS posterior stops improving, drop it from the batch, go on
 * with the rest - the cost of a call follows the sum of the per-image iteration counts, not batch x max.  One handle entry and the two
 * stateless device steps it is made of (no handle, no workspace, no allocation, no synchronise, no atomics; everything on `stream`).
 *
 * The stopping rule (tests/adaptive_reference.py is its definition, numpy float64).  ll_i(b), kl_i(b): the fp32 per-image terms of ELBO
 * evaluation i; s_i(b) = (double)ll_i(b) - beta * (double)kl_i(b); R = check_every.  Decisions are taken after t = R, 2R, .. < max_iters
 * updates only.  After t updates image b stops when  t >= budget[b]  (with a budget), or when  t >= max(min_iters, 2)  and
 *     s_{t-1} - s_{t-2} < tol + rtol * |s_{t-2}|
 * evaluated in fp64 in exactly that order - one multiply, one add, one subtract, one compare, no fused multiply-add (the kernel uses the
 * round-to-nearest intrinsics), so the device agrees with numpy bit for bit.  A NaN on either side makes the comparison false: the image
 * continues.  At t = max_iters every remaining image stops.  tol may be any finite number or +-inf (-inf: never stop early; +inf: stop at
 * the first permitted check).  Each evaluation draws fresh noise: s is a one-sample estimate, tol has to sit above that noise, and with
 * check_every > 1 only evaluations t - 1 and t - 2 are compared. */
typedef struct iodine_adaptive_ctl {
    int max_iters;                       /* >= 1: the updates an image gets at most */
    int min_iters;                       /* 1..max_iters: no stop by the score before this many updates (and never before 2) */
    int check_every;                     /* R >= 1: updates per round */
    double tol, rtol;                    /* tol: not NaN; rtol >= 0 */
} iodine_adaptive_ctl;
/* iodine_adaptive_select: the decisions after one round.  All pointers device memory.
 *   terms (rounds, n, 2) fp32 = {ll, kl} of the round's evaluations t - rounds .. t - 1 for the n active images in their current layout (the
 *   handle's workspace lays a round at batch n out like this); idx_in (n) int32 = their original indices in 0..batch-1 (NULL: position =
 *   index, the first round); t = updates done; ctl and beta as above; budget_or_null (batch) int32.  With rounds = 1 and a decision by the
 *   score, s_{t-2} is read from row t - 2 of the traces, where the round before left it.
 *   -> idx_out / pos_out (n): original index / position in the current layout of the images that continue, in ascending order of position
 *   (a stable compaction); stop_idx / stop_pos (n): the same pair for those that stop; counts[2] = {continue, stop}; iters[orig] = t for
 *   the images that stop; ll, kl (max_iters, batch) fp32 traces: rows t - rounds .. t - 1, column orig, of every image active in the round.
 *   idx_out must not be idx_in.  An idx_in entry outside 0..batch-1 addresses nothing and is listed as stopped.
 *   One block; a wave64 ballot / popcount scan, looped over n with the running offsets carried in LDS: no atomics, the same order and the
 *   same bits on every call, any n >= 1.
 *   IODINE_ERR_INVALID before anything touches the device (iodine_last_error(NULL) names the argument): a NULL among terms, ctl, the
 *   outputs; n < 1 or n > batch; rounds outside 1..t; t > max_iters; min_iters outside 1..max_iters; check_every < 1; tol NaN; rtol < 0 or
 *   NaN; beta NaN; idx_out == idx_in.
 *
 * iodine_adaptive_move: a table of 1..16 row gathers / scatters (host memory) in ONE launch.  Entry: row r < rows of row_floats floats
 *   goes from src row src_index[r] to dst row dst_index[r] (a NULL index: r); src_rows / dst_rows are the extents in rows of the two arrays
 *   (0 = rows) - an index outside its extent moves nothing.  float4 accesses where row_floats % 4 == 0 and src and dst are 16-byte
 *   aligned, scalar otherwise, per entry.  Rows of one entry with the same destination are the caller's mistake (last writer unknown).
 *   Source and destination of one entry never alias: a parallel in-place compaction would read rows other blocks have overwritten, so an
 *   entry whose ranges [src, src + src_rows row_floats) and [dst, dst + dst_rows row_floats) overlap is refused; use a second buffer.
 *   IODINE_ERR_INVALID before anything touches the device: table NULL, n_entries outside 1..16, an entry with src or dst NULL,
 *   row_floats < 1, rows < 1, an extent below rows where there is no index, overlapping ranges. */
typedef struct iodine_move_entry {
    const float* src; float* dst;
    long long row_floats;
    const int* src_index; const int* dst_index;      /* device, int32, or NULL */
    int rows, src_rows, dst_rows;
} iodine_move_entry;
int iodine_adaptive_select(void* stream, const float* terms, const int* idx_in, int n, int rounds, int t, int batch,
                           const iodine_adaptive_ctl* ctl, double beta, const int* budget_or_null, int* idx_out, int* pos_out,
                           int* stop_idx, int* stop_pos, int* counts, int* iters, float* ll, float* kl);
int iodine_adaptive_move(void* stream, const iodine_move_entry* table, int n_entries);
/* iodine_reconstruct_adaptive: iodine_reconstruct_seq with a per-image iteration count.  The handle's run shape must be (slots, iters =
 * ctl->check_every): a round is check_every iterations (the last one what is left up to max_iters) on the first n_active rows of the
 * workspace, each exactly the loop body of iodine_reconstruct_seq; after it one iodine_adaptive_select, one 8-byte read-back of the two
 * counts (pinned memory, a synchronise on the call's stream - never of the device) and one iodine_adaptive_move: the stopped rows of
 * (post_mean, post_logvar, h, c) go straight to the caller's tensors at their original index, the continuing rows of the state, of the
 * packed image and of the next round's noise are gathered to the front of second buffers (owned by the handle, grown on demand).  While no
 * image has stopped the noise is read in place.  After the last round one sample + decode over all `batch` images, from the caller's
 * post_mean / post_logvar with eps[max_iters] - the last row for every image - gives pred / mask / mean / z.
 *   x (B,3,S,S); eps (max_iters + 1, B, K, L); budget_or_null (B) int32 device, values in 1..max_iters (the caller's contract);
 *   state_in: NULL or {post_mean, post_logvar, h, c} as iodine_reconstruct_seq takes it.
 *   -> pred, mask, mean, z (each may be NULL); post_mean, post_logvar (B,K,L), lstm_h, lstm_c (B,K,MLP_UNITS), iters (B) int32, ll, kl
 *   (max_iters, B) fp32, all required: image b holds what iodine_reconstruct_seq + iodine_last_refine_state give for it at iters[b]
 *   iterations with the noise rows {0 .. iters[b] - 1, max_iters}, bit for bit; ll / kl are pre-filled with NaN by the entry, so rows
 *   iters[b] .. of column b read NaN.  active_out_or_null: host ints, ceil(max_iters / check_every) of them: the batch each round ran at
 *   (0 for rounds that did not run).  Pixel weights (iodine_set_pixel_weights) are taken like by every call that packs x.
 * The call synchronises its stream; it is never captured in a hipGraph (option "graph": it runs eagerly) and refuses with IODINE_ERR_STATE
 * on a stream that is being captured.  Clips (iodine_set_frames > 0) are refused.  Afterwards the workspace holds no evaluation of the
 * whole batch: iodine_last_refine_state / iodine_last_elbo_outputs / iodine_last_posterior refuse until the next compute call.
 * Profile categories: "adaptive_select", "adaptive_move" (the two launches between rounds). */
int iodine_reconstruct_adaptive(iodine_handle* h, void* stream, int batch, const float* x, const float* eps, const iodine_adaptive_ctl* ctl,
                                const int* budget_or_null, const float* const* state_in, float* pred, float* mask, float* mean, float* z,
                                float* post_mean, float* post_logvar, float* lstm_h, float* lstm_c, int* iters, float* ll, float* kl,
                                int* active_out_or_null);

/* Slots matched to ground-truth masks: the K slots are exchangeable, so a loss (or a metric) against G object masks needs a minimum-cost
 * assignment of objects to slots per image.  Five stateless entries - no handle, no workspace, no synchronise - of which a training step
 * uses three: a per-pixel pass (iodine_mask_overlap), a tiny pass (iodine_mask_match), a per-pixel pass (iodine_mask_match_backward).
 *   mask (B,K,1,S,S) fp32 (device, as iodine_reconstruct / iodine_decode / a trajectory or frames entry returns it), gt (B,G,S,S) uint8
 *   (device; a byte != 0 counts as 1), P = S * S.  Per image:
 *     n_g = sum_p gt_gp (gt_area, int32, exact)    a_k = sum_p m_kp (mask_area)
 *     I_gk = sum_p gt_gp m_kp (inter)              N_gk = -sum_p gt_gp logf(m_kp + eps) (nll; left out when nll_or_null is NULL)
 *   A row with n_g = 0 is padding wherever it sits (the convention of iodine_ari_table's callers); R = the rows with n_g > 0.
 *   Pair values, kind 0 = 'iou': 1 - I_gk / U_gk with U_gk = n_g + a_k - I_gk; kind 1 = 'ce': N_gk / n_g.
 * Statistics: every term is an exact fp32 number (m + eps is one fp32 add, logf the accurate 1-ulp one) added in fp64 in a fixed order -
 * per thread in pixel order, per wave in a fixed butterfly, across waves in index order - and rounded to fp32 once: inter and mask_area are
 * within 2^-23 relative of the exact sums, and the same input gives the same bits on every call (no float atomics, no scratch buffer).
 * Assignment: M = min(|R|, K); an injective map pi from exactly M rows of R to slots that minimises the sum of the pair values of
 * match_kind; unmatched and padding rows read -1.  Among equal-cost optima the choice is unspecified but a fixed function of the input
 * (shortest augmenting paths, potentials in fp64, the lowest column on a tie; csrc/assign.h).  Every loop of the solver is bounded by G and
 * K alone; an image with a NaN or +-inf cost in a real row is refused before the search: its assign is all -1 and its total / loss NaN.
 * Loss: loss[b] = (1 / M) sum over matched rows of the pair value of loss_kind (chosen independently of match_kind), 0 when M = 0; formed
 * in fp64 from the fp32 statistics, rounded once.  Gradient, the assignment held constant, for k = pi(g):
 *   'ce':  d loss_b / d m_kp = -gt_gp / (M n_g (m_kp + eps))         'iou': -(gt_gp U - I (1 - gt_gp)) / (M U^2)
 * and exactly 0 for a slot that is no row's match.  coef (B,G,2) fp32 carries the per-row factors {on, off} between the two passes:
 * 'ce' {-1 / (M n_g), 0}, 'iou' {-1 / (M U), I / (M U^2)}, zeros for an unmatched row.
 *
 * iodine_mask_overlap: one launch, each mask plane read once; outputs inter (B,G,K), nll_or_null (B,G,K), mask_area (B,K) fp32 and
 *   gt_area (B,G) int32, all overwritten.  16-byte loads where P % 4 == 0 and mask / gt are 16- / 4-byte aligned, scalar loads otherwise.
 * iodine_assign: any cost (B,G,K) fp32 on the device (hard IoU for the matched metrics, 1 - IoU of two segmentations to follow slots);
 *   row_valid_or_null (B,G) uint8, NULL = every row is real; assign (B,G) int32, total (B) fp32 = sum of the matched costs (fp64, row order,
 *   rounded once; 0 when no row is real).
 * iodine_assign_host: one matrix on host pointers through the same function as the device kernel runs: the same bits.
 * iodine_mask_match: statistics -> assign (B,G) int32, loss (B) fp32, coef (B,G,2) fp32, and optionally the pair values of match_kind
 *   (cost_or_null) and I / U (iou_or_null), both (B,G,K) fp32 with 0 in padding rows.
 * iodine_mask_match_backward: grad_loss (B) fp32 on the device = d L / d loss_b; grad_mask (B,K,1,S,S) fp32 is written completely, zeros
 *   included.  assign is only compared against slot indices, never used as an index.
 * IODINE_ERR_INVALID, before anything touches the device, with the entry's name in iodine_last_error(NULL): a NULL required pointer,
 * batch < 1, slots / n_gt / n_rows / n_cols outside 1..16, size outside 1..1024, eps <= 0 (or NaN), a kind other than 0 / 1, kind 1
 * without nll. */
int iodine_mask_overlap(void* stream, const float* mask, const unsigned char* gt, int batch, int slots, int n_gt, int size, float eps,
                        float* inter, float* nll_or_null, float* mask_area, int* gt_area);
int iodine_assign(void* stream, const float* cost, const unsigned char* row_valid_or_null, int batch, int n_rows, int n_cols,
                  int* assign, float* total);
int iodine_assign_host(const float* cost, const unsigned char* row_valid_or_null, int n_rows, int n_cols, int* assign, float* total);
int iodine_mask_match(void* stream, const float* inter, const float* nll_or_null, const float* mask_area, const int* gt_area, int batch,
                      int slots, int n_gt, int match_kind, int loss_kind, int* assign, float* loss, float* coef, float* cost_or_null,
                      float* iou_or_null);
int iodine_mask_match_backward(void* stream, const float* mask, const unsigned char* gt, const int* assign, const float* coef,
                               const float* grad_loss, int batch, int slots, int n_gt, int size, int loss_kind, float eps,
                               float* grad_mask);

/* Device-resident datasets (iodine_amd/resident.py): the whole data set sits in device memory and a batch is assembled there.  Two stateless
 * entries - no handle, no workspace, one launch, no synchronise.
 *
 * iodine_batch_gather: item j of the batch is store entry index[j]; index (count) int64 in device memory.  A frame of a clip is an entry:
 *   the caller resolves (clip n, frame f) to n F + f, so count = B F for a batch of clips.
 *   images, image_kind 0: uint8 (N,S,S,3), HWC as decoded;  x[j][c][p] = (float)u / 255.f with an IEEE division - the bits of ToTensor's
 *                         .float().div_(255.0);
 *           image_kind 1: float32 (N,3,S,S); copied.
 *   masks_or_null uint16 (N,S,S): bit g of a word is set where the pixel lies inside ground-truth mask g (overlapping masks are exact).
 *   x (count,3,S,S) fp32 and gt_or_null (count,planes,S,S) uint8 0/1 are written completely: gt[j][g][p] = bit g of the word, which is 0 for
 *   g at or beyond the image's number of masks - the layout iodine_mask_overlap and iodine_ari_table take.  gt is left alone when either
 *   of masks_or_null / gt_or_null is NULL.
 *   Where S * S % 4 == 0 and the pointers are aligned for it (x 16, images 4 / 16, masks 8, gt 4 bytes) a thread takes four consecutive
 *   pixels, with 16-byte stores per channel plane and 4-byte stores per mask plane; element-wise otherwise.  Traffic per pixel: 3 (kind 1:
 *   12) + 2 bytes read, 12 + planes written.  Offsets are 64-bit throughout.
 *   THE INDICES ARE NOT CHECKED ON THE DEVICE: the caller validates them against [0, N) on the host before the launch.
 *
 * iodine_synth_scenes: the deterministic test scenes of iodine_amd/synth.py (make_images) generated in device memory, bit for bit: splitmix64
 *   hashing in 64-bit integers, object parameters and the inside test in fp64 without contraction, painter's order (the last object wins a
 *   pixel), colours rounded to fp32 once.  Item i draws from uniform01(seed + i seed_step, stream + i stream_step).  kind 0 = 'uniform'
 *   (every element a uniform; masks_or_null / n_gt_or_null are not touched), 1 = 'blobs' (grey background, 3..max_objects discs / squares).
 *   frames = 0: images (n,3,S,S), masks_or_null (n,S,S) uint16 - bit o where object o owns the pixel -, n_gt_or_null (n) uint8 = the
 *   number of objects.  frames = F >= 1: images (n,F,3,S,S), masks (n,F,S,S); frame f is the scene rolled by (f, 2 f) pixels (rows, columns).
 * IODINE_ERR_INVALID, before anything touches the device, with the entry's name in iodine_last_error(NULL): a NULL required pointer,
 * count / n < 1, size outside 1..4096 (synth: 1..1024), planes / max_objects outside 1..16, a kind other than 0 / 1, frames < 0. */
int iodine_batch_gather(void* stream, const long long* index, int count, const void* images, int image_kind,
                        const unsigned short* masks_or_null, int size, int planes, float* x, unsigned char* gt_or_null);
int iodine_synth_scenes(void* stream, int n, int size, unsigned long long seed, unsigned long long seed_step, unsigned long long stream_id,
                        unsigned long long stream_step, int kind, int max_objects, int frames, float* images,
                        unsigned short* masks_or_null, unsigned char* n_gt_or_null);

/* Windowed batches (iodine_amd/windows.py): the store keeps its frames at their native H x W and every item of a batch is a window of its
 * frame resampled to size x size on the device - crop, antialiased resize, mirror and colour gain in one launch.  Stateless like the two
 * entries above: no handle, no workspace, one launch, no synchronise, no atomics, deterministic.
 *
 * iodine_batch_window: item j is a window of store entry index[j] (a frame of a clip is an entry, as for iodine_batch_gather).
 *   images, image_kind 0: uint8 (N,H,W,3), v = (float)u / 255.f (IEEE division);  image_kind 1: float32 (N,3,H,W), v as stored.
 *   masks_or_null uint16 (N,H,W), bit g = inside mask g.  H = src_h, W = src_w, S = size.
 *   windows (count,8) fp32 in device memory: y0, x0, h, w, flip, gain_r, gain_g, gain_b - y0, x0, h, w in source pixels, fractional values
 *   allowed, h, w > 0, the window inside the frame, h / S <= 4 and w / S <= 4, flip 0 or 1, gains >= 0.
 *   THE RULE (tests/window_reference.py states it in fp64): crop, then resize with a triangle filter, separably - PIL's BILINEAR with
 *   antialiasing on the cut-out window.  Per axis (rows; columns alike with x0, w, W):
 *     scale = h / S, support = max(scale, 1), centre = y0 + (i + 0.5) scale;
 *     taps = the whole rows r of [lo, hi), lo = max(floor(y0), 0, int(centre - support + 0.5)), hi = min(ceil(y0 + h), H,
 *     int(centre + support + 0.5)), int truncating: the taps are clamped to the window rounded outward to whole pixels, so a window is
 *     resampled as if it had been cut out first; at most 9 of them;
 *     weight of r = max(0, 1 - |r + 0.5 - centre| / support), normalised by the sum over the taps.
 *   x[j][c][i][k] = clamp(gain_c * sum_r sum_q wy_r wx_q v[r][q][c], 0, 1), columns first, then rows.
 *   gt[j][g][i][k] = bit g of the word of source pixel (floor(centre_y(i)), floor(centre_x(k))), clamped to the frame (PIL's NEAREST).
 *   flip = 1: output column k holds what column S - 1 - k would have held, image and masks.
 *   Coordinates, tap ranges and weights are computed in fp64 without contraction (a fused multiply-add changes which tap a border falls
 *   on), the weights rounded to fp32 once; both passes accumulate in fp32.  Hence at scale 1 with whole y0, x0 the taps weigh {1, 0}: a
 *   plain crop, a whole-pixel shift and a mirror with gains 1 give, bit for bit, the slice (or mirrored slice) of what iodine_batch_gather
 *   writes for the same frame, and the identity window the gather itself.
 *   x (count,3,S,S) fp32 and gt_or_null (count,planes,S,S) uint8 0/1 are written completely; gt is left alone when either of masks_or_null /
 *   gt_or_null is NULL.  One block per (item, tile of output rows): column and row tap tables and the horizontal pass of the tile's source
 *   rows are staged in LDS.  uint8 frames with W % 4 == 0 and a 4-byte aligned store are read as whole dwords, byte-wise otherwise.
 *   Traffic per item: the window's pixels once (3 bytes, or 12, + 2 for the word of S * S of them) plus the rows two row tiles share, read;
 *   (12 + planes) S * S written.  Offsets are 64-bit throughout.
 *   THE INDICES AND WINDOWS ARE NOT CHECKED ON THE DEVICE: the caller validates them on the host before the launch (windows.py does).
 *   The kernel clamps every tap into the frame, so a bad window gives wrong pixels, never a read outside the store.
 * IODINE_ERR_INVALID, before anything touches the device, with the entry's name in iodine_last_error(NULL): a NULL required pointer,
 * count < 1, src_h / src_w outside 1..4096, size outside 1..512, planes outside 1..16, a kind other than 0 / 1. */
int iodine_batch_window(void* stream, const long long* index, int count, const void* images, int image_kind,
                        const unsigned short* masks_or_null, int src_h, int src_w, const float* windows /* (count, 8) device */,
                        int size, int planes, float* x, unsigned char* gt_or_null);

/* Decomposition figures (iodine_amd/figures.py): image, reconstruction, segmentation and one panel per slot, for a few scenes or for the
 * refinement iterations of one scene, assembled on the device into one uint8 picture.  Stateless: no handle, no workspace, one launch, no
 * atomics, no scratch, no synchronise.
 *
 * A sheet has `rows` rows (one scene each: a batch, the T + 1 entries of a trajectory, the frames of a clip) of `n_panels` panels.  A panel
 * is size * scale pixels square (nearest-neighbour replication by the integer `scale`); `pad` pixels of pad_value surround and separate the
 * panels:  H = pad + rows (size scale + pad),  W = pad + n_panels (size scale + pad).  The sheet is uint8 (H, W, 3), HWC, contiguous.
 * Panel c is (panel_kind[c], panel_slot[c]); the slot is read by the three slot kinds only.  R = rows, K = slots, G = n_gt, S = size:
 *   IODINE_SHEET_IMAGE        x                                                          x (R,3,S,S)
 *   IODINE_SHEET_PRED         pred                                                       pred (R,3,S,S)
 *   IODINE_SHEET_SEG          palette[slot_color[r][argmax_k mask]]                      mask (R,K,1,S,S)
 *   IODINE_SHEET_OVERLAY      (1 - alpha) x + alpha (palette colour of the label); with draw_edges a pixel whose label differs from that of
 *                             its right or lower neighbour inside the image takes `edge` instead      x, mask
 *   IODINE_SHEET_GT           palette[gt_color[r][g]], g the lowest ground-truth row with a non-zero byte at the pixel; palette[16]
 *                             ("none") where no row has one                              gt (R,G,S,S) uint8
 *   IODINE_SHEET_ERROR        grey gain ((|x0 - p0| + |x1 - p1|) + |x2 - p2|) / 3        x, pred
 *   IODINE_SHEET_SLOT_MASKED  m_k mean_k + (1 - m_k) background                          mask, mean (R,K,3,S,S)
 *   IODINE_SHEET_SLOT_MEAN    mean_k                                                     mean
 *   IODINE_SHEET_SLOT_MASK    grey m_k                                                   mask
 * palette: 17 RGB triples, 16 slot colours and "none".  slot_color (R,K) / gt_color (R,G): uint8 palette indices in device memory, NULL =
 * the identity; an index above 16 reads entry 16.
 * Arithmetic, so that float32 code without fused operations gives the same bytes: the argmax compares `v > best` from -inf, slot 0 upwards
 * (the lowest index wins a tie, a NaN never wins: the rule of iodine_slot_table); a channel value v becomes
 * (uint8)(int)(clamp(v) * 255 + 0.5) with clamp(v) = v > 0 ? (v < 1 ? v : 1) : 0, so a NaN becomes 0; every multiply, add, subtract and
 * divide of a blend, of the error panel and of the quantisation is one IEEE float32 operation rounded on its own; a palette colour enters
 * a blend as (float)c / 255.f; 1 - alpha and the error's gain * sum / 3.f are evaluated in that order.
 * One block takes a band of source rows of one panel: it reads the planes once per SOURCE pixel (16-byte loads where size % 4 == 0 and
 * every plane pointer is 16-byte aligned - gt 4 -, element loads otherwise), keeps the band's colours in LDS, and writes the band's output
 * rows with the padding left of and above the panel (right of / below it for the last panel / row): every byte of the sheet is written
 * exactly once.  The rows are stored as aligned 32-bit words, with byte stores at the two ends of a run, where W % 4 == 0 and the sheet is
 * 4-byte aligned; byte by byte otherwise.  iodine_sheet_form tells which forms a call takes: bit 0 = 16-byte loads, bit 1 = word stores
 * (-1 for arguments iodine_render_sheet refuses).  Host only.
 * iodine_sheet_size: H and W of the sheet.  Host only.
 * IODINE_ERR_INVALID, before anything touches the device, with the entry's name in iodine_last_error(NULL): a NULL spec, mask or sheet (the
 * size query: a NULL spec or result pointer), rows < 1, slots outside 1..16, n_gt outside 0..16, size outside 1..1024, scale outside 1..8, pad
 * outside 0..16, n_panels outside 1..64, an unknown kind, a slot index outside 0..slots - 1, a panel whose input is NULL (gt also: n_gt = 0),
 * H W 3 >= 2^31 (the kernel indexes the sheet in 32 bits). */
#define IODINE_SHEET_IMAGE 0
#define IODINE_SHEET_PRED 1
#define IODINE_SHEET_SEG 2
#define IODINE_SHEET_OVERLAY 3
#define IODINE_SHEET_GT 4
#define IODINE_SHEET_ERROR 5
#define IODINE_SHEET_SLOT_MASKED 6
#define IODINE_SHEET_SLOT_MEAN 7
#define IODINE_SHEET_SLOT_MASK 8
#define IODINE_SHEET_MAX_PANELS 64

typedef struct iodine_sheet_spec {
    int rows;                        /* R: scenes, one sheet row each */
    int slots;                       /* K */
    int n_gt;                        /* G, 0 = no ground truth */
    int size;                        /* S */
    int scale;                       /* 1..8 */
    int pad;                         /* 0..16 */
    int n_panels;                    /* 1..64 */
    int draw_edges;                  /* overlay: 0 / 1 */
    float background[3];             /* slot_masked: what shows where the mask is 0 */
    float alpha;                     /* overlay: weight of the label colour */
    float error_gain;
    unsigned char pad_value[3];
    unsigned char edge[3];
    unsigned char panel_kind[IODINE_SHEET_MAX_PANELS];
    unsigned char panel_slot[IODINE_SHEET_MAX_PANELS];
    unsigned char palette[51];       /* 17 x RGB */
} iodine_sheet_spec;

int iodine_sheet_size(const iodine_sheet_spec* spec, int* height, int* width);
int iodine_sheet_form(const iodine_sheet_spec* spec, const float* x, const float* pred, const float* mask, const float* mean,
                      const unsigned char* gt, const unsigned char* sheet);
int iodine_render_sheet(void* stream, const iodine_sheet_spec* spec, const float* x, const float* pred, const float* mask,
                        const float* mean, const unsigned char* gt, const unsigned char* slot_color, const unsigned char* gt_color,
                        unsigned char* sheet);

/* Options: "stop_after_iters" (debug: run only the first v refinement iterations of reconstruct, no final decode),
 * "graph" (1: replay the fixed-shape launch sequence of reconstruct / decode / elbo / train_forward / train_backward through a
 * hipGraph per distinct argument tuple -- first call eager, second captured, later ones one hipGraphLaunch; needs a non-default
 * stream; ignored while "profile" is on; 0 -- default.  Host-side scalars are baked into the captured nodes, so the tuple includes the
 * objective of iodine_set_objective -- sigma, beta, the weight table: a schedule that changes beta every step sees each key once and
 * simply runs eagerly, a repeated objective replays),
 * "save_for_backward" (1: the following iodine_decode / iodine_elbo calls keep their state for iodine_decode_backward /
 * iodine_elbo_backward - workspace mode 2, see there; 0 -- default: the inference forms, unchanged),
 * "sigma_grad" (1: iodine_train_forward* and an iodine_elbo under "save_for_backward" also compute d LL / d sigma of every ELBO
 * evaluation -- one more per-pixel kernel and a one-block reduction per evaluation, read back with iodine_last_sigma_grad; part of the
 * hipGraph key; 0 -- default: no launch differs.  The two small buffers behind it -- 8 bytes per image and 512 pixels, 4 per evaluation --
 * are part of every workspace plan, option on or off, so iodine_workspace_bytes does not depend on it),
 * "input_grad" (bit 1 = image, bit 2 = pixel weights; with a bit set iodine_train_forward* and an iodine_elbo under "save_for_backward"
 * also accumulate sum_e a_e d LL_e / d x (d w) -- one more per-pixel kernel per evaluation, read back with iodine_last_input_grad; part of
 * the hipGraph key.  The accumulators are carved behind everything else and only while a bit is set: with 0 -- default -- no launch
 * differs and iodine_workspace_bytes returns what it returned before the option existed; a change re-plans the workspace at the next
 * compute call),
 * "stable_encoding" (channel 8 of the refinement input, mask_posterior.  0 -- default, the reference: exp(s_k) / sum_j exp(s_j) with
 * s_k = sum_c log N(x_c; mu_kc, sigma) and NO max-subtraction (iodine.py:286-293), which is 0 / 0 = NaN at a pixel every slot misses by
 * about 8.5 sigma in all three channels (float32 exp returns 0 below s_k = -103.98) and then poisons that image's refinement; 1: q_k / sum_j q_j with q_k = exp(s_k - max_j s_j), the softmax over the
 * slots the channel was meant to be -- the same value wherever the reference's is finite up to rounding, finite everywhere; libm expf
 * and IEEE division either way, one definition for every kernel that writes the channel (pixel_terms.h).  The likelihood and
 * leave-one-out channels, the ELBO and every backward are unchanged.  Part of the hipGraph key; takes effect with the next call),
 * "joint_likelihood" (the form of the pixel likelihood.  0 -- default, the reference (iodine.py:210-216): a K-component mixture for each
 * colour channel, LL_p = sum_c log sum_k (m_k + 1e-12) N(x_c; mu_kc, sigma); 1: the IODINE paper's, ONE mixture per pixel over the RGB
 * vector, LL_p = log sum_k (m_k + 1e-12) prod_c N(x_c; mu_kc, sigma) = logsumexp_k(log(m_k + 1e-12) + sum_c l_kc).  Every kernel that
 * evaluates the per-pixel terms takes the form (pixel_terms.h): the ELBO and LL every call reports, the inner gradients and channels 9-13
 * of the refinement input, d LL / d sigma, d LL / d x and d LL / d w, iodine_predictive's ll, iodine_last_likelihood (whose log_likelihood
 * is then (count,1,S,S)).  Channels 8 and 14 (mask_posterior, leave-one-out: products over RGB in the reference already), K_log_likelihood,
 * the decode and the KL are the same bits in both forms; with 0 every launch and every bit is what it was before the option existed.
 * Part of the hipGraph key.  A change while a training forward or a decode / elbo under "save_for_backward" is saved DISCARDS that
 * pass -- iodine_train_backward_frames decodes earlier evaluations again and would mix the forms: the backward that follows returns
 * IODINE_ERR_STATE with a message that says so.  Other values: IODINE_ERR_INVALID),
 * "profile" (bracket kernel launches with HIP events on the launch stream: 1 = the dominant "conv_tile_*" launches only --
 * 54 of ~330 per training step, what bench.py keeps on inside its timed region; 2 = every category; 0 = off),
 * "conv_precision" (3x3 convs of the decoder and refinement stacks: 0 = exact fp32 MFMA -- IEEE fp32 products, fp32 accumulate,
 * the reference's arithmetic (nn.Conv2d fp32, iodine.py:583), and with it the per-pixel mixture terms (sigmoid, slot softmax,
 * responsibilities: iodine.py:185-216) on libm expf + IEEE division like ATen, where the default path uses v_exp_f32 / v_rcp_f32
 * on their bounded arguments (pixel_terms.h); 1 = fp32 operands split into fp16 hi+lo with one power-of-two
 * scale per 8 x 16 cell, 3 fp16 MFMAs, fp32 accumulate: products carry >= 22 bits relative to the CELL maximum (tile-relative,
 * not element-relative) -- default; 2 = 1 everywhere except in the weight-stationary decoder kernel (3 x 3 convs C -> C, C = 32 / 64,
 * power-of-two image sizes >= 16, conv_variant 6): there the forward, the data gradient and its two row-sum forms take each product
 * from ONE fp16 MFMA -- the hi half of the same weight pack (round to nearest) times the activations rounded to fp16 to NEAREST EVEN at
 * the same per-cell scale (no lo halves are loaded, computed or staged); fp32 accumulate, bias, ELU / ELU', side buffers and row sums
 * as before.  Products then carry 11 bits: fp16-class results (ELBO ~2e-4, reconstruction ~5e-3 abs. against fp64), meant for
 * evaluation; training works and is differentiated consistently, outside the 1e-3 gradient budget.  Weight gradients, the broadcast
 * layer, the output conv, the refinement stack, the per-pixel kernels and the LDS-tiled / generic decoder kernels keep the
 * arithmetic and bits of 1: where the weight-stationary kernel does not run (other image sizes, conv_variant 1) 2 computes exactly
 * what 1 computes.  Other values: IODINE_ERR_INVALID.  Only the selected path's weight packs are maintained, so a change must be
 * followed by iodine_set_params before the next compute call (1 and 2 read the same packs; a change between them asks for it too)),
 * "gen_conv_precision" (the stride-1 convs C -> C of a decoder on the GENERIC path -- DEC.KERNEL_SIZE 5 / 7 or channel counts other than
 * 32 / 64: 0 -- default = exact fp32 MFMA (v_mfma_f32_16x16x4_f32, kernels_generic.hip); 1 = forward and data gradient on the split-fp16
 * kernel of kernels_gensplit.hip -- fp16 hi + lo operands, one power-of-two scale per staged 16 x 16-tile halo and channel chunk and per
 * 16-output-channel weight slice, three v_mfma_f32_16x16x32_f16 per product, fp32 accumulation -- wherever it covers the layer: kernel
 * size 3 / 5 / 7, a channel count that is a multiple of 16, weight slice + halo within the LDS (5 x 5 up to 64 channels, 7 x 7 up to 32).
 * The weight + bias gradient of those layers runs on the split kernel of the same file (K = pixels; up to 64 channels, 7 x 7 up to 32).
 * Every other launch keeps its fp32 kernel without an error: uncovered shapes, the broadcast layer, the output conv C -> 4, stride-2
 * convs.  The packs are allocations of the handle (hipMalloc in the first iodine_set_params that runs with the option at 1, kept until
 * iodine_destroy, also after the option returns to 0: 2 x (layers - 1) x the fp32 weight bytes); they are NOT part of the workspace, so
 * iodine_workspace_bytes is the same for both settings.  Independent of conv_precision, which keeps selecting the tuned refinement kernels beside a generic decoder;
 * ignored by a decoder on the tuned path.  Other values: IODINE_ERR_INVALID.  Like conv_precision a change must be followed by
 * iodine_set_params, which builds the hi / lo weight packs only while the option is 1),
 * "conv_variant" (stride-1 conv C -> C of the decoder, either precision: 6 = weight-stationary persistent kernel, weights in
 * registers -- default for power-of-two image sizes; 1 = LDS-tiled kernel, 16x16 tiles, two blocks per CU -- the fallback for
 * other sizes; like conv_precision a change must be followed by iodine_set_params),
 * "fuse_l0" (1 -- default: the last decoder data gradient reduces its result to the broadcast layer's row sums in its epilogue
 * instead of storing it; 0 = store and reduce in a second kernel),
 * "out_bwd_fused" (1 -- default: in training the output conv's data gradient and weight / bias gradient come from ONE pass
 * over the saved activation; 0 = two kernels, as iodine_reconstruct's data gradient + the GEMM-form weight gradient),
 * "refine_split" (1 -- default on the split-fp16 path: the first refinement layer is computed as a per-slot conv over the 11
 * encoding channels that differ between the slots of an image plus a per-image conv over the 6 they share; 0 = one conv
 * over the 20-float encoding per slot; a change takes effect with the next forward),
 * "head_fused" (1 -- default: the back-propagation through time of the refinement head runs as ONE launch, a block per 8 slots
 * walking the T iterations; 0 = nine launches per iteration -- also the automatic fallback when MLP_UNITS is too large for the
 * fused kernel's LDS footprint),
 * "refine_bwd_fused" (1 -- default: training backward, data gradient of refinement layer 1 + weight / bias gradient of layer 0
 * in ONE launch, d(pre-activation 0) never stored (kernels_refbwd.hip; power-of-two image sizes >= 64, split first layer);
 * 0 = the two launches),
 * "refine_ws" (1 -- default: forward stride-2 convs of refinement layers 1.. on the weight-stationary kernel
 * (kernels_refws.hip); 0 = the LDS-tiled stride-2 kernel),
 * "refine_l0_fused" (1 -- default: the 17-channel encoding of get_input_encoding (iodine.py:243-343) and the first refinement
 * layer in ONE kernel (kernels_refl0.hip) -- in inference the encoding is never written, so iodine_debug_copy("enc") then
 * needs "stop_after_iters" >= 0 or this option 0; 0 = pixel_pass2 writes the encoding, two convs read it),
 * "head_mfma" (1 -- default: the LSTM gate pre-activations of the refinement head as one fp32-MFMA GEMM over all slots,
 * three launches; 0 = the one-launch head kernel; the option chooses only where both forms can run -- 4 * MLP_UNITS not a multiple of 32
 * runs in one launch, MLP_UNITS above about 356 in three, whatever it says),
 * "dec_out_rows" (1 -- default: the output conv's forward runs as a row-streaming kernel -- a block walks a strip of image
 * rows, every row of the [pixels x 36] product is computed once and kept in an LDS ring until the rows above and below are
 * there -- for image sizes 32 / 64 / 128 on the split path; 0 = 16 x 16 tiles, each recomputing its 18 x 18 halo),
 * "wgrad_accum" (0 -- default: the partial weight-gradient tiles of a decoder launch are reduced right behind it; 1 = every block
 * keeps its partial tile over the T + 1 decoder passes of a training step (adds alpha_i x pass i; alpha_i = the pass's loss
 * weight) and the fixed-order reduction runs once per layer and step, 3 + 1 instead of 18 + 6 reductions per cfg3 step --
 * measured equal in time, so not the default; a change re-plans the workspace),
 * "profile_stride" (n >= 1, default 1: at "profile" level 1 only every n-th launch of a category is bracketed with events --
 * a pair of event records idles the GPU for ~12 us; iodine_profile_read("seen:<category>") returns how many launches the
 * category had in all),
 * "xskip" (timing-only ablation libraries built with -DIODINE_XSKIP_HOOK; absent from the product build).
 * (The A/B-only selections of rounds 1-2 -- conv_variant 5, wgrad_ws, out_variant, out_dgrad_variant, zigzag -- were retired in
 * round 3; their kernels and measurements live under tools/experiments/ and DESIGN.md 4.3-4.5.) */
int iodine_set_option(iodine_handle* h, const char* key, double value);
/* Sum of event-measured durations (ms) and number of launches of one kernel category since the last reset:
 * "conv_tile_fwd", "conv_tile_dgrad", "conv_tile_wgrad", "dec_out", "dec_out_dgrad", "dec_out_wgrad", "dec_out_bwd", "dec_l0",
 * "l0_reduce",
 * "pixel_pass1", "pixel_pass2", "pixel_sigma_grad" (option sigma_grad), "pixel_input_grad" (option input_grad), "refine_l0" (first refinement layer), "refine_l0f" (encoding + first refinement layer in one
 * kernel, option refine_l0_fused), "refine_conv" (the others), "refine_head", "refine_wgrad", "refine_dgrad", "refine_bwd01"
 * (fused layer-1 data gradient + layer-0 weight gradient, option refine_bwd_fused), "refine_bias_grad", "head_bwd", "gen_conv"
 * (the fp32 convs of the generic path), "gen_conv_f16x3" (its split-fp16 launches, option gen_conv_precision 1), "gen_l0" (its spatial-broadcast layer: prefix-table forward, tap-sum backward), "render_bwd" (backward of the rendering - sigmoid, slot softmax, sum_k mask x mean - in iodine_decode_backward; the decoder pass behind it is booked under the categories of the training step), "frames_in" (the image / clip conversion at the head of
 * iodine_reconstruct / iodine_train_forward: one launch for all frames), "traj_out" (the per-iteration output launches of a trajectory,
 * iodine_reconstruct_seq), "scene_edit" (the per-pixel rendering launches of iodine_scene_edit), "predictive" (the per-pixel accumulate launches of iodine_predictive).  "seen:<category>" returns in *launches the number of launches of <category> since the
 * last reset, bracketed or not (option profile_stride; counted at profile levels 1 -- the bracketed categories -- and 2 -- all).  Synchronises on the recorded events.  Two more names report
 * the hipGraph bookkeeping of option "graph" in *launches: "graph_captures" (graphs instantiated) and "graph_replays". */
int iodine_profile_read(iodine_handle* h, const char* category, double* total_ms, long long* launches, int reset);
/* Copy an internal buffer of the last call (name as listed in DESIGN.md "workspace") to dst (device). */
int iodine_debug_copy(iodine_handle* h, void* stream, const char* name, int iter, float* dst, size_t max_floats,
                      size_t* n_floats);

/* ---- operator-level entry points (used by tests/ to check each kernel against the oracle) ------------- */
/* torch.linspace(-1, 1, n) in fp32, bit-exact restatement of ATen's CPU kernel (iodine.py:334-335,526-527). HOST. */
void iodine_linspace_host(int n, float* out);
/* 3x3 conv, NHWC activations, OIHW weights; mode 0: stride-1 LDS-tiled fp32 MFMA (epi 0 bias+ELU, 1 multiply by
 * ELU'(aux), 2 none; transpose_flip=1 computes the data-gradient conv), mode 1: strided gather kernel (bias+ELU),
 * mode 2: stride-1 LDS-tiled split-fp16 (3 MFMA) variant of mode 0, modes 9 / 10: the weight-stationary split-fp16 kernel,
 * mode 12: its exact-fp32 form (weights as fp32 in the same registers, v_mfma_f32_16x16x4_f32; conv_precision 0),
 * modes 5 / 6: split-fp16 stride-2 forward / data gradient of the refinement stack, modes 13 / 14: their exact-fp32 forms
 * (v_mfma_f32_32x32x2_f32, conv_precision 0), modes 15 / 16: the weight-stationary stride-2 conv c -> c of refinement layers 1 ..
 * (c = 64; split-fp16 / exact fp32), mode 17: mode 10 with ONE fp16 MFMA per product (conv_precision 2: same arguments, epilogues
 * and launch_cell_max side buffer).  Any other mode runs the gather kernel, as mode 1 does. */
enum { IODINE_CONV_TILE_F32 = 0, IODINE_CONV_GATHER = 1, IODINE_CONV_TILE_F16 = 2, IODINE_CONV_S2_FWD = 5, IODINE_CONV_S2_DGRAD = 6, IODINE_CONV_WS = 9,
       IODINE_CONV_WS_B = 10 /* the same kernel */, IODINE_CONV_WINO = 11 /* experiment libraries only */, IODINE_CONV_WS_F32 = 12,
       IODINE_CONV_S2_FWD_F32 = 13, IODINE_CONV_S2_DGRAD_F32 = 14, IODINE_CONV_S2WS = 15, IODINE_CONV_S2WS_F32 = 16, IODINE_CONV_WS_1P = 17 };
int iodine_op_conv3x3(void* stream, int mode, const float* in_nhwc, const float* w_oihw, const float* bias,
                      const float* aux, float* out_nhwc, int n, int ih, int iw, int w_o, int w_i, int cin_pad,
                      int cout, int stride, int epi, int transpose_flip);
int iodine_op_dec_out(void* stream, const float* in_nhwc, const float* w_oihw, const float* bias, float* out_nhwc4,
                      int n, int s, int c);
/* the split-fp16 forms of the output conv C -> 4 (GEMM + 9-tap sum): variant 0 = 16 x 16 tiles with halo recompute
 * (dec_out_stream_f16x3_kernel, per-cell max side buffer), 1 = row-streaming kernel without halo recompute
 * (dec_out_rows_f16x3_kernel, s in {32, 64, 128}), 2 = the tiled kernel without a side buffer, 3 = the row-streaming kernel on
 * exact fp32 MFMA (conv_precision 0). */
enum { IODINE_DEC_OUT_TILES = 0, IODINE_DEC_OUT_ROWS = 1, IODINE_DEC_OUT_TILES_NOMAX = 2, IODINE_DEC_OUT_ROWS_F32 = 3 };
int iodine_op_dec_out_f16x3(void* stream, const float* in_nhwc, const float* w_oihw, const float* bias, float* out_nhwc4,
                            int n, int s, int c, int variant);
/* weight + bias gradient of a 3x3 conv (kernel-level tests): in_nhwc [n][s][s][ci_pad] (ci_real of them meaningful),
 * d_nhwc [n][so][so][co] with so = s (stride 1) or s/2 (stride 2); gw_oihw [co][ci_real][3][3] and gb [co] are
 * ACCUMULATED into.  Split-fp16 kernels (stride 1: decoder stack, stride 2: refinement stack); stride -2 selects the
 * exact-fp32 form of the stride-2 kernel (conv_precision 0). */
enum { IODINE_WGRAD_STRIDE2_F32 = -2 };
int iodine_op_conv3x3_wgrad(void* stream, const float* in_nhwc, const float* d_nhwc, float* gw_oihw, float* gb, int n,
                            int s, int ci_pad, int ci_real, int co, int stride);

/* the same for the stride-1 conv c -> c (c = 32 / 64) on the exact-fp32 path (conv_precision 0): persistent, prefetched
 * v_mfma_f32_32x32x2_f32 kernel (kernels_wgrad32.hip); gw_oihw / gb are ACCUMULATED into.  c < 0: the output conv |c| -> 4 in
 * GEMM form (d_nhwc has 4 channels, gw_oihw [4][|c|][3][3], gb [4]). */
int iodine_op_conv3x3_wgrad_f32(void* stream, const float* in_nhwc, const float* d_nhwc, float* gw_oihw, float* gb, int n,
                                int s, int c);

/* the generic path's convolution (kernel size k in {3, 5, 7}, stride s in 1..8 as REF.STRIDE may be: s = 1 on the stride-1 MFMA kernels
 * of kernels_generic.hip, s = 2 on kernels_gens2.hip, s >= 3 and what neither covers on the scalar kernels -- the launchers the library runs), one
 * direction per call - mode 0: out_nhwc [n][so][so][co] = act(bias + conv(in_nhwc [n][si][si][ldc], w_oihw [co][ci][k][k])), elu = 1
 * applies ELU; mode 1: out_nhwc [n][si][si][ldc] = ELU'(aux [n][si][si][ldc]) * data gradient of the gradient in_nhwc [n][so][so][co], the first
 * ci channels of every pixel (the rest is neither read nor written), with w_oihw [co][ldc][k][k] in this mode; mode 2: weight +
 * bias gradient of (in_nhwc, aux = gradient [n][so][so][co]) ADDED to out_nhwc = gw [co][ci][k][k] and gb [co].  so = (si - 1) / s + 1.
 * Modes 0 / 2, tests only: elu | 0x100 | (mask << 9) hands the kernels the per-channel mask of input channels that can be non-zero (bit c =
 * channel c; ci <= 22), as the library does for the first refinement layer of an ARCH.ENCODING subset - channel groups that are zero in
 * the input AND the weights are skipped; the result must equal the unmasked call. */
enum { IODINE_GEN_FWD = 0, IODINE_GEN_DGRAD = 1, IODINE_GEN_WGRAD = 2 };    /* mode of every generic-path entry below (the broadcast layer: 0 / 1) */
int iodine_op_gen_conv(void* stream, int mode, const float* in_nhwc, const float* w_oihw, const float* bias, const float* aux,
                       float* out_nhwc, float* gb, int n, int si, int ci, int ldc, int co, int k, int s, int elu);

/* which kernel iodine_op_gen_conv (= the library, through the same launchers) runs for these arguments: host arithmetic only, no HIP call,
 * no GPU needed.  Returns tier | np << 8 | seg << 16, or -1 for arguments iodine_op_gen_conv rejects.  tier, modes 0 / 1: 0 / 1 / 2 = the stride-1 MFMA
 * kernel with 16- / 8- / 4-channel chunks, 3 = the stride-2 MFMA kernels, 4 = the scalar kernels; mode 2: 5 = the GEMM form of a
 * 4-output-channel conv (np = its NP instantiation 1 / 2 / 4 / 8, otherwise 0), 6 = the row-staged form, 7 = the per-tap MFMA form,
 * 3 = stride-2 MFMA, 4 = scalar.  seg, modes 0 / 1: 0 = every output is one fp32 fmaf chain over its products (up to 1600 of them: 5 x 5 x 64
 * channels); otherwise the chain is summed in segments of about 800 products and seg is the segment length, in staged chunks (MFMA kernel)
 * or products (scalar kernels).  The kernel-level tests assert the tier each of their cases is meant to hit. */
int iodine_op_gen_conv_tier(int mode, int si, int ci, int ldc, int co, int k, int s);

/* the generic path's spatial-broadcast layer (kernels_genl0.hip: SpatialBroadcast + the first decoder conv without the broadcast tensor),
 * kernel-level tests only -- it packs w_oihw [co][L + 2][k][k] (input channels: L latents, then the x and the y coordinate plane), builds
 * the coordinates with iodine_linspace_host, allocates, synchronises and frees per call.  mode 0: out [n][s][s][co] = ELU(bias + conv) of
 * z [n][L] broadcast over s x s (odd k <= 7, padding k / 2).  mode 1: dpre [n][s][s][co] = gradient wrt the pre-activation -> dz [n][ld]
 * (L entries per row written, ld >= L), and gw [co][L + 2][k][k] += alpha dW, gb [co] += alpha db; alpha = 0 leaves gw / gb alone. */
int iodine_op_gen_l0(void* stream, int mode, const float* z, const float* w_oihw, const float* bias, const float* dpre, float* out,
                     float* gw, float* gb, float* dz, int n, int L, int s, int co, int k, int ld, float alpha);

/* the split-fp16 form of the same (kernels_gensplit.hip, option gen_conv_precision 1), same arguments: mode 0 forward, mode 1 data
 * gradient x ELU'(aux), mode 2 weight + bias gradient ADDED to out_nhwc = gw and gb.  IODINE_ERR_INVALID -- never the fp32 kernel -- for
 * everything the split kernels do not cover: s != 1, ci != co, ldc != ci, a channel count that is not a multiple of 16, a slice that does
 * not fit the LDS (7 x 7 with 64 channels).  Kernel-level tests only: it allocates, synchronises and frees per call -- not for timing. */
int iodine_op_gen_conv_f16x3(void* stream, int mode, const float* in_nhwc, const float* w_oihw, const float* bias, const float* aux,
                             float* out_nhwc, float* gb, int n, int si, int ci, int ldc, int co, int k, int s, int elu);

/* backward of the rendering step of decode (kernels_render.hip): dec_out [batch * slots][pixels][4] as the decoder leaves it, g_pred
 * (batch,3,pixels), g_mask (batch,slots,1,pixels), g_mean (batch,slots,3,pixels) NCHW (any may be NULL = zero) -> g_out
 * [batch * slots][pixels][4] = gradient wrt dec_out; strict = 1: libm expf + IEEE division (conv_precision 0), 0: the default path's
 * v_exp_f32 / v_rcp_f32.  Synchronises. */
int iodine_op_render_bwd(void* stream, const float* dec_out, const float* g_pred, const float* g_mask, const float* g_mean, float* g_out,
                         int batch, int slots, int pixels, int strict);

/* the same with g_logits (batch,slots,1,pixels) = a gradient wrt the mask logits themselves (the fourth channel of dec_out), added behind
 * the softmax backward -- the rendering backward of iodine_train_backward_aux; g_logits NULL: iodine_op_render_bwd, bit for bit. */
int iodine_op_render_bwd_logits(void* stream, const float* dec_out, const float* g_pred, const float* g_mask, const float* g_mean,
                                const float* g_logits, float* g_out, int batch, int slots, int pixels, int strict);

/* the two per-pixel kernels of kernels_pixmap.hip (iodine.py:210-220) on a caller's decoder output, for kernel-level tests at any pixel
 * count: x_nchw (batch,3,pixels), w (batch,pixels) or NULL (= 1), dec_out [batch * slots][pixels][4]; slots 1..16.
 *   ll (batch,3,pixels), kll (batch,slots,3,pixels): the raw maps (iodine_last_likelihood);
 *   gx (batch,3,pixels) = (first ? 0 : gx) + coef * -sum_k g1_kc,  gw (batch,pixels) = (first ? 0 : gw) + coef * sum_c ll_c
 *   (iodine_last_input_grad with coef = a_e / B).  Any of the four may be NULL.  `strict` is a flag word: bit 0 strict as for
 *   iodine_op_render_bwd, bit 1 joint (option "joint_likelihood"): ll is then (batch,1,pixels), gx is built from the joint
 *   responsibilities and gw = (first ? 0 : gw) + coef * ll.  Allocates,
 * synchronises and frees per call -- not for timing.  IODINE_ERR_INVALID, without a launch, for a bad argument. */
int iodine_op_pixel_maps(void* stream, const float* x_nchw, const float* w_or_null, const float* dec_out_nhwc4, int batch, int slots,
                         int pixels, float sigma, int strict, float coef, float* ll, float* kll, float* gx, float* gw, int first);

/* the per-pixel mixture kernels of one ELBO evaluation (kernels_pixel.hip, pixel_terms.h; iodine.py:185-220, 277-340, 385-394) on a caller's
 * decoder output, for kernel-level tests at any image size: the library's launchers in the library's order --
 *   x_to_nhwc4 (w NULL = 1), { pixel_pass1, pixel_finalize_elbo } x repeat on ONE zero-initialised ticket counter (scal is set to NaN in
 *   front of every launch but the first: a finalize that elects no last block shows), pixel_sigma_grad (if out[5]), pixel_pass2 (if out[6];
 *   the split form if out[7]), final_out.
 * x_nchw (batch,3,size^2), w (batch,size^2) or NULL, dec_out [batch * slots][size^2][4], pm / plv (batch,slots,latent), lin [size] (the
 * coordinate table, iodine_linspace_host).  flags: bit 0 strict (as for iodine_op_render_bwd), bit 1 layer-norm statistics (0: lnstat = {0, 1}),
 * bit 2 stable_encoding, bit 3 joint (option "joint_likelihood": pass 1, sigma-grad and pass 2 in the joint form).  chmask: bit c = internal channel c of the encoding is written, an absent one is 0.  out[12]:
 *   g [batch * slots][size^2][4] = d(B ELBO) / d dec_out, lnstat (batch,slots,8) = {mean, 1 / (sd + 1e-5)} of g_mean, g_mask, leave-one-out,
 *   likelihood, ll_img [batch], img_terms (batch,2) = {ll, kl}, scal [3] = {elbo, kl, ll}                         -- required;
 *   sgrad [1] = d LL / d sigma; enc [batch * slots][size^2][20] (split: [..][12]); enc_sh [batch][size^2][8];
 *   pred (batch,3,size^2), mask (batch,slots,size^2), mean (batch,slots,3,size^2), logits (batch,slots,size^2)    -- each may be NULL.
 * Allocates, synchronises and frees per call -- not for timing.  IODINE_ERR_INVALID, without a launch, for a bad argument: slots outside
 * 1..16, size / batch / latent / repeat < 1, sigma <= 0, a required pointer NULL, enc_sh without enc, an index product >= 2^31. */
int iodine_op_pixel_encode(void* stream, const float* x_nchw, const float* w_or_null, const float* dec_out_nhwc4, const float* pm, const float* plv,
                           const float* lin, int batch, int slots, int size, int latent, float sigma, float beta, int flags, unsigned chmask,
                           int repeat, float* const* out);

/* ---- the refinement head, kernel-level tests only: each call allocates and frees its scratch around the launches and synchronises -- not
 * for timing.  IODINE_ERR_INVALID, without a launch, for arguments or shapes the requested form does not take (never another form). */

/* C = alpha op(A) op(B) + beta C, row-major.  form 0: the library's dispatch (launch_sgemm), op(A) [M][K] = A or A^T (ta), op(B) [K][N] = B
 * or B^T (tb).  forms 1 - 3: the fp32-MFMA kernel for A^T B with B [K][N] and M, N multiples of 32 -- 1: A [K][M]; 2: A row-major [M][K];
 * 3: A [K][M] and C written through the broadcast layer's weight map, row = latent channel, column = tap * mode_c + co ->
 * C[(co * ldc + row) * 9 + tap] with N = 9 mode_c and ldc = L + 2.  beta = 0: C is not read. */
enum { IODINE_SGEMM_DISPATCH = 0, IODINE_SGEMM_MFMA = 1, IODINE_SGEMM_MFMA_ROWMAJOR = 2, IODINE_SGEMM_MFMA_L0MAP = 3 };
int iodine_op_sgemm(void* stream, int form, int ta, int tb, int M, int N, int K, float alpha, const float* A, int lda, const float* B, int ldb,
                    float beta, float* C, int ldc, int mode_c);

/* dst[c] += alpha * sum_r src[r * ld + c].  form 0: one block per column; form 1: the streaming form for tall contiguous matrices, only
 * where the library takes it (ld == cols, rows >= 8192, cols % 4 == 0, cols <= 256, 256 % (cols / 4) == 0). */
enum { IODINE_COLSUM_BLOCK = 0, IODINE_COLSUM_TALL = 1 };
int iodine_op_colsum(void* stream, int form, const float* src, int rows, int cols, int ld, float alpha, float* dst);

/* one step of the refinement head (iodine.py:481-503, 642-643) from reference-shaped parameters.  in[14]: mlp.weight [H][C], mlp.bias [H],
 * lstm.weight_ih [4H][H + 4L], weight_hh [4H][H], bias_ih, bias_hh [4H], mean_update.weight [L][H], .bias [L], logvar_update.weight, .bias,
 * feat [N][PL][C], latent [N][4L], h_prev, c_prev [N][H].  out[10]: h, c [N][H], pm, plv [N][L] (IN / OUT: the update is added),
 * d_mean, d_logvar [N][L], pooled [N][C], s [N][H] (MLP pre-activation), gates [N][4H] (post-activation i, f, g, o), xin [N][H + 4L]; the last
 * six may be NULL.  H, L multiples of 4, C divides 256.  form 0: single launch; form 1: three launches (pre, gate GEMM, post). */
enum { IODINE_HEAD_ONE_LAUNCH = 0, IODINE_HEAD_THREE_LAUNCHES = 1 };
int iodine_op_refine_head(void* stream, int form, const float* const* in, float* const* out, int N, int PL, int C, int H, int L);

/* which form the library runs at these (padded) widths: 0 single launch, 1 three launches, -1 refused at create time.  Host arithmetic. */
int iodine_op_refine_head_form(int C, int H, int L, int prefer_split);

/* back-propagation through time of the head over T saved steps.  form 0: the fused kernel (Cr <= H; L, H, Cr multiples of 4); form 1: the
 * launch sequence.  in[16]: g_pm, g_plv [T + 1][N][L], gates [T][N][4H], c [T + 1][N][H], s [T][N][H], mean_update.weight,
 * logvar_update.weight [L][H], weight_hh [4H][H], weight_ih [4H][H + 4L], mlp.weight [H][Cr], then optional (NULL): seed_m, seed_v ([N][L] joining
 * step T - 1, or [T][N][L] with seed_stride = N L floats), gl (device scalar; NULL = 0), wtab (device, T + 1 loss weights), dh_in, dc_in [N][H].
 * out[7]: ddm, ddv [T][N][L], dgates [T][N][4H], ds [T][N][H], dpooled [T][N][Cr], optional dh_out, dc_out [N][H].  gl, the carries and
 * seed_stride need seed_m / seed_v.  B: the batch size in the loss weight -(i + 2) / (T + 1) / B. */
enum { IODINE_BPTT_FUSED = 0, IODINE_BPTT_SEQUENCE = 1 };
int iodine_op_head_bptt(void* stream, int form, const float* const* in, float* const* out, int T, int N, int B, int L, int H, int Cr,
                        long long seed_stride);

/* dpre [N][PL][C] = dpooled [N][C] / PL * ELU'(act), act = ELU output of the last refinement conv layer */
int iodine_op_pool_bwd(void* stream, const float* dpooled, const float* act, float* dpre, int N, int PL, int C);

#ifdef __cplusplus
}
#endif
#endif /* IODINE_HIP_H */
