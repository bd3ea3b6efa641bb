// What the translation units of libiodine_hip.so share: the handle, its workspace carve-up and call state, and the declarations the
// padded-handle adapter (iodine_pad.cpp) needs from the compute handle (iodine_checks.cpp, iodine_train.cpp).  What the compute handle's own
// files share - selectors, launch sequences, the planning layer - is in iodine_host.h, included at the end.  Not part of the ABI
// (include/iodine_hip.h).
#pragma once
#include "../../include/iodine_hip.h"
#include "common.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <list>
#include <string>
#include <utility>
#include <vector>

// (hidden: nothing declared here is part of the library's dynamic symbol table)
#pragma GCC visibility push(hidden)

// Message of the calling thread's last failed iodine_create / handle-free entry point (iodine_last_error(NULL)).  One slot per thread -
// these entry points hold no handle, so two threads may be refused at once - and one writer: every refusal below goes through free_fail.
extern thread_local std::string g_create_error;
inline int free_fail(int rc, std::string msg) { g_create_error = std::move(msg); return rc; }
inline int free_hip(const char* who, hipError_t e)          // the end of a handle-free launch: "who: <HIP's text>" unless it succeeded
{
    return e == hipSuccess ? IODINE_OK : free_fail(IODINE_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e));
}

struct ParamInfo {
    std::string name;
    int ndim;
    long long dims[4];
    size_t numel() const { size_t n = 1; for (int i = 0; i < ndim; ++i) n *= (size_t)dims[i]; return n; }
};

struct Buffers {               // workspace carve-up for one batch size / mode / run shape
    int B = 0, mode = -1;
    int K = 0, T = 0;                          // the run shape (slots, iterations) it was planned for: the shape of the state it holds
    int F = 0;                                 // frames x4 holds ([F][B][P][4]; iodine_set_frames, 1 = the single image)
    size_t bytes = 0;
    float *x4, *V, *dec_out, *g, *lnstat, *ll_img, *img_terms, *scal, *rows, *rows_p, *Rc, *pm, *plv;
    double* part;
    double* sg_part = nullptr;                 // option sigma_grad: per-block partials of one evaluation, [B][pixel_blocks_per_image]
    float* sgrad = nullptr;                    // ... and d LL_e / d sigma of the T + 1 evaluations of the call (iodine_last_sigma_grad)
    int ig = 0;                                // option input_grad as planned (bit 1: ig_x, bit 2: ig_w; 0: neither is carved)
    float* ig_x = nullptr;                     // sum_e a_e d LL_e / d x, (B,3,P); a clip: (B,F,3,P), one frame per evaluation
    float* ig_w = nullptr;                     // sum_e a_e d LL_e / d w, (B,P) (a clip with per-frame weights: (B,F,P))
    std::vector<float*> act;                   // decoder activations a[0..Dd-1]   (N,P,Cd)
    float *head_xh = nullptr, *head_gp = nullptr;   // refinement head in three launches: LSTM input rows, gate pre-activations
    float* dpre[2];                            // ping-pong gradient wrt pre-activations
    std::vector<float*> tmax_act;              // per-cell max |act[l]| (4 floats per 8 x 16 cell): tile scales of the weight-stationary conv
    float* tmax_dpre[2] = {nullptr, nullptr};  // the same for the two gradient buffers
    // per-iteration buffers: index i (training keeps all T(+1) copies, inference aliases them)
    std::vector<float*> z, g_pm, g_plv, latent, enc, pooled, u, gates, xin, h, c;
    std::vector<float*> enck, encs;             // split refinement input: per-slot [N][P][12], per-image [B][P][8] (alias enc's memory)
    float* rmap = nullptr;                      // split first refinement layer: conv of the per-image channels, [B][S/2][S/2][Cr]
    std::vector<std::vector<float*>> ract;     // [iter][layer] refinement activations
    // training only
    float *wg_part = nullptr, *wg_part_b = nullptr, *wg_fold = nullptr, *Dsum = nullptr, *Dpart = nullptr, *RT = nullptr, *tmp_lz = nullptr;
    // round 5 (option wgrad_accum): per-layer partial weight-gradient tiles kept over the T + 1 decoder passes of a step (one reduction
    // per layer and step); [0] = the output conv, [l] = decoder layer l
    std::vector<float*> wg_acc, wg_acc_b;
    float *rown = nullptr, *Rsum = nullptr;     // training row-sum form of the broadcast layer's backward (EPI_L0ROWSX)
    float* l0scr = nullptr;                     // partial class sums of the row-sum reductions (l0_rows_scratch_floats)
    float *ddm = nullptr, *ddv = nullptr, *dc1 = nullptr, *dgates = nullptr, *dxin = nullptr, *ds = nullptr,
          *dpooled = nullptr;
    float* carry_h[2] = {nullptr, nullptr};
    float* carry_c[2] = {nullptr, nullptr};
    std::vector<float*> rdpre;                 // gradient wrt refinement pre-activations, per layer
    float* aux_seed = nullptr;                 // [2][T + 1][N][L]: seeds of the head BPTT from auxiliary cotangents (iodine_train_backward_aux:
                                               // the first [2][N][L]; iodine_train_backward_frames: slice e = the seeds of evaluation e)
    float *gen_scr = nullptr, *gen_l0 = nullptr;                // generic path: wgrad partials; layer-0 scratch (kernels_genl0.hip)
};

// index of every parameter in the parameter table (= in gacc and in the caller's pointer array), resolved once by build_param_table
struct ParamSlots {
    std::vector<int> ref_w, ref_b;              // refine.mlc.layers.<l>
    int mlp_w, mlp_b, wih, whh, bih, bhh, wm, bm, wv, bv;   // the refinement head
    std::vector<int> dec_w, dec_b;              // decoder.mlc.layers.<l>
    int out_w, out_b;                           // decoder.conv
    int init_mean, init_logvar;
};

#pragma GCC visibility pop

// HIP-event profiler: when enabled every launch of a category is bracketed by two events on the
// launch stream; totals are read back (after a sync) with iodine_profile_read.
struct ProfCat { std::string name; std::vector<std::pair<hipEvent_t, hipEvent_t>> ev; size_t used = 0; unsigned long long seen = 0, seen_win = 0; };

struct GraphEntry { std::vector<uintptr_t> key; hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr; unsigned long long used = 0; };

// The objective a call optimises (iodine_set_objective): likelihood scale, KL weight and the per-iteration loss weights.  Held by value:
// a training forward / a saved elbo keeps the copy it ran with, its backward reads that copy and not the handle's current one.
// wtab: device table of nw = T + 1 floats, nullptr = the default weighting w_i = (i + 1) / (T + 1), which stays the closed-form
// expression in the kernels and on the host.  Tables are immutable once uploaded (WeightTable below), so a copy of the pointer is a snapshot;
// wgen names the table in the hipGraph key (0 = default).
struct Objective {
    double sigma = 0.1, beta = 1.0;
    const float* wtab = nullptr;
    const float* whost = nullptr;               // the same weights on the host (owned by the handle's table list)
    int nw = 0, wgen = 0;
};
struct WeightTable { std::vector<float> w; float* dev = nullptr; int gen = 0; };

#pragma GCC visibility push(hidden)
// What the calls so far have left in the arena.  A call SETS its fields on success, next to its run_graphed and outside the graphed body;
// they are CLEARED by the three transitions below and nowhere else.
struct CallState {
    bool fwd_done = false;                      // a training forward is saved: iodine_train_backward* may run
    int fwd_batch = 0;
    bool fwd_split = false;                     // the form the saved training forward used
    bool fwd_from_state = false;                // the saved training forward started from a caller's (lambda, h, c) (iodine_train_forward_seq)
    Objective fwd_obj, diff_obj;                // what the saved training forward / the saved elbo ran with
    // a single decode / elbo that ran "for backward" (option save_for_backward): its z, decoder activations and dec_out stay in the arena
    // (workspace mode 2) until the next compute call; iodine_decode_backward / iodine_elbo_backward consume it
    int diff_kind = 0;                          // 0 = nothing saved, 1 = a decode, 2 = an elbo
    int diff_batch = 0;
    bool diff_init = false;                     // the saved elbo sampled from the initial posterior (init_mean / init_logvar receive gradients)
    // last elbo() call (iodine.py:161-241): which z buffer / batch the decoder output in buf.dec_out belongs to
    int last_elbo_iter = -1, last_elbo_batch = 0;
    int state_iter = -1;                        // buf.h / buf.c [state_iter] = LSTM state the last iodine_reconstruct (buf.mode 0) or training
                                                // forward (buf.mode 1) left (-1: none to read)
    bool enc_valid = false;                     // the last call left the refinement input ("enc") of its iterations in the workspace
    int sgrad_n = 0;                            // values buf.sgrad holds: T + 1 after a training forward, 1 after a saved elbo - that ran with
                                                // option sigma_grad; 0: the last compute call produced none (iodine_last_sigma_grad refuses)
    int ig_bits = 0;                            // what buf.ig_x / ig_w hold of the last compute call (option input_grad; 0: nothing -
    int ig_frames = 0, ig_wpf = 0;              // iodine_last_input_grad refuses), the frames of that call (0: a still image) and whether its
                                                // weight gradient is per frame
    bool form_changed = false;                  // option joint_likelihood changed while a pass was saved: that pass is gone, and its backward says why
    bool redecoded = false;                     // a backward decoded an earlier evaluation again (iodine_train_backward_frames): buf.dec_out no
                                                // longer belongs to the last elbo(); the posterior and the LSTM state are untouched

    // iodine_set_params, a changed run shape or frames setting, a consumed backward (like autograd without retain_graph)
    void saved_passes_gone() { fwd_done = false; diff_kind = 0; }
    // a compute call re-uses the arena.  keep_lstm_state: a plain iodine_decode does not touch buf.h / buf.c
    void compute_begins(bool keep_lstm_state = false) { saved_passes_gone(); form_changed = false; redecoded = false; sgrad_n = 0; ig_bits = 0; if (!keep_lstm_state) state_iter = -1; }
    // a re-plan (ensure_workspace), iodine_set_workspace, a wgrad_accum toggle: nothing the arena held can be read any more.
    // (iodine_set_workspace used to leave enc_valid and the wgrad_accum toggle state_iter: unobservable, every reader of the two also
    // refuses while buf.bytes == 0, and the next compute call re-plans)
    void arena_gone() { saved_passes_gone(); form_changed = false; last_elbo_iter = -1; state_iter = -1; enc_valid = false; redecoded = false; sgrad_n = 0; ig_bits = 0; }
};
#pragma GCC visibility pop

// A weight pack (pack_geom.h: extent and index order) with the meta block that holds its power-of-two scale (nullptr: an fp32 pack)
struct Pack { void* data = nullptr; float* meta = nullptr; };

// What iodine_set_option sets.  conv_precision / conv_variant / gen_conv_precision invalidate the parameters (the packs follow dec_path)
struct Options {
    int precision = 1;                          // 0: exact fp32 MFMA, 1: 3 x fp16 MFMA split (fp32-class accuracy), 2: hi.hi alone on DEC_WS_F16
    int variant = 6;                            // split-fp16 stride-1 conv: 6 = weight-stationary persistent kernel (power-of-two image sizes;
                                                // other sizes use 1), 1 = LDS-tiled 16x16 tiles (2 blocks/CU)
    int gen_precision = 0;                      // gen_conv_precision 1 (kernels_gensplit.hip): the generic decoder's C -> C layers on split fp16
    int out_bwd_fused = 1;                      // training: output conv data + weight gradient in one pass over the activation
    int fuse_l0 = 1;                            // inference: layer-1 data gradient reduces straight to the layer-0 row sums
    int dec_out_rows = 1;                       // output conv forward: row-streaming kernel without halo recompute (S in {32, 64, 128}); 0 = 16 x 16 tiles
    int wgrad_accum = 0;                        // 1: the decoder's partial weight-gradient tiles accumulate over the T + 1 passes of a training step
                                                // and are reduced once per layer and step.  Measured equal to the default (round 5): kept as an option
    int refine_split = 1;                       // first refinement layer split into a per-slot and a per-image part (split-fp16 path)
    int refine_l0_fused = 1;                    // encoding + first refinement layer in one kernel (kernels_refl0.hip); 0: pixel_pass2 + two convs
    int refine_ws = 1;                          // forward stride-2 convs of refinement layers 1 .. on the weight-stationary kernel (kernels_refws.hip)
    int refine_bwd_fused = 1;                   // training backward: data gradient of refinement layer 1 + weight gradient of layer 0 in one
                                                // launch, d(pre-activation 0) never stored (kernels_refbwd.hip; 0 = the two launches)
    int head_mfma = 1;                          // LSTM gate pre-activations of the refinement head as one fp32-MFMA GEMM over all slots
    int head_fused = 1;                         // training backward: the head's BPTT recurrence as ONE launch (0 = 9 launches per iteration)
    int sigma_grad = 0;                         // a training forward / a saved elbo also leaves d LL_e / d sigma of every evaluation (one more
                                                // per-pixel kernel per evaluation; off: no launch differs)
    int input_grad = 0;                         // bit 1 image, bit 2 pixel weights - a training forward / a saved elbo also accumulates
                                                // sum_e a_e d LL_e / d x (d w) (kernels_pixmap.hip; 0: no launch, no buffer)
    int stable_enc = 0;                         // stable_encoding: channel 8 of the encoding as a max-subtracted softmax (pixel_terms.h)
    int joint_ll = 0;                           // joint_likelihood: one mixture per pixel over the RGB vector (pixel_terms.h), every launch
                                                // of the per-pixel terms takes it; a change discards the saved passes (iodine_set_option)
    int save_bwd = 0;                           // save_for_backward: a decode / elbo keeps what its backward reads (calls.diff_*)
    int graph = 0;                              // hipGraph replay of the fixed-shape launch sequences: one instantiated graph per distinct argument tuple
    int stop_after = -1;                        // stop_after_iters
    int profile = 0;                            // 0 off, 1 the dominant conv kernels ("conv_tile_*") only, 2 every category
    int profile_stride = 1;                     // level 1: bracket every n-th launch of a category only - an event pair costs ~12 us of idle GPU
                                                // (tools/step_timeline.py); a stride coprime to the layer count samples every layer
};

// The packs below are parameter-derived device buffers the handle owns (h->owned).  Each group is allocated by one alloc_* function of
// iodine_params.cpp, next to the pack_* function of iodine_set_params that fills it; a launch site (iodine_dispatch.cpp) reads a pack only
// on the path / behind the predicate named here.

// the tuned decoder: layers 1 .. Dd-1 (index 0 unused) per DecPath, the broadcast layer and the output conv
struct DecPacks {
    float *wcls = nullptr, *wclsT = nullptr, *cmap = nullptr;    // broadcast layer (launch_dec_l0_prepare)
    std::vector<float*> bias;                   // bias copies of layers 1 .. (generic path too)
    std::vector<Pack> ws_f, ws_b;               // DEC_WS_F16 / DEC_WS_F32 (the same buffers: fp16 split with meta, or fp32): forward / data gradient
    std::vector<Pack> tile_f, tile_b;           // DEC_TILE_F16
    std::vector<float*> tile32_f, tile32_b;     // DEC_TILE_F32
    struct Out {
        float* bias = nullptr;
        Pack gemm, dgrad;                       // dec_f16(path): GEMM form / data-gradient form, one shared scale
        float *taps = nullptr, *dgrad32 = nullptr;   // exact fp32: round-1 tap form, LDS-tile f32 pack of the data gradient
        float* rows32 = nullptr;                // exact fp32, row-streaming forward (Cd 32 / 64 only, else nullptr)
    } out;
};
// the tuned refinement conv stack, per RefFamily and ref_pack_* predicate (iodine_dispatch.cpp)
struct RefPacks {
    std::vector<float*> bias;                   // every family (generic too)
    std::vector<float*> gather_f, gather_b;     // REF_GATHER: LDS-tile f32 packs, forward [0 ..] / data gradient [1 ..]
    std::vector<Pack> s2_f, s2_b;               // REF_S2_F16 / REF_S2_F32: stride-2 tile packs, forward [0 ..] / data gradient [1 ..]
    float *wk = nullptr, *wsh = nullptr;        // split first layer: weights in the internal channel order [Cr][12][9], [Cr][8][9]
    Pack split_k, split_sh;                     // ... and their stride-2 tile packs (two 16-channel convs)
    Pack l0k, l0s;                              // ref_pack_l0f: operands of the fused encoding + first layer (kernels_refl0.hip)
    std::vector<Pack> ws;                       // ref_pack_ws: layers 1 .. in the weight-stationary layout (kernels_refws.hip)
    Pack bwd01;                                 // ref_pack_bwd01: layer 1's weights as the A operand of the fused layer-1 / layer-0 backward
    float* g20 = nullptr;                       // [Cr][20][9] weight gradient in the internal order
    float *w17 = nullptr, *g17 = nullptr;       // ARCH.ENCODING subsets: [Cr][17][kr * kr] expanded weights / gradient scratch
};
// the refinement head as the forward reads it, and raw copies for the GEMMs of its backward
struct HeadPacks {
    float *mlp_wT = nullptr, *mlp_b = nullptr, *wihT = nullptr, *whhT = nullptr, *lstm_b = nullptr;   // [W_ih^T ; W_hh^T] are one block
    float *wmT = nullptr, *bm = nullptr, *wvT = nullptr, *bv = nullptr, *init_mean = nullptr, *init_logvar = nullptr;
    float *raw_mlp_w = nullptr, *raw_wih = nullptr, *raw_whh = nullptr, *raw_wm = nullptr, *raw_wv = nullptr;
};
// GENERIC fallback path (kernels_generic.hip): KERNEL_SIZE other than 3 or CONV_CHAN other than 32 / 64.  Weights re-packed to
// [tap][ci][co]; the broadcast layer is materialised; nothing of the tuned conv kernels runs.
struct GenPacks {
    std::vector<float*> wdec, wref;             // [layer]: DEC_GENERIC / REF_GENERIC
    float *wout = nullptr, *cterm = nullptr, *ident = nullptr;   // output conv pack, [P][Cd] bias + coordinate term of decoder layer 0, [9 Cd][L] identity
    // option gen_conv_precision 1 (kernels_gensplit.hip): split-fp16 slice images + per-slice inverse scales of the decoder's C -> C layers,
    // forward / data gradient; allocated by the first iodine_set_params that needs them.  split_on: the packs are current and the shape is covered
    bool split_on = false;
    std::vector<Pack> split_f, split_b;
};

// the second buffers of iodine_reconstruct_adaptive (iodine_adaptive.cpp): one device block and the pinned pair of counts, made by the first
// adaptive call, grown on demand, freed by iodine_destroy
struct AdaptiveScratch { void* dev = nullptr; size_t bytes = 0; int* counts_host = nullptr; };

struct iodine_handle {
    iodine_config cfg;
    Options opt;
    Objective obj;                              // current; initially (ARCH.SIGMA, 1, default weighting)
    CallState calls;                            // what the calls so far have left in the arena
    std::list<WeightTable> wtabs;               // every distinct weight table this handle was given (content-addressed, never rewritten)
    int wgen_next = 1;                          // generation of the next new table: counts up for the life of the handle, never re-used
    std::string err;
    std::vector<ProfCat> prof;
    ProfCat* prof_cat(const char* name) {
        for (auto& c : prof) if (c.name == name) return &c;
        prof.push_back(ProfCat()); prof.back().name = name; return &prof.back();
    }
    int L, T, K, S, P, Cd, Dd, Cr, Dr, H;       // K / T: the RUN shape (iodine_set_run_shape; cfg.slots / cfg.iters initially) - the
                                                // state a call leaves behind has the shape in buf.K / buf.T
    std::vector<ParamInfo> params;
    ParamSlots slot;
    bool params_set = false;
    int frames = 0;                             // iodine_set_frames: 0 = x is one image per batch entry, E = a clip of E frames, one per ELBO evaluation
    // iodine_set_pixel_weights: per-pixel observation weights of the NEXT compute call that takes x.  One-shot: that call takes them
    // (PixelWeights below) before anything else, so they are gone whether it succeeds or not.  The caller's memory, read on the call's stream.
    const float* pix_w = nullptr;
    int pix_w_per_frame = 0;                    // 1: (B, frames, P), one weight image per frame; 0: (B, P), the same for every frame
    int ig_call_wpf = 0;                        // (the running call's pixel weights are per frame: read by elbo_and_gradients inside the call)

    // parameter-derived device buffers (owned)
    float* lin = nullptr;                       // linspace(-1,1,S)
    unsigned* elbo_counter = nullptr;           // ticket of pixel_finalize_elbo_kernel (zero between launches)
    DecPacks dec;
    RefPacks ref;
    HeadPacks head;
    GenPacks gen;
    // ARCH.ENCODING subsets: reference input channel j of the first refinement layer = internal channel enc_map[j] (code order of
    // iodine.py:277-340); n_in < 17 -> weights expanded to / gradients gathered from the 17 internal channels
    int n_in = 17;
    int enc_map[17];
    unsigned enc_chmask = 0x1ffffu;             // bit c: internal channel c is part of the encoding (absent ones are written as 0)
    bool generic = false;                       // the DECODER runs on the generic path
    bool gen_ref = false;                       // the REFINEMENT conv stack runs on the generic path (round 5: decided separately -
                                                // the reference's default ARCH has REF.KERNEL_SIZE 3 / 32 channels beside DEC.KERNEL_SIZE 5)
    int kd = 3, kr = 3;                         // DEC / REF kernel sizes
    int rs = 2;                                 // REF.STRIDE (round 6: other strides run on the generic path's kernels)
    std::vector<float*> gacc;                   // one per parameter, reference shapes (slices of gacc_arena)
    float* gacc_arena = nullptr;
    size_t gacc_total = 0;
    std::vector<GraphEntry> graphs;             // option graph
    std::vector<std::vector<uintptr_t>> seen_keys;       // argument tuples that ran eagerly once (the next call captures)
    unsigned long long graph_clock = 0;
    long long graph_replays = 0, graph_captures = 0;
    std::vector<void*> owned;
    // round 6: DIM_LATENT / REF.MLP_UNITS that are not multiples of 4.  Lreal: the reference's DIM_LATENT when this handle runs at a padded
    // latent width (the 3-D layer-norm and the logger means are taken over the real entries); shim: this handle is only the boundary of a
    // padded INNER handle (iodine_pad.cpp)
    int Lreal = 0;
    struct PadShim* shim = nullptr;

    // workspace
    void* ws_user = nullptr; size_t ws_user_bytes = 0;
    void* ws_own = nullptr; size_t ws_own_bytes = 0;
    Buffers buf;
    AdaptiveScratch adapt;

    int fail(int code, const std::string& m) { err = m; return code; }
};

// the pending pixel weights, taken (and cleared) by the compute call that packs x
#pragma GCC visibility push(hidden)
struct PixelWeights {
    const float* w; int per_frame;
    explicit PixelWeights(iodine_handle* h) : w(h->pix_w), per_frame(h->pix_w ? h->pix_w_per_frame : 0) { h->pix_w = nullptr; h->pix_w_per_frame = 0; }
};
#pragma GCC visibility pop

#define HIPCHK(h, expr)                                                                          \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess)                                                                    \
            return (h)->fail(IODINE_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

// (diff_ready and the adapter's shim_flat_out have C names in the library's dynamic symbol table since they were written; kept, so that the
// table does not change.  Everything else below is hidden.)
extern "C" int diff_ready(iodine_handle* h, int kind, const char* who);      // a check like those below; kind 1: a saved decode, 2: a saved elbo
extern "C" int shim_flat_out(iodine_handle* h, hipStream_t st, float* flat, int accumulate);

#pragma GCC visibility push(hidden)

// cotangents of iodine_train_backward_aux (device pointers, each may be NULL): gl = d(out) / d(loss); the rest on the final evaluation's
// mean / mask / mask_logits / z and on lambda_T
// iodine_train_backward_seq adds lstm_h / lstm_c = cotangents on the LSTM state after the last update and g_state = NULL or four output
// pointers (each may be NULL): d / d (post_mean, post_logvar, h, c) of the state the forward started from
// chosen evaluations of a training forward (iodine_train_forward_frames / iodine_train_backward_frames): idx = n ascending, unique indices
// in 0..T (host memory); six device pointers in the order {z, mean, mask, mask_logits, post_mean, post_logvar}, each (n, B, ..) or NULL -
// `out` of the forward, `g` = the cotangents of the backward
struct FrameSet { const int* idx = nullptr; int n = 0; float* const* out = nullptr; const float* const* g = nullptr; };
// (frames: NULL or the cotangents on chosen evaluations)
struct AuxCot { const float *gl, *mean, *mask, *logits, *z, *pm, *plv, *lstm_h, *lstm_c; float* const* g_state; const FrameSet* frames; };

// The host-only refusals of the entry points (iodine_checks.cpp): null and batch checks, params_set, the 2^31 limits, the frames and
// iteration-weight counts, the stop_after / trajectory rule, stale state.  They launch nothing, allocate nothing and change nothing but the
// handle's message.  An entry point calls its check first; the padded boundary calls it on the inner handle with the caller's pointers (only
// their nullness matters) before it allocates scratch or launches a resize, so both kinds of handle refuse the same calls in the same words.
int set_params_check(iodine_handle* h, const float* const* dev, int n);
int reconstruct_check(iodine_handle* h, int batch, const float* x, const float* eps, const float* const* state_in, float* const* traj);
int decode_check(iodine_handle* h, int batch, const float* z);
// (iodine_adaptive.cpp; the outputs the rounds write to are required: only their nullness matters here)
int adaptive_check(iodine_handle* h, int batch, const float* x, const float* eps, const iodine_adaptive_ctl* ctl, const float* const* state_in,
                   const void* post_mean, const void* post_logvar, const void* lstm_h, const void* lstm_c, const void* iters, const void* ll,
                   const void* kl);
int scene_edit_check(iodine_handle* h, int batch, const float* z, int n_edits, const int* image, const int* slot, const int* kind,
                     const float* z_new, int chunk_images);
int elbo_check(iodine_handle* h, int batch, const float* x, const float* eps, const float* post_mean, const float* post_logvar);
constexpr int PREDICTIVE_MAX_SAMPLES = 1 << 24;    // iodine_predictive: the sample index enters the running moments as an fp32 number
int predictive_check(iodine_handle* h, int batch, int n_samples, const float* post_mean, const float* post_logvar, const float* eps,
                     const float* x, int chunk_images, const float* ll);
int train_forward_check(iodine_handle* h, int batch, const float* x, const float* eps, const float* loss, const float* const* state_in = nullptr,
                        const FrameSet* fr = nullptr);
int train_backward_check(iodine_handle* h, float* const* param_grads, int n, const AuxCot* aux = nullptr);
int train_frames_check(iodine_handle* h, const char* who, const int* idx, int n, const void* ptrs);   // the list of chosen evaluations
int decode_backward_check(iodine_handle* h, int batch);
int last_elbo_outputs_check(iodine_handle* h, int count);
int last_posterior_check(iodine_handle* h, int count);
int last_refine_state_check(iodine_handle* h, int count);
int last_train_state_check(iodine_handle* h, int count);

int train_backward_impl(iodine_handle* h, void* stream, float grad_scale, const float* grad_scale_dev, float* const* param_grads, int n,
                        int accumulate, const AuxCot* aux = nullptr);
int train_forward_impl(iodine_handle* h, void* stream, int batch, const float* x, const float* eps, const float* const* state_in, float* loss,
                       float* elbo_iter, const FrameSet* fr);

// The boundary of a zero-padded inner handle (iodine_pad.cpp), one function per entry point: h->shim != nullptr
int pad_create(iodine_handle* h);               // h: cfg and the reference-shaped parameter table are set
iodine_handle* pad_inner(iodine_handle* h);     // the padded handle behind the boundary (it holds the run shape)
void pad_destroy(iodine_handle* h);
int pad_set_params(iodine_handle* h, void* stream, const float* const* dev, int n);
size_t pad_workspace_bytes(const iodine_handle* h, int batch, int mode);
int pad_set_workspace(iodine_handle* h, void* dev_ptr, size_t bytes);
int pad_set_run_shape(iodine_handle* h, int slots, int iters);
int pad_set_frames(iodine_handle* h, int frames);
int pad_set_pixel_weights(iodine_handle* h, const float* w_dev, int per_frame);
int pad_set_objective(iodine_handle* h, double sigma, double beta, const double* iter_weights, int n_weights);
int pad_set_option(iodine_handle* h, const char* key, double value);
int pad_reconstruct_seq(iodine_handle* h, void* stream, int batch, const float* x, const float* eps, float* pred, float* mask, float* mean,
                        float* z, float* post_mean, float* post_logvar, float* elbo_iter, const float* const* state_in, float* const* traj);
int pad_reconstruct_adaptive(iodine_handle* h, void* stream, int batch, const float* x, const float* eps, const iodine_adaptive_ctl* ctl,
                             const int* budget_or_null, const float* const* state_in, float* pred, float* mask, float* mean, float* z,
                             float* post_mean, float* post_logvar, float* lstm_h, float* lstm_c, int* iters, float* ll, float* kl,
                             int* active_out_or_null);
int pad_last_refine_state(iodine_handle* h, void* stream, int count, float* lstm_h, float* lstm_c, bool train = false);
int pad_decode(iodine_handle* h, void* stream, int batch, const float* z, float* pred, float* mask, float* mean);
int pad_scene_edit(iodine_handle* h, void* stream, int batch, const float* z, int n_edits, const int* image, const int* slot, const int* kind,
                   const float* z_new, int chunk_images, float* pred, float* mask, float* mean, float* base_pred, float* base_mask,
                   float* base_mean);
int pad_elbo(iodine_handle* h, void* stream, int batch, const float* x, const float* post_mean, const float* post_logvar, const float* eps,
             float* terms);
int pad_predictive(iodine_handle* h, void* stream, int batch, int n_samples, const float* post_mean, const float* post_logvar, const float* eps,
                   const float* x, int chunk_images, float* z, float* pred_mean, float* pred_m2, float* mask_mean, float* mask_m2, int* votes,
                   float* ll);
int pad_decode_backward(iodine_handle* h, void* stream, int batch, const float* g_pred, const float* g_mask, const float* g_mean, float* dz,
                        float* flat_grads, int accumulate);
int pad_elbo_backward(iodine_handle* h, void* stream, const float* grad_out_dev, float* g_post_mean, float* g_post_logvar, float* flat_grads,
                      int accumulate);
int pad_last_elbo_outputs(iodine_handle* h, void* stream, int count, float* z, float* mean, float* mask, float* mask_logits, float* pred);
int pad_last_posterior(iodine_handle* h, void* stream, int count, float* post_mean, float* post_logvar);
int pad_train_forward(iodine_handle* h, void* stream, int batch, const float* x, const float* eps, const float* const* state_in, float* loss,
                      float* elbo_iter, const FrameSet* fr);
int pad_train_backward(iodine_handle* h, void* stream, float grad_scale, const float* grad_scale_dev, float* const* param_grads, int n,
                       int accumulate, const AuxCot* aux);
int pad_logger_scalars(iodine_handle* h, void* stream, float* out2);
int pad_last_sigma_grad(iodine_handle* h, void* stream, float* out, int n);
int pad_last_input_grad(iodine_handle* h, void* stream, float* g_x, float* g_w);
int pad_last_likelihood(iodine_handle* h, void* stream, int count, float* log_likelihood, float* k_log_likelihood);
int pad_debug_copy(iodine_handle* h, void* stream, const char* name, int iter, float* dst, size_t max_floats, size_t* n_floats);
int pad_profile_read(iodine_handle* h, const char* category, double* total_ms, long long* launches, int reset);

#pragma GCC visibility pop

#include "iodine_host.h"
