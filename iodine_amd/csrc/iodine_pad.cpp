// The reference-shaped boundary of a zero-padded inner handle: everything libiodine_hip.so knows about padding.
// Round 6 - DIM_LATENT / REF.MLP_UNITS that are not multiples of 4 (the reference takes any: iodine.py:8-32, 446-464).
// The refinement-head kernels move weight rows as 16-byte vectors, so such a model runs on an INNER handle created at Lp = ceil4(L),
// Hp = ceil4(H) with every parameter zero-padded into the wider shapes.  Padding is exact, not approximate:
//   * padded latent entries have init_mean = init_logvar = 0, their decoder-input weights and the rows of mean_update / logvar_update
//     that produce them are 0, eps is padded with 0: z = mu = 0, logvar = 0 for the whole loop, KL contribution 1/2 (0 + 1 - 0 - 1) = 0,
//     d ELBO / d lambda = 0, and the LSTM reads them through zero columns of weight_ih;
//   * padded hidden units: zero MLP row and bias -> u = ELU(ELU(0)) = 0; zero gate rows and biases -> i = f = o = 1/2, g = 0 -> c1 = h1 = 0
//     from c0 = h0 = 0; the read-out and weight_hh see them through zero columns;
//   * the one place where the WIDTH itself enters the arithmetic - the layer-norm of the lambda gradients over the latent axis
//     (iodine.py:263-272, 376-384: mean and unbiased std over L) - runs over the real L (inner->Lreal, dz_latent_kernel), and so does the
//     logger's mean of init_mean / init_logvar.
// The outer handle owns the reference-shaped boundary: parameter table, padded copies of the parameters, the element maps, scratch for the
// tensors with a latent axis (eps, z, posterior), and the gradient in padded shape; every entry point forwards to the inner handle.
#include "iodine_internal.h"

struct PadShim {
    iodine_handle* inner = nullptr;
    int L = 0, H = 0, Lp = 0, Hp = 0;
    std::vector<float*> pparam;            // padded parameter copies [param]
    std::vector<int*> pmap;                // [param][padded element] -> element of the reference-shaped tensor, or -1 (zero)
    std::vector<int> pnumel;               // padded element counts
    float* pgrad = nullptr;                // flat gradient in padded shapes (the inner handle's named_parameters() order)
    std::vector<size_t> poff;
    size_t pgrad_total = 0;
    // scratch for one call's tensors with a latent axis: grown on demand (outside the refinement loop)
    size_t cap = 0;                        // floats per buffer
    float *eps = nullptr, *z = nullptr, *pm = nullptr, *plv = nullptr, *pm_in = nullptr, *plv_in = nullptr;
    float *hs = nullptr, *cs = nullptr;    // LSTM state rows at the padded width (initial state in / state out; cotangents on the final state)
    float *gh = nullptr, *gc = nullptr;    // gradient of the initial LSTM state at the padded width (iodine_train_backward_seq, g_state)
    std::vector<void*> owned;
};

namespace {

int shim_fail(iodine_handle* h, int rc)
{
    if (rc && h->shim && h->shim->inner) h->err = h->shim->inner->err.empty() ? std::string(iodine_last_error(nullptr)) : h->shim->inner->err;
    return rc;
}

// per-dimension index map of a concatenation of segments (real length -> padded length): padded index -> real index or -1
std::vector<int> seg_map(std::initializer_list<std::pair<int, int>> segs)
{
    std::vector<int> m;
    int real0 = 0;
    for (const auto& sg : segs) {
        for (int i = 0; i < sg.second; ++i) m.push_back(i < sg.first ? real0 + i : -1);
        real0 += sg.first;
    }
    return m;
}

int shim_build(iodine_handle* h)
{
    PadShim* sh = h->shim;
    const int L = sh->L, H = sh->H, Lp = sh->Lp, Hp = sh->Hp;
    iodine_handle* in = sh->inner;
    const size_t np = h->params.size();
    if (in->params.size() != np) return h->fail(IODINE_ERR_INVALID, "padded inner handle: parameter tables differ");
    sh->pparam.assign(np, nullptr); sh->pmap.assign(np, nullptr); sh->pnumel.assign(np, 0); sh->poff.assign(np, 0);
    auto ident = [](int n) { std::vector<int> m(n); for (int i = 0; i < n; ++i) m[i] = i; return m; };
    const std::vector<int> mH = seg_map({{H, Hp}}), mL = seg_map({{L, Lp}}), m4H = seg_map({{H, Hp}, {H, Hp}, {H, Hp}, {H, Hp}}),
                           mIN = seg_map({{H, Hp}, {L, Lp}, {L, Lp}, {L, Lp}, {L, Lp}}), mL2 = seg_map({{L, Lp}, {2, 2}});
    size_t off = 0;
    for (size_t i = 0; i < np; ++i) {
        const ParamInfo &pr = h->params[i], &pp = in->params[i];
        if (pr.name != pp.name || pr.ndim != pp.ndim) return h->fail(IODINE_ERR_INVALID, "padded inner handle: parameter " + pr.name + " differs");
        std::vector<int> dm[4];
        for (int d = 0; d < 4; ++d) dm[d] = ident((int)pp.dims[d]);
        const std::string& n = pr.name;
        if (n == "refine.mlp.layers.0.weight" || n == "refine.mlp.layers.0.bias") dm[0] = mH;
        else if (n == "refine.lstm.weight_ih") { dm[0] = m4H; dm[1] = mIN; }
        else if (n == "refine.lstm.weight_hh") { dm[0] = m4H; dm[1] = mH; }
        else if (n == "refine.lstm.bias_ih" || n == "refine.lstm.bias_hh") dm[0] = m4H;
        else if (n == "refine.mean_update.weight" || n == "refine.logvar_update.weight") { dm[0] = mL; dm[1] = mH; }
        else if (n == "refine.mean_update.bias" || n == "refine.logvar_update.bias" || n == "posterior.init_mean" || n == "posterior.init_logvar") dm[0] = mL;
        else if (n == "decoder.mlc.layers.0.weight") dm[1] = mL2;          // [Cd][L latent channels | x, y][k][k]
        for (int d = 0; d < 4; ++d)
            if ((long long)dm[d].size() != pp.dims[d]) return h->fail(IODINE_ERR_INVALID, "padded inner handle: shape of " + n);
        const size_t numel = pp.numel();
        std::vector<int> map(numel);
        size_t e = 0;
        for (int a = 0; a < (int)pp.dims[0]; ++a)
            for (int b2 = 0; b2 < (int)pp.dims[1]; ++b2)
                for (int c = 0; c < (int)pp.dims[2]; ++c)
                    for (int d = 0; d < (int)pp.dims[3]; ++d, ++e) {
                        const int ia = dm[0][a], ib = dm[1][b2], ic = dm[2][c], id = dm[3][d];
                        map[e] = (ia < 0 || ib < 0 || ic < 0 || id < 0) ? -1
                                 : (int)((((size_t)ia * pr.dims[1] + ib) * pr.dims[2] + ic) * pr.dims[3] + id);
                    }
        void *dmap = nullptr, *dpar = nullptr;
        HIPCHK(h, hipMalloc(&dmap, numel * sizeof(int))); sh->owned.push_back(dmap);
        HIPCHK(h, hipMemcpy(dmap, map.data(), numel * sizeof(int), hipMemcpyHostToDevice));
        HIPCHK(h, hipMalloc(&dpar, numel * sizeof(float))); sh->owned.push_back(dpar);
        sh->pmap[i] = (int*)dmap; sh->pparam[i] = (float*)dpar; sh->pnumel[i] = (int)numel; sh->poff[i] = off;
        off += numel;
    }
    sh->pgrad_total = off;
    void* g = nullptr;
    HIPCHK(h, hipMalloc(&g, off * sizeof(float))); sh->owned.push_back(g);
    sh->pgrad = (float*)g;
    return IODINE_OK;
}

// scratch for (rows x Lp) tensors of a call; rows_eps = (T + 1) * N for the noise, N for the others
// (the new set is allocated in full before the old one is released: a failed hipMalloc leaves the old set and `cap` as they were)
int shim_scratch(iodine_handle* h, size_t floats)
{
    PadShim* sh = h->shim;
    if (floats <= sh->cap) return IODINE_OK;
    constexpr int NB = 10;
    float** bufs[NB] = {&sh->eps, &sh->z, &sh->pm, &sh->plv, &sh->pm_in, &sh->plv_in, &sh->hs, &sh->cs, &sh->gh, &sh->gc};
    void* fresh[NB] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    for (int i = 0; i <= NB; ++i) {
        // (i == NB: the old buffers may still be read by queued work)
        const hipError_t e = i < NB ? hipMalloc(&fresh[i], floats * sizeof(float)) : (sh->cap > 0 ? hipDeviceSynchronize() : hipSuccess);
        if (e != hipSuccess) {
            for (int j = 0; j < i && j < NB; ++j) (void)hipFree(fresh[j]);
            return h->fail(IODINE_ERR_HIP, std::string(i < NB ? "hipMalloc" : "hipDeviceSynchronize") + " (padded-handle scratch): " +
                                               hipGetErrorString(e));
        }
    }
    for (int i = 0; i < NB; ++i) {
        if (*bufs[i]) (void)hipFree(*bufs[i]);
        *bufs[i] = (float*)fresh[i];
    }
    sh->cap = floats;
    return IODINE_OK;
}

}  // namespace

// padded flat gradient -> the caller's reference-shaped one (diff_flat_out of the compute handle: only the decoder and the initial
// posterior can have received anything; when accumulating, the refinement network's gradients are not touched)
int shim_flat_out(iodine_handle* h, hipStream_t st, float* flat, int accumulate)
{
    PadShim* sh = h->shim;
    size_t off = 0;
    for (size_t p = 0; p < h->params.size(); ++p) {
        if (!accumulate || (int)p >= h->slot.dec_w[0])
            HIPCHK(h, launch_pad_scatter(st, sh->pgrad + sh->poff[p], sh->pmap[p], flat + off, sh->pnumel[p], accumulate));
        off += h->params[p].numel();
    }
    return IODINE_OK;
}

// ---- the entry points.  Each reads the run shape, the frames setting and the batch of the last call from the inner handle, asks the inner
// handle's check (iodine_internal.h) before its first scratch allocation or launch, and forwards a refusal's message with shim_fail.

// pixel weights are one-shot: whatever way a call that takes x leaves the boundary, the inner handle holds none afterwards (the inner
// call takes them first; this covers the boundary's own refusals and failures before it)
struct PendingWeights {
    iodine_handle* in;
    explicit PendingWeights(iodine_handle* inner) : in(inner) {}
    ~PendingWeights() { in->pix_w = nullptr; in->pix_w_per_frame = 0; }
};

int pad_create(iodine_handle* h)
{
    PadShim* sh = h->shim = new PadShim();
    sh->L = h->cfg.dim_latent; sh->H = h->cfg.ref_mlp_units;
    sh->Lp = (sh->L + 3) / 4 * 4; sh->Hp = (sh->H + 3) / 4 * 4;
    iodine_config pc = h->cfg;
    pc.dim_latent = sh->Lp; pc.ref_mlp_units = sh->Hp;
    const int rc = iodine_create(&pc, &sh->inner);
    if (rc) return rc;                                                  // (the thread's error slot holds the inner message)
    sh->inner->Lreal = sh->L;
    const int rb = shim_build(h);
    return rb ? free_fail(rb, h->err) : IODINE_OK;
}

void pad_destroy(iodine_handle* h)
{
    PadShim* sh = h->shim;
    if (sh->inner) iodine_destroy(sh->inner);
    for (void* p : sh->owned) (void)hipFree(p);
    for (float* p : {sh->eps, sh->z, sh->pm, sh->plv, sh->pm_in, sh->plv_in, sh->hs, sh->cs, sh->gh, sh->gc}) if (p) (void)hipFree(p);
    delete sh;
    h->shim = nullptr;
}

int pad_set_params(iodine_handle* h, void* stream, const float* const* dev, int n)
{
    PadShim* sh = h->shim;                                     // reference shapes -> zero-padded copies -> the inner handle
    if (int rc = set_params_check(sh->inner, dev, n)) return shim_fail(h, rc);
    for (int i = 0; i < n; ++i) HIPCHK(h, launch_pad_gather((hipStream_t)stream, dev[i], sh->pmap[i], sh->pparam[i], sh->pnumel[i]));
    return shim_fail(h, iodine_set_params(sh->inner, stream, sh->pparam.data(), n));
}

// settings and read-outs without a latent axis: the inner handle's own
size_t pad_workspace_bytes(const iodine_handle* h, int batch, int mode) { return iodine_workspace_bytes(h->shim->inner, batch, mode); }
int pad_set_workspace(iodine_handle* h, void* dev_ptr, size_t bytes) { return shim_fail(h, iodine_set_workspace(h->shim->inner, dev_ptr, bytes)); }
iodine_handle* pad_inner(iodine_handle* h) { return h->shim->inner; }
int pad_set_run_shape(iodine_handle* h, int slots, int iters) { return shim_fail(h, iodine_set_run_shape(h->shim->inner, slots, iters)); }
int pad_set_frames(iodine_handle* h, int frames) { return shim_fail(h, iodine_set_frames(h->shim->inner, frames)); }
int pad_set_pixel_weights(iodine_handle* h, const float* w_dev, int per_frame)
{
    return shim_fail(h, iodine_set_pixel_weights(h->shim->inner, w_dev, per_frame));      // (the inner handle packs x: it holds them)
}
int pad_set_objective(iodine_handle* h, double sigma, double beta, const double* iter_weights, int n_weights)
{
    return shim_fail(h, iodine_set_objective(h->shim->inner, sigma, beta, iter_weights, n_weights));
}
int pad_set_option(iodine_handle* h, const char* key, double value) { return shim_fail(h, iodine_set_option(h->shim->inner, key, value)); }
int pad_logger_scalars(iodine_handle* h, void* stream, float* out2) { return shim_fail(h, iodine_logger_scalars(h->shim->inner, stream, out2)); }
int pad_last_sigma_grad(iodine_handle* h, void* stream, float* out, int n) { return shim_fail(h, iodine_last_sigma_grad(h->shim->inner, stream, out, n)); }
// (per-pixel quantities: the padding is in the latent and channel widths, the slots and pixels are the caller's)
int pad_last_input_grad(iodine_handle* h, void* stream, float* g_x, float* g_w) { return shim_fail(h, iodine_last_input_grad(h->shim->inner, stream, g_x, g_w)); }
int pad_last_likelihood(iodine_handle* h, void* stream, int count, float* log_likelihood, float* k_log_likelihood)
{
    return shim_fail(h, iodine_last_likelihood(h->shim->inner, stream, count, log_likelihood, k_log_likelihood));
}
int pad_debug_copy(iodine_handle* h, void* stream, const char* name, int iter, float* dst, size_t max_floats, size_t* n_floats)
{
    return shim_fail(h, iodine_debug_copy(h->shim->inner, stream, name, iter, dst, max_floats, n_floats));   // (padded widths)
}
int pad_profile_read(iodine_handle* h, const char* category, double* total_ms, long long* launches, int reset)
{
    return shim_fail(h, iodine_profile_read(h->shim->inner, category, total_ms, launches, reset));
}

int pad_reconstruct_seq(iodine_handle* h, void* stream, int batch, const float* x, const float* eps, float* pred, float* mask, float* mean,
                        float* z, float* post_mean, float* post_logvar, float* elbo_iter, const float* const* state_in, float* const* traj)
{
    PadShim* sh = h->shim;
    iodine_handle* in = sh->inner;
    PendingWeights once(in);
    if (int rc = reconstruct_check(in, batch, x, eps, state_in, traj)) return shim_fail(h, rc);
    hipStream_t st = (hipStream_t)stream;
    const long long N = (long long)batch * in->K, R = (long long)(in->T + 1) * N;
    if (int r = shim_scratch(h, std::max((size_t)R * sh->Lp, state_in ? (size_t)N * sh->Hp : (size_t)0))) return r;
    HIPCHK(h, launch_resize_rows(st, eps, sh->eps, R, sh->L, sh->Lp));
    const float* pstate[4] = {sh->pm_in, sh->plv_in, sh->hs, sh->cs};
    if (state_in) {                                        // lambda: L -> padded L, LSTM state: MLP_UNITS -> padded, zero columns
        HIPCHK(h, launch_resize_rows(st, state_in[0], sh->pm_in, N, sh->L, sh->Lp));
        HIPCHK(h, launch_resize_rows(st, state_in[1], sh->plv_in, N, sh->L, sh->Lp));
        HIPCHK(h, launch_resize_rows(st, state_in[2], sh->hs, N, sh->H, sh->Hp));
        HIPCHK(h, launch_resize_rows(st, state_in[3], sh->cs, N, sh->H, sh->Hp));
    }
    const int rc = iodine_reconstruct_seq(in, stream, batch, x, sh->eps, pred, mask, mean, z ? sh->z : nullptr, post_mean ? sh->pm : nullptr,
                                          post_logvar ? sh->plv : nullptr, elbo_iter, state_in ? pstate : nullptr, traj);
    if (rc) return shim_fail(h, rc);
    if (z) HIPCHK(h, launch_resize_rows(st, sh->z, z, N, sh->Lp, sh->L));
    if (post_mean) HIPCHK(h, launch_resize_rows(st, sh->pm, post_mean, N, sh->Lp, sh->L));
    if (post_logvar) HIPCHK(h, launch_resize_rows(st, sh->plv, post_logvar, N, sh->Lp, sh->L));
    return IODINE_OK;
}

// as pad_reconstruct_seq; the LSTM state comes back too (sh->gh / gc: sh->hs / cs hold the initial one)
int pad_reconstruct_adaptive(iodine_handle* h, void* stream, int batch, const float* x, const float* eps, const iodine_adaptive_ctl* ctl,
                             const int* budget_or_null, const float* const* state_in, float* pred, float* mask, float* mean, float* z,
                             float* post_mean, float* post_logvar, float* lstm_h, float* lstm_c, int* iters, float* ll, float* kl,
                             int* active_out_or_null)
{
    PadShim* sh = h->shim;
    iodine_handle* in = sh->inner;
    PendingWeights once(in);
    if (int rc = adaptive_check(in, batch, x, eps, ctl, state_in, post_mean, post_logvar, lstm_h, lstm_c, iters, ll, kl)) return shim_fail(h, rc);
    hipStream_t st = (hipStream_t)stream;
    const long long N = (long long)batch * in->K, R = (long long)(ctl->max_iters + 1) * N;
    if (int r = shim_scratch(h, std::max((size_t)R * sh->Lp, (size_t)N * sh->Hp))) return r;
    HIPCHK(h, launch_resize_rows(st, eps, sh->eps, R, sh->L, sh->Lp));
    const float* pstate[4] = {sh->pm_in, sh->plv_in, sh->hs, sh->cs};
    if (state_in) {
        HIPCHK(h, launch_resize_rows(st, state_in[0], sh->pm_in, N, sh->L, sh->Lp));
        HIPCHK(h, launch_resize_rows(st, state_in[1], sh->plv_in, N, sh->L, sh->Lp));
        HIPCHK(h, launch_resize_rows(st, state_in[2], sh->hs, N, sh->H, sh->Hp));
        HIPCHK(h, launch_resize_rows(st, state_in[3], sh->cs, N, sh->H, sh->Hp));
    }
    const int rc = iodine_reconstruct_adaptive(in, stream, batch, x, sh->eps, ctl, budget_or_null, state_in ? pstate : nullptr, pred, mask, mean,
                                               z ? sh->z : nullptr, sh->pm, sh->plv, sh->gh, sh->gc, iters, ll, kl, active_out_or_null);
    if (rc) return shim_fail(h, rc);
    if (z) HIPCHK(h, launch_resize_rows(st, sh->z, z, N, sh->Lp, sh->L));
    HIPCHK(h, launch_resize_rows(st, sh->pm, post_mean, N, sh->Lp, sh->L));
    HIPCHK(h, launch_resize_rows(st, sh->plv, post_logvar, N, sh->Lp, sh->L));
    HIPCHK(h, launch_resize_rows(st, sh->gh, lstm_h, N, sh->Hp, sh->H));
    HIPCHK(h, launch_resize_rows(st, sh->gc, lstm_c, N, sh->Hp, sh->H));
    return IODINE_OK;
}

// (train: iodine_last_train_state - the same read-out after a training forward)
int pad_last_refine_state(iodine_handle* h, void* stream, int count, float* lstm_h, float* lstm_c, bool train)
{
    PadShim* sh = h->shim;
    if (int rc = train ? last_train_state_check(sh->inner, count) : last_refine_state_check(sh->inner, count)) return shim_fail(h, rc);
    hipStream_t st = (hipStream_t)stream;
    const long long N = (long long)count * sh->inner->buf.K;        // the slots of the call that produced the state, not the run shape
    if (int r = shim_scratch(h, (size_t)N * sh->Hp)) return r;
    const int rc = (train ? iodine_last_train_state : iodine_last_refine_state)(sh->inner, stream, count, lstm_h ? sh->hs : nullptr,
                                                                                 lstm_c ? sh->cs : nullptr);
    if (rc) return shim_fail(h, rc);
    if (lstm_h) HIPCHK(h, launch_resize_rows(st, sh->hs, lstm_h, N, sh->Hp, sh->H));
    if (lstm_c) HIPCHK(h, launch_resize_rows(st, sh->cs, lstm_c, N, sh->Hp, sh->H));
    return IODINE_OK;
}

int pad_decode(iodine_handle* h, void* stream, int batch, const float* z, float* pred, float* mask, float* mean)
{
    PadShim* sh = h->shim;
    if (int rc = decode_check(sh->inner, batch, z)) return shim_fail(h, rc);
    const long long N = (long long)batch * sh->inner->K;
    if (int r = shim_scratch(h, (size_t)N * sh->Lp)) return r;
    HIPCHK(h, launch_resize_rows((hipStream_t)stream, z, sh->z, N, sh->L, sh->Lp));
    return shim_fail(h, iodine_decode(sh->inner, stream, batch, sh->z, pred, mask, mean));
}

int pad_scene_edit(iodine_handle* h, void* stream, int batch, const float* z, int n_edits, const int* image, const int* slot, const int* kind,
                   const float* z_new, int chunk_images, float* pred, float* mask, float* mean, float* base_pred, float* base_mask,
                   float* base_mean)
{
    PadShim* sh = h->shim;
    if (int rc = scene_edit_check(sh->inner, batch, z, n_edits, image, slot, kind, z_new, chunk_images)) return shim_fail(h, rc);
    const long long N = (long long)batch * sh->inner->K;
    if (int r = shim_scratch(h, (size_t)std::max(N, (long long)n_edits) * sh->Lp)) return r;
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(h, launch_resize_rows(st, z, sh->z, N, sh->L, sh->Lp));
    // z_new (n_edits, L) -> sh->pm (n_edits, Lp), row for row; the rows of removals are not read (and stay as they are: never decoded)
    for (int e = 0; e < n_edits;) {
        if (kind[e] == 1) { ++e; continue; }
        int f = e;
        while (f < n_edits && kind[f] == 0) ++f;
        HIPCHK(h, launch_resize_rows(st, z_new + (size_t)e * sh->L, sh->pm + (size_t)e * sh->Lp, f - e, sh->L, sh->Lp));
        e = f;
    }
    return shim_fail(h, iodine_scene_edit(sh->inner, stream, batch, sh->z, n_edits, image, slot, kind, z_new ? sh->pm : nullptr, chunk_images,
                                          pred, mask, mean, base_pred, base_mask, base_mean));
}

int pad_elbo(iodine_handle* h, void* stream, int batch, const float* x, const float* post_mean, const float* post_logvar, const float* eps,
             float* terms)
{
    PadShim* sh = h->shim;
    PendingWeights once(sh->inner);
    if (int rc = elbo_check(sh->inner, batch, x, eps, post_mean, post_logvar)) return shim_fail(h, rc);
    hipStream_t st = (hipStream_t)stream;
    const long long N = (long long)batch * sh->inner->K;
    if (int r = shim_scratch(h, (size_t)N * sh->Lp)) return r;
    HIPCHK(h, launch_resize_rows(st, eps, sh->eps, N, sh->L, sh->Lp));
    if (post_mean) {
        HIPCHK(h, launch_resize_rows(st, post_mean, sh->pm_in, N, sh->L, sh->Lp));
        HIPCHK(h, launch_resize_rows(st, post_logvar, sh->plv_in, N, sh->L, sh->Lp));
    }
    return shim_fail(h, iodine_elbo(sh->inner, stream, batch, x, post_mean ? sh->pm_in : nullptr, post_mean ? sh->plv_in : nullptr, sh->eps, terms));
}

// (the per-pixel outputs have no latent axis: the caller's own buffers; padded latent entries have mean = logvar = eps = 0, so z = 0 there)
int pad_predictive(iodine_handle* h, void* stream, int batch, int n_samples, const float* post_mean, const float* post_logvar, const float* eps,
                   const float* x, int chunk_images, float* z, float* pred_mean, float* pred_m2, float* mask_mean, float* mask_m2, int* votes,
                   float* ll)
{
    PadShim* sh = h->shim;
    PendingWeights once(sh->inner);
    if (int rc = predictive_check(sh->inner, batch, n_samples, post_mean, post_logvar, eps, x, chunk_images, ll)) return shim_fail(h, rc);
    hipStream_t st = (hipStream_t)stream;
    const long long N = (long long)batch * sh->inner->K, R = (long long)n_samples * N;
    if (int r = shim_scratch(h, (size_t)R * sh->Lp)) return r;
    HIPCHK(h, launch_resize_rows(st, eps, sh->eps, R, sh->L, sh->Lp));
    if (post_mean) {
        HIPCHK(h, launch_resize_rows(st, post_mean, sh->pm_in, N, sh->L, sh->Lp));
        HIPCHK(h, launch_resize_rows(st, post_logvar, sh->plv_in, N, sh->L, sh->Lp));
    }
    const int rc = iodine_predictive(sh->inner, stream, batch, n_samples, post_mean ? sh->pm_in : nullptr, post_mean ? sh->plv_in : nullptr, sh->eps,
                                     x, chunk_images, z ? sh->z : nullptr, pred_mean, pred_m2, mask_mean, mask_m2, votes, ll);
    if (rc) return shim_fail(h, rc);
    if (z) HIPCHK(h, launch_resize_rows(st, sh->z, z, R, sh->Lp, sh->L));
    return IODINE_OK;
}

// (the two single-pass backwards write into the scratch their forward sized: the inner call is their first launch, and checks first)
int pad_decode_backward(iodine_handle* h, void* stream, int batch, const float* g_pred, const float* g_mask, const float* g_mean, float* dz,
                        float* flat_grads, int accumulate)
{
    PadShim* sh = h->shim;
    hipStream_t st = (hipStream_t)stream;
    const int rc = iodine_decode_backward(sh->inner, stream, batch, g_pred, g_mask, g_mean, dz ? sh->z : nullptr, flat_grads ? sh->pgrad : nullptr, 0);
    if (rc) return shim_fail(h, rc);
    if (dz) HIPCHK(h, launch_resize_rows(st, sh->z, dz, (long long)batch * sh->inner->K, sh->Lp, sh->L));
    return flat_grads ? shim_flat_out(h, st, flat_grads, accumulate) : IODINE_OK;
}

int pad_elbo_backward(iodine_handle* h, void* stream, const float* grad_out_dev, float* g_post_mean, float* g_post_logvar, float* flat_grads,
                      int accumulate)
{
    PadShim* sh = h->shim;
    iodine_handle* in = sh->inner;
    if (int rc = diff_ready(in, 2, "iodine_elbo_backward")) return shim_fail(h, rc);
    hipStream_t st = (hipStream_t)stream;
    const long long N = (long long)in->calls.diff_batch * in->buf.K;
    const int rc = iodine_elbo_backward(in, stream, grad_out_dev, g_post_mean ? sh->pm : nullptr, g_post_logvar ? sh->plv : nullptr,
                                        flat_grads ? sh->pgrad : nullptr, 0);
    if (rc) return shim_fail(h, rc);
    if (g_post_mean) HIPCHK(h, launch_resize_rows(st, sh->pm, g_post_mean, N, sh->Lp, sh->L));
    if (g_post_logvar) HIPCHK(h, launch_resize_rows(st, sh->plv, g_post_logvar, N, sh->Lp, sh->L));
    return flat_grads ? shim_flat_out(h, st, flat_grads, accumulate) : IODINE_OK;
}

int pad_last_elbo_outputs(iodine_handle* h, void* stream, int count, float* z, float* mean, float* mask, float* mask_logits, float* pred)
{
    PadShim* sh = h->shim;
    if (int rc = last_elbo_outputs_check(sh->inner, count)) return shim_fail(h, rc);
    const long long N = (long long)count * sh->inner->buf.K;        // the slots of the call that produced the state, not the run shape
    if (z) if (int r = shim_scratch(h, (size_t)N * sh->Lp)) return r;
    const int rc = iodine_last_elbo_outputs(sh->inner, stream, count, z ? sh->z : nullptr, mean, mask, mask_logits, pred);
    if (rc) return shim_fail(h, rc);
    if (z) HIPCHK(h, launch_resize_rows((hipStream_t)stream, sh->z, z, N, sh->Lp, sh->L));
    return IODINE_OK;
}

int pad_last_posterior(iodine_handle* h, void* stream, int count, float* post_mean, float* post_logvar)
{
    PadShim* sh = h->shim;
    if (int rc = last_posterior_check(sh->inner, count)) return shim_fail(h, rc);
    const long long N = (long long)count * sh->inner->buf.K;
    if (int r = shim_scratch(h, (size_t)N * sh->Lp)) return r;
    const int rc = iodine_last_posterior(sh->inner, stream, count, post_mean ? sh->pm : nullptr, post_logvar ? sh->plv : nullptr);
    if (rc) return shim_fail(h, rc);
    if (post_mean) HIPCHK(h, launch_resize_rows((hipStream_t)stream, sh->pm, post_mean, N, sh->Lp, sh->L));
    if (post_logvar) HIPCHK(h, launch_resize_rows((hipStream_t)stream, sh->plv, post_logvar, N, sh->Lp, sh->L));
    return IODINE_OK;
}

int pad_train_forward(iodine_handle* h, void* stream, int batch, const float* x, const float* eps, const float* const* state_in, float* loss,
                      float* elbo_iter, const FrameSet* fr)
{
    PadShim* sh = h->shim;
    iodine_handle* in = sh->inner;
    PendingWeights once(in);
    if (int rc = train_forward_check(in, batch, x, eps, loss, state_in, fr)) return shim_fail(h, rc);
    hipStream_t st = (hipStream_t)stream;
    const long long N = (long long)batch * in->K, R = (long long)(in->T + 1) * N;
    if (int r = shim_scratch(h, std::max((size_t)R * sh->Lp, state_in ? (size_t)N * sh->Hp : (size_t)0))) return r;
    HIPCHK(h, launch_resize_rows(st, eps, sh->eps, R, sh->L, sh->Lp));
    const float* pstate[4] = {sh->pm_in, sh->plv_in, sh->hs, sh->cs};
    if (state_in) {                                        // as pad_reconstruct_seq: zero columns at the padded widths
        HIPCHK(h, launch_resize_rows(st, state_in[0], sh->pm_in, N, sh->L, sh->Lp));
        HIPCHK(h, launch_resize_rows(st, state_in[1], sh->plv_in, N, sh->L, sh->Lp));
        HIPCHK(h, launch_resize_rows(st, state_in[2], sh->hs, N, sh->H, sh->Hp));
        HIPCHK(h, launch_resize_rows(st, state_in[3], sh->cs, N, sh->H, sh->Hp));
    }
    if (!fr) return shim_fail(h, iodine_train_forward_seq(in, stream, batch, x, sh->eps, state_in ? pstate : nullptr, loss, elbo_iter));
    // chosen evaluations: the tensors with a latent axis come back at the padded width (at most (T + 1) * N rows each: the scratch holds them)
    float* const pout[6] = {fr->out[0] ? sh->z : nullptr, fr->out[1], fr->out[2], fr->out[3], fr->out[4] ? sh->pm : nullptr,
                            fr->out[5] ? sh->plv : nullptr};
    FrameSet pf = *fr; pf.out = pout;
    if (int rc = train_forward_impl(in, stream, batch, x, sh->eps, state_in ? pstate : nullptr, loss, elbo_iter, &pf)) return shim_fail(h, rc);
    for (int q : {0, 4, 5})
        if (fr->out[q]) HIPCHK(h, launch_resize_rows(st, pout[q], fr->out[q], (long long)fr->n * N, sh->Lp, sh->L));
    return IODINE_OK;
}

// the inner handle writes its (scaled) gradient in padded shapes; the real entries are scattered (or added) into the caller's tensors
int pad_train_backward(iodine_handle* h, void* stream, float grad_scale, const float* grad_scale_dev, float* const* param_grads, int n,
                       int accumulate, const AuxCot* aux)
{
    PadShim* sh = h->shim;
    iodine_handle* in = sh->inner;
    if (int rc = train_backward_check(in, param_grads, n, aux)) return shim_fail(h, rc);
    hipStream_t st = (hipStream_t)stream;
    std::vector<float*> ptrs(h->params.size());
    for (size_t p = 0; p < ptrs.size(); ++p) ptrs[p] = sh->pgrad + sh->poff[p];
    AuxCot pa;
    FrameSet pf;
    const float* pfg[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    float* pgs[4] = {nullptr, nullptr, nullptr, nullptr};
    const long long N = (long long)in->calls.fwd_batch * in->buf.K;
    if (aux) {
        // cotangents with a latent axis: rows widened to the padded width (zeros in the padded entries), like iodine_decode_backward's dz
        const bool hid = aux->lstm_h || aux->lstm_c || aux->g_state;
        const size_t nf = aux->frames && aux->frames->n > 0 ? (size_t)aux->frames->n : 0;
        if (int r = shim_scratch(h, std::max(std::max((size_t)N * sh->Lp, hid ? (size_t)N * sh->Hp : (size_t)0), (size_t)(3 * nf * N * sh->Lp)))) return r;
        pa = *aux;
        if (nf) {
            // ... those on chosen evaluations too: three kinds of (n_frames * N) rows, back to back in the (free) noise scratch
            pf = *aux->frames;
            int slot = 0;
            for (int q = 0; q < 6; ++q) {
                pfg[q] = aux->frames->g[q];
                if ((q == 0 || q >= 4) && pfg[q]) {
                    float* dst = sh->eps + (size_t)slot * nf * N * sh->Lp;
                    HIPCHK(h, launch_resize_rows(st, pfg[q], dst, (long long)nf * N, sh->L, sh->Lp));
                    pfg[q] = dst;
                }
                if (q == 0 || q >= 4) ++slot;
            }
            pf.g = pfg; pa.frames = &pf;
        }
        // ... and those on the LSTM state after the last update; the gradient of the initial state comes back at the padded widths
        if (aux->lstm_h) { HIPCHK(h, launch_resize_rows(st, aux->lstm_h, sh->hs, N, sh->H, sh->Hp)); pa.lstm_h = sh->hs; }
        if (aux->lstm_c) { HIPCHK(h, launch_resize_rows(st, aux->lstm_c, sh->cs, N, sh->H, sh->Hp)); pa.lstm_c = sh->cs; }
        if (aux->g_state) {
            float* const scr[4] = {sh->pm, sh->plv, sh->gh, sh->gc};
            for (int j = 0; j < 4; ++j) pgs[j] = aux->g_state[j] ? scr[j] : nullptr;
            pa.g_state = pgs;
        }
        if (aux->z) { HIPCHK(h, launch_resize_rows(st, aux->z, sh->z, N, sh->L, sh->Lp)); pa.z = sh->z; }
        if (aux->pm) { HIPCHK(h, launch_resize_rows(st, aux->pm, sh->pm_in, N, sh->L, sh->Lp)); pa.pm = sh->pm_in; }
        if (aux->plv) { HIPCHK(h, launch_resize_rows(st, aux->plv, sh->plv_in, N, sh->L, sh->Lp)); pa.plv = sh->plv_in; }
    }
    const int rc = train_backward_impl(in, stream, grad_scale, grad_scale_dev, ptrs.data(), n, 0, aux ? &pa : nullptr);
    if (rc) return shim_fail(h, rc);
    for (int j = 0; j < 4; ++j)                              // the state's gradient, sliced back to the real widths
        if (pgs[j]) HIPCHK(h, launch_resize_rows(st, pgs[j], aux->g_state[j], N, j < 2 ? sh->Lp : sh->Hp, j < 2 ? sh->L : sh->H));
    for (size_t p = 0; p < ptrs.size(); ++p)
        if (param_grads[p]) HIPCHK(h, launch_pad_scatter(st, ptrs[p], sh->pmap[p], param_grads[p], sh->pnumel[p], accumulate));
    return IODINE_OK;
}
