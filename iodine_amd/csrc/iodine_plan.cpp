// What a call needs before it may launch: the parameter table, the workspace carve-up (plan) and its owner (ensure_workspace), the
// hipGraph cache's key and clean-up, the readiness check every compute call starts with.  Declarations: iodine_host.h.
#include "iodine_internal.h"

void build_param_table(iodine_handle* h)
{
    // names / shapes of the reference module tree in named_parameters() order
    // (iodine.py:26-33, 412-423, 446-464, 543-557, 570-584, 596-604)
    // (returns the parameter's index: h->slot keeps it, so nothing downstream looks a parameter up by name)
    auto add = [&](const std::string& n, std::initializer_list<long long> d) {
        ParamInfo p; p.name = n; p.ndim = (int)d.size(); int i = 0;
        for (long long v : d) p.dims[i++] = v;
        for (; i < 4; ++i) p.dims[i] = 1;
        h->params.push_back(p);
        return (int)h->params.size() - 1;
    };
    const iodine_config& c = h->cfg;
    ParamSlots& s = h->slot;
    int cin = h->n_in;
    for (int i = 0; i < c.ref_conv_layers; ++i) {
        s.ref_w.push_back(add("refine.mlc.layers." + std::to_string(i) + ".weight", {c.ref_conv_chan, cin, c.ref_kernel_size, c.ref_kernel_size}));
        s.ref_b.push_back(add("refine.mlc.layers." + std::to_string(i) + ".bias", {c.ref_conv_chan}));
        cin = c.ref_conv_chan;
    }
    const long long H = c.ref_mlp_units, L = c.dim_latent;
    s.mlp_w = add("refine.mlp.layers.0.weight", {H, c.ref_conv_chan});
    s.mlp_b = add("refine.mlp.layers.0.bias", {H});
    s.wih = add("refine.lstm.weight_ih", {4 * H, H + 4 * L});
    s.whh = add("refine.lstm.weight_hh", {4 * H, H});
    s.bih = add("refine.lstm.bias_ih", {4 * H});
    s.bhh = add("refine.lstm.bias_hh", {4 * H});
    s.wm = add("refine.mean_update.weight", {L, H});
    s.bm = add("refine.mean_update.bias", {L});
    s.wv = add("refine.logvar_update.weight", {L, H});
    s.bv = add("refine.logvar_update.bias", {L});
    cin = c.dim_latent + 2;
    for (int i = 0; i < c.dec_conv_layers; ++i) {
        s.dec_w.push_back(add("decoder.mlc.layers." + std::to_string(i) + ".weight", {c.dec_conv_chan, cin, c.dec_kernel_size, c.dec_kernel_size}));
        s.dec_b.push_back(add("decoder.mlc.layers." + std::to_string(i) + ".bias", {c.dec_conv_chan}));
        cin = c.dec_conv_chan;
    }
    s.out_w = add("decoder.conv.weight", {4, c.dec_conv_chan, c.dec_kernel_size, c.dec_kernel_size});
    s.out_b = add("decoder.conv.bias", {4});
    s.init_mean = add("posterior.init_mean", {L});
    s.init_logvar = add("posterior.init_logvar", {L});
}

// spatial size of refinement layer l's OUTPUT
// (k x k, pad k // 2, stride rs: floor((s + 2 (k // 2) - k) / rs) + 1 = (s - 1) / rs + 1 for odd k)
int ref_out_size(const iodine_handle* h, int s) { return (s - 1) / h->rs + 1; }

void plan(const iodine_handle* h, int B, int mode, Arena& a, Buffers& b)
{
    const int N = B * h->K, P = h->P, L = h->L, Cd = h->Cd, Cr = h->Cr, H = h->H, T = h->T;
    const bool gen_dec = dec_path(h) == DEC_GENERIC, gen_ref = ref_family(h) == REF_GENERIC;
    b.B = B; b.mode = mode; b.K = h->K; b.T = h->T;
    b.F = h->frames > 0 ? h->frames : 1;
    b.x4 = a.take<float>((size_t)b.F * B * P * 4);           // [F][B][P][4]: evaluation i reads frame i (x4_frame)
    b.V = a.take<float>((size_t)N * 9 * Cd);
    b.dec_out = a.take<float>((size_t)N * P * 4);
    b.g = a.take<float>((size_t)N * P * 4);
    b.part = a.take<double>((size_t)B * pixel_blocks_per_image(P) * (6 * h->K + 3));
    b.lnstat = a.take<float>((size_t)N * 8);
    b.ll_img = a.take<float>((size_t)B);
    b.img_terms = a.take<float>((size_t)(T + 1) * B * 2);
    b.scal = a.take<float>((size_t)(T + 1) * 3 + 4);
    b.rows = a.take<float>((size_t)N * h->S * 3 * Cd);
    b.rows_p = a.take<float>((size_t)N * h->S * (h->S / 16 > 0 ? h->S / 16 : 1) * (mode != 0 ? 4 : 3) * Cd);   // per-tile row sums (EPI_L0ROWS / EPI_L0ROWSX)
    b.l0scr = a.take<float>(l0_rows_scratch_floats(N, Cd));
    b.Rc = a.take<float>((size_t)N * 9 * Cd);
    b.pm = a.take<float>((size_t)N * L);
    b.plv = a.take<float>((size_t)N * L);
    b.act.resize(h->Dd);
    for (int l = 0; l < h->Dd; ++l) b.act[l] = a.take<float>((size_t)N * P * Cd);
    b.dpre[0] = a.take<float>((size_t)N * P * Cd);
    b.dpre[1] = a.take<float>((size_t)N * P * Cd);
    b.tmax_act.resize(h->Dd);
    for (int l = 0; l < h->Dd; ++l) b.tmax_act[l] = a.take<float>(conv_ws_tmax_floats(N, h->S));
    b.tmax_dpre[0] = a.take<float>(conv_ws_tmax_floats(N, h->S));
    b.tmax_dpre[1] = a.take<float>(conv_ws_tmax_floats(N, h->S));
    const int ncopy = mode == 1 ? T + 1 : 1;
    auto per_iter = [&](std::vector<float*>& v, size_t n, int copies) {      // `copies` instances back to back, the rest alias [0]
        v.resize(T + 1);
        float* base = a.take<float>(n * (size_t)copies);
        for (int i = 0; i <= T; ++i) v[i] = (i < copies && base) ? base + (size_t)i * n : base;
    };
    per_iter(b.z, (size_t)N * L, ncopy);
    if (mode != 1) b.z[T] = a.take<float>((size_t)N * L);   // the final sample must not overwrite the last elbo()'s z (self.z)
    per_iter(b.g_pm, (size_t)N * L, ncopy);
    per_iter(b.g_plv, (size_t)N * L, ncopy);
    per_iter(b.latent, (size_t)N * 4 * L, ncopy);
    {
        // training keeps the refinement inputs of all T iterations, back to back: the conv stack of the refinement network is
        // back-propagated for all iterations in ONE batch of T * N slot-images (iodine_train_backward)
        const size_t n_enc = (size_t)N * P * 20;
        float* base = a.take<float>(n_enc * (mode == 1 ? T : 1));
        b.enc.resize(T + 1);
        for (int i = 0; i <= T; ++i) b.enc[i] = (mode == 1 && i < T) ? (base ? base + (size_t)i * n_enc : nullptr) : base;
        // split form (refine_split): the same memory as per-slot tensors [N][P][12] of all kept iterations back to back,
        // followed by the per-image tensors [B][P][8]
        const size_t n_k = (size_t)N * P * 12, n_s = (size_t)B * P * 8;
        const int keep = mode == 1 ? T : 1;
        b.enck.resize(T + 1); b.encs.resize(T + 1);
        for (int i = 0; i <= T; ++i) {
            const int j = (mode == 1 && i < T) ? i : 0;
            b.enck[i] = base ? base + (size_t)j * n_k : nullptr;
            b.encs[i] = base ? base + (size_t)keep * n_k + (size_t)j * n_s : nullptr;
        }
        b.rmap = a.take<float>((size_t)B * (h->S / 2) * (h->S / 2) * Cr);
    }
    per_iter(b.pooled, (size_t)N * Cr, ncopy);
    per_iter(b.u, (size_t)N * H, ncopy);
    per_iter(b.gates, (size_t)N * 4 * H, ncopy);
    per_iter(b.xin, (size_t)N * (H + 4 * L), ncopy);
    {   // gate GEMM of the refinement head (head_mfma): its input rows [u | latent | h_prev] and its output, rows padded to a multiple of 32
        const size_t Np = ((size_t)N + 31) / 32 * 32;
        b.head_xh = a.take<float>(Np * (size_t)(H + 4 * L + H));
        b.head_gp = a.take<float>(Np * (size_t)4 * H);
    }
    // LSTM state: h[i], c[i] = state BEFORE iteration i; inference ping-pongs two copies
    b.h.resize(T + 2); b.c.resize(T + 2);
    if (mode == 1) {
        // (each array contiguous over the iterations: the head's weight gradients are one GEMM over all T * N rows)
        float* hb = a.take<float>((size_t)(T + 2) * N * H);
        float* cb = a.take<float>((size_t)(T + 2) * N * H);
        for (int i = 0; i <= T + 1; ++i) { b.h[i] = hb ? hb + (size_t)i * N * H : nullptr; b.c[i] = cb ? cb + (size_t)i * N * H : nullptr; }
    } else {
        float* hh[2] = {a.take<float>((size_t)N * H), a.take<float>((size_t)N * H)};
        float* cc[2] = {a.take<float>((size_t)N * H), a.take<float>((size_t)N * H)};
        for (int i = 0; i <= T + 1; ++i) { b.h[i] = hh[i & 1]; b.c[i] = cc[i & 1]; }
    }
    b.ract.assign(T + 1, std::vector<float*>(h->Dr));
    {
        int s = h->S;
        for (int l = 0; l < h->Dr; ++l) {
            s = ref_out_size(h, s);
            const size_t n_l = (size_t)N * s * s * Cr;
            float* base = a.take<float>(n_l * (mode == 1 ? T : 1));         // [T][N][s][s][Cr] in training (see enc)
            for (int i = 0; i <= T; ++i) b.ract[i][l] = (mode == 1 && i < T) ? (base ? base + (size_t)i * n_l : nullptr) : base;
        }
    }
    if (mode != 0) {
        // what one weight-gradient pass of the decoder needs: training, and mode 2 = "decoder backward" (a single decode / elbo kept for
        // iodine_decode_backward / iodine_elbo_backward): the inference carve-up plus this block
        const int Cmax = Cd > Cr ? Cd : Cr;
        const size_t part_elems = (size_t)512 * 4 * 9 * 32 * 32 > (size_t)512 * 9 * Cmax * Cmax
                                      ? (size_t)512 * 4 * 9 * 32 * 32 : (size_t)512 * 9 * Cmax * Cmax;
        b.wg_part = a.take<float>(part_elems);
        b.wg_part_b = a.take<float>((size_t)512 * 64);
        b.wg_acc.assign(h->Dd, nullptr); b.wg_acc_b.assign(h->Dd, nullptr);
        if (h->opt.wgrad_accum && !gen_dec && mode == 1) {      // (a single pass has nothing to accumulate over: shared scratch)
            b.wg_acc[0] = a.take<float>((size_t)1024 * 2 * 9 * Cd * 4);       // dec_out_bwd_fused: <= 1024 blocks x KS <= 2 tiles of [9][Cd][4]
            b.wg_acc_b[0] = a.take<float>((size_t)1024 * 4);
            for (int l = 1; l < h->Dd; ++l) {
                b.wg_acc[l] = a.take<float>((size_t)512 * 4 * 9 * 32 * 32 > (size_t)512 * 9 * Cd * Cd ? (size_t)512 * 4 * 9 * 32 * 32 : (size_t)512 * 9 * Cd * Cd);
                b.wg_acc_b[l] = a.take<float>((size_t)512 * 64);
            }
        }
        b.wg_fold = a.take<float>((size_t)WGRAD_FOLD * 9 * Cmax * Cmax);
        b.Dsum = a.take<float>((size_t)P * Cd);
        b.Dpart = a.take<float>((size_t)l0_dgroups(N) * P * Cd);
        b.rown = a.take<float>((size_t)N * h->S * 4 * Cd);
        b.Rsum = a.take<float>((size_t)h->S * 4 * Cd);
        b.RT = a.take<float>((size_t)N * 9 * Cd);
        b.tmp_lz = a.take<float>((size_t)L * 9 * Cd);
    }
    if (mode == 1) {
        // ddm / ddv / dgates / ds: one instance per iteration (weight gradients of the head in one pass over all of them)
        b.ddm = a.take<float>((size_t)T * N * L); b.ddv = a.take<float>((size_t)T * N * L);
        b.dc1 = a.take<float>((size_t)N * H); b.dgates = a.take<float>((size_t)T * N * 4 * H);
        b.dxin = a.take<float>((size_t)N * H); b.ds = a.take<float>((size_t)T * N * H);
        b.dpooled = a.take<float>((size_t)T * N * Cr);                     // all iterations (batched conv-stack backward)
        for (int j = 0; j < 2; ++j) { b.carry_h[j] = a.take<float>((size_t)N * H); b.carry_c[j] = a.take<float>((size_t)N * H); }
        b.rdpre.resize(h->Dr);
        int s = h->S;
        for (int l = 0; l < h->Dr; ++l) { s = ref_out_size(h, s); b.rdpre[l] = a.take<float>((size_t)T * N * s * s * Cr); }
        b.aux_seed = a.take<float>((size_t)2 * (T + 1) * N * L);
    }
    if (gen_dec) {
        b.gen_l0 = a.take<float>(gen_l0_scratch_floats(N, h->S, Cd, h->kd));   // row / tap sums, prefix table of the broadcast layer
    }
    if ((gen_dec || gen_ref) && mode != 0) {
        size_t scr = 0;
        if (gen_dec) scr = std::max(gen_wgrad_scratch_floats(Cd, 4, h->kd), gen_wgrad_scratch_floats(Cd, Cd, h->kd));
        if (gen_ref && mode == 1) scr = std::max(scr, std::max(gen_wgrad_scratch_floats(17, Cr, h->kr), gen_wgrad_scratch_floats(Cr, Cr, h->kr)));
        b.gen_scr = a.take<float>(scr);
    }
    // option sigma_grad (at the end: the carve-up in front of it is the same with or without a reader of these two)
    b.sg_part = a.take<double>((size_t)B * pixel_blocks_per_image(P));
    b.sgrad = a.take<float>((size_t)T + 1);
    // option input_grad: carved only while a bit is set, behind everything else - with the option off the plan is what it was
    b.ig = h->opt.input_grad;
    b.ig_x = (b.ig & 1) ? a.take<float>((size_t)b.F * B * 3 * P) : nullptr;
    b.ig_w = (b.ig & 2) ? a.take<float>((size_t)b.F * B * P) : nullptr;
    b.bytes = (a.off + 255) & ~(size_t)255;
}

void drop_graphs(iodine_handle* h)
{
    for (auto& g : h->graphs) {
        if (g.exec) (void)hipGraphExecDestroy(g.exec);
        if (g.graph) (void)hipGraphDestroy(g.graph);
    }
    h->graphs.clear();
    h->seen_keys.clear();
}

int ensure_workspace(iodine_handle* h, int B, int mode)
{
    if (h->buf.B == B && h->buf.mode == mode && h->buf.K == h->K && h->buf.T == h->T && h->buf.F == (h->frames > 0 ? h->frames : 1) &&
        h->buf.ig == h->opt.input_grad && h->buf.bytes > 0)
        return IODINE_OK;
    Arena q(nullptr); Buffers tmp; plan(h, B, mode, q, tmp);
    void* base = nullptr;
    if (h->ws_user) {
        if (h->ws_user_bytes < tmp.bytes) {
            char m[200];
            snprintf(m, sizeof m, "workspace too small: need %zu bytes for batch %d mode %d at %d slots / %d iterations / %d frame(s), have %zu",
                     tmp.bytes, B, mode, h->K, h->T, tmp.F, h->ws_user_bytes);
            return h->fail(IODINE_ERR_WORKSPACE, m);
        }
        base = h->ws_user;
    } else {
        if (h->ws_own_bytes < tmp.bytes) {
            if (h->ws_own) { HIPCHK(h, hipFree(h->ws_own)); h->ws_own = nullptr; h->ws_own_bytes = 0; }
            HIPCHK(h, hipMalloc(&h->ws_own, tmp.bytes));
            h->ws_own_bytes = tmp.bytes;
        }
        base = h->ws_own;
    }
    Arena a(base);
    plan(h, B, mode, a, h->buf);
    h->calls.arena_gone();                                 // a re-planned arena no longer holds the saved forward / the last elbo() outputs
    // captured graphs stay: their key holds the arena's base address, the batch, the run shape and (through the entry point) the mode,
    // and the carve-up is a pure function of those - a step that alternates training and reconstruct calls keeps replaying both
    return IODINE_OK;
}

int check_ready(iodine_handle* h, int batch)
{
    if (!h) return IODINE_ERR_INVALID;
    if (!h->params_set) return h->fail(IODINE_ERR_STATE, "iodine_set_params has not been called");
    if (batch < 1) return h->fail(IODINE_ERR_INVALID, "batch must be >= 1");
    // several kernels index one activation tensor [N][P][C] with 32-bit element offsets
    const size_t cmax = (size_t)std::max(std::max(h->Cd, h->Cr), 20);
    if ((size_t)batch * h->K * h->P * cmax >= ((size_t)1 << 31))
        return h->fail(IODINE_ERR_INVALID, "batch too large for one device: batch * slots * pixels * channels must stay below 2^31 "
                                           "(shard the images over ranks, iodine_amd.parallel)");
    return IODINE_OK;
}

// o: the objective the body runs with - host scalars are baked into the captured nodes, so the key carries the bit patterns of sigma and
// beta and the generation of the weight table (the handle's current objective; a backward passes the one its forward saved)
// pw: the pixel weights of a call that packs x - the captured pack kernel bakes the pointer and the flag like every other address
std::vector<uintptr_t> graph_key(const iodine_handle* h, int entry, int batch, std::initializer_list<const void*> ptrs, const Objective* o,
                                 const PixelWeights* pw)
{
    if (!o) o = &h->obj;
    uint64_t sb, bb;
    memcpy(&sb, &o->sigma, 8); memcpy(&bb, &o->beta, 8);
    std::vector<uintptr_t> k = {(uintptr_t)entry, (uintptr_t)batch, (uintptr_t)h->K, (uintptr_t)h->T, (uintptr_t)h->opt.stop_after, (uintptr_t)h->opt.precision,
                                (uintptr_t)h->opt.variant, (uintptr_t)h->opt.fuse_l0, (uintptr_t)h->opt.out_bwd_fused, (uintptr_t)h->opt.refine_split, (uintptr_t)(h->opt.head_fused | (h->opt.refine_bwd_fused << 1) | (h->opt.refine_ws << 2) | (h->opt.refine_l0_fused << 3) | (h->opt.head_mfma << 4) | (h->opt.wgrad_accum << 5) | (h->opt.dec_out_rows << 6) | (h->opt.gen_precision << 7) | (h->opt.sigma_grad << 8) | (h->opt.stable_enc << 9) | (h->opt.input_grad << 10) | (h->opt.joint_ll << 12)),
                                (uintptr_t)(h->ws_user ? h->ws_user : h->ws_own), (uintptr_t)h->frames};
    k.push_back((uintptr_t)sb); k.push_back((uintptr_t)bb); k.push_back((uintptr_t)o->wgen);
    k.push_back((uintptr_t)(pw ? pw->w : nullptr)); k.push_back((uintptr_t)(pw ? pw->per_frame : 0));
    for (const void* p : ptrs) k.push_back((uintptr_t)p);
    return k;
}
