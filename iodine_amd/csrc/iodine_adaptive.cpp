// Adaptive refinement (include/iodine_hip.h): iodine_reconstruct_adaptive - rounds of the reconstruct loop on a batch that shrinks as
// images converge - and the two stateless device steps between its rounds, iodine_adaptive_select / iodine_adaptive_move
// (kernels_adaptive.hip).  Nothing here changes another entry point: a round is the loop body of iodine_reconstruct_seq
// (elbo_and_gradients + refine_step, iodine_dispatch.cpp) at batch n_active on the first n_active rows of the workspace.
//
// Second buffers.  A parallel in-place compaction would read rows other blocks have overwritten, so every buffer whose rows move has a
// twin (AdaptiveScratch, one device block owned by the handle, grown on demand): the continuing rows are gathered into the twin and the
// two pointers of h->buf change places for the rounds that follow; the LSTM state, which the loop ping-pongs between two buffers, rotates
// through three.  h->buf is put back as planned when the call returns, whichever way it returns.
#include "iodine_internal.h"

namespace {

const char* rule_bad(const iodine_adaptive_ctl* c)
{
    return !c ? "ctl is NULL" : c->max_iters < 1 ? "max_iters must be >= 1"
        : (c->min_iters < 1 || c->min_iters > c->max_iters) ? "min_iters must be in 1..max_iters" : c->check_every < 1 ? "check_every must be >= 1"
        : std::isnan(c->tol) ? "tol is NaN" : !(c->rtol >= 0.0) ? "rtol must be >= 0" : nullptr;
}

AdaptiveRule make_rule(const iodine_adaptive_ctl* c, double beta)
{
    return AdaptiveRule{c->max_iters, c->min_iters, c->check_every, c->tol, c->rtol, beta};
}

// the device block behind the second buffers, carved for one call
struct Twins {
    float *pm, *plv, *h, *c, *x4, *eps;
    int *idx[2], *pos, *stop_idx, *stop_pos, *counts;
    size_t bytes;
    Twins(void* base, size_t B, size_t K, size_t L, size_t H, size_t P, size_t R)
    {
        Arena a(base);
        pm = a.take<float>(B * K * L); plv = a.take<float>(B * K * L);
        h = a.take<float>(B * K * H); c = a.take<float>(B * K * H);
        x4 = a.take<float>(B * P * 4);
        eps = a.take<float>(R * B * K * L);
        idx[0] = a.take<int>(B); idx[1] = a.take<int>(B);
        pos = a.take<int>(B); stop_idx = a.take<int>(B); stop_pos = a.take<int>(B);
        counts = a.take<int>(4);
        bytes = (a.off + 255) & ~(size_t)255;
    }
};

int adaptive_scratch(iodine_handle* h, size_t bytes)
{
    AdaptiveScratch& s = h->adapt;
    if (!s.counts_host) HIPCHK(h, hipHostMalloc((void**)&s.counts_host, 4 * sizeof(int), hipHostMallocDefault));
    if (s.bytes >= bytes) return IODINE_OK;
    void* fresh = nullptr;
    HIPCHK(h, hipMalloc(&fresh, bytes));
    if (s.dev) (void)hipFree(s.dev);                       // (like ensure_workspace's own arena: hipFree waits for the work queued on it)
    s.dev = fresh; s.bytes = bytes;
    return IODINE_OK;
}

// h->buf as planned, back in place when the call leaves
struct PlannedBuffers {
    iodine_handle* h; Buffers planned;
    explicit PlannedBuffers(iodine_handle* hh) : h(hh), planned(hh->buf) {}
    ~PlannedBuffers() { h->buf = std::move(planned); }
};

// a table of moves issued ADAPTIVE_MOVE_MAX entries per launch
struct MoveBatch {
    iodine_handle* h; hipStream_t st;
    MoveEntry e[ADAPTIVE_MOVE_MAX]; int count = 0;
    MoveBatch(iodine_handle* hh, hipStream_t s) : h(hh), st(s) {}
    int flush()
    {
        if (count == 0) return IODINE_OK;
        PROF(h, st, "adaptive_move", launch_adaptive_move(st, e, count));
        count = 0;
        return IODINE_OK;
    }
    int add(const float* src, float* dst, size_t row_floats, const int* si, const int* di, int rows, int src_rows, int dst_rows)
    {
        if (count == ADAPTIVE_MOVE_MAX) if (int r = flush()) return r;
        e[count++] = MoveEntry{src, dst, (long long)row_floats, si, di, rows, src_rows, dst_rows, 0};
        return IODINE_OK;
    }
};

}  // namespace

int adaptive_check(iodine_handle* h, int batch, const float* x, const float* eps, const iodine_adaptive_ctl* ctl, const float* const* state_in,
                   const void* post_mean, const void* post_logvar, const void* lstm_h, const void* lstm_c, const void* iters, const void* ll,
                   const void* kl)
{
    if (const char* bad = rule_bad(ctl)) return h->fail(IODINE_ERR_INVALID, std::string("iodine_reconstruct_adaptive: ") + bad);
    if (state_in && !(state_in[0] && state_in[1] && state_in[2] && state_in[3]))
        return h->fail(IODINE_ERR_INVALID, "iodine_reconstruct_adaptive: an initial state needs all four tensors - post_mean, post_logvar (B,K,L) "
                                           "and the LSTM state h, c (B,K,MLP_UNITS)");
    if (h->frames > 0)
        return h->fail(IODINE_ERR_INVALID, "iodine_reconstruct_adaptive: clips are not taken (the frames setting must be 0: one image per batch entry)");
    if (h->opt.stop_after >= 0)
        return h->fail(IODINE_ERR_INVALID, "iodine_reconstruct_adaptive: not available with option stop_after_iters");
    if (h->T != ctl->check_every) {
        char m[200];
        snprintf(m, sizeof m, "iodine_reconstruct_adaptive: the run shape's iterations (%d) must equal check_every (%d): a round is one pass over "
                              "the per-iteration slots (iodine_set_run_shape)", h->T, ctl->check_every);
        return h->fail(IODINE_ERR_INVALID, m);
    }
    if (int rc = check_ready(h, batch)) return rc;
    if (!x || !eps) return h->fail(IODINE_ERR_INVALID, "iodine_reconstruct_adaptive: x and eps are required");
    if (!post_mean || !post_logvar || !lstm_h || !lstm_c || !iters || !ll || !kl)
        return h->fail(IODINE_ERR_INVALID, "iodine_reconstruct_adaptive: post_mean, post_logvar, lstm_h, lstm_c, iters, ll and kl are required "
                                           "(the stopped rows are written there between the rounds)");
    return IODINE_OK;
}

extern "C" {

int iodine_adaptive_select(void* stream, const float* terms, const int* idx_in, int n, int rounds, int t, int batch,
                           const iodine_adaptive_ctl* ctl, double beta, const int* budget_or_null, int* idx_out, int* pos_out,
                           int* stop_idx, int* stop_pos, int* counts, int* iters, float* ll, float* kl)
{
    const char* bad = rule_bad(ctl);
    if (!bad)
        bad = !terms ? "terms is NULL" : !idx_out ? "idx_out is NULL" : !pos_out ? "pos_out is NULL" : !stop_idx ? "stop_idx is NULL"
            : !stop_pos ? "stop_pos is NULL" : !counts ? "counts is NULL" : !iters ? "iters is NULL" : !ll ? "ll is NULL" : !kl ? "kl is NULL"
            : n < 1 ? "n must be >= 1" : n > batch ? "n must be <= batch" : (rounds < 1 || rounds > t) ? "rounds must be in 1..t"
            : t > ctl->max_iters ? "t must be <= max_iters" : std::isnan(beta) ? "beta is NaN"
            : idx_out == idx_in ? "idx_out must not be idx_in (the compaction is not in place)" : nullptr;
    if (bad) return free_fail(IODINE_ERR_INVALID, std::string("iodine_adaptive_select: ") + bad);
    return free_hip("iodine_adaptive_select", launch_adaptive_select((hipStream_t)stream, terms, idx_in, n, rounds, t, batch, make_rule(ctl, beta),
                                                                     budget_or_null, idx_out, pos_out, stop_idx, stop_pos, counts, iters, ll, kl));
}

int iodine_adaptive_move(void* stream, const iodine_move_entry* table, int n_entries)
{
    if (!table) return free_fail(IODINE_ERR_INVALID, "iodine_adaptive_move: table is NULL");
    if (n_entries < 1 || n_entries > ADAPTIVE_MOVE_MAX) return free_fail(IODINE_ERR_INVALID, "iodine_adaptive_move: n_entries must be in 1..16");
    MoveEntry e[ADAPTIVE_MOVE_MAX];
    for (int i = 0; i < n_entries; ++i) {
        const iodine_move_entry& q = table[i];
        const int sr = q.src_rows ? q.src_rows : q.rows, dr = q.dst_rows ? q.dst_rows : q.rows;
        const char* bad = !q.src ? "src is NULL" : !q.dst ? "dst is NULL" : q.row_floats < 1 ? "row_floats must be >= 1" : q.rows < 1 ? "rows must be >= 1"
            : (sr < 1 || (!q.src_index && sr < q.rows)) ? "src_rows must be >= rows where there is no src_index"
            : (dr < 1 || (!q.dst_index && dr < q.rows)) ? "dst_rows must be >= rows where there is no dst_index" : nullptr;
        if (!bad) {
            const uintptr_t s0 = (uintptr_t)q.src, s1 = s0 + (uintptr_t)sr * (uintptr_t)q.row_floats * sizeof(float);
            const uintptr_t d0 = (uintptr_t)q.dst, d1 = d0 + (uintptr_t)dr * (uintptr_t)q.row_floats * sizeof(float);
            if (s0 < d1 && d0 < s1) bad = "source and destination rows overlap (a parallel move is not in place: use a second buffer)";
        }
        if (bad) {
            char m[256];
            snprintf(m, sizeof m, "iodine_adaptive_move: entry %d: %s", i, bad);
            return free_fail(IODINE_ERR_INVALID, m);
        }
        e[i] = MoveEntry{q.src, q.dst, q.row_floats, q.src_index, q.dst_index, q.rows, sr, dr, 0};
    }
    return free_hip("iodine_adaptive_move", launch_adaptive_move((hipStream_t)stream, e, n_entries));
}

int iodine_reconstruct_adaptive(iodine_handle* h, void* stream, int batch, const float* x, const float* eps, const iodine_adaptive_ctl* ctl,
                                const int* budget_or_null, const float* const* state_in, float* pred, float* mask, float* mean, float* z,
                                float* post_mean, float* post_logvar, float* lstm_h, float* lstm_c, int* iters, float* ll, float* kl,
                                int* active_out_or_null)
{
    if (!h) return IODINE_ERR_INVALID;
    if (h->shim)
        return pad_reconstruct_adaptive(h, stream, batch, x, eps, ctl, budget_or_null, state_in, pred, mask, mean, z, post_mean, post_logvar, lstm_h,
                                        lstm_c, iters, ll, kl, active_out_or_null);
    const PixelWeights pw(h);                              // one-shot: taken before the first refusal
    int rc = adaptive_check(h, batch, x, eps, ctl, state_in, post_mean, post_logvar, lstm_h, lstm_c, iters, ll, kl);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    HIPCHK(h, hipStreamIsCapturing(st, &cap));
    if (cap != hipStreamCaptureStatusNone)
        return h->fail(IODINE_ERR_STATE, "iodine_reconstruct_adaptive: the stream is being captured - the call reads two counts back after every "
                                         "round and cannot be part of a hipGraph");
    rc = ensure_workspace(h, batch, 0);
    if (rc) return rc;
    const int B = batch, K = h->K, L = h->L, H = h->H, R = ctl->check_every, M = ctl->max_iters, N = B * K;
    const size_t rowL = (size_t)K * L, rowH = (size_t)K * H, rowX = (size_t)h->P * 4;
    rc = adaptive_scratch(h, Twins(nullptr, B, K, L, H, h->P, R).bytes);
    if (rc) return rc;
    Twins tw(h->adapt.dev, B, K, L, H, h->P, R);
    int* const counts_host = h->adapt.counts_host;
    // the arena is re-used, and afterwards it holds no evaluation of the whole batch: the iodine_last_* readers refuse
    h->calls.compute_begins();
    h->calls.last_elbo_iter = -1;
    h->calls.enc_valid = false;
    const int n_rounds = (M + R - 1) / R;
    if (active_out_or_null) for (int r = 0; r < n_rounds; ++r) active_out_or_null[r] = 0;
    const AdaptiveRule rule = make_rule(ctl, h->obj.beta);

    PlannedBuffers planned(h);
    Buffers& b = h->buf;
    PROF(h, st, "frames_in", launch_x_to_nhwc4(st, x, b.x4, B, h->P, 1, pw.w, 0));
    if (state_in) {
        HIPCHK(h, hipMemcpyAsync(b.pm, state_in[0], sizeof(float) * N * L, hipMemcpyDeviceToDevice, st));
        HIPCHK(h, hipMemcpyAsync(b.plv, state_in[1], sizeof(float) * N * L, hipMemcpyDeviceToDevice, st));
        HIPCHK(h, hipMemcpyAsync(b.h[0], state_in[2], sizeof(float) * N * H, hipMemcpyDeviceToDevice, st));
        HIPCHK(h, hipMemcpyAsync(b.c[0], state_in[3], sizeof(float) * N * H, hipMemcpyDeviceToDevice, st));
    } else
        HIPCHK(h, launch_posterior_init(st, h->head.init_mean, h->head.init_logvar, b.pm, b.plv, b.h[0], b.c[0], N, L, H));
    // the traces read NaN wherever no evaluation ran (all bits set is a quiet NaN)
    HIPCHK(h, hipMemsetAsync(ll, 0xFF, sizeof(float) * (size_t)M * B, st));
    HIPCHK(h, hipMemsetAsync(kl, 0xFF, sizeof(float) * (size_t)M * B, st));

    // the LSTM state rotates through three buffers: b.h[even i] = hp[even], b.h[odd i] = hp[odd] (the loop's ping-pong), one is free
    float* hp[3] = {b.h[0], b.h[1], tw.h};
    float* cp[3] = {b.c[0], b.c[1], tw.c};
    int even = 0, odd = 1;
    auto point_state = [&]() {
        for (size_t i = 0; i < b.h.size(); ++i) { b.h[i] = hp[(i & 1) ? odd : even]; b.c[i] = cp[(i & 1) ? odd : even]; }
    };
    float *pm_twin = tw.pm, *plv_twin = tw.plv, *x4_twin = tw.x4;
    const int* idx_cur = nullptr;                          // original indices of the active rows (NULL: nothing has moved yet)
    int flip = 0;
    bool packed = false;                                   // the round's noise rows were gathered into tw.eps (else: the caller's, in place)
    int n = B, t = 0;
    MoveBatch mv(h, st);
    for (int round = 0; n > 0 && t < M; ++round) {
        const int Rr = std::min(R, M - t);
        const float* eps_r = packed ? tw.eps : eps + (size_t)t * B * rowL;
        const size_t eps_stride = (size_t)(packed ? n : B) * rowL;
        if (active_out_or_null) active_out_or_null[round] = n;
        for (int i = 0; i < Rr; ++i) {                     // the loop body of iodine_reconstruct_seq at batch n
            if (int r = elbo_and_gradients(h, st, n, eps_r + (size_t)i * eps_stride, i, true)) return r;
            if (int r = refine_step(h, st, n, i, false)) return r;
        }
        t += Rr;
        int* idx_next = tw.idx[flip];
        PROF(h, st, "adaptive_select", launch_adaptive_select(st, b.img_terms, idx_cur, n, Rr, t, B, rule, budget_or_null, idx_next, tw.pos, tw.stop_idx,
                                                              tw.stop_pos, tw.counts, iters, ll, kl));
        HIPCHK(h, hipMemcpyAsync(counts_host, tw.counts, 2 * sizeof(int), hipMemcpyDeviceToHost, st));
        HIPCHK(h, hipStreamSynchronize(st));
        const int n_cont = counts_host[0], n_stop = counts_host[1];
        if (n_cont < 0 || n_stop < 0 || n_cont + n_stop != n || (t >= M && n_cont != 0))
            return h->fail(IODINE_ERR_HIP, "iodine_reconstruct_adaptive: the select step returned inconsistent counts");
        const int cur = (Rr & 1) ? odd : even;             // b.h[Rr] / b.c[Rr]: the state after the round
        if (n_stop > 0) {                                  // stopped rows: straight to the caller's tensors at their original index
            if (int r = mv.add(b.pm, post_mean, rowL, tw.stop_pos, tw.stop_idx, n_stop, n, B)) return r;
            if (int r = mv.add(b.plv, post_logvar, rowL, tw.stop_pos, tw.stop_idx, n_stop, n, B)) return r;
            if (int r = mv.add(hp[cur], lstm_h, rowH, tw.stop_pos, tw.stop_idx, n_stop, n, B)) return r;
            if (int r = mv.add(cp[cur], lstm_c, rowH, tw.stop_pos, tw.stop_idx, n_stop, n, B)) return r;
        }
        if (n_cont > 0) {
            if (n_stop > 0) {                              // continuing rows: to the front of the twins, which take the buffers' places
                const int to = (cur + 1) % 3, other = (cur + 2) % 3;
                if (int r = mv.add(b.pm, pm_twin, rowL, tw.pos, nullptr, n_cont, n, n_cont)) return r;
                if (int r = mv.add(b.plv, plv_twin, rowL, tw.pos, nullptr, n_cont, n, n_cont)) return r;
                if (int r = mv.add(hp[cur], hp[to], rowH, tw.pos, nullptr, n_cont, n, n_cont)) return r;
                if (int r = mv.add(cp[cur], cp[to], rowH, tw.pos, nullptr, n_cont, n, n_cont)) return r;
                if (int r = mv.add(b.x4, x4_twin, rowX, tw.pos, nullptr, n_cont, n, n_cont)) return r;
                std::swap(b.pm, pm_twin); std::swap(b.plv, plv_twin); std::swap(b.x4, x4_twin);
                even = to; odd = other;
                idx_cur = idx_next; flip ^= 1;
                packed = true;
            } else if (cur != even)
                std::swap(even, odd);                      // nothing moved: the next round starts where this one ended
            point_state();
            if (packed) {                                  // the next round's noise rows of the images still active, by original index
                const int Rn = std::min(R, M - t);
                for (int i = 0; i < Rn; ++i)
                    if (int r = mv.add(eps + (size_t)(t + i) * B * rowL, tw.eps + (size_t)i * n_cont * rowL, rowL, idx_cur, nullptr, n_cont, B, n_cont)) return r;
            }
        }
        if (int r = mv.flush()) return r;
        n = n_cont;
    }
    // z = posterior.sample(); decode(z) over the whole batch, from the posteriors the rounds left in the caller's tensors (iodine.py:103,110)
    HIPCHK(h, launch_dec_v(st, post_mean, post_logvar, eps + (size_t)M * B * rowL, nullptr, h->dec.wcls, b.z[h->T], b.V, N, L, h->Cd));
    if (int r = decoder_forward(h, st, N, b.z[h->T], b.g)) return r;
    if (pred || mask || mean) HIPCHK(h, launch_final_out(st, b.g, pred, mask, mean, nullptr, B, K, h->P));
    if (z) HIPCHK(h, hipMemcpyAsync(z, b.z[h->T], sizeof(float) * N * L, hipMemcpyDeviceToDevice, st));
    return IODINE_OK;
}

}  // extern "C"
