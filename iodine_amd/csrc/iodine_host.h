// What the host translation units of the compute handle share beyond the handle itself (iodine_internal.h includes this at its end):
// the workspace arena and the profiler bracket, the path selectors and launch sequences of iodine_dispatch.cpp, the planning layer of
// iodine_plan.cpp and the hipGraph runner.  Everything here is hidden: nothing of it is part of the library's dynamic symbol table.
#pragma once

#pragma GCC visibility push(hidden)

// bump allocator over a (possibly NULL = size query) base pointer
struct Arena {
    char* base;
    size_t off = 0;
    explicit Arena(void* b) : base((char*)b) {}
    template <typename T> T* take(size_t n) {
        off = (off + 255) & ~(size_t)255;
        T* p = base ? (T*)(base + off) : nullptr;
        off += n * sizeof(T);
        return p;
    }
};

// several small device-to-device copies, transposes [R][Cc] -> [Cc][R] and sums of two vectors, collected and issued as ONE launch
struct CopyBatch {
    hipStream_t st;
    MultiCopy mc;
    explicit CopyBatch(hipStream_t s) : st(s) { mc.count = 0; }
    hipError_t flush() { const hipError_t e = launch_multi_copy(st, mc); mc.count = 0; return e; }
    hipError_t copy(float* dst, const float* src, size_t count, int op = 0, int cols = 0, const float* src2 = nullptr) {
        if (mc.count == MCOPY_MAX) if (const hipError_t e = flush(); e != hipSuccess) return e;
        mc.src[mc.count] = src; mc.src2[mc.count] = src2; mc.dst[mc.count] = dst; mc.n[mc.count] = (int)count; mc.op[mc.count] = op;
        mc.cols[mc.count] = cols; ++mc.count;
        return hipSuccess;
    }
    hipError_t transpose(float* dst, const float* src, int R, int Cc) { return copy(dst, src, (size_t)R * Cc, 1, Cc); }
    hipError_t add2(float* dst, const float* a, const float* b2, int count) { return copy(dst, a, (size_t)count, 2, 0, b2); }
};

// bracket one launch expression with profiler events (no-op unless profiling is on)
#define PROF(h, st, cat, expr)                                                       \
    do {                                                                             \
        hipEvent_t e0_ = nullptr, e1_ = nullptr;                                     \
        ProfCat* pc_ = nullptr;                                                      \
        if ((h)->opt.profile > 1) { pc_ = (h)->prof_cat(cat); pc_->seen_win++; }         \
        else if ((h)->opt.profile == 1 && !strncmp(cat, "conv_tile_", 10)) {             \
            pc_ = (h)->prof_cat(cat);                                                \
            pc_->seen_win++;                                                         \
            if (pc_->seen++ % (unsigned long long)(h)->opt.profile_stride) pc_ = nullptr;    \
        }                                                                            \
        if (pc_) {                                                                   \
            if (pc_->used == pc_->ev.size()) {                                       \
                hipEvent_t a_, b_;                                                   \
                HIPCHK(h, hipEventCreate(&a_)); HIPCHK(h, hipEventCreate(&b_));      \
                pc_->ev.push_back({a_, b_});                                         \
            }                                                                        \
            e0_ = pc_->ev[pc_->used].first; e1_ = pc_->ev[pc_->used].second;         \
            pc_->used++;                                                             \
            HIPCHK(h, hipEventRecord(e0_, st));                                      \
        }                                                                            \
        HIPCHK(h, expr);                                                             \
        if (e1_) HIPCHK(h, hipEventRecord(e1_, st));                                 \
    } while (0)

// ---- iodine_dispatch.cpp: which kernels run and in what order

// Which kernels the decoder runs on.  Decided by dec_path and nowhere else: the launch sites, the packs iodine_set_params refreshes and the
// workspace plan all switch on it, so a weight pack that is read is a pack that was written.  A function, not a cached field: the options
// may change between calls (conv_precision / conv_variant invalidate the parameters, and the graph key holds both).
enum DecPath {
    DEC_GENERIC,      // kernels_generic.hip: KERNEL_SIZE other than 3, CONV_CHAN other than 32 / 64, sizes that are no multiple of 16
    DEC_WS_F16,       // split-fp16, weight-stationary persistent kernel (conv_variant 6, power-of-two image sizes >= 16)
    DEC_TILE_F16,     // split-fp16, LDS-tiled 16 x 16 tiles
    DEC_WS_F32,       // exact fp32 (conv_precision 0): the weight-stationary kernel's fp32 form (v_mfma_f32_16x16x4_f32, no tile scales / side buffers)
    DEC_TILE_F32,     // exact fp32, the round-1 LDS-tiled kernels
};
DecPath dec_path(const iodine_handle* h);
bool dec_f16(DecPath p);
int dec_ws_products(const iodine_handle* h);

// Which kernels the refinement conv stack runs on, decided the same way.  The family depends on the configuration and conv_precision only:
// iodine_set_params switches on it alone and keeps every pack of the family current - the per-form options do not invalidate the parameters.
enum RefFamily {
    REF_GENERIC,      // kernels_generic.hip: KERNEL_SIZE other than 3, CONV_CHAN other than 32 / 64, sizes that are no multiple of 16, stride != 2
    REF_S2_F16,       // the tuned stride-2 kernels, split fp16
    REF_S2_F32,       // the same kernels in their fp32-MFMA form (conv_precision 0): same buffers, fp32 weights in the same layouts
    REF_GATHER,       // the gather kernels: some layer has an odd input size, which the tuned kernels do not take
};
RefFamily ref_family(const iodine_handle* h);
bool ref_s2(RefFamily f);
bool ref_pack_ws(const iodine_handle* h);
bool ref_pack_bwd01(const iodine_handle* h);
bool ref_pack_l0f(const iodine_handle* h);
// The form of a forward pass: the family with the options and the kernels' own shape limits.  A pure function of the handle: it is evaluated
// inside graphed bodies, which a replay does not execute - what a later call needs of it (CallState) is stored outside of them.
// split: the channels every slot of an image shares are written and convolved once per image (split first layer); l0f: ... and encoding +
// layer 0 are one kernel, the encoding stays on chip unless a reader asks for it
struct RefForm { RefFamily fam; bool split, l0f; };
RefForm ref_form(const iodine_handle* h);
bool ref_layer_ws(const iodine_handle* h, const RefForm& f, int l, int s);
bool ref_bwd01(const iodine_handle* h, bool fwd_split);

// where one weight-gradient launch of a decoder pass leaves its partial tiles and when they are reduced.  Option wgrad_accum (round 5): a
// block's partial tile accumulates alpha_i x (pass i) in a per-layer buffer and is reduced once, after the last pass (it == T); otherwise
// the shared scratch, reduced with the pass factor straight away
struct WgradPass { float *part, *part_b; float alpha; int accum; float reduce_alpha; bool reduce; };

// the launch sequences the entry points are made of
int decoder_forward(iodine_handle* h, hipStream_t st, int N, const float* z, float* out = nullptr);
int decoder_backward_data(iodine_handle* h, hipStream_t st, int N, float** dpre0, bool train, float train_alpha, int it, bool single = false);
const float* x4_frame(const iodine_handle* h, int i);
int elbo_and_gradients(iodine_handle* h, hipStream_t st, int B, const float* eps_i, int i, bool need_grads,
                       bool train = false, float train_alpha = 0.f, bool sgrad = false, int igrad = 0, float ig_coef = 0.f);
int refine_stack_backward(iodine_handle* h, hipStream_t st, int NT, bool fwd_split);
int refine_step(iodine_handle* h, hipStream_t st, int B, int i, bool save);

// ---- iodine_plan.cpp: the parameter table, the workspace carve-up, what a call needs before it may launch

void build_param_table(iodine_handle* h);
int ref_out_size(const iodine_handle* h, int s);
void plan(const iodine_handle* h, int B, int mode, Arena& a, Buffers& b);
void drop_graphs(iodine_handle* h);
int ensure_workspace(iodine_handle* h, int B, int mode);
int check_ready(iodine_handle* h, int batch);

// first element of a graph key: the entry point (1, 4, 5: reconstruct, train forward, train backward)
enum { GK_DECODE = 2, GK_ELBO = 3, GK_DECODE_SAVED = 6, GK_ELBO_SAVED = 7, GK_DECODE_BWD = 8, GK_ELBO_BWD = 9 };
// (o, pw: see the definition)
std::vector<uintptr_t> graph_key(const iodine_handle* h, int entry, int batch, std::initializer_list<const void*> ptrs, const Objective* o = nullptr,
                                 const PixelWeights* pw = nullptr);

// Run `body` (a fixed-shape sequence of launches on `st`) eagerly, or - with option "graph" - through a hipGraph keyed by
// the full argument tuple: the first call with a tuple runs eagerly (it also performs the one-time hipFuncSetAttribute
// calls of the launchers), the second is captured + instantiated, later ones are a single hipGraphLaunch.  Host-side state
// changes must NOT live in `body` (a replay does not execute it).
template <typename F>
int run_graphed(iodine_handle* h, hipStream_t st, const std::vector<uintptr_t>& key, F&& body)
{
    if (!h->opt.graph || h->opt.profile) return body();
    if (!st) return h->fail(IODINE_ERR_INVALID, "option graph=1 needs a non-default stream (the legacy null stream cannot be captured)");
    for (auto& g : h->graphs)
        if (g.key == key) {
            g.used = ++h->graph_clock;
            HIPCHK(h, hipGraphLaunch(g.exec, st));
            ++h->graph_replays;
            return IODINE_OK;
        }
    bool seen = false;
    for (auto& k : h->seen_keys) if (k == key) { seen = true; break; }
    if (!seen) {
        if (h->seen_keys.size() >= 64) h->seen_keys.clear();
        h->seen_keys.push_back(key);
        return body();
    }
    HIPCHK(h, hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
    const int rc = body();
    hipGraph_t graph = nullptr;
    const hipError_t e = hipStreamEndCapture(st, &graph);
    if (rc) { if (graph) (void)hipGraphDestroy(graph); return rc; }
    if (e != hipSuccess) return h->fail(IODINE_ERR_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(e));
    GraphEntry ge;
    ge.key = key; ge.graph = graph;
    const hipError_t e2 = hipGraphInstantiate(&ge.exec, graph, nullptr, nullptr, 0);
    if (e2 != hipSuccess) { (void)hipGraphDestroy(graph); return h->fail(IODINE_ERR_HIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(e2)); }
    if (h->graphs.size() >= 8) {                           // least recently used out
        size_t lru = 0;
        for (size_t i = 1; i < h->graphs.size(); ++i) if (h->graphs[i].used < h->graphs[lru].used) lru = i;
        (void)hipGraphExecDestroy(h->graphs[lru].exec); (void)hipGraphDestroy(h->graphs[lru].graph);
        h->graphs.erase(h->graphs.begin() + lru);
    }
    ge.used = ++h->graph_clock;
    h->graphs.push_back(ge);
    ++h->graph_captures;
    HIPCHK(h, hipGraphLaunch(ge.exec, st));
    return IODINE_OK;
}

#pragma GCC visibility pop
