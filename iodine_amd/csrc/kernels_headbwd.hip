// Training-only kernels: backward of the refinement head - the pointwise LSTM / MLP pieces, the whole BPTT in one
// launch (head_bptt_kernel) or as a launch sequence, and the average-pool backward.
//
// The refinement network is back-propagated through time after the forward loop (its inputs are detached,
// lib/modeling/iodine.py:343; lambda is detached before the additive update, iodine.py:642-643).
#include "common.h"

// LSTM cell backward, pointwise part.  gates = post-activation (i, f, g, o); c1 = f*c0 + i*g; h1 = o*tanh(c1).
//   in : dc1 (from the update read-out), dh1 / dc1_carry (from the next iteration; may be NULL)
//   out: dgates (pre-activation gradients, [N][4H]), dc0 (carry to the previous iteration)
__global__ void lstm_bwd_pointwise_kernel(const float* __restrict__ gates, const float* __restrict__ c0,
                                          const float* __restrict__ c1, const float* __restrict__ dc1_read,
                                          const float* __restrict__ dh1, const float* __restrict__ dc1_carry,
                                          float* __restrict__ dgates, float* __restrict__ dc0, int N, int H)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= N * H) return;
    const int n = idx / H, j = idx % H;
    const float* g = gates + (size_t)n * 4 * H;
    const float gi = g[j], gf = g[H + j], gg = g[2 * H + j], go = g[3 * H + j];
    const float tc = tanhf(c1[idx]);
    const float dh = dh1 ? dh1[idx] : 0.f;
    float dc = dc1_read[idx] + (dc1_carry ? dc1_carry[idx] : 0.f);
    dc += dh * go * (1.f - tc * tc);
    float* dg = dgates + (size_t)n * 4 * H;
    dg[j] = dc * gg * gi * (1.f - gi);
    dg[H + j] = dc * c0[idx] * gf * (1.f - gf);
    dg[2 * H + j] = dc * gi * (1.f - gg * gg);
    dg[3 * H + j] = dh * tc * go * (1.f - go);
    dc0[idx] = dc * gf;
}

hipError_t launch_lstm_bwd_pointwise(hipStream_t st, const float* gates, const float* c0, const float* c1,
                                     const float* dc1_read, const float* dh1, const float* dc1_carry, float* dgates,
                                     float* dc0, int N, int H)
{
    IOD_XSKIP(64);
    hipLaunchKernelGGL(lstm_bwd_pointwise_kernel, dim3((N * H + 255) / 256), dim3(256), 0, st, gates, c0, c1, dc1_read,
                       dh1, dc1_carry, dgates, dc0, N, H);
    return hipGetLastError();
}

// u = ELU(ELU(s)): ds = du * ELU'(y) * ELU'(s), y = ELU(s)     (iodine.py:485,565)
__global__ void mlp_bwd_pointwise_kernel(const float* __restrict__ du, int ldu, const float* __restrict__ s,
                                         float* __restrict__ ds, int N, int H)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= N * H) return;
    const int n = idx / H, j = idx % H;
    const float sv = s[idx];
    const float y = elu1(sv);
    const float g1 = sv > 0.f ? 1.f : y + 1.f;          // ELU'(s)
    const float g2 = y > 0.f ? 1.f : expf(y);           // ELU'(y)
    ds[idx] = du[(size_t)n * ldu + j] * g1 * g2;
}

hipError_t launch_mlp_bwd_pointwise(hipStream_t st, const float* du, int ldu, const float* s, float* ds, int N, int H)
{
    IOD_XSKIP(64);
    hipLaunchKernelGGL(mlp_bwd_pointwise_kernel, dim3((N * H + 255) / 256), dim3(256), 0, st, du, ldu, s, ds, N, H);
    return hipGetLastError();
}

// =========================================================================================
// Back-propagation through time of the refinement HEAD (read-out layers, LSTM cell, double-ELU MLP, average pool) for all T
// iterations in ONE launch.  Every row (slot) of the head is independent of the others - only the weight gradients sum over
// rows, and those stay separate GEMMs over all T * N rows - so a block takes HB rows and walks i = T-1 .. 0 itself:
//   ddm, ddv = alpha_i * d(B ELBO_{i+1}) / d lambda_{i+1}          (lambda_{i+1} = detach(lambda_i) + delta_i, iodine.py:642-643)
//   dc1  = ddm . Wm + ddv . Wv                                      (read-out from the CELL state, iodine.py:488-492)
//   dgates, dc0 = LSTM cell backward (+ the carries dh, dc of iteration i + 1)
//   dh0  = dgates . Whh        (carry)         dxin = dgates . Wih[:, :H]
//   ds   = dxin * ELU'(ELU(s)) * ELU'(s)       dpooled = ds . Wmlp
// It replaces 9 launches per iteration (2 scale, 4 + 1 SGEMM, 2 pointwise: 45 launches, ~0.45 ms per cfg3 step - each of them
// tens of microseconds of latency for a few MFLOP) by one.  The row vectors sit in LDS, a weight element is read once per block and used
// for all HB rows; the k loop is bound by that L2 stream, so the sixteen waves of a block split it and load 16 bytes per lane (head_matvec).
// SEED (iodine_train_backward_aux): the ELBO seeds are multiplied by *gl_dev (autograd's d(out) / d(loss), device memory; NULL = 0) and
// the first step, i = T - 1, adds seed_m / seed_v [N][L] = the cotangents that reach delta_{T-1} through lambda_T - unscaled by alpha and
// by *gl_dev.  SEED = false is the kernel as it was.
// seed_stride (floats) != 0: seed_m / seed_v are [T][N][L], one slice per iteration, and EVERY step i adds slice i = the cotangents that reach
// delta_i through lambda_{i+1} (iodine_train_backward_frames: auxiliary terms on chosen evaluations); 0: the one slice of step T - 1 above.
// The seeded instance also takes the carries across the ends of the saved forward (iodine_train_backward_seq), each pointer optional and
// tested once outside the iteration loop: dh_in / dc_in [N][H] = cotangents on the LSTM state (h_T, c_T) after the last update - they take
// the place of the zero carries iteration T - 1 starts from; dh_out / dc_out [N][H] receive the carries left after iteration 0 =
// d / d (h_0, c_0), the initial LSTM state (rows of the tail block beyond N are not written, as everywhere in this kernel).
// =========================================================================================
constexpr int HB = 2;      // rows per block
constexpr int HKG = 16;    // k groups = waves of the 1024-thread block; a lane owns four adjacent output columns (16-byte weight loads)

// vout[w][r][j] = sum_k vin[r][k] * W[w][k * ldw[w] + j]   for r < HB, j < J (J, ldw multiples of 4); vin / vout / s_part in LDS.
// The loop streams the weights once per block from L2 and is bound by that stream: wave g sums the k range of group g for the
// column quads lane, lane + 64, ... in ascending k with eight 16-byte loads in flight; the HKG partial sums are added in group order.
template <int NW>
IOD_DEVINL void head_matvec(const float* const (&W)[NW], const int (&ldw)[NW], int K, int J, const float* __restrict__ vin, int ldv,
                            float* const (&vout)[NW], int ldo, float* __restrict__ s_part)
{
    const int lane = threadIdx.x & 63, kg = threadIdx.x >> 6;
    const int kq = (K + HKG - 1) / HKG, k0 = kg * kq, k1 = min(K, k0 + kq);
    for (int jb = 0; jb < J; jb += 256) {
        const int j = jb + 4 * lane;
        f32x4 acc[NW][HB];
#pragma unroll
        for (int w = 0; w < NW; ++w)
#pragma unroll
            for (int r = 0; r < HB; ++r) acc[w][r] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (j < J) {
            int k = k0;
            for (; k + 7 < k1; k += 8) {
                f32x4 wv[NW][8];
#pragma unroll
                for (int w = 0; w < NW; ++w)
#pragma unroll
                    for (int u = 0; u < 8; ++u) wv[w][u] = *reinterpret_cast<const f32x4*>(W[w] + (size_t)(k + u) * ldw[w] + j);
#pragma unroll
                for (int u = 0; u < 8; ++u)
#pragma unroll
                    for (int r = 0; r < HB; ++r) {
                        const float x = vin[r * ldv + k + u];
#pragma unroll
                        for (int w = 0; w < NW; ++w) acc[w][r] += x * wv[w][u];
                    }
            }
            for (; k < k1; ++k)
#pragma unroll
                for (int r = 0; r < HB; ++r) {
                    const float x = vin[r * ldv + k];
#pragma unroll
                    for (int w = 0; w < NW; ++w) acc[w][r] += x * *reinterpret_cast<const f32x4*>(W[w] + (size_t)k * ldw[w] + j);
                }
#pragma unroll
            for (int w = 0; w < NW; ++w)
#pragma unroll
                for (int r = 0; r < HB; ++r) *reinterpret_cast<f32x4*>(s_part + ((kg * NW + w) * HB + r) * 256 + 4 * lane) = acc[w][r];
        }
        __syncthreads();
        // fixed-order sum over the k groups
        const int ncol = min(256, J - jb);
        for (int o = threadIdx.x; o < NW * HB * ncol; o += blockDim.x) {
            const int c = o % ncol, wr = o / ncol;
            float sum = s_part[(0 * NW * HB + wr) * 256 + c];
#pragma unroll
            for (int g = 1; g < HKG; ++g) sum += s_part[(g * NW * HB + wr) * 256 + c];
            vout[wr / HB][(wr % HB) * ldo + jb + c] = sum;
        }
        __syncthreads();
    }
}

template <bool SEED>
__global__ __launch_bounds__(1024)
void head_bptt_kernel(const float* __restrict__ g_pm, const float* __restrict__ g_plv, const float* __restrict__ gates,
                      const float* __restrict__ cst, const float* __restrict__ u, const float* __restrict__ Wm,
                      const float* __restrict__ Wv, const float* __restrict__ Whh, const float* __restrict__ Wih,
                      const float* __restrict__ Wmlp, float* __restrict__ ddm_o, float* __restrict__ ddv_o,
                      float* __restrict__ dgates_o, float* __restrict__ ds_o, float* __restrict__ dpooled_o, int T, int N, int B,
                      int L, int H, int Cr, const float* __restrict__ seed_m, const float* __restrict__ seed_v,
                      const float* __restrict__ gl_dev, const float* __restrict__ wtab, const float* __restrict__ dh_in,
                      const float* __restrict__ dc_in, float* __restrict__ dh_out, float* __restrict__ dc_out, size_t seed_stride)
{
    // wtab: the objective's table of T + 1 loss weights (one uniform 4-byte load per iteration), NULL = the default (i + 1) / (T + 1)
    extern __shared__ __attribute__((aligned(16))) float s_hb[];
    float* s_dd = s_hb;                              // [HB][2L]   ddm | ddv
    float* s_dc1 = s_dd + HB * 2 * L;                // [HB][H]    (two halves summed: see below)
    float* s_dc1b = s_dc1 + HB * H;                  // [HB][H]
    float* s_dg = s_dc1b + HB * H;                   // [HB][4H]
    float* s_dh = s_dg + HB * 4 * H;                 // [HB][H]    carry dh (from iteration i + 1)
    float* s_dcc = s_dh + HB * H;                    // [HB][H]    carry dc
    float* s_dx = s_dcc + HB * H;                    // [HB][H]    dxin, then ds
    float* s_dhn = s_dx + HB * H;                    // [HB][H]    new carry dh
    float* s_part = s_dhn + HB * H;                  // [HKG][2][HB][256] partial sums of head_matvec (16-byte aligned: all sizes are multiples of 4)
    const int tid = threadIdx.x, n0 = blockIdx.x * HB;
    const int IN = H + 4 * L;
    for (int idx = tid; idx < HB * H; idx += 1024) { s_dh[idx] = 0.f; s_dcc[idx] = 0.f; }
    if constexpr (SEED) {
        if (dh_in)
            for (int idx = tid; idx < HB * H; idx += 1024) s_dh[idx] = dh_in[(size_t)min(n0 + idx / H, N - 1) * H + idx % H];
        if (dc_in)
            for (int idx = tid; idx < HB * H; idx += 1024) s_dcc[idx] = dc_in[(size_t)min(n0 + idx / H, N - 1) * H + idx % H];
    }
    __syncthreads();
    float gl = 0.f;
    if constexpr (SEED) gl = gl_dev ? gl_dev[0] : 0.f;
    for (int i = T - 1; i >= 0; --i) {
        const float alpha = wtab ? -wtab[i + 1] / (float)B : -((float)(i + 2) / (float)(T + 1)) / (float)B;
        // 1. scaled posterior gradients of iteration i + 1
        for (int idx = tid; idx < HB * L; idx += 1024) {
            const int r = idx / L, l = idx % L, n = min(n0 + r, N - 1);
            float a = alpha * g_pm[((size_t)(i + 1) * N + n) * L + l], b = alpha * g_plv[((size_t)(i + 1) * N + n) * L + l];
            if constexpr (SEED) {
                a *= gl; b *= gl;
                if (seed_stride != 0 || i == T - 1) {
                    const size_t so = seed_stride * (size_t)i + (size_t)n * L + l;
                    a += seed_m[so]; b += seed_v[so];
                }
            }
            s_dd[r * 2 * L + l] = a; s_dd[r * 2 * L + L + l] = b;
            if (n0 + r < N) { ddm_o[((size_t)i * N + n) * L + l] = a; ddv_o[((size_t)i * N + n) * L + l] = b; }
        }
        __syncthreads();
        // 2. read-out layers: dc1 = ddm . Wm (+) ddv . Wv, the two products summed in that order like the two SGEMM calls it replaces
        {
            const float* const W0[1] = {Wm}; const float* const W1[1] = {Wv};
            const int ld0[1] = {H};
            float* const o0[1] = {s_dc1}; float* const o1[1] = {s_dc1b};
            head_matvec<1>(W0, ld0, L, H, s_dd, 2 * L, o0, H, s_part);
            head_matvec<1>(W1, ld0, L, H, s_dd + L, 2 * L, o1, H, s_part);
        }
        __syncthreads();
        // 3. LSTM cell backward (pointwise)
        for (int idx = tid; idx < HB * H; idx += 1024) {
            const int r = idx / H, j = idx % H, n = min(n0 + r, N - 1);
            const float* g = gates + ((size_t)i * N + n) * 4 * H;
            const float gi = g[j], gf = g[H + j], gg = g[2 * H + j], go = g[3 * H + j];
            const float c0v = cst[((size_t)i * N + n) * H + j], tc = tanhf(cst[((size_t)(i + 1) * N + n) * H + j]);
            const float dh = s_dh[idx];
            float dc = (s_dc1[idx] + s_dc1b[idx]) + s_dcc[idx];
            dc += dh * go * (1.f - tc * tc);
            const float d0 = dc * gg * gi * (1.f - gi), d1 = dc * c0v * gf * (1.f - gf), d2 = dc * gi * (1.f - gg * gg),
                        d3 = dh * tc * go * (1.f - go);
            float* sg = s_dg + r * 4 * H;
            sg[j] = d0; sg[H + j] = d1; sg[2 * H + j] = d2; sg[3 * H + j] = d3;
            if (n0 + r < N) {
                float* og = dgates_o + ((size_t)i * N + n) * 4 * H;
                og[j] = d0; og[H + j] = d1; og[2 * H + j] = d2; og[3 * H + j] = d3;
            }
            s_dcc[idx] = dc * gf;                                           // carry dc for iteration i - 1 (own element: no hazard)
        }
        __syncthreads();
        // 4. + 5. dh0 = dgates . Whh (carry), dxin = dgates . Wih[:, :H]: one pass over k for both
        {
            const float* const W[2] = {Whh, Wih};
            const int ld[2] = {H, IN};
            float* const out[2] = {s_dhn, s_dx};
            head_matvec<2>(W, ld, 4 * H, H, s_dg, 4 * H, out, H, s_part);
        }
        __syncthreads();
        // 6. double-ELU MLP backward (pointwise); the new dh carry moves into place
        for (int idx = tid; idx < HB * H; idx += 1024) {
            const int r = idx / H, j = idx % H, n = min(n0 + r, N - 1);
            const float sv = u[((size_t)i * N + n) * H + j];
            const float y = elu1(sv);
            const float g1 = sv > 0.f ? 1.f : y + 1.f, g2 = y > 0.f ? 1.f : expf(y);
            const float d = s_dx[idx] * g1 * g2;
            s_dx[idx] = d;
            if (n0 + r < N) ds_o[((size_t)i * N + n) * H + j] = d;
            s_dh[idx] = s_dhn[idx];
        }
        __syncthreads();
        // 7. average-pool input gradient: dpooled = ds . Wmlp  (written straight to global: s_dc1 is free, used as staging)
        {
            const float* const W[1] = {Wmlp};
            const int ld[1] = {Cr};
            float* const out[1] = {s_dc1};
            head_matvec<1>(W, ld, H, Cr, s_dx, H, out, H, s_part);
        }
        __syncthreads();
        for (int idx = tid; idx < HB * Cr; idx += 1024) {
            const int r = idx / Cr, c = idx % Cr;
            if (n0 + r < N) dpooled_o[((size_t)i * N + n0 + r) * Cr + c] = s_dc1[r * H + c];
        }
        __syncthreads();
    }
    if constexpr (SEED) {
        // the carries iteration 0 left (its last barrier is behind every write of s_dh / s_dcc)
        if (dh_out)
            for (int idx = tid; idx < HB * H; idx += 1024)
                if (n0 + idx / H < N) dh_out[(size_t)(n0 + idx / H) * H + idx % H] = s_dh[idx];
        if (dc_out)
            for (int idx = tid; idx < HB * H; idx += 1024)
                if (n0 + idx / H < N) dc_out[(size_t)(n0 + idx / H) * H + idx % H] = s_dcc[idx];
    }
}

// does the fused kernel's LDS footprint fit: 2 (2L + 10H) + 16384 floats <= 160 KB holds for every accepted width (151.5 KB at L = 256, H = 1024);
// what sends a configuration to the launch sequence is REF.CONV_CHAN > MLP_UNITS
static size_t head_bptt_lds(int L, int H) { return ((size_t)HB * (2 * L + 10 * H) + (size_t)HKG * 2 * HB * 256) * sizeof(float); }
// (head_matvec reads the weights as 16-byte f32x4 rows: every row length / leading dimension - H, H + 4L, Cr, L - must be a multiple of 4)
bool head_bptt_fits(int L, int H, int Cr) { return Cr <= H && H % 4 == 0 && Cr % 4 == 0 && L % 4 == 0 && head_bptt_lds(L, H) <= 160 * 1024; }

hipError_t launch_head_bptt(hipStream_t st, const float* g_pm, const float* g_plv, const float* gates, const float* cst, const float* u,
                            const float* Wm, const float* Wv, const float* Whh, const float* Wih, const float* Wmlp, float* ddm,
                            float* ddv, float* dgates, float* ds, float* dpooled, int T, int N, int B, int L, int H, int Cr,
                            const float* seed_m, const float* seed_v, const float* gl_dev, const float* wtab, const float* dh_in,
                            const float* dc_in, float* dh_out, float* dc_out, size_t seed_stride)
{
    IOD_XSKIP(2);
    if (Cr > H) return hipErrorInvalidValue;                                // (the pool gradient is staged in an [HB][H] buffer)
    if ((seed_m == nullptr) != (seed_v == nullptr)) return hipErrorInvalidValue;
    if (!seed_m && (dh_in || dc_in || dh_out || dc_out || seed_stride)) return hipErrorInvalidValue;   // (the carries across the ends: the seeded instance only)
    const size_t lds = head_bptt_lds(L, H);
    if (lds > 160 * 1024) return hipErrorInvalidValue;
    const dim3 grid((N + HB - 1) / HB), block(64 * HKG);
    if (seed_m)                                                             // auxiliary cotangents: the seeded instance
        return iod_launch<head_bptt_kernel<true>>(st, grid, block, lds, 160 * 1024, g_pm, g_plv, gates, cst, u, Wm, Wv, Whh, Wih, Wmlp, ddm, ddv, dgates, ds,
                                                  dpooled, T, N, B, L, H, Cr, seed_m, seed_v, gl_dev, wtab, dh_in, dc_in, dh_out, dc_out, seed_stride);
    return iod_launch<head_bptt_kernel<false>>(st, grid, block, lds, 160 * 1024, g_pm, g_plv, gates, cst, u, Wm, Wv, Whh, Wih, Wmlp, ddm, ddv, dgates, ds,
                                               dpooled, T, N, B, L, H, Cr, nullptr, nullptr, nullptr, wtab, nullptr, nullptr, nullptr, nullptr, (size_t)0);
}

// The same recurrence as a launch sequence: per iteration 2 scale (+ 2 seed adds), 5 SGEMMs and the two pointwise kernels; what runs when
// head_bptt_fits says no (REF.CONV_CHAN > MLP_UNITS) or option head_fused is 0.  Arguments as launch_head_bptt, except: whost = the loss
// weights as a HOST table (NULL = default), seeded = the aux backward (gl_dev scales the ELBO seeds, seed_m / seed_v may be NULL), and the
// scratch dc1, dxin, carry_h[2], carry_c[2], each [N][H].  The per-iteration tensors lie back to back as in the fused kernel.
hipError_t launch_head_bptt_unfused(hipStream_t st, const float* g_pm, const float* g_plv, const float* gates, const float* cst, const float* u,
                                    const float* Wm, const float* Wv, const float* Whh, const float* Wih, const float* Wmlp, float* ddm_all,
                                    float* ddv_all, float* dgates_all, float* ds_all, float* dpooled_all, int T, int N, int B, int L, int H, int Cr,
                                    int seeded, const float* seed_m, const float* seed_v, const float* gl_dev, const float* whost,
                                    const float* dh_in, const float* dc_in, float* dh_out, float* dc_out, size_t seed_stride,
                                    float* dc1, float* dxin, float* const carry_h[2], float* const carry_c[2])
{
#define HBU(call) do { if (hipError_t e_ = (call); e_ != hipSuccess) return e_; } while (0)
    const int IN = H + 4 * L;
    int cf = 0;                                            // carry buffer flip
    for (int i = T - 1; i >= 0; --i) {
        // d loss / d delta_i = -w_{i+1}/B * d(B*ELBO_{i+1})/d lambda_{i+1}   (lambda_{i+1} = detach(lambda_i) + delta_i)
        const float alpha = whost ? -whost[i + 1] / (float)B : -((float)(i + 2) / (float)(T + 1)) / (float)B;
        float *ddm = ddm_all + (size_t)i * N * L, *ddv = ddv_all + (size_t)i * N * L;
        float *dgates = dgates_all + (size_t)i * N * 4 * H, *ds = ds_all + (size_t)i * N * H;
        HBU(launch_scale(st, g_pm + (size_t)(i + 1) * N * L, alpha, ddm, N * L));
        HBU(launch_scale(st, g_plv + (size_t)(i + 1) * N * L, alpha, ddv, N * L));
        if (seeded) {                                      // ELBO seeds x d(out) / d(loss); lambda_T's cotangents join delta_{T-1} unscaled
            // (cotangents on chosen evaluations: those of lambda_{i+1} join delta_i, every i)
            const float *sm = seed_stride ? seed_m + (size_t)i * seed_stride : i == T - 1 ? seed_m : nullptr;
            const float *sv = seed_stride ? seed_v + (size_t)i * seed_stride : i == T - 1 ? seed_v : nullptr;
            HBU(launch_scale_dev_add(st, ddm, gl_dev, sm, N * L));
            HBU(launch_scale_dev_add(st, ddv, gl_dev, sv, N * L));
        }
        const float *c0 = cst + (size_t)i * N * H, *c1 = cst + (size_t)(i + 1) * N * H;
        // read-out layers act on the cell state (iodine.py:488-492)
        HBU(launch_sgemm(st, 0, 0, N, H, L, 1.f, ddm, L, Wm, H, 0.f, dc1, H));
        HBU(launch_sgemm(st, 0, 0, N, H, L, 1.f, ddv, L, Wv, H, 1.f, dc1, H));
        const bool last = (i == T - 1);
        HBU(launch_lstm_bwd_pointwise(st, gates + (size_t)i * N * 4 * H, c0, c1, dc1, last ? dh_in : carry_h[cf],
                                      last ? dc_in : carry_c[cf], dgates, carry_c[cf ^ 1], N, H));
        HBU(launch_sgemm(st, 0, 0, N, H, 4 * H, 1.f, dgates, 4 * H, Whh, H, 0.f, carry_h[cf ^ 1], H));
        cf ^= 1;
        // MLP (double ELU) and average pool
        HBU(launch_sgemm(st, 0, 0, N, H, 4 * H, 1.f, dgates, 4 * H, Wih, IN, 0.f, dxin, H));
        HBU(launch_mlp_bwd_pointwise(st, dxin, H, u + (size_t)i * N * H, ds, N, H));
        HBU(launch_sgemm(st, 0, 0, N, Cr, H, 1.f, ds, H, Wmlp, Cr, 0.f, dpooled_all + (size_t)i * N * Cr, Cr));
    }
    if (dh_out) HBU(hipMemcpyAsync(dh_out, carry_h[cf], sizeof(float) * (size_t)N * H, hipMemcpyDeviceToDevice, st));
    if (dc_out) HBU(hipMemcpyAsync(dc_out, carry_c[cf], sizeof(float) * (size_t)N * H, hipMemcpyDeviceToDevice, st));
#undef HBU
    return hipSuccess;
}

// avg-pool backward fused with the ELU derivative of the last refinement conv layer
__global__ void pool_bwd_kernel(const float* __restrict__ dpooled, const float* __restrict__ act, float* __restrict__ dpre,
                                int PL, int C, size_t total)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int c = i % C;
    const size_t n = i / ((size_t)PL * C);
    dpre[i] = dpooled[n * C + c] / (float)PL * elu1_grad_from_out(act[i]);
}

hipError_t launch_pool_bwd(hipStream_t st, const float* dpooled, const float* act, float* dpre, int N, int PL, int C)
{
    IOD_XSKIP(64);
    const size_t total = (size_t)N * PL * C;
    hipLaunchKernelGGL(pool_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, dpooled, act, dpre, PL, C,
                       total);
    return hipGetLastError();
}
