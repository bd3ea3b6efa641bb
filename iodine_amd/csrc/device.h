// Device-side helpers shared by every kernel file of libiodine_hip.so (gfx950 only): vector types, ELU / sigmoid, the one- or
// four-float load (vec_load), the butterfly wave sum / minimum / maximum of the stateless kernels (wave_sum, wave_min, wave_max), the
// DPP wave maximum, the split-fp16 scale and split helpers, the compile-time loop, the raw-buffer descriptor and the phase-timing
// macros.  A helper that two kernel files need lives here, once; common.h (host side: launchers, geometry) includes it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include <utility>

#define IOD_DEVINL __device__ __forceinline__

// ---- native vector types (MFMA operands, inline-asm operands), one name per type ----------------
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>) as straight-line code: the index is a constant
// expression inside f (literal offsets, named registers)
template <class F, int... Is>
IOD_DEVINL void static_for_impl(F&& f, std::integer_sequence<int, Is...>) { (f(std::integral_constant<int, Is>{}), ...); }
template <int N, class F>
IOD_DEVINL void static_for(F&& f) { static_for_impl(f, std::make_integer_sequence<int, N>{}); }

// raw dword buffer descriptor (gfx9 / CDNA: stride 0, no swizzle) over `bytes` bytes at `base`, in SGPRs: loads and stores
// past the end return 0 / are dropped in hardware
IOD_DEVINL i32x4 iod_make_rsrc(const void* base, unsigned bytes)
{
    const unsigned long long p = (unsigned long long)base;
    i32x4 r;
    r.x = __builtin_amdgcn_readfirstlane((int)(unsigned)p);
    r.y = __builtin_amdgcn_readfirstlane((int)(unsigned)(p >> 32));
    r.z = __builtin_amdgcn_readfirstlane((int)bytes);
    r.w = 0x00020000;
    return r;
}

// ELU with alpha = 1 (torch.nn.functional.elu): x > 0 ? x : expm1(x)
IOD_DEVINL float elu1(float v) { return v > 0.f ? v : expm1f(v); }
// the same through v_exp_f32 (absolute error ~1e-7, as in the conv epilogues): the streaming kernels are otherwise VALU-bound on expm1f
IOD_DEVINL float elu1_fast(float v) { return v > 0.f ? v : __expf(v) - 1.f; }
// derivative of ELU expressed through its OUTPUT a = ELU(x): a > 0 ? 1 : a + 1
IOD_DEVINL float elu1_grad_from_out(float a) { return a > 0.f ? 1.f : a + 1.f; }
IOD_DEVINL float sigmoidf_(float v) { return 1.f / (1.f + expf(-v)); }

// v[0..W-1] = p[0..W-1]: one 16-byte load for W = 4 (p 16-byte aligned: the launcher decides), one float for W = 1
template <int W> IOD_DEVINL void vec_load(const float* __restrict__ p, float (&v)[W])
{
    if constexpr (W == 4) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
        v[0] = *p;
    }
}

// Sum / minimum / maximum over the 64 lanes of a wave in a fixed xor butterfly, valid in every lane: the form of the stateless kernels
// (objects, chains, match), whose fp64 sums are reproducible to the bit because the order is fixed.  Off the hot path, where the DPP
// form of wave_max_f32 below is used.
IOD_DEVINL double wave_sum(double v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
IOD_DEVINL unsigned wave_sum(unsigned v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += (unsigned)__shfl_xor((int)v, d, 64);
    return v;
}
IOD_DEVINL int wave_min(int v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = min(v, __shfl_xor(v, d, 64));
    return v;
}
IOD_DEVINL int wave_max(int v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = max(v, __shfl_xor(v, d, 64));
    return v;
}

// max over the 64 lanes of a wave, returned to every lane.  DPP steps inside the 16-lane rows, row broadcasts across
// them and one v_readlane - about a dozen VALU instructions; the __shfl_xor butterfly it replaces is six dependent
// ds_bpermute round trips (~100 cycles each), which sat on the staging path of every tile chunk.
IOD_DEVINL float wave_max_f32(float v)
{
    auto dpp = [](float x, auto ctrl, auto rmask) {
        const int r = __builtin_amdgcn_update_dpp(__float_as_int(x), __float_as_int(x), decltype(ctrl)::value,
                                                  decltype(rmask)::value, 0xf, false);
        return __int_as_float(r);
    };
    using std::integral_constant;
    v = fmaxf(v, dpp(v, integral_constant<int, 0xB1>{}, integral_constant<int, 0xf>{}));     // quad_perm [1,0,3,2]
    v = fmaxf(v, dpp(v, integral_constant<int, 0x4E>{}, integral_constant<int, 0xf>{}));     // quad_perm [2,3,0,1]
    v = fmaxf(v, dpp(v, integral_constant<int, 0x141>{}, integral_constant<int, 0xf>{}));    // row_half_mirror
    v = fmaxf(v, dpp(v, integral_constant<int, 0x140>{}, integral_constant<int, 0xf>{}));    // row_mirror: row max in all 16 lanes
    v = fmaxf(v, dpp(v, integral_constant<int, 0x142>{}, integral_constant<int, 0xa>{}));    // row_bcast:15 into rows 1, 3
    v = fmaxf(v, dpp(v, integral_constant<int, 0x143>{}, integral_constant<int, 0xc>{}));    // row_bcast:31 into rows 2, 3
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}

// phase-timing macros TP_DECL / TP_STAMP / TP_FLUSH (empty in the product library) and the host report
#include "tile_prof.h"

// ---- helpers of the split-fp16 kernels ------------------------------------------------
// out[e] = in[(e + r) & 3] with conditional moves only (a runtime-indexed vector would be demoted to scratch)
IOD_DEVINL float4 rot4(const float4 v, int r)
{
    const bool b0 = r & 1, b1 = r & 2;
    float4 t;
    t.x = b0 ? v.y : v.x; t.y = b0 ? v.z : v.y; t.z = b0 ? v.w : v.z; t.w = b0 ? v.x : v.w;
    float4 o;
    o.x = b1 ? t.z : t.x; o.y = b1 ? t.w : t.y; o.z = b1 ? t.x : t.z; o.w = b1 ? t.y : t.w;
    return o;
}

// (x0, x1) -> packed fp16 pairs hi, lo with x = hi + lo: hi = x rounded toward zero to fp16 (v_cvt_pkrtz: the 11 leading bits for the scaled
// range), lo = x - hi (exact in fp32; hipcc emits v_fma_mix_f32 with the fp16 hi as a source and folds the caller's power-of-two scale multiply
// into it), each pair packed by one v_cvt_pkrtz: 6 VALU instructions per pair where the mask-and-subtract form took 8 - every split site was
// instruction-issue-bound (one VALU instruction per 4 cycles and wave).  Same bits as the mask form except below the fp16 normal range, where
// lo now also carries what the conversion of hi dropped.
IOD_DEVINL unsigned pack_hi_lo(float x0, float x1, unsigned& lo_out)
{
    typedef __fp16 h2_ __attribute__((ext_vector_type(2)));
    const h2_ hi = __builtin_amdgcn_cvt_pkrtz(x0, x1);
    const h2_ lo = __builtin_amdgcn_cvt_pkrtz(x0 - (float)hi.x, x1 - (float)hi.y);
    unsigned uh;
    __builtin_memcpy(&uh, &hi, 4); __builtin_memcpy(&lo_out, &lo, 4);
    return uh;
}

// power-of-two scale that puts max |x| = mx into [2^12, 2^13) (a pure function of mx: results must not depend on which
// block processed which tile before)
IOD_DEVINL float fresh_scale(float mx)
{
    if (!(mx > 0.f) || !(mx < 3.0e38f)) return 1.f;
    const int e = (int)((__float_as_uint(mx) >> 23) & 0xffu) - 127;
    int se = 12 - e;
    se = se > 100 ? 100 : (se < -100 ? -100 : se);
    return __uint_as_float((unsigned)(127 + se) << 23);
}

// power-of-two scale for a tile with max |x| = mx, keeping the current one while mx*cur stays in [2^9, 2^14.5)
IOD_DEVINL float tile_scale(float mx, float cur)
{
    if (!(mx > 0.f) || !(mx < 3.0e38f)) return cur;
    const float t = mx * cur;
    if (t >= 512.f && t < 23170.f) return cur;
    return fresh_scale(mx);
}
