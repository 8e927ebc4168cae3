// adam.hip -- the dense Adam every model trains through (torch.optim.Adam's single-tensor path on ONE flat buffer):
//   K2   one launch per step (skr_adam_step)
//   K2b  temporally blocked: mark / cold pass / hot step (skr_adam_block_*), bit-identical to K2 after every step
//   K2w  both with torch.optim.Adam(weight_decay=...) (the *_wd entry points): the WD instantiations of the same kernels
// *_tf: tf.train.AdamOptimizer's placement of the second bias correction (adam_scalars).  The arithmetic is in adam_math.h,
// which the fused BPR step (bpr_fused.hip, K2c) shares.
#include "adam_math.h"

#include <climits>
#include <cstdio>
#include <cstdlib>

using namespace skr;

namespace {

// non-temporal 16-byte accesses (NT = false: plain ones)
template <bool NT>
__device__ __forceinline__ float4 ld4(const float4* q) {
    if (NT) {
        float4 r;
        r.x = __builtin_nontemporal_load(&q->x); r.y = __builtin_nontemporal_load(&q->y);
        r.z = __builtin_nontemporal_load(&q->z); r.w = __builtin_nontemporal_load(&q->w);
        return r;
    }
    return *q;
}
template <bool NT>
__device__ __forceinline__ void st4(float4* q, const float4& r) {
    if (NT) {
        __builtin_nontemporal_store(r.x, &q->x); __builtin_nontemporal_store(r.y, &q->y);
        __builtin_nontemporal_store(r.z, &q->z); __builtin_nontemporal_store(r.w, &q->w);
    } else {
        *q = r;
    }
}

// WD: torch.optim.Adam(weight_decay=wd).  The gradient becomes g' = fmaf(wd, p, g), ONE rounding (torch's
// grad.add(param, alpha=weight_decay)), written identically in the three kernels, then adam_elem.  A block without a
// gradient still moves (g' = wd * p of the current p), so the cold pass and the hot step's catch-up run the full update in
// registers; the only shortcut is for elements whose p, m and v are all +0 (padded columns, padding rows, filler
// between tables), which the arithmetic leaves exactly as they are when eps > 0: g' = +0, m = +0, v = +0,
// p + (nss * 0) / eps = p.  The WD instantiations take adam_elem at every step: the scalar test for adam_elem_unit_bc2 costs
// the ALU-bound cold pass 7 % before step ~16 600 (2.93 against 2.73 ms per 32-step pass of 76.9 M parameters) and
// saves 15 % after it (profiles/adam_unify_timing.json): which of the two matters is a question of how long a run is.
template <bool WD>
__device__ __forceinline__ float grad_wd(float g, float p, float wd) { return WD ? fmaf(wd, p, g) : g; }

// ------------------------------------------------------------------------------------------------
// K2: dense Adam (torch.optim.Adam single-tensor path), 16-byte vectors, grid-stride
// ------------------------------------------------------------------------------------------------
template <bool TOUCH, int UNROLL, bool NT, bool WD>
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                                   float* __restrict__ v, int64_t n, AdamArgs a, float wd, int zero_grad,
                                                   uint8_t* __restrict__ touch) {
    const int64_t n4 = n >> 2;
    float4* p4 = reinterpret_cast<float4*>(p);
    float4* g4 = reinterpret_cast<float4*>(g);
    float4* m4 = reinterpret_cast<float4*>(m);
    float4* v4 = reinterpret_cast<float4*>(v);
    const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    // WD has ONE instantiation (TOUCH = true) and tests the pointer at run time: with touch == NULL that form is the faster
    // one (0.453 against 0.474 ms for the TOUCH = false instantiation on 76.9 M parameters, profiles/adam_unify_timing.json)
    const bool use_touch = TOUCH && (!WD || touch != nullptr);
    for (int64_t i0 = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; i0 < n4; i0 += stride * UNROLL) {
        float4 pp[UNROLL], mm[UNROLL], vv[UNROLL], gg[UNROLL];
        uint8_t flag[UNROLL];
#pragma unroll
        for (int k = 0; k < UNROLL; ++k) {   // issue every load of this trip before the first use
            const int64_t i = i0 + k * stride;
            gg[k] = zero4;
            flag[k] = 0;
            if (i < n4) {
                pp[k] = ld4<NT>(&p4[i]);
                mm[k] = ld4<NT>(&m4[i]);
                vv[k] = ld4<NT>(&v4[i]);
                // 16 consecutive lanes share one 64-float block and its byte; they all read it in this
                // instruction, before the lane with (i & 15) == 0 clears it further down
                flag[k] = use_touch ? touch[i >> 4] : 2;
                if (flag[k]) gg[k] = g4[i];
            }
        }
#pragma unroll
        for (int k = 0; k < UNROLL; ++k) {
            const int64_t i = i0 + k * stride;
            if (i < n4) {
                adam_elem(pp[k].x, grad_wd<WD>(gg[k].x, pp[k].x, wd), mm[k].x, vv[k].x, a);
                adam_elem(pp[k].y, grad_wd<WD>(gg[k].y, pp[k].y, wd), mm[k].y, vv[k].y, a);
                adam_elem(pp[k].z, grad_wd<WD>(gg[k].z, pp[k].z, wd), mm[k].z, vv[k].z, a);
                adam_elem(pp[k].w, grad_wd<WD>(gg[k].w, pp[k].w, wd), mm[k].w, vv[k].w, a);
                st4<NT>(&p4[i], pp[k]);
                st4<NT>(&m4[i], mm[k]);
                st4<NT>(&v4[i], vv[k]);
                if (flag[k]) {
                    if (zero_grad) g4[i] = zero4;
                    if (use_touch && flag[k] == 1 && (i & 15) == 0) touch[i >> 4] = 0;
                }
            }
        }
    }
    // tail (n not a multiple of 4): always read
    for (int64_t i = (n4 << 2) + blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; i < n; i += stride) {
        float pp = p[i], mm = m[i], vv = v[i];
        adam_elem(pp, grad_wd<WD>(g[i], pp, wd), mm, vv, a);
        p[i] = pp;
        m[i] = mm;
        v[i] = vv;
        if (zero_grad) g[i] = 0.f;
        if (use_touch && touch[i >> 6] == 1) touch[i >> 6] = 0;
    }
}

// ------------------------------------------------------------------------------------------------
// K2b: the same dense Adam, temporally blocked.  The reference's optimiser moves EVERY parameter at EVERY
// step, but a BPR step puts a non-zero gradient into at most 3*batch of the ~1.1 M rows, and the batches of an
// epoch are known in advance.  For a block of k consecutive steps the 64-float blocks of the flat buffer
// are split into HOT (touched by at least one of the k steps) and COLD.  A cold block sees k zero-gradient
// updates: they are applied in ONE pass (p, m, v read and written once instead of k times), each of the k
// updates evaluated exactly as adam_elem does with g = 0 and that step's bias corrections.  Hot blocks get
// the ordinary update at every step, through the id lists of the block (each block claimed once per step).
// Every parameter still receives every update, in the same arithmetic: results are bit-identical to calling
// skr_adam_step after every step (tests/test_gpu_train.py::test_blocked_adam_is_bit_identical).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void adam_mark_kernel(const int32_t* __restrict__ ids, int64_t n, int64_t offset,
                                                        int stride, int32_t* __restrict__ tag, int32_t value,
                                                        int32_t* __restrict__ claim, int32_t claim_value) {
    const int64_t g = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
    if (g < n && ids[g] >= 0) {   // negative id: an empty slot of a de-duplicated list
        const int64_t blk = (offset + static_cast<int64_t>(ids[g]) * stride) >> 6;
        tag[blk] = value;
        if (claim) claim[blk] = claim_value;
    }
}

// cold pass: every float4 whose 64-float block is not tagged gets k zero-gradient updates (WD: each with g' = wd * p of
// the current p)
template <int UNROLL, bool WD>
__global__ __launch_bounds__(256) void adam_cold_kernel(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v,
                                                        int64_t n, AdamBlockArgs a, float wd, const int32_t* __restrict__ tag,
                                                        int32_t hot_value) {
    const int64_t n4 = n >> 2;
    float4* p4 = reinterpret_cast<float4*>(p);
    float4* m4 = reinterpret_cast<float4*>(m);
    float4* v4 = reinterpret_cast<float4*>(v);
    const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
    const bool skip_zero = WD && a.eps > 0.0f;
    auto all_zero = [](const float4& x) { return (__float_as_uint(x.x) | __float_as_uint(x.y) | __float_as_uint(x.z) | __float_as_uint(x.w)) == 0; };
    auto steps = [&](float& pp, float& mm, float& vv) {
        for (int s = 0; s < a.k; ++s) {
            AdamArgs one{a.one_minus_b1, a.b2, a.one_minus_b2, a.neg_step_size[s], a.bc2_sqrt[s], a.eps};
            adam_elem(pp, grad_wd<WD>(0.0f, pp, wd), mm, vv, one);
        }
    };
    // the same k updates for the four lanes of a float4, step-major: the four independent chains of one step sit
    // next to each other, which lets the compiler pair them into packed fp32 instructions
    auto steps4 = [&](float4& pp, float4& mm, float4& vv) {
        for (int s = 0; s < a.k; ++s) {
            AdamArgs one{a.one_minus_b1, a.b2, a.one_minus_b2, a.neg_step_size[s], a.bc2_sqrt[s], a.eps};
            if (!WD && __builtin_amdgcn_readfirstlane(__float_as_int(one.bc2_sqrt)) == 0x3f800000) {   // scalar branch, not a select
                adam_elem_unit_bc2(pp.x, grad_wd<WD>(0.0f, pp.x, wd), mm.x, vv.x, one);
                adam_elem_unit_bc2(pp.y, grad_wd<WD>(0.0f, pp.y, wd), mm.y, vv.y, one);
                adam_elem_unit_bc2(pp.z, grad_wd<WD>(0.0f, pp.z, wd), mm.z, vv.z, one);
                adam_elem_unit_bc2(pp.w, grad_wd<WD>(0.0f, pp.w, wd), mm.w, vv.w, one);
            } else {
                adam_elem(pp.x, grad_wd<WD>(0.0f, pp.x, wd), mm.x, vv.x, one);
                adam_elem(pp.y, grad_wd<WD>(0.0f, pp.y, wd), mm.y, vv.y, one);
                adam_elem(pp.z, grad_wd<WD>(0.0f, pp.z, wd), mm.z, vv.z, one);
                adam_elem(pp.w, grad_wd<WD>(0.0f, pp.w, wd), mm.w, vv.w, one);
            }
        }
    };
    for (int64_t i0 = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; i0 < n4; i0 += stride * UNROLL) {
        float4 pp[UNROLL], mm[UNROLL], vv[UNROLL];
        bool cold[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const int64_t i = i0 + u * stride;
            cold[u] = i < n4 && tag[i >> 4] != hot_value;
            if (cold[u]) {
                pp[u] = ld4<true>(&p4[i]);
                mm[u] = ld4<true>(&m4[i]);
                vv[u] = ld4<true>(&v4[i]);
            }
        }
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            if (cold[u] && !(skip_zero && all_zero(pp[u]) && all_zero(mm[u]) && all_zero(vv[u]))) {
                const int64_t i = i0 + u * stride;
                steps4(pp[u], mm[u], vv[u]);
                st4<true>(&p4[i], pp[u]);
                st4<true>(&m4[i], mm[u]);
                st4<true>(&v4[i], vv[u]);
            }
        }
    }
    // tail (n not a multiple of 4)
    for (int64_t i = (n4 << 2) + blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; i < n; i += stride)
        if (tag[i >> 6] != hot_value) steps(p[i], m[i], v[i]);
}

__global__ __launch_bounds__(256) void selftest_cold_math_kernel(uint32_t lo, uint32_t hi, uint64_t n_pairs,
                                                                 unsigned long long* __restrict__ bad) {
    const uint64_t tid = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    const uint64_t nth = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    unsigned long long bs = 0, bd = 0, b1 = 0, b2 = 0;
    for (uint64_t b = lo + tid; b <= hi; b += nth) {
        const float x = __uint_as_float(static_cast<uint32_t>(b));
        const uint32_t want = __float_as_uint(sqrtf(x));
        bs += __float_as_uint(sqrt_ordinary(x)) != want;
        b1 += __float_as_uint(__builtin_amdgcn_sqrtf(x)) != want;   // control
        b2 += 1;
    }
    for (uint64_t i = tid; i < n_pairs; i += nth) {
        uint64_t h = (i + 1) * 0x9E3779B97F4A7C15ull;   // splitmix64
        h = (h ^ (h >> 30)) * 0xBF58476D1CE4E5B9ull;
        h = (h ^ (h >> 27)) * 0x94D049BB133111EBull;
        h ^= h >> 31;
        // d: exponent in [-48, 21], n: exponent in [-100, 40], random mantissas and signs
        const uint32_t hd = static_cast<uint32_t>(h), hn = static_cast<uint32_t>(h >> 32);
        const uint32_t ed = 127 - 48 + (hd >> 23) % 70, en = 127 - 100 + ((hn >> 23) & 0xff) % 141;
        const float d = __uint_as_float((hd & 0x807fffffu) | (ed << 23)), n = __uint_as_float((hn & 0x807fffffu) | (en << 23));
        bd += __float_as_uint(div_ordinary(n, d)) != __float_as_uint(n / d);
    }
    if (bs) atomicAdd(&bad[0], bs);
    if (bd) atomicAdd(&bad[1], bd);
    if (b1) atomicAdd(&bad[2], b1);
    if (b2) atomicAdd(&bad[3], b2);
}

// skr_selftest_grad_math: the gradient update of the lazy rows (adam_grad_run) against adam_elem / adam_elem_unit_bc2, bits of
// p, m and v.  One wavefront per group of 64 hashed tuples of the ordinary ranges, all at the same step of the block.  Of
// every 16 groups, groups 3 and 7 are CONTROLS with lanes outside the ordinary ranges (3: untouched moments m = v = +0 and
// lanes at rest with |m| = 2^-95; 7: one lane with m = -0, a NaN p, v = +inf or a stalled denormal m), so the wavefront must
// take the general form -- and must still give the same bits.
__global__ __launch_bounds__(256) void selftest_grad_math_kernel(uint64_t n_groups, AdamBlockArgs a, int run_len,
                                                                 unsigned long long* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const uint64_t n_waves = static_cast<uint64_t>(gridDim.x) * 4;
    unsigned long long bad = 0, fast = 0, ctl_general = 0, ctl_fast = 0, tested = 0;
    for (uint64_t gi = static_cast<uint64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6); gi < n_groups; gi += n_waves) {
        auto mix = [](uint64_t h) {      // splitmix64
            h *= 0x9E3779B97F4A7C15ull;
            h = (h ^ (h >> 30)) * 0xBF58476D1CE4E5B9ull;
            h = (h ^ (h >> 27)) * 0x94D049BB133111EBull;
            return h ^ (h >> 31);
        };
        const uint64_t h1 = mix(2 * (gi * 64 + lane) + 1), h2 = mix(2 * (gi * 64 + lane) + 2);
        const int s = static_cast<int>(mix(~gi) % static_cast<uint64_t>(a.k));
        auto make = [](uint32_t h, int e_lo, int e_n) {      // random sign and mantissa, exponent in [e_lo, e_lo + e_n)
            return __uint_as_float((h & 0x807fffffu) | ((127 + e_lo + (h >> 23 & 0xff) % e_n) << 23));
        };
        float p = make(static_cast<uint32_t>(h1), -20, 30), m = make(static_cast<uint32_t>(h1 >> 32), -40, 50);
        float v = fabsf(make(static_cast<uint32_t>(h2), -60, 70)), g = make(static_cast<uint32_t>(h2 >> 32), -30, 36);
        {   // no cancellation in m + c1 * (g - m) down to the bottom of the ordinary range: opposite signs only where |g| is far from 9 |m|
            const int de = static_cast<int>(__float_as_uint(g) >> 23 & 0xff) - static_cast<int>(__float_as_uint(m) >> 23 & 0xff);
            if (de >= 1 && de <= 5) g = copysignf(g, m);
        }
        const int kind = static_cast<int>(gi & 15);
        const bool control = kind == 7 || kind == 3;
        if (kind == 3) {
            if ((lane & 7) == 1) {           // null: untouched moments, g = +-0, any p without NaN (+-0 among them)
                m = 0.0f, v = 0.0f, g = (lane & 8) ? -0.0f : 0.0f;
                if (lane & 16) p = (lane & 32) ? -0.0f : 0.0f;
            } else if ((lane & 7) == 2) {    // at rest and below the ordinary range
                m = copysignf(0x1p-95f, m), g = (lane & 8) ? -0.0f : 0.0f;
                v = 0x1p-20f * (1.0f + 0x1p-3f * (lane >> 3));
                p = copysignf(fmaxf(fabsf(p), 0x1p-10f), p);
            }
        } else if (kind == 7 && lane == 5) {
            switch (static_cast<int>(gi >> 4 & 3)) {
                case 0: m = -0.0f, v = 0.0f, g = 0.0f, p = 0.0f; break;      // (beside an ordinary p, m = -0 is at rest)
                case 1: m = 0.0f, v = 0.0f, g = 0.0f, p = __uint_as_float(0x7fc00001u); break;
                case 2: v = __uint_as_float(0x7f800000u); break;
                default: m = __uint_as_float(0x00000123u), g = 0.0f, p = 0x1p-70f; break;
            }
        }
        // the gradient update and run_len - 1 zero-gradient updates behind it (as far as the block goes): the reference update
        // by update, the lazy rows' form in one call (the gradient's quotient is then the first of the side-by-side chains)
        const int s_to = s + run_len < a.k ? s + run_len : a.k;
        float wp = p, wm = m, wv = v;
        for (int q = s; q < s_to; ++q) {
            AdamArgs one{a.one_minus_b1, a.b2, a.one_minus_b2, a.neg_step_size[q], a.bc2_sqrt[q], a.eps};
            if (__builtin_amdgcn_readfirstlane(__float_as_int(one.bc2_sqrt)) == 0x3f800000)
                adam_elem_unit_bc2(wp, q == s ? g : 0.0f, wm, wv, one);
            else
                adam_elem(wp, q == s ? g : 0.0f, wm, wv, one);
        }
        const bool took_fast = adam_grad_run(p, g, m, v, a, s, s_to, FC_END);
        bad += (__float_as_uint(p) != __float_as_uint(wp)) || (__float_as_uint(m) != __float_as_uint(wm)) ||
               (__float_as_uint(v) != __float_as_uint(wv));
        tested += 1;
        if (lane == 0) {
            if (control) (took_fast ? ctl_fast : ctl_general) += 1;
            else fast += took_fast;
        }
    }
    if (tested) atomicAdd(&out[0], tested);
    if (bad) atomicAdd(&out[1], bad);
    if (fast) atomicAdd(&out[2], fast);
    if (ctl_general) atomicAdd(&out[3], ctl_general);
    if (ctl_fast) atomicAdd(&out[4], ctl_fast);
}

// skr_selftest_step_chain: the step kernel's catch-up on the lane tables (chain_advance, adam_math.h: the very function the
// kernel inlines) against adam_grad_run / adam_zero_run, bits of p, m and v.  The generator and the controls of
// selftest_grad_math_kernel; every wavefront at step s_from of the block: with_grad: the gradient update s_from and the
// zero-gradient updates behind it, otherwise the zero-gradient updates alone, up to s_from + run_len (as far as the block goes)
__global__ __launch_bounds__(256) void selftest_step_chain_kernel(uint64_t n_groups, AdamBlockArgs a, int s_from, int run_len,
                                                                  int with_grad, unsigned long long* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const uint64_t n_waves = static_cast<uint64_t>(gridDim.x) * 4;
    const AdamChainArgs ca = adam_chain_args(a);
    unsigned long long bad = 0, fast = 0, ctl_general = 0, ctl_fast = 0, tested = 0;
    for (uint64_t gi = static_cast<uint64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6); gi < n_groups; gi += n_waves) {
        auto mix = [](uint64_t h) {      // splitmix64
            h *= 0x9E3779B97F4A7C15ull;
            h = (h ^ (h >> 30)) * 0xBF58476D1CE4E5B9ull;
            h = (h ^ (h >> 27)) * 0x94D049BB133111EBull;
            return h ^ (h >> 31);
        };
        const uint64_t h1 = mix(2 * (gi * 64 + lane) + 1), h2 = mix(2 * (gi * 64 + lane) + 2);
        auto make = [](uint32_t h, int e_lo, int e_n) {      // random sign and mantissa, exponent in [e_lo, e_lo + e_n)
            return __uint_as_float((h & 0x807fffffu) | ((127 + e_lo + (h >> 23 & 0xff) % e_n) << 23));
        };
        float p = make(static_cast<uint32_t>(h1), -20, 30), m = make(static_cast<uint32_t>(h1 >> 32), -40, 50);
        float v = fabsf(make(static_cast<uint32_t>(h2), -60, 70)), g = make(static_cast<uint32_t>(h2 >> 32), -30, 36);
        {
            const int de = static_cast<int>(__float_as_uint(g) >> 23 & 0xff) - static_cast<int>(__float_as_uint(m) >> 23 & 0xff);
            if (de >= 1 && de <= 5) g = copysignf(g, m);
        }
        const int kind = static_cast<int>(gi & 15);
        const bool control = kind == 7 || kind == 3;
        if (kind == 3) {
            if ((lane & 7) == 1) {
                m = 0.0f, v = 0.0f, g = (lane & 8) ? -0.0f : 0.0f;
                if (lane & 16) p = (lane & 32) ? -0.0f : 0.0f;
            } else if ((lane & 7) == 2) {
                m = copysignf(0x1p-95f, m), g = (lane & 8) ? -0.0f : 0.0f;
                v = 0x1p-20f * (1.0f + 0x1p-3f * (lane >> 3));
                p = copysignf(fmaxf(fabsf(p), 0x1p-10f), p);
            }
        } else if (kind == 7 && lane == 5) {
            switch (static_cast<int>(gi >> 4 & 3)) {
                case 0: m = -0.0f, v = 0.0f, g = 0.0f, p = 0.0f; break;
                case 1: m = 0.0f, v = 0.0f, g = 0.0f, p = __uint_as_float(0x7fc00001u); break;
                case 2: v = __uint_as_float(0x7f800000u); break;
                default: m = __uint_as_float(0x00000123u), g = 0.0f, p = 0x1p-70f; break;
            }
        }
        const int s_to = s_from + run_len < a.k ? s_from + run_len : a.k;
        float wp = p, wm = m, wv = v;
        if (with_grad)
            adam_grad_run(wp, g, wm, wv, a, s_from, s_to, FC_END);
        else
            adam_zero_run(wp, wm, wv, a, s_from, s_to, FC_END);
        const AdamRowState r = chain_advance(p, g, m, v, with_grad ? s_from + 1 : 0, s_from, s_to, FC_END, ca);
        bad += (__float_as_uint(r.p) != __float_as_uint(wp)) || (__float_as_uint(r.m) != __float_as_uint(wm)) ||
               (__float_as_uint(r.v) != __float_as_uint(wv));
        tested += 1;
        if (lane == 0) {
            if (control) {
                ctl_fast += r.cls == FC_ORD;
                ctl_general += r.cls == FC_GENERAL;
            } else {
                fast += r.cls == FC_ORD;
            }
        }
    }
    if (tested) atomicAdd(&out[0], tested);
    if (bad) atomicAdd(&out[1], bad);
    if (fast) atomicAdd(&out[2], fast);
    if (ctl_general) atomicAdd(&out[3], ctl_general);
    if (ctl_fast) atomicAdd(&out[4], ctl_fast);
}

// cold pass, one wavefront per 64-float block (= one embedding row), with a cheap exact path for rows AT REST.
//
// A zero-gradient update is p += (nss*m') / (sqrt(v')/bc2 + eps) with m' = m + c1*(0 - m), v' = v*b2.  A row that
// no batch has touched for a few hundred steps has |m| decayed so far that the quotient q is below a quarter of
// the spacing of the floats around p: then fl(p + q) == p and the correctly rounded sqrt and divisions (about 36 of
// the ~41 issue slots of an update) decide nothing.  A block is AT REST for all k updates of the pass when every lane
// passes, on the values the pass starts from,
//     sign(v) = +, v not NaN;  |p| >= 2^-60;
//     |nss[0]*m| < 2^-28 * |p| * eps            or    |nss[0]*m|^2 < 2^-58 * p^2 * v * lb(b2^k)   (and that bound is normal)
// Proof sketch: |m| and |nss[s]| never grow over the pass and v never drops below v*b2^k, so for every
// update |n| = |fl(nss[s]*m')| <= |fl(nss[0]*m)| and d = fl(fl(sqrt(v')/bc2) + eps) >= max(eps, sqrt(v*b2^k))*(1 - 2^-22);
// hence |fl(n/d)| < 2^-27 |p| < spacing(p)/4 and p is unchanged, bit for bit, by each of the k updates.  m and v still get
// their k decays in the arithmetic of adam_elem (v*b2 + (c2*0)*0 == v*b2 because v*b2 carries a + sign).  The thresholds
// are zero (tests off) unless 0 < beta1, beta2 < 1, lr > 0, eps >= 0.  Blocks not at rest take adam_elem as before.
//
// REST (skr_adam_block_cold_rest): a word per row carries what an earlier pass established into the next one, so that a row
// whose answer is known is not read again to find it out.  word[b] = (pass_id << 2) | state, written by lane 0 for EVERY cold
// row of EVERY pass; a pass c trusts a word only when it carries c - 1 (a row that was hot in between was skipped by that
// pass: its word is stale and the row is examined from scratch -- nothing ever clears a word).  The caller promises for
// pass_id = previous + 1 that the rows the previous pass left cold have seen nothing but zero-gradient updates since, and
// that lr, betas and eps are the previous pass's and step_t0 is where it ended.  States:
//   1 QUIET  at the pass that read p every lane passed the sign / NaN test on v, |p| >= 2^-60 and the eps alternative
//            |nss[0]*m| < 2^-28 * |p| * eps.  That test stays true from pass to pass: p is fixed, |m| only decays (fl is
//            monotone: |fl(m + fl(c1 * -m))| <= |m|), torch's |nss| = lr / (1 - beta1^t) only shrinks with t, and v keeps
//            its sign.  So the pass would find the row at rest again -- without reading p: only m and v are loaded, decayed
//            and stored.  (The v alternative is NOT carried over: v decays, and with it the bound.)
//   2 ZERO   every lane of m and v is +0 (bits), and the row is quiet or (eps > 0 and no lane of p is NaN).  Then a
//            zero-gradient update is m = +0 + c1 * (+0 - +0) = +0, v = +0 * b2 + (c2 * 0) * 0 = +0, q = (nss * +0) / (+0 / bc2
//            + eps) = -0 / eps = -0 and p + (-0) = p for every p that is not NaN, +-0 and +-inf included: nothing changes,
//            nothing is loaded.  (|p| < 2^-60 is allowed here: the zero-initialised bias rows.)
// No state is set while the thresholds are off (rest_eps == 0: eps == 0, eps * 2^-28 underflows, or lr / betas out of range).
// The tail (n not a multiple of 64) has no word.  Census: stats[4] / stats[5] count the rows trusted as quiet / as zero.
__device__ __forceinline__ bool lane_quiet(float pp, float mm, float vv, const AdamBlockArgs& a) {   // lane_at_rest, eps alternative only
    const float ap = fabsf(pp), n0 = a.nss_bound[0] * fabsf(mm);
    return __float_as_uint(vv) <= 0x7f800000u && ap >= 0x1p-60f && n0 < ap * a.rest_eps;
}

// (at most 96 SGPRs, 8 wavefronts' worth per SIMD: the pass shares its CUs with the step and planning launches, whose workgroups
//  must find registers beside six workgroups of this kernel -- with the state words' scalars it would otherwise take 106)
template <int U, bool REST>
__global__ __launch_bounds__(256) __attribute__((amdgpu_num_sgpr(96))) void adam_cold_rows_kernel(float* __restrict__ p, float* __restrict__ m,
                                                             float* __restrict__ v, int64_t n, AdamBlockArgs a,
                                                             const int32_t* __restrict__ tag, int32_t hot_value,
                                                             int32_t* __restrict__ word, int32_t pass_id) {
    const int lane = threadIdx.x & 63;
    const int64_t nb = n >> 6;
    const int64_t n_waves = static_cast<int64_t>(gridDim.x) * 4;
    const int64_t wave0 = static_cast<int64_t>(blockIdx.x) * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    auto general = [&](float& pp, float& mm, float& vv) {
        for (int s = 0; s < a.k; ++s) {
            AdamArgs one{a.one_minus_b1, a.b2, a.one_minus_b2, a.neg_step_size[s], a.bc2_sqrt[s], a.eps};
            if (__builtin_amdgcn_readfirstlane(__float_as_int(one.bc2_sqrt)) == 0x3f800000)   // scalar branch, not a select
                adam_elem_unit_bc2(pp, 0.0f, mm, vv, one);
            else
                adam_elem(pp, 0.0f, mm, vv, one);
        }
    };
    // two rows of ordinary magnitudes advance together (packed fp32 for the element-wise parts, the two square
    // root / division chains interleaved): the first waits in `held` until the wavefront meets the second
    auto ordinary2 = [&](f32x2& p2, f32x2& m2, f32x2& v2) {
        for (int s = 0; s < a.k; ++s) {
            AdamArgs one{a.one_minus_b1, a.b2, a.one_minus_b2, a.neg_step_size[s], a.bc2_sqrt[s], a.eps};
            if (__builtin_amdgcn_readfirstlane(__float_as_int(one.bc2_sqrt)) == 0x3f800000)
                adam_pair_ordinary<true>(p2, m2, v2, one);
            else
                adam_pair_ordinary<false>(p2, m2, v2, one);
        }
    };
    bool have = false;
    float hp = 0.0f, hm = 0.0f, hv = 0.0f;
    int64_t hi = 0;
    for (int64_t b0 = wave0; b0 < nb; b0 += n_waves * U) {
        float pp[U], mm[U], vv[U];
        bool cold[U];
        int trust[U];      // REST: what the previous pass left in the row's word, if it is that pass's (0: nothing)
        // REST: lane u fetches row u's tag and word -- the U rows' tags and words in ONE round trip -- and the rows read them
        // from its registers; then only the loads a row's state needs
        int32_t tg_l = hot_value;
        uint32_t w_l = 0;
        if (REST && lane < U) {
            const int64_t b = b0 + lane * n_waves;
            if (b < nb) {
                tg_l = tag[b];
                w_l = static_cast<uint32_t>(word[b]);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t b = b0 + u * n_waves;
            trust[u] = 0;
            if (REST) {
                const int32_t tg = __builtin_amdgcn_readlane(tg_l, u);
                const uint32_t w = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int32_t>(w_l), u));
                cold[u] = tg != hot_value;
                if (cold[u] && a.rest_eps > 0.0f && (w >> 2) == static_cast<uint32_t>(pass_id - 1) && (w & 3u) != 3u)
                    trust[u] = static_cast<int>(w & 3u);
                pp[u] = 1.0f, mm[u] = 0.0f, vv[u] = 0.0f;
                if (cold[u]) {
                    const int64_t i = (b << 6) + lane;
                    if (trust[u] == 0) pp[u] = __builtin_nontemporal_load(&p[i]);
                    if (trust[u] != 2) {
                        mm[u] = __builtin_nontemporal_load(&m[i]);
                        vv[u] = __builtin_nontemporal_load(&v[i]);
                    }
                }
                continue;
            }
            cold[u] = b < nb && tag[b] != hot_value;
            if (cold[u]) {
                const int64_t i = (b << 6) + lane;
                pp[u] = __builtin_nontemporal_load(&p[i]);
                mm[u] = __builtin_nontemporal_load(&m[i]);
                vv[u] = __builtin_nontemporal_load(&v[i]);
            }
        }
        // rows at rest (4 of 5 cold rows): only the moments decay, 3 vector instructions per element and step -- as much
        // vector-ALU time over the pass as the rows of ordinary magnitudes.  Neighbours (u, u + 1) that are both at rest
        // decay together in packed fp32 (the same multiply and add on each half); a row whose moments are all zero
        // (never touched) has nothing to decay.
        bool rest[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (REST && trust[u] != 0) {
                // known to be at rest (a trusted ZERO row holds m = v = +0 here: nothing to decay, nothing to store)
                rest[u] = true;
                if (a.stats && lane == 0) atomicAdd(&a.stats[3 + trust[u]], 1ull);
            } else {
                rest[u] = cold[u] && __builtin_amdgcn_ballot_w64(!lane_at_rest(pp[u], mm[u], vv[u], a.nss_bound[0], a)) == 0;
            }
            if (REST && cold[u]) {
                // the row's state for the next pass, from the values this pass starts from (zero moments stay zero)
                int state = trust[u];
                if (state != 2 && a.rest_eps > 0.0f) {
                    const bool zero = __builtin_amdgcn_ballot_w64((__float_as_uint(mm[u]) | __float_as_uint(vv[u])) != 0) == 0;
                    if (state == 1) {
                        state = zero ? 2 : 1;
                    } else {
                        const bool quiet = __builtin_amdgcn_ballot_w64(!lane_quiet(pp[u], mm[u], vv[u], a)) == 0;
                        const bool p_ok = quiet || __builtin_amdgcn_ballot_w64(pp[u] != pp[u]) == 0;
                        state = (zero && p_ok) ? 2 : (quiet ? 1 : 0);
                    }
                }
                if (lane == 0) word[b0 + u * n_waves] = static_cast<int32_t>((static_cast<uint32_t>(pass_id) << 2) | static_cast<uint32_t>(state));
            }
        }
        auto store_rest = [&](int64_t i, float m0, float v0, float m1, float v1) {
            if (__builtin_amdgcn_ballot_w64(__float_as_uint(m1) != __float_as_uint(m0)) != 0) __builtin_nontemporal_store(m1, &m[i]);
            if (__builtin_amdgcn_ballot_w64(__float_as_uint(v1) != __float_as_uint(v0)) != 0) __builtin_nontemporal_store(v1, &v[i]);
        };
#pragma unroll
        for (int u = 0; u + 1 < U; u += 2) {
            if (!(rest[u] && rest[u + 1])) continue;
            if (a.stats && lane == 0) atomicAdd(&a.stats[0], 2ull);
            f32x2 m2{mm[u], mm[u + 1]}, v2{vv[u], vv[u + 1]};
            if (__builtin_amdgcn_ballot_w64((__float_as_uint(m2.x) | __float_as_uint(m2.y) | __float_as_uint(v2.x) |
                                             __float_as_uint(v2.y)) != 0) != 0) {
                for (int s = 0; s < a.k; ++s) {
                    // -m for (0 - m): a sign modifier on the multiply instead of an instruction.  They differ for m = +-0
                    // only (+0 vs -0 into the product), and m + (+-0) is m, resp. +0 for m = +-0, either way
                    m2 = m2 + a.one_minus_b1 * (-m2);
                    v2 = v2 * a.b2;
                }
                store_rest(((b0 + u * n_waves) << 6) + lane, mm[u], vv[u], m2.x, v2.x);
                store_rest(((b0 + (u + 1) * n_waves) << 6) + lane, mm[u + 1], vv[u + 1], m2.y, v2.y);
            }
            cold[u] = cold[u + 1] = false;      // done
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (!cold[u]) continue;
            const int64_t i = ((b0 + u * n_waves) << 6) + lane;
            if (rest[u]) {
                if (a.stats && lane == 0) atomicAdd(&a.stats[0], 1ull);
                if (REST && trust[u] == 2) continue;
                float m1 = mm[u], v1 = vv[u];
                for (int s = 0; s < a.k; ++s) {
                    m1 = m1 + a.one_minus_b1 * (0.0f - m1);
                    v1 = v1 * a.b2;
                }
                store_rest(i, mm[u], vv[u], m1, v1);
                continue;
            }
            const bool lane_ord = lane_ordinary(mm[u], vv[u], a);
            if (__builtin_amdgcn_ballot_w64(!lane_ord) == 0) {
                if (a.stats && lane == 0) atomicAdd(&a.stats[1], 1ull);
                if (!have) {
                    hp = pp[u], hm = mm[u], hv = vv[u], hi = i;
                    have = true;
                    continue;
                }
                f32x2 p2{hp, pp[u]}, m2{hm, mm[u]}, v2{hv, vv[u]};
                ordinary2(p2, m2, v2);
                __builtin_nontemporal_store(p2.x, &p[hi]);
                __builtin_nontemporal_store(m2.x, &m[hi]);
                __builtin_nontemporal_store(v2.x, &v[hi]);
                __builtin_nontemporal_store(p2.y, &p[i]);
                __builtin_nontemporal_store(m2.y, &m[i]);
                __builtin_nontemporal_store(v2.y, &v[i]);
                have = false;
                continue;
            }
            if (a.stats && lane == 0) atomicAdd(&a.stats[2], 1ull);
            general(pp[u], mm[u], vv[u]);
            __builtin_nontemporal_store(pp[u], &p[i]);
            __builtin_nontemporal_store(mm[u], &m[i]);
            __builtin_nontemporal_store(vv[u], &v[i]);
        }
    }
    if (have) {   // an odd one out
        general(hp, hm, hv);
        __builtin_nontemporal_store(hp, &p[hi]);
        __builtin_nontemporal_store(hm, &m[hi]);
        __builtin_nontemporal_store(hv, &v[hi]);
    }
    // tail (n not a multiple of 64)
    const int64_t i = (nb << 6) + blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
    if (i < n && tag[nb] != hot_value) general(p[i], m[i], v[i]);
}

// hot step: one wavefront per id.  claim[block] holds the optimiser step the block has been advanced to (the mark
// kernel sets it to the step count the k-step block starts from).  The wavefront that raises it to step_t owns the
// block for this launch and ADVANCES it: zero-gradient updates for the steps it has not seen yet, then step_t's update
// with the accumulated gradient, which is consumed.  A caller that names every hot block at every step gets one
// update per launch; a caller that names only the rows of batch t and of batch t+1 (the next batch must READ current
// rows) visits a row when it matters and catches up there -- the same updates in the same order, fewer passes over
// HBM.  The last step of a k-step block must name every hot block, so that all of them end at the same step.
template <bool WD>
__global__ __launch_bounds__(256) void adam_hot_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                                       float* __restrict__ v, int64_t n, AdamBlockArgs a, float wd, int32_t t0,
                                                       int32_t t, const int32_t* __restrict__ ids, int64_t n_ids,
                                                       int64_t offset, int stride, int32_t* __restrict__ claim) {
    const int lane = threadIdx.x & 63;
    const int64_t e = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (e >= n_ids) return;
    const int32_t id = ids[e];
    if (id < 0) return;                            // an empty slot of a de-duplicated list
    const int64_t blk = (offset + static_cast<int64_t>(id) * stride) >> 6;
    // the row is loaded while the claim is in flight (one memory round trip less on a latency-bound kernel); a
    // wavefront that loses the claim drops what it loaded.  Nobody writes the row during this launch but its owner.
    const int64_t i = blk * 64 + lane;
    float pp = 1.0f, mm = 0.0f, vv = 0.0f, gg = 0.0f;   // lanes beyond n: values that pass every wavefront-wide test
    if (i < n) {
        pp = p[i];
        mm = m[i];
        vv = v[i];
        gg = g[i];
    }
    int old = 0;
    if (lane == 0) old = atomicExch(&claim[blk], t);
    old = __builtin_amdgcn_readfirstlane(old);
    if (old >= t) return;
    if (old < t0) old = t0;
    // The steps the block is behind are zero-gradient updates, and they sit on the critical path of the training step
    // (the slowest wavefront of this launch is one with a row that is 20 steps behind).  The same three exact evaluations
    // as in the cold pass: AT REST (a row no batch has touched for long -- most user rows when their turn comes: only the
    // moments decay), ORDINARY MAGNITUDES (scaling-free square root / division: a dependent chain 2.5x shorter), general.
    // The first two hold for a zero gradient only: under weight decay (g' = wd * p) every step takes the general one.
    const int s_grad = t - t0 - 1;                 // the step that takes the gradient
    int s = old - t0;
    if (!WD && s < s_grad) {
        if (__builtin_amdgcn_ballot_w64(!lane_at_rest(pp, mm, vv, a.nss_bound[s], a)) == 0) {
            for (; s < s_grad; ++s) {
                mm = mm + a.one_minus_b1 * (0.0f - mm);
                vv = vv * a.b2;
            }
        } else if (__builtin_amdgcn_ballot_w64(!lane_ordinary(mm, vv, a)) == 0) {
            for (; s < s_grad; ++s) {
                AdamArgs one{a.one_minus_b1, a.b2, a.one_minus_b2, a.neg_step_size[s], a.bc2_sqrt[s], a.eps};
                if (__builtin_amdgcn_readfirstlane(__float_as_int(one.bc2_sqrt)) == 0x3f800000)
                    adam_one_ordinary<true>(pp, mm, vv, one);
                else
                    adam_one_ordinary<false>(pp, mm, vv, one);
            }
        }
    }
    if (i < n) {
        for (; s < t - t0; ++s) {   // step t0 + s + 1: what is left of the zero-gradient steps, then the gradient step
            AdamArgs one{a.one_minus_b1, a.b2, a.one_minus_b2, a.neg_step_size[s], a.bc2_sqrt[s], a.eps};
            const float gs = (s == s_grad) ? gg : 0.0f;
            if (!WD && __builtin_amdgcn_readfirstlane(__float_as_int(one.bc2_sqrt)) == 0x3f800000)
                adam_elem_unit_bc2(pp, grad_wd<WD>(gs, pp, wd), mm, vv, one);
            else
                adam_elem(pp, grad_wd<WD>(gs, pp, wd), mm, vv, one);
        }
        p[i] = pp;
        m[i] = mm;
        v[i] = vv;
    }
    // a row named only because the NEXT batch reads it has no gradient yet: nothing to clear
    if (__builtin_amdgcn_ballot_w64(gg != 0.0f) != 0 && i < n) g[i] = 0.0f;
}

}  // namespace

// SKR_COLD_STATS=1: a device census of how the cold passes sorted their blocks (read with skr_cold_pass_census /
// skr_cold_rest_census): [0..2] at rest / ordinary / general, [4] / [5] rows trusted as quiet / as zero ([3], [6], [7] unused)
static constexpr int COLD_COUNTERS = 8;
// The environment is read at the first launch and again whenever skr_cold_rest_census is called (reread), so a process can
// switch the census on and off between launches (plain function-static state, as fused_stats_buffer below).
unsigned long long* skr::cold_stats_buffer(bool reread) {
    static unsigned long long* buf = nullptr;
    static bool on = false, read = false;
    if (!read || reread) {
        read = true;
        const char* e = getenv("SKR_COLD_STATS");
        on = e && atoi(e) == 1;
        if (on && !buf) {
            if (hipMalloc(&buf, COLD_COUNTERS * sizeof(unsigned long long)) == hipSuccess)
                (void)hipMemset(buf, 0, COLD_COUNTERS * sizeof(unsigned long long));
            else
                buf = nullptr;
        }
    }
    return on ? buf : nullptr;
}

// SKR_FUSED_STATS=1: a device census of how the fused BPR step's lazily advanced rows were evaluated.  The
// environment is read at the first launch and again whenever skr_fused_census is called (reread), so a process can
// switch the census on and off between launches.
// (Like cold_stats_buffer, plain function-static state: the census is a single-threaded measurement hook, and a process
// that launches from several host threads must switch it on before they start.)
unsigned long long* skr::fused_stats_buffer(bool reread) {
    static unsigned long long* buf = nullptr;
    static bool on = false, read = false;
    if (!read || reread) {
        read = true;
        const char* e = getenv("SKR_FUSED_STATS");
        on = e && atoi(e) == 1;
        if (on && !buf) {
            if (hipMalloc(&buf, FC_COUNTERS * sizeof(unsigned long long)) == hipSuccess)
                (void)hipMemset(buf, 0, FC_COUNTERS * sizeof(unsigned long long));
            else
                buf = nullptr;
        }
    }
    return on ? buf : nullptr;
}

extern "C" {

// The three launches behind the nine public functions.  who: the called function's name, for its error messages;
// tf: tf.train.AdamOptimizer's scalars; wd: the weight decay of the *_wd functions (NULL otherwise; never with tf).
static int adam_step_impl(const char* who, float* d_p, float* d_g, float* d_m, float* d_v, int64_t n, float lr, float beta1,
                          float beta2, float eps, int64_t step_t, int zero_grad, uint8_t* d_touch, bool tf, const float* wd,
                          void* stream) {
    SKR_REQUIRE(d_p && d_g && d_m && d_v, "%s: NULL argument", who);
    SKR_REQUIRE(n >= 0 && step_t >= 1, "%s: n must be >= 0 and step_t >= 1", who);
    SKR_REQUIRE(((reinterpret_cast<uintptr_t>(d_p) | reinterpret_cast<uintptr_t>(d_g) | reinterpret_cast<uintptr_t>(d_m) |
                  reinterpret_cast<uintptr_t>(d_v)) & 15) == 0, "%s: buffers must be 16-byte aligned", who);
    if (n == 0) return SKR_OK;
    AdamArgs a;
    adam_shared_fields(a, beta1, beta2, eps);
    adam_scalars(lr, beta1, beta2, step_t, &a.neg_step_size, &a.bc2_sqrt, tf);
    // Launch shape measured on MI355X (tools/tune_adam.sh, profiles/r01_adam_tuning.txt): 2 workgroups
    // per CU, 4 float4 per lane in flight, non-temporal accesses.  SKR_ADAM_CFG="<blocks_per_cu>,
    // <unroll>,<nt>" overrides it for tuning runs (not for the weight-decay launch).
    static int cfg_bpc = 2, cfg_unroll = 4, cfg_nt = 1;
    static bool cfg_read = false;
    if (!cfg_read) {
        cfg_read = true;
        if (const char* e = getenv("SKR_ADAM_CFG")) sscanf(e, "%d,%d,%d", &cfg_bpc, &cfg_unroll, &cfg_nt);
    }
    int64_t blocks = ((n >> 2) + 255) / 256;
    if (blocks > 256 * (wd ? 2 : cfg_bpc)) blocks = 256 * (wd ? 2 : cfg_bpc);
    if (blocks < 1) blocks = 1;
    const dim3 grid(static_cast<unsigned>(blocks)), blk(256);
    hipStream_t st = skr::as_stream(stream);
#define SKR_ADAM_LAUNCH(T, U_, N_, W_)                                                                                   \
    hipLaunchKernelGGL((adam_kernel<T, U_, N_, W_>), grid, blk, 0, st, d_p, d_g, d_m, d_v, n, a, wd ? *wd : 0.0f, zero_grad, \
                       d_touch)
#define SKR_ADAM_PICK(T)                                                        \
    if (cfg_nt) {                                                               \
        if (cfg_unroll == 4) SKR_ADAM_LAUNCH(T, 4, true, false);                \
        else if (cfg_unroll == 2) SKR_ADAM_LAUNCH(T, 2, true, false);           \
        else SKR_ADAM_LAUNCH(T, 1, true, false);                                \
    } else {                                                                    \
        if (cfg_unroll == 4) SKR_ADAM_LAUNCH(T, 4, false, false);               \
        else if (cfg_unroll == 2) SKR_ADAM_LAUNCH(T, 2, false, false);          \
        else SKR_ADAM_LAUNCH(T, 1, false, false);                               \
    }
    if (wd) { SKR_ADAM_LAUNCH(true, 4, true, true); } else if (d_touch) { SKR_ADAM_PICK(true) } else { SKR_ADAM_PICK(false) }
#undef SKR_ADAM_PICK
#undef SKR_ADAM_LAUNCH
    SKR_LAUNCH_CHECK();
    return SKR_OK;
}

int skr_adam_block_mark(const int32_t* d_ids, int64_t n_ids, int64_t offset_floats, int stride_floats, int32_t* d_tag,
                        int32_t tag_value, int32_t* d_claim, int64_t step_t0, void* stream) {
    SKR_REQUIRE(d_ids && d_tag, "skr_adam_block_mark: NULL argument");
    SKR_REQUIRE(n_ids >= 0 && offset_floats >= 0 && stride_floats >= 1, "skr_adam_block_mark: bad shape");
    SKR_REQUIRE(step_t0 >= 0 && step_t0 < INT32_MAX - AB_KMAX, "skr_adam_block_mark: step_t0 out of range");
    if (n_ids == 0) return SKR_OK;
    hipLaunchKernelGGL(adam_mark_kernel, dim3(static_cast<unsigned>((n_ids + 255) / 256)), dim3(256), 0, skr::as_stream(stream),
                       d_ids, n_ids, offset_floats, stride_floats, d_tag, tag_value, d_claim, static_cast<int32_t>(step_t0));
    SKR_LAUNCH_CHECK();
    return SKR_OK;
}


int skr_cold_pass_census(uint64_t* h_counts3, int reset) {
    SKR_REQUIRE(h_counts3, "skr_cold_pass_census: NULL argument");
    unsigned long long* buf = cold_stats_buffer();
    h_counts3[0] = h_counts3[1] = h_counts3[2] = 0;
    if (!buf) return SKR_OK;
    unsigned long long h[COLD_COUNTERS];
    SKR_HIP(hipDeviceSynchronize());
    SKR_HIP(hipMemcpy(h, buf, sizeof(h), hipMemcpyDeviceToHost));
    if (reset) SKR_HIP(hipMemset(buf, 0, sizeof(h)));
    for (int i = 0; i < 3; ++i) h_counts3[i] = h[i];
    return SKR_OK;
}

int skr_cold_rest_census(uint64_t* h_counts2, int reset) {
    SKR_REQUIRE(h_counts2, "skr_cold_rest_census: NULL argument");
    unsigned long long* buf = cold_stats_buffer(true);
    h_counts2[0] = h_counts2[1] = 0;
    if (!buf) return SKR_OK;
    unsigned long long h[COLD_COUNTERS];
    SKR_HIP(hipDeviceSynchronize());
    SKR_HIP(hipMemcpy(h, buf, sizeof(h), hipMemcpyDeviceToHost));
    if (reset) SKR_HIP(hipMemset(buf, 0, sizeof(h)));
    h_counts2[0] = h[4];
    h_counts2[1] = h[5];
    return SKR_OK;
}


int skr_fused_census(uint64_t* h_counts, int n_counts, int reset) {
    SKR_REQUIRE(h_counts && n_counts >= 0, "skr_fused_census: bad argument");
    for (int i = 0; i < n_counts; ++i) h_counts[i] = 0;
    unsigned long long* buf = fused_stats_buffer(true);
    if (!buf) return SKR_OK;
    unsigned long long h[FC_COUNTERS];
    SKR_HIP(hipDeviceSynchronize());
    SKR_HIP(hipMemcpy(h, buf, sizeof(h), hipMemcpyDeviceToHost));
    if (reset) SKR_HIP(hipMemset(buf, 0, sizeof(h)));
    for (int i = 0; i < n_counts && i < FC_COUNTERS; ++i) h_counts[i] = h[i];
    return SKR_OK;
}

static int adam_block_cold_impl(const char* who, float* d_p, float* d_m, float* d_v, int64_t n, float lr, float beta1, float beta2,
                                float eps, int64_t step_t0, int k, const int32_t* d_tag, int32_t hot_value, bool tf, const float* wd,
                                void* stream, int32_t* d_rest = nullptr, int32_t pass_id = 0) {
    SKR_REQUIRE(d_p && d_m && d_v && d_tag, "%s: NULL argument", who);
    SKR_REQUIRE(n >= 0 && step_t0 >= 0 && k >= 1 && k <= AB_KMAX, "%s: need 1 <= k <= %d", who, AB_KMAX);
    SKR_REQUIRE(((reinterpret_cast<uintptr_t>(d_p) | reinterpret_cast<uintptr_t>(d_m) | reinterpret_cast<uintptr_t>(d_v)) & 15) == 0,
                "%s: buffers must be 16-byte aligned", who);
    if (n == 0) return SKR_OK;
    AdamBlockArgs a{};
    adam_shared_fields(a, beta1, beta2, eps);
    a.k = k;
    adam_block_scalars(a, lr, beta1, beta2, step_t0, k, tf);
    hipStream_t st = skr::as_stream(stream);
    if (wd) {
        // every update moves every element, so there is no row at rest to find: the float4 kernel, and the pass is ALU-bound
        // (k dependent updates per element): fill the CUs
        int64_t blocks = ((n >> 2) + 255) / 256;
        if (blocks > 256 * 8) blocks = 256 * 8;
        if (blocks < 1) blocks = 1;
        hipLaunchKernelGGL((adam_cold_kernel<2, true>), dim3(static_cast<unsigned>(blocks)), dim3(256), 0, st, d_p, d_m, d_v, n, a,
                           *wd, d_tag, hot_value);
        SKR_LAUNCH_CHECK();
        return SKR_OK;
    }
    static const int bpc = [] { const char* e = getenv("SKR_COLD_BPC"); const int v = e ? atoi(e) : 5; return v < 1 ? 1 : (v > 8 ? 8 : v); }();   // workgroups per CU.  The pass runs beside the k-step block's small launches: round 2 settled on 4 (960 timed steps: 24.9 / 31.3 / 30.3 / 28.1 M interactions/s at 2 / 3 / 4 / 8); round 3: 5, together with the step kernel's issue priority (see bpr_fused_step_kernel)
    // SKR_COLD_REST=0 keeps every cold block on the full update (the float4 kernel): the A/B switch of tools/microbench.py
    // (a caller that hands in state words -- skr_adam_block_cold_rest -- has asked for the row kernel and gets it)
    static const bool rest = [] { const char* e = getenv("SKR_COLD_REST"); return !(e && atoi(e) == 0); }();
    // A pass over a WHOLE block of the default length (32 steps and more) of the BPR tables takes six workgroups per CU
    // (SKR_COLD_BPC_FULL; 0: SKR_COLD_BPC for every pass): in the steady state of an epoch the pass and the step stream are
    // balanced (0.53 ms against 32 x 15 us + the write-back), and the sixth workgroup takes 0.04 ms off the pass for 0.4 us per
    // step launch -- an epoch 0.997 -> 0.956 s on the same box (tools/r3_bpc_full.sh).  Shorter blocks (the 20-step slice of
    // the bench line, an epoch's ragged last block) leave the step stream less work to hide the pass behind and keep five: with
    // six for every pass the short slice scatters (34.5-39.5 M interactions/s against 39.4-41.0).  GRU4RecPlus's pass (TF
    // arithmetic) keeps SKR_COLD_BPC: its step is a chain of eight small launches that was measured with five.
    static const int bpc_full = [] { const char* e = getenv("SKR_COLD_BPC_FULL"); const int v = e ? atoi(e) : 6; return v < 1 ? 0 : (v > 8 ? 8 : v); }();
    const int bpc_k = (bpc_full && k >= 32 && !tf) ? bpc_full : bpc;
    adam_block_thresholds(a, lr, beta1, beta2, eps, k);
    a.stats = cold_stats_buffer();
    if (rest || d_rest) {
        int64_t blocks = ((n >> 6) + 4 * 4 - 1) / (4 * 4);
        if (blocks > 256 * bpc_k) blocks = 256 * bpc_k;
        if (blocks < 1) blocks = 1;
        if (d_rest)
            hipLaunchKernelGGL((adam_cold_rows_kernel<4, true>), dim3(static_cast<unsigned>(blocks)), dim3(256), 0, st, d_p, d_m, d_v,
                               n, a, d_tag, hot_value, d_rest, pass_id);
        else
            hipLaunchKernelGGL((adam_cold_rows_kernel<4, false>), dim3(static_cast<unsigned>(blocks)), dim3(256), 0, st, d_p, d_m, d_v,
                               n, a, d_tag, hot_value, static_cast<int32_t*>(nullptr), 0);
    } else {
        int64_t blocks = ((n >> 2) + 255) / 256;
        if (blocks > 256 * bpc) blocks = 256 * bpc;
        if (blocks < 1) blocks = 1;
        hipLaunchKernelGGL((adam_cold_kernel<2, false>), dim3(static_cast<unsigned>(blocks)), dim3(256), 0, st, d_p, d_m, d_v, n, a,
                           0.0f, d_tag, hot_value);
    }
    SKR_LAUNCH_CHECK();
    return SKR_OK;
}

static int adam_block_hot_impl(const char* who, float* d_p, float* d_g, float* d_m, float* d_v, int64_t n, float lr, float beta1,
                               float beta2, float eps, int64_t step_t0, int64_t step_t, const int32_t* d_ids, int64_t n_ids,
                               int64_t offset_floats, int stride_floats, int32_t* d_claim, bool tf, const float* wd, void* stream) {
    SKR_REQUIRE(d_p && d_g && d_m && d_v && d_ids && d_claim, "%s: NULL argument", who);
    SKR_REQUIRE(n >= 0 && step_t0 >= 0 && step_t > step_t0 && step_t - step_t0 <= AB_KMAX && step_t < INT32_MAX,
                "%s: need step_t0 < step_t <= step_t0 + %d", who, AB_KMAX);
    SKR_REQUIRE(n_ids >= 0 && offset_floats >= 0 && stride_floats >= 1, "%s: bad shape", who);
    if (n_ids == 0) return SKR_OK;
    AdamBlockArgs a{};
    adam_shared_fields(a, beta1, beta2, eps);
    a.k = static_cast<int>(step_t - step_t0);
    adam_block_scalars(a, lr, beta1, beta2, step_t0, a.k, tf);
    if (!wd) adam_block_thresholds(a, lr, beta1, beta2, eps, a.k);   // for the zero-gradient steps a block may be behind
#define SKR_HOT_LAUNCH(W_)                                                                                                         \
    hipLaunchKernelGGL(adam_hot_kernel<W_>, dim3(static_cast<unsigned>((n_ids + 3) / 4)), dim3(256), 0, skr::as_stream(stream), d_p, \
                       d_g, d_m, d_v, n, a, wd ? *wd : 0.0f, static_cast<int32_t>(step_t0), static_cast<int32_t>(step_t), d_ids, \
                       n_ids, offset_floats, stride_floats, d_claim)
    if (wd) SKR_HOT_LAUNCH(true); else SKR_HOT_LAUNCH(false);
#undef SKR_HOT_LAUNCH
    SKR_LAUNCH_CHECK();
    return SKR_OK;
}

int skr_adam_step(float* d_p, float* d_g, float* d_m, float* d_v, int64_t n, float lr, float beta1, float beta2,
                  float eps, int64_t step_t, int zero_grad, uint8_t* d_touch, void* stream) {
    return adam_step_impl("skr_adam_step", d_p, d_g, d_m, d_v, n, lr, beta1, beta2, eps, step_t, zero_grad, d_touch, false, nullptr,
                          stream);
}
int skr_adam_step_tf(float* d_p, float* d_g, float* d_m, float* d_v, int64_t n, float lr, float beta1, float beta2,
                     float eps, int64_t step_t, int zero_grad, uint8_t* d_touch, void* stream) {
    return adam_step_impl("skr_adam_step_tf", d_p, d_g, d_m, d_v, n, lr, beta1, beta2, eps, step_t, zero_grad, d_touch, true, nullptr,
                          stream);
}
int skr_adam_step_wd(float* d_p, float* d_g, float* d_m, float* d_v, int64_t n, float lr, float beta1, float beta2, float eps,
                     float weight_decay, int64_t step_t, int zero_grad, uint8_t* d_touch, void* stream) {
    return adam_step_impl("skr_adam_step_wd", d_p, d_g, d_m, d_v, n, lr, beta1, beta2, eps, step_t, zero_grad, d_touch, false,
                          &weight_decay, stream);
}

int skr_adam_block_cold(float* d_p, float* d_m, float* d_v, int64_t n, float lr, float beta1, float beta2, float eps,
                        int64_t step_t0, int k, const int32_t* d_tag, int32_t hot_value, void* stream) {
    return adam_block_cold_impl("skr_adam_block_cold", d_p, d_m, d_v, n, lr, beta1, beta2, eps, step_t0, k, d_tag, hot_value, false,
                                nullptr, stream);
}
int skr_adam_block_cold_rest(float* d_p, float* d_m, float* d_v, int64_t n, float lr, float beta1, float beta2, float eps,
                             int64_t step_t0, int k, const int32_t* d_tag, int32_t hot_value, int32_t* d_rest, int32_t pass_id,
                             void* stream) {
    SKR_REQUIRE(d_rest, "skr_adam_block_cold_rest: NULL argument");
    SKR_REQUIRE(pass_id >= 1 && pass_id < (1 << 29), "skr_adam_block_cold_rest: need 1 <= pass_id < 2^29");
    return adam_block_cold_impl("skr_adam_block_cold_rest", d_p, d_m, d_v, n, lr, beta1, beta2, eps, step_t0, k, d_tag, hot_value,
                                false, nullptr, stream, d_rest, pass_id);
}
int skr_adam_block_cold_tf(float* d_p, float* d_m, float* d_v, int64_t n, float lr, float beta1, float beta2, float eps,
                           int64_t step_t0, int k, const int32_t* d_tag, int32_t hot_value, void* stream) {
    return adam_block_cold_impl("skr_adam_block_cold_tf", d_p, d_m, d_v, n, lr, beta1, beta2, eps, step_t0, k, d_tag, hot_value, true,
                                nullptr, stream);
}
int skr_adam_block_cold_wd(float* d_p, float* d_m, float* d_v, int64_t n, float lr, float beta1, float beta2, float eps,
                           float weight_decay, int64_t step_t0, int k, const int32_t* d_tag, int32_t hot_value, void* stream) {
    return adam_block_cold_impl("skr_adam_block_cold_wd", d_p, d_m, d_v, n, lr, beta1, beta2, eps, step_t0, k, d_tag, hot_value, false,
                                &weight_decay, stream);
}

int skr_adam_block_hot(float* d_p, float* d_g, float* d_m, float* d_v, int64_t n, float lr, float beta1, float beta2,
                       float eps, int64_t step_t0, int64_t step_t, const int32_t* d_ids, int64_t n_ids, int64_t offset_floats,
                       int stride_floats, int32_t* d_claim, void* stream) {
    return adam_block_hot_impl("skr_adam_block_hot", d_p, d_g, d_m, d_v, n, lr, beta1, beta2, eps, step_t0, step_t, d_ids, n_ids,
                               offset_floats, stride_floats, d_claim, false, nullptr, stream);
}
int skr_adam_block_hot_tf(float* d_p, float* d_g, float* d_m, float* d_v, int64_t n, float lr, float beta1, float beta2,
                          float eps, int64_t step_t0, int64_t step_t, const int32_t* d_ids, int64_t n_ids, int64_t offset_floats,
                          int stride_floats, int32_t* d_claim, void* stream) {
    return adam_block_hot_impl("skr_adam_block_hot_tf", d_p, d_g, d_m, d_v, n, lr, beta1, beta2, eps, step_t0, step_t, d_ids, n_ids,
                               offset_floats, stride_floats, d_claim, true, nullptr, stream);
}
int skr_adam_block_hot_wd(float* d_p, float* d_g, float* d_m, float* d_v, int64_t n, float lr, float beta1, float beta2,
                          float eps, float weight_decay, int64_t step_t0, int64_t step_t, const int32_t* d_ids, int64_t n_ids,
                          int64_t offset_floats, int stride_floats, int32_t* d_claim, void* stream) {
    return adam_block_hot_impl("skr_adam_block_hot_wd", d_p, d_g, d_m, d_v, n, lr, beta1, beta2, eps, step_t0, step_t, d_ids, n_ids,
                               offset_floats, stride_floats, d_claim, false, &weight_decay, stream);
}

int skr_selftest_cold_math(uint64_t n_pairs, uint64_t* h_mismatches, void* stream) {
    SKR_REQUIRE(h_mismatches, "skr_selftest_cold_math: NULL argument");
    unsigned long long* d_bad = nullptr;
    SKR_HIP(hipMalloc(&d_bad, 4 * sizeof(unsigned long long)));
    SKR_HIP(hipMemsetAsync(d_bad, 0, 4 * sizeof(unsigned long long), skr::as_stream(stream)));
    // square root: every float in [2^-96, largest finite]
    hipLaunchKernelGGL(selftest_cold_math_kernel, dim3(256 * 8), dim3(256), 0, skr::as_stream(stream), 0x0f800000u, 0x7f7fffffu,
                       n_pairs, d_bad);
    SKR_LAUNCH_CHECK();
    unsigned long long h[4] = {0, 0, 0, 0};
    SKR_HIP(hipMemcpyAsync(h, d_bad, sizeof(h), hipMemcpyDeviceToHost, skr::as_stream(stream)));
    SKR_HIP(hipStreamSynchronize(skr::as_stream(stream)));
    (void)hipFree(d_bad);
    h_mismatches[0] = h[0];
    h_mismatches[1] = h[1];
    h_mismatches[2] = h[2];
    h_mismatches[3] = h[3];
    return SKR_OK;
}

int skr_selftest_grad_math(uint64_t n_tuples, float lr, float beta1, float beta2, float eps, int64_t step_t0, int k, int tf,
                           int run_len, uint64_t* h_counts5, void* stream) {
    SKR_REQUIRE(h_counts5, "skr_selftest_grad_math: NULL argument");
    SKR_REQUIRE(step_t0 >= 0 && k >= 1 && k <= AB_KMAX && run_len >= 1, "skr_selftest_grad_math: need 1 <= k <= %d, run_len >= 1", AB_KMAX);
    AdamBlockArgs a{};
    adam_shared_fields(a, beta1, beta2, eps);
    a.k = k;
    adam_block_scalars(a, lr, beta1, beta2, step_t0, k, tf != 0);
    adam_block_thresholds(a, lr, beta1, beta2, eps, k);
    unsigned long long* d_out = nullptr;
    SKR_HIP(hipMalloc(&d_out, 5 * sizeof(unsigned long long)));
    SKR_HIP(hipMemsetAsync(d_out, 0, 5 * sizeof(unsigned long long), skr::as_stream(stream)));
    hipLaunchKernelGGL(selftest_grad_math_kernel, dim3(256 * 4), dim3(256), 0, skr::as_stream(stream), n_tuples / 64, a, run_len, d_out);
    SKR_LAUNCH_CHECK();
    unsigned long long h[5] = {0, 0, 0, 0, 0};
    SKR_HIP(hipMemcpyAsync(h, d_out, sizeof(h), hipMemcpyDeviceToHost, skr::as_stream(stream)));
    SKR_HIP(hipStreamSynchronize(skr::as_stream(stream)));
    (void)hipFree(d_out);
    for (int q = 0; q < 5; ++q) h_counts5[q] = h[q];
    return SKR_OK;
}

int skr_selftest_step_chain(uint64_t n_tuples, float lr, float beta1, float beta2, float eps, int64_t step_t0, int k, int s_from,
                            int run_len, int with_grad, uint64_t* h_counts5, void* stream) {
    SKR_REQUIRE(h_counts5, "skr_selftest_step_chain: NULL argument");
    SKR_REQUIRE(step_t0 >= 0 && k >= 1 && k <= AB_KMAX && s_from >= 0 && s_from < k && run_len >= 1,
                "skr_selftest_step_chain: need 0 <= s_from < k <= %d, run_len >= 1", AB_KMAX);
    AdamBlockArgs a{};
    adam_shared_fields(a, beta1, beta2, eps);
    a.k = k;
    adam_block_scalars(a, lr, beta1, beta2, step_t0, k, false);
    adam_block_thresholds(a, lr, beta1, beta2, eps, k);
    unsigned long long* d_out = nullptr;
    SKR_HIP(hipMalloc(&d_out, 5 * sizeof(unsigned long long)));
    SKR_HIP(hipMemsetAsync(d_out, 0, 5 * sizeof(unsigned long long), skr::as_stream(stream)));
    hipLaunchKernelGGL(selftest_step_chain_kernel, dim3(256 * 4), dim3(256), 0, skr::as_stream(stream), n_tuples / 64, a, s_from,
                       run_len, with_grad, d_out);
    SKR_LAUNCH_CHECK();
    unsigned long long h[5] = {0, 0, 0, 0, 0};
    SKR_HIP(hipMemcpyAsync(h, d_out, sizeof(h), hipMemcpyDeviceToHost, skr::as_stream(stream)));
    SKR_HIP(hipStreamSynchronize(skr::as_stream(stream)));
    (void)hipFree(d_out);
    for (int q = 0; q < 5; ++q) h_counts5[q] = h[q];
    return SKR_OK;
}

}  // extern "C"
