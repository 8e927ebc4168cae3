// adam_math.h -- the Adam arithmetic shared by the optimiser (adam.hip) and the fused BPR step (bpr_fused.hip): the
// per-element update (moment update + step quotient), its exact cheaper evaluations -- for zero-gradient updates in the cold
// pass, for gradient updates and zero-gradient runs of the lazily advanced rows (adam_grad_run / adam_zero_run) -- their
// census, and the per-step scalars on the host.
#pragma once
#include "skr_common.h"

#include <cassert>
#include <cmath>

namespace skr {

// per-step scalars of torch.optim.Adam's single-tensor path (adam_scalars)
struct AdamArgs {
    float one_minus_b1, b2, one_minus_b2, neg_step_size, bc2_sqrt, eps;
};

// the moment update every evaluation shares (AdamArgs or AdamBlockArgs): m' and v' are the same bits on every path
template <class A>
__device__ __forceinline__ void adam_moments(float g, float& m, float& v, const A& a) {
    m = m + a.one_minus_b1 * (g - m);           // exp_avg.lerp_(grad, 1-beta1)
    v = v * a.b2 + (a.one_minus_b2 * g) * g;    // mul_(beta2).addcmul_(grad, grad, value=1-beta2)
}

// the step's quotient from the updated moments, general form.  UNIT_BC2: sqrt(1 - beta2^t) is exactly 1.0f (beta2 = 0.999:
// from step ~16 600 on): x / 1.0f == x, so the correctly rounded division by the bias correction (a dozen instructions) is
// left out -- results are identical
template <bool UNIT_BC2>
__device__ __forceinline__ float adam_quot(float m, float v, float neg_step_size, float bc2_sqrt, float eps) {
    const float denom = UNIT_BC2 ? sqrtf(v) + eps : sqrtf(v) / bc2_sqrt + eps;
    return (neg_step_size * m) / denom;         // addcdiv_(exp_avg, denom, value=-step_size)
}

__device__ __forceinline__ void adam_elem(float& p, float g, float& m, float& v, const AdamArgs& a) {
    adam_moments(g, m, v, a);
    p = p + adam_quot<false>(m, v, a.neg_step_size, a.bc2_sqrt, a.eps);
}

__device__ __forceinline__ void adam_elem_unit_bc2(float& p, float g, float& m, float& v, const AdamArgs& a) {
    adam_moments(g, m, v, a);
    p = p + adam_quot<true>(m, v, a.neg_step_size, a.bc2_sqrt, a.eps);
}

// the scalars of a block of k <= AB_KMAX consecutive steps (adam.hip K2b, bpr_fused.hip K2c)
constexpr int AB_KMAX = 64;
struct AdamBlockArgs {
    float one_minus_b1, b2, one_minus_b2, eps;
    float neg_step_size[AB_KMAX], bc2_sqrt[AB_KMAX];
    float nss_bound[AB_KMAX];   // max |neg_step_size[s']| over s' >= s: the bound the at-rest test of a run starting at s needs
                                // (torch's -lr / bc1 only shrinks with the step: then this IS |neg_step_size[s]|; TF's
                                //  -lr * sqrt(bc2) / bc1 falls, then rises again towards lr)
    int k;
    // thresholds of the "parameter at rest" test of adam_cold_rows_kernel (0 switches the test off)
    float rest_eps;   // 2^-28 * eps
    float rest_b2k;   // a lower bound of beta2^k
    // ranges of the "ordinary magnitudes" test (fast_mlo = +inf switches it off)
    float fast_vlo, fast_mlo, fast_mhi;
    unsigned long long* stats;   // optional census: the cold pass's (SKR_COLD_STATS=1: blocks at rest / ordinary / general) or,
                                 // in the fused step's launches, theirs (SKR_FUSED_STATS=1: FC_* below)
    int first_unit;              // the smallest s with bc2_sqrt[s] == 1.0f, k if there is none (from there on it stays 1.0f)
};

// Square root and division for ORDINARY MAGNITUDES, bit-identical to sqrtf(x) and n / d as compiled under
// -fhip-fp32-correctly-rounded-divide-sqrt but cheaper:
//   div_ordinary   the compiler's own expansion (v_rcp_f32, one Newton step, two quotient corrections, final fma)
//                  minus v_div_scale_f32 and v_div_fixup_f32, which are the identity (VCC = 0) / a pass-through when
//                  d is normal with |d| < 2^126, |n| >= 2^-103 and -125 <= exponent(n) - exponent(d) < 96
//                  (CDNA3/4 ISA, V_DIV_SCALE_F32 / V_DIV_FIXUP_F32): same instructions on the same values;
//   sqrt_ordinary  v_rsq_f32 and one fused correction s + (x - s*s) * r/2 instead of v_sqrt_f32 and two residual tests:
//                  a different route to the correctly rounded root, so it is PROVEN BY ENUMERATION -- the self-test runs
//                  it against sqrtf on every float of [2^-96, FLT_MAX] (the range it is used on is [2^-90, 2^20]).
// skr_selftest_cold_math does that enumeration and tries the division on 2^32 hashed operand pairs of its range; as
// a control it also counts how often the raw v_sqrt_f32 differs from sqrtf (it must: that is why a correction exists).
__device__ __forceinline__ float sqrt_ordinary(float x) {
    const float r = __builtin_amdgcn_rsqf(x);
    const float s = x * r, h = 0.5f * r;
    return __builtin_fmaf(__builtin_fmaf(-s, s, x), h, s);
}

__device__ __forceinline__ float div_ordinary(float n, float d) {
    float r = __builtin_amdgcn_rcpf(d);
    const float e = __builtin_fmaf(-d, r, 1.0f);
    r = __builtin_fmaf(e, r, r);
    float q = n * r;
    float t = __builtin_fmaf(-d, q, n);
    q = __builtin_fmaf(t, r, q);
    t = __builtin_fmaf(-d, q, n);
    return __builtin_fmaf(t, r, q);
}

typedef float f32x2 __attribute__((ext_vector_type(2)));

// one zero-gradient update of two rows of ordinary magnitudes (v > 0, so v*b2 + (c2*0)*0 == v*b2)
template <bool UNIT_BC2>
__device__ __forceinline__ void adam_pair_ordinary(f32x2& p, f32x2& m, f32x2& v, const AdamArgs& a) {
    m = m + a.one_minus_b1 * (0.0f - m);
    v = v * a.b2;
    f32x2 sq;
    sq.x = sqrt_ordinary(v.x);
    sq.y = sqrt_ordinary(v.y);
    if (!UNIT_BC2) {
        sq.x = div_ordinary(sq.x, a.bc2_sqrt);
        sq.y = div_ordinary(sq.y, a.bc2_sqrt);
    }
    const f32x2 d = sq + a.eps, n = a.neg_step_size * m;
    f32x2 q;
    q.x = div_ordinary(n.x, d.x);
    q.y = div_ordinary(n.y, d.y);
    p = p + q;
}

template <bool UNIT_BC2>
__device__ __forceinline__ void adam_one_ordinary(float& p, float& m, float& v, const AdamArgs& a) {
    m = m + a.one_minus_b1 * (0.0f - m);
    v = v * a.b2;
    float sq = sqrt_ordinary(v);
    if (!UNIT_BC2) sq = div_ordinary(sq, a.bc2_sqrt);
    p = p + div_ordinary(a.neg_step_size * m, sq + a.eps);
}

// the two per-lane tests of the cold pass (and of the hot step's catch-up): see adam_cold_rows_kernel (adam.hip).  nss0 = the largest
// |neg_step_size| among the zero-gradient updates in question (AdamBlockArgs::nss_bound of the first of them)
__device__ __forceinline__ bool lane_at_rest(float pp, float mm, float vv, float nss0, const AdamBlockArgs& a) {
    const float ap = fabsf(pp), n0 = nss0 * fabsf(mm);
    const float r = ap * 0x1p-29f;
    const float bound = (r * r) * (vv * a.rest_b2k);
    const bool small = n0 < ap * a.rest_eps || (n0 * n0 < bound && bound >= 0x1p-120f);
    return __float_as_uint(vv) <= 0x7f800000u && ap >= 0x1p-60f && small;
}

__device__ __forceinline__ bool lane_ordinary(float mm, float vv, const AdamBlockArgs& a) {
    const float am = fabsf(mm);
    return vv >= a.fast_vlo && vv <= 0x1p20f && am >= a.fast_mlo && am <= a.fast_mhi;
}

// ---- the lazy rows' updates (fused_advance of bpr_fused.hip) -----------------------------------------------------------------
// The scaling-free quotient of one update from the UPDATED moments: the same operations as adam_one_ordinary
template <bool UNIT_BC2>
__device__ __forceinline__ float adam_quot_ordinary(float m, float v, float neg_step_size, float bc2_sqrt, float eps) {
    float sq = sqrt_ordinary(v);
    if (!UNIT_BC2) sq = div_ordinary(sq, bc2_sqrt);
    return div_ordinary(neg_step_size * m, sq + eps);
}

// census of the lazy rows' evaluations (SKR_FUSED_STATS=1, skr_fused_census): counter = 8 * kernel + 4 * kind + class
enum { FC_STEP_ROW = 0, FC_STEP_BIAS = 1, FC_END = 2, FC_PRE = 3, FC_KERNELS = 4 };   // kernel
enum { FC_GRAD = 0, FC_RUN = 1 };                                                               // kind: gradient update / zero-gradient run
enum { FC_REST = 0, FC_ORD = 1, FC_GENERAL = 3 };                                               // class (2: not used)
constexpr int FC_END_PAIRED = 8 * FC_KERNELS;       // end launch: slots advanced two to a wavefront / alone
constexpr int FC_END_SINGLE = FC_END_PAIRED + 1;
constexpr int FC_COUNTERS = FC_END_PAIRED + 2;

__device__ __forceinline__ void fused_count(const AdamBlockArgs& a, int ck, int kind, int cls) {
    if (a.stats && (threadIdx.x & 63) == 0) atomicAdd(&a.stats[8 * ck + 4 * kind + cls], 1ull);
}

// Updates [s, s_to) of a row of ordinary magnitudes.  `updated`: the moments already hold update s (the gradient update's,
// which then is the first chain here); every other update is a zero-gradient one.  The quotient of an update depends on
// that update's m and v only -- not on p -- so the square-root / division chains of consecutive updates are independent of
// each other: four of them are laid side by side (one wavefront alone on its SIMD otherwise waits out the latency of every
// one of the ~25 dependent instructions of a chain: ~200 cycles per update instead of ~70), and p takes the quotients in
// order -- the same operations on the same values as update after update.
template <bool UNIT_BC2>
__device__ __forceinline__ void ordinary_run(float& p, float& m, float& v, const AdamBlockArgs& a, int& s, int s_to, bool& updated) {
    for (; s + 4 <= s_to; s += 4) {
        float ms[4], vs[4], q[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (u > 0 || !updated) {
                m = m + a.one_minus_b1 * (0.0f - m);
                v = v * a.b2;
            }
            ms[u] = m;
            vs[u] = v;
        }
        updated = false;
#pragma unroll
        for (int u = 0; u < 4; ++u) q[u] = adam_quot_ordinary<UNIT_BC2>(ms[u], vs[u], a.neg_step_size[s + u], a.bc2_sqrt[s + u], a.eps);
#pragma unroll
        for (int u = 0; u < 4; ++u) p = p + q[u];
    }
    for (; s < s_to; ++s) {
        if (!updated) {
            m = m + a.one_minus_b1 * (0.0f - m);
            v = v * a.b2;
        }
        updated = false;
        p = p + adam_quot_ordinary<UNIT_BC2>(m, v, a.neg_step_size[s], a.bc2_sqrt[s], a.eps);
    }
}

// the same, choosing the form: sqrt(1 - beta2^t) rises with t and stays at 1.0f once it gets there, so a run is all-unit,
// all-non-unit, or (around step 16 600, once) mixed -- then update by update
__device__ __forceinline__ void fast_run(float& p, float& m, float& v, const AdamBlockArgs& a, int s, int s_to, bool updated) {
    if (s >= s_to) return;
    if (__builtin_amdgcn_readfirstlane(__float_as_int(a.bc2_sqrt[s])) == 0x3f800000) {
        ordinary_run<true>(p, m, v, a, s, s_to, updated);
    } else if (__builtin_amdgcn_readfirstlane(__float_as_int(a.bc2_sqrt[s_to - 1])) != 0x3f800000) {
        ordinary_run<false>(p, m, v, a, s, s_to, updated);
    } else {
        for (; s < s_to; ++s) {
            int s1 = s;
            if (__builtin_amdgcn_readfirstlane(__float_as_int(a.bc2_sqrt[s])) == 0x3f800000)
                ordinary_run<true>(p, m, v, a, s1, s + 1, updated);
            else
                ordinary_run<false>(p, m, v, a, s1, s + 1, updated);
        }
    }
}

// zero-gradient updates [s, s_to) of one row, on the cold pass's three evaluations (all 64 lanes at rest: the moments decay;
// all of ordinary magnitudes: scaling-free; general otherwise).  ck: the census's kernel index
__device__ __forceinline__ void adam_zero_run(float& p, float& m, float& v, const AdamBlockArgs& a, int s, int s_to, int ck) {
    if (s >= s_to) return;
    if (__builtin_amdgcn_ballot_w64(!lane_at_rest(p, m, v, a.nss_bound[s], a)) == 0) {
        fused_count(a, ck, FC_RUN, FC_REST);
        for (; s < s_to; ++s) {
            m = m + a.one_minus_b1 * (0.0f - m);
            v = v * a.b2;
        }
    } else if (__builtin_amdgcn_ballot_w64(!lane_ordinary(m, v, a)) == 0) {
        fused_count(a, ck, FC_RUN, FC_ORD);
        fast_run(p, m, v, a, s, s_to, false);
    } else {
        fused_count(a, ck, FC_RUN, FC_GENERAL);
        for (; s < s_to; ++s) {
            AdamArgs one{a.one_minus_b1, a.b2, a.one_minus_b2, a.neg_step_size[s], a.bc2_sqrt[s], a.eps};
            if (__builtin_amdgcn_readfirstlane(__float_as_int(one.bc2_sqrt)) == 0x3f800000)
                adam_elem_unit_bc2(p, 0.0f, m, v, one);
            else
                adam_elem(p, 0.0f, m, v, one);
        }
    }
}

// update s with gradient g, then the zero-gradient updates [s + 1, s_to).  The lanes are tested ONCE, after the moment
// update, on (m', v'): the ranges of sqrt_ordinary / div_ordinary then hold for the very operands of this update's quotient,
// and the block's thresholds cover the decays of every later update of the block -- so the run behind the gradient update
// needs no test of its own, and the gradient update's quotient is the first of ordinary_run's side-by-side chains.
// Needs s < s_to <= a.k (update s is always made).  Returns whether the wavefront took the scaling-free evaluation.
// adam_grad_finish is the part behind the moment update and the test (`ord`: every lane passed lane_ordinary on m', v').
__device__ __forceinline__ bool adam_grad_finish(float& p, float& m, float& v, const AdamBlockArgs& a, int s, int s_to, int ck, bool ord) {
    if (ord) {
        fused_count(a, ck, FC_GRAD, FC_ORD);
        if (s + 1 < s_to) fused_count(a, ck, FC_RUN, FC_ORD);
        fast_run(p, m, v, a, s, s_to, true);
        return true;
    }
    fused_count(a, ck, FC_GRAD, FC_GENERAL);
    const float nss = a.neg_step_size[s], bc2 = a.bc2_sqrt[s];
    if (__builtin_amdgcn_readfirstlane(__float_as_int(bc2)) == 0x3f800000)
        p = p + adam_quot<true>(m, v, nss, bc2, a.eps);
    else
        p = p + adam_quot<false>(m, v, nss, bc2, a.eps);
    adam_zero_run(p, m, v, a, s + 1, s_to, ck);
    return false;
}

__device__ __forceinline__ bool adam_grad_run(float& p, float g, float& m, float& v, const AdamBlockArgs& a, int s, int s_to, int ck) {
    adam_moments(g, m, v, a);
    return adam_grad_finish(p, m, v, a, s, s_to, ck, __builtin_amdgcn_ballot_w64(!lane_ordinary(m, v, a)) == 0);
}

// zero-gradient updates [s, s_to) of TWO rows of ordinary magnitudes in one wavefront, on the cold pass's packed pair form
__device__ __forceinline__ void adam_pair_run(f32x2& p, f32x2& m, f32x2& v, const AdamBlockArgs& a, int s, int s_to) {
    for (; s < s_to; ++s) {
        AdamArgs one{a.one_minus_b1, a.b2, a.one_minus_b2, a.neg_step_size[s], a.bc2_sqrt[s], a.eps};
        if (__builtin_amdgcn_readfirstlane(__float_as_int(one.bc2_sqrt)) == 0x3f800000)
            adam_pair_ordinary<true>(p, m, v, one);
        else
            adam_pair_ordinary<false>(p, m, v, one);
    }
}

// ---- the lazy rows' updates with the block's per-step scalars held in LANES (bpr_fused_step_kernel) ------------------------
// The forms above read a.neg_step_size[s], a.bc2_sqrt[s] and a.nss_bound[s] from the kernel-argument segment: a scalar load
// and a full wait each time, on the critical path of the one wavefront a SIMD holds.  Here lane l of four registers holds
// step l's scalars (AB_KMAX is the wavefront size), loaded once per wavefront; a step's scalar is then one v_readlane_b32.
// The fourth register holds the refined reciprocal of bc2_sqrt[l] -- the first three instructions of div_ordinary(x, bc2),
// which depend on the step only -- so that a division by bc2 starts at q = n * r (div_ordinary_r).  first_unit replaces the
// comparisons of bc2_sqrt with 1.0f.  Same operations on the same values as adam_grad_run / adam_zero_run
// (skr_selftest_step_chain compares the two, bits of p, m and v).
static_assert(AB_KMAX == 64, "the lane tables hold one step per lane of a 64-wide wavefront");

// div_ordinary with the refined reciprocal r of d handed in: r = rcp(d); r = fma(fma(-d, r, 1), r, r)
__device__ __forceinline__ float div_ordinary_r(float n, float d, float r) {
    float q = n * r;
    float t = __builtin_fmaf(-d, q, n);
    q = __builtin_fmaf(t, r, q);
    t = __builtin_fmaf(-d, q, n);
    return __builtin_fmaf(t, r, q);
}

// what the chain reads: AdamBlockArgs' scalars (in scalar registers) and the four lane tables
struct AdamChainArgs {
    float one_minus_b1, b2, one_minus_b2, eps;
    float rest_eps, rest_b2k, fast_vlo, fast_mlo, fast_mhi;
    int first_unit;
    unsigned long long* stats;
    float t_nss, t_bc2, t_bound, t_rbc2;      // lane l: neg_step_size[l], bc2_sqrt[l], nss_bound[l], refined 1 / bc2_sqrt[l]
};

// (lanes k .. 63 hold the arrays' zero padding and what its reciprocal gives: no step reads them)
__device__ __forceinline__ AdamChainArgs adam_chain_args(const AdamBlockArgs& a) {
    const int l = threadIdx.x & 63;
    AdamChainArgs c;
    c.one_minus_b1 = a.one_minus_b1, c.b2 = a.b2, c.one_minus_b2 = a.one_minus_b2, c.eps = a.eps;
    c.rest_eps = a.rest_eps, c.rest_b2k = a.rest_b2k, c.fast_vlo = a.fast_vlo, c.fast_mlo = a.fast_mlo, c.fast_mhi = a.fast_mhi;
    c.first_unit = a.first_unit;
    c.stats = a.stats;
    c.t_nss = a.neg_step_size[l], c.t_bc2 = a.bc2_sqrt[l], c.t_bound = a.nss_bound[l];
    const float r = __builtin_amdgcn_rcpf(c.t_bc2);
    c.t_rbc2 = __builtin_fmaf(__builtin_fmaf(-c.t_bc2, r, 1.0f), r, r);
    return c;
}

// step s's entry of a lane table (s is wave-uniform)
__device__ __forceinline__ float lane_scalar(float table, int s) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(table), s));
}

// lane_at_rest / lane_ordinary / fused_count on the chain's copy of the thresholds: the same tests
__device__ __forceinline__ bool lane_at_rest(float pp, float mm, float vv, float nss0, const AdamChainArgs& c) {
    const float ap = fabsf(pp), n0 = nss0 * fabsf(mm);
    const float r = ap * 0x1p-29f;
    const float bound = (r * r) * (vv * c.rest_b2k);
    const bool small = n0 < ap * c.rest_eps || (n0 * n0 < bound && bound >= 0x1p-120f);
    return __float_as_uint(vv) <= 0x7f800000u && ap >= 0x1p-60f && small;
}

__device__ __forceinline__ bool lane_ordinary(float mm, float vv, const AdamChainArgs& c) {
    const float am = fabsf(mm);
    return vv >= c.fast_vlo && vv <= 0x1p20f && am >= c.fast_mlo && am <= c.fast_mhi;
}

__device__ __forceinline__ void fused_count(const AdamChainArgs& c, int ck, int kind, int cls) {
    if (c.stats && (threadIdx.x & 63) == 0) atomicAdd(&c.stats[8 * ck + 4 * kind + cls], 1ull);
}

// adam_quot_ordinary with step s's scalars from the lane tables
template <bool UNIT_BC2>
__device__ __forceinline__ float chain_quot_ordinary(float m, float v, const AdamChainArgs& c, int s) {
    float sq = sqrt_ordinary(v);
    if (!UNIT_BC2) sq = div_ordinary_r(sq, lane_scalar(c.t_bc2, s), lane_scalar(c.t_rbc2, s));
    return div_ordinary(lane_scalar(c.t_nss, s) * m, sq + c.eps);
}

// The same three forms on TWO values at once: every multiply, add and fused multiply-add is one packed instruction
// (v_pk_mul_f32 / v_pk_add_f32 / v_pk_fma_f32) on both halves, v_rsq_f32 and v_rcp_f32 stay per half.  Operation for
// operation the scalar forms -- under -ffp-contract=off a vector `*` or `+` stays unfused and __builtin_elementwise_fma
// stays fused, exactly as there -- so each half sees the same IEEE operations on the same values.  Measured for one
// wavefront alone on its SIMD (profiles/fused_pack_timing.json): a packed FMA holds the issue as long as two plain ones,
// but in a DEPENDENT chain it costs 9.3 ticks against 6.3 -- two updates for one and a half times the price of one.
__device__ __forceinline__ f32x2 sqrt_ordinary(f32x2 x) {
    f32x2 r;
    r.x = __builtin_amdgcn_rsqf(x.x);
    r.y = __builtin_amdgcn_rsqf(x.y);
    const f32x2 s = x * r, h = 0.5f * r;
    return __builtin_elementwise_fma(__builtin_elementwise_fma(-s, s, x), h, s);
}

__device__ __forceinline__ f32x2 div_ordinary_r(f32x2 n, f32x2 d, f32x2 r) {
    f32x2 q = n * r;
    f32x2 t = __builtin_elementwise_fma(-d, q, n);
    q = __builtin_elementwise_fma(t, r, q);
    t = __builtin_elementwise_fma(-d, q, n);
    return __builtin_elementwise_fma(t, r, q);
}

__device__ __forceinline__ f32x2 div_ordinary(f32x2 n, f32x2 d) {
    f32x2 r;
    r.x = __builtin_amdgcn_rcpf(d.x);
    r.y = __builtin_amdgcn_rcpf(d.y);
    const f32x2 one = {1.0f, 1.0f};
    const f32x2 e = __builtin_elementwise_fma(-d, r, one);
    r = __builtin_elementwise_fma(e, r, r);
    return div_ordinary_r(n, d, r);
}

// steps s0 and s1's entries of a lane table in the two halves
__device__ __forceinline__ f32x2 lane_scalar2(float table, int s0, int s1) {
    f32x2 t;
    t.x = lane_scalar(table, s0);
    t.y = lane_scalar(table, s1);
    return t;
}

// chain_quot_ordinary for two updates of one row: .x holds the moments of update s0, .y those of update s1 (both of one
// form: a pair never straddles first_unit, see chain_fast_run)
template <bool UNIT_BC2>
__device__ __forceinline__ f32x2 chain_quot_ordinary(f32x2 m, f32x2 v, const AdamChainArgs& c, int s0, int s1) {
    f32x2 sq = sqrt_ordinary(v);
    if (!UNIT_BC2) sq = div_ordinary_r(sq, lane_scalar2(c.t_bc2, s0, s1), lane_scalar2(c.t_rbc2, s0, s1));
    return div_ordinary(lane_scalar2(c.t_nss, s0, s1) * m, sq + c.eps);
}

// Updates [s, s + n) of a row of ordinary magnitudes as NP pairs side by side, n = 2 NP - 1 or 2 NP (wave-uniform).  The
// quotient of an update depends on that update's m and v only -- not on p -- so the moments are produced in order, the
// square-root / division chains of the NP pairs are independent of each other, and p takes the quotients in order: the same
// operations on the same values as update after update.  With n odd the last pair's second half is no update: it repeats
// the first half's moments and step index (a valid lane of the tables, whatever s + n is -- index 63 has no successor
// lane), and its quotient goes nowhere.
template <bool UNIT_BC2, int NP>
__device__ __forceinline__ void chain_ordinary_group(float& p, float& m, float& v, const AdamChainArgs& c, int s, int n, bool& updated) {
    const bool full = n == 2 * NP;
    f32x2 ms[NP], vs[NP], q[NP];
#pragma unroll
    for (int u = 0; u < NP; ++u) {
        if (u > 0 || !updated) {
            m = m + c.one_minus_b1 * (0.0f - m);
            v = v * c.b2;
        }
        ms[u].x = m;
        vs[u].x = v;
        if (u + 1 < NP || full) {
            m = m + c.one_minus_b1 * (0.0f - m);
            v = v * c.b2;
        }
        ms[u].y = m;
        vs[u].y = v;
    }
    updated = false;
#pragma unroll
    for (int u = 0; u < NP; ++u)
        q[u] = chain_quot_ordinary<UNIT_BC2>(ms[u], vs[u], c, s + 2 * u, u + 1 < NP || full ? s + 2 * u + 1 : s + 2 * u);
#pragma unroll
    for (int u = 0; u < NP; ++u) {
        p = p + q[u].x;
        if (u + 1 < NP || full) p = p + q[u].y;
    }
}

// ordinary_run: CHAIN_G pairs (2 CHAIN_G updates) side by side while that many are left, then what is left as ONE narrower
// group; a single update takes the scalar chain.  (4: the step kernel's five rows no longer stay in registers)
constexpr int CHAIN_G = 2;
static_assert(CHAIN_G == 2 || CHAIN_G == 4, "chain_ordinary_run spells out the groups of one to four pairs");

template <bool UNIT_BC2>
__device__ __forceinline__ void chain_ordinary_run(float& p, float& m, float& v, const AdamChainArgs& c, int& s, int s_to, bool& updated) {
    while (s_to - s >= 2 * CHAIN_G - 1) {
        const int n = s_to - s < 2 * CHAIN_G ? s_to - s : 2 * CHAIN_G;
        chain_ordinary_group<UNIT_BC2, CHAIN_G>(p, m, v, c, s, n, updated);
        s += n;
    }
    const int n = s_to - s;
    if (n <= 0) return;
    if (n == 1) {
        if (!updated) {
            m = m + c.one_minus_b1 * (0.0f - m);
            v = v * c.b2;
        }
        updated = false;
        p = p + chain_quot_ordinary<UNIT_BC2>(m, v, c, s);
    } else if (n <= 2) {
        chain_ordinary_group<UNIT_BC2, 1>(p, m, v, c, s, n, updated);
    } else if (CHAIN_G > 2 && n <= 4) {
        chain_ordinary_group<UNIT_BC2, 2>(p, m, v, c, s, n, updated);
    } else if (CHAIN_G > 2) {
        chain_ordinary_group<UNIT_BC2, 3>(p, m, v, c, s, n, updated);
    }
    s = s_to;
}

// fast_run: the updates below first_unit on the non-unit form, the others on the unit form (a run is all of one kind
// except, once, around step 16 600: then the first loop hands over to the second where bc2_sqrt turns 1.0f)
__device__ __forceinline__ void chain_fast_run(float& p, float& m, float& v, const AdamChainArgs& c, int s, int s_to, bool updated) {
    chain_ordinary_run<false>(p, m, v, c, s, s_to < c.first_unit ? s_to : c.first_unit, updated);
    chain_ordinary_run<true>(p, m, v, c, s, s_to, updated);
}

// one update's general quotient from the updated moments (the last line of adam_elem / adam_elem_unit_bc2)
__device__ __forceinline__ float chain_quot_general(float m, float v, const AdamChainArgs& c, int s) {
    const float nss = lane_scalar(c.t_nss, s), bc2 = lane_scalar(c.t_bc2, s);
    return s >= c.first_unit ? adam_quot<true>(m, v, nss, bc2, c.eps) : adam_quot<false>(m, v, nss, bc2, c.eps);
}

// adam_zero_run.  Returns the class the wavefront took (FC_REST / FC_ORD / FC_GENERAL), -1 for an empty run
__device__ __forceinline__ int chain_zero_run(float& p, float& m, float& v, const AdamChainArgs& c, int s, int s_to, int ck) {
    if (s >= s_to) return -1;
    if (__builtin_amdgcn_ballot_w64(!lane_at_rest(p, m, v, lane_scalar(c.t_bound, s), c)) == 0) {
        fused_count(c, ck, FC_RUN, FC_REST);
        for (; s < s_to; ++s) {
            m = m + c.one_minus_b1 * (0.0f - m);
            v = v * c.b2;
        }
        return FC_REST;
    }
    if (__builtin_amdgcn_ballot_w64(!lane_ordinary(m, v, c)) == 0) {
        fused_count(c, ck, FC_RUN, FC_ORD);
        chain_fast_run(p, m, v, c, s, s_to, false);
        return FC_ORD;
    }
    fused_count(c, ck, FC_RUN, FC_GENERAL);
    for (; s < s_to; ++s) {
        adam_moments(0.0f, m, v, c);
        p = p + chain_quot_general(m, v, c, s);
    }
    return FC_GENERAL;
}

// adam_grad_run.  Returns FC_ORD when the wavefront took the scaling-free evaluation, FC_GENERAL otherwise
__device__ __forceinline__ int chain_grad_run(float& p, float g, float& m, float& v, const AdamChainArgs& c, int s, int s_to, int ck) {
    adam_moments(g, m, v, c);
    if (__builtin_amdgcn_ballot_w64(!lane_ordinary(m, v, c)) == 0) {
        fused_count(c, ck, FC_GRAD, FC_ORD);
        if (s + 1 < s_to) fused_count(c, ck, FC_RUN, FC_ORD);
        chain_fast_run(p, m, v, c, s, s_to, true);
        return FC_ORD;
    }
    fused_count(c, ck, FC_GRAD, FC_GENERAL);
    p = p + chain_quot_general(m, v, c, s);
    chain_zero_run(p, m, v, c, s + 1, s_to, ck);
    return FC_GENERAL;
}

// fused_advance (bpr_fused.hip) on the lane tables: prev1 > 0: index prev1 - 1 with gradient g, then the zero-gradient indices
// [prev1, s_to);  prev1 == 0: the zero-gradient indices [s_from, s_to) only
struct AdamRowState {
    float p, m, v;
    int cls;      // what chain_grad_run / chain_zero_run returned
};

__device__ __forceinline__ AdamRowState chain_advance(float p, float g, float m, float v, int prev1, int s_from, int s_to, int ck,
                                                      const AdamChainArgs& c) {
    AdamRowState r{p, m, v, -1};
    if (prev1 > 0)
        r.cls = chain_grad_run(r.p, g, r.m, r.v, c, prev1 - 1, s_to, ck);
    else
        r.cls = chain_zero_run(r.p, r.m, r.v, c, s_from, s_to, ck);
    return r;
}

// ---- host side -------------------------------------------------------------------------------------------------
// SKR_COLD_STATS=1: the device census of how the cold passes sorted their blocks (8 counters), or NULL (defined in adam.hip)
__attribute__((visibility("hidden"))) unsigned long long* cold_stats_buffer(bool reread = false);
// SKR_FUSED_STATS=1: the census of the lazy rows' evaluations (FC_COUNTERS counters), or NULL (defined in adam.hip)
__attribute__((visibility("hidden"))) unsigned long long* fused_stats_buffer(bool reread = false);

// the fields every step of a run shares (A: AdamArgs or AdamBlockArgs)
template <class A>
static inline void adam_shared_fields(A& a, float beta1, float beta2, float eps) {
    a.one_minus_b1 = static_cast<float>(1.0 - static_cast<double>(beta1));
    a.b2 = beta2;
    a.one_minus_b2 = static_cast<float>(1.0 - static_cast<double>(beta2));
    a.eps = eps;
}

static inline void adam_scalars(float lr, float beta1, float beta2, int64_t step_t, float* neg_step_size, float* bc2_sqrt, bool tf = false) {
    // torch/optim/adam.py _single_tensor_adam: python-double scalars, cast to fp32 at the tensor ops
    const double b1 = static_cast<double>(beta1), b2 = static_cast<double>(beta2);
    const double bc1 = 1.0 - std::pow(b1, static_cast<double>(step_t));
    const double bc2 = 1.0 - std::pow(b2, static_cast<double>(step_t));
    if (tf) {
        // tf.train.AdamOptimizer (GRU4RecPlus.py:192): p -= lr_t * m / (sqrt(v) + eps), lr_t = lr * sqrt(1 - b2^t) / (1 - b1^t):
        // the second bias correction sits in the step size, the denominator has none
        *neg_step_size = static_cast<float>(-(static_cast<double>(lr) * std::sqrt(bc2) / bc1));
        *bc2_sqrt = 1.0f;
        return;
    }
    *neg_step_size = static_cast<float>(-(static_cast<double>(lr) / bc1));
    *bc2_sqrt = static_cast<float>(std::sqrt(bc2));
}

// the k steps' scalars of a block that starts after step_t0, and the running maximum the at-rest tests use
static inline void adam_block_scalars(AdamBlockArgs& a, float lr, float beta1, float beta2, int64_t step_t0, int k, bool tf) {
    for (int s = 0; s < k; ++s) adam_scalars(lr, beta1, beta2, step_t0 + 1 + s, &a.neg_step_size[s], &a.bc2_sqrt[s], tf);
    float mx = 0.0f;
    for (int s = k - 1; s >= 0; --s) {
        mx = std::fmax(mx, std::fabs(a.neg_step_size[s]));
        a.nss_bound[s] = mx;
    }
    // sqrt(1 - beta2^t) rises with t and stays at 1.0f once it gets there (TF's is 1.0f throughout): the forms that choose
    // between the unit and the non-unit quotient by `s >= first_unit` rely on it
    a.first_unit = k;
    for (int s = 0; s < k; ++s) {
        if (a.bc2_sqrt[s] == 1.0f && a.first_unit == k) a.first_unit = s;
        assert((s >= a.first_unit) == (a.bc2_sqrt[s] == 1.0f) && "bc2_sqrt left 1.0f again");
    }
}

// thresholds of the at-rest / ordinary-magnitude tests for a run of up to k zero-gradient updates whose scalars sit in
// a.neg_step_size[0 .. k-1] / a.bc2_sqrt[0 .. k-1] (|neg_step_size| falls, bc2_sqrt rises with the step)
static inline void adam_block_thresholds(AdamBlockArgs& a, float lr, float beta1, float beta2, float eps, int k) {
    const bool sane = beta1 > 0.0f && beta1 < 1.0f && beta2 > 0.0f && beta2 < 1.0f && lr > 0.0f && eps >= 0.0f &&
                      std::isfinite(lr) && std::isfinite(eps);
    a.rest_eps = sane ? eps * 0x1p-28f : 0.0f;
    a.rest_b2k = sane ? static_cast<float>(std::pow(static_cast<double>(beta2), k) * (1.0 - 1e-4)) : 0.0f;
    // ordinary magnitudes for all k updates (ranges of sqrt_ordinary / div_ordinary with room to spare): v in
    // [2^-90, 2^20] throughout, |nss*m| in [2^-100, 2^40] throughout, eps <= 2^20, sqrt(1 - beta2^t) >= 2^-10
    double nss_max = 0.0, nss_min = INFINITY;      // torch's scalars: the first and the last step's; TF's are not monotone
    for (int s_ = 0; s_ < k; ++s_) {
        nss_max = std::fmax(nss_max, std::fabs(static_cast<double>(a.neg_step_size[s_])));
        nss_min = std::fmin(nss_min, std::fabs(static_cast<double>(a.neg_step_size[s_])));
    }
    const double m_lo = 0x1p-100 / (nss_min * std::pow(static_cast<double>(beta1), k) * 0.99), m_hi = 0x1p40 / nss_max;
    const bool ord = sane && eps <= 0x1p20f && a.bc2_sqrt[0] >= 0x1p-10f && a.rest_b2k > 0.0f && m_lo < 1e30 && m_hi > 1e-30 &&
                     std::isfinite(m_lo) && std::isfinite(m_hi);
    a.fast_vlo = ord ? static_cast<float>(0x1p-90 / static_cast<double>(a.rest_b2k)) : 0.0f;
    a.fast_mlo = ord ? static_cast<float>(m_lo) : INFINITY;
    a.fast_mhi = ord ? static_cast<float>(std::fmin(m_hi, 1e38)) : 0.0f;
}

}  // namespace skr
