// cdae.hip -- CDAE, the collaborative denoising autoencoder (reference: recommender/CDAE.py:95-130,168-206).
//
// A training step works on a ragged pair list: user b of the batch owns the pairs [uptr[b], uptr[b + 1]), its
// positives and its de-duplicated negatives in ascending item order, each with a label bit and a dropout keep flag.
// The same pairs are listed a second time item-major: distinct item j of the batch owns ipair[iptr[j] .. iptr[j + 1]).
// Three launches, no floating-point atomic, every sum in a fixed order:
//   user side   one wavefront per user: h = act(sum_kept E_en[i] / keep_prob + U[u] + offset), per pair the logit
//               r = <h, E_de[i]> + b[i] and dr = sigmoid(r) - y, dh = sum dr E_de[i], dpre = dh act'(h); writes dU[u],
//               and h, dpre, dr, the user's BCE sum and 0.5 |U[u]|^2 to the workspace
//   item side   one wavefront per distinct item walks its pairs: dE_de[i] = sum dr h_u + reg E_de[i],
//               db[i] = sum dr + reg b[i], dE_en[i] = sum_kept dpre_u / keep_prob + reg E_en[i]; 0.5 of the three squares
//   finish      one workgroup: d offset = sum_u dpre_u + reg offset, and the two loss words
// What is skipped contributes nothing: a user out of range or behind a broken pointer owns no pairs (user_pairs, read by
// both sides, so the item side follows a pair only where the user side wrote its dr), a pair whose item is out of range
// is skipped alone, and an item none of whose pairs is followed gets no row and no l2 term.
// Rows are 64 floats (256 bytes).  A wavefront reads them as four rows side by side: 16 lanes x float4 per row, so one
// load instruction has four rows in flight; the four partial sums are combined at the end, (g0 + g1) + (g2 + g3).
// Columns beyond `dim` are held at zero: h is masked there (sigmoid(0) would put 0.5 into them).
// Gradient rows are WRITTEN, not added to: the rows a batch does not name stay as the optimiser left them (zero).
#include "skr_common.h"
#include "fast_rng.h"
#include "mfma_tile.h"
#include "step_common.h"

#include <cmath>

namespace {

using namespace skr;

constexpr int D = 64;
constexpr int HW = 4;          // wavefronts per workgroup: item side (thousands of distinct items) and queries
#ifndef SKR_CDAE_UW
#define SKR_CDAE_UW 1
#endif
constexpr int UW = SKR_CDAE_UW;  // user side: a batch is a few hundred long rows, so one wavefront per workgroup spreads
                                 // them over the compute units (256 users -> 256 workgroups, not 64)

__device__ __forceinline__ float4 row4(const float* __restrict__ T, int64_t row, int c4) {
    return reinterpret_cast<const float4*>(T)[row * 16 + c4];
}
__device__ __forceinline__ void put4(float* __restrict__ T, int64_t row, int c4, const float4& v) {
    reinterpret_cast<float4*>(T)[row * 16 + c4] = v;
}
__device__ __forceinline__ float4 add4(const float4& a, const float4& b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float4 fma4(float s, const float4& a, const float4& b) {
    return make_float4(fmaf(s, a.x, b.x), fmaf(s, a.y, b.y), fmaf(s, a.z, b.z), fmaf(s, a.w, b.w));
}
__device__ __forceinline__ float dot4(const float4& a, const float4& b) { return fmaf(a.w, b.w, fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x))); }
// the four row groups' partial sums: (g0 + g1) + (g2 + g3) in every lane
__device__ __forceinline__ float groups(float v) {
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}
__device__ __forceinline__ float4 groups4(const float4& v) { return make_float4(groups(v.x), groups(v.y), groups(v.z), groups(v.w)); }
// columns 4 c4 .. 4 c4 + 3 beyond dim become zero
__device__ __forceinline__ float4 mask4(const float4& v, int c4, int dim) {
    const int c = 4 * c4;
    return make_float4(c < dim ? v.x : 0.0f, c + 1 < dim ? v.y : 0.0f, c + 2 < dim ? v.z : 0.0f, c + 3 < dim ? v.w : 0.0f);
}
__device__ __forceinline__ float sigmoidf(float x) { return 1.0f / (1.0f + expf(-x)); }
template <int ACT>
__device__ __forceinline__ float4 act4(const float4& v) {
    if (ACT == 0) return v;
    return make_float4(sigmoidf(v.x), sigmoidf(v.y), sigmoidf(v.z), sigmoidf(v.w));
}

// sum of v over the workgroup's threads in a fixed order (a tree over the thread index); the result in thread 0
__device__ __forceinline__ float block_sum(float v, float* s) {
    const int t = threadIdx.x;
    s[t] = v;
    __syncthreads();
    for (int o = blockDim.x >> 1; o > 0; o >>= 1) {
        if (t < o) s[t] += s[t + o];
        __syncthreads();
    }
    const float r = s[0];
    __syncthreads();
    return r;
}

struct Work {                  // float offsets into the workspace
    int64_t h, dpre, dr, bce, l2u, l2i, total;
};
inline Work work_layout(int n, int64_t n_pairs) {
    Work w;
    int64_t o = 0;
    w.h = o; o += static_cast<int64_t>(n) * D;
    w.dpre = o; o += static_cast<int64_t>(n) * D;
    w.dr = o; o += round4(n_pairs);
    w.bce = o; o += round4(n);
    w.l2u = o; o += round4(n);
    w.l2i = o; o += round4(n_pairs);
    w.total = o;
    return w;
}

// The pairs [p0, p1) that batch position b owns, as the user side walks them and the item side follows them: empty for a
// user outside [0, n_users) and for a broken pointer (below the batch's first pair, descending, or past n_pairs), so
// that the item side never reads a dr the user side did not write.
__device__ __forceinline__ void user_pairs(const int32_t* __restrict__ users, const int32_t* __restrict__ uptr, int b,
                                           int64_t pair0, int64_t n_pairs, int n_users, int64_t& p0, int64_t& p1) {
    p0 = uptr[b];
    p1 = uptr[b + 1];
    const int u = users[b];
    if (u < 0 || u >= n_users || p0 < pair0 || p1 < p0 || p1 - pair0 > n_pairs) p0 = p1 = pair0;
}

// ------------------------------------------------------------------------------------------------
// user side
// ------------------------------------------------------------------------------------------------
template <int ACT>
__global__ __launch_bounds__(UW * 64) void cdae_user_kernel(
    const float* __restrict__ E_en, const float* __restrict__ E_de, const float* __restrict__ bias,
    const float* __restrict__ offset, const float* __restrict__ U, const int32_t* __restrict__ users,
    const int32_t* __restrict__ uptr, const int32_t* __restrict__ pitem, const uint8_t* __restrict__ plabel,
    const uint8_t* __restrict__ pkeep, int n, int64_t n_pairs, int n_users, int n_items, int dim, float inv_keep, float reg,
    float* __restrict__ gU, float* __restrict__ h_ws, float* __restrict__ dpre_ws, float* __restrict__ dr_ws,
    float* __restrict__ bce_ws, float* __restrict__ l2u_ws) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int b = blockIdx.x * UW + wv;
    if (b >= n) return;
    const int g = lane >> 4, c4 = lane & 15;
    const int64_t pair0 = uptr[0];
    int64_t p0, p1;
    user_pairs(users, uptr, b, pair0, n_pairs, n_users, p0, p1);           // a skipped user, a broken pointer: an empty row
    const int u = users[b];
    const bool valid = u >= 0 && u < n_users;                              // a skipped user: no U row, no l2, no gradient
    const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    // encoder: the kept rows of E_en
    float4 acc = zero;
#pragma unroll 2
    for (int64_t p = p0 + g; p < p1; p += 4) {
        const int it = pitem[p];
        if (pkeep[p] != 0 && it >= 0 && it < n_items) acc = add4(acc, row4(E_en, it, c4));
    }
    acc = groups4(acc);
    const float4 urow = valid ? row4(U, u, c4) : zero;
    const float4 off = row4(offset, 0, c4);
    float4 pre = make_float4(fmaf(acc.x, inv_keep, urow.x) + off.x, fmaf(acc.y, inv_keep, urow.y) + off.y,
                             fmaf(acc.z, inv_keep, urow.z) + off.z, fmaf(acc.w, inv_keep, urow.w) + off.w);
    const float4 h = mask4(act4<ACT>(pre), c4, dim);
    // decoder: every pair, kept or dropped
    float4 dh = zero;
    float bce = 0.0f;
#pragma unroll 2
    for (int64_t p = p0 + g; p < p1; p += 4) {
        const int it = pitem[p];
        float dr = 0.0f;
        if (it >= 0 && it < n_items) {
            const float4 e = row4(E_de, it, c4);
            const float r = sum16(dot4(h, e)) + bias[it];
            const bool pos = plabel[p] != 0;
            // binary_cross_entropy_with_logits: max(r, 0) - r y + log(1 + exp(-|r|)); its derivative sigmoid(r) - y, for
            // y = 1 as -sigmoid(-r) (no cancellation at large r)
            bce += fmaxf(r, 0.0f) - (pos ? r : 0.0f) + log1pf(expf(-fabsf(r)));
            dr = pos ? -sigmoidf(-r) : sigmoidf(r);
            dh = fma4(dr, e, dh);
        }
        if (c4 == 0) dr_ws[p - pair0] = dr;
    }
    dh = groups4(dh);
    bce = groups(bce);
    float4 dpre = dh;
    if (ACT == 1) dpre = make_float4(dh.x * (h.x * (1.0f - h.x)), dh.y * (h.y * (1.0f - h.y)), dh.z * (h.z * (1.0f - h.z)), dh.w * (h.w * (1.0f - h.w)));
    dpre = mask4(dpre, c4, dim);
    const float l2u = sum16(dot4(urow, urow));
    if (g == 0) {
        put4(h_ws, b, c4, h);
        put4(dpre_ws, b, c4, dpre);
        if (valid) put4(gU, u, c4, fma4(reg, urow, dpre));
        if (c4 == 0) {
            bce_ws[b] = bce;
            l2u_ws[b] = 0.5f * l2u;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// item side
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(HW * 64) void cdae_item_kernel(
    const float* __restrict__ E_en, const float* __restrict__ E_de, const float* __restrict__ bias,
    const int32_t* __restrict__ users, const int32_t* __restrict__ uptr, const int32_t* __restrict__ pitem,
    const uint8_t* __restrict__ pkeep, const int32_t* __restrict__ puser, const int32_t* __restrict__ ditems,
    const int32_t* __restrict__ iptr, const int32_t* __restrict__ ipair, int n, int64_t n_pairs, int n_distinct, int n_users,
    int n_items, float inv_keep, float reg, const float* __restrict__ h_ws,
    const float* __restrict__ dpre_ws, const float* __restrict__ dr_ws, float* __restrict__ gE_en, float* __restrict__ gE_de,
    float* __restrict__ gbias, float* __restrict__ l2i_ws) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int j = blockIdx.x * HW + wv;
    if (j >= n_distinct) return;
    const int g = lane >> 4, c4 = lane & 15;
    const int64_t pair0 = uptr[0], q00 = iptr[0];
    int64_t q0 = iptr[j], q1 = iptr[j + 1];
    if (q0 < q00 || q1 < q0 || q1 - q00 > n_pairs) q0 = q1 = q00;
    const int it = ditems[j];
    const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float4 ad = zero, ae = zero;
    float ab = 0.0f;
    bool named = false;
#pragma unroll 2
    for (int64_t q = q0 + g; q < q1; q += 4) {
        const int64_t lp = ipair[q];
        if (lp < 0 || lp >= n_pairs) continue;
        const int b = puser[pair0 + lp];
        if (b < 0 || b >= n) continue;
        // A pair is followed only where the user side wrote its dr: it is a pair of this item inside its owner's range.
        // Everything is requested before the test (all of it lies inside the arrays): the test adds no round trip.
        int64_t p0, p1;
        user_pairs(users, uptr, b, pair0, n_pairs, n_users, p0, p1);
        const bool mine = pitem[pair0 + lp] == it;
        const bool kept = pkeep[pair0 + lp] != 0;
        const float dr = dr_ws[lp];
        const float4 hb = row4(h_ws, b, c4), db = row4(dpre_ws, b, c4);
        if (!mine || pair0 + lp < p0 || pair0 + lp >= p1) continue;
        named = true;
        ad = fma4(dr, hb, ad);
        ab += dr;
        if (kept) ae = add4(ae, db);
    }
    ad = groups4(ad);
    ae = groups4(ae);
    ab = groups(ab);
    named = __builtin_amdgcn_ballot_w64(named) != 0;      // an item none of whose pairs is followed is not named by the batch
    float l2 = 0.0f;
    if (it >= 0 && it < n_items && named) {
        const float4 en = row4(E_en, it, c4), de = row4(E_de, it, c4);
        const float bi = bias[it];
        l2 = 0.5f * (sum16(dot4(en, en)) + sum16(dot4(de, de)) + bi * bi);
        if (g == 0) {
            put4(gE_de, it, c4, fma4(reg, de, ad));
            put4(gE_en, it, c4, make_float4(fmaf(ae.x, inv_keep, reg * en.x), fmaf(ae.y, inv_keep, reg * en.y),
                                            fmaf(ae.z, inv_keep, reg * en.z), fmaf(ae.w, inv_keep, reg * en.w)));
            if (c4 == 0) gbias[it] = fmaf(reg, bi, ab);
        }
    }
    if (lane == 0) l2i_ws[j] = l2;
}

// ------------------------------------------------------------------------------------------------
// finish: the offset's gradient and the loss words
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void cdae_finish_kernel(const float* __restrict__ offset, int n, int n_distinct, float reg,
                                                           const float* __restrict__ dpre_ws, const float* __restrict__ bce_ws,
                                                           const float* __restrict__ l2u_ws, const float* __restrict__ l2i_ws,
                                                           float* __restrict__ goffset, float* __restrict__ loss) {
    __shared__ float s[1024];
    const int t = threadIdx.x, c = t & 63, part = t >> 6;
    float a = 0.0f;
    for (int b = part; b < n; b += 16) a += dpre_ws[static_cast<int64_t>(b) * D + c];
    s[t] = a;
    __syncthreads();
    const float o = offset[c];
    if (t < D) {
        float v = 0.0f;
        for (int k = 0; k < 16; ++k) v += s[k * 64 + t];
        goffset[t] = fmaf(reg, o, v);
    }
    __syncthreads();
    float bce = 0.0f, l2 = t < D ? 0.5f * o * o : 0.0f;
    for (int b = t; b < n; b += 1024) {
        bce += bce_ws[b];
        l2 += l2u_ws[b];
    }
    for (int j = t; j < n_distinct; j += 1024) l2 += l2i_ws[j];
    bce = block_sum(bce, s);
    l2 = block_sum(l2, s);
    if (t == 0) {
        loss[0] = bce;
        loss[1] = l2;
    }
}

// query rows: Q[u] = act(sum E_en[train(u)] + U[u] + offset), no negatives, no dropout (CDAE.py:126-130)
template <int ACT>
__global__ __launch_bounds__(HW * 64) void cdae_queries_kernel(const float* __restrict__ E_en, const float* __restrict__ offset,
                                                               const float* __restrict__ U, const int64_t* __restrict__ rowptr,
                                                               const int32_t* __restrict__ items, const int32_t* __restrict__ users,
                                                               int n, int n_users, int n_items, int dim, float* __restrict__ Q) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, g = lane >> 4, c4 = lane & 15;
    const float4 off = row4(offset, 0, c4);
    for (int b = blockIdx.x * HW + wv; b < n; b += gridDim.x * HW) {
        const int64_t u = users ? users[b] : b;
        if (u < 0 || u >= n_users) continue;
        const int64_t beg = rowptr[u], end = rowptr[u + 1];
        float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll 2
        for (int64_t p = beg + g; p < end; p += 4) {
            const int it = items[p];
            if (it >= 0 && it < n_items) acc = add4(acc, row4(E_en, it, c4));
        }
        acc = groups4(acc);
        const float4 ur = row4(U, u, c4);
        const float4 pre = make_float4((acc.x + ur.x) + off.x, (acc.y + ur.y) + off.y, (acc.z + ur.z) + off.z, (acc.w + ur.w) + off.w);
        if (g == 0) put4(Q, u, c4, mask4(act4<ACT>(pre), c4, dim));
    }
}

// keep flags of a pair list on the device: pair p of batch position puser[p] is keyed by (seed, step, user, item)
__global__ __launch_bounds__(256) void cdae_draws_kernel(const int32_t* __restrict__ users, const int32_t* __restrict__ puser,
                                                         const int32_t* __restrict__ pitem, const int32_t* __restrict__ pstep,
                                                         int64_t n_pairs, int n, float keep_prob, uint64_t seed, uint64_t step,
                                                         uint8_t* __restrict__ pkeep) {
    const int64_t p = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
    if (p >= n_pairs) return;
    const int b = puser[p];
    uint8_t k = 0;
    if (b >= 0 && b < n) k = keep_draw(seed, step + (pstep ? static_cast<uint64_t>(pstep[p]) : 0ull), users[b], pitem[p], keep_prob) ? 1 : 0;
    pkeep[p] = k;
}

}  // namespace

extern "C" {

size_t skr_cdae_workspace(int n, int64_t n_pairs) {
    if (n <= 0 || n > SKR_CDAE_MAX_BATCH || n_pairs < 0) return 0;
    return static_cast<size_t>(work_layout(n, n_pairs).total) * sizeof(float);
}

static int cdae_run_step(const float* d_E_en, const float* d_E_de, const float* d_bias, const float* d_offset, const float* d_U,
                         const int32_t* d_users, const int32_t* d_uptr, const int32_t* d_pitem, const uint8_t* d_plabel,
                         const uint8_t* d_pkeep, const int32_t* d_puser, const int32_t* d_ditems, const int32_t* d_iptr,
                         const int32_t* d_ipair, int n, int64_t n_pairs, int n_distinct, int n_users, int n_items, int dim, int act,
                         float keep_prob, float reg, float* d_gE_en, float* d_gE_de, float* d_gbias, float* d_goffset, float* d_gU,
                         void* d_work, size_t work_bytes, float* d_loss, void* stream, float* h_ms) {
    SKR_REQUIRE(d_E_en && d_E_de && d_bias && d_offset && d_U && d_users && d_uptr && d_pitem && d_plabel && d_pkeep && d_puser &&
                    d_ditems && d_iptr && d_ipair && d_gE_en && d_gE_de && d_gbias && d_goffset && d_gU && d_work && d_loss,
                "skr_cdae_step: NULL argument");
    SKR_REQUIRE(n >= 0 && n <= SKR_CDAE_MAX_BATCH && n_users > 0 && n_items > 0,
                "skr_cdae_step: n = %d (at most %d), n_users = %d, n_items = %d", n, SKR_CDAE_MAX_BATCH, n_users, n_items);
    SKR_REQUIRE(n_pairs >= 0 && n_pairs < (1ll << 31) && n_distinct >= 0 && n_distinct <= n_pairs,
                "skr_cdae_step: n_pairs = %lld, n_distinct = %d", static_cast<long long>(n_pairs), n_distinct);
    SKR_REQUIRE(dim >= 1 && dim <= D, "skr_cdae_step: 1 <= dim <= 64 (got %d); rows are 64 floats, zero-padded", dim);
    SKR_REQUIRE(act == SKR_CDAE_IDENTITY || act == SKR_CDAE_SIGMOID, "skr_cdae_step: act = %d is neither identity nor sigmoid", act);
    SKR_REQUIRE(keep_prob > 0.0f && keep_prob <= 1.0f, "skr_cdae_step: keep_prob = %g is not in (0, 1]", keep_prob);
    if (n == 0) {                                   // the empty batch: both loss words are written, nothing else is touched
        SKR_HIP(hipMemsetAsync(d_loss, 0, 2 * sizeof(float), skr::as_stream(stream)));
        return SKR_OK;
    }
    const Work W = work_layout(n, n_pairs);
    SKR_REQUIRE(work_bytes >= static_cast<size_t>(W.total) * sizeof(float),
                "skr_cdae_step: d_work holds %zu bytes, skr_cdae_workspace(%d, %lld) asks for %zu", work_bytes, n,
                static_cast<long long>(n_pairs), static_cast<size_t>(W.total) * sizeof(float));
    SKR_REQUIRE(((reinterpret_cast<uintptr_t>(d_E_en) | reinterpret_cast<uintptr_t>(d_E_de) | reinterpret_cast<uintptr_t>(d_offset) |
                  reinterpret_cast<uintptr_t>(d_U) | reinterpret_cast<uintptr_t>(d_gE_en) | reinterpret_cast<uintptr_t>(d_gE_de) |
                  reinterpret_cast<uintptr_t>(d_gU) | reinterpret_cast<uintptr_t>(d_work)) & 15) == 0,
                "skr_cdae_step: tables, gradients and d_work must be 16-byte aligned");
    float* w = static_cast<float*>(d_work);
    hipStream_t st = skr::as_stream(stream);
    const float inv_keep = 1.0f / keep_prob;
    StepTimer<SKR_CDAE_LAUNCHES + 1> mk(h_ms, st);     // h_ms: an event after every launch; otherwise nothing
    SKR_HIP(mk.mark());
#define SKR_CDAE_USER(A_)                                                                                                         \
    hipLaunchKernelGGL(cdae_user_kernel<A_>, dim3((n + UW - 1) / UW), dim3(UW * 64), 0, st, d_E_en, d_E_de, d_bias, d_offset, d_U, \
                       d_users, d_uptr, d_pitem, d_plabel, d_pkeep, n, n_pairs, n_users, n_items, dim, inv_keep, reg, d_gU,       \
                       w + W.h, w + W.dpre, w + W.dr, w + W.bce, w + W.l2u)
    if (act == SKR_CDAE_SIGMOID) SKR_CDAE_USER(1); else SKR_CDAE_USER(0);
#undef SKR_CDAE_USER
    SKR_HIP(mk.mark());
    if (n_distinct > 0)
        hipLaunchKernelGGL(cdae_item_kernel, dim3((n_distinct + HW - 1) / HW), dim3(HW * 64), 0, st, d_E_en, d_E_de, d_bias, d_users,
                           d_uptr, d_pitem, d_pkeep, d_puser, d_ditems, d_iptr, d_ipair, n, n_pairs, n_distinct, n_users, n_items,
                           inv_keep, reg, w + W.h,
                           w + W.dpre, w + W.dr, d_gE_en, d_gE_de, d_gbias, w + W.l2i);
    SKR_HIP(mk.mark());
    hipLaunchKernelGGL(cdae_finish_kernel, dim3(1), dim3(1024), 0, st, d_offset, n, n_distinct, reg, w + W.dpre, w + W.bce,
                       w + W.l2u, w + W.l2i, d_goffset, d_loss);
    SKR_HIP(mk.mark());
    SKR_LAUNCH_CHECK();
    SKR_HIP(mk.finish());
    return SKR_OK;
}

int skr_cdae_step(const float* d_E_en, const float* d_E_de, const float* d_bias, const float* d_offset, const float* d_U,
                  const int32_t* d_users, const int32_t* d_uptr, const int32_t* d_pitem, const uint8_t* d_plabel,
                  const uint8_t* d_pkeep, const int32_t* d_puser, const int32_t* d_ditems, const int32_t* d_iptr,
                  const int32_t* d_ipair, int n, int64_t n_pairs, int n_distinct, int n_users, int n_items, int dim, int act,
                  float keep_prob, float reg, float* d_gE_en, float* d_gE_de, float* d_gbias, float* d_goffset, float* d_gU,
                  void* d_work, size_t work_bytes, float* d_loss, void* stream) {
    return cdae_run_step(d_E_en, d_E_de, d_bias, d_offset, d_U, d_users, d_uptr, d_pitem, d_plabel, d_pkeep, d_puser, d_ditems, d_iptr,
                         d_ipair, n, n_pairs, n_distinct, n_users, n_items, dim, act, keep_prob, reg, d_gE_en, d_gE_de, d_gbias,
                         d_goffset, d_gU, d_work, work_bytes, d_loss, stream, nullptr);
}

int skr_cdae_step_timed(const float* d_E_en, const float* d_E_de, const float* d_bias, const float* d_offset, const float* d_U,
                        const int32_t* d_users, const int32_t* d_uptr, const int32_t* d_pitem, const uint8_t* d_plabel,
                        const uint8_t* d_pkeep, const int32_t* d_puser, const int32_t* d_ditems, const int32_t* d_iptr,
                        const int32_t* d_ipair, int n, int64_t n_pairs, int n_distinct, int n_users, int n_items, int dim, int act,
                        float keep_prob, float reg, float* d_gE_en, float* d_gE_de, float* d_gbias, float* d_goffset, float* d_gU,
                        void* d_work, size_t work_bytes, float* d_loss, void* stream, float* h_ms) {
    SKR_REQUIRE(h_ms != nullptr, "skr_cdae_step_timed: NULL argument");
    return cdae_run_step(d_E_en, d_E_de, d_bias, d_offset, d_U, d_users, d_uptr, d_pitem, d_plabel, d_pkeep, d_puser, d_ditems, d_iptr,
                         d_ipair, n, n_pairs, n_distinct, n_users, n_items, dim, act, keep_prob, reg, d_gE_en, d_gE_de, d_gbias,
                         d_goffset, d_gU, d_work, work_bytes, d_loss, stream, h_ms);
}

int skr_cdae_queries(const float* d_E_en, const float* d_offset, const float* d_U, const int64_t* d_rowptr, const int32_t* d_items,
                     const int32_t* d_users, int n, int n_users, int n_items, int dim, int act, float* d_Q, void* stream) {
    SKR_REQUIRE(d_E_en && d_offset && d_U && d_rowptr && d_items && d_Q, "skr_cdae_queries: NULL argument");
    SKR_REQUIRE(n >= 0 && n_users > 0 && n_items > 0, "skr_cdae_queries: n = %d, n_users = %d, n_items = %d", n, n_users, n_items);
    SKR_REQUIRE(d_users || n <= n_users, "skr_cdae_queries: without a user list n = %d must not exceed n_users = %d", n, n_users);
    SKR_REQUIRE(dim >= 1 && dim <= D, "skr_cdae_queries: 1 <= dim <= 64 (got %d)", dim);
    SKR_REQUIRE(act == SKR_CDAE_IDENTITY || act == SKR_CDAE_SIGMOID, "skr_cdae_queries: act = %d is neither identity nor sigmoid", act);
    SKR_REQUIRE(((reinterpret_cast<uintptr_t>(d_E_en) | reinterpret_cast<uintptr_t>(d_offset) | reinterpret_cast<uintptr_t>(d_U) |
                  reinterpret_cast<uintptr_t>(d_Q)) & 15) == 0, "skr_cdae_queries: tables and d_Q must be 16-byte aligned");
    if (n == 0) return SKR_OK;
    int blocks = (n + HW - 1) / HW;
    if (blocks > 8192) blocks = 8192;
    if (act == SKR_CDAE_SIGMOID)
        hipLaunchKernelGGL(cdae_queries_kernel<1>, dim3(blocks), dim3(HW * 64), 0, skr::as_stream(stream), d_E_en, d_offset, d_U,
                           d_rowptr, d_items, d_users, n, n_users, n_items, dim, d_Q);
    else
        hipLaunchKernelGGL(cdae_queries_kernel<0>, dim3(blocks), dim3(HW * 64), 0, skr::as_stream(stream), d_E_en, d_offset, d_U,
                           d_rowptr, d_items, d_users, n, n_users, n_items, dim, d_Q);
    SKR_LAUNCH_CHECK();
    return SKR_OK;
}

int skr_cdae_draws(const int32_t* d_users, const int32_t* d_puser, const int32_t* d_pitem, const int32_t* d_pstep, int64_t n_pairs,
                   int n, float keep_prob, uint64_t seed, uint64_t step, uint8_t* d_pkeep, void* stream) {
    SKR_REQUIRE(d_users && d_puser && d_pitem && d_pkeep, "skr_cdae_draws: NULL argument");
    SKR_REQUIRE(n_pairs >= 0 && n >= 0, "skr_cdae_draws: n_pairs = %lld, n = %d", static_cast<long long>(n_pairs), n);
    SKR_REQUIRE(keep_prob > 0.0f && keep_prob <= 1.0f, "skr_cdae_draws: keep_prob = %g is not in (0, 1]", keep_prob);
    if (n_pairs == 0) return SKR_OK;
    hipLaunchKernelGGL(cdae_draws_kernel, dim3(static_cast<unsigned>((n_pairs + 255) / 256)), dim3(256), 0, skr::as_stream(stream),
                       d_users, d_puser, d_pitem, d_pstep, n_pairs, n, keep_prob, seed, step, d_pkeep);
    SKR_LAUNCH_CHECK();
    return SKR_OK;
}

}  // extern "C"
