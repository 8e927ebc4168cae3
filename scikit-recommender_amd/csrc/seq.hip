// seq.hip -- the sequential pairwise recommenders: FPMC and TransRec training steps, and their dense score rows.
//
// Replaces the stock torch ops the reference issues per step and per evaluation batch (no native code there):
//   recommender/FPMC.py:71-79,118-128       four gathers, two inner products, bpr_loss.sum(), l2_loss, backward
//   recommender/FPMC.py:81-86               predict: two [B, d] x [d, I] products
//   recommender/TransRec.py:75-84,125-135   gathers, (u + T) + last, -l2_distance + bias, bpr_loss, l2_loss, backward
//   recommender/TransRec.py:86-93           predict: -l2_distance against every item row + bias
//   utils/torch.py:20-29,62-74              inner_product, l2_distance (torch.norm), bpr_loss, l2_loss
//
// Step kernels map a row of dp = 64 C floats onto the 64 lanes of one wavefront (lane l owns floats l, l + 64, ...), as
// bpr_step_kernel (train.hip) does: every row access is one coalesced 256-byte access per 64 floats, scores are wave
// reductions, row gradients are 256-byte global_atomic_add_f32 scatters.  TransRec's global transition row T is in every
// triple; its gradient is summed in a fixed order (per-wave registers, per-workgroup LDS, then one ordered pass over the
// workgroups' partials in a second launch) so that it does not depend on timing.
#include "skr_common.h"

#include <cmath>

namespace {

constexpr int D = 64;
constexpr int SEQ_WAVES = 4;                       // wavefronts per workgroup of the step kernels
constexpr int SEQ_MAX_BLOCKS = SKR_TRANSREC_MAX_BLOCKS;

__device__ __forceinline__ void bpr_terms(float x, float& l, float& c) {
    // -logsigmoid(x) = -(min(0,x) - log1p(exp(-|x|)))  (torch's log_sigmoid forward); dl/dx = -sigmoid(-x)
    const float z = expf(-fabsf(x));
    l = -(fminf(0.0f, x) - log1pf(z));
    c = -((x >= 0.0f) ? z / (1.0f + z) : 1.0f / (1.0f + z));
}

__device__ __forceinline__ void add_loss(float* loss, int loss_slots, float a, float b) {
    // same convention as bpr_step_kernel: workgroup g adds to pair g % loss_slots
    const int sl = 2 * (static_cast<int>(blockIdx.x) % loss_slots);
    atomicAdd(&loss[sl], a);
    atomicAdd(&loss[sl + 1], b);
}

// ------------------------------------------------------------------------------------------------
// FPMC step: y = <UI[u], IU[i]> + <LI[l], IL[i]>, i = p or n
// ------------------------------------------------------------------------------------------------
template <int C>
__global__ __launch_bounds__(SEQ_WAVES * 64) void fpmc_step_kernel(
    const float* __restrict__ UI, const float* __restrict__ IU, const float* __restrict__ IL, const float* __restrict__ LI,
    const int32_t* __restrict__ u_ids, const int32_t* __restrict__ l_ids, const int32_t* __restrict__ p_ids,
    const int32_t* __restrict__ n_ids, int n, int n_users, int n_items, float reg, float* __restrict__ gUI,
    float* __restrict__ gIU, float* __restrict__ gIL, float* __restrict__ gLI, float* __restrict__ loss, int loss_slots) {
    __shared__ float s_loss[SEQ_WAVES], s_l2[SEQ_WAVES];
    constexpr int DW = D * C;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float acc_loss = 0.0f, acc_l2 = 0.0f;
    for (int b = blockIdx.x * SEQ_WAVES + wv; b < n; b += gridDim.x * SEQ_WAVES) {
        const int64_t u = u_ids[b], l = l_ids[b], p = p_ids[b], q = n_ids[b];
        // ids are wave-uniform: an out-of-range triple is skipped by the whole wave (it contributes nothing)
        if (u < 0 || u >= n_users || l < 0 || l >= n_items || p < 0 || p >= n_items || q < 0 || q >= n_items) continue;
        float ui[C], li[C], iup[C], iun[C], ilp[C], iln[C];
        float a_p = 0.0f, a_n = 0.0f, b_p = 0.0f, b_n = 0.0f, sl = 0.0f;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const int k = c * D + lane;
            ui[c] = UI[u * DW + k]; li[c] = LI[l * DW + k];
            iup[c] = IU[p * DW + k]; iun[c] = IU[q * DW + k];
            ilp[c] = IL[p * DW + k]; iln[c] = IL[q * DW + k];
            a_p += ui[c] * iup[c]; a_n += ui[c] * iun[c];
            b_p += li[c] * ilp[c]; b_n += li[c] * iln[c];
            sl += ui[c] * ui[c] + li[c] * li[c] + iup[c] * iup[c] + iun[c] * iun[c] + ilp[c] * ilp[c] + iln[c] * iln[c];
        }
        // the two inner products of each score are reduced separately and then added (FPMC.py:77)
        const float yp = skr::wave_sum(a_p) + skr::wave_sum(b_p);
        const float yn = skr::wave_sum(a_n) + skr::wave_sum(b_n);
        const float sq = skr::wave_sum(sl);
        float lo, cc;
        bpr_terms(yp - yn, lo, cc);
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const int k = c * D + lane;
            atomicAdd(&gUI[u * DW + k], cc * (iup[c] - iun[c]) + reg * ui[c]);
            atomicAdd(&gLI[l * DW + k], cc * (ilp[c] - iln[c]) + reg * li[c]);
            atomicAdd(&gIU[p * DW + k], cc * ui[c] + reg * iup[c]);
            atomicAdd(&gIU[q * DW + k], -cc * ui[c] + reg * iun[c]);
            atomicAdd(&gIL[p * DW + k], cc * li[c] + reg * ilp[c]);
            atomicAdd(&gIL[q * DW + k], -cc * li[c] + reg * iln[c]);
        }
        acc_loss += lo;
        acc_l2 += 0.5f * sq;
    }
    if (lane == 0) {
        s_loss[wv] = acc_loss;
        s_l2[wv] = acc_l2;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float a = 0.0f, b2 = 0.0f;
        for (int w = 0; w < SEQ_WAVES; ++w) {
            a += s_loss[w];
            b2 += s_l2[w];
        }
        add_loss(loss, loss_slots, a, b2);
    }
}

// ------------------------------------------------------------------------------------------------
// TransRec step: t = (U[u] + T) + V[l];  y = -||t - V[i]|| + b[i], i = p or n
// ------------------------------------------------------------------------------------------------
template <int C>
__global__ __launch_bounds__(SEQ_WAVES * 64) void transrec_step_kernel(
    const float* __restrict__ U, const float* __restrict__ V, const float* __restrict__ bias, const float* __restrict__ T,
    const int32_t* __restrict__ u_ids, const int32_t* __restrict__ l_ids, const int32_t* __restrict__ p_ids,
    const int32_t* __restrict__ n_ids, int n, int n_users, int n_items, float reg, float* __restrict__ gU,
    float* __restrict__ gV, float* __restrict__ gb, float* __restrict__ partial, float* __restrict__ loss, int loss_slots) {
    constexpr int DW = D * C;
    __shared__ float s_loss[SEQ_WAVES], s_l2[SEQ_WAVES];
    __shared__ float s_dt[SEQ_WAVES][DW];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float acc_loss = 0.0f, acc_l2 = 0.0f;
    float tr[C], dt_acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        tr[c] = T[c * D + lane];
        dt_acc[c] = 0.0f;
    }
    for (int b = blockIdx.x * SEQ_WAVES + wv; b < n; b += gridDim.x * SEQ_WAVES) {
        const int64_t u = u_ids[b], l = l_ids[b], p = p_ids[b], q = n_ids[b];
        if (u < 0 || u >= n_users || l < 0 || l >= n_items || p < 0 || p >= n_items || q < 0 || q >= n_items) continue;
        float uu[C], vl[C], vp[C], vn[C], ep[C], en[C];
        float sp = 0.0f, sn = 0.0f, sl = 0.0f;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const int k = c * D + lane;
            uu[c] = U[u * DW + k]; vl[c] = V[l * DW + k]; vp[c] = V[p * DW + k]; vn[c] = V[q * DW + k];
            const float t = (uu[c] + tr[c]) + vl[c];          // TransRec.py:81, in its order of additions
            ep[c] = t - vp[c];
            en[c] = t - vn[c];
            sp += ep[c] * ep[c];
            sn += en[c] * en[c];
            sl += uu[c] * uu[c] + vl[c] * vl[c] + vp[c] * vp[c] + vn[c] * vn[c];
        }
        const float dp = sqrtf(skr::wave_sum(sp)), dn = sqrtf(skr::wave_sum(sn));
        const float bp = bias[p], bn = bias[q];
        const float sq = skr::wave_sum(sl) + bp * bp + bn * bn;
        float lo, cc;
        bpr_terms((-dp + bp) - (-dn + bn), lo, cc);
        // dL/dy_p = cc, dL/dy_n = -cc;  dy/dt = -(t - V[i]) / ||t - V[i]|| (0 at distance 0: torch's norm subgradient)
        const float wp = dp > 0.0f ? cc / dp : 0.0f, wn = dn > 0.0f ? cc / dn : 0.0f;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const int k = c * D + lane;
            const float g_t = -wp * ep[c] + wn * en[c];
            dt_acc[c] += g_t;
            atomicAdd(&gU[u * DW + k], g_t + reg * uu[c]);
            atomicAdd(&gV[l * DW + k], g_t + reg * vl[c]);
            atomicAdd(&gV[p * DW + k], wp * ep[c] + reg * vp[c]);
            atomicAdd(&gV[q * DW + k], -wn * en[c] + reg * vn[c]);
        }
        if (lane == 0) {
            atomicAdd(&gb[p], cc + reg * bp);
            atomicAdd(&gb[q], -cc + reg * bn);
        }
        acc_loss += lo;
        acc_l2 += 0.5f * sq;
    }
#pragma unroll
    for (int c = 0; c < C; ++c) s_dt[wv][c * D + lane] = dt_acc[c];
    if (lane == 0) {
        s_loss[wv] = acc_loss;
        s_l2[wv] = acc_l2;
    }
    __syncthreads();
    // this workgroup's partial of dL/dT: its waves in order
    for (int k = threadIdx.x; k < DW; k += SEQ_WAVES * 64) {
        float s = 0.0f;
        for (int w = 0; w < SEQ_WAVES; ++w) s += s_dt[w][k];
        partial[static_cast<int64_t>(blockIdx.x) * DW + k] = s;
    }
    if (threadIdx.x == 0) {
        float a = 0.0f, b2 = 0.0f;
        for (int w = 0; w < SEQ_WAVES; ++w) {
            a += s_loss[w];
            b2 += s_l2[w];
        }
        add_loss(loss, loss_slots, a, b2);
    }
}

// gT += sum over the step kernel's workgroups + reg * T; T's own l2 term once per batch.  Wavefront w of T_WAVES adds
// the partials w, w + T_WAVES, ... in that order (lane-per-float like the step), then wavefront 0 adds the T_WAVES sums
// in order: a fixed order of additions for a given number of partials.
constexpr int T_WAVES = 16;

template <int C>
__global__ __launch_bounds__(T_WAVES * 64) void transrec_t_kernel(const float* __restrict__ T, const float* __restrict__ partial,
                                                                  int n_parts, float reg, float* __restrict__ gT,
                                                                  float* __restrict__ loss) {
    constexpr int DW = D * C;
    __shared__ float s_part[T_WAVES][DW];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int k = c * D + lane;
        float s = 0.0f;
        int g = wv;
        for (; g + 3 * T_WAVES < n_parts; g += 4 * T_WAVES) {     // four loads in flight, added in order
            const float a0 = partial[static_cast<int64_t>(g) * DW + k];
            const float a1 = partial[static_cast<int64_t>(g + T_WAVES) * DW + k];
            const float a2 = partial[static_cast<int64_t>(g + 2 * T_WAVES) * DW + k];
            const float a3 = partial[static_cast<int64_t>(g + 3 * T_WAVES) * DW + k];
            s += a0; s += a1; s += a2; s += a3;
        }
        for (; g < n_parts; g += T_WAVES) s += partial[static_cast<int64_t>(g) * DW + k];
        s_part[wv][k] = s;
    }
    __syncthreads();
    if (wv != 0) return;
    float sl = 0.0f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int k = c * D + lane;
        float s = 0.0f;
        for (int w = 0; w < T_WAVES; ++w) s += s_part[w][k];
        const float t = T[k];
        gT[k] += s + reg * t;
        sl += t * t;
    }
    const float sq = skr::wave_sum(sl);
    if (lane == 0) atomicAdd(&loss[1], 0.5f * sq);
}

// ------------------------------------------------------------------------------------------------
// Dense score rows.  A workgroup = SC_ITEMS items (one per thread) x QB users; the users' query rows are staged in LDS
// (every lane reads the same LDS words: broadcasts), every item row is read once per workgroup, 128 bytes per lane per
// burst of 8 float4 loads (one whole cache line per lane, so the line is used while it is in flight).
//   mode 0 (FPMC):     out = <UI[u], IU[i]> + <LI[last], IL[i]>, the two sums kept apart (FPMC.py:81-86)
//   mode 1 (TransRec): out = -sqrt(sum_k (t_k - V[i]_k)^2) + b[i], t = (U[u] + T) + V[last], from the differences
// ------------------------------------------------------------------------------------------------
constexpr int SC_ITEMS = 256;

template <int MODE, int C>
__global__ __launch_bounds__(SC_ITEMS) void seq_scores_kernel(
    const float* __restrict__ QU, const float* __restrict__ QL, const float* __restrict__ IA, const float* __restrict__ IB,
    const float* __restrict__ T, const float* __restrict__ bias, const int32_t* __restrict__ users, int B,
    const int32_t* __restrict__ last_item, int n_users, int n_items, float* __restrict__ out, int64_t ld) {
    constexpr int DW = D * C;
    constexpr int NQ = MODE == 0 ? 2 : 1;          // query rows per user
    constexpr int QB = MODE == 0 ? 16 : 32;        // users per workgroup
    __shared__ float4 s_q[QB * NQ * DW / 4];
    __shared__ int s_ok[QB];
    const int q0 = blockIdx.y * QB;
    float* sqf = reinterpret_cast<float*>(s_q);
    for (int e = threadIdx.x; e < QB * DW; e += SC_ITEMS) {
        const int q = e / DW, k = e - q * DW, b = q0 + q;
        bool ok = false;
        int64_t u = -1, l = -1;
        if (b < B) {
            u = users[b];
            if (u >= 0 && u < n_users) {
                l = last_item[u];
                ok = l >= 0 && l < n_items;
            }
        }
        if (MODE == 0) {
            sqf[(q * 2) * DW + k] = ok ? QU[u * DW + k] : 0.0f;
            sqf[(q * 2 + 1) * DW + k] = ok ? QL[l * DW + k] : 0.0f;
        } else {
            sqf[q * DW + k] = ok ? (QU[u * DW + k] + T[k]) + QL[l * DW + k] : 0.0f;
        }
        if (k == 0) s_ok[q] = ok;
    }
    __syncthreads();
    const int64_t i = static_cast<int64_t>(blockIdx.x) * SC_ITEMS + threadIdx.x;
    if (i >= n_items) return;
    float acc[QB], acc2[MODE == 0 ? QB : 1];
#pragma unroll
    for (int q = 0; q < QB; ++q) acc[q] = 0.0f;
#pragma unroll
    for (int q = 0; q < (MODE == 0 ? QB : 1); ++q) acc2[q] = 0.0f;
    const float4* ra = reinterpret_cast<const float4*>(IA + i * DW);
    const float4* rb = reinterpret_cast<const float4*>(MODE == 0 ? IB + i * DW : IA + i * DW);
    for (int k8 = 0; k8 < DW / 4; k8 += 8) {
        float4 xa[8], xb[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) xa[j] = ra[k8 + j];
        if (MODE == 0) {
#pragma unroll
            for (int j = 0; j < 8; ++j) xb[j] = rb[k8 + j];
        }
#pragma unroll
        for (int q = 0; q < QB; ++q) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float4 s = s_q[(q * NQ) * (DW / 4) + k8 + j];
                if (MODE == 0) {
                    const float4 r = s_q[(q * NQ + 1) * (DW / 4) + k8 + j];
                    acc[q] = fmaf(s.x, xa[j].x, acc[q]); acc[q] = fmaf(s.y, xa[j].y, acc[q]);
                    acc[q] = fmaf(s.z, xa[j].z, acc[q]); acc[q] = fmaf(s.w, xa[j].w, acc[q]);
                    acc2[q] = fmaf(r.x, xb[j].x, acc2[q]); acc2[q] = fmaf(r.y, xb[j].y, acc2[q]);
                    acc2[q] = fmaf(r.z, xb[j].z, acc2[q]); acc2[q] = fmaf(r.w, xb[j].w, acc2[q]);
                } else {
                    const float dx = s.x - xa[j].x, dy = s.y - xa[j].y, dz = s.z - xa[j].z, dw = s.w - xa[j].w;
                    acc[q] = fmaf(dx, dx, acc[q]); acc[q] = fmaf(dy, dy, acc[q]);
                    acc[q] = fmaf(dz, dz, acc[q]); acc[q] = fmaf(dw, dw, acc[q]);
                }
            }
        }
    }
    const float bi = MODE == 1 ? bias[i] : 0.0f;
#pragma unroll
    for (int q = 0; q < QB; ++q) {
        const int b = q0 + q;
        if (b < B) {
            float v;
            if (MODE == 0) v = acc[q] + acc2[q];
            else v = -sqrtf(acc[q]) + bi;
            out[static_cast<int64_t>(b) * ld + i] = s_ok[q] ? v : __builtin_nanf("");
        }
    }
}

int check_dim(int dim, const char* fn) {
    if (dim == 64 || dim == 128 || dim == 192 || dim == 256) return SKR_OK;
    return skr::fail(SKR_EINVAL, "%s: dim must be 64, 128, 192 or 256 (got %d); pad narrower rows with zeros", fn, dim);
}

int step_blocks(int n) {
    int blocks = (n + SEQ_WAVES - 1) / SEQ_WAVES;
    return blocks > SEQ_MAX_BLOCKS ? SEQ_MAX_BLOCKS : blocks;
}

}  // namespace

extern "C" {

int skr_fpmc_step(const float* d_UI, const float* d_IU, const float* d_IL, const float* d_LI, const int32_t* d_u,
                  const int32_t* d_l, const int32_t* d_p, const int32_t* d_n, int n, int n_users, int n_items, int dim,
                  float reg, float* d_gUI, float* d_gIU, float* d_gIL, float* d_gLI, float* d_loss, int loss_slots,
                  void* stream) {
    SKR_REQUIRE(d_UI && d_IU && d_IL && d_LI && d_u && d_l && d_p && d_n && d_gUI && d_gIU && d_gIL && d_gLI && d_loss,
                "skr_fpmc_step: NULL argument");
    SKR_REQUIRE(n >= 0 && n_users > 0 && n_items > 0, "skr_fpmc_step: n = %d, n_users = %d, n_items = %d", n, n_users, n_items);
    SKR_REQUIRE(loss_slots == 1 || loss_slots == SKR_LOSS_SLOTS, "skr_fpmc_step: loss_slots must be 1 or %d", SKR_LOSS_SLOTS);
    if (int rc = check_dim(dim, "skr_fpmc_step")) return rc;
    if (n == 0) return SKR_OK;
    const int blocks = step_blocks(n);
#define SKR_FPMC_LAUNCH(C_)                                                                                                 \
    hipLaunchKernelGGL(fpmc_step_kernel<C_>, dim3(blocks), dim3(SEQ_WAVES * 64), 0, skr::as_stream(stream), d_UI, d_IU,   \
                       d_IL, d_LI, d_u, d_l, d_p, d_n, n, n_users, n_items, reg, d_gUI, d_gIU, d_gIL, d_gLI, d_loss,       \
                       loss_slots)
    switch (dim / 64) {
        case 1: SKR_FPMC_LAUNCH(1); break;
        case 2: SKR_FPMC_LAUNCH(2); break;
        case 3: SKR_FPMC_LAUNCH(3); break;
        default: SKR_FPMC_LAUNCH(4); break;
    }
#undef SKR_FPMC_LAUNCH
    SKR_LAUNCH_CHECK();
    return SKR_OK;
}

int skr_transrec_step(const float* d_U, const float* d_V, const float* d_bias, const float* d_T, const int32_t* d_u,
                      const int32_t* d_l, const int32_t* d_p, const int32_t* d_n, int n, int n_users, int n_items, int dim,
                      float reg, float* d_gU, float* d_gV, float* d_gb, float* d_gT, float* d_work, float* d_loss,
                      int loss_slots, void* stream) {
    SKR_REQUIRE(d_U && d_V && d_bias && d_T && d_u && d_l && d_p && d_n && d_gU && d_gV && d_gb && d_gT && d_work && d_loss,
                "skr_transrec_step: NULL argument");
    SKR_REQUIRE(n >= 0 && n_users > 0 && n_items > 0, "skr_transrec_step: n = %d, n_users = %d, n_items = %d", n, n_users,
                n_items);
    SKR_REQUIRE(loss_slots == 1 || loss_slots == SKR_LOSS_SLOTS, "skr_transrec_step: loss_slots must be 1 or %d",
                SKR_LOSS_SLOTS);
    if (int rc = check_dim(dim, "skr_transrec_step")) return rc;
    if (n == 0) return SKR_OK;
    const int blocks = step_blocks(n);
    hipStream_t st = skr::as_stream(stream);
#define SKR_TRANSREC_LAUNCH(C_)                                                                                             \
    do {                                                                                                                    \
        hipLaunchKernelGGL(transrec_step_kernel<C_>, dim3(blocks), dim3(SEQ_WAVES * 64), 0, st, d_U, d_V, d_bias, d_T, d_u, \
                           d_l, d_p, d_n, n, n_users, n_items, reg, d_gU, d_gV, d_gb, d_work, d_loss, loss_slots);          \
        hipLaunchKernelGGL(transrec_t_kernel<C_>, dim3(1), dim3(T_WAVES * 64), 0, st, d_T, d_work, blocks, reg, d_gT, d_loss);      \
    } while (0)
    switch (dim / 64) {
        case 1: SKR_TRANSREC_LAUNCH(1); break;
        case 2: SKR_TRANSREC_LAUNCH(2); break;
        case 3: SKR_TRANSREC_LAUNCH(3); break;
        default: SKR_TRANSREC_LAUNCH(4); break;
    }
#undef SKR_TRANSREC_LAUNCH
    SKR_LAUNCH_CHECK();
    return SKR_OK;
}

int skr_seq_scores(int mode, const float* d_user_table, const float* d_last_table, const float* d_item_table,
                   const float* d_item_table2, const float* d_transition, const float* d_item_bias, const int32_t* d_users,
                   int B, const int32_t* d_last_item, int n_users, int n_items, int dim, float* d_out, int64_t ld,
                   void* stream) {
    SKR_REQUIRE(mode == SKR_SEQ_FPMC || mode == SKR_SEQ_TRANSREC, "skr_seq_scores: unknown mode %d", mode);
    SKR_REQUIRE(d_user_table && d_last_table && d_item_table && d_users && d_last_item && d_out,
                "skr_seq_scores: NULL argument");
    SKR_REQUIRE(mode != SKR_SEQ_FPMC || d_item_table2, "skr_seq_scores: NULL argument (FPMC needs d_item_table2)");
    SKR_REQUIRE(mode != SKR_SEQ_TRANSREC || (d_transition && d_item_bias),
                "skr_seq_scores: NULL argument (TransRec needs d_transition and d_item_bias)");
    SKR_REQUIRE(B >= 0 && n_users > 0 && n_items > 0 && ld >= n_items, "skr_seq_scores: B = %d, n_users = %d, n_items = %d, ld = %lld",
                B, n_users, n_items, static_cast<long long>(ld));
    SKR_REQUIRE(((reinterpret_cast<uintptr_t>(d_item_table) | reinterpret_cast<uintptr_t>(d_item_table2)) & 15) == 0,
                "skr_seq_scores: item tables must be 16-byte aligned");
    if (int rc = check_dim(dim, "skr_seq_scores")) return rc;
    if (B == 0) return SKR_OK;
    const int qb = mode == SKR_SEQ_FPMC ? 16 : 32;
    const int gy = (B + qb - 1) / qb;
    SKR_REQUIRE(gy <= 65535, "skr_seq_scores: B = %d is more than %d users per call", B, 65535 * qb);
    const dim3 grid((n_items + SC_ITEMS - 1) / SC_ITEMS, gy), blk(SC_ITEMS);
    hipStream_t st = skr::as_stream(stream);
#define SKR_SCORES_LAUNCH(M_, C_)                                                                                           \
    hipLaunchKernelGGL((seq_scores_kernel<M_, C_>), grid, blk, 0, st, d_user_table, d_last_table, d_item_table,             \
                       d_item_table2, d_transition, d_item_bias, d_users, B, d_last_item, n_users, n_items, d_out, ld)
#define SKR_SCORES_PICK(M_)                                     \
    switch (dim / 64) {                                         \
        case 1: SKR_SCORES_LAUNCH(M_, 1); break;                \
        case 2: SKR_SCORES_LAUNCH(M_, 2); break;                \
        case 3: SKR_SCORES_LAUNCH(M_, 3); break;                \
        default: SKR_SCORES_LAUNCH(M_, 4); break;               \
    }
    if (mode == SKR_SEQ_FPMC) { SKR_SCORES_PICK(0) } else { SKR_SCORES_PICK(1) }
#undef SKR_SCORES_PICK
#undef SKR_SCORES_LAUNCH
    SKR_LAUNCH_CHECK();
    return SKR_OK;
}

}  // extern "C"
