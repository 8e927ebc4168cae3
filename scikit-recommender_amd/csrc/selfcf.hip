// selfcf.hip -- SelfCF (SelfCF: A Simple Framework for Self-supervised Collaborative Filtering, TORS 2023), the
// embedding-dropout variant on a LightGCN encoder with per-step edge dropout: the keep flags of a step's plan runs, the
// predictor, the cosine loss and the whole backward of one training step, the host entry that issues the step, and the
// query rows of the ranking.
//
// Replaces the stock torch ops the reference issues per step (no native code there):
//   recommender/SelfCF.py:133-144  sparse_dropout: a fresh mask over the 2 nnz entries of the square adjacency, a new sparse
//                                  tensor, the scaling by 1 / (1 - rate)
//   recommender/SelfCF.py:146-168  n_layers torch.sparse.mm on the masked matrix, the mean of the layers, the batch's rows
//   recommender/SelfCF.py:205-233  F.dropout of the detached targets, the predictor on both sides, the two cosine terms, the
//                                  regulariser, and autograd's backward through all of it
//   recommender/SelfCF.py:235-241  full_sort_predict: the two score matrices
//
// Layout: every table has 64-float rows, zero beyond d.  Users and items share flat [U + I, 64] tables (user rows first).
// The parameters are one flat buffer: the [U + I, 64] rows, then the predictor's row-major W [64 out][64 in] and b [64],
// zero beyond d.  The gradient has the same layout.
//
// Launches of a step:
//   2L dropped runs  X_k = A-hat' X_(k-1): user rows from A with k1, item rows from A^T with k2; the mean M rides in the
//                    accum epilogue
//   batch            per 64 batch rows and side: p = W x + b as 16-row tiles on v_mfma_f32_16x16x4_f32 (exact fp32), the
//                    dropped-out target, the cosine, g_p, g_x = W^T g_p + reg x (the transposed W in LDS), dW and db as the
//                    workgroup's partial sums
//   pred_reduce      the partial sums in workgroup order
//   loss             the two loss components and their sum
//   rank, seg_add    the g_x rows into the cleared table G, per distinct node id, in rank order
//   2L dropped runs  acc = G; acc = (A-hat')^T acc + G (the addend epilogue) with the backward keeps; the last writes
//                    acc / (L + 1) into the gradient
//
// The MFMA operand mapping is mfma_tile.h's k = 16 g + kk.
//
// Determinism: there is no floating-point atomic anywhere in the step.
#include "skr_common.h"
#include "fast_rng.h"
#include "mfma_tile.h"
#include "step_common.h"

#include <algorithm>

namespace {

using namespace skr;

constexpr int D = 64;          // columns of every table
constexpr int LDP = 68;        // LDS row stride
constexpr int HW = 4;          // wavefronts per workgroup
constexpr int TB = 64;         // rows of a workgroup's tile: 16 per wavefront
constexpr int MAXB = SKR_SELFCF_MAX_BATCH;
constexpr int MAXL = SKR_SELFCF_MAX_LAYERS;
constexpr int PRED = SKR_SELFCF_PRED_FLOATS;
constexpr float COS_EPS = 1e-8f;   // F.cosine_similarity's default

// streams of the device draws: the two halves of the edge mask, the two target masks (the user side first)
enum { DRAW_K1 = 0, DRAW_K2 = 1, DRAW_KU = 2, DRAW_KI = 3 };

// ------------------------------------------------------------------------------------------------
// the keep flags of a step's plan runs
// ------------------------------------------------------------------------------------------------
// thread i: fu[i] = k1[i], fi[i] = k2[i], bu[i] = k2[perm[i]] (k2 in A's order), bi[perm[i]] = k1[i] (k1 in At's order):
// perm is a bijection, so every byte of bi is written once
__global__ __launch_bounds__(256) void sc_keeps_kernel(const int32_t* __restrict__ perm, int64_t nnz, const uint8_t* __restrict__ k1,
                                                       const uint8_t* __restrict__ k2, float rate, uint64_t seed, uint64_t step,
                                                       uint8_t* __restrict__ fu, uint8_t* __restrict__ fi, uint8_t* __restrict__ bu,
                                                       uint8_t* __restrict__ bi) {
    const int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
    if (i >= nnz) return;
    const int64_t p = perm[i];
    const bool in = p >= 0 && p < nnz;
    const bool a = k1 ? k1[i] != 0 : draw_keep(seed, step, DRAW_K1, static_cast<uint64_t>(i), rate);
    const bool b = k2 ? k2[i] != 0 : draw_keep(seed, step, DRAW_K2, static_cast<uint64_t>(i), rate);
    const bool bp = !in ? false : (k2 ? k2[p] != 0 : draw_keep(seed, step, DRAW_K2, static_cast<uint64_t>(p), rate));
    fu[i] = a ? 1 : 0;
    fi[i] = b ? 1 : 0;
    bu[i] = bp ? 1 : 0;
    if (in) bi[p] = a ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------
// batch: the predictor, the targets, the cosine terms and their backward for 64 batch rows
// ------------------------------------------------------------------------------------------------
// side 0: x = u = M[users], target t_i = i ki / (1 - p); side 1: x = i = M[U + items], target t_u = u ku / (1 - p).
//   P = W x + b;  c = <P, t> / (max(|P|, eps) max(|t|, eps));  g_P = -coef (t / (nP nt) - [|P| > eps] c P / nP^2), coef = 0.5 / n
//   g_x = W^T g_P + reg x  -> Gx [2][n][64] (side-major);  dW += g_P x^T, db += g_P
// lossb [4][n]: c of side 0, c of side 1, |u|^2, |i|^2 per batch row.  part [gridDim.x][PRED]: the workgroup's dW and db.
__global__ __launch_bounds__(HW * 64) void sc_batch_kernel(const float* __restrict__ M, const float* __restrict__ pred,
                                                           const int32_t* __restrict__ users, const int32_t* __restrict__ items,
                                                           const uint8_t* __restrict__ ku, const uint8_t* __restrict__ ki, int n, int U,
                                                           int I, float inv_keep, float p_drop, uint64_t seed, uint64_t step, float reg,
                                                           float coef, float* __restrict__ Gx, float* __restrict__ lossb,
                                                           float* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float sW[D * LDP];      // sW[out][in]
    __shared__ __attribute__((aligned(16))) float sWT[D * LDP];     // sWT[in][out]
    __shared__ __attribute__((aligned(16))) float sG[TB * LDP];     // g_P[row][out]
    __shared__ __attribute__((aligned(16))) float sGT[D * LDP];     // g_P^T[out][row]
    __shared__ __attribute__((aligned(16))) float sXT[D * LDP];     // x^T[in][row]
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
    for (int idx = threadIdx.x; idx < D * 16; idx += HW * 64) {
        const int row = idx >> 4, c4 = idx & 15;
        const float4 v = *reinterpret_cast<const float4*>(pred + row * D + c4 * 4);
        *reinterpret_cast<float4*>(sW + row * LDP + c4 * 4) = v;
        sWT[(c4 * 4 + 0) * LDP + row] = v.x;
        sWT[(c4 * 4 + 1) * LDP + row] = v.y;
        sWT[(c4 * 4 + 2) * LDP + row] = v.z;
        sWT[(c4 * 4 + 3) * LDP + row] = v.w;
    }
    const float* __restrict__ bias = pred + D * D;
    const int b0 = blockIdx.x * TB + wv * 16;
    f32x4 dW[4];
    zero_acc(dW);
    float db = 0.0f;
    __syncthreads();
    for (int side = 0; side < 2; ++side) {
        // ---- A layout: lane (r, g) holds columns [16 g, 16 g + 16) of the wavefront's row r
        const int bA = b0 + r;
        const int64_t uA = bA < n ? checked(users[bA], U) : -1, iA = bA < n ? checked(items[bA], I) : -1;
        const bool validA = uA >= 0 && iA >= 0;
        float xa[16];
        load_row_a(xa, M, validA ? (side == 0 ? uA : U + iA) : -1, g);
        {
            float sq = 0.0f;
#pragma unroll
            for (int kk = 0; kk < 16; ++kk) sq += xa[kk] * xa[kk];
            sq += __shfl_xor(sq, 16, 64);
            sq += __shfl_xor(sq, 32, 64);
            if (g == 0 && bA < n) lossb[static_cast<int64_t>(2 + side) * n + bA] = sq;
        }
        f32x4 P[4];
        zero_acc(P);
        tile_product<LDP>(P, xa, sW, r, g);
        // ---- D layout: lane (r, g) holds column 16 nb + r of the rows 4 g + rr
        const uint8_t* __restrict__ karr = side == 0 ? ki : ku;
        const uint64_t kstream = side == 0 ? DRAW_KI : DRAW_KU;
        f32x4 gp[4];
        int64_t nodeX[4];
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int bD = b0 + 4 * g + rr;
            const bool in = bD < n;
            const int64_t uD = in ? checked(users[bD], U) : -1, iD = in ? checked(items[bD], I) : -1;
            const bool valid = uD >= 0 && iD >= 0;
            nodeX[rr] = valid ? (side == 0 ? uD : U + iD) : -1;
            const int64_t nodeT = side == 0 ? U + iD : uD;
            float tv[4], dot = 0.0f, pp = 0.0f, tt = 0.0f;
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) {
                const int col = nb * 16 + r;
                P[nb][rr] += bias[col];
                float t = 0.0f;
                if (valid) {
                    const int64_t f = static_cast<int64_t>(bD) * D + col;
                    const bool kf = karr ? karr[f] != 0 : draw_keep(seed, step, kstream, static_cast<uint64_t>(f), p_drop);
                    if (kf) t = M[nodeT * D + col] * inv_keep;
                }
                tv[nb] = t;
                dot += P[nb][rr] * t;
                pp += P[nb][rr] * P[nb][rr];
                tt += t * t;
            }
            dot = sum16(dot); pp = sum16(pp); tt = sum16(tt);
            const float nPr = sqrtf(pp), nP = fmaxf(nPr, COS_EPS), nT = fmaxf(sqrtf(tt), COS_EPS);
            const float c = valid ? dot / (nP * nT) : 0.0f;
            if (r == 0 && in) lossb[static_cast<int64_t>(side) * n + bD] = c;
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) {
                float gv = 0.0f;
                if (valid) {
                    gv = tv[nb] / (nP * nT);
                    if (nPr > COS_EPS) gv -= c * P[nb][rr] / (nP * nP);     // (a clamped norm has zero slope)
                    gv = -coef * gv;
                }
                gp[nb][rr] = gv;
            }
        }
        __syncthreads();                                       // the previous side's products still read the images
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) {
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                sG[(wv * 16 + 4 * g + rr) * LDP + nb * 16 + r] = gp[nb][rr];
                sGT[(nb * 16 + r) * LDP + wv * 16 + 4 * g + rr] = gp[nb][rr];
            }
        }
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) sXT[(16 * g + kk) * LDP + wv * 16 + r] = xa[kk];
        __syncthreads();
        float ga[16];
        load_slab<LDP>(ga, sG, wv * 16 + r, g);
        f32x4 gx[4];
        zero_acc(gx);
        tile_product<LDP>(gx, ga, sWT, r, g);
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int bD = b0 + 4 * g + rr;
            if (bD >= n) continue;
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) {
                const int col = nb * 16 + r;
                float v = gx[nb][rr];
                if (nodeX[rr] >= 0) v += reg * M[nodeX[rr] * D + col];
                Gx[(static_cast<int64_t>(side) * n + bD) * D + col] = v;
            }
        }
        float slab[16];
        load_slab<LDP>(slab, sGT, wv * 16 + r, g);
        tile_product<LDP>(dW, slab, sXT, r, g);
        if (threadIdx.x < D) db += column_sum<LDP>(sGT, threadIdx.x);
    }
    float* out = part + static_cast<int64_t>(blockIdx.x) * PRED;
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) {
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) out[(wv * 16 + 4 * g + rr) * D + nb * 16 + r] = dW[nb][rr];
    }
    if (threadIdx.x < D) out[D * D + threadIdx.x] = db;
}

// loss[0] = the two cosine terms (SelfCF.py:230-231), loss[1] = reg * reg_loss (:226, :233), loss[2] = their sum
__global__ __launch_bounds__(1024) void sc_loss_kernel(const float* __restrict__ lossb, int n, float reg, float* __restrict__ loss) {
    __shared__ float s[1024];
    const int t = threadIdx.x;
    float a = 0.0f, b = 0.0f, c = 0.0f, d = 0.0f;
    for (int k = t; k < n; k += 1024) { a += lossb[k]; b += lossb[n + k]; c += lossb[2 * n + k]; d += lossb[3 * n + k]; }
    const float fn = static_cast<float>(n);
    const float s1 = block_sum_1024(a, s), s2 = block_sum_1024(b, s), s3 = block_sum_1024(c, s), s4 = block_sum_1024(d, s);
    if (t == 0) {
        const float cosl = -(s1 / fn) / 2.0f - (s2 / fn) / 2.0f;
        const float regl = reg * (s3 * 0.5f + s4 * 0.5f);
        loss[0] = cosl;
        loss[1] = regl;
        loss[2] = cosl + regl;
    }
}

// ------------------------------------------------------------------------------------------------
// the g_x rows into the table G
// ------------------------------------------------------------------------------------------------
// G[id] = the sum of the g_x rows whose list entry is id, in rank order, by the wavefront of the id's first rank: one writer
// per distinct id (the table was cleared).  Blocks [0, blocks_u) walk the user list, the others the item list.
__global__ __launch_bounds__(HW * 64) void sc_seg_add_kernel(float* __restrict__ G, const int32_t* __restrict__ users,
                                                             const int32_t* __restrict__ items, const int32_t* __restrict__ order_u,
                                                             const int32_t* __restrict__ order_i, int n, int U, int I, int blocks_u,
                                                             const float* __restrict__ Gx) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const bool user = static_cast<int>(blockIdx.x) < blocks_u;
    const int rk = (user ? blockIdx.x : blockIdx.x - blocks_u) * HW + wv;
    if (rk >= n) return;
    const int32_t* ids = user ? users : items;
    const int32_t* order = user ? order_u : order_i;
    const int limit = user ? U : I;
    const int id = ids[order[rk]];
    if (id < 0 || id >= limit) return;
    if (rk > 0 && ids[order[rk - 1]] == id) return;
    const float* src = Gx + (user ? 0 : static_cast<int64_t>(n) * D);
    float acc = 0.0f;
    for (int k = rk; k < n; ++k) {
        const int o = order[k];
        if (ids[o] != id) break;
        acc += src[static_cast<int64_t>(o) * D + lane];
    }
    G[(static_cast<int64_t>(user ? 0 : U) + id) * D + lane] = acc;
}

// ------------------------------------------------------------------------------------------------
// ranking: Q = (W + W^T) M_u, <b, M_i>, <b, M_u>
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(HW * 64) void sc_queries_kernel(const float* __restrict__ pred, const float* __restrict__ M, int U, int I,
                                                             float* __restrict__ Q, float* __restrict__ item_bias,
                                                             float* __restrict__ user_const) {
    __shared__ float sS[D * D];        // sS[k][j] = W[j][k] + W[k][j]
    __shared__ float sb[D];
    for (int idx = threadIdx.x; idx < D * D; idx += HW * 64) {
        const int k = idx >> 6, j = idx & 63;
        sS[idx] = pred[j * D + k] + pred[k * D + j];
    }
    if (threadIdx.x < D) sb[threadIdx.x] = pred[D * D + threadIdx.x];
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t N = static_cast<int64_t>(U) + I;
    for (int64_t row = static_cast<int64_t>(blockIdx.x) * HW + wv; row < N; row += static_cast<int64_t>(gridDim.x) * HW) {
        const float m = M[row * D + lane];
        const float bd = skr::wave_sum(sb[lane] * m);
        if (row < U) {
            float q = 0.0f;
#pragma unroll 16
            for (int k = 0; k < D; ++k) q = fmaf(sS[k * D + lane], __shfl(m, k, 64), q);
            Q[row * D + lane] = q;
            if (lane == 0) user_const[row] = bd;
        } else if (lane == 0) {
            item_bias[row - U] = bd;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
struct StepLayout {            // float offsets into the step's workspace
    int64_t Gx, lossb, part, ordu, ordi, total;
};

inline int batch_workgroups(int n) { return (n + TB - 1) / TB; }

inline StepLayout step_layout(int n) {
    StepLayout L;
    const int64_t n4 = round4(n);
    int64_t o = 0;
    L.Gx = o; o += 2 * n4 * D;
    L.lossb = o; o += 4 * n4;
    L.part = o; o += static_cast<int64_t>(batch_workgroups(n)) * PRED;
    L.ordu = o; o += n4;
    L.ordi = o; o += n4;
    L.total = o;
    return L;
}

int run_step(const skr_selfcf_step_args* a, void* stream, float* h_ms) {
    SKR_REQUIRE(a, "skr_selfcf_step: NULL argument");
    const int U = a->n_users, I = a->n_items, n = a->n, L = a->n_layers;
    SKR_REQUIRE(a->params && a->users && a->items && a->M && a->grad && a->loss && a->work, "skr_selfcf_step: NULL argument");
    SKR_REQUIRE(U > 0 && I > 0 && n >= 0 && n <= MAXB, "skr_selfcf_step: n_users = %d, n_items = %d, n = %d (at most %d rows)", U, I, n, MAXB);
    SKR_REQUIRE(a->dim >= 1 && a->dim <= D, "skr_selfcf_step: 1 <= dim <= 64 (got %d); rows are 64 floats, zero-padded", a->dim);
    SKR_REQUIRE(L >= 0 && L <= MAXL, "skr_selfcf_step: 0 <= n_layers <= %d (got %d)", MAXL, L);
    SKR_REQUIRE(L == 0 || (a->plan_a && a->plan_at), "skr_selfcf_step: n_layers > 0 needs both plans");
    SKR_REQUIRE(L == 0 || (a->keep_fu && a->keep_fi && a->keep_bu && a->keep_bi), "skr_selfcf_step: n_layers > 0 needs the four keep arrays");
    SKR_REQUIRE(L == 0 || a->G, "skr_selfcf_step: n_layers > 0 needs the table G");
    SKR_REQUIRE(L < 2 || (a->ping[0] && a->ping[1]), "skr_selfcf_step: n_layers > 1 needs both ping tables");
    SKR_REQUIRE(a->dropout >= 0.0f && a->dropout < 1.0f && a->reg >= 0.0f, "skr_selfcf_step: dropout = %g (0 <= dropout < 1), reg = %g", a->dropout, a->reg);
    SKR_REQUIRE(L == 0 || (a->edge_scale > 0.0f && a->edge_scale < 3.0e38f), "skr_selfcf_step: edge_scale = %g", a->edge_scale);
    if (n == 0) return SKR_OK;
    const StepLayout W = step_layout(n);
    SKR_REQUIRE(a->work_bytes >= static_cast<size_t>(W.total) * sizeof(float),
                "skr_selfcf_step: work holds %zu bytes, skr_selfcf_workspace(%d, %d) asks for %zu", a->work_bytes, n, L,
                static_cast<size_t>(W.total) * sizeof(float));
    uintptr_t align = reinterpret_cast<uintptr_t>(a->params) | reinterpret_cast<uintptr_t>(a->grad) | reinterpret_cast<uintptr_t>(a->work) |
                      reinterpret_cast<uintptr_t>(a->M) | reinterpret_cast<uintptr_t>(a->G) | reinterpret_cast<uintptr_t>(a->ping[0]) |
                      reinterpret_cast<uintptr_t>(a->ping[1]);
    SKR_REQUIRE((align & 15) == 0, "skr_selfcf_step: the tables and work must be 16-byte aligned");
    hipStream_t st = skr::as_stream(stream);
    float* w = static_cast<float*>(a->work);
    int32_t* ordu = reinterpret_cast<int32_t*>(w + W.ordu);
    int32_t* ordi = reinterpret_cast<int32_t*>(w + W.ordi);
    const int64_t UO = static_cast<int64_t>(U) * D, N = static_cast<int64_t>(U) + I;
    const float* pred = a->params + N * D;
    StepTimer<SKR_SELFCF_GROUPS + 1> mk(h_ms, st);     // h_ms: an event after every launch group; otherwise nothing
    SKR_HIP(mk.mark());
    // ---- forward (SelfCF.py:151-159): the layer means of X_k = A-hat' X_(k-1), A-hat' the dropped, rescaled matrix
    int rc = mean_forward(a->plan_a, a->plan_at, a->params, UO, N, L, a->ping, a->M, st,
                          [&](const skr_spmm_plan* plan, const float* X, const skr_spmm_epilogue& ep, bool item_half) {
                              return skr_spmm_plan_run_dropped(plan, X, D, &ep, item_half ? a->keep_fi : a->keep_fu, a->edge_scale, stream);
                          });
    if (rc != SKR_OK) return rc;
    SKR_HIP(mk.mark());
    const int n_wg = batch_workgroups(n);
    hipLaunchKernelGGL(sc_batch_kernel, dim3(n_wg), dim3(HW * 64), 0, st, a->M, pred, a->users, a->items, a->ku, a->ki, n, U, I,
                       1.0f / (1.0f - a->dropout), a->dropout, a->seed, a->step, a->reg, 0.5f / static_cast<float>(n), w + W.Gx, w + W.lossb,
                       w + W.part);
    hipLaunchKernelGGL(part_reduce_kernel<PRED>, dim3((PRED + 255) / 256), dim3(256), 0, st, w + W.part, n_wg, a->grad + N * D);
    hipLaunchKernelGGL(sc_loss_kernel, dim3(1), dim3(1024), 0, st, w + W.lossb, n, a->reg, a->loss);
    SKR_LAUNCH_CHECK();
    SKR_HIP(mk.mark());
    // ---- the g_x rows into the cleared table (the gradient itself when there is no propagation)
    float* G = L == 0 ? a->grad : a->G;
    SKR_HIP(hipMemsetAsync(G, 0, static_cast<size_t>(N) * D * sizeof(float), st));
    hipLaunchKernelGGL(rank_lists_kernel<256>, dim3((2 * n + 255) / 256), dim3(256), 0, st, a->users, a->items, n, ordu, ordi);
    const int blocks = (n + HW - 1) / HW;
    hipLaunchKernelGGL(sc_seg_add_kernel, dim3(2 * blocks), dim3(HW * 64), 0, st, G, a->users, a->items, ordu, ordi, n, U, I, blocks, w + W.Gx);
    SKR_LAUNCH_CHECK();
    SKR_HIP(mk.mark());
    // ---- backward: acc = G; L times acc = (A-hat')^T acc + G; the last product writes acc / (L + 1) into the gradient
    rc = chain_backward(a->plan_a, a->plan_at, G, UO, L, a->ping, a->grad,
                        [&](const skr_spmm_plan* plan, const float* X, const skr_spmm_epilogue& ep, bool item_half) {
                            return skr_spmm_plan_run_dropped(plan, X, D, &ep, item_half ? a->keep_bi : a->keep_bu, a->edge_scale, stream);
                        });
    if (rc != SKR_OK) return rc;
    SKR_HIP(mk.mark());
    SKR_HIP(mk.finish());
    return SKR_OK;
}

}  // namespace

extern "C" {

int skr_selfcf_keeps(const int32_t* d_perm, int64_t nnz, const uint8_t* d_k1, const uint8_t* d_k2, float rate, uint64_t seed, uint64_t step,
                     uint8_t* d_fu, uint8_t* d_fi, uint8_t* d_bu, uint8_t* d_bi, void* stream) {
    SKR_REQUIRE(nnz >= 0 && nnz < (int64_t{1} << 31), "skr_selfcf_keeps: 0 <= nnz < 2^31 (got %lld)", static_cast<long long>(nnz));
    if (nnz == 0) return SKR_OK;
    SKR_REQUIRE(d_perm && d_fu && d_fi && d_bu && d_bi, "skr_selfcf_keeps: NULL argument");
    SKR_REQUIRE((d_k1 == nullptr) == (d_k2 == nullptr), "skr_selfcf_keeps: k1 and k2 are handed in together or not at all");
    SKR_REQUIRE(d_k1 || (rate >= 0.0f && rate < 1.0f), "skr_selfcf_keeps: 0 <= rate < 1 (got %g)", rate);
    hipLaunchKernelGGL(sc_keeps_kernel, dim3(static_cast<unsigned>((nnz + 255) / 256)), dim3(256), 0, skr::as_stream(stream), d_perm, nnz, d_k1,
                       d_k2, rate, seed, step, d_fu, d_fi, d_bu, d_bi);
    SKR_LAUNCH_CHECK();
    return SKR_OK;
}

size_t skr_selfcf_workspace(int n, int n_layers) {
    if (n <= 0 || n > MAXB || n_layers < 0 || n_layers > MAXL) return 0;
    return static_cast<size_t>(step_layout(n).total) * sizeof(float);
}

int skr_selfcf_step(const skr_selfcf_step_args* args, void* stream) { return run_step(args, stream, nullptr); }

int skr_selfcf_step_timed(const skr_selfcf_step_args* args, void* stream, float* h_ms) {
    SKR_REQUIRE(h_ms != nullptr, "skr_selfcf_step_timed: NULL argument");
    return run_step(args, stream, h_ms);
}

int skr_selfcf_queries(const float* d_pred, const float* d_M, int n_users, int n_items, float* d_Q, float* d_item_bias, float* d_user_const,
                       void* stream) {
    SKR_REQUIRE(d_pred && d_M && d_Q && d_item_bias && d_user_const, "skr_selfcf_queries: NULL argument");
    SKR_REQUIRE(n_users > 0 && n_items > 0, "skr_selfcf_queries: n_users = %d, n_items = %d", n_users, n_items);
    const int64_t N = static_cast<int64_t>(n_users) + n_items;
    const int64_t wgs = std::min<int64_t>((N + HW - 1) / HW, 4096);
    hipLaunchKernelGGL(sc_queries_kernel, dim3(static_cast<unsigned>(wgs)), dim3(HW * 64), 0, skr::as_stream(stream), d_pred, d_M, n_users,
                       n_items, d_Q, d_item_bias, d_user_const);
    SKR_LAUNCH_CHECK();
    return SKR_OK;
}

}  // extern "C"
