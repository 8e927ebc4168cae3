// bm3.hip -- BM3 (Bootstrap Latent Representations for Multi-modal Recommendation, WWW 2023): a LightGCN encoder with the
// item rows' residual, trainable item feature tables projected to the embedding width, a shared predictor and six cosine
// terms against dropped-out, detached targets, plus the Frobenius norms of the whole propagated tables: the gather-and-project
// product and its backward, the batch kernel, the host entry that issues one training step, and the factor rows of the ranking.
//
// Replaces the stock torch ops the reference issues per step (no native code there):
//   recommender/BM3.py:142-153  n_layers torch.sparse.mm on the square adjacency, the mean of the layers, + h on the item rows
//   recommender/BM3.py:157-162  text_trs / image_trs on the WHOLE [I, F] tables (here: on the batch's rows only)
//   recommender/BM3.py:164-204  F.dropout of the four detached targets, the predictor on four row sets, the six cosine terms,
//                               EmbLoss, and autograd's backward through all of it (the dense [I, F] feature gradients included)
//   recommender/BM3.py:206-210  full_sort_predict: the predictor on both tables
//
// Layout: see include/skrec_hip.h, section J.
//
// Launches of a step:
//   clear            the feature-gradient rows the previous step wrote
//   2L plan runs     X_k = A-hat X_(k-1): user rows from A, item rows from A^T; the mean M rides in the accum epilogue
//   addh_sumsq       M_i += X0_i; the sums of squares of M_u and M_i as 512 partial sums per side; norm_final adds them
//   project          per present modality: Y = X[items] W^T + b, 16-row tiles on v_mfma_f32_16x16x4_f32
//   batch            per 64 batch rows and row set (M_u[u], M_i[i], T[i], V[i]): p = W x + b on the matrix pipe, the set's one
//                    or two dropped-out targets, the cosines, g_p, g_x = W^T g_p, dW and db as the workgroup's partial sums
//   pred_reduce      the partial sums in workgroup order;  loss: the components
//   rank             the positions of the user and item lists sorted by (id, position)
//   per modality     trs_bgrad (db), trs_wgrad (dW = dY^T X[items]: a workgroup owns 64 columns and walks the batch in order),
//                    seg_rows (g_j per distinct item, in batch order), feat_grad (dX[j] = g_j W, one writer per distinct item)
//   reg_fill         G = reg / (I |M_side|) M over all U + I rows (zero where the norm is zero);  seg_add: the g_x rows on top
//   2L plan runs     acc = G; acc = A-hat acc + G (the addend epilogue); the last writes acc / (L + 1) into the gradient
//   addh_grad        the item rows' + h path: grad_i += G_i
//
// The MFMA operand mapping is mfma_tile.h's k = 16 g + kk.  The cosine, its clamp and its backward are selfcf.hip's
// expressions.
//
// Determinism: there is no floating-point atomic anywhere in the step; every sum has a fixed order.
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
constexpr int MAXB = SKR_BM3_MAX_BATCH;
constexpr int MAXL = SKR_BM3_MAX_LAYERS;
constexpr int MAXF = SKR_BM3_MAX_FEAT;
constexpr int PRED = SKR_BM3_PRED_FLOATS;
constexpr int NB = 512;        // partial sums per side of the sums of squares
constexpr float COS_EPS = 1e-8f;   // F.cosine_similarity's default

// ------------------------------------------------------------------------------------------------
// the device draws on their own (tests)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bm_draws_kernel(const int32_t* __restrict__ ids, int n, int table, float rate, uint64_t seed,
                                                       uint64_t step, uint8_t* __restrict__ out) {
    const int64_t e = blockIdx.x * static_cast<int64_t>(256) + threadIdx.x;
    if (e >= static_cast<int64_t>(n) * D) return;
    const int id = ids[e >> 6];
    out[e] = id >= 0 && draw_keep(seed, step, static_cast<uint64_t>(table), static_cast<uint64_t>(id) * D + (e & 63), rate) ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------
// the gather-and-project product
// ------------------------------------------------------------------------------------------------
// Y[b] = X[ids[b], :] W^T + bias: a wavefront owns 16 batch rows and walks the ld columns 64 at a time; lane (r, g) carries
// the columns k0 + 16 g + kk of row r.  ld is a multiple of 4 and the columns beyond feat_dim are zero in X and in W.
__global__ __launch_bounds__(HW * 64) void bm_project_kernel(const float* __restrict__ X, int n_rows, int ld, const float* __restrict__ trs,
                                                             const int32_t* __restrict__ ids, int n, float* __restrict__ Y) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
    const int b0 = blockIdx.x * TB + wv * 16;
    if (b0 >= n) return;
    const int bA = b0 + r;
    const int64_t id = bA < n ? checked(ids[bA], n_rows) : -1;
    const float* __restrict__ xrow = X + (id < 0 ? 0 : id) * ld;
    const float* __restrict__ bias = trs + static_cast<int64_t>(D) * ld;
    const float4 zero4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    f32x4 acc[4];
    zero_acc(acc);
    for (int k0 = 0; k0 < ld; k0 += 64) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int kq = k0 + 16 * g + 4 * q;
            const bool in = kq < ld;
            const float4 a = in && id >= 0 ? *reinterpret_cast<const float4*>(xrow + kq) : zero4;
            float4 w[4];
#pragma unroll
            for (int nb = 0; nb < 4; ++nb)
                w[nb] = in ? *reinterpret_cast<const float4*>(trs + static_cast<int64_t>(nb * 16 + r) * ld + kq) : zero4;
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) acc[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, w[nb].x, acc[nb], 0, 0, 0);
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) acc[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, w[nb].y, acc[nb], 0, 0, 0);
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) acc[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, w[nb].z, acc[nb], 0, 0, 0);
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) acc[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, w[nb].w, acc[nb], 0, 0, 0);
        }
    }
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        const int bD = b0 + 4 * g + rr;
        if (bD >= n) continue;
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) Y[static_cast<int64_t>(bD) * D + nb * 16 + r] = acc[nb][rr] + bias[nb * 16 + r];
    }
}

// db[o] = sum_b dY[b][o], in batch order
__global__ __launch_bounds__(D) void bm_trs_bgrad_kernel(const float* __restrict__ dY, int n, float* __restrict__ db) {
    float t = 0.0f;
    for (int b = 0; b < n; ++b) t += dY[static_cast<int64_t>(b) * D + threadIdx.x];
    db[threadIdx.x] = t;
}

// dW[o][f] = sum_b dY[b][o] X[ids[b]][f]: a wavefront owns 16 columns f and walks the batch in order, four rows per MFMA
// (A = dY^T, B = the gathered rows); acc[mb][rr] = dW[16 mb + 4 g + rr][f0 + r]
__global__ __launch_bounds__(HW * 64) void bm_trs_wgrad_kernel(const float* __restrict__ X, int n_rows, int ld, const int32_t* __restrict__ ids,
                                                               int n, const float* __restrict__ dY, float* __restrict__ dW) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
    const int f = blockIdx.x * 64 + wv * 16 + r;
    const bool fin = f < ld;
    f32x4 acc[4];
    zero_acc(acc);
    for (int k0 = 0; k0 < n; k0 += 16) {                       // four MFMA steps per trip: their loads are issued together
        float a[4][4], b[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int bk = k0 + 4 * j + g;
            const bool in = bk < n;
            const int64_t id = in ? checked(ids[bk], n_rows) : -1;
            b[j] = id >= 0 && fin ? X[id * ld + f] : 0.0f;
#pragma unroll
            for (int mb = 0; mb < 4; ++mb) a[j][mb] = in ? dY[static_cast<int64_t>(bk) * D + mb * 16 + r] : 0.0f;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int mb = 0; mb < 4; ++mb) acc[mb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j][mb], b[j], acc[mb], 0, 0, 0);
        }
    }
    if (!fin) return;
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) {
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) dW[static_cast<int64_t>(mb * 16 + 4 * g + rr) * ld + f] = acc[mb][rr];
    }
}

// Gseg[rk] = the sum of the dY rows whose item is the one at rank rk, in rank (= batch) order, head[rk] = that item -- at
// the first rank of every distinct valid item; zeros and -1 at every other rank
__global__ __launch_bounds__(HW * 64) void bm_seg_rows_kernel(const int32_t* __restrict__ items, const int32_t* __restrict__ order, int n, int I,
                                                              const float* __restrict__ dY, float* __restrict__ Gseg, int32_t* __restrict__ head) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int rk = blockIdx.x * HW + wv;
    if (rk >= n) return;
    const int id = items[order[rk]];
    const bool first = id >= 0 && id < I && !(rk > 0 && items[order[rk - 1]] == id);
    float acc = 0.0f;
    if (first) {
        for (int k = rk; k < n; ++k) {
            const int o = order[k];
            if (items[o] != id) break;
            acc += dY[static_cast<int64_t>(o) * D + lane];
        }
    }
    Gseg[static_cast<int64_t>(rk) * D + lane] = acc;
    if (lane == 0) head[rk] = first ? id : -1;
}

// ------------------------------------------------------------------------------------------------
// + h and the sums of squares
// ------------------------------------------------------------------------------------------------
// blocks [0, NB): the user rows, [NB, 2 NB): the item rows, which first get M_i += X0_i.  Wavefront w of a side walks the
// rows w, w + NB HW, ...; part[block] = the block's sum, its four wavefronts added in order
__global__ __launch_bounds__(HW * 64) void bm_addh_sumsq_kernel(float* __restrict__ M, const float* __restrict__ X0, int U, int I,
                                                                float* __restrict__ part) {
    __shared__ float s[HW];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const bool item = blockIdx.x >= NB;
    const int64_t rows = item ? I : U, base = item ? U : 0;
    float acc = 0.0f;
    const int64_t stride = static_cast<int64_t>(NB) * HW;
    for (int64_t row0 = static_cast<int64_t>(item ? blockIdx.x - NB : blockIdx.x) * HW + wv; row0 < rows; row0 += 4 * stride) {
        float v[4];                                            // four rows per trip: their loads are issued together
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t row = row0 + j * stride, e = (base + row) * D + lane;
            v[j] = row < rows ? M[e] : 0.0f;
            if (item && row < rows) v[j] += X0[e];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t row = row0 + j * stride;
            if (item && row < rows) M[(base + row) * D + lane] = v[j];
            acc += v[j] * v[j];
        }
    }
    acc = skr::wave_sum(acc);
    if (lane == 0) s[wv] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = ((s[0] + s[1]) + s[2]) + s[3];
}

// ss[0] = |M_u|^2, ss[1] = |M_i|^2: the NB partial sums of a side by a fixed tree
__global__ __launch_bounds__(2 * NB) void bm_norm_final_kernel(const float* __restrict__ part, float* __restrict__ ss) {
    __shared__ float s[2 * NB];
    const int t = threadIdx.x, side = t / NB, k = t % NB;
    s[t] = part[t];
    __syncthreads();
    for (int o = NB / 2; o > 0; o >>= 1) {
        if (k < o) s[side * NB + k] += s[side * NB + k + o];
        __syncthreads();
    }
    if (k == 0) ss[side] = s[side * NB];
}

// ------------------------------------------------------------------------------------------------
// batch: the predictor, the targets, the cosine terms and their backward for 64 batch rows
// ------------------------------------------------------------------------------------------------
// row set 0: x = M[users], target i_tgt;  1: x = M[U + items], target u_tgt;  2: x = T[b], targets i_tgt and t_tgt;
// 3: x = V[b], targets i_tgt and v_tgt.  A target of table k is value * keep / (1 - p).
//   P = W x + b;  c = <P, t> / (max(|P|, eps) max(|t|, eps));  g_P = -coef sum_t (t / (nP nt) - [|P| > eps] c P / nP^2)
//   g_x = W^T g_P -> Gx [4][n4][64];  dW += g_P x^T, db += g_P
// lossb [6][n4]: the cosines of (set 0), (set 1), (set 2: i_tgt, t_tgt), (set 3: i_tgt, v_tgt).
// part [gridDim.x][PRED]: the workgroup's dW and db.
struct BatchParams {
    const float* M;
    const float* pred;
    const float* Yt;               // T at the batch rows, NULL when there is no text block
    const float* Yv;
    const int32_t* users;
    const int32_t* items;
    const uint8_t* keep[4];
    int n, U, I;
    int64_t n4;
    float inv_keep, p_drop, coef_graph, coef_modal;
    uint64_t seed, step;
    float* Gx;
    float* lossb;
    float* part;
};

__device__ __forceinline__ float target_value(const BatchParams& p, int kind, int bD, int64_t uD, int64_t iD, int col) {
    const int64_t f = static_cast<int64_t>(bD) * D + col;
    const uint64_t node = static_cast<uint64_t>(kind == SKR_BM3_DRAW_USER ? uD : iD);
    const bool kf = p.keep[kind] ? p.keep[kind][f] != 0 : draw_keep(p.seed, p.step, static_cast<uint64_t>(kind), node * D + col, p.p_drop);
    if (!kf) return 0.0f;
    float v;
    if (kind == SKR_BM3_DRAW_USER) v = p.M[uD * D + col];
    else if (kind == SKR_BM3_DRAW_ITEM) v = p.M[(p.U + iD) * D + col];
    else if (kind == SKR_BM3_DRAW_TEXT) v = p.Yt[f];
    else v = p.Yv[f];
    return v * p.inv_keep;
}

__global__ __launch_bounds__(HW * 64) void bm_batch_kernel(BatchParams p) {
    __shared__ __attribute__((aligned(16))) float sW[D * LDP];      // sW[out][in]
    __shared__ __attribute__((aligned(16))) float sWT[D * LDP];     // sWT[in][out]
    __shared__ __attribute__((aligned(16))) float sG[TB * LDP];     // g_P[row][out]
    __shared__ __attribute__((aligned(16))) float sGT[D * LDP];     // g_P^T[out][row]
    __shared__ __attribute__((aligned(16))) float sXT[D * LDP];     // x^T[in][row]
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
    const int n = p.n, U = p.U, I = p.I;
    for (int idx = threadIdx.x; idx < D * 16; idx += HW * 64) {
        const int row = idx >> 4, c4 = idx & 15;
        const float4 v = *reinterpret_cast<const float4*>(p.pred + row * D + c4 * 4);
        *reinterpret_cast<float4*>(sW + row * LDP + c4 * 4) = v;
        sWT[(c4 * 4 + 0) * LDP + row] = v.x;
        sWT[(c4 * 4 + 1) * LDP + row] = v.y;
        sWT[(c4 * 4 + 2) * LDP + row] = v.z;
        sWT[(c4 * 4 + 3) * LDP + row] = v.w;
    }
    const float* __restrict__ bias = p.pred + D * D;
    const int b0 = blockIdx.x * TB + wv * 16;
    f32x4 dW[4];
    zero_acc(dW);
    float db = 0.0f;
    __syncthreads();
    for (int set = 0; set < 4; ++set) {
        if ((set == 2 && p.Yt == nullptr) || (set == 3 && p.Yv == nullptr)) continue;
        const int n_tgt = set < 2 ? 1 : 2;
        const int kind0 = set == 1 ? SKR_BM3_DRAW_USER : SKR_BM3_DRAW_ITEM;
        const int kind1 = set == 2 ? SKR_BM3_DRAW_TEXT : SKR_BM3_DRAW_IMAGE;
        const int slot = set < 2 ? set : 2 * set - 2;
        const float coef = set < 2 ? p.coef_graph : p.coef_modal;
        // ---- A layout: lane (r, g) holds columns [16 g, 16 g + 16) of the wavefront's row r
        const int bA = b0 + r;
        const int64_t uA = bA < n ? checked(p.users[bA], U) : -1, iA = bA < n ? checked(p.items[bA], I) : -1;
        const bool validA = uA >= 0 && iA >= 0;
        float xa[16];
        if (set < 2) load_row_a(xa, p.M, validA ? (set == 0 ? uA : U + iA) : -1, g);
        else load_row_a(xa, set == 2 ? p.Yt : p.Yv, validA ? bA : -1, g);
        f32x4 P[4];
        zero_acc(P);
        tile_product<LDP>(P, xa, sW, r, g);
        // ---- D layout: lane (r, g) holds column 16 nb + r of the rows 4 g + rr
        f32x4 gp[4];
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int bD = b0 + 4 * g + rr;
            const bool in = bD < n;
            const int64_t uD = in ? checked(p.users[bD], U) : -1, iD = in ? checked(p.items[bD], I) : -1;
            const bool valid = uD >= 0 && iD >= 0;
            float pp = 0.0f, gacc[4];
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) {
                P[nb][rr] += bias[nb * 16 + r];
                pp += P[nb][rr] * P[nb][rr];
                gacc[nb] = 0.0f;
            }
            pp = sum16(pp);
            const float nPr = sqrtf(pp), nP = fmaxf(nPr, COS_EPS);
            for (int t = 0; t < n_tgt; ++t) {
                const int kind = t == 0 ? kind0 : kind1;
                float tv[4], dot = 0.0f, tt = 0.0f;
#pragma unroll
                for (int nb = 0; nb < 4; ++nb) {
                    const float tval = valid ? target_value(p, kind, bD, uD, iD, nb * 16 + r) : 0.0f;
                    tv[nb] = tval;
                    dot += P[nb][rr] * tval;
                    tt += tval * tval;
                }
                dot = sum16(dot); tt = sum16(tt);
                const float nT = fmaxf(sqrtf(tt), COS_EPS);
                const float c = valid ? dot / (nP * nT) : 0.0f;
                if (r == 0 && in) p.lossb[static_cast<int64_t>(slot + t) * p.n4 + bD] = c;
#pragma unroll
                for (int nb = 0; nb < 4; ++nb) {
                    float gv = 0.0f;
                    if (valid) {
                        gv = tv[nb] / (nP * nT);
                        if (nPr > COS_EPS) gv -= c * P[nb][rr] / (nP * nP);     // (a clamped norm has zero slope)
                        gv = -coef * gv;
                    }
                    gacc[nb] += gv;
                }
            }
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) gp[nb][rr] = gacc[nb];
        }
        __syncthreads();                                       // the previous set's products still read the images
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
            for (int nb = 0; nb < 4; ++nb) p.Gx[(static_cast<int64_t>(set) * p.n4 + bD) * D + nb * 16 + r] = gx[nb][rr];
        }
        float slab[16];
        load_slab<LDP>(slab, sGT, wv * 16 + r, g);
        tile_product<LDP>(dW, slab, sXT, r, g);
        if (threadIdx.x < D) db += column_sum<LDP>(sGT, threadIdx.x);
    }
    float* out = p.part + static_cast<int64_t>(blockIdx.x) * PRED;
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) {
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) out[(wv * 16 + 4 * g + rr) * D + nb * 16 + r] = dW[nb][rr];
    }
    if (threadIdx.x < D) out[D * D + threadIdx.x] = db;
}

// loss[0] = the graph cosines, loss[1] = cl_weight * the modal cosines, loss[2] = reg (|M_u| + |M_i|) / I, loss[3] = their sum
__global__ __launch_bounds__(1024) void bm_loss_kernel(const float* __restrict__ lossb, int n, int64_t n4, int has_t, int has_v, float cl,
                                                       float reg, int I, const float* __restrict__ ss, float* __restrict__ loss) {
    __shared__ float s[1024];
    const int t = threadIdx.x;
    float a[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    for (int k = t; k < n; k += 1024) {
        a[0] += lossb[k];
        a[1] += lossb[n4 + k];
        if (has_t) { a[2] += lossb[2 * n4 + k]; a[3] += lossb[3 * n4 + k]; }
        if (has_v) { a[4] += lossb[4 * n4 + k]; a[5] += lossb[5 * n4 + k]; }
    }
    float m[6];
    const float fn = static_cast<float>(n);
    for (int j = 0; j < 6; ++j) m[j] = 1.0f - block_sum_1024(a[j], s) / fn;
    if (t == 0) {
        const float graph = m[0] + m[1];
        float modal = 0.0f;
        if (has_t) modal += m[2] + m[3];
        if (has_v) modal += m[4] + m[5];
        modal *= cl;
        const float regl = reg * (sqrtf(ss[0]) + sqrtf(ss[1])) / static_cast<float>(I);
        loss[0] = graph;
        loss[1] = modal;
        loss[2] = regl;
        loss[3] = (graph + modal) + regl;
    }
}

// ------------------------------------------------------------------------------------------------
// the gradient with respect to M: the dense regulariser, then the g_x rows
// ------------------------------------------------------------------------------------------------
// G_side = reg / (I |M_side|) M_side on every row; exactly zero where the norm is zero
__global__ __launch_bounds__(256) void bm_reg_fill_kernel(const float* __restrict__ M, int64_t n_user4, int64_t n_all4, float reg, int I,
                                                          const float* __restrict__ ss, float* __restrict__ G) {
    const float fi = static_cast<float>(I);
    const float cu = ss[0] > 0.0f ? reg / (fi * sqrtf(ss[0])) : 0.0f, ci = ss[1] > 0.0f ? reg / (fi * sqrtf(ss[1])) : 0.0f;
    for (int64_t e = blockIdx.x * static_cast<int64_t>(256) + threadIdx.x; e < n_all4; e += static_cast<int64_t>(gridDim.x) * 256) {
        const float c = e < n_user4 ? cu : ci;
        const float4 v = reinterpret_cast<const float4*>(M)[e];
        reinterpret_cast<float4*>(G)[e] = make_float4(c * v.x, c * v.y, c * v.z, c * v.w);
    }
}

// G[id] += the sum of the g_x rows whose list entry is id, in rank order, by the wavefront of the id's first rank: one
// writer per distinct id.  Blocks [0, blocks_u) walk the user list (row set 0), the others the item list (row set 1).
__global__ __launch_bounds__(HW * 64) void bm_seg_add_kernel(float* __restrict__ G, const int32_t* __restrict__ users,
                                                             const int32_t* __restrict__ items, const int32_t* __restrict__ order_u,
                                                             const int32_t* __restrict__ order_i, int n, int64_t n4, int U, int I, int blocks_u,
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
    const float* src = Gx + (user ? 0 : n4 * D);
    float acc = 0.0f;
    for (int k = rk; k < n; ++k) {
        const int o = order[k];
        if (ids[o] != id) break;
        acc += src[static_cast<int64_t>(o) * D + lane];
    }
    const int64_t e = (static_cast<int64_t>(user ? 0 : U) + id) * D + lane;
    G[e] = G[e] + acc;
}

// the item rows' + h path: grad_i += G_i (grad and G are the same table when there is no propagation)
__global__ __launch_bounds__(256) void bm_addh_grad_kernel(float* grad, const float* G, int64_t n) {
    for (int64_t e = blockIdx.x * static_cast<int64_t>(256) + threadIdx.x; e < n; e += static_cast<int64_t>(gridDim.x) * 256) {
        const float v = grad[e], w = G[e];
        grad[e] = v + w;
    }
}

// ------------------------------------------------------------------------------------------------
// ranking: W M_r + b for every row
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(HW * 64) void bm_queries_kernel(const float* __restrict__ pred, const float* __restrict__ M, int U, int I,
                                                             float* __restrict__ Qu, float* __restrict__ Qi) {
    __shared__ float sT[D * D];        // sT[k][j] = W[j][k]
    __shared__ float sb[D];
    for (int idx = threadIdx.x; idx < D * D; idx += HW * 64) {
        const int k = idx >> 6, j = idx & 63;
        sT[idx] = pred[j * D + k];
    }
    if (threadIdx.x < D) sb[threadIdx.x] = pred[D * D + threadIdx.x];
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t N = static_cast<int64_t>(U) + I;
    for (int64_t row = static_cast<int64_t>(blockIdx.x) * HW + wv; row < N; row += static_cast<int64_t>(gridDim.x) * HW) {
        const float m = M[row * D + lane];
        float q = 0.0f;
#pragma unroll 16
        for (int k = 0; k < D; ++k) q = fmaf(sT[k * D + lane], __shfl(m, k, 64), q);
        q += sb[lane];
        if (row < U) Qu[row * D + lane] = q;
        else Qi[(row - U) * D + lane] = q;
    }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
struct StepLayout {            // float offsets into the step's workspace
    int64_t Gx, Y, lossb, part, ordu, ordi, Gseg, head, npart, ss, total;
};

inline int batch_workgroups(int n) { return (n + TB - 1) / TB; }

inline StepLayout step_layout(int n) {
    StepLayout L;
    const int64_t n4 = round4(n);
    int64_t o = 0;
    L.Gx = o; o += 4 * n4 * D;
    L.Y = o; o += 2 * n4 * D;
    L.lossb = o; o += 6 * n4;
    L.part = o; o += static_cast<int64_t>(batch_workgroups(n)) * PRED;
    L.ordu = o; o += n4;
    L.ordi = o; o += n4;
    L.Gseg = o; o += n4 * D;
    L.head = o; o += n4;
    L.npart = o; o += 2 * NB;
    L.ss = o; o += 4;
    L.total = o;
    return L;
}

int check_feature(const char* who, int F, int ld) {
    SKR_REQUIRE(F >= 1 && F <= MAXF, "%s: 1 <= feat_dim <= %d (got %d)", who, MAXF, F);
    SKR_REQUIRE(ld >= F && ld % 4 == 0 && ld <= MAXF, "%s: feat_ld = %d must be a multiple of 4, >= feat_dim = %d and <= %d", who, ld, F, MAXF);
    return SKR_OK;
}

int launch_project(const float* X, int n_rows, int ld, const float* trs, const int32_t* ids, int n, float* Y, hipStream_t st) {
    hipLaunchKernelGGL(bm_project_kernel, dim3(batch_workgroups(n)), dim3(HW * 64), 0, st, X, n_rows, ld, trs, ids, n, Y);
    SKR_LAUNCH_CHECK();
    return SKR_OK;
}

int run_step(const skr_bm3_step_args* a, void* stream, float* h_ms) {
    SKR_REQUIRE(a, "skr_bm3_step: NULL argument");
    const int U = a->n_users, I = a->n_items, n = a->n, L = a->n_layers;
    SKR_REQUIRE(a->params && a->users && a->items && a->M && a->grad && a->loss && a->work, "skr_bm3_step: NULL argument");
    SKR_REQUIRE(U > 0 && I > 0 && n >= 0 && n <= MAXB, "skr_bm3_step: n_users = %d, n_items = %d, n = %d (at most %d rows)", U, I, n, MAXB);
    SKR_REQUIRE(a->dim >= 1 && a->dim <= D, "skr_bm3_step: 1 <= dim <= 64 (got %d); rows are 64 floats, zero-padded", a->dim);
    SKR_REQUIRE(L >= 0 && L <= MAXL, "skr_bm3_step: 0 <= n_layers <= %d (got %d)", MAXL, L);
    SKR_REQUIRE(L == 0 || (a->plan_a && a->plan_at), "skr_bm3_step: n_layers > 0 needs both plans");
    SKR_REQUIRE(L == 0 || a->G, "skr_bm3_step: n_layers > 0 needs the table G");
    SKR_REQUIRE(L < 2 || (a->ping[0] && a->ping[1]), "skr_bm3_step: n_layers > 1 needs both ping tables");
    SKR_REQUIRE(a->dropout >= 0.0f && a->dropout < 1.0f && a->reg >= 0.0f && a->cl_weight >= 0.0f,
                "skr_bm3_step: dropout = %g (0 <= dropout < 1), reg = %g, cl_weight = %g", a->dropout, a->reg, a->cl_weight);
    const int n_keep = (a->keep[0] != nullptr) + (a->keep[1] != nullptr) + (a->keep[2] != nullptr) + (a->keep[3] != nullptr);
    SKR_REQUIRE(n_keep == 0 || n_keep == 4, "skr_bm3_step: the four keep arrays are handed in together or not at all");
    SKR_REQUIRE(a->n_clear >= 0 && a->n_clear <= MAXB && (a->n_clear == 0 || a->clear_items),
                "skr_bm3_step: n_clear = %d (at most %d ids, clear_items not NULL)", a->n_clear, MAXB);
    uintptr_t align = reinterpret_cast<uintptr_t>(a->params) | reinterpret_cast<uintptr_t>(a->grad) | reinterpret_cast<uintptr_t>(a->work) |
                      reinterpret_cast<uintptr_t>(a->M) | reinterpret_cast<uintptr_t>(a->G) | reinterpret_cast<uintptr_t>(a->ping[0]) |
                      reinterpret_cast<uintptr_t>(a->ping[1]);
    for (int m = 0; m < 2; ++m) {
        if (a->feat_dim[m] == 0) continue;
        const int rc = check_feature("skr_bm3_step", a->feat_dim[m], a->feat_ld[m]);
        if (rc != SKR_OK) return rc;
        SKR_REQUIRE(a->trs[m] && a->feat[m] && a->trs_grad[m] && a->feat_grad[m], "skr_bm3_step: a present modality needs its four tables");
        align |= reinterpret_cast<uintptr_t>(a->trs[m]) | reinterpret_cast<uintptr_t>(a->feat[m]) | reinterpret_cast<uintptr_t>(a->trs_grad[m]) |
                 reinterpret_cast<uintptr_t>(a->feat_grad[m]);
    }
    if (n == 0) return SKR_OK;
    const StepLayout W = step_layout(n);
    SKR_REQUIRE(a->work_bytes >= static_cast<size_t>(W.total) * sizeof(float), "skr_bm3_step: work holds %zu bytes, skr_bm3_workspace(%d) asks for %zu",
                a->work_bytes, n, static_cast<size_t>(W.total) * sizeof(float));
    SKR_REQUIRE((align & 15) == 0, "skr_bm3_step: the tables and work must be 16-byte aligned");
    hipStream_t st = skr::as_stream(stream);
    float* w = static_cast<float*>(a->work);
    int32_t* ordu = reinterpret_cast<int32_t*>(w + W.ordu);
    int32_t* ordi = reinterpret_cast<int32_t*>(w + W.ordi);
    int32_t* head = reinterpret_cast<int32_t*>(w + W.head);
    const int64_t n4 = round4(n);
    const int64_t UO = static_cast<int64_t>(U) * D, N = static_cast<int64_t>(U) + I;
    const float* pred = a->params + N * D;
    float* Y[2] = {a->feat_dim[0] ? w + W.Y : nullptr, a->feat_dim[1] ? w + W.Y + n4 * D : nullptr};
    StepTimer<SKR_BM3_GROUPS + 1> mk(h_ms, st);        // h_ms: an event after every launch group; otherwise nothing
    SKR_HIP(mk.mark());
    if (a->n_clear > 0 && (a->feat_dim[0] || a->feat_dim[1])) {
        ClearParams cp = {{a->feat_dim[0] ? a->feat_grad[0] : nullptr, a->feat_dim[1] ? a->feat_grad[1] : nullptr}, {a->feat_ld[0], a->feat_ld[1]}};
        hipLaunchKernelGGL(clear_rows_kernel<256>, dim3(a->n_clear, 2), dim3(256), 0, st, cp, a->clear_items, I);
        SKR_LAUNCH_CHECK();
    }
    // ---- forward (BM3.py:145-151): the layer means of X_k = A-hat X_(k-1)
    const auto product = [&](const skr_spmm_plan* plan, const float* X, const skr_spmm_epilogue& ep, bool) {
        return skr_spmm_plan_run_ex(plan, X, D, &ep, nullptr, nullptr, stream);
    };
    int rc = mean_forward(a->plan_a, a->plan_at, a->params, UO, N, L, a->ping, a->M, st, product);
    if (rc != SKR_OK) return rc;
    SKR_HIP(mk.mark());
    // ---- + h (BM3.py:153) and the Frobenius norms of the whole tables (BM3.py:66-71)
    hipLaunchKernelGGL(bm_addh_sumsq_kernel, dim3(2 * NB), dim3(HW * 64), 0, st, a->M, a->params, U, I, w + W.npart);
    hipLaunchKernelGGL(bm_norm_final_kernel, dim3(1), dim3(2 * NB), 0, st, w + W.npart, w + W.ss);
    SKR_LAUNCH_CHECK();
    SKR_HIP(mk.mark());
    for (int m = 0; m < 2; ++m) {
        if (a->feat_dim[m] == 0) continue;
        const int rc = launch_project(a->feat[m], I, a->feat_ld[m], a->trs[m], a->items, n, Y[m], st);
        if (rc != SKR_OK) return rc;
    }
    SKR_HIP(mk.mark());
    const int n_wg = batch_workgroups(n);
    BatchParams bp = {};
    bp.M = a->M; bp.pred = pred; bp.Yt = Y[1]; bp.Yv = Y[0]; bp.users = a->users; bp.items = a->items;
    for (int k = 0; k < 4; ++k) bp.keep[k] = a->keep[k];
    bp.n = n; bp.U = U; bp.I = I; bp.n4 = n4;
    bp.inv_keep = 1.0f / (1.0f - a->dropout); bp.p_drop = a->dropout;
    bp.coef_graph = 1.0f / static_cast<float>(n); bp.coef_modal = a->cl_weight / static_cast<float>(n);
    bp.seed = a->seed; bp.step = a->step;
    bp.Gx = w + W.Gx; bp.lossb = w + W.lossb; bp.part = w + W.part;
    hipLaunchKernelGGL(bm_batch_kernel, dim3(n_wg), dim3(HW * 64), 0, st, bp);
    hipLaunchKernelGGL(part_reduce_kernel<PRED>, dim3((PRED + 255) / 256), dim3(256), 0, st, w + W.part, n_wg, a->grad + N * D);
    hipLaunchKernelGGL(bm_loss_kernel, dim3(1), dim3(1024), 0, st, w + W.lossb, n, n4, Y[1] != nullptr ? 1 : 0, Y[0] != nullptr ? 1 : 0, a->cl_weight,
                       a->reg, I, w + W.ss, a->loss);
    SKR_LAUNCH_CHECK();
    SKR_HIP(mk.mark());
    // ---- the projection backward: dY = the g_x rows of the modality's row set (text: 2, image: 3)
    hipLaunchKernelGGL(rank_lists_kernel<256>, dim3((2 * n + 255) / 256), dim3(256), 0, st, a->users, a->items, n, ordu, ordi);
    const int blocks = (n + HW - 1) / HW;
    for (int m = 0; m < 2; ++m) {
        if (a->feat_dim[m] == 0) continue;
        const int ld = a->feat_ld[m];
        const float* dY = w + W.Gx + static_cast<int64_t>(m == 1 ? 2 : 3) * n4 * D;
        hipLaunchKernelGGL(bm_trs_bgrad_kernel, dim3(1), dim3(D), 0, st, dY, n, a->trs_grad[m] + static_cast<int64_t>(D) * ld);
        hipLaunchKernelGGL(bm_trs_wgrad_kernel, dim3((ld + 63) / 64), dim3(HW * 64), 0, st, a->feat[m], I, ld, a->items, n, dY, a->trs_grad[m]);
        hipLaunchKernelGGL(bm_seg_rows_kernel, dim3(blocks), dim3(HW * 64), 0, st, a->items, ordi, n, I, dY, w + W.Gseg, head);
        hipLaunchKernelGGL(feat_grad_kernel<HW>, dim3((n + 15) / 16, (ld + 64 * HW - 1) / (64 * HW)), dim3(HW * 64), 0, st, w + W.Gseg, head, n, ld,
                           a->trs[m], a->feat_grad[m]);
    }
    SKR_LAUNCH_CHECK();
    SKR_HIP(mk.mark());
    // ---- the gradient with respect to M: the dense regulariser on every row, the g_x rows per distinct node on top
    float* G = L == 0 ? a->grad : a->G;
    {
        const int64_t all4 = N * D / 4;
        const unsigned wgs = static_cast<unsigned>(std::min<int64_t>((all4 + 255) / 256, 8192));
        hipLaunchKernelGGL(bm_reg_fill_kernel, dim3(wgs), dim3(256), 0, st, a->M, UO / 4, all4, a->reg, I, w + W.ss, G);
    }
    hipLaunchKernelGGL(bm_seg_add_kernel, dim3(2 * blocks), dim3(HW * 64), 0, st, G, a->users, a->items, ordu, ordi, n, n4, U, I, blocks, w + W.Gx);
    SKR_LAUNCH_CHECK();
    SKR_HIP(mk.mark());
    // ---- backward: acc = G; L times acc = A-hat acc + G (A-hat is symmetric); the last product writes acc / (L + 1) into
    // the gradient; then the item rows' + h path
    {
        rc = chain_backward(a->plan_a, a->plan_at, G, UO, L, a->ping, a->grad, product);
        if (rc != SKR_OK) return rc;
        const int64_t ni = static_cast<int64_t>(I) * D;
        const unsigned wgs = static_cast<unsigned>(std::min<int64_t>((ni + 255) / 256, 8192));
        hipLaunchKernelGGL(bm_addh_grad_kernel, dim3(wgs), dim3(256), 0, st, a->grad + UO, G + UO, ni);
        SKR_LAUNCH_CHECK();
    }
    SKR_HIP(mk.mark());
    SKR_HIP(mk.finish());
    return SKR_OK;
}

}  // namespace

extern "C" {

int skr_bm3_project(const float* d_X, int n_rows, int feat_dim, int feat_ld, const float* d_trs, const int32_t* d_ids, int n, float* d_Y,
                    void* stream) {
    SKR_REQUIRE(d_X && d_trs && d_ids && d_Y, "skr_bm3_project: NULL argument");
    SKR_REQUIRE(n_rows > 0 && n >= 0 && n <= MAXB, "skr_bm3_project: n_rows = %d, n = %d (at most %d rows)", n_rows, n, MAXB);
    const int rc = check_feature("skr_bm3_project", feat_dim, feat_ld);
    if (rc != SKR_OK) return rc;
    SKR_REQUIRE(((reinterpret_cast<uintptr_t>(d_X) | reinterpret_cast<uintptr_t>(d_trs) | reinterpret_cast<uintptr_t>(d_Y)) & 15) == 0,
                "skr_bm3_project: the tables must be 16-byte aligned");
    if (n == 0) return SKR_OK;
    return launch_project(d_X, n_rows, feat_ld, d_trs, d_ids, n, d_Y, skr::as_stream(stream));
}

int skr_bm3_draws(const int32_t* d_ids, int n, int table, float rate, uint64_t seed, uint64_t step, uint8_t* d_out, void* stream) {
    SKR_REQUIRE(d_ids && d_out, "skr_bm3_draws: NULL argument");
    SKR_REQUIRE(n >= 0 && n <= MAXB, "skr_bm3_draws: n = %d (at most %d rows)", n, MAXB);
    SKR_REQUIRE(table >= 0 && table < 4, "skr_bm3_draws: table = %d (one of SKR_BM3_DRAW_*)", table);
    SKR_REQUIRE(rate >= 0.0f && rate < 1.0f, "skr_bm3_draws: 0 <= rate < 1 (got %g)", rate);
    if (n == 0) return SKR_OK;
    hipLaunchKernelGGL(bm_draws_kernel, dim3((n * D + 255) / 256), dim3(256), 0, skr::as_stream(stream), d_ids, n, table, rate, seed, step, d_out);
    SKR_LAUNCH_CHECK();
    return SKR_OK;
}

size_t skr_bm3_workspace(int n) {
    if (n <= 0 || n > MAXB) return 0;
    return static_cast<size_t>(step_layout(n).total) * sizeof(float);
}

int skr_bm3_step(const skr_bm3_step_args* args, void* stream) { return run_step(args, stream, nullptr); }

int skr_bm3_step_timed(const skr_bm3_step_args* args, void* stream, float* h_ms) {
    SKR_REQUIRE(h_ms != nullptr, "skr_bm3_step_timed: NULL argument");
    return run_step(args, stream, h_ms);
}

int skr_bm3_queries(const float* d_pred, const float* d_M, int n_users, int n_items, float* d_Qu, float* d_Qi, void* stream) {
    SKR_REQUIRE(d_pred && d_M && d_Qu && d_Qi, "skr_bm3_queries: NULL argument");
    SKR_REQUIRE(n_users > 0 && n_items > 0, "skr_bm3_queries: n_users = %d, n_items = %d", n_users, n_items);
    const int64_t N = static_cast<int64_t>(n_users) + n_items;
    const int64_t wgs = std::min<int64_t>((N + HW - 1) / HW, 4096);
    hipLaunchKernelGGL(bm_queries_kernel, dim3(static_cast<unsigned>(wgs)), dim3(HW * 64), 0, skr::as_stream(stream), d_pred, d_M, n_users, n_items,
                       d_Qu, d_Qi);
    SKR_LAUNCH_CHECK();
    return SKR_OK;
}

}  // extern "C"
