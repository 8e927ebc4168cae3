// mgcn.hip -- MGCN (Multi-View Graph Convolutional Network for Multimedia Recommendation, ACM MM 2023): two trainable feature
// tables projected to 64 columns over ALL items, a sigmoid purifier gate on the item embeddings, a LightGCN user-item view, two
// weighted item-item kNN graphs, a row-local attention fuser, and a loss of BPR, an L2 term on the batch's output rows and two
// normalised B x B InfoNCE terms.  Here: the dense building blocks (projection forward and backward, purifier forward and
// backward, the fuser), the batch kernels and the host entry that issues one training step.
//
// Replaces the stock torch ops the reference issues (no native code there):
//   recommender/MGCN.py:250-258  image_trs / text_trs on the whole [I, F] tables, gate_v / gate_t, the multiply
//   recommender/MGCN.py:260-289  n_ui_layers torch.sparse.mm on the square adjacency and the mean; n_layers on each item graph; R
//   recommender/MGCN.py:291-312  the fuser over all U + I rows (here: over the batch's 3 n rows in training)
//   recommender/MGCN.py:314-353  bpr_loss, InfoNCE (two [B, B] matrices; here none is formed), and autograd's backward
//
// Layout: see include/skrec_hip.h, section M.
//
// Launches of a step:
//   per modality     project (F = T W^T + b over all items), purify (g = sigmoid(F Wg^T + bg), X = E_i * g)
//   2 Lu plan runs   the layer mean M in the accum epilogue (step_common.h)
//   per modality     Ln plan runs on S_m, one run of R: Z_m = [R X_m; X_m]
//   prep, fuse       node ids of the 3 n slots (users | pos | neg, -1 where a batch row names an id out of range); the fuser
//                    at the slots, keeping what the backward needs
//   bpr, nce         BPR and L2 on the out rows; normalise, log-sum-exp, the two weighted sums of InfoNCE per term; loss
//   fuse_bwd         the row-local backward, four rows-times-W products, the weight gradients as per-workgroup partial sums
//                    added in workgroup order, rank, seg_add into the three dense gradient tables dM, dZv, dZt
//   plan runs        mean's backward chain; per modality R^T with the item rows as addend, Ln runs of S_m^T
//   per modality     purify backward (dE_i += dX g, dz, dF = dz Wg, dWg, dbg), projection backward (dW, db, dT)
//
// Every matrix product takes fp32 operands in mfma_tile.h's layouts; the fuser's run on v_mfma_f32_16x16x4_f32, the others add
// the same operands on v_mfma_f64_16x16x4_f64 ("the products' accumulators" below says why and what it buys).  Determinism: no floating-point atomic;
// every reduction over rows is split into contiguous row blocks whose partial sums are added in block order.
#include "skr_common.h"
#include "mfma_tile.h"
#include "step_common.h"
#include "dense_ops.h"

#include <algorithm>

namespace {

using namespace skr;

constexpr int D = 64;          // columns of every table
constexpr int HW = 4;          // wavefronts per workgroup
constexpr int TB = HW * 16;    // rows per workgroup of the tiled kernels
constexpr int LD = 68;         // row stride of the LDS images
constexpr int MAXB = SKR_MGCN_MAX_BATCH;
constexpr int MAXL = SKR_MGCN_MAX_LAYERS;
constexpr int MAXF = SKR_MGCN_MAX_FEAT;
constexpr int GATE = SKR_MGCN_GATE_FLOATS;
constexpr int XTY_ROWS = 256;  // the least rows of a row block of the X^T Y reductions
constexpr int XTY_BLOCKS = 64; // ... and the most row blocks above XTY_ROWS * XTY_BLOCKS rows
constexpr float INV_TAU = 5.0f;    // the reference's literal temperature 0.2 (MGCN.py:350)
constexpr float NORM_EPS = 1e-12f; // F.normalize

__device__ __forceinline__ float sigmoid(float x) { return sigmoid_neg(-x); }

// ---- the products' accumulators (mfma_tile.h: zero_acc64, mfma64, tile_product64, logits_tile64).  The operands are fp32
// everywhere, laid out as mfma_tile.h says; the projections, the gate
// products, the rows-times-W products, InfoNCE's two products and the reductions behind the weight gradients add them on
// v_mfma_f64_16x16x4_f64 -- same operand lanes as the fp32 instruction, the lane's four results are the rows g + 4 rr (not
// 4 g + rr) of column 16 nb + r -- and round once; the fuser's four products stay on the fp32 instruction.  Why: every tensor
// has elements whose first gradient lies beside Adam's eps, where the first update magnifies an error of the gradient by up to
// lr / eps, and these sums (up to 4 096 terms for a projection, all I rows for a weight gradient) are where an fp32 evaluation
// differs most from one order of summation to another.  What it buys on the golden run's first batch is small and is said
// here as measured: the root mean square error of gate_v.0.weight's gradient against float64 went from 8.6e-11 to 7.8e-11 (a
// torch-CPU fp32 evaluation: 8.9e-11) -- the fp32 roundings of the stored intermediates and of the SpMM plans remain.
// ------------------------------------------------------------------------------------------------
// dense building blocks
// ------------------------------------------------------------------------------------------------
// Y[b] = X[b, :] W^T + bias for all n rows: bm3.hip's project without the gather.  A wavefront owns 16 rows and walks the ld
// columns 64 at a time in a fixed order.
__global__ __launch_bounds__(HW * 64) void mg_project_kernel(const float* __restrict__ X, int n, int ld, const float* __restrict__ trs,
                                                             float* __restrict__ Y) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
    const int64_t b0 = static_cast<int64_t>(blockIdx.x) * TB + wv * 16;
    if (b0 >= n) return;
    const bool rin = b0 + r < n;
    const float* __restrict__ xrow = X + (rin ? b0 + r : 0) * ld;
    const float* __restrict__ bias = trs + static_cast<int64_t>(D) * ld;
    const float4 zero4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    f64x4 acc[4];
    zero_acc64(acc);
    for (int k0 = 0; k0 < ld; k0 += 64) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int kq = k0 + 16 * g + 4 * q;
            const bool in = kq < ld;
            const float4 a = in && rin ? *reinterpret_cast<const float4*>(xrow + kq) : zero4;
            float4 w[4];
#pragma unroll
            for (int nb = 0; nb < 4; ++nb)
                w[nb] = in ? *reinterpret_cast<const float4*>(trs + static_cast<int64_t>(nb * 16 + r) * ld + kq) : zero4;
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) acc[nb] = mfma64(a.x, w[nb].x, acc[nb]);
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) acc[nb] = mfma64(a.y, w[nb].y, acc[nb]);
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) acc[nb] = mfma64(a.z, w[nb].z, acc[nb]);
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) acc[nb] = mfma64(a.w, w[nb].w, acc[nb]);
        }
    }
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        const int64_t bD = b0 + g + 4 * rr;
        if (bD >= n) continue;
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) Y[bD * D + nb * 16 + r] = static_cast<float>(acc[nb][rr] + static_cast<double>(bias[nb * 16 + r]));
    }
}

// out[b][f] (+)= sum_o Dm[b][o] W[o][f] for W [64][ld]: a wavefront owns 16 rows and 64 columns; with ld <= 64 the four
// wavefronts of a workgroup own four 16-row tiles, otherwise four 64-column blocks of one
__global__ __launch_bounds__(HW * 64) void mg_rows_w_kernel(const float* __restrict__ Dm, int n, int ld, const float* __restrict__ W,
                                                            float* __restrict__ out, int accumulate) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
    const bool narrow = ld <= 64;              // every wavefront its own 16-row tile; otherwise its own 64 columns of one tile
    const int64_t b0 = narrow ? (static_cast<int64_t>(blockIdx.x) * HW + wv) * 16 : static_cast<int64_t>(blockIdx.x) * 16;
    const int f0 = narrow ? 0 : (blockIdx.y * HW + wv) * 64;
    if (f0 >= ld || b0 >= n) return;
    float a[16];
    load_row_a(a, Dm, b0 + r < n ? b0 + r : -1, g);
    f64x4 acc[4];
    zero_acc64(acc);
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
        const float* __restrict__ wrow = W + static_cast<int64_t>(16 * g + kk) * ld + f0 + r;
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) {
            const float b = f0 + nb * 16 + r < ld ? wrow[nb * 16] : 0.0f;
            acc[nb] = mfma64(a[kk], b, acc[nb]);
        }
    }
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        const int64_t row = b0 + g + 4 * rr;
        if (row >= n) continue;
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) {
            const int f = f0 + nb * 16 + r;
            if (f >= ld) continue;
            float* p = out + row * ld + f;
            *p = static_cast<float>(accumulate ? static_cast<double>(*p) + acc[nb][rr] : acc[nb][rr]);
        }
    }
}

// part[bx][o][f] = sum over the rows of row block bx of Dm[row][o] Y[row][f], in row order: a wavefront owns 16 columns f and
// walks the block's rows four per MFMA (A = Dm^T, B = Y^T).  The fp32 operands are summed on v_mfma_f64_16x16x4_f64
// (acc[mb][rr] = the element [16 mb + g + 4 rr][f0 + r]), as freedom.hip's weight gradient is and as the products above are.
__global__ __launch_bounds__(HW * 64) void mg_xty_kernel(const float* __restrict__ Dm, const float* __restrict__ Y, int64_t n, int ld,
                                                         int rows_per_block, float* __restrict__ part, int64_t stride) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
    const int f = blockIdx.y * 64 + wv * 16 + r;
    const bool fin = f < ld;
    const int64_t row0 = static_cast<int64_t>(blockIdx.x) * rows_per_block;
    const int64_t row1 = row0 + rows_per_block < n ? row0 + rows_per_block : n;
    f64x4 acc[4];
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) acc[mb] = f64x4{0.0, 0.0, 0.0, 0.0};
    for (int64_t k0 = row0; k0 < row1; k0 += 16) {
        double a[4][4], b[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t bk = k0 + 4 * j + g;
            const bool in = bk < row1;
            b[j] = in && fin ? static_cast<double>(Y[bk * ld + f]) : 0.0;
#pragma unroll
            for (int mb = 0; mb < 4; ++mb) a[j][mb] = in ? static_cast<double>(Dm[bk * D + mb * 16 + r]) : 0.0;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int mb = 0; mb < 4; ++mb) acc[mb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[j][mb], b[j], acc[mb], 0, 0, 0);
        }
    }
    if (!fin) return;
    float* __restrict__ dst = part + static_cast<int64_t>(blockIdx.x) * stride;
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) {
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) dst[static_cast<int64_t>(mb * 16 + g + 4 * rr) * ld + f] = static_cast<float>(acc[mb][rr]);
    }
}

// part[bx][offset + o] = the sum of Dm[row][o] over the rows of row block bx: four interleaved float64 sums per column in row
// order, added as ((s0 + s1) + s2) + s3 and rounded once
__global__ __launch_bounds__(256) void mg_colsum_kernel(const float* __restrict__ Dm, int64_t n, int rows_per_block, float* __restrict__ part,
                                                        int64_t stride, int64_t offset) {
    __shared__ double s[4][D];
    const int o = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int64_t row0 = static_cast<int64_t>(blockIdx.x) * rows_per_block;
    const int64_t row1 = row0 + rows_per_block < n ? row0 + rows_per_block : n;
    double t = 0.0;
    for (int64_t k = row0 + q; k < row1; k += 4) t += static_cast<double>(Dm[k * D + o]);
    s[q][o] = t;
    __syncthreads();
    if (q == 0) part[static_cast<int64_t>(blockIdx.x) * stride + offset + o] = static_cast<float>(((s[0][o] + s[1][o]) + s[2][o]) + s[3][o]);
}

// out[e] = the row blocks' partial sums part[w][e] in block order, e < len
__global__ __launch_bounds__(256) void mg_reduce_kernel(const float* __restrict__ part, int n_wg, int64_t stride, int64_t len,
                                                        float* __restrict__ out) {
    const int64_t e = blockIdx.x * static_cast<int64_t>(256) + threadIdx.x;
    if (e >= len) return;
    float t = 0.0f;
    for (int w = 0; w < n_wg; ++w) t += part[static_cast<int64_t>(w) * stride + e];
    out[e] = t;
}

// ------------------------------------------------------------------------------------------------
// the purifier
// ------------------------------------------------------------------------------------------------
// g = sigmoid(F Wg^T + bg) (zero beyond dim), X = E * g: the gate in LDS, a wavefront per 16-row tile
__global__ __launch_bounds__(HW * 64) void mg_purify_kernel(const float* __restrict__ F, const float* __restrict__ E, const float* __restrict__ gate,
                                                            int n, int dim, float* __restrict__ G, float* __restrict__ X) {
    __shared__ __attribute__((aligned(16))) float sW[D * LD];
    load_tile<LD, HW>(sW, gate, 0, D);
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
    const int64_t b0 = static_cast<int64_t>(blockIdx.x) * TB + wv * 16;
    if (b0 >= n) return;
    float a[16];
    load_row_a(a, F, b0 + r < n ? b0 + r : -1, g);
    f64x4 acc[4];
    zero_acc64(acc);
    tile_product64<LD, 16>(acc, a, sW, r, g);
    const float* __restrict__ bias = gate + D * D;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        const int64_t row = b0 + g + 4 * rr;
        if (row >= n) continue;
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) {
            const int col = nb * 16 + r;
            const float gv = col < dim ? sigmoid(static_cast<float>(acc[nb][rr] + static_cast<double>(bias[col]))) : 0.0f;
            G[row * D + col] = gv;
            X[row * D + col] = E[row * D + col] * gv;
        }
    }
}

// dE += dX g;  dz = dX E g (1 - g)
__global__ __launch_bounds__(256) void mg_purify_bwd_kernel(const float* __restrict__ dX, const float* __restrict__ E, const float* __restrict__ G,
                                                            int64_t len, float* __restrict__ dE, float* __restrict__ dz) {
    const int64_t e = blockIdx.x * static_cast<int64_t>(256) + threadIdx.x;
    if (e >= len) return;
    const float dx = dX[e], gv = G[e], ev = E[e];
    dE[e] = dE[e] + dx * gv;
    dz[e] = (dx * ev) * (gv * (1.0f - gv));
}

// ------------------------------------------------------------------------------------------------
// the fuser
// ------------------------------------------------------------------------------------------------
struct FuseParams {
    const float* M;                // [N][64]
    const float* Zv;
    const float* Zt;
    const float* query;            // Wc [64][64] | bc [64] | q [64]
    const float* pref_v;           // W [64][64] | b [64]
    const float* pref_t;
    const int32_t* rows;           // [n] node ids, -1: no row; NULL: row b is node b
    int n, dim;
    float* out;                    // [n][64] or NULL
    float* side;                   // [n][64] or NULL
    float* zg;                     // [3][n][64] the gathered zv, zt, m, or NULL (with h, p, w)
    float* h;                      // [2][n][64] tanh(Wc z_m + bc)
    float* p;                      // [2][n][64] the preference gates
    float* w;                      // [n][2] the softmax weights, or NULL
};

__global__ __launch_bounds__(HW * 64) void mg_fuse_kernel(FuseParams p) {
    __shared__ __attribute__((aligned(16))) float sW[3][D * LD];
    load_tile<LD, HW>(sW[0], p.query, 0, D);
    load_tile<LD, HW>(sW[1], p.pref_v, 0, D);
    load_tile<LD, HW>(sW[2], p.pref_t, 0, D);
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
    const int64_t b0 = static_cast<int64_t>(blockIdx.x) * TB + wv * 16;
    const int64_t n = p.n;
    if (b0 >= n) return;
    const int64_t node = b0 + r < n ? (p.rows ? static_cast<int64_t>(p.rows[b0 + r]) : b0 + r) : -1;
    float a[16];
    f32x4 accv[4], acct[4], accp[4], accq[4];
    zero_acc(accv); zero_acc(acct); zero_acc(accp); zero_acc(accq);
    load_row_a(a, p.Zv, node, g);
    tile_product<LD, 16>(accv, a, sW[0], r, g);
    load_row_a(a, p.Zt, node, g);
    tile_product<LD, 16>(acct, a, sW[0], r, g);
    load_row_a(a, p.M, node, g);
    tile_product<LD, 16>(accp, a, sW[1], r, g);
    tile_product<LD, 16>(accq, a, sW[2], r, g);
    const float* __restrict__ bc = p.query + D * D;
    const float* __restrict__ q = p.query + D * D + D;
    const float* __restrict__ bv = p.pref_v + D * D;
    const float* __restrict__ bt = p.pref_t + D * D;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        const int64_t row = b0 + 4 * g + rr;
        const int64_t nd = __shfl(static_cast<int>(node), 4 * g + rr, 64);
        float hv[4], ht[4], av = 0.0f, at = 0.0f;
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) {
            const int col = nb * 16 + r;
            hv[nb] = tanhf(accv[nb][rr] + bc[col]);
            ht[nb] = tanhf(acct[nb][rr] + bc[col]);
            av += q[col] * hv[nb];
            at += q[col] * ht[nb];
        }
        av = sum16(av);
        at = sum16(at);
        const float mx = fmaxf(av, at), ev = expf(av - mx), et = expf(at - mx);
        const float wgv = ev / (ev + et), wgt = et / (ev + et);
        if (row >= n) continue;
        const bool ok = nd >= 0;
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) {
            const int col = nb * 16 + r;
            const float zv = ok ? p.Zv[nd * D + col] : 0.0f, zt = ok ? p.Zt[nd * D + col] : 0.0f, m = ok ? p.M[nd * D + col] : 0.0f;
            const float c = wgv * zv + wgt * zt;
            const float sv = zv - c, st = zt - c;
            const float pv = ok && col < p.dim ? sigmoid(accp[nb][rr] + bv[col]) : 0.0f;
            const float pt = ok && col < p.dim ? sigmoid(accq[nb][rr] + bt[col]) : 0.0f;
            const float side = ((pv * sv + pt * st) + c) / 3.0f;
            const int64_t e = row * D + col;
            if (p.out) p.out[e] = m + side;
            if (p.side) p.side[e] = side;
            if (p.zg) {
                p.zg[e] = zv;
                p.zg[n * D + e] = zt;
                p.zg[2 * n * D + e] = m;
                p.h[e] = ok ? hv[nb] : 0.0f;
                p.h[n * D + e] = ok ? ht[nb] : 0.0f;
                p.p[e] = pv;
                p.p[n * D + e] = pt;
            }
        }
        if (p.w && r == 0) {
            p.w[row * 2] = ok ? wgv : 0.0f;
            p.w[row * 2 + 1] = ok ? wgt : 0.0f;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// the batch: slots [0, n16) the users, [n16, 2 n16) pos, [2 n16, 3 n16) neg; n16 = n rounded up to 16
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mg_prep_kernel(const int32_t* __restrict__ users, const int32_t* __restrict__ pos,
                                                      const int32_t* __restrict__ neg, int n, int n16, int U, int I, int32_t* __restrict__ rows) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= 3 * n16) return;
    const int list = s / n16, b = s - list * n16;
    int node = -1;
    if (b < n) {
        const int u = users[b], i = pos[b], j = neg[b];
        if (u >= 0 && u < U && i >= 0 && i < I && j >= 0 && j < I) node = list == 0 ? u : U + (list == 1 ? i : j);
    }
    rows[s] = node;
}

// a wavefront per batch row: x = <o_u, o_i - o_j>, the gradient of -logsigmoid(x) / n + reg (|o_u|^2 + |o_i|^2 + |o_j|^2) / (2 n)
// with respect to the three out rows; part[bx] = (sum of -logsigmoid, sum of squares)
__global__ __launch_bounds__(HW * 64) void mg_bpr_kernel(const float* __restrict__ out, const int32_t* __restrict__ rows, int n, int n16,
                                                         float inv_n, float reg, float* __restrict__ dout, float* __restrict__ part) {
    __shared__ float s[HW][2];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int b = blockIdx.x * HW + wv;
    float lg = 0.0f, sq = 0.0f;
    if (b < n16) {
        const bool ok = b < n && rows[b] >= 0;
        const int64_t eu = static_cast<int64_t>(b) * D + lane, ei = eu + static_cast<int64_t>(n16) * D, ej = ei + static_cast<int64_t>(n16) * D;
        float gu = 0.0f, gi = 0.0f, gj = 0.0f;
        if (ok) {
            const float ou = out[eu], oi = out[ei], oj = out[ej];
            const float diff = oi - oj;
            const float x = wave_sum(ou * diff);
            const float c = -sigmoid_neg(x) * inv_n, rg = reg * inv_n;
            lg = -log_sigmoid(x);
            sq = wave_sum((ou * ou + oi * oi) + oj * oj);
            gu = c * diff + rg * ou;
            gi = c * ou + rg * oi;
            gj = rg * oj - c * ou;
        }
        dout[eu] = gu;
        dout[ei] = gi;
        dout[ej] = gj;
    }
    if (lane == 0) { s[wv][0] = lg; s[wv][1] = sq; }
    __syncthreads();
    if (threadIdx.x < 2) {
        const int k = threadIdx.x;
        part[static_cast<int64_t>(blockIdx.x) * 2 + k] = ((s[0][k] + s[1][k]) + s[2][k]) + s[3][k];
    }
}

// The InfoNCE terms: t = 0 over pos (a = side, b = M at the slots n16 + b), t = 1 over the users (slots b).
// ah = a / max(|a|, eps), bh likewise, diag = <ah, bh>; zero rows where the batch row is no row
__global__ __launch_bounds__(HW * 64) void mg_nce_norm_kernel(const float* __restrict__ side, const float* __restrict__ mg,
                                                              const int32_t* __restrict__ rows, int n, int n16, float* __restrict__ AH,
                                                              float* __restrict__ BH, float* __restrict__ NA, float* __restrict__ NB,
                                                              float* __restrict__ DG) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int b = blockIdx.x * HW + wv, t = blockIdx.y;
    if (b >= n16) return;
    const bool ok = b < n && rows[b] >= 0;
    const int64_t slot = t == 0 ? n16 + b : b;
    const float a = ok ? side[slot * D + lane] : 0.0f, bb = ok ? mg[slot * D + lane] : 0.0f;
    const double da = a, db = bb;
    const float na = fmaxf(static_cast<float>(sqrt(wave_sum(da * da))), NORM_EPS), nb = fmaxf(static_cast<float>(sqrt(wave_sum(db * db))), NORM_EPS);
    const float ah = a / na, bh = bb / nb;
    const int64_t o = static_cast<int64_t>(t) * n16 + b;
    AH[o * D + lane] = ah;
    BH[o * D + lane] = bh;
    const float dg = static_cast<float>(wave_sum(static_cast<double>(ah) * static_cast<double>(bh)));
    if (lane == 0) { NA[o] = na; NB[o] = nb; DG[o] = dg; }
}

// lse[r] = log sum_k exp(<ah_r, bh_k> / tau) over the batch's rows k, as an online log-sum-exp: a lane keeps a running maximum
// and a sum scaled by it over its columns (tile after tile, in column order), the 16 lanes of a row are joined at the end by a
// fixed tree.  With one column the result is the logit itself, bit for bit, so that P = exp(l - lse) = 1 and InfoNCE's gradient
// is an exact zero, as it is in exact arithmetic.  A wavefront owns 16 rows and walks the columns 64 at a time.
__global__ __launch_bounds__(HW * 64) void mg_nce_lse_kernel(const float* __restrict__ AH, const float* __restrict__ BH,
                                                             const int32_t* __restrict__ rows, int n, int n16, float* __restrict__ LSE) {
    __shared__ __attribute__((aligned(16))) float sY[D * LD];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
    const int t = blockIdx.y;
    const int q0 = blockIdx.x * TB + wv * 16;
    const float* __restrict__ A = AH + static_cast<int64_t>(t) * n16 * D;
    const float* __restrict__ B = BH + static_cast<int64_t>(t) * n16 * D;
    float a[16];
    load_a(a, A, q0, n16, r, g);
    float mx[4], s[4];
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) { mx[rr] = -INFINITY; s[rr] = 0.0f; }
    for (int c0 = 0; c0 < n; c0 += 64) {
        __syncthreads();
        load_tile<LD, HW>(sY, B, c0, n16);
        __syncthreads();
        f64x4 acc[4];
        logits_tile64<LD>(acc, a, sY, r, g);
        bool okc[4];
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) {
            const int col = c0 + nb * 16 + r;
            okc[nb] = col < n && rows[col] >= 0;
        }
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            float tm = mx[rr];
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) tm = okc[nb] ? fmaxf(tm, static_cast<float>(acc[nb][rr] * 5.0)) : tm;
            if (tm == -INFINITY) continue;
            float ts = s[rr] * expf(mx[rr] - tm);
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) ts += okc[nb] ? expf(static_cast<float>(acc[nb][rr] * 5.0) - tm) : 0.0f;
            mx[rr] = tm;
            s[rr] = ts;
        }
    }
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        const float top = max16(mx[rr]);
        const float tot = sum16(top == -INFINITY ? 0.0f : s[rr] * expf(mx[rr] - top));
        const int row = q0 + g + 4 * rr;
        if (r == 0 && row < n16) LSE[static_cast<int64_t>(t) * n16 + row] = tot > 0.0f ? top + logf(tot) : 0.0f;
    }
}

// z = 0: d side[r] from sum_k P_rk bh_k - bh_r; z = 1: d M[k] from sum_r P_rk ah_r - ah_k, P_rk = exp(<ah_r, bh_k> / tau -
// lse_r); then the backward of the normalisation.  The owner's 16 x 64 weights go through LDS to become the A operand of the
// second product, whose B operand is the same LDS tile read by columns.
__global__ __launch_bounds__(HW * 64) void mg_nce_grad_kernel(const float* __restrict__ AH, const float* __restrict__ BH, const float* __restrict__ NA,
                                                              const float* __restrict__ NB, const float* __restrict__ LSE,
                                                              const int32_t* __restrict__ rows, int n, int n16, float coef,
                                                              float* __restrict__ dside, float* __restrict__ dm) {
    __shared__ __attribute__((aligned(16))) float sY[D * LD];
    __shared__ __attribute__((aligned(16))) float sP[HW][16 * LD];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
    const int t = blockIdx.y, z = blockIdx.z;
    const int q0 = blockIdx.x * TB + wv * 16;
    const int64_t to = static_cast<int64_t>(t) * n16;
    const float* __restrict__ X = (z == 0 ? AH : BH) + to * D;
    const float* __restrict__ Y = (z == 0 ? BH : AH) + to * D;
    const float* __restrict__ lse = LSE + to;
    float a[16];
    load_a(a, X, q0, n16, r, g);
    bool ok_o[4];
    float lse_o[4];
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        const int row = q0 + g + 4 * rr;
        ok_o[rr] = row < n && rows[row] >= 0;
        lse_o[rr] = ok_o[rr] ? lse[row] : 0.0f;
    }
    f64x4 acc2[4];
    zero_acc64(acc2);
    for (int c0 = 0; c0 < n; c0 += 64) {
        __syncthreads();
        load_tile<LD, HW>(sY, Y, c0, n16);
        __syncthreads();
        f64x4 acc[4];
        logits_tile64<LD>(acc, a, sY, r, g);
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) {
            const int col = c0 + nb * 16 + r;
            const bool okc = col < n && rows[col] >= 0;
            const float lse_c = okc ? lse[col] : 0.0f;
#pragma unroll
            for (int rr = 0; rr < 4; ++rr)
                sP[wv][(g + 4 * rr) * LD + nb * 16 + r] =
                    okc && ok_o[rr] ? expf(static_cast<float>(acc[nb][rr] * 5.0) - (z == 0 ? lse_o[rr] : lse_c)) : 0.0f;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) {
            const float pa = sP[wv][r * LD + 4 * kk + g];
#pragma unroll
            for (int nb = 0; nb < 4; ++nb)
                acc2[nb] = mfma64(pa, sY[(4 * kk + g) * LD + nb * 16 + r], acc2[nb]);
        }
    }
    float* __restrict__ dst = z == 0 ? dside : dm;
    const float* __restrict__ norm = (z == 0 ? NA : NB) + to;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        const int row = q0 + g + 4 * rr;
        const bool in = row < n16;
        float xh[4];
        double dh[4], dot = 0.0;
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) {
            const int col = nb * 16 + r;
            xh[nb] = in ? X[static_cast<int64_t>(row) * D + col] : 0.0f;
            const float yh = in ? Y[static_cast<int64_t>(row) * D + col] : 0.0f;
            dh[nb] = ok_o[rr] ? (acc2[nb][rr] - static_cast<double>(yh)) * static_cast<double>(coef) : 0.0;
            dot += static_cast<double>(xh[nb]) * dh[nb];
        }
        dot = sum16d(dot);
        if (!in) continue;
        const float inv = ok_o[rr] ? 1.0f / norm[row] : 0.0f;
        const int64_t slot = t == 0 ? n16 + row : row;
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) dst[slot * D + nb * 16 + r] = static_cast<float>((dh[nb] - static_cast<double>(xh[nb]) * dot) * static_cast<double>(inv));
    }
}

// loss[0] = BPR, loss[1] = the regulariser, loss[2] = cl_loss * (InfoNCE over pos + InfoNCE over the users), loss[3] = total
__global__ __launch_bounds__(64) void mg_loss_kernel(const float* __restrict__ part, int n_wg, const float* __restrict__ LSE,
                                                     const float* __restrict__ DG, const int32_t* __restrict__ rows, int n, int n16, float reg,
                                                     float cl, float* __restrict__ loss) {
    const int lane = threadIdx.x;
    float lg = 0.0f, sq = 0.0f, nce = 0.0f;
    for (int w = lane; w < n_wg; w += 64) { lg += part[2 * w]; sq += part[2 * w + 1]; }
    for (int t = 0; t < 2; ++t) {
        for (int b = lane; b < n; b += 64) {
            if (rows[b] >= 0) nce += LSE[t * n16 + b] - INV_TAU * DG[t * n16 + b];
        }
    }
    lg = wave_sum(lg); sq = wave_sum(sq); nce = wave_sum(nce);
    if (lane != 0) return;
    const float fn = static_cast<float>(n);
    const float l0 = lg / fn, l1 = reg * sq / (2.0f * fn), l2 = cl * (nce / fn);
    loss[0] = l0; loss[1] = l1; loss[2] = l2; loss[3] = (l0 + l1) + l2;
}

// the row-local backward of the fuser, a wavefront per slot (lane = column): everything but the four products with Wc, W_ip
// and W_tp, whose left operands it leaves in dpre / dpp
struct FuseBwdParams {
    const int32_t* rows;           // [3 n16]
    int n16;
    const float* dout;             // [3 n16][64]
    const float* dsx;              // [2 n16][64] InfoNCE's gradient with respect to side (users, pos)
    const float* dmx;              // [2 n16][64] ... with respect to M
    const float* zg;               // [3][3 n16][64]
    const float* h;                // [2][3 n16][64]
    const float* p;                // [2][3 n16][64]
    const float* w;                // [3 n16][2]
    const float* q;                // [64]
    float* dz;                     // [2][3 n16][64]
    float* dm;                     // [3 n16][64]
    float* dpre;                   // [2][3 n16][64]
    float* dpp;                    // [2][3 n16][64]
    float* dq;                     // [3 n16][64]
};

__global__ __launch_bounds__(HW * 64) void mg_fuse_bwd_kernel(FuseBwdParams p) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t S = 3 * static_cast<int64_t>(p.n16);
    const int64_t slot = static_cast<int64_t>(blockIdx.x) * HW + wv;
    if (slot >= S) return;
    const int64_t e = slot * D + lane;
    const bool ok = p.rows[slot] >= 0, extra = slot < 2 * static_cast<int64_t>(p.n16);
    float dzv = 0.0f, dzt = 0.0f, dm = 0.0f, dprev = 0.0f, dpret = 0.0f, dppv = 0.0f, dppt = 0.0f, dq = 0.0f;
    if (ok) {
        const float dout = p.dout[e];
        const float ds = (dout + (extra ? p.dsx[e] : 0.0f)) / 3.0f;
        dm = dout + (extra ? p.dmx[e] : 0.0f);
        const float zv = p.zg[e], zt = p.zg[S * D + e];
        const float hv = p.h[e], ht = p.h[S * D + e], pv = p.p[e], pt = p.p[S * D + e];
        const float wgv = p.w[slot * 2], wgt = p.w[slot * 2 + 1];
        const float c = wgv * zv + wgt * zt;
        const float sv = zv - c, st = zt - c;
        const float d_pv = ds * sv, d_pt = ds * st, d_sv = ds * pv, d_st = ds * pt;
        const float d_c = (ds - d_sv) - d_st;
        dzv = d_sv + wgv * d_c;
        dzt = d_st + wgt * d_c;
        const float dwv = wave_sum(d_c * zv), dwt = wave_sum(d_c * zt);
        const float dav = (wgv * wgt) * (dwv - dwt);
        const float qv = p.q[lane];
        dq = dav * hv - dav * ht;
        dprev = (dav * qv) * (1.0f - hv * hv);
        dpret = -(dav * qv) * (1.0f - ht * ht);
        dppv = d_pv * (pv * (1.0f - pv));
        dppt = d_pt * (pt * (1.0f - pt));
    }
    p.dz[e] = dzv;
    p.dz[S * D + e] = dzt;
    p.dm[e] = dm;
    p.dpre[e] = dprev;
    p.dpre[S * D + e] = dpret;
    p.dpp[e] = dppv;
    p.dpp[S * D + e] = dppt;
    p.dq[e] = dq;
}

// G_k[id] = the sum of the slot rows of S_k whose list entry is id, in rank order, by the wavefront of the id's first rank: one
// writer per distinct id (the three tables are cleared first)
struct SegParams {
    float* G[3];                   // dM, dZv, dZt: [N][64]
    const float* S[3];             // [3 n16][64]
};
__global__ __launch_bounds__(HW * 64) void mg_seg_add_kernel(SegParams p, const int32_t* __restrict__ users, const int32_t* __restrict__ pos,
                                                             const int32_t* __restrict__ neg, const int32_t* __restrict__ order_u,
                                                             const int32_t* __restrict__ order_i, int n, int n16, int U, int I, int blocks_u) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const bool user = static_cast<int>(blockIdx.x) < blocks_u;
    const int rk = (user ? blockIdx.x : blockIdx.x - blocks_u) * HW + wv;
    const int len = user ? n : 2 * n;
    if (rk >= len) return;
    const int32_t* order = user ? order_u : order_i;
    const auto id_at = [&](int o) { return user ? users[o] : item_at(pos, neg, n, o); };
    const int id = id_at(order[rk]);
    if (id < 0 || id >= (user ? U : I)) return;
    if (rk > 0 && id_at(order[rk - 1]) == id) return;
    float acc[3] = {0.0f, 0.0f, 0.0f};
    for (int k = rk; k < len; ++k) {
        const int o = order[k];
        if (id_at(o) != id) break;
        const int64_t slot = user ? o : (o < n ? n16 + o : 2 * static_cast<int64_t>(n16) + (o - n));
#pragma unroll
        for (int t = 0; t < 3; ++t) acc[t] += p.S[t][slot * D + lane];
    }
    const int64_t row = static_cast<int64_t>(user ? 0 : U) + id;
#pragma unroll
    for (int t = 0; t < 3; ++t) p.G[t][row * D + lane] = acc[t];
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
inline int rows_per_block(int64_t n) {
    int64_t r = (n + XTY_BLOCKS - 1) / XTY_BLOCKS;
    r = (r + 15) / 16 * 16;
    return static_cast<int>(std::max<int64_t>(XTY_ROWS, r));
}
inline int xty_blocks(int64_t n) { return static_cast<int>((n + rows_per_block(n) - 1) / rows_per_block(n)); }
// floats of the partial sums of one X^T Y reduction over n rows with ld columns
inline int64_t xty_floats(int64_t n, int ld) { return static_cast<int64_t>(xty_blocks(n)) * (static_cast<int64_t>(D) * ld + D); }

// out [64][ld] | [64] = Dm^T Y | the column sums of Dm, over n rows; Y == NULL: the column sums alone, out [64]
int launch_xty(const float* Dm, const float* Y, int64_t n, int ld, float* part, float* out, hipStream_t st) {
    const int rpb = rows_per_block(n), nb = xty_blocks(n);
    const int64_t stride = Y ? static_cast<int64_t>(D) * ld + D : D, off = Y ? static_cast<int64_t>(D) * ld : 0;
    if (Y) hipLaunchKernelGGL(mg_xty_kernel, dim3(nb, (ld + 63) / 64), dim3(HW * 64), 0, st, Dm, Y, n, ld, rpb, part, stride);
    hipLaunchKernelGGL(mg_colsum_kernel, dim3(nb), dim3(256), 0, st, Dm, n, rpb, part, stride, off);
    hipLaunchKernelGGL(mg_reduce_kernel, dim3(static_cast<unsigned>((stride + 255) / 256)), dim3(256), 0, st, part, nb, stride, stride, out);
    SKR_LAUNCH_CHECK();
    return SKR_OK;
}

int launch_rows_w(const float* Dm, int64_t n, int ld, const float* W, float* out, int accumulate, hipStream_t st) {
    const dim3 grid = ld <= 64 ? dim3(static_cast<unsigned>((n + 16 * HW - 1) / (16 * HW)), 1)
                               : dim3(static_cast<unsigned>((n + 15) / 16), (ld + 64 * HW - 1) / (64 * HW));
    hipLaunchKernelGGL(mg_rows_w_kernel, grid, dim3(HW * 64), 0, st, Dm,
                       static_cast<int>(n), ld, W, out, accumulate);
    SKR_LAUNCH_CHECK();
    return SKR_OK;
}

inline unsigned tile_blocks(int64_t n) { return static_cast<unsigned>((n + TB - 1) / TB); }

int check_feature(const char* who, int F, int ld) {
    SKR_REQUIRE(F >= 1 && F <= MAXF, "%s: 1 <= feat_dim <= %d (got %d)", who, MAXF, F);
    SKR_REQUIRE(ld >= F && ld % 4 == 0 && ld <= MAXF, "%s: feat_ld = %d must be a multiple of 4, >= feat_dim = %d and <= %d", who, ld, F, MAXF);
    return SKR_OK;
}

// the projection backward: dtrs = dF^T X | column sums of dF, dX = dF W
int project_bwd(const float* dF, const float* X, int n, int ld, const float* trs, float* dtrs, float* dX, float* part, hipStream_t st) {
    int rc = launch_xty(dF, X, n, ld, part, dtrs, st);
    if (rc != SKR_OK) return rc;
    return launch_rows_w(dF, n, ld, trs, dX, 0, st);
}

// the purifier backward: dE += dX g, dz (scratch [n][64]), dF = dz Wg, dgate = dz^T F | column sums of dz
int purify_bwd(const float* dX, const float* E, const float* G, const float* F, const float* gate, int n, float* dE, float* dF, float* dgate,
               float* dz, float* part, hipStream_t st) {
    const int64_t len = static_cast<int64_t>(n) * D;
    hipLaunchKernelGGL(mg_purify_bwd_kernel, dim3(static_cast<unsigned>((len + 255) / 256)), dim3(256), 0, st, dX, E, G, len, dE, dz);
    SKR_LAUNCH_CHECK();
    int rc = launch_rows_w(dz, n, D, gate, dF, 0, st);
    if (rc != SKR_OK) return rc;
    return launch_xty(dz, F, n, D, part, dgate, st);
}

struct StepLayout {            // float offsets into the step's workspace
    int64_t rows, out, side, zg, h, p, w, dout, dsx, dmx, ah, bh, na, nb, dg, lse, bpart, dz, dm, dpre, dpp, dq, ordu, ordi, dF, dzI, part, total;
};

inline int bpr_workgroups(int n16) { return n16 / HW; }

inline StepLayout step_layout(int n, int n_items, int ld_max) {
    StepLayout L;
    const int64_t n16 = (static_cast<int64_t>(n) + 15) / 16 * 16, S = 3 * n16, I = n_items;
    int64_t o = 0;
    L.rows = o; o += S;
    L.out = o; o += S * D;
    L.side = o; o += S * D;
    L.zg = o; o += 3 * S * D;
    L.h = o; o += 2 * S * D;
    L.p = o; o += 2 * S * D;
    L.w = o; o += 2 * S;
    L.dout = o; o += S * D;
    L.dsx = o; o += 2 * n16 * D;
    L.dmx = o; o += 2 * n16 * D;
    L.ah = o; o += 2 * n16 * D;
    L.bh = o; o += 2 * n16 * D;
    L.na = o; o += 2 * n16;
    L.nb = o; o += 2 * n16;
    L.dg = o; o += 2 * n16;
    L.lse = o; o += 2 * n16;
    L.bpart = o; o += round4(2 * static_cast<int64_t>(bpr_workgroups(static_cast<int>(n16))));
    L.dz = o; o += 2 * S * D;
    L.dm = o; o += S * D;
    L.dpre = o; o += 2 * S * D;
    L.dpp = o; o += 2 * S * D;
    L.dq = o; o += S * D;
    L.ordu = o; o += n16;
    L.ordi = o; o += 2 * n16;
    L.dF = o; o += I * D;
    L.dzI = o; o += I * D;
    L.part = o; o += std::max(xty_floats(I, std::max(ld_max, D)), xty_floats(2 * S, D));    // the widest of the reductions' partials
    L.total = o;
    return L;
}

int run_step(const skr_mgcn_step_args* a, void* stream, float* h_ms) {
    SKR_REQUIRE(a, "skr_mgcn_step: NULL argument");
    const int U = a->n_users, I = a->n_items, n = a->n, Lu = a->n_ui_layers, Ln = a->n_layers;
    SKR_REQUIRE(a->params && a->users && a->pos && a->neg && a->M && a->grad && a->loss && a->work && a->query && a->query_grad,
                "skr_mgcn_step: NULL argument");
    SKR_REQUIRE(U > 0 && I > 0 && n >= 0 && n <= MAXB, "skr_mgcn_step: n_users = %d, n_items = %d, n = %d (at most %d rows)", U, I, n, MAXB);
    SKR_REQUIRE(a->dim >= 1 && a->dim <= D, "skr_mgcn_step: 1 <= dim <= 64 (got %d); rows are 64 floats, zero-padded", a->dim);
    SKR_REQUIRE(Lu >= 0 && Lu <= MAXL && Ln >= 0 && Ln <= MAXL, "skr_mgcn_step: 0 <= n_ui_layers, n_layers <= %d (got %d, %d)", MAXL, Lu, Ln);
    SKR_REQUIRE(a->plan_a && a->plan_at, "skr_mgcn_step: both plans of the user-item graph are needed (R enters the item-item view)");
    SKR_REQUIRE(a->ping[0] && a->ping[1], "skr_mgcn_step: both ping tables are needed");
    SKR_REQUIRE(a->reg >= 0.0f && a->cl_loss >= 0.0f, "skr_mgcn_step: reg = %g, cl_loss = %g (>= 0)", a->reg, a->cl_loss);
    uintptr_t align = reinterpret_cast<uintptr_t>(a->params) | reinterpret_cast<uintptr_t>(a->grad) | reinterpret_cast<uintptr_t>(a->work) |
                      reinterpret_cast<uintptr_t>(a->M) | reinterpret_cast<uintptr_t>(a->ping[0]) | reinterpret_cast<uintptr_t>(a->ping[1]) |
                      reinterpret_cast<uintptr_t>(a->query) | reinterpret_cast<uintptr_t>(a->query_grad);
    int ld_max = 0;
    for (int m = 0; m < 2; ++m) {
        const int rc = check_feature("skr_mgcn_step", a->feat_dim[m], a->feat_ld[m]);
        if (rc != SKR_OK) return rc;
        ld_max = std::max(ld_max, a->feat_ld[m]);
        SKR_REQUIRE(Ln == 0 || (a->plan_s[m] && a->plan_st[m]), "skr_mgcn_step: n_layers > 0 needs both plans of both item graphs");
        SKR_REQUIRE(a->trs[m] && a->feat[m] && a->gate[m] && a->prefer[m] && a->F[m] && a->gate_out[m] && a->Z[m] && a->trs_grad[m] &&
                        a->feat_grad[m] && a->gate_grad[m] && a->prefer_grad[m],
                    "skr_mgcn_step: both modalities need their tables");
        align |= reinterpret_cast<uintptr_t>(a->trs[m]) | reinterpret_cast<uintptr_t>(a->feat[m]) | reinterpret_cast<uintptr_t>(a->gate[m]) |
                 reinterpret_cast<uintptr_t>(a->prefer[m]) | reinterpret_cast<uintptr_t>(a->F[m]) | reinterpret_cast<uintptr_t>(a->gate_out[m]) |
                 reinterpret_cast<uintptr_t>(a->Z[m]) | reinterpret_cast<uintptr_t>(a->trs_grad[m]) | reinterpret_cast<uintptr_t>(a->feat_grad[m]) |
                 reinterpret_cast<uintptr_t>(a->gate_grad[m]) | reinterpret_cast<uintptr_t>(a->prefer_grad[m]);
    }
    for (int t = 0; t < 3; ++t) {
        SKR_REQUIRE(a->G[t], "skr_mgcn_step: the three gradient tables G are needed");
        align |= reinterpret_cast<uintptr_t>(a->G[t]);
    }
    if (n == 0) return SKR_OK;
    const StepLayout W = step_layout(n, I, ld_max);
    SKR_REQUIRE(a->work_bytes >= static_cast<size_t>(W.total) * sizeof(float),
                "skr_mgcn_step: work holds %zu bytes, skr_mgcn_workspace(%d, %d, %d) asks for %zu", a->work_bytes, n, I, ld_max,
                static_cast<size_t>(W.total) * sizeof(float));
    SKR_REQUIRE((align & 15) == 0, "skr_mgcn_step: the tables and work must be 16-byte aligned");
    hipStream_t st = skr::as_stream(stream);
    float* w = static_cast<float*>(a->work);
    int32_t* rows = reinterpret_cast<int32_t*>(w + W.rows);
    int32_t* ordu = reinterpret_cast<int32_t*>(w + W.ordu);
    int32_t* ordi = reinterpret_cast<int32_t*>(w + W.ordi);
    const int n16 = (n + 15) / 16 * 16;
    const int64_t S = 3 * static_cast<int64_t>(n16);
    const int64_t UO = static_cast<int64_t>(U) * D, N = static_cast<int64_t>(U) + I;
    const float* Ei = a->params + UO;
    StepTimer<SKR_MGCN_GROUPS + 1> mk(h_ms, st);
    SKR_HIP(mk.mark());
    int rc;
    // ---- 0: F_m = T_m W_m^T + b_m over all items (MGCN.py:251-254)
    for (int m = 0; m < 2; ++m)
        hipLaunchKernelGGL(mg_project_kernel, dim3(tile_blocks(I)), dim3(HW * 64), 0, st, a->feat[m], I, a->feat_ld[m], a->trs[m], a->F[m]);
    SKR_LAUNCH_CHECK();
    SKR_HIP(mk.mark());
    // ---- 1: the user-item view (MGCN.py:260-271)
    const auto product = [&](const skr_spmm_plan* plan, const float* X, const skr_spmm_epilogue& ep, bool) {
        return skr_spmm_plan_run_ex(plan, X, D, &ep, nullptr, nullptr, stream);
    };
    rc = mean_forward(a->plan_a, a->plan_at, a->params, UO, N, Lu, a->ping, a->M, st, product);
    if (rc != SKR_OK) return rc;
    SKR_HIP(mk.mark());
    // ---- 2: the purifier (MGCN.py:257-258) and the item-item view (:273-289); the ping tables are free again: X_m lands
    // where the item-graph runs start
    for (int m = 0; m < 2; ++m) {
        hipLaunchKernelGGL(mg_purify_kernel, dim3(tile_blocks(I)), dim3(HW * 64), 0, st, a->F[m], Ei, a->gate[m], I, a->dim, a->gate_out[m],
                           Ln == 0 ? a->Z[m] + UO : a->ping[0]);
        SKR_LAUNCH_CHECK();
        for (int k = 1; k <= Ln; ++k) {
            float* dst = k == Ln ? a->Z[m] + UO : a->ping[k & 1];
            rc = plain_run(a->plan_s[m], a->ping[(k - 1) & 1], nullptr, dst, nullptr, nullptr, stream);
            if (rc != SKR_OK) return rc;
        }
        rc = plain_run(a->plan_a, a->Z[m] + UO, nullptr, a->Z[m], nullptr, nullptr, stream);
        if (rc != SKR_OK) return rc;
    }
    SKR_HIP(mk.mark());
    // ---- 3: the fuser at the batch's slots, the loss (MGCN.py:291-353)
    hipLaunchKernelGGL(mg_prep_kernel, dim3(static_cast<unsigned>((S + 255) / 256)), dim3(256), 0, st, a->users, a->pos, a->neg, n, n16, U, I, rows);
    FuseParams fp = {};
    fp.M = a->M; fp.Zv = a->Z[0]; fp.Zt = a->Z[1]; fp.query = a->query; fp.pref_v = a->prefer[0]; fp.pref_t = a->prefer[1];
    fp.rows = rows; fp.n = static_cast<int>(S); fp.dim = a->dim;
    fp.out = w + W.out; fp.side = w + W.side; fp.zg = w + W.zg; fp.h = w + W.h; fp.p = w + W.p; fp.w = w + W.w;
    hipLaunchKernelGGL(mg_fuse_kernel, dim3(tile_blocks(S)), dim3(HW * 64), 0, st, fp);
    const int n_wg = bpr_workgroups(n16);
    const float inv_n = 1.0f / static_cast<float>(n);
    hipLaunchKernelGGL(mg_bpr_kernel, dim3(n_wg), dim3(HW * 64), 0, st, w + W.out, rows, n, n16, inv_n, a->reg, w + W.dout, w + W.bpart);
    hipLaunchKernelGGL(mg_nce_norm_kernel, dim3(n16 / HW, 2), dim3(HW * 64), 0, st, w + W.side, w + W.zg + 2 * S * D, rows, n, n16, w + W.ah,
                       w + W.bh, w + W.na, w + W.nb, w + W.dg);
    const unsigned nce_blocks = (n16 + TB - 1) / TB;
    hipLaunchKernelGGL(mg_nce_lse_kernel, dim3(nce_blocks, 2), dim3(HW * 64), 0, st, w + W.ah, w + W.bh, rows, n, n16, w + W.lse);
    hipLaunchKernelGGL(mg_nce_grad_kernel, dim3(nce_blocks, 2, 2), dim3(HW * 64), 0, st, w + W.ah, w + W.bh, w + W.na, w + W.nb, w + W.lse, rows, n,
                       n16, a->cl_loss * INV_TAU * inv_n, w + W.dsx, w + W.dmx);
    hipLaunchKernelGGL(mg_loss_kernel, dim3(1), dim3(64), 0, st, w + W.bpart, n_wg, w + W.lse, w + W.dg, rows, n, n16, a->reg, a->cl_loss, a->loss);
    SKR_LAUNCH_CHECK();
    SKR_HIP(mk.mark());
    // ---- 4: the fuser's backward at the slots, its weight gradients, the three dense gradient tables
    FuseBwdParams bp = {};
    bp.rows = rows; bp.n16 = n16; bp.dout = w + W.dout; bp.dsx = w + W.dsx; bp.dmx = w + W.dmx; bp.zg = w + W.zg; bp.h = w + W.h; bp.p = w + W.p;
    bp.w = w + W.w; bp.q = a->query + GATE; bp.dz = w + W.dz; bp.dm = w + W.dm; bp.dpre = w + W.dpre; bp.dpp = w + W.dpp; bp.dq = w + W.dq;
    hipLaunchKernelGGL(mg_fuse_bwd_kernel, dim3(static_cast<unsigned>((S + HW - 1) / HW)), dim3(HW * 64), 0, st, bp);
    SKR_LAUNCH_CHECK();
    if ((rc = launch_rows_w(w + W.dpre, S, D, a->query, w + W.dz, 1, st)) != SKR_OK) return rc;
    if ((rc = launch_rows_w(w + W.dpre + S * D, S, D, a->query, w + W.dz + S * D, 1, st)) != SKR_OK) return rc;
    if ((rc = launch_rows_w(w + W.dpp, S, D, a->prefer[0], w + W.dm, 1, st)) != SKR_OK) return rc;
    if ((rc = launch_rows_w(w + W.dpp + S * D, S, D, a->prefer[1], w + W.dm, 1, st)) != SKR_OK) return rc;
    if ((rc = launch_xty(w + W.dpre, w + W.zg, 2 * S, D, w + W.part, a->query_grad, st)) != SKR_OK) return rc;      // Wc | bc over v then t
    if ((rc = launch_xty(w + W.dq, nullptr, S, D, w + W.part, a->query_grad + GATE, st)) != SKR_OK) return rc;      // q
    if ((rc = launch_xty(w + W.dpp, w + W.zg + 2 * S * D, S, D, w + W.part, a->prefer_grad[0], st)) != SKR_OK) return rc;
    if ((rc = launch_xty(w + W.dpp + S * D, w + W.zg + 2 * S * D, S, D, w + W.part, a->prefer_grad[1], st)) != SKR_OK) return rc;
    for (int t = 0; t < 3; ++t) SKR_HIP(hipMemsetAsync(a->G[t], 0, static_cast<size_t>(N) * D * sizeof(float), st));
    hipLaunchKernelGGL(rank_triples_kernel<256>, dim3((3 * n + 255) / 256), dim3(256), 0, st, a->users, a->pos, a->neg, n, ordu, ordi);
    const int blocks_u = (n + HW - 1) / HW, blocks_i = (2 * n + HW - 1) / HW;
    SegParams sp = {{a->G[0], a->G[1], a->G[2]}, {w + W.dm, w + W.dz, w + W.dz + S * D}};
    hipLaunchKernelGGL(mg_seg_add_kernel, dim3(blocks_u + blocks_i), dim3(HW * 64), 0, st, sp, a->users, a->pos, a->neg, ordu, ordi, n, n16, U, I,
                       blocks_u);
    SKR_LAUNCH_CHECK();
    SKR_HIP(mk.mark());
    // ---- 5: the mean's backward chain into the gradient's rows; per modality dX = R^T dZ_users + dZ_items, then S_m^T Ln times
    if (Lu == 0) SKR_HIP(hipMemcpyAsync(a->grad, a->G[0], static_cast<size_t>(N) * D * sizeof(float), hipMemcpyDeviceToDevice, st));
    rc = chain_backward(a->plan_a, a->plan_at, a->G[0], UO, Lu, a->ping, a->grad, product);
    if (rc != SKR_OK) return rc;
    SKR_HIP(mk.mark());
    // ---- 6, 7: per modality dX = R^T dZ_users + dZ_items, S_m^T Ln times, then the purifier's and the projection's backward
    for (int m = 0; m < 2; ++m) {
        float* cur = a->ping[0];
        rc = plain_run(a->plan_at, a->G[1 + m], a->G[1 + m] + UO, cur, nullptr, nullptr, stream);
        if (rc != SKR_OK) return rc;
        for (int k = 1; k <= Ln; ++k) {
            float* dst = a->ping[k & 1];
            rc = plain_run(a->plan_st[m], cur, nullptr, dst, nullptr, nullptr, stream);
            if (rc != SKR_OK) return rc;
            cur = dst;
        }
        rc = purify_bwd(cur, Ei, a->gate_out[m], a->F[m], a->gate[m], I, a->grad + UO, w + W.dF, a->gate_grad[m], w + W.dzI, w + W.part, st);
        if (rc != SKR_OK) return rc;
        rc = project_bwd(w + W.dF, a->feat[m], I, a->feat_ld[m], a->trs[m], a->trs_grad[m], a->feat_grad[m], w + W.part, st);
        if (rc != SKR_OK) return rc;
        SKR_HIP(mk.mark());
    }
    SKR_HIP(mk.finish());
    return SKR_OK;
}

}  // namespace

// dense_ops.h: the two dense products over rows, for the other models' steps (slmrec.hip)
namespace skr {
int64_t dense_xty_floats(int64_t n, int ld) { return xty_floats(n, ld); }
int dense_xty(const float* Dm, const float* Y, int64_t n, int ld, float* part, float* out, hipStream_t st) {
    return launch_xty(Dm, Y, n, ld, part, out, st);
}
int dense_rows_w(const float* Dm, int64_t n, int ld, const float* W, float* out, int accumulate, hipStream_t st) {
    return launch_rows_w(Dm, n, ld, W, out, accumulate, st);
}
}  // namespace skr

extern "C" {

int skr_mgcn_project(const float* d_X, int n_rows, int feat_dim, int feat_ld, const float* d_trs, float* d_Y, void* stream) {
    SKR_REQUIRE(d_X && d_trs && d_Y, "skr_mgcn_project: NULL argument");
    SKR_REQUIRE(n_rows > 0, "skr_mgcn_project: n_rows = %d", n_rows);
    const int rc = check_feature("skr_mgcn_project", feat_dim, feat_ld);
    if (rc != SKR_OK) return rc;
    SKR_REQUIRE(((reinterpret_cast<uintptr_t>(d_X) | reinterpret_cast<uintptr_t>(d_trs) | reinterpret_cast<uintptr_t>(d_Y)) & 15) == 0,
                "skr_mgcn_project: the tables must be 16-byte aligned");
    hipLaunchKernelGGL(mg_project_kernel, dim3(tile_blocks(n_rows)), dim3(HW * 64), 0, skr::as_stream(stream), d_X, n_rows, feat_ld, d_trs, d_Y);
    SKR_LAUNCH_CHECK();
    return SKR_OK;
}

int skr_mgcn_row_block(int n_rows) { return n_rows > 0 ? rows_per_block(n_rows) : 0; }

size_t skr_mgcn_project_bwd_workspace(int n_rows, int feat_ld) {
    if (n_rows <= 0 || feat_ld <= 0 || feat_ld > MAXF) return 0;
    return static_cast<size_t>(xty_floats(n_rows, feat_ld)) * sizeof(float);
}

int skr_mgcn_project_bwd(const float* d_dF, const float* d_X, int n_rows, int feat_dim, int feat_ld, const float* d_trs, float* d_dtrs, float* d_dX,
                         void* d_work, size_t work_bytes, void* stream) {
    SKR_REQUIRE(d_dF && d_X && d_trs && d_dtrs && d_dX && d_work, "skr_mgcn_project_bwd: NULL argument");
    SKR_REQUIRE(n_rows > 0, "skr_mgcn_project_bwd: n_rows = %d", n_rows);
    const int rc = check_feature("skr_mgcn_project_bwd", feat_dim, feat_ld);
    if (rc != SKR_OK) return rc;
    SKR_REQUIRE(work_bytes >= skr_mgcn_project_bwd_workspace(n_rows, feat_ld), "skr_mgcn_project_bwd: work holds %zu bytes, %zu are needed",
                work_bytes, skr_mgcn_project_bwd_workspace(n_rows, feat_ld));
    SKR_REQUIRE(((reinterpret_cast<uintptr_t>(d_dF) | reinterpret_cast<uintptr_t>(d_X) | reinterpret_cast<uintptr_t>(d_trs) |
                  reinterpret_cast<uintptr_t>(d_dtrs) | reinterpret_cast<uintptr_t>(d_dX) | reinterpret_cast<uintptr_t>(d_work)) & 15) == 0,
                "skr_mgcn_project_bwd: the tables and work must be 16-byte aligned");
    return project_bwd(d_dF, d_X, n_rows, feat_ld, d_trs, d_dtrs, d_dX, static_cast<float*>(d_work), skr::as_stream(stream));
}

// the weight part of skr_mgcn_project_bwd alone -- the same launches, without dX = dF W: for a model whose feature table is a
// constant (SLMRec)
int skr_slmrec_project_bwd_w(const float* d_dF, const float* d_X, int n_rows, int feat_dim, int feat_ld, float* d_dtrs, void* d_work,
                             size_t work_bytes, void* stream) {
    SKR_REQUIRE(d_dF && d_X && d_dtrs && d_work, "skr_slmrec_project_bwd_w: NULL argument");
    SKR_REQUIRE(n_rows > 0, "skr_slmrec_project_bwd_w: n_rows = %d", n_rows);
    const int rc = check_feature("skr_slmrec_project_bwd_w", feat_dim, feat_ld);
    if (rc != SKR_OK) return rc;
    SKR_REQUIRE(work_bytes >= skr_mgcn_project_bwd_workspace(n_rows, feat_ld), "skr_slmrec_project_bwd_w: work holds %zu bytes, %zu are needed",
                work_bytes, skr_mgcn_project_bwd_workspace(n_rows, feat_ld));
    SKR_REQUIRE(((reinterpret_cast<uintptr_t>(d_dF) | reinterpret_cast<uintptr_t>(d_X) | reinterpret_cast<uintptr_t>(d_dtrs) |
                  reinterpret_cast<uintptr_t>(d_work)) & 15) == 0,
                "skr_slmrec_project_bwd_w: the tables and work must be 16-byte aligned");
    return launch_xty(d_dF, d_X, n_rows, feat_ld, static_cast<float*>(d_work), d_dtrs, skr::as_stream(stream));
}

int skr_mgcn_purify(const float* d_F, const float* d_E, const float* d_gate, int n_rows, int dim, float* d_g, float* d_X, void* stream) {
    SKR_REQUIRE(d_F && d_E && d_gate && d_g && d_X, "skr_mgcn_purify: NULL argument");
    SKR_REQUIRE(n_rows > 0 && dim >= 1 && dim <= D, "skr_mgcn_purify: n_rows = %d, 1 <= dim <= 64 (got %d)", n_rows, dim);
    SKR_REQUIRE(((reinterpret_cast<uintptr_t>(d_F) | reinterpret_cast<uintptr_t>(d_E) | reinterpret_cast<uintptr_t>(d_gate) |
                  reinterpret_cast<uintptr_t>(d_g) | reinterpret_cast<uintptr_t>(d_X)) & 15) == 0,
                "skr_mgcn_purify: the tables must be 16-byte aligned");
    hipLaunchKernelGGL(mg_purify_kernel, dim3(tile_blocks(n_rows)), dim3(HW * 64), 0, skr::as_stream(stream), d_F, d_E, d_gate, n_rows, dim, d_g,
                       d_X);
    SKR_LAUNCH_CHECK();
    return SKR_OK;
}

size_t skr_mgcn_purify_bwd_workspace(int n_rows) {
    if (n_rows <= 0) return 0;
    return static_cast<size_t>(static_cast<int64_t>(n_rows) * D + xty_floats(n_rows, D)) * sizeof(float);
}

int skr_mgcn_purify_bwd(const float* d_dX, const float* d_E, const float* d_g, const float* d_F, const float* d_gate, int n_rows, float* d_dE,
                        float* d_dF, float* d_dgate, void* d_work, size_t work_bytes, void* stream) {
    SKR_REQUIRE(d_dX && d_E && d_g && d_F && d_gate && d_dE && d_dF && d_dgate && d_work, "skr_mgcn_purify_bwd: NULL argument");
    SKR_REQUIRE(n_rows > 0, "skr_mgcn_purify_bwd: n_rows = %d", n_rows);
    SKR_REQUIRE(work_bytes >= skr_mgcn_purify_bwd_workspace(n_rows), "skr_mgcn_purify_bwd: work holds %zu bytes, %zu are needed", work_bytes,
                skr_mgcn_purify_bwd_workspace(n_rows));
    SKR_REQUIRE(((reinterpret_cast<uintptr_t>(d_dX) | reinterpret_cast<uintptr_t>(d_E) | reinterpret_cast<uintptr_t>(d_g) |
                  reinterpret_cast<uintptr_t>(d_F) | reinterpret_cast<uintptr_t>(d_gate) | reinterpret_cast<uintptr_t>(d_dE) |
                  reinterpret_cast<uintptr_t>(d_dF) | reinterpret_cast<uintptr_t>(d_dgate) | reinterpret_cast<uintptr_t>(d_work)) & 15) == 0,
                "skr_mgcn_purify_bwd: the tables and work must be 16-byte aligned");
    float* w = static_cast<float*>(d_work);
    return purify_bwd(d_dX, d_E, d_g, d_F, d_gate, n_rows, d_dE, d_dF, d_dgate, w, w + static_cast<int64_t>(n_rows) * D, skr::as_stream(stream));
}

int skr_mgcn_fuse(const float* d_M, const float* d_Zv, const float* d_Zt, const float* d_query, const float* d_pref_v, const float* d_pref_t,
                  int64_t n_rows, int dim, float* d_out, float* d_w, void* stream) {
    SKR_REQUIRE(d_M && d_Zv && d_Zt && d_query && d_pref_v && d_pref_t && d_out, "skr_mgcn_fuse: NULL argument");
    SKR_REQUIRE(n_rows > 0 && n_rows <= 2147483647LL && dim >= 1 && dim <= D, "skr_mgcn_fuse: n_rows = %lld, 1 <= dim <= 64 (got %d)",
                static_cast<long long>(n_rows), dim);
    SKR_REQUIRE(((reinterpret_cast<uintptr_t>(d_M) | reinterpret_cast<uintptr_t>(d_Zv) | reinterpret_cast<uintptr_t>(d_Zt) |
                  reinterpret_cast<uintptr_t>(d_query) | reinterpret_cast<uintptr_t>(d_pref_v) | reinterpret_cast<uintptr_t>(d_pref_t) |
                  reinterpret_cast<uintptr_t>(d_out)) & 15) == 0,
                "skr_mgcn_fuse: the tables must be 16-byte aligned");
    FuseParams fp = {};
    fp.M = d_M; fp.Zv = d_Zv; fp.Zt = d_Zt; fp.query = d_query; fp.pref_v = d_pref_v; fp.pref_t = d_pref_t;
    fp.n = static_cast<int>(n_rows); fp.dim = dim; fp.out = d_out; fp.w = d_w;
    hipLaunchKernelGGL(mg_fuse_kernel, dim3(tile_blocks(n_rows)), dim3(HW * 64), 0, skr::as_stream(stream), fp);
    SKR_LAUNCH_CHECK();
    return SKR_OK;
}

size_t skr_mgcn_workspace(int n, int n_items, int feat_ld_max) {
    if (n <= 0 || n > MAXB || n_items <= 0 || feat_ld_max <= 0 || feat_ld_max > MAXF) return 0;
    return static_cast<size_t>(step_layout(n, n_items, feat_ld_max).total) * sizeof(float);
}

int skr_mgcn_step(const skr_mgcn_step_args* args, void* stream) { return run_step(args, stream, nullptr); }

int skr_mgcn_step_timed(const skr_mgcn_step_args* args, void* stream, float* h_ms) {
    SKR_REQUIRE(h_ms != nullptr, "skr_mgcn_step_timed: NULL argument");
    return run_step(args, stream, h_ms);
}

}  // extern "C"
