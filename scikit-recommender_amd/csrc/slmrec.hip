// slmrec.hip -- SLMRec (Self-supervised Learning for Multimedia Recommendation, TMM 2022): two constant, row-normalised feature
// tables projected to 64 columns over ALL items, three LightGCN-style propagations over the user-item graph (the id table and
// the two projected tables, each with the user embeddings on top), two Linear(3 d, d) fusion layers, a cosine InfoNCE between
// the batch's users and items, and two un-normalised InfoNCE terms through a chain of five small linear layers ("fine and
// coarse").  Here: the batch kernels and the host entry that issues one training step, and the row-local fusion of the ranking.
//
// Replaces the stock torch ops the reference issues (no native code there):
//   recommender/SLMRec.py:136-142  v_dense / t_dense on the whole [I, F] tables (skr_mgcn_project)
//   recommender/SLMRec.py:144-165  3 x layer_num torch.sparse.mm on the square adjacency, stack and mean
//   recommender/SLMRec.py:174-175  the fusion layers over all U + I rows (here: at the batch's 2 n rows in training)
//   recommender/SLMRec.py:337-362, 423-432  three [B, B] logit matrices (here none is formed) and autograd's backward
//
// Layout: see include/skrec_hip.h, section O.
//
// Launches of a step:
//   2 project        D_m = X_m W_m^T + b_m over all items
//   6 L plan runs    the layer means M[0..2] in the accum epilogue (step_common.h); the user rows of all three start from E_u
//   prep, fuse       node ids of the n16 slots (-1 where a batch row names an id out of range); both fusion blocks through LDS on
//                    v_mfma_f32_16x16x4_f32, keeping the gathered rows
//   linear x 3       x, y, w (one launch); g_iv_iva(x); z: the five chain layers, a gate block in LDS each
//   norm, lse, loss  the row norms; per term an online log-sum-exp over the n columns, tile after tile on the matrix pipe
//   nce_grad         per term and side the weighted sums P B - B_r, P^T A - A_k; the normalisation's backward for the main term
//   rows_w, xty      the chain's and the fusion's backward and the seven weight gradients (dense_ops.h: mgcn.hip's kernels)
//   rank, seg_add    one writer per distinct node id, rows added in rank order, into the three tables G[0..2]
//   plan runs        three backward chains acc = A acc + G / (L + 1); the user halves add up into grad in chain order
//   2 xty            dW_m = dD_m^T X_m | column sums (skr_slmrec_project_bwd_w: no dX, the features are constants)
//
// Determinism: no floating-point atomic; every reduction over rows is split into contiguous row blocks whose partial sums are
// added in block order.
#include "skr_common.h"
#include "mfma_tile.h"
#include "step_common.h"
#include "dense_ops.h"

#include <algorithm>

namespace {

using namespace skr;

constexpr int D = 64;          // columns of every table
constexpr int D3 = 192;        // columns of a fusion block's input
constexpr int HW = 4;          // wavefronts per workgroup
constexpr int TB = HW * 16;    // rows per workgroup of the tiled kernels
constexpr int LD = 68;         // row stride of the LDS images
constexpr int MAXB = SKR_SLMREC_MAX_BATCH;
constexpr int MAXL = SKR_SLMREC_MAX_LAYERS;
constexpr int MAXF = SKR_SLMREC_MAX_FEAT;
constexpr float NORM_EPS = 1e-12f; // F.normalize

// rows[b] = users[b], rows[n16 + b] = n_users + pos[b]; -1 in both where either id is out of range or b >= n
__global__ __launch_bounds__(256) void sl_prep_kernel(const int32_t* __restrict__ users, const int32_t* __restrict__ pos, int n, int n16, int U,
                                                      int I, int32_t* __restrict__ rows) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= n16) return;
    int u = -1, i = -1;
    if (b < n) {
        u = users[b];
        i = pos[b];
        if (u < 0 || u >= U || i < 0 || i >= I) u = i = -1;
    }
    rows[b] = u;
    rows[n16 + b] = i < 0 ? -1 : U + i;
}

// ------------------------------------------------------------------------------------------------
// the fusion: out[r] = W [Mi_r | Mv_r | Mt_r] + b.  The block's three 64 x 64 slices lie in LDS (3 x 17 KB); a wavefront owns a
// 16-row tile and adds the three products into one set of accumulators.
// ------------------------------------------------------------------------------------------------
struct FuseSide {
    const float* M[3];             // the three tables (for the ranking: the side's first row)
    const float* fusion;           // W [64][192] | b [64]
    const int32_t* rows;           // [n] node ids, -1: no row; NULL: row b is node b
    float* out;                    // [n][64]
    float* cat;                    // [n][192] the gathered [Mi | Mv | Mt], or NULL
    float* zg;                     // [3][n][64] the same rows table by table, or NULL
};
struct FuseParams {
    FuseSide side[2];
    int64_t n;
};

__global__ __launch_bounds__(HW * 64) void sl_fuse_kernel(FuseParams p) {
    __shared__ __attribute__((aligned(16))) float sW[3][D * LD];
    const FuseSide& s = p.side[blockIdx.y];
    {   // W[o][64 t + c] -> sW[t][o][c]
        const float4* W4 = reinterpret_cast<const float4*>(s.fusion);
        for (int idx = threadIdx.x; idx < D * (D3 / 4); idx += HW * 64) {
            const int o = idx / (D3 / 4), c4 = idx - o * (D3 / 4);
            const int t = c4 >> 4, c = (c4 & 15) * 4;
            *reinterpret_cast<float4*>(&sW[t][o * LD + c]) = W4[idx];
        }
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
    const int64_t b0 = static_cast<int64_t>(blockIdx.x) * TB + wv * 16;
    const int64_t n = p.n;
    if (b0 >= n) return;
    const int64_t node = b0 + r < n ? (s.rows ? static_cast<int64_t>(s.rows[b0 + r]) : b0 + r) : -1;
    float a[16];
    f32x4 acc[4];
    zero_acc(acc);
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        load_row_a(a, s.M[t], node, g);
        tile_product<LD, 16>(acc, a, sW[t], r, g);
    }
    const float* __restrict__ bias = s.fusion + D * D3;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        const int64_t row = b0 + 4 * g + rr;
        // the node of row 4 g + rr: the ranking's row index may pass 2^31, a batch's node id does not
        const int64_t nd = s.rows ? static_cast<int64_t>(__shfl(static_cast<int>(node), 4 * g + rr, 64)) : (row < n ? row : -1);
        if (row >= n) continue;
        const bool ok = nd >= 0;
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) {
            const int col = nb * 16 + r;
            s.out[row * D + col] = ok ? acc[nb][rr] + bias[col] : 0.0f;
            if (s.cat) {
#pragma unroll
                for (int t = 0; t < 3; ++t) {
                    const float v = ok ? s.M[t][nd * D + col] : 0.0f;
                    s.cat[row * D3 + t * D + col] = v;
                    if (s.zg) s.zg[(static_cast<int64_t>(t) * n + row) * D + col] = v;
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// a chain layer: Y[b] = X[b] W^T + bias over the n16 slots (zero where the batch row is no row), the gate block in LDS; up to
// three independent layers per launch (blockIdx.y)
// ------------------------------------------------------------------------------------------------
struct LinearJobs {
    const float* X[3];             // [n16][64]
    const float* gate[3];          // W [64][64] | b [64]
    float* Y[3];                   // [n16][64]
};

__global__ __launch_bounds__(HW * 64) void sl_linear_kernel(LinearJobs p, const int32_t* __restrict__ rows, int n16) {
    __shared__ __attribute__((aligned(16))) float sW[D * LD];
    const float* __restrict__ gate = p.gate[blockIdx.y];
    load_tile<LD, HW>(sW, gate, 0, D);
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
    const int b0 = blockIdx.x * TB + wv * 16;
    if (b0 >= n16) return;
    float a[16];
    load_row_a(a, p.X[blockIdx.y], b0 + r < n16 ? b0 + r : -1, g);
    f64x4 acc[4];
    zero_acc64(acc);
    tile_product64<LD, 16>(acc, a, sW, r, g);
    const float* __restrict__ bias = gate + D * D;
    float* __restrict__ Y = p.Y[blockIdx.y];
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        const int row = b0 + g + 4 * rr;
        if (row >= n16) continue;
        const bool ok = rows[row] >= 0;
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) {
            const int col = nb * 16 + r;
            Y[static_cast<int64_t>(row) * D + col] = ok ? static_cast<float>(acc[nb][rr] + static_cast<double>(bias[col])) : 0.0f;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// the three InfoNCE terms t = 0 (main: A = user / |user|, B = item / |item|), 1 (A = x, B = y), 2 (A = z, B = w): A and B are
// [3][n16][64], zero rows where the batch row is no row
// ------------------------------------------------------------------------------------------------
struct Scales {
    float inv_tau[3];              // 1 / temp, 1 / ssl_temp, 1 / ssl_temp
    float coef[3];                 // weight of the term / (tau n): the factor of its gradient with respect to A and B
    float weight[3];               // 1, ssl_alpha, ssl_alpha
};

// a wavefront per slot: the normalised rows of the main term and their norms
__global__ __launch_bounds__(HW * 64) void sl_norm_kernel(const float* __restrict__ out_u, const float* __restrict__ out_i,
                                                          const int32_t* __restrict__ rows, int n16, float* __restrict__ AH,
                                                          float* __restrict__ BH, float* __restrict__ NA, float* __restrict__ NB) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int b = blockIdx.x * HW + wv;
    if (b >= n16) return;
    const bool ok = rows[b] >= 0;
    const float a = ok ? out_u[static_cast<int64_t>(b) * D + lane] : 0.0f, bb = ok ? out_i[static_cast<int64_t>(b) * D + lane] : 0.0f;
    const double da = a, db = bb;
    const float na = fmaxf(static_cast<float>(sqrt(wave_sum(da * da))), NORM_EPS), nb = fmaxf(static_cast<float>(sqrt(wave_sum(db * db))), NORM_EPS);
    AH[static_cast<int64_t>(b) * D + lane] = a / na;
    BH[static_cast<int64_t>(b) * D + lane] = bb / nb;
    if (lane == 0) { NA[b] = na; NB[b] = nb; }
}

__device__ __forceinline__ double max16d(double v) {
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

// lse[r] = log sum_k exp(l_rk), l_rk = <a_r, b_k> / tau over the batch's rows k, as an online log-sum-exp: a lane keeps a running
// maximum and a sum scaled by it over its columns (tile after tile, in column order), the 16 lanes of a row are joined at the
// end by a fixed tree.  The FAC logits are unbounded: nothing is exponentiated before the maximum is taken off.  The logits
// leave the matrix pipe in float64 and stay there: lse is kept as a double, because an lse rounded to fp32 scales every weight
// P_rk = exp(l_rk - lse_r) of its row by the same 1 + 5e-7, which the column sums behind the bias gradients do not average out
// (measured on the golden run's first batch: their root mean square error against float64 was 4 x that of a torch-CPU fp32
// evaluation).  rowloss[r] = (top - l_rr) + log(sum): the diagonal logit is the very value the sum saw, so that with one
// column, or with n equal columns, the row's loss is exactly 0, or log n.  A wavefront owns 16 rows and walks the columns 64 at
// a time.
__global__ __launch_bounds__(HW * 64) void sl_lse_kernel(const float* __restrict__ A3, const float* __restrict__ B3,
                                                         const int32_t* __restrict__ rows, int n, int n16, Scales sc, double* __restrict__ LSE,
                                                         float* __restrict__ ROWLOSS) {
    __shared__ __attribute__((aligned(16))) float sY[D * LD];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
    const int t = blockIdx.y;
    const int q0 = blockIdx.x * TB + wv * 16;
    const float* __restrict__ A = A3 + static_cast<int64_t>(t) * n16 * D;
    const float* __restrict__ B = B3 + static_cast<int64_t>(t) * n16 * D;
    const double inv_tau = static_cast<double>(sc.inv_tau[t]);
    float a[16];
    load_a(a, A, q0, n16, r, g);
    double mx[4], s[4], dg[4];
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) { mx[rr] = -INFINITY; s[rr] = 0.0; dg[rr] = 0.0; }
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
            double l[4], tm = mx[rr];
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) {
                l[nb] = acc[nb][rr] * inv_tau;
                tm = okc[nb] ? fmax(tm, l[nb]) : tm;
                if (c0 + nb * 16 + r == q0 + g + 4 * rr) dg[rr] = l[nb];
            }
            if (tm == -INFINITY) continue;
            double ts = s[rr] * exp(mx[rr] - tm);
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) ts += okc[nb] ? exp(l[nb] - tm) : 0.0;
            mx[rr] = tm;
            s[rr] = ts;
        }
    }
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        const double top = max16d(mx[rr]);
        const double tot = sum16d(top == -INFINITY || mx[rr] == -INFINITY ? 0.0 : s[rr] * exp(mx[rr] - top));
        const double diag = sum16d(dg[rr]);      // one lane of the 16 holds it, the others 0
        const int row = q0 + g + 4 * rr;
        if (r == 0 && row < n16) {
            const bool ok = row < n && rows[row] >= 0 && tot > 0.0;
            LSE[static_cast<int64_t>(t) * n16 + row] = ok ? top + log(tot) : 0.0;
            ROWLOSS[static_cast<int64_t>(t) * n16 + row] = ok ? static_cast<float>((top - diag) + log(tot)) : 0.0f;
        }
    }
}

// z = 0: dA[r] = coef (sum_k P_rk b_k - b_r); z = 1: dB[k] = coef (sum_r P_rk a_r - a_k), P_rk = exp(l_rk - lse_r); for the main
// term then the backward of the normalisation.  The owner's 16 x 64 weights go through LDS to become the A operand of the second
// product, whose B operand is the same LDS tile read by columns (mgcn.hip's mg_nce_grad_kernel, three terms and any tau).
__global__ __launch_bounds__(HW * 64) void sl_nce_grad_kernel(const float* __restrict__ A3, const float* __restrict__ B3, const float* __restrict__ NA,
                                                              const float* __restrict__ NB, const double* __restrict__ LSE,
                                                              const int32_t* __restrict__ rows, int n, int n16, Scales sc,
                                                              float* __restrict__ dA3, float* __restrict__ dB3) {
    __shared__ __attribute__((aligned(16))) float sY[D * LD];
    __shared__ __attribute__((aligned(16))) double sP[HW][16 * LD];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
    const int t = blockIdx.y, z = blockIdx.z;
    const int q0 = blockIdx.x * TB + wv * 16;
    const int64_t to = static_cast<int64_t>(t) * n16;
    const float* __restrict__ X = (z == 0 ? A3 : B3) + to * D;
    const float* __restrict__ Y = (z == 0 ? B3 : A3) + to * D;
    const double* __restrict__ lse = LSE + to;
    const double inv_tau = static_cast<double>(sc.inv_tau[t]);
    float a[16];
    load_a(a, X, q0, n16, r, g);
    bool ok_o[4];
    double lse_o[4];
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        const int row = q0 + g + 4 * rr;
        ok_o[rr] = row < n && rows[row] >= 0;
        lse_o[rr] = ok_o[rr] ? lse[row] : 0.0;
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
            const double lse_c = okc ? lse[col] : 0.0;
#pragma unroll
            for (int rr = 0; rr < 4; ++rr)
                sP[wv][(g + 4 * rr) * LD + nb * 16 + r] = okc && ok_o[rr] ? exp(acc[nb][rr] * inv_tau - (z == 0 ? lse_o[rr] : lse_c)) : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) {
            const double pa = sP[wv][r * LD + 4 * kk + g];
#pragma unroll
            for (int nb = 0; nb < 4; ++nb)
                acc2[nb] = __builtin_amdgcn_mfma_f64_16x16x4f64(pa, static_cast<double>(sY[(4 * kk + g) * LD + nb * 16 + r]), acc2[nb], 0, 0, 0);
        }
    }
    float* __restrict__ dst = (z == 0 ? dA3 : dB3) + to * D;
    const float* __restrict__ norm = z == 0 ? NA : NB;
    const double coef = static_cast<double>(sc.coef[t]);
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
            dh[nb] = ok_o[rr] ? (acc2[nb][rr] - static_cast<double>(yh)) * coef : 0.0;
            dot += static_cast<double>(xh[nb]) * dh[nb];
        }
        dot = sum16d(dot);
        if (!in) continue;
        if (t == 0) {
            const float inv = ok_o[rr] ? 1.0f / norm[row] : 0.0f;
#pragma unroll
            for (int nb = 0; nb < 4; ++nb)
                dst[static_cast<int64_t>(row) * D + nb * 16 + r] = static_cast<float>((dh[nb] - static_cast<double>(xh[nb]) * dot) * static_cast<double>(inv));
        } else {
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) dst[static_cast<int64_t>(row) * D + nb * 16 + r] = static_cast<float>(dh[nb]);
        }
    }
}

// loss[t] = weight_t * (the sum of the term's row losses, in a fixed order) / n; loss[3] = their sum
__global__ __launch_bounds__(64) void sl_loss_kernel(const float* __restrict__ ROWLOSS, int n, int n16, Scales sc, float* __restrict__ loss) {
    const int lane = threadIdx.x;
    float l[3];
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        double v = 0.0;
        for (int b = lane; b < n; b += 64) v += static_cast<double>(ROWLOSS[static_cast<int64_t>(t) * n16 + b]);
        v = wave_sum(v);
        l[t] = sc.weight[t] * static_cast<float>(v / static_cast<double>(n));
    }
    if (lane != 0) return;
    loss[0] = l[0]; loss[1] = l[1]; loss[2] = l[2]; loss[3] = (l[0] + l[1]) + l[2];
}

// G_t[node] = the sum of the gradient rows of the slots whose list entry is the node's id, in rank order, by the wavefront of
// the id's first rank: one writer per distinct id (the three tables are cleared first).  A user slot's rows are the three
// 64-column slices of dcat_u; an item slot's those of dcat_i plus the chain's rows fac[t].
__global__ __launch_bounds__(HW * 64) void sl_seg_add_kernel(float* __restrict__ G0, float* __restrict__ G1, float* __restrict__ G2,
                                                             const float* __restrict__ dcat_u, const float* __restrict__ dcat_i,
                                                             const float* __restrict__ fac, const int32_t* __restrict__ users,
                                                             const int32_t* __restrict__ pos, const int32_t* __restrict__ order_u,
                                                             const int32_t* __restrict__ order_i, int n, int n16, int U, int I, int blocks_u) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const bool user = static_cast<int>(blockIdx.x) < blocks_u;
    const int rk = (user ? blockIdx.x : blockIdx.x - blocks_u) * HW + wv;
    if (rk >= n) return;
    const int32_t* __restrict__ order = user ? order_u : order_i;
    const int32_t* __restrict__ ids = user ? users : pos;
    const int id = ids[order[rk]];
    if (id < 0 || id >= (user ? U : I)) return;
    if (rk > 0 && ids[order[rk - 1]] == id) return;
    float acc[3] = {0.0f, 0.0f, 0.0f};
    for (int k = rk; k < n; ++k) {
        const int64_t o = order[k];
        if (ids[o] != id) break;
#pragma unroll
        for (int t = 0; t < 3; ++t)
            acc[t] += user ? dcat_u[o * D3 + t * D + lane] : dcat_i[o * D3 + t * D + lane] + fac[(static_cast<int64_t>(t) * n16 + o) * D + lane];
    }
    const int64_t e = (static_cast<int64_t>(user ? 0 : U) + id) * D + lane;
    G0[e] = acc[0];
    G1[e] = acc[1];
    G2[e] = acc[2];
}

// n_layers == 0: out = (a + b) + c
__global__ __launch_bounds__(256) void sl_add3_kernel(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ c,
                                                      int64_t len, float* __restrict__ out) {
    const int64_t e = blockIdx.x * static_cast<int64_t>(256) + threadIdx.x;
    if (e < len) out[e] = (a[e] + b[e]) + c[e];
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
inline unsigned tile_blocks(int64_t n) { return static_cast<unsigned>((n + TB - 1) / TB); }

int check_feature(const char* who, int F, int ld) {
    SKR_REQUIRE(F >= 1 && F <= MAXF, "%s: 1 <= feat_dim <= %d (got %d)", who, MAXF, F);
    SKR_REQUIRE(ld >= F && ld % 4 == 0 && ld <= MAXF, "%s: feat_ld = %d must be a multiple of 4, >= feat_dim = %d and <= %d", who, ld, F, MAXF);
    return SKR_OK;
}

struct StepLayout {            // float offsets into the step's workspace
    int64_t rows, cat, zg, out, A, B, x2, na, nb, lse, rowloss, dA, dB, dx2, dcat, fac, ordu, ordi, part, total;
    int64_t part_floats;
};

inline StepLayout step_layout(int n, int n_items, int ld_max) {
    StepLayout L;
    const int64_t n16 = (static_cast<int64_t>(n) + 15) / 16 * 16;
    int64_t o = 0;
    L.rows = o; o += 2 * n16;
    L.cat = o; o += 2 * n16 * D3;
    L.zg = o; o += 3 * n16 * D;
    L.out = o; o += 2 * n16 * D;
    L.A = o; o += 3 * n16 * D;
    L.B = o; o += 3 * n16 * D;
    L.x2 = o; o += n16 * D;
    L.na = o; o += n16;
    L.nb = o; o += n16;
    L.lse = o; o += round4(6 * n16);      // doubles
    L.rowloss = o; o += round4(3 * n16);
    L.dA = o; o += 3 * n16 * D;
    L.dB = o; o += 3 * n16 * D;
    L.dx2 = o; o += n16 * D;
    L.dcat = o; o += 2 * n16 * D3;
    L.fac = o; o += 3 * n16 * D;
    L.ordu = o; o += n16;
    L.ordi = o; o += n16;
    L.part_floats = std::max(dense_xty_floats(n_items, std::max(ld_max, D)), dense_xty_floats(n16, D3));    // the widest of the reductions' partials
    L.part = o; o += L.part_floats;
    L.total = o;
    return L;
}

// mean_forward of step_common.h with the table's two halves in different buffers: M = mean_k A^k [Xu0; Xi0]
int mean_forward_split(const skr_spmm_plan* plan_a, const skr_spmm_plan* plan_at, const float* Xu0, const float* Xi0, int64_t U, int64_t I, int L,
                       float* const* ping, float* M, void* stream) {
    const int64_t UO = U * D;
    hipStream_t st = as_stream(stream);
    if (L == 0) {
        SKR_HIP(hipMemcpyAsync(M, Xu0, static_cast<size_t>(UO) * sizeof(float), hipMemcpyDeviceToDevice, st));
        SKR_HIP(hipMemcpyAsync(M + UO, Xi0, static_cast<size_t>(I) * D * sizeof(float), hipMemcpyDeviceToDevice, st));
        return SKR_OK;
    }
    const float *Xu = Xu0, *Xi = Xi0;
    for (int k = 1; k <= L; ++k) {
        float* Y = k == L ? nullptr : ping[(k - 1) & 1];
        skr_spmm_epilogue ep = {};
        ep.mode = SKR_EPI_PLAIN;
        ep.accum_scale = 1.0f / static_cast<float>(L + 1);
        ep.Y = Y;
        ep.accum = M;
        ep.accum_base = k == 1 ? Xu0 : nullptr;
        int rc = skr_spmm_plan_run_ex(plan_a, Xi, D, &ep, nullptr, nullptr, stream);
        if (rc != SKR_OK) return rc;
        ep.Y = Y ? Y + UO : nullptr;
        ep.accum = M + UO;
        ep.accum_base = k == 1 ? Xi0 : nullptr;
        rc = skr_spmm_plan_run_ex(plan_at, Xu, D, &ep, nullptr, nullptr, stream);
        if (rc != SKR_OK) return rc;
        Xu = Y;
        Xi = Y ? Y + UO : nullptr;
    }
    return SKR_OK;
}

// chain_backward of step_common.h for L >= 1 whose last product ADDS the user half into grad_u and WRITES the item half to out_i
int chain_backward_split(const skr_spmm_plan* plan_a, const skr_spmm_plan* plan_at, const float* G, int64_t UO, int L, float* const* ping,
                         float* grad_u, float* out_i, void* stream) {
    const float* X = G;
    for (int k = 1; k <= L; ++k) {
        const bool last = k == L;
        float* Y = last ? nullptr : ping[(k - 1) & 1];
        skr_spmm_epilogue ep = {};
        ep.mode = SKR_EPI_PLAIN;
        ep.accum_scale = 1.0f / static_cast<float>(L + 1);
        ep.addend = G;
        ep.Y = Y;
        if (last) { ep.accum = grad_u; ep.accum_init = 0; }
        int rc = skr_spmm_plan_run_ex(plan_a, X + UO, D, &ep, nullptr, nullptr, stream);
        if (rc != SKR_OK) return rc;
        ep.addend = G + UO;
        ep.Y = Y ? Y + UO : nullptr;
        if (last) { ep.accum = out_i; ep.accum_init = 1; }
        rc = skr_spmm_plan_run_ex(plan_at, X, D, &ep, nullptr, nullptr, stream);
        if (rc != SKR_OK) return rc;
        X = Y;
    }
    return SKR_OK;
}

int run_step(const skr_slmrec_step_args* a, void* stream, float* h_ms) {
    SKR_REQUIRE(a, "skr_slmrec_step: NULL argument");
    const int U = a->n_users, I = a->n_items, n = a->n, L = a->n_layers;
    SKR_REQUIRE(a->params && a->users && a->pos && a->grad && a->loss && a->work && a->fusion_user && a->fusion_item && a->fusion_user_grad &&
                    a->fusion_item_grad && a->dD,
                "skr_slmrec_step: NULL argument");
    SKR_REQUIRE(U > 0 && I > 0 && n >= 0 && n <= MAXB, "skr_slmrec_step: n_users = %d, n_items = %d, n = %d (at most %d rows)", U, I, n, MAXB);
    SKR_REQUIRE(a->dim >= 1 && a->dim <= D, "skr_slmrec_step: 1 <= dim <= 64 (got %d); rows are 64 floats, zero-padded", a->dim);
    SKR_REQUIRE(L >= 0 && L <= MAXL, "skr_slmrec_step: 0 <= n_layers <= %d (got %d)", MAXL, L);
    SKR_REQUIRE(a->plan_a && a->plan_at, "skr_slmrec_step: NULL plan: both plans of the user-item graph are needed");
    SKR_REQUIRE(a->ping[0] && a->ping[1], "skr_slmrec_step: both ping tables are needed");
    SKR_REQUIRE(a->temp > 0.0f && a->ssl_temp > 0.0f && a->ssl_alpha >= 0.0f, "skr_slmrec_step: temp = %g, ssl_temp = %g (> 0), ssl_alpha = %g (>= 0)",
                a->temp, a->ssl_temp, a->ssl_alpha);
    uintptr_t align = reinterpret_cast<uintptr_t>(a->params) | reinterpret_cast<uintptr_t>(a->grad) | reinterpret_cast<uintptr_t>(a->work) |
                      reinterpret_cast<uintptr_t>(a->ping[0]) | reinterpret_cast<uintptr_t>(a->ping[1]) | reinterpret_cast<uintptr_t>(a->dD) |
                      reinterpret_cast<uintptr_t>(a->fusion_user) | reinterpret_cast<uintptr_t>(a->fusion_item) |
                      reinterpret_cast<uintptr_t>(a->fusion_user_grad) | reinterpret_cast<uintptr_t>(a->fusion_item_grad);
    int ld_max = 0;
    for (int m = 0; m < 2; ++m) {
        const int rc = check_feature("skr_slmrec_step", a->feat_dim[m], a->feat_ld[m]);
        if (rc != SKR_OK) return rc;
        ld_max = std::max(ld_max, a->feat_ld[m]);
        SKR_REQUIRE(a->dense[m] && a->feat[m] && a->D[m] && a->dense_grad[m], "skr_slmrec_step: both modalities need their tables");
        align |= reinterpret_cast<uintptr_t>(a->dense[m]) | reinterpret_cast<uintptr_t>(a->feat[m]) | reinterpret_cast<uintptr_t>(a->D[m]) |
                 reinterpret_cast<uintptr_t>(a->dense_grad[m]);
    }
    for (int t = 0; t < 3; ++t) {
        SKR_REQUIRE(a->M[t] && a->G[t], "skr_slmrec_step: the three tables M and the three gradient tables G are needed");
        align |= reinterpret_cast<uintptr_t>(a->M[t]) | reinterpret_cast<uintptr_t>(a->G[t]);
    }
    for (int c = 0; c < 5; ++c) {
        SKR_REQUIRE(a->chain[c] && a->chain_grad[c], "skr_slmrec_step: the five chain layers need their blocks");
        align |= reinterpret_cast<uintptr_t>(a->chain[c]) | reinterpret_cast<uintptr_t>(a->chain_grad[c]);
    }
    SKR_REQUIRE((align & 15) == 0, "skr_slmrec_step: the tables and work must be 16-byte aligned");
    if (n == 0) return SKR_OK;
    const StepLayout W = step_layout(n, I, ld_max);
    SKR_REQUIRE(a->work_bytes >= static_cast<size_t>(W.total) * sizeof(float),
                "skr_slmrec_step: work holds %zu bytes, skr_slmrec_workspace(%d, %d, %d) asks for %zu", a->work_bytes, n, I, ld_max,
                static_cast<size_t>(W.total) * sizeof(float));
    hipStream_t st = as_stream(stream);
    float* w = static_cast<float*>(a->work);
    int32_t* rows = reinterpret_cast<int32_t*>(w + W.rows);
    int32_t* ordu = reinterpret_cast<int32_t*>(w + W.ordu);
    int32_t* ordi = reinterpret_cast<int32_t*>(w + W.ordi);
    double* lse = reinterpret_cast<double*>(w + W.lse);
    const int n16 = (n + 15) / 16 * 16;
    const int64_t S = static_cast<int64_t>(n16) * D, S3 = static_cast<int64_t>(n16) * D3;
    const int64_t UO = static_cast<int64_t>(U) * D, N = static_cast<int64_t>(U) + I;
    const size_t part_bytes = static_cast<size_t>(W.part_floats) * sizeof(float);
    StepTimer<SKR_SLMREC_GROUPS + 1> mk(h_ms, st);
    SKR_HIP(mk.mark());
    int rc;
    // ---- 0: D_m = X_m W_m^T + b_m over all items (SLMRec.py:136-142)
    for (int m = 0; m < 2; ++m)
        if ((rc = skr_mgcn_project(a->feat[m], I, a->feat_dim[m], a->feat_ld[m], a->dense[m], a->D[m], stream)) != SKR_OK) return rc;
    SKR_HIP(mk.mark());
    // ---- 1: the three layer means (SLMRec.py:144-165)
    for (int t = 0; t < 3; ++t)
        if ((rc = mean_forward_split(a->plan_a, a->plan_at, a->params, t == 0 ? a->params + UO : a->D[t - 1], U, I, L, a->ping, a->M[t], stream)) != SKR_OK)
            return rc;
    SKR_HIP(mk.mark());
    // ---- 2: the batch forward (SLMRec.py:174-175 at the batch's rows, 337-362, 423-432)
    hipLaunchKernelGGL(sl_prep_kernel, dim3((n16 + 255) / 256), dim3(256), 0, st, a->users, a->pos, n, n16, U, I, rows);
    FuseParams fp = {};
    fp.n = n16;
    for (int s = 0; s < 2; ++s) {
        FuseSide& fs = fp.side[s];
        for (int t = 0; t < 3; ++t) fs.M[t] = a->M[t];
        fs.fusion = s == 0 ? a->fusion_user : a->fusion_item;
        fs.rows = rows + s * n16;
        fs.out = w + W.out + s * S;
        fs.cat = w + W.cat + s * S3;
        fs.zg = s == 1 ? w + W.zg : nullptr;
    }
    hipLaunchKernelGGL(sl_fuse_kernel, dim3(tile_blocks(n16), 2), dim3(HW * 64), 0, st, fp);
    float *A3 = w + W.A, *B3 = w + W.B, *dA3 = w + W.dA, *dB3 = w + W.dB;
    LinearJobs j1 = {{w + W.zg, w + W.zg + S, w + W.zg + 2 * S}, {a->chain[0], a->chain[1], a->chain[4]}, {A3 + S, B3 + S, B3 + 2 * S}};      // x, y, w
    hipLaunchKernelGGL(sl_linear_kernel, dim3(tile_blocks(n16), 3), dim3(HW * 64), 0, st, j1, rows, n16);
    LinearJobs j2 = {{A3 + S, nullptr, nullptr}, {a->chain[2], nullptr, nullptr}, {w + W.x2, nullptr, nullptr}};
    hipLaunchKernelGGL(sl_linear_kernel, dim3(tile_blocks(n16), 1), dim3(HW * 64), 0, st, j2, rows, n16);
    LinearJobs j3 = {{w + W.x2, nullptr, nullptr}, {a->chain[3], nullptr, nullptr}, {A3 + 2 * S, nullptr, nullptr}};                          // z
    hipLaunchKernelGGL(sl_linear_kernel, dim3(tile_blocks(n16), 1), dim3(HW * 64), 0, st, j3, rows, n16);
    hipLaunchKernelGGL(sl_norm_kernel, dim3(n16 / HW), dim3(HW * 64), 0, st, w + W.out, w + W.out + S, rows, n16, A3, B3, w + W.na, w + W.nb);
    const float inv_n = 1.0f / static_cast<float>(n), it = 1.0f / a->temp, is = 1.0f / a->ssl_temp;
    const Scales sc = {{it, is, is}, {it * inv_n, a->ssl_alpha * is * inv_n, a->ssl_alpha * is * inv_n}, {1.0f, a->ssl_alpha, a->ssl_alpha}};
    hipLaunchKernelGGL(sl_lse_kernel, dim3(tile_blocks(n16), 3), dim3(HW * 64), 0, st, A3, B3, rows, n, n16, sc, lse, w + W.rowloss);
    hipLaunchKernelGGL(sl_loss_kernel, dim3(1), dim3(64), 0, st, w + W.rowloss, n, n16, sc, a->loss);
    SKR_LAUNCH_CHECK();
    SKR_HIP(mk.mark());
    // ---- 3: the batch backward: the three terms, the chain, the fusion, the seven weight gradients
    hipLaunchKernelGGL(sl_nce_grad_kernel, dim3(tile_blocks(n16), 3, 2), dim3(HW * 64), 0, st, A3, B3, w + W.na, w + W.nb, lse, rows, n, n16, sc, dA3, dB3);
    SKR_LAUNCH_CHECK();
    float* part = w + W.part;
    if ((rc = dense_xty(dA3 + 2 * S, w + W.x2, n16, D, part, a->chain_grad[3], st)) != SKR_OK) return rc;           // g_iva_ivat: dz^T x2
    if ((rc = dense_rows_w(dA3 + 2 * S, n16, D, a->chain[3], w + W.dx2, 0, st)) != SKR_OK) return rc;               // dx2 = dz W
    if ((rc = dense_xty(w + W.dx2, A3 + S, n16, D, part, a->chain_grad[2], st)) != SKR_OK) return rc;               // g_iv_iva: dx2^T x
    if ((rc = dense_rows_w(w + W.dx2, n16, D, a->chain[2], dA3 + S, 1, st)) != SKR_OK) return rc;                   // dx += dx2 W
    if ((rc = dense_xty(dA3 + S, w + W.zg, n16, D, part, a->chain_grad[0], st)) != SKR_OK) return rc;               // g_i_iv
    if ((rc = dense_xty(dB3 + S, w + W.zg + S, n16, D, part, a->chain_grad[1], st)) != SKR_OK) return rc;           // g_v_iv
    if ((rc = dense_xty(dB3 + 2 * S, w + W.zg + 2 * S, n16, D, part, a->chain_grad[4], st)) != SKR_OK) return rc;   // g_t_ivat
    if ((rc = dense_rows_w(dA3 + S, n16, D, a->chain[0], w + W.fac, 0, st)) != SKR_OK) return rc;
    if ((rc = dense_rows_w(dB3 + S, n16, D, a->chain[1], w + W.fac + S, 0, st)) != SKR_OK) return rc;
    if ((rc = dense_rows_w(dB3 + 2 * S, n16, D, a->chain[4], w + W.fac + 2 * S, 0, st)) != SKR_OK) return rc;
    if ((rc = dense_xty(dA3, w + W.cat, n16, D3, part, a->fusion_user_grad, st)) != SKR_OK) return rc;
    if ((rc = dense_xty(dB3, w + W.cat + S3, n16, D3, part, a->fusion_item_grad, st)) != SKR_OK) return rc;
    if ((rc = dense_rows_w(dA3, n16, D3, a->fusion_user, w + W.dcat, 0, st)) != SKR_OK) return rc;
    if ((rc = dense_rows_w(dB3, n16, D3, a->fusion_item, w + W.dcat + S3, 0, st)) != SKR_OK) return rc;
    SKR_HIP(mk.mark());
    // ---- 4: the three dense gradient tables
    for (int t = 0; t < 3; ++t) SKR_HIP(hipMemsetAsync(a->G[t], 0, static_cast<size_t>(N) * D * sizeof(float), st));
    hipLaunchKernelGGL(rank_lists_kernel<256>, dim3((2 * n + 255) / 256), dim3(256), 0, st, a->users, a->pos, n, ordu, ordi);
    const int blocks = (n + HW - 1) / HW;
    hipLaunchKernelGGL(sl_seg_add_kernel, dim3(2 * blocks), dim3(HW * 64), 0, st, a->G[0], a->G[1], a->G[2], w + W.dcat, w + W.dcat + S3, w + W.fac,
                       a->users, a->pos, ordu, ordi, n, n16, U, I, blocks);
    SKR_LAUNCH_CHECK();
    SKR_HIP(mk.mark());
    // ---- 5, 6, 7: the backward chains (A is symmetric: the same plan pair); the user halves add up in chain order
    const auto product = [&](const skr_spmm_plan* plan, const float* X, const skr_spmm_epilogue& ep, bool) {
        return skr_spmm_plan_run_ex(plan, X, D, &ep, nullptr, nullptr, stream);
    };
    if (L == 0) {
        const int64_t len = UO;
        hipLaunchKernelGGL(sl_add3_kernel, dim3(static_cast<unsigned>((len + 255) / 256)), dim3(256), 0, st, a->G[0], a->G[1], a->G[2], len, a->grad);
        SKR_LAUNCH_CHECK();
        SKR_HIP(hipMemcpyAsync(a->grad + UO, a->G[0] + UO, static_cast<size_t>(I) * D * sizeof(float), hipMemcpyDeviceToDevice, st));
    } else if ((rc = chain_backward(a->plan_a, a->plan_at, a->G[0], UO, L, a->ping, a->grad, product)) != SKR_OK) {
        return rc;
    }
    SKR_HIP(mk.mark());
    for (int m = 0; m < 2; ++m) {
        const float* dD = a->G[1 + m] + UO;
        if (L > 0) {
            if ((rc = chain_backward_split(a->plan_a, a->plan_at, a->G[1 + m], UO, L, a->ping, a->grad, a->dD, stream)) != SKR_OK) return rc;
            dD = a->dD;
        }
        if ((rc = skr_slmrec_project_bwd_w(dD, a->feat[m], I, a->feat_dim[m], a->feat_ld[m], a->dense_grad[m], part, part_bytes, stream)) != SKR_OK)
            return rc;
        SKR_HIP(mk.mark());
    }
    SKR_HIP(mk.finish());
    return SKR_OK;
}

}  // namespace

extern "C" {

int skr_slmrec_fuse(const float* d_Mi, const float* d_Mv, const float* d_Mt, const float* d_fusion, int64_t n_rows, int dim, float* d_out,
                    void* stream) {
    SKR_REQUIRE(d_Mi && d_Mv && d_Mt && d_fusion && d_out, "skr_slmrec_fuse: NULL argument");
    SKR_REQUIRE(n_rows > 0 && n_rows <= 2147483647LL && dim >= 1 && dim <= D, "skr_slmrec_fuse: n_rows = %lld, 1 <= dim <= 64 (got %d)",
                static_cast<long long>(n_rows), dim);
    SKR_REQUIRE(((reinterpret_cast<uintptr_t>(d_Mi) | reinterpret_cast<uintptr_t>(d_Mv) | reinterpret_cast<uintptr_t>(d_Mt) |
                  reinterpret_cast<uintptr_t>(d_fusion) | reinterpret_cast<uintptr_t>(d_out)) & 15) == 0,
                "skr_slmrec_fuse: the tables must be 16-byte aligned");
    FuseParams fp = {};
    fp.n = n_rows;
    fp.side[0].M[0] = d_Mi; fp.side[0].M[1] = d_Mv; fp.side[0].M[2] = d_Mt;
    fp.side[0].fusion = d_fusion;
    fp.side[0].out = d_out;
    hipLaunchKernelGGL(sl_fuse_kernel, dim3(tile_blocks(n_rows), 1), dim3(HW * 64), 0, skr::as_stream(stream), fp);
    SKR_LAUNCH_CHECK();
    return SKR_OK;
}

size_t skr_slmrec_workspace(int n, int n_items, int feat_ld_max) {
    if (n <= 0 || n > MAXB || n_items <= 0 || feat_ld_max <= 0 || feat_ld_max > MAXF) return 0;
    return static_cast<size_t>(step_layout(n, n_items, feat_ld_max).total) * sizeof(float);
}

int skr_slmrec_step(const skr_slmrec_step_args* args, void* stream) { return run_step(args, stream, nullptr); }

int skr_slmrec_step_timed(const skr_slmrec_step_args* args, void* stream, float* h_ms) {
    SKR_REQUIRE(h_ms != nullptr, "skr_slmrec_step_timed: NULL argument");
    return run_step(args, stream, h_ms);
}

}  // extern "C"
