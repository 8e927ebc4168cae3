// sasrec.hip -- SASRec (self-attentive sequential recommendation): one training step, forward and backward, and the per-user
// query rows.
//
// Replaces the TensorFlow graph the reference builds and runs per step and per evaluation batch (no native code there):
//   recommender/SASRec.py:60-87     normalize
//   recommender/SASRec.py:174-269   multihead_attention (causal, key-masked, dropout on the weights, + queries)
//   recommender/SASRec.py:272-308   feedforward (two kernel-size-1 convolutions, dropout, + inputs)
//   recommender/SASRec.py:387-463   _build_model: the tables, the block stack, the two log losses, all_logits
//
// The launches of a step, in order (SKR_SASREC_LAUNCHES groups, the events of skr_sasrec_step_timed):
//   step      sas_step_kernel: at most SKR_SASREC_WORKGROUPS persistent workgroups of four wavefronts; workgroup w owns the
//             sequences w, w + G, ... and runs each one's forward, loss and backward.  The sequence's [64, 64] activations lie in
//             LDS (eight images of 64 x 68 floats, 136 KiB: one workgroup per CU); a 64 x 64 weight is staged through one of
//             them.  Every product runs on v_mfma_f32_16x16x4_f32: the three projections and the two feed-forward layers through
//             mfma_tile.h's tile_product, Q K^T, P V and the whole backward through mm<> below, which reads either operand by
//             rows or by columns, so that no image is ever transposed.  LayerNorm and softmax are 16-lane reductions on the
//             accumulators' own layout.  What the backward needs of a block (x, Q, K, V, y, relu(h)) goes to the workgroup's
//             part of the workspace; LayerNorm's statistics, the softmax and every keep flag are computed again.  A workgroup
//             adds its sequences' weight, bias and LayerNorm gradients into its own slab of the workspace, in sequence order.
//   reduce    the slabs are added in workgroup order into the shared block's gradient.
//   positions the position rows' gradient: for every (t, column) the sequences' rows in batch order.
//   rank      seq || pos || neg (3 n T ids) ranked by (id, list position) by counting, the list walked through LDS.
//   adds      one wavefront per distinct id adds that id's rows in rank order and adds sqrt(d) times the sum to the item rows'
//             gradient once.  The padding row and ids out of range get nothing.
//   loss      one workgroup adds the sequences' loss sums by a fixed tree and divides by the number of targets.
// No floating-point atomic anywhere: two calls on the same inputs give the same bits.
#include "skr_common.h"
#include "fast_rng.h"
#include "mfma_tile.h"
#include "step_common.h"

#include <cmath>

namespace {

using namespace skr;

constexpr int D = 64;
constexpr int HW = 4;             // wavefronts per workgroup
constexpr int NT = HW * 64;
constexpr int LD = 68;            // LDS row stride of a 64-float row (16-byte aligned rows, rows 4 banks apart)
constexpr int IMG = 64 * LD;      // floats of one LDS image
constexpr int SAVED = 6;          // images a block keeps for the backward: x, Q, K, V, y, relu(h)
constexpr int G = SKR_SASREC_WORKGROUPS;

// rows (of 64 floats) of a block's part of the shared parameters (the header's layout); weights are stored [out][in]
constexpr int R_G1 = 0, R_B1 = 1, R_WQ = 2, R_BQ = 66, R_WK = 67, R_BK = 131, R_WV = 132, R_BV = 196, R_G2 = 197, R_B2 = 198,
              R_W1 = 199, R_C1 = 263, R_W2 = 264, R_C2 = 328, R_BLOCK = SKR_SASREC_BLOCK_ROWS;
static_assert(R_C2 + 1 == R_BLOCK, "the block's rows");

struct Shape {
    int n, I, d, T, blocks, heads, dh, KS, shared_floats;
    float rate, scale, sqrt_d, inv_sqrt_dh;
};

inline Shape make_shape(int n, int I, int d, int T, int blocks, int heads, float rate) {
    Shape s;
    s.n = n; s.I = I; s.d = d; s.T = T; s.blocks = blocks; s.heads = heads;
    s.dh = d / heads;
    s.KS = SKR_SASREC_KEEP_BYTES(d, T, blocks, heads);
    s.shared_floats = SKR_SASREC_SHARED_FLOATS(blocks);
    s.rate = rate;
    s.scale = rate > 0.0f ? 1.0f / (1.0f - rate) : 1.0f;
    s.sqrt_d = sqrtf(static_cast<float>(d));
    s.inv_sqrt_dh = 1.0f / sqrtf(static_cast<float>(s.dh));
    return s;
}

// the keep flag of element e of a sequence's flag layout: handed in, drawn (keyed by seed, step, sequence, element) or 1
struct Keep {
    const uint8_t* in;
    float rate;
    uint64_t seed, step;
    int64_t b;
    int KS;
    __device__ __forceinline__ bool operator()(int e) const {
        if (in) return in[b * KS + e] != 0;
        if (!(rate > 0.0f)) return true;
        Xoshiro128pp g;
        g.seed(seed, step, (static_cast<uint64_t>(b) << 32) | static_cast<uint32_t>(e));
        return static_cast<float>(g.next() >> 8) * 0x1p-24f >= rate;
    }
};

struct Lds {
    float *X, *N, *W, *Q, *K, *V, *P, *T;
};

// Lane (r, g) of wavefront wv owns, of a [64, 64] result, the rows 16 wv + 4 g + rr and the columns 16 nb + r: the layout of
// mfma_tile.h's accumulators acc[nb][rr], and the layout LayerNorm and softmax work on.
#define OWN_LOOP                        \
    _Pragma("unroll") for (int nb = 0; nb < 4; ++nb) \
    _Pragma("unroll") for (int rr = 0; rr < 4; ++rr)

// acc[nb][rr] += sum_k A(row, k) B(k, col): A read by rows (sA[row][k]) or, AT, by columns (sA[k][row]); B by columns
// (sB[k][col]) or, BT, by rows (sB[col][k]); with !AT only k in [klo, khi) count (a head's columns).  k = 4 kk + g.
template <bool AT, bool BT>
__device__ __forceinline__ void mm(f32x4 acc[4], const float* __restrict__ sA, const float* __restrict__ sB, int wv, int r, int g,
                                   int klo = 0, int khi = 64) {
#pragma unroll 4
    for (int kk = 0; kk < 16; ++kk) {
        const int k = 4 * kk + g;
        float a = AT ? sA[k * LD + 16 * wv + r] : sA[(16 * wv + r) * LD + k];
        if (!AT) a = (k >= klo && k < khi) ? a : 0.0f;
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) {
            const float b = BT ? sB[(16 * nb + r) * LD + k] : sB[k * LD + 16 * nb + r];
            acc[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[nb], 0, 0, 0);
        }
    }
}

// acc = rows 16 wv .. 16 wv + 15 of sA times the weight image sW ([out][in]) transposed
__device__ __forceinline__ void linear(f32x4 acc[4], const float* __restrict__ sA, const float* __restrict__ sW, int wv, int r, int g) {
    float a[16];
    load_slab<LD>(a, sA, 16 * wv + r, g);
    zero_acc(acc);
    tile_product<LD, 16>(acc, a, sW, r, g);
}

__device__ __forceinline__ void img_store(float* __restrict__ dst, const float* __restrict__ s) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int idx = threadIdx.x + q * NT, row = idx >> 4, c4 = idx & 15;
        *reinterpret_cast<float4*>(dst + row * 64 + 4 * c4) = *reinterpret_cast<const float4*>(s + row * LD + 4 * c4);
    }
}
__device__ __forceinline__ void img_load(float* __restrict__ s, const float* __restrict__ src) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int idx = threadIdx.x + q * NT, row = idx >> 4, c4 = idx & 15;
        *reinterpret_cast<float4*>(s + row * LD + 4 * c4) = *reinterpret_cast<const float4*>(src + row * 64 + 4 * c4);
    }
}

// the reference's normalize over the true d columns of the owned rows: out = xh gamma + beta, xh = (x - mean) rstd
__device__ __forceinline__ void ln_rows(const float* __restrict__ sX, const float* __restrict__ gam, const float* __restrict__ bet, int d,
                                        int wv, int r, int g, float out[4][4], float xh[4][4], float rstd[4]) {
    const float inv_d = 1.0f / static_cast<float>(d);
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        const int row = 16 * wv + 4 * g + rr;
        float x[4], s = 0.0f;
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) {
            const int c = 16 * nb + r;
            x[nb] = c < d ? sX[row * LD + c] : 0.0f;
            s += x[nb];
        }
        const float mean = sum16(s) * inv_d;
        float q = 0.0f;
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) {
            const float dl = 16 * nb + r < d ? x[nb] - mean : 0.0f;
            q += dl * dl;
        }
        const float rs = 1.0f / sqrtf(sum16(q) * inv_d + 1e-8f);
        rstd[rr] = rs;
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) {
            const int c = 16 * nb + r;
            const bool in = c < d;
            const float h = in ? (x[nb] - mean) * rs : 0.0f;
            xh[nb][rr] = h;
            out[nb][rr] = in ? h * gam[c] + bet[c] : 0.0f;
        }
    }
}

// its backward on the same layout: dx = rstd (dxh - mean(dxh) - xh mean(dxh xh)), dxh = dy gamma
__device__ __forceinline__ void ln_bwd(const float dy[4][4], const float xh[4][4], const float rstd[4], const float* __restrict__ gam, int d,
                                       int r, float dx[4][4]) {
    const float inv_d = 1.0f / static_cast<float>(d);
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        float dh[4], a = 0.0f, b = 0.0f;
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) {
            const int c = 16 * nb + r;
            dh[nb] = c < d ? dy[nb][rr] * gam[c] : 0.0f;
            a += dh[nb];
            b += dh[nb] * xh[nb][rr];
        }
        const float m1 = sum16(a) * inv_d, m2 = sum16(b) * inv_d;
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) dx[nb][rr] = 16 * nb + r < d ? rstd[rr] * (dh[nb] - m1 - xh[nb][rr] * m2) : 0.0f;
    }
}

// the causal, key-masked softmax of the owned rows of the scores acc (times inv), in place of p; 0 where masked
__device__ __forceinline__ void softmax_own(const f32x4 acc[4], float p[4][4], const int* __restrict__ s_live, float inv, int wv, int r,
                                            int g) {
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        const int t = 16 * wv + 4 * g + rr;
        const bool lv = s_live[t] != 0;
        float s[4], m = -INFINITY;
        bool ok[4];
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) {
            const int j = 16 * nb + r;
            ok[nb] = lv && j <= t && s_live[j] != 0;
            s[nb] = ok[nb] ? acc[nb][rr] * inv : -INFINITY;
            m = fmaxf(m, s[nb]);
        }
        m = max16(m);
        float e[4], sum = 0.0f;
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) {
            e[nb] = ok[nb] ? expf(s[nb] - m) : 0.0f;
            sum += e[nb];
        }
        sum = sum16(sum);
        const float is = lv ? 1.0f / sum : 0.0f;       // a live query always has its own key
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) p[nb][rr] = e[nb] * is;
    }
}

// dst[o][i] += acc over the true d x d part (a weight's gradient in the workgroup's slab); always the same thread per element
__device__ __forceinline__ void slab_add(float* __restrict__ dst, const f32x4 acc[4], int d, int wv, int r, int g) {
    OWN_LOOP {
        const int o = 16 * wv + 4 * g + rr, i = 16 * nb + r;
        if (o < d && i < d) dst[o * 64 + i] += acc[nb][rr];
    }
}

// dst[c] += sum_t sA[t][c] (sB[t][c]) over the T rows, c < d: the first wavefront, a column per lane
__device__ __forceinline__ void col_add(float* __restrict__ dst, const float* __restrict__ sA, const float* __restrict__ sB, int T, int d) {
    const int c = threadIdx.x;
    if (c >= d) return;
    float s = 0.0f;
    for (int t = 0; t < T; ++t) {
        float v = sA[t * LD + c];
        if (sB) v *= sB[t * LD + c];
        s += v;
    }
    dst[c] += s;
}

// -log(sigmoid(y) + 1e-24) and its derivative
__device__ __forceinline__ float neg_log_sigmoid(float y, float& dy) {
    const float e = expf(-fabsf(y));
    if (y >= 0.0f) {
        dy = -(e / (1.0f + e));
        return log1pf(e);
    }
    const float s = e / (1.0f + e), q = 1.0f / (1.0f + e);
    dy = -(s * q) / (s + 1e-24f);
    return -logf(s + 1e-24f);
}

// x = mask dropout(sqrt(d) E[seq] + P) of all 64 rows (zeros beyond T and d)
__device__ __forceinline__ void input_rows(const Shape& S, float* __restrict__ sX, const float* __restrict__ E, const float* __restrict__ P,
                                           const int* __restrict__ s_seq, const int* __restrict__ s_live, const Keep* keep) {
    for (int idx = threadIdx.x; idx < 64 * 64; idx += NT) {
        const int t = idx >> 6, c = idx & 63;
        float v = 0.0f;
        if (s_live[t] && c < S.d) {
            v = S.sqrt_d * E[static_cast<int64_t>(s_seq[t]) * D + c] + P[t * D + c];
            if (keep) v = (*keep)(t * S.d + c) ? v * S.scale : 0.0f;
        }
        sX[t * LD + c] = v;
    }
}

// one block, forward: L.X (the block's input) -> L.X (its output).  only_wave >= 0: the rows of that wavefront alone go through
// the queries, the attention and the feed-forward part (the last block of the query rows).
template <bool TRAIN>
__device__ __forceinline__ void block_forward(const Shape& S, const Lds& L, const float* __restrict__ blk, float* __restrict__ save,
                                              const int* __restrict__ s_live, const Keep& keep, int kbase, int only_wave) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r = lane & 15, g = lane >> 4;
    const bool act = only_wave < 0 || wv == only_wave;
    const int d = S.d, T = S.T;
    f32x4 acc[4];
    if (TRAIN) img_store(save, L.X);
    {
        float o[4][4], xh[4][4], rs[4];
        ln_rows(L.X, blk + R_G1 * 64, blk + R_B1 * 64, d, wv, r, g, o, xh, rs);
        OWN_LOOP {
            const int row = 16 * wv + 4 * g + rr;
            L.N[row * LD + 16 * nb + r] = s_live[row] ? o[nb][rr] : 0.0f;
        }
    }
    load_tile<LD, HW>(L.W, blk + R_WQ * 64, 0, 64);
    __syncthreads();
    if (act) {
        linear(acc, L.N, L.W, wv, r, g);
        OWN_LOOP L.Q[(16 * wv + 4 * g + rr) * LD + 16 * nb + r] = acc[nb][rr] + blk[R_BQ * 64 + 16 * nb + r];
    }
    __syncthreads();
    load_tile<LD, HW>(L.W, blk + R_WK * 64, 0, 64);
    __syncthreads();
    linear(acc, L.X, L.W, wv, r, g);
    OWN_LOOP L.K[(16 * wv + 4 * g + rr) * LD + 16 * nb + r] = acc[nb][rr] + blk[R_BK * 64 + 16 * nb + r];
    __syncthreads();
    load_tile<LD, HW>(L.W, blk + R_WV * 64, 0, 64);
    __syncthreads();
    linear(acc, L.X, L.W, wv, r, g);
    OWN_LOOP L.V[(16 * wv + 4 * g + rr) * LD + 16 * nb + r] = acc[nb][rr] + blk[R_BV * 64 + 16 * nb + r];
    __syncthreads();
    if (TRAIN) {
        img_store(save + 1 * 4096, L.Q);
        img_store(save + 2 * 4096, L.K);
        img_store(save + 3 * 4096, L.V);
    }
    f32x4 oacc[4];
    zero_acc(oacc);
    for (int h = 0; h < S.heads; ++h) {
        const int c0 = h * S.dh, c1 = c0 + S.dh;
        if (act) {
            float p[4][4];
            zero_acc(acc);
            mm<false, true>(acc, L.Q, L.K, wv, r, g, c0, c1);
            softmax_own(acc, p, s_live, S.inv_sqrt_dh, wv, r, g);
            OWN_LOOP {
                const int t = 16 * wv + 4 * g + rr, j = 16 * nb + r;
                float v = p[nb][rr];
                if (TRAIN && v != 0.0f) v = keep(kbase + (h * T + t) * T + j) ? v * S.scale : 0.0f;
                L.P[t * LD + j] = v;
            }
        }
        __syncthreads();
        if (act) {
            zero_acc(acc);
            mm<false, false>(acc, L.P, L.V, wv, r, g);
            OWN_LOOP {
                const int c = 16 * nb + r;
                if (c >= c0 && c < c1) oacc[nb][rr] = acc[nb][rr];
            }
        }
        __syncthreads();
    }
    OWN_LOOP {
        const int row = 16 * wv + 4 * g + rr, c = 16 * nb + r;
        L.T[row * LD + c] = s_live[row] ? oacc[nb][rr] + L.N[row * LD + c] : 0.0f;
    }
    __syncthreads();
    if (TRAIN) img_store(save + 4 * 4096, L.T);
    {
        float o[4][4], xh[4][4], rs[4];
        ln_rows(L.T, blk + R_G2 * 64, blk + R_B2 * 64, d, wv, r, g, o, xh, rs);
        OWN_LOOP {
            const int row = 16 * wv + 4 * g + rr;
            L.N[row * LD + 16 * nb + r] = s_live[row] ? o[nb][rr] : 0.0f;
        }
    }
    load_tile<LD, HW>(L.W, blk + R_W1 * 64, 0, 64);
    __syncthreads();
    if (act) {
        linear(acc, L.N, L.W, wv, r, g);
        OWN_LOOP {
            const int row = 16 * wv + 4 * g + rr, c = 16 * nb + r;
            float h1 = fmaxf(acc[nb][rr] + blk[R_C1 * 64 + c], 0.0f);
            if (TRAIN) {
                save[5 * 4096 + row * 64 + c] = h1;
                if (s_live[row] && c < d && h1 != 0.0f) h1 = keep(kbase + S.heads * T * T + row * d + c) ? h1 * S.scale : 0.0f;
            }
            L.Q[row * LD + c] = h1;
        }
    }
    __syncthreads();
    load_tile<LD, HW>(L.W, blk + R_W2 * 64, 0, 64);
    __syncthreads();
    if (act) {
        linear(acc, L.Q, L.W, wv, r, g);
        OWN_LOOP {
            const int row = 16 * wv + 4 * g + rr, c = 16 * nb + r;
            float v = 0.0f;
            if (s_live[row] && c < d) {
                v = acc[nb][rr] + blk[R_C2 * 64 + c];
                if (TRAIN) v = keep(kbase + S.heads * T * T + T * d + row * d + c) ? v * S.scale : 0.0f;
                v += L.N[row * LD + c];
            }
            L.X[row * LD + c] = v;
        }
    }
    __syncthreads();
}

// one block, backward: L.X (d of the block's output, zero on rows that are not live) -> L.X (d of its input); the parameters'
// gradients are added to gblk, the block's part of the workgroup's slab
__device__ __forceinline__ void block_backward(const Shape& S, const Lds& L, const float* __restrict__ blk, float* __restrict__ gblk,
                                               const float* __restrict__ save, const int* __restrict__ s_live, const Keep& keep, int kbase) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r = lane & 15, g = lane >> 4;
    const int d = S.d, T = S.T;
    f32x4 acc[4];
    // ---- feed-forward part: x' = mask (dropout(dropout(relu(f W1 + c1)) W2 + c2) + f), f = LN2(y)
    img_load(L.T, save + 4 * 4096);
    img_load(L.Q, save + 5 * 4096);
    __syncthreads();
    float xh2[4][4], rs2[4], m1[4][4];
    {
        float f[4][4];
        ln_rows(L.T, blk + R_G2 * 64, blk + R_B2 * 64, d, wv, r, g, f, xh2, rs2);
        OWN_LOOP {
            const int row = 16 * wv + 4 * g + rr, c = 16 * nb + r, at = row * LD + c;
            const bool in = s_live[row] && c < d;
            L.N[at] = in ? f[nb][rr] : 0.0f;
            L.P[at] = xh2[nb][rr];
            const float gx = L.X[at];
            float k2 = 0.0f, k1 = 0.0f;
            if (in) {
                k2 = keep(kbase + S.heads * T * T + T * d + row * d + c) ? S.scale : 0.0f;
                const float h1 = L.Q[at];
                if (h1 != 0.0f) k1 = keep(kbase + S.heads * T * T + row * d + c) ? S.scale : 0.0f;
            }
            m1[nb][rr] = k1;
            L.K[at] = gx * k2;                       // d(h W2 + c2)
            L.V[at] = L.Q[at] * k1;                  // dropout(relu(..))
        }
    }
    load_tile<LD, HW>(L.W, blk + R_W2 * 64, 0, 64);
    __syncthreads();
    zero_acc(acc);
    mm<true, false>(acc, L.K, L.V, wv, r, g);
    slab_add(gblk + R_W2 * 64, acc, d, wv, r, g);
    col_add(gblk + R_C2 * 64, L.K, nullptr, T, d);
    zero_acc(acc);
    mm<false, false>(acc, L.K, L.W, wv, r, g);
    __syncthreads();
    OWN_LOOP L.V[(16 * wv + 4 * g + rr) * LD + 16 * nb + r] = acc[nb][rr] * m1[nb][rr];     // through dropout and relu (m1 = 0 where h = 0)
    load_tile<LD, HW>(L.W, blk + R_W1 * 64, 0, 64);
    __syncthreads();
    zero_acc(acc);
    mm<true, false>(acc, L.V, L.N, wv, r, g);
    slab_add(gblk + R_W1 * 64, acc, d, wv, r, g);
    col_add(gblk + R_C1 * 64, L.V, nullptr, T, d);
    zero_acc(acc);
    mm<false, false>(acc, L.V, L.W, wv, r, g);
    {
        float df[4][4], dy[4][4];
        OWN_LOOP {
            const int at = (16 * wv + 4 * g + rr) * LD + 16 * nb + r;
            df[nb][rr] = acc[nb][rr] + L.X[at];
            L.K[at] = df[nb][rr];
        }
        ln_bwd(df, xh2, rs2, blk + R_G2 * 64, d, r, dy);
        OWN_LOOP {
            const int row = 16 * wv + 4 * g + rr;
            L.X[row * LD + 16 * nb + r] = s_live[row] ? dy[nb][rr] : 0.0f;     // d y = d(attention) = d(LN1(x))
        }
    }
    __syncthreads();
    col_add(gblk + R_G2 * 64, L.K, L.P, T, d);
    col_add(gblk + R_B2 * 64, L.K, nullptr, T, d);
    __syncthreads();
    // ---- attention part
    img_load(L.Q, save + 1 * 4096);
    img_load(L.K, save + 2 * 4096);
    img_load(L.V, save + 3 * 4096);
    __syncthreads();
    f32x4 dq[4], dk[4], dv[4];
    zero_acc(dq);
    zero_acc(dk);
    zero_acc(dv);
    for (int h = 0; h < S.heads; ++h) {
        const int c0 = h * S.dh, c1 = c0 + S.dh;
        float p[4][4], ds[4][4];
        zero_acc(acc);
        mm<false, true>(acc, L.Q, L.K, wv, r, g, c0, c1);
        softmax_own(acc, p, s_live, S.inv_sqrt_dh, wv, r, g);
        zero_acc(acc);
        mm<false, true>(acc, L.X, L.V, wv, r, g, c0, c1);          // d(dropped weights)[t][j] = <dO[t], V[j]> over the head
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int t = 16 * wv + 4 * g + rr;
            float dp[4], dot = 0.0f;
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) {
                const int j = 16 * nb + r;
                float kf = 0.0f;
                if (p[nb][rr] != 0.0f) kf = keep(kbase + (h * T + t) * T + j) ? S.scale : 0.0f;
                L.P[t * LD + j] = p[nb][rr] * kf;
                dp[nb] = acc[nb][rr] * kf;
                dot += dp[nb] * p[nb][rr];
            }
            dot = sum16(dot);
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) ds[nb][rr] = p[nb][rr] * (dp[nb] - dot) * S.inv_sqrt_dh;
        }
        __syncthreads();
        zero_acc(acc);
        mm<true, false>(acc, L.P, L.X, wv, r, g);                  // dV[j] = sum_t P[t][j] dO[t]
        OWN_LOOP {
            const int c = 16 * nb + r;
            if (c >= c0 && c < c1) dv[nb][rr] = acc[nb][rr];
        }
        __syncthreads();
        OWN_LOOP L.P[(16 * wv + 4 * g + rr) * LD + 16 * nb + r] = ds[nb][rr];
        __syncthreads();
        zero_acc(acc);
        mm<false, false>(acc, L.P, L.K, wv, r, g);                 // dQ[t] = sum_j dS[t][j] K[j]
        OWN_LOOP {
            const int c = 16 * nb + r;
            if (c >= c0 && c < c1) dq[nb][rr] = acc[nb][rr];
        }
        zero_acc(acc);
        mm<true, false>(acc, L.P, L.Q, wv, r, g);                  // dK[j] = sum_t dS[t][j] Q[t]
        OWN_LOOP {
            const int c = 16 * nb + r;
            if (c >= c0 && c < c1) dk[nb][rr] = acc[nb][rr];
        }
        __syncthreads();
    }
    OWN_LOOP {
        const int at = (16 * wv + 4 * g + rr) * LD + 16 * nb + r;
        L.T[at] = dq[nb][rr];
        L.P[at] = dk[nb][rr];
        L.N[at] = dv[nb][rr];
    }
    img_load(L.Q, save);                                           // the block's input x (Q, K, V were last read before the barrier above)
    __syncthreads();
    float xh1[4][4], rs1[4];
    {
        float qn[4][4];
        ln_rows(L.Q, blk + R_G1 * 64, blk + R_B1 * 64, d, wv, r, g, qn, xh1, rs1);
        OWN_LOOP {
            const int row = 16 * wv + 4 * g + rr, at = row * LD + 16 * nb + r;
            L.K[at] = s_live[row] ? qn[nb][rr] : 0.0f;
            L.V[at] = xh1[nb][rr];
        }
    }
    load_tile<LD, HW>(L.W, blk + R_WQ * 64, 0, 64);
    __syncthreads();
    zero_acc(acc);
    mm<true, false>(acc, L.T, L.K, wv, r, g);
    slab_add(gblk + R_WQ * 64, acc, d, wv, r, g);
    col_add(gblk + R_BQ * 64, L.T, nullptr, T, d);
    zero_acc(acc);
    mm<true, false>(acc, L.P, L.Q, wv, r, g);
    slab_add(gblk + R_WK * 64, acc, d, wv, r, g);
    col_add(gblk + R_BK * 64, L.P, nullptr, T, d);
    zero_acc(acc);
    mm<true, false>(acc, L.N, L.Q, wv, r, g);
    slab_add(gblk + R_WV * 64, acc, d, wv, r, g);
    col_add(gblk + R_BV * 64, L.N, nullptr, T, d);
    zero_acc(acc);
    mm<false, false>(acc, L.T, L.W, wv, r, g);                     // dQ Wq^T
    float dqn[4][4];
    OWN_LOOP dqn[nb][rr] = acc[nb][rr] + L.X[(16 * wv + 4 * g + rr) * LD + 16 * nb + r];      // + the residual's share
    __syncthreads();
    OWN_LOOP L.T[(16 * wv + 4 * g + rr) * LD + 16 * nb + r] = dqn[nb][rr];
    load_tile<LD, HW>(L.W, blk + R_WK * 64, 0, 64);
    __syncthreads();
    zero_acc(acc);
    mm<false, false>(acc, L.P, L.W, wv, r, g);                     // dK Wk^T
    __syncthreads();
    load_tile<LD, HW>(L.W, blk + R_WV * 64, 0, 64);
    __syncthreads();
    mm<false, false>(acc, L.N, L.W, wv, r, g);                     // + dV Wv^T
    {
        float dx[4][4];
        ln_bwd(dqn, xh1, rs1, blk + R_G1 * 64, d, r, dx);
        OWN_LOOP {
            const int row = 16 * wv + 4 * g + rr;
            L.X[row * LD + 16 * nb + r] = s_live[row] ? acc[nb][rr] + dx[nb][rr] : 0.0f;
        }
    }
    col_add(gblk + R_G1 * 64, L.T, L.V, T, d);
    col_add(gblk + R_B1 * 64, L.T, nullptr, T, d);
    __syncthreads();
}

__device__ __forceinline__ Lds carve(float* lds) {
    Lds L;
    L.X = lds; L.N = lds + IMG; L.W = lds + 2 * IMG; L.Q = lds + 3 * IMG;
    L.K = lds + 4 * IMG; L.V = lds + 5 * IMG; L.P = lds + 6 * IMG; L.T = lds + 7 * IMG;
    return L;
}

__global__ __launch_bounds__(NT) void sas_step_kernel(Shape S, const float* __restrict__ E, const float* __restrict__ P,
                                                      const float* __restrict__ shared, const int32_t* __restrict__ seq,
                                                      const int32_t* __restrict__ pos, const int32_t* __restrict__ neg,
                                                      const uint8_t* __restrict__ keep_in, uint8_t* __restrict__ keep_out, uint64_t seed,
                                                      uint64_t step, float* __restrict__ slabs, float* __restrict__ saves,
                                                      float* __restrict__ DE, float* __restrict__ LOSSB) {
    __shared__ __attribute__((aligned(16))) float lds[8 * IMG];
    __shared__ int s_seq[64], s_pos[64], s_neg[64], s_live[64];
    __shared__ int s_cnt[HW], s_flag[2];
    __shared__ float s_red[HW];
    const Lds L = carve(lds);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r = lane & 15, g = lane >> 4;
    const int n = S.n, I = S.I, d = S.d, T = S.T;
    const int64_t nT = static_cast<int64_t>(n) * T;
    float* __restrict__ slab = slabs + static_cast<int64_t>(blockIdx.x) * S.shared_floats;
    float* __restrict__ save = saves + static_cast<int64_t>(blockIdx.x) * S.blocks * SAVED * 4096;
    for (int i = tid; i < S.shared_floats; i += NT) slab[i] = 0.0f;
    {   // the batch's targets
        int c = 0;
        for (int64_t i = tid; i < nT; i += NT) c += pos[i] != I ? 1 : 0;
        c = wave_sum(c);
        if (lane == 0) s_cnt[wv] = c;
    }
    __syncthreads();
    const int count = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    const float invc = count > 0 ? 1.0f / static_cast<float>(count) : 0.0f;
    for (int64_t b = blockIdx.x; b < n; b += gridDim.x) {
        __syncthreads();
        if (tid < 2) s_flag[tid] = 0;
        __syncthreads();
        if (tid < 64) {
            const int t = tid;
            int sq = I, ps = I, ng = I;
            if (t < T) {
                sq = seq[b * T + t];
                ps = pos[b * T + t];
                ng = neg[b * T + t];
                if (sq < 0 || sq > I || ps < 0 || ps > I || ng < 0 || ng > I) s_flag[0] = 1;     // an id out of range: the sequence is skipped
                if (ps != I) s_flag[1] = 1;
            }
            s_seq[t] = sq; s_pos[t] = ps; s_neg[t] = ng;
            s_live[t] = (t < T && sq != I) ? 1 : 0;
        }
        __syncthreads();
        const Keep keep{keep_in, S.rate, seed, step, b, S.KS};
        if (keep_out)
            for (int e = tid; e < S.KS; e += NT) keep_out[b * S.KS + e] = keep(e) ? 1 : 0;
        if (s_flag[0] || !s_flag[1]) {                   // nothing to learn from: zero rows, zero loss
            for (int idx = tid; idx < 3 * T * 64; idx += NT) {
                const int part = idx / (T * 64), rest = idx % (T * 64);
                DE[(part * nT + b * T) * 64 + rest] = 0.0f;
            }
            if (tid == 0) LOSSB[b] = 0.0f;
            continue;
        }
        // ---- forward
        input_rows(S, L.X, E, P, s_seq, s_live, &keep);
        __syncthreads();
        for (int k = 0; k < S.blocks; ++k)
            block_forward<true>(S, L, shared + static_cast<int64_t>(k) * R_BLOCK * 64, save + static_cast<int64_t>(k) * SAVED * 4096, s_live,
                                keep, T * d + k * (S.heads * T * T + 2 * T * d), -1);
        const float* __restrict__ lno = shared + static_cast<int64_t>(S.blocks) * R_BLOCK * 64;
        float xho[4][4], rso[4];
        {
            float o[4][4];
            ln_rows(L.X, lno, lno + 64, d, wv, r, g, o, xho, rso);          // a row of zeros (padding) gives beta
            OWN_LOOP {
                const int at = (16 * wv + 4 * g + rr) * LD + 16 * nb + r;
                L.N[at] = o[nb][rr];
                L.T[at] = xho[nb][rr];
            }
        }
        __syncthreads();
        // ---- the two log losses of every target; d out -> L.Q; the target rows' gradients (without the sqrt(d))
        {
            float lsum = 0.0f;
            for (int t = wv; t < 64; t += HW) {
                const bool target = t < T && s_pos[t] != I;
                const float o = L.N[t * LD + lane];
                float dout = 0.0f, gp = 0.0f, gn = 0.0f;
                if (target) {
                    const int ip = s_pos[t], in_ = s_neg[t];
                    const float ep = E[static_cast<int64_t>(ip) * D + lane];
                    const float en = in_ != I ? E[static_cast<int64_t>(in_) * D + lane] : 0.0f;
                    const float yp = S.sqrt_d * wave_sum(o * ep), yn = S.sqrt_d * wave_sum(o * en);
                    float dp_, dn_;
                    lsum += neg_log_sigmoid(yp, dp_);
                    lsum += neg_log_sigmoid(-yn, dn_);
                    const float dyp = dp_ * invc, dyn = -dn_ * invc;
                    dout = S.sqrt_d * (dyp * ep + dyn * en);
                    gp = dyp * o;
                    gn = dyn * o;
                }
                L.Q[t * LD + lane] = dout;
                if (t < T) {
                    DE[(nT + b * T + t) * 64 + lane] = gp;
                    DE[(2 * nT + b * T + t) * 64 + lane] = gn;
                }
            }
            if (lane == 0) s_red[wv] = lsum;
        }
        __syncthreads();
        if (tid == 0) LOSSB[b] = ((s_red[0] + s_red[1]) + s_red[2]) + s_red[3];
        // ---- backward
        float* __restrict__ glno = slab + static_cast<int64_t>(S.blocks) * R_BLOCK * 64;
        {
            float dy[4][4], dx[4][4];
            OWN_LOOP dy[nb][rr] = L.Q[(16 * wv + 4 * g + rr) * LD + 16 * nb + r];
            ln_bwd(dy, xho, rso, lno, d, r, dx);
            OWN_LOOP {
                const int row = 16 * wv + 4 * g + rr;
                L.X[row * LD + 16 * nb + r] = s_live[row] ? dx[nb][rr] : 0.0f;
            }
        }
        col_add(glno, L.Q, L.T, T, d);
        col_add(glno + 64, L.Q, nullptr, T, d);
        __syncthreads();
        for (int k = S.blocks - 1; k >= 0; --k)
            block_backward(S, L, shared + static_cast<int64_t>(k) * R_BLOCK * 64, slab + static_cast<int64_t>(k) * R_BLOCK * 64,
                           save + static_cast<int64_t>(k) * SAVED * 4096, s_live, keep, T * d + k * (S.heads * T * T + 2 * T * d));
        // ---- through the input's dropout: the rows of seq (without the sqrt(d)), which are the position rows' too
        for (int idx = tid; idx < T * 64; idx += NT) {
            const int t = idx >> 6, c = idx & 63;
            float v = 0.0f;
            if (s_live[t] && c < d) v = keep(t * d + c) ? L.X[t * LD + c] * S.scale : 0.0f;
            DE[(b * T + t) * 64 + c] = v;
        }
    }
}

// gshared += the workgroups' slabs in workgroup order
__global__ __launch_bounds__(256) void sas_reduce_kernel(const float* __restrict__ slabs, int n_wg, int len, float* __restrict__ gshared) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= len) return;
    float t = 0.0f;
    for (int w = 0; w < n_wg; ++w) t += slabs[static_cast<int64_t>(w) * len + e];
    gshared[e] += t;
}

// gP[t][c] += the sequences' input-gradient rows in batch order
__global__ __launch_bounds__(256) void sas_position_kernel(const float* __restrict__ DE, int n, int T, float* __restrict__ gP) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= T * 64) return;
    float t = 0.0f;
    for (int64_t b = 0; b < n; ++b) t += DE[b * T * 64 + e];
    gP[e] += t;
}

__device__ __forceinline__ int id_at(const int32_t* __restrict__ seq, const int32_t* __restrict__ pos, const int32_t* __restrict__ neg, int nT,
                                     int o) {
    return o < nT ? seq[o] : (o < 2 * nT ? pos[o - nT] : neg[o - 2 * nT]);
}

// order [3 n T]: the positions of seq || pos || neg sorted by (id, position) -- a rank by counting, the list walked through
// LDS RC ids at a time (caser.hip's cs_rank_kernel for one list)
constexpr int RC = 2048;

__global__ __launch_bounds__(256) void sas_rank_kernel(const int32_t* __restrict__ seq, const int32_t* __restrict__ pos,
                                                       const int32_t* __restrict__ neg, int nT, int32_t* __restrict__ order) {
    __shared__ __attribute__((aligned(16))) int32_t s_ids[RC];
    const int len = 3 * nT;
    const int kk = blockIdx.x * 256 + threadIdx.x;
    const bool live = kk < len;
    const int id = live ? id_at(seq, pos, neg, nT, kk) : 0;
    int rank = 0;
    for (int c0 = 0; c0 < len; c0 += RC) {
        __syncthreads();
        // ids beyond the list: INT_MAX, which is below no id and equal to none that is ranked before its own position
        for (int j = threadIdx.x; j < RC; j += 256) s_ids[j] = c0 + j < len ? id_at(seq, pos, neg, nT, c0 + j) : 0x7fffffff;
        __syncthreads();
        const int lim = len - c0 < RC ? len - c0 : RC;
        const int before = kk - c0;
        for (int j = 0; j < lim; j += 4) {
            const int4 o = *reinterpret_cast<const int4*>(s_ids + j);
            rank += (o.x < id || (o.x == id && j < before)) ? 1 : 0;
            rank += (o.y < id || (o.y == id && j + 1 < before)) ? 1 : 0;
            rank += (o.z < id || (o.z == id && j + 2 < before)) ? 1 : 0;
            rank += (o.w < id || (o.w == id && j + 3 < before)) ? 1 : 0;
        }
    }
    if (live) order[rank] = kk;
}

// a wavefront per rank: the wavefront of an id's first rank adds that id's rows in rank order (ascending list position) and adds
// sqrt(d) times the sum to the item rows' gradient -- one writer per distinct id; the padding row I and ids out of range: nothing
__global__ __launch_bounds__(NT) void sas_seg_add_kernel(const int32_t* __restrict__ seq, const int32_t* __restrict__ pos,
                                                         const int32_t* __restrict__ neg, const int32_t* __restrict__ order, int nT, int I,
                                                         float sqrt_d, const float* __restrict__ DE, float* __restrict__ gE) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t w = static_cast<int64_t>(blockIdx.x) * HW + wv;
    const int len = 3 * nT;
    if (w >= len) return;
    const int rk = static_cast<int>(w);
    const int id = id_at(seq, pos, neg, nT, order[rk]);
    if (id < 0 || id >= I || (rk > 0 && id_at(seq, pos, neg, nT, order[rk - 1]) == id)) return;
    float acc = 0.0f;
    for (int k = rk; k < len; ++k) {
        const int o = order[k];
        if (id_at(seq, pos, neg, nT, o) != id) break;
        acc += DE[static_cast<int64_t>(o) * D + lane];
    }
    gE[static_cast<int64_t>(id) * D + lane] += sqrt_d * acc;
}

// loss[0] = the sequences' sums by a fixed tree over the number of targets; every other word = 0
__global__ __launch_bounds__(1024) void sas_loss_kernel(const float* __restrict__ LOSSB, const int32_t* __restrict__ pos, int n, int T, int I,
                                                        float* __restrict__ loss, int loss_slots) {
    __shared__ float s[1024];
    float a = 0.0f, c = 0.0f;
    for (int b = threadIdx.x; b < n; b += 1024) a += LOSSB[b];
    for (int64_t i = threadIdx.x; i < static_cast<int64_t>(n) * T; i += 1024) c += pos[i] != I ? 1.0f : 0.0f;     // exact below 2^24
    const float ta = block_sum_1024(a, s);
    const float tc = block_sum_1024(c, s);
    if (threadIdx.x == 0) loss[0] = tc > 0.0f ? ta / tc : 0.0f;
    for (int k = 1 + threadIdx.x; k < 2 * loss_slots; k += 1024) loss[k] = 0.0f;
}

// the query row of one user: the forward without dropout, the last block for the last position's 16-row tile alone
__global__ __launch_bounds__(NT) void sas_query_kernel(Shape S, const float* __restrict__ E, const float* __restrict__ P,
                                                       const float* __restrict__ shared, const int32_t* __restrict__ users,
                                                       const int32_t* __restrict__ windows, int n_users, float* __restrict__ Qout) {
    __shared__ __attribute__((aligned(16))) float lds[8 * IMG];
    __shared__ int s_seq[64], s_live[64];
    const Lds L = carve(lds);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r = lane & 15, g = lane >> 4;
    const int I = S.I, d = S.d, T = S.T;
    const int64_t i = blockIdx.x;
    const int u = users ? users[i] : static_cast<int>(i);
    if (u < 0 || u >= n_users) return;                   // (the whole workgroup)
    if (tid < 64) {
        int sq = I;
        if (tid < T) {
            sq = windows[static_cast<int64_t>(u) * T + tid];
            if (sq < 0 || sq > I) sq = I;                // an id out of range reads as padding
        }
        s_seq[tid] = sq;
        s_live[tid] = sq != I ? 1 : 0;
    }
    __syncthreads();
    input_rows(S, L.X, E, P, s_seq, s_live, nullptr);
    __syncthreads();
    const Keep keep{nullptr, 0.0f, 0, 0, 0, 0};
    const int last_wave = (T - 1) >> 4;
    for (int k = 0; k < S.blocks; ++k)
        block_forward<false>(S, L, shared + static_cast<int64_t>(k) * R_BLOCK * 64, nullptr, s_live, keep, 0,
                             k == S.blocks - 1 ? last_wave : -1);
    if (wv != last_wave) return;
    const float* __restrict__ lno = shared + static_cast<int64_t>(S.blocks) * R_BLOCK * 64;
    float o[4][4], xh[4][4], rs[4];
    ln_rows(L.X, lno, lno + 64, d, wv, r, g, o, xh, rs);
    OWN_LOOP {
        if (16 * wv + 4 * g + rr == T - 1) Qout[i * D + 16 * nb + r] = S.sqrt_d * o[nb][rr];
    }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
struct Work {     // offsets in bytes, every one a multiple of 16
    int64_t slabs, saves, de, lossb, order, total;
};

inline int64_t up16(int64_t x) { return (x + 15) & ~static_cast<int64_t>(15); }

inline Work work_layout(int64_t n, int T, int blocks) {
    Work w;
    int64_t o = 0;
    const int64_t f = sizeof(float), wg = n < G ? n : G;
    w.slabs = o; o += up16(wg * SKR_SASREC_SHARED_FLOATS(blocks) * f);
    w.saves = o; o += up16(wg * blocks * SAVED * 4096 * f);
    w.de = o; o += up16(3 * n * T * D * f);
    w.lossb = o; o += up16(n * f);
    w.order = o; o += up16(3 * n * T * 4);
    w.total = o;
    return w;
}

int check_shape(const char* who, int d, int T, int blocks, int heads) {
    SKR_REQUIRE(d >= 1 && d <= SKR_SASREC_MAX_HIDDEN, "%s: need 1 <= hidden_units <= %d (got %d)", who, SKR_SASREC_MAX_HIDDEN, d);
    SKR_REQUIRE(T >= 1 && T <= SKR_SASREC_MAX_LEN, "%s: need 1 <= max_len <= %d (got %d)", who, SKR_SASREC_MAX_LEN, T);
    SKR_REQUIRE(blocks >= 1 && blocks <= SKR_SASREC_MAX_BLOCKS, "%s: need 1 <= num_blocks <= %d (got %d)", who, SKR_SASREC_MAX_BLOCKS,
                blocks);
    SKR_REQUIRE(heads >= 1 && heads <= SKR_SASREC_MAX_HEADS && d % heads == 0,
                "%s: need 1 <= num_heads <= %d dividing hidden_units = %d (got %d)", who, SKR_SASREC_MAX_HEADS, d, heads);
    return SKR_OK;
}

int step_impl(const float* d_E, const float* d_P, const float* d_shared, const int32_t* d_seq, const int32_t* d_pos, const int32_t* d_neg,
              int n, int n_items, int hidden, int max_len, int blocks, int heads, float rate, const uint8_t* d_keep, uint8_t* d_keep_out,
              uint64_t seed, uint64_t step, float* d_gE, float* d_gP, float* d_gshared, void* d_work, size_t work_bytes, float* d_loss,
              int loss_slots, void* stream, float* h_ms) {
    const char* who = "skr_sasrec_step";
    SKR_REQUIRE(d_E && d_P && d_shared && d_seq && d_pos && d_neg && d_gE && d_gP && d_gshared && d_work && d_loss, "%s: NULL argument",
                who);
    SKR_REQUIRE(n >= 0 && n <= SKR_SASREC_MAX_BATCH, "%s: need 0 <= n <= %d (got %d)", who, SKR_SASREC_MAX_BATCH, n);
    SKR_REQUIRE(n_items > 0, "%s: n_items = %d", who, n_items);
    int rc = check_shape(who, hidden, max_len, blocks, heads);
    if (rc != SKR_OK) return rc;
    SKR_REQUIRE(rate >= 0.0f && rate < 1.0f, "%s: need 0 <= rate < 1 (got %g)", who, static_cast<double>(rate));
    SKR_REQUIRE(loss_slots == 1 || loss_slots == SKR_LOSS_SLOTS, "%s: loss_slots must be 1 or %d", who, SKR_LOSS_SLOTS);
    if (n == 0) return SKR_OK;
    const Shape S = make_shape(n, n_items, hidden, max_len, blocks, heads, rate);
    const Work W = work_layout(n, max_len, blocks);
    SKR_REQUIRE(work_bytes >= static_cast<size_t>(W.total), "%s: d_work holds %zu bytes, skr_sasrec_workspace asks for %lld", who, work_bytes,
                static_cast<long long>(W.total));
    SKR_REQUIRE(((reinterpret_cast<uintptr_t>(d_shared) | reinterpret_cast<uintptr_t>(d_E) | reinterpret_cast<uintptr_t>(d_P) |
                  reinterpret_cast<uintptr_t>(d_work)) & 15) == 0,
                "%s: d_E, d_P, d_shared and d_work must be 16-byte aligned", who);
    hipStream_t st = as_stream(stream);
    char* w = static_cast<char*>(d_work);
    float* slabs = reinterpret_cast<float*>(w + W.slabs);
    float* saves = reinterpret_cast<float*>(w + W.saves);
    float* DE = reinterpret_cast<float*>(w + W.de);
    float* LOSSB = reinterpret_cast<float*>(w + W.lossb);
    int32_t* order = reinterpret_cast<int32_t*>(w + W.order);
    const int wg = n < G ? n : G, nT = n * max_len, len = 3 * nT;
    StepTimer<SKR_SASREC_LAUNCHES + 1> mk(h_ms, st);
    SKR_HIP(mk.mark());
    hipLaunchKernelGGL(sas_step_kernel, dim3(wg), dim3(NT), 0, st, S, d_E, d_P, d_shared, d_seq, d_pos, d_neg, d_keep, d_keep_out, seed, step,
                       slabs, saves, DE, LOSSB);
    SKR_HIP(mk.mark());
    hipLaunchKernelGGL(sas_reduce_kernel, dim3((S.shared_floats + 255) / 256), dim3(256), 0, st, slabs, wg, S.shared_floats, d_gshared);
    SKR_HIP(mk.mark());
    hipLaunchKernelGGL(sas_position_kernel, dim3((max_len * 64 + 255) / 256), dim3(256), 0, st, DE, n, max_len, d_gP);
    SKR_HIP(mk.mark());
    hipLaunchKernelGGL(sas_rank_kernel, dim3((len + 255) / 256), dim3(256), 0, st, d_seq, d_pos, d_neg, nT, order);
    SKR_HIP(mk.mark());
    hipLaunchKernelGGL(sas_seg_add_kernel, dim3((len + HW - 1) / HW), dim3(NT), 0, st, d_seq, d_pos, d_neg, order, nT, n_items, S.sqrt_d, DE,
                       d_gE);
    SKR_HIP(mk.mark());
    hipLaunchKernelGGL(sas_loss_kernel, dim3(1), dim3(1024), 0, st, LOSSB, d_pos, n, max_len, n_items, d_loss, loss_slots);
    SKR_HIP(mk.mark());
    SKR_LAUNCH_CHECK();
    SKR_HIP(mk.finish());
    return SKR_OK;
}

}  // namespace

extern "C" {

int64_t skr_sasrec_workspace(int n_max, int max_len, int blocks, int heads) {
    if (n_max < 1 || n_max > SKR_SASREC_MAX_BATCH || max_len < 1 || max_len > SKR_SASREC_MAX_LEN || blocks < 1 ||
        blocks > SKR_SASREC_MAX_BLOCKS || heads < 1 || heads > SKR_SASREC_MAX_HEADS)
        return 0;
    return work_layout(n_max, max_len, blocks).total;
}

int skr_sasrec_step(const float* d_E, const float* d_P, const float* d_shared, const int32_t* d_seq, const int32_t* d_pos,
                    const int32_t* d_neg, int n, int n_items, int hidden, int max_len, int blocks, int heads, float rate,
                    const uint8_t* d_keep, uint8_t* d_keep_out, uint64_t seed, uint64_t step, float* d_gE, float* d_gP, float* d_gshared,
                    void* d_work, size_t work_bytes, float* d_loss, int loss_slots, void* stream) {
    return step_impl(d_E, d_P, d_shared, d_seq, d_pos, d_neg, n, n_items, hidden, max_len, blocks, heads, rate, d_keep, d_keep_out, seed,
                     step, d_gE, d_gP, d_gshared, d_work, work_bytes, d_loss, loss_slots, stream, nullptr);
}

int skr_sasrec_step_timed(const float* d_E, const float* d_P, const float* d_shared, const int32_t* d_seq, const int32_t* d_pos,
                          const int32_t* d_neg, int n, int n_items, int hidden, int max_len, int blocks, int heads, float rate,
                          const uint8_t* d_keep, uint8_t* d_keep_out, uint64_t seed, uint64_t step, float* d_gE, float* d_gP,
                          float* d_gshared, void* d_work, size_t work_bytes, float* d_loss, int loss_slots, void* stream, float* h_ms) {
    SKR_REQUIRE(h_ms != nullptr, "skr_sasrec_step_timed: NULL argument");
    return step_impl(d_E, d_P, d_shared, d_seq, d_pos, d_neg, n, n_items, hidden, max_len, blocks, heads, rate, d_keep, d_keep_out, seed,
                     step, d_gE, d_gP, d_gshared, d_work, work_bytes, d_loss, loss_slots, stream, h_ms);
}

int skr_sasrec_queries(const float* d_E, const float* d_P, const float* d_shared, const int32_t* d_users, int n, const int32_t* d_windows,
                       int n_users, int n_items, int hidden, int max_len, int blocks, int heads, float* d_Q, void* stream) {
    const char* who = "skr_sasrec_queries";
    SKR_REQUIRE(d_E && d_P && d_shared && d_windows && d_Q, "%s: NULL argument", who);
    SKR_REQUIRE(n >= 0 && n_users > 0 && n_items > 0, "%s: n = %d, n_users = %d, n_items = %d", who, n, n_users, n_items);
    SKR_REQUIRE(d_users || n <= n_users, "%s: without a user list n = %d must not exceed n_users = %d", who, n, n_users);
    const int rc = check_shape(who, hidden, max_len, blocks, heads);
    if (rc != SKR_OK) return rc;
    if (n == 0) return SKR_OK;
    SKR_REQUIRE(((reinterpret_cast<uintptr_t>(d_shared) | reinterpret_cast<uintptr_t>(d_E) | reinterpret_cast<uintptr_t>(d_P)) & 15) == 0,
                "%s: d_E, d_P and d_shared must be 16-byte aligned", who);
    const Shape S = make_shape(n, n_items, hidden, max_len, blocks, heads, 0.0f);
    hipLaunchKernelGGL(sas_query_kernel, dim3(n), dim3(NT), 0, as_stream(stream), S, d_E, d_P, d_shared, d_users, d_windows, n_users, d_Q);
    SKR_LAUNCH_CHECK();
    return SKR_OK;
}

}  // extern "C"
