// caser.hip -- Caser (convolutional sequence embedding): one training step, forward and backward, and the per-user query rows.
//
// Replaces the stock torch ops the reference issues per step and per evaluation batch (no native code there):
//   recommender/Caser.py:118-147   _forward_user: conv_v, the L conv_h with ReLU and max_pool1d, dropout, fc1 with ReLU, [z, p]
//   recommender/Caser.py:149-157   forward: baddbmm(b2, W2[t], x) for the 2T targets
//   recommender/Caser.py:196-207   the two sigmoid cross entropies, their mean, backward
//   recommender/Caser.py:159-162   predict: x in eval mode against every W2 row (here: the query rows; skr_score_matrix ranks)
//
// The launches of a step, in order (SKR_CASER_LAUNCHES groups, the events of skr_caser_step_timed):
//   conv      cs_conv_kernel: a workgroup owns IB = 8 instances.  Their L x 8 window rows lie in LDS (the (position, instance)
//             pairs: row 8 t + i); the horizontal filters are ONE product [pairs, 64] x [64, filter rows] on
//             v_mfma_f32_16x16x4_f32, the filter rows streamed through LDS 64 at a time (1 152 rows at L = 8, nh = 32 do
//             not fit).  A tile never cuts the h rows of one filter (h, k): it takes floor(64 / h) filters of one height, which
//             are consecutive rows of the block, so a[h,k,t] = bias + sum_r P[(t + r, i)][(k, r)] needs the tile's products
//             alone.  ReLU, max and the lowest arg-position are taken on those sums; the vertical filters (nv L FMAs per
//             output) run on the VALU from the same LDS rows.  Dropout is applied as the outputs are written.
//   fc1       cs_fc_kernel: [n, Fp] x [Fp, 64] on the same MFMA, W1 streamed through LDS in chunks of 64 columns.
//   score     cs_score_kernel: a wavefront per instance: the 2T scores, both cross entropies, dy, dz (through the ReLU), dp.
//   d_out     dense_rows_w: d_out = dz W1.                       dW1 | db1: dense_xty: dz^T out and dz's column sums (fixed order).
//   conv bwd  cs_conv_bwd_kernel: a wavefront per instance: d_out through the dropout, the ReLU and the arg-max; the
//             gradient rows of the window's L positions.
//   filters   cs_filter_grad_kernel: a workgroup per filter row (h, k, r), per vertical weight and per vertical bias: its four
//             wavefronts walk the instances w, w + 4, ... in order and are added in wavefront order -- a fixed order.
//   rank, ordered adds: the user list, the n L window entries and the 2 n T targets ranked by (id, position) by counting (the
//             list walked through LDS), then one wavefront per distinct id adds that id's rows in rank order and adds the sum
//             to the table's gradient once.
//   loss      one workgroup adds the instances' two cross entropies by a fixed tree.
// No floating-point atomic anywhere: two calls on the same inputs give the same bits.
#include "skr_common.h"
#include "dense_ops.h"
#include "fast_rng.h"
#include "mfma_tile.h"
#include "step_common.h"

#include <cmath>

namespace {

using namespace skr;

constexpr int D = 64;
constexpr int HW = 4;        // wavefronts per workgroup
constexpr int IB = 8;        // instances of a conv workgroup: 8 L <= 64 (position, instance) pairs
constexpr int LD = 68;       // LDS row stride of a 64-float row (16-byte aligned rows)
constexpr int SP = 65;       // LDS row stride of the products

// the shapes of one model and the offsets of its shared block (the header's layout)
struct Shape {
    int L, T, nv, nh, width;
    int F, Fp, Fref, rows, HK;
    int o_wv, o_bv, o_wh, o_bh, o_w1, o_b1, total;
};

inline Shape make_shape(int L, int T, int nv, int nh, int width) {
    Shape s;
    s.L = L; s.T = T; s.nv = nv; s.nh = nh; s.width = width;
    s.HK = nh * L;
    s.F = nv * D + s.HK;
    s.Fp = SKR_CASER_FP(L, nv, nh);
    s.Fref = nv * width + s.HK;
    s.rows = SKR_CASER_ROWS(L, nh);
    s.o_wv = 0;
    s.o_bv = D;
    s.o_wh = 2 * D;
    s.o_bh = s.o_wh + D * s.rows;
    s.o_w1 = s.o_bh + D * ((s.HK + D - 1) / D);
    s.o_b1 = s.o_w1 + D * s.Fp;
    s.total = s.o_b1 + D;
    return s;
}

__host__ __device__ inline int filter_base(int nh, int h) { return nh * h * (h - 1) / 2; }   // the first row of height h

// ------------------------------------------------------------------------------------------------
// conv: out = dropout([out_v, out_h]) of IB instances
// ------------------------------------------------------------------------------------------------
template <bool TRAIN>
__global__ __launch_bounds__(HW * 64) void cs_conv_kernel(
    Shape S, const float* __restrict__ E, const float* __restrict__ shared, const int32_t* __restrict__ users, int u_base,
    const int32_t* __restrict__ seqs, const int32_t* __restrict__ pos, const int32_t* __restrict__ neg, int n, int n_users, int n_rows,
    int pad, float rate, float scale, const uint8_t* __restrict__ keep_in, uint8_t* __restrict__ keep_out, uint64_t seed, uint64_t step,
    float* __restrict__ OUT, uint8_t* __restrict__ MASK, int8_t* __restrict__ ARG, int32_t* __restrict__ VALID) {
    __shared__ __attribute__((aligned(16))) float sE[64 * LD];
    __shared__ __attribute__((aligned(16))) float sB[64 * LD];
    __shared__ float sP[64 * SP];
    __shared__ int s_ok[IB], s_user[IB];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r = lane & 15, g = lane >> 4;
    const int b0 = blockIdx.x * IB;
    const int L = S.L, T = S.T, nh = S.nh;
    // 1 = a live instance, 0 = an id of its window or targets is out of range, -1 = its user is (or b >= n)
    if (tid < IB) {
        const int b = b0 + tid;
        int ok = -1, u = -1;
        if (b < n) {
            u = users ? users[b] : u_base + b;
            ok = (u >= 0 && u < n_users) ? 1 : -1;
        }
        s_ok[tid] = ok;
        s_user[tid] = u;
    }
    __syncthreads();
    {
        const int i = tid & (IB - 1), j = tid >> 3, b = b0 + i;     // j < 32: a window position and a target
        bool bad = false;
        if (b < n) {
            if (j < L) {
                const int s = seqs[static_cast<int64_t>(b) * L + j];
                bad = s < 0 || s >= n_rows;
            }
            if (TRAIN && j < 2 * T) {
                const int t = j < T ? pos[static_cast<int64_t>(b) * T + j] : neg[static_cast<int64_t>(b) * T + j - T];
                bad = bad || t < 0 || t >= n_rows;
            }
        }
        if (bad && s_ok[i] == 1) s_ok[i] = 0;
    }
    __syncthreads();
    if (tid < IB && b0 + tid < n) VALID[b0 + tid] = s_ok[tid];
    // the window rows: LDS row 8 t + i = E[s_t of instance i], zeros for the padding item, a skipped instance and t >= L
    {
        const float4* E4 = reinterpret_cast<const float4*>(E);
        float4 v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int idx = tid + q * HW * 64, row = idx >> 4, c4 = idx & 15, t = row >> 3, i = row & (IB - 1), b = b0 + i;
            int64_t s = -1;
            if (t < L && b < n && s_ok[i] == 1) {
                s = seqs[static_cast<int64_t>(b) * L + t];
                if (s == pad) s = -1;
            }
            v[q] = s >= 0 ? E4[s * 16 + c4] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int idx = tid + q * HW * 64, row = idx >> 4, c4 = idx & 15;
            *reinterpret_cast<float4*>(sE + row * LD + 4 * c4) = v[q];
        }
    }
    __syncthreads();
    // column j of instance b0 + i (jr: its column in the reference's order, -1 for a zero-padded one) through the dropout
    auto emit = [&](int i, int j, int jr, float v) {
        const int64_t b = b0 + i;
        bool keep = jr >= 0 && s_ok[i] == 1;
        if (TRAIN && keep && rate > 0.0f)
            keep = keep_in ? keep_in[b * S.Fref + jr] != 0 : keep_draw(seed, step, s_user[i], jr, 1.0f - rate);
        OUT[b * S.Fp + j] = keep ? v * scale : 0.0f;
        if (TRAIN) {
            MASK[b * S.Fp + j] = keep ? 1 : 0;
            if (keep_out && jr >= 0) keep_out[b * S.Fref + jr] = keep ? 1 : 0;
        }
    };
    // vertical filters: out_v[c][col] = bv[c] + sum_l wv[c][l] E_l[col]; the columns beyond `width` stay zero
    {
        const float* __restrict__ wvp = shared + S.o_wv;
        const float* __restrict__ bvp = shared + S.o_bv;
        for (int idx = tid; idx < IB * S.nv * D; idx += HW * 64) {
            const int col = idx & 63, c = (idx >> 6) % S.nv, i = (idx >> 6) / S.nv;
            if (b0 + i >= n) continue;
            float v = 0.0f;
            const bool real = col < S.width;
            if (real && s_ok[i] == 1) {
                v = bvp[c];
                for (int l = 0; l < L; ++l) v = fmaf(wvp[c * L + l], sE[(l * IB + i) * LD + col], v);
            }
            emit(i, c * D + col, real ? c * S.width + col : -1, v);
        }
        const int tail = S.Fp - S.F;
        for (int idx = tid; idx < IB * tail; idx += HW * 64) {
            const int i = idx / tail;
            if (b0 + i < n) emit(i, S.F + idx % tail, -1, 0.0f);
        }
    }
    // horizontal filters, a tile of floor(64 / h) filters of height h at a time
    const float* __restrict__ WH = shared + S.o_wh;
    const float* __restrict__ bhp = shared + S.o_bh;
    const int pair_tiles = (IB * L + 15) / 16;
    for (int h = 1; h <= L; ++h) {
        const int per = 64 / h, base = filter_base(nh, h);
        for (int k0 = 0; k0 < nh; k0 += per) {
            const int k1 = k0 + per < nh ? k0 + per : nh;
            __syncthreads();
            load_tile<LD, HW>(sB, WH, base + k0 * h, base + k1 * h);
            __syncthreads();
            if (wv < pair_tiles) {
                float a[16];
                f32x4 acc[4];
                load_slab<LD>(a, sE, 16 * wv + r, g);
                zero_acc(acc);
                tile_product<LD, 16>(acc, a, sB, r, g);
#pragma unroll
                for (int nb = 0; nb < 4; ++nb) {
#pragma unroll
                    for (int rr = 0; rr < 4; ++rr) sP[(16 * wv + 4 * g + rr) * SP + 16 * nb + r] = acc[nb][rr];
                }
            }
            __syncthreads();
            for (int item = tid; item < IB * (k1 - k0); item += HW * 64) {
                const int i = item & (IB - 1), kk = item >> 3, k = k0 + kk;
                if (b0 + i >= n) continue;
                const float bias = bhp[(h - 1) * nh + k];
                float best = 0.0f;
                int arg = 0;
                for (int t = 0; t + h <= L; ++t) {
                    float s = bias;
                    for (int q = 0; q < h; ++q) s += sP[((t + q) * IB + i) * SP + kk * h + q];
                    if (t == 0 || s > best) { best = s; arg = t; }     // the lowest position among ties, as max_pool1d
                }
                const bool alive = best > 0.0f;                        // relu'(0) = 0
                const int hk = (h - 1) * nh + k;
                emit(i, S.nv * D + hk, S.nv * S.width + hk, alive ? best : 0.0f);
                if (TRAIN) ARG[static_cast<int64_t>(b0 + i) * S.HK + hk] = static_cast<int8_t>(alive && s_ok[i] == 1 ? arg : -1);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// fc1: z = relu(out W1^T + b1); a wavefront owns 16 instances
// ------------------------------------------------------------------------------------------------
template <bool TRAIN>
__global__ __launch_bounds__(HW * 64) void cs_fc_kernel(Shape S, const float* __restrict__ shared, const float* __restrict__ OUT, int n,
                                                        const int32_t* __restrict__ VALID, const int32_t* __restrict__ users, int u_base,
                                                        const float* __restrict__ U, float* __restrict__ X) {
    __shared__ __attribute__((aligned(16))) float sB[64 * LD];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r = lane & 15, g = lane >> 4;
    const int b0 = (blockIdx.x * HW + wv) * 16;
    const int fp4 = S.Fp / 4;
    const float4* W4 = reinterpret_cast<const float4*>(shared + S.o_w1);
    f32x4 acc[4];
    zero_acc(acc);
    for (int c = 0; c < S.Fp / 64; ++c) {
        float4 v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int idx = tid + q * HW * 64, row = idx >> 4, c4 = idx & 15;
            v[q] = W4[static_cast<int64_t>(row) * fp4 + c * 16 + c4];
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int idx = tid + q * HW * 64, row = idx >> 4, c4 = idx & 15;
            *reinterpret_cast<float4*>(sB + row * LD + 4 * c4) = v[q];
        }
        __syncthreads();
        float a[16];
        const bool in = b0 + r < n;            // rows beyond the batch: a row inside it, times zero
        const float4* p = reinterpret_cast<const float4*>(OUT + static_cast<int64_t>(in ? b0 + r : 0) * S.Fp + c * 64 + 16 * g);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 w = p[q];
            a[4 * q + 0] = in ? w.x : 0.0f; a[4 * q + 1] = in ? w.y : 0.0f; a[4 * q + 2] = in ? w.z : 0.0f; a[4 * q + 3] = in ? w.w : 0.0f;
        }
        tile_product<LD, 16>(acc, a, sB, r, g);
    }
    const float* __restrict__ b1 = shared + S.o_b1;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        const int row = b0 + 4 * g + rr;
        if (row >= n) continue;
        int ok = 1;
        int64_t u = 0;
        if (!TRAIN) {
            ok = VALID[row];
            if (ok < 0) continue;                       // a user out of range: no row to write
            u = users ? users[row] : u_base + row;
        }
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) {
            const int j = 16 * nb + r;
            const float zp = acc[nb][rr] + b1[j];
            const float z = zp > 0.0f ? zp : 0.0f;
            if (TRAIN) {
                X[static_cast<int64_t>(row) * 128 + j] = z;
            } else {                                    // the query row [z, p], NaN for a user without history
                const float nan = __builtin_nanf("");
                X[u * 128 + j] = ok ? z : nan;
                X[u * 128 + 64 + j] = ok ? U[u * D + j] : nan;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// scores, loss and what flows back into x = [z, p]: a wavefront per instance
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(HW * 64) void cs_score_kernel(Shape S, const float* __restrict__ U, const float* __restrict__ W2,
                                                           const float* __restrict__ b2, const int32_t* __restrict__ users,
                                                           const int32_t* __restrict__ pos, const int32_t* __restrict__ neg,
                                                           const int32_t* __restrict__ VALID, int n, float inv, float* __restrict__ X,
                                                           float* __restrict__ DY, float* __restrict__ DZ, float* __restrict__ DP,
                                                           float* __restrict__ LOSSB) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t b = static_cast<int64_t>(blockIdx.x) * HW + wv;
    if (b >= n) return;
    const int T = S.T;
    if (VALID[b] != 1) {                                // a skipped instance contributes nothing
        X[b * 128 + lane] = 0.0f;
        X[b * 128 + 64 + lane] = 0.0f;
        DZ[b * D + lane] = 0.0f;
        DP[b * D + lane] = 0.0f;
        if (lane < 2 * T) DY[b * 2 * T + lane] = 0.0f;
        if (lane < 2) LOSSB[b * 2 + lane] = 0.0f;
        return;
    }
    const int64_t u = users[b];
    const float z = X[b * 128 + lane], p = U[u * D + lane];
    X[b * 128 + 64 + lane] = p;
    float dx0 = 0.0f, dx1 = 0.0f, lp = 0.0f, ln = 0.0f;
    for (int j = 0; j < 2 * T; ++j) {
        const bool is_pos = j < T;
        const int64_t t = is_pos ? pos[b * T + j] : neg[b * T + j - T];
        const float w0 = W2[t * 128 + lane], w1 = W2[t * 128 + 64 + lane];
        const float y = wave_sum(w0 * z + w1 * p) + b2[t];
        // binary_cross_entropy_with_logits and its derivative sigmoid(y) - label, times the mean's 1 / (n T)
        const float l = fmaxf(y, 0.0f) - (is_pos ? y : 0.0f) + log1pf(expf(-fabsf(y)));
        const float d = (is_pos ? -sigmoid_neg(y) : sigmoid_neg(-y)) * inv;
        if (is_pos) lp += l; else ln += l;
        dx0 = fmaf(d, w0, dx0);
        dx1 = fmaf(d, w1, dx1);
        if (lane == 0) DY[b * 2 * T + j] = d;
    }
    DZ[b * D + lane] = z > 0.0f ? dx0 : 0.0f;
    DP[b * D + lane] = dx1;
    if (lane == 0) {
        LOSSB[b * 2] = lp;
        LOSSB[b * 2 + 1] = ln;
    }
}

// ------------------------------------------------------------------------------------------------
// conv backward per instance: d_out through dropout, ReLU and arg-max (in place), the window rows' gradients
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(HW * 64) void cs_conv_bwd_kernel(Shape S, const float* __restrict__ shared, float* __restrict__ DOUT,
                                                              const uint8_t* __restrict__ MASK, const int8_t* __restrict__ ARG, int n,
                                                              float scale, float* __restrict__ DE) {
    __shared__ float sdE[HW][SKR_CASER_MAX_L * D];      // lane j owns column j of its wavefront's rows
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t b = static_cast<int64_t>(blockIdx.x) * HW + wv;
    if (b >= n) return;
    const int L = S.L, nh = S.nh, HK = S.HK;
    float* de = sdE[wv];
    for (int l = 0; l < L; ++l) de[l * D + lane] = 0.0f;
    const float* __restrict__ wvp = shared + S.o_wv;
    const float* __restrict__ WH = shared + S.o_wh;
    float* __restrict__ drow = DOUT + b * S.Fp;
    const uint8_t* __restrict__ mrow = MASK + b * S.Fp;
    for (int c = 0; c < S.nv; ++c) {
        const int j = c * D + lane;
        const float dv = mrow[j] ? drow[j] * scale : 0.0f;
        drow[j] = dv;
        for (int l = 0; l < L; ++l) de[l * D + lane] = fmaf(wvp[c * L + l], dv, de[l * D + lane]);
    }
    float hg[4];
    int ha[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int hk = 64 * q + lane;
        hg[q] = 0.0f;
        ha[q] = -1;
        if (hk < HK) {
            const int j = S.nv * D + hk;
            const int a = ARG[b * HK + hk];
            const float v = (mrow[j] && a >= 0) ? drow[j] * scale : 0.0f;
            drow[j] = v;
            hg[q] = v;
            ha[q] = a;
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        for (int i = 0; i < 64 && 64 * q + i < HK; ++i) {
            const float gv = __shfl(hg[q], i, 64);
            if (gv == 0.0f) continue;
            const int a = __shfl(ha[q], i, 64);
            const int hk = 64 * q + i, h = hk / nh + 1, k = hk % nh;
            const float* __restrict__ w = WH + static_cast<int64_t>(filter_base(nh, h) + k * h) * D + lane;
            for (int rr = 0; rr < h; ++rr) de[(a + rr) * D + lane] = fmaf(gv, w[rr * D], de[(a + rr) * D + lane]);
        }
    }
    for (int l = 0; l < L; ++l) DE[(b * L + l) * D + lane] = de[l * D + lane];
}

// ------------------------------------------------------------------------------------------------
// the filters' gradients: a workgroup per filter row, per vertical weight, per vertical bias
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(HW * 64) void cs_filter_grad_kernel(Shape S, const float* __restrict__ E, const int32_t* __restrict__ seqs,
                                                                 const float* __restrict__ DOUT, const int8_t* __restrict__ ARG, int n,
                                                                 int n_rows, int pad, float* __restrict__ gshared) {
    __shared__ float s_part[HW][D];
    __shared__ float s_b[HW];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int R = blockIdx.x, L = S.L, nh = S.nh;
    float acc = 0.0f, accb = 0.0f;
    int h = 1, hk = 0, rr = 0;
    if (R < S.rows) {
        // dWh[h,k,r,:] = sum_b g_b E[s_(t* + r)], dbh[h,k] = sum_b g_b: wavefront w takes the instances w, w + 4, ...
        while (filter_base(nh, h + 1) <= R) ++h;
        const int k = (R - filter_base(nh, h)) / h;
        rr = (R - filter_base(nh, h)) % h;
        hk = (h - 1) * nh + k;
        const int j = S.nv * D + hk;
        for (int c0 = 0; c0 < n; c0 += HW * 64) {
            const int64_t b = c0 + HW * lane + wv;
            float gl = 0.0f;
            int sl = -1;
            if (b < n) {
                gl = DOUT[b * S.Fp + j];
                if (gl != 0.0f) {
                    const int s = seqs[b * L + ARG[b * S.HK + hk] + rr];
                    sl = s == pad ? -1 : static_cast<int>(checked(s, n_rows));
                }
            }
            accb += gl;
            for (int i = 0; i < 64; ++i) {
                const float gv = __shfl(gl, i, 64);
                const int s = __shfl(sl, i, 64);
                if (gv != 0.0f && s >= 0) acc = fmaf(gv, E[static_cast<int64_t>(s) * D + lane], acc);
            }
        }
        accb = wave_sum(accb);
    } else if (R < S.rows + S.nv * L) {
        // dwv[c,l] = sum_b <d_out_v[b,c,:], E[s_l]>
        const int c = (R - S.rows) / L, l = (R - S.rows) % L;
        for (int64_t b = wv; b < n; b += HW) {
            const int s = seqs[b * L + l];
            const int64_t sc = s == pad ? -1 : checked(s, n_rows);
            if (sc >= 0) acc = fmaf(DOUT[b * S.Fp + c * D + lane], E[sc * D + lane], acc);
        }
        accb = wave_sum(acc);
    } else {
        // dbv[c] = sum_b sum_col d_out_v[b,c,col]
        const int c = R - S.rows - S.nv * L;
        for (int64_t b = wv; b < n; b += HW) acc += DOUT[b * S.Fp + c * D + lane];
        accb = wave_sum(acc);
    }
    s_part[wv][lane] = acc;
    if (lane == 0) s_b[wv] = accb;
    __syncthreads();
    if (wv != 0) return;
    const float tb = ((s_b[0] + s_b[1]) + s_b[2]) + s_b[3];
    if (R < S.rows) {
        gshared[S.o_wh + static_cast<int64_t>(R) * D + lane] += ((s_part[0][lane] + s_part[1][lane]) + s_part[2][lane]) + s_part[3][lane];
        if (rr == 0 && lane == 0) gshared[S.o_bh + hk] += tb;
    } else if (lane == 0) {
        if (R < S.rows + S.nv * L) gshared[S.o_wv + (R - S.rows)] += tb;
        else gshared[S.o_bv + (R - S.rows - S.nv * L)] += tb;
    }
}

// ------------------------------------------------------------------------------------------------
// rank by counting (as step_common.h's rank kernels, for three lists of different lengths) and the ordered adds
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int target_at(const int32_t* __restrict__ pos, const int32_t* __restrict__ neg, int nT, int o) {
    return o < nT ? pos[o] : neg[o - nT];
}

// order_u [n], order_s [n L], order_t [2 n T]: the positions of the user list, of the window entries and of pos || neg
// (both flattened) sorted by (id, position).  A workgroup ranks 256 entries of ONE list (blocks [0, bu) the users, [bu, bu + bs)
// the windows, the rest the targets) and walks that list through LDS, RC ids at a time: every thread reads the same word, four
// ids per 16-byte read.  (Walking the list in global memory, as the rank kernels of step_common.h do for their lists of at most
// 2 048 ids, took 386 us per step at n = 1024, L = 5, T = 3: the lists here are 5 120 and 6 144 long.)
constexpr int RC = 2048;

__global__ __launch_bounds__(256) void cs_rank_kernel(const int32_t* __restrict__ users, const int32_t* __restrict__ seqs,
                                                      const int32_t* __restrict__ pos, const int32_t* __restrict__ neg, int n, int nL, int nT,
                                                      int bu, int bs, int32_t* __restrict__ order_u, int32_t* __restrict__ order_s,
                                                      int32_t* __restrict__ order_t) {
    __shared__ __attribute__((aligned(16))) int32_t s_ids[RC];
    const int blk = blockIdx.x;
    const int which = blk < bu ? 0 : (blk < bu + bs ? 1 : 2);
    const int len = which == 0 ? n : (which == 1 ? nL : 2 * nT);
    const int kk = (blk - (which == 0 ? 0 : (which == 1 ? bu : bu + bs))) * 256 + threadIdx.x;
    auto at = [&](int o) { return which == 0 ? users[o] : (which == 1 ? seqs[o] : target_at(pos, neg, nT, o)); };
    const bool live = kk < len;
    const int id = live ? at(kk) : 0;
    int rank = 0;
    for (int c0 = 0; c0 < len; c0 += RC) {
        __syncthreads();
        // ids beyond the list: INT_MAX, which is below no id and equal to none that is ranked before its own position
        for (int j = threadIdx.x; j < RC; j += 256) s_ids[j] = c0 + j < len ? at(c0 + j) : 0x7fffffff;
        __syncthreads();
        const int lim = len - c0 < RC ? len - c0 : RC;
        const int before = kk - c0;                        // the entries j < before of this chunk precede position kk
        for (int j = 0; j < lim; j += 4) {
            const int4 o = *reinterpret_cast<const int4*>(s_ids + j);
            rank += (o.x < id || (o.x == id && j < before)) ? 1 : 0;
            rank += (o.y < id || (o.y == id && j + 1 < before)) ? 1 : 0;
            rank += (o.z < id || (o.z == id && j + 2 < before)) ? 1 : 0;
            rank += (o.w < id || (o.w == id && j + 3 < before)) ? 1 : 0;
        }
    }
    if (live) (which == 0 ? order_u : (which == 1 ? order_s : order_t))[rank] = kk;
}

// a wavefront per rank: the wavefront of an id's first rank adds that id's rows in rank order and adds the sum to the
// table's gradient -- one writer per distinct id.  The padding row and ids out of range get nothing.
__global__ __launch_bounds__(HW * 64) void cs_seg_add_kernel(Shape S, const int32_t* __restrict__ users, const int32_t* __restrict__ seqs,
                                                             const int32_t* __restrict__ pos, const int32_t* __restrict__ neg,
                                                             const int32_t* __restrict__ order_u, const int32_t* __restrict__ order_s,
                                                             const int32_t* __restrict__ order_t, int n, int n_users, int n_rows, int pad,
                                                             const float* __restrict__ DP, const float* __restrict__ DE,
                                                             const float* __restrict__ DY, const float* __restrict__ X,
                                                             float* __restrict__ gU, float* __restrict__ gE, float* __restrict__ gW2,
                                                             float* __restrict__ gb2) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int nL = n * S.L, nT = n * S.T, T = S.T;
    const int64_t w = static_cast<int64_t>(blockIdx.x) * HW + wv;
    if (w < n) {
        const int rk = static_cast<int>(w);
        const int id = users[order_u[rk]];
        if (id < 0 || id >= n_users || (rk > 0 && users[order_u[rk - 1]] == id)) return;
        float acc = 0.0f;
        for (int k = rk; k < n; ++k) {
            const int o = order_u[k];
            if (users[o] != id) break;
            acc += DP[static_cast<int64_t>(o) * D + lane];
        }
        gU[static_cast<int64_t>(id) * D + lane] += acc;
    } else if (w < n + nL) {
        const int rk = static_cast<int>(w - n);
        const int id = seqs[order_s[rk]];
        if (id < 0 || id >= n_rows || id == pad || (rk > 0 && seqs[order_s[rk - 1]] == id)) return;
        float acc = 0.0f;
        for (int k = rk; k < nL; ++k) {
            const int o = order_s[k];
            if (seqs[o] != id) break;
            acc += DE[static_cast<int64_t>(o) * D + lane];
        }
        gE[static_cast<int64_t>(id) * D + lane] += acc;
    } else if (w < n + nL + 2 * nT) {
        const int rk = static_cast<int>(w - n - nL);
        const int id = target_at(pos, neg, nT, order_t[rk]);
        if (id < 0 || id >= n_rows || id == pad || (rk > 0 && target_at(pos, neg, nT, order_t[rk - 1]) == id)) return;
        float a0 = 0.0f, a1 = 0.0f, ab = 0.0f;
        for (int k = rk; k < 2 * nT; ++k) {
            const int o = order_t[k];
            if (target_at(pos, neg, nT, o) != id) break;
            const int oo = o < nT ? o : o - nT;
            const int64_t b = oo / T;
            const float d = DY[b * 2 * T + (o < nT ? 0 : T) + oo % T];
            a0 = fmaf(d, X[b * 128 + lane], a0);
            a1 = fmaf(d, X[b * 128 + 64 + lane], a1);
            ab += d;
        }
        gW2[static_cast<int64_t>(id) * 128 + lane] += a0;
        gW2[static_cast<int64_t>(id) * 128 + 64 + lane] += a1;
        if (lane == 0) gb2[id] += ab;
    }
}

// loss[0], loss[1] = the batch's two cross-entropy sums, by a fixed tree; the other slots' words = 0
__global__ __launch_bounds__(1024) void cs_loss_kernel(const float* __restrict__ LOSSB, int n, float* __restrict__ loss, int loss_slots) {
    __shared__ float s[1024];
    float a = 0.0f, c = 0.0f;
    for (int b = threadIdx.x; b < n; b += 1024) {
        a += LOSSB[2 * b];
        c += LOSSB[2 * b + 1];
    }
    const float ta = block_sum_1024(a, s);
    const float tc = block_sum_1024(c, s);
    if (threadIdx.x == 0) {
        loss[0] = ta;
        loss[1] = tc;
    }
    for (int k = 2 + threadIdx.x; k < 2 * loss_slots; k += 1024) loss[k] = 0.0f;
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
struct Work {     // offsets in bytes, every one a multiple of 16
    int64_t out, dout, x, dz, dp, dy, de, lossb, dw1, part, arg, mask, valid, ordu, ords, ordt, total;
};

inline int64_t up16(int64_t x) { return (x + 15) & ~static_cast<int64_t>(15); }

inline Work work_layout(int64_t n, const Shape& S) {
    Work w;
    int64_t o = 0;
    const int64_t f = sizeof(float);
    w.out = o; o += up16(n * S.Fp * f);
    w.dout = o; o += up16(n * S.Fp * f);
    w.x = o; o += up16(n * 128 * f);
    w.dz = o; o += up16(n * D * f);
    w.dp = o; o += up16(n * D * f);
    w.dy = o; o += up16(n * 2 * SKR_CASER_MAX_T * f);
    w.de = o; o += up16(n * S.L * D * f);
    w.lossb = o; o += up16(n * 2 * f);
    w.dw1 = o; o += up16((static_cast<int64_t>(D) * S.Fp + D) * f);
    w.part = o; o += up16(dense_xty_floats(n, S.Fp) * f);
    w.arg = o; o += up16(n * S.HK);
    w.mask = o; o += up16(n * S.Fp);
    w.valid = o; o += up16(n * 4);
    w.ordu = o; o += up16(n * 4);
    w.ords = o; o += up16(n * S.L * 4);
    w.ordt = o; o += up16(n * 2 * SKR_CASER_MAX_T * 4);
    w.total = o;
    return w;
}

int check_shape(const char* who, int dim, int width, int seq_L, int nv, int nh) {
    SKR_REQUIRE(dim == D, "%s: dim must be 64 (got %d); pad narrower rows with zeros", who, dim);
    SKR_REQUIRE(width >= 1 && width <= D, "%s: 1 <= width <= 64 (got %d)", who, width);
    SKR_REQUIRE(seq_L >= 1 && seq_L <= SKR_CASER_MAX_L, "%s: need 1 <= seq_L <= %d (got %d)", who, SKR_CASER_MAX_L, seq_L);
    SKR_REQUIRE(nv >= 1 && nv <= SKR_CASER_MAX_NV, "%s: need 1 <= nv <= %d (got %d)", who, SKR_CASER_MAX_NV, nv);
    SKR_REQUIRE(nh >= 1 && nh <= SKR_CASER_MAX_NH, "%s: need 1 <= nh <= %d (got %d)", who, SKR_CASER_MAX_NH, nh);
    return SKR_OK;
}

int step_impl(const float* d_U, const float* d_E, const float* d_W2, const float* d_b2, const float* d_shared, const int32_t* d_u,
              const int32_t* d_seq, const int32_t* d_pos, const int32_t* d_neg, int n, int n_users, int n_rows, int pad_idx, int dim,
              int width, int seq_L, int seq_T, int nv, int nh, float dropout, const uint8_t* d_keep, uint8_t* d_keep_out, uint64_t seed,
              uint64_t step, float* d_gU, float* d_gE, float* d_gW2, float* d_gb2, float* d_gshared, void* d_work, size_t work_bytes,
              float* d_loss, int loss_slots, void* stream, float* h_ms) {
    const char* who = "skr_caser_step";
    SKR_REQUIRE(d_U && d_E && d_W2 && d_b2 && d_shared && d_u && d_seq && d_pos && d_neg && d_gU && d_gE && d_gW2 && d_gb2 &&
                    d_gshared && d_work && d_loss,
                "%s: NULL argument", who);
    SKR_REQUIRE(n >= 0 && n <= SKR_CASER_MAX_BATCH, "%s: need 0 <= n <= %d (got %d)", who, SKR_CASER_MAX_BATCH, n);
    SKR_REQUIRE(n_users > 0 && n_rows > 0, "%s: n_users = %d, n_rows = %d", who, n_users, n_rows);
    SKR_REQUIRE(pad_idx >= -1 && pad_idx < n_rows, "%s: pad_idx = %d is not a row of the item tables (or -1)", who, pad_idx);
    int rc = check_shape(who, dim, width, seq_L, nv, nh);
    if (rc != SKR_OK) return rc;
    SKR_REQUIRE(seq_T >= 1 && seq_T <= SKR_CASER_MAX_T, "%s: need 1 <= seq_T <= %d (got %d)", who, SKR_CASER_MAX_T, seq_T);
    SKR_REQUIRE(dropout >= 0.0f && dropout < 1.0f, "%s: need 0 <= dropout < 1 (got %g)", who, static_cast<double>(dropout));
    SKR_REQUIRE(loss_slots == 1 || loss_slots == SKR_LOSS_SLOTS, "%s: loss_slots must be 1 or %d", who, SKR_LOSS_SLOTS);
    if (n == 0) return SKR_OK;
    const Shape S = make_shape(seq_L, seq_T, nv, nh, width);
    const Work W = work_layout(n, S);
    SKR_REQUIRE(work_bytes >= static_cast<size_t>(W.total), "%s: d_work holds %zu bytes, skr_caser_workspace asks for %lld", who,
                work_bytes, static_cast<long long>(W.total));
    SKR_REQUIRE(((reinterpret_cast<uintptr_t>(d_shared) | reinterpret_cast<uintptr_t>(d_E) | reinterpret_cast<uintptr_t>(d_work)) & 15) == 0,
                "%s: d_shared, d_E and d_work must be 16-byte aligned", who);
    hipStream_t st = as_stream(stream);
    char* w = static_cast<char*>(d_work);
    float* OUT = reinterpret_cast<float*>(w + W.out);
    float* DOUT = reinterpret_cast<float*>(w + W.dout);
    float* X = reinterpret_cast<float*>(w + W.x);
    float* DZ = reinterpret_cast<float*>(w + W.dz);
    float* DP = reinterpret_cast<float*>(w + W.dp);
    float* DY = reinterpret_cast<float*>(w + W.dy);
    float* DE = reinterpret_cast<float*>(w + W.de);
    float* LOSSB = reinterpret_cast<float*>(w + W.lossb);
    float* DW1 = reinterpret_cast<float*>(w + W.dw1);
    float* part = reinterpret_cast<float*>(w + W.part);
    int8_t* ARG = reinterpret_cast<int8_t*>(w + W.arg);
    uint8_t* MASK = reinterpret_cast<uint8_t*>(w + W.mask);
    int32_t* VALID = reinterpret_cast<int32_t*>(w + W.valid);
    int32_t* ordu = reinterpret_cast<int32_t*>(w + W.ordu);
    int32_t* ords = reinterpret_cast<int32_t*>(w + W.ords);
    int32_t* ordt = reinterpret_cast<int32_t*>(w + W.ordt);
    const float scale = dropout > 0.0f ? 1.0f / (1.0f - dropout) : 1.0f;
    const float inv = 1.0f / static_cast<float>(static_cast<int64_t>(n) * seq_T);
    const int per4 = (n + HW - 1) / HW;
    StepTimer<SKR_CASER_LAUNCHES + 1> mk(h_ms, st);
    SKR_HIP(mk.mark());
    hipLaunchKernelGGL(cs_conv_kernel<true>, dim3((n + IB - 1) / IB), dim3(HW * 64), 0, st, S, d_E, d_shared, d_u, 0, d_seq, d_pos, d_neg,
                       n, n_users, n_rows, pad_idx, dropout, scale, d_keep, d_keep_out, seed, step, OUT, MASK, ARG, VALID);
    SKR_HIP(mk.mark());
    hipLaunchKernelGGL(cs_fc_kernel<true>, dim3((n + 16 * HW - 1) / (16 * HW)), dim3(HW * 64), 0, st, S, d_shared, OUT, n, VALID, d_u, 0,
                       d_U, X);
    SKR_HIP(mk.mark());
    hipLaunchKernelGGL(cs_score_kernel, dim3(per4), dim3(HW * 64), 0, st, S, d_U, d_W2, d_b2, d_u, d_pos, d_neg, VALID, n, inv, X, DY, DZ,
                       DP, LOSSB);
    SKR_HIP(mk.mark());
    if ((rc = dense_rows_w(DZ, n, S.Fp, d_shared + S.o_w1, DOUT, 0, st)) != SKR_OK) return rc;      // d_out = dz W1
    SKR_HIP(mk.mark());
    if ((rc = dense_xty(DZ, OUT, n, S.Fp, part, DW1, st)) != SKR_OK) return rc;                     // dW1 | db1 = dz^T out | column sums
    {
        const int64_t len = static_cast<int64_t>(D) * S.Fp + D;
        hipLaunchKernelGGL(add_kernel<256>, dim3(static_cast<unsigned>((len + 255) / 256)), dim3(256), 0, st, d_gshared + S.o_w1, DW1, len);
    }
    SKR_HIP(mk.mark());
    hipLaunchKernelGGL(cs_conv_bwd_kernel, dim3(per4), dim3(HW * 64), 0, st, S, d_shared, DOUT, MASK, ARG, n, scale, DE);
    SKR_HIP(mk.mark());
    hipLaunchKernelGGL(cs_filter_grad_kernel, dim3(S.rows + nv * seq_L + nv), dim3(HW * 64), 0, st, S, d_E, d_seq, DOUT, ARG, n, n_rows,
                       pad_idx, d_gshared);
    SKR_HIP(mk.mark());
    const int nL = n * seq_L, nT = n * seq_T, lists = n + nL + 2 * nT;
    const int bu = (n + 255) / 256, bs = (nL + 255) / 256, bt = (2 * nT + 255) / 256;
    hipLaunchKernelGGL(cs_rank_kernel, dim3(bu + bs + bt), dim3(256), 0, st, d_u, d_seq, d_pos, d_neg, n, nL, nT, bu, bs, ordu, ords, ordt);
    SKR_HIP(mk.mark());
    hipLaunchKernelGGL(cs_seg_add_kernel, dim3((lists + HW - 1) / HW), dim3(HW * 64), 0, st, S, d_u, d_seq, d_pos, d_neg, ordu, ords, ordt,
                       n, n_users, n_rows, pad_idx, DP, DE, DY, X, d_gU, d_gE, d_gW2, d_gb2);
    SKR_HIP(mk.mark());
    hipLaunchKernelGGL(cs_loss_kernel, dim3(1), dim3(1024), 0, st, LOSSB, n, d_loss, loss_slots);
    SKR_HIP(mk.mark());
    SKR_LAUNCH_CHECK();
    SKR_HIP(mk.finish());
    return SKR_OK;
}

}  // namespace

extern "C" {

size_t skr_caser_workspace(int n, int seq_L, int nv, int nh) {
    if (n < 1 || n > SKR_CASER_MAX_BATCH || seq_L < 1 || seq_L > SKR_CASER_MAX_L || nv < 1 || nv > SKR_CASER_MAX_NV || nh < 1 ||
        nh > SKR_CASER_MAX_NH)
        return 0;
    return static_cast<size_t>(work_layout(n, make_shape(seq_L, 1, nv, nh, D)).total);
}

int skr_caser_step(const float* d_U, const float* d_E, const float* d_W2, const float* d_b2, const float* d_shared, const int32_t* d_u,
                   const int32_t* d_seq, const int32_t* d_pos, const int32_t* d_neg, int n, int n_users, int n_rows, int pad_idx, int dim,
                   int width, int seq_L, int seq_T, int nv, int nh, float dropout, const uint8_t* d_keep, uint8_t* d_keep_out,
                   uint64_t seed, uint64_t step, float* d_gU, float* d_gE, float* d_gW2, float* d_gb2, float* d_gshared, void* d_work,
                   size_t work_bytes, float* d_loss, int loss_slots, void* stream) {
    return step_impl(d_U, d_E, d_W2, d_b2, d_shared, d_u, d_seq, d_pos, d_neg, n, n_users, n_rows, pad_idx, dim, width, seq_L, seq_T, nv,
                     nh, dropout, d_keep, d_keep_out, seed, step, d_gU, d_gE, d_gW2, d_gb2, d_gshared, d_work, work_bytes, d_loss,
                     loss_slots, stream, nullptr);
}

int skr_caser_step_timed(const float* d_U, const float* d_E, const float* d_W2, const float* d_b2, const float* d_shared,
                         const int32_t* d_u, const int32_t* d_seq, const int32_t* d_pos, const int32_t* d_neg, int n, int n_users,
                         int n_rows, int pad_idx, int dim, int width, int seq_L, int seq_T, int nv, int nh, float dropout,
                         const uint8_t* d_keep, uint8_t* d_keep_out, uint64_t seed, uint64_t step, float* d_gU, float* d_gE, float* d_gW2,
                         float* d_gb2, float* d_gshared, void* d_work, size_t work_bytes, float* d_loss, int loss_slots, void* stream,
                         float* h_ms) {
    SKR_REQUIRE(h_ms != nullptr, "skr_caser_step_timed: NULL argument");
    return step_impl(d_U, d_E, d_W2, d_b2, d_shared, d_u, d_seq, d_pos, d_neg, n, n_users, n_rows, pad_idx, dim, width, seq_L, seq_T, nv,
                     nh, dropout, d_keep, d_keep_out, seed, step, d_gU, d_gE, d_gW2, d_gb2, d_gshared, d_work, work_bytes, d_loss,
                     loss_slots, stream, h_ms);
}

int skr_caser_queries(const float* d_U, const float* d_E, const float* d_shared, const int32_t* d_users, int n, const int32_t* d_windows,
                      int n_users, int n_rows, int pad_idx, int dim, int width, int seq_L, int nv, int nh, void* d_work,
                      size_t work_bytes, float* d_Q, void* stream) {
    const char* who = "skr_caser_queries";
    SKR_REQUIRE(d_U && d_E && d_shared && d_windows && d_work && d_Q, "%s: NULL argument", who);
    SKR_REQUIRE(n >= 0 && n_users > 0 && n_rows > 0, "%s: n = %d, n_users = %d, n_rows = %d", who, n, n_users, n_rows);
    SKR_REQUIRE(d_users || n <= n_users, "%s: without a user list n = %d must not exceed n_users = %d", who, n, n_users);
    SKR_REQUIRE(pad_idx >= -1 && pad_idx < n_rows, "%s: pad_idx = %d is not a row of the item table (or -1)", who, pad_idx);
    const int rc = check_shape(who, dim, width, seq_L, nv, nh);
    if (rc != SKR_OK) return rc;
    if (n == 0) return SKR_OK;
    const Shape S = make_shape(seq_L, 1, nv, nh, width);
    // the users go through d_work in chunks: a chunk's `out` rows [m][Fp], then its flags [m]
    const int64_t per_user = static_cast<int64_t>(S.Fp) * sizeof(float) + sizeof(int32_t);
    int64_t m = (static_cast<int64_t>(work_bytes) - 16) / per_user;
    m = m / 64 * 64;
    SKR_REQUIRE(m >= 64, "%s: d_work holds %zu bytes, fewer than a chunk of 64 users needs (%lld)", who, work_bytes,
                static_cast<long long>(64 * per_user + 16));
    SKR_REQUIRE(((reinterpret_cast<uintptr_t>(d_shared) | reinterpret_cast<uintptr_t>(d_E) | reinterpret_cast<uintptr_t>(d_work)) & 15) == 0,
                "%s: d_shared, d_E and d_work must be 16-byte aligned", who);
    hipStream_t st = as_stream(stream);
    float* OUT = static_cast<float*>(d_work);
    int32_t* VALID = reinterpret_cast<int32_t*>(static_cast<char*>(d_work) + up16(m * S.Fp * static_cast<int64_t>(sizeof(float))));
    for (int64_t c0 = 0; c0 < n; c0 += m) {
        const int cn = static_cast<int>(n - c0 < m ? n - c0 : m);
        const int32_t* us = d_users ? d_users + c0 : nullptr;
        const int32_t* win = d_windows + c0 * seq_L;
        hipLaunchKernelGGL(cs_conv_kernel<false>, dim3((cn + IB - 1) / IB), dim3(HW * 64), 0, st, S, d_E, d_shared, us, static_cast<int>(c0),
                           win, nullptr, nullptr, cn, n_users, n_rows, pad_idx, 0.0f, 1.0f, nullptr, nullptr, 0, 0, OUT, nullptr, nullptr,
                           VALID);
        hipLaunchKernelGGL(cs_fc_kernel<false>, dim3((cn + 16 * HW - 1) / (16 * HW)), dim3(HW * 64), 0, st, S, d_shared, OUT, cn, VALID, us,
                           static_cast<int>(c0), d_U, d_Q);
    }
    SKR_LAUNCH_CHECK();
    return SKR_OK;
}

}  // extern "C"
