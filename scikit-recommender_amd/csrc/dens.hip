// dens.hip -- DENS (Disentangled Negative Sampling for Collaborative Filtering, WSDM 2023): the gated hard-negative
// selection, the loss and the whole backward of one training step, and the host entry that issues the step.
//
// Replaces the stock torch ops the reference issues per step (no native code there):
//   recommender/DENS.py:115-136  the H propagations of the normalised bipartite adjacency, every hop kept
//   recommender/DENS.py:236-257  the four gates on [B, n_negs, H + 1, d] intermediates and the arg-max per (row, hop)
//   recommender/DENS.py:318-374  the pooled BPR term, the four gated terms (the gates evaluated a second time there), the
//                                regulariser on the hop-0 rows, and autograd's backward through all of it
//
// Layout: every table has 64-float rows, zero beyond d.  Users and items share flat [U + I, 64] tables (user rows first).
// The parameters are one flat buffer: the [U + I, 64] rows, then four gate blocks (user, item, pos, neg) of a row-major
// W [64 out][64 in] followed by b [64], zero beyond d.  The gradient has the same layout.
//
// Launches of a step:
//   2H plan runs   X_h = A-hat X_(h-1): user rows from A, item rows from A^T; all hop tables are kept
//   select         per (64 batch rows, hop): the four gates in LDS, the gate products as 16-row tiles on
//                  v_mfma_f32_16x16x4_f32 (exact fp32), the scores and the arg-max; keeps the gate values gp and gn of the
//                  chosen candidate -- the loss uses the same numbers
//   pool           per batch row: the pooled vectors, the five scores, the loss terms and the pooled vectors' gradients
//   loss           the three loss components
//   back           per 64 (row, hop) pairs: the gradient rows of s, p and the chosen candidate through the gates (the
//                  transposed gates in LDS), the gates' weight and bias gradients as per-workgroup partial sums
//   gate_reduce    the partial sums in workgroup order
//   rank, seg_add  the gradient rows into G_h, per distinct node id, in rank order
//   2H plan runs   acc = G_H; acc = A-hat acc + G_h for h = H-1 .. 0 (the addend epilogue); the last writes the gradient
//
// The MFMA operand mapping is mfma_tile.h's k = 16 g + kk.
//
// Determinism: there is no floating-point atomic anywhere in the step.
#include "skr_common.h"
#include "mfma_tile.h"
#include "step_common.h"

#include <algorithm>
#include <cmath>

namespace {

using namespace skr;

constexpr int D = 64;          // columns of every table
constexpr int LDP = 68;        // LDS row stride
constexpr int HW = 4;          // wavefronts per workgroup
constexpr int TB = 64;         // rows of a workgroup's tile: 16 per wavefront
constexpr int MAXH = SKR_DENS_MAX_HOPS;
constexpr int MAXK = SKR_DENS_MAX_NEGS;
constexpr int MAXB = SKR_DENS_MAX_BATCH;
constexpr int GATE = D * D + D;   // floats of one gate block
constexpr int NGATE = 4;          // user, item, pos, neg
constexpr int MAX_WG = SKR_DENS_MAX_WG;

struct Tables { const float* x[MAXH + 1]; };

__device__ __forceinline__ const float* hop_table(const Tables& T, int h) {
    return h == 0 ? T.x[0] : h == 1 ? T.x[1] : h == 2 ? T.x[2] : T.x[3];
}

__device__ __forceinline__ float sigmoid_f(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ float softplus_f(float x) { return fmaxf(x, 0.0f) + log1pf(expf(-fabsf(x))); }

// the four gates into LDS: sW[m][row][col], row stride LDP; transposed: sW[m][in][out] = W_m[out][in]
__device__ __forceinline__ void load_gates(float* __restrict__ sW, const float* __restrict__ gates, bool transposed) {
    for (int idx = threadIdx.x; idx < NGATE * D * 16; idx += HW * 64) {
        const int m = idx >> 10, row = (idx >> 4) & 63, c4 = idx & 15;
        const float4 v = *reinterpret_cast<const float4*>(gates + static_cast<int64_t>(m) * GATE + row * D + c4 * 4);
        float* base = sW + m * D * LDP;
        if (!transposed) {
            *reinterpret_cast<float4*>(base + row * LDP + c4 * 4) = v;
        } else {
            base[(c4 * 4 + 0) * LDP + row] = v.x;
            base[(c4 * 4 + 1) * LDP + row] = v.y;
            base[(c4 * 4 + 2) * LDP + row] = v.z;
            base[(c4 * 4 + 3) * LDP + row] = v.w;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// select: gates, scores and the arg-max of (64 batch rows, one hop)
// ------------------------------------------------------------------------------------------------
// gp_out / gn_out [(H + 1) n, 64] at row h n + b: sigmoid(item_gate(p) + user_gate(s)) and the chosen candidate's
// sigmoid(neg_gate(c) + pos_gate(p gp)); selitem [(H + 1) n]: the chosen item (-1: out of range); sel_out [n, H + 1]
__global__ __launch_bounds__(HW * 64) void dn_select_kernel(Tables T, const float* __restrict__ gates,
                                                            const int32_t* __restrict__ uids, const int32_t* __restrict__ pos,
                                                            const int32_t* __restrict__ cand, const int32_t* __restrict__ sel_in,
                                                            int n, int U, int I, int H, int K, float w, float* __restrict__ gp_out,
                                                            float* __restrict__ gn_out, int32_t* __restrict__ selitem,
                                                            int32_t* __restrict__ sel_out) {
    __shared__ __attribute__((aligned(16))) float sW[NGATE * D * LDP];
    __shared__ __attribute__((aligned(16))) float sT[TB * LDP];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
    const int h = blockIdx.y;
    const float* __restrict__ X = hop_table(T, h);
    load_gates(sW, gates, false);
    const int b0 = blockIdx.x * TB + wv * 16;
    // the A operands: lane (r, g) holds columns [16 g, 16 g + 16) of the wavefront's row r
    const int bA = b0 + r;
    const int64_t uA = bA < n ? checked(uids[bA], U) : -1, pA = bA < n ? checked(pos[bA], I) : -1;
    float sa[16], pa[16];
    load_row_a(sa, X, uA, g);
    load_row_a(pa, X, pA < 0 ? -1 : U + pA, g);
    // the results: lane (r, g) holds column 16 nb + r of the rows 4 g + rr
    int bD[4], forced[4];
    int64_t uD[4], pD[4];
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        bD[rr] = b0 + 4 * g + rr;
        const bool in = bD[rr] < n;
        uD[rr] = in ? checked(uids[bD[rr]], U) : -1;
        pD[rr] = in ? checked(pos[bD[rr]], I) : -1;
        forced[rr] = (in && sel_in != nullptr) ? sel_in[static_cast<int64_t>(bD[rr]) * (H + 1) + h] : -1;
        if (forced[rr] >= K) forced[rr] = K - 1;
    }
    __syncthreads();
    f32x4 acc[4];
    zero_acc(acc);
    tile_product<LDP>(acc, pa, sW + 1 * D * LDP, r, g);
    tile_product<LDP>(acc, sa, sW + 0 * D * LDP, r, g);
    f32x4 sD[4];
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) {
        const int col = nb * 16 + r;
        const float bias = gates[0 * GATE + D * D + col] + gates[1 * GATE + D * D + col];
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const float pv = pD[rr] >= 0 ? X[(U + pD[rr]) * D + col] : 0.0f;
            sD[nb][rr] = uD[rr] >= 0 ? X[uD[rr] * D + col] : 0.0f;
            const float gpv = sigmoid_f(acc[nb][rr] + bias);
            if (bD[rr] < n) gp_out[(static_cast<int64_t>(h) * n + bD[rr]) * D + col] = gpv;
            sT[(wv * 16 + 4 * g + rr) * LDP + col] = pv * gpv;
        }
    }
    __syncthreads();
    float pra[16];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float4 v = *reinterpret_cast<const float4*>(sT + (wv * 16 + r) * LDP + 16 * g + 4 * q);
        pra[4 * q + 0] = v.x; pra[4 * q + 1] = v.y; pra[4 * q + 2] = v.z; pra[4 * q + 3] = v.w;
    }
    f32x4 qv[4];
    zero_acc(qv);
    tile_product<LDP>(qv, pra, sW + 2 * D * LDP, r, g);
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) {
        const int col = nb * 16 + r;
        const float bias = gates[2 * GATE + D * D + col] + gates[3 * GATE + D * D + col];
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) qv[nb][rr] += bias;
    }
    float best[4];
    int bestk[4];
    int64_t bestid[4];
    f32x4 bgn[4];
    zero_acc(bgn);
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) { best[rr] = -INFINITY; bestk[rr] = 0; bestid[rr] = -1; }
    for (int k = 0; k < K; ++k) {
        const int64_t cA = bA < n ? checked(cand[static_cast<int64_t>(bA) * K + k], I) : -1;
        float ca[16];
        load_row_a(ca, X, cA < 0 ? -1 : U + cA, g);
        f32x4 z[4];
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) z[nb] = qv[nb];
        tile_product<LDP>(z, ca, sW + 3 * D * LDP, r, g);
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int64_t cD = bD[rr] < n ? checked(cand[static_cast<int64_t>(bD[rr]) * K + k], I) : -1;
            float gnv[4], part = 0.0f;
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) {
                const float cv = cD >= 0 ? X[(U + cD) * D + nb * 16 + r] : 0.0f;
                gnv[nb] = sigmoid_f(z[nb][rr]);
                part += sD[nb][rr] * (w * cv - cv * gnv[nb]);
            }
            const float score = sum16(part);
            const bool take = forced[rr] >= 0 ? k == forced[rr] : (k == 0 || score > best[rr]);
            if (take) {
                best[rr] = score;
                bestk[rr] = k;
                bestid[rr] = cD;
#pragma unroll
                for (int nb = 0; nb < 4; ++nb) bgn[nb][rr] = gnv[nb];
            }
        }
    }
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        if (bD[rr] >= n) continue;
        const int64_t row = static_cast<int64_t>(h) * n + bD[rr];
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) gn_out[row * D + nb * 16 + r] = bgn[nb][rr];
        if (r == 0) {
            selitem[row] = static_cast<int32_t>(bestid[rr]);
            if (sel_out != nullptr) sel_out[static_cast<int64_t>(bD[rr]) * (H + 1) + h] = bestk[rr];
        }
    }
}

// ------------------------------------------------------------------------------------------------
// pool: per batch row the pooled vectors, the scores, the loss terms, the pooled vectors' gradients
// ------------------------------------------------------------------------------------------------
// PG [5][n][64]: the gradients of one hop's s (through u), p, chosen c, p gp, c gn -- the pooled vectors' gradients / (H + 1)
// lossb [3][n]: softplus(u.N - u.P), the sum of the four gated terms, |s_0|^2 + |p_0|^2 + |c_0|^2
__global__ __launch_bounds__(HW * 64) void dn_pool_kernel(Tables T, const int32_t* __restrict__ uids, const int32_t* __restrict__ pos,
                                                          const int32_t* __restrict__ selitem, int n, int U, int I, int H,
                                                          float gamma, const float* __restrict__ gp, const float* __restrict__ gn,
                                                          float* __restrict__ PG, float* __restrict__ lossb) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int b = blockIdx.x * HW + wv;
    if (b >= n) return;
    const int64_t u = checked(uids[b], U), p = checked(pos[b], I);
    const bool valid = u >= 0 && p >= 0;
    float vu = 0.0f, vP = 0.0f, vN = 0.0f, vPr = 0.0f, vNr = 0.0f, sq = 0.0f;
    for (int h = 0; h <= H; ++h) {
        const float* __restrict__ X = hop_table(T, h);
        const int64_t row = static_cast<int64_t>(h) * n + b;
        const int64_t c = checked(selitem[row], I);
        const float s = u >= 0 ? X[u * D + lane] : 0.0f;
        const float pv = p >= 0 ? X[(U + p) * D + lane] : 0.0f;
        const float cv = c >= 0 ? X[(U + c) * D + lane] : 0.0f;
        vu += s; vP += pv; vN += cv;
        vPr += pv * gp[row * D + lane];
        vNr += cv * gn[row * D + lane];
        if (h == 0) sq = (s * s + pv * pv) + cv * cv;
    }
    const float inv = 1.0f / static_cast<float>(H + 1);
    vu *= inv; vP *= inv; vN *= inv; vPr *= inv; vNr *= inv;
    const float a = skr::wave_sum(vu * vP), bn = skr::wave_sum(vu * vN), r = skr::wave_sum(vu * vPr), t = skr::wave_sum(vu * vNr);
    sq = skr::wave_sum(sq);
    // u.P_ir = a - r, u.N_ir = bn - t
    const float x1 = bn - a, x2 = (a - r) - r, x3 = t - (bn - t), x4 = t - r, x5 = (a - r) - (bn - t);
    const float gq = gamma > 0.0f ? 0.25f * gamma : 0.0f;
    float l1 = 0.0f, l2 = 0.0f, da = 0.0f, db = 0.0f, dr = 0.0f, dt = 0.0f;
    if (valid) {
        l1 = softplus_f(x1);
        const float s1 = sigmoid_f(x1);
        da = -s1;
        db = s1;
        if (gq > 0.0f) {
            l2 = (softplus_f(x2) + softplus_f(x3)) + (softplus_f(x4) + softplus_f(x5));
            const float s2 = sigmoid_f(x2), s3 = sigmoid_f(x3), s4 = sigmoid_f(x4), s5 = sigmoid_f(x5);
            da += gq * (s2 + s5);
            db -= gq * (s3 + s5);
            dr = -gq * (2.0f * s2 + s4 + s5);
            dt = gq * (2.0f * s3 + s4 + s5);
        }
    } else {
        sq = 0.0f;
    }
    const float sc = inv / static_cast<float>(n);            // the mean over the batch, the mean over the hops
    da *= sc; db *= sc; dr *= sc; dt *= sc;
    const int64_t nD = static_cast<int64_t>(n) * D, o = static_cast<int64_t>(b) * D + lane;
    PG[0 * nD + o] = ((da * vP + db * vN) + dr * vPr) + dt * vNr;
    PG[1 * nD + o] = da * vu;
    PG[2 * nD + o] = db * vu;
    PG[3 * nD + o] = dr * vu;
    PG[4 * nD + o] = dt * vu;
    if (lane == 0) {
        lossb[b] = l1;
        lossb[n + b] = l2;
        lossb[2 * n + b] = sq;
    }
}

// loss[0] = mf (DENS.py:333, :361-366), loss[1] = emb (:369-372), loss[2] = their sum
__global__ __launch_bounds__(1024) void dn_loss_kernel(const float* __restrict__ lossb, int n, float gamma, float l2,
                                                       float* __restrict__ loss) {
    __shared__ float s[1024];
    const int t = threadIdx.x;
    float a = 0.0f, b = 0.0f, c = 0.0f;
    for (int k = t; k < n; k += 1024) { a += lossb[k]; b += lossb[n + k]; c += lossb[2 * n + k]; }
    const float fn = static_cast<float>(n);
    const float s1 = block_sum_1024(a, s) / fn, s2 = block_sum_1024(b, s) / fn, s3 = block_sum_1024(c, s);
    if (t == 0) {
        const float mf = gamma > 0.0f ? s1 + gamma * s2 / 4.0f : s1;
        const float emb = l2 * (s3 / 2.0f) / fn;
        loss[0] = mf;
        loss[1] = emb;
        loss[2] = mf + emb;
    }
}

// ------------------------------------------------------------------------------------------------
// back: the gradient rows through the gates, the gates' gradients
// ------------------------------------------------------------------------------------------------
// the lane's share of an A operand (a[kk] = v[row][16 g + kk]) into the transposed image sXT[col][row]
__device__ __forceinline__ void store_transposed(float* __restrict__ sXT, const float a[16], int row, int g) {
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) sXT[(16 * g + kk) * LDP + row] = a[kk];
}

__device__ __forceinline__ void load_vec_a(float a[16], const float* __restrict__ rows, int64_t row, int g) {
    load_row_a(a, rows, row, g);
}

// rows are the (hop, batch row) pairs h n + b.  Per row, with z = neg_gate(c) + pos_gate(p gp), a = item_gate(p) + user_gate(s):
//   dz = d(c gn) c gn (1 - gn);  dc = dN + d(c gn) gn + W_neg^T dz;  d(p gp) = dP_r + W_pos^T dz
//   da = d(p gp) p gp (1 - gp);  dp = dP + d(p gp) gp + W_item^T da;  ds = du + W_user^T da
// and at hop 0 the regulariser's l2 / n times the row.  Gs / Gp / Gc [(H + 1) n, 64] receive ds / dp / dc.
// part [gridDim.x][4 GATE]: the workgroup's sums of dW_user = da^T s, dW_item = da^T p, dW_pos = dz^T (p gp), dW_neg = dz^T c and
// of the biases' da, da, dz, dz.
__global__ __launch_bounds__(HW * 64) void dn_back_kernel(Tables T, const float* __restrict__ gates, const int32_t* __restrict__ uids,
                                                          const int32_t* __restrict__ pos, const int32_t* __restrict__ selitem, int n,
                                                          int U, int I, int H, float regc, const float* __restrict__ gp,
                                                          const float* __restrict__ gn, const float* __restrict__ PG,
                                                          float* __restrict__ Gs, float* __restrict__ Gp, float* __restrict__ Gc,
                                                          float* __restrict__ part, int chunks) {
    __shared__ __attribute__((aligned(16))) float sWT[NGATE * D * LDP];
    __shared__ __attribute__((aligned(16))) float sG[D * LDP];
    __shared__ __attribute__((aligned(16))) float sX0[D * LDP];
    __shared__ __attribute__((aligned(16))) float sX1[D * LDP];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
    const int64_t R = static_cast<int64_t>(n) * (H + 1), nD = static_cast<int64_t>(n) * D;
    load_gates(sWT, gates, true);
    f32x4 dW[NGATE][4];
#pragma unroll
    for (int m = 0; m < NGATE; ++m) zero_acc(dW[m]);
    float dbz = 0.0f, dba = 0.0f;
    for (int chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
        const int64_t row0 = static_cast<int64_t>(chunk) * TB + wv * 16;
        // ---- A layout: row r of the wavefront
        const int64_t rowA = row0 + r;
        const bool inA = rowA < R;
        const int hA = inA ? static_cast<int>(rowA / n) : 0;
        const int bA = inA ? static_cast<int>(rowA - static_cast<int64_t>(hA) * n) : 0;
        const float* __restrict__ XA = hop_table(T, hA);
        const int64_t uA = inA ? checked(uids[bA], U) : -1, pA = inA ? checked(pos[bA], I) : -1, cA = inA ? checked(selitem[rowA], I) : -1;
        float dz[16], pa[16], tmp[16], tmp2[16];
        {
            load_row_a(tmp, XA, cA < 0 ? -1 : U + cA, g);                 // c
            load_vec_a(tmp2, gn, inA ? rowA : -1, g);                    // gn
            load_vec_a(dz, PG + 4 * nD, inA ? bA : -1, g);               // d(c gn)
#pragma unroll
            for (int kk = 0; kk < 16; ++kk) dz[kk] = dz[kk] * tmp[kk] * (tmp2[kk] * (1.0f - tmp2[kk]));
        }
        __syncthreads();                                       // the previous chunk's products still read the images
        store_transposed(sG, dz, wv * 16 + r, g);
        store_transposed(sX0, tmp, wv * 16 + r, g);
        load_row_a(pa, XA, pA < 0 ? -1 : U + pA, g);                      // p
        load_vec_a(tmp2, gp, inA ? rowA : -1, g);                        // gp
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) tmp[kk] = pa[kk] * tmp2[kk];     // p gp
        store_transposed(sX1, tmp, wv * 16 + r, g);
        __syncthreads();
        float slab[16];
        load_slab<LDP>(slab, sG, wv * 16 + r, g);
        if (threadIdx.x < D) dbz += column_sum<LDP>(sG, threadIdx.x);
        tile_product<LDP>(dW[3], slab, sX0, r, g);
        tile_product<LDP>(dW[2], slab, sX1, r, g);
        f32x4 mm1[4], mm2[4];
        zero_acc(mm1);
        zero_acc(mm2);
        tile_product<LDP>(mm1, dz, sWT + 3 * D * LDP, r, g);
        tile_product<LDP>(mm2, dz, sWT + 2 * D * LDP, r, g);
        // ---- D layout: rows 4 g + rr, column 16 nb + r
        f32x4 daD[4], dpg[4], pDv[4];
        int64_t rowD[4];
        int hD[4], bD[4];
        int64_t uD[4], pD[4];
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            rowD[rr] = row0 + 4 * g + rr;
            const bool in = rowD[rr] < R;
            hD[rr] = in ? static_cast<int>(rowD[rr] / n) : 0;
            bD[rr] = in ? static_cast<int>(rowD[rr] - static_cast<int64_t>(hD[rr]) * n) : 0;
            uD[rr] = in ? checked(uids[bD[rr]], U) : -1;
            pD[rr] = in ? checked(pos[bD[rr]], I) : -1;
            const int64_t cD = in ? checked(selitem[rowD[rr]], I) : -1;
            const float* __restrict__ XD = hop_table(T, hD[rr]);
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) {
                const int col = nb * 16 + r;
                float da = 0.0f, pg = 0.0f, pv = 0.0f;
                if (in) {
                    const int64_t o = static_cast<int64_t>(bD[rr]) * D + col;
                    const float gnv = gn[rowD[rr] * D + col], gpv = gp[rowD[rr] * D + col];
                    float dc = (PG[2 * nD + o] + PG[4 * nD + o] * gnv) + mm1[nb][rr];
                    if (hD[rr] == 0 && cD >= 0 && uD[rr] >= 0 && pD[rr] >= 0) dc += regc * XD[(U + cD) * D + col];
                    Gc[rowD[rr] * D + col] = dc;
                    const float dpr = PG[3 * nD + o] + mm2[nb][rr];
                    pv = pD[rr] >= 0 ? XD[(U + pD[rr]) * D + col] : 0.0f;
                    da = dpr * pv * (gpv * (1.0f - gpv));
                    pg = dpr * gpv;
                }
                daD[nb][rr] = da;
                dpg[nb][rr] = pg;
                pDv[nb][rr] = pv;
            }
        }
        __syncthreads();                                       // the products above have read sG, sX0 and sX1
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) {
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) sG[(nb * 16 + r) * LDP + wv * 16 + 4 * g + rr] = daD[nb][rr];
        }
        store_transposed(sX0, pa, wv * 16 + r, g);
        load_row_a(tmp, XA, uA, g);                                      // s
        store_transposed(sX1, tmp, wv * 16 + r, g);
        __syncthreads();
        load_slab<LDP>(slab, sG, wv * 16 + r, g);
        float daA[16];
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) daA[kk] = sG[(16 * g + kk) * LDP + wv * 16 + r];
        if (threadIdx.x < D) dba += column_sum<LDP>(sG, threadIdx.x);
        tile_product<LDP>(dW[1], slab, sX0, r, g);
        tile_product<LDP>(dW[0], slab, sX1, r, g);
        zero_acc(mm1);
        zero_acc(mm2);
        tile_product<LDP>(mm1, daA, sWT + 1 * D * LDP, r, g);
        tile_product<LDP>(mm2, daA, sWT + 0 * D * LDP, r, g);
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            if (rowD[rr] >= R) continue;
            const float* __restrict__ XD = hop_table(T, hD[rr]);
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) {
                const int col = nb * 16 + r;
                const int64_t o = static_cast<int64_t>(bD[rr]) * D + col;
                float dp = (PG[1 * nD + o] + dpg[nb][rr]) + mm1[nb][rr];
                float ds = PG[0 * nD + o] + mm2[nb][rr];
                if (hD[rr] == 0 && uD[rr] >= 0 && pD[rr] >= 0) {     // a skipped row has no regulariser either (pool: sq = 0)
                    dp += regc * pDv[nb][rr];
                    ds += regc * XD[uD[rr] * D + col];
                }
                Gp[rowD[rr] * D + col] = dp;
                Gs[rowD[rr] * D + col] = ds;
            }
        }
    }
    float* out = part + static_cast<int64_t>(blockIdx.x) * NGATE * GATE;
#pragma unroll
    for (int m = 0; m < NGATE; ++m) {
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) {
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) out[m * GATE + (wv * 16 + 4 * g + rr) * D + nb * 16 + r] = dW[m][nb][rr];
        }
    }
    if (threadIdx.x < D) {
        out[0 * GATE + D * D + threadIdx.x] = dba;
        out[1 * GATE + D * D + threadIdx.x] = dba;
        out[2 * GATE + D * D + threadIdx.x] = dbz;
        out[3 * GATE + D * D + threadIdx.x] = dbz;
    }
}

// ------------------------------------------------------------------------------------------------
// the gradient rows into the hop's table
// ------------------------------------------------------------------------------------------------
// item_at (step_common.h): position k < n of a hop's item list is pos[k], position n + b the hop's chosen item sel[b]
// order_u [n]: the positions of the user list sorted by (id, position); order_i [H + 1][2 n]: those of hop h's item list
// cat(pos, the hop's chosen items) -- a rank by counting.  blockIdx.y = hop; the user list is ranked by hop 0's blocks.
__global__ __launch_bounds__(256) void dn_rank_kernel(const int32_t* __restrict__ uids, const int32_t* __restrict__ pos,
                                                      const int32_t* __restrict__ selitem, int n, int32_t* __restrict__ order_u,
                                                      int32_t* __restrict__ order_i) {
    const int k = blockIdx.x * 256 + threadIdx.x, h = blockIdx.y;
    const int32_t* sel = selitem + static_cast<int64_t>(h) * n;
    if (k < 2 * n) {
        const int id = item_at(pos, sel, n, k);
        int rank = 0;
        for (int j = 0; j < 2 * n; ++j) {
            const int o = item_at(pos, sel, n, j);
            rank += (o < id || (o == id && j < k)) ? 1 : 0;
        }
        order_i[static_cast<int64_t>(h) * 2 * n + rank] = k;
    } else if (k < 3 * n && h == 0) {
        const int kk = k - 2 * n;
        const int id = uids[kk];
        int rank = 0;
        for (int j = 0; j < n; ++j) {
            const int o = uids[j];
            rank += (o < id || (o == id && j < kk)) ? 1 : 0;
        }
        order_u[rank] = kk;
    }
}

// G_h[id] = the sum of the hop's gradient rows whose list entry is id, in rank order, by the wavefront of the id's first rank:
// one writer per distinct id (the table was cleared).  blockIdx.y = hop; blocks [0, blocks_u) walk the user list.
struct GradTables { float* g[MAXH + 1]; };
__global__ __launch_bounds__(HW * 64) void dn_seg_add_kernel(GradTables G, const int32_t* __restrict__ uids, const int32_t* __restrict__ pos,
                                                             const int32_t* __restrict__ selitem, const int32_t* __restrict__ order_u,
                                                             const int32_t* __restrict__ order_i, int n, int U, int I, int blocks_u,
                                                             const float* __restrict__ Gs, const float* __restrict__ Gp,
                                                             const float* __restrict__ Gc) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, h = blockIdx.y;
    const bool user = static_cast<int>(blockIdx.x) < blocks_u;
    const int rk = (user ? blockIdx.x : blockIdx.x - blocks_u) * HW + wv;
    const int cnt = user ? n : 2 * n, limit = user ? U : I;
    if (rk >= cnt) return;
    const int32_t* sel = selitem + static_cast<int64_t>(h) * n;
    const int32_t* order = user ? order_u : order_i + static_cast<int64_t>(h) * 2 * n;
    const int first = order[rk];
    const int id = user ? uids[first] : item_at(pos, sel, n, first);
    if (id < 0 || id >= limit) return;
    if (rk > 0) {
        const int prev = order[rk - 1];
        if ((user ? uids[prev] : item_at(pos, sel, n, prev)) == id) return;
    }
    const int64_t base = static_cast<int64_t>(h) * n;
    float acc = 0.0f;
    for (int k = rk; k < cnt; ++k) {
        const int o = order[k];
        if ((user ? uids[o] : item_at(pos, sel, n, o)) != id) break;
        const float* src = user ? Gs + (base + o) * D : (o < n ? Gp + (base + o) * D : Gc + (base + o - n) * D);
        acc += src[lane];
    }
    float* dst = (h == 0 ? G.g[0] : h == 1 ? G.g[1] : h == 2 ? G.g[2] : G.g[3]) + (user ? 0 : static_cast<int64_t>(U) * D);
    dst[static_cast<int64_t>(id) * D + lane] = acc;
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
struct StepLayout {            // float offsets into the step's workspace
    int64_t gp, gn, PG, Gs, Gp, Gc, lossb, part, selitem, ordu, ordi, total;
};

inline int back_workgroups(int n, int H) {
    const int64_t chunks = (static_cast<int64_t>(n) * (H + 1) + TB - 1) / TB;
    return static_cast<int>(chunks < MAX_WG ? chunks : MAX_WG);
}

inline StepLayout step_layout(int n, int H) {
    StepLayout L;
    const int64_t n4 = round4(n), R = n4 * (H + 1);
    int64_t o = 0;
    L.gp = o; o += R * D;
    L.gn = o; o += R * D;
    L.PG = o; o += 5 * n4 * D;
    L.Gs = o; o += R * D;
    L.Gp = o; o += R * D;
    L.Gc = o; o += R * D;
    L.lossb = o; o += 3 * n4;
    L.part = o; o += static_cast<int64_t>(back_workgroups(n, H)) * NGATE * GATE;
    L.selitem = o; o += R;
    L.ordu = o; o += n4;
    L.ordi = o; o += 2 * R;
    L.total = o;
    return L;
}

int run_step(const skr_dens_step_args* a, void* stream, float* h_ms) {
    SKR_REQUIRE(a, "skr_dens_step: NULL argument");
    const int U = a->n_users, I = a->n_items, n = a->n, H = a->n_hops, K = a->n_negs;
    SKR_REQUIRE(a->params && a->uids && a->pos && a->cand && a->grad && a->loss && a->work, "skr_dens_step: NULL argument");
    SKR_REQUIRE(U > 0 && I > 0 && n >= 0 && n <= MAXB, "skr_dens_step: n_users = %d, n_items = %d, n = %d (at most %d rows)", U, I, n, MAXB);
    SKR_REQUIRE(a->dim >= 1 && a->dim <= D, "skr_dens_step: 1 <= dim <= 64 (got %d); rows are 64 floats, zero-padded", a->dim);
    SKR_REQUIRE(H >= 0 && H <= MAXH, "skr_dens_step: 0 <= n_hops <= %d (got %d)", MAXH, H);
    SKR_REQUIRE(K >= 1 && K <= MAXK, "skr_dens_step: 1 <= n_negs <= %d (got %d)", MAXK, K);
    SKR_REQUIRE(H == 0 || (a->plan_a && a->plan_at), "skr_dens_step: n_hops > 0 needs both plans");
    for (int h = 0; h < H; ++h) SKR_REQUIRE(a->hop[h], "skr_dens_step: hop table %d is NULL", h + 1);
    for (int h = 0; h <= H && H > 0; ++h) SKR_REQUIRE(a->G[h], "skr_dens_step: gradient table %d is NULL", h);
    SKR_REQUIRE(H < 2 || a->ping, "skr_dens_step: n_hops > 1 needs the ping table");
    SKR_REQUIRE(a->gamma >= 0.0f && a->l2 >= 0.0f && a->w >= 0.0f && a->w <= 1.0f, "skr_dens_step: gamma = %g, l2 = %g, w = %g", a->gamma,
                a->l2, a->w);
    if (n == 0) return SKR_OK;
    const StepLayout L = step_layout(n, H);
    SKR_REQUIRE(a->work_bytes >= static_cast<size_t>(L.total) * sizeof(float),
                "skr_dens_step: work holds %zu bytes, skr_dens_workspace(%d, %d) asks for %zu", a->work_bytes, n, H,
                static_cast<size_t>(L.total) * sizeof(float));
    uintptr_t align = reinterpret_cast<uintptr_t>(a->params) | reinterpret_cast<uintptr_t>(a->grad) | reinterpret_cast<uintptr_t>(a->work);
    for (int h = 0; h < H; ++h) align |= reinterpret_cast<uintptr_t>(a->hop[h]);
    SKR_REQUIRE((align & 15) == 0, "skr_dens_step: the tables and work must be 16-byte aligned");
    hipStream_t st = skr::as_stream(stream);
    float* w = static_cast<float*>(a->work);
    int32_t* selitem = reinterpret_cast<int32_t*>(w + L.selitem);
    int32_t* ordu = reinterpret_cast<int32_t*>(w + L.ordu);
    int32_t* ordi = reinterpret_cast<int32_t*>(w + L.ordi);
    const int64_t UO = static_cast<int64_t>(U) * D, N = static_cast<int64_t>(U) + I;
    const float* gates = a->params + N * D;
    Tables T = {};
    T.x[0] = a->params;
    for (int h = 1; h <= MAXH; ++h) T.x[h] = h <= H ? a->hop[h - 1] : a->params;
    StepTimer<SKR_DENS_GROUPS + 1> mk(h_ms, st);       // h_ms: an event after every launch group; otherwise nothing
    SKR_HIP(mk.mark());
    // ---- forward (DENS.py:125-134): X_h = A-hat X_(h-1)
    for (int h = 1; h <= H; ++h) {
        int rc = plain_run(a->plan_a, T.x[h - 1] + UO, nullptr, a->hop[h - 1], nullptr, nullptr, stream);
        if (rc != SKR_OK) return rc;
        rc = plain_run(a->plan_at, T.x[h - 1], nullptr, a->hop[h - 1] + UO, nullptr, nullptr, stream);
        if (rc != SKR_OK) return rc;
    }
    SKR_HIP(mk.mark());
    const int tiles = (n + TB - 1) / TB;
    hipLaunchKernelGGL(dn_select_kernel, dim3(tiles, H + 1), dim3(HW * 64), 0, st, T, gates, a->uids, a->pos, a->cand, a->sel_in, n, U, I,
                       H, K, a->w, w + L.gp, w + L.gn, selitem, a->sel_out);
    SKR_LAUNCH_CHECK();
    SKR_HIP(mk.mark());
    hipLaunchKernelGGL(dn_pool_kernel, dim3((n + HW - 1) / HW), dim3(HW * 64), 0, st, T, a->uids, a->pos, selitem, n, U, I, H, a->gamma,
                       w + L.gp, w + L.gn, w + L.PG, w + L.lossb);
    hipLaunchKernelGGL(dn_loss_kernel, dim3(1), dim3(1024), 0, st, w + L.lossb, n, a->gamma, a->l2, a->loss);
    SKR_LAUNCH_CHECK();
    SKR_HIP(mk.mark());
    const int n_wg = back_workgroups(n, H);
    const int chunks = static_cast<int>((static_cast<int64_t>(n) * (H + 1) + TB - 1) / TB);
    hipLaunchKernelGGL(dn_back_kernel, dim3(n_wg), dim3(HW * 64), 0, st, T, gates, a->uids, a->pos, selitem, n, U, I, H,
                       a->l2 / static_cast<float>(n), w + L.gp, w + L.gn, w + L.PG, w + L.Gs, w + L.Gp, w + L.Gc, w + L.part, chunks);
    hipLaunchKernelGGL(part_reduce_kernel<NGATE * GATE>, dim3((NGATE * GATE + 255) / 256), dim3(256), 0, st, w + L.part, n_wg, a->grad + N * D);
    SKR_LAUNCH_CHECK();
    SKR_HIP(mk.mark());
    // ---- the gradient rows into the cleared hop tables (hop 0's is the gradient itself when there is no propagation)
    GradTables G = {};
    for (int h = 0; h <= MAXH; ++h) G.g[h] = H == 0 ? a->grad : (h <= H ? a->G[h] : a->G[0]);
    for (int h = 0; h <= H; ++h) SKR_HIP(hipMemsetAsync(G.g[h], 0, static_cast<size_t>(N) * D * sizeof(float), st));
    hipLaunchKernelGGL(dn_rank_kernel, dim3((3 * n + 255) / 256, H + 1), dim3(256), 0, st, a->uids, a->pos, selitem, n, ordu, ordi);
    const int blocks_u = (n + HW - 1) / HW, blocks_i = (2 * n + HW - 1) / HW;
    hipLaunchKernelGGL(dn_seg_add_kernel, dim3(blocks_u + blocks_i, H + 1), dim3(HW * 64), 0, st, G, a->uids, a->pos, selitem, ordu, ordi, n,
                       U, I, blocks_u, w + L.Gs, w + L.Gp, w + L.Gc);
    SKR_LAUNCH_CHECK();
    SKR_HIP(mk.mark());
    // ---- backward: acc = G_H; acc = A-hat acc + G_h for h = H-1 .. 0; the last product writes the gradient of X_0
    {
        const float* X = H > 0 ? a->G[H] : nullptr;
        for (int h = H - 1; h >= 0; --h) {
            float* Y = h == 0 ? a->grad : (X == a->G[H] ? a->ping : a->G[H]);
            int rc = plain_run(a->plan_a, X + UO, a->G[h], Y, nullptr, nullptr, stream);
            if (rc != SKR_OK) return rc;
            rc = plain_run(a->plan_at, X, a->G[h] + UO, Y + UO, nullptr, nullptr, stream);
            if (rc != SKR_OK) return rc;
            X = Y;
        }
    }
    SKR_HIP(mk.mark());
    SKR_HIP(mk.finish());
    return SKR_OK;
}

}  // namespace

extern "C" {

size_t skr_dens_workspace(int n, int n_hops) {
    if (n <= 0 || n > MAXB || n_hops < 0 || n_hops > MAXH) return 0;
    return static_cast<size_t>(step_layout(n, n_hops).total) * sizeof(float);
}

int skr_dens_step(const skr_dens_step_args* args, void* stream) { return run_step(args, stream, nullptr); }

int skr_dens_step_timed(const skr_dens_step_args* args, void* stream, float* h_ms) {
    SKR_REQUIRE(h_ms != nullptr, "skr_dens_step_timed: NULL argument");
    return run_step(args, stream, h_ms);
}

}  // extern "C"
