// lightgcl.hip -- LightGCL (Simple Yet Effective Graph Contrastive Learning for Recommendation): the fused InfoNCE term,
// the low-rank (SVD) view and the batch kernel of one training step, and the host entry that issues the whole step.
//
// Replaces the stock torch ops the reference issues per step (no native code there):
//   recommender/LightGCL.py:117-137  the L propagations of both sides, the SVD view G = sum_l u_mul_s (vt E^(l-1)), the sums
//   recommender/LightGCL.py:139-150  the contrastive term: log(sum exp(G[ids] E^T / temp) + 1e-8) over ALL users / items
//                                    (dense [B, U] and [2B, I] matrices there), the clamped positive scores
//   recommender/LightGCL.py:152-169  the BPR term, the total, and autograd's backward through all of it
//
// Layout: every table has 64-float rows, zero beyond d.  Users and items share flat [U + I, 64] tables (user rows first).
// The four SVD factors are stored row-major [N, 16], zero beyond q: u_mul_s [U, 16], v_mul_s [I, 16], ut^T [U, 16],
// vt^T [I, 16] -- a node's factors are one 64-byte read.
//
// The SVD view is linear, so it folds: with S = sum_{l<L} E^(l) of the OTHER side, G_u = E_u_0 + u_mul_s (vt S_i), and only
// the batch's rows of G are read: two [q, N] x [N, 64] reductions per step and a rank-q expansion per batch row.
//
// Launches of a step (lambda1 > 0):
//   2L plan runs   E_u^(l) = A E_i^(l-1), E_i^(l) = A^T E_u^(l-1); the row epilogues keep S (layers below L) and the sum E
//   sumsq          |E_0|^2 by blocks (the l2 term's value; its gradient is the optimiser's weight decay)
//   prep           iids = cat(pos, neg); the batch's ids ranked (id, position) -> a fixed order for the duplicates
//   lowrank        T_i = vt S_i, T_u = ut S_u: row blocks, then the blocks in order
//   gather         the batch's G rows: Q_u[b] = E_u_0[u_b] + u_mul_s[u_b] T_i, Q_i[k] likewise
//   cl (x2)        pass 1 / merge / pass 2 / reduce below: lse, dQ and dE of one side, no [n, N] array
//   finish         per pair: clamped positive scores, BPR, the rows' gradient contributions, the final dQ
//   seg_add        the contributions into dE, per distinct id, in rank order
//   loss           the three loss components
//   dT, expand     dT = factor[batch]^T dQ in a fixed order; addend = dE + factor dT over all rows
//   2L plan runs   h^(l-1) = addend + A h^(l) (other side), the last one writes the gradient of E_0
//   seg_add        dQ into the gradient of E_0 at the batch's rows
//
// The InfoNCE kernels are multvae.hip's decoder passes with the roles renamed (the MFMA operand mapping is mfma_tile.h's
// k = 4 kk + g): a wavefront owns 16 query rows (the A operand of v_mfma_f32_16x16x4_f32, exact fp32), a workgroup of four a
// chunk of 64; workgroups are persistent over tiles of 64 table rows; a tile is staged in LDS once per tile and chunk.
// dE[tile] is written by the one workgroup that owns the tile (first chunk stores, later chunks add -- the same thread every
// time), dQ is per-workgroup partials added in workgroup order.
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
constexpr int QF = SKR_LIGHTGCL_MAX_Q;   // columns of a factor table
constexpr int TI = 64;         // table rows of a tile
constexpr int UC = 64;         // queries of a chunk: 16 per wavefront
constexpr int HW = 4;          // wavefronts per workgroup
constexpr int LDP = 68;        // LDS row stride (as multvae.hip)
constexpr int R_WAVES = 16;
constexpr int MAX_WG = SKR_LIGHTGCL_MAX_WG;
constexpr int MAX_N = SKR_LIGHTGCL_MAX_QUERIES;
constexpr int LR_BLOCKS = 256; // row blocks of the low-rank reductions
constexpr int SQ_BLOCKS = 1024;
constexpr float LOG_EPS = -18.420680743952367f;   // log(1e-8)

inline int n_workgroups(int n_rows) {
    const int tiles = (n_rows + TI - 1) / TI;
    return tiles < MAX_WG ? tiles : MAX_WG;
}

struct ClLayout { int64_t lse, part, dqpart, total; };   // float offsets

inline ClLayout cl_layout(int n, int n_wg) {
    ClLayout L;
    const int64_t n4 = round4(n);
    int64_t o = 0;
    L.lse = o; o += n4;
    L.part = o; o += static_cast<int64_t>(n_wg) * n4 * 2;
    L.dqpart = o; o += static_cast<int64_t>(n_wg) * n4 * D;
    L.total = o;
    return L;
}

// ------------------------------------------------------------------------------------------------
// the InfoNCE term of one side
// ------------------------------------------------------------------------------------------------
// pass 1: part[wg][query] = (max, sum exp(s - max)) over the workgroup's tiles, s = <Q, E> / temp
__global__ __launch_bounds__(HW * 64) void cl_pass1_kernel(const float* __restrict__ E, const float* __restrict__ Q, int n, int n4,
                                                           int n_rows, int tiles, float inv_temp, float* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float sW[TI * LDP];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
    int t0, t1;
    tile_range(tiles, t0, t1);
    for (int u0 = 0; u0 < n; u0 += UC) {
        const int qb = u0 + wv * 16;
        float a[16];
        load_a(a, Q, qb, n, r, g);
        float m[4], s[4];
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) { m[rr] = -INFINITY; s[rr] = 0.0f; }
        for (int t = t0; t < t1; ++t) {
            __syncthreads();
            load_tile<LDP, HW>(sW, E, t * TI, n_rows);
            __syncthreads();
            f32x4 acc[4];
            logits_tile<LDP>(acc, a, sW, r, g);
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                float v[4];
#pragma unroll
                for (int nb = 0; nb < 4; ++nb)      // rows beyond the table: exp(-inf) = 0
                    v[nb] = t * TI + nb * 16 + r < n_rows ? acc[nb][rr] * inv_temp : -INFINITY;
                const float tm = max16(fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3])));    // finite: a tile has a row
                const float mn = fmaxf(m[rr], tm);
                const float ts = sum16((expf(v[0] - mn) + expf(v[1] - mn)) + (expf(v[2] - mn) + expf(v[3] - mn)));
                s[rr] = s[rr] * expf(m[rr] - mn) + ts;
                m[rr] = mn;
            }
        }
        if (r == 0) {
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int q = qb + 4 * g + rr;
                if (q < n) {
                    float* p = part + (static_cast<int64_t>(blockIdx.x) * n4 + q) * 2;
                    p[0] = m[rr];
                    p[1] = s[rr];
                }
            }
        }
    }
}

// merge: lse_b = log(sum exp(s) + 1e-8) from the partials in workgroup order (LightGCL.py:146-147, without the overflow
// of exp(s) at s > 88 nor of exp(-max) at max < -88); loss[0] = weight * sum_b lse_b by a fixed tree
// ids (may be NULL) / limit: a query whose id is out of range is a zero row; its lse stays out of the loss
__global__ __launch_bounds__(1024) void cl_merge_kernel(const float* __restrict__ part, int n_wg, int n, int n4, float weight,
                                                        const int32_t* __restrict__ ids, int limit, float* __restrict__ lse,
                                                        float* __restrict__ loss) {
    __shared__ float s_l[1024];
    const int t = threadIdx.x;
    float tot = 0.0f;
    for (int b = t; b < n; b += 1024) {
        float M = -INFINITY;
        for (int w = 0; w < n_wg; ++w) M = fmaxf(M, part[(static_cast<int64_t>(w) * n4 + b) * 2]);
        float S = 0.0f;
        for (int w = 0; w < n_wg; ++w) {
            const float* p = part + (static_cast<int64_t>(w) * n4 + b) * 2;
            S += p[1] * expf(p[0] - M);
        }
        const float M2 = fmaxf(M, LOG_EPS);
        const float l = M2 + logf(S * expf(M - M2) + expf(LOG_EPS - M2));
        lse[b] = l;
        if (ids == nullptr || (ids[b] >= 0 && ids[b] < limit)) tot += l;
    }
    s_l[t] = tot;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if (t < o) s_l[t] += s_l[t + o];
        __syncthreads();
    }
    if (t == 0) loss[0] = weight * s_l[0];
}

// pass 2: P = coef exp(s - lse) in LDS, then the dQ partial and dE[tile]
__global__ __launch_bounds__(HW * 64) void cl_pass2_kernel(const float* __restrict__ E, const float* __restrict__ Q,
                                                           const float* __restrict__ lse, int n, int n4, int n_rows, int tiles,
                                                           float inv_temp, float coef, float* __restrict__ dE,
                                                           float* __restrict__ dqpart) {
    __shared__ __attribute__((aligned(16))) float sW[TI * LDP];
    __shared__ float sG[UC * LDP];
    __shared__ float sQ[UC * LDP];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
    int t0, t1;
    tile_range(tiles, t0, t1);
    for (int u0 = 0; u0 < n; u0 += UC) {
        const int qb = u0 + wv * 16;
        __syncthreads();                                   // the previous chunk's last tile still reads sQ
        for (int idx = threadIdx.x; idx < UC * D; idx += HW * 64) {
            const int row = idx >> 6, c = idx & 63;
            sQ[row * LDP + c] = u0 + row < n ? Q[static_cast<int64_t>(u0 + row) * D + c] : 0.0f;
        }
        float a[16];
        load_a(a, Q, qb, n, r, g);
        float lsev[4];
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int q = qb + 4 * g + rr;
            lsev[rr] = q < n ? lse[q] : INFINITY;          // rows beyond the batch: exp(-inf) = 0
        }
        f32x4 dq[4];
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) dq[nb] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        for (int t = t0; t < t1; ++t) {
            const int row0 = t * TI;
            __syncthreads();                               // the previous tile's products still read sW and sG
            load_tile<LDP, HW>(sW, E, row0, n_rows);
            __syncthreads();
            f32x4 acc[4];
            logits_tile<LDP>(acc, a, sW, r, g);
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) {
                const bool in = row0 + nb * 16 + r < n_rows;
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) {
                    const float p = in ? coef * expf(acc[nb][rr] * inv_temp - lsev[rr]) : 0.0f;
                    sG[(wv * 16 + 4 * g + rr) * LDP + nb * 16 + r] = p;
                }
            }
            __syncthreads();
            // dQ[query][col] += sum_row P[query][row] E[row][col]: the wavefront's own 16 rows of P
#pragma unroll
            for (int kk = 0; kk < 16; ++kk) {
                const float ga = sG[(wv * 16 + r) * LDP + 4 * kk + g];
#pragma unroll
                for (int nb = 0; nb < 4; ++nb)
                    dq[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(ga, sW[(4 * kk + g) * LDP + nb * 16 + r], dq[nb], 0, 0, 0);
            }
            // dE[row][col] = sum_query P[query][row] Q[query][col] over the chunk: the wavefront's 16 table rows
            f32x4 dw[4];
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) dw[nb] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int kk = 0; kk < 16; ++kk) {
                const float gt = sG[(4 * kk + g) * LDP + wv * 16 + r];
#pragma unroll
                for (int nb = 0; nb < 4; ++nb)
                    dw[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(gt, sQ[(4 * kk + g) * LDP + nb * 16 + r], dw[nb], 0, 0, 0);
            }
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int row = row0 + wv * 16 + 4 * g + rr;
                if (row < n_rows) {
                    float* o = dE + static_cast<int64_t>(row) * D;
#pragma unroll
                    for (int nb = 0; nb < 4; ++nb) {
                        // the first chunk stores, the later ones add: the same thread owns the element in every chunk
                        if (u0 == 0) o[nb * 16 + r] = dw[nb][rr];
                        else o[nb * 16 + r] += dw[nb][rr];
                    }
                }
            }
        }
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int q = qb + 4 * g + rr;
            if (q < n) {
                float* p = dqpart + (static_cast<int64_t>(blockIdx.x) * n4 + q) * D;
#pragma unroll
                for (int nb = 0; nb < 4; ++nb) p[nb * 16 + r] = dq[nb][rr];
            }
        }
    }
}

// dQ = the workgroups' partials in a fixed order (as mv_reduce_kernel)
__global__ __launch_bounds__(R_WAVES * 64) void cl_reduce_kernel(const float* __restrict__ dqpart, int n_wg, int n4,
                                                                 float* __restrict__ dQ) {
    __shared__ float s_part[R_WAVES][D];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t b = blockIdx.x;
    float s = 0.0f;
    int w = wv;
    for (; w + 3 * R_WAVES < n_wg; w += 4 * R_WAVES) {
        const float a0 = dqpart[(static_cast<int64_t>(w) * n4 + b) * D + lane];
        const float a1 = dqpart[(static_cast<int64_t>(w + R_WAVES) * n4 + b) * D + lane];
        const float a2 = dqpart[(static_cast<int64_t>(w + 2 * R_WAVES) * n4 + b) * D + lane];
        const float a3 = dqpart[(static_cast<int64_t>(w + 3 * R_WAVES) * n4 + b) * D + lane];
        s += a0; s += a1; s += a2; s += a3;
    }
    for (; w < n_wg; w += R_WAVES) s += dqpart[(static_cast<int64_t>(w) * n4 + b) * D + lane];
    s_part[wv][lane] = s;
    __syncthreads();
    if (wv != 0) return;
    float t = 0.0f;
    for (int k = 0; k < R_WAVES; ++k) t += s_part[k][lane];
    dQ[b * D + lane] = t;
}

// ------------------------------------------------------------------------------------------------
// the low-rank view
// ------------------------------------------------------------------------------------------------
// part[block][q][col] = sum over the block's rows of F[row][q] S[row][col]: a wavefront walks its rows in order, the four
// wavefronts are added in order
__global__ __launch_bounds__(HW * 64) void lr_partial_kernel(const float* __restrict__ F, const float* __restrict__ S, int n_rows,
                                                             float* __restrict__ part) {
    __shared__ float s_acc[HW][QF][D];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t r0 = static_cast<int64_t>(blockIdx.x) * n_rows / gridDim.x, r1 = static_cast<int64_t>(blockIdx.x + 1) * n_rows / gridDim.x;
    float acc[QF];
#pragma unroll
    for (int q = 0; q < QF; ++q) acc[q] = 0.0f;
    for (int64_t row = r0 + wv; row < r1; row += HW) {
        const float s = S[row * D + lane];
        const float4* f4 = reinterpret_cast<const float4*>(F + row * QF);
#pragma unroll
        for (int q4 = 0; q4 < QF / 4; ++q4) {
            const float4 f = f4[q4];
            acc[4 * q4 + 0] = fmaf(f.x, s, acc[4 * q4 + 0]);
            acc[4 * q4 + 1] = fmaf(f.y, s, acc[4 * q4 + 1]);
            acc[4 * q4 + 2] = fmaf(f.z, s, acc[4 * q4 + 2]);
            acc[4 * q4 + 3] = fmaf(f.w, s, acc[4 * q4 + 3]);
        }
    }
#pragma unroll
    for (int q = 0; q < QF; ++q) s_acc[wv][q][lane] = acc[q];
    __syncthreads();
    for (int idx = threadIdx.x; idx < QF * D; idx += HW * 64) {
        const int q = idx >> 6, c = idx & 63;
        float t = 0.0f;
#pragma unroll
        for (int k = 0; k < HW; ++k) t += s_acc[k][q][c];
        part[static_cast<int64_t>(blockIdx.x) * QF * D + idx] = t;
    }
}

// T[q][col] = the blocks' partials by a fixed tree: 1024 threads, one per element, four strided runs added pairwise
__global__ __launch_bounds__(1024) void lr_final_kernel(const float* __restrict__ part, int n_blocks, float* __restrict__ T) {
    const int idx = threadIdx.x;
    float a[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int b = 0; b < n_blocks; ++b) a[b & 3] += part[static_cast<int64_t>(b) * QF * D + idx];
    T[idx] = (a[0] + a[1]) + (a[2] + a[3]);
}

// out[row] = base[row] + F[row] dT: q FMAs per element (dT [16][64] in registers, lane = column)
__global__ __launch_bounds__(HW * 64) void lr_expand_kernel(const float* __restrict__ F, const float* __restrict__ dT,
                                                            const float* __restrict__ base, int64_t n_rows, float* __restrict__ out) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float t[QF];
#pragma unroll
    for (int q = 0; q < QF; ++q) t[q] = dT[q * D + lane];
    for (int64_t row = static_cast<int64_t>(blockIdx.x) * HW + wv; row < n_rows; row += static_cast<int64_t>(gridDim.x) * HW) {
        float v = base[row * D + lane];
        const float4* f4 = reinterpret_cast<const float4*>(F + row * QF);
#pragma unroll
        for (int q4 = 0; q4 < QF / 4; ++q4) {
            const float4 f = f4[q4];
            v = fmaf(f.x, t[4 * q4 + 0], v);
            v = fmaf(f.y, t[4 * q4 + 1], v);
            v = fmaf(f.z, t[4 * q4 + 2], v);
            v = fmaf(f.w, t[4 * q4 + 3], v);
        }
        out[row * D + lane] = v;
    }
}

// ------------------------------------------------------------------------------------------------
// the batch
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int item_of(const int32_t* __restrict__ pos, const int32_t* __restrict__ neg, int n, int k) {
    return k < n ? pos[k] : neg[k - n];
}

// iids = cat(pos, neg); order_u / order_i: the positions of the user list [n] and of the item list [2n] sorted by
// (id, position) -- a rank by counting, n <= 2048
__global__ __launch_bounds__(256) void bk_prep_kernel(const int32_t* __restrict__ uids, const int32_t* __restrict__ pos,
                                                      const int32_t* __restrict__ neg, int n, int32_t* __restrict__ iids,
                                                      int32_t* __restrict__ order_u, int32_t* __restrict__ order_i) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k < n) {
        const int id = uids[k];
        int rank = 0;
        for (int j = 0; j < n; ++j) {
            const int o = uids[j];
            rank += (o < id || (o == id && j < k)) ? 1 : 0;
        }
        order_u[rank] = k;
    } else if (k < 3 * n) {
        const int kk = k - n;
        const int id = item_of(pos, neg, n, kk);
        iids[kk] = id;
        int rank = 0;
        for (int j = 0; j < 2 * n; ++j) {
            const int o = item_of(pos, neg, n, j);
            rank += (o < id || (o == id && j < kk)) ? 1 : 0;
        }
        order_i[rank] = kk;
    }
}

// the batch's G rows (LightGCL.py:122-133 folded): Q[k] = E_0[id] + factor[id] T; one wavefront per row, user rows first
__global__ __launch_bounds__(HW * 64) void bk_gather_kernel(const float* __restrict__ E0u, const float* __restrict__ E0i,
                                                            const float* __restrict__ Fus, const float* __restrict__ Fvs,
                                                            const float* __restrict__ Ti, const float* __restrict__ Tu,
                                                            const int32_t* __restrict__ uids, const int32_t* __restrict__ pos,
                                                            const int32_t* __restrict__ neg, int n, int n_users, int n_items,
                                                            float* __restrict__ Qu, float* __restrict__ Qi) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int k = blockIdx.x * HW + wv;
    if (k >= 3 * n) return;
    const bool user = k < n;
    const int kk = user ? k : k - n;
    const int64_t id = user ? uids[kk] : item_of(pos, neg, n, kk);
    float* out = (user ? Qu : Qi) + static_cast<int64_t>(kk) * D;
    if (id < 0 || id >= (user ? n_users : n_items)) {      // an id out of range: a zero row, skipped everywhere
        out[lane] = 0.0f;
        return;
    }
    const float* F = (user ? Fus : Fvs) + id * QF;
    const float* T = user ? Ti : Tu;
    float v = (user ? E0u : E0i)[id * D + lane];
#pragma unroll
    for (int q = 0; q < QF; ++q) v = fmaf(F[q], T[q * D + lane], v);
    out[lane] = v;
}

__device__ __forceinline__ float softplus_neg(float x) {   // -logsigmoid(x) = softplus(-x), as torch computes it
    return fmaxf(-x, 0.0f) + log1pf(expf(-fabsf(x)));
}

// per pair b: the clamped positive scores (LightGCL.py:148), the BPR term (:153-159), the rows' gradient contributions
// Cu [n] / Ci [2n] (to dE at the ids' rows) and the final dQ (the InfoNCE part is there already); one wavefront per pair
__global__ __launch_bounds__(HW * 64) void bk_finish_kernel(const float* __restrict__ Eu, const float* __restrict__ Ei,
                                                            const int32_t* __restrict__ uids, const int32_t* __restrict__ pos,
                                                            const int32_t* __restrict__ neg, int n, int n_users, int n_items,
                                                            float inv_temp, float lambda1, const float* __restrict__ Qu,
                                                            const float* __restrict__ Qi, float* __restrict__ dQu,
                                                            float* __restrict__ dQi, float* __restrict__ Cu, float* __restrict__ Ci,
                                                            float* __restrict__ s_bpr, float* __restrict__ s_posu,
                                                            float* __restrict__ s_posi) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int b = blockIdx.x * HW + wv;
    if (b >= n) return;
    const int64_t u = uids[b], p = pos[b], q = neg[b];
    const bool vu = u >= 0 && u < n_users, vp = p >= 0 && p < n_items, vq = q >= 0 && q < n_items;
    const float eu = vu ? Eu[u * D + lane] : 0.0f, ep = vp ? Ei[p * D + lane] : 0.0f, en = vq ? Ei[q * D + lane] : 0.0f;
    const float invn = 1.0f / static_cast<float>(n);
    float cu = 0.0f, cp = 0.0f, cn = 0.0f, bpr = 0.0f;
    if (vu && vp && vq) {
        const float x = skr::wave_sum(eu * ep) - skr::wave_sum(eu * en);
        bpr = softplus_neg(x);
        const float gx = -invn / (1.0f + expf(x));         // d mean(-logsigmoid(x)) / dx = -sigmoid(-x) / n
        cu = gx * (ep - en);
        cp = gx * eu;
        cn = -gx * eu;
    }
    float posu = 0.0f, posp = 0.0f, posn = 0.0f;
    if (lambda1 > 0.0f) {
        const int64_t bu = static_cast<int64_t>(b) * D + lane, bp = bu, bn = static_cast<int64_t>(n + b) * D + lane;
        const float cu1 = -lambda1 * invn * inv_temp, ci1 = 0.5f * cu1;    // the item side's mean is over 2n rows
        if (vu) {
            const float g = Qu[bu];
            const float s = skr::wave_sum(g * eu) * inv_temp;
            posu = fminf(fmaxf(s, -5.0f), 5.0f);
            if (s >= -5.0f && s <= 5.0f) {                 // the clamp passes gradient only inside its bounds
                dQu[bu] += cu1 * eu;
                cu += cu1 * g;
            }
        }
        if (vp) {
            const float g = Qi[bp];
            const float s = skr::wave_sum(g * ep) * inv_temp;
            posp = fminf(fmaxf(s, -5.0f), 5.0f);
            if (s >= -5.0f && s <= 5.0f) {
                dQi[bp] += ci1 * ep;
                cp += ci1 * g;
            }
        }
        if (vq) {
            const float g = Qi[bn];
            const float s = skr::wave_sum(g * en) * inv_temp;
            posn = fminf(fmaxf(s, -5.0f), 5.0f);
            if (s >= -5.0f && s <= 5.0f) {
                dQi[bn] += ci1 * en;
                cn += ci1 * g;
            }
        }
    }
    Cu[static_cast<int64_t>(b) * D + lane] = cu;
    Ci[static_cast<int64_t>(b) * D + lane] = cp;
    Ci[static_cast<int64_t>(n + b) * D + lane] = cn;
    if (lane == 0) {
        s_bpr[b] = bpr;
        s_posu[b] = posu;
        s_posi[b] = posp;
        s_posi[n + b] = posn;
    }
}

// dst[id] += the rows of src whose list entry is id, in rank order, by the wavefront of the id's first rank: one writer per
// distinct id.  Blocks [0, blocks_u) walk the user list, the others the item list.
__global__ __launch_bounds__(HW * 64) void bk_seg_add_kernel(const int32_t* __restrict__ uids, const int32_t* __restrict__ order_u,
                                                             int n_u, int n_users, const float* __restrict__ src_u,
                                                             float* __restrict__ dst_u, int blocks_u,
                                                             const int32_t* __restrict__ iids, const int32_t* __restrict__ order_i,
                                                             int n_i, int n_items, const float* __restrict__ src_i,
                                                             float* __restrict__ dst_i) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const bool user = static_cast<int>(blockIdx.x) < blocks_u;
    const int r = (user ? blockIdx.x : blockIdx.x - blocks_u) * HW + wv;
    const int32_t* ids = user ? uids : iids;
    const int32_t* order = user ? order_u : order_i;
    const int n = user ? n_u : n_i, limit = user ? n_users : n_items;
    if (r >= n) return;
    const int id = ids[order[r]];
    if (id < 0 || id >= limit) return;
    if (r > 0 && ids[order[r - 1]] == id) return;
    const float* src = user ? src_u : src_i;
    float acc = 0.0f;
    for (int k = r; k < n; ++k) {
        const int o = order[k];
        if (ids[o] != id) break;
        acc += src[static_cast<int64_t>(o) * D + lane];
    }
    float* dst = (user ? dst_u : dst_i) + static_cast<int64_t>(id) * D;
    dst[lane] += acc;
}

// dT[side][q][col] = sum_k factor[id_k][q] dQ[k][col]: block (side, q), 16 wavefronts strided over k, added in order
__global__ __launch_bounds__(R_WAVES * 64) void bk_dt_kernel(const float* __restrict__ Fus, const float* __restrict__ Fvs,
                                                             const int32_t* __restrict__ uids, const int32_t* __restrict__ iids,
                                                             int n, int n_users, int n_items, const float* __restrict__ dQu,
                                                             const float* __restrict__ dQi, float* __restrict__ dTi,
                                                             float* __restrict__ dTu) {
    __shared__ float s_part[R_WAVES][D];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const bool user = blockIdx.x < QF;                      // the user list feeds dT_i = u_mul_s[batch]^T dQ_u
    const int q = user ? blockIdx.x : blockIdx.x - QF;
    const int cnt = user ? n : 2 * n, limit = user ? n_users : n_items;
    const int32_t* ids = user ? uids : iids;
    const float* F = user ? Fus : Fvs;
    const float* dQ = user ? dQu : dQi;
    float acc = 0.0f;
    for (int k = wv; k < cnt; k += R_WAVES) {
        const int64_t id = ids[k];
        if (id < 0 || id >= limit) continue;
        acc = fmaf(F[id * QF + q], dQ[static_cast<int64_t>(k) * D + lane], acc);
    }
    s_part[wv][lane] = acc;
    __syncthreads();
    if (wv != 0) return;
    float t = 0.0f;
    for (int k = 0; k < R_WAVES; ++k) t += s_part[k][lane];
    (user ? dTi : dTu)[q * D + lane] = t;
}

// part[block] = the sum of squares of the block's stretch of x (fixed tree)
__global__ __launch_bounds__(256) void sumsq_kernel(const float* __restrict__ x, int64_t n, float* __restrict__ part) {
    __shared__ float s[256];
    const int64_t i0 = static_cast<int64_t>(blockIdx.x) * n / gridDim.x, i1 = static_cast<int64_t>(blockIdx.x + 1) * n / gridDim.x;
    float a = 0.0f;
    for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) a = fmaf(x[i], x[i], a);
    s[threadIdx.x] = a;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (static_cast<int>(threadIdx.x) < o) s[threadIdx.x] += s[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = s[0];
}

// loss[0] = the BPR mean, loss[1] = lambda1 (neg_score - pos_score), loss[2] = lambda2 |E_0|^2, loss[3] = their sum
// (LightGCL.py:149-168); cl_loss[0 / 1] = lambda1 * the mean lse of the user / item side
__global__ __launch_bounds__(1024) void bk_loss_kernel(const float* __restrict__ s_bpr, const float* __restrict__ s_posu,
                                                       const float* __restrict__ s_posi, int n, float lambda1, float lambda2,
                                                       const float* __restrict__ cl_loss, const float* __restrict__ sq_part,
                                                       float* __restrict__ loss) {
    __shared__ float s[1024];
    const int t = threadIdx.x;
    float a = 0.0f, pu = 0.0f, pi = 0.0f, sq = 0.0f;
    for (int k = t; k < n; k += 1024) { a += s_bpr[k]; pu += s_posu[k]; }
    for (int k = t; k < 2 * n; k += 1024) pi += s_posi[k];
    for (int k = t; k < SQ_BLOCKS; k += 1024) sq += sq_part[k];
    const float bpr = block_sum_1024(a, s) / static_cast<float>(n);
    const float posu = block_sum_1024(pu, s) / static_cast<float>(n);
    const float posi = block_sum_1024(pi, s) / static_cast<float>(2 * n);
    const float sqs = block_sum_1024(sq, s);
    if (t == 0) {
        const float cl = lambda1 > 0.0f ? (cl_loss[0] + cl_loss[1]) - lambda1 * (posu + posi) : 0.0f;
        const float reg = lambda2 * sqs;
        loss[0] = bpr;
        loss[1] = cl;
        loss[2] = reg;
        loss[3] = (bpr + cl) + reg;
    }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
using Timer = StepTimer<SKR_LIGHTGCL_GROUPS + 1>;   // h_ms: an event after every launch group; otherwise nothing

// the launches of one side's InfoNCE term; mk (may be NULL) gets a mark behind pass 1 + merge and one behind pass 2 + reduce
int cl_run(const float* d_Q, int n, const float* d_E, int n_rows, float inv_temp, float weight, const int32_t* ids, float* d_dQ,
           float* d_dE, float* d_loss, float* w, hipStream_t st, Timer* mk) {
    const int n_wg = n_workgroups(n_rows), tiles = (n_rows + TI - 1) / TI, n4 = static_cast<int>(round4(n));
    const ClLayout L = cl_layout(n, n_wg);
    hipLaunchKernelGGL(cl_pass1_kernel, dim3(n_wg), dim3(HW * 64), 0, st, d_E, d_Q, n, n4, n_rows, tiles, inv_temp, w + L.part);
    hipLaunchKernelGGL(cl_merge_kernel, dim3(1), dim3(1024), 0, st, w + L.part, n_wg, n, n4, weight, ids, n_rows, w + L.lse, d_loss);
    if (mk) SKR_HIP(mk->mark());
    hipLaunchKernelGGL(cl_pass2_kernel, dim3(n_wg), dim3(HW * 64), 0, st, d_E, d_Q, w + L.lse, n, n4, n_rows, tiles, inv_temp,
                       weight * inv_temp, d_dE, w + L.dqpart);
    hipLaunchKernelGGL(cl_reduce_kernel, dim3(n), dim3(R_WAVES * 64), 0, st, w + L.dqpart, n_wg, n4, d_dQ);
    if (mk) SKR_HIP(mk->mark());
    SKR_LAUNCH_CHECK();
    return SKR_OK;
}

struct StepLayout {            // float offsets into the step's workspace
    int64_t T, dT, lrpart, Qu, Qi, dQu, dQi, Cu, Ci, sbpr, sposu, sposi, clloss, sqpart, iids, ordu, ordi, cl, total;
};

inline StepLayout step_layout(int n, int n_users, int n_items) {
    StepLayout L;
    const int64_t n4 = round4(n);
    int64_t o = 0;
    L.T = o; o += 2 * QF * D;
    L.dT = o; o += 2 * QF * D;
    L.lrpart = o; o += static_cast<int64_t>(LR_BLOCKS) * QF * D;
    L.Qu = o; o += n4 * D;
    L.Qi = o; o += 2 * n4 * D;
    L.dQu = o; o += n4 * D;
    L.dQi = o; o += 2 * n4 * D;
    L.Cu = o; o += n4 * D;
    L.Ci = o; o += 2 * n4 * D;
    L.sbpr = o; o += n4;
    L.sposu = o; o += n4;
    L.sposi = o; o += 2 * n4;
    L.clloss = o; o += 4;
    L.sqpart = o; o += SQ_BLOCKS;
    L.iids = o; o += 2 * n4;
    L.ordu = o; o += n4;
    L.ordi = o; o += 2 * n4;
    L.cl = o;
    const int64_t a = cl_layout(n, n_workgroups(n_users)).total, b = cl_layout(2 * n, n_workgroups(n_items)).total;
    o += a > b ? a : b;
    L.total = o;
    return L;
}

int run_step(const skr_lightgcl_step_args* a, void* stream, float* h_ms) {
    SKR_REQUIRE(a, "skr_lightgcl_step: NULL argument");
    const int U = a->n_users, I = a->n_items, n = a->n, Ly = a->n_layers;
    SKR_REQUIRE(a->plan_a && a->plan_at && a->E0 && a->uids && a->pos && a->neg && a->sum && a->gsum && a->grad && a->loss && a->work,
                "skr_lightgcl_step: NULL argument");
    SKR_REQUIRE(U > 0 && I > 0 && n >= 0 && n <= MAX_N / 2, "skr_lightgcl_step: n_users = %d, n_items = %d, n = %d (at most %d pairs)",
                U, I, n, MAX_N / 2);
    SKR_REQUIRE(a->dim >= 1 && a->dim <= D, "skr_lightgcl_step: 1 <= dim <= 64 (got %d); rows are 64 floats, zero-padded", a->dim);
    SKR_REQUIRE(Ly >= 1, "skr_lightgcl_step: n_layers = %d must be positive", Ly);
    SKR_REQUIRE(Ly == 1 || (a->below && a->ping[0] && a->ping[1]), "skr_lightgcl_step: n_layers > 1 needs below and both ping tables");
    SKR_REQUIRE(a->inv_temp > 0.0f && a->lambda1 >= 0.0f && a->lambda2 >= 0.0f, "skr_lightgcl_step: inv_temp = %g, lambda1 = %g, lambda2 = %g",
                a->inv_temp, a->lambda1, a->lambda2);
    const bool cl = a->lambda1 > 0.0f;
    SKR_REQUIRE(!cl || (a->q >= 1 && a->q <= QF && a->fac_us && a->fac_vs && a->fac_ut && a->fac_vt && a->addend),
                "skr_lightgcl_step: lambda1 > 0 needs the four factor tables, 1 <= q <= %d (got %d) and the addend table", QF, a->q);
    if (n == 0) return SKR_OK;
    const StepLayout L = step_layout(n, U, I);
    SKR_REQUIRE(a->work_bytes >= static_cast<size_t>(L.total) * sizeof(float),
                "skr_lightgcl_step: work holds %zu bytes, skr_lightgcl_workspace(%d, %d, %d) asks for %zu", a->work_bytes, n, U, I,
                static_cast<size_t>(L.total) * sizeof(float));
    const uintptr_t align = reinterpret_cast<uintptr_t>(a->E0) | reinterpret_cast<uintptr_t>(a->sum) | reinterpret_cast<uintptr_t>(a->work) |
                            reinterpret_cast<uintptr_t>(a->fac_us) | reinterpret_cast<uintptr_t>(a->fac_vs) |
                            reinterpret_cast<uintptr_t>(a->fac_ut) | reinterpret_cast<uintptr_t>(a->fac_vt);
    SKR_REQUIRE((align & 15) == 0, "skr_lightgcl_step: the tables and work must be 16-byte aligned");
    hipStream_t st = skr::as_stream(stream);
    float* w = static_cast<float*>(a->work);
    int32_t* iids = reinterpret_cast<int32_t*>(w + L.iids);
    int32_t* ordu = reinterpret_cast<int32_t*>(w + L.ordu);
    int32_t* ordi = reinterpret_cast<int32_t*>(w + L.ordi);
    const int64_t UO = static_cast<int64_t>(U) * D;          // the item rows' offset in a flat table
    const int64_t N = static_cast<int64_t>(U) + I;
    Timer mk(h_ms, st);
    SKR_HIP(mk.mark());
    // ---- forward (LightGCL.py:117-137): layer l reads layer l - 1 of the other side; below = sum_{l<L}, sum = sum_{l<=L}
    const float* below = Ly == 1 ? a->E0 : a->below;
    {
        const float* X = a->E0;
        for (int l = 1; l <= Ly; ++l) {
            const bool last = l == Ly;
            float* Y = last ? nullptr : a->ping[(l - 1) & 1];
            float* acc = last ? a->sum : a->below;
            const float* base = last ? below : (l == 1 ? a->E0 : nullptr);
            int rc = plain_run(a->plan_a, X + UO, nullptr, Y, acc, base, stream);
            if (rc != SKR_OK) return rc;
            rc = plain_run(a->plan_at, X, nullptr, Y ? Y + UO : nullptr, acc + UO, base ? base + UO : nullptr, stream);
            if (rc != SKR_OK) return rc;
            X = Y;
        }
    }
    SKR_HIP(mk.mark());
    hipLaunchKernelGGL(sumsq_kernel, dim3(SQ_BLOCKS), dim3(256), 0, st, a->E0, N * D, w + L.sqpart);
    hipLaunchKernelGGL(bk_prep_kernel, dim3((3 * n + 255) / 256), dim3(256), 0, st, a->uids, a->pos, a->neg, n, iids, ordu, ordi);
    float* Ti = w + L.T;                                     // vt S_i
    float* Tu = w + L.T + QF * D;                            // ut S_u
    float* dTi = w + L.dT;
    float* dTu = w + L.dT + QF * D;
    if (cl) {
        const int bi = I < LR_BLOCKS ? I : LR_BLOCKS, bu = U < LR_BLOCKS ? U : LR_BLOCKS;
        hipLaunchKernelGGL(lr_partial_kernel, dim3(bi), dim3(HW * 64), 0, st, a->fac_vt, below + UO, I, w + L.lrpart);
        hipLaunchKernelGGL(lr_final_kernel, dim3(1), dim3(1024), 0, st, w + L.lrpart, bi, Ti);
        hipLaunchKernelGGL(lr_partial_kernel, dim3(bu), dim3(HW * 64), 0, st, a->fac_ut, below, U, w + L.lrpart);
        hipLaunchKernelGGL(lr_final_kernel, dim3(1), dim3(1024), 0, st, w + L.lrpart, bu, Tu);
        hipLaunchKernelGGL(bk_gather_kernel, dim3((3 * n + HW - 1) / HW), dim3(HW * 64), 0, st, a->E0, a->E0 + UO, a->fac_us, a->fac_vs,
                           Ti, Tu, a->uids, a->pos, a->neg, n, U, I, w + L.Qu, w + L.Qi);
        SKR_LAUNCH_CHECK();
        SKR_HIP(mk.mark());
        // LightGCL.py:146-147: the mean over the n users, resp. the 2n items, times lambda1
        int rc = cl_run(w + L.Qu, n, a->sum, U, a->inv_temp, a->lambda1 / static_cast<float>(n), a->uids, w + L.dQu, a->gsum, w + L.clloss,
                        w + L.cl, st, &mk);
        if (rc != SKR_OK) return rc;
        rc = cl_run(w + L.Qi, 2 * n, a->sum + UO, I, a->inv_temp, a->lambda1 / static_cast<float>(2 * n), iids, w + L.dQi, a->gsum + UO,
                    w + L.clloss + 1, w + L.cl, st, &mk);
        if (rc != SKR_OK) return rc;
    } else {
        SKR_HIP(hipMemsetAsync(a->gsum, 0, static_cast<size_t>(N) * D * sizeof(float), st));
        for (int k = 0; k < 5; ++k) SKR_HIP(mk.mark());
    }
    hipLaunchKernelGGL(bk_finish_kernel, dim3((n + HW - 1) / HW), dim3(HW * 64), 0, st, a->sum, a->sum + UO, a->uids, a->pos, a->neg, n,
                       U, I, a->inv_temp, a->lambda1, w + L.Qu, w + L.Qi, w + L.dQu, w + L.dQi, w + L.Cu, w + L.Ci, w + L.sbpr,
                       w + L.sposu, w + L.sposi);
    const int blocks_u = (n + HW - 1) / HW, blocks_i = (2 * n + HW - 1) / HW;
    hipLaunchKernelGGL(bk_seg_add_kernel, dim3(blocks_u + blocks_i), dim3(HW * 64), 0, st, a->uids, ordu, n, U, w + L.Cu, a->gsum,
                       blocks_u, iids, ordi, 2 * n, I, w + L.Ci, a->gsum + UO);
    hipLaunchKernelGGL(bk_loss_kernel, dim3(1), dim3(1024), 0, st, w + L.sbpr, w + L.sposu, w + L.sposi, n, a->lambda1, a->lambda2,
                       w + L.clloss, w + L.sqpart, a->loss);
    const float* addend = a->gsum;
    if (cl) {
        hipLaunchKernelGGL(bk_dt_kernel, dim3(2 * QF), dim3(R_WAVES * 64), 0, st, a->fac_us, a->fac_vs, a->uids, iids, n, U, I,
                           w + L.dQu, w + L.dQi, dTi, dTu);
        // dS_u = ut^T dT_u, dS_i = vt^T dT_i: every layer below L of a side sees dE + dS
        const int eb_u = static_cast<int>(std::min<int64_t>((U + HW - 1) / HW, 4096)), eb_i = static_cast<int>(std::min<int64_t>((I + HW - 1) / HW, 4096));
        hipLaunchKernelGGL(lr_expand_kernel, dim3(eb_u), dim3(HW * 64), 0, st, a->fac_ut, dTu, a->gsum, static_cast<int64_t>(U), a->addend);
        hipLaunchKernelGGL(lr_expand_kernel, dim3(eb_i), dim3(HW * 64), 0, st, a->fac_vt, dTi, a->gsum + UO, static_cast<int64_t>(I),
                           a->addend + UO);
        addend = a->addend;
    }
    SKR_LAUNCH_CHECK();
    SKR_HIP(mk.mark());
    // ---- backward: h^(L) = dE; h_u^(l-1) = addend_u + A h_i^(l), h_i^(l-1) = addend_i + A^T h_u^(l); the gradient of E_0 is h^(0)
    {
        const float* H = a->gsum;
        for (int k = 1; k <= Ly; ++k) {
            float* Y = k == Ly ? a->grad : a->ping[(k - 1) & 1];
            int rc = plain_run(a->plan_a, H + UO, addend, Y, nullptr, nullptr, stream);
            if (rc != SKR_OK) return rc;
            rc = plain_run(a->plan_at, H, addend + UO, Y + UO, nullptr, nullptr, stream);
            if (rc != SKR_OK) return rc;
            H = Y;
        }
    }
    if (cl) {   // G's own E_0 term: dQ at the batch's rows
        hipLaunchKernelGGL(bk_seg_add_kernel, dim3(blocks_u + blocks_i), dim3(HW * 64), 0, st, a->uids, ordu, n, U, w + L.dQu, a->grad,
                           blocks_u, iids, ordi, 2 * n, I, w + L.dQi, a->grad + UO);
        SKR_LAUNCH_CHECK();
    }
    SKR_HIP(mk.mark());
    SKR_HIP(mk.finish());
    return SKR_OK;
}

}  // namespace

extern "C" {

size_t skr_lightgcl_cl_workspace(int n, int n_rows) {
    if (n <= 0 || n > MAX_N || n_rows <= 0) return 0;
    return static_cast<size_t>(cl_layout(n, n_workgroups(n_rows)).total) * sizeof(float);
}

int skr_lightgcl_cl(const float* d_Q, int n, const float* d_E, int n_rows, float inv_temp, float weight, float* d_dQ, float* d_dE,
                    float* d_loss, void* d_work, size_t work_bytes, void* stream) {
    SKR_REQUIRE(d_Q && d_E && d_dQ && d_dE && d_loss && d_work, "skr_lightgcl_cl: NULL argument");
    SKR_REQUIRE(n >= 0 && n <= MAX_N && n_rows > 0, "skr_lightgcl_cl: n = %d (at most %d), n_rows = %d", n, MAX_N, n_rows);
    SKR_REQUIRE(inv_temp > 0.0f, "skr_lightgcl_cl: inv_temp = %g must be positive", inv_temp);
    if (n == 0) return SKR_OK;
    const size_t need = skr_lightgcl_cl_workspace(n, n_rows);
    SKR_REQUIRE(work_bytes >= need, "skr_lightgcl_cl: d_work holds %zu bytes, skr_lightgcl_cl_workspace(%d, %d) asks for %zu", work_bytes,
                n, n_rows, need);
    SKR_REQUIRE((reinterpret_cast<uintptr_t>(d_E) & 15) == 0 && (reinterpret_cast<uintptr_t>(d_work) & 15) == 0,
                "skr_lightgcl_cl: d_E and d_work must be 16-byte aligned");
    return cl_run(d_Q, n, d_E, n_rows, inv_temp, weight, nullptr, d_dQ, d_dE, d_loss, static_cast<float*>(d_work), skr::as_stream(stream), nullptr);
}

size_t skr_lightgcl_workspace(int n, int n_users, int n_items) {
    if (n <= 0 || n > MAX_N / 2 || n_users <= 0 || n_items <= 0) return 0;
    return static_cast<size_t>(step_layout(n, n_users, n_items).total) * sizeof(float);
}

int skr_lightgcl_step(const skr_lightgcl_step_args* args, void* stream) { return run_step(args, stream, nullptr); }

int skr_lightgcl_step_timed(const skr_lightgcl_step_args* args, void* stream, float* h_ms) {
    SKR_REQUIRE(h_ms != nullptr, "skr_lightgcl_step_timed: NULL argument");
    return run_step(args, stream, h_ms);
}

}  // extern "C"
