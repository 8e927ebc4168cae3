// hgn.hip -- HGN (Hierarchical Gating Networks): one fused training step and the per-user query rows.
//
// Replaces the stock torch ops the reference issues per step and per evaluation batch (no native code there):
//   recommender/HGN.py:101-115   _forward_user: feature gate (two Linear(d, d) + sigmoid), instance gate, weighted mean
//   recommender/HGN.py:117-140   forward: b2 + <W2[t], p_u> + <W2[t], union> + sum_l <e_l, W2[t]> for the 2T targets
//   recommender/HGN.py:200-207   bpr_loss(yui, yuj).sum(), backward
//   recommender/HGN.py:147-163   predict: the same three terms against every W2 row
//
// Mapping, as seq.hip: a row of 64 floats on the 64 lanes of a wavefront (lane j owns column j), one instance per
// wavefront at a time, scores are wave reductions, row gradients are 256-byte global_atomic_add_f32 scatters.
//
// The two 64 x 64 gate matrices live in LDS for the workgroup's lifetime with a row stride of 65 floats: W x (lane j
// reads row j: address 65 j + k, bank (j + k) mod 32) and W^T y (lane k reads column k: address 65 j + k, consecutive)
// are both free of bank conflicts for ds_read_b32's 32-lane groups.  The mat-vecs run on the VALU: the other operand
// comes from v_readlane (an SGPR operand of the FMA), and a batch of 1024 is about 0.25 GFLOP -- a few microseconds of
// one wavefront per SIMD, below the launch and the latency of the row gathers; an MFMA tile of instances x L rows
// would need the rows staged and transposed in LDS to save time that is not on the critical path.
//
// The feature gate of a window position is recomputed in the backward pass instead of being kept, so L is bounded only
// by the lanes that hold the window and the instance-gate values (32).  A step is latency-bound: every row an instance
// reads is requested at its start (stage_window), not where the loops over positions and pairs use it.
//
// Shared-parameter gradients (8384 + 64 L floats: both gate matrices, the gate bias, instance_gate_item,
// instance_gate_user) are named by every instance.  They are summed in a FIXED order: per-wavefront registers over the
// wavefront's instances, the workgroup's wavefronts in order through LDS (in the matrices' place), one partial per
// workgroup in the scratch buffer, and hgn_reduce_kernel adds the partials in workgroup order.
#include "skr_common.h"

#include <cmath>

namespace {

constexpr int D = 64;
constexpr int HW = 4;                  // wavefronts per workgroup
constexpr int LDW = D + 1;             // LDS row stride of a gate matrix
constexpr int MAT = D * LDW;           // floats of one gate matrix in LDS
constexpr int G_BI = 2 * D * D, G_BU = G_BI + D, G_IGI = G_BU + D, G_IGU = G_IGI + D;

__device__ __forceinline__ void bpr_terms(float x, float& l, float& c) {
    // as seq.hip: -logsigmoid(x) in torch's form; dl/dx = -sigmoid(-x)
    const float z = expf(-fabsf(x));
    l = -(fminf(0.0f, x) - log1pf(z));
    c = -((x >= 0.0f) ? z / (1.0f + z) : 1.0f / (1.0f + z));
}

__device__ __forceinline__ float sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// the value lane l holds (l wave-uniform)
__device__ __forceinline__ float bcast(float v, int l) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}
__device__ __forceinline__ int bcast(int v, int l) { return __builtin_amdgcn_readlane(v, l); }

// lane j: sum_k M[j][k] x[k], x spread over the lanes.  One 4-byte LDS read per FMA: the mat-vecs are bound by the LDS
// read rate (measured: skr_hgn_queries moves 30 TB/s of LDS reads, 0.4 of the chip's ds_read_b32 rate).  Fully unrolled
// on purpose: with the loops rolled to eight terms per trip the query launch took 4.3 instead of 3.3 ms and the step
// 59 instead of 51 us.
__device__ __forceinline__ float matvec(const float* __restrict__ sM, float x, int lane) {
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
    const float* row = sM + lane * LDW;
#pragma unroll
    for (int k = 0; k < D; k += 4) {
        a0 = fmaf(row[k], bcast(x, k), a0);
        a1 = fmaf(row[k + 1], bcast(x, k + 1), a1);
        a2 = fmaf(row[k + 2], bcast(x, k + 2), a2);
        a3 = fmaf(row[k + 3], bcast(x, k + 3), a3);
    }
    return (a0 + a1) + (a2 + a3);
}

// lane k: sum_j M[j][k] y[j]
__device__ __forceinline__ float matvec_t(const float* __restrict__ sM, float y, int lane) {
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
    const float* col = sM + lane;
#pragma unroll
    for (int j = 0; j < D; j += 4) {
        a0 = fmaf(col[j * LDW], bcast(y, j), a0);
        a1 = fmaf(col[(j + 1) * LDW], bcast(y, j + 1), a1);
        a2 = fmaf(col[(j + 2) * LDW], bcast(y, j + 2), a2);
        a3 = fmaf(col[(j + 3) * LDW], bcast(y, j + 3), a3);
    }
    return (a0 + a1) + (a2 + a3);
}

// the two matrices into LDS: every thread's eight 16-byte loads are issued before the first store (one memory round
// trip instead of one per element; the rows' odd stride leaves 4-byte LDS stores)
__device__ __forceinline__ void load_matrices(float* __restrict__ s_mat, const float* __restrict__ gates) {
    constexpr int N4 = 2 * D * D / 4 / (HW * 64);
    const float4* g4 = reinterpret_cast<const float4*>(gates);
    float4 r[N4];
#pragma unroll
    for (int i = 0; i < N4; ++i) r[i] = g4[threadIdx.x + i * HW * 64];
#pragma unroll
    for (int i = 0; i < N4; ++i) {
        const int idx = 4 * (threadIdx.x + i * HW * 64);
        const int m = idx >> 12, j = (idx >> 6) & 63, k = idx & 63;
        float* dst = s_mat + m * MAT + j * LDW + k;
        dst[0] = r[i].x; dst[1] = r[i].y; dst[2] = r[i].z; dst[3] = r[i].w;
    }
}

// what the forward pass of one user leaves behind, per lane
struct Fwd {
    float p;       // user row
    float hu;      // (Wu p + bu) + bi: the part of the feature gate's argument that does not depend on the position
    float pu;      // lane l < L: (p^T instance_gate_user)_l
    float aval;    // lane l < L: the instance gate a_l
    float num;     // sum_l a_l g_l
    float den;     // sum_l a_l (pad positions count: HGN.py:114)
    float sum_e;   // sum_l e_l
};

// The window's item rows, all requested before the first is used: a rolled loop of load-then-use is a chain of L memory
// round trips (measured: 45 us per batch of 1024 against 7 of arithmetic).  Lane j keeps column j of the first STAGE
// rows in LDS words only it reads and writes (registers cannot be indexed by a runtime position); rows of longer
// windows come from global memory when their turn comes.  The padding row reads as zeros.
constexpr int STAGE = 16;

__device__ __forceinline__ void stage_window(float* __restrict__ se, const float* __restrict__ E, int seqv, int L, int pad,
                                             int lane) {
    const int Ls = L < STAGE ? L : STAGE;
    for (int l0 = 0; l0 < Ls; l0 += 8) {
        float r[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int s = l0 + i < Ls ? bcast(seqv, l0 + i) : pad;
            r[i] = (l0 + i < Ls && s != pad) ? E[static_cast<int64_t>(s) * D + lane] : 0.0f;
        }
#pragma unroll
        for (int i = 0; i < 8; ++i)
            if (l0 + i < Ls) se[(l0 + i) * D + lane] = r[i];
    }
}

__device__ __forceinline__ float window_row(const float* __restrict__ se, const float* __restrict__ E, int l, int s, int lane) {
    return l < STAGE ? se[l * D + lane] : E[static_cast<int64_t>(s) * D + lane];
}

// _forward_user (HGN.py:101-115) of the window in `seqv` (lane l < L holds s_l), staged in `se` by stage_window
__device__ __forceinline__ void forward_user(Fwd& f, const float* __restrict__ s_mat, const float* __restrict__ se,
                                             const float* __restrict__ E, const float* __restrict__ gates, int seqv, int L,
                                             int pad, int lane) {
    const float wi = gates[G_IGI + lane];
    f.hu = matvec(s_mat + MAT, f.p, lane) + (gates[G_BU + lane] + gates[G_BI + lane]);
    f.pu = 0.0f;
    for (int l = 0; l < L; ++l) {
        const float t = skr::wave_sum(f.p * gates[G_IGU + l * D + lane]);
        if (lane == l) f.pu = t;
    }
    f.aval = f.num = f.den = f.sum_e = 0.0f;
    for (int l = 0; l < L; ++l) {
        const int s = bcast(seqv, l);
        float g = 0.0f, dot = 0.0f;
        if (s != pad) {
            const float e = window_row(se, E, l, s, lane);
            g = e * sigmoid(f.hu + matvec(s_mat, e, lane));
            dot = skr::wave_sum(g * wi);
            f.sum_e += e;
        }
        const float a = sigmoid(dot + bcast(f.pu, l));
        f.num = fmaf(a, g, f.num);
        f.den += a;
        if (lane == l) f.aval = a;
    }
}

// ------------------------------------------------------------------------------------------------
// training step
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(HW * 64) void hgn_step_kernel(
    const float* __restrict__ U, const float* __restrict__ E, const float* __restrict__ W2, const float* __restrict__ b2,
    const float* __restrict__ gates, const int32_t* __restrict__ u_ids, const int32_t* __restrict__ seqs,
    const int32_t* __restrict__ pos, const int32_t* __restrict__ neg, int n, int n_users, int n_rows, int pad, int L, int T,
    float* __restrict__ gU, float* __restrict__ gE, float* __restrict__ gW2, float* __restrict__ gb2,
    float* __restrict__ partial, float* __restrict__ loss, int loss_slots) {
    __shared__ float s_mat[2 * MAT];                        // Wi, Wu; afterwards the workgroup's sums of their gradients
    __shared__ float s_small[2 * D + SKR_HGN_MAX_L * LDW];  // sums of the gate-bias, instance_gate_item, instance_gate_user gradients
    __shared__ float s_loss[HW];
    __shared__ float s_e[HW][STAGE * D];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float* se = s_e[wv];
    load_matrices(s_mat, gates);
    __syncthreads();
    const float wi = gates[G_IGI + lane];
    float acc_wi[D], acc_wu[D], acc_igu[D];      // dWi[lane][k], dWu[lane][k]; lane l < L: d instance_gate_user[k][l]
#pragma unroll
    for (int k = 0; k < D; ++k) acc_wi[k] = acc_wu[k] = acc_igu[k] = 0.0f;
    float acc_b = 0.0f, acc_igi = 0.0f, acc_loss = 0.0f;
    for (int b = blockIdx.x * HW + wv; b < n; b += gridDim.x * HW) {
        const int64_t u = u_ids[b];
        const int seqv = lane < L ? seqs[static_cast<int64_t>(b) * L + lane] : 0;
        const int posv = lane < T ? pos[static_cast<int64_t>(b) * T + lane] : 0;
        const int negv = lane < T ? neg[static_cast<int64_t>(b) * T + lane] : 0;
        // ids are checked by the whole wave: an instance with one out of range is skipped (it contributes nothing)
        const bool bad = seqv < 0 || seqv >= n_rows || posv < 0 || posv >= n_rows || negv < 0 || negv >= n_rows;
        if (u < 0 || u >= n_users || __builtin_amdgcn_ballot_w64(bad) != 0) continue;
        // every row the instance reads is requested here, in one round trip: the user row, the window, and the first
        // four pairs of target rows (later pairs, four at a time, while the previous four are scored)
        Fwd f;
        f.p = U[u * D + lane];
        stage_window(se, E, seqv, L, pad, lane);
        float wp[4], wn[4], bp[4], bn[4];
        auto load_pairs = [&](int k0) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int k = k0 + i < T ? k0 + i : 0;
                const int tp = bcast(posv, k), tn = bcast(negv, k);
                wp[i] = W2[static_cast<int64_t>(tp) * D + lane];
                wn[i] = W2[static_cast<int64_t>(tn) * D + lane];
                bp[i] = b2[tp];
                bn[i] = b2[tn];
            }
        };
        load_pairs(0);
        forward_user(f, s_mat, se, E, gates, seqv, L, pad, lane);
        const float uni = f.num / f.den;
        const float q = (f.p + uni) + f.sum_e;
        // the T pairs: scores, loss, and what flows back into q; W2 / b2 gradients leave at once
        float dq = 0.0f;
        for (int k0 = 0; k0 < T; k0 += 4) {
            float cs[4], dw[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float yp = skr::wave_sum(wp[i] * q) + bp[i], yn = skr::wave_sum(wn[i] * q) + bn[i];
                float lo;
                bpr_terms(yp - yn, lo, cs[i]);
                dw[i] = wp[i] - wn[i];
                if (k0 + i < T) acc_loss += lo;
            }
            if (k0 + 4 < T) load_pairs(k0 + 4);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (k0 + i >= T) continue;
                const int tp = bcast(posv, k0 + i), tn = bcast(negv, k0 + i);
                const float cc = cs[i];
                dq = fmaf(cc, dw[i], dq);
                if (tp != pad) {
                    atomicAdd(&gW2[static_cast<int64_t>(tp) * D + lane], cc * q);
                    if (lane == 0) atomicAdd(&gb2[tp], cc);
                }
                if (tn != pad) {
                    atomicAdd(&gW2[static_cast<int64_t>(tn) * D + lane], -cc * q);
                    if (lane == 0) atomicAdd(&gb2[tn], -cc);
                }
            }
        }
        // q = p + num / den + sum_l e_l
        const float dnum = dq / f.den;
        const float dden = -skr::wave_sum(dq * uni) / f.den;
        float dp = dq, dhu = 0.0f, dapv = 0.0f;
        for (int l = 0; l < L; ++l) {
            const int s = bcast(seqv, l);
            const float a = bcast(f.aval, l);
            const float igu = gates[G_IGU + l * D + lane];
            if (s == pad) {           // g_l = 0: only the instance gate's user term sees this position
                const float dapre = dden * a * (1.0f - a);
                if (lane == l) dapv = dapre;
                dp = fmaf(dapre, igu, dp);
                continue;
            }
            const float e = window_row(se, E, l, s, lane);
            const float gate = sigmoid(f.hu + matvec(s_mat, e, lane));
            const float g = e * gate;
            const float da = skr::wave_sum(dnum * g) + dden;
            const float dapre = da * a * (1.0f - a);
            if (lane == l) dapv = dapre;
            dp = fmaf(dapre, igu, dp);
            acc_igi = fmaf(dapre, g, acc_igi);
            const float dg = fmaf(dapre, wi, a * dnum);
            const float dpre = (dg * e) * (gate * (1.0f - gate));
            dhu += dpre;
#pragma unroll
            for (int k = 0; k < D; ++k) acc_wi[k] = fmaf(dpre, bcast(e, k), acc_wi[k]);
            const float de = (dq + dg * gate) + matvec_t(s_mat, dpre, lane);
            atomicAdd(&gE[static_cast<int64_t>(s) * D + lane], de);
        }
        acc_b += dhu;
#pragma unroll
        for (int k = 0; k < D; ++k) {
            const float pk = bcast(f.p, k);
            acc_wu[k] = fmaf(dhu, pk, acc_wu[k]);
            acc_igu[k] = fmaf(dapv, pk, acc_igu[k]);
        }
        dp += matvec_t(s_mat + MAT, dhu, lane);
        atomicAdd(&gU[u * D + lane], dp);
    }
    // this workgroup's partial: its wavefronts in order, in the matrices' place
    if (lane == 0) s_loss[wv] = acc_loss;
    for (int w = 0; w < HW; ++w) {
        __syncthreads();
        if (wv != w) continue;
        float* r0 = s_mat + lane * LDW;
        float* r1 = s_mat + MAT + lane * LDW;
        float* r2 = s_small + 2 * D + lane * LDW;
        if (w == 0) {
#pragma unroll
            for (int k = 0; k < D; ++k) {
                r0[k] = acc_wi[k];
                r1[k] = acc_wu[k];
                if (lane < L) r2[k] = acc_igu[k];
            }
            s_small[lane] = acc_b;
            s_small[D + lane] = acc_igi;
        } else {
#pragma unroll
            for (int k = 0; k < D; ++k) {
                r0[k] += acc_wi[k];
                r1[k] += acc_wu[k];
                if (lane < L) r2[k] += acc_igu[k];
            }
            s_small[lane] += acc_b;
            s_small[D + lane] += acc_igi;
        }
    }
    __syncthreads();
    const int ng = SKR_HGN_GATE_FLOATS(L);
    float* out = partial + static_cast<int64_t>(blockIdx.x) * ng;
    for (int idx = threadIdx.x; idx < ng; idx += HW * 64) {
        float v;
        if (idx < G_BI) {
            const int m = idx >> 12, j = (idx >> 6) & 63, k = idx & 63;
            v = s_mat[m * MAT + j * LDW + k];
        } else if (idx < G_IGI) {
            v = s_small[idx & 63];                              // the two gate biases have the same gradient
        } else if (idx < G_IGU) {
            v = s_small[D + (idx & 63)];
        } else {
            const int l = (idx - G_IGU) >> 6, k = idx & 63;     // stored [L][64]: row l = column l of instance_gate_user
            v = s_small[2 * D + l * LDW + k];
        }
        out[idx] = v;
    }
    if (threadIdx.x == 0) {
        float a = 0.0f;
        for (int w = 0; w < HW; ++w) a += s_loss[w];
        const int sl = 2 * (static_cast<int>(blockIdx.x) % loss_slots);    // as seq.hip; the l2 word stays as it is
        atomicAdd(&loss[sl], a);
    }
}

// g_gates += the workgroups' partials, 64 floats per workgroup, as transrec_t_kernel: wavefront w of R_WAVES adds the
// partials w, w + R_WAVES, ... in that order (four loads in flight), then wavefront 0 adds the R_WAVES sums in order --
// a fixed order of additions for a given number of partials.  (One thread walking all 256 partials of its float is a
// chain of 64 memory round trips: that form made the pair of launches 70 us.)
constexpr int R_WAVES = 16;

__global__ __launch_bounds__(R_WAVES * 64) void hgn_reduce_kernel(const float* __restrict__ partial, int n_parts, int ng,
                                                                  float* __restrict__ g_gates) {
    __shared__ float s_part[R_WAVES][D];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int idx = blockIdx.x * D + lane;
    float s = 0.0f;
    if (idx < ng) {
        int g = wv;
        for (; g + 3 * R_WAVES < n_parts; g += 4 * R_WAVES) {
            const float a0 = partial[static_cast<int64_t>(g) * ng + idx];
            const float a1 = partial[static_cast<int64_t>(g + R_WAVES) * ng + idx];
            const float a2 = partial[static_cast<int64_t>(g + 2 * R_WAVES) * ng + idx];
            const float a3 = partial[static_cast<int64_t>(g + 3 * R_WAVES) * ng + idx];
            s += a0; s += a1; s += a2; s += a3;
        }
        for (; g < n_parts; g += R_WAVES) s += partial[static_cast<int64_t>(g) * ng + idx];
    }
    s_part[wv][lane] = s;
    __syncthreads();
    if (wv != 0 || idx >= ng) return;
    float t = 0.0f;
    for (int w = 0; w < R_WAVES; ++w) t += s_part[w][lane];
    g_gates[idx] += t;
}

// ------------------------------------------------------------------------------------------------
// query rows: Q[u] = p_u + union(u) + sum_l e_{s_l}
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(HW * 64) void hgn_queries_kernel(
    const float* __restrict__ U, const float* __restrict__ E, const float* __restrict__ gates,
    const int32_t* __restrict__ users, const int32_t* __restrict__ windows, int n, int n_users, int n_rows, int pad, int L,
    float* __restrict__ Q) {
    __shared__ float s_mat[2 * MAT];
    __shared__ float s_e[HW][STAGE * D];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float* se = s_e[wv];
    load_matrices(s_mat, gates);
    __syncthreads();
    for (int b = blockIdx.x * HW + wv; b < n; b += gridDim.x * HW) {
        const int64_t u = users ? users[b] : b;
        if (u < 0 || u >= n_users) continue;
        const int seqv = lane < L ? windows[static_cast<int64_t>(b) * L + lane] : 0;
        // a window that starts with a negative entry: a user without training history
        if (__builtin_amdgcn_ballot_w64(seqv < 0 || seqv >= n_rows) != 0) {
            Q[u * D + lane] = __builtin_nanf("");
            continue;
        }
        Fwd f;
        f.p = U[u * D + lane];
        stage_window(se, E, seqv, L, pad, lane);
        forward_user(f, s_mat, se, E, gates, seqv, L, pad, lane);
        Q[u * D + lane] = (f.p + f.num / f.den) + f.sum_e;
    }
}

}  // namespace

extern "C" {

int skr_hgn_step(const float* d_U, const float* d_E, const float* d_W2, const float* d_b2, const float* d_gates,
                 const int32_t* d_u, const int32_t* d_seq, const int32_t* d_pos, const int32_t* d_neg, int n, int n_users,
                 int n_rows, int pad_idx, int dim, int seq_L, int seq_T, float* d_gU, float* d_gE, float* d_gW2, float* d_gb2,
                 float* d_ggates, float* d_work, float* d_loss, int loss_slots, void* stream) {
    SKR_REQUIRE(d_U && d_E && d_W2 && d_b2 && d_gates && d_u && d_seq && d_pos && d_neg && d_gU && d_gE && d_gW2 && d_gb2 &&
                    d_ggates && d_work && d_loss,
                "skr_hgn_step: NULL argument");
    SKR_REQUIRE(n >= 0 && n_users > 0 && n_rows > 0, "skr_hgn_step: n = %d, n_users = %d, n_rows = %d", n, n_users, n_rows);
    SKR_REQUIRE(pad_idx >= -1 && pad_idx < n_rows, "skr_hgn_step: pad_idx = %d is not a row of the item tables (or -1)", pad_idx);
    SKR_REQUIRE(dim == D, "skr_hgn_step: dim must be 64 (got %d); pad narrower rows with zeros", dim);
    SKR_REQUIRE(seq_L >= 1 && seq_L <= SKR_HGN_MAX_L && seq_T >= 1 && seq_T <= SKR_HGN_MAX_T,
                "skr_hgn_step: need 1 <= seq_L <= %d and 1 <= seq_T <= %d (got %d, %d)", SKR_HGN_MAX_L, SKR_HGN_MAX_T, seq_L,
                seq_T);
    SKR_REQUIRE(loss_slots == 1 || loss_slots == SKR_LOSS_SLOTS, "skr_hgn_step: loss_slots must be 1 or %d", SKR_LOSS_SLOTS);
    if (n == 0) return SKR_OK;
    SKR_REQUIRE((reinterpret_cast<uintptr_t>(d_gates) & 15) == 0, "skr_hgn_step: d_gates must be 16-byte aligned");
    int blocks = (n + HW - 1) / HW;
    if (blocks > SKR_HGN_MAX_BLOCKS) blocks = SKR_HGN_MAX_BLOCKS;
    const int ng = SKR_HGN_GATE_FLOATS(seq_L);
    hipStream_t st = skr::as_stream(stream);
    hipLaunchKernelGGL(hgn_step_kernel, dim3(blocks), dim3(HW * 64), 0, st, d_U, d_E, d_W2, d_b2, d_gates, d_u, d_seq, d_pos,
                       d_neg, n, n_users, n_rows, pad_idx, seq_L, seq_T, d_gU, d_gE, d_gW2, d_gb2, d_work, d_loss, loss_slots);
    hipLaunchKernelGGL(hgn_reduce_kernel, dim3((ng + D - 1) / D), dim3(R_WAVES * 64), 0, st, d_work, blocks, ng, d_ggates);
    SKR_LAUNCH_CHECK();
    return SKR_OK;
}

int skr_hgn_queries(const float* d_U, const float* d_E, const float* d_gates, const int32_t* d_users, int n,
                    const int32_t* d_windows, int n_users, int n_rows, int pad_idx, int dim, int seq_L, float* d_Q,
                    void* stream) {
    SKR_REQUIRE(d_U && d_E && d_gates && d_windows && d_Q, "skr_hgn_queries: NULL argument");
    SKR_REQUIRE(n >= 0 && n_users > 0 && n_rows > 0, "skr_hgn_queries: n = %d, n_users = %d, n_rows = %d", n, n_users, n_rows);
    SKR_REQUIRE(d_users || n <= n_users, "skr_hgn_queries: without a user list n = %d must not exceed n_users = %d", n, n_users);
    SKR_REQUIRE(pad_idx >= -1 && pad_idx < n_rows, "skr_hgn_queries: pad_idx = %d is not a row of the item table (or -1)", pad_idx);
    SKR_REQUIRE(dim == D, "skr_hgn_queries: dim must be 64 (got %d); pad narrower rows with zeros", dim);
    SKR_REQUIRE(seq_L >= 1 && seq_L <= SKR_HGN_MAX_L, "skr_hgn_queries: need 1 <= seq_L <= %d (got %d)", SKR_HGN_MAX_L, seq_L);
    if (n == 0) return SKR_OK;
    SKR_REQUIRE((reinterpret_cast<uintptr_t>(d_gates) & 15) == 0, "skr_hgn_queries: d_gates must be 16-byte aligned");
    int blocks = (n + HW - 1) / HW;
    if (blocks > 2048) blocks = 2048;      // 8 workgroups per CU: each stages the matrices once and walks its users
    hipLaunchKernelGGL(hgn_queries_kernel, dim3(blocks), dim3(HW * 64), 0, skr::as_stream(stream), d_U, d_E, d_gates, d_users,
                       d_windows, n, n_users, n_rows, pad_idx, seq_L, d_Q);
    SKR_LAUNCH_CHECK();
    return SKR_OK;
}

}  // extern "C"
