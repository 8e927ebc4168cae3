// lattice.hip -- LATTICE (Mining Latent Structures for Multimedia Recommendation, ACM MM 2021): an item-item graph that is
// LEARNED -- the kNN of the projected feature rows, normalised, mixed with the frozen graph of the raw features -- whose
// propagation of the item embeddings is normalised and added to the item rows of a LightGCN (or plain) encoder.  Here: the
// sparse assembly of the mixed graph, the sampled product that gives dLoss/dS, the hand-derived backward of the assembly
// down to the projected rows and the modal weights, the batch kernel and the host entry that issues one training step.
//
// Replaces the stock torch ops the reference issues on dense [I, I] matrices (no native code there):
//   recommender/LATTICE.py:67-85    build_sim, build_knn_neighbourhood, compute_normalized_laplacian
//   recommender/LATTICE.py:203-268  the mix of the learned and the frozen graph, n_layers torch.mm with the dense item_adj,
//                                   n_ui_layers torch.sparse.mm on the square adjacency, the mean, F.normalize
//   recommender/LATTICE.py:270-294  bpr_loss on the propagated rows, and autograd's backward through all of it
//
// Layout: see include/skrec_hip.h, section N.
//
// Launches of skr_lattice_graph:      merge<count>, scan, merge<fill> (columns, slots, L, r, q), values, tail
// Launches of skr_lattice_graph_bwd:  norms, rho, dl (+ the workgroups' dw sums), dw, cosine backward
// Launches of a step:
//   Lu plan runs     X_k = P X_(k-1) on the square adjacency; the mean M rides in the accum epilogue
//   mark, n plan runs  h_l = S h_(l-1); the last at the batch's item rows only (a build step keeps h_0 .. h_(n-1))
//   batch            one wavefront per batch row: u, p = M_i + h_i / |h_i|, q; logsigmoid, the regulariser, the rows' gradients
//                    and the gradient that enters h through the normalisation
//   part_reduce, loss
//   rank, seg_add    G = 0, dh_n = 0; one writer per distinct id (users; items into G; items into dh_n)
//   Lu plan runs     acc = G; acc = P^T acc + G; the last writes acc / (Lu + 1) into the gradient
//   n plan runs      dh_(l-1) = S^T dh_l; the last adds into the gradient's item rows
//   sddmm            a build step only: g = sum_l <dh_l[i], h_(l-1)[j]> on the entries of S
#include "skr_common.h"
#include "mfma_tile.h"
#include "step_common.h"

#include <algorithm>

namespace {

using namespace skr;

constexpr int D = 64;          // columns of every table
constexpr int HW = 4;          // wavefronts per workgroup
constexpr int MAXB = SKR_LATTICE_MAX_BATCH;
constexpr int MAXL = SKR_LATTICE_MAX_LAYERS;
constexpr int MAXK = SKR_KNN_MAX_K;
constexpr int MAXC = 4 * MAXK;  // candidates of a row
constexpr int LOSSP = 4;       // loss sums per workgroup: BPR, regulariser, unused, unused

struct Lists {                 // the four lists of a row: learned image, learned text, frozen image, frozen text
    const int32_t* ids[4];
    const float* val[4];
};

inline size_t round16(size_t x) { return (x + 15) & ~static_cast<size_t>(15); }

// ------------------------------------------------------------------------------------------------
// the graph: count, scan, fill, values
// ------------------------------------------------------------------------------------------------
// L of an entry of row `row` from its slots
__device__ __forceinline__ float learned_value(const Lists& ls, const int32_t* __restrict__ slots, int64_t e, int64_t row, int k, float w0,
                                               float w1) {
    const int s0 = slots[e * 4 + 0], s1 = slots[e * 4 + 1];
    const float a = s0 >= 0 && ls.val[0] ? ls.val[0][row * k + s0] : 0.0f;
    const float b = s1 >= 0 && ls.val[1] ? ls.val[1][row * k + s1] : 0.0f;
    return w0 * a + w1 * b;
}

// a wavefront per row: the row's candidates (list t, position p) = c = t k + p in LDS; a candidate is `first` when no
// earlier candidate names its column; the rank of a first candidate = the first candidates of a smaller column.
// FILL false: cnt[row] = the distinct columns.  FILL true: columns, slots, L (into val) of the row's entries, r and q.
template <bool FILL>
__global__ __launch_bounds__(HW * 64) void la_merge_kernel(Lists ls, int I, int k, const float* __restrict__ w, int32_t* __restrict__ cnt,
                                                           const int64_t* __restrict__ rowptr, int32_t* __restrict__ col,
                                                           float* __restrict__ val, int32_t* __restrict__ slots, float* __restrict__ r,
                                                           float* __restrict__ q) {
    __shared__ int32_t scol[HW][MAXC];
    __shared__ int32_t sfirst[HW][MAXC];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t row = blockIdx.x * static_cast<int64_t>(HW) + wv;
    const bool active = row < I;
    const int nc = 4 * k;
    int mycol[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int c = lane + 64 * h;
        int v = -1;
        if (active && c < nc) {
            const int t = c / k, p = c - t * k;
            if (ls.ids[t] != nullptr) {
                const int id = ls.ids[t][row * k + p];
                v = id >= 0 && id < I ? id : -1;
            }
        }
        mycol[h] = v;
        scol[wv][c] = v;
    }
    __syncthreads();
    int first[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int c = lane + 64 * h;
        int f = mycol[h] >= 0 ? 1 : 0;
        for (int o = 0; o < c && o < nc; ++o) f = scol[wv][o] == mycol[h] ? 0 : f;
        first[h] = f;
        sfirst[wv][c] = f;
    }
    __syncthreads();
    if (!FILL) {
        const int n = wave_sum(first[0] + first[1]);
        if (active && lane == 0) cnt[row] = n;
        return;
    }
    const float w0 = w[0], w1 = w[1];
    float lsum = 0.0f;
    const int64_t base = active ? rowptr[row] : 0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        if (!first[h]) continue;
        int rank = 0, sl[4] = {-1, -1, -1, -1};
        for (int o = 0; o < nc; ++o) {
            const int oc = scol[wv][o];
            rank += sfirst[wv][o] && oc < mycol[h] ? 1 : 0;
            if (oc == mycol[h]) {
                const int t = o / k;
                if (sl[t] < 0) sl[t] = o - t * k;
            }
        }
        const int64_t e = base + rank;
        col[e] = mycol[h];
#pragma unroll
        for (int t = 0; t < 4; ++t) slots[e * 4 + t] = sl[t];
        const float a = sl[0] >= 0 ? ls.val[0][row * k + sl[0]] : 0.0f;
        const float b = sl[1] >= 0 ? ls.val[1][row * k + sl[1]] : 0.0f;
        const float L = w0 * a + w1 * b;
        val[e] = L;
        lsum += L;
    }
    lsum = wave_sum(lsum);
    if (active && lane == 0) {
        r[row] = lsum;
        q[row] = lsum > 0.0f ? static_cast<float>(1.0 / sqrt(static_cast<double>(lsum))) : 0.0f;
    }
}

// out [n + 1] = the exclusive prefix sums of cnt [n] and their total: one workgroup walks the array 1024 at a time
// (freedom.hip's fd_scan_kernel, which lives in that file's unnamed namespace)
__global__ __launch_bounds__(1024) void la_scan_kernel(const int32_t* __restrict__ cnt, int64_t n, int64_t* __restrict__ out) {
    __shared__ int64_t s[1024];
    __shared__ int64_t carry;
    const int t = threadIdx.x;
    if (t == 0) carry = 0;
    for (int64_t base = 0; base < n; base += 1024) {
        __syncthreads();
        const int64_t v = base + t < n ? static_cast<int64_t>(cnt[base + t]) : 0;
        s[t] = v;
        __syncthreads();
        for (int o = 1; o < 1024; o <<= 1) {
            const int64_t a = t >= o ? s[t - o] : 0;
            __syncthreads();
            s[t] += a;
            __syncthreads();
        }
        const int64_t c = carry;
        if (base + t < n) out[base + t] = c + s[t] - v;
        __syncthreads();
        if (t == 1023) carry = c + s[1023];
    }
    __syncthreads();
    if (t == 0) out[n] = carry;
}

// a wavefront per row: val[e] = (1 - lam) (q_i L_e) q_j + lam (w0 O_v + w1 O_t), L_e as the fill left it in val
__global__ __launch_bounds__(HW * 64) void la_values_kernel(Lists ls, int I, int k, const float* __restrict__ w, float oml, float lam,
                                                            const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                            const int32_t* __restrict__ slots, const float* __restrict__ q,
                                                            float* __restrict__ val) {
    const int lane = threadIdx.x & 63;
    const int64_t row = blockIdx.x * static_cast<int64_t>(HW) + (threadIdx.x >> 6);
    if (row >= I) return;
    const float w0 = w[0], w1 = w[1], qi = q[row];
    for (int64_t e = rowptr[row] + lane; e < rowptr[row + 1]; e += 64) {
        const int s2 = slots[e * 4 + 2], s3 = slots[e * 4 + 3];
        const float ov = s2 >= 0 ? ls.val[2][row * k + s2] : 0.0f;
        const float ot = s3 >= 0 ? ls.val[3][row * k + s3] : 0.0f;
        const float learned = (qi * val[e]) * q[col[e]];
        const float frozen = w0 * ov + w1 * ot;
        val[e] = oml * learned + lam * frozen;
    }
}

// the entries beyond the last one: column 0, value 0, slots -1
__global__ __launch_bounds__(256) void la_tail_kernel(const int64_t* __restrict__ rowptr, int I, int64_t cap, int32_t* __restrict__ col,
                                                      float* __restrict__ val, int32_t* __restrict__ slots) {
    const int64_t nnz = rowptr[I];
    for (int64_t e = nnz + blockIdx.x * static_cast<int64_t>(256) + threadIdx.x; e < cap; e += static_cast<int64_t>(gridDim.x) * 256) {
        col[e] = 0;
        val[e] = 0.0f;
#pragma unroll
        for (int t = 0; t < 4; ++t) slots[e * 4 + t] = -1;
    }
}

// ------------------------------------------------------------------------------------------------
// the sampled product
// ------------------------------------------------------------------------------------------------
// a wavefront per row; 16 lanes per entry, four entries side by side: a lane holds 4 columns of the row of A
__global__ __launch_bounds__(HW * 64) void la_sddmm_kernel(int n_rows, int n_cols, const int64_t* __restrict__ rowptr,
                                                           const int32_t* __restrict__ col, const float* __restrict__ A, int64_t sa,
                                                           const float* __restrict__ B, int64_t sb, int nl,
                                                           const uint8_t* __restrict__ mask, int accumulate, float* __restrict__ g) {
    const int lane = threadIdx.x & 63, r = lane & 15, gq = lane >> 4;
    const int64_t row = blockIdx.x * static_cast<int64_t>(HW) + (threadIdx.x >> 6);
    if (row >= n_rows) return;
    const int64_t beg = rowptr[row], end = rowptr[row + 1];
    if (mask != nullptr && mask[row] == 0) {
        if (!accumulate) {
            for (int64_t e = beg + lane; e < end; e += 64) g[e] = 0.0f;
        }
        return;
    }
    float4 a[MAXL];
#pragma unroll
    for (int l = 0; l < MAXL; ++l) {
        a[l] = l < nl ? *reinterpret_cast<const float4*>(A + l * sa + row * D + 4 * r) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    for (int64_t e0 = beg; e0 < end; e0 += 4) {
        const int64_t e = e0 + gq;
        const bool in = e < end;
        const int64_t j = in ? checked(col[e], n_cols) : -1;
        float tot = 0.0f;
#pragma unroll
        for (int l = 0; l < MAXL; ++l) {
            if (l >= nl) break;
            float p = 0.0f;
            if (j >= 0) {
                const float4 b = *reinterpret_cast<const float4*>(B + l * sb + j * D + 4 * r);
                p = (a[l].x * b.x + a[l].y * b.y) + (a[l].z * b.z + a[l].w * b.w);
            }
            tot += sum16(p);
        }
        if (in && r == 0) g[e] = accumulate ? g[e] + tot : tot;
    }
}

// ------------------------------------------------------------------------------------------------
// the backward of the graph
// ------------------------------------------------------------------------------------------------
// invn[m][i] = 1 / max(|F_m[i]|, 1e-12): skr_knn_topk's clamp
__global__ __launch_bounds__(HW * 64) void la_norm_kernel(const float* __restrict__ F0, const float* __restrict__ F1, int I,
                                                          float* __restrict__ invn) {
    const int lane = threadIdx.x & 63;
    const int64_t row = blockIdx.x * static_cast<int64_t>(HW) + (threadIdx.x >> 6);
    if (row >= I) return;
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        const float* F = m == 0 ? F0 : F1;
        float v = 0.0f;
        if (F != nullptr) {
            const float x = F[row * D + lane];
            v = 1.0f / fmaxf(sqrtf(wave_sum(x * x)), 1e-12f);
        }
        if (lane == 0) invn[static_cast<int64_t>(m) * I + row] = v;
    }
}

struct BwdParams {
    Lists ls;
    int I, k;
    int64_t nnz;
    const float* g;
    const int64_t* rowptr;
    const int32_t* col;
    const int32_t* slots;
    const int64_t* rowptr_t;
    const int32_t* col_t;
    const int32_t* perm_t;
    const float* w;
    float oml, lam;
    const float* q;
    const float* F[2];
    float* dF[2];
    float* rho;                    // [I]
    float* dL;                     // [nnz]
    float* invn;                   // [2][I]
    float* part;                   // [gridDim.x][2]
};

// rho_i = -1/2 q_i^3 t_i: the row's entries and the column's, a lane walks its share in ascending order
__global__ __launch_bounds__(HW * 64) void la_rho_kernel(BwdParams p) {
    const int lane = threadIdx.x & 63;
    const int64_t row = blockIdx.x * static_cast<int64_t>(HW) + (threadIdx.x >> 6);
    if (row >= p.I) return;
    const float w0 = p.w[0], w1 = p.w[1];
    float t = 0.0f;
    for (int64_t e = p.rowptr[row] + lane; e < p.rowptr[row + 1]; e += 64) {
        const float a = p.oml * p.g[e];
        t += (a * learned_value(p.ls, p.slots, e, row, p.k, w0, w1)) * p.q[p.col[e]];
    }
    for (int64_t et = p.rowptr_t[row] + lane; et < p.rowptr_t[row + 1]; et += 64) {
        const int64_t e = p.perm_t[et], kk = p.col_t[et];
        if (e < 0 || e >= p.nnz || kk < 0 || kk >= p.I) continue;
        const float a = p.oml * p.g[e];
        t += (a * learned_value(p.ls, p.slots, e, kk, p.k, w0, w1)) * p.q[kk];
    }
    t = wave_sum(t);
    const float qi = p.q[row];
    if (lane == 0) p.rho[row] = -0.5f * ((qi * qi) * qi) * t;
}

// dL_e = a q_i q_j + rho_i on the learned entries, 0 elsewhere; part[wg] = the workgroup's share of dw_0 and dw_1
__global__ __launch_bounds__(HW * 64) void la_dl_kernel(BwdParams p) {
    __shared__ float s[HW][2];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t row = blockIdx.x * static_cast<int64_t>(HW) + wv;
    float d0 = 0.0f, d1 = 0.0f;
    if (row < p.I) {
        const float qi = p.q[row], rho = p.rho[row];
        for (int64_t e = p.rowptr[row] + lane; e < p.rowptr[row + 1]; e += 64) {
            const int32_t* sl = p.slots + e * 4;
            const float ge = p.g[e];
            const bool learned = sl[0] >= 0 || sl[1] >= 0;
            const float dl = learned ? ((p.oml * ge) * qi) * p.q[p.col[e]] + rho : 0.0f;
            p.dL[e] = dl;
            if (sl[0] >= 0) d0 += dl * p.ls.val[0][row * p.k + sl[0]];
            if (sl[1] >= 0) d1 += dl * p.ls.val[1][row * p.k + sl[1]];
            if (sl[2] >= 0) d0 += p.lam * (ge * p.ls.val[2][row * p.k + sl[2]]);
            if (sl[3] >= 0) d1 += p.lam * (ge * p.ls.val[3][row * p.k + sl[3]]);
        }
    }
    d0 = wave_sum(d0);
    d1 = wave_sum(d1);
    if (lane == 0) { s[wv][0] = d0; s[wv][1] = d1; }
    __syncthreads();
    if (threadIdx.x < 2) {
        const int c = threadIdx.x;
        p.part[static_cast<int64_t>(blockIdx.x) * 2 + c] = ((s[0][c] + s[1][c]) + s[2][c]) + s[3][c];
    }
}

// dw [4] = dw_0, dw_1 (the workgroups' sums in workgroup order) and the gradient of the two softmax logits
__global__ __launch_bounds__(64) void la_dw_kernel(const float* __restrict__ part, int n_wg, const float* __restrict__ w, float* __restrict__ dw) {
    if (threadIdx.x != 0) return;
    float d0 = 0.0f, d1 = 0.0f;
    for (int b = 0; b < n_wg; ++b) { d0 += part[2 * b]; d1 += part[2 * b + 1]; }
    const float mean = w[0] * d0 + w[1] * d1;
    dw[0] = d0;
    dw[1] = d1;
    dw[2] = w[0] * (d0 - mean);
    dw[3] = w[1] * (d1 - mean);
}

// dF_m[i]: a wavefront per row, a lane per column; first the row's entries, then the column's (row i of S^T), both in
// ascending order
__global__ __launch_bounds__(HW * 64) void la_cos_bwd_kernel(BwdParams p) {
    const int lane = threadIdx.x & 63;
    const int64_t row = blockIdx.x * static_cast<int64_t>(HW) + (threadIdx.x >> 6);
    if (row >= p.I) return;
    float fi[2], acc[2] = {0.0f, 0.0f}, wm[2] = {p.w[0], p.w[1]};
#pragma unroll
    for (int m = 0; m < 2; ++m) fi[m] = p.F[m] ? p.F[m][row * D + lane] * p.invn[static_cast<int64_t>(m) * p.I + row] : 0.0f;
    for (int64_t e = p.rowptr[row]; e < p.rowptr[row + 1]; ++e) {
        const float dl = p.dL[e];
        const int64_t j = p.col[e];
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const int sl = p.slots[e * 4 + m];
            if (sl < 0 || p.F[m] == nullptr) continue;
            const float ds = wm[m] * dl, s = p.ls.val[m][row * p.k + sl];
            const float fj = p.F[m][j * D + lane] * p.invn[static_cast<int64_t>(m) * p.I + j];
            acc[m] += ds * (fj - s * fi[m]);
        }
    }
    for (int64_t et = p.rowptr_t[row]; et < p.rowptr_t[row + 1]; ++et) {
        const int64_t e = p.perm_t[et], kk = p.col_t[et];
        if (e < 0 || e >= p.nnz || kk < 0 || kk >= p.I) continue;
        const float dl = p.dL[e];
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const int sl = p.slots[e * 4 + m];
            if (sl < 0 || p.F[m] == nullptr) continue;
            const float ds = wm[m] * dl, s = p.ls.val[m][kk * p.k + sl];
            const float fk = p.F[m][kk * D + lane] * p.invn[static_cast<int64_t>(m) * p.I + kk];
            acc[m] += ds * (fk - s * fi[m]);
        }
    }
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        if (p.dF[m] != nullptr) p.dF[m][row * D + lane] = acc[m] * p.invn[static_cast<int64_t>(m) * p.I + row];
    }
}

struct BwdLayout {             // byte offsets into the graph backward's workspace
    size_t rho, dL, invn, part, total;
};
inline int row_workgroups(int64_t rows) { return static_cast<int>((rows + HW - 1) / HW); }
inline BwdLayout bwd_layout(int64_t I, int64_t nnz) {
    BwdLayout L;
    size_t o = 0;
    L.rho = o; o += round16(static_cast<size_t>(I) * sizeof(float));
    L.dL = o; o += round16(static_cast<size_t>(nnz > 0 ? nnz : 1) * sizeof(float));
    L.invn = o; o += round16(static_cast<size_t>(2 * I) * sizeof(float));
    L.part = o; o += round16(static_cast<size_t>(row_workgroups(I)) * 2 * sizeof(float));
    L.total = o;
    return L;
}

// ------------------------------------------------------------------------------------------------
// the step: batch kernel, loss, ordered adds
// ------------------------------------------------------------------------------------------------
// Item list: position o < n is pos[o], position n + b is neg[b]; its rows of Gi and Hi lie at o resp. n4 + b.
struct BatchParams {
    const float* M;                // [N][64]: the user-item part
    const float* h;                // [I][64]: S^n E_items, valid at the batch's item rows
    const int32_t* users;
    const int32_t* pos;
    const int32_t* neg;
    int n, U, I;
    int64_t n4;
    float inv_n, reg;
    float* Gu;                     // [n4][64]   dLoss/du
    float* Gi;                     // [2 n4][64] dLoss/dp, then dLoss/dq
    float* Hi;                     // [2 n4][64] dLoss/dh at pos, then at neg
    float* part;                   // [gridDim.x][LOSSP]
};

// y = h / max(|h|, 1e-12) (F.normalize) -> the row M_i + y; *inv = 1 / max(|h|, 1e-12)
__device__ __forceinline__ float item_row(const BatchParams& p, int64_t i, int lane, float* y, float* inv) {
    const float hv = p.h[i * D + lane];
    *inv = 1.0f / fmaxf(sqrtf(wave_sum(hv * hv)), 1e-12f);
    *y = hv * *inv;
    return p.M[(p.U + i) * D + lane] + *y;
}

__global__ __launch_bounds__(HW * 64) void la_batch_kernel(BatchParams p) {
    __shared__ float s[HW][LOSSP];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int b = blockIdx.x * HW + wv;
    float lb = 0.0f, lr = 0.0f;
    if (b < p.n) {
        const int64_t u = checked(p.users[b], p.U), i = checked(p.pos[b], p.I), j = checked(p.neg[b], p.I);
        float gu = 0.0f, gp = 0.0f, gq = 0.0f, hp = 0.0f, hq = 0.0f;
        if (u >= 0 && i >= 0 && j >= 0) {
            float yp, yq, ip, iq;
            const float uv = p.M[u * D + lane];
            const float pv = item_row(p, i, lane, &yp, &ip), qv = item_row(p, j, lane, &yq, &iq);
            const float x = wave_sum(uv * (pv - qv));
            const float c = -sigmoid_neg(x) * p.inv_n, rn = p.reg * p.inv_n;
            lb = -log_sigmoid(x);
            lr = 0.5f * wave_sum((uv * uv + pv * pv) + qv * qv);
            gu = c * (pv - qv) + rn * uv;
            gp = c * uv + rn * pv;
            gq = rn * qv - c * uv;
            // through y = h / |h|: dh = (dy - y <y, dy>) / |h|; below the clamp y = h / 1e-12 is linear
            const bool cp = ip < 1e12f, cq = iq < 1e12f;
            const float tp = wave_sum(yp * gp), tq = wave_sum(yq * gq);
            hp = (cp ? gp - yp * tp : gp) * ip;
            hq = (cq ? gq - yq * tq : gq) * iq;
        }
        const int64_t f = static_cast<int64_t>(b) * D + lane;
        p.Gu[f] = gu;
        p.Gi[f] = gp;
        p.Gi[p.n4 * D + f] = gq;
        p.Hi[f] = hp;
        p.Hi[p.n4 * D + f] = hq;
    }
    if (lane == 0) { s[wv][0] = lb; s[wv][1] = lr; s[wv][2] = 0.0f; s[wv][3] = 0.0f; }
    __syncthreads();
    if (threadIdx.x < LOSSP) {
        const int k = threadIdx.x;
        p.part[static_cast<int64_t>(blockIdx.x) * LOSSP + k] = ((s[0][k] + s[1][k]) + s[2][k]) + s[3][k];
    }
}

// loss[0] = the BPR term, loss[1] = reg * regulariser / n, loss[2] = their sum
__global__ __launch_bounds__(64) void la_loss_kernel(const float* __restrict__ sums, int n, float reg, float* __restrict__ loss) {
    if (threadIdx.x != 0) return;
    const float fn = static_cast<float>(n);
    const float b = sums[0] / fn, r = reg * (sums[1] / fn);
    loss[0] = b;
    loss[1] = r;
    loss[2] = b + r;
}

// The BPR scalars, the pos || neg item list, the rank by counting (rank_triples_kernel) and dst += src (add_kernel) are
// step_common.h's: one text with freedom.hip and mgcn.hip.
//
// G[id] (users, items) and DHn[id] (items) = the sums of the rows whose list entry is id, in rank order, by the wavefront of
// the id's first rank: one writer per distinct id (both tables are cleared first).  Blocks [0, blocks_u) walk the user list.
__global__ __launch_bounds__(HW * 64) void la_seg_add_kernel(float* __restrict__ G, float* __restrict__ DHn, const int32_t* __restrict__ users,
                                                             const int32_t* __restrict__ pos, const int32_t* __restrict__ neg,
                                                             const int32_t* __restrict__ order_u, const int32_t* __restrict__ order_i, int n,
                                                             int64_t n4, int U, int I, int blocks_u, const float* __restrict__ Gu,
                                                             const float* __restrict__ Gi, const float* __restrict__ Hi) {
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
    float acc = 0.0f, acch = 0.0f;
    for (int k = rk; k < len; ++k) {
        const int o = order[k];
        if (id_at(o) != id) break;
        const int64_t row = user ? o : (o < n ? o : n4 + (o - n));
        acc += (user ? Gu : Gi)[row * D + lane];
        if (!user) acch += Hi[row * D + lane];
    }
    G[(static_cast<int64_t>(user ? 0 : U) + id) * D + lane] = acc;
    if (!user) DHn[static_cast<int64_t>(id) * D + lane] = acch;
}

// out_r += h_r / max(|h_r|, 1e-12): a wavefront per row
__global__ __launch_bounds__(HW * 64) void la_add_normalized_kernel(const float* __restrict__ h, int64_t n_rows, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t row = blockIdx.x * static_cast<int64_t>(HW) + (threadIdx.x >> 6);
    if (row >= n_rows) return;
    const float hv = h[row * D + lane];
    const float inv = 1.0f / fmaxf(sqrtf(wave_sum(hv * hv)), 1e-12f);
    out[row * D + lane] += hv * inv;
}

// mask[id] = 1 for the ids of pos and of neg inside [0, I)
__global__ __launch_bounds__(256) void la_mark_kernel(const int32_t* __restrict__ pos, const int32_t* __restrict__ neg, int n, int I,
                                                      uint8_t* __restrict__ mask) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= 2 * n) return;
    const int id = item_at(pos, neg, n, k);
    if (id >= 0 && id < I) mask[id] = 1;
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
struct StepLayout {            // float offsets into the step's workspace
    int64_t Gu, Gi, Hi, part, sums, ordu, ordi, mask, total;
};

inline int batch_workgroups(int n) { return (n + HW - 1) / HW; }

inline StepLayout step_layout(int n, int I) {
    StepLayout L;
    const int64_t n4 = round4(n);
    int64_t o = 0;
    L.Gu = o; o += n4 * D;
    L.Gi = o; o += 2 * n4 * D;
    L.Hi = o; o += 2 * n4 * D;
    L.part = o; o += round4(static_cast<int64_t>(batch_workgroups(n)) * LOSSP);
    L.sums = o; o += 4;
    L.ordu = o; o += n4;
    L.ordi = o; o += 2 * n4;
    L.mask = o; o += round4((static_cast<int64_t>(I) + 3) / 4);
    L.total = o;
    return L;
}

int run_square(const skr_spmm_plan* plan, const float* X, const skr_spmm_epilogue& ep, void* stream) {
    return skr_spmm_plan_run_ex(plan, X, D, &ep, nullptr, nullptr, stream);
}

int run_step(const skr_lattice_step_args* a, void* stream, float* h_ms) {
    SKR_REQUIRE(a, "skr_lattice_step: NULL argument");
    const int U = a->n_users, I = a->n_items, n = a->n, Ln = a->n_layers;
    SKR_REQUIRE(a->params && a->users && a->pos && a->neg && a->G && a->DH && a->grad && a->loss && a->work && a->ping[0] && a->ping[1],
                "skr_lattice_step: NULL argument");
    SKR_REQUIRE(U > 0 && I > 0 && n >= 0 && n <= MAXB, "skr_lattice_step: n_users = %d, n_items = %d, n = %d (at most %d rows)", U, I, n, MAXB);
    SKR_REQUIRE(a->dim >= 1 && a->dim <= D, "skr_lattice_step: 1 <= dim <= 64 (got %d); rows are 64 floats, zero-padded", a->dim);
    SKR_REQUIRE(a->cf_model == SKR_LATTICE_CF_LIGHTGCN || a->cf_model == SKR_LATTICE_CF_MF, "skr_lattice_step: cf_model = %d (lightgcn 0, mf 1)",
                a->cf_model);
    const int Lu = a->cf_model == SKR_LATTICE_CF_MF ? 0 : a->n_ui_layers;
    SKR_REQUIRE(a->n_ui_layers >= 0 && a->n_ui_layers <= MAXL && Ln >= 0 && Ln <= MAXL,
                "skr_lattice_step: 0 <= n_ui_layers, n_layers <= %d (got %d, %d)", MAXL, a->n_ui_layers, Ln);
    SKR_REQUIRE(Lu == 0 || (a->plan_p && a->plan_pt && a->M), "skr_lattice_step: n_ui_layers > 0 needs both plans of the square adjacency and M");
    SKR_REQUIRE(Ln == 0 || (a->plan_s && a->plan_st), "skr_lattice_step: n_layers > 0 needs both plans of the item graph");
    SKR_REQUIRE(a->reg >= 0.0f, "skr_lattice_step: reg = %g (>= 0)", a->reg);
    const bool build = a->g_out != nullptr && Ln > 0;
    SKR_REQUIRE(!build || (a->H && a->s_rowptr && a->s_col), "skr_lattice_step: g_out needs H and the pattern of S");
    const uintptr_t align = reinterpret_cast<uintptr_t>(a->params) | reinterpret_cast<uintptr_t>(a->grad) | reinterpret_cast<uintptr_t>(a->work) |
                            reinterpret_cast<uintptr_t>(a->M) | reinterpret_cast<uintptr_t>(a->G) | reinterpret_cast<uintptr_t>(a->ping[0]) |
                            reinterpret_cast<uintptr_t>(a->ping[1]) | reinterpret_cast<uintptr_t>(a->DH) | reinterpret_cast<uintptr_t>(a->H);
    if (n == 0) return SKR_OK;
    const StepLayout W = step_layout(n, I);
    SKR_REQUIRE(a->work_bytes >= static_cast<size_t>(W.total) * sizeof(float),
                "skr_lattice_step: work holds %zu bytes, skr_lattice_workspace(%d, %d) asks for %zu", a->work_bytes, n, I,
                static_cast<size_t>(W.total) * sizeof(float));
    SKR_REQUIRE((align & 15) == 0, "skr_lattice_step: the tables and work must be 16-byte aligned");
    hipStream_t st = skr::as_stream(stream);
    float* w = static_cast<float*>(a->work);
    int32_t* ordu = reinterpret_cast<int32_t*>(w + W.ordu);
    int32_t* ordi = reinterpret_cast<int32_t*>(w + W.ordi);
    uint8_t* mask = reinterpret_cast<uint8_t*>(w + W.mask);
    const int64_t n4 = round4(n);
    const int64_t UO = static_cast<int64_t>(U) * D, N = static_cast<int64_t>(U) + I, IO = static_cast<int64_t>(I) * D;
    const float scale = 1.0f / static_cast<float>(Lu + 1);
    StepTimer<SKR_LATTICE_GROUPS + 1> mk(h_ms, st);
    SKR_HIP(mk.mark());
    int rc = SKR_OK;
    // ---- forward, the user-item part (LATTICE.py:255-264): the layer means of X_k = P X_(k-1)
    const float* Mtab = Lu == 0 ? a->params : a->M;
    {
        const float* X = a->params;
        for (int k = 1; k <= Lu; ++k) {
            skr_spmm_epilogue ep = {};
            ep.mode = SKR_EPI_PLAIN;
            ep.accum_scale = scale;
            ep.Y = k == Lu ? nullptr : a->ping[(k - 1) & 1];
            ep.accum = a->M;
            ep.accum_base = k == 1 ? a->params : nullptr;
            rc = run_square(a->plan_p, X, ep, stream);
            if (rc != SKR_OK) return rc;
            X = ep.Y;
        }
    }
    SKR_HIP(mk.mark());
    // ---- h = S^Ln E_items (LATTICE.py:232-234); the last run at the batch's item rows only
    const float* hn = a->params + UO;
    if (Ln > 0) {
        SKR_HIP(hipMemsetAsync(mask, 0, static_cast<size_t>(I), st));
        hipLaunchKernelGGL(la_mark_kernel, dim3((2 * n + 255) / 256), dim3(256), 0, st, a->pos, a->neg, n, I, mask);
        SKR_LAUNCH_CHECK();
        if (build) SKR_HIP(hipMemcpyAsync(a->H, a->params + UO, static_cast<size_t>(IO) * sizeof(float), hipMemcpyDeviceToDevice, st));
        const float* X = a->params + UO;
        for (int l = 1; l <= Ln; ++l) {
            const bool last = l == Ln;
            float* Y = last || !build ? a->ping[(l - 1) & 1] : a->H + l * IO;
            skr_spmm_epilogue ep = {};
            ep.mode = SKR_EPI_PLAIN;
            ep.Y = Y;
            ep.accum_scale = 1.0f;
            rc = skr_spmm_plan_run_ex(a->plan_s, X, D, &ep, last ? mask : nullptr, nullptr, stream);
            if (rc != SKR_OK) return rc;
            X = Y;
        }
        hn = X;
    }
    SKR_HIP(mk.mark());
    // ---- the batch (LATTICE.py:270-294)
    const int n_wg = batch_workgroups(n);
    BatchParams bp = {};
    bp.M = Mtab; bp.h = hn; bp.users = a->users; bp.pos = a->pos; bp.neg = a->neg;
    bp.n = n; bp.U = U; bp.I = I; bp.n4 = n4;
    bp.inv_n = 1.0f / static_cast<float>(n); bp.reg = a->reg;
    bp.Gu = w + W.Gu; bp.Gi = w + W.Gi; bp.Hi = w + W.Hi; bp.part = w + W.part;
    hipLaunchKernelGGL(la_batch_kernel, dim3(n_wg), dim3(HW * 64), 0, st, bp);
    hipLaunchKernelGGL(part_reduce_kernel<LOSSP>, dim3(1), dim3(256), 0, st, w + W.part, n_wg, w + W.sums);
    hipLaunchKernelGGL(la_loss_kernel, dim3(1), dim3(64), 0, st, w + W.sums, n, a->reg, a->loss);
    SKR_LAUNCH_CHECK();
    SKR_HIP(mk.mark());
    // ---- the gradients with respect to M and to h_n: one ordered sum per distinct node into the cleared tables
    float* DHn = a->DH + static_cast<int64_t>(Ln > 0 ? Ln - 1 : 0) * IO;
    SKR_HIP(hipMemsetAsync(a->G, 0, static_cast<size_t>(N) * D * sizeof(float), st));
    SKR_HIP(hipMemsetAsync(DHn, 0, static_cast<size_t>(IO) * sizeof(float), st));
    hipLaunchKernelGGL(rank_triples_kernel<256>, dim3((3 * n + 255) / 256), dim3(256), 0, st, a->users, a->pos, a->neg, n, ordu, ordi);
    const int blocks_u = (n + HW - 1) / HW, blocks_i = (2 * n + HW - 1) / HW;
    hipLaunchKernelGGL(la_seg_add_kernel, dim3(blocks_u + blocks_i), dim3(HW * 64), 0, st, a->G, DHn, a->users, a->pos, a->neg, ordu, ordi, n, n4,
                       U, I, blocks_u, w + W.Gu, w + W.Gi, w + W.Hi);
    SKR_LAUNCH_CHECK();
    SKR_HIP(mk.mark());
    // ---- backward, the user-item part: acc = G; Lu times acc = P^T acc + G; the last writes acc / (Lu + 1) into the gradient
    if (Lu == 0) SKR_HIP(hipMemcpyAsync(a->grad, a->G, static_cast<size_t>(N) * D * sizeof(float), hipMemcpyDeviceToDevice, st));
    {
        const float* X = a->G;
        for (int k = 1; k <= Lu; ++k) {
            const bool last = k == Lu;
            skr_spmm_epilogue ep = {};
            ep.mode = SKR_EPI_PLAIN;
            ep.accum_scale = scale;
            ep.addend = a->G;
            ep.Y = last ? nullptr : a->ping[(k - 1) & 1];
            if (last) { ep.accum = a->grad; ep.accum_init = 1; }
            rc = run_square(a->plan_pt, X, ep, stream);
            if (rc != SKR_OK) return rc;
            X = ep.Y;
        }
    }
    SKR_HIP(mk.mark());
    // ---- backward through h: dh_(l-1) = S^T dh_l; the last adds into the gradient's item rows
    if (Ln == 0) {
        const unsigned wgs = static_cast<unsigned>(std::min<int64_t>((IO + 255) / 256, 8192));
        hipLaunchKernelGGL(add_kernel<256>, dim3(wgs), dim3(256), 0, st, a->grad + UO, DHn, IO);
        SKR_LAUNCH_CHECK();
    }
    for (int l = Ln; l >= 1; --l) {
        const bool last = l == 1;
        rc = plain_run(a->plan_st, a->DH + (l - 1) * IO, nullptr, last ? nullptr : a->DH + (l - 2) * IO, last ? a->grad + UO : nullptr, nullptr,
                       stream);
        if (rc != SKR_OK) return rc;
    }
    SKR_HIP(mk.mark());
    // ---- a build step: g = dLoss/dS on the entries of S; with one layer dh_1 is zero outside the batch's item rows
    if (build) {
        hipLaunchKernelGGL(la_sddmm_kernel, dim3(row_workgroups(I)), dim3(HW * 64), 0, st, I, I, a->s_rowptr, a->s_col, a->DH, IO, a->H, IO, Ln,
                           Ln == 1 ? mask : nullptr, 0, a->g_out);
        SKR_LAUNCH_CHECK();
    }
    SKR_HIP(mk.mark());
    SKR_HIP(mk.finish());
    return SKR_OK;
}

}  // namespace

extern "C" {

size_t skr_lattice_graph_workspace(int n_items) {
    if (n_items <= 0) return 0;
    return round16(static_cast<size_t>(n_items) * sizeof(int32_t));
}

int skr_lattice_graph(int n_items, int k, const int32_t* const* d_ids, const float* const* d_vals, const float* d_w, double lam,
                      int64_t* d_rowptr, int32_t* d_col, float* d_val, int32_t* d_slots, float* d_r, float* d_q, void* d_work,
                      size_t work_bytes, void* stream) {
    SKR_REQUIRE(d_ids && d_vals && d_w && d_rowptr && d_col && d_val && d_slots && d_r && d_q && d_work, "skr_lattice_graph: NULL argument");
    SKR_REQUIRE(n_items > 0 && k >= 1 && k <= MAXK && k <= n_items, "skr_lattice_graph: n_items = %d, 1 <= k <= min(%d, n_items) (got %d)", n_items,
                MAXK, k);
    SKR_REQUIRE(static_cast<int64_t>(n_items) * 4 * k <= INT32_MAX, "skr_lattice_graph: 4 k n_items must stay below 2^31");
    Lists ls;
    for (int t = 0; t < 4; ++t) {
        ls.ids[t] = d_ids[t];
        ls.val[t] = d_vals[t];
        SKR_REQUIRE((d_ids[t] == nullptr) == (d_vals[t] == nullptr), "skr_lattice_graph: list %d has ids without values or values without ids", t);
    }
    SKR_REQUIRE(ls.ids[0] || ls.ids[1], "skr_lattice_graph: no learned list at all");
    SKR_REQUIRE(work_bytes >= skr_lattice_graph_workspace(n_items), "skr_lattice_graph: work holds %zu bytes, skr_lattice_graph_workspace asks for %zu",
                work_bytes, skr_lattice_graph_workspace(n_items));
    SKR_REQUIRE((reinterpret_cast<uintptr_t>(d_work) & 15) == 0, "skr_lattice_graph: work must be 16-byte aligned");
    hipStream_t st = skr::as_stream(stream);
    int32_t* cnt = static_cast<int32_t*>(d_work);
    const int wgs = row_workgroups(n_items);
    const int64_t cap = static_cast<int64_t>(n_items) * 4 * k;
    hipLaunchKernelGGL(la_merge_kernel<false>, dim3(wgs), dim3(HW * 64), 0, st, ls, n_items, k, d_w, cnt, nullptr, nullptr, nullptr, nullptr, nullptr,
                       nullptr);
    hipLaunchKernelGGL(la_scan_kernel, dim3(1), dim3(1024), 0, st, cnt, static_cast<int64_t>(n_items), d_rowptr);
    hipLaunchKernelGGL(la_merge_kernel<true>, dim3(wgs), dim3(HW * 64), 0, st, ls, n_items, k, d_w, cnt, d_rowptr, d_col, d_val, d_slots, d_r, d_q);
    hipLaunchKernelGGL(la_values_kernel, dim3(wgs), dim3(HW * 64), 0, st, ls, n_items, k, d_w, static_cast<float>(1.0 - lam), static_cast<float>(lam),
                       d_rowptr, d_col, d_slots, d_q, d_val);
    hipLaunchKernelGGL(la_tail_kernel, dim3(static_cast<unsigned>(std::min<int64_t>((cap + 255) / 256, 4096))), dim3(256), 0, st, d_rowptr, n_items,
                       cap, d_col, d_val, d_slots);
    SKR_LAUNCH_CHECK();
    return SKR_OK;
}

int skr_lattice_sddmm(int n_rows, int n_cols, const int64_t* d_rowptr, const int32_t* d_col, const float* d_A, int64_t stride_a,
                      const float* d_B, int64_t stride_b, int n_layers, const uint8_t* d_row_mask, int accumulate, float* d_g,
                      void* stream) {
    SKR_REQUIRE(d_rowptr && d_col && d_A && d_B && d_g, "skr_lattice_sddmm: NULL argument");
    SKR_REQUIRE(n_rows > 0 && n_cols > 0, "skr_lattice_sddmm: n_rows = %d, n_cols = %d", n_rows, n_cols);
    SKR_REQUIRE(n_layers >= 1 && n_layers <= MAXL, "skr_lattice_sddmm: 1 <= n_layers <= %d (got %d)", MAXL, n_layers);
    SKR_REQUIRE(stride_a >= 0 && stride_b >= 0 && stride_a % 4 == 0 && stride_b % 4 == 0, "skr_lattice_sddmm: the layer strides must be multiples of 4");
    SKR_REQUIRE(((reinterpret_cast<uintptr_t>(d_A) | reinterpret_cast<uintptr_t>(d_B)) & 15) == 0, "skr_lattice_sddmm: the tables must be 16-byte aligned");
    hipLaunchKernelGGL(la_sddmm_kernel, dim3(row_workgroups(n_rows)), dim3(HW * 64), 0, skr::as_stream(stream), n_rows, n_cols, d_rowptr, d_col, d_A,
                       stride_a, d_B, stride_b, n_layers, d_row_mask, accumulate, d_g);
    SKR_LAUNCH_CHECK();
    return SKR_OK;
}

size_t skr_lattice_graph_bwd_workspace(int n_items, int64_t nnz) {
    if (n_items <= 0 || nnz < 0) return 0;
    return bwd_layout(n_items, nnz).total;
}

int skr_lattice_graph_bwd(int n_items, int k, int64_t nnz, const float* d_g, const int64_t* d_rowptr, const int32_t* d_col,
                          const int32_t* d_slots, const int64_t* d_rowptr_t, const int32_t* d_col_t, const int32_t* d_perm_t,
                          const int32_t* const* d_ids, const float* const* d_vals, const float* d_w, double lam, const float* d_q,
                          const float* const* d_F, float* const* d_dF, float* d_dw, void* d_work, size_t work_bytes, void* stream) {
    SKR_REQUIRE(d_g && d_rowptr && d_col && d_slots && d_rowptr_t && d_col_t && d_perm_t && d_ids && d_vals && d_w && d_q && d_F && d_dF && d_dw &&
                    d_work,
                "skr_lattice_graph_bwd: NULL argument");
    SKR_REQUIRE(n_items > 0 && k >= 1 && k <= MAXK && k <= n_items, "skr_lattice_graph_bwd: n_items = %d, 1 <= k <= min(%d, n_items) (got %d)",
                n_items, MAXK, k);
    SKR_REQUIRE(nnz >= 0 && nnz <= static_cast<int64_t>(n_items) * 4 * k, "skr_lattice_graph_bwd: 0 <= nnz <= 4 k n_items (got %lld)",
                static_cast<long long>(nnz));
    BwdParams p = {};
    for (int t = 0; t < 4; ++t) {
        p.ls.ids[t] = d_ids[t];
        p.ls.val[t] = d_vals[t];
        SKR_REQUIRE((d_ids[t] == nullptr) == (d_vals[t] == nullptr), "skr_lattice_graph_bwd: list %d has ids without values or values without ids", t);
    }
    for (int m = 0; m < 2; ++m) {
        SKR_REQUIRE((d_F[m] != nullptr) == (d_vals[m] != nullptr) && (d_F[m] != nullptr) == (d_dF[m] != nullptr),
                    "skr_lattice_graph_bwd: modality %d needs its learned list, F and dF together", m);
        SKR_REQUIRE(((reinterpret_cast<uintptr_t>(d_F[m]) | reinterpret_cast<uintptr_t>(d_dF[m])) & 15) == 0,
                    "skr_lattice_graph_bwd: the tables must be 16-byte aligned");
        p.F[m] = d_F[m];
        p.dF[m] = d_dF[m];
    }
    const BwdLayout L = bwd_layout(n_items, nnz);
    SKR_REQUIRE(work_bytes >= L.total, "skr_lattice_graph_bwd: work holds %zu bytes, skr_lattice_graph_bwd_workspace asks for %zu", work_bytes, L.total);
    SKR_REQUIRE((reinterpret_cast<uintptr_t>(d_work) & 15) == 0, "skr_lattice_graph_bwd: work must be 16-byte aligned");
    hipStream_t st = skr::as_stream(stream);
    char* wk = static_cast<char*>(d_work);
    p.I = n_items; p.k = k; p.nnz = nnz;
    p.g = d_g; p.rowptr = d_rowptr; p.col = d_col; p.slots = d_slots;
    p.rowptr_t = d_rowptr_t; p.col_t = d_col_t; p.perm_t = d_perm_t;
    p.w = d_w; p.oml = static_cast<float>(1.0 - lam); p.lam = static_cast<float>(lam); p.q = d_q;
    p.rho = reinterpret_cast<float*>(wk + L.rho);
    p.dL = reinterpret_cast<float*>(wk + L.dL);
    p.invn = reinterpret_cast<float*>(wk + L.invn);
    p.part = reinterpret_cast<float*>(wk + L.part);
    const int wgs = row_workgroups(n_items);
    hipLaunchKernelGGL(la_norm_kernel, dim3(wgs), dim3(HW * 64), 0, st, p.F[0], p.F[1], n_items, p.invn);
    hipLaunchKernelGGL(la_rho_kernel, dim3(wgs), dim3(HW * 64), 0, st, p);
    hipLaunchKernelGGL(la_dl_kernel, dim3(wgs), dim3(HW * 64), 0, st, p);
    hipLaunchKernelGGL(la_dw_kernel, dim3(1), dim3(64), 0, st, p.part, wgs, d_w, d_dw);
    hipLaunchKernelGGL(la_cos_bwd_kernel, dim3(wgs), dim3(HW * 64), 0, st, p);
    SKR_LAUNCH_CHECK();
    return SKR_OK;
}

int skr_lattice_add_normalized(const float* d_h, int64_t n_rows, float* d_out, void* stream) {
    SKR_REQUIRE(d_h && d_out, "skr_lattice_add_normalized: NULL argument");
    SKR_REQUIRE(n_rows >= 0 && n_rows <= INT32_MAX, "skr_lattice_add_normalized: n_rows = %lld", static_cast<long long>(n_rows));
    if (n_rows == 0) return SKR_OK;
    hipLaunchKernelGGL(la_add_normalized_kernel, dim3(row_workgroups(n_rows)), dim3(HW * 64), 0, skr::as_stream(stream), d_h, n_rows, d_out);
    SKR_LAUNCH_CHECK();
    return SKR_OK;
}

size_t skr_lattice_workspace(int n, int n_items) {
    if (n <= 0 || n > MAXB || n_items <= 0) return 0;
    return static_cast<size_t>(step_layout(n, n_items).total) * sizeof(float);
}

int skr_lattice_step(const skr_lattice_step_args* args, void* stream) { return run_step(args, stream, nullptr); }

int skr_lattice_step_timed(const skr_lattice_step_args* args, void* stream, float* h_ms) {
    SKR_REQUIRE(h_ms != nullptr, "skr_lattice_step_timed: NULL argument");
    return run_step(args, stream, h_ms);
}

}  // extern "C"
