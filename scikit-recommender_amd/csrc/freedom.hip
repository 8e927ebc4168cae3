// freedom.hip -- FREEDOM (A Tale of Two Graphs: Freezing and Denoising Graph Structures for Multimodal Recommendation, ACM MM
// 2023): a LightGCN encoder over a user-item graph that is pruned anew every epoch, a frozen item-item kNN graph whose
// propagation of the item embeddings is added to the item rows, and three BPR terms that share the user row -- the graph
// term and, per present modality, one against the projected feature rows.  Here: the degree-sensitive edge pruning (keys,
// select, the compacted and renormalised CSR pair), the batch kernel and the host entry that issues one training step.
//
// Replaces the stock torch ops the reference issues (no native code there):
//   recommender/FREEDOM.py:175-201  torch.multinomial over all edges, _normalize_adj_m of the kept ones, the square COO tensor
//   recommender/FREEDOM.py:211-225  n_mm_layers torch.sparse.mm on the item graph, n_ui_layers on the square adjacency, the mean
//   recommender/FREEDOM.py:227-252  the three bpr_loss terms, text_trs / image_trs on the WHOLE [I, F] tables (here: on the
//                                   batch's rows only), and autograd's backward through all of it
//
// Layout: see include/skrec_hip.h, section L.
//
// Launches of a step (reg > 0 only: the lines marked *):
//   2 Lu plan runs   X_k = A' X_(k-1): user rows from A', item rows from A'^T; the mean M rides in the accum epilogue
//   Lm plan runs     h_k = S h_(k-1) on the item rows; the last adds into M's item rows (Lm == 0: M_i += X0_i)
// * clear, project   the feature-gradient rows the previous step wrote := 0; per modality skr_bm3_project at pos and at neg
//   batch            one wavefront per batch row: x_g, x_m, logsigmoid, c = -sigmoid(-x) / n, the rows' gradients
//   part_reduce      the workgroups' loss sums in workgroup order;  loss: the components
//   rank, seg_add    G = 0; the positions of the user list and of pos || neg sorted by (id, position); one writer per distinct id
// * per modality     db = 0, trs_wgrad (dW = sum_r g_m[r] (f[pos_r] - f[neg_r])^T: a workgroup owns 64 columns and walks the
//                    batch in order), seg_rows (+-g_m per distinct item, in rank order), feat_grad (dX[j] = g_j W)
//   2 Lu plan runs   acc = G; acc = A'^T acc + G; the last writes acc / (Lu + 1) into the gradient (Lu == 0: grad = G)
//   Lm plan runs     t_k = S^T t_(k-1) on G's item rows; the last adds into the gradient's item rows (Lm == 0: grad_i += G_i)
//
// trs_wgrad and seg_rows are bm3.hip's, restated for the difference of two feature rows and the 2 n long item list; the
// kernels that are the same text -- rank_triples, add, feat_grad, clear_rows -- are step_common.h's.  Determinism: no floating-point atomic anywhere; the select's histograms are integer atomics, whose result does
// not depend on their order.
#include "skr_common.h"
#include "fast_rng.h"
#include "mfma_tile.h"
#include "step_common.h"

#include <algorithm>

namespace {

using namespace skr;

constexpr int D = 64;          // columns of every table
constexpr int HW = 4;          // wavefronts per workgroup
constexpr int MAXB = SKR_FREEDOM_MAX_BATCH;
constexpr int MAXL = SKR_FREEDOM_MAX_LAYERS;
constexpr int MAXF = SKR_FREEDOM_MAX_FEAT;
constexpr int LOSSP = 4;       // loss sums per workgroup: graph, image, text, unused
constexpr int SEL_T = 256;     // select: threads per workgroup
constexpr int SEL_ITEMS = 16;  // ... consecutive entries per thread
constexpr int SEL_CHUNK = SEL_T * SEL_ITEMS;

// ------------------------------------------------------------------------------------------------
// pruning, part 1: the keys
// ------------------------------------------------------------------------------------------------
// keys[e] = w[e] / E_e, E_e = -log(u), u = (r + 0.5) 2^-32 in (0, 1) from 32 random bits keyed by (seed, epoch, e): the
// largest n_keep keys are a weighted sample without replacement (Efraimidis and Spirakis).  E lies in [1.1e-10, 22.2], so a
// key is finite, and positive where w is.
__global__ __launch_bounds__(256) void fd_keys_kernel(const float* __restrict__ w, int64_t nnz, uint64_t seed, uint64_t epoch,
                                                      float* __restrict__ keys) {
    const int64_t e = blockIdx.x * static_cast<int64_t>(256) + threadIdx.x;
    if (e >= nnz) return;
    Xoshiro128pp g;
    g.seed(seed, epoch, static_cast<uint64_t>(e));
    const double u = (static_cast<double>(g.next()) + 0.5) * 0x1p-32;
    keys[e] = static_cast<float>(static_cast<double>(w[e]) / -log(u));
}

// ------------------------------------------------------------------------------------------------
// pruning, part 2: radix select on the bit patterns of the positive keys
// ------------------------------------------------------------------------------------------------
// state[0] = the threshold's bits found so far (the digits below are zero), state[1] = how many entries are still wanted among
// those that share them
__global__ __launch_bounds__(1024) void fd_sel_init_kernel(uint32_t* __restrict__ hist, uint32_t* __restrict__ state, uint32_t n_keep) {
    hist[threadIdx.x] = 0;
    if (threadIdx.x == 0) { state[0] = 0; state[1] = n_keep; state[2] = 0; state[3] = 0; }
}

// hist[d] += the entries whose higher digits equal the threshold's and whose digit of this pass is d
__global__ __launch_bounds__(SEL_T) void fd_sel_hist_kernel(const uint32_t* __restrict__ bits, int64_t nnz, int pass,
                                                            const uint32_t* __restrict__ state, uint32_t* __restrict__ hist) {
    __shared__ uint32_t h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const int shift = 24 - 8 * pass;
    const uint32_t prefix = state[0];
    const uint32_t himask = pass == 0 ? 0u : 0xFFFFFFFFu << (shift + 8);
    const int64_t base = blockIdx.x * static_cast<int64_t>(SEL_CHUNK);
    for (int j = 0; j < SEL_ITEMS; ++j) {
        const int64_t e = base + j * SEL_T + threadIdx.x;
        if (e < nnz) {
            const uint32_t b = bits[e];
            if ((b & himask) == prefix) atomicAdd(&h[(b >> shift) & 255u], 1u);
        }
    }
    __syncthreads();
    if (h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], h[threadIdx.x]);
}

// the digit of this pass: the largest d with (entries of a larger digit) < wanted <= (entries of a digit >= d)
__global__ __launch_bounds__(64) void fd_sel_pick_kernel(const uint32_t* __restrict__ hist, int pass, uint32_t* __restrict__ state) {
    if (threadIdx.x != 0) return;
    const uint32_t want = state[1];
    uint32_t above = 0;
    int d = 255;
    for (; d > 0; --d) {
        const uint32_t c = hist[d];
        if (above + c >= want) break;
        above += c;
    }
    state[0] |= static_cast<uint32_t>(d) << (24 - 8 * pass);
    state[1] = want - above;
}

// cnt[block] = the block's entries equal to the threshold
__global__ __launch_bounds__(SEL_T) void fd_sel_ties_kernel(const uint32_t* __restrict__ bits, int64_t nnz, const uint32_t* __restrict__ state,
                                                            uint32_t* __restrict__ cnt) {
    __shared__ int s[HW];
    const uint32_t T = state[0];
    const int64_t base = blockIdx.x * static_cast<int64_t>(SEL_CHUNK);
    int c = 0;
    for (int j = 0; j < SEL_ITEMS; ++j) {
        const int64_t e = base + j * SEL_T + threadIdx.x;
        c += e < nnz && bits[e] == T ? 1 : 0;
    }
    c = wave_sum(c);
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) cnt[blockIdx.x] = static_cast<uint32_t>(s[0] + s[1] + s[2] + s[3]);
}

// out [n + 1] = the exclusive prefix sums of cnt [n] and their total: one workgroup walks the array 1024 at a time
template <class T>
__global__ __launch_bounds__(1024) void fd_scan_kernel(const T* __restrict__ cnt, int64_t n, int64_t* __restrict__ out) {
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

// keep[e] = key above the threshold, or equal to it and among the first state[1] such entries by index.  A thread owns
// SEL_ITEMS consecutive entries, so that the ranks of the ties follow the index.
__global__ __launch_bounds__(SEL_T) void fd_sel_mark_kernel(const uint32_t* __restrict__ bits, int64_t nnz, const uint32_t* __restrict__ state,
                                                            const int64_t* __restrict__ off, uint8_t* __restrict__ keep) {
    __shared__ int s[SEL_T];
    const uint32_t T = state[0];
    const int64_t want = state[1];
    const int t = threadIdx.x;
    const int64_t e0 = blockIdx.x * static_cast<int64_t>(SEL_CHUNK) + static_cast<int64_t>(t) * SEL_ITEMS;
    uint32_t b[SEL_ITEMS];
    int c = 0;
#pragma unroll
    for (int j = 0; j < SEL_ITEMS; ++j) {
        b[j] = e0 + j < nnz ? bits[e0 + j] : 0u;
        c += e0 + j < nnz && b[j] == T ? 1 : 0;
    }
    s[t] = c;
    __syncthreads();
    for (int o = 1; o < SEL_T; o <<= 1) {
        const int a = t >= o ? s[t - o] : 0;
        __syncthreads();
        s[t] += a;
        __syncthreads();
    }
    int64_t rank = off[blockIdx.x] + s[t] - c;
#pragma unroll
    for (int j = 0; j < SEL_ITEMS; ++j) {
        if (e0 + j >= nnz) break;
        bool k = b[j] > T;
        if (b[j] == T) { k = rank < want; ++rank; }
        keep[e0 + j] = k ? 1 : 0;
    }
}

struct SelectLayout {          // byte offsets into the select's workspace
    size_t off, hist, state, cnt, total;
    int64_t blocks;
};
inline SelectLayout select_layout(int64_t nnz) {
    SelectLayout L;
    L.blocks = (nnz + SEL_CHUNK - 1) / SEL_CHUNK;
    size_t o = 0;
    L.off = o; o += static_cast<size_t>(L.blocks + 1) * sizeof(int64_t);
    L.hist = o; o += 4 * 256 * sizeof(uint32_t);
    L.state = o; o += 4 * sizeof(uint32_t);
    L.cnt = o; o += static_cast<size_t>(L.blocks) * sizeof(uint32_t);
    L.total = (o + 15) & ~static_cast<size_t>(15);
    return L;
}

// ------------------------------------------------------------------------------------------------
// pruning, part 3: the compacted, renormalised CSR pair
// ------------------------------------------------------------------------------------------------
// keep_t (R^T's entry order) from keep (R's)
__global__ __launch_bounds__(256) void fd_keep_t_kernel(const uint8_t* __restrict__ keep, const int32_t* __restrict__ perm, int64_t nnz,
                                                        uint8_t* __restrict__ keep_t) {
    const int64_t e = blockIdx.x * static_cast<int64_t>(256) + threadIdx.x;
    if (e >= nnz) return;
    const int64_t p = perm[e];
    if (p >= 0 && p < nnz) keep_t[p] = keep[e] ? 1 : 0;
}

// a wavefront per row of [[R], [R^T]]: cnt[r] = its kept entries, inv[r] = float((1e-7 + cnt)^-0.5), the power in float64
__global__ __launch_bounds__(HW * 64) void fd_row_count_kernel(const int64_t* __restrict__ rowptr, const int64_t* __restrict__ rowptr_t,
                                                               const uint8_t* __restrict__ keep, const uint8_t* __restrict__ keep_t, int U,
                                                               int I, int64_t nnz, int32_t* __restrict__ cnt, float* __restrict__ inv) {
    const int lane = threadIdx.x & 63;
    const int64_t r = blockIdx.x * static_cast<int64_t>(HW) + (threadIdx.x >> 6);
    if (r >= static_cast<int64_t>(U) + I) return;
    const bool user = r < U;
    const int64_t* rp = user ? rowptr + r : rowptr_t + (r - U);
    const uint8_t* flags = user ? keep : keep_t;
    const int64_t beg = rp[0] > 0 ? rp[0] : 0, end = rp[1] < nnz ? rp[1] : nnz;
    int c = 0;
    for (int64_t e = beg + lane; e < end; e += 64) c += flags[e] ? 1 : 0;
    c = wave_sum(c);
    if (lane == 0) {
        cnt[r] = c;
        inv[r] = static_cast<float>(pow(1e-7 + static_cast<double>(c), -0.5));
    }
}

// a wavefront per row: the kept entries in their order, value = inv[user] * inv[U + item] (one fp32 product)
__global__ __launch_bounds__(HW * 64) void fd_fill_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                          const int64_t* __restrict__ rowptr_t, const int32_t* __restrict__ col_t,
                                                          const uint8_t* __restrict__ keep, const uint8_t* __restrict__ keep_t, int U, int I,
                                                          int64_t nnz, const float* __restrict__ inv, const int64_t* __restrict__ out_rp,
                                                          int32_t* __restrict__ out_col, float* __restrict__ out_val,
                                                          const int64_t* __restrict__ out_rp_t, int32_t* __restrict__ out_col_t,
                                                          float* __restrict__ out_val_t) {
    const int lane = threadIdx.x & 63;
    const int64_t r = blockIdx.x * static_cast<int64_t>(HW) + (threadIdx.x >> 6);
    if (r >= static_cast<int64_t>(U) + I) return;
    const bool user = r < U;
    const int64_t row = user ? r : r - U;
    const int64_t* rp = (user ? rowptr : rowptr_t) + row;
    const int32_t* cols = user ? col : col_t;
    const uint8_t* flags = user ? keep : keep_t;
    int32_t* oc = user ? out_col : out_col_t;
    float* ov = user ? out_val : out_val_t;
    const int limit = user ? I : U;
    const int64_t beg = rp[0] > 0 ? rp[0] : 0, end = rp[1] < nnz ? rp[1] : nnz;
    int64_t at = (user ? out_rp : out_rp_t)[row];
    for (int64_t e0 = beg; e0 < end; e0 += 64) {
        const int64_t e = e0 + lane;
        const bool k = e < end && flags[e] != 0;
        const uint64_t mask = __ballot(k);
        if (k) {
            const int64_t pos = at + __popcll(mask & ((1ull << lane) - 1ull));
            const int c = cols[e];
            const int cc = c < 0 ? 0 : (c < limit ? c : limit - 1);
            if (pos >= 0 && pos < nnz) {
                oc[pos] = c;
                ov[pos] = user ? inv[r] * inv[U + cc] : inv[cc] * inv[r];
            }
        }
        at += __popcll(mask);
    }
}

struct PruneLayout {           // byte offsets into the compaction's workspace
    size_t keep_t, cnt, inv, total;
};
inline PruneLayout prune_layout(int64_t N, int64_t nnz) {
    PruneLayout L;
    size_t o = 0;
    L.keep_t = o; o += (static_cast<size_t>(nnz) + 15) & ~static_cast<size_t>(15);
    L.cnt = o; o += (static_cast<size_t>(N) * sizeof(int32_t) + 15) & ~static_cast<size_t>(15);
    L.inv = o; o += (static_cast<size_t>(N) * sizeof(float) + 15) & ~static_cast<size_t>(15);
    L.total = o;
    return L;
}

// ------------------------------------------------------------------------------------------------
// the step: batch kernel, loss, ordered adds
// ------------------------------------------------------------------------------------------------
// Item list: position o < n is pos[o], position n + b is neg[b]; its rows of Gi lie at o resp. n4 + b.
struct BatchParams {
    const float* M;
    const float* Yp[2];            // the projected rows at pos, NULL: the modality takes no part (absent, or reg == 0)
    const float* Yn[2];
    const int32_t* users;
    const int32_t* pos;
    const int32_t* neg;
    int n, U, I;
    int64_t n4;
    float inv_n, reg;
    float* Gu;                     // [n4][64]   c_g (p - q) + reg sum_m c_m (P_m - Q_m)
    float* Gi;                     // [2 n4][64] + c_g u, then - c_g u
    float* Gm[2];                  // [n4][64]   reg c_m u
    float* part;                   // [gridDim.x][LOSSP]
};

__global__ __launch_bounds__(HW * 64) void fd_batch_kernel(BatchParams p) {
    __shared__ float s[HW][LOSSP];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int b = blockIdx.x * HW + wv;
    float lg = 0.0f, lm[2] = {0.0f, 0.0f};
    if (b < p.n) {
        const int64_t u = checked(p.users[b], p.U), i = checked(p.pos[b], p.I), j = checked(p.neg[b], p.I);
        const bool valid = u >= 0 && i >= 0 && j >= 0;
        float gu = 0.0f, gi = 0.0f, gm[2] = {0.0f, 0.0f};
        if (valid) {
            const float uv = p.M[u * D + lane];
            const float diff = p.M[(p.U + i) * D + lane] - p.M[(p.U + j) * D + lane];
            const float x = wave_sum(uv * diff);
            const float c = -sigmoid_neg(x) * p.inv_n;
            lg = -log_sigmoid(x);
            gu = c * diff;
            gi = c * uv;
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                if (p.Yp[m] == nullptr) continue;
                const int64_t f = static_cast<int64_t>(b) * D + lane;
                const float dm = p.Yp[m][f] - p.Yn[m][f];
                const float xm = wave_sum(uv * dm);
                const float cm = p.reg * (-sigmoid_neg(xm) * p.inv_n);
                lm[m] = -log_sigmoid(xm);
                gu += cm * dm;
                gm[m] = cm * uv;
            }
        }
        const int64_t f = static_cast<int64_t>(b) * D + lane;
        p.Gu[f] = gu;
        p.Gi[f] = gi;
        p.Gi[p.n4 * D + f] = -gi;
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            if (p.Gm[m] != nullptr) p.Gm[m][f] = gm[m];
        }
    }
    if (lane == 0) { s[wv][0] = lg; s[wv][1] = lm[0]; s[wv][2] = lm[1]; s[wv][3] = 0.0f; }
    __syncthreads();
    if (threadIdx.x < LOSSP) {
        const int k = threadIdx.x;
        p.part[static_cast<int64_t>(blockIdx.x) * LOSSP + k] = ((s[0][k] + s[1][k]) + s[2][k]) + s[3][k];
    }
}

// loss[0] = the graph term, loss[1] = reg * (text + image), loss[2] = their sum; sums [LOSSP]: graph, image, text
__global__ __launch_bounds__(64) void fd_loss_kernel(const float* __restrict__ sums, int n, float reg, float* __restrict__ loss) {
    if (threadIdx.x != 0) return;
    const float fn = static_cast<float>(n);
    const float g = sums[0] / fn, modal = reg * (sums[2] / fn + sums[1] / fn);
    loss[0] = g;
    loss[1] = modal;
    loss[2] = g + modal;
}

// G[id] = the sum of the rows whose list entry is id, in rank order, by the wavefront of the id's first rank: one writer
// per distinct id (G is cleared first).  Blocks [0, blocks_u) walk the user list, the others the item list.  (lattice.hip's
// la_seg_add_kernel sums a second table beside it, mgcn.hip's three slot tables, bm3.hip's adds onto G over one item list.)
__global__ __launch_bounds__(HW * 64) void fd_seg_add_kernel(float* __restrict__ G, const int32_t* __restrict__ users,
                                                             const int32_t* __restrict__ pos, const int32_t* __restrict__ neg,
                                                             const int32_t* __restrict__ order_u, const int32_t* __restrict__ order_i, int n,
                                                             int64_t n4, int U, int I, int blocks_u, const float* __restrict__ Gu,
                                                             const float* __restrict__ Gi) {
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
    float acc = 0.0f;
    for (int k = rk; k < len; ++k) {
        const int o = order[k];
        if (id_at(o) != id) break;
        const int64_t row = user ? o : (o < n ? o : n4 + (o - n));
        acc += (user ? Gu : Gi)[row * D + lane];
    }
    G[(static_cast<int64_t>(user ? 0 : U) + id) * D + lane] = acc;
}

// ------------------------------------------------------------------------------------------------
// the projection backward (bm3.hip's kernels on f[pos] - f[neg] and on the 2 n long item list; feat_grad: step_common.h)
// ------------------------------------------------------------------------------------------------
// dW[o][f] = sum_b g[b][o] (X[pos_b][f] - X[neg_b][f]): a wavefront owns 16 columns f and walks the batch in order, four rows
// per MFMA (A = g^T, B = the differences of the gathered rows); acc[mb][rr] = dW[16 mb + g + 4 rr][f0 + r].
// (bm_trs_wgrad_kernel: one gathered row, not a difference, summed in fp32.)
// The sum runs on v_mfma_f64_16x16x4_f64 (A and B as the fp32 instruction of that shape, the result's row g + 4 rr): it is the one long sum
// of the step -- up to 2 048 terms of either sign that nearly cancel -- and an element that starts with a gradient beside
// Adam's eps has its fp32 rounding magnified by up to lr / eps in the first update.  In float64 only the terms' own
// rounding is left; the sum is rounded to fp32 once.
__global__ __launch_bounds__(HW * 64) void fd_trs_wgrad_kernel(const float* __restrict__ X, int n_rows, int ld, const int32_t* __restrict__ pos,
                                                               const int32_t* __restrict__ neg, int n, const float* __restrict__ dY,
                                                               float* __restrict__ dW) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
    const int f = blockIdx.x * 64 + wv * 16 + r;
    const bool fin = f < ld;
    f64x4 acc[4];
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) acc[mb] = f64x4{0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < n; k0 += 16) {
        double a[4][4], b[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int bk = k0 + 4 * j + g;
            const bool in = bk < n;
            const int64_t ip = in ? checked(pos[bk], n_rows) : -1, iq = in ? checked(neg[bk], n_rows) : -1;
            b[j] = ip >= 0 && iq >= 0 && fin ? static_cast<double>(X[ip * ld + f]) - static_cast<double>(X[iq * ld + f]) : 0.0;
#pragma unroll
            for (int mb = 0; mb < 4; ++mb) a[j][mb] = in ? static_cast<double>(dY[static_cast<int64_t>(bk) * D + mb * 16 + r]) : 0.0;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int mb = 0; mb < 4; ++mb) acc[mb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[j][mb], b[j], acc[mb], 0, 0, 0);
        }
    }
    if (!fin) return;
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) {
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) dW[static_cast<int64_t>(mb * 16 + g + 4 * rr) * ld + f] = static_cast<float>(acc[mb][rr]);
    }
}

// Gseg[rk] = the signed sum (+ at pos, - at neg) of the g rows whose item is the one at rank rk, in rank order, head[rk] =
// that item -- at the first rank of every distinct valid item; zeros and -1 at every other rank.  len = 2 n ranks.
// (bm_seg_rows_kernel: one list of n items, no sign.)
__global__ __launch_bounds__(HW * 64) void fd_seg_rows_kernel(const int32_t* __restrict__ pos, const int32_t* __restrict__ neg,
                                                              const int32_t* __restrict__ order, int n, int I, const float* __restrict__ dY,
                                                              float* __restrict__ Gseg, int32_t* __restrict__ head) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int rk = blockIdx.x * HW + wv;
    if (rk >= 2 * n) return;
    const int id = item_at(pos, neg, n, order[rk]);
    const bool first = id >= 0 && id < I && !(rk > 0 && item_at(pos, neg, n, order[rk - 1]) == id);
    float acc = 0.0f;
    if (first) {
        for (int k = rk; k < 2 * n; ++k) {
            const int o = order[k];
            if (item_at(pos, neg, n, o) != id) break;
            const float v = dY[static_cast<int64_t>(o < n ? o : o - n) * D + lane];
            acc += o < n ? v : -v;
        }
    }
    Gseg[static_cast<int64_t>(rk) * D + lane] = acc;
    if (lane == 0) head[rk] = first ? id : -1;
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
struct StepLayout {            // float offsets into the step's workspace
    int64_t Gu, Gi, Gm, Yp, Yn, part, sums, ordu, ordi, Gseg, head, total;
};

inline int batch_workgroups(int n) { return (n + HW - 1) / HW; }

inline StepLayout step_layout(int n) {
    StepLayout L;
    const int64_t n4 = round4(n);
    int64_t o = 0;
    L.Gu = o; o += n4 * D;
    L.Gi = o; o += 2 * n4 * D;
    L.Gm = o; o += 2 * n4 * D;
    L.Yp = o; o += 2 * n4 * D;
    L.Yn = o; o += 2 * n4 * D;
    L.part = o; o += round4(static_cast<int64_t>(batch_workgroups(n)) * LOSSP);
    L.sums = o; o += 4;
    L.ordu = o; o += n4;
    L.ordi = o; o += 2 * n4;
    L.Gseg = o; o += 2 * n4 * D;
    L.head = o; o += 2 * n4;
    L.total = o;
    return L;
}

int run_step(const skr_freedom_step_args* a, void* stream, float* h_ms) {
    SKR_REQUIRE(a, "skr_freedom_step: NULL argument");
    const int U = a->n_users, I = a->n_items, n = a->n, Lu = a->n_ui_layers, Lm = a->n_mm_layers;
    SKR_REQUIRE(a->params && a->users && a->pos && a->neg && a->M && a->G && a->grad && a->loss && a->work, "skr_freedom_step: NULL argument");
    SKR_REQUIRE(U > 0 && I > 0 && n >= 0 && n <= MAXB, "skr_freedom_step: n_users = %d, n_items = %d, n = %d (at most %d rows)", U, I, n, MAXB);
    SKR_REQUIRE(a->dim >= 1 && a->dim <= D, "skr_freedom_step: 1 <= dim <= 64 (got %d); rows are 64 floats, zero-padded", a->dim);
    SKR_REQUIRE(Lu >= 0 && Lu <= MAXL && Lm >= 0 && Lm <= MAXL, "skr_freedom_step: 0 <= n_ui_layers, n_mm_layers <= %d (got %d, %d)", MAXL, Lu, Lm);
    SKR_REQUIRE(Lu == 0 || (a->plan_a && a->plan_at), "skr_freedom_step: n_ui_layers > 0 needs both plans of the user-item graph");
    SKR_REQUIRE(Lm == 0 || (a->plan_s && a->plan_st), "skr_freedom_step: n_mm_layers > 0 needs both plans of the item graph");
    SKR_REQUIRE((Lu < 2 && Lm < 2) || (a->ping[0] && a->ping[1]), "skr_freedom_step: more than one layer needs both ping tables");
    SKR_REQUIRE(a->reg >= 0.0f, "skr_freedom_step: reg = %g (>= 0)", a->reg);
    const bool modal = a->reg > 0.0f;
    SKR_REQUIRE(a->n_clear >= 0 && a->n_clear <= 2 * MAXB && (a->n_clear == 0 || a->clear_items),
                "skr_freedom_step: n_clear = %d (at most %d ids, clear_items not NULL)", a->n_clear, 2 * MAXB);
    uintptr_t align = reinterpret_cast<uintptr_t>(a->params) | reinterpret_cast<uintptr_t>(a->grad) | reinterpret_cast<uintptr_t>(a->work) |
                      reinterpret_cast<uintptr_t>(a->M) | reinterpret_cast<uintptr_t>(a->G) | reinterpret_cast<uintptr_t>(a->ping[0]) |
                      reinterpret_cast<uintptr_t>(a->ping[1]);
    for (int m = 0; m < 2 && modal; ++m) {
        if (a->feat_dim[m] == 0) continue;
        const int F = a->feat_dim[m], ld = a->feat_ld[m];
        SKR_REQUIRE(F >= 1 && F <= MAXF, "skr_freedom_step: 1 <= feat_dim <= %d (got %d)", MAXF, F);
        SKR_REQUIRE(ld >= F && ld % 4 == 0 && ld <= MAXF, "skr_freedom_step: feat_ld = %d must be a multiple of 4, >= feat_dim = %d and <= %d", ld,
                    F, MAXF);
        SKR_REQUIRE(a->trs[m] && a->feat[m] && a->trs_grad[m] && a->feat_grad[m], "skr_freedom_step: a present modality needs its four tables");
        align |= reinterpret_cast<uintptr_t>(a->trs[m]) | reinterpret_cast<uintptr_t>(a->feat[m]) | reinterpret_cast<uintptr_t>(a->trs_grad[m]) |
                 reinterpret_cast<uintptr_t>(a->feat_grad[m]);
    }
    if (n == 0) return SKR_OK;
    const StepLayout W = step_layout(n);
    SKR_REQUIRE(a->work_bytes >= static_cast<size_t>(W.total) * sizeof(float),
                "skr_freedom_step: work holds %zu bytes, skr_freedom_workspace(%d) asks for %zu", a->work_bytes, n,
                static_cast<size_t>(W.total) * sizeof(float));
    SKR_REQUIRE((align & 15) == 0, "skr_freedom_step: the tables and work must be 16-byte aligned");
    hipStream_t st = skr::as_stream(stream);
    float* w = static_cast<float*>(a->work);
    int32_t* ordu = reinterpret_cast<int32_t*>(w + W.ordu);
    int32_t* ordi = reinterpret_cast<int32_t*>(w + W.ordi);
    int32_t* head = reinterpret_cast<int32_t*>(w + W.head);
    const int64_t n4 = round4(n);
    const int64_t UO = static_cast<int64_t>(U) * D, N = static_cast<int64_t>(U) + I, IO = static_cast<int64_t>(I) * D;
    const bool has[2] = {modal && a->feat_dim[0] != 0, modal && a->feat_dim[1] != 0};
    StepTimer<SKR_FREEDOM_GROUPS + 1> mk(h_ms, st);        // h_ms: an event after every launch group; otherwise nothing
    SKR_HIP(mk.mark());
    // ---- forward (FREEDOM.py:216-224): the layer means of X_k = A' X_(k-1)
    const auto product = [&](const skr_spmm_plan* plan, const float* X, const skr_spmm_epilogue& ep, bool) {
        return skr_spmm_plan_run_ex(plan, X, D, &ep, nullptr, nullptr, stream);
    };
    int rc = mean_forward(a->plan_a, a->plan_at, a->params, UO, N, Lu, a->ping, a->M, st, product);
    if (rc != SKR_OK) return rc;
    SKR_HIP(mk.mark());
    // ---- h = S^Lm X0_items (FREEDOM.py:212-214), added to M's item rows (:225); the ping tables are free again
    if (Lm == 0) {
        const unsigned wgs = static_cast<unsigned>(std::min<int64_t>((IO + 255) / 256, 8192));
        hipLaunchKernelGGL(add_kernel<256>, dim3(wgs), dim3(256), 0, st, a->M + UO, a->params + UO, IO);
        SKR_LAUNCH_CHECK();
    }
    {
        const float* X = a->params + UO;
        for (int k = 1; k <= Lm; ++k) {
            const bool last = k == Lm;
            float* Y = last ? nullptr : a->ping[(k - 1) & 1];
            rc = plain_run(a->plan_s, X, nullptr, Y, last ? a->M + UO : nullptr, nullptr, stream);
            if (rc != SKR_OK) return rc;
            X = Y;
        }
    }
    SKR_HIP(mk.mark());
    // ---- the projected rows of pos and of neg (FREEDOM.py:246-251, on the batch's rows only)
    float* Yp[2] = {nullptr, nullptr};
    float* Yn[2] = {nullptr, nullptr};
    float* Gm[2] = {nullptr, nullptr};
    if (modal && a->n_clear > 0 && (has[0] || has[1])) {
        ClearParams cp = {{has[0] ? a->feat_grad[0] : nullptr, has[1] ? a->feat_grad[1] : nullptr}, {a->feat_ld[0], a->feat_ld[1]}};
        hipLaunchKernelGGL(clear_rows_kernel<256>, dim3(a->n_clear, 2), dim3(256), 0, st, cp, a->clear_items, I);
        SKR_LAUNCH_CHECK();
    }
    for (int m = 0; m < 2; ++m) {
        if (!has[m]) continue;
        Yp[m] = w + W.Yp + m * n4 * D;
        Yn[m] = w + W.Yn + m * n4 * D;
        Gm[m] = w + W.Gm + m * n4 * D;
        rc = skr_bm3_project(a->feat[m], I, a->feat_dim[m], a->feat_ld[m], a->trs[m], a->pos, n, Yp[m], stream);
        if (rc != SKR_OK) return rc;
        rc = skr_bm3_project(a->feat[m], I, a->feat_dim[m], a->feat_ld[m], a->trs[m], a->neg, n, Yn[m], stream);
        if (rc != SKR_OK) return rc;
    }
    SKR_HIP(mk.mark());
    // ---- the three BPR terms (FREEDOM.py:227-252)
    const int n_wg = batch_workgroups(n);
    BatchParams bp = {};
    bp.M = a->M; bp.users = a->users; bp.pos = a->pos; bp.neg = a->neg;
    for (int m = 0; m < 2; ++m) { bp.Yp[m] = Yp[m]; bp.Yn[m] = Yn[m]; bp.Gm[m] = Gm[m]; }
    bp.n = n; bp.U = U; bp.I = I; bp.n4 = n4;
    bp.inv_n = 1.0f / static_cast<float>(n); bp.reg = a->reg;
    bp.Gu = w + W.Gu; bp.Gi = w + W.Gi; bp.part = w + W.part;
    hipLaunchKernelGGL(fd_batch_kernel, dim3(n_wg), dim3(HW * 64), 0, st, bp);
    hipLaunchKernelGGL(part_reduce_kernel<LOSSP>, dim3(1), dim3(256), 0, st, w + W.part, n_wg, w + W.sums);
    hipLaunchKernelGGL(fd_loss_kernel, dim3(1), dim3(64), 0, st, w + W.sums, n, a->reg, a->loss);
    SKR_LAUNCH_CHECK();
    SKR_HIP(mk.mark());
    // ---- the gradient with respect to M: one ordered sum per distinct node into the cleared G
    SKR_HIP(hipMemsetAsync(a->G, 0, static_cast<size_t>(N) * D * sizeof(float), st));
    hipLaunchKernelGGL(rank_triples_kernel<256>, dim3((3 * n + 255) / 256), dim3(256), 0, st, a->users, a->pos, a->neg, n, ordu, ordi);
    const int blocks_u = (n + HW - 1) / HW, blocks_i = (2 * n + HW - 1) / HW;
    hipLaunchKernelGGL(fd_seg_add_kernel, dim3(blocks_u + blocks_i), dim3(HW * 64), 0, st, a->G, a->users, a->pos, a->neg, ordu, ordi, n, n4, U, I,
                       blocks_u, w + W.Gu, w + W.Gi);
    SKR_LAUNCH_CHECK();
    SKR_HIP(mk.mark());
    // ---- the projection backward; the bias cancels in x_m, so its gradient is an exact zero
    for (int m = 0; m < 2; ++m) {
        if (!has[m]) continue;
        const int ld = a->feat_ld[m];
        SKR_HIP(hipMemsetAsync(a->trs_grad[m] + static_cast<int64_t>(D) * ld, 0, D * sizeof(float), st));
        hipLaunchKernelGGL(fd_trs_wgrad_kernel, dim3((ld + 63) / 64), dim3(HW * 64), 0, st, a->feat[m], I, ld, a->pos, a->neg, n, Gm[m],
                           a->trs_grad[m]);
        hipLaunchKernelGGL(fd_seg_rows_kernel, dim3(blocks_i), dim3(HW * 64), 0, st, a->pos, a->neg, ordi, n, I, Gm[m], w + W.Gseg, head);
        hipLaunchKernelGGL(feat_grad_kernel<HW>, dim3((2 * n + 15) / 16, (ld + 64 * HW - 1) / (64 * HW)), dim3(HW * 64), 0, st, w + W.Gseg, head,
                           2 * n, ld, a->trs[m], a->feat_grad[m]);
        SKR_LAUNCH_CHECK();
    }
    SKR_HIP(mk.mark());
    // ---- backward: acc = G; Lu times acc = A'^T acc + G; the last product writes acc / (Lu + 1) into the gradient; then the
    // item rows' path through S^T
    if (Lu == 0) SKR_HIP(hipMemcpyAsync(a->grad, a->G, static_cast<size_t>(N) * D * sizeof(float), hipMemcpyDeviceToDevice, st));
    rc = chain_backward(a->plan_a, a->plan_at, a->G, UO, Lu, a->ping, a->grad, product);
    if (rc != SKR_OK) return rc;
    if (Lm == 0) {
        const unsigned wgs = static_cast<unsigned>(std::min<int64_t>((IO + 255) / 256, 8192));
        hipLaunchKernelGGL(add_kernel<256>, dim3(wgs), dim3(256), 0, st, a->grad + UO, a->G + UO, IO);
        SKR_LAUNCH_CHECK();
    }
    {
        const float* X = a->G + UO;
        for (int k = 1; k <= Lm; ++k) {
            const bool last = k == Lm;
            float* Y = last ? nullptr : a->ping[(k - 1) & 1];
            rc = plain_run(a->plan_st, X, nullptr, Y, last ? a->grad + UO : nullptr, nullptr, stream);
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

int skr_freedom_keys(const float* d_w, int64_t nnz, uint64_t seed, uint64_t epoch, float* d_keys, void* stream) {
    SKR_REQUIRE(d_w && d_keys, "skr_freedom_keys: NULL argument");
    SKR_REQUIRE(nnz >= 0 && nnz <= SKR_FREEDOM_MAX_NNZ, "skr_freedom_keys: 0 <= nnz <= %lld (got %lld)", static_cast<long long>(SKR_FREEDOM_MAX_NNZ),
                static_cast<long long>(nnz));
    if (nnz == 0) return SKR_OK;
    hipLaunchKernelGGL(fd_keys_kernel, dim3(static_cast<unsigned>((nnz + 255) / 256)), dim3(256), 0, skr::as_stream(stream), d_w, nnz, seed, epoch,
                       d_keys);
    SKR_LAUNCH_CHECK();
    return SKR_OK;
}

size_t skr_freedom_select_workspace(int64_t nnz) {
    if (nnz <= 0 || nnz > SKR_FREEDOM_MAX_NNZ) return 0;
    return select_layout(nnz).total;
}

int skr_freedom_select(const float* d_keys, int64_t nnz, int64_t n_keep, uint8_t* d_keep, void* d_work, size_t work_bytes, void* stream) {
    SKR_REQUIRE(d_keys && d_keep && d_work, "skr_freedom_select: NULL argument");
    SKR_REQUIRE(nnz >= 0 && nnz <= SKR_FREEDOM_MAX_NNZ, "skr_freedom_select: 0 <= nnz <= %lld (got %lld)",
                static_cast<long long>(SKR_FREEDOM_MAX_NNZ), static_cast<long long>(nnz));
    SKR_REQUIRE(n_keep >= 0 && n_keep <= nnz, "skr_freedom_select: 0 <= n_keep <= nnz = %lld (got %lld)", static_cast<long long>(nnz),
                static_cast<long long>(n_keep));
    if (nnz == 0) return SKR_OK;
    const SelectLayout L = select_layout(nnz);
    SKR_REQUIRE(work_bytes >= L.total, "skr_freedom_select: work holds %zu bytes, skr_freedom_select_workspace(%lld) asks for %zu", work_bytes,
                static_cast<long long>(nnz), L.total);
    SKR_REQUIRE((reinterpret_cast<uintptr_t>(d_work) & 15) == 0 && (reinterpret_cast<uintptr_t>(d_keys) & 3) == 0,
                "skr_freedom_select: work must be 16-byte aligned");
    hipStream_t st = skr::as_stream(stream);
    if (n_keep == 0 || n_keep == nnz) {
        SKR_HIP(hipMemsetAsync(d_keep, n_keep == 0 ? 0 : 1, static_cast<size_t>(nnz), st));
        return SKR_OK;
    }
    char* wk = static_cast<char*>(d_work);
    int64_t* off = reinterpret_cast<int64_t*>(wk + L.off);
    uint32_t* hist = reinterpret_cast<uint32_t*>(wk + L.hist);
    uint32_t* state = reinterpret_cast<uint32_t*>(wk + L.state);
    uint32_t* cnt = reinterpret_cast<uint32_t*>(wk + L.cnt);
    const uint32_t* bits = reinterpret_cast<const uint32_t*>(d_keys);
    const unsigned blocks = static_cast<unsigned>(L.blocks);
    hipLaunchKernelGGL(fd_sel_init_kernel, dim3(1), dim3(1024), 0, st, hist, state, static_cast<uint32_t>(n_keep));
    for (int pass = 0; pass < 4; ++pass) {
        hipLaunchKernelGGL(fd_sel_hist_kernel, dim3(blocks), dim3(SEL_T), 0, st, bits, nnz, pass, state, hist + 256 * pass);
        hipLaunchKernelGGL(fd_sel_pick_kernel, dim3(1), dim3(64), 0, st, hist + 256 * pass, pass, state);
    }
    hipLaunchKernelGGL(fd_sel_ties_kernel, dim3(blocks), dim3(SEL_T), 0, st, bits, nnz, state, cnt);
    hipLaunchKernelGGL(fd_scan_kernel<uint32_t>, dim3(1), dim3(1024), 0, st, cnt, L.blocks, off);
    hipLaunchKernelGGL(fd_sel_mark_kernel, dim3(blocks), dim3(SEL_T), 0, st, bits, nnz, state, off, d_keep);
    SKR_LAUNCH_CHECK();
    return SKR_OK;
}

size_t skr_freedom_pruned_workspace(int n_users, int n_items, int64_t nnz) {
    if (n_users <= 0 || n_items <= 0 || nnz <= 0 || nnz > SKR_FREEDOM_MAX_NNZ) return 0;
    return prune_layout(static_cast<int64_t>(n_users) + n_items, nnz).total;
}

int skr_freedom_pruned_csr(int n_users, int n_items, int64_t nnz, const int64_t* d_rowptr, const int32_t* d_col, const int64_t* d_rowptr_t,
                           const int32_t* d_col_t, const int32_t* d_perm, const uint8_t* d_keep, int64_t* d_out_rowptr, int32_t* d_out_col,
                           float* d_out_val, int64_t* d_out_rowptr_t, int32_t* d_out_col_t, float* d_out_val_t, int64_t* d_n_kept, void* d_work,
                           size_t work_bytes, void* stream) {
    SKR_REQUIRE(d_rowptr && d_col && d_rowptr_t && d_col_t && d_perm && d_keep && d_out_rowptr && d_out_col && d_out_val && d_out_rowptr_t &&
                    d_out_col_t && d_out_val_t && d_n_kept && d_work,
                "skr_freedom_pruned_csr: NULL argument");
    SKR_REQUIRE(n_users > 0 && n_items > 0, "skr_freedom_pruned_csr: n_users = %d, n_items = %d", n_users, n_items);
    SKR_REQUIRE(nnz >= 0 && nnz <= SKR_FREEDOM_MAX_NNZ, "skr_freedom_pruned_csr: 0 <= nnz <= %lld (got %lld)",
                static_cast<long long>(SKR_FREEDOM_MAX_NNZ), static_cast<long long>(nnz));
    hipStream_t st = skr::as_stream(stream);
    const int64_t N = static_cast<int64_t>(n_users) + n_items;
    if (nnz == 0) {
        SKR_HIP(hipMemsetAsync(d_out_rowptr, 0, static_cast<size_t>(n_users + 1) * sizeof(int64_t), st));
        SKR_HIP(hipMemsetAsync(d_out_rowptr_t, 0, static_cast<size_t>(n_items + 1) * sizeof(int64_t), st));
        SKR_HIP(hipMemsetAsync(d_n_kept, 0, sizeof(int64_t), st));
        return SKR_OK;
    }
    const PruneLayout L = prune_layout(N, nnz);
    SKR_REQUIRE(work_bytes >= L.total, "skr_freedom_pruned_csr: work holds %zu bytes, skr_freedom_pruned_workspace asks for %zu", work_bytes,
                L.total);
    SKR_REQUIRE((reinterpret_cast<uintptr_t>(d_work) & 15) == 0, "skr_freedom_pruned_csr: work must be 16-byte aligned");
    char* wk = static_cast<char*>(d_work);
    uint8_t* keep_t = reinterpret_cast<uint8_t*>(wk + L.keep_t);
    int32_t* cnt = reinterpret_cast<int32_t*>(wk + L.cnt);
    float* inv = reinterpret_cast<float*>(wk + L.inv);
    SKR_HIP(hipMemsetAsync(keep_t, 0, static_cast<size_t>(nnz), st));
    hipLaunchKernelGGL(fd_keep_t_kernel, dim3(static_cast<unsigned>((nnz + 255) / 256)), dim3(256), 0, st, d_keep, d_perm, nnz, keep_t);
    const unsigned row_blocks = static_cast<unsigned>((N + HW - 1) / HW);
    hipLaunchKernelGGL(fd_row_count_kernel, dim3(row_blocks), dim3(HW * 64), 0, st, d_rowptr, d_rowptr_t, d_keep, keep_t, n_users, n_items, nnz, cnt,
                       inv);
    hipLaunchKernelGGL(fd_scan_kernel<int32_t>, dim3(1), dim3(1024), 0, st, cnt, static_cast<int64_t>(n_users), d_out_rowptr);
    hipLaunchKernelGGL(fd_scan_kernel<int32_t>, dim3(1), dim3(1024), 0, st, cnt + n_users, static_cast<int64_t>(n_items), d_out_rowptr_t);
    hipLaunchKernelGGL(fd_fill_kernel, dim3(row_blocks), dim3(HW * 64), 0, st, d_rowptr, d_col, d_rowptr_t, d_col_t, d_keep, keep_t, n_users, n_items,
                       nnz, inv, d_out_rowptr, d_out_col, d_out_val, d_out_rowptr_t, d_out_col_t, d_out_val_t);
    SKR_LAUNCH_CHECK();
    SKR_HIP(hipMemcpyAsync(d_n_kept, d_out_rowptr + n_users, sizeof(int64_t), hipMemcpyDeviceToDevice, st));
    return SKR_OK;
}

size_t skr_freedom_workspace(int n) {
    if (n <= 0 || n > MAXB) return 0;
    return static_cast<size_t>(step_layout(n).total) * sizeof(float);
}

int skr_freedom_step(const skr_freedom_step_args* args, void* stream) { return run_step(args, stream, nullptr); }

int skr_freedom_step_timed(const skr_freedom_step_args* args, void* stream, float* h_ms) {
    SKR_REQUIRE(h_ms != nullptr, "skr_freedom_step_timed: NULL argument");
    return run_step(args, stream, h_ms);
}

}  // extern "C"
