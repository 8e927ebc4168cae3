// train.hip -- T rows: BPR lookup-and-score forward/backward (K1), CSR propagation (K3), LayerGCN's refinement, row
// gather / scatter and the multi-GPU gradient pack / unpack.  The dense Adam -- K2, its temporally blocked form K2b and the
// weight-decay variants K2w -- is in adam.hip; K2c, the BPR batch and the hot rows' Adam in one launch, in bpr_fused.hip.
//
// Replaces the stock torch ops the reference issues per step (no native code there):
//   recommender/BPRMF.py:77-82,114-127   gathers, inner_product, bpr_loss.sum(), l2_loss, backward, Adam
//   recommender/LightGCN.py:89-100       torch.sparse.mm per layer + stack/mean
//   recommender/LayerGCN.py:207-220      sparse.mm + cosine_similarity re-weighting + layer sum
//   utils/torch.py:20-21,62-74           inner_product, bpr_loss, l2_loss
//
// Every kernel maps the d = 64 embedding row onto the 64 lanes of one wavefront: a row is one
// coalesced 256-byte access, dot products are wave reductions, gradient scatter-adds are one
// 256-byte global_atomic_add_f32 per row (the shape the memory-side atomic units like).
#include "skr_common.h"

#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>

namespace {

constexpr int D = 64;

// ------------------------------------------------------------------------------------------------
// K1: fused BPR batch (forward + backward)
// ------------------------------------------------------------------------------------------------
constexpr int BPR_WAVES = 4;

// C: the row is 64 C floats wide (embedding widths beyond 64, zero-padded to a multiple of 64 by the caller); lane l owns
// floats l, l + 64, ...: every access is still a coalesced 256-byte one
template <int C>
__global__ __launch_bounds__(BPR_WAVES * 64) void bpr_step_kernel(
    const float* __restrict__ P, const float* __restrict__ Q, const float* __restrict__ bias,
    const float* __restrict__ RP, const float* __restrict__ RQ, const int32_t* __restrict__ u_ids,
    const int32_t* __restrict__ i_ids, const int32_t* __restrict__ j_ids, int n, float loss_scale, float reg,
    float reg_scale, float* __restrict__ gP, float* __restrict__ gQ, float* __restrict__ gb, float* __restrict__ gRP,
    float* __restrict__ gRQ, float* __restrict__ loss, uint8_t* __restrict__ touch, const float* touch_base,
    int loss_slots, int shard_world, int shard_rank, float grad_scale) {
    __shared__ float s_loss[BPR_WAVES], s_l2[BPR_WAVES];
    // mark the 64-float gradient block that starts at `a` as touched (one lane per row is enough)
    // (a byte that is already non-zero -- 1, or the sticky 2 -- is left alone)
    auto mark = [&](const float* a) {
        uint8_t* t = &touch[(a - touch_base) >> 6];
        if (*t == 0) *t = 1;
    };
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float acc_loss = 0.0f, acc_l2 = 0.0f;
    const float rs = reg * reg_scale;
    const bool same_tables = RP == P && RQ == Q && gRP == gP && gRQ == gQ;
    for (int b = blockIdx.x * BPR_WAVES + wv; b < n; b += gridDim.x * BPR_WAVES) {
        int64_t u = u_ids[b];
        const int64_t i = i_ids[b], j = j_ids[b];
        if (shard_world > 1) {      // a GLOBAL batch on a user-sharded rank: only the triples of the users this rank owns
            if (u % shard_world != shard_rank) continue;
            u /= shard_world;       // row of the local user table
        }
        constexpr int DW = D * C;
        float pu[C], qi[C], qj[C];
        float di = 0.0f, dj = 0.0f;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            pu[c] = P[u * DW + c * D + lane]; qi[c] = Q[i * DW + c * D + lane]; qj[c] = Q[j * DW + c * D + lane];
            di += pu[c] * qi[c];
            dj += pu[c] * qj[c];
        }
        // x_ui - x_uj; the two inner products are reduced separately like inner_product() does
        float xi = skr::wave_sum(di), xj = skr::wave_sum(dj);
        float bi = 0.0f, bj = 0.0f;
        if (bias) {
            bi = bias[i];
            bj = bias[j];
            xi += bi;
            xj += bj;
        }
        const float x = xi - xj;
        // -logsigmoid(x) = -(min(0,x) - log1p(exp(-|x|)))   (torch's log_sigmoid forward)
        const float z = expf(-fabsf(x));
        const float l = -(fminf(0.0f, x) - log1pf(z));
        // d/dx = -sigmoid(-x)
        const float sig_neg = (x >= 0.0f) ? z / (1.0f + z) : 1.0f / (1.0f + z);
        // grad_scale: an extra factor on the SCORE part of the gradient only (LightGCN: dL/dE-bar enters the backward
        // propagation as H = dL/dE-bar / (K + 1); scaling here saves a pass over the [N, 64] buffer)
        const float c = -sig_neg * loss_scale * grad_scale;
        float sq;
        if (same_tables) {
            // BPRMF: the regulariser rows ARE the score rows -- no second read, one atomic per row for both gradient parts
            float sl = 0.0f;
#pragma unroll
            for (int c_ = 0; c_ < C; ++c_) {
                sl += pu[c_] * pu[c_] + qi[c_] * qi[c_] + qj[c_] * qj[c_];
                atomicAdd(&gP[u * DW + c_ * D + lane], c * (qi[c_] - qj[c_]) + rs * pu[c_]);
                atomicAdd(&gQ[i * DW + c_ * D + lane], c * pu[c_] + rs * qi[c_]);
                atomicAdd(&gQ[j * DW + c_ * D + lane], -c * pu[c_] + rs * qj[c_]);
            }
            sq = skr::wave_sum(sl);
        } else {
            // score-part gradients
            float sl = 0.0f;
#pragma unroll
            for (int c_ = 0; c_ < C; ++c_) {
                atomicAdd(&gP[u * DW + c_ * D + lane], c * (qi[c_] - qj[c_]));
                atomicAdd(&gQ[i * DW + c_ * D + lane], c * pu[c_]);
                atomicAdd(&gQ[j * DW + c_ * D + lane], -c * pu[c_]);
                // regulariser rows (other tables than the score tables: LightGCN's ego embeddings)
                const float ru = RP[u * DW + c_ * D + lane], ri = RQ[i * DW + c_ * D + lane], rj = RQ[j * DW + c_ * D + lane];
                sl += ru * ru + ri * ri + rj * rj;
                if (rs != 0.0f) {
                    atomicAdd(&gRP[u * DW + c_ * D + lane], rs * ru);
                    atomicAdd(&gRQ[i * DW + c_ * D + lane], rs * ri);
                    atomicAdd(&gRQ[j * DW + c_ * D + lane], rs * rj);
                }
            }
            sq = skr::wave_sum(sl);
        }
        if (bias) {
            sq += bi * bi + bj * bj;
            if (lane == 0 && gb) {
                atomicAdd(&gb[i], c + rs * bi);
                atomicAdd(&gb[j], -c + rs * bj);
            }
        }
        if (touch && lane < C) {      // lane c marks the c-th 64-float block of each row
            mark(&gP[u * DW + lane * D]); mark(&gQ[i * DW + lane * D]); mark(&gQ[j * DW + lane * D]);
            if (rs != 0.0f) { mark(&gRP[u * DW + lane * D]); mark(&gRQ[i * DW + lane * D]); mark(&gRQ[j * DW + lane * D]); }
        }
        if (touch && lane == 0) {
            if (bias && gb) { mark(&gb[i]); mark(&gb[j]); }
        }
        acc_loss += l;
        acc_l2 += 0.5f * sq;
    }
    if (lane == 0) {
        s_loss[wv] = acc_loss;
        s_l2[wv] = acc_l2;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float a = 0.0f, b2 = 0.0f;
        for (int w = 0; w < BPR_WAVES; ++w) {
            a += s_loss[w];
            b2 += s_l2[w];
        }
        // same-address float atomics serialise (~20 ns each): 256 workgroups on ONE pair of words cost 4.5 us of a
        // 10.9 us launch (by ablation).  loss_slots > 1 spreads them over that many pairs; the caller adds the pairs up.
        const int sl = 2 * (static_cast<int>(blockIdx.x) % loss_slots);
        atomicAdd(&loss[sl], a * loss_scale);
        atomicAdd(&loss[sl + 1], b2);
    }
}

// ------------------------------------------------------------------------------------------------
// K3: CSR SpMM, d = 64, nnz-balanced: one wavefront per CH consecutive non-zeros
// ------------------------------------------------------------------------------------------------
constexpr int SP_CH = 512;     // non-zeros per wavefront
constexpr int SP_WAVES = 4;

__device__ __forceinline__ int64_t row_of(const int64_t* __restrict__ rowptr, int n_rows, int64_t e) {
    int64_t lo = 0, hi = n_rows - 1;  // largest r with rowptr[r] <= e
    while (lo < hi) {
        int64_t mid = (lo + hi + 1) >> 1;
        if (rowptr[mid] <= e) lo = mid; else hi = mid - 1;
    }
    return lo;
}
__device__ __forceinline__ bool row_is_split(int64_t rb, int64_t re) { return (rb / SP_CH) != ((re - 1) / SP_CH); }

// rows no chunk completes: empty rows get their final value here, split rows are zeroed for atomics
__global__ void spmm_prep_kernel(int n_rows, const int64_t* __restrict__ rowptr, const float* __restrict__ addend,
                                 float* __restrict__ Y, float* __restrict__ accum, float accum_scale, int ld) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x) >> 6;
    if (r >= n_rows) return;
    const int64_t rb = rowptr[r], re = rowptr[r + 1];
    if (re == rb) {
        const float y = addend ? addend[r * ld + lane] : 0.0f;
        Y[r * ld + lane] = y;
        if (accum) accum[r * ld + lane] += accum_scale * y;
    } else if (row_is_split(rb, re)) {
        Y[r * ld + lane] = 0.0f;
    }
}

__global__ __launch_bounds__(SP_WAVES * 64) void spmm_main_kernel(int n_rows, const int64_t* __restrict__ rowptr,
                                                                  const int32_t* __restrict__ col,
                                                                  const float* __restrict__ val,
                                                                  const float* __restrict__ X,
                                                                  const float* __restrict__ addend, float* __restrict__ Y,
                                                                  float* __restrict__ accum, float accum_scale,
                                                                  int64_t nnz, int ld) {
    const int lane = threadIdx.x & 63;
    const int64_t w = blockIdx.x * static_cast<int64_t>(SP_WAVES) + (threadIdx.x >> 6);
    const int64_t e0 = w * SP_CH;
    if (e0 >= nnz) return;
    const int64_t e1 = (e0 + SP_CH < nnz) ? e0 + SP_CH : nnz;
    int64_t r = row_of(rowptr, n_rows, e0);
    int64_t e = e0;
    while (e < e1) {
        while (rowptr[r + 1] <= e) ++r;  // skip rows that ended (empty rows included)
        const int64_t rb = rowptr[r], re = rowptr[r + 1];
        const int64_t se = re < e1 ? re : e1;
        float acc = 0.0f;
        for (int64_t c0 = e; c0 < se; c0 += 64) {
            const int m = static_cast<int>(se - c0 < 64 ? se - c0 : 64);
            int cl = 0;
            float vl = 0.0f;
            if (lane < m) {
                cl = col[c0 + lane];
                vl = val[c0 + lane];
            }
            int k = 0;
            for (; k + 4 <= m; k += 4) {  // four independent 256-byte row gathers in flight
                const int c_0 = __shfl(cl, k), c_1 = __shfl(cl, k + 1), c_2 = __shfl(cl, k + 2), c_3 = __shfl(cl, k + 3);
                const float x0 = X[static_cast<int64_t>(c_0) * ld + lane], x1 = X[static_cast<int64_t>(c_1) * ld + lane];
                const float x2 = X[static_cast<int64_t>(c_2) * ld + lane], x3 = X[static_cast<int64_t>(c_3) * ld + lane];
                acc = fmaf(__shfl(vl, k), x0, acc);
                acc = fmaf(__shfl(vl, k + 1), x1, acc);
                acc = fmaf(__shfl(vl, k + 2), x2, acc);
                acc = fmaf(__shfl(vl, k + 3), x3, acc);
            }
            for (; k < m; ++k) {
                const int c_0 = __shfl(cl, k);
                acc = fmaf(__shfl(vl, k), X[static_cast<int64_t>(c_0) * ld + lane], acc);
            }
        }
        if (!row_is_split(rb, re)) {  // this wave saw the whole row: finish it here
            float y = acc;
            if (addend) y += addend[r * ld + lane];
            Y[r * ld + lane] = y;
            if (accum) accum[r * ld + lane] += accum_scale * y;
        } else {
            atomicAdd(&Y[r * ld + lane], acc);
        }
        e = se;
    }
}

__global__ void spmm_fix_kernel(int n_rows, const int64_t* __restrict__ rowptr, const float* __restrict__ addend,
                                float* __restrict__ Y, float* __restrict__ accum, float accum_scale, int ld) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x) >> 6;
    if (r >= n_rows) return;
    const int64_t rb = rowptr[r], re = rowptr[r + 1];
    if (re > rb && row_is_split(rb, re)) {
        float y = Y[r * ld + lane];
        if (addend) {
            y += addend[r * ld + lane];
            Y[r * ld + lane] = y;
        }
        if (accum) accum[r * ld + lane] += accum_scale * y;
    }
}

// ------------------------------------------------------------------------------------------------
// LayerGCN refinement (LayerGCN.py:214-216) forward / backward, one wavefront per row
// ------------------------------------------------------------------------------------------------
constexpr float COS_EPS = 1e-8f;  // F.cosine_similarity default

template <int C>
__global__ void refine_fwd_kernel(const float* __restrict__ Y, const float* __restrict__ E, int64_t n_rows,
                                  float* __restrict__ Z, float* __restrict__ w_out, float* __restrict__ accum) {
    constexpr int DW = D * C;
    const int lane = threadIdx.x & 63;
    const int64_t r = (blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x) >> 6;
    if (r >= n_rows) return;
    float y[C], e[C];
    float sy = 0.0f, se = 0.0f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        y[c] = Y[r * DW + c * D + lane]; e[c] = E[r * DW + c * D + lane];
        sy += y[c] * y[c];
        se += e[c] * e[c];
    }
    const float ny = fmaxf(sqrtf(skr::wave_sum(sy)), COS_EPS);
    const float ne = fmaxf(sqrtf(skr::wave_sum(se)), COS_EPS);
    float sw = 0.0f;
#pragma unroll
    for (int c = 0; c < C; ++c) sw += (y[c] / ny) * (e[c] / ne);
    const float w = skr::wave_sum(sw);
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float z = w * y[c];
        Z[r * DW + c * D + lane] = z;
        if (accum) accum[r * DW + c * D + lane] += z;
    }
    if (lane == 0) w_out[r] = w;
}

template <int C>
__global__ void refine_bwd_kernel(const float* __restrict__ Y, const float* __restrict__ E, const float* __restrict__ w_in,
                                  const float* __restrict__ dZ, int64_t n_rows, float* __restrict__ dY,
                                  float* __restrict__ dE, const uint8_t* __restrict__ row_mask, int zero_skipped) {
    constexpr int DW = D * C;
    const int lane = threadIdx.x & 63;
    const int64_t r = (blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x) >> 6;
    if (r >= n_rows) return;
    if (row_mask && !row_mask[r]) {            // dZ_r is zero: dY_r is zero and nothing is added to dE_r
        if (zero_skipped) {
#pragma unroll
            for (int c = 0; c < C; ++c) dY[r * DW + c * D + lane] = 0.0f;
        }
        return;
    }
    float y[C], e[C], dz[C];
    float sy = 0.0f, se = 0.0f, sd = 0.0f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        y[c] = Y[r * DW + c * D + lane]; e[c] = E[r * DW + c * D + lane]; dz[c] = dZ[r * DW + c * D + lane];
        sy += y[c] * y[c];
        se += e[c] * e[c];
        sd += dz[c] * y[c];
    }
    const float w = w_in[r];
    const float nyr = sqrtf(skr::wave_sum(sy)), ner = sqrtf(skr::wave_sum(se));
    const float ny = fmaxf(nyr, COS_EPS), ne = fmaxf(ner, COS_EPS);
    const float dw = skr::wave_sum(sd);
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float yh = y[c] / ny, eh = e[c] / ne;
        // d(yh)/dy = (I - yh yh^T)/ny when the norm is not clamped, I/eps when it is (clamp_min has zero slope)
        const float gy = (nyr > COS_EPS) ? (eh - w * yh) / ny : eh / ny;
        const float ge = (ner > COS_EPS) ? (yh - w * eh) / ne : yh / ne;
        dY[r * DW + c * D + lane] = w * dz[c] + dw * gy;
        dE[r * DW + c * D + lane] += dw * ge;
    }
}

// rows whose mask byte is set are zeroed (and the byte cleared): restores the "all zero" state of a buffer of which only a
// batch's rows were written, without a fill of the whole buffer
__global__ void clear_marked_rows_kernel(uint8_t* __restrict__ mask, int64_t n_rows, int clear_mask, float* __restrict__ table, int dim) {
    const int lane = threadIdx.x & 63;
    const int64_t r0 = ((blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x) >> 6) * 64;     // 64 rows per wavefront
    if (r0 >= n_rows) return;
    const bool set = r0 + lane < n_rows && mask[r0 + lane] != 0;
    unsigned long long b = __ballot(set);
    if (set && clear_mask) mask[r0 + lane] = 0;
    while (b) {
        const int j = __ffsll(static_cast<long long>(b)) - 1;
        b &= b - 1;
        for (int c = lane; c < dim; c += 64) table[(r0 + j) * dim + c] = 0.0f;
    }
}

__global__ void gather_rows_kernel(const float* __restrict__ table, const int32_t* __restrict__ idx, int64_t n,
                                   float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t k = (blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x) >> 6;
    if (k >= n) return;
    out[k * D + lane] = table[static_cast<int64_t>(idx[k]) * D + lane];
}
// any row width (the GRU4RecPlus tables: 32 / 64 / 128 floats, biases: 1): one thread per element
__global__ void gather_rows_any_kernel(const float* __restrict__ table, const int32_t* __restrict__ idx, int64_t n, int dim,
                                       float* __restrict__ out) {
    const int64_t e = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
    if (e >= n * dim) return;
    const int64_t k = e / dim;
    out[e] = table[static_cast<int64_t>(idx[k]) * dim + (e - k * dim)];
}
__global__ void scatter_rows_any_kernel(const float* __restrict__ src, const int32_t* __restrict__ idx, int64_t n, int dim,
                                        float* __restrict__ table) {
    const int64_t e = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
    if (e >= n * dim) return;
    const int64_t k = e / dim;
    if (idx[k] < 0) return;
    table[static_cast<int64_t>(idx[k]) * dim + (e - k * dim)] = src[e];
}

// table[idx[k]] = src[k]; negative ids are skipped; duplicate ids must carry identical rows
__global__ void scatter_rows_kernel(const float* __restrict__ src, const int32_t* __restrict__ idx, int64_t n,
                                    float* __restrict__ table) {
    const int lane = threadIdx.x & 63;
    const int64_t k = (blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x) >> 6;
    if (k >= n || idx[k] < 0) return;
    table[static_cast<int64_t>(idx[k]) * D + lane] = src[k * D + lane];
}

// out[i] = ((in[0][i] + in[1][i]) + in[2][i]) + ...   -- the ranks' blocks added in rank order, the same bits on every rank
__global__ void sum_blocks_kernel(const float* __restrict__ in, int n_blocks, int64_t n, float* __restrict__ out) {
    const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
    for (int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; i < n; i += stride) {
        float acc = in[i];
        for (int b = 1; b < n_blocks; ++b) acc += in[b * n + i];
        out[i] = acc;
    }
}

__global__ void axpy_kernel(float a, const float* __restrict__ x, float* __restrict__ y, int64_t n) {
    const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
    for (int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; i < n; i += stride)
        y[i] = fmaf(a, x[i], y[i]);
}

__global__ void scale_copy_kernel(float a, const float* __restrict__ x, float* __restrict__ y, int64_t n) {
    const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
    for (int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; i < n; i += stride) y[i] = a * x[i];
}

__global__ void scale_kernel(float a, float* __restrict__ x, int64_t n) {
    const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
    for (int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; i < n; i += stride) x[i] *= a;
}

inline unsigned rows_to_blocks(int64_t n_rows) { return static_cast<unsigned>((n_rows * 64 + 255) / 256); }

// ------------------------------------------------------------------------------------------------
// Sparse exchange of the replicated item table's gradient (multi-GPU BPRMF).  A step touches at
// most 2 * batch of the I item rows, so the ranks exchange packed rows [id | dV (64) | db] instead of
// all-reducing the dense [I, 65] block (26 MB at I = 100 k): pack -> all-gather -> unpack.
// ------------------------------------------------------------------------------------------------
constexpr int PK_W = D + 2;   // floats per packed row

// one wavefront per slot; ids are unique within a call or negative (empty slot).  The dense rows are
// cleared after packing so that every rank re-accumulates all contributions in the same (rank) order.
__global__ __launch_bounds__(256) void pack_grad_rows_kernel(const int32_t* __restrict__ ids, int n, float* __restrict__ gV,
                                                             float* __restrict__ gb, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= n) return;
    const int id = ids[k];
    float* o = out + static_cast<int64_t>(k) * PK_W;
    if (id < 0) {
        if (lane == 0) o[0] = __int_as_float(-1);
        return;
    }
    float* src = gV + static_cast<int64_t>(id) * D;
    o[1 + lane] = src[lane];
    src[lane] = 0.0f;
    if (lane == 0) {
        o[0] = __int_as_float(id);
        o[1 + D] = gb ? gb[id] : 0.0f;
        if (gb) gb[id] = 0.0f;
    }
}

// dense += packed rows of ONE rank (unique ids: plain read-modify-write, no atomics, deterministic)
__global__ __launch_bounds__(256) void unpack_grad_rows_kernel(const float* __restrict__ in, int n, float* __restrict__ gV,
                                                               float* __restrict__ gb, uint8_t* __restrict__ touch,
                                                               const float* touch_base) {
    const int lane = threadIdx.x & 63;
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= n) return;
    const float* r = in + static_cast<int64_t>(k) * PK_W;
    const int id = __float_as_int(r[0]);
    if (id < 0) return;
    float* dst = gV + static_cast<int64_t>(id) * D;
    dst[lane] += r[1 + lane];
    if (lane == 0) {
        if (gb) gb[id] += r[1 + D];
        if (touch) {
            uint8_t* t = &touch[(dst - touch_base) >> 6];
            if (*t == 0) *t = 1;
            if (gb) {
                uint8_t* tb = &touch[(gb + id - touch_base) >> 6];
                if (*tb == 0) *tb = 1;
            }
        }
    }
}

// The same sum in ONE launch, for packs whose valid ids ascend with the empty slots last.  One wavefront per (rank, slot):
// it looks the id up in every other rank's id column (64 lanes probe a stride, then the 32 entries of the stride that
// can hold it); the lowest rank that holds the id owns it and adds the ranks' rows to the dense row in rank order --
// the order of the per-rank launches above, so the results are the same bits -- with a plain read-modify-write.
constexpr int UP_MAX_RANKS = 16;

__device__ __forceinline__ int pack_find(const float* __restrict__ col0, int n, int id, int lane) {
    // col0: &in[rank][0][0]; ids sit PK_W floats apart.  -> slot of `id`, or -1
    auto key = [&](int j) -> int {
        const int v = j < n ? __float_as_int(col0[static_cast<int64_t>(j) * PK_W]) : -1;
        return v < 0 ? 0x7fffffff : v;
    };
    const int stride = (n + 63) >> 6;                       // 64 probes cover the column
    const int k0 = key(lane * stride);
    // first probe whose key exceeds id -> the stride before it may hold id
    const uint64_t gt = __builtin_amdgcn_ballot_w64(k0 > id);
    const int first_gt = gt ? __builtin_ctzll(gt) : 64;
    if (first_gt == 0) return -1;
    const int base = (first_gt - 1) * stride;
    int found = -1;
    for (int off = 0; off < stride; off += 64) {
        const int j = base + off + lane;
        const bool hit = off + lane < stride && key(j) == id;
        const uint64_t hb = __builtin_amdgcn_ballot_w64(hit);
        if (hb) found = base + off + __builtin_ctzll(hb);
    }
    return found;
}

__global__ __launch_bounds__(256) void unpack_grad_rows_sorted_kernel(const float* __restrict__ in, int n, int n_ranks,
                                                                      float* __restrict__ gV, float* __restrict__ gb,
                                                                      uint8_t* __restrict__ touch, const float* touch_base) {
    const int lane = threadIdx.x & 63;
    const int64_t w = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= static_cast<int64_t>(n) * n_ranks) return;
    const int r = static_cast<int>(w / n), k = static_cast<int>(w % n);
    const float* mine = in + (static_cast<int64_t>(r) * n + k) * PK_W;
    const int id = __float_as_int(mine[0]);
    if (id < 0) return;
    int pos[UP_MAX_RANKS];
#pragma unroll
    for (int q = 0; q < UP_MAX_RANKS; ++q)
        pos[q] = (q < n_ranks && q != r) ? pack_find(in + static_cast<int64_t>(q) * n * PK_W, n, id, lane) : -1;
#pragma unroll
    for (int q = 0; q < UP_MAX_RANKS; ++q)
        if (q < r && pos[q] >= 0) return;                    // a lower rank holds the id: that wavefront owns it
    float* dst = gV + static_cast<int64_t>(id) * D;
    float acc = dst[lane] + mine[1 + lane];
    float accb = 0.0f;
    if (gb && lane == 0) accb = gb[id] + mine[1 + D];
#pragma unroll
    for (int q = 0; q < UP_MAX_RANKS; ++q) {
        if (q > r && pos[q] >= 0) {
            const float* row = in + (static_cast<int64_t>(q) * n + pos[q]) * PK_W;
            acc += row[1 + lane];
            if (gb && lane == 0) accb += row[1 + D];
        }
    }
    dst[lane] = acc;
    if (lane == 0) {
        if (gb) gb[id] = accb;
        if (touch) {
            uint8_t* t = &touch[(dst - touch_base) >> 6];
            if (*t == 0) *t = 1;
            if (gb) {
                uint8_t* tb = &touch[(gb + id - touch_base) >> 6];
                if (*tb == 0) *tb = 1;
            }
        }
    }
}

}  // namespace

extern "C" {

static int bpr_step_launch(const float* d_P, const float* d_Q, const float* d_bias, const float* d_RP, const float* d_RQ,
                 const int32_t* d_u, const int32_t* d_i, const int32_t* d_j, int n, float loss_scale, float reg,
                 float reg_scale, float* d_gP, float* d_gQ, float* d_gb, float* d_gRP, float* d_gRQ, float* d_loss,
                 uint8_t* d_touch, const float* d_touch_base, int loss_slots, void* stream, int shard_world = 1,
                 int shard_rank = 0, float grad_scale = 1.0f, int dim = D) {
    SKR_REQUIRE(d_P && d_Q && d_RP && d_RQ && d_u && d_i && d_j && d_gP && d_gQ && d_gRP && d_gRQ && d_loss,
                "skr_bpr_step: NULL argument");
    SKR_REQUIRE(shard_world >= 1 && shard_rank >= 0 && shard_rank < shard_world, "skr_bpr_step_sharded: rank %d of %d", shard_rank,
                shard_world);
    SKR_REQUIRE(n >= 0, "skr_bpr_step: negative batch size");
    SKR_REQUIRE(!d_touch || d_touch_base, "skr_bpr_step: d_touch needs d_touch_base");
    SKR_REQUIRE(dim == 64 || dim == 128 || dim == 192 || dim == 256, "skr_bpr_step: dim must be 64, 128, 192 or 256 (got %d); pad narrower "
                "rows with zeros", dim);
    if (n == 0) return SKR_OK;
    int blocks = (n + BPR_WAVES - 1) / BPR_WAVES;
    if (blocks > 4096) blocks = 4096;
#define SKR_BPR_LAUNCH(C_)                                                                                                       \
    hipLaunchKernelGGL(bpr_step_kernel<C_>, dim3(blocks), dim3(BPR_WAVES * 64), 0, skr::as_stream(stream), d_P, d_Q, d_bias,     \
                       d_RP, d_RQ, d_u, d_i, d_j, n, loss_scale, reg, reg_scale, d_gP, d_gQ, d_gb, d_gRP, d_gRQ, d_loss,        \
                       d_touch, d_touch_base, loss_slots, shard_world, shard_rank, grad_scale)
    switch (dim / 64) {
        case 1: SKR_BPR_LAUNCH(1); break;
        case 2: SKR_BPR_LAUNCH(2); break;
        case 3: SKR_BPR_LAUNCH(3); break;
        default: SKR_BPR_LAUNCH(4); break;
    }
#undef SKR_BPR_LAUNCH
    SKR_LAUNCH_CHECK();
    return SKR_OK;
}

int skr_bpr_step_dim(const float* d_P, const float* d_Q, const float* d_bias, const float* d_RP, const float* d_RQ,
                     const int32_t* d_u, const int32_t* d_i, const int32_t* d_j, int n, int dim, float loss_scale, float reg,
                     float reg_scale, float* d_gP, float* d_gQ, float* d_gb, float* d_gRP, float* d_gRQ, float* d_loss,
                     int loss_slots, uint8_t* d_touch, const float* d_touch_base, float grad_scale, void* stream) {
    SKR_REQUIRE(loss_slots == 1 || loss_slots == SKR_LOSS_SLOTS, "skr_bpr_step_dim: loss_slots must be 1 or %d", SKR_LOSS_SLOTS);
    return bpr_step_launch(d_P, d_Q, d_bias, d_RP, d_RQ, d_u, d_i, d_j, n, loss_scale, reg, reg_scale, d_gP, d_gQ, d_gb, d_gRP,
                           d_gRQ, d_loss, d_touch, d_touch_base, loss_slots, stream, 1, 0, grad_scale, dim);
}

int skr_bpr_step(const float* d_P, const float* d_Q, const float* d_bias, const float* d_RP, const float* d_RQ,
                 const int32_t* d_u, const int32_t* d_i, const int32_t* d_j, int n, float loss_scale, float reg,
                 float reg_scale, float* d_gP, float* d_gQ, float* d_gb, float* d_gRP, float* d_gRQ, float* d_loss,
                 uint8_t* d_touch, const float* d_touch_base, void* stream) {
    return bpr_step_launch(d_P, d_Q, d_bias, d_RP, d_RQ, d_u, d_i, d_j, n, loss_scale, reg, reg_scale, d_gP, d_gQ, d_gb, d_gRP,
                           d_gRQ, d_loss, d_touch, d_touch_base, 1, stream);
}

int skr_bpr_step_sharded(const float* d_P, const float* d_Q, const float* d_bias, const float* d_RP, const float* d_RQ,
                         const int32_t* d_u, const int32_t* d_i, const int32_t* d_j, int n, float loss_scale, float reg,
                         float reg_scale, float* d_gP, float* d_gQ, float* d_gb, float* d_gRP, float* d_gRQ, float* d_loss,
                         uint8_t* d_touch, const float* d_touch_base, int shard_world, int shard_rank, float grad_scale,
                         void* stream) {
    return bpr_step_launch(d_P, d_Q, d_bias, d_RP, d_RQ, d_u, d_i, d_j, n, loss_scale, reg, reg_scale, d_gP, d_gQ, d_gb, d_gRP,
                           d_gRQ, d_loss, d_touch, d_touch_base, 1, stream, shard_world, shard_rank, grad_scale);
}

int skr_bpr_step_spread(const float* d_P, const float* d_Q, const float* d_bias, const float* d_RP, const float* d_RQ,
                        const int32_t* d_u, const int32_t* d_i, const int32_t* d_j, int n, float loss_scale, float reg,
                        float reg_scale, float* d_gP, float* d_gQ, float* d_gb, float* d_gRP, float* d_gRQ, float* d_loss64,
                        uint8_t* d_touch, const float* d_touch_base, void* stream) {
    return bpr_step_launch(d_P, d_Q, d_bias, d_RP, d_RQ, d_u, d_i, d_j, n, loss_scale, reg, reg_scale, d_gP, d_gQ, d_gb, d_gRP,
                           d_gRQ, d_loss64, d_touch, d_touch_base, SKR_LOSS_SLOTS, stream);
}

int skr_csr_spmm(int n_rows, const int64_t* d_rowptr, const int32_t* d_col, const float* d_val, const float* d_X,
                 int dim, int64_t nnz, const float* d_addend, float* d_Y, float* d_accum, float accum_scale,
                 void* stream) {
    return skr_csr_spmm_strided(n_rows, d_rowptr, d_col, d_val, d_X, dim, D, nnz, d_addend, d_Y, d_accum, accum_scale, stream);
}

int skr_csr_spmm_strided(int n_rows, const int64_t* d_rowptr, const int32_t* d_col, const float* d_val, const float* d_X,
                         int dim, int ld, int64_t nnz, const float* d_addend, float* d_Y, float* d_accum, float accum_scale,
                         void* stream) {
    SKR_REQUIRE(d_rowptr && d_col && d_val && d_X && d_Y, "skr_csr_spmm: NULL argument");
    SKR_REQUIRE(dim == D, "skr_csr_spmm: dim must be 64 (got %d): wider tables are multiplied in 64-column slices (ld)", dim);
    SKR_REQUIRE(ld >= D, "skr_csr_spmm: the row stride must be at least 64 floats (got %d)", ld);
    SKR_REQUIRE(n_rows >= 0 && nnz >= 0, "skr_csr_spmm: negative size");
    SKR_REQUIRE(d_Y != d_X, "skr_csr_spmm: in-place propagation is not supported");
    if (n_rows == 0) return SKR_OK;
    hipStream_t st = skr::as_stream(stream);
    hipLaunchKernelGGL(spmm_prep_kernel, dim3(rows_to_blocks(n_rows)), dim3(256), 0, st, n_rows, d_rowptr, d_addend, d_Y,
                       d_accum, accum_scale, ld);
    SKR_LAUNCH_CHECK();
    if (nnz > 0) {
        const int64_t waves = (nnz + SP_CH - 1) / SP_CH;
        hipLaunchKernelGGL(spmm_main_kernel, dim3(static_cast<unsigned>((waves + SP_WAVES - 1) / SP_WAVES)),
                           dim3(SP_WAVES * 64), 0, st, n_rows, d_rowptr, d_col, d_val, d_X, d_addend, d_Y, d_accum,
                           accum_scale, nnz, ld);
        SKR_LAUNCH_CHECK();
        hipLaunchKernelGGL(spmm_fix_kernel, dim3(rows_to_blocks(n_rows)), dim3(256), 0, st, n_rows, d_rowptr, d_addend,
                           d_Y, d_accum, accum_scale, ld);
        SKR_LAUNCH_CHECK();
    }
    return SKR_OK;
}

int skr_layer_refine_fwd(const float* d_Y, const float* d_E, int64_t n_rows, int dim, float* d_Z, float* d_w,
                         float* d_accum, void* stream) {
    SKR_REQUIRE(d_Y && d_E && d_Z && d_w, "skr_layer_refine_fwd: NULL argument");
    SKR_REQUIRE(dim == 64 || dim == 128 || dim == 192 || dim == 256, "skr_layer_refine_fwd: dim must be 64, 128, 192 or 256 (got %d)", dim);
    if (n_rows <= 0) return SKR_OK;
#define SKR_RF(C_) hipLaunchKernelGGL(refine_fwd_kernel<C_>, dim3(rows_to_blocks(n_rows)), dim3(256), 0, skr::as_stream(stream), d_Y, d_E, \
                                      n_rows, d_Z, d_w, d_accum)
    switch (dim / 64) { case 1: SKR_RF(1); break; case 2: SKR_RF(2); break; case 3: SKR_RF(3); break; default: SKR_RF(4); break; }
#undef SKR_RF
    SKR_LAUNCH_CHECK();
    return SKR_OK;
}

int skr_layer_refine_bwd_masked(const float* d_Y, const float* d_E, const float* d_w, const float* d_dZ, int64_t n_rows, int dim,
                                float* d_dY, float* d_dE, const uint8_t* d_row_mask, int zero_skipped, void* stream) {
    SKR_REQUIRE(d_Y && d_E && d_w && d_dZ && d_dY && d_dE, "skr_layer_refine_bwd: NULL argument");
    SKR_REQUIRE(dim == 64 || dim == 128 || dim == 192 || dim == 256, "skr_layer_refine_bwd: dim must be 64, 128, 192 or 256 (got %d)", dim);
    if (n_rows <= 0) return SKR_OK;
#define SKR_RB(C_) hipLaunchKernelGGL(refine_bwd_kernel<C_>, dim3(rows_to_blocks(n_rows)), dim3(256), 0, skr::as_stream(stream), d_Y, d_E, \
                                      d_w, d_dZ, n_rows, d_dY, d_dE, d_row_mask, zero_skipped)
    switch (dim / 64) { case 1: SKR_RB(1); break; case 2: SKR_RB(2); break; case 3: SKR_RB(3); break; default: SKR_RB(4); break; }
#undef SKR_RB
    SKR_LAUNCH_CHECK();
    return SKR_OK;
}

int skr_layer_refine_bwd(const float* d_Y, const float* d_E, const float* d_w, const float* d_dZ, int64_t n_rows, int dim,
                         float* d_dY, float* d_dE, void* stream) {
    return skr_layer_refine_bwd_masked(d_Y, d_E, d_w, d_dZ, n_rows, dim, d_dY, d_dE, nullptr, 0, stream);
}

int skr_clear_marked_rows(uint8_t* d_mask, int64_t n_rows, int64_t clear_mask, float* d_table, int dim, void* stream) {
    SKR_REQUIRE(n_rows >= 0 && dim >= 1, "skr_clear_marked_rows: bad shape");
    if (n_rows == 0) return SKR_OK;
    SKR_REQUIRE(d_mask && d_table, "skr_clear_marked_rows: NULL argument");
    const int64_t waves = (n_rows + 63) / 64;
    hipLaunchKernelGGL(clear_marked_rows_kernel, dim3(static_cast<unsigned>((waves + 3) / 4)), dim3(256), 0, skr::as_stream(stream), d_mask,
                       n_rows, clear_mask ? 1 : 0, d_table, dim);
    SKR_LAUNCH_CHECK();
    return SKR_OK;
}

int skr_gather_rows(const float* d_table, const int32_t* d_idx, int64_t n, int dim, float* d_out, void* stream) {
    SKR_REQUIRE(d_table && d_idx && d_out, "skr_gather_rows: NULL argument");
    SKR_REQUIRE(dim >= 1, "skr_gather_rows: dim must be positive (got %d)", dim);
    if (n <= 0) return SKR_OK;
    if (dim == D)
        hipLaunchKernelGGL(gather_rows_kernel, dim3(rows_to_blocks(n)), dim3(256), 0, skr::as_stream(stream), d_table, d_idx,
                           n, d_out);
    else
        hipLaunchKernelGGL(gather_rows_any_kernel, dim3(static_cast<unsigned>((n * dim + 255) / 256)), dim3(256), 0,
                           skr::as_stream(stream), d_table, d_idx, n, dim, d_out);
    SKR_LAUNCH_CHECK();
    return SKR_OK;
}

int skr_scatter_rows(const float* d_src, const int32_t* d_idx, int64_t n, int dim, float* d_table, void* stream) {
    SKR_REQUIRE(d_table && d_idx && d_src, "skr_scatter_rows: NULL argument");
    SKR_REQUIRE(dim >= 1, "skr_scatter_rows: dim must be positive (got %d)", dim);
    if (n <= 0) return SKR_OK;
    if (dim == D)
        hipLaunchKernelGGL(scatter_rows_kernel, dim3(rows_to_blocks(n)), dim3(256), 0, skr::as_stream(stream), d_src, d_idx, n,
                           d_table);
    else
        hipLaunchKernelGGL(scatter_rows_any_kernel, dim3(static_cast<unsigned>((n * dim + 255) / 256)), dim3(256), 0,
                           skr::as_stream(stream), d_src, d_idx, n, dim, d_table);
    SKR_LAUNCH_CHECK();
    return SKR_OK;
}

int skr_scale_copy(float a, const float* d_x, float* d_y, int64_t n, void* stream) {
    SKR_REQUIRE(d_x && d_y, "skr_scale_copy: NULL argument");
    if (n <= 0) return SKR_OK;
    int64_t blocks = (n + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(scale_copy_kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, skr::as_stream(stream), a, d_x, d_y, n);
    SKR_LAUNCH_CHECK();
    return SKR_OK;
}

int skr_sum_blocks(const float* d_in, int n_blocks, int64_t n, float* d_out, void* stream) {
    SKR_REQUIRE(d_in && d_out && n_blocks >= 1 && n >= 0, "skr_sum_blocks: bad argument");
    if (n == 0) return SKR_OK;
    int64_t blocks = (n + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(sum_blocks_kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, skr::as_stream(stream), d_in, n_blocks, n,
                       d_out);
    SKR_LAUNCH_CHECK();
    return SKR_OK;
}

int skr_axpy(float a, const float* d_x, float* d_y, int64_t n, void* stream) {
    SKR_REQUIRE(d_x && d_y, "skr_axpy: NULL argument");
    if (n <= 0) return SKR_OK;
    int64_t blocks = (n + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(axpy_kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, skr::as_stream(stream), a, d_x, d_y,
                       n);
    SKR_LAUNCH_CHECK();
    return SKR_OK;
}

int skr_scale(float a, float* d_x, int64_t n, void* stream) {
    SKR_REQUIRE(d_x, "skr_scale: NULL argument");
    if (n <= 0) return SKR_OK;
    int64_t blocks = (n + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(scale_kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, skr::as_stream(stream), a, d_x, n);
    SKR_LAUNCH_CHECK();
    return SKR_OK;
}

int skr_pack_grad_rows(const int32_t* d_ids, int n, float* d_g_table, float* d_g_bias, int dim, float* d_out, void* stream) {
    SKR_REQUIRE(d_ids && d_g_table && d_out, "skr_pack_grad_rows: NULL argument");
    SKR_REQUIRE(dim == D, "skr_pack_grad_rows: dim must be 64 (got %d)", dim);
    if (n <= 0) return SKR_OK;
    hipLaunchKernelGGL(pack_grad_rows_kernel, dim3((n + 3) / 4), dim3(256), 0, skr::as_stream(stream), d_ids, n, d_g_table,
                       d_g_bias, d_out);
    SKR_LAUNCH_CHECK();
    return SKR_OK;
}

int skr_unpack_grad_rows(const float* d_in, int n_per_rank, int n_ranks, float* d_g_table, float* d_g_bias, int dim,
                         uint8_t* d_touch, const float* d_touch_base, void* stream) {
    SKR_REQUIRE(d_in && d_g_table, "skr_unpack_grad_rows: NULL argument");
    SKR_REQUIRE(dim == D, "skr_unpack_grad_rows: dim must be 64 (got %d)", dim);
    SKR_REQUIRE((d_touch == nullptr) == (d_touch_base == nullptr), "touch: both pointers or neither");
    if (n_per_rank <= 0 || n_ranks <= 0) return SKR_OK;
    // one launch per rank, in rank order: ids are unique inside a rank's block, and every replica adds the
    // blocks in the same order, so the replicated tables stay bit-identical
    for (int r = 0; r < n_ranks; ++r) {
        hipLaunchKernelGGL(unpack_grad_rows_kernel, dim3((n_per_rank + 3) / 4), dim3(256), 0, skr::as_stream(stream),
                           d_in + static_cast<int64_t>(r) * n_per_rank * PK_W, n_per_rank, d_g_table, d_g_bias, d_touch,
                           d_touch_base);
        SKR_LAUNCH_CHECK();
    }
    return SKR_OK;
}

int skr_unpack_grad_rows_sorted(const float* d_in, int n_per_rank, int n_ranks, float* d_g_table, float* d_g_bias, int dim,
                                uint8_t* d_touch, const float* d_touch_base, void* stream) {
    SKR_REQUIRE(d_in && d_g_table, "skr_unpack_grad_rows_sorted: NULL argument");
    SKR_REQUIRE(dim == D, "skr_unpack_grad_rows_sorted: dim must be 64 (got %d)", dim);
    SKR_REQUIRE((d_touch == nullptr) == (d_touch_base == nullptr), "touch: both pointers or neither");
    if (n_per_rank <= 0 || n_ranks <= 0) return SKR_OK;
    if (n_ranks > UP_MAX_RANKS)   // beyond the kernel's register table: the per-rank launches give the same bits
        return skr_unpack_grad_rows(d_in, n_per_rank, n_ranks, d_g_table, d_g_bias, dim, d_touch, d_touch_base, stream);
    const int64_t waves = static_cast<int64_t>(n_per_rank) * n_ranks;
    hipLaunchKernelGGL(unpack_grad_rows_sorted_kernel, dim3(static_cast<unsigned>((waves + 3) / 4)), dim3(256), 0,
                       skr::as_stream(stream), d_in, n_per_rank, n_ranks, d_g_table, d_g_bias, d_touch, d_touch_base);
    SKR_LAUNCH_CHECK();
    return SKR_OK;
}

}  // extern "C"
