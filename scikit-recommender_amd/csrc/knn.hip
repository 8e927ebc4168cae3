// knn.hip -- the item-item k-nearest-neighbour lists of a feature table by cosine similarity, without the [n, n] matrix.
//
// Replaces the stock torch ops the reference's multimodal models issue when they build their item graph (no native code
// there):
//   recommender/FREEDOM.py:126-129   X / |X|, torch.mm(X, X^T) as a dense [I, I] matrix, torch.topk per row
//   recommender/LATTICE.py:67-90, recommender/MGCN.py:61-110   the same construction
//
// Layout: see include/skrec_hip.h, section K.
//
// Launches:
//   inv_norm   inv[i] = 1 / max(|X_i|, 1e-12): one wavefront per row
//   topk       a workgroup owns 64 query rows and sweeps the table 256 rows (columns of the similarity matrix) at a time.  Per
//              column block it walks the features 32 at a time: both operand tiles are staged through LDS (the next chunk's
//              global loads are in flight while the current one is multiplied), a wavefront owns 16 query rows and forms its
//              16 x 256 dot products on v_mfma_f32_16x16x4_f32 with fp32 operands, 256 features to a partial sum and the partial
//              sums added in order (blocked summation: the error of a 4 096-term product stays at a BLAS's).  The finished tile
//              is scaled by inv[q] inv[c] and merged, 64 columns at a time, into the rows' running lists: k packed (similarity,
//              id) keys per row in LDS (sized by the launch), sorted descending; a candidate is inserted only if it beats the
//              row's k-th key.
//
// No [n, n] array and no O(n^2) array exists anywhere: the similarities live in accumulators and one LDS tile.
//
// The MFMA operand mapping is mfma_tile.h's k = 8 g + kk of the chunk.
//
// Determinism: every dot product is summed in one fixed order by one wavefront, a row's list is owned by one wavefront,
// and the order (similarity descending, id ascending) is total: two calls are bit-identical.  No atomic of any kind.
#include "skr_common.h"
#include "mfma_tile.h"

namespace {

using namespace skr;

constexpr int TQ = 64;         // query rows of a workgroup: 16 per wavefront
constexpr int TC = 256;        // table rows of a column block
constexpr int KC = 32;         // features of a chunk
constexpr int FLUSH = 8;       // chunks summed in one accumulator before it is added to the row's total (a power of two)
constexpr int LDP = 36;        // LDS row stride of the operand tiles
constexpr int LDS_S = 65;      // LDS row stride of the similarity tile
constexpr int HW = 4;          // wavefronts per workgroup
constexpr int MAXK = SKR_KNN_MAX_K;
constexpr int MAXF = SKR_BM3_MAX_FEAT;
constexpr float NORM_EPS = 1e-12f;

static_assert(TQ * LDS_S <= TC * LDP, "the similarity tile takes the column tile's place");
static_assert((TQ + TC) * LDP * 4 + TQ * MAXK * 8 <= 65536, "64 KiB of LDS per workgroup");
static_assert(MAXK <= 32, "a row's list is held by the lower half of a wavefront");

__global__ __launch_bounds__(HW * 64) void knn_inv_norm_kernel(const float* __restrict__ X, int n, int ld, float* __restrict__ inv) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t row = static_cast<int64_t>(blockIdx.x) * HW + wv;
    if (row >= n) return;
    const float* __restrict__ x = X + row * ld;
    float s = 0.0f;
    for (int k = 4 * lane; k < ld; k += 256) {
        const float4 v = *reinterpret_cast<const float4*>(x + k);
        s += (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
    }
    s = skr::wave_sum(s);
    if (lane == 0) inv[row] = 1.0f / fmaxf(sqrtf(s), NORM_EPS);
}

// the chunk [k0, k0 + KC) of the query rows q0.. and of the table rows c0..: 2 + 8 float4 per thread, zeros outside the table
struct Chunk {
    float4 a0, a1, b0, b1, b2, b3, b4, b5, b6, b7;
};
__device__ __forceinline__ float4 fetch_row(const float* __restrict__ X, int n, int ld, int64_t row, int kq) {
    return kq < ld && row < n ? *reinterpret_cast<const float4*>(X + row * ld + kq) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}
__device__ __forceinline__ Chunk fetch(const float* __restrict__ X, int n, int ld, int q0, int c0, int k0) {
    const int c4 = threadIdx.x & 7, r0 = threadIdx.x >> 3;
    const int kq = k0 + 4 * c4;
    const int64_t q = static_cast<int64_t>(q0) + r0, c = static_cast<int64_t>(c0) + r0;
    Chunk v;
    v.a0 = fetch_row(X, n, ld, q, kq);
    v.a1 = fetch_row(X, n, ld, q + 32, kq);
    v.b0 = fetch_row(X, n, ld, c, kq);
    v.b1 = fetch_row(X, n, ld, c + 32, kq);
    v.b2 = fetch_row(X, n, ld, c + 64, kq);
    v.b3 = fetch_row(X, n, ld, c + 96, kq);
    v.b4 = fetch_row(X, n, ld, c + 128, kq);
    v.b5 = fetch_row(X, n, ld, c + 160, kq);
    v.b6 = fetch_row(X, n, ld, c + 192, kq);
    v.b7 = fetch_row(X, n, ld, c + 224, kq);
    return v;
}

// The 64 columns col0.. of the finished tile, scaled by inv[q] inv[c], go through LDS into the lists of the wavefront's 16 rows,
// one row after the other: lane = column, lanes [0, k) = the row's list.  A wavefront touches its own rows of sS and sL only.
__device__ __forceinline__ void merge_quarter(const f32x4 acc[4], int col0, int q0, int n, int k, const float* __restrict__ inv, const float invq[4],
                                           float* __restrict__ sS, unsigned long long* __restrict__ sL) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
    __syncthreads();                                    // every wavefront is done with the column tile, whose place sS takes
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) {
        const int col = col0 + nb * 16 + r;
        const float invc = col < n ? inv[col] : 0.0f;
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) sS[(wv * 16 + 4 * g + rr) * LDS_S + nb * 16 + r] = (acc[nb][rr] * invq[rr]) * invc;
    }
    __syncthreads();
    const int col = col0 + lane;
    for (int j = 0; j < 16; ++j) {
        const int row = wv * 16 + j;
        if (q0 + row >= n) break;
        const unsigned long long ck = col < n ? skr::rank_key(sS[row * LDS_S + lane], col) : SKR_KEY_MIN;
        unsigned long long mine = lane < k ? sL[row * k + lane] : SKR_KEY_MIN;
        unsigned long long thr = __shfl(mine, k - 1, 64);
        unsigned long long m = __ballot(ck > thr);
        if (m == 0) continue;
        while (m != 0) {                                // (uniform: m, c and thr are the same in every lane)
            const int src = __ffsll(m) - 1;
            m &= m - 1;
            const unsigned long long c = __shfl(ck, src, 64);
            if (c <= thr) continue;                     // the threshold has risen since the ballot
            const int pos = __popcll(__ballot(lane < k && mine > c));
            const unsigned long long up = __shfl_up(mine, 1, 64);
            if (lane < k) {
                if (lane == pos) mine = c;
                else if (lane > pos) mine = up;
            }
            thr = __shfl(mine, k - 1, 64);
        }
        if (lane < k) sL[row * k + lane] = mine;
    }
}

// ids[q][0..k) / sims[q][0..k): the k table rows most similar to row q, by (similarity descending, id ascending)
__global__ __launch_bounds__(HW * 64, 2) void knn_topk_kernel(const float* __restrict__ X, int n, int ld, const float* __restrict__ inv, int k,
                                                           int32_t* __restrict__ ids, float* __restrict__ sims) {
    __shared__ __attribute__((aligned(16))) float sA[TQ * LDP];
    __shared__ __attribute__((aligned(16))) float sB[TC * LDP];
    extern __shared__ unsigned long long sL[];          // [TQ][k] (sized by the launch): a row's list, keys in descending order
    float* sS = sB;     // a quarter of a scaled similarity tile, [TQ][64], between two column blocks; a wavefront touches its 16 rows only
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
    const int c4 = threadIdx.x & 7, r0 = threadIdx.x >> 3;
    const int q0 = blockIdx.x * TQ;
    for (int e = threadIdx.x; e < TQ * k; e += HW * 64) sL[e] = SKR_KEY_MIN;
    float invq[4];
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        const int q = q0 + wv * 16 + 4 * g + rr;
        invq[rr] = q < n ? inv[q] : 0.0f;
    }
    const int nk = (ld + KC - 1) / KC;
    Chunk nx = fetch(X, n, ld, q0, 0, 0);
    for (int c0 = 0; c0 < n; c0 += TC) {
        // per quarter of the column block (64 columns): the running sums of at most FLUSH chunks, and the sums of those.  A
        // product of 4 096 terms added one after the other loses sqrt(4 096) ulps; in blocks of 256 it stays beside a BLAS's error
        f32x4 acc[4][4], sum[4][4];                     // [quarter][16 columns]
#pragma unroll
        for (int h = 0; h < 4; ++h) {
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[h][j] = sum[h][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        }
        for (int kc = 0; kc < nk; ++kc) {
            __syncthreads();                            // the previous chunk's products, or the merge, have read the tiles
            *reinterpret_cast<float4*>(sA + r0 * LDP + 4 * c4) = nx.a0;
            *reinterpret_cast<float4*>(sA + (r0 + 32) * LDP + 4 * c4) = nx.a1;
            *reinterpret_cast<float4*>(sB + r0 * LDP + 4 * c4) = nx.b0;
            *reinterpret_cast<float4*>(sB + (r0 + 32) * LDP + 4 * c4) = nx.b1;
            *reinterpret_cast<float4*>(sB + (r0 + 64) * LDP + 4 * c4) = nx.b2;
            *reinterpret_cast<float4*>(sB + (r0 + 96) * LDP + 4 * c4) = nx.b3;
            *reinterpret_cast<float4*>(sB + (r0 + 128) * LDP + 4 * c4) = nx.b4;
            *reinterpret_cast<float4*>(sB + (r0 + 160) * LDP + 4 * c4) = nx.b5;
            *reinterpret_cast<float4*>(sB + (r0 + 192) * LDP + 4 * c4) = nx.b6;
            *reinterpret_cast<float4*>(sB + (r0 + 224) * LDP + 4 * c4) = nx.b7;
            __syncthreads();
            // the next chunk, or the first one of the next column block, is in flight while this one is multiplied (behind the
            // last block the table rows are all >= n: nothing is loaded for them)
            const bool wrap = kc + 1 == nk;
            nx = fetch(X, n, ld, q0, wrap ? c0 + TC : c0, wrap ? 0 : (kc + 1) * KC);
            float a[8];
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const float4 v = *reinterpret_cast<const float4*>(sA + (wv * 16 + r) * LDP + 8 * g + 4 * q);
                a[4 * q + 0] = v.x; a[4 * q + 1] = v.y; a[4 * q + 2] = v.z; a[4 * q + 3] = v.w;
            }
#pragma unroll
            for (int h = 0; h < 4; ++h) tile_product<LDP>(acc[h], a, sB + h * 64 * LDP, r, g);
            if ((kc & (FLUSH - 1)) == FLUSH - 1 || wrap) {
#pragma unroll
                for (int h = 0; h < 4; ++h) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        sum[h][j] += acc[h][j];
                        acc[h][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                    }
                }
            }
        }
        merge_quarter(sum[0], c0, q0, n, k, inv, invq, sS, sL);
        merge_quarter(sum[1], c0 + 64, q0, n, k, inv, invq, sS, sL);
        merge_quarter(sum[2], c0 + 128, q0, n, k, inv, invq, sS, sL);
        merge_quarter(sum[3], c0 + 192, q0, n, k, inv, invq, sS, sL);
    }
    __syncthreads();
    for (int e = threadIdx.x; e < TQ * k; e += HW * 64) {
        const int row = e / k, slot = e - row * k;
        const int64_t q = static_cast<int64_t>(q0) + row;
        if (q >= n) break;
        const unsigned long long key = sL[row * k + slot];
        ids[q * k + slot] = skr::key_id(key);
        if (sims != nullptr) sims[q * k + slot] = skr::key_score(key);
    }
}

inline size_t workspace_bytes(int n_rows) { return ((static_cast<size_t>(n_rows) * sizeof(float) + 255) / 256) * 256; }

}  // namespace

extern "C" {

size_t skr_knn_workspace(int n_rows, int k) {
    if (n_rows <= 0 || k < 1 || k > MAXK || k > n_rows) return 0;
    return workspace_bytes(n_rows);
}

int skr_knn_topk(const float* d_X, int n_rows, int feat_dim, int feat_ld, int k, int32_t* d_ids, float* d_sims, void* d_work, size_t work_bytes,
                 void* stream) {
    SKR_REQUIRE(d_X && d_ids && d_work, "skr_knn_topk: NULL argument");
    SKR_REQUIRE(n_rows > 0, "skr_knn_topk: n_rows = %d", n_rows);
    SKR_REQUIRE(k >= 1 && k <= MAXK && k <= n_rows, "skr_knn_topk: 1 <= k <= min(%d, n_rows = %d) (got %d)", MAXK, n_rows, k);
    SKR_REQUIRE(feat_dim >= 1 && feat_dim <= MAXF, "skr_knn_topk: 1 <= feat_dim <= %d (got %d)", MAXF, feat_dim);
    SKR_REQUIRE(feat_ld >= feat_dim && feat_ld % 4 == 0 && feat_ld <= MAXF,
                "skr_knn_topk: feat_ld = %d must be a multiple of 4, >= feat_dim = %d and <= %d", feat_ld, feat_dim, MAXF);
    SKR_REQUIRE(((reinterpret_cast<uintptr_t>(d_X) | reinterpret_cast<uintptr_t>(d_work)) & 15) == 0,
                "skr_knn_topk: the table and work must be 16-byte aligned");
    SKR_REQUIRE(((reinterpret_cast<uintptr_t>(d_ids) | reinterpret_cast<uintptr_t>(d_sims)) & 3) == 0, "skr_knn_topk: the outputs must be 4-byte aligned");
    SKR_REQUIRE(work_bytes >= workspace_bytes(n_rows), "skr_knn_topk: work holds %zu bytes, skr_knn_workspace(%d, %d) asks for %zu", work_bytes, n_rows,
                k, workspace_bytes(n_rows));
    hipStream_t st = skr::as_stream(stream);
    float* inv = static_cast<float*>(d_work);
    hipLaunchKernelGGL(knn_inv_norm_kernel, dim3((n_rows + HW - 1) / HW), dim3(HW * 64), 0, st, d_X, n_rows, feat_ld, inv);
    hipLaunchKernelGGL(knn_topk_kernel, dim3((n_rows + TQ - 1) / TQ), dim3(HW * 64), static_cast<size_t>(TQ) * k * sizeof(unsigned long long), st, d_X, n_rows, feat_ld, inv, k, d_ids, d_sims);
    SKR_LAUNCH_CHECK();
    return SKR_OK;
}

}  // extern "C"
