// step_common.h -- what the models' step drivers share: the small kernels that several of bm3.hip, selfcf.hip, dens.hip,
// freedom.hip, mgcn.hip and lattice.hip launch alike, the BPR scalars and the pos || neg item list of the triple models, the
// host-side plan runs of the graph models, and the timer of the profiling entries.
#pragma once
#include "skr_common.h"
#include "mfma_tile.h"

namespace skr {

// log(sigmoid(x)) as torch's log_sigmoid forward writes it
__device__ __forceinline__ float log_sigmoid(float x) { return fminf(x, 0.0f) - log1pf(expf(-fabsf(x))); }
// sigmoid(-x) without overflow
__device__ __forceinline__ float sigmoid_neg(float x) {
    const float e = expf(-fabsf(x));
    return x >= 0.0f ? e / (1.0f + e) : 1.0f / (1.0f + e);
}

// the item list of a batch of triples (dens.hip: pos and a hop's chosen items): position o < n is pos[o], position n + b is neg[b]
__device__ __forceinline__ int item_at(const int32_t* __restrict__ pos, const int32_t* __restrict__ neg, int n, int o) {
    return o < n ? pos[o] : neg[o - n];
}

namespace {   // kernels: templates, so that only a translation unit that launches one holds a copy; none is exported

// order_u [n] / order_i [n]: the positions of the user / item list sorted by (id, position) -- a rank by counting, which
// gives a batch's duplicate ids a fixed order; THREADS per workgroup.  The loop is written out here, in rank_triples_kernel,
// in dn_rank_kernel and in bk_prep_kernel: behind a helper that takes the list as an accessor it compiles to other code, and
// the launch groups measured 1 - 5 us slower (profiles/tile_helpers_timing.json).  rank_triples_kernel is one text for the
// three models that launch it, not such a helper: its two loops stay written out.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void rank_lists_kernel(const int32_t* __restrict__ users, const int32_t* __restrict__ items, int n,
                                                             int32_t* __restrict__ order_u, int32_t* __restrict__ order_i) {
    const int k = blockIdx.x * THREADS + threadIdx.x;
    if (k >= 2 * n) return;
    const int32_t* ids = k < n ? users : items;
    const int kk = k < n ? k : k - n;
    const int id = ids[kk];
    int rank = 0;
    for (int j = 0; j < n; ++j) {
        const int o = ids[j];
        rank += (o < id || (o == id && j < kk)) ? 1 : 0;
    }
    (k < n ? order_u : order_i)[rank] = kk;
}

// order_u [n] / order_i [2 n]: the positions of the user list and of pos || neg sorted by (id, position) -- the same rank
// by counting for an item list twice as long as the user list (freedom.hip, mgcn.hip, lattice.hip)
template <int THREADS>
__global__ __launch_bounds__(THREADS) void rank_triples_kernel(const int32_t* __restrict__ users, const int32_t* __restrict__ pos,
                                                               const int32_t* __restrict__ neg, int n, int32_t* __restrict__ order_u,
                                                               int32_t* __restrict__ order_i) {
    const int k = blockIdx.x * THREADS + threadIdx.x;
    if (k >= 3 * n) return;
    int rank = 0;
    if (k < n) {
        const int id = users[k];
        for (int j = 0; j < n; ++j) {
            const int o = users[j];
            rank += (o < id || (o == id && j < k)) ? 1 : 0;
        }
        order_u[rank] = k;
    } else {
        const int kk = k - n;
        const int id = item_at(pos, neg, n, kk);
        for (int j = 0; j < 2 * n; ++j) {
            const int o = item_at(pos, neg, n, j);
            rank += (o < id || (o == id && j < kk)) ? 1 : 0;
        }
        order_i[rank] = kk;
    }
}

// dst += src (freedom.hip, lattice.hip: the item rows' + h path)
template <int THREADS>
__global__ __launch_bounds__(THREADS) void add_kernel(float* dst, const float* src, int64_t n) {
    for (int64_t e = blockIdx.x * static_cast<int64_t>(THREADS) + threadIdx.x; e < n; e += static_cast<int64_t>(gridDim.x) * THREADS) {
        const float v = dst[e], w = src[e];
        dst[e] = v + w;
    }
}

// dX[head[rk]][f] = sum_o Gseg[rk][o] W[o][f]: a wavefront owns 16 ranks and 64 columns; rows that are no head are not written
// (bm3.hip, freedom.hip: the feature tables' gradient, one writer per distinct item); HW wavefronts per workgroup
template <int HW>
__global__ __launch_bounds__(HW * 64) void feat_grad_kernel(const float* __restrict__ Gseg, const int32_t* __restrict__ head, int n, int ld,
                                                            const float* __restrict__ W, float* __restrict__ dX) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
    const int rk0 = blockIdx.x * 16;
    const int f0 = (blockIdx.y * HW + wv) * 64;
    if (f0 >= ld) return;
    float a[16];
    load_row_a(a, Gseg, rk0 + r < n ? rk0 + r : -1, g);
    f32x4 acc[4];
    zero_acc(acc);
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
        const float* __restrict__ wrow = W + static_cast<int64_t>(16 * g + kk) * ld + f0 + r;
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) {
            const float b = f0 + nb * 16 + r < ld ? wrow[nb * 16] : 0.0f;
            acc[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[kk], b, acc[nb], 0, 0, 0);
        }
    }
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        const int rk = rk0 + 4 * g + rr;
        const int64_t id = rk < n ? head[rk] : -1;
        if (id < 0) continue;
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) {
            const int f = f0 + nb * 16 + r;
            if (f < ld) dX[id * ld + f] = acc[nb][rr];
        }
    }
}

// the feature-gradient rows of the listed items := 0 (blockIdx.y: the modality; bm3.hip, freedom.hip)
struct ClearParams {
    float* table[2];
    int ld[2];
};
template <int THREADS>
__global__ __launch_bounds__(THREADS) void clear_rows_kernel(ClearParams p, const int32_t* __restrict__ ids, int I) {
    float* t = p.table[blockIdx.y];
    if (t == nullptr) return;
    const int id = ids[blockIdx.x], ld = p.ld[blockIdx.y];
    if (id < 0 || id >= I) return;
    float4* row = reinterpret_cast<float4*>(t + static_cast<int64_t>(id) * ld);
    for (int k = threadIdx.x; k < ld / 4; k += THREADS) row[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

// out [LEN] = the workgroups' partial sums part [n_wg][LEN] in workgroup order
template <int LEN>
__global__ __launch_bounds__(256) void part_reduce_kernel(const float* __restrict__ part, int n_wg, float* __restrict__ out) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= LEN) return;
    float t = 0.0f;
    for (int w = 0; w < n_wg; ++w) t += part[static_cast<int64_t>(w) * LEN + e];
    out[e] = t;
}

}  // namespace

// ---- host side: the plan runs of the graph models' steps.  Every table is [n_users + n_items, 64]: the user rows, then the
// item rows, which start UO = 64 n_users floats in; A-hat maps the item rows to the user rows through plan_a and back through
// plan_at.

// one product with the plain epilogue: Y = plan X (+ addend); with accum, accum = accum_base + Y or accum += Y
inline int plain_run(const skr_spmm_plan* plan, const float* X, const float* addend, float* Y, float* accum, const float* accum_base,
                     void* stream) {
    skr_spmm_epilogue ep = {};
    ep.mode = SKR_EPI_PLAIN;
    ep.addend = addend;
    ep.Y = Y;
    ep.accum = accum;
    ep.accum_base = accum_base;
    ep.accum_scale = 1.0f;
    return skr_spmm_plan_run_ex(plan, X, 64, &ep, nullptr, nullptr, stream);
}

// M = the mean of X_0 .. X_L, X_k = A-hat X_(k-1): M = s X_0 + s X_1, then M += s X_k, s = 1 / (L + 1); X_k for k < L goes
// to ping[(k - 1) & 1].  run(plan, X, epilogue, item_half) -> int runs one product: the model's A-hat, plain or edge-dropped.
template <class Run>
int mean_forward(const skr_spmm_plan* plan_a, const skr_spmm_plan* plan_at, const float* X0, int64_t UO, int64_t N, int L,
                 float* const* ping, float* M, hipStream_t st, Run run) {
    if (L == 0) {
        SKR_HIP(hipMemcpyAsync(M, X0, static_cast<size_t>(N) * 64 * sizeof(float), hipMemcpyDeviceToDevice, st));
        return SKR_OK;
    }
    const float* X = X0;
    for (int k = 1; k <= L; ++k) {
        float* Y = k == L ? nullptr : ping[(k - 1) & 1];
        skr_spmm_epilogue ep = {};
        ep.mode = SKR_EPI_PLAIN;
        ep.accum_scale = 1.0f / static_cast<float>(L + 1);
        ep.Y = Y;
        ep.accum = M;
        ep.accum_base = k == 1 ? X0 : nullptr;
        int rc = run(plan_a, X + UO, ep, false);
        if (rc != SKR_OK) return rc;
        ep.Y = Y ? Y + UO : nullptr;
        ep.accum = M + UO;
        ep.accum_base = k == 1 ? X0 + UO : nullptr;
        rc = run(plan_at, X, ep, true);
        if (rc != SKR_OK) return rc;
        X = Y;
    }
    return SKR_OK;
}

// the backward of mean_forward: acc = G; L times acc = A-hat^T acc + G; the last product writes acc / (L + 1) into grad.
// ``run`` as above, on the transposed matrix' entries (SelfCF's dropped one is not symmetric).
template <class Run>
int chain_backward(const skr_spmm_plan* plan_a, const skr_spmm_plan* plan_at, const float* G, int64_t UO, int L, float* const* ping,
                   float* grad, Run run) {
    const float* X = G;
    for (int k = 1; k <= L; ++k) {
        const bool last = k == L;
        float* Y = last ? nullptr : ping[(k - 1) & 1];
        skr_spmm_epilogue ep = {};
        ep.mode = SKR_EPI_PLAIN;
        ep.accum_scale = 1.0f / static_cast<float>(L + 1);
        ep.addend = G;
        ep.Y = Y;
        if (last) { ep.accum = grad; ep.accum_init = 1; }
        int rc = run(plan_a, X + UO, ep, false);
        if (rc != SKR_OK) return rc;
        ep.addend = G + UO;
        ep.Y = Y ? Y + UO : nullptr;
        if (last) ep.accum = grad + UO;
        rc = run(plan_at, X, ep, true);
        if (rc != SKR_OK) return rc;
        X = Y;
    }
    return SKR_OK;
}

// The events of a step's profiling entry: one after every launch group, at most MARKS of them.  With h_ms == NULL (the
// plain entry) nothing here calls the runtime.  The destructor releases the events on every way out of the step.
template <int MARKS>
class StepTimer {
public:
    StepTimer(float* h_ms, hipStream_t st) : h_ms_(h_ms), st_(st) {}
    StepTimer(const StepTimer&) = delete;
    StepTimer& operator=(const StepTimer&) = delete;
    ~StepTimer() {
        for (int k = 0; k < n_; ++k) (void)hipEventDestroy(ev_[k]);
    }
    hipError_t mark() {
        if (h_ms_ == nullptr) return hipSuccess;
        if (n_ >= MARKS) return hipErrorInvalidValue;
        const hipError_t e = hipEventCreate(&ev_[n_]);
        return e == hipSuccess ? hipEventRecord(ev_[n_++], st_) : e;
    }
    // waits for the last mark; h_ms[k] = milliseconds between marks k and k + 1
    hipError_t finish() {
        if (h_ms_ == nullptr || n_ == 0) return hipSuccess;
        hipError_t e = hipEventSynchronize(ev_[n_ - 1]);
        for (int k = 0; e == hipSuccess && k + 1 < n_; ++k) e = hipEventElapsedTime(&h_ms_[k], ev_[k], ev_[k + 1]);
        return e;
    }

private:
    float* h_ms_;
    hipStream_t st_;
    hipEvent_t ev_[MARKS];
    int n_ = 0;
};

}  // namespace skr
