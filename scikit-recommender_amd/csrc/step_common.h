// step_common.h -- what the models' step drivers share: the two small kernels that bm3.hip and selfcf.hip (and, for the
// reduction, dens.hip) launch alike, the host-side plan runs of the four graph models, and the timer of the profiling entries.
#pragma once
#include "skr_common.h"

namespace skr {

namespace {   // kernels: templates, so that only a translation unit that launches one holds a copy; none is exported

// order_u [n] / order_i [n]: the positions of the user / item list sorted by (id, position) -- a rank by counting, which
// gives a batch's duplicate ids a fixed order; THREADS per workgroup.  The loop is written out here, in dn_rank_kernel and
// in bk_prep_kernel: behind a helper that takes the list as an accessor it compiles to other code, and the launch groups
// measured 1 - 5 us slower (profiles/tile_helpers_timing.json).
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
