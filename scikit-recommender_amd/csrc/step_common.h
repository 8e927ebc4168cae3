// step_common.h -- what the models' step drivers share: the two small kernels that bm3.hip and selfcf.hip (and, for the
// reduction, dens.hip) launch alike, and the host-side timer of the profiling entries.
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
