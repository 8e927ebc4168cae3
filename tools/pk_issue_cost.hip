// What a plain and a packed fp32 FMA (and v_rcp_f32) cost ONE wavefront alone on its SIMD -- the situation of the fused BPR
// step's catch-up (bpr_fused_step_kernel: one wavefront per interaction): C independent chains of dependent instructions,
// 256 workgroups of four wavefronts, ticks of s_memtime per instruction (median and minimum over the wavefronts).
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -fno-fast-math -ffp-contract=off -o pk_issue_cost tools/pk_issue_cost.hip
// Numbers and their reading: profiles/fused_pack_timing.json.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <vector>

typedef float f32x2 __attribute__((ext_vector_type(2)));
constexpr int ITER = 2048;
enum { PLAIN, PACKED, RCP };

template <int C, int KIND>
__global__ __launch_bounds__(256) void chains_kernel(float a, float b, long long* out, float* sink) {
    f32x2 x[C];
    float y[C];
    for (int c = 0; c < C; ++c) {
        x[c] = f32x2{a + c, b + c} * (threadIdx.x + 1.0f);
        y[c] = a * c + threadIdx.x;
    }
    const f32x2 m2 = {a, b}, c2 = {b, a};
    const long long t0 = __builtin_amdgcn_s_memtime();
    for (int i = 0; i < ITER; ++i) {
#pragma unroll
        for (int c = 0; c < C; ++c) {
            if (KIND == PACKED) x[c] = __builtin_elementwise_fma(x[c], m2, c2);
            else if (KIND == RCP) y[c] = __builtin_amdgcn_rcpf(y[c]);
            else y[c] = __builtin_fmaf(y[c], a, b);
        }
    }
    const long long t1 = __builtin_amdgcn_s_memtime();
    float s = 0;
    for (int c = 0; c < C; ++c) s += x[c].x + x[c].y + y[c];
    if (s == 12345.678f) sink[0] = s;      // keeps the chains alive
    if ((threadIdx.x & 63) == 0) out[blockIdx.x * 4 + (threadIdx.x >> 6)] = t1 - t0;
}

template <int C, int KIND>
static bool run(const char* name, long long* d_out, float* d_sink) {
    const int nb = 256;
    for (int rep = 0; rep < 3; ++rep) chains_kernel<C, KIND><<<nb, 256>>>(1.0001f, 0.0001f, d_out, d_sink);
    std::vector<long long> h(nb * 4);
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(h.data(), d_out, h.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) return false;
    std::sort(h.begin(), h.end());
    std::printf("%-14s chains %d: median %.2f ticks per instruction (min %.2f)\n", name, C, double(h[h.size() / 2]) / (ITER * C),
                double(h[0]) / (ITER * C));
    return true;
}

int main() {
    long long* d_out;
    float* d_sink;
    if (hipMalloc(&d_out, 1024 * 8) != hipSuccess || hipMalloc(&d_sink, 4) != hipSuccess) return 1;
    bool ok = run<1, PLAIN>("v_fma_f32", d_out, d_sink) && run<2, PLAIN>("v_fma_f32", d_out, d_sink) &&
              run<4, PLAIN>("v_fma_f32", d_out, d_sink) && run<8, PLAIN>("v_fma_f32", d_out, d_sink) &&
              run<1, PACKED>("v_pk_fma_f32", d_out, d_sink) && run<2, PACKED>("v_pk_fma_f32", d_out, d_sink) &&
              run<4, PACKED>("v_pk_fma_f32", d_out, d_sink) && run<8, PACKED>("v_pk_fma_f32", d_out, d_sink) &&
              run<1, RCP>("v_rcp_f32", d_out, d_sink) && run<4, RCP>("v_rcp_f32", d_out, d_sink);
    return ok ? 0 : 1;
}
