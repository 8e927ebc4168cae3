// fast_rng.h -- the counter-keyed generator of the fast sampler (sampler.hip) and of the models' device draws:
// splitmix64 turns (seed, epoch, slot) into the state of a xoshiro128++ stream of that slot alone.  The two dropout
// draws below key a slot by what they drop: draw_keep an element of a numbered stream (selfcf.hip, bm3.hip), keep_draw
// a (user, item) pair (cdae.hip, multvae.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

__host__ __device__ __forceinline__ uint64_t splitmix64(uint64_t& x) {
    x += 0x9E3779B97F4A7C15ull;
    uint64_t z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__host__ __device__ __forceinline__ uint32_t rotl32(uint32_t x, int k) { return (x << k) | (x >> (32 - k)); }

struct Xoshiro128pp {
    uint32_t s0, s1, s2, s3;
    __host__ __device__ void seed(uint64_t seed, uint64_t epoch, uint64_t slot) {
        uint64_t x = seed;
        uint64_t k = splitmix64(x) ^ (epoch * 0xD1B54A32D192ED03ull);
        x = k;
        k = splitmix64(x) ^ slot;
        x = k;
        const uint64_t a = splitmix64(x), b = splitmix64(x);
        s0 = static_cast<uint32_t>(a); s1 = static_cast<uint32_t>(a >> 32);
        s2 = static_cast<uint32_t>(b); s3 = static_cast<uint32_t>(b >> 32);
        if ((s0 | s1 | s2 | s3) == 0) s0 = 1;
    }
    __host__ __device__ uint32_t next() {
        const uint32_t r = rotl32(s0 + s3, 7) + s0;
        const uint32_t t = s1 << 9;
        s2 ^= s0; s3 ^= s1; s1 ^= s2; s0 ^= s3; s2 ^= t;
        s3 = rotl32(s3, 11);
        return r;
    }
};

// keep iff a 24-bit uniform is >= rate.  Slot: the stream's number in the top 4 bits, the element's index below them.
__device__ __forceinline__ bool draw_keep(uint64_t seed, uint64_t step, uint64_t stream, uint64_t idx, float rate) {
    Xoshiro128pp g;
    g.seed(seed, step, (stream << 60) | idx);
    return static_cast<float>(g.next() >> 8) * (1.0f / 16777216.0f) >= rate;
}

// keep iff a 24-bit uniform is < keep_prob.  Slot: the user in the upper 32 bits, the item in the lower 32.
__device__ __forceinline__ bool keep_draw(uint64_t seed, uint64_t step, int user, int item, float keep_prob) {
    Xoshiro128pp g;
    g.seed(seed, step, (static_cast<uint64_t>(static_cast<uint32_t>(user)) << 32) | static_cast<uint32_t>(item));
    return static_cast<float>(g.next() >> 8) * 0x1p-24f < keep_prob;
}
