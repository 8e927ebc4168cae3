// bpr_fused.hip -- K2c: the BPR batch and the hot rows' Adam in ONE launch per step (skr_bpr_fused_*).  The Adam arithmetic
// (adam_math.h) is shared with the optimiser's own kernels (adam.hip); the two-launch form of the step is train.hip's K1.
#include "adam_math.h"

#include <cstdlib>

using namespace skr;

namespace {

constexpr int BPR_WAVES = 4;      // wavefronts per workgroup, as bpr_step_kernel (train.hip)

// ------------------------------------------------------------------------------------------------
// K2c: the BPR batch and the hot rows' Adam in ONE launch per step (single GPU).
//
// With bpr_step_kernel + adam_hot_kernel a training step is a chain of two dependent launches (6-8 us + 13 us): the
// gradient of batch t must be complete before any row moves, and batch t+1 reads rows that step t moved.  The chain is
// cut to one launch by evaluating the hot rows LAZILY: a row is advanced when a batch reads it, by the wavefronts that
// read it, and a gradient is applied at the row's NEXT naming (or by the block's end launch).  The batches of a k-step
// block are known in advance, so for every reference (step s, row r) the host precomputes (skrec/recommender/fused.py)
//     slot   the row's index in the block's compact workspace
//     n0     how many earlier steps of the block named the row (0-based naming index), modulo 6
//     prev   the step of the previous naming (or none)
//     owner  exactly one reference per (step, row) pair
// The row's state before step s:  n0 == 0: the dense tables (no step of the block has touched it);  n0 > 0: workspace copy
// n0 & 1, valid through optimiser index prev - 1, plus the gradient of step `prev` waiting in gradient buffer (n0 - 1) % 3.
// Every wavefront that reads the row applies, in registers, index `prev` with that gradient and the zero-gradient indices
// prev + 1 .. s - 1 -- the updates the dense optimiser makes, in its arithmetic (adam_math.h: the shared moment update, then
// the scaling-free quotient when every lane is of ordinary magnitudes -- tested on the updated moments, once for the gradient
// update and the run behind it -- the general form otherwise: the same bits) -- and uses the result for its scores.  The pair's OWNER also
// writes it to copy (n0 + 1) & 1 and clears gradient buffer (n0 + 1) % 3; all of them add this step's gradient into buffer
// n0 % 3.  Within one launch nobody writes what another wavefront reads: two state copies and three gradient buffers keep
// readers, the writer and the accumulators apart, so no wavefront waits for another and no hand-off crosses the L2s.
// bpr_fused_end_kernel brings every slot to the block's last index and writes it back to the dense tables.
// Same updates of every parameter in the same order and arithmetic as one dense Adam launch per step
// (tests/test_gpu_train.py::test_fused_step_is_bit_identical).
// ------------------------------------------------------------------------------------------------
constexpr int FUSED_SLOT_BITS = 20;
constexpr int FUSED_PRE = 7;     // value of a word's n0 field (n0 mod 6 otherwise): first naming, state waiting in the pre buffer

struct FusedRow {
    float p, m, v, g;
};

// prev1 > 0: index prev1 - 1 with gradient r.g, then the zero-gradient indices [prev1, s_to) (the plan has prev1 <= s_to: the
// previous naming lies before this step);  prev1 == 0: the zero-gradient indices [s_from, s_to) only.  ck: the census's kernel
// index (adam_math.h)
__device__ __forceinline__ void fused_advance(FusedRow& r, int prev1, int s_from, int s_to, const AdamBlockArgs& a, int ck) {
    if (prev1 > 0)
        adam_grad_run(r.p, r.g, r.m, r.v, a, prev1 - 1, s_to, ck);
    else
        adam_zero_run(r.p, r.m, r.v, a, s_from, s_to, ck);
}

// an address put together from two scalars: in the global address space by its type, so that the load is a global_load
typedef const float __attribute__((address_space(1)))* GlobalFloats;

struct FusedWork {
    float *wp, *wm, *wv, *g;   // wp / wm / wv: [2][cap][64];  g: [3][cap][64]
    int64_t cap;
};

// (the one element of the deferred step kernel's parameter pack)
__device__ __forceinline__ float* fused_loss_part(float* row) { return row; }

// One wavefront per interaction, its five rows one after the other (dbg: timing switches of tools/fused_lab.py).  A
// workgroup of five wavefronts per interaction (one per row, the rows meeting in LDS) was tried and is slower (18.4 vs 12.7 us
// per launch alone on the chip): a CU holds four interactions either way, so the catch-up arithmetic per SIMD is the same,
// and the barrier and the second id load come on top.
//
// The load phase.  A wavefront's time is a chain of memory round trips, and the launch lasts as long as its slowest
// wavefront, so the phase is written to make exactly two of them, whatever the rows' sources (three on a stack that does not
// preload kernel arguments):
//   1. the arguments the first loads need (the id and word columns, n) cost no trip: they are the first 14 dwords of the
//      parameter list, which the Makefile has this file's kernels receive in SGPRs at wavefront launch
//      (-amdgpu-kernarg-preload-count; firmware that does not preload runs the compiler's prologue, which loads the
//      same registers: the round trip of before).  Keep them first when the list changes;
//   2. the first interaction's ids and words (two loads: one row per group of four lanes) and the per-step tables, with
//      every other argument fetched beside them in one round of scalar loads;
//   3. all twenty row loads (p, m, v and the gradient word of the five rows), issued back to back with no wait between
//      the first and the last.  Lane 4 r + q computes the address of plane q of row r -- the row's source (pre buffer,
//      dense tables, workspace) selects the BASE, nothing is loaded from a source that is not the row's (pre may be NULL) --
//      and the loads take their bases from the lanes with v_readlane.
// What a source does not supply is put in afterwards by selects: {1, 0, 0} for the lanes of the last bias block that lie
// past the end of the dense buffer (they load the last element inside), 0 for the gradient of a row that has none pending.
// Written with a branch per source the same loads compile to a wait at every join of the branches (the defaults written
// on one path are load destinations on the others, so all older loads must have returned first): up to five dependent
// trips for the rows, and four for the arguments and tables in front of them.  The values that reach chain_advance are
// the same: the kernel stays bit-identical.
//
// The loss words, two forms.  bpr_fused_step_kernel<> adds one pair per WORKGROUP to the step's SKR_LOSS_SLOTS pairs.  The
// DEFERRED form, bpr_fused_step_kernel<float*>, takes one more argument at the END of the list (the first 14 dwords stay
// where they are): the step's row of the block's partials buffer, float[2 * BPR_WAVES * gridDim.x].  Lane 0 of every
// launched wavefront stores its two sums there with one 8-byte store -- exact zeros where the wavefront had no interaction,
// so that every pair of the row is written by this launch and the buffer never needs clearing -- and the block's end launch
// folds the rows into the pairs (bpr_fused_end_kernel).  No LDS, no barrier and no atomic on the loss in that form.
template <typename... LossPart>
__global__ __launch_bounds__(BPR_WAVES * 64) void bpr_fused_step_kernel(
    const int32_t* __restrict__ u_ids, const int32_t* __restrict__ i_ids, const int32_t* __restrict__ j_ids,
    const int32_t* __restrict__ meta, int n, int s_now, int dbg, int loss_slots, const float* __restrict__ P,
    const float* __restrict__ M, const float* __restrict__ V, int64_t n_par, FusedWork w, int64_t ublk0, int64_t iblk0,
    int64_t bblk0, AdamBlockArgs a, float reg, float* __restrict__ loss, const float* __restrict__ pre, LossPart... loss_part) {
    constexpr bool DEFER = sizeof...(LossPart) == 1;
    static_assert(sizeof...(LossPart) <= 1, "the existing form, or one pointer to the step's row of partials");
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    // round 1: the ids and the words in two loads -- lane L works for row L >> 2 (lanes 20 .. 63: row 4 again) and fetches
    // that row's id and word.  The first interaction's are issued here, before anything branches and beside the tables below
    // (an index past the batch is clamped: the wavefront then loads what it will not use), the next one's inside the loop
    const int lr = lane < 16 ? lane >> 2 : 4, lq = lane & 3;
    const int32_t* my_ids = lr == 0 ? u_ids : (lr & 1) ? i_ids : j_ids;
    const int32_t* my_meta = meta + static_cast<int64_t>(lr) * n;
    const int b0 = blockIdx.x * BPR_WAVES + wv, b_step = gridDim.x * BPR_WAVES;
    int32_t next_id = my_ids[b0 < n ? b0 : n - 1], next_mt = my_meta[b0 < n ? b0 : n - 1];
    // the block's per-step scalars, one step per lane (adam_math.h): loaded once, beside the ids, and read with v_readlane
    const AdamChainArgs ca = adam_chain_args(a);
    // every other argument is fetched here too, in one round of scalar loads beside the vector loads above: left alone the
    // compiler fetches each where it is first used -- behind the branches below, one dependent round after the other.  (An
    // empty statement that names them as operands: they must be in registers when it is reached.)
    asm volatile("" ::"s"(P), "s"(M), "s"(V), "s"(n_par), "s"(w.wp), "s"(w.wm), "s"(w.wv), "s"(w.g), "s"(w.cap), "s"(pre), "s"(loss));
    asm volatile("" ::"s"(ublk0), "s"(iblk0), "s"(bblk0), "s"(s_now), "s"(reg), "s"(loss_slots), "s"(dbg), "s"(ca.stats), "s"(ca.first_unit));
    asm volatile("" ::"s"(ca.one_minus_b1), "s"(ca.b2), "s"(ca.one_minus_b2), "s"(ca.eps), "s"(ca.rest_eps), "s"(ca.rest_b2k), "s"(ca.fast_vlo),
                 "s"(ca.fast_mlo), "s"(ca.fast_mhi));
    if constexpr (DEFER) asm volatile("" ::"s"(fused_loss_part(loss_part...)));
    // Issue priority over the cold pass that shares the SIMDs (side stream); dbg & 16 switches it off.  (Set behind the
    // argument loads: in front of them its test of dbg is a dependent scalar round of its own.)  Round 2 measured it
    // alone (the step +6 %, but the cold pass 0.47 -> 0.57 ms, which then bounded the block) and left it off; round 3 pairs it
    // with one more cold-pass workgroup per CU (SKR_COLD_BPC 4 -> 5), which gives the pass back what the priority takes:
    // step launch 18.7 -> 15.3 us, cold pass 0.56 -> 0.54 ms, epoch 1.083 -> 1.010 s, the 20-step slice 36.2 -> 40.2 M
    // interactions/s on the same box (tools/cold_bpc_sweep.sh; 6 per CU: epoch 0.965 s but the short slice scatters 32-40 M,
    // 7 and more: the step kernel finds no room, 21.5 us)
    if (!(dbg & 16)) __builtin_amdgcn_s_setprio(3);
    float acc_loss = 0.0f, acc_l2 = 0.0f;
    for (int b = b0; b < n; b += b_step) {
        const int32_t my_id = next_id;
        int32_t my_mt = next_mt;
        // round 2, the addresses: lane L computes ONE of the twenty, plane L & 3 (p, m, v, gradient) of its row -- the row's
        // source decides the base of p / m / v; the gradient word always comes from the workspace (any n0 field, 7
        // included, gives a buffer index 0 .. 2: inside w.g)
        int my_lim, my_from;      // my_lim, dense source: the last lane inside the buffer (the last bias block's tail; -1: none); 63 otherwise
        uint64_t my_addr;
        {
            const int64_t blk = lr == 0 ? ublk0 + my_id : lr < 3 ? iblk0 + my_id : bblk0 + (my_id >> 6);
            const int64_t slot = my_mt & ((1 << FUSED_SLOT_BITS) - 1);
            const int n0 = (my_mt >> FUSED_SLOT_BITS) & 7, prev1 = (my_mt >> 24) & 0x7f;
            // n0 == FUSED_PRE: the row's first naming in the block, and the row was cold in the block before: its zero-gradient
            // updates up to this step were applied ahead of time, beside the previous block (bpr_fused_pre_kernel) -- same bits
            const bool is_pre = n0 == FUSED_PRE, is_dense = !is_pre && prev1 == 0;
            const int64_t tail = n_par - 1 - blk * 64;
            const bool in_dense = is_dense && tail >= 0;      // (a block wholly past the end reads its slot and keeps nothing)
            my_lim = is_dense && tail < 63 ? (tail < 0 ? -1 : static_cast<int>(tail)) : 63;
            my_from = is_pre ? s_now : prev1;
            if (is_pre) my_mt &= ~(7 << FUSED_SLOT_BITS);        // n0 = 0 from here on
            const uint64_t b_dense = reinterpret_cast<uint64_t>(lq == 0 ? P : lq == 1 ? M : V);
            const uint64_t b_work = reinterpret_cast<uint64_t>(lq == 0 ? w.wp : lq == 1 ? w.wm : lq == 2 ? w.wv : w.g);
            const uint64_t b_pre = reinterpret_cast<uint64_t>(pre) + static_cast<uint64_t>(lq * w.cap) * 256;
            const int64_t e_work = lq == 3 ? ((n0 + 2) % 3) * w.cap + slot : (n0 & 1) * w.cap + slot;
            my_addr = lq == 3 ? b_work + e_work * 256 : is_pre ? b_pre + slot * 256 : in_dense ? b_dense + blk * 256 : b_work + e_work * 256;
        }
        // ... the scalars the rest of the kernel works with, and the twenty loads, issued back to back
        const int64_t i = __builtin_amdgcn_readlane(my_id, 4), j = __builtin_amdgcn_readlane(my_id, 8);
        int32_t mt[5];
        FusedRow row[5];
        int from[5];      // first zero-gradient index still to apply
        int lim[5];
#pragma unroll
        for (int r = 0; r < 5; ++r) {
            mt[r] = __builtin_amdgcn_readlane(my_mt, 4 * r);
            from[r] = __builtin_amdgcn_readlane(my_from, 4 * r);
            lim[r] = __builtin_amdgcn_readlane(my_lim, 4 * r);
            const uint32_t lo = lane < lim[r] ? lane : (lim[r] < 0 ? 0 : lim[r]);      // a lane past the end loads the last element inside
            GlobalFloats src[4];
#pragma unroll
            for (int q = 0; q < 4; ++q)
                src[q] = reinterpret_cast<GlobalFloats>(
                    static_cast<uint64_t>(static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(my_addr), 4 * r + q))) |
                    static_cast<uint64_t>(static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(my_addr >> 32), 4 * r + q))) << 32);
            row[r].p = src[0][lo];
            row[r].m = src[1][lo];
            row[r].v = src[2][lo];
            // (a relaxed load of wavefront scope: the plain load instruction, but one the compiler may not sink into the
            // branch of its only use, behind the waits for the other rows; other wavefronts may be adding to the word)
            row[r].g = __hip_atomic_load(src[3] + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        }
        next_id = my_ids[b + b_step < n ? b + b_step : n - 1], next_mt = my_meta[b + b_step < n ? b + b_step : n - 1];
        // the refined reciprocal of the bias-correction table (adam_chain_args' own three operations) is made here, behind the
        // rows' loads: made ahead of the loop it puts the wait for the tables in front of all the set-up the loop needs
        AdamChainArgs cb = ca;
        asm volatile("" : "+v"(cb.t_bc2));
        const float rb = __builtin_amdgcn_rcpf(cb.t_bc2);
        cb.t_rbc2 = __builtin_fmaf(__builtin_fmaf(-cb.t_bc2, rb, 1.0f), rb, rb);
        // (selects, never products: a gradient word that does not count may be mid-accumulation by other wavefronts)
#pragma unroll
        for (int r = 0; r < 5; ++r) {
            const bool past = lane > lim[r];
            row[r].p = past ? 1.0f : row[r].p;
            row[r].m = past ? 0.0f : row[r].m;
            row[r].v = past ? 0.0f : row[r].v;
            row[r].g = ((mt[r] >> 24) & 0x7f) != 0 ? row[r].g : 0.0f;      // (a pre-buffer row is a first naming: no previous step)
            if (!(dbg & 1)) {
                const int prev1 = (mt[r] >> 24) & 0x7f;
                const AdamRowState o = chain_advance(row[r].p, row[r].g, row[r].m, row[r].v, prev1, from[r], s_now,
                                                     r < 3 ? FC_STEP_ROW : FC_STEP_BIAS, cb);
                row[r].p = o.p, row[r].m = o.m, row[r].v = o.v;
            }
        }
        if (!(dbg & 4)) {
#pragma unroll
            for (int r = 0; r < 5; ++r) {
                if ((mt[r] >> 23) & 1) {
                    const int64_t slot = mt[r] & ((1 << FUSED_SLOT_BITS) - 1);
                    const int n0 = (mt[r] >> FUSED_SLOT_BITS) & 7;
                    const int64_t e = (((n0 + 1) & 1) * w.cap + slot) * 64 + lane;
                    // write-through (relaxed stores of agent scope: the plain vector store with sc1): nothing in this launch
                    // reads them, and the lines drain while the wavefront works, not at the kernel's end
                    __hip_atomic_store(&w.wp[e], row[r].p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(&w.wm[e], row[r].m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(&w.wv[e], row[r].v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(&w.g[(((n0 + 1) % 3) * w.cap + slot) * 64 + lane], 0.0f, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
                }
            }
        }
        const float pu = row[0].p, qi = row[1].p, qj = row[2].p;
        const float bi = __shfl(row[3].p, static_cast<int>(i & 63)), bj = __shfl(row[4].p, static_cast<int>(j & 63));
        const float xi = skr::wave_sum(pu * qi) + bi, xj = skr::wave_sum(pu * qj) + bj;
        const float x = xi - xj;
        const float z = expf(-fabsf(x));
        const float l = -(fminf(0.0f, x) - log1pf(z));
        const float sig_neg = (x >= 0.0f) ? z / (1.0f + z) : 1.0f / (1.0f + z);
        const float c = -sig_neg;
        float sq = skr::wave_sum(pu * pu + qi * qi + qj * qj);
        float* gcur[5];
#pragma unroll
        for (int r = 0; r < 5; ++r) {
            const int64_t slot = mt[r] & ((1 << FUSED_SLOT_BITS) - 1);
            const int n0 = (mt[r] >> FUSED_SLOT_BITS) & 7;
            gcur[r] = w.g + ((n0 % 3) * w.cap + slot) * 64;
        }
        if (!(dbg & 2)) {
            // a row only this interaction names at this step takes a plain store (its buffer holds nothing that counts: it was
            // cleared two namings ago, or never written); shared rows are summed by the memory-side atomic units
            const float gu = c * (qi - qj) + reg * pu, gi = c * pu + reg * qi, gj = -c * pu + reg * qj;
            if (mt[0] < 0) gcur[0][lane] = gu; else atomicAdd(&gcur[0][lane], gu);
            if (mt[1] < 0) gcur[1][lane] = gi; else atomicAdd(&gcur[1][lane], gi);
            if (mt[2] < 0) gcur[2][lane] = gj; else atomicAdd(&gcur[2][lane], gj);
        }
        sq += bi * bi + bj * bj;
        if (lane == 0 && !(dbg & 2)) {
            atomicAdd(&gcur[3][i & 63], c + reg * bi);
            atomicAdd(&gcur[4][j & 63], -c + reg * bj);
        }
        acc_loss += l;
        acc_l2 += 0.5f * sq;
    }
    if constexpr (DEFER) {
        // the loss words: one pair per WAVEFRONT, stored, for the end launch to fold
        // (b0 < BPR_WAVES * gridDim.x: inside the row.  A plain store: write-through as the owner stores, dbg & 32 for
        // tools/fused_lab.py, measured 0.14 us per launch slower -- 9.20 against 9.06 us)
        if (lane == 0 && !(dbg & 8)) {
            float* part = fused_loss_part(loss_part...) + 2 * b0;
            if (dbg & 32)
                __hip_atomic_store(reinterpret_cast<uint64_t*>(part),
                                   static_cast<uint64_t>(__float_as_uint(acc_l2)) << 32 | __float_as_uint(acc_loss), __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
            else
                *reinterpret_cast<float2*>(part) = make_float2(acc_loss, acc_l2);
        }
    } else {
        // the loss words: one pair of adds per WORKGROUP.  The SKR_LOSS_SLOTS pairs of a step lie in four 128-byte lines, and what
        // the adds cost follows their number per line: 1.5 us of the launch for these 512 (SKR_FUSED_DBG=8 takes them out), 9 us
        // for one pair per wavefront issued ahead of the gradient traffic -- built, measured, removed
        __shared__ float s_loss[BPR_WAVES], s_l2[BPR_WAVES];
        if (lane == 0) {
            s_loss[wv] = acc_loss;
            s_l2[wv] = acc_l2;
        }
        __syncthreads();
        if (threadIdx.x == 0 && !(dbg & 8)) {
            float x = 0.0f, y = 0.0f;
            for (int q = 0; q < BPR_WAVES; ++q) {
                x += s_loss[q];
                y += s_l2[q];
            }
            const int sl = 2 * (static_cast<int>(blockIdx.x) % loss_slots);
            atomicAdd(&loss[sl], x);
            atomicAdd(&loss[sl + 1], y);
        }
    }
}

// Ahead of a block, beside the block before it (side stream, behind that block's cold pass): the rows the block names that
// were COLD in the previous block -- nearly every user row -- are advanced from the block's first index to the step of their
// first naming, into the pre buffer ([3][cap][64]: p, m, v).  These zero-gradient updates depend on nothing the block
// itself does; the step launch that first names such a row then finds it current and spends nothing on catching up
// (16 updates on average at k = 32, on the critical path of the step before).  The same fused_advance call the step
// would have made: the same bits.  (Parameter order, here and in bpr_fused_end_kernel: what the first loads need -- the slot
// count, the slot tables, the tags -- inside the first 14 dwords, which arrive in SGPRs at wavefront launch.)
__global__ __launch_bounds__(256) void bpr_fused_pre_kernel(const int32_t* __restrict__ n_slots, const int32_t* __restrict__ slot_blk,
                                                            const int32_t* __restrict__ slot_fin, const int32_t* __restrict__ tag_prev,
                                                            int32_t tag_prev_value, int64_t n_par, int64_t cap,
                                                            const float* __restrict__ P, const float* __restrict__ M,
                                                            const float* __restrict__ V, float* __restrict__ pre, AdamBlockArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t slot = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (slot >= *n_slots) return;
    const int64_t blk = slot_blk[slot];
    const int first = (slot_fin[slot] >> 16) & 0xff;
    if (first == 0 || tag_prev[blk] == tag_prev_value) return;       // nothing to catch up / the previous block still owns the row
    const int64_t e = blk * 64 + lane;
    FusedRow r{1.0f, 0.0f, 0.0f, 0.0f};
    if (e < n_par) { r.p = P[e]; r.m = M[e]; r.v = V[e]; }
    fused_advance(r, 0, 0, first, a, FC_PRE);
    const int64_t o = slot * 64 + lane;
    pre[o] = r.p;
    pre[cap * 64 + o] = r.m;
    pre[2 * cap * 64 + o] = r.v;
}

// end of a k-step block: every slot is brought to the block's last index and written back; its gradient buffers are
// left zero for the next block.  fin = (number of namings mod 6) | (step of the last naming << 8) | (step of the first << 16).
// A wavefront takes two neighbouring slots.  Each row makes its own gradient update (index `last`) and its zero-gradient
// updates up to the later of the two rows' last namings; from there to the block's end two rows that both passed the
// ordinary test advance together on the packed pair form (adam_pair_ordinary: the cold pass's, the same operations per
// component).  A pair with a row that failed the test or that the `which` filter drops, and a lone last slot, run one by one.
//
// The fold of the deferred loss words (fold_wgs > 0; skr_bpr_fused_end3): the first fold_wgs workgroups of the grid -- in front,
// so that they are dispatched first and are not the launch's tail -- take one step of the block per wavefront and sum the row
// of partials its launch wrote (part_wgs workgroups of BPR_WAVES pairs).  Lane L owns word L & 1 of pair L >> 1: for the
// workgroups g = pair, pair + SKR_LOSS_SLOTS, ... in ascending order it adds ((w0 + w1) + w2) + w3 of the workgroup's four
// wavefronts -- the association of the step kernel's other form, in a fixed order instead of the atomics' -- and adds the
// sum to the step's loss word with ONE atomic (the contract stays "adds to what is there", and a stride of 0 lets the
// steps collide).  The slot workgroups' index shifts by fold_wgs.
__global__ __launch_bounds__(256) void bpr_fused_end_kernel(const int32_t* __restrict__ n_slots, const int32_t* __restrict__ slot_blk,
                                                            const int32_t* __restrict__ slot_fin, const int32_t* __restrict__ tag_next,
                                                            int32_t tag_next_value, int which, int64_t n_par, float* __restrict__ P,
                                                            float* __restrict__ M, float* __restrict__ V, FusedWork w, AdamBlockArgs a,
                                                            int fold_wgs, int part_wgs, const float* __restrict__ loss_part,
                                                            float* __restrict__ loss, int64_t loss_stride) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (static_cast<int>(blockIdx.x) < fold_wgs) {
        const int s = static_cast<int>(blockIdx.x) * 4 + wave;
        if (s >= a.k) return;
        const float* row = loss_part + static_cast<int64_t>(s) * part_wgs * (2 * BPR_WAVES) + (lane & 1);
        float sum = 0.0f;
        for (int g = lane >> 1; g < part_wgs; g += SKR_LOSS_SLOTS) {
            const float* p = row + g * (2 * BPR_WAVES);
            sum += ((p[0] + p[2]) + p[4]) + p[6];
        }
        atomicAdd(&loss[s * loss_stride + lane], sum);
        return;
    }
    const int64_t slot0 = 2 * ((static_cast<int64_t>(blockIdx.x) - fold_wgs) * 4 + wave);
    const int64_t n = *n_slots;
    if (slot0 >= n) return;
    FusedRow r[2];
    int64_t e[2];
    int last[2];
    bool live[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int64_t slot = slot0 + h;
        live[h] = slot < n;
        e[h] = 0, last[h] = 0;
        r[h] = FusedRow{1.0f, 0.0f, 0.0f, 0.0f};
        if (!live[h]) continue;
        const int64_t blk = slot_blk[slot];
        // which = 1: only the rows the NEXT block touches too (it must find them in the dense tables); 2: only the others (they
        // can be written back beside the next block's steps); 0: all
        if (which != 0 && ((tag_next[blk] == tag_next_value) != (which == 1))) {
            live[h] = false;
            continue;
        }
        const int fin = slot_fin[slot], nn = fin & 7;
        last[h] = (fin >> 8) & 0xff;
        e[h] = blk * 64 + lane;
        if (e[h] < n_par) {
            const int64_t o = ((nn & 1) * w.cap + slot) * 64 + lane;
            r[h].p = w.wp[o];
            r[h].m = w.wm[o];
            r[h].v = w.wv[o];
            r[h].g = w.g[(((nn + 2) % 3) * w.cap + slot) * 64 + lane];
        }
    }
    if (live[0] && live[1]) {
        bool ord[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            adam_moments(r[h].g, r[h].m, r[h].v, a);
            ord[h] = __builtin_amdgcn_ballot_w64(!lane_ordinary(r[h].m, r[h].v, a)) == 0;
        }
        if (ord[0] && ord[1]) {
            const int hi = last[0] > last[1] ? last[0] : last[1];
#pragma unroll
            for (int h = 0; h < 2; ++h) adam_grad_finish(r[h].p, r[h].m, r[h].v, a, last[h], hi + 1, FC_END, true);
            f32x2 p2{r[0].p, r[1].p}, m2{r[0].m, r[1].m}, v2{r[0].v, r[1].v};
            adam_pair_run(p2, m2, v2, a, hi + 1, a.k);
            r[0].p = p2.x, r[0].m = m2.x, r[0].v = v2.x;
            r[1].p = p2.y, r[1].m = m2.y, r[1].v = v2.y;
            if (a.stats && lane == 0) atomicAdd(&a.stats[FC_END_PAIRED], 2ull);
        } else {
#pragma unroll
            for (int h = 0; h < 2; ++h) adam_grad_finish(r[h].p, r[h].m, r[h].v, a, last[h], a.k, FC_END, ord[h]);
            if (a.stats && lane == 0) atomicAdd(&a.stats[FC_END_SINGLE], 2ull);
        }
    } else {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (!live[h]) continue;
            adam_grad_run(r[h].p, r[h].g, r[h].m, r[h].v, a, last[h], a.k, FC_END);
            if (a.stats && lane == 0) atomicAdd(&a.stats[FC_END_SINGLE], 1ull);
        }
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        if (!live[h]) continue;
        if (e[h] < n_par) {
            P[e[h]] = r[h].p;
            M[e[h]] = r[h].m;
            V[e[h]] = r[h].v;
        }
#pragma unroll
        for (int q = 0; q < 3; ++q) w.g[(q * w.cap + slot0 + h) * 64 + lane] = 0.0f;
    }
}

// ---- the references' words of a k-step block (skr_bpr_fused_plan): four small launches, no sort -------------------------
// named[blk] collects, as a 64-bit mask, the steps of the block that name flat block `blk`; everything a reference needs
// follows from the mask: n0 = popcount below its own step, prev = the highest set bit below it.  claimed[blk] hands out
// one owner per (step, row); the owner of a row's FIRST naming draws the row's slot.  named / claimed are all-zero between
// calls (the last launch clears what the first two set).
struct FusedPlanArgs {
    const int32_t *u, *i, *j;
    int k, b;
    int64_t ublk0, iblk0, bblk0;
    unsigned long long *named, *claimed, *shared;
    int32_t *slot_of, *meta, *slot_block, *slot_fin, *n_slots;
    const int32_t* tag_prev;      // hot-block tags of the block BEFORE this one (NULL: no row is pre-advanced)
    int32_t tag_prev_value;
};

__device__ __forceinline__ void fused_plan_refs(const FusedPlanArgs& a, int64_t t, int64_t blk[5]) {
    const int64_t u = a.u[t], i = a.i[t], j = a.j[t];
    blk[0] = a.ublk0 + u;
    blk[1] = a.iblk0 + i;
    blk[2] = a.iblk0 + j;
    blk[3] = a.bblk0 + (i >> 6);
    blk[4] = a.bblk0 + (j >> 6);
}

template <int PASS>
__global__ __launch_bounds__(256) void fused_plan_kernel(FusedPlanArgs a) {
    const int64_t t = blockIdx.x * 256ll + threadIdx.x;      // position in the block's step-major columns
    if (PASS == 0 && t == 0) *a.n_slots = 0;
    if (t >= static_cast<int64_t>(a.k) * a.b) return;
    const int s = static_cast<int>(t / a.b);
    const int64_t col = t - static_cast<int64_t>(s) * a.b;
    int64_t blk[5];
    fused_plan_refs(a, t, blk);
    const unsigned long long bit = 1ull << s;
#pragma unroll
    for (int r = 0; r < 5; ++r) {
        const int64_t e = (static_cast<int64_t>(s) * 5 + r) * a.b + col;      // this reference's word
        if (PASS == 0) {
            atomicOr(&a.named[blk[r]], bit);
            a.slot_block[e] = -1;
        } else if (PASS == 1) {
            const bool owner = (atomicOr(&a.claimed[blk[r]], bit) & bit) == 0;
            if (!owner) atomicOr(&a.shared[blk[r]], bit);                     // a second reference to the pair
            a.meta[e] = owner ? (1 << 23) : 0;
            const unsigned long long mask = a.named[blk[r]];
            // the row's first naming draws its slot: one atomic per wavefront on the shared counter (its lanes' draws are
            // numbered by their rank among the drawing lanes) -- 60 k same-address atomics per block otherwise
            const bool draws = owner && (mask & (bit - 1)) == 0;
            const unsigned long long db = __ballot(draws);
            int base = 0;
            if (db) {
                const int leader = __ffsll(static_cast<long long>(db)) - 1;
                if (static_cast<int>(threadIdx.x & 63) == leader) base = atomicAdd(a.n_slots, __popcll(db));
                base = __shfl(base, leader);
            }
            if (draws) {
                const int slot = base + __popcll(db & ((1ull << (threadIdx.x & 63)) - 1ull));
                a.slot_of[blk[r]] = slot;
                a.slot_block[slot] = static_cast<int32_t>(blk[r]);
                a.slot_fin[slot] = (__popcll(mask) % 6) | ((63 - __clzll(static_cast<long long>(mask))) << 8) | (s << 16);
            }
        } else if (PASS == 2) {
            const unsigned long long below = a.named[blk[r]] & (bit - 1);
            const int n0 = __popcll(below), prev1 = below ? 64 - __clzll(static_cast<long long>(below)) : 0;
            const int sole = (a.shared[blk[r]] & bit) ? 0 : 1;                // the pair's only reference (bit 31)
            // a first naming at step s > 0 of a row the previous block did not touch: bpr_fused_pre_kernel catches it up
            const bool pre = a.tag_prev && below == 0 && s > 0 && a.tag_prev[blk[r]] != a.tag_prev_value;
            a.meta[e] = a.meta[e] | a.slot_of[blk[r]] | ((pre ? FUSED_PRE : n0 % 6) << FUSED_SLOT_BITS) | (prev1 << 24) |
                        static_cast<int32_t>(static_cast<uint32_t>(sole) << 31);
        } else {
            a.named[blk[r]] = 0;
            a.claimed[blk[r]] = 0;
            a.shared[blk[r]] = 0;
        }
    }
}

}  // namespace

extern "C" {

// scalars and thresholds of a k-step block, kept between the k + 1 launches of the block (2k pow() calls otherwise)
static const AdamBlockArgs& fused_block_args(float lr, float beta1, float beta2, float eps, int64_t step_t0, int k) {
    struct Key {
        float lr, b1, b2, eps;
        int64_t t0;
        int k;
    };
    thread_local Key key{0, 0, 0, 0, -1, 0};
    thread_local AdamBlockArgs a{};
    if (key.lr != lr || key.b1 != beta1 || key.b2 != beta2 || key.eps != eps || key.t0 != step_t0 || key.k != k) {
        a = AdamBlockArgs{};
        adam_shared_fields(a, beta1, beta2, eps);
        a.k = k;
        adam_block_scalars(a, lr, beta1, beta2, step_t0, k, false);
        adam_block_thresholds(a, lr, beta1, beta2, eps, k);
        key = Key{lr, beta1, beta2, eps, step_t0, k};
    }
    a.stats = fused_stats_buffer();
    return a;
}

static FusedWork fused_work(float* d_work, int64_t cap) {
    const int64_t plane = cap * 64;
    return FusedWork{d_work, d_work + 2 * plane, d_work + 4 * plane, d_work + 6 * plane, cap};
}

int skr_bpr_fused_step(const float* d_p, const float* d_m, const float* d_v, int64_t n, float* d_work, int64_t cap,
                       const int32_t* d_u, const int32_t* d_i, const int32_t* d_j, const int32_t* d_meta, int n_batch,
                       int64_t user_block0, int64_t item_block0, int64_t bias_block0, float lr, float beta1, float beta2,
                       float eps, int64_t step_t0, int k, int s, float reg, float* d_loss64, void* stream) {
    return skr_bpr_fused_step2(d_p, d_m, d_v, n, d_work, cap, d_u, d_i, d_j, d_meta, n_batch, user_block0, item_block0, bias_block0, lr,
                               beta1, beta2, eps, step_t0, k, s, reg, d_loss64, nullptr, stream);
}

// workgroups of a step launch (4 096: the grid's cap, wavefronts loop beyond it); the deferred form's row of partials has
// BPR_WAVES pairs per workgroup
static int fused_step_wgs(int n_batch) {
    const int wgs = (n_batch + BPR_WAVES - 1) / BPR_WAVES;
    return wgs > 256 * 16 ? 256 * 16 : wgs;
}

// d_loss_part: NULL, the form that adds to d_loss64; else the block's partials, of which step s writes row s
static int fused_step_launch(const float* d_p, const float* d_m, const float* d_v, int64_t n, float* d_work, int64_t cap,
                             const int32_t* d_u, const int32_t* d_i, const int32_t* d_j, const int32_t* d_meta, int n_batch,
                             int64_t user_block0, int64_t item_block0, int64_t bias_block0, float lr, float beta1, float beta2,
                             float eps, int64_t step_t0, int k, int s, float reg, float* d_loss64, const float* d_pre,
                             float* d_loss_part, void* stream) {
    SKR_REQUIRE(d_p && d_m && d_v && d_work && d_u && d_i && d_j && d_meta && d_loss64, "skr_bpr_fused_step: NULL argument");
    SKR_REQUIRE(n >= 0 && n_batch >= 0 && cap >= 1 && cap <= (1 << FUSED_SLOT_BITS), "skr_bpr_fused_step: need 1 <= cap <= 2^%d",
                FUSED_SLOT_BITS);
    SKR_REQUIRE(step_t0 >= 0 && k >= 1 && k <= AB_KMAX && s >= 0 && s < k, "skr_bpr_fused_step: need 0 <= s < k <= %d", AB_KMAX);
    SKR_REQUIRE(user_block0 >= 0 && item_block0 >= 0 && bias_block0 >= 0, "skr_bpr_fused_step: bad table offsets");
    if (n_batch == 0) return SKR_OK;
    const AdamBlockArgs& a = fused_block_args(lr, beta1, beta2, eps, step_t0, k);
    static const int dbg = [] { const char* e = getenv("SKR_FUSED_DBG"); return e ? atoi(e) : 0; }();
    const int blocks = fused_step_wgs(n_batch);
    if (d_loss_part)
        hipLaunchKernelGGL(bpr_fused_step_kernel<float*>, dim3(blocks), dim3(BPR_WAVES * 64), 0, skr::as_stream(stream), d_u, d_i, d_j,
                           d_meta, n_batch, s, dbg, SKR_LOSS_SLOTS, d_p, d_m, d_v, n, fused_work(d_work, cap), user_block0, item_block0,
                           bias_block0, a, reg, d_loss64, d_pre, d_loss_part + static_cast<int64_t>(s) * blocks * (2 * BPR_WAVES));
    else
        hipLaunchKernelGGL(bpr_fused_step_kernel<>, dim3(blocks), dim3(BPR_WAVES * 64), 0, skr::as_stream(stream), d_u, d_i, d_j, d_meta,
                           n_batch, s, dbg, SKR_LOSS_SLOTS, d_p, d_m, d_v, n, fused_work(d_work, cap), user_block0, item_block0,
                           bias_block0, a, reg, d_loss64, d_pre);
    SKR_LAUNCH_CHECK();
    return SKR_OK;
}

int skr_bpr_fused_step2(const float* d_p, const float* d_m, const float* d_v, int64_t n, float* d_work, int64_t cap,
                        const int32_t* d_u, const int32_t* d_i, const int32_t* d_j, const int32_t* d_meta, int n_batch,
                        int64_t user_block0, int64_t item_block0, int64_t bias_block0, float lr, float beta1, float beta2,
                        float eps, int64_t step_t0, int k, int s, float reg, float* d_loss64, const float* d_pre, void* stream) {
    return fused_step_launch(d_p, d_m, d_v, n, d_work, cap, d_u, d_i, d_j, d_meta, n_batch, user_block0, item_block0, bias_block0, lr,
                             beta1, beta2, eps, step_t0, k, s, reg, d_loss64, d_pre, nullptr, stream);
}

int64_t skr_bpr_fused_loss_part_floats(int n_batch, int k) {
    if (n_batch <= 0 || k <= 0) return 0;
    return static_cast<int64_t>(k) * (2 * BPR_WAVES) * fused_step_wgs(n_batch);
}

int skr_bpr_fused_step3(const float* d_p, const float* d_m, const float* d_v, int64_t n, float* d_work, int64_t cap,
                        const int32_t* d_u, const int32_t* d_i, const int32_t* d_j, const int32_t* d_meta, int n_batch,
                        int64_t user_block0, int64_t item_block0, int64_t bias_block0, float lr, float beta1, float beta2,
                        float eps, int64_t step_t0, int k, int s, float reg, float* d_loss64, const float* d_pre,
                        float* d_loss_part, void* stream) {
    SKR_REQUIRE(d_loss_part, "skr_bpr_fused_step3: NULL argument");
    SKR_REQUIRE((reinterpret_cast<uintptr_t>(d_loss_part) & 7) == 0, "skr_bpr_fused_step3: d_loss_part must be 8-byte aligned");
    return fused_step_launch(d_p, d_m, d_v, n, d_work, cap, d_u, d_i, d_j, d_meta, n_batch, user_block0, item_block0, bias_block0, lr,
                             beta1, beta2, eps, step_t0, k, s, reg, d_loss64, d_pre, d_loss_part, stream);
}

int skr_bpr_fused_plan(const int32_t* d_u, const int32_t* d_i, const int32_t* d_j, int n_batch, int k, int64_t user_block0,
                       int64_t item_block0, int64_t bias_block0, int64_t n_flat_blocks, void* d_scratch, int32_t* d_meta,
                       int32_t* d_slot_block, int32_t* d_slot_fin, int32_t* d_n_slots, void* stream) {
    return skr_bpr_fused_plan2(d_u, d_i, d_j, n_batch, k, user_block0, item_block0, bias_block0, n_flat_blocks, d_scratch, d_meta,
                               d_slot_block, d_slot_fin, d_n_slots, nullptr, 0, stream);
}

int skr_bpr_fused_plan2(const int32_t* d_u, const int32_t* d_i, const int32_t* d_j, int n_batch, int k, int64_t user_block0,
                        int64_t item_block0, int64_t bias_block0, int64_t n_flat_blocks, void* d_scratch, int32_t* d_meta,
                        int32_t* d_slot_block, int32_t* d_slot_fin, int32_t* d_n_slots, const int32_t* d_tag_prev,
                        int32_t tag_prev_value, void* stream) {
    SKR_REQUIRE(d_u && d_i && d_j && d_scratch && d_meta && d_slot_block && d_slot_fin && d_n_slots, "skr_bpr_fused_plan: NULL argument");
    SKR_REQUIRE(n_batch >= 1 && k >= 1 && k <= AB_KMAX && static_cast<int64_t>(k) * 5 * n_batch <= (1 << FUSED_SLOT_BITS),
                "skr_bpr_fused_plan: need 1 <= k <= %d and k * 5 * n_batch <= 2^%d", AB_KMAX, FUSED_SLOT_BITS);
    SKR_REQUIRE(user_block0 >= 0 && item_block0 >= 0 && bias_block0 >= 0 && n_flat_blocks >= 1 && n_flat_blocks < INT32_MAX,
                "skr_bpr_fused_plan: bad table offsets");
    SKR_REQUIRE((reinterpret_cast<uintptr_t>(d_scratch) & 7) == 0, "skr_bpr_fused_plan: scratch must be 8-byte aligned");
    FusedPlanArgs a;
    a.u = d_u, a.i = d_i, a.j = d_j;
    a.k = k, a.b = n_batch;
    a.ublk0 = user_block0, a.iblk0 = item_block0, a.bblk0 = bias_block0;
    a.named = static_cast<unsigned long long*>(d_scratch);
    a.claimed = a.named + n_flat_blocks;
    a.shared = a.claimed + n_flat_blocks;
    a.slot_of = reinterpret_cast<int32_t*>(a.shared + n_flat_blocks);
    a.meta = d_meta, a.slot_block = d_slot_block, a.slot_fin = d_slot_fin, a.n_slots = d_n_slots;
    a.tag_prev = d_tag_prev, a.tag_prev_value = tag_prev_value;
    const dim3 grid(static_cast<unsigned>((static_cast<int64_t>(k) * n_batch + 255) / 256)), wg(256);
    hipLaunchKernelGGL(fused_plan_kernel<0>, grid, wg, 0, skr::as_stream(stream), a);
    hipLaunchKernelGGL(fused_plan_kernel<1>, grid, wg, 0, skr::as_stream(stream), a);
    hipLaunchKernelGGL(fused_plan_kernel<2>, grid, wg, 0, skr::as_stream(stream), a);
    hipLaunchKernelGGL(fused_plan_kernel<3>, grid, wg, 0, skr::as_stream(stream), a);
    SKR_LAUNCH_CHECK();
    return SKR_OK;
}

int skr_bpr_fused_pre(const float* d_p, const float* d_m, const float* d_v, int64_t n, float* d_pre, int64_t cap,
                      const int32_t* d_slot_block, const int32_t* d_slot_fin, const int32_t* d_n_slots, float lr, float beta1,
                      float beta2, float eps, int64_t step_t0, int k, const int32_t* d_tag_prev, int32_t tag_prev_value,
                      void* stream) {
    SKR_REQUIRE(d_p && d_m && d_v && d_pre && d_slot_block && d_slot_fin && d_n_slots && d_tag_prev, "skr_bpr_fused_pre: NULL argument");
    SKR_REQUIRE(n >= 0 && cap >= 1 && cap <= (1 << FUSED_SLOT_BITS), "skr_bpr_fused_pre: need 1 <= cap <= 2^%d", FUSED_SLOT_BITS);
    SKR_REQUIRE(step_t0 >= 0 && k >= 1 && k <= AB_KMAX, "skr_bpr_fused_pre: need 1 <= k <= %d", AB_KMAX);
    // (scalars of its own: this runs on another stream than the block's steps, one block ahead of them)
    AdamBlockArgs a{};
    adam_shared_fields(a, beta1, beta2, eps);
    a.k = k;
    adam_block_scalars(a, lr, beta1, beta2, step_t0, k, false);
    adam_block_thresholds(a, lr, beta1, beta2, eps, k);
    a.stats = fused_stats_buffer();
    hipLaunchKernelGGL(bpr_fused_pre_kernel, dim3(static_cast<unsigned>((cap + 3) / 4)), dim3(256), 0, skr::as_stream(stream), d_n_slots,
                       d_slot_block, d_slot_fin, d_tag_prev, tag_prev_value, n, cap, d_p, d_m, d_v, d_pre, a);
    SKR_LAUNCH_CHECK();
    return SKR_OK;
}

// fold_wgs > 0: the launch also folds the block's deferred loss words (part_wgs: the workgroups of its step launches)
static int fused_end_launch(float* d_p, float* d_m, float* d_v, int64_t n, float* d_work, int64_t cap, const int32_t* d_slot_block,
                            const int32_t* d_slot_fin, const int32_t* d_n_slots, float lr, float beta1, float beta2, float eps,
                            int64_t step_t0, int k, const int32_t* d_tag_next, int32_t tag_next_value, int which, int fold_wgs,
                            int part_wgs, const float* d_loss_part, float* d_loss64, int64_t loss_stride_floats, void* stream) {
    SKR_REQUIRE(d_p && d_m && d_v && d_work && d_slot_block && d_slot_fin && d_n_slots, "skr_bpr_fused_end: NULL argument");
    SKR_REQUIRE(n >= 0 && cap >= 1 && cap <= (1 << FUSED_SLOT_BITS), "skr_bpr_fused_end: need 1 <= cap <= 2^%d", FUSED_SLOT_BITS);
    SKR_REQUIRE(step_t0 >= 0 && k >= 1 && k <= AB_KMAX, "skr_bpr_fused_end: need 1 <= k <= %d", AB_KMAX);
    SKR_REQUIRE(which >= 0 && which <= 2 && (which == 0 || d_tag_next), "skr_bpr_fused_end: which must be 0, or 1 / 2 with the next block's tags");
    const AdamBlockArgs& a = fused_block_args(lr, beta1, beta2, eps, step_t0, k);
    hipLaunchKernelGGL(bpr_fused_end_kernel, dim3(static_cast<unsigned>(fold_wgs + (cap + 7) / 8)), dim3(256), 0, skr::as_stream(stream),
                       d_n_slots, d_slot_block, d_slot_fin, d_tag_next, tag_next_value, which, n, d_p, d_m, d_v, fused_work(d_work, cap), a,
                       fold_wgs, part_wgs, d_loss_part, d_loss64, loss_stride_floats);
    SKR_LAUNCH_CHECK();
    return SKR_OK;
}

int skr_bpr_fused_end(float* d_p, float* d_m, float* d_v, int64_t n, float* d_work, int64_t cap, const int32_t* d_slot_block,
                      const int32_t* d_slot_fin, const int32_t* d_n_slots, float lr, float beta1, float beta2, float eps,
                      int64_t step_t0, int k, const int32_t* d_tag_next, int32_t tag_next_value, int which, void* stream) {
    return fused_end_launch(d_p, d_m, d_v, n, d_work, cap, d_slot_block, d_slot_fin, d_n_slots, lr, beta1, beta2, eps, step_t0, k,
                            d_tag_next, tag_next_value, which, 0, 0, nullptr, nullptr, 0, stream);
}

int skr_bpr_fused_end3(float* d_p, float* d_m, float* d_v, int64_t n, float* d_work, int64_t cap, const int32_t* d_slot_block,
                       const int32_t* d_slot_fin, const int32_t* d_n_slots, float lr, float beta1, float beta2, float eps,
                       int64_t step_t0, int k, const int32_t* d_tag_next, int32_t tag_next_value, int which,
                       const float* d_loss_part, float* d_loss64, int64_t loss_stride_floats, int n_batch, void* stream) {
    SKR_REQUIRE(d_loss_part && d_loss64, "skr_bpr_fused_end3: NULL argument");
    SKR_REQUIRE(loss_stride_floats >= 0 && n_batch >= 0, "skr_bpr_fused_end3: bad shape");
    // one wavefront per step, four to a workgroup; the which = 2 launch (the leftovers, on another stream) folds nothing, and
    // an empty batch launched no step
    const bool fold = which != 2 && n_batch > 0 && k >= 1;
    return fused_end_launch(d_p, d_m, d_v, n, d_work, cap, d_slot_block, d_slot_fin, d_n_slots, lr, beta1, beta2, eps, step_t0, k,
                            d_tag_next, tag_next_value, which, fold ? (k + 3) / 4 : 0, fused_step_wgs(n_batch), d_loss_part, d_loss64,
                            loss_stride_floats, stream);
}

int skr_bpr_fused_block(float* d_p, float* d_m, float* d_v, int64_t n, float* d_work, int64_t cap, const int32_t* d_u,
                        const int32_t* d_i, const int32_t* d_j, const int32_t* d_meta, int n_batch, int64_t user_block0,
                        int64_t item_block0, int64_t bias_block0, float lr, float beta1, float beta2, float eps, int64_t step_t0,
                        int k, float reg, float* d_loss64, int64_t loss_stride_floats, const int32_t* d_slot_block,
                        const int32_t* d_slot_fin, const int32_t* d_n_slots, const int32_t* d_tag_next, int32_t tag_next_value,
                        void* stream) {
    return skr_bpr_fused_block2(d_p, d_m, d_v, n, d_work, cap, d_u, d_i, d_j, d_meta, n_batch, user_block0, item_block0, bias_block0, lr,
                                beta1, beta2, eps, step_t0, k, reg, d_loss64, loss_stride_floats, d_slot_block, d_slot_fin, d_n_slots,
                                d_tag_next, tag_next_value, nullptr, stream);
}

int skr_bpr_fused_block2(float* d_p, float* d_m, float* d_v, int64_t n, float* d_work, int64_t cap, const int32_t* d_u,
                         const int32_t* d_i, const int32_t* d_j, const int32_t* d_meta, int n_batch, int64_t user_block0,
                         int64_t item_block0, int64_t bias_block0, float lr, float beta1, float beta2, float eps, int64_t step_t0,
                         int k, float reg, float* d_loss64, int64_t loss_stride_floats, const int32_t* d_slot_block,
                         const int32_t* d_slot_fin, const int32_t* d_n_slots, const int32_t* d_tag_next, int32_t tag_next_value,
                         const float* d_pre, void* stream) {
    SKR_REQUIRE(k >= 1 && k <= AB_KMAX && n_batch >= 0 && loss_stride_floats >= 0, "skr_bpr_fused_block: bad shape");
    for (int s = 0; s < k; ++s) {
        const int64_t o = static_cast<int64_t>(s) * n_batch;
        const int rc = skr_bpr_fused_step2(d_p, d_m, d_v, n, d_work, cap, d_u + o, d_i + o, d_j + o, d_meta + 5 * o, n_batch, user_block0,
                                           item_block0, bias_block0, lr, beta1, beta2, eps, step_t0, k, s, reg,
                                           d_loss64 + s * loss_stride_floats, d_pre, stream);
        if (rc != SKR_OK) return rc;
    }
    return skr_bpr_fused_end(d_p, d_m, d_v, n, d_work, cap, d_slot_block, d_slot_fin, d_n_slots, lr, beta1, beta2, eps, step_t0, k,
                             d_tag_next, tag_next_value, d_tag_next ? 1 : 0, stream);
}

int skr_bpr_fused_block3(float* d_p, float* d_m, float* d_v, int64_t n, float* d_work, int64_t cap, const int32_t* d_u,
                         const int32_t* d_i, const int32_t* d_j, const int32_t* d_meta, int n_batch, int64_t user_block0,
                         int64_t item_block0, int64_t bias_block0, float lr, float beta1, float beta2, float eps, int64_t step_t0,
                         int k, float reg, float* d_loss64, int64_t loss_stride_floats, const int32_t* d_slot_block,
                         const int32_t* d_slot_fin, const int32_t* d_n_slots, const int32_t* d_tag_next, int32_t tag_next_value,
                         const float* d_pre, float* d_loss_part, void* stream) {
    SKR_REQUIRE(k >= 1 && k <= AB_KMAX && n_batch >= 0 && loss_stride_floats >= 0, "skr_bpr_fused_block3: bad shape");
    SKR_REQUIRE(d_loss_part && d_loss64, "skr_bpr_fused_block3: NULL argument");
    for (int s = 0; s < k; ++s) {
        const int64_t o = static_cast<int64_t>(s) * n_batch;
        const int rc = skr_bpr_fused_step3(d_p, d_m, d_v, n, d_work, cap, d_u + o, d_i + o, d_j + o, d_meta + 5 * o, n_batch, user_block0,
                                           item_block0, bias_block0, lr, beta1, beta2, eps, step_t0, k, s, reg, d_loss64, d_pre,
                                           d_loss_part, stream);
        if (rc != SKR_OK) return rc;
    }
    return skr_bpr_fused_end3(d_p, d_m, d_v, n, d_work, cap, d_slot_block, d_slot_fin, d_n_slots, lr, beta1, beta2, eps, step_t0, k,
                              d_tag_next, tag_next_value, d_tag_next ? 1 : 0, d_loss_part, d_loss64, loss_stride_floats, n_batch,
                              stream);
}

}  // extern "C"
