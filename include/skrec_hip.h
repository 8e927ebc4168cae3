/* skrec_hip.h -- C ABI of libskrec_hip.so, the MI355X (gfx950) implementation of
 * scikit-recommender's data-parallel hot path.
 *
 * Rules of the boundary
 *   - plain C: no C++ types, no exceptions, no torch types; every pointer named d_* is a DEVICE
 *     pointer (HBM), every other pointer is a host pointer;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); all work is enqueued on it
 *     and nothing synchronises the host unless the function says so;
 *   - caller-owned buffers, like the reference's native functions (randint.h:75, evaluate.h:57);
 *   - every function returns 0 on success or a negative skr_status; skr_last_error() gives the text.
 *     Where the reference would spin forever or crash on bad input (randint.h:38-48 with an
 *     exclusion set covering the range; metric_dict[] with an unknown id, evaluate.h:50) this
 *     library returns SKR_EINVAL instead.
 *   - integer widths follow the reference: item/user ids and sizes are 32-bit `int`
 *     (pyx_init.pyx:6-16 asserts it), CSR row pointers are int64.
 *
 * Each entry point cites the reference interface it replaces (paths relative to the reference
 * root, skrec/...).  INTEGRATION.md shows the reference-side binding for each.
 */
#ifndef SKREC_HIP_H
#define SKREC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum skr_status {
    SKR_OK = 0,
    SKR_EINVAL = -1,   /* bad argument (the text says which) */
    SKR_EHIP = -2,     /* a HIP runtime call failed */
    SKR_ENOMEM = -3,   /* workspace too small / allocation failed */
    SKR_ENODEV = -4,   /* no gfx950 device visible */
    SKR_EOVERFLOW = -5 /* an internal bounded buffer overflowed (result invalid) */
} skr_status;

/* metric ids = skrec/utils/py/evaluator.py:57 and utils/py/cython/include/metric.h:112-118 */
enum { SKR_PRECISION = 1, SKR_RECALL = 2, SKR_MAP = 3, SKR_NDCG = 4, SKR_MRR = 5 };

int skr_abi_version(void);            /* bumped on every signature change */
const char* skr_last_error(void);     /* thread-local, valid until the next failing call */
int skr_device_count(void);           /* number of visible HIP devices (0 on a CPU-only host) */
int skr_device_summary(char* buf, size_t n); /* "gfx950 256CU ..." of the current device */
/* Longest row of a device CSR (host result; synchronises).  The host mirror uses it for the
 * reference's argument checks (pyx_random.pyx:49) and for the fused evaluator's precondition. */
int skr_csr_max_row_len(const int64_t* d_rowptr, int n_rows, int* out_max, void* stream);

/* ============================================================================================
 * S -- negative sampling
 * replaces: c_randint_choice / _random_int / global `std::mt19937 _gen(2020)`
 *           (utils/py/cython/include/randint.h:20-88), its Cython glue pyx_randint_choice
 *           (utils/py/cython/pyx_random.pyx:20-76) and the per-user Python loop
 *           _sampling_negative_items (io/data_iterator.py:81-94).
 * ========================================================================================== */
typedef struct skr_sampler skr_sampler; /* owns one MT19937 stream, resident in HBM */

/* seed 2020 reproduces the reference's process-global stream (randint.h:20). */
int skr_sampler_create(uint32_t seed, skr_sampler** out);
int skr_sampler_destroy(skr_sampler* s);
/* Raw state exchange (624 untempered words + position 0..624), host buffers; synchronises. */
int skr_sampler_get_state(skr_sampler* s, uint32_t* words624, int* pos);
int skr_sampler_set_state(skr_sampler* s, const uint32_t* words624, int pos);
/* Total raw 32-bit words consumed since creation / set_state (synchronises). */
int skr_sampler_draws(skr_sampler* s, uint64_t* n);
/* How the last exact epoch ran (test / measurement hook; synchronises the device): h_info4 = {status, handed_over,
 * slots filled, words consumed}.  status 0 = the one-workgroup path (dense data, small calls, SKR_EXACT_PATH=serial),
 * 1 = the slab path (sampler.hip 2d) and every slot was filled, 2 = slab path, the generated words ran out (the next
 * exact-epoch call reports it as an error).  handed_over 1 = the slab path met a case it leaves to the serial kernel and
 * that kernel finished the stream. */
int skr_sampler_last_epoch(skr_sampler* s, int64_t* h_info4);
/* The slab path's resolver in the last exact epoch (test / measurement hook; synchronises): h_info2 = {most fixed-point rounds
 * one slab took, slabs the rounds did not settle within their cap (32; SKR_SLAB_ROUNDS lowers it) and the one-lane walk
 * decided}.  Both 0 when no slab was resolved by rounds (the serial path, SKR_SLAB_WALK=1). */
int skr_sampler_slab_stats(skr_sampler* s, int64_t* h_info2);
/* The next n tempered words of the stream (what std::mt19937's operator() returns, in order) to d_out (uint32[n], device);
 * the stream moves past them.  Queues work only.  Long stretches take the jump-ahead generator (SKR_MT_JUMP=0: the
 * one-workgroup generator, same words). */
int skr_sampler_words(skr_sampler* s, int64_t n, uint32_t* d_out, void* stream);
/* Host only, no GPU: the MT19937 state n words after (words624, pos), by jump-ahead polynomial (test hook of the generator
 * above).  The result is the block that holds the next word and the position in it (out_pos < 624 unless n + pos <= 624). */
int skr_mt_jump_host(const uint32_t* words624, int pos, int64_t n, uint32_t* out624, int* out_pos);

/* One call of c_randint_choice (randint.h:75): `size` draws from [0, high), written to d_result.
 *   replace      as the reference's bool;
 *   d_prob       NULL (uniform, randint.h:84) or float[high] weights (discrete, randint.h:79);
 *   d_exclusion  NULL or int[n_exclusion] SORTED ascending, unique (replaces unordered_set<int>).
 * Runs the reference's serial algorithm on the device (one lane), bit-exact with the reference
 * stream; meant for the API-surface calls (random.py:9), not for epochs.  Validates like
 * pyx_random.pyx:34-54 and returns SKR_EINVAL where the reference raises ValueError. */
int skr_randint_choice(skr_sampler* s, int high, int size, int replace, const float* d_prob,
                       const int32_t* d_exclusion, int n_exclusion, int32_t* d_result, void* stream);

/* A whole epoch of _sampling_negative_items (data_iterator.py:81-94) in one call, EXACT STREAM:
 * for users 0..n_users-1 ascending, rows with no positives skipped, n_pos(u)*num_neg uniform draws
 * from [0, num_items) rejecting u's train positives -- consuming the sampler's MT19937 stream in
 * exactly the reference's order, so d_out is bit-identical to the reference's concatenated array
 * and the stream continues into the next epoch.
 *   d_rowptr      int64[n_users+1] CSR offsets of the train positives
 *   d_pos_sorted  int32[nnz] positives, ascending within each row (membership test only; the
 *                 pairing with positives in file order is the caller's, data_iterator.py:30-42)
 *   nnz           == rowptr[n_users] (the caller knows it; avoids a device read-back)
 *   d_out         int32[nnz*num_neg]  (== reshape [nnz, num_neg] when num_neg > 1, :91)
 * Synchronises the stream once at the end (it must learn how many words were consumed). */
int skr_sample_epoch_exact(skr_sampler* s, int num_items, int n_users, const int64_t* d_rowptr,
                           const int32_t* d_pos_sorted, int64_t nnz, int num_neg, int32_t* d_out, void* stream);
/* The same epoch without the read-back at the start of the call: the row statistics of the CSR (longest row, sum of squared
 * row lengths: h_stats2[0], [1]) are taken ONCE with skr_csr_row_stats (which waits for its own kernel) -- a data set's CSR does
 * not change between epochs (data_iterator.py:30-42 builds it in the constructor) -- and the call only queues work.  A failure of
 * the PREVIOUS epoch (stream exhausted) is reported from a status word that was copied to the host behind that epoch. */
int skr_csr_row_stats(const int64_t* d_rowptr, int n_rows, int64_t* h_stats2, void* stream);
int skr_sample_epoch_exact_stats(skr_sampler* s, int num_items, int n_users, const int64_t* d_rowptr, const int32_t* d_pos_sorted,
                                 int64_t nnz, int num_neg, int32_t* d_out, const int64_t* h_stats2, void* stream);

/* The same exact-stream epoch when the number of draws of a user is NOT the size of its exclusion set:
 * the sequential iterators (data_iterator.py:237-331: one draw group per training sequence, exclusion =
 * the user's whole history, `user_n_pos` from _generative_time_order_positive_items :44-78) and the
 * knowledge-graph iterator (_sampling_negative_tails :406-420: one group per triple of a head,
 * exclusion = its distinct tails).  Users ascending, users with no draws skipped, exactly as the
 * reference's loop over `user_n_pos.items()`.
 *   d_rowptr / d_excl_sorted  CSR of the exclusion sets (ascending within a row), nnz entries
 *   d_drawptr                 int64[n_users+1] cumulative number of draws; n_draws == d_drawptr[n_users]
 *   d_out                     int32[n_draws] */
int skr_sample_epoch_exact_counts(skr_sampler* s, int num_items, int n_users, const int64_t* d_rowptr,
                                  const int32_t* d_excl_sorted, int64_t nnz, const int64_t* d_drawptr, int64_t n_draws,
                                  int32_t* d_out, void* stream);

/* The same distribution, embarrassingly parallel: slot a of user u in epoch e draws from a
 * xoshiro128++ stream keyed by (seed, epoch, global slot index), Lemire-mapped to [0, num_items),
 * retried until not in u's positives.  Bit-exact with its CPU twin (tests/fast_sampler_twin.py),
 * equal to the reference in law only; independent of how users are sharded over GPUs when
 * slot_offset is the global index of this shard's first slot.  Never synchronises.  A row that
 * covers the whole catalogue (rejected with ValueError by pyx_random.pyx:49; the host mirror checks
 * it) yields -1 instead of spinning. */
int skr_sample_epoch_fast(uint64_t seed, uint64_t epoch, int64_t slot_offset, int num_items, int n_users,
                          const int64_t* d_rowptr, const int32_t* d_pos_sorted, int64_t nnz, int num_neg,
                          int32_t* d_out, void* stream);

/* ============================================================================================
 * E -- full-catalogue top-K evaluation
 * replaces: cpp_evaluate_matrix / eval_one_user (utils/py/cython/include/evaluate.h:24-76),
 *           the five metric functions (include/metric.h:19-118), eval_score_matrix
 *           (utils/py/cython/pyx_eval_matrix.pyx:22-37), and -- in the fused form -- also
 *           _MF.predict / _LightGCN.predict's U[b] @ V.T (+bias) (recommender/BPRMF.py:84-88,
 *           LightGCN.py:102-107) and the -inf train masking loop (utils/py/evaluator.py:197-200).
 * Equal scores: skr_eval_scores reproduces the reference's order, which is whatever libstdc++'s
 * partial_sort_copy heap leaves (evaluate.h:42-43) -- rows with ties among their best K+1 scores are
 * re-ranked by that very algorithm.  The fused form ranks equal scores by ascending item id (its fp32
 * summation order differs from any host GEMM's anyway, so score ties are not reproducible there).
 * ========================================================================================== */

/* Drop-in for cpp_evaluate_matrix (evaluate.h:57): d_scores [n_users, ld] row-major fp32 (first
 * n_items columns used), already train-masked by the caller.
 *   d_test_rowptr/d_test_items  CSR of each row's ground truth, items SORTED ascending, unique
 *   metric[n_metric]            host array of metric ids 1..5, output is metric-major
 *   d_rows      float[n_users, n_metric*top_k]   per-user metric rows (may be NULL)
 *   d_topk_ids  int32[n_users, top_k]            the arg-top-K lists (may be NULL)
 *   d_sums      double[n_metric*top_k]           += column sums over users (may be NULL)
 * Requires 1 <= top_k <= min(n_items, SKR_MAX_TOPK). */
#define SKR_MAX_TOPK 128
/* skr_eval_scores and skr_rank_metrics (the score-matrix path) rank deeper: the reference's top_k is a free integer
 * (run_config.py:16; its default (10, ..., 100) fits the fused kernel too) */
#define SKR_MAX_TOPK_SCORES 512
int skr_eval_scores(const float* d_scores, int n_users, int n_items, int64_t ld,
                    const int64_t* d_test_rowptr, const int32_t* d_test_items,
                    const int* metric, int n_metric, int top_k,
                    float* d_rows, int32_t* d_topk_ids, double* d_sums, void* stream);

/* Fused scoring + masking + top-K, no [B, I] matrix in HBM:
 *   score(b, i) = dot(d_user_table[d_users[b]], d_item_table[i]) (+ d_item_bias[i] if non-NULL),
 *   train positives of user d_users[b] excluded, K best (score desc, id asc) written per row.
 *   d_user_table [*, dim], d_item_table [n_items, dim] fp32 row-major, 16-byte aligned; dim is 64, 128, 192 or 256
 *                (anything else: SKR_EINVAL naming the four widths).  Narrower factors live in rows zero-padded by the
 *                caller to the next of these widths; the padding adds exact zeros and does not change a score.
 *   d_users      int32[B] user ids (also index the train CSR rows)
 *   d_train_rowptr/d_train_items  CSR over ALL users, items sorted ascending (may be NULL: no mask)
 *   d_topk_ids int32[B, top_k], d_topk_scores float[B, top_k] (may be NULL)
 *   d_work / work_bytes   scratch from skr_eval_fused_workspace(B, top_k): the same size at every width (the candidate
 *                lists are per user; at 64 C columns a wavefront holds 64 / C users of them, 16 at C = 3)
 * Arithmetic (environment SKR_FUSED_MODE, read per call).  "f16x2" (default): every operand, scaled by a power of two
 * per table, is split into TWO fp16 pieces and a product formed from three fp16 MFMA products with fp32 accumulation;
 * fp32-level accuracy (measured error vs float64 below the plain chain's) holds while the scores that decide a list
 * lie well above an absolute floor set by the largest elements of the two tables -- checked per user on the device,
 * and every user that fails is recomputed by the bf16x3 kernel inside the same call (skr_eval_fused_rejected counts
 * them).  The guard accepts a user whose smallest returned |score| is at least 2^19 * 2^ceil(log2(dim / 64)) / (s_u s_v),
 * s_u, s_v being the two tables' scales: the floor grows with the length of the dot product, the constant with it, and at
 * dim == 64 it is the 2^19 it has always been.  "bf16x3": three bf16 pieces, six MFMA products, no condition on the operands (fused_topk_kernel_v6, 16-item
 * steps on v_mfma_f32_16x16x32_bf16).
 * "fp32": exact fp32 FMA chains on the FP32 MFMA, built for dim == 64 only: with dim > 64 the call is refused with
 * SKR_EINVAL (the message names the mode and the width) before any device call, and the caller ranks through
 * skr_score_matrix / skr_mask_train / skr_eval_scores.  Within a row the summation order is fixed (64-column slices in
 * ascending order, the bias first), so two calls give the same bits; no floating-point atomic is used.  The split modes keep library-owned device buffers for the split
 * item table (n_items*dim*6 bytes, f16x2: + n_items*dim*4), one set per process: calls in a split mode must be issued
 * on ONE stream at a time (calls on the same stream queue behind each other, which is what the evaluator does).
 * Requires n_items - max train row length >= top_k (else SKR_EINVAL: use skr_eval_scores). */
size_t skr_eval_fused_workspace(int B, int top_k);
/* SKR_FUSED_MODE=f16x2 only: how many rows of the LAST skr_eval_fused_topk call on `stream` its guard did not accept and
 * handed to the bf16x3 kernel (written to *h_count on the host; blocks until that call is done; 0 in the other modes). */
int skr_eval_fused_rejected(int32_t* h_count, void* stream);
int skr_eval_fused_topk(const float* d_user_table, const int32_t* d_users, int B,
                        const float* d_item_table, const float* d_item_bias, int n_items, int dim,
                        const int64_t* d_train_rowptr, const int32_t* d_train_items,
                        int top_k, int32_t* d_topk_ids, float* d_topk_scores,
                        void* d_work, size_t work_bytes, void* stream);

/* Dense score matrix of the predict() API surface (_MF.predict, BPRMF.py:84-88; _LightGCN.predict,
 * LightGCN.py:102-107): d_scores[b, i] = <user_table[d_users[b]], item_table[i]> (+ d_item_bias[i]),
 * fp32 fma chain in ascending k, bias added last.  The evaluator does not use it (it never needs
 * the matrix); it exists so that predict() has no torch kernel behind it.  dim == 64. */
int skr_score_matrix(const float* d_user_table, const int32_t* d_users, int B, const float* d_item_table,
                     const float* d_item_bias, int n_items, int dim, float* d_scores, int64_t ld, void* stream);

/* evaluator.py:197-200 on the device: d_scores[b, i] = -inf for every train item i of user
 * d_users[b] (generic path, when a foreign model hands over a dense [B, n_items] score matrix). */
int skr_mask_train(float* d_scores, int B, int n_items, int64_t ld, const int32_t* d_users,
                   const int64_t* d_train_rowptr, const int32_t* d_train_items, void* stream);

/* Metric rows from arg-top-K lists (metric.h:19-109); truth row of list b is d_truth_rows[b]
 * (NULL: row b).  Same outputs as skr_eval_scores. */
int skr_rank_metrics(const int32_t* d_topk_ids, int B, int top_k, const int32_t* d_truth_rows,
                     const int64_t* d_test_rowptr, const int32_t* d_test_items,
                     const int* metric, int n_metric, float* d_rows, double* d_sums, void* stream);

/* ============================================================================================
 * T -- BPR lookup-and-score forward/backward, optimiser, graph propagation
 * replaces stock torch ops of the reference (no native counterpart there):
 *   _MF.forward + bpr_loss + l2_loss + autograd backward   recommender/BPRMF.py:77-82,114-126,
 *                                                           utils/torch.py:20-21,62-74
 *   torch.optim.Adam (dense, every row every step)          BPRMF.py:99,127
 *   torch.sparse.mm(norm_adj, E) per layer, layer mean      LightGCN.py:89-100
 *   cosine re-weighting, layer sum                          LayerGCN.py:207-220
 * All tables fp32 row-major with dim == 64.
 * ========================================================================================== */

/* One BPR batch, forward + backward, gradients ACCUMULATED (atomically) into dense buffers that
 * the caller zeroed:  x = <P_u,Q_i> + b_i - <P_u,Q_j> - b_j ;  loss_b = softplus(-x)
 *   d_loss[0] += sum_b loss_b * loss_scale      (BPRMF: 1, sum, BPRMF.py:117; LightGCN: 1/n, mean)
 *   d_loss[1] += 0.5*sum of squares of the gathered REG rows (l2_loss, torch.py:66-74)
 *   grads of the score part go to d_gP/d_gQ/d_gb (tables the scores were computed from);
 *   reg * reg_scale * row goes to d_gRP/d_gRQ (+ d_gb for the bias), computed from d_RP/d_RQ --
 *   for BPRMF these are the same tables (BPRMF.py:118-124); for LightGCN/LayerGCN the scores use
 *   the propagated tables and the regulariser the ego tables (LightGCN.py:192-196).
 *   d_bias / d_gb may be NULL (no item bias).
 *   d_touch (may be NULL): one byte per 64-float block of the gradient allocation that starts at
 *   d_touch_base; every block this call adds into gets its byte set to 1, so that skr_adam_step
 *   can skip reading (and re-zeroing) the gradient of blocks nobody touched. */
int skr_bpr_step(const float* d_P, const float* d_Q, const float* d_bias,
                 const float* d_RP, const float* d_RQ,
                 const int32_t* d_u, const int32_t* d_i, const int32_t* d_j, int n,
                 float loss_scale, float reg, float reg_scale,
                 float* d_gP, float* d_gQ, float* d_gb, float* d_gRP, float* d_gRQ,
                 float* d_loss, uint8_t* d_touch, const float* d_touch_base, void* stream);
/* skr_bpr_step on one rank of a user-sharded job: d_u / d_i / d_j hold a GLOBAL batch of n triples with
 * GLOBAL user ids; only the triples whose user this rank owns (u % shard_world == shard_rank) are processed, against row
 * u / shard_world of the rank's local user tables.  No selection on the host, no read-back of a count.
 * grad_scale multiplies the score part of the gradient only (d_gP / d_gQ / d_gb), not the loss sums nor the regulariser's
 * gradient: LightGCN passes 1 / (n_layers + 1), the factor of the layer mean (LightGCN.py:97-99), instead of scaling the
 * [N, 64] gradient buffer in a pass of its own. */
int skr_bpr_step_sharded(const float* d_P, const float* d_Q, const float* d_bias, const float* d_RP, const float* d_RQ,
                         const int32_t* d_u, const int32_t* d_i, const int32_t* d_j, int n, float loss_scale, float reg,
                         float reg_scale, float* d_gP, float* d_gQ, float* d_gb, float* d_gRP, float* d_gRQ, float* d_loss,
                         uint8_t* d_touch, const float* d_touch_base, int shard_world, int shard_rank, float grad_scale,
                         void* stream);
/* skr_bpr_step with the two loss sums spread over SKR_LOSS_SLOTS pairs: d_loss64 is float[2 * SKR_LOSS_SLOTS], pair q
 * receives the sums of the workgroups q, q + SKR_LOSS_SLOTS, ...; the batch's sums are the sums over the pairs.  (One
 * pair of words for all workgroups makes their atomics serialise: 4.5 us of a 10.9 us launch at batch 1024.) */
#define SKR_LOSS_SLOTS 32
int skr_bpr_step_spread(const float* d_P, const float* d_Q, const float* d_bias,
                 const float* d_RP, const float* d_RQ,
                 const int32_t* d_u, const int32_t* d_i, const int32_t* d_j, int n,
                 float loss_scale, float reg, float reg_scale,
                 float* d_gP, float* d_gQ, float* d_gb, float* d_gRP, float* d_gRQ,
                 float* d_loss64, uint8_t* d_touch, const float* d_touch_base, void* stream);
/* The general form: rows of `dim` floats (64, 128, 192 or 256; an embedding width that is not a multiple of 64 -- n_dim /
 * embed_size are free integers in the reference, BPRMF.py:27,51, LightGCN.py:34 -- is zero-padded by the caller: padded
 * columns have zero gradients and stay zero under Adam), loss_slots 1 (d_loss[2]) or SKR_LOSS_SLOTS (d_loss[2 * slots]),
 * grad_scale as in skr_bpr_step_sharded. */
int skr_bpr_step_dim(const float* d_P, const float* d_Q, const float* d_bias, const float* d_RP, const float* d_RQ,
                     const int32_t* d_u, const int32_t* d_i, const int32_t* d_j, int n, int dim, float loss_scale,
                     float reg, float reg_scale, float* d_gP, float* d_gQ, float* d_gb, float* d_gRP, float* d_gRQ,
                     float* d_loss, int loss_slots, uint8_t* d_touch, const float* d_touch_base, float grad_scale,
                     void* stream);

/* torch.optim.Adam.step for one dense parameter (single-tensor path): for every element
 *   m = m + (g-m)*(1-b1);  v = v*b2 + (1-b2)*g*g;
 *   p -= (lr/(1-b1^t)) * m / (sqrt(v)/sqrt(1-b2^t) + eps)
 * step_t is the 1-based step count.  If zero_grad != 0 the gradient buffer is zeroed in the same
 * pass (the next step's optimizer.zero_grad(), BPRMF.py:125).
 * d_touch (may be NULL): one byte per 64-float block of d_g.  0 = the block's gradient is known to
 * be all zero (it is neither read nor written: 24 instead of 32 bytes of traffic per parameter,
 * same result bit for bit); 1 = read it, then clear the byte; 2 = always read, never cleared. */
int skr_adam_step(float* d_p, float* d_g, float* d_m, float* d_v, int64_t n,
                  float lr, float beta1, float beta2, float eps, int64_t step_t, int zero_grad,
                  uint8_t* d_touch, void* stream);

/* Y = A * X for a CSR matrix with fp32 values and dim == 64 (torch.sparse.mm, LightGCN.py:94);
 *   optional fused epilogues:  Y += d_addend (same shape, may be NULL);
 *                              d_accum += accum_scale * Y (layer mean/sum, may be NULL). */
int skr_csr_spmm(int n_rows, const int64_t* d_rowptr, const int32_t* d_col, const float* d_val,
                 const float* d_X, int dim, int64_t nnz, const float* d_addend, float* d_Y,
                 float* d_accum, float accum_scale, void* stream);

/* The same with a row stride: X, addend, Y and accum are 64-column slices of [*, ld] tables (ld >= 64 floats) -- a wider
 * embedding is multiplied slice by slice (pointers advanced by 64 c), the product being separable in the columns. */
int skr_csr_spmm_strided(int n_rows, const int64_t* d_rowptr, const int32_t* d_col, const float* d_val,
                         const float* d_X, int dim, int ld, int64_t nnz, const float* d_addend, float* d_Y,
                         float* d_accum, float accum_scale, void* stream);

/* The same product through a per-matrix PLAN (csrc/spmm.hip): rows shorter than `long_rows_from` entries are gathered
 * one wavefront per row with 16 bytes per lane; longer rows are cut into tasks of <= 256 entries inside one block of
 * 16 384 columns, run block by block on the workgroups that share an XCD's L2, and their partial rows are added in a
 * fixed order (no float atomics: results do not depend on timing).  Same epilogues as skr_csr_spmm.
 *   skr_spmm_plan_create  analyses the CSR once (device work, synchronises the stream twice); the plan keeps the three
 *                         CSR pointers -- the arrays must outlive it and keep their contents -- plus a task list and a
 *                         scratch buffer of its own.  Columns must ascend within a row and be < n_cols.
 *                         long_rows_from: 0 = default (512), otherwise >= 2.
 *   skr_spmm_plan_info    h_info4 = {long rows + (hot rows << 32), tasks, column blocks, long_rows_from + (column windows << 32)};
 *                         hot rows: the densest long rows (>= SKR_SPMM_HOT_DENSITY, default 4, entries per 128 columns on
 *                         average; at most 96) are not gathered at all in calls without d_col_mask -- X is streamed through
 *                         LDS in blocks of 128 rows and their entries, re-packed block-major at plan time, read it there
 *                         (SKR_SPMM_HOT=0: off)
 *                         SKR_SPMM_WINDOWS=n (default 1) makes the short-row kernel gather from X in n column windows, one
 *                         launch each (an experiment switch: no gain measured at X = 256 MB)
 *                         SKR_SPMM_HOT_DENSITY, SKR_SPMM_HOT_WGS, SKR_SPMM_CBLK and SKR_SPMM_WINDOWS are read when a plan is
 *                         created; the switches of a run (SKR_SPMM_HOT, _HOT_PF, _ROWS_WGS, _TASK_WGS, _TASK_SPAN) once per process
 * A plan may be run any number of times, by one stream at a time (the scratch buffer is shared between runs).
 * X must be finite in a run without d_col_mask and d_keep: short lists are padded with column 0 of the row or of the block
 * of X times 0, so a NaN or Inf there would reach rows that do not name that column. */
typedef struct skr_spmm_plan skr_spmm_plan;
int skr_spmm_plan_create(int n_rows, int n_cols, const int64_t* d_rowptr, const int32_t* d_col, const float* d_val,
                         int64_t nnz, int long_rows_from, skr_spmm_plan** out, void* stream);
int skr_spmm_plan_run(const skr_spmm_plan* plan, const float* d_X, int dim, const float* d_addend, float* d_Y,
                      float* d_accum, float accum_scale, void* stream);
/* The same product where parts of it are known not to be needed (LightGCN's step: only the batch's rows of the LAST
 * forward layer are read, and the gradient that enters the FIRST backward hop is zero outside the batch's rows):
 *   d_row_mask  uint8[n_rows] or NULL: rows with a 0 byte are skipped entirely (their Y / accum rows are left as they are)
 *   d_col_mask  uint8[n_cols] or NULL: entries whose column has a 0 byte are skipped, and the rows of X of those columns are
 *               not read (they may hold anything, NaN included): the result is the product of the marked entries -- the
 *               full product's, up to the sign of a zero, where those rows of X are zero
 * skr_mark_ids sets d_mask[offset + ids[k]] = 1 (negative ids skipped); clear the mask first. */
int skr_spmm_plan_run_masked(const skr_spmm_plan* plan, const float* d_X, int dim, const float* d_addend, float* d_Y,
                             float* d_accum, float accum_scale, const uint8_t* d_row_mask, const uint8_t* d_col_mask,
                             void* stream);
int skr_mark_ids(const int32_t* d_ids, int64_t n, int64_t offset, uint8_t* d_mask, void* stream);
/* The product with the TRANSPOSE of a CSR matrix A [n_rows, *] where X [n_rows, 64] is zero outside the rows marked in
 * d_row_mask:  Y[c] += A[r, c] * X[r]  for every entry of every marked row (Y initialised by the caller: zeros, or the
 * addend).  The item side of LightGCN's FIRST backward hop is this: dL/dE-bar is zero outside the batch's <= batch users, so
 * instead of every item row scanning its users for marked ones (48 M entries looked at) the batch users' own rows -- the
 * user-side block, whose entries are the same non-zeros -- are walked (~50 k entries) with one 256-byte row atomic each.
 * Float atomics: the order of the additions into a row varies from run to run, as it does in skr_bpr_step's scatter. */
int skr_csr_scatter_marked_rows(int n_rows, const int64_t* d_rowptr, const int32_t* d_col, const float* d_val,
                                const uint8_t* d_row_mask, const float* d_X, int dim, float* d_Y, void* stream);
/* The general form: what happens to a finished row y = (A X)_r (+ addend_r) is described by a skr_spmm_epilogue, so that the
 * row-local passes around a propagation ride in the product's row epilogue instead of being launches of their own (a
 * wavefront holds the whole 64-float row there):
 *   SKR_EPI_PLAIN       Y_r = y (Y may be NULL when only accum is wanted); accum_r = accum_r + accum_scale * y, or, with
 *                       accum_base, accum_r = accum_scale * accum_base_r + accum_scale * y (LightGCN's layer mean including
 *                       its E0 term: LightGCN.py:89-100), or, with accum_init, accum_r = accum_scale * y (accum is not read);
 *   SKR_EPI_REFINE_FWD  LayerGCN.py:214-216 on the finished row: w_r = cos(y, E_r) (torch eps 1e-8) -> w[r]; Z_r = w_r * y;
 *                       Y_r = y (the raw row the backward needs; Y may be NULL for inference); accum_r += Z_r (accum_init:
 *                       accum_r = Z_r);
 *   SKR_EPI_REFINE_BWD  the finished row is dZ of the layer below (hop k+1 of the backward feeds layer k's refinement):
 *                       Y_r = dY_r = the backward of that refinement at (rawY_r, E_r, w[r]); dE_r += its E0 part
 *                       (skr_layer_refine_bwd's arithmetic).
 * Rows skipped by d_row_mask get no epilogue. */
enum { SKR_EPI_PLAIN = 0, SKR_EPI_REFINE_FWD = 1, SKR_EPI_REFINE_BWD = 2 };
typedef struct skr_spmm_epilogue {
    int32_t mode;
    int32_t accum_init;
    const float* addend;
    float* Y;
    float* accum;
    const float* accum_base;
    float accum_scale;
    int32_t ld;                   /* row stride, in floats, of X and of every dense operand named here; 0 = 64.  With ld = 64 C
                                     and the pointers advanced by 64 c the call multiplies the c-th 64-column slice of [n, 64 C]
                                     tables (embedding widths beyond 64: the product is separable in the columns);
                                     SKR_EPI_PLAIN only */
    const float* E;
    float* w;
    float* Z;
    const float* rawY;
    float* dE;
    const uint8_t* accum_mask;    /* uint8[n_rows] or NULL: accum_r is only updated where the byte is set (a training step reads
                                     the layer mean / sum at its batch's rows only) */
    const uint8_t* addend_mask;   /* uint8[n_rows] or NULL: addend_r IS zero where the byte is 0 and is not read there (dL/d output
                                     is zero outside the batch's rows) */
} skr_spmm_epilogue;
int skr_spmm_plan_run_ex(const skr_spmm_plan* plan, const float* d_X, int dim, const skr_spmm_epilogue* epi,
                         const uint8_t* d_row_mask, const uint8_t* d_col_mask, void* stream);
/* The product with per-ENTRY dropout (edge dropout drawn anew for every step, no new plan):
 *   A'[e] = d_keep[e] ? val[e] * scale : 0     (one fp32 multiply; the reference's v[mask] * (1. / (1 - rate)),
 *                                                recommender/SelfCF.py:133-144, with scale = float32(1 / (1 - rate)))
 * d_keep: uint8 [nnz] in the plan's CSR entry order.  A dropped entry is SKIPPED: its row of X is not read (where every entry
 * of a column is dropped, that row of X may hold anything, NaN included).  Same row / task / reduce structure and the same
 * fixed order of additions as skr_spmm_plan_run_ex; the plan's densest rows go through the task path (their block-major
 * copies hold no flags).  No float atomic: repeated runs are bit-identical.  SKR_EPI_PLAIN only (any other mode: SKR_EINVAL);
 * a row whose entries are all dropped still gets its epilogue (y = addend_r or 0). */
int skr_spmm_plan_run_dropped(const skr_spmm_plan* plan, const float* d_X, int dim, const skr_spmm_epilogue* epi,
                              const uint8_t* d_keep, float scale, void* stream);
int skr_spmm_plan_info(const skr_spmm_plan* plan, int64_t* h_info4);
int skr_spmm_plan_destroy(skr_spmm_plan* plan);

/* LayerGCN layer refinement (LayerGCN.py:214-216): w_r = cos(Y_r, E_r) (torch eps 1e-8),
 * Z_r = w_r * Y_r; d_accum += Z (may be NULL); d_w[n_rows] keeps w for the backward. */
int skr_layer_refine_fwd(const float* d_Y, const float* d_E, int64_t n_rows, int dim,
                         float* d_Z, float* d_w, float* d_accum, void* stream);
/* Backward of the above: given dZ -> dY (written) and dE (accumulated). */
int skr_layer_refine_bwd(const float* d_Y, const float* d_E, const float* d_w, const float* d_dZ,
                         int64_t n_rows, int dim, float* d_dY, float* d_dE, void* stream);

/* The same restricted to the rows whose byte in d_row_mask (uint8[n_rows], NULL = all) is set: where dZ_r is known to be
 * zero (LayerGCN's first backward refinement: dL/d out is zero outside the batch's rows) dY_r = 0 and dE_r gets nothing, so
 * the row is skipped.  zero_skipped != 0: dY_r = 0 is written for the skipped rows; 0: dY_r is left as it is (the product
 * that follows must then skip those columns: d_col_mask). */
int skr_layer_refine_bwd_masked(const float* d_Y, const float* d_E, const float* d_w, const float* d_dZ, int64_t n_rows,
                                int dim, float* d_dY, float* d_dE, const uint8_t* d_row_mask, int zero_skipped, void* stream);
/* Rows of d_table [n_rows, dim] whose byte in d_mask is set are zeroed; with clear_mask != 0 the bytes are cleared too.
 * Restores the all-zero state of a gradient buffer of which only one batch's rows were written (instead of a fill of
 * the whole buffer; no reference counterpart: autograd allocates a fresh zero tensor per step). */
int skr_clear_marked_rows(uint8_t* d_mask, int64_t n_rows, int64_t clear_mask, float* d_table, int dim, void* stream);

/* Row gather out[k] = table[idx[k]] (F.embedding; any row width `dim`, 64 has its own kernel) and  y = a*x + y  helpers
 * used by the host mirror so that no torch kernel sits on the hot path. */
int skr_gather_rows(const float* d_table, const int32_t* d_idx, int64_t n, int dim, float* d_out, void* stream);
/* table[idx[k]] = src[k] (negative ids skipped; rows of duplicate ids must be identical): with skr_gather_rows, the
 * compact form in which the user-sharded engines exchange the FEW rows of a replicated block a step touches */
int skr_scatter_rows(const float* d_src, const int32_t* d_idx, int64_t n, int dim, float* d_table, void* stream);
/* d_out[i] = ((d_in[0][i] + d_in[1][i]) + d_in[2][i]) + ... over n_blocks blocks of n floats: the ranks' all-gathered
 * blocks added in rank order, so that every replica ends with the same bits whatever the collective library does */
int skr_sum_blocks(const float* d_in, int n_blocks, int64_t n, float* d_out, void* stream);
int skr_axpy(float a, const float* d_x, float* d_y, int64_t n, void* stream);
int skr_scale_copy(float a, const float* d_x, float* d_y, int64_t n, void* stream);    /* y = a * x */
int skr_scale(float a, float* d_x, int64_t n, void* stream);                 /* x *= a */

/* ---------------------------------------------------------------------------------------------
 * Epoch shuffle + batch assembly.  replaces: BatchIterator's per-element Python batching
 * (utils/py/batch_iterator.py:48-66,132-155: idx = np.random.permutation(n); [data[i] for i in idx] per column) and
 * the zip of the users / pos / neg columns (io/data_iterator.py:226-234).
 * ONE launch per epoch: for r < n_out, row r of every output column = row src(r) of its input column, with
 *   src(r) = d_perm[r]     when d_perm != NULL (int32[>= n_out], values in [0, n_src): the numpy-compatible contract --
 *                          the values of the epoch's np.random.permutation(n), e.g. from skr_host_permutation), or
 *   src(r) = pi_seed(r)    when d_perm == NULL: a keyed bijection of [0, n_src) evaluated in registers (no permutation
 *                          array, no sort; equal to the reference's shuffle in law only).
 * d_cols / d_outs: HOST arrays of n_cols (1..4) DEVICE pointers; widths[k] = 32-bit words per row of column k (1 for an
 * id or label column, num_neg for a [n, num_neg] block).  Input and output must not alias.  n_out <= n_src < 2^31. */
int skr_shuffle_gather(const int32_t* d_perm, uint64_t seed, int64_t n_src, int64_t n_out, int n_cols,
                       const void* const* d_cols, const int* widths, void* const* d_outs, void* stream);
/* pi_seed(0 .. n_out-1) itself (int32), on the device / on the host (the host form needs no GPU) */
int skr_shuffle_permutation(uint64_t seed, int64_t n, int64_t n_out, int32_t* d_out, void* stream);
int skr_shuffle_permutation_host(uint64_t seed, int64_t n, int64_t n_out, int32_t* h_out);

/* HOST function (no GPU): np.random.permutation(n) of numpy's legacy global generator, restated natively.  The
 * reference shuffles each epoch with it (skrec/io/batch_iterator.py:61-63).  key624 / pos: the generator's MT19937 state
 * as np.random.get_state() returns it (uint32[624], position 0..624); both are advanced exactly as numpy advances
 * them, so np.random.set_state() with the returned values leaves the generator where the reference's would be.
 * h_out int32[n], n < 2^31.  Runs outside the GIL when called through ctypes. */
int skr_host_permutation(uint32_t* h_key624, int* h_pos, int64_t n, int32_t* h_out);

/* The same dense Adam, temporally blocked over k consecutive steps whose batches are known in advance (an epoch's
 * batches are: data_iterator.py:230-234).  64-float blocks of the flat buffer that none of the k steps touches get
 * their k zero-gradient updates in ONE pass; touched blocks get the ordinary update at every step.  Every
 * parameter receives every update in the arithmetic of skr_adam_step: the results are bit-identical.
 *   skr_adam_block_mark   d_tag[(offset + id*stride) >> 6] = tag_value and d_claim[same] = step_t0 for every id (call
 *                         once per id list: user rows offset 0 stride 64, item rows offset U*64, bias offset
 *                         (U+I)*64 stride 1).  step_t0 = optimiser steps taken before the k-step block.
 *   skr_adam_block_cold   steps step_t0+1 .. step_t0+k with zero gradient on every block whose tag != hot_value
 *   skr_adam_block_hot    ADVANCES the blocks the ids name to step_t (step_t0 < step_t <= step_t0 + 64): a block that
 *                         d_claim says is at step c gets zero-gradient updates for steps c+1 .. step_t-1 and then
 *                         step_t's update with its accumulated gradient, which is read and cleared; d_claim becomes
 *                         step_t (duplicate ids: one wavefront wins).  Either name every hot block at every step, or
 *                         at step t only the rows of batch t and of batch t+1 (which must read current rows) and
 *                         every hot block at the LAST step of the k-step block -- all hot blocks must end at
 *                         step_t0 + k.  Both orders of visiting apply the same updates in the same order.
 *   d_tag, d_claim        int32[ceil(n / 64)], zero-initialised; use a fresh non-zero tag_value for every k-step block
 *   ids                   negative entries are skipped by _mark and _hot (empty slots of a de-duplicated list) */
int skr_adam_block_mark(const int32_t* d_ids, int64_t n_ids, int64_t offset_floats, int stride_floats, int32_t* d_tag,
                        int32_t tag_value, int32_t* d_claim, int64_t step_t0, void* stream);
int skr_adam_block_cold(float* d_p, float* d_m, float* d_v, int64_t n, float lr, float beta1, float beta2, float eps,
                        int64_t step_t0, int k, const int32_t* d_tag, int32_t hot_value, void* stream);
int skr_adam_block_hot(float* d_p, float* d_g, float* d_m, float* d_v, int64_t n, float lr, float beta1, float beta2,
                       float eps, int64_t step_t0, int64_t step_t, const int32_t* d_ids, int64_t n_ids, int64_t offset_floats,
                       int stride_floats, int32_t* d_claim, void* stream);
/* skr_adam_block_cold with a state word per row that carries what one pass established into the next (torch's plain
 * arithmetic only; results are those of skr_adam_block_cold, bit for bit).
 *   d_rest    int32[(n + 63) / 64], zero-initialised by the caller and from then on written by these calls only.  A cold
 *             row's word is (pass_id << 2) | state, written for EVERY cold row of EVERY pass; rows tagged hot are skipped,
 *             so their words go stale by themselves: nothing ever clears a word.
 *   pass_id   1 <= pass_id < 2^29.  A row's recorded state is trusted only if its word carries pass_id - 1.
 *             pass_id = previous + 1 is the caller's PROMISE that, since the previous call on these buffers, (a) the rows
 *             that call left cold have received nothing but zero-gradient Adam updates (in effect: nothing wrote them),
 *             (b) lr, beta1, beta2 and eps are that call's, and (c) step_t0 is that call's step_t0 + k.  Any other
 *             pass_id (use previous + 2) means "trust nothing": every row is examined from scratch.
 *   states    0 unknown: handled as by skr_adam_block_cold.
 *             1 quiet: when p was last read, every lane had v >= +0 and not NaN, |p| >= 2^-60 and
 *               |nss * m| < 2^-28 * |p| * eps; under the promise that stays true (|m| and torch's |nss| only fall), so the
 *               row is at rest again: only m and v are loaded, decayed and stored.
 *             2 zero: additionally (or with eps > 0 and no NaN in p) every lane of m and v is +0: nothing is loaded.
 *             No state is set with eps == 0 or with lr / betas outside the at-rest test's range; the tail block
 *             (n % 64 != 0) has no word.
 * With SKR_COLD_STATS=1, skr_cold_rest_census returns h_counts2 = {rows trusted as quiet, rows trusted as zero} (they are
 * also counted as "at rest" by skr_cold_pass_census); either census function's reset clears both.  The variable is read
 * at the first cold pass and again at every call of skr_cold_rest_census, so a process can switch the census on and off
 * between passes.  Synchronises the device.  (Measurement hook.) */
int skr_adam_block_cold_rest(float* d_p, float* d_m, float* d_v, int64_t n, float lr, float beta1, float beta2, float eps,
                             int64_t step_t0, int k, const int32_t* d_tag, int32_t hot_value, int32_t* d_rest, int32_t pass_id,
                             void* stream);
int skr_cold_rest_census(uint64_t* h_counts2, int reset);
/* The same three entry points with tf.train.AdamOptimizer's arithmetic (GRU4RecPlus.py:192): p -= lr_t * m / (sqrt(v) + eps)
 * with lr_t = lr * sqrt(1 - beta2^t) / (1 - beta1^t) -- the second bias correction sits in the step size, eps is added to
 * the raw sqrt(v).  |lr_t| falls and then rises again with t, so the at-rest test of a run of zero-gradient updates uses
 * the largest |lr_t| of the run.  Blocked == one skr_adam_step_tf per step, bit for bit. */
int skr_adam_step_tf(float* d_p, float* d_g, float* d_m, float* d_v, int64_t n, float lr, float beta1, float beta2, float eps,
                     int64_t step_t, int zero_grad, uint8_t* d_touch, void* stream);
int skr_adam_block_cold_tf(float* d_p, float* d_m, float* d_v, int64_t n, float lr, float beta1, float beta2, float eps,
                           int64_t step_t0, int k, const int32_t* d_tag, int32_t hot_value, void* stream);
int skr_adam_block_hot_tf(float* d_p, float* d_g, float* d_m, float* d_v, int64_t n, float lr, float beta1, float beta2,
                          float eps, int64_t step_t0, int64_t step_t, const int32_t* d_ids, int64_t n_ids,
                          int64_t offset_floats, int stride_floats, int32_t* d_claim, void* stream);

/* The same three entry points with torch.optim.Adam(weight_decay=...)'s arithmetic (HGN.py:182): every element's gradient
 * becomes g' = fmaf(weight_decay, p, g) -- ONE rounding, as torch's grad.add(param, alpha=weight_decay) -- with the p the
 * step starts from, then the update of skr_adam_step.  A block without a gradient is therefore not at rest: the cold pass
 * runs its k updates, each with g' = weight_decay * p of the current p, back to back in registers, and so do the hot
 * step's catch-up updates; only elements whose p, m and v are all +0 (padded columns, padding rows) are left alone,
 * which is what the arithmetic gives for them (eps > 0).  Blocked == one skr_adam_step_wd per step, bit for bit. */
int skr_adam_step_wd(float* d_p, float* d_g, float* d_m, float* d_v, int64_t n, float lr, float beta1, float beta2, float eps,
                     float weight_decay, int64_t step_t, int zero_grad, uint8_t* d_touch, void* stream);
int skr_adam_block_cold_wd(float* d_p, float* d_m, float* d_v, int64_t n, float lr, float beta1, float beta2, float eps,
                           float weight_decay, int64_t step_t0, int k, const int32_t* d_tag, int32_t hot_value, void* stream);
int skr_adam_block_hot_wd(float* d_p, float* d_g, float* d_m, float* d_v, int64_t n, float lr, float beta1, float beta2,
                          float eps, float weight_decay, int64_t step_t0, int64_t step_t, const int32_t* d_ids, int64_t n_ids,
                          int64_t offset_floats, int stride_floats, int32_t* d_claim, void* stream);

/* One training step of BPRMF in ONE launch: skr_bpr_step (score rows == regulariser rows, loss_scale 1) and the hot rows'
 * part of the blocked dense Adam together, for a k-step block whose batches are known (replaces, per step, the pair
 * skr_bpr_step_spread + skr_adam_block_hot; BPRMF.py:108-127).  Hot rows are evaluated lazily: the wavefronts that read a
 * row first apply, in registers, the updates the row is behind (its pending gradient of the previous naming, then
 * zero-gradient updates -- the arithmetic of skr_adam_step, bit for bit), and a step's gradient waits in the block's
 * workspace until the row is named again or the block ends.  Per reference (step, row) the caller supplies one word
 *   d_meta[r * n_batch + b], r = 0..4: user row, positive item row, negative item row, the 64-word bias block of the
 *   positive item, of the negative item;   bits 0-19 slot of the row in the block's workspace (dense numbering 0 .. n_slots-1),
 *   bits 20-22 (number of EARLIER steps of the block that name the row) mod 6, bit 23 set on exactly one reference per
 *   (step, row), bits 24-30 1 + the step of the previous naming (0: none), bit 31 set when the reference is the only one
 *   of its (step, row) pair (its gradient is then stored, not added atomically)
 * -- skr_bpr_fused_plan writes them, and the slot tables of skr_bpr_fused_end, for the k batches of a block (d_u / d_i / d_j:
 * k * n_batch entries, step-major) in four small launches:  d_scratch = 28 * n_flat_blocks bytes, 8-byte aligned, ZERO before
 * the first call and left usable by every call (n_flat_blocks = ceil(n / 64));  d_meta int32[k * 5 * n_batch];
 * d_slot_block / d_slot_fin int32[k * 5 * n_batch] (d_slot_block: -1 beyond n_slots -- a valid id list for
 * skr_adam_block_mark);  d_n_slots int32[1].  Which slot a row gets may differ between calls; nothing depends on it.
 *   d_work   float[9 * cap * 64], ZERO before the first block and left as skr_bpr_fused_end leaves it; cap >= n_slots
 *   *_block0 index (in 64-float blocks of the flat buffer d_p) of user row 0, item row 0, bias word 0
 *   s        the step inside the block (0 .. k-1); the k launches of a block are followed by ONE skr_bpr_fused_end, which
 *            brings every slot (d_slot_block[slot] = its block of the flat buffer, d_slot_fin[slot] = (number of namings
 *            mod 6) | (step of the last naming << 8), *d_n_slots on the device) to step step_t0 + k and writes it back.
 * The cold blocks of the k-step block are skr_adam_block_cold's as before (tags from skr_adam_block_mark).
 * d_loss64: as skr_bpr_step_spread.  1 <= k <= 64. */
int skr_bpr_fused_plan(const int32_t* d_u, const int32_t* d_i, const int32_t* d_j, int n_batch, int k, int64_t user_block0,
                       int64_t item_block0, int64_t bias_block0, int64_t n_flat_blocks, void* d_scratch, int32_t* d_meta,
                       int32_t* d_slot_block, int32_t* d_slot_fin, int32_t* d_n_slots, void* stream);
int skr_bpr_fused_step(const float* d_p, const float* d_m, const float* d_v, int64_t n, float* d_work, int64_t cap,
                       const int32_t* d_u, const int32_t* d_i, const int32_t* d_j, const int32_t* d_meta, int n_batch,
                       int64_t user_block0, int64_t item_block0, int64_t bias_block0, float lr, float beta1, float beta2,
                       float eps, int64_t step_t0, int k, int s, float reg, float* d_loss64, void* stream);
/* skr_bpr_fused_end, `which`: 0 every slot; with the NEXT block's tags (d_tag_next[flat block] == tag_next_value: the next block
 * touches the row too -- skr_adam_block_mark of its slot table) 1 = only those rows, which the next block must find in the
 * dense tables, 2 = only the others, which may be written back beside the next block's steps (another stream; they must be
 * back before the next block's cold pass, and the two blocks then need workspaces of their own). */
int skr_bpr_fused_end(float* d_p, float* d_m, float* d_v, int64_t n, float* d_work, int64_t cap, const int32_t* d_slot_block,
                      const int32_t* d_slot_fin, const int32_t* d_n_slots, float lr, float beta1, float beta2, float eps,
                      int64_t step_t0, int k, const int32_t* d_tag_next, int32_t tag_next_value, int which, void* stream);
/* The k skr_bpr_fused_step launches of a block (batch s at d_u / d_i / d_j + s * n_batch, its words at d_meta + 5 * s * n_batch, its
 * loss sums at d_loss64 + s * loss_stride_floats) followed by skr_bpr_fused_end (which = 1 when d_tag_next is given, else 0), in one call: the host side of a step is then a
 * loop in C, not 24-argument calls from the caller's language. */
int skr_bpr_fused_block(float* d_p, float* d_m, float* d_v, int64_t n, float* d_work, int64_t cap, const int32_t* d_u,
                        const int32_t* d_i, const int32_t* d_j, const int32_t* d_meta, int n_batch, int64_t user_block0,
                        int64_t item_block0, int64_t bias_block0, float lr, float beta1, float beta2, float eps, int64_t step_t0,
                        int k, float reg, float* d_loss64, int64_t loss_stride_floats, const int32_t* d_slot_block,
                        const int32_t* d_slot_fin, const int32_t* d_n_slots, const int32_t* d_tag_next, int32_t tag_next_value,
                        void* stream);
/* The first naming of a row in a block costs the step launch the zero-gradient updates from the block's start to that step
 * (16 on average at k = 32) -- on the critical path.  For the rows that were COLD in the block before (nearly every user
 * row) these updates depend on nothing the block itself does, so they are made ahead of time, beside the previous block:
 *   skr_bpr_fused_plan2   as skr_bpr_fused_plan; with d_tag_prev / tag_prev_value = the hot-block tags of the PREVIOUS block
 *                         (skr_adam_block_mark) a first naming at a step > 0 of a row that block did not touch gets the
 *                         value 7 in its word's n0 field: "the state waits in the pre buffer"
 *   skr_bpr_fused_pre     fills d_pre (float [3][cap][64]: p, m, v by slot) for those rows from the dense tables, which
 *                         must hold the state the block starts from for them (i.e. behind the previous block's cold
 *                         pass; it never reads a row the previous block named).  step_t0 / k: the block's own.
 *   skr_bpr_fused_step2 / _block2   as _step / _block, reading d_pre where a word says so (NULL if no word does).
 * The same updates in the same arithmetic (the call the step launch would have made): bit-identical results. */
int skr_bpr_fused_plan2(const int32_t* d_u, const int32_t* d_i, const int32_t* d_j, int n_batch, int k, int64_t user_block0,
                        int64_t item_block0, int64_t bias_block0, int64_t n_flat_blocks, void* d_scratch, int32_t* d_meta,
                        int32_t* d_slot_block, int32_t* d_slot_fin, int32_t* d_n_slots, const int32_t* d_tag_prev,
                        int32_t tag_prev_value, void* stream);
int skr_bpr_fused_pre(const float* d_p, const float* d_m, const float* d_v, int64_t n, float* d_pre, int64_t cap,
                      const int32_t* d_slot_block, const int32_t* d_slot_fin, const int32_t* d_n_slots, float lr, float beta1,
                      float beta2, float eps, int64_t step_t0, int k, const int32_t* d_tag_prev, int32_t tag_prev_value,
                      void* stream);
int skr_bpr_fused_step2(const float* d_p, const float* d_m, const float* d_v, int64_t n, float* d_work, int64_t cap,
                        const int32_t* d_u, const int32_t* d_i, const int32_t* d_j, const int32_t* d_meta, int n_batch,
                        int64_t user_block0, int64_t item_block0, int64_t bias_block0, float lr, float beta1, float beta2,
                        float eps, int64_t step_t0, int k, int s, float reg, float* d_loss64, const float* d_pre, void* stream);
int skr_bpr_fused_block2(float* d_p, float* d_m, float* d_v, int64_t n, float* d_work, int64_t cap, const int32_t* d_u,
                         const int32_t* d_i, const int32_t* d_j, const int32_t* d_meta, int n_batch, int64_t user_block0,
                         int64_t item_block0, int64_t bias_block0, float lr, float beta1, float beta2, float eps,
                         int64_t step_t0, int k, float reg, float* d_loss64, int64_t loss_stride_floats,
                         const int32_t* d_slot_block, const int32_t* d_slot_fin, const int32_t* d_n_slots,
                         const int32_t* d_tag_next, int32_t tag_next_value, const float* d_pre, void* stream);
/* The loss words off the step's path.  Nothing reads a step's loss words before its block has ended, so the step launch
 * need not add them to d_loss64 itself (512 float atomics on 256 bytes at n_batch = 1 024):
 *   skr_bpr_fused_step3   as _step2, but every launched wavefront stores its two sums, with one plain 8-byte store, into
 *                         row s of d_loss_part (exact zeros where the wavefront had no interaction); d_loss64 is not
 *                         touched.  d_loss_part: float[skr_bpr_fused_loss_part_floats(n_batch, k)], 8-byte aligned, of any
 *                         content: every pair _end3 reads was written by the block's own launches.  One buffer serves
 *                         all blocks of a stream.
 *   skr_bpr_fused_end3    as _end; with which 0 / 1 the launch also folds the k rows of d_loss_part into the block's loss
 *                         words: d_loss64[s * loss_stride_floats + 2 * q + c] += the sum over the workgroups q,
 *                         q + SKR_LOSS_SLOTS, ... (ascending) of ((w0 + w1) + w2) + w3, the workgroup's four wavefronts --
 *                         _step2's sums, in a FIXED order: two runs give the same bits.  It adds to what is there (one
 *                         atomic per word and step: a stride of 0 sums the steps); a pair no workgroup feeds receives
 *                         +0.0f.  which = 2 folds nothing.  n_batch: the step launches'.
 *   skr_bpr_fused_block3  as _block2 through _step3 / _end3: the same k + 1 launches.
 *   skr_bpr_fused_loss_part_floats   k * 8 * min(ceil(n_batch / 4), 4 096) (one pair per wavefront of a step launch's grid;
 *                         256 KB at k = 32, n_batch = 1 024); 0 for an empty batch.
 * Parameters and moments: _step2's bits. */
int64_t skr_bpr_fused_loss_part_floats(int n_batch, int k);
int skr_bpr_fused_step3(const float* d_p, const float* d_m, const float* d_v, int64_t n, float* d_work, int64_t cap,
                        const int32_t* d_u, const int32_t* d_i, const int32_t* d_j, const int32_t* d_meta, int n_batch,
                        int64_t user_block0, int64_t item_block0, int64_t bias_block0, float lr, float beta1, float beta2,
                        float eps, int64_t step_t0, int k, int s, float reg, float* d_loss64, const float* d_pre,
                        float* d_loss_part, void* stream);
int skr_bpr_fused_end3(float* d_p, float* d_m, float* d_v, int64_t n, float* d_work, int64_t cap, const int32_t* d_slot_block,
                       const int32_t* d_slot_fin, const int32_t* d_n_slots, float lr, float beta1, float beta2, float eps,
                       int64_t step_t0, int k, const int32_t* d_tag_next, int32_t tag_next_value, int which,
                       const float* d_loss_part, float* d_loss64, int64_t loss_stride_floats, int n_batch, void* stream);
int skr_bpr_fused_block3(float* d_p, float* d_m, float* d_v, int64_t n, float* d_work, int64_t cap, const int32_t* d_u,
                         const int32_t* d_i, const int32_t* d_j, const int32_t* d_meta, int n_batch, int64_t user_block0,
                         int64_t item_block0, int64_t bias_block0, float lr, float beta1, float beta2, float eps,
                         int64_t step_t0, int k, float reg, float* d_loss64, int64_t loss_stride_floats,
                         const int32_t* d_slot_block, const int32_t* d_slot_fin, const int32_t* d_n_slots,
                         const int32_t* d_tag_next, int32_t tag_next_value, const float* d_pre, float* d_loss_part,
                         void* stream);

/* The cold pass sorts each 64-float block, by the values it starts from, into one of three exact evaluations of
 * the same k updates: AT REST (the update provably rounds to p + q == p for all k steps: only the moments decay),
 * ORDINARY MAGNITUDES (square root and divisions without the scaling / fix-up steps that cannot act there), or the
 * general form.  skr_selftest_cold_math checks the second one's building blocks against the compiler's sqrtf and
 * division on the device.  h_mismatches (uint64[4], host): [0] differing results of the square root over EVERY float
 * in [2^-96, FLT_MAX], [1] of the division over n_pairs hashed (n, d) pairs of its range -- both must be 0;
 * [2] control: how often the raw v_sqrt_f32 differs from sqrtf over the same floats (> 0), [3] floats enumerated.
 * (Test hook; synchronises the stream.) */
int skr_selftest_cold_math(uint64_t n_pairs, uint64_t* h_mismatches, void* stream);
/* With SKR_COLD_STATS=1 in the environment the cold passes count their blocks by evaluation: h_counts3 = {at rest,
 * ordinary magnitudes, general} since the start / the last reset (all zero when the census is off).  Synchronises the
 * device.  (Measurement hook: tools/e2e_scale.py prints the shares of a real epoch.) */
int skr_cold_pass_census(uint64_t* h_counts3, int reset);

/* The lazily advanced rows of skr_bpr_fused_step / _pre / _end take a gradient update on the scaling-free
 * square root and divisions when, AFTER the moment update, every lane of the wavefront holds moments of ordinary magnitudes;
 * the zero-gradient run behind it then needs no test of its own.  With SKR_FUSED_STATS=1 in the environment the launches
 * count their evaluations: h_counts[8 * kernel + 4 * kind + class], kernel = {0 step launch: user / item rows, 1 step launch:
 * bias blocks, 2 end launch, 3 pre launch}, kind = {0 gradient update, 1 run of zero-gradient updates},
 * class = {0 at rest, 1 ordinary, 3 general}; then [32] / [33] slots the end launch advanced two to a wavefront / one by one
 * (a paired slot counts one gradient update and, where its partner was named later, one run up to that step under kernel 2;
 * the run the two rows make together is counted in [32] only).
 * n_counts <= 34 counters are copied (all zero when the census is off).  The
 * variable is read at the first launch and again at every call of this function.  Synchronises the device.
 * (Measurement hook.) */
#define SKR_FUSED_CENSUS_COUNTERS 34
int skr_fused_census(uint64_t* h_counts, int n_counts, int reset);
/* skr_selftest_grad_math: that gradient update against the dense kernel's arithmetic, bits of p, m and v, on n_tuples
 * hashed (p, g, m, v) tuples of the ordinary ranges in wavefronts of 64 at a hashed step of the block (step_t0, k; tf: TF's
 * scalars), followed by run_len - 1 zero-gradient updates (as far as the block goes) in the same call.  Of every 16 wavefronts two are CONTROLS with lanes outside the ordinary ranges.  h_counts5 (host): [0] tuples
 * tested, [1] mismatches (must be 0), [2] non-control wavefronts that took the scaling-free form (must be all of them),
 * [3] / [4] controls that took the general / the scaling-free form ([4] must be 0).  (Test hook; synchronises the stream.) */
int skr_selftest_grad_math(uint64_t n_tuples, float lr, float beta1, float beta2, float eps, int64_t step_t0, int k, int tf,
                           int run_len, uint64_t* h_counts5, void* stream);
/* skr_selftest_step_chain: the catch-up of skr_bpr_fused_step's kernel -- the block's per-step scalars held in lanes and read
 * with v_readlane_b32, the reciprocal of the second bias correction refined once per step (chain_advance, adam_math.h) --
 * against the forms skr_selftest_grad_math tests, bits of p, m and v, on the same hashed tuples and controls,
 * every wavefront at step s_from of the block: with_grad != 0: the gradient update s_from and the zero-gradient updates
 * behind it, otherwise zero-gradient updates alone, up to step s_from + run_len (as far as the block goes).  h_counts5 as
 * there: [2] counts the non-control wavefronts on the scaling-free form, [3] / [4] the controls on the general / the
 * scaling-free form.  (Test hook; synchronises the stream.) */
int skr_selftest_step_chain(uint64_t n_tuples, float lr, float beta1, float beta2, float eps, int64_t step_t0, int k, int s_from,
                            int run_len, int with_grad, uint64_t* h_counts5, void* stream);

/* Sparse exchange of a replicated table's gradient between ranks (no reference counterpart -- the
 * reference is single-process).  A BPR step touches at most 2*batch item rows, so instead of all-reducing the
 * dense [I, 65] block each rank packs its touched rows, the ranks all-gather the packs, and every rank adds
 * all packs to its dense gradient in rank order (replicas stay bit-identical).
 *   skr_pack_grad_rows:   d_ids int32[n], unique or negative (empty slot); d_out float32[n, dim+2] rows
 *                         [id bits | dV[id] | db[id]]; the packed dense rows are CLEARED.  d_g_bias may be NULL.
 *   skr_unpack_grad_rows: d_in float32[n_ranks, n_per_rank, dim+2]; dense += every valid row, rank 0 first. */
int skr_pack_grad_rows(const int32_t* d_ids, int n, float* d_g_table, float* d_g_bias, int dim, float* d_out, void* stream);
/* skr_unpack_grad_rows_sorted: the same sum, same order of additions, same bits, in ONE launch instead of n_ranks -- for
 * packs made from id lists whose valid ids ASCEND with the empty slots (-1) last (every rank's). */
int skr_unpack_grad_rows_sorted(const float* d_in, int n_per_rank, int n_ranks, float* d_g_table, float* d_g_bias, int dim,
                                uint8_t* d_touch, const float* d_touch_base, void* stream);
int skr_unpack_grad_rows(const float* d_in, int n_per_rank, int n_ranks, float* d_g_table, float* d_g_bias, int dim,
                         uint8_t* d_touch, const float* d_touch_base, void* stream);

/* ---------------------------------------------------------------------------------------------
 * G rows: GRU4RecPlus, recommender/GRU4RecPlus.py.  PARITY UNPINNED -- the reference runs this
 * model on TensorFlow 1.14, absent here; these entry points follow the graph of GRU4RecPlus.py:124-200 and
 * the published semantics of tf.nn.rnn_cell.GRUCell / tf.train.AdamOptimizer (oracle/gru4rec.py).
 * hid in {32, 64, 128}, in_dim <= 128.  hidden_act_kind: 0 tanh, 1 relu (:76-81).  final_act_kind:
 * 0 linear, 1 relu, 2 leaky_relu(0.2) (:84-91).  loss_kind: 0 bpr_max, 1 top1_max (:93-98).
 * ------------------------------------------------------------------------------------------- */

/* One GRUCell.call for B sessions (GRU4RecPlus.py:168-178):
 *   [r|u] = sigmoid([x,h] Wg + bg), c = act([x, r*h] Wc + bc), h' = u*h + (1-u)*c.
 *   d_x        float32 [B, in_dim], or -- when d_x_index != NULL -- an embedding table whose row
 *              d_x_index[b] is the input of session b (tf.nn.embedding_lookup fused in)
 *   d_active   uint8 [B] or NULL: 0 keeps h' = h (histories that already ended, _get_user_embeddings)
 *   d_Wg [in_dim+hid, 2*hid], d_bg [2*hid], d_Wc [in_dim+hid, hid], d_bc [hid]   (TF kernel layout)
 *   d_r, d_u, d_c  float32 [B, hid] saved for the backward pass, each may be NULL;  d_h_new [B, hid] */
int skr_gru_cell_fwd(const float* d_x, const int32_t* d_x_index, const float* d_h, const uint8_t* d_active, int B,
                     int in_dim, int hid, const float* d_Wg, const float* d_bg, const float* d_Wc, const float* d_bc,
                     int hidden_act_kind, float* d_r, float* d_u, float* d_c, float* d_h_new, void* stream);

/* Its backward for one step (the state enters through a placeholder, :127: no gradient into h).
 * Accumulates (+=) into d_gWg, d_gbg, d_gWc, d_gbc; writes dL/dx to d_dx [B, in_dim].
 * d_work: float32 scratch of 3*B*hid elements. */
int skr_gru_cell_bwd(const float* d_x, const int32_t* d_x_index, const float* d_h, int B, int in_dim, int hid,
                     const float* d_Wg, const float* d_Wc, int hidden_act_kind, const float* d_r, const float* d_u,
                     const float* d_c, const float* d_dh_new, float* d_gWg, float* d_gbg, float* d_gWc, float* d_gbc,
                     float* d_dx, float* d_work, void* stream);

/* skr_gru_cell_bwd of the FIRST layer (its input rows are gathered: d_x = the input item table, d_x_index = the batch's
 * items) followed by skr_scatter_add_rows(d_dx, d_x_index, B, in_dim, d_x, reg, d_g_table, ...): the input-embedding
 * gradient rides in the weight-gradient launch (both only need what the rows kernel in front of them has written). */
int skr_gru_cell_bwd_scatter(const float* d_x, const int32_t* d_x_index, const float* d_h, int B, int in_dim, int hid,
                             const float* d_Wg, const float* d_Wc, int hidden_act_kind, const float* d_r, const float* d_u,
                             const float* d_c, const float* d_dh_new, float* d_gWg, float* d_gbg, float* d_gWc, float* d_gbc,
                             float* d_dx, float* d_work, float reg, float* d_g_table, uint8_t* d_touch,
                             const float* d_touch_base, void* stream);

/* logits = final_act(out . E[Y]^T + bias[Y]) for B sessions against n_y targets (the batch's own next
 * items first: column b is session b's positive, :180-186), bpr_max / top1_max loss (:137-166) and its
 * gradient.  d_loss[0] = mean loss (the call clears the word first); d_dlogits [B, n_y] = dL/d(pre-activation logits);
 * d_dout [B, hid] = dL/d out.  B <= n_y <= 8192. */
int skr_session_loss(const float* d_out, int B, int hid, const float* d_item_table, const float* d_item_bias,
                     const int32_t* d_y, int n_y, int final_act_kind, int loss_kind, float bpr_reg, float* d_dlogits,
                     float* d_dout, float* d_loss, void* stream);

/* One rank's share of a SESSION-SHARDED step (BASELINE configs[4]): the B_local sessions of this call are the
 * slots slot_offset .. slot_offset + B_local - 1 of a batch of B_global sessions whose next items are the first B_global
 * entries of d_y on every rank (row r's positive is column slot_offset + r); the loss is the mean over B_global. */
int skr_session_loss_sharded(const float* d_out, int B_local, int hid, const float* d_item_table, const float* d_item_bias,
                             const int32_t* d_y, int n_y, int final_act_kind, int loss_kind, float bpr_reg, float* d_dlogits,
                             float* d_dout, float* d_loss, int slot_offset, int B_global, void* stream);

/* skr_session_loss_sharded followed by skr_session_out_grads (arguments as there; slot_offset = 0 and B_global = B_local for
 * a whole batch) with dL/dout and the output-side gradients in ONE launch: three launches per call instead of four. */
int skr_session_loss_grads(const float* d_out, int B_local, int hid, const float* d_item_table, const float* d_item_bias,
                           const int32_t* d_y, int n_y, int final_act_kind, int loss_kind, float bpr_reg, float* d_dlogits,
                           float* d_dout, float* d_loss, int slot_offset, int B_global, float reg, float* d_g_table,
                           float* d_g_bias, uint8_t* d_touch, const float* d_touch_base, void* stream);

/* Output-side gradients of the same step, accumulated into dense gradient tables:
 *   d_g_table[Y[y]] += sum_b dlogits[b,y] out[b] + reg * E[Y[y]],  d_g_bias[Y[y]] += sum_b dlogits[b,y] + reg * bias[Y[y]]
 * (reg: the l2_loss term of :189-191; repeated targets count each time).  d_touch / d_touch_base as in skr_bpr_step. */
int skr_session_out_grads(const float* d_dlogits, const float* d_out, int B, int hid, const int32_t* d_y, int n_y,
                          const float* d_item_table, const float* d_item_bias, float reg, float* d_g_table,
                          float* d_g_bias, uint8_t* d_touch, const float* d_touch_base, void* stream);

/* The popularity^alpha negatives of the session-parallel loop (`_sample_neg_items`, GRU4RecPlus.py:198-200:
 * np.searchsorted(pop_cumsum, np.random.rand(size))) on the device: d_out[k] = first index with d_cumsum[idx] >= u_k.
 * d_uniform float64[n]: the uniforms drawn on the host from numpy's global generator (the reference's stream), or NULL:
 * a counter-keyed device generator (seed, k) -- equal to the reference in law only.  d_cumsum float64[n_items], ascending. */
int skr_pop_sample(const double* d_cumsum, int n_items, const double* d_uniform, uint64_t seed, int64_t n, int32_t* d_out,
                   void* stream);

/* d_g_table[index[n]] += src[n] + reg * table[index[n]]: gradient of an embedding lookup (+ l2_loss of the looked-up rows) */
int skr_scatter_add_rows(const float* d_src, const int32_t* d_index, int n, int dim, const float* d_table, float reg,
                         float* d_g_table, uint8_t* d_touch, const float* d_touch_base, void* stream);

/* ============================================================================================
 * Q -- sequential pairwise recommenders: FPMC and TransRec (csrc/seq.hip)
 * replaces: _FPMC.forward / predict and FPMC.fit's step (recommender/FPMC.py:71-86,118-128),
 *           _TransRec.forward / predict and TransRec.fit's step (recommender/TransRec.py:75-93,125-135),
 *           inner_product / l2_distance / bpr_loss / l2_loss (utils/torch.py:20-29,62-74).
 * Rows are `dim` floats (64, 128, 192 or 256: narrower embeddings zero-padded by the caller, as for skr_bpr_step_dim).
 * A triple (u, l = last item, p = positive, n = negative) with an id outside [0, n_users) / [0, n_items) is skipped.
 * d_loss: float[2 * loss_slots], loss_slots 1 or SKR_LOSS_SLOTS, as skr_bpr_step_dim: the batch's
 * sum of -logsigmoid(y_p - y_n) and its un-normalised l2 (0.5 * sum of squares of the gathered rows; a repeated id
 * counts once per occurrence) are ADDED to the pairs, spread over the workgroups.
 * ========================================================================================== */
/* FPMC: y_i = <UI[u], IU[i]> + <LI[l], IL[i]> (the two inner products reduced separately, then added).  With
 * c = -sigmoid(-(y_p - y_n)) the gradients are scatter-added (atomically) into the four gradient tables:
 *   gUI[u] += c (IU[p] - IU[n]) + reg UI[u];   gLI[l] += c (IL[p] - IL[n]) + reg LI[l];
 *   gIU[p|n] += +-c UI[u] + reg IU[p|n];       gIL[p|n] += +-c LI[l] + reg IL[p|n].
 * l2 rows: UI[u], LI[l], IU[p], IU[n], IL[p], IL[n]. */
int skr_fpmc_step(const float* d_UI, const float* d_IU, const float* d_IL, const float* d_LI, const int32_t* d_u,
                  const int32_t* d_l, const int32_t* d_p, const int32_t* d_n, int n, int n_users, int n_items, int dim,
                  float reg, float* d_gUI, float* d_gIU, float* d_gIL, float* d_gLI, float* d_loss, int loss_slots,
                  void* stream);
/* TransRec: t = (U[u] + T) + V[l], y_i = -||t - V[i]||_2 + b[i]; T is the one global transition row (d_T: dim floats).
 * dy_i/dt = -(t - V[i]) / ||t - V[i]|| (0 at distance 0, torch's norm subgradient); dL/dt goes to U[u], V[l] and T,
 * the mirrored terms to V[p], V[n], +-c to b[p], b[n]; each row also gets reg * itself, T once per batch.
 * l2 rows: U[u], V[l], V[p], V[n], b[p], b[n] per triple and T once.  Row gradients are atomic scatters; T's gradient is
 * summed in a FIXED order (per wavefront, per workgroup, then the workgroups in order, in a second launch), so two
 * calls on the same inputs give the same bits.  d_work: float[SKR_TRANSREC_MAX_BLOCKS * dim] scratch, no initial
 * contents, not to be shared by calls that may run at the same time. */
#define SKR_TRANSREC_MAX_BLOCKS 1024
int skr_transrec_step(const float* d_U, const float* d_V, const float* d_bias, const float* d_T, const int32_t* d_u,
                      const int32_t* d_l, const int32_t* d_p, const int32_t* d_n, int n, int n_users, int n_items, int dim,
                      float reg, float* d_gU, float* d_gV, float* d_gb, float* d_gT, float* d_work, float* d_loss,
                      int loss_slots, void* stream);
/* Dense score rows d_out[b * ld + i], b < B, i < n_items, of the users d_users[b]; d_last_item: int32[n_users], the last
 * training item of every user (-1: none).  A user out of range or without a last item gets a row of NaN (callers raise
 * before they ask: the reference raises KeyError, FPMC.py:147).
 *   SKR_SEQ_FPMC      <user_table[u], item_table[i]> + <last_table[last], item_table2[i]>, the two sums kept apart
 *                     (UI, LI, IU, IL; d_transition and d_item_bias unused)
 *   SKR_SEQ_TRANSREC  -sqrt(sum_k (t_k - item_table[i]_k)^2) + d_item_bias[i], t = (user_table[u] + d_transition) +
 *                     last_table[last], from the differences, never from |t|^2 - 2 t.v + |v|^2 (U, V, V; item_table2 unused)
 * Item tables 16-byte aligned; B <= 65535 * 16. */
enum { SKR_SEQ_FPMC = 0, SKR_SEQ_TRANSREC = 1 };
int skr_seq_scores(int mode, const float* d_user_table, const float* d_last_table, const float* d_item_table,
                   const float* d_item_table2, const float* d_transition, const float* d_item_bias, const int32_t* d_users,
                   int B, const int32_t* d_last_item, int n_users, int n_items, int dim, float* d_out, int64_t ld,
                   void* stream);

/* ============================================================================================
 * R -- HGN, Hierarchical Gating Networks (csrc/hgn.hip)
 * replaces: _HGN._forward_user / forward / predict and HGN.fit's step (recommender/HGN.py:101-163,194-207).
 * Rows are 64 floats (dim must be 64: narrower embeddings zero-padded by the caller; the two gate matrices have to fit
 * LDS).  Tables: d_U [n_users, 64]; d_E (item_embeddings), d_W2 [n_rows, 64] and d_b2 [n_rows] with n_rows = items + 1,
 * row pad_idx being the padding row (-1: none): it reads as zeros in a window and never receives a gradient.
 * d_gates: the shared parameters, SKR_HGN_GATE_FLOATS(L) floats, 16-byte aligned:
 *   feature_gate_item.weight [64][64] (out, in) | feature_gate_user.weight [64][64] | feature_gate_item.bias [64] |
 *   feature_gate_user.bias [64] | instance_gate_item [64] | instance_gate_user TRANSPOSED, [L][64]
 * Per instance (u, window s_1..s_L, positives t_1..t_T, negatives t_T+1..t_2T), with p = U[u], e_l = E[s_l]:
 *   gate_l = sigmoid(Wi e_l + bi + Wu p + bu), g_l = e_l * gate_l, a_l = sigmoid(<g_l, w_item> + (p^T W_user)_l),
 *   union = sum_l a_l g_l / sum_l a_l (padding positions have g_l = 0 and count in the denominator),
 *   q = p + union + sum_l e_l,   y_t = b2[t] + <W2[t], q>.
 * Limits: 1 <= seq_L <= SKR_HGN_MAX_L, 1 <= seq_T <= SKR_HGN_MAX_T (the window, the instance gates and the targets of
 * an instance are held one per lane of a wavefront).
 * ========================================================================================== */
#define SKR_HGN_MAX_L 32
#define SKR_HGN_MAX_T 16
#define SKR_HGN_MAX_BLOCKS 256
#define SKR_HGN_GATE_FLOATS(L) (2 * 64 * 64 + 3 * 64 + 64 * (L))
/* One training batch, forward and backward: d_u int32[n], d_seq int32[n][seq_L], d_pos / d_neg int32[n][seq_T].  The
 * batch's sum over instances and pairs of -logsigmoid(y_pos_k - y_neg_k) is ADDED to word 0 of the d_loss pairs (float
 * [2 * loss_slots], loss_slots 1 or SKR_LOSS_SLOTS, spread over the workgroups as skr_fpmc_step; word 1 is left alone:
 * there is no l2 term, the regulariser is the optimiser's weight decay).  Row gradients (d_gU, d_gE, d_gW2, d_gb2) are
 * atomic scatter-adds; the padding row gets none.  The gate parameters' gradients are named by every instance and are
 * summed in a FIXED order (per wavefront, per workgroup, then the workgroups in order in a second launch) and ADDED to
 * d_ggates (layout of d_gates): two calls on the same inputs give the same bits for them.  An instance with an id
 * outside [0, n_users) / [0, n_rows) is skipped: it adds nothing to the loss or to any gradient (with pad_idx = -1 a -1 in
 * a window is such an id, not padding).  The loss is a sum, so n == 0 returns at once and touches nothing.  d_work: float[SKR_HGN_MAX_BLOCKS * SKR_HGN_GATE_FLOATS(seq_L)] scratch,
 * no initial contents, not to be shared by calls that may run at the same time. */
int skr_hgn_step(const float* d_U, const float* d_E, const float* d_W2, const float* d_b2, const float* d_gates,
                 const int32_t* d_u, const int32_t* d_seq, const int32_t* d_pos, const int32_t* d_neg, int n, int n_users,
                 int n_rows, int pad_idx, int dim, int seq_L, int seq_T, float* d_gU, float* d_gE, float* d_gW2, float* d_gb2,
                 float* d_ggates, float* d_work, float* d_loss, int loss_slots, void* stream);
/* Query rows: d_Q[u][0..63] = q of user u = d_users[i] (d_users NULL: u = i) from the window d_windows[i][0..seq_L), so
 * that the model's score of item t is <d_Q[u], W2[t]> + b2[t] (skr_eval_fused_topk, skr_score_matrix).  A window with an
 * entry outside [0, n_rows) -- by convention a negative first entry marks a user without training history -- gives a row
 * of NaN (callers raise before they ask: the reference raises KeyError, HGN.py:223).  Users out of range are skipped. */
int skr_hgn_queries(const float* d_U, const float* d_E, const float* d_gates, const int32_t* d_users, int n,
                    const int32_t* d_windows, int n_users, int n_rows, int pad_idx, int dim, int seq_L, float* d_Q,
                    void* stream);

/* ============================================================================================
 * S -- MultVAE, variational autoencoder with a multinomial likelihood (csrc/multvae.hip)
 * replaces: _MultVAE.q_graph / forward and MultVAE.fit's step (recommender/MultVAE.py:99-136,179-201) for p_dims = [d],
 * q_dims = None, d <= 64.
 * Tables: d_WqT [n_items, 128], the encoder weight transposed: an item's row is 64 mu columns then 64 logvar columns,
 * each half zero beyond dim; d_bq [128] likewise; d_Wp [n_items, 64] (16-byte aligned) and d_bp [n_items], the decoder.
 * A user's input is its row of the train CSR (d_rowptr int64 [n_users + 1], d_items int32, ASCENDING inside a row).
 * Per user u of the batch (n users, n <= SKR_MULTVAE_MAX_BATCH; a user outside [0, n_users) counts as an empty row, and
 * an empty row is a row of the batch: n stays the divisor of both means, the row's h is zero, so it adds nothing to
 * neg_ll and the KL of bq to kl, with that term's gradient going to d_gbq alone; the same user twice is two rows):
 *   h = x_u / ||x_u|| * keep / keep_prob,  e = h Wq^T + bq,  mu = e[:dim], logvar = e[64:64 + dim],
 *   z = mu + eps * exp(logvar / 2),  logits = z Wp^T + bp,
 *   neg_ll = -mean_u sum_{i in x_u} log_softmax(logits)_ui,  kl = mean_u sum 0.5 (-logvar + exp(logvar) + mu^2 - 1).
 * ========================================================================================== */
#define SKR_MULTVAE_MAX_BATCH 1024
#define SKR_MULTVAE_MAX_WG 512
/* bytes of d_work for a batch of n users: grows with n * 64 * min(ceil(n_items / 64), SKR_MULTVAE_MAX_WG), never with
 * n * n_items; 0 for arguments out of range */
size_t skr_multvae_workspace(int n, int n_items);
/* One training batch, forward and backward of neg_ll + anneal * kl (the l2 term is the optimiser's weight decay).
 * d_loss[0] = neg_ll, d_loss[1] = kl are WRITTEN.  The four gradients are ADDED to d_gWqT, d_gbq, d_gWp, d_gbp (layouts
 * of the tables; the caller's optimiser zeroes them).  Draws: d_keep (one byte per non-zero of the batch's rows, user
 * after user in batch order, items ascending) and d_eps (float [n, 64]) together, or both NULL: then the step draws on
 * the device, keyed by (seed, step, user, item) and (seed, step, user, column) -- a user's draws do not depend on the
 * rest of the batch; equal to the reference's torch draws in law only.  Nothing on the decoder side is a float atomic:
 * d_gWp, d_gbp, d_loss of two calls on the same inputs are bit-equal; d_gWqT rows are atomic scatter-adds.
 * n == 0 WRITES d_loss = (0, 0) and touches no gradient and no workspace.
 * d_work: skr_multvae_workspace(n, n_items) bytes, 16-byte aligned, no initial contents, not to be shared by calls that
 * may run at the same time. */
int skr_multvae_step(const float* d_WqT, const float* d_bq, const float* d_Wp, const float* d_bp, const int64_t* d_rowptr,
                     const int32_t* d_items, const int32_t* d_users, int n, int n_users, int n_items, int dim, float keep_prob,
                     float anneal, const uint8_t* d_keep, const float* d_eps, uint64_t seed, uint64_t step, float* d_gWqT,
                     float* d_gbq, float* d_gWp, float* d_gbp, void* d_work, size_t work_bytes, float* d_loss, void* stream);
/* The same step with an event after each of its SKR_MULTVAE_LAUNCHES launches (prep, encode, pass 1, merge, pass 2,
 * reduce, encoder backward, dbq): h_ms[k] (host) = milliseconds of launch k; synchronises the stream (timing tools). */
#define SKR_MULTVAE_LAUNCHES 8
int skr_multvae_step_timed(const float* d_WqT, const float* d_bq, const float* d_Wp, const float* d_bp,
                           const int64_t* d_rowptr, const int32_t* d_items, const int32_t* d_users, int n, int n_users,
                           int n_items, int dim, float keep_prob, float anneal, const uint8_t* d_keep, const float* d_eps,
                           uint64_t seed, uint64_t step, float* d_gWqT, float* d_gbq, float* d_gWp, float* d_gbp, void* d_work,
                           size_t work_bytes, float* d_loss, void* stream, float* h_ms);
/* Query rows: d_Q[u][0..63] = mu of user u = d_users[i] (d_users NULL: u = i) from its whole train row, no dropout, so
 * that the model's score of item t is <d_Q[u], Wp[t]> + bp[t] (skr_eval_fused_topk, skr_score_matrix).  An empty row
 * gives bq[0..63] (MultVAE.py:216-220 ranks such a user like any other).  Users out of range are skipped. */
int skr_multvae_queries(const float* d_WqT, const float* d_bq, const int64_t* d_rowptr, const int32_t* d_items,
                        const int32_t* d_users, int n, int n_users, int n_items, float* d_Q, void* stream);
/* The draws skr_multvae_step makes for (seed, step) when it is handed none, in the explicit form: d_off int32 [n + 1]
 * (offsets of the batch's rows in d_keep), d_keep one byte per non-zero, d_eps float [n, 64] (zero beyond dim). */
int skr_multvae_draws(const int64_t* d_rowptr, const int32_t* d_items, const int32_t* d_users, int n, int n_users, int dim,
                      float keep_prob, uint64_t seed, uint64_t step, int32_t* d_off, uint8_t* d_keep, float* d_eps,
                      void* stream);

/* ============================================================================================
 * S -- CDAE, collaborative denoising autoencoder (csrc/cdae.hip)
 * replaces: _CDAE.forward / _encoding / predict and CDAE.fit's step (recommender/CDAE.py:95-130,168-206) for
 * hidden_dim <= 64 and the sigmoid cross entropy loss.
 * Tables of 64-float rows, zero beyond dim, 16-byte aligned: d_E_en, d_E_de [n_items, 64], d_offset [64], d_U [n_users, 64];
 * d_bias [n_items].
 * A batch of n DISTINCT users (n <= SKR_CDAE_MAX_BATCH) is a pair list: user b = d_users[b] owns the pairs
 * [d_uptr[b], d_uptr[b + 1]) of d_pitem / d_plabel / d_pkeep -- its positives (label 1) and its de-duplicated negatives
 * (label 0), items ASCENDING, d_pkeep the dropout keep flag of the encoder input.  d_uptr[0] is the batch's first pair:
 * the three pair arrays and d_puser may belong to a longer list (a block of batches prepared at once) and are indexed by
 * the values of d_uptr as they are; n_pairs = d_uptr[n] - d_uptr[0].  d_puser[p] is the batch position of pair p.
 * The item-major view: distinct item d_ditems[j] (j < n_distinct) owns d_ipair[d_iptr[j] .. d_iptr[j + 1]), pair numbers
 * RELATIVE to d_uptr[0]; every pair is listed once.  Entries out of range are skipped, never followed, and what is
 * skipped contributes nothing to either loss word or to any gradient:
 *   - a user outside [0, n_users), and a user whose d_uptr pair is broken (below d_uptr[0], descending, or past n_pairs),
 *     owns no pairs: none of them is scored, counted in the BCE sum or followed from the item-major view; the user outside
 *     the range has no U row either (no l2 term, no d_gU row).  The BCE is a sum, so no divisor changes.
 *   - a pair whose d_pitem is outside [0, n_items) is skipped alone: nothing goes into its user's h, its dr is 0.
 *   - the item-major view follows a d_ipair entry only if it is inside [0, n_pairs), its d_puser is inside [0, n), the pair
 *     lies inside that user's d_uptr range (so its dr was written: d_work needs no initial contents whatever the pointers
 *     say) and the pair's d_pitem is the item that lists it; a broken d_iptr pair is an empty list.  A distinct item none
 *     of whose pairs is followed, or which is itself outside [0, n_items), is not named by the batch: no l2 term, no
 *     gradient row.
 *   h_u = act(sum_{kept i} E_en[i] / keep_prob + U[u] + offset),   r = <h_u, E_de[i]> + bias[i] for every pair,
 *   loss = sum_pairs bce_with_logits(r, label) + reg * l2,
 *   l2 = 0.5 (|E_en[J]|^2 + |offset|^2 + |U[users]|^2 + |E_de[J]|^2 + |bias[J]|^2), J the distinct items.
 * ========================================================================================== */
#define SKR_CDAE_MAX_BATCH 1024
#define SKR_CDAE_IDENTITY 0
#define SKR_CDAE_SIGMOID 1
/* bytes of d_work for n users and n_pairs pairs; 0 for arguments out of range */
size_t skr_cdae_workspace(int n, int64_t n_pairs);
/* One training batch, forward and backward.  d_loss[0] = the BCE sum, d_loss[1] = l2 (without reg) are WRITTEN.  The
 * gradient of the whole loss is WRITTEN into the rows the batch names -- d_gU[users], d_gE_en[J], d_gE_de[J], d_gbias[J]
 * and d_goffset [64] (layouts of the tables) -- and nothing else is touched: the caller's optimiser leaves the other
 * rows at zero.  No floating-point atomic: two calls on the same inputs give bit-equal results.
 * n == 0 WRITES d_loss = (0, 0) and touches no gradient and no workspace: the offset's batch-independent terms, its
 * 0.5 |offset|^2 in l2 and the reg * offset in d_goffset, are not produced for an empty batch.
 * d_work: skr_cdae_workspace(n, n_pairs) bytes, 16-byte aligned, no initial contents. */
int skr_cdae_step(const float* d_E_en, const float* d_E_de, const float* d_bias, const float* d_offset, const float* d_U,
                  const int32_t* d_users, const int32_t* d_uptr, const int32_t* d_pitem, const uint8_t* d_plabel,
                  const uint8_t* d_pkeep, const int32_t* d_puser, const int32_t* d_ditems, const int32_t* d_iptr,
                  const int32_t* d_ipair, int n, int64_t n_pairs, int n_distinct, int n_users, int n_items, int dim, int act,
                  float keep_prob, float reg, float* d_gE_en, float* d_gE_de, float* d_gbias, float* d_goffset, float* d_gU,
                  void* d_work, size_t work_bytes, float* d_loss, void* stream);
/* The same step with an event after each of its SKR_CDAE_LAUNCHES launches (user side, item side, finish): h_ms[k]
 * (host) = milliseconds of launch k; synchronises the stream (timing tools). */
#define SKR_CDAE_LAUNCHES 3
int skr_cdae_step_timed(const float* d_E_en, const float* d_E_de, const float* d_bias, const float* d_offset, const float* d_U,
                        const int32_t* d_users, const int32_t* d_uptr, const int32_t* d_pitem, const uint8_t* d_plabel,
                        const uint8_t* d_pkeep, const int32_t* d_puser, const int32_t* d_ditems, const int32_t* d_iptr,
                        const int32_t* d_ipair, int n, int64_t n_pairs, int n_distinct, int n_users, int n_items, int dim, int act,
                        float keep_prob, float reg, float* d_gE_en, float* d_gE_de, float* d_gbias, float* d_goffset, float* d_gU,
                        void* d_work, size_t work_bytes, float* d_loss, void* stream, float* h_ms);
/* Query rows: d_Q[u][0..63] = act(sum E_en[train(u)] + U[u] + offset) of user u = d_users[i] (d_users NULL: u = i) from
 * its train row (d_rowptr int64 [n_users + 1], d_items int32), no negatives, no dropout, zero beyond dim: the model's
 * score of item t is <d_Q[u], E_de[t]> + bias[t].  An empty row gives act(U[u] + offset).  Users out of range are skipped. */
int skr_cdae_queries(const float* d_E_en, const float* d_offset, const float* d_U, const int64_t* d_rowptr, const int32_t* d_items,
                     const int32_t* d_users, int n, int n_users, int n_items, int dim, int act, float* d_Q, void* stream);
/* Keep flags drawn on the device: d_pkeep[p] for pair p of batch position d_puser[p] is keyed by (seed, step + d_pstep[p],
 * user, item) (d_pstep NULL: step) -- a user's flags do not depend on the rest of the batch; equal to the reference's
 * torch draws in law only. */
int skr_cdae_draws(const int32_t* d_users, const int32_t* d_puser, const int32_t* d_pitem, const int32_t* d_pstep, int64_t n_pairs,
                   int n, float keep_prob, uint64_t seed, uint64_t step, uint8_t* d_pkeep, void* stream);

/* ============================================================================================
 * G -- LightGCL, graph contrastive learning with an SVD view (csrc/lightgcl.hip)
 * replaces: _LightGCL.forward and LightGCL.fit's step (recommender/LightGCL.py:117-169,222-232) at dropout = 0, d <= 64,
 * svd_q <= 16.
 * Tables of 64-float rows, zero beyond dim, 16-byte aligned; users and items share flat [n_users + n_items, 64] tables,
 * user rows first.  The SVD factors (LightGCL.py:202-204) are row-major [N, 16], zero beyond q.
 * ========================================================================================== */
#define SKR_LIGHTGCL_MAX_QUERIES 4096
#define SKR_LIGHTGCL_MAX_Q 16
#define SKR_LIGHTGCL_MAX_WG 512
/* The InfoNCE term of one side (LightGCL.py:146-147), forward and backward, with no [n, n_rows] array:
 *   s_bk = <d_Q[b], d_E[k]> * inv_temp,   lse_b = log(sum_k exp(s_bk) + 1e-8)   (evaluated without overflow for any s),
 *   d_loss[0] = weight * sum_b lse_b                                               WRITTEN
 *   d_dQ[b]   = weight * inv_temp * sum_k exp(s_bk - lse_b) d_E[k]                 WRITTEN, [n, 64]
 *   d_dE[k]   = weight * inv_temp * sum_b exp(s_bk - lse_b) d_Q[b]                 WRITTEN, [n_rows, 64]
 * d_Q [n, 64] (rows may repeat), n <= SKR_LIGHTGCL_MAX_QUERIES; d_E [n_rows, 64], any n_rows.  Products on the fp32 matrix
 * pipe with exact fp32 operands; no floating-point atomic: two calls on the same inputs give the same bits.
 * d_work: skr_lightgcl_cl_workspace(n, n_rows) bytes (0 for arguments out of range; grows with n * 64 * min(ceil(n_rows / 64),
 * SKR_LIGHTGCL_MAX_WG)), 16-byte aligned, no initial contents, not to be shared by calls that may run at the same time. */
size_t skr_lightgcl_cl_workspace(int n, int n_rows);
int skr_lightgcl_cl(const float* d_Q, int n, const float* d_E, int n_rows, float inv_temp, float weight, float* d_dQ, float* d_dE,
                    float* d_loss, void* d_work, size_t work_bytes, void* stream);
/* One training step, forward and backward, issued on `stream`: 2 n_layers plan runs forward, the low-rank view
 * G = E_0 + factor (factor^T S) at the batch's rows, the two InfoNCE terms, the clamped positive scores, the BPR term, and
 * 2 n_layers plan runs backward.  Every pointer is a device pointer except the plans.
 *   loss[0] = mean -logsigmoid(<E_u[u], E_i[p]> - <E_u[u], E_i[n]>), loss[1] = lambda1 (neg_score - pos_score),
 *   loss[2] = lambda2 |E0|^2, loss[3] = their sum (LightGCL.py:168)                 WRITTEN
 *   grad = the gradient of loss[0] + loss[1] with respect to E0                      WRITTEN, every row (the l2 term is the
 *          optimiser's weight decay 2 lambda2)
 *   sum  = E_u | E_i, the sums over the layers the reference keeps for evaluate()    WRITTEN
 * lambda1 == 0 skips the contrastive and low-rank work (factor tables, q and addend are then not used).  Ids out of range
 * are skipped, each id on its own: the BPR term of a pair needs its three ids, the log-sum-exp and the positive score of a
 * user (an item) need that id alone; n and 2 n stay the divisors of the means.  With n == 0 nothing is launched and NOTHING is
 * written, neither loss, grad nor sum (the arguments are still checked).
 * n <= SKR_LIGHTGCL_MAX_QUERIES / 2 pairs.  No floating-point atomic: the step is bit-reproducible. */
typedef struct skr_lightgcl_step_args {
    const skr_spmm_plan* plan_a;       /* A [n_users, n_items], values 1 / sqrt(rowdeg coldeg) (LightGCL.py:185-196) */
    const skr_spmm_plan* plan_at;      /* its transpose */
    int32_t n_users, n_items, dim, n_layers, q, n;
    const float* E0;                   /* [n_users + n_items, 64] the parameters */
    const float* fac_us;               /* u_mul_s [n_users, 16] */
    const float* fac_vs;               /* v_mul_s [n_items, 16] */
    const float* fac_ut;               /* ut^T    [n_users, 16] */
    const float* fac_vt;               /* vt^T    [n_items, 16] */
    const int32_t* uids;               /* [n] */
    const int32_t* pos;                /* [n] */
    const int32_t* neg;                /* [n] */
    float inv_temp, lambda1, lambda2;
    float* sum;                        /* [n_users + n_items, 64] */
    float* below;                      /* [n_users + n_items, 64] scratch: the sum of the layers below the last; NULL if n_layers == 1 */
    float* ping[2];                    /* [n_users + n_items, 64] scratch each; NULL if n_layers == 1 */
    float* gsum;                       /* [n_users + n_items, 64] scratch: dL / d sum */
    float* addend;                     /* [n_users + n_items, 64] scratch; NULL if lambda1 == 0 */
    float* grad;                       /* [n_users + n_items, 64] */
    float* loss;                       /* [4] */
    void* work;                        /* skr_lightgcl_workspace(n, n_users, n_items) bytes, 16-byte aligned, no initial contents */
    size_t work_bytes;
} skr_lightgcl_step_args;
size_t skr_lightgcl_workspace(int n, int n_users, int n_items);
int skr_lightgcl_step(const skr_lightgcl_step_args* args, void* stream);
/* The same step with an event after each of its SKR_LIGHTGCL_GROUPS launch groups (forward plan runs; sumsq, prep, low-rank
 * reductions, gather; user side pass 1 + merge; user side pass 2 + reduce; item side pass 1 + merge; item side pass 2 +
 * reduce; finish, seg_add, loss, dT, expansion; backward plan runs + seg_add): h_ms[k] (host) = milliseconds of group k;
 * synchronises the stream (timing tools). */
#define SKR_LIGHTGCL_GROUPS 8
int skr_lightgcl_step_timed(const skr_lightgcl_step_args* args, void* stream, float* h_ms);

/* ============================================================================================
 * H -- DENS, disentangled negative sampling on a propagated embedding (csrc/dens.hip)
 * replaces: _DENS.forward, dise_negative_sampling, create_bpr_loss and DENS.fit's step (recommender/DENS.py:115-136,
 * 196-257, 318-374, 449-453) at ns = "dens", pool = "mean", K = 1, no message or edge dropout, dim <= 64.
 * Tables of 64-float rows, zero beyond dim, 16-byte aligned; users and items share flat [n_users + n_items, 64] tables,
 * user rows first.  The parameters are ONE flat buffer: the [n_users + n_items, 64] rows, then the four gate blocks
 * user_gate, item_gate, pos_gate, neg_gate of SKR_DENS_GATE_FLOATS each: W row-major [64 out][64 in], then b [64], zero
 * beyond dim.  The gradient has the same layout.
 * ========================================================================================== */
#define SKR_DENS_MAX_BATCH 2048
#define SKR_DENS_MAX_NEGS 16
#define SKR_DENS_MAX_HOPS 3
#define SKR_DENS_MAX_WG 128
#define SKR_DENS_GATE_FLOATS (64 * 64 + 64)
/* One training step, forward and backward, issued on `stream`.  Every pointer is a device pointer except the plans.
 *   X_0 = the parameter rows, X_h = A-hat X_(h-1): 2 n_hops plan runs; per batch row b and hop h, with s = X_h[u],
 *   p = X_h[pos], c_k = X_h[cand_k]:  gp = sigmoid(item_gate(p) + user_gate(s)), gn_k = sigmoid(neg_gate(c_k) + pos_gate(p gp)),
 *   k*(b, h) = argmax_k <s, w c_k - c_k gn_k> (the first of equal scores); the loss of DENS.py:318-374 on the hop means with the
 *   gate values of the selection; its backward, the hop-h gradient rows added per distinct node in a fixed order, then
 *   acc = G_H, acc = A-hat acc + G_h for h = n_hops-1 .. 0: 2 n_hops plan runs.
 *   loss[0] = mf, loss[1] = emb, loss[2] = mf + emb                                   WRITTEN
 *   grad = the gradient of loss[2] with respect to the flat parameter buffer          WRITTEN, every element
 *   sel_out[b, h] = k*(b, h)                                                           WRITTEN when not NULL
 *   sel_in[b, h] >= 0 forces k*(b, h) to that candidate (values beyond n_negs - 1 are clamped); -1: the kernel chooses
 * The gamma terms apply when gamma > 0.  Rows whose user or positive item is out of range contribute nothing, neither to mf
 * nor to emb nor to a gradient (n stays the divisor of both); a candidate out of range counts as a zero row.  With n == 0
 * nothing is launched and NOTHING is written, neither loss, grad, sel_out nor a hop table (the arguments are still checked).
 * Every product of the selection is fp32 (v_mfma_f32_16x16x4_f32 and fp32 VALU).
 * No floating-point atomic: the step is bit-reproducible. */
typedef struct skr_dens_step_args {
    const skr_spmm_plan* plan_a;       /* A [n_users, n_items], values 1 / sqrt(rowdeg coldeg); may be NULL if n_hops == 0 */
    const skr_spmm_plan* plan_at;      /* its transpose */
    int32_t n_users, n_items, dim, n_hops, n_negs, n;
    const float* params;               /* the flat parameter buffer */
    const int32_t* uids;               /* [n] */
    const int32_t* pos;                /* [n] */
    const int32_t* cand;               /* [n, n_negs] */
    const int32_t* sel_in;             /* [n, n_hops + 1] or NULL */
    int32_t* sel_out;                  /* [n, n_hops + 1] or NULL */
    float w;                           /* 1 - min(1, epoch / warmup) */
    float gamma, l2;
    float* hop[SKR_DENS_MAX_HOPS];     /* X_1 .. X_(n_hops), [n_users + n_items, 64] each              WRITTEN */
    float* G[SKR_DENS_MAX_HOPS + 1];   /* scratch, [n_users + n_items, 64] each: G_0 .. G_(n_hops); not used if n_hops == 0 */
    float* ping;                       /* scratch, [n_users + n_items, 64]; NULL if n_hops < 2 */
    float* grad;                       /* the flat gradient buffer */
    float* loss;                       /* [3] */
    void* work;                        /* skr_dens_workspace(n, n_hops) bytes, 16-byte aligned, no initial contents */
    size_t work_bytes;
} skr_dens_step_args;
size_t skr_dens_workspace(int n, int n_hops);
int skr_dens_step(const skr_dens_step_args* args, void* stream);
/* The same step with an event after each of its SKR_DENS_GROUPS launch groups (forward plan runs; select; pool and loss;
 * back and gate_reduce; clears, rank and seg_add; backward plan runs): h_ms[k] (host) = milliseconds of group k;
 * synchronises the stream (timing tools). */
#define SKR_DENS_GROUPS 6
int skr_dens_step_timed(const skr_dens_step_args* args, void* stream, float* h_ms);

/* ============================================================================================
 * I -- SelfCF, self-supervised collaborative filtering with edge dropout (csrc/selfcf.hip)
 * replaces: LightGCN_Encoder.sparse_dropout / forward, SELFCFED_LGN.forward / calculate_loss / full_sort_predict and
 * SelfCF.fit's step (recommender/SelfCF.py:133-168, 205-241, 267-274) at embed_dim <= 64.
 * Tables of 64-float rows, zero beyond dim, 16-byte aligned; users and items share flat [n_users + n_items, 64] tables,
 * user rows first.  The parameters are ONE flat buffer: the [n_users + n_items, 64] rows, then the predictor's W row-major
 * [64 out][64 in] and b [64] (SKR_SELFCF_PRED_FLOATS), zero beyond dim.  The gradient has the same layout.
 * R is the binary train matrix in CSR, A the plan of its normalisation (SelfCF.py:118-123), At the plan of the transpose;
 * perm[e] is the position in At's entry order of entry e of A's.
 * ========================================================================================== */
#define SKR_SELFCF_MAX_BATCH 2048
#define SKR_SELFCF_MAX_LAYERS 4
#define SKR_SELFCF_PRED_FLOATS (64 * 64 + 64)
/* The four keep arrays of one step's plan runs, nnz bytes each.  The reference masks the 2 nnz entries of the square
 * matrix independently (SelfCF.py:147-149): k1 [nnz] covers the user rows (A's order), k2 [nnz] the item rows (At's order),
 * and the masked matrix [[0, R1], [R2^T, 0]] is not symmetric.
 *   d_fu = k1 (forward, user rows: runs of A)        d_fi = k2 (forward, item rows: runs of At)
 *   d_bu = k2 in A's order (backward, user rows)     d_bi = k1 in At's order (backward, item rows)
 * d_k1 / d_k2 NULL: drawn on the device -- keep iff a 24-bit uniform keyed by (seed, step, half, entry) is >= rate (the
 * reference's floor(1 - rate + rand), equal in law only). */
int skr_selfcf_keeps(const int32_t* d_perm, int64_t nnz, const uint8_t* d_k1, const uint8_t* d_k2, float rate, uint64_t seed,
                     uint64_t step, uint8_t* d_fu, uint8_t* d_fi, uint8_t* d_bu, uint8_t* d_bi, void* stream);
/* One training step, forward and backward, issued on `stream`.  Every pointer is a device pointer except the plans.
 *   X_0 = the parameter rows, X_k = A-hat' X_(k-1) through skr_spmm_plan_run_dropped (2 n_layers runs), M = mean_k X_k;
 *   with u = M[users], i = M[n_users + items]:  p_u = W u + b, p_i = W i + b, t_u = u ku / (1 - dropout),
 *   t_i = i ki / (1 - dropout), c(x, y) = <x, y> / (max(|x|, 1e-8) max(|y|, 1e-8)),
 *   loss[0] = -mean c(p_u, t_i) / 2 - mean c(p_i, t_u) / 2, loss[1] = reg * 0.5 * (sum u^2 + sum i^2) over the batch rows
 *   (duplicates counted), loss[2] = their sum (SelfCF.py:221-233)                      WRITTEN
 *   grad = the gradient of loss[2] with respect to the flat parameter buffer            WRITTEN, every element
 *   M                                                                                  WRITTEN
 * The targets carry no gradient.  ku / ki NULL: drawn on the device, keyed by (seed, step, side, row, column), the user
 * side first.  Rows whose user or item is out of range contribute nothing (n stays the divisor of the two means; loss[1] is a
 * sum over the remaining rows).  With n == 0 nothing is launched and NOTHING is written, neither loss, grad nor M (the
 * arguments are still checked).  The predictor's products run as 16-row tiles on
 * v_mfma_f32_16x16x4_f32 with fp32 operands.  No floating-point atomic: the step is bit-reproducible. */
typedef struct skr_selfcf_step_args {
    const skr_spmm_plan* plan_a;       /* A [n_users, n_items]; may be NULL if n_layers == 0 */
    const skr_spmm_plan* plan_at;      /* its transpose */
    int32_t n_users, n_items, dim, n_layers, n;
    const float* params;               /* the flat parameter buffer */
    const int32_t* users;              /* [n] */
    const int32_t* items;              /* [n] */
    const uint8_t* keep_fu;            /* skr_selfcf_keeps' four arrays; not used if n_layers == 0 */
    const uint8_t* keep_fi;
    const uint8_t* keep_bu;
    const uint8_t* keep_bi;
    float edge_scale;                  /* float32(1 / (1 - rate)) */
    const uint8_t* ku;                 /* [n, 64] the user targets' keep flags, or NULL */
    const uint8_t* ki;                 /* [n, 64] the item targets' keep flags, or NULL */
    float dropout, reg;
    uint64_t seed, step;               /* key of the device draws of ku / ki */
    float* M;                          /* [n_users + n_items, 64] */
    float* ping[2];                    /* scratch, [n_users + n_items, 64] each; NULL if n_layers < 2 */
    float* G;                          /* scratch, [n_users + n_items, 64]; not used if n_layers == 0 */
    float* grad;                       /* the flat gradient buffer */
    float* loss;                       /* [3] */
    void* work;                        /* skr_selfcf_workspace(n, n_layers) bytes, 16-byte aligned, no initial contents */
    size_t work_bytes;
} skr_selfcf_step_args;
size_t skr_selfcf_workspace(int n, int n_layers);
int skr_selfcf_step(const skr_selfcf_step_args* args, void* stream);
/* The same step with an event after each of its SKR_SELFCF_GROUPS launch groups (forward plan runs; batch kernel, predictor
 * reduction and loss; clear, rank and seg_add; backward plan runs): h_ms[k] (host) = milliseconds of group k; synchronises
 * the stream (timing tools). */
#define SKR_SELFCF_GROUPS 4
int skr_selfcf_step_timed(const skr_selfcf_step_args* args, void* stream, float* h_ms);
/* Ranking (SelfCF.py:235-241): the score (W u + b).i + u.(W i + b) = u^T (W + W^T) i + <b, i> + <b, u>, so
 *   d_Q[r] = (W + W^T) M_r for the n_users user rows, d_item_bias[t] = <b, M_(n_users + t)>, d_user_const[r] = <b, M_r>:
 * skr_eval_fused_topk ranks <d_Q[u], M_i> + d_item_bias[i]; the per-user constant does not move a ranking.
 * d_pred: the predictor's W and b (SKR_SELFCF_PRED_FLOATS floats). */
int skr_selfcf_queries(const float* d_pred, const float* d_M, int n_users, int n_items, float* d_Q, float* d_item_bias,
                       float* d_user_const, void* stream);

/* ============================================================================================
 * J -- BM3, bootstrapped multi-modal recommendation (csrc/bm3.hip)
 * replaces: _BM3.forward / calculate_loss / full_sort_predict and BM3.fit's step (recommender/BM3.py:142-210, 236-243) at
 * embed_dim <= 64, with trainable item feature tables of up to SKR_BM3_MAX_FEAT columns per modality.
 * Tables of 64-float rows, zero beyond dim, 16-byte aligned; users and items share flat [n_users + n_items, 64] tables,
 * user rows first.  params = the [n_users + n_items, 64] rows, then the predictor's W row-major [64 out][64 in] and b [64]
 * (SKR_BM3_PRED_FLOATS), zero beyond dim; grad has the same layout.  Modality 0 is the image block, 1 the text block
 * (feat_dim 0 = absent): a feature table is [n_items][feat_ld] floats, feat_ld = feat_dim rounded up to a multiple of 4,
 * zero beyond feat_dim; its projection block is W [64 out][feat_ld], then b [64], zero beyond dim and feat_dim.
 * A is the plan of the normalised train matrix (BM3.py:116-140; the same values as SelfCF's), At the plan of its transpose.
 * ========================================================================================== */
#define SKR_BM3_MAX_BATCH 2048
#define SKR_BM3_MAX_LAYERS 4
#define SKR_BM3_MAX_FEAT 4096
#define SKR_BM3_PRED_FLOATS (64 * 64 + 64)
/* the tables of the target draws, in the order the reference draws them (BM3.py:168-177) */
enum { SKR_BM3_DRAW_USER = 0, SKR_BM3_DRAW_ITEM = 1, SKR_BM3_DRAW_TEXT = 2, SKR_BM3_DRAW_IMAGE = 3 };
/* d_Y[r, :] = X[ids[r], :feat_dim] W^T + b for r < n (nn.Linear on the batch's rows of an nn.Embedding, BM3.py:160-162): d_X
 * [n_rows][feat_ld], d_trs = W [64][feat_ld] then b [64], d_Y [n][64].  16-row tiles on v_mfma_f32_16x16x4_f32, fp32 operands,
 * one wavefront per tile walking the feat_dim terms 64 at a time in a fixed order (the range is not split over workgroups).
 * A row whose id is outside [0, n_rows) gets b alone. */
int skr_bm3_project(const float* d_X, int n_rows, int feat_dim, int feat_ld, const float* d_trs, const int32_t* d_ids, int n,
                    float* d_Y, void* stream);
/* The keep flags of the device draws: d_out[r][c] (uint8 [n][64]) = 1 iff a 24-bit uniform keyed by (seed, step, table,
 * ids[r], c) is >= rate -- rows of one node are identical.  F.dropout's mask in law only. */
int skr_bm3_draws(const int32_t* d_ids, int n, int table, float rate, uint64_t seed, uint64_t step, uint8_t* d_out, void* stream);
/* One training step, forward and backward, issued on `stream`.  Every pointer is a device pointer except the plans.
 *   M = mean_{k=0..n_layers} A-hat^k X_0 through skr_spmm_plan_run_ex (2 n_layers runs), then M_items += X_0 items (BM3.py:153);
 *   T = skr_bm3_project of the text block at the batch's items, V of the image block; P(x) = W x + b;
 *   targets x keep / (1 - dropout) of M_u, M_i, T, V at the batch's rows, no gradient; c = F.cosine_similarity (eps 1e-8);
 *   loss[0] = (1 - mean c(P(M_u[u]), i_tgt)) + (1 - mean c(P(M_i[i]), u_tgt))
 *   loss[1] = cl_weight * sum over the present X in (T, V) of (1 - mean c(P(X[i]), i_tgt)) + (1 - mean c(P(X[i]), x_tgt))
 *   loss[2] = reg * (|M_u|_F + |M_i|_F) / n_items over the WHOLE tables;  loss[3] = their sum          WRITTEN
 *   grad, trs_grad[m]: the gradient of loss[3], every element                                          WRITTEN
 *   feat_grad[m]: first the rows named by clear_items are zeroed (the rows the previous step wrote: the table is never
 *   filled as a whole), then the row of every distinct item of the batch is written; all other rows are left as they are
 *   (zero, if every step hands in the previous step's items).
 * keep[t] ([n, 64] bytes per table of SKR_BM3_DRAW_*; a repeated node must carry equal rows) are handed in together or all
 * NULL: drawn on the device, keyed by (seed, step, table, node id, column).  Rows whose user or item is out of range
 * contribute nothing (n stays the divisor of every mean; loss[2] does not depend on the batch).  With n == 0 nothing is
 * launched and NOTHING is written, neither loss, a gradient nor M, and no feat_grad row is cleared (the arguments are still
 * checked).  The predictor's and the projections' products run on v_mfma_f32_16x16x4_f32 with fp32 operands.  No
 * floating-point atomic, every sum in a fixed order: the step is bit-reproducible. */
typedef struct skr_bm3_step_args {
    const skr_spmm_plan* plan_a;       /* A [n_users, n_items]; may be NULL if n_layers == 0 */
    const skr_spmm_plan* plan_at;      /* its transpose */
    int32_t n_users, n_items, dim, n_layers, n;
    int32_t feat_dim[2];               /* image, text; 0 = the modality is absent */
    int32_t feat_ld[2];
    const float* params;
    const float* trs[2];               /* W [64][feat_ld], then b [64] */
    const float* feat[2];              /* [n_items][feat_ld] */
    const int32_t* users;              /* [n] */
    const int32_t* items;              /* [n] */
    const int32_t* clear_items;        /* [n_clear] item ids whose feat_grad rows are zeroed first; may be NULL if n_clear == 0 */
    int32_t n_clear;
    const uint8_t* keep[4];            /* [n, 64] each, indexed by SKR_BM3_DRAW_*; all NULL: device draws */
    float dropout, reg, cl_weight;
    uint64_t seed, step;               /* key of the device draws */
    float* M;                          /* [n_users + n_items, 64] */
    float* ping[2];                    /* scratch, [n_users + n_items, 64] each; NULL if n_layers < 2 */
    float* G;                          /* scratch, [n_users + n_items, 64]; not used if n_layers == 0 */
    float* grad;
    float* trs_grad[2];
    float* feat_grad[2];
    float* loss;                       /* [4] */
    void* work;                        /* skr_bm3_workspace(n) bytes, 16-byte aligned, no initial contents */
    size_t work_bytes;
} skr_bm3_step_args;
size_t skr_bm3_workspace(int n);
int skr_bm3_step(const skr_bm3_step_args* args, void* stream);
/* The same step with an event after each of its SKR_BM3_GROUPS launch groups (forward plan runs; + h and the sums of squares;
 * projections; batch kernel, predictor reduction and loss; projection backward; dense regulariser, rank and seg_add; backward
 * plan runs): h_ms[k] (host) = milliseconds of group k; synchronises the stream (timing tools). */
#define SKR_BM3_GROUPS 7
int skr_bm3_step_timed(const skr_bm3_step_args* args, void* stream, float* h_ms);
/* Ranking (BM3.py:206-210): d_Qu[r] = W M_r + b for the n_users user rows, d_Qi[t] = W M_(n_users + t) + b for the item rows
 * (zero beyond dim): skr_eval_fused_topk ranks <d_Qu[u], d_Qi[i]>.  d_pred: SKR_BM3_PRED_FLOATS floats. */
int skr_bm3_queries(const float* d_pred, const float* d_M, int n_users, int n_items, float* d_Qu, float* d_Qi, void* stream);

/* ============================================================================================
 * K -- k-nearest-neighbour lists of a feature table by cosine similarity (csrc/knn.hip)
 * replaces: the item-graph construction of the reference's multimodal models -- X / |X|, torch.mm(X, X^T) as a dense
 * [I, I] matrix and torch.topk per row (recommender/FREEDOM.py:126-129, LATTICE.py:67-90, MGCN.py:61-110).
 * d_X is a feature table in the layout of section J: [n_rows][feat_ld] floats, 16-byte aligned, feat_ld a multiple of 4,
 * zero beyond feat_dim.
 * ========================================================================================== */
#define SKR_KNN_MAX_K 32
/* Bytes of d_work for skr_knn_topk (the rows' inverse norms); 0 unless n_rows > 0 and 1 <= k <= min(SKR_KNN_MAX_K, n_rows). */
size_t skr_knn_workspace(int n_rows, int k);
/* d_ids[i][0..k) = the k rows j with the largest s(i, j) = <X_i, X_j> / (max(|X_i|, 1e-12) max(|X_j|, 1e-12)), row i itself
 * included, in descending order of s; equal similarities rank by ascending j.  d_sims[i][0..k) = those similarities, or NULL.
 * WRITTEN: all n_rows * k entries of d_ids (and of d_sims), nothing else.
 * The one deviation from the reference: a norm is clamped at 1e-12, so an all-zero row has similarity 0 to every row (its own
 * list is the k lowest ids) where the reference's division yields NaN.
 * Limits: 1 <= feat_dim <= SKR_BM3_MAX_FEAT, feat_dim <= feat_ld <= SKR_BM3_MAX_FEAT, 1 <= k <= SKR_KNN_MAX_K, k <= n_rows.
 * The products run on v_mfma_f32_16x16x4_f32 with fp32 operands; the inverse norms (one small launch) scale the finished
 * 64 x 256 tile, the table is never copied.  No [n_rows, n_rows] array nor any O(n_rows^2) array is formed: d_work holds
 * n_rows floats.  Every sum has a fixed order and there is no atomic: two calls give the same bits. */
int skr_knn_topk(const float* d_X, int n_rows, int feat_dim, int feat_ld, int k, int32_t* d_ids, float* d_sims, void* d_work,
                 size_t work_bytes, void* stream);

/* ============================================================================================
 * L -- FREEDOM, frozen item graph and degree-sensitive edge pruning (csrc/freedom.hip)
 * replaces: _FREEDOM.pre_epoch_processing / _normalize_adj_m / forward / calculate_loss and FREEDOM.fit's step
 * (recommender/FREEDOM.py:175-252, 285-295) at embed_dim <= 64.
 * Tables of 64-float rows, zero beyond dim, 16-byte aligned; users and items share flat [n_users + n_items, 64] tables,
 * user rows first.  Feature tables and projection blocks are section J's: [n_items][feat_ld] and W [64][feat_ld] | b [64].
 * R is the binary train matrix in CSR (nnz entries, columns ascending), R^T its transpose, perm[e] the position in R^T's
 * entry order of entry e of R's.  S is the frozen item graph [n_items, n_items] (section K, build_item_graph).
 * ========================================================================================== */
#define SKR_FREEDOM_MAX_BATCH 2048
#define SKR_FREEDOM_MAX_LAYERS 4
#define SKR_FREEDOM_MAX_FEAT 4096
#define SKR_FREEDOM_MAX_NNZ 2147483647LL
/* The pruning of one epoch (FREEDOM.py:175-190) in three entries.
 * d_keys[e] = d_w[e] / E_e with E_e a unit exponential from 32 random bits of fast_rng.h's generator keyed by (seed, epoch, e),
 * the division in float64: the n_keep largest keys are a sample without replacement with probabilities proportional to w.
 * torch.multinomial is built the same way on another generator: the kept set equals the reference's in law only.  A key is
 * finite, and positive where w is. */
int skr_freedom_keys(const float* d_w, int64_t nnz, uint64_t seed, uint64_t epoch, float* d_keys, void* stream);
/* d_keep[e] (uint8 [nnz]) = 1 for exactly n_keep entries: those with the largest keys, equal keys ranked by ascending e.
 * Keys must be >= 0 and no NaN: the select is a radix select on their bit patterns -- four histogram passes of 8 bits
 * (integer atomics), then one ordered pass that admits the ties at the threshold by index.  0 <= n_keep <= nnz.  d_work:
 * skr_freedom_select_workspace(nnz) bytes, 16-byte aligned, no initial contents.  Two calls give the same bytes. */
size_t skr_freedom_select_workspace(int64_t nnz);
int skr_freedom_select(const float* d_keys, int64_t nnz, int64_t n_keep, uint8_t* d_keep, void* d_work, size_t work_bytes,
                       void* stream);
/* The kept entries (d_keep, uint8 [nnz] in R's entry order) as the CSR of R' and of R'^T, every array sized for nnz entries
 * (an empty row is fine): rowptr int64, columns int32 ascending, values fp32
 *   float(pow(1e-7 + kept entries of the row, -0.5)) * float(pow(1e-7 + kept entries of the column, -0.5))
 * with the powers in float64 and one fp32 product (_normalize_adj_m, FREEDOM.py:192-201, whose fp32 powers are within 1 ulp).
 * d_n_kept[0] = the number of kept entries.  d_work: skr_freedom_pruned_workspace bytes, 16-byte aligned. */
size_t skr_freedom_pruned_workspace(int n_users, int n_items, int64_t nnz);
int skr_freedom_pruned_csr(int n_users, int n_items, int64_t nnz, const int64_t* d_rowptr, const int32_t* d_col,
                           const int64_t* d_rowptr_t, const int32_t* d_col_t, const int32_t* d_perm, const uint8_t* d_keep,
                           int64_t* d_out_rowptr, int32_t* d_out_col, float* d_out_val, int64_t* d_out_rowptr_t,
                           int32_t* d_out_col_t, float* d_out_val_t, int64_t* d_n_kept, void* d_work, size_t work_bytes,
                           void* stream);
/* One training step, forward and backward, issued on `stream`.  Every pointer is a device pointer except the plans.
 *   M = mean_{k=0..n_ui_layers} A'^k X_0 through skr_spmm_plan_run_ex (2 n_ui_layers runs), then M_items += S^n_mm_layers
 *   X_0 items (n_mm_layers runs; with n_mm_layers == 0, X_0's item rows);
 *   u = M[users], p = M[n_users + pos], q = M[n_users + neg], x_g = <u, p - q>; at reg > 0, per present modality m,
 *   x_m = <u, P_m - Q_m> with P_m / Q_m = skr_bm3_project at pos / neg; ls(x) = min(x, 0) - log1p(exp(-|x|));
 *   loss[0] = -mean ls(x_g), loss[1] = reg * sum_m -mean ls(x_m), loss[2] = their sum                   WRITTEN
 *   grad: the gradient of loss[2] with respect to the [n_users + n_items, 64] rows, every element        WRITTEN
 *   at reg > 0: trs_grad[m] (W: every element; b: exact zeros, it cancels in x_m) and feat_grad[m] -- first the rows named
 *   by clear_items are zeroed, then the row of every distinct item of pos || neg is written; other rows are left alone.
 * At reg == 0 the modal arguments are not looked at and nothing is launched for them.  Rows with a user or item out of range
 * contribute nothing (n stays the divisor of every mean).  With n == 0 nothing is launched and NOTHING is written, neither
 * loss, a gradient nor M, and no feat_grad row is cleared (the arguments are still checked).
 * No floating-point atomic, every sum in a fixed order: the step is bit-reproducible. */
typedef struct skr_freedom_step_args {
    const skr_spmm_plan* plan_a;       /* A' [n_users, n_items]: this epoch's pruned matrix; may be NULL if n_ui_layers == 0 */
    const skr_spmm_plan* plan_at;      /* its transpose */
    const skr_spmm_plan* plan_s;       /* S [n_items, n_items]; may be NULL if n_mm_layers == 0 */
    const skr_spmm_plan* plan_st;      /* its transpose */
    int32_t n_users, n_items, dim, n_ui_layers, n_mm_layers, n;
    int32_t feat_dim[2];               /* image, text; 0 = the modality is absent */
    int32_t feat_ld[2];
    const float* params;               /* [n_users + n_items, 64] */
    const float* trs[2];               /* W [64][feat_ld], then b [64] */
    const float* feat[2];              /* [n_items][feat_ld] */
    const int32_t* users;              /* [n] */
    const int32_t* pos;                /* [n] */
    const int32_t* neg;                /* [n] */
    const int32_t* clear_items;        /* [n_clear <= 2 * SKR_FREEDOM_MAX_BATCH] item ids whose feat_grad rows are zeroed first */
    int32_t n_clear;
    float reg;
    float* M;                          /* [n_users + n_items, 64] */
    float* ping[2];                    /* scratch, [n_users + n_items, 64] each; NULL if both layer counts are < 2 */
    float* G;                          /* scratch, [n_users + n_items, 64] */
    float* grad;                       /* [n_users + n_items, 64] */
    float* trs_grad[2];
    float* feat_grad[2];
    float* loss;                       /* [3] */
    void* work;                        /* skr_freedom_workspace(n) bytes, 16-byte aligned, no initial contents */
    size_t work_bytes;
} skr_freedom_step_args;
size_t skr_freedom_workspace(int n);
int skr_freedom_step(const skr_freedom_step_args* args, void* stream);
/* The same step with an event after each of its SKR_FREEDOM_GROUPS launch groups (user-item plan runs forward; item-graph
 * runs; clear and projections; batch kernel and loss; clear of G, rank and seg_add; projection backward; backward plan runs of
 * both graphs): h_ms[k] (host) = milliseconds of group k; synchronises the stream (timing tools). */
#define SKR_FREEDOM_GROUPS 7
int skr_freedom_step_timed(const skr_freedom_step_args* args, void* stream, float* h_ms);

/* ============================================================================================
 * M -- MGCN, multi-view graph convolution with a purifier and a fuser (csrc/mgcn.hip)
 * replaces: _MGCN.forward / calculate_loss / full_sort_predict and MGCN.fit's step (recommender/MGCN.py:250-361, 388-396) at
 * embed_dim <= 64, sparse branch.
 * Tables of 64-float rows, zero beyond dim, 16-byte aligned; users and items share flat [n_users + n_items, 64] tables,
 * user rows first.  Feature tables and projection blocks are section J's: [n_items][feat_ld] and W [64][feat_ld] | b [64];
 * modality 0 is the image block, 1 the text block, and both are required.  A gate block is W [64 out][64 in] | b [64]
 * (SKR_MGCN_GATE_FLOATS), zero beyond dim.  The query block is the gate block of query_common.0 followed by q [64]
 * (query_common.2.weight): SKR_MGCN_QUERY_FLOATS floats.
 * DEVIATION from "every product on v_mfma_f32_16x16x4_f32": operands are fp32 in mfma_tile.h's layouts everywhere, but only the
 * fuser's four products run on that instruction.  The projections forward and backward, the gate and rows-times-W products,
 * InfoNCE's two products and the reductions over rows behind the weight gradients add the same operands on
 * v_mfma_f64_16x16x4_f64 (mfma_tile.h's float64 helpers; half the matrix rate) and round once.  With fp32 accumulators the
 * golden replay of the reference missed its bound in one tensor through one element whose first gradient lies beside Adam's eps
 * (MGCN).  No floating-point atomic, every sum in a fixed order: all entries are bit-reproducible.
 * ========================================================================================== */
#define SKR_MGCN_MAX_BATCH 2048
#define SKR_MGCN_MAX_LAYERS 4
#define SKR_MGCN_MAX_FEAT 4096
#define SKR_MGCN_GATE_FLOATS (64 * 64 + 64)
#define SKR_MGCN_QUERY_FLOATS (64 * 64 + 64 + 64)
/* d_Y[r, :] = X[r, :feat_dim] W^T + b for ALL n_rows rows (nn.Linear on the whole nn.Embedding, MGCN.py:251-254): d_X
 * [n_rows][feat_ld], d_trs = W [64][feat_ld] then b [64], d_Y [n_rows][64].  skr_bm3_project's tile without the gather (that
 * entry takes at most SKR_BM3_MAX_BATCH rows), summed in float64. */
int skr_mgcn_project(const float* d_X, int n_rows, int feat_dim, int feat_ld, const float* d_trs, float* d_Y, void* stream);
/* The rows of one row block of the reductions over rows below (a multiple of 16, 256 up to 16 384 rows): a reduction over
 * n_rows rows adds ceil(n_rows / block) partial sums in block order. */
int skr_mgcn_row_block(int n_rows);
/* The backward of skr_mgcn_project given d_dF [n_rows][64]: d_dtrs = dW [64][feat_ld] = dF^T X, then db [64] = the column sums
 * of dF; d_dX [n_rows][feat_ld] = dF W.  EVERY element of d_dtrs and d_dX is WRITTEN.  dW and db are reductions over the rows:
 * per-row-block partial sums in d_work, added in block order.  d_work: skr_mgcn_project_bwd_workspace bytes, 16-byte aligned. */
size_t skr_mgcn_project_bwd_workspace(int n_rows, int feat_ld);
int skr_mgcn_project_bwd(const float* d_dF, const float* d_X, int n_rows, int feat_dim, int feat_ld, const float* d_trs,
                         float* d_dtrs, float* d_dX, void* d_work, size_t work_bytes, void* stream);
/* The purifier (MGCN.py:257-258): d_g = sigmoid(F Wg^T + bg) (zero beyond dim), d_X = E * g, all [n_rows][64]; the gate lies
 * in LDS, a wavefront owns a 16-row tile. */
int skr_mgcn_purify(const float* d_F, const float* d_E, const float* d_gate, int n_rows, int dim, float* d_g, float* d_X,
                    void* stream);
/* Its backward given d_dX: d_dE += dX g (ACCUMULATED); dz = dX E g (1 - g); d_dF = dz Wg (WRITTEN); d_dgate = dz^T F | the
 * column sums of dz (WRITTEN, ordered partial sums as above).  d_work: skr_mgcn_purify_bwd_workspace bytes. */
size_t skr_mgcn_purify_bwd_workspace(int n_rows);
int skr_mgcn_purify_bwd(const float* d_dX, const float* d_E, const float* d_g, const float* d_F, const float* d_gate, int n_rows,
                        float* d_dE, float* d_dF, float* d_dgate, void* d_work, size_t work_bytes, void* stream);
/* The fuser (MGCN.py:291-305), row-local over n_rows rows of M, Zv, Zt [n_rows][64], forward only:
 *   a_m = q . tanh(Wc z_m + bc); (w_v, w_t) = softmax(a_v, a_t); c = w_v z_v + w_t z_t; s_m = z_m - c;
 *   p_v = sigmoid(W_ip M + b_ip), p_t = sigmoid(W_tp M + b_tp); d_out = M + (p_v s_v + p_t s_t + c) / 3.
 * d_query: SKR_MGCN_QUERY_FLOATS floats; d_pref_v / d_pref_t: gate blocks.  d_w [n_rows][2] receives (w_v, w_t), or NULL. */
int skr_mgcn_fuse(const float* d_M, const float* d_Zv, const float* d_Zt, const float* d_query, const float* d_pref_v,
                  const float* d_pref_t, int64_t n_rows, int dim, float* d_out, float* d_w, void* stream);
/* One training step, forward and backward, issued on `stream`.  Every pointer is a device pointer except the plans.
 *   F_m = skr_mgcn_project of modality m; X_m = S_m^n_layers (E_items * g_m) (skr_mgcn_purify, n_layers runs of plan_s[m]);
 *   Z_m = [R X_m; X_m] (one run of plan_a); M = mean_{k=0..n_ui_layers} A-hat^k params (2 n_ui_layers runs);
 *   the fuser at the batch's 3 n rows (users, n_users + pos, n_users + neg) only -> out, side;
 *   loss[0] = -mean logsigmoid(<o_u, o_i - o_j>), loss[1] = reg (|o_u|^2 + |o_i|^2 + |o_j|^2) / (2 n),
 *   loss[2] = cl_loss * (InfoNCE(side[pos], M[pos]) + InfoNCE(side[users], M[users])), InfoNCE(a, b) = mean_r [-<a_r, b_r> / 0.2
 *   + log sum_k exp(<a_r, b_k> / 0.2)] over rows normalised with eps 1e-12, all n columns, no [n, n] array in HBM;
 *   loss[3] = their sum                                                                                     WRITTEN
 *   grad (the rows), trs_grad, feat_grad, gate_grad, query_grad, prefer_grad: the gradient of loss[3], every element WRITTEN.
 * A batch row with an id out of range contributes nothing (n stays the divisor).  With n == 0 nothing is launched and NOTHING is
 * written, neither loss nor a gradient (the arguments are still checked).  Bit-reproducible. */
typedef struct skr_mgcn_step_args {
    const skr_spmm_plan* plan_a;       /* R [n_users, n_items], D^-1/2 A D^-1/2 */
    const skr_spmm_plan* plan_at;      /* its transpose */
    const skr_spmm_plan* plan_s[2];    /* S_m [n_items, n_items]; may be NULL if n_layers == 0 */
    const skr_spmm_plan* plan_st[2];   /* their transposes */
    int32_t n_users, n_items, dim, n_ui_layers, n_layers, n;
    int32_t feat_dim[2];
    int32_t feat_ld[2];
    const float* params;               /* [n_users + n_items, 64] */
    const float* trs[2];               /* W [64][feat_ld], then b [64] */
    const float* feat[2];              /* [n_items][feat_ld] */
    const float* gate[2];              /* gate_v, gate_t */
    const float* query;                /* query_common: Wc | bc | q */
    const float* prefer[2];            /* gate_image_prefer, gate_text_prefer */
    const int32_t* users;              /* [n] */
    const int32_t* pos;                /* [n] */
    const int32_t* neg;                /* [n] */
    float reg, cl_loss;
    float* F[2];                       /* [n_items, 64] the projected features */
    float* gate_out[2];                /* [n_items, 64] g_m */
    float* Z[2];                       /* [n_users + n_items, 64] */
    float* M;                          /* [n_users + n_items, 64] */
    float* G[3];                       /* scratch, [n_users + n_items, 64] each: dM, dZv, dZt */
    float* ping[2];                    /* scratch, [n_users + n_items, 64] each */
    float* grad;                       /* [n_users + n_items, 64] */
    float* trs_grad[2];
    float* feat_grad[2];
    float* gate_grad[2];
    float* query_grad;
    float* prefer_grad[2];
    float* loss;                       /* [4] */
    void* work;                        /* skr_mgcn_workspace bytes, 16-byte aligned, no initial contents */
    size_t work_bytes;
} skr_mgcn_step_args;
size_t skr_mgcn_workspace(int n, int n_items, int feat_ld_max);
int skr_mgcn_step(const skr_mgcn_step_args* args, void* stream);
/* The same step with an event after each of its SKR_MGCN_GROUPS launch groups (projections; user-item plan runs; purifier,
 * item-graph runs and R; fuser, BPR, InfoNCE and loss at the batch; the batch backward with its weight gradients, rank and
 * seg_add; the mean's backward chain; the image side's R^T and S^T runs with its purifier and projection backward; the text
 * side's): h_ms[k] (host) = milliseconds of group k; synchronises the stream (timing tools). */
#define SKR_MGCN_GROUPS 8
int skr_mgcn_step_timed(const skr_mgcn_step_args* args, void* stream, float* h_ms);

/* ============================================================================================
 * N -- LATTICE, a learned item graph (csrc/lattice.hip)
 * replaces: _LATTICE.forward / calculate_loss / full_sort_predict and LATTICE.fit's step (recommender/LATTICE.py:203-302,
 * 326-337) at embed_dim, feat_embed_dim <= 64 and cf_model in {lightgcn, mf}, without any dense [I, I] matrix.
 * Tables of 64-float rows, zero beyond dim, 16-byte aligned.  A neighbour list is [n_items][k] (ids int32, values fp32); the
 * four lists of a row are, in this order, the learned image list, the learned text list (ids and cosine similarities of
 * skr_knn_topk on the projected rows) and the frozen image and text lists (columns and values of build_weighted_item_graph's
 * CSR, k entries per row).  The ids of ONE list are distinct; an id outside [0, n_items) is ignored.  An absent list is NULL.
 * No floating-point atomic, every sum in a fixed order: every entry point is bit-reproducible.
 * ============================================================================================ */
#define SKR_LATTICE_MAX_BATCH 2048
#define SKR_LATTICE_MAX_LAYERS 4
#define SKR_LATTICE_CF_LIGHTGCN 0
#define SKR_LATTICE_CF_MF 1
/* The mixed graph S = item_adj (LATTICE.py:209-228) as CSR over the union pattern of the up to four lists of a row, columns
 * ascending, duplicates merged (at most 4 k <= 128 entries per row, merged inside one wavefront):
 *   L_ij = w[0] s_v,ij + w[1] s_t,ij (a missing term is 0);  r_i = sum_j L_ij;  q_i = r_i^-1/2, 0 where r_i <= 0 (the
 *   reference gives 0 at r = 0 and NaN below);  S_ij = (1 - lam) (q_i L_ij) q_j + lam (w[0] O_v,ij + w[1] O_t,ij).
 * d_ids, d_vals: HOST arrays of the four lists' device addresses.  d_w [2] (device): the modal weights; with one modality
 * pass 1 at the present one.
 * WRITTEN: d_rowptr [n_items + 1]; d_col, d_val [4 k n_items] (entries beyond d_rowptr[n_items]: column 0, value 0);
 * d_slots [4 k n_items][4]: the position of the entry in each of the four lists of its row, or -1 (beyond the last entry: -1);
 * d_r, d_q [n_items].  d_work: skr_lattice_graph_workspace bytes, 16-byte aligned. */
size_t skr_lattice_graph_workspace(int n_items);
int skr_lattice_graph(int n_items, int k, const int32_t* const* d_ids, const float* const* d_vals, const float* d_w, double lam,
                      int64_t* d_rowptr, int32_t* d_col, float* d_val, int32_t* d_slots, float* d_r, float* d_q, void* d_work,
                      size_t work_bytes, void* stream);
/* The sampled product over the entries of a CSR pattern: g[e] (+)= sum_{l < n_layers} <A_l[row(e)], B_l[col(e)]> with
 * A_l = d_A + l * stride_a and B_l = d_B + l * stride_b (floats), the layers added in order.  d_row_mask (uint8 [n_rows] or
 * NULL): the rows with a 0 byte are not visited; without `accumulate` their entries are written as zeros. */
int skr_lattice_sddmm(int n_rows, int n_cols, const int64_t* d_rowptr, const int32_t* d_col, const float* d_A, int64_t stride_a,
                      const float* d_B, int64_t stride_b, int n_layers, const uint8_t* d_row_mask, int accumulate, float* d_g,
                      void* stream);
/* The backward of skr_lattice_graph given d_g [nnz] = dLoss/dS: through the surviving similarities, the normalisation and the
 * modal weights, then through the cosine of the projected rows d_F[m] [n_items][64] (NULL: the modality is absent):
 *   a = (1 - lam) g;  t_i = sum_(row i) a L q_j + sum_(column i) a L q_k;  rho_i = -1/2 q_i^3 t_i;  dL_ij = a q_i q_j + rho_i
 *   ds_m = w[m] dL;  dw_m = sum dL s_m + lam sum g O_m;  dF_i += ds_ij (f^_j - s_ij f^_i) / |f_i| and the same at j.
 * The column-side sums are taken by the wavefront of row i of S^T (d_rowptr_t, d_col_t; d_perm_t [nnz]: the entry of S that
 * entry e of S^T is).  WRITTEN: d_dF[m] [n_items][64], every element; d_dw [4] = dw_0, dw_1 and the gradient of the two
 * softmax logits w_m (dw_m - sum_n w_n dw_n).  d_work: skr_lattice_graph_bwd_workspace bytes, 16-byte aligned. */
size_t skr_lattice_graph_bwd_workspace(int n_items, int64_t nnz);
int skr_lattice_graph_bwd(int n_items, int k, int64_t nnz, const float* d_g, const int64_t* d_rowptr, const int32_t* d_col,
                          const int32_t* d_slots, const int64_t* d_rowptr_t, const int32_t* d_col_t, const int32_t* d_perm_t,
                          const int32_t* const* d_ids, const float* const* d_vals, const float* d_w, double lam, const float* d_q,
                          const float* const* d_F, float* const* d_dF, float* d_dw, void* d_work, size_t work_bytes, void* stream);
/* d_out[r] += d_h[r] / max(|d_h[r]|, 1e-12) over n_rows rows of 64 floats: the item rows' + F.normalize(h) of the ranking
 * (LATTICE.py:265, 268). */
int skr_lattice_add_normalized(const float* d_h, int64_t n_rows, float* d_out, void* stream);
/* One training step, forward and backward, issued on `stream`.  Every pointer is a device pointer except the plans.
 *   lightgcn: M = mean_{k=0..n_ui_layers} P^k X_0 with P = D^-1 (A + I) on the square [n_users + n_items] adjacency (plan_p,
 *   the diagonal inside; plan_pt its transpose, whose values differ);  mf: M = X_0;
 *   h = S^n_layers X_0 items (the last run at the batch's item rows only);  item rows: M_i + h_i / max(|h_i|, 1e-12);
 *   loss[0] = -mean logsigmoid(<u, p> - <u, q>), loss[1] = reg (|u|^2 + |p|^2 + |q|^2) / (2 n), loss[2] = their sum   WRITTEN
 *   grad: the gradient of loss[2] with respect to the [n_users + n_items, 64] rows, every element                     WRITTEN
 *   with g_out (a build step): g_out[e] = dLoss/dS_e = sum_l <dh_l[row(e)], h_(l-1)[col(e)]> over the entries of S   WRITTEN
 * Rows with a user or item out of range contribute nothing. */
typedef struct skr_lattice_step_args {
    const skr_spmm_plan* plan_p;       /* P [N, N], N = n_users + n_items; may be NULL with mf or n_ui_layers == 0 */
    const skr_spmm_plan* plan_pt;      /* its transpose */
    const skr_spmm_plan* plan_s;       /* S [n_items, n_items]; may be NULL if n_layers == 0 */
    const skr_spmm_plan* plan_st;      /* its transpose */
    int32_t n_users, n_items, dim, n_ui_layers, n_layers, cf_model, n;
    float reg;
    const float* params;               /* [N, 64] */
    const int32_t* users;              /* [n] */
    const int32_t* pos;                /* [n] */
    const int32_t* neg;                /* [n] */
    float* M;                          /* [N, 64]; not used with mf or n_ui_layers == 0 */
    float* ping[2];                    /* scratch, [N, 64] each */
    float* G;                          /* scratch, [N, 64] */
    float* DH;                         /* scratch, [max(n_layers, 1)][n_items][64]: dh_1 .. dh_n */
    float* H;                          /* with g_out: [n_layers][n_items][64] receives h_0 .. h_(n-1); otherwise not used */
    float* grad;                       /* [N, 64] */
    float* g_out;                      /* [nnz of S] or NULL */
    const int64_t* s_rowptr;           /* with g_out: the CSR pattern of S */
    const int32_t* s_col;
    float* loss;                       /* [3] */
    void* work;                        /* skr_lattice_workspace bytes, 16-byte aligned, no initial contents */
    size_t work_bytes;
} skr_lattice_step_args;
size_t skr_lattice_workspace(int n, int n_items);
int skr_lattice_step(const skr_lattice_step_args* args, void* stream);
/* The same step with an event after each of its SKR_LATTICE_GROUPS launch groups (user-item runs forward; runs of S; batch
 * kernel and loss; clears, rank and ordered adds; user-item runs backward; runs of S^T; the sampled product): h_ms[k] (host) =
 * milliseconds of group k; synchronises the stream (timing tools). */
#define SKR_LATTICE_GROUPS 7
int skr_lattice_step_timed(const skr_lattice_step_args* args, void* stream, float* h_ms);

/* ============================================================================================
 * O -- SLMRec, self-supervised multimedia recommendation (csrc/slmrec.hip; skr_slmrec_project_bwd_w beside the projection
 * backward it shares its kernels with, csrc/mgcn.hip)
 * replaces: _SLMRec.compute / infonce / fac / full_sort_predict and SLMRec.fit's step (recommender/SLMRec.py:132-177, 337-376,
 * 423-432, 559-566) at rec_dim <= 64, ssl_task = "FAC", mm_fusion_mode = "concat", adj_type = "pre", both modalities.
 * Tables of 64-float rows, zero beyond dim, 16-byte aligned; users and items share flat [n_users + n_items, 64] tables, user
 * rows first.  Feature tables and projection blocks are section J's: [n_items][feat_ld] and W [64][feat_ld] | b [64]; modality
 * 0 is the image block (v_dense), 1 the text block (t_dense); the feature tables are CONSTANTS (row-normalised once by the
 * caller) and get no gradient.  A gate block is W [64 out][64 in] | b [64] (SKR_SLMREC_GATE_FLOATS), zero beyond the layer's
 * widths (dim / 2 rows for g_iva_ivat and g_t_ivat).  A fusion block is W [64 out][192 in] | b [64]
 * (SKR_SLMREC_FUSION_FLOATS): input column 64 t + c is column c of table t (Mi, Mv, Mt), the reference's column t dim + c.
 * The fusion runs on v_mfma_f32_16x16x4_f32; the five chain layers, the three log-sum-exp products and every backward product
 * add the same fp32 operands on v_mfma_f64_16x16x4_f64 and round once, as section M's do.  No floating-point atomic, every sum
 * in a fixed order: all entries are bit-reproducible.
 * ========================================================================================== */
#define SKR_SLMREC_MAX_BATCH 2048
#define SKR_SLMREC_MAX_LAYERS 4
#define SKR_SLMREC_MAX_FEAT 4096
#define SKR_SLMREC_GATE_FLOATS (64 * 64 + 64)
#define SKR_SLMREC_FUSION_FLOATS (64 * 192 + 64)
/* The weight part of skr_mgcn_project_bwd alone, by the same kernels and bit for bit the same values: d_dtrs = dW [64][feat_ld]
 * = dF^T X, then db [64] = the column sums of dF, EVERY element WRITTEN; dX is not formed (the feature table is a constant:
 * at 100 k items of 4 096 columns it would be a 1.6 GB write per step).  d_work: skr_mgcn_project_bwd_workspace bytes. */
int skr_slmrec_project_bwd_w(const float* d_dF, const float* d_X, int n_rows, int feat_dim, int feat_ld, float* d_dtrs,
                             void* d_work, size_t work_bytes, void* stream);
/* The fusion over all rows of one side (SLMRec.py:174-175), row-local: d_out[r] = W [Mi_r | Mv_r | Mt_r] + b over n_rows rows
 * of d_Mi, d_Mv, d_Mt [n_rows][64]; d_fusion: a fusion block in HBM, staged through LDS.  For the ranking only. */
int skr_slmrec_fuse(const float* d_Mi, const float* d_Mv, const float* d_Mt, const float* d_fusion, int64_t n_rows, int dim,
                    float* d_out, void* stream);
/* One training step, forward and backward, issued on `stream`.  Every pointer is a device pointer except the plans.
 *   D_m = skr_mgcn_project of modality m; M[0] = P([E_u; E_i]), M[1] = P([E_u; D_0]), M[2] = P([E_u; D_1]) with
 *   P(x) = mean_{k=0..n_layers} A^k x (2 n_layers plan runs per table, the mean in the accum epilogue); A is symmetric:
 *   plan_a is its user x item block, plan_at that block's transpose;
 *   at the batch's n rows only: user = fusion_user [M[t][users]], item = fusion_item [M[t][n_users + pos]];
 *   x = g_i_iv(M[0] item row), y = g_v_iv(M[1] item row), z = g_iva_ivat(g_iv_iva(x)), w = g_t_ivat(M[2] item row);
 *   CE(a, b, tau) = mean_r [log sum_k exp(<a_r, b_k> / tau) - <a_r, b_r> / tau], the running maximum subtracted, all n columns,
 *   no [n, n] array in HBM;
 *   loss[0] = CE(user / max(|user|, 1e-12), item / max(|item|, 1e-12), temp), loss[1] = ssl_alpha CE(x, y, ssl_temp),
 *   loss[2] = ssl_alpha CE(z, w, ssl_temp), loss[3] = their sum                                                     WRITTEN
 *   grad (the rows), dense_grad, fusion_*_grad, chain_grad: the gradient of loss[3], every element                  WRITTEN
 *   M[0..2] keep the three propagated tables (the ranking fuses them with skr_slmrec_fuse).
 * A batch row with an id out of range contributes nothing (n stays the divisor).  With n == 0 nothing is launched and NOTHING is
 * written, neither loss nor a gradient (the arguments are still checked).  Bit-reproducible. */
typedef struct skr_slmrec_step_args {
    const skr_spmm_plan* plan_a;       /* the user x item block of the 'pre' adjacency */
    const skr_spmm_plan* plan_at;      /* its transpose */
    int32_t n_users, n_items, dim, n_layers, n;
    int32_t feat_dim[2];
    int32_t feat_ld[2];
    float temp, ssl_temp, ssl_alpha;
    const float* params;               /* [n_users + n_items, 64] */
    const float* dense[2];             /* v_dense, t_dense: W [64][feat_ld], then b [64] */
    const float* feat[2];              /* [n_items][feat_ld], constants */
    const float* fusion_user;          /* embedding_user_after_GCN: a fusion block */
    const float* fusion_item;          /* embedding_item_after_GCN */
    const float* chain[5];             /* gate blocks: g_i_iv, g_v_iv, g_iv_iva, g_iva_ivat, g_t_ivat */
    const int32_t* users;              /* [n] */
    const int32_t* pos;                /* [n] */
    float* D[2];                       /* [n_items, 64] the projected features */
    float* M[3];                       /* [n_users + n_items, 64] */
    float* G[3];                       /* scratch, [n_users + n_items, 64] each */
    float* ping[2];                    /* scratch, [n_users + n_items, 64] each */
    float* dD;                         /* scratch, [n_items, 64] */
    float* grad;                       /* [n_users + n_items, 64] */
    float* dense_grad[2];
    float* fusion_user_grad;
    float* fusion_item_grad;
    float* chain_grad[5];
    float* loss;                       /* [4] */
    void* work;                        /* skr_slmrec_workspace bytes, 16-byte aligned, no initial contents */
    size_t work_bytes;
} skr_slmrec_step_args;
size_t skr_slmrec_workspace(int n, int n_items, int feat_ld_max);
int skr_slmrec_step(const skr_slmrec_step_args* args, void* stream);
/* The same step with an event after each of its SKR_SLMREC_GROUPS launch groups (projections; the 6 n_layers plan runs of the
 * forward; the batch forward: fusion, chain, norms, log-sum-exp, loss; the batch backward with its weight gradients; clears,
 * rank and ordered adds; the backward chain of M[0]; that of M[1] with v_dense's weight gradient; that of M[2] with t_dense's):
 * h_ms[k] (host) = milliseconds of group k; synchronises the stream (timing tools). */
#define SKR_SLMREC_GROUPS 8
int skr_slmrec_step_timed(const skr_slmrec_step_args* args, void* stream, float* h_ms);

/* ============================================================================================
 * Caser -- convolutional sequence embedding (csrc/caser.hip)
 * replaces: _Caser._forward_user / forward / predict and Caser.fit's step (recommender/Caser.py:118-162,191-207).
 * Rows are 64 floats (dim must be 64; `width` <= 64 is the model's embed_size: narrower embeddings are zero-padded by the
 * caller, and the vertical filters' outputs beyond `width` are held at zero).  Tables: d_U [n_users, 64]; d_E
 * (item_embeddings) [n_rows, 64]; d_W2 [n_rows, 128], a row being the z half then the p half, each zero beyond width;
 * d_b2 [n_rows]; n_rows = items + 1.  pad_idx names a padding row that reads as zeros in a window and never receives a
 * gradient, in d_E, d_W2 and d_b2 alike; -1: no such row (the reference builds its tables without padding_idx,
 * Caser.py:179, so its padding item is an ordinary row: skrec/recommender/Caser.py passes -1).
 * d_shared: the shared parameters, SKR_CASER_SHARED_FLOATS(L, nv, nh) floats, 16-byte aligned, every part on a 64-float
 * boundary and zero where padded:
 *   conv_v.weight [nv][L] (64 floats) | conv_v.bias [nv] (64 floats) |
 *   the horizontal filters, SKR_CASER_ROWS(L, nh) rows of 64 floats: for h = 1..L, for k < nh, for r < h the row
 *     conv_h[h-1].weight[k, 0, r, :] -- row nh h (h - 1) / 2 + k h + r |
 *   conv_h[h-1].bias[k] at (h - 1) nh + k, L nh floats rounded up to a multiple of 64 |
 *   fc1.weight [64][Fp]: row j (an output), column c 64 + col for the vertical filter c's column col, column nv 64 + (h - 1) nh + k
 *     for the horizontal filter (h, k); Fp = SKR_CASER_FP(L, nv, nh), the nv 64 + nh L columns rounded up to a multiple of 64 |
 *   fc1.bias [64]
 * Per instance (u, window s_1..s_L, positives t_1..t_T, negatives t_T+1..t_2T), with E_l = E[s_l] and p = U[u]:
 *   out_v[c] = bv[c] + sum_l wv[c][l] E_l,   a[h,k,t] = bh[h,k] + sum_{r<h} <Wh[h,k,r], E_(t+r)>,   out_h[h,k] = max_t relu(a[h,k,t]),
 *   out = dropout([out_v, out_h]),   z = relu(W1 out + b1),   x = [z, p],   y_j = <W2[t_j], x> + b2[t_j].
 * max takes the lowest position among exact ties and relu'(0) = 0, as torch's max_pool1d and relu do.
 * Limits (refused with a message): width <= 64, 1 <= seq_L <= SKR_CASER_MAX_L, 1 <= seq_T <= SKR_CASER_MAX_T,
 * 1 <= nv <= SKR_CASER_MAX_NV, 1 <= nh <= SKR_CASER_MAX_NH, n <= SKR_CASER_MAX_BATCH.
 * ========================================================================================== */
#define SKR_CASER_MAX_L 8
#define SKR_CASER_MAX_T 16
#define SKR_CASER_MAX_NV 8
#define SKR_CASER_MAX_NH 32
#define SKR_CASER_MAX_BATCH 2048
#define SKR_CASER_ROWS(L, nh) ((nh) * (L) * ((L) + 1) / 2)
#define SKR_CASER_FP(L, nv, nh) (64 * (((nv) * 64 + (nh) * (L) + 63) / 64))
#define SKR_CASER_SHARED_FLOATS(L, nv, nh) \
    (128 + 64 * SKR_CASER_ROWS(L, nh) + 64 * (((L) * (nh) + 63) / 64) + 64 * SKR_CASER_FP(L, nv, nh) + 64)
/* bytes of d_work for a batch of n instances (and for skr_caser_queries, which walks its users through it in chunks); 0 for
 * arguments out of range */
size_t skr_caser_workspace(int n, int seq_L, int nv, int nh);
/* One training batch, forward and backward of mean over n seq_T of (bce(y_pos, 1) + bce(y_neg, 0)): d_u int32[n], d_seq
 * int32[n][seq_L], d_pos / d_neg int32[n][seq_T].  The batch's two cross-entropy SUMS are WRITTEN to words 0 and 1 of d_loss
 * (float [2 * loss_slots], loss_slots 1 or SKR_LOSS_SLOTS; the other slots' words are written as zeros).  The gradients are
 * ADDED to d_gU, d_gE, d_gW2, d_gb2 and d_gshared, in the tables' layouts (the caller's optimiser zeroes them).  Dropout at
 * rate `dropout` (0: keeps everything and draws nothing): d_keep holds one byte per [n, nv width + nh seq_L] element in the
 * reference's column order (c width + col, then (h - 1) nh + k); NULL: the step draws on the device, keyed by (seed, step,
 * user, column) -- a user's draws do not depend on the rest of the batch; equal to torch's draws in law only.  d_keep_out
 * (optional, same shape) records the flags that were used.  An instance with an id outside [0, n_users) / [0, n_rows) is
 * skipped: it adds nothing to the sums or the gradients (the mean still divides by n seq_T) and its ids are not
 * dereferenced.  No floating-point atomic: row gradients are added once per distinct id in rank order, the shared
 * parameters' in a fixed order, so two calls on the same inputs give the same bits.  d_work: skr_caser_workspace(n, ...)
 * bytes, 16-byte aligned, no initial contents, not to be shared by calls that may run at the same time. */
int skr_caser_step(const float* d_U, const float* d_E, const float* d_W2, const float* d_b2, const float* d_shared, const int32_t* d_u,
                   const int32_t* d_seq, const int32_t* d_pos, const int32_t* d_neg, int n, int n_users, int n_rows, int pad_idx, int dim,
                   int width, int seq_L, int seq_T, int nv, int nh, float dropout, const uint8_t* d_keep, uint8_t* d_keep_out,
                   uint64_t seed, uint64_t step, float* d_gU, float* d_gE, float* d_gW2, float* d_gb2, float* d_gshared, void* d_work,
                   size_t work_bytes, float* d_loss, int loss_slots, void* stream);
/* The same step with an event after each of its SKR_CASER_LAUNCHES launch groups (conv; fc1; scores and loss terms; d_out = dz W1;
 * dW1 | db1; conv backward; filter gradients; rank; ordered adds; loss sums): h_ms[k] (host) = milliseconds of group k;
 * synchronises the stream (timing tools). */
#define SKR_CASER_LAUNCHES 10
int skr_caser_step_timed(const float* d_U, const float* d_E, const float* d_W2, const float* d_b2, const float* d_shared,
                         const int32_t* d_u, const int32_t* d_seq, const int32_t* d_pos, const int32_t* d_neg, int n, int n_users,
                         int n_rows, int pad_idx, int dim, int width, int seq_L, int seq_T, int nv, int nh, float dropout,
                         const uint8_t* d_keep, uint8_t* d_keep_out, uint64_t seed, uint64_t step, float* d_gU, float* d_gE, float* d_gW2,
                         float* d_gb2, float* d_gshared, void* d_work, size_t work_bytes, float* d_loss, int loss_slots, void* stream,
                         float* h_ms);
/* Query rows: d_Q[u][0..127] = x = [z, p] of user u = d_users[i] (d_users NULL: u = i) in eval mode (no dropout) from the
 * window d_windows[i][0..seq_L), so that the model's score of item t is <d_Q[u], W2[t]> + b2[t] (skr_score_matrix at
 * dim = 128).  A window with an entry outside [0, n_rows) -- by convention a negative first entry marks a user without training
 * history -- gives a row of NaN (callers raise before they ask: the reference raises KeyError, Caser.py:223).  Users out of
 * range are skipped.  d_work: at least 64 (4 SKR_CASER_FP + 4) + 16 bytes; skr_caser_workspace of any batch is enough. */
int skr_caser_queries(const float* d_U, const float* d_E, const float* d_shared, const int32_t* d_users, int n, const int32_t* d_windows,
                      int n_users, int n_rows, int pad_idx, int dim, int width, int seq_L, int nv, int nh, void* d_work,
                      size_t work_bytes, float* d_Q, void* stream);

/* ============================================================================================
 * SASRec -- self-attentive sequential recommendation (csrc/sasrec.hip)
 * replaces: the TensorFlow graph of recommender/SASRec.py:60-87 (normalize), :174-269 (multihead_attention), :272-308
 * (feedforward), :387-463 (_build_model) and the session runs of fit / predict (:465-498).
 * Rows are 64 floats; `hidden` <= 64 is the model's hidden_units: narrower rows are zero-padded by the caller and the padded
 * columns take no part in LayerNorm, receive no gradient and stay zero.  Tables: d_E (item_embeddings) [n_items + 1, 64], whose
 * row n_items is the padding item: it is never read (a padded position is a row of zeros) and never receives a gradient;
 * d_P (position_embeddings) [max_len, 64].
 * d_shared: every other parameter, SKR_SASREC_SHARED_FLOATS(blocks) floats, 16-byte aligned, in rows of 64 floats, zero where
 * padded.  A dense kernel of the reference, [in, out], is stored TRANSPOSED, row o holding the weights of output o.  Per block,
 * SKR_SASREC_BLOCK_ROWS rows:
 *   ln1_gamma | ln1_beta | Wq^T [64 rows] | bq | Wk^T [64] | bk | Wv^T [64] | bv | ln2_gamma | ln2_beta | W1^T [64] | b1 |
 *   W2^T [64] | b2
 * and behind the last block: ln_out_gamma | ln_out_beta.
 * Per sequence (seq, pos, neg: int32 [max_len] each, left-padded with n_items), with m[t] = (seq[t] != n_items):
 *   x = m dropout(sqrt(hidden) E[seq] + P);  per block:  q = LN1(x), Q = q Wq + bq, K = x Wk + bk, V = x Wv + bv, per head
 *   A = dropout(softmax over the keys j <= t with m[j] of Q_h K_h^T / sqrt(hidden / heads)), y = concat_h(A V_h) + q,
 *   f = LN2(y), x = m (dropout(dropout(relu(f W1 + b1)) W2 + b2) + f);  out = LN_out(x);
 *   loss = sum over t with pos[t] != n_items of -log(sigmoid(y_pos) + 1e-24) - log(sigmoid(-y_neg) + 1e-24), over their number,
 *   y_pos = sqrt(hidden) <out[t], E[pos[t]]>, y_neg likewise (0 for neg[t] == n_items).
 * LN is the reference's normalize: (x - mean) / sqrt(var + 1e-8) gamma + beta, biased variance.  Rows with m = 0 are skipped
 * as queries and as keys (the reference masks a key by a row sum of exactly 0, and evaluates 1 - sigmoid(x) where this takes
 * sigmoid(-x): DESIGN.md names both deviations).
 * Keep flags: one byte per element, per sequence SKR_SASREC_KEEP_BYTES(hidden, max_len, blocks, heads) bytes in this order:
 *   the input [max_len][hidden] | per block: the attention weights [heads][max_len][max_len] (query, then key) |
 *   the first feed-forward site [max_len][hidden] | the second [max_len][hidden]
 * Limits (refused with a message): hidden <= SKR_SASREC_MAX_HIDDEN, max_len <= SKR_SASREC_MAX_LEN, blocks <=
 * SKR_SASREC_MAX_BLOCKS, heads <= SKR_SASREC_MAX_HEADS and dividing hidden, n <= SKR_SASREC_MAX_BATCH.
 * ========================================================================================== */
#define SKR_SASREC_MAX_HIDDEN 64
#define SKR_SASREC_MAX_LEN 64
#define SKR_SASREC_MAX_BLOCKS 4
#define SKR_SASREC_MAX_HEADS 8
#define SKR_SASREC_MAX_BATCH 2048
#define SKR_SASREC_WORKGROUPS 256 /* the step's persistent workgroups: sequence b belongs to workgroup b mod this */
#define SKR_SASREC_BLOCK_ROWS 329
#define SKR_SASREC_SHARED_FLOATS(blocks) (64 * (SKR_SASREC_BLOCK_ROWS * (blocks) + 2))
#define SKR_SASREC_KEEP_BYTES(hidden, max_len, blocks, heads) \
    ((max_len) * (hidden) + (blocks) * ((heads) * (max_len) * (max_len) + 2 * (max_len) * (hidden)))
/* bytes of d_work for batches of at most n_max sequences; 0 for arguments out of range */
int64_t skr_sasrec_workspace(int n_max, int max_len, int blocks, int heads);
/* One training batch, forward and backward: d_seq, d_pos, d_neg int32 [n][max_len].  The mean loss is WRITTEN to word 0 of
 * d_loss (float [2 * loss_slots], loss_slots 1 or SKR_LOSS_SLOTS) and every other word is written as zero: word 1 is the l2
 * term's, which the caller fills in (SASRec.py adds l2_emb w to the two tables' gradients itself).  The gradients are ADDED to
 * d_gE, d_gP and d_gshared, in the tables' layouts.  Dropout at `rate` (0: keeps everything and draws nothing): d_keep holds
 * the flags of the n sequences in the layout above; NULL: the step draws on the device, keyed by (seed, step, the sequence's
 * number in the batch, the element's offset in the layout), so that the backward draws them again; equal to TensorFlow's draws
 * in law only.  d_keep_out (optional, same shape) records the flag of every element, used or not.  A sequence with an id
 * outside [0, n_items] adds nothing to the sum or the gradients (its targets still count in the divisor) and its ids are not
 * dereferenced.  A batch without any target gives loss 0 and zero gradients (unreachable through fit(): every training row
 * holds a target).  No floating-point atomic: a workgroup adds its sequences' weight gradients in sequence order, the
 * workgroups' sums are added in workgroup order, the position rows in batch order and the item rows once per distinct id of
 * seq || pos || neg in ascending list position, so two calls on the same inputs give the same bits.  d_work:
 * skr_sasrec_workspace(n, ...) bytes, 16-byte aligned, no initial contents, not to be shared by calls that may run at the
 * same time. */
int skr_sasrec_step(const float* d_E, const float* d_P, const float* d_shared, const int32_t* d_seq, const int32_t* d_pos,
                    const int32_t* d_neg, int n, int n_items, int hidden, int max_len, int blocks, int heads, float rate,
                    const uint8_t* d_keep, uint8_t* d_keep_out, uint64_t seed, uint64_t step, float* d_gE, float* d_gP, float* d_gshared,
                    void* d_work, size_t work_bytes, float* d_loss, int loss_slots, void* stream);
/* The same step with an event after each of its SKR_SASREC_LAUNCHES launch groups (the fused forward-loss-backward; the slabs'
 * sum; the position rows; rank; ordered adds; loss): h_ms[k] (host) = milliseconds of group k; synchronises the stream. */
#define SKR_SASREC_LAUNCHES 6
int skr_sasrec_step_timed(const float* d_E, const float* d_P, const float* d_shared, const int32_t* d_seq, const int32_t* d_pos,
                          const int32_t* d_neg, int n, int n_items, int hidden, int max_len, int blocks, int heads, float rate,
                          const uint8_t* d_keep, uint8_t* d_keep_out, uint64_t seed, uint64_t step, float* d_gE, float* d_gP,
                          float* d_gshared, void* d_work, size_t work_bytes, float* d_loss, int loss_slots, void* stream, float* h_ms);
/* Query rows: d_Q[i][0..63] = sqrt(hidden) out[max_len - 1] of user u = d_users[i] (d_users NULL: u = i), the forward without
 * dropout over the window d_windows[u][0..max_len) of the [n_users, max_len] table, so that the model's score of item t is
 * <d_Q[i], E[t]> on the raw parameter rows.  An all-padding window gives sqrt(hidden) ln_out_beta, as the reference does; an
 * id outside [0, n_items] reads as padding; a user out of range is skipped.  The last block runs for the 16-row tile of the
 * last position alone. */
int skr_sasrec_queries(const float* d_E, const float* d_P, const float* d_shared, const int32_t* d_users, int n, const int32_t* d_windows,
                       int n_users, int n_items, int hidden, int max_len, int blocks, int heads, float* d_Q, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SKREC_HIP_H */
