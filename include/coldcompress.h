/*
 * coldcompress.h — C ABI of the MI355X-native KV-cache eviction + pruned-cache attention path.
 *
 * This is the drop-in boundary.  The reference (AnswerDotAI/cold-compress) has no
 * FFI of its own: its boundary is the Python class surface in cache.py / attention_utils.py /
 * prompt_compression.py.  The Python mirror of that surface lives in cold_compress_amd/ and reaches the
 * device ONLY through the entry points declared here (ctypes, see cold_compress_amd/_abi.py and
 * INTEGRATION.md).  Each entry point cites the reference code it replaces as
 * "ref: <file>:<lines>" (paths relative to the reference checkout).
 *
 * Conventions
 *  - Every pointer is a DEVICE pointer (HBM) unless stated otherwise.  Batch is 1 (ref: model.py:188-189).
 *  - `stream` is a hipStream_t passed as void*.  No entry point synchronises the stream, allocates or
 *    frees memory; scratch is supplied by the caller (torch's caching allocator) and sized by the
 *    matching *_workspace_bytes() query.  All entry points are hipGraph-capturable.
 *  - Return value: CC_OK (0) or a negative CC_ERR_* code.  Nothing throws.
 *  - `input_pos` for decode is a device int32[1] (the reference's decode `input_pos` tensor,
 *    generation_utils.py:482) so that captured graphs replay with an advancing position.
 *  - Arg-min rule everywhere: lowest slot index wins ties, NaN counts as the minimum (torch.argmin).
 *  - dtype codes: element type of K/V/q/probabilities ("model dtype" in the reference).
 *
 * The CPU oracle (oracle/cc_oracle.c) exports the same functions with a `_cpu` suffix and identical
 * signatures taking HOST pointers; it is test infrastructure only.
 */
#ifndef COLDCOMPRESS_H
#define COLDCOMPRESS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CC_ABI_VERSION 1

#define CC_OK 0
#define CC_ERR_BAD_ARG (-1)      /* null pointer / non-positive size / inconsistent shape           */
#define CC_ERR_UNSUPPORTED (-2)  /* dtype / head_dim / window size the kernels are not built for     */
#define CC_ERR_HIP (-3)          /* hipGetLastError() != hipSuccess after a launch                   */
#define CC_ERR_WORKSPACE (-4)    /* workspace too small                                              */

#define CC_DT_F32 0
#define CC_DT_BF16 1
#define CC_DT_F16 2

/* priority dtypes for cc_topk_keep (prompt compaction) */
#define CC_PRIO_F32 0
#define CC_PRIO_BF16 1
#define CC_PRIO_F16 2
#define CC_PRIO_I64 3

typedef void* cc_stream_t;

/* View of one layer's cache buffers; mirrors the nn.Module buffers of ref: cache.py:178-227.
 *   k_cache, v_cache : [H, S, D] model dtype           (cache.py:185-201)
 *   pos              : [Hp, S] int32, -1 = empty slot; Hp = H if head_specific else 1 (cache.py:207-218)
 *   mask             : [H, S] bool (1 byte)            (cache.py:226-227)
 *   cache_cts        : [Hc] int32; Hc = H if variable_length else 1 (cache.py:219-222)
 */
typedef struct cc_kv_view {
  void* k_cache;
  void* v_cache;
  int32_t* pos;
  uint8_t* mask;
  int32_t* cache_cts;
  int32_t H;
  int32_t Hp;
  int32_t Hc;
  int32_t S;
  int32_t D;
  int32_t dtype;
} cc_kv_view;

int cc_abi_version(void);
const char* cc_error_string(int code);
/* Device properties of the current HIP device (host ints out); used by bench.py / DESIGN numbers. */
int cc_device_info(int* n_cu, int* wave_size, int* lds_bytes_per_cu, char* name, int name_len);

/* ------------------------------------------------------------------------------------------------
 * Decode-time update_kv: choose the slot to overwrite, then insert the new token in place.
 * ref: KVCache.update_kv cache.py:314-340 -> _decoding_update :348-364 -> _eviction_idx + _fill.
 *
 * Common behaviour (Appendix A of SURVEY.md):
 *   idx[h] chosen per policy; num_ins[h] = (pos[h or 0][idx]== -1); then
 *   pos[.,idx] <- *input_pos; K[h,idx,:] <- k_new[h,:]; V likewise; mask[h,idx] <- 1;
 *   cache_cts[j] += num_ins[j] for j < Hc                     (cache.py:330, 356-362, 390-401, 460-490)
 * k_new/v_new: [H, D] model dtype.  idx_out: int64 [Hp] (what _eviction_idx returns).
 * If k_new == NULL the call is "select only": idx_out is produced (plus the policy's own side effects,
 * e.g. heavy-hitter history zeroing, which the reference performs inside _eviction_idx) and nothing is
 * inserted.
 * ---------------------------------------------------------------------------------------------- */

/* ref: KVCacheFull._eviction_idx cache.py:500-502 — argmin over pos (first empty slot). Hp must be 1. */
int cc_decode_update_full(const cc_kv_view* c, const void* k_new, const void* v_new,
                          const int32_t* input_pos, int64_t* idx_out, cc_stream_t stream);

/* ref: KVCacheRecentGlobal._eviction_idx cache.py:552-556 — g + argmin(pos[g:]). Hp must be 1. */
int cc_decode_update_recent_global(const cc_kv_view* c, const void* k_new, const void* v_new,
                                   const int32_t* input_pos, int32_t global_tokens, int64_t* idx_out,
                                   cc_stream_t stream);

/* Generic base path for caller-supplied importances.
 * ref: KVCache._eviction_idx cache.py:366-379 — scores[:, :g]=+inf; pos==-1 -> -inf; argmin.
 * scores: [Hs, S] of score_dtype (CC_DT_*), Hs = Hp or 1 (a 1-D score vector is broadcast like
 * scores.unsqueeze(0), cache.py:369-370, and then Hp must be 1).  Scores are NOT modified. */
int cc_decode_update_scores(const cc_kv_view* c, const void* k_new, const void* v_new,
                            const int32_t* input_pos, const void* scores, int32_t score_dtype,
                            int32_t global_tokens, int64_t* idx_out, cc_stream_t stream);

/* ref: KVCacheRandom._token_importances cache.py:519-524 + base _eviction_idx :366-379.
 * rand_u: [S] f32 uniform [0,1) drawn by the caller (the RNG stream is backend-specific; parity is
 * defined given this vector).  pos[s] >= *input_pos - recent_window -> +inf. Hp must be 1. */
int cc_decode_update_random(const cc_kv_view* c, const void* k_new, const void* v_new,
                            const int32_t* input_pos, const float* rand_u, int32_t global_tokens,
                            int32_t recent_window, int64_t* idx_out, cc_stream_t stream);

/* ref: KVCacheL2 cache.py:580-605 — score = dtype(max(key_norm) - key_norm) with the max taken over
 * ALL heads and slots, recent window -> +inf, then base rules; on insert key_norm[h,idx] <- ||k_new[h]||2
 * (fp32 accumulate, rounded to model dtype).  key_norm: [H, S] model dtype.  Hp must be H.
 * workspace: cc_decode_update_l2_workspace_bytes(H,S) bytes. */
size_t cc_decode_update_l2_workspace_bytes(int32_t H, int32_t S);
int cc_decode_update_l2(const cc_kv_view* c, const void* k_new, const void* v_new,
                        const int32_t* input_pos, void* key_norm, int32_t global_tokens,
                        int32_t recent_window, int64_t* idx_out, void* workspace, size_t workspace_bytes,
                        cc_stream_t stream);

/* ref: KVCacheHeavyHitter._eviction_idx cache.py:725-765 (history_window_size W == 1, float64 history).
 *   avg = f32(num) / f32(max(denom,1));  (pos<g)|(pos>=p-w) -> 1.0;  pos==-1 -> 0.0;  argmin;
 *   num[h,idx] <- 0; denom[h,idx] <- 0; then the common insert.
 * num: [H, S] float64; denom: [H, S] int32.  Hp must be H. */
int cc_decode_update_heavy_hitter(const cc_kv_view* c, const void* k_new, const void* v_new,
                                  const int32_t* input_pos, double* num, int32_t* denom,
                                  int32_t global_tokens, int32_t recent_window, int64_t* idx_out,
                                  cc_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Heavy-hitter history update.  ref: KVCacheHeavyHitter.update_state cache.py:690-723 (W == 1).
 *   num[h,s] += (double)attn[h,s] for s < T (zero padding to S beyond T); denom[h,s] += 1 for ALL s;
 *   *counter += 1.  attn: [H, T] model dtype, already averaged over the query group.
 * ---------------------------------------------------------------------------------------------- */
int cc_hh_update(double* num, int32_t* denom, int64_t* counter, const void* attn, int32_t H, int32_t S,
                 int32_t T, int32_t dtype, cc_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Decode attention over the pruned cache, GQA-aware (K/V read once, no repeat_interleave).
 * ref: model.py:395-418 + attention_utils.py:27-54.
 *   q: [HQ, D]; k,v: [H, S, D]; mask: [H, S] bool or NULL; R = HQ/H; query head j uses kv head j/R.
 *   score = dtype(dtype(q.k) * scale) (+ -inf where mask==0); P = dtype(softmax_fp32(score));
 *   y[HQ, D] = dtype(sum_s P*v);  probs_out[HQ, S] = P (optional, may be NULL);
 *   attn_out[H, S] = dtype(mean over the R heads of the group of P) (optional, may be NULL).
 * For CC_DT_F32 the "dtype()" roundings are identities.
 * If hh_num != NULL the heavy-hitter history update (cc_hh_update with T = S) is fused into the
 * combine pass: hh_num += attn_out, hh_denom += 1, *hh_counter += 1.
 * ---------------------------------------------------------------------------------------------- */
size_t cc_decode_attn_workspace_bytes(int32_t HQ, int32_t H, int32_t S, int32_t D, int32_t dtype);
int cc_decode_attn_gqa(const void* q, const void* k, const void* v, const uint8_t* mask, int32_t HQ,
                       int32_t H, int32_t S, int32_t D, int32_t dtype, float scale, void* y,
                       void* attn_out, void* probs_out, double* hh_num, int32_t* hh_denom,
                       int64_t* hh_counter, void* workspace, size_t workspace_bytes,
                       cc_stream_t stream);

/* The same attention with the W > 1 history ring folded into the combine pass (cf. hh_num/hh_denom/hh_counter above,
 * which fold the W == 1 history): ring[h, s, *counter % W] = group-mean attention; denom += 1; *counter += 1
 * (ref: cache.py:716-723), and the tracked window-sum state (wsum_acc / wsum, see cc_hh_ring_update) kept current.
 * Equivalent to cc_decode_attn_gqa(attn_out) followed by cc_hh_ring_update(attn = attn_out, T = S, tracked). */
int cc_decode_attn_gqa_ring(const void* q, const void* k, const void* v, const uint8_t* mask, int32_t HQ, int32_t H,
                            int32_t S, int32_t D, int32_t dtype, float scale, void* y, void* attn_out, void* ring_num,
                            int32_t* denom, int64_t* counter, int32_t W, uint64_t* wsum_acc, float* wsum,
                            void* workspace, size_t workspace_bytes, cc_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Fused heavy-hitter decode step (history_window_size == 1): update_kv + attention + update_state of one layer
 * in TWO launches instead of three.  Same reference lines as cc_decode_update_heavy_hitter, cc_decode_attn_gqa
 * and cc_hh_update; the only difference is WHEN the arg-min runs:
 *   launch 1 (K/V streaming pass): the insert of this step's token is folded into its prologue — the slot is the
 *     minimum over the partial arg-min keys next_key[h][0 .. NK) left by the previous step (or by
 *     cc_hh_next_key_init);
 *   launch 2 (combine): y, group-averaged probabilities, history update, and the arg-min for position
 *     *input_pos + 1 evaluated on the freshly updated history: one partial minimum per 128-slot chunk
 *     -> next_key[h][chunk] (plain stores; no atomics, no reset pass).
 * next_key: uint64 [H, NK], NK = cc_hh_next_key_slots(S) = the row stride: eight LIVE entries per 128-slot chunk (the combine pass
 * fills the first eighth of them and keeps the others at ~0; the single-launch step below publishes one key per WAVE of its
 * 64-slot workgroups, so that no wave waits for another at the end of the launch) plus, r6, a TAIL of eight entries no arg-min
 * ever reads (reserved, unread);
 * entry = (orderable(score) << 32) | slot << 1 | was_empty, ~0 = "no candidate".  Valid as long as positions advance by one and nothing else mutates pos / history in
 * between; re-seed with cc_hh_next_key_init otherwise.
 * Results are bit-identical to the three-call sequence (tests/test_gpu_fused_step.py).
 * ---------------------------------------------------------------------------------------------- */
int32_t cc_hh_next_key_slots(int32_t S);
int cc_hh_next_key_init(const cc_kv_view* c, const int32_t* input_pos, const double* num, const int32_t* denom,
                        int32_t global_tokens, int32_t recent_window, uint64_t* next_key, cc_stream_t stream);
int cc_decode_step_heavy_hitter(const cc_kv_view* c, const void* q, const void* k_new, const void* v_new,
                                const int32_t* input_pos, double* num, int32_t* denom, int64_t* counter,
                                uint64_t* next_key, int32_t global_tokens, int32_t recent_window, int32_t HQ,
                                float scale, void* y, void* attn_out, void* workspace, size_t workspace_bytes,
                                cc_stream_t stream);
/* The same two-launch step for the head-constant ring policies: KVCacheRecentGlobal (cache.py:527-556: arg-min of
 * pos over the slots behind the first `global_tokens` sinks; empty slots, pos == -1, first) and KVCacheFull
 * (cache.py:493-502: global_tokens = 0).  c->Hp must be 1; next_key: uint64 [H, NK] — one row per kv head, all holding the same
 * keys: every head reads and rewrites its own copy, so that no workgroup of one head can read a row another head's workgroups
 * have already rewritten for the next position (the single-launch form has no launch boundary between the two).  No history,
 * no group-mean output. */
int cc_rg_next_key_init(const cc_kv_view* c, const int32_t* input_pos, int32_t global_tokens, uint64_t* next_key,
                        cc_stream_t stream);
int cc_decode_step_recent_global(const cc_kv_view* c, const void* q, const void* k_new, const void* v_new,
                                 const int32_t* input_pos, uint64_t* next_key, int32_t global_tokens, int32_t HQ,
                                 float scale, void* y, void* workspace, size_t workspace_bytes, cc_stream_t stream);
/* The same two-launch step for KVCacheRandom (cache.py:505-524: uniform scores, the `recent_window` newest positions
 * -> +inf, then the base rules cache.py:373-376).  `rand_u` / `rand_next`: float32 [S] uniform draws — the init call takes
 * the draw for position *input_pos, every step the draw for position *input_pos + 1 (the reference draws one vector
 * per step, cache.py:521; the order of draws is unchanged).  c->Hp must be 1; next_key: uint64 [H, NK] (as cc_decode_step_recent_global). */
int cc_random_next_key_init(const cc_kv_view* c, const int32_t* input_pos, const float* rand_u, int32_t global_tokens,
                            int32_t recent_window, uint64_t* next_key, cc_stream_t stream);
int cc_decode_step_random(const cc_kv_view* c, const void* q, const void* k_new, const void* v_new,
                          const int32_t* input_pos, const float* rand_next, uint64_t* next_key, int32_t global_tokens,
                          int32_t recent_window, int32_t HQ, float scale, void* y, void* workspace,
                          size_t workspace_bytes, cc_stream_t stream);
/* KVCacheRandom's fused step with the uniform draws made IN the kernels (r3): ref cache.py:519-524 draws torch.rand(S) per
 * eviction — a backend-specific stream, so parity is defined given the vector (cc_decode_step_random, the injection point of the
 * tests); a product run needs no vector and no extra launch: the draw for slot s at position p is
 *   u(seed, p, s) = (mix64(seed + p * 0x9E3779B97F4A7C15 + s) >> 40) * 2^-24   (24 bits, like torch.rand's float32)
 * with mix64 = the murmur3 64-bit finaliser applied twice — stateless (a hipGraph replay advances with *input_pos), identical in
 * the single-launch step, the two-launch step, cc_random_next_key_init_rng and the oracle's twins. */
int cc_random_next_key_init_rng(const cc_kv_view* c, const int32_t* input_pos, uint64_t seed, int32_t global_tokens,
                                int32_t recent_window, uint64_t* next_key, cc_stream_t stream);
int cc_decode_step_random_rng(const cc_kv_view* c, const void* q, const void* k_new, const void* v_new, const int32_t* input_pos,
                              uint64_t seed, uint64_t* next_key, int32_t global_tokens, int32_t recent_window, int32_t HQ,
                              float scale, void* y, void* workspace, size_t workspace_bytes, cc_stream_t stream);
/* The head-constant steps with the RECOVERABLE hand-off (late r3; semantics as cc_decode_step_heavy_hitter_rc below: commit words,
 * replay of committed heads, no-op behind a set status word).  policy: 2 = recent_global / full (rand_next must be NULL), 3 = random
 * (rand_next: the uniform vector for position *input_pos + 1, or NULL: the draws are made in the kernels from `seed`, as
 * cc_decode_step_random_rng — the only form a retry may use: a retried step must score the same draw).  step_commit: int32
 * [H, cc_decode_step_commit_stride()], -1 = nothing committed; may be NULL (no replay).  The rows of next_key [H, NK] stay identical across kv heads through a
 * recovered fault: every head scores the shared positions and the same draws.  The position row (shared) is written by kv head
 * 0's inserting workgroup ahead of the hand-off — idempotent on a retry; the count by kv head 0 at its commit. */
int cc_decode_step_head_constant_rc(const cc_kv_view* c, int32_t policy, const void* q, const void* k_new, const void* v_new,
                                    const int32_t* input_pos, const float* rand_next, uint64_t seed, uint64_t* next_key,
                                    int32_t* step_commit, int32_t global_tokens, int32_t recent_window, int32_t HQ, float scale,
                                    void* y, void* workspace, size_t workspace_bytes, cc_stream_t stream);
/* The same two-launch step for KVCacheL2 (cache.py:559-612: score = dtype(max over ALL heads' and slots' key norms -
 * norm), recent window -> +inf, base rules; the inserted key's norm recorded, cache.py:592-593).  The global maximum
 * is folded across the step boundary: the streaming pass publishes per-wave maxima of the surviving norms, the
 * combine pass folds them with the freshly inserted ones.  16-bit caches with head_dim 128 only (CC_ERR_UNSUPPORTED
 * otherwise: use cc_decode_update_l2 + cc_decode_attn_gqa).  c->Hp must be H; key_norm: [H, S] model dtype;
 * next_key: uint64 [H, NK]. */
int cc_l2_next_key_init(const cc_kv_view* c, const int32_t* input_pos, void* key_norm, int32_t global_tokens,
                        int32_t recent_window, uint64_t* next_key, cc_stream_t stream);
int cc_decode_step_l2(const cc_kv_view* c, const void* q, const void* k_new, const void* v_new, const int32_t* input_pos,
                      void* key_norm, uint64_t* next_key, int32_t global_tokens, int32_t recent_window, int32_t HQ,
                      float scale, void* y, void* workspace, size_t workspace_bytes, cc_stream_t stream);
/* ... with the recoverable hand-off (r4; step_commit as in cc_decode_step_heavy_hitter_rc).  The norm maximum crosses kv heads, but
 * every workgroup republishes its own maximum on a retry and the inserted key's norm is stored with the insert (idempotent), so a
 * retried head scores against the same maximum the committed ones did. */
int cc_decode_step_l2_rc(const cc_kv_view* c, const void* q, const void* k_new, const void* v_new, const int32_t* input_pos,
                         void* key_norm, uint64_t* next_key, int32_t* step_commit, int32_t global_tokens, int32_t recent_window,
                         int32_t HQ, float scale, void* y, void* workspace, size_t workspace_bytes, cc_stream_t stream);
/* The same two-launch step for KVCacheHeavyHitter with a finite history window (history_window_size W > 1): the score is
 * dtype(sum_W ring) / clamp(denom, 1, W) over the TRACKED window sums (see cc_hh_ring_update); the evicted slot's ring
 * row, shadow column, accumulator and denom restart from zero inside the combine pass (cache.py:754-763), which also
 * records this step's attention (cache.py:716-723).  ring_num / denom / counter / wsum_acc / wsum as for
 * cc_decode_attn_gqa_ring; next_key: uint64 [H, NK]; attn_out optional. */
int cc_hh_ring_next_key_init(const cc_kv_view* c, const int32_t* input_pos, const int32_t* denom, int32_t W, const float* wsum,
                             int32_t global_tokens, int32_t recent_window, uint64_t* next_key, cc_stream_t stream);
int cc_decode_step_heavy_hitter_ring(const cc_kv_view* c, const void* q, const void* k_new, const void* v_new,
                                     const int32_t* input_pos, void* ring_num, int32_t* denom, int64_t* counter, int32_t W,
                                     uint64_t* wsum_acc, float* wsum, uint64_t* next_key, int32_t global_tokens,
                                     int32_t recent_window, int32_t HQ, float scale, void* y, void* attn_out,
                                     void* workspace, size_t workspace_bytes, cc_stream_t stream);
/* ------------------------------------------------------------------------------------------------
 * Single-launch layer step.  cc_decode_step_heavy_hitter runs the whole step — insert, K/V streaming pass, softmax
 * normalisation, group mean, history update (cache.py:716-722), the arg-min for position *input_pos + 1 (cache.py:725-749)
 * and y — in ONE launch whenever cc_decode_step_single_launch(...) returns 1: 16-bit caches, head_dim 128, HQ / H in
 * {1, 2, 4, 8}, at most 64 workgroups per kv head (the launch plan's split count: n_split <= 64), each with one 64-slot tile per
 * workgroup (S <= 4096) or — HQ / H in {4, 8}, heavy hitter / recent_global / full / random — up to eight of them (S <= 32768
 * where the plan keeps 64 splits, i.e. 8 kv heads and more per rank), at most 32 kv heads, and the n_split * H workgroups all
 * resident on the device at once.  Every workgroup publishes its partial (m, l, O) through the workspace as
 * self-validating tagged granules (write-through stores), waits — bounded — for the other workgroups of its kv head,
 * and finishes its own 64 slots from the scores still in its registers.  pos, mask, cache_cts, K/V, num, denom, counter,
 * attn_out and the next keys are bit-identical to the two-launch step; y agrees up to fp32 summation order.
 * The kernels the single launch normally runs carry no measurement hooks and no attn_out store (0.3-0.5 us of the step): a call
 * that passes attn_out, sets a measurement bit of `phases` or runs while a trace buffer is installed (cc_decode_step_trace) is
 * served by a full-featured instantiation where one exists (bf16, HQ / H = 4), by the two-launch step otherwise — with
 * CC_PHASE_ONE_LAUNCH, CC_ERR_UNSUPPORTED (a trace buffer alone never changes which step runs: no stamps are written then).
 * Workspace contract for this mode: the first 4 KiB + 288 KiB + 16 MiB of every decode workspace (sized in by
 * cc_decode_attn_workspace_bytes, at fixed offsets whatever the shape, so that caches of different lengths may share one
 * workspace) hold per-head epoch words and the granules; they must be ZERO before first use and written by nobody
 * else; a launch that could not complete its hand-off (a device that did not keep the grid resident) sets the 32-bit
 * word at byte offset cc_decode_step_status_offset() to 1 — its results are then invalid.
 * phases for cc_decode_step_heavy_hitter_phases: 1 / 2 / 3 select the launches of the two-launch step as before
 * (3 = both = let the library choose single or two launches); | CC_PHASE_TWO_LAUNCH never uses the single launch;
 * CC_PHASE_ONE_LAUNCH demands it (CC_ERR_UNSUPPORTED when not possible).
 * ---------------------------------------------------------------------------------------------- */
#define CC_PHASE_TWO_LAUNCH 0x10000
#define CC_PHASE_ONE_LAUNCH 0x20000
int32_t cc_decode_step_single_launch(int32_t HQ, int32_t H, int32_t S, int32_t D, int32_t dtype);
int32_t cc_decode_step_status_offset(void);
/* r6: every wait of the in-launch hand-off is bounded by DEVICE TIME (the 100 MHz clock all XCDs share), not by a number of poll
 * rounds: a workgroup that has waited this many microseconds for its kv head's other workgroups gives up (status word, fail word:
 * below).  The failure latency a caller's recovery path sees is this plus the kernel's own few microseconds.  (r2-r5: 2^18 poll
 * rounds — 1.6 s measured with memory polls.)  ref: the reference has no hand-off (cache.py:725-765 runs in one eager op chain). */
int32_t cc_decode_step_wait_bound_us(void);
/* The heavy-hitter layer step with the RECOVERABLE hand-off (r3; per-workgroup commit words r4): cc_decode_step_heavy_hitter_phases
 * plus `step_commit`, int32 [H, cc_decode_step_commit_stride()] on the device, all -1 = nothing committed (reset it whenever
 * positions restart).  ref: the reference has no hand-off to time out (cache.py:725-765, 716-722); this is what makes ours safe.
 * Words of kv head h: [0] = (slot << 1) | was_empty of the slot position [1]'s insert went to (-1: none), [2 + split] = the last
 * position whose step workgroup `split` of the head has committed.  Single-launch form (early (m, l) hand-off; since late r4 also
 * the several-tiles-per-wave form, whose tail keeps the memory order — one gather — and commits EVERYTHING, y included, behind it):
 *   - a launch that finds the status word set returns at once (a step of this token failed: nothing is built on its output);
 *   - a workgroup that gives up waiting sets the status word and its head's fail word; a workgroup that reads the fail word with
 *     its last gather commits nothing; one that does not commits ITS part — its slots' history, its next-eviction keys, its word
 *     [2 + split] = *input_pos (split 0: also the head's count and the step counter) — and nothing else;
 *   - a workgroup whose word equals *input_pos recomputes its scores and partials (the hand-off needs them: same values, bit for
 *     bit) and stores nothing; every workgroup of a head whose word [1] equals *input_pos takes the insert slot from word [0] (the
 *     key row may already hold the next position's keys).  Whatever the interleaving of give-ups and commits inside the failed
 *     launch, every slot's history is updated exactly once per position: a retry is idempotent per workgroup.
 * So the caller recovers by clearing the status word, advancing the workspace's epoch words (attention_utils.
 * reset_single_launch_status does both) and running the SAME token again.  Other launch forms ignore step_commit (nothing in them
 * can time out).  step_commit may be NULL: no replay, counts bumped at the insert. */
int32_t cc_decode_step_commit_stride(void);
int cc_decode_step_heavy_hitter_rc(const cc_kv_view* c, const void* q, const void* k_new, const void* v_new,
                                   const int32_t* input_pos, double* num, int32_t* denom, int64_t* counter,
                                   uint64_t* next_key, int32_t* step_commit, int32_t global_tokens, int32_t recent_window,
                                   int32_t HQ, float scale, void* y, void* workspace, size_t workspace_bytes,
                                   cc_stream_t stream, int32_t phases);
/* The layer step WITH THE LAYER'S QKV PROJECTION FOLDED IN (r5) — ref: model.py:375-387 (wqkv, split, apply_rotary_emb), :452-457
 * (RMSNorm), then :389-427 as cc_decode_step_*_rc.  One launch: every workgroup requests the weight rows of its share of its kv
 * head's projection AHEAD of its K / V tile (the tile does not depend on q), computes them with cc_gemv_fused's arithmetic — the
 * residual add x + delta in the model dtype (h_out <- it, may be NULL), RMSNorm in fp32 with two roundings, fp32 dot chains in
 * cc_gemv_fused's order, bias, the Linear's rounding, RoPE on the (even, odd) pairs of the q and k rows: q / k_new / v_new are
 * bit-identical to cc_gemv_fused(wqkv, ..., rope_rows = (HQ + H) * D) — hands them to the head's workgroups through tagged
 * granules (the step's own transports) and runs the recoverable single-launch step on them; the cache's 2 * H * S * D * 2 bytes
 * stream in the shadow of the (HQ + 2H) * D * K * 2 bytes of weights.
 *   wqkv [(HQ + 2H) * D, K] row major (q heads, k heads, v heads), bias [(HQ + 2H) * D] or NULL, x / delta (may be NULL) /
 *   norm_w [K], freqs [D / 2, 2] (cos, sin) of *input_pos in the model dtype (NULL: no RoPE), qkv_out [(HQ + 2H) * D] or NULL
 *   (a plain copy of the projection; nothing in the step reads it).
 *   policy: 1 = heavy hitter (num, denom, counter; c->Hp == H), 2 = recent_global / full, 3 = random (rand_next or, NULL, the
 *   in-kernel draws of `seed`) — the arguments of cc_decode_step_heavy_hitter_rc / cc_decode_step_head_constant_rc.
 * Shapes: cc_decode_step_qkv_available(HQ, H, S, D, dtype, K) != 0 — 16-bit caches, D = 128, HQ / H in {4, 8}, one 16-row tile
 * per wave, K % 8 == 0 and K <= 4096, all workgroups resident; CC_ERR_UNSUPPORTED otherwise (the caller runs cc_gemv_fused and
 * the plain step).  A retry of a failed token recomputes the projection (x and delta are not modified: idempotent). */
int32_t cc_decode_step_qkv_available(int32_t HQ, int32_t H, int32_t S, int32_t D, int32_t dtype, int32_t K);
int cc_decode_step_qkv_rc(const cc_kv_view* c, int32_t policy, const void* wqkv, const void* bias, const void* x, const void* delta,
                          const void* norm_w, float eps, void* h_out, const void* freqs, int32_t K, void* qkv_out,
                          const int32_t* input_pos, double* num, int32_t* denom, int64_t* counter, const float* rand_next,
                          uint64_t seed, uint64_t* next_key, int32_t* step_commit, int32_t global_tokens, int32_t recent_window,
                          int32_t HQ, float scale, void* y, void* workspace, size_t workspace_bytes, cc_stream_t stream);
/* The L2-resident hand-off of the single-launch step (r4).  ref: nothing in the reference corresponds — it is HOW the one launch that
 * replaces cache.py:725-765 + model.py:395-418 + cache.py:716-722 exchanges its partials.  On a device whose dispatcher puts block b
 * of a launch on XCD b % 8 (MI355X in SPX mode), a cache with a multiple of 8 kv heads runs its single-tile step with kv head =
 * block % H: the 16 .. 64 workgroups of a kv head share one XCD, and the head's (m, l) and partial-O granules travel through that
 * XCD's L2 (plain stores, sc1 polls) instead of through memory (write-through stores, sc0 sc1 polls): 9.4 -> 8.5 us per layer step
 * at the Llama-3-8B / cache_len 4096 shape together with the other r4 changes (profiles/r04_ab_step_variants.md).  Results are
 * bit-identical to the memory hand-off (same arithmetic, same fixed orders).  Safety: what the placement needs — blocks b and b + 8
 * of one launch share an XCD; which XCD block 0 lands on varies from launch to launch and is not relied upon — is OBSERVED per device
 * (cc_decode_step_probe_xcd) before the form is ever chosen.  Should it not hold for some launch, a head's workgroups do not see each
 * other's granules: the bounded wait ends the step as a hand-off timeout (status word, nothing committed by the recoverable kinds),
 * a workgroup that gives up sets the head's fail word and its peers stop waiting when they read it, and the harness retries — from
 * the fourth attempt on with the memory hand-off (until the next generation).
 *   cc_decode_step_probe_xcd: synchronous, call OUTSIDE stream capture (the Python layer does so when it creates a decode
 *     workspace on a device); 1 = verified for the current device (cached; two grid shapes, four launches), 0 = refuted or
 *     not probed -> memory hand-off.
 *   cc_decode_step_l2_handoff(): 1 if verified on the current device AND neither demoted there (below) nor switched off by the A/B
 *     switch of include/coldcompress_debug.h.
 *   cc_decode_step_demote_l2_handoff(demoted): state of the CURRENT DEVICE only (r5; the recovery path's lever — the process-wide
 *     switch is a debug hook): 1 = every step launched on this device from now on takes the memory hand-off whatever the probe said,
 *     0 = the probe's verdict counts again.  Returns the previous value.  The forms give bit-identical cache state, so a flip never
 *     changes results; a step captured into a hipGraph keeps the form it was captured with. */
int32_t cc_decode_step_probe_xcd(void);
int32_t cc_decode_step_l2_handoff(void);
int32_t cc_decode_step_demote_l2_handoff(int32_t demoted);
/* The two-launch step for KVCacheHybrid (FastGen per-head policies; cache.py:896-1019 + the fused ring update of
 * cc_decode_attn_gqa_ring): three launches -> two.  What a head does with the incoming token — append at the end of its
 * live slots, evict its candidate, or drop the token (slot S - 1, mask untouched) — depends on its policy, its count, the
 * budget terms and whether the token is punctuation (cache.py:905-950): decided at the top of the K/V streaming pass, from
 * device scalars.  The CANDIDATE (arg-min over the head's live slots of window-sum / min(denom, W) or of pos, with the
 * protections of cache.py:876-889 applied) depends only on the state the previous step left behind: the combine pass
 * scores it for position *input_pos + 1 from the freshly updated window sums, commits the counts the inserts produced
 * and bumps num_punc (cache.py:1017).  cc_hybrid_next_key_init seeds the candidates.  Arguments as for
 * cc_hybrid_decode_update / cc_decode_attn_gqa_ring; ring_num may be NULL when no head scores by accumulated attention
 * (then denom / counter / wsum_acc / wsum are unused).  reset-history-on-evict is not part of this step (the reference's
 * effective behaviour, see cache.py of this package); 16-bit caches with head_dim 128 and at most 21 policy rows only
 * (CC_ERR_UNSUPPORTED otherwise: use cc_hybrid_decode_update + cc_decode_attn_gqa[_ring]).  next_key: uint64 [H, NK].
 * Bit-identical to the three-launch sequence (tests/test_gpu_hybrid.py). */
int cc_hybrid_next_key_init(const cc_kv_view* c, const int32_t* input_pos, const int64_t* strategies, const int32_t* policy_table,
                            int32_t n_policies, const int32_t* denom, int32_t W, const float* wsum, const uint8_t* special_mask,
                            const uint8_t* punc_mask, int32_t global_tokens, uint64_t* next_key, cc_stream_t stream);
int cc_decode_step_hybrid(const cc_kv_view* c, const void* q, const void* k_new, const void* v_new, const int32_t* input_pos,
                          const int64_t* strategies, const int32_t* policy_table, int32_t n_policies, void* ring_num, int32_t* denom,
                          int64_t* counter, int32_t W, uint64_t* wsum_acc, float* wsum, const uint8_t* special_mask,
                          uint8_t* punc_mask, const int64_t* token_id, const int64_t* punc_ids, int32_t n_punc_ids,
                          const int32_t* num_special, int32_t* num_punc, uint64_t* next_key, int32_t global_tokens, int32_t HQ,
                          float scale, void* y, void* attn_out, void* workspace, size_t workspace_bytes, cc_stream_t stream);
/* The same step with the recoverable hand-off's commit words (step_commit: int32 [H, cc_decode_step_commit_stride()], -1 before
 * the first step; null: cc_decode_step_hybrid).  Single-launch form: a workgroup that gives up waiting, or finds that a workgroup
 * of its kv head did, stores NOTHING of the step (no y, no ring column / window sum / denominator, no keys, no counts); the others
 * commit their part and mark it in their word.  The per-head decision of the position (slot, append / evict / drop, the head's
 * count before the step, the ring column) is recorded in words [0], [1], [66], [67] before anything can be committed, and a retry
 * of the position takes it from there: committed workgroups recompute (the hand-off needs their partials, y is written again)
 * and store nothing else.  The two-launch form ignores step_commit (nothing to time out). */
int cc_decode_step_hybrid_rc(const cc_kv_view* c, const void* q, const void* k_new, const void* v_new, const int32_t* input_pos,
                             const int64_t* strategies, const int32_t* policy_table, int32_t n_policies, void* ring_num,
                             int32_t* denom, int64_t* counter, int32_t W, uint64_t* wsum_acc, float* wsum, const uint8_t* special_mask,
                             uint8_t* punc_mask, const int64_t* token_id, const int64_t* punc_ids, int32_t n_punc_ids,
                             const int32_t* num_special, int32_t* num_punc, uint64_t* next_key, int32_t* step_commit,
                             int32_t global_tokens, int32_t HQ, float scale, void* y, void* attn_out, void* workspace,
                             size_t workspace_bytes, cc_stream_t stream);
/* cc_decode_step_hybrid runs as ONE launch (the single-launch form above: in-launch hand-off, every workgroup resident) when
 * this returns 1: 16-bit caches, head_dim 128, HQ / H in {4, 8}, up to eight 64-slot tiles per workgroup (S <= 32768 at 64
 * workgroups per kv head).  The tail then also does what the combine pass did for this policy: ring column, exact window sum and
 * denominator of every slot (on all lanes), the head's candidate for the next position, the head's count (committed by the
 * head's first workgroup once all of them have published), and the step counter / num_punc (committed by the LAST head to
 * complete, through a ticket word in the workspace header: the workgroups of every head read them in their prologue).
 * Bit-identical to the two-launch step in every buffer but y (one rounding, as for the other policies).
 * cc_decode_step_set_single_launch(0) switches it off; the status word is shared with the other single-launch steps. */
int32_t cc_decode_step_hybrid_single_launch(int32_t HQ, int32_t H, int32_t S, int32_t D, int32_t dtype);
/* ------------------------------------------------------------------------------------------------
 * Quantised KV cache, --cache_bits {8, 4, 2}.  ref: quantization_utils.py:4-98 (quantize_tensor /
 * dequantize_tensor with axis = 2), KVCache.quantize_cache / dequantize_cache cache.py:283-309, called around
 * every update (cache.py:323-338).  One (scale, zero point) per cache slot, shared by all heads and channels;
 * every elementwise op rounds to the cache dtype as torch does:
 *   scale[s] = dtype(max(dtype(max_s - min_s), dtype(1e-6)) / (2^n - 1));  zero[s] = dtype(min_s + dtype(scale * 2^(n-1)));
 *   q = clamp(roundeven(dtype(dtype(x - min_s) / scale)), 0, 2^n - 1);  dequant = dtype(dtype((q - 2^(n-1)) * scale) + zero).
 * q image: n = 8 -> int8 [H, S, D] holding (uint8)q;  n = 4 / 2 -> uint8 [H*S*D*n/8], 8/n consecutive values of the
 * flattened [H, S, D] tensor per byte, value j shifted left by j*n bits (D % (8/n) == 0).
 * cc_kv_requant: work <- dequant(quant(work)) in place and the q image / scales / zeros are emitted — the
 *   reference's quantize_cache() at the end of one update followed by dequantize_cache() at the start of the next.
 * cc_kv_dequant: work_out <- dequant(q image) (loading a quantised state).
 * ---------------------------------------------------------------------------------------------- */
int cc_kv_requant(void* work, void* q_out, void* scales, void* zeros, int32_t H, int32_t S, int32_t D,
                  int32_t dtype, int32_t n_bit, cc_stream_t stream);
/* K and V in one launch (what KVCache.quantize_cache does every step).
 * Optional exact skipping (stable != NULL): the round trip of a slot is a pure function of that slot's rows, so once a
 * pass left them bit-identical (stable[kv, s] = 1) and no insert touched the slot since (pos[:, s] still equals
 * pos_seen[kv, :, s]; an insert always writes a new position), repeating it would reproduce the same rows, image,
 * scale and zero point — the slot is skipped.  stable: uint8 [2, S], pos_seen: int32 [2, Hp, S], both zero-initialised
 * (and zeroed again whenever the working caches are written by anything but the cache's own inserts); pos: [Hp, S]. */
int cc_kv_requant_pair(void* k_work, void* k_q, void* k_scales, void* k_zeros, void* v_work, void* v_q, void* v_scales,
                       void* v_zeros, int32_t H, int32_t S, int32_t D, int32_t dtype, int32_t n_bit, const int32_t* pos,
                       int32_t Hp, uint8_t* stable, int32_t* pos_seen, cc_stream_t stream);
/* The same round trip for SEVERAL caches in ONE launch: what a model runs at the end of a token for all its layers (the
 * reference does it per layer inside update_kv, cache.py:323-338; the round trip of layer l is only needed before layer l's
 * NEXT step, so one launch behind the last layer replaces one launch per layer).  table (device): n_caches x 16 int64 —
 * k_work, k_q, k_scales, k_zeros, v_work, v_q, v_scales, v_zeros, pos, stable, pos_seen (pointers as for the pair call; stable
 * and pos_seen are required here), S, Hp, 0, 0, 0.  All caches share H, D, dtype, n_bit; S may differ (S_max = the largest).
 * Slot for slot the arithmetic of the pair call.  CC_ERR_UNSUPPORTED where the pair call would take its element-wise form
 * (D not a multiple of the 16-byte vector, or H * D / vector > 1024). */
int cc_kv_requant_batch(const int64_t* table, int32_t n_caches, int32_t H, int32_t S_max, int32_t D, int32_t dtype, int32_t n_bit,
                        cc_stream_t stream);
int cc_kv_dequant(const void* q, const void* scales, const void* zeros, void* work_out, int32_t H, int32_t S,
                  int32_t D, int32_t dtype, int32_t n_bit, cc_stream_t stream);

/* Image format of the fused quantised cache's FP8 mode (the n_bit argument below): OCP e4m3fn codes, a power-of-two scale per row. */
#define CC_QUANT_FP8_E4M3 (0x100 | 8)
/* Image format of the fused quantised cache's 4-bit mode (the n_bit argument below): the uint8 grid with 15 steps, two codes per byte. */
#define CC_QUANT_UINT4 (0x200 | 4)
/* Image format of the fused quantised cache's MXFP4 mode (the n_bit argument below): OCP e2m1 codes, two per byte, one e8m0 scale per 32 values. */
#define CC_QUANT_MXFP4 (0x300 | 4)

/* ------------------------------------------------------------------------------------------------
 * FUSED quantised KV cache — opt-in (`cache_quant_mode="fused"`, or "fp8" / "uint4" / "mxfp4" below), a DIFFERENT numerical contract from the reference's
 * ("fuse dequant into the attention read instead of whole-cache round trips").
 * The reference (cache.py:283-338, quantization_utils.py:4-45) keeps ONE (scale, zero) per slot shared by all heads and
 * re-quantises the whole cache every step; its numbers are reproduced by cc_kv_requant above.  Here instead:
 *   - one (scale, minimum) pair per (head, slot) ROW of K and one per row of V, float32, fixed when the row is written:
 *       mn, mx = min / max over the row's D values;  range = max(mx - mn, 1e-6f);  scale = range / 255.f;
 *       q[d]   = (uint8) clamp(rintf((x[d] - mn) * (255.f / range)), 0, 255)          (IEEE fp32 ops, round-half-even)
 *       value  = T(fmaf((float)q[d], scale, mn))                                      (one rounding to the model dtype)
 *   - a row is quantised exactly once (at prefill or when the decode step inserts it) and never re-quantised: no drift;
 *     the inserted token is attended to through its image in the step that inserts it (the reference attends to the
 *     unquantised new token once and to its round trip afterwards);
 *   - the decode kernels stream the uint8 images (half the bytes of a 16-bit cache) and dequantise in registers on the way
 *     to the matrix cores; everything else of the step (scores -> dtype, softmax, P.V, history, next-eviction key) is the
 *     fused step of cc_decode_step_heavy_hitter / _heavy_hitter_ring / _recent_global / _random / _hybrid applied to the
 *     dequantised values.  Only K and V become images: history ring, denominators, counters, window sums, positions, mask
 *     and the hybrid cache's counts and punctuation / special masks are the 16-bit caches' own.
 * qparams: float32 [H, S, 4] = (k_scale, k_min, v_scale, v_min) per (head, slot).
 * Every image format serves a multiple of 4 query heads per kv head (HQ / H = 4, 8, 12, ...: 4 or 8 per pass); any other
 * ratio (Qwen2's 7 among them) is CC_ERR_UNSUPPORTED with every cache buffer left untouched.
 * n_bit is the image FORMAT: 8 = the uint8 grid above; CC_QUANT_FP8_E4M3 = FP8 images (`cache_quant_mode="fp8"`);
 * CC_QUANT_UINT4 = 4-bit images (`cache_quant_mode="uint4"`); CC_QUANT_MXFP4 = MXFP4 images (`cache_quant_mode="mxfp4"`); 4, 2 and
 * anything else: CC_ERR_UNSUPPORTED, before any launch.
 * FP8 images: one OCP e4m3fn code per value (the `fn` encoding: no infinities, NaN = 0x7f / 0xff; not the `fnuz` one) and one
 * power-of-two scale 2^e per (head, slot) row of K and of V; qparams holds (2^e_k, 0, 2^e_v, 0), so that buffers, loads and
 * workspace sizes are the uint8 format's:
 *       amax  = max |x[d]| over the row's FINITE values;  amax = m * 2^k with m in [0.5, 1) (frexpf)
 *       e     = m <= 0.875 ? k - 9 : k - 8   (the smallest e with amax <= 448 * 2^e; 448 = 0.875 * 2^9), clamped to [-120, 120];
 *               e = 0 for an all-zero row
 *       q[d]  = e4m3_rne(f32(x[d]) * 2^-e)   (exact scaling; never above 448, so no saturation); a non-finite x[d] encodes
 *               to the e4m3 NaN with its sign (0x7f | sign)
 *       value = T(f32(e4m3(q[d])) * 2^e)     (exact in bf16; in f16 one round to nearest even: inf from 65520 up, subnormals rounded)
 *   The kernels decode with v_cvt_scalef32_pk_{bf16,f16}_fp8 (two values per instruction, the scale applied by the hardware) and
 *   encode the inserted token with v_cvt_pk_fp8_f32.  16-bit model dtypes only (the converters return CC_ERR_UNSUPPORTED for fp32).
 * 4-bit images (CC_QUANT_UINT4): the uint8 grid with 15 steps; qparams keeps its shape and meaning (k_scale, k_min, v_scale, v_min):
 *       mn, mx = min / max over the row's D values;  range = max(mx - mn, 1e-6f);  scale = range / 15.f;
 *       q[d]   = clamp(rintf((x[d] - mn) * (15.f / range)), 0, 15)                  (IEEE fp32 ops, round-half-even, no contraction)
 *       value  = T(fmaf((float)q[d], scale, mn))
 *       byte j of a row's D / 2-byte image holds q[2j] | q[2j + 1] << 4   (low nibble first, as the reference's pack_low_bit_tensor)
 *   Images are [H, S, D / 2] bytes, a quarter of the 16-bit cache.  16-bit model dtypes only (the converters return
 *   CC_ERR_UNSUPPORTED for fp32), even D.
 * MXFP4 images (CC_QUANT_MXFP4): OCP microscaling FP4.  A row's D values are blocks of 32 consecutive channels (D = 128: four), each
 * with its own power-of-two scale 2^e_b, stored as an e8m0 byte; the values are e2m1 codes (sign | magnitude on {0, 0.5, 1, 1.5, 2,
 * 3, 4, 6}):
 *       amax_b = max |x[d]| over the block's FINITE values;  amax_b = m * 2^k with m in [0.5, 1) (frexpf)
 *       e_b    = m <= 0.75 ? k - 3 : k - 2   (the smallest e with amax_b <= 6 * 2^e; 6 = 0.75 * 2^3), clamped to [-120, 120];
 *                e_b = -120 for an all-zero block.  (The OCP recipe's floor(log2 amax) - 2 lets (6, 8) * 2^e saturate; this rule does
 *                not, and the image is a valid MXFP4 image all the same.)  Scale byte = e_b + 127.
 *       code   = sign(x[d]) << 3 | e2m1 magnitude of |f32(x[d]) * 2^-e_b| (exact scaling), round to nearest, ties to the even
 *                mantissa (0.25 -> 0, 0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4); -0 keeps its sign; above 6 (only
 *                where e_b was clamped at 120): 6
 *       value  = T(e2m1(code) * 2^e_b)       (exact in bf16; in f16 one round to nearest even: +-inf from 65520 up, subnormals
 *                rounded, +-0 below half the smallest subnormal)
 *       a block that holds a non-finite value: scale byte 0xff (e8m0's NaN), e_b and the codes as above from the finite values
 *                (+-inf: code 7 under its sign, NaN: code 0 under its sign); EVERY element of such a block decodes to the
 *                quiet NaN the conversion instruction returns (bf16 0xffc0, f16 0xfe00), whatever its code
 *       byte j of a row's D / 2-byte image holds code[2j] | code[2j + 1] << 4   (low nibble first, the uint4 images' order)
 *   qparams keeps its shape: word 0 = K's four scale bytes (byte b = block b, little end first), word 2 = V's, words 1 and 3 zero.
 *   They are BIT PATTERNS held in float32 storage, never used as floats (read them as int32).
 *   The kernels decode with v_cvt_scalef32_pk_{bf16,f16}_fp4 (one byte = two values per instruction, the block's power of two applied
 *   by the hardware: four instructions per 8 values) and encode the inserted token on the VALU.  Images are [H, S, D / 2] bytes.
 *   16-bit model dtypes only (the converters return CC_ERR_UNSUPPORTED for fp32); D a multiple of 32, at most 128.
 * cc_kv_quant_rows / cc_kv_dequant_rows convert whole caches ([H, S, D] model dtype <-> uint8 / FP8 / 4-bit / MXFP4 images + qparams).
 * cc_decode_step_quant: c->k_cache / c->v_cache are the IMAGES [H, S, D] (4-bit and MXFP4: [H, S, D / 2]), c->dtype the MODEL dtype (of q, k_new,
 *   v_new, y, attn_out); 16-bit dtype, D == 128, HQ / H in {4, 8} (CC_ERR_UNSUPPORTED otherwise).
 *   policy: 1 = heavy hitter (num / denom / counter as in cc_decode_step_heavy_hitter, c->Hp == H),
 *           2 = recent_global / full (num = denom = NULL, c->Hp == 1), 3 = random (rand_next as in cc_decode_step_random).
 *   next_key comes from the policy's own *_next_key_init (it reads positions and history only, never K / V).
 *   phases: as cc_decode_step_heavy_hitter_phases (3 = the whole step; CC_PHASE_* select the launch form);
 *   cc_decode_step_quant_single_launch: 1 when the single-launch form is available for the shape on this device.
 * ---------------------------------------------------------------------------------------------- */
int cc_kv_quant_rows(const void* k, const void* v, int32_t H, int32_t S, int32_t D, int32_t dtype, int32_t n_bit,
                     uint8_t* k_q, uint8_t* v_q, float* qparams, cc_stream_t stream);
int cc_kv_dequant_rows(const uint8_t* k_q, const uint8_t* v_q, const float* qparams, int32_t H, int32_t S, int32_t D,
                       int32_t dtype, int32_t n_bit, void* k_out, void* v_out, cc_stream_t stream);
int cc_decode_step_quant(const cc_kv_view* c, float* qparams, int32_t n_bit, int32_t policy, const void* q,
                         const void* k_new, const void* v_new, const int32_t* input_pos, double* num, int32_t* denom,
                         int64_t* counter, const float* rand_next, uint64_t* next_key, int32_t global_tokens,
                         int32_t recent_window, int32_t HQ, float scale, void* y, void* attn_out, void* workspace,
                         size_t workspace_bytes, cc_stream_t stream, int32_t phases);
/* ... with the recoverable hand-off and, for policy 3, the in-kernel uniform draws (r4): rand_next may be NULL — the draws are then
 * the stateless hash of (seed, position, slot) that cc_decode_step_random_rng uses (the pipeline must have been seeded with
 * cc_random_next_key_init_rng on the same seed).  step_commit as in cc_decode_step_heavy_hitter_rc (may be NULL). */
int cc_decode_step_quant_rc(const cc_kv_view* c, float* qparams, int32_t n_bit, int32_t policy, const void* q, const void* k_new,
                            const void* v_new, const int32_t* input_pos, double* num, int32_t* denom, int64_t* counter,
                            const float* rand_next, uint64_t seed, uint64_t* next_key, int32_t* step_commit, int32_t global_tokens,
                            int32_t recent_window, int32_t HQ, float scale, void* y, void* workspace, size_t workspace_bytes,
                            cc_stream_t stream, int32_t phases);
int32_t cc_decode_step_quant_single_launch(int32_t HQ, int32_t H, int32_t S, int32_t D, int32_t dtype, int32_t n_bit);
/* The same images for the two history-ring policies.  Arguments as cc_decode_step_heavy_hitter_ring / cc_decode_step_hybrid_rc, plus
 * qparams [H, S, 4] and n_bit (the format: 8, CC_QUANT_FP8_E4M3, CC_QUANT_UINT4 or CC_QUANT_MXFP4; others: CC_ERR_UNSUPPORTED, before any launch);
 * c->k_cache / c->v_cache are the images,
 * c->dtype the model dtype.  16-bit dtype, D == 128, HQ / H in {4, 8} (CC_ERR_UNSUPPORTED otherwise).
 * cc_decode_step_heavy_hitter_ring_quant (history_window_size W > 1): two launches, as in 16 bits — the streaming pass reads the
 *   images and quantises the inserted token's rows ahead of its tile, the combine pass updates the ring, the window sums and the
 *   next-eviction keys.  Seed next_key with cc_hh_ring_next_key_init (it never reads K / V).
 * cc_decode_step_hybrid_quant_rc: the hybrid step (decision, ring column, counts, punctuation, commit words unchanged); only the
 *   K / V source and the insert differ.  One launch where cc_decode_step_hybrid_quant_single_launch says so (up to eight 64-slot tiles
 *   per wave, as the 16-bit hybrid step), two otherwise.  Seed next_key with cc_hybrid_next_key_init. */
int cc_decode_step_heavy_hitter_ring_quant(const cc_kv_view* c, float* qparams, int32_t n_bit, const void* q, const void* k_new,
                                           const void* v_new, const int32_t* input_pos, void* ring_num, int32_t* denom, int64_t* counter,
                                           int32_t W, uint64_t* wsum_acc, float* wsum, uint64_t* next_key, int32_t global_tokens,
                                           int32_t recent_window, int32_t HQ, float scale, void* y, void* attn_out, void* workspace,
                                           size_t workspace_bytes, cc_stream_t stream);
int cc_decode_step_hybrid_quant_rc(const cc_kv_view* c, float* qparams, int32_t n_bit, const void* q, const void* k_new,
                                   const void* v_new, const int32_t* input_pos, const int64_t* strategies, const int32_t* policy_table,
                                   int32_t n_policies, void* ring_num, int32_t* denom, int64_t* counter, int32_t W, uint64_t* wsum_acc,
                                   float* wsum, const uint8_t* special_mask, uint8_t* punc_mask, const int64_t* token_id,
                                   const int64_t* punc_ids, int32_t n_punc_ids, const int32_t* num_special, int32_t* num_punc,
                                   uint64_t* next_key, int32_t* step_commit, int32_t global_tokens, int32_t HQ, float scale, void* y,
                                   void* attn_out, void* workspace, size_t workspace_bytes, cc_stream_t stream);
int32_t cc_decode_step_hybrid_quant_single_launch(int32_t HQ, int32_t H, int32_t S, int32_t D, int32_t dtype, int32_t n_bit);
/* ... and for the l2 step (cc_decode_step_l2[_rc]); cc_decode_step_single_launch_enabled: 1 while the process-wide switch
 * (cc_decode_step_set_single_launch, include/coldcompress_debug.h) AND the current device's own (cc_decode_step_device_single_launch,
 * below) allow the single-launch forms at all.  Together with the
 * per-kind queries they tell a caller which FORM a step call will take: only the single-launch forms read the status / commit words
 * of the recoverable hand-off (the two-launch and three-call forms have nothing that can time out and ignore them). */
int32_t cc_decode_step_l2_single_launch(int32_t HQ, int32_t H, int32_t S, int32_t D, int32_t dtype);
int32_t cc_decode_step_single_launch_enabled(void);
/* r6 — the knob for SHARED devices (per device, like the co-residency it is about).  The single-launch forms need all
 * workgroups of a launch resident together: on a GPU that this process shares with other processes or concurrent kernels (several TP
 * ranks on one GPU, a co-tenant job) that does not hold, and every hand-off would end in the bounded wait.  enabled == 0: steps
 * launched on the CURRENT device take the two-launch forms from now on (nothing in them can time out; the cache state they leave is
 * bit-identical, so the switch may be flipped between any two steps); != 0: the single-launch forms again.  Other devices of the
 * process are untouched; cc_decode_step_single_launch_enabled and the per-kind queries answer for the current device.  -> the previous
 * value.  (A step captured into a hipGraph keeps the form it was captured with.)  ref: the reference has no such form to switch
 * (cache.py:314-364 runs as eager ops). */
int32_t cc_decode_step_device_single_launch(int32_t enabled);

/* ------------------------------------------------------------------------------------------------
 * Prefill-time cache fill.  ref: KVCache._prefill_update / _fill_contiguous cache.py:381-401.
 *   slots 0..T-1 of every head <- k_val/v_val rows; pos[hp, t] <- pos_val[min(hp,PH-1), t] (int32 cast);
 *   mask[h, t] <- 1; cache_cts[j] += T.
 * k_val, v_val: [H, T, D] contiguous; pos_val: int64 [PH, T] with PH == 1 or PH == Hp.
 * ---------------------------------------------------------------------------------------------- */
int cc_prefill_fill(const cc_kv_view* c, const void* k_val, const void* v_val, const int64_t* pos_val,
                    int32_t PH, int32_t T, cc_stream_t stream);

/* Row L2 norms.  ref: KVCacheL2.update_state cache.py:607-612; PromptCompressorL2 prompt_compression.py:201-203.
 * x: [H, N, D] dtype -> out[H, N] dtype = dtype(sqrt(sum_d x^2)) (fp32 accumulate); negate != 0 -> -norm. */
int cc_row_l2_norm(const void* x, int32_t H, int32_t N, int32_t D, int32_t dtype, int32_t negate,
                   void* out, cc_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Prompt compaction.  ref: PromptCompressor._keep_idxs prompt_compression.py:21-26 and
 * _filter_kv :69-72 / :82-88.
 * cc_topk_keep: keep[hs, 0..K) = ascending-sorted indices of the K largest priorities of row hs.
 *   Ties at the K-th value are broken lowest-index-first (torch's CPU order there is
 *   implementation-defined; see DESIGN.md "top-k tie contract").  NaN ranks above +inf (torch.topk).
 *   priority: [Hs, L] of prio_dtype (CC_PRIO_*).  keep_out: int64 [Hs, K].
 * cc_gather_rows: dst[h, j, :] = src[h, keep[min(h,Hk-1), j], :]; src [H, L, D], dst [H, K, D].
 * ---------------------------------------------------------------------------------------------- */
size_t cc_topk_keep_workspace_bytes(int32_t Hs, int32_t L, int32_t K);
int cc_topk_keep(const void* priority, int32_t prio_dtype, int32_t Hs, int32_t L, int32_t K,
                 int64_t* keep_out, void* workspace, size_t workspace_bytes, cc_stream_t stream);
int cc_gather_rows(const void* src, const int64_t* keep, int32_t Hk, int32_t H, int32_t L, int32_t K,
                   int32_t D, int32_t dtype, void* dst, cc_stream_t stream);
/* dst[hs, j] = src[hs, keep[hs, j]] for a [Hs, L] vector of `dtype` (cumulative-attention gather,
 * ref: PromptCompressorHeavyHitter._update_state prompt_compression.py:189-194). */
int cc_gather_vec(const void* src, const int64_t* keep, int32_t Hs, int32_t L, int32_t K, int32_t dtype,
                  void* dst, cc_stream_t stream);

/* KVCacheAnalysis (`debug_<strategy>`) decode-time bookkeeping in one launch.  ref: cache.py:1391-1404.
 *   attn: [>= Hp, S_full] dtype — the group-mean attention row over the FULL cache (row h = kv head h; a head-constant shadow
 *         cache reads row 0 only, like the reference's gather with a [1, 1, S] index);
 *   pos:  [Hp, S] int32 — the shadow cache's positions, -1 = unfilled (reads the last column, which is zero);
 *   sub_out: [Hp, S] dtype = attn[h, pos[h, s]] — what the shadow cache's update_state receives;
 *   losses[*loss_ctr] = dtype(mean_h dtype(1 - dtype(sum_s sub_out[h, s]))), then *loss_ctr += 1 (device scalars; cap = length of
 *   losses; an index beyond it is counted but not stored).  Hp <= 64. */
int cc_analysis_loss(const void* attn, const int32_t* pos, int32_t Hp, int32_t S_full, int32_t S, int32_t dtype, void* sub_out,
                     void* losses, int32_t* loss_ctr, int32_t cap, cc_stream_t stream);

/* SnapKV priority.  ref: PromptCompressorHeavyHitter._token_importances prompt_compression.py:170-187.
 *   obs_mean: [H, L] dtype = mean over the last min(16,L) query rows of the group-averaged probabilities.
 *   out[h,t] = dtype(avgpool5(obs_mean)[h,t]) (pad 2, count_include_pad=False);
 *   t >= L-obs_len -> 1.0; t < global_tokens -> 1.0. */
int cc_snapkv_priority(const void* obs_mean, int32_t H, int32_t L, int32_t dtype, int32_t obs_len,
                       int32_t global_tokens, void* out, cc_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Prefill attention with the side outputs the eviction policies need, without materialising [HQ,L,L].
 * ref: attention_utils.py:36-54 (naive path, causal mask) + model.py:413-418 (group mean) +
 *      cache.py:704 / prompt_compression.py:170-173,189-192 (column mean, observation-window mean).
 *   q: [HQ, L, D]; k, v: [H, L, D]; causal.  y: [HQ, L, D] dtype.
 *   colsum_out [H, L] f32 (optional): sum over queries of the group-averaged dtype-rounded probabilities.
 *   obs_out    [H, L] f32 (optional): mean over the last obs_len queries of the same.
 * ---------------------------------------------------------------------------------------------- */
size_t cc_prefill_attn_workspace_bytes(int32_t HQ, int32_t H, int32_t L, int32_t D, int32_t dtype);
int cc_prefill_attn(const void* q, const void* k, const void* v, int32_t HQ, int32_t H, int32_t L,
                    int32_t D, int32_t dtype, float scale, void* y, float* colsum_out, float* obs_out,
                    int32_t obs_len, void* workspace, size_t workspace_bytes, cc_stream_t stream);

/* The same with band-sum side outputs for the hybrid profiling score: band_out[b, h, k] = sum over queries
 * q in [k, k + bands[b]) of the group-averaged dtype-rounded probabilities (cf. cc_attn_bandsum).
 * bands: HOST int32[n_bands], n_bands <= 4; band_out: device f32 [n_bands, H, L]. */
int cc_prefill_attn_bands(const void* q, const void* k, const void* v, int32_t HQ, int32_t H, int32_t L, int32_t D,
                          int32_t dtype, float scale, void* y, float* colsum_out, float* obs_out, int32_t obs_len,
                          const int32_t* bands, int32_t n_bands, float* band_out, void* workspace,
                          size_t workspace_bytes, cc_stream_t stream);

/* Column sums of a materialised attention tensor (API-compat path when a caller hands the reference's
 * own [H, L, L] probabilities).  ref: cache.py:704.  out[h,k] = sum_q attn[h,q,k] (fp32 accumulate). */
int cc_attn_colsum(const void* attn, int32_t H, int32_t Lq, int32_t Lk, int32_t dtype, float* out,
                   cc_stream_t stream);

/* Column mean used by the heavy-hitter prefill state and the SnapKV state.
 * ref: cache.py:704 and prompt_compression.py:191: `attn.sum(dim=2) / (seq_len - input_pos)` on a
 * model-dtype tensor: out[h,t] = dtype( dtype(colsum[h,t]) / (float)(L - input_pos[t]) ).
 * input_pos: int64 [L] or NULL (= arange(L), what prefill always passes, generation_utils.py:462). */
int cc_colsum_to_mean(const float* colsum, const int64_t* input_pos, int32_t H, int32_t L, int32_t dtype,
                      void* out, cc_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Hybrid (FastGen) cache and the W-slot attention-history ring.  ref: KVCacheHybrid cache.py:768-1288.
 * ---------------------------------------------------------------------------------------------- */

/* Decode-time update for a cache whose heads follow different policies.
 * ref: _decoding_update cache.py:965-1019, _select_fill_idx :896-950, _eviction_idx_for_head :844-894.
 *   strategies: int64 [H], policy index of each head (cache_strategies).
 *   policy_table: int32 [n_policies, 3] on the device = {flags, window slots = round(recent_window*S),
 *     heavy-hitter slots = round(heavy_hitter_frac*S)}; flags: 1 heavy_hitter, 2 window, 4 punc, 8 special, 16 full.
 *   num: [H, S, W] model dtype history ring; denom: [H, S] int32.  The heavy-hitter score of a slot is
 *     dtype(sum_W num) / min(denom, W) over the first cache_cts[h] slots; protected slots (first g slots,
 *     special/punctuation slots, pos > p - window) -> +inf; arg-min.
 *   is_punc: device bool[1] (torch.isin(input_ids, punc_ids), cache.py:975) or NULL; with is_punc == NULL and
 *     token_id (device int64[1]) + punc_ids (device int64[n_punc_ids]) given, the same membership test is evaluated
 *     inside the launch.  num_special / num_punc: device int32[1] or NULL.
 *   c must be head-specific and variable-length (Hp == Hc == H).  fill_out: int64 [H] (dropped tokens report S-1).
 * Effects: pos/K/V written at fill_out for every head; mask and cache_cts only on appends; history zeroed on
 * evictions when requires_heavy_hitter; punc_mask set and num_punc += 1 when is_punc. */
int cc_hybrid_decode_update(const cc_kv_view* c, const void* k_new, const void* v_new, const int32_t* input_pos,
                            const int64_t* strategies, const int32_t* policy_table, int32_t n_policies, void* num,
                            int32_t* denom, int32_t W, const uint8_t* special_mask, uint8_t* punc_mask,
                            const uint8_t* is_punc, const int64_t* token_id, const int64_t* punc_ids,
                            int32_t n_punc_ids, const int32_t* num_special, int32_t* num_punc,
                            int32_t global_tokens, int32_t requires_heavy_hitter, int64_t* fill_out,
                            float* wsum_workspace, uint64_t* wsum_acc, cc_stream_t stream);

/* Heavy-hitter decode update with a finite history window (history_window_size W > 1; model-dtype ring).
 * ref: KVCacheHeavyHitter._eviction_idx cache.py:725-765:
 *   avg = float(dtype(sum_W num)) / clamp(denom, 1, W); (pos<g)|(pos>=p-w) -> 1.0; pos==-1 -> 0.0; arg-min;
 *   ring row and denom of the chosen slot zeroed; then the common insert (k_new == NULL: select only).
 * num: [H, S, W] model dtype; denom: [H, S] int32; Hp must be H.
 *
 * Window sums (both ring entry points).  dtype(sum_W num) is DEFINED as the exact sum of the W ring entries rounded
 * once, nearest-even, to the model dtype (torch's own fp32 summation order is unspecified); being exact it does not
 * depend on summation order, so it can be produced two ways with identical results:
 *   wsum_acc == NULL (stateless): wsum_workspace, float [H*S], is caller scratch; a chip-wide pre-pass (one wave per
 *     slot, coalesced) re-reads the whole [H, S, W] ring on every call — 118 MB at H = 8, S = 18432, W = 400.
 *   wsum_acc != NULL (tracked): wsum_workspace / wsum_acc are PERSISTENT state kept current by cc_hh_ring_update
 *     (the overwritten ring entry leaves the sum, the new one enters) and by the evictions here (row zeroed -> sum
 *     zeroed); no pre-pass.  wsum_acc: uint64 [cc_hh_ring_acc_words(H, S, W, dtype)] = per slot a 192-bit
 *     two's-complement fixed-point accumulator in units of 2^-149 plus a count of entries with |v| >= 4 or non-finite
 *     (their window sum is NaN; attention probabilities are <= 1); then two launch-ticket words; then a column-major
 *     [W][H*S] shadow of the ring (the entry a step overwrites is read from there, coalesced); then 2H words where the
 *     workgroups sharing a head meet (zero between launches).  Zero-initialise it
 *     together with the ring, or (re)build it from an existing ring with cc_hh_ring_window_sums. */
int cc_decode_update_heavy_hitter_ring(const cc_kv_view* c, const void* k_new, const void* v_new,
                                       const int32_t* input_pos, void* num, int32_t* denom, int32_t W,
                                       int32_t global_tokens, int32_t recent_window, int64_t* idx_out,
                                       float* wsum_workspace, uint64_t* wsum_acc, cc_stream_t stream);

/* History ring update, history_window_size W > 1.  ref: cache.py:716-723:
 *   num[h, s, *counter % W] = attn[h, s] (0 beyond T); denom += 1 everywhere; *counter += 1.
 * num: [H, S, W] dtype; attn: [H, T] dtype.  wsum_acc / wsum: both NULL, or the tracked window-sum state (above). */
int cc_hh_ring_update(void* num, int32_t* denom, int64_t* counter, const void* attn, int32_t H, int32_t S, int32_t T,
                      int32_t W, int32_t dtype, uint64_t* wsum_acc, float* wsum, cc_stream_t stream);
size_t cc_hh_ring_acc_words(int32_t H, int32_t S, int32_t W, int32_t dtype);
/* Exact window sums of a whole ring: wsum float [H*S]; wsum_acc (optional) the tracked state rebuilt from the ring. */
int cc_hh_ring_window_sums(const void* num, int32_t H, int32_t S, int32_t W, int32_t dtype, float* wsum,
                           uint64_t* wsum_acc, cc_stream_t stream);

/* Band sums of a materialised attention tensor: out[h,k] = sum_{q=k}^{k+band-1} attn[h,q,k] (fp32, sequential).
 * Used by the hybrid profiling score for window policies (ref: create_window_attention_mask cache.py:142-149 +
 * profile_attn_heads :1165-1168 rewritten per key instead of per [L, L] mask). */
int cc_attn_bandsum(const void* attn, int32_t H, int32_t Lq, int32_t Lk, int32_t dtype, int32_t band, float* out,
                    cc_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Caller glue around the hot path (ref: model.py Attention.forward / TransformerBlock / RMSNorm /
 * apply_rotary_emb / FeedForward).  The reference leaves these to ~45 eager elementwise launches per layer
 * (or to torch.compile); here they are three fused launches so the decode step is GEMV-bound.
 * ---------------------------------------------------------------------------------------------- */

/* (optional residual add) + RMSNorm.  ref: model.py:452-457 and :325-326.
 *   h = delta ? x + delta : x   (model dtype add, written to h_out if non-NULL; h_out may alias x)
 *   out = dtype( dtype( float(h) * rsqrt(mean(float(h)^2) + eps) ) * weight )
 * x, delta, h_out, out: [T, dim] dtype; weight: [dim] dtype. */
int cc_add_rmsnorm(const void* x, const void* delta, const void* weight, int32_t T, int32_t dim, float eps,
                   int32_t dtype, void* h_out, void* out, cc_stream_t stream);

/* Split the fused QKV projection, apply rotary embedding to q and k, and lay the heads out for attention.
 * ref: model.py:375-387 + apply_rotary_emb :507-519 (adjacent pairs, fp32 math, table stored in model dtype).
 *   qkv: [T, (HQ + 2H) * D] dtype (q block, k block, v block); freqs: [T, D/2, 2] dtype = rows of the
 *   (cos, sin) table already gathered at the token positions.
 *   q_out: [HQ, T, D]; k_out, v_out: [H, T, D]  (== the transposes model.py:385-387 produces). */
int cc_qkv_rope(const void* qkv, const void* freqs, int32_t T, int32_t HQ, int32_t H, int32_t D, int32_t dtype,
                void* q_out, void* k_out, void* v_out, cc_stream_t stream);

/* SwiGLU gate: out = dtype( dtype(silu(a)) * b ).  ref: model.py:442-443 F.silu(w1 x) * w3 x.  a, b, out: [n]. */
int cc_silu_mul(const void* a, const void* b, int64_t n, int32_t dtype, void* out, cc_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Decode-time dense layer (one token) with the caller glue fused in.  ref (caller side): model.py:317-327 (pre-norm
 * block + residual adds), :375-387 (qkv split + apply_rotary_emb), :442-443 (FFN), :452-457 (RMSNorm), :507-519 (RoPE).
 *   prologue  (norm_w != NULL): h = dtype(x + delta) (delta may be NULL), h_out <- h (optional, the updated residual
 *             stream), in = dtype(dtype(h * rsqrt(mean(h^2) + eps)) * norm_w);  else in = x.
 *   product   t[n] = dtype(sum_k W[n,k] * in[k] (+ bias[n])), fp32 accumulation; W: [N, K] row-major (nn.Linear.weight).
 *   W3 != NULL: y[n] = dtype(dtype(silu(t[n])) * dtype(sum_k W3[n,k] * in[k]))           (SwiGLU: w1, w3 in one pass)
 *   freqs != NULL: rows [0, rope_rows) are rotated in (even, odd) pairs with freqs[(row % head_dim)/2] = (cos, sin)
 *             of the current position, fp32 math on the dtype-rounded t (q and k heads of a fused wqkv); rows beyond
 *             rope_rows (v) are copied.
 * K * sizeof(dtype) <= 64 KiB (16 input chunks per lane).  Summation order inside a dot product is the
 * kernel's own (tolerance class, like any GEMM library).
 * ---------------------------------------------------------------------------------------------- */
int cc_gemv_fused(const void* W, const void* W3, const void* x, const void* delta, const void* norm_w, float eps,
                  void* h_out, const void* bias, const void* freqs, int32_t rope_rows, int32_t head_dim, void* y,
                  int32_t N, int32_t K, int32_t dtype, cc_stream_t stream);

/* cc_gemv_fused for T input vectors from ONE pass over the weights, 1 <= T <= CC_GEMV_MULTI_MAX_T: a block of decode steps whose
 * input tokens are known (teacher forcing, the tail of a long prompt) streams W once instead of T times.
 *   x, delta (or NULL), h_out (or NULL): [T, K];  freqs (or NULL): [T, head_dim / 2, 2], row t the (cos, sin) of token t's position;
 *   y: [T, N];  W, W3, norm_w, bias: as cc_gemv_fused, shared by the T rows.
 * Row t of y and of h_out is BIT-IDENTICAL to cc_gemv_fused called with row t of x, delta and freqs, for every dtype, form and
 * shape cc_gemv_fused serves (a row's arithmetic there depends neither on the rows and column steps in flight nor on the grid, and
 * is kept per token here).  Same argument checks and CC_ERR_UNSUPPORTED cases; T outside 1 .. CC_GEMV_MULTI_MAX_T:
 * CC_ERR_BAD_ARG.  Dense weights only (int8 / MXFP4 / int4: cc_gemv_fused_w8_multi / cc_gemv_fused_mx4_multi / cc_gemv_fused_w4_multi).  A plain grid: no workgroup waits for another.  Arguments are validated before any launch:
 * an error writes nothing. */
#define CC_GEMV_MULTI_MAX_T 4
int cc_gemv_fused_multi(const void* W, const void* W3, const void* x, const void* delta, const void* norm_w, float eps,
                        void* h_out, const void* bias, const void* freqs, int32_t rope_rows, int32_t head_dim, void* y,
                        int32_t N, int32_t K, int32_t T, int32_t dtype, cc_stream_t stream);

/* cc_gemv_fused over a LOSSLESS 12-bit packed copy of dense bf16 weights ("w12"): y and h_out are BIT-IDENTICAL to cc_gemv_fused
 * with the same arguments, for three quarters of the weight bytes read.
 *   codes     uint32 [N, K / 8, 3]: the 8 weights of 16-byte chunk c of a row as 12 bytes — dwords 0, 1: byte i = sign << 7 |
 *             mantissa of weight i; dword 2: 4-bit exponent indices (exponent = base + index), weight 2 j at bits [4 j, 4 j + 4),
 *             weight 2 j + 1 at bits [16 + 4 j, 16 + 4 j + 4).
 *   records   uint32 [ceil(N / RB), ceil(nstep / CU), 4, 8] with nstep = ceil(ceil(K / 512) / 4): the weights whose exponent lies
 *             outside [base, base + 15] ("escapes": ±0, subnormals, inf, NaN and outliers among them) of the RB x CU chunks per
 *             lane that wave w of a workgroup requests together for row group g and issue phase p — element t = r * CU + u is
 *             chunk ((p * CU + u) * 4 + w) * 64 + lane of row g * RB + r.  Word 0: the count, 0 .. 7, or 0xFFFFFFFF when there
 *             are more than 7 (the kernel then reads that tile from W itself); words 1 .. 7: t << 25 | lane << 19 | weight in
 *             chunk << 16 | the raw bf16 bits.  The code of an escaped weight is arbitrary.
 * cc_w12_geometry: out[0 .. 3] = RB, CU, input chunks kept per lane, most workgroups of the launch for (N, K) and the form (swiglu:
 *             the W / W3 pair); out[4] = 1 when that launch class measured faster than cc_gemv_fused on MI355X (the pair, and plain
 *             matrices of 32768 rows or more, at K <= 4096), else 0: callers should keep such weights dense by default.
 *             CC_ERR_UNSUPPORTED when K % 8 != 0 or K > 16384.  Host only.
 * cc_w12_pack: packs W (bf16 [N, K], dense) for the geometry (rb, cu) into codes and records; meta is a device scratch of
 *             cc_w12_meta_words() int32 that afterwards holds base (word 0), the number of records (1), of overflowing records (2)
 *             and of escapes (3).  CC_ERR_UNSUPPORTED for 2^31 weights or more.  base is the start of the window of 16 exponents that covers most weights, 0 .. 240.
 *             Asynchronous on `stream`; three launches, run once per tensor.
 * cc_gemv_fused_w12: cc_gemv_fused's arguments behind the packed copy of W (and of W3, when W3 != NULL) and the (rb, cu) they were
 *             packed for; CC_ERR_BAD_ARG when that is not cc_w12_geometry's answer for this call.  W and W3 stay arguments: tiles
 *             whose record overflowed are read from them.  dtype: CC_DT_BF16 (others: CC_ERR_UNSUPPORTED).  A plain grid, no
 *             atomics; arguments are validated before any launch: an error writes nothing.
 *
 * A packed copy exists in one of three LAYOUTS (two code formats; id 2 is a launch and record layout over the second).  The id travels in bits 8 .. 15 of the `rb` word of cc_w12_pack and
 * cc_gemv_fused_w12 and of the `swiglu` word of cc_w12_geometry (the low byte keeps its meaning; higher bits must be 0; an id other
 * than 0, 1 or 2: CC_ERR_BAD_ARG).  Id 0 is the layout above.  Id 1, "planar", keeps chunk index, records, overflow rule and the
 * dense fallback and changes the 12 bytes of a chunk, with e the 8-bit exponent, s the sign, `base` EVEN and B = base / 2:
 *   dword 0, 1  byte k = the low byte of bf16 weight k resp. 4 + k as it is (e & 1 in bit 7, the mantissa below)
 *   dword 2     byte k = s of weight k << 7 | ((e >> 1) - B) of weight 4 + k << 4 | s of weight 4 + ((k + 3) & 3) << 3 |
 *               ((e >> 1) - B) of weight k — the sign of weight 4 + k sits in bit 3 of byte (k + 1) & 3
 * In-window is base <= e < base + 16 as before; cc_w12_pack searches even bases only for it, and cc_gemv_fused_w12 rejects an odd
 * base.  The kernel decodes a chunk in nine operations (mask 0x87878787 and a bytewise add of B on dword 2 and on dword 2 rotated
 * right by 4 give the eight high bytes; four byte permutes interleave them with the low bytes) against 24 for layout 0.
 * cc_w12_geometry answers per layout: its own (RB, CU, chunks, workgroups) and, as out[4], whether that layout's launch class
 * measured faster than cc_gemv_fused AND than layout 0 on MI355X, in the regime measured (N >= RB x workgroups: a full grid).
 * A copy is tied to its layout as to (rb, cu): cc_w12_pack notes the layout by the address of `codes` (host memory, this
 * process), and cc_gemv_fused_w12 returns CC_ERR_BAD_ARG, before any launch, for codes handed in under another id.
 * Id 2, "long": planar codes (id 1's 12 bytes, an even base) behind a launch of its own for LONG rows — plain matrices (W3 == NULL)
 * with 3 <= nstep <= 8, i.e. 4096 < K <= 16384.  Under id 2 all three entry points return CC_ERR_UNSUPPORTED for anything else (the
 * pair form; every K <= 4096; cc_w12_pack, which does not see the form, for such a K).  The kernel keeps small RB x CU tiles of codes
 * in two register sets and requests the tile after the current one (record first) before it decodes the current one, also across
 * the end of a row group; records have the format above and are laid out for that (RB, CU) — cc_w12_geometry(..., swiglu = 2 << 8)
 * gives it, with out[2] = 8 and out[4] = 1 where the class measured faster than cc_gemv_fused AND than id 1's launch, with a full
 * grid (seven column steps per wave, e.g. 4096 x 14336, and four, K = 8192).  A copy packed under id 1 is refused under id 2 and
 * the other way round (the records differ). */
int cc_w12_geometry(int32_t N, int32_t K, int32_t swiglu, int32_t* out);
size_t cc_w12_meta_words(void);
int cc_w12_pack(const void* W, int32_t N, int32_t K, int32_t rb, int32_t cu, void* codes, void* records, void* meta,
                cc_stream_t stream);
int cc_gemv_fused_w12(const void* codes, const void* records, int32_t base, const void* codes3, const void* records3,
                      int32_t base3, int32_t rb, int32_t cu, const void* W, const void* W3, const void* x, const void* delta,
                      const void* norm_w, float eps, void* h_out, const void* bias, const void* freqs, int32_t rope_rows,
                      int32_t head_dim, void* y, int32_t N, int32_t K, int32_t dtype, cc_stream_t stream);

/* The same decode-time dense layer over INT8 WEIGHT-ONLY matrices (the weight-only int8 checkpoint format, ref: quantize.py
 * WeightOnlyInt8QuantHandler / WeightOnlyInt8Linear): W, W3 int8 [N, K] row major, one scale per output row, scales / scales3 [N]
 * in `dtype`, which is also the activation, bias, freqs and output dtype.
 *   quantisation (the checkpoint's, per row n of w = weight.float()): lo = min(min_k w, 0), hi = max(max_k w, 0),
 *             s32 = max(max(-lo, hi) / 127.5, FLT_EPSILON) in fp32, q = clamp(round_half_even(w / s32), -128, 127),
 *             scales[n] = dtype(s32) (the division uses the fp32 scale, the product the rounded one: the reference's asymmetry).
 *   prologue  exactly cc_gemv_fused's: h_out and the normalised input `in` are bit-identical to it.
 *   product   p[n] = dtype(sum_k in[k] * q[n,k]), fp32 accumulation (int8 x 16-bit products are exact);
 *             t[n] = dtype(p[n] * scales[n]); with bias t[n] = dtype(t[n] + bias[n])   (F.linear -> * scales -> += bias).
 *   W3 != NULL (needs scales3): t3 likewise with scales3, y = dtype(dtype(silu(t)) * t3); no bias.
 *   freqs != NULL: RoPE on rows [0, rope_rows) of the rounded t, as cc_gemv_fused.
 * dtype: CC_DT_BF16 or CC_DT_F16 (CC_DT_F32: CC_ERR_UNSUPPORTED).  K % 16 == 0 and K * sizeof(dtype) <= 64 KiB, else
 * CC_ERR_UNSUPPORTED.  Summation order inside a dot product is the kernel's own (tolerance class) but fixed: results are
 * bit-reproducible from run to run and under graph replay.  Arguments are validated before any launch: an error writes nothing. */
int cc_gemv_fused_w8(const int8_t* W, const void* scales, const int8_t* W3, const void* scales3, const void* x,
                     const void* delta, const void* norm_w, float eps, void* h_out, const void* bias, const void* freqs,
                     int32_t rope_rows, int32_t head_dim, void* y, int32_t N, int32_t K, int32_t dtype, cc_stream_t stream);

/* The same decode-time dense layer over INT4 GROUP-WISE WEIGHT-ONLY matrices (the reference's int4 weight-only mode, ref: quantize.py
 * group_quantize_tensor / WeightOnlyInt4Linear, with this project's code layout): W, W3 uint8 [N, K / 2] row major, two 4-bit codes
 * q in [0, 15] per byte, column 2j in the low nibble of byte j; qparams / qparams3 bf16 [N, K / groupsize, 2] row major, the
 * (scale, zero) pair of each row and group of `groupsize` consecutive columns.  bf16 activations, bias, freqs and output.
 *   quantisation (the checkpoint's, per group of w = bf16 weight, every step rounded to bf16): s = (max - min).clamp(min=1e-6) / 15,
 *             z = min + s * 8, q = clamp(round((w - (z - s * 8)) / s), 0, 15).
 *   prologue  exactly cc_gemv_fused's: h_out and the normalised input `in` are bit-identical to it.
 *   product   p[n] = sum_k in[k] * ((q[n,k] - 8) * s + z), (s, z) the pair of k's group, the weight in fp32 (exact: the
 *             reference's group_dequantize_tensor), fp32 accumulation; t[n] = bf16(p[n]); with bias t[n] = bf16(t[n] + bias[n]).
 *   W3 != NULL (needs qparams3): t3 likewise, y = bf16(bf16(silu(t)) * t3); no bias.
 *   freqs != NULL: RoPE on rows [0, rope_rows) of the rounded t, as cc_gemv_fused.
 * The reference's backends do not round this product identically (CUDA tinygemm rounds each dequantised weight to bf16, the CPU
 * kernel does not), so the contract is a tolerance class around p: the kernel's summation order is its own (group-factored,
 * DESIGN §2.8) but fixed, and results are bit-reproducible from run to run and under graph replay.
 * groupsize in {32, 64, 128, 256} (else CC_ERR_BAD_ARG).  dtype CC_DT_BF16 only (CC_DT_F16 / CC_DT_F32: CC_ERR_UNSUPPORTED).
 * K % groupsize == 0 and K * 2 <= 64 KiB, else CC_ERR_UNSUPPORTED.  Arguments are validated before any launch: an error writes
 * nothing. */
int cc_gemv_fused_w4(const uint8_t* W, const void* qparams, const uint8_t* W3, const void* qparams3, const void* x,
                     const void* delta, const void* norm_w, float eps, void* h_out, const void* bias, const void* freqs,
                     int32_t rope_rows, int32_t head_dim, void* y, int32_t N, int32_t K, int32_t groupsize, int32_t dtype,
                     cc_stream_t stream);

/* The same decode-time dense layer over MXFP4 WEIGHT-ONLY matrices (OCP microscaling FP4, the 4-bit format of gfx950's conversion
 * instructions; harness/quantize.py WeightOnlyMxfp4Linear): W, W3 uint8 [N, K / 2] row major, two e2m1 codes per byte, column 2j in
 * the low nibble of byte j (the int4 / uint4 / MXFP4-KV order, and the order v_cvt_scalef32_pk_bf16_fp4 reads); scales / scales3
 * uint8 [N, K / 32] row major, one e8m0 byte per row and block of 32 consecutive columns, value 2^(byte - 127).  A code is a sign bit
 * over a magnitude in {0, 0.5, 1, 1.5, 2, 3, 4, 6}.  bf16 activations, bias, freqs and output.
 *   quantisation (the checkpoint's, per block b of w = weight.float()): e_b = the smallest integer with amax_b <= 6 * 2^e_b (from
 *             frexp, no division), clamped to [-120, 120]; -120 for an all-zero block (the MXFP4 KV mode's rule: nothing finite
 *             saturates).  codes = round-to-nearest of w * 2^-e_b (an exact product), ties to the even mantissa; -0 keeps its sign.
 *             byte = e_b + 127, so stored scale bytes lie in [7, 247], where code x scale is exact in bf16; the loader refuses any
 *             other byte, and the quantiser refuses a non-finite weight.
 *   prologue  exactly cc_gemv_fused's: h_out and the normalised input `in` are bit-identical to it.
 *   product   p[n] = sum_k in[k] * (e2m1(q[n,k]) * 2^(byte - 127)), the byte of k's block, fp32 accumulation;
 *             t[n] = bf16(p[n]); with bias t[n] = bf16(t[n] + bias[n]).
 *   W3 != NULL (needs scales3): t3 likewise, y = bf16(bf16(silu(t)) * t3); no bias.
 *   freqs != NULL: RoPE on rows [0, rope_rows) of the rounded t, as cc_gemv_fused.
 * The summation order is the kernel's own (tolerance class) but fixed: results are bit-reproducible from run to run and under graph
 * replay.  dtype CC_DT_BF16 only (CC_DT_F16 / CC_DT_F32: CC_ERR_UNSUPPORTED).  K % 32 == 0 and K * 2 <= 64 KiB, else
 * CC_ERR_UNSUPPORTED.  A null required pointer, W / W3 / x / delta / norm_w / h_out not 16-byte aligned, or bias / freqs / y not
 * 2-byte aligned: CC_ERR_BAD_ARG.  Arguments are validated before any launch: an error writes nothing. */
int cc_gemv_fused_mx4(const uint8_t* W, const uint8_t* scales, const uint8_t* W3, const uint8_t* scales3, const void* x,
                      const void* delta, const void* norm_w, float eps, void* h_out, const void* bias, const void* freqs,
                      int32_t rope_rows, int32_t head_dim, void* y, int32_t N, int32_t K, int32_t dtype, cc_stream_t stream);

/* cc_gemv_fused_w8 and cc_gemv_fused_mx4 for T input vectors from ONE pass over the weights, 1 <= T <= CC_GEMV_MULTI_MAX_T: what
 * cc_gemv_fused_multi is to cc_gemv_fused, for weight-only int8 and MXFP4 models.
 *   x, delta (or NULL), h_out (or NULL): [T, K];  freqs (or NULL): [T, head_dim / 2, 2], row t the (cos, sin) of token t's position;
 *   y: [T, N];  W, W3, scales, scales3 (int8: per row, in `dtype`; MXFP4: the e8m0 block bytes), norm_w, bias: as the single-vector
 *   entry point, shared by the T rows.
 * Row t of y and of h_out is BIT-IDENTICAL to the single-vector entry point (cc_gemv_fused_w8 / cc_gemv_fused_mx4) called with row t
 * of x, delta and freqs, for every dtype, form and shape that entry point serves, K * 2 = 64 KiB with the norm prologue included: the
 * lane that owns a weight chunk, the order of its dot chain, the wave and workgroup reductions (MXFP4: the waves per row, a function
 * of K) and every rounding point are kept per token; a weight register is loaded and decoded once and feeds T accumulator chains.
 * The norm prologue passes the T tokens one after the other through ONE staging buffer: the dynamic LDS of a workgroup is the
 * single-vector kernel's.  Same argument checks and CC_ERR_UNSUPPORTED cases as the single-vector entry point; T outside
 * 1 .. CC_GEMV_MULTI_MAX_T: CC_ERR_BAD_ARG.  T = 1 launches the single-vector kernel itself.  A plain grid: no workgroup waits for
 * another.  Arguments are validated before any launch: an error writes nothing.  (Int4 group-wise weights: cc_gemv_fused_w4_multi,
 * below.)
 * Under the tuning hooks (CC_GEMV_W8_CFG / CC_GEMV_MX4_CFG) the refusals are the single-vector entry point's too; the MXFP4 form
 * builds the default geometries only and runs the shape's default one where the hook names another that cc_gemv_fused_mx4 serves
 * (results do not depend on the geometry). */
int cc_gemv_fused_w8_multi(const int8_t* W, const void* scales, const int8_t* W3, const void* scales3, const void* x,
                           const void* delta, const void* norm_w, float eps, void* h_out, const void* bias, const void* freqs,
                           int32_t rope_rows, int32_t head_dim, void* y, int32_t N, int32_t K, int32_t T, int32_t dtype,
                           cc_stream_t stream);
int cc_gemv_fused_mx4_multi(const uint8_t* W, const uint8_t* scales, const uint8_t* W3, const uint8_t* scales3, const void* x,
                            const void* delta, const void* norm_w, float eps, void* h_out, const void* bias, const void* freqs,
                            int32_t rope_rows, int32_t head_dim, void* y, int32_t N, int32_t K, int32_t T, int32_t dtype,
                            cc_stream_t stream);

/* cc_gemv_fused_w4 for T input vectors from ONE pass over the weights, 1 <= T <= CC_GEMV_MULTI_MAX_T: what cc_gemv_fused_mx4_multi is
 * to cc_gemv_fused_mx4, for int4 group-wise weight-only models.
 *   x, delta (or NULL), h_out (or NULL): [T, K];  freqs (or NULL): [T, head_dim / 2, 2], row t the (cos, sin) of token t's position;
 *   y: [T, N];  W, W3, qparams, qparams3, norm_w, bias: as cc_gemv_fused_w4, shared by the T rows.
 * Row t of y and of h_out is BIT-IDENTICAL to cc_gemv_fused_w4 called with row t of x, delta and freqs, for every form, groupsize and
 * shape it serves, K * 2 = 64 KiB with the norm prologue included: the lane that owns a 16-byte code chunk, the order of its dot
 * chain from -136 Sx, the two fused multiply-adds per chunk (scale, then zero times Sx), the wave and workgroup reductions (the waves
 * per row are a function of K) and every rounding point are kept per token; a code register and its (scale, zero) word are loaded and
 * decoded once and feed T accumulator chains.  The norm prologue passes the T tokens one after the other through ONE staging buffer:
 * the dynamic LDS of a workgroup is the single-vector kernel's.  cc_gemv_fused_w4's argument checks and return codes, through the
 * same function (qparams present and paired with W3, groupsize, the shared conditions, bf16 only, K % groupsize == 0); T outside
 * 1 .. CC_GEMV_MULTI_MAX_T: CC_ERR_BAD_ARG; and, here only, W / W3 / x / delta / norm_w / h_out not 16-byte aligned or qparams /
 * qparams3 not 4-byte aligned: CC_ERR_BAD_ARG.  T = 1 launches the single-vector kernel itself.  A plain grid: no workgroup waits
 * for another, no atomics.  Arguments are validated before any launch: an error writes nothing.  Under the tuning hook
 * (CC_GEMV_W4_CFG) the refusals are cc_gemv_fused_w4's too; only the default geometries are built for T > 1, and the shape's default
 * one runs where the hook names another that cc_gemv_fused_w4 serves, under the hook's grid cap (results do not depend on the
 * geometry). */
int cc_gemv_fused_w4_multi(const uint8_t* W, const void* qparams, const uint8_t* W3, const void* qparams3, const void* x,
                           const void* delta, const void* norm_w, float eps, void* h_out, const void* bias, const void* freqs,
                           int32_t rope_rows, int32_t head_dim, void* y, int32_t N, int32_t K, int32_t groupsize, int32_t T,
                           int32_t dtype, cc_stream_t stream);

/* Greedy sampling tail, ref: generation_utils.py:136-142: probs[V] = dtype(softmax_fp32(logits[V])),
 * *idx_out = first index of the largest rounded probability (torch.argmax semantics).  Two small launches; `workspace`
 * (cc_softmax_argmax_workspace_bytes) needs no initialisation.
 * Infinite and NaN logits follow torch.softmax / torch.argmax:
 *   -inf   (a banned token, LogitPenalties' bias) has probability exactly 0 and takes no part in the sum, wherever it stands and
 *          however many there are — whole slices of the vocabulary included; one finite logit among -inf gives exactly 1.0 there;
 *   all -inf, any +inf, any NaN: every probability is NaN and *idx_out = 0 (NaN counts as the maximum, the first one wins), an
 *          index inside the vocabulary. */
size_t cc_softmax_argmax_workspace_bytes(void);
int cc_softmax_argmax(const void* logits, int32_t V, int32_t dtype, void* probs, int32_t* idx_out, void* workspace,
                      size_t workspace_bytes, cc_stream_t stream);

/* Seeded temperature / top-k sampling tail, ref: generation_utils.py:125-133 (logits_to_probs) followed by a STATELESS draw: one
 * answer per (logits, temperature, top_k, seed, *input_pos), the same in eager launches, under hipGraph replay (a replay advances
 * through *input_pos, which is read from DEVICE memory) and on every tensor-parallel rank (replicated logits: no communication).
 * logits[V] and probs[V] in the model dtype T (`dtype`); temperature > 0; top_k <= 0: none; input_pos: the position of the step
 * whose logits these are.
 *   1. scaling   x[i] = T(float(logits[i]) / max(temperature, 1e-5f)): ONE IEEE fp32 division, then rounded to T (the reference's
 *                `logits / temperature` in the model dtype).
 *   2. top-k     k = min(top_k, V); pivot = the k-th largest x counted with multiplicity; kept = {i : x[i] >= pivot} — ties at the
 *                pivot are ALL kept (the reference's torch.where(logits < pivot, -inf, logits)).  No top_k: everything is kept.
 *   3. probs     m = the largest kept x.  Kept i: probs[i] = T(exp(x[i] - m) / sum over kept j of exp(x[j] - m)), in fp32, the exp
 *                and the summation order in cc_softmax_argmax's accuracy class; every other probs[i] is exactly 0.
 *   4. draw      h_i = mix64(mix64((seed ^ 0x53414D504C45) + p * 0x9E3779B97F4A7C15 + i)) in uint64 arithmetic, p = *input_pos and i
 *                widened from unsigned 32 bits, mix64 = the murmur3 finaliser (x ^= x >> 33; x *= 0xff51afd7ed558ccd; x ^= x >> 33;
 *                x *= 0xc4ceb9fe1a85ec53; x ^= x >> 33), applied twice as KVCacheRandom's generator does.
 *                u_i = (2 * (h_i >> 41) + 1) * 2^-24: exact in fp32, never 0 or 1.
 *   5. token     *idx_out = the kept i that maximises key_i = (x[i] - m) - log(-log(u_i)) in fp32 (the Gumbel-max rule: i wins with
 *                probability probs[i]); the smallest index wins a tie.  Both logarithms are libm-grade (<= 2 ulp), -log(u) as
 *                -log1pf(u - 1) for u > 1/2, where u - 1 is exact.  When top_k keeps one element the token is that element.
 *   6. NaN       if any x is NaN, *idx_out is the first NaN's index (cc_softmax_argmax's rule: inside the vocabulary).  Nothing else
 *                is promised then, nor for infinite x.
 * The answer does not depend on the grid or on any reduction order: the pivot is an exact radix select over the orderable bit
 * pattern of x (8 bits per launch: two launches for the 16-bit dtypes, four for fp32, none without top_k), the token an arg-min
 * over 64-bit keys (~orderable(key_i) << 32 | i), the sum a fixed-order fold of per-workgroup partials.  Never synchronises, never
 * allocates, stream-capturable; `workspace` (cc_sample_topk_workspace_bytes, 8-byte aligned) needs no initialisation.
 * temperature <= 0 or NaN, V <= 0, a null pointer: CC_ERR_BAD_ARG before any launch. */
size_t cc_sample_topk_workspace_bytes(void);
int cc_sample_topk(const void* logits, int32_t V, int32_t dtype, float temperature, int32_t top_k, uint64_t seed,
                   const int32_t* input_pos, void* probs, int32_t* idx_out, void* workspace, size_t workspace_bytes,
                   cc_stream_t stream);

/* cc_sample_topk with two more filters, top-p (nucleus) and min-p, between its step 2 and its softmax.  Steps 1 (scaling), 2 (top-k,
 * ties at the pivot all kept), 4 and 5 (uniforms, Gumbel-max key) and 6 (NaN rule) are cc_sample_topk's, word for word; so are the
 * launch properties (never synchronises, never allocates, stream-capturable, *input_pos read from device memory, one answer per
 * (logits, settings, seed, *input_pos) whatever the grid, the launch mode or the rank).  Let K be the kept set of step 2 (NaNs
 * excluded) and m the global maximum of x.  Both filters are level sets of x, so the final kept set is again {i : x[i] >= v}.
 *   2a. top-p    e_i = exp(x[i] - m) in fp32, computed exactly as step 3 computes it; the MASS of i is the integer
 *                w_i = floor(e_i * 2^40) (unsigned 64 bits; e_i <= 1), Z = sum over K of w_i, and the target is
 *                t = min(Z, ceil((double)top_p * (double)Z)), one double-precision product of the two conversions.  The nucleus is the
 *                smallest level set {i in K : x[i] >= v} whose mass is >= t; ties at v are ALL kept, as at the top-k pivot.  Integer
 *                addition is associative, so Z and every partial sum are independent of the grid, the wave order and the order of
 *                the LDS atomics that accumulate them.  V <= CC_SAMPLE_NUCLEUS_MAX_V = 2^24 - 1 keeps Z below 2^64 (each
 *                w_i <= 2^40); for V < 2^17, Z < 2^57.  A larger V with the filter on: CC_ERR_BAD_ARG.
 *                top_p >= 1: the filter is off.  top_p <= 0 or NaN: CC_ERR_BAD_ARG before any launch.
 *   2b. min-p    i survives iff fp32(x[i] - m) >= dmin (one IEEE subtraction, rounded to nearest), dmin = the fp32 rounding of the
 *                double-precision log((double)min_p), computed once on the host side of the call: p_i >= min_p * p_max in the logit
 *                domain, exact and without an exponential.  It is relative to the global maximum and independent of top-p: the kept
 *                set is the intersection of K, the nucleus and the min-p set.  min_p <= 0: off.  min_p > 1 or NaN: CC_ERR_BAD_ARG.
 *                min_p == 1 keeps exactly the elements equal to the maximum.
 *   3.  probs    as cc_sample_topk's step 3 over the final kept set (renormalised); exactly 0 elsewhere.
 * *n_kept_out (may be NULL) receives the number of kept elements: the one observable that identifies the level set (f16
 * probabilities below 2^-24 read as 0) and the nucleus size.  With both filters off, probs and token are cc_sample_topk's bit for bit
 * (the same launches run).  The nucleus pivot is a second radix select over the same orderable pattern, after the top-k select, whose
 * 256-bin histograms hold 64-bit masses: one more launch per 8-bit digit (the first also yields Z).  `workspace`
 * (cc_sample_nucleus_workspace_bytes, 8-byte aligned) needs no initialisation.  Otherwise cc_sample_topk's refusals. */
#define CC_SAMPLE_NUCLEUS_MAX_V ((1 << 24) - 1)
size_t cc_sample_nucleus_workspace_bytes(void);
int cc_sample_nucleus(const void* logits, int32_t V, int32_t dtype, float temperature, int32_t top_k, float top_p, float min_p,
                      uint64_t seed, const int32_t* input_pos, void* probs, int32_t* idx_out, int32_t* n_kept_out,
                      void* workspace, size_t workspace_bytes, cc_stream_t stream);

/* cc_sample_nucleus for T rows of logits (1 <= T <= CC_SAMPLE_MAX_ROWS) in the launches of ONE row: every kernel of the tail runs on
 * a (128, T) grid whose second index is the row.  Row r starts at logits + r * row_stride ELEMENTS (row_stride >= V; any value, any
 * alignment of a row's base: the kernels read and write element by element and bound every access by the row's own V), is drawn
 * under seeds[r] at the position input_pos[r], and writes probs + r * V (T contiguous rows), idx_out[r] and, unless it is NULL,
 * n_kept_out[r]: the bits cc_sample_nucleus writes for (logits + r * row_stride, V, dtype, temperature, top_k, top_p, min_p,
 * seeds[r], input_pos + r), whatever T and whatever the other rows hold (a NaN in one row is that row's alone).  The settings are
 * the call's, shared by the rows.  With both filters off and n_kept_out NULL the three (bf16 / f16) or five (fp32) launches of
 * cc_sample_topk run, as in cc_sample_nucleus.  `seeds` is a HOST array of T values, copied before the call returns; `input_pos`
 * is a DEVICE array of T positions, read by the kernels (a captured call advances through it).  Never synchronises, never
 * allocates, stream-capturable; `workspace` (cc_sample_rows_workspace_bytes(T), 8-byte aligned: T records of cc_sample_nucleus's)
 * needs no initialisation.  Refused before any launch: CC_ERR_BAD_ARG for T < 1, T > CC_SAMPLE_MAX_ROWS, row_stride < V, a NULL
 * logits / seeds / input_pos / probs / idx_out / workspace and everything cc_sample_nucleus refuses; CC_ERR_WORKSPACE for a
 * workspace shorter than cc_sample_rows_workspace_bytes(T) (which is 0 for a T out of range). */
#define CC_SAMPLE_MAX_ROWS 8
size_t cc_sample_rows_workspace_bytes(int32_t T);
int cc_sample_rows(const void* logits, int32_t T, int32_t V, int64_t row_stride, int32_t dtype, float temperature, int32_t top_k,
                   float top_p, float min_p, const uint64_t* seeds, const int32_t* input_pos, void* probs, int32_t* idx_out,
                   int32_t* n_kept_out, void* workspace, size_t workspace_bytes, cc_stream_t stream);

/* Per-token log-probabilities: what a perplexity evaluation reads from the logits (ref: eval.py:230-241 takes the log of a probability
 * row that generate() returned; this entry point returns the one number per token instead of the row).  logits: T rows of V elements
 * of the model dtype (`dtype`), row r at logits + r * row_stride elements, row_stride >= V — a [1, T, V] block of logits, a single row,
 * or a strided view of either.  EVERY pointer is a device pointer, targets and fallback included: nothing is read on the host, so a
 * captured step advances through them.  logprob[T] (fp32), lse[T] (fp32, may be NULL), rank[T] (int32, may be NULL).
 *   1. values    x_i = float(logits[r][i]), exact.  No temperature and no filters: the model's own distribution, whatever the sampler
 *                of the step was asked to do.
 *   2. target    t = targets[r] if targets is non-NULL and targets[r] >= 0, else fallback[r] (a captured step scores either the forced
 *                token or the token its sampler just wrote).  A t outside [0, V), or no pointer to take it from: logprob[r] = NaN and
 *                rank[r] = -1; lse[r] is still written.  No address outside the row is ever formed from t.
 *   3. lse       in fp32.  The vocabulary is cut into the launch's fixed number of slices (128, slice starts at multiples of 8
 *                elements); slice g leaves (m_g, s_g = sum of exp(x_i - m_g)) in the workspace, and ONE fold in a fixed order gives
 *                M = max m_g and S = sum of s_g * exp(m_g - M); empty slices contribute nothing.  lse = M + log S and
 *                logprob = (x_t - M) - log S.  exp and log are libm-grade (<= 2 ulp) for every dtype: the result is fp32, so the
 *                greedy tail's v_exp_f32 shortcut for 16-bit outputs does not apply.  exp(x - m) is taken as exactly 1 where x == m.
 *   4. rank      rank[r] = the number of i with x_i > x_t, exact: 0 means the target is the top logit or tied for it.  NaN elements
 *                never count; rank[r] = -1 when x_t is NaN.
 *   5. classes   the class of logprob[r] and lse[r] (finite, -inf, NaN) is that of float64 torch.log_softmax / torch.logsumexp on the
 *                same row, rounded to fp32: a NaN anywhere gives NaN for both; a +inf gives lse = +inf and logprob = NaN; a row of
 *                -inf alone gives lse = -inf and logprob = NaN; a -inf target under a finite maximum gives logprob = -inf.
 *   6. determinism  a row's three results are a pure function of that row's values and its target: bit-identical from run to run, in
 *                eager launches and under hipGraph replay, and whether the row is scored alone or as row r of T with any rows around
 *                it and at any alignment (an element's place in the summation order depends on its index alone, not on how it was
 *                loaded: 16 bytes per lane where the row's base is 16-byte aligned, element-wise otherwise).  No atomics on global
 *                memory and no tickets: per-slice partials folded in a fixed order, as cc_sample_topk's.
 * Two launches: a (128, T) grid for the partials, with the target compare counted in the same pass, and T workgroups for the fold.
 * Never synchronises, never allocates, stream-capturable; `workspace` (cc_logprob_rows_workspace_bytes, 16-byte aligned) needs no
 * initialisation.  CC_ERR_BAD_ARG before any launch: a NULL logits / logprob / workspace, T < 1, T > CC_LOGPROB_MAX_ROWS, V < 1,
 * row_stride < V, a dtype that is none of the three.  CC_ERR_WORKSPACE: a workspace shorter than cc_logprob_rows_workspace_bytes(). */
#define CC_LOGPROB_MAX_ROWS 64
size_t cc_logprob_rows_workspace_bytes(void);
int cc_logprob_rows(const void* logits, int32_t T, int32_t V, int64_t row_stride, int32_t dtype, const int32_t* targets,
                    const int32_t* fallback, float* logprob, float* lse, int32_t* rank, void* workspace, size_t workspace_bytes,
                    cc_stream_t stream);

/* The N most likely alternatives of each row next to its target's score: the OpenAI API's `top_logprobs`, vLLM's `logprobs=N`.
 * logits, T, V, row_stride, dtype, targets and fallback are cc_logprob_rows' in every respect (T <= CC_LOGPROB_MAX_ROWS, every
 * pointer a device pointer), and logprob[T], lse[T], rank[T] receive the bits cc_logprob_rows writes for the same arguments; each of
 * the three may be NULL here (a caller may want the alternatives alone).  top_ids[T * N] (int32) and top_logprobs[T * N] (fp32), row r
 * at + r * N, 1 <= N <= CC_LOGPROB_MAX_TOPN.
 *   1. order     top_ids[r * N + j], j = 0 .. N-1, are the indices of the N first elements of row r in this total order over its
 *                non-NaN elements: larger x_i = float(logits[r][i]) first, compared as floats (+0 and -0 are equal), equal values by
 *                lower index first.  NaN elements are never listed; -inf elements are ordinary candidates and come last, in index
 *                order.  The order is exact: ids carry no tolerance.
 *   2. padding   a row with fewer than N non-NaN elements (V < N included) ends in ids of -1 with log-probabilities of NaN.
 *   3. values    top_logprobs[r * N + j] = (x_id - M) - log S with the M and log S of the row's logprob (cc_logprob_rows, item 3):
 *                bit-identical to cc_logprob_rows called with that id as the row's target.  Hence the classes: a NaN anywhere in the
 *                row makes every listed value NaN while the ids stay the order's; a +inf gives NaN; a -inf candidate under a finite
 *                maximum gives -inf.
 *   4. target    when the row's target has 0 <= rank[r] < N, top_logprobs[r * N + rank[r]] has the bits of logprob[r]: position
 *                `rank` of the order is the first element of the target's tie group.
 *   5. determinism  item 6 of cc_logprob_rows, word for word, for all five results: a pure function of the row and its target, the
 *                same bits in eager launches and under hipGraph replay, alone or as row r of T, at any alignment of the row's base.
 *                No atomics on global memory and no tickets.
 * Two launches, as cc_logprob_rows: the (128, T) grid additionally leaves each slice's N first elements of the order in the
 * workspace (the whole top-N may sit in one slice), as 64-bit keys that no two elements share — round j takes the largest key below
 * round j-1's pick, so nothing is marked as taken — and the per-row fold merges the 128 lists the same way and writes the results.
 * Never synchronises, never allocates, stream-capturable; `workspace` (cc_logprob_topn_workspace_bytes, under 4 MB, 16-byte aligned)
 * needs no initialisation: nothing is read that the call did not write.  CC_ERR_BAD_ARG before any launch: a NULL logits / top_ids /
 * top_logprobs / workspace, N < 1, N > CC_LOGPROB_MAX_TOPN, and cc_logprob_rows' refusals for T, V, row_stride, dtype and alignment.
 * CC_ERR_WORKSPACE: a workspace shorter than cc_logprob_topn_workspace_bytes(); a bad argument is named before the workspace. */
#define CC_LOGPROB_MAX_TOPN 20
size_t cc_logprob_topn_workspace_bytes(void);
int cc_logprob_topn(const void* logits, int32_t T, int32_t V, int64_t row_stride, int32_t dtype, const int32_t* targets,
                    const int32_t* fallback, int32_t N, float* logprob, float* lse, int32_t* rank, int32_t* top_ids,
                    float* top_logprobs, void* workspace, size_t workspace_bytes, cc_stream_t stream);

/* Token-history penalties and a logit bias in FRONT of the sampling tail: HF / vLLM's repetition_penalty, the OpenAI API's
 * frequency_penalty / presence_penalty / logit_bias.  Unlike every other stage of the tail they depend on what has been fed so far, so
 * the history lives on the DEVICE: prompt_count[V] and gen_count[V] (int32: how often each token has been an input) and gen_start[1]
 * (int32, a position).  An input token at position p counts as GENERATED when p >= *gen_start and as PROMPT otherwise.  The same answer
 * in eager launches, under hipGraph replay (the step's input token and position are read from device memory, and the counts advance
 * in place), in blocks of T known steps and on every tensor-parallel rank (replicated logits: identical counts, no communication).
 *
 * cc_token_counts_add: tokens[n] (device int32) are the inputs at positions first_pos .. first_pos + n - 1 (first_pos: a host int);
 * each is added to the array its position selects, by integer atomicAdd — exact in any order.  A token outside [0, V) counts nothing
 * and no address is formed from it.  n == 0: CC_OK without a launch.  For the prefill (the whole prompt in one launch) and for
 * rebuilding the state after a rewind.  A NULL array / gen_start, V <= 0, n < 0, NULL tokens with n > 0: CC_ERR_BAD_ARG.
 *
 * cc_logits_penalize: logits and out are T rows of V elements of the model dtype (`dtype`), row t at + t * row_stride elements,
 * 1 <= T <= CC_GEMV_MULTI_MAX_T; out may be logits itself (in place) but must not overlap it otherwise.  tokens[T] / pos[T] (device
 * int32): the input tokens of the T steps whose rows these are and their positions; tokens NULL: count nothing (the prefill's row:
 * its prompt was added by cc_token_counts_add).  bias: float[V] or NULL.  Element v of all T rows has ONE owner:
 *     cp = prompt_count[v]; cg = gen_count[v]
 *     for t in 0 .. T-1:                                  row t sees the inputs of steps <= t
 *         if tokens and tokens[t] == v: (pos[t] >= *gen_start ? cg : cp) += 1
 *         x = float(logits[t][v])                                           exact
 *         if cp + cg > 0: x = x > 0 ? x / r : x * r       repetition (HF / vLLM: prompt and generated); one IEEE fp32 operation
 *         x = x - f * float(cg)                           frequency (OpenAI / vLLM: generated only); two roundings, no fma
 *         if cg > 0: x = x - p                            presence  (generated only)
 *         if bias: x = x + bias[v]                        -inf bans a token
 *         out[t][v] = T(x)                                ONE rounding to the model dtype
 *     prompt_count[v] = cp; gen_count[v] = cg             stored only where it changed
 * r == 1, f == 0 and p == 0 each skip their line (exactly, also for infinities); fp32 subnormals are kept; a NaN logit stays NaN; zeros
 * of both signs take the product (x > 0 is false).  A token outside [0, V) matches no v.  The bits do not depend on how an element
 * was loaded: 16 bytes at a time where the base of a row (of the counts, of bias) is 16-byte aligned, element by element where it is
 * not (rows 1 .. T-1 of an odd V).  One launch, no atomics, no workspace; plain vector stores.  Never synchronises, never allocates,
 * stream-capturable.  Before any launch — CC_ERR_BAD_ARG: T outside 1 .. CC_GEMV_MULTI_MAX_T, V <= 0, row_stride < V, a NULL logits /
 * out / prompt_count / gen_count / gen_start (or pos with tokens given), out overlapping logits without being it,
 * repetition_penalty not finite or <= 0, frequency_penalty or presence_penalty not finite; CC_ERR_UNSUPPORTED: a dtype that is none
 * of CC_DT_F32 / CC_DT_BF16 / CC_DT_F16. */
int cc_token_counts_add(int32_t* prompt_count, int32_t* gen_count, int32_t V, const int32_t* tokens, int32_t n, int32_t first_pos,
                        const int32_t* gen_start, cc_stream_t stream);
int cc_logits_penalize(const void* logits, void* out, int32_t T, int32_t V, int64_t row_stride, int32_t dtype, int32_t* prompt_count,
                       int32_t* gen_count, const int32_t* tokens, const int32_t* pos, const int32_t* gen_start,
                       float repetition_penalty, float frequency_penalty, float presence_penalty, const float* bias,
                       cc_stream_t stream);

/* Sequence rules in FRONT of the sampling tail: HF's no_repeat_ngram_size, bad_words_ids and min_new_tokens.  They need the ORDER of
 * what has been fed, so the state is positional: hist[cap] (device int32), hist[q] = the input token at position q, and gen_start[1]
 * (device int32: positions from it on are generated).  A row computed at position p predicts the token at p + 1; its history is
 * s[0 .. p].  A step at position p writes hist[p] and reads hist only in FRONT of its own position, so launches behind a failed step
 * (which write positions past it, written again in order before they are read) leave nothing to put back: no rebuild, no snapshot.
 *
 * cc_token_history_write: hist[first_pos + i] = tokens[i] (device int32 [n]; first_pos: a host int) wherever that position lies in
 * [0, cap): the prompt in one launch.  n == 0: CC_OK without a launch.  A NULL or misaligned hist / tokens (tokens with n > 0),
 * cap <= 0, n < 0: CC_ERR_BAD_ARG.
 *
 * cc_logits_constrain: logits and out are T rows of V elements of the model dtype (`dtype`), row t at + t * row_stride elements,
 * 1 <= T <= CC_GEMV_MULTI_MAX_T; out may be logits itself (in place) and must share nothing with it otherwise (the input rows are
 * then left as they were).  pos: device int32, pos[0] is read: row t is at position p = pos[0] + t.  tokens: device int32 [T], the
 * rows' input tokens, or NULL (the prefill's row: its history is in hist up to p).  Element j of the history of every row of the
 * launch is s[j] = hist[j] for j < pos[0] (for every j with tokens NULL) and tokens[j - pos[0]] otherwise, so a pattern may straddle
 * the block's start or lie inside the block.  An element that a rule bans becomes -inf of the dtype whatever it held (NaN included);
 * every other element keeps its bits; a banned id outside [0, V) bans nothing and no address is formed from it.  Row t, 0 <= p < cap:
 *   ngram = n > 0:       for i in i0 .. p - n + 1 with s[i .. i+n-2] == s[p-n+2 .. p]: ban s[i+n-1]      (n = 1: every token seen)
 *                        i0 = 0, or max(*gen_start, 0) with ngram_from_gen != 0 (n-grams wholly in the generated part)
 *   min_new_tokens = m:  while p + 1 - *gen_start < m: ban term_ids[0 .. n_term-1]
 *   banned sequences:    sequence b = bw_tokens[bw_offsets[b] .. bw_offsets[b+1] - 1] (device int32; bw_offsets [n_bw + 1], ascending
 *                        from 0; 1 .. CC_CONSTRAIN_MAX_NGRAM tokens each, CC_CONSTRAIN_MAX_BW_TOKENS in all) of length k + 1 bans its last
 *                        token when k == 0, or when k <= p + 1 and s[p-k+1 .. p] equals its first k
 * A row at a position outside [0, cap) is copied unchanged.  The launch also stores hist[pos[0] + t] = tokens[t] for the positions
 * inside [0, cap) (tokens NULL: nothing).  At most two launches on `stream`, no workspace, no atomics (threads that ban one element
 * store the same value), no waits between workgroups: a copy of the rows when out != logits (16 bytes at a time where a row's base
 * is 16-byte aligned, element by element where not), and the ban pass, whose grid covers (CC_CONSTRAIN_SLICE candidate starts i, row)
 * and is sized from cap, so a captured launch serves every later position.  Never synchronises, never allocates, capturable.
 * Before any launch, every CC_ERR_BAD_ARG before CC_ERR_UNSUPPORTED — CC_ERR_BAD_ARG: a NULL logits / out / hist / pos / gen_start,
 * T outside 1 .. CC_GEMV_MULTI_MAX_T, V <= 0, row_stride < V, cap <= 0, ngram outside 0 .. CC_CONSTRAIN_MAX_NGRAM, min_new_tokens < 0,
 * n_term outside 0 .. CC_CONSTRAIN_MAX_TERMINATORS (or NULL term_ids with n_term > 0), n_bw outside 0 .. CC_CONSTRAIN_MAX_BW (or a NULL
 * bw_tokens / bw_offsets with n_bw > 0), a misaligned pointer, out overlapping logits without being it; CC_ERR_UNSUPPORTED: a dtype
 * that is none of CC_DT_F32 / CC_DT_BF16 / CC_DT_F16. */
#define CC_CONSTRAIN_MAX_NGRAM 32
#define CC_CONSTRAIN_MAX_TERMINATORS 64
#define CC_CONSTRAIN_MAX_BW 1024
#define CC_CONSTRAIN_MAX_BW_TOKENS 4096
#define CC_CONSTRAIN_SLICE 1024
int cc_token_history_write(int32_t* hist, int32_t cap, const int32_t* tokens, int32_t n, int32_t first_pos, cc_stream_t stream);
int cc_logits_constrain(const void* logits, void* out, int32_t T, int32_t V, int64_t row_stride, int32_t dtype, int32_t* hist,
                        int32_t cap, const int32_t* tokens, const int32_t* pos, const int32_t* gen_start, int32_t ngram,
                        int32_t ngram_from_gen, int32_t min_new_tokens, const int32_t* term_ids, int32_t n_term,
                        const int32_t* bw_tokens, const int32_t* bw_offsets, int32_t n_bw, cc_stream_t stream);

/* The two logit processors for rows that belong to DIFFERENT sequences: the joint step of up to CC_GEMV_MULTI_MAX_T decode streams,
 * whose row t has its own counts, its own history, its own gen_start and its own position.  cc_logits_penalize reads its T rows as T
 * consecutive steps of ONE sequence and cc_logits_constrain takes their positions as pos[0] + t over ONE history; here the grid's
 * second index is the row and selects the row's state, as in cc_sample_rows, and a row's arithmetic does not depend on T.
 *
 * `rows` is a HOST array of T records, 1 <= T <= CC_GEMV_MULTI_MAX_T, copied into the kernel arguments by value before the call
 * returns.  The pointers INSIDE a record are device pointers, which a captured launch holds: they must live as long as the graph.
 * The settings in a record travel by value: other settings, another capture.  logits / out / T / V / row_stride / dtype are the
 * single-sequence entry points'; tokens[T] / pos[T] are device int32, read by the kernels (a captured call advances through them).
 *
 * THE CONTRACT of both: row t of a T-row call carries exactly the bits, in `out` and in the state, that the single-sequence entry
 * point writes when it is called with T = 1 for that row (logits + t * row_stride, tokens + t, pos + t) on rows[t]'s state.
 *
 * cc_logits_penalize_streams: row t is penalised against rows[t] alone by the per-element formula above (same operations, same
 * rounding points, fp32 first and then one rounding to the dtype).  tokens[t] at pos[t] is counted into rows[t]'s tables before the
 * row is computed — generated when pos[t] >= *rows[t].gen_start — and the count is stored only where it changed.  tokens NULL: nothing
 * is counted (the prefill's row).  A record whose prompt_count is NULL means no penalties for that row: it is copied bit for bit
 * (out != logits) or left alone (in place), and the record's other fields are not looked at.  One launch on a (groups of 16 bytes, T)
 * grid: an element of a row has one owner; no atomics, no workspace, plain vector stores; 16-byte loads where the base of a row, of a
 * count table or of a bias is 16-byte aligned, element by element where it is not.  Refused before any launch: everything
 * cc_logits_penalize refuses, per record, a NULL rows, and — CC_ERR_BAD_ARG — two records that name one table (prompt_count or
 * gen_count, in either role): two rows would race on it.
 *
 * cc_logits_constrain_streams: row t sits at its OWN position p = pos[t]; its history is rows[t].hist[0 .. p-1] followed by tokens[t]
 * (tokens NULL: hist[0 .. p]), and the bans are cc_logits_constrain's: -inf of the dtype, every other element keeps its bits, an id
 * outside [0, V) bans nothing, a position outside [0, cap) leaves the row as it is and stores nothing.  The launch stores
 * hist[pos[t]] = tokens[t] for each row; no workgroup reads that position back from hist: it is taken from tokens.  A record whose
 * hist is NULL passes its row through.  A copy of the rows when out != logits, then one launch on a (max over rows of the slice
 * count + 1, T) grid; no workgroup waits for another.  Refused before any launch: everything cc_logits_constrain refuses, per
 * record, a NULL rows, and two records that share one hist. */
typedef struct cc_penalty_row_t {
  int32_t* prompt_count;    /* NULL: no penalties for this row */
  int32_t* gen_count;
  const int32_t* gen_start;
  const float* bias;        /* float[V] or NULL */
  float r, f, p;            /* repetition_penalty, frequency_penalty, presence_penalty */
} cc_penalty_row_t;
typedef struct cc_constraint_row_t {
  int32_t* hist;            /* NULL: no rules for this row */
  int32_t cap;
  const int32_t* gen_start;
  int32_t ngram, ngram_from_gen, min_new_tokens;
  const int32_t* term_ids;
  int32_t n_term;
  const int32_t* bw_tokens;
  const int32_t* bw_offsets;
  int32_t n_bw;
} cc_constraint_row_t;
int cc_logits_penalize_streams(const void* logits, void* out, int32_t T, int32_t V, int64_t row_stride, int32_t dtype,
                               const cc_penalty_row_t* rows, const int32_t* tokens, const int32_t* pos, cc_stream_t stream);
int cc_logits_constrain_streams(const void* logits, void* out, int32_t T, int32_t V, int64_t row_stride, int32_t dtype,
                                const cc_constraint_row_t* rows, const int32_t* tokens, const int32_t* pos, cc_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * One-shot sum all-reduce over the GPUs of ONE node, for the decode-size messages of tensor parallelism.
 * ref: tp.py:134-138, 156-160 (`all_reduce(sum)` of the wo and FFN outputs: 2 * dim bytes, 8-16 KiB, twice per layer).
 * Every rank stores its vector straight into a slot of every peer's buffer over the xGMI mesh, raises a flag, waits for the
 * flags raised for it, and adds the `world` slots in RANK ORDER (fp32 accumulate, one rounding): one launch of one workgroup,
 * no ring hops, capturable in a hipGraph, bitwise-identical results on every rank.  RCCL (torch.distributed "nccl") remains
 * the general collective and the oracle this is tested against (tests/test_gpu_tp.py).
 *   cc_allreduce_create   allocates this rank's symmetric buffer (uncached fine-grained device memory; the ONE allocating,
 *                         synchronising entry point of this ABI: call it at start-up, not on the decode path);
 *   cc_allreduce_export   copies the buffer's hipIpcMemHandle_t (cc_allreduce_handle_bytes() bytes) into HOST memory;
 *   cc_allreduce_connect  takes the world's handles in rank order (HOST memory; the host exchanges them, e.g. with
 *                         torch.distributed.all_gather) and maps the peers' buffers;
 *   cc_allreduce_sum      in place on `data` (device, 16-byte aligned, n elements of `dtype`, n * size <= max_bytes); every
 *                         rank must call it in the same order on its stream; never synchronises;
 *   cc_allreduce_status   0, or 1 if an all-reduce gave up waiting for a peer (bounded polling) — synchronising read.
 * ---------------------------------------------------------------------------------------------- */
typedef struct cc_comm cc_comm;
size_t cc_allreduce_handle_bytes(void);
int cc_allreduce_create(int32_t rank, int32_t world, size_t max_bytes, cc_comm** out);
int cc_allreduce_export(cc_comm* comm, void* handle_out);
int cc_allreduce_connect(cc_comm* comm, const void* handles);
int cc_allreduce_sum(cc_comm* comm, void* data, int64_t n, int32_t dtype, cc_stream_t stream);
int32_t cc_allreduce_status(cc_comm* comm);
int cc_allreduce_destroy(cc_comm* comm);

#ifdef __cplusplus
}
#endif
#endif /* COLDCOMPRESS_H */
